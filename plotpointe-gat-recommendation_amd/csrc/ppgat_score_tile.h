// ppgat_score_tile.h -- the pieces of the matrix-core score-tile engine that k_full_rank
// (ppgat_fullrank.hip), k_full_topk (ppgat_fulltopk.hip) and k_shs (ppgat_shs.hip) have in common.
//
// The engine: a block owns TM rows (32 per wave) and keeps them as split bf16 B fragments in
// registers for the whole kernel; the other table is streamed in tiles of TN rows, each loaded
// once per block as fp32, cut once into the three bf16 terms of ppgat_split.h and staged in LDS
// (double buffered, XOR swizzled), where every wave reads it as the A operand of
// v_mfma_f32_32x32x16_bf16.  The product is taken transposed: the streamed row sits on the
// accumulator's row, the owned row on the lane's column.
//
// Shared here: the tile geometry and its bank swizzle, the accumulator-row map, the owned rows'
// fragment load, the diagonal score of the owned rows against one partner row each, the sorted
// history cursor with the per-tile mask words, the tile's load / split / store, the A-fragment
// read, and the host's item-range split plan.  One definition each, so the three kernels cannot
// drift apart: the rank / top-K score identity is bitwise and is tested.
//
// NOT shared: the tile loops and their epilogues (compare-and-count, thresholds and compaction,
// the softmax sweeps with their second product).  Every piece here is __forceinline__ and leaves
// the caller's loop, and with it the caller's registers and schedule, where it was; one main loop
// templated over an epilogue policy would put k_full_rank<256>, which stands at 256 VGPRs, at the
// mercy of the largest epilogue.
//
// No floating-point multiply-add chain may be written in this header: ppgat_shs.hip includes it
// BEFORE its `#pragma clang fp contract(off)` (where ppgat_split.h stands), and the code here must
// round the same on either side of that pragma.  For the same reason it does not include
// ppgat_device.h, which that file includes after the pragma.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ppgat_split.h"

namespace ppgat {
namespace score {

using split::f32x16;
using split::mfma32_x6;
using split::split3;
using split::u32x4;

// accumulator register q of lane (r, hf) holds streamed row acc_row(q) + 4 hf of the 32-row
// subtile, for owned column r
__host__ __device__ constexpr int acc_row(int q) { return (q & 3) + 8 * (q >> 2); }

template <int C, int WAVES_, int TN_>
struct Geo {
  static constexpr int WAVES = WAVES_;
  static constexpr int NT = 64 * WAVES;      // threads
  static constexpr int TM = 32 * WAVES;      // owned rows per block
  static constexpr int TN = TN_;             // streamed rows per tile
  static constexpr int SUB = TN / 32;        // 32-row subtiles (mask words per owned row)
  static constexpr int CPR = C / 8;          // 16-byte (8 x bf16) units per row
  static constexpr int UPT = TN * CPR / NT;  // units staged per thread
  static constexpr int ROWB = 2 * C;         // bytes per staged row
  static constexpr int PART = TN * ROWB;     // bytes per split term
  static constexpr int BUF = 3 * PART;       // one staged tile
  static constexpr int KS = C / 16;          // k steps of the 32x32x16 MFMA
  static_assert(TN % 32 == 0 && UPT * NT == TN * CPR, "score tile: staging covers the tile");
  // ds_read_b128 is banked by 16-byte slot of a 256-byte line, in 16-lane groups whose rows are
  // distinct mod 16: XOR the unit index with the row's position among the 16 rows (rows of 256
  // bytes or more), or among the lines when several rows share one (C = 64: 2, C = 32: 4)
  __host__ __device__ static constexpr int swz(int row) {
    return CPR >= 16 ? (row & 15) : ((row / (16 / CPR)) & (CPR - 1));
  }
  // lane (r, hf) reads unit 2 ks + hf of its row, swizzled: ((2 ks) ^ hf ^ swz) << 4 = (32 ks) ^ xoff
  // (swz(32 sb + r) = swz(r): one xoff serves every subtile)
  __host__ __device__ static constexpr int xoff(int r, int hf) { return (hf ^ swz(r)) << 4; }
};

// ---- the owned row's split fragments, the B operand of all KS k steps (lane half hf) ----
template <class F>
__device__ __forceinline__ void load_owned(const float* row, int hf, u32x4 (&ub)[F::KS][3]) {
  const float4* up = reinterpret_cast<const float4*>(row + 8 * hf);
#pragma unroll
  for (int ks = 0; ks < F::KS; ++ks) split3(up[4 * ks], up[4 * ks + 1], ub[ks][0], ub[ks][1], ub[ks][2]);
}

// ---- <owned row of lane column r, partner row `prow` of the same lane>: the wave's 32 owned rows
// against their 32 partners as one 32x32 product, by the six-term chain of the tile scores, the
// diagonal kept (so a streamed row equal to the partner's gives a bitwise equal score).  k_shs's
// s0; k_full_rank writes the same lines out for its s(p), see there ----
template <class F>
__device__ __forceinline__ float diag_score(const float* prow, const u32x4 (&ub)[F::KS][3], int r, int hf) {
  f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.f;
  const float4* pp = reinterpret_cast<const float4*>(prow + 8 * hf);
#pragma unroll
  for (int ks = 0; ks < F::KS; ++ks) {
    u32x4 ia[3];
    split3(pp[4 * ks], pp[4 * ks + 1], ia[0], ia[1], ia[2]);
    acc = mfma32_x6(ia, ub[ks], acc);
  }
  // row r of column r is acc_row(qsel) + 4 hf with hf = (r >> 2) & 1: in this lane or its partner
  const int qsel = (r & 3) + 4 * (r >> 3);
  float v = 0.f;
#pragma unroll
  for (int q = 0; q < 16; ++q) v = q == qsel ? acc[q] : v;
  const float vo = __shfl_xor(v, 32);
  return hf == ((r >> 2) & 1) ? v : vo;
}

// ---- exclusion by index: streamed items ascend and each history is sorted, so one thread per
// owned row keeps a cursor into the history and sets, tile by tile, the bits of its items ----
constexpr int64_t kNoItem = INT64_MAX;

struct HistCursor {
  int64_t cur = 0, cend = 0, nxt = 0;  // [cur, cend) of the history still ahead; nxt = its first item

  // the history of `user`, from its first item >= jlo (a block that starts mid-table)
  __device__ __forceinline__ void seek(const int64_t* uptr, const int32_t* hist, int64_t user, int64_t jlo) {
    cur = uptr[user];
    cend = uptr[user + 1];
    if (jlo > 0) {
      int64_t lo = cur, hi = cend;
      while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (hist[mid] < jlo) lo = mid + 1; else hi = mid;
      }
      cur = lo;
    }
  }
  // after seek, or on a cursor left empty (no history, no entry): every thread calls it once
  __device__ __forceinline__ void start(const int32_t* hist) { nxt = cur < cend ? (int64_t)hist[cur] : kNoItem; }
};

// the SUB mask words of one owned row for the tile of items [j0, j0 + TN): the columns at or past
// jhi (outside the item range; jhi > j0) and the history items, the cursor moving past them
template <class F>
__device__ __forceinline__ void mask_words(uint32_t* w, int64_t j0, int64_t jhi, HistCursor& c, const int32_t* hist) {
  const int64_t jend = j0 + F::TN, valid = jhi - j0;
#pragma unroll
  for (int s = 0; s < F::SUB; ++s) {
    const int64_t v = valid - 32 * s;
    w[s] = v >= 32 ? 0u : (v <= 0 ? 0xffffffffu : (0xffffffffu << (int)v));
  }
  while (c.nxt < jend) {
    const int64_t d = c.nxt - j0;
    if (d >= 0) w[d >> 5] |= 1u << (int)(d & 31);
    ++c.cur;
    c.nxt = c.cur < c.cend ? (int64_t)hist[c.cur] : kNoItem;
  }
}

// ---- tile t of the streamed table: this thread's UPT units, fp32, into registers.  row(j) is
// streamed row j's address; rows past n_rows repeat the last ----
template <class F, class RowFn>
__device__ __forceinline__ void tile_load(float4 (&pf)[F::UPT][2], int64_t t, int64_t n_rows, int tid, RowFn row) {
#pragma unroll
  for (int k = 0; k < F::UPT; ++k) {
    const int e = tid + k * F::NT, rw = e / F::CPR, ch = e % F::CPR;
    int64_t j = t * F::TN + rw;
    j = j < n_rows ? j : n_rows - 1;
    const float4* src = reinterpret_cast<const float4*>(row(j) + 8 * ch);
    pf[k][0] = src[0];
    pf[k][1] = src[1];
  }
}

// ---- the loaded units cut into the three terms and staged in the LDS tile `buf`, swizzled ----
template <class F>
__device__ __forceinline__ void tile_store(unsigned char* buf, const float4 (&pf)[F::UPT][2], int tid) {
#pragma unroll
  for (int k = 0; k < F::UPT; ++k) {
    const int e = tid + k * F::NT, rw = e / F::CPR, ch = e % F::CPR;
    u32x4 h, m, l;
    split3(pf[k][0], pf[k][1], h, m, l);
    unsigned char* dst = buf + rw * F::ROWB + ((ch ^ F::swz(rw)) << 4);
    *reinterpret_cast<u32x4*>(dst) = h;
    *reinterpret_cast<u32x4*>(dst + F::PART) = m;
    *reinterpret_cast<u32x4*>(dst + 2 * F::PART) = l;
  }
}

// ---- the three A terms of (subtile, k step) idx = sb KS + ks for the lane whose row r starts at
// tile_r = tile + r ROWB, xoff = F::xoff(r, hf) ----
template <class F>
__device__ __forceinline__ void read_a(const unsigned char* tile_r, int idx, int xoff, u32x4 (&f)[3]) {
  const unsigned char* pa = tile_r + (idx / F::KS) * 32 * F::ROWB + ((32 * (idx % F::KS)) ^ xoff);
  f[0] = *reinterpret_cast<const u32x4*>(pa);
  f[1] = *reinterpret_cast<const u32x4*>(pa + F::PART);
  f[2] = *reinterpret_cast<const u32x4*>(pa + 2 * F::PART);
}

// ---- host: how the catalogue walks cut the item range.  A launch with fewer owned tiles than
// CUs splits its `ntiles` item tiles over blockIdx.y ----
struct ItemSplit {
  int64_t nsplit, tiles_per_split;
};
inline ItemSplit split_items(int64_t utiles, int64_t ntiles, int ncu) {
  int64_t nsplit = 1;
  if (utiles > 0 && utiles < ncu) {
    nsplit = (ncu + utiles - 1) / utiles;
    if (nsplit > ntiles) nsplit = ntiles;
  }
  const int64_t per = (ntiles + nsplit - 1) / nsplit;
  return {(ntiles + per - 1) / per, per};  // every split non-empty
}

inline hipError_t cu_count(int* ncu) {
  int dev = 0;
  const hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  return hipDeviceGetAttribute(ncu, hipDeviceAttributeMultiprocessorCount, dev);
}

}  // namespace score
}  // namespace ppgat
