// ppgat_fullrank.hip -- full-catalogue ranking for evaluation: every evaluated (user, positive)
// pair ranked against every item outside the user's train history, in one fused pass.
//
//   s(i) = <U[u], I[i]>;  rank = 1 + #{ i not in X : s(i) > s(p) },  ties = #{ i not in X : s(i) == s(p) }
//   X = history(u) + {p}, excluded by index (never by score)
//
// The [n_eval, n_items] score matrix is a matrix-core product with a compare-and-count epilogue
// and is never written.  The product is the score-tile engine of ppgat_score_tile.h (geometry,
// user fragments, tile staging, history cursor, A-fragment read), which k_full_topk and k_shs use
// too: a block owns TM evaluated entries, walks the item table in ascending TN-item tiles (the
// next tile's loads in flight during the current tile's MFMAs, one barrier per tile) and takes
// the product transposed -- items on the accumulator's rows, the user on the lane's column -- so
// a lane compares its 16 accumulator values with ONE s(p) and counts into ONE pair of registers.
// What is this file's own is the tile loop: a flat (subtile, k step) sequence, each step's
// fragments read one step ahead of its MFMAs, with the counting epilogue.
//
// Exclusion: the mask words of score::mask_words (history items, columns past the item range)
// with the positive's bit ORed in, one 32-bit word per entry and 32-item subtile in LDS.  The
// epilogue tests the lane's bit; a subtile with no bit set in the wave skips the test.
//
// s(p) is formed by the same six-term MFMA chain as the tile scores (a 32x32 product of the
// wave's users with their own positives' rows, the diagonal kept), so an item whose row equals
// the positive's row gives a bitwise equal score: ties are exact.
//
// A launch too small to fill the chip splits the item range over blockIdx.y; partial counts are
// combined with integer adds (exact and order-independent), rank starting from the 1 that the
// first split adds.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ppgat_internal.h"
#include "ppgat_device.h"
#include "ppgat_score_tile.h"

namespace ppgat {
namespace {

using split::f32x16;
using split::mfma32_x6;
using split::u32x4;

// 8 waves (C = 256: 4, the user fragments take 192 VGPRs, one wave per SIMD); 128, 128, 64, 32 items per tile
template <int C>
using FrGeo = score::Geo<C, (C == 256 ? 4 : 8), (C >= 64 ? 8192 / C : 128)>;
template <int C>
struct FrCfg : FrGeo<C> {
  static constexpr size_t LDS = 2 * (size_t)FrGeo<C>::BUF + 2 * (size_t)FrGeo<C>::TM * FrGeo<C>::SUB * 4;  // + masks
};

struct FrArg {
  const float* U;
  int64_t ldu, n_users;
  const float* I;
  int64_t ldi, n_items;
  const int64_t* users;
  const int64_t* pos;
  int64_t n_eval;
  const int64_t* uptr;
  const int32_t* hist;
  int32_t* rank;
  int32_t* ties;
  int64_t tiles_per_split;
};

template <int C>
__global__ void __launch_bounds__(FrCfg<C>::NT, 1) k_full_rank(FrArg a) {
  using F = FrCfg<C>;
  extern __shared__ __attribute__((aligned(16))) unsigned char fr_lds[];
  uint32_t* sMask = reinterpret_cast<uint32_t*>(fr_lds + 2 * F::BUF);  // [2][TM][SUB]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hf = lane >> 5;
  const int64_t n_items = a.n_items, ldi = a.ldi;
  const int64_t ntiles = (n_items + F::TN - 1) / F::TN;
  const int64_t t0 = (int64_t)blockIdx.y * a.tiles_per_split;  // t0 < ntiles (launcher)
  const int64_t t1 = t0 + a.tiles_per_split < ntiles ? t0 + a.tiles_per_split : ntiles;
  const int64_t jlo = t0 * F::TN;
  const int64_t jhi = t1 * F::TN < n_items ? t1 * F::TN : n_items;

  // ---- this lane's entry: user column r of the wave's 32; rows past n_eval repeat the last ----
  const int64_t b = (int64_t)blockIdx.x * F::TM + wave * 32 + r;
  const int64_t bc = b < a.n_eval ? b : a.n_eval - 1;
  const int64_t u = clamp_idx(a.users[bc], a.n_users);
  const int64_t p = clamp_idx(a.pos[bc], n_items);
  u32x4 ub[F::KS][3];
  score::load_owned<F>(a.U + u * a.ldu, hf, ub);
  // ---- s(p): the users against their own positives' rows, the diagonal of the 32x32 product.
  // score::diag_score (k_shs's s0) written out: called as a function it compiles here to another
  // packing of the positives' split, and k_full_rank<128> then measured 0.6-0.9 % slower ----
  float sp;
  {
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    const float* pp = a.I + p * ldi + 8 * hf;
#pragma unroll
    for (int ks = 0; ks < F::KS; ++ks) {
      u32x4 ia[3];
      split::split3(ld4(pp + 16 * ks), ld4(pp + 16 * ks + 4), ia[0], ia[1], ia[2]);
      acc = mfma32_x6(ia, ub[ks], acc);
    }
    const int qsel = (r & 3) + 4 * (r >> 3);
    float v = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) v = q == qsel ? acc[q] : v;
    const float vo = __shfl_xor(v, 32);
    sp = hf == ((r >> 2) & 1) ? v : vo;
  }

  // ---- the exclusion cursor of entry tid (threads 0 .. TM-1) ----
  score::HistCursor cursor;
  int64_t pt = -1;
  {
    const int64_t be = (int64_t)blockIdx.x * F::TM + tid;
    if (tid < F::TM && be < a.n_eval) {
      pt = clamp_idx(a.pos[be], n_items);
      if (a.uptr) cursor.seek(a.uptr, a.hist, clamp_idx(a.users[be], a.n_users), jlo);
    }
  }
  cursor.start(a.hist);
  auto build_mask = [&](int64_t t, int bufi) {
    if (tid < F::TM) {
      const int64_t j0 = t * F::TN;
      uint32_t* w = sMask + ((size_t)bufi * F::TM + tid) * F::SUB;
      score::mask_words<F>(w, j0, jhi, cursor, a.hist);
      const int64_t d = pt - j0;  // the positive's bit
      if (d >= 0 && d < F::TN) w[d >> 5] |= 1u << (int)(d & 31);
    }
  };

  float4 pf[F::UPT][2];
  auto load_tile = [&](int64_t t) {
    score::tile_load<F>(pf, t, n_items, tid, [&](int64_t j) { return a.I + j * ldi; });
  };
  auto store_tile = [&](int bufi) { score::tile_store<F>(fr_lds + bufi * F::BUF, pf, tid); };

  load_tile(t0);
  store_tile(0);
  build_mask(t0, 0);
  __syncthreads();

  int gt = 0, eq = 0;
  const int xoff = F::xoff(r, hf);
  for (int64_t t = t0; t < t1; ++t) {
    const int bufi = (int)((t - t0) & 1);
    if (t + 1 < t1) load_tile(t + 1);
    // SUB x KS (subtile, k step) steps; the next step's three A units are read from LDS while the
    // current step's six MFMAs run (the scheduling barrier keeps each read one step ahead)
    const unsigned char* tile_r = fr_lds + bufi * F::BUF + r * F::ROWB;
    u32x4 fa[3];
    score::read_a<F>(tile_r, 0, xoff, fa);
    f32x16 acc;
#pragma unroll
    for (int idx = 0; idx < F::SUB * F::KS; ++idx) {
      const int sb = idx / F::KS, ks = idx % F::KS;
      if (ks == 0) {
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.f;
      }
      u32x4 fn[3];
      if (idx + 1 < F::SUB * F::KS) score::read_a<F>(tile_r, idx + 1, xoff, fn);
      acc = mfma32_x6(fa, ub[ks], acc);
      __builtin_amdgcn_sched_barrier(0);
      if (idx + 1 < F::SUB * F::KS) {
        fa[0] = fn[0];
        fa[1] = fn[1];
        fa[2] = fn[2];
      }
      if (ks != F::KS - 1) continue;
      const uint32_t m = sMask[((size_t)bufi * F::TM + wave * 32 + r) * F::SUB + sb] >> (4 * hf);
      if (__builtin_amdgcn_ballot_w64(m != 0u) == 0) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          gt += acc[q] > sp ? 1 : 0;
          eq += acc[q] == sp ? 1 : 0;
        }
      } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const bool in = ((m >> score::acc_row(q)) & 1u) == 0u;
          gt += (in && acc[q] > sp) ? 1 : 0;
          eq += (in && acc[q] == sp) ? 1 : 0;
        }
      }
    }
    if (t + 1 < t1) {
      store_tile(bufi ^ 1);
      build_mask(t + 1, bufi ^ 1);
    }
    __syncthreads();
  }
  gt += __shfl_xor(gt, 32);
  eq += __shfl_xor(eq, 32);
  if (hf == 0 && b < a.n_eval) {
    atomicAdd(a.rank + b, gt + (blockIdx.y == 0 ? 1 : 0));
    if (a.ties) atomicAdd(a.ties + b, eq);
  }
}

template <int C>
hipError_t launch_full_rank(FrArg a, int ncu, hipStream_t st) {
  using F = FrCfg<C>;
  const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_full_rank<C>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)F::LDS);
  if (attr != hipSuccess) return attr;
  const int64_t utiles = (a.n_eval + F::TM - 1) / F::TM;
  // too few entry tiles to fill the chip: the item range is split
  const score::ItemSplit sp = score::split_items(utiles, (a.n_items + F::TN - 1) / F::TN, ncu);
  a.tiles_per_split = sp.tiles_per_split;
  if (utiles > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_full_rank<C>, dim3((unsigned)utiles, (unsigned)sp.nsplit), dim3(F::NT), F::LDS, st, a);
  return hipGetLastError();
}

}  // namespace

bool full_rank_channels_ok(int C) { return C == 32 || C == 64 || C == 128 || C == 256; }

hipError_t full_rank(const float* U, int64_t ldu, int64_t n_users, const float* I, int64_t ldi, int64_t n_items, int C,
                     const int64_t* users, const int64_t* pos, int64_t n_eval, const int64_t* uptr,
                     const int32_t* hist, int32_t* rank, int32_t* ties, hipStream_t st) {
  if (n_eval == 0) return hipSuccess;
  int ncu = 0;
  hipError_t e = score::cu_count(&ncu);
  if (e != hipSuccess) return e;
  // the counts are added: rank starts from 0 and the first item split adds the 1
  e = hipMemsetAsync(rank, 0, (size_t)n_eval * sizeof(int32_t), st);
  if (e != hipSuccess) return e;
  if (ties) {
    e = hipMemsetAsync(ties, 0, (size_t)n_eval * sizeof(int32_t), st);
    if (e != hipSuccess) return e;
  }
  FrArg a{U, ldu, n_users, I, ldi, n_items, users, pos, n_eval, uptr, hist, rank, ties, 0};
  switch (C) {
    case 32: return launch_full_rank<32>(a, ncu, st);
    case 64: return launch_full_rank<64>(a, ncu, st);
    case 128: return launch_full_rank<128>(a, ncu, st);
    case 256: return launch_full_rank<256>(a, ncu, st);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace ppgat
