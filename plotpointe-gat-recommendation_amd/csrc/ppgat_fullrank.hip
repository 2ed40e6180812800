// ppgat_fullrank.hip -- full-catalogue ranking for evaluation: every evaluated (user, positive)
// pair ranked against every item outside the user's train history, in one fused pass.
//
//   s(i) = <U[u], I[i]>;  rank = 1 + #{ i not in X : s(i) > s(p) },  ties = #{ i not in X : s(i) == s(p) }
//   X = history(u) + {p}, excluded by index (never by score)
//
// The [n_eval, n_items] score matrix is a matrix-core product with a compare-and-count epilogue
// and is never written: a block owns TM evaluated entries (32 per wave), keeps their user rows
// as split bf16 B fragments in registers for the whole kernel, and walks the item table in
// ascending TN-item tiles.  Each tile is loaded once per block (fp32, the next tile's loads in
// flight during the current tile's MFMAs), cut into the three bf16 terms of ppgat_split.h once,
// and staged in LDS (double buffered, one barrier per tile), where every wave reads it as the A
// operand of v_mfma_f32_32x32x16_bf16, each k step's fragments read one step ahead of its MFMAs.  The product is taken transposed -- items on the
// accumulator's rows, the user on the lane's column -- so a lane compares its 16 accumulator
// values with ONE s(p) and counts into ONE pair of registers.
//
// Exclusion: items ascend and each history is sorted, so one thread per entry keeps a cursor into
// items_sorted and, per tile, sets the bits of the history items, of the positive and of the
// columns past the item range in an LDS mask (one 32-bit word per entry and 32-item subtile).
// The epilogue tests the lane's bit; a subtile with no bit set in the wave skips the test.
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
#include "ppgat_split.h"

namespace ppgat {
namespace {

using split::f32x16;
using split::mfma32_x6;
using split::split3;
using split::u32x4;

__device__ __forceinline__ float4 fr_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ int64_t fr_clamp(int64_t v, int64_t n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

template <int C>
struct FrCfg {
  static constexpr int WAVES = C == 256 ? 4 : 8;       // C = 256: 192 VGPRs of user fragments, one wave per SIMD
  static constexpr int NT = 64 * WAVES;                // threads
  static constexpr int TM = 32 * WAVES;                // evaluated entries per block
  static constexpr int TN = C >= 64 ? 8192 / C : 128;  // items per tile: 128, 128, 64, 32
  static constexpr int SUB = TN / 32;                  // 32-item subtiles (mask words per entry)
  static constexpr int CPR = C / 8;                    // 16-byte (8 x bf16) units per row
  static constexpr int UPT = TN * CPR / NT;            // units staged per thread: 1, 2, 2, 4
  static constexpr int ROWB = 2 * C;                   // bytes per staged row
  static constexpr int PART = TN * ROWB;               // bytes per split term
  static constexpr int BUF = 3 * PART;                 // one staged tile
  static constexpr int KS = C / 16;                    // k steps of the 32x32x16 MFMA
  static constexpr size_t LDS = 2 * (size_t)BUF + 2 * (size_t)TM * SUB * 4;
  // ds_read_b128 is banked by 16-byte slot of a 256-byte line, in 16-lane groups whose rows are
  // distinct mod 16: XOR the unit index with the row's position among the 16 rows (rows of 256
  // bytes or more), or among the lines when several rows share one (C = 64: 2, C = 32: 4)
  __host__ __device__ static constexpr int swz(int row) {
    return CPR >= 16 ? (row & 15) : ((row / (16 / CPR)) & (CPR - 1));
  }
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

constexpr int64_t kNoItem = INT64_MAX;

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
  const int64_t u = fr_clamp(a.users[bc], a.n_users);
  const int64_t p = fr_clamp(a.pos[bc], n_items);
  u32x4 ub[F::KS][3];
  {
    const float* up = a.U + u * a.ldu + 8 * hf;
#pragma unroll
    for (int ks = 0; ks < F::KS; ++ks) split3(fr_ld4(up + 16 * ks), fr_ld4(up + 16 * ks + 4), ub[ks][0], ub[ks][1], ub[ks][2]);
  }
  // ---- s(p): the users against their own positives' rows, the diagonal of the 32x32 product ----
  float sp;
  {
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    const float* pp = a.I + p * ldi + 8 * hf;
#pragma unroll
    for (int ks = 0; ks < F::KS; ++ks) {
      u32x4 ia[3];
      split3(fr_ld4(pp + 16 * ks), fr_ld4(pp + 16 * ks + 4), ia[0], ia[1], ia[2]);
      acc = mfma32_x6(ia, ub[ks], acc);
    }
    // accumulator q of lane (r, hf) is item row (q & 3) + 8 (q >> 2) + 4 hf of user column r
    const int qsel = (r & 3) + 4 * (r >> 3);
    float v = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) v = q == qsel ? acc[q] : v;
    const float vo = __shfl_xor(v, 32);
    sp = hf == ((r >> 2) & 1) ? v : vo;
  }

  // ---- the exclusion cursor of entry tid (threads 0 .. TM-1) ----
  int64_t cur = 0, cend = 0, pt = -1;
  {
    const int64_t be = (int64_t)blockIdx.x * F::TM + tid;
    if (tid < F::TM && be < a.n_eval) {
      pt = fr_clamp(a.pos[be], n_items);
      if (a.uptr) {
        const int64_t ue = fr_clamp(a.users[be], a.n_users);
        cur = a.uptr[ue];
        cend = a.uptr[ue + 1];
        if (jlo > 0) {  // first history item >= jlo
          int64_t lo = cur, hi = cend;
          while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (a.hist[mid] < jlo) lo = mid + 1; else hi = mid;
          }
          cur = lo;
        }
      }
    }
  }
  int64_t nxt = cur < cend ? (int64_t)a.hist[cur] : kNoItem;

  auto build_mask = [&](int64_t t, int bufi) {
    if (tid < F::TM) {
      const int64_t j0 = t * F::TN, jend = j0 + F::TN;
      uint32_t* w = sMask + ((size_t)bufi * F::TM + tid) * F::SUB;
      const int64_t valid = jhi - j0;  // >= 1; columns past it are outside the item range
#pragma unroll
      for (int s = 0; s < F::SUB; ++s) {
        const int64_t v = valid - 32 * s;
        w[s] = v >= 32 ? 0u : (v <= 0 ? 0xffffffffu : (0xffffffffu << (int)v));
      }
      while (nxt < jend) {
        const int64_t d = nxt - j0;
        if (d >= 0) w[d >> 5] |= 1u << (int)(d & 31);
        ++cur;
        nxt = cur < cend ? (int64_t)a.hist[cur] : kNoItem;
      }
      const int64_t d = pt - j0;
      if (d >= 0 && d < F::TN) w[d >> 5] |= 1u << (int)(d & 31);
    }
  };

  float4 pf[F::UPT][2];
  auto load_tile = [&](int64_t t) {
#pragma unroll
    for (int k = 0; k < F::UPT; ++k) {
      const int e = tid + k * F::NT, row = e / F::CPR, ch = e % F::CPR;
      int64_t j = t * F::TN + row;
      j = j < n_items ? j : n_items - 1;
      const float* src = a.I + j * ldi + 8 * ch;
      pf[k][0] = fr_ld4(src);
      pf[k][1] = fr_ld4(src + 4);
    }
  };
  auto store_tile = [&](int bufi) {
#pragma unroll
    for (int k = 0; k < F::UPT; ++k) {
      const int e = tid + k * F::NT, row = e / F::CPR, ch = e % F::CPR;
      u32x4 h, m, l;
      split3(pf[k][0], pf[k][1], h, m, l);
      unsigned char* dst = fr_lds + bufi * F::BUF + row * F::ROWB + ((ch ^ F::swz(row)) << 4);
      *reinterpret_cast<u32x4*>(dst) = h;
      *reinterpret_cast<u32x4*>(dst + F::PART) = m;
      *reinterpret_cast<u32x4*>(dst + 2 * F::PART) = l;
    }
  };

  load_tile(t0);
  store_tile(0);
  build_mask(t0, 0);
  __syncthreads();

  int gt = 0, eq = 0;
  // unit 2 ks + hf of row r, swizzled: ((2 ks) ^ hf ^ swz) << 4 = (32 ks) ^ xoff
  const int xoff = (hf ^ F::swz(r)) << 4;
  for (int64_t t = t0; t < t1; ++t) {
    const int bufi = (int)((t - t0) & 1);
    if (t + 1 < t1) load_tile(t + 1);
    // SUB x KS (subtile, k step) steps; the next step's three A units are read from LDS while the
    // current step's six MFMAs run (the scheduling barrier keeps each read one step ahead)
    const unsigned char* tile = fr_lds + bufi * F::BUF + r * F::ROWB;
    auto read_a = [&](int idx, u32x4 (&f)[3]) {
      const unsigned char* pa = tile + (idx / F::KS) * 32 * F::ROWB + ((32 * (idx % F::KS)) ^ xoff);
      f[0] = *reinterpret_cast<const u32x4*>(pa);
      f[1] = *reinterpret_cast<const u32x4*>(pa + F::PART);
      f[2] = *reinterpret_cast<const u32x4*>(pa + 2 * F::PART);
    };
    u32x4 fa[3];
    read_a(0, fa);
    f32x16 acc;
#pragma unroll
    for (int idx = 0; idx < F::SUB * F::KS; ++idx) {
      const int sb = idx / F::KS, ks = idx % F::KS;
      if (ks == 0) {
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.f;
      }
      u32x4 fn[3];
      if (idx + 1 < F::SUB * F::KS) read_a(idx + 1, fn);
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
          const bool in = ((m >> ((q & 3) + 8 * (q >> 2))) & 1u) == 0u;
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
  const int64_t ntiles = (a.n_items + F::TN - 1) / F::TN;
  int64_t nsplit = 1;
  if (utiles < ncu) {  // too few entry tiles to fill the chip: split the item range
    nsplit = (ncu + utiles - 1) / utiles;
    if (nsplit > ntiles) nsplit = ntiles;
  }
  a.tiles_per_split = (ntiles + nsplit - 1) / nsplit;
  nsplit = (ntiles + a.tiles_per_split - 1) / a.tiles_per_split;  // every split non-empty
  if (utiles > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_full_rank<C>, dim3((unsigned)utiles, (unsigned)nsplit), dim3(F::NT), F::LDS, st, a);
  return hipGetLastError();
}

}  // namespace

bool full_rank_channels_ok(int C) { return C == 32 || C == 64 || C == 128 || C == 256; }

hipError_t full_rank(const float* U, int64_t ldu, int64_t n_users, const float* I, int64_t ldi, int64_t n_items, int C,
                     const int64_t* users, const int64_t* pos, int64_t n_eval, const int64_t* uptr,
                     const int32_t* hist, int32_t* rank, int32_t* ties, hipStream_t st) {
  if (n_eval == 0) return hipSuccess;
  int dev = 0, ncu = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  e = hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
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
