// ppgat_shs.hip -- softmax loss with negatives shared across the batch, on the matrix cores
// (gfx950, MI355X).
//
// One pool of P item ids (strictly ascending) per step; every positive is scored against all:
//   mask[t, j] = pool[j] == pos[t]  or  pool[j] in history(u[t])
//   s0[t]   = <Z[u_t], Z[n_users + pos_t]> / tau,   s[t, j] = <Z[u_t], Z[n_users + pool_j]> / tau
//   lse[t]  = log( exp(s0[t]) + sum_{j not masked} exp(s[t, j]) ),   loss = mean_t (lse[t] - s0[t])
//   c0[t]   = (p0[t] - 1) / (S tau),   c[t, j] = p[t, j] / (S tau) unmasked, 0 masked
//
// The [S, P] scores are a product of gathered rows on v_mfma_f32_32x32x16_bf16 with the
// three-term split of ppgat_split.h (fp32 accuracy) and are never written.  One kernel, k_shs,
// serves the three sweeps on the score-tile engine of ppgat_score_tile.h (shared with the
// full-catalogue rank and top-K kernels: geometry and swizzle, owned fragments, tile staging, the
// A-fragment read, the diagonal score).  A block "owns" 128 rows (32 per wave) whose split
// fragments stay in registers as the B operand, and "streams" the other side's gathered rows
// through double-buffered LDS tiles as the A operand, so the streamed row sits on the
// accumulator's row and the owned row on the lane.  The sweeps' loops, their second product and
// the lse / mask / correction staging beside the tile are this file's own:
//   FWD       owns samples (rows Z[u_t]), streams the pool.  Epilogue: an online (max, sum) per
//             lane over the unmasked scores; the two lane halves merge with the symmetric rule of
//             the sampled loss.  A launch with few sample tiles splits the pool range over
//             blockIdx.y; every split leaves its (max, sum) in the workspace and k_shs_finish
//             merges them in split order, joins the positive (so p0 - 1 = -(mass of the
//             negatives) / (total mass) never cancels), and writes lse, c0 and the loss terms.
//             s0 comes from the same six-term chain (the diagonal of the wave's users against
//             their own positives' rows).
//   BWD_USER  the forward's orientation again: p = exp(s - lse[lane]) sits with the pool item on
//             the accumulator row, so dU^T[c, t] = sum_j I^T[c, j] p[j, t] sums over the
//             accumulator's row index and takes the accumulator tile, split into three bf16 terms,
//             as the next MFMA's B operand with no lane movement.  Its A operand is the pool tile
//             already in LDS, read a second time column-wise, in the k order the accumulator
//             registers impose (element e of lane half h is row 16 s + 8 (e >> 2) + 4 h + (e & 3)).
//             Output: the per-sample gradient [S, C], the positive's term c0 Z[pos] folded in.
//   BWD_ITEM  the roles exchanged: a block owns 128 pool items, streams the gathered user rows
//             (with their lse and mask words beside the tile), and accumulates
//             dI^T[c, j] = sum_t U^T[c, t] p[t, j].  Few pool tiles: the sample range is split
//             over blockIdx.y into partial sums that k_shs_pool_add adds in split order.
// The mask words [S, ceil(P / 32)] (1/32 of the score matrix) are made once by k_shs_mask -- one
// thread per sample walks its sorted history through the ascending pool -- and read by all three
// sweeps; bits past P are set, so a tile's tail needs no second test.
//
// Assembly of dZ, no float atomics: the samples are sorted by user and by positive (rs_sort,
// stable), each sorted array is cut into chunks of 32 records summed in order with head / tail
// slots and a fix-up pass (the scheme of ppgat_ssm.hip); a user's row is the ordered sum of its
// samples' gradients, a positive's row the ordered sum of c0[t] Z[u_t].  k_shs_pool_add then adds
// the pool sums (each pool row has one owner: the ids are distinct) and k_shs_zero clears the
// rows nothing reached.  Two launches give the same bits; grids and splits depend on the shapes
// only.  Contraction is off and every fused multiply-add is an explicit fmaf, so the -O1 debug
// objects round as the -O3 ones.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "ppgat_internal.h"
#include "ppgat_score_tile.h"  // before the pragma, as ppgat_split.h was: it has no chain to contract

#pragma clang fp contract(off)

#include "ppgat_device.h"  // after the pragma: its helpers must not contract here either

namespace ppgat {
namespace {

using split::f32x16;
using split::mfma32_x6;
using split::split3;
using split::u32x4;

inline size_t sh_align(size_t x) { return (x + 255) & ~size_t(255); }

unsigned sh_key_bits(int64_t n) {
  unsigned b = 1;
  while (b < 31 && ((int64_t)1 << b) < n) ++b;
  return b;
}

// (m, l) <- (m, l) merged with (mo, lo); symmetric in its two states, -inf marks an empty one
__device__ __forceinline__ void sh_merge(float& m, float& l, float mo, float lo) {
  const float mn = fmaxf(m, mo);
  const float ms = mn == -INFINITY ? 0.f : mn;
  l = l * expf(m - ms) + lo * expf(mo - ms);
  m = mn;
}

enum { SH_FWD = 0, SH_USER = 1, SH_ITEM = 2 };

constexpr int kShFill = 256;    // blocks wanted before a sweep stops splitting its streamed range
constexpr int kShMinTiles = 4;  // streamed tiles a split holds at least

// 4 waves, one per SIMD (the backward's accumulators need the file); 128 (C = 64) or 64 (C = 128)
// streamed rows per tile, 4 units staged per thread
template <int C>
using ShTile = score::Geo<C, 4, 8192 / C>;
template <int C>
struct ShCfg : ShTile<C> {
  using G = ShTile<C>;
  static constexpr int CB = C / 32;                     // 32-channel blocks of the second product
  static constexpr int MPT = G::TN * G::WAVES / G::NT;  // streamed mask words staged per thread (ITEM)
  static constexpr size_t LDS = 2 * (size_t)G::BUF + 2 * (size_t)G::TN * 4 + 2 * (size_t)G::TN * G::WAVES * 4;
  static_assert(C == 64 || C == 128, "shs: C in {64, 128}");
  static_assert(G::TN <= G::NT && MPT * G::NT == G::TN * G::WAVES, "shs: staging covers the tile");
};

struct ShArg {
  const float* Z;
  int64_t n_users, n_items;
  const int64_t* u;
  const int64_t* pos;
  const int64_t* pool;
  int64_t S, P, W;       // W = ceil(P / 32) mask words per sample
  const uint32_t* mask;  // [S, W]
  float inv_tau;
  int64_t tiles_per_split;
  // FWD
  float* pm;  // [splits, S] partial max
  float* pl;  // [splits, S] partial sum
  float* s0;  // [S]
  // BWD
  const float* lse;
  const float* c0;
  const float* grad_loss;
  float scale;  // 1 / (S tau)
  float* G;     // USER: [S, C];  ITEM: [splits, P, C]
  // CORR
  const float* corrp;  // [P]: the correction of pool[j], gathered once per call (k_shs_corr)
};

// CORR (compile time, as EDGE in the GAT kernels): the logit of pool column j is
// (acc * inv_tau) - corrp[j], in this association in all three sweeps, so the backward
// recomputes the forward's bits.  FWD / USER stream the pool: the tile's corrections ride in the
// LDS slots ITEM uses for the streamed lse.  ITEM owns the pool row: one register.  Without CORR
// the instantiations are the kernels they were.
template <int C, int MODE, bool CORR>
__global__ void __launch_bounds__(ShCfg<C>::NT, 1) k_shs(ShArg a) {
  using F = ShCfg<C>;
  extern __shared__ __attribute__((aligned(16))) unsigned char sh_lds[];
  float* sLse = reinterpret_cast<float*>(sh_lds + 2 * F::BUF);                    // [2][TN]        (ITEM)
  uint32_t* sMsk = reinterpret_cast<uint32_t*>(sh_lds + 2 * F::BUF + 2 * F::TN * 4);  // [2][TN][WAVES] (ITEM)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hf = lane >> 5;
  constexpr bool ITEM = MODE == SH_ITEM;
  const int64_t NO = ITEM ? a.P : a.S;  // owned rows
  const int64_t NS = ITEM ? a.S : a.P;  // streamed rows
  const int64_t W = a.W;
  const int64_t ntiles = (NS + F::TN - 1) / F::TN;
  const int64_t t0 = (int64_t)blockIdx.y * a.tiles_per_split;  // t0 < ntiles (launcher)
  const int64_t t1 = t0 + a.tiles_per_split < ntiles ? t0 + a.tiles_per_split : ntiles;

  auto owned_row = [&](int64_t i) -> const float* {
    return ITEM ? a.Z + (a.n_users + clamp_idx(a.pool[i], a.n_items)) * C : a.Z + clamp_idx(a.u[i], a.n_users) * C;
  };
  auto streamed_row = [&](int64_t i) -> const float* {
    return ITEM ? a.Z + clamp_idx(a.u[i], a.n_users) * C : a.Z + (a.n_users + clamp_idx(a.pool[i], a.n_items)) * C;
  };

  // ---- this lane's owned row: column r of the wave's 32; rows past NO repeat the last ----
  const int64_t b = (int64_t)blockIdx.x * F::TM + wave * 32 + r;
  const int64_t bc = b < NO ? b : NO - 1;
  u32x4 ub[F::KS][3];
  score::load_owned<F>(owned_row(bc), hf, ub);
  // ---- FWD, first split: s0, the users against their own positives' rows, the diagonal ----
  if (MODE == SH_FWD && blockIdx.y == 0) {
    const float sp = score::diag_score<F>(a.Z + (a.n_users + clamp_idx(a.pos[bc], a.n_items)) * C, ub, r, hf);
    if (hf == 0 && b < NO) a.s0[b] = sp * a.inv_tau;
  }
  const float lse_own = MODE == SH_USER ? a.lse[bc] : 0.f;
  const float corr_own = (CORR && ITEM) ? a.corrp[bc] : 0.f;

  float4 pf[F::UPT][2];
  float pf_lse = 0.f;
  uint32_t pf_msk[F::MPT];
  auto load_tile = [&](int64_t t) {
    score::tile_load<F>(pf, t, NS, tid, streamed_row);
    if (ITEM) {
      if (tid < F::TN) {
        const int64_t j = t * F::TN + tid;
        pf_lse = a.lse[j < NS ? j : NS - 1];
      }
#pragma unroll
      for (int k = 0; k < F::MPT; ++k) {
        const int e = tid + k * F::NT, row = e / F::WAVES, w = e % F::WAVES;
        const int64_t j = t * F::TN + row, wi = (int64_t)blockIdx.x * F::WAVES + w;
        pf_msk[k] = (j < NS && wi < W) ? a.mask[j * W + wi] : 0xffffffffu;  // rows / words outside: masked
      }
    } else if (CORR) {
      if (tid < F::TN) {
        const int64_t j = t * F::TN + tid;
        pf_lse = a.corrp[j < NS ? j : NS - 1];
      }
    }
  };
  auto store_tile = [&](int bufi) {
    score::tile_store<F>(sh_lds + bufi * F::BUF, pf, tid);
    if (ITEM) {
      if (tid < F::TN) sLse[bufi * F::TN + tid] = pf_lse;
#pragma unroll
      for (int k = 0; k < F::MPT; ++k) sMsk[bufi * F::TN * F::WAVES + tid + k * F::NT] = pf_msk[k];
    } else if (CORR) {
      if (tid < F::TN) sLse[bufi * F::TN + tid] = pf_lse;
    }
  };

  load_tile(t0);
  store_tile(0);
  __syncthreads();

  float mx = -INFINITY, lsum = 0.f;  // FWD: the unmasked scores this lane has seen
  f32x16 acc2[F::CB];                // BWD: the second product, channel on the row, owned row on the lane
  if (MODE != SH_FWD) {
#pragma unroll
    for (int cb = 0; cb < F::CB; ++cb)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc2[cb][q] = 0.f;
  }
  const int xoff = F::xoff(r, hf);
  for (int64_t t = t0; t < t1; ++t) {
    const int bufi = (int)((t - t0) & 1);
    uint32_t mw[F::SUB];  // FWD / USER: this owned row's mask words of the tile (words past W: all masked)
    if (!ITEM) {
#pragma unroll
      for (int sb = 0; sb < F::SUB; ++sb) {
        const int64_t wi = t * F::SUB + sb;
        mw[sb] = wi < W ? a.mask[bc * W + wi] : 0xffffffffu;
      }
    }
    if (t + 1 < t1) load_tile(t + 1);
    const unsigned char* tile = sh_lds + bufi * F::BUF;
#pragma unroll
    for (int sb = 0; sb < F::SUB; ++sb) {
      f32x16 acc;
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[q] = 0.f;
#pragma unroll
      for (int ks = 0; ks < F::KS; ++ks) {
        u32x4 fa[3];
        score::read_a<F>(tile + r * F::ROWB, sb * F::KS + ks, xoff, fa);
        acc = mfma32_x6(fa, ub[ks], acc);
      }
      // accumulator q: streamed row 32 sb + acc_row(q) + 4 hf, owned column r
      if (MODE == SH_FWD) {
        const uint32_t m = mw[sb] >> (4 * hf);
        const float* cs = sLse + bufi * F::TN + 32 * sb + 4 * hf;  // CORR: the streamed rows' corrections
        float sc[16];
        float tm = -INFINITY;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int row = score::acc_row(q);
          const bool in = ((m >> row) & 1u) == 0u;
          const float lg = CORR ? acc[q] * a.inv_tau - cs[row] : acc[q] * a.inv_tau;
          sc[q] = in ? lg : -INFINITY;
          tm = fmaxf(tm, sc[q]);
        }
        if (tm != -INFINITY) {
          const float mn = fmaxf(mx, tm);
          float add = 0.f;
#pragma unroll
          for (int q = 0; q < 16; ++q) add += __expf(sc[q] - mn);  // masked: exp(-inf) = 0
          lsum = lsum * __expf(mx - mn) + add;
          mx = mn;
        }
      } else {
        float p[16];
        if (ITEM) {
          const float* ls = sLse + bufi * F::TN + 32 * sb + 4 * hf;
          const uint32_t* ms = sMsk + (bufi * F::TN + 32 * sb + 4 * hf) * F::WAVES + wave;
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int row = score::acc_row(q);
            const bool in = ((ms[row * F::WAVES] >> r) & 1u) == 0u;
            const float lg = CORR ? acc[q] * a.inv_tau - corr_own : acc[q] * a.inv_tau;
            p[q] = in ? __expf(lg - ls[row]) : 0.f;
          }
        } else {
          const uint32_t m = mw[sb] >> (4 * hf);
          const float* cs = sLse + bufi * F::TN + 32 * sb + 4 * hf;  // CORR: the streamed rows' corrections
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int row = score::acc_row(q);
            const bool in = ((m >> row) & 1u) == 0u;
            const float lg = CORR ? acc[q] * a.inv_tau - cs[row] : acc[q] * a.inv_tau;
            p[q] = in ? __expf(lg - lse_own) : 0.f;
          }
        }
        // the accumulator tile as the B operand: registers 8 s .. 8 s + 7 are k step s, element
        // e of lane half hf being streamed row 16 s + 8 (e >> 2) + 4 hf + (e & 3); the A operand
        // takes the same rows of channel 32 cb + r from the staged tile, column-wise
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          u32x4 pb[3];
          split3(make_float4(p[8 * s], p[8 * s + 1], p[8 * s + 2], p[8 * s + 3]),
                 make_float4(p[8 * s + 4], p[8 * s + 5], p[8 * s + 6], p[8 * s + 7]), pb[0], pb[1], pb[2]);
#pragma unroll
          for (int cb = 0; cb < F::CB; ++cb) {
            const int unit = 4 * cb + (r >> 3), within = (r & 7) * 2;
            u32x4 ia[3];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int j0 = 32 * sb + 16 * s + 8 * (i >> 1) + 4 * hf + 2 * (i & 1);  // elements 2 i, 2 i + 1
              const unsigned char* p0 = tile + j0 * F::ROWB + ((unit ^ F::swz(j0)) << 4) + within;
              const unsigned char* p1 = tile + (j0 + 1) * F::ROWB + ((unit ^ F::swz(j0 + 1)) << 4) + within;
#pragma unroll
              for (int term = 0; term < 3; ++term) {
                const uint32_t lo = *reinterpret_cast<const uint16_t*>(p0 + term * F::PART);
                const uint32_t hi = *reinterpret_cast<const uint16_t*>(p1 + term * F::PART);
                ia[term][i] = lo | (hi << 16);
              }
            }
            acc2[cb] = mfma32_x6(ia, pb, acc2[cb]);
          }
        }
      }
    }
    if (t + 1 < t1) store_tile(bufi ^ 1);
    __syncthreads();
  }

  if (MODE == SH_FWD) {
    const float mo = __shfl_xor(mx, 32), lo = __shfl_xor(lsum, 32);
    sh_merge(mx, lsum, mo, lo);
    if (hf == 0 && b < NO) {
      a.pm[(int64_t)blockIdx.y * a.S + b] = mx;
      a.pl[(int64_t)blockIdx.y * a.S + b] = lsum;
    }
  } else if (b < NO) {
    // acc2[cb][q]: channel 32 cb + acc_row(q) + 4 hf of owned row b
    const float g = a.grad_loss[0];
    const float sg = a.scale * g;
    float* out = a.G + ((int64_t)blockIdx.y * NO + b) * C + 4 * hf;
    float c0g = 0.f;
    const float* zp = a.Z;
    if (MODE == SH_USER) {  // the positive's term of the sample's gradient
      c0g = a.c0[b] * g;
      zp = a.Z + (a.n_users + clamp_idx(a.pos[b], a.n_items)) * C + 4 * hf;
    }
#pragma unroll
    for (int cb = 0; cb < F::CB; ++cb)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        float4 v = make_float4(acc2[cb][4 * gq] * sg, acc2[cb][4 * gq + 1] * sg, acc2[cb][4 * gq + 2] * sg,
                               acc2[cb][4 * gq + 3] * sg);
        if (MODE == SH_USER) v = fma4(c0g, ld4(zp + 32 * cb + 8 * gq), v);
        st4(out + 32 * cb + 8 * gq, v);
      }
  }
}

// ---------------------------------------------------------------------------
// the mask words, and the index checks
// ---------------------------------------------------------------------------
// the mask words and the two counts cleared by a kernel (16 B per thread; the region is padded to
// 256 B), so a captured step holds kernels only
__global__ void __launch_bounds__(256) k_shs_clear(uint4* __restrict__ words, int64_t n16, int32_t* __restrict__ bad) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c < n16) words[c] = make_uint4(0u, 0u, 0u, 0u);
  if (c == 0) {
    bad[0] = 0;
    bad[1] = 0;
  }
}

// thread t < S: sample t's words (cleared by k_shs_clear): its history and its positive looked up
// in the ascending pool, and the bits past P.  thread t < P: pool[t] in range and above pool[t-1].
// bad[0] counts out-of-range indices (clamped), bad[1] pool entries out of order.
__global__ void __launch_bounds__(256) k_shs_mask(const int64_t* __restrict__ u, const int64_t* __restrict__ pos,
                                                  const int64_t* __restrict__ pool, int64_t S, int64_t P, int64_t W,
                                                  int64_t n_users, int64_t n_items, const int64_t* __restrict__ uptr,
                                                  const int32_t* __restrict__ hist, uint32_t* __restrict__ mask,
                                                  int32_t* __restrict__ bad) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int nbad = 0, nord = 0;
  if (t < P) {
    const int64_t v = pool[t];
    if (v < 0 || v >= n_items) ++nbad;
    if (t > 0 && pool[t - 1] >= v) ++nord;
  }
  if (t < S) {
    const int64_t u0 = u[t], p0 = pos[t];
    if (u0 < 0 || u0 >= n_users) ++nbad;
    if (p0 < 0 || p0 >= n_items) ++nbad;
    uint32_t* w = mask + t * W;
    if (P & 31) w[W - 1] = 0xffffffffu << (int)(P & 31);
    // first pool index >= v in [lo, P)
    auto lower = [&](int64_t v, int64_t lo) {
      int64_t hi = P;
      while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (pool[mid] < v) lo = mid + 1; else hi = mid;
      }
      return lo;
    };
    const int64_t pc = clamp_idx(p0, n_items);
    const int64_t kp = lower(pc, 0);
    if (kp < P && pool[kp] == pc) w[kp >> 5] |= 1u << (int)(kp & 31);
    if (uptr != nullptr) {
      const int64_t uc = clamp_idx(u0, n_users);
      int64_t k = 0;  // the history ascends: the search window only moves forward
      for (int64_t cur = uptr[uc], cend = uptr[uc + 1]; cur < cend && k < P; ++cur) {
        const int64_t h = hist[cur];
        k = lower(h, k);
        if (k < P && pool[k] == h) w[k >> 5] |= 1u << (int)(k & 31);
      }
    }
  }
  if (nbad) atomicAdd(bad, nbad);  // (integer counts: exact in any order)
  if (nord) atomicAdd(bad + 1, nord);
}

// corrp[j] = corr[pool[j]] (clamped like every other use of the pool), once per call
__global__ void __launch_bounds__(256) k_shs_corr(const float* __restrict__ corr, const int64_t* __restrict__ pool,
                                                  int64_t P, int64_t n_items, float* __restrict__ corrp) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < P) corrp[j] = corr[clamp_idx(pool[j], n_items)];
}

// ---------------------------------------------------------------------------
// forward finish: the splits' (max, sum) merged in split order, the positive joined
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_shs_finish(const float* __restrict__ pm, const float* __restrict__ pl,
                                                    const float* __restrict__ s0v, int64_t S, int nsplit, float scale,
                                                    float* __restrict__ lse, float* __restrict__ c0,
                                                    float* __restrict__ block_loss) {
  __shared__ float red[256];
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float term = 0.f;
  if (t < S) {
    float mx = pm[t], l = pl[t];
    for (int y = 1; y < nsplit; ++y) sh_merge(mx, l, pm[(int64_t)y * S + t], pl[(int64_t)y * S + t]);
    const float s0 = s0v[t];
    // en = mass of the negatives, e0 = the positive's, both relative to mt
    const float mt = fmaxf(mx, s0);
    const float en = l * expf(mx - mt), e0 = expf(s0 - mt);
    const float inv = 1.f / (en + e0);
    term = mt == s0 ? log1pf(en) : (mt - s0) + logf(en + e0);
    lse[t] = mt == s0 ? s0 + log1pf(en) : mt + logf(en + e0);
    c0[t] = -(en * inv) * scale;
  }
  red[threadIdx.x] = term;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) block_loss[blockIdx.x] = red[0];
}

// ordered sum of the block partials -> the mean loss
__global__ void __launch_bounds__(1024) k_shs_loss(const float* __restrict__ block_loss, int64_t nb, float denom,
                                                   float* __restrict__ loss) {
  __shared__ float red[1024];
  float s = 0.f;
  for (int64_t b = threadIdx.x; b < nb; b += 1024) s += block_loss[b];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = red[0] / denom;
}

// ---------------------------------------------------------------------------
// backward assembly
// ---------------------------------------------------------------------------
template <int C>
struct ShGeo {
  static constexpr int LPR = C / 4;      // lanes per row (float4 each)
  static constexpr int SPB = 256 / LPR;  // subgroups per 256-thread block
};

// sort keys of both sides, and the touched-row map cleared (16 B per thread)
__global__ void k_shs_keys(const int64_t* __restrict__ u, const int64_t* __restrict__ pos, int64_t S, int64_t n_users,
                           int64_t n_items, int64_t n_rows, int32_t* __restrict__ ukey, int32_t* __restrict__ uval,
                           int32_t* __restrict__ ikey, int32_t* __restrict__ ival, uint8_t* __restrict__ touched) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c * 16 < n_rows) *reinterpret_cast<uint4*>(touched + c * 16) = make_uint4(0u, 0u, 0u, 0u);
  if (c < S) {
    ukey[c] = (int32_t)clamp_idx(u[c], n_users);
    uval[c] = (int32_t)c;
    ikey[c] = (int32_t)(n_users + clamp_idx(pos[c], n_items));
    ival[c] = (int32_t)c;
  }
}

constexpr int kShChunk = 32;

// The S records of one side, sorted by destination row (skey[p], sval[p] = sample t):
//   user side      source = row t of the per-sample gradients, coefficient 1
//   positive side  source = Z[u_t], coefficient c0[t] grad
struct ShRecs {
  const int32_t* skey;
  const int32_t* sval;
  const float* table;
  const int64_t* u;
  int64_t n_users;
  const float* c0;
};

template <bool USER>
__device__ __forceinline__ void sh_rec_load(const ShRecs& r, int64_t p, float g, int32_t& dst, int32_t& src, float& cf) {
  const int32_t t = r.sval[p];
  dst = r.skey[p];
  if (USER) {
    src = t;
    cf = 1.f;
  } else {
    src = (int32_t)clamp_idx(r.u[t], r.n_users);
    cf = r.c0[t] * g;
  }
}

// chunk pass: a subgroup owns 32 consecutive records.  Runs of one destination row complete
// inside the chunk are written to dZ; one that continues from the previous chunk goes to slot
// "head", one that continues into the next to slot "tail".
template <int C, bool USER>
__global__ void __launch_bounds__(256) k_shs_chunks(ShRecs r, int64_t total, const float* __restrict__ grad_loss,
                                                    float* __restrict__ dZ, float* __restrict__ slots) {
  constexpr int LPR = ShGeo<C>::LPR, SPB = ShGeo<C>::SPB;
  __shared__ int32_t s_src[SPB][kShChunk];
  __shared__ int32_t s_dst[SPB][kShChunk];
  __shared__ float s_cf[SPB][kShChunk];
  const int tid = threadIdx.x;
  const int sg = tid / LPR, sl = tid % LPR;
  const int64_t ch = (int64_t)blockIdx.x * SPB + sg;
  const int64_t b0 = ch * kShChunk;
  const float g = grad_loss[0];
  if (b0 < total) {
    for (int q = sl; q < kShChunk; q += LPR) {
      const int64_t p = b0 + q;
      int32_t src = 0, dst = -1;
      float cf = 0.f;
      if (p < total) sh_rec_load<USER>(r, p, g, dst, src, cf);
      s_src[sg][q] = src;
      s_dst[sg][q] = dst;
      s_cf[sg][q] = cf;
    }
  }
  __syncthreads();
  if (b0 >= total) return;
  const int len = (int)min((int64_t)kShChunk, total - b0);
  const bool starts_before = b0 > 0 && r.skey[b0 - 1] == s_dst[sg][0];
  const bool ends_after = b0 + len < total && r.skey[b0 + len] == s_dst[sg][len - 1];
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  int seg_start = 0;
  constexpr int UB = 8;  // source rows in flight per subgroup
  for (int q0 = 0; q0 < len; q0 += UB) {
    float4 v[UB];
#pragma unroll
    for (int k = 0; k < UB; ++k) {
      const int q = q0 + k;
      v[k] = q < len ? ld4(r.table + (int64_t)s_src[sg][q] * C + sl * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int k = 0; k < UB; ++k) {
      const int q = q0 + k;
      if (q >= len) break;
      acc = fma4(s_cf[sg][q], v[k], acc);
      const bool last_of_seg = q == len - 1 || s_dst[sg][q + 1] != s_dst[sg][q];
      if (last_of_seg) {
        const bool first = seg_start == 0, last = q == len - 1;
        if (first && starts_before) st4(slots + (ch * 2 + 0) * C + sl * 4, acc);
        else if (last && ends_after) st4(slots + (ch * 2 + 1) * C + sl * 4, acc);
        else st4(dZ + (int64_t)s_dst[sg][q] * C + sl * 4, acc);
        acc = make_float4(0.f, 0.f, 0.f, 0.f);
        seg_start = q + 1;
      }
    }
  }
}

// fix-up: the chunk in which a chunk-spanning run starts sums its tail slot and the head slots
// of the following chunks, in chunk order, and writes the row
template <int C>
__global__ void __launch_bounds__(256) k_shs_fixup(const int32_t* __restrict__ skey, int64_t total,
                                                   const float* __restrict__ slots, float* __restrict__ dZ) {
  constexpr int LPR = ShGeo<C>::LPR, SPB = ShGeo<C>::SPB;
  const int sg = threadIdx.x / LPR, sl = threadIdx.x % LPR;
  const int64_t ch = (int64_t)blockIdx.x * SPB + sg;
  const int64_t b0 = ch * kShChunk;
  if (b0 >= total) return;
  const int64_t b1 = min(b0 + kShChunk, total);
  if (b1 >= total) return;
  const int32_t row = skey[b1 - 1];
  if (skey[b1] != row) return;                                   // does not continue
  if (skey[b0] == row && b0 > 0 && skey[b0 - 1] == row) return;  // started earlier
  float4 acc = ld4(slots + (ch * 2 + 1) * C + sl * 4);
  for (int64_t c2 = ch + 1;; ++c2) {
    const int64_t e0 = c2 * kShChunk;
    const int64_t e1 = min(e0 + kShChunk, total);
    acc = add4(acc, ld4(slots + (c2 * 2 + 0) * C + sl * 4));
    if (!(skey[e1 - 1] == row && e1 < total && skey[e1] == row)) break;
  }
  st4(dZ + (int64_t)row * C + sl * 4, acc);
}

// the pool rows: the splits' partial sums in split order, then the positive records already in
// dZ (if any reached the row).  One subgroup per pool item; k_shs_pool_mark then marks the rows.
template <int C>
__global__ void __launch_bounds__(256) k_shs_pool_add(const float* __restrict__ Gp, int nsplit,
                                                      const int64_t* __restrict__ pool, int64_t P, int64_t n_users,
                                                      int64_t n_items, const uint8_t* __restrict__ touched,
                                                      float* __restrict__ dZ) {
  constexpr int LPR = ShGeo<C>::LPR, SPB = ShGeo<C>::SPB;
  const int sg = threadIdx.x / LPR, sl = threadIdx.x % LPR;
  const int64_t j = (int64_t)blockIdx.x * SPB + sg;
  if (j >= P) return;
  const int64_t row = n_users + clamp_idx(pool[j], n_items);
  float4 acc = ld4(Gp + j * C + sl * 4);
  for (int y = 1; y < nsplit; ++y) acc = add4(acc, ld4(Gp + ((int64_t)y * P + j) * C + sl * 4));
  if (touched[row]) acc = add4(acc, ld4(dZ + row * C + sl * 4));
  st4(dZ + row * C + sl * 4, acc);
}

__global__ void __launch_bounds__(256) k_shs_pool_mark(const int64_t* __restrict__ pool, int64_t P, int64_t n_users,
                                                       int64_t n_items, uint8_t* __restrict__ touched) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < P) touched[n_users + clamp_idx(pool[j], n_items)] = 1;
}

// rows nothing reaches
template <int C>
__global__ void __launch_bounds__(256) k_shs_zero(const uint8_t* __restrict__ touched, int64_t n_rows,
                                                  float* __restrict__ dZ) {
  constexpr int LPR = ShGeo<C>::LPR, SPB = ShGeo<C>::SPB;
  const int sg = threadIdx.x / LPR, sl = threadIdx.x % LPR;
  for (int64_t row = (int64_t)blockIdx.x * SPB + sg; row < n_rows; row += (int64_t)gridDim.x * SPB)
    if (!touched[row]) st4(dZ + row * C + sl * 4, make_float4(0.f, 0.f, 0.f, 0.f));
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
// how a sweep with `otiles` owned tiles cuts its `stiles` streamed tiles (shapes only)
struct ShSplit {
  int64_t n, tiles_per_split;
};
ShSplit sh_split(int64_t otiles, int64_t stiles) {
  int64_t n = 1;
  if (otiles < kShFill) {
    n = (kShFill + otiles - 1) / otiles;
    if (n > stiles / kShMinTiles) n = stiles / kShMinTiles;  // a split is worth its owned rows' load and split
  }
  if (n < 1) n = 1;
  const int64_t per = stiles > 0 ? (stiles + n - 1) / n : 1;
  n = stiles > 0 ? (stiles + per - 1) / per : 1;  // every split non-empty
  return {n, per};
}

template <int C>
ShSplit sh_split_fwd(int64_t S, int64_t P) {
  using F = ShCfg<C>;
  return sh_split((S + F::TM - 1) / F::TM, (P + F::TN - 1) / F::TN);
}
template <int C>
ShSplit sh_split_item(int64_t S, int64_t P) {
  using F = ShCfg<C>;
  return sh_split((P + F::TM - 1) / F::TM, (S + F::TN - 1) / F::TN);
}

// workspace: finish block partials | forward (max, sum) per split | s0 | mask words | per-sample
// gradients [S, C] | pool partial sums [splits, P, C] | user keys, vals and their ping-pong pair,
// positive keys, vals and pair [S] each | slots [chunks][2][C] | radix sort | touched [N]
struct ShWs {
  float* block_loss;
  float* pm;
  float* pl;
  float* s0;
  uint32_t* mask;
  float* Gu;
  float* Gp;
  int32_t* uk[2];
  int32_t* uv[2];
  int32_t* ik[2];
  int32_t* iv[2];
  float* slots;
  void* tmp;
  uint8_t* touched;
  size_t mask_bytes;
  size_t bytes;
};

ShWs sh_ws(void* ws, int64_t N, int64_t S, int64_t P, int C) {
  const int64_t S1 = S > 0 ? S : 1, P1 = P > 0 ? P : 1;
  const int64_t W = (P1 + 31) / 32;
  const ShSplit sf = C == 64 ? sh_split_fwd<64>(S1, P1) : sh_split_fwd<128>(S1, P1);
  const ShSplit si = C == 64 ? sh_split_item<64>(S1, P1) : sh_split_item<128>(S1, P1);
  const int64_t chunks = (S1 + kShChunk - 1) / kShChunk;
  const unsigned bits = sh_key_bits(N + 1);
  char* p = static_cast<char*>(ws);
  size_t o = 0;
  ShWs w;
  w.block_loss = reinterpret_cast<float*>(p + o); o += sh_align((size_t)((S1 + 255) / 256) * 4);
  w.pm = reinterpret_cast<float*>(p + o); o += sh_align((size_t)sf.n * S1 * 4);
  w.pl = reinterpret_cast<float*>(p + o); o += sh_align((size_t)sf.n * S1 * 4);
  w.s0 = reinterpret_cast<float*>(p + o); o += sh_align((size_t)S1 * 4);
  w.mask = reinterpret_cast<uint32_t*>(p + o);
  w.mask_bytes = (size_t)S1 * W * 4;
  o += sh_align(w.mask_bytes);
  w.Gu = reinterpret_cast<float*>(p + o); o += sh_align((size_t)S1 * C * 4);
  w.Gp = reinterpret_cast<float*>(p + o); o += sh_align((size_t)si.n * P1 * C * 4);
  const size_t s4 = sh_align((size_t)S1 * 4);
  for (int k = 0; k < 2; ++k) {
    w.uk[k] = reinterpret_cast<int32_t*>(p + o); o += s4;
    w.uv[k] = reinterpret_cast<int32_t*>(p + o); o += s4;
    w.ik[k] = reinterpret_cast<int32_t*>(p + o); o += s4;
    w.iv[k] = reinterpret_cast<int32_t*>(p + o); o += s4;
  }
  w.slots = reinterpret_cast<float*>(p + o); o += sh_align((size_t)chunks * 2 * C * 4);
  w.tmp = p + o; o += rs_workspace_bytes(S1, bits);
  w.touched = reinterpret_cast<uint8_t*>(p + o); o += sh_align((size_t)N + 16);
  w.bytes = o;
  return w;
}

template <int C, int MODE, bool CORR>
hipError_t sh_launch_c(const ShArg& a, int64_t otiles, int64_t nsplit, hipStream_t st) {
  using F = ShCfg<C>;
  const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_shs<C, MODE, CORR>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)F::LDS);
  if (attr != hipSuccess) return attr;
  if (otiles > 0x7fffffff || nsplit > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_shs<C, MODE, CORR>), dim3((unsigned)otiles, (unsigned)nsplit), dim3(F::NT), F::LDS, st, a);
  return hipGetLastError();
}

template <int C, int MODE>
hipError_t sh_launch(const ShArg& a, int64_t otiles, int64_t nsplit, hipStream_t st) {
  return a.corrp != nullptr ? sh_launch_c<C, MODE, true>(a, otiles, nsplit, st)
                            : sh_launch_c<C, MODE, false>(a, otiles, nsplit, st);
}

// the gathered corrections sit behind the uncorrected layout, which stays what it was
float* sh_corrp(void* ws, int64_t N, int64_t S, int64_t P, int C) {
  return reinterpret_cast<float*>(static_cast<char*>(ws) + sh_ws(nullptr, N, S, P, C).bytes);
}

template <int C>
hipError_t sh_fwd(const float* Z, int64_t n_users, int64_t n_items, const int64_t* u, const int64_t* pos, int64_t S,
                  const int64_t* pool, int64_t P, const int64_t* uptr, const int32_t* hist, const float* corr,
                  float tau, float* loss, float* lse, float* c0, int32_t* bad, void* ws, hipStream_t st) {
  using F = ShCfg<C>;
  const ShWs w = sh_ws(ws, n_users + n_items, S, P, C);
  float* corrp = corr != nullptr ? sh_corrp(ws, n_users + n_items, S, P, C) : nullptr;
  if (corrp != nullptr)
    hipLaunchKernelGGL(k_shs_corr, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, corr, pool, P, n_items, corrp);
  const int64_t W = (P + 31) / 32;
  const int64_t n16 = S > 0 ? (int64_t)((w.mask_bytes + 15) / 16) : 0;
  hipLaunchKernelGGL(k_shs_clear, dim3((unsigned)((n16 + 255) / 256 + 1)), dim3(256), 0, st,
                     reinterpret_cast<uint4*>(w.mask), n16, bad);
  hipError_t e = hipSuccess;
  const int64_t mt = S > P ? S : P;
  hipLaunchKernelGGL(k_shs_mask, dim3((unsigned)((mt + 255) / 256)), dim3(256), 0, st, u, pos, pool, S, P, W, n_users,
                     n_items, uptr, hist, w.mask, bad);
  const int64_t nb = (S + 255) / 256;
  if (S > 0) {
    const ShSplit sp = sh_split_fwd<C>(S, P);
    ShArg a{};
    a.Z = Z; a.n_users = n_users; a.n_items = n_items; a.u = u; a.pos = pos; a.pool = pool;
    a.S = S; a.P = P; a.W = W; a.mask = w.mask; a.inv_tau = 1.f / tau; a.tiles_per_split = sp.tiles_per_split;
    a.pm = w.pm; a.pl = w.pl; a.s0 = w.s0; a.corrp = corrp;
    e = sh_launch<C, SH_FWD>(a, (S + F::TM - 1) / F::TM, sp.n, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_shs_finish, dim3((unsigned)nb), dim3(256), 0, st, w.pm, w.pl, w.s0, S, (int)sp.n,
                       1.f / ((float)S * tau), lse, c0, w.block_loss);
  }
  hipLaunchKernelGGL(k_shs_loss, dim3(1), dim3(1024), 0, st, w.block_loss, S > 0 ? nb : 0, S > 0 ? (float)S : 1.f,
                     loss);
  return hipGetLastError();
}

template <int C>
hipError_t sh_bwd(const float* Z, int64_t n_users, int64_t n_items, const int64_t* u, const int64_t* pos, int64_t S,
                  const int64_t* pool, int64_t P, bool corrected, float tau, const float* lse, const float* c0,
                  const float* grad_loss, float* dZ, void* ws, hipStream_t st) {
  using F = ShCfg<C>;
  using G = ShGeo<C>;
  const int64_t N = n_users + n_items;
  const ShWs w = sh_ws(ws, N, S, P, C);
  ShArg a{};
  a.Z = Z; a.n_users = n_users; a.n_items = n_items; a.u = u; a.pos = pos; a.pool = pool;
  a.S = S; a.P = P; a.W = (P + 31) / 32; a.mask = w.mask; a.inv_tau = 1.f / tau;
  a.lse = lse; a.c0 = c0; a.grad_loss = grad_loss; a.scale = 1.f / ((float)S * tau);
  a.corrp = corrected ? sh_corrp(ws, N, S, P, C) : nullptr;  // (the forward's gather, like its mask words)
  // the two sweeps
  a.G = w.Gu;
  a.tiles_per_split = (P + F::TN - 1) / F::TN;
  hipError_t e = sh_launch<C, SH_USER>(a, (S + F::TM - 1) / F::TM, 1, st);
  if (e != hipSuccess) return e;
  const ShSplit si = sh_split_item<C>(S, P);
  a.G = w.Gp;
  a.tiles_per_split = si.tiles_per_split;
  e = sh_launch<C, SH_ITEM>(a, (P + F::TM - 1) / F::TM, si.n, st);
  if (e != hipSuccess) return e;
  // the samples sorted by user and by positive
  const unsigned bits = sh_key_bits(N + 1);
  const int64_t kthreads = S > (N + 15) / 16 ? S : (N + 15) / 16;  // (enough threads to clear the map)
  hipLaunchKernelGGL(k_shs_keys, dim3((unsigned)((kthreads + 255) / 256)), dim3(256), 0, st, u, pos, S, n_users,
                     n_items, N, w.uk[0], w.uv[0], w.ik[0], w.iv[0], w.touched);
  bool u1 = false, i1 = false;
  e = rs_sort(w.uk[0], w.uv[0], w.uk[1], w.uv[1], S, bits, w.tmp, &u1, st, w.touched, N);
  if (e != hipSuccess) return e;
  e = rs_sort(w.ik[0], w.iv[0], w.ik[1], w.iv[1], S, bits, w.tmp, &i1, st, w.touched, N);
  if (e != hipSuccess) return e;
  const ShRecs ru{w.uk[u1], w.uv[u1], w.Gu, u, n_users, c0};
  const ShRecs ri{w.ik[i1], w.iv[i1], Z, u, n_users, c0};
  const int64_t chunks = (S + kShChunk - 1) / kShChunk;
  const unsigned g = (unsigned)((chunks + G::SPB - 1) / G::SPB);
  // the two sides one after the other on the stream: they share the slots
  hipLaunchKernelGGL((k_shs_chunks<C, true>), dim3(g), dim3(256), 0, st, ru, S, grad_loss, dZ, w.slots);
  hipLaunchKernelGGL(k_shs_fixup<C>, dim3(g), dim3(256), 0, st, ru.skey, S, w.slots, dZ);
  hipLaunchKernelGGL((k_shs_chunks<C, false>), dim3(g), dim3(256), 0, st, ri, S, grad_loss, dZ, w.slots);
  hipLaunchKernelGGL(k_shs_fixup<C>, dim3(g), dim3(256), 0, st, ri.skey, S, w.slots, dZ);
  hipLaunchKernelGGL(k_shs_pool_add<C>, dim3((unsigned)((P + G::SPB - 1) / G::SPB)), dim3(256), 0, st, w.Gp, (int)si.n,
                     pool, P, n_users, n_items, w.touched, dZ);
  hipLaunchKernelGGL(k_shs_pool_mark, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, pool, P, n_users, n_items,
                     w.touched);
  int64_t gz = (N + G::SPB - 1) / G::SPB;
  if (gz > 4096) gz = 4096;
  hipLaunchKernelGGL(k_shs_zero<C>, dim3((unsigned)gz), dim3(256), 0, st, w.touched, N, dZ);
  return hipGetLastError();
}

}  // namespace

bool shs_channels_ok(int C) { return C == 64 || C == 128; }

size_t shs_workspace_bytes(int64_t N, int64_t S, int64_t P, int C) { return sh_ws(nullptr, N, S, P, C).bytes; }

size_t shs_corr_workspace_bytes(int64_t N, int64_t S, int64_t P, int C) {
  return sh_ws(nullptr, N, S, P, C).bytes + sh_align((size_t)(P > 0 ? P : 1) * 4);
}

hipError_t shs_fwd(const float* Z, int64_t n_users, int64_t n_items, int C, const int64_t* u, const int64_t* pos,
                   int64_t S, const int64_t* pool, int64_t P, const int64_t* uptr, const int32_t* hist,
                   const float* corr, float tau, float* loss, float* lse, float* c0, int32_t* bad, void* ws,
                   hipStream_t st) {
  switch (C) {
    case 64:
      return sh_fwd<64>(Z, n_users, n_items, u, pos, S, pool, P, uptr, hist, corr, tau, loss, lse, c0, bad, ws, st);
    case 128:
      return sh_fwd<128>(Z, n_users, n_items, u, pos, S, pool, P, uptr, hist, corr, tau, loss, lse, c0, bad, ws, st);
    default: return hipErrorInvalidValue;
  }
}

hipError_t shs_bwd(const float* Z, int64_t n_users, int64_t n_items, int C, const int64_t* u, const int64_t* pos,
                   int64_t S, const int64_t* pool, int64_t P, bool corrected, float tau, const float* lse,
                   const float* c0, const float* grad_loss, float* dZ, void* ws, hipStream_t st) {
  if (S == 0) return hipMemsetAsync(dZ, 0, (size_t)(n_users + n_items) * C * 4, st);
  switch (C) {
    case 64:
      return sh_bwd<64>(Z, n_users, n_items, u, pos, S, pool, P, corrected, tau, lse, c0, grad_loss, dZ, ws, st);
    case 128:
      return sh_bwd<128>(Z, n_users, n_items, u, pos, S, pool, P, corrected, tau, lse, c0, grad_loss, dZ, ws, st);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace ppgat
