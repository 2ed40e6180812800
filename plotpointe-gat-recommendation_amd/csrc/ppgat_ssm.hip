// ppgat_ssm.hip -- fused sampled-softmax loss with many negatives per positive, for CDNA4
// (gfx950, MI355X).
//
// One positive scored against M sampled negatives; cand [S, K1 = M + 1], column 0 the positive:
//   s[t, m] = <Z[u_t], Z[n_users + cand[t, m]]> / tau
//   loss    = (1/S) sum_t ( logsumexp_m s[t, m] - s[t, 0] )
//   c[t, m] = (softmax_m(s[t, :]) - [m == 0]) / (S tau)
//   dZ[u_t] += sum_m c[t, m] Z[n_users + cand[t, m]];   dZ[n_users + cand[t, m]] += c[t, m] Z[u_t]
//
// Layout: a row of C floats is C/4 lanes ("subgroup") x float4; the 64/(C/4) subgroups of a wave
// take different candidates of the same sample, U gathered rows in flight each (>= 8 per wave).
//   forward   one wave per sample, Z[u_t] in registers.  Pass 1 gathers the candidate rows, leaves
//             the raw scores in coef and keeps an online (max, sum) over the NEGATIVES per
//             subgroup, merged across subgroups with a symmetric rule (both partners of an
//             exchange get the same bits).  The positive joins at the end, so
//               p_0 - 1 = -(mass of the negatives) / (total mass)
//             is formed without the cancellation of "p_0 - 1" when p_0 -> 1, and the loss term is
//             log1p(mass of the negatives) when the positive holds the maximum.  Pass 2 turns the
//             scores into c: the lane that wrote a score reads it back (a thread sees its own
//             stores), so no fence or LDS is needed.  Loss terms: one partial per block, summed
//             in block order (k_ssm_loss).
//   backward  no float atomics.  Users and items own disjoint row ranges of dZ.
//             item side: the S K1 records (row n_users + cand[t, m]; source u_t; c[t, m]) are
//             sorted by row (rs_sort, stable: equal rows stay in record order);
//             user side: the S samples are sorted by u_t, and the records of a user are then
//             the K1 candidates of each of its samples, sample after sample -- an implicit
//             array of S K1 records that is never written out; the gathers are recomputed
//             from coef rather than kept by the forward (DESIGN section 17 says why).
//             Either record array is cut into chunks of 32; a subgroup sums its chunk in order,
//             rows complete inside the chunk are written, a row that spans chunks leaves head /
//             tail partials in slots and k_ssm_fixup adds them in chunk order.  Rows no record
//             reaches are zeroed from the touched-byte map the sorts' last passes fill.
// Every row of dZ is written exactly once; two launches give the same bits.  Contraction is off
// and every fused multiply-add is an explicit fmaf, so the -O1 debug objects round as the -O3 ones.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "ppgat_internal.h"
#include "ppgat_lanes.h"

#pragma clang fp contract(off)

#include "ppgat_device.h"  // after the pragma: its helpers must not contract here either

namespace ppgat {
namespace {

inline size_t align_up(size_t x) { return (x + 255) & ~size_t(255); }

unsigned key_bits(int64_t n) {
  unsigned b = 1;
  while (b < 31 && ((int64_t)1 << b) < n) ++b;
  return b;
}

template <int C>
struct Geo {
  static constexpr int LPR = C / 4;                      // lanes per row
  static constexpr int EPW = 64 / LPR;                   // candidates side by side per wave
  static constexpr int U = (8 / EPW) >= 2 ? 8 / EPW : 2;  // gathered rows in flight per subgroup
  static constexpr int SPB = 256 / LPR;                  // subgroups per 256-thread block
  static_assert(C == 32 || C == 64 || C == 128 || C == 256, "ssm: C in {32, 64, 128, 256}");
};

constexpr int kWaves = 4;  // waves (samples in flight) per forward block

// (m, l) <- (m, l) merged with (mo, lo); symmetric in its two states (products, then one add),
// so both lanes of an exchange end with the same bits.  -inf marks a state without candidates.
__device__ __forceinline__ void merge_ml(float& m, float& l, float mo, float lo) {
  const float mn = fmaxf(m, mo);
  const float ms = mn == -INFINITY ? 0.f : mn;
  l = l * expf(m - ms) + lo * expf(mo - ms);
  m = mn;
}

// ---------------------------------------------------------------------------
// forward: one wave per sample
// ---------------------------------------------------------------------------
// CORR: corr [n_items] is subtracted from the logit of every negative (columns >= 1; never from
// the positive's) as the score is formed, so it is inside the online (max, sum) and inside the
// scores pass 2 reads back: coef is the softmax of the corrected logits and the backward is the
// uncorrected one's.  Without CORR the kernel is the one it was.
template <int C, bool CORR>
__global__ void __launch_bounds__(256) k_ssm_fwd(const float* __restrict__ Z, int64_t n_users, int64_t n_items,
                                                 const int64_t* __restrict__ u, const int64_t* __restrict__ cand,
                                                 const float* __restrict__ corr, int64_t S, int K1, float tau,
                                                 float* coef,
                                                 float* __restrict__ block_loss, int32_t* __restrict__ block_bad) {
  using G = Geo<C>;
  constexpr int LPR = G::LPR, EPW = G::EPW, U = G::U;
  __shared__ float sl_loss[kWaves];
  __shared__ int sl_bad;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int sg = lane / LPR, sl = lane % LPR;
  if (tid == 0) sl_bad = 0;
  __syncthreads();
  float lsum = 0.f;  // this wave's samples, in order (fixed grid => fixed partition)
  int nbad = 0;      // out-of-range indices seen by this lane (clamped; the caller raises)
  const float scale = 1.f / ((float)S * tau);
  for (int64_t t = (int64_t)blockIdx.x * kWaves + wave; t < S; t += (int64_t)gridDim.x * kWaves) {  // wave-uniform
    const int64_t u0 = u[t];
    if (lane == 0 && (u0 < 0 || u0 >= n_users)) ++nbad;
    const float4 a = ld4(Z + clamp_idx(u0, n_users) * C + sl * 4);
    const int64_t base = t * K1;
    float mx = -INFINITY, l = 0.f;  // the negatives this subgroup has seen
    float s0 = 0.f;                 // the positive's score (subgroup 0)
    // pass 1: candidate mb + k EPW + sg for k < U; lane sl == k of the subgroup keeps its score
    for (int mb = 0; mb < K1; mb += EPW * U) {
      float4 v[U];
      float cr[U];  // CORR: the candidates' correction terms (0 for the positive)
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const int m = mb + k * EPW + sg;
        v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        cr[k] = 0.f;
        if (m < K1) {
          const int64_t id = cand[base + m];
          if (sl == 0 && (id < 0 || id >= n_items)) ++nbad;
          v[k] = ld4(Z + (n_users + clamp_idx(id, n_items)) * C + sl * 4);
          if (CORR && m > 0) cr[k] = corr[clamp_idx(id, n_items)];
        }
      }
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const int m = mb + k * EPW + sg;
        const float d = group_reduce<Op::Sum, 1, LPR / 2>(dot4(a, v[k]));  // (every lane: DPP / permlane steps)
        const float s = CORR ? d / tau - cr[k] : d / tau;
        if (m < K1) {
          if (sl == k) coef[base + m] = s;
          if (m == 0) s0 = s;
          else {
            const float mn = fmaxf(mx, s);
            l = l * expf(mx - mn) + expf(s - mn);
            mx = mn;
          }
        }
      }
    }
    // the subgroups' states -> the wave's (offsets >= LPR >= 8: plain exchanges)
#pragma unroll
    for (int off = LPR; off < 64; off <<= 1) {
      const float mo = __shfl_xor(mx, off), lo = __shfl_xor(l, off);
      merge_ml(mx, l, mo, lo);
    }
    s0 = __shfl(s0, 0);
    // the positive joins: en = mass of the negatives, e0 = the positive's, both relative to mt
    const float mt = fmaxf(mx, s0);
    const float en = l * expf(mx - mt), e0 = expf(s0 - mt);
    const float inv = 1.f / (en + e0);
    if (lane == 0) lsum += mt == s0 ? log1pf(en) : (mt - s0) + logf(en + e0);
    // pass 2: scores -> c, by the lanes that wrote them
    if (sl < U) {
      for (int m = sl * EPW + sg; m < K1; m += EPW * U) {
        const float s = coef[base + m];
        const float p = m == 0 ? -(en * inv) : expf(s - mt) * inv;
        coef[base + m] = p * scale;
      }
    }
  }
  if (lane == 0) sl_loss[wave] = lsum;
  if (nbad) atomicAdd(&sl_bad, nbad);  // (an integer count: exact in any order)
  __syncthreads();
  if (tid == 0) {
    float s = 0.f;
    for (int k = 0; k < kWaves; ++k) s += sl_loss[k];
    block_loss[blockIdx.x] = s;
    block_bad[blockIdx.x] = sl_bad;
  }
}

// ordered sum of the block losses -> loss (mean), and the blocks' out-of-range counts -> *bad
__global__ void __launch_bounds__(1024) k_ssm_loss(const float* __restrict__ block_loss,
                                                   const int32_t* __restrict__ block_bad, int64_t nb, float denom,
                                                   float* __restrict__ loss, int32_t* __restrict__ bad) {
  __shared__ float red[1024];
  __shared__ int redb[1024];
  float s = 0.f;
  int c = 0;
  for (int64_t b = threadIdx.x; b < nb; b += 1024) {
    s += block_loss[b];
    c += block_bad[b];
  }
  red[threadIdx.x] = s;
  redb[threadIdx.x] = c;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      red[threadIdx.x] += red[threadIdx.x + w];
      redb[threadIdx.x] += redb[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    loss[0] = red[0] / denom;
    if (bad != nullptr) bad[0] = redb[0];
  }
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------
// sort keys of both sides, and the touched-row map cleared (16 B per thread; the region is a
// multiple of 16 B), set by the sorts' last passes
__global__ void k_ssm_keys(const int64_t* __restrict__ u, const int64_t* __restrict__ cand, int64_t S, int64_t R,
                           int64_t n_users, int64_t n_items, int64_t n_rows, int32_t* __restrict__ ikey,
                           int32_t* __restrict__ ival, int32_t* __restrict__ ukey, int32_t* __restrict__ uval,
                           uint8_t* __restrict__ touched) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c * 16 < n_rows) *reinterpret_cast<uint4*>(touched + c * 16) = make_uint4(0u, 0u, 0u, 0u);
  if (c < R) {
    ikey[c] = (int32_t)(n_users + clamp_idx(cand[c], n_items));
    ival[c] = (int32_t)c;
  }
  if (c < S) {
    ukey[c] = (int32_t)clamp_idx(u[c], n_users);
    uval[c] = (int32_t)c;
  }
}

constexpr int kChunk = 32;

// The record array of one side, position p in [0, R):
//   item side  (skey[p], sval[p]) = (row, record t K1 + m), sorted;      source = row of u_t
//   user side  (skey[q], sval[q]) = (row u_t, sample t), sorted, q = p / K1, m = p % K1;
//              source = row of cand[t, m]
struct Recs {
  const int32_t* skey;
  const int32_t* sval;
  const int64_t* u;
  const int64_t* cand;
  const float* coef;
  int64_t n_users, n_items;
  uint32_t K1;
};

template <bool USER>
__device__ __forceinline__ int32_t rec_dst(const Recs& r, int64_t p) {
  return USER ? r.skey[(uint32_t)p / r.K1] : r.skey[p];
}

template <bool USER>
__device__ __forceinline__ void rec_load(const Recs& r, int64_t p, int32_t& dst, int32_t& src, float& cf) {
  if (USER) {
    const uint32_t q = (uint32_t)p / r.K1, m = (uint32_t)p - q * r.K1;
    const int64_t rec = (int64_t)r.sval[q] * r.K1 + m;
    dst = r.skey[q];
    src = (int32_t)(r.n_users + clamp_idx(r.cand[rec], r.n_items));
    cf = r.coef[rec];
  } else {
    const int32_t rec = r.sval[p];
    dst = r.skey[p];
    src = (int32_t)clamp_idx(r.u[(uint32_t)rec / r.K1], r.n_users);
    cf = r.coef[rec];
  }
}

// chunk pass: a subgroup owns 32 consecutive records.  Segments (runs of one destination row)
// complete inside the chunk are written to dZ; one touching the chunk start while continuing
// from the previous chunk goes to slot "head"; one touching the chunk end and continuing goes
// to slot "tail".
template <int C, bool USER>
__global__ void __launch_bounds__(256) k_ssm_chunks(Recs r, int64_t total, const float* __restrict__ grad_loss,
                                                    const float* __restrict__ Z, float* __restrict__ dZ,
                                                    float* __restrict__ slots) {
  constexpr int LPR = Geo<C>::LPR, SPB = Geo<C>::SPB;
  __shared__ int32_t s_src[SPB][kChunk];
  __shared__ int32_t s_dst[SPB][kChunk];
  __shared__ float s_cf[SPB][kChunk];
  const int tid = threadIdx.x;
  const int sg = tid / LPR, sl = tid % LPR;
  const int64_t ch = (int64_t)blockIdx.x * SPB + sg;
  const int64_t b0 = ch * kChunk;
  const float g = grad_loss[0];
  if (b0 < total) {
    for (int q = sl; q < kChunk; q += LPR) {
      const int64_t p = b0 + q;
      int32_t src = 0, dst = -1;
      float cf = 0.f;
      if (p < total) rec_load<USER>(r, p, dst, src, cf);
      s_src[sg][q] = src;
      s_dst[sg][q] = dst;
      s_cf[sg][q] = cf * g;
    }
  }
  __syncthreads();
  if (b0 >= total) return;
  const int len = (int)min((int64_t)kChunk, total - b0);
  const bool starts_before = b0 > 0 && rec_dst<USER>(r, b0 - 1) == s_dst[sg][0];
  const bool ends_after = b0 + len < total && rec_dst<USER>(r, b0 + len) == s_dst[sg][len - 1];
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  int seg_start = 0;
  constexpr int UB = 8;  // source rows in flight per subgroup
  for (int q0 = 0; q0 < len; q0 += UB) {
    float4 v[UB];
#pragma unroll
    for (int k = 0; k < UB; ++k) {
      const int q = q0 + k;
      v[k] = q < len ? ld4(Z + (int64_t)s_src[sg][q] * C + sl * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
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

// fix-up: the chunk in which a chunk-spanning segment starts sums its tail slot and the head
// slots of the following chunks, in chunk order, and writes the row
template <int C, bool USER>
__global__ void __launch_bounds__(256) k_ssm_fixup(Recs r, int64_t total, const float* __restrict__ slots,
                                                   float* __restrict__ dZ) {
  constexpr int LPR = Geo<C>::LPR, SPB = Geo<C>::SPB;
  const int sg = threadIdx.x / LPR, sl = threadIdx.x % LPR;
  const int64_t ch = (int64_t)blockIdx.x * SPB + sg;
  const int64_t b0 = ch * kChunk;
  if (b0 >= total) return;
  const int64_t b1 = min(b0 + kChunk, total);
  if (b1 >= total) return;
  const int32_t row = rec_dst<USER>(r, b1 - 1);
  if (rec_dst<USER>(r, b1) != row) return;                                          // does not continue
  if (rec_dst<USER>(r, b0) == row && b0 > 0 && rec_dst<USER>(r, b0 - 1) == row) return;  // started earlier
  float4 acc = ld4(slots + (ch * 2 + 1) * C + sl * 4);
  for (int64_t c2 = ch + 1;; ++c2) {
    const int64_t e0 = c2 * kChunk;
    const int64_t e1 = min(e0 + kChunk, total);
    acc = add4(acc, ld4(slots + (c2 * 2 + 0) * C + sl * 4));
    if (!(rec_dst<USER>(r, e1 - 1) == row && e1 < total && rec_dst<USER>(r, e1) == row)) break;
  }
  st4(dZ + (int64_t)row * C + sl * 4, acc);
}

// rows no record reaches
template <int C>
__global__ void __launch_bounds__(256) k_ssm_zero_untouched(const uint8_t* __restrict__ touched, int64_t n_rows,
                                                            float* __restrict__ dZ) {
  constexpr int LPR = Geo<C>::LPR, SPB = Geo<C>::SPB;
  const int sg = threadIdx.x / LPR, sl = threadIdx.x % LPR;
  for (int64_t row = (int64_t)blockIdx.x * SPB + sg; row < n_rows; row += (int64_t)gridDim.x * SPB)
    if (!touched[row]) st4(dZ + row * C + sl * 4, make_float4(0.f, 0.f, 0.f, 0.f));
}

#define PPGAT_DISPATCH_SSM_C(C_, ...)                          \
  switch (C_) {                                                \
    case 32: { constexpr int CC = 32; __VA_ARGS__; break; }    \
    case 64: { constexpr int CC = 64; __VA_ARGS__; break; }    \
    case 128: { constexpr int CC = 128; __VA_ARGS__; break; }  \
    case 256: { constexpr int CC = 256; __VA_ARGS__; break; }  \
    default: return hipErrorInvalidValue;                      \
  }

// fixed grid (a function of S only): <= 16384 block partials for the one-block loss sum
int64_t ssm_fwd_blocks(int64_t S) {
  const int64_t b = (S + kWaves - 1) / kWaves;
  return b < 16384 ? b : 16384;
}

// workspace: forward block partials (loss | bad) | item keys, vals and their ping-pong pair [R]
// each | user keys, vals and pair [S] each | slots [chunks][2][C] | radix sort | touched [N]
struct SsmWs {
  float* block_loss;
  int32_t* block_bad;
  int32_t* ik[2];
  int32_t* iv[2];
  int32_t* uk[2];
  int32_t* uv[2];
  float* slots;
  void* tmp;
  uint8_t* touched;
  size_t bytes;
};

SsmWs ssm_ws(void* ws, int64_t N, int64_t S, int K1, int C) {
  const int64_t R = S * K1 > 0 ? S * K1 : 1, S1 = S > 0 ? S : 1;
  const int64_t chunks = (R + kChunk - 1) / kChunk;
  const unsigned bits = key_bits(N + 1);
  char* p = static_cast<char*>(ws);
  size_t o = 0;
  SsmWs w;
  w.block_loss = reinterpret_cast<float*>(p + o);
  w.block_bad = reinterpret_cast<int32_t*>(p + o) + ssm_fwd_blocks(S1);
  o += align_up((size_t)ssm_fwd_blocks(S1) * 8);
  const size_t r4 = align_up((size_t)R * 4), s4 = align_up((size_t)S1 * 4);
  for (int k = 0; k < 2; ++k) {
    w.ik[k] = reinterpret_cast<int32_t*>(p + o); o += r4;
    w.iv[k] = reinterpret_cast<int32_t*>(p + o); o += r4;
  }
  for (int k = 0; k < 2; ++k) {
    w.uk[k] = reinterpret_cast<int32_t*>(p + o); o += s4;
    w.uv[k] = reinterpret_cast<int32_t*>(p + o); o += s4;
  }
  w.slots = reinterpret_cast<float*>(p + o);
  o += align_up((size_t)chunks * 2 * C * 4);
  w.tmp = p + o;
  const size_t ta = rs_workspace_bytes(R, bits), tb = rs_workspace_bytes(S1, bits);
  o += ta > tb ? ta : tb;
  w.touched = reinterpret_cast<uint8_t*>(p + o);
  o += align_up((size_t)N + 16);
  w.bytes = o;
  return w;
}

}  // namespace

size_t ssm_workspace_bytes(int64_t N, int64_t S, int K1, int C) { return ssm_ws(nullptr, N, S, K1, C).bytes; }

hipError_t ssm_fwd(const float* Z, int64_t n_users, int64_t n_items, int C, const int64_t* u, const int64_t* cand,
                   const float* corr, int64_t S, int K1, float tau, float* loss, float* coef, int32_t* bad, void* ws,
                   hipStream_t st) {
  const SsmWs w = ssm_ws(ws, n_users + n_items, S, K1, C);
  const int64_t nb = ssm_fwd_blocks(S);
  if (S > 0 && corr != nullptr) {
    PPGAT_DISPATCH_SSM_C(C, hipLaunchKernelGGL((k_ssm_fwd<CC, true>), dim3((unsigned)nb), dim3(256), 0, st, Z, n_users,
                                               n_items, u, cand, corr, S, K1, tau, coef, w.block_loss, w.block_bad));
  } else if (S > 0) {
    PPGAT_DISPATCH_SSM_C(C, hipLaunchKernelGGL((k_ssm_fwd<CC, false>), dim3((unsigned)nb), dim3(256), 0, st, Z, n_users,
                                               n_items, u, cand, corr, S, K1, tau, coef, w.block_loss, w.block_bad));
  }
  hipLaunchKernelGGL(k_ssm_loss, dim3(1), dim3(1024), 0, st, w.block_loss, w.block_bad, S > 0 ? nb : 0,
                     S > 0 ? (float)S : 1.f, loss, bad);
  return hipGetLastError();
}

hipError_t ssm_bwd(const float* Z, int64_t n_users, int64_t n_items, int C, const int64_t* u, const int64_t* cand,
                   int64_t S, int K1, const float* coef, const float* grad_loss, float* dZ, void* ws,
                   hipStream_t st) {
  const int64_t N = n_users + n_items;
  if (S == 0) return hipMemsetAsync(dZ, 0, (size_t)N * C * 4, st);
  const SsmWs w = ssm_ws(ws, N, S, K1, C);
  const int64_t R = S * K1;
  const unsigned bits = key_bits(N + 1);
  const int64_t kthreads = R > (N + 15) / 16 ? R : (N + 15) / 16;  // (enough threads to clear the map)
  hipLaunchKernelGGL(k_ssm_keys, dim3((unsigned)((kthreads + 255) / 256)), dim3(256), 0, st, u, cand, S, R, n_users,
                     n_items, N, w.ik[0], w.iv[0], w.uk[0], w.uv[0], w.touched);
  bool i1 = false, u1 = false;
  hipError_t e = rs_sort(w.ik[0], w.iv[0], w.ik[1], w.iv[1], R, bits, w.tmp, &i1, st, w.touched, N);
  if (e != hipSuccess) return e;
  e = rs_sort(w.uk[0], w.uv[0], w.uk[1], w.uv[1], S, bits, w.tmp, &u1, st, w.touched, N);
  if (e != hipSuccess) return e;
  const Recs ri{w.ik[i1], w.iv[i1], u, cand, coef, n_users, n_items, (uint32_t)K1};
  const Recs ru{w.uk[u1], w.uv[u1], u, cand, coef, n_users, n_items, (uint32_t)K1};
  const int64_t chunks = (R + kChunk - 1) / kChunk;
  PPGAT_DISPATCH_SSM_C(C, {
    constexpr int SPB = Geo<CC>::SPB;
    const unsigned g = (unsigned)((chunks + SPB - 1) / SPB);
    // the two sides one after the other on the stream: they share the slots
    hipLaunchKernelGGL((k_ssm_chunks<CC, true>), dim3(g), dim3(256), 0, st, ru, R, grad_loss, Z, dZ, w.slots);
    hipLaunchKernelGGL((k_ssm_fixup<CC, true>), dim3(g), dim3(256), 0, st, ru, R, w.slots, dZ);
    hipLaunchKernelGGL((k_ssm_chunks<CC, false>), dim3(g), dim3(256), 0, st, ri, R, grad_loss, Z, dZ, w.slots);
    hipLaunchKernelGGL((k_ssm_fixup<CC, false>), dim3(g), dim3(256), 0, st, ri, R, w.slots, dZ);
    int64_t gz = (N + SPB - 1) / SPB;
    if (gz > 4096) gz = 4096;
    hipLaunchKernelGGL(k_ssm_zero_untouched<CC>, dim3((unsigned)gz), dim3(256), 0, st, w.touched, N, dZ);
  });
  return hipGetLastError();
}

}  // namespace ppgat
