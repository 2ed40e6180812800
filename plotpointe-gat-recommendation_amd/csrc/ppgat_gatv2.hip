// ppgat_gatv2.hip -- fused GATv2 (dynamic attention) layer for CDNA4 (gfx950, MI355X).
//
// Replaces torch_geometric.nn.GATv2Conv (concat=False, add_self_loops=False, no edge features)
// after its two projections x_l = lin_l(x), x_r = lin_r(x), both [N, H, C]:
//   t_ij   = x_l[j] + x_r[i]                                    per edge j -> i and head
//   e_ij   = sum_c att[h, c] * leaky_relu(t_ij[c])
//   alpha  = exp(e_ij - max_i) / (sum_in-edges exp(e - max_i) + 1e-16)
//   out_i  = mean_h sum_j mask_ij alpha_ij x_l[j] + bias        (mask: the dropout multiplier)
// Unlike GAT v1 (ppgat_kernels.hip) the logit does not separate into two per-node scalars: it
// is a C-wide LeakyReLU and dot product per edge and head, and its gradient is a C-wide row to
// both endpoints of every edge.
//
// Layout: a node row of H * C floats is C/4 lanes ("subgroup") x H float4 -- lane sl holds the
// columns [4 sl, 4 sl + 4) of every head -- so the per-head dot products reduce over the lanes
// of one subgroup with DPP / permlane steps (ppgat_lanes.h) and never touch LDS.  The 64/(C/4)
// subgroups of a wave take different edges of the same item, U gathered rows in flight each.
//   forward        one wave per item of the CSR-by-destination schedule; x_r[i] in registers,
//                  x_l[j] gathered once per edge for logit and message; one online softmax
//                  state (m, l, acc) per subgroup and head, merged across subgroups at the end;
//                  hub pieces leave (m, l, acc) in the workspace, merged in piece order.
//   backward       a sweep by destination that forms D_i = sum_j alpha_ij dalpha_ij edge by edge
//                  (see below) and packs the node state, then one pass by source over the CSC
//                  schedule (owns dx_l[j]; gathers g_i, x_r[i] and {m, inv_l, D} of the
//                  destination) and one by destination over the CSR schedule (owns dx_r[i];
//                  gathers x_l[j] again and recomputes de_ij from g_i . x_l[j], both operands
//                  being at hand).  datt rides in the destination pass: a fixed grid of waves
//                  strides over the items, each block leaves one partial row, and the rows are
//                  summed in block order (launch_col_reduce); dbias likewise from a row sweep.
// D is NOT taken from the identity D_i = g_i . agg_i / H that the v1 kernels use.  de_ij =
// alpha (dalpha - D) cancels: a destination with one in-edge has alpha = 1 and D = dalpha, so
// de = 0.  With D summed from the very dalpha values the edge passes recompute (same operands,
// same order, same bits) that cancellation is exact; with g . agg it leaves the rounding of a
// C-wide dot product that itself cancels, which on the test graph reached 1.2e-5 of the row's
// term scale (bound 1e-5).  The price is one more gather of x_l per edge in the backward.
// No float atomics: every sum is owned by one wave in a fixed order, so two launches give the
// same bits.  Contraction is off in this file and every fused multiply-add is written as fmaf,
// so the -O1 debug objects round exactly as the -O3 ones.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "ppgat_internal.h"
#include "ppgat_lanes.h"

#pragma clang fp contract(off)

#include "ppgat_device.h"  // after the pragma: its mul4 / add4 must not contract to FMAs here either

namespace ppgat {
namespace {

// lrelu per component
__device__ __forceinline__ float4 leaky4(float4 t, float slope) {
  return make_float4(lrelu(t.x, slope), lrelu(t.y, slope), lrelu(t.z, slope), lrelu(t.w, slope));
}
// de * att (.) leaky'(t)
__device__ __forceinline__ float4 dleaky4(float de, float4 att, float4 t, float slope) {
  const float4 c = mul4(att, de);
  return make_float4(t.x > 0.f ? c.x : c.x * slope, t.y > 0.f ? c.y : c.y * slope, t.z > 0.f ? c.z : c.z * slope,
                     t.w > 0.f ? c.w : c.w * slope);
}

template <int H, int C>
struct Geo {
  static constexpr int LPR = C / 4;     // lanes per row piece (one float4 per head each)
  static constexpr int EPW = 64 / LPR;  // edges side by side per wave
  static constexpr int U = (8 / (EPW * H)) >= 1 ? 8 / (EPW * H) : 1;  // gathered rows in flight per subgroup
  static constexpr int W = H * C;       // floats per node row
  static_assert(C == 32 || C == 64 || C == 128, "gatv2: C in {32, 64, 128}");
  static_assert(H == 1 || H == 2 || H == 4, "gatv2: H in {1, 2, 4}");
};

// online-softmax merge of (mo, lo, ao) into (m, l, a); -inf marks a state without edges
__device__ __forceinline__ void merge_state(float& m, float& l, float4& a, float mo, float lo, float4 ao) {
  const float mn = fmaxf(m, mo);
  const float ms = mn == -INFINITY ? 0.f : mn;
  const float s1 = expf(m - ms), s2 = expf(mo - ms);
  l = fmaf(l, s1, lo * s2);
  a = fma4(s1, a, mul4(ao, s2));
  m = mn;
}

struct FwdArgs {
  const float* xl;
  const float* xr;
  const float* att;
  const float* bias;     // nullable
  float slope, p, inv_keep;
  const uint64_t* seed;  // device slot, read when p > 0
  float* out;
  float* m;
  float* invl;
  float* partial;        // hub pieces: per (item, head) [acc C | m | l | pad pad]
};

constexpr float kEps = 1e-16f;

// out / m / inv_l of one finished destination row; lanes of subgroup 0 store
template <int H, int C>
__device__ __forceinline__ void fwd_finish(const FwdArgs& a, int64_t i, int sl, bool writer, bool first,
                                           bool has_edges, const float (&m)[H], const float (&l)[H],
                                           const float4 (&acc)[H]) {
  float4 osum = f4(0.f);
#pragma unroll
  for (int h = 0; h < H; ++h) {
    const float invl = 1.f / (l[h] + kEps);
    osum = add4(osum, mul4(acc[h], invl));
    if (first) {
      a.m[i * H + h] = has_edges ? m[h] : 0.f;
      a.invl[i * H + h] = invl;
    }
  }
  if (H > 1) osum = mul4(osum, 1.f / (float)H);
  if (a.bias != nullptr) osum = add4(osum, ld4(a.bias + sl * 4));
  if (writer) st4(a.out + i * C + sl * 4, osum);
}

// one wave per item: a destination row or a hub piece
template <int H, int C>
__global__ void __launch_bounds__(256) k_v2_fwd(Items it, const int32_t* __restrict__ col,
                                                const int32_t* __restrict__ eid, FwdArgs a) {
  using G = Geo<H, C>;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t w = (int64_t)blockIdx.x * 4 + wv;
  if (w >= it.n_items) return;  // wave-uniform
  const int sg = lane / G::LPR, sl = lane % G::LPR;
  const int64_t i = it.row[w];
  const int rs = it.beg[w], re = it.end[w];
  const bool drop = a.p > 0.f;
  const uint64_t seed = drop ? a.seed[0] : 0;
  float4 xr[H], at[H], acc[H];
  float m[H], l[H];
#pragma unroll
  for (int h = 0; h < H; ++h) {
    xr[h] = ld4(a.xr + (i * H + h) * C + sl * 4);
    at[h] = ld4(a.att + h * C + sl * 4);
    acc[h] = f4(0.f);
    m[h] = -INFINITY;
    l[h] = 0.f;
  }
  for (int k0 = rs; k0 < re; k0 += G::EPW * G::U) {  // wave-uniform trip count
    float4 v[G::U][H];
    int ed[G::U];
    bool ok[G::U];
#pragma unroll
    for (int u = 0; u < G::U; ++u) {
      const int k = k0 + u * G::EPW + sg;
      ok[u] = k < re;
      const int64_t j = ok[u] ? col[k] : 0;
      ed[u] = (drop && ok[u]) ? eid[k] : 0;
#pragma unroll
      for (int h = 0; h < H; ++h) v[u][h] = ok[u] ? ld4(a.xl + (j * H + h) * C + sl * 4) : f4(0.f);
    }
#pragma unroll
    for (int u = 0; u < G::U; ++u) {
#pragma unroll
      for (int h = 0; h < H; ++h) {
        const float4 lr = leaky4(add4(v[u][h], xr[h]), a.slope);
        float e = group_reduce<Op::Sum, 1, G::LPR / 2>(dot4(at[h], lr));
        if (!ok[u]) e = -INFINITY;
        const float mn = fmaxf(m[h], e);
        const float ms = mn == -INFINITY ? 0.f : mn;
        const float sc = expf(m[h] - ms), pe = expf(e - ms);
        l[h] = fmaf(l[h], sc, pe);
        float pw = pe;
        if (drop) pw *= drop_scale(seed, (uint32_t)ed[u], (uint32_t)h, a.p, a.inv_keep);
        acc[h] = fma4(pw, v[u][h], mul4(acc[h], sc));
        m[h] = mn;
      }
    }
  }
  // subgroup states -> subgroup 0 (fixed butterfly order)
#pragma unroll
  for (int off = G::LPR; off < 64; off <<= 1) {
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const float mo = __shfl_xor(m[h], off), lo = __shfl_xor(l[h], off);
      const float4 ao = shfl_xor4(acc[h], off);
      merge_state(m[h], l[h], acc[h], mo, lo, ao);
    }
  }
  if (w < it.n_hub_items) {
#pragma unroll
    for (int h = 0; h < H; ++h) {
      float* slot = a.partial + (w * H + h) * (C + 4);
      if (sg == 0) st4(slot + sl * 4, acc[h]);
      if (lane == 0) st4(slot + C, make_float4(m[h], l[h], 0.f, 0.f));
    }
    return;
  }
  fwd_finish<H, C>(a, i, sl, sg == 0, lane == 0, re > rs, m, l, acc);
}

// the pieces of one hub row merged in piece order; one wave per hub, its first subgroup works
template <int H, int C>
__global__ void __launch_bounds__(256) k_v2_fwd_merge(const int32_t* __restrict__ hub_row,
                                                      const int32_t* __restrict__ hub_ptr, int64_t n_hubs,
                                                      FwdArgs a) {
  using G = Geo<H, C>;
  const int lane = threadIdx.x & 63;
  const int64_t hb = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (hb >= n_hubs || lane >= G::LPR) return;  // no cross-lane step below
  const int64_t i = hub_row[hb];
  const int p0 = hub_ptr[hb], p1 = hub_ptr[hb + 1];
  float m[H], l[H];
  float4 acc[H];
#pragma unroll
  for (int h = 0; h < H; ++h) {
    m[h] = -INFINITY;
    l[h] = 0.f;
    acc[h] = f4(0.f);
    for (int q = p0; q < p1; ++q) {
      const float* slot = a.partial + ((int64_t)q * H + h) * (C + 4);
      merge_state(m[h], l[h], acc[h], slot[C], slot[C + 1], ld4(slot + lane * 4));
    }
  }
  fwd_finish<H, C>(a, i, lane, true, lane == 0, p1 > p0, m, l, acc);
}

// ---------------------------------------------------------------------------
// Attention weights (ppgat_dynatt_attention): alpha = exp(e_ij - m_i) inv_l_i per edge and head,
// before the dropout mask, from the forward's final state.  x_l[j] is gathered per edge and the
// logit formed exactly as k_v2_fwd forms it (x_l[j] + x_r[i], leaky, dot with att, the same
// subgroup reduction), so e <= m and a destination's largest weight is inv_l bit for bit.  One
// wave per item, a hub piece being just another item; after the reduction every lane of a
// subgroup holds every head's logit, and lane h of the subgroup stores head h.
// ---------------------------------------------------------------------------
struct AttnArgs {
  const float* xl;
  const float* xr;
  const float* att;
  const float* m;
  const float* invl;
  float slope;
  int scatter;  // alpha at eid[k] (the caller's edge order) instead of at slot k
  float* alpha;
};

template <int H, int C>
__global__ void __launch_bounds__(256) k_v2_attn(Items it, const int32_t* __restrict__ col,
                                                 const int32_t* __restrict__ eid, AttnArgs a) {
  using G = Geo<H, C>;
  static_assert(H <= G::LPR, "one lane of a subgroup per head");
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t w = (int64_t)blockIdx.x * 4 + wv;
  if (w >= it.n_items) return;  // wave-uniform
  const int sg = lane / G::LPR, sl = lane % G::LPR;
  const int64_t i = it.row[w];
  const int rs = it.beg[w], re = it.end[w];
  float4 xr[H], at[H];
  float mi[H], il[H];
#pragma unroll
  for (int h = 0; h < H; ++h) {
    xr[h] = ld4(a.xr + (i * H + h) * C + sl * 4);
    at[h] = ld4(a.att + h * C + sl * 4);
    mi[h] = a.m[i * H + h];
    il[h] = a.invl[i * H + h];
  }
  for (int k0 = rs; k0 < re; k0 += G::EPW * G::U) {  // wave-uniform trip count
    float4 v[G::U][H];
    int64_t o[G::U];
    bool ok[G::U];
#pragma unroll
    for (int u = 0; u < G::U; ++u) {
      const int k = k0 + u * G::EPW + sg;
      ok[u] = k < re;
      const int64_t j = ok[u] ? col[k] : 0;
      o[u] = ok[u] ? (a.scatter ? eid[k] : k) : 0;
#pragma unroll
      for (int h = 0; h < H; ++h) v[u][h] = ok[u] ? ld4(a.xl + (j * H + h) * C + sl * 4) : f4(0.f);
    }
#pragma unroll
    for (int u = 0; u < G::U; ++u) {
      float mine = 0.f;
#pragma unroll
      for (int h = 0; h < H; ++h) {
        const float4 lr = leaky4(add4(v[u][h], xr[h]), a.slope);
        const float e = group_reduce<Op::Sum, 1, G::LPR / 2>(dot4(at[h], lr));
        const float al = expf(e - mi[h]) * il[h];
        if (sl == h) mine = al;
      }
      if (ok[u] && sl < H) a.alpha[o[u] * H + sl] = mine;
    }
  }
}

// ---------------------------------------------------------------------------
// dbias: the block partial column sums of g in a fixed order (rows side by side within a block,
// the block's waves in wave order, blocks by launch_col_reduce).
// ---------------------------------------------------------------------------
template <int C>
__global__ void __launch_bounds__(256) k_v2_bias_part(const float* __restrict__ g, int64_t n,
                                                      float* __restrict__ bias_part) {
  constexpr int LPR = C / 4, SPB = 256 / LPR;
  __shared__ float4 red[4][LPR];
  const int sgb = threadIdx.x / LPR, sl = threadIdx.x % LPR;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float4 bsum = f4(0.f);
  for (int64_t n0 = (int64_t)blockIdx.x * SPB; n0 < n; n0 += (int64_t)gridDim.x * SPB) {  // block-uniform
    const int64_t nd = n0 + sgb;
    if (nd < n) bsum = add4(bsum, ld4(g + nd * C + sl * 4));
  }
  bsum = across_subgroups<LPR>(bsum);
  if (lane < LPR) red[wv][lane] = bsum;
  __syncthreads();
  if (threadIdx.x < LPR) {
    float4 t = red[0][threadIdx.x];
    for (int q = 1; q < 4; ++q) t = add4(t, red[q][threadIdx.x]);
    st4(bias_part + (int64_t)blockIdx.x * C + threadIdx.x * 4, t);
  }
}

struct BwdArgs {
  const float* xl;
  const float* xr;
  const float* att;
  const float* g;        // grad_out [N, C]
  const float* m;        // [N, H] the forward's softmax state
  const float* invl;
  float4* nstate;        // [N, H] {m, inv_l, D, 0}: written by the D sweep, read by the two passes
  float slope, p, inv_keep;
  const uint64_t* seed;
  float* dx;             // SRC: grad x_l, else grad x_r; [N, H * C]
  float* partial;        // hub pieces' partial rows [n_hub_items, H * C]
  float* att_part;       // destination pass: [gridDim.x, H * C]
  float* d_part;         // D sweep: the hub pieces' partial sums [n_hub_items, H]
};

constexpr int kSrc = 0, kDst = 1, kDsum = 2;

// Edge pass of the backward over a fixed grid of waves striding the items.
//   kSrc  items are source rows j (CSC schedule): own x_l[j]; per edge gather g_i, x_r[i], nstate_i
//         dx_l[j] = sum_i (mask alpha / H) g_i + dt_ij
//   kDst  items are destination rows i (CSR schedule): own x_r[i], g_i, nstate_i; gather x_l[j]
//         dx_r[i] = sum_j dt_ij,  datt += de_ij leaky(t_ij)
//   kDsum the destination sweep that runs first: D_i = sum_j alpha_ij dalpha_ij -> nstate_i
// with dalpha = mask (g_i . x_l[j]) / H, de = alpha (dalpha - D_i), dt = de att (.) leaky'(t).
// Every mode forms e_ij and dalpha_ij from the same operands in the same order.
template <int H, int C, int MODE>
__global__ void __launch_bounds__(256) k_v2_bwd(Items it, const int32_t* __restrict__ idx,
                                                const int32_t* __restrict__ eid, BwdArgs a) {
  using G = Geo<H, C>;
  constexpr bool SRC = MODE == kSrc, DSUM = MODE == kDsum;
  constexpr int U = SRC ? (G::U > 1 ? G::U / 2 : 1) : G::U;  // the source pass gathers two rows per edge
  __shared__ float4 red[4][H * G::LPR];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int sg = lane / G::LPR, sl = lane % G::LPR;
  const bool drop = a.p > 0.f;
  const uint64_t seed = drop ? a.seed[0] : 0;
  const float inv_h = 1.f / (float)H;
  const float* own_tab = SRC ? a.xl : a.xr;
  const float* oth_tab = SRC ? a.xr : a.xl;
  float4 at[H], datt[H];
#pragma unroll
  for (int h = 0; h < H; ++h) {
    at[h] = ld4(a.att + h * C + sl * 4);
    datt[h] = f4(0.f);
  }
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (int64_t w = (int64_t)blockIdx.x * 4 + wv; w < it.n_items; w += stride) {  // wave-uniform
    const int64_t r = it.row[w];
    const int rs = it.beg[w], re = it.end[w];
    float4 own[H], dx[H], ns_own[H];
    float dsum[H];
    float4 g_own = f4(0.f);
#pragma unroll
    for (int h = 0; h < H; ++h) {
      own[h] = ld4(own_tab + (r * H + h) * C + sl * 4);
      dx[h] = f4(0.f);
      dsum[h] = 0.f;
      ns_own[h] = f4(0.f);
      if (MODE == kDst) ns_own[h] = a.nstate[r * H + h];
      if (DSUM) ns_own[h] = make_float4(a.m[r * H + h], a.invl[r * H + h], 0.f, 0.f);
    }
    if (!SRC) g_own = ld4(a.g + r * C + sl * 4);
    for (int k0 = rs; k0 < re; k0 += G::EPW * U) {
      float4 v[U][H], nsv[U][H], gv[U];
      int ed[U];
      bool ok[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int k = k0 + u * G::EPW + sg;
        ok[u] = k < re;
        const int64_t o = ok[u] ? idx[k] : 0;
        ed[u] = (drop && ok[u]) ? eid[k] : 0;
        gv[u] = f4(0.f);
        if (SRC && ok[u]) gv[u] = ld4(a.g + o * C + sl * 4);
#pragma unroll
        for (int h = 0; h < H; ++h) {
          v[u][h] = ok[u] ? ld4(oth_tab + (o * H + h) * C + sl * 4) : f4(0.f);
          nsv[u][h] = f4(0.f);
          if (SRC && ok[u]) nsv[u][h] = a.nstate[o * H + h];
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int h = 0; h < H; ++h) {
          const float4 xlv = SRC ? own[h] : v[u][h];
          const float4 gg = SRC ? gv[u] : g_own;
          const float4 st = SRC ? nsv[u][h] : ns_own[h];
          const float4 t = SRC ? add4(own[h], v[u][h]) : add4(v[u][h], own[h]);  // x_l[j] + x_r[i]
          const float4 lr = leaky4(t, a.slope);
          const float e = group_reduce<Op::Sum, 1, G::LPR / 2>(dot4(at[h], lr));
          const float gx = group_reduce<Op::Sum, 1, G::LPR / 2>(dot4(gg, xlv));
          const float alpha = ok[u] ? expf(e - st.x) * st.y : 0.f;
          const float mask = drop ? drop_scale(seed, (uint32_t)ed[u], (uint32_t)h, a.p, a.inv_keep) : 1.f;
          float dal = mask * gx;
          if (H > 1) dal *= inv_h;
          if (DSUM) {
            dsum[h] = fmaf(alpha, dal, dsum[h]);
            continue;
          }
          const float de = alpha * (dal - st.z);
          dx[h] = add4(dx[h], dleaky4(de, at[h], t, a.slope));
          if (SRC) {
            float wm = mask * alpha;
            if (H > 1) wm *= inv_h;
            dx[h] = fma4(wm, gg, dx[h]);
          } else {
            datt[h] = fma4(de, lr, datt[h]);
          }
        }
      }
    }
    if (DSUM) {
#pragma unroll
      for (int h = 0; h < H; ++h) {
        float d = dsum[h];  // uniform within a subgroup; subgroups added in butterfly order
#pragma unroll
        for (int off = G::LPR; off < 64; off <<= 1) d += __shfl_xor(d, off);
        if (lane == 0) {
          if (w < it.n_hub_items) a.d_part[w * H + h] = d;
          else a.nstate[r * H + h] = make_float4(ns_own[h].x, ns_own[h].y, d, 0.f);
        }
      }
      continue;
    }
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const float4 s = across_subgroups<G::LPR>(dx[h]);
      if (sg == 0) {
        if (w < it.n_hub_items) st4(a.partial + (w * H + h) * C + sl * 4, s);
        else st4(a.dx + (r * H + h) * C + sl * 4, s);
      }
    }
  }
  if (MODE != kDst) return;
  // datt: subgroups, then the block's waves in wave order, one partial row per block
#pragma unroll
  for (int h = 0; h < H; ++h) {
    const float4 s = across_subgroups<G::LPR>(datt[h]);
    if (sg == 0) red[wv][h * G::LPR + sl] = s;
  }
  __syncthreads();
  if (threadIdx.x < H * G::LPR) {
    float4 s = red[0][threadIdx.x];
    for (int q = 1; q < 4; ++q) s = add4(s, red[q][threadIdx.x]);
    st4(a.att_part + ((int64_t)blockIdx.x * (H * G::LPR) + threadIdx.x) * 4, s);
  }
}

// hub rows of a backward pass: the pieces' partial rows added in piece order, one thread per float4
__global__ void __launch_bounds__(256) k_v2_row_merge(const int32_t* __restrict__ hub_row,
                                                      const int32_t* __restrict__ hub_ptr, int64_t n_hubs, int w4,
                                                      const float* __restrict__ partial, float* __restrict__ dx) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t hb = t / w4;
  const int c = (int)(t % w4);
  if (hb >= n_hubs) return;
  const int p0 = hub_ptr[hb], p1 = hub_ptr[hb + 1];
  float4 acc = f4(0.f);
  for (int q = p0; q < p1; ++q) acc = add4(acc, ld4(partial + ((int64_t)q * w4 + c) * 4));
  st4(dx + ((int64_t)hub_row[hb] * w4 + c) * 4, acc);
}

// D of the hub rows: the pieces' partial sums added in piece order, one thread per (hub, head)
__global__ void __launch_bounds__(256) k_v2_d_merge(const int32_t* __restrict__ hub_row,
                                                    const int32_t* __restrict__ hub_ptr, int64_t n_hubs, int H,
                                                    const float* __restrict__ d_part, const float* __restrict__ m,
                                                    const float* __restrict__ invl, float4* __restrict__ nstate) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t hb = t / H;
  const int h = (int)(t % H);
  if (hb >= n_hubs) return;
  float d = 0.f;
  for (int q = hub_ptr[hb]; q < hub_ptr[hb + 1]; ++q) d += d_part[(int64_t)q * H + h];
  const int64_t i = hub_row[hb];
  nstate[i * H + h] = make_float4(m[i * H + h], invl[i * H + h], d, 0.f);
}

constexpr int64_t kBwdBlocks = 2048;  // the fixed grid of the backward's edge passes (4 waves each)

inline unsigned bwd_grid(int64_t n_items) {
  int64_t b = (n_items + 3) / 4;
  if (b < 1) b = 1;
  if (b > kBwdBlocks) b = kBwdBlocks;
  return (unsigned)b;
}

struct Offsets {
  size_t nstate, bias_part, att_part, rows, d_part, total;
};

inline size_t up256(size_t x) { return (x + 255) & ~size_t(255); }

inline Offsets carve(int64_t n, int64_t src_hub_items, int64_t dst_hub_items, int H, int C) {
  Offsets o;
  size_t at = 0;
  o.nstate = at;
  at += up256((size_t)(n > 0 ? n : 1) * H * 16);
  o.bias_part = at;
  at += up256((size_t)epi_blocks(n) * C * 4);
  o.att_part = at;
  at += up256((size_t)kBwdBlocks * H * C * 4);
  o.rows = at;
  const int64_t hubs = src_hub_items > dst_hub_items ? src_hub_items : dst_hub_items;
  at += up256((size_t)(hubs > 0 ? hubs : 1) * H * C * 4);
  o.d_part = at;
  at += up256((size_t)(dst_hub_items > 0 ? dst_hub_items : 1) * H * 4);
  o.total = at;
  return o;
}

template <int H, int C>
hipError_t fwd_t(const ppgat_schedule& sch, const int32_t* col, const int32_t* eid, const FwdArgs& a,
                 hipStream_t st) {
  const Items its = items_of(sch, sch.n_items);
  hipLaunchKernelGGL((k_v2_fwd<H, C>), dim3((unsigned)((sch.n_items + 3) / 4)), dim3(256), 0, st, its, col, eid,
                     a);
  if (sch.n_hubs > 0)
    hipLaunchKernelGGL((k_v2_fwd_merge<H, C>), dim3((unsigned)((sch.n_hubs + 3) / 4)), dim3(256), 0, st,
                       sch.hub_row, sch.hub_ptr, sch.n_hubs, a);
  return hipGetLastError();
}

template <int H, int C>
hipError_t bwd_t(const ppgat_schedule& src, const ppgat_schedule& dst, const int32_t* row, const int32_t* csc_eid,
                 const int32_t* col, const int32_t* csr_eid, int64_t n,
                 BwdArgs a, float* dxl, float* dxr, float* datt, float* dbias, char* ws, hipStream_t st) {
  const Offsets o = carve(n, src.n_hub_items, dst.n_hub_items, H, C);
  float* bias_part = reinterpret_cast<float*>(ws + o.bias_part);
  a.nstate = reinterpret_cast<float4*>(ws + o.nstate);
  a.partial = reinterpret_cast<float*>(ws + o.rows);
  a.att_part = reinterpret_cast<float*>(ws + o.att_part);
  a.d_part = reinterpret_cast<float*>(ws + o.d_part);
  if (dbias != nullptr) {
    const int64_t pb = epi_blocks(n);
    hipLaunchKernelGGL((k_v2_bias_part<C>), dim3((unsigned)pb), dim3(256), 0, st, a.g, n, bias_part);
    hipError_t e = launch_col_reduce(bias_part, pb, C, C, dbias, nullptr, st);
    if (e != hipSuccess) return e;
  }
  constexpr int W4 = H * C / 4;
  const Items si = items_of(src, src.n_items);
  const Items di = items_of(dst, dst.n_items);
  const unsigned dgrid = bwd_grid(dst.n_items);
  a.dx = nullptr;
  hipLaunchKernelGGL((k_v2_bwd<H, C, kDsum>), dim3(dgrid), dim3(256), 0, st, di, col, csr_eid, a);
  if (dst.n_hubs > 0)
    hipLaunchKernelGGL(k_v2_d_merge, dim3((unsigned)((dst.n_hubs * H + 255) / 256)), dim3(256), 0, st,
                       dst.hub_row, dst.hub_ptr, dst.n_hubs, H, a.d_part, a.m, a.invl, a.nstate);
  a.dx = dxl;
  hipLaunchKernelGGL((k_v2_bwd<H, C, kSrc>), dim3(bwd_grid(src.n_items)), dim3(256), 0, st, si, row, csc_eid, a);
  if (src.n_hubs > 0)
    hipLaunchKernelGGL(k_v2_row_merge, dim3((unsigned)((src.n_hubs * W4 + 255) / 256)), dim3(256), 0, st,
                       src.hub_row, src.hub_ptr, src.n_hubs, W4, a.partial, dxl);
  a.dx = dxr;
  hipLaunchKernelGGL((k_v2_bwd<H, C, kDst>), dim3(dgrid), dim3(256), 0, st, di, col, csr_eid, a);
  if (dst.n_hubs > 0)
    hipLaunchKernelGGL(k_v2_row_merge, dim3((unsigned)((dst.n_hubs * W4 + 255) / 256)), dim3(256), 0, st,
                       dst.hub_row, dst.hub_ptr, dst.n_hubs, W4, a.partial, dxr);
  hipError_t e = launch_col_reduce(a.att_part, dgrid, H * C, H * C, datt, nullptr, st);
  if (e != hipSuccess) return e;
  return hipGetLastError();
}

#define PPGAT_V2_DISPATCH(H, C, CALL)                          \
  do {                                                         \
    if (H == 1 && C == 32) { constexpr int HH = 1, CC = 32; return CALL; }   \
    if (H == 1 && C == 64) { constexpr int HH = 1, CC = 64; return CALL; }   \
    if (H == 1 && C == 128) { constexpr int HH = 1, CC = 128; return CALL; } \
    if (H == 2 && C == 64) { constexpr int HH = 2, CC = 64; return CALL; }   \
    if (H == 2 && C == 128) { constexpr int HH = 2, CC = 128; return CALL; } \
    if (H == 4 && C == 64) { constexpr int HH = 4, CC = 64; return CALL; }   \
    if (H == 4 && C == 128) { constexpr int HH = 4, CC = 128; return CALL; } \
    return hipErrorInvalidValue;                               \
  } while (0)

}  // namespace

bool gatv2_shape_ok(int H, int C) {
  return (H == 1 && (C == 32 || C == 64 || C == 128)) || ((H == 2 || H == 4) && (C == 64 || C == 128));
}

size_t gatv2_fwd_workspace_bytes(int64_t n_hub_items, int H, int C) {
  return up256((size_t)(n_hub_items > 0 ? n_hub_items : 1) * H * (C + 4) * 4);
}

size_t gatv2_bwd_workspace_bytes(int64_t n, int64_t src_hub_items, int64_t dst_hub_items, int H, int C) {
  return carve(n, src_hub_items, dst_hub_items, H, C).total;
}

hipError_t gatv2_fwd(const ppgat_schedule& sch, const int32_t* col, const int32_t* eid, int H, int C,
                     const float* xl, const float* xr, const float* att, const float* bias, float slope, float p,
                     const uint64_t* seed, float* out, float* m, float* invl, float* partial, hipStream_t st) {
  if (sch.n_items <= 0) return hipSuccess;
  const FwdArgs a{xl, xr, att, bias, slope, p, p > 0.f ? 1.f / (1.f - p) : 1.f, seed, out, m, invl, partial};
  PPGAT_V2_DISPATCH(H, C, (fwd_t<HH, CC>(sch, col, eid, a, st)));
}

namespace {
template <int H, int C>
hipError_t attn_t(const ppgat_schedule& sch, const int32_t* col, const int32_t* eid, const AttnArgs& a,
                  hipStream_t st) {
  hipLaunchKernelGGL((k_v2_attn<H, C>), dim3((unsigned)((sch.n_items + 3) / 4)), dim3(256), 0, st,
                     items_of(sch, sch.n_items), col, eid, a);
  return hipGetLastError();
}
}  // namespace

hipError_t gatv2_attention(const ppgat_schedule& sch, const int32_t* col, const int32_t* eid, int H, int C,
                           const float* xl, const float* xr, const float* att, const float* m, const float* invl,
                           float slope, bool scatter, float* alpha, hipStream_t st) {
  if (sch.n_items <= 0) return hipSuccess;
  const AttnArgs a{xl, xr, att, m, invl, slope, scatter ? 1 : 0, alpha};
  PPGAT_V2_DISPATCH(H, C, (attn_t<HH, CC>(sch, col, eid, a, st)));
}

hipError_t gatv2_bwd(const ppgat_schedule& src, const ppgat_schedule& dst, const int32_t* row, const int32_t* csc_eid,
                     const int32_t* col, const int32_t* csr_eid,
                     int64_t n, int H, int C, const float* xl, const float* xr, const float* att, const float* m,
                     const float* invl, const float* g, float slope, float p, const uint64_t* seed, float* dxl,
                     float* dxr, float* datt, float* dbias, void* ws, hipStream_t st) {
  BwdArgs a{xl,  xr,      att,     g,       m,       invl,    nullptr, slope, p, p > 0.f ? 1.f / (1.f - p) : 1.f,
            seed, nullptr, nullptr, nullptr, nullptr};
  PPGAT_V2_DISPATCH(H, C, (bwd_t<HH, CC>(src, dst, row, csc_eid, col, csr_eid, n, a, dxl, dxr, datt, dbias,
                                        static_cast<char*>(ws), st)));
}

}  // namespace ppgat
