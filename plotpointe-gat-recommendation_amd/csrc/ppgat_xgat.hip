// ppgat_xgat.hip -- the multi-head GAT layer in the aggregate-then-transform formulation (gfx950).
// Its dense products run on the matrix-core GEMMs of ppgat_xform.hip.
//
// GATConv(C_in, C, heads=H, concat=False) (scripts/train_gat_pyg.py:77)
// computes out_i = 1/H sum_h sum_{j->i} alpha_ij^h W_h x_j + bias with W_h = lin.weight rows
// [h C, (h+1) C).  The message is linear in x_j, so
//     out_i = 1/H sum_h W_h ax_i^h + bias,   ax_i^h = sum_{j->i} alpha_ij^h x_j   [H, C_in]
// and the attention logits only need s_src_j^h = x_j . A_src^h with A_src^h = W_h^T att_src^h
// (likewise s_dst).  With H*C > C_in (config 5: 4*256 = 1024 against 256) the edge pass
// gathers x_j (C_in floats) instead of h_j (H*C floats), h is never materialised, and a
// row-sharded rank exchanges x for its halo rows (dist.py).  Backward, with g = dOut:
//     gt_i^h = W_h^T g_i / H                  (GEMM [n, C] x [C, H C_in])
//     D_i^h  = gt_i^h . ax_i^h                (= sum_k beta dalpha, Appendix B)
//     per edge k = (j -> i): dz = alpha (d gt_i^h . x_j - D_i^h) lrelu'
//     dx_j   = sum_k sum_h beta_k^h gt_i^h + sum_h ds_src_j^h A_src^h + sum_h ds_dst_j^h A_dst^h
//     dW_h   = g^T ax^h / H + att_src^h (x) (ds_src^h)^T x + att_dst^h (x) (ds_dst^h)^T x
//     datt_src^h = W_h (ds_src^h)^T x, datt_dst^h likewise,  dbias = sum_i g_i.
// One edge pass by source (CSC) produces dx_msg, ds_src and the per-edge dz (at its CSR
// slot, summed per destination by k_dst_sum); no atomics anywhere, fixed summation orders.
// The logit and dropout rules are those of ppgat_kernels.hip (ppgat_device.h), PyG mode only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "ppgat_internal.h"
#include "ppgat_lanes.h"
#include "ppgat_device.h"

namespace ppgat {
namespace {

// ===========================================================================
// aggregate-then-transform layer pieces
// ===========================================================================
// A[v][h][k] = sum_c att_v[h][c] W[h C + c][k]  (v = 0: src, 1: dst) -> [2, H, K]
// (16 outputs per block, the c sum split over 16 threads in fixed 16-wide chunks and combined in
// chunk order: 128 blocks instead of eight, each with 256-long serial chains, which left the
// kernel at 98 us)
__global__ void __launch_bounds__(256) k_att_proj(const float* __restrict__ W, const float* __restrict__ att_src,
                                                  const float* __restrict__ att_dst, int H, int C, int K,
                                                  float* __restrict__ A) {
  __shared__ float red[16][16];
  const int kl = threadIdx.x & 15, cq = threadIdx.x >> 4;
  const int64_t t = (int64_t)blockIdx.x * 16 + kl;
  const bool live = t < (int64_t)2 * H * K;
  float s = 0.f;
  if (live) {
    const int v = (int)(t / ((int64_t)H * K));
    const int h = (int)((t / K) % H), k = (int)(t % K);
    const float* att = (v == 0 ? att_src : att_dst) + h * C;
    const int cw = (C + 15) / 16, c0 = cq * cw, c1 = min(C, c0 + cw);
    for (int c = c0; c < c1; ++c) s = fmaf(att[c], W[(int64_t)(h * C + c) * K + k], s);
  }
  red[cq][kl] = s;
  __syncthreads();
  if (cq == 0 && live) {
    float a = red[0][kl];
#pragma unroll
    for (int q = 1; q < 16; ++q) a += red[q][kl];
    A[t] = a;
  }
}

// Wt[h K + k][c] = W[h C + c][k]  (the transform, [H K, C]) and Wg[c][h K + k] = W[h C + c][k] / H
__global__ void __launch_bounds__(256) k_wperm(const float* __restrict__ W, int H, int C, int K,
                                               float* __restrict__ Wt, float* __restrict__ Wg) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)H * C * K) return;
  const int hc = (int)(t / K), k = (int)(t % K);
  const int h = hc / C, c = hc % C;
  const float w = W[t];
  if (Wt) Wt[((int64_t)h * K + k) * C + c] = w;
  if (Wg) Wg[(int64_t)c * H * K + (int64_t)h * K + k] = w * (1.f / (float)H);
}

// s_src[n][h] = x_n . A_src[h] (n < n_rows), s_dst[n][h] = x_n . A_dst[h] (n < n_dst).
// K = 256: a row is one float4 per lane; a wave takes 4 rows per iteration (their loads in
// flight together), and each row's 2H lane partials are summed by one transposing butterfly
// (lanes 64 / 2H * v .. hold score v): 2H - 1 exchanges + a short reduction instead of 2H
// full-wave reductions.  (One row at a time with 2H six-step reductions ran at 3.0 TB/s.)
template <int K, int H>
__global__ void __launch_bounds__(256) k_xscores(const float* __restrict__ x, int64_t ldx, int64_t n_rows,
                                                 int64_t n_dst, const float* __restrict__ A, float* __restrict__ s_src,
                                                 float* __restrict__ s_dst) {
  static_assert(K == 256 && (H == 2 || H == 4), "k_xscores: K = 256, H in {2, 4}");
  constexpr int V = 2 * H, R = 4, LV = 64 / V;
  const int lane = threadIdx.x & 63;
  float4 av[V];
#pragma unroll
  for (int v = 0; v < V; ++v) av[v] = ld4(A + v * K + lane * 4);
  const int64_t nw = (int64_t)gridDim.x * 4;
  const int vi = lane / LV;  // the score this lane ends with
  for (int64_t base = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * R; base < n_rows; base += nw * R) {
    float4 xv[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t n = base + r;
      xv[r] = ld4(x + (n < n_rows ? n : n_rows - 1) * ldx + lane * 4);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float pv[V];
#pragma unroll
      for (int v = 0; v < V; ++v) pv[v] = dot4(xv[r], av[v]);
      const float sum = transpose_reduce<64, V>(pv, lane);
      const int64_t n = base + r;
      if (n < n_rows && lane % LV == 0) {
        if (vi < H) s_src[n * H + vi] = sum;
        else if (n < n_dst) s_dst[n * H + vi - H] = sum;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// forward edge pass: one wave per destination item (CSR), the neighbour row x_j (K floats)
// gathered ONCE per edge for all H heads: ax^h += p^h x_j with the online softmax per head.
// K = 256: one float4 per lane, one edge at a time across the wave, U rows in flight.
// Hub pieces leave [ax^h (K) | m | l | - -] per (item, head) for k_fwd_merge_wg.
// ---------------------------------------------------------------------------
// U rows in flight per wave: 4 (96 VGPRs, five waves per SIMD) -- 8 rows (144 VGPRs, three waves)
// left the pass at 7.1 ms per call on the config-5 share, 4 gives 6.0-6.3 (profiles/r06/x2/x3_bench5_fwdx_u*.log;
// 2, 3 and 6 within noise of 4); the FMA order per lane is the same for every U (same bits)
template <int K, int H, int U = 4>
__global__ void __launch_bounds__(256) k_fwd_x(Items it, const int32_t* __restrict__ col,
                                               const int32_t* __restrict__ eid, const float* __restrict__ x,
                                               int64_t ldx, const float* __restrict__ s_src,
                                               const float* __restrict__ s_dst, float slope, float p, float inv_keep,
                                               uint64_t seed, const uint64_t* __restrict__ seed_in,
                                               float* __restrict__ agg, float* __restrict__ m_out,
                                               float* __restrict__ invl_out, float* __restrict__ partial,
                                               unsigned* __restrict__ xmax) {
  // xmax != NULL: the column maxima of |x_j| over the gathered rows (every source of an edge)
  // merged into it -- the bound of |agg| the weight gradient's fp16 split needs, for free
  static_assert(K == 256, "k_fwd_x: K == 256 (one float4 per lane)");
  if (p > 0.f) seed = *seed_in;
  __shared__ int recj[4][64];
  __shared__ float recw[4][H][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t w = (int64_t)blockIdx.x * 4 + wv;
  if (w >= it.n_items) return;
  const int64_t i = it.row[w];
  const int rs = it.beg[w], re = it.end[w];
  const bool hub = w < it.n_hub_items;
  float sd[H], mh[H], lh[H];
  float4 acc[H];
  float4 xm = f4(0.f);
#pragma unroll
  for (int h = 0; h < H; ++h) {
    sd[h] = s_dst[i * H + h];
    mh[h] = -INFINITY;
    lh[h] = 0.f;
    acc[h] = f4(0.f);
  }
  for (int base = rs; base < re; base += 64) {
    const int k = base + lane;
    const bool valid = k < re;
    const int j = valid ? col[k] : 0;
    const uint32_t e_id = (valid && p > 0.f) ? (uint32_t)eid[k] : 0u;
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const float e = valid ? lrelu(s_src[(int64_t)j * H + h] + sd[h], slope) : -INFINITY;
      const float mn = fmaxf(mh[h], wave_max(e));
      const float sc = expf(mh[h] - mn);
      const float pe = valid ? expf(e - mn) : 0.f;
      lh[h] = fmaf(lh[h], sc, wave_sum(pe));
      acc[h] = mul4(acc[h], sc);
      mh[h] = mn;
      float pw = pe;
      if (p > 0.f && valid) pw *= drop_scale(seed, e_id, (uint32_t)h, p, inv_keep);
      recw[wv][h][lane] = pw;
    }
    recj[wv][lane] = j;
    wave_sync();
    const int n = min(64, re - base);
    for (int q0 = 0; q0 < n; q0 += U) {
      float4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int q = q0 + u;
        v[u] = q < n ? ld4(x + (int64_t)recj[wv][q] * ldx + lane * 4) : f4(0.f);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int q = min(q0 + u, 63);
#pragma unroll
        for (int h = 0; h < H; ++h) acc[h] = fma4(q0 + u < n ? recw[wv][h][q] : 0.f, v[u], acc[h]);
        xm = absmax4(xm, v[u]);
      }
    }
    wave_sync();
  }
  if (xmax != nullptr) colmax_merge4(xmax, lane * 4, xm);
#pragma unroll
  for (int h = 0; h < H; ++h) {
    if (hub) {
      float* slot = partial + (w * H + h) * (K + 4);
      st4(slot + lane * 4, acc[h]);
      if (lane == 0) st4(slot + K, make_float4(mh[h], lh[h], 0.f, 0.f));
      continue;
    }
    const float invl = 1.f / (lh[h] + 1e-16f);
    st4(agg + (i * H + h) * K + lane * 4, mul4(acc[h], invl));
    if (lane == 0) {
      m_out[i * H + h] = re > rs ? mh[h] : 0.f;
      invl_out[i * H + h] = invl;
    }
  }
}

// backward prologue: nstate[i][h] = {s_dst, m, inv_l, D = gt_i^h . ax_i^h}; one wave per row
template <int K, int H>
__global__ void __launch_bounds__(256) k_bwd_x_pro(const float* __restrict__ gt, const float* __restrict__ agg,
                                                   const float* __restrict__ s_dst, const float* __restrict__ m,
                                                   const float* __restrict__ invl, int64_t n,
                                                   float4* __restrict__ nstate) {
  static_assert(K == 256, "k_bwd_x_pro: K == 256");
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += nw) {
    float d[16];
#pragma unroll
    for (int h = 0; h < 16; ++h) d[h] = 0.f;
#pragma unroll
    for (int h = 0; h < H; ++h)
      d[h] = dot4(ld4(gt + (i * H + h) * K + lane * 4), ld4(agg + (i * H + h) * K + lane * 4));
#pragma unroll
    for (int h = 0; h < H; ++h) d[h] = wave_sum(d[h]);
    if (lane < H) {
      float dv = d[0];
#pragma unroll
      for (int h = 1; h < H; ++h) dv = lane == h ? d[h] : dv;
      const int64_t pr = i * H + lane;
      nstate[pr] = make_float4(s_dst[pr], m[pr], invl[pr], dv);
    }
  }
}

// ---------------------------------------------------------------------------
// backward edge pass by SOURCE (CSC): one wave per source item; x_j in registers (float4
// per lane), per out-edge the destination's gt_i (H x K floats) and packed state gathered
// once.  Per group of 4 edges the 16 partial dots <gt_i^h, x_j> are summed over the wave
// with a transposing butterfly.  Writes dx_j = sum beta gt + sum_h ds_src^h A_src^h (hub
// pieces: [msg (K) | ds_h (H <= 4)] partials), ds_src[j][h], and dz at each edge's CSR slot.
// ---------------------------------------------------------------------------
template <int OFF, int N>
__device__ __forceinline__ int tr_reduce(float (&v)[16], int sl, int& base) {
  if constexpr (OFF >= 8 && N > 1) {
    constexpr int Hh = N / 2;
    const bool bit = (sl & OFF) != 0;
#pragma unroll
    for (int t = 0; t < Hh; ++t) {
      if constexpr (OFF >= 16) {
        float r0, r1;
        row_swap<OFF>(v[t], v[Hh + t], r0, r1);
        v[t] = r0 + r1;
      } else {
        const float send = bit ? v[t] : v[Hh + t];
        const float keep = bit ? v[Hh + t] : v[t];
        v[t] = keep + dpp<0x128>(send);
      }
    }
    if (bit) base += Hh;
    return tr_reduce<OFF / 2, Hh>(v, sl, base);
  } else {
#pragma unroll
    for (int t = 0; t < N; ++t) v[t] = group_reduce<Op::Sum, 1, 4>(v[t]);
    return N;
  }
}

template <int K, int H>
__global__ void __launch_bounds__(256) k_bwd_x(Items it, const int32_t* __restrict__ row,
                                               const int32_t* __restrict__ csc_eid,
                                               const int32_t* __restrict__ csc2csr, const float* __restrict__ x,
                                               int64_t ldx, const float* __restrict__ s_src,
                                               const float4* __restrict__ nstate, const float* __restrict__ gt,
                                               const float* __restrict__ A_src, float slope, float p, float inv_keep,
                                               uint64_t seed, const uint64_t* __restrict__ seed_in,
                                               float* __restrict__ dx, int64_t lddx, float* __restrict__ S,
                                               int64_t lds, float* __restrict__ dz, float* __restrict__ partial) {
  static_assert(K == 256 && H <= 4, "k_bwd_x: K == 256, H <= 4");
  constexpr int U = 16 / H;  // edges per reduction group (16 partial dots per lane)
  if (p > 0.f) seed = *seed_in;
  __shared__ int2 recA[4][64];          // {dst row, CSR slot}
  __shared__ float4 recH[4][H][64];     // per head {beta, c1, c0, -}
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t w = (int64_t)blockIdx.x * 4 + wv;
  if (w >= it.n_items) return;
  const int64_t j = it.row[w];
  const int cs = it.beg[w], ce = it.end[w];
  const bool hub = w < it.n_hub_items;
  const float4 xv = ld4(x + j * ldx + lane * 4);
  float ss[H], dsa[H];
#pragma unroll
  for (int h = 0; h < H; ++h) {
    ss[h] = s_src[j * H + h];
    dsa[h] = 0.f;
  }
  float4 acc = f4(0.f);
  for (int base = cs; base < ce; base += 64) {
    const int k = base + lane;
    const bool valid = k < ce;
    const int i = valid ? row[k] : 0;
    const int slot = valid ? (csc2csr != nullptr ? csc2csr[k] : k) : 0;  // NULL: dz in CSC order
    const uint32_t e_id = (valid && p > 0.f) ? (uint32_t)csc_eid[k] : 0u;
#pragma unroll
    for (int h = 0; h < H; ++h) {
      float bg = 0.f, c1 = 0.f, c0 = 0.f;
      if (valid) {
        const float4 st = nstate[(int64_t)i * H + h];  // {s_dst, m, inv_l, D}
        const float z = ss[h] + st.x;
        const float af = expf(lrelu(z, slope) - st.y) * st.z;
        const float dm = p > 0.f ? drop_scale(seed, e_id, (uint32_t)h, p, inv_keep) : 1.f;
        bg = af * dm;
        const float a1 = af * dlrelu(z, slope);
        c1 = a1 * dm;
        c0 = a1 * st.w;
      }
      recH[wv][h][lane] = make_float4(bg, c1, c0, 0.f);
    }
    recA[wv][lane] = make_int2(i, slot);
    wave_sync();
    const int n = min(64, ce - base);
    for (int q0 = 0; q0 < n; q0 += U) {
      float4 g[U][H];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int q = q0 + u;
        const int64_t ii = recA[wv][min(q, 63)].x;
#pragma unroll
        for (int h = 0; h < H; ++h) g[u][h] = q < n ? ld4(gt + (ii * H + h) * K + lane * 4) : f4(0.f);
      }
      float part[16];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int q = min(q0 + u, 63);
#pragma unroll
        for (int h = 0; h < H; ++h) {
          const float bq = q0 + u < n ? recH[wv][h][q].x : 0.f;
          acc = fma4(bq, g[u][h], acc);
          part[u * H + h] = dot4(g[u][h], xv);
        }
      }
      int vbase = 0;
      const int R = tr_reduce<32, 16>(part, lane, vbase);
      const int t = lane & 7;
      if (t < R) {
        float dot = part[0];
#pragma unroll
        for (int c = 1; c < 8; ++c)
          if (c == t) dot = part[c];
        const int vi = vbase + t;
        const int u = vi / H, h = vi % H;
        const int q = q0 + u;
        if (q < n) {
          const float4 rb = recH[wv][h][q];
          const float dzv = fmaf(rb.y, dot, -rb.z);
#pragma unroll
          for (int c = 0; c < H; ++c)
            if (c == h) dsa[c] += dzv;
          dz[(int64_t)recA[wv][q].y * H + h] = dzv;
        }
      }
    }
    wave_sync();
  }
  float ds[H];
#pragma unroll
  for (int h = 0; h < H; ++h) ds[h] = wave_sum(dsa[h]);
  if (hub) {
    float* sp = partial + w * (K + 4);
    st4(sp + lane * 4, acc);
    if (lane == 0) {
      float4 d = f4(0.f);
      d.x = ds[0];
      if (H > 1) d.y = ds[1];
      if (H > 2) d.z = ds[2];
      if (H > 3) d.w = ds[3];
      st4(sp + K, d);
    }
    return;
  }
#pragma unroll
  for (int h = 0; h < H; ++h) acc = fma4(ds[h], ld4(A_src + h * K + lane * 4), acc);
  st4(dx + j * lddx + lane * 4, acc);
  if (lane < H) {
    float v = ds[0];
#pragma unroll
    for (int h = 1; h < H; ++h) v = lane == h ? ds[h] : v;
    S[j * lds + lane] = v;
  }
}

// hub sources: sum the pieces in order, add the attention term
template <int K, int H>
__global__ void __launch_bounds__(256) k_bwd_x_merge(const int32_t* __restrict__ hub_row,
                                                     const int32_t* __restrict__ hub_ptr, int64_t n_hubs,
                                                     const float* __restrict__ partial, const float* __restrict__ A_src,
                                                     float* __restrict__ dx, int64_t lddx, float* __restrict__ S,
                                                     int64_t lds) {
  const int lane = threadIdx.x & 63;
  const int64_t hb = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (hb >= n_hubs) return;
  const int64_t j = hub_row[hb];
  float4 acc = f4(0.f), d = f4(0.f);
  for (int q = hub_ptr[hb]; q < hub_ptr[hb + 1]; ++q) {
    acc = add4(acc, ld4(partial + (int64_t)q * (K + 4) + lane * 4));
    d = add4(d, ld4(partial + (int64_t)q * (K + 4) + K));
  }
  const float ds[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
  for (int h = 0; h < H; ++h) acc = fma4(ds[h], ld4(A_src + h * K + lane * 4), acc);
  st4(dx + j * lddx + lane * 4, acc);
  if (lane < H) S[j * lds + lane] = ds[lane];
}

// ---------------------------------------------------------------------------
// The backward edge pass gathering g_i (C floats per edge) instead of gt_i (H x C_in):
// dalpha^h_ij = gt^h_i . x_j = g_i . hs^h_j with hs^h_j = W_h x_j / H (one GEMM over the
// sources, read once per source here), and the message gradient is accumulated per head as
// acc^h_j = sum_i beta^h_ij g_i (written once per source, [n_src, H, C]); then
// dx_j = acc_j . W (one NN GEMM, rows h C + c of W = W_h) + the attention terms.  Per edge
// 1 KB instead of 4 KB of gathers at config 5.  Summation orders as k_bwd_x (edges in CSC
// order, hub pieces merged in piece order): deterministic.
// ---------------------------------------------------------------------------
template <int C, int H>
__global__ void __launch_bounds__(256) k_bwd_g(Items it, const int32_t* __restrict__ row,
                                               const int32_t* __restrict__ csc_eid,
                                               const int32_t* __restrict__ csc2csr, const float* __restrict__ hs,
                                               const float* __restrict__ s_src, const float4* __restrict__ nstate,
                                               const float* __restrict__ g, int64_t ldg, float slope, float p,
                                               float inv_keep, uint64_t seed, const uint64_t* __restrict__ seed_in,
                                               float* __restrict__ acc_out, float* __restrict__ S, int64_t lds,
                                               float* __restrict__ dz, float* __restrict__ partial,
                                               float* __restrict__ pz, unsigned* __restrict__ gmax) {
  // pz != NULL (deferred D): dz receives dalpha = g_i . hs_j and pz beta * dalpha per edge and
  // head (D_i = sum_j beta dalpha by a destination sum, dz by k_xgat_dz); no ds_src here.
  // gmax != NULL: the column maxima of |g_i| over the gathered rows (every destination of an
  // edge) merged into it
  static_assert(C == 256 && H <= 4, "k_bwd_g: C == 256, H <= 4");
  constexpr int U = 16 / H;  // edges per reduction group (16 partial dots per lane)
  if (p > 0.f) seed = *seed_in;
  __shared__ int2 recA[4][64];          // {dst row, dz slot}
  __shared__ float4 recH[4][H][64];     // per head {beta, c1, c0, -}
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t w = (int64_t)blockIdx.x * 4 + wv;
  if (w >= it.n_items) return;
  const int64_t j = it.row[w];
  const int cs = it.beg[w], ce = it.end[w];
  const bool hub = w < it.n_hub_items;
  float4 hv[H], acc[H];
  float4 gm = f4(0.f);
  float ss[H], dsa[H];
#pragma unroll
  for (int h = 0; h < H; ++h) {
    hv[h] = ld4(hs + (j * H + h) * C + lane * 4);
    acc[h] = f4(0.f);
    ss[h] = s_src[j * H + h];
    dsa[h] = 0.f;
  }
  for (int base = cs; base < ce; base += 64) {
    const int k = base + lane;
    const bool valid = k < ce;
    const int i = valid ? row[k] : 0;
    const int slot = valid ? (csc2csr != nullptr ? csc2csr[k] : k) : 0;  // NULL: dz in CSC order
    const uint32_t e_id = (valid && p > 0.f) ? (uint32_t)csc_eid[k] : 0u;
#pragma unroll
    for (int h = 0; h < H; ++h) {
      float bg = 0.f, c1 = 0.f, c0 = 0.f;
      if (valid) {
        const float4 st = nstate[(int64_t)i * H + h];  // {s_dst, m, inv_l, D}
        const float z = ss[h] + st.x;
        const float af = expf(lrelu(z, slope) - st.y) * st.z;
        const float dm = p > 0.f ? drop_scale(seed, e_id, (uint32_t)h, p, inv_keep) : 1.f;
        bg = af * dm;
        const float a1 = af * dlrelu(z, slope);
        c1 = a1 * dm;
        c0 = a1 * st.w;
      }
      recH[wv][h][lane] = make_float4(bg, c1, c0, 0.f);
    }
    recA[wv][lane] = make_int2(i, slot);
    wave_sync();
    const int n = min(64, ce - base);
    for (int q0 = 0; q0 < n; q0 += U) {
      float4 gq[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int q = q0 + u;
        const int64_t ii = recA[wv][min(q, 63)].x;
        gq[u] = q < n ? ld4(g + ii * ldg + lane * 4) : f4(0.f);
        gm = absmax4(gm, gq[u]);
      }
      float part[16];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int q = min(q0 + u, 63);
#pragma unroll
        for (int h = 0; h < H; ++h) {
          const float bq = q0 + u < n ? recH[wv][h][q].x : 0.f;
          acc[h] = fma4(bq, gq[u], acc[h]);
          part[u * H + h] = dot4(gq[u], hv[h]);
        }
      }
      int vbase = 0;
      const int R = tr_reduce<32, 16>(part, lane, vbase);
      const int t = lane & 7;
      if (t < R) {
        float dot = part[0];
#pragma unroll
        for (int c = 1; c < 8; ++c)
          if (c == t) dot = part[c];
        const int vi = vbase + t;
        const int u = vi / H, h = vi % H;
        const int q = q0 + u;
        if (q < n) {
          const float4 rb = recH[wv][h][q];
          const int64_t o = (int64_t)recA[wv][q].y * H + h;
          if (pz != nullptr) {
            dz[o] = dot;
            pz[o] = rb.x * dot;
          } else {
            const float dzv = fmaf(rb.y, dot, -rb.z);
#pragma unroll
            for (int c = 0; c < H; ++c)
              if (c == h) dsa[c] += dzv;
            dz[o] = dzv;
          }
        }
      }
    }
    wave_sync();
  }
  if (gmax != nullptr) colmax_merge4(gmax, lane * 4, gm);
  float ds[H];
#pragma unroll
  for (int h = 0; h < H; ++h) ds[h] = wave_sum(dsa[h]);
  if (hub) {
    float* sp = partial + w * (H * C + 4);
#pragma unroll
    for (int h = 0; h < H; ++h) st4(sp + h * C + lane * 4, acc[h]);
    if (lane == 0) {
      float4 d = f4(0.f);
      d.x = ds[0];
      if (H > 1) d.y = ds[1];
      if (H > 2) d.z = ds[2];
      if (H > 3) d.w = ds[3];
      st4(sp + H * C, d);
    }
    return;
  }
#pragma unroll
  for (int h = 0; h < H; ++h) st4(acc_out + (j * H + h) * C + lane * 4, acc[h]);
  if (lane < H && S != nullptr) {  // deferred D: ds_src comes from k_xgat_dz
    float v = ds[0];
#pragma unroll
    for (int h = 1; h < H; ++h) v = lane == h ? ds[h] : v;
    S[j * lds + lane] = v;
  }
}

// nstate[i][h] = {s_dst, m, inv_l, D or 0} (the deferred-D backward builds it twice: without D
// for k_bwd_g, with D for k_xgat_dz)
__global__ void __launch_bounds__(256) k_xgat_nstate(const float* __restrict__ s_dst, const float* __restrict__ m,
                                                     const float* __restrict__ invl, const float* __restrict__ D,
                                                     int64_t n, float4* __restrict__ nstate) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  nstate[t] = make_float4(s_dst[t], m[t], invl[t], D != nullptr ? D[t] : 0.f);
}

// deferred-D backward, by SOURCE over the CSC: dz = alpha e'(z) (dm dalpha - D_i) per edge and
// head, in place over dalpha (the formula and rounding of k_bwd_g's dz), and ds_src_j = sum of
// the source's dz.  LPI lanes per source item over items [w0, w1): 16 for the hub and long items,
// 4 for the short ones (<= 16 edges: four rows per lane group keep four times as many items in
// flight).  Each lane takes every LPI-th edge, four at a time with all their loads issued
// first, summed in edge order, then the LPI-lane tree; hub pieces leave a partial that
// k_xgat_dz_merge_wg adds up (pieces dealt to the waves, combined in wave order).
template <int H, int LPI>
__global__ void __launch_bounds__(256) k_xgat_dz(Items it, int64_t w0, int64_t w1, const int32_t* __restrict__ row,
                                                 const int32_t* __restrict__ csc_eid,
                                                 const int32_t* __restrict__ csc2csr, const float* __restrict__ s_src,
                                                 const float4* __restrict__ nstate, float slope, float p,
                                                 float inv_keep, uint64_t seed, const uint64_t* __restrict__ seed_in,
                                                 float* __restrict__ dz, float* __restrict__ S, int64_t lds,
                                                 float* __restrict__ partial) {
  if (p > 0.f) seed = *seed_in;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t w = w0 + t / LPI;
  const int l = (int)(t % LPI);
  const bool live = w < w1;
  float ds[H];
#pragma unroll
  for (int h = 0; h < H; ++h) ds[h] = 0.f;
  int64_t j = 0;
  if (live) {
    j = it.row[w];
    float ss[H];
#pragma unroll
    for (int h = 0; h < H; ++h) ss[h] = s_src[j * H + h];
    const int ce = it.end[w];
    for (int k0 = it.beg[w] + l; k0 < ce; k0 += 4 * LPI) {
      int64_t ii[4], sl[4];
      uint32_t e_id[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k = k0 + u * LPI < ce ? k0 + u * LPI : k0;
        ii[u] = row[k];
        sl[u] = csc2csr != nullptr ? (int64_t)csc2csr[k] : (int64_t)k;
        e_id[u] = p > 0.f ? (uint32_t)csc_eid[k] : 0u;
      }
      float4 st[4][H];
      float dv[4][H];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int h = 0; h < H; ++h) {
          st[u][h] = nstate[ii[u] * H + h];  // {s_dst, m, inv_l, D}
          dv[u][h] = dz[sl[u] * H + h];
        }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (k0 + u * LPI < ce) {
#pragma unroll
          for (int h = 0; h < H; ++h) {
            const float z = ss[h] + st[u][h].x;
            const float af = expf(lrelu(z, slope) - st[u][h].y) * st[u][h].z;
            const float dm = p > 0.f ? drop_scale(seed, e_id[u], (uint32_t)h, p, inv_keep) : 1.f;
            const float a1 = af * dlrelu(z, slope);
            const float dzv = fmaf(a1 * dm, dv[u][h], -(a1 * st[u][h].w));
            dz[sl[u] * H + h] = dzv;
            ds[h] += dzv;
          }
        }
      }
    }
  }
#pragma unroll
  for (int h = 0; h < H; ++h) {
    const float x = group_reduce<Op::Sum, 1, LPI / 2>(ds[h]);  // the LPI lanes of the item
    if (live && l == 0) {
      if (w < it.n_hub_items) partial[w * H + h] = x;
      else S[j * lds + h] = x;
    }
  }
}

// ---------------------------------------------------------------------------
// Hub merges with a whole workgroup on each hub: the pieces are dealt to the kMW waves in
// turn (each wave keeps several partial rows in flight), and the waves' sums are combined in
// wave order through LDS -- a fixed order, deterministic.  One wave per hub (k_fwd_merge,
// k_bwd_g_merge, k_xgat_dz_merge: pieces in a single wave's loop) left config 5's top item --
// 1M edges = 3,900 pieces of 256 edges, on the rank that owns it -- merging for 4 ms per call,
// 10 ms per step of that rank (profiles/r04/v16_probe5_r0_kernel_stats.csv).
// ---------------------------------------------------------------------------
constexpr int kMW = 8;    // waves per hub in the dz merge
constexpr int kMWf = 16;  // waves per (hub, head) in the forward merge (its hubs all above kSmallP pieces)
constexpr int kMWb = 8;   // waves per (hub, component) in the backward merge (16: 27.4 us per call at the config-5 share, 8: 23.1)
// Hubs of at most kSmallP pieces (most of them: config 5's share has 3,740 hubs, few above a
// dozen pieces) are merged by one wave per (hub, head) instead -- a workgroup of 8-16 waves on
// a 3-piece hub leaves most of its waves idle through three barriers.  The workgroup kernels
// skip those hubs.
constexpr int kSmallP = 16;

// one wave per (hub, head) for the small hubs: lanes hold the pieces' m and l, then the rows
// in piece order, four loads in flight
__global__ void __launch_bounds__(256) k_fwd_merge_small(const int32_t* __restrict__ hub_row,
                                                         const int32_t* __restrict__ hub_ptr, int64_t n_hubs,
                                                         int heads, const float* __restrict__ partial, float eps,
                                                         float* __restrict__ m_out, float* __restrict__ invl_out,
                                                         float* __restrict__ agg_out) {
  constexpr int C = 256;
  const int lane = threadIdx.x & 63;
  const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= n_hubs * heads) return;
  const int64_t hb = u / heads;
  const int hd = (int)(u - hb * heads);
  const int p0 = hub_ptr[hb], p1 = hub_ptr[hb + 1];
  if (p1 - p0 > kSmallP) return;
  const int64_t i = hub_row[hb];
  auto slot = [&](int q) { return partial + ((int64_t)q * heads + hd) * (C + 4); };
  float mq = -INFINITY, lq = 0.f;
  if (p0 + lane < p1) {
    mq = slot(p0 + lane)[C];
    lq = slot(p0 + lane)[C + 1];
  }
  const float M = wave_max(mq);
  const float l = wave_sum(p0 + lane < p1 ? lq * expf(mq - M) : 0.f);
  float4 a0 = f4(0.f), a1 = f4(0.f), a2 = f4(0.f), a3 = f4(0.f);
  int q = p0;
  for (; q + 3 < p1; q += 4) {
    const float4 v0 = ld4(slot(q) + lane * 4), v1 = ld4(slot(q + 1) + lane * 4), v2 = ld4(slot(q + 2) + lane * 4),
                 v3 = ld4(slot(q + 3) + lane * 4);
    a0 = fma4(expf(__shfl(mq, q - p0) - M), v0, a0);
    a1 = fma4(expf(__shfl(mq, q + 1 - p0) - M), v1, a1);
    a2 = fma4(expf(__shfl(mq, q + 2 - p0) - M), v2, a2);
    a3 = fma4(expf(__shfl(mq, q + 3 - p0) - M), v3, a3);
  }
  for (; q < p1; ++q) a0 = fma4(expf(__shfl(mq, q - p0) - M), ld4(slot(q) + lane * 4), a0);
  const float invl = 1.f / (l + eps);
  st4(agg_out + (i * heads + hd) * C + lane * 4, mul4(add4(add4(a0, a1), add4(a2, a3)), invl));
  if (lane == 0) {
    m_out[i * heads + hd] = M;
    invl_out[i * heads + hd] = invl;
  }
}

// aggregate-then-transform forward: agg[i,h] = sum_q e^(m_q - M) ax_q / sum_q e^(m_q - M) l_q
__global__ void __launch_bounds__(64 * kMWf) k_fwd_merge_wg(const int32_t* __restrict__ hub_row,
                                                           const int32_t* __restrict__ hub_ptr, int heads,
                                                           const float* __restrict__ partial, float eps,
                                                           float* __restrict__ m_out, float* __restrict__ invl_out,
                                                           float* __restrict__ agg_out) {
  constexpr int C = 256;
  __shared__ float4 red[kMWf][64];
  __shared__ float sr[kMWf];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t hb = blockIdx.x;
  const int64_t i = hub_row[hb];
  const int p0 = hub_ptr[hb], p1 = hub_ptr[hb + 1];
  if (p1 - p0 <= kSmallP) return;  // k_fwd_merge_small's
  auto slot = [&](int q, int hd) { return partial + ((int64_t)q * heads + hd) * (C + 4); };
  {
    const int hd = blockIdx.y;  // one workgroup per (hub, head): 3,740 hubs x 4 heads at the config-5 share
    float M = -INFINITY;
    for (int q = p0 + tid; q < p1; q += 64 * kMWf) M = fmaxf(M, slot(q, hd)[C]);
    M = wave_max(M);
    if (lane == 0) sr[w] = M;
    __syncthreads();
    M = sr[0];
    for (int k = 1; k < kMWf; ++k) M = fmaxf(M, sr[k]);
    __syncthreads();
    float t = 0.f;
    for (int q = p0 + tid; q < p1; q += 64 * kMWf) t += slot(q, hd)[C + 1] * expf(slot(q, hd)[C] - M);
    t = wave_sum(t);
    if (lane == 0) sr[w] = t;
    float4 a0 = f4(0.f), a1 = f4(0.f), a2 = f4(0.f), a3 = f4(0.f);
    int q = p0 + w;
    for (; q + 3 * kMWf < p1; q += 4 * kMWf) {
      const float* s0 = slot(q, hd);
      const float* s1 = slot(q + kMWf, hd);
      const float* s2 = slot(q + 2 * kMWf, hd);
      const float* s3 = slot(q + 3 * kMWf, hd);
      const float4 v0 = ld4(s0 + lane * 4), v1 = ld4(s1 + lane * 4), v2 = ld4(s2 + lane * 4), v3 = ld4(s3 + lane * 4);
      a0 = fma4(expf(s0[C] - M), v0, a0);
      a1 = fma4(expf(s1[C] - M), v1, a1);
      a2 = fma4(expf(s2[C] - M), v2, a2);
      a3 = fma4(expf(s3[C] - M), v3, a3);
    }
    for (; q < p1; q += kMWf) a0 = fma4(expf(slot(q, hd)[C] - M), ld4(slot(q, hd) + lane * 4), a0);
    red[w][lane] = add4(add4(a0, a1), add4(a2, a3));
    __syncthreads();
    if (w == 0) {
      float l = 0.f;
      for (int k = 0; k < kMWf; ++k) l += sr[k];
      float4 acc = red[0][lane];
      for (int k = 1; k < kMWf; ++k) acc = add4(acc, red[k][lane]);
      const float invl = 1.f / (l + eps);
      st4(agg_out + (i * heads + hd) * C + lane * 4, mul4(acc, invl));
      if (lane == 0) {
        m_out[i * heads + hd] = M;
        invl_out[i * heads + hd] = invl;
      }
    }
  }
}

// hub sources of k_bwd_g: the pieces' [acc^h (C) x H | ds] summed, waves in order; one workgroup
// per (hub, component): blockIdx.y = h < H sums head h's row, blockIdx.y = H the ds quad
template <int C, int H>
__global__ void __launch_bounds__(64 * kMWb) k_bwd_g_merge_wg(const int32_t* __restrict__ hub_row,
                                                             const int32_t* __restrict__ hub_ptr,
                                                             const float* __restrict__ partial,
                                                             float* __restrict__ acc_out, float* __restrict__ S,
                                                             int64_t lds) {
  static_assert(C == 256, "one float4 per lane");
  __shared__ float4 red[kMWb][64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t hb = blockIdx.x;
  const int h = blockIdx.y;
  if (h == H && S == nullptr) return;
  const int p0 = hub_ptr[hb], p1 = hub_ptr[hb + 1];
  if (p1 - p0 <= kSmallP) return;  // k_bwd_g_merge_small's
  const int64_t j = hub_row[hb];
  const int off = h < H ? h * C + lane * 4 : H * C;
  float4 a = f4(0.f), b = f4(0.f);
  int q = p0 + w;
  // eight, then four pieces' loads in flight per wave (the first half into a, the rest into b)
  for (; q + 7 * kMWb < p1; q += 8 * kMWb) {
    float4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = ld4(partial + (int64_t)(q + u * kMWb) * (H * C + 4) + off);
    a = add4(add4(add4(add4(a, v[0]), v[1]), v[2]), v[3]);
    b = add4(add4(add4(add4(b, v[4]), v[5]), v[6]), v[7]);
  }
  for (; q + 3 * kMWb < p1; q += 4 * kMWb) {
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = ld4(partial + (int64_t)(q + u * kMWb) * (H * C + 4) + off);
    a = add4(add4(a, v[0]), v[1]);
    b = add4(add4(b, v[2]), v[3]);
  }
  for (; q + kMWb < p1; q += 2 * kMWb) {
    const float4 v0 = ld4(partial + (int64_t)q * (H * C + 4) + off);
    const float4 v1 = ld4(partial + (int64_t)(q + kMWb) * (H * C + 4) + off);
    a = add4(a, v0);
    b = add4(b, v1);
  }
  if (q < p1) a = add4(a, ld4(partial + (int64_t)q * (H * C + 4) + off));
  red[w][lane] = add4(a, b);
  __syncthreads();
  if (w != 0) return;
  float4 acc = red[0][lane];
  for (int k = 1; k < kMWb; ++k) acc = add4(acc, red[k][lane]);
  if (h < H) {
    st4(acc_out + (j * H + h) * C + lane * 4, acc);
  } else if (lane < H) {
    const float ds[4] = {acc.x, acc.y, acc.z, acc.w};
    S[j * lds + lane] = ds[lane];
  }
}

// one wave per (hub, component) for the small hubs: the pieces in order, four loads in flight
template <int C, int H>
__global__ void __launch_bounds__(256) k_bwd_g_merge_small(const int32_t* __restrict__ hub_row,
                                                           const int32_t* __restrict__ hub_ptr, int64_t n_hubs,
                                                           const float* __restrict__ partial,
                                                           float* __restrict__ acc_out, float* __restrict__ S,
                                                           int64_t lds) {
  static_assert(C == 256, "one float4 per lane");
  const int lane = threadIdx.x & 63;
  const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= n_hubs * (H + 1)) return;
  const int64_t hb = u / (H + 1);
  const int h = (int)(u - hb * (H + 1));
  if (h == H && S == nullptr) return;
  const int p0 = hub_ptr[hb], p1 = hub_ptr[hb + 1];
  if (p1 - p0 > kSmallP) return;
  const int64_t j = hub_row[hb];
  const int off = h < H ? h * C + lane * 4 : H * C;
  float4 a0 = f4(0.f), a1 = f4(0.f), a2 = f4(0.f), a3 = f4(0.f);
  int q = p0;
  for (; q + 3 < p1; q += 4) {
    const float* s = partial + (int64_t)q * (H * C + 4) + off;
    const float4 v0 = ld4(s), v1 = ld4(s + (H * C + 4)), v2 = ld4(s + 2 * (H * C + 4)), v3 = ld4(s + 3 * (H * C + 4));
    a0 = add4(a0, v0);
    a1 = add4(a1, v1);
    a2 = add4(a2, v2);
    a3 = add4(a3, v3);
  }
  for (; q < p1; ++q) a0 = add4(a0, ld4(partial + (int64_t)q * (H * C + 4) + off));
  const float4 acc = add4(add4(a0, a1), add4(a2, a3));
  if (h < H) {
    st4(acc_out + (j * H + h) * C + lane * 4, acc);
  } else if (lane < H) {
    const float ds[4] = {acc.x, acc.y, acc.z, acc.w};
    S[j * lds + lane] = ds[lane];
  }
}

// hub sources of k_xgat_dz: ds_src = the pieces' partial sums, threads over pieces, then the
// lanes (tree) and the waves (in order)
template <int H>
__global__ void __launch_bounds__(64 * kMW) k_xgat_dz_merge_wg(const int32_t* __restrict__ hub_row,
                                                               const int32_t* __restrict__ hub_ptr,
                                                               const float* __restrict__ partial, float* __restrict__ S,
                                                               int64_t lds) {
  __shared__ float sr[kMW][H];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t hb = blockIdx.x;
  const int p0 = hub_ptr[hb], p1 = hub_ptr[hb + 1];
  float x[H];
#pragma unroll
  for (int h = 0; h < H; ++h) x[h] = 0.f;
  for (int q = p0 + tid; q < p1; q += 64 * kMW) {
#pragma unroll
    for (int h = 0; h < H; ++h) x[h] += partial[(int64_t)q * H + h];
  }
#pragma unroll
  for (int h = 0; h < H; ++h) {
    x[h] = wave_sum(x[h]);
    if (lane == 0) sr[w][h] = x[h];
  }
  __syncthreads();
  if (tid < H) {
    float v = 0.f;
    for (int k = 0; k < kMW; ++k) v += sr[k][tid];
    S[(int64_t)hub_row[hb] * lds + tid] = v;
  }
}

// dx_i += sum_h ds_dst_i^h A_dst[h] over the destination rows (S[i][H + h] = ds_dst)
template <int K, int H>
__global__ void __launch_bounds__(256) k_bwd_x_epi(const float* __restrict__ S, int64_t lds,
                                                   const float* __restrict__ A_dst, int64_t n, float* __restrict__ dx,
                                                   int64_t lddx) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t i = t / (K / 4);
  if (i >= n) return;
  const int c4 = (int)(t % (K / 4)) * 4;
  float4 v = ld4(dx + i * lddx + c4);
#pragma unroll
  for (int h = 0; h < H; ++h) v = fma4(S[i * lds + H + h], ld4(A_dst + h * K + c4), v);
  st4(dx + i * lddx + c4, v);
}

// dx[i][k] += sum_{v < nv} S[i][v] A[v][k] (v ascending): the rank-nv attention terms of a
// multi-head layer's input gradient, dx = D W + S [A_src; A_dst], after the D W GEMM.  One
// thread per float4 of dx, nv <= 16 runtime (the transform-then-aggregate layer, any K % 4).
__global__ void __launch_bounds__(256) k_rank_update(const float* __restrict__ S, int64_t lds, int nv,
                                                     const float* __restrict__ A, int64_t lda, int64_t n, int K,
                                                     float* __restrict__ dx, int64_t lddx) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int q = K / 4;
  const int64_t i = t / q;
  if (i >= n) return;
  const int c4 = (int)(t % q) * 4;
  float4 v = ld4(dx + i * lddx + c4);
  for (int r = 0; r < nv; ++r) v = fma4(S[i * lds + r], ld4(A + r * lda + c4), v);
  st4(dx + i * lddx + c4, v);
}

// dW[h C + c][k] = G[c][h K + k] * gs + att_src[h][c] GV[h][k] + att_dst[h][c] GV[H + h][k];
// datt_v[h][c] = sum_k W[h C + c][k] GV[v H + h][k].  One wave per (h, c) row of W.
__global__ void __launch_bounds__(256) k_wgrad_x(const float* __restrict__ G, const float* __restrict__ GV,
                                                 const float* __restrict__ W, const float* __restrict__ att_src,
                                                 const float* __restrict__ att_dst, int H, int C, int K, float gs,
                                                 float* __restrict__ dW, float* __restrict__ datt_src,
                                                 float* __restrict__ datt_dst) {
  const int lane = threadIdx.x & 63;
  const int64_t hc = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (hc >= (int64_t)H * C) return;
  const int h = (int)(hc / C), c = (int)(hc % C);
  const float as = att_src[hc], ad = att_dst[hc];
  float ps = 0.f, pd = 0.f;
  for (int k = lane; k < K; k += 64) {
    const float gs_ = GV[(int64_t)h * K + k], gd = GV[(int64_t)(H + h) * K + k];
    const float w = W[hc * K + k];
    dW[hc * K + k] = fmaf(G[(int64_t)c * H * K + (int64_t)h * K + k], gs, fmaf(as, gs_, ad * gd));
    ps = fmaf(w, gs_, ps);
    pd = fmaf(w, gd, pd);
  }
  ps = wave_sum(ps);
  pd = wave_sum(pd);
  if (lane == 0) {
    datt_src[hc] = ps;
    datt_dst[hc] = pd;
  }
}

// block partial column sums of Y [n, C] (dbias); reduced by k_col_reduce in block order
template <int C>
__global__ void __launch_bounds__(256) k_colsum_part(const float* __restrict__ Y, int64_t ldy, int64_t n,
                                                     float* __restrict__ part) {
  constexpr int LPR = C / 4, SPB = 256 / LPR;
  __shared__ float4 red[SPB][LPR];
  const int sg = threadIdx.x / LPR, sl = threadIdx.x % LPR;
  float4 s = f4(0.f);
  for (int64_t i = (int64_t)blockIdx.x * SPB + sg; i < n; i += (int64_t)gridDim.x * SPB)
    s = add4(s, ld4(Y + i * ldy + sl * 4));
  red[sg][sl] = s;
  __syncthreads();
  if (threadIdx.x < LPR) {
    float4 t = red[0][threadIdx.x];
    for (int q = 1; q < SPB; ++q) t = add4(t, red[q][threadIdx.x]);
    st4(part + ((int64_t)blockIdx.x * LPR + threadIdx.x) * 4, t);
  }
}

}  // namespace

bool xgat_shape_ok(int K, int H, int C) { return K == 256 && (H == 2 || H == 4) && C >= 128 && C % 128 == 0; }

#define PPGAT_XH(H_, ...)                                   \
  do {                                                      \
    if ((H_) == 2) { constexpr int HH = 2; __VA_ARGS__; }   \
    else { constexpr int HH = 4; __VA_ARGS__; }             \
  } while (0)

hipError_t xgat_weights(const float* W, const float* att_src, const float* att_dst, int H, int C, int K, float* A,
                        float* Wt, float* Wg, hipStream_t st) {
  const int64_t na = (int64_t)2 * H * K;
  if (A) hipLaunchKernelGGL(k_att_proj, dim3((unsigned)((na + 15) / 16)), dim3(256), 0, st, W, att_src, att_dst, H, C,
                            K, A);
  const int64_t nw = (int64_t)H * C * K;
  if (Wt || Wg) hipLaunchKernelGGL(k_wperm, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, st, W, H, C, K, Wt, Wg);
  return hipGetLastError();
}

hipError_t xgat_scores(const float* x, int64_t ldx, int64_t n_rows, int64_t n_dst, int K, int H, const float* A,
                       float* s_src, float* s_dst, hipStream_t st) {
  if (n_rows <= 0) return hipSuccess;
  int64_t blocks = (n_rows + 15) / 16;  // four rows per wave and iteration (K = 256), grid-stride
  if (blocks > 4096) blocks = 4096;
  PPGAT_XH(H, hipLaunchKernelGGL((k_xscores<256, HH>), dim3((unsigned)blocks), dim3(256), 0, st, x, ldx, n_rows, n_dst,
                                 A, s_src, s_dst));
  (void)K;
  return hipGetLastError();
}

hipError_t xgat_fwd(const ppgat_schedule& sch, const int32_t* col, const int32_t* eid, const float* x, int64_t ldx,
                    int K, int H, const float* s_src, const float* s_dst, float slope, float p, uint64_t seed,
                    const uint64_t* seed_in, float* agg, float* m, float* invl, float* partial, hipStream_t st,
                    unsigned* xmax) {
  const float inv_keep = p > 0.f ? 1.f / (1.f - p) : 1.f;
  const Items its = items_of(sch, sch.n_items);
  if (sch.n_items > 0)
    PPGAT_XH(H, hipLaunchKernelGGL((k_fwd_x<256, HH>), dim3((unsigned)((sch.n_items + 3) / 4)), dim3(256), 0, st, its,
                                   col, eid, x, ldx, s_src, s_dst, slope, p, inv_keep, seed, seed_in, agg, m, invl,
                                   partial, xmax));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  (void)K;
  if (sch.n_hubs > 0) {
    hipLaunchKernelGGL(k_fwd_merge_small, dim3((unsigned)((sch.n_hubs * H + 3) / 4)), dim3(256), 0, st, sch.hub_row,
                       sch.hub_ptr, sch.n_hubs, H, partial, 1e-16f, m, invl, agg);
    hipLaunchKernelGGL(k_fwd_merge_wg, dim3((unsigned)sch.n_hubs, (unsigned)H), dim3(64 * kMWf), 0, st, sch.hub_row,
                       sch.hub_ptr, H, partial, 1e-16f, m, invl, agg);
  }
  return hipGetLastError();
}

hipError_t xgat_bwd_pro(const float* gt, const float* agg, const float* s_dst, const float* m, const float* invl,
                        int64_t n, int K, int H, float* nstate, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  int64_t blocks = (n + 3) / 4;
  if (blocks > 8192) blocks = 8192;
  PPGAT_XH(H, hipLaunchKernelGGL((k_bwd_x_pro<256, HH>), dim3((unsigned)blocks), dim3(256), 0, st, gt, agg, s_dst, m,
                                 invl, n, reinterpret_cast<float4*>(nstate)));
  (void)K;
  return hipGetLastError();
}

hipError_t xgat_bwd_edges(const ppgat_schedule& sch, const int32_t* row, const int32_t* csc_eid, const int32_t* csc2csr,
                          const float* x, int64_t ldx, int K, int H, const float* s_src, const float* nstate,
                          const float* gt, const float* A_src, float slope, float p, uint64_t seed,
                          const uint64_t* seed_in, float* dx, int64_t lddx, float* S, int64_t lds, float* dz,
                          float* partial, hipStream_t st) {
  const float inv_keep = p > 0.f ? 1.f / (1.f - p) : 1.f;
  const Items its = items_of(sch, sch.n_items);
  if (sch.n_items > 0)
    PPGAT_XH(H, hipLaunchKernelGGL((k_bwd_x<256, HH>), dim3((unsigned)((sch.n_items + 3) / 4)), dim3(256), 0, st, its,
                                   row, csc_eid, csc2csr, x, ldx, s_src, reinterpret_cast<const float4*>(nstate), gt,
                                   A_src, slope, p, inv_keep, seed, seed_in, dx, lddx, S, lds, dz, partial));
  if (sch.n_hubs > 0)
    PPGAT_XH(H, hipLaunchKernelGGL((k_bwd_x_merge<256, HH>), dim3((unsigned)((sch.n_hubs + 3) / 4)), dim3(256), 0, st,
                                   sch.hub_row, sch.hub_ptr, sch.n_hubs, partial, A_src, dx, lddx, S, lds));
  (void)K;
  return hipGetLastError();
}

hipError_t xgat_bwd_edges_g(const ppgat_schedule& sch, const int32_t* row, const int32_t* csc_eid,
                            const int32_t* csc2csr, const float* hs, int C, int H, const float* s_src,
                            const float* nstate, const float* g, int64_t ldg, float slope, float p, uint64_t seed,
                            const uint64_t* seed_in, float* acc, float* S, int64_t lds, float* dz, float* partial,
                            hipStream_t st, float* pz, unsigned* gmax) {
  const float inv_keep = p > 0.f ? 1.f / (1.f - p) : 1.f;
  const Items its = items_of(sch, sch.n_items);
  if (sch.n_items > 0)
    PPGAT_XH(H, hipLaunchKernelGGL((k_bwd_g<256, HH>), dim3((unsigned)((sch.n_items + 3) / 4)), dim3(256), 0, st, its,
                                   row, csc_eid, csc2csr, hs, s_src, reinterpret_cast<const float4*>(nstate), g, ldg,
                                   slope, p, inv_keep, seed, seed_in, acc, S, lds, dz, partial, pz, gmax));
  if (sch.n_hubs > 0)
    PPGAT_XH(H, {
      hipLaunchKernelGGL((k_bwd_g_merge_small<256, HH>), dim3((unsigned)((sch.n_hubs * (HH + 1) + 3) / 4)), dim3(256),
                         0, st, sch.hub_row, sch.hub_ptr, sch.n_hubs, partial, acc, S, lds);
      hipLaunchKernelGGL((k_bwd_g_merge_wg<256, HH>), dim3((unsigned)sch.n_hubs, HH + 1), dim3(64 * kMWb), 0, st,
                         sch.hub_row, sch.hub_ptr, partial, acc, S, lds);
    });
  (void)C;
  return hipGetLastError();
}

// nstate[i][h].w = D[i][h] for every row of a table whose {s_dst, m, inv_l} came by exchange (the
// halo partition's deferred D: the completed D arrives as its own [rows, H] table).  One thread
// per (row, head); replaces a strided torch copy that ran at ~1 TB/s.
__global__ void __launch_bounds__(256) k_xgat_nstate_set_d(float* __restrict__ nstate, const float* __restrict__ D,
                                                           int64_t nh) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < nh) nstate[t * 4 + 3] = D[t];
}

hipError_t xgat_nstate_set_d(float* nstate, const float* D, int64_t n, int H, hipStream_t st) {
  const int64_t nh = n * H;
  if (nh > 0)
    hipLaunchKernelGGL(k_xgat_nstate_set_d, dim3((unsigned)((nh + 255) / 256)), dim3(256), 0, st, nstate, D, nh);
  return hipGetLastError();
}

hipError_t xgat_nstate(const float* s_dst, const float* m, const float* invl, const float* D, int64_t n, int H,
                       float* nstate, hipStream_t st) {
  const int64_t nh = n * H;
  if (nh > 0)
    hipLaunchKernelGGL(k_xgat_nstate, dim3((unsigned)((nh + 255) / 256)), dim3(256), 0, st, s_dst, m, invl, D, nh,
                       reinterpret_cast<float4*>(nstate));
  return hipGetLastError();
}

hipError_t xgat_bwd_dz(const ppgat_schedule& sch, const int32_t* row, const int32_t* csc_eid, const int32_t* csc2csr,
                       int H, const float* s_src, const float* nstate, float slope, float p, uint64_t seed,
                       const uint64_t* seed_in, float* dz, float* S, int64_t lds, float* partial, hipStream_t st) {
  const float inv_keep = p > 0.f ? 1.f / (1.f - p) : 1.f;
  const Items its = items_of(sch, sch.n_items);
  // [0, wl): hub pieces and long items, 16 lanes each; [wl, n_items): short items, 4 lanes each
  const int64_t wl =
      sch.n_long_items >= sch.n_hub_items && sch.n_long_items <= sch.n_items ? sch.n_long_items : sch.n_items;
  if (wl > 0)
    PPGAT_XH(H, hipLaunchKernelGGL((k_xgat_dz<HH, 16>), dim3((unsigned)((wl * 16 + 255) / 256)), dim3(256), 0, st,
                                   its, (int64_t)0, wl, row, csc_eid, csc2csr, s_src,
                                   reinterpret_cast<const float4*>(nstate), slope, p, inv_keep, seed, seed_in, dz, S,
                                   lds, partial));
  if (sch.n_items > wl)
    PPGAT_XH(H, hipLaunchKernelGGL((k_xgat_dz<HH, 4>), dim3((unsigned)(((sch.n_items - wl) * 4 + 255) / 256)),
                                   dim3(256), 0, st, its, wl, sch.n_items, row, csc_eid, csc2csr, s_src,
                                   reinterpret_cast<const float4*>(nstate), slope, p, inv_keep, seed, seed_in, dz, S,
                                   lds, partial));
  if (sch.n_hubs > 0)
    PPGAT_XH(H, hipLaunchKernelGGL((k_xgat_dz_merge_wg<HH>), dim3((unsigned)sch.n_hubs), dim3(64 * kMW), 0, st,
                                   sch.hub_row, sch.hub_ptr, partial, S, lds));
  return hipGetLastError();
}

hipError_t xgat_bwd_epi(const float* S, int64_t lds, const float* A_dst, int64_t n, int K, int H, float* dx,
                        int64_t lddx, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const int64_t th = n * (K / 4);
  PPGAT_XH(H, hipLaunchKernelGGL((k_bwd_x_epi<256, HH>), dim3((unsigned)((th + 255) / 256)), dim3(256), 0, st, S, lds,
                                 A_dst, n, dx, lddx));
  return hipGetLastError();
}

hipError_t att_proj(const float* W, const float* att_src, const float* att_dst, int H, int C, int K, float* A,
                    hipStream_t st) {
  const int64_t na = (int64_t)2 * H * K;
  if (na > 0) hipLaunchKernelGGL(k_att_proj, dim3((unsigned)((na + 15) / 16)), dim3(256), 0, st, W, att_src, att_dst,
                                 H, C, K, A);
  return hipGetLastError();
}

hipError_t rank_update(const float* S, int64_t lds, int nv, const float* A, int64_t lda, int64_t n, int K, float* dx,
                       int64_t lddx, hipStream_t st) {
  if (n <= 0 || nv <= 0) return hipSuccess;
  const int64_t th = n * (K / 4);
  hipLaunchKernelGGL(k_rank_update, dim3((unsigned)((th + 255) / 256)), dim3(256), 0, st, S, lds, nv, A, lda, n, K, dx,
                     lddx);
  return hipGetLastError();
}

hipError_t xgat_wgrad(const float* G, const float* GV, const float* W, const float* att_src, const float* att_dst,
                      int H, int C, int K, float* dW, float* datt_src, float* datt_dst, hipStream_t st) {
  const int64_t rows = (int64_t)H * C;
  hipLaunchKernelGGL(k_wgrad_x, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, G, GV, W, att_src, att_dst, H, C,
                     K, 1.f / (float)H, dW, datt_src, datt_dst);
  return hipGetLastError();
}

int64_t colsum_blocks(int64_t n) {
  int64_t b = (n + 63) / 64;
  return b < 1 ? 1 : (b > 1024 ? 1024 : b);
}

hipError_t colsum(const float* Y, int64_t ldy, int64_t n, int C, float* out, float* part, hipStream_t st) {
  const int64_t blocks = colsum_blocks(n);
  if (C == 256) hipLaunchKernelGGL((k_colsum_part<256>), dim3((unsigned)blocks), dim3(256), 0, st, Y, ldy, n, part);
  else if (C == 128) hipLaunchKernelGGL((k_colsum_part<128>), dim3((unsigned)blocks), dim3(256), 0, st, Y, ldy, n, part);
  else return hipErrorInvalidValue;
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_col_reduce(part, blocks, C, C, out, nullptr, st);
}

}  // namespace ppgat
