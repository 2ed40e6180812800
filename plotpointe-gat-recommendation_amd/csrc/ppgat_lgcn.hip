// ppgat_lgcn.hip -- LightGCN propagation hop for CDNA4 (gfx950, MI355X).
//
// Replaces one iteration of LightGCN.propagate (scripts/train_lightgcn.py:69-72):
//   out = torch.sparse.mm(A, out); acc = acc + out        (and :73, acc / (K + 1), on the last)
// as one weighted sparse product with the layer-mean epilogue fused in.  For every
// destination row i of a CSR (rowptr through a work schedule, col, a value per slot):
//   s_i     = sum_{k in row i, slot order} val[k] * src[col[k]]       fp32 FMAs
//   out[i]  = s_i                                  when out  != NULL
//   accw[i] = (acc_in[i] + s_i) / div              when accw != NULL (IEEE division, div != 1)
// The backward of a K-hop propagate is the same recurrence over the CSC view (A^T).
//
// Work decomposition as in ppgat_kernels.hip (k_fwd / k_fwd_short): items with more than
// kShortItemEdges edges take one wavefront each, C/4 lanes x float4 per row ("subgroup"),
// 64/(C/4) subgroups on different edges of the row with U gathers in flight each; col and
// val of a 64-edge chunk are staged in LDS.  Short items run four per wavefront, one per
// 16-lane row, kSU neighbour rows in flight each.  Hub rows arrive cut into pieces; a piece
// writes its partial row to the caller's workspace and the pieces are added in piece order
// by one wave per hub (at the head of the short-item launch when there is one).
// The gather is latency-bound (the table sits in the Infinity Cache at the reference's size:
// 255k rows x 256 B = 65 MB), so what matters is rows in flight per wave, not arithmetic.
// No float atomics: every sum is owned by one wave in a fixed order, so two launches give
// the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ppgat_internal.h"
#include "ppgat_lanes.h"
#include "ppgat_device.h"

namespace ppgat {
namespace {

constexpr int kSU = 4;  // neighbour rows in flight per short item (per 16-lane row)

__device__ __forceinline__ float4 div4(float4 a, float d) { return make_float4(a.x / d, a.y / d, a.z / d, a.w / d); }

template <int C>
struct Geo {
  static constexpr int LPR = C / 4;                   // lanes per row (float4 each)
  static constexpr int EPW = 64 / LPR;                // edges side by side per wave
  static constexpr int U = EPW >= 2 ? 4 : 8;          // gathers in flight per subgroup
  static_assert(C == 64 || C == 128 || C == 256, "lgcn: C in {64, 128, 256}");
  static_assert(64 % (EPW * U) == 0, "chunk tiling");
};

// a table given as two row segments: rows [0, split) at p0, the rest at p1
struct Rows {
  const float* p0;
  const float* p1;
  int split;
};
template <int C>
__device__ __forceinline__ const float* row_of(const Rows& r, int j) {
  return j < r.split ? r.p0 + (int64_t)j * C : r.p1 + (int64_t)(j - r.split) * C;
}

// out / accw of one finished row.  accw may be acc_in's own buffer (in-place running sum):
// each element is read and then written by the same lane.
struct Epi {
  Rows acc;     // acc.p0 == NULL: acc_in = 0
  float div;
  float* out;   // nullable
  float* accw;  // nullable
};
template <int C>
__device__ __forceinline__ void finish(const Epi& e, int i, int col4, float4 s) {
  if (e.out != nullptr) st4(e.out + (int64_t)i * C + col4, s);
  if (e.accw != nullptr) {
    const float4 a = e.acc.p0 != nullptr ? ld4s(row_of<C>(e.acc, i) + col4) : f4(0.f);
    float4 r = add4(a, s);
    if (e.div != 1.f) r = div4(r, e.div);
    st4s(e.accw + (int64_t)i * C + col4, r);
  }
}

// one wave per item: a destination row with more than kShortItemEdges edges, or a hub piece
template <int C>
__global__ void __launch_bounds__(256) k_lgcn_long(Items it, const int32_t* __restrict__ col,
                                                   const float* __restrict__ val, Rows src, Epi epi,
                                                   float* __restrict__ partial) {
  using G = Geo<C>;
  __shared__ int2 rec[4][64];  // per wave: chunk edges {src row, value}
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t w = (int64_t)blockIdx.x * (blockDim.x >> 6) + wv;
  if (w >= it.n_items) return;  // wave-uniform
  const int sg = lane / G::LPR, sl = lane % G::LPR;
  const int i = it.row[w];
  const int rs = it.beg[w], re = it.end[w];
  float4 acc = f4(0.f);
  for (int base = rs; base < re; base += 64) {
    const int k = base + lane;
    const bool valid = k < re;
    rec[wv][lane] = make_int2(valid ? col[k] : 0, valid ? __float_as_int(val[k]) : 0);
    wave_sync();
    const int n = min(64, re - base);
    for (int q0 = 0; q0 < n; q0 += G::EPW * G::U) {
      float4 v[G::U];
      float wq[G::U];
#pragma unroll
      for (int u = 0; u < G::U; ++u) {
        const int q = q0 + u * G::EPW + sg;  // < 64: the chunk tiling divides 64
        const int2 r = rec[wv][q];
        wq[u] = __int_as_float(r.y);
        v[u] = q < n ? ld4(row_of<C>(src, r.x) + sl * 4) : f4(0.f);
      }
#pragma unroll
      for (int u = 0; u < G::U; ++u) acc = fma4(wq[u], v[u], acc);
    }
    wave_sync();
  }
  acc = across_subgroups<G::LPR>(acc);
  if (sg != 0) return;
  if (w < it.n_hub_items) st4(partial + w * C + sl * 4, acc);
  else finish<C>(epi, i, sl * 4, acc);
}

// the pieces of one hub row added in piece order; lanes [0, C/4) of the wave
template <int C>
__device__ __forceinline__ void merge_wave(int64_t hb, const int32_t* __restrict__ hub_row,
                                           const int32_t* __restrict__ hub_ptr,
                                           const float* __restrict__ partial, const Epi& epi) {
  const int lane = threadIdx.x & 63;
  if (lane >= C / 4) return;
  const int i = hub_row[hb];
  const int p0 = hub_ptr[hb], p1 = hub_ptr[hb + 1];
  float4 acc = f4(0.f);
  int q = p0;
  for (; q + 4 <= p1; q += 4) {
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = ld4(partial + (int64_t)(q + u) * C + lane * 4);
#pragma unroll
    for (int u = 0; u < 4; ++u) acc = add4(acc, v[u]);
  }
  for (; q < p1; ++q) acc = add4(acc, ld4(partial + (int64_t)q * C + lane * 4));
  finish<C>(epi, i, lane * 4, acc);
}

struct HubMerge {
  const int32_t* hub_row;
  const int32_t* hub_ptr;
  int64_t n_hubs;
  const float* partial;
  int64_t mblocks;  // blocks [0, mblocks) of the short-item launch merge hubs, one per wave
};

template <int C>
__global__ void __launch_bounds__(256) k_lgcn_merge(HubMerge mg, Epi epi) {
  const int64_t hb = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (hb < mg.n_hubs) merge_wave<C>(hb, mg.hub_row, mg.hub_ptr, mg.partial, epi);
}

// short items (<= kShortItemEdges edges): four per wave, one per 16-lane row.  Lane ql stages
// slot rs + ql and takes the float4 columns ql, ql + 16, ... of every neighbour row.
template <int C>
__global__ void __launch_bounds__(256) k_lgcn_short(Items it, int64_t first, const int32_t* __restrict__ col,
                                                    const float* __restrict__ val, Rows src, Epi epi,
                                                    HubMerge mg) {
  constexpr int NV = C / 64;  // float4 columns per lane
  __shared__ int2 rec[4][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if ((int64_t)blockIdx.x < mg.mblocks) {
    const int64_t hb = (int64_t)blockIdx.x * 4 + wv;
    if (hb < mg.n_hubs) merge_wave<C>(hb, mg.hub_row, mg.hub_ptr, mg.partial, epi);
    return;
  }
  const int qr = lane >> 4, ql = lane & 15;
  const int64_t item = first + (((int64_t)blockIdx.x - mg.mblocks) * 4 + wv) * 4 + qr;
  const bool live = item < it.n_items;
  const int64_t ic = live ? item : first;
  const int i = it.row[ic];
  const int rs = it.beg[ic], re = live ? it.end[ic] : rs;
  const int n = min(re - rs, kShortItemEdges);  // the schedule's bound; never past the 16 staged slots
  const int k = rs + ql;
  const bool valid = ql < n;
  rec[wv][lane] = make_int2(valid ? col[k] : 0, valid ? __float_as_int(val[k]) : 0);
  wave_sync();
  const int2* rq = &rec[wv][qr * 16];
  float4 acc[NV];
#pragma unroll
  for (int c = 0; c < NV; ++c) acc[c] = f4(0.f);
  for (int t0 = 0; t0 < n; t0 += kSU) {
    float4 v[kSU][NV];
    float wt[kSU];
#pragma unroll
    for (int u = 0; u < kSU; ++u) {
      const int t = t0 + u;
      const int2 r = rq[t & 15];
      wt[u] = t < n ? __int_as_float(r.y) : 0.f;
      const float* p = row_of<C>(src, r.x);
#pragma unroll
      for (int c = 0; c < NV; ++c) v[u][c] = t < n ? ld4(p + (ql + 16 * c) * 4) : f4(0.f);
    }
#pragma unroll
    for (int u = 0; u < kSU; ++u)
#pragma unroll
      for (int c = 0; c < NV; ++c) acc[c] = fma4(wt[u], v[u][c], acc[c]);
  }
  if (!live) return;
#pragma unroll
  for (int c = 0; c < NV; ++c) finish<C>(epi, i, (ql + 16 * c) * 4, acc[c]);
}

inline unsigned blocks_for(int64_t threads) { return (unsigned)((threads + 255) / 256); }

inline Rows rows_arg(const float* p0, const float* p1, int64_t split) {
  if (p1 == nullptr) return Rows{p0, p0, INT32_MAX};
  return Rows{p0, p1, (int)split};
}

template <int C>
hipError_t hop(const ppgat_schedule& sch, const int32_t* col, const float* val, const Rows& src, const Epi& epi,
               float* partial, hipStream_t st) {
  // first item of the four-per-wave path (n_items when the schedule does not know it)
  int64_t n_long = sch.n_long_items;
  if (n_long < sch.n_hub_items || n_long > sch.n_items) n_long = sch.n_items;
  const Items its = items_of(sch, n_long);
  if (n_long > 0)
    hipLaunchKernelGGL(k_lgcn_long<C>, dim3(blocks_for(n_long * 64)), dim3(256), 0, st, its, col, val, src, epi,
                       partial);
  const bool fold = n_long < sch.n_items;
  HubMerge mg{sch.hub_row, sch.hub_ptr, sch.n_hubs, partial, sch.n_hubs > 0 ? (sch.n_hubs + 3) / 4 : 0};
  if (fold) {
    const Items all = items_of(sch, sch.n_items);
    const unsigned g = (unsigned)((sch.n_items - n_long + 15) / 16 + mg.mblocks);  // 4 waves x 4 items per block
    hipLaunchKernelGGL(k_lgcn_short<C>, dim3(g), dim3(256), 0, st, all, n_long, col, val, src, epi, mg);
  } else if (sch.n_hubs > 0) {
    hipLaunchKernelGGL(k_lgcn_merge<C>, dim3((unsigned)mg.mblocks), dim3(256), 0, st, mg, epi);
  }
  return hipGetLastError();
}

}  // namespace

bool lgcn_channels_ok(int C) { return C == 64 || C == 128 || C == 256; }

size_t lgcn_workspace_bytes(int64_t n_hub_items, int C) {
  return (((size_t)(n_hub_items > 0 ? n_hub_items : 1) * C * 4) + 255) & ~size_t(255);
}

hipError_t lgcn_hop(const ppgat_schedule& sch, const int32_t* col, const float* val, int C, const float* src0,
                    const float* src1, int64_t src_split, const float* acc0, const float* acc1, int64_t acc_split,
                    float div, float* out, float* accw, float* partial, hipStream_t st) {
  if (sch.n_items <= 0) return hipSuccess;
  const Rows src = rows_arg(src0, src1, src_split);
  const Epi epi{acc0 != nullptr ? rows_arg(acc0, acc1, acc_split) : Rows{nullptr, nullptr, 0}, div, out, accw};
  switch (C) {
    case 64: return hop<64>(sch, col, val, src, epi, partial, st);
    case 128: return hop<128>(sch, col, val, src, epi, partial, st);
    case 256: return hop<256>(sch, col, val, src, epi, partial, st);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace ppgat
