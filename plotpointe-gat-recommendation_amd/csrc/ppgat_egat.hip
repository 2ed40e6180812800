// ppgat_egat.hip -- GATConv edge features (edge_dim = D <= 16) around the fused edge kernels.
//
// PyG: a_e[k, h] = sum_c lin_edge(edge_attr[k])[h, c] att_edge[h, c], added to the logit.  With
//   v[h, d] = sum_c att_edge[h, c] W_e[h C + c, d]   [H, D]   (formed by the caller)
// this is a_e[k, h] = <edge_attr[k, :], v[h, :]>.  Three kernels:
//   k_attr_permute  edge_attr [E, D] -> slot order of a CSR or CSC view, once per (graph, tensor):
//                   every later access is a per-lane read of consecutive slots, no gather by edge id
//   k_edge_terms    per step: t_csr[k, h] and t_csc[k, h] from the two staged tables and v; the
//                   edge kernels (ppgat_kernels.hip, EDGE instantiations) then read one float per
//                   (slot, head) and do not depend on D.  Both tables take the same fmaf chain
//                   over d, so an edge's term has the same bits in the forward and in pass B.
//   k_edge_dv       dv[h, d] = sum_k dz[k, h] attr_csc[k, d] over a fixed grid: one partial row
//                   per block (lanes by butterfly, waves in order), blocks summed in block order
//                   by k_col_reduce -- no float atomics, the same bits on every launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ppgat_internal.h"
#include "ppgat_lanes.h"
#include "ppgat_device.h"

namespace ppgat {

constexpr int kEdgeMaxD = 16;  // include/ppgat.h PPGAT_EDGE_MAX_DIM

__global__ void __launch_bounds__(256) k_attr_permute(const float* __restrict__ attr,
                                                      const int32_t* __restrict__ eid, int64_t n, int D,
                                                      float* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // one element of out [E, D]
  if (t >= n) return;
  const int64_t k = t / D;
  const int d = (int)(t - k * D);
  out[t] = attr[(int64_t)eid[k] * D + d];
}

// blockIdx.y: 0 the CSR table, 1 the CSC table; one thread per slot
__global__ void __launch_bounds__(256) k_edge_terms(const float* __restrict__ attr_csr,
                                                    const float* __restrict__ attr_csc,
                                                    const float* __restrict__ v, int64_t E, int D, int H,
                                                    float* __restrict__ t_csr, float* __restrict__ t_csc) {
  __shared__ float vs[kMaxHeads * kEdgeMaxD];
  for (int t = threadIdx.x; t < H * D; t += blockDim.x) vs[t] = v[t];
  __syncthreads();
  const float* attr = blockIdx.y == 0 ? attr_csr : attr_csc;
  float* out = blockIdx.y == 0 ? t_csr : t_csc;
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= E) return;
  float a[kEdgeMaxD];
#pragma unroll
  for (int d = 0; d < kEdgeMaxD; ++d) a[d] = d < D ? attr[k * D + d] : 0.f;
  for (int hd = 0; hd < H; ++hd) {
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < kEdgeMaxD; ++d)
      if (d < D) s = fmaf(a[d], vs[hd * D + d], s);
    out[k * H + hd] = s;
  }
}

__global__ void __launch_bounds__(256) k_edge_dv(const float* __restrict__ dz, const float* __restrict__ attr,
                                                 int64_t E, int H, int D, float* __restrict__ part) {
  __shared__ float red[4][kEdgeMaxD];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int hd = 0; hd < H; ++hd) {
    float acc[kEdgeMaxD];
#pragma unroll
    for (int d = 0; d < kEdgeMaxD; ++d) acc[d] = 0.f;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < E; k += stride) {
      const float z = dz[k * H + hd];
#pragma unroll
      for (int d = 0; d < kEdgeMaxD; ++d)
        if (d < D) acc[d] = fmaf(z, attr[k * D + d], acc[d]);
    }
#pragma unroll
    for (int d = 0; d < kEdgeMaxD; ++d) {
      const float s = wave_sum(acc[d]);
      if (lane == 0) red[wv][d] = s;
    }
    __syncthreads();
    if (threadIdx.x < D) {
      const int d = threadIdx.x;
      part[((int64_t)blockIdx.x * H + hd) * D + d] = ((red[0][d] + red[1][d]) + red[2][d]) + red[3][d];
    }
    __syncthreads();
  }
}

hipError_t edge_attr_permute(const float* attr, const int32_t* eid, int64_t E, int D, float* out, hipStream_t st) {
  const int64_t n = E * D;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_attr_permute, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, attr, eid, n, D, out);
  return hipGetLastError();
}

hipError_t edge_terms(const float* attr_csr, const float* attr_csc, const float* v, int64_t E, int D, int H,
                      float* t_csr, float* t_csc, hipStream_t st) {
  if (E <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_edge_terms, dim3((unsigned)((E + 255) / 256), t_csc != nullptr ? 2u : 1u), dim3(256), 0, st,
                     attr_csr, attr_csc, v, E, D, H, t_csr, t_csc);
  return hipGetLastError();
}

// fixed partition: a function of E alone, capped so the partial slab stays small
int64_t edge_dv_blocks(int64_t E) {
  int64_t b = (E + 2047) / 2048;
  if (b < 1) b = 1;
  if (b > 1024) b = 1024;
  return b;
}

hipError_t edge_dv(const float* dz, const float* attr, int64_t E, int H, int D, float* dv, float* part,
                   hipStream_t st) {
  const int64_t blocks = edge_dv_blocks(E);
  hipLaunchKernelGGL(k_edge_dv, dim3((unsigned)blocks), dim3(256), 0, st, dz, attr, E, H, D, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_col_reduce(part, blocks, H * D, H * D, dv, nullptr, st);
}

}  // namespace ppgat
