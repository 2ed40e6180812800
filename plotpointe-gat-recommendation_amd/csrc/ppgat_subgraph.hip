// ppgat_subgraph.hip -- seed-subgraph sampling: the L-hop sampled in-neighbourhood of a seed set,
// relabelled into a small graph (include/ppgat.h "seed-subgraph sampling").
//
// Replaces: nothing in the reference (it trains on the whole graph at every step).  The sampler of
// ppgat_nsample.hip keeps a row's sample a function of (seed, i, d, f) alone, so the subgraph of a
// seed set is a restriction of the whole sampled graph:
//   seed    depth = -1 everywhere, 0 at the seeds; an out-of-range seed raises a flag       (N, T)
//   expand  one launch per hop h: the rows of depth h mark the sources of their kept slots
//           with depth h + 1 where none is set yet (d <= f: every slot; d > f: Floyd's
//           subset, one wave per row, keyed by the node's global id)                        (N, kept)
//   plan    the cap table (the cap of the rows of depth < L, 0 elsewhere) for
//           ppgat_neighbor_count / _sample / _derive, and newnode = exclusive scan of
//           (depth >= 0): the relabel map, N_s and the user count                           (N)
//   relabel the pointers compacted to the kept nodes; col / row / edge_index_s through
//           the map, in place; n_id, depth, seed_local                                      (N, E_s, T)
// Relabelling is monotone, so slot orders do not change and no sort is needed.  Integers only, no
// atomics: a depth or a flag may be stored by several threads, always with the same value.
// wave64 throughout.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "ppgat_floyd.h"
#include "ppgat_internal.h"

namespace ppgat {
namespace {

constexpr int kRows = 256;  // destination rows per block of the expansion

inline size_t align_up(size_t b) { return (b + 255) & ~size_t(255); }

struct Reached {
  __host__ __device__ int32_t operator()(int32_t depth) const { return depth >= 0 ? 1 : 0; }
};

using ReachedIt = rocprim::transform_iterator<const int32_t*, Reached, int32_t>;

// the workspace: depth [N + 1] (entry N stays -1: the scan's last input), newnode [N + 1], scan temp
struct Carve {
  int32_t* depth;
  int32_t* newnode;
  void* tmp;
  size_t tmp_bytes;
};

size_t scan_temp_bytes(int64_t N) {
  size_t b = 0;
  (void)rocprim::exclusive_scan(nullptr, b, ReachedIt((const int32_t*)nullptr, Reached()), (int32_t*)nullptr,
                                (int32_t)0, (size_t)(N + 1), rocprim::plus<int32_t>());
  return b;
}

size_t carve(int64_t N, void* ws, size_t ws_bytes, Carve* out) {
  const size_t n4 = align_up((size_t)(N + 1) * 4);
  if (out != nullptr) {
    char* p = static_cast<char*>(ws);
    out->depth = reinterpret_cast<int32_t*>(p);
    out->newnode = reinterpret_cast<int32_t*>(p + n4);
    out->tmp = p + 2 * n4;
    out->tmp_bytes = ws_bytes - 2 * n4;
  }
  return 2 * n4 + align_up(scan_temp_bytes(N));
}

// the cap of destination i with in-degree d (k_count's rule, include/ppgat.h)
__device__ __forceinline__ int32_t cap_of(int fanout, const int32_t* __restrict__ fanout_of, int64_t i, int32_t d) {
  if (fanout_of == nullptr) return fanout;
  const int32_t v = fanout_of[i];
  return v < 0 ? d : min(v, kMaxFanout);
}

__global__ void __launch_bounds__(256) k_seed(const int64_t* __restrict__ seeds, int64_t T, int64_t N,
                                              int32_t* __restrict__ depth, int32_t* __restrict__ bad) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  const int64_t v = seeds[t];
  if (v < 0 || v >= N)
    *bad = 1;
  else
    depth[v] = 0;
}

// One block per kRows destination rows; the rows of depth `hop` that have in-edges are listed in
// LDS by ballot and take one wave each.  d <= f: the wave strides over the row's slots.  d > f:
// Floyd's subset, lane s holding element s.  A source without a depth gets hop + 1; one that has a
// depth keeps it (it is <= hop + 1: the frontier is expanded hop by hop).
__global__ void __launch_bounds__(256) k_expand(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                int64_t N, int hop, int fanout,
                                                const int32_t* __restrict__ fanout_of, uint64_t seed,
                                                int32_t* __restrict__ depth) {
  __shared__ int32_t s_act[kRows], s_wc[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * kRows;
  const int64_t row = r0 + tid;
  bool act = false;
  if (row < N && depth[row] == hop) act = rowptr[row + 1] > rowptr[row];
  const uint64_t bm = __ballot(act);
  if (lane == 0) s_wc[wave] = (int32_t)__popcll(bm);
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += s_wc[w];
  const int nact = s_wc[0] + s_wc[1] + s_wc[2] + s_wc[3];
  if (act) s_act[base + (int)__popcll(bm & ((1ull << lane) - 1))] = tid;
  __syncthreads();
  for (int q = wave; q < nact; q += 4) {
    const int r = __builtin_amdgcn_readfirstlane(s_act[q]);
    const int64_t i = r0 + r;
    const int32_t b = __builtin_amdgcn_readfirstlane(rowptr[i]);
    const int32_t d = __builtin_amdgcn_readfirstlane(rowptr[i + 1]) - b;
    const int32_t f = __builtin_amdgcn_readfirstlane(cap_of(fanout, fanout_of, i, d));
    if (f <= 0) continue;
    if (d <= f) {
      for (int32_t p = lane; p < d; p += 64) {
        const int32_t s = col[b + p];
        if (depth[s] < 0) depth[s] = hop + 1;
      }
    } else {
      const int32_t val = floyd_wave(seed, (uint64_t)i, d, f, lane);
      if (lane < f) {
        const int32_t s = col[b + val];
        if (depth[s] < 0) depth[s] = hop + 1;
      }
    }
  }
}

// cap[i] = the cap of row i where 0 <= depth[i] < hops (fanout without a table), 0 elsewhere;
// bad_fanout = 1 where a fanout_of entry exceeds kMaxFanout, whatever the row's depth
__global__ void __launch_bounds__(256) k_cap(const int32_t* __restrict__ depth, int64_t N, int hops, int fanout,
                                             const int32_t* __restrict__ fanout_of, int32_t* __restrict__ cap,
                                             int32_t* __restrict__ bad_fanout) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  int32_t f = fanout;
  if (fanout_of != nullptr) {
    f = fanout_of[i];
    if (f > kMaxFanout) *bad_fanout = 1;
  }
  const int32_t dp = depth[i];
  cap[i] = dp >= 0 && dp < hops ? f : 0;
}

__global__ void k_counts(const int32_t* __restrict__ newnode, int64_t N, int64_t n_users, int32_t* __restrict__ info) {
  info[0] = newnode[N];
  info[1] = newnode[n_users];
}

// the node side of the relabel: thread v < N with a depth writes its new row, thread N the two ends
__global__ void __launch_bounds__(256) k_nodes(const int32_t* __restrict__ depth, const int32_t* __restrict__ newnode,
                                               int64_t N, int64_t Ns, int64_t Es,
                                               const int32_t* __restrict__ rowptr_p,
                                               const int32_t* __restrict__ colptr_p, int64_t* __restrict__ n_id,
                                               int32_t* __restrict__ depth_s, int32_t* __restrict__ rowptr_s,
                                               int32_t* __restrict__ colptr_s) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v > N) return;
  if (v == N) {
    rowptr_s[Ns] = (int32_t)Es;
    colptr_s[Ns] = (int32_t)Es;
    return;
  }
  const int32_t dp = depth[v];
  if (dp < 0) return;
  const int32_t n = newnode[v];
  if (n >= Ns) return;  // a caller's n_sub below the plan's count: nothing past the stated length
  n_id[n] = v;
  depth_s[n] = dp;
  rowptr_s[n] = rowptr_p[v];
  colptr_s[n] = colptr_p[v];
}

// the edge side, in place: every endpoint of a kept edge has a depth, so its newnode entry is its id
__global__ void __launch_bounds__(256) k_edges(const int32_t* __restrict__ newnode, int64_t Es,
                                               int32_t* __restrict__ col_s, int32_t* __restrict__ row_s,
                                               int64_t* __restrict__ ei_s) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= Es) return;
  col_s[k] = newnode[col_s[k]];
  row_s[k] = newnode[row_s[k]];
  ei_s[k] = newnode[ei_s[k]];
  ei_s[Es + k] = newnode[ei_s[Es + k]];
}

__global__ void __launch_bounds__(256) k_seed_local(const int64_t* __restrict__ seeds, int64_t T, int64_t N,
                                                    const int32_t* __restrict__ newnode,
                                                    int64_t* __restrict__ seed_local) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  const int64_t v = seeds[t];
  seed_local[t] = v >= 0 && v < N ? (int64_t)newnode[v] : -1;
}

inline unsigned grid(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

size_t subgraph_workspace_bytes(int64_t N) { return carve(N, nullptr, 0, nullptr); }

hipError_t subgraph_seed(const int64_t* seeds, int64_t T, int64_t N, int32_t* info, void* ws, size_t ws_bytes,
                         hipStream_t st) {
  Carve c;
  if (ws_bytes < carve(N, ws, ws_bytes, &c)) return hipErrorInvalidValue;
  hipError_t err = hipMemsetAsync(info, 0, 4 * sizeof(int32_t), st);
  if (err != hipSuccess) return err;
  err = hipMemsetAsync(c.depth, 0xFF, (size_t)(N + 1) * sizeof(int32_t), st);
  if (err != hipSuccess) return err;
  if (T > 0) hipLaunchKernelGGL(k_seed, dim3(grid(T)), dim3(256), 0, st, seeds, T, N, c.depth, info + 2);
  return hipGetLastError();
}

hipError_t subgraph_expand(const int32_t* rowptr, const int32_t* col, int64_t N, int hop, int fanout,
                           const int32_t* fanout_of, uint64_t seed, void* ws, size_t ws_bytes, hipStream_t st) {
  Carve c;
  if (ws_bytes < carve(N, ws, ws_bytes, &c)) return hipErrorInvalidValue;
  if (N == 0) return hipSuccess;
  hipLaunchKernelGGL(k_expand, dim3((unsigned)((N + kRows - 1) / kRows)), dim3(256), 0, st, rowptr, col, N, hop,
                     fanout, fanout_of, seed, c.depth);
  return hipGetLastError();
}

hipError_t subgraph_plan(int64_t N, int64_t n_users, int hops, int fanout, const int32_t* fanout_of, int32_t* cap,
                         int32_t* info, void* ws, size_t ws_bytes, hipStream_t st) {
  Carve c;
  if (ws_bytes < carve(N, ws, ws_bytes, &c)) return hipErrorInvalidValue;
  if (N > 0)
    hipLaunchKernelGGL(k_cap, dim3(grid(N)), dim3(256), 0, st, c.depth, N, hops, fanout, fanout_of, cap, info + 3);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  size_t tmp_bytes = c.tmp_bytes;
  err = rocprim::exclusive_scan(c.tmp, tmp_bytes, ReachedIt(c.depth, Reached()), c.newnode, (int32_t)0,
                                (size_t)(N + 1), rocprim::plus<int32_t>(), st);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(k_counts, dim3(1), dim3(1), 0, st, c.newnode, N, n_users, info);
  return hipGetLastError();
}

hipError_t subgraph_relabel(int64_t N, int64_t Ns, int64_t Es, const int64_t* seeds, int64_t T,
                            const int32_t* rowptr_p, const int32_t* colptr_p, int64_t* n_id, int32_t* depth_s,
                            int32_t* rowptr_s, int32_t* colptr_s, int32_t* col_s, int32_t* row_s, int64_t* ei_s,
                            int64_t* seed_local, void* ws, size_t ws_bytes, hipStream_t st) {
  Carve c;
  if (ws_bytes < carve(N, ws, ws_bytes, &c)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_nodes, dim3(grid(N + 1)), dim3(256), 0, st, c.depth, c.newnode, N, Ns, Es, rowptr_p, colptr_p,
                     n_id, depth_s, rowptr_s, colptr_s);
  if (Es > 0) hipLaunchKernelGGL(k_edges, dim3(grid(Es)), dim3(256), 0, st, c.newnode, Es, col_s, row_s, ei_s);
  if (T > 0) hipLaunchKernelGGL(k_seed_local, dim3(grid(T)), dim3(256), 0, st, seeds, T, N, c.newnode, seed_local);
  return hipGetLastError();
}

}  // namespace ppgat
