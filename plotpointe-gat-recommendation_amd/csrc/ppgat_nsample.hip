// ppgat_nsample.hip -- fan-out neighbour sampling: a sampled graph's CSR / CSC views compacted
// out of its parent's (include/ppgat.h "fan-out neighbour sampling").
//
// Replaces: nothing in the reference (it trains on the whole graph at every step); what it spares
// is csr_build's two radix sorts over a resampled edge_index each epoch.  A sampled graph keeps a
// subset of its parent's edges and a stable sort of a subset is the subset of the stable sort, so
// every view follows from the parent's by a scan of keep flags and a streaming scatter:
//   count   rowptr' = exclusive scan of min(d, f)                              (N)
//   pick    the kept slots of each row straight into its CSR' range; keep flags by edge id
//           and by CSC slot (through the parent's csr2csc)                     (E')
//   renum   newid = exclusive scan of keep in edge-id order; COO' and eid      (E)
//   derive  the CSC side: scan of the CSC-order keep flags, scatter            (E)
// Integers only, no atomics on data: deterministic.  wave64 throughout.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "ppgat_floyd.h"
#include "ppgat_internal.h"

namespace ppgat {
namespace {

constexpr int kRows = 256;  // destination rows per block of the pick

inline size_t align_up(size_t b) { return (b + 255) & ~size_t(255); }

struct ByteFlag {
  __host__ __device__ int32_t operator()(uint8_t v) const { return (int32_t)v; }
};

using ByteIt = rocprim::transform_iterator<const uint8_t*, ByteFlag, int32_t>;

// the carried workspace: keep [E] bytes (by edge id), keepc [E] bytes (by CSC slot), newid [E],
// newslot [E], cscpos [E], scan temp.  The count runs before any of it is live and takes cnt [N + 1]
// and its scan temp from the front.
struct Carve {
  uint8_t* keep;
  uint8_t* keepc;
  int32_t* newid;
  int32_t* newslot;
  int32_t* cscpos;
  void* tmp;
  size_t tmp_bytes;
};

size_t count_temp_bytes(int64_t N) {
  size_t a = 0;
  (void)rocprim::exclusive_scan(nullptr, a, (int32_t*)nullptr, (int32_t*)nullptr, (int32_t)0, (size_t)(N + 1),
                                rocprim::plus<int32_t>());
  return a;
}

size_t count_bytes(int64_t N) { return align_up((size_t)(N + 1) * 4) + align_up(count_temp_bytes(N)); }

size_t scan_temp_bytes(int64_t E) {
  size_t b = 0;
  const size_t e = (size_t)(E > 0 ? E : 1);
  (void)rocprim::exclusive_scan(nullptr, b, ByteIt((const uint8_t*)nullptr, ByteFlag()), (int32_t*)nullptr,
                                (int32_t)0, e, rocprim::plus<int32_t>());
  return b;
}

size_t carve(int64_t E, void* ws, size_t ws_bytes, Carve* out) {
  const size_t e = (size_t)(E > 0 ? E : 1);
  const size_t e1 = align_up(e), e4 = align_up(e * 4);
  const size_t fixed = 2 * e1 + 3 * e4;
  if (out != nullptr) {
    char* p = static_cast<char*>(ws);
    out->keep = reinterpret_cast<uint8_t*>(p);
    out->keepc = reinterpret_cast<uint8_t*>(p + e1);
    out->newid = reinterpret_cast<int32_t*>(p + 2 * e1);
    out->newslot = reinterpret_cast<int32_t*>(p + 2 * e1 + e4);
    out->cscpos = reinterpret_cast<int32_t*>(p + 2 * e1 + 2 * e4);
    out->tmp = p + fixed;
    out->tmp_bytes = ws_bytes - fixed;
  }
  return fixed + align_up(scan_temp_bytes(E));
}

// cnt[i] = min(d_i, f_i), cnt[N] = 0; bad |= 1 where fanout_of[i] > kMaxFanout (counted as capped there)
__global__ void __launch_bounds__(256) k_count(const int32_t* __restrict__ rowptr, int64_t N, int fanout,
                                               const int32_t* __restrict__ fanout_of, int32_t* __restrict__ cnt,
                                               int32_t* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > N) return;
  if (i == N) {
    cnt[N] = 0;
    return;
  }
  const int32_t d = rowptr[i + 1] - rowptr[i];
  int32_t f = fanout;
  if (fanout_of != nullptr) {
    const int32_t v = fanout_of[i];
    if (v > kMaxFanout) atomicOr(bad, 1);
    f = v < 0 ? d : min(v, kMaxFanout);
  }
  cnt[i] = min(d, f);
}

// One block per kRows destination rows.  (1) The rows kept whole (d == kept) are copied by a
// streaming pass over the block's sampled slots: slot ns finds its row by a binary search of the
// block's rowptr' in LDS, so loads and stores are both contiguous and a sampled hub costs nothing
// here.  (2) The rows with d > f take one wave each: lane s computes its own draw t_s up front,
// the f Floyd steps then run in sequence (readlane of t_s, compare, ballot), the positions are
// ranked within the wave and lane s writes the slot of rank(s).
__global__ void __launch_bounds__(256) k_pick(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                              const int32_t* __restrict__ csr_eid,
                                              const int32_t* __restrict__ csr2csc, int64_t N, uint64_t seed,
                                              const int32_t* __restrict__ rowptr_s, int32_t* __restrict__ col_s,
                                              int32_t* __restrict__ csr_eid_s, int32_t* __restrict__ newslot,
                                              uint8_t* __restrict__ keep, uint8_t* __restrict__ keepc) {
  __shared__ int32_t s_rp[kRows + 1], s_rps[kRows + 1], s_big[kRows], s_wc[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * kRows;
  const int nr = (int)min((int64_t)kRows, N - r0);
  for (int t = tid; t <= nr; t += 256) {
    s_rp[t] = rowptr[r0 + t];
    s_rps[t] = rowptr_s[r0 + t];
  }
  __syncthreads();
  const int32_t sb = s_rps[0], se = s_rps[nr];
  for (int32_t ns = sb + tid; ns < se; ns += 256) {
    int lo = 0, hi = nr;  // s_rps[lo] <= ns < s_rps[hi]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (s_rps[mid] <= ns) lo = mid; else hi = mid;
    }
    if (s_rp[lo + 1] - s_rp[lo] == s_rps[lo + 1] - s_rps[lo]) {
      const int32_t old = s_rp[lo] + (ns - s_rps[lo]);
      const int32_t e = csr_eid[old];
      col_s[ns] = col[old];
      csr_eid_s[ns] = e;  // the original id; k_renumber turns it into the new one
      newslot[old] = ns;
      keep[e] = 1;
      keepc[csr2csc[old]] = 1;
    }
  }
  // the block's sampled rows, in row order
  bool big = false;
  if (tid < nr) {
    const int32_t d = s_rp[tid + 1] - s_rp[tid], f = s_rps[tid + 1] - s_rps[tid];
    big = d > f && f > 0;
  }
  const uint64_t bm = __ballot(big);
  if (lane == 0) s_wc[wave] = (int32_t)__popcll(bm);
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += s_wc[w];
  const int nbig = s_wc[0] + s_wc[1] + s_wc[2] + s_wc[3];
  if (big) s_big[base + (int)__popcll(bm & ((1ull << lane) - 1))] = tid;
  __syncthreads();
  for (int q = wave; q < nbig; q += 4) {
    const int r = __builtin_amdgcn_readfirstlane(s_big[q]);
    const int32_t d = __builtin_amdgcn_readfirstlane(s_rp[r + 1] - s_rp[r]);
    const int32_t f = __builtin_amdgcn_readfirstlane(s_rps[r + 1] - s_rps[r]);
    const uint64_t i = (uint64_t)(r0 + r);
    const int32_t val = floyd_wave(seed, i, d, f, lane);  // lane s: element s of S
    int rank = 0;
    for (int l = 0; l < f; ++l) rank += __builtin_amdgcn_readlane(val, l) < val ? 1 : 0;
    if (lane < f) {
      const int32_t old = s_rp[r] + val, ns = s_rps[r] + rank;
      const int32_t e = csr_eid[old];
      col_s[ns] = col[old];
      csr_eid_s[ns] = e;
      newslot[old] = ns;
      keep[e] = 1;
      keepc[csr2csc[old]] = 1;
    }
  }
}

// the kept columns of edge_index and their original ids, at their new ids
__global__ void __launch_bounds__(256) k_coo(const int64_t* __restrict__ ei, int64_t E, int64_t Es,
                                             const uint8_t* __restrict__ keep, const int32_t* __restrict__ newid,
                                             int64_t* __restrict__ ei_s, int64_t* __restrict__ eid) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E || !keep[e]) return;
  const int64_t n = newid[e];
  ei_s[n] = ei[e];
  ei_s[Es + n] = ei[E + e];
  eid[n] = e;
}

__global__ void __launch_bounds__(256) k_renumber(int32_t* __restrict__ csr_eid_s, int64_t Es,
                                                  const int32_t* __restrict__ newid) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < Es) csr_eid_s[k] = newid[csr_eid_s[k]];
}

__global__ void __launch_bounds__(256) k_csc(const int32_t* __restrict__ row, const int32_t* __restrict__ csc_eid,
                                             const int32_t* __restrict__ csc2csr, int64_t E,
                                             const uint8_t* __restrict__ keepc, const int32_t* __restrict__ newid,
                                             const int32_t* __restrict__ newslot, const int32_t* __restrict__ cscpos,
                                             int32_t* __restrict__ row_s, int32_t* __restrict__ csc_eid_s,
                                             int32_t* __restrict__ csc2csr_s, int32_t* __restrict__ csr2csc_s) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= E || !keepc[k]) return;
  const int32_t e = csc_eid[k];
  const int32_t kk = cscpos[k], s = newslot[csc2csr[k]];
  row_s[kk] = row[k];
  csc_eid_s[kk] = newid[e];
  csc2csr_s[kk] = s;
  csr2csc_s[s] = kk;
}

__global__ void __launch_bounds__(256) k_colptr(const int32_t* __restrict__ colptr, int64_t N, int64_t E, int64_t Es,
                                                const int32_t* __restrict__ cscpos, int32_t* __restrict__ colptr_s) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r > N) return;
  const int32_t k = colptr[r];
  colptr_s[r] = k < E ? cscpos[k] : (int32_t)Es;
}

inline unsigned grid(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

size_t neighbor_workspace_bytes(int64_t N, int64_t E) {
  const size_t a = carve(E, nullptr, 0, nullptr), b = count_bytes(N);
  return a > b ? a : b;
}

hipError_t neighbor_count(const int32_t* rowptr, int64_t N, int fanout, const int32_t* fanout_of, int32_t* rowptr_s,
                          int32_t* info, void* ws, size_t ws_bytes, hipStream_t st) {
  const size_t n4 = align_up((size_t)(N + 1) * 4);
  if (ws_bytes < count_bytes(N)) return hipErrorInvalidValue;
  size_t tmp_bytes = 0;
  int32_t* cnt = static_cast<int32_t*>(ws);
  void* tmp = static_cast<char*>(ws) + n4;
  hipError_t err = hipMemsetAsync(info, 0, 2 * sizeof(int32_t), st);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(k_count, dim3(grid(N + 1)), dim3(256), 0, st, rowptr, N, fanout, fanout_of, cnt, info + 1);
  err = hipGetLastError();
  if (err != hipSuccess) return err;
  tmp_bytes = ws_bytes - n4;
  err = rocprim::exclusive_scan(tmp, tmp_bytes, cnt, rowptr_s, (int32_t)0, (size_t)(N + 1),
                                rocprim::plus<int32_t>(), st);
  if (err != hipSuccess) return err;
  return hipMemcpyAsync(info, rowptr_s + N, sizeof(int32_t), hipMemcpyDeviceToDevice, st);
}

hipError_t neighbor_sample(const int32_t* rowptr, const int32_t* col, const int32_t* csr_eid,
                           const int32_t* csr2csc, const int64_t* ei, int64_t N, int64_t E, uint64_t seed, const int32_t* rowptr_s, int64_t Es, int32_t* col_s,
                           int32_t* csr_eid_s, int64_t* ei_s, int64_t* eid, void* ws, size_t ws_bytes,
                           hipStream_t st) {
  Carve c;
  if (ws_bytes < carve(E, ws, ws_bytes, &c)) return hipErrorInvalidValue;
  if (E == 0) return hipSuccess;
  hipError_t err = hipMemsetAsync(c.keep, 0, (size_t)E, st);
  if (err != hipSuccess) return err;
  err = hipMemsetAsync(c.keepc, 0, (size_t)E, st);
  if (err != hipSuccess) return err;
  if (Es > 0)
    hipLaunchKernelGGL(k_pick, dim3((unsigned)((N + kRows - 1) / kRows)), dim3(256), 0, st, rowptr, col, csr_eid,
                       csr2csc, N, seed, rowptr_s, col_s, csr_eid_s, c.newslot, c.keep, c.keepc);
  size_t tmp_bytes = c.tmp_bytes;
  err = rocprim::exclusive_scan(c.tmp, tmp_bytes, ByteIt(c.keep, ByteFlag()), c.newid, (int32_t)0, (size_t)E,
                                rocprim::plus<int32_t>(), st);
  if (err != hipSuccess) return err;
  if (Es > 0) {
    hipLaunchKernelGGL(k_coo, dim3(grid(E)), dim3(256), 0, st, ei, E, Es, c.keep, c.newid, ei_s, eid);
    hipLaunchKernelGGL(k_renumber, dim3(grid(Es)), dim3(256), 0, st, csr_eid_s, Es, c.newid);
  }
  return hipGetLastError();
}

hipError_t neighbor_derive(const int32_t* colptr, const int32_t* row, const int32_t* csc_eid, const int32_t* csc2csr,
                           int64_t N, int64_t E, int64_t Es, int32_t* colptr_s, int32_t* row_s, int32_t* csc_eid_s,
                           int32_t* csc2csr_s, int32_t* csr2csc_s, void* ws, size_t ws_bytes, hipStream_t st) {
  Carve c;
  if (ws_bytes < carve(E, ws, ws_bytes, &c)) return hipErrorInvalidValue;
  if (E > 0) {
    size_t tmp_bytes = c.tmp_bytes;
    hipError_t err = rocprim::exclusive_scan(c.tmp, tmp_bytes, ByteIt(c.keepc, ByteFlag()), c.cscpos, (int32_t)0,
                                             (size_t)E, rocprim::plus<int32_t>(), st);
    if (err != hipSuccess) return err;
    if (Es > 0)
      hipLaunchKernelGGL(k_csc, dim3(grid(E)), dim3(256), 0, st, row, csc_eid, csc2csr, E, c.keepc, c.newid,
                         c.newslot, c.cscpos, row_s, csc_eid_s, csc2csr_s, csr2csc_s);
  }
  hipLaunchKernelGGL(k_colptr, dim3(grid(N + 1)), dim3(256), 0, st, colptr, N, E, Es, c.cscpos, colptr_s);
  return hipGetLastError();
}

}  // namespace ppgat
