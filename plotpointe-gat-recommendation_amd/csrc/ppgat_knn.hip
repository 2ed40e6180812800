// ppgat_knn.hip -- neighbour selection of the I-I kNN build (graphs/build_ii_knn.py:76-99),
// after the cosine-similarity block S = E_q E^T (library GEMM, the only dense part):
// per query row, the k largest similarities excluding the item itself, sorted descending
// (ties: smaller item index first), and how many of them reach min_similarity.  An entry of
// -inf or NaN is absent: it never beats a lane's threshold (s > thr is false for both), so it
// is never selected and never counted.
//
// One wave per row.  Each lane scans a strided slice of the row (coalesced 256-B loads,
// 4 in flight) keeping its own sorted top-k list in LDS ([slot][lane] so the 64 lanes hit
// 64 banks); an insertion happens only when a value beats the lane's current k-th, i.e.
// O(k log(n/64k)) times per lane.  The 64 lists are then merged by k rounds of a wave
// argmax (value desc, index asc).  No atomics: the result is deterministic.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "ppgat_internal.h"
#include "ppgat_lanes.h"

namespace ppgat {

namespace {

template <int K>
__global__ void __launch_bounds__(256) k_knn_topk(const float* __restrict__ S, int64_t ld, int64_t rows,
                                                  int64_t n_cols, int64_t q0, int k, float min_sim,
                                                  int32_t* __restrict__ out_idx, float* __restrict__ out_sim,
                                                  int32_t* __restrict__ out_cnt) {
  __shared__ float lv[4][K][64];
  __shared__ int32_t li[4][K][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * 4 + wv;
  if (r >= rows) return;  // whole wave
  for (int t = 0; t < k; ++t) {
    lv[wv][t][lane] = -INFINITY;
    li[wv][t][lane] = INT32_MAX;
  }
  float thr = -INFINITY;  // this lane's current k-th value
  const float* srow = S + r * ld;
  const int64_t self = q0 + r;
  for (int64_t j0 = 0; j0 < n_cols; j0 += 256) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t j = j0 + u * 64 + lane;
      v[u] = j < n_cols ? srow[j] : -INFINITY;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t j = j0 + u * 64 + lane;
      const float s = j == self ? -INFINITY : v[u];
      if (s > thr) {  // strict: an equal later value (larger index) does not displace
        int p = k - 1;
        while (p > 0 && lv[wv][p - 1][lane] < s) {
          lv[wv][p][lane] = lv[wv][p - 1][lane];
          li[wv][p][lane] = li[wv][p - 1][lane];
          --p;
        }
        lv[wv][p][lane] = s;
        li[wv][p][lane] = (int32_t)j;
        thr = lv[wv][k - 1][lane];
      }
    }
  }
  // merge the 64 sorted lists: k rounds of a wave argmax over the lanes' heads
  int h = 0;
  int cnt = 0;
  for (int t = 0; t < k; ++t) {
    float bv = h < k ? lv[wv][h][lane] : -INFINITY;
    int32_t bi = h < k ? li[wv][h][lane] : INT32_MAX;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off);
      const int32_t oi = __shfl_xor(bi, off);
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
      }
    }
    if (h < k && li[wv][h][lane] == bi && lv[wv][h][lane] == bv) ++h;  // indices are unique per row
    if (lane == 0) {
      out_sim[r * k + t] = bv;
      out_idx[r * k + t] = bi == INT32_MAX ? -1 : bi;
    }
    // sorted descending: the kept entries are a prefix; a pad (-1 / -inf) is no item and is not
    // counted even where min_sim = -inf
    cnt += (bi != INT32_MAX && bv >= min_sim) ? 1 : 0;
  }
  if (lane == 0 && out_cnt != nullptr) out_cnt[r] = cnt;
}

// The most-attended in-edges of every destination (ppgat_attention_topk): k_knn_topk's selection
// over a CSR row instead of a dense one.  The ranked value of slot s is the head mean
// (sum_h val[s, h]) * inv_h, its id the original edge id eid[s]; ids within a row arrive in no
// particular order, so the order (value descending, id ascending) is kept as a total order
// through the lane lists -- a later slot displaces an equal value when its id is smaller.  NaN
// ranks as -inf.  One wave walks its whole row, however long.  A row of at most 64 edges (nearly
// every row of a recommender graph) needs no lists: each lane holds one entry and finds its place
// by counting the entries that come before it (ids are unique, so the places are).
__device__ __forceinline__ float head_mean(const float* __restrict__ val, int64_t s, int heads, float inv_h) {
  float x = val[s * heads];
  for (int h = 1; h < heads; ++h) x += val[s * heads + h];
  x *= inv_h;
  return x == x ? x : -INFINITY;
}

template <int K>
__global__ void __launch_bounds__(256) k_attn_topk(const int32_t* __restrict__ rowptr,
                                                   const int32_t* __restrict__ eid, const float* __restrict__ val,
                                                   int64_t rows, int heads, float inv_h, int k,
                                                   int32_t* __restrict__ out_eid, float* __restrict__ out_val,
                                                   int32_t* __restrict__ out_cnt) {
  __shared__ float lv[4][K][64];
  __shared__ int32_t li[4][K][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * 4 + wv;
  if (r >= rows) return;  // whole wave
  const int rs = rowptr[r], re = rowptr[r + 1];
  if (re - rs <= 64) {  // wave-uniform
    const int deg = re - rs;
    const bool has = lane < deg;
    const float v = has ? head_mean(val, rs + lane, heads, inv_h) : -INFINITY;
    const int32_t id = has ? eid[rs + lane] : INT32_MAX;
    lv[wv][0][lane] = v;
    li[wv][0][lane] = id;
    wave_sync();
    int place = 0;
    for (int j = 0; j < deg; ++j) {  // (one address per step: a broadcast read)
      const float ov = lv[wv][0][j];
      const int32_t oi = li[wv][0][j];
      place += (ov > v || (ov == v && oi < id)) ? 1 : 0;
    }
    if (has && place < k) {
      out_val[r * k + place] = v;
      out_eid[r * k + place] = id;
    }
    if (!has && lane < k) {  // places [deg, k)
      out_val[r * k + lane] = 0.f;
      out_eid[r * k + lane] = -1;
    }
    if (lane == 0) out_cnt[r] = deg < k ? deg : k;
    return;
  }
  for (int t = 0; t < k; ++t) {
    lv[wv][t][lane] = -INFINITY;
    li[wv][t][lane] = INT32_MAX;
  }
  float thr = -INFINITY;       // this lane's current k-th entry
  int32_t thr_id = INT32_MAX;
  for (int s0 = rs; s0 < re; s0 += 256) {  // wave-uniform trip count
    float v[4];
    int32_t id[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int s = s0 + u * 64 + lane;
      v[u] = -INFINITY;
      id[u] = INT32_MAX;
      if (s < re) {
        v[u] = head_mean(val, s, heads, inv_h);
        id[u] = eid[s];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float s = v[u];
      const int32_t e = id[u];
      if (s > thr || (s == thr && e < thr_id)) {  // (a pad, -inf / INT32_MAX, never passes)
        int p = k - 1;
        while (p > 0 && (lv[wv][p - 1][lane] < s || (lv[wv][p - 1][lane] == s && li[wv][p - 1][lane] > e))) {
          lv[wv][p][lane] = lv[wv][p - 1][lane];
          li[wv][p][lane] = li[wv][p - 1][lane];
          --p;
        }
        lv[wv][p][lane] = s;
        li[wv][p][lane] = e;
        thr = lv[wv][k - 1][lane];
        thr_id = li[wv][k - 1][lane];
      }
    }
  }
  // merge the 64 sorted lists: k rounds of a wave argmax over the lanes' heads
  int h = 0;
  int cnt = 0;
  for (int t = 0; t < k; ++t) {
    float bv = h < k ? lv[wv][h][lane] : -INFINITY;
    int32_t bi = h < k ? li[wv][h][lane] : INT32_MAX;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off);
      const int32_t oi = __shfl_xor(bi, off);
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
      }
    }
    if (h < k && li[wv][h][lane] == bi && bi != INT32_MAX) ++h;  // edge ids are unique
    const bool pad = bi == INT32_MAX;
    if (lane == 0) {
      out_val[r * k + t] = pad ? 0.f : bv;
      out_eid[r * k + t] = pad ? -1 : bi;
    }
    cnt += pad ? 0 : 1;
  }
  if (lane == 0) out_cnt[r] = cnt;
}

}  // namespace

hipError_t attention_topk(const int32_t* rowptr, const int32_t* eid, const float* val, int64_t rows, int heads,
                          int k, int32_t* out_eid, float* out_val, int32_t* out_cnt, hipStream_t st) {
  if (rows <= 0) return hipSuccess;
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  const float inv_h = 1.f / (float)heads;
  if (k <= 8) hipLaunchKernelGGL(k_attn_topk<8>, grid, block, 0, st, rowptr, eid, val, rows, heads, inv_h, k, out_eid, out_val, out_cnt);
  else if (k <= 16) hipLaunchKernelGGL(k_attn_topk<16>, grid, block, 0, st, rowptr, eid, val, rows, heads, inv_h, k, out_eid, out_val, out_cnt);
  else hipLaunchKernelGGL(k_attn_topk<32>, grid, block, 0, st, rowptr, eid, val, rows, heads, inv_h, k, out_eid, out_val, out_cnt);
  return hipGetLastError();
}

int knn_max_k() { return 64; }

hipError_t knn_topk(const float* S, int64_t ld, int64_t rows, int64_t n_cols, int64_t q0, int k, float min_sim,
                    int32_t* out_idx, float* out_sim, int32_t* out_cnt, hipStream_t st) {
  if (rows <= 0) return hipSuccess;
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  if (k <= 8) hipLaunchKernelGGL(k_knn_topk<8>, grid, block, 0, st, S, ld, rows, n_cols, q0, k, min_sim, out_idx, out_sim, out_cnt);
  else if (k <= 16) hipLaunchKernelGGL(k_knn_topk<16>, grid, block, 0, st, S, ld, rows, n_cols, q0, k, min_sim, out_idx, out_sim, out_cnt);
  else if (k <= 32) hipLaunchKernelGGL(k_knn_topk<32>, grid, block, 0, st, S, ld, rows, n_cols, q0, k, min_sim, out_idx, out_sim, out_cnt);
  else hipLaunchKernelGGL(k_knn_topk<64>, grid, block, 0, st, S, ld, rows, n_cols, q0, k, min_sim, out_idx, out_sim, out_cnt);
  return hipGetLastError();
}

}  // namespace ppgat
