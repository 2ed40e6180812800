// ppgat_device.h -- the device helpers every kernel family shares: float4 arithmetic, streamed
// row access, the attention logit's LeakyReLU, the dropout mask and the work-item view.
//
// One definition each.  A forward and its backward must draw the same dropout mask, and one
// training step mixes kernels of several translation units (v1, aggregate-then-transform,
// GATv2), so drop_scale in particular lives here and nowhere else.
//
// A translation unit that switches floating-point contraction off (ppgat_gatv2.hip) includes
// this header AFTER its pragma, so the helpers round there as the rest of that file does.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ppgat.h"

namespace ppgat {

// an index input brought into [0, n): the product library clamps, the debug library refuses first
__device__ __forceinline__ int64_t clamp_idx(int64_t v, int64_t n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float4 f4(float a) { return make_float4(a, a, a, a); }
__device__ __forceinline__ float4 fma4(float s, float4 v, float4 a) {
  return make_float4(fmaf(s, v.x, a.x), fmaf(s, v.y, a.y), fmaf(s, v.z, a.z), fmaf(s, v.w, a.w));
}
__device__ __forceinline__ float4 add4(float4 a, float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
__device__ __forceinline__ float4 mul4(float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
__device__ __forceinline__ float dot4(float4 a, float4 b) {
  return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)));
}
__device__ __forceinline__ float comp(const float4& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }
__device__ __forceinline__ float4 shfl_xor4(float4 v, int m) {
  return make_float4(__shfl_xor(v.x, m), __shfl_xor(v.y, m), __shfl_xor(v.z, m), __shfl_xor(v.w, m));
}
__device__ __forceinline__ float4 absmax4(float4 m, float4 v) {
  return make_float4(fmaxf(m.x, fabsf(v.x)), fmaxf(m.y, fabsf(v.y)), fmaxf(m.z, fabsf(v.z)), fmaxf(m.w, fabsf(v.w)));
}
// merge a lane's maxima of |v| for columns c0 .. c0 + 3 into bits (IEEE bits, ordered as unsigned
// for v >= 0): read first, atomic only where larger -- after the first waves almost never.  A max
// is order-free, so the result is deterministic.
__device__ __forceinline__ void colmax_merge4(unsigned* bits, int c0, float4 m) {
  const uint4 cur = *reinterpret_cast<const uint4*>(bits + c0);
  if (__float_as_uint(m.x) > cur.x) atomicMax(bits + c0, __float_as_uint(m.x));
  if (__float_as_uint(m.y) > cur.y) atomicMax(bits + c0 + 1, __float_as_uint(m.y));
  if (__float_as_uint(m.z) > cur.z) atomicMax(bits + c0 + 2, __float_as_uint(m.z));
  if (__float_as_uint(m.w) > cur.w) atomicMax(bits + c0 + 3, __float_as_uint(m.w));
}

// Streamed (once-touched) rows of the edge kernels -- a forward's output rows, a backward's own
// source rows, LightGCN's running layer sum -- with the non-temporal hint when PPGAT_NT_STREAM=1,
// so they do not push the gathered table out of the Infinity Cache.
#ifndef PPGAT_NT_STREAM
#define PPGAT_NT_STREAM 1
#endif
__device__ __forceinline__ float4 ld4s(const float* p) {
#if PPGAT_NT_STREAM
  using v4 = __attribute__((ext_vector_type(4))) float;
  const v4 v = __builtin_nontemporal_load(reinterpret_cast<const v4*>(p));
  return make_float4(v.x, v.y, v.z, v.w);
#else
  return *reinterpret_cast<const float4*>(p);
#endif
}
__device__ __forceinline__ void st4s(float* p, float4 a) {
#if PPGAT_NT_STREAM
  using v4 = __attribute__((ext_vector_type(4))) float;
  __builtin_nontemporal_store(v4{a.x, a.y, a.z, a.w}, reinterpret_cast<v4*>(p));
#else
  *reinterpret_cast<float4*>(p) = a;
#endif
}

// torch leaky_relu and its backward rule (slope where z <= 0)
__device__ __forceinline__ float lrelu(float z, float slope) { return z > 0.f ? z : z * slope; }
__device__ __forceinline__ float dlrelu(float z, float slope) { return z > 0.f ? 1.f : slope; }

// Counter-based dropout mask on alpha (restated in oracle/gat_oracle.py:dropout_scale).  seed is
// the forward's effective seed (the epoch already folded in); the backward reads the same one.
__device__ __forceinline__ float drop_scale(uint64_t seed, uint32_t eid, uint32_t head, float p, float inv_keep) {
  uint64_t x = seed ^ ((uint64_t)eid * 0x9E3779B97F4A7C15ull) ^ ((uint64_t)head * 0xC2B2AE3D27D4EB4Full);
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  const float u = (float)(x >> 40) * (1.0f / 16777216.0f);
  return u >= p ? inv_keep : 0.f;
}

// Gather skipping (include/ppgat.h, ppgat_set_gather_skip).  nstate.w = D with the bit pattern of
// -0.0f marks a destination whose grad_out row is all zeros; every D writer of the GAT path emits
// that pattern for such rows only and +0 for any other zero (canon_d).  Pass B needs g_i of an
// edge for beta g_i and c1 <g_i, h_j> alone: with beta = c1 = 0 (a dropped edge) or a marked row
// both are exact zeros, so the row is not gathered (grow_unneeded).
constexpr int kZeroRowBits = (int)0x80000000u;
__device__ __forceinline__ float canon_d(float d, bool zero_row) {
  return zero_row ? __int_as_float(kZeroRowBits) : (d == 0.f ? 0.f : d);
}
__device__ __forceinline__ bool grow_unneeded(float bg, float c1, float d) {
  return (bg == 0.f && c1 == 0.f) || __float_as_int(d) == kZeroRowBits;
}

// Work items, as the edge kernels take them.  Rows (destination rows for a forward, source rows
// for a backward pass by source) are cut into items of at most T edges by ppgat_schedule_build:
// hub rows (deg > T) become ceil(deg/T) pieces that write partial state to a scratch slab and are
// merged in piece order by a second small kernel (deterministic); all other rows are one item.
// Items are ordered hub pieces first, then rows by descending degree, so the longest work starts
// first and the tail is short (largest in-degree on config 2: 5,180).
struct Items {
  const int32_t* row;
  const int32_t* beg;
  const int32_t* end;
  int64_t n_items;
  int64_t n_hub_items;  // items [0, n_hub_items) are hub pieces, slot = item index
};
// items [0, n) of a schedule, as a launcher hands them to its kernel
inline Items items_of(const ppgat_schedule& sch, int64_t n) {
  return Items{sch.item_row, sch.item_beg, sch.item_end, n, sch.n_hub_items};
}

}  // namespace ppgat
