// ppgat_floyd.h -- the samplers' counter stream and Robert Floyd's subset step, one wave per row
// (include/ppgat.h "fan-out neighbour sampling"; oracle/sampler_oracle.py restates the stream).
// Shared by ppgat_nsample.hip (the pick) and ppgat_subgraph.hip (the frontier expansion), so that a
// row's sample is the same (seed, i, d, f) function in both.  Device code only, integers only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ppgat {

// the counter stream of ppgat_sample.hip (draw64 / below), restated: oracle/sampler_oracle.py
__device__ __forceinline__ uint64_t draw64(uint64_t seed, uint64_t t, uint64_t k) {
  uint64_t z = seed + (t + 1) * 0x9E3779B97F4A7C15ull;
  z ^= (k + 1) * 0xD1B54A32D192ED03ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ int64_t below(uint64_t r, int64_t n) { return (int64_t)__umul64hi(r, (uint64_t)n); }

// Floyd's f-subset of the positions 0 .. d - 1 of row i (d > f >= 1, f <= 64; i, d, f wave-uniform),
// by one whole wave: lane s computes its own draw t_s up front, the f steps then run in sequence
// (readlane of t_s, compare, ballot).  Returns element s of S in lane s, -1 in the lanes >= f.
__device__ __forceinline__ int32_t floyd_wave(uint64_t seed, uint64_t i, int32_t d, int32_t f, int lane) {
  const int32_t tl =
      lane < f ? (int32_t)below(draw64(seed, i, (uint64_t)lane), (int64_t)(d - f + lane) + 1) : -1;
  int32_t val = -1;  // lane s: element s of S once step s has run
  for (int s = 0; s < f; ++s) {
    const int32_t t = __builtin_amdgcn_readlane(tl, s);
    const bool hit = __ballot(val == t) != 0;  // lanes >= s still hold -1 and t >= 0
    if (lane == s) val = hit ? d - f + s : t;
  }
  return val;
}

}  // namespace ppgat
