// ppgat_xform.hip -- the fp32 and split (bf16 / fp16) matrix-core GEMMs that the
// aggregate-then-transform layer (ppgat_xgat.hip) and the row-sharded config-5 path run on (gfx950).
//
// GEMMs (v_mfma_f32_32x32x2_f32, exact fp32 FMA chains; 157 TF peak):
//  * k_gemm_nn: Y = alpha X B (+ bias), X [M, K] row-major streamed from HBM straight into
//    the A-operand layout (float4 per lane = 4 MFMA steps, reduction index permuted),
//    B [K, N] (row-major) or [N, K] (X W^T) staged per 32-deep k chunk in LDS; each wave owns
//    32 rows x BN columns (NT 32x32 accumulator tiles), workgroups mapped XCD-aware so the
//    column blocks of one row block share an L2.
//  * k_gemm_tn: G = A^T B over M rows (weight gradients): 128 x 256 output tile per
//    workgroup, 32-row chunks staged in LDS, row splits summed in split order (deterministic);
//    the tiles of one row split run on one XCD, so the rows leave HBM once.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "ppgat_internal.h"
#include "ppgat_lanes.h"
#include "ppgat_device.h"
#include "ppgat_split.h"
#include "ppgat_nnh_pipe.h"

namespace ppgat {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
inline size_t align_up(size_t x) { return (x + 255) & ~size_t(255); }

// ===========================================================================
// NN GEMM: Y[M, N] = alpha X[M, K] B + bias
// ===========================================================================
constexpr int kGBM = 128;  // rows per workgroup (4 waves x 32)
constexpr int kGBK = 32;   // reduction chunk
constexpr int kNkLd = kGBK + 4;  // LDS row stride of the [n][k] image (NK mode): conflict-free b128 reads

struct NnArg {
  const float* X;
  int64_t ldx;
  int64_t M;
  int K;
  const float* B;
  int64_t ldb;
  int N;
  float alpha;
  const float* bias;
  float* Y;
  int64_t ldy;
  int n_blocks;
  int64_t row_blocks;
  int splits;     // > 1: split-K, raw partial tiles to part[split][M][N] (k_nn_split_sum finishes)
  int k_per;      // reduction length per split (multiple of kGBK)
  float* part;
  // optional rank update fused into k_gemm_nnh's epilogue: Y += rS[row][:nv] rA[:nv][col]
  // (v ascending, after alpha and bias -- the order of k_rank_update, so the same bits)
  const float* rS;
  int64_t ldrs;
  int nv;
  const float* rA;
  int64_t ldra;
};

// BMODE 0: B[k][n] = B[k * ldb + n] (image [k][n], b32 reads); 1: B[k][n] = B[n * ldb + k] (X W^T,
// image [n][k], b128 reads).  MFMA 32x32x2 lane maps (r = lane & 31, hf = lane >> 5): A operand
// X[row r][k], B operand B[k][col r], accumulator q at row (q & 3) + 8 (q >> 2) + 4 hf, col r;
// within a group of 8 k, lane half hf supplies k = 8g + 4 hf + s at MFMA step s.
template <int NT, int BMODE>
__global__ void __launch_bounds__(256, 2) k_gemm_nn(NnArg a) {
  constexpr int BN = 32 * NT;
  constexpr int IMG = BMODE == 0 ? kGBK * BN : BN * kNkLd;
  __shared__ float sB[IMG];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r = lane & 31, hf = lane >> 5;
  // XCD-aware order: blocks b, b + 8, b + 16, ... land on one XCD; the n blocks of a row block
  // are consecutive there, so its X rows are fetched from HBM once
  const int64_t b = blockIdx.x;
  int64_t rb;
  int n0, split = 0;
  if (a.splits > 1) {  // small M: (row block, n block, k split), splits fastest
    split = (int)(b % a.splits);
    const int64_t rest = b / a.splits;
    n0 = (int)(rest % a.n_blocks) * BN;
    rb = rest / a.n_blocks;
  } else {
    const int64_t idx = b >> 3;
    rb = (idx / a.n_blocks) * 8 + (b & 7);
    n0 = (int)(idx % a.n_blocks) * BN;
  }
  if (rb >= a.row_blocks) return;
  const int64_t M = a.M;
  const int kbeg = split * a.k_per;
  const int K = a.splits > 1 ? (kbeg + a.k_per < a.K ? kbeg + a.k_per : a.K) : a.K;
  const int64_t m = rb * kGBM + wv * 32 + r;
  const float* xrow = a.X + (m < M ? m : M - 1) * a.ldx + 4 * hf;  // rows past M re-read row M-1 (never stored)

  float4 bst[NT];
  auto load_b = [&](int kc) {
#pragma unroll
    for (int s = 0; s < NT; ++s) {
      const int e = tid + 256 * s;
      if (BMODE == 0) {
        const int k = e / (BN / 4), n4 = (e % (BN / 4)) * 4;
        bst[s] = ld4(a.B + (int64_t)(kc + k) * a.ldb + n0 + n4);
      } else {
        const int n = e >> 3, k4 = (e & 7) * 4;
        bst[s] = ld4(a.B + (int64_t)(n0 + n) * a.ldb + kc + k4);
      }
    }
  };
  auto store_b = [&]() {
#pragma unroll
    for (int s = 0; s < NT; ++s) {
      const int e = tid + 256 * s;
      if (BMODE == 0) {
        const int k = e / (BN / 4), n4 = (e % (BN / 4)) * 4;
        st4(&sB[k * BN + n4], bst[s]);
      } else {
        const int n = e >> 3, k4 = (e & 7) * 4;
        st4(&sB[n * kNkLd + k4], bst[s]);
      }
    }
  };
  float4 xa[4], xn[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) xa[g] = ld4(xrow + 8 * g);
  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x16{};
  if (kbeg > 0) {
#pragma unroll
    for (int g = 0; g < 4; ++g) xa[g] = ld4(xrow + kbeg + 8 * g);
  }
  load_b(kbeg);
  store_b();
  __syncthreads();
  for (int kc = kbeg; kc < K; kc += kGBK) {
    const bool more = kc + kGBK < K;
    if (more) {
      load_b(kc + kGBK);
#pragma unroll
      for (int g = 0; g < 4; ++g) xn[g] = ld4(xrow + kc + kGBK + 8 * g);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      if (BMODE == 1) {
        float4 bv[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) bv[t] = ld4(&sB[(32 * t + r) * kNkLd + 8 * g + 4 * hf]);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int t = 0; t < NT; ++t) acc[t] = mfma32(comp(xa[g], s), comp(bv[t], s), acc[t]);
      } else {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const float* brow = &sB[(8 * g + 4 * hf + s) * BN + r];
#pragma unroll
          for (int t = 0; t < NT; ++t) acc[t] = mfma32(comp(xa[g], s), brow[32 * t], acc[t]);
        }
      }
    }
    __syncthreads();
    if (more) {
      store_b();
#pragma unroll
      for (int g = 0; g < 4; ++g) xa[g] = xn[g];
    }
    __syncthreads();
  }
  const int64_t row0 = rb * kGBM + wv * 32;
  if (a.splits > 1) {
    float* part = a.part + (int64_t)split * M * a.N;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int col = n0 + 32 * t + r;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int64_t row = row0 + (q & 3) + 8 * (q >> 2) + 4 * hf;
        if (row < M) part[row * a.N + col] = acc[t][q];
      }
    }
    return;
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int col = n0 + 32 * t + r;
    const float bv = a.bias != nullptr ? a.bias[col] : 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int64_t row = row0 + (q & 3) + 8 * (q >> 2) + 4 * hf;
      if (row < M) a.Y[row * a.ldy + col] = fmaf(a.alpha, acc[t][q], bv);
    }
  }
}

// NN GEMM on the split bf16 matrix cores (ppgat_split.h), same contract, block order and
// split-K partials as k_gemm_nn.  v_mfma_f32_32x32x16_bf16: lane (r, hf) holds A[row r][8 hf + j]
// and B[8 hf + j][col r]; a 32-deep k chunk is two MFMA steps u, and lane half hf's element j
// of step u is k = 16 u + 4 hf + (j & 3) + 8 (j >> 2) -- exactly the two float4 xa[2u], xa[2u+1]
// a lane already streams from its X row.  The B chunk is split once per workgroup while being
// staged: three bf16 images [n][kk] with kk the position of k in that order (80-B rows: the 16
// lanes of every ds_read_b128 group hit distinct bank slots), one b128 read per part per tile.
template <int NT, int BMODE, int KC>
__global__ void __launch_bounds__(256, 2) k_gemm_nnx(NnArg a) {
  constexpr int BN = 32 * NT;
  constexpr int LDK = KC + 8;             // bf16 per image row (KC + 8 pad: an odd number of 16-B units)
  constexpr int PART = BN * LDK;          // bf16 per part
  constexpr int G = BN * (KC / 4) / 256;  // 4-k groups staged per thread per chunk
  constexpr int XG = KC / 8;              // float4 of X per lane per chunk
  __shared__ __attribute__((aligned(16))) uint16_t sB[3 * PART];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r = lane & 31, hf = lane >> 5;
  const int64_t b = blockIdx.x;
  int64_t rb;
  int n0, split = 0;
  if (a.splits > 1) {
    split = (int)(b % a.splits);
    const int64_t rest = b / a.splits;
    n0 = (int)(rest % a.n_blocks) * BN;
    rb = rest / a.n_blocks;
  } else {
    const int64_t idx = b >> 3;
    rb = (idx / a.n_blocks) * 8 + (b & 7);
    n0 = (int)(idx % a.n_blocks) * BN;
  }
  if (rb >= a.row_blocks) return;
  const int64_t M = a.M;
  const int kbeg = split * a.k_per;
  const int K = a.splits > 1 ? (kbeg + a.k_per < a.K ? kbeg + a.k_per : a.K) : a.K;
  const int64_t m = rb * kGBM + wv * 32 + r;
  const float* xrow = a.X + (m < M ? m : M - 1) * a.ldx + 4 * hf;

  // staged group e = tid + 256 s: column n, reduction indices 4 q .. 4 q + 3 of the chunk
  auto grp = [&](int s, int& n, int& q) {
    const int e = tid + 256 * s;
    if (BMODE == 0) { n = e % BN; q = e / BN; }                   // a k row is contiguous in n
    else if (KC == 32) {  // an n row is contiguous in k; rows n, n + 4 share a 16-lane write group
      n = 8 * (e >> 6) + ((((e >> 3) & 1) << 2) | ((e >> 4) & 3));  // (80 dwords apart: no bank conflict)
      q = e & 7;
    } else { n = e / (KC / 4); q = e % (KC / 4); }
  };
  float4 bst[G];
  auto load_b = [&](int kc) {
#pragma unroll
    for (int s = 0; s < G; ++s) {
      int n, q;
      grp(s, n, q);
      if (BMODE == 0) {
        const float* p = a.B + (int64_t)(kc + 4 * q) * a.ldb + n0 + n;
        bst[s] = make_float4(p[0], p[a.ldb], p[2 * a.ldb], p[3 * a.ldb]);
      } else {
        bst[s] = ld4(a.B + (int64_t)(n0 + n) * a.ldb + kc + 4 * q);
      }
    }
  };
  auto store_b = [&]() {
#pragma unroll
    for (int s = 0; s < G; ++s) {
      int n, q;
      grp(s, n, q);
      const int kk = 16 * (q >> 2) + 8 * (q & 1) + 4 * ((q >> 1) & 1);
      const float v[4] = {bst[s].x, bst[s].y, bst[s].z, bst[s].w};
      uint2 h, mm, l;
      uint32_t* ph = &h.x;
      uint32_t* pm = &mm.x;
      uint32_t* pl = &l.x;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const uint32_t hh = split::pk_bf16(v[2 * i], v[2 * i + 1]);
        const float r0 = v[2 * i] - split::bf_lo(hh), r1 = v[2 * i + 1] - split::bf_hi(hh);
        const uint32_t m2 = split::pk_bf16(r0, r1);
        ph[i] = hh;
        pm[i] = m2;
        pl[i] = split::pk_bf16(r0 - split::bf_lo(m2), r1 - split::bf_hi(m2));
      }
      const int off = n * LDK + kk;
      *reinterpret_cast<uint2*>(&sB[off]) = h;
      *reinterpret_cast<uint2*>(&sB[PART + off]) = mm;
      *reinterpret_cast<uint2*>(&sB[2 * PART + off]) = l;
    }
  };
  float4 xa[XG], xn[XG];
#pragma unroll
  for (int g = 0; g < XG; ++g) xa[g] = ld4(xrow + kbeg + 8 * g);
  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x16{};
  load_b(kbeg);
  store_b();
  __syncthreads();
  for (int kc = kbeg; kc < K; kc += KC) {
    const bool more = kc + KC < K;
    if (more) {
      load_b(kc + KC);
#pragma unroll
      for (int g = 0; g < XG; ++g) xn[g] = ld4(xrow + kc + KC + 8 * g);
    }
    // (u, t) steps in order; the next step's three B units are read from LDS while the
    // current step's six MFMAs run (a read waited on right before its MFMAs exposes the LDS
    // latency against only six MFMAs)
    auto read_b = [&](int idx, split::u32x4 (&f)[3]) {
      const int off = (32 * (idx % NT) + r) * LDK + 16 * (idx / NT) + 8 * hf;
#pragma unroll
      for (int p = 0; p < 3; ++p) f[p] = *reinterpret_cast<const split::u32x4*>(&sB[p * PART + off]);
    };
    split::u32x4 fx[3], fb[3];
    read_b(0, fb);
#pragma unroll
    for (int idx = 0; idx < (KC / 16) * NT; ++idx) {
      const int u = idx / NT, t = idx % NT;
      if (t == 0) split::split3(xa[2 * u], xa[2 * u + 1], fx[0], fx[1], fx[2]);
      split::u32x4 fn[3];
      if (idx + 1 < (KC / 16) * NT) read_b(idx + 1, fn);
      acc[t] = split::mfma32_x6(fx, fb, acc[t]);
      __builtin_amdgcn_sched_barrier(0);
      if (idx + 1 < (KC / 16) * NT) {
        fb[0] = fn[0];
        fb[1] = fn[1];
        fb[2] = fn[2];
      }
    }
    __syncthreads();
    if (more) {
      store_b();
#pragma unroll
      for (int g = 0; g < XG; ++g) xa[g] = xn[g];
    }
    __syncthreads();
  }
  const int64_t row0 = rb * kGBM + wv * 32;
  if (a.splits > 1) {
    float* part = a.part + (int64_t)split * M * a.N;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int col = n0 + 32 * t + r;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int64_t row = row0 + (q & 3) + 8 * (q >> 2) + 4 * hf;
        if (row < M) part[row * a.N + col] = acc[t][q];
      }
    }
    return;
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int col = n0 + 32 * t + r;
    const float bv = a.bias != nullptr ? a.bias[col] : 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int64_t row = row0 + (q & 3) + 8 * (q >> 2) + 4 * hf;
      if (row < M) a.Y[row * a.ldy + col] = fmaf(a.alpha, acc[t][q], bv);
    }
  }
}

// ---------------------------------------------------------------------------
// The pre-split NN kernels: 8 waves x 32 rows per workgroup share every staged B chunk.
// ---------------------------------------------------------------------------
constexpr int kPBM = 256;  // rows per workgroup (8 waves x 32)

// the three-part bf16 chunk image of the lab build's k_gemm_nnp (lab/ppgat_xform_lab.h); here for
// nnx_image_bytes, which sizes the workspaces of both builds alike
template <int NT>
struct NnpImg {
  static constexpr int KC = 32, BN = 32 * NT, LDK = KC + 8, PART = BN * LDK, ELEMS = 3 * PART, BYTES = 2 * ELEMS;
  static_assert(BYTES % 1024 == 0, "an image is a whole number of 1-KB wave copies");
};

// ---------------------------------------------------------------------------
// NN GEMM on the fp16 matrix cores through the scaled two-term split (ppgat_split.h): three
// MFMAs per product instead of six.  B is pre-split once per call with a power-of-two scale per
// column (k_colscale16 + k_nnh_presplit: two fp16 images per (column block, k chunk), the same
// 80-B rows and permuted reduction order as the lab build's bf16 images).  X streams in 32-deep chunks, so a
// row's scale is set ONLINE: by the first chunk in which the row is nonzero (largest |x| s in
// [2^9, 2^10)), and lowered only when a later chunk would reach 2^15 (fp16 overflows at 65,520,
// so 32x headroom) -- then that row's accumulators are multiplied by the exact power of two
// s_new / s_old (a wave-uniform branch, rare on real data: first-chunk maxima within 32x of the
// row's).  Elements far below their row's max keep an absolute error <= 2^-34 of that max.
// ---------------------------------------------------------------------------

// per column of B [K x N]: the scale exponent (largest |b| 2^e in [2^9, 2^10); 0 for a zero column)
template <int BMODE>
__global__ void __launch_bounds__(256) k_colscale16(const float* __restrict__ B, int64_t ldb, int K, int N,
                                                    int* __restrict__ ecol) {
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (n >= N) return;
  float m = 0.f;
  for (int k = lane; k < K; k += 64) m = fmaxf(m, fabsf(BMODE == 0 ? B[(int64_t)k * ldb + n] : B[(int64_t)n * ldb + k]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if (lane == 0) ecol[n] = m > 0.f && m <= 3.4e38f ? split::scale_exp16(m) : 0;
}

template <int NT, int BMODE>
__global__ void __launch_bounds__(256) k_nnh_presplit(const float* __restrict__ B, int64_t ldb, int K, int N,
                                                      const int* __restrict__ ecol, uint16_t* __restrict__ img) {
  using I = NnhImg<NT>;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)N * (K / 4)) return;
  const int ng = (int)(t % N), kq = (int)(t / N);
  const int k0 = 4 * kq, c = k0 / I::KC, q = (k0 % I::KC) / 4;
  const int nb = ng / I::BN, n = ng % I::BN;
  const float s = ldexpf(1.f, ecol[ng]);
  float v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = (BMODE == 0 ? B[(int64_t)(k0 + j) * ldb + ng] : B[(int64_t)ng * ldb + k0 + j]) * s;
  uint2 h, l;
  uint32_t* ph = &h.x;
  uint32_t* pl = &l.x;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const uint32_t hh = split::pk_f16(v[2 * i], v[2 * i + 1]);
    const split::f32x2e back = __builtin_convertvector(__builtin_bit_cast(split::f16x2, hh), split::f32x2e);
    ph[i] = hh;
    pl[i] = split::pk_f16(v[2 * i] - back.x, v[2 * i + 1] - back.y);
  }
  const int kk = 16 * (q >> 2) + 8 * (q & 1) + 4 * ((q >> 1) & 1);
  uint16_t* base = img + ((int64_t)nb * (K / I::KC) + c) * I::ELEMS + n * I::LDK + kk;
  *reinterpret_cast<uint2*>(base) = h;
  *reinterpret_cast<uint2*>(base + I::PART) = l;
}

constexpr int kNnhRank = 8;  // rank terms the fused epilogue keeps in registers

// ---------------------------------------------------------------------------
// k_gemm_nnh3: the pipelined main loop of ppgat_nnh_pipe.h (nnh3_loop) -- B chunks by LDS-DMA two
// chunks ahead, the next chunk prepared inside the current chunk's MFMA sequence -- and the
// epilogue.  The same products in the same order as its predecessors k_gemm_nnh and k_gemm_nnh2
// (lab/ppgat_xform_lab.h; bitwise equal results, tests/test_gpu_gemm_f16.py).
// ---------------------------------------------------------------------------
// libppgat.so instantiates NT and RK only; XT, E4 and OCC are the lab build's measured variants,
// which the lab tests pin bitwise against the product kernel.
// XT (lab, PPGAT_NNH2=6): X loaded coalesced and transposed through LDS (see nnh3_loop).
// E4 (lab, PPGAT_NNH_E4=1): the epilogue without rank terms through a per-wave LDS
// transpose -- each lane's column of 16 rows is written to the (now idle) B buffers and read back
// as float4 pieces of rows, so a wave stores its 32 x 32 block per column tile in 4 float4
// instructions (8 rows x 128 B each) instead of 16 scalar ones; the same values (same bits).
// OCC (lab, PPGAT_NNH_OCC2=1 with NT = 4): at least OCC waves per SIMD (HIP's launch_bounds), i.e. two
// workgroups per CU at OCC = 4, so one's epilogue stores can run beside the other's products.
template <int NT, bool RK, bool XT = false, bool E4 = false, int OCC = 1>
__global__ void __launch_bounds__(512, OCC) k_gemm_nnh3(NnArg a, const uint16_t* __restrict__ img,
                                                      const int* __restrict__ ecol) {
  using I = NnhImg<NT>;
  constexpr int KC = I::KC;
  __shared__ __attribute__((aligned(16))) uint16_t sB[3 * I::ELEMS];
  __shared__ __attribute__((aligned(16))) float sF[8][32];  // per wave: a factor per row (rescale, epilogue)
  __shared__ __attribute__((aligned(16))) float sX[XT ? 8 : 1][XT ? 32 * 36 : 4];  // per wave: X transpose (XT)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, hf = lane >> 5;
  const int64_t b = blockIdx.x;
  const int64_t idx = b >> 3;
  const int64_t rb = (idx / a.n_blocks) * 8 + (b & 7);  // XCD-aware: a row block's column blocks share an L2
  const int nb = (int)(idx % a.n_blocks);
  if (rb >= a.row_blocks) return;
  const int64_t M = a.M;
  const int chunks = a.K / KC;
  const int64_t m = rb * kPBM + wv * 32 + r;
  const float* xrow = a.X + (m < M ? m : M - 1) * a.ldx + 4 * hf;  // rows past M re-read row M-1 (never stored)
  f32x16 acc[NT];
  int erow = 0;
  if constexpr (XT) {
    // coalesced: lane l reads floats [4 (l & 7), +4) of rows (l >> 3) + 8 j of the wave's 32
    const float* xr[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t row = rb * kPBM + wv * 32 + (lane >> 3) + 8 * j;
      xr[j] = a.X + (row < M ? row : M - 1) * a.ldx + 4 * (lane & 7);
    }
    auto loadx = [&](int c, float4 (&x)[4]) {
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = ld4(xr[j] + c * KC);
    };
    nnh3_loop<NT, true>(img + (int64_t)nb * chunks * I::ELEMS, sB, chunks, loadx, acc, erow, sF[wv], wv, lane,
                        sX[wv]);
  } else {
    auto loadx = [&](int c, float4 (&x)[4]) {
#pragma unroll
      for (int g = 0; g < 4; ++g) x[g] = ld4(xrow + c * KC + 8 * g);
    };
    nnh3_loop<NT>(img + (int64_t)nb * chunks * I::ELEMS, sB, chunks, loadx, acc, erow, sF[wv], wv, lane);
  }
  float fr[16];  // unscale: 1 / (s_row s_col), both exact powers of two
  split::row_unscale(erow, sF[wv], r, hf, fr);
  const int64_t row0 = rb * kPBM + wv * 32;
  const int n0 = nb * I::BN;
  if constexpr (RK) {
    const int nv = a.nv;
    float ra[NT][kNnhRank], bv[NT], ic[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int col = n0 + 32 * t + r;
      bv[t] = a.bias != nullptr ? a.bias[col] : 0.f;
      ic[t] = ldexpf(a.alpha, -ecol[col]);
#pragma unroll
      for (int v = 0; v < kNnhRank; ++v) ra[t][v] = v < nv ? a.rA[v * a.ldra + col] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int64_t row = row0 + (q & 3) + 8 * (q >> 2) + 4 * hf;
      const int64_t rr = row < M ? row : M - 1;
      float sv[kNnhRank];
#pragma unroll
      for (int v = 0; v < kNnhRank; ++v) sv[v] = v < nv ? a.rS[rr * a.ldrs + v] : 0.f;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        float y = fmaf(acc[t][q] * fr[q], ic[t], bv[t]);
#pragma unroll
        for (int v = 0; v < kNnhRank; ++v)
          if (v < nv) y = fmaf(sv[v], ra[t][v], y);
        if (row < M) a.Y[row * a.ldy + n0 + 32 * t + r] = y;
      }
    }
  } else if constexpr (E4) {
    // the B buffers are idle: every wave passed the last chunk's barrier after its last B reads
    float* T = reinterpret_cast<float*>(sB) + wv * (32 * 40);  // this wave's [32 rows][40] tile
    const int rl = lane >> 3, c4 = 4 * (lane & 7);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int col = n0 + 32 * t + r;
      const float bv = a.bias != nullptr ? a.bias[col] : 0.f;
      const float ic = ldexpf(a.alpha, -ecol[col]);
#pragma unroll
      for (int q = 0; q < 16; ++q) T[((q & 3) + 8 * (q >> 2) + 4 * hf) * 40 + r] = fmaf(acc[t][q] * fr[q], ic, bv);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t row = row0 + rl + 8 * j;
        const float4 v = *reinterpret_cast<const float4*>(T + (rl + 8 * j) * 40 + c4);
        if (row < M) *reinterpret_cast<float4*>(a.Y + row * a.ldy + n0 + 32 * t + c4) = v;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  } else {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int col = n0 + 32 * t + r;
      const float bv = a.bias != nullptr ? a.bias[col] : 0.f;
      const float ic = ldexpf(a.alpha, -ecol[col]);
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int64_t row = row0 + (q & 3) + 8 * (q >> 2) + 4 * hf;
        if (row < M) a.Y[row * a.ldy + col] = fmaf(acc[t][q] * fr[q], ic, bv);
      }
    }
  }
}

// split-K finish: Y = alpha * sum_s part[s] (split order) + bias, float4 per thread
__global__ void __launch_bounds__(256) k_nn_split_sum(const float* __restrict__ part, int64_t M, int N, int splits,
                                                      float alpha, const float* __restrict__ bias,
                                                      float* __restrict__ Y, int64_t ldy) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int n4 = N / 4;
  if (e >= M * n4) return;
  const int64_t row = e / n4;
  const int c = (int)(e % n4) * 4;
  const size_t stride = (size_t)M * N;
  float4 s = ld4(part + row * N + c);
  for (int k = 1; k < splits; ++k) s = add4(s, ld4(part + k * stride + row * N + c));
  float4 o;
  o.x = fmaf(alpha, s.x, bias ? bias[c] : 0.f);
  o.y = fmaf(alpha, s.y, bias ? bias[c + 1] : 0.f);
  o.z = fmaf(alpha, s.z, bias ? bias[c + 2] : 0.f);
  o.w = fmaf(alpha, s.w, bias ? bias[c + 3] : 0.f);
  st4(Y + row * ldy + c, o);
}

// ===========================================================================
// TN GEMM: part[split] = A[rows of split]^T B[rows of split], A [M, Ma], B [M, Nb]
// ===========================================================================
constexpr int kTA = 128;  // a-tile (output rows)
constexpr int kTR = 32;   // rows per LDS chunk

struct TnArg {
  const float* A;
  int64_t lda;
  const float* B;
  int64_t ldb;
  int64_t M;
  int Ma, Nb;
  int tiles_a, tiles_b, splits;
  int64_t rows_per_split;  // multiple of kTR
  float* part;             // [splits, Ma, Nb]
};

// BT: b-tile width (256 or 128).  Waves 2 x 2: wave (wa, wb) owns a-columns [64 wa, +64) (2 MFMA
// tiles) x b-columns [BT/2 wb, +BT/2) (BT/64 tiles).  MFMA: i = a column, j = b column, kk = row.
template <int BT>
__global__ void __launch_bounds__(256, 2) k_gemm_tn(TnArg a) {
  constexpr int NB = BT / 64;  // b tiles per wave
  constexpr int LA = kTA + 4, LB = BT + 4;
  __shared__ float sA[kTR * LA];
  __shared__ float sB[kTR * LB];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r = lane & 31, hf = lane >> 5;
  const int wa = wv & 1, wb = wv >> 1;
  const int T = a.tiles_a * a.tiles_b;
  const int64_t b = blockIdx.x;
  const int64_t idx = b >> 3;
  const int tile = (int)(idx % T);
  const int64_t split = (b & 7) + 8 * (idx / T);  // one split's tiles share an XCD (and its L2)
  if (split >= a.splits) return;
  const int ta = tile % a.tiles_a, tb = tile / a.tiles_a;
  const int64_t r0 = split * a.rows_per_split;
  const int64_t r1 = min(a.M, r0 + a.rows_per_split);
  constexpr int A4 = kTR * kTA / 4 / 256;  // float4 per thread per chunk (4)
  constexpr int B4 = kTR * BT / 4 / 256;   // (8 or 4)
  float4 ar[A4], br[B4];
  auto load = [&](int64_t c0) {
#pragma unroll
    for (int s = 0; s < A4; ++s) {
      const int e = tid + 256 * s;
      const int rr = e / (kTA / 4), c4 = (e % (kTA / 4)) * 4;
      const int64_t row = c0 + rr;
      ar[s] = row < r1 ? ld4(a.A + row * a.lda + ta * kTA + c4) : f4(0.f);
    }
#pragma unroll
    for (int s = 0; s < B4; ++s) {
      const int e = tid + 256 * s;
      const int rr = e / (BT / 4), c4 = (e % (BT / 4)) * 4;
      const int64_t row = c0 + rr;
      br[s] = row < r1 ? ld4(a.B + row * a.ldb + tb * BT + c4) : f4(0.f);
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int s = 0; s < A4; ++s) {
      const int e = tid + 256 * s;
      st4(&sA[(e / (kTA / 4)) * LA + (e % (kTA / 4)) * 4], ar[s]);
    }
#pragma unroll
    for (int s = 0; s < B4; ++s) {
      const int e = tid + 256 * s;
      st4(&sB[(e / (BT / 4)) * LB + (e % (BT / 4)) * 4], br[s]);
    }
  };
  f32x16 acc[2][NB];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int t = 0; t < NB; ++t) acc[u][t] = f32x16{};
  if (r0 < r1) {
    load(r0);
    store();
  }
  __syncthreads();
  for (int64_t c0 = r0; c0 < r1; c0 += kTR) {
    const bool more = c0 + kTR < r1;
    if (more) load(c0 + kTR);
#pragma unroll 4
    for (int s = 0; s < kTR / 2; ++s) {
      const int row = 2 * s + hf;
      float av[2], bv[NB];
#pragma unroll
      for (int u = 0; u < 2; ++u) av[u] = sA[row * LA + 64 * wa + 32 * u + r];
#pragma unroll
      for (int t = 0; t < NB; ++t) bv[t] = sB[row * LB + (BT / 2) * wb + 32 * t + r];
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int t = 0; t < NB; ++t) acc[u][t] = mfma32(av[u], bv[t], acc[u][t]);
    }
    __syncthreads();
    if (more) store();
    __syncthreads();
  }
  float* P = a.part + (size_t)split * a.Ma * a.Nb;
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int t = 0; t < NB; ++t) {
      const int col = tb * BT + (BT / 2) * wb + 32 * t + r;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int arow = ta * kTA + 64 * wa + 32 * u + (q & 3) + 8 * (q >> 2) + 4 * hf;
        P[(size_t)arow * a.Nb + col] = acc[u][t][q];
      }
    }
}

// out[e] = scale * sum_s part[s][e] (split order) -- float4 per thread
__global__ void __launch_bounds__(256) k_split_sum(const float* __restrict__ part, int64_t n4, int splits,
                                                   float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n4) return;
  float4 s = ld4(part + e * 4);
#pragma unroll 8
  for (int k = 1; k < splits; ++k) s = add4(s, ld4(part + ((size_t)k * n4 + e) * 4));  // (loads in flight, adds in order)
  st4(out + e * 4, s);
}

// ===========================================================================
// TN GEMM on the fp16 matrix cores: two-term split with per-column power-of-two scales
// ===========================================================================
// part[split] = A[rows of split]^T B[rows of split] as in k_gemm_tn, but the reduction runs
// over rows, so a row-wise online scale (k_gemm_nnh) cannot apply: each column of A and of B
// gets ONE scale over all M rows -- the power of two that puts the column's largest |v| in
// [2^9, 2^10) (ppgat_split.h scale_exp16) -- from a max pre-pass (k_colmax_bits: the max of
// the IEEE bits of |v|, order-free, so deterministic).  Elements far below their column's max
// keep an absolute error <= 2^-34 of that max; the rest carry 22 bits (2^-21 per product, as
// k_gemm_nnh).  Workgroup tile 128 (A columns) x 256 (B columns), 8 waves (4 x 2), each wave
// one 32-column A block against four 32-column B blocks (64 accumulators); the rows of a
// 32-row chunk are split ONCE by the staging threads into swizzled row-major fp16 images (A:
// [32][128], B: two [32][128] halves; hi and lo terms) and both operands -- columns over the
// chunk's rows -- come back through the transposing ds_read_b64_tr_b16 (conflict-free, see
// k_dxw).  The tiles of one row split run on one XCD, so the rows leave HBM once.
constexpr int kThImg = kTR * 128 * 2;       // bytes per fp16 image [32][128]
constexpr int kThBuf = 6 * kThImg;          // A hi/lo, B half 0 hi/lo, B half 1 hi/lo (48 KB)
constexpr size_t kThLds = 2 * kThBuf + (2 * 128 + 2 * 256 + 16 * 128) * sizeof(float);  // + sC (colsum)

// column maxima of |X| over rows [r0, r1) of a row block, merged into out[] as IEEE bits;
// with rp (CSC pointers [M + 1]) only over the rows that are the source of an edge
__global__ void __launch_bounds__(256) k_colmax_bits(const float* __restrict__ X, int64_t ldx, int64_t M, int C,
                                                     int64_t rows_per_block, const int32_t* __restrict__ rp,
                                                     unsigned* __restrict__ out) {
  __shared__ float4 red[256];
  const int T = C >> 2, P = 256 / T, t = threadIdx.x, cg = t % T, rl = t / T;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block, r1 = min(M, r0 + rows_per_block);
  float4 m = f4(0.f);
  auto mx = [](float4 a, float4 v) {
    return make_float4(fmaxf(a.x, fabsf(v.x)), fmaxf(a.y, fabsf(v.y)), fmaxf(a.z, fabsf(v.z)), fmaxf(a.w, fabsf(v.w)));
  };
  if (rl < P && rp == nullptr) {  // eight rows' loads in flight per thread (a max: any order, same bits)
    int64_t r = r0 + rl;
    for (; r + 7 * P < r1; r += 8 * P) {
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = ld4(X + (r + u * P) * ldx + 4 * cg);
#pragma unroll
      for (int u = 0; u < 8; ++u) m = mx(m, v[u]);
    }
    for (; r < r1; r += P) m = mx(m, ld4(X + r * ldx + 4 * cg));
  } else if (rl < P) {
    for (int64_t r = r0 + rl; r < r1; r += P) {
      if (rp != nullptr && rp[r + 1] == rp[r]) continue;
      const float4 v = ld4(X + r * ldx + 4 * cg);
      m = make_float4(fmaxf(m.x, fabsf(v.x)), fmaxf(m.y, fabsf(v.y)), fmaxf(m.z, fabsf(v.z)), fmaxf(m.w, fabsf(v.w)));
    }
  }
  red[t] = m;
  __syncthreads();
  if (t < T) {
    for (int q = 1; q < P; ++q) {
      const float4 v = red[q * T + t];
      m = make_float4(fmaxf(m.x, v.x), fmaxf(m.y, v.y), fmaxf(m.z, v.z), fmaxf(m.w, v.w));
    }
    atomicMax(out + 4 * t, __float_as_uint(m.x));
    atomicMax(out + 4 * t + 1, __float_as_uint(m.y));
    atomicMax(out + 4 * t + 2, __float_as_uint(m.z));
    atomicMax(out + 4 * t + 3, __float_as_uint(m.w));
  }
}

struct TnhArg {
  const float* A;
  int64_t lda;
  const float* B;
  int64_t ldb;
  int64_t M;
  int Ma, Nb;
  int tiles_a, tiles_b, splits;
  int64_t rows_per_split;
  const unsigned* amax;  // [Ma] column maxima (IEEE bits of |v|)
  int aclamp;            // amax covers only the rows whose B row is nonzero: clamp A's scaled values
  const unsigned* bmax;  // B column n's bound: bmax[n % bperiod] * bscale
  int bperiod;
  float bscale;
  float* part;           // [splits, Ma, Nb]
  float* cpart;          // nullable: [splits, Ma] column sums of A (the workgroups of B tile 0)
};

__device__ __forceinline__ int th_off(int r, int ch) { return 256 * r + 16 * (ch ^ (((r & 3) << 2) | ((r >> 2) & 3))); }

using th_s16x4 = __attribute__((ext_vector_type(4))) short;
__device__ __forceinline__ uint2 th_tr16(const unsigned char* p) {
  const th_s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) th_s16x4*)(p));
  return __builtin_bit_cast(uint2, v);
}

// 4 values times their column scales -> two fp16x4 terms (split2h's arithmetic); clamp: the
// scaled values limited to the fp16 range first (rows a caller's bound does not cover, whose
// product partners are zero: they add 0 instead of inf * 0)
__device__ __forceinline__ void split2h_4(const float4& v, const float4& s, uint2& h, uint2& l, bool clamp = false) {
  float e[4] = {v.x * s.x, v.y * s.y, v.z * s.z, v.w * s.w};
  if (clamp) {
#pragma unroll
    for (int i = 0; i < 4; ++i) e[i] = fminf(fmaxf(e[i], -65504.f), 65504.f);
  }
  uint32_t hh[2], ll[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    hh[i] = split::pk_f16(e[2 * i], e[2 * i + 1]);
    const split::f32x2e back = __builtin_convertvector(__builtin_bit_cast(split::f16x2, hh[i]), split::f32x2e);
    ll[i] = split::pk_f16(e[2 * i] - back.x, e[2 * i + 1] - back.y);
  }
  h = make_uint2(hh[0], hh[1]);
  l = make_uint2(ll[0], ll[1]);
}

__global__ void __launch_bounds__(512, 1) k_gemm_tnh(TnhArg a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char th_lds[];
  float* const sFa = reinterpret_cast<float*>(th_lds + 2 * kThBuf);  // [0,128): 2^e, [128,256): 2^-e
  float* const sFb = sFa + 2 * 128;                                  // [0,256): 2^e, [256,512): 2^-e
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, hf = lane >> 5;
  const int wa = w & 3, wb = w >> 2;
  const int T = a.tiles_a * a.tiles_b;
  const int64_t b = blockIdx.x;
  const int64_t idx = b >> 3;
  const int tile = (int)(idx % T);
  const int64_t split = (b & 7) + 8 * (idx / T);  // one split's tiles share an XCD (and its L2)
  if (split >= a.splits) return;
  const int ta = tile % a.tiles_a, tb = tile / a.tiles_a;
  const int64_t r0 = split * a.rows_per_split;
  const int64_t r1 = min(a.M, r0 + a.rows_per_split);
  const int steps = r1 > r0 ? (int)((r1 - r0 + kTR - 1) / kTR) : 0;
  if (tid < 128) {
    const float m = __uint_as_float(a.amax[ta * 128 + tid]);
    const int e = (m > 0.f && m <= 3.4e38f) ? split::scale_exp16(m) : 0;
    sFa[tid] = ldexpf(1.f, e);
    sFa[128 + tid] = ldexpf(1.f, -e);
  }
  if (tid < 256) {
    const float m = __uint_as_float(a.bmax[(tb * 256 + tid) % a.bperiod]) * a.bscale;
    const int e = (m > 0.f && m <= 3.4e38f) ? split::scale_exp16(m) : 0;
    sFb[tid] = ldexpf(1.f, e);
    sFb[256 + tid] = ldexpf(1.f, -e);
  }
  __syncthreads();

  // ---- staging: thread t -> rows t / 32 and t / 32 + 16 of the chunk, columns 4 (t % 32) .. +3
  // of the A tile and of both B halves ----
  const int sc = (tid & 31) * 4, slr = tid >> 5;
  const float4 sa = *reinterpret_cast<const float4*>(sFa + sc);
  const float4 sb0 = *reinterpret_cast<const float4*>(sFb + sc);
  const float4 sb1 = *reinterpret_cast<const float4*>(sFb + 128 + sc);
  const float* const Ab = a.A + ta * 128 + sc;
  const float* const Bb = a.B + tb * 256 + sc;
  struct Stage {
    float4 a[2], b0[2], b1[2];
  };
  auto load = [&](int64_t row0, Stage& S) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int64_t row = min(row0 + slr + 16 * p, r1 - 1);
      S.a[p] = ld4(Ab + row * a.lda);
      S.b0[p] = ld4(Bb + row * a.ldb);
      S.b1[p] = ld4(Bb + row * a.ldb + 128);
    }
  };
  // column sums of A over this split's rows (cpart; the B tile 0 workgroups of each A tile): the
  // staging thread's 4 columns over its rows in chunk order, the raw values (before any clamp),
  // kept in its own LDS slot sC[slr][sc .. +3] (no registers held across the loop)
  const bool csum = a.cpart != nullptr && tb == 0;
  float4* const sCs = reinterpret_cast<float4*>(sFb + 2 * 256) + slr * 32 + (sc >> 2);  // sC: [16][128]
  if (csum) *sCs = f4(0.f);
  auto put = [&](int buf, int64_t row0, const Stage& S) {
    unsigned char* img = th_lds + buf * kThBuf;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int lr = slr + 16 * p;
      const bool ok = row0 + lr < r1;
      const int off = th_off(lr, sc >> 3) + 8 * ((sc >> 2) & 1);
      if (csum && ok) {
        const float4 c = *sCs;
        *sCs = make_float4(c.x + S.a[p].x, c.y + S.a[p].y, c.z + S.a[p].z, c.w + S.a[p].w);
      }
      uint2 h, l;
      split2h_4(ok ? S.a[p] : f4(0.f), sa, h, l, a.aclamp != 0);
      *reinterpret_cast<uint2*>(img + off) = h;
      *reinterpret_cast<uint2*>(img + kThImg + off) = l;
      split2h_4(ok ? S.b0[p] : f4(0.f), sb0, h, l);
      *reinterpret_cast<uint2*>(img + 2 * kThImg + off) = h;
      *reinterpret_cast<uint2*>(img + 3 * kThImg + off) = l;
      split2h_4(ok ? S.b1[p] : f4(0.f), sb1, h, l);
      *reinterpret_cast<uint2*>(img + 4 * kThImg + off) = h;
      *reinterpret_cast<uint2*>(img + 5 * kThImg + off) = l;
    }
  };

  // transposed-read lane address (see k_dxw): lane 4 q + p of 16-lane group g reads row q of a
  // 4-row block, columns 4 p .. +3 of the group's 16 (16 (g & 1) within a 32-column block)
  const int tg = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
  int oa[4], ob[4][4];  // [2 ks + t] for A; [t'][2 ks + t] for B's four blocks (image-relative)
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int row = 16 * (u >> 1) + 8 * (tg >> 1) + 4 * (u & 1) + tq;
    const int ca = 32 * wa + 16 * (tg & 1) + 4 * tp;
    oa[u] = th_off(row, ca >> 3) + 8 * ((ca >> 2) & 1);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int cb = 32 * t + 16 * (tg & 1) + 4 * tp;
      ob[t][u] = th_off(row, cb >> 3) + 8 * ((cb >> 2) & 1);
    }
  }
  f32x16 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x16{};

  auto compute = [&](const int buf) {
    const unsigned char* img = th_lds + buf * kThBuf;
    const unsigned char* bimg = img + (2 + 2 * wb) * kThImg;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      split::u32x4 fa[2], fb[4][2];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const uint2 v = th_tr16(img + e * kThImg + oa[2 * ks + t]);
          fa[e][2 * t] = v.x;
          fa[e][2 * t + 1] = v.y;
        }
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const uint2 v = th_tr16(bimg + e * kThImg + ob[q][2 * ks + t]);
            fb[q][e][2 * t] = v.x;
            fb[q][e][2 * t + 1] = v.y;
          }
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = split::mfma32_h3(fa, fb[q], acc[q]);
    }
  };

  // two register stages (S0 / S1): chunks c + 1 and c + 2 are in flight while chunk c computes
  // (one stage left the kernel waiting on HBM latency: 48 KB in flight per CU)
  Stage S0, S1;
  if (steps > 0) {
    load(r0, S0);
    load(r0 + kTR, S1);
    put(0, r0, S0);
    __syncthreads();
  }
  for (int st = 0; st < steps; st += 2) {
    load(r0 + (int64_t)(st + 2) * kTR, S0);
    compute(0);
    if (st + 1 < steps) put(1, r0 + (int64_t)(st + 1) * kTR, S1);
    __syncthreads();
    if (st + 1 >= steps) break;
    load(r0 + (int64_t)(st + 3) * kTR, S1);
    compute(1);
    if (st + 2 < steps) put(0, r0 + (int64_t)(st + 2) * kTR, S0);
    __syncthreads();
  }
  // ---- unscale (exact powers of two) and store this split's partial ----
  float* P = a.part + (size_t)split * a.Ma * a.Nb;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int nl = 128 * wb + 32 * t + r;
    const float fb = sFb[256 + nl];
    const int col = tb * 256 + nl;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int ml = 32 * wa + (q & 3) + 8 * (q >> 2) + 4 * hf;
      P[(size_t)(ta * 128 + ml) * a.Nb + col] = acc[t][q] * sFa[128 + ml] * fb;
    }
  }
  if (csum) {  // (workgroup-uniform) the 16 row threads of each column in row-thread order
    const float* sC = sFb + 2 * 256;
    __syncthreads();
    if (tid < 128) {
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < 16; ++q) s += sC[q * 128 + tid];
      a.cpart[(size_t)split * a.Ma + ta * 128 + tid] = s;
    }
  }
}

// ---------------------------------------------------------------------------
// k_gemm_tnh256: k_gemm_tnh with a 256 x 256 output tile (A's 256 columns x B's 256) when Ma is a
// multiple of 256 (config 5's weight gradient G = g^T agg: Ma = 256, Nb = 1024).  The 128 x 256
// tile split every staged A row once per B tile (four times) and every B row once per A tile
// (twice): 3,072 fp16 splits per row of the product against 2,048 here (A four times, B once).
// 16 waves (1,024 threads, four per SIMD, <= 128 registers): wave w owns A block w & 7 (32
// columns) x B half w >> 3 (128 columns), acc[4] as in k_gemm_tnh; threads 0-511 stage the two
// A halves, 512-1023 the two B halves, two rows x four columns of each per thread, one register
// stage (chunk c + 1 loads while chunk c computes).  LDS: two buffers of eight [32][128] fp16
// images (A half 0/1 and B half 0/1, hi/lo each) = 128 KB, + scales + colsum slots.  The row
// splits are tnh_splits(M, tiles of the 128 x 256 kernel) and every output element takes
// k_gemm_tnh's products in k_gemm_tnh's order: the same bits (tests/test_gpu_gemm_f16.py).
// ---------------------------------------------------------------------------
constexpr int kTh2Buf = 8 * kThImg;  // 64 KB
constexpr size_t kTh2Lds = 2 * kTh2Buf + (2 * 256 + 2 * 256 + 16 * 256) * sizeof(float);

__global__ void __launch_bounds__(1024, 1) k_gemm_tnh256(TnhArg a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char th_lds[];
  float* const sFa = reinterpret_cast<float*>(th_lds + 2 * kTh2Buf);  // [0,256): 2^e, [256,512): 2^-e
  float* const sFb = sFa + 2 * 256;                                   // [0,256): 2^e, [256,512): 2^-e
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, hf = lane >> 5;
  const int wa = w & 7, wb = w >> 3;
  const int T = a.tiles_a * a.tiles_b;
  const int64_t b = blockIdx.x;
  const int64_t idx = b >> 3;
  const int tile = (int)(idx % T);
  const int64_t split = (b & 7) + 8 * (idx / T);  // one split's tiles share an XCD (and its L2)
  if (split >= a.splits) return;
  const int ta = tile % a.tiles_a, tb = tile / a.tiles_a;
  const int64_t r0 = split * a.rows_per_split;
  const int64_t r1 = min(a.M, r0 + a.rows_per_split);
  const int steps = r1 > r0 ? (int)((r1 - r0 + kTR - 1) / kTR) : 0;
  if (tid < 256) {
    const float m = __uint_as_float(a.amax[ta * 256 + tid]);
    const int e = (m > 0.f && m <= 3.4e38f) ? split::scale_exp16(m) : 0;
    sFa[tid] = ldexpf(1.f, e);
    sFa[256 + tid] = ldexpf(1.f, -e);
  } else if (tid < 512) {
    const int c = tid - 256;
    const float m = __uint_as_float(a.bmax[(tb * 256 + c) % a.bperiod]) * a.bscale;
    const int e = (m > 0.f && m <= 3.4e38f) ? split::scale_exp16(m) : 0;
    sFb[c] = ldexpf(1.f, e);
    sFb[256 + c] = ldexpf(1.f, -e);
  }
  __syncthreads();

  // ---- staging: thread t -> operand t >> 9 (A / B), rows (t >> 5) & 15 and + 16 of the chunk,
  // columns 4 (t % 32) .. +3 of both 128-column halves of that operand ----
  const int sc = (tid & 31) * 4, slr = (tid >> 5) & 15, isb = tid >> 9;
  const float* const src = isb ? a.B + tb * 256 + sc : a.A + ta * 256 + sc;
  const int64_t ld = isb ? a.ldb : a.lda;
  const float* const scl = (isb ? sFb : sFa) + sc;
  const bool clamp = !isb && a.aclamp != 0;
  float4 S[2][2];  // [row p][half]
  auto load = [&](int64_t row0) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int64_t row = min(row0 + slr + 16 * p, r1 - 1);
      S[p][0] = ld4(src + row * ld);
      S[p][1] = ld4(src + row * ld + 128);
    }
  };
  // column sums of A (cpart; the B tile 0 workgroups): the A staging thread's 4 columns of each
  // half over its rows in chunk order, raw values, in its own LDS slots sC[slr][256]
  const bool csum = a.cpart != nullptr && tb == 0 && !isb;
  float4* const sCs = reinterpret_cast<float4*>(sFb + 2 * 256) + slr * 64 + (sc >> 2);  // sC: [16][256]
  if (csum) {
    sCs[0] = f4(0.f);
    sCs[32] = f4(0.f);
  }
  auto put = [&](int buf, int64_t row0) {
    unsigned char* img = th_lds + buf * kTh2Buf + 4 * isb * kThImg;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int lr = slr + 16 * p;
      const bool ok = row0 + lr < r1;
      const int off = th_off(lr, sc >> 3) + 8 * ((sc >> 2) & 1);
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        if (csum && ok) {
          const float4 c = sCs[32 * hh];
          sCs[32 * hh] = make_float4(c.x + S[p][hh].x, c.y + S[p][hh].y, c.z + S[p][hh].z, c.w + S[p][hh].w);
        }
        uint2 h, l;
        split2h_4(ok ? S[p][hh] : f4(0.f), *reinterpret_cast<const float4*>(scl + 128 * hh), h, l, clamp);
        *reinterpret_cast<uint2*>(img + 2 * hh * kThImg + off) = h;
        *reinterpret_cast<uint2*>(img + (2 * hh + 1) * kThImg + off) = l;
      }
    }
  };

  // transposed-read lane address (as k_gemm_tnh): lane 4 q + p of 16-lane group g reads row q of
  // a 4-row block, columns 4 p .. +3 of the group's 16 (16 (g & 1) within a 32-column block)
  // th_off(row, (32 blk + c0) >> 3) + 8 ((c0 >> 2) & 1) with c0 = 16 (tg & 1) + 4 tp splits into a
  // row part and a block part: the row's swizzle is (tq << 2) | (2 (tg >> 1) + (u & 1)) for every
  // row this lane reads, so block blk sits at 64 (blk ^ tq) -- 9 registers instead of 20
  const int tg = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
  const int c0 = 16 * (tg & 1) + 4 * tp;
  int obase[4], oq[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int row = 16 * (u >> 1) + 8 * (tg >> 1) + 4 * (u & 1) + tq;
    obase[u] = 256 * row + 16 * ((c0 >> 3) ^ (2 * (tg >> 1) + (u & 1))) + 8 * ((c0 >> 2) & 1);
    oq[u] = 64 * (u ^ tq);
  }
  const int oqa = 64 * ((wa & 3) ^ tq);
  f32x16 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x16{};

  auto compute = [&](const int buf) {
    const unsigned char* img = th_lds + buf * kTh2Buf;
    const unsigned char* aimg = img + 2 * (wa >> 2) * kThImg;
    const unsigned char* bimg = img + (4 + 2 * wb) * kThImg;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      split::u32x4 fa[2];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const uint2 v = th_tr16(aimg + e * kThImg + obase[2 * ks + t] + oqa);
          fa[e][2 * t] = v.x;
          fa[e][2 * t + 1] = v.y;
        }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        split::u32x4 fb[2];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const uint2 v = th_tr16(bimg + e * kThImg + obase[2 * ks + t] + oq[q]);
            fb[e][2 * t] = v.x;
            fb[e][2 * t + 1] = v.y;
          }
        acc[q] = split::mfma32_h3(fa, fb, acc[q]);
      }
    }
  };

  if (steps > 0) {
    load(r0);
    put(0, r0);
    __syncthreads();
  }
  for (int st = 0; st < steps; ++st) {
    const bool more = st + 1 < steps;
    if (more) load(r0 + (int64_t)(st + 1) * kTR);
    compute(st & 1);
    if (more) put((st + 1) & 1, r0 + (int64_t)(st + 1) * kTR);
    __syncthreads();
  }
  // ---- unscale (exact powers of two) and store this split's partial ----
  float* P = a.part + (size_t)split * a.Ma * a.Nb;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int nl = 128 * wb + 32 * t + r;
    const float fb = sFb[256 + nl];
    const int col = tb * 256 + nl;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int ml = 32 * wa + (q & 3) + 8 * (q >> 2) + 4 * hf;
      P[(size_t)(ta * 256 + ml) * a.Nb + col] = acc[t][q] * sFa[256 + ml] * fb;
    }
  }
  if (a.cpart != nullptr && tb == 0) {  // (workgroup-uniform) the 16 row threads of each column in order
    const float* sC = sFb + 2 * 256;
    __syncthreads();
    if (tid < 256) {
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < 16; ++q) s += sC[q * 256 + tid];
      a.cpart[(size_t)split * a.Ma + ta * 256 + tid] = s;
    }
  }
}

}  // namespace

// ===========================================================================
// host launchers
// ===========================================================================
bool gemm_nn_shape_ok(int64_t M, int K, int N, int bmode) {
  return M >= 0 && K >= kGBK && K % kGBK == 0 && N >= 128 && N % 128 == 0 && (bmode == 0 || bmode == 1);
}

// split-K for small M (few row blocks, long K): the partial tiles go to the caller's workspace
int gemm_nn_splits(int64_t M, int K, int N) {
  const int64_t tiles = (M + kGBM - 1) / kGBM * (N / (N % 256 == 0 ? 256 : 128));
  if (tiles >= 128 || K < 4 * kGBK) return 1;
  int s = 1;
  while (s * 2 * tiles <= 256 && (K / kGBK) >= 4 * s * 2 && s < 32) s *= 2;  // >= 4 chunks per split
  return s;
}

// bytes of the three bf16 images of B [K x N] per (column block of 32 nt columns, 32-deep k
// chunk); only the lab build writes them (nnx_presplit), both builds size workspaces by them
size_t nnx_image_bytes(int K, int N, int nt) {
  const size_t img = nt == 8 ? (size_t)NnpImg<8>::BYTES : (size_t)NnpImg<4>::BYTES;
  return (size_t)(N / (32 * nt)) * (size_t)(K / 32) * img;
}

#ifdef PPGAT_LAB_BUILD
#include "lab/ppgat_xform_lab.h"  // the superseded kernel generations, their switches and launches
#endif

// the pre-split path: large M, K % 32 == 0, on k_gemm_nnh3, which takes the K chunks in pairs:
// other shapes go to the general x6 kernel (k_gemm_nnx)
static bool nnp_ok(int64_t M, int K, int N) {
  bool chunks_ok = (K / kGBK) % 2 == 0;
#ifdef PPGAT_LAB_BUILD
  chunks_ok = chunks_ok || lab::odd_chunks_ok();
#endif
  return chunks_ok && gemm_split_enabled() && M >= 4 * kPBM && K % 32 == 0 && N % 128 == 0 &&
         gemm_nn_splits(M, K, N) == 1;
}

static size_t nnp_image_bytes(int K, int N) { return nnx_image_bytes(K, N, N % 256 == 0 ? 8 : 4); }

// the fp16 two-term family (the pre-split NN path, k_gemm_tnh): always on in libppgat.so
static bool nnh_enabled() {
#ifdef PPGAT_LAB_BUILD
  if (lab::f16_off()) return false;
#endif
  return true;
}

size_t nnh_image_bytes(int K, int N, int nt) {
  const size_t img = nt == 8 ? (size_t)NnhImg<8>::BYTES : (size_t)NnhImg<4>::BYTES;
  return (size_t)(N / (32 * nt)) * (size_t)(K / 32) * img;
}

// B's column scales and two fp16 images (layout as nnx_presplit's, two parts instead of three)
hipError_t nnh_presplit(const float* B, int64_t ldb, int bmode, int K, int N, int nt, uint16_t* img, int* ecol,
                        hipStream_t st) {
  const int64_t groups = (int64_t)N * (K / 4);
  if (groups <= 0) return hipSuccess;
  const unsigned gc = (unsigned)((N + 3) / 4), gp = (unsigned)((groups + 255) / 256);
  if (bmode == 0) hipLaunchKernelGGL((k_colscale16<0>), dim3(gc), dim3(256), 0, st, B, ldb, K, N, ecol);
  else hipLaunchKernelGGL((k_colscale16<1>), dim3(gc), dim3(256), 0, st, B, ldb, K, N, ecol);
#define PPGAT_NNH_PRE(NT_, BM_) \
  hipLaunchKernelGGL((k_nnh_presplit<NT_, BM_>), dim3(gp), dim3(256), 0, st, B, ldb, K, N, ecol, img)
  if (nt == 8) {
    if (bmode == 0) PPGAT_NNH_PRE(8, 0); else PPGAT_NNH_PRE(8, 1);
  } else {
    if (bmode == 0) PPGAT_NNH_PRE(4, 0); else PPGAT_NNH_PRE(4, 1);
  }
#undef PPGAT_NNH_PRE
  return hipGetLastError();
}

static size_t nnq_bytes(int K, int N) {  // image + column exponents, either family
  const int nt = N % 256 == 0 ? 8 : 4;
  return nnh_enabled() ? align_up(nnh_image_bytes(K, N, nt)) + align_up((size_t)N * 4) : nnp_image_bytes(K, N);
}

size_t gemm_nn_workspace_bytes(int64_t M, int K, int N) {
  if (nnp_ok(M, K, N)) return align_up(nnq_bytes(K, N));
  const int s = gemm_nn_splits(M, K, N);
  return s > 1 ? align_up((size_t)s * M * N * 4) : 0;
}

hipError_t gemm_nn(const float* X, int64_t ldx, int64_t M, int K, const float* B, int64_t ldb, int bmode, int N,
                   float alpha, const float* bias, float* Y, int64_t ldy, hipStream_t st, void* ws, const float* rS,
                   int64_t ldrs, int nv, const float* rA, int64_t ldra) {
  if (M <= 0) return hipSuccess;
  if (nv > 0 && !(ws != nullptr && nnp_ok(M, K, N) && nnh_enabled() && nv <= kNnhRank)) {
    // no fused epilogue on this path: the GEMM, then the rank update as its own pass
    hipError_t e = gemm_nn(X, ldx, M, K, B, ldb, bmode, N, alpha, bias, Y, ldy, st, ws);
    if (e != hipSuccess) return e;
    return rank_update(rS, ldrs, nv, rA, ldra, M, N, Y, ldy, st);
  }
  NnArg a{};
  a.rS = rS; a.ldrs = ldrs; a.nv = nv; a.rA = rA; a.ldra = ldra;
  a.X = X; a.ldx = ldx; a.M = M; a.K = K; a.B = B; a.ldb = ldb; a.N = N; a.alpha = alpha; a.bias = bias;
  a.Y = Y; a.ldy = ldy;
  if (ws != nullptr && nnp_ok(M, K, N)) {  // B pre-split once, then k_gemm_nnh3
    const bool w8 = N % 256 == 0;
    uint16_t* img = static_cast<uint16_t*>(ws);
    a.row_blocks = (M + kPBM - 1) / kPBM;
    a.n_blocks = N / (w8 ? 256 : 128);
    a.splits = 1;
    const unsigned grid = (unsigned)((a.row_blocks + 7) / 8 * 8 * a.n_blocks);
#ifdef PPGAT_LAB_BUILD
    if (hipError_t e; lab::gemm_nn_presplit(a, bmode, w8, grid, ws, st, &e)) return e;
#endif
    // fp16 two-term split: three MFMAs per product
    int* ecol = reinterpret_cast<int*>(reinterpret_cast<char*>(ws) + align_up(nnh_image_bytes(K, N, w8 ? 8 : 4)));
    hipError_t e = nnh_presplit(B, ldb, bmode, K, N, w8 ? 8 : 4, img, ecol, st);
    if (e != hipSuccess) return e;
#define PPGAT_NNH3(NT_, RK_) \
  hipLaunchKernelGGL((k_gemm_nnh3<NT_, RK_>), dim3(grid), dim3(512), 0, st, a, img, ecol)
    if (nv > 0) {
      if (w8) PPGAT_NNH3(8, true); else PPGAT_NNH3(4, true);
    } else {
      if (w8) PPGAT_NNH3(8, false); else PPGAT_NNH3(4, false);
    }
#undef PPGAT_NNH3
    return hipGetLastError();
  }
  a.row_blocks = (M + kGBM - 1) / kGBM;
  const int64_t padded = (a.row_blocks + 7) / 8 * 8;
  const bool wide = N % 256 == 0;
  a.n_blocks = N / (wide ? 256 : 128);
  a.splits = ws != nullptr ? gemm_nn_splits(M, K, N) : 1;
  if (a.splits > 1) {  // every split non-empty: splits = ceil(chunks / chunks per split)
    const int chunks = K / kGBK;
    const int per = (chunks + a.splits - 1) / a.splits;
    a.k_per = per * kGBK;
    a.splits = (chunks + per - 1) / per;
    a.part = static_cast<float*>(ws);
  }
  if (gemm_split_enabled()) {  // split bf16 matrix cores, two workgroups per CU
    a.n_blocks = N / 128;
    // 256-wide tiles when N allows (measured at config-5 shapes: 5.6-6.5 ms against 5.9-7.0 for
    // 128-wide tiles or 64-deep k chunks, profiles/r02/v13_gemm_split_cfg5.log)
    const bool w8 = N % 256 == 0;
    if (w8) a.n_blocks = N / 256;
    const unsigned gv = a.splits > 1 ? (unsigned)(a.row_blocks * a.n_blocks * a.splits)
                                     : (unsigned)(padded * a.n_blocks);
#define PPGAT_NNX(NT_, KC_)                                                                     \
  do {                                                                                          \
    if (bmode == 0) hipLaunchKernelGGL((k_gemm_nnx<NT_, 0, KC_>), dim3(gv), dim3(256), 0, st, a); \
    else hipLaunchKernelGGL((k_gemm_nnx<NT_, 1, KC_>), dim3(gv), dim3(256), 0, st, a);            \
  } while (0)
    if (w8) PPGAT_NNX(8, 32);
    else PPGAT_NNX(4, 32);
#undef PPGAT_NNX
  } else {
  const unsigned grid = a.splits > 1 ? (unsigned)(a.row_blocks * a.n_blocks * a.splits)
                                     : (unsigned)(padded * a.n_blocks);
#define PPGAT_NN(NT_, BM_) hipLaunchKernelGGL((k_gemm_nn<NT_, BM_>), dim3(grid), dim3(256), 0, st, a)
  if (wide) {
    if (bmode == 0) PPGAT_NN(8, 0); else PPGAT_NN(8, 1);
  } else {
    if (bmode == 0) PPGAT_NN(4, 0); else PPGAT_NN(4, 1);
  }
#undef PPGAT_NN
  }
  if (a.splits > 1) {
    const int64_t n4 = M * (N / 4);
    hipLaunchKernelGGL(k_nn_split_sum, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, a.part, M, N, a.splits,
                       alpha, bias, Y, ldy);
  }
  return hipGetLastError();
}

static int tn_splits(int64_t M, int T) {
  int s = 8;
  while (s < 512 && (int64_t)s * T < 512 && M / (2 * s) >= 4 * kTR) s *= 2;
  return s;
}

bool gemm_tn_big_shape_ok(int Ma, int Nb) { return Ma >= 128 && Ma % 128 == 0 && Nb >= 128 && Nb % 128 == 0; }

// the fp16 two-term TN kernel (k_gemm_tnh): Nb % 256 == 0, with the fp16 family on, and long
// reductions only -- below ~64k rows its three extra launches (max buffer clear, two column-max
// passes) cost more than the fp32 kernel's MFMA time (the FusionMLP training batch of 512 rows)
static bool tnh_ok(int64_t M, int Ma, int Nb) {
  return gemm_split_enabled() && nnh_enabled() && M >= 65536 && Ma % 128 == 0 && Nb % 256 == 0;
}
static int tnh_splits(int64_t M, int T) {  // one workgroup per CU: splits * tiles <= 256, >= 128 rows per split
  // two workgroup rounds per CU: the same time as one (3.96 vs 3.98 ms at the config-5 share,
  // profiles/r03/v16_tnh_*), half the rows per fp32 accumulator chain: 3.3e-6 vs 5.3e-6
  // max-abs/max-abs on 1.875M-row reductions (fp32 MFMA kernel: 3.5e-6)
  constexpr int waves = 2;
  int s = 256 * waves / T;
  if (s < 1) s = 1;
  while (s > 1 && M / s < 4 * kTR) s /= 2;
  return s;
}

// (+ the column sums' partials: [splits, Ma] on the fp16 path, the colsum kernel's otherwise)
size_t gemm_tn_big_workspace_bytes(int64_t M, int Ma, int Nb) {
  if (tnh_ok(M, Ma, Nb)) {
    const int T = (Ma / 128) * (Nb / 256);
    const int s = tnh_splits(M, T);
    return align_up((size_t)s * Ma * Nb * 4) + align_up((size_t)(Ma + Nb) * 4) + align_up((size_t)s * Ma * 4);
  }
  const int T = (Ma / kTA) * (Nb / (Nb % 256 == 0 ? 256 : 128));
  return align_up((size_t)tn_splits(M, T) * Ma * Nb * 4) + align_up((size_t)colsum_blocks(M) * 256 * 4);
}

static hipError_t colmax_bits(const float* X, int64_t ldx, int64_t M, int C, unsigned* out, hipStream_t st,
                              const int32_t* rp = nullptr) {
  // C columns in slices of <= 1024 (256 float4 lanes per row pass)
  for (int c0 = 0; c0 < C; c0 += 1024) {
    const int c = C - c0 < 1024 ? C - c0 : 1024;
    int64_t blocks = (M + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    const int64_t rpb = (M + blocks - 1) / blocks;
    blocks = (M + rpb - 1) / rpb;
    hipLaunchKernelGGL(k_colmax_bits, dim3((unsigned)blocks), dim3(256), 0, st, X + c0, ldx, M, c, rpb, rp, out + c0);
  }
  return hipGetLastError();
}

hipError_t colmax_abs(const float* X, int64_t ldx, int64_t M, int C, unsigned* out, hipStream_t st,
                      const int32_t* src_ptr) {
  hipError_t e = hipMemsetAsync(out, 0, (size_t)C * 4, st);
  if (e == hipSuccess && M > 0) e = colmax_bits(X, ldx, M, C, out, st, src_ptr);
  return e;
}

hipError_t gemm_tn_big(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t M, int Ma, int Nb, float* out,
                       void* ws, hipStream_t st, const unsigned* b_bound, int b_period, float b_scale,
                       const unsigned* a_bound, float* colsum_out) {
  if (M <= 0) {  // empty sums (no partials)
    hipError_t e = hipMemsetAsync(out, 0, (size_t)Ma * Nb * 4, st);
    if (e == hipSuccess && colsum_out) e = hipMemsetAsync(colsum_out, 0, (size_t)Ma * 4, st);
    return e;
  }
  if (tnh_ok(M, Ma, Nb)) {
    static const bool attr = [] {
      return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gemm_tnh), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)kThLds) == hipSuccess;
    }();
    (void)attr;
    TnhArg a{};
    a.A = A; a.lda = lda; a.B = B; a.ldb = ldb; a.M = M; a.Ma = Ma; a.Nb = Nb;
    a.tiles_a = Ma / 128;
    a.tiles_b = Nb / 256;
    const int T = a.tiles_a * a.tiles_b;
    a.splits = tnh_splits(M, T);
    a.rows_per_split = ((M + a.splits - 1) / a.splits + kTR - 1) / kTR * kTR;
    a.part = static_cast<float*>(ws);
    unsigned* mx = reinterpret_cast<unsigned*>(static_cast<char*>(ws) + align_up((size_t)a.splits * Ma * Nb * 4));
    a.amax = a_bound ? a_bound : mx;       // a caller's bound of |A| (rows with nonzero B) skips A's pass
    a.aclamp = a_bound ? 1 : 0;
    a.bmax = b_bound ? b_bound : mx + Ma;  // a caller's bound of |B| per column skips B's pass
    a.bperiod = b_bound ? b_period : Nb;
    a.bscale = b_bound ? b_scale : 1.f;
    a.cpart = colsum_out ? reinterpret_cast<float*>(reinterpret_cast<char*>(mx) + align_up((size_t)(Ma + Nb) * 4))
                         : nullptr;
    hipError_t e = hipSuccess;
    if (!a_bound || !b_bound) e = hipMemsetAsync(mx, 0, (size_t)(Ma + Nb) * 4, st);
    if (e == hipSuccess && !a_bound) e = colmax_bits(A, lda, M, Ma, mx, st);
    if (e == hipSuccess && !b_bound) e = colmax_bits(B, ldb, M, Nb, mx + Ma, st);
    if (e != hipSuccess) return e;
    bool t256 = Ma % 256 == 0;  // the 256 x 256 tile, the same row splits (the same bits)
#ifdef PPGAT_LAB_BUILD
    t256 = t256 && !lab::tnh256_off();
#endif
    if (t256) {
      static const bool attr2 = [] {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gemm_tnh256),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTh2Lds) == hipSuccess;
      }();
      (void)attr2;
      a.tiles_a = Ma / 256;
      const int T2 = a.tiles_a * a.tiles_b;
      hipLaunchKernelGGL(k_gemm_tnh256, dim3((unsigned)(8 * T2 * ((a.splits + 7) / 8))), dim3(1024), kTh2Lds, st, a);
    } else {
      const unsigned grid = (unsigned)(8 * T * ((a.splits + 7) / 8));
      hipLaunchKernelGGL(k_gemm_tnh, dim3(grid), dim3(512), kThLds, st, a);
    }
    const int64_t n4 = (int64_t)Ma * Nb / 4;
    hipLaunchKernelGGL(k_split_sum, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, a.part, n4, a.splits, out);
    if (colsum_out)
      hipLaunchKernelGGL(k_split_sum, dim3((unsigned)((Ma / 4 + 255) / 256)), dim3(256), 0, st, a.cpart,
                         (int64_t)Ma / 4, a.splits, colsum_out);
    return hipGetLastError();
  }
  const bool wide = Nb % 256 == 0;
  TnArg a{};
  a.A = A; a.lda = lda; a.B = B; a.ldb = ldb; a.M = M; a.Ma = Ma; a.Nb = Nb;
  a.tiles_a = Ma / kTA;
  a.tiles_b = Nb / (wide ? 256 : 128);
  const int T = a.tiles_a * a.tiles_b;
  a.splits = tn_splits(M, T);
  a.rows_per_split = ((M + a.splits - 1) / a.splits + kTR - 1) / kTR * kTR;
  a.part = static_cast<float*>(ws);
  const unsigned grid = (unsigned)(8 * T * ((a.splits + 7) / 8));
  if (wide) hipLaunchKernelGGL((k_gemm_tn<256>), dim3(grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((k_gemm_tn<128>), dim3(grid), dim3(256), 0, st, a);
  const int64_t n4 = (int64_t)Ma * Nb / 4;
  hipLaunchKernelGGL(k_split_sum, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, a.part, n4, a.splits, out);
  if (colsum_out) {  // the colsum kernel over 256- (or 128-) column slabs of A
    float* part = reinterpret_cast<float*>(static_cast<char*>(ws) + align_up((size_t)a.splits * Ma * Nb * 4));
    for (int c0 = 0; c0 < Ma; c0 += 256) {
      const hipError_t e = colsum(A + c0, lda, M, Ma - c0 >= 256 ? 256 : 128, colsum_out + c0, part, st);
      if (e != hipSuccess) return e;
    }
  }
  return hipGetLastError();
}

}  // namespace ppgat
