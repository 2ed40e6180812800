// lab/ppgat_fusion_lab.h -- the superseded FusionMLP forward kernels and their dispatch.  Lab
// builds only (make lab, -DPPGAT_LAB_BUILD=1): ppgat_fusion.hip includes this file once, inside
// namespace ppgat, after the product kernels and helpers it uses (PBM, kPatchB, kH1Img ...,
// the split helpers, row_of).  Never part of libppgat.so.
//
//   PPGAT_GEMM_F16=0      k_fusion_fwdp  (bf16 x6, W1 / W2 pre-split by nnx_presplit)
//   PPGAT_NNH2=0 or 2     k_fusion_fwdh  (fp16 two-term, the unpipelined GEMM1 loop)
//   odd chunk counts      k_fusion_fwdh
// Everything else falls through to the product dispatch (k_fusion_fwdh3).
#pragma once

#include "ppgat_lab_switches.h"

namespace {

// ---------------------------------------------------------------------------
// The same MLP with W1 and W2 pre-split once per call (ppgat::nnx_presplit: the three bf16
// images per 32-deep chunk in exactly the layout k_fusion_fwdx builds in LDS, so the products
// and results are bitwise those of k_fusion_fwdx) and staged by global_load_lds_dwordx4:
// 8 waves = 256 rows per workgroup share every staged chunk, two LDS buffers, one barrier
// per chunk.  k_fusion_fwdx splits each chunk while staging it (VALU beside the MFMAs) and
// waits at two barriers per chunk (PMC: MFMA busy 0.51, profiles/r02/v15_fusion_fwdx_pmc.json).
// LDS: GEMM1 2 x 61,440 B; GEMM2 reuses it: 8 wave patches (36,864 B) + 2 x 30,720 B W2 slices.
// ---------------------------------------------------------------------------
constexpr int kW1Img = 3 * XP1;                // bf16 per W1 chunk image
constexpr int kW2Img = 3 * XP2;                // bf16 per W2 slice image

// buffer_load ... lds (MUBUF LDS-DMA, tracked on vmcnt only): with global_load_lds the compiler
// turned every LDS-read wait behind it into lgkmcnt(0), so no fragment read overlapped an MFMA
__device__ __forceinline__ void glds_copy(const uint16_t* src, uint16_t* dst, int bytes, int wv, int lane) {
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(src), 0, bytes, 0x00020000);
  char* d = reinterpret_cast<char*>(dst);
  for (int i = wv; i < bytes / 1024; i += 8)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(d + i * 1024), 16,
                                             lane * 16 + i * 1024, 0, 0, 0);
}

__global__ void __launch_bounds__(512, 1) k_fusion_fwdp(const float* __restrict__ txt, const float* __restrict__ img,
                                                        const int32_t* __restrict__ img_index,
                                                        const float* __restrict__ img_fallback, int64_t B, int Dt,
                                                        int Di, const uint16_t* __restrict__ w1i,
                                                        const float* __restrict__ b1, const uint16_t* __restrict__ w2i_g,
                                                        const float* __restrict__ b2, int normalize,
                                                        float* __restrict__ out, float* __restrict__ z1_out) {
  static_assert(kW1Img * 2 % 1024 == 0 && kW2Img * 2 % 1024 == 0, "1-KB wave copies");
  __shared__ __attribute__((aligned(16))) uint16_t lds[2 * kW1Img];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, hf = lane >> 5;
  const int64_t row0 = (int64_t)blockIdx.x * PBM + 32 * w;
  const int K = Dt + Di, chunks = K / BK;
  const int64_t b = row0 + r < B ? row0 + r : B - 1;
  const float* trow = txt + b * Dt + 4 * hf;
  const float* irow;
  if (Di > 0) {
    const int32_t ii = img_index ? img_index[b] : (int32_t)b;
    irow = (ii >= 0 ? img + (int64_t)ii * Di : img_fallback) + 4 * hf;
  } else {
    irow = trow;
  }
  auto load_x = [&](int k0, float4 (&xv)[4]) {
    const float* src = k0 < Dt ? trow + k0 : irow + (k0 - Dt);
#pragma unroll
    for (int g = 0; g < 4; ++g) xv[g] = ld4(src + 8 * g);
  };

  // ---- GEMM1 ----
  f32x16 acc[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) acc[t] = f32x16{};
  float4 xa[4], xn[4];
  load_x(0, xa);
  glds_copy(w1i, lds, kW1Img * 2, w, lane);
  __syncthreads();  // vmcnt(0): chunk 0 and the first x fragments have landed
  for (int c = 0; c < chunks; ++c) {
    const uint16_t* sb = lds + (c & 1) * kW1Img;
    const bool more = c + 1 < chunks;
    if (more) {
      glds_copy(w1i + (int64_t)(c + 1) * kW1Img, lds + ((c + 1) & 1) * kW1Img, kW1Img * 2, w, lane);
      load_x((c + 1) * BK, xn);
    }
    auto read_w = [&](int idx, split::u32x4 (&f)[3]) {
      const int off = (32 * (idx & 7) + r) * XLD + 16 * (idx >> 3) + 8 * hf;
#pragma unroll
      for (int p = 0; p < 3; ++p) f[p] = *reinterpret_cast<const split::u32x4*>(&sb[p * XP1 + off]);
    };
    // two fragment sets used alternately; each step issues the next step's three LDS reads
    // before its six MFMAs (see k_gemm_nnp)
    split::u32x4 fx[3], fb[2][3];
    read_w(0, fb[0]);
#pragma unroll
    for (int idx = 0; idx < 16; ++idx) {
      const int u = idx >> 3, t = idx & 7;
      if (t == 0) split::split3(xa[2 * u], xa[2 * u + 1], fx[0], fx[1], fx[2]);
      if (idx + 1 < 16) read_w(idx + 1, fb[(idx + 1) & 1]);
      acc[t] = split::mfma32_x6(fx, fb[idx & 1], acc[t]);
      if (idx + 1 < 16) __builtin_amdgcn_sched_group_barrier(0x0100, 3, 0);
      __builtin_amdgcn_sched_group_barrier(0x0008, 6, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();  // chunk c + 1 landed; every wave is done with this buffer
    if (more) {
#pragma unroll
      for (int g = 0; g < 4; ++g) xa[g] = xn[g];
    }
  }

  // ---- GEMM2 over eight 32-column slices of h (W2 slice images double-buffered after the patches) ----
  float* hp = reinterpret_cast<float*>(lds) + w * 32 * XLH;                   // this wave's patch [32][XLH]
  uint16_t* w2s = lds + kPatchB / 2;                                           // [2][3][128][XLD]
  f32x16 acc2[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) acc2[u] = f32x16{};
  glds_copy(w2i_g, w2s, kW2Img * 2, w, lane);
#pragma unroll
  for (int c = 0; c < H1 / BK; ++c) {
    const int col = BK * c + r;
    const float bias = b1[col];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int row = row_of(q, hf);
      const float z = acc[c][q] + bias;
      hp[row * XLH + r] = fmaxf(z, 0.f);
      if (z1_out != nullptr && row0 + row < B) z1_out[(row0 + row) * H1 + col] = z;
    }
    __syncthreads();  // vmcnt(0): slice c landed; the patch is written
    if (c + 1 < H1 / BK) glds_copy(w2i_g + (int64_t)(c + 1) * kW2Img, w2s + ((c + 1) & 1) * kW2Img, kW2Img * 2, w, lane);
    const uint16_t* ws2 = w2s + (c & 1) * kW2Img;
    auto read_w2 = [&](int i, split::u32x4 (&f)[3]) {
      const int off = (32 * (i & 3) + r) * XLD + 16 * (i >> 2) + 8 * hf;
#pragma unroll
      for (int p = 0; p < 3; ++p) f[p] = *reinterpret_cast<const split::u32x4*>(&ws2[p * XP2 + off]);
    };
    split::u32x4 fh[3], fb2[2][3];
    read_w2(0, fb2[0]);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int u = i >> 2, uu = i & 3;
      if (uu == 0)
        split::split3(ld4(&hp[r * XLH + 16 * u + 4 * hf]), ld4(&hp[r * XLH + 16 * u + 8 + 4 * hf]), fh[0], fh[1],
                      fh[2]);
      if (i + 1 < 8) read_w2(i + 1, fb2[(i + 1) & 1]);
      acc2[uu] = split::mfma32_x6(fh, fb2[i & 1], acc2[uu]);
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();  // the patch and this slice's buffer are free again
  }

  // ---- bias, row L2 norm (inside the wave), store ----
  float ss[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) ss[q] = 0.f;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const float bias2 = b2[32 * u + r];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      acc2[u][q] += bias2;
      ss[q] = fmaf(acc2[u][q], acc2[u][q], ss[q]);
    }
  }
  if (normalize) {
#pragma unroll
    for (int q = 0; q < 16; ++q) ss[q] = 1.f / (sqrtf(group_reduce<Op::Sum, 1, 16>(ss[q])) + 1e-8f);
  }
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int64_t row = row0 + row_of(q, hf);
    if (row >= B) continue;
#pragma unroll
    for (int u = 0; u < 4; ++u) out[row * DO + 32 * u + r] = normalize ? acc2[u][q] * ss[q] : acc2[u][q];
  }
}

// The fp16 two-term MLP before k_fusion_fwdh3 (described at HLDK in ppgat_fusion.hip): GEMM1 on
// k_gemm_nnh's loop, two LDS buffers, one __syncthreads per chunk.  The bitwise reference of
// tests/test_gpu_gemm_f16.py's fusion lab tests.
__global__ void __launch_bounds__(512, 1) k_fusion_fwdh(const float* __restrict__ txt, const float* __restrict__ img,
                                                        const int32_t* __restrict__ img_index,
                                                        const float* __restrict__ img_fallback, int64_t B, int Dt,
                                                        int Di, const uint16_t* __restrict__ w1i,
                                                        const int* __restrict__ e1, const float* __restrict__ b1,
                                                        const uint16_t* __restrict__ w2i_g, const int* __restrict__ e2,
                                                        const float* __restrict__ b2, int normalize,
                                                        float* __restrict__ out, float* __restrict__ z1_out) {
  static_assert(kH1Img * 2 % 1024 == 0 && kH2Img * 2 % 1024 == 0, "1-KB wave copies");
  static_assert(kPatchB + 2 * kH2Img * 2 <= 2 * kH1Img * 2, "GEMM2 fits GEMM1's LDS");
  __shared__ __attribute__((aligned(16))) uint16_t lds[2 * kH1Img];
  __shared__ __attribute__((aligned(16))) float sF[8][32];  // per wave: a factor per row
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, hf = lane >> 5;
  const int64_t row0 = (int64_t)blockIdx.x * PBM + 32 * w;
  const int K = Dt + Di, chunks = K / BK;
  const int64_t b = row0 + r < B ? row0 + r : B - 1;
  const float* trow = txt + b * Dt + 4 * hf;
  const float* irow;
  if (Di > 0) {
    const int32_t ii = img_index ? img_index[b] : (int32_t)b;
    irow = (ii >= 0 ? img + (int64_t)ii * Di : img_fallback) + 4 * hf;
  } else {
    irow = trow;
  }
  auto load_x = [&](int k0, float4 (&xv)[4]) {
    const float* src = k0 < Dt ? trow + k0 : irow + (k0 - Dt);
#pragma unroll
    for (int g = 0; g < 4; ++g) xv[g] = ld4(src + 8 * g);
  };

  // ---- GEMM1: rows scaled online, W1 columns by their pre-split scales ----
  f32x16 acc[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) acc[t] = f32x16{};
  float4 xa[4], xn[4];
  int erow = 0;
  bool set = false;
  load_x(0, xa);
  glds_copy(w1i, lds, kH1Img * 2, w, lane);
  __syncthreads();  // vmcnt(0): chunk 0 and the first x fragments have landed
  for (int c = 0; c < chunks; ++c) {
    const uint16_t* sb = lds + (c & 1) * kH1Img;
    const bool more = c + 1 < chunks;
    if (more) {
      glds_copy(w1i + (int64_t)(c + 1) * kH1Img, lds + ((c + 1) & 1) * kH1Img, kH1Img * 2, w, lane);
      load_x((c + 1) * BK, xn);
    }
    const float s = split::row_scale_online<8>(xa, erow, set, acc, sF[w], r, hf);
    auto read_w = [&](int idx, split::u32x4 (&f)[2]) {
      const int off = (32 * (idx & 7) + r) * HLDK + 16 * (idx >> 3) + 8 * hf;
#pragma unroll
      for (int p = 0; p < 2; ++p) f[p] = *reinterpret_cast<const split::u32x4*>(&sb[p * kH1Part + off]);
    };
    split::u32x4 fx[2], fb[2][2];
    read_w(0, fb[0]);
#pragma unroll
    for (int idx = 0; idx < 16; ++idx) {
      const int u = idx >> 3, t = idx & 7;
      if (t == 0) split::split2h(xa[2 * u], xa[2 * u + 1], s, fx[0], fx[1]);
      if (idx + 1 < 16) read_w(idx + 1, fb[(idx + 1) & 1]);
      acc[t] = split::mfma32_h3(fx, fb[idx & 1], acc[t]);
      if (idx + 1 < 16) __builtin_amdgcn_sched_group_barrier(0x0100, 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x0008, 3, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();  // chunk c + 1 landed; every wave is done with this buffer
    if (more) {
#pragma unroll
      for (int g = 0; g < 4; ++g) xa[g] = xn[g];
    }
  }

  // ---- h = relu(z), z = acc / (s_row s_col) + b1 (exact unscale); h's row maxima ----
  float fr[16];
  split::row_unscale(erow, sF[w], r, hf, fr);
  float hm[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) hm[q] = 0.f;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const int col = BK * t + r;
    const float fc = ldexpf(1.f, -e1[col]), bias = b1[col];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const float z = fmaf(acc[t][q] * fr[q], fc, bias);
      const int row = row_of(q, hf);
      if (z1_out != nullptr && row0 + row < B) z1_out[(row0 + row) * H1 + col] = z;
      const float h = fmaxf(z, 0.f);
      acc[t][q] = h;
      hm[q] = fmaxf(hm[q], h);
    }
  }
  float fr2[16];  // 1 / s_h of this lane's accumulator rows (GEMM2 epilogue)
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const float m = group_reduce<Op::Max, 1, 16>(hm[q]);
    const int e = (m > 0.f && m <= 3.4e38f) ? split::scale_exp16(m) : 0;
    fr2[q] = ldexpf(1.f, -e);
    if (r == q) sF[w][row_of(q, hf)] = ldexpf(1.f, e);  // s_h for the A-operand lanes
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const float sh = sF[w][r];  // this lane's GEMM2 A-operand row is row r

  // ---- GEMM2 over eight 32-column slices of h ----
  float* hp = reinterpret_cast<float*>(lds) + w * 32 * XLH;   // this wave's patch [32][XLH]
  uint16_t* w2s = lds + kPatchB / 2;                           // [2][kH2Img]
  f32x16 acc2[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) acc2[u] = f32x16{};
  glds_copy(w2i_g, w2s, kH2Img * 2, w, lane);
#pragma unroll
  for (int c = 0; c < H1 / BK; ++c) {
#pragma unroll
    for (int q = 0; q < 16; ++q) hp[row_of(q, hf) * XLH + r] = acc[c][q];
    __syncthreads();  // vmcnt(0): slice c landed; the patch is written
    if (c + 1 < H1 / BK) glds_copy(w2i_g + (int64_t)(c + 1) * kH2Img, w2s + ((c + 1) & 1) * kH2Img, kH2Img * 2, w, lane);
    const uint16_t* ws2 = w2s + (c & 1) * kH2Img;
    auto read_w2 = [&](int i, split::u32x4 (&f)[2]) {
      const int off = (32 * (i & 3) + r) * HLDK + 16 * (i >> 2) + 8 * hf;
#pragma unroll
      for (int p = 0; p < 2; ++p) f[p] = *reinterpret_cast<const split::u32x4*>(&ws2[p * kH2Part + off]);
    };
    split::u32x4 fh[2], fb2[2][2];
    read_w2(0, fb2[0]);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int u = i >> 2, uu = i & 3;
      if (uu == 0) split::split2h(ld4(&hp[r * XLH + 16 * u + 4 * hf]), ld4(&hp[r * XLH + 16 * u + 8 + 4 * hf]), sh, fh[0], fh[1]);
      if (i + 1 < 8) read_w2(i + 1, fb2[(i + 1) & 1]);
      acc2[uu] = split::mfma32_h3(fh, fb2[i & 1], acc2[uu]);
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();  // the patch and this slice's buffer are free again
  }

  // ---- unscale, bias, row L2 norm (inside the wave), store ----
  float ss[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) ss[q] = 0.f;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int col = 32 * u + r;
    const float fc = ldexpf(1.f, -e2[col]), bias2 = b2[col];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      acc2[u][q] = fmaf(acc2[u][q] * fr2[q], fc, bias2);
      ss[q] = fmaf(acc2[u][q], acc2[u][q], ss[q]);
    }
  }
  if (normalize) {
#pragma unroll
    for (int q = 0; q < 16; ++q) ss[q] = 1.f / (sqrtf(group_reduce<Op::Sum, 1, 16>(ss[q])) + 1e-8f);
  }
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int64_t row = row0 + row_of(q, hf);
    if (row >= B) continue;
#pragma unroll
    for (int u = 0; u < 4; ++u) out[row * DO + 32 * u + r] = normalize ? acc2[u][q] * ss[q] : acc2[u][q];
  }
}

}  // namespace

namespace lab {

// The lab's share of fusion_fwd: true when a superseded kernel ran (*err holds its status), false
// when the product dispatch should go on.
inline bool fusion_fwd(const float* txt, const float* img, const int32_t* img_index, const float* img_fallback,
                       int64_t B, int Dt, int Di, const float* W1, const float* b1, const float* W2, const float* b2,
                       int normalize, float* out, float* z1_out, hipStream_t st, void* ws, hipError_t* err) {
  if (ws == nullptr || !gemm_split_enabled()) return false;
  const dim3 grid((unsigned)((B + PBM - 1) / PBM));
  uint16_t* w1i = static_cast<uint16_t*>(ws);
  if (f16_off()) {  // W1 / W2 pre-split once into bf16 images, then the glds-staged x6 kernel
    uint16_t* w2i = w1i + nnx_image_bytes(Dt + Di, H1, 8) / 2;
    hipError_t e = nnx_presplit(W1, Dt + Di, 1, Dt + Di, H1, 8, w1i, st);
    if (e == hipSuccess) e = nnx_presplit(W2, H1, 1, H1, DO, 4, w2i, st);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(k_fusion_fwdp, grid, dim3(512), 0, st, txt, img, img_index, img_fallback, B, Dt, Di, w1i, b1,
                         w2i, b2, normalize, out, z1_out);
      e = hipGetLastError();
    }
    *err = e;
    return true;
  }
  if (nnh_variant() >= 3 && ((Dt + Di) / BK) % 2 == 0) return false;  // k_fusion_fwdh3
  uint16_t* w2i = w1i + nnh_image_bytes(Dt + Di, H1, 8) / 2;
  int* e1 = reinterpret_cast<int*>(static_cast<char*>(ws) + fusion_h_bytes(Dt, Di));
  int* e2 = e1 + H1;
  hipError_t e = nnh_presplit(W1, Dt + Di, 1, Dt + Di, H1, 8, w1i, e1, st);
  if (e == hipSuccess) e = nnh_presplit(W2, H1, 1, H1, DO, 4, w2i, e2, st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_fusion_fwdh, grid, dim3(512), 0, st, txt, img, img_index, img_fallback, B, Dt, Di, w1i, e1,
                       b1, w2i, e2, b2, normalize, out, z1_out);
    e = hipGetLastError();
  }
  *err = e;
  return true;
}

}  // namespace lab
