// lab/ppgat_xform_lab.h -- the superseded generations of the pre-split NN GEMM, the switches that
// select them and the measured variants of k_gemm_nnh3, and their launch code.  Lab builds only
// (make lab, -DPPGAT_LAB_BUILD=1): ppgat_xform.hip includes this file once, inside namespace
// ppgat, after the product kernels and helpers it uses (NnArg, NnpImg, NnhImg, kPBM, kNnhRank,
// k_gemm_nnh3, dma_lds16, wait_vm ...).  Never part of libppgat.so.
//
//   PPGAT_GEMM_F16=0    k_nnx_presplit + k_gemm_nnp (bf16 x6), and no fp16 TN kernel
//   PPGAT_NNH2=0        k_gemm_nnh
//   PPGAT_NNH2=2        k_gemm_nnh2
//   PPGAT_NNH2=6        k_gemm_nnh3 with XT
//   PPGAT_NNH_E4=1      k_gemm_nnh3 with the E4 epilogue
//   PPGAT_NNH_OCC2=1    k_gemm_nnh3 on the 128-column tile with OCC = 4
//   PPGAT_TNH256=0      the 128 x 256 TN tile everywhere
//   odd chunk counts    k_gemm_nnh, under every variant
#pragma once

#include "ppgat_lab_switches.h"

namespace {

// ---------------------------------------------------------------------------
// NN GEMM on the split bf16 matrix cores, B pre-split once per call (the large-M shapes:
// config 5's [1.9M x 1024] x [1024 x 256] and [1.9M x 256] x [256 x 1024]).
//
// k_gemm_nnx splits its 32-deep B chunk while staging it (per workgroup, per chunk: ~1.8 VALU
// instructions per MFMA, PMC profiles/r03/v1_gemm_nnx_cfg5_pmc.json: MFMA busy 0.49) and
// stages it through registers with two barriers per chunk.  Here:
//  * k_nnx_presplit writes the three bf16 images of every (column block, k chunk) to the
//    workspace ONCE per call, in exactly the LDS layout k_gemm_nnx uses (80-B rows, the
//    permuted reduction order), so the products are the same -- bitwise equal results;
//  * k_gemm_nnp stages them with global_load_lds_dwordx4 (an image is a contiguous byte
//    range, so the lane-linear LDS destination is the image itself), two LDS buffers, one
//    barrier per chunk, 8 waves (256 rows) sharing every staged chunk.
// ---------------------------------------------------------------------------
template <int NT, int BMODE>
__global__ void __launch_bounds__(256) k_nnx_presplit(const float* __restrict__ B, int64_t ldb, int K, int N,
                                                      uint16_t* __restrict__ img) {
  using I = NnpImg<NT>;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)N * (K / 4)) return;
  const int ng = (int)(t % N), kq = (int)(t / N);
  const int k0 = 4 * kq, c = k0 / I::KC, q = (k0 % I::KC) / 4;
  const int nb = ng / I::BN, n = ng % I::BN;
  float v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = BMODE == 0 ? B[(int64_t)(k0 + j) * ldb + ng] : B[(int64_t)ng * ldb + k0 + j];
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
  const int kk = 16 * (q >> 2) + 8 * (q & 1) + 4 * ((q >> 1) & 1);
  uint16_t* base = img + ((int64_t)nb * (K / I::KC) + c) * I::ELEMS + n * I::LDK + kk;
  *reinterpret_cast<uint2*>(base) = h;
  *reinterpret_cast<uint2*>(base + I::PART) = mm;
  *reinterpret_cast<uint2*>(base + 2 * I::PART) = l;
}

template <int NT>
__global__ void __launch_bounds__(512, 1) k_gemm_nnp(NnArg a, const uint16_t* __restrict__ img) {
  using I = NnpImg<NT>;
  constexpr int KC = I::KC, LDK = I::LDK, PART = I::PART, NI = I::BYTES / 1024;
  __shared__ __attribute__((aligned(16))) uint16_t sB[2][I::ELEMS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, hf = lane >> 5;
  const int64_t b = blockIdx.x;
  const int64_t idx = b >> 3;
  const int64_t rb = (idx / a.n_blocks) * 8 + (b & 7);  // XCD-aware: a row block's column blocks share an L2
  const int nb = (int)(idx % a.n_blocks);
  if (rb >= a.row_blocks) return;
  const int64_t M = a.M;
  const int K = a.K, chunks = K / KC;
  const int64_t m = rb * kPBM + wv * 32 + r;
  const float* xrow = a.X + (m < M ? m : M - 1) * a.ldx + 4 * hf;  // rows past M re-read row M-1 (never stored)
  // buffer_load ... lds (MUBUF), not global_load_lds: the compiler counts a FLAT LDS-DMA as a
  // pending LDS access, and every LDS-read wait behind it became lgkmcnt(0) -- the ds_reads of
  // step i + 1 could not overlap step i's MFMAs.  A MUBUF LDS-DMA is tracked on vmcnt only.
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint16_t*>(img + (int64_t)nb * chunks * I::ELEMS), 0, chunks * I::BYTES, 0x00020000);
  auto issue = [&](int c, int buf) {  // chunk c's three images -> sB[buf], 1 KB per wave instruction
    const int src = c * I::BYTES + lane * 16;
    char* dst = reinterpret_cast<char*>(sB[buf]);
    for (int i = wv; i < NI; i += 8)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(dst + i * 1024), 16,
                                               src + i * 1024, 0, 0, 0);
  };
  float4 xa[4], xn[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) xa[g] = ld4(xrow + 8 * g);
  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x16{};
  issue(0, 0);
  __syncthreads();  // vmcnt(0): chunk 0 and the first x fragments have landed
  for (int c = 0; c < chunks; ++c) {
    const int buf = c & 1;
    const bool more = c + 1 < chunks;
    if (more) {
      issue(c + 1, buf ^ 1);  // the buffer every wave finished reading before the last barrier
#pragma unroll
      for (int g = 0; g < 4; ++g) xn[g] = ld4(xrow + (c + 1) * KC + 8 * g);
    }
    const uint16_t* sb = sB[buf];
    auto read_b = [&](int i, split::u32x4 (&f)[3]) {
      const int off = (32 * (i % NT) + r) * LDK + 16 * (i / NT) + 8 * hf;
#pragma unroll
      for (int p = 0; p < 3; ++p) f[p] = *reinterpret_cast<const split::u32x4*>(&sb[p * PART + off]);
    };
    // B fragments in two register sets used alternately (no copy between them, so the register
    // allocator cannot merge them): the reads of step i + 1 issue before the six MFMAs of step i
    // and have those ~190 cycles to land (with one merged set they were scheduled after the
    // step's fifth MFMA and the next step waited on the LDS latency)
    split::u32x4 fx[3], fb[2][3];
    read_b(0, fb[0]);
#pragma unroll
    for (int i = 0; i < (KC / 16) * NT; ++i) {
      const int u = i / NT, t = i % NT;
      if (t == 0) split::split3(xa[2 * u], xa[2 * u + 1], fx[0], fx[1], fx[2]);
      if (i + 1 < (KC / 16) * NT) read_b(i + 1, fb[(i + 1) & 1]);
      acc[t] = split::mfma32_x6(fx, fb[i & 1], acc[t]);
      // order inside the step: the next step's three LDS reads first, then the six MFMAs
      if (i + 1 < (KC / 16) * NT) __builtin_amdgcn_sched_group_barrier(0x0100, 3, 0);
      __builtin_amdgcn_sched_group_barrier(0x0008, 6, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();  // vmcnt(0): chunk c + 1 has landed; every wave is done with sB[buf]
    if (more) {
#pragma unroll
      for (int g = 0; g < 4; ++g) xa[g] = xn[g];
    }
  }
  const int64_t row0 = rb * kPBM + wv * 32;
  const int n0 = nb * I::BN;
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
// k_gemm_nnh: the first fp16 two-term kernel (the family is described at k_colscale16 in
// ppgat_xform.hip) -- two LDS buffers, one __syncthreads per chunk, any chunk count.  The bitwise
// reference of k_gemm_nnh2 and k_gemm_nnh3.
// ---------------------------------------------------------------------------
template <int NT, bool RK>
__global__ void __launch_bounds__(512, 1) k_gemm_nnh(NnArg a, const uint16_t* __restrict__ img,
                                                     const int* __restrict__ ecol) {
  using I = NnhImg<NT>;
  constexpr int KC = I::KC, LDK = I::LDK, PART = I::PART, NI = I::BYTES / 1024;
  __shared__ __attribute__((aligned(16))) uint16_t sB[2][I::ELEMS];
  __shared__ __attribute__((aligned(16))) float sF[8][32];  // per wave: a factor per row (rescale, epilogue)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, hf = lane >> 5;
  const int64_t b = blockIdx.x;
  const int64_t idx = b >> 3;
  const int64_t rb = (idx / a.n_blocks) * 8 + (b & 7);  // XCD-aware: a row block's column blocks share an L2
  const int nb = (int)(idx % a.n_blocks);
  if (rb >= a.row_blocks) return;
  const int64_t M = a.M;
  const int K = a.K, chunks = K / KC;
  const int64_t m = rb * kPBM + wv * 32 + r;
  const float* xrow = a.X + (m < M ? m : M - 1) * a.ldx + 4 * hf;  // rows past M re-read row M-1 (never stored)
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint16_t*>(img + (int64_t)nb * chunks * I::ELEMS), 0, chunks * I::BYTES, 0x00020000);
  auto issue = [&](int c, int buf) {  // chunk c's two images -> sB[buf], 1 KB per wave instruction
    const int src = c * I::BYTES + lane * 16;
    char* dst = reinterpret_cast<char*>(sB[buf]);
    for (int i = wv; i < NI; i += 8)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(dst + i * 1024), 16,
                                               src + i * 1024, 0, 0, 0);
  };
  float4 xa[4], xn[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) xa[g] = ld4(xrow + 8 * g);
  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x16{};
  int erow = 0;
  bool set = false;  // the row has had a nonzero element (its scale is fixed until an overflow)
  issue(0, 0);
  __syncthreads();  // vmcnt(0): chunk 0 and the first x fragments have landed
  for (int c = 0; c < chunks; ++c) {
    const int buf = c & 1;
    const bool more = c + 1 < chunks;
    if (more) {
      issue(c + 1, buf ^ 1);  // the buffer every wave finished reading before the last barrier
#pragma unroll
      for (int g = 0; g < 4; ++g) xn[g] = ld4(xrow + (c + 1) * KC + 8 * g);
    }
    const float s = split::row_scale_online<NT>(xa, erow, set, acc, sF[wv], r, hf);  // chunk c's row scales
    const uint16_t* sb = sB[buf];
    auto read_b = [&](int i, split::u32x4 (&f)[2]) {
      const int off = (32 * (i % NT) + r) * LDK + 16 * (i / NT) + 8 * hf;
#pragma unroll
      for (int p = 0; p < 2; ++p) f[p] = *reinterpret_cast<const split::u32x4*>(&sb[p * PART + off]);
    };
    // two fragment sets used alternately; each step issues the next step's two LDS reads before
    // its three MFMAs (see k_gemm_nnp)
    split::u32x4 fx[2], fb[2][2];
    read_b(0, fb[0]);
#pragma unroll
    for (int i = 0; i < (KC / 16) * NT; ++i) {
      const int u = i / NT, t = i % NT;
      if (t == 0) split::split2h(xa[2 * u], xa[2 * u + 1], s, fx[0], fx[1]);
      if (i + 1 < (KC / 16) * NT) read_b(i + 1, fb[(i + 1) & 1]);
      acc[t] = split::mfma32_h3(fx, fb[i & 1], acc[t]);
      if (i + 1 < (KC / 16) * NT) __builtin_amdgcn_sched_group_barrier(0x0100, 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x0008, 3, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();  // vmcnt(0): chunk c + 1 has landed; every wave is done with sB[buf]
    if (more) {
#pragma unroll
      for (int g = 0; g < 4; ++g) xa[g] = xn[g];
    }
  }
  float fr[16];  // unscale: 1 / (s_row s_col), both exact powers of two
  split::row_unscale(erow, sF[wv], r, hf, fr);
  const int64_t row0 = rb * kPBM + wv * 32;
  const int n0 = nb * I::BN;
  if constexpr (RK) {
    // + S A (nv <= kNnhRank): this lane's columns of A in registers, each row's S terms loaded
    // once (broadcast over the 32 lanes of the row), the terms added in v order after alpha, bias
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

// ---------------------------------------------------------------------------
// k_gemm_nnh2: k_gemm_nnh's arithmetic (the same products in the same order: bitwise equal
// results) with a deeper pipeline.  In k_gemm_nnh the compiler waits for the whole vector-memory
// queue twice per 32-deep chunk -- before the first LDS read after an LDS-DMA issue (it cannot
// tell the DMA target from the buffer being read) and at every __syncthreads (its workgroup
// fence) -- so the next chunk's X rows, streamed from HBM one chunk ahead, had only part of a
// chunk to arrive (MFMA busy 0.41, 46 % of the wave cycles waiting; profiles/r03/v27_nnh_pmc.json).
// Here:
//  * B chunks go to LDS by LDS-DMA issued in inline asm (the compiler sees no memory access, so
//    it adds no wait before LDS reads), three buffers, issued two chunks ahead;
//  * X rows stream two chunks ahead in two register sets; a chunk's rows are scaled and split
//    into their fp16 fragments at the top of the chunk, which frees the set for chunk c + 2;
//  * the chunk barrier is a bare s_barrier after an explicit vmcnt wait for exactly this
//    wave's DMA of chunk c + 1 (the only operation the barrier must cover: everything issued
//    after it -- X of c + 1, DMA and X of c + 2 -- stays in flight).
// Global issue order per wave: DMA(0) X(0) DMA(1) X(1) | chunk c: DMA(c+2) X(c+2) ...
// ---------------------------------------------------------------------------
template <int NT, bool RK>
__global__ void __launch_bounds__(512, 1) k_gemm_nnh2(NnArg a, const uint16_t* __restrict__ img,
                                                      const int* __restrict__ ecol) {
  using I = NnhImg<NT>;
  constexpr int KC = I::KC, LDK = I::LDK, PART = I::PART, NI = I::BYTES / 1024;
  __shared__ __attribute__((aligned(16))) uint16_t sB[3][I::ELEMS];
  __shared__ __attribute__((aligned(16))) float sF[8][32];  // per wave: a factor per row (rescale, epilogue)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, hf = lane >> 5;
  const int64_t b = blockIdx.x;
  const int64_t idx = b >> 3;
  const int64_t rb = (idx / a.n_blocks) * 8 + (b & 7);  // XCD-aware: a row block's column blocks share an L2
  const int nb = (int)(idx % a.n_blocks);
  if (rb >= a.row_blocks) return;
  const int64_t M = a.M;
  const int K = a.K, chunks = K / KC;
  const int64_t m = rb * kPBM + wv * 32 + r;
  const float* xrow = a.X + (m < M ? m : M - 1) * a.ldx + 4 * hf;  // rows past M re-read row M-1 (never stored)
  // buffer resource of this column block's images (stride 0, raw bytes), wave-uniform
  const uint64_t base = reinterpret_cast<uint64_t>(img + (int64_t)nb * chunks * I::ELEMS);
  const i32x4 rsrc = {__builtin_amdgcn_readfirstlane((int)(uint32_t)base),
                      __builtin_amdgcn_readfirstlane((int)((base >> 32) & 0xffff)),
                      __builtin_amdgcn_readfirstlane(chunks * I::BYTES), 0x00020000};
  const uint32_t lds0 = (uint32_t)reinterpret_cast<uintptr_t>(&sB[0][0]);
  const uint32_t voff = (uint32_t)lane * 16u;
  constexpr int ND = (NI + 7) / 8;  // DMA instructions of waves 0 .. (NI % 8) - 1 (one fewer for the rest)
  const bool full = (NI % 8 == 0) || wv < NI % 8;
  auto issue = [&](int c) {  // chunk c's two images -> sB[c % 3], 1 KB per wave instruction
    const uint32_t dst = lds0 + (uint32_t)((c % 3) * I::ELEMS * 2);
    for (int i = wv; i < NI; i += 8) dma_lds16(rsrc, dst + i * 1024, voff, (uint32_t)(c * I::BYTES + i * 1024));
  };
  auto loadx = [&](int c, float4 (&x)[4]) {
#pragma unroll
    for (int g = 0; g < 4; ++g) x[g] = ld4(xrow + c * KC + 8 * g);
  };
  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x16{};
  int erow = 0;
  bool set = false;  // the row has had a nonzero element (its scale is fixed until an overflow)
  // chunks is even (>= 2; the launcher checks): the loop below runs chunk pairs (xA, xB) and
  // every chunk loads an X set, the last two re-reading chunk chunks - 1, so the compiler sees
  // the same four loads per chunk on every path and waits for exactly the set it reads
  float4 xA[4], xB[4];
  issue(0);
  loadx(0, xA);
  issue(1);
  loadx(1, xB);
  if (full) wait_vm<4 + ND + 4>(); else wait_vm<4 + ND - 1 + 4>();  // DMA(0) has landed
  __builtin_amdgcn_s_barrier();

  auto body = [&](const int c, float4 (&xc)[4]) {
    // X(c): this chunk's row scales and fp16 fragments (both k steps), then the set is free
    const float s = split::row_scale_online<NT>(xc, erow, set, acc, sF[wv], r, hf);
    split::u32x4 fx[2][2];
    split::split2h(xc[0], xc[1], s, fx[0][0], fx[0][1]);
    split::split2h(xc[2], xc[3], s, fx[1][0], fx[1][1]);
    const bool ahead = c + 2 < chunks;
    if (ahead) issue(c + 2);
    loadx(ahead ? c + 2 : chunks - 1, xc);
    const uint16_t* sb = sB[c % 3];
    auto read_b = [&](int i, split::u32x4 (&f)[2]) {
      const int off = (32 * (i % NT) + r) * LDK + 16 * (i / NT) + 8 * hf;
#pragma unroll
      for (int p = 0; p < 2; ++p) f[p] = *reinterpret_cast<const split::u32x4*>(&sb[p * PART + off]);
    };
    split::u32x4 fb[2][2];
    read_b(0, fb[0]);
#pragma unroll
    for (int i = 0; i < (KC / 16) * NT; ++i) {
      const int u = i / NT, t = i % NT;
      if (i + 1 < (KC / 16) * NT) read_b(i + 1, fb[(i + 1) & 1]);
      acc[t] = split::mfma32_h3(fx[u], fb[i & 1], acc[t]);
      if (i + 1 < (KC / 16) * NT) __builtin_amdgcn_sched_group_barrier(0x0100, 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x0008, 3, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    // DMA(c + 1) must have landed before any wave reads it, and every wave must be done with
    // sB[c % 3] before chunk c + 3's DMA (issued in chunk c + 1) overwrites it.  Issued after
    // DMA(c + 1): X(c + 1), and in this chunk DMA(c + 2) (if any) and an X set.
    if (ahead) {
      if (full) wait_vm<4 + ND + 4>(); else wait_vm<4 + ND - 1 + 4>();
    } else {
      wait_vm<4 + 4>();
    }
    __builtin_amdgcn_s_barrier();
  };
  for (int c = 0; c < chunks; c += 2) {
    body(c, xA);
    body(c + 1, xB);
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

}  // namespace

// the three bf16 images of B [K x N] (bmode 0: B[k][n] = B[k ldb + n]; 1: B[n ldb + k]) per
// (column block of 32 nt columns, 32-deep k chunk), in the LDS layout the split kernels read
hipError_t nnx_presplit(const float* B, int64_t ldb, int bmode, int K, int N, int nt, uint16_t* img, hipStream_t st) {
  const int64_t groups = (int64_t)N * (K / 4);
  const unsigned gp = (unsigned)((groups + 255) / 256);
  if (groups <= 0) return hipSuccess;
  if (nt == 8) {
    if (bmode == 0) hipLaunchKernelGGL((k_nnx_presplit<8, 0>), dim3(gp), dim3(256), 0, st, B, ldb, K, N, img);
    else hipLaunchKernelGGL((k_nnx_presplit<8, 1>), dim3(gp), dim3(256), 0, st, B, ldb, K, N, img);
  } else {
    if (bmode == 0) hipLaunchKernelGGL((k_nnx_presplit<4, 0>), dim3(gp), dim3(256), 0, st, B, ldb, K, N, img);
    else hipLaunchKernelGGL((k_nnx_presplit<4, 1>), dim3(gp), dim3(256), 0, st, B, ldb, K, N, img);
  }
  return hipGetLastError();
}

namespace lab {

// nnp_ok: k_gemm_nnh and k_gemm_nnp take any chunk count, so the lab's pre-split path does too
inline bool odd_chunks_ok() { return true; }

// gemm_tn_big: PPGAT_TNH256=0, the 128 x 256 tile everywhere (A/B runs against the 256 x 256 one)
inline bool tnh256_off() {
  static const bool off = env_char("PPGAT_TNH256") == '0';
  return off;
}

inline bool env_is_1(const char* name) {
  const char* e = getenv(name);
  return e != nullptr && atoi(e) == 1;
}

// The lab's share of gemm_nn's pre-split branch (a, w8 and grid as gemm_nn set them up; ws holds
// the image): true when a lab kernel ran (*err holds its status), false when the product launch
// of k_gemm_nnh3 should go on.
inline bool gemm_nn_presplit(const NnArg& a, int bmode, bool w8, unsigned grid, void* ws, hipStream_t st,
                             hipError_t* err) {
  const int K = a.K, N = a.N, nv = a.nv;
  uint16_t* img = static_cast<uint16_t*>(ws);
  if (f16_off()) {  // bf16 x6
    hipError_t e = nnx_presplit(a.B, a.ldb, bmode, K, N, w8 ? 8 : 4, img, st);
    if (e == hipSuccess) {
      if (w8) hipLaunchKernelGGL((k_gemm_nnp<8>), dim3(grid), dim3(512), 0, st, a, img);
      else hipLaunchKernelGGL((k_gemm_nnp<4>), dim3(grid), dim3(512), 0, st, a, img);
      e = hipGetLastError();
    }
    *err = e;
    return true;
  }
  const int v = nnh_variant();
  const bool pairs = (K / kGBK) % 2 == 0;  // k_gemm_nnh2 and k_gemm_nnh3 run chunk pairs
  static const bool e4_on = env_is_1("PPGAT_NNH_E4");
  static const bool occ2_on = env_is_1("PPGAT_NNH_OCC2");  // two workgroups per CU on the 128-column tile (<= 128 VGPRs)
  const bool nnh3 = v >= 3 && pairs;
  const bool occ2 = nnh3 && occ2_on && nv == 0;
  const bool e4 = nnh3 && !occ2 && e4_on && nv == 0 && a.ldy % 4 == 0 && reinterpret_cast<uintptr_t>(a.Y) % 16 == 0;
  if (nnh3 && v != 6 && !occ2 && !e4) return false;  // the product's k_gemm_nnh3
  int* ecol = reinterpret_cast<int*>(reinterpret_cast<char*>(ws) + align_up(nnh_image_bytes(K, N, w8 ? 8 : 4)));
  hipError_t e = nnh_presplit(a.B, a.ldb, bmode, K, N, w8 ? 8 : 4, img, ecol, st);
  if (e == hipSuccess && occ2 && w8) {  // re-split B for the 128-column tile
    ecol = reinterpret_cast<int*>(reinterpret_cast<char*>(ws) + align_up(nnh_image_bytes(K, N, 4)));
    e = nnh_presplit(a.B, a.ldb, bmode, K, N, 4, img, ecol, st);
  }
  if (e != hipSuccess) {
    *err = e;
    return true;
  }
#define PPGAT_LAB_NN(KERNEL, ...)                                                                          \
  do {                                                                                                     \
    if (nv > 0) {                                                                                          \
      if (w8) hipLaunchKernelGGL((KERNEL<8, true, ##__VA_ARGS__>), dim3(grid), dim3(512), 0, st, a, img, ecol);  \
      else hipLaunchKernelGGL((KERNEL<4, true, ##__VA_ARGS__>), dim3(grid), dim3(512), 0, st, a, img, ecol);     \
    } else if (w8) {                                                                                       \
      hipLaunchKernelGGL((KERNEL<8, false, ##__VA_ARGS__>), dim3(grid), dim3(512), 0, st, a, img, ecol);         \
    } else {                                                                                               \
      hipLaunchKernelGGL((KERNEL<4, false, ##__VA_ARGS__>), dim3(grid), dim3(512), 0, st, a, img, ecol);         \
    }                                                                                                      \
  } while (0)
  if (occ2) {
    NnArg b2 = a;
    b2.n_blocks = N / 128;
    const unsigned g2 = (unsigned)((b2.row_blocks + 7) / 8 * 8 * b2.n_blocks);
    hipLaunchKernelGGL((k_gemm_nnh3<4, false, false, false, 4>), dim3(g2), dim3(512), 0, st, b2, img, ecol);
  } else if (e4) {
    if (w8) hipLaunchKernelGGL((k_gemm_nnh3<8, false, false, true>), dim3(grid), dim3(512), 0, st, a, img, ecol);
    else hipLaunchKernelGGL((k_gemm_nnh3<4, false, false, true>), dim3(grid), dim3(512), 0, st, a, img, ecol);
  } else if (nnh3) {
    PPGAT_LAB_NN(k_gemm_nnh3, true);  // v == 6: XT
  } else if (v == 2 && pairs) {
    PPGAT_LAB_NN(k_gemm_nnh2);
  } else {
    PPGAT_LAB_NN(k_gemm_nnh);
  }
#undef PPGAT_LAB_NN
  *err = hipGetLastError();
  return true;
}

}  // namespace lab
