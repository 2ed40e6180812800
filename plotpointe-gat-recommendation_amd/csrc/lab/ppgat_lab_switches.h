// lab/ppgat_lab_switches.h -- the environment switches both lab headers read, and what one lab
// translation unit calls in the other.  Included inside namespace ppgat (through
// ppgat_xform_lab.h / ppgat_fusion_lab.h), lab builds only.  Each switch is read once per process.
#pragma once

namespace lab {

// the value of a one-character switch, 0 when it is unset or longer
inline char env_char(const char* name) {
  const char* e = getenv(name);
  return e && e[0] && !e[1] ? e[0] : 0;
}

// PPGAT_GEMM_F16=0: the pre-split paths on the bf16 x6 kernels (k_gemm_nnp, k_fusion_fwdp), and
// the fp32 TN kernel instead of the fp16 two-term ones
inline bool f16_off() {
  static const bool off = env_char("PPGAT_GEMM_F16") == '0';
  return off;
}

// PPGAT_NNH2: the fp16 two-term NN main loop -- 0: k_gemm_nnh (1), 2: k_gemm_nnh2 (2), 6:
// k_gemm_nnh3 with X through LDS (6); anything else the product's k_gemm_nnh3 (3).  All compute
// the same products in the same order (tests/test_gpu_gemm_f16.py pins them bitwise).
inline int nnh_variant() {
  static const char c = env_char("PPGAT_NNH2");
  return c == '0' ? 1 : c == '2' ? 2 : c == '6' ? 6 : 3;
}

}  // namespace lab

// the three bf16 images of B per (column block, 32-deep k chunk): ppgat_xform_lab.h
hipError_t nnx_presplit(const float* B, int64_t ldb, int bmode, int K, int N, int nt, uint16_t* img, hipStream_t st);
