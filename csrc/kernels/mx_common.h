// trtlab_amd — OCP MX block quantization rules shared by every producer
// of MX rows: the row quantizers (gemm_mx.hip) and the LayerNorm-fused
// quantizer (normalize.hip). The scaled-MFMA GEMMs consume either, so the
// two must agree bit for bit; they do because both call these functions.
#pragma once
#include <hip/hip_fp8.h>

#include "../common.h"

namespace trtlab {

// Shared exponent of one 32-element block: floor(log2 amax) - emax of the
// element format (e4m3: 8, e2m1: 2), clamped to the e8m0 range; 0 for an
// all-zero block. The stored scale byte is e + 127.
__device__ __forceinline__ int mx_block_exponent(float amax, int emax) {
  int e = (amax > 0.f) ? (int)floorf(log2f(amax)) - emax : 0;
  return e < -127 ? -127 : (e > 127 ? 127 : e);
}

// e2m1 code (sign bit 3) of an already scaled value: round to nearest on
// {0, .5, 1, 1.5, 2, 3, 4, 6}, saturating. Tie rule: an exact midpoint
// rounds AWAY from zero (0.25 -> 0.5, 5 -> 6). The host codec
// engine/mx.py::quantize_mxfp4 rounds midpoints toward zero instead; see
// NOTES.md before changing either.
__device__ __forceinline__ unsigned char mx_encode_e2m1(float q) {
  float a = fabsf(q);
  int m;
  if (a < 0.25f) m = 0;
  else if (a < 0.75f) m = 1;
  else if (a < 1.25f) m = 2;
  else if (a < 1.75f) m = 3;
  else if (a < 2.5f) m = 4;
  else if (a < 3.5f) m = 5;
  else if (a < 5.0f) m = 6;
  else m = 7;
  return (unsigned char)(q < 0.f ? (m | 8) : m);
}

// e4m3 byte of an already scaled value: saturate to +-448, round to
// nearest even.
__device__ __forceinline__ unsigned char mx_encode_e4m3(float q) {
  return __hip_fp8_e4m3(fminf(fmaxf(q, -448.f), 448.f)).__x;
}

}  // namespace trtlab
