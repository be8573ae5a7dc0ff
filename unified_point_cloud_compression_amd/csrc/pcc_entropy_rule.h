// Element rules that more than one kernel must evaluate to the SAME BITS: the Gaussian conditional's scale bound, table
// search and quantisation (k_gauss, pcc_entropy.hip) and the rANS payload cost of one symbol (k_rans_estimate,
// pcc_rans.hip).  pcc_rate.hip evaluates both per candidate gain row and promises the integer the two kernels give one
// after the other, so each expression exists once, here, and every user inlines it: the contraction of y*g - mean*g into a
// fused multiply-add and the approximate __log2f are then the same instructions in all of them.
#pragma once
#include "pcc_common.h"

static constexpr float SCALE_BOUND = 0.11f;

struct RansTab { const int* cdf; int stride; const int* sizes; const int* offsets; };

__device__ inline int table_index(float s, const float* __restrict__ tab, int nt) {
  // idx = (nt-1) - #{t < nt-1 : s <= tab[t]}   (GaussianConditional.build_indexes)
  int idx = nt - 1;
  for (int t = 0; t < nt - 1; ++t) idx -= (s <= tab[t]) ? 1 : 0;
  return idx;
}

__device__ inline float gauss_bound_scale(float scale, float g) { return fmaxf(scale * g, SCALE_BOUND); }

// rint(y*g - mean*g) with the contraction written out: mean*g rounded, y*g exact inside the fused multiply-add.  Left to
// the compiler the form is a choice per call site (this one in k_gauss; inside a loop over gain rows a packed multiply of
// both products and a subtraction), and the two differ where the difference sits next to a half-integer.
__device__ inline float gauss_quantise(float y, float mean, float g) {
  float m = mean * g;
  asm("" : "+v"(m));            // m is a value of its own: not paired with y*g, its sign not folded into the product
  return rintf(__builtin_fmaf(g, y, -m));
}

// Cost in 1/256 bit of the value v = symbol - offsets[ci] under the cdf row of table row ci, max_value = sizes[ci] - 2:
// round(256 * (16 - log2 freq)), plus the 4-bit bypass digits of a value outside the row's support (coded through the
// sentinel, the last value of the row).
__device__ inline unsigned rans_value_bits256(int v, int max_value, const int* row) {
  unsigned raw = 0;
  if (v < 0) { raw = (unsigned)(-2 * v - 1); v = max_value; }
  else if (v >= max_value) { raw = (unsigned)(2 * (v - max_value)); v = max_value; }
  const int freq = max(row[v + 1] - row[v], 1);
  unsigned b = (unsigned)__float2int_rn(256.f * (16.f - __log2f((float)freq)));
  if (v == max_value) b += 256u * 4u * (unsigned)((32 - __clz((int)(raw | 1u)) + 3) / 4 + 1);   // bypass digits, 4 bits each
  return b;
}
