// Building blocks the MFMA kernels share (the convolution sources and pcc_wgrad.hip): vector types, the exact bf16 / scaled
// fp16 operand splits, the term order of a split product, the XCD work id and the C-fragment row mapping.  Bit-identity between
// the kernel forms rests on the split and on the term order, so each is written once, here.  Every helper is forced inline and
// takes and returns vectors BY VALUE: passed by reference they cost registers and instructions in the larger kernels.
#pragma once
#include "pcc_common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2v __attribute__((ext_vector_type(2)));
typedef float f32x2v __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// BUF: feature rows and weight rows are fetched with buffer loads whose offset is out of range for an absent neighbour
// (reads 0, no memory access): no per-row branch, no zero fill, 32-bit address arithmetic and a fixed number of loads
// in flight, so the s_waitcnt distances the compiler derives are exact.  Needs feat and wp below 4 GB each.
static constexpr unsigned BUF_OOB = 0xFFFF0000u;
static constexpr long long BUF_MAX_BYTES = 0xFFFE0000ll;

// ---- XCD-aware work mapping --------------------------------------------------------------------
// Workgroups are dealt round-robin over the 8 XCDs (private L2 each).  Neighbouring tiles gather almost the same
// input rows, so XCD x is given a CONTIGUOUS range of work ids: its L2 then serves the re-reads that otherwise go
// to the fabric 8 times (measured with rocprofv3 FETCH_SIZE: 12-25x the compulsory bytes without this).  The
// column blocks of one row tile are adjacent ids (same gathered rows).  Speed only, never correctness.
__device__ __forceinline__ int xcd_work_id() {
  const int cpx = gridDim.x >> 3;                         // grid is a multiple of 8
  return (blockIdx.x & 7) * cpx + (blockIdx.x >> 3);
}

// Element e of a 32x32 MFMA accumulator held by a lane of half-wave `half` belongs to row (e & 3) + 8 (e >> 2) + 4 half of the
// fragment (its column is lane & 31); `base` is the fragment's first row in the tile.
__device__ __forceinline__ int cfrag_row(int base, int e, int half) { return base + (e & 3) + 8 * (e >> 2) + 4 * half; }

__device__ __forceinline__ f32x16 acc_zero() { return f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}; }

// ---- exact split of fp32 into three bf16 planes, x = h + m + l (pcc_conv_bf.hip, "split" path) ---------------
__host__ __device__ inline long long bf_plane_elems(long long fp32_elems) { return fp32_elems / 2 * 3; }   // floats holding 3 bf16 planes

__device__ __forceinline__ void bf_split2(float x0, float x1, unsigned& h, unsigned& m, unsigned& l) {
  const f32x2v v = {x0, x1};
  h = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2v));
  const f32x2v r1 = {x0 - __builtin_bit_cast(float, h << 16), x1 - __builtin_bit_cast(float, h & 0xFFFF0000u)};
  m = __builtin_bit_cast(unsigned, __builtin_convertvector(r1, bf16x2v));
  const f32x2v r2 = {r1.x - __builtin_bit_cast(float, m << 16), r1.y - __builtin_bit_cast(float, m & 0xFFFF0000u)};
  l = __builtin_bit_cast(unsigned, __builtin_convertvector(r2, bf16x2v));
}

// ---- staging of the split kernels: LDS images [row][13 x 16 B], the 12 units (plane, slot) of a row's 192-byte piece + padding --
// role of a thread for the 16-byte unit u of a [rows][12 units] piece: its row (-1 past the end) and its unit within the row
__device__ __forceinline__ void stage_role(int u, int rows, int& row, int& w) {
  row = u / 12; w = u - row * 12;
  if (u >= rows * 12) row = -1;
}
// unit q * 256 + tid of the weight piece at byte offset wbase (absent units read zeros)
__device__ __forceinline__ uint4 load_b_unit(__amdgpu_buffer_rsrc_t rsB, unsigned wbase, int row, int q, int tid) {
  const unsigned off = row >= 0 ? wbase + (unsigned)(q * 256 + tid) * 16u : BUF_OOB;
  return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsB, off, 0, 0));
}
// four consecutive fp32 channels split in registers and written to the 8-byte slots o, o + 8, o + 16 of the image's three planes
__device__ __forceinline__ void stage_split4(unsigned long long* As64, int o, float x0, float x1, float x2, float x3) {
  unsigned h0, m0, l0, h1, m1, l1;
  bf_split2(x0, x1, h0, m0, l0);
  bf_split2(x2, x3, h1, m1, l1);
  As64[o] = (unsigned long long)h0 | ((unsigned long long)h1 << 32);
  As64[o + 8] = (unsigned long long)m0 | ((unsigned long long)m1 << 32);
  As64[o + 16] = (unsigned long long)l0 | ((unsigned long long)l1 << 32);
}

// acc += a * b over the six cross terms of first and second order, smallest first (planes 0 = h, 1 = m, 2 = l).  Every
// kernel that multiplies split operands goes through this order: their results are bit-identical.
__device__ __forceinline__ f32x16 bf6_terms(bf16x8 a0, bf16x8 a1, bf16x8 a2, bf16x8 b0, bf16x8 b1, bf16x8 b2, f32x16 acc) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b0, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b2, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc, 0, 0, 0);
  return acc;
}

// acc += a * b over the three terms l*h, h*l, h*h of scaled fp16 pairs, small terms first (planes 0 = h, 1 = l)
__device__ __forceinline__ f32x16 h3_terms(f16x8 a0, f16x8 a1, f16x8 b0, f16x8 b1, f32x16 acc) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b0, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b1, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0, acc, 0, 0, 0);
  return acc;
}
