// Sparse convolution forward for gfx950: output-stationary implicit GEMM on the fp32 MFMA
// (v_mfma_f32_32x32x2_f32), deterministic (no atomics, fixed summation order).
//
// A workgroup owns BM consecutive positions of one map segment and BN output channels.  The
// reduction dimension is the flattened (active kernel offset, input channel) axis, consumed in
// chunks of 32: the BM gathered feature-row pieces and the BN weight rows of a chunk are staged
// through LDS as [row][32+4] tiles (16-byte pad: conflict-free ds_read_b128 / ds_write_b128), and
// every wave multiplies its 32x32 tiles with 4 MFMAs per pair of 16-byte fragment reads.
// Kernel offsets for which no position of the tile has a neighbour are skipped (wave ballots over
// the neighbour table), so sparse tiles do not pay for empty offsets.
//
// The same kernel body computes the fused GDN / IGDN (model/blocks.py:38-57): A = |x|, W = gamma^T,
// epilogue x / (acc + beta) or x * (acc + beta).
//
// This file is the dispatcher and what it owns: operand splitting and the library scratch, weight packing, the profiling state, the
// env switches, launch_mfma / launch_pair_product, GDN, the 4-channel input layer, pcc_conv_fwd and the pair-list planner.  Every
// variable of the family is defined here, once.  The kernel families are in files of their own (pcc_conv_f32.hip, pcc_conv_bf.hip,
// pcc_conv_dense.hip, pcc_conv_thin.hip, pcc_convt.hip); pcc_conv.h holds what they share.
#include <vector>

#include "pcc_conv.h"

// k_conv_mfma<WM, WN, TM, TN, MODE, BUF>, the kernel described at the top: pcc_conv_f32.hip

// ------------------------------------------------------------------------------------------
// The same implicit GEMM on the bf16 matrix pipe at fp32 accuracy ("split" path, cin a multiple of 32).
//
// gfx950 runs fp32-input MFMAs at the vector rate (157 TFLOP/s) and bf16-input MFMAs 16 times faster.  Every fp32
// operand is split EXACTLY into three bf16 values, x = h + m + l (h = rne_bf16(x), m = rne_bf16(x - h),
// l = x - h - m: 8 + 8 + 8 mantissa bits and a sign each, both subtractions exact), and a product is evaluated as the
// six cross terms of first and second order,
//     x*w ~= l*h' + h*l' + m*m' + m*h' + h*m' + h*h'        (dropped: m*l' + l*m' + l*l' <= 2^-23 |x*w|)
// each an exact bf16 x bf16 product accumulated in fp32 by v_mfma_f32_32x32x16_bf16 -- the same fp32 accumulation the
// fp32 MFMA performs.  Six bf16 MFMAs of K = 16 replace eight fp32 MFMAs of K = 2 at a quarter of the cycles each
// (MI355X_MICROARCH.md: 32 against 64 cycles per SIMD): 2.67x the matrix throughput, error at the level of fp32
// rounding (tests/test_gpu_map_conv.py::test_split_path_accuracy compares both paths with a float64 evaluation).
// Weights are split once when packed (three bf16 planes behind the fp32 image); the feature rows of a convolution's
// input are split by one pass of k_feat_split into planes [row][cin/32][3][32] (library scratch), so the MFMA kernel
// stages pure 16-byte copies.  (First version: split while staging, 5.5 VALU operations per element -- SQ counters
// showed 5.4 VALU instructions per MFMA and the SIMD issue-bound at 33 % MFMA utilisation; and for the shallow
// generative GEMMs every column block repeated the split of the same rows.)
// ------------------------------------------------------------------------------------------
// fp32 packed image [rows][32] -> bf16 planes [rows][3][32]
__global__ void k_split_packed(const float* __restrict__ src, long long pairs, unsigned* __restrict__ dst) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;      // one pair of consecutive channels
  if (t >= pairs) return;
  const long long row = t >> 4;
  const int cp = (int)(t & 15);
  unsigned h, m, l;
  bf_split2(src[2 * t], src[2 * t + 1], h, m, l);
  unsigned* d = dst + row * 48 + cp;
  d[0] = h; d[16] = m; d[32] = l;
}

// feature rows fp32 [n][c] -> bf16 planes [n][c/32][3][32] (of |x| for the GDN modes: the split is odd, so the planes of
// -x are the negated planes of x).  One pass per convolution input, so that the MFMA kernel stages pure copies.
__global__ void k_feat_split(const float* __restrict__ x, long long pairs, int cpairs, int take_abs, unsigned* __restrict__ dst) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;      // one pair of consecutive channels
  if (t >= pairs) return;
  const long long row = t / cpairs;
  const int cp = (int)(t - row * cpairs);
  float2 v = reinterpret_cast<const float2*>(x)[t];
  if (take_abs) { v.x = fabsf(v.x); v.y = fabsf(v.y); }
  unsigned h, m, l;
  bf_split2(v.x, v.y, h, m, l);
  unsigned* d = dst + (row * (cpairs >> 4) + (cp >> 4)) * 48 + (cp & 15);
  d[0] = h; d[16] = m; d[32] = l;
}

// ---- scaled fp16 pairs (dense products of the generative transposed convolutions) ----------------------------------
// T = X W with every fp32 operand written as s^-1 (h + l): s a power of two that brings the row's (X) or column's (W)
// largest magnitude into [2^14, 2^15), h = fp16(s x), l = fp16(s x - h).  h + l carries >= 22 significant bits of every
// element within 2^-18 of its row / column maximum (smaller ones lose bits they could not contribute to an fp32 sum anyway),
// and the three products l*h, h*l, h*h (fp32 accumulate, v_mfma_f32_32x32x16_f16) leave out only l*l < 2^-22 of a term: the
// error stays at the level of the fp32 accumulation itself (tests/test_gpu_map_conv.py::test_dense_products_accuracy), at
// HALF the matrix instructions of the six-term bf16 form and 2/3 of its operand bytes.  Row scales factor out of a dense
// product (one input row per output row) but not out of a gathered convolution, which is why only the dense products take
// this form.  The kernels are bound by energy, not by issue slots: the chip holds ~1.3 GHz on them (GRBM_GUI_ACTIVE / 8 /
// wall), and every phase's cost adds up whether or not it overlaps, so fewer MFMAs is what pays.
__device__ __forceinline__ float pow2_scale_exp(float mx, int& e) {      // s = 2^(14 - e), e = floor(log2 mx) (0 for mx = 0)
  e = mx > 0.f ? ilogbf(mx) : 0;
  e = e < -100 ? -100 : (e > 120 ? 120 : e);
  return ldexpf(1.f, 14 - e);
}
__device__ __forceinline__ void h_split4(const float4 v, float s, f16x4& h, f16x4& l) {
  const float x[4] = {v.x * s, v.y * s, v.z * s, v.w * s};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    h[i] = (_Float16)x[i];
    l[i] = (_Float16)(x[i] - (float)h[i]);
  }
}

// fp32 packed GEMM image [piece][cout_pad][32] -> fp16 planes [piece][cout_pad][2][32] scaled per column, and 1/scale per column
// (blockIdx.y: kernel offset of a convolution pack [K*ppo][cout_pad][32]; 0 for the flat operand of a dense product)
__global__ void k_split_packed_h(const float* __restrict__ src, int ppo, int cout_pad, unsigned char* __restrict__ dst,
                                 float* __restrict__ cinv) {
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= cout_pad) return;
  src += (size_t)blockIdx.y * ppo * cout_pad * 32;
  dst += (size_t)blockIdx.y * ppo * cout_pad * 128;
  cinv += (size_t)blockIdx.y * cout_pad;
  float mx = 0.f;
  for (int pc = 0; pc < ppo; ++pc) {
    const float4* r = reinterpret_cast<const float4*>(src + ((size_t)pc * cout_pad + col) * 32);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const float4 v = r[q];
      mx = fmaxf(mx, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    }
  }
  int e;
  const float sc = pow2_scale_exp(mx, e);
  for (int pc = 0; pc < ppo; ++pc) {
    const float4* r = reinterpret_cast<const float4*>(src + ((size_t)pc * cout_pad + col) * 32);
    unsigned char* d = dst + ((size_t)pc * cout_pad + col) * 128;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      f16x4 h, l;
      h_split4(r[q], sc, h, l);
      *reinterpret_cast<f16x4*>(d + q * 8) = h;
      *reinterpret_cast<f16x4*>(d + 64 + q * 8) = l;
    }
  }
  cinv[col] = ldexpf(1.f, e - 14);
}

// feature rows fp32 [n][c] -> fp16 planes [n][c/32][2][32] scaled per row, and 1/scale per row.  G = 2^g_log2 lanes per row.
__global__ void __launch_bounds__(256) k_feat_split_h(const float* __restrict__ x, long long n, int cin, int g_log2,
                                                      unsigned char* __restrict__ dst, float* __restrict__ rinv) {
  const int lane = threadIdx.x & 63;
  const int G = 1 << g_log2, lg = lane & (G - 1);
  const long long row = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * (64 >> g_log2) + (lane >> g_log2);
  const bool live = row < n;
  const int c4 = cin >> 2;
  const float4* xr = reinterpret_cast<const float4*>(x) + (live ? row : 0) * c4;
  float4 v[2];
  float mx = 0.f;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int q = lg + it * G;
    v[it] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live && q < c4) v[it] = xr[q];
    mx = fmaxf(mx, fmaxf(fmaxf(fabsf(v[it].x), fabsf(v[it].y)), fmaxf(fabsf(v[it].z), fabsf(v[it].w))));
  }
  for (int d = G >> 1; d >= 1; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d, 64));
  int e;
  const float sc = pow2_scale_exp(mx, e);
  if (!live) return;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int q = lg + it * G;
    if (q >= c4) continue;
    f16x4 h, l;
    h_split4(v[it], sc, h, l);
    unsigned char* d = dst + ((size_t)row * (cin >> 5) + (q >> 3)) * 128 + (q & 7) * 8;
    *reinterpret_cast<f16x4*>(d) = h;
    *reinterpret_cast<f16x4*>(d + 64) = l;
  }
  if (lg == 0) rinv[row] = ldexpf(1.f, e - 14);
}

// Grow-only device scratch of the library (per device; stream-ordered reuse on the caller's stream): the bf16 planes of
// the current convolution's input.  The only memory libpcc_hip owns.
static void* g_scratch[64];
static size_t g_scratch_bytes[64];
int lib_scratch(size_t bytes, void** out) {
  int dev = 0;
  PCC_CHECK_HIP(hipGetDevice(&dev));
  dev &= 63;
  if (g_scratch_bytes[dev] < bytes) {
    if (g_scratch[dev]) { PCC_CHECK_HIP(hipDeviceSynchronize()); PCC_CHECK_HIP(hipFree(g_scratch[dev])); g_scratch[dev] = nullptr; g_scratch_bytes[dev] = 0; }
    const size_t want = bytes + bytes / 4 + (1 << 20);
    PCC_CHECK_HIP(hipMalloc(&g_scratch[dev], want));
    g_scratch_bytes[dev] = want;
  }
  *out = g_scratch[dev];
  return PCC_OK;
}
// a second, small grow-only scratch (tables that live beside the planes of the same call)
static void* g_scratch_small[64];
static size_t g_scratch_small_bytes[64];
int lib_scratch_small(size_t bytes, void** out) {
  int dev = 0;
  PCC_CHECK_HIP(hipGetDevice(&dev));
  dev &= 63;
  if (g_scratch_small_bytes[dev] < bytes) {
    if (g_scratch_small[dev]) { PCC_CHECK_HIP(hipDeviceSynchronize()); PCC_CHECK_HIP(hipFree(g_scratch_small[dev])); g_scratch_small[dev] = nullptr; g_scratch_small_bytes[dev] = 0; }
    const size_t want = bytes < (1u << 20) ? (1u << 20) : bytes;
    PCC_CHECK_HIP(hipMalloc(&g_scratch_small[dev], want));
    g_scratch_small_bytes[dev] = want;
  }
  *out = g_scratch_small[dev];
  return PCC_OK;
}
static int make_planes(ConvArgs& a, bool take_abs, hipStream_t s) {
  void* p = nullptr;
  PCC_TRY(lib_scratch((size_t)a.n_in * a.cin * 6, &p));
  const long long pairs = (long long)a.n_in * a.cin / 2;
  k_feat_split<<<(unsigned)pcc_cdiv(pairs, 256), 256, 0, s>>>(a.feat, pairs, a.cin / 2, take_abs ? 1 : 0, (unsigned*)p);
  PCC_LAUNCH_CHECK();
  a.featb = (const unsigned char*)p;
  return PCC_OK;
}

// Range guard of the fp16-pair products: a device word (the entry point's d_guard) the kernels OR 1 into when a tile's scales
// admit an absolute product error above PCC_H_GUARD_BUDGET (cin * 2^-27 * max|row| * max|column| > budget); NULL = no guard.
// The caller zeroes the word, reads it back with a size it reads anyway, and repeats the operation with PCC_ARITH_BF6 when it is
// set.  The form and the guard word are ARGUMENTS of every call: the library keeps no arithmetic state (round 4; the process-wide
// pcc_set_gemm_h / pcc_set_mfma_split / pcc_set_h_guard switches of rounds 2-3 are gone).
int set_arith(ConvArgs& a, int arith, int32_t* d_guard, const char* who) {
  if (arith < PCC_ARITH_F32 || arith > PCC_ARITH_H3) { pcc_set_error("%s: arith=%d is not a PCC_ARITH_* form", who, arith); return PCC_EINVAL; }
  a.arith = arith;
  a.guard = arith == PCC_ARITH_H3 ? d_guard : nullptr;
  a.guard_lim = PCC_H_GUARD_BUDGET;              // compared with cin * 2^-27 * (rinv * 2^15) * (cinv * 2^15) = rinv * cinv * 8 * cin
  return PCC_OK;
}

static int make_planes_h(ConvArgs& a, hipStream_t s) {
  PCC_REQUIRE(a.cin % 32 == 0 && a.cin <= 512, "dense products: cin=%d (needs a multiple of 32 up to 512)", a.cin);
  void* p = nullptr;
  const size_t plane_bytes = pcc_align_up((size_t)a.n_in * a.cin * 4);
  PCC_TRY(lib_scratch(plane_bytes + pcc_align_up((size_t)a.n_in * 4), &p));
  int g = 0;
  while ((1 << g) < a.cin / 4 && g < 6) ++g;
  const long long rows_per_block = 4ll * (64 >> g);
  k_feat_split_h<<<(unsigned)pcc_cdiv(a.n_in, rows_per_block), 256, 0, s>>>(a.feat, a.n_in, a.cin, g, (unsigned char*)p,
                                                                         (float*)((char*)p + plane_bytes));
  PCC_LAUNCH_CHECK();
  a.feath = (const unsigned char*)p;
  a.frow_inv = (const float*)((char*)p + plane_bytes);
  return PCC_OK;
}

// k_conv_mfma_bf<WM, WN, TM, TN, MODE>, the same implicit GEMM on the planes: pcc_conv_bf.hip

// dense_tile, k_gemm_bf2, k_gemm_h2, k_pair_h2, the stripped GEMMs of the dense and pair products: pcc_conv_dense.hip

// GDN / IGDN with the split folded into the staging (round 3): out = x / (beta + |x| gamma^T)  (or x * (...)).  The general
// kernel above reads bf16 planes that a k_feat_split pass wrote first -- for this K = C, one-row-per-row product that pass and
// the planes' round trip are more HBM traffic than the operation itself (205 k x 128 rows: 50 us split + 170 us product for
// 205 MB of algorithmic traffic).  Here a thread loads the fp32 rows, takes |x| and splits in registers (the same bf_split2,
// so planes, term order and chunk order are those of k_conv_mfma_bf: bit-identical results) and writes the LDS image itself.
// TM = 2: 128-row tiles, TM = 1: 64-row tiles (more workgroups for the mid-sized sets).
template <int TM, int MODE>
__global__ void __launch_bounds__(256, 3) k_gdn_bf(ConvArgs a) {
  static_assert(MODE == MODE_GDN || MODE == MODE_IGDN, "GDN modes only");
  constexpr int WM = 2, WN = 2, TN = 2;
  constexpr int BM = WM * TM * 32, BN = WN * TN * 32, LDU = 13;
  __shared__ __attribute__((aligned(16))) uint4 As[BM * LDU];
  __shared__ __attribute__((aligned(16))) uint4 Bs[BN * LDU];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wid = xcd_work_id();
  const int gy = a.cout_pad / BN;
  const int tile_id = wid / gy;
  const int colblock = (wid - tile_id * gy) * BN;
  const long long p0 = (long long)tile_id * BM;
  if (p0 >= a.n_out) return;
  const int pos0 = (int)p0;
  const int npos = (int)min((long long)BM, a.n_out - p0);
  const int nchunks = a.ppo;                                          // 32 channels per chunk

  constexpr int NX = BM * 8 / 256, NB = (BN * 12 + 255) / 256;      // float4 of x / 16-byte weight units per thread and chunk
  int x_row[NX], x_j[NX], b_row[NB], b_w[NB];
#pragma unroll
  for (int q = 0; q < NX; ++q) { const int u = q * 256 + tid; x_row[q] = u >> 3; x_j[q] = u & 7; }
#pragma unroll
  for (int q = 0; q < NB; ++q) stage_role(q * 256 + tid, BN, b_row[q], b_w[q]);

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = acc_zero();
  const int wm = w / WN, wn = w % WN;
  const int half = lane >> 5, r31 = lane & 31;

  const float* wb = a.wp + a.wp_elems;                                // bf16 planes behind the fp32 image
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(wb), (short)0, (int)(unsigned)((size_t)bf_plane_elems(a.wp_elems) * 4), 0x00020000);
  const float* const xt = a.feat + (size_t)pos0 * a.cin;

  float4 xv[NX];
  uint4 bv[NB];
  auto issue = [&](int cbi) {
#pragma unroll
    for (int q = 0; q < NX; ++q) {
      const int rc = min(x_row[q], npos - 1);                         // tail rows repeat the tile's last row (never stored)
      xv[q] = *reinterpret_cast<const float4*>(xt + (size_t)rc * a.cin + cbi * 32 + x_j[q] * 4);
    }
    const unsigned wbase = (unsigned)(cbi * a.cout_pad + colblock) * 192u;
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      const unsigned off = b_row[q] >= 0 ? wbase + (unsigned)(q * 256 + tid) * 16u : BUF_OOB;     // load_b_unit (pcc_mfma.h) written out: the helper reorders this kernel
      bv[q] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsB, off, 0, 0));
    }
  };
  issue(0);
  unsigned long long* const As64 = reinterpret_cast<unsigned long long*>(As);
  for (int c = 0; c < nchunks; ++c) {
    __syncthreads();   // previous chunk's fragment reads are done
#pragma unroll
    for (int q = 0; q < NX; ++q) {
      const int o = x_row[q] * (LDU * 2) + x_j[q];                    // 8-byte slots: plane p of the row starts at slot 8 p
      stage_split4(As64, o, fabsf(xv[q].x), fabsf(xv[q].y), fabsf(xv[q].z), fabsf(xv[q].w));
    }
#pragma unroll
    for (int q = 0; q < NB; ++q)
      if (b_row[q] >= 0) Bs[b_row[q] * LDU + b_w[q]] = bv[q];
    __syncthreads();
    if (c + 1 < nchunks) issue(c + 1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 af[3][TM], bf[3][TN];
#pragma unroll
      for (int p = 0; p < 3; ++p) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
          af[p][i] = __builtin_bit_cast(bf16x8, As[((wm * TM + i) * 32 + r31) * LDU + p * 4 + ks * 2 + half]);
#pragma unroll
        for (int j = 0; j < TN; ++j)
          bf[p][j] = __builtin_bit_cast(bf16x8, Bs[((wn * TN + j) * 32 + r31) * LDU + p * 4 + ks * 2 + half]);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {           // smallest terms first (the order of k_conv_mfma_bf)
          // bf6_terms (pcc_mfma.h) written out: through the helper the TM = 1 kernels schedule differently
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[2][i], bf[0][j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0][i], bf[2][j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[1][i], bf[1][j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[1][i], bf[0][j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0][i], bf[1][j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0][i], bf[0][j], acc[i][j], 0, 0, 0);
        }
    }
  }
  // ---- epilogue: out = x / (beta + acc)  or  x * (beta + acc) --------------------------------------------------------
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = colblock + (wn * TN + j) * 32 + r31;
    if (col >= a.cout) continue;
    const float b = a.bias ? a.bias[col] : 0.f;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int r = cfrag_row((wm * TM + i) * 32, e, half);
        if (r >= npos) continue;
        const size_t o = (size_t)(pos0 + r) * a.cout + col;
        const float v = acc[i][j][e] + b;
        const float x = a.feat[o];
        a.out[o] = (MODE == MODE_GDN) ? x / v : x * v;
      }
  }
}

// The input layer (4 -> 128 channels, 5x5x5, stride 2: `g_a.down_conv_1[0]`) with its (offset, channel) pairs flattened into
// ONE reduction axis of K * 4 <= 512 (round 3).  The general kernel walks the 125 offsets one at a time -- a 4-deep reduction per
// staging round, 125 rounds of gather -> LDS -> barrier -> MFMA per tile: 2.8 us per round of pure latency, 22 TFLOP/s.  Here a
// chunk is 8 offsets x 4 channels = the 32-wide piece the split kernels work on: a thread gathers the 16-byte feature rows of
// (output row, offset) pairs through the map, splits them into bf16 planes in registers (as k_gdn_bf does) and writes the LDS
// image; 16 rounds instead of 125, six bf16 MFMA terms per product.  Absent neighbours are out-of-range buffer loads (zeros).
// Weights: planes [16 pieces][cout_pad][3][32] bf16 of the flattened kernel, converted from the packed fp32 image per call
// (k_in4_weight_planes, 0.4 MB).  Map indices are fetched two chunks ahead, rows one chunk ahead.
__global__ void __launch_bounds__(256) k_in4_weight_planes(const float* __restrict__ wp /*[K][cout_pad][4]*/, int K, int cout_pad,
                                                           unsigned* __restrict__ planes /*[16][cout_pad][48 dwords]*/) {
  const int t = blockIdx.x * 256 + threadIdx.x;                       // one pair of consecutive flat indices of one column
  if (t >= 16 * cout_pad * 16) return;
  const int cp = t & 15, col = (t >> 4) % cout_pad, piece = t / (16 * cout_pad);
  const int f0 = piece * 32 + 2 * cp;                                 // flat index = 4 * offset + channel
  const int k = f0 >> 2, c = f0 & 3;                                  // (f0 even: both elements of the pair belong to offset k)
  float v0 = 0.f, v1 = 0.f;
  if (k < K) { const float* w = wp + ((size_t)k * cout_pad + col) * 4 + c; v0 = w[0]; v1 = w[1]; }
  unsigned h, m, l;
  bf_split2(v0, v1, h, m, l);
  unsigned* d = planes + ((size_t)piece * cout_pad + col) * 48 + cp;
  d[0] = h; d[16] = m; d[32] = l;
}

template <int TM>
__global__ void __launch_bounds__(256, 3) k_conv_in4_bf(ConvArgs a, const unsigned* __restrict__ wplanes, int K) {
  constexpr int WM = 2, WN = 2, TN = 2;
  constexpr int BM = WM * TM * 32, BN = WN * TN * 32, LDU = 13, NCHUNK = 16;
  __shared__ __attribute__((aligned(16))) uint4 As[BM * LDU];
  __shared__ __attribute__((aligned(16))) uint4 Bs[BN * LDU];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wid = xcd_work_id();
  const int gy = a.cout_pad / BN;
  const int tile_id = wid / gy;
  const int colblock = (wid - tile_id * gy) * BN;
  const long long p0 = (long long)tile_id * BM;
  if (p0 >= a.n_out) return;
  const int pos0 = (int)p0;
  const int npos = (int)min((long long)BM, a.n_out - p0);
  const int nchunks = (K * 4 + 31) / 32;                              // <= NCHUNK

  constexpr int NX = BM * 8 / 256, NB = (BN * 12 + 255) / 256;
  int x_row[NX], x_j[NX], b_row[NB], b_w[NB];
#pragma unroll
  for (int q = 0; q < NX; ++q) { const int u = q * 256 + tid; x_row[q] = u >> 3; x_j[q] = u & 7; }
#pragma unroll
  for (int q = 0; q < NB; ++q) stage_role(q * 256 + tid, BN, b_row[q], b_w[q]);

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = acc_zero();
  const int wm = w / WN, wn = w % WN;
  const int half = lane >> 5, r31 = lane & 31;

  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned*>(wplanes), (short)0, (int)(unsigned)((size_t)NCHUNK * a.cout_pad * 192u), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.feat), (short)0, (int)(unsigned)((size_t)a.n_in * 16u), 0x00020000);
  const int* const nb0 = a.nbr + pos0;

  int id[NX];
  uint4 xv[NX], bv[NB];
  auto load_idx = [&](int c) {
#pragma unroll
    for (int q = 0; q < NX; ++q) {
      const int k = c * 8 + x_j[q];
      id[q] = (k < K && x_row[q] < npos) ? nb0[(long long)k * a.n_out + x_row[q]] : -1;
    }
  };
  auto issue = [&](int c) {                                           // rows of chunk c (indices already in id[]) + its weights
#pragma unroll
    for (int q = 0; q < NX; ++q)
      xv[q] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsX, id[q] >= 0 ? (unsigned)id[q] * 16u : BUF_OOB, 0, 0));
    const unsigned wbase = (unsigned)(c * a.cout_pad + colblock) * 192u;
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      bv[q] = load_b_unit(rsB, wbase, b_row[q], q, tid);
    }
  };
  load_idx(0);
  issue(0);
  if (nchunks > 1) load_idx(1);
  unsigned long long* const As64 = reinterpret_cast<unsigned long long*>(As);
  for (int c = 0; c < nchunks; ++c) {
    __syncthreads();   // previous chunk's fragment reads are done
#pragma unroll
    for (int q = 0; q < NX; ++q) {
      const int o = x_row[q] * (LDU * 2) + x_j[q];                    // 8-byte slots: plane p of the row starts at slot 8 p
      stage_split4(As64, o, __uint_as_float(xv[q].x), __uint_as_float(xv[q].y), __uint_as_float(xv[q].z), __uint_as_float(xv[q].w));
    }
#pragma unroll
    for (int q = 0; q < NB; ++q)
      if (b_row[q] >= 0) Bs[b_row[q] * LDU + b_w[q]] = bv[q];
    __syncthreads();
    if (c + 1 < nchunks) {
      issue(c + 1);                                                   // (its indices arrived during the previous chunk)
      if (c + 2 < nchunks) load_idx(c + 2);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 af[3][TM], bf[3][TN];
#pragma unroll
      for (int p = 0; p < 3; ++p) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
          af[p][i] = __builtin_bit_cast(bf16x8, As[((wm * TM + i) * 32 + r31) * LDU + p * 4 + ks * 2 + half]);
#pragma unroll
        for (int j = 0; j < TN; ++j)
          bf[p][j] = __builtin_bit_cast(bf16x8, Bs[((wn * TN + j) * 32 + r31) * LDU + p * 4 + ks * 2 + half]);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {           // smallest terms first
          acc[i][j] = bf6_terms(af[0][i], af[1][i], af[2][i], bf[0][j], bf[1][j], bf[2][j], acc[i][j]);
        }
    }
  }
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = colblock + (wn * TN + j) * 32 + r31;
    if (col >= a.cout) continue;
    const float b = a.bias ? a.bias[col] : 0.f;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int r = cfrag_row((wm * TM + i) * 32, e, half);
        if (r >= npos) continue;
        a.out[(size_t)(pos0 + r) * a.cout + col] = act1(acc[i][j][e] + b, a.act, a.slope);
      }
  }
}

// k_conv_thin, k_thin_project*, k_thin_gather*, k_conv_wave16*, the narrow-output kernels: pcc_conv_thin.hip

// ------------------------------------------------------------------------------------------
// dispatch, packing (mfma_ok, conv_kind and the other pure shape helpers: pcc_conv.h)
// ------------------------------------------------------------------------------------------
int split_planes(float* packed, int64_t fp32_elems, int cin, hipStream_t s) {
  if (cin % 32 != 0) return PCC_OK;
  k_split_packed<<<(unsigned)pcc_cdiv(fp32_elems / 2, 256), 256, 0, s>>>(packed, fp32_elems / 2, (unsigned*)(packed + fp32_elems));
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}
// the scaled fp16 planes and column scales behind the bf16 planes of a pack of K offsets (K = 1: the flat operand of a dense product)
int split_planes_h(float* packed, int64_t fp32_elems, int K, int cin, int cout_pad, hipStream_t s) {
  float* const planes = packed + fp32_elems + bf_plane_elems(fp32_elems);
  k_split_packed_h<<<dim3((unsigned)pcc_cdiv(cout_pad, 128), (unsigned)K), 128, 0, s>>>(packed, cin >> 5, cout_pad, (unsigned char*)planes,
                                                                                       planes + fp32_elems);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}
// The fields every MFMA launch fills: an identity map (no header, one output row per input row or pair) of a K-offset pack.
// Callers with a kernel map set hdr / nbr / rows afterwards; pair products set pair_in / tile_k / n_tiles.
ConvArgs conv_args(const float* feat, long long n_in, int cin, const float* wp, int K, int cout, const float* bias, float* out,
                   long long n_out, int act, float slope) {
  ConvArgs a;
  a.feat = feat; a.wp = wp; a.bias = bias; a.hdr = nullptr; a.nbr = nullptr; a.rows = nullptr; a.out = out;
  a.n_out = n_out; a.cin = cin; a.cout = cout; a.cout_pad = cout_pad_for(cout);
  a.n_in = n_in; a.wp_elems = (long long)K * cin * a.cout_pad;
  a.cb_log2 = cb_log2_for(cin); a.ppo = cin >> a.cb_log2; a.act = act; a.slope = slope;
  return a;
}
extern "C" int64_t pcc_conv_packed_elems(int32_t K, int32_t cin, int32_t cout) {
  if (K <= 0 || cin <= 0 || cout <= 0) return 0;
  switch (conv_kind(K, cin, cout)) {
    case KIND_MFMA: {
      const int64_t base = (int64_t)K * cin * cout_pad_for(cout);
      return mfma_packed_total(base, cin) + (conv_has_h(K, cin, cout) ? base + (int64_t)K * cout_pad_for(cout) : 0);
    }
    case KIND_WAVE16: return (int64_t)K * 16 * cin;
    case KIND_THIN_T: case KIND_THIN: return (int64_t)K * cin * cout;
    default: return 0;
  }
}

// scratch floats pcc_conv_fwd needs (two-pass thin form: the projection buffer t[K*cout][n_in])
extern "C" size_t pcc_conv_ws_bytes(int64_t n_in, int32_t K, int32_t cin, int32_t cout) {
  if (conv_kind(K, cin, cout) == KIND_THIN_T) return (size_t)K * cout * (size_t)n_in * sizeof(float) + 256;
  return 256;
}

// W [K][cin][cout] -> MFMA layout [K*ppo][cout_pad][CB] (zero padded columns)
__global__ void k_pack_mfma(const float* __restrict__ W, int K, int cin, int cout, int cout_pad, int cb_log2,
                            float* __restrict__ out) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long total = (long long)K * cin * cout_pad;
  if (t >= total) return;
  const int CB = 1 << cb_log2;
  const int within = (int)(t & (CB - 1));
  const long long q = t >> cb_log2;
  const int col = (int)(q % cout_pad);
  const long long piece = q / cout_pad;
  const int ppo = cin >> cb_log2;
  const int kid = (int)(piece / ppo), cbi = (int)(piece % ppo);
  const int ci = (cbi << cb_log2) + within;
  out[t] = (col < cout) ? W[((long long)kid * cin + ci) * cout + col] : 0.f;
}

// The same for cin a multiple of 32 with the three bf16 planes of the split path written in the same pass (round 4: pack + split
// were two launches per weight and a training step packs ~45 weights), reading the source through strides: W'[k][ci][co] =
// W[kk * sk + ci * sci + co * sco], kk = K-1-k when `flip` -- the data gradient's transposed / offset-reversed kernels are
// packed straight from the parameter (no torch flip / permute / copy in front).  One thread = two consecutive channels.
__global__ void k_pack_mfma_split(const float* __restrict__ W, int K, int cin, int cout, int cout_pad, long long sk, long long sci,
                                  long long sco, int flip, float* __restrict__ out, unsigned* __restrict__ planes) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;      // pair index of the packed image
  const long long pairs = (long long)K * cin * cout_pad / 2;
  if (t >= pairs) return;
  const int within = (int)(t & 15) * 2;
  const long long q = t >> 4;                                                 // packed row = (piece, column)
  const int col = (int)(q % cout_pad);
  const long long piece = q / cout_pad;
  const int ppo = cin >> 5;
  const int kid = (int)(piece / ppo), cbi = (int)(piece % ppo);
  const int ci = (cbi << 5) + within;
  const int kk = flip ? K - 1 - kid : kid;
  float v0 = 0.f, v1 = 0.f;
  if (col < cout) {
    const float* w = W + kk * sk + col * sco;
    v0 = w[ci * sci];
    v1 = w[(ci + 1) * sci];
  }
  *reinterpret_cast<float2*>(out + 2 * t) = make_float2(v0, v1);
  unsigned h, m, l;
  bf_split2(v0, v1, h, m, l);
  unsigned* d = planes + q * 48 + (t & 15);
  d[0] = h; d[16] = m; d[32] = l;
}

// W [K][cin][cout] -> wave16 layout [K][cin/4][16][4] (k-quad major, 16 zero-padded output columns, 4 channels each:
// the LDS image of k_conv_wave16*, see wave16_w)
__global__ void k_pack_wave16(const float* __restrict__ W, int K, int cin, int cout, float* __restrict__ out) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)K * 16 * cin) return;
  const int c4 = (int)(t & 3);
  const int o = (int)((t >> 2) & 15);
  const int kq = (int)((t >> 6) % (cin / 4));
  const int k = (int)(t / ((long long)cin * 16));
  const int c = kq * 4 + c4;
  out[t] = o < cout ? W[((long long)k * cin + c) * cout + o] : 0.f;
}

// W [K][cin][cout] -> thin layout [K][cout][cin]
__global__ void k_pack_thin(const float* __restrict__ W, int K, int cin, int cout, float* __restrict__ out) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)K * cin * cout) return;
  const int c = (int)(t % cin);
  const int o = (int)((t / cin) % cout);
  const int k = (int)(t / ((long long)cin * cout));
  out[t] = W[((long long)k * cin + c) * cout + o];
}

static int pack_weights_impl(const float* W, int32_t K, int32_t cin, int32_t cout, long long sk, long long sci, long long sco,
                             int flip, float* packed, int64_t packed_cap, hipStream_t s);

extern "C" int pcc_conv_pack_weights(const float* W, int32_t K, int32_t cin, int32_t cout, float* packed,
                                     int64_t packed_cap, void* stream) {
  return pack_weights_impl(W, K, cin, cout, (long long)cin * cout, cout, 1, 0, packed, packed_cap, (hipStream_t)stream);
}

// The pack of W'[k][ci][co] = W[(flip ? K-1-k : k)][co][ci] when `transpose` (W stored [K][cout][cin]: the kernel of the
// convolution whose data gradient is being computed), else of W itself with the offsets reversed.
extern "C" int pcc_conv_pack_weights_ex(const float* W, int32_t K, int32_t cin, int32_t cout, int32_t transpose, int32_t flip,
                                        float* packed, int64_t packed_cap, void* stream) {
  return pack_weights_impl(W, K, cin, cout, (long long)cin * cout, transpose ? 1 : cout, transpose ? cin : 1, flip ? 1 : 0, packed,
                           packed_cap, (hipStream_t)stream);
}

static int pack_weights_impl(const float* W, int32_t K, int32_t cin, int32_t cout, long long sk, long long sci, long long sco,
                             int flip, float* packed, int64_t packed_cap, hipStream_t s) {
  PCC_REQUIRE(W && packed && K >= 1 && K <= MAXK && cin >= 1 && cout >= 1, "pcc_conv_pack_weights: bad arguments");
  const bool plain = sk == (long long)cin * cout && sci == cout && sco == 1 && !flip;
  const int64_t total = pcc_conv_packed_elems(K, cin, cout);
  if (packed_cap < total) {   // a buffer sized with another layout's query (round 1: GDN sized by the conv query) is refused
    pcc_set_error("pcc_conv_pack_weights: packed buffer holds %lld floats, the layout needs %lld", (long long)packed_cap, (long long)total);
    return PCC_EWS;
  }
  const unsigned g = (unsigned)pcc_cdiv(total > 0 ? total : 1, 256);
  switch (conv_kind(K, cin, cout)) {
    case KIND_MFMA: {
      const int64_t base = (int64_t)K * cin * cout_pad_for(cout);
      if (cin % 32 == 0) {
        k_pack_mfma_split<<<(unsigned)pcc_cdiv(base / 2, 256), 256, 0, s>>>(W, K, cin, cout, cout_pad_for(cout), sk, sci, sco, flip,
                                                                             packed, (unsigned*)(packed + base));
        PCC_LAUNCH_CHECK();
      } else {
        PCC_REQUIRE(plain, "pcc_conv_pack_weights_ex: transposed / reversed source needs cin a multiple of 32");
        k_pack_mfma<<<(unsigned)pcc_cdiv(base, 256), 256, 0, s>>>(W, K, cin, cout, cout_pad_for(cout), cb_log2_for(cin), packed);
        PCC_LAUNCH_CHECK();
      }
      if (conv_has_h(K, cin, cout)) {
        const int cp = cout_pad_for(cout);
        PCC_TRY(split_planes_h(packed, base, K, cin, cp, s));
      }
      break;
    }
    case KIND_WAVE16:
      PCC_REQUIRE(plain, "pcc_conv_pack_weights_ex: transposed / reversed source is packed for the MFMA layout only");
      k_pack_wave16<<<g, 256, 0, s>>>(W, K, cin, cout, packed);
      break;
    case KIND_THIN_T: case KIND_THIN:
      PCC_REQUIRE(plain, "pcc_conv_pack_weights_ex: transposed / reversed source is packed for the MFMA layout only");
      k_pack_thin<<<g, 256, 0, s>>>(W, K, cin, cout, packed);
      break;
    default:
      pcc_set_error("pcc_conv: unsupported shape cin=%d cout=%d (MFMA path needs cin in {4,8,16} or a multiple of 32)", cin, cout);
      return PCC_EINVAL;
  }
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

// ---- per-launch event timing (bench.py roofline) ------------------------------------------------
static bool g_prof_on = false;
static std::vector<hipEvent_t> g_ev_pool;
static size_t g_ev_used = 0;
static int64_t g_launches = 0;
// which kernel form a timed launch took, with the work the library itself knows (dense products: rows x columns x depth;
// gathered forms report 0 -- their pair counts live on the device, the caller accounts them)
// bm / bn / ksplit: the row tile, column tile and reduction split as launched (0, 0, 1: a form without such a choice)
struct ProfRec { int form; double flops, bytes; int bm, bn, ksplit; };
static std::vector<ProfRec> g_prof_recs;
static ProfRec g_form = {PCC_FORM_OTHER, 0.0, 0.0, 0, 0, 1};
void prof_note(int form, double flops, double bytes) { g_form = {form, flops, bytes, 0, 0, 1}; }
void prof_tile(int bm, int bn, int ksplit) { g_form.bm = bm; g_form.bn = bn; g_form.ksplit = ksplit; }   // after prof_note
static void prof_push() {
  g_prof_recs.push_back(g_form);
  g_form = {PCC_FORM_OTHER, 0.0, 0.0, 0, 0, 1};
  ++g_launches;
}

extern "C" int pcc_prof_enable(int32_t on) {
  g_prof_on = on != 0;
  g_ev_used = 0;
  g_launches = 0;
  g_prof_recs.clear();
  return PCC_OK;
}

static int prof_event(hipStream_t s) {
  if (g_ev_used == g_ev_pool.size()) {
    hipEvent_t e;
    PCC_CHECK_HIP(hipEventCreate(&e));
    g_ev_pool.push_back(e);
  }
  PCC_CHECK_HIP(hipEventRecord(g_ev_pool[g_ev_used++], s));
  return PCC_OK;
}
// event pair around a launch while pcc_prof_enable is on (and `when`)
int prof_begin(hipStream_t s, bool when) { return (g_prof_on && when) ? prof_event(s) : PCC_OK; }
int prof_end(hipStream_t s, bool when, int form) {   // form >= 0: noted between the end event and the record
  if (!(g_prof_on && when)) return PCC_OK;
  PCC_TRY(prof_event(s));
  if (form >= 0) prof_note(form, 0.0, 0.0);
  prof_push();
  return PCC_OK;
}
bool prof_on() { return g_prof_on; }

extern "C" int pcc_prof_collect(double* h_conv_ms, int64_t* h_conv_launches) {
  double ms = 0.0;
  for (size_t i = 0; i + 1 < g_ev_used; i += 2) {
    PCC_CHECK_HIP(hipEventSynchronize(g_ev_pool[i + 1]));
    float t = 0.f;
    PCC_CHECK_HIP(hipEventElapsedTime(&t, g_ev_pool[i], g_ev_pool[i + 1]));
    ms += t;
  }
  if (h_conv_ms) *h_conv_ms = ms;
  if (h_conv_launches) *h_conv_launches = g_launches;
  g_ev_used = 0;
  g_launches = 0;
  g_prof_recs.clear();
  return PCC_OK;
}

extern "C" int64_t pcc_prof_sequence(int32_t* h_forms, int64_t cap) {
  const int64_t n = (int64_t)g_prof_recs.size();
  for (int64_t i = 0; i < n && i < cap && h_forms; ++i) h_forms[i] = g_prof_recs[(size_t)i].form;
  return n;
}

extern "C" int64_t pcc_prof_sequence_tiles(int32_t* h_tiles, int64_t cap) {
  const int64_t n = (int64_t)g_prof_recs.size();
  for (int64_t i = 0; i < n && i < cap && h_tiles; ++i) {
    const ProfRec& r = g_prof_recs[(size_t)i];
    h_tiles[3 * i] = r.bm; h_tiles[3 * i + 1] = r.bn; h_tiles[3 * i + 2] = r.ksplit;
  }
  return n;
}

extern "C" int pcc_prof_collect_forms(double* h_ms, int64_t* h_launches, double* h_flops, double* h_bytes) {
  PCC_REQUIRE(h_ms && h_launches && h_flops && h_bytes, "pcc_prof_collect_forms: NULL array");
  for (int f = 0; f < PCC_FORM_COUNT; ++f) { h_ms[f] = 0.0; h_launches[f] = 0; h_flops[f] = 0.0; h_bytes[f] = 0.0; }
  for (size_t i = 0; i + 1 < g_ev_used && i / 2 < g_prof_recs.size(); i += 2) {
    PCC_CHECK_HIP(hipEventSynchronize(g_ev_pool[i + 1]));
    float t = 0.f;
    PCC_CHECK_HIP(hipEventElapsedTime(&t, g_ev_pool[i], g_ev_pool[i + 1]));
    const ProfRec& r = g_prof_recs[i / 2];
    const int f = (r.form >= 0 && r.form < PCC_FORM_COUNT) ? r.form : PCC_FORM_OTHER;
    h_ms[f] += t; h_launches[f] += 1; h_flops[f] += r.flops; h_bytes[f] += r.bytes;
  }
  g_ev_used = 0;
  g_launches = 0;
  g_prof_recs.clear();
  return PCC_OK;
}

static bool g_mfma_buf = getenv("PCC_MFMA_BUF") ? atoi(getenv("PCC_MFMA_BUF")) != 0 : true;
// split path (fp32 products as six bf16 MFMA terms, k_conv_mfma_bf) unless the call asks for PCC_ARITH_F32 (fp32-input MFMA kernels);
// dense / pair products in scaled fp16 pairs (k_gemm_h2, k_pair_h2) only under PCC_ARITH_H3
static bool split_ok(const ConvArgs& a) {
  return a.arith != PCC_ARITH_F32 && g_mfma_buf && a.cb_log2 == 5 && a.n_in > 0 && a.n_in * a.cin * 6 <= BUF_MAX_BYTES && a.wp_elems > 0 &&
         bf_plane_elems(a.wp_elems) * 4 <= BUF_MAX_BYTES;
}

// out = act(bias + sum_s part[s]) in ascending s (fixed order: deterministic); 4 channels per thread
__global__ void __launch_bounds__(256) k_splitk_reduce(const float* __restrict__ part, int S, long long n4, int cout4,
                                                       const float* __restrict__ bias, int act, float slope, float* __restrict__ out) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n4) return;
  float4 v = reinterpret_cast<const float4*>(part)[t];
  for (int sidx = 1; sidx < S; ++sidx) {
    const float4 p = reinterpret_cast<const float4*>(part)[(long long)sidx * n4 + t];
    v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
  }
  if (bias) {
    const float4 b = reinterpret_cast<const float4*>(bias)[t % cout4];
    v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
  }
  v.x = act1(v.x, act, slope); v.y = act1(v.y, act, slope); v.z = act1(v.z, act, slope); v.w = act1(v.w, act, slope);
  reinterpret_cast<float4*>(out)[t] = v;
}

static constexpr int SPLITK_CHUNKS = 40;     // chunks of a split reduction per workgroup
static int g_dbg = getenv("PCC_DBG") ? atoi(getenv("PCC_DBG")) : 0;
// non-temporal accesses of the streamed multi-GB buffers (bit 0 dense products' stores, 1 pair products' stores, 2 gather-sum
// product loads, 3 gather-sum output stores, 4 projection-plane stores, 5 projection-plane gathers); env PCC_NT
static int g_nt = getenv("PCC_NT") ? atoi(getenv("PCC_NT")) : 1;
int nt_flags() { return g_nt; }

int launch_mfma(int mode, const ConvArgs& a_in, int tiles_bound_extra, hipStream_t s) {
  ConvArgs a = a_in;
  const int bn = bn_for(a.cout);
  const long long gy = a.cout_pad / bn;
  const bool gemm_groups = !a.hdr && !a.pair_in && gy > 8;      // k_conv_mfma*: row tiles in groups of 8 (whole groups in the grid)
  auto tiles = [&](int bm) {
    const long long t = pcc_cdiv(a.n_out, bm) + tiles_bound_extra;
    return gemm_groups ? (t + 7) / 8 * 8 : t;
  };
  int ksplit_grid = 1;
  auto grid = [&](int bm) { return dim3((unsigned)((tiles(bm) * gy * ksplit_grid + 7) / 8 * 8)); };   // 1-D, multiple of 8 (XCD ranges)
  // few rows: shrink the row tile until the grid covers the 256 CUs about twice
  const long long want = 512;
  const bool buf = g_mfma_buf && a.n_in > 0 && a.n_in * a.cin * 4 <= BUF_MAX_BYTES && a.wp_elems > 0 &&
                   a.wp_elems * 4 <= BUF_MAX_BYTES;
  const bool split = split_ok(a);
  // few row tiles but a deep (offset x channel-block) reduction -- the 15 k-row / 4 k-row / 1 k-row layers of the hyper-prior:
  // a serial loop of 100-160 chunks at ~2 us per chunk on a handful of CUs.  Cut the reduction over ksplit workgroups
  // (partial tiles in the library scratch, summed in fixed order): the chain gets ksplit times shorter and the grid fills.
  int ksplit = 1;
  // (round 4: also the K = 1 products with a very deep reduction -- the data gradient of a generative transposed convolution is
  //  dT [n, 125 * cout] x Wflat^T: 500 chunks in one workgroup per 128 rows, 45 workgroups, 0.58 ms for 23 GFLOP)
  if (split && mode == MODE_CONV && !a.pair_in && !a.rows && (a.cout & 3) == 0) {
    const int depth = (a.hdr ? 27 : 1) * a.ppo;        // chunks of a 3x3x3 map (the maps that reach here; 5x5x5 take the pair form)
    if (tiles(128) * gy < 256 && depth >= 64) {
      ksplit = depth / SPLITK_CHUNKS;                  // ~40 chunks per workgroup
      if (ksplit > 8) ksplit = 8;
      if (ksplit < 2) ksplit = 1;
    }
  }
  // dense products of the generative transposed convolutions whose pack carries fp16 planes: three-term fp16 form
  if (split && a.arith == PCC_ARITH_H3 && a.wh_ok && mode == MODE_CONV && !a.hdr && !a.pair_in && !a.rows && !a.bias && a.act == 0 && ksplit == 1 &&
      bn == 128 && (tiles(128) * gy >= want || a.feath) && (size_t)128 * a.cout * 4 < (1ull << 31) &&
      nch_ok(a.ppo)) {      // (caller's planes: the caller chose the form)
    if (!a.feath) PCC_TRY(make_planes_h(a, s));
    a.dbg = g_dbg;
    a.nt = g_nt;
    prof_note(PCC_FORM_GEMM_H2, 2.0 * a.n_out * a.cin * a.cout, 4.0 * ((double)a.n_out * a.cin + (double)a.n_out * a.cout + (double)a.cin * a.cout));
    prof_tile(128, 128, 1);
    return launch_gemm_h2(a, grid(128), s);
  }
  if (split && a.featb) {
    PCC_REQUIRE(ksplit == 1, "launch_mfma: caller planes with a split reduction");
  } else if (split) {
    const size_t plane_bytes = pcc_align_up((size_t)a.n_in * a.cin * 6);
    const size_t part_bytes = ksplit > 1 ? (size_t)ksplit * (size_t)a.n_out * a.cout * 4 : 0;
    void* p = nullptr;
    PCC_TRY(lib_scratch(plane_bytes + part_bytes, &p));
    const long long pairs = (long long)a.n_in * a.cin / 2;
    k_feat_split<<<(unsigned)pcc_cdiv(pairs, 256), 256, 0, s>>>(a.feat, pairs, a.cin / 2, mode != MODE_CONV ? 1 : 0, (unsigned*)p);
    PCC_LAUNCH_CHECK();
    a.featb = (const unsigned char*)p;
    if (ksplit > 1) { a.ksplit = ksplit; a.part = (float*)((char*)p + plane_bytes); }
  }
  a.dbg = g_dbg;
  a.nt = g_nt;
  ksplit_grid = a.ksplit;
  // plain dense products (generative transposed convolutions): the stripped GEMM kernel
  if (split && mode == MODE_CONV && !a.hdr && !a.pair_in && !a.rows && !a.bias && a.act == 0 && a.ksplit == 1 &&
      bn == 128 && tiles(128) * gy >= want && (size_t)128 * a.cout * 4 < (1ull << 31)) {
    prof_note(PCC_FORM_GEMM_BF2, 2.0 * a.n_out * a.cin * a.cout, 4.0 * ((double)a.n_out * a.cin + (double)a.n_out * a.cout + (double)a.cin * a.cout));
    if (nch_ok(a.ppo)) {
      prof_tile(128, 128, 1);
      return launch_gemm_bf2(a, grid(128), s);
    }
  }
  prof_note(split ? PCC_FORM_CONV_BF : PCC_FORM_CONV_F32, (!a.hdr && !a.pair_in) ? 2.0 * a.n_out * a.cin * a.cout : 0.0, 0.0);
#define PCC_LAUNCH_MFMA(WM, WN, TM, TN, BMV)                                                     \
  do {                                                                                           \
    prof_tile(BMV, bn, a.ksplit);                                                                \
    if (split) PCC_TRY(launch_conv_bf(mode, WM, WN, TM, TN, a, grid(BMV), s));                   \
    else PCC_TRY(launch_conv_f32(mode, WM, WN, TM, TN, buf, a, grid(BMV), s));                   \
  } while (0)
  // (a split reduction multiplies the grid: count it, so that split layers keep the large row tile and its weight reuse)
  const long long ksg = a.ksplit;
  if (bn == 128) {
    if (tiles(128) * gy * ksg >= want) PCC_LAUNCH_MFMA(2, 2, 2, 2, 128);
    else if (tiles(64) * gy * ksg >= want) PCC_LAUNCH_MFMA(2, 2, 1, 2, 64);
    else PCC_LAUNCH_MFMA(1, 4, 1, 1, 32);
  } else if (bn == 64) {
    if (tiles(128) * gy >= want) PCC_LAUNCH_MFMA(2, 2, 2, 1, 128);
    else PCC_LAUNCH_MFMA(2, 2, 1, 1, 64);
  } else PCC_LAUNCH_MFMA(4, 1, 1, 1, 128);
#undef PCC_LAUNCH_MFMA
  PCC_LAUNCH_CHECK();
  if (a.ksplit > 1) {
    const long long n4 = a.n_out * a.cout / 4;
    k_splitk_reduce<<<(unsigned)pcc_cdiv(n4, 256), 256, 0, s>>>(a.part, a.ksplit, n4, a.cout / 4, a.bias, a.act, a.slope, a.out);
    PCC_LAUNCH_CHECK();
  }
  return PCC_OK;
}

// The gathered pair GEMM of pcc_conv_fwd_pairs and pcc_convt_fwd_rows: a (pair mode, form set) in, T = a.out written.
int launch_pair_product(ConvArgs& a, int K, long long tiles, hipStream_t s) {
  PCC_TRY(prof_begin(s));
  const int bn = bn_for(a.cout);
  const long long gy = a.cout_pad / bn;
  const dim3 grid((unsigned)((tiles * gy + 7) / 8 * 8));
  const bool buf = g_mfma_buf && a.n_in * a.cin * 4 <= BUF_MAX_BYTES && a.wp_elems * 4 <= BUF_MAX_BYTES;
  const bool split = split_ok(a);
  const bool pair_h = split && a.arith == PCC_ARITH_H3 && conv_has_h(K, a.cin, a.cout) && (size_t)a.n_in * a.cin * 4 <= (size_t)BUF_MAX_BYTES &&
                      nch_ok(a.ppo);
  prof_note(pair_h ? PCC_FORM_PAIR_H2 : split ? PCC_FORM_PAIR_BF : PCC_FORM_CONV_F32, 0.0, 0.0);
#define PCC_LAUNCH_PAIR(WM, WN, TM, TN)                                                         \
  do {                                                                                          \
    prof_tile(128, bn, 1);                                                                      \
    if (split) PCC_TRY(launch_conv_bf(MODE_CONV, WM, WN, TM, TN, a, grid, s));                  \
    else PCC_TRY(launch_conv_f32(MODE_CONV, WM, WN, TM, TN, buf, a, grid, s));                  \
  } while (0)
  if (pair_h) {                                   // scaled fp16 pairs, three MFMA terms (k_pair_h2)
    PCC_TRY(make_planes_h(a, s));
    prof_tile(128, 128, 1);
    PCC_TRY(launch_pair_h2(a, grid, s));
  } else {
    if (split) PCC_TRY(make_planes(a, false, s));
    if (bn == 128) PCC_LAUNCH_PAIR(2, 2, 2, 2);
    else if (bn == 64) PCC_LAUNCH_PAIR(2, 2, 2, 1);
    else PCC_LAUNCH_PAIR(4, 1, 1, 1);
    PCC_LAUNCH_CHECK();
  }
#undef PCC_LAUNCH_PAIR
  return prof_end(s);
}

// 4-channel inputs: output rows from which the flattened form (k_conv_in4_bf) replaces the offset-by-offset kernel; negative = never
static long long g_in4_min_rows = 65536;
extern "C" int pcc_set_in4_min_rows(int64_t rows) { g_in4_min_rows = rows; return PCC_OK; }

extern "C" int pcc_conv_fwd(const float* feat_in, int64_t n_in, int32_t cin, const float* packed_w,
                            const float* bias, int32_t K, int32_t cout, const int32_t* hdr, const int32_t* nbr,
                            const int32_t* rows, int64_t n_out, float* out, int32_t act, float slope,
                            void* ws, size_t ws_bytes, int32_t arith, int32_t* d_guard, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n_out <= 0) return PCC_OK;
  PCC_REQUIRE(feat_in && packed_w && out && n_in > 0, "pcc_conv_fwd: NULL array");
  PCC_REQUIRE(K >= 1 && K <= MAXK, "pcc_conv_fwd: K=%d unsupported", K);
  PCC_REQUIRE(hdr ? (nbr != nullptr) : (K == 1 && n_in == n_out), "pcc_conv_fwd: map missing (only K=1 may omit it)");
  PCC_REQUIRE(act >= 0 && act <= 2, "pcc_conv_fwd: bad activation");
  PCC_REQUIRE(n_in < (1ll << 31) && n_out < (1ll << 31), "pcc_conv_fwd: too many rows");
  const int kind = conv_kind(K, cin, cout);
  PCC_REQUIRE(kind != KIND_NONE, "pcc_conv_fwd: unsupported shape cin=%d cout=%d", cin, cout);
  const bool timed = kind == KIND_MFMA || kind == KIND_WAVE16;   // the roofline kernels: MFMA launches
  PCC_TRY(prof_begin(s, timed));
  if (kind == KIND_MFMA) {
    ConvArgs a = conv_args(feat_in, n_in, cin, packed_w, K, cout, bias, out, n_out, act, slope);
    a.hdr = hdr; a.nbr = nbr; a.rows = rows;
    PCC_TRY(set_arith(a, arith, d_guard, "pcc_conv_fwd"));
    const bool in4 = g_in4_min_rows >= 0 && arith != PCC_ARITH_F32;
    // the input layer: 4 channels, K * 4 <= 512 flattened into one reduction axis (k_conv_in4_bf); plain conv maps of >= 64 k
    // output rows (one segment, canonical row order: what pcc_kernel_map_build makes for a non-transposed map)
    if (in4 && cin == 4 && K * 4 <= 512 && K > 1 && hdr && !rows && bn_for(cout) == 128 && n_out >= g_in4_min_rows &&
        n_in * 16 <= BUF_MAX_BYTES && n_out * (long long)K < (1ll << 31) && ((uintptr_t)feat_in & 15) == 0) {
      void* wpl = nullptr;
      PCC_TRY(lib_scratch_small((size_t)16 * a.cout_pad * 192, &wpl));
      k_in4_weight_planes<<<(unsigned)pcc_cdiv(16 * a.cout_pad * 16, 256), 256, 0, s>>>(packed_w, K, a.cout_pad, (unsigned*)wpl);
      const long long gy = a.cout_pad / 128;
      const unsigned grid = (unsigned)((pcc_cdiv(n_out, 128) * gy + 7) / 8 * 8);
      prof_note(PCC_FORM_CONV_BF, 0.0, 0.0);
      prof_tile(128, 128, 1);
      k_conv_in4_bf<2><<<grid, 256, 0, s>>>(a, (const unsigned*)wpl, K);
      PCC_LAUNCH_CHECK();
    } else
    PCC_TRY(launch_mfma(MODE_CONV, a, rows ? PCC_MAP_MAX_SEG : 0, s));
  } else if (kind == KIND_WAVE16) {
    PCC_TRY(launch_conv_wave16(feat_in, n_in, cin, packed_w, bias, K, cout, hdr, nbr, rows, n_out, out, act, slope, s));
  } else if (kind == KIND_THIN_T) {
    PCC_TRY(launch_conv_thin_t(feat_in, n_in, cin, packed_w, bias, K, cout, hdr, nbr, rows, n_out, out, act, slope, ws, ws_bytes, s));
  } else {
    PCC_TRY(launch_conv_thin(feat_in, cin, packed_w, bias, cout, hdr, nbr, rows, n_out, out, act, slope, s));
  }
  PCC_TRY(prof_end(s, timed));
  return PCC_OK;
}

// ------------------------------------------------------------------------------------------
// Pair-list form of a sparse convolution, for maps where most (offset, output row) slots are empty (5x5x5 kernels on
// surfaces: 36 of 125).  The output-stationary kernel multiplies whole 128-row tiles per active offset, so its MFMA
// work scales with K * rows, not with the pairs.  Here the pairs of each offset are compacted (padded to whole
// 128-pair tiles), T[p] = feat[in(p)] @ W[k(p)] runs as a gathered GEMM with one offset per tile -- every MFMA row is
// a real pair -- and out[o] = bias + sum_k T[pos(k, o)] is taken in ascending k: deterministic, no atomics.
// ------------------------------------------------------------------------------------------
__global__ void k_pair_flags(const int* __restrict__ nbr, long long n, int* __restrict__ f) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) f[e] = nbr[e] >= 0 ? 1 : 0;
}

// one block: padded start of every offset's pair range; info = {padded pairs, tiles, pairs}
__global__ void __launch_bounds__(128) k_pair_starts(const int* __restrict__ g, const int* __restrict__ nbr, long long n_out, int K,
                                                     int* __restrict__ pstart /*[K+1]*/, long long* __restrict__ info) {
  __shared__ long long cnt[MAXK];
  const long long n = n_out * K;
  const long long total = (long long)g[n - 1] + (nbr[n - 1] >= 0 ? 1 : 0);
  for (int k = threadIdx.x; k < K; k += blockDim.x) {         // the 2K boundary reads in parallel, then a short serial prefix
    const long long b = g[(long long)k * n_out];
    const long long e = (k + 1 < K) ? g[(long long)(k + 1) * n_out] : total;
    cnt[k] = e - b;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  long long run = 0;
  for (int k = 0; k < K; ++k) {
    pstart[k] = (int)run;
    run += (cnt[k] + PAIR_BM - 1) / PAIR_BM * PAIR_BM;
  }
  pstart[K] = (int)run;
  info[0] = run; info[1] = run / PAIR_BM; info[2] = total;
}

__global__ void k_pair_pos(const int* __restrict__ nbr, const int* __restrict__ g, const int* __restrict__ pstart,
                           long long n_out, int K, int* __restrict__ pos) {
  const long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int k = blockIdx.y;
  if (o >= n_out) return;
  const long long e = (long long)k * n_out + o;
  pos[e] = nbr[e] >= 0 ? pstart[k] + (g[e] - g[(long long)k * n_out]) : -1;
}

__global__ void k_pair_fill(const int* __restrict__ nbr, const int* __restrict__ pos, long long n,
                            int* __restrict__ pair_in) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n && pos[e] >= 0) pair_in[pos[e]] = nbr[e];
}

__global__ void k_pair_tile_k(const int* __restrict__ pstart, int K, long long tiles, int* __restrict__ tile_k) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= tiles) return;
  const long long p = t * PAIR_BM;
  int lo = 0, hi = K;                 // last k with pstart[k] <= p
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (pstart[mid] <= p) lo = mid; else hi = mid; }
  tile_k[t] = lo;
}

int launch_pair_tile_k(const int* pstart, int K, long long tiles, int* tile_k, hipStream_t s) {   // also pcc_convt_fwd_rows
  k_pair_tile_k<<<(unsigned)pcc_cdiv(tiles, 256), 256, 0, s>>>(pstart, K, tiles, tile_k);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_conv_pairs_supported(int32_t K, int32_t cin, int32_t cout) {
  return (K >= 1 && K <= MAXK && conv_kind(K, cin, cout) == KIND_MFMA && cout % 4 == 0) ? 1 : 0;
}

extern "C" size_t pcc_pair_plan_ws_bytes(int64_t n_out, int32_t K) {
  const int64_t n = n_out * K;
  return 2 * pcc_align_up((size_t)n * 4) + pcc_scan_ws_bytes(n) + 1024;
}

// phase 1: pos[k][o] (row of pair (k,o) in the padded pair list, -1 = no pair), pstart[K+1], info[3]
extern "C" int pcc_pair_plan_rank(const int32_t* nbr, int64_t n_out, int32_t K, int32_t* pos, int32_t* pstart,
                                  int64_t* info, void* ws, size_t ws_bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PCC_REQUIRE(nbr && pos && pstart && info && ws && n_out > 0 && K >= 1 && K <= MAXK, "pcc_pair_plan_rank: bad arguments");
  const int64_t n = n_out * K;
  PCC_REQUIRE(n + (int64_t)K * PAIR_BM < (1ll << 31), "pcc_pair_plan_rank: too many map slots");
  if (ws_bytes < pcc_pair_plan_ws_bytes(n_out, K)) { pcc_set_error("pcc_pair_plan_rank: workspace too small"); return PCC_EWS; }
  char* p = (char*)ws;
  int* f = (int*)p;  p += pcc_align_up((size_t)n * 4);
  int* g = (int*)p;  p += pcc_align_up((size_t)n * 4);
  k_pair_flags<<<(unsigned)pcc_cdiv(n, 256), 256, 0, s>>>(nbr, n, f);
  PCC_LAUNCH_CHECK();
  PCC_TRY(pcc_scan_exclusive_i32(f, g, n, p, ws_bytes - (size_t)(p - (char*)ws), s));
  k_pair_starts<<<1, 128, 0, s>>>(g, nbr, n_out, K, pstart, (long long*)info);
  PCC_LAUNCH_CHECK();
  k_pair_pos<<<dim3((unsigned)pcc_cdiv(n_out, 256), (unsigned)K), 256, 0, s>>>(nbr, g, pstart, n_out, K, pos);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

// phase 2 (after the host has read info and sized the arrays): pair_in[padded pairs], tile_k[tiles]
extern "C" int pcc_pair_plan_fill(const int32_t* nbr, const int32_t* pos, const int32_t* pstart, int64_t n_out, int32_t K,
                                  int64_t padded_pairs, int32_t* pair_in, int32_t* tile_k, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PCC_REQUIRE(nbr && pos && pstart && pair_in && tile_k && padded_pairs % PAIR_BM == 0, "pcc_pair_plan_fill: bad arguments");
  if (padded_pairs == 0) return PCC_OK;
  PCC_CHECK_HIP(hipMemsetAsync(pair_in, 0xFF, (size_t)padded_pairs * 4, s));
  const int64_t n = n_out * K;
  k_pair_fill<<<(unsigned)pcc_cdiv(n, 256), 256, 0, s>>>(nbr, pos, n, pair_in);
  PCC_LAUNCH_CHECK();
  const int64_t tiles = padded_pairs / PAIR_BM;
  return launch_pair_tile_k(pstart, K, tiles, tile_k, s);
}

struct PairReduceArgs {
  const float* T; const float* bias; const int* pos; float* out; long long n_out; int K, cout, act; float slope; int lpr_log2;
};

// LPR lanes per output row, 4 channels per lane and pass; pair rows of JB offsets loaded independently.
// (Round 3: a form that fetches a row's K position entries side by side, finds the present ones by ballot and walks only those
//  in batches of 8 product loads measured the same 117 us per launch: with 8 waves per SIMD the empty offsets' round trips are
//  hidden, the kernel runs at the rate its T reads allow -- 3.7 TB/s.  Not kept.)
__global__ void __launch_bounds__(256) k_pair_reduce(PairReduceArgs a) {
  constexpr int JB = 5;
  const int lane = threadIdx.x & 63;
  const int lpr = 1 << a.lpr_log2;
  const int rpw = 64 >> a.lpr_log2;
  const long long o = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * rpw + (lane >> a.lpr_log2);
  const int cl = lane & (lpr - 1);
  if (o >= a.n_out) return;
  const int cvec = a.cout / 4;
  for (int cv = cl; cv < cvec; cv += lpr) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k0 = 0; k0 < a.K; k0 += JB) {
      int pr[JB];
#pragma unroll
      for (int u = 0; u < JB; ++u) pr[u] = (k0 + u < a.K) ? a.pos[(long long)(k0 + u) * a.n_out + o] : -1;
      float4 x[JB];
#pragma unroll
      for (int u = 0; u < JB; ++u) {
        x[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (pr[u] >= 0) x[u] = reinterpret_cast<const float4*>(a.T + (long long)pr[u] * a.cout)[cv];
      }
#pragma unroll
      for (int u = 0; u < JB; ++u) { acc.x += x[u].x; acc.y += x[u].y; acc.z += x[u].z; acc.w += x[u].w; }
    }
    if (a.bias) {
      const float4 b = reinterpret_cast<const float4*>(a.bias)[cv];
      acc.x += b.x; acc.y += b.y; acc.z += b.z; acc.w += b.w;
    }
    acc.x = act1(acc.x, a.act, a.slope); acc.y = act1(acc.y, a.act, a.slope);
    acc.z = act1(acc.z, a.act, a.slope); acc.w = act1(acc.w, a.act, a.slope);
    reinterpret_cast<float4*>(a.out + o * a.cout)[cv] = acc;
  }
}

extern "C" int pcc_conv_fwd_pairs(const float* feat_in, int64_t n_in, int32_t cin, const float* packed_w,
                                  const float* bias, int32_t K, int32_t cout, const int32_t* pair_in,
                                  const int32_t* tile_k, const int64_t* d_info, int64_t padded_pairs,
                                  const int32_t* pos, int64_t n_out, float* T, float* out, int32_t act, float slope,
                                  int32_t arith, int32_t* d_guard, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n_out <= 0) return PCC_OK;
  PCC_REQUIRE(feat_in && packed_w && pair_in && tile_k && d_info && pos && T && out, "pcc_conv_fwd_pairs: NULL array");
  PCC_REQUIRE(conv_kind(K, cin, cout) == KIND_MFMA && cout % 4 == 0, "pcc_conv_fwd_pairs: shape cin=%d cout=%d not on the MFMA path", cin, cout);
  PCC_REQUIRE(padded_pairs % PAIR_BM == 0 && padded_pairs < (1ll << 31), "pcc_conv_fwd_pairs: bad pair count");
  PCC_REQUIRE(act >= 0 && act <= 2, "pcc_conv_fwd_pairs: bad activation");
  if (padded_pairs > 0) {
    ConvArgs a = conv_args(feat_in, n_in, cin, packed_w, K, cout, nullptr, T, padded_pairs);
    a.pair_in = pair_in; a.tile_k = tile_k; a.n_tiles = (const long long*)d_info + 1;
    PCC_TRY(set_arith(a, arith, d_guard, "pcc_conv_fwd_pairs"));
    PCC_TRY(launch_pair_product(a, K, padded_pairs / PAIR_BM, s));
  }
  PairReduceArgs r;
  r.T = T; r.bias = bias; r.pos = pos; r.out = out; r.n_out = n_out; r.K = K; r.cout = cout; r.act = act; r.slope = slope;
  int l = 0;
  while ((1 << l) < cout / 4 && l < 6) ++l;
  r.lpr_log2 = l;
  const int64_t waves = pcc_cdiv(n_out, 64 >> l);
  k_pair_reduce<<<(unsigned)pcc_cdiv(waves, 4), 256, 0, s>>>(r);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

// the transposed (generative) convolutions: pcc_convt.hip; the grid-indexed thin forms: pcc_conv_thin.hip

// ------------------------------------------------------------------------------------------
// GDN
// ------------------------------------------------------------------------------------------
__global__ void k_gdn_pack(const float* __restrict__ beta_raw, const float* __restrict__ gamma_raw, int c,
                           float beta_bound, float gamma_bound, float pedestal, int cout_pad, int cb_log2,
                           float* __restrict__ packed, float* __restrict__ beta_eff) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < c) {
    const float b = fmaxf(beta_raw[t], beta_bound);
    beta_eff[t] = b * b - pedestal;
  }
  const long long total = (long long)c * cout_pad;
  if (t >= total) return;
  // conv weight W[ci][co] = gamma[co][ci]; packed layout [ppo][cout_pad][CB]
  const int CB = 1 << cb_log2;
  const int within = (int)(t & (CB - 1));
  const long long q = t >> cb_log2;
  const int col = (int)(q % cout_pad);
  const int cbi = (int)(q / cout_pad);
  const int ci = (cbi << cb_log2) + within;
  float v = 0.f;
  if (col < c) {
    const float g = fmaxf(gamma_raw[(long long)col * c + ci], gamma_bound);
    v = g * g - pedestal;
  }
  packed[t] = v;
}

extern "C" int64_t pcc_gdn_packed_elems(int32_t c) { return mfma_ok(c, c) ? mfma_packed_total((int64_t)c * cout_pad_for(c), c) : 0; }

extern "C" int pcc_gdn_pack(const float* beta_raw, const float* gamma_raw, int32_t c, float beta_min, float* packed,
                            int64_t packed_cap, float* beta_eff, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PCC_REQUIRE(beta_raw && gamma_raw && packed && beta_eff, "pcc_gdn_pack: NULL array");
  PCC_REQUIRE(mfma_ok(c, c), "pcc_gdn: channel count %d unsupported (needs 8, 16 or a multiple of 32)", c);
  const double pedestal = 1.0 / 68719476736.0;   // 2^-36
  const float beta_bound = (float)sqrt((double)beta_min + pedestal);
  const float gamma_bound = (float)sqrt(pedestal);
  const int64_t total = pcc_gdn_packed_elems(c);
  if (packed_cap < total) {
    pcc_set_error("pcc_gdn_pack: packed buffer holds %lld floats, the layout needs %lld", (long long)packed_cap, (long long)total);
    return PCC_EWS;
  }
  const int64_t base = (int64_t)c * cout_pad_for(c);
  k_gdn_pack<<<(unsigned)pcc_cdiv(base, 256), 256, 0, s>>>(beta_raw, gamma_raw, c, beta_bound, gamma_bound,
                                                          (float)pedestal, cout_pad_for(c), cb_log2_for(c), packed,
                                                          beta_eff);
  PCC_LAUNCH_CHECK();
  return split_planes(packed, base, c, s);
}

// {kernel, row tile, column tile, inverse} of the most recent pcc_gdn_fwd that launched (pcc_gdn_last_launch): GDN launches are
// not event-timed, so the profiling record never lists them
static int32_t g_gdn_last[4] = {PCC_GDN_KERNEL_NONE, 0, 0, 0};
static void gdn_note(int kernel, int bm, int bn, int inverse) {
  g_gdn_last[0] = kernel; g_gdn_last[1] = bm; g_gdn_last[2] = bn; g_gdn_last[3] = inverse ? 1 : 0;
}

extern "C" int pcc_gdn_last_launch(int32_t* h_rec) {
  PCC_REQUIRE(h_rec, "pcc_gdn_last_launch: NULL array");
  for (int i = 0; i < 4; ++i) h_rec[i] = g_gdn_last[i];
  return PCC_OK;
}

extern "C" int pcc_gdn_fwd(const float* x, int64_t n, int32_t c, const float* packed, const float* beta_eff,
                           int32_t inverse, float* out, int32_t arith, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n <= 0) return PCC_OK;
  PCC_REQUIRE(x && packed && beta_eff && out && x != out, "pcc_gdn_fwd: bad arguments");
  PCC_REQUIRE(mfma_ok(c, c), "pcc_gdn: channel count %d unsupported", c);
  ConvArgs a = conv_args(x, n, c, packed, 1, c, beta_eff, out, n);
  PCC_TRY(set_arith(a, arith, nullptr, "pcc_gdn_fwd"));
  // large sets: split folded into the staging (k_gdn_bf), no plane round trip; small ones keep the general kernel (its
  // smaller row tiles fill the chip better below ~30 k rows)
  if (split_ok(a) && c % 32 == 0 && (c & 3) == 0 && ((uintptr_t)x & 15) == 0 && n >= 32768) {
    const int bn = bn_for(c);
    if (bn == 128) {
      const long long gy = a.cout_pad / 128;
      const bool big = pcc_cdiv(n, 128) * gy >= 1024;
      const long long tiles = pcc_cdiv(n, big ? 128 : 64);
      const unsigned grid = (unsigned)((tiles * gy + 7) / 8 * 8);
      if (big) { if (inverse) k_gdn_bf<2, MODE_IGDN><<<grid, 256, 0, s>>>(a); else k_gdn_bf<2, MODE_GDN><<<grid, 256, 0, s>>>(a); }
      else { if (inverse) k_gdn_bf<1, MODE_IGDN><<<grid, 256, 0, s>>>(a); else k_gdn_bf<1, MODE_GDN><<<grid, 256, 0, s>>>(a); }
      PCC_LAUNCH_CHECK();
      gdn_note(PCC_GDN_KERNEL_FUSED, big ? 128 : 64, 128, inverse);
      return PCC_OK;
    }
  }
  PCC_TRY(launch_mfma(inverse ? MODE_IGDN : MODE_GDN, a, 0, s));
  // what prof_note / prof_tile left in g_form (they set it whether or not profiling is on)
  gdn_note(g_form.form == PCC_FORM_CONV_BF ? PCC_GDN_KERNEL_CONV_BF : PCC_GDN_KERNEL_CONV_F32, g_form.bm, g_form.bn, inverse);
  return PCC_OK;
}
