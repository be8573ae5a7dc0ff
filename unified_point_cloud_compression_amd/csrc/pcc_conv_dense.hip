// The stripped GEMM kernels of the dense products (generative transposed convolutions: k_gemm_bf2, k_gemm_h2) and of the gathered
// pair products (k_pair_h2), unrolled over the chunk count cin / 32, each behind one launcher.  launch_mfma and
// launch_pair_product (pcc_conv.hip) choose them; the operands' planes are made there (k_feat_split*, split_planes*).
#include <type_traits>

#include "pcc_conv.h"

// (row tile, first column) of work id `wid` in a dense product with gy column blocks of BN.  Many column blocks (weights > L2):
// groups of 8 row tiles sweep the column blocks together, so a block's weights are fetched once per group instead of once
// per row tile (the grid covers whole groups, launch_mfma).
template <int BN>
__device__ __forceinline__ int2 dense_tile(int wid, int gy) {   // .x = row tile, .y = first column
  int tile_id, colblock;
  if (gy > 8) {
    const int g = wid / (8 * gy), rem = wid - g * 8 * gy;
    colblock = (rem >> 3) * BN;
    tile_id = g * 8 + (rem & 7);
  } else {
    tile_id = wid / gy;
    colblock = (wid - tile_id * gy) * BN;
  }
  return make_int2(tile_id, colblock);
}

// ------------------------------------------------------------------------------------------
// Dense GEMM form of the split kernel, stripped to what the products of the generative transposed convolutions need:
//   T[n, ncol] = X[n, cin] x W[cin, ncol],  cin = NCH * 32, no bias / activation / row list, 128 x 128 tiles.
// Same data flow as k_conv_mfma_bf (bf16 planes -> registers -> padded LDS images -> six MFMA terms, fp32 accumulate), but a
// tile here is only NCH = 4 chunks deep, so the fixed cost per tile decided the run time of the general kernel: with loads,
// MFMAs and stores all switched off it still took 0.77 of 2.65 ms on the level-2 products (PCC_DBG) --
// tile decode through the map header, per-chunk offset arithmetic for gathered rows, 64-bit address arithmetic for each of the
// 64 stores of a lane.  Here every address is (per-tile scalar base in a buffer descriptor) + (per-lane offset computed once)
// + (compile-time immediate or a scalar), the chunk loop is unrolled, and tail tiles take their own path.
// ------------------------------------------------------------------------------------------
template <int NCH>
__global__ void __launch_bounds__(256, 3) k_gemm_bf2(ConvArgs a) {
  constexpr int BM = 128, BN = 128, LDU = 13;
  constexpr unsigned ROWB = NCH * 192u;                // bytes of a feature row's planes
  __shared__ __attribute__((aligned(16))) uint4 As[BM * LDU];
  __shared__ __attribute__((aligned(16))) uint4 Bs[BN * LDU];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wid = xcd_work_id();
  const int gy = a.cout_pad / BN;
  const int2 tc = dense_tile<BN>(wid, gy);
  const int tile_id = tc.x, colblock = tc.y;
  const long long p0 = (long long)tile_id * BM;
  if (p0 >= a.n_out) return;
  const int npos = (int)min((long long)BM, a.n_out - p0);

  // descriptors: the tile's feature rows (rows past the end read as zero), the column block's weights, the tile's output rows
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned char*>(a.featb) + (size_t)p0 * ROWB, (short)0, (int)((unsigned)npos * ROWB), 0x00020000);
  const unsigned char* wb = reinterpret_cast<const unsigned char*>(a.wp + a.wp_elems) + (size_t)colblock * 192u;
  const unsigned b_stride = (unsigned)a.cout_pad * 192u;             // bytes between the weight planes of consecutive chunks
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned char*>(wb), (short)0, (int)((NCH - 1) * b_stride + BN * 192u), 0x00020000);

  // staging roles: 16-byte unit u = j * 256 + tid of the tile's [128 rows][12 units] piece, j = 0..5
  unsigned vA[6], ld[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const unsigned u = (unsigned)(j * 256 + tid), row = u / 12u, wu = u - row * 12u;
    vA[j] = row * ROWB + wu * 16u;
    ld[j] = row * LDU + wu;
  }
  const unsigned vB = (unsigned)tid * 16u;

  uint4 av[6], bv[6];
  auto issue = [&](int cbi) {
#pragma unroll
    for (int j = 0; j < 6; ++j)
      av[j] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsA, PCC_DBG_ON(a, 4) ? BUF_OOB : vA[j] + (unsigned)cbi * 192u, 0, 0));
#pragma unroll
    for (int j = 0; j < 6; ++j)
      bv[j] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsB, PCC_DBG_ON(a, 4) ? BUF_OOB : vB, (int)((unsigned)cbi * b_stride + (unsigned)j * 4096u), 0));
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = acc_zero();

  const int wm = w >> 1, wn = w & 1;
  const int half = lane >> 5, r31 = lane & 31;
  const unsigned fa = (unsigned)((wm * 64 + r31) * LDU + half), fb = (unsigned)((wn * 64 + r31) * LDU + half);

  issue(0);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    __syncthreads();   // previous chunk's fragment reads are done
#pragma unroll
    for (int j = 0; j < 6; ++j) As[ld[j]] = av[j];
#pragma unroll
    for (int j = 0; j < 6; ++j) Bs[ld[j]] = bv[j];
    __syncthreads();
    if (c + 1 < NCH) issue(c + 1);            // next chunk's global loads fly during this chunk's MFMAs
    __builtin_amdgcn_sched_barrier(0);
    if (PCC_DBG_ON(a, 2)) continue;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 af[3][2], bf[3][2];
#pragma unroll
      for (int p = 0; p < 3; ++p) {
#pragma unroll
        for (int i = 0; i < 2; ++i) af[p][i] = __builtin_bit_cast(bf16x8, As[fa + i * 32 * LDU + p * 4 + ks * 2]);
#pragma unroll
        for (int j = 0; j < 2; ++j) bf[p][j] = __builtin_bit_cast(bf16x8, Bs[fb + j * 32 * LDU + p * 4 + ks * 2]);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {           // smallest terms first (same order as k_conv_mfma_bf: identical results)
          // bf6_terms (pcc_mfma.h) written out: the probe hook sits between its terms
          if (!PCC_DBG_ON(a, 8)) {                  // (timing experiment: three of the six terms)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[2][i], bf[0][j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0][i], bf[2][j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[1][i], bf[1][j], acc[i][j], 0, 0, 0);
          }
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[1][i], bf[0][j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0][i], bf[1][j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0][i], bf[0][j], acc[i][j], 0, 0, 0);
        }
    }
  }
  if (PCC_DBG_ON(a, 1)) { if (acc[0][0][0] != 12345.678f) return; }

  // ---- range guard: the elements of a row / column far below its maximum are carried with an
  //      ABSOLUTE error of 2^-28 of that maximum, so a product's error can reach cin * 2^-27 * max|row| * max|column|; the
  //      scales bound the maxima (max < 2^15 / scale).  A lane's rows x a lane's columns are exactly its outputs.
  // (evaluated on the row scales the epilogue reads anyway)
  // ---- stores: element e of acc[i][j] is row wm*64 + i*32 + (e&3) + 8*(e>>2) + 4*half, column wn*64 + j*32 + r31 of the tile
  const unsigned ncol = (unsigned)a.cout;
  float* const obase = a.out + (size_t)p0 * ncol + colblock;
  const __amdgpu_buffer_rsrc_t rsO = __builtin_amdgcn_make_buffer_rsrc(
      obase, (short)0, (int)(((unsigned)(npos - 1) * ncol + min((unsigned)BN, ncol - (unsigned)colblock)) * 4u), 0x00020000);
  const unsigned vO = ((unsigned)(wm * 64 + 4 * half) * ncol + (unsigned)(wn * 64 + r31)) * 4u;
  if (npos == BM && (unsigned)colblock + BN <= ncol) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const unsigned so = (unsigned)cfrag_row(i * 32, e, 0) * ncol * 4u;      // scalar
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const float v = acc[i][j][e];          // (a bit_cast of the vector element itself compiles to element 0)
          if ((a.nt & 1) && NCH >= 2) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rsO, vO + (unsigned)j * 128u, (int)so, 2);   // non-temporal, as k_gemm_h2
          else __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rsO, vO + (unsigned)j * 128u, (int)so, 0);
        }
      }
    return;
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if ((unsigned)colblock + (unsigned)(wn * 64 + j * 32 + r31) >= ncol) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int r = cfrag_row(wm * 64 + i * 32, e, half);
        if (r >= npos) continue;
        obase[(size_t)r * ncol + (unsigned)(wn * 64 + j * 32 + r31)] = acc[i][j][e];
      }
  }
}

// (Round 3, tools/gemm_h2_probe.py + PCC_DBG on the level-2 composite shape 58 051 x 128 x 21 952, and tools/write_probe.hip:
//  the chip stores this 5.1 GB buffer in 0.90 ms at best (5.65 TB/s, this kernel's own store pattern, any occupancy); this
//  kernel takes 1.68-1.78 = LDS skeleton 0.38 + loads 0.05 + MFMA 0.27 + stores 0.56 measured one at a time, but loads + stores
//  + skeleton = 1.36 = (loads + skeleton 0.43) + (stores + skeleton 0.94): L2 reads and HBM-bound stores of one CU do not
//  overlap, whatever issues them.  Built and measured against it, bit-identical results, all slower and removed: start-up skew
//  between the workgroups of a CU (no change); a persistent LDS-DMA chunk stream (global_load_lds into a 4-slot ring three
//  chunks ahead, operands stored in HBM in the LDS image, 16-byte stores after a quad transpose): 2.17 ms with every wave
//  loading and storing (vmcnt orders a wave's stores with its loads), 2.15 ms with four loader waves and eight store-only
//  compute waves, 2.08 with nt / write-through stores; its loads + stores alone take 2.0 ms.  DESIGN.md section 8.)
// The dense products in scaled fp16 pairs (see k_feat_split_h): the structure of k_gemm_bf2 with two planes per operand
// (8 units of 16 bytes per 32-channel piece, LDS rows of 9 units: 9 is odd, so a fragment read's 16 rows fall on 16 different
// bank quads), three MFMA terms, and the row and column scales applied to the accumulators on the way out.
// TN = 2 32-column MFMA tiles per wave: the 128 x 128 workgroup tile.  Per tile the kernel reads (128 + BN) operand rows of
// NCH * 128 B from L2 for 128 * BN * 4 B of products: 2 B read per B written.
template <int NCH>
__global__ void __launch_bounds__(256, 3) k_gemm_h2(ConvArgs a) {
  constexpr int TN = 2, BM = 128, BN = 64 * TN, LDU = 9, NB = BN / 32;
  constexpr unsigned ROWB = NCH * 128u;                // bytes of a feature row's planes
  __shared__ __attribute__((aligned(16))) uint4 As[BM * LDU];
  __shared__ __attribute__((aligned(16))) uint4 Bs[BN * LDU];
  __shared__ __attribute__((aligned(16))) float rs[BM];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wid = xcd_work_id();
  const int gy = (a.cout_pad + BN - 1) / BN;
  const int2 tc = dense_tile<BN>(wid, gy);
  const int tile_id = tc.x, colblock = tc.y;
  const long long p0 = (long long)tile_id * BM;
  if (p0 >= a.n_out) return;
  const int npos = (int)min((long long)BM, a.n_out - p0);

  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned char*>(a.feath) + (size_t)p0 * ROWB, (short)0, (int)((unsigned)npos * ROWB), 0x00020000);
  const float* const wplanes = a.wp + a.wp_elems + bf_plane_elems(a.wp_elems);      // fp16 planes behind the bf16 planes
  const unsigned char* wb = reinterpret_cast<const unsigned char*>(wplanes) + (size_t)colblock * 128u;
  const float* const cinv = wplanes + a.wp_elems;                                    // [cout_pad] column 1/scale
  const unsigned b_stride = (unsigned)a.cout_pad * 128u;
  const int bcols = min(BN, a.cout_pad - colblock);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned char*>(wb), (short)0, (int)((NCH - 1) * b_stride + (unsigned)bcols * 128u), 0x00020000);

  unsigned vA[4], ld[NB];
#pragma unroll
  for (int j = 0; j < 4; ++j) vA[j] = (unsigned)((j * 256 + tid) >> 3) * ROWB + (unsigned)(tid & 7) * 16u;
#pragma unroll
  for (int j = 0; j < NB; ++j) ld[j] = (unsigned)((j * 256 + tid) >> 3) * LDU + (unsigned)(tid & 7);
  // column (tid >> 3) + 32 j of the block; columns past cout_pad read zeros
  unsigned vB[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) vB[j] = ((tid >> 3) + 32 * j < bcols) ? (unsigned)tid * 16u + (unsigned)j * 4096u : BUF_OOB;

  uint4 av[4], bv[NB];
  auto issue = [&](int cbi) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      av[j] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsA, PCC_DBG_ON(a, 4) ? BUF_OOB : vA[j] + (unsigned)cbi * 128u, 0, 0));
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      bv[j] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsB, PCC_DBG_ON(a, 4) ? BUF_OOB : vB[0], (int)((unsigned)cbi * b_stride + (unsigned)j * 4096u), 0));
    }
  };

  f32x16 acc[2][TN];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = acc_zero();

  const int wm = w >> 1, wn = w & 1;
  const int half = lane >> 5, r31 = lane & 31;
  const unsigned fa = (unsigned)((wm * 64 + r31) * LDU + half), fb = (unsigned)((wn * 32 * TN + r31) * LDU + half);

  issue(0);
  if (tid < BM) rs[tid] = tid < npos ? a.frow_inv[p0 + tid] : 0.f;
  float cs[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = colblock + wn * 32 * TN + j * 32 + r31;
    cs[j] = col < a.cout_pad ? cinv[col] : 0.f;
  }
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    __syncthreads();   // previous chunk's fragment reads are done
#pragma unroll
    for (int j = 0; j < 4; ++j) As[ld[j]] = av[j];
#pragma unroll
    for (int j = 0; j < NB; ++j) Bs[ld[j]] = bv[j];
    __syncthreads();
    if (c + 1 < NCH) issue(c + 1);            // next chunk's global loads fly during this chunk's MFMAs
    __builtin_amdgcn_sched_barrier(0);
    if (PCC_DBG_ON(a, 2)) continue;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      f16x8 af[2][2], bf[2][TN];
#pragma unroll
      for (int p = 0; p < 2; ++p) {
#pragma unroll
        for (int i = 0; i < 2; ++i) af[p][i] = __builtin_bit_cast(f16x8, As[fa + i * 32 * LDU + p * 4 + ks * 2]);
#pragma unroll
        for (int j = 0; j < TN; ++j) bf[p][j] = __builtin_bit_cast(f16x8, Bs[fb + j * 32 * LDU + p * 4 + ks * 2]);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {           // small terms first
          acc[i][j] = h3_terms(af[0][i], af[1][i], bf[0][j], bf[1][j], acc[i][j]);
        }
    }
  }
  if (PCC_DBG_ON(a, 1)) { if (acc[0][0][0] != 12345.678f) return; }

  // ---- stores: element e of acc[i][j] is row wm*64 + i*32 + (e&3) + 8*(e>>2) + 4*half, column wn*32*TN + j*32 + r31 of the tile
  const unsigned ncol = (unsigned)a.cout;
  float* const obase = a.out + (size_t)p0 * ncol + colblock;
  const __amdgpu_buffer_rsrc_t rsO = __builtin_amdgcn_make_buffer_rsrc(
      obase, (short)0, (int)(((unsigned)(npos - 1) * ncol + min((unsigned)BN, ncol - (unsigned)colblock)) * 4u), 0x00020000);
  const unsigned vO = ((unsigned)(wm * 64 + 4 * half) * ncol + (unsigned)(wn * 32 * TN + r31)) * 4u;
  const bool full = npos == BM && (unsigned)colblock + BN <= ncol;
  // The product buffer is written once and read back by the gather-sum long after it left the caches (5 GB per level):
  // non-temporal stores keep it from evicting the operands this kernel re-reads from L2 (round 3: 3.4 -> 4.2 TB/s of
  // algorithmic traffic on the composite levels, decode -0.6 ms; PCC_NT bit 0).
  // (32-deep products have hardly any operand to protect, and as a pure stream non-temporal stores are the slower ones --
  //  4.2 against 5.0 TB/s, tools/gemm_nt_probe.sh: the hint is taken from 64 input channels on; PCC_NT bit 6 forces it.)
  const bool nt = (a.nt & 1) != 0 && (NCH >= 2 || (a.nt & 64));
  // The scaled store below (row scales from LDS, rr * cs, nt / plain / out-of-range buffer stores, range guard) is mirrored by
  // k_pair_h2, kept in step by hand: one function template over acc[2][TN] and cs[TN] changed all ten instantiations of the two.
  const int row_lim = npos - wm * 64 - 4 * half;
  const int col_lim = (int)ncol - colblock - wn * 32 * TN - r31;
  float guard_mr = 0.f, guard_mc = 0.f;
#pragma unroll
  for (int j = 0; j < TN; ++j) guard_mc = fmaxf(guard_mc, cs[j]);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int e4 = 0; e4 < 4; ++e4) {
      const float4 r4 = *reinterpret_cast<const float4*>(&rs[wm * 64 + i * 32 + 8 * e4 + 4 * half]);
      const float rr[4] = {r4.x, r4.y, r4.z, r4.w};
      guard_mr = fmaxf(guard_mr, fmaxf(fmaxf(r4.x, r4.y), fmaxf(r4.z, r4.w)));
#pragma unroll
      for (int e1 = 0; e1 < 4; ++e1) {
        const int e = e4 * 4 + e1;
        const int rrow = i * 32 + e1 + 8 * e4;
        const unsigned so = (unsigned)rrow * ncol * 4u;      // scalar
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const float v = acc[i][j][e] * (rr[e1] * cs[j]);
          if (full && nt) {
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rsO, vO + (unsigned)j * 128u, (int)so, 2);
          } else if (full) {
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rsO, vO + (unsigned)j * 128u, (int)so, 0);
          } else {                                           // last row tile / column block: invalid elements go out of range
            const unsigned off = (rrow < row_lim && j * 32 < col_lim) ? vO + (unsigned)j * 128u + so : BUF_OOB;
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rsO, off, 0, 0);
          }
        }
      }
    }
  // range guard: elements of a row / column far below its maximum are carried with an ABSOLUTE error of
  // 2^-28 of that maximum, so a product's error can reach cin * 2^-27 * max|row| * max|column|; the scales bound the maxima
  // (max < 2^15 / scale).  A lane's rows x a lane's columns are exactly its outputs.
  if (a.guard && guard_mr * guard_mc * (8.f * (float)a.cin) > a.guard_lim) atomicOr(a.guard, 1);
}

// The gathered pair GEMM (pcc_conv_fwd_pairs, pcc_convt_fwd_rows: one kernel offset per 128-pair tile, T[pair] = x[in(pair)] W[k])
// in the scaled fp16 form of k_gemm_h2: a pair's product row is scaled like its input row, the weights per (offset, column).
template <int NCH>
__global__ void __launch_bounds__(256, 3) k_pair_h2(ConvArgs a) {
  constexpr int BM = 128, BN = 128, LDU = 9;
  constexpr unsigned ROWB = NCH * 128u;
  __shared__ __attribute__((aligned(16))) uint4 As[BM * LDU];
  __shared__ __attribute__((aligned(16))) uint4 Bs[BN * LDU];
  __shared__ __attribute__((aligned(16))) float rs[BM];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wid = xcd_work_id();
  const int gy = a.cout_pad / BN;
  const int tile_id = wid / gy;
  const int colblock = (wid - tile_id * gy) * BN;
  if (tile_id >= *a.n_tiles) return;
  const long long p0 = (long long)tile_id * BM;
  const int kid = a.tile_k[tile_id];

  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned char*>(a.feath), (short)0, (int)(unsigned)((size_t)a.n_in * ROWB), 0x00020000);
  const float* const wplanes = a.wp + a.wp_elems + bf_plane_elems(a.wp_elems);
  const unsigned char* wb = reinterpret_cast<const unsigned char*>(wplanes) + ((size_t)kid * NCH * a.cout_pad + colblock) * 128u;
  const float* const cinv = wplanes + a.wp_elems + (size_t)kid * a.cout_pad;
  const unsigned b_stride = (unsigned)a.cout_pad * 128u;
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned char*>(wb), (short)0, (int)((NCH - 1) * b_stride + BN * 128u), 0x00020000);

  unsigned vA[4], ld[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned u = (unsigned)(j * 256 + tid), row = u >> 3, wu = u & 7u;
    const int g = a.pair_in[p0 + row];                                       // input row of the pair (-1: padding, reads zeros)
    vA[j] = g >= 0 ? (unsigned)g * ROWB + wu * 16u : BUF_OOB;
    ld[j] = row * LDU + wu;
  }
  const unsigned vB = (unsigned)tid * 16u;

  uint4 av[4], bv[4];
  auto issue = [&](int cbi) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      av[j] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsA, vA[j] == BUF_OOB ? BUF_OOB : vA[j] + (unsigned)cbi * 128u, 0, 0));
#pragma unroll
    for (int j = 0; j < 4; ++j)
      bv[j] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsB, vB, (int)((unsigned)cbi * b_stride + (unsigned)j * 4096u), 0));
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = acc_zero();

  const int wm = w >> 1, wn = w & 1;
  const int half = lane >> 5, r31 = lane & 31;
  const unsigned fa = (unsigned)((wm * 64 + r31) * LDU + half), fb = (unsigned)((wn * 64 + r31) * LDU + half);

  issue(0);
  if (tid < BM) {
    const int g = a.pair_in[p0 + tid];
    rs[tid] = g >= 0 ? a.frow_inv[g] : 0.f;
  }
  float cs[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) cs[j] = cinv[colblock + wn * 64 + j * 32 + r31];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) As[ld[j]] = av[j];
#pragma unroll
    for (int j = 0; j < 4; ++j) Bs[ld[j]] = bv[j];
    __syncthreads();
    if (c + 1 < NCH) issue(c + 1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      f16x8 af[2][2], bf[2][2];
#pragma unroll
      for (int p = 0; p < 2; ++p) {
#pragma unroll
        for (int i = 0; i < 2; ++i) af[p][i] = __builtin_bit_cast(f16x8, As[fa + i * 32 * LDU + p * 4 + ks * 2]);
#pragma unroll
        for (int j = 0; j < 2; ++j) bf[p][j] = __builtin_bit_cast(f16x8, Bs[fb + j * 32 * LDU + p * 4 + ks * 2]);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          acc[i][j] = h3_terms(af[0][i], af[1][i], bf[0][j], bf[1][j], acc[i][j]);
        }
    }
  }
  // ---- stores: the tile's 128 product rows are consecutive rows of T (padding pairs included: they are zero).  The scaled store
  //      of k_gemm_h2 without its row check, kept in step with it by hand (see there)
  const unsigned ncol = (unsigned)a.cout;
  float* const obase = a.out + (size_t)p0 * ncol + colblock;
  const __amdgpu_buffer_rsrc_t rsO = __builtin_amdgcn_make_buffer_rsrc(
      obase, (short)0, (int)(((unsigned)(BM - 1) * ncol + min((unsigned)BN, ncol - (unsigned)colblock)) * 4u), 0x00020000);
  const unsigned vO = ((unsigned)(wm * 64 + 4 * half) * ncol + (unsigned)(wn * 64 + r31)) * 4u;
  const bool full = (unsigned)colblock + BN <= ncol;
  const int col_lim = (int)ncol - colblock - wn * 64 - r31;
  float guard_mr = 0.f;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int e4 = 0; e4 < 4; ++e4) {
      const float4 r4 = *reinterpret_cast<const float4*>(&rs[wm * 64 + i * 32 + 8 * e4 + 4 * half]);
      const float rr[4] = {r4.x, r4.y, r4.z, r4.w};
      guard_mr = fmaxf(guard_mr, fmaxf(fmaxf(r4.x, r4.y), fmaxf(r4.z, r4.w)));
#pragma unroll
      for (int e1 = 0; e1 < 4; ++e1) {
        const int e = e4 * 4 + e1;
        const unsigned so = (unsigned)(i * 32 + e1 + 8 * e4) * ncol * 4u;      // scalar
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const float v = acc[i][j][e] * (rr[e1] * cs[j]);
          if (full && (a.nt & 2)) {
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rsO, vO + (unsigned)j * 128u, (int)so, 2);
          } else if (full) {
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rsO, vO + (unsigned)j * 128u, (int)so, 0);
          } else {
            const unsigned off = (j * 32 < col_lim) ? vO + (unsigned)j * 128u + so : BUF_OOB;
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rsO, off, 0, 0);
          }
        }
      }
    }
  if (a.guard && guard_mr * fmaxf(cs[0], cs[1]) * (8.f * (float)a.cin) > a.guard_lim) atomicOr(a.guard, 1);   // range guard, as in k_gemm_h2
}

// the chunk counts NCH = cin / 32 the unrolled products (k_gemm_bf2, k_gemm_h2, k_pair_h2) are built for
bool nch_ok(int nch) { return nch == 1 || nch == 2 || nch == 4 || nch == 6 || nch == 8; }
// f(integral_constant<NCH>) for the chunk count nch, one of nch_ok()
template <typename F>
static void with_nch(int nch, F f) {
  switch (nch) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    default: f(std::integral_constant<int, 8>{}); break;
  }
}

int launch_gemm_bf2(const ConvArgs& a, dim3 grid, hipStream_t s) {
  with_nch(a.ppo, [&](auto nch) { k_gemm_bf2<decltype(nch)::value><<<grid, 256, 0, s>>>(a); });
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}
int launch_gemm_h2(const ConvArgs& a, dim3 grid, hipStream_t s) {
  with_nch(a.ppo, [&](auto nch) { k_gemm_h2<decltype(nch)::value><<<grid, 256, 0, s>>>(a); });
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}
int launch_pair_h2(const ConvArgs& a, dim3 grid, hipStream_t s) {
  with_nch(a.ppo, [&](auto nch) { k_pair_h2<decltype(nch)::value><<<grid, 256, 0, s>>>(a); });
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}
