// The general MFMA convolution on three bf16 planes per fp32 operand (k_conv_mfma_bf; the split path is described above
// k_split_packed in pcc_conv.hip) and its launcher.
#include "pcc_conv.h"

// (launch bounds: the 128 x 128 tile needs ~240 registers; capped at 168 for three workgroups per CU it spilled 96 bytes per
//  thread and reloaded loop-invariant offsets inside the chunk loop.  With two workgroups per CU nothing spills; measured equal
//  (282 against 287 us on the last hyper-synthesis layer: that launch is bound by its L2 operand traffic).)
template <int WM, int WN, int TM, int TN, int MODE, int MINWG = (TM * TN >= 4 ? 2 : 3)>
__global__ void __launch_bounds__(256, MINWG) k_conv_mfma_bf(ConvArgs a) {
  constexpr int BM = WM * TM * 32;
  constexpr int BN = WN * TN * 32;
  static_assert(WM * WN == 4, "4 waves per workgroup");
  static_assert(BN <= 128 && BM <= 128, "one feature row and one weight row per thread (pair)");
  // LDS images [row][13 x 16 B]: the 12 units (plane, slot) of a row's 192-byte piece plus one unit of padding.  Staging
  // writes go 8 consecutive units at a time (contiguous), a fragment read takes one unit of 16 different rows: row * 52
  // dwords mod 64 is a permutation of the bank quads over the rows of any ds_read_b128 lane group.  Conflict-free both ways.
  constexpr int LDU = 13;
  __shared__ __attribute__((aligned(16))) uint4 As[BM * LDU];
  __shared__ __attribute__((aligned(16))) uint4 Bs[BN * LDU];
  __shared__ unsigned char act_flag[MAXK];
  __shared__ unsigned char act_list[MAXK];
  __shared__ unsigned char act_kid[MAXK];
  __shared__ int s_nact;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int wid = xcd_work_id();
  const int ks_id = wid % a.ksplit;                   // which slice of the reduction (ksplit == 1: the whole of it)
  wid /= a.ksplit;
  const int gy = a.cout_pad / BN;
  int tile_id = wid / gy;
  int colblock = (wid - tile_id * gy) * BN;
  if (a.hdr == nullptr && a.pair_in == nullptr && gy > 8) {
    // dense GEMM with many column blocks (generative transposed convs: [n_in, cin] x [cin, K*cout], weights > L2):
    // groups of 8 row tiles sweep the column blocks together, so a block's weights are fetched once per group instead of
    // once per row tile (the grid covers whole groups, launch_mfma)
    const int g = wid / (8 * gy), rem = wid - g * 8 * gy;
    colblock = (rem >> 3) * BN;
    tile_id = g * 8 + (rem & 7);
  }

  // locate (segment, tile) and compact the active offsets: the passage of k_conv_mfma, kept in step with it by hand (as one
  // shared function, by reference or by value, it changed the instructions of every instantiation of both kernels)
  int pos0, npos, k_count, koff_begin;
  long long seg_pos_count;
  const int* seg_nbr = nullptr;
  const bool pair_mode = (a.pair_in != nullptr);
  const bool identity = (a.hdr == nullptr) && !pair_mode;
  if (pair_mode) {
    if (tile_id >= *a.n_tiles) return;
    pos0 = tile_id * BM; npos = BM; k_count = 1; koff_begin = 0; seg_pos_count = 0;
    seg_nbr = a.pair_in + pos0;
  } else if (identity) {
    const long long p0 = (long long)tile_id * BM;
    if (p0 >= a.n_out) return;
    pos0 = (int)p0;
    npos = (int)min((long long)BM, a.n_out - p0);
    k_count = 1; koff_begin = 0; seg_pos_count = a.n_out;
  } else {
    const int nseg = a.hdr[HDR_NSEG];
    int tile = tile_id, sgi = 0;
    bool found = false;
    int pb = 0, pc = 0;
    for (; sgi < nseg; ++sgi) {
      const int* sg = a.hdr + HDR_SEG0 + sgi * SEG_WORDS;
      pb = sg[SEG_POS_BEGIN]; pc = sg[SEG_POS_COUNT];
      const int tiles = (pc + BM - 1) / BM;
      if (tile < tiles) { found = true; break; }
      tile -= tiles;
    }
    if (!found) return;
    const int* sg = a.hdr + HDR_SEG0 + sgi * SEG_WORDS;
    k_count = sg[SEG_K_COUNT];
    koff_begin = sg[SEG_KOFF_BEGIN];
    const long long nb = ((long long)(unsigned)sg[SEG_NBR_LO]) | ((long long)sg[SEG_NBR_HI] << 32);
    seg_nbr = a.nbr + nb;
    seg_pos_count = pc;
    const int local0 = tile * BM;
    pos0 = pb + local0;
    npos = min(BM, pc - local0);
    seg_nbr += local0;
  }

  if (pair_mode) {
    if (tid == 0) { act_list[0] = 0; act_kid[0] = (unsigned char)a.tile_k[tile_id]; s_nact = 1; }
  } else if (identity) {
    if (tid == 0) { act_list[0] = 0; act_kid[0] = 0; s_nact = 1; }
  } else {
    for (int j = w; j < k_count; j += 4) {
      bool any = false;
      for (int r = lane; r < npos; r += 64) any |= (seg_nbr[(long long)j * seg_pos_count + r] >= 0);
      const unsigned long long mk = __ballot(any);
      if (lane == 0) act_flag[j] = mk ? 1 : 0;
    }
    __syncthreads();
    if (w == 0) {
      int nn = 0;
      for (int j0 = 0; j0 < k_count; j0 += 64) {
        const int u = j0 + lane;
        const int j = (u < k_count) ? a.hdr[HDR_ORDER + koff_begin + u] : 0;
        const bool f = (u < k_count) && act_flag[j];
        const unsigned long long mk = __ballot(f);
        if (f) {
          const int p = nn + __popcll(mk & ((1ull << lane) - 1ull));
          act_list[p] = (unsigned char)j;
          act_kid[p] = (unsigned char)a.hdr[HDR_KOFFS + koff_begin + j];
        }
        nn += __popcll(mk);
      }
      if (lane == 0) s_nact = nn;
    }
  }
  __syncthreads();
  const int nact = s_nact;
  const int nchunks_all = nact * a.ppo;               // CB = 32: one piece per chunk
  // split-K: slice ks_id takes the chunks [c_lo, c_hi) (contiguous: whole offsets stay together as far as possible)
  const int c_lo = (int)((long long)nchunks_all * ks_id / a.ksplit), c_hi = (int)((long long)nchunks_all * (ks_id + 1) / a.ksplit);
  const int nchunks = c_hi - c_lo;

  // staging roles: the 16-byte units u = j * 256 + tid of the tile's piece, 12 per row (3 planes x 4 slots), rows contiguous:
  // consecutive lanes read consecutive 16-byte units of a feature / weight row (coalesced), and write them side by side
  constexpr int NA = (BM * 12 + 255) / 256, NB = (BN * 12 + 255) / 256;
  int a_row[NA], a_w[NA], b_row[NB], b_w[NB];
#pragma unroll
  for (int j = 0; j < NA; ++j) stage_role(j * 256 + tid, BM, a_row[j], a_w[j]);
#pragma unroll
  for (int j = 0; j < NB; ++j) stage_role(j * 256 + tid, BN, b_row[j], b_w[j]);

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;   // acc_zero() (pcc_mfma.h) written out: it costs the 128 x 128 tile 5 instructions

  const int wm = w / WN, wn = w % WN;
  const int half = lane >> 5, r31 = lane & 31;

  const unsigned row_bytes = (unsigned)a.cin * 6u;    // [cin/32][3][32] bf16
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned char*>(a.featb), (short)0, (int)(unsigned)((size_t)a.n_in * row_bytes), 0x00020000);
  const float* wb = a.wp + a.wp_elems;                // bf16 planes behind the fp32 image: [piece][cout_pad][3][32] bf16
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(wb), (short)0, (int)(unsigned)((size_t)bf_plane_elems(a.wp_elems) * 4), 0x00020000);

  auto load_rows = [&](int ai, int (&rows)[NA]) {
    const int slot = act_list[ai];
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      const int rc = min(max(a_row[j], 0), npos - 1);          // tail rows repeat the tile's last row (never stored)
      rows[j] = identity ? (pos0 + rc) : seg_nbr[(long long)slot * seg_pos_count + rc];
      if (a_row[j] < 0) rows[j] = -1;
    }
  };
  auto issue = [&](int ai, int cbi, const int (&rows)[NA], uint4 (&av)[NA], uint4 (&bv)[NB]) {
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      const unsigned off = rows[j] >= 0 ? (unsigned)rows[j] * row_bytes + (unsigned)cbi * 192u + (unsigned)a_w[j] * 16u : BUF_OOB;
      av[j] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsA, PCC_DBG_ON(a, 4) ? BUF_OOB : off, 0, 0));
    }
    const unsigned wbase = (unsigned)((act_kid[ai] * a.ppo + cbi) * a.cout_pad + colblock) * 192u;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const unsigned off = b_row[j] >= 0 ? wbase + (unsigned)(j * 256 + tid) * 16u : BUF_OOB;
      bv[j] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsB, PCC_DBG_ON(a, 4) ? BUF_OOB : off, 0, 0));
    }
  };

  int rows_cur[NA], rows_nxt[NA];
  uint4 av[NA], bv[NB];
  int ai_c = 0, cbi_c = 0, ai_n = 0, cbi_n = 0;
  if (nchunks > 0) {
    ai_c = c_lo / a.ppo; cbi_c = c_lo - ai_c * a.ppo;
    load_rows(ai_c, rows_cur);
    issue(ai_c, cbi_c, rows_cur, av, bv);
    if (nchunks > 1) {
      ai_n = (c_lo + 1) / a.ppo; cbi_n = (c_lo + 1) - ai_n * a.ppo;
      if (ai_n != ai_c) load_rows(ai_n, rows_nxt);
      else {
#pragma unroll
        for (int j = 0; j < NA; ++j) rows_nxt[j] = rows_cur[j];
      }
    }
  }

  for (int c = 0; c < nchunks; ++c) {
    __syncthreads();   // previous chunk's fragment reads are done
#pragma unroll
    for (int j = 0; j < NA; ++j)
      if (a_row[j] >= 0) As[a_row[j] * LDU + a_w[j]] = av[j];
#pragma unroll
    for (int j = 0; j < NB; ++j)
      if (b_row[j] >= 0) Bs[b_row[j] * LDU + b_w[j]] = bv[j];
    __syncthreads();
    if (c + 1 < nchunks) {          // next chunk's global loads fly during this chunk's MFMAs
#pragma unroll
      for (int j = 0; j < NA; ++j) rows_cur[j] = rows_nxt[j];
      ai_c = ai_n; cbi_c = cbi_n;
      issue(ai_c, cbi_c, rows_cur, av, bv);
      if (c + 2 < nchunks) {
        ai_n = (c_lo + c + 2) / a.ppo; cbi_n = (c_lo + c + 2) - ai_n * a.ppo;
        if (ai_n != ai_c) load_rows(ai_n, rows_nxt);
      }
    }
    __builtin_amdgcn_sched_barrier(0);   // keep the prefetch ahead of the MFMAs, not next to its use
    if (PCC_DBG_ON(a, 2)) continue;
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

  if (PCC_DBG_ON(a, 1)) { if (acc[0][0][0] != 12345.678f) return; }
  if (a.ksplit > 1) {                                 // raw partial sums; bias / activation are applied by k_splitk_reduce
    // (the indexing of the epilogue's general loop below)
    float* const part = a.part + (size_t)ks_id * (size_t)a.n_out * a.cout;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = colblock + (wn * TN + j) * 32 + r31;
      if (col >= a.cout) continue;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int r = cfrag_row((wm * TM + i) * 32, e, half);
          if (r >= npos) continue;
          const long long orow = a.rows ? a.rows[pos0 + r] : (pos0 + r);
          part[orow * a.cout + col] = acc[i][j][e];
        }
    }
    return;
  }
  // ---- epilogue: bias, activation (or GDN), store: the epilogue of k_conv_mfma, kept in step with it by hand (a shared function
  //      over the accumulator array changed the instructions of both kernels, whatever the form of its other arguments)
  if (!a.rows && npos == BM) {
    const size_t lane_off = (size_t)(pos0 + wm * TM * 32 + 4 * half) * a.cout + colblock + wn * TN * 32 + r31;
    float* const lane_out = a.out + lane_off;
    const float* const lane_x = a.feat + lane_off;             // GDN / IGDN: cin == cout, same element of the input
    auto store_tile = [&](auto actf) {
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int col = colblock + (wn * TN + j) * 32 + r31;
        if (col >= a.cout) continue;
        const float b = a.bias ? a.bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const size_t o = (size_t)cfrag_row(i * 32, e, 0) * a.cout + j * 32;
            lane_out[o] = actf(acc[i][j][e] + b, o);
          }
      }
    };
    if (MODE == MODE_GDN) store_tile([&](float v, size_t o) { return lane_x[o] / v; });
    else if (MODE == MODE_IGDN) store_tile([&](float v, size_t o) { return lane_x[o] * v; });
    else if (a.act == PCC_ACT_RELU) store_tile([](float v, size_t) { return fmaxf(v, 0.f); });
    else if (a.act == PCC_ACT_LEAKY) { const float sl = a.slope; store_tile([sl](float v, size_t) { return v >= 0.f ? v : v * sl; }); }
    else store_tile([](float v, size_t) { return v; });
    return;
  }
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = colblock + (wn * TN + j) * 32 + r31;
    if (col >= a.cout) continue;
    const float b = a.bias ? a.bias[col] : 0.f;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int r = cfrag_row((wm * TM + i) * 32, e, half);
        if (r >= npos) continue;
        const long long orow = a.rows ? a.rows[pos0 + r] : (pos0 + r);
        float v = acc[i][j][e] + b;
        if (MODE == MODE_CONV) {
          if (a.act == PCC_ACT_RELU) v = fmaxf(v, 0.f);
          else if (a.act == PCC_ACT_LEAKY) v = v >= 0.f ? v : v * a.slope;
        } else {
          const float x = a.feat[orow * a.cin + col];
          v = (MODE == MODE_GDN) ? x / v : x * v;
        }
        a.out[orow * a.cout + col] = v;
      }
    }
  }
}

// The instantiations of k_conv_mfma_bf: the six tiles of launch_mfma in its three modes (launch_pair_product takes three of
// them).  Tile choice and grid are the caller's.
int launch_conv_bf(int mode, int wm, int wn, int tm, int tn, const ConvArgs& a, dim3 grid, hipStream_t s) {
#define PCC_BF_TILE(MODE, WM, WN, TM, TN)                                                        \
  if (mode == MODE && wm == WM && wn == WN && tm == TM && tn == TN) {                            \
    k_conv_mfma_bf<WM, WN, TM, TN, MODE><<<grid, 256, 0, s>>>(a);                                \
    return PCC_OK;                                                                               \
  }
#define PCC_BF_MODES(WM, WN, TM, TN)                                                             \
  PCC_BF_TILE(MODE_CONV, WM, WN, TM, TN) PCC_BF_TILE(MODE_GDN, WM, WN, TM, TN) PCC_BF_TILE(MODE_IGDN, WM, WN, TM, TN)
  PCC_BF_MODES(2, 2, 2, 2)
  PCC_BF_MODES(2, 2, 1, 2)
  PCC_BF_MODES(1, 4, 1, 1)
  PCC_BF_MODES(2, 2, 2, 1)
  PCC_BF_MODES(2, 2, 1, 1)
  PCC_BF_MODES(4, 1, 1, 1)
#undef PCC_BF_MODES
#undef PCC_BF_TILE
  PCC_REQUIRE(false, "launch_conv_bf: no kernel for mode %d, tile %d x %d waves of %d x %d fragments", mode, wm, wn, tm, tn);
  return PCC_EINVAL;
}
