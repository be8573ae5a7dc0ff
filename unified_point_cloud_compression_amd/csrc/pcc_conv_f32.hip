// The general MFMA convolution on fp32 operands (k_conv_mfma; the file comment of pcc_conv.hip describes it) and its launcher.
#include "pcc_conv.h"

static constexpr int LDS_LD = 36;   // floats per LDS tile row: 32 + 4 pad

template <int WM, int WN, int TM, int TN, int MODE, bool BUF>
__global__ void __launch_bounds__(256) k_conv_mfma(ConvArgs a) {
  constexpr int BM = WM * TM * 32;
  constexpr int BN = WN * TN * 32;
  static_assert(WM * WN == 4, "4 waves per workgroup");
  __shared__ __attribute__((aligned(16))) float As[BM * LDS_LD];
  __shared__ __attribute__((aligned(16))) float Bs[BN * LDS_LD];
  __shared__ unsigned char act_flag[MAXK];
  __shared__ unsigned char act_list[MAXK];   // segment-local offset slot
  __shared__ unsigned char act_kid[MAXK];    // kernel offset id (weight index)
  __shared__ int s_nact;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;

  const int wid = xcd_work_id();
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

  // ---- locate (segment, tile) --------------------------------------------------------------
  int pos0, npos, k_count, koff_begin;
  long long seg_pos_count;
  const int* seg_nbr = nullptr;
  const bool pair_mode = (a.pair_in != nullptr);
  bool identity = (a.hdr == nullptr) && !pair_mode;
  if (pair_mode) {          // one kernel offset per tile, rows = compacted pairs of that offset
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
    int tile = tile_id, s = 0;
    bool found = false;
    int pb = 0, pc = 0;
    for (; s < nseg; ++s) {
      const int* sg = a.hdr + HDR_SEG0 + s * SEG_WORDS;
      pb = sg[SEG_POS_BEGIN]; pc = sg[SEG_POS_COUNT];
      const int tiles = (pc + BM - 1) / BM;
      if (tile < tiles) { found = true; break; }
      tile -= tiles;
    }
    if (!found) return;   // grid is an upper bound on the tile count
    const int* sg = a.hdr + HDR_SEG0 + s * SEG_WORDS;
    k_count = sg[SEG_K_COUNT];
    koff_begin = sg[SEG_KOFF_BEGIN];
    const long long nb = ((long long)(unsigned)sg[SEG_NBR_LO]) | ((long long)sg[SEG_NBR_HI] << 32);
    seg_nbr = a.nbr + nb;
    seg_pos_count = pc;
    const int local0 = tile * BM;
    pos0 = pb + local0;
    npos = min(BM, pc - local0);
    seg_nbr += local0;     // seg_nbr[j * seg_pos_count + r] = input row of tile row r for slot j
  }

  // ---- active offsets of this tile ---------------------------------------------------------
  if (pair_mode) {
    if (tid == 0) { act_list[0] = 0; act_kid[0] = (unsigned char)a.tile_k[tile_id]; s_nact = 1; }
  } else if (identity) {
    if (tid == 0) { act_list[0] = 0; act_kid[0] = 0; s_nact = 1; }
  } else {
    for (int j = w; j < k_count; j += 4) {
      bool any = false;
      for (int r = lane; r < npos; r += 64) any |= (seg_nbr[(long long)j * seg_pos_count + r] >= 0);
      const unsigned long long m = __ballot(any);
      if (lane == 0) act_flag[j] = m ? 1 : 0;
    }
    __syncthreads();
    if (w == 0) {
      int n = 0;
      for (int j0 = 0; j0 < k_count; j0 += 64) {
        const int u = j0 + lane;                                          // visiting position -> slot
        const int j = (u < k_count) ? a.hdr[HDR_ORDER + koff_begin + u] : 0;
        const bool f = (u < k_count) && act_flag[j];
        const unsigned long long m = __ballot(f);
        if (f) {
          const int p = n + __popcll(m & ((1ull << lane) - 1ull));
          act_list[p] = (unsigned char)j;
          act_kid[p] = (unsigned char)a.hdr[HDR_KOFFS + koff_begin + j];
        }
        n += __popcll(m);
      }
      if (lane == 0) s_nact = n;
    }
  }
  __syncthreads();
  const int nact = s_nact;

  const int CB = 1 << a.cb_log2;
  const int ppc_log2 = 5 - a.cb_log2;                 // pieces per 32-wide chunk
  const int npieces = nact * a.ppo;
  const int nchunks = (npieces + (1 << ppc_log2) - 1) >> ppc_log2;

  // staging role of this thread: 16-byte part `part` of tile rows r0 + 32*i
  const int part = tid & 7;
  const int r0 = tid >> 3;
  const int kk0 = part * 4;
  const int piece_in_chunk = kk0 >> a.cb_log2;
  const int within = kk0 & (CB - 1);
  constexpr int AI = BM / 32, BI = BN / 32;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = acc_zero();

  const int wm = w / WN, wn = w % WN;
  const int half = lane >> 5, r31 = lane & 31;

  // ---- software pipeline over the 32-wide chunks -------------------------------------------------
  //   neighbour rows of chunk c+2  -> registers   (dependent-load chain hidden two chunks ahead)
  //   global loads  of chunk c+1  -> registers   (in flight while chunk c is multiplied)
  //   chunk c: registers -> LDS -> fragments -> MFMA
  auto chunk_ids = [&](int c, int& ai, int& cbi, bool& pvalid) {
    const int piece = (c << ppc_log2) + piece_in_chunk;
    ai = piece / a.ppo;            // active-offset index of my 16-byte part
    cbi = piece - ai * a.ppo;      // channel block within the offset
    pvalid = ai < nact;
  };
  __amdgpu_buffer_rsrc_t rsA, rsB;
  if constexpr (BUF) {
    rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.feat), (short)0,
                                            (int)(unsigned)((size_t)a.n_in * a.cin * 4), 0x00020000);
    rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wp), (short)0, (int)(unsigned)((size_t)a.wp_elems * 4),
                                            0x00020000);
  }
  const unsigned cin_bytes = (unsigned)a.cin * 4u;
  auto load_rows = [&](int ai, bool pvalid, int (&rows)[AI]) {
    const int slot = pvalid ? act_list[ai] : 0;
#pragma unroll
    for (int i = 0; i < AI; ++i) {
      const int r = r0 + 32 * i;
      if constexpr (BUF) {         // tail rows repeat the tile's last row (never stored); !pvalid is handled in issue()
        const int rc = min(r, npos - 1);
        rows[i] = identity ? (pos0 + rc) : seg_nbr[(long long)slot * seg_pos_count + rc];
      } else {
        int v = -1;
        if (pvalid && r < npos) v = identity ? (pos0 + r) : seg_nbr[(long long)slot * seg_pos_count + r];
        rows[i] = v;
      }
    }
  };
  auto issue = [&](int ai, int cbi, bool pvalid, const int (&rows)[AI], float4 (&av)[AI], float4 (&bv)[BI]) {
    if constexpr (BUF) {
      const unsigned cb_off = (unsigned)(((cbi << a.cb_log2) + within) * 4);
#pragma unroll
      for (int i = 0; i < AI; ++i) {
        const unsigned off = (rows[i] >= 0 && pvalid) ? (unsigned)rows[i] * cin_bytes + cb_off : BUF_OOB;
        av[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsA, off, 0, 0));
      }
      const unsigned wbase = pvalid ? (unsigned)((act_kid[ai] * a.ppo + cbi) * a.cout_pad + colblock + r0) : 0u;
#pragma unroll
      for (int i = 0; i < BI; ++i) {
        const unsigned off = pvalid ? (((wbase + 32u * i) << a.cb_log2) + within) * 4u : BUF_OOB;
        bv[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsB, off, 0, 0));
      }
    } else {
#pragma unroll
      for (int i = 0; i < AI; ++i) {
        av[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (rows[i] >= 0)
          av[i] = *reinterpret_cast<const float4*>(a.feat + (long long)rows[i] * a.cin + (cbi << a.cb_log2) + within);
      }
      const long long wbase = pvalid ? ((long long)(act_kid[ai] * a.ppo + cbi) * a.cout_pad) : 0;
#pragma unroll
      for (int i = 0; i < BI; ++i) {
        bv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (pvalid) {
          const int col = colblock + r0 + 32 * i;
          bv[i] = *reinterpret_cast<const float4*>(a.wp + ((wbase + col) << a.cb_log2) + within);
        }
      }
    }
  };

  int rows_cur[AI], rows_nxt[AI];
  float4 av[AI], bv[BI];
  int ai_c, cbi_c, ai_n = -1, cbi_n = 0;
  bool pv_c, pv_n = false;
  if (nchunks > 0) {
    chunk_ids(0, ai_c, cbi_c, pv_c);
    load_rows(ai_c, pv_c, rows_cur);
    issue(ai_c, cbi_c, pv_c, rows_cur, av, bv);
    if (nchunks > 1) {
      chunk_ids(1, ai_n, cbi_n, pv_n);
      if (ai_n != ai_c) load_rows(ai_n, pv_n, rows_nxt);
      else {
#pragma unroll
        for (int i = 0; i < AI; ++i) rows_nxt[i] = rows_cur[i];
      }
    }
  }

  for (int c = 0; c < nchunks; ++c) {
    if (MODE != MODE_CONV) {
#pragma unroll
      for (int i = 0; i < AI; ++i) {
        av[i].x = fabsf(av[i].x); av[i].y = fabsf(av[i].y); av[i].z = fabsf(av[i].z); av[i].w = fabsf(av[i].w);
      }
    }
    __syncthreads();   // previous chunk's fragment reads are done
#pragma unroll
    for (int i = 0; i < AI; ++i)
      *reinterpret_cast<float4*>(&As[(r0 + 32 * i) * LDS_LD + kk0]) = av[i];
#pragma unroll
    for (int i = 0; i < BI; ++i)
      *reinterpret_cast<float4*>(&Bs[(r0 + 32 * i) * LDS_LD + kk0]) = bv[i];
    __syncthreads();
    if (c + 1 < nchunks) {          // next chunk's global loads fly during this chunk's MFMAs
#pragma unroll
      for (int i = 0; i < AI; ++i) rows_cur[i] = rows_nxt[i];
      ai_c = ai_n; cbi_c = cbi_n; pv_c = pv_n;
      issue(ai_c, cbi_c, pv_c, rows_cur, av, bv);
      if (c + 2 < nchunks) {
        chunk_ids(c + 2, ai_n, cbi_n, pv_n);
        if (ai_n != ai_c) load_rows(ai_n, pv_n, rows_nxt);
      }
    }
    if constexpr (BUF) __builtin_amdgcn_sched_barrier(0);   // keep the prefetch ahead of the MFMAs, not next to its use
    // LDS -> fragments -> MFMA
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float4 af[TM], bf[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i)
        af[i] = *reinterpret_cast<const float4*>(&As[((wm * TM + i) * 32 + r31) * LDS_LD + g * 8 + half * 4]);
#pragma unroll
      for (int j = 0; j < TN; ++j)
        bf[j] = *reinterpret_cast<const float4*>(&Bs[((wn * TN + j) * 32 + r31) * LDS_LD + g * 8 + half * 4]);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].x, bf[j].x, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].y, bf[j].y, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].z, bf[j].z, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].w, bf[j].w, acc[i][j], 0, 0, 0);
        }
    }
  }

  // ---- epilogue: bias, activation (or GDN), store -------------------------------------------
  // Full tiles written to consecutive rows take a branch-free path: one base pointer per lane, the activation chosen
  // once per tile.  (The general loop below costs ~50 instructions per element -- row-list lookups, tail checks and
  // the activation switch for each of the 64 values a lane holds -- which is as much as the whole MFMA phase of a
  // 128-deep GEMM tile.)
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

// The instantiations of k_conv_mfma: the six tiles of launch_mfma in its three modes (launch_pair_product takes three of them),
// each with and without buffer loads.  Tile choice and grid are the caller's.
int launch_conv_f32(int mode, int wm, int wn, int tm, int tn, bool buf, const ConvArgs& a, dim3 grid, hipStream_t s) {
#define PCC_F32_TILE(MODE, WM, WN, TM, TN)                                                       \
  if (mode == MODE && wm == WM && wn == WN && tm == TM && tn == TN) {                            \
    if (buf) k_conv_mfma<WM, WN, TM, TN, MODE, true><<<grid, 256, 0, s>>>(a);                    \
    else k_conv_mfma<WM, WN, TM, TN, MODE, false><<<grid, 256, 0, s>>>(a);                       \
    return PCC_OK;                                                                               \
  }
#define PCC_F32_MODES(WM, WN, TM, TN)                                                            \
  PCC_F32_TILE(MODE_CONV, WM, WN, TM, TN) PCC_F32_TILE(MODE_GDN, WM, WN, TM, TN) PCC_F32_TILE(MODE_IGDN, WM, WN, TM, TN)
  PCC_F32_MODES(2, 2, 2, 2)
  PCC_F32_MODES(2, 2, 1, 2)
  PCC_F32_MODES(1, 4, 1, 1)
  PCC_F32_MODES(2, 2, 2, 1)
  PCC_F32_MODES(2, 2, 1, 1)
  PCC_F32_MODES(4, 1, 1, 1)
#undef PCC_F32_MODES
#undef PCC_F32_TILE
  PCC_REQUIRE(false, "launch_conv_f32: no kernel for mode %d, tile %d x %d waves of %d x %d fragments", mode, wm, wn, tm, tn);
  return PCC_EINVAL;
}
