// Inter-frame RAHT colour, device side (DESIGN.md section 7f "Inter frames", stream format 0xB4): the transform, rows, quantiser
// and groups of pcc_raht.hip with a prediction in the coefficient domain.  P [n, C] is a Q8 signal over the CURRENT voxels taken
// from a motion-compensated reference cloud (blocks, vectors and matches are those of the lossless inter coder:
// pcc_geom_inter_motion, pcc_lift_inter_match); the same integer forward transform runs over P with the current geometry's
// weights, and a row travels as quantise(H - Hp).  Per block (a node of level first = max(0, depth - 4)) P is kept (mode 1) or
// zeroed (mode 0); the levels above the blocks are transformed after that decision.
//   k_raht_inter_sums      per block: integer sums of the matched voxels' reference rows per channel, and their count
//   k_raht_inter_fill      P[i] = the match's row, else floor(block sum / count), else (no match in the block, or mode 0) zero
//   k_raht_inter_forward   k_raht_forward over source and prediction in one walk of the node (probes and factor pairs shared):
//                          both DCs, quantise(H) and quantise(H - Hp) at the node's rows, sum |symbol| of either set added to
//                          the node's block (runs of lanes of one block reduced in the wave before the two atomics)
//   k_raht_inter_modes     mode[b] = the block has a match and its predicted sum is strictly smaller; the prediction's DC of a
//                          mode-0 block is zeroed for the levels above
//   k_raht_inter_select    per node of a level >= first: the group of its rows (the extra set 6 * depth + ... in a mode-1 block)
//                          or the member the side bytes give it; on the encoder the intra symbols of mode-0 blocks copied in
//   k_raht_inter_predict   decoder: the forward transform of the prediction alone, unquantised Hp rows and DCs
//   k_raht_inter_inverse   k_raht_inverse with Hp added to q * step (and the prediction's DC to the root's) before the butterflies
// One thread per voxel or node as in pcc_raht.hip; all arithmetic is integer.  No kernel reads a bitstream: every row access is
// bounded by caller-given counts; a block row, a mode or a match outside its range counts as mode 0 / unmatched and sets the flag.
#include "pcc_raht.h"

// Rows are in key order, so runs of lanes share a block.  A run starts where the block differs from the lane below; `end` is the
// lane after this lane's run.  Every lane of the wave must call these.
__device__ inline bool raht_run_head(int blk, int& end) {
  const int lane = threadIdx.x & 63;
  const int below = __shfl_up(blk, 1);
  const unsigned long long heads = __ballot(lane == 0 || below != blk);
  const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
  end = above ? lane + __ffsll((long long)above) : 64;
  return (heads >> lane) & 1ull;
}

// the sum of `v` over this lane and the lanes above it inside its run (the run's total in its first lane)
__device__ inline int raht_run_sum(int v, int end) {
  const int lane = threadIdx.x & 63;
  for (int d = 1; d < 64; d <<= 1) {
    const int a = __shfl_down(v, d);
    if (lane + d < end) v += a;
  }
  return v;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------
// sums [blocks, C + 1]: per channel the sum of the matched voxels' reference rows (|value| < 2^17, at most 4096 voxels: int32),
// then their count
__global__ void __launch_bounds__(256) k_raht_inter_sums(const int64_t* __restrict__ vkeys, int n, OctBlocks B, const int* __restrict__ match,
                                                         const int* __restrict__ tv, int nr, int C, int* __restrict__ sums,
                                                         int* __restrict__ d_flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  int blk = -1, m = -1;
  if (i < n) {
    blk = oct_block_of(B, vkeys[i]);
    m = match[i];
    if (m < -1 || m >= nr || blk < 0) { atomicOr(d_flag, 1); m = -1; }
  }
  int end;
  const bool head = raht_run_head(blk, end);
  for (int c = 0; c <= C; ++c) {
    const int v = m < 0 ? 0 : (c < C ? tv[(size_t)m * C + c] : 1);
    const int s = raht_run_sum(v, end);
    if (head && blk >= 0 && s != 0) atomicAdd(&sums[(size_t)blk * (C + 1) + c], s);
  }
}

__global__ void __launch_bounds__(256) k_raht_inter_fill(const int64_t* __restrict__ vkeys, int n, OctBlocks B, const int* __restrict__ match,
                                                         const int* __restrict__ tv, int nr, int C, const int* __restrict__ sums,
                                                         const int* __restrict__ mode, int* __restrict__ pred, int* __restrict__ d_flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int blk = oct_block_of(B, vkeys[i]);
  int m = match[i];
  if (m < -1 || m >= nr) m = -1;                      // k_raht_inter_sums has set the flag
  int keep = blk < 0 ? 0 : (mode ? mode[blk] : 1);
  if (keep != 0 && keep != 1) { atomicOr(d_flag, 1); keep = 0; }
  const int cnt = blk < 0 ? 0 : sums[(size_t)blk * (C + 1) + C];
  if (cnt <= 0) keep = 0;                             // a block without any match is mode 0 by rule
  for (int c = 0; c < C; ++c) {
    int p = 0;
    if (keep) p = m >= 0 ? tv[(size_t)m * C + c] : oct_floor_div32(sums[(size_t)blk * (C + 1) + c], cnt);
    pred[(size_t)i * C + c] = p;
  }
}

__global__ void __launch_bounds__(256) k_raht_inter_forward(RahtLevel L, OctBlocks B, const int* __restrict__ off, const int* __restrict__ cw,
                                                            const int* __restrict__ cv, const int* __restrict__ cp, int C, RahtSteps steps,
                                                            int* __restrict__ wout, int* __restrict__ vout, int* __restrict__ pout,
                                                            int* __restrict__ coef, int* __restrict__ coef_p, long long row_base,
                                                            long long rows_total, int* __restrict__ sums, int* __restrict__ d_flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < L.n;                          // with sums every lane stays for the wave's shuffles
  int blk = -1, s_intra = 0, s_inter = 0;
  if (live) {
    int kid[8], w[8];
    oct_kids(L, i, kid);
    oct_child_weights(cw, kid, w);
    RahtNode nd;
    raht_node(w, nd);
    wout[i] = nd.weight;
    if (sums) {
      blk = oct_block_of(B, L.keys[i]);
      if (blk < 0) atomicOr(d_flag, 1);
    }
    long long row[7], r = row_base + off[i] - i;
#pragma unroll
    for (int t = 0; t < 7; ++t) { row[t] = (nd.e[t] && r >= 0 && r < rows_total) ? r : -1; r += nd.e[t]; }
    for (int c = 0; c < C; ++c) {
      const long long step = steps.v[c];
      long long x[8], p[8], h[7], hp[7];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        x[j] = kid[j] < 0 ? 0 : cv[(size_t)kid[j] * C + c];
        p[j] = kid[j] < 0 ? 0 : cp[(size_t)kid[j] * C + c];
      }
      vout[(size_t)i * C + c] = (int)raht_node_fwd(nd, x, h);
      pout[(size_t)i * C + c] = (int)raht_node_fwd(nd, p, hp);
#pragma unroll
      for (int t = 0; t < 7; ++t) {
        if (row[t] < 0) continue;
        const int q0 = raht_quantise(h[t], step), q1 = raht_quantise(h[t] - hp[t], step);
        coef[row[t] * C + c] = q0;
        coef_p[row[t] * C + c] = q1;
        s_intra += q0 < 0 ? -q0 : q0;
        s_inter += q1 < 0 ? -q1 : q1;
      }
    }
  }
  if (!sums) return;                                  // uniform: a kernel argument
  int end;
  const bool head = raht_run_head(blk, end);
  s_intra = raht_run_sum(s_intra, end);
  s_inter = raht_run_sum(s_inter, end);
  if (head && blk >= 0) {
    atomicAdd(&sums[2 * blk], s_intra);
    atomicAdd(&sums[2 * blk + 1], s_inter);
  }
}

__global__ void __launch_bounds__(256) k_raht_inter_modes(const int* __restrict__ sums, const int* __restrict__ fill_sums, int nb, int C,
                                                          int* __restrict__ mode, int* __restrict__ pdc) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nb) return;
  const int m = (fill_sums[(size_t)b * (C + 1) + C] > 0 && sums[2 * b + 1] < sums[2 * b]) ? 1 : 0;
  mode[b] = m;
  if (!m)
    for (int c = 0; c < C; ++c) pdc[(size_t)b * C + c] = 0;
}

__global__ void __launch_bounds__(256) k_raht_inter_select(const int64_t* __restrict__ keys, const int* __restrict__ mask,
                                                           const int* __restrict__ off, int n, int level, int depth, int C, OctBlocks B,
                                                           const int* __restrict__ mode, const int* __restrict__ side,
                                                           int* __restrict__ idx, int* __restrict__ coef_p, const int* __restrict__ coef,
                                                           long long row_base, long long rows_total, int* __restrict__ d_flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bool e[7];
  oct_emits(mask[i] & 255, e);
  const int blk = oct_block_of(B, keys[i]);
  int m = blk < 0 ? -1 : mode[blk];
  if (m != 0 && m != 1) { atomicOr(d_flag, 1); m = 0; }
  long long r = row_base + off[i] - i;
#pragma unroll
  for (int t = 0; t < 7; ++t) {
    if (!e[t]) continue;
    if (r >= 0 && r < rows_total) {
      const int stage = t == 0 ? 2 : (t < 3 ? 1 : 0);   // 0: z (stage 1), 1: y (stage 2), 2: x (stage 3)
      for (int c = 0; c < C; ++c) {
        const int g = (m ? depth : level) * 6 + (c ? 3 : 0) + stage;
        idx[r * C + c] = side ? (side[g] & 63) : g;
        if (coef && !m) coef_p[r * C + c] = coef[r * C + c];
      }
    }
    ++r;
  }
}

__global__ void __launch_bounds__(256) k_raht_inter_predict(RahtLevel L, const int* __restrict__ off, const int* __restrict__ cw,
                                                            const int* __restrict__ cp, int C, int* __restrict__ pout,
                                                            int* __restrict__ hp_rows, long long row_base, long long rows_total) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L.n) return;
  int kid[8], w[8];
  oct_kids(L, i, kid);
  oct_child_weights(cw, kid, w);
  RahtNode nd;
  raht_node(w, nd);
  long long row[7], r = row_base + off[i] - i;
#pragma unroll
  for (int t = 0; t < 7; ++t) { row[t] = (nd.e[t] && r >= 0 && r < rows_total) ? r : -1; r += nd.e[t]; }
  for (int c = 0; c < C; ++c) {
    long long p[8], hp[7];
#pragma unroll
    for (int j = 0; j < 8; ++j) p[j] = kid[j] < 0 ? 0 : cp[(size_t)kid[j] * C + c];
    pout[(size_t)i * C + c] = (int)raht_node_fwd(nd, p, hp);
#pragma unroll
    for (int t = 0; t < 7; ++t)
      if (row[t] >= 0) hp_rows[row[t] * C + c] = (int)hp[t];
  }
}

// The body below the dequantisation is k_raht_inverse's (pcc_raht.hip): the same clamps in the same places.
__global__ void __launch_bounds__(256) k_raht_inter_inverse(RahtLevel L, const int* __restrict__ off, const int* __restrict__ cw,
                                                            const int* __restrict__ v, const int* __restrict__ dcp, int C, RahtSteps steps,
                                                            const int* __restrict__ coef, const int* __restrict__ hp_rows,
                                                            long long row_base, long long rows_total, int* __restrict__ cv,
                                                            int* __restrict__ d_flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L.n) return;
  int kid[8], w[8];
  oct_kids(L, i, kid);
  oct_child_weights(cw, kid, w);
  RahtNode nd;
  raht_node(w, nd);
  long long row[7], r = row_base + off[i] - i;
#pragma unroll
  for (int t = 0; t < 7; ++t) { row[t] = (nd.e[t] && r >= 0 && r < rows_total) ? r : -1; r += nd.e[t]; }
  bool clamped = false;
  auto lim = [&](long long t) {
    if (t > RAHT_LIMIT) { clamped = true; return RAHT_LIMIT; }
    if (t < -RAHT_LIMIT) { clamped = true; return -RAHT_LIMIT; }
    return t;
  };
  for (int c = 0; c < C; ++c) {
    const long long step = steps.v[c];
    long long h[7];
#pragma unroll
    for (int t = 0; t < 7; ++t)
      h[t] = row[t] < 0 ? 0 : lim((long long)hp_rows[row[t] * C + c] + lim((long long)coef[row[t] * C + c] * step));
    long long x[8], y[4], u[2];
    const long long dc = lim((long long)v[(size_t)i * C + c] + (dcp ? (long long)dcp[(size_t)i * C + c] : 0ll));
    if (nd.e[0]) { raht_inv(nd.a[0], nd.b[0], dc, h[0], u[0], u[1]); u[0] = lim(u[0]); u[1] = lim(u[1]); }
    else { u[0] = (w[0] + w[1] + w[2] + w[3]) > 0 ? dc : 0; u[1] = (w[4] + w[5] + w[6] + w[7]) > 0 ? dc : 0; }
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      if (nd.e[1 + m]) {
        raht_inv(nd.a[1 + m], nd.b[1 + m], u[m], h[1 + m], y[2 * m], y[2 * m + 1]);
        y[2 * m] = lim(y[2 * m]); y[2 * m + 1] = lim(y[2 * m + 1]);
      } else {
        y[2 * m] = (w[4 * m] + w[4 * m + 1]) > 0 ? u[m] : 0;
        y[2 * m + 1] = (w[4 * m + 2] + w[4 * m + 3]) > 0 ? u[m] : 0;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (nd.e[3 + k]) {
        raht_inv(nd.a[3 + k], nd.b[3 + k], y[k], h[3 + k], x[2 * k], x[2 * k + 1]);
        x[2 * k] = lim(x[2 * k]); x[2 * k + 1] = lim(x[2 * k + 1]);
      } else {
        x[2 * k] = y[k]; x[2 * k + 1] = y[k];            // only the present one is stored
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (kid[j] >= 0) cv[(size_t)kid[j] * C + c] = (int)x[j];
  }
  if (clamped) atomicOr(d_flag, 1);
}

// ---- entry points --------------------------------------------------------------------------------------------------------------
extern "C" int pcc_raht_inter_fill(const int64_t* voxel_keys, int64_t n, const int64_t* block_keys, int64_t n_blocks,
                                   const uint64_t* block_bits, const int32_t* block_rank, const int32_t* h_block, int32_t block_log2,
                                   const int32_t* match, const int32_t* ref_values, int64_t n_ref, int32_t channels, const int32_t* mode,
                                   int32_t* sums, int32_t* pred, int32_t* d_flag, void* stream) {
  const char* what = "pcc_raht_inter_fill";
  OctBlocks B;
  if (!oct_blocks(what, block_keys, n_blocks, block_bits, block_rank, h_block, block_log2, &B)) return PCC_EINVAL;
  PCC_REQUIRE(voxel_keys && match && sums && pred && d_flag && n > 0 && n < (1ll << 26) && channels >= 1 && channels <= RAHT_MAX_C &&
              n_ref >= 0 && n_ref < (1ll << 26) && (n_ref == 0 || ref_values), "pcc_raht_inter_fill: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  PCC_CHECK_HIP(hipMemsetAsync(sums, 0, (size_t)n_blocks * (channels + 1) * 4, s));
  k_raht_inter_sums<<<(unsigned)pcc_cdiv(n, 256), 256, 0, s>>>(voxel_keys, (int)n, B, match, ref_values, (int)n_ref, channels, sums, d_flag);
  PCC_LAUNCH_CHECK();
  k_raht_inter_fill<<<(unsigned)pcc_cdiv(n, 256), 256, 0, s>>>(voxel_keys, (int)n, B, match, ref_values, (int)n_ref, channels, sums, mode, pred,
                                                              d_flag);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_raht_inter_forward(const int64_t* keys, int64_t n, int32_t pitch, const int64_t* child_keys, int64_t n_child,
                                      const uint64_t* child_bits, const int32_t* child_rank, const int32_t* h_child,
                                      const int64_t* block_keys, int64_t n_blocks, const uint64_t* block_bits, const int32_t* block_rank,
                                      const int32_t* h_block, int32_t block_log2, const int32_t* off, const int32_t* child_w,
                                      const int32_t* child_v, const int32_t* child_p, int32_t channels, const int32_t* h_steps, int32_t* w,
                                      int32_t* v, int32_t* p, int32_t* coef, int32_t* coef_p, int64_t row_base, int64_t rows_total,
                                      int32_t* sums, int32_t* d_flag, void* stream) {
  const char* what = "pcc_raht_inter_forward";
  RahtLevel L;
  RahtSteps st;
  OctBlocks B = {};
  if (!raht_level(what, keys, n, pitch, child_keys, n_child, child_bits, child_rank, h_child, &L)) return PCC_EINVAL;
  if (!raht_steps(what, channels, h_steps, &st)) return PCC_EINVAL;
  if (sums) {                                         // a level at or below the blocks: its nodes' sums go to their blocks
    if (!oct_blocks(what, block_keys, n_blocks, block_bits, block_rank, h_block, block_log2, &B)) return PCC_EINVAL;
    PCC_REQUIRE(pitch <= (1 << block_log2) && d_flag, "pcc_raht_inter_forward: sums belong to the levels inside the blocks");
  }
  PCC_REQUIRE(off && child_v && child_p && w && v && p && coef && coef_p && row_base >= 0 && rows_total > 0,
              "pcc_raht_inter_forward: bad arguments");
  k_raht_inter_forward<<<(unsigned)pcc_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(L, B, off, child_w, child_v, child_p, channels, st, w, v, p,
                                                                                  coef, coef_p, row_base, rows_total, sums, d_flag);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_raht_inter_modes(const int32_t* sums, const int32_t* fill_sums, int64_t n_blocks, int32_t channels, int32_t* mode,
                                    int32_t* block_p, void* stream) {
  PCC_REQUIRE(sums && fill_sums && mode && block_p && n_blocks > 0 && n_blocks < (1ll << 24) && channels >= 1 && channels <= RAHT_MAX_C,
              "pcc_raht_inter_modes: bad arguments");
  k_raht_inter_modes<<<(unsigned)pcc_cdiv(n_blocks, 256), 256, 0, (hipStream_t)stream>>>(sums, fill_sums, (int)n_blocks, channels, mode,
                                                                                       block_p);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_raht_inter_select(const int64_t* keys, const int32_t* mask, const int32_t* off, int64_t n, int32_t level, int32_t depth,
                                     int32_t channels, const int64_t* block_keys, int64_t n_blocks, const uint64_t* block_bits,
                                     const int32_t* block_rank, const int32_t* h_block, int32_t block_log2, const int32_t* mode,
                                     const int32_t* side, int32_t* idx, int32_t* coef_p, const int32_t* coef, int64_t row_base,
                                     int64_t rows_total, int32_t* d_flag, void* stream) {
  const char* what = "pcc_raht_inter_select";
  OctBlocks B;
  if (!oct_blocks(what, block_keys, n_blocks, block_bits, block_rank, h_block, block_log2, &B)) return PCC_EINVAL;
  PCC_REQUIRE(keys && mask && off && mode && idx && d_flag && n > 0 && n < (1ll << 26) && depth >= 1 && depth < 15 &&
              level >= depth - block_log2 && level >= 0 && level < depth && channels >= 1 && channels <= RAHT_MAX_C && row_base >= 0 &&
              rows_total > 0 && rows_total < (1ll << 26) && (!coef || coef_p),
              "pcc_raht_inter_select: bad arguments (a level inside the blocks of a cloud of depth <= 14)");
  k_raht_inter_select<<<(unsigned)pcc_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(keys, mask, off, (int)n, level, depth, channels, B, mode,
                                                                                 side, idx, coef_p, coef, row_base, rows_total, d_flag);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_raht_inter_predict(const int64_t* keys, int64_t n, int32_t pitch, const int64_t* child_keys, int64_t n_child,
                                      const uint64_t* child_bits, const int32_t* child_rank, const int32_t* h_child, const int32_t* off,
                                      const int32_t* child_w, const int32_t* child_p, int32_t channels, int32_t* p, int32_t* hp,
                                      int64_t row_base, int64_t rows_total, void* stream) {
  RahtLevel L;
  if (!raht_level("pcc_raht_inter_predict", keys, n, pitch, child_keys, n_child, child_bits, child_rank, h_child, &L)) return PCC_EINVAL;
  PCC_REQUIRE(off && child_p && p && hp && channels >= 1 && channels <= RAHT_MAX_C && row_base >= 0 && rows_total > 0,
              "pcc_raht_inter_predict: bad arguments");
  k_raht_inter_predict<<<(unsigned)pcc_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(L, off, child_w, child_p, channels, p, hp, row_base,
                                                                                  rows_total);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_raht_inter_inverse(const int64_t* keys, int64_t n, int32_t pitch, const int64_t* child_keys, int64_t n_child,
                                      const uint64_t* child_bits, const int32_t* child_rank, const int32_t* h_child, const int32_t* off,
                                      const int32_t* child_w, const int32_t* v, const int32_t* dc_p, int32_t channels,
                                      const int32_t* h_steps, const int32_t* coef, const int32_t* hp, int64_t row_base, int64_t rows_total,
                                      int32_t* child_v, int32_t* d_flag, void* stream) {
  const char* what = "pcc_raht_inter_inverse";
  RahtLevel L;
  RahtSteps st;
  if (!raht_level(what, keys, n, pitch, child_keys, n_child, child_bits, child_rank, h_child, &L)) return PCC_EINVAL;
  if (!raht_steps(what, channels, h_steps, &st)) return PCC_EINVAL;
  PCC_REQUIRE(off && v && child_v && d_flag && coef && hp && row_base >= 0 && rows_total > 0, "pcc_raht_inter_inverse: bad arguments");
  k_raht_inter_inverse<<<(unsigned)pcc_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(L, off, child_w, v, dc_p, channels, st, coef, hp, row_base,
                                                                                  rows_total, child_v, d_flag);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}
