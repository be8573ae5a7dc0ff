// Inter-frame lossless colour, device side (DESIGN.md section 7i "Inter frames", stream format 0xB6): the lifting coder of
// pcc_lift.hip with a second source for the prediction of the LAST level (the nodes whose children are voxels) -- the colour of
// the voxel's match in a motion-compensated reference cloud.  Blocks and vectors are those of the inter geometry coder
// (pcc_geom_inter.hip); the decoder re-runs the search, so no vector travels.  Levels above the last are coded by pcc_lift.hip.
//   k_lift_inter_match      per voxel p of a block with vector d: the reference row at p - d or, when that cell is empty, at the
//                           first occupied of its 26 neighbours by (|o|^2, k = 9 (ox + 1) + 3 (oy + 1) + (oz + 1)); -1: unmatched
//   k_lift_inter_match_wide the same with a packed displacement per block (the wide search of pcc_geom_wide.hip, streams 0xB7 / 0xB8)
//   k_lift_inter_residual   per last-level node both residual sets -- rows -= Hp of the spatial prediction, as k_lift_residual, and
//                           H - Hp of the temporal one (a matched child predicted by its match's values, an unmatched one spatially)
//                           into a second buffer -- and sum |symbol| of each set added to the node's block (int32, order independent)
//   k_lift_inter_modes      mode[b] = the temporal sum is strictly smaller
//   k_lift_inter_select     per last-level node: the group (or, with side bytes, the table member) of its rows -- the groups of
//                           level `level + 1` for a mode-1 block -- and, on the encoder, the temporal rows of mode-1 blocks copied in
//   k_lift_inter_inverse    k_lift_inverse for the last level with the block's mode choosing the prediction
// One thread per voxel or node, the loops over children, cells and butterflies unrolled as in pcc_lift.hip.  No kernel reads a
// bitstream: every row access is bounded by caller-given counts, a block row, a vector index, a mode or a match outside its range
// counts as vector 0 / mode 0 / unmatched and sets the flag word.
#include "pcc_geom_inter.h"
#include "pcc_lift.h"

// the matches of a node's children, validated: tm[j] in [-1, nr); returns false when one had to be dropped
__device__ inline bool lift_kid_matches(const int* __restrict__ match, int nr, const int kid[8], int tm[8]) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    int m = kid[j] < 0 ? -1 : match[kid[j]];
    if (m < -1 || m >= nr) { ok = false; m = -1; }
    tm[j] = m;
  }
  return ok;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_lift_inter_match(const int64_t* __restrict__ vkeys, int n, OctBlocks B, const int* __restrict__ vec,
                                                          InterCands cands, const int64_t* __restrict__ rkeys, int nr, PccGrid rg, int ox,
                                                          int oy, int oz, int* __restrict__ match, int* __restrict__ d_flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t key = vkeys[i];
  const int row = oct_block_of(B, key);
  int j = row < 0 ? -1 : vec[row];
  if (j < 0 || j >= cands.n) { atomicOr(d_flag, 1); j = 0; }
  int dx, dy, dz;
  inter_cand(cands, j, dx, dy, dz);
  const int qx = ox + pcc_key_x(key) - dx, qy = oy + pcc_key_y(key) - dy, qz = oz + pcc_key_z(key) - dz;
  int m = -1;
  for (int d2 = 0; d2 <= 3 && m < 0; ++d2)
    for (int k = 0; k < 27 && m < 0; ++k) {
      const int ax = k / 9 - 1, ay = (k / 3) % 3 - 1, az = k % 3 - 1;
      if (ax * ax + ay * ay + az * az == d2) m = inter_row(rg, rkeys, nr, qx + ax, qy + ay, qz + az);
    }
  match[i] = m;
}

// k_lift_inter_match with a packed displacement per block (the wide search); one outside +-search counts as zero and sets the flag
__global__ void __launch_bounds__(256) k_lift_inter_match_wide(const int64_t* __restrict__ vkeys, int n, OctBlocks B, const int* __restrict__ disp,
                                                               int search, const int64_t* __restrict__ rkeys, int nr, PccGrid rg, int ox,
                                                               int oy, int oz, int* __restrict__ match, int* __restrict__ d_flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t key = vkeys[i];
  const int row = oct_block_of(B, key);
  int dx, dy, dz;
  if (!wide_unpack(row < 0 ? -1 : disp[row], search, dx, dy, dz)) atomicOr(d_flag, 1);
  const int qx = ox + pcc_key_x(key) - dx, qy = oy + pcc_key_y(key) - dy, qz = oz + pcc_key_z(key) - dz;
  int m = -1;
  for (int d2 = 0; d2 <= 3 && m < 0; ++d2)
    for (int k = 0; k < 27 && m < 0; ++k) {
      const int ax = k / 9 - 1, ay = (k / 3) % 3 - 1, az = k % 3 - 1;
      if (ax * ax + ay * ay + az * az == d2) m = inter_row(rg, rkeys, nr, qx + ax, qy + ay, qz + az);
    }
  match[i] = m;
}

__global__ void __launch_bounds__(256) k_lift_inter_residual(LiftLevel L, OctBlocks B, const int* __restrict__ off,
                                                             const int* __restrict__ v, int C, const int* __restrict__ match,
                                                             const int* __restrict__ tv, int nr, int* __restrict__ coef,
                                                             int* __restrict__ coef_t, long long row_base, long long rows_total,
                                                             int* __restrict__ sums, int* __restrict__ d_flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < L.n;                          // every lane stays for the wave's shuffles
  int blk = -1, s_sp = 0, s_tm = 0;
  if (live) {
    int kid[8], w[8], nb[27], tm[8];
    bool e[7];
    oct_emits(oct_kids(L, i, kid), e);
    oct_child_weights(nullptr, kid, w);
    lift_neighbours(L, i, nb);
    bool ok = lift_kid_matches(match, nr, kid, tm);
    blk = oct_block_of(B, L.keys[i]);
    if (blk < 0) ok = false;
    long long row[7], r = row_base + off[i] - i;
#pragma unroll
    for (int t = 0; t < 7; ++t) { row[t] = (e[t] && r >= row_base && r < rows_total) ? r : -1; r += e[t]; }
    for (int c = 0; c < C; ++c) {
      int pred[8], hp[7], ht[7];
      lift_child_preds(v, C, c, nb, kid, pred);
      lift_node_fwd(w, e, pred, hp);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (tm[j] >= 0) pred[j] = tv[(size_t)tm[j] * C + c];
      lift_node_fwd(w, e, pred, ht);
#pragma unroll
      for (int t = 0; t < 7; ++t) {
        if (row[t] < 0) continue;
        const int h = coef[row[t] * C + c], a = h - hp[t], b = h - ht[t];
        coef[row[t] * C + c] = a;
        coef_t[(row[t] - row_base) * C + c] = b;
        s_sp += a < 0 ? -a : a;
        s_tm += b < 0 ? -b : b;
      }
    }
    if (!ok) atomicOr(d_flag, 1);
  }
  // rows are in key order, so runs of lanes share a block: a run starts where the block differs from the lane below, its first
  // lane collects the run's sums (suffix sums that stop at the next run's start) and issues the two atomics
  const int lane = threadIdx.x & 63;
  const int below = __shfl_up(blk, 1);
  const unsigned long long heads = __ballot(lane == 0 || below != blk);
  const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
  const int end = above ? lane + __ffsll((long long)above) : 64;      // the lane after this lane's run
  for (int d = 1; d < 64; d <<= 1) {
    const int a = __shfl_down(s_sp, d), b = __shfl_down(s_tm, d);
    if (lane + d < end) { s_sp += a; s_tm += b; }
  }
  if (((heads >> lane) & 1ull) && blk >= 0) {
    atomicAdd(&sums[2 * blk], s_sp);
    atomicAdd(&sums[2 * blk + 1], s_tm);
  }
}

__global__ void __launch_bounds__(256) k_lift_inter_modes(const int* __restrict__ sums, int nb, int* __restrict__ mode) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < nb) mode[b] = sums[2 * b + 1] < sums[2 * b] ? 1 : 0;
}

__global__ void __launch_bounds__(256) k_lift_inter_select(const int64_t* __restrict__ keys, const int* __restrict__ mask,
                                                           const int* __restrict__ off, int n, int level, int C, OctBlocks B,
                                                           const int* __restrict__ mode, const int* __restrict__ side,
                                                           int* __restrict__ idx, int* __restrict__ coef, const int* __restrict__ coef_t,
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
    if (r >= row_base && r < rows_total) {
      const int stage = t == 0 ? 2 : (t < 3 ? 1 : 0);   // 0: z (stage 1), 1: y (stage 2), 2: x (stage 3)
      for (int c = 0; c < C; ++c) {
        const int g = (level + m) * 6 + (c ? 3 : 0) + stage;
        idx[r * C + c] = side ? (side[g] & 63) : g;
        if (coef_t && m) coef[r * C + c] = coef_t[(r - row_base) * C + c];
      }
    }
    ++r;
  }
}

// The body below the prediction is k_lift_inverse's (pcc_lift.hip): the same clamps in the same places.
__global__ void __launch_bounds__(256) k_lift_inter_inverse(LiftLevel L, OctBlocks B, const int* __restrict__ mode,
                                                            const int* __restrict__ off, const int* __restrict__ v, int C, int colour,
                                                            const int* __restrict__ match, const int* __restrict__ tv, int nr,
                                                            const int* __restrict__ coef, long long row_base, long long rows_total,
                                                            int* __restrict__ cv, int* __restrict__ d_flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L.n) return;
  int kid[8], w[8], nb[27], tm[8];
  bool e[7];
  oct_emits(oct_kids(L, i, kid), e);
  oct_child_weights(nullptr, kid, w);
  lift_neighbours(L, i, nb);
  bool clamped = !lift_kid_matches(match, nr, kid, tm);
  const int blk = oct_block_of(B, L.keys[i]);
  int m = blk < 0 ? -1 : mode[blk];
  if (m != 0 && m != 1) { clamped = true; m = 0; }
  long long row[7], r = row_base + off[i] - i;
#pragma unroll
  for (int t = 0; t < 7; ++t) { row[t] = (e[t] && r >= 0 && r < rows_total) ? r : -1; r += e[t]; }
  int wy[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) wy[k] = w[2 * k] + w[2 * k + 1];
  for (int c = 0; c < C; ++c) {
    const int lo = (colour && c) ? -255 : 0, hi = 255;
    auto lim = [&](int t) {
      if (t > hi) { clamped = true; return hi; }
      if (t < lo) { clamped = true; return lo; }
      return t;
    };
    int pred[8], h[7];
    lift_child_preds(v, C, c, nb, kid, pred);
    if (m) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (tm[j] >= 0) pred[j] = tv[(size_t)tm[j] * C + c];
    }
    lift_node_fwd(w, e, pred, h);
#pragma unroll
    for (int t = 0; t < 7; ++t) {
      if (row[t] < 0) continue;
      int s = coef[row[t] * C + c];
      if (s > LIFT_SYMBOL_LIMIT) { clamped = true; s = LIFT_SYMBOL_LIMIT; }
      if (s < -LIFT_SYMBOL_LIMIT) { clamped = true; s = -LIFT_SYMBOL_LIMIT; }
      h[t] += s;
    }
    int x[8], y[4], u[2];
    const int dc = lim(v[(size_t)i * C + c]);
    if (e[0]) { lift_inv(wy[0] + wy[1], wy[2] + wy[3], dc, h[0], u[0], u[1]); u[0] = lim(u[0]); u[1] = lim(u[1]); }
    else { u[0] = dc; u[1] = dc; }                      // only the present half is carried on
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      if (e[1 + q]) {
        lift_inv(wy[2 * q], wy[2 * q + 1], u[q], h[1 + q], y[2 * q], y[2 * q + 1]);
        y[2 * q] = lim(y[2 * q]); y[2 * q + 1] = lim(y[2 * q + 1]);
      } else { y[2 * q] = u[q]; y[2 * q + 1] = u[q]; }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (e[3 + k]) {
        lift_inv(w[2 * k], w[2 * k + 1], y[k], h[3 + k], x[2 * k], x[2 * k + 1]);
        x[2 * k] = lim(x[2 * k]); x[2 * k + 1] = lim(x[2 * k + 1]);
      } else { x[2 * k] = y[k]; x[2 * k + 1] = y[k]; }    // only the present one is stored
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (kid[j] >= 0) cv[(size_t)kid[j] * C + c] = x[j];
  }
  if (clamped) atomicOr(d_flag, 1);
}

// ---- entry points --------------------------------------------------------------------------------------------------------------
// the last level of a cloud: nodes at pitch 2 whose children are the voxels
static bool lift_last_level(const char* what, const int64_t* keys, int64_t n, int32_t pitch, const uint64_t* bits, const int32_t* rank,
                            const int32_t* h_grid, const int64_t* child_keys, int64_t n_child, const uint64_t* child_bits,
                            const int32_t* child_rank, const int32_t* h_child, LiftLevel* L) {
  if (pitch != 2) {
    pcc_set_error("%s: the inter prediction belongs to the last level (pitch 2), got pitch %d", what, pitch);
    return false;
  }
  return lift_level(what, keys, n, pitch, bits, rank, h_grid, child_keys, n_child, child_bits, child_rank, h_child, L);
}

static bool lift_reference(const char* what, const int32_t* match, const int32_t* ref_values, int64_t n_ref) {
  if (!(match && n_ref >= 0 && n_ref < (1ll << 26) && (n_ref == 0 || ref_values))) {
    pcc_set_error("%s: bad reference (match rows, and values for 0 .. 2^26 - 1 reference voxels)", what);
    return false;
  }
  return true;
}

extern "C" int pcc_lift_inter_match(const int64_t* voxel_keys, int64_t n, const int64_t* block_keys, int64_t n_blocks,
                                    const uint64_t* block_bits, const int32_t* block_rank, const int32_t* h_block, int32_t block_log2,
                                    const int32_t* vec, int32_t search, const int64_t* ref_keys, int64_t n_ref, const uint64_t* ref_bits,
                                    const int32_t* ref_rank, const int32_t* h_ref, int32_t ox, int32_t oy, int32_t oz, int32_t* match,
                                    int32_t* d_flag, void* stream) {
  PCC_REQUIRE(voxel_keys && vec && match && d_flag && n > 0 && n < (1ll << 26), "pcc_lift_inter_match: bad arguments");
  PCC_REQUIRE(n_ref >= 0 && n_ref < (1ll << 26) && (n_ref == 0 || ref_keys), "pcc_lift_inter_match: bad reference set");
  PCC_REQUIRE(inter_origin_ok(ox, oy, oz), "pcc_lift_inter_match: origin outside the 16-bit key range");
  OctBlocks B;
  if (!oct_blocks("pcc_lift_inter_match", block_keys, n_blocks, block_bits, block_rank, h_block, block_log2, &B)) return PCC_EINVAL;
  InterCands c;
  PCC_TRY(inter_cands(search, "pcc_lift_inter_match", &c));
  PccGrid g;
  PCC_TRY(pcc_grid_from_host(n_ref ? ref_bits : nullptr, ref_rank, h_ref, "pcc_lift_inter_match", &g));
  PCC_REQUIRE(!g.bits || h_ref[6] == 1, "pcc_lift_inter_match: the reference grid must have pitch 1");
  k_lift_inter_match<<<(unsigned)pcc_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(voxel_keys, (int)n, B, vec, c, ref_keys, (int)n_ref, g, ox,
                                                                                oy, oz, match, d_flag);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_lift_inter_match_wide(const int64_t* voxel_keys, int64_t n, const int64_t* block_keys, int64_t n_blocks,
                                         const uint64_t* block_bits, const int32_t* block_rank, const int32_t* h_block, int32_t block_log2,
                                         const int32_t* disp, int32_t search, const int64_t* ref_keys, int64_t n_ref,
                                         const uint64_t* ref_bits, const int32_t* ref_rank, const int32_t* h_ref, int32_t ox, int32_t oy,
                                         int32_t oz, int32_t* match, int32_t* d_flag, void* stream) {
  PCC_REQUIRE(voxel_keys && disp && match && d_flag && n > 0 && n < (1ll << 26), "pcc_lift_inter_match_wide: bad arguments");
  PCC_REQUIRE(n_ref >= 0 && n_ref < (1ll << 26) && (n_ref == 0 || ref_keys), "pcc_lift_inter_match_wide: bad reference set");
  PCC_REQUIRE(inter_origin_ok(ox, oy, oz), "pcc_lift_inter_match_wide: origin outside the 16-bit key range");
  PCC_REQUIRE(search >= 1 && search <= 7, "pcc_lift_inter_match_wide: search range %d outside 1..7", search);
  OctBlocks B;
  if (!oct_blocks("pcc_lift_inter_match_wide", block_keys, n_blocks, block_bits, block_rank, h_block, block_log2, &B)) return PCC_EINVAL;
  PccGrid g;
  PCC_TRY(pcc_grid_from_host(n_ref ? ref_bits : nullptr, ref_rank, h_ref, "pcc_lift_inter_match_wide", &g));
  PCC_REQUIRE(!g.bits || h_ref[6] == 1, "pcc_lift_inter_match_wide: the reference grid must have pitch 1");
  k_lift_inter_match_wide<<<(unsigned)pcc_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(voxel_keys, (int)n, B, disp, search, ref_keys, (int)n_ref,
                                                                                     g, ox, oy, oz, match, d_flag);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_lift_inter_residual(const int64_t* keys, int64_t n, int32_t pitch, const uint64_t* bits, const int32_t* rank,
                                       const int32_t* h_grid, const int64_t* child_keys, int64_t n_child, const uint64_t* child_bits,
                                       const int32_t* child_rank, const int32_t* h_child, const int64_t* block_keys, int64_t n_blocks,
                                       const uint64_t* block_bits, const int32_t* block_rank, const int32_t* h_block, int32_t block_log2,
                                       const int32_t* off, const int32_t* v, int32_t channels, const int32_t* match,
                                       const int32_t* ref_values, int64_t n_ref, int32_t* coef, int32_t* coef_t, int64_t row_base,
                                       int64_t rows_total, int32_t* sums, int32_t* d_flag, void* stream) {
  const char* what = "pcc_lift_inter_residual";
  LiftLevel L;
  OctBlocks B;
  if (!lift_last_level(what, keys, n, pitch, bits, rank, h_grid, child_keys, n_child, child_bits, child_rank, h_child, &L)) return PCC_EINVAL;
  if (!oct_blocks(what, block_keys, n_blocks, block_bits, block_rank, h_block, block_log2, &B)) return PCC_EINVAL;
  if (!lift_reference(what, match, ref_values, n_ref)) return PCC_EINVAL;
  // rows_total == row_base: no node of the level has two children -- no row is touched, coef_t may be NULL, the sums stay 0
  PCC_REQUIRE(channels >= 1 && channels <= LIFT_MAX_C && off && v && coef && sums && d_flag && row_base >= 0 && rows_total > 0 &&
              rows_total >= row_base && (coef_t || rows_total == row_base) && rows_total < (1ll << 26),
              "pcc_lift_inter_residual: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  PCC_CHECK_HIP(hipMemsetAsync(sums, 0, (size_t)n_blocks * 8, s));
  k_lift_inter_residual<<<(unsigned)pcc_cdiv(n, 256), 256, 0, s>>>(L, B, off, v, channels, match, ref_values, (int)n_ref, coef, coef_t, row_base,
                                                                  rows_total, sums, d_flag);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_lift_inter_select(const int64_t* keys, const int32_t* mask, const int32_t* off, int64_t n, int32_t level,
                                     int32_t channels, const int64_t* block_keys, int64_t n_blocks, const uint64_t* block_bits,
                                     const int32_t* block_rank, const int32_t* h_block, int32_t block_log2, const int32_t* sums,
                                     int32_t* mode, const int32_t* side, int32_t* idx, int32_t* coef, const int32_t* coef_t,
                                     int64_t row_base, int64_t rows_total, int32_t* d_flag, void* stream) {
  const char* what = "pcc_lift_inter_select";
  OctBlocks B;
  if (!oct_blocks(what, block_keys, n_blocks, block_bits, block_rank, h_block, block_log2, &B)) return PCC_EINVAL;
  PCC_REQUIRE(keys && mask && off && mode && idx && d_flag && n > 0 && n < (1ll << 26) && level >= 0 && level < 14 && channels >= 1 &&
              channels <= LIFT_MAX_C && row_base >= 0 && rows_total > 0 && rows_total >= row_base && rows_total < (1ll << 26),
              "pcc_lift_inter_select: bad arguments (the last level of a cloud of depth <= 14)");
  // a level without rows (rows_total == row_base) copies nothing: coef_t may be NULL there
  PCC_REQUIRE(!coef_t || coef, "pcc_lift_inter_select: coef_t needs coef");
  PCC_REQUIRE(!coef || coef_t || rows_total == row_base, "pcc_lift_inter_select: coef needs coef_t where the level has rows");
  hipStream_t s = (hipStream_t)stream;
  if (sums) {
    k_lift_inter_modes<<<(unsigned)pcc_cdiv(n_blocks, 256), 256, 0, s>>>(sums, (int)n_blocks, mode);
    PCC_LAUNCH_CHECK();
  }
  k_lift_inter_select<<<(unsigned)pcc_cdiv(n, 256), 256, 0, s>>>(keys, mask, off, (int)n, level, channels, B, mode, side, idx, coef, coef_t,
                                                                row_base, rows_total, d_flag);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_lift_inter_inverse(const int64_t* keys, int64_t n, int32_t pitch, const uint64_t* bits, const int32_t* rank,
                                      const int32_t* h_grid, const int64_t* child_keys, int64_t n_child, const uint64_t* child_bits,
                                      const int32_t* child_rank, const int32_t* h_child, const int64_t* block_keys, int64_t n_blocks,
                                      const uint64_t* block_bits, const int32_t* block_rank, const int32_t* h_block, int32_t block_log2,
                                      const int32_t* mode, const int32_t* off, const int32_t* v, int32_t channels, int32_t colour,
                                      const int32_t* match, const int32_t* ref_values, int64_t n_ref, const int32_t* coef,
                                      int64_t row_base, int64_t rows_total, int32_t* child_v, int32_t* d_flag, void* stream) {
  const char* what = "pcc_lift_inter_inverse";
  LiftLevel L;
  OctBlocks B;
  if (!lift_last_level(what, keys, n, pitch, bits, rank, h_grid, child_keys, n_child, child_bits, child_rank, h_child, &L)) return PCC_EINVAL;
  if (!oct_blocks(what, block_keys, n_blocks, block_bits, block_rank, h_block, block_log2, &B)) return PCC_EINVAL;
  if (!lift_reference(what, match, ref_values, n_ref)) return PCC_EINVAL;
  PCC_REQUIRE(channels >= 1 && channels <= LIFT_MAX_C && (!colour || channels == 3) && mode && off && v && coef && child_v && d_flag &&
              row_base >= 0 && rows_total > 0 && rows_total < (1ll << 26), "pcc_lift_inter_inverse: bad arguments");
  k_lift_inter_inverse<<<(unsigned)pcc_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(L, B, mode, off, v, channels, colour, match, ref_values,
                                                                                  (int)n_ref, coef, row_base, rows_total, child_v, d_flag);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}
