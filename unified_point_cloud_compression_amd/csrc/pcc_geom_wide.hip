// Wide block motion of the inter coders, device side (DESIGN.md section 7e "Wide search", stream formats 0xAA / 0xB7 / 0xB8): the
// exhaustive search of pcc_geom_inter.hip over [-search, search]^3 for search up to 7 (3375 vectors), where a candidate table in
// the kernel arguments, a byte per index and an LDS atomic per (row, candidate) no longer serve.  A vector is a DISPLACEMENT here,
// packed (dx + 8) | (dy + 8) << 4 | (dz + 8) << 8 (the packing of InterCands), never an index.
//   k_wide_motion      one 256-thread workgroup per block.  The reference around the block is staged in LDS as z-bit columns
//                      (30 x 30 words at search 7; grid index: one bit field of the bitmap per column, else probed cell by cell),
//                      the block's non-empty z rows are compacted into LDS (most of the 256 rows of a surface block are empty), then
//                      thread (dx, dy) walks the rows and keeps 2 search + 1 counts in registers, count[dz] += popc(row & (col >>
//                      (search - dz))).  The winner is the maximum of the key (count, -|v|^2, -lexicographic rank) over the
//                      workgroup: most matches, then the shorter vector, then the lexicographically smaller one -- the "lowest
//                      index of candidates(search)" of the narrow kernel.  No atomics; every sum is an integer.
//   k_wide_block_bits  k_inter_block_bits with a displacement per block; a component outside +-search sets *d_bad, counts as zero
//   k_wide_pack        components [n, 3] (dx + search, ...) -> displacements; a component above 2 search sets *d_bad, counts as zero
//   k_wide_unpack      displacements -> components [n, 3], what the vector list of an 0xAA stream codes
#include "pcc_geom_inter.h"

static constexpr int WIDE_MAX_SEARCH = 7;
static constexpr int WIDE_K = 2 * WIDE_MAX_SEARCH + 1;      // vectors per axis at most
static constexpr int WIDE_WIN = 16 + 2 * WIDE_MAX_SEARCH;   // window columns per axis at most (and z bits per column: fits a word)
// Row pitch of the window in LDS.  Thread t holds (dx, dy) = (t >> 4, t & 15), so the 32 lanes that share a ds_read_b32 cycle read
// two runs of 16 consecutive words one pitch apart: at 48 words (16 mod 32) the two runs fall on disjoint banks.
static constexpr int WIDE_PITCH = 48;

__global__ void __launch_bounds__(256) k_wide_motion(const int64_t* __restrict__ bkeys, int bl, const unsigned long long* __restrict__ cur,
                                                     const int64_t* __restrict__ rkeys, int nr, PccGrid rg, int ox, int oy, int oz,
                                                     int search, int* __restrict__ counts, int* __restrict__ disp) {
  __shared__ unsigned win[WIDE_WIN * WIDE_PITCH];
  __shared__ unsigned rows[256];                         // a non-empty row: its z bits | (lx * S + ly) << 16
  __shared__ int wave_rows[4];
  __shared__ unsigned long long wave_best[4];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t key = bkeys[b];
  // the reference around the block, [origin + block - R, origin + block + S + R)^3, one word of z bits per (x, y) column
  const int S = 1 << bl, Wd = S + 2 * search, K = 2 * search + 1;
  const int wx0 = ox + pcc_key_x(key) - search, wy0 = oy + pcc_key_y(key) - search, wz0 = oz + pcc_key_z(key) - search;
  for (int c = t; c < Wd * Wd; c += 256) {
    const int cx = c / Wd, cy = c % Wd, x = wx0 + cx, y = wy0 + cy;
    unsigned f = 0;
    if (nr > 0 && rg.bits) {
      const int gx = x - rg.lat.lo[0], gy = y - rg.lat.lo[1], za = wz0 - rg.lat.lo[2];
      if (gx >= 0 && gy >= 0 && gx < rg.lat.dims[0] && gy < rg.lat.dims[1]) {
        const int zlo = za < 0 ? 0 : za, zhi = za + Wd < rg.lat.dims[2] ? za + Wd : rg.lat.dims[2];
        if (zlo < zhi) {
          const long long cell = ((long long)gx * rg.lat.dims[1] + gy) * rg.lat.dims[2] + zlo;
          const long long wi = cell >> 6;
          const int sh = (int)(cell & 63), nbit = zhi - zlo;          // nbit <= 30
          unsigned long long f64 = rg.bits[wi] >> sh;
          if (sh + nbit > 64) f64 |= rg.bits[wi + 1] << (64 - sh);
          f = ((unsigned)f64 & ((1u << nbit) - 1u)) << (zlo - za);
        }
      }
    } else if (nr > 0) {
      for (int z = 0; z < Wd; ++z)
        if (inter_has(rg, rkeys, nr, x, y, wz0 + z)) f |= 1u << z;
    }
    win[cx * WIDE_PITCH + cy] = f;
  }
  // the block's own rows (S z bits at bit (lx * S + ly) * S of the finest tier), the non-empty ones packed to the front in row order
  const unsigned long long* cw = cur + (int64_t)b * INTER_PYR + inter_tier(bl);
  unsigned row = 0;
  if (t < S * S) {
    const int at = t << bl;
    row = (unsigned)(cw[at >> 6] >> (at & 63)) & ((1u << S) - 1u);
  }
  const unsigned long long full = __ballot(row != 0);
  if (lane == 0) wave_rows[wave] = __popcll(full);
  __syncthreads();
  int before = __popcll(full & ((1ull << lane) - 1ull)), n_rows = 0;
  for (int w = 0; w < 4; ++w) {
    if (w < wave) before += wave_rows[w];
    n_rows += wave_rows[w];
  }
  if (row) rows[before] = row | ((unsigned)t << 16);
  __syncthreads();
  // thread (dx, dy): one window column per row, 2 search + 1 counts
  const int ix = t >> 4, iy = t & 15;
  const bool live = ix < K && iy < K;
  int acc[WIDE_K];
#pragma unroll
  for (int k = 0; k < WIDE_K; ++k) acc[k] = 0;
  if (live) {
    const int dx = ix - search, dy = iy - search;
    for (int i = 0; i < n_rows; ++i) {
      const unsigned r = rows[i], bitsz = r & 0xFFFFu;
      const int lx = (int)(r >> 16) >> bl, ly = (int)(r >> 16) & (S - 1);
      const unsigned col = win[(lx - dx + search) * WIDE_PITCH + (ly - dy + search)];
#pragma unroll
      for (int k = 0; k < WIDE_K; ++k)
        if (k < K) acc[k] += __popc(bitsz & (col >> (2 * search - k)));      // dz = k - search
    }
  }
  unsigned long long best = 0;                          // count << 24 | (255 - |v|^2) << 12 | (4095 - rank): a live thread's is > 0
  if (live) {
    const int dx = ix - search, dy = iy - search, rank0 = (ix * K + iy) * K;
#pragma unroll
    for (int k = 0; k < WIDE_K; ++k)
      if (k < K) {
        const int dz = k - search, norm = dx * dx + dy * dy + dz * dz;
        const unsigned long long v = ((unsigned long long)acc[k] << 24) | ((unsigned long long)(255 - norm) << 12) | (unsigned long long)(4095 - (rank0 + k));
        best = v > best ? v : best;
        if (counts) counts[(int64_t)b * K * K * K + rank0 + k] = acc[k];
      }
  }
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned long long o = __shfl_xor(best, d);
    best = o > best ? o : best;
  }
  if (lane == 0) wave_best[wave] = best;
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < 4; ++w) best = wave_best[w] > best ? wave_best[w] : best;
    const int rank = 4095 - (int)(best & 4095u);
    disp[b] = wide_pack(rank / (K * K) - search, (rank / K) % K - search, rank % K - search);
  }
}

__global__ void __launch_bounds__(64) k_wide_block_bits(const int64_t* __restrict__ bkeys, int bl, const int64_t* __restrict__ skeys, int ns,
                                                        PccGrid sg, int ox, int oy, int oz, const int* __restrict__ disp, int search,
                                                        unsigned long long* __restrict__ pyr, int* __restrict__ d_bad) {
  __shared__ unsigned long long w[INTER_PYR];
  const int b = blockIdx.x, lane = threadIdx.x;
  for (int t = lane; t < INTER_PYR; t += 64) w[t] = 0;
  __syncthreads();
  const int64_t key = bkeys[b];
  int dx, dy, dz;
  if (!wide_unpack(disp[b], search, dx, dy, dz) && lane == 0) atomicOr(d_bad, 1);
  const int x0 = ox + pcc_key_x(key) - dx, y0 = oy + pcc_key_y(key) - dy, z0 = oz + pcc_key_z(key) - dz;
  INTER_PROBE_FINEST(w, lane, bl, sg, skeys, ns, x0, y0, z0)
  __syncthreads();
  for (int e = bl - 1; e >= 0; --e) {
    const int ce = 1 << (3 * e), se = (1 << e) - 1;
    for (int c = lane; c < ce; c += 64) {
      const int lx = c >> (2 * e), ly = (c >> e) & se, lz = c & se;
      int any = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int cc = ((2 * lx + ((j >> 2) & 1)) << (2 * (e + 1))) | ((2 * ly + ((j >> 1) & 1)) << (e + 1)) | (2 * lz + (j & 1));
        any |= (int)((w[inter_tier(e + 1) + (cc >> 6)] >> (cc & 63)) & 1ull);
      }
      if (any) atomicOr(&w[inter_tier(e) + (c >> 6)], 1ull << (c & 63));
    }
    __syncthreads();
  }
  for (int t = lane; t < INTER_PYR; t += 64) pyr[(int64_t)b * INTER_PYR + t] = w[t];
}

__global__ void __launch_bounds__(256) k_wide_pack(const int* __restrict__ comps, int n, int search, int* __restrict__ disp,
                                                   int* __restrict__ d_bad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int c[3];
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    c[a] = comps[3 * (int64_t)i + a];
    if (c[a] < 0 || c[a] > 2 * search) { ok = false; c[a] = search; }
  }
  if (!ok) atomicOr(d_bad, 1);
  disp[i] = wide_pack(c[0] - search, c[1] - search, c[2] - search);
}

__global__ void __launch_bounds__(256) k_wide_unpack(const int* __restrict__ disp, int n, int search, int* __restrict__ comps) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int dx, dy, dz;
  wide_unpack(disp[i], search, dx, dy, dz);
  comps[3 * (int64_t)i] = dx + search; comps[3 * (int64_t)i + 1] = dy + search; comps[3 * (int64_t)i + 2] = dz + search;
}

// ---- host entry points --------------------------------------------------------------------------------------------------
static int wide_search_ok(int search, const char* who) {
  PCC_REQUIRE(search >= 1 && search <= WIDE_MAX_SEARCH, "%s: search range %d outside 1..%d", who, search, WIDE_MAX_SEARCH);
  return PCC_OK;
}

extern "C" int pcc_geom_wide_motion(const int64_t* block_keys, int64_t n_blocks, int32_t block_log2, const uint64_t* cur_pyramid,
                                    const int64_t* ref_keys, int64_t n_ref, const uint64_t* ref_bits, const int32_t* ref_rank,
                                    const int32_t* h_ref, int32_t ox, int32_t oy, int32_t oz, int32_t search, int32_t* counts,
                                    int32_t* disp, void* stream) {
  PCC_REQUIRE(block_keys && cur_pyramid && disp && n_blocks > 0 && n_blocks < (1ll << 24), "pcc_geom_wide_motion: bad arguments");
  PCC_REQUIRE(block_log2 >= 0 && block_log2 <= 4, "pcc_geom_wide_motion: block_log2 %d outside 0..4", block_log2);
  PCC_REQUIRE(n_ref >= 0 && n_ref < (1ll << 31) && (n_ref == 0 || ref_keys), "pcc_geom_wide_motion: bad reference set");
  PCC_REQUIRE(inter_origin_ok(ox, oy, oz), "pcc_geom_wide_motion: origin outside the 16-bit key range");
  PCC_TRY(wide_search_ok(search, "pcc_geom_wide_motion"));
  PccGrid g;
  PCC_TRY(pcc_grid_from_host(n_ref ? ref_bits : nullptr, ref_rank, h_ref, "pcc_geom_wide_motion", &g));
  PCC_REQUIRE(!g.bits || h_ref[6] == 1, "pcc_geom_wide_motion: the reference grid must have pitch 1");
  k_wide_motion<<<(unsigned)n_blocks, 256, 0, (hipStream_t)stream>>>(block_keys, block_log2, (const unsigned long long*)cur_pyramid, ref_keys,
                                                                    (int)n_ref, g, ox, oy, oz, search, counts, disp);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_geom_wide_block_bits(const int64_t* block_keys, int64_t n_blocks, int32_t block_log2, const int64_t* src_keys,
                                        int64_t n_src, const uint64_t* src_bits, const int32_t* src_rank, const int32_t* h_src,
                                        int32_t ox, int32_t oy, int32_t oz, const int32_t* disp, int32_t search, uint64_t* pyramid,
                                        int32_t* d_bad, void* stream) {
  PCC_REQUIRE(block_keys && disp && pyramid && d_bad && n_blocks > 0 && n_blocks < (1ll << 24), "pcc_geom_wide_block_bits: bad arguments");
  PCC_REQUIRE(block_log2 >= 0 && block_log2 <= 4, "pcc_geom_wide_block_bits: block_log2 %d outside 0..4", block_log2);
  PCC_REQUIRE(n_src >= 0 && n_src < (1ll << 31) && (n_src == 0 || src_keys), "pcc_geom_wide_block_bits: bad source set");
  PCC_REQUIRE(inter_origin_ok(ox, oy, oz), "pcc_geom_wide_block_bits: origin outside the 16-bit key range");
  PCC_TRY(wide_search_ok(search, "pcc_geom_wide_block_bits"));
  PccGrid g;
  PCC_TRY(pcc_grid_from_host(n_src ? src_bits : nullptr, src_rank, h_src, "pcc_geom_wide_block_bits", &g));
  PCC_REQUIRE(!g.bits || h_src[6] == 1, "pcc_geom_wide_block_bits: the source grid must have pitch 1");
  k_wide_block_bits<<<(unsigned)n_blocks, 64, 0, (hipStream_t)stream>>>(block_keys, block_log2, src_keys, (int)n_src, g, ox, oy, oz, disp, search,
                                                                       (unsigned long long*)pyramid, d_bad);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_geom_wide_pack(const int32_t* comps, int64_t n, int32_t search, int32_t* disp, int32_t* d_bad, void* stream) {
  PCC_REQUIRE(comps && disp && d_bad && n > 0 && n < (1ll << 24), "pcc_geom_wide_pack: bad arguments");
  PCC_TRY(wide_search_ok(search, "pcc_geom_wide_pack"));
  k_wide_pack<<<(unsigned)pcc_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(comps, (int)n, search, disp, d_bad);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_geom_wide_unpack(const int32_t* disp, int64_t n, int32_t search, int32_t* comps, void* stream) {
  PCC_REQUIRE(disp && comps && n > 0 && n < (1ll << 24), "pcc_geom_wide_unpack: bad arguments");
  PCC_TRY(wide_search_ok(search, "pcc_geom_wide_unpack"));
  k_wide_unpack<<<(unsigned)pcc_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(disp, (int)n, search, comps);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}
