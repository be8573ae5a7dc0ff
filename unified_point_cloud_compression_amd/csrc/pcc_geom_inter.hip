// Inter-frame lossless geometry, device side (stream format 0xA8): the octree coder of pcc_geom.hip with a
// block-motion-compensated reference cloud as a second source of context for the levels at and below the block pitch.
//   k_inter_block_bits   per block (a node of the level at pitch 2^bl, bl <= 4) the occupancy pyramid of a source set displaced by
//                        the block's vector: 75 words, bit (lx << 2e | ly << e | lz) of tier e = the cell of side 2^(bl - e) at
//                        (lx, ly, lz) holds a source voxel.  vec == NULL: no displacement (the current frame's own pyramid).
//   k_inter_motion       per block the match count of every candidate vector and the arg-max (most matches, lowest index): the
//                        reference around the block is staged in LDS as z-bit columns, a count is popcounts of row AND column
//   k_inter_occ_ctx      node -> face-neighbour context, `present` (the node's cell in the predicted pyramid), r (the predicted
//                        node's child byte) and, on the encoder, the occupancy byte s and the symbol (rho^-1(s ^ r) when present)
//   k_inter_map          byte <-> symbol of a level given (idx, r): the decoder's inverse map, and the forward map of its raw levels
//   k_inter_hist         (row, symbol) histogram over the 128 table rows + the two class histograms; LDS holds 32 rows per workgroup
//   k_inter_tables       the 128 frequency rows of a level and the rANS decoder table, one workgroup per row
// The prediction is never a key list: a block's pyramid is addressed by the block's row in its level, so every size follows from
// the node count of that level, which the stream header gives.  The reference is probed in absolute coordinates through its
// grid index or, without one, by binary search over its keys.  Integers only; every sum is order independent.
#include "pcc_geom_inter.h"

static constexpr int INTER_ROWS = 128;
static constexpr int INTER_HIST = INTER_ROWS * 256;      // [row][symbol], then 8 popcount classes (absent), 9 distance classes (present)
static constexpr int INTER_CLASSES = 17;
static constexpr int INTER_CDF_STRIDE = 258;
static constexpr int INTER_CDF_TOTAL = 64 * 257 + 64 * 258;

struct InterRho { unsigned char rho[256], inv[256]; };   // rho: symbol -> t = s ^ r by (popcount(t), t); inv: t -> symbol

static constexpr InterRho inter_make_rho() {
  InterRho t{};
  int j = 0;
  for (int d = 0; d <= 8; ++d)
    for (int v = 0; v < 256; ++v) {
      int p = 0;
      for (int b = 0; b < 8; ++b) p += (v >> b) & 1;
      if (p == d) { t.rho[j] = (unsigned char)v; t.inv[v] = (unsigned char)j; ++j; }
    }
  return t;
}
__constant__ InterRho INTER_RHO = inter_make_rho();

__device__ __forceinline__ int inter_bit(const unsigned long long* w, int e, int lx, int ly, int lz) {
  const int c = (lx << (2 * e)) | (ly << e) | lz;
  return (int)((w[inter_tier(e) + (c >> 6)] >> (c & 63)) & 1ull);
}

// a node of a level of the coder (origin-relative cells, never negative)
__device__ inline bool inter_node(const PccGrid& g, const int64_t* __restrict__ keys, int n, int x, int y, int z) {
  if ((x | y | z) < 0 || x >= (int)PCC_BIAS || y >= (int)PCC_BIAS || z >= (int)PCC_BIAS) return false;
  return pcc_lookup(g, keys, n, pcc_key_pack(0, x, y, z)) >= 0;
}

__global__ void __launch_bounds__(64) k_inter_block_bits(const int64_t* __restrict__ bkeys, int bl, const int64_t* __restrict__ skeys, int ns,
                                                         PccGrid sg, int ox, int oy, int oz, const int* __restrict__ vec, InterCands cands,
                                                         unsigned long long* __restrict__ pyr, int* __restrict__ d_bad) {
  __shared__ unsigned long long w[INTER_PYR];
  const int b = blockIdx.x, lane = threadIdx.x;
  for (int t = lane; t < INTER_PYR; t += 64) w[t] = 0;
  __syncthreads();
  const int64_t key = bkeys[b];
  int dx = 0, dy = 0, dz = 0;
  if (vec) {
    int j = vec[b];
    if (j < 0 || j >= cands.n) { if (lane == 0) atomicOr(d_bad, 1); j = 0; }
    inter_cand(cands, j, dx, dy, dz);
  }
  const int x0 = ox + pcc_key_x(key) - dx, y0 = oy + pcc_key_y(key) - dy, z0 = oz + pcc_key_z(key) - dz;
  INTER_PROBE_FINEST(w, lane, bl, sg, skeys, ns, x0, y0, z0)
  __syncthreads();
  for (int e = bl - 1; e >= 0; --e) {
    const int ce = 1 << (3 * e), se = (1 << e) - 1;
    for (int c = lane; c < ce; c += 64) {
      const int lx = c >> (2 * e), ly = (c >> e) & se, lz = c & se;
      int any = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) any |= inter_bit(w, e + 1, 2 * lx + ((j >> 2) & 1), 2 * ly + ((j >> 1) & 1), 2 * lz + (j & 1));
      if (any) atomicOr(&w[inter_tier(e) + (c >> 6)], 1ull << (c & 63));
    }
    __syncthreads();
  }
  for (int t = lane; t < INTER_PYR; t += 64) pyr[(int64_t)b * INTER_PYR + t] = w[t];
}

__global__ void __launch_bounds__(64) k_inter_motion(const int64_t* __restrict__ bkeys, int bl, const unsigned long long* __restrict__ cur,
                                                     const int64_t* __restrict__ rkeys, int nr, PccGrid rg, int ox, int oy, int oz,
                                                     int search, InterCands cands, int* __restrict__ counts, int* __restrict__ vec) {
  __shared__ int cnt[128];
  __shared__ unsigned win[20 * 20];                      // (16 + 2 * 2)^2 columns at most
  const int b = blockIdx.x, lane = threadIdx.x;
  cnt[lane] = 0;
  cnt[lane + 64] = 0;
  __syncthreads();
  const int64_t key = bkeys[b];
  // the reference around the block, [origin + block - R, origin + block + S + R)^3, as one word of z bits per (x, y) column: with a
  // grid index a column is one bit field of the bitmap (z is the fastest axis of the lattice), without one it is probed cell by cell
  const int S = 1 << bl, Wd = S + 2 * search;
  const int wx0 = ox + pcc_key_x(key) - search, wy0 = oy + pcc_key_y(key) - search, wz0 = oz + pcc_key_z(key) - search;
  for (int c = lane; c < Wd * Wd; c += 64) {
    const int x = wx0 + c / Wd, y = wy0 + c % Wd;
    unsigned f = 0;
    if (nr > 0 && rg.bits) {
      const int gx = x - rg.lat.lo[0], gy = y - rg.lat.lo[1], za = wz0 - rg.lat.lo[2];
      if (gx >= 0 && gy >= 0 && gx < rg.lat.dims[0] && gy < rg.lat.dims[1]) {
        const int zlo = za < 0 ? 0 : za, zhi = za + Wd < rg.lat.dims[2] ? za + Wd : rg.lat.dims[2];
        if (zlo < zhi) {
          const long long cell = ((long long)gx * rg.lat.dims[1] + gy) * rg.lat.dims[2] + zlo;
          const long long wi = cell >> 6;
          const int sh = (int)(cell & 63), nbit = zhi - zlo;
          unsigned long long f64 = rg.bits[wi] >> sh;
          if (sh + nbit > 64) f64 |= rg.bits[wi + 1] << (64 - sh);
          f = ((unsigned)f64 & ((1u << nbit) - 1u)) << (zlo - za);
        }
      }
    } else if (nr > 0) {
      for (int t = 0; t < Wd; ++t)
        if (inter_has(rg, rkeys, nr, x, y, wz0 + t)) f |= 1u << t;
    }
    win[c] = f;
  }
  __syncthreads();
  // the block's own voxels, row by row (S z bits at bit (lx * S + ly) * S of the finest tier), against the displaced columns
  const unsigned long long* cw = cur + (int64_t)b * INTER_PYR + inter_tier(bl);
  const unsigned mask = (1u << S) - 1u;
  for (int r = lane; r < S * S; r += 64) {
    const int at = r << bl;
    const unsigned row = (unsigned)(cw[at >> 6] >> (at & 63)) & mask;
    if (!row) continue;
    const int lx = r >> bl, ly = r & (S - 1);
    for (int j = 0; j < cands.n; ++j) {
      int dx, dy, dz;
      inter_cand(cands, j, dx, dy, dz);
      const int hits = __popc(row & (win[(lx - dx + search) * Wd + (ly - dy + search)] >> (search - dz)));
      if (hits) atomicAdd(&cnt[j], hits);
    }
  }
  __syncthreads();
  if (counts)
    for (int j = lane; j < cands.n; j += 64) counts[(int64_t)b * cands.n + j] = cnt[j];
  if (lane == 0) {
    int best = 0;
    for (int j = 1; j < cands.n; ++j)
      if (cnt[j] > cnt[best]) best = j;
    vec[b] = best;
  }
}

__global__ void __launch_bounds__(256) k_inter_occ_ctx(const int64_t* __restrict__ keys, int n, PccGrid g, int pitch,
                                                       const int64_t* __restrict__ ckeys, int nc, PccGrid cg,
                                                       const int64_t* __restrict__ bkeys, int nb, PccGrid bg, int bl,
                                                       const unsigned long long* __restrict__ pyr, int* __restrict__ byte,
                                                       int* __restrict__ sym, int* __restrict__ r_out, int* __restrict__ idx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t key = keys[i];
  const int x = pcc_key_x(key), y = pcc_key_y(key), z = pcc_key_z(key);
  int c = 0;
  c |= inter_node(g, keys, n, x - pitch, y, z) ? 1 : 0;
  c |= inter_node(g, keys, n, x + pitch, y, z) ? 2 : 0;
  c |= inter_node(g, keys, n, x, y - pitch, z) ? 4 : 0;
  c |= inter_node(g, keys, n, x, y + pitch, z) ? 8 : 0;
  c |= inter_node(g, keys, n, x, y, z - pitch) ? 16 : 0;
  c |= inter_node(g, keys, n, x, y, z + pitch) ? 32 : 0;
  // the node's cell in its block's predicted pyramid (a key a damaged stream put outside every block counts as absent)
  const int bm = (1 << bl) - 1, sh = 31 - __clz(pitch), e = bl - sh;
  int present = 0, r = 0;
  if ((x | y | z) >= 0 && x < (int)PCC_BIAS && y < (int)PCC_BIAS && z < (int)PCC_BIAS) {
    const int row = pcc_lookup(bg, bkeys, nb, pcc_key_pack(0, x & ~bm, y & ~bm, z & ~bm));
    if (row >= 0 && row < nb) {
      const unsigned long long* w = pyr + (int64_t)row * INTER_PYR;
      const int lx = (x & bm) >> sh, ly = (y & bm) >> sh, lz = (z & bm) >> sh;
      present = inter_bit(w, e, lx, ly, lz);
      if (present)
#pragma unroll
        for (int j = 0; j < 8; ++j) r |= inter_bit(w, e + 1, 2 * lx + ((j >> 2) & 1), 2 * ly + ((j >> 1) & 1), 2 * lz + (j & 1)) << j;
    }
  }
  idx[i] = c + 64 * present;
  if (r_out) r_out[i] = r;
  if (byte) {
    const int cp = pitch >> 1;
    int s = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      s |= inter_node(cg, ckeys, nc, x + ((j >> 2) & 1) * cp, y + ((j >> 1) & 1) * cp, z + (j & 1) * cp) ? (1 << j) : 0;
    byte[i] = s;
    sym[i] = present ? (int)INTER_RHO.inv[(s ^ r) & 255] : s;
  }
}

// inverse != 0: symbol -> byte (absent: the byte itself, 1..255; present: rho(sym) ^ r, never 0); else byte -> symbol.
// What cannot occur sets *d_bad and counts as byte 1.
__global__ void __launch_bounds__(256) k_inter_map(const int* __restrict__ in, const int* __restrict__ idx, const int* __restrict__ r, int n,
                                                   int inverse, int* __restrict__ out, int* __restrict__ d_bad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int v = in[i], present = (idx[i] >> 6) & 1, p = r[i] & 255;
  int o;
  if (!present) {
    o = v;
    if (v < 1 || v > 255) { atomicOr(d_bad, 1); o = 1; }
  } else if (inverse) {
    o = (v < 0 || v > 255) ? 0 : ((int)INTER_RHO.rho[v] ^ p);
    if (o == 0) { atomicOr(d_bad, 1); o = 1; }
  } else {
    if (v < 1 || v > 255) { atomicOr(d_bad, 1); o = (int)INTER_RHO.inv[1 ^ p]; }
    else o = (int)INTER_RHO.inv[v ^ p];
  }
  out[i] = o;
}

__global__ void __launch_bounds__(256) k_inter_hist(const int* __restrict__ sym, const int* __restrict__ idx, int n,
                                                    unsigned* __restrict__ hist, int* __restrict__ d_bad) {
  __shared__ unsigned h[32 * 256];
  __shared__ unsigned cls[INTER_CLASSES];
  const int q = blockIdx.y;                                   // rows 32 q .. 32 q + 31
  for (int t = threadIdx.x; t < 32 * 256; t += blockDim.x) h[t] = 0;
  if (threadIdx.x < INTER_CLASSES) cls[threadIdx.x] = 0;
  __syncthreads();
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int s = sym[i], row = idx[i] & (INTER_ROWS - 1);
    if (s < (row < 64 ? 1 : 0) || s > 255) { atomicOr(d_bad, 1); continue; }
    if ((row >> 5) == q) atomicAdd(&h[(row & 31) * 256 + s], 1u);
  }
  __syncthreads();
  for (int t = threadIdx.x; t < 32 * 256; t += blockDim.x) {
    const unsigned v = h[t];
    if (!v) continue;
    const int row = q * 32 + (t >> 8), s = t & 255;
    atomicAdd(&hist[row * 256 + s], v);
    atomicAdd(&cls[row < 64 ? __popc(s) - 1 : 8 + __popc((int)INTER_RHO.rho[s])], v);
  }
  __syncthreads();
  if (threadIdx.x < INTER_CLASSES && cls[threadIdx.x]) atomicAdd(&hist[INTER_HIST + threadIdx.x], cls[threadIdx.x]);
}

// ---- the 128-row table family on the device: the integer rule of geometry.derive_tables_inter ------------
// One workgroup per row, thread s <-> live symbol s of the row's population (absent rows: byte s + 1, 255 live; present rows:
// symbol s, 256 live).  The bounds on the intermediates are those of k_geom_tables (pcc_geom.hip).
struct InterClassHist { unsigned long long v[INTER_CLASSES]; };

__device__ inline unsigned long long inter_block_sum(unsigned long long x, unsigned long long* red) {
  __syncthreads();
  red[threadIdx.x] = x;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) red[threadIdx.x] += red[threadIdx.x + d];
    __syncthreads();
  }
  return red[0];
}

__global__ void __launch_bounds__(256) k_inter_tables(const unsigned long long* __restrict__ A, InterClassHist ch, int* __restrict__ cdf,
                                                      int* __restrict__ blob) {
  __shared__ unsigned long long red[256];
  __shared__ unsigned long long E[9];
  __shared__ unsigned long long R[9];
  __shared__ int cum[INTER_CDF_STRIDE];
  const int c = blockIdx.x, s = threadIdx.x;
  const int fam = c >> 6, base = fam * 64, nsym = fam ? 256 : 255, classes = fam ? 9 : 8;
  const bool live = s < nsym;
  const int b = fam ? s : s + 1;
  const int k = fam ? __popc((int)INTER_RHO.rho[s]) : __popc(b & 255) - 1;
  const unsigned long long* hist = ch.v + (fam ? 8 : 0);
  unsigned long long col = 0;
  if (live) for (int cc = 0; cc < 64; ++cc) col += A[(base + cc) * 256 + b];
  const unsigned long long total = inter_block_sum(col, red);
  int shift = 0;
  while ((total >> shift) >= (1ull << 20)) ++shift;
  unsigned long long G = 0;
  if (live) for (int cc = 0; cc < 64; ++cc) G += A[(base + cc) * 256 + b] >> shift;
  const unsigned long long gt = inter_block_sum(G, red) + (unsigned long long)nsym;
  if (s < 9) E[s] = 0;
  __syncthreads();
  if (live) atomicAdd(&E[k], G + 1);
  __syncthreads();
  if (s < classes) {
    unsigned long long ptot = 0, r = 0;
    for (int j = 0; j < classes; ++j) ptot += hist[j];
    if (ptot == 0) r = 1;                                    // a population without a node in this level: no class correction
    else if (hist[s] > 0) {
      const unsigned long long num = hist[s] * gt, den = ptot * E[s];
      unsigned long long q = num / den, rem = num % den;
      if (q >= (1ull << 8)) r = 1ull << 20;
      else {
        for (int t = 0; t < 12; ++t) {
          rem <<= 1; q <<= 1;
          if (rem >= den) { rem -= den; q |= 1; }
        }
        r = q < 1 ? 1 : (q > (1ull << 20) ? (1ull << 20) : q);
      }
    }
    R[s] = r;
  }
  __syncthreads();
  const unsigned long long N = live ? (A[c * 256 + b] >> shift) : 0;
  const unsigned long long W = live ? N * gt + 16ull * (G + 1) : 0;
  const unsigned long long wsum = inter_block_sum(W, red);
  const unsigned long long w = live ? (1 + (W << 20) / wsum) * R[k] : 0;
  const unsigned long long vsum = inter_block_sum(w, red);
  unsigned long long f = live ? 1 + w * (65535ull - (unsigned long long)nsym) / vsum : 0;
  const unsigned long long fsum = inter_block_sum(f, red);
  __syncthreads();
  red[s] = live ? ((f << 8) | (unsigned long long)(255 - s)) : 0;      // first largest frequency: max over (f << 8 | 255 - s)
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if (s < d && red[s + d] > red[s]) red[s] = red[s + d];
    __syncthreads();
  }
  if (live && (int)(255 - (red[0] & 255)) == s) f += 65535ull - fsum;
  __syncthreads();
  cum[s] = (int)f;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const int v = s >= d ? cum[s - d] : 0;
    __syncthreads();
    cum[s] += v;
    __syncthreads();
  }
  const int mine = cum[s];                       // cdf[s + 1] of a live symbol
  __syncthreads();
  if (s == 0) { cum[0] = 0; cum[256] = 0; cum[257] = 0; }
  __syncthreads();
  if (live) cum[s + 1] = mine;
  __syncthreads();
  if (s == 0) cum[nsym + 1] = 65536;
  __syncthreads();
  const int size = nsym + 2;
  for (int v = s; v < INTER_CDF_STRIDE; v += 256) cdf[c * INTER_CDF_STRIDE + v] = cum[v];
  // decoder table blob of pcc_rans_build_dec_table: int32 rows | int32 total | int32 row_off[129] | u16 lut[128 * 256] | u16 cdf16[total]
  unsigned short* lut = (unsigned short*)(blob + 2 + INTER_ROWS + 1);
  unsigned short* cdf16 = lut + INTER_ROWS * 256;
  const int row_off = c < 64 ? c * 257 : 64 * 257 + (c - 64) * 258;
  for (int v = s; v < size; v += 256) cdf16[row_off + v] = (unsigned short)(cum[v] & 0xFFFF);
  int lo = 0, hi = size - 2;                     // largest v in [0, size - 2] with cdf[v] <= s * 256
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (cum[mid] <= s * 256) lo = mid; else hi = mid - 1;
  }
  lut[c * 256 + s] = (unsigned short)lo;
  if (c == 0) {
    if (s == 0) { blob[0] = INTER_ROWS; blob[1] = INTER_CDF_TOTAL; }
    if (s <= INTER_ROWS) blob[2 + s] = s < 64 ? s * 257 : 64 * 257 + (s - 64) * 258;
  }
}

// ---- host entry points --------------------------------------------------------------------------------------------------
extern "C" int32_t pcc_geom_inter_pyramid_words(void) { return INTER_PYR; }

extern "C" int32_t pcc_geom_inter_candidates(int32_t search, int32_t* h_out /*[n, 3]*/) {
  InterCands c;
  if (inter_cands(search, "pcc_geom_inter_candidates", &c) != PCC_OK) return -1;
  if (h_out)
    for (int i = 0; i < c.n; ++i) {
      h_out[3 * i] = (c.v[i] & 15) - 8; h_out[3 * i + 1] = ((c.v[i] >> 4) & 15) - 8; h_out[3 * i + 2] = ((c.v[i] >> 8) & 15) - 8;
    }
  return c.n;
}

extern "C" int pcc_geom_inter_block_bits(const int64_t* block_keys, int64_t n_blocks, int32_t block_log2, const int64_t* src_keys,
                                         int64_t n_src, const uint64_t* src_bits, const int32_t* src_rank, const int32_t* h_src,
                                         int32_t ox, int32_t oy, int32_t oz, const int32_t* vec, int32_t search, uint64_t* pyramid,
                                         int32_t* d_bad, void* stream) {
  PCC_REQUIRE(block_keys && pyramid && d_bad && n_blocks > 0 && n_blocks < (1ll << 24), "pcc_geom_inter_block_bits: bad arguments");
  PCC_REQUIRE(block_log2 >= 0 && block_log2 <= 4, "pcc_geom_inter_block_bits: block_log2 %d outside 0..4", block_log2);
  PCC_REQUIRE(n_src >= 0 && n_src < (1ll << 31) && (n_src == 0 || src_keys), "pcc_geom_inter_block_bits: bad source set");
  PCC_REQUIRE(inter_origin_ok(ox, oy, oz), "pcc_geom_inter_block_bits: origin outside the 16-bit key range");
  InterCands c;
  PCC_TRY(inter_cands(search, "pcc_geom_inter_block_bits", &c));
  PccGrid g;
  PCC_TRY(pcc_grid_from_host(n_src ? src_bits : nullptr, src_rank, h_src, "pcc_geom_inter_block_bits", &g));
  PCC_REQUIRE(!g.bits || h_src[6] == 1, "pcc_geom_inter_block_bits: the source grid must have pitch 1");
  k_inter_block_bits<<<(unsigned)n_blocks, 64, 0, (hipStream_t)stream>>>(block_keys, block_log2, src_keys, (int)n_src, g, ox, oy, oz, vec, c,
                                                                        (unsigned long long*)pyramid, d_bad);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_geom_inter_motion(const int64_t* block_keys, int64_t n_blocks, int32_t block_log2, const uint64_t* cur_pyramid,
                                     const int64_t* ref_keys, int64_t n_ref, const uint64_t* ref_bits, const int32_t* ref_rank,
                                     const int32_t* h_ref, int32_t ox, int32_t oy, int32_t oz, int32_t search, int32_t* counts,
                                     int32_t* vec, void* stream) {
  PCC_REQUIRE(block_keys && cur_pyramid && vec && n_blocks > 0 && n_blocks < (1ll << 24), "pcc_geom_inter_motion: bad arguments");
  PCC_REQUIRE(block_log2 >= 0 && block_log2 <= 4, "pcc_geom_inter_motion: block_log2 %d outside 0..4", block_log2);
  PCC_REQUIRE(n_ref >= 0 && n_ref < (1ll << 31) && (n_ref == 0 || ref_keys), "pcc_geom_inter_motion: bad reference set");
  PCC_REQUIRE(inter_origin_ok(ox, oy, oz), "pcc_geom_inter_motion: origin outside the 16-bit key range");
  InterCands c;
  PCC_TRY(inter_cands(search, "pcc_geom_inter_motion", &c));
  PccGrid g;
  PCC_TRY(pcc_grid_from_host(n_ref ? ref_bits : nullptr, ref_rank, h_ref, "pcc_geom_inter_motion", &g));
  PCC_REQUIRE(!g.bits || h_ref[6] == 1, "pcc_geom_inter_motion: the reference grid must have pitch 1");
  k_inter_motion<<<(unsigned)n_blocks, 64, 0, (hipStream_t)stream>>>(block_keys, block_log2, (const unsigned long long*)cur_pyramid, ref_keys,
                                                                    (int)n_ref, g, ox, oy, oz, search, c, counts, vec);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_geom_inter_occ_ctx(const int64_t* keys, int64_t n, int32_t pitch, const uint64_t* bits, const int32_t* rank,
                                      const int32_t* h_grid, const int64_t* child_keys, int64_t n_child, const uint64_t* child_bits,
                                      const int32_t* child_rank, const int32_t* h_child, const int64_t* block_keys, int64_t n_blocks,
                                      const uint64_t* block_bits, const int32_t* block_rank, const int32_t* h_block, int32_t block_log2,
                                      const uint64_t* pyramid, int32_t* byte, int32_t* sym, int32_t* r, int32_t* idx, void* stream) {
  PCC_REQUIRE(keys && idx && block_keys && pyramid && n > 0 && n < (1ll << 31) && n_blocks > 0 && n_blocks < (1ll << 24),
              "pcc_geom_inter_occ_ctx: bad arguments");
  PCC_REQUIRE(block_log2 >= 0 && block_log2 <= 4 && pcc_is_pow2(pitch) && pitch >= 2 && pitch <= (1 << block_log2),
              "pcc_geom_inter_occ_ctx: pitch %d is not a power of two in [2, 2^block_log2 = %d]", pitch, 1 << block_log2);
  PCC_REQUIRE((byte != nullptr) == (sym != nullptr), "pcc_geom_inter_occ_ctx: byte and sym come together");
  PccGrid g, cg, bg;
  PCC_TRY(pcc_grid_from_host(bits, rank, h_grid, "pcc_geom_inter_occ_ctx", &g));
  PCC_TRY(pcc_grid_from_host(byte ? child_bits : nullptr, child_rank, h_child, "pcc_geom_inter_occ_ctx", &cg));
  PCC_TRY(pcc_grid_from_host(block_bits, block_rank, h_block, "pcc_geom_inter_occ_ctx", &bg));
  PCC_REQUIRE(!h_grid || !bits || h_grid[6] == pitch, "pcc_geom_inter_occ_ctx: the level's grid has another pitch");
  PCC_REQUIRE(!bg.bits || h_block[6] == (1 << block_log2), "pcc_geom_inter_occ_ctx: the block grid has another pitch");
  if (byte) {
    PCC_REQUIRE(child_keys && n_child > 0 && n_child < (1ll << 31), "pcc_geom_inter_occ_ctx: bytes need a child set at half the pitch");
    PCC_REQUIRE(!cg.bits || h_child[6] == pitch / 2, "pcc_geom_inter_occ_ctx: the child grid has another pitch");
  }
  k_inter_occ_ctx<<<(unsigned)pcc_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(keys, (int)n, g, pitch, child_keys, (int)n_child, cg, block_keys,
                                                                              (int)n_blocks, bg, block_log2,
                                                                              (const unsigned long long*)pyramid, byte, sym, r, idx);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_geom_inter_map(const int32_t* in, const int32_t* idx, const int32_t* r, int64_t n, int32_t inverse, int32_t* out,
                                  int32_t* d_bad, void* stream) {
  PCC_REQUIRE(in && idx && r && out && d_bad && n > 0 && n < (1ll << 31), "pcc_geom_inter_map: bad arguments");
  k_inter_map<<<(unsigned)pcc_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(in, idx, r, (int)n, inverse, out, d_bad);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int32_t pcc_geom_inter_hist_words(void) { return INTER_HIST + INTER_CLASSES; }

extern "C" int pcc_geom_inter_hist(const int32_t* sym, const int32_t* idx, int64_t n, uint32_t* hist, int32_t* d_bad, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PCC_REQUIRE(sym && idx && hist && d_bad && n > 0 && n < (1ll << 27), "pcc_geom_inter_hist: bad arguments (n < 2^27)");
  PCC_CHECK_HIP(hipMemsetAsync(hist, 0, (size_t)(INTER_HIST + INTER_CLASSES) * 4, s));
  int64_t blocks = pcc_cdiv(n, 256 * 32);
  if (blocks > 64) blocks = 64;
  k_inter_hist<<<dim3((unsigned)blocks, 4), 256, 0, s>>>(sym, idx, (int)n, hist, d_bad);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int64_t pcc_geom_inter_dec_table_bytes(void) {
  const int64_t b = 8 + 4 * (INTER_ROWS + 1) + 2 * INTER_ROWS * 256 + 2 * INTER_CDF_TOTAL;
  return (b + 15) / 16 * 16;
}

extern "C" int pcc_geom_inter_tables(const uint64_t* state, const uint32_t* h_pop, const uint32_t* h_dist, int32_t* cdf, void* dec_table,
                                     void* stream) {
  PCC_REQUIRE(state && h_pop && h_dist && cdf && dec_table, "pcc_geom_inter_tables: NULL array");
  InterClassHist ch;
  unsigned long long tot = 0;
  for (int k = 0; k < 8; ++k) { ch.v[k] = h_pop[k]; tot += h_pop[k]; }
  for (int k = 0; k < 9; ++k) { ch.v[8 + k] = h_dist[k]; tot += h_dist[k]; }
  PCC_REQUIRE(tot > 0 && tot < (1ull << 31), "pcc_geom_inter_tables: the class histograms must count 1 .. 2^31 - 1 nodes");
  k_inter_tables<<<INTER_ROWS, 256, 0, (hipStream_t)stream>>>((const unsigned long long*)state, ch, cdf, (int*)dec_table);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}
