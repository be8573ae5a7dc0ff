// Lossless geometry coder, device side: a breadth-first octree over one block's voxel set whose levels
// are the set's own stride chain.  The kernels here produce and consume the per-node symbols; the entropy coding itself is the
// rANS stream coder of pcc_rans.hip over an [nodes, 1] symbol matrix with the context as table row.
//   k_geom_occ_ctx      node -> 8-bit child-occupancy byte (bit j = child j in ascending key order: j = dx<<2 | dy<<1 | dz) and
//                       6-bit face-neighbour context (bit 0/1: -x/+x, 2/3: -y/+y, 4/5: -z/+z neighbour exists in the level)
//   k_geom_hist         (context, byte) histogram + popcount histogram of a level, integer atomics reduced in LDS per workgroup
//   k_geom_child_count  children per node (popcount of the byte), flags bytes outside 1..255
//   k_geom_expand       child keys of every node at its scan offset, parent-major (canonical order: pcc_keys_canonicalize_grid)
//   k_geom_finish       cell keys + origin -> absolute keys and int32 [n,3] rows
//   k_geom_tables       a level's 64 frequency rows and the rANS decoder table from the adaptive counts, one workgroup per context
//   k_geom_state_update counts = (counts >> 1) + the level's histogram
// All coordinates of the coder are origin-relative cells in [0, 2^15): every neighbour / child coordinate is range-checked
// before it is packed, so no key field carries into the next.  No kernel reads the bitstream: bytes arrive as int32 symbols
// (decoded by pcc_rans or uploaded raw), are validated here, and every write is bounded by a caller-given capacity.
#include "pcc_common.h"
#include "pcc_conv.h"

static constexpr int GEOM_CTX = 64;
static constexpr int GEOM_HIST = GEOM_CTX * 256;        // global layout [ctx][byte], then 8 popcount counters
static constexpr int GEOM_LDS = GEOM_CTX * 255 + 8;     // byte 0 does not occur: 255 columns per context in LDS (65 312 bytes)

__device__ inline bool geom_has(const PccGrid& g, const int64_t* __restrict__ keys, int n, int x, int y, int z) {
  if ((x | y | z) < 0 || x >= (int)PCC_BIAS || y >= (int)PCC_BIAS || z >= (int)PCC_BIAS) return false;
  return pcc_lookup(g, keys, n, pcc_key_pack(0, x, y, z)) >= 0;
}

__global__ void __launch_bounds__(256) k_geom_occ_ctx(const int64_t* __restrict__ keys, int n, PccGrid g, int pitch,
                                                      const int64_t* __restrict__ ckeys, int nc, PccGrid cg,
                                                      int* __restrict__ sym, int* __restrict__ ctx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t key = keys[i];
  const int x = pcc_key_x(key), y = pcc_key_y(key), z = pcc_key_z(key);
  int c = 0;
  c |= geom_has(g, keys, n, x - pitch, y, z) ? 1 : 0;
  c |= geom_has(g, keys, n, x + pitch, y, z) ? 2 : 0;
  c |= geom_has(g, keys, n, x, y - pitch, z) ? 4 : 0;
  c |= geom_has(g, keys, n, x, y + pitch, z) ? 8 : 0;
  c |= geom_has(g, keys, n, x, y, z - pitch) ? 16 : 0;
  c |= geom_has(g, keys, n, x, y, z + pitch) ? 32 : 0;
  ctx[i] = c;
  if (sym) {
    const int cp = pitch >> 1;
    int b = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      b |= geom_has(cg, ckeys, nc, x + ((j >> 2) & 1) * cp, y + ((j >> 1) & 1) * cp, z + (j & 1) * cp) ? (1 << j) : 0;
    sym[i] = b;
  }
}

__global__ void __launch_bounds__(256) k_geom_hist(const int* __restrict__ sym, const int* __restrict__ ctx, int n,
                                                   unsigned* __restrict__ hist, int* __restrict__ d_bad) {
  __shared__ unsigned h[GEOM_LDS];
  for (int t = threadIdx.x; t < GEOM_LDS; t += blockDim.x) h[t] = 0;
  __syncthreads();
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int s = sym[i];
    if (s < 1 || s > 255) { atomicOr(d_bad, 1); continue; }
    atomicAdd(&h[(ctx[i] & (GEOM_CTX - 1)) * 255 + s - 1], 1u);
  }
  __syncthreads();
  // the popcount histogram is a function of the byte counts: summed while the non-zero entries are flushed
  for (int t = threadIdx.x; t < GEOM_CTX * 255; t += blockDim.x) {
    const unsigned v = h[t];
    if (!v) continue;
    const int c = t / 255, s = t - c * 255 + 1;
    atomicAdd(&hist[c * 256 + s], v);
    atomicAdd(&h[GEOM_CTX * 255 + __popc(s) - 1], v);
  }
  __syncthreads();
  if (threadIdx.x < 8 && h[GEOM_CTX * 255 + threadIdx.x]) atomicAdd(&hist[GEOM_HIST + threadIdx.x], h[GEOM_CTX * 255 + threadIdx.x]);
}

__global__ void __launch_bounds__(256) k_geom_child_count(const int* __restrict__ sym, int n, int* __restrict__ cnt,
                                                          int* __restrict__ d_bad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  if (i == n) { cnt[n] = 0; return; }        // the exclusive scan leaves the total here
  const int s = sym[i];
  if (s < 1 || s > 255) { atomicOr(d_bad, 1); cnt[i] = 1; return; }
  cnt[i] = __popc(s);
}

__global__ void k_geom_total(const int* __restrict__ off, int n, long long* __restrict__ d_total) { *d_total = off[n]; }

__global__ void __launch_bounds__(256) k_geom_expand(const int64_t* __restrict__ keys, const int* __restrict__ sym,
                                                     const int* __restrict__ off, int n, int cp, int64_t cap,
                                                     int64_t* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int s = sym[i];
  if (s < 1 || s > 255) s = 1;
  const int64_t key = keys[i];
  int64_t o = off[i];
  while (s) {
    const int j = __ffs(s) - 1;
    s &= s - 1;
    if (o >= 0 && o < cap)
      out[o] = key + ((int64_t)(((j >> 2) & 1) * cp) << PCC_KEY_X_SHIFT) + ((int64_t)(((j >> 1) & 1) * cp) << PCC_KEY_Y_SHIFT) +
               (int64_t)((j & 1) * cp);
    ++o;
  }
}

__global__ void __launch_bounds__(256) k_geom_finish(const int64_t* __restrict__ keys, int64_t n, int ox, int oy, int oz,
                                                     int64_t* __restrict__ out_keys, int* __restrict__ out_xyz) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t key = keys[i];
  // (fields read in place, not through pcc_key_x/y/z: with the accessors the compiler no longer cancels the two biases below and
  //  this kernel comes out with other instructions, tools/kernel_identity.py)
  const int x = (int)((key >> PCC_KEY_X_SHIFT) & PCC_KEY_FIELD) - (int)PCC_BIAS + ox;
  const int y = (int)((key >> PCC_KEY_Y_SHIFT) & PCC_KEY_FIELD) - (int)PCC_BIAS + oy;
  const int z = (int)(key & PCC_KEY_FIELD) - (int)PCC_BIAS + oz;
  if (out_keys)      // (batch 0; each field wraps inside its 16 bits, so a coordinate outside the key range cannot carry into the next)
    out_keys[i] = ((int64_t)((x + (int)PCC_BIAS) & PCC_KEY_FIELD) << PCC_KEY_X_SHIFT) |
                  ((int64_t)((y + (int)PCC_BIAS) & PCC_KEY_FIELD) << PCC_KEY_Y_SHIFT) | (int64_t)((z + (int)PCC_BIAS) & PCC_KEY_FIELD);
  if (out_xyz) { out_xyz[3 * i] = x; out_xyz[3 * i + 1] = y; out_xyz[3 * i + 2] = z; }
}


// ---- backward-adaptive tables on the device (the integer rule of geometry.derive_tables) ----------------
// One workgroup per context, thread s <-> byte s + 1.  Every intermediate fits 64 bits: N < 2^20 after the shift, Gt < 2^21,
// W < 2^41, W << 20 < 2^61, w = q * r < 2^42, w * 65280 < 2^58; the class ratio r[k] = (pop * Gt << 12) / (ptot * E) is a
// 64-bit quotient (pop * Gt < 2^52) refined by twelve steps of binary long division.
struct GeomPop { unsigned long long v[8]; };

__device__ inline unsigned long long geom_block_sum(unsigned long long x, unsigned long long* red) {
  __syncthreads();
  red[threadIdx.x] = x;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) red[threadIdx.x] += red[threadIdx.x + d];
    __syncthreads();
  }
  return red[0];
}

__global__ void __launch_bounds__(256) k_geom_tables(const unsigned long long* __restrict__ A, GeomPop pop, int* __restrict__ cdf,
                                                     int* __restrict__ blob) {
  __shared__ unsigned long long red[256];
  __shared__ unsigned long long E[8];
  __shared__ unsigned long long R[8];
  __shared__ int cum[257];
  const int c = blockIdx.x, s = threadIdx.x;
  const bool live = s < 255;
  const int b = s + 1, k = __popc(b) - 1;
  unsigned long long col = 0;
  if (live) for (int cc = 0; cc < GEOM_CTX; ++cc) col += A[cc * 256 + b];
  const unsigned long long total = geom_block_sum(col, red);
  int shift = 0;
  while ((total >> shift) >= (1ull << 20)) ++shift;
  unsigned long long G = 0;
  if (live) for (int cc = 0; cc < GEOM_CTX; ++cc) G += A[cc * 256 + b] >> shift;
  const unsigned long long gt = geom_block_sum(G, red) + 255;
  if (s < 8) E[s] = 0;
  __syncthreads();
  if (live) atomicAdd(&E[k], G + 1);
  __syncthreads();
  if (s < 8) {
    unsigned long long ptot = 0, r = 0;
    for (int j = 0; j < 8; ++j) ptot += pop.v[j];
    if (pop.v[s] > 0) {
      const unsigned long long num = pop.v[s] * gt, den = ptot * E[s];
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
  const unsigned long long wsum = geom_block_sum(W, red);
  const unsigned long long w = live ? (1 + (W << 20) / wsum) * R[k] : 0;
  const unsigned long long vsum = geom_block_sum(w, red);
  unsigned long long f = live ? 1 + w * (65535ull - 255ull) / vsum : 0;
  const unsigned long long fsum = geom_block_sum(f, red);
  // first largest frequency: max over (f << 8 | 255 - s)
  __syncthreads();
  red[s] = live ? ((f << 8) | (unsigned long long)(255 - s)) : 0;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if (s < d && red[s + d] > red[s]) red[s] = red[s + d];
    __syncthreads();
  }
  if (live && (int)(255 - (red[0] & 255)) == s) f += 65535ull - fsum;
  __syncthreads();
  // inclusive scan of the 255 frequencies -> cdf[1..255]
  cum[s] = (int)f;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const int v = s >= d ? cum[s - d] : 0;
    __syncthreads();
    cum[s] += v;
    __syncthreads();
  }
  const int mine = cum[s];                      // cdf[s + 1] for s < 255
  __syncthreads();
  if (s == 0) { cum[0] = 0; cum[256] = 65536; }
  __syncthreads();
  if (live) cum[s + 1] = mine;
  __syncthreads();
  for (int v = s; v < 257; v += 256) cdf[c * 257 + v] = cum[v];
  // decoder table blob of pcc_rans_build_dec_table: int32 rows | int32 total | int32 row_off[65] | u16 lut[64*256] | u16 cdf16[64*257]
  unsigned short* lut = (unsigned short*)(blob + 2 + GEOM_CTX + 1);
  unsigned short* cdf16 = lut + GEOM_CTX * 256;
  for (int v = s; v < 257; v += 256) cdf16[c * 257 + v] = (unsigned short)(cum[v] & 0xFFFF);
  int lo = 0, hi = 255;                         // largest v in [0, 255] with cdf[v] <= s * 256
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (cum[mid] <= s * 256) lo = mid; else hi = mid - 1;
  }
  lut[c * 256 + s] = (unsigned short)lo;
  if (c == 0) {
    if (s == 0) { blob[0] = GEOM_CTX; blob[1] = GEOM_CTX * 257; }
    if (s <= GEOM_CTX) blob[2 + s] = s * 257;
  }
}

__global__ void __launch_bounds__(256) k_geom_state_update(unsigned long long* __restrict__ A, const unsigned* __restrict__ hist) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < GEOM_HIST) A[i] = (A[i] >> 1) + hist[i];
}

extern "C" int pcc_geom_occ_ctx(const int64_t* keys, int64_t n, int32_t pitch, const uint64_t* bits, const int32_t* rank,
                                const int32_t* h_grid, const int64_t* child_keys, int64_t n_child, const uint64_t* child_bits,
                                const int32_t* child_rank, const int32_t* h_child, int32_t* sym, int32_t* ctx, void* stream) {
  PCC_REQUIRE(keys && ctx && n > 0 && n < (1ll << 31), "pcc_geom_occ_ctx: bad arguments");
  PCC_REQUIRE(pcc_is_pow2(pitch) && pitch <= (1 << 15), "pcc_geom_occ_ctx: pitch %d is not a power of two in [1, 2^15]", pitch);
  PccGrid g, cg;                              // bits == NULL: binary search over the keys
  PCC_TRY(pcc_grid_from_host(bits, rank, h_grid, "pcc_geom_occ_ctx", &g));
  PCC_TRY(pcc_grid_from_host(sym ? child_bits : nullptr, child_rank, h_child, "pcc_geom_occ_ctx", &cg));
  PCC_REQUIRE(!h_grid || h_grid[6] == pitch, "pcc_geom_occ_ctx: the level's grid has another pitch");
  if (sym) {
    PCC_REQUIRE(child_keys && n_child > 0 && n_child < (1ll << 31) && pitch >= 2, "pcc_geom_occ_ctx: bytes need a child set at half the pitch");
    PCC_REQUIRE(!h_child || h_child[6] == pitch / 2, "pcc_geom_occ_ctx: the child grid has another pitch");
  }
  k_geom_occ_ctx<<<(unsigned)pcc_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(keys, (int)n, g, pitch, child_keys, (int)n_child, cg, sym,
                                                                             ctx);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int32_t pcc_geom_hist_words(void) { return GEOM_HIST + 8; }

extern "C" int pcc_geom_hist(const int32_t* sym, const int32_t* ctx, int64_t n, uint32_t* hist, int32_t* d_bad, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PCC_REQUIRE(sym && ctx && hist && d_bad && n > 0 && n < (1ll << 27), "pcc_geom_hist: bad arguments (n < 2^27)");
  PCC_CHECK_HIP(hipMemsetAsync(hist, 0, (size_t)(GEOM_HIST + 8) * 4, s));
  int64_t blocks = pcc_cdiv(n, 256 * 32);
  if (blocks > 256) blocks = 256;
  k_geom_hist<<<(unsigned)blocks, 256, 0, s>>>(sym, ctx, (int)n, hist, d_bad);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" size_t pcc_geom_offsets_ws_bytes(int64_t n) { return pcc_scan_ws_bytes(n + 1) + 256; }

extern "C" int pcc_geom_child_offsets(const int32_t* sym, int64_t n, int32_t* off, int64_t* d_total, int32_t* d_bad, void* ws,
                                      size_t ws_bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PCC_REQUIRE(sym && off && d_total && d_bad && n > 0 && n < (1ll << 27), "pcc_geom_child_offsets: bad arguments (n < 2^27)");
  if (ws_bytes < pcc_geom_offsets_ws_bytes(n)) { pcc_set_error("pcc_geom_child_offsets: workspace too small"); return PCC_EWS; }
  k_geom_child_count<<<(unsigned)pcc_cdiv(n + 1, 256), 256, 0, s>>>(sym, (int)n, off, d_bad);
  PCC_LAUNCH_CHECK();
  PCC_TRY(pcc_scan_exclusive_i32(off, off, n + 1, ws, ws_bytes, s));
  k_geom_total<<<1, 1, 0, s>>>(off, (int)n, (long long*)d_total);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_geom_expand(const int64_t* keys, const int32_t* sym, const int32_t* off, int64_t n, int32_t child_pitch,
                               int64_t* out_keys, int64_t cap, void* stream) {
  PCC_REQUIRE(keys && sym && off && out_keys && n > 0 && n < (1ll << 27) && cap >= n, "pcc_geom_expand: bad arguments");
  PCC_REQUIRE(pcc_is_pow2(child_pitch) && child_pitch < (1 << 15), "pcc_geom_expand: bad child pitch %d", child_pitch);
  k_geom_expand<<<(unsigned)pcc_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(keys, sym, off, (int)n, child_pitch, cap, out_keys);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_geom_finish(const int64_t* keys, int64_t n, int32_t ox, int32_t oy, int32_t oz, int64_t* out_keys,
                               int32_t* out_xyz, void* stream) {
  PCC_REQUIRE(keys && n > 0 && (out_keys || out_xyz), "pcc_geom_finish: bad arguments");
  PCC_REQUIRE(ox >= -(1 << 15) && oy >= -(1 << 15) && oz >= -(1 << 15) && ox < (1 << 15) && oy < (1 << 15) && oz < (1 << 15),
              "pcc_geom_finish: origin outside the 16-bit key range");
  k_geom_finish<<<(unsigned)pcc_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(keys, n, ox, oy, oz, out_keys, out_xyz);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int64_t pcc_geom_dec_table_bytes(void) {
  const int64_t b = 8 + 4 * (GEOM_CTX + 1) + 2 * GEOM_CTX * 256 + 2 * GEOM_CTX * 257;
  return (b + 15) / 16 * 16;
}

extern "C" int pcc_geom_tables(const uint64_t* state, const uint32_t* h_pop, int32_t* cdf, void* dec_table, void* stream) {
  PCC_REQUIRE(state && h_pop && cdf && dec_table, "pcc_geom_tables: NULL array");
  GeomPop pop;
  unsigned long long tot = 0;
  for (int k = 0; k < 8; ++k) { pop.v[k] = h_pop[k]; tot += h_pop[k]; }
  PCC_REQUIRE(tot > 0 && tot < (1ull << 31), "pcc_geom_tables: the popcount histogram must count 1 .. 2^31 - 1 nodes");
  k_geom_tables<<<GEOM_CTX, 256, 0, (hipStream_t)stream>>>((const unsigned long long*)state, pop, cdf, (int*)dec_table);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_geom_state_update(uint64_t* state, const uint32_t* hist, void* stream) {
  PCC_REQUIRE(state && hist, "pcc_geom_state_update: NULL array");
  k_geom_state_update<<<GEOM_HIST / 256, 256, 0, (hipStream_t)stream>>>((unsigned long long*)state, hist);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}
