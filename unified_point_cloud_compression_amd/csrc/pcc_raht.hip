// RAHT colour coder, device side: the region-adaptive hierarchical transform over the level sets of the
// octree geometry coder (pcc_geom.hip).  Level l is the set at pitch 2^(depth - l); a node's children are the up to eight cells
// of level l + 1 below it, child j = dx<<2 | dy<<1 | dz.  Inside a node three stages of weighted Haar butterflies merge the
// children along z (pairs (0,1) (2,3) (4,5) (6,7) -> even slot), y (slots (0,2) (4,6)) and x (slots (0,4)); a lone sibling
// passes through.  A node with m children emits m - 1 coefficient rows in the order stage 3, stage 2 (slot 0, 4), stage 1
// (slots 0, 2, 4, 6), parent-major: node i of level l starts at row (nodes(l) - 1) + off[i] - i, off = exclusive scan of the
// child counts (pcc_geom_child_offsets), so all levels share one [n - 1, C] matrix and nothing is scanned across levels.
//   k_raht_prepare   uint8 attributes (through the canonical permutation) -> Q8 int32 values, integer BT.709 for colour
//   k_raht_mask      node -> child-occupancy byte (the scan's input; the index kernel's stage pattern)
//   k_raht_forward   bottom-up: children's weights and values -> node weight and DC, quantised coefficients at their rows
//   k_raht_index     per symbol the (level, class, stage) group, or the table member the side bytes give that group
//   k_raht_hist      [groups][128] histogram of the quantised symbols (value + 63, or 127 for the escape), LDS integer atomics
//   k_raht_weights   bottom-up, decoder: node weights alone
//   k_raht_inverse   top-down: dequantise, the butterflies in reverse, children's DCs
//   k_raht_finish    Q8 values -> uint8 (inverse colour transform, clamp)
// Every kernel is one thread per node with eight child probes through the child level's grid index (binary search over the
// keys without one): dependent gathers, latency-bound like the geometry coder's; only the row writes are shaped (consecutive
// nodes write consecutive rows).  All arithmetic is integer (DESIGN.md 7f gives the bounds: values < 2^30, products < 2^61).
// No kernel reads a bitstream; every write is bounded by a caller-given row count.  The arithmetic, the probes and the argument
// checks live in pcc_raht.h, shared with the inter frames' kernels (pcc_raht_inter.hip).
#include "pcc_raht.h"

__global__ void __launch_bounds__(256) k_raht_prepare(const uint8_t* __restrict__ attrs, const int64_t* __restrict__ perm, int64_t n,
                                                      int C, int colour, int* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int64_t src = perm ? perm[i] : i;
  if (src < 0 || src >= n) src = i;
  const uint8_t* a = attrs + src * C;
  if (colour) {
    const int r = a[0], g = a[1], b = a[2];
    const int y = 54 * r + 183 * g + 19 * b;
    out[3 * i] = y;
    out[3 * i + 1] = ((256 * b - y) * 138 + 128) >> 8;
    out[3 * i + 2] = ((256 * r - y) * 163 + 128) >> 8;
  } else {
    for (int c = 0; c < C; ++c) out[i * C + c] = (int)a[c] << 8;
  }
}

__global__ void __launch_bounds__(256) k_raht_mask(RahtLevel L, int* __restrict__ mask) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L.n) return;
  int kid[8];
  mask[i] = oct_kids(L, i, kid);
}

__global__ void __launch_bounds__(256) k_raht_weights(RahtLevel L, const int* __restrict__ cw, int* __restrict__ wout) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L.n) return;
  int kid[8], w[8], s = 0;
  oct_kids(L, i, kid);
  oct_child_weights(cw, kid, w);
#pragma unroll
  for (int j = 0; j < 8; ++j) s += w[j];
  wout[i] = s;
}

__global__ void __launch_bounds__(256) k_raht_forward(RahtLevel L, const int* __restrict__ off, const int* __restrict__ cw,
                                                      const int* __restrict__ cv, int C, RahtSteps steps, int* __restrict__ wout,
                                                      int* __restrict__ vout, int* __restrict__ coef, long long row_base,
                                                      long long rows_total) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L.n) return;
  int kid[8], w[8];
  oct_kids(L, i, kid);
  oct_child_weights(cw, kid, w);
  RahtNode nd;
  raht_node(w, nd);
  wout[i] = nd.weight;
  long long row[7], r = row_base + off[i] - i;
#pragma unroll
  for (int t = 0; t < 7; ++t) { row[t] = (nd.e[t] && r >= 0 && r < rows_total) ? r : -1; r += nd.e[t]; }
  for (int c = 0; c < C; ++c) {
    const long long step = steps.v[c], half = step >> 1;
    long long x[8], h[7];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = kid[j] < 0 ? 0 : cv[(size_t)kid[j] * C + c];
    long long y[4], u[2], dc;
#pragma unroll
    for (int k = 0; k < 4; ++k) {                       // absent values are 0: a lone sibling is the sum
      h[3 + k] = 0;
      if (nd.e[3 + k]) raht_fwd(nd.a[3 + k], nd.b[3 + k], x[2 * k], x[2 * k + 1], y[k], h[3 + k]);
      else y[k] = x[2 * k] + x[2 * k + 1];
    }
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      h[1 + m] = 0;
      if (nd.e[1 + m]) raht_fwd(nd.a[1 + m], nd.b[1 + m], y[2 * m], y[2 * m + 1], u[m], h[1 + m]);
      else u[m] = y[2 * m] + y[2 * m + 1];
    }
    h[0] = 0;
    if (nd.e[0]) raht_fwd(nd.a[0], nd.b[0], u[0], u[1], dc, h[0]);
    else dc = u[0] + u[1];
    vout[(size_t)i * C + c] = (int)dc;
#pragma unroll
    for (int t = 0; t < 7; ++t) {
      if (row[t] < 0) continue;
      const long long m = h[t] < 0 ? -h[t] : h[t];
      const long long q = (m + half) / step;
      coef[row[t] * C + c] = (int)(h[t] < 0 ? -q : q);
    }
  }
}

__global__ void __launch_bounds__(256) k_raht_inverse(RahtLevel L, const int* __restrict__ off, const int* __restrict__ cw,
                                                      const int* __restrict__ v, int C, RahtSteps steps, const int* __restrict__ coef,
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
    for (int t = 0; t < 7; ++t) h[t] = row[t] < 0 ? 0 : lim((long long)coef[row[t] * C + c] * step);
    long long x[8], y[4], u[2];
    const long long dc = lim(v[(size_t)i * C + c]);
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

__global__ void __launch_bounds__(256) k_raht_index(const int* __restrict__ mask, const int* __restrict__ off, int n, int level, int C,
                                                    const int* __restrict__ side, int* __restrict__ idx, long long row_base,
                                                    long long rows_total) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bool e[7];
  oct_emits(mask[i] & 255, e);
  long long r = row_base + off[i] - i;
#pragma unroll
  for (int t = 0; t < 7; ++t) {
    if (!e[t]) continue;
    if (r >= 0 && r < rows_total) {
      const int stage = t == 0 ? 2 : (t < 3 ? 1 : 0);   // 0: z (stage 1), 1: y (stage 2), 2: x (stage 3)
      for (int c = 0; c < C; ++c) {
        const int g = level * 6 + (c ? 3 : 0) + stage;
        idx[r * C + c] = side ? (side[g] & 63) : g;
      }
    }
    ++r;
  }
}

__global__ void __launch_bounds__(256) k_raht_hist(const int* __restrict__ sym, const int* __restrict__ grp, long long n, int groups,
                                                   unsigned* __restrict__ hist) {
  __shared__ unsigned h[RAHT_MAX_GROUPS * RAHT_BINS];
  const int words = groups * RAHT_BINS;
  for (int t = threadIdx.x; t < words; t += blockDim.x) h[t] = 0;
  __syncthreads();
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
    const int g = grp[e], s = sym[e];
    if (g < 0 || g >= groups) continue;
    atomicAdd(&h[g * RAHT_BINS + ((s >= -63 && s <= 63) ? s + 63 : RAHT_BINS - 1)], 1u);
  }
  __syncthreads();
  for (int t = threadIdx.x; t < words; t += blockDim.x)
    if (h[t]) atomicAdd(&hist[t], h[t]);
}

__device__ inline uint8_t raht_u8(long long v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

__global__ void __launch_bounds__(256) k_raht_finish(const int* __restrict__ values, int64_t n, int C, int colour,
                                                     uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (colour) {
    const long long y = values[3 * i], cb = values[3 * i + 1], cr = values[3 * i + 2];
    const uint8_t r = raht_u8((256 * y + 403 * cr + 32768) >> 16);
    const uint8_t b = raht_u8((256 * y + 475 * cb + 32768) >> 16);
    out[3 * i] = r;
    out[3 * i + 1] = raht_u8(((y - 54 * (long long)r - 19 * (long long)b) * 358 + 32768) >> 16);
    out[3 * i + 2] = b;
  } else {
    for (int c = 0; c < C; ++c) out[i * C + c] = raht_u8(((long long)values[i * C + c] + 128) >> 8);
  }
}

// ---- entry points --------------------------------------------------------------------------------------------------------------
extern "C" uint64_t pcc_raht_isqrt(uint64_t x) { return x < (1ull << 62) ? raht_isqrt(x) : 0; }

extern "C" int pcc_raht_butterfly(uint32_t w1, uint32_t w2, int64_t x1, int64_t x2, int64_t* h_out) {
  PCC_REQUIRE(h_out && w1 >= 1 && w2 >= 1 && (uint64_t)w1 + w2 < (1ull << 27), "pcc_raht_butterfly: weights of 1 .. 2^27 - 1 in total");
  PCC_REQUIRE(x1 > -(1ll << 31) && x1 < (1ll << 31) && x2 > -(1ll << 31) && x2 < (1ll << 31), "pcc_raht_butterfly: values outside 32 bits");
  long long a, b, lo, hi, y1, y2;
  raht_factors(w1, w2, a, b);
  raht_fwd(a, b, x1, x2, lo, hi);
  raht_inv(a, b, lo, hi, y1, y2);
  h_out[0] = a; h_out[1] = b; h_out[2] = lo; h_out[3] = hi; h_out[4] = y1; h_out[5] = y2;
  return PCC_OK;
}

extern "C" int pcc_raht_prepare(const uint8_t* attrs, const int64_t* perm, int64_t n, int32_t channels, int32_t colour, int32_t* values,
                                void* stream) {
  PCC_REQUIRE(attrs && values && n > 0 && n < (1ll << 26) && channels >= 1 && channels <= RAHT_MAX_C, "pcc_raht_prepare: bad arguments");
  PCC_REQUIRE(!colour || channels == 3, "pcc_raht_prepare: the colour transform needs three channels");
  k_raht_prepare<<<(unsigned)pcc_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(attrs, perm, n, channels, colour, values);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_raht_mask(const int64_t* keys, int64_t n, int32_t pitch, const int64_t* child_keys, int64_t n_child,
                             const uint64_t* child_bits, const int32_t* child_rank, const int32_t* h_child, int32_t* mask, void* stream) {
  RahtLevel L;
  if (!raht_level("pcc_raht_mask", keys, n, pitch, child_keys, n_child, child_bits, child_rank, h_child, &L)) return PCC_EINVAL;
  PCC_REQUIRE(mask, "pcc_raht_mask: NULL array");
  k_raht_mask<<<(unsigned)pcc_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(L, mask);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_raht_weights(const int64_t* keys, int64_t n, int32_t pitch, const int64_t* child_keys, int64_t n_child,
                                const uint64_t* child_bits, const int32_t* child_rank, const int32_t* h_child, const int32_t* child_w,
                                int32_t* w, void* stream) {
  RahtLevel L;
  if (!raht_level("pcc_raht_weights", keys, n, pitch, child_keys, n_child, child_bits, child_rank, h_child, &L)) return PCC_EINVAL;
  PCC_REQUIRE(w, "pcc_raht_weights: NULL array");
  k_raht_weights<<<(unsigned)pcc_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(L, child_w, w);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_raht_forward(const int64_t* keys, int64_t n, int32_t pitch, const int64_t* child_keys, int64_t n_child,
                                const uint64_t* child_bits, const int32_t* child_rank, const int32_t* h_child, const int32_t* off,
                                const int32_t* child_w, const int32_t* child_v, int32_t channels, const int32_t* h_steps, int32_t* w,
                                int32_t* v, int32_t* coef, int64_t row_base, int64_t rows_total, void* stream) {
  RahtLevel L;
  RahtSteps st;
  if (!raht_level("pcc_raht_forward", keys, n, pitch, child_keys, n_child, child_bits, child_rank, h_child, &L)) return PCC_EINVAL;
  if (!raht_steps("pcc_raht_forward", channels, h_steps, &st)) return PCC_EINVAL;
  PCC_REQUIRE(off && child_v && w && v && (coef || rows_total == 0) && row_base >= 0 && rows_total >= 0, "pcc_raht_forward: bad arguments");
  k_raht_forward<<<(unsigned)pcc_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(L, off, child_w, child_v, channels, st, w, v, coef, row_base,
                                                                            rows_total);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_raht_inverse(const int64_t* keys, int64_t n, int32_t pitch, const int64_t* child_keys, int64_t n_child,
                                const uint64_t* child_bits, const int32_t* child_rank, const int32_t* h_child, const int32_t* off,
                                const int32_t* child_w, const int32_t* v, int32_t channels, const int32_t* h_steps, const int32_t* coef,
                                int64_t row_base, int64_t rows_total, int32_t* child_v, int32_t* d_flag, void* stream) {
  RahtLevel L;
  RahtSteps st;
  if (!raht_level("pcc_raht_inverse", keys, n, pitch, child_keys, n_child, child_bits, child_rank, h_child, &L)) return PCC_EINVAL;
  if (!raht_steps("pcc_raht_inverse", channels, h_steps, &st)) return PCC_EINVAL;
  PCC_REQUIRE(off && v && child_v && d_flag && (coef || rows_total == 0) && row_base >= 0 && rows_total >= 0, "pcc_raht_inverse: bad arguments");
  k_raht_inverse<<<(unsigned)pcc_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(L, off, child_w, v, channels, st, coef, row_base, rows_total,
                                                                            child_v, d_flag);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_raht_index(const int32_t* mask, const int32_t* off, int64_t n, int32_t level, int32_t channels, const int32_t* side,
                              int32_t* idx, int64_t row_base, int64_t rows_total, void* stream) {
  PCC_REQUIRE(mask && off && idx && n > 0 && n < (1ll << 26) && level >= 0 && level < 15 && channels >= 1 && channels <= RAHT_MAX_C &&
              row_base >= 0 && rows_total > 0, "pcc_raht_index: bad arguments");
  k_raht_index<<<(unsigned)pcc_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(mask, off, (int)n, level, channels, side, idx, row_base,
                                                                          rows_total);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_raht_hist(const int32_t* sym, const int32_t* grp, int64_t n_sym, int32_t groups, uint32_t* hist, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PCC_REQUIRE(sym && grp && hist && n_sym > 0 && n_sym < (1ll << 31) && groups >= 1 && groups <= RAHT_MAX_GROUPS,
              "pcc_raht_hist: bad arguments (1 .. 90 groups, fewer than 2^31 symbols)");
  PCC_CHECK_HIP(hipMemsetAsync(hist, 0, (size_t)groups * RAHT_BINS * 4, s));
  int64_t blocks = pcc_cdiv(n_sym, 256 * 32);
  if (blocks > 256) blocks = 256;
  k_raht_hist<<<(unsigned)blocks, 256, 0, s>>>(sym, grp, n_sym, groups, hist);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_raht_finish(const int32_t* values, int64_t n, int32_t channels, int32_t colour, uint8_t* out, void* stream) {
  PCC_REQUIRE(values && out && n > 0 && n < (1ll << 26) && channels >= 1 && channels <= RAHT_MAX_C, "pcc_raht_finish: bad arguments");
  PCC_REQUIRE(!colour || channels == 3, "pcc_raht_finish: the colour transform needs three channels");
  k_raht_finish<<<(unsigned)pcc_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(values, n, channels, colour, out);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}
