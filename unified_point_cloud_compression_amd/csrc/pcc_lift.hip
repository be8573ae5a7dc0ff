// Lossless attribute coder, device side: the levels, the stage order, the slot pairs and the row order of
// the RAHT coder (pcc_raht.hip, section 7f) with a reversible arithmetic.  Values are plain int32 levels (0..255; Co and Cg of
// YCoCg-R in -255..255).  Two present siblings with weights w1, w2 (w = w1 + w2) and values x1, x2 give H = x2 - x1 and
// L = x1 + floor(w2 * H / w), the node's rounded mean; x1 = L - floor(w2 * H / w), x2 = H + x1 invert it exactly.  A lone
// sibling passes through.  The coded symbol of a butterfly is H - Hp, where Hp comes from running the same lifting over a
// prediction of every child: the mean, with weights 27 / 9 / 3 / 1, of the up to eight cells of the node's OWN level that
// surround the child's corner (the node itself and its neighbours towards the child).
//   k_lift_prepare    uint8 attributes (through the canonical permutation) -> int32 values, YCoCg-R for colour
//   k_lift_forward    bottom-up: children's weights and values -> node weight and value, H at the node's rows
//   k_lift_residual   encoder, any level order: rows -= Hp (26 neighbour probes of the node's level, 8 child probes)
//   k_lift_inverse    top-down: H = symbol + Hp, the lifting in reverse, the children's values, every result clamped
//   k_lift_finish     int32 values -> uint8 (inverse YCoCg-R), out-of-range levels clamped and flagged
// One thread per node, as in pcc_raht.hip: dependent gathers, latency-bound.  Every loop over children, cells and butterflies
// is unrolled so that the per-thread arrays stay in registers.  No kernel reads a bitstream; every row access is bounded by a
// caller-given row count and every child or neighbour row by its set's size.
#include "pcc_common.h"
#include "pcc_conv.h"

static constexpr int LIFT_MAX_C = 8;
static constexpr int LIFT_SYMBOL_LIMIT = 1023;        // the decoder's clamp on a symbol (a valid one is within +-1020)
static constexpr int LIFT_VALUE_LIMIT = 1023;         // the host exports' argument range

struct LiftLevel {
  const int64_t* keys; int n; int pitch; PccGrid g;   // the nodes and their own grid index (neighbour probes)
  const int64_t* ckeys; int nc; PccGrid cg;           // their children: the canonical set at pitch / 2
};

// ---- the arithmetic, host and device ---------------------------------------------------------------------------------------
// floor(p / w) for w >= 1 and |p| < 2^52: 64-bit integer division is emulated on the device, a double division is not, and
// with |p / w| < 2^12 its error is far below the 1 / w that separates a non-integer quotient from an integer; the remainder
// check makes the result exact whatever the rounding.
__host__ __device__ inline long long lift_floor_div(long long p, long long w) {
  long long q = (long long)floor((double)p / (double)w);
  const long long r = p - q * w;
  if (r < 0) --q;
  else if (r >= w) ++q;
  return q;
}

__host__ __device__ inline int lift_floor_div32(int a, int d) {      // d >= 1
  int q = a / d;
  if (a % d < 0) --q;
  return q;
}

__host__ __device__ inline void lift_fwd(int w1, int w2, int x1, int x2, int& lo, int& hi) {
  hi = x2 - x1;
  lo = x1 + (int)lift_floor_div((long long)w2 * hi, (long long)w1 + w2);
}

__host__ __device__ inline void lift_inv(int w1, int w2, int lo, int hi, int& x1, int& x2) {
  x1 = lo - (int)lift_floor_div((long long)w2 * hi, (long long)w1 + w2);
  x2 = hi + x1;
}

__host__ __device__ constexpr int lift_cell_weight(int b) {         // 27, 9, 3, 1 for 0, 1, 2, 3 non-zero components of b
  return b == 0 ? 27 : (b == 7 ? 1 : ((b == 1 || b == 2 || b == 4) ? 9 : 3));
}

// weighted mean of the present cells b = bx<<2 | by<<1 | bz (mask != 0): floor((num + (den >> 1)) / den)
__host__ __device__ inline int lift_predict(const int v[8], int mask) {
  int den = 0, num = 0;
#pragma unroll
  for (int b = 0; b < 8; ++b)
    if ((mask >> b) & 1) { den += lift_cell_weight(b); num += lift_cell_weight(b) * v[b]; }
  return lift_floor_div32(num + (den >> 1), den);
}

// which of the seven butterflies of a node exist, in row order: [0] stage 3, [1] [2] stage 2 (slot 0, 4), [3..6] stage 1
__host__ __device__ inline void lift_emits(int mask, bool e[7]) {
  bool p[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int two = (mask >> (2 * k)) & 3;
    e[3 + k] = two == 3;
    p[k] = two != 0;
  }
  e[1] = p[0] && p[1];
  e[2] = p[2] && p[3];
  e[0] = (p[0] || p[1]) && (p[2] || p[3]);
}

// the three stages over the children's weights w[8] (0: absent) and values x[8] (0 where absent): the node's value, h[7] in
// row order (0 where the butterfly does not exist)
__host__ __device__ inline int lift_node_fwd(const int w[8], const bool e[7], const int x[8], int h[7]) {
  int y[4], u[2], wy[4], dc;
#pragma unroll
  for (int k = 0; k < 4; ++k) {                       // absent values are 0: a lone sibling is the sum
    h[3 + k] = 0;
    wy[k] = w[2 * k] + w[2 * k + 1];
    if (e[3 + k]) lift_fwd(w[2 * k], w[2 * k + 1], x[2 * k], x[2 * k + 1], y[k], h[3 + k]);
    else y[k] = x[2 * k] + x[2 * k + 1];
  }
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    h[1 + m] = 0;
    if (e[1 + m]) lift_fwd(wy[2 * m], wy[2 * m + 1], y[2 * m], y[2 * m + 1], u[m], h[1 + m]);
    else u[m] = y[2 * m] + y[2 * m + 1];
  }
  h[0] = 0;
  if (e[0]) lift_fwd(wy[0] + wy[1], wy[2] + wy[3], u[0], u[1], dc, h[0]);
  else dc = u[0] + u[1];
  return dc;
}

// ---- probes ----------------------------------------------------------------------------------------------------------------
// rows of the eight children (-1: absent); returns the occupancy byte
__device__ inline int lift_kids(const LiftLevel& L, int i, int kid[8]) {
  const int64_t key = L.keys[i];
  const int x = pcc_key_x(key), y = pcc_key_y(key), z = pcc_key_z(key);
  const int cp = L.pitch >> 1;
  int mask = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int cx = x + ((j >> 2) & 1) * cp, cy = y + ((j >> 1) & 1) * cp, cz = z + (j & 1) * cp;
    int r = -1;
    if ((cx | cy | cz) >= 0 && cx < (int)PCC_BIAS && cy < (int)PCC_BIAS && cz < (int)PCC_BIAS) {
      r = pcc_lookup(L.cg, L.ckeys, L.nc, pcc_key_pack(0, cx, cy, cz));
      if (r >= L.nc) r = -1;
    }
    kid[j] = r;
    if (r >= 0) mask |= 1 << j;
  }
  return mask;
}

// rows of the 27 cells around node i in its own level, k = 9 (dx + 1) + 3 (dy + 1) + (dz + 1) (-1: absent; k = 13 is i)
__device__ inline void lift_neighbours(const LiftLevel& L, int i, int nb[27]) {
  const int64_t key = L.keys[i];
  const int x = pcc_key_x(key), y = pcc_key_y(key), z = pcc_key_z(key);
#pragma unroll
  for (int k = 0; k < 27; ++k) {
    if (k == 13) { nb[k] = i; continue; }
    const int qx = x + (k / 9 - 1) * L.pitch, qy = y + ((k / 3) % 3 - 1) * L.pitch, qz = z + (k % 3 - 1) * L.pitch;
    int r = -1;
    if ((qx | qy | qz) >= 0 && qx < (int)PCC_BIAS && qy < (int)PCC_BIAS && qz < (int)PCC_BIAS) {
      r = pcc_lookup(L.g, L.keys, L.n, pcc_key_pack(0, qx, qy, qz));
      if (r >= L.n) r = -1;
    }
    nb[k] = r;
  }
}

__device__ inline void lift_child_weights(const int* __restrict__ cw, const int kid[8], int w[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) w[j] = kid[j] < 0 ? 0 : (cw ? cw[kid[j]] : 1);      // cw == nullptr: the children are voxels
}

// hp[7] of channel c of a node: the predictions of its present children from the level's values v, lifted with the children's
// weights.  Cell b of child j lies at offset d * b per axis, d = 2 * (the child's bit) - 1.
__device__ inline void lift_node_hp(const int* __restrict__ v, int C, int c, const int nb[27], const int kid[8], const int w[8],
                                    const bool e[7], int hp[7]) {
  int nv[27];
#pragma unroll
  for (int k = 0; k < 27; ++k) nv[k] = nb[k] < 0 ? 0 : v[(size_t)nb[k] * C + c];
  int pred[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    int cell[8], mask = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const int k = 9 * (1 + (2 * ((j >> 2) & 1) - 1) * ((b >> 2) & 1)) + 3 * (1 + (2 * ((j >> 1) & 1) - 1) * ((b >> 1) & 1)) +
                    (1 + (2 * (j & 1) - 1) * (b & 1));
      cell[b] = nv[k];
      mask |= (nb[k] >= 0) << b;
    }
    pred[j] = kid[j] < 0 ? 0 : lift_predict(cell, mask);
  }
  lift_node_fwd(w, e, pred, hp);
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_lift_prepare(const uint8_t* __restrict__ attrs, const int64_t* __restrict__ perm, int64_t n,
                                                      int C, int colour, int* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int64_t src = perm ? perm[i] : i;
  if (src < 0 || src >= n) src = i;
  const uint8_t* a = attrs + src * C;
  if (colour) {
    const int r = a[0], g = a[1], b = a[2];
    const int co = r - b, t = b + (co >> 1), cg = g - t;
    out[3 * i] = t + (cg >> 1);
    out[3 * i + 1] = co;
    out[3 * i + 2] = cg;
  } else {
    for (int c = 0; c < C; ++c) out[i * C + c] = a[c];
  }
}

__global__ void __launch_bounds__(256) k_lift_forward(LiftLevel L, const int* __restrict__ off, const int* __restrict__ cw,
                                                      const int* __restrict__ cv, int C, int* __restrict__ wout, int* __restrict__ vout,
                                                      int* __restrict__ coef, long long row_base, long long rows_total) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L.n) return;
  int kid[8], w[8];
  bool e[7];
  lift_emits(lift_kids(L, i, kid), e);
  lift_child_weights(cw, kid, w);
  int s = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) s += w[j];
  wout[i] = s;
  long long row[7], r = row_base + off[i] - i;
#pragma unroll
  for (int t = 0; t < 7; ++t) { row[t] = (e[t] && r >= 0 && r < rows_total) ? r : -1; r += e[t]; }
  for (int c = 0; c < C; ++c) {
    int x[8], h[7];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = kid[j] < 0 ? 0 : cv[(size_t)kid[j] * C + c];
    vout[(size_t)i * C + c] = lift_node_fwd(w, e, x, h);
#pragma unroll
    for (int t = 0; t < 7; ++t)
      if (row[t] >= 0) coef[row[t] * C + c] = h[t];
  }
}

__global__ void __launch_bounds__(256) k_lift_residual(LiftLevel L, const int* __restrict__ off, const int* __restrict__ cw,
                                                       const int* __restrict__ v, int C, int* __restrict__ coef, long long row_base,
                                                       long long rows_total) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L.n) return;
  int kid[8], w[8], nb[27];
  bool e[7];
  lift_emits(lift_kids(L, i, kid), e);
  lift_child_weights(cw, kid, w);
  lift_neighbours(L, i, nb);
  long long row[7], r = row_base + off[i] - i;
#pragma unroll
  for (int t = 0; t < 7; ++t) { row[t] = (e[t] && r >= 0 && r < rows_total) ? r : -1; r += e[t]; }
  for (int c = 0; c < C; ++c) {
    int hp[7];
    lift_node_hp(v, C, c, nb, kid, w, e, hp);
#pragma unroll
    for (int t = 0; t < 7; ++t)
      if (row[t] >= 0) coef[row[t] * C + c] -= hp[t];
  }
}

__global__ void __launch_bounds__(256) k_lift_inverse(LiftLevel L, const int* __restrict__ off, const int* __restrict__ cw,
                                                      const int* __restrict__ v, int C, int colour, int predict,
                                                      const int* __restrict__ coef, long long row_base, long long rows_total,
                                                      int* __restrict__ cv, int* __restrict__ d_flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L.n) return;
  int kid[8], w[8], nb[27];
  bool e[7];
  lift_emits(lift_kids(L, i, kid), e);
  lift_child_weights(cw, kid, w);
  if (predict) lift_neighbours(L, i, nb);
  long long row[7], r = row_base + off[i] - i;
#pragma unroll
  for (int t = 0; t < 7; ++t) { row[t] = (e[t] && r >= 0 && r < rows_total) ? r : -1; r += e[t]; }
  int wy[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) wy[k] = w[2 * k] + w[2 * k + 1];
  bool clamped = false;
  for (int c = 0; c < C; ++c) {
    const int lo = (colour && c) ? -255 : 0, hi = 255;
    auto lim = [&](int t) {
      if (t > hi) { clamped = true; return hi; }
      if (t < lo) { clamped = true; return lo; }
      return t;
    };
    int h[7];
#pragma unroll
    for (int t = 0; t < 7; ++t) h[t] = 0;
    if (predict) lift_node_hp(v, C, c, nb, kid, w, e, h);
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
    for (int m = 0; m < 2; ++m) {
      if (e[1 + m]) {
        lift_inv(wy[2 * m], wy[2 * m + 1], u[m], h[1 + m], y[2 * m], y[2 * m + 1]);
        y[2 * m] = lim(y[2 * m]); y[2 * m + 1] = lim(y[2 * m + 1]);
      } else { y[2 * m] = u[m]; y[2 * m + 1] = u[m]; }
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

__global__ void __launch_bounds__(256) k_lift_finish(const int* __restrict__ values, int64_t n, int C, int colour,
                                                     uint8_t* __restrict__ out, int* __restrict__ d_flag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bool clamped = false;
  auto u8 = [&](int v) {
    if (v < 0) { clamped = true; return (uint8_t)0; }
    if (v > 255) { clamped = true; return (uint8_t)255; }
    return (uint8_t)v;
  };
  if (colour) {
    const int y = values[3 * i], co = values[3 * i + 1], cg = values[3 * i + 2];
    const int t = y - (cg >> 1), g = cg + t, b = t - (co >> 1);
    out[3 * i] = u8(b + co);
    out[3 * i + 1] = u8(g);
    out[3 * i + 2] = u8(b);
  } else {
    for (int c = 0; c < C; ++c) out[i * C + c] = u8(values[i * C + c]);
  }
  if (clamped) atomicOr(d_flag, 1);
}

// ---- entry points --------------------------------------------------------------------------------------------------------------
static bool lift_level(const char* what, const int64_t* keys, int64_t n, int32_t pitch, const uint64_t* bits, const int32_t* rank,
                       const int32_t* h_grid, const int64_t* child_keys, int64_t n_child, const uint64_t* child_bits,
                       const int32_t* child_rank, const int32_t* h_child, LiftLevel* L) {
  if (!(keys && child_keys && n > 0 && n_child >= n && n_child < (1ll << 26))) {
    pcc_set_error("%s: bad arguments (a level of n >= 1 nodes with n .. 2^26 - 1 children)", what);
    return false;
  }
  if (!(pitch >= 2 && pitch <= (1 << 15) && pcc_is_pow2(pitch))) {
    pcc_set_error("%s: pitch %d is not a power of two in [2, 2^15]", what, pitch);
    return false;
  }
  if (pcc_grid_from_host(bits, rank, h_grid, what, &L->g) != PCC_OK) return false;                 // bits == NULL: binary search
  if (pcc_grid_from_host(child_bits, child_rank, h_child, what, &L->cg) != PCC_OK) return false;
  if ((L->g.bits && h_grid[6] != pitch) || (L->cg.bits && h_child[6] != pitch / 2)) {
    pcc_set_error("%s: a grid index has another pitch than its level", what);
    return false;
  }
  L->keys = keys; L->n = (int)n; L->pitch = pitch; L->ckeys = child_keys; L->nc = (int)n_child;
  return true;
}

extern "C" int pcc_lift_pair(uint32_t w1, uint32_t w2, int32_t x1, int32_t x2, int64_t* h_out) {
  PCC_REQUIRE(h_out && w1 >= 1 && w2 >= 1 && (uint64_t)w1 + w2 < (1ull << 27), "pcc_lift_pair: weights of 1 .. 2^27 - 1 in total");
  PCC_REQUIRE(x1 >= -LIFT_VALUE_LIMIT && x1 <= LIFT_VALUE_LIMIT && x2 >= -LIFT_VALUE_LIMIT && x2 <= LIFT_VALUE_LIMIT,
              "pcc_lift_pair: values outside +-1023");
  int lo, hi, y1, y2;
  lift_fwd((int)w1, (int)w2, x1, x2, lo, hi);
  lift_inv((int)w1, (int)w2, lo, hi, y1, y2);
  h_out[0] = lo; h_out[1] = hi; h_out[2] = y1; h_out[3] = y2;
  return PCC_OK;
}

extern "C" int pcc_lift_predict(const int32_t* h_values, int32_t mask, int32_t* h_out) {
  PCC_REQUIRE(h_values && h_out && mask >= 1 && mask <= 255, "pcc_lift_predict: eight values and a presence mask of 1 .. 255");
  int v[8];
  for (int b = 0; b < 8; ++b) {
    PCC_REQUIRE(h_values[b] >= -LIFT_VALUE_LIMIT && h_values[b] <= LIFT_VALUE_LIMIT, "pcc_lift_predict: values outside +-1023");
    v[b] = h_values[b];
  }
  *h_out = lift_predict(v, mask);
  return PCC_OK;
}

extern "C" int pcc_lift_prepare(const uint8_t* attrs, const int64_t* perm, int64_t n, int32_t channels, int32_t colour, int32_t* values,
                                void* stream) {
  PCC_REQUIRE(attrs && values && n > 0 && n < (1ll << 26) && channels >= 1 && channels <= LIFT_MAX_C, "pcc_lift_prepare: bad arguments");
  PCC_REQUIRE(!colour || channels == 3, "pcc_lift_prepare: the colour transform needs three channels");
  k_lift_prepare<<<(unsigned)pcc_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(attrs, perm, n, channels, colour, values);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_lift_forward(const int64_t* keys, int64_t n, int32_t pitch, const int64_t* child_keys, int64_t n_child,
                                const uint64_t* child_bits, const int32_t* child_rank, const int32_t* h_child, const int32_t* off,
                                const int32_t* child_w, const int32_t* child_v, int32_t channels, int32_t* w, int32_t* v, int32_t* coef,
                                int64_t row_base, int64_t rows_total, void* stream) {
  LiftLevel L;
  if (!lift_level("pcc_lift_forward", keys, n, pitch, nullptr, nullptr, nullptr, child_keys, n_child, child_bits, child_rank, h_child, &L))
    return PCC_EINVAL;
  PCC_REQUIRE(channels >= 1 && channels <= LIFT_MAX_C && off && child_v && w && v && (coef || rows_total == 0) && row_base >= 0 &&
              rows_total >= 0 && rows_total < (1ll << 26), "pcc_lift_forward: bad arguments");
  k_lift_forward<<<(unsigned)pcc_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(L, off, child_w, child_v, channels, w, v, coef, row_base,
                                                                            rows_total);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_lift_residual(const int64_t* keys, int64_t n, int32_t pitch, const uint64_t* bits, const int32_t* rank,
                                 const int32_t* h_grid, const int64_t* child_keys, int64_t n_child, const uint64_t* child_bits,
                                 const int32_t* child_rank, const int32_t* h_child, const int32_t* off, const int32_t* child_w,
                                 const int32_t* v, int32_t channels, int32_t* coef, int64_t row_base, int64_t rows_total, void* stream) {
  LiftLevel L;
  if (!lift_level("pcc_lift_residual", keys, n, pitch, bits, rank, h_grid, child_keys, n_child, child_bits, child_rank, h_child, &L))
    return PCC_EINVAL;
  PCC_REQUIRE(channels >= 1 && channels <= LIFT_MAX_C && off && v && coef && row_base >= 0 && rows_total > 0 && rows_total < (1ll << 26),
              "pcc_lift_residual: bad arguments");
  k_lift_residual<<<(unsigned)pcc_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(L, off, child_w, v, channels, coef, row_base, rows_total);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_lift_inverse(const int64_t* keys, int64_t n, int32_t pitch, const uint64_t* bits, const int32_t* rank,
                                const int32_t* h_grid, const int64_t* child_keys, int64_t n_child, const uint64_t* child_bits,
                                const int32_t* child_rank, const int32_t* h_child, const int32_t* off, const int32_t* child_w,
                                const int32_t* v, int32_t channels, int32_t colour, int32_t predict, const int32_t* coef, int64_t row_base,
                                int64_t rows_total, int32_t* child_v, int32_t* d_flag, void* stream) {
  LiftLevel L;
  if (!lift_level("pcc_lift_inverse", keys, n, pitch, bits, rank, h_grid, child_keys, n_child, child_bits, child_rank, h_child, &L))
    return PCC_EINVAL;
  PCC_REQUIRE(channels >= 1 && channels <= LIFT_MAX_C && (!colour || channels == 3) && off && v && child_v && d_flag &&
              (coef || rows_total == 0) && row_base >= 0 && rows_total >= 0 && rows_total < (1ll << 26), "pcc_lift_inverse: bad arguments");
  k_lift_inverse<<<(unsigned)pcc_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(L, off, child_w, v, channels, colour, predict, coef, row_base,
                                                                            rows_total, child_v, d_flag);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_lift_finish(const int32_t* values, int64_t n, int32_t channels, int32_t colour, uint8_t* out, int32_t* d_flag,
                               void* stream) {
  PCC_REQUIRE(values && out && d_flag && n > 0 && n < (1ll << 26) && channels >= 1 && channels <= LIFT_MAX_C, "pcc_lift_finish: bad arguments");
  PCC_REQUIRE(!colour || channels == 3, "pcc_lift_finish: the colour transform needs three channels");
  k_lift_finish<<<(unsigned)pcc_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(values, n, channels, colour, out, d_flag);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}
