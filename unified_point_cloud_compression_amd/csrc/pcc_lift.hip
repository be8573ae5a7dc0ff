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
// caller-given row count and every child or neighbour row by its set's size.  The arithmetic and the probes are in pcc_lift.h,
// shared with the inter frames' last level (pcc_lift_inter.hip).
#include "pcc_lift.h"

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
  oct_emits(oct_kids(L, i, kid), e);
  oct_child_weights(cw, kid, w);
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
  oct_emits(oct_kids(L, i, kid), e);
  oct_child_weights(cw, kid, w);
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
  oct_emits(oct_kids(L, i, kid), e);
  oct_child_weights(cw, kid, w);
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
