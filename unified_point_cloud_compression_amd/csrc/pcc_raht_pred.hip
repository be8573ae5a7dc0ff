// RAHT colour with prediction from the parent level, device side (DESIGN.md section 7f "Prediction from the parent level",
// stream format 0xB9): the levels, rows, quantiser and groups of pcc_raht.hip, every coefficient coded as quantise(H - Hp).  Hp is
// the node's own three butterfly stages over a prediction of its children: per child the 27 / 9 / 3 / 1 weighted mean (the
// lifting coder's 2 x 2 x 2 rule, pcc_lift.h) of the MEANS m = DC / sqrt(w) of the node's level as the decoder has reconstructed
// them, scaled by sqrt(w_child) into the child's domain.  The loop is closed: the encoder first takes the true H of every level
// from pcc_raht_forward with every step 1, then walks top-down with the decoder's arithmetic.
//   k_raht_pred_root     the root: DC -> quantise(DC) * step as the decoder will hold it, and its mean
//   k_raht_pred_level    top-down, one launch per level.  Encoder: reads the true H rows, writes quantise(H - Hp) to the rows
//                        0xB3 uses; decoder: reads the symbols.  Both: H' = Hp + q * step, the butterflies in reverse, the
//                        children's DCs and means -- through raht_pred_channel, the one function for "predict, dequantise,
//                        inverse", so the two sides cannot drift apart
// One thread per node as in pcc_raht.hip and pcc_lift.hip: 8 child probes through the child level's grid index and 26 neighbour
// probes through the node level's (binary search without one: the same bits), dependent gathers, latency-bound; consecutive
// nodes write consecutive rows.  The loops over children, cells and butterflies are unrolled so the per-thread arrays stay in
// registers.  All arithmetic is integer.  No kernel reads a bitstream: every row access is bounded by a caller-given row count,
// every child or neighbour row by its set's size.
#include "pcc_raht.h"
#include "pcc_lift.h"

// One channel of one node: the children's predictions from the level's means m, scaled by sc[j] = sqrt(w_j) and transformed to
// Hp; sym(t, Hp_t) gives the symbol of butterfly t (the encoder quantises H - Hp there, the decoder reads it); H' = Hp + q * step,
// both terms and the sum clamped; then k_raht_inverse's butterflies with the same clamps in the same places.  x[8]: the children's DCs.
template <class Sym>
__device__ inline void raht_pred_channel(const RahtNode& nd, const int w[8], const int kid[8], const int nb[27], const int sc[8],
                                         const int* __restrict__ m, int C, int c, long long dc, long long step, Sym sym,
                                         long long x[8], bool& clamped) {
  auto lim = [&](long long t) {
    if (t > RAHT_LIMIT) { clamped = true; return RAHT_LIMIT; }
    if (t < -RAHT_LIMIT) { clamped = true; return -RAHT_LIMIT; }
    return t;
  };
  int pred[8];
  lift_child_preds(m, C, c, nb, kid, pred);
  long long p[8], h[7];
#pragma unroll
  for (int j = 0; j < 8; ++j) p[j] = kid[j] < 0 ? 0 : lim(raht_pred_scale(pred[j], sc[j]));
  raht_node_fwd(nd, p, h);
#pragma unroll
  for (int t = 0; t < 7; ++t) {
    if (!nd.e[t]) { h[t] = 0; continue; }
    const long long hp = lim(h[t]);
    h[t] = lim(hp + lim((long long)sym(t, hp) * step));
  }
  long long y[4], u[2];
  dc = lim(dc);
  if (nd.e[0]) { raht_inv(nd.a[0], nd.b[0], dc, h[0], u[0], u[1]); u[0] = lim(u[0]); u[1] = lim(u[1]); }
  else { u[0] = (w[0] + w[1] + w[2] + w[3]) > 0 ? dc : 0; u[1] = (w[4] + w[5] + w[6] + w[7]) > 0 ? dc : 0; }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    if (nd.e[1 + k]) {
      raht_inv(nd.a[1 + k], nd.b[1 + k], u[k], h[1 + k], y[2 * k], y[2 * k + 1]);
      y[2 * k] = lim(y[2 * k]); y[2 * k + 1] = lim(y[2 * k + 1]);
    } else {
      y[2 * k] = (w[4 * k] + w[4 * k + 1]) > 0 ? u[k] : 0;
      y[2 * k + 1] = (w[4 * k + 2] + w[4 * k + 3]) > 0 ? u[k] : 0;
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
}

// a mean as the next level reads it: clamped so that 64 weighted means sum in int32 (a valid stream stays below 2^17)
__device__ inline int raht_pred_mean_clamped(long long dc, unsigned a, bool& clamped) {
  long long t = raht_pred_mean(dc, a);
  if (t > RAHT_PRED_MEAN_LIMIT) { clamped = true; t = RAHT_PRED_MEAN_LIMIT; }
  if (t < -RAHT_PRED_MEAN_LIMIT) { clamped = true; t = -RAHT_PRED_MEAN_LIMIT; }
  return (int)t;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_raht_pred_root(const int* __restrict__ v, int w, int C, RahtSteps steps, int* __restrict__ vout,
                                                       int* __restrict__ mout, int* __restrict__ d_flag) {
  const int c = threadIdx.x;
  if (blockIdx.x || c >= C) return;
  bool clamped = false;
  const long long step = steps.v[c];
  long long dc = (long long)raht_quantise(v[c], step) * step;
  if (dc > RAHT_LIMIT) { clamped = true; dc = RAHT_LIMIT; }
  if (dc < -RAHT_LIMIT) { clamped = true; dc = -RAHT_LIMIT; }
  vout[c] = (int)dc;
  mout[c] = raht_pred_mean_clamped(dc, raht_pred_mean_factor((unsigned)w), clamped);
  if (clamped) atomicOr(d_flag, 1);
}

template <bool ENCODE>
__global__ void __launch_bounds__(256) k_raht_pred_level(LiftLevel L, const int* __restrict__ off, const int* __restrict__ cw,
                                                         const int* __restrict__ v, const int* __restrict__ m, int C, RahtSteps steps,
                                                         const int* __restrict__ htrue, int* __restrict__ coef, long long row_base,
                                                         long long rows_total, int* __restrict__ cv, int* __restrict__ cm,
                                                         int* __restrict__ d_flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L.n) return;
  int kid[8], w[8], nb[27], sc[8];
  oct_kids(L, i, kid);
  oct_child_weights(cw, kid, w);
  lift_neighbours(L, i, nb);
  RahtNode nd;
  raht_node(w, nd);
#pragma unroll
  for (int j = 0; j < 8; ++j) sc[j] = raht_pred_factor((unsigned)w[j]);
  unsigned am[8];                                     // the children's mean factors; cm == nullptr: the children are voxels, no level reads their means
#pragma unroll
  for (int j = 0; j < 8; ++j) am[j] = (cm && w[j] > 0) ? raht_pred_mean_factor((unsigned)w[j]) : 0u;
  long long row[7], r = row_base + off[i] - i;
#pragma unroll
  for (int t = 0; t < 7; ++t) { row[t] = (nd.e[t] && r >= 0 && r < rows_total) ? r : -1; r += nd.e[t]; }
  bool clamped = false;
  for (int c = 0; c < C; ++c) {
    const long long step = steps.v[c];
    auto sym = [&](int t, long long hp) {
      if (row[t] < 0) return 0;
      if constexpr (ENCODE) {
        const int q = raht_quantise((long long)htrue[row[t] * C + c] - hp, step);
        coef[row[t] * C + c] = q;
        return q;
      }
      return coef[row[t] * C + c];
    };
    long long x[8];
    raht_pred_channel(nd, w, kid, nb, sc, m, C, c, v[(size_t)i * C + c], step, sym, x, clamped);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (kid[j] < 0) continue;
      cv[(size_t)kid[j] * C + c] = (int)x[j];
      if (cm) cm[(size_t)kid[j] * C + c] = raht_pred_mean_clamped(x[j], am[j], clamped);
    }
  }
  if (clamped) atomicOr(d_flag, 1);
}

// ---- entry points --------------------------------------------------------------------------------------------------------------
extern "C" int pcc_raht_pred_mean(int64_t dc, uint32_t w, int64_t* h_out) {
  PCC_REQUIRE(h_out && w >= 1 && w < (1u << 26) && dc >= -RAHT_LIMIT && dc <= RAHT_LIMIT, "pcc_raht_pred_mean: a DC within +-2^30 and a weight of 1 .. 2^26 - 1");
  *h_out = raht_pred_mean(dc, raht_pred_mean_factor(w));
  return PCC_OK;
}

extern "C" int pcc_raht_pred_scale(int64_t pred, uint32_t w, int64_t* h_out) {
  PCC_REQUIRE(h_out && w >= 1 && w < (1u << 26) && pred >= -RAHT_PRED_MEAN_LIMIT && pred <= RAHT_PRED_MEAN_LIMIT,
              "pcc_raht_pred_scale: a prediction within +-2^24 and a weight of 1 .. 2^26 - 1");
  *h_out = raht_pred_scale(pred, raht_pred_factor(w));
  return PCC_OK;
}

extern "C" int pcc_raht_pred_predict(const int32_t* h_means, int32_t mask, int32_t* h_out) {
  PCC_REQUIRE(h_means && h_out && mask >= 1 && mask <= 255, "pcc_raht_pred_predict: eight means and a presence mask of 1 .. 255");
  int v[8];
  for (int b = 0; b < 8; ++b) {
    PCC_REQUIRE(h_means[b] >= -RAHT_PRED_MEAN_LIMIT && h_means[b] <= RAHT_PRED_MEAN_LIMIT, "pcc_raht_pred_predict: means outside +-2^24");
    v[b] = h_means[b];
  }
  *h_out = lift_predict(v, mask);
  return PCC_OK;
}

extern "C" int pcc_raht_pred_root(const int32_t* v, int64_t weight, int32_t channels, const int32_t* h_steps, int32_t* v_out, int32_t* m_out,
                                  int32_t* d_flag, void* stream) {
  RahtSteps st;
  if (!raht_steps("pcc_raht_pred_root", channels, h_steps, &st)) return PCC_EINVAL;
  PCC_REQUIRE(v && v_out && m_out && d_flag && weight >= 1 && weight < (1ll << 26), "pcc_raht_pred_root: bad arguments");
  k_raht_pred_root<<<1, 64, 0, (hipStream_t)stream>>>(v, (int)weight, channels, st, v_out, m_out, d_flag);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

static int raht_pred_launch(const char* what, bool encode, const int64_t* keys, int64_t n, int32_t pitch, const uint64_t* bits,
                            const int32_t* rank, const int32_t* h_grid, const int64_t* child_keys, int64_t n_child,
                            const uint64_t* child_bits, const int32_t* child_rank, const int32_t* h_child, const int32_t* off,
                            const int32_t* child_w, const int32_t* v, const int32_t* m, int32_t channels, const int32_t* h_steps,
                            const int32_t* h_true, int32_t* coef, int64_t row_base, int64_t rows_total, int32_t* child_v, int32_t* child_m,
                            int32_t* d_flag, void* stream) {
  LiftLevel L;
  RahtSteps st;
  if (!lift_level(what, keys, n, pitch, bits, rank, h_grid, child_keys, n_child, child_bits, child_rank, h_child, &L)) return PCC_EINVAL;
  if (!raht_steps(what, channels, h_steps, &st)) return PCC_EINVAL;
  if (!(off && v && m && coef && child_v && d_flag && (!encode || h_true) && row_base >= 0 && rows_total > 0 && rows_total < (1ll << 26) &&
        (child_m || !child_w))) {
    pcc_set_error("%s: bad arguments (the children's means are left out only where the children are voxels)", what);
    return PCC_EINVAL;
  }
  const unsigned blocks = (unsigned)pcc_cdiv(n, 256);
  if (encode)
    k_raht_pred_level<true><<<blocks, 256, 0, (hipStream_t)stream>>>(L, off, child_w, v, m, channels, st, h_true, coef, row_base, rows_total,
                                                                      child_v, child_m, d_flag);
  else
    k_raht_pred_level<false><<<blocks, 256, 0, (hipStream_t)stream>>>(L, off, child_w, v, m, channels, st, nullptr, coef, row_base, rows_total,
                                                                       child_v, child_m, d_flag);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_raht_pred_encode(const int64_t* keys, int64_t n, int32_t pitch, const uint64_t* bits, const int32_t* rank,
                                    const int32_t* h_grid, const int64_t* child_keys, int64_t n_child, const uint64_t* child_bits,
                                    const int32_t* child_rank, const int32_t* h_child, const int32_t* off, const int32_t* child_w,
                                    const int32_t* v, const int32_t* m, int32_t channels, const int32_t* h_steps, const int32_t* h_true,
                                    int32_t* coef, int64_t row_base, int64_t rows_total, int32_t* child_v, int32_t* child_m, int32_t* d_flag,
                                    void* stream) {
  return raht_pred_launch("pcc_raht_pred_encode", true, keys, n, pitch, bits, rank, h_grid, child_keys, n_child, child_bits, child_rank, h_child,
                          off, child_w, v, m, channels, h_steps, h_true, coef, row_base, rows_total, child_v, child_m, d_flag, stream);
}

extern "C" int pcc_raht_pred_inverse(const int64_t* keys, int64_t n, int32_t pitch, const uint64_t* bits, const int32_t* rank,
                                     const int32_t* h_grid, const int64_t* child_keys, int64_t n_child, const uint64_t* child_bits,
                                     const int32_t* child_rank, const int32_t* h_child, const int32_t* off, const int32_t* child_w,
                                     const int32_t* v, const int32_t* m, int32_t channels, const int32_t* h_steps, const int32_t* coef,
                                     int64_t row_base, int64_t rows_total, int32_t* child_v, int32_t* child_m, int32_t* d_flag, void* stream) {
  return raht_pred_launch("pcc_raht_pred_inverse", false, keys, n, pitch, bits, rank, h_grid, child_keys, n_child, child_bits, child_rank,
                          h_child, off, child_w, v, m, channels, h_steps, nullptr, const_cast<int32_t*>(coef), row_base, rows_total, child_v,
                          child_m, d_flag, stream);
}
