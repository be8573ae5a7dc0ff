// RAHT colour coder, the device helpers its source files share: the integer butterfly arithmetic, a
// node's factor pairs, the three forward stages of a node over one channel, the quantiser, the mean and scale of the prediction
// from the parent level, and the argument checks of a level's entry point with its quantiser steps.  The probes of a level's
// children, the existence rule of a node's seven butterflies and the block level of an inter frame are pcc_oct_level.h's, shared
// with the lifting coder.  pcc_raht.hip (the intra coder), pcc_raht_inter.hip (inter frames) and pcc_raht_pred.hip (prediction
// from the parent level) include it.
#pragma once
#include "pcc_oct_level.h"

static constexpr int RAHT_MAX_C = 8;
static constexpr int RAHT_BINS = 128;                 // 127 values -63..63 + the escape slot
static constexpr int RAHT_MAX_GROUPS = 15 * 6;        // (level, class, stage)
static constexpr long long RAHT_ROUND = 1ll << 29;    // Q30 products
static constexpr long long RAHT_LIMIT = 1ll << 30;    // the decoder's clamp (valid streams stay below 2^29 + quantisation error)

struct RahtSteps { int v[RAHT_MAX_C]; };

struct RahtLevel {
  const int64_t* keys; int n; int pitch;              // the nodes
  const int64_t* ckeys; int nc; PccGrid cg;           // their children: the canonical set at pitch / 2
};

__host__ __device__ inline unsigned long long raht_isqrt(unsigned long long x) {      // exact floor square root, x < 2^62
  unsigned long long r = (unsigned long long)sqrt((double)x);
  while (r * r > x) --r;
  while ((r + 1) * (r + 1) <= x) ++r;
  return r;
}

// Q30 factors sqrt(w1 / w), sqrt(w2 / w) of a butterfly, w1, w2 >= 1, w1 + w2 < 2^27
__host__ __device__ inline void raht_factors(unsigned w1, unsigned w2, long long& a, long long& b) {
  const unsigned long long w = (unsigned long long)w1 + w2;
  a = (long long)raht_isqrt((((unsigned long long)w1 << 32) / w) << 28);
  b = (long long)raht_isqrt((((unsigned long long)w2 << 32) / w) << 28);
}

__host__ __device__ inline void raht_fwd(long long a, long long b, long long x1, long long x2, long long& lo, long long& hi) {
  lo = (a * x1 + b * x2 + RAHT_ROUND) >> 30;
  hi = (a * x2 - b * x1 + RAHT_ROUND) >> 30;
}

__host__ __device__ inline void raht_inv(long long a, long long b, long long lo, long long hi, long long& x1, long long& x2) {
  x1 = (a * lo - b * hi + RAHT_ROUND) >> 30;
  x2 = (b * lo + a * hi + RAHT_ROUND) >> 30;
}

// the butterflies' factors (weights only: shared by the channels), the slot weights, and the node's weight
struct RahtNode { long long a[7], b[7]; bool e[7]; int weight; };

__device__ inline void raht_node(const int w[8], RahtNode& nd) {
  int mask = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) mask |= (w[j] > 0) << j;
  oct_emits(mask, nd.e);
  int w1[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    w1[k] = w[2 * k] + w[2 * k + 1];
    nd.a[3 + k] = nd.b[3 + k] = 0;
    if (nd.e[3 + k]) raht_factors((unsigned)w[2 * k], (unsigned)w[2 * k + 1], nd.a[3 + k], nd.b[3 + k]);
  }
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    nd.a[1 + m] = nd.b[1 + m] = 0;
    if (nd.e[1 + m]) raht_factors((unsigned)w1[2 * m], (unsigned)w1[2 * m + 1], nd.a[1 + m], nd.b[1 + m]);
  }
  nd.a[0] = nd.b[0] = 0;
  if (nd.e[0]) raht_factors((unsigned)(w1[0] + w1[1]), (unsigned)(w1[2] + w1[3]), nd.a[0], nd.b[0]);
  nd.weight = w1[0] + w1[1] + w1[2] + w1[3];
}

// the three stages of a node over one channel's child values x[8] (0 where absent): h[7] in row order (0 where the butterfly
// does not exist); returns the node's DC.  The arithmetic of k_raht_forward.
__device__ inline long long raht_node_fwd(const RahtNode& nd, const long long x[8], long long h[7]) {
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
  return dc;
}

__device__ inline int raht_quantise(long long h, long long step) {
  const long long m = h < 0 ? -h : h;
  const long long q = (m + (step >> 1)) / step;
  return (int)(h < 0 ? -q : q);
}

// ---- prediction from the parent level (stream 0xB9; pcc_raht_pred.hip) ---------------------------------------------------------
static constexpr int RAHT_PRED_MEAN_LIMIT = 1 << 24;  // the clamp on a node's mean (a valid one is below 2^17): 64 of them sum in int32

// a node's mean from its DC, dc / sqrt(w): a is the Q30 factor of "1 of w" (at most 2^30), so w = 1 gives the DC itself.
// |dc| <= 2^30, 1 <= w < 2^26
__host__ __device__ inline unsigned raht_pred_mean_factor(unsigned w) { return (unsigned)raht_isqrt(((1ull << 32) / w) << 28); }
__host__ __device__ inline long long raht_pred_mean(long long dc, unsigned a) { return ((long long)a * dc + RAHT_ROUND) >> 30; }

// Q16 sqrt(w) of a child, 0 <= w < 2^26 (below 2^29), and a prediction brought into that child's domain: pred * sqrt(w)
__host__ __device__ inline int raht_pred_factor(unsigned w) { return (int)raht_isqrt((unsigned long long)w << 32); }
__host__ __device__ inline long long raht_pred_scale(long long pred, int s) { return (pred * s + (1ll << 15)) >> 16; }

// ---- argument checks of the entry points -----------------------------------------------------------------------------------
static bool raht_level(const char* what, const int64_t* keys, int64_t n, int32_t pitch, const int64_t* child_keys, int64_t n_child,
                       const uint64_t* child_bits, const int32_t* child_rank, const int32_t* h_child, RahtLevel* L) {
  if (!oct_level(what, keys, n, pitch, child_keys, n_child, L)) return false;
  if (pcc_grid_from_host(child_bits, child_rank, h_child, what, &L->cg) != PCC_OK) return false;   // bits == NULL: binary search
  if (L->cg.bits && h_child[6] != pitch / 2) {
    pcc_set_error("%s: the child grid has another pitch", what);
    return false;
  }
  return true;
}

static bool raht_steps(const char* what, int32_t channels, const int32_t* h_steps, RahtSteps* s) {
  if (channels < 1 || channels > RAHT_MAX_C || !h_steps) { pcc_set_error("%s: 1 .. 8 channels and their steps are required", what); return false; }
  for (int c = 0; c < RAHT_MAX_C; ++c) s->v[c] = 1;
  for (int c = 0; c < channels; ++c) {
    if (h_steps[c] < 1 || h_steps[c] > (1 << 16)) { pcc_set_error("%s: step %d outside 1 .. 2^16", what, h_steps[c]); return false; }
    s->v[c] = h_steps[c];
  }
  return true;
}
