// RAHT colour coder, the device helpers its source files share: the integer butterfly arithmetic, the
// existence rule of a node's seven butterflies, a node's factor pairs, the probes of a level's children, and the argument
// checks of a level's entry point.  pcc_raht.hip (the intra coder) and pcc_raht_inter.hip (inter frames) include it.
#pragma once
#include "pcc_common.h"
#include "pcc_conv.h"

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

// rows of the eight children (-1: absent); returns the occupancy byte
__device__ inline int raht_kids(const RahtLevel& L, int i, int kid[8]) {
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

// which of the seven butterflies of a node exist, in row order: [0] stage 3, [1] [2] stage 2 (slot 0, 4), [3..6] stage 1
__host__ __device__ inline void raht_emits(int mask, bool e[7]) {
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

// the butterflies' factors (weights only: shared by the channels), the slot weights, and the node's weight
struct RahtNode { long long a[7], b[7]; bool e[7]; int weight; };

__device__ inline void raht_node(const int w[8], RahtNode& nd) {
  int mask = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) mask |= (w[j] > 0) << j;
  raht_emits(mask, nd.e);
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

__device__ inline void raht_child_weights(const int* __restrict__ cw, const int kid[8], int w[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) w[j] = kid[j] < 0 ? 0 : (cw ? cw[kid[j]] : 1);      // cw == nullptr: the children are voxels
}

// ---- argument checks of the entry points -----------------------------------------------------------------------------------
static bool raht_level(const char* what, const int64_t* keys, int64_t n, int32_t pitch, const int64_t* child_keys, int64_t n_child,
                       const uint64_t* child_bits, const int32_t* child_rank, const int32_t* h_child, RahtLevel* L) {
  if (!(keys && child_keys && n > 0 && n_child >= n && n_child < (1ll << 26))) {
    pcc_set_error("%s: bad arguments (a level of n >= 1 nodes with n .. 2^26 - 1 children)", what);
    return false;
  }
  if (!(pitch >= 2 && pitch <= (1 << 15) && pcc_is_pow2(pitch))) {
    pcc_set_error("%s: pitch %d is not a power of two in [2, 2^15]", what, pitch);
    return false;
  }
  if (pcc_grid_from_host(child_bits, child_rank, h_child, what, &L->cg) != PCC_OK) return false;   // bits == NULL: binary search
  if (L->cg.bits && h_child[6] != pitch / 2) {
    pcc_set_error("%s: the child grid has another pitch", what);
    return false;
  }
  L->keys = keys; L->n = (int)n; L->pitch = pitch; L->ckeys = child_keys; L->nc = (int)n_child;
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
