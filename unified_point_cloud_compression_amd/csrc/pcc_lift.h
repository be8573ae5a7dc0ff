// Lossless attribute coder, the device helpers its source files share: the reversible lifting arithmetic
// and the probes only this coder makes -- the 27 cells around a node in its own level, and the lifted prediction of the children
// from the level's own values.  A node's eight children, their weights, the existence rule of its seven butterflies and the block
// level of an inter frame are pcc_oct_level.h's, shared with the RAHT coder.
// pcc_lift.hip (the intra coder) and pcc_lift_inter.hip (the last level of an inter frame) include it.
#pragma once
#include "pcc_oct_level.h"

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
  return oct_floor_div32(num + (den >> 1), den);
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

// the predictions of channel c of a node's present children from the level's values v (0 where kid[j] < 0).  Cell b of child j
// lies at offset d * b per axis, d = 2 * (the child's bit) - 1.
__device__ inline void lift_child_preds(const int* __restrict__ v, int C, int c, const int nb[27], const int kid[8], int pred[8]) {
  int nv[27];
#pragma unroll
  for (int k = 0; k < 27; ++k) nv[k] = nb[k] < 0 ? 0 : v[(size_t)nb[k] * C + c];
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
}

// hp[7] of channel c of a node: the predictions of its present children from the level's values v, lifted with the children's
// weights.  The first half is lift_child_preds written out again: with a call in its place the compiler schedules k_lift_residual
// and k_lift_inverse differently (7 instructions fewer each; tools/kernel_identity.py shows it), and those kernels stay as they are.
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

// the bounds and the grid indices of a level's entry point (node grid NULL: the neighbours are searched)
static bool lift_level(const char* what, const int64_t* keys, int64_t n, int32_t pitch, const uint64_t* bits, const int32_t* rank,
                       const int32_t* h_grid, const int64_t* child_keys, int64_t n_child, const uint64_t* child_bits,
                       const int32_t* child_rank, const int32_t* h_child, LiftLevel* L) {
  if (!oct_level(what, keys, n, pitch, child_keys, n_child, L)) return false;
  if (pcc_grid_from_host(bits, rank, h_grid, what, &L->g) != PCC_OK) return false;                 // bits == NULL: binary search
  if (pcc_grid_from_host(child_bits, child_rank, h_child, what, &L->cg) != PCC_OK) return false;
  if ((L->g.bits && h_grid[6] != pitch) || (L->cg.bits && h_child[6] != pitch / 2)) {
    pcc_set_error("%s: a grid index has another pitch than its level", what);
    return false;
  }
  return true;
}
