// One level of the octree as the colour coders walk it (DESIGN.md sections 7f and 7i), the device helpers the RAHT and the lifting
// coder share: the block level of an inter frame with its lookup and host validator, the probe of a node's eight children, the
// existence rule of a node's seven butterflies, the children's weights, the 32-bit floor division, and the argument checks every
// level's entry point opens with.  pcc_raht.h and pcc_lift.h include it; each keeps its own level type (the kernels' argument
// layouts), which the templates below read by member name.
#pragma once
#include "pcc_common.h"
#include "pcc_conv.h"

struct OctBlocks { const int64_t* keys; int n; PccGrid g; int bl; };       // the nodes of the block level, origin-relative

// the row of the block that holds an origin-relative cell (-1: none, which a consistent geometry never gives)
__device__ inline int oct_block_of(const OctBlocks& B, int64_t key) {
  const int bm = (1 << B.bl) - 1;
  const int x = pcc_key_x(key), y = pcc_key_y(key), z = pcc_key_z(key);
  if ((x | y | z) < 0 || x >= (int)PCC_BIAS || y >= (int)PCC_BIAS || z >= (int)PCC_BIAS) return -1;
  const int row = pcc_lookup(B.g, B.keys, B.n, pcc_key_pack(0, x & ~bm, y & ~bm, z & ~bm));
  return (row >= 0 && row < B.n) ? row : -1;
}

__host__ __device__ inline int oct_floor_div32(int a, int d) {      // d >= 1
  int q = a / d;
  if (a % d < 0) --q;
  return q;
}

// rows of the eight children (-1: absent); returns the occupancy byte.  Level: RahtLevel or LiftLevel (keys, pitch, ckeys, nc, cg)
template <class Level>
__device__ inline int oct_kids(const Level& L, int i, int kid[8]) {
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
__host__ __device__ inline void oct_emits(int mask, bool e[7]) {
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

__device__ inline void oct_child_weights(const int* __restrict__ cw, const int kid[8], int w[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) w[j] = kid[j] < 0 ? 0 : (cw ? cw[kid[j]] : 1);      // cw == nullptr: the children are voxels
}

// ---- argument checks of the entry points -----------------------------------------------------------------------------------
// the bounds of a level and its children; fills every member of L but the grid indices, which the caller checks next
template <class Level>
static bool oct_level(const char* what, const int64_t* keys, int64_t n, int32_t pitch, const int64_t* child_keys, int64_t n_child, Level* L) {
  if (!(keys && child_keys && n > 0 && n_child >= n && n_child < (1ll << 26))) {
    pcc_set_error("%s: bad arguments (a level of n >= 1 nodes with n .. 2^26 - 1 children)", what);
    return false;
  }
  if (!(pitch >= 2 && pitch <= (1 << 15) && pcc_is_pow2(pitch))) {
    pcc_set_error("%s: pitch %d is not a power of two in [2, 2^15]", what, pitch);
    return false;
  }
  L->keys = keys; L->n = (int)n; L->pitch = pitch; L->ckeys = child_keys; L->nc = (int)n_child;
  return true;
}

static bool oct_blocks(const char* what, const int64_t* keys, int64_t n, const uint64_t* bits, const int32_t* rank, const int32_t* h,
                       int32_t block_log2, OctBlocks* B) {
  if (!(keys && n > 0 && n < (1ll << 24) && block_log2 >= 1 && block_log2 <= 4)) {
    pcc_set_error("%s: bad block level (1 .. 2^24 - 1 blocks, block_log2 in 1..4)", what);
    return false;
  }
  if (pcc_grid_from_host(bits, rank, h, what, &B->g) != PCC_OK) return false;
  if (B->g.bits && h[6] != (1 << block_log2)) {
    pcc_set_error("%s: the block grid has another pitch", what);
    return false;
  }
  B->keys = keys; B->n = (int)n; B->bl = block_log2;
  return true;
}
