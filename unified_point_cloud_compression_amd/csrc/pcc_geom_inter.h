// Block motion of the inter frames, what the geometry coder (pcc_geom_inter.hip) and the colour coder (pcc_lift_inter.hip) share:
// the candidate vectors in their coded order, the packed displacements of the wide search, the layout of a block's occupancy
// pyramid and the probe of a reference set given in absolute coordinates.
#pragma once
#include "pcc_common.h"
#include "pcc_conv.h"

static constexpr int INTER_MAX_CAND = 125;

static constexpr int INTER_PYR = 75;                     // words per block: tier 4 at 0 (64), tier 3 at 64 (8), tiers 2, 1, 0 at 72, 73, 74

__device__ __forceinline__ int inter_tier(int e) { return e == 4 ? 0 : (e == 3 ? 64 : 74 - e); }

struct InterCands { int n; int v[INTER_MAX_CAND]; };     // (dx + 8) | (dy + 8) << 4 | (dz + 8) << 8, by |v|^2 then lexicographically

// a voxel of a set given in ABSOLUTE coordinates (any sign inside the key range)
__device__ inline bool inter_has(const PccGrid& g, const int64_t* __restrict__ keys, int n, int x, int y, int z) {
  const int B = (int)PCC_BIAS;
  if (x < -B || y < -B || z < -B || x >= B || y >= B || z >= B) return false;
  return pcc_lookup(g, keys, n, pcc_key_pack(0, x, y, z)) >= 0;
}

// The finest tier of a block's pyramid, probed by one wave: word `lane` of tier bl in the LDS pyramid w gets bit `bit` = cell
// c = 64 lane + bit = (lx << 2 bl | ly << bl | lz) of the block whose corner, already displaced, is (x0, y0, z0), set when the
// source (sg, skeys, ns) holds that voxel.  Shared by the block-bits kernels of pcc_geom_inter.hip, pcc_geom_wide.hip and
// pcc_geom_multi.hip -- as a statement macro, not a function: through a function (by reference, by value, returning the word) the
// two older kernels came out with other scalar registers (tools/kernel_identity.py), and their instruction text is a record.
// Declares cells, side, words and per in the caller's scope.
#define INTER_PROBE_FINEST(w, lane, bl, sg, skeys, ns, x0, y0, z0)                                                                  \
  const int cells = 1 << (3 * (bl)), side = (1 << (bl)) - 1;                                                                        \
  const int words = cells > 64 ? cells >> 6 : 1, per = cells < 64 ? cells : 64;                                                     \
  if ((lane) < words) {                                                                                                             \
    unsigned long long m = 0;                                                                                                       \
    for (int bit = 0; bit < per; ++bit) {                                                                                           \
      const int c = (lane) * 64 + bit;                                                                                              \
      if (inter_has(sg, skeys, ns, (x0) + (c >> (2 * (bl))), (y0) + ((c >> (bl)) & side), (z0) + (c & side))) m |= 1ull << bit;      \
    }                                                                                                                               \
    (w)[inter_tier(bl) + (lane)] = m;                                                                                               \
  }

// its row in the set (-1: absent, or a row the set does not have)
__device__ inline int inter_row(const PccGrid& g, const int64_t* __restrict__ keys, int n, int x, int y, int z) {
  const int B = (int)PCC_BIAS;
  if (n <= 0 || x < -B || y < -B || z < -B || x >= B || y >= B || z >= B) return -1;
  const int r = pcc_lookup(g, keys, n, pcc_key_pack(0, x, y, z));
  return r < n ? r : -1;
}

__device__ __forceinline__ void inter_cand(const InterCands& c, int j, int& dx, int& dy, int& dz) {
  const int p = c.v[j];
  dx = (p & 15) - 8; dy = ((p >> 4) & 15) - 8; dz = ((p >> 8) & 15) - 8;
}

// ---- the wide search (pcc_geom_wide.hip): a vector is a packed DISPLACEMENT, the packing of InterCands::v, not an index ----------
__device__ __forceinline__ int wide_pack(int dx, int dy, int dz) { return (dx + 8) | ((dy + 8) << 4) | ((dz + 8) << 8); }

// the displacement of a packed word, (0, 0, 0) and false when a component leaves +-search
__device__ __forceinline__ bool wide_unpack(int p, int search, int& dx, int& dy, int& dz) {
  dx = (p & 15) - 8; dy = ((p >> 4) & 15) - 8; dz = ((p >> 8) & 15) - 8;
  const bool ok = (p >> 12) == 0 && dx >= -search && dx <= search && dy >= -search && dy <= search && dz >= -search && dz <= search;
  if (!ok) dx = dy = dz = 0;
  return ok;
}

static int inter_cands(int search, const char* who, InterCands* out) {
  PCC_REQUIRE(search >= 0 && search <= 2, "%s: search range %d outside 0..2", who, search);
  int n = 0, v[INTER_MAX_CAND][3];
  for (int dx = -search; dx <= search; ++dx)
    for (int dy = -search; dy <= search; ++dy)
      for (int dz = -search; dz <= search; ++dz) { v[n][0] = dx; v[n][1] = dy; v[n][2] = dz; ++n; }
  // by |v|^2, then lexicographically: the enumeration above is lexicographic, and an insertion sort on the norm is stable
  for (int i = 1; i < n; ++i) {
    int t[3] = {v[i][0], v[i][1], v[i][2]};
    const int nt = t[0] * t[0] + t[1] * t[1] + t[2] * t[2];
    int j = i - 1;
    while (j >= 0 && v[j][0] * v[j][0] + v[j][1] * v[j][1] + v[j][2] * v[j][2] > nt) {
      v[j + 1][0] = v[j][0]; v[j + 1][1] = v[j][1]; v[j + 1][2] = v[j][2];
      --j;
    }
    v[j + 1][0] = t[0]; v[j + 1][1] = t[1]; v[j + 1][2] = t[2];
  }
  memset(out, 0, sizeof(*out));
  out->n = n;
  for (int i = 0; i < n; ++i) out->v[i] = (v[i][0] + 8) | ((v[i][1] + 8) << 4) | ((v[i][2] + 8) << 8);
  return PCC_OK;
}

static bool inter_origin_ok(int ox, int oy, int oz) {
  const int B = 1 << 15;
  return ox >= -B && oy >= -B && oz >= -B && ox < B && oy < B && oz < B;
}
