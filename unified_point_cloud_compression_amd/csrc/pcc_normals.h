// Helpers shared by the radius kernels over a canonical pitch-1 set (pcc_normals.hip, pcc_pcqm.hip): the z cells of a
// (dx, dy) column as one bit field of the set's occupancy bitmap (or of a binary search over the keys: the same field), and
// the fixed-sweep Jacobi that gives the normal.
#pragma once
#include "pcc_common.h"

static constexpr int NRM_JACOBI_SWEEPS = 8;

struct NrmArgs {
  const long long* keys; int n;
  PccGrid g;                                     // g.bits == nullptr: binary search
  int lim, R;                                    // R = floor(sqrt(lim))
};

// z field of column (dx, dy), half-height zr, around the point with key `key` (decoded: b, X, Y, Z biased fields), for columns
// wider than k_normals' and for kernels that read the members' rows: F holds 2 * zr + 1 bits.  When the column holds a member,
// use(f, base, row0) is called once with the field f, bit t <-> dz = t + base.  ROWS: row0 = the canonical row
// of the field's lowest set bit, and the other set bits follow it consecutively (canonical order is ascending cell index, z
// fastest): with a grid that is rank + popcount (g.rank must be set), without one the search's lower bound.  Else row0 = 0.
// (k_normals keeps its own 32-bit nrm_column in pcc_normals.hip: routed through this template it computes the same field but
// its registers are allocated differently, and its code is held to the instruction.)
template <typename F, bool ROWS, typename Use>
__device__ inline void nrm_field(const NrmArgs& a, long long b, int X, int Y, int Z, int dx, int dy, int zr, Use use) {
  if (a.g.bits) {
    const PccLattice& L = a.g.lat;
    const int nx = X - (int)PCC_BIAS - L.lo[0] + dx, ny = Y - (int)PCC_BIAS - L.lo[1] + dy;
    if (nx < 0 || ny < 0 || nx >= L.dims[0] || ny >= L.dims[1]) return;
    const int z = Z - (int)PCC_BIAS - L.lo[2];
    const int zlo = max(z - zr, 0), zhi = min(z + zr, L.dims[2] - 1);
    if (zlo > zhi || b >= L.nbatch) return;                      // (a key of the set never is outside its own lattice)
    const int nz = zhi - zlo + 1;
    // (spelled out: through pcc_lat_cell the pcqm kernels come out with other instructions, tools/kernel_identity.py)
    const long long cell = ((b * L.dims[0] + nx) * L.dims[1] + ny) * (long long)L.dims[2] + zlo;
    const long long wi = cell >> 6;
    const int sh = (int)(cell & 63);
    unsigned long long f64 = a.g.bits[wi] >> sh;
    if (sh + nz > 64) f64 |= a.g.bits[wi + 1] << (64 - sh);     // (the field's last cell is inside the lattice)
    const F f = (F)f64 & (((F)1 << nz) - (F)1);
    if (f) use(f, zlo - z, ROWS ? a.g.rank[wi] + __popcll(a.g.bits[wi] & ((1ull << sh) - 1ull)) : 0);
    return;
  }
  const int tx = X + dx, ty = Y + dy;
  if (tx < 0 || ty < 0 || tx > PCC_KEY_FIELD || ty > PCC_KEY_FIELD) return;
  const int zlo = max(Z - zr, 0), zhi = min(Z + zr, PCC_KEY_FIELD);
  const long long col = (b << PCC_KEY_B_SHIFT) | ((long long)tx << PCC_KEY_X_SHIFT) | ((long long)ty << PCC_KEY_Y_SHIFT);
  const long long klo = col | zlo, khi = col | zhi;
  int lo = 0, hi = a.n;                                          // first key >= klo
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a.keys[mid] < klo) lo = mid + 1; else hi = mid;
  }
  F f = 0;
  int row0 = 0;
  if constexpr (ROWS) row0 = lo;
  for (; lo < a.n; ++lo) {                                       // at most 2 * zr + 1 keys
    const long long k = a.keys[lo];
    if (k > khi) break;
    f |= (F)1 << (int)((k & PCC_KEY_FIELD) - zlo);
  }
  if (f) use(f, zlo - Z, row0);
}

// eigenvector of the smallest eigenvalue of the symmetric A (fp64, overwritten) by cyclic Jacobi with a fixed sweep count
__device__ inline void nrm_smallest_eigvec(double A[3][3], double v[3]) {
  double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int sweep = 0; sweep < NRM_JACOBI_SWEEPS; ++sweep) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int p = r == 2 ? 1 : 0, q = r == 0 ? 1 : 2, o = 3 - p - q;
      const double apq = A[p][q];
      if (apq == 0.0) continue;
      const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
      const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
      const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
      A[p][p] -= t * apq;
      A[q][q] += t * apq;
      A[p][q] = A[q][p] = 0.0;
      const double aop = A[o][p], aoq = A[o][q];
      A[o][p] = A[p][o] = c * aop - s * aoq;
      A[o][q] = A[q][o] = s * aop + c * aoq;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double vp = V[k][p], vq = V[k][q];
        V[k][p] = c * vp - s * vq;
        V[k][q] = s * vp + c * vq;
      }
    }
  }
  int j = 0;                                     // (selects, not an indexed read: keeps A and V in registers)
  double lo = A[0][0];
  if (A[1][1] < lo) { lo = A[1][1]; j = 1; }
  if (A[2][2] < lo) j = 2;
#pragma unroll
  for (int k = 0; k < 3; ++k) v[k] = j == 0 ? V[k][0] : (j == 1 ? V[k][1] : V[k][2]);
}

// half-height of column (dx, dy) inside |d|^2 <= lim, -1: the column is outside the radius
__device__ inline int nrm_column_half_height(int lim, int dx, int dy) {
  const int rest = lim - dx * dx - dy * dy;
  int zr = -1;
  if (rest >= 0) { zr = 0; while ((zr + 1) * (zr + 1) <= rest) ++zr; }
  return zr;
}

// the host side of NrmArgs: the grid header (pitch 1) or none, lim and its R
static inline int nrm_fill_args(NrmArgs& a, const char* who, const int64_t* keys, int64_t n, const uint64_t* grid_bits,
                                const int32_t* grid_rank, const int32_t* h_grid, int32_t lim) {
  a = NrmArgs();
  if (grid_bits) {                               // (rank[] is optional here: only the kernels that read rows need it)
    PCC_TRY(pcc_lattice_from_host(h_grid, who, &a.g.lat));
    PCC_REQUIRE(h_grid[6] == 1, "%s: grid pitch %d, the set must be at pitch 1", who, h_grid[6]);
    a.g.bits = (const unsigned long long*)grid_bits;
    a.g.rank = grid_rank;
  }
  a.keys = (const long long*)keys; a.n = (int)n; a.lim = lim;
  a.R = 0;
  while ((a.R + 1) * (a.R + 1) <= lim) ++a.R;
  return PCC_OK;
}
