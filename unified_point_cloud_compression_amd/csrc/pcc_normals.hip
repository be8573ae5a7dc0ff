// Radius normal estimation for the point-to-plane (D2) distortion (reference `evaluate.py:153`:
// `rec_pc.estimate_normals(KDTreeSearchParamRadius(radius=5.0))`, whose normals `utils.py:223` hands to pc_error).
//
// One thread per point of a canonical set at pitch 1, in canonical order.  The neighbourhood of a point is every occupied
// cell at an integer offset d with |d|^2 <= lim (the point itself included); the host passes lim = ceil(r^2) - 1, the strict
// dist^2 < r^2 of a radius search.  It is a set of (dx, dy) columns, and the z cells of a column within the radius are one bit
// field of the set's occupancy bitmap (at most 15 bits for lim <= 63, so at most two 64-bit words), clipped to the lattice as
// in pcc_chconv.  Only the moments of the neighbourhood are needed -- n, S1 = sum d, S2 = sum d d^T -- and they are exact
// integers: sum dz and sum dz^2 of a column come from weighted popcounts of its field, the x / y terms are the column's dx / dy
// times those.  No rows are gathered (the rank array is not read).  Without a grid a column is a binary search for its lowest
// key and a walk over at most 15 keys; the field and so every moment is the same.
//
// M = n S2 - S1 S1^T (int64, n^2 times the covariance Open3D forms) goes to fp64 and a fixed cyclic Jacobi; the eigenvector of
// the smallest eigenvalue is normalised, rounded to fp32 and flipped so that its largest-magnitude component is positive
// (first axis on a tie).  Fewer than 3 neighbours: (0, 0, 1), as Open3D's EstimateNormals.  Every step is integer or
// order-fixed, so the grid and search paths give the same bits, call after call.
#include "pcc_normals.h"

static constexpr int NRM_MAX_LIM = 63;          // r <= 8: column half-height <= 7, a z field <= 15 bits
static constexpr int NRM_MAX_R = 7;             // floor(sqrt(NRM_MAX_LIM))
static constexpr int NRM_SIDE = 2 * NRM_MAX_R + 1;

struct NrmMoments {
  int n, sx, sy, sz, sxx, syy, szz, sxy, sxz, syz;
};

// column (dx, dy) with field f: bit t <-> dz = t + base.  sum t and sum t^2 over the set bits by weighted popcounts.
__device__ inline void nrm_add_column(NrmMoments& m, unsigned f, int base, int dx, int dy) {
  const int c = __popc(f);
  const int p0 = __popc(f & 0xAAAAu), p1 = __popc(f & 0xCCCCu), p2 = __popc(f & 0xF0F0u), p3 = __popc(f & 0xFF00u);
  const int st = p0 + 2 * p1 + 4 * p2 + 8 * p3;
  const int stt = p0 + 4 * p1 + 16 * p2 + 64 * p3 +
                  2 * (2 * __popc(f & 0x8888u) + 4 * __popc(f & 0xA0A0u) + 8 * __popc(f & 0xAA00u) +
                       8 * __popc(f & 0xC0C0u) + 16 * __popc(f & 0xCC00u) + 32 * __popc(f & 0xF000u));
  const int sz = st + c * base;
  const int szz = stt + 2 * base * st + c * base * base;
  m.n += c;
  m.sx += dx * c; m.sy += dy * c; m.sz += sz;
  m.sxx += dx * dx * c; m.syy += dy * dy * c; m.szz += szz;
  m.sxy += dx * dy * c; m.sxz += dx * sz; m.syz += dy * sz;
}

// z field of column (dx, dy), half-height zr, around the point with key `key` (decoded: b, X, Y, Z biased fields)
__device__ inline void nrm_column(const NrmArgs& a, NrmMoments& m, long long b, int X, int Y, int Z, int dx, int dy, int zr) {
  if (a.g.bits) {
    const PccLattice& L = a.g.lat;
    const int nx = X - (int)PCC_BIAS - L.lo[0] + dx, ny = Y - (int)PCC_BIAS - L.lo[1] + dy;
    if (nx < 0 || ny < 0 || nx >= L.dims[0] || ny >= L.dims[1]) return;
    const int z = Z - (int)PCC_BIAS - L.lo[2];
    const int zlo = max(z - zr, 0), zhi = min(z + zr, L.dims[2] - 1);
    if (zlo > zhi || b >= L.nbatch) return;                      // (a key of the set never is outside its own lattice)
    const int nz = zhi - zlo + 1;
    const long long cell = pcc_lat_cell(L, b, nx, ny, zlo);
    const long long wi = cell >> 6;
    const int sh = (int)(cell & 63);
    unsigned long long f64 = a.g.bits[wi] >> sh;
    if (sh + nz > 64) f64 |= a.g.bits[wi + 1] << (64 - sh);     // (the field's last cell is inside the lattice)
    const unsigned f = (unsigned)f64 & ((1u << nz) - 1u);
    if (f) nrm_add_column(m, f, zlo - z, dx, dy);
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
  unsigned f = 0;
  for (; lo < a.n; ++lo) {                                       // at most 2 * zr + 1 <= 15 keys
    const long long k = a.keys[lo];
    if (k > khi) break;
    f |= 1u << (int)((k & PCC_KEY_FIELD) - zlo);
  }
  if (f) nrm_add_column(m, f, zlo - Z, dx, dy);
}

__global__ void __launch_bounds__(256) k_normals(NrmArgs a, float* __restrict__ normals, int* __restrict__ counts) {
  __shared__ signed char s_zr[NRM_SIDE * NRM_SIDE];            // half-height of column (dx, dy), -1: outside the radius
  for (int i = threadIdx.x; i < NRM_SIDE * NRM_SIDE; i += blockDim.x) {
    const int dx = i % NRM_SIDE - NRM_MAX_R, dy = i / NRM_SIDE - NRM_MAX_R;
    const int rest = a.lim - dx * dx - dy * dy;
    int zr = -1;
    if (rest >= 0) { zr = 0; while ((zr + 1) * (zr + 1) <= rest) ++zr; }
    s_zr[i] = (signed char)zr;
  }
  __syncthreads();
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const long long key = a.keys[i];
  const long long b = key >> PCC_KEY_B_SHIFT;
  const int X = (int)((key >> PCC_KEY_X_SHIFT) & PCC_KEY_FIELD), Y = (int)((key >> PCC_KEY_Y_SHIFT) & PCC_KEY_FIELD), Z = (int)(key & PCC_KEY_FIELD);
  NrmMoments m = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int dy = -a.R; dy <= a.R; ++dy)
    for (int dx = -a.R; dx <= a.R; ++dx) {
      const int zr = s_zr[(dy + NRM_MAX_R) * NRM_SIDE + dx + NRM_MAX_R];
      if (zr >= 0) nrm_column(a, m, b, X, Y, Z, dx, dy, zr);
    }
  if (counts) counts[i] = m.n;
  float out[3] = {0.f, 0.f, 1.f};
  if (m.n >= 3) {
    const long long N = m.n;
    const long long m00 = N * m.sxx - (long long)m.sx * m.sx, m11 = N * m.syy - (long long)m.sy * m.sy;
    const long long m22 = N * m.szz - (long long)m.sz * m.sz, m01 = N * m.sxy - (long long)m.sx * m.sy;
    const long long m02 = N * m.sxz - (long long)m.sx * m.sz, m12 = N * m.syz - (long long)m.sy * m.sz;
    double A[3][3] = {{(double)m00, (double)m01, (double)m02}, {(double)m01, (double)m11, (double)m12},
                      {(double)m02, (double)m12, (double)m22}};
    double v[3];
    nrm_smallest_eigvec(A, v);
    const double inv = 1.0 / sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    for (int k = 0; k < 3; ++k) out[k] = (float)(v[k] * inv);
    float big = out[0];                          // the largest-magnitude component, the first one on a tie
    if (fabsf(out[1]) > fabsf(big)) big = out[1];
    if (fabsf(out[2]) > fabsf(big)) big = out[2];
    if (big < 0.f) { out[0] = -out[0]; out[1] = -out[1]; out[2] = -out[2]; }
  }
  normals[3 * i] = out[0];
  normals[3 * i + 1] = out[1];
  normals[3 * i + 2] = out[2];
}

extern "C" int pcc_normals_grid(const int64_t* keys, int64_t n, const uint64_t* grid_bits, const int32_t* h_grid, int32_t lim,
                                float* normals, int32_t* counts, void* stream) {
  PCC_REQUIRE(lim >= 0 && lim <= NRM_MAX_LIM, "pcc_normals_grid: lim %d outside 0 .. %d (radius above 8)", lim, NRM_MAX_LIM);
  PCC_REQUIRE(n >= 0 && n < (1ll << 31), "pcc_normals_grid: too many rows");
  if (n == 0) return PCC_OK;
  PCC_REQUIRE(keys && normals, "pcc_normals_grid: NULL array");
  NrmArgs a;
  PCC_TRY(nrm_fill_args(a, "pcc_normals_grid", keys, n, grid_bits, nullptr, h_grid, lim));
  k_normals<<<(unsigned)pcc_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(a, normals, counts);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}
