// The two radius kernels of the PCQM quality metric (metrics.py `pcqm`; Meynet, Nehme, Digne, Lavoue, QoMEX 2020, restated on
// a voxel lattice): the curvature field of a cloud and the eight local features of a paired table.
//
// Both work on a canonical set at pitch 1 and walk the (dx, dy) columns of the integer neighbourhood |d|^2 <= lim as
// k_normals does; the z cells of a column are one bit field of the occupancy bitmap (pcc_normals.h), up to 33 bits for
// lim <= 288 (radius <= 17), so still at most two 64-bit words.  Without a grid a column is a binary search for its lowest
// key and a walk over its keys: the same field, the same rows, the same bits out.
//
// k_curvature: one thread per point.  Pass 1 gives the exact integer moments of the neighbourhood and from them the normal
// of pcc_normals_grid (same matrix, same Jacobi, same sign rule, kept in fp64).  Pass 2 visits the members in the fixed
// order dx, dy, dz ascending, takes each offset to the local frame (u, v, n) and accumulates the 6 x 6 normal equations of
// z = a x^2 + b xy + c y^2 + d x + e y + f in fp64; Cholesky; the absolute mean curvature of the fitted surface at the
// point's foot.  It needs the members' offsets only, so it never reads the rank array or a row.
//
// k_pcqm_features: one wave per point.  Lane l takes the columns l, l + 64, ... of the (dx ascending, dy ascending)
// enumeration, turns every set bit of a column into its row (rank + popcount, the rows of a column are consecutive), reads
// that row of the paired table and accumulates the Gaussian-weighted moments in fp64, every attribute shifted by the
// centre's own value.  The 64 partial sums meet in an xor butterfly: which members a lane sees and the order of every
// addition depend on the set alone, there are no atomics, so the result is the same bits call after call and on both paths.
#include "pcc_normals.h"

static constexpr int PCQM_MAX_LIM = 288;         // radius <= 17: column half-height <= 16, a z field <= 33 bits
static constexpr int PCQM_MAX_R = 16;            // floor(sqrt(PCQM_MAX_LIM))
static constexpr int PCQM_SIDE = 2 * PCQM_MAX_R + 1;
static constexpr int PCQM_MIN_FIT = 6;           // fewer members than unknowns: curvature 0
static constexpr int PCQM_NSUM = 17;
static constexpr int PCQM_COLS = 10;             // columns of the paired table
static constexpr double PCQM_PIVOT_REL = 1e-12;
// feature constants of the published metric (restated from the paper, metrics.py holds the same values)
static constexpr double PCQM_K = 1.0, PCQM_C1 = 0.002, PCQM_C2 = 0.1, PCQM_C3 = 0.1, PCQM_C4 = 0.002, PCQM_C5 = 0.008;

// half-heights of the columns of the (2 R + 1)^2 square, index (dx + R) * (2 R + 1) + dy + R
__device__ inline void pcqm_fill_half_heights(signed char* s_zr, int lim, int R) {
  const int side = 2 * R + 1;
  for (int i = threadIdx.x; i < side * side; i += blockDim.x)
    s_zr[i] = (signed char)nrm_column_half_height(lim, i / side - R, i % side - R);
}

__global__ void __launch_bounds__(256) k_curvature(NrmArgs a, double* __restrict__ out) {
  __shared__ signed char s_zr[PCQM_SIDE * PCQM_SIDE];
  pcqm_fill_half_heights(s_zr, a.lim, a.R);
  __syncthreads();
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const long long key = a.keys[i];
  const long long b = key >> PCC_KEY_B_SHIFT;
  const int X = (int)((key >> PCC_KEY_X_SHIFT) & PCC_KEY_FIELD), Y = (int)((key >> PCC_KEY_Y_SHIFT) & PCC_KEY_FIELD), Z = (int)(key & PCC_KEY_FIELD);
  const int side = 2 * a.R + 1;

  long long cnt = 0, sx = 0, sy = 0, sz = 0, sxx = 0, syy = 0, szz = 0, sxy = 0, sxz = 0, syz = 0;
  for (int dx = -a.R; dx <= a.R; ++dx)
    for (int dy = -a.R; dy <= a.R; ++dy) {
      const int zr = s_zr[(dx + a.R) * side + dy + a.R];
      if (zr < 0) continue;
      nrm_field<unsigned long long, false>(a, b, X, Y, Z, dx, dy, zr, [&](unsigned long long f, int base, int) {
        int c = 0, st = 0, stt = 0;
        while (f) {
          const int dz = __ffsll((long long)f) - 1 + base;
          f &= f - 1;
          ++c; st += dz; stt += dz * dz;
        }
        cnt += c;
        sx += dx * c; sy += dy * c; sz += st;
        sxx += dx * dx * c; syy += dy * dy * c; szz += stt;
        sxy += dx * dy * c; sxz += dx * st; syz += dy * st;
      });
    }
  if (cnt < PCQM_MIN_FIT) { out[i] = 0.0; return; }

  double nv[3];
  {
    const long long m00 = cnt * sxx - sx * sx, m11 = cnt * syy - sy * sy, m22 = cnt * szz - sz * sz;
    const long long m01 = cnt * sxy - sx * sy, m02 = cnt * sxz - sx * sz, m12 = cnt * syz - sy * sz;
    double A[3][3] = {{(double)m00, (double)m01, (double)m02}, {(double)m01, (double)m11, (double)m12},
                      {(double)m02, (double)m12, (double)m22}};
    nrm_smallest_eigvec(A, nv);
    const double inv = 1.0 / sqrt(nv[0] * nv[0] + nv[1] * nv[1] + nv[2] * nv[2]);
    nv[0] *= inv; nv[1] *= inv; nv[2] *= inv;
    double big = nv[0];                          // the largest-magnitude component, the first one on a tie
    if (fabs(nv[1]) > fabs(big)) big = nv[1];
    if (fabs(nv[2]) > fabs(big)) big = nv[2];
    if (big < 0.0) { nv[0] = -nv[0]; nv[1] = -nv[1]; nv[2] = -nv[2]; }
  }
  // in-plane axes: e = the axis where |n| is smallest (the first one on a tie), u = normalise(e x n), v = n x u
  double uv[3], vv[3];
  {
    int e = 0;
    double small = fabs(nv[0]);
    if (fabs(nv[1]) < small) { small = fabs(nv[1]); e = 1; }
    if (fabs(nv[2]) < small) e = 2;
    const double e0 = e == 0 ? 1.0 : 0.0, e1 = e == 1 ? 1.0 : 0.0, e2 = e == 2 ? 1.0 : 0.0;
    uv[0] = e1 * nv[2] - e2 * nv[1];
    uv[1] = e2 * nv[0] - e0 * nv[2];
    uv[2] = e0 * nv[1] - e1 * nv[0];
    const double inv = 1.0 / sqrt(uv[0] * uv[0] + uv[1] * uv[1] + uv[2] * uv[2]);
    uv[0] *= inv; uv[1] *= inv; uv[2] *= inv;
    vv[0] = nv[1] * uv[2] - nv[2] * uv[1];
    vv[1] = nv[2] * uv[0] - nv[0] * uv[2];
    vv[2] = nv[0] * uv[1] - nv[1] * uv[0];
  }

  double G[6][6], g[6];                            // upper triangle of the normal equations and their right-hand side
#pragma unroll
  for (int p = 0; p < 6; ++p) {
    g[p] = 0.0;
#pragma unroll
    for (int q = 0; q < 6; ++q) G[p][q] = 0.0;
  }
  for (int dx = -a.R; dx <= a.R; ++dx)
    for (int dy = -a.R; dy <= a.R; ++dy) {
      const int zr = s_zr[(dx + a.R) * side + dy + a.R];
      if (zr < 0) continue;
      nrm_field<unsigned long long, false>(a, b, X, Y, Z, dx, dy, zr, [&](unsigned long long f, int base, int) {
        while (f) {
          const int dz = __ffsll((long long)f) - 1 + base;
          f &= f - 1;
          const double x = dx * uv[0] + dy * uv[1] + dz * uv[2];
          const double y = dx * vv[0] + dy * vv[1] + dz * vv[2];
          const double z = dx * nv[0] + dy * nv[1] + dz * nv[2];
          const double phi[6] = {x * x, x * y, y * y, x, y, 1.0};
#pragma unroll
          for (int p = 0; p < 6; ++p) {
            g[p] += phi[p] * z;
#pragma unroll
            for (int q = p; q < 6; ++q) G[p][q] += phi[p] * phi[q];
          }
        }
      });
    }

  // Cholesky G = L L^T in place (L^T kept in the upper triangle), a pivot <= 1e-12 x the largest diagonal entry: 0
  double dmax = G[0][0];
#pragma unroll
  for (int p = 1; p < 6; ++p) dmax = fmax(dmax, G[p][p]);
  bool ok = true;
#pragma unroll
  for (int p = 0; p < 6; ++p) {
    double d = G[p][p];
#pragma unroll
    for (int k = 0; k < p; ++k) d -= G[k][p] * G[k][p];
    if (!(d > PCQM_PIVOT_REL * dmax)) { ok = false; d = 1.0; }
    const double l = sqrt(d), il = 1.0 / l;
    G[p][p] = l;
#pragma unroll
    for (int q = p + 1; q < 6; ++q) {
      double s = G[p][q];
#pragma unroll
      for (int k = 0; k < p; ++k) s -= G[k][p] * G[k][q];
      G[p][q] = s * il;
    }
  }
  if (!ok) { out[i] = 0.0; return; }
  double c[6];
#pragma unroll
  for (int p = 0; p < 6; ++p) {                    // L w = g
    double s = g[p];
#pragma unroll
    for (int k = 0; k < p; ++k) s -= G[k][p] * c[k];
    c[p] = s / G[p][p];
  }
#pragma unroll
  for (int p = 5; p >= 0; --p) {                   // L^T c = w
    double s = c[p];
#pragma unroll
    for (int k = p + 1; k < 6; ++k) s -= G[p][k] * c[k];
    c[p] = s / G[p][p];
  }
  const double fa = c[0], fb = c[1], fc = c[2], fd = c[3], fe = c[4];
  const double w = 1.0 + fd * fd + fe * fe;
  out[i] = fabs(((1.0 + fe * fe) * fa - fd * fe * fb + (1.0 + fd * fd) * fc) / (w * sqrt(w)));
}

__global__ void __launch_bounds__(256) k_pcqm_features(NrmArgs a, double inv_two_sigma2, const double* __restrict__ table,
                                                       double* __restrict__ out) {
  __shared__ signed char s_zr[PCQM_SIDE * PCQM_SIDE];
  __shared__ double s_w[PCQM_MAX_LIM + 1];       // Gaussian weight of |d|^2
  pcqm_fill_half_heights(s_zr, a.lim, a.R);
  for (int i = threadIdx.x; i <= a.lim; i += blockDim.x) s_w[i] = exp(-(double)i * inv_two_sigma2);
  __syncthreads();
  const int lane = threadIdx.x & (PCC_WAVE - 1);
  const long long i = (long long)blockIdx.x * (blockDim.x / PCC_WAVE) + threadIdx.x / PCC_WAVE;
  if (i >= a.n) return;                           // (whole waves leave; no barrier follows)
  const long long key = a.keys[i];
  const long long b = key >> PCC_KEY_B_SHIFT;
  const int X = (int)((key >> PCC_KEY_X_SHIFT) & PCC_KEY_FIELD), Y = (int)((key >> PCC_KEY_Y_SHIFT) & PCC_KEY_FIELD), Z = (int)(key & PCC_KEY_FIELD);
  const int side = 2 * a.R + 1;
  const double* own = table + i * PCQM_COLS;
  const double k0 = own[0], l0 = own[2], a0 = own[4], b0 = own[6], c0 = own[8];

  // 0: sum w; curvature 1..5 and lightness 6..10: sum w (xr, xd, xr^2, xd^2, xr xd); a, b, C 11..16: sum w (xr, xd)
  double s[PCQM_NSUM];
#pragma unroll
  for (int k = 0; k < PCQM_NSUM; ++k) s[k] = 0.0;
  for (int col = lane; col < side * side; col += PCC_WAVE) {
    const int zr = s_zr[col];
    if (zr < 0) continue;
    const int dx = col / side - a.R, dy = col % side - a.R;
    nrm_field<unsigned long long, true>(a, b, X, Y, Z, dx, dy, zr, [&](unsigned long long f, int base, int row) {
      const int d2xy = dx * dx + dy * dy;
      while (f) {
        const int dz = __ffsll((long long)f) - 1 + base;
        f &= f - 1;
        const double w = s_w[d2xy + dz * dz];
        const double* t = table + (long long)row * PCQM_COLS;
        ++row;
        const double kr = t[0] - k0, kd = t[1] - k0, lr = t[2] - l0, ld = t[3] - l0;
        s[0] += w;
        s[1] += w * kr; s[2] += w * kd; s[3] += w * kr * kr; s[4] += w * kd * kd; s[5] += w * kr * kd;
        s[6] += w * lr; s[7] += w * ld; s[8] += w * lr * lr; s[9] += w * ld * ld; s[10] += w * lr * ld;
        s[11] += w * (t[4] - a0); s[12] += w * (t[5] - a0);
        s[13] += w * (t[6] - b0); s[14] += w * (t[7] - b0);
        s[15] += w * (t[8] - c0); s[16] += w * (t[9] - c0);
      }
    });
  }
#pragma unroll
  for (int k = 0; k < PCQM_NSUM; ++k)
#pragma unroll
    for (int m = 1; m < PCC_WAVE; m <<= 1) s[k] += __shfl_xor(s[k], m, PCC_WAVE);
  if (lane != 0) return;

  const double iw = 1.0 / s[0];                    // (the centre is a member: s[0] >= 1)
  double mr[5], md[5];                             // shifted means of curvature, lightness, a, b, C
  mr[0] = s[1] * iw; md[0] = s[2] * iw; mr[1] = s[6] * iw; md[1] = s[7] * iw;
#pragma unroll
  for (int k = 0; k < 3; ++k) { mr[2 + k] = s[11 + 2 * k] * iw; md[2 + k] = s[12 + 2 * k] * iw; }
  const double kvr = fmax(s[3] * iw - mr[0] * mr[0], 0.0), kvd = fmax(s[4] * iw - md[0] * md[0], 0.0);
  const double kcov = s[5] * iw - mr[0] * md[0];
  const double lvr = fmax(s[8] * iw - mr[1] * mr[1], 0.0), lvd = fmax(s[9] * iw - md[1] * md[1], 0.0);
  const double lcov = s[10] * iw - mr[1] * md[1];
  const double ksr = sqrt(kvr), ksd = sqrt(kvd), lsr = sqrt(lvr), lsd = sqrt(lvd);
  const double kmr = k0 + mr[0], kmd = k0 + md[0];
  double* o = out + i * 8;
  o[0] = fabs(kmr - kmd) / (fmax(kmr, kmd) + PCQM_K);
  o[1] = fabs(ksr - ksd) / (fmax(ksr, ksd) + PCQM_K);
  o[2] = fabs(ksr * ksd - kcov) / (ksr * ksd + PCQM_K);
  const double dl = mr[1] - md[1];
  o[3] = 1.0 - 1.0 / (PCQM_C1 * dl * dl + 1.0);
  o[4] = 1.0 - (2.0 * lsr * lsd + PCQM_C2) / (lsr * lsr + lsd * lsd + PCQM_C2);
  o[5] = 1.0 - (lcov + PCQM_C3) / (lsr * lsd + PCQM_C3);
  const double da = mr[2] - md[2], db = mr[3] - md[3], dc = mr[4] - md[4];
  o[6] = 1.0 - 1.0 / (PCQM_C4 * dc * dc + 1.0);
  const double dh2 = fmax(da * da + db * db - dc * dc, 0.0);
  o[7] = 1.0 - 1.0 / (PCQM_C5 * dh2 + 1.0);
}

static int pcqm_args(NrmArgs& a, const char* who, const int64_t* keys, int64_t n, const uint64_t* grid_bits,
                     const int32_t* grid_rank, const int32_t* h_grid, int32_t lim, bool rows) {
  PCC_REQUIRE(lim >= 0 && lim <= PCQM_MAX_LIM, "%s: lim %d outside 0 .. %d (radius above 17)", who, lim, PCQM_MAX_LIM);
  PCC_REQUIRE(n >= 0 && n < (1ll << 31), "%s: too many rows", who);
  PCC_REQUIRE(n == 0 || keys, "%s: NULL array", who);
  PCC_REQUIRE(!(rows && grid_bits && !grid_rank), "%s: a grid needs its rank array", who);
  return nrm_fill_args(a, who, keys, n, grid_bits, grid_rank, h_grid, lim);
}

extern "C" int pcc_curvature_grid(const int64_t* keys, int64_t n, const uint64_t* grid_bits, const int32_t* grid_rank,
                                  const int32_t* h_grid, int32_t lim, double* out, void* stream) {
  NrmArgs a;
  PCC_TRY(pcqm_args(a, "pcc_curvature_grid", keys, n, grid_bits, grid_rank, h_grid, lim, false));
  if (n == 0) return PCC_OK;
  PCC_REQUIRE(out, "pcc_curvature_grid: NULL array");
  k_curvature<<<(unsigned)pcc_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(a, out);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_pcqm_features(const int64_t* keys, int64_t n, const uint64_t* grid_bits, const int32_t* grid_rank,
                                 const int32_t* h_grid, int32_t lim, double inv_two_sigma2, const double* table, double* out,
                                 void* stream) {
  NrmArgs a;
  PCC_TRY(pcqm_args(a, "pcc_pcqm_features", keys, n, grid_bits, grid_rank, h_grid, lim, true));
  PCC_REQUIRE(inv_two_sigma2 >= 0.0 && inv_two_sigma2 < 1e300, "pcc_pcqm_features: inv_two_sigma2 %g", inv_two_sigma2);
  if (n == 0) return PCC_OK;
  PCC_REQUIRE(table && out, "pcc_pcqm_features: NULL array");
  k_pcqm_features<<<(unsigned)pcc_cdiv(n, 256 / PCC_WAVE), 256, 0, (hipStream_t)stream>>>(a, inv_two_sigma2, table, out);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}
