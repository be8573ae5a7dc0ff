// Global motion compensation of the inter-frame coders (motion.py; DESIGN.md section 7e "Global motion").
//
// k_motion_warp: the integer warp every side of a stream repeats.  One thread per key of a pitch-1 key array: the voxel p goes
// to q_i = (sum_j M_ij p_j + (t_i << 16) + 2^23) >> 24 in int64 (M in Q24, t in Q8 voxels, the shift floors), and the key of q
// is written to the thread's own row -- PCC_MOTION_DROPPED when a coordinate of q leaves the range a coordinate set may hold.
// Which source wins a cell that several land in is not decided here: the caller sorts the rows stably with their input index
// as payload (pcc_sort_keys) and takes the first row of every run (pcc_unique_sorted), the source of lowest input rank.
// k_motion_gather carries up to PCC_MOTION_MAX_ATTRS uint8 columns of the winners.
//
// k_motion_icp_terms: the normal-equation terms of one point-to-plane ICP iteration.  One thread per reference voxel p in the
// order of the array; x = R p + t in fp64; the candidates are the current frame's voxels c in the cube |c_k - round(x_k)| <=
// ceil(radius) with |c - x|^2 < radius^2, found column by column as bit fields of the current frame's occupancy bitmap (or by
// binary search over its keys: the same fields, pcc_normals.h), visited dx, dy, dz ascending -- canonical order, so a strict
// comparison leaves the lowest rank on a tie.  A thread's 29 terms meet in an xor butterfly per wave, the four waves of a
// workgroup are added in wave order, and k_motion_icp_reduce adds the workgroups' partials in workgroup order: no floating-
// point atomics, the sums depend on the inputs alone.  Contraction is off in this file: every product and sum below rounds on
// its own, so a float64 restatement that follows the same order of operations matches term for term.
#include <limits.h>

#include "pcc_normals.h"

#pragma clang fp contract(off)

static constexpr int MOT_T = 256;
static constexpr int MOT_WAVES = MOT_T / PCC_WAVE;
static constexpr int MOT_NSUM = PCC_MOTION_ICP_SUMS;
static constexpr int MOT_LO = -(int)PCC_BIAS + 64, MOT_HI = (int)PCC_BIAS - 64;      // a set holds coordinates in [MOT_LO, MOT_HI)
static constexpr int MOT_MAX_CR = 4;                                                 // ceil(radius) <= 4: a column is a 9-bit field

struct MotionT { int M[9]; int t[3]; };

__global__ void __launch_bounds__(MOT_T) k_motion_warp(const long long* __restrict__ keys, long long n, MotionT T,
                                                       long long* __restrict__ out, int* __restrict__ info) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN}, dropped = 0;
  if (i < n) {
    const long long key = keys[i];
    const long long p[3] = {pcc_key_x(key), pcc_key_y(key), pcc_key_z(key)};
    int q[3];
    bool keep = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const long long v = ((long long)T.M[3 * k] * p[0] + (long long)T.M[3 * k + 1] * p[1] + (long long)T.M[3 * k + 2] * p[2] +
                           (long long)T.t[k] * 65536 + (1ll << 23)) >> 24;
      keep = keep && v >= MOT_LO && v < MOT_HI;
      q[k] = (int)v;
    }
    if (keep) {
      out[i] = pcc_key_pack(pcc_key_b(key), q[0], q[1], q[2]);
#pragma unroll
      for (int k = 0; k < 3; ++k) lo[k] = hi[k] = q[k];
    } else {
      out[i] = PCC_MOTION_DROPPED;
      dropped = 1;
    }
  }
  // bounds of the kept rows and the number of dropped ones: integer min / max / add, a wave at a time
#pragma unroll
  for (int m = 1; m < PCC_WAVE; m <<= 1) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      lo[k] = min(lo[k], __shfl_xor(lo[k], m, PCC_WAVE));
      hi[k] = max(hi[k], __shfl_xor(hi[k], m, PCC_WAVE));
    }
    dropped += __shfl_xor(dropped, m, PCC_WAVE);
  }
  if ((threadIdx.x & (PCC_WAVE - 1)) == 0) {
    if (lo[0] != INT_MAX) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        atomicMin(info + k, lo[k]);
        atomicMax(info + 3 + k, hi[k]);
      }
    }
    if (dropped) atomicAdd(info + 6, dropped);
  }
}

__global__ void __launch_bounds__(MOT_T) k_motion_gather(const unsigned char* __restrict__ attrs, int c, long long n_src,
                                                         const int* __restrict__ perm, const int* __restrict__ first, long long n_out,
                                                         unsigned char* __restrict__ out) {
  const long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n_out) return;
  // (indices are clamped into the arrays: with what pcc_sort_keys / pcc_unique_sorted left, the clamps never act)
  const long long f = min(max((long long)first[u], 0ll), n_src - 1);
  const long long row = min(max((long long)perm[f], 0ll), n_src - 1);
  for (int k = 0; k < c; ++k) out[u * c + k] = attrs[row * c + k];
}

struct IcpArgs {
  NrmArgs cur;                                   // the current frame: keys, rows, grid index (R = ceil(radius))
  const long long* ref; int n_ref;
  const float* normals;                          // [cur.n, 3]
  double R[9], t[3], g[3], r2;
};

__global__ void __launch_bounds__(MOT_T) k_motion_icp_terms(IcpArgs a, double* __restrict__ partial, int* __restrict__ match) {
  __shared__ double s_w[MOT_WAVES][MOT_NSUM];
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  double s[MOT_NSUM];
#pragma unroll
  for (int k = 0; k < MOT_NSUM; ++k) s[k] = 0.0;
  if (i < a.n_ref) {
    const long long key = a.ref[i];
    const double p0 = (double)pcc_key_x(key), p1 = (double)pcc_key_y(key), p2 = (double)pcc_key_z(key);
    double x[3], r[3];
    bool inside = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      x[k] = ((a.R[3 * k] * p0 + a.R[3 * k + 1] * p1) + a.R[3 * k + 2] * p2) + a.t[k];
      r[k] = floor(x[k] + 0.5);
      // the current frame lies in [MOT_LO, MOT_HI): a cube further out than that holds no candidate
      inside = inside && r[k] >= (double)(MOT_LO - 2 * MOT_MAX_CR) && r[k] < (double)(MOT_HI + 2 * MOT_MAX_CR);
    }
    int best_row = -1;
    double best = a.r2, e[3] = {0.0, 0.0, 0.0};
    if (inside) {
      const int cr = a.cur.R;
      const int X = (int)r[0] + (int)PCC_BIAS, Y = (int)r[1] + (int)PCC_BIAS, Z = (int)r[2] + (int)PCC_BIAS;
      for (int dx = -cr; dx <= cr; ++dx)
        for (int dy = -cr; dy <= cr; ++dy)
          nrm_field<unsigned, true>(a.cur, 0, X, Y, Z, dx, dy, cr, [&](unsigned f, int base, int row) {
            const double e0 = (r[0] + (double)dx) - x[0], e1 = (r[1] + (double)dy) - x[1];
            const double d01 = e0 * e0 + e1 * e1;
            while (f) {
              const int dz = __ffs((int)f) - 1 + base;
              f &= f - 1;
              const double e2 = (r[2] + (double)dz) - x[2];
              const double d2 = d01 + e2 * e2;
              if (d2 < best) { best = d2; best_row = row; e[0] = e0; e[1] = e1; e[2] = e2; }    // (strict: the lowest rank on a tie)
              ++row;
            }
          });
    }
    if (match) match[i] = best_row;
    if (best_row >= 0) {
      const float* nf = a.normals + 3ll * best_row;
      const double n0 = (double)nf[0], n1 = (double)nf[1], n2 = (double)nf[2];
      const double u0 = x[0] - a.g[0], u1 = x[1] - a.g[1], u2 = x[2] - a.g[2];
      const double av[6] = {u1 * n2 - u2 * n1, u2 * n0 - u0 * n2, u0 * n1 - u1 * n0, n0, n1, n2};
      const double b = (e[0] * n0 + e[1] * n1) + e[2] * n2;
      int at = 0;
#pragma unroll
      for (int p = 0; p < 6; ++p)
#pragma unroll
        for (int q = p; q < 6; ++q) s[at++] = av[p] * av[q];
#pragma unroll
      for (int p = 0; p < 6; ++p) s[21 + p] = av[p] * b;
      s[27] = 1.0;
      s[28] = best;
    }
  }
#pragma unroll
  for (int k = 0; k < MOT_NSUM; ++k)
#pragma unroll
    for (int m = 1; m < PCC_WAVE; m <<= 1) s[k] += __shfl_xor(s[k], m, PCC_WAVE);
  const int lane = threadIdx.x & (PCC_WAVE - 1), w = threadIdx.x / PCC_WAVE;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < MOT_NSUM; ++k) s_w[w][k] = s[k];
  }
  __syncthreads();
  if (threadIdx.x < MOT_NSUM) {
    double v = s_w[0][threadIdx.x];
    for (int j = 1; j < MOT_WAVES; ++j) v += s_w[j][threadIdx.x];
    partial[(long long)blockIdx.x * MOT_NSUM + threadIdx.x] = v;
  }
}

__global__ void __launch_bounds__(PCC_WAVE) k_motion_icp_reduce(const double* __restrict__ partial, int blocks, double* __restrict__ out) {
  if (threadIdx.x >= MOT_NSUM) return;
  double v = 0.0;
  for (int j = 0; j < blocks; ++j) v += partial[(long long)j * MOT_NSUM + threadIdx.x];
  out[threadIdx.x] = v;
}

extern "C" int pcc_motion_warp(const int64_t* keys, int64_t n, const int32_t* h_transform, int64_t* out_keys, int32_t* d_info,
                               void* stream) {
  PCC_REQUIRE(n >= 0 && n < (1ll << 31), "pcc_motion_warp: too many rows");
  PCC_REQUIRE(h_transform, "pcc_motion_warp: the transform is 12 host integers");
  MotionT T;
  for (int k = 0; k < 9; ++k) {
    PCC_REQUIRE(h_transform[k] >= -PCC_MOTION_MAX_M && h_transform[k] <= PCC_MOTION_MAX_M,
                "pcc_motion_warp: matrix entry %d is %d, outside +-2^25 (Q24)", k, h_transform[k]);
    T.M[k] = h_transform[k];
  }
  for (int k = 0; k < 3; ++k) {
    PCC_REQUIRE(h_transform[9 + k] > -PCC_MOTION_MAX_T && h_transform[9 + k] < PCC_MOTION_MAX_T,
                "pcc_motion_warp: translation entry %d is %d, outside +-2^24 (Q8)", k, h_transform[9 + k]);
    T.t[k] = h_transform[9 + k];
  }
  if (n == 0) return PCC_OK;
  PCC_REQUIRE(keys && out_keys && d_info && keys != out_keys, "pcc_motion_warp: NULL or aliased array");
  k_motion_warp<<<(unsigned)pcc_cdiv(n, MOT_T), MOT_T, 0, (hipStream_t)stream>>>((const long long*)keys, n, T, (long long*)out_keys, d_info);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_motion_gather(const uint8_t* attrs, int32_t c, int64_t n_src, const int32_t* perm, const int32_t* first, int64_t n_out,
                                 uint8_t* out, void* stream) {
  PCC_REQUIRE(c >= 1 && c <= PCC_MOTION_MAX_ATTRS, "pcc_motion_gather: %d attribute columns, 1 .. %d are carried", c, PCC_MOTION_MAX_ATTRS);
  PCC_REQUIRE(n_src >= 0 && n_src < (1ll << 31) && n_out >= 0 && n_out <= n_src, "pcc_motion_gather: %lld winners of %lld rows",
              (long long)n_out, (long long)n_src);
  if (n_out == 0) return PCC_OK;
  PCC_REQUIRE(attrs && perm && first && out, "pcc_motion_gather: NULL array");
  k_motion_gather<<<(unsigned)pcc_cdiv(n_out, MOT_T), MOT_T, 0, (hipStream_t)stream>>>(attrs, c, n_src, perm, first, n_out, out);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" size_t pcc_motion_icp_ws_bytes(int64_t n_ref) {
  return pcc_align_up((size_t)pcc_cdiv(n_ref > 0 ? n_ref : 1, MOT_T) * MOT_NSUM * sizeof(double)) + 256;
}

extern "C" int pcc_motion_icp_terms(const int64_t* ref_keys, int64_t n_ref, const int64_t* cur_keys, int64_t n_cur,
                                    const uint64_t* grid_bits, const int32_t* grid_rank, const int32_t* h_grid, const float* normals,
                                    const double* h_rt, const double* h_centre, double radius, double* out, int32_t* match, void* ws,
                                    size_t ws_bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PCC_REQUIRE(n_ref >= 0 && n_ref < (1ll << 31) && n_cur >= 0 && n_cur < (1ll << 31), "pcc_motion_icp_terms: too many rows");
  PCC_REQUIRE(radius > 0.0 && radius <= (double)MOT_MAX_CR, "pcc_motion_icp_terms: radius %g outside (0, %d]", radius, MOT_MAX_CR);
  PCC_REQUIRE(h_rt && h_centre && out, "pcc_motion_icp_terms: NULL array");
  for (int k = 0; k < 15; ++k) {
    const double v = k < 12 ? h_rt[k] : h_centre[k - 12];
    PCC_REQUIRE(v == v && v > -1e300 && v < 1e300, "pcc_motion_icp_terms: parameter %d is not finite", k);
  }
  PCC_REQUIRE(!(grid_bits && !grid_rank), "pcc_motion_icp_terms: a grid needs its rank array");
  if (n_ref == 0) {
    PCC_CHECK_HIP(hipMemsetAsync(out, 0, MOT_NSUM * sizeof(double), s));
    return PCC_OK;
  }
  PCC_REQUIRE(ref_keys && (n_cur == 0 || (cur_keys && normals)), "pcc_motion_icp_terms: NULL array");
  if (ws_bytes < pcc_motion_icp_ws_bytes(n_ref) || !ws) {
    pcc_set_error("pcc_motion_icp_terms: workspace too small");
    return PCC_EWS;
  }
  IcpArgs a;
  PCC_TRY(nrm_fill_args(a.cur, "pcc_motion_icp_terms", cur_keys, n_cur, n_cur ? grid_bits : nullptr, grid_rank, h_grid, 0));
  a.cur.R = 1;
  while ((double)a.cur.R < radius) ++a.cur.R;    // ceil(radius)
  a.ref = (const long long*)ref_keys; a.n_ref = (int)n_ref; a.normals = normals;
  for (int k = 0; k < 9; ++k) a.R[k] = h_rt[k];
  for (int k = 0; k < 3; ++k) { a.t[k] = h_rt[9 + k]; a.g[k] = h_centre[k]; }
  a.r2 = radius * radius;
  const int blocks = (int)pcc_cdiv(n_ref, MOT_T);
  k_motion_icp_terms<<<(unsigned)blocks, MOT_T, 0, s>>>(a, (double*)ws, match);
  PCC_LAUNCH_CHECK();
  k_motion_icp_reduce<<<1, PCC_WAVE, 0, s>>>((const double*)ws, blocks, out);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}
