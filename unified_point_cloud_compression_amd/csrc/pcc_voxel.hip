// Voxel-grid down-sampling with averaged attributes (reference data/utils/RawLoader.py:48-57: Open3D's voxel_down_sample):
// a key per point, then -- after the stable key sort and the run starts that coordinate sets use -- one reduction over the
// runs of equal keys.  Every sum is fp64 in an order that depends on (n, run layout) only; there are no floating-point
// atomics, so equal inputs give equal bits on every run.
#include "pcc_common.h"

#include <math.h>

static constexpr int VOX_T = 256;                           // threads per workgroup
static constexpr int VOX_G = 4;                             // lanes that share a short run
static constexpr int VOX_WAVE_RUNS = PCC_WAVE / VOX_G;      // runs a wave holds
static constexpr int VOX_WG_RUNS = VOX_T / VOX_G;           // runs a workgroup holds
static constexpr int VOX_TILE = PCC_VOXEL_TILE_ROWS;        // sorted rows per workgroup of the split pass
static constexpr int VOX_MAXCH = 3 + PCC_VOXEL_MAX_ATTRS;   // xyz + attributes
// A run that is split is longer than a tile, so it cannot lie inside one: a tile meets at most two split runs, the one that
// holds its first row and the one that holds its last.
static_assert(PCC_VOXEL_SPLIT_RUN > VOX_TILE && PCC_VOXEL_WAVE_RUN <= PCC_VOXEL_SPLIT_RUN, "thresholds");
static_assert(VOX_TILE % VOX_T == 0, "whole rounds");

// ------------------------------------------------------------------------------------------
// keys
// ------------------------------------------------------------------------------------------
// idx = floor(((double)p - origin) / voxel) per axis: the subtraction and the division are single correctly rounded fp64
// operations (hipcc's default for `/`; nothing here can contract), so numpy's float64 gives the same integer.
__global__ void __launch_bounds__(256) k_voxel_keys(const float* __restrict__ pts, long long n, double ox, double oy, double oz,
                                                    double voxel, long long* __restrict__ keys, int* __restrict__ bad) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double o[3] = {ox, oy, oz};
  long long k = 0;
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double q = floor(((double)pts[i * 3 + a] - o[a]) / voxel);
    const bool in = q >= -(double)PCC_BIAS && q < (double)PCC_BIAS;      // (NaN and the infinities fail)
    ok = ok && in;
    k = (k << 16) | (long long)((in ? (int)q : 0) + (int)PCC_BIAS);
  }
  keys[i] = k;
  if (!ok) *bad = 1;       // benign race: every writer stores 1
}

extern "C" int pcc_voxel_keys(const float* points, int64_t n, double ox, double oy, double oz, double voxel_size, int64_t* keys,
                              int32_t* d_bad, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PCC_REQUIRE(d_bad, "pcc_voxel_keys: d_bad is NULL");
  PCC_REQUIRE(n >= 0 && n < (1ll << 31), "pcc_voxel_keys: n = %lld outside 0..2^31-1", (long long)n);
  PCC_REQUIRE(isfinite(voxel_size) && voxel_size > 0.0, "pcc_voxel_keys: voxel size %g is not finite and positive", voxel_size);
  PCC_REQUIRE(isfinite(ox) && isfinite(oy) && isfinite(oz), "pcc_voxel_keys: origin is not finite");
  PCC_REQUIRE(n == 0 || (points && keys), "pcc_voxel_keys: NULL array");
  PCC_CHECK_HIP(hipMemsetAsync(d_bad, 0, sizeof(int32_t), s));
  if (n == 0) return PCC_OK;
  k_voxel_keys<<<(unsigned)pcc_cdiv(n, 256), 256, 0, s>>>(points, n, ox, oy, oz, voxel_size, (long long*)keys, d_bad);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

// ------------------------------------------------------------------------------------------
// means per run
// ------------------------------------------------------------------------------------------
struct VoxArgs {
  const float* pts;          // [n,3]
  const float* attrs;        // [n,c] or nullptr (c == 0)
  const int* perm;           // [n] sorted position -> input row
  const long long* ukeys;    // [m]
  const int* first;          // [m] first sorted position of every run, ascending from 0
  const long long* d_count;  // m, on the device
  int n, c;
  double* partials;          // [tiles][2][3 + c]
  int* index;                // [n,3]
  int* counts;               // [n]
  float* mean_pts;           // [n,3]
  float* mean_attrs;         // [n,c]
};

__device__ __forceinline__ int vox_runs(const VoxArgs& A) {
  const long long m = *A.d_count;
  return (int)(m < 0 ? 0 : (m > A.n ? A.n : m));
}

// rows [a, b) of run r in the sorted order; an array that is no list of run starts gives an empty range, never one
// outside [0, n)
__device__ __forceinline__ void vox_range(const VoxArgs& A, int r, int m, int& a, int& b) {
  a = A.first[r];
  b = r + 1 < m ? A.first[r + 1] : A.n;
  if (a < 0 || b > A.n || b < a) a = b = 0;
}

// one sorted row added to the NCH accumulators (channels 0..2 the point, 3.. the attributes)
template <int NCH>
__device__ __forceinline__ void vox_add(const VoxArgs& A, int row, double (&acc)[NCH]) {
  const long long j = A.perm[row];
  if (j < 0 || j >= A.n) return;                  // a permutation never does this; a foreign array cannot read outside
  const float* p = A.pts + j * 3;
  acc[0] += (double)p[0]; acc[1] += (double)p[1]; acc[2] += (double)p[2];
  if (NCH > 3) {
    const float* q = A.attrs + j * A.c;
#pragma unroll
    for (int k = 3; k < NCH; ++k)
      if (k - 3 < A.c) acc[k] += (double)q[k - 3];
  }
}

// fixed butterfly over the WIDTH lanes of a group: every lane ends with the same sum, added in the same order on every run
template <int NCH, int WIDTH>
__device__ __forceinline__ void vox_butterfly(double (&acc)[NCH]) {
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
#pragma unroll
    for (int d = WIDTH / 2; d >= 1; d >>= 1) acc[k] += __shfl_xor(acc[k], d);
  }
}

template <int NCH>
__device__ __forceinline__ void vox_write(const VoxArgs& A, int r, int count, const double (&acc)[NCH]) {
  const long long key = A.ukeys[r];
  A.index[r * 3LL + 0] = pcc_key_x(key);
  A.index[r * 3LL + 1] = pcc_key_y(key);
  A.index[r * 3LL + 2] = pcc_key_z(key);
  A.counts[r] = count;
  const double cnt = (double)count;
#pragma unroll
  for (int k = 0; k < 3; ++k) A.mean_pts[r * 3LL + k] = (float)(acc[k] / cnt);     // one fp64 division, rounded once to fp32
#pragma unroll
  for (int k = 3; k < NCH; ++k)
    if (k - 3 < A.c) A.mean_attrs[(long long)r * A.c + (k - 3)] = (float)(acc[k] / cnt);
}

// largest r in [0, m) with first[r] <= row (first[0] == 0)
__device__ __forceinline__ int vox_run_of(const int* __restrict__ first, int m, int row) {
  int lo = 0, hi = m;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first[mid] <= row) lo = mid; else hi = mid;
  }
  return lo;
}

// Split pass: workgroup t owns sorted rows [t * TILE, (t + 1) * TILE).  Of the run that holds its first row (piece 0) and
// of the run that holds its last row, when that is another one (piece 1), it sums the rows inside the tile -- when the run
// is long enough to be split -- and stores the sums at partials[t][piece][channel]: thread i takes rows i, i + 256, ... of the
// piece, lanes of a wave by butterfly, the four waves in order.  A tile without a split run costs two binary searches.
template <int NCH>
__global__ void __launch_bounds__(VOX_T) k_voxel_partials(const VoxArgs A) {
  __shared__ int s_piece[2][2];
  __shared__ double s_w[VOX_T / PCC_WAVE][NCH];
  const int nch = 3 + A.c;
  const int r0 = blockIdx.x * VOX_TILE;
  const int r1 = min(r0 + VOX_TILE, A.n);               // r0 < n by the grid's size; n + TILE fits an int (checked on the host)
  if (threadIdx.x == 0) {
    const int m = vox_runs(A);
    int lo[2] = {0, 0}, hi[2] = {0, 0};
    if (m > 0) {
      const int ra = vox_run_of(A.first, m, r0), rb = vox_run_of(A.first, m, r1 - 1);
      int a, b;
      vox_range(A, ra, m, a, b);
      if (b - a >= PCC_VOXEL_SPLIT_RUN) { lo[0] = max(a, r0); hi[0] = min(b, r1); }
      if (rb != ra) {
        vox_range(A, rb, m, a, b);
        if (b - a >= PCC_VOXEL_SPLIT_RUN) { lo[1] = max(a, r0); hi[1] = min(b, r1); }
      }
    }
    s_piece[0][0] = lo[0]; s_piece[0][1] = hi[0]; s_piece[1][0] = lo[1]; s_piece[1][1] = hi[1];
  }
  __syncthreads();
  for (int piece = 0; piece < 2; ++piece) {              // uniform over the workgroup
    const int lo = s_piece[piece][0], hi = s_piece[piece][1];
    if (hi <= lo) continue;
    double acc[NCH];
#pragma unroll
    for (int k = 0; k < NCH; ++k) acc[k] = 0.0;
    for (int row = lo + (int)threadIdx.x; row < hi; row += VOX_T) vox_add<NCH>(A, row, acc);
    vox_butterfly<NCH, PCC_WAVE>(acc);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int k = 0; k < NCH; ++k) s_w[threadIdx.x >> 6][k] = acc[k];
    }
    __syncthreads();
    if ((int)threadIdx.x < nch) {
      const int k = threadIdx.x;
      A.partials[((long long)blockIdx.x * 2 + piece) * nch + k] = ((s_w[0][k] + s_w[1][k]) + s_w[2][k]) + s_w[3][k];
    }
    __syncthreads();
  }
}

// Means: a wave holds 16 consecutive runs, four lanes each.
//   short run  (< WAVE_RUN rows)   its four lanes stride the rows, butterfly over the four;
//   longer run (< SPLIT_RUN rows)  the whole wave strides the rows, butterfly over the 64 lanes;
//   split run                      the wave's lanes stride the tiles of the run and add the split pass's partials, butterfly.
// The longer runs of a wave are taken one after the other, in run order.
template <int NCH>
__global__ void __launch_bounds__(VOX_T) k_voxel_means(const VoxArgs A) {
  const int m = vox_runs(A);
  const int lane = threadIdx.x & 63, g = lane / VOX_G, q = lane % VOX_G;
  const int wave_first = blockIdx.x * VOX_WG_RUNS + (threadIdx.x >> 6) * VOX_WAVE_RUNS;
  if (wave_first >= m) return;                           // uniform over the wave
  const int r = wave_first + g;
  int a = 0, b = 0;
  if (r < m) vox_range(A, r, m, a, b);
  const int len = b - a;
  double acc[NCH];
#pragma unroll
  for (int k = 0; k < NCH; ++k) acc[k] = 0.0;
  if (r < m && len < PCC_VOXEL_WAVE_RUN)
    for (int row = a + q; row < b; row += VOX_G) vox_add<NCH>(A, row, acc);
  vox_butterfly<NCH, VOX_G>(acc);
  if (r < m && len < PCC_VOXEL_WAVE_RUN && q == 0) vox_write<NCH>(A, r, len, acc);

  unsigned long long todo = __ballot(r < m && q == 0 && len >= PCC_VOXEL_WAVE_RUN);
  const int nch = 3 + A.c;
  while (todo) {                                         // uniform over the wave
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int ra = __shfl(a, src), rb = __shfl(b, src), rr = wave_first + src / VOX_G;
#pragma unroll
    for (int k = 0; k < NCH; ++k) acc[k] = 0.0;
    if (rb - ra < PCC_VOXEL_SPLIT_RUN) {
      for (int row = ra + lane; row < rb; row += PCC_WAVE) vox_add<NCH>(A, row, acc);
    } else {
      const int t0 = ra / VOX_TILE, t1 = (rb - 1) / VOX_TILE;
      for (int t = t0 + lane; t <= t1; t += PCC_WAVE) {
        const int piece = (long long)t * VOX_TILE >= ra ? 0 : 1;      // the run holds the tile's first row, or only its last
        const double* p = A.partials + ((long long)t * 2 + piece) * nch;
#pragma unroll
        for (int k = 0; k < NCH; ++k)
          if (k < nch) acc[k] += p[k];
      }
    }
    vox_butterfly<NCH, PCC_WAVE>(acc);
    if (lane == 0) vox_write<NCH>(A, rr, rb - ra, acc);
  }
}

extern "C" size_t pcc_voxel_means_ws_bytes(int64_t n, int32_t c) {
  if (n <= 0 || c < 0 || c > PCC_VOXEL_MAX_ATTRS) return 256;
  return pcc_align_up((size_t)pcc_cdiv(n, VOX_TILE) * 2 * (size_t)(3 + c) * sizeof(double));
}

template <int NCH>
static int voxel_means_launch(const VoxArgs& A, hipStream_t s) {
  k_voxel_partials<NCH><<<(unsigned)pcc_cdiv(A.n, VOX_TILE), VOX_T, 0, s>>>(A);
  PCC_LAUNCH_CHECK();
  k_voxel_means<NCH><<<(unsigned)pcc_cdiv(A.n, VOX_WG_RUNS), VOX_T, 0, s>>>(A);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_voxel_means(const float* points, const float* attrs, int32_t c, int64_t n, const int32_t* perm,
                               const int64_t* uniq_keys, const int32_t* first, const int64_t* d_count, int32_t* index,
                               int32_t* counts, float* mean_points, float* mean_attrs, void* ws, size_t ws_bytes, void* stream) {
  PCC_REQUIRE(n >= 0 && n < (1ll << 31) - 2 * VOX_TILE, "pcc_voxel_means: n = %lld outside 0..2^31-2049", (long long)n);
  PCC_REQUIRE(c >= 0 && c <= PCC_VOXEL_MAX_ATTRS, "pcc_voxel_means: %d attribute columns outside 0..%d", c, PCC_VOXEL_MAX_ATTRS);
  PCC_REQUIRE(index && counts && mean_points && (c == 0 || mean_attrs), "pcc_voxel_means: NULL output");
  PCC_REQUIRE(c == 0 || attrs, "pcc_voxel_means: %d attribute columns but no attribute matrix", c);
  if (n == 0) return PCC_OK;
  PCC_REQUIRE(points && perm && uniq_keys && first && d_count, "pcc_voxel_means: NULL input");
  if (!ws || ws_bytes < pcc_voxel_means_ws_bytes(n, c)) {
    pcc_set_error("pcc_voxel_means: workspace of %zu bytes, %zu needed", ws_bytes, pcc_voxel_means_ws_bytes(n, c));
    return PCC_EWS;
  }
  VoxArgs A;
  A.pts = points; A.attrs = attrs; A.perm = perm; A.ukeys = (const long long*)uniq_keys; A.first = first;
  A.d_count = (const long long*)d_count; A.n = (int)n; A.c = c; A.partials = (double*)ws;
  A.index = index; A.counts = counts; A.mean_pts = mean_points; A.mean_attrs = mean_attrs;
  hipStream_t s = (hipStream_t)stream;
  // accumulators live in registers, so the channel count is a compile-time bound: the smallest of four that holds 3 + c
  if (c == 0) return voxel_means_launch<3>(A, s);
  if (c <= 3) return voxel_means_launch<6>(A, s);
  if (c <= 9) return voxel_means_launch<12>(A, s);
  return voxel_means_launch<VOX_MAXCH>(A, s);
}
