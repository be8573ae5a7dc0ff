// Rate sweep of the Gaussian conditional: the rANS payload estimate of y under K candidate gain rows in one launch.
// Per candidate k the result is the integer that pcc_gauss_encode (gain row k) followed by pcc_rans_estimate_bits gives;
// the element rules are the inlined functions of pcc_entropy_rule.h that those two kernels use, and the sums are integers.
// Neither the symbols nor the table rows are written.
#include "pcc_common.h"
#include "pcc_entropy_rule.h"

static constexpr int RATE_THREADS = 1024;   // 16 waves: with at most RATE_BLOCKS workgroups, one per CU, four waves per SIMD
static constexpr int RATE_BLOCKS = 256;     // bounds the same-address adds at the end to RATE_BLOCKS per candidate
static constexpr int RATE_MAX_K = 256;

// A lane owns one element per pass and walks the candidates: y, scale and mean are read once, the gain rows come through
// the cache in coalesced rows (lane <-> channel).  The cost of (element, k) is at most 13 312 (16 bits of payload and nine
// bypass digits), so a wave's sum fits 32 bits; it is reduced across the wave, lane 0 adds it to the workgroup's 64-bit
// accumulator of k in LDS, and the workgroup adds each accumulator to the result once.
__global__ void __launch_bounds__(RATE_THREADS) k_gauss_rate_sweep(const float* __restrict__ y, const float* __restrict__ params,
                                                                   long long total, int c, const float* __restrict__ gains, int K,
                                                                   const float* __restrict__ table, int nt, RansTab t,
                                                                   unsigned long long* __restrict__ bits256) {
  __shared__ float tab[256];
  __shared__ unsigned long long acc[RATE_MAX_K];
  if (threadIdx.x < nt) tab[threadIdx.x] = table[threadIdx.x];
  if (threadIdx.x < K) acc[threadIdx.x] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  for (long long base = (long long)blockIdx.x * RATE_THREADS; base < total; base += (long long)gridDim.x * RATE_THREADS) {
    const long long e = base + threadIdx.x;
    const bool on = e < total;                      // lanes past the end take part in the wave sums with zero
    float yv = 0.f, scale = 0.f, mean = 0.f;
    int ch = 0;
    if (on) {
      const long long r = e / c;
      ch = (int)(e - r * c);
      yv = y[e];
      scale = params[r * 2 * c + ch];
      mean = params[r * 2 * c + c + ch];
    }
    for (int k = 0; k < K; ++k) {
      unsigned b = 0;
      if (on) {
        const float g = gains[(long long)k * c + ch];
        const float s = gauss_bound_scale(scale, g);
        const int ci = table_index(s, tab, nt);
        const float q = gauss_quantise(yv, mean, g);
        b = rans_value_bits256((int)q - t.offsets[ci], t.sizes[ci] - 2, t.cdf + (size_t)ci * t.stride);
      }
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) b += __shfl_xor(b, d, 64);
      if (lane == 0 && b) atomicAdd(&acc[k], (unsigned long long)b);
    }
  }
  __syncthreads();
  if (threadIdx.x < K && acc[threadIdx.x]) atomicAdd(bits256 + threadIdx.x, acc[threadIdx.x]);
}

extern "C" int pcc_gauss_rate_sweep(const float* y, const float* params, int64_t n, int32_t c, const float* gains, int32_t K,
                                    const float* table, int32_t n_table, const int32_t* cdf, int32_t cdf_stride,
                                    const int32_t* sizes, const int32_t* offsets, int64_t* d_bits256, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PCC_REQUIRE(K >= 1 && K <= RATE_MAX_K, "pcc_gauss_rate_sweep: %d candidates (1 to %d)", K, RATE_MAX_K);
  PCC_REQUIRE(c >= 1 && n >= 0 && n_table >= 2 && n_table <= 256, "pcc_gauss_rate_sweep: bad sizes (n %lld, c %d, n_table %d)",
              (long long)n, c, n_table);
  PCC_REQUIRE(n < (1ll << 31) && n * c < (1ll << 31), "pcc_gauss_rate_sweep: n * c must stay below 2^31");
  PCC_REQUIRE(d_bits256, "pcc_gauss_rate_sweep: d_bits256 is NULL");
  PCC_CHECK_HIP(hipMemsetAsync(d_bits256, 0, sizeof(int64_t) * (size_t)K, s));
  if (n == 0) return PCC_OK;
  PCC_REQUIRE(y && params && gains && table && cdf && sizes && offsets && cdf_stride >= 2, "pcc_gauss_rate_sweep: NULL array");
  RansTab t{cdf, cdf_stride, sizes, offsets};
  const long long total = (long long)n * c;
  const long long blocks = pcc_cdiv(total, RATE_THREADS);
  k_gauss_rate_sweep<<<(unsigned)(blocks < RATE_BLOCKS ? blocks : RATE_BLOCKS), RATE_THREADS, 0, s>>>(
      y, params, total, c, gains, K, table, n_table, t, (unsigned long long*)d_bits256);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}
