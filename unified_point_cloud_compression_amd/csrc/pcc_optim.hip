// Multi-tensor optimiser step: gradient clipping by the total norm (torch.nn.utils.clip_grad_norm_) and Adam / SGD with
// momentum (torch.optim.Adam / SGD, default forms) for ALL tensors of an optimiser in two launches over a segment table
// (one row per tensor) and a chunk table (PCC_OPTIM_CHUNK elements of one tensor per workgroup).  Every sum is fp64 in an
// order that depends on the tensors' sizes only; there are no floating-point atomics, so equal inputs give equal bits.
#include "pcc_common.h"

#include <math.h>

static constexpr int OPT_T = 256;                              // threads per workgroup
static constexpr int OPT_CHUNK = PCC_OPTIM_CHUNK;              // elements per workgroup
static constexpr int OPT_GROUPS = OPT_CHUNK / 4;               // groups of four elements in a chunk
static_assert(OPT_GROUPS % OPT_T == 0 && OPT_T == 4 * PCC_WAVE, "whole rounds of four waves");

struct OptSeg {                // one row of the segment table: PCC_OPTIM_SEG_WORDS int64 words
  float* p;
  const float* g;              // nullptr: the tensor has no gradient this step and is left alone
  float* s1;                   // exp_avg / momentum_buffer
  float* s2;                   // exp_avg_sq (Adam)
  long long n;
  long long t;                 // the tensor's step count, this step included (1 = its first)
};
static_assert(sizeof(OptSeg) == PCC_OPTIM_SEG_WORDS * sizeof(int64_t), "segment row layout");

// the chunk of this workgroup: its segment and the element range [start, start + len) inside it; len = 0: nothing to do
// (a table entry that names no segment or lies outside its tensor gives len = 0, never an access)
__device__ __forceinline__ int opt_chunk(const OptSeg* __restrict__ segs, int n_segs, const int* __restrict__ chunks, OptSeg& S,
                                         long long& start) {
  const int seg = chunks[2 * (long long)blockIdx.x], idx = chunks[2 * (long long)blockIdx.x + 1];
  if (seg < 0 || seg >= n_segs || idx < 0) return 0;
  S = segs[seg];
  start = (long long)idx * OPT_CHUNK;
  if (!S.g || start >= S.n) return 0;
  const long long left = S.n - start;
  return (int)(left < OPT_CHUNK ? left : OPT_CHUNK);
}

__device__ __forceinline__ bool opt_aligned16(const void* a, const void* b, const void* c, const void* d) {
  return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)d)) & 15) == 0;
}

// sum over the workgroup in a fixed order: lanes of a wave by butterfly, the four waves in order; every thread gets it
__device__ __forceinline__ double opt_block_sum(double acc, double* s_w) {
#pragma unroll
  for (int d = PCC_WAVE / 2; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = acc;
  __syncthreads();
  const double total = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
  __syncthreads();
  return total;
}

// Squared-norm pass: partials[chunk] = sum of g * g over the chunk.  Thread i takes the groups i, i + 256, ... of four
// consecutive elements, each group's elements in order -- the same order whether a group is one 16-byte load or (a base
// that is not 16-byte aligned, the last group of a tensor) up to four scalar loads.
__global__ void __launch_bounds__(OPT_T) k_optim_sqnorm(const OptSeg* __restrict__ segs, int n_segs, const int* __restrict__ chunks,
                                                        double* __restrict__ partials) {
  __shared__ double s_w[OPT_T / PCC_WAVE];
  OptSeg S;
  long long start = 0;
  const int len = opt_chunk(segs, n_segs, chunks, S, start);     // uniform over the workgroup
  double acc = 0.0;
  if (len > 0) {
    const float* g = S.g + start;
    const bool vec = opt_aligned16(g, nullptr, nullptr, nullptr);
    const int groups = (len + 3) >> 2;
    for (int j = threadIdx.x; j < groups; j += OPT_T) {
      const int e = 4 * j;
      if (vec && e + 4 <= len) {
        const float4 v = *reinterpret_cast<const float4*>(g + e);
        acc = fma((double)v.x, (double)v.x, acc);
        acc = fma((double)v.y, (double)v.y, acc);
        acc = fma((double)v.z, (double)v.z, acc);
        acc = fma((double)v.w, (double)v.w, acc);
      } else {
        const int m = min(4, len - e);
        for (int k = 0; k < m; ++k) {
          const double v = (double)g[e + k];
          acc = fma(v, v, acc);
        }
      }
    }
  }
  const double total = opt_block_sum(acc, s_w);
  if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

struct OptScalars {
  int mode;                    // PCC_OPTIM_ADAM / PCC_OPTIM_SGD
  float lr, b1, b2, eps;       // b1: Adam's beta1 or SGD's momentum
  float one_m_b1, one_m_b2;    // 1 - beta, rounded once from the double difference (as torch's scalar arguments are)
  double db1, db2;             // the betas in double, for the bias corrections
  float max_norm;              // <= 0: no clipping
};

// (every fused multiply-add is written out, so the vector and the scalar path round alike whatever the compiler contracts)
template <int MODE>
__device__ __forceinline__ void opt_update(float& p, float g, float& s1, float& s2, float coef, bool first, float step_size,
                                           float bc2_sqrt, const OptScalars& A) {
  g *= coef;                                   // the clipped gradient; the stored gradient keeps its value
  if (MODE == PCC_OPTIM_ADAM) {
    s1 = fmaf(A.b1, s1, A.one_m_b1 * g);
    s2 = fmaf(A.b2, s2, A.one_m_b2 * (g * g));
    p = fmaf(-step_size, s1 / (sqrtf(s2) / bc2_sqrt + A.eps), p);
  } else {
    s1 = first ? g : fmaf(A.b1, s1, g);
    p = fmaf(-A.lr, s1, p);
  }
}

// Update pass.  Every workgroup adds the partials in the same fixed order (thread i takes partials i, i + 256, ...; then
// opt_block_sum), so all of them hold the same norm and the same clipping coefficient without a second launch or a read.
template <int MODE>
__global__ void __launch_bounds__(OPT_T) k_optim_step(const OptSeg* __restrict__ segs, int n_segs, const int* __restrict__ chunks,
                                                      int n_chunks, const double* __restrict__ partials, const OptScalars A,
                                                      float* __restrict__ d_norm) {
  __shared__ double s_w[OPT_T / PCC_WAVE];
  float coef = 1.0f;
  if (A.max_norm > 0.0f) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_chunks; i += OPT_T) acc += partials[i];
    const float norm = (float)sqrt(opt_block_sum(acc, s_w));
    const float c = A.max_norm / (norm + 1e-6f);
    coef = c > 1.0f ? 1.0f : c;                // torch.clamp(c, max=1.0): a NaN stays a NaN
    if (blockIdx.x == 0 && threadIdx.x == 0 && d_norm) *d_norm = norm;
  }
  OptSeg S;
  long long start = 0;
  const int len = opt_chunk(segs, n_segs, chunks, S, start);
  if (len <= 0) return;
  float step_size = A.lr, bc2_sqrt = 1.0f;
  if (MODE == PCC_OPTIM_ADAM) {                // torch: step_size = lr / (1 - b1^t), sqrt(1 - b2^t), in double
    const double t = (double)S.t;
    step_size = (float)((double)A.lr / (1.0 - pow(A.db1, t)));
    bc2_sqrt = (float)sqrt(1.0 - pow(A.db2, t));
  }
  const bool first = S.t <= 1;
  float* p = S.p + start;
  const float* g = S.g + start;
  float* s1 = S.s1 + start;
  float* s2 = MODE == PCC_OPTIM_ADAM ? S.s2 + start : nullptr;
  const bool vec = opt_aligned16(p, g, s1, s2);
  const int groups = (len + 3) >> 2;
  for (int j = threadIdx.x; j < groups; j += OPT_T) {
    const int e = 4 * j;
    if (vec && e + 4 <= len) {
      float4 vp = *reinterpret_cast<const float4*>(p + e);
      const float4 vg = *reinterpret_cast<const float4*>(g + e);
      float4 v1 = *reinterpret_cast<const float4*>(s1 + e);
      float4 v2 = make_float4(0.f, 0.f, 0.f, 0.f);
      if (MODE == PCC_OPTIM_ADAM) v2 = *reinterpret_cast<const float4*>(s2 + e);
      opt_update<MODE>(vp.x, vg.x, v1.x, v2.x, coef, first, step_size, bc2_sqrt, A);
      opt_update<MODE>(vp.y, vg.y, v1.y, v2.y, coef, first, step_size, bc2_sqrt, A);
      opt_update<MODE>(vp.z, vg.z, v1.z, v2.z, coef, first, step_size, bc2_sqrt, A);
      opt_update<MODE>(vp.w, vg.w, v1.w, v2.w, coef, first, step_size, bc2_sqrt, A);
      *reinterpret_cast<float4*>(p + e) = vp;
      *reinterpret_cast<float4*>(s1 + e) = v1;
      if (MODE == PCC_OPTIM_ADAM) *reinterpret_cast<float4*>(s2 + e) = v2;
    } else {
      const int m = min(4, len - e);
      for (int k = 0; k < m; ++k) {
        float vp = p[e + k], v1 = s1[e + k], v2 = MODE == PCC_OPTIM_ADAM ? s2[e + k] : 0.f;
        opt_update<MODE>(vp, g[e + k], v1, v2, coef, first, step_size, bc2_sqrt, A);
        p[e + k] = vp;
        s1[e + k] = v1;
        if (MODE == PCC_OPTIM_ADAM) s2[e + k] = v2;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
extern "C" int32_t pcc_optim_chunk_elems(void) { return OPT_CHUNK; }

extern "C" int64_t pcc_optim_build_chunks(const int64_t* h_sizes, int32_t n_segs, int32_t* h_chunks, int64_t cap) {
  if (n_segs < 0 || (n_segs > 0 && !h_sizes)) return -1;
  int64_t count = 0;
  for (int32_t s = 0; s < n_segs; ++s) {
    if (h_sizes[s] < 0) return -1;
    const int64_t c = pcc_cdiv(h_sizes[s], OPT_CHUNK);
    if (c >= (1ll << 31) || count + c >= (1ll << 31)) return -1;
    if (h_chunks)
      for (int64_t i = 0; i < c && count + i < cap; ++i) {
        h_chunks[2 * (count + i)] = s;
        h_chunks[2 * (count + i) + 1] = (int32_t)i;
      }
    count += c;
  }
  return count;
}

extern "C" size_t pcc_optim_ws_bytes(int64_t n_chunks) {
  return pcc_align_up((size_t)(n_chunks > 0 ? n_chunks : 0) * sizeof(double));
}

static int optim_check(const char* who, const void* d_segs, int32_t n_segs, const void* d_chunks, int64_t n_chunks, const void* ws,
                       size_t ws_bytes, bool need_ws) {
  PCC_REQUIRE(n_segs >= 0, "%s: n_segs = %d is negative", who, n_segs);
  PCC_REQUIRE(n_chunks >= 0 && n_chunks < (1ll << 31), "%s: n_chunks = %lld outside 0..2^31-1", who, (long long)n_chunks);
  if (n_chunks == 0) return PCC_OK;
  PCC_REQUIRE(d_segs && n_segs > 0, "%s: %lld chunks but no segment table", who, (long long)n_chunks);
  PCC_REQUIRE(d_chunks, "%s: the chunk table is NULL", who);
  if (need_ws && (!ws || ws_bytes < pcc_optim_ws_bytes(n_chunks))) {
    pcc_set_error("%s: workspace of %zu bytes, %zu needed", who, ws ? ws_bytes : (size_t)0, pcc_optim_ws_bytes(n_chunks));
    return PCC_EWS;
  }
  return PCC_OK;
}

extern "C" int pcc_optim_sqnorm(const int64_t* d_segs, int32_t n_segs, const int32_t* d_chunks, int64_t n_chunks, void* ws,
                                size_t ws_bytes, void* stream) {
  PCC_TRY(optim_check("pcc_optim_sqnorm", d_segs, n_segs, d_chunks, n_chunks, ws, ws_bytes, true));
  if (n_chunks == 0) return PCC_OK;
  k_optim_sqnorm<<<(unsigned)n_chunks, OPT_T, 0, (hipStream_t)stream>>>((const OptSeg*)d_segs, n_segs, d_chunks, (double*)ws);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_optim_step(const int64_t* d_segs, int32_t n_segs, const int32_t* d_chunks, int64_t n_chunks, const void* ws,
                              size_t ws_bytes, int32_t mode, double lr, double beta1, double beta2, double eps, double max_norm,
                              float* d_norm, void* stream) {
  const bool clip = max_norm > 0.0;
  PCC_REQUIRE(mode == PCC_OPTIM_ADAM || mode == PCC_OPTIM_SGD, "pcc_optim_step: mode %d is neither Adam nor SGD", mode);
  PCC_REQUIRE(!isnan(max_norm), "pcc_optim_step: max_norm is NaN");
  PCC_TRY(optim_check("pcc_optim_step", d_segs, n_segs, d_chunks, n_chunks, ws, ws_bytes, clip));
  if (n_chunks == 0) return PCC_OK;
  OptScalars A;
  A.mode = mode;
  A.lr = (float)lr; A.b1 = (float)beta1; A.b2 = (float)beta2; A.eps = (float)eps;
  A.one_m_b1 = (float)(1.0 - beta1); A.one_m_b2 = (float)(1.0 - beta2);
  A.db1 = beta1; A.db2 = beta2;
  A.max_norm = clip ? (float)max_norm : 0.0f;
  hipStream_t s = (hipStream_t)stream;
  if (mode == PCC_OPTIM_ADAM)
    k_optim_step<PCC_OPTIM_ADAM><<<(unsigned)n_chunks, OPT_T, 0, s>>>((const OptSeg*)d_segs, n_segs, d_chunks, (int)n_chunks,
                                                                     (const double*)ws, A, d_norm);
  else
    k_optim_step<PCC_OPTIM_SGD><<<(unsigned)n_chunks, OPT_T, 0, s>>>((const OptSeg*)d_segs, n_segs, d_chunks, (int)n_chunks,
                                                                    (const double*)ws, A, d_norm);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}
