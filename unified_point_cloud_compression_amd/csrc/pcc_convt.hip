// Transposed (generative) convolutions: the row-subset form on CSR pair lists (pcc_convt_fwd_rows), the input-stationary dense
// product with its ordered gather-sums (pcc_convt_fwd, pcc_convt_fwd_csr, pcc_convt_fwd_csr_grid) and their weight pack.
// The products themselves are launch_mfma / launch_pair_product of pcc_conv.hip; this file holds the bucketing and gather-sum
// kernels and the entry points, which are called from the Python side only.
#include "pcc_conv.h"

static constexpr int MAXK_T = 512;  // offsets of the input-stationary transposed conv (a flat GEMM: 7^3 composites fit)

// ------------------------------------------------------------------------------------------
// Transposed convolution on a SUBSET of its output rows (the rows that survive the top-k pruning), straight from their
// CSR pair lists: the P pairs are bucketed by kernel offset (LDS counting sort; the position inside a bucket does not
// matter, every T row depends on its own pair only), T[p] = feat[in(p)] @ W[k(p)] runs as the gathered pair GEMM, and
// out[o] = act(bias + sum over the row's CSR entries of T[slot(entry)]) is summed in CSR order.  Work ~ P, where the
// dense input-stationary form computes all n_in*K products and the slot-map form touches K*n_out slots.
// ------------------------------------------------------------------------------------------
static constexpr int CK_T = 256, CK_I = 8, CK_B = CK_T * CK_I;

__global__ void __launch_bounds__(CK_T) k_csr_khist(const int* __restrict__ pair_ids, const int* __restrict__ d_P, int K,
                                                    int nb, int* __restrict__ hist) {
  __shared__ int h[MAXK];
  for (int i = threadIdx.x; i < K; i += CK_T) h[i] = 0;
  __syncthreads();
  const int P = *d_P;
  const long long base = (long long)blockIdx.x * CK_B;
#pragma unroll
  for (int r = 0; r < CK_I; ++r) {
    const long long t = base + r * CK_T + threadIdx.x;
    if (t < P) atomicAdd(&h[pair_ids[t] % K], 1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < K; i += CK_T) hist[(long long)i * nb + blockIdx.x] = h[i];
}

__global__ void __launch_bounds__(128) k_csr_kstarts(const int* __restrict__ off, const int* __restrict__ d_P, int K, int nb,
                                                     int* __restrict__ pstart, long long* __restrict__ info) {
  __shared__ long long cnt[MAXK];
  const long long total = *d_P;
  for (int k = threadIdx.x; k < K; k += blockDim.x) {
    const long long b = off[(long long)k * nb];
    const long long e = (k + 1 < K) ? off[(long long)(k + 1) * nb] : total;
    cnt[k] = e - b;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  long long run = 0;
  for (int k = 0; k < K; ++k) {
    pstart[k] = (int)run;
    run += (cnt[k] + PAIR_BM - 1) / PAIR_BM * PAIR_BM;
  }
  pstart[K] = (int)run;
  info[0] = run; info[1] = run / PAIR_BM; info[2] = total;
}

__global__ void __launch_bounds__(CK_T) k_csr_kscatter(const int* __restrict__ pair_ids, const int* __restrict__ d_P, int K,
                                                       int nb, const int* __restrict__ off, const int* __restrict__ pstart,
                                                       int* __restrict__ pair_in, int* __restrict__ slot) {
  __shared__ int cur[MAXK];
  for (int i = threadIdx.x; i < K; i += CK_T)
    cur[i] = pstart[i] + off[(long long)i * nb + blockIdx.x] - off[(long long)i * nb];
  __syncthreads();
  const int P = *d_P;
  const long long base = (long long)blockIdx.x * CK_B;
#pragma unroll
  for (int r = 0; r < CK_I; ++r) {
    const long long t = base + r * CK_T + threadIdx.x;
    if (t < P) {
      const int pid = pair_ids[t];
      const int i = pid / K, k = pid - i * K;
      const int pos = atomicAdd(&cur[k], 1);
      pair_in[pos] = i;
      slot[t] = pos;
    }
  }
}

struct CsrReduceArgs {
  const float* T; const float* bias; const int* first; const int* slot; float* out; long long n_out;
  int cout, act; float slope; int lpr_log2;
};

__global__ void __launch_bounds__(256) k_csr_reduce(CsrReduceArgs a) {
  constexpr int JB = 4;
  const int lane = threadIdx.x & 63;
  const int lpr = 1 << a.lpr_log2;
  const int rpw = 64 >> a.lpr_log2;
  const long long o = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * rpw + (lane >> a.lpr_log2);
  const int cl = lane & (lpr - 1);
  if (o >= a.n_out) return;
  const int cvec = a.cout / 4;
  const int t0 = a.first[o], t1 = a.first[o + 1];
  for (int cv = cl; cv < cvec; cv += lpr) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t = t0; t < t1; t += JB) {
      int sl[JB];
#pragma unroll
      for (int u = 0; u < JB; ++u) sl[u] = (t + u < t1) ? a.slot[t + u] : -1;
      float4 x[JB];
#pragma unroll
      for (int u = 0; u < JB; ++u) {
        x[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (sl[u] >= 0) x[u] = reinterpret_cast<const float4*>(a.T + (long long)sl[u] * a.cout)[cv];
      }
#pragma unroll
      for (int u = 0; u < JB; ++u) { acc.x += x[u].x; acc.y += x[u].y; acc.z += x[u].z; acc.w += x[u].w; }
    }
    if (a.bias) {
      const float4 b = reinterpret_cast<const float4*>(a.bias)[cv];
      acc.x += b.x; acc.y += b.y; acc.z += b.z; acc.w += b.w;
    }
    acc.x = act1(acc.x, a.act, a.slope); acc.y = act1(acc.y, a.act, a.slope);
    acc.z = act1(acc.z, a.act, a.slope); acc.w = act1(acc.w, a.act, a.slope);
    reinterpret_cast<float4*>(a.out + o * a.cout)[cv] = acc;
  }
}

// pairs: host value of first[n_out] (the number of CSR entries).  Scratch: int_ws and T sized by the two queries.
extern "C" size_t pcc_convt_rows_int_ws_bytes(int64_t pairs, int32_t K) {
  const int64_t nb = pcc_cdiv(pairs > 0 ? pairs : 1, CK_B);
  const int64_t padded = pairs + (int64_t)K * PAIR_BM;
  return pcc_align_up((size_t)K * nb * 4) + pcc_align_up((size_t)padded * 4) + pcc_align_up((size_t)(pairs + 1) * 4) +
         pcc_align_up((size_t)(padded / PAIR_BM + 1) * 4) + pcc_align_up((size_t)(K + 1) * 4) + 64 +
         pcc_scan_ws_bytes((int64_t)K * nb) + 1024;
}
extern "C" int64_t pcc_convt_rows_t_elems(int64_t pairs, int32_t K, int32_t cout) {
  return (pairs + (int64_t)K * PAIR_BM) * cout;
}

extern "C" int pcc_convt_fwd_rows(const float* feat_in, int64_t n_in, int32_t cin, const float* packed_w,
                                  const float* bias, int32_t K, int32_t cout, const int32_t* first,
                                  const int32_t* pair_ids, int64_t n_out, int64_t pairs, float* T, float* out,
                                  int32_t act, float slope, void* int_ws, size_t int_ws_bytes, int32_t arith, int32_t* d_guard,
                                  void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n_out <= 0) return PCC_OK;
  PCC_REQUIRE(feat_in && packed_w && first && pair_ids && T && out && int_ws, "pcc_convt_fwd_rows: NULL array");
  PCC_REQUIRE(K >= 1 && K <= MAXK && conv_kind(K, cin, cout) == KIND_MFMA && cout % 4 == 0,
              "pcc_convt_fwd_rows: shape K=%d cin=%d cout=%d not on the MFMA path", K, cin, cout);
  PCC_REQUIRE(pairs >= 0 && pairs + (int64_t)K * PAIR_BM < (1ll << 31) && act >= 0 && act <= 2, "pcc_convt_fwd_rows: bad arguments");
  if (int_ws_bytes < pcc_convt_rows_int_ws_bytes(pairs, K)) { pcc_set_error("pcc_convt_fwd_rows: workspace too small"); return PCC_EWS; }
  const int64_t nb = pcc_cdiv(pairs > 0 ? pairs : 1, CK_B);
  const int64_t padded_cap = pairs + (int64_t)K * PAIR_BM;
  char* p = (char*)int_ws;
  int* hist = (int*)p;        p += pcc_align_up((size_t)K * nb * 4);
  int* pair_in = (int*)p;     p += pcc_align_up((size_t)padded_cap * 4);
  int* slot = (int*)p;        p += pcc_align_up((size_t)(pairs + 1) * 4);
  int* tile_k = (int*)p;      p += pcc_align_up((size_t)(padded_cap / PAIR_BM + 1) * 4);
  int* pstart = (int*)p;      p += pcc_align_up((size_t)(K + 1) * 4);
  long long* info = (long long*)p;  p += 64;
  void* scan_ws = p;
  const size_t scan_bytes = int_ws_bytes - (size_t)(p - (char*)int_ws);
  const int* d_P = first + n_out;
  k_csr_khist<<<(unsigned)nb, CK_T, 0, s>>>(pair_ids, d_P, K, (int)nb, hist);
  PCC_LAUNCH_CHECK();
  PCC_TRY(pcc_scan_exclusive_i32(hist, hist, (int64_t)K * nb, scan_ws, scan_bytes, s));
  k_csr_kstarts<<<1, 128, 0, s>>>(hist, d_P, K, (int)nb, pstart, info);
  PCC_LAUNCH_CHECK();
  PCC_CHECK_HIP(hipMemsetAsync(pair_in, 0xFF, (size_t)padded_cap * 4, s));
  k_csr_kscatter<<<(unsigned)nb, CK_T, 0, s>>>(pair_ids, d_P, K, (int)nb, hist, pstart, pair_in, slot);
  PCC_LAUNCH_CHECK();
  const int64_t tiles_cap = padded_cap / PAIR_BM;
  PCC_TRY(launch_pair_tile_k(pstart, K, tiles_cap, tile_k, s));
  ConvArgs a = conv_args(feat_in, n_in, cin, packed_w, K, cout, nullptr, T, padded_cap);
  a.pair_in = pair_in; a.tile_k = tile_k; a.n_tiles = info + 1;
  PCC_TRY(set_arith(a, arith, d_guard, "pcc_convt_fwd_rows"));
  PCC_TRY(launch_pair_product(a, K, tiles_cap, s));
  CsrReduceArgs r;
  r.T = T; r.bias = bias; r.first = first; r.slot = slot; r.out = out; r.n_out = n_out; r.cout = cout; r.act = act; r.slope = slope;
  int l = 0;
  while ((1 << l) < cout / 4 && l < 6) ++l;
  r.lpr_log2 = l;
  const int64_t waves = pcc_cdiv(n_out, 64 >> l);
  k_csr_reduce<<<(unsigned)pcc_cdiv(waves, 4), 256, 0, s>>>(r);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

// ------------------------------------------------------------------------------------------
// Generative transposed convolution, input stationary.
//   Every (input row i, kernel offset k) is exactly one pair of the map, so the products
//   T[i][k][:] = feat[i] @ W[k] form ONE dense GEMM  [n_in, cin] x [cin, K*cout]  with no gather and no padding
//   waste, however sparse the output neighbourhoods are.  The sum over the pairs of an output row is then taken
//   in fixed order (class offsets ascending) through the transposed map: deterministic, no atomics.
// ------------------------------------------------------------------------------------------
__global__ void k_pack_convt(const float* __restrict__ W, int K, int cin, int cout, int ncol, int cout_pad,
                             int cb_log2, float* __restrict__ out) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long total = (long long)cin * cout_pad;
  if (t >= total) return;
  const int CB = 1 << cb_log2;
  const int within = (int)(t & (CB - 1));
  const long long q = t >> cb_log2;
  const int col = (int)(q % cout_pad);
  const int cbi = (int)(q / cout_pad);
  const int ci = (cbi << cb_log2) + within;
  float v = 0.f;
  if (col < ncol) {
    const int k = col / cout, co = col - k * cout;
    v = W[((long long)k * cin + ci) * cout + co];
  }
  out[t] = v;
}

// dense-product packs (cin a multiple of 32): fp32 image | three bf16 planes | two scaled fp16 planes | 1/scale per column
static bool convt_has_h(int cin) { return cin % 32 == 0 && cin <= 256; }
extern "C" int64_t pcc_convt_packed_elems(int32_t K, int32_t cin, int32_t cout) {
  if (K <= 0 || cin <= 0 || cout <= 0 || !mfma_ok(cin, K * cout)) return 0;
  const int64_t base = (int64_t)cin * cout_pad_for(K * cout);
  return mfma_packed_total(base, cin) + (convt_has_h(cin) ? base + cout_pad_for(K * cout) : 0);
}

extern "C" int pcc_convt_pack_weights(const float* W, int32_t K, int32_t cin, int32_t cout, float* packed,
                                      int64_t packed_cap, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PCC_REQUIRE(W && packed && K >= 1 && K <= MAXK_T && cin >= 1 && cout >= 1, "pcc_convt_pack_weights: bad arguments");
  PCC_REQUIRE(mfma_ok(cin, K * cout), "pcc_convt: unsupported shape cin=%d (needs 4, 8, 16 or a multiple of 32)", cin);
  const int64_t total = pcc_convt_packed_elems(K, cin, cout);
  if (packed_cap < total) {
    pcc_set_error("pcc_convt_pack_weights: packed buffer holds %lld floats, the layout needs %lld", (long long)packed_cap, (long long)total);
    return PCC_EWS;
  }
  const int64_t base = (int64_t)cin * cout_pad_for(K * cout);
  k_pack_convt<<<(unsigned)pcc_cdiv(base, 256), 256, 0, s>>>(W, K, cin, cout, K * cout, cout_pad_for(K * cout),
                                                            cb_log2_for(cin), packed);
  PCC_LAUNCH_CHECK();
  PCC_TRY(split_planes(packed, base, cin, s));
  if (convt_has_h(cin)) {
    const int cp = cout_pad_for(K * cout);
    PCC_TRY(split_planes_h(packed, base, 1, cin, cp, s));
  }
  return PCC_OK;
}

struct GatherArgs {
  const float* T; const float* bias; const int* hdr; const int* nbr; const int* rows;
  float* out; long long n_out; int K, cout, act; float slope; int lpr_log2;
};

// LPR lanes per output position, VEC channels per lane and pass; offsets in batches of independent loads
template <int VEC>
__global__ void __launch_bounds__(256) k_convt_gather(GatherArgs a) {
  typedef typename ThinVec<VEC>::T VT;
  constexpr int JB = 9;
  const int lane = threadIdx.x & 63;
  const int lpr = 1 << a.lpr_log2;
  const int rpw = 64 >> a.lpr_log2;
  const long long p = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * rpw + (lane >> a.lpr_log2);
  const int cl = lane & (lpr - 1);
  if (p >= a.n_out) return;
  const int cvec = a.cout / VEC;
  const int nseg = a.hdr[HDR_NSEG];
  int s = 0;
  for (; s < nseg - 1; ++s) {
    const int* sg = a.hdr + HDR_SEG0 + s * SEG_WORDS;
    if (p < (long long)sg[SEG_POS_BEGIN] + sg[SEG_POS_COUNT]) break;
  }
  const int* sg = a.hdr + HDR_SEG0 + s * SEG_WORDS;
  const int k_count = sg[SEG_K_COUNT], koff_begin = sg[SEG_KOFF_BEGIN];
  const long long spc = sg[SEG_POS_COUNT], local = p - sg[SEG_POS_BEGIN];
  const int* seg_nbr = a.nbr + (((long long)(unsigned)sg[SEG_NBR_LO]) | ((long long)sg[SEG_NBR_HI] << 32));
  const long long orow = a.rows ? a.rows[p] : p;
  for (int cv = cl; cv < cvec; cv += lpr) {
    VT acc;
    thin_zero(acc);
    for (int j0 = 0; j0 < k_count; j0 += JB) {
      int ir[JB];
#pragma unroll
      for (int u = 0; u < JB; ++u) ir[u] = (j0 + u < k_count) ? seg_nbr[(long long)(j0 + u) * spc + local] : -1;
      VT x[JB];
#pragma unroll
      for (int u = 0; u < JB; ++u) {
        thin_zero(x[u]);
        if (ir[u] >= 0) {
          const int kid = a.hdr[HDR_KOFFS + koff_begin + j0 + u];
          x[u] = reinterpret_cast<const VT*>(a.T + ((long long)ir[u] * a.K + kid) * a.cout)[cv];
        }
      }
#pragma unroll
      for (int u = 0; u < JB; ++u) thin_acc(acc, x[u]);     // fixed order: offsets ascending
    }
    VT b;
    thin_zero(b);
    if (a.bias) b = reinterpret_cast<const VT*>(a.bias)[cv];
    thin_acc(acc, b);
    thin_act(acc, a.act, a.slope);
    reinterpret_cast<VT*>(a.out + orow * a.cout)[cv] = acc;
  }
}

extern "C" int pcc_convt_fwd(const float* feat_in, int64_t n_in, int32_t cin, const float* packed_w, const float* bias,
                             int32_t K, int32_t cout, const int32_t* hdr, const int32_t* nbr, const int32_t* rows,
                             int64_t n_out, float* T, float* out, int32_t act, float slope, int32_t arith, int32_t* d_guard,
                             void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n_out <= 0 || n_in <= 0) return PCC_OK;
  PCC_REQUIRE(feat_in && packed_w && hdr && nbr && rows && T && out, "pcc_convt_fwd: NULL array");
  PCC_REQUIRE(K >= 1 && K <= MAXK && mfma_ok(cin, K * cout), "pcc_convt_fwd: unsupported shape K=%d cin=%d cout=%d", K, cin, cout);
  PCC_REQUIRE(act >= 0 && act <= 2, "pcc_convt_fwd: bad activation");
  PCC_REQUIRE(n_in < (1ll << 31) && n_out < (1ll << 31), "pcc_convt_fwd: too many rows");
  // 1) dense GEMM  T[n_in, K*cout] = feat[n_in, cin] @ Wflat[cin, K*cout]
  ConvArgs a = conv_args(feat_in, n_in, cin, packed_w, 1, K * cout, nullptr, T, n_in);
  a.wh_ok = convt_has_h(cin);
  PCC_TRY(set_arith(a, arith, d_guard, "pcc_convt_fwd"));
  PCC_TRY(prof_begin(s));
  PCC_TRY(launch_mfma(MODE_CONV, a, 0, s));
  PCC_TRY(prof_end(s));
  // 2) ordered gather-sum through the transposed map
  GatherArgs g;
  g.T = T; g.bias = bias; g.hdr = hdr; g.nbr = nbr; g.rows = rows; g.out = out; g.n_out = n_out; g.K = K; g.cout = cout;
  g.act = act; g.slope = slope;
  const int vec = (cout % 4 == 0) ? 4 : 1;
  int l = 0;
  while ((1 << l) < cout / vec && l < 6) ++l;
  g.lpr_log2 = l;
  const int64_t waves = pcc_cdiv(n_out, 64 >> l);
  if (vec == 4) k_convt_gather<4><<<(unsigned)pcc_cdiv(waves, 4), 256, 0, s>>>(g);
  else k_convt_gather<1><<<(unsigned)pcc_cdiv(waves, 4), 256, 0, s>>>(g);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

// CSR form of the generative transposed convolution: out[o] = act(bias + sum_{t in [first[o], first[o+1])} T[pair_ids[t]])
// (pair lists from pcc_coords_expand_csr; outputs are written in canonical row order, no `rows` indirection).
// Subset sums of the per-neighbour constants: tab[j][m][c] = sum over the set bits b of m (ascending) of ex_bias[7j + b][c].
// A row's 27-bit neighbour mask then costs four table rows instead of a loop over its ~22 set bits (the loop was a third of the
// gather-sum's VALU instructions, and the kernel is VALU-bound: 6.6e8 wave instructions on the last level, SQ counters).
__global__ void k_presence_tables(const float* __restrict__ ex_bias, int cout, float* __restrict__ tab) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 512 * cout) return;
  const int c = t % cout, m = (t / cout) & 127, j = t / (128 * cout);
  float sum = 0.f;
  for (int b = 0; b < 7; ++b) {
    const int k = 7 * j + b;
    if (k < 27 && ((m >> b) & 1)) sum += ex_bias[k * cout + c];
  }
  tab[t] = sum;
}

// non-temporal accesses of HIP's vector structs (the builtins take native vector types)
typedef float f32x4n __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 nt_load(const float4* p) {
  const f32x4n v = __builtin_nontemporal_load(reinterpret_cast<const f32x4n*>(p));
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ float nt_load(const float* p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ void nt_store(const float4& v, float4* p) {
  const f32x4n w = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(w, reinterpret_cast<f32x4n*>(p));
}
__device__ __forceinline__ void nt_store(float v, float* p) { __builtin_nontemporal_store(v, p); }

struct GatherCsrArgs {
  const float* T; const float* bias; const int* first; const int* pair_ids;
  const int* wg_end = nullptr;                            // slotted lists (pcc_coords_expand_grid_csr_slots): end of the last row of every 256 rows
  float* out; long long n_out; int cout, act; float slope; int lpr_log2;
  const int* ex_nbr; const float* ex_bias; int ex_K;      // optional: + sum over the existing neighbours k of ex_bias[k]
  const float* ex_tab;                                    //   as subset-sum tables [4][128][cout] over 7+7+7+6 neighbour bits (k_presence_tables)
  PccGrid ex_grid; const long long* out_keys;             //   presence flags from a [K][n_out] table (ex_nbr) or the set's grid index
  int nt;                                                 // g_nt: 4 = non-temporal product loads, 8 = non-temporal output stores
};

template <int VEC, int JB>
__global__ void __launch_bounds__(256) k_convt_gather_csr(GatherCsrArgs a) {
  typedef typename ThinVec<VEC>::T VT;
  const int lane = threadIdx.x & 63;
  const int lpr = 1 << a.lpr_log2;
  const int rpw = 64 >> a.lpr_log2;
  const long long o = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * rpw + (lane >> a.lpr_log2);
  const int cl = lane & (lpr - 1);
  if (o >= a.n_out) return;
  const int cvec = a.cout / VEC;
  const int t0 = a.first[o];
  const int t1 = (a.wg_end && ((o & 255) == 255 || o + 1 == a.n_out)) ? a.wg_end[o >> 8] : a.first[o + 1];
  // optional constant per existing neighbour (two fused affine layers): the lanes of the row's group fetch the ex_K presence
  // flags side by side and share them by ballot (one load per lane instead of ex_K dependent loads: the serial loop cost
  // 2.1 ms on the level-2 head in round 2)
  unsigned long long present = 0;
  // 3x3x3 presence straight from the output set's bitmap, the nine (dx, dy) columns dealt over the row's lanes.  Branch-free
  // (round 3): a lane's <= 3 columns are 64-bit windows that start at the 32-bit word of the column's first cell (the 3-bit z
  // field never straddles), absent columns re-read cell 0 and are masked -- all of a lane's loads are in flight together and
  // are consumed after the pair loop below.  (The loop form waited for each column's word in turn: three exposed L2 latencies
  // per row on the last level, where a row has four lanes.)
  unsigned pw_lo[3] = {0, 0, 0}, pw_hi[3] = {0, 0, 0};
  int psh[3] = {64, 64, 64}, pcol[3] = {0, 0, 0};
  int p_nz = 0, p_dz0 = 0;
  if (a.ex_grid.bits && lpr < 4) {                                  // (<= 8 channels: a row has one or two lanes, the loop form)
    unsigned m = pcc_grid_nbr27(a.ex_grid, a.out_keys[o], cl, lpr, nullptr);
    for (int d = lpr >> 1; d >= 1; d >>= 1) m |= __shfl_xor((int)m, d);
    present = m;
  } else if (a.ex_grid.bits) {
    const PccGrid& g = a.ex_grid;
    const PccLattice& L = g.lat;
    const long long key = a.out_keys[o];
    const int b = pcc_key_b(key);
    const int cx = (pcc_key_x(key) - L.lo[0]) >> L.ts_log2;
    const int cy = (pcc_key_y(key) - L.lo[1]) >> L.ts_log2;
    const int cz = (pcc_key_z(key) - L.lo[2]) >> L.ts_log2;
    const int z_lo = cz > 0 ? cz - 1 : 0, z_hi = cz + 1 < L.dims[2] ? cz + 1 : L.dims[2] - 1;
    p_nz = z_hi - z_lo + 1;
    p_dz0 = z_lo - cz + 1;
    const long long col_stride = L.dims[2], slab_stride = (long long)L.dims[1] * L.dims[2];
    const long long cell0 = pcc_lat_cell(L, b, cx, cy, z_lo);
    const long long cells = (long long)L.nbatch * L.dims[0] * slab_stride;
    const long long last_dw = 2 * ((cells + 63) >> 6) - 2;
    const unsigned* const bits32 = reinterpret_cast<const unsigned*>(g.bits);
    const int step = lpr < 9 ? lpr : 9;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int c = cl + t * step;
      const int dx = c % 3 - 1, dy = c / 3 - 1;
      const int nx = cx + dx, ny = cy + dy;
      const bool ok = c < 9 && (lpr >= 9 ? t == 0 : true) && nx >= 0 && ny >= 0 && nx < L.dims[0] && ny < L.dims[1];
      const long long cell = ok ? cell0 + dx * slab_stride + dy * col_stride : 0ll;
      const long long dw = cell >> 5, dw2 = dw < last_dw ? dw : last_dw;
      psh[t] = ok ? (int)(cell & 31) + 32 * (int)(dw - dw2) : 64;
      pcol[t] = c;
      pw_lo[t] = bits32[dw2];
      pw_hi[t] = bits32[dw2 + 1];
    }
  } else if (a.ex_nbr) {
    for (int k0 = 0; k0 < a.ex_K; k0 += lpr) {
      const int k = k0 + cl;
      const bool v = k < a.ex_K && a.ex_nbr[(long long)k * a.n_out + o] >= 0;
      const unsigned long long bal = __ballot(v);
      present |= ((bal >> ((lane >> a.lpr_log2) << a.lpr_log2)) & (lpr == 64 ? ~0ull : ((1ull << lpr) - 1ull))) << k0;
    }
  }
  if (a.ex_grid.bits && lpr >= 4) {                                  // finish the presence mask from the windows fetched above
    unsigned pm = 0;
    const unsigned fmask = (1u << p_nz) - 1u;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const unsigned long long w = (unsigned long long)pw_lo[t] | ((unsigned long long)pw_hi[t] << 32);
      const unsigned f = psh[t] < 64 ? (unsigned)(w >> (psh[t] & 63)) & fmask : 0u;
      pm |= ((f & 1u) | ((f & 2u) << 8) | ((f & 4u) << 16)) << (pcol[t] + 9 * p_dz0);     // bit t of the field -> k = c + 9 (dz0 + t)
    }
    for (int d = lpr >> 1; d >= 1; d >>= 1) pm |= __shfl_xor((int)pm, d);
    present = pm;
  }
  for (int cv = cl; cv < cvec; cv += lpr) {
    VT acc;
    thin_zero(acc);
    // branch-free batches: slots past the end of the list re-read the last pair (same cache line) and are weighted 0, so the
    // JB index loads and then the JB product loads of a batch are independent and in flight together
    for (int t = t0; t < t1; t += JB) {
      int pid[JB];
#pragma unroll
      for (int u = 0; u < JB; ++u) pid[u] = a.pair_ids[min(t + u, t1 - 1)];
      VT x[JB];
      if (a.nt & 4) {
#pragma unroll
        for (int u = 0; u < JB; ++u) x[u] = nt_load(reinterpret_cast<const VT*>(a.T + (long long)pid[u] * a.cout) + cv);
      } else {
#pragma unroll
        for (int u = 0; u < JB; ++u) x[u] = reinterpret_cast<const VT*>(a.T + (long long)pid[u] * a.cout)[cv];
      }
#pragma unroll
      for (int u = 0; u < JB; ++u) thin_fma(acc, x[u], (t + u < t1) ? 1.f : 0.f);     // fixed order: pair id ascending
    }
    if (a.ex_tab) {                                                        // constants of the existing neighbours: four subset sums
      const VT* tb = reinterpret_cast<const VT*>(a.ex_tab);
      const unsigned m = (unsigned)present;
      thin_acc(acc, tb[(m & 127u) * cvec + cv]);
      thin_acc(acc, tb[(128u + ((m >> 7) & 127u)) * cvec + cv]);
      thin_acc(acc, tb[(256u + ((m >> 14) & 127u)) * cvec + cv]);
      thin_acc(acc, tb[(384u + ((m >> 21) & 63u)) * cvec + cv]);
    }
    VT b;
    thin_zero(b);
    if (a.bias) b = reinterpret_cast<const VT*>(a.bias)[cv];
    thin_acc(acc, b);
    thin_act(acc, a.act, a.slope);
    if (a.nt & 8) nt_store(acc, reinterpret_cast<VT*>(a.out + o * a.cout) + cv);
    else reinterpret_cast<VT*>(a.out + o * a.cout)[cv] = acc;
  }
}

// (Round 4 built the head's 27 projections INTO this kernel for the 16-channel level -- from the gather-sum's registers, on the
//  matrix pipe, hidden layer never stored -- three ways: stored straight from the MFMA layout (64-byte half lines per wave) 1.60 ms,
//  a wave making four passes to collect whole lines in registers 2.14 (a quarter of the occupancy), the workgroup's planes staged
//  through LDS 1.76 -- against 1.13 for this kernel + 0.58 for k_thin_project_z.  The gather-sum is latency-bound: every
//  instruction added behind its loads costs more than the streaming projection pass saves.  Removed; round-4 history.)
static int presence_tables(const float* ex_bias, int cout, const float** tab, hipStream_t s) {
  void* p = nullptr;
  PCC_TRY(lib_scratch_small((size_t)512 * cout * 4, &p));
  k_presence_tables<<<(unsigned)pcc_cdiv(512 * cout, 256), 256, 0, s>>>(ex_bias, cout, (float*)p);
  PCC_LAUNCH_CHECK();
  *tab = (const float*)p;
  return PCC_OK;
}

// ex_grid / ex_keys: presence source of pcc_convt_fwd_csr_grid (the output set's grid index) or NULL
static int convt_fwd_csr_impl(const float* feat_in, int64_t n_in, int32_t cin, const float* packed_w,
                              const float* bias, int32_t K, int32_t cout, const int32_t* first,
                              const int32_t* pair_ids, int64_t n_out, float* T, float* out, int32_t act, float slope,
                              const int32_t* ex_nbr, int32_t ex_K, const float* ex_bias, const PccGrid* ex_grid,
                              const long long* ex_keys, int32_t arith, int32_t* d_guard, void* stream, const int32_t* wg_end = nullptr) {
  hipStream_t s = (hipStream_t)stream;
  if (n_out <= 0 || n_in <= 0) return PCC_OK;
  PCC_REQUIRE(feat_in && packed_w && first && pair_ids && T && out, "pcc_convt_fwd_csr: NULL array");
  PCC_REQUIRE(K >= 1 && K <= MAXK_T && mfma_ok(cin, K * cout), "pcc_convt_fwd_csr: unsupported shape K=%d cin=%d cout=%d", K, cin, cout);
  PCC_REQUIRE(!ex_nbr || (ex_bias && ex_K >= 1), "pcc_convt_fwd_csr: ex_nbr needs ex_bias and ex_K");
  PCC_REQUIRE(act >= 0 && act <= 2, "pcc_convt_fwd_csr: bad activation");
  PCC_REQUIRE(n_in * K < (1ll << 31) && n_out < (1ll << 31), "pcc_convt_fwd_csr: too many rows");
  ConvArgs a = conv_args(feat_in, n_in, cin, packed_w, 1, K * cout, nullptr, T, n_in);
  a.wh_ok = convt_has_h(cin);
  PCC_TRY(set_arith(a, arith, d_guard, "pcc_convt_fwd_csr"));
  PCC_TRY(prof_begin(s));
  PCC_TRY(launch_mfma(MODE_CONV, a, 0, s));
  PCC_TRY(prof_end(s));
  GatherCsrArgs g;
  g.T = T; g.bias = bias; g.first = first; g.pair_ids = pair_ids; g.out = out; g.n_out = n_out; g.cout = cout;
  g.act = act; g.slope = slope; g.ex_nbr = ex_nbr; g.ex_bias = ex_bias; g.ex_K = ex_K; g.nt = nt_flags();
  g.wg_end = wg_end;
  g.ex_grid.bits = nullptr; g.out_keys = nullptr;
  if (ex_grid) { g.ex_grid = *ex_grid; g.out_keys = ex_keys; g.ex_nbr = nullptr; }
  g.ex_tab = nullptr;
  if (ex_bias) {
    PCC_REQUIRE(ex_K == 27, "pcc_convt_fwd_csr: the per-neighbour constants are those of a 3x3x3 neighbourhood (ex_K=%d)", ex_K);
    PCC_TRY(presence_tables(ex_bias, cout, &g.ex_tab, s));
  }
  const int vec = (cout % 4 == 0) ? 4 : 1;
  int l = 0;
  while ((1 << l) < cout / vec && l < 6) ++l;
  g.lpr_log2 = l;
  const int64_t waves = pcc_cdiv(n_out, 64 >> l);
  const unsigned gg = (unsigned)pcc_cdiv(waves, 4);
  // pair slots per batch of independent loads: narrow outputs (the last level, ~4 pairs per row) take 4, the others 8
  // (measurement: the gather-sum of a composite level is event-timed too -- with the dense products it is the SURVEY 8d unit)
  const bool timed_gather = prof_on() && ex_grid;
  PCC_TRY(prof_begin(s, timed_gather));
  // (round 4 probe: 8 slots on the last level as well -- 1.698 vs 1.703 ms per composite level: the gather-sum is bound by the
  //  memory system's rate on 64-byte pieces, not by loads in flight)
  if (vec == 4 && l <= 2) k_convt_gather_csr<4, 4><<<gg, 256, 0, s>>>(g);
  else if (vec == 4) k_convt_gather_csr<4, 8><<<gg, 256, 0, s>>>(g);
  else k_convt_gather_csr<1, 8><<<gg, 256, 0, s>>>(g);
  PCC_LAUNCH_CHECK();
  PCC_TRY(prof_end(s, timed_gather, PCC_FORM_GATHER_CSR));
  return PCC_OK;
}

extern "C" int pcc_convt_fwd_csr(const float* feat_in, int64_t n_in, int32_t cin, const float* packed_w,
                                 const float* bias, int32_t K, int32_t cout, const int32_t* first,
                                 const int32_t* pair_ids, int64_t n_out, float* T, float* out, int32_t act, float slope,
                                 const int32_t* ex_nbr, int32_t ex_K, const float* ex_bias, int32_t arith, int32_t* d_guard,
                                 void* stream) {
  return convt_fwd_csr_impl(feat_in, n_in, cin, packed_w, bias, K, cout, first, pair_ids, n_out, T, out, act, slope, ex_nbr,
                            ex_K, ex_bias, nullptr, nullptr, arith, d_guard, stream);
}

// pcc_convt_fwd_csr with the constant-per-existing-neighbour term taken from the OUTPUT set's own grid index instead of a
// [27][n_out] neighbour table: the composite up+head convolutions then need no 3x3x3 kernel map of the candidate set at all
// (1.6 GB to write and 1.6 GB to read twice on the benchmark's last level).
extern "C" int pcc_convt_fwd_csr_grid(const float* feat_in, int64_t n_in, int32_t cin, const float* packed_w,
                                      const float* bias, int32_t K, int32_t cout, const int32_t* first,
                                      const int32_t* pair_ids, int64_t n_out, float* T, float* out, int32_t act, float slope,
                                      const int64_t* out_keys, const uint64_t* out_bits, const int32_t* out_rank,
                                      const int32_t* h_out, const float* ex_bias, const int32_t* wg_end, int32_t arith,
                                      int32_t* d_guard, void* stream) {
  PCC_REQUIRE(out_keys && out_bits && out_rank && ex_bias, "pcc_convt_fwd_csr_grid: NULL array");
  PccGrid ex;
  PCC_TRY(pcc_grid_from_host(out_bits, out_rank, h_out, "pcc_convt_fwd_csr_grid", &ex));
  return convt_fwd_csr_impl(feat_in, n_in, cin, packed_w, bias, K, cout, first, pair_ids, n_out, T, out, act, slope,
                            nullptr, 27, ex_bias, &ex, (const long long*)out_keys, arith, d_guard, stream, wg_end);
}
