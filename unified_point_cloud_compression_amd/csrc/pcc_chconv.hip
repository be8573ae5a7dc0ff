// Channelwise sparse convolution by grid gather (reference `loss.py:181-189,219-273`: the Shepard's-loss window sum, and
// `ME.MinkowskiChannelwiseConvolution`).
//
//   out[q][c] = sum_t W[t][c or 0] * feat[row(q + off_t * step)][c]
//
// Output-stationary: one thread per (query, group of channels).  The taps are grouped into (dx, dy) columns by the caller
// (column table: dx, dy, z mask of the taps, first entry in widx[]); for each column the z cells within the kernel radius are
// one bit field of the input set's occupancy bitmap (at most 9 bits, so at most two 64-bit words), clipped to the lattice on
// every axis, and the row of its first occupied cell is rank + popcount; the others follow consecutively (as in
// pcc_grid_nbr27).  Without a grid every tap is a binary search.  Both paths visit columns in table order and the taps of a
// column in ascending dz, so the result does not depend on the path and is bitwise reproducible (no atomics anywhere).
//
// The weight gradient dW[t][c] = sum_j g[j][c] * feat[row(q_j + off_t)][c] runs per (row chunk, column): every workgroup writes
// a partial slab [T][C] (each tap of each slab exactly once) and a second pass sums the slabs in a fixed order.
#include "pcc_common.h"

static constexpr int CH_MAX_RADIUS = 4;          // kernel_size <= 9: a column's z field is at most 9 bits
static constexpr int CH_MAX_C = 64;
static constexpr int CH_MAX_COLS = 81;
static constexpr int CH_MAX_TAPS = 729;
static constexpr int CH_WG_MAX_BLOCKS = 128;     // row chunks of the weight gradient (partial slabs)

struct ChArgs {
  const long long* keys; int n;                  // input set (canonical)
  const float* feat; int c;                      // [n][c]
  PccGrid g;                                     // g.bits == nullptr: binary search
  int step;                                      // tap pitch (== grid pitch when a grid is given)
  const int* cols; int ncol;                     // [ncol][4]: dx, dy, zmask (bit k <-> dz = k - radius), first
  const int* widx; int ntaps;                    // weight row of the k-th set bit of a column's mask: widx[first + k']
  int radius;
  const long long* q; long long nq;              // query keys
};

// a query decoded once: batch, biased coordinates, and its place in the grid
struct ChQuery {
  long long b;
  int X, Y, Z;                                   // biased 16-bit fields of the key
  int cx, cy, cz;                                // grid cell (grid path)
  int zlo, nz, s;                                // clipped z range of the column fields; s = taps clipped below
  bool any;                                      // false: no tap can hit (other batch, off the lattice, far outside in z)
};

__device__ inline ChQuery ch_query(const ChArgs& a, long long key) {
  ChQuery d;
  d.b = key >> PCC_KEY_B_SHIFT;
  d.X = (int)((key >> PCC_KEY_X_SHIFT) & PCC_KEY_FIELD); d.Y = (int)((key >> PCC_KEY_Y_SHIFT) & PCC_KEY_FIELD); d.Z = (int)(key & PCC_KEY_FIELD);
  d.cx = d.cy = d.cz = 0; d.zlo = 0; d.nz = 0; d.s = 0;
  d.any = true;
  if (a.g.bits) {
    const PccLattice& L = a.g.lat;
    const int x = d.X - (int)PCC_BIAS - L.lo[0], y = d.Y - (int)PCC_BIAS - L.lo[1], z = d.Z - (int)PCC_BIAS - L.lo[2];
    if (d.b >= L.nbatch || ((x | y | z) & ((1 << L.ts_log2) - 1))) { d.any = false; return d; }
    d.cx = x >> L.ts_log2; d.cy = y >> L.ts_log2; d.cz = z >> L.ts_log2;
    const int zlo = max(d.cz - a.radius, 0), zhi = min(d.cz + a.radius, L.dims[2] - 1);
    if (zlo > zhi) { d.any = false; return d; }
    d.zlo = zlo; d.nz = zhi - zlo + 1; d.s = zlo - (d.cz - a.radius);
  }
  return d;
}

// rows of the taps of one (dx, dy) column around a query, in ascending dz: visit(k, row) with k the tap bit (dz = k - radius)
template <typename F>
__device__ inline void ch_column(const ChArgs& a, const ChQuery& d, int dx, int dy, unsigned zm, F&& visit) {
  if (a.g.bits) {
    const int nx = d.cx + dx, ny = d.cy + dy;
    if (nx < 0 || ny < 0 || nx >= a.g.lat.dims[0] || ny >= a.g.lat.dims[1]) return;
    const unsigned tm = (zm >> d.s) & ((1u << d.nz) - 1u);      // taps inside the lattice, in field bits
    if (!tm) return;
    // (spelled out: through pcc_lat_cell these kernels come out with other instructions, tools/kernel_identity.py)
    const long long cell = ((d.b * a.g.lat.dims[0] + nx) * a.g.lat.dims[1] + ny) * (long long)a.g.lat.dims[2] + d.zlo;
    const long long wi = cell >> 6;
    const int sh = (int)(cell & 63);
    const unsigned long long w0 = a.g.bits[wi];
    unsigned long long f64 = w0 >> sh;
    if (sh + d.nz > 64) f64 |= a.g.bits[wi + 1] << (64 - sh);   // (the field's last cell is inside the lattice)
    const unsigned f = (unsigned)f64 & ((1u << d.nz) - 1u);
    unsigned hit = f & tm;
    if (!hit) return;
    const int base = a.g.rank[wi] + __popcll(w0 & ((1ull << sh) - 1ull));
    while (hit) {
      const int t = __ffs((int)hit) - 1;
      hit &= hit - 1;
      visit(t + d.s, base + __popc(f & ((1u << t) - 1u)));
    }
    return;
  }
  const int tx = d.X + dx * a.step, ty = d.Y + dy * a.step;
  if (tx < 0 || ty < 0 || tx > PCC_KEY_FIELD || ty > PCC_KEY_FIELD) return;
  unsigned m = zm;
  while (m) {
    const int k = __ffs((int)m) - 1;
    m &= m - 1;
    const int tz = d.Z + (k - a.radius) * a.step;
    if (tz < 0 || tz > PCC_KEY_FIELD) continue;
    const long long key =
        (d.b << PCC_KEY_B_SHIFT) | ((long long)tx << PCC_KEY_X_SHIFT) | ((long long)ty << PCC_KEY_Y_SHIFT) | (long long)tz;
    const int row = pcc_find((const int64_t*)a.keys, a.n, key);
    if (row >= 0) visit(k, row);
  }
}

// ---- forward: thread per (query, VW channels) ------------------------------------------------------------------------
template <int VW>
__global__ void __launch_bounds__(256) k_chconv_fwd(ChArgs a, const float* __restrict__ w, int wc, float* __restrict__ out) {
  __shared__ int4 s_cols[CH_MAX_COLS];
  __shared__ int s_widx[CH_MAX_TAPS];
  for (int i = threadIdx.x; i < a.ncol; i += blockDim.x) s_cols[i] = ((const int4*)a.cols)[i];
  for (int i = threadIdx.x; i < a.ntaps; i += blockDim.x) s_widx[i] = a.widx[i];
  __syncthreads();
  const int groups = a.c / VW;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.nq * groups) return;
  const long long qi = t / groups;
  const int c0 = (int)(t - qi * groups) * VW;
  const ChQuery d = ch_query(a, a.q[qi]);
  float acc[VW];
#pragma unroll
  for (int v = 0; v < VW; ++v) acc[v] = 0.f;
  if (d.any) {
    for (int i = 0; i < a.ncol; ++i) {
      const int4 cd = s_cols[i];
      const unsigned zm = (unsigned)cd.z;
      ch_column(a, d, cd.x, cd.y, zm, [&](int k, int row) {
        const int wr = s_widx[cd.w + __popc(zm & ((1u << k) - 1u))];
        const float* fp = a.feat + (long long)row * a.c + c0;
        if constexpr (VW == 4) {
          const float4 fv = *(const float4*)fp;
          float4 wv;
          if (wc == 1) { const float s = w[wr]; wv = make_float4(s, s, s, s); }
          else wv = *(const float4*)(w + (long long)wr * wc + c0);
          acc[0] += wv.x * fv.x; acc[1] += wv.y * fv.y; acc[2] += wv.z * fv.z; acc[3] += wv.w * fv.w;
        } else {
          acc[0] += w[(long long)wr * wc + (wc == 1 ? 0 : c0)] * fp[0];
        }
      });
    }
  }
  float* op = out + qi * a.c + c0;
  if constexpr (VW == 4) *(float4*)op = make_float4(acc[0], acc[1], acc[2], acc[3]);
  else op[0] = acc[0];
}

// ---- weight gradient: partial slab per (row chunk, column), then a fixed-order sum ---------------------------------------
// 256 threads = R rows x CP channel lanes (CP = C rounded up to a power of two); every thread keeps the 9 taps of the column
// for its channel over its rows, the R lanes of a channel are summed in order through LDS.
__global__ void __launch_bounds__(256) k_chconv_wgrad(ChArgs a, const float* __restrict__ g, int cp, int nblocks,
                                                      float* __restrict__ partial) {
  __shared__ float s_red[256 * 9];
  const int col = blockIdx.y;
  const int4 cd = ((const int4*)a.cols)[col];
  const unsigned zm = (unsigned)cd.z;
  const int tid = threadIdx.x, ch = tid % cp, r = tid / cp, R = 256 / cp;
  long long per = (a.nq + nblocks - 1) / nblocks;
  const long long lo = (long long)blockIdx.x * per, hi = min(a.nq, lo + per);
  float acc[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = 0.f;
  if (ch < a.c) {
    for (long long j = lo + r; j < hi; j += R) {
      const ChQuery d = ch_query(a, a.q[j]);
      if (!d.any) continue;
      const float gv = g[j * a.c + ch];
      ch_column(a, d, cd.x, cd.y, zm, [&](int k, int row) {
        const float p = gv * a.feat[(long long)row * a.c + ch];
#pragma unroll
        for (int kk = 0; kk < 9; ++kk)
          if (kk == k) acc[kk] += p;
      });
    }
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) s_red[(r * 9 + k) * cp + ch] = acc[k];
  __syncthreads();
  for (int e = tid; e < 9 * cp; e += 256) {
    const int k = e / cp, c = e % cp;
    if (c < a.c && ((zm >> k) & 1u)) {
      float s = 0.f;
      for (int rr = 0; rr < R; ++rr) s += s_red[(rr * 9 + k) * cp + c];
      const int wr = a.widx[cd.w + __popc(zm & ((1u << k) - 1u))];
      partial[((long long)blockIdx.x * a.ntaps + wr) * a.c + c] = s;
    }
  }
}

// dW[t][c] = sum_b partial[b][t][c]  (wc == C);  dW[t] = sum_c sum_b partial[b][t][c]  (wc == 1)
__global__ void k_chconv_wgrad_reduce(const float* __restrict__ partial, int nblocks, int ntaps, int c, int wc,
                                      float* __restrict__ dw) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)ntaps * wc) return;
  const long long slab = (long long)ntaps * c;
  float s = 0.f;
  if (wc == 1) {
    for (int ch = 0; ch < c; ++ch)
      for (int b = 0; b < nblocks; ++b) s += partial[b * slab + i * c + ch];
  } else {
    for (int b = 0; b < nblocks; ++b) s += partial[b * slab + i];
  }
  dw[i] = s;
}

// ---- host side ---------------------------------------------------------------------------------------------------------
static int ch_args(ChArgs& a, const int64_t* keys, int64_t n, const float* feat, int32_t c, const uint64_t* grid_bits,
                   const int32_t* grid_rank, const int32_t* h_grid, int32_t step, const int32_t* cols, int32_t ncol,
                   const int32_t* widx, int32_t ntaps, int32_t kernel_size, const int64_t* query_keys, int64_t nq,
                   const char* who) {
  a = ChArgs();
  PCC_REQUIRE(pcc_chconv_supported(kernel_size, c), "%s: kernel_size %d / channels %d unsupported (odd kernel_size <= 9, 1 <= C <= 64)",
              who, kernel_size, c);
  PCC_REQUIRE(ncol >= 1 && ncol <= kernel_size * kernel_size && ntaps >= 1 && ntaps <= kernel_size * kernel_size * kernel_size,
              "%s: %d columns / %d taps do not fit kernel_size %d", who, ncol, ntaps, kernel_size);
  PCC_REQUIRE(pcc_is_pow2(step), "%s: step %d is not a power of two", who, step);
  PCC_REQUIRE(cols && widx && (nq == 0 || query_keys) && (n == 0 || (keys && feat)), "%s: NULL array", who);
  PCC_REQUIRE(n < (1ll << 31) && nq < (1ll << 40), "%s: too many rows", who);
  PCC_TRY(pcc_grid_from_host(grid_bits, grid_rank, h_grid, who, &a.g));
  PCC_REQUIRE(!grid_bits || h_grid[6] == step, "%s: grid pitch %d differs from the tap step %d", who, h_grid[6], step);
  a.keys = (const long long*)keys; a.n = (int)n; a.feat = feat; a.c = c; a.step = step;
  a.cols = cols; a.ncol = ncol; a.widx = widx; a.ntaps = ntaps; a.radius = kernel_size / 2;
  a.q = (const long long*)query_keys; a.nq = nq;
  return PCC_OK;
}

static bool ch_aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

extern "C" int pcc_chconv_supported(int32_t kernel_size, int32_t c) {
  return kernel_size >= 1 && kernel_size <= 2 * CH_MAX_RADIUS + 1 && (kernel_size & 1) && c >= 1 && c <= CH_MAX_C;
}

extern "C" int pcc_chconv_fwd(const int64_t* keys, int64_t n, const float* feat, int32_t c, const uint64_t* grid_bits,
                              const int32_t* grid_rank, const int32_t* h_grid, int32_t step, const int32_t* cols, int32_t ncol,
                              const int32_t* widx, int32_t ntaps, int32_t kernel_size, const float* w, int32_t wc,
                              const int64_t* query_keys, int64_t nq, float* out, void* stream) {
  ChArgs a;
  PCC_TRY(ch_args(a, keys, n, feat, c, grid_bits, grid_rank, h_grid, step, cols, ncol, widx, ntaps, kernel_size, query_keys, nq,
                  "pcc_chconv_fwd"));
  PCC_REQUIRE(w && (wc == 1 || wc == c), "pcc_chconv_fwd: weights must be [T][C] or [T][1]");
  if (nq <= 0) return PCC_OK;
  PCC_REQUIRE(out, "pcc_chconv_fwd: NULL output");
  hipStream_t s = (hipStream_t)stream;
  const bool v4 = c % 4 == 0 && ch_aligned16(feat) && ch_aligned16(out) && (wc == 1 || ch_aligned16(w));
  const long long threads = nq * (v4 ? c / 4 : c);
  if (v4) k_chconv_fwd<4><<<(unsigned)pcc_cdiv(threads, 256), 256, 0, s>>>(a, w, wc, out);
  else k_chconv_fwd<1><<<(unsigned)pcc_cdiv(threads, 256), 256, 0, s>>>(a, w, wc, out);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

static int ch_wgrad_blocks(int64_t nq) {
  int64_t b = pcc_cdiv(nq, 2048);
  if (b < 1) b = 1;
  if (b > CH_WG_MAX_BLOCKS) b = CH_WG_MAX_BLOCKS;
  return (int)b;
}

extern "C" size_t pcc_chconv_wgrad_ws_bytes(int64_t nq, int32_t ntaps, int32_t c) {
  return (size_t)ch_wgrad_blocks(nq) * (size_t)ntaps * (size_t)c * sizeof(float) + 256;
}

extern "C" int pcc_chconv_wgrad(const int64_t* keys, int64_t n, const float* feat, int32_t c, const uint64_t* grid_bits,
                                const int32_t* grid_rank, const int32_t* h_grid, int32_t step, const int32_t* cols, int32_t ncol,
                                const int32_t* widx, int32_t ntaps, int32_t kernel_size, const int64_t* query_keys, int64_t nq,
                                const float* grad_out, float* dw, int32_t wc, void* ws, size_t ws_bytes, void* stream) {
  ChArgs a;
  PCC_TRY(ch_args(a, keys, n, feat, c, grid_bits, grid_rank, h_grid, step, cols, ncol, widx, ntaps, kernel_size, query_keys, nq,
                  "pcc_chconv_wgrad"));
  PCC_REQUIRE(dw && (wc == 1 || wc == c), "pcc_chconv_wgrad: dW must be [T][C] or [T][1]");
  hipStream_t s = (hipStream_t)stream;
  if (nq <= 0) {
    PCC_CHECK_HIP(hipMemsetAsync(dw, 0, (size_t)ntaps * wc * sizeof(float), s));
    return PCC_OK;
  }
  PCC_REQUIRE(grad_out && ws, "pcc_chconv_wgrad: NULL array");
  if (ws_bytes < pcc_chconv_wgrad_ws_bytes(nq, ntaps, c)) {
    pcc_set_error("pcc_chconv_wgrad: workspace too small");
    return PCC_EWS;
  }
  int cp = 1;
  while (cp < c) cp <<= 1;
  const int nblocks = ch_wgrad_blocks(nq);
  float* partial = (float*)ws;
  k_chconv_wgrad<<<dim3((unsigned)nblocks, (unsigned)ncol), 256, 0, s>>>(a, grad_out, cp, nblocks, partial);
  PCC_LAUNCH_CHECK();
  k_chconv_wgrad_reduce<<<(unsigned)pcc_cdiv((long long)ntaps * wc, 256), 256, 0, s>>>(partial, nblocks, ntaps, c, wc, dw);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}
