// Narrow outputs: the VALU kernels for cout <= 4 (direct, two-pass project + gather, and the grid-indexed forms of the heads) and the
// wave-autonomous 16x16x4 MFMA kernels for 4 < cout <= 16 with the band-tile table and the fused occupancy head.
// pcc_conv_fwd (pcc_conv.hip) reaches them through launch_conv_wave16 / launch_conv_thin_t / launch_conv_thin; the head, band-tile
// and grid entry points are called from the Python side.
//
// Thin outputs (Cout <= 4: occupancy logits, colours, model/transforms.py:141-160) are gather-bound;
// they use a VALU kernel with lanes spread over the input channels of a row.
#include "pcc_conv.h"

// ------------------------------------------------------------------------------------------
// thin outputs (cout <= 4) or channel counts the MFMA tiling does not take: VALU, gather-bound.
// Wt layout [K][cout][cin].  LPR lanes share one output position.
// ------------------------------------------------------------------------------------------
struct ThinArgs {
  const float* feat; const float* wt; const float* bias;
  const int* hdr; const int* nbr; const int* rows;
  float* out; long long n_out; int cin, cout, act; float slope; int lpr_log2;
};

// LPR lanes share one output position, each lane owns VEC consecutive input channels per pass.  Offsets are
// processed in batches of JB with all neighbour-index loads, then all feature loads, issued back to back
// (memory-level parallelism instead of a dependent chain per offset).
template <int COUT_MAX, int VEC>
__global__ void __launch_bounds__(256) k_conv_thin(ThinArgs a) {
  typedef typename ThinVec<VEC>::T VT;
  constexpr int JB = 9;
  const int lane = threadIdx.x & 63;
  const int lpr = 1 << a.lpr_log2;
  const int rpw = 64 >> a.lpr_log2;                       // rows per wave
  const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long long p = wave * rpw + (lane >> a.lpr_log2);  // position handled by my lane group
  const int cl = lane & (lpr - 1);
  const bool valid = p < a.n_out;
  const int cvec = a.cin / VEC;                           // vectors per row

  int k_count = 1, koff_begin = 0;
  long long seg_pos_count = a.n_out, local = p;
  const int* seg_nbr = nullptr;
  const bool identity = (a.hdr == nullptr);
  if (!identity && valid) {
    const int nseg = a.hdr[HDR_NSEG];
    int s = 0;
    for (; s < nseg - 1; ++s) {
      const int* sg = a.hdr + HDR_SEG0 + s * SEG_WORDS;
      if (p < (long long)sg[SEG_POS_BEGIN] + sg[SEG_POS_COUNT]) break;
    }
    const int* sg = a.hdr + HDR_SEG0 + s * SEG_WORDS;
    k_count = sg[SEG_K_COUNT];
    koff_begin = sg[SEG_KOFF_BEGIN];
    seg_pos_count = sg[SEG_POS_COUNT];
    local = p - sg[SEG_POS_BEGIN];
    seg_nbr = a.nbr + (((long long)(unsigned)sg[SEG_NBR_LO]) | ((long long)sg[SEG_NBR_HI] << 32));
  }
  float acc[COUT_MAX];
#pragma unroll
  for (int o = 0; o < COUT_MAX; ++o) acc[o] = 0.f;
  if (valid) {
    for (int cv = cl; cv < cvec; cv += lpr) {
      for (int j0 = 0; j0 < k_count; j0 += JB) {
        int ir[JB];
#pragma unroll
        for (int u = 0; u < JB; ++u) {
          const int j = j0 + u;
          ir[u] = (j < k_count) ? (identity ? (int)p : seg_nbr[(long long)j * seg_pos_count + local]) : -1;
        }
        VT x[JB];
#pragma unroll
        for (int u = 0; u < JB; ++u) {
          thin_zero(x[u]);
          if (ir[u] >= 0) x[u] = reinterpret_cast<const VT*>(a.feat + (long long)ir[u] * a.cin)[cv];
        }
#pragma unroll
        for (int u = 0; u < JB; ++u) {
          const int j = j0 + u;
          if (j < k_count) {
            const int kid = identity ? 0 : a.hdr[HDR_KOFFS + koff_begin + j];
            const float* wk = a.wt + (long long)kid * a.cout * a.cin;
#pragma unroll
            for (int o = 0; o < COUT_MAX; ++o)
              if (o < a.cout) acc[o] += thin_dot(x[u], reinterpret_cast<const VT*>(wk + o * a.cin)[cv]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int o = 0; o < COUT_MAX; ++o)
    for (int d = lpr >> 1; d >= 1; d >>= 1) acc[o] += __shfl_xor(acc[o], d);
  if (valid && cl == 0) {
    const long long orow = a.rows ? a.rows[p] : p;
#pragma unroll
    for (int o = 0; o < COUT_MAX; ++o) {
      if (o >= a.cout) break;
      float v = acc[o] + (a.bias ? a.bias[o] : 0.f);
      if (a.act == PCC_ACT_RELU) v = fmaxf(v, 0.f);
      else if (a.act == PCC_ACT_LEAKY) v = v >= 0.f ? v : v * a.slope;
      a.out[orow * a.cout + o] = v;
    }
  }
}

// ------------------------------------------------------------------------------------------
// Thin outputs, two-pass form (cout <= 4, cin <= 64):  out[o] = b + sum_k  <feat[nbr_k(o)], w_k>
//   pass 1  t[k*cout+co][i] = <feat[i], w_k[co]>      per input row, features read ONCE, coalesced writes
//   pass 2  out[o][co]      = b + sum_k t[k*cout+co][nbr_k(o)]   scalar gathers, near-contiguous per offset
// 16x (cin=16) to 64x (cin=64) fewer gathered bytes than fetching whole neighbour rows per offset.
// ------------------------------------------------------------------------------------------
template <int CIN>
__global__ void __launch_bounds__(256) k_thin_project(const float* __restrict__ feat, long long n_in,
                                                      const float* __restrict__ wt, int kc, float* __restrict__ t) {
  extern __shared__ __attribute__((aligned(16))) float w_s[];
  for (int i = threadIdx.x; i < kc * CIN; i += 256) w_s[i] = wt[i];
  __syncthreads();
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_in) return;
  float4 x[CIN / 4];
#pragma unroll
  for (int c = 0; c < CIN / 4; ++c) x[c] = reinterpret_cast<const float4*>(feat + i * CIN)[c];
  for (int k = 0; k < kc; ++k) {
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < CIN / 4; ++c) {
      const float4 w = reinterpret_cast<const float4*>(w_s + k * CIN)[c];   // wave-uniform address: LDS broadcast
      acc += x[c].x * w.x + x[c].y * w.y + x[c].z * w.z + x[c].w * w.w;
    }
    t[(long long)k * n_in + i] = acc;
  }
}

struct ThinGatherArgs {
  const float* t; const float* bias; const int* hdr; const int* nbr; const int* rows;
  float* out; long long n_in, n_out; int cout, act; float slope;
};

template <int COUT_MAX>
__global__ void __launch_bounds__(256) k_thin_gather(ThinGatherArgs a) {
  constexpr int JB = 9;
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.n_out) return;
  int k_count = 1, koff_begin = 0;
  long long spc = a.n_out, local = p;
  const int* seg_nbr = nullptr;
  const bool identity = (a.hdr == nullptr);
  if (!identity) {
    const int nseg = a.hdr[HDR_NSEG];
    int s = 0;
    for (; s < nseg - 1; ++s) {
      const int* sg = a.hdr + HDR_SEG0 + s * SEG_WORDS;
      if (p < (long long)sg[SEG_POS_BEGIN] + sg[SEG_POS_COUNT]) break;
    }
    const int* sg = a.hdr + HDR_SEG0 + s * SEG_WORDS;
    k_count = sg[SEG_K_COUNT]; koff_begin = sg[SEG_KOFF_BEGIN]; spc = sg[SEG_POS_COUNT];
    local = p - sg[SEG_POS_BEGIN];
    seg_nbr = a.nbr + (((long long)(unsigned)sg[SEG_NBR_LO]) | ((long long)sg[SEG_NBR_HI] << 32));
  }
  float acc[COUT_MAX];
#pragma unroll
  for (int o = 0; o < COUT_MAX; ++o) acc[o] = 0.f;
  for (int j0 = 0; j0 < k_count; j0 += JB) {
    int ir[JB];
#pragma unroll
    for (int u = 0; u < JB; ++u)
      ir[u] = (j0 + u < k_count) ? (identity ? (int)p : seg_nbr[(long long)(j0 + u) * spc + local]) : -1;
    float v[JB][COUT_MAX];
#pragma unroll
    for (int u = 0; u < JB; ++u) {
      const int kid = (ir[u] >= 0 && !identity) ? a.hdr[HDR_KOFFS + koff_begin + j0 + u] : 0;
#pragma unroll
      for (int o = 0; o < COUT_MAX; ++o)
        v[u][o] = (ir[u] >= 0 && o < a.cout) ? a.t[(long long)(kid * a.cout + o) * a.n_in + ir[u]] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < JB; ++u)
#pragma unroll
      for (int o = 0; o < COUT_MAX; ++o) acc[o] += v[u][o];
  }
  const long long orow = a.rows ? a.rows[p] : p;
#pragma unroll
  for (int o = 0; o < COUT_MAX; ++o)
    if (o < a.cout) a.out[orow * a.cout + o] = act1(acc[o] + (a.bias ? a.bias[o] : 0.f), a.act, a.slope);
}

// ------------------------------------------------------------------------------------------
// Narrow outputs with weights that fit LDS (4 < cout <= 16, cin in {16,32,64}): wave-autonomous kernel on
// v_mfma_f32_16x16x4_f32.  All K weight slices sit in LDS for the whole (persistent) workgroup; each wave owns
// 32 positions (two 16-row MFMA tiles), reads the neighbour rows straight from global memory into the MFMA A
// layout (lane = row, 16-byte k-quads) and never meets a workgroup barrier in its main loop.  No padding to a
// 32-wide column tile, offsets with no neighbour in the wave's 32 rows are skipped by ballot.
// ------------------------------------------------------------------------------------------

struct Wave16Args {
  const float* feat; const float* wl; const float* bias; const int* hdr; const int* nbr; const int* rows;
  float* out; long long n_out, n_in; int K, cout, act; float slope;
  // z-run kernel only: optional tile table (band order, pcc_band_tiles_build) and the fused 16 -> 1 head projection
  const int* tiles = nullptr; const int* n_tiles = nullptr;
  const float* w2 = nullptr;      // [27][cout] second convolution of an occupancy head (thin layout), PROJ variant
  float* t = nullptr;             // [27][n_out] projections t[k][i] = <relu(h_i), w2_k>, PROJ variant
};

// LDS image of the narrow-output weights: [K][CIN/4][16][4] -- k-quad major, then the 16 output columns, 4 channels
// each.  A ds_read_b128 is served in groups of 16 lanes and every group holds each column r16 exactly once (lanes
// {0-3,12-15,20-27}, ... of MI355X_MICROARCH.md's LDS table), so with the column as the fastest 16-byte index the 16
// lanes of a group always hit 16 different bank quads: conflict-free.  (The round-1 layout [K][16][CIN+4] put the
// k-quad in the low address bits: SQ_LDS_BANK_CONFLICT = 1/2 SQ_LDS_IDX_ACTIVE, profiles/r01_sq_counters_conv.txt.)
template <int CIN>
__device__ __forceinline__ const float* wave16_w(const float* wl_s, int kid, int kq, int r16) {
  return wl_s + ((kid * (CIN / 4) + kq) * 16 + r16) * 4;
}

template <int CIN>
__global__ void __launch_bounds__(512) k_conv_wave16(Wave16Args a) {
  constexpr int G = CIN / 16;
  constexpr int NW = 8;                                            // waves per workgroup
  extern __shared__ __attribute__((aligned(16))) float wl_s[];   // [K][CIN/4][16][4]
  for (int i = threadIdx.x; i < a.K * 16 * (CIN / 4); i += 512)
    reinterpret_cast<float4*>(wl_s)[i] = reinterpret_cast<const float4*>(a.wl)[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, r16 = lane & 15, q = lane >> 4;
  const bool identity = (a.hdr == nullptr);
  const int nseg = identity ? 1 : a.hdr[HDR_NSEG];
  long long total_tiles = 0;
  if (identity) total_tiles = (a.n_out + 31) / 32;
  else
    for (int s = 0; s < nseg; ++s) total_tiles += (a.hdr[HDR_SEG0 + s * SEG_WORDS + SEG_POS_COUNT] + 31) / 32;

  // XCD x sweeps its own contiguous eighth of the tiles with all of its waves side by side (L2 locality of the gathers)
  const int cpx = gridDim.x >> 3;                                   // workgroups per XCD (grid is a multiple of 8)
  const long long per_xcd = (total_tiles + 7) / 8;
  const long long xcd_lo = (long long)(blockIdx.x & 7) * per_xcd;
  const long long xcd_hi = min(total_tiles, xcd_lo + per_xcd);
  for (long long wt = xcd_lo + (long long)(blockIdx.x >> 3) * NW + (threadIdx.x >> 6); wt < xcd_hi;
       wt += (long long)cpx * NW) {
    long long pos0, spc;
    int npos, k_count = 1, koff_begin = 0;
    const int* seg_nbr = nullptr;
    if (identity) {
      pos0 = wt * 32; npos = (int)min(32ll, a.n_out - pos0); spc = a.n_out;
    } else {
      long long tile = wt;
      int s = 0;
      for (; s < nseg - 1; ++s) {
        const long long tiles = (a.hdr[HDR_SEG0 + s * SEG_WORDS + SEG_POS_COUNT] + 31) / 32;
        if (tile < tiles) break;
        tile -= tiles;
      }
      const int* sg = a.hdr + HDR_SEG0 + s * SEG_WORDS;
      k_count = sg[SEG_K_COUNT]; koff_begin = sg[SEG_KOFF_BEGIN]; spc = sg[SEG_POS_COUNT];
      const long long local0 = tile * 32;
      pos0 = sg[SEG_POS_BEGIN] + local0;
      npos = (int)min(32ll, spc - local0);
      seg_nbr = a.nbr + (((long long)(unsigned)sg[SEG_NBR_LO]) | ((long long)sg[SEG_NBR_HI] << 32)) + local0;
    }
    const bool vA = r16 < npos, vB = 16 + r16 < npos;
    f32x4 accA0 = {0.f, 0.f, 0.f, 0.f}, accA1 = accA0, accB0 = accA0, accB1 = accA0;
    auto fetch = [&](int j, int& iA, int& iB) {     // natural slot order: no dependent table read ahead of the index load
      iA = -1; iB = -1;
      if (j < k_count) {
        if (vA) iA = identity ? (int)(pos0 + r16) : seg_nbr[(long long)j * spc + r16];
        if (vB) iB = identity ? (int)(pos0 + 16 + r16) : seg_nbr[(long long)j * spc + 16 + r16];
      }
    };
    auto gather = [&](int iA, int iB, float4 (&xa)[G], float4 (&xb)[G]) {
#pragma unroll
      for (int g = 0; g < G; ++g) {
        xa[g] = make_float4(0.f, 0.f, 0.f, 0.f);
        xb[g] = xa[g];
        if (iA >= 0) xa[g] = *reinterpret_cast<const float4*>(a.feat + (long long)iA * CIN + 16 * g + 4 * q);
        if (iB >= 0) xb[g] = *reinterpret_cast<const float4*>(a.feat + (long long)iB * CIN + 16 * g + 4 * q);
      }
    };
    // three-stage pipeline per wave: indices of offset j+2, feature rows of offset j+1, MFMAs of offset j
    int iA0, iB0, iA1, iB1, iA2, iB2;
    float4 xa[G], xb[G], ya[G], yb[G];
    fetch(0, iA0, iB0);
    fetch(1, iA1, iB1);
    gather(iA0, iB0, xa, xb);
    for (int j = 0; j < k_count; ++j) {
      fetch(j + 2, iA2, iB2);
      gather(iA1, iB1, ya, yb);
      if (__ballot(iA0 >= 0 || iB0 >= 0)) {
        const int kid = identity ? 0 : a.hdr[HDR_KOFFS + koff_begin + j];
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const float4 w = *reinterpret_cast<const float4*>(wave16_w<CIN>(wl_s, kid, 4 * g + q, r16));
          accA0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[g].x, w.x, accA0, 0, 0, 0);
          accB0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xb[g].x, w.x, accB0, 0, 0, 0);
          accA1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[g].y, w.y, accA1, 0, 0, 0);
          accB1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xb[g].y, w.y, accB1, 0, 0, 0);
          accA0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[g].z, w.z, accA0, 0, 0, 0);
          accB0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xb[g].z, w.z, accB0, 0, 0, 0);
          accA1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[g].w, w.w, accA1, 0, 0, 0);
          accB1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xb[g].w, w.w, accB1, 0, 0, 0);
        }
      }
#pragma unroll
      for (int g = 0; g < G; ++g) { xa[g] = ya[g]; xb[g] = yb[g]; }
      iA0 = iA1; iB0 = iB1; iA1 = iA2; iB1 = iB2;
    }
    // D layout: col = lane & 15, row = 4 * (lane >> 4) + reg
    if (r16 < a.cout) {
      const float b = a.bias ? a.bias[r16] : 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int rA = 4 * q + e, rB = 16 + 4 * q + e;
        if (rA < npos) {
          const long long orow = a.rows ? a.rows[pos0 + rA] : pos0 + rA;
          a.out[orow * a.cout + r16] = act1(accA0[e] + accA1[e] + b, a.act, a.slope);
        }
        if (rB < npos) {
          const long long orow = a.rows ? a.rows[pos0 + rB] : pos0 + rB;
          a.out[orow * a.cout + r16] = act1(accB0[e] + accB1[e] + b, a.act, a.slope);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// k_conv_wave16 for 3x3x3 conv maps in canonical row order (one segment, all 27 offsets, no row list), with z-run
// reuse.  Rows are sorted with z fastest, so the dz = -1 / +1 neighbour of row r under offset (dx, dy) is, inside a
// z-run, the dz = 0 neighbour of row r -/+ 1: the lane next door already holds it.  Per (dx, dy) group a wave gathers
// the dz = 0 rows of its 16 positions once, takes the dz = -+1 operands from the adjacent lane (DPP row shift, guarded
// by index equality, so any geometry is handled) and points the loads of everything it does not need at one shared
// zero row (an L1 hit), which also removes every per-row validity branch.  PMC on the first version showed 7 VALU
// instructions per MFMA competing for the SIMD; this one is written for instruction count: 32-bit offsets, no
// identity / segment generality, tail rows clamped instead of predicated.
// ------------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true); }
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
static constexpr int DPP_SHL1 = 0x101, DPP_SHR1 = 0x111;

template <int CIN, bool PROJ>
__global__ void __launch_bounds__(512) k_conv_wave16z(Wave16Args a) {
  constexpr int G = CIN / 16;
  constexpr int NW = 8;
  extern __shared__ __attribute__((aligned(16))) float wl_s[];   // [27][CIN/4][16][4] (+ PROJ: per-wave 16x17 scratch)
  for (int i = threadIdx.x; i < 27 * 16 * (CIN / 4); i += 512)
    reinterpret_cast<float4*>(wl_s)[i] = reinterpret_cast<const float4*>(a.wl)[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, r16 = lane & 15, q = lane >> 4;
  const unsigned spc = (unsigned)a.n_out;                          // one segment: positions = output rows
  // tiles of <= 16 consecutive rows: plain 16-row cuts, or the band-ordered table of pcc_band_tiles_build (rows of one
  // (x, y-band) run per tile, bands outermost: the dx = +-1 neighbours of a band's current x-slab then stay in the
  // XCD's L2 until that slab is processed itself)
  const unsigned total_tiles = a.tiles ? (unsigned)*a.n_tiles : (spc + 15) / 16;
  const unsigned cpx = gridDim.x >> 3;
  const unsigned per_xcd = (total_tiles + 7) / 8;
  const unsigned xcd_lo = (blockIdx.x & 7) * per_xcd;
  const unsigned xcd_hi = min(total_tiles, xcd_lo + per_xcd);
  const float* wl_lane = wl_s + r16 * 4 + q * 64;                  // wave16_w(kid, 4g+q, r16) = wl_lane + (kid*(CIN/4) + 4g) * 64

  // PROJ: B operand of the head's second convolution, out[o] = b2 + sum_k <relu(h[nbr_k(o)]), w2_k>, evaluated as
  // t[k][i] = <relu(h_i), w2_k> for the tile in registers (one more 16x16x4 MFMA block), so h never goes to memory
  float w2r[2][4];
  float* hs = nullptr;
  if constexpr (PROJ) {
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = 16 * nt + r16, c = 4 * j + q;
        w2r[nt][j] = (k < 27 && c < a.cout) ? a.w2[k * a.cout + c] : 0.f;
      }
    hs = wl_s + 27 * 16 * CIN + (threadIdx.x >> 6) * (16 * 17);
  }

  // One (dx,dy) group of a 16-row tile: the dz=0 rows, and the dz=-+1 rows, each either the neighbouring lane's dz=0
  // row (mask k*) or loaded.  All rows come through buffer loads whose offset is out of range for an absent or
  // not-needed row: those lanes read 0 without touching memory, the number of loads in flight is fixed (exact
  // s_waitcnt distances; conditional loads made the compiler wait for the prefetch itself), and no branch is left.
  struct Grp { float4 c[G], m[G], p[G]; unsigned km, kp; };
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.feat), (short)0, (int)(unsigned)((size_t)a.n_in * CIN * 4), 0x00020000);
  constexpr unsigned OOB = 0xFFFFFF00u;

  for (unsigned wt = xcd_lo + (blockIdx.x >> 3) * NW + (threadIdx.x >> 6); wt < xcd_hi; wt += cpx * NW) {
    unsigned pos0, npos;
    if (a.tiles) {
      const unsigned tw = (unsigned)a.tiles[wt];
      pos0 = tw & 0x07FFFFFFu; npos = (tw >> 27) + 1;
    } else {
      pos0 = wt * 16; npos = min(16u, spc - pos0);
    }
    const unsigned r = pos0 + min((unsigned)r16, npos - 1);        // tail rows repeat the tile's last row, never stored
    const int* nb = a.nbr + r;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0, acc2 = acc0, acc3 = acc0;

    auto issue = [&](int im, int ic, int ip, Grp& x) {
      const int cm = dpp_i<DPP_SHR1>(ic), cp = dpp_i<DPP_SHL1>(ic);
      const bool mm = im >= 0 && im == cm && r16 != 0;
      const bool mp = ip >= 0 && ip == cp && r16 != 15;
      x.km = mm ? 0xFFFFFFFFu : 0u;
      x.kp = mp ? 0xFFFFFFFFu : 0u;
      asm volatile("" : "+v"(x.km), "+v"(x.kp));       // opaque: keeps (shifted & k) | loaded as one v_and_or_b32
      const unsigned oc = ic >= 0 ? (unsigned)ic * (CIN * 4) + 16 * q : OOB;
      const unsigned om = (im >= 0 && !mm) ? (unsigned)im * (CIN * 4) + 16 * q : OOB;
      const unsigned op = (ip >= 0 && !mp) ? (unsigned)ip * (CIN * 4) + 16 * q : OOB;
#pragma unroll
      for (int g = 0; g < G; ++g) {
        x.c[g] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rs, oc + 64 * g, 0, 0));
        x.m[g] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rs, om + 64 * g, 0, 0));
        x.p[g] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rs, op + 64 * g, 0, 0));
      }
    };
    auto mfma4 = [&](const float4& x, int slot, int g) {
      const float4 w = *reinterpret_cast<const float4*>(wl_lane + (slot * (CIN / 4) + 4 * g) * 64);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.x, w.x, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.y, w.y, acc1, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.z, w.z, acc2, 0, 0, 0);
      acc3 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.w, w.w, acc3, 0, 0, 0);
    };
    auto mix = [](unsigned k, float shifted, float loaded) {   // (shifted & k) | loaded: loaded is 0 wherever k is set
      return __builtin_bit_cast(float, (__builtin_bit_cast(unsigned, shifted) & k) | __builtin_bit_cast(unsigned, loaded));
    };

    // pipeline per wave: indices of group g9+2, feature rows of group g9+1, MFMAs of group g9
    int im1 = nb[spc], ic1 = nb[10ull * spc], ip1 = nb[19ull * spc];                 // group 1
    Grp x, y;
    issue(nb[0], nb[9ull * spc], nb[18ull * spc], x);                                // group 0
    auto compute = [&](const Grp& x, int g9) {
#pragma unroll
      for (int g = 0; g < G; ++g) {
        float4 vm, vp;
        vm.x = mix(x.km, dpp_f<DPP_SHR1>(x.c[g].x), x.m[g].x);  vp.x = mix(x.kp, dpp_f<DPP_SHL1>(x.c[g].x), x.p[g].x);
        vm.y = mix(x.km, dpp_f<DPP_SHR1>(x.c[g].y), x.m[g].y);  vp.y = mix(x.kp, dpp_f<DPP_SHL1>(x.c[g].y), x.p[g].y);
        vm.z = mix(x.km, dpp_f<DPP_SHR1>(x.c[g].z), x.m[g].z);  vp.z = mix(x.kp, dpp_f<DPP_SHL1>(x.c[g].z), x.p[g].z);
        vm.w = mix(x.km, dpp_f<DPP_SHR1>(x.c[g].w), x.m[g].w);  vp.w = mix(x.kp, dpp_f<DPP_SHL1>(x.c[g].w), x.p[g].w);
        mfma4(vm, g9, g);
        mfma4(x.c[g], g9 + 9, g);
        mfma4(vp, g9 + 18, g);
      }
    };
    // two groups per trip, the buffers swapping roles, so that no register copy ties this group's MFMAs to the
    // loads just issued for the next one (a copy made the compiler wait for them: no overlap at all)
    // (sched_barrier: the machine scheduler otherwise sinks the prefetch loads next to their first use)
#pragma unroll 1
    for (int g9 = 0; g9 < 8; g9 += 2) {
      const unsigned ga = (unsigned)(g9 + 2), gb = (unsigned)min(g9 + 3, 8);
      const int am = nb[(size_t)ga * spc], ac = nb[(size_t)(ga + 9) * spc], ap = nb[(size_t)(ga + 18) * spc];
      issue(im1, ic1, ip1, y);                                                       // group g9+1
      __builtin_amdgcn_sched_barrier(0);
      compute(x, g9);
      __builtin_amdgcn_sched_barrier(0);
      const int bm = nb[(size_t)gb * spc], bc = nb[(size_t)(gb + 9) * spc], bp = nb[(size_t)(gb + 18) * spc];
      issue(am, ac, ap, x);                                                          // group g9+2
      __builtin_amdgcn_sched_barrier(0);
      compute(y, g9 + 1);
      __builtin_amdgcn_sched_barrier(0);
      im1 = bm; ic1 = bc; ip1 = bp;
    }
    compute(x, 8);
    // D layout: col = lane & 15, row = 4 * (lane >> 4) + reg
    const float b = (a.bias && r16 < a.cout) ? a.bias[r16] : 0.f;
    if constexpr (!PROJ) {
      if (r16 < a.cout) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const unsigned lr = 4 * q + e;
          if (lr < npos) a.out[(size_t)(pos0 + lr) * a.cout + r16] = act1(acc0[e] + acc1[e] + acc2[e] + acc3[e] + b, a.act, a.slope);
        }
      }
    } else {
      // h tile (activation applied) -> per-wave LDS scratch [row][17] -> A operand (lane = row, k = channel quad)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        hs[(4 * q + e) * 17 + r16] = r16 < a.cout ? act1(acc0[e] + acc1[e] + acc2[e] + acc3[e] + b, a.act, a.slope) : 0.f;
      __builtin_amdgcn_wave_barrier();      // same wave writes and reads: LDS executes a wave's operations in order
      f32x4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = d0;
      // t^T tile = W2 (A: lane = offset, k = channel quad) x h^T (B: lane = row): rows end up across the lanes, so each
      // store instruction writes four 64-byte runs of consecutive rows instead of 64 scattered words
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float hv = hs[r16 * 17 + 4 * j + q];
        d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w2r[0][j], hv, d0, 0, 0, 0);
        d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w2r[1][j], hv, d1, 0, 0, 0);
      }
      __builtin_amdgcn_wave_barrier();      // the next tile's scratch writes stay behind these reads
      // D: lane (row = r16, q) holds t[k = 4q+e (+16)][row]
      if ((unsigned)r16 < npos) {
        float* tp = a.t + (size_t)(4 * q) * spc + pos0 + r16;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          tp[(size_t)e * spc] = d0[e];
          if (16 + 4 * q + e < 27) tp[(size_t)(16 + e) * spc] = d1[e];
        }
      }
    }
  }
}

static bool g_wave16_zrun = getenv("PCC_WAVE16_ZRUN") ? atoi(getenv("PCC_WAVE16_ZRUN")) != 0 : true;

template <int CIN>
static int launch_wave16(const Wave16Args& a, hipStream_t s) {
  const size_t lds = (size_t)a.K * 16 * CIN * sizeof(float);
  int dev = 0;
  PCC_CHECK_HIP(hipGetDevice(&dev));
  static unsigned long long attr_set = 0;                         // one bit per device (hipFuncSetAttribute is per device)
  if (!(attr_set >> (dev & 63) & 1ull)) {
    PCC_CHECK_HIP(hipFuncSetAttribute((const void*)k_conv_wave16<CIN>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
    PCC_CHECK_HIP(hipFuncSetAttribute((const void*)k_conv_wave16z<CIN, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
    PCC_CHECK_HIP(hipFuncSetAttribute((const void*)k_conv_wave16z<CIN, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
    attr_set |= 1ull << (dev & 63);
  }
  prof_note(PCC_FORM_WAVE16, 0.0, 0.0);
  prof_tile(32, 16, 1);
  const long long tiles = pcc_cdiv(a.n_out, 32) + (a.rows ? PCC_MAP_MAX_SEG : 0);
  long long want = pcc_cdiv(tiles, 8);
  want = (want + 7) / 8 * 8;                                     // multiple of 8: one contiguous tile range per XCD
  const unsigned grid = (unsigned)(want < 512 ? want : 512);     // persistent: 2 workgroups (16 waves) per CU re-use the LDS weights
  // 3x3x3 conv map in canonical row order (k_map_conv: one segment, all 27 offsets, no row list): z-run reuse variant
  if (g_wave16_zrun && a.K == 27 && a.hdr && !a.rows && a.n_out * 27 < (1ll << 31) &&
      a.n_in * CIN * 4 <= 0xFFFFFE00ll) {                          // 32-bit buffer offsets
    if (a.t) k_conv_wave16z<CIN, true><<<grid, 512, lds + 8 * 16 * 17 * sizeof(float), s>>>(a);
    else k_conv_wave16z<CIN, false><<<grid, 512, lds, s>>>(a);
    PCC_LAUNCH_CHECK();
    return PCC_OK;
  }
  PCC_REQUIRE(!a.t, "pcc_conv_head_fwd: the fused head needs a canonical 3x3x3 map (one segment, no row list)");
  k_conv_wave16<CIN><<<grid, 512, lds, s>>>(a);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

// The same projections on the matrix pipe, for wide inputs (cin 32 / 64) and at most 32 projections (the one-channel heads:
// 27): t^T = W2 x^T as v_mfma_f32_32x32x2_f32 with the WEIGHTS as the A operand (its 32 rows = the projections k) and 32 feature
// rows as the B operand (its 32 columns), so that an accumulator register holds t[k][32 consecutive rows] across the lanes of a
// half wave: every store instruction writes two 128-byte runs of the k-major planes -- the layout the gather reads.  A lane
// (row r = lane & 31, half h) carries the channels h * CIN/2 ... of its row (CIN/8 16-byte loads, its half of the row,
// contiguous) and of its projection (CIN/2 registers, loaded once per wave); CIN/2 MFMAs per 32 rows.  The VALU form above
// spends 27 * CIN FMAs + 27 * CIN/4 broadcast LDS reads per row (24 TFLOP/s on the 64-channel heads: issue-bound).
template <int CIN>
__global__ void __launch_bounds__(256) k_thin_project_mfma(const float* __restrict__ feat, long long n_in,
                                                           const float* __restrict__ wt, int kc, float* __restrict__ t) {
  constexpr int HC = CIN / 2, NV = HC / 4;
  const int lane = threadIdx.x & 63, r31 = lane & 31, half = lane >> 5;
  const long long ntiles = (n_in + 31) / 32;
  float wa[HC];
#pragma unroll
  for (int c = 0; c < HC; ++c) wa[c] = r31 < kc ? wt[r31 * CIN + half * HC + c] : 0.f;
  const long long tstep = (long long)gridDim.x * 4;
  long long tile = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile >= ntiles) return;
  auto load = [&](long long tl, float4 (&x)[NV]) {
    long long row = tl * 32 + r31;
    if (row >= n_in) row = n_in - 1;                       // tail rows repeat the last row (never stored)
    const float4* src = reinterpret_cast<const float4*>(feat + row * CIN + half * HC);
#pragma unroll
    for (int v = 0; v < NV; ++v) x[v] = src[v];
  };
  auto run = [&](long long tl, const float4 (&x)[NV]) {
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v) {                         // fixed order: channels ascending inside each half
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[4 * v + 0], x[v].x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[4 * v + 1], x[v].y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[4 * v + 2], x[v].z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[4 * v + 3], x[v].w, acc, 0, 0, 0);
    }
    const long long row = tl * 32 + r31;
    if (row < n_in) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int k = cfrag_row(0, e, half);
        if (k < kc) t[(long long)k * n_in + row] = acc[e];
      }
    }
  };
  float4 xa[NV], xb[NV];
  load(tile, xa);
  for (;;) {                                               // two tiles per trip, the buffers swapping roles
    const long long t1 = tile + tstep;
    if (t1 < ntiles) load(t1, xb);
    run(tile, xa);
    if (t1 >= ntiles) break;
    const long long t2 = t1 + tstep;
    if (t2 < ntiles) load(t2, xa);
    run(t1, xb);
    if (t2 >= ntiles) break;
    tile = t2;
  }
}

template <int CIN>
static int launch_project(const float* feat, int64_t n_in, const float* wt, int kc, float* t, hipStream_t s) {
  if constexpr (CIN >= 32) {
    if (kc <= 32) {
      const long long tiles = pcc_cdiv(n_in, 32);
      long long grid = pcc_cdiv(tiles, 4 * 4);             // ~4 tiles per wave: the weight registers are loaded once per wave
      if (grid > 4096) grid = 4096;
      if (grid < 1) grid = 1;
      k_thin_project_mfma<CIN><<<(unsigned)grid, 256, 0, s>>>(feat, n_in, wt, kc, t);
      PCC_LAUNCH_CHECK();
      return PCC_OK;
    }
  }
  k_thin_project<CIN><<<(unsigned)pcc_cdiv(n_in, 256), 256, (size_t)kc * CIN * sizeof(float), s>>>(feat, n_in, wt, kc, t);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

// The three kinds of pcc_conv_fwd that live here, behind one launcher each (declared in pcc_conv.h).
int launch_conv_wave16(const float* feat_in, int64_t n_in, int32_t cin, const float* packed_w, const float* bias, int32_t K,
                       int32_t cout, const int32_t* hdr, const int32_t* nbr, const int32_t* rows, int64_t n_out, float* out,
                       int32_t act, float slope, hipStream_t s, const int32_t* tiles, const int32_t* n_tiles, const float* w2,
                       float* t) {
  Wave16Args a;
  a.feat = feat_in; a.wl = packed_w; a.bias = bias; a.hdr = hdr; a.nbr = nbr; a.rows = rows; a.out = out;
  a.n_out = n_out; a.n_in = n_in; a.K = K; a.cout = cout; a.act = act; a.slope = slope;
  a.tiles = tiles; a.n_tiles = n_tiles; a.w2 = w2; a.t = t;
  if (cin == 16) PCC_TRY(launch_wave16<16>(a, s));
  else if (cin == 32) PCC_TRY(launch_wave16<32>(a, s));
  else PCC_TRY(launch_wave16<64>(a, s));
  return PCC_OK;
}

int launch_conv_thin_t(const float* feat_in, int64_t n_in, int32_t cin, const float* packed_w, const float* bias, int32_t K,
                       int32_t cout, const int32_t* hdr, const int32_t* nbr, const int32_t* rows, int64_t n_out, float* out,
                       int32_t act, float slope, void* ws, size_t ws_bytes, hipStream_t s) {
  if (!ws || ws_bytes < pcc_conv_ws_bytes(n_in, K, cin, cout)) {
    pcc_set_error("pcc_conv_fwd: workspace too small (need pcc_conv_ws_bytes)");
    return PCC_EWS;
  }
  float* t = (float*)ws;
  const int kc = K * cout;
  switch (cin) {
    case 4: PCC_TRY(launch_project<4>(feat_in, n_in, packed_w, kc, t, s)); break;
    case 8: PCC_TRY(launch_project<8>(feat_in, n_in, packed_w, kc, t, s)); break;
    case 16: PCC_TRY(launch_project<16>(feat_in, n_in, packed_w, kc, t, s)); break;
    case 32: PCC_TRY(launch_project<32>(feat_in, n_in, packed_w, kc, t, s)); break;
    default: PCC_TRY(launch_project<64>(feat_in, n_in, packed_w, kc, t, s)); break;
  }
  ThinGatherArgs g;
  g.t = t; g.bias = bias; g.hdr = hdr; g.nbr = nbr; g.rows = rows; g.out = out; g.n_in = n_in; g.n_out = n_out;
  g.cout = cout; g.act = act; g.slope = slope;
  k_thin_gather<4><<<(unsigned)pcc_cdiv(n_out, 256), 256, 0, s>>>(g);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

int launch_conv_thin(const float* feat_in, int32_t cin, const float* packed_w, const float* bias, int32_t cout, const int32_t* hdr,
                     const int32_t* nbr, const int32_t* rows, int64_t n_out, float* out, int32_t act, float slope, hipStream_t s) {
  ThinArgs t;
  t.feat = feat_in; t.wt = packed_w; t.bias = bias; t.hdr = hdr; t.nbr = nbr; t.rows = rows; t.out = out;
  t.n_out = n_out; t.cin = cin; t.cout = cout; t.act = act; t.slope = slope;
  const int vec = (cin % 4 == 0) ? 4 : 1;
  int l = 0;
  while ((1 << l) < cin / vec && l < 6) ++l;
  t.lpr_log2 = l;
  const int64_t rpw = 64 >> l;
  const int64_t waves = pcc_cdiv(n_out, rpw);
  if (vec == 4) k_conv_thin<4, 4><<<(unsigned)pcc_cdiv(waves, 4), 256, 0, s>>>(t);
  else k_conv_thin<4, 1><<<(unsigned)pcc_cdiv(waves, 4), 256, 0, s>>>(t);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

// ------------------------------------------------------------------------------------------
// Band-ordered tile table for stencil kernels over large canonical sets (k_conv_wave16z).
// Canonical order is (x, y, z) with x slowest: the dx = +-1 neighbours of a row live one whole x-slab away, and on the
// 14.5 M-row level of the decoder three slabs of features (8 MB) do not fit an XCD's 4 MB L2, so every row was
// fetched from the fabric three times (round 1: 14.6 GB per launch for 1.86 GB of input).  Here the y range is cut into
// bands; the rows of one (band, x) pair are a contiguous run of the canonical order (found by two binary searches);
// tiles are cut inside the runs and numbered band-major, x ascending.  An XCD's contiguous tile range then sweeps
// x inside one band: the band's part of a slab (~0.3 MB) is still in L2 when it is needed again as dx = 0 and dx = -1.
// Tile word: row0 | (rows - 1) << 27.
// ------------------------------------------------------------------------------------------
__global__ void k_band_segments(const long long* __restrict__ keys, long long n, int lo_x, int nx, int lo_y, int ny, int ts,
                                int nbands, int band_h, int* __restrict__ seg_row0, int* __restrict__ seg_tiles) {
  const int sidx = blockIdx.x * blockDim.x + threadIdx.x;
  if (sidx >= nbands * nx) return;
  const int band = sidx / nx, xi = sidx - band * nx;
  const long long x = (long long)lo_x + (long long)xi * ts + PCC_BIAS;
  const int cy0 = band * band_h, cy1 = min(ny, cy0 + band_h);
  auto lower = [&](long long key) {
    long long lo = 0, hi = n;
    while (lo < hi) {
      const long long mid = (lo + hi) >> 1;
      if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
  };
  long long b = 0, e = 0;
  if (cy0 < cy1) {
    const long long y0 = (long long)lo_y + (long long)cy0 * ts + PCC_BIAS, y1 = (long long)lo_y + (long long)cy1 * ts + PCC_BIAS;
    b = lower((x << PCC_KEY_X_SHIFT) | (y0 << PCC_KEY_Y_SHIFT));      // (batch 0, below every z)
    e = lower((x << PCC_KEY_X_SHIFT) | (y1 << PCC_KEY_Y_SHIFT));
  }
  seg_row0[sidx] = (int)b;
  seg_tiles[sidx] = (int)((e - b + 15) / 16);
  seg_row0[nbands * nx + sidx] = (int)(e - b);       // second half of the array: rows of the run
}

__global__ void __launch_bounds__(1024) k_band_scan(const int* __restrict__ seg_tiles, int nseg, int* __restrict__ seg_tile0,
                                                    int* __restrict__ n_tiles) {
  __shared__ int part[1024];
  const int per = (nseg + 1023) / 1024;
  const int b = threadIdx.x * per, e = min(nseg, b + per);
  int sum = 0;
  for (int i = b; i < e; ++i) sum += seg_tiles[i];
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const int v = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  int run = part[threadIdx.x] - sum;
  for (int i = b; i < e; ++i) { seg_tile0[i] = run; run += seg_tiles[i]; }
  if (threadIdx.x == 1023) *n_tiles = part[1023];
}

__global__ void __launch_bounds__(256) k_band_fill(const int* __restrict__ seg_row0, const int* __restrict__ seg_rows,
                                                   const int* __restrict__ seg_tile0, int nseg, int* __restrict__ tiles) {
  const int sidx = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (sidx >= nseg) return;
  const int rows = seg_rows[sidx], r0 = seg_row0[sidx], t0 = seg_tile0[sidx];
  const int nt = (rows + 15) / 16;
  for (int j = threadIdx.x & 63; j < nt; j += 64) {
    const int cnt = min(16, rows - 16 * j);
    tiles[t0 + j] = (r0 + 16 * j) | ((cnt - 1) << 27);
  }
}

extern "C" int64_t pcc_band_tiles_cap(int64_t n, int32_t nx, int32_t nbands) { return n / 16 + (int64_t)nx * nbands + 16; }
extern "C" size_t pcc_band_tiles_ws_bytes(int32_t nx, int32_t nbands) { return pcc_align_up((size_t)nx * nbands * 4) * 4 + 256; }

extern "C" int pcc_band_tiles_build(const int64_t* keys, int64_t n, int32_t lo_x, int32_t nx, int32_t lo_y, int32_t ny,
                                    int32_t ts, int32_t nbands, int32_t* tiles, int64_t tiles_cap, int32_t* n_tiles,
                                    void* ws, size_t ws_bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PCC_REQUIRE(keys && tiles && n_tiles && ws && n > 0 && n < (1ll << 27), "pcc_band_tiles_build: bad arguments (rows must stay below 2^27)");
  PCC_REQUIRE(nx >= 1 && ny >= 1 && ts >= 1 && nbands >= 1 && (int64_t)nx * nbands <= (1 << 20), "pcc_band_tiles_build: bad lattice");
  PCC_REQUIRE(tiles_cap >= pcc_band_tiles_cap(n, nx, nbands), "pcc_band_tiles_build: tile table too small (pcc_band_tiles_cap)");
  if (ws_bytes < pcc_band_tiles_ws_bytes(nx, nbands)) { pcc_set_error("pcc_band_tiles_build: workspace too small"); return PCC_EWS; }
  const int nseg = nx * nbands;
  const size_t st = pcc_align_up((size_t)nseg * 4);
  int* seg_row0 = (int*)ws;                              // [2][nseg]: first row, row count
  int* seg_tiles = (int*)((char*)ws + 2 * st);
  int* seg_tile0 = (int*)((char*)ws + 3 * st);
  PCC_REQUIRE(st >= (size_t)nseg * 4, "pcc_band_tiles_build: internal");
  const int band_h = (ny + nbands - 1) / nbands;
  // seg_row0 holds both arrays back to back (k_band_segments writes seg_row0[nseg + s] = rows): needs 2*nseg ints
  k_band_segments<<<(unsigned)pcc_cdiv(nseg, 256), 256, 0, s>>>((const long long*)keys, n, lo_x, nx, lo_y, ny, ts, nbands, band_h,
                                                                seg_row0, seg_tiles);
  PCC_LAUNCH_CHECK();
  k_band_scan<<<1, 1024, 0, s>>>(seg_tiles, nseg, seg_tile0, n_tiles);
  PCC_LAUNCH_CHECK();
  k_band_fill<<<(unsigned)pcc_cdiv(nseg, 4), 256, 0, s>>>(seg_row0, seg_row0 + nseg, seg_tile0, nseg, tiles);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

// ------------------------------------------------------------------------------------------
// Occupancy head in one pass over the features (model/transforms.py:141-160, `predict_i`):
//   logits = conv_k3(relu(conv_k3(x; W0, b0)); W2, b2),   W0: cin -> cmid <= 16,  W2: cmid -> 1
// k_conv_wave16z<.., PROJ> evaluates the first convolution, the ReLU and the projections t[k][i] = <h_i, w2_k> tile by
// tile (h never reaches memory), k_thin_gather sums t through the same 3x3x3 map in ascending offset order (fixed
// order, deterministic; the projection runs on the MFMA, so the last bits differ from k_thin_project's VALU dot).
// ------------------------------------------------------------------------------------------
extern "C" int pcc_conv_head_supported(int32_t cin, int32_t cmid) {
  return (cmid > 4 && cmid <= 16 && conv_kind(27, cin, cmid) == KIND_WAVE16 && (size_t)27 * 16 * cin * 4 + 8 * 16 * 17 * 4 <= 64 * 1024) ? 1 : 0;
}
extern "C" size_t pcc_conv_head_ws_bytes(int64_t n) { return (size_t)27 * (size_t)(n > 0 ? n : 1) * sizeof(float) + 256; }

extern "C" int pcc_conv_head_fwd(const float* feat, int64_t n, int32_t cin, const float* packed_w0, const float* bias0,
                                 int32_t cmid, const float* w2, const float* bias2, const int32_t* hdr, const int32_t* nbr,
                                 const int32_t* tiles, const int32_t* n_tiles, float* logits, void* ws, size_t ws_bytes,
                                 void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n <= 0) return PCC_OK;
  PCC_REQUIRE(feat && packed_w0 && w2 && hdr && nbr && logits && ws, "pcc_conv_head_fwd: NULL array");
  PCC_REQUIRE(pcc_conv_head_supported(cin, cmid), "pcc_conv_head_fwd: unsupported shape cin=%d cmid=%d", cin, cmid);
  PCC_REQUIRE((tiles == nullptr) == (n_tiles == nullptr), "pcc_conv_head_fwd: tiles and n_tiles go together");
  PCC_REQUIRE(n * 27 < (1ll << 31) && n * cin * 4 <= 0xFFFFFE00ll && g_wave16_zrun, "pcc_conv_head_fwd: set too large for 32-bit offsets");
  if (ws_bytes < pcc_conv_head_ws_bytes(n)) { pcc_set_error("pcc_conv_head_fwd: workspace too small"); return PCC_EWS; }
  PCC_TRY(prof_begin(s));
  PCC_TRY(launch_conv_wave16(feat, n, cin, packed_w0, bias0, 27, cmid, hdr, nbr, nullptr, n, nullptr, PCC_ACT_RELU, 0.f, s, tiles,
                             n_tiles, w2, (float*)ws));
  PCC_TRY(prof_end(s));
  ThinGatherArgs g;
  g.t = (const float*)ws; g.bias = bias2; g.hdr = hdr; g.nbr = nbr; g.rows = nullptr; g.out = logits; g.n_in = n; g.n_out = n;
  g.cout = 1; g.act = PCC_ACT_NONE; g.slope = 0.f;
  k_thin_gather<1><<<(unsigned)pcc_cdiv(n, 256), 256, 0, s>>>(g);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

// 3x3x3 convolution to <= 4 channels on a full set, neighbours from the set's grid index (no kernel map):
//   t[k*cout+co][i] = <feat[i], w_k[co]>  (k_thin_project),  out[o][co] = b + sum_k t[k*cout+co][nbr_k(o)]
struct ThinGridArgs {
  const float* t; const float* bias; const long long* keys; PccGrid g; float* out; long long n; int cout;
};

template <int COUT_MAX>
__global__ void __launch_bounds__(256) k_thin_gather_grid(ThinGridArgs a) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.n) return;
  const PccGrid& g = a.g;
  const long long key = a.keys[p];
  const PccLattice& L = g.lat;
  const int b = pcc_key_b(key);
  const int cx = (pcc_key_x(key) - L.lo[0]) >> L.ts_log2;
  const int cy = (pcc_key_y(key) - L.lo[1]) >> L.ts_log2;
  const int cz = (pcc_key_z(key) - L.lo[2]) >> L.ts_log2;
  const int z_lo = cz > 0 ? cz - 1 : 0, z_hi = cz + 1 < L.dims[2] ? cz + 1 : L.dims[2] - 1;
  const int nz = z_hi - z_lo + 1;
  float acc[COUT_MAX];
#pragma unroll
  for (int o = 0; o < COUT_MAX; ++o) acc[o] = 0.f;
  // fixed order: (dx,dy) columns ascending, z ascending inside a column (no neighbour table: rows come from the bitmap + rank)
#pragma unroll
  for (int c = 0; c < 9; ++c) {
    const int nx = cx + c % 3 - 1, ny = cy + c / 3 - 1;
    if (nx < 0 || ny < 0 || nx >= L.dims[0] || ny >= L.dims[1]) continue;
    // (spelled out: through pcc_lat_cell this kernel comes out with other instructions, tools/kernel_identity.py)
    const long long cell = (((long long)b * L.dims[0] + nx) * L.dims[1] + ny) * L.dims[2] + z_lo;
    const long long wi = cell >> 6;
    const int sh = (int)(cell & 63);
    const unsigned long long w0 = g.bits[wi];
    unsigned long long f64 = w0 >> sh;
    if (sh + nz > 64) f64 |= g.bits[wi + 1] << (64 - sh);
    unsigned f = (unsigned)f64 & ((1u << nz) - 1u);
    if (!f) continue;
    int r = g.rank[wi] + __popcll(w0 & ((1ull << sh) - 1ull));
    while (f) {
      const int t = __ffs((int)f) - 1;
      f &= f - 1;
      const int k = c + 9 * (z_lo + t - cz + 1);
#pragma unroll
      for (int o = 0; o < COUT_MAX; ++o)
        if (o < a.cout) acc[o] += a.t[(long long)(k * a.cout + o) * a.n + r];
      ++r;
    }
  }
#pragma unroll
  for (int o = 0; o < COUT_MAX; ++o)
    if (o < a.cout) a.out[p * a.cout + o] = acc[o] + (a.bias ? a.bias[o] : 0.f);
}

// one output channel, branch-free: the 9 (bitmap word, rank) pairs of a row are fetched together, then its 27 projected
// values with buffer loads whose offset is out of range for an absent neighbour (27 independent loads in flight per row,
// where the loop form above serialised column after column behind its branches).  t must stay below 4 GB.
__global__ void __launch_bounds__(256) k_thin_gather_grid1(ThinGridArgs a) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.n) return;
  const PccGrid& g = a.g;
  const long long key = a.keys[p];
  const PccLattice& L = g.lat;
  const int b = pcc_key_b(key);
  const int cx = (pcc_key_x(key) - L.lo[0]) >> L.ts_log2;
  const int cy = (pcc_key_y(key) - L.lo[1]) >> L.ts_log2;
  const int cz = (pcc_key_z(key) - L.lo[2]) >> L.ts_log2;
  const int z_lo = cz > 0 ? cz - 1 : 0, z_hi = cz + 1 < L.dims[2] ? cz + 1 : L.dims[2] - 1;
  const int nz = z_hi - z_lo + 1;
  const int dz0 = z_lo - cz + 1;
  unsigned long long w0[9], w1[9];
  int rk[9], sh[9];
  bool ok[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) {
    const int nx = cx + c % 3 - 1, ny = cy + c / 3 - 1;
    ok[c] = !(nx < 0 || ny < 0 || nx >= L.dims[0] || ny >= L.dims[1]);
    const long long cell = ok[c] ? pcc_lat_cell(L, b, nx, ny, z_lo) : 0ll;
    const long long wi = cell >> 6;
    sh[c] = (int)(cell & 63);
    w0[c] = g.bits[wi];
    rk[c] = g.rank[wi];
    w1[c] = (sh[c] + nz > 64) ? g.bits[wi + 1] : 0ull;        // (rare: the field straddles two words)
  }
  const __amdgpu_buffer_rsrc_t rsT = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.t), (short)0,
                                                                       (int)(unsigned)((size_t)27 * a.n * 4), 0x00020000);
  float v[27];
#pragma unroll
  for (int c = 0; c < 9; ++c) {
    unsigned long long f64 = w0[c] >> sh[c];
    if (sh[c] + nz > 64) f64 |= w1[c] << (64 - sh[c]);
    const unsigned f = ok[c] ? ((unsigned)f64 & ((1u << nz) - 1u)) : 0u;
    const int r = rk[c] + __popcll(w0[c] & ((1ull << sh[c]) - 1ull));
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int k = c + 9 * (dz0 + t);                         // (k < 27 whenever bit t can be set: t < nz)
      const unsigned row = (unsigned)(r + __popc(f & ((1u << t) - 1u)));
      const unsigned off = ((f >> t) & 1u) ? ((unsigned)k * (unsigned)a.n + row) * 4u : BUF_OOB;
      v[c * 3 + t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsT, off, 0, 0));
    }
  }
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < 27; ++i) acc += v[i];                    // fixed order: columns ascending, z ascending (absent: + 0)
  a.out[p] = acc + (a.bias ? a.bias[0] : 0.f);
}

// z-folded planes (round 3, one output channel over <= 16 hidden channels: the last level's head).  Canonical order is z fastest,
// so the dz = -1 / +1 neighbours of row i inside a (x, y) column are rows i - 1 / i + 1.  The projection pass therefore pre-adds a
// column's three terms for the row in the MIDDLE:   S_g[i] = <h_i, w(g,0)> + [i-1 adjacent] <h_{i-1}, w(g,-1)> + [i+1 adjacent]
// <h_{i+1}, w(g,+1)>   (g = the 9 (dx, dy) columns), and keeps the dz = -1 / +1 single terms as U_g[i], D_g[i] for the rare
// column whose middle cell is absent.  The gather then reads ONE value per column (9 x 4 B per row instead of 27 x 4 B, the
// same 27 planes in memory): 2.0 -> ~1.0 GB of L2 / HBM reads on the last level.
template <int CIN>
__global__ void __launch_bounds__(256) k_thin_project_z(const float* __restrict__ feat, const long long* __restrict__ keys,
                                                        long long n_in, long long ts, const float* __restrict__ wt,
                                                        float* __restrict__ t) {
  // A workgroup owns 256 consecutive rows (aligned 256-byte store runs per wave and plane).  Pass 1 projects every row on the
  // 27 kernels into LDS (one column per row + one halo column each side: the rows just outside the workgroup are projected by
  // 18 of its threads); pass 2 adds a column's neighbour terms from the adjacent LDS columns.  The loops over the kernels stay
  // rolled: unrolled, the compiler keeps all 27 x CIN weights in registers (256 VGPRs + spills, one wave per SIMD: 1.6 ms).
  extern __shared__ __attribute__((aligned(16))) float w_s[];          // 27 * CIN weights
  __shared__ float sd[27][258];                                        // [kernel][1 + thread] (+ halo columns 0 and 257)
  for (int i = threadIdx.x; i < 27 * CIN; i += 256) w_s[i] = wt[i];
  __syncthreads();
  const long long base = (long long)blockIdx.x * 256;
  const long long i = base + threadIdx.x;
  const bool valid = i < n_in;
  float4 x[CIN / 4];
#pragma unroll
  for (int c = 0; c < CIN / 4; ++c) x[c] = valid ? reinterpret_cast<const float4*>(feat + i * CIN)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
  const long long key = valid ? keys[i] : -(1ll << 62);
  const bool adjm = valid && i > 0 && keys[i - 1] == key - ts;         // row i - 1 is the z - 1 cell of the same column
  const bool adjp = valid && i + 1 < n_in && keys[i + 1] == key + ts;
#pragma unroll 1
  for (int k = 0; k < 27; ++k) {
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < CIN / 4; ++c) {
      const float4 w = reinterpret_cast<const float4*>(w_s + k * CIN)[c];   // wave-uniform address: LDS broadcast
      acc += x[c].x * w.x + x[c].y * w.y + x[c].z * w.z + x[c].w * w.w;
    }
    sd[k][1 + threadIdx.x] = acc;
  }
  // the rows just outside the workgroup: thread e < 9 projects row base - 1 on w(e, dz = -1), thread 9 + e row base + 256 on
  // w(e, dz = +1) (same dot, same order of additions as above)
  if (threadIdx.x < 18) {
    const int e = threadIdx.x < 9 ? threadIdx.x : threadIdx.x - 9;
    const long long r = threadIdx.x < 9 ? base - 1 : base + 256;
    const int k = threadIdx.x < 9 ? e : e + 18;
    float acc = 0.f;
    if (r >= 0 && r < n_in) {
#pragma unroll
      for (int c = 0; c < CIN / 4; ++c) {
        const float4 xv = reinterpret_cast<const float4*>(feat + r * CIN)[c];
        const float4 w = reinterpret_cast<const float4*>(w_s + k * CIN)[c];
        acc += xv.x * w.x + xv.y * w.y + xv.z * w.z + xv.w * w.w;
      }
    }
    sd[k][threadIdx.x < 9 ? 0 : 257] = acc;
  }
  __syncthreads();
  if (!valid) return;
  const int col = 1 + threadIdx.x;
#pragma unroll 1
  for (int g = 0; g < 9; ++g) {
    const float lo = sd[g][col], mid = sd[g + 9][col], hi = sd[g + 18][col];
    const float from_dn = sd[g][col - 1];                               // <h_{i-1}, w(g, dz = -1)>
    const float from_up = sd[g + 18][col + 1];                          // <h_{i+1}, w(g, dz = +1)>
    t[(long long)g * n_in + i] = (mid + (adjm ? from_dn : 0.f)) + (adjp ? from_up : 0.f);
    t[(long long)(9 + g) * n_in + i] = lo;
    t[(long long)(18 + g) * n_in + i] = hi;
  }
}

// gather over the z-folded planes: per column the middle cell's S value, or -- middle absent -- the U / D singles of the cells
// below / above it.  Three buffer loads per column, at most two of them in range.
__global__ void __launch_bounds__(256) k_thin_gather_grid1z(ThinGridArgs a) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.n) return;
  const PccGrid& g = a.g;
  const long long key = a.keys[p];
  const PccLattice& L = g.lat;
  const int b = pcc_key_b(key);
  const int cx = (pcc_key_x(key) - L.lo[0]) >> L.ts_log2;
  const int cy = (pcc_key_y(key) - L.lo[1]) >> L.ts_log2;
  const int cz = (pcc_key_z(key) - L.lo[2]) >> L.ts_log2;
  const int z_lo = cz > 0 ? cz - 1 : 0, z_hi = cz + 1 < L.dims[2] ? cz + 1 : L.dims[2] - 1;
  const int nz = z_hi - z_lo + 1;
  const int dz0 = z_lo - cz + 1;                                      // dz index (0, 1, 2 = -1, 0, +1) of the field's bit 0
  unsigned long long w0[9], w1[9];
  int rk[9], sh[9];
  bool ok[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) {
    const int nx = cx + c % 3 - 1, ny = cy + c / 3 - 1;
    ok[c] = !(nx < 0 || ny < 0 || nx >= L.dims[0] || ny >= L.dims[1]);
    const long long cell = ok[c] ? pcc_lat_cell(L, b, nx, ny, z_lo) : 0ll;
    const long long wi = cell >> 6;
    sh[c] = (int)(cell & 63);
    w0[c] = g.bits[wi];
    rk[c] = g.rank[wi];
    w1[c] = (sh[c] + nz > 64) ? g.bits[wi + 1] : 0ull;
  }
  const __amdgpu_buffer_rsrc_t rsT = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.t), (short)0,
                                                                       (int)(unsigned)((size_t)27 * a.n * 4), 0x00020000);
  const int tm = 1 - dz0;                                             // bit of the middle cell (dz0 <= 1: it is inside the field)
  float v[27];
#pragma unroll
  for (int c = 0; c < 9; ++c) {
    unsigned long long f64 = w0[c] >> sh[c];
    if (sh[c] + nz > 64) f64 |= w1[c] << (64 - sh[c]);
    const unsigned f = ok[c] ? ((unsigned)f64 & ((1u << nz) - 1u)) : 0u;
    const unsigned r = (unsigned)(rk[c] + __popcll(w0[c] & ((1ull << sh[c]) - 1ull)));
    const bool mid = (f >> tm) & 1u;
    const bool low = dz0 == 0 && (f & 1u);                            // the dz = -1 cell is bit 0, present only when z_lo = cz - 1
    const int tu = 2 - dz0;                                           // bit of the dz = +1 cell (may lie past the field: then absent)
    const bool upp = tu < nz && ((f >> tu) & 1u);
    const unsigned row_mid = r + __popc(f & ((1u << tm) - 1u));
    const unsigned row_up = r + __popc(f & ((1u << tu) - 1u));
    const unsigned n = (unsigned)a.n;
    const unsigned o_s = mid ? ((unsigned)c * n + row_mid) * 4u : BUF_OOB;
    const unsigned o_u = (!mid && low) ? ((unsigned)(9 + c) * n + r) * 4u : BUF_OOB;
    const unsigned o_d = (!mid && upp) ? ((unsigned)(18 + c) * n + row_up) * 4u : BUF_OOB;
    v[c * 3 + 0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsT, o_s, 0, 0));
    v[c * 3 + 1] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsT, o_u, 0, 0));
    v[c * 3 + 2] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsT, o_d, 0, 0));
  }
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < 27; ++i) acc += v[i];                    // fixed order: columns ascending (absent: + 0)
  a.out[p] = acc + (a.bias ? a.bias[0] : 0.f);
}

// (Round 3 built a one-pass form of this convolution -- gather the 27 neighbours' hidden rows and dot them with w2 in
//  registers, dz = +-1 terms taken from the adjacent candidate by lane shuffle -- three times: columns walked one after the
//  other (latency-bound, +0.8 ms per step), all loads independent with index arithmetic per lane (issue-bound, +1.6 ms), index
//  arithmetic once per row and four lanes per row for coalesced 64-byte loads (+1.1 ms: 1.59 ms on the last level against
//  0.55 + 0.60 for project + gather).  Moving 9 x 64 B per output through L1 costs more than writing 27 floats per row and
//  gathering 27 x 4 B: the two-kernel form stays.)
// one-channel heads over 16 hidden channels: rows from which the z-folded planes are used (negative: never)
static long long g_thin_z_min_rows = 1ll << 20;
extern "C" int pcc_set_thin_z_min_rows(int64_t rows) { g_thin_z_min_rows = rows; return PCC_OK; }

extern "C" size_t pcc_thin_grid_ws_bytes(int64_t n, int32_t cout) { return (size_t)27 * cout * (size_t)(n > 0 ? n : 1) * sizeof(float) + 256; }

extern "C" int pcc_conv_thin_grid_fwd(const float* feat, int64_t n, int32_t cin, const float* packed_w /*thin layout [27][cout][cin]*/,
                                      const float* bias, int32_t cout, const int64_t* keys, const uint64_t* bits,
                                      const int32_t* rank, const int32_t* h_grid, float* out, void* ws, size_t ws_bytes,
                                      void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n <= 0) return PCC_OK;
  PCC_REQUIRE(feat && packed_w && keys && bits && rank && out && ws, "pcc_conv_thin_grid_fwd: NULL array");
  PccGrid g;
  PCC_TRY(pcc_grid_from_host(bits, rank, h_grid, "pcc_conv_thin_grid_fwd", &g));
  PCC_REQUIRE(cout >= 1 && cout <= 4 && conv_kind(27, cin, cout) == KIND_THIN_T, "pcc_conv_thin_grid_fwd: unsupported shape cin=%d cout=%d", cin, cout);
  if (ws_bytes < pcc_thin_grid_ws_bytes(n, cout)) { pcc_set_error("pcc_conv_thin_grid_fwd: workspace too small"); return PCC_EWS; }
  float* t = (float*)ws;
  const int kc = 27 * cout;
  if (g_thin_z_min_rows >= 0 && cout == 1 && cin == 16 && (size_t)27 * n * 4 <= (size_t)BUF_MAX_BYTES && n >= g_thin_z_min_rows) {
    // narrow hidden layer over a large set (the last level): z-folded planes, one value per column in the gather
    k_thin_project_z<16><<<(unsigned)pcc_cdiv(n, 256), 256, (size_t)27 * 16 * sizeof(float), s>>>(
        feat, (const long long*)keys, n, (long long)h_grid[6], packed_w, t);
    ThinGridArgs az;
    az.t = t; az.bias = bias; az.keys = (const long long*)keys; az.g = g; az.out = out; az.n = n; az.cout = 1;
    k_thin_gather_grid1z<<<(unsigned)pcc_cdiv(n, 256), 256, 0, s>>>(az);
    PCC_LAUNCH_CHECK();
    return PCC_OK;
  }
  switch (cin) {
    case 4: PCC_TRY(launch_project<4>(feat, n, packed_w, kc, t, s)); break;
    case 8: PCC_TRY(launch_project<8>(feat, n, packed_w, kc, t, s)); break;
    case 16: PCC_TRY(launch_project<16>(feat, n, packed_w, kc, t, s)); break;
    case 32: PCC_TRY(launch_project<32>(feat, n, packed_w, kc, t, s)); break;
    default: PCC_TRY(launch_project<64>(feat, n, packed_w, kc, t, s)); break;
  }
  ThinGridArgs a;
  a.t = t; a.bias = bias; a.keys = (const long long*)keys; a.g = g; a.out = out; a.n = n; a.cout = cout;
  if (cout == 1 && (size_t)27 * n * 4 <= (size_t)BUF_MAX_BYTES) k_thin_gather_grid1<<<(unsigned)pcc_cdiv(n, 256), 256, 0, s>>>(a);
  else if (cout == 1) k_thin_gather_grid<1><<<(unsigned)pcc_cdiv(n, 256), 256, 0, s>>>(a);
  else k_thin_gather_grid<4><<<(unsigned)pcc_cdiv(n, 256), 256, 0, s>>>(a);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}
