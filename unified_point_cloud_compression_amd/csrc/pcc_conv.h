// What the forward-convolution sources share: pcc_conv.hip (the dispatcher, packing, the library scratch, the profiling state), the
// two general MFMA kernels (pcc_conv_f32.hip, pcc_conv_bf.hip), the stripped GEMMs of the dense and pair products
// (pcc_conv_dense.hip), the narrow-output kernels (pcc_conv_thin.hip) and the transposed convolutions (pcc_convt.hip).
// The rule: this header holds types, constants, pure functions (static inline, one body each) and DECLARATIONS -- never a variable.
// All state of the family (scratch buffers, profiling log, env switches) is defined once, in pcc_conv.hip, and the other files
// reach it only through the hidden functions declared at the end.
#pragma once
#include "pcc_common.h"
#include "pcc_mfma.h"

static constexpr int MAXK = 128;    // kernel offsets per segment (K <= 125)
static constexpr int PAIR_BM = 128; // pairs per tile of the gathered pair GEMM (pair-list planner, pcc_convt_fwd_rows)

enum { MODE_CONV = 0, MODE_GDN = 1, MODE_IGDN = 2 };
// Phase switches of the GEMM kernels (tools/gemm_probe.py): compiled in only by `make DBG=1` (-DPCC_DBG_BUILD); in the shipped
// library the tests are the constant 0 and the compiler drops them.
#ifdef PCC_DBG_BUILD
#define PCC_DBG_ON(a, bit) (((a).dbg & (bit)) != 0)
#else
#define PCC_DBG_ON(a, bit) false
#endif

struct ConvArgs {
  const float* feat;      // [n_in, cin]
  const float* wp;        // packed weights [K*ppo][cout_pad][CB]
  const float* bias;      // [cout] or null (GDN: beta_eff)
  const int* hdr;         // map header (null: identity, one segment of n_out positions)
  const int* nbr;
  const int* rows;
  float* out;             // [n_out, cout]
  long long n_out;
  long long n_in;         // rows of feat (buffer-addressed gathers)
  long long wp_elems;     // floats in wp
  const int* pair_in = nullptr;   // pair mode (pcc_conv_fwd_pairs): input row of every (padded) pair, -1 = padding
  const int* tile_k = nullptr;    // pair mode: kernel offset of each 128-pair tile
  const long long* n_tiles = nullptr;   // pair mode: device count of tiles (the grid is an upper bound)
  const unsigned char* featb = nullptr; // split path: bf16 planes of feat, [n_in][cin/32][3][32] (k_feat_split)
  int ksplit = 1;                       // split path, map mode: the (offset, channel-block) reduction cut over ksplit workgroups
  float* part = nullptr;                //   partial tiles [ksplit][n_out][cout], summed in fixed order by k_splitk_reduce
  int dbg = 0;                          // diagnostics (probe builds only, `make DBG=1` + env PCC_DBG): 1 = no output stores, 2 = no MFMA phase, 4 = no staging loads
  int nt = 0;                           // non-temporal accesses of streamed buffers (g_nt): 1 = dense products' stores, 2 = pair products' stores
  bool wh_ok = false;                   // dense products: the pack carries scaled fp16 planes + column scales (split_planes_h)
  const unsigned char* feath = nullptr; //   scaled fp16 planes of feat, [n_in][cin/32][2][32] (k_feat_split_h)
  const float* frow_inv = nullptr;      //   and 1 / (power-of-two scale) of every feature row
  int arith = PCC_ARITH_H3;             // arithmetic form of this call (include/pcc_hip.h PCC_ARITH_*): an argument of every entry point, no process state
  int* guard = nullptr;                 //   range guard of the fp16-pair products (the entry point's d_guard): set to 1 when a (row, column) pair of
  float guard_lim = 0.f;                //   a tile has rinv * cinv * 8 * cin > guard_lim, i.e. max|row| * max|column| * cin * 2^-27 may exceed the budget
  int cin, cout, cout_pad;
  int cb_log2;            // log2(CB), CB = min(cin, 32)
  int ppo;                // pieces per offset = cin / CB
  int act;
  float slope;
};

// ---- pure shape helpers: which kernel form a shape takes and how its weights are packed ---------------------------------------
__host__ __device__ inline int bn_for(int cout) { return cout >= 128 ? 128 : (cout > 32 ? 64 : 32); }
static inline bool mfma_ok(int cin, int cout) {
  if (cout <= 4) return false;
  if (cin == 4 || cin == 8 || cin == 16) return true;
  return cin >= 32 && cin % 32 == 0;
}
static inline int cb_log2_for(int cin) { return cin >= 32 ? 5 : (cin == 16 ? 4 : (cin == 8 ? 3 : 2)); }
static inline int cout_pad_for(int cout) { const int bn = bn_for(cout); return (cout + bn - 1) / bn * bn; }

enum { KIND_NONE = -1, KIND_MFMA = 0, KIND_WAVE16 = 1, KIND_THIN_T = 2, KIND_THIN = 3 };
// MFMA weight images: the fp32 layout, followed (cin a multiple of 32) by the three bf16 planes of the split path
static inline int64_t mfma_packed_total(int64_t fp32_elems, int cin) { return cin % 32 == 0 ? fp32_elems + bf_plane_elems(fp32_elems) : fp32_elems; }
static inline int conv_kind(int K, int cin, int cout) {
  if (cout <= 4) {
    const bool pow2 = cin == 4 || cin == 8 || cin == 16 || cin == 32 || cin == 64;
    if (pow2 && (int64_t)K * cout * cin * 4 <= 48 * 1024) return KIND_THIN_T;
    return KIND_THIN;
  }
  if (cout <= 16 && (cin == 16 || cin == 32 || cin == 64) && (int64_t)K * 16 * (cin + 4) * 4 <= 64 * 1024)
    return KIND_WAVE16;
  return mfma_ok(cin, cout) ? KIND_MFMA : KIND_NONE;
}

// convolutions that run as gathered pair GEMMs (5x5x5 and wider, 128+ output channels): the pack also carries the scaled fp16
// planes and the 1/scale of every (offset, column), fp32 image | bf16 planes | fp16 planes | K*cout_pad scales
static inline bool conv_has_h(int K, int cin, int cout) {
  return K >= 64 && cin % 32 == 0 && cin <= 256 && cout % 4 == 0 && bn_for(cout) == 128;
}

// ---- pure device helpers of the VALU kernels: one scalar or one float4 of channels per lane (the thin kernels of
//      pcc_conv_thin.hip and the gather-sums of pcc_convt.hip), and the activation every epilogue applies ------------------------
template <int VEC> struct ThinVec;
template <> struct ThinVec<4> { typedef float4 T; };
template <> struct ThinVec<1> { typedef float T; };
__device__ inline float thin_dot(float4 x, float4 w) { return x.x * w.x + x.y * w.y + x.z * w.z + x.w * w.w; }
__device__ inline float thin_dot(float x, float w) { return x * w; }
__device__ inline void thin_zero(float4& v) { v = make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ inline void thin_zero(float& v) { v = 0.f; }
__device__ inline void thin_acc(float4& a, const float4 x) { a.x += x.x; a.y += x.y; a.z += x.z; a.w += x.w; }
__device__ inline void thin_acc(float& a, const float x) { a += x; }
// a += x * m with m = 1 or 0 (one rounding, so m = 1 gives exactly a + x)
__device__ inline void thin_fma(float4& a, const float4 x, float m) { a.x = fmaf(x.x, m, a.x); a.y = fmaf(x.y, m, a.y); a.z = fmaf(x.z, m, a.z); a.w = fmaf(x.w, m, a.w); }
__device__ inline void thin_fma(float& a, const float x, float m) { a = fmaf(x, m, a); }
__device__ inline float act1(float v, int act, float slope) {
  if (act == PCC_ACT_RELU) return fmaxf(v, 0.f);
  if (act == PCC_ACT_LEAKY) return v >= 0.f ? v : v * slope;
  return v;
}
__device__ inline void thin_act(float4& a, int act, float s) { a.x = act1(a.x, act, s); a.y = act1(a.y, act, s); a.z = act1(a.z, act, s); a.w = act1(a.w, act, s); }
__device__ inline void thin_act(float& a, int act, float s) { a = act1(a, act, s); }

// ---- what one file of the family calls in another.  C++ linkage, hidden: the library's dynamic symbol table holds none of it ----
#pragma GCC visibility push(hidden)
// The two general MFMA kernels, each compiled in a file of its own: k_conv_mfma<WM, WN, TM, TN, MODE, BUF> (pcc_conv_f32.hip) and
// k_conv_mfma_bf<WM, WN, TM, TN, MODE> (pcc_conv_bf.hip) for the tiles launch_mfma and launch_pair_product choose (pcc_conv.hip);
// any other (mode, tile) is an error.
int launch_conv_f32(int mode, int wm, int wn, int tm, int tn, bool buf, const ConvArgs& a, dim3 grid, hipStream_t s);
int launch_conv_bf(int mode, int wm, int wn, int tm, int tn, const ConvArgs& a, dim3 grid, hipStream_t s);

// pcc_conv_dense.hip: k_gemm_bf2 / k_gemm_h2 / k_pair_h2 for the chunk count a.ppo = cin / 32, one of nch_ok()
bool nch_ok(int nch);
int launch_gemm_bf2(const ConvArgs& a, dim3 grid, hipStream_t s);
int launch_gemm_h2(const ConvArgs& a, dim3 grid, hipStream_t s);
int launch_pair_h2(const ConvArgs& a, dim3 grid, hipStream_t s);

// pcc_conv_thin.hip: the three kinds of pcc_conv_fwd that are not KIND_MFMA, each taking the entry point's own arguments
// (wave16: the trailing four are the tile table and the fused 16 -> 1 projection of pcc_conv_head_fwd)
int launch_conv_wave16(const float* feat_in, int64_t n_in, int32_t cin, const float* packed_w, const float* bias, int32_t K,
                       int32_t cout, const int32_t* hdr, const int32_t* nbr, const int32_t* rows, int64_t n_out, float* out,
                       int32_t act, float slope, hipStream_t s, const int32_t* tiles = nullptr, const int32_t* n_tiles = nullptr,
                       const float* w2 = nullptr, float* t = nullptr);
int launch_conv_thin_t(const float* feat_in, int64_t n_in, int32_t cin, const float* packed_w, const float* bias, int32_t K,
                       int32_t cout, const int32_t* hdr, const int32_t* nbr, const int32_t* rows, int64_t n_out, float* out,
                       int32_t act, float slope, void* ws, size_t ws_bytes, hipStream_t s);
int launch_conv_thin(const float* feat_in, int32_t cin, const float* packed_w, const float* bias, int32_t cout, const int32_t* hdr,
                     const int32_t* nbr, const int32_t* rows, int64_t n_out, float* out, int32_t act, float slope, hipStream_t s);

// pcc_conv.hip: the state of the family behind functions
int lib_scratch(size_t bytes, void** out);          // grow-only device scratch (planes of the current convolution's input)
int lib_scratch_small(size_t bytes, void** out);    // a second, small one (tables that live beside the planes of the same call)
int prof_begin(hipStream_t s, bool when = true);    // event pair around a launch while pcc_prof_enable is on (and `when`)
int prof_end(hipStream_t s, bool when = true, int form = -1);
void prof_note(int form, double flops, double bytes);
void prof_tile(int bm, int bn, int ksplit);         // after prof_note
bool prof_on();                                     // pcc_prof_enable is on
int nt_flags();                                     // env PCC_NT (g_nt): which streamed buffers take non-temporal accesses
// and the steps of an MFMA launch the other files use
ConvArgs conv_args(const float* feat, long long n_in, int cin, const float* wp, int K, int cout, const float* bias, float* out,
                   long long n_out, int act = 0, float slope = 0.f);
int set_arith(ConvArgs& a, int arith, int32_t* d_guard, const char* who);
int split_planes(float* packed, int64_t fp32_elems, int cin, hipStream_t s);
int split_planes_h(float* packed, int64_t fp32_elems, int K, int cin, int cout_pad, hipStream_t s);
int launch_mfma(int mode, const ConvArgs& a_in, int tiles_bound_extra, hipStream_t s);
int launch_pair_product(ConvArgs& a, int K, long long tiles, hipStream_t s);
int launch_pair_tile_k(const int* pstart, int K, long long tiles, int* tile_k, hipStream_t s);   // k_pair_tile_k of the pair planner
#pragma GCC visibility pop
