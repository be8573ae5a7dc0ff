// What pcc_conv.hip shares with the two files that hold its general MFMA kernels, pcc_conv_f32.hip and pcc_conv_bf.hip: the kernel
// argument struct, the constants the kernels use and the two launchers.  No state.
#pragma once
#include "pcc_common.h"
#include "pcc_mfma.h"

static constexpr int MAXK = 128;    // kernel offsets per segment (K <= 125)

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

// The two general MFMA kernels, each compiled in a file of its own: k_conv_mfma<WM, WN, TM, TN, MODE, BUF> (pcc_conv_f32.hip) and
// k_conv_mfma_bf<WM, WN, TM, TN, MODE> (pcc_conv_bf.hip) for the tiles launch_mfma and launch_pair_product choose (pcc_conv.hip);
// any other (mode, tile) is an error.  C++ linkage, hidden: the library's dynamic symbol table holds neither.
#pragma GCC visibility push(hidden)
int launch_conv_f32(int mode, int wm, int wn, int tm, int tn, bool buf, const ConvArgs& a, dim3 grid, hipStream_t s);
int launch_conv_bf(int mode, int wm, int wn, int tm, int tn, const ConvArgs& a, dim3 grid, hipStream_t s);
#pragma GCC visibility pop
