/*
 * pcc_hip.h -- C ABI of libpcc_hip.so, the MI355X (gfx950) sparse-voxel codec hot path.
 *
 * This is the drop-in boundary.  The reference
 * (ikt-luh/Unified-Point-Cloud-Compression) reaches this path through two Python import
 * surfaces, `import MinkowskiEngine as ME` and `compressai.*`; the Python shims in
 * unified_point_cloud_compression_amd/{MinkowskiEngine,compressai}/ bind these entry points
 * with ctypes.  Every entry point names the reference interface it replaces (file:line in
 * /root/reference).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name starts with `h_`;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - functions return 0 on success, a negative PCC_E* code otherwise; pcc_last_error()
 *     gives the message of the calling thread's last failure; no exceptions, no ownership
 *     transfer: outputs and workspaces are caller-allocated (sizes from the *_ws_bytes /
 *     *_elems queries).  Two exceptions, owned by the library per process: a grow-only device
 *     scratch for the 16-bit operand planes / split-K partial tiles of the convolution entry
 *     points (pcc_conv_fwd, pcc_conv_fwd_pairs, pcc_convt_fwd*, pcc_gdn_fwd) and a small table
 *     buffer of pcc_convt_fwd_csr*.  They are allocated with hipMalloc outside the caller's
 *     allocator, and GROWING one synchronises the device once (hipDeviceSynchronize + hipFree);
 *     otherwise nothing here synchronises the stream;
 *   - threading: ONE stream per device at a time for the convolution entry points (they share
 *     the scratch above in stream order); calls from two host threads or on two streams of the
 *     same device must be serialised by the caller.  The pure coordinate / entropy entry points
 *     keep no state;
 *   - coordinates are packed int64 keys  b<<48 | (x+2^15)<<32 | (y+2^15)<<16 | (z+2^15);
 *     a coordinate set is a strictly ascending key array ("canonical order" = the order
 *     `utils.sort_tensor` produces, utils.py:142-165);
 *   - features are row-major float32 [N, C].
 */
#ifndef PCC_HIP_H
#define PCC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCC_OK 0
#define PCC_EINVAL (-1)   /* bad argument / unsupported shape */
#define PCC_EHIP (-2)     /* HIP runtime error              */
#define PCC_EWS (-3)      /* workspace too small            */

#define PCC_ACT_NONE 0
#define PCC_ACT_RELU 1    /* ME.MinkowskiReLU      (model/transforms.py:148,153,158)          */
#define PCC_ACT_LEAKY 2   /* ME.MinkowskiLeakyReLU (model/entropy_models.py:179,181,187,189)  */

#define PCC_MAP_HDR_INTS 512  /* int32 words of a kernel-map header (device resident)        */
#define PCC_MAP_MAX_SEG 8

int pcc_version(void);
const char* pcc_last_error(void);
/* number of compute units / name of the current device (sanity: must be gfx950). */
int pcc_device_info(int* h_cu_count, char* h_arch, int h_arch_len);

/* ------------------------------------------------------------------------------------------
 * a1 / a11  coordinate keys            (ME.SparseTensor ctor: model/model.py:66-70,147-161,227;
 *                                       ME.utils.sparse_quantize: model/model.py:152-156)
 * ---------------------------------------------------------------------------------------- */
/* {min b,x,y,z, max b,x,y,z} of [n,4] coordinates (int32, or float: floored) -- sizes the key range / grid lattices */
int pcc_coords_bounds(const void* coords, int32_t is_float, int64_t n, int32_t* out8 /*device*/, void* stream);
/* dst[i][:] = src[idx[i]][:]: features of user-ordered rows in canonical order (ME.SparseTensor) */
int pcc_rows_gather(const float* src, const int64_t* idx, int64_t m, int32_t c, float* dst, void* stream);
/* int32 [n,4] (b,x,y,z) -> keys */
int pcc_keys_pack_i32(const int32_t* coords, int64_t n, int64_t* keys, void* stream);
/* float [n,4] -> floor -> keys (the reference passes float coordinates, model/model.py:142-149) */
int pcc_keys_pack_f32(const float* coords, int64_t n, int64_t* keys, void* stream);
int pcc_keys_unpack(const int64_t* keys, int64_t n, int32_t* coords, void* stream);
/* Row ranges per batch index of a canonical key array whose row count *d_n may still be on the device: out[e] = first row with batch
 * index >= e for e in [0, entries), entries <= 12 (out_a: entries 0-3, out_b: 4-7, out_c: 8-11; 4 int64 each).  Lets a caller read a derived
 * set's size and its per-batch ranges (reference model/transforms.py:228-254: top-k per batch) in one host read. */
int pcc_batch_bounds(const int64_t* keys, const int64_t* d_n /*nullable: then n_host rows*/, int64_t n_host, int32_t entries,
                     int64_t* out_a, int64_t* out_b, int64_t* out_c, void* stream);

/* LSD radix sort of keys (stable), optional payload perm_out[i] = input index of output i.
 * Only 8-bit digits intersecting `bit_mask` (bits that may differ between keys) are sorted. */
size_t pcc_sort_ws_bytes(int64_t n);
int pcc_sort_keys(const int64_t* keys_in, int64_t n, uint64_t bit_mask, int64_t* keys_out,
                  int32_t* perm_out /*nullable*/, void* ws, size_t ws_bytes, void* stream);

/* adjacent-unique of a sorted key array.  uniq[] (capacity n), first[] (nullable; index in the
 * sorted array of the first occurrence), *d_count = number of unique keys (device int64). */
size_t pcc_unique_ws_bytes(int64_t n);
int pcc_unique_sorted(const int64_t* sorted_keys, int64_t n, int64_t* uniq, int32_t* first,
                      int64_t* d_count, void* ws, size_t ws_bytes, void* stream);

/* *d_flag != 0 when keys[] is strictly ascending, else 0 (device int32). */
int pcc_keys_is_canonical(const int64_t* keys, int64_t n, int32_t* d_flag, void* stream);

/* a2(i)  strided output set, ME stride map: out = unique(floor(c/m)*m), m = new tensor stride
 * (power of two).  (ME.MinkowskiConvolution stride=2: model/transforms.py:33,37,41;
 * model/entropy_models.py:180,182; coordinate-only use model/model.py:227-229 = row a12.) */
size_t pcc_stride_ws_bytes(int64_t n);
int pcc_coords_stride(const int64_t* keys, int64_t n, int32_t new_stride, uint64_t bit_mask,
                      int64_t* out_keys /*cap n*/, int64_t* d_count, void* ws, size_t ws_bytes,
                      void* stream);

/* a3(i)  generative output set: unique{ c + off_k * ts_out }, K = kernel_size^3 offsets
 * (ME.MinkowskiGenerativeConvolutionTranspose: model/transforms.py:129,133,137;
 * model/entropy_models.py:186,188). out_keys capacity n*K. */
size_t pcc_expand_ws_bytes(int64_t n, int32_t kernel_size);
int pcc_coords_expand(const int64_t* keys, int64_t n, int32_t kernel_size, int32_t ts_out,
                      uint64_t bit_mask, int64_t* out_keys /*cap n*K*/, int64_t* d_count, void* ws,
                      size_t ws_bytes, void* stream);

/* a3(i)+(ii) fused: generative output set AND its transposed kernel map in CSR form from ONE sort.
 * Candidates are sorted as 32-bit cell indices of the output lattice h_lattice = {lo_x,lo_y,lo_z, cells_x,cells_y,
 * cells_z, pitch (= ts_out), batches} (needs <= 2^32 cells) with the pair id i*K+k as payload:
 *   out_keys[o]                       the output coordinate set (capacity n*K), *d_count rows
 *   pair_ids[first[o] .. first[o+1])  the (input row, offset) pairs landing on output row o, ascending
 * pair_ids: n*K ints, first: n*K+1 ints. */
size_t pcc_expand_csr_ws_bytes(int64_t n, int32_t kernel_size);
int pcc_coords_expand_csr(const int64_t* keys, int64_t n, int32_t kernel_size, int32_t ts_out,
                          const int32_t* h_lattice, int64_t* out_keys, int64_t* d_count, int32_t* pair_ids,
                          int32_t* first, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * a2(ii) / a3  kernel map              (ME kernel map behind every conv forward)
 *
 * A map is three device arrays:
 *   hdr  int32[PCC_MAP_HDR_INTS]  segment table (written by the build kernels)
 *   nbr  int32[...]               per segment a [k_count][pos_count] table of input rows (-1 none)
 *   rows int32[n_out] or NULL     output row of each position (NULL: position == output row)
 * conv:       one segment, all K offsets, positions = output rows; when `rows` is given (non-transposed build) the
 *             positions are the output rows in Morton (Z-curve) order of their coordinates and rows[] receives that
 *             permutation: tiles of consecutive positions are compact 3-D blobs (L1/L2 locality of the gathers).
 * transposed: outputs are grouped by their residue class modulo the up-sampling stride
 *             (stride^3 segments); a class only lists the offsets that can reach it.
 * ---------------------------------------------------------------------------------------- */
/* number of int32 the nbr array needs (upper bound for transposed maps) */
int64_t pcc_map_nbr_elems(int64_t n_out, int32_t kernel_size, int32_t stride, int32_t transposed);
size_t pcc_map_ws_bytes(int64_t n_out);
/* in = out + off_k*step (conv, step = input tensor stride)
 * out = in + off_k*step (transposed, step = output tensor stride, stride = up-sampling factor)
 * *d_pairs (device int64, nullable) receives the number of valid (in,out) pairs. */
int pcc_kernel_map_build(const int64_t* in_keys, int64_t n_in, const int64_t* out_keys, int64_t n_out,
                         int32_t kernel_size, int32_t step, int32_t stride, int32_t transposed,
                         int32_t* hdr, int32_t* nbr, int32_t* rows /*transposed: required; conv: optional (Morton)*/,
                         int64_t* d_pairs, const uint64_t* grid_bits /*nullable*/, const int32_t* grid_rank,
                         const int32_t* h_grid, void* ws, size_t ws_bytes, void* stream);

/* Grid index of the INPUT set of a map (replaces MinkowskiEngine's coordinate hash map for lookups): an occupancy
 * bitmap over the set's bounding lattice plus an exclusive popcount prefix per 64-bit word.  Canonical order equals
 * ascending cell order, so row(cell) = rank[word] + popcount(bits below) -- two coalesced reads per neighbour query.
 * h_grid (host int32[8]) = {lo_x, lo_y, lo_z, cells_x, cells_y, cells_z, pitch (tensor stride), batches}.
 * Without a grid the map build falls back to binary search over the sorted keys. */
int64_t pcc_grid_words(const int32_t* h_grid);
size_t pcc_grid_ws_bytes(int64_t words);
int pcc_grid_build(const int64_t* keys, int64_t n, const int32_t* h_grid, uint64_t* bits /*[words]*/,
                   int32_t* rank /*[words]*/, void* ws, size_t ws_bytes, void* stream);
/* a2-i through the bitmap: strided set = occupancy of the coarse cells.  keys = the FINE canonical set; h_grid = the
 * COARSE lattice (pitch h_grid[6] = new tensor stride, origin a multiple of it).  Marks, ranks and reads the set back
 * out in bitmap (= canonical) order: out_keys (capacity n), *d_count, plus the coarse set's grid index in bits / rank.
 * Same result as pcc_coords_stride without the sort; ws of pcc_grid_ws_bytes(words). */
/* keys may be in ANY order and hold duplicates (marking a cell is idempotent).  d_n (device int64, nullable): the number
 * of valid rows when it is still on the device -- a set derived a moment ago whose size the host has not read; n is then
 * the capacity of keys[].  A chain of strided sets is queued this way without a host read between its links. */
int pcc_coords_stride_grid(const int64_t* keys, int64_t n, const int64_t* d_n, const int32_t* h_grid, uint64_t* bits,
                           int32_t* rank, int64_t* out_keys, int64_t* d_count, void* ws, size_t ws_bytes, void* stream);
/* a1 through the bitmap: canonical order and first-wins de-duplication of USER-ordered keys without a sort.
 * bits / rank = the set's grid index, out_keys (capacity n) = canonical keys, first_user[canonical position] = smallest
 * user row with that coordinate, d_count[0] = number of distinct coordinates, d_count[1] != 0 when some key is off the
 * lattice (results invalid: use pcc_sort_keys + pcc_unique_sorted).  h_grid must cover all keys. */
int pcc_keys_canonicalize_grid(const int64_t* keys, int64_t n, const int32_t* h_grid, uint64_t* bits, int32_t* rank,
                               int64_t* out_keys, int32_t* first_user, int64_t* d_count, void* ws, size_t ws_bytes,
                               void* stream);
/* a3-i through the bitmaps: generative expansion without sorting the n*K candidates.
 *   pcc_coords_expand_grid     : marks the output lattice h_out (pitch ts_out), ranks it and reads the canonical output
 *                                keys back out; bits / rank = grid index of the output set; *d_count = n_out.
 *   pcc_coords_expand_grid_csr : (n_out known) CSR pair lists of the transposed map by probing the INPUT set's grid at
 *                                c - off_k in ascending input row: first[n_out+1], pair_ids[n_in*K] (pair = i*K + k),
 *                                identical to pcc_coords_expand_csr's. */
int pcc_coords_expand_grid(const int64_t* keys, int64_t n, int32_t kernel_size, const int32_t* h_out, uint64_t* bits,
                           int32_t* rank, int64_t* out_keys, int64_t* d_count, void* ws, size_t ws_bytes, void* stream);
/* Transposed convolution on a SUBSET of its output rows (the rows kept by the top-k pruning), straight from their CSR
 * pair lists (pcc_coords_expand_grid_csr on those rows): pairs bucketed by offset, gathered pair GEMM, sum in CSR order.
 * packed_w: pcc_conv_pack_weights layout.  pairs = host value of first[n_out].  T: pcc_convt_rows_t_elems floats. */
size_t pcc_convt_rows_int_ws_bytes(int64_t pairs, int32_t K);
int64_t pcc_convt_rows_t_elems(int64_t pairs, int32_t K, int32_t cout);
int pcc_convt_fwd_rows(const float* feat_in, int64_t n_in, int32_t cin, const float* packed_w, const float* bias,
                       int32_t K, int32_t cout, const int32_t* first, const int32_t* pair_ids, int64_t n_out,
                       int64_t pairs, float* T, float* out, int32_t act, float slope, void* int_ws, size_t int_ws_bytes,
                       int32_t arith /*PCC_ARITH_*, see the convolution section*/, int32_t* d_guard /*nullable*/, void* stream);
/* conv-form map (one segment, nbr[k*n_out + o] = input row or -1) from CSR pair lists: evaluates a transposed conv on a
 * subset of its output rows with pcc_conv_fwd / pcc_conv_fwd_pairs.  hdr: PCC_MAP_HDR_INTS ints, nbr: K*n_out ints. */
int pcc_map_from_csr(const int32_t* first, const int32_t* pair_ids, int64_t n_out, int32_t kernel_size, int32_t* hdr,
                     int32_t* nbr, void* stream);
size_t pcc_expand_grid_csr_ws_bytes(int64_t n_out);
/* d_total (device int64, nullable) receives first[n_out], the number of pairs: lets the caller read that size together
 * with others it is waiting for instead of indexing first[] from the host. */
int pcc_coords_expand_grid_csr(const int64_t* out_keys, int64_t n_out, int32_t kernel_size, int32_t ts_out,
                               const uint64_t* in_bits, const int32_t* in_rank, const int32_t* h_in, int64_t n_in,
                               int32_t* first, int32_t* pair_ids, int64_t* d_total, void* ws, size_t ws_bytes, void* stream);
/* the same lists, kernel offsets of the pair ids numbered z fastest (iz + KS*iy + KS*KS*ix) -- for product buffers laid out
 * [input row][kx][ky][kz][c]: the composite levels gather z-runs of output rows from adjacent memory */
/* The same pair lists in ONE pass (round 4): the 256 rows of a workgroup write into a slot of their own, pair_ids[w * SLOT ...) with
 * SLOT = 256 x the most pairs a row can have ((k+1)/2)^3, so no prefix sum over all rows (and no second probing pass) is needed.
 * first[o] (n_out entries) = absolute start of row o's list; the list ends at first[o + 1], except for the last row of a workgroup
 * (o % 256 == 255, or the last row): wg_end[o / 256].  Same pairs, same order inside a row as pcc_coords_expand_grid_csr[_zk].
 * kernel_size 5 or 7, input pitch >= 2 x output pitch.  pair_ids: pcc_expand_grid_csr_slot_elems(n_out, kernel_size) ints (sized for
 * the worst case; only the written part is touched); wg_end: ceil(n_out / 256) ints; d_total (nullable): receives the pair total. */
int64_t pcc_expand_grid_csr_slot_elems(int64_t n_out, int32_t kernel_size);
int pcc_coords_expand_grid_csr_slots(const int64_t* out_keys, int64_t n_out, int32_t kernel_size, int32_t ts_out,
                                     const uint64_t* in_bits, const int32_t* in_rank, const int32_t* h_in, int64_t n_in,
                                     int32_t* first, int32_t* pair_ids, int32_t* wg_end, int64_t* d_total /*nullable*/, int32_t zk,
                                     void* stream);
int pcc_coords_expand_grid_csr_zk(const int64_t* out_keys, int64_t n_out, int32_t kernel_size, int32_t ts_out,
                               const uint64_t* in_bits, const int32_t* in_rank, const int32_t* h_in, int64_t n_in,
                               int32_t* first, int32_t* pair_ids, int64_t* d_total, void* ws, size_t ws_bytes, void* stream);
/* dense [K][n_out] view of any map (testing / inspection): -1 where no pair */
int pcc_map_to_dense(const int32_t* hdr, const int32_t* nbr, const int32_t* rows, int64_t n_out,
                     int32_t K, int32_t* dense, void* stream);

/* ------------------------------------------------------------------------------------------
 * a2(iii) / a3  sparse convolution forward, output stationary, fp32 MFMA
 *   out[o] = act( bias + sum_k feat_in[nbr_k(o)] @ W[k] )
 * (ME.MinkowskiConvolution / MinkowskiGenerativeConvolutionTranspose forward, 17+5 sites:
 *  model/transforms.py:33-43,127-166; model/entropy_models.py:178-190.)
 * Weights are consumed in a packed layout produced once per parameter update.
 * ---------------------------------------------------------------------------------------- */
/* MFMA-path arithmetic is an ARGUMENT of every convolution entry point (`arith`), never process state: two threads, or the
 * encoder and the decoder of one process, may use different forms at the same time, and a caller that must reproduce a result
 * bit for bit elsewhere (the hyper-synthesis h_s, whose scales / means select the rANS table rows on both sides:
 * model/entropy_models.py:371-400,438-484) names the form it was produced in.
 *   PCC_ARITH_F32  fp32-input MFMA instructions only (v_mfma_f32_32x32x2_f32);
 *   PCC_ARITH_BF6  every fp32 product on the bf16 matrix pipe from an exact three-way bf16 split of both operands (six cross
 *                  terms, fp32 accumulation: 24 bits per element, no range condition, 2.67x the fp32-MFMA rate);
 *   PCC_ARITH_H3   as BF6 for the gathered 3x3x3 convolutions and GDN; the products whose output row depends on ONE input row
 *                  (dense products of the generative transposed convolutions, pair-list GEMMs) as row / column-scaled fp16
 *                  pairs, three MFMA terms, under the range guard below.
 * Range guard of the three-term form.  The form carries every element within 2^-18 of its row / column
 * maximum to >= 22 bits and smaller ones with an absolute error of 2^-28 of that maximum, so a product of depth cin is off by
 * at most cin * 2^-27 * max|row| * max|column| beyond fp32 behaviour.  With `d_guard` non-NULL every fp16-pair launch of the
 * call ORs 1 into *d_guard (device int32, zeroed by the caller) when the scales of one of its tiles admit more than
 * PCC_H_GUARD_BUDGET (absolute, in output units); the caller reads the word with a size it reads anyway and repeats THAT call
 * with PCC_ARITH_BF6.  d_guard is ignored by the other two forms. */
#define PCC_ARITH_F32 0
#define PCC_ARITH_BF6 1
#define PCC_ARITH_H3 2
#define PCC_H_GUARD_BUDGET 2.5e-5f   /* a quarter of the 1e-4 parity bar: max|row| * max|column| > 26 at cin = 128 */
/* 4-channel inputs (the codec's first layer, 4 -> 128, 5x5x5, stride 2): from `rows` output rows on, the (offset, channel)
 * pairs are flattened into one reduction axis and the convolution runs in 32-wide chunks of 8 offsets on the six-term bf16
 * form (default 65536; negative: never).  Tests lower it to reach the path on small inputs. */
int pcc_set_in4_min_rows(int64_t rows);
/* pcc_conv_thin_grid_fwd with one output channel over 16 input channels (the last level's occupancy head): from `rows` rows on
 * the projection pass pre-adds a column's three z terms for the middle row and the gather reads one value per (dx, dy) column
 * (default 2^20; negative: never).  Tests lower it to reach the path on small inputs. */
int pcc_set_thin_z_min_rows(int64_t rows);
int64_t pcc_conv_packed_elems(int32_t K, int32_t cin, int32_t cout);
/* W: ME layout [K, cin, cout] row-major (state_dict `kernel`).  packed_cap: floats available at
 * `packed`; a buffer smaller than pcc_conv_packed_elems(K, cin, cout) is refused (PCC_EWS), never written past. */
int pcc_conv_pack_weights(const float* W, int32_t K, int32_t cin, int32_t cout, float* packed,
                          int64_t packed_cap, void* stream);
/* The same pack read through a transposed / offset-reversed view of a stored kernel: W'[k][ci][co] = W[flip ? K-1-k : k][co][ci]
 * when `transpose` (W stored [K][cout][cin]), else W[flip ? K-1-k : k][ci][co] -- the kernels of the data gradient
 * (reference train.py:221-227 back-propagates through every ME convolution) without a copy in front.  MFMA layout only
 * (cin a multiple of 32, cout > 16); other shapes are refused. */
int pcc_conv_pack_weights_ex(const float* W, int32_t K, int32_t cin, int32_t cout, int32_t transpose, int32_t flip, float* packed,
                             int64_t packed_cap, void* stream);
size_t pcc_conv_ws_bytes(int64_t n_in, int32_t K, int32_t cin, int32_t cout);
/* Occupancy head `predict_i` (model/transforms.py:141-160) in one pass over the features:
 *   logits = conv_k3(relu(conv_k3(x; W0, b0)); W2, b2),  W0: cin -> cmid (4 < cmid <= 16), W2: cmid -> 1.
 * packed_w0: pcc_conv_pack_weights(27, cin, cmid) layout; w2: the second kernel as [27][cmid] (its
 * pcc_conv_pack_weights(27, cmid, 1) layout); hdr/nbr: the canonical 3x3x3 map of the set onto itself;
 * tiles/n_tiles: optional band-ordered tile table (pcc_band_tiles_build) or both NULL; ws: pcc_conv_head_ws_bytes(n). */
int pcc_conv_head_supported(int32_t cin, int32_t cmid);
size_t pcc_conv_head_ws_bytes(int64_t n);
int pcc_conv_head_fwd(const float* feat, int64_t n, int32_t cin, const float* packed_w0, const float* bias0 /*nullable*/,
                      int32_t cmid, const float* w2, const float* bias2 /*nullable [1]*/, const int32_t* hdr,
                      const int32_t* nbr, const int32_t* tiles, const int32_t* n_tiles, float* logits, void* ws,
                      size_t ws_bytes, void* stream);
/* Band-ordered tiles (<= 16 consecutive canonical rows each, word = row0 | (rows-1) << 27) of a single-batch canonical
 * set for the stencil kernels: y cut into `nbands` bands, tiles numbered band-major then x ascending, so that a
 * contiguous tile range sweeps x inside one band and the dx = +-1 neighbour slabs stay in an XCD's L2.
 * lo_x/lo_y: smallest coordinate per axis, nx/ny: lattice cells per axis at pitch ts.  n < 2^27. */
int64_t pcc_band_tiles_cap(int64_t n, int32_t nx, int32_t nbands);
size_t pcc_band_tiles_ws_bytes(int32_t nx, int32_t nbands);
int pcc_band_tiles_build(const int64_t* keys, int64_t n, int32_t lo_x, int32_t nx, int32_t lo_y, int32_t ny, int32_t ts,
                         int32_t nbands, int32_t* tiles, int64_t tiles_cap, int32_t* n_tiles /*device*/, void* ws,
                         size_t ws_bytes, void* stream);
int pcc_conv_fwd(const float* feat_in, int64_t n_in, int32_t cin, const float* packed_w,
                 const float* bias /*nullable [cout]*/, int32_t K, int32_t cout, const int32_t* hdr,
                 const int32_t* nbr, const int32_t* rows, int64_t n_out, float* out, int32_t act,
                 float slope, void* ws, size_t ws_bytes, int32_t arith, int32_t* d_guard /*nullable*/, void* stream);
/* Pair-list form of the same convolution for maps with mostly empty (offset, row) slots (5x5x5 kernels on surfaces):
 * the pairs of each offset are compacted and padded to 128-pair tiles, T[p] = feat[in(p)] @ W[k(p)] runs as a gathered
 * GEMM in which every MFMA row is a real pair, and out[o] = act(bias + sum_k T[pos(k,o)]) is summed in ascending k.
 * Conv maps only (one segment, nbr[k*n_out + o], no row list).  Same results as pcc_conv_fwd up to fp32 summation order.
 *   pcc_pair_plan_rank : pos[K*n_out], pstart[K+1], info[3] = {padded pairs, tiles, pairs}      (device arrays)
 *   pcc_pair_plan_fill : pair_in[padded pairs] (-1 = padding), tile_k[tiles]   -- after the host has read info
 *   pcc_conv_fwd_pairs : T is scratch of padded_pairs*cout floats */
int pcc_conv_pairs_supported(int32_t K, int32_t cin, int32_t cout);
size_t pcc_pair_plan_ws_bytes(int64_t n_out, int32_t K);
int pcc_pair_plan_rank(const int32_t* nbr, int64_t n_out, int32_t K, int32_t* pos, int32_t* pstart, int64_t* info,
                       void* ws, size_t ws_bytes, void* stream);
int pcc_pair_plan_fill(const int32_t* nbr, const int32_t* pos, const int32_t* pstart, int64_t n_out, int32_t K,
                       int64_t padded_pairs, int32_t* pair_in, int32_t* tile_k, void* stream);
int pcc_conv_fwd_pairs(const float* feat_in, int64_t n_in, int32_t cin, const float* packed_w, const float* bias,
                       int32_t K, int32_t cout, const int32_t* pair_in, const int32_t* tile_k, const int64_t* d_info,
                       int64_t padded_pairs, const int32_t* pos, int64_t n_out, float* T, float* out, int32_t act,
                       float slope, int32_t arith, int32_t* d_guard /*nullable*/, void* stream);


/* a3  generative transposed convolution, input stationary (ME.MinkowskiGenerativeConvolutionTranspose forward:
 * model/transforms.py:129,133,137; model/entropy_models.py:186,188).  Every (input row, offset) is one pair, so
 *   T[i][k][:] = feat_in[i] @ W[k]       one dense [n_in,cin] x [cin,K*cout] GEMM on the fp32 MFMA
 *   out[o]     = act(bias + sum_k T[nbr_k(o)][k][:])   ordered gather-sum through the transposed map
 * T: caller scratch of n_in*K*cout floats.  hdr/nbr/rows: a transposed map from pcc_kernel_map_build. */
int64_t pcc_convt_packed_elems(int32_t K, int32_t cin, int32_t cout);
int pcc_convt_pack_weights(const float* W, int32_t K, int32_t cin, int32_t cout, float* packed,
                           int64_t packed_cap, void* stream);
int pcc_convt_fwd(const float* feat_in, int64_t n_in, int32_t cin, const float* packed_w,
                  const float* bias /*nullable [cout]*/, int32_t K, int32_t cout, const int32_t* hdr,
                  const int32_t* nbr, const int32_t* rows, int64_t n_out, float* T, float* out, int32_t act,
                  float slope, int32_t arith, int32_t* d_guard /*nullable*/, void* stream);

/* same with the CSR pair lists of pcc_coords_expand_csr (row pair_id of T); outputs in canonical row order */
int pcc_convt_fwd_csr(const float* feat_in, int64_t n_in, int32_t cin, const float* packed_w,
                      const float* bias /*nullable [cout]*/, int32_t K, int32_t cout, const int32_t* first,
                      const int32_t* pair_ids, int64_t n_out, float* T, float* out, int32_t act, float slope,
                      const int32_t* ex_nbr /*nullable [ex_K][n_out]*/, int32_t ex_K,
                      const float* ex_bias /*[ex_K][cout]*/, int32_t arith, int32_t* d_guard /*nullable*/, void* stream);

/* pcc_convt_fwd_csr with the constant-per-existing-neighbour term (ex_bias [27][cout]) keyed on the OUTPUT set's own grid
 * index (out_keys + pcc_grid_build arrays) instead of a [27][n_out] neighbour table; and a 3x3x3 convolution to <= 4 channels
 * whose neighbours also come straight from the grid index (packed_w: pcc_conv_pack_weights(27, cin, cout) thin layout).
 * Together they spare the composite up+head convolutions the 3x3x3 kernel map of their candidate set. */
int pcc_convt_fwd_csr_grid(const float* feat_in, int64_t n_in, int32_t cin, const float* packed_w, const float* bias /*nullable*/,
                           int32_t K, int32_t cout, const int32_t* first, const int32_t* pair_ids, int64_t n_out, float* T,
                           float* out, int32_t act, float slope, const int64_t* out_keys, const uint64_t* out_bits,
                           const int32_t* out_rank, const int32_t* h_out, const float* ex_bias,
                           const int32_t* wg_end /*nullable: first / pair_ids are the slotted lists of pcc_coords_expand_grid_csr_slots*/,
                           int32_t arith, int32_t* d_guard /*nullable*/, void* stream);
size_t pcc_thin_grid_ws_bytes(int64_t n, int32_t cout);
int pcc_conv_thin_grid_fwd(const float* feat, int64_t n, int32_t cin, const float* packed_w, const float* bias /*nullable*/,
                           int32_t cout, const int64_t* keys, const uint64_t* bits, const int32_t* rank, const int32_t* h_grid,
                           float* out, void* ws, size_t ws_bytes, void* stream);

/* a5  fused GDN / IGDN (GDN1 form), MinkowskiGDN.forward model/blocks.py:26-57:
 *   norm = beta + |x| @ gamma^T ; out = x / norm (inverse=0) or x * norm (inverse=1)
 * beta_raw/gamma_raw are the raw (un-reparametrised) CompressAI parameters; the
 * NonNegativeParametrizer is applied by pcc_gdn_pack. packed: pcc_gdn_packed_elems(c) floats
 * (0 = unsupported channel count), beta_eff: c floats. */
int64_t pcc_gdn_packed_elems(int32_t c);
int pcc_gdn_pack(const float* beta_raw, const float* gamma_raw, int32_t c, float beta_min,
                 float* packed, int64_t packed_cap, float* beta_eff, void* stream);
int pcc_gdn_fwd(const float* x, int64_t n, int32_t c, const float* packed, const float* beta_eff,
                int32_t inverse, float* out, int32_t arith, void* stream);
/* {kernel, row tile, column tile, inverse} of the most recent pcc_gdn_fwd that launched (a call with n <= 0 launches nothing and
 * leaves the record).  GDN launches are not event-timed, so pcc_prof_sequence never lists them; this query costs a few integer
 * stores per call and lets a test READ the regime a call reached.  Process state, like the profiling record; not thread-safe. */
#define PCC_GDN_KERNEL_NONE 0      /* no pcc_gdn_fwd has launched yet */
#define PCC_GDN_KERNEL_CONV_F32 1  /* k_conv_mfma in GDN mode: fp32-input MFMA (c = 8, 16; PCC_ARITH_F32; PCC_MFMA_BUF=0) */
#define PCC_GDN_KERNEL_CONV_BF 2   /* k_conv_mfma_bf in GDN mode: six bf16 terms over planes k_feat_split wrote */
#define PCC_GDN_KERNEL_FUSED 3     /* k_gdn_bf: six bf16 terms, the split folded into the staging */
int pcc_gdn_last_launch(int32_t* h_rec /* [4] */);

/* ------------------------------------------------------------------------------------------
 * Frame intake and hand-over of UnifiedModel.compress / decompress (model/model.py:141-161, 240-250), one launch each.
 * pcc_frame_intake: pc [n,6] fp32 rows (x y z r g b) -> keys of (0, floor x, floor y, floor z), features [n,4] = (1, r, g, b),
 *   out12 (device int32[12]): [0..3] min of (b, floored x y z), [4..7] MINUS their max, [8] != 0: rows already in
 *   canonical (strictly ascending key) order.  ws: pcc_frame_intake_ws_bytes() (per-workgroup
 *   partial results; no global atomics).
 * pcc_decode_finish: keys [n] + colour features [n,3] -> out [n,6] = (x, y, z, clamp(round(255 f), 0, 255) / 255).
 * ---------------------------------------------------------------------------------------- */
/* pcc_coords_intake_i32: int32 [n,4] rows (b, x, y, z) -> keys, out12 as above with [0] / [4] = min b / MINUS max b (the latent
 *   coordinates `decompress` is handed, model/model.py:218-229): pack + bounds + order check in one pass. */
size_t pcc_frame_intake_ws_bytes(void);
int pcc_coords_intake_i32(const int32_t* coords, int64_t n, int64_t* keys, int32_t* out12, void* ws, size_t ws_bytes,
                          void* stream);
int pcc_frame_intake(const float* pc, int64_t n, int64_t* keys, float* feats, int32_t* out12, void* ws, size_t ws_bytes,
                     void* stream);
int pcc_decode_finish(const int64_t* keys, const float* feats3, int64_t n, float* out6, void* stream);

/* ------------------------------------------------------------------------------------------
 * a4  top-k occupancy mask + pruning   (model/transforms.py:228-282, ME.MinkowskiPruning :163)
 * Total order: logit descending, then canonical row ascending.
 * seg_begin: h_ host array [nb+1] of row ranges per batch index, h_k: host array [nb].
 * ---------------------------------------------------------------------------------------- */
size_t pcc_topk_ws_bytes(int64_t n);
int pcc_topk_mask(const float* logits, int64_t stride_elems, const int64_t* h_seg_begin,
                  const int64_t* h_k, int32_t nb, uint8_t* mask, void* ws, size_t ws_bytes,
                  void* stream);
/* the same selection with the kept rows' keys compacted in the same pass (the decoder's "top-k, then prune the coordinates",
 * model/transforms.py:246-282 without the features): keys [rows], keys_out capacity sum_b min(max(k_b,0), rows_b), written
 * batch after batch in canonical order; mask as pcc_topk_mask. */
int pcc_topk_prune_keys(const float* logits, int64_t stride_elems, const int64_t* h_seg_begin,
                        const int64_t* h_k, int32_t nb, const int64_t* keys, uint8_t* mask, int64_t* keys_out,
                        void* ws, size_t ws_bytes, void* stream);
/* row compaction by mask: keys_out/feat_out capacity n; *d_count device int64 */
size_t pcc_prune_ws_bytes(int64_t n);
int pcc_prune_rows(const uint8_t* mask, int64_t n, const int64_t* keys, const float* feat, int32_t c,
                   int64_t* keys_out, float* feat_out, int64_t* d_count, void* ws, size_t ws_bytes,
                   void* stream);

/* a6  SparseTensor.features_at_coordinates for on-grid queries
 * (model/entropy_models.py:294,381,446): out[q] = feat[row(query_keys[q])] or zeros. */
int pcc_lookup_gather(const int64_t* keys, int64_t n, const float* feat, int32_t c,
                      const int64_t* query_keys, int64_t nq, float* out, void* stream);
/* row index of each query (-1 absent) */
int pcc_lookup_rows(const int64_t* keys, int64_t n, const int64_t* query_keys, int64_t nq,
                    int32_t* rows_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * a7  Gaussian conditional, fused      (compressai GaussianConditional as used at
 *                                       model/entropy_models.py:299-333,396-400,468-484)
 * y [n,c]; params [n,2c] = (scales_hat | means_hat) as h_s emits them; gain [nb,c] nullable
 * (scale_nn(q)+eps rows, indexed by the batch field of keys[]; NULL = 1).
 *   s   = max(scales*gain, 0.11)
 *   sym = rint(y*gain - means*gain)            idx = 63 - #{t<63 : s <= table[t]}
 *   lik = max(Phi((.5-|sym|)/s) - Phi((-.5-|sym|)/s), 1e-9)
 * Any of sym/idx/lik may be NULL.
 * ---------------------------------------------------------------------------------------- */
int pcc_gauss_encode(const float* y, const float* params, const int64_t* keys, const float* gain,
                     int64_t n, int32_t c, const float* table, int32_t n_table, int32_t* sym,
                     int32_t* idx, float* lik, void* stream);
/* decode side: y_hat = sym + means*gain (no offsets, model/entropy_models.py:484), idx as above */
int pcc_gauss_decode(const int32_t* sym, const float* params, const int64_t* keys, const float* gain,
                     int64_t n, int32_t c, const float* table, int32_t n_table, float* y_hat,
                     int32_t* idx, void* stream);
/* Rate sweep: the rANS payload estimate (pcc_rans_estimate_bits below, 1/256 bit) of y under each of K candidate gain rows,
 * gains [K, c], every row applied to all n rows of y (one batch).  d_bits256[k] is exactly the integer that
 * pcc_gauss_encode with gain row k (keys of batch 0) followed by pcc_rans_estimate_bits on its sym / idx gives: the same
 * element rules (csrc/pcc_entropy_rule.h), integer sums.  y and params are read once per element, neither sym nor idx is
 * written; one launch, no workspace.  table: the scale table of a7; cdf / sizes / offsets: its rANS tables (n_table rows).
 * Limits: 1 <= K <= 256, c >= 1, 2 <= n_table <= 256, n * c < 2^31; n == 0 zeroes d_bits256 [K] and launches nothing. */
int pcc_gauss_rate_sweep(const float* y, const float* params, int64_t n, int32_t c, const float* gains /*[K,c]*/, int32_t K,
                         const float* table, int32_t n_table, const int32_t* cdf, int32_t cdf_stride, const int32_t* sizes,
                         const int32_t* offsets, int64_t* d_bits256 /*[K], device*/, void* stream);

/* Differentiable Gaussian likelihood of the TRAINING forward (GaussianConditional._likelihood + lower bound 1e-9;
 * model/entropy_models.py:312-316,327-331; rate term loss.py:77-79) on n elements:
 *   lik = max(Phi((.5 - |v - mean|)/s) - Phi((-.5 - |v - mean|)/s), 1e-9),  s = max(scale, 0.11)
 * and its gradients w.r.t. v, scale and mean (CompressAI LowerBound gradient rule on both bounds); mean nullable. */
int pcc_gauss_lik_fwd(const float* v, const float* scale, const float* mean, int64_t n, float* lik, void* stream);
int pcc_gauss_lik_bwd(const float* v, const float* scale, const float* mean, const float* grad_lik, int64_t n,
                      float* dv /*nullable*/, float* dscale /*nullable*/, float* dmean /*nullable*/, void* stream);

/* a8  factorised prior on z            (compressai EntropyBottleneck, model/entropy_models.py:272,
 *                                       282-285,371-372,438); filters (3,3,3,3).
 * eb_packed [c,58]: softplus(matrices) (3,9,9,9,3) | biases (3,3,3,3,1) | tanh(factors) (3,3,3,3);
 * medians [c]. sym = rint(z - med), z_hat = sym + med, lik = |sig(s*u) - sig(s*l)| >= 1e-9. */
int pcc_eb_encode(const float* z, int64_t n, int32_t c, const float* eb_packed, const float* medians,
                  int32_t* sym, float* z_hat, float* lik, void* stream);

/* Differentiable factorised-prior likelihood of the TRAINING forward (EntropyBottleneck._likelihood + lower bound 1e-9;
 * model/entropy_models.py:272,282-285; rate term loss.py:77-79), [n, c] rows, filters (3,3,3,3):
 *   lik = max(|sigmoid(sg up) - sigmoid(sg lo)|, 1e-9),  lo / up = logits(v -+ .5),  sg = -sign(lo + up) (no gradient)
 * backward: dv [n, c] (nullable) and d_packed [c, 58], the gradient of the packed parameters (eb_packed layout: softplus /
 * tanh already applied -- the caller differentiates those reparametrisations), rows summed in a fixed order. */
/* Quantisation-offset network of the training forward (reference model/entropy_models.py:210-233 `quant_nn`, call sites
 * :318-322): a 2 -> 10 -> 10 -> 1 perceptron with ReLUs per element on (scale, stddev), one kernel per direction.
 * params [pcc_quant_mlp_params() = 151]: W1 [10][2] | b1 [10] | W2 [10][10] | b2 [10] | W3 [10] | b3 (torch.nn.Linear layouts).
 * bwd: d_scale / d_stddev nullable; d_params [151] summed in a fixed order (deterministic). */
/* GDN backward, element-wise parts (reference model/blocks.py:38-57; the products n = beta + |x| gamma^T, v = u gamma and
 * d gamma = u^T |x| run on the convolution / weight-gradient entry points):
 *   pre : GDN y = x / n: u = -g x / n^2, dx0 = g / n;  IGDN y = x n: u = g x, dx0 = g n        (elems = rows * C, a multiple of 4)
 *   post: dx += sign(x) v
 *   gamma_eff [C][C] = CompressAI's reparametrisation of gamma_raw (as pcc_gdn_pack applies it)
 *   reparam_bwd: gradients of the RAW parameters from those of the effective ones (LowerBound's rule); d_gamma_t is [ci][co]
 *   as pcc_conv_wgrad(|x|, u) returns it, gamma_raw / d_gamma_raw are [co][ci]. */
int pcc_gdn_bwd_pre(const float* x, const float* g, const float* n, int64_t elems, int32_t inverse, float* u, float* dx0, void* stream);
int pcc_gdn_bwd_post(float* dx, const float* x, const float* v, int64_t elems, void* stream);
int pcc_gdn_gamma_eff(const float* gamma_raw, int32_t c, float* gamma_eff, void* stream);
int pcc_gdn_reparam_bwd(const float* beta_raw, const float* gamma_raw, const float* d_beta, const float* d_gamma_t, int32_t c,
                        float beta_min, float* d_beta_raw, float* d_gamma_raw, void* stream);
/* Focal loss rows of one occupancy level (reference loss.py:115-157 Multiscale_FocalLoss): f[i] = -(occ ? alpha : 1-alpha) *
 * (1-pt)^gamma * log(pt) * q_map[batch(i)][0] with pt = clip(occ ? p : 1-p, 1e-2, 1), p = sigmoid(logit), and df[i] = d f[i] /
 * d logit[i].  occ_row: pcc_lookup_rows of the candidate keys in the ground-truth set (>= 0: occupied); keys: the candidates. */
int pcc_focal_rows(const float* logits, int64_t stride_elems, const int32_t* occ_row, const int64_t* keys, int64_t n,
                   const float* q_map, int32_t q_pitch, float alpha, float gamma, float* f, float* df, void* stream);
int32_t pcc_quant_mlp_params(void);
size_t pcc_quant_mlp_ws_bytes(int64_t n);
int pcc_quant_mlp_fwd(const float* scale, const float* stddev, int64_t n, const float* params, float* out, void* stream);
int pcc_quant_mlp_bwd(const float* scale, const float* stddev, const float* grad_out, int64_t n, const float* params,
                      float* d_scale, float* d_stddev, float* d_params, void* ws, size_t ws_bytes, void* stream);
int pcc_eb_lik_fwd(const float* v, int64_t n, int32_t c, const float* eb_packed, float* lik, void* stream);
int pcc_eb_lik_bwd(const float* v, const float* grad_lik, int64_t n, int32_t c, const float* eb_packed, float* dv,
                   float* d_packed, void* stream);

/* ------------------------------------------------------------------------------------------
 * training (BASELINE config 4; reference train.py:221-227 back-propagates through every ME convolution)
 *   data gradient  : the forward entry points on the inverse map with transposed weights (no extra kernel)
 *   weight gradient: dW[k][ci][co] = sum over pairs (i,o) of offset k of feat_in[i][ci] * grad_out[o][co]
 *                    MFMA GEMM whose reduction runs over the pair list; partial tiles per position slice are summed
 *                    in slice order (deterministic).  hdr/nbr/rows: the FORWARD map (NULL hdr: K = 1 identity).
 *   pcc_convt_scatter_rows: dT[pair] = grad_out[output row of pair] for the input-stationary transposed conv.
 * ---------------------------------------------------------------------------------------- */
size_t pcc_conv_wgrad_ws_bytes(int64_t n_out, int32_t K, int32_t cin, int32_t cout);
int pcc_conv_wgrad(const float* feat_in, int64_t n_in, int32_t cin, const float* grad_out, int64_t n_out, int32_t cout,
                   int32_t K, const int32_t* hdr, const int32_t* nbr, const int32_t* rows, float* dW /*[K,cin,cout]*/,
                   void* ws, size_t ws_bytes, void* stream);
int pcc_convt_scatter_rows(const float* grad_out, const int32_t* first, const int32_t* pair_ids, int64_t n_out,
                           int32_t cout, float* dT /*[n_in*K, cout]*/, void* stream);
/* Convolution over a set mapped onto ITSELF with 1 or 16 output channels (reference model/transforms.py:146-161, predict_*[0] /
 * predict_*[2]; odd K <= 27, stride 1; cout 1 with cin in {16,32,64}, cout 16 with cin in {16,32}): dW[k][ci][co] = sum_i feat[i][ci] * grad_out[nbr_{K-1-k}(i)][co] --
 * input-stationary, the feature rows are streamed once, only the thin gradient rows are gathered.  hdr/nbr: the map of the set
 * onto ITSELF (the caller guarantees in_set == out_set). */
int pcc_conv_wgrad_self_supported(int32_t K, int32_t cin, int32_t cout);
size_t pcc_conv_wgrad_self_ws_bytes(int64_t n, int32_t K, int32_t cin, int32_t cout);
int pcc_conv_wgrad_self(const float* feat, int64_t n, int32_t cin, const float* grad_out /*[n,cout]*/, int32_t cout, int32_t K,
                        const int32_t* hdr, const int32_t* nbr, float* dW /*[K,cin,cout]*/, void* ws, size_t ws_bytes,
                        void* stream);

/* ------------------------------------------------------------------------------------------
 * Channelwise sparse convolution by grid gather (reference loss.py:181-189,219-273: ShepardsLoss' conv_sum over
 * ME.MinkowskiChannelwiseConvolution, the colour-loss ablation configs/CVPR_inverse_scaling_shepard.yaml)
 *   out[q][c] = sum_t W[t][c or 0] * feat[row(q + off_t * step)][c]
 * Input: a canonical set (keys, n) with fp32 features [n][c], 1 <= c <= 64, and optionally its grid index (grid_bits,
 * grid_rank, h_grid as pcc_kernel_map_build takes them; the grid pitch must equal `step`; NULL: binary search).  Queries:
 * arbitrary keys at the set's pitch (members or not, inside its lattice or not, any batch).  Taps: odd kernel_size <= 9,
 * grouped by the caller into ncol (dx, dy) columns, cols int32 [ncol][4] = (dx, dy, zmask, first) in units of `step`, zmask
 * bit k <-> dz = k - kernel_size / 2; widx int32 [ntaps] = weight row of the j-th set bit of a column's zmask at
 * widx[first + j].  Every tap appears in exactly one column and widx is a permutation of 0..ntaps-1.  W is [ntaps][wc] with
 * wc = c, or wc = 1 (broadcast over channels, the reference's (729, 1) window).  Fixed summation order (columns in table order,
 * dz ascending), no atomics: bitwise reproducible, and the grid and search paths give the same bits.
 * The feature gradient of a set mapped onto itself is pcc_chconv_fwd over the set with the negated taps. */
int pcc_chconv_supported(int32_t kernel_size, int32_t c);
int pcc_chconv_fwd(const int64_t* keys, int64_t n, const float* feat, int32_t c, const uint64_t* grid_bits,
                   const int32_t* grid_rank, const int32_t* h_grid, int32_t step, const int32_t* cols, int32_t ncol,
                   const int32_t* widx, int32_t ntaps, int32_t kernel_size, const float* w, int32_t wc,
                   const int64_t* query_keys, int64_t nq, float* out /*[nq, c]*/, void* stream);
/* dW[t][c] = sum_j grad_out[j][c] * feat[row(q_j + off_t * step)][c], summed over c as well when wc = 1: per-workgroup partial
 * slabs [ntaps][c] in `ws` and a fixed-order reduce pass (no atomics). */
size_t pcc_chconv_wgrad_ws_bytes(int64_t nq, int32_t ntaps, int32_t c);
int pcc_chconv_wgrad(const int64_t* keys, int64_t n, const float* feat, int32_t c, const uint64_t* grid_bits,
                     const int32_t* grid_rank, const int32_t* h_grid, int32_t step, const int32_t* cols, int32_t ncol,
                     const int32_t* widx, int32_t ntaps, int32_t kernel_size, const int64_t* query_keys, int64_t nq,
                     const float* grad_out /*[nq, c]*/, float* dW /*[ntaps, wc]*/, int32_t wc, void* ws, size_t ws_bytes,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * 8f-1  rANS entropy coder + CDF tables  (CompressAI `_CXX`: `pmf_to_quantized_cdf`, `BufferedRansEncoder`,
 *       `RansDecoder`; reference call sites model/entropy_models.py:371-372,397-400,438,471,484, model/model.py:30-34)
 * rans64 scheme: 64-bit state, 32-bit words, 16-bit probabilities, 4-bit bypass digits outside a table.
 * Tables: cdf [rows, cdf_stride] int32, sizes[rows] (= pmf length + 2), offsets[rows]; a symbol with table row r is
 * coded as value = symbol - offsets[r] in [0, sizes[r]-2), anything else through the bypass sentinel.
 * ---------------------------------------------------------------------------------------- */
int pcc_pmf_to_quantized_cdf(const float* h_pmf, int32_t n, int32_t precision, int32_t* h_cdf /*[n+1]*/);
/* single stream on HOST buffers: the byte layout of BufferedRansEncoder.flush() */
int64_t pcc_rans_max_bytes(int64_t n);
int pcc_rans_encode_host(const int32_t* h_sym, const int32_t* h_idx, int64_t n, const int32_t* h_cdf,
                         int32_t cdf_stride, const int32_t* h_sizes, const int32_t* h_offsets, uint8_t* h_out,
                         int64_t cap, int64_t* h_nbytes);
int pcc_rans_decode_host(const uint8_t* h_data, int64_t nbytes, const int32_t* h_idx, int64_t n,
                         const int32_t* h_cdf, int32_t cdf_stride, const int32_t* h_sizes, const int32_t* h_offsets,
                         int32_t* h_sym);
/* GPU, n_groups * n_segments independent streams over a row-major [n, channels] int32 symbol matrix.  The matrix is
 * cut into n_groups channel groups (channels/n_groups adjacent channels each, a power of two) and n_segments row
 * segments of R = ceil(n / n_segments) rows; stream s = segment * n_groups + group codes its tile row by row, with table
 * row idx[same element] (idx NULL: row = channel, the factorised prior).  Container (device buffer `out`, capacity
 * pcc_rans_container_max_bytes(pcc_rans_stream_symbols(...), n_groups * n_segments)):
 *   u32 n_streams | u32 nwords[n_streams] | stream words.
 * Every stream is byte-identical to the host single-stream coder run on that tile.  With n_groups = channels and
 * n_segments = 1 the concatenation of the streams is the reference's [1,C,N] channel-major order.  Each stream costs
 * 12 bytes of framing: few streams for rate, many for speed (one lane per stream).  Limits: 65536 streams,
 * n * channels < 2^31. */
int64_t pcc_rans_stream_symbols(int64_t n, int32_t channels, int32_t n_groups, int32_t n_segments); /* longest stream; -1: bad geometry */
int64_t pcc_rans_container_max_bytes(int64_t stream_symbols, int32_t n_streams);
size_t pcc_rans_streams_ws_bytes(int64_t stream_symbols, int32_t n_streams);
/* enc_table (device, required): division-free entries from pcc_rans_build_enc_table (16 bytes per (row, value),
 * layout [rows][cdf_stride]). */
int pcc_rans_build_enc_table(const int32_t* h_cdf, int32_t rows, int32_t cdf_stride, const int32_t* h_sizes,
                             void* h_table /*16*rows*cdf_stride bytes*/);
/* Payload estimate (in 1/256 bit) of a symbol matrix under the tables, independent of any stream geometry and of the
 * order of evaluation (integer sum): the encoder sizes its stream count from it (framing <= 2 % of the payload). */
int pcc_rans_estimate_bits(const int32_t* sym, const int32_t* idx, int64_t n, int32_t channels, const int32_t* cdf,
                           int32_t cdf_stride, const int32_t* sizes, const int32_t* offsets, int64_t* d_bits256 /*device*/,
                           void* stream);
int pcc_rans_encode_streams(const int32_t* sym, const int32_t* idx, int64_t n, int32_t channels,
                            int32_t n_groups, int32_t n_segments, const int32_t* cdf, int32_t cdf_stride,
                            const int32_t* sizes, const int32_t* offsets, const void* enc_table, uint8_t* out,
                            int64_t* d_nbytes, void* ws, size_t ws_bytes, void* stream);
/* compact decoder table (host): 16-bit CDF rows back to back + a 256-bucket start table per row, one blob of
 * pcc_rans_dec_table_bytes() bytes; kept in LDS by pcc_rans_decode_streams when it fits (<= 150 KB), so the per-symbol
 * CDF search runs at LDS latency.  dec_table may be NULL (binary search over the int32 tables in global memory). */
int64_t pcc_rans_dec_table_bytes(int32_t rows, const int32_t* h_sizes);
int pcc_rans_build_dec_table(const int32_t* h_cdf, int32_t rows, int32_t cdf_stride, const int32_t* h_sizes,
                             void* h_blob);
/* *d_status != 0 after the kernel: malformed container.  `data` must be readable 8 bytes past nbytes (look-ahead). */
int pcc_rans_decode_streams(const uint8_t* data, int64_t nbytes, const int32_t* idx, int64_t n, int32_t channels,
                            int32_t n_groups, int32_t n_segments, const int32_t* cdf, int32_t cdf_stride,
                            const int32_t* sizes, const int32_t* offsets, const void* dec_table /*nullable, device*/,
                            int64_t dec_bytes, int32_t* sym_out, int32_t* d_status, void* stream);
/* The same with the decoder form chosen by the caller (tests, A/B runs).  With the table in LDS there are two decoders:
 * form 1, one LANE per stream (256 streams per workgroup), and form 2, one WAVE per stream (the lanes share the symbol
 * search; up to 16 streams per workgroup).  form 0 picks form 2 while one round of workgroups covers all streams and
 * form 1 above that; pcc_rans_decode_streams passes form 0.  Both forms
 * give the same symbols and status words.  Without an LDS table the form is ignored. */
int pcc_rans_decode_streams_form(const uint8_t* data, int64_t nbytes, const int32_t* idx, int64_t n, int32_t channels,
                                 int32_t n_groups, int32_t n_segments, const int32_t* cdf, int32_t cdf_stride,
                                 const int32_t* sizes, const int32_t* offsets, const void* dec_table /*nullable, device*/,
                                 int64_t dec_bytes, int32_t* sym_out, int32_t* d_status, void* stream, int32_t form);

/* ------------------------------------------------------------------------------------------
 * 8f-3  lossless coder for the stride-8 latent coordinates (replaces the PLY file + `tmc3` subprocess round trip of
 *       UnifiedModel.gpcc_encode / gpcc_decode, model/model.py:388-486).  Host buffers.  Octree occupancy bits under an
 *       adaptive binary range coder; stream = u32 n | u8 depth | payload.  Cells are (x,y,z) in [0, 2^depth), unique;
 *       the decoder returns them in Morton order (x most significant).  Not G-PCC syntax; lossless.
 * ---------------------------------------------------------------------------------------- */
int64_t pcc_octree_max_bytes(int64_t n, int32_t depth);
int pcc_octree_encode_host(const int32_t* h_cells /*[n,3]*/, int64_t n, int32_t depth, uint8_t* h_out, int64_t cap,
                           int64_t* h_nbytes);
/* h_cells NULL: only *h_n / *h_depth are returned (size query) */
int pcc_octree_decode_host(const uint8_t* h_data, int64_t nbytes, int32_t* h_cells, int64_t cap_points, int64_t* h_n,
                           int32_t* h_depth);

/* ------------------------------------------------------------------------------------------
 * 8f-3b lossless geometry of a whole block on the device: a breadth-first octree whose levels are the
 *       voxel set's own stride chain, in origin-relative cells 0 <= x, y, z < 2^15 (single batch).  A node's symbol is its
 *       child-occupancy byte 1..255, bit j = child (dx, dy, dz) with j = dx<<2 | dy<<1 | dz (ascending key order); its context
 *       is the 6-bit pattern of face neighbours present in the node's own level (bit 0/1: -x/+x, 2/3: -y/+y, 4/5: -z/+z).
 *       The symbols travel through pcc_rans_encode_streams / pcc_rans_decode_streams as an [nodes, 1] matrix, idx = context.
 *       None of these reads a bitstream; symbols outside 1..255 set *d_bad (device int32, zeroed by the caller) and count as 1.
 * pcc_geom_occ_ctx       ctx[i] (and, with sym non-NULL, the byte sym[i]) of every node of a canonical level at `pitch`.
 *                        bits / rank / h_grid: the level's grid index (pcc_grid_build layout, pitch h_grid[6] == pitch), or NULL:
 *                        binary search over keys.  child_*: the canonical set at pitch / 2 and its grid index (or NULL), needed
 *                        for the bytes only.
 * pcc_geom_hist          hist[pcc_geom_hist_words() = 64 * 256 + 8] (uint32, zeroed here): hist[ctx * 256 + byte] counts, then
 *                        the popcount histogram (entry k: nodes with k + 1 children).  Integer atomics, reduced in LDS per
 *                        workgroup first: the sums do not depend on arrival order.
 * pcc_geom_child_offsets off[n + 1] = exclusive scan of the nodes' child counts (off[n] = *d_total, device int64): the host
 *                        compares the total with the stream header before anything is sized by it.  n < 2^27.
 *                        ws: pcc_geom_offsets_ws_bytes(n); a short buffer returns PCC_EWS.
 * pcc_geom_expand        out_keys[off[i] + r] = key of the r-th child of node i (child pitch = node pitch / 2), parent-major;
 *                        writes at or past `cap` (>= n) are dropped.  Canonical order: pcc_keys_canonicalize_grid / pcc_sort_keys.
 * pcc_geom_finish        cell keys + origin -> absolute keys (nullable) and int32 [n, 3] rows (x, y, z) (nullable).
 * pcc_geom_tables        the decoder's tables of one level without a host round trip: from the adaptive counts state[64 * 256]
 *                        (uint64, device) and the level's popcount histogram h_pop[8] (HOST, from the stream header), the integer
 *                        rule of DESIGN.md 7e -> cdf int32 [64, 257] and the decoder table blob of pcc_rans_build_dec_table
 *                        (pcc_geom_dec_table_bytes() bytes, its padding zeroed by the caller), both on the device.
 * pcc_geom_state_update  state = (state >> 1) + hist (the first 64 * 256 words of a pcc_geom_hist result).
 * ---------------------------------------------------------------------------------------- */
int pcc_geom_occ_ctx(const int64_t* keys, int64_t n, int32_t pitch, const uint64_t* bits, const int32_t* rank,
                     const int32_t* h_grid, const int64_t* child_keys, int64_t n_child, const uint64_t* child_bits,
                     const int32_t* child_rank, const int32_t* h_child, int32_t* sym /*nullable*/, int32_t* ctx, void* stream);
int32_t pcc_geom_hist_words(void);
int pcc_geom_hist(const int32_t* sym, const int32_t* ctx, int64_t n, uint32_t* hist, int32_t* d_bad, void* stream);
size_t pcc_geom_offsets_ws_bytes(int64_t n);
int pcc_geom_child_offsets(const int32_t* sym, int64_t n, int32_t* off /*[n+1]*/, int64_t* d_total, int32_t* d_bad, void* ws,
                           size_t ws_bytes, void* stream);
int pcc_geom_expand(const int64_t* keys, const int32_t* sym, const int32_t* off, int64_t n, int32_t child_pitch,
                    int64_t* out_keys, int64_t cap, void* stream);
int pcc_geom_finish(const int64_t* keys, int64_t n, int32_t ox, int32_t oy, int32_t oz, int64_t* out_keys /*nullable*/,
                    int32_t* out_xyz /*nullable [n,3]*/, void* stream);
int64_t pcc_geom_dec_table_bytes(void);
int pcc_geom_tables(const uint64_t* state, const uint32_t* h_pop, int32_t* cdf, void* dec_table, void* stream);
int pcc_geom_state_update(uint64_t* state, const uint32_t* hist, void* stream);

/* ------------------------------------------------------------------------------------------
 * 8f-3b' inter-frame lossless geometry (stream format 0xA8): the levels at and below the block pitch
 *       2^block_log2 (block_log2 <= 4; a block is a node of that level) are coded against a reference cloud displaced per block
 *       by one of the (2 search + 1)^3 integer vectors, search <= 2, ordered by |v|^2 and then lexicographically (index 0 = zero).
 *       The displaced reference is held as one occupancy pyramid per block, pcc_geom_inter_pyramid_words() = 75 uint64 words:
 *       tier e (cells of side 2^(block_log2 - e), bit lx << 2e | ly << e | lz) at word 0 / 64 / 72 / 73 / 74 for e = 4 .. 0.
 *       The reference set is given in ABSOLUTE coordinates with its pitch-1 grid index (or three NULLs: binary search; n_ref == 0:
 *       an empty reference); (ox, oy, oz) is the origin the coder's cells are relative to.  Integers only, no arrival order.
 * pcc_geom_inter_candidates  HOST: the vector table h_out[n, 3] (nullable) of a search range; returns n, -1 on a bad range.
 * pcc_geom_inter_block_bits  pyramid[b] of every block: cell p is set when source(origin + p - v[vec[b]]) is occupied; vec NULL:
 *                            no displacement.  An index outside the table sets *d_bad and counts as 0.
 * pcc_geom_inter_motion      vec[b] = the candidate with the most voxels p of the block (cur_pyramid, built from the current frame
 *                            itself) for which reference(origin + p - v) is occupied; ties to the lowest index.  counts
 *                            (nullable) receives the [n_blocks, candidates] match counts.
 * pcc_geom_inter_occ_ctx     the counterpart of pcc_geom_occ_ctx for a level at 2 <= pitch <= 2^block_log2: idx[i] = context +
 *                            64 * present, r[i] (nullable) = the predicted node's child byte (0: absent); with byte / sym
 *                            non-NULL (encoder, needs the child set) the occupancy byte and the coded symbol: the byte for an
 *                            absent node, rho^-1(byte ^ r) for a present one, rho = 0..255 ordered by (popcount, value).
 *                            block_*: the canonical level at pitch 2^block_log2 and its grid index (or NULLs).
 * pcc_geom_inter_map         inverse != 0: out = the byte of symbol in[i] under (idx, r); else the symbol of byte in[i].  What
 *                            cannot occur (an absent node's value outside 1..255, a present node's byte 0) sets *d_bad, byte 1.
 * pcc_geom_inter_hist        hist[pcc_geom_inter_hist_words() = 128 * 256 + 8 + 9] (uint32, zeroed here): hist[idx * 256 + sym],
 *                            then the popcount classes of the absent nodes and the distance classes popcount(byte ^ r) of the
 *                            present ones.  Integer atomics, reduced in LDS (32 rows per workgroup) first.
 * pcc_geom_inter_tables      the decoder's 128 rows of one level from state[128 * 256] (uint64, device; rows 0..63 are the state of
 *                            pcc_geom_tables) and the HOST class histograms: cdf int32 [128, 258] (rows 0..63: 257 entries) and
 *                            the decoder table blob (pcc_geom_inter_dec_table_bytes(), padding zeroed by the caller).
 *                            The state is updated by pcc_geom_state_update on each half.
 * ---------------------------------------------------------------------------------------- */
int32_t pcc_geom_inter_pyramid_words(void);
int32_t pcc_geom_inter_candidates(int32_t search, int32_t* h_out /*nullable [n,3]*/);
int pcc_geom_inter_block_bits(const int64_t* block_keys, int64_t n_blocks, int32_t block_log2, const int64_t* src_keys,
                              int64_t n_src, const uint64_t* src_bits, const int32_t* src_rank, const int32_t* h_src,
                              int32_t ox, int32_t oy, int32_t oz, const int32_t* vec /*nullable*/, int32_t search, uint64_t* pyramid,
                              int32_t* d_bad, void* stream);
int pcc_geom_inter_motion(const int64_t* block_keys, int64_t n_blocks, int32_t block_log2, const uint64_t* cur_pyramid,
                          const int64_t* ref_keys, int64_t n_ref, const uint64_t* ref_bits, const int32_t* ref_rank,
                          const int32_t* h_ref, int32_t ox, int32_t oy, int32_t oz, int32_t search, int32_t* counts /*nullable*/,
                          int32_t* vec, void* stream);
int pcc_geom_inter_occ_ctx(const int64_t* keys, int64_t n, int32_t pitch, const uint64_t* bits, const int32_t* rank,
                           const int32_t* h_grid, const int64_t* child_keys, int64_t n_child, const uint64_t* child_bits,
                           const int32_t* child_rank, const int32_t* h_child, const int64_t* block_keys, int64_t n_blocks,
                           const uint64_t* block_bits, const int32_t* block_rank, const int32_t* h_block, int32_t block_log2,
                           const uint64_t* pyramid, int32_t* byte /*nullable*/, int32_t* sym /*nullable*/, int32_t* r /*nullable*/,
                           int32_t* idx, void* stream);
int pcc_geom_inter_map(const int32_t* in, const int32_t* idx, const int32_t* r, int64_t n, int32_t inverse, int32_t* out,
                       int32_t* d_bad, void* stream);
int32_t pcc_geom_inter_hist_words(void);
int pcc_geom_inter_hist(const int32_t* sym, const int32_t* idx, int64_t n, uint32_t* hist, int32_t* d_bad, void* stream);
int64_t pcc_geom_inter_dec_table_bytes(void);
int pcc_geom_inter_tables(const uint64_t* state, const uint32_t* h_pop, const uint32_t* h_dist, int32_t* cdf, void* dec_table,
                          void* stream);

/* ------------------------------------------------------------------------------------------
 * 8f-3b* wide block motion of the inter coders (DESIGN.md section 7e "Wide search", stream format 0xAA): the search of 8f-3b' over
 *       [-search, search]^3 with 1 <= search <= 7.  A vector is a DISPLACEMENT, int32 (dx + 8) | (dy + 8) << 4 | (dz + 8) << 8, never
 *       an index into a table.  Blocks, pyramids, the reference set and the origin are given as in 8f-3b'.
 * pcc_geom_wide_motion      disp[b] = the vector with the most voxels p of the block for which reference(origin + p - v) is
 *                           occupied; ties to the smaller dx^2 + dy^2 + dz^2, then to the lexicographically smaller (dx, dy, dz):
 *                           for search <= 2 the vector pcc_geom_inter_motion picks.  counts (nullable) receives the match counts
 *                           [n_blocks, (2 search + 1)^3] in plain lexicographic (dx, dy, dz) order.  No atomics, integers only.
 * pcc_geom_wide_block_bits  pcc_geom_inter_block_bits with disp[b] in place of an index (disp is required).  A component outside
 *                           +-search (or a bit above the 12) sets *d_bad and the block's vector counts as zero.
 * pcc_geom_wide_pack        disp[i] from comps[i] = (dx + search, dy + search, dz + search), what an 0xAA vector list codes; a
 *                           component outside 0 .. 2 search sets *d_bad and counts as zero displacement on that axis.
 * pcc_geom_wide_unpack      the inverse (a displacement outside the range unpacks as zero).
 * ---------------------------------------------------------------------------------------- */
int pcc_geom_wide_motion(const int64_t* block_keys, int64_t n_blocks, int32_t block_log2, const uint64_t* cur_pyramid,
                         const int64_t* ref_keys, int64_t n_ref, const uint64_t* ref_bits, const int32_t* ref_rank,
                         const int32_t* h_ref, int32_t ox, int32_t oy, int32_t oz, int32_t search, int32_t* counts /*nullable*/,
                         int32_t* disp, void* stream);
int pcc_geom_wide_block_bits(const int64_t* block_keys, int64_t n_blocks, int32_t block_log2, const int64_t* src_keys,
                             int64_t n_src, const uint64_t* src_bits, const int32_t* src_rank, const int32_t* h_src,
                             int32_t ox, int32_t oy, int32_t oz, const int32_t* disp, int32_t search, uint64_t* pyramid,
                             int32_t* d_bad, void* stream);
int pcc_geom_wide_pack(const int32_t* comps, int64_t n, int32_t search, int32_t* disp, int32_t* d_bad, void* stream);
int pcc_geom_wide_unpack(const int32_t* disp, int64_t n, int32_t search, int32_t* comps, void* stream);

/* ------------------------------------------------------------------------------------------
 * 8f-3b** several references per frame (DESIGN.md section 7e "Several references", stream format 0xAB): every block takes its
 *       prediction from one of n_slots (1..4) reference slots.  A slot is a reference set of 8f-3b': ref_keys[s], n_ref[s] (0: an
 *       empty slot), and its pitch-1 grid index ref_bits[s] / ref_rank[s] / h_ref[s] (NULLs: binary search); the five arrays are
 *       HOST arrays of n_slots entries.  Blocks, pyramids and the origin as in 8f-3b', vectors as packed displacements of 8f-3b*
 *       with 1 <= search <= 7.  One wave per block; no atomics, integers only.
 * pcc_geom_multi_block_bits
 *   encoder form (cur_pyramid given): vecs[n_slots, n_blocks] holds every slot's own vector for every block.  For each slot in
 *       order the slot's pyramid under its vector is built and its match count c = |finest tier AND cur_pyramid's| taken; the
 *       block keeps the slot with the largest count, the LOWER slot on a tie.  Writes sel[b], disp[b] (the chosen slot's vector),
 *       pyramid[b] (its pyramid) and, with counts non-NULL, counts[n_blocks, n_slots].
 *   decoder form (cur_pyramid NULL): sel[n_blocks] is an INPUT and vecs[n_blocks] the one vector per block the stream carries;
 *       pyramid[b] is the pyramid of slot sel[b] under vecs[b].  disp and counts are not used (counts must be NULL).
 *   A selector outside 0 .. n_slots - 1 counts as slot 0, a displacement outside +-search as zero; either sets *d_bad.
 * ---------------------------------------------------------------------------------------- */
int pcc_geom_multi_block_bits(const int64_t* block_keys, int64_t n_blocks, int32_t block_log2, int32_t n_slots,
                              const int64_t* const* ref_keys, const int64_t* n_ref, const uint64_t* const* ref_bits,
                              const int32_t* const* ref_rank, const int32_t* const* h_ref, int32_t ox, int32_t oy, int32_t oz,
                              const int32_t* vecs, int32_t search, const uint64_t* cur_pyramid /*nullable*/, int32_t* sel,
                              int32_t* disp /*nullable*/, uint64_t* pyramid, int32_t* counts /*nullable*/, int32_t* d_bad, void* stream);

/* ------------------------------------------------------------------------------------------
 * 8f-3b'' global motion of the inter coders (DESIGN.md section 7e "Global motion"; motion.py): one rigid transform per frame,
 *       applied to the reference before the block motion of 8f-3b'.
 *       The transform is 12 int32 on the HOST: M[3][3] row-major in Q24, then t[3] in Q8 voxels; |M_ij| <= PCC_MOTION_MAX_M,
 *       |t_i| < PCC_MOTION_MAX_T, else PCC_EINVAL before any launch.
 * pcc_motion_warp       out_keys[i] = the key of q, q_k = (sum_j M_kj p_j + (t_k << 16) + 2^23) >> 24 in int64 (the shift
 *                       floors), p the voxel of keys[i] (a pitch-1 key array in any order, duplicates allowed; the batch index is
 *                       carried); PCC_MOTION_DROPPED when a coordinate of q is outside [-2^15 + 64, 2^15 - 64), the range a
 *                       coordinate set holds -- nothing else is written for such a row.  d_info (device int32 [8], the caller sets
 *                       {INT32_MAX x3, INT32_MIN x3, 0, 0}): min q | max q over the kept rows | number of dropped rows | unused;
 *                       integer atomics, so the values do not depend on arrival order.
 *                       The warped cloud is the set of distinct kept keys: pcc_sort_keys (stable, with its permutation) and
 *                       pcc_unique_sorted over out_keys; PCC_MOTION_DROPPED sorts behind every key.  Over a canonical input the
 *                       first row of a run is the source of LOWEST CANONICAL RANK: the winner whose attributes the cell carries.
 * pcc_motion_gather     out[u, :] = attrs[perm[first[u]], :] for u < n_out: the uint8 [n_src, c] rows (1 <= c <=
 *                       PCC_MOTION_MAX_ATTRS) of the winners, perm / first as those two entry points left them (indices are clamped
 *                       into [0, n_src): nothing is read outside the arrays).
 * pcc_motion_icp_terms  the normal-equation terms of one point-to-plane ICP iteration for the transform h_rt = R[3][3] row-major,
 *                       t[3] (HOST, fp64).  Per reference voxel p, in the order of ref_keys (one thread each): x = R p + t;
 *                       candidates are the voxels c of the CURRENT frame (cur_keys: canonical, pitch 1; grid_* its pcc_grid_build
 *                       index or NULL bits: binary search, same bits out) with |c_k - floor(x_k + 0.5)| <= ceil(radius) on every
 *                       axis and |c - x|^2 < radius^2; the match is the candidate of least |c - x|^2, the lowest canonical rank on a
 *                       tie; no candidate: the voxel adds nothing.  With n the normal at c (normals fp32 [n_cur, 3], those of
 *                       pcc_normals_grid) and g = h_centre[3]: a = [(x - g) x n, n], b = (c - x) . n, and
 *                       out[PCC_MOTION_ICP_SUMS] (device fp64) = the 21 entries a_i a_j, i <= j, row by row | the 6 entries a_i b |
 *                       the number of matches | sum |c - x|^2.  Every product and sum is a separate fp64 rounding in the order
 *                       written in csrc/pcc_motion.hip; a wave's terms meet in an xor butterfly, the waves and then the workgroups'
 *                       partials (ws: pcc_motion_icp_ws_bytes(n_ref), a short buffer returns PCC_EWS) are added in index order: no
 *                       floating-point atomics, two calls give the same bits.  match (nullable int32 [n_ref]): the matched rank
 *                       or -1.  0 < radius <= 4.
 * ---------------------------------------------------------------------------------------- */
#define PCC_MOTION_MAX_M (1 << 25)
#define PCC_MOTION_MAX_T (1 << 24)
#define PCC_MOTION_MAX_ATTRS 8
#define PCC_MOTION_ICP_SUMS 29
#define PCC_MOTION_DROPPED 0x7FFFFFFFFFFFFFFFll
int pcc_motion_warp(const int64_t* keys, int64_t n, const int32_t* h_transform /*[12]*/, int64_t* out_keys /*[n]*/,
                    int32_t* d_info /*[8]*/, void* stream);
int pcc_motion_gather(const uint8_t* attrs, int32_t c, int64_t n_src, const int32_t* perm, const int32_t* first, int64_t n_out,
                      uint8_t* out /*[n_out,c]*/, void* stream);
size_t pcc_motion_icp_ws_bytes(int64_t n_ref);
int pcc_motion_icp_terms(const int64_t* ref_keys, int64_t n_ref, const int64_t* cur_keys, int64_t n_cur,
                         const uint64_t* grid_bits /*nullable*/, const int32_t* grid_rank, const int32_t* h_grid,
                         const float* normals /*[n_cur,3]*/, const double* h_rt /*[12]*/, const double* h_centre /*[3]*/,
                         double radius, double* out /*[PCC_MOTION_ICP_SUMS]*/, int32_t* match /*nullable [n_ref]*/, void* ws,
                         size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * 8f-3c RAHT colour coder over the level sets of 8f-3b: the anchor the reference compares against is
 *       `tmc3 --transformType=0` (`utils.py:505-529`); this is the same transform family in our own stream, no G-PCC syntax.
 *       A level is given as its canonical node keys at `pitch` plus the canonical child set at pitch / 2 with that set's grid
 *       index (child_bits / child_rank / h_child, pcc_grid_build layout; three NULLs: binary search over child_keys).  Child j of
 *       a node is (dx, dy, dz), j = dx<<2 | dy<<1 | dz.  Values are Q8 int32 [rows, channels], 1 <= channels <= 8; weights int32.
 *       Coefficient rows: a node with m children emits m - 1 rows (stage 3, stage 2 slots 0 and 4, stage 1 slots 0 2 4 6) from row
 *       row_base + off[i] - i of one [rows_total, channels] matrix shared by all levels (row_base = nodes(level) - 1, off from
 *       pcc_geom_child_offsets over the masks); rows at or past rows_total are never touched.  n, n_child < 2^26.
 * pcc_raht_isqrt / pcc_raht_butterfly  HOST: the kernels' own arithmetic for the CPU tests.  isqrt: exact floor square root
 *                      (x < 2^62, else 0).  butterfly: h_out[6] = a, b (Q30 factors of weights w1, w2), L, H, and the inverse's x1, x2.
 * pcc_raht_prepare     uint8 attrs [n, channels] (row perm[i] of the caller's order, perm NULL: row i) -> Q8 values; colour != 0
 *                      (channels == 3): the integer BT.709 transform of DESIGN.md 7f instead of v << 8.
 * pcc_raht_mask        mask[i] = child-occupancy byte of node i.
 * pcc_raht_weights     w[i] = sum of the children's weights (child_w NULL: the children are voxels of weight 1).
 * pcc_raht_forward     w[i], v[i, :] (the node's DC) and the node's quantised coefficients, q = sign(H) * ((|H| + step / 2) / step)
 *                      with h_steps[channels] (HOST, Q8).
 * pcc_raht_inverse     child_v of every child from v, the rows' q * step (clamped to +-2^30 like every butterfly output; a clamp
 *                      sets bit 0 of *d_flag, device int32 zeroed by the caller).
 * pcc_raht_index       idx[row, c] of a level's rows from its masks: side NULL: the group level * 6 + (c ? 3 : 0) + stage - 1;
 *                      else side[group] & 63 (device int32 [levels * 6]), the table member of that group.
 * pcc_raht_hist        hist[groups * 128] (uint32, zeroed here; groups <= 90): hist[grp * 128 + value + 63], values outside
 *                      -63 .. 63 in slot 127.  Integer atomics, reduced in LDS per workgroup first.
 * pcc_raht_finish      Q8 values -> uint8: (v + 128) >> 8 clamped, or the inverse colour transform (colour != 0, channels == 3).
 * ---------------------------------------------------------------------------------------- */
uint64_t pcc_raht_isqrt(uint64_t x);
int pcc_raht_butterfly(uint32_t w1, uint32_t w2, int64_t x1, int64_t x2, int64_t* h_out /*[6]*/);
int pcc_raht_prepare(const uint8_t* attrs, const int64_t* perm /*nullable*/, int64_t n, int32_t channels, int32_t colour,
                     int32_t* values, void* stream);
int pcc_raht_mask(const int64_t* keys, int64_t n, int32_t pitch, const int64_t* child_keys, int64_t n_child,
                  const uint64_t* child_bits, const int32_t* child_rank, const int32_t* h_child, int32_t* mask, void* stream);
int pcc_raht_weights(const int64_t* keys, int64_t n, int32_t pitch, const int64_t* child_keys, int64_t n_child,
                     const uint64_t* child_bits, const int32_t* child_rank, const int32_t* h_child,
                     const int32_t* child_w /*nullable*/, int32_t* w, void* stream);
int pcc_raht_forward(const int64_t* keys, int64_t n, int32_t pitch, const int64_t* child_keys, int64_t n_child,
                     const uint64_t* child_bits, const int32_t* child_rank, const int32_t* h_child, const int32_t* off,
                     const int32_t* child_w /*nullable*/, const int32_t* child_v, int32_t channels, const int32_t* h_steps,
                     int32_t* w, int32_t* v, int32_t* coef, int64_t row_base, int64_t rows_total, void* stream);
int pcc_raht_inverse(const int64_t* keys, int64_t n, int32_t pitch, const int64_t* child_keys, int64_t n_child,
                     const uint64_t* child_bits, const int32_t* child_rank, const int32_t* h_child, const int32_t* off,
                     const int32_t* child_w /*nullable*/, const int32_t* v, int32_t channels, const int32_t* h_steps,
                     const int32_t* coef, int64_t row_base, int64_t rows_total, int32_t* child_v, int32_t* d_flag, void* stream);
int pcc_raht_index(const int32_t* mask, const int32_t* off, int64_t n, int32_t level, int32_t channels,
                   const int32_t* side /*nullable*/, int32_t* idx, int64_t row_base, int64_t rows_total, void* stream);
int pcc_raht_hist(const int32_t* sym, const int32_t* grp, int64_t n_sym, int32_t groups, uint32_t* hist, void* stream);
int pcc_raht_finish(const int32_t* values, int64_t n, int32_t channels, int32_t colour, uint8_t* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * 8f-3c' inter frames of the RAHT colour coder (DESIGN.md section 7f "Inter frames", stream 0xB4): a prediction signal P (Q8
 *       int32 [n, channels]) over the CURRENT voxels goes through the same integer forward transform as the source, over the
 *       same geometry and weights, and a row travels as quantise(H - Hp); the decoder forms Hp the same way and adds it to
 *       q * step.  Blocks, block grid and block_log2 as in 8f-3e (the nodes of level max(0, depth - 4)); match from
 *       pcc_lift_inter_match; ref_values int32 [n_ref, channels] from pcc_raht_prepare over the reference's levels.  Levels are
 *       given as in 8f-3c.  d_flag: device int32 zeroed by the caller; bit 0 is set by a block row, a mode or a match outside
 *       its range (counted as mode 0 / unmatched) and by the clamps of the inverse.
 * pcc_raht_inter_fill     sums [n_blocks, channels + 1] int32 (cleared here): per channel the sum of ref_values over the block's
 *                         matched voxels, then their count.  pred[i] = ref_values[match[i]], or for an unmatched voxel
 *                         floor(sum / count) of its block; zero in a block without a match and, with mode != NULL (decoder),
 *                         in a block of mode 0.
 * pcc_raht_inter_forward  pcc_raht_forward over child_v and child_p in one pass: w, v and p (the prediction's DC) of the node,
 *                         coef = quantise(H) and coef_p = quantise(H - Hp) at the node's rows.  sums != NULL (a level inside the
 *                         blocks, pitch <= 2^block_log2): sums [n_blocks, 2] int32 (zeroed by the caller, accumulated over the
 *                         levels) += sum |coef|, sum |coef_p| of the node's rows over all channels.  sums == NULL (a level above
 *                         the blocks): the block arguments are ignored.
 * pcc_raht_inter_modes    mode[b] = sums[b, 1] < sums[b, 0] and fill_sums[b, channels] > 0; block_p [n_blocks, channels] (the p
 *                         of the block level) is zeroed for a mode-0 block, so the levels above see the decision.
 * pcc_raht_inter_select   a level >= depth - block_log2: idx of its rows: group (mode ? depth : level) * 6 + 3 * (channel > 0) +
 *                         stage, or side[group] & 63; coef != NULL (encoder): rows of mode-0 blocks are copied from coef into
 *                         coef_p.  mask / off as for pcc_raht_index.
 * pcc_raht_inter_predict  decoder: p (DC) of the node and the unquantised Hp of its rows into hp [rows_total, channels].
 * pcc_raht_inter_inverse  pcc_raht_inverse with H = hp + q * step (both terms and the sum clamped to +-2^30) and, dc_p != NULL
 *                         (the root), DC = v + dc_p.
 * ---------------------------------------------------------------------------------------- */
int pcc_raht_inter_fill(const int64_t* voxel_keys, int64_t n, const int64_t* block_keys, int64_t n_blocks,
                        const uint64_t* block_bits, const int32_t* block_rank, const int32_t* h_block, int32_t block_log2,
                        const int32_t* match, const int32_t* ref_values /*nullable when n_ref == 0*/, int64_t n_ref,
                        int32_t channels, const int32_t* mode /*nullable*/, int32_t* sums, int32_t* pred, int32_t* d_flag,
                        void* stream);
int pcc_raht_inter_forward(const int64_t* keys, int64_t n, int32_t pitch, const int64_t* child_keys, int64_t n_child,
                           const uint64_t* child_bits, const int32_t* child_rank, const int32_t* h_child,
                           const int64_t* block_keys, int64_t n_blocks, const uint64_t* block_bits, const int32_t* block_rank,
                           const int32_t* h_block, int32_t block_log2, const int32_t* off, const int32_t* child_w /*nullable*/,
                           const int32_t* child_v, const int32_t* child_p, int32_t channels, const int32_t* h_steps, int32_t* w,
                           int32_t* v, int32_t* p, int32_t* coef, int32_t* coef_p, int64_t row_base, int64_t rows_total,
                           int32_t* sums /*nullable*/, int32_t* d_flag /*nullable without sums*/, void* stream);
int pcc_raht_inter_modes(const int32_t* sums, const int32_t* fill_sums, int64_t n_blocks, int32_t channels, int32_t* mode,
                         int32_t* block_p, void* stream);
int pcc_raht_inter_select(const int64_t* keys, const int32_t* mask, const int32_t* off, int64_t n, int32_t level, int32_t depth,
                          int32_t channels, const int64_t* block_keys, int64_t n_blocks, const uint64_t* block_bits,
                          const int32_t* block_rank, const int32_t* h_block, int32_t block_log2, const int32_t* mode,
                          const int32_t* side /*nullable*/, int32_t* idx, int32_t* coef_p /*nullable*/,
                          const int32_t* coef /*nullable*/, int64_t row_base, int64_t rows_total, int32_t* d_flag, void* stream);
int pcc_raht_inter_predict(const int64_t* keys, int64_t n, int32_t pitch, const int64_t* child_keys, int64_t n_child,
                           const uint64_t* child_bits, const int32_t* child_rank, const int32_t* h_child, const int32_t* off,
                           const int32_t* child_w /*nullable*/, const int32_t* child_p, int32_t channels, int32_t* p, int32_t* hp,
                           int64_t row_base, int64_t rows_total, void* stream);
int pcc_raht_inter_inverse(const int64_t* keys, int64_t n, int32_t pitch, const int64_t* child_keys, int64_t n_child,
                           const uint64_t* child_bits, const int32_t* child_rank, const int32_t* h_child, const int32_t* off,
                           const int32_t* child_w /*nullable*/, const int32_t* v, const int32_t* dc_p /*nullable*/,
                           int32_t channels, const int32_t* h_steps, const int32_t* coef, const int32_t* hp, int64_t row_base,
                           int64_t rows_total, int32_t* child_v, int32_t* d_flag, void* stream);

/* ------------------------------------------------------------------------------------------
 * 8f-3c" prediction from the parent level in the RAHT colour coder (DESIGN.md section 7f "Prediction from the parent level",
 *       stream 0xB9): the rows, steps and groups of 8f-3c, every row coded as quantise(H - Hp).  Per node of a level with
 *       reconstructed DC D and weight w: its mean m = (a D + 2^29) >> 30, a = isqrt(((1 << 32) / w) << 28), clamped to +-2^24;
 *       child (dx, dy, dz) is predicted from the means of the present cells node + d * b of the node's own level by the 27 / 9 /
 *       3 / 1 rule of 8f-3d; P = (pred * isqrt(w_child << 32) + 2^15) >> 16, clamped to +-2^30; Hp = the node's three butterfly
 *       stages over the present children's P with the children's weights; the decoder takes H = Hp + q * step (both terms and
 *       the sum clamped to +-2^30) and the inverse butterflies of pcc_raht_inverse with L = D.  Closed loop: the encoder runs
 *       pcc_raht_forward with every step 1 (h_true = the unquantised H rows), then pcc_raht_pred_root and pcc_raht_pred_encode
 *       level by level from the root.  A level is given as in 8f-3d: bits / rank / h_grid are the NODE level's own grid index
 *       (pitch h_grid[6] == pitch) or three NULLs: binary search over keys.  Same bits either way.  v, m: the level's
 *       reconstructed DCs and means, int32 [n, channels]; child_v, child_m: those of the children, written here (child_m NULL
 *       exactly where child_w is NULL: the children are voxels, whose means nothing reads).  d_flag: device int32 zeroed by the
 *       caller; a clamp sets bit 0 (a valid stream never clamps).
 * pcc_raht_pred_mean / pcc_raht_pred_scale / pcc_raht_pred_predict  HOST: the kernels' own arithmetic for the CPU tests.  mean:
 *                         *h_out = m before its clamp (|dc| <= 2^30, 1 <= w < 2^26).  scale: *h_out = P before its clamp (|pred|
 *                         <= 2^24, 1 <= w < 2^26).  predict: *h_out = the prediction from h_means[8] (cell b = bx<<2 | by<<1 | bz,
 *                         |mean| <= 2^24) and the presence mask 1..255.
 * pcc_raht_pred_root      v_out[c] = quantise(v[c]) * step (clamped) and m_out[c] = its mean for the root of weight `weight`:
 *                         the encoder hands in the true root DC, the decoder the header's q * step (which comes back unchanged).
 * pcc_raht_pred_encode    coef rows of the level = quantise(h_true - Hp); child_v, child_m as the decoder will reconstruct them.
 * pcc_raht_pred_inverse   child_v, child_m from v, m and the rows' symbols.
 * ---------------------------------------------------------------------------------------- */
int pcc_raht_pred_mean(int64_t dc, uint32_t w, int64_t* h_out);
int pcc_raht_pred_scale(int64_t pred, uint32_t w, int64_t* h_out);
int pcc_raht_pred_predict(const int32_t* h_means /*[8]*/, int32_t mask, int32_t* h_out);
int pcc_raht_pred_root(const int32_t* v, int64_t weight, int32_t channels, const int32_t* h_steps, int32_t* v_out, int32_t* m_out,
                       int32_t* d_flag, void* stream);
int pcc_raht_pred_encode(const int64_t* keys, int64_t n, int32_t pitch, const uint64_t* bits, const int32_t* rank,
                         const int32_t* h_grid, const int64_t* child_keys, int64_t n_child, const uint64_t* child_bits,
                         const int32_t* child_rank, const int32_t* h_child, const int32_t* off, const int32_t* child_w /*nullable*/,
                         const int32_t* v, const int32_t* m, int32_t channels, const int32_t* h_steps, const int32_t* h_true,
                         int32_t* coef, int64_t row_base, int64_t rows_total, int32_t* child_v, int32_t* child_m /*nullable*/,
                         int32_t* d_flag, void* stream);
int pcc_raht_pred_inverse(const int64_t* keys, int64_t n, int32_t pitch, const uint64_t* bits, const int32_t* rank,
                          const int32_t* h_grid, const int64_t* child_keys, int64_t n_child, const uint64_t* child_bits,
                          const int32_t* child_rank, const int32_t* h_child, const int32_t* off, const int32_t* child_w /*nullable*/,
                          const int32_t* v, const int32_t* m, int32_t channels, const int32_t* h_steps, const int32_t* coef,
                          int64_t row_base, int64_t rows_total, int32_t* child_v, int32_t* child_m /*nullable*/, int32_t* d_flag,
                          void* stream);

/* ------------------------------------------------------------------------------------------
 * 8f-3d lossless attribute coder over the same level sets: the levels, stages, slot pairs, rows and
 *       groups of 8f-3c (pcc_raht_mask / pcc_raht_weights / pcc_raht_index / pcc_raht_hist and pcc_geom_child_offsets serve both)
 *       with a reversible arithmetic.  Values are plain int32 levels [rows, channels], 1 <= channels <= 8: 0..255, and with
 *       colour != 0 (channels == 3) YCoCg-R: Co = R - B, t = B + (Co >> 1), Cg = G - t, Y = t + (Cg >> 1), Co and Cg in
 *       -255..255.  Butterfly of present siblings (w1, x1), (w2, x2): H = x2 - x1, L = x1 + floor(w2 * H / (w1 + w2)); inverse
 *       x1 = L - floor(w2 * H / (w1 + w2)), x2 = H + x1.  Prediction of a child (dx, dy, dz): over the present cells node + d * b
 *       of the node's own level, d = 2 * (dx, dy, dz) - 1, b in {0, 1}^3, weights 27 / 9 / 3 / 1 by the non-zero components of b,
 *       floor((sum wt * value + (sum wt >> 1)) / sum wt); the children's predictions go through the same lifting and give Hp per
 *       butterfly; the coded symbol is H - Hp.  A level is given as in 8f-3c; bits / rank / h_grid are the NODE level's own grid
 *       index (pitch h_grid[6] == pitch) or three NULLs: binary search over keys.  Same bits either way.
 * pcc_lift_pair / pcc_lift_predict  HOST: the kernels' own arithmetic for the CPU tests.  pair: h_out[4] = L, H and the
 *                      inverse's x1, x2 (weights >= 1, below 2^27 in total; |x| <= 1023).  predict: *h_out = the prediction from
 *                      h_values[8] (cell b = bx<<2 | by<<1 | bz, |value| <= 1023) and the presence mask 1..255.
 * pcc_lift_prepare     uint8 attrs [n, channels] (row perm[i] of the caller's order, perm NULL: row i) -> values.
 * pcc_lift_forward     w[i], v[i, :] (the node's rounded mean) and H of the node's butterflies at its rows.
 * pcc_lift_residual    rows of the level -= Hp, from the level's own values v [n, channels] (all levels' v and the H rows exist
 *                      after the forward pass; the levels are independent here).
 * pcc_lift_inverse     child_v of every child from v and the rows' symbols: H = symbol + Hp (predict != 0) or symbol.  A symbol
 *                      is clamped to +-1023 and every reconstructed value into its channel's range; a clamp sets bit 0 of
 *                      *d_flag (device int32 zeroed by the caller).
 * pcc_lift_finish      values -> uint8 (inverse YCoCg-R for colour != 0); a level outside 0..255 is clamped and sets *d_flag.
 * ---------------------------------------------------------------------------------------- */
int pcc_lift_pair(uint32_t w1, uint32_t w2, int32_t x1, int32_t x2, int64_t* h_out /*[4]*/);
int pcc_lift_predict(const int32_t* h_values /*[8]*/, int32_t mask, int32_t* h_out);
int pcc_lift_prepare(const uint8_t* attrs, const int64_t* perm /*nullable*/, int64_t n, int32_t channels, int32_t colour,
                     int32_t* values, void* stream);
int pcc_lift_forward(const int64_t* keys, int64_t n, int32_t pitch, const int64_t* child_keys, int64_t n_child,
                     const uint64_t* child_bits, const int32_t* child_rank, const int32_t* h_child, const int32_t* off,
                     const int32_t* child_w /*nullable*/, const int32_t* child_v, int32_t channels, int32_t* w, int32_t* v,
                     int32_t* coef, int64_t row_base, int64_t rows_total, void* stream);
int pcc_lift_residual(const int64_t* keys, int64_t n, int32_t pitch, const uint64_t* bits, const int32_t* rank,
                      const int32_t* h_grid, const int64_t* child_keys, int64_t n_child, const uint64_t* child_bits,
                      const int32_t* child_rank, const int32_t* h_child, const int32_t* off, const int32_t* child_w /*nullable*/,
                      const int32_t* v, int32_t channels, int32_t* coef, int64_t row_base, int64_t rows_total, void* stream);
int pcc_lift_inverse(const int64_t* keys, int64_t n, int32_t pitch, const uint64_t* bits, const int32_t* rank,
                     const int32_t* h_grid, const int64_t* child_keys, int64_t n_child, const uint64_t* child_bits,
                     const int32_t* child_rank, const int32_t* h_child, const int32_t* off, const int32_t* child_w /*nullable*/,
                     const int32_t* v, int32_t channels, int32_t colour, int32_t predict, const int32_t* coef, int64_t row_base,
                     int64_t rows_total, int32_t* child_v, int32_t* d_flag, void* stream);
int pcc_lift_finish(const int32_t* values, int64_t n, int32_t channels, int32_t colour, uint8_t* out, int32_t* d_flag,
                    void* stream);

/* ------------------------------------------------------------------------------------------
 * 8f-3e inter frames of the lossless attribute coder (DESIGN.md section 7i "Inter frames", stream 0xB6): the LAST level (nodes
 *       at pitch 2, children = the voxels) may predict a child from its match in a reference cloud instead of from the level.
 *       Blocks: the nodes of level max(0, depth - 4) of the current cloud (block_keys origin-relative, block_log2 = depth - that
 *       level, 1..4; block_bits / block_rank / h_block their grid index at pitch 2^block_log2, or NULLs: binary search), vec the
 *       vector index per block as pcc_geom_inter_motion gives it.  The reference: canonical pitch-1 keys in ABSOLUTE
 *       coordinates (n_ref == 0: empty) with its grid index or NULLs, and ref_values int32 [n_ref, channels] from
 *       pcc_lift_prepare.  d_flag: device int32 zeroed by the caller; bit 0 is set by a block row, a vector index, a mode or a
 *       match outside its range (counted as vector 0 / mode 0 / unmatched) and by the clamps of pcc_lift_inverse.
 * pcc_lift_inter_match     match[i] of voxel i (voxel_keys origin-relative, origin ox, oy, oz): with its block's vector d the
 *                          reference row at p - d, else at the first occupied of the 26 cells around it ordered by
 *                          (|o|^2, 9 (ox + 1) + 3 (oy + 1) + (oz + 1)), else -1.
 * pcc_lift_inter_match_wide  the same with disp[b], a packed displacement of 8f-3b* with 1 <= search <= 7, in place of an index
 *                          (streams 0xB7 and 0xB8); a displacement outside +-search counts as zero and sets bit 0 of *d_flag.
 * pcc_lift_inter_residual  after pcc_lift_forward: rows of the level -= Hp of the spatial prediction (what pcc_lift_residual
 *                          does) and coef_t [rows_total - row_base, channels] = H - Hp of the temporal prediction (a matched
 *                          child: ref_values of its match; an unmatched one: the spatial prediction); sums [n_blocks, 2] int32
 *                          (cleared here) += sum |symbol| of the spatial / temporal rows of the block's nodes.  A level without
 *                          rows (rows_total == row_base: every voxel alone in its cell) is legal here and in
 *                          pcc_lift_inter_select: nothing is written but the zero sums, coef_t may be NULL.
 * pcc_lift_inter_select    sums != NULL: mode[b] = sums[b, 1] < sums[b, 0] first.  Then idx of the level's rows: group
 *                          (level + mode) * 6 + 3 * (channel > 0) + stage, or side[group] & 63; coef / coef_t given (together):
 *                          the rows of mode-1 blocks are copied from coef_t into coef.  mask / off as for pcc_raht_index.
 * pcc_lift_inter_inverse   pcc_lift_inverse with predict != 0 for this level, the children of a mode-1 block's nodes predicted as
 *                          in pcc_lift_inter_residual.
 * ---------------------------------------------------------------------------------------- */
int pcc_lift_inter_match(const int64_t* voxel_keys, int64_t n, const int64_t* block_keys, int64_t n_blocks,
                         const uint64_t* block_bits, const int32_t* block_rank, const int32_t* h_block, int32_t block_log2,
                         const int32_t* vec, int32_t search, const int64_t* ref_keys, int64_t n_ref, const uint64_t* ref_bits,
                         const int32_t* ref_rank, const int32_t* h_ref, int32_t ox, int32_t oy, int32_t oz, int32_t* match,
                         int32_t* d_flag, void* stream);
int pcc_lift_inter_match_wide(const int64_t* voxel_keys, int64_t n, const int64_t* block_keys, int64_t n_blocks,
                              const uint64_t* block_bits, const int32_t* block_rank, const int32_t* h_block, int32_t block_log2,
                              const int32_t* disp, int32_t search, const int64_t* ref_keys, int64_t n_ref, const uint64_t* ref_bits,
                              const int32_t* ref_rank, const int32_t* h_ref, int32_t ox, int32_t oy, int32_t oz, int32_t* match,
                              int32_t* d_flag, void* stream);
int pcc_lift_inter_residual(const int64_t* keys, int64_t n, int32_t pitch, const uint64_t* bits, const int32_t* rank,
                            const int32_t* h_grid, const int64_t* child_keys, int64_t n_child, const uint64_t* child_bits,
                            const int32_t* child_rank, const int32_t* h_child, const int64_t* block_keys, int64_t n_blocks,
                            const uint64_t* block_bits, const int32_t* block_rank, const int32_t* h_block, int32_t block_log2,
                            const int32_t* off, const int32_t* v, int32_t channels, const int32_t* match,
                            const int32_t* ref_values /*nullable when n_ref == 0*/, int64_t n_ref, int32_t* coef, int32_t* coef_t,
                            int64_t row_base, int64_t rows_total, int32_t* sums, int32_t* d_flag, void* stream);
int pcc_lift_inter_select(const int64_t* keys, const int32_t* mask, const int32_t* off, int64_t n, int32_t level,
                          int32_t channels, const int64_t* block_keys, int64_t n_blocks, const uint64_t* block_bits,
                          const int32_t* block_rank, const int32_t* h_block, int32_t block_log2, const int32_t* sums /*nullable*/,
                          int32_t* mode, const int32_t* side /*nullable*/, int32_t* idx, int32_t* coef /*nullable*/,
                          const int32_t* coef_t /*nullable*/, int64_t row_base, int64_t rows_total, int32_t* d_flag, void* stream);
int pcc_lift_inter_inverse(const int64_t* keys, int64_t n, int32_t pitch, const uint64_t* bits, const int32_t* rank,
                           const int32_t* h_grid, const int64_t* child_keys, int64_t n_child, const uint64_t* child_bits,
                           const int32_t* child_rank, const int32_t* h_child, const int64_t* block_keys, int64_t n_blocks,
                           const uint64_t* block_bits, const int32_t* block_rank, const int32_t* h_block, int32_t block_log2,
                           const int32_t* mode, const int32_t* off, const int32_t* v, int32_t channels, int32_t colour,
                           const int32_t* match, const int32_t* ref_values /*nullable when n_ref == 0*/, int64_t n_ref,
                           const int32_t* coef, int64_t row_base, int64_t rows_total, int32_t* child_v, int32_t* d_flag,
                           void* stream);

/* ------------------------------------------------------------------------------------------
 * 8f-4  nearest-neighbour association of the distortion report (replaces the two Open3D KD-trees and the per-point
 *       Python loop of PointCloudMetric.__init__, metrics/metric.py:36-43).  Exact, integer coordinates.
 *       a_xyz [n_a,3] int32 queries (any order; canonical order is fastest); b_xyz [n_b,3] int32 SORTED BY x ascending
 *       (canonical key order is).  d2[i] = min_j |a_i - b_j|^2, nn[i] = the smallest such j.
 * ---------------------------------------------------------------------------------------- */
int pcc_nn_sorted_x(const int32_t* a_xyz, int64_t n_a, const int32_t* b_xyz, int64_t n_b, int64_t* d2, int32_t* nn,
                    void* stream);

/* ------------------------------------------------------------------------------------------
 * 8f-5  radius normal estimation of the point-to-plane (D2) report (reference evaluate.py:153,
 *       rec_pc.estimate_normals(KDTreeSearchParamRadius(radius=5.0)); the normals go to pc_error at utils.py:223).
 *       keys: a canonical, de-duplicated set at pitch 1 (n < 2^31); grid_bits / h_grid: its pcc_grid_build bitmap and host
 *       parameters (pitch h_grid[6] must be 1; the rank array is not needed), or NULL: binary search over the keys, same bits.
 *       Neighbourhood of a point: every member at integer offset d with |d|^2 <= lim, the point itself included; the caller
 *       passes lim = ceil(r^2) - 1 (the strict dist^2 < r^2 of a radius search); 0 <= lim <= 63 (r <= 8), else an error.
 *       normals [n,3] fp32: the eigenvector of the smallest eigenvalue of M = n S2 - S1 S1^T (exact int64 moments of the
 *       neighbourhood, n^2 times its covariance), solved in fp64, normalised, flipped so that its largest-magnitude component
 *       is positive (the first such axis on a tie); fewer than 3 neighbours: (0, 0, 1); a degenerate (collinear)
 *       neighbourhood: some unit vector of the smallest eigenspace.  counts [n] int32 (nullable): neighbourhood sizes.
 *       One thread per point in canonical order, no atomics, no order-dependent float sums: bitwise reproducible.
 * ---------------------------------------------------------------------------------------- */
int pcc_normals_grid(const int64_t* keys, int64_t n, const uint64_t* grid_bits /*nullable*/, const int32_t* h_grid, int32_t lim,
                     float* normals /*[n,3]*/, int32_t* counts /*nullable*/, void* stream);

/* ------------------------------------------------------------------------------------------
 * 8f-6  the two radius kernels of the PCQM quality metric (Meynet, Nehme, Digne, Lavoue, QoMEX 2020; the reference
 *       reads it from an external binary, utils.py:270-322; restated on the voxel lattice, see metrics.py `pcqm`).
 *       keys / grid_bits / grid_rank / h_grid: a canonical set at pitch 1 and its pcc_grid_build index, or NULL bits:
 *       binary search over the keys, same bits out.  Neighbourhoods as in pcc_normals_grid: |d|^2 <= lim, the point itself
 *       included; 0 <= lim <= 288 (radius <= 17), else an error.  No atomics, every sum in an order fixed by the set.
 *       pcc_curvature_grid: out[n] fp64 = the absolute mean curvature, at the point's foot, of the quadric
 *       z = a x^2 + b xy + c y^2 + d x + e y + f fitted (unweighted least squares, 6 x 6 normal equations in fp64 summed in
 *       the order dx, dy, dz ascending, Cholesky) to the neighbourhood in the frame (u, v, n): n the normal of
 *       pcc_normals_grid kept in fp64, u = normalise(e x n) with e the axis of the smallest |n| (first on a tie), v = n x u.
 *       Fewer than 6 members, or a pivot <= 1e-12 x the largest diagonal entry: 0.  (Offsets only: the rank array is not read.)
 *       pcc_pcqm_features: table [n,10] fp64 holds per point (curvature, lightness, a, b, chroma), each as the pair (own
 *       value, value of the paired point).  out [n,8] fp64 = the features f1 .. f8 from the Gaussian-weighted
 *       (w = exp(-|d|^2 inv_two_sigma2)) means, deviations and covariance over the neighbourhood, every attribute shifted
 *       by the centre's own value before it is summed.  One wave per point, rows gathered through the rank array.
 * ---------------------------------------------------------------------------------------- */
int pcc_curvature_grid(const int64_t* keys, int64_t n, const uint64_t* grid_bits /*nullable*/, const int32_t* grid_rank,
                       const int32_t* h_grid, int32_t lim, double* out /*[n]*/, void* stream);
int pcc_pcqm_features(const int64_t* keys, int64_t n, const uint64_t* grid_bits /*nullable*/, const int32_t* grid_rank,
                      const int32_t* h_grid, int32_t lim, double inv_two_sigma2, const double* table /*[n,10]*/,
                      double* out /*[n,8]*/, void* stream);

/* ------------------------------------------------------------------------------------------
 * 9    training batches: cube slicing and the per-step augmented batch (reference data/dataloader.py:168-208
 *      StaticDataset.slice_into_cubes; data/transform.py:32-54 ColorJitter, :57-123 RandomRotate; train.py:199-208
 *      sparse_collate + sparse_quantize).
 * ---------------------------------------------------------------------------------------- */
/* dataloader.py:186,196-197: per point of [n,3] fp32, keys[i] = the cube indices floor(p / cube_size) (fp32 division,
 * round to nearest), each biased by 2^15 into a 16-bit field, x most significant -- integer order is the lexicographic
 * (ix, iy, iz) order of torch.unique(dim=0) -- and local[i] = p - index * cube_size.  *d_bad (device int32) != 0 when an
 * index does not fit its field or a point is not finite.  Group with the stable sort + run starts that exist for keys. */
int pcc_cube_keys(const float* points, int64_t n, int32_t cube_size, int64_t* keys, float* local /*[n,3]*/, int32_t* d_bad,
                  void* stream);
/* dataloader.py:191-194: out[i] = in[perm[i]] for both [n,3] arrays at once (perm: the sort's permutation) */
int pcc_cube_regroup(const float* local, const float* colors, const int32_t* perm, int64_t n, float* out_points,
                     float* out_colors, void* stream);

/* Batch-slot descriptor: PCC_AUG_SLOT_WORDS 4-byte words per slot, host-built, uploaded once per step.
 *   [0] in_begin   first row of the slot's cube in the table        [1] rows
 *   [2] out_begin  first row of the slot in the batch arrays        [3] nsteps (0..4 colour steps)
 *   [4..7]   steps, applied in this order (PCC_AUG_*)               [8..11]  fp32 factors by step kind: b, c, s, hue shift
 *   [12..20] fp32 rotation matrix R, row-major                      [21]     fp32 centre c (block_size / 2)
 *   [22] first_block, [23] nblocks: the slot's run in the block table
 *   [24..26] lo, [27..29] hi: int32 box that holds every output coordinate of the slot (the caller's bound; the caller sizes
 *            its de-duplication lattice from it without reading coordinates back); the rest is padding.
 * Block table: int32 pairs (slot, first row in the slot), PCC_AUG_BLOCK_ROWS rows per workgroup, slots ascending.
 * Both tables are passed twice, as the host original (validated before any launch: ranges inside the table, output ranges
 * tiling [0, out_rows) in slot order, block table equal to the enumeration) and as its device copy (read by the kernels). */
#define PCC_AUG_SLOT_WORDS 32
#define PCC_AUG_BLOCK_ROWS 1024
#define PCC_AUG_MAX_SLOTS 4096
#define PCC_AUG_BRIGHTNESS 0
#define PCC_AUG_CONTRAST 1
#define PCC_AUG_SATURATION 2
#define PCC_AUG_HUE 3
/* transform.py:36-40, the contrast step of ColorJitter: means[slot] = mean over the slot's rows of the grey value
 * 0.2989 r + 0.587 g + 0.114 b of the colour as the contrast step finds it (after the steps before it in the slot's order);
 * 0 for a slot without one.  fp64 sums in a fixed order (partials [nblocks] fp64, one per workgroup; no atomics): the same
 * inputs give the same bits.  Launches nothing when no slot has a contrast step. */
int pcc_aug_gray_sums(const float* colors, int64_t table_rows, const int32_t* h_slots, const int32_t* d_slots, int32_t nslots,
                      const int32_t* h_blocks, const int32_t* d_blocks, int32_t nblocks, double* partials, float* means,
                      void* stream);
/* transform.py:42-54,74-93 + train.py:199-201 in one launch: for every row of every slot the colour steps in the slot's
 * order, out = (p - c) R^T + c evaluated as ((dx R[j][0] + dy R[j][1]) + dz R[j][2]) + c with every product and sum rounded
 * to fp32 separately (no FMA), floor; out_coords [out_rows,4] int32 = (slot, x, y, z), out_feats [out_rows,3] fp32.
 * means: from the gray-sums call (nullable when no slot has a colour step).  A coordinate outside its slot's box is moved
 * onto the box and *d_outside (device int32, zeroed here) is set: with a correct bound that never happens. */
int pcc_aug_batch(const float* points, const float* colors, int64_t table_rows, const int32_t* h_slots, const int32_t* d_slots,
                  int32_t nslots, const int32_t* h_blocks, const int32_t* d_blocks, int32_t nblocks, const float* means,
                  int32_t* out_coords, float* out_feats, int64_t out_rows, int32_t* d_outside, void* stream);

/* ------------------------------------------------------------------------------------------
 * 10   PLY vertex bodies (reference evaluate.py:30-37,105 and data/utils/RawLoader.py:47 read ASCII PLY frames;
 *      utils.py:503 save_ply and model/model.py:409 write them).  The header is parsed and written by the caller
 *      (ply.py); these entry points see the body bytes only, uploaded on their own so that their base is aligned.
 * ---------------------------------------------------------------------------------------- */
#define PCC_PLY_MAX_PROPS 32      /* vertex properties of a file, and selected properties of a call */
#define PCC_PLY_TILE_BYTES 4096   /* body bytes per workgroup of the token passes */
#define PCC_PLY_STAGE_BYTES 16384 /* most body bytes a workgroup of the binary reader stages in LDS */
#define PCC_PLY_TOKEN_MAX 40      /* longest token the device converts */
#define PCC_PLY_I8 0
#define PCC_PLY_U8 1
#define PCC_PLY_I16 2
#define PCC_PLY_U16 3
#define PCC_PLY_I32 4
#define PCC_PLY_U32 5
#define PCC_PLY_F32 6
#define PCC_PLY_F64 7
/* Property table of the two readers: h_table [nsel][5] int32 on the HOST = (where, type PCC_PLY_*, destination array,
 * destination column, colour scale 0/1) per selected property; `where` is the byte offset in a record (binary) or the
 * property's index in the vertex element (ASCII).  Destination arrays: 0 = cloud [n, cloud_cols] row-major (3 or 6
 * columns), 1 = normals [n,3] row-major (nullable), 2 = extra [extra_cols][n], one contiguous run per column.  Integer types
 * and double convert to fp32 round-to-nearest; with the colour scale (uchar only) the value is the fp32 quotient k / 255.
 * The table is validated before any launch (fields inside the record, columns inside their arrays, no destination twice):
 * PCC_EINVAL otherwise; it reaches the kernels by value. */
/* records per workgroup of the binary reader for this record size (0: unsupported size) */
int32_t pcc_ply_block_records(int32_t stride);
/* evaluate.py:30-37 for binary files: n records of `stride` bytes from body (16-byte aligned; n * stride <= body_bytes or
 * PCC_EINVAL), fields at any byte offset, either endianness.  n = 0 launches nothing. */
int pcc_ply_unpack_binary(const uint8_t* body, int64_t body_bytes, int64_t n, int32_t stride, const int32_t* h_table, int32_t nsel,
                          int32_t big_endian, float* cloud, int32_t cloud_cols, float* normals, float* extra, int32_t extra_cols,
                          void* stream);
/* bytes per tile of pcc_ply_count_tokens (PCC_PLY_TILE_BYTES) */
int32_t pcc_ply_tile_bytes(void);
/* evaluate.py:30-37 / RawLoader.py:47, pass 1: a token starts at a byte that is not whitespace (blank, \t, \r, \n) and whose
 * predecessor is whitespace or the start of the body; tile_counts [ceil(body_bytes / tile)] = token starts per tile.  The
 * caller scans them (exclusive) into tile_base. */
int pcc_ply_count_tokens(const uint8_t* body, int64_t body_bytes, int32_t* tile_counts, void* stream);
/* pass 2: token t is property t % nprops of vertex t / nprops; tokens from n * nprops on (face data) are ignored, so are
 * unselected properties.  starts [n * nprops] int32 is scratch (the byte offset of every token).  Integer-typed properties
 * are read exactly ([+-]digits; a decimal point or an exponent there, or a value outside the type, is an error); float-typed
 * ones take sign, digits, optional point, optional exponent, and are converted when that is exact arithmetic: at most 15
 * significant digits and a power of ten within +-22 make m * 10^e (or m / 10^e) one correctly rounded fp64 operation, then
 * rounded to fp32 -- the bits of float32(float(token)).  Anything else is not guessed: a longer significand, a larger
 * exponent, a token over PCC_PLY_TOKEN_MAX bytes, nan / inf go to fallback [fallback_cap][2] int64 = (token ordinal, byte
 * offset) for the host to convert.  status [4] int64 (device): [0] tokens in the body, [1] fallback tokens met (more than
 * fallback_cap: the list overflowed), [2] -1 or (ordinal << 32 | byte offset) of the first token that is no number.
 * A body with fewer than n * nprops tokens converts what it has; the caller sees status[0].  Every read is bounded by
 * body_bytes. */
int pcc_ply_parse_ascii(const uint8_t* body, int64_t body_bytes, int64_t n, int32_t nprops, const int32_t* h_table, int32_t nsel,
                        const int32_t* tile_base, int32_t* starts, float* cloud, int32_t cloud_cols, float* normals, float* extra,
                        int32_t extra_cols, int64_t* status, int64_t* fallback, int32_t fallback_cap, void* stream);
/* utils.py:503 save_ply as a binary little-endian body: records x y z [nx ny nz] [r g b] from cloud [n, 3|6] (and normals
 * [n,3], nullable); coordinates as fp32 or (coords_int) int32, colours as uchar clamp(rint(255 f), 0, 255), the rule of
 * pcc_decode_finish.  *d_flag (device int32, zeroed here) is set when coords_int meets a coordinate that is not an integer
 * of int32 range.  out: 16-byte aligned, out_bytes >= n * record size. */
int pcc_ply_pack_binary(const float* cloud, int32_t cloud_cols, const float* normals, int64_t n, int32_t coords_int, uint8_t* out,
                        int64_t out_bytes, int32_t* d_flag, void* stream);
/* utils.py:503 / model/model.py:409 as text, pass 1: lengths[i] = bytes of line i, "x y z[ r g b]\n" with integer
 * coordinates and 8-bit colour levels; *d_flag (zeroed here) is set when a coordinate is not an integer of int32 range. */
int pcc_ply_row_lengths(const float* cloud, int32_t cloud_cols, int64_t n, int32_t* lengths, int32_t* d_flag, void* stream);
/* pass 2: the characters.  row_offsets [n + 1] int64 = the caller's exclusive scan of the lengths (last entry: the body's
 * size); a row whose offsets do not hold its text, or lie outside out_bytes, is not written. */
int pcc_ply_format_ascii(const float* cloud, int32_t cloud_cols, int64_t n, const int64_t* row_offsets, uint8_t* out, int64_t out_bytes,
                         void* stream);

/* ------------------------------------------------------------------------------------------
 * 11   voxel-grid down-sampling with averaged attributes (reference data/utils/RawLoader.py:48-57: Open3D's
 *      voxel_down_sample(factor), then the division by the factor and the rounding).
 * ---------------------------------------------------------------------------------------- */
#define PCC_VOXEL_MAX_ATTRS 32    /* attribute columns averaged beside the point */
#define PCC_VOXEL_WAVE_RUN 32     /* a run of this many rows or more is summed by a whole wave, a shorter one by four lanes */
#define PCC_VOXEL_SPLIT_RUN 2048  /* a run of this many rows or more is summed by several workgroups into fp64 partials */
#define PCC_VOXEL_TILE_ROWS 1024  /* sorted rows per workgroup of that split pass */
/* Per point of [n,3] fp32 and per axis idx = floor(((double)p - origin) / voxel_size): one fp64 subtraction and one true
 * fp64 division (no reciprocal), so a float64 restatement gives the same integer.  keys[i] = the three indices, each biased
 * by 2^15 into a 16-bit field, x most significant (the layout of pcc_cube_keys: integer order is (ix, iy, iz) order).
 * *d_bad (device int32, zeroed here) != 0 when a point is not finite or an index lies outside [-2^15, 2^15).  PCC_EINVAL,
 * before anything is launched, unless 0 <= n < 2^31 and voxel_size and the origin are finite, voxel_size > 0. */
int pcc_voxel_keys(const float* points, int64_t n, double origin_x, double origin_y, double origin_z, double voxel_size,
                   int64_t* keys, int32_t* d_bad, void* stream);
/* Means per run of equal keys.  perm: the permutation of pcc_sort_keys over those keys; uniq_keys / first / *d_count: what
 * pcc_unique_sorted made of the sorted keys (the count stays on the device: the grids are sized for n runs).  For every run
 * r < *d_count: counts[r], index[r] = the three unbiased fields of uniq_keys[r], mean_points[r] and mean_attrs[r] = the mean
 * over the run's rows of points [n,3] and of attrs [n,c] fp32 (0 <= c <= PCC_VOXEL_MAX_ATTRS; c = 0: both attribute
 * pointers may be NULL).  Outputs hold n rows; rows from *d_count on are not written.  Every sum is fp64, the mean one fp64
 * division rounded once to fp32; no floating-point atomics, and the order of the additions depends on n and the run
 * layout only: equal inputs give equal bits.  Runs below PCC_VOXEL_WAVE_RUN rows share a wave sixteen at a time, longer ones
 * take a whole wave each, runs of PCC_VOXEL_SPLIT_RUN rows or more are summed tile by tile into ws (fp64 partials) by a
 * first launch and added in tile order.  Every index read from perm / first is checked against n before it is used. */
size_t pcc_voxel_means_ws_bytes(int64_t n, int32_t c);
int pcc_voxel_means(const float* points, const float* attrs /*nullable*/, int32_t c, int64_t n, const int32_t* perm,
                    const int64_t* uniq_keys, const int32_t* first, const int64_t* d_count, int32_t* index /*[n,3]*/,
                    int32_t* counts /*[n]*/, float* mean_points /*[n,3]*/, float* mean_attrs /*[n,c], nullable*/, void* ws,
                    size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * 12   multi-tensor optimiser step: clip_grad_norm_ + Adam / SGD with momentum over all tensors of an optimiser
 *      (reference train.py:224-227: torch.nn.utils.clip_grad_norm_, optim.Adam / optim.SGD(momentum=0.9)).
 * ---------------------------------------------------------------------------------------- */
#define PCC_OPTIM_CHUNK 16384     /* elements of one tensor per workgroup */
#define PCC_OPTIM_SEG_WORDS 6     /* int64 words per row of the segment table */
#define PCC_OPTIM_ADAM 0
#define PCC_OPTIM_SGD 1
/* Segment table (device) [n_segs][PCC_OPTIM_SEG_WORDS] int64, one row per tensor: param*, grad*, state1*, state2*, n, t.
 * All arrays fp32 with n elements.  grad* = 0: the tensor has no gradient this step; nothing of it is read or written.
 * state1 = exp_avg (Adam) / momentum_buffer (SGD); state2 = exp_avg_sq (Adam; unused and may be 0 for SGD).  t = the
 * tensor's step count with this step counted (1 = its first step): a tensor that was skipped keeps its own count, as in
 * torch, so t travels with the gradient pointers and not as one kernel argument.
 * Chunk table (device) [n_chunks][2] int32 = (segment, chunk index inside it): chunk i of a tensor holds its elements
 * [i * PCC_OPTIM_CHUNK, min(n, (i + 1) * PCC_OPTIM_CHUNK)).  Sizes never change, so it is built once, on the host:
 * pcc_optim_build_chunks returns the number of chunks of tensors of the given sizes (a tensor of 0 elements has none) and,
 * when h_chunks is not NULL, writes the first `cap` entries; -1 for a negative size or count, or 2^31 chunks or more.
 * An entry that names no segment or lies outside its tensor is skipped by the kernels, never dereferenced. */
int32_t pcc_optim_chunk_elems(void);
int64_t pcc_optim_build_chunks(const int64_t* h_sizes, int32_t n_segs, int32_t* h_chunks /*nullable*/, int64_t cap);
size_t pcc_optim_ws_bytes(int64_t n_chunks); /* the fp64 partials, one per chunk */
/* ws[chunk] = sum of g * g over the chunk in fp64 (0 for a tensor without gradient), in an order fixed by the chunk's
 * length: no atomics, equal inputs give equal bits.  One launch of n_chunks workgroups.  PCC_EINVAL / PCC_EWS before any
 * launch for n_segs < 0, n_chunks outside 0..2^31-1, a NULL table, a workspace below pcc_optim_ws_bytes(n_chunks). */
int pcc_optim_sqnorm(const int64_t* d_segs, int32_t n_segs, const int32_t* d_chunks, int64_t n_chunks, void* ws, size_t ws_bytes,
                     void* stream);
/* One launch: every workgroup adds ws[0..n_chunks) in the same fixed order, norm = (float)sqrt(sum),
 * coef = min(1, max_norm / (norm + 1e-6)) in fp32 (clip_grad_norm_'s rule; a NaN norm gives a NaN coefficient, an
 * infinite one 0, as torch's arithmetic does), and updates its chunk with g * coef:
 *   PCC_OPTIM_ADAM  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
 *                   (torch.optim.Adam without amsgrad and weight decay; the bias corrections in fp64)
 *   PCC_OPTIM_SGD   buf = g when t = 1, else beta1 buf + g;  p -= lr buf      (beta1 = the momentum; beta2, eps unused)
 * The gradients themselves are NOT overwritten with g * coef (clip_grad_norm_ does overwrite them).  max_norm <= 0: no
 * clipping, ws is not read (pcc_optim_sqnorm need not have run) and *d_norm is not written; otherwise workgroup 0
 * stores the norm to *d_norm (device fp32, nullable).  Refusals as for pcc_optim_sqnorm, and an unknown mode. */
int pcc_optim_step(const int64_t* d_segs, int32_t n_segs, const int32_t* d_chunks, int64_t n_chunks, const void* ws, size_t ws_bytes,
                   int32_t mode, double lr, double beta1, double beta2, double eps, double max_norm, float* d_norm /*nullable*/,
                   void* stream);

/* ------------------------------------------------------------------------------------------
 * measurement support: per-launch HIP-event timing of the conv kernel (bench.py roofline)
 * ---------------------------------------------------------------------------------------- */
int pcc_prof_enable(int32_t on);
/* sums over launches since the last reset; also resets. flops = 2*P*Cin*Cout needs the pair
 * counts, which the caller accumulates itself (d_pairs). Synchronises the recorded events. */
int pcc_prof_collect(double* h_conv_ms, int64_t* h_conv_launches);
/* The same timings split by the kernel form each launch actually took (so that a report never has to mirror the dispatch
 * rules): arrays of PCC_FORM_COUNT entries.  flops / bytes: algorithmic work of the dense products (rows x columns x depth,
 * 4 bytes per operand / result element), 0 for the gathered forms whose pair counts live on the device.  Also resets. */
#define PCC_FORM_OTHER 0      /* anything else that is event-timed */
#define PCC_FORM_GEMM_H2 1    /* k_gemm_h2: dense products, scaled fp16 pairs, 3 MFMA terms */
#define PCC_FORM_GEMM_BF2 2   /* k_gemm_bf2: dense products, bf16 split, 6 terms */
#define PCC_FORM_PAIR_H2 3    /* k_pair_h2: gathered pair GEMM, 3 terms */
#define PCC_FORM_PAIR_BF 4    /* gathered pair GEMM, 6 terms */
#define PCC_FORM_CONV_BF 5    /* k_conv_mfma_bf: gathered output-stationary convolution, 6 terms */
#define PCC_FORM_CONV_F32 6   /* k_conv_mfma: fp32-input MFMA */
#define PCC_FORM_WAVE16 7     /* k_conv_wave16 / wave16z: narrow outputs, fp32-input 16x16x4 MFMA */
#define PCC_FORM_GATHER_CSR 8 /* k_convt_gather_csr of a composite level (pcc_convt_fwd_csr_grid): not an MFMA launch; timed because
                                 dense products + gather-sum are ONE unit of SURVEY 8d's accounting */
#define PCC_FORM_COUNT 9
int pcc_prof_collect_forms(double* h_ms, int64_t* h_launches, double* h_flops, double* h_bytes);
/* forms of the timed launches recorded so far, in launch order (up to cap entries); returns their number; no reset */
int64_t pcc_prof_sequence(int32_t* h_forms, int64_t cap);
/* row tile, column tile and reduction split (BM, BN, ksplit as launched; 0, 0, 1 for a form without such a choice) of the same
 * launches: h_tiles [cap][3], same order and count as pcc_prof_sequence; no reset */
int64_t pcc_prof_sequence_tiles(int32_t* h_tiles, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* PCC_HIP_H */
