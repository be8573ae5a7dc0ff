// Training batches on the device: cube slicing of a frame, and the per-step assembly of a batch of augmented cubes
// (reference data/dataloader.py:168-208, data/transform.py:32-123, train.py:199-208).  HBM-bound element-wise work:
// consecutive lanes take consecutive rows, everything that is uniform over a workgroup (its slot's descriptor) is read
// through a uniform address, i.e. with scalar loads; no atomics, no order-dependent float sums.
#include "pcc_common.h"

static constexpr int AUG_T = 256;                    // threads per workgroup
static constexpr int AUG_R = PCC_AUG_BLOCK_ROWS / AUG_T;   // rows per thread, AUG_T apart
static_assert(PCC_AUG_BLOCK_ROWS % AUG_T == 0, "whole rounds");

// ------------------------------------------------------------------------------------------
// slicing
// ------------------------------------------------------------------------------------------
// cube index = floor(p / cube_size) per axis (fp32 division, correctly rounded: hipcc's default for `/`), cube-local
// point = p - index * cube_size (the shift is an exact integer, one fp32 subtraction as in dataloader.py:196-197)
__global__ void __launch_bounds__(256) k_cube_keys(const float* __restrict__ pts, long long n, float cube, long long* __restrict__ keys,
                                                   float* __restrict__ local, int* __restrict__ bad) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  long long k = 0;
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float p = pts[i * 3 + a];
    const float q = floorf(p / cube);
    ok = ok && q >= -(float)PCC_BIAS && q < (float)PCC_BIAS;      // (NaN fails both)
    const int c = ok ? (int)q : 0;
    local[i * 3 + a] = p - (float)(c * (int)cube);               // |c| <= 2^15, cube <= 2^15: fits
    k = (k << 16) | (long long)(c + (int)PCC_BIAS);
  }
  keys[i] = k;
  if (!ok) *bad = 1;       // benign race: every writer stores 1
}

extern "C" int pcc_cube_keys(const float* points, int64_t n, int32_t cube_size, int64_t* keys, float* local, int32_t* d_bad,
                             void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PCC_REQUIRE(d_bad, "pcc_cube_keys: d_bad is NULL");
  PCC_REQUIRE(cube_size >= 1 && cube_size <= (1 << 15), "pcc_cube_keys: cube_size %d outside 1..32768", cube_size);
  PCC_CHECK_HIP(hipMemsetAsync(d_bad, 0, sizeof(int32_t), s));
  if (n <= 0) return PCC_OK;
  PCC_REQUIRE(points && keys && local && n < (1ll << 31), "pcc_cube_keys: bad arguments");
  k_cube_keys<<<(unsigned)pcc_cdiv(n, 256), 256, 0, s>>>(points, n, (float)cube_size, (long long*)keys, local, d_bad);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

// both [n,3] arrays into the order of the stable sort by cube key: one pass, 3 floats per thread each
__global__ void __launch_bounds__(256) k_cube_regroup(const float* __restrict__ local, const float* __restrict__ colors,
                                                      const int* __restrict__ perm, long long n, float* __restrict__ out_p,
                                                      float* __restrict__ out_c) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long j = perm[i];
  if (j < 0 || j >= n) return;                    // a permutation never does this; a foreign array cannot read outside
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    out_p[i * 3 + a] = local[j * 3 + a];
    out_c[i * 3 + a] = colors[j * 3 + a];
  }
}

extern "C" int pcc_cube_regroup(const float* local, const float* colors, const int32_t* perm, int64_t n, float* out_points,
                                float* out_colors, void* stream) {
  if (n <= 0) return PCC_OK;
  PCC_REQUIRE(local && colors && perm && out_points && out_colors && n < (1ll << 31), "pcc_cube_regroup: bad arguments");
  PCC_REQUIRE(out_points != local && out_colors != colors, "pcc_cube_regroup: in place");
  k_cube_regroup<<<(unsigned)pcc_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(local, colors, perm, n, out_points, out_colors);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

// ------------------------------------------------------------------------------------------
// per-step batch assembly
// ------------------------------------------------------------------------------------------
// One descriptor per batch slot, PCC_AUG_SLOT_WORDS 4-byte words (include/pcc_hip.h lists them).
struct AugSlot {
  int in_begin, rows, out_begin, nsteps;
  int step[4];              // PCC_AUG_BRIGHTNESS .. PCC_AUG_HUE, applied in this order
  float factor[4];          // indexed by step kind
  float rot[9];             // row-major R
  float centre;
  int first_block, nblocks;
  int lo[3], hi[3];         // host-computed box that holds every output coordinate of the slot
  int pad[PCC_AUG_SLOT_WORDS - 30];
};
static_assert(sizeof(AugSlot) == PCC_AUG_SLOT_WORDS * 4, "descriptor layout");

// The tables come from the host, and the kernels index by them: everything is checked here, before any launch.  The block
// table has to be exactly the enumeration (slot ascending, first row ascending in steps of PCC_AUG_BLOCK_ROWS) and the slots'
// output ranges have to tile [0, out_rows) in slot order, so they are disjoint and inside the batch arrays.
static int aug_validate(const char* who, const int32_t* h_slots, int32_t nslots, const int32_t* h_blocks, int32_t nblocks,
                        int64_t table_rows, int64_t out_rows, bool* any_contrast) {
  PCC_REQUIRE(h_slots && h_blocks && nslots >= 1 && nslots <= PCC_AUG_MAX_SLOTS && nblocks >= 1 && table_rows >= 1 &&
              table_rows < (1ll << 31), "%s: bad arguments", who);
  const AugSlot* sl = (const AugSlot*)h_slots;
  int64_t out = 0, blk = 0;
  bool contrast = false;
  for (int s = 0; s < nslots; ++s) {
    const AugSlot& d = sl[s];
    PCC_REQUIRE(d.rows >= 1 && d.in_begin >= 0 && (int64_t)d.in_begin + d.rows <= table_rows,
                "%s: slot %d reads rows [%d, %lld) of a table of %lld", who, s, d.in_begin, (long long)d.in_begin + d.rows,
                (long long)table_rows);
    PCC_REQUIRE(d.out_begin == out, "%s: slot %d writes from row %d, expected %lld", who, s, d.out_begin, (long long)out);
    PCC_REQUIRE(d.nsteps >= 0 && d.nsteps <= 4, "%s: slot %d has %d colour steps", who, s, d.nsteps);
    unsigned seen = 0;
    for (int k = 0; k < d.nsteps; ++k) {
      PCC_REQUIRE(d.step[k] >= 0 && d.step[k] <= 3 && !((seen >> d.step[k]) & 1u), "%s: slot %d: bad or repeated colour step", who, s);
      seen |= 1u << d.step[k];
      contrast = contrast || d.step[k] == PCC_AUG_CONTRAST;
    }
    for (int a = 0; a < 3; ++a)
      PCC_REQUIRE(d.lo[a] <= d.hi[a] && d.lo[a] > -(int)PCC_BIAS + 64 && d.hi[a] < (int)PCC_BIAS - 64,
                  "%s: slot %d: coordinate box [%d, %d] is empty or outside the 16-bit key range", who, s, d.lo[a], d.hi[a]);
    const int64_t nb = pcc_cdiv(d.rows, PCC_AUG_BLOCK_ROWS);
    PCC_REQUIRE(d.first_block == blk && d.nblocks == nb && blk + nb <= nblocks, "%s: slot %d: block range does not match", who, s);
    for (int64_t b = 0; b < nb; ++b)
      PCC_REQUIRE(h_blocks[2 * (blk + b)] == s && h_blocks[2 * (blk + b) + 1] == b * PCC_AUG_BLOCK_ROWS,
                  "%s: block %lld is not (slot %d, row %lld)", who, (long long)(blk + b), s, (long long)b * PCC_AUG_BLOCK_ROWS);
    out += d.rows;
    blk += nb;
  }
  PCC_REQUIRE(blk == nblocks, "%s: %d blocks given, the slots need %lld", who, nblocks, (long long)blk);
  PCC_REQUIRE(out_rows < 0 || out == out_rows, "%s: the slots write %lld rows, the batch arrays hold %lld", who, (long long)out,
              (long long)out_rows);
  PCC_REQUIRE(out < (1ll << 31), "%s: batch too large", who);
  if (any_contrast) *any_contrast = contrast;
  return PCC_OK;
}

// ---- colour steps (torchvision ColorJitter on float images, restated; data.py's docstring has the formulas) ----------
// Contraction is switched off here as well: the steps are then the same fp32 operations, one rounding each, as the host
// restatement, and the kernel stays within the reference's own rounding noise of it (`/` is correctly rounded, fmodf and
// floorf are exact).  The rule is REQUIRED only for the rotation below.
__device__ __forceinline__ float aug_clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

__device__ __forceinline__ float aug_grey(float r, float g, float b) {
#pragma clang fp contract(off)
  return (0.2989f * r + 0.587f * g) + 0.114f * b;
}

__device__ __forceinline__ void aug_blend(float& r, float& g, float& b, float yr, float yg, float yb, float f) {
#pragma clang fp contract(off)
  const float f1 = 1.0f - f;
  r = aug_clamp01(f * r + f1 * yr);
  g = aug_clamp01(f * g + f1 * yg);
  b = aug_clamp01(f * b + f1 * yb);
}

__device__ __forceinline__ void aug_hue(float& r, float& g, float& b, float shift) {
#pragma clang fp contract(off)
  const float maxc = fmaxf(fmaxf(r, g), b), minc = fminf(fminf(r, g), b);
  const bool eqc = maxc == minc;
  const float cr = maxc - minc;
  const float s = cr / (eqc ? 1.0f : maxc);
  const float div = eqc ? 1.0f : cr;
  const float rc = (maxc - r) / div, gc = (maxc - g) / div, bc = (maxc - b) / div;
  const float hr = (maxc == r) ? bc - gc : 0.0f;
  const float hg = (maxc == g && maxc != r) ? (2.0f + rc) - bc : 0.0f;
  const float hb = (maxc != g && maxc != r) ? (4.0f + gc) - rc : 0.0f;
  float h = (hr + hg) + hb;
  h = fmodf(h / 6.0f + 1.0f, 1.0f);
  h = fmodf(h + shift, 1.0f);                                   // floored modulo: the divisor is positive
  if (h < 0.0f) h += 1.0f;
  const float v = maxc;
  const float h6 = h * 6.0f;
  const float fi = floorf(h6);
  const float f = h6 - fi;
  const int i = (int)fi % 6;
  const float p = aug_clamp01(v * (1.0f - s));
  const float q = aug_clamp01(v * (1.0f - s * f));
  const float t = aug_clamp01(v * (1.0f - s * (1.0f - f)));
  r = i == 0 ? v : i == 1 ? q : i == 2 ? p : i == 3 ? p : i == 4 ? t : v;
  g = i == 0 ? t : i == 1 ? v : i == 2 ? v : i == 3 ? q : i == 4 ? p : p;
  b = i == 0 ? p : i == 1 ? p : i == 2 ? t : i == 3 ? v : i == 4 ? v : q;
}

// steps [0, upto) of a slot; the slot's fields are uniform over the workgroup, so the branches do not diverge
__device__ __forceinline__ void aug_colour_steps(const AugSlot& d, int upto, float mean, float& r, float& g, float& b) {
  for (int k = 0; k < upto; ++k) {
    const int st = d.step[k];
    if (st == PCC_AUG_BRIGHTNESS) aug_blend(r, g, b, 0.0f, 0.0f, 0.0f, d.factor[0]);
    else if (st == PCC_AUG_CONTRAST) aug_blend(r, g, b, mean, mean, mean, d.factor[1]);
    else if (st == PCC_AUG_SATURATION) { const float y = aug_grey(r, g, b); aug_blend(r, g, b, y, y, y, d.factor[2]); }
    else aug_hue(r, g, b, d.factor[3]);
  }
}

// ---- the mean the contrast step blends with ----------------------------------------------------------------
// Grey value of every row AS THE CONTRAST STEP FINDS IT (after the steps drawn before it), summed in fp64 in a fixed order:
// lanes of a wave by butterfly, the four waves of a workgroup in order, one partial per workgroup at its own index; then
// one wave per slot sums that slot's partials (lane-strided, butterfly).  The same inputs give the same bits on every run.
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

__global__ void __launch_bounds__(AUG_T) k_aug_gray_partials(const float* __restrict__ colors, const AugSlot* __restrict__ slots,
                                                             const int2* __restrict__ blocks, double* __restrict__ partials) {
  __shared__ double s_w[AUG_T / PCC_WAVE];
  const int2 blk = blocks[blockIdx.x];
  const AugSlot& d = slots[blk.x];
  int at = -1;
  for (int k = 0; k < d.nsteps; ++k)
    if (d.step[k] == PCC_AUG_CONTRAST) at = k;
  if (at < 0) {                                   // uniform: the whole workgroup leaves
    if (threadIdx.x == 0) partials[blockIdx.x] = 0.0;
    return;
  }
  double acc = 0.0;
#pragma unroll
  for (int r = 0; r < AUG_R; ++r) {
    const int row = blk.y + r * AUG_T + (int)threadIdx.x;
    if (row < d.rows) {
      const float* c = colors + (long long)(d.in_begin + row) * 3;
      float cr = c[0], cg = c[1], cb = c[2];
      aug_colour_steps(d, at, 0.0f, cr, cg, cb);
      acc += (double)aug_grey(cr, cg, cb);
    }
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

__global__ void __launch_bounds__(PCC_WAVE) k_aug_gray_means(const AugSlot* __restrict__ slots, const double* __restrict__ partials,
                                                             float* __restrict__ means) {
  const AugSlot& d = slots[blockIdx.x];
  double acc = 0.0;
  for (int b = threadIdx.x; b < d.nblocks; b += PCC_WAVE) acc += partials[d.first_block + b];
  acc = wave_sum(acc);
  if (threadIdx.x == 0) means[blockIdx.x] = (float)(acc / (double)d.rows);
}

extern "C" int pcc_aug_gray_sums(const float* colors, int64_t table_rows, const int32_t* h_slots, const int32_t* d_slots,
                                 int32_t nslots, const int32_t* h_blocks, const int32_t* d_blocks, int32_t nblocks,
                                 double* partials, float* means, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  bool contrast = false;
  PCC_TRY(aug_validate("pcc_aug_gray_sums", h_slots, nslots, h_blocks, nblocks, table_rows, -1, &contrast));
  PCC_REQUIRE(colors && d_slots && d_blocks && partials && means, "pcc_aug_gray_sums: NULL array");
  if (!contrast) {                                // nothing to reduce: no launch
    PCC_CHECK_HIP(hipMemsetAsync(means, 0, (size_t)nslots * sizeof(float), s));
    return PCC_OK;
  }
  k_aug_gray_partials<<<(unsigned)nblocks, AUG_T, 0, s>>>(colors, (const AugSlot*)d_slots, (const int2*)d_blocks, partials);
  PCC_LAUNCH_CHECK();
  k_aug_gray_means<<<(unsigned)nslots, PCC_WAVE, 0, s>>>((const AugSlot*)d_slots, partials, means);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

// ---- the batch ---------------------------------------------------------------------------------------------
// out = (p - c) R^T + c, evaluated per axis as ((dx R[j][0] + dy R[j][1]) + dz R[j][2]) + c with EVERY product and sum
// rounded to fp32 on its own, then floorf: the voxel a point lands in is a defined function of its inputs that a host
// restatement reproduces bit for bit.  hipcc contracts a*b + c into an FMA by default, and __fmul_rn / __fadd_rn do not
// stop it; `#pragma clang fp contract(off)` at the top of the body does.  Checked on the built code object
// (llvm-objdump -d of the gfx950 image): k_aug_batch<false>, which holds the rotation and no division, contains
// v_mul_f32 / v_add_f32 / v_sub_f32 (and their packed forms) and no v_fma* / v_fmac*; in k_aug_batch<true> the only
// v_fma / v_div_fmas are the expansion of the hue step's correctly rounded divisions.
__device__ __forceinline__ void aug_rotate(const AugSlot& d, float px, float py, float pz, int& x, int& y, int& z) {
#pragma clang fp contract(off)
  const float c = d.centre;
  const float dx = px - c, dy = py - c, dz = pz - c;
  x = (int)floorf(((dx * d.rot[0] + dy * d.rot[1]) + dz * d.rot[2]) + c);
  y = (int)floorf(((dx * d.rot[3] + dy * d.rot[4]) + dz * d.rot[5]) + c);
  z = (int)floorf(((dx * d.rot[6] + dy * d.rot[7]) + dz * d.rot[8]) + c);
}

// One workgroup = PCC_AUG_BLOCK_ROWS consecutive rows of one slot (blocks[]: slot, first row).  Lane l of round r takes row
// first + r * 256 + l: a wave reads 768 contiguous bytes of points and of colours and writes 1024 contiguous bytes of
// coordinates (one 16-byte store per lane) and 768 of colours.
template <bool COLOUR>
__global__ void __launch_bounds__(AUG_T) k_aug_batch(const float* __restrict__ points, const float* __restrict__ colors,
                                                     const AugSlot* __restrict__ slots, const int2* __restrict__ blocks,
                                                     const float* __restrict__ means, int4* __restrict__ out_coords,
                                                     float* __restrict__ out_feats, int* __restrict__ outside) {
  const int2 blk = blocks[blockIdx.x];
  const int slot = blk.x;
  const AugSlot& d = slots[slot];
  const float mean = COLOUR ? means[slot] : 0.0f;
#pragma unroll
  for (int r = 0; r < AUG_R; ++r) {
    const int row = blk.y + r * AUG_T + (int)threadIdx.x;
    if (row >= d.rows) break;
    const long long src = (long long)(d.in_begin + row) * 3, dst = (long long)d.out_begin + row;
    int x, y, z;
    aug_rotate(d, points[src], points[src + 1], points[src + 2], x, y, z);
    // The caller sizes the de-duplication's lattice from the slot's box without reading the coordinates back.  The box is a
    // rigorous bound, so this never fires; if it ever did, the row stays inside the lattice and the caller is told.
    const int cx = min(max(x, d.lo[0]), d.hi[0]), cy = min(max(y, d.lo[1]), d.hi[1]), cz = min(max(z, d.lo[2]), d.hi[2]);
    if (cx != x || cy != y || cz != z) *outside = 1;          // benign race: every writer stores 1
    x = cx; y = cy; z = cz;
    out_coords[dst] = make_int4(slot, x, y, z);
    float cr = colors[src], cg = colors[src + 1], cb = colors[src + 2];
    if (COLOUR) aug_colour_steps(d, d.nsteps, mean, cr, cg, cb);
    out_feats[dst * 3] = cr; out_feats[dst * 3 + 1] = cg; out_feats[dst * 3 + 2] = cb;
  }
}

extern "C" int pcc_aug_batch(const float* points, const float* colors, int64_t table_rows, const int32_t* h_slots,
                             const int32_t* d_slots, int32_t nslots, const int32_t* h_blocks, const int32_t* d_blocks,
                             int32_t nblocks, const float* means, int32_t* out_coords, float* out_feats, int64_t out_rows,
                             int32_t* d_outside, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PCC_REQUIRE(d_outside, "pcc_aug_batch: d_outside is NULL");
  PCC_TRY(aug_validate("pcc_aug_batch", h_slots, nslots, h_blocks, nblocks, table_rows, out_rows, nullptr));
  PCC_REQUIRE(points && colors && d_slots && d_blocks && out_coords && out_feats, "pcc_aug_batch: NULL array");
  PCC_REQUIRE(((uintptr_t)out_coords & 15) == 0 && ((uintptr_t)d_blocks & 7) == 0 && ((uintptr_t)d_slots & 15) == 0,
              "pcc_aug_batch: coordinates / tables must be 16-byte aligned");
  bool colour = false;
  for (int i = 0; i < nslots; ++i) colour = colour || ((const AugSlot*)h_slots)[i].nsteps > 0;
  PCC_REQUIRE(!colour || means, "pcc_aug_batch: colour steps need the means array");
  PCC_CHECK_HIP(hipMemsetAsync(d_outside, 0, sizeof(int32_t), s));
  if (colour)
    k_aug_batch<true><<<(unsigned)nblocks, AUG_T, 0, s>>>(points, colors, (const AugSlot*)d_slots, (const int2*)d_blocks, means,
                                                          (int4*)out_coords, out_feats, d_outside);
  else
    k_aug_batch<false><<<(unsigned)nblocks, AUG_T, 0, s>>>(points, colors, (const AugSlot*)d_slots, (const int2*)d_blocks,
                                                           nullptr, (int4*)out_coords, out_feats, d_outside);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}
