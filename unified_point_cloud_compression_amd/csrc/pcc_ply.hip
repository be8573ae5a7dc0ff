// PLY vertex bodies on the device (include/pcc_hip.h section 10): binary records unpacked / packed through LDS, ASCII bodies
// tokenised, converted and formatted.  The header is the caller's business (ply.py parses and writes it in Python); these
// kernels see only body bytes.  Every read of the body is bounded by body_bytes and every write by the destination's extent:
// bad DATA (a short body, a token that is no number) is reported, never followed.  The property tables are small, come
// from the host and are validated there before any launch; they reach the kernels by value (uniform reads).
#include "pcc_common.h"

static constexpr int PLY_T = 256;                                  // threads per workgroup, every kernel here
static constexpr int PLY_CHUNK = PCC_PLY_TILE_BYTES / PLY_T;       // body bytes per thread of the token passes
static_assert(PLY_CHUNK == 16, "one 16-byte load per thread");
static constexpr int PLY_STAGE_LDS = PCC_PLY_STAGE_BYTES + 32;     // + the misalignment of a span's first byte, rounded up
static constexpr int PLY_ROW_MAX = 48;                             // 3 x "-2147483647" + 3 x "255" + 5 blanks + '\n'
static constexpr int PLY_TEXT_LDS = PLY_T * PLY_ROW_MAX;

struct PlySel { int off, type, arr, col, scale; };                 // off: byte offset in a record (binary) / property index (ASCII)
struct PlyTable {
  int nsel, nprops;
  PlySel sel[PCC_PLY_MAX_PROPS];
  signed char sel_of_prop[PCC_PLY_MAX_PROPS];                      // ASCII: property index -> entry of sel[], -1 = not selected
};
struct PlyDst {                                                    // element (row, column) of array a lives at base[a][row * rs[a] + col * cs[a]]
  float* base[3];
  long long rs[3], cs[3];
};

static const int PLY_SIZE[8] = {1, 1, 2, 2, 4, 4, 4, 8};

// The table as the kernels will use it, or PCC_EINVAL: every destination inside its array, no destination twice, the colour
// scale on uchar only, and (binary) every field inside the record / (ASCII) every property index below nprops and used once.
static int ply_table(const char* who, const int32_t* h_table, int32_t nsel, bool ascii, int32_t stride_or_nprops, int64_t n,
                     float* cloud, int32_t cloud_cols, float* normals, float* extra, int32_t extra_cols, PlyTable* tb, PlyDst* dst) {
  PCC_REQUIRE(h_table && nsel >= 1 && nsel <= PCC_PLY_MAX_PROPS, "%s: %d selected properties (1..%d)", who, nsel, PCC_PLY_MAX_PROPS);
  PCC_REQUIRE(cloud && (cloud_cols == 3 || cloud_cols == 6), "%s: the cloud has 3 or 6 columns, not %d", who, cloud_cols);
  PCC_REQUIRE(extra_cols >= 0 && extra_cols <= PCC_PLY_MAX_PROPS && (extra_cols == 0 || extra), "%s: bad extra columns", who);
  const int cols[3] = {cloud_cols, normals ? 3 : 0, extra_cols};
  unsigned seen[3] = {0, 0, 0}, seen_prop = 0;
  tb->nsel = nsel;
  tb->nprops = ascii ? stride_or_nprops : 0;
  for (int p = 0; p < PCC_PLY_MAX_PROPS; ++p) tb->sel_of_prop[p] = -1;
  for (int k = 0; k < nsel; ++k) {
    const int32_t* e = h_table + 5 * k;
    PCC_REQUIRE(e[1] >= 0 && e[1] <= PCC_PLY_F64, "%s: entry %d: unknown type %d", who, k, e[1]);
    PCC_REQUIRE(e[2] >= 0 && e[2] <= 2 && e[3] >= 0 && e[3] < cols[e[2]], "%s: entry %d: destination (%d, %d) outside its array", who, k,
                e[2], e[3]);
    PCC_REQUIRE(!((seen[e[2]] >> e[3]) & 1u), "%s: entry %d: destination (%d, %d) given twice", who, k, e[2], e[3]);
    seen[e[2]] |= 1u << e[3];
    PCC_REQUIRE(e[4] == 0 || (e[4] == 1 && e[1] == PCC_PLY_U8), "%s: entry %d: the colour scale is for uchar", who, k);
    if (ascii) {
      PCC_REQUIRE(e[0] >= 0 && e[0] < stride_or_nprops && !((seen_prop >> e[0]) & 1u), "%s: entry %d: property %d outside 0..%d or given twice",
                  who, k, e[0], stride_or_nprops - 1);
      seen_prop |= 1u << e[0];
      tb->sel_of_prop[e[0]] = (signed char)k;
    } else {
      PCC_REQUIRE(e[0] >= 0 && e[0] + PLY_SIZE[e[1]] <= stride_or_nprops, "%s: entry %d: bytes [%d, %d) outside a record of %d", who, k, e[0],
                  e[0] + PLY_SIZE[e[1]], stride_or_nprops);
    }
    tb->sel[k] = PlySel{e[0], e[1], e[2], e[3], e[4]};
  }
  dst->base[0] = cloud; dst->rs[0] = cloud_cols; dst->cs[0] = 1;
  dst->base[1] = normals; dst->rs[1] = 3; dst->cs[1] = 1;
  dst->base[2] = extra; dst->rs[2] = 1; dst->cs[2] = n;             // [extra_cols][n]: each column contiguous
  return PCC_OK;
}

// integer types round to nearest fp32 (exact below 2^24), double rounds to nearest; a uchar colour is the fp32 quotient
// k / 255 (hipcc's `/` is the correctly rounded division, not a reciprocal multiply)
__device__ __forceinline__ float ply_convert(unsigned long long raw, int type, int scale) {
  float v;
  switch (type) {
    case PCC_PLY_I8: v = (float)(signed char)raw; break;
    case PCC_PLY_U8: v = (float)(unsigned char)raw; break;
    case PCC_PLY_I16: v = (float)(short)raw; break;
    case PCC_PLY_U16: v = (float)(unsigned short)raw; break;
    case PCC_PLY_I32: v = (float)(int)raw; break;
    case PCC_PLY_U32: v = (float)(unsigned)raw; break;
    case PCC_PLY_F32: v = __uint_as_float((unsigned)raw); break;
    default: v = (float)__longlong_as_double((long long)raw); break;
  }
  return scale ? v / 255.0f : v;
}

// 16 bytes at offset g (a multiple of 16; the base is 16-byte aligned) of a buffer of nbytes: one wide load where the
// buffer holds all of them, single bytes (absent ones read as `fill`) at its end
__device__ __forceinline__ uint4 ply_load16(const unsigned char* __restrict__ buf, long long nbytes, long long g, unsigned fill) {
  if (g + 16 <= nbytes) return *reinterpret_cast<const uint4*>(buf + g);
  unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < 16; ++k) w[k >> 2] |= (g + k < nbytes ? (unsigned)buf[g + k] : fill) << (8 * (k & 3));
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// ------------------------------------------------------------------------------------------
// binary read
// ------------------------------------------------------------------------------------------
// One workgroup = rb consecutive records = one contiguous span of rb * stride <= PCC_PLY_STAGE_BYTES body bytes.  The span
// is brought into LDS with aligned 16-byte loads (from the 16-byte boundary at or below its first byte), then every thread
// picks the selected fields of its records out of LDS byte by byte: records of 15 or 27 bytes put fields at any offset, and
// nothing here assumes an alignment.
__global__ void __launch_bounds__(PLY_T) k_ply_unpack(const unsigned char* __restrict__ body, long long body_bytes, long long n, int stride,
                                                      int rb, int big, PlyTable tb, PlyDst dst) {
  __shared__ uint4 s_q[PLY_STAGE_LDS / 16];
  const unsigned char* s = reinterpret_cast<const unsigned char*>(s_q);
  const long long r0 = (long long)blockIdx.x * rb;
  const int nr = (int)min((long long)rb, n - r0);
  const long long b0 = r0 * stride, b1 = b0 + (long long)nr * stride;      // b1 <= n * stride <= body_bytes (checked by the host)
  const long long a0 = b0 & ~15ll;
  const int shift = (int)(b0 - a0);
  const int nq = (int)((b1 - a0 + 15) >> 4);                                // <= (STAGE + 15 + 15) / 16 < PLY_STAGE_LDS / 16
  for (int q = threadIdx.x; q < nq; q += PLY_T) s_q[q] = ply_load16(body, body_bytes, a0 + 16ll * q, 0u);
  __syncthreads();
  for (int r = threadIdx.x; r < nr; r += PLY_T) {
    const unsigned char* rec = s + shift + r * stride;
    for (int k = 0; k < tb.nsel; ++k) {
      const PlySel e = tb.sel[k];
      const int size = e.type == PCC_PLY_F64 ? 8 : e.type >= PCC_PLY_I32 ? 4 : e.type >= PCC_PLY_I16 ? 2 : 1;
      unsigned long long raw = 0;
      for (int b = 0; b < size; ++b) raw |= (unsigned long long)rec[e.off + b] << (8 * (big ? size - 1 - b : b));
      dst.base[e.arr][(r0 + r) * dst.rs[e.arr] + e.col * dst.cs[e.arr]] = ply_convert(raw, e.type, e.scale);
    }
  }
}

extern "C" int32_t pcc_ply_block_records(int32_t stride) {
  if (stride < 1 || stride > PCC_PLY_STAGE_BYTES) return 0;
  const int rb = PCC_PLY_STAGE_BYTES / stride;
  return rb > 1024 ? 1024 : rb;
}

extern "C" int pcc_ply_unpack_binary(const uint8_t* body, int64_t body_bytes, int64_t n, int32_t stride, const int32_t* h_table,
                                     int32_t nsel, int32_t big_endian, float* cloud, int32_t cloud_cols, float* normals, float* extra,
                                     int32_t extra_cols, void* stream) {
  PCC_REQUIRE(n >= 0 && n < (1ll << 31) && stride >= 1 && stride <= PCC_PLY_MAX_PROPS * 8, "pcc_ply_unpack_binary: %lld records of %d bytes",
              (long long)n, stride);
  PCC_REQUIRE(body_bytes >= 0 && n * stride <= body_bytes, "pcc_ply_unpack_binary: %lld records of %d bytes need %lld bytes, the body has %lld",
              (long long)n, stride, (long long)n * stride, (long long)body_bytes);
  if (n == 0) return PCC_OK;
  PlyTable tb;
  PlyDst dst;
  PCC_TRY(ply_table("pcc_ply_unpack_binary", h_table, nsel, false, stride, n, cloud, cloud_cols, normals, extra, extra_cols, &tb, &dst));
  PCC_REQUIRE(body && ((uintptr_t)body & 15) == 0, "pcc_ply_unpack_binary: the body must be 16-byte aligned");
  const int rb = pcc_ply_block_records(stride);
  k_ply_unpack<<<(unsigned)pcc_cdiv(n, rb), PLY_T, 0, (hipStream_t)stream>>>(body, body_bytes, n, stride, rb, big_endian ? 1 : 0, tb, dst);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

// ------------------------------------------------------------------------------------------
// ASCII read
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ bool ply_ws(unsigned c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n'; }

// bit k set: byte g + k starts a token (it is not whitespace and the byte before it is whitespace or the body's start).
// Bytes past the end of the body read as blanks.
__device__ __forceinline__ unsigned ply_starts16(const unsigned char* __restrict__ body, long long nbytes, long long g) {
  if (g >= nbytes) return 0u;
  const uint4 v = ply_load16(body, nbytes, g, (unsigned)' ');
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
  bool prev_ws = g == 0 || ply_ws(body[g - 1]);
  unsigned mask = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const bool ws = ply_ws((w[k >> 2] >> (8 * (k & 3))) & 0xFFu);
    if (!ws && prev_ws) mask |= 1u << k;
    prev_ws = ws;
  }
  return mask;
}

// exclusive prefix of v over the workgroup (thread order) and the workgroup's total
__device__ __forceinline__ int ply_block_scan(int v, int* s_w, int& total) {
  int inc = v;
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d);
    if (lane >= d) inc += o;
  }
  if (lane == 63) s_w[threadIdx.x >> 6] = inc;
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < PLY_T / 64; ++w) {
    if (w < (int)(threadIdx.x >> 6)) base += s_w[w];
    total += s_w[w];
  }
  return base + inc - v;
}

// pass 1: token starts per tile of PCC_PLY_TILE_BYTES
__global__ void __launch_bounds__(PLY_T) k_ply_count(const unsigned char* __restrict__ body, long long nbytes, int* __restrict__ counts) {
  __shared__ int s_w[PLY_T / 64];
  const long long g = (long long)blockIdx.x * PCC_PLY_TILE_BYTES + threadIdx.x * PLY_CHUNK;
  int total;
  ply_block_scan(__popc(ply_starts16(body, nbytes, g)), s_w, total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// pass 2a: the byte offset of token t, for t below `limit` (= n * nprops: later tokens are face data); the last tile leaves
// the body's token count in status[0]
__global__ void __launch_bounds__(PLY_T) k_ply_mark(const unsigned char* __restrict__ body, long long nbytes, const int* __restrict__ tile_base,
                                                    long long limit, int* __restrict__ starts, long long* __restrict__ status) {
  __shared__ int s_w[PLY_T / 64];
  const long long g = (long long)blockIdx.x * PCC_PLY_TILE_BYTES + threadIdx.x * PLY_CHUNK;
  unsigned mask = ply_starts16(body, nbytes, g);
  int total;
  long long t = (long long)tile_base[blockIdx.x] + ply_block_scan(__popc(mask), s_w, total);
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) status[0] = (long long)tile_base[blockIdx.x] + total;
  while (mask) {
    const int k = __ffs((int)mask) - 1;
    mask &= mask - 1;
    if (t >= 0 && t < limit) starts[t] = (int)(g + k);
    ++t;
  }
}

__constant__ double PLY_POW10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                     1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

enum { PLY_TOK_OK = 0, PLY_TOK_FALLBACK = 1, PLY_TOK_ERROR = 2 };

// One token of `len` (<= PCC_PLY_TOKEN_MAX) bytes at tok.  Integer types: [+-]digits, exact, inside the type's range.
// Float types: [+-](digits[.digits] | .digits)[(e|E)[+-]digits]; with at most 15 significant digits and a power of ten
// within +-22 the value is m * 10^e or m / 10^e, ONE correctly rounded fp64 operation on two exact operands, which is the
// correctly rounded double of the decimal string (what `float(token)` returns); rounding that to fp32 follows.  A number
// outside these limits, and nan / inf / infinity, is left to the host (FALLBACK); anything else is no number (ERROR).
__device__ int ply_parse_token(const unsigned char* __restrict__ tok, int len, int type, float* out) {
  int i = 0;
  bool neg = false;
  auto at = [&](int j) -> unsigned { return j < len ? (unsigned)tok[j] : 0u; };
  if (at(0) == '+' || at(0) == '-') { neg = at(0) == '-'; i = 1; }
  unsigned long long m = 0;
  int sig = 0, nd = 0, frac = 0;
  for (unsigned c = at(i); c >= '0' && c <= '9'; c = at(++i)) {
    ++nd;
    if (m || c != '0') ++sig;
    if (sig <= 18) m = m * 10 + (c - '0');
  }
  if (type < PCC_PLY_F32) {
    if (nd == 0 || i != len) return PLY_TOK_ERROR;                  // also a decimal point or an exponent in an integer property
    if (sig > 18) return PLY_TOK_FALLBACK;
    const long long v = neg ? -(long long)m : (long long)m;
    const long long lo = type == PCC_PLY_I8 ? -128 : type == PCC_PLY_I16 ? -32768 : type == PCC_PLY_I32 ? -2147483648ll : 0;
    const long long hi = type == PCC_PLY_I8 ? 127 : type == PCC_PLY_U8 ? 255 : type == PCC_PLY_I16 ? 32767 : type == PCC_PLY_U16 ? 65535
                         : type == PCC_PLY_I32 ? 2147483647ll : 4294967295ll;
    if (v < lo || v > hi) return PLY_TOK_ERROR;
    *out = (float)v;
    return PLY_TOK_OK;
  }
  if (nd == 0 && at(i) != '.') {                                    // nan, inf, infinity in any letter case: the host's
    const int rest = len - i;
    const char* word = rest == 3 && (at(i) | 32u) == 'n' ? "nan" : rest == 3 ? "inf" : rest == 8 ? "infinity" : nullptr;
    if (!word) return PLY_TOK_ERROR;
    for (int j = 0; j < rest; ++j)
      if ((at(i + j) | 32u) != (unsigned)word[j]) return PLY_TOK_ERROR;
    return PLY_TOK_FALLBACK;
  }
  if (at(i) == '.') {
    for (unsigned c = at(++i); c >= '0' && c <= '9'; c = at(++i)) {
      ++nd;
      if (m || c != '0') ++sig;
      if (sig <= 18) { m = m * 10 + (c - '0'); ++frac; }
    }
  }
  if (nd == 0) return PLY_TOK_ERROR;
  int ex = 0;
  bool ex_big = false;
  if (at(i) == 'e' || at(i) == 'E') {
    ++i;
    bool eneg = false;
    if (at(i) == '+' || at(i) == '-') { eneg = at(i) == '-'; ++i; }
    int ed = 0;
    for (unsigned c = at(i); c >= '0' && c <= '9'; c = at(++i)) {
      ++ed;
      if (ex < 100000) ex = ex * 10 + (int)(c - '0'); else ex_big = true;
    }
    if (ed == 0) return PLY_TOK_ERROR;
    if (eneg) ex = -ex;
  }
  if (i != len) return PLY_TOK_ERROR;
  if (sig > 15 || ex_big) return PLY_TOK_FALLBACK;
  double v;
  const int e10 = ex - frac;
  if (m == 0) v = 0.0;
  else if (e10 >= 0 && e10 <= 22) v = (double)m * PLY_POW10[e10];
  else if (e10 < 0 && e10 >= -22) v = (double)m / PLY_POW10[-e10];
  else return PLY_TOK_FALLBACK;
  *out = (float)(neg ? -v : v);
  return PLY_TOK_OK;
}

// pass 2b: one lane per token.  Token t is property t % nprops of vertex t / nprops.
__global__ void __launch_bounds__(PLY_T) k_ply_parse(const unsigned char* __restrict__ body, long long nbytes, const int* __restrict__ starts,
                                                     long long limit, PlyTable tb, PlyDst dst, long long* __restrict__ status,
                                                     long long* __restrict__ fallback, int cap) {
  const long long t = (long long)blockIdx.x * PLY_T + threadIdx.x;
  if (t >= limit || t >= status[0]) return;                        // a truncated body: the host sees the count and refuses
  const int k = tb.sel_of_prop[(int)(t % tb.nprops)];
  if (k < 0) return;
  const PlySel e = tb.sel[k];
  const long long off = starts[t];
  if (off < 0 || off >= nbytes) return;                            // (pass 2a writes offsets inside the body only)
  int len = 0;
  while (len <= PCC_PLY_TOKEN_MAX && off + len < nbytes && !ply_ws(body[off + len])) ++len;
  float v = 0.0f;
  const int rc = len > PCC_PLY_TOKEN_MAX ? PLY_TOK_FALLBACK : ply_parse_token(body + off, len, e.type, &v);
  if (rc == PLY_TOK_OK) {
    dst.base[e.arr][(t / tb.nprops) * dst.rs[e.arr] + e.col * dst.cs[e.arr]] = e.scale ? v / 255.0f : v;
  } else if (rc == PLY_TOK_FALLBACK) {
    const unsigned long long slot = atomicAdd(reinterpret_cast<unsigned long long*>(status + 1), 1ull);
    if (slot < (unsigned long long)cap) {
      fallback[2 * slot] = t;
      fallback[2 * slot + 1] = off;
    }
  } else {
    atomicMin(reinterpret_cast<unsigned long long*>(status + 2), ((unsigned long long)t << 32) | (unsigned long long)off);
  }
}

extern "C" int32_t pcc_ply_tile_bytes(void) { return PCC_PLY_TILE_BYTES; }

extern "C" int pcc_ply_count_tokens(const uint8_t* body, int64_t body_bytes, int32_t* tile_counts, void* stream) {
  PCC_REQUIRE(body_bytes >= 0 && body_bytes < (1ll << 31), "pcc_ply_count_tokens: a body of %lld bytes (below 2^31)", (long long)body_bytes);
  if (body_bytes == 0) return PCC_OK;
  PCC_REQUIRE(body && tile_counts && ((uintptr_t)body & 15) == 0, "pcc_ply_count_tokens: NULL array or a body that is not 16-byte aligned");
  k_ply_count<<<(unsigned)pcc_cdiv(body_bytes, PCC_PLY_TILE_BYTES), PLY_T, 0, (hipStream_t)stream>>>(body, body_bytes, tile_counts);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_ply_parse_ascii(const uint8_t* body, int64_t body_bytes, int64_t n, int32_t nprops, const int32_t* h_table, int32_t nsel,
                                   const int32_t* tile_base, int32_t* starts, float* cloud, int32_t cloud_cols, float* normals, float* extra,
                                   int32_t extra_cols, int64_t* status, int64_t* fallback, int32_t fallback_cap, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PCC_REQUIRE(status, "pcc_ply_parse_ascii: status is NULL");
  PCC_REQUIRE(body_bytes >= 0 && body_bytes < (1ll << 31), "pcc_ply_parse_ascii: a body of %lld bytes (below 2^31)", (long long)body_bytes);
  PCC_REQUIRE(n >= 0 && nprops >= 1 && nprops <= PCC_PLY_MAX_PROPS && n * nprops < (1ll << 31), "pcc_ply_parse_ascii: %lld vertices of %d properties",
              (long long)n, nprops);
  PCC_REQUIRE(fallback_cap >= 0 && (fallback_cap == 0 || fallback), "pcc_ply_parse_ascii: bad fallback list");
  PCC_CHECK_HIP(hipMemsetAsync(status, 0, 2 * sizeof(int64_t), s));
  PCC_CHECK_HIP(hipMemsetAsync(status + 2, 0xFF, sizeof(int64_t), s));
  if (n == 0 || body_bytes == 0) return PCC_OK;                      // (an empty body with n > 0: status[0] = 0 tokens)
  PlyTable tb;
  PlyDst dst;
  PCC_TRY(ply_table("pcc_ply_parse_ascii", h_table, nsel, true, nprops, n, cloud, cloud_cols, normals, extra, extra_cols, &tb, &dst));
  PCC_REQUIRE(body && tile_base && starts && ((uintptr_t)body & 15) == 0, "pcc_ply_parse_ascii: NULL array or a body that is not 16-byte aligned");
  const long long limit = n * nprops;
  k_ply_mark<<<(unsigned)pcc_cdiv(body_bytes, PCC_PLY_TILE_BYTES), PLY_T, 0, s>>>(body, body_bytes, tile_base, limit, starts, (long long*)status);
  PCC_LAUNCH_CHECK();
  k_ply_parse<<<(unsigned)pcc_cdiv(limit, PLY_T), PLY_T, 0, s>>>(body, body_bytes, starts, limit, tb, dst, (long long*)status, (long long*)fallback,
                                                                 fallback_cap);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

// ------------------------------------------------------------------------------------------
// writers
// ------------------------------------------------------------------------------------------
// clamp(rint(255 f), 0, 255): the 8-bit level `UnifiedModel.decompress` rounds a colour to (k_decode_finish)
__device__ __forceinline__ unsigned ply_level(float f) { return (unsigned)fminf(fmaxf(rintf(f * 255.0f), 0.0f), 255.0f); }

__device__ __forceinline__ bool ply_is_int(float x) { return x == rintf(x) && fabsf(x) < 2147483648.0f; }   // (NaN fails the first)

// Binary little-endian records x y z [nx ny nz] [r g b].  One workgroup builds PLY_T records in LDS and writes their span
// with 16-byte stores: PLY_T * stride is a multiple of 16 for every stride, so each span starts aligned.
__global__ void __launch_bounds__(PLY_T) k_ply_pack(const float* __restrict__ cloud, int cols, const float* __restrict__ normals, long long n,
                                                    int stride, int coords_int, unsigned char* __restrict__ out, int* __restrict__ flag) {
  __shared__ uint4 s_q[PLY_T * 27 / 16];
  unsigned char* s = reinterpret_cast<unsigned char*>(s_q);
  const long long r0 = (long long)blockIdx.x * PLY_T, r = r0 + threadIdx.x;
  if (r < n) {
    unsigned char* rec = s + threadIdx.x * stride;
    int at = 0;
    auto put32 = [&](unsigned w) {
#pragma unroll
      for (int b = 0; b < 4; ++b) rec[at + b] = (unsigned char)(w >> (8 * b));
      at += 4;
    };
    for (int a = 0; a < 3; ++a) {
      const float x = cloud[r * cols + a];
      if (coords_int) {
        if (!ply_is_int(x)) *flag = 1;                               // benign race: every writer stores 1
        put32((unsigned)(int)x);
      } else {
        put32(__float_as_uint(x));
      }
    }
    if (normals)
      for (int a = 0; a < 3; ++a) put32(__float_as_uint(normals[r * 3 + a]));
    if (cols == 6)
      for (int a = 0; a < 3; ++a) rec[at++] = (unsigned char)ply_level(cloud[r * 6 + 3 + a]);
  }
  __syncthreads();
  const int nr = (int)min((long long)PLY_T, n - r0);
  const int nbytes = nr * stride;
  unsigned char* o = out + r0 * stride;
  for (int q = threadIdx.x; q * 16 < nbytes; q += PLY_T) {
    if (q * 16 + 16 <= nbytes) reinterpret_cast<uint4*>(o)[q] = s_q[q];
    else
      for (int b = q * 16; b < nbytes; ++b) o[b] = s[b];
  }
}

extern "C" int pcc_ply_pack_binary(const float* cloud, int32_t cloud_cols, const float* normals, int64_t n, int32_t coords_int, uint8_t* out,
                                   int64_t out_bytes, int32_t* d_flag, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PCC_REQUIRE(d_flag, "pcc_ply_pack_binary: d_flag is NULL");
  PCC_REQUIRE(cloud_cols == 3 || cloud_cols == 6, "pcc_ply_pack_binary: the cloud has 3 or 6 columns, not %d", cloud_cols);
  PCC_CHECK_HIP(hipMemsetAsync(d_flag, 0, sizeof(int32_t), s));
  if (n <= 0) return PCC_OK;
  const int stride = 12 + (normals ? 12 : 0) + (cloud_cols == 6 ? 3 : 0);
  PCC_REQUIRE(cloud && out && n < (1ll << 31) && ((uintptr_t)out & 15) == 0, "pcc_ply_pack_binary: bad arguments");
  PCC_REQUIRE(out_bytes >= n * stride, "pcc_ply_pack_binary: %lld records of %d bytes do not fit %lld bytes", (long long)n, stride,
              (long long)out_bytes);
  k_ply_pack<<<(unsigned)pcc_cdiv(n, PLY_T), PLY_T, 0, s>>>(cloud, cloud_cols, normals, n, stride, coords_int ? 1 : 0, out, d_flag);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

__device__ __forceinline__ int ply_int_len(int v) {
  unsigned u = v < 0 ? 0u - (unsigned)v : (unsigned)v;
  int len = v < 0 ? 2 : 1;
  while (u >= 10u) { u /= 10u; ++len; }
  return len;
}

// text pass 1: bytes of row i = its integers' digits and signs, a blank between two of them, '\n'
__global__ void __launch_bounds__(PLY_T) k_ply_row_len(const float* __restrict__ cloud, int cols, long long n, int* __restrict__ lengths,
                                                       int* __restrict__ flag) {
  const long long i = (long long)blockIdx.x * PLY_T + threadIdx.x;
  if (i >= n) return;
  int len = cols;                                                    // cols - 1 blanks and the line end
  for (int a = 0; a < 3; ++a) {
    const float x = cloud[i * cols + a];
    const bool ok = ply_is_int(x);
    if (!ok) *flag = 1;                                              // benign race: every writer stores 1
    len += ply_int_len(ok ? (int)x : 0);
  }
  if (cols == 6)
    for (int a = 0; a < 3; ++a) len += ply_int_len((int)ply_level(cloud[i * 6 + 3 + a]));
  lengths[i] = len;
}

__device__ __forceinline__ int ply_put_int(unsigned char* p, int v) {   // writes v at p, returns its length
  const int len = ply_int_len(v);
  unsigned u = v < 0 ? 0u - (unsigned)v : (unsigned)v;
  for (int k = len - 1; k >= (v < 0 ? 1 : 0); --k) { p[k] = (unsigned char)('0' + u % 10u); u /= 10u; }
  if (v < 0) p[0] = '-';
  return len;
}

// text pass 2: the rows of a workgroup are one contiguous span of the output, [offs[r0], offs[r0 + nr]).  Each lane writes
// its row into LDS at its offset in the span; the span then leaves as whole aligned 4-byte words, single bytes at its ends.
// The offsets are the caller's scan of pass 1; a row whose offsets do not hold its text is dropped, not written elsewhere.
__global__ void __launch_bounds__(PLY_T) k_ply_format(const float* __restrict__ cloud, int cols, long long n, const long long* __restrict__ offs,
                                                      unsigned char* __restrict__ out, long long out_bytes) {
  __shared__ unsigned s_w[PLY_TEXT_LDS / 4];
  unsigned char* s = reinterpret_cast<unsigned char*>(s_w);
  const long long r0 = (long long)blockIdx.x * PLY_T, r = r0 + threadIdx.x;
  const int nr = (int)min((long long)PLY_T, n - r0);
  const long long b0 = offs[r0], b1 = offs[r0 + nr];
  if (b0 < 0 || b1 < b0 || b1 > out_bytes || b1 - b0 > PLY_TEXT_LDS) return;     // uniform over the workgroup
  if (r < n) {
    int v[6];
    int len = cols;
    for (int a = 0; a < 3; ++a) {
      const float x = cloud[r * cols + a];
      v[a] = ply_is_int(x) ? (int)x : 0;
    }
    for (int a = 3; a < cols; ++a) v[a] = (int)ply_level(cloud[r * 6 + a]);
    for (int a = 0; a < cols; ++a) len += ply_int_len(v[a]);
    const long long lo = offs[r] - b0;
    if (lo >= 0 && lo + len <= b1 - b0 && offs[r + 1] - offs[r] == len) {
      unsigned char* p = s + lo;
      for (int a = 0; a < cols; ++a) {
        p += ply_put_int(p, v[a]);
        *p++ = a + 1 < cols ? ' ' : '\n';
      }
    }
  }
  __syncthreads();
  const long long w0 = b0 & ~3ll;
  for (long long g = w0 + 4ll * threadIdx.x; g < b1; g += 4ll * PLY_T) {
    if (g >= b0 && g + 4 <= b1) {
      const unsigned char* p = s + (g - b0);
      *reinterpret_cast<unsigned*>(out + g) = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24);
    } else {
      for (long long b = g < b0 ? b0 : g; b < g + 4 && b < b1; ++b) out[b] = s[b - b0];
    }
  }
}

extern "C" int pcc_ply_row_lengths(const float* cloud, int32_t cloud_cols, int64_t n, int32_t* lengths, int32_t* d_flag, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PCC_REQUIRE(d_flag, "pcc_ply_row_lengths: d_flag is NULL");
  PCC_REQUIRE(cloud_cols == 3 || cloud_cols == 6, "pcc_ply_row_lengths: the cloud has 3 or 6 columns, not %d", cloud_cols);
  PCC_CHECK_HIP(hipMemsetAsync(d_flag, 0, sizeof(int32_t), s));
  if (n <= 0) return PCC_OK;
  PCC_REQUIRE(cloud && lengths && n < (1ll << 31), "pcc_ply_row_lengths: bad arguments");
  k_ply_row_len<<<(unsigned)pcc_cdiv(n, PLY_T), PLY_T, 0, s>>>(cloud, cloud_cols, n, lengths, d_flag);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}

extern "C" int pcc_ply_format_ascii(const float* cloud, int32_t cloud_cols, int64_t n, const int64_t* row_offsets, uint8_t* out, int64_t out_bytes,
                                    void* stream) {
  PCC_REQUIRE(cloud_cols == 3 || cloud_cols == 6, "pcc_ply_format_ascii: the cloud has 3 or 6 columns, not %d", cloud_cols);
  if (n <= 0) return PCC_OK;
  PCC_REQUIRE(cloud && row_offsets && out && n < (1ll << 31) && out_bytes >= 0 && ((uintptr_t)out & 3) == 0, "pcc_ply_format_ascii: bad arguments");
  k_ply_format<<<(unsigned)pcc_cdiv(n, PLY_T), PLY_T, 0, (hipStream_t)stream>>>(cloud, cloud_cols, n, (const long long*)row_offsets, out, out_bytes);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}
