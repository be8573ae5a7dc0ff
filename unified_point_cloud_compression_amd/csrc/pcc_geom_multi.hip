// Several references per frame, device side (DESIGN.md section 7e "Several references", stream format 0xAB): every block of an inter
// frame takes its prediction from one of up to four reference slots.
//   k_multi_block_bits   one wave per block.  Encoder form (cur given): for each slot in order, the slot's occupancy pyramid under
//                        the slot's own vector for this block (the probe of k_inter_block_bits, then the coarser tiers word by word
//                        from a ballot), its match count = popcount of the finest tier AND the current frame's, summed over the wave
//                        by shuffles; the best pyramid so far is kept in a second LDS buffer and replaced only by a strictly larger
//                        count, so a tie stays with the lower slot.  Decoder form (cur NULL): the pyramid of the slot sel[b] names,
//                        under the one vector the stream carries for the block.
// A vector is a packed displacement (pcc_geom_inter.h), so one kernel serves every search range.  No atomics, integers only; every
// store is a vector store, every buffer is addressed by the block's row.  LDS: two pyramids, 1200 bytes.
#include "pcc_geom_inter.h"

static constexpr int MULTI_MAX_SLOTS = 4;

struct MultiRefs {
  const int64_t* keys[MULTI_MAX_SLOTS];
  int n[MULTI_MAX_SLOTS];
  PccGrid g[MULTI_MAX_SLOTS];
};

// the pyramid of one source in w (all 75 words), for the block whose displaced corner is (x0, y0, z0)
__device__ __forceinline__ void multi_pyramid(unsigned long long* w, int lane, int bl, const PccGrid& sg, const int64_t* __restrict__ skeys,
                                              int ns, int x0, int y0, int z0) {
  for (int t = lane; t < INTER_PYR; t += 64) w[t] = 0;
  __syncthreads();
  INTER_PROBE_FINEST(w, lane, bl, sg, skeys, ns, x0, y0, z0)
  __syncthreads();
  for (int e = bl - 1; e >= 0; --e) {
    const int ce = 1 << (3 * e), se = (1 << e) - 1, tier_words = ce > 64 ? ce >> 6 : 1;
    for (int i = 0; i < tier_words; ++i) {                    // lane <-> cell 64 i + lane: the ballot is word i of the tier
      const int c = i * 64 + lane;
      int any = 0;
      if (c < ce) {
        const int lx = c >> (2 * e), ly = (c >> e) & se, lz = c & se;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int cc = ((2 * lx + ((j >> 2) & 1)) << (2 * (e + 1))) | ((2 * ly + ((j >> 1) & 1)) << (e + 1)) | (2 * lz + (j & 1));
          any |= (int)((w[inter_tier(e + 1) + (cc >> 6)] >> (cc & 63)) & 1ull);
        }
      }
      const unsigned long long m = __ballot(any);
      if (lane == 0) w[inter_tier(e) + i] = m;
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(64) k_multi_block_bits(const int64_t* __restrict__ bkeys, int nb, int bl, MultiRefs refs, int K, int ox,
                                                         int oy, int oz, const int* __restrict__ vecs, int search,
                                                         const unsigned long long* __restrict__ cur, int* __restrict__ sel,
                                                         int* __restrict__ disp, unsigned long long* __restrict__ pyr,
                                                         int* __restrict__ counts, int* __restrict__ d_bad) {
  __shared__ unsigned long long w[INTER_PYR];
  __shared__ unsigned long long keep[INTER_PYR];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int64_t key = bkeys[b];
  const int bx = ox + pcc_key_x(key), by = oy + pcc_key_y(key), bz = oz + pcc_key_z(key);
  const int cells = 1 << (3 * bl), words = cells > 64 ? cells >> 6 : 1;
  const bool encoder = cur != nullptr;
  int chosen = 0;
  if (!encoder) {
    chosen = sel[b];
    if (chosen < 0 || chosen >= K) { if (lane == 0) *d_bad = 1; chosen = 0; }
  }
  const unsigned long long mine = (encoder && lane < words) ? cur[(int64_t)b * INTER_PYR + inter_tier(bl) + lane] : 0ull;
  int best = -1, best_slot = 0, best_disp = wide_pack(0, 0, 0);
#pragma unroll
  for (int s = 0; s < MULTI_MAX_SLOTS; ++s) {
    if (s >= K || (!encoder && s != chosen)) continue;
    int p = vecs[encoder ? (int64_t)s * nb + b : (int64_t)b], dx, dy, dz;
    if (!wide_unpack(p, search, dx, dy, dz)) { if (lane == 0) *d_bad = 1; p = wide_pack(0, 0, 0); }
    multi_pyramid(w, lane, bl, refs.g[s], refs.keys[s], refs.n[s], bx - dx, by - dy, bz - dz);
    if (!encoder) break;
    int c = lane < words ? __popcll(mine & w[inter_tier(bl) + lane]) : 0;
    for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d);
    if (counts && lane == 0) counts[(int64_t)b * K + s] = c;
    if (c > best) {                                      // (uniform over the wave)
      best = c; best_slot = s; best_disp = p;
      for (int t = lane; t < INTER_PYR; t += 64) keep[t] = w[t];
    }
    __syncthreads();
  }
  const unsigned long long* out = encoder ? keep : w;
  for (int t = lane; t < INTER_PYR; t += 64) pyr[(int64_t)b * INTER_PYR + t] = out[t];
  if (encoder && lane == 0) { sel[b] = best_slot; disp[b] = best_disp; }
}

// ---- host entry point ---------------------------------------------------------------------------------------------------
extern "C" int pcc_geom_multi_block_bits(const int64_t* block_keys, int64_t n_blocks, int32_t block_log2, int32_t n_slots,
                                         const int64_t* const* ref_keys, const int64_t* n_ref, const uint64_t* const* ref_bits,
                                         const int32_t* const* ref_rank, const int32_t* const* h_ref, int32_t ox, int32_t oy, int32_t oz,
                                         const int32_t* vecs, int32_t search, const uint64_t* cur_pyramid, int32_t* sel, int32_t* disp,
                                         uint64_t* pyramid, int32_t* counts, int32_t* d_bad, void* stream) {
  PCC_REQUIRE(block_keys && vecs && sel && pyramid && d_bad && n_blocks > 0 && n_blocks < (1ll << 24), "pcc_geom_multi_block_bits: bad arguments");
  PCC_REQUIRE(block_log2 >= 0 && block_log2 <= 4, "pcc_geom_multi_block_bits: block_log2 %d outside 0..4", block_log2);
  PCC_REQUIRE(n_slots >= 1 && n_slots <= MULTI_MAX_SLOTS && ref_keys && n_ref && ref_bits && ref_rank && h_ref,
              "pcc_geom_multi_block_bits: 1..%d reference slots and their five arrays are required", MULTI_MAX_SLOTS);
  PCC_REQUIRE(search >= 1 && search <= 7, "pcc_geom_multi_block_bits: search range %d outside 1..7", search);
  PCC_REQUIRE(inter_origin_ok(ox, oy, oz), "pcc_geom_multi_block_bits: origin outside the 16-bit key range");
  PCC_REQUIRE(cur_pyramid ? disp != nullptr : counts == nullptr,
              "pcc_geom_multi_block_bits: the encoder form (cur_pyramid) writes disp, the decoder form has no counts");
  MultiRefs refs;
  memset(&refs, 0, sizeof(refs));
  for (int s = 0; s < n_slots; ++s) {
    PCC_REQUIRE(n_ref[s] >= 0 && n_ref[s] < (1ll << 31) && (n_ref[s] == 0 || ref_keys[s]), "pcc_geom_multi_block_bits: bad reference set in slot %d", s);
    PCC_TRY(pcc_grid_from_host(n_ref[s] ? ref_bits[s] : nullptr, ref_rank[s], h_ref[s], "pcc_geom_multi_block_bits", &refs.g[s]));
    PCC_REQUIRE(!refs.g[s].bits || h_ref[s][6] == 1, "pcc_geom_multi_block_bits: the grid of slot %d must have pitch 1", s);
    refs.keys[s] = ref_keys[s];
    refs.n[s] = (int)n_ref[s];
  }
  k_multi_block_bits<<<(unsigned)n_blocks, 64, 0, (hipStream_t)stream>>>(block_keys, (int)n_blocks, block_log2, refs, n_slots, ox, oy, oz, vecs,
                                                                        search, (const unsigned long long*)cur_pyramid, sel, disp,
                                                                        (unsigned long long*)pyramid, counts, d_bad);
  PCC_LAUNCH_CHECK();
  return PCC_OK;
}
