// sdf_bits_layers_kernels.hip -- the hot kernel of the bit-parallel signed-distance-field build (overview: sdf_bits_kernels.hip), gfx950:
// k_sdfbit_layers runs up to eight layers on the regions that k_sdfbit_list found active; launch_sdfbit_layers launches the pair.
#include "sdf_device.hpp"

namespace clvr {

// A barrier of k_sdfbit_layers: LDS only.  __syncthreads() also waits for the wave's outstanding GLOBAL stores and atomics (a release fence
// at workgroup scope) -- here the write-back of a region (bit rows, plane ORs, state bytes), which nobody reads before the next launch; with
// it, the first barrier of a block's NEXT region stalled until those partial-line stores had been acknowledged.  LDS operations are
// still complete (lgkmcnt(0)) before the wave arrives, and the compiler may not move memory operations across it.
__device__ __forceinline__ void sdfbit_lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// lane i <- lane i - 1 / lane i + 1 of the wave (0 beyond the ends): the neighbouring rows along y
__device__ __forceinline__ uint32_t sdfbit_lane_prev(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xF, 0xF, true); }
__device__ __forceinline__ uint32_t sdfbit_lane_next(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130, 0xF, 0xF, true); }

// the blocks that can change in the next launch: a front inside, complete since the last launch (the other buffer is still to be
// brought up to date), or empty and woken for this launch by a neighbour (sdfbit_wake_neighbours).
// (The first version woke an empty block as soon as a neighbour held ANY reached voxel, up to 16 launches before the front
// arrived; the second read the 27 neighbours' states and boxes here: 11 us per launch of dependent loads.)
__device__ __forceinline__ void sdfbit_build_list(const SdfBitArgs &a, uint32_t *count, int first, int stride) {
  const int n_blocks = a.BX * a.BY * a.BZ;
  const int rounds = (n_blocks + stride - 1) / stride;  // every wave runs the same number of rounds (ballots below)
  const uint8_t stamp = (uint8_t)(a.launch + 1);
  for (int r = 0; r < rounds; ++r) {
    const int b = first + r * stride;
    bool active = false, complete = false;
    if (b < n_blocks) {
      const int st = a.state[b];
      const uint8_t wk = a.wake[b];
      active = st == 1 || st == 2 || (st == 0 && wk == stamp);
      complete = st == 2;
    }
    const unsigned long long m = __ballot(active);
    if (m == 0ull) continue;
    uint32_t base = 0u;
    if ((threadIdx.x & 63u) == 0u) base = atomicAdd(count, (uint32_t)__popcll(m));
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    if (active)
      a.list[base + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u))] = (uint32_t)b | (complete ? 0x80000000u : 0u);
  }
}

// (one launch per list: letting the last block of the layers kernel make the next list was tried -- a single block needs 30 us
// for the dependent state / bounding-box reads that 2816 threads spread over the chip finish in 5)
__global__ __launch_bounds__(256) void k_sdfbit_list(const SdfBitArgs a) {
  sdfbit_build_list(a, a.list_count, (int)(blockIdx.x * 256u + threadIdx.x), (int)(gridDim.x * 256u));
}

// Eight layers on a 128 x 64 x (4 waves) voxel region of the reached set.  A lane owns four consecutive z-rows (four words
// each: 32 halo bits, the block's 64 core bits, 32 halo bits) at one y; the rows y - 1 / y + 1 are the neighbouring LANES
// (two DPP moves per word, no memory), the rows z - 1 / z + 1 the lane's own registers -- only a strip's first and last
// row cross to the neighbouring wave through LDS (one barrier per layer, ping-pong buffers).  The first version kept the
// whole region in LDS and read four neighbour rows per row and layer.  INTERIOR: the region touches no face of the volume
// (no clamped neighbour, no missing row or bit): about half the instructions.
struct SdfBitLane {
  uint32_t cur[kBitRows][4];
  // newly reached bits of the core words (1, 2) and the layer they appeared in, bit-sliced
  uint32_t rec_any[kBitRows][2], rec_b0[kBitRows][2], rec_b1[kBitRows][2], rec_b2[kBitRows][2];
  uint32_t step_mask;
};

// REC_LDS: the bit-sliced layer records (32 registers of a lane) live in LDS instead -- `rec` points at this lane's first word, the words of
// (plane, row, word) lie kRecStride apart -- and the exchange rows are single-buffered (a second barrier per layer): 41 KB of LDS and 80
// VGPRs, three blocks per CU instead of two.
template <int NW>
constexpr int kSdfBitRecStride = (NW - 2 * kBitHalo / kBitRows) * kBitCoreY;  // core strips x core rows: words between consecutive (plane, row, word)
template <int NW, bool INTERIOR, bool REC_LDS>
__device__ __forceinline__ void sdfbit_steps(SdfBitLane &L, uint4 (*s_x)[NW][2][64], uint32_t *rec, int steps, int strip, unsigned lane, bool core_lane, bool core_strip,
                                             const uint32_t (&valid)[4], const uint32_t (&clampfix)[4], bool y_in, bool y_border, int zfirst, int Z) {
  constexpr int kRegZ = kBitRows * NW;
  constexpr int kRecStride = kSdfBitRecStride<NW>;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (k >= steps) break;
    // after k layers a row is exact if it lies at least k rows inside the region: layer k + 1 is computed for the rows
    // [k + 1, region - 2 - k] from the y-neighbour unions V of the rows [k, region - 1 - k] (the other rows' V is
    // computed too -- branch-free -- and only ever read by rows that are not needed either)
    uint32_t v[kBitRows][4];
#pragma unroll
    for (int i = 0; i < kBitRows; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[i][j] = sdfbit_lane_prev(L.cur[i][j]) | sdfbit_lane_next(L.cur[i][j]);
        if (!INTERIOR) v[i][j] |= y_border ? L.cur[i][j] : 0u;
      }
    uint4 *xbuf = &s_x[REC_LDS ? 0 : (k & 1)][0][0][0];
    xbuf[(strip * 2 + 0) * 64 + lane] = uint4{v[0][0], v[0][1], v[0][2], v[0][3]};
    xbuf[(strip * 2 + 1) * 64 + lane] = uint4{v[kBitRows - 1][0], v[kBitRows - 1][1], v[kBitRows - 1][2], v[kBitRows - 1][3]};
    sdfbit_lds_barrier();
    uint4 below = uint4{0u, 0u, 0u, 0u}, above = uint4{0u, 0u, 0u, 0u};
    if (strip > 0) below = xbuf[((strip - 1) * 2 + 1) * 64 + lane];
    if (strip < NW - 1) above = xbuf[((strip + 1) * 2 + 0) * 64 + lane];
    if (REC_LDS) sdfbit_lds_barrier();  // one buffer: everybody has read its neighbours' rows before the next layer overwrites them
#pragma unroll
    for (int i = 0; i < kBitRows; ++i) {
      const int rz = kBitRows * strip + i, gz = zfirst + i;
      bool need = rz >= k + 1 && rz <= kRegZ - 2 - k;  // wave-uniform
      if (!INTERIOR) need = need && gz >= 0 && gz < Z;
      if (!need) continue;
      const bool z_border = !INTERIOR && (gz == 0 || gz == Z - 1);
      uint32_t u[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t lo = i > 0 ? v[i - 1][j] : (j == 0 ? below.x : j == 1 ? below.y : j == 2 ? below.z : below.w);
        const uint32_t hi = i < kBitRows - 1 ? v[i + 1][j] : (j == 0 ? above.x : j == 1 ? above.y : j == 2 ? above.z : above.w);
        u[j] = lo | hi;
        if (!INTERIOR) u[j] |= z_border ? v[i][j] : 0u;
      }
      uint32_t nxt[4];
      if (INTERIOR) {
        nxt[0] = L.cur[i][0] | sdfbit_x_neighbours(0u, u[0], u[1], 0u);
        nxt[1] = L.cur[i][1] | sdfbit_x_neighbours(u[0], u[1], u[2], 0u);
        nxt[2] = L.cur[i][2] | sdfbit_x_neighbours(u[1], u[2], u[3], 0u);
        nxt[3] = L.cur[i][3] | sdfbit_x_neighbours(u[2], u[3], 0u, 0u);
      } else {
        nxt[0] = L.cur[i][0] | (sdfbit_x_neighbours(0u, u[0], u[1], clampfix[0]) & valid[0]);
        nxt[1] = L.cur[i][1] | (sdfbit_x_neighbours(u[0], u[1], u[2], clampfix[1]) & valid[1]);
        nxt[2] = L.cur[i][2] | (sdfbit_x_neighbours(u[1], u[2], u[3], clampfix[2]) & valid[2]);
        nxt[3] = L.cur[i][3] | (sdfbit_x_neighbours(u[2], u[3], 0u, clampfix[3]) & valid[3]);
        if (!y_in) nxt[0] = nxt[1] = nxt[2] = nxt[3] = 0u;  // rows beyond the volume do not exist
      }
      if (core_strip) {
        const uint32_t nb0 = core_lane ? (nxt[1] & ~L.cur[i][1]) : 0u, nb1 = core_lane ? (nxt[2] & ~L.cur[i][2]) : 0u;
        if (REC_LDS) {
          // ds_or without return; plane p of (row i, word j) at rec[((p * kBitRows + i) * 2 + j) * kRecStride]; plane 0 = "reached in this launch"
          if (nb0) { atomicOr(rec + ((0 * kBitRows + i) * 2 + 0) * kRecStride, nb0);
                     if (k & 1) atomicOr(rec + ((1 * kBitRows + i) * 2 + 0) * kRecStride, nb0);
                     if (k & 2) atomicOr(rec + ((2 * kBitRows + i) * 2 + 0) * kRecStride, nb0);
                     if (k & 4) atomicOr(rec + ((3 * kBitRows + i) * 2 + 0) * kRecStride, nb0); }
          if (nb1) { atomicOr(rec + ((0 * kBitRows + i) * 2 + 1) * kRecStride, nb1);
                     if (k & 1) atomicOr(rec + ((1 * kBitRows + i) * 2 + 1) * kRecStride, nb1);
                     if (k & 2) atomicOr(rec + ((2 * kBitRows + i) * 2 + 1) * kRecStride, nb1);
                     if (k & 4) atomicOr(rec + ((3 * kBitRows + i) * 2 + 1) * kRecStride, nb1); }
        } else {
          L.rec_any[i][0] |= nb0; L.rec_any[i][1] |= nb1;
          if (k & 1) { L.rec_b0[i][0] |= nb0; L.rec_b0[i][1] |= nb1; }
          if (k & 2) { L.rec_b1[i][0] |= nb0; L.rec_b1[i][1] |= nb1; }
          if (k & 4) { L.rec_b2[i][0] |= nb0; L.rec_b2[i][1] |= nb1; }
        }
        if (nb0 | nb1) L.step_mask |= 1u << k;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) L.cur[i][j] = nxt[j];
    }
  }
}

// The grid is persistent: its blocks take the active regions from the list k_sdfbit_list made (a launch over ALL regions
// spent 30 us on the inactive ones alone); a block's first region is list[blockIdx.x], the following ones come from a queue.
template <int NW, bool REC_LDS>
__global__ __launch_bounds__(64 * NW, REC_LDS ? 6 : 4) void k_sdfbit_layers(const SdfBitArgs a) {
  constexpr int kRegZ = kBitRows * NW, kCoreZ = kRegZ - 2 * kBitHalo;
  __shared__ uint4 s_x[REC_LDS ? 1 : 2][NW][2][64];
  constexpr int kRecStride = kSdfBitRecStride<NW>;
  __shared__ uint32_t s_rec[REC_LDS ? 4 * kBitRows * 2 * kRecStride : 1];
  if (REC_LDS)
    for (int i = (int)threadIdx.x; i < 4 * kBitRows * 2 * kRecStride; i += 64 * NW) s_rec[i] = 0u;  // (a region leaves them cleared)
  __shared__ uint32_t s_all, s_any, s_steps, s_entry, s_orx[2];
  __shared__ int s_box[4];  // min y, max y, min z, max z of the core's reached voxels
  const unsigned tid = threadIdx.x, lane = tid & 63u;
  const int strip = __builtin_amdgcn_readfirstlane((int)(tid >> 6));  // wave-uniform: scalar branches on the row ranges below
  const uint32_t n_active = *a.list_count;
  const bool core_lane = lane >= (unsigned)kBitHalo && lane < (unsigned)(kBitHalo + kBitCoreY);
  const bool core_strip = strip >= kBitHalo / kBitRows && strip < NW - kBitHalo / kBitRows;
  for (uint32_t round = 0u;; ++round) {
    sdfbit_lds_barrier();  // the previous region's flags and exchange rows are no longer read
    if (tid == 0u) {
      // dynamic: regions differ in cost (complete ones only copy); a static round-robin over the list measured 1.84 ms against 1.60.
      // (Fetching the NEXT region's ticket and list entry while the block works on the current one -- two dependent round trips off
      // every visit -- was measured at 1.41 ms against 1.33: two more live registers in a kernel that already spills.)
      s_entry = round == 0u ? blockIdx.x : gridDim.x + atomicAdd(a.list_head, 1u);
      s_all = 1u; s_any = 0u; s_steps = 0u; s_orx[0] = 0u; s_orx[1] = 0u;
      s_box[0] = 255; s_box[1] = -1; s_box[2] = 255; s_box[3] = -1;
    }
    sdfbit_lds_barrier();
    SdfBitProbe probe(tid);
    const uint32_t entry = s_entry;
    if (entry >= n_active) return;
    const uint32_t item = a.list[entry];  // block | complete-since-the-previous-launch << 31
    const int b = (int)(item & 0x7FFFFFFFu);
    const int bx = b % a.BX, by = (b / a.BX) % a.BY, bz = b / (a.BX * a.BY);
    uint32_t valid[4], clampfix[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int gw = 2 * bx - 1 + j, x_lo = gw * 32;
      valid[j] = 0u;
      clampfix[j] = 0u;
      if (gw >= 0 && gw < a.WP && x_lo < a.X) {
        valid[j] = (a.X - x_lo >= 32) ? 0xFFFFFFFFu : ((1u << (a.X - x_lo)) - 1u);
        clampfix[j] = (gw == 0 ? 1u : 0u) | ((((a.X - 1) >> 5) == gw) ? (1u << ((a.X - 1) & 31)) : 0u);
      }
    }
    if (item >> 31) {
      // complete since the previous launch: bring the other buffer up to date, then never come back
      for (int r = (int)tid; r < kBitCoreY * kCoreZ; r += 64 * NW) {
        const int gy = by * kBitCoreY + (r % kBitCoreY), gz = bz * kCoreZ + (r / kBitCoreY);
        if (gy >= a.Y || gz >= a.Z) continue;
#pragma unroll
        for (int j = 1; j <= 2; ++j) {
          const int gw = 2 * bx - 1 + j;
          if (gw < a.WP) a.r_out[(size_t)b * (size_t)(2 * kBitCoreY * kCoreZ) + (size_t)(r * 2 + j - 1)] = valid[j];
        }
      }
      if (tid == 0u) a.state[b] = 3;
      sdfbit_wake_neighbours(a, bx, by, bz, 0, 63, 0, kBitCoreY - 1, 0, kCoreZ - 1, tid, (uint8_t)(a.launch + 2));
      continue;
    }

    const int gy = by * kBitCoreY - kBitHalo + (int)lane;
    const int zfirst = bz * kCoreZ - kBitHalo + kBitRows * strip;  // gz of this lane's row 0
    const bool y_in = gy >= 0 && gy < a.Y;
    const bool y_border = gy == 0 || gy == a.Y - 1;  // the clamped neighbour along y is the row itself (signed_distance_field.cl:72)
    // no face of the volume inside the region or next to it: every word, row and neighbour exists, nothing is clamped
    const bool interior = bx >= 1 && (2 * bx + 3) * 32 < a.X && by * kBitCoreY - kBitHalo >= 1 && by * kBitCoreY - kBitHalo + 63 <= a.Y - 2 &&
                          bz * kCoreZ - kBitHalo >= 1 && bz * kCoreZ - kBitHalo + kRegZ - 1 <= a.Z - 2;
    probe.mark(1);
    SdfBitLane L;
    // this lane's y: its tile row (by - 1 / by / by + 1) and row inside the tile
    const int lane_by = by + ((int)lane < kBitHalo ? -1 : ((int)lane >= kBitHalo + kBitCoreY ? 1 : 0));
    const int lane_cy = (int)lane < kBitHalo ? kBitCoreY - kBitHalo + (int)lane : ((int)lane >= kBitHalo + kBitCoreY ? (int)lane - kBitHalo - kBitCoreY : (int)lane - kBitHalo);
    const bool y_tile = lane_by >= 0 && lane_by < a.BY;
    constexpr size_t kTileWords = (size_t)2 * kBitCoreY * kCoreZ;
#pragma unroll
    for (int i = 0; i < kBitRows; ++i) {
      const int rz = kBitRows * strip + i;
      const int row_bz = bz + (rz < kBitHalo ? -1 : (rz >= kBitHalo + kCoreZ ? 1 : 0));
      const int row_cz = rz < kBitHalo ? kCoreZ - kBitHalo + rz : (rz >= kBitHalo + kCoreZ ? rz - kBitHalo - kCoreZ : rz - kBitHalo);
      const bool row_in = y_tile && row_bz >= 0 && row_bz < a.BZ;  // the tile exists; its rows beyond the volume hold zeros
      // all loads are issued unconditionally (one round trip): a missing tile reads tile 0 and is masked afterwards
      const size_t t_mid = row_in ? (((size_t)row_bz * a.BY + lane_by) * a.BX + bx) : (size_t)0;
      const size_t in_tile = (size_t)((row_cz * kBitCoreY + lane_cy) * 2);
      const uint32_t *mid = a.r_in + t_mid * kTileWords + in_tile;
      const bool left_in = row_in && bx > 0, right_in = row_in && bx + 1 < a.BX;
      const uint32_t w0 = (left_in ? mid - kTileWords : a.r_in)[1], w3 = (right_in ? mid + kTileWords : a.r_in)[0];
      const uint2 w12 = *reinterpret_cast<const uint2 *>(mid);
      L.cur[i][0] = left_in ? w0 : 0u;
      L.cur[i][1] = row_in ? w12.x : 0u;
      L.cur[i][2] = row_in ? w12.y : 0u;
      L.cur[i][3] = right_in ? w3 : 0u;
#pragma unroll
      for (int j = 0; j < 2; ++j)
        if (!REC_LDS) L.rec_any[i][j] = L.rec_b0[i][j] = L.rec_b1[i][j] = L.rec_b2[i][j] = 0u;
    }
    L.step_mask = 0u;
    probe.mark_after_wait(2);
    // this lane's first record word (core lanes of core strips only; the others never touch the records)
    uint32_t *rec = s_rec + (core_strip && core_lane ? (strip - kBitHalo / kBitRows) * kBitCoreY + ((int)lane - kBitHalo) : 0);
    if (interior)
      sdfbit_steps<NW, true, REC_LDS>(L, s_x, rec, a.steps, strip, lane, core_lane, core_strip, valid, clampfix, y_in, y_border, zfirst, a.Z);
    else
      sdfbit_steps<NW, false, REC_LDS>(L, s_x, rec, a.steps, strip, lane, core_lane, core_strip, valid, clampfix, y_in, y_border, zfirst, a.Z);
    probe.mark(3);
    // core rows back to the other bit buffer; the block's state and the box around its reached voxels (whom to wake) for the next launch
    bool any = false, all = true;
    if (core_strip && core_lane && y_in) {
#pragma unroll
      for (int i = 0; i < kBitRows; ++i) {
        const int gz = zfirst + i;
        if (gz < 0 || gz >= a.Z) continue;
        const int cz = kBitRows * strip + i - kBitHalo;
        *reinterpret_cast<uint2 *>(a.r_out + (size_t)b * kTileWords + (size_t)((cz * kBitCoreY + ((int)lane - kBitHalo)) * 2)) = uint2{L.cur[i][1], L.cur[i][2]};
        any |= (L.cur[i][1] | L.cur[i][2]) != 0u;
        all &= L.cur[i][1] == valid[1] && L.cur[i][2] == valid[2];  // a word beyond the volume: 0 == 0
        if (L.cur[i][1] | L.cur[i][2]) {  // words beyond the volume are zero (valid mask)
          atomicMin(&s_box[2], cz);
          atomicMax(&s_box[3], cz);
        }
      }
    }
    if (any) {
      s_any = 1u;
      uint32_t o1 = 0u, o2 = 0u;
#pragma unroll
      for (int i = 0; i < kBitRows; ++i) { o1 |= L.cur[i][1]; o2 |= L.cur[i][2]; }  // rows outside the volume hold zeros
      if (o1) atomicOr(&s_orx[0], o1);
      if (o2) atomicOr(&s_orx[1], o2);
      atomicMin(&s_box[0], (int)lane - kBitHalo);
      atomicMax(&s_box[1], (int)lane - kBitHalo);
    }
    if (!all) s_all = 0u;
    if (L.step_mask) atomicOr(&s_steps, L.step_mask);

    // values: NOT written here.  Round 2 let every lane rewrite the 64 bytes of its rows that gained voxels -- a load and a store of
    // 16 bytes per lane at a 512-byte stride, partial lines whose completion the next barrier waited for: two thirds of a region's
    // time.  Now the layer in which a voxel was reached goes into seven bit planes (tiled like the reached sets: a wave's rows are
    // contiguous) with fire-and-forget atomic ORs -- a voxel is reached exactly once, so the launches never write the same bit -- and
    // k_sdfbit_expand turns planes + final reached set + event bits into bytes ONCE, after the last launch, with full-line stores.
    // layer index = r0 + k + 1 (1..127; r0 = 8 x launch, k the layer inside the launch as recorded bit-sliced in rec_b0..2)
    if (core_strip && core_lane && y_in) {
      const uint32_t hi_lo = (uint32_t)a.r0 >> 3, hi_carry = hi_lo + 1u;  // bits 3.. of the index while k + 1 < 8 / when k + 1 == 8
      // (a plane holds at most 2^28 words: 32-bit word offsets from the plane's own, wave-uniform base keep the addresses out of the VGPRs)
      const uint32_t lane_word = (uint32_t)b * (uint32_t)kTileWords + (uint32_t)(((kBitRows * strip - kBitHalo) * kBitCoreY + ((int)lane - kBitHalo)) * 2);
#pragma unroll
      for (int i = 0; i < kBitRows; ++i) {
        // the row's two core words are one aligned 8-byte pair in every plane: one 64-bit OR per plane and row
        uint32_t r_any[2], r_b0[2], r_b1[2], r_b2[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if (REC_LDS) {
            r_any[j] = rec[((0 * kBitRows + i) * 2 + j) * kRecStride];
            r_b0[j] = r_b1[j] = r_b2[j] = 0u;
          } else {
            r_any[j] = L.rec_any[i][j]; r_b0[j] = L.rec_b0[i][j]; r_b1[j] = L.rec_b1[i][j]; r_b2[j] = L.rec_b2[i][j];
          }
        }
        if ((r_any[0] | r_any[1]) == 0u) continue;  // (then the row also lies inside the volume)
        if (REC_LDS) {
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            r_b0[j] = rec[((1 * kBitRows + i) * 2 + j) * kRecStride];
            r_b1[j] = rec[((2 * kBitRows + i) * 2 + j) * kRecStride];
            r_b2[j] = rec[((3 * kBitRows + i) * 2 + j) * kRecStride];
#pragma unroll
            for (int p = 0; p < 4; ++p) rec[((p * kBitRows + i) * 2 + j) * kRecStride] = 0u;  // cleared for the block's next region
          }
        }
        uint32_t v[7][2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const uint32_t any = r_any[j], b0 = r_b0[j], b1 = r_b1[j], b2 = r_b2[j];
          const uint32_t m7 = b0 & b1 & b2, m = any & ~m7;  // k == 7: the index's low three bits are 0 and bit 3.. carries
          v[0][j] = ~b0 & m; v[1][j] = (b1 ^ b0) & m; v[2][j] = (b2 ^ (b1 & b0)) & m;  // k + 1, bit-sliced
#pragma unroll
          for (int p = 0; p < 4; ++p) v[3 + p][j] = (((hi_lo >> p) & 1u) ? m : 0u) | (((hi_carry >> p) & 1u) ? m7 : 0u);
        }
        const uint32_t w = lane_word + (uint32_t)(i * kBitCoreY * 2);
#pragma unroll
        for (int p = 0; p < 7; ++p)
          if (v[p][0] | v[p][1])
            atomicOr(reinterpret_cast<unsigned long long *>(a.planes + (size_t)p * a.plane_words + w), (unsigned long long)v[p][0] | ((unsigned long long)v[p][1] << 32));
      }
    }
    probe.mark_after_wait(4);
    sdfbit_lds_barrier();
    probe.flush(a, interior);
    if (s_any) {
      const unsigned long long orx64 = (unsigned long long)s_orx[0] | ((unsigned long long)s_orx[1] << 32);
      sdfbit_wake_neighbours(a, bx, by, bz, __ffsll((long long)orx64) - 1, 63 - __clzll((long long)orx64), s_box[0], s_box[1], s_box[2], s_box[3], tid,
                             (uint8_t)(a.launch + 2));  // for the next launch
    }
    if (tid == 0u) {
      a.state[b] = s_all ? 2 : (s_any ? 1 : 0);
      for (uint32_t m = s_steps; m; m &= m - 1u) a.presence[a.r0 + __ffs((int)m)] = 1;  // layer r0 + k + 1 settled something
    }
  }
}

// one launch = the list of the regions that can change + up to eight layers on them (persistent grid of `grid_blocks`)
hipError_t launch_sdfbit_layers(const SdfBitArgs &a, int waves, unsigned grid_blocks, bool rec_in_lds, hipStream_t s) {
  const unsigned n_blocks = (unsigned)(a.BX * a.BY * a.BZ);
  hipLaunchKernelGGL(k_sdfbit_list, dim3(std::min((n_blocks + 255u) / 256u, 1024u)), dim3(256), 0, s, a);
  const unsigned grid = std::min(n_blocks, grid_blocks);
  if (waves == 16)
    hipLaunchKernelGGL((k_sdfbit_layers<16, false>), dim3(grid), dim3(64 * 16), 0, s, a);
  else if (rec_in_lds)
    hipLaunchKernelGGL((k_sdfbit_layers<8, true>), dim3(grid), dim3(64 * 8), 0, s, a);
  else
    hipLaunchKernelGGL((k_sdfbit_layers<8, false>), dim3(grid), dim3(64 * 8), 0, s, a);
  return hipGetLastError();
}

}  // namespace clvr
