// thin_kernels.hip -- topology-preserving thinning (clwh_mask_thin) and the list of a mask's voxels (clwh_mask_points), gfx950.  The
// definition is in include/clwh.h: per iteration the candidates C = border \ ends \ anchors are fixed on the mask as it stands, then
// eight sub-passes, one per parity s = (x & 1) | (y & 1) << 1 | (z & 1) << 2, each delete the candidates of that parity that are still
// set and simple.  Mask layout and tiles are grow's (grow_kernels.hip): a tile = 64 x 16 x 16 voxels = one 64-bit word of 256 rows, a
// 256-thread block owns the tile it works on.
//   k_thin_candidates, once per iteration, a thread per 64-bit word: B and E are shifts and bit-sliced counts of the word's nine rows;
//   it stores C and appends every tile that holds a candidate to the list, once (the tile's stamp is the iteration that listed it).
//   k_thin_subpass, eight times per iteration: a block per listed tile loads the tile's 18 x 18 rows (the word, and the two bits beside
//   it along x) into LDS, compacts its candidates of parity s into a table, gives a lane a candidate, gathers the candidate's 3 x 3 x 3
//   block from LDS and tests it in registers; the verdicts are collected per row in LDS and the owner of a row stores it once.
// What has to hold, and why.
//   In place.  A sub-pass reads M and clears bits of M in the same buffer.  Every voxel it deletes has parity s.  The 26 neighbours of
//   a voxel differ from it by 1 in some coordinate, so none of them has its parity: the bits a test looks at are not the bits the
//   sub-pass clears, and the test of p gives the same verdict on M before, during and after the sub-pass' deletions.  "All at once"
//   and "in any order" are therefore the same set.
//   Owner stores.  Only the block that works a tile stores that tile's words (a tile is listed once per iteration: the stamp), and
//   inside the block only a row's thread stores the row; the verdicts reach it through LDS.
//   Halo.  A block reads its neighbours' words while their owners may be clearing parity-s bits in them.  Of such a word it uses only
//   bits of other parities (above), which nobody changes in this sub-pass: the old word, the new word or a torn mix give the same
//   answer.  The next sub-pass starts behind a kernel boundary.
//   Gather.  A candidate at row (ry, rz), bit b of a tile reads rows ry - 1 .. ry + 1, rz - 1 .. rz + 1 of the 18 x 18 region, which
//   covers up to four tiles in y and z, and bits b - 1 .. b + 1, where bit -1 is bit 63 of the word to the left and bit 64 is bit 0
//   of the word to the right (both kept beside the word): up to eight tiles in all.  Rows and words outside the volume are empty, and
//   so are the bits at x >= X (k_thin_begin clears them, thin_row masks them): outside is background.
//   Bounded loops.  The component fill makes at most 26 expansions of at most 26 elements; a row holds at most 32 candidates of one x
//   parity, a tile at most 64 rows x 32 = 2048 of them = 8 per lane; a block takes at most ceil(tiles / blocks) tiles.
//   Nothing depends on the order of blocks or lanes: the list's order and the table's order are the scheduler's, the stored set is not.
#include <rocprim/device/device_scan.hpp>

#include "mask_device.hpp"

namespace clvr {

namespace {

typedef unsigned long long u64;
constexpr int kTile = 16;  // rows of a tile along y and along z

// ---- the 3 x 3 x 3 block as a word: offset (dx, dy, dz) at bit (dx + 1) + 3 (dy + 1) + 9 (dz + 1); bit 13 is the centre and stays
// clear, so the word holds the 26 neighbours.  Adjacency is shifts under masks; the two adjacency tables of the definition are
// generated below at compile time and pin the shifts.
constexpr uint32_t kAll27 = 0x7FFFFFFu, kCentre = 1u << 13;
constexpr uint32_t kX0 = 0x1249249u, kX2 = kX0 << 2;  // the positions with dx = -1, with dx = +1
constexpr uint32_t kY0 = 0x01C0E07u, kY2 = kY0 << 6;  // dy = -1, dy = +1

constexpr uint32_t thin_dilate26(uint32_t g) {  // g with everything 26-adjacent to it: the box, separable
  g = (g | ((g << 1) & ~kX0) | ((g >> 1) & ~kX2)) & kAll27;  // (a bit shifted out of the block must not come back)
  g = (g | ((g << 3) & ~kY0) | ((g >> 3) & ~kY2)) & kAll27;
  return (g | (g << 9) | (g >> 9)) & kAll27;
}
constexpr uint32_t thin_dilate6(uint32_t g) {  // g with everything 6-adjacent to it
  return (g | ((g << 1) & ~kX0) | ((g >> 1) & ~kX2) | ((g << 3) & ~kY0) | ((g >> 3) & ~kY2) | (g << 9) | (g >> 9)) & kAll27;
}

constexpr int thin_abs(int v) { return v < 0 ? -v : v; }
// the positions whose offset has an L1 norm in [lo, hi]
constexpr uint32_t thin_positions(int lo, int hi) {
  uint32_t m = 0u;
  for (int i = 0; i < 27; ++i) {
    const int n = thin_abs(i % 3 - 1) + thin_abs(i / 3 % 3 - 1) + thin_abs(i / 9 - 1);
    if (n >= lo && n <= hi) m |= 1u << i;
  }
  return m;
}
constexpr uint32_t kN6 = thin_positions(1, 1), kN18 = thin_positions(1, 2);
// row i of the definition's tables: the positions adjacent to position i, by the largest (26) or the summed (6) coordinate difference
constexpr uint32_t thin_adjacent(int i, bool faces_only) {
  uint32_t m = 0u;
  for (int j = 0; j < 27; ++j) {
    const int dx = thin_abs(i % 3 - j % 3), dy = thin_abs(i / 3 % 3 - j / 3 % 3), dz = thin_abs(i / 9 - j / 9);
    const bool adjacent = faces_only ? dx + dy + dz == 1 : (i != j && dx <= 1 && dy <= 1 && dz <= 1);
    if (adjacent) m |= 1u << j;
  }
  return m;
}
constexpr bool thin_shifts_are_the_tables() {
  for (int i = 0; i < 27; ++i) {
    if (thin_dilate26(1u << i) != (thin_adjacent(i, false) | (1u << i))) return false;
    if (thin_dilate6(1u << i) != (thin_adjacent(i, true) | (1u << i))) return false;
  }
  return true;
}
static_assert(thin_shifts_are_the_tables(), "the shifts are the adjacency tables of the definition");
static_assert(kN6 == 0x0415410u && kN18 == (kAll27 & ~kCentre & ~0x5140145u), "faces; everything but the centre and the corners");

// Is the centre simple?  n: its 26 neighbours.  (a) they are one 26-component; (b) the clear face neighbours exist and lie in one
// 6-component of the clear part of the 18-neighbourhood.  Both fills grow the lowest set bit and stop when nothing is added.
__device__ __forceinline__ bool thin_simple(uint32_t n) {
  if (n == 0u) return false;
  uint32_t g = n & (0u - n);
#pragma unroll 1
  for (int k = 0; k < 26; ++k) {
    const uint32_t next = thin_dilate26(g) & n;
    if (next == g) break;
    g = next;
  }
  if (g != n) return false;
  const uint32_t clear = ~n & kN18, faces = clear & kN6;
  if (faces == 0u) return false;
  g = faces & (0u - faces);
#pragma unroll 1
  for (int k = 0; k < 18; ++k) {
    const uint32_t next = thin_dilate6(g) & clear;
    if (next == g) break;
    g = next;
  }
  return (g & kN6) == faces;
}

// the bits of word wx of a row that are voxels
__device__ __forceinline__ u64 thin_valid(int X, int wx) { return (wx + 1) * 64 <= X ? ~0ull : (1ull << (X - wx * 64)) - 1ull; }

struct ThinRow {
  u64 c;     // the row's word
  u64 l, r;  // at every bit the voxel's neighbour at x - 1, at x + 1
};
// word wx of row (y, z); rows outside the volume and bits at x >= X are empty
__device__ __forceinline__ ThinRow thin_row(const u64 *mask, int X, int Y, int Z, int W64, int wx, int y, int z) {
  ThinRow q{0ull, 0ull, 0ull};
  if (y < 0 || y >= Y || z < 0 || z >= Z) return q;
  const u64 *row = mask + ((size_t)z * (size_t)Y + (size_t)y) * (size_t)W64;
  q.c = row[wx] & thin_valid(X, wx);
  q.l = q.c << 1;
  q.r = q.c >> 1;
  if (wx > 0) q.l |= row[wx - 1] >> 63;
  if (wx + 1 < W64) q.r |= (row[wx + 1] & thin_valid(X, wx + 1)) << 63;
  return q;
}

__device__ __forceinline__ uint32_t *thin_listed(const ThinArgs &a, int slot) { return a.counters + 2 + 2 * slot; }
__device__ __forceinline__ uint32_t *thin_deleted(const ThinArgs &a, int slot) { return a.counters + 3 + 2 * slot; }

}  // namespace

// M = mask_in without its padding, and count_in.  In place a lane reads its word before it writes it and nobody else's.
__global__ __launch_bounds__(256) void k_thin_begin(const ThinArgs a, const u64 *mask_in) {
  const size_t total = (size_t)a.W64 * (size_t)a.Y * (size_t)a.Z, id = (size_t)blockIdx.x * 256u + threadIdx.x;
  u64 v = 0ull;
  if (id < total) {
    v = mask_in[id] & thin_valid(a.X, (int)(id % (size_t)a.W64));
    a.mask[id] = v;
  }
  u64 count = (u64)__popcll(v);
  for (int off = 32; off > 0; off >>= 1) count += __shfl_xor(count, off);
  if ((threadIdx.x & 63u) == 0u && count != 0ull) atomicAdd(reinterpret_cast<u64 *>(a.counters), count);
}

// C of this iteration, and the tiles that hold a candidate.  An iteration behind one that deleted nothing has nothing to do.
__global__ __launch_bounds__(256) void k_thin_candidates(const ThinArgs a, uint32_t iteration, int slot) {
  if (slot > 0 && *thin_deleted(a, slot - 1) == 0u) return;
  const size_t total = (size_t)a.W64 * (size_t)a.Y * (size_t)a.Z, id = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (id >= total) return;
  if (id == 0u && a.dense) *thin_listed(a, slot) = (uint32_t)(a.TX * a.TY * a.TZ);
  const size_t row = id / (size_t)a.W64;
  const int wx = (int)(id - row * (size_t)a.W64), z = (int)(row / (size_t)a.Y), y = (int)(row - (size_t)z * (size_t)a.Y);
  // ones / twos: the positions with at least one / at least two set neighbours among the 26; faces: with all six face neighbours set
  u64 m = 0ull, faces = ~0ull, ones = 0ull, twos = 0ull;
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    const int dy = q % 3 - 1, dz = q / 3 - 1;
    const ThinRow n = thin_row(a.mask, a.X, a.Y, a.Z, a.W64, wx, y + dy, z + dz);
    twos |= ones & n.l;
    ones |= n.l;
    twos |= ones & n.r;
    ones |= n.r;
    if (dy == 0 && dz == 0) {
      m = n.c;
      faces &= n.l & n.r;
    } else {
      twos |= ones & n.c;
      ones |= n.c;
      if (dy == 0 || dz == 0) faces &= n.c;
    }
  }
  u64 c = m & ~faces;
  if (a.keep_ends) c &= ~(ones & ~twos);
  if (a.anchors) c &= ~a.anchors[id];
  a.cand[id] = c;
  if (c != 0ull && !a.dense) {
    const uint32_t tile = (uint32_t)(((z >> 4) * a.TY + (y >> 4)) * a.TX + wx);
    if (a.stamps[tile] != iteration && atomicExch(&a.stamps[tile], iteration) != iteration) a.list[atomicAdd(thin_listed(a, slot), 1u)] = tile;
  }
}

// Sub-pass s of an iteration over the listed tiles; see the head of the file.
__global__ __launch_bounds__(256) void k_thin_subpass(const ThinArgs a, int slot, int s) {
  __shared__ u64 rows[kTile + 2][kTile + 2];       // [rz + 1][ry + 1]: the region's words in this tile's column
  __shared__ uint8_t beside[kTile + 2][kTile + 2];  // bit 0: bit 63 of the word to the left, bit 1: bit 0 of the word to the right
  __shared__ u64 verdict[256];                      // per core row: the bits to delete
  __shared__ uint16_t table[2048];                  // the tile's candidates of parity s: row << 6 | bit
  __shared__ uint32_t s_n, s_deleted;
  const uint32_t n = *thin_listed(a, slot);
  if (n == 0u) return;  // an iteration that is not run, or without a candidate: one word read
  const unsigned t = threadIdx.x;
  const int cy = (int)(t & 15u), cz = (int)(t >> 4);
  // (a tile starts at even x, y and z: parity in the tile is parity in the volume)
  const bool my_rows = (cy & 1) == ((s >> 1) & 1) && (cz & 1) == ((s >> 2) & 1);
  const u64 my_bits = (s & 1) ? 0xAAAAAAAAAAAAAAAAull : 0x5555555555555555ull;
  for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
    const uint32_t tile = a.dense ? i : a.list[i];
    const int tx = (int)(tile % (uint32_t)a.TX), ty = (int)((tile / (uint32_t)a.TX) % (uint32_t)a.TY), tz = (int)(tile / (uint32_t)(a.TX * a.TY));
    __syncthreads();  // the previous tile's last reads of the shared arrays
    if (t == 0u) s_n = s_deleted = 0u;
    verdict[t] = 0ull;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int r = (int)t + 256 * k;
      if (r < (kTile + 2) * (kTile + 2)) {
        const int ry = r % (kTile + 2) - 1, rz = r / (kTile + 2) - 1;
        const ThinRow q = thin_row(a.mask, a.X, a.Y, a.Z, a.W64, tx, ty * kTile + ry, tz * kTile + rz);
        rows[rz + 1][ry + 1] = q.c;
        beside[rz + 1][ry + 1] = (uint8_t)((q.l & 1ull) | ((q.r >> 63) << 1));
      }
    }
    __syncthreads();
    const int gy = ty * kTile + cy, gz = tz * kTile + cz;
    const bool mine = my_rows && gy < a.Y && gz < a.Z;
    const size_t own = ((size_t)gz * (size_t)a.Y + (size_t)gy) * (size_t)a.W64 + (size_t)tx;
    const u64 m = rows[cz + 1][cy + 1];
    u64 c = mine ? (a.cand[own] & m & my_bits) : 0ull;
    if (c != 0ull) {
      uint32_t at = atomicAdd(&s_n, (uint32_t)__popcll(c));
#pragma unroll 1
      for (int k = 0; k < 32 && c != 0ull; ++k) {
        table[at++] = (uint16_t)((t << 6) | (unsigned)(__ffsll((long long)c) - 1));
        c &= c - 1ull;
      }
    }
    __syncthreads();
    const uint32_t listed = s_n;
#pragma unroll 1
    for (int pass = 0; pass < 8; ++pass) {
      const uint32_t k = (uint32_t)pass * 256u + t;
      if (k >= listed) break;
      const unsigned e = table[k], b = e & 63u;
      const int ry = (int)((e >> 6) & 15u), rz = (int)(e >> 10);
      uint32_t nb = 0u;
#pragma unroll
      for (int q = 0; q < 9; ++q) {
        const u64 w = rows[rz + q / 3][ry + q % 3];
        const uint32_t h = beside[rz + q / 3][ry + q % 3];
        const uint32_t three = b == 0u ? ((uint32_t)(w & 3ull) << 1) | (h & 1u) : b == 63u ? (uint32_t)(w >> 62) | ((h >> 1) << 2) : (uint32_t)(w >> (b - 1u)) & 7u;
        nb |= three << (3 * q);
      }
      if (thin_simple(nb & ~kCentre)) atomicOr(&verdict[e >> 6], 1ull << b);
    }
    __syncthreads();
    const u64 gone = verdict[t];
    if (gone != 0ull) {  // (a row of mine: it exists)
      a.mask[own] = m & ~gone;
      atomicAdd(&s_deleted, (uint32_t)__popcll(gone));
    }
    __syncthreads();
    if (t == 0u && s_deleted != 0u) atomicAdd(thin_deleted(a, slot), s_deleted);
  }
}

// ---- the list of a mask's voxels: per-word counts, their scan, and a lane per word that writes its voxels in ascending x
__global__ __launch_bounds__(256) void k_points_count(const PointsArgs a) {
  const size_t total = (size_t)a.W64 * (size_t)a.Y * (size_t)a.Z, id = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (id > total) return;
  a.counts[id] = id < total ? (uint32_t)__popcll(a.mask[id] & thin_valid(a.X, (int)(id % (size_t)a.W64))) : 0u;  // (one more: its base is the total)
}

__global__ __launch_bounds__(256) void k_points_fill(const PointsArgs a) {
  const size_t total = (size_t)a.W64 * (size_t)a.Y * (size_t)a.Z, id = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (id >= total || a.counts[id] == 0u) return;
  const size_t row = id / (size_t)a.W64;
  const int wx = (int)(id - row * (size_t)a.W64), z = (int)(row / (size_t)a.Y), y = (int)(row - (size_t)z * (size_t)a.Y);
  ThinRow n[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) n[q] = thin_row(a.mask, a.X, a.Y, a.Z, a.W64, wx, y + q % 3 - 1, z + q / 3 - 1);
  u64 m = n[4].c;
  size_t at = a.bases[id];
#pragma unroll 1
  for (int k = 0; k < 64 && m != 0ull; ++k) {
    const int b = __ffsll((long long)m) - 1;
    m &= m - 1ull;
    uint32_t n26 = 0u;
#pragma unroll
    for (int q = 0; q < 9; ++q) n26 += (uint32_t)((n[q].l >> b) & 1ull) + (uint32_t)((n[q].r >> b) & 1ull) + (q == 4 ? 0u : (uint32_t)((n[q].c >> b) & 1ull));
    const uint32_t x = (uint32_t)(wx * 64 + b);
    uint32_t *p = a.points + 4u * at;
    p[0] = x;
    p[1] = (uint32_t)y;
    p[2] = (uint32_t)z;
    p[3] = n26;
    if (a.values) a.values[at] = a.map[row * (size_t)a.X + (size_t)x];
    ++at;
  }
}

hipError_t launch_thin_begin(const ThinArgs &a, const unsigned long long *mask_in, hipStream_t s) {
  hipLaunchKernelGGL(k_thin_begin, dim3(blocks_for((size_t)a.W64 * (size_t)a.Y * (size_t)a.Z)), dim3(256), 0, s, a, mask_in);
  return hipGetLastError();
}

hipError_t launch_thin_iteration(const ThinArgs &a, uint32_t iteration, int slot, hipStream_t s) {
  hipLaunchKernelGGL(k_thin_candidates, dim3(blocks_for((size_t)a.W64 * (size_t)a.Y * (size_t)a.Z)), dim3(256), 0, s, a, iteration, slot);
  // six blocks per CU hold the 9.6 KB of LDS and 256 threads each
  const size_t n_tiles = (size_t)a.TX * (size_t)a.TY * (size_t)a.TZ;
  const unsigned grid = (unsigned)(n_tiles < 1536u ? n_tiles : 1536u);
  for (int sub = 0; sub < 8; ++sub) hipLaunchKernelGGL(k_thin_subpass, dim3(grid), dim3(256), 0, s, a, slot, sub);
  return hipGetLastError();
}

hipError_t launch_points_count(const PointsArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_points_count, dim3(blocks_for((size_t)a.W64 * (size_t)a.Y * (size_t)a.Z + 1u)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_points_scan(void *temp, size_t &temp_bytes, const uint32_t *counts, uint32_t *bases, size_t n, hipStream_t s) {
  return rocprim::exclusive_scan(temp, temp_bytes, counts, bases, (uint32_t)0, n, rocprim::plus<uint32_t>(), s);
}

hipError_t launch_points_fill(const PointsArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_points_fill, dim3(blocks_for((size_t)a.W64 * (size_t)a.Y * (size_t)a.Z)), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace clvr
