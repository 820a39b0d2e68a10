// geodesic_kernels.hip -- shortest paths inside a mask from labelled seeds (clwh_mask_geodesic) and the path behind a distance
// (clwh_geodesic_trace), gfx950.  The state of a voxel is the 64-bit key  dist << 32 | id.
//   The result.  With D the domain, w(q, p) >= 1 the cost of the step from q to its neighbour p and cap the largest distance kept, the
//   result is the one solution of
//       key(p) = min(seed keys at p,  min over neighbours q in D of key(q) + (w(q, p) << 32))          for p in D,
//   where a candidate whose distance exceeds the cap does not count.  It is the only fixpoint: in any solution the voxel with the
//   smallest key that differs from the true (shortest length, smallest id among the seeds that attain it) pair would have to take that
//   key from a neighbour with a strictly smaller one, since every weight is positive -- and that neighbour is already right.
//   Never below.  Every key a kernel stores is a seed's (0, id) or a stored key of a neighbour in D plus that step's weight: by induction
//   the length and the id of a real path from a real seed, so never below the solution.  Keys only ever get smaller.
//   At rest.  When a round lists no tile, every tile is at its local fixpoint with the halo it would read now, so the equations hold
//   everywhere.  No result depends on the order of blocks, and no block waits for another.
//   The cap.  Distances grow along a shortest path, so a voxel within the cap has a shortest path whose voxels are all within it:
//   dropping every candidate above the cap removes no key that belongs to the result.
//   NO TORN KEYS.  Grow tolerates a halo word read while its owner stores to it, because any mix of old and new bits is a subset of
//   the answer.  Here a new distance with an old id can lie BELOW the answer and would never be corrected.  So the working keys live in
//   a packed uint64 array of the context's scratch (the caller's two uint32 maps cannot carry a pair atomically), every key is a
//   naturally aligned 64-bit word, and every access that can race -- a tile's loads of its halo, the owner's stores -- is ONE relaxed
//   64-bit atomic load or store.  Only the owner stores a tile's keys during the rounds; a halo key read meanwhile is the old or the
//   new one, both real, and the owner whose boundary changed stamps the reader for the next round, behind a kernel boundary.
//   Inside a tile a sweep is two phases with a barrier between them: everybody reads neighbours from LDS, then everybody writes its
//   own voxels, so no LDS word is read while it is written either.
// Tile = 16 x 16 x 8 voxels with a one-voxel halo: 18 x 18 x 10 keys = 25 920 bytes of LDS, six blocks of 256 threads per CU (grow's
// 64 x 16 x 16 would need 128 KiB; 32 x 8 x 8, 64 x 4 x 8 and 32 x 8 x 16 were timed and lost: DESIGN.md, section 4).  A thread owns the column of 8 voxels along z at its (x, y), in registers.  Voxels outside D hold
// the all-ones key, voxels of D that nothing has reached yet hold kUnreached: neither is ever a candidate (their distance field is
// above every cap), and a voxel takes candidates iff its key is not all ones.
#include "tile_work_device.hpp"

namespace clvr {

namespace {

typedef unsigned long long u64;
constexpr int kGX = kGeoTileX, kGY = kGeoTileY, kGZ = kGeoTileZ;  // the tile's core: 16 x 16 x 8
constexpr int kLX = kGX + 2, kLY = kGY + 2, kLZ = kGZ + 2;  // with the halo
constexpr u64 kOutside = ~0ull;                           // not in D (or not in the volume)
constexpr u64 kUnreached = 0xFFFFFFFF00000000ull;         // in D, no seed has reached it: dist = CLWH_DIST_NONE, label = 0

__device__ __forceinline__ u64 geo_load(const u64 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void geo_store(u64 *p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ u64 geo_min(u64 a, u64 b) { return a < b ? a : b; }
// the key one step of cost w behind k; all ones if k is no real key or the distance passes the cap (no sum of real operands wraps:
// dist <= cap <= 0xFFFF0000 and w <= 0xFFFF)
__device__ __forceinline__ u64 geo_step(u64 k, uint32_t w, uint32_t cap) {
  const u64 c = k + ((u64)w << 32);
  return (c < k || (uint32_t)(c >> 32) > cap) ? kOutside : c;
}
__device__ __forceinline__ uint32_t geo_tile_of(const GeoArgs &a, int x, int y, int z) {
  return (uint32_t)(((z / kGZ) * a.tiles.TY + (y / kGY)) * a.tiles.TX + (x / kGX));
}
__device__ __forceinline__ size_t geo_voxel(const GeoArgs &a, int x, int y, int z) {
  return ((size_t)z * (size_t)a.Y + (size_t)y) * (size_t)a.X + (size_t)x;
}

}  // namespace

// every key from the domain's bit and, with CLWH_GEO_FROM_LABELS, the caller's word: all ones outside D, (0, word) for a seed,
// kUnreached else; a tile that holds a seed is stamped for round 1.  A thread per voxel.
__global__ __launch_bounds__(256) void k_geo_init(const GeoArgs a) {
  const size_t total = (size_t)a.X * (size_t)a.Y * (size_t)a.Z, id = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (id >= total) return;
  const size_t row = id / (size_t)a.X;
  const int x = (int)(id - row * (size_t)a.X), z = (int)(row / (size_t)a.Y), y = (int)(row - (size_t)z * (size_t)a.Y);
  const uint32_t byte = a.domain[row * (size_t)a.W64 * 8u + (size_t)(x >> 3)];
  u64 key = kOutside;
  if ((byte >> (x & 7)) & 1u) {
    key = kUnreached;
    const uint32_t word = a.seed_labels ? a.seed_labels[id] : 0u;
    if (word) {
      key = (u64)word;
      a.tiles.stamps[geo_tile_of(a, x, y, z)] = 1u;
    }
  }
  a.keys[id] = key;
}

// the listed seeds (inside the volume with id >= 1: the host checked) that lie in D: the smallest id wins the voxel
__global__ __launch_bounds__(256) void k_geo_seeds(const GeoArgs a) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.n_seeds) return;
  const int x = (int)a.seeds[4u * i], y = (int)a.seeds[4u * i + 1u], z = (int)a.seeds[4u * i + 2u];
  u64 *key = a.keys + geo_voxel(a, x, y, z);
  if (*key == kOutside) return;  // (nobody turns a key into all ones or back)
  atomicMin(key, (u64)a.seeds[4u * i + 3u]);
  a.tiles.stamps[geo_tile_of(a, x, y, z)] = 1u;
}

// One round: a persistent grid takes the listed tiles by ticket; see the head of the file and tile_work_device.hpp.
template <bool CONN26>
__global__ __launch_bounds__(256) void k_geo_round(const GeoArgs a, uint32_t round, int slot) {
  __shared__ u64 s_key[kLZ * kLY * kLX];  // [z + 1][y + 1][x + 1]
  __shared__ TileShared s_tile;
  const uint32_t n = a.tiles.counters[2 * slot];
  if (n == 0u) return;  // an empty round: one word read
  const unsigned t = threadIdx.x;
  const int cx = (int)(t % (unsigned)kGX), cy = (int)(t / (unsigned)kGX);
  const uint32_t cap = a.cap;
  const uint32_t wfx = a.w_face[0], wfy = a.w_face[1], wfz = a.w_face[2];
  u64 *const mine = s_key + (kLY + cy + 1) * kLX + (cx + 1);  // the column's voxel z = 0; a z step is kLY * kLX words
  for (int tx, ty, tz; tile_take(a.tiles, n, slot, s_tile, tx, ty, tz);) {  // (its first barrier: the previous tile's last reads of s_key)
    // the region's keys; what lies outside the volume is outside D
    for (unsigned i = t; i < (unsigned)(kLZ * kLY * kLX); i += 256u) {
      const int lz = (int)(i / (unsigned)(kLY * kLX)), rem = (int)(i % (unsigned)(kLY * kLX)), ly = rem / kLX, lx = rem % kLX;
      const int gx = tx * kGX + lx - 1, gy = ty * kGY + ly - 1, gz = tz * kGZ + lz - 1;
      u64 key = kOutside;
      if (gx >= 0 && gx < a.X && gy >= 0 && gy < a.Y && gz >= 0 && gz < a.Z) key = geo_load(a.keys + geo_voxel(a, gx, gy, gz));
      s_key[i] = key;
    }
    __syncthreads();
    u64 k[kGZ];
#pragma unroll
    for (int z = 0; z < kGZ; ++z) k[z] = mine[z * kLY * kLX];
    const u64 below = mine[-kLY * kLX], above = mine[kGZ * kLY * kLX];  // the halo under and over the column never changes
    uint32_t lowered = 0u;  // bit z: this visit made k[z] smaller

    for (;;) {
      // phase 1: the best candidate from the other columns, read from LDS
      u64 cand[kGZ];
      if (CONN26) {
        // per z of the region (index z + 1): the smallest key among the two columns beside along x, the two along y, the four diagonal
        u64 ax[kLZ], ay[kLZ], ad[kLZ];
#pragma unroll
        for (int z = 0; z < kLZ; ++z) {
          const u64 *p = mine + (z - 1) * kLY * kLX;
          ax[z] = geo_min(p[-1], p[1]);
          ay[z] = geo_min(p[-kLX], p[kLX]);
          ad[z] = geo_min(geo_min(p[-kLX - 1], p[-kLX + 1]), geo_min(p[kLX - 1], p[kLX + 1]));
        }
#pragma unroll
        for (int z = 0; z < kGZ; ++z) {
          u64 c = geo_min(geo_step(ax[z + 1], wfx, cap), geo_step(ay[z + 1], wfy, cap));
          c = geo_min(c, geo_step(ad[z + 1], a.w_edge[2], cap));                          // x and y change
          c = geo_min(c, geo_step(geo_min(ax[z], ax[z + 2]), a.w_edge[1], cap));          // x and z
          c = geo_min(c, geo_step(geo_min(ay[z], ay[z + 2]), a.w_edge[0], cap));          // y and z
          c = geo_min(c, geo_step(geo_min(ad[z], ad[z + 2]), a.w_corner, cap));
          cand[z] = c;
        }
      } else {
#pragma unroll
        for (int z = 0; z < kGZ; ++z) {
          const u64 *p = mine + z * kLY * kLX;
          cand[z] = geo_min(geo_step(geo_min(p[-1], p[1]), wfx, cap), geo_step(geo_min(p[-kLX], p[kLX]), wfy, cap));
        }
      }
      // the column itself, in registers: up, then down
      uint32_t changed = 0u;
      u64 prev = below;
#pragma unroll
      for (int z = 0; z < kGZ; ++z) {
        const u64 c = geo_min(cand[z], geo_step(prev, wfz, cap));
        if (k[z] != kOutside && c < k[z]) {
          k[z] = c;
          changed |= 1u << z;
        }
        prev = k[z];
      }
      prev = above;
#pragma unroll
      for (int z = kGZ - 1; z >= 0; --z) {
        const u64 c = geo_step(prev, wfz, cap);
        if (k[z] != kOutside && c < k[z]) {
          k[z] = c;
          changed |= 1u << z;
        }
        prev = k[z];
      }
      lowered |= changed;
      if (!__syncthreads_or((int)changed)) break;  // (also the barrier between phase 1's reads and phase 2's stores)
      // phase 2: everybody writes its own voxels
#pragma unroll
      for (int z = 0; z < kGZ; ++z)
        if ((changed >> z) & 1u) mine[z * kLY * kLX] = k[z];
      __syncthreads();
    }

    // the owner's stores (a lowered voxel is in D, so inside the volume)
    const int gx = tx * kGX + cx, gy = ty * kGY + cy;
#pragma unroll
    for (int z = 0; z < kGZ; ++z)
      if ((lowered >> z) & 1u) geo_store(a.keys + geo_voxel(a, gx, gy, tz * kGZ + z), k[z]);
    // the neighbouring tiles that can see a lowered key are woken; round 1 counts every real key as lowered
    uint32_t fresh = lowered;
    if (round == 1u) {
#pragma unroll
      for (int z = 0; z < kGZ; ++z) fresh |= (uint32_t)(k[z] >> 32) != 0xFFFFFFFFu ? 1u << z : 0u;
    }
    const bool at_x[3] = {cx == 0, true, cx == kGX - 1}, at_y[3] = {cy == 0, true, cy == kGY - 1};
    const bool at_z[3] = {(fresh & 1u) != 0u, true, ((fresh >> (kGZ - 1)) & 1u) != 0u};
    tile_wake<CONN26>(a.tiles, round, s_tile, tx, ty, tz, fresh != 0u, at_x, at_y, at_z);
  }
}

// the keys split into the caller's maps; reached and max_dist, one set of vector atomics per block (k_grow_reduce's shape).  In place
// (labels = seed_labels) nothing reads seed_labels any more.
__global__ __launch_bounds__(256) void k_geo_finish(const GeoArgs a) {
  const size_t total = (size_t)a.X * (size_t)a.Y * (size_t)a.Z;
  u64 reached = 0ull;
  uint32_t max_dist = 0u;
  for (size_t id = (size_t)blockIdx.x * 256u + threadIdx.x; id < total; id += (size_t)gridDim.x * 256u) {
    const u64 key = a.keys[id];
    const uint32_t d = (uint32_t)(key >> 32);
    const bool is_reached = d != 0xFFFFFFFFu;
    if (a.dist) a.dist[id] = d;
    if (a.labels) a.labels[id] = is_reached ? (uint32_t)key : 0u;
    if (is_reached) {
      ++reached;
      max_dist = max(max_dist, d);
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    reached += __shfl_xor(reached, off);
    max_dist = max(max_dist, (uint32_t)__shfl_xor((int)max_dist, off));
  }
  __shared__ u64 part_reached[4];
  __shared__ uint32_t part_max[4];
  const unsigned wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0u) {
    part_reached[wave] = reached;
    part_max[wave] = max_dist;
  }
  __syncthreads();
  if (threadIdx.x != 0u) return;
  for (int w = 1; w < 4; ++w) {
    reached += part_reached[w];
    max_dist = max(max_dist, part_max[w]);
  }
  if (reached == 0ull) return;
  atomicAdd(&a.result->reached, reached);
  atomicMax(&a.result->max_dist, max_dist);
}

// The path behind a distance: one wave.  Lanes 0 .. 25 test one direction each, in the order (dz, dy, dx) ascending with dx fastest; a
// ballot and the lowest set lane pick the step.  Every step strictly lowers dist, so the walk ends whatever the map holds.
__global__ __launch_bounds__(64) void k_geo_trace(const GeoTraceArgs a) {
  const unsigned lane = threadIdx.x;
  const int q = (int)(lane < 13u ? lane : lane + 1u);  // 13 is the voxel itself
  const int dx = q % 3 - 1, dy = (q / 3) % 3 - 1, dz = q / 9 - 1;
  const int moved = (dx != 0) + (dy != 0) + (dz != 0);
  uint32_t w = 0u;  // 0: no neighbour under the connectivity
  if (lane < 26u) {
    if (moved == 1) w = a.w_face[dx != 0 ? 0 : dy != 0 ? 1 : 2];
    else if (a.conn26) w = moved == 3 ? a.w_corner : a.w_edge[dx == 0 ? 0 : dy == 0 ? 1 : 2];
  }
  int x = a.target[0], y = a.target[1], z = a.target[2];
  size_t at = ((size_t)z * (size_t)a.Y + (size_t)y) * (size_t)a.X + (size_t)x;
  uint32_t d = a.dist[at];
  u64 n = 0ull;
  uint32_t broken = 0u;
  if (d != 0xFFFFFFFFu) {
    for (;;) {
      if (lane < 3u && n < a.capacity) a.points[3u * n + lane] = (uint32_t)(lane == 0u ? x : lane == 1u ? y : z);
      ++n;
      if (d == 0u) break;
      const int px = x + dx, py = y + dy, pz = z + dz;
      bool ok = false;
      uint32_t dn = 0u;
      if (w != 0u && px >= 0 && px < a.X && py >= 0 && py < a.Y && pz >= 0 && pz < a.Z) {
        const size_t to = ((size_t)pz * (size_t)a.Y + (size_t)py) * (size_t)a.X + (size_t)px;
        dn = a.dist[to];
        ok = dn != 0xFFFFFFFFu && dn < d && dn + w == d;  // (dn < d: a sum that wrapped is no step)
        if (ok && a.labels) ok = a.labels[to] == a.labels[at];
      }
      const u64 votes = __ballot(ok);
      if (votes == 0ull) {
        broken = 1u;
        break;
      }
      const int pick = __ffsll((long long)votes) - 1;
      x = __shfl(px, pick);
      y = __shfl(py, pick);
      z = __shfl(pz, pick);
      d = (uint32_t)__shfl((int)dn, pick);
      at = ((size_t)z * (size_t)a.Y + (size_t)y) * (size_t)a.X + (size_t)x;
    }
  }
  if (lane == 0u) {
    a.result->n_points = n;
    a.result->broken = broken;
  }
}

hipError_t launch_geo_init(const GeoArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_geo_init, dim3(blocks_for((size_t)a.X * (size_t)a.Y * (size_t)a.Z)), dim3(256), 0, s, a);
  if (a.n_seeds != 0u) hipLaunchKernelGGL(k_geo_seeds, dim3(blocks_for(a.n_seeds)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_geo_round(const GeoArgs &a, uint32_t round, int slot, hipStream_t s) {
  // five blocks per CU hold their 26 KB of LDS each with room to spare
  return launch_tile_round(a.conn26 ? k_geo_round<true> : k_geo_round<false>, 1280u, a, round, slot, s);
}

hipError_t launch_geo_finish(const GeoArgs &a, hipStream_t s) {
  const unsigned need = blocks_for((size_t)a.X * (size_t)a.Y * (size_t)a.Z), grid = need < 2048u ? need : 2048u;
  hipLaunchKernelGGL(k_geo_finish, dim3(grid), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_geo_trace(const GeoTraceArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_geo_trace, dim3(1), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace clvr
