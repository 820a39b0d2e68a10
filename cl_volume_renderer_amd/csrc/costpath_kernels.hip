// costpath_kernels.hip -- shortest paths through a cost field from labelled seeds (clwh_cost_geodesic), the path behind such a distance
// (clwh_cost_trace) and the cost field from a table (clwh_cost_from_field), gfx950.  The state of a voxel is geodesic_kernels.hip's
// 64-bit key  dist << 32 | id, and everything the head of that file proves holds here word for word with
//       w(q, p) = mult(direction of the step) * cost(p),     D = { p : cost(p) >= 1 and p's bit in the domain, if there is one },
// because the proof needs of w only that it is positive: the one fixpoint, never below, at rest, the cap, NO TORN KEYS (the working
// keys are the same packed uint64 scratch; every key that crosses a tile face is one relaxed 64-bit atomic load or store; only the
// owner stores), the two-phase LDS sweep.  The init / seeds kernels are the geodesic's with the domain test extended to cost >= 1;
// the finish kernel IS the geodesic's (launch_geo_finish).
//   Why the cost of the voxel ENTERED and not a symmetric cost(p) + cost(q).  A design decision, not a measurement.  The thread that
//   owns a column of the tile relaxes its own eight voxels, so with the entered voxel's cost it needs only its own eight costs, which
//   it keeps in registers: neighbours' costs never go to LDS and the tile stays at 18 x 18 x 10 keys.  The geodesic's grouping "the
//   minimum per direction class, then one add per class" survives, because every step of a class into p has the same cost; the add
//   becomes mult_class * cost[z], at most 255 * 65535 < 2^24 and so exact in a 24-bit multiply.  With the symmetric cost the minimum
//   would have to be taken over key(q) + mult * cost(q): an add per neighbour instead of per class, and 5832 more bytes of LDS.
//   The eight costs are 16 bits each and travel two to a register, four VGPRs per column, and the products are made where they are
//   added (see the sweep).  The 26-connected instance has 168 registers to stay at the geodesic's three waves per SIMD (512 / 3,
//   rounded down to the granule of 8) and k_geo_round<true> takes 158 of them; the 6-connected one has 80 for six waves.  Both fit,
//   without scratch memory: profiles/costpath_resource_usage.txt.
//   No sum wraps.  dist <= cap <= 0xFF000000 and w <= 0xFEFF01, so dist + w < 2^32; the two keys that are no distances (all ones,
//   kUnreached) wrap the 64-bit sum instead, which cost_step sees.
#include "tile_work_device.hpp"

namespace clvr {

namespace {

typedef unsigned long long u64;
constexpr int kGX = kGeoTileX, kGY = kGeoTileY, kGZ = kGeoTileZ;  // the tile's core: 16 x 16 x 8
constexpr int kLX = kGX + 2, kLY = kGY + 2, kLZ = kGZ + 2;  // with the halo
constexpr u64 kOutside = ~0ull;                           // not in D (or not in the volume)
constexpr u64 kUnreached = 0xFFFFFFFF00000000ull;         // in D, no seed has reached it: dist = CLWH_DIST_NONE, label = 0
static_assert(kGZ % 2 == 0, "a column's costs travel two to a register");

__device__ __forceinline__ u64 cost_load(const u64 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cost_store(u64 *p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ u64 cost_min(u64 a, u64 b) { return a < b ? a : b; }
// the key one step of cost w < 2^24 behind k; all ones if k is no real key or the distance passes the cap
__device__ __forceinline__ u64 cost_step(u64 k, uint32_t w, uint32_t cap) {
  const u64 c = k + ((u64)w << 32);
  return (c < k || (uint32_t)(c >> 32) > cap) ? kOutside : c;
}
__device__ __forceinline__ uint32_t cost_tile_of(const GeoArgs &g, int x, int y, int z) {
  return (uint32_t)(((z / kGZ) * g.tiles.TY + (y / kGY)) * g.tiles.TX + (x / kGX));
}
__device__ __forceinline__ size_t cost_voxel(const GeoArgs &g, int x, int y, int z) {
  return ((size_t)z * (size_t)g.Y + (size_t)y) * (size_t)g.X + (size_t)x;
}

}  // namespace

// every key from the cost, the domain's bit if there is a domain and, with CLWH_GEO_FROM_LABELS, the caller's word: all ones outside
// D, (0, word) for a seed, kUnreached else; a tile that holds a seed is stamped for round 1.  A thread per voxel.
__global__ __launch_bounds__(256) void k_cost_init(const CostArgs a) {
  const GeoArgs &g = a.g;
  const size_t total = (size_t)g.X * (size_t)g.Y * (size_t)g.Z, id = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (id >= total) return;
  const size_t row = id / (size_t)g.X;
  const int x = (int)(id - row * (size_t)g.X), z = (int)(row / (size_t)g.Y), y = (int)(row - (size_t)z * (size_t)g.Y);
  bool in = a.cost[id] != 0u;
  if (in && g.domain) in = ((g.domain[row * (size_t)g.W64 * 8u + (size_t)(x >> 3)] >> (x & 7)) & 1u) != 0u;
  u64 key = kOutside;
  if (in) {
    key = kUnreached;
    const uint32_t word = g.seed_labels ? g.seed_labels[id] : 0u;
    if (word) {
      key = (u64)word;
      g.tiles.stamps[cost_tile_of(g, x, y, z)] = 1u;
    }
  }
  g.keys[id] = key;
}

// the listed seeds (inside the volume with id >= 1: the host checked) that lie in D: the smallest id wins the voxel
__global__ __launch_bounds__(256) void k_cost_seeds(const CostArgs a) {
  const GeoArgs &g = a.g;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= g.n_seeds) return;
  const int x = (int)g.seeds[4u * i], y = (int)g.seeds[4u * i + 1u], z = (int)g.seeds[4u * i + 2u];
  u64 *key = g.keys + cost_voxel(g, x, y, z);
  if (*key == kOutside) return;  // (nobody turns a key into all ones or back)
  atomicMin(key, (u64)g.seeds[4u * i + 3u]);
  g.tiles.stamps[cost_tile_of(g, x, y, z)] = 1u;
}

// One round: a persistent grid takes the listed tiles by ticket; see the head of the file and tile_work_device.hpp.
template <bool CONN26>
__global__ __launch_bounds__(256) void k_cost_round(const CostArgs a, uint32_t round, int slot) {
  __shared__ u64 s_key[kLZ * kLY * kLX];  // [z + 1][y + 1][x + 1]
  __shared__ TileShared s_tile;
  const GeoArgs &g = a.g;
  const uint32_t n = g.tiles.counters[2 * slot];
  if (n == 0u) return;  // an empty round: one word read
  const unsigned t = threadIdx.x;
  const int cx = (int)(t % (unsigned)kGX), cy = (int)(t / (unsigned)kGX);
  const uint32_t cap = g.cap;
  const uint32_t mfx = g.w_face[0], mfy = g.w_face[1], mfz = g.w_face[2];
  u64 *const mine = s_key + (kLY + cy + 1) * kLX + (cx + 1);  // the column's voxel z = 0; a z step is kLY * kLX words
  for (int tx, ty, tz; tile_take(g.tiles, n, slot, s_tile, tx, ty, tz);) {  // (its first barrier: the previous tile's last reads of s_key)
    // the region's keys; what lies outside the volume is outside D
    for (unsigned i = t; i < (unsigned)(kLZ * kLY * kLX); i += 256u) {
      const int lz = (int)(i / (unsigned)(kLY * kLX)), rem = (int)(i % (unsigned)(kLY * kLX)), ly = rem / kLX, lx = rem % kLX;
      const int gx = tx * kGX + lx - 1, gy = ty * kGY + ly - 1, gz = tz * kGZ + lz - 1;
      u64 key = kOutside;
      if (gx >= 0 && gx < g.X && gy >= 0 && gy < g.Y && gz >= 0 && gz < g.Z) key = cost_load(g.keys + cost_voxel(g, gx, gy, gz));
      s_key[i] = key;
    }
    // the column's own costs, two to a register; 0 outside the volume, where the key is all ones and takes no candidate
    const int gx = tx * kGX + cx, gy = ty * kGY + cy;
    uint32_t pair[kGZ / 2];
#pragma unroll
    for (int z = 0; z < kGZ; z += 2) {
      uint32_t lo = 0u, hi = 0u;
      if (gx < g.X && gy < g.Y) {
        if (tz * kGZ + z < g.Z) lo = a.cost[cost_voxel(g, gx, gy, tz * kGZ + z)];
        if (tz * kGZ + z + 1 < g.Z) hi = a.cost[cost_voxel(g, gx, gy, tz * kGZ + z + 1)];
      }
      pair[z / 2] = lo | hi << 16;
    }
#define COST_OF(z) (((z) & 1) ? pair[(z) / 2] >> 16 : pair[(z) / 2] & 0xFFFFu)
    __syncthreads();
    u64 k[kGZ];
#pragma unroll
    for (int z = 0; z < kGZ; ++z) k[z] = mine[z * kLY * kLX];
    const u64 below = mine[-kLY * kLX], above = mine[kGZ * kLY * kLX];  // the halo under and over the column never changes
    uint32_t lowered = 0u;  // bit z: this visit made k[z] smaller

    for (;;) {
      // The step costs are products of values that do not change in this loop, and the compiler would keep all of them (seven per
      // voxel under 26-connectivity) in registers across it: 254 VGPRs and two waves per SIMD.  The empty statement makes the costs
      // opaque once per sweep, so a product lives from its multiply to its add.
#pragma unroll
      for (int i = 0; i < kGZ / 2; ++i) asm volatile("" : "+v"(pair[i]));
      // phase 1: the best candidate from the other columns, read from LDS
      u64 cand[kGZ];
      if (CONN26) {
        // per z of the region (index z + 1): the smallest key among the two columns beside along x, the two along y, the four diagonal
        u64 ax[kLZ], ay[kLZ], ad[kLZ];
#pragma unroll
        for (int z = 0; z < kLZ; ++z) {
          const u64 *p = mine + (z - 1) * kLY * kLX;
          ax[z] = cost_min(p[-1], p[1]);
          ay[z] = cost_min(p[-kLX], p[kLX]);
          ad[z] = cost_min(cost_min(p[-kLX - 1], p[-kLX + 1]), cost_min(p[kLX - 1], p[kLX + 1]));
        }
#pragma unroll
        for (int z = 0; z < kGZ; ++z) {
          const uint32_t cz = COST_OF(z);
          u64 c = cost_min(cost_step(ax[z + 1], __umul24(mfx, cz), cap), cost_step(ay[z + 1], __umul24(mfy, cz), cap));
          c = cost_min(c, cost_step(ad[z + 1], __umul24(g.w_edge[2], cz), cap));                          // x and y change
          c = cost_min(c, cost_step(cost_min(ax[z], ax[z + 2]), __umul24(g.w_edge[1], cz), cap));         // x and z
          c = cost_min(c, cost_step(cost_min(ay[z], ay[z + 2]), __umul24(g.w_edge[0], cz), cap));         // y and z
          c = cost_min(c, cost_step(cost_min(ad[z], ad[z + 2]), __umul24(g.w_corner, cz), cap));
          cand[z] = c;
        }
      } else {
#pragma unroll
        for (int z = 0; z < kGZ; ++z) {
          const u64 *p = mine + z * kLY * kLX;
          const uint32_t cz = COST_OF(z);
          cand[z] = cost_min(cost_step(cost_min(p[-1], p[1]), __umul24(mfx, cz), cap), cost_step(cost_min(p[-kLX], p[kLX]), __umul24(mfy, cz), cap));
        }
      }
      // the column itself, in registers: up, then down; either way the step enters voxel z
      uint32_t changed = 0u;
      u64 prev = below;
#pragma unroll
      for (int z = 0; z < kGZ; ++z) {
        const u64 c = cost_min(cand[z], cost_step(prev, __umul24(mfz, COST_OF(z)), cap));
        if (k[z] != kOutside && c < k[z]) {
          k[z] = c;
          changed |= 1u << z;
        }
        prev = k[z];
      }
      prev = above;
#pragma unroll
      for (int z = kGZ - 1; z >= 0; --z) {
        const u64 c = cost_step(prev, __umul24(mfz, COST_OF(z)), cap);
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
#undef COST_OF

    // the owner's stores (a lowered voxel is in D, so inside the volume)
#pragma unroll
    for (int z = 0; z < kGZ; ++z)
      if ((lowered >> z) & 1u) cost_store(g.keys + cost_voxel(g, gx, gy, tz * kGZ + z), k[z]);
    // the neighbouring tiles that can see a lowered key are woken; round 1 counts every real key as lowered
    uint32_t fresh = lowered;
    if (round == 1u) {
#pragma unroll
      for (int z = 0; z < kGZ; ++z) fresh |= (uint32_t)(k[z] >> 32) != 0xFFFFFFFFu ? 1u << z : 0u;
    }
    const bool at_x[3] = {cx == 0, true, cx == kGX - 1}, at_y[3] = {cy == 0, true, cy == kGY - 1};
    const bool at_z[3] = {(fresh & 1u) != 0u, true, ((fresh >> (kGZ - 1)) & 1u) != 0u};
    tile_wake<CONN26>(g.tiles, round, s_tile, tx, ty, tz, fresh != 0u, at_x, at_y, at_z);
  }
}

// The path behind a distance: one wave, k_geo_trace's walk.  Lanes 0 .. 25 test one direction each, in the order (dz, dy, dx) ascending
// with dx fastest; a ballot and the lowest set lane pick the step.  The forward path entered the CURRENT voxel from the one the walk
// goes to next, so the step's cost is mult(dir) * cost(current).  Every step strictly lowers dist, so the walk ends whatever the maps hold.
__global__ __launch_bounds__(64) void k_cost_trace(const CostTraceArgs a) {
  const GeoTraceArgs &g = a.g;
  const unsigned lane = threadIdx.x;
  const int q = (int)(lane < 13u ? lane : lane + 1u);  // 13 is the voxel itself
  const int dx = q % 3 - 1, dy = (q / 3) % 3 - 1, dz = q / 9 - 1;
  const int moved = (dx != 0) + (dy != 0) + (dz != 0);
  uint32_t m = 0u;  // 0: no neighbour under the connectivity
  if (lane < 26u) {
    if (moved == 1) m = g.w_face[dx != 0 ? 0 : dy != 0 ? 1 : 2];
    else if (g.conn26) m = moved == 3 ? g.w_corner : g.w_edge[dx == 0 ? 0 : dy == 0 ? 1 : 2];
  }
  int x = g.target[0], y = g.target[1], z = g.target[2];
  size_t at = ((size_t)z * (size_t)g.Y + (size_t)y) * (size_t)g.X + (size_t)x;
  uint32_t d = g.dist[at];
  u64 n = 0ull;
  uint32_t broken = 0u;
  if (d != 0xFFFFFFFFu) {
    for (;;) {
      if (lane < 3u && n < g.capacity) g.points[3u * n + lane] = (uint32_t)(lane == 0u ? x : lane == 1u ? y : z);
      ++n;
      if (d == 0u) break;
      const uint32_t w = __umul24(m, (uint32_t)a.cost[at]);  // 0: no neighbour, or a wall that no path enters
      const int px = x + dx, py = y + dy, pz = z + dz;
      bool ok = false;
      uint32_t dn = 0u;
      if (w != 0u && px >= 0 && px < g.X && py >= 0 && py < g.Y && pz >= 0 && pz < g.Z) {
        const size_t to = ((size_t)pz * (size_t)g.Y + (size_t)py) * (size_t)g.X + (size_t)px;
        dn = g.dist[to];
        ok = dn != 0xFFFFFFFFu && dn < d && (u64)dn + w == (u64)d;
        if (ok && g.labels) ok = g.labels[to] == g.labels[at];
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
      at = ((size_t)z * (size_t)g.Y + (size_t)y) * (size_t)g.X + (size_t)x;
    }
  }
  if (lane == 0u) {
    g.result->n_points = n;
    g.result->broken = broken;
  }
}

// cost(p) = table[clamp((s(p) - lo) >> shift, 0, n - 1)], 0 where the domain's bit is clear.  A lane per voxel, x fastest: the 16-bit
// stores of a wave are one run of 128 bytes.  The difference is taken in unsigned 64 bits once s >= lo is known, so no lo overflows it.
__global__ __launch_bounds__(256) void k_cost_field(const CostFieldArgs a) {
  const size_t total = (size_t)a.X * (size_t)a.Y * (size_t)a.Z, id = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (id >= total) return;
  const size_t row = id / (size_t)a.X;
  const int x = (int)(id - row * (size_t)a.X);
  if (a.domain && !((a.domain[row * (size_t)a.W64 * 8u + (size_t)(x >> 3)] >> (x & 7)) & 1u)) {
    a.cost[id] = 0u;
    return;
  }
  long long s;
  if (a.kind == CLWH_COST_SRC_U32) {
    s = (long long)a.words[id];
  } else if (a.kind == CLWH_COST_SRC_VALUE) {
    s = (long long)a.volume[id];
  } else {
    const int z = (int)(row / (size_t)a.Y), y = (int)(row - (size_t)z * (size_t)a.Y);
    const size_t sy = (size_t)a.X, sz = (size_t)a.X * (size_t)a.Y;
    const long long gx = (long long)a.volume[id + (x + 1 < a.X ? 1u : 0u)] - (long long)a.volume[id - (x > 0 ? 1u : 0u)];
    const long long gy = (long long)a.volume[id + (y + 1 < a.Y ? sy : 0u)] - (long long)a.volume[id - (y > 0 ? sy : 0u)];
    const long long gz = (long long)a.volume[id + (z + 1 < a.Z ? sz : 0u)] - (long long)a.volume[id - (z > 0 ? sz : 0u)];
    s = gx * gx + gy * gy + gz * gz;
  }
  u64 index = 0ull;
  if (s > a.lo) {
    index = ((u64)s - (u64)a.lo) >> a.shift;
    if (index > (u64)(a.n - 1u)) index = (u64)(a.n - 1u);
  }
  a.cost[id] = a.table[index];
}

hipError_t launch_cost_init(const CostArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_cost_init, dim3(blocks_for((size_t)a.g.X * (size_t)a.g.Y * (size_t)a.g.Z)), dim3(256), 0, s, a);
  if (a.g.n_seeds != 0u) hipLaunchKernelGGL(k_cost_seeds, dim3(blocks_for(a.g.n_seeds)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_cost_round(const CostArgs &a, uint32_t round, int slot, hipStream_t s) {
  // launch_tile_round with the worklist at a.g.tiles, and the geodesic's grid: five blocks per CU hold their 26 KB of LDS each
  enqueue_tile_list(a.g.tiles, round, slot, s);
  const size_t n_tiles = (size_t)a.g.tiles.TX * (size_t)a.g.tiles.TY * (size_t)a.g.tiles.TZ;
  const unsigned grid = (unsigned)(n_tiles < 1280u ? n_tiles : 1280u);
  if (a.g.conn26) hipLaunchKernelGGL(k_cost_round<true>, dim3(grid), dim3(256), 0, s, a, round, slot);
  else hipLaunchKernelGGL(k_cost_round<false>, dim3(grid), dim3(256), 0, s, a, round, slot);
  return hipGetLastError();
}

hipError_t launch_cost_trace(const CostTraceArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_cost_trace, dim3(1), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_cost_field(const CostFieldArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_cost_field, dim3(blocks_for((size_t)a.X * (size_t)a.Y * (size_t)a.Z)), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace clvr
