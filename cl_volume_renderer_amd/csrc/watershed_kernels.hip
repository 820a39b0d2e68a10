// watershed_kernels.hip -- the seeded watershed of a cost field (clwh_watershed), gfx950: every voxel of
//       D = { p : cost(p) >= 1 and p's bit in the domain, if there is one }
// gets the height of the lowest pass to it from a seed, and the seed whose flood arrives first.  Two phases over the geodesic's tiles
// and worklist (tile_work_device.hpp), because one key  level << 32 | id  relaxed to rest depends on the schedule under a maximum: two
// different keys at a voxel can step to the same key at its neighbour, so a candidate that came before the voxel's own key fell stays.
//   The state of a voxel is ONE uint32, key = M << 16 | L, L <= plateau_cap <= 65534; a seed's voxel holds 0, and all ones (kNone) is
//   "nothing has arrived".  Stepping into p with c = cost(p) >= 1 is
//       step(k, c) = c << 16            if k < c << 16          (c > M: the pass gets higher, the plateau count starts again)
//                    k + (L < cap)      else                    ((M, min(L + 1, cap)); kNone stays kNone, its L being 65535)
//   which is monotone in k (k <= k' gives step(k, c) <= step(k', c)) and never lowers (step(k, c) >= k).  A voxel of D whose cost is
//   above level_cap takes no candidate: M rises only by entering a voxel, to that voxel's cost, so that drops exactly the states whose
//   M exceeds the cap.  The thread folds both tests into the cost it keeps: 0 = takes nothing.
//   Phase 1, the result.  ML(p) = the smallest state of a path in D from a seed to p.  Every key a kernel stores is 0 at a seed or
//   step(a stored key of a neighbour in D, cost(p)): by induction the state of a real path, so NEVER BELOW ML.  Keys only get smaller.
//   AT REST (a round lists no tile) every tile is at its local fixpoint with the halo it would read now, so key(p) <= step(key(q),
//   cost(p)) for every pair of neighbours in D; along a path s = p0, .., pn that attains ML(p), key(p0) = 0 and, by monotonicity,
//   key(p_i) <= step(key(p_i-1), c_i) <= the path's state at p_i: key(p) <= ML(p).  So the keys at rest are ML, the ONE FIXPOINT
//   among the assignments of real paths' states, whatever the order of blocks.  All neighbours step into p by the same function, so
//   the minimum over them is taken first and one step made per voxel and sweep (under 26-connectivity too: there are no multipliers).
//   A HALO READ WHILE ITS OWNER STORES.  A key is one naturally aligned 32-bit word; every access that can race -- a tile's loads of
//   its halo, the owner's stores -- is one relaxed 32-bit atomic load or store at agent scope, and only the owner stores a tile's keys
//   during the rounds.  The word read is the old key or the new one, both states of real paths; the owner whose boundary fell stamps
//   the reader for the next round, behind a kernel boundary.  Inside a tile a sweep reads neighbours from LDS, then a barrier, then
//   everybody writes its own voxels.
//   The rounds.  Cutting a loop out of a path never raises its state (the state where the loop closes is no lower than where it
//   opened, and the rest is monotone), so ML(p) is attained by a path that visits no voxel twice, which crosses fewer tile faces than
//   the volume has voxels; after round r every voxel with such a path across fewer than r faces is final: X * Y * Z + 2 rounds.
//   Phase 2, the labels, behind the kernel boundary, when every state is final.  q -> p is an edge iff step(ML(q), cost(p)) == ML(p);
//   label(p) = the smallest id of a seed from whose voxel p is reached along edges.  No edge enters a seed's voxel (a step gives at
//   least 1 << 16) or an unreached one (a step of a real key is real, and the label of an unreached q is none), so the test needs
//   neither the domain nor the caps.  The working label is id - 1 with all ones for none, and the relaxation is
//       wlab(p) = min(wlab(p), wlab(q))  over the edges q -> p.
//   Every label stored is a seed's own or a stored label of a q with an edge to p: a seed that reaches p, never below the answer; labels
//   only fall; at rest wlab(p) <= wlab(q) along the edges from the smallest such seed, whose voxel holds its id.  The halo argument is
//   phase 1's, word for word.  The longest chain of edges that the answer needs visits no voxel twice either: the same bound.
//   Per voxel the edges are found once per visit, as a bit per neighbour, from the interval of states that step to ML(p):
//       [0, c << 16)  if ML(p) == c << 16;    else { ML(p) - 1 };    and ML(p) itself if L == cap   (cap == 0: never ML(p) - 1).
// Tile = the geodesic's 16 x 16 x 8 with a one-voxel halo, 256 threads, a thread per column of eight voxels, its costs two to a VGPR.
// Phase 1 keeps 18 x 18 x 10 uint32 keys in LDS, 12 960 bytes; phase 2 the states and the labels, 25 920 bytes.  Phase 2's loads are
// fenced voxel by voxel (the empty asm statements): written plainly the 26-connected instance takes 256 VGPRs, one wave per SIMD, and
// spills when launch bounds ask for more; fenced it takes 128, four waves.  No kernel uses scratch memory:
// profiles/watershed_resource_usage.txt.
#include "tile_work_device.hpp"

namespace clvr {

namespace {

constexpr int kGX = kGeoTileX, kGY = kGeoTileY, kGZ = kGeoTileZ;  // the tile's core: 16 x 16 x 8
constexpr int kLX = kGX + 2, kLY = kGY + 2, kLZ = kGZ + 2;  // with the halo
constexpr int kPlane = kLY * kLX, kRegion = kLZ * kPlane;
constexpr uint32_t kNone = 0xFFFFFFFFu;  // a state: nothing has arrived (or can); a working label: no seed
static_assert(kGZ % 2 == 0, "a column's costs travel two to a register");

__device__ __forceinline__ uint32_t ws_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void ws_store(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t ws_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
// the state one step into a voxel of cost c behind k (see the head of the file); kNone gives kNone as long as c <= 65535
__device__ __forceinline__ uint32_t ws_step(uint32_t k, uint32_t c, uint32_t cap) {
  const uint32_t hi = c << 16;
  return k < hi ? hi : k + ((k & 0xFFFFu) < cap ? 1u : 0u);
}
__device__ __forceinline__ uint32_t ws_tile_of(const WsArgs &a, int x, int y, int z) {
  return (uint32_t)(((z / kGZ) * a.tiles.TY + (y / kGY)) * a.tiles.TX + (x / kGX));
}
__device__ __forceinline__ size_t ws_voxel(const WsArgs &a, int x, int y, int z) {
  return ((size_t)z * (size_t)a.Y + (size_t)y) * (size_t)a.X + (size_t)x;
}
// a region of the tile with its halo from a word array; what lies outside the volume holds kNone
__device__ __forceinline__ void ws_load_region(const WsArgs &a, const uint32_t *words, uint32_t *s, int tx, int ty, int tz) {
  for (unsigned i = threadIdx.x; i < (unsigned)kRegion; i += 256u) {
    const int lz = (int)(i / (unsigned)kPlane), rem = (int)(i % (unsigned)kPlane), ly = rem / kLX, lx = rem % kLX;
    const int gx = tx * kGX + lx - 1, gy = ty * kGY + ly - 1, gz = tz * kGZ + lz - 1;
    uint32_t v = kNone;
    if (gx >= 0 && gx < a.X && gy >= 0 && gy < a.Y && gz >= 0 && gz < a.Z) v = ws_load(words + ws_voxel(a, gx, gy, gz));
    s[i] = v;
  }
}

}  // namespace

// both arrays from the cost, the domain's bit if there is a domain and, with CLWH_GEO_FROM_LABELS, the caller's word: state 0 and
// label word - 1 for a seed, none and none else; a tile that holds a seed is stamped for round 1 of both phases.  A thread per voxel.
__global__ __launch_bounds__(256) void k_ws_init(const WsArgs a) {
  const size_t total = (size_t)a.X * (size_t)a.Y * (size_t)a.Z, id = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (id >= total) return;
  const size_t row = id / (size_t)a.X;
  const int x = (int)(id - row * (size_t)a.X), z = (int)(row / (size_t)a.Y), y = (int)(row - (size_t)z * (size_t)a.Y);
  bool in = a.cost[id] != 0u;
  if (in && a.domain) in = ((a.domain[row * (size_t)a.W64 * 8u + (size_t)(x >> 3)] >> (x & 7)) & 1u) != 0u;
  uint32_t state = kNone, lab = kNone;
  if (in) {
    const uint32_t word = a.seed_labels ? a.seed_labels[id] : 0u;
    if (word) {
      state = 0u;
      lab = word - 1u;
      const uint32_t tile = ws_tile_of(a, x, y, z);
      a.stamps_level[tile] = 1u;
      a.stamps_label[tile] = 1u;
    }
  }
  a.state[id] = state;
  a.wlab[id] = lab;
}

// the listed seeds (inside the volume with id >= 1: the host checked) that lie in D: the smallest id wins the voxel
__global__ __launch_bounds__(256) void k_ws_seeds(const WsArgs a) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.n_seeds) return;
  const int x = (int)a.seeds[4u * i], y = (int)a.seeds[4u * i + 1u], z = (int)a.seeds[4u * i + 2u];
  const size_t id = ws_voxel(a, x, y, z);
  bool in = a.cost[id] != 0u;
  if (in && a.domain) in = ((a.domain[((size_t)z * (size_t)a.Y + (size_t)y) * (size_t)a.W64 * 8u + (size_t)(x >> 3)] >> (x & 7)) & 1u) != 0u;
  if (!in) return;
  a.state[id] = 0u;  // (every writer of this word in this kernel writes 0)
  atomicMin(a.wlab + id, a.seeds[4u * i + 3u] - 1u);
  const uint32_t tile = ws_tile_of(a, x, y, z);
  a.stamps_level[tile] = 1u;
  a.stamps_label[tile] = 1u;
}

// One round of phase 1: a persistent grid takes the listed tiles by ticket; see the head of the file and tile_work_device.hpp.
template <bool CONN26>
__global__ __launch_bounds__(256) void k_ws_level_round(const WsArgs a, uint32_t round, int slot) {
  __shared__ uint32_t s_key[kRegion];  // [z + 1][y + 1][x + 1]
  __shared__ TileShared s_tile;
  const uint32_t n = a.tiles.counters[2 * slot];
  if (n == 0u) return;  // an empty round: one word read
  const unsigned t = threadIdx.x;
  const int cx = (int)(t % (unsigned)kGX), cy = (int)(t / (unsigned)kGX);
  const uint32_t cap = a.plateau_cap, level_cap = a.level_cap;
  uint32_t *const mine = s_key + (kLY + cy + 1) * kLX + (cx + 1);  // the column's voxel z = 0; a z step is kPlane words
  for (int tx, ty, tz; tile_take(a.tiles, n, slot, s_tile, tx, ty, tz);) {  // (its first barrier: the previous tile's last reads of s_key)
    ws_load_region(a, a.state, s_key, tx, ty, tz);
    // the column's own costs, two to a register; 0 where the voxel takes no candidate: outside the volume or D, or above the level cap
    const int gx = tx * kGX + cx, gy = ty * kGY + cy;
    uint32_t pair[kGZ / 2];
#pragma unroll
    for (int z = 0; z < kGZ; z += 2) {
      uint32_t c2[2] = {0u, 0u};
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int gz = tz * kGZ + z + h;
        if (gx < a.X && gy < a.Y && gz < a.Z) {
          uint32_t c = a.cost[ws_voxel(a, gx, gy, gz)];
          if (c > level_cap) c = 0u;
          if (c && a.domain && !((a.domain[((size_t)gz * (size_t)a.Y + (size_t)gy) * (size_t)a.W64 * 8u + (size_t)(gx >> 3)] >> (gx & 7)) & 1u)) c = 0u;
          c2[h] = c;
        }
      }
      pair[z / 2] = c2[0] | c2[1] << 16;
    }
#define WS_COST_OF(z) (((z) & 1) ? pair[(z) / 2] >> 16 : pair[(z) / 2] & 0xFFFFu)
    __syncthreads();
    uint32_t k[kGZ];
#pragma unroll
    for (int z = 0; z < kGZ; ++z) k[z] = mine[z * kPlane];
    const uint32_t below = mine[-kPlane], above = mine[kGZ * kPlane];  // the halo under and over the column never changes
    uint32_t lowered = 0u;  // bit z: this visit made k[z] smaller

    for (;;) {
      // the smallest key among the other columns' neighbours of each voxel, read from LDS
      uint32_t lat[kGZ];
      if (CONN26) {
        uint32_t ring[kLZ];  // per z of the region (index z + 1): the smallest of the eight columns around
#pragma unroll
        for (int z = 0; z < kLZ; ++z) {
          const uint32_t *p = mine + (z - 1) * kPlane;
          ring[z] = ws_min(ws_min(ws_min(p[-1], p[1]), ws_min(p[-kLX], p[kLX])), ws_min(ws_min(p[-kLX - 1], p[-kLX + 1]), ws_min(p[kLX - 1], p[kLX + 1])));
        }
#pragma unroll
        for (int z = 0; z < kGZ; ++z) lat[z] = ws_min(ring[z], ws_min(ring[z + 1], ring[z + 2]));
      } else {
#pragma unroll
        for (int z = 0; z < kGZ; ++z) {
          const uint32_t *p = mine + z * kPlane;
          lat[z] = ws_min(ws_min(p[-1], p[1]), ws_min(p[-kLX], p[kLX]));
        }
      }
      // the column itself, in registers: up, then down
      uint32_t changed = 0u;
#pragma unroll
      for (int z = 0; z < kGZ; ++z) {
        const uint32_t c = WS_COST_OF(z);
        const uint32_t m = ws_min(lat[z], ws_min(z > 0 ? k[z > 0 ? z - 1 : 0] : below, z + 1 < kGZ ? k[z + 1 < kGZ ? z + 1 : 0] : above));
        const uint32_t s = ws_step(m, c, cap);
        if (c != 0u && s < k[z]) {
          k[z] = s;
          changed |= 1u << z;
        }
      }
#pragma unroll
      for (int z = kGZ - 2; z >= 0; --z) {
        const uint32_t c = WS_COST_OF(z);
        const uint32_t s = ws_step(k[z + 1], c, cap);
        if (c != 0u && s < k[z]) {
          k[z] = s;
          changed |= 1u << z;
        }
      }
      lowered |= changed;
      if (!__syncthreads_or((int)changed)) break;  // (also the barrier between the reads above and the stores below)
#pragma unroll
      for (int z = 0; z < kGZ; ++z)
        if ((changed >> z) & 1u) mine[z * kPlane] = k[z];
      __syncthreads();
    }
#undef WS_COST_OF

    // the owner's stores (a lowered voxel is in D, so inside the volume)
#pragma unroll
    for (int z = 0; z < kGZ; ++z)
      if ((lowered >> z) & 1u) ws_store(a.state + ws_voxel(a, gx, gy, tz * kGZ + z), k[z]);
    // the neighbouring tiles that can see a lowered key are woken; round 1 counts every real key as lowered
    uint32_t fresh = lowered;
    if (round == 1u) {
#pragma unroll
      for (int z = 0; z < kGZ; ++z) fresh |= k[z] != kNone ? 1u << z : 0u;
    }
    const bool at_x[3] = {cx == 0, true, cx == kGX - 1}, at_y[3] = {cy == 0, true, cy == kGY - 1};
    const bool at_z[3] = {(fresh & 1u) != 0u, true, ((fresh >> (kGZ - 1)) & 1u) != 0u};
    tile_wake<CONN26>(a.tiles, round, s_tile, tx, ty, tz, fresh != 0u, at_x, at_y, at_z);
  }
}

// One round of phase 2, over the final states.
template <bool CONN26>
__global__ __launch_bounds__(256) void k_ws_label_round(const WsArgs a, uint32_t round, int slot) {
  __shared__ uint32_t s_state[kRegion];  // [z + 1][y + 1][x + 1]
  __shared__ uint32_t s_lab[kRegion];
  __shared__ TileShared s_tile;
  const uint32_t n = a.tiles.counters[2 * slot];
  if (n == 0u) return;  // an empty round: one word read
  const unsigned t = threadIdx.x;
  const int cx = (int)(t % (unsigned)kGX), cy = (int)(t / (unsigned)kGX);
  const uint32_t cap = a.plateau_cap;
  const int at0 = (kLY + cy + 1) * kLX + (cx + 1);  // the column's voxel z = 0
  uint32_t *const mine = s_lab + at0;
  for (int tx, ty, tz; tile_take(a.tiles, n, slot, s_tile, tx, ty, tz);) {  // (its first barrier: the previous tile's last reads)
    ws_load_region(a, a.state, s_state, tx, ty, tz);
    ws_load_region(a, a.wlab, s_lab, tx, ty, tz);
    const int gx = tx * kGX + cx, gy = ty * kGY + cy;
    uint32_t pair[kGZ / 2];  // the column's own costs, two to a register; 0 outside the volume
#pragma unroll
    for (int z = 0; z < kGZ; z += 2) {
      uint32_t lo = 0u, hi = 0u;
      if (gx < a.X && gy < a.Y) {
        if (tz * kGZ + z < a.Z) lo = a.cost[ws_voxel(a, gx, gy, tz * kGZ + z)];
        if (tz * kGZ + z + 1 < a.Z) hi = a.cost[ws_voxel(a, gx, gy, tz * kGZ + z + 1)];
      }
      pair[z / 2] = lo | hi << 16;
    }
    __syncthreads();
    // The edges into the column's voxels, a bit per neighbour: bit (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1).  The states are final, so
    // this is done once per visit.  A voxel outside the volume holds kNone and has no edge: no interval below contains kNone.
    uint32_t edges[kGZ], w[kGZ];
    uint32_t any = 0u;
#pragma unroll
    for (int z = 0; z < kGZ; ++z) {
      asm volatile("" ::: "memory");  // a voxel's 26 loads at a time: left alone the compiler issues all eight voxels' loads first, 256 VGPRs
      const uint32_t *p = s_state + at0 + z * kPlane;
      const uint32_t sp = *p;
      const uint32_t c = (z & 1) ? pair[z / 2] >> 16 : pair[z / 2] & 0xFFFFu;
      // the states that step to sp: lo .. lo + span
      uint32_t lo, span;
      if (sp == c << 16) {
        lo = 0u;
        span = cap == 0u ? sp : sp - 1u;  // (cap == 0: (c, 0) steps to itself.  sp == 0 is a seed's voxel: `real` below)
      } else {
        const bool saturated = (sp & 0xFFFFu) == cap;
        lo = cap == 0u ? sp : sp - 1u;
        span = (saturated && cap != 0u) ? 1u : 0u;
      }
      const bool real = sp != kNone && sp != 0u;
      uint32_t e = 0u;
#pragma unroll
      for (int q = 0; q < 27; ++q) {
        const int dx = q % 3 - 1, dy = (q / 3) % 3 - 1, dz = q / 9 - 1;
        const int moved = (dx != 0) + (dy != 0) + (dz != 0);
        if (moved == 0 || (!CONN26 && moved != 1)) continue;
        const uint32_t sq = p[dz * kPlane + dy * kLX + dx];
        if (sq - lo <= span) e |= 1u << q;
      }
      edges[z] = real ? e : 0u;
      asm volatile("" : "+v"(edges[z]));  // (the word is made here, before the next voxel's loads)
      any |= edges[z];
      w[z] = mine[z * kPlane];
    }
    uint32_t lowered = 0u;  // bit z: this visit made w[z] smaller

    for (;;) {
      uint32_t changed = 0u;
      // The edge bits do not change in this loop, and the compiler would keep every test of one (26 per voxel) across it, more than
      // the registers hold.  The empty statement makes the words opaque once per sweep, so a test lives from its bit to its select.
#pragma unroll
      for (int z = 0; z < kGZ; ++z) asm volatile("" : "+v"(edges[z]));
      if (any) {
#pragma unroll
        for (int z = 0; z < kGZ; ++z) {
          asm volatile("" ::: "memory");  // (as above)
          const uint32_t *p = mine + z * kPlane;
          const uint32_t e = edges[z];
          uint32_t m = w[z];
#pragma unroll
          for (int q = 0; q < 27; ++q) {
            const int dx = q % 3 - 1, dy = (q / 3) % 3 - 1, dz = q / 9 - 1;
            const int moved = (dx != 0) + (dy != 0) + (dz != 0);
            if (moved == 0 || (!CONN26 && moved != 1)) continue;
            if (dx == 0 && dy == 0) continue;  // the column itself: below
            const uint32_t v = p[dz * kPlane + dy * kLX + dx];
            m = ws_min(m, (e >> q) & 1u ? v : kNone);
          }
          // the column's own neighbours, in registers, in the order of the sweep
          const uint32_t under = z > 0 ? w[z > 0 ? z - 1 : 0] : mine[-kPlane];
          m = ws_min(m, (e >> 4) & 1u ? under : kNone);
          if (m < w[z]) {
            w[z] = m;
            changed |= 1u << z;
          }
          asm volatile("" : "+v"(w[z]));  // (made here, before the next voxel's loads)
        }
#pragma unroll
        for (int z = kGZ - 1; z >= 0; --z) {
          const uint32_t over = z + 1 < kGZ ? w[z + 1 < kGZ ? z + 1 : 0] : mine[kGZ * kPlane];
          if (((edges[z] >> 22) & 1u) && over < w[z]) {
            w[z] = over;
            changed |= 1u << z;
          }
        }
      }
      lowered |= changed;
      if (!__syncthreads_or((int)changed)) break;  // (also the barrier between the reads above and the stores below)
#pragma unroll
      for (int z = 0; z < kGZ; ++z)
        if ((changed >> z) & 1u) mine[z * kPlane] = w[z];
      __syncthreads();
    }

    // the owner's stores (a lowered voxel is reached, so inside the volume)
#pragma unroll
    for (int z = 0; z < kGZ; ++z)
      if ((lowered >> z) & 1u) ws_store(a.wlab + ws_voxel(a, gx, gy, tz * kGZ + z), w[z]);
    // round 1 counts every label the tile holds as lowered
    uint32_t fresh = lowered;
    if (round == 1u) {
#pragma unroll
      for (int z = 0; z < kGZ; ++z) fresh |= w[z] != kNone ? 1u << z : 0u;
    }
    const bool at_x[3] = {cx == 0, true, cx == kGX - 1}, at_y[3] = {cy == 0, true, cy == kGY - 1};
    const bool at_z[3] = {(fresh & 1u) != 0u, true, ((fresh >> (kGZ - 1)) & 1u) != 0u};
    tile_wake<CONN26>(a.tiles, round, s_tile, tx, ty, tz, fresh != 0u, at_x, at_y, at_z);
  }
}

// the caller's maps from the two arrays, and the call's result: k_geo_finish's shape
__global__ __launch_bounds__(256) void k_ws_finish(const WsArgs a) {
  const size_t total = (size_t)a.X * (size_t)a.Y * (size_t)a.Z;
  unsigned long long reached = 0ull;
  uint32_t max_level = 0u;
  for (size_t id = (size_t)blockIdx.x * 256u + threadIdx.x; id < total; id += (size_t)gridDim.x * 256u) {
    const uint32_t state = a.state[id];
    const bool is_reached = state != kNone;
    if (a.level) a.level[id] = state;
    if (a.labels) a.labels[id] = is_reached ? a.wlab[id] + 1u : 0u;
    if (is_reached) {
      ++reached;
      max_level = max(max_level, state >> 16);
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    reached += __shfl_xor(reached, off);
    max_level = max(max_level, (uint32_t)__shfl_xor((int)max_level, off));
  }
  __shared__ unsigned long long part_reached[4];
  __shared__ uint32_t part_max[4];
  const unsigned wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0u) {
    part_reached[wave] = reached;
    part_max[wave] = max_level;
  }
  __syncthreads();
  if (threadIdx.x != 0u) return;
  for (int w = 1; w < 4; ++w) {
    reached += part_reached[w];
    max_level = max(max_level, part_max[w]);
  }
  if (reached == 0ull) return;
  atomicAdd(&a.result->reached, reached);
  atomicMax(&a.result->max_level, max_level);
}

hipError_t launch_ws_init(const WsArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_ws_init, dim3(blocks_for((size_t)a.X * (size_t)a.Y * (size_t)a.Z)), dim3(256), 0, s, a);
  if (a.n_seeds != 0u) hipLaunchKernelGGL(k_ws_seeds, dim3(blocks_for(a.n_seeds)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_ws_level_round(const WsArgs &a, uint32_t round, int slot, hipStream_t s) {
  // 13 KB of LDS a block: the grid is the geodesic's, five blocks per CU
  return launch_tile_round(a.conn26 ? k_ws_level_round<true> : k_ws_level_round<false>, 1280u, a, round, slot, s);
}

hipError_t launch_ws_label_round(const WsArgs &a, uint32_t round, int slot, hipStream_t s) {
  return launch_tile_round(a.conn26 ? k_ws_label_round<true> : k_ws_label_round<false>, 1280u, a, round, slot, s);
}

hipError_t launch_ws_finish(const WsArgs &a, hipStream_t s) {
  const unsigned need = blocks_for((size_t)a.X * (size_t)a.Y * (size_t)a.Z), grid = need < 2048u ? need : 2048u;
  hipLaunchKernelGGL(k_ws_finish, dim3(grid), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace clvr
