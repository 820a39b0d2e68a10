// grow_kernels.hip -- seeded region growing (clwh_segment_grow) and masked volumes (clwh_volume_apply_mask), gfx950.  The grown set R is
// the least fixpoint of  R = seeds | (dilate(R) & A)  over one bit per voxel, A the admissible image (value window and box), dilate the
// 6 face neighbours or the 26 of the box.  The search is the SDF build's (sdf_bits_kernels.hip): bit rows, tiles worked from a list,
// stamps that wake a tile's neighbours -- with two differences.  The dilation is masked by A, and there is no layer cap: a tile is
// iterated to its LOCAL fixpoint in LDS before anything returns to memory, so a round moves the front by whole tiles, not by one voxel,
// and the number of rounds follows the number of tile faces the component's paths cross, not its geodesic depth.
//   Tile = 64 x 16 x 16 voxels = one 64-bit word of 256 rows; a 256-thread block owns a tile, a thread one row.
//   Only the owner stores to a tile's words, and a tile is listed once per round.  A halo word read while its owner stores to it in the
//   same round is the old or the new word (or, torn, a mix): every one of them is a subset of the final set, since bits are only ever
//   set; and an owner whose boundary changed stamps the reader for the next round, which starts behind a kernel boundary.  So every
//   stored set lies between the seeds and the least fixpoint, and when a round lists no tile every tile is at its local fixpoint with
//   the halos it would read now: the global fixpoint.  No result depends on the order of blocks, and no block waits for another.
#include "tile_work_device.hpp"

namespace clvr {

namespace {

typedef unsigned long long u64;
constexpr int kTile = 16;  // rows of a tile along y and along z

__device__ __forceinline__ uint32_t grow_tile_of(const GrowArgs &a, int x, int y, int z) {
  return (uint32_t)(((z >> 4) * a.tiles.TY + (y >> 4)) * a.tiles.TX + (x >> 6));
}

}  // namespace

// A, and the mask's start: mask &= A (CLWH_GROW_FROM_MASK; a tile that keeps a bit is stamped for round 1) or mask = 0.  Rows of a
// multiple of 8 voxels: a lane owns one byte of both bit images (admissible_byte).
__global__ __launch_bounds__(256) void k_grow_admissible8(const GrowArgs a) {
  const size_t total = (size_t)a.W64 * 8u * (size_t)a.Y * (size_t)a.Z, id = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (id >= total) return;
  int x0, y, z;
  const uint32_t bits = admissible_byte(a, id, x0, y, z);
  reinterpret_cast<uint8_t *>(a.adm)[id] = (uint8_t)bits;
  uint8_t *mask = reinterpret_cast<uint8_t *>(a.mask);
  const uint32_t m = a.from_mask ? ((uint32_t)mask[id] & bits) : 0u;
  mask[id] = (uint8_t)m;
  if (m) a.tiles.stamps[grow_tile_of(a, x0, y, z)] = 1u;
}

// the same for any row length: a thread per voxel of the padded row, a wave per 64-bit word (admissible_voxel)
__global__ __launch_bounds__(256) void k_grow_admissible(const GrowArgs a) {
  const size_t total = (size_t)a.W64 * 64u * (size_t)a.Y * (size_t)a.Z, id = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (id >= total) return;  // (whole waves: `total` and a wave's first id are multiples of 64)
  int x, y, z;
  const u64 bits = __ballot(admissible_voxel(a, id, x, y, z));
  if ((threadIdx.x & 63u) == 0u) {
    const size_t w = id >> 6;
    a.adm[w] = bits;
    const u64 m = a.from_mask ? (a.mask[w] & bits) : 0ull;
    a.mask[w] = m;
    if (m) a.tiles.stamps[grow_tile_of(a, x, y, z)] = 1u;
  }
}

// the listed seeds (inside the volume: the host checked) that are admissible, OR-ed into the mask; their tiles are stamped for round 1
__global__ __launch_bounds__(256) void k_grow_seeds(const GrowArgs a) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.n_seeds) return;
  const int x = (int)a.seeds[3u * i], y = (int)a.seeds[3u * i + 1u], z = (int)a.seeds[3u * i + 2u];
  const size_t w = ((size_t)z * (size_t)a.Y + (size_t)y) * (size_t)a.W64 + (size_t)(x >> 6);
  const u64 bit = 1ull << (x & 63);
  if (a.adm[w] & bit) {
    atomicOr(&a.mask[w], bit);
    a.tiles.stamps[grow_tile_of(a, x, y, z)] = 1u;
  }
}

namespace {

// every admissible run of the word that holds a bit of r, whole: the fixpoint of r |= (r << 1 | r >> 1) & adm in six doubling steps
// per direction (a Kogge-Stone fill)
__device__ __forceinline__ u64 grow_fill_x(u64 r, u64 adm) {
  u64 g = r, p = adm;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    g |= p & (g << s);
    p &= p << s;
  }
  p = adm;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    g |= p & (g >> s);
    p &= p >> s;
  }
  return g;
}

struct GrowRow {
  u64 word;      // the row's word in this tile's column
  u64 from_x;    // the neighbouring words' nearest bits, moved to this word's bit 0 and bit 63
};
// row (ry, rz) of the tile's 18 x 18 region, -1 <= ry, rz <= 16; rows outside the volume are empty
__device__ __forceinline__ GrowRow grow_load_row(const GrowArgs &a, int tx, int ty, int tz, int ry, int rz) {
  GrowRow r{0ull, 0ull};
  const int gy = ty * kTile + ry, gz = tz * kTile + rz;
  if (gy < 0 || gy >= a.Y || gz < 0 || gz >= a.Z) return r;
  const u64 *row = a.mask + ((size_t)gz * (size_t)a.Y + (size_t)gy) * (size_t)a.W64;
  r.word = row[tx];
  if (tx > 0) r.from_x |= row[tx - 1] >> 63;
  if (tx + 1 < a.W64) r.from_x |= row[tx + 1] << 63;
  return r;
}
__device__ __forceinline__ u64 grow_dilate_x(const GrowRow &r) { return r.word | (r.word << 1) | (r.word >> 1) | r.from_x; }

}  // namespace

// One round: a persistent grid takes the listed tiles by ticket; see the head of the file and tile_work_device.hpp.
template <bool CONN26>
__global__ __launch_bounds__(256) void k_grow_round(const GrowArgs a, uint32_t round, int slot) {
  // 6: the region's rows of R; 26: the same dilated along x.  [rz + 1][ry + 1]
  __shared__ u64 lx[kTile + 2][kTile + 2];
  __shared__ u64 ly[kTile + 2][kTile];  // 26 only: lx dilated along y, [rz + 1][ry]
  __shared__ TileShared s_tile;
  const uint32_t n = a.tiles.counters[2 * slot];
  if (n == 0u) return;  // an empty round: one word read
  const unsigned t = threadIdx.x;
  const int cy = (int)(t & 15u), cz = (int)(t >> 4);
  for (int tx, ty, tz; tile_take(a.tiles, n, slot, s_tile, tx, ty, tz);) {
    // the core row of this thread, and the halo: 18 + 18 rows at rz = -1 and 16, 16 + 16 at ry = -1 and 16
    const int gy = ty * kTile + cy, gz = tz * kTile + cz;
    const bool exists = gy < a.Y && gz < a.Z;
    const size_t own = ((size_t)gz * (size_t)a.Y + (size_t)gy) * (size_t)a.W64 + (size_t)tx;
    GrowRow me = grow_load_row(a, tx, ty, tz, cy, cz);
    const u64 adm = exists ? a.adm[own] : 0ull;
    const u64 r0 = me.word;
    if (t < 68u) {
      int ry, rz;
      if (t < 36u) {
        rz = t < 18u ? -1 : kTile;
        ry = (int)(t % 18u) - 1;
      } else {
        ry = t < 52u ? -1 : kTile;
        rz = (int)((t - 36u) & 15u);
      }
      const GrowRow h = grow_load_row(a, tx, ty, tz, ry, rz);
      lx[rz + 1][ry + 1] = CONN26 ? grow_dilate_x(h) : h.word;
    }
    if (CONN26) {
      __syncthreads();
      if (t < 32u) {  // the y-dilated rows at rz = -1 and 16 never change
        const int rz = t < 16u ? 0 : kTile + 1, y = (int)(t & 15u);
        ly[rz][y] = lx[rz][y] | lx[rz][y + 1] | lx[rz][y + 2];
      }
    }

    u64 r = r0;
    for (;;) {
      u64 grown;
      if (CONN26) {  // the box dilation, separable: x, then y, then z, each over the stage before
        me.word = r;
        lx[cz + 1][cy + 1] = grow_dilate_x(me);
        __syncthreads();
        ly[cz + 1][cy] = lx[cz + 1][cy] | lx[cz + 1][cy + 1] | lx[cz + 1][cy + 2];
        __syncthreads();
        grown = ly[cz][cy] | ly[cz + 1][cy] | ly[cz + 2][cy];
      } else {
        lx[cz + 1][cy + 1] = r;
        __syncthreads();
        grown = (r << 1) | (r >> 1) | me.from_x | lx[cz + 1][cy] | lx[cz + 1][cy + 2] | lx[cz][cy + 1] | lx[cz + 2][cy + 1];
      }
      const u64 next = grow_fill_x(r | (grown & adm), adm);
      const int changed = next != r;
      r = next;
      if (!__syncthreads_or(changed)) break;  // (also the barrier between this iteration's reads and the next one's stores)
    }

    if (exists && r != r0) a.mask[own] = r;
    // the neighbouring tiles that a new voxel touches are woken; round 1 counts every voxel as new
    const u64 fresh = round == 1u ? r : (r & ~r0);
    const bool at_x[3] = {(fresh & 1ull) != 0ull, true, (fresh >> 63) != 0ull};
    const bool at_y[3] = {cy == 0, true, cy == kTile - 1}, at_z[3] = {cz == 0, true, cz == kTile - 1};
    tile_wake<CONN26>(a.tiles, round, s_tile, tx, ty, tz, fresh != 0ull, at_x, at_y, at_z);
  }
}

// count, sum, sum of squares, extremes and bounding box of V over the mask, in one pass: a lane takes bytes of the mask (8 voxels) in a
// grid-stride loop, a block reduces and adds its part with vector atomics.  All integer: the order does not matter.
template <bool ROWS8>
__global__ __launch_bounds__(256) void k_grow_reduce(const GrowArgs a) {
  const size_t bytes_per_row = (size_t)a.W64 * 8u, total = bytes_per_row * (size_t)a.Y * (size_t)a.Z;
  const uint8_t *mask = reinterpret_cast<const uint8_t *>(a.mask);
  u64 count = 0ull, sum_sq = 0ull;
  long long sum = 0;
  int vmin = 0x7fffffff, vmax = -0x7fffffff - 1;
  uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
  for (size_t id = (size_t)blockIdx.x * 256u + threadIdx.x; id < total; id += (size_t)gridDim.x * 256u) {
    const uint32_t m = mask[id];
    if (!m) continue;
    const size_t row = id / bytes_per_row;
    const uint32_t x0 = (uint32_t)(id - row * bytes_per_row) * 8u;
    const uint32_t z = (uint32_t)(row / (size_t)a.Y), y = (uint32_t)(row - (size_t)z * (size_t)a.Y);
    const int16_t *p = a.volume + row * (size_t)a.X + (size_t)x0;  // (set bits lie at x < X)
    int v[8];
    if (ROWS8) {
      load8(p, v);
    } else {
#pragma unroll
      for (int h = 0; h < 8; ++h) v[h] = ((m >> h) & 1u) ? (int)p[h] : 0;
    }
#pragma unroll
    for (int h = 0; h < 8; ++h) {
      if (!((m >> h) & 1u)) continue;
      ++count;
      sum += v[h];
      sum_sq += (u64)((long long)v[h] * (long long)v[h]);
      vmin = min(vmin, v[h]);
      vmax = max(vmax, v[h]);
    }
    lo[0] = min(lo[0], x0 + (uint32_t)(__ffs((int)m) - 1));
    hi[0] = max(hi[0], x0 + (uint32_t)(31 - __clz((int)m)));
    lo[1] = min(lo[1], y);
    hi[1] = max(hi[1], y);
    lo[2] = min(lo[2], z);
    hi[2] = max(hi[2], z);
  }
  for (int off = 32; off > 0; off >>= 1) {
    count += __shfl_xor(count, off);
    sum += __shfl_xor(sum, off);
    sum_sq += __shfl_xor(sum_sq, off);
    vmin = min(vmin, __shfl_xor(vmin, off));
    vmax = max(vmax, __shfl_xor(vmax, off));
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      lo[q] = min(lo[q], (uint32_t)__shfl_xor((int)lo[q], off));
      hi[q] = max(hi[q], (uint32_t)__shfl_xor((int)hi[q], off));
    }
  }
  __shared__ GrowDeviceResult part[4];
  const unsigned wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0u) {
    part[wave].count = count;
    part[wave].sum = (u64)sum;
    part[wave].sum_sq = sum_sq;
    part[wave].vmin = vmin;
    part[wave].vmax = vmax;
    for (int q = 0; q < 3; ++q) {
      part[wave].lo[q] = lo[q];
      part[wave].hi[q] = hi[q];
    }
  }
  __syncthreads();
  if (threadIdx.x != 0u) return;
  GrowDeviceResult s = part[0];
  for (int w = 1; w < 4; ++w) {
    s.count += part[w].count;
    s.sum += part[w].sum;
    s.sum_sq += part[w].sum_sq;
    s.vmin = min(s.vmin, part[w].vmin);
    s.vmax = max(s.vmax, part[w].vmax);
    for (int q = 0; q < 3; ++q) {
      s.lo[q] = min(s.lo[q], part[w].lo[q]);
      s.hi[q] = max(s.hi[q], part[w].hi[q]);
    }
  }
  if (s.count == 0ull) return;
  atomicAdd(&a.result->count, s.count);
  atomicAdd(&a.result->sum, s.sum);
  atomicAdd(&a.result->sum_sq, s.sum_sq);
  atomicMin(&a.result->vmin, s.vmin);
  atomicMax(&a.result->vmax, s.vmax);
  for (int q = 0; q < 3; ++q) {
    atomicMin(&a.result->lo[q], s.lo[q]);
    atomicMax(&a.result->hi[q], s.hi[q]);
  }
}

// out = (bit != invert) ? in : fill.  Rows of a multiple of 8 voxels at 16-byte aligned images: a lane takes one byte of the mask, one
// 16-byte load and one 16-byte store; in place, a lane reads its voxels before it writes them and nobody else's
__global__ __launch_bounds__(256) void k_apply_mask8(const int16_t *in, int16_t *out, const uint8_t *__restrict__ mask, int32_t X, size_t rows,
                                                      int32_t W64, uint32_t fill, uint32_t invert) {
  const size_t units = (size_t)(X / 8), id = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (id >= units * rows) return;
  const size_t row = id / units, unit = id - row * units;
  const uint32_t keep = (uint32_t)mask[row * (size_t)W64 * 8u + unit] ^ (invert ? 0xFFu : 0u);
  const uint4 q = *reinterpret_cast<const uint4 *>(in + id * 8u);
  uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t sel = (((keep >> (2 * k)) & 1u) ? 0x0000FFFFu : 0u) | (((keep >> (2 * k + 1)) & 1u) ? 0xFFFF0000u : 0u);
    w[k] = (w[k] & sel) | ((fill * 0x00010001u) & ~sel);
  }
  *reinterpret_cast<uint4 *>(out + id * 8u) = uint4{w[0], w[1], w[2], w[3]};
}
// any row length or alignment: a lane per voxel
__global__ __launch_bounds__(256) void k_apply_mask(const int16_t *in, int16_t *out, const uint8_t *__restrict__ mask, int32_t X, size_t rows,
                                                     int32_t W64, uint32_t fill, uint32_t invert) {
  const size_t id = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (id >= (size_t)X * rows) return;
  const size_t row = id / (size_t)X, x = id - row * (size_t)X;
  const uint32_t bit = ((uint32_t)mask[row * (size_t)W64 * 8u + (x >> 3)] >> (x & 7u)) & 1u;
  out[id] = bit != invert ? in[id] : (int16_t)(uint16_t)fill;
}

hipError_t launch_grow_admissible(const GrowArgs &a, hipStream_t s) {
  const size_t rows = (size_t)a.Y * (size_t)a.Z;
  if (rows_of_8(a.volume, a.X)) hipLaunchKernelGGL(k_grow_admissible8, dim3(blocks_for(rows * (size_t)a.W64 * 8u)), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(k_grow_admissible, dim3(blocks_for(rows * (size_t)a.W64 * 64u)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_grow_seeds(const GrowArgs &a, hipStream_t s) {
  if (a.n_seeds == 0u) return hipSuccess;
  hipLaunchKernelGGL(k_grow_seeds, dim3(blocks_for(a.n_seeds)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_grow_round(const GrowArgs &a, uint32_t round, int slot, hipStream_t s) {
  // four blocks per CU hold the 4.8 KB of LDS and 256 threads each with room to spare
  return launch_tile_round(a.conn26 ? k_grow_round<true> : k_grow_round<false>, 1024u, a, round, slot, s);
}

hipError_t launch_grow_reduce(const GrowArgs &a, hipStream_t s) {
  const size_t bytes = (size_t)a.Y * (size_t)a.Z * (size_t)a.W64 * 8u;
  const unsigned need = blocks_for(bytes), grid = need < 2048u ? need : 2048u;
  hipLaunchKernelGGL(rows_of_8(a.volume, a.X) ? k_grow_reduce<true> : k_grow_reduce<false>, dim3(grid), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_apply_mask(const int16_t *in, int16_t *out, const unsigned long long *mask, int32_t X, int32_t Y, int32_t Z, int32_t W64,
                             int32_t fill, int32_t invert, hipStream_t s) {
  const size_t rows = (size_t)Y * (size_t)Z;
  const uint32_t f = (uint32_t)(uint16_t)(int16_t)fill, inv = invert ? 1u : 0u;
  if (rows_of_8(in, X) && rows_of_8(out, X))
    hipLaunchKernelGGL(k_apply_mask8, dim3(blocks_for(rows * (size_t)(X / 8))), dim3(256), 0, s, in, out, (const uint8_t *)mask, X, rows, W64, f, inv);
  else
    hipLaunchKernelGGL(k_apply_mask, dim3(blocks_for(rows * (size_t)X)), dim3(256), 0, s, in, out, (const uint8_t *)mask, X, rows, W64, f, inv);
  return hipGetLastError();
}

}  // namespace clvr
