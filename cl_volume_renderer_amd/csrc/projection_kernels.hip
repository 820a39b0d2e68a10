// projection_kernels.hip -- maximum / minimum / mean intensity projections of the caller's S16 image (clwh_render_projection).
//
// The contract (include/clwh.h) is exact so that it can be tested bit for bit: sample k of a pixel's ray sits at t_k = (float)k * h,
// p_k = o + d * t_k (per component one multiply, then one add; the library is built without contraction), and is KEPT iff
// t_near <= t_k <= t_far and 0 <= p_k.c < dim_c on all three axes; its value is the voxel at floor(p_k).
//
// Why the kernels may bound loops by boxes: float multiply and add are monotone, so each coordinate of p_k is monotone in k (and t_k
// too).  Every condition of "kept" therefore switches at most once along the ray, and the kept samples of a ray form ONE contiguous
// range of k; so do the kept samples inside any axis-aligned box, such as an 8^3 brick, and once the march has left a brick it never
// comes back to it.  Box intersections in float only give a starting guess for a search; the exact per-sample test decides every
// boundary (first_false below), so the sample set is the dense loop's whatever the guess.
//
//   k_proj_repack            the caller's image -> brick order (packed_volume.hpp inner_index: one 4^3 sub-brick of int16 = one 128-byte
//                            line) + a {min, max} pair per 8^3 brick over its real voxels
//   k_projection<MODE, SKIP> one wave per 8x8 pixel tile, tiles in XCD-contiguous order (as k_primary); each lane walks its ray's kept
//                            range brick by brick.  SKIP (MAX / MIN without CLWH_PROJ_DENSE): a brick whose table entry cannot beat the
//                            running extreme -- max <= best for MAX, min >= best for MIN -- is stepped over without reading it.  A tie
//                            cannot move t_extreme (the first sample that attains the extreme wins and the walk runs front to back), so
//                            the result is bit-identical to the dense walk.
#include "render_device.hpp"

namespace clvr {

// ------------------------------------------------------------------------------------------------
// k_proj_repack: a block turns a 64 x 8 x 8 box of the caller's x-fastest image (eight bricks side by side, whole 128-byte lines of each
// row) into brick order.  The box is read once with coalesced 16-byte loads into LDS (the staging of k_repack, render_kernels.hip); every
// wave then writes whole sub-bricks (64 lanes x 2 bytes = one line) and takes their minimum and maximum with the DPP wave minimum.
constexpr int kProjRepackX = 64;
__global__ __launch_bounds__(256) void k_proj_repack(const ProjRepackArgs a) {
  __shared__ __attribute__((aligned(16))) int16_t s_val[8][8][kProjRepackX];  // [z][y][x - x0]
  __shared__ uint32_t s_lo[8][8], s_hi[8][8];                                 // [brick of the block][sub-brick]: wave-minimum keys
  const int x0 = (int)blockIdx.x * kProjRepackX, y0 = (int)blockIdx.y * 8, z0 = (int)blockIdx.z * 8;
  const unsigned tid = threadIdx.x;
  if ((a.X & 7) == 0 && (reinterpret_cast<uintptr_t>(a.volume) & 15u) == 0u) {
    // rows of a multiple of 8 voxels: every 16-byte piece lies wholly inside or wholly outside the row
    for (unsigned i = tid; i < 8u * 8u * (kProjRepackX / 8); i += 256u) {
      const unsigned c = i & 7u, ry = (i >> 3) & 7u, rz = i >> 6;
      const int x = x0 + 8 * (int)c, y = y0 + (int)ry, z = z0 + (int)rz;
      uint4 v = uint4{0u, 0u, 0u, 0u};
      if (x < a.X && y < a.Y && z < a.Z) v = *reinterpret_cast<const uint4 *>(a.volume + ((size_t)z * (size_t)a.Y + (size_t)y) * (size_t)a.X + (size_t)x);
      *reinterpret_cast<uint4 *>(&s_val[rz][ry][8u * c]) = v;
    }
  } else {
    for (unsigned i = tid; i < 8u * 8u * kProjRepackX; i += 256u) {
      const unsigned rx = i & (kProjRepackX - 1u), ry = (i >> 6) & 7u, rz = i >> 9;
      const int x = x0 + (int)rx, y = y0 + (int)ry, z = z0 + (int)rz;
      int16_t v = 0;
      if (x < a.X && y < a.Y && z < a.Z) v = a.volume[((size_t)z * (size_t)a.Y + (size_t)y) * (size_t)a.X + (size_t)x];
      s_val[rz][ry][rx] = v;
    }
  }
  __syncthreads();
  const unsigned wave = tid >> 6, lane = tid & 63u;
  const size_t brick_row = ((size_t)blockIdx.z * (size_t)a.NBY + (size_t)blockIdx.y) * (size_t)a.NBX;
  for (unsigned half = 0u; half < 2u; ++half) {  // a wave writes the sub-bricks `wave` and `wave + 4` of each brick
    const unsigned sub = wave + 4u * half;
    unsigned ix, iy, iz;
    VolumePacked::inner_coords(sub * 64u + lane, ix, iy, iz);
    const int y = y0 + (int)iy, z = z0 + (int)iz;
    for (unsigned bq = 0u; bq < (unsigned)(kProjRepackX / 8); ++bq) {
      const int bx = (int)blockIdx.x * (kProjRepackX / 8) + (int)bq;
      if (bx >= a.NBX) break;  // (uniform over the block: wave_min_u32 needs every lane)
      const int lx = (int)(bq * 8u + ix);
      const bool real = x0 + lx < a.X && y < a.Y && z < a.Z;
      const int v = real ? (int)s_val[iz][iy][lx] : 0;
      a.bricks[((brick_row + (size_t)bx) << 9) + sub * 64u + lane] = (int16_t)v;
      // minimum and maximum as unsigned minima of v + 32768 and 32767 - v; padding voxels take no part
      const uint32_t lo = wave_min_u32(real ? (uint32_t)(v + 32768) : 0xFFFFFFFFu);
      const uint32_t hi = wave_min_u32(real ? (uint32_t)(32767 - v) : 0xFFFFFFFFu);
      if (lane == 0u) {
        s_lo[bq][sub] = lo;
        s_hi[bq][sub] = hi;
      }
    }
  }
  __syncthreads();
  if (tid < (unsigned)(kProjRepackX / 8)) {
    const int bx = (int)blockIdx.x * (kProjRepackX / 8) + (int)tid;
    if (bx < a.NBX) {  // every brick of the grid holds at least one real voxel
      uint32_t lo = 0xFFFFFFFFu, hi = 0xFFFFFFFFu;
      for (int s = 0; s < 8; ++s) {
        lo = s_lo[tid][s] < lo ? s_lo[tid][s] : lo;
        hi = s_hi[tid][s] < hi ? s_hi[tid][s] : hi;
      }
      const int vmin = (int)lo - 32768, vmax = 32767 - (int)hi;
      a.table[brick_row + (size_t)bx] = (uint32_t)(uint16_t)vmin | ((uint32_t)(uint16_t)vmax << 16);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// the exact sample test
struct ProjRay {
  f3 o, d;
  float h, t_near, t_far;
  float dx, dy, dz;  // volume dims
};

__device__ __forceinline__ f3 proj_sample(const ProjRay &r, int k, float &t) {
  t = (float)k * r.h;
  return f3{r.o.x + r.d.x * t, r.o.y + r.d.y * t, r.o.z + r.d.z * t};
}
// "kept" split into the conditions that can only switch from false to true as k grows (rising) and those that can only switch from
// true to false (falling): kept(k) = rising(k) && falling(k), so the kept range is [first rising k, last falling k].  An axis the ray
// does not move along (d.c == +-0, or NaN) keeps p.c == o.c while t is finite: its test is falling (an infinite t makes it NaN).
__device__ __forceinline__ bool axis_rising(float p, float d, float dim) { return d > 0.0f ? p >= 0.0f : (d < 0.0f ? p < dim : true); }
__device__ __forceinline__ bool axis_falling(float p, float d, float dim) {
  return d > 0.0f ? p < dim : (d < 0.0f ? p >= 0.0f : (p >= 0.0f && p < dim));
}
__device__ __forceinline__ bool proj_rising(const ProjRay &r, int k) {
  float t;
  const f3 p = proj_sample(r, k, t);
  return t >= r.t_near && axis_rising(p.x, r.d.x, r.dx) && axis_rising(p.y, r.d.y, r.dy) && axis_rising(p.z, r.d.z, r.dz);
}
__device__ __forceinline__ bool proj_falling(const ProjRay &r, int k) {
  float t;
  const f3 p = proj_sample(r, k, t);
  return t <= r.t_far && axis_falling(p.x, r.d.x, r.dx) && axis_falling(p.y, r.d.y, r.dy) && axis_falling(p.z, r.d.z, r.dz);
}

// The smallest k in (lo, hi] with pred(k) false, given pred(lo) true and pred true-then-false on [lo, hi]; hi + 1 if there is none.
// `guess` (a float estimate of the answer) only decides where the search starts: gallop away from it, then bisect.
template <class Pred>
__device__ __forceinline__ int first_false(int lo, int hi, int guess, Pred pred) {
  int f = hi + 1;  // pred is false at f, or f lies past the range
  const int g = guess <= lo ? lo + 1 : (guess > f ? f : guess);
  if (g < f && pred(g)) {
    lo = g;
    for (int s = 1; lo + s < f; s <<= 1) {
      if (!pred(lo + s)) { f = lo + s; break; }
      lo += s;
    }
  } else {
    f = g;
    for (int s = 1; f - s > lo; s <<= 1) {
      if (pred(f - s)) { lo = f - s; break; }
      f -= s;
    }
  }
  while (f - lo > 1) {
    const int m = lo + ((f - lo) >> 1);
    if (pred(m)) lo = m; else f = m;
  }
  return f;
}

// a float sample index as a search start in [0, cap] (NaN -> 0)
__device__ __forceinline__ int index_guess(float kf, int cap) { return (int)fminf(fmaxf(kf, 0.0f), (float)cap); }

// the ray's kept range [ka, kb]; false if it is empty
__device__ __forceinline__ bool proj_kept_range(const ProjRay &r, int k_cap, int &ka, int &kb) {
  float te = r.t_near, tx = r.t_far;  // slab estimate of the entry and exit
  const float dv[3] = {r.d.x, r.d.y, r.d.z}, ov[3] = {r.o.x, r.o.y, r.o.z}, dim[3] = {r.dx, r.dy, r.dz};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (dv[c] != 0.0f) {
      const float a = (0.0f - ov[c]) / dv[c], b = (dim[c] - ov[c]) / dv[c];
      te = fmaxf(te, fminf(a, b));
      tx = fminf(tx, fmaxf(a, b));
    }
  }
  if (!proj_falling(r, 0)) return false;
  kb = first_false(0, k_cap - 1, index_guess(floorf(tx / r.h) + 1.0f, k_cap), [&](int k) { return proj_falling(r, k); }) - 1;
  ka = proj_rising(r, 0) ? 0 : first_false(0, kb, index_guess(ceilf(te / r.h), k_cap), [&](int k) { return !proj_rising(r, k); });
  return ka <= kb;
}

enum : int { PROJ_MAX = CLWH_PROJ_MAX, PROJ_MIN = CLWH_PROJ_MIN, PROJ_MEAN = CLWH_PROJ_MEAN };

template <int MODE, bool SKIP>
__global__ __launch_bounds__(64) void k_projection(const ProjArgs a) {
  const uint32_t slot = xcd_contiguous_slot(blockIdx.x, (uint32_t)a.num_tiles);
  const uint32_t tx = slot % (uint32_t)a.tiles_x, ty = slot / (uint32_t)a.tiles_x;
  const uint32_t lane = threadIdx.x;
  const uint32_t x = tx * 8u + (lane & 7u), y = ty * 8u + (lane >> 3);

  const f3 cam_o = f3{a.cam_pos[0], a.cam_pos[1], a.cam_pos[2]};
  const f3 cam_d = f3{a.cam_dir[0], a.cam_dir[1], a.cam_dir[2]};
  const Ray ray = generate_ray(cam_o, cam_d, (int)x, (int)y, a.frame_w, a.frame_h);
  const ProjRay r{ray.origin, ray.direction, a.step, a.t_near, a.t_far, (float)a.X, (float)a.Y, (float)a.Z};

  constexpr int kNone = MODE == PROJ_MAX ? -32769 : 32768;  // beyond int16: no sample yet
  int best = kNone;
  float best_t = __builtin_nanf("");
  long long sum = 0;
  int count = 0;
  int k, kb;
  if (proj_kept_range(r, a.k_cap, k, kb)) {
    while (k <= kb) {  // one brick per iteration, front to back
      float t;
      const f3 p = proj_sample(r, k, t);  // kept: 0 <= p < dim, so the conversions are floors
      const unsigned bx = (unsigned)(int)p.x >> 3, by = (unsigned)(int)p.y >> 3, bz = (unsigned)(int)p.z >> 3;
      const size_t brick = ((size_t)bz * (size_t)a.NBY + (size_t)by) * (size_t)a.NBX + (size_t)bx;
      // where the ray leaves the brick's box (the guess), then the exact first sample outside it
      float tb = INFINITY;
      if (r.d.x != 0.0f) tb = fminf(tb, ((float)((bx + (r.d.x > 0.0f ? 1u : 0u)) * 8u) - r.o.x) / r.d.x);
      if (r.d.y != 0.0f) tb = fminf(tb, ((float)((by + (r.d.y > 0.0f ? 1u : 0u)) * 8u) - r.o.y) / r.d.y);
      if (r.d.z != 0.0f) tb = fminf(tb, ((float)((bz + (r.d.z > 0.0f ? 1u : 0u)) * 8u) - r.o.z) / r.d.z);
      const int k_end = first_false(k, kb, index_guess(floorf(tb / r.h) + 1.0f, a.k_cap), [&](int j) {
        float tj;
        const f3 q = proj_sample(r, j, tj);
        return ((unsigned)(int)q.x >> 3) == bx && ((unsigned)(int)q.y >> 3) == by && ((unsigned)(int)q.z >> 3) == bz;
      });
      bool skip = false;
      if constexpr (SKIP) {
        const uint32_t mm = a.table[brick];
        skip = MODE == PROJ_MAX ? (int)(int16_t)(mm >> 16) <= best : (int)(int16_t)(mm & 0xFFFFu) >= best;
      }
      if (!skip) {
        const int16_t *__restrict__ b = a.bricks + (brick << 9);
        for (int j = k; j < k_end; ++j) {
          float tj;
          const f3 q = proj_sample(r, j, tj);
          const int v = b[VolumePacked::inner_index((unsigned)(int)q.x, (unsigned)(int)q.y, (unsigned)(int)q.z)];
          if constexpr (MODE == PROJ_MEAN) {
            sum += v;
            count += 1;
          } else if (MODE == PROJ_MAX ? v > best : v < best) {  // strict: the first sample attaining the extreme keeps its t
            best = v;
            best_t = tj;
          }
        }
      }
      k = k_end;
    }
  }
  float value;
  if constexpr (MODE == PROJ_MEAN) {
    value = count > 0 ? (float)((double)sum / (double)count) : __builtin_nanf("");
    best_t = __builtin_nanf("");
  } else {
    value = best != kNone ? (float)best : __builtin_nanf("");
  }
  uint32_t px = 0u;  // no kept sample: (0, 0, 0, 0)
  if (value == value) {
    const float u = ((value - a.window_center) / a.window_width + 0.5f) * 255.0f + 0.5f;
    const uint32_t grey = (uint32_t)(int)fminf(fmaxf(u, 0.0f), 255.0f);
    px = grey * 0x010101u | 0xFF000000u;
  }
  a.frame[(size_t)y * (size_t)a.frame_w + x] = px;
  const size_t o = (size_t)y * (size_t)a.launch_w + x;
  if (a.values) a.values[o] = value;
  if (a.t_extreme) a.t_extreme[o] = best_t;
}

hipError_t launch_proj_repack(const ProjRepackArgs &a, hipStream_t s) {
  const dim3 grid((unsigned)((a.X + kProjRepackX - 1) / kProjRepackX), (unsigned)a.NBY, (unsigned)a.NBZ);
  hipLaunchKernelGGL(k_proj_repack, grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_projection(const ProjArgs &a, int mode, bool dense, hipStream_t s) {
  const dim3 grid((unsigned)a.num_tiles), block(64);
  if (mode == PROJ_MEAN)
    hipLaunchKernelGGL((k_projection<PROJ_MEAN, false>), grid, block, 0, s, a);
  else if (mode == PROJ_MAX && dense)
    hipLaunchKernelGGL((k_projection<PROJ_MAX, false>), grid, block, 0, s, a);
  else if (mode == PROJ_MAX)
    hipLaunchKernelGGL((k_projection<PROJ_MAX, true>), grid, block, 0, s, a);
  else if (dense)
    hipLaunchKernelGGL((k_projection<PROJ_MIN, false>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((k_projection<PROJ_MIN, true>), grid, block, 0, s, a);
  return hipGetLastError();
}

}  // namespace clvr
