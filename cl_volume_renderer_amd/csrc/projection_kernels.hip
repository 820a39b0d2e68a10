// projection_kernels.hip -- maximum / minimum / mean intensity projections of the caller's S16 image (clwh_render_projection).
//
// The pixel mapping, the exact sample set of a ray and the brick walk over it are in view_device.hpp, shared by all the views.
//
//   k_proj_repack            the caller's image -> brick order (packed_volume.hpp inner_index: one 4^3 sub-brick of int16 = one 128-byte
//                            line) + a {min, max} pair per 8^3 brick over its real voxels
//   k_projection<MODE, SKIP> one wave per 8x8 pixel tile (view_pixel); each lane walks its ray's kept range brick by brick
//                            (walk_bricks).  SKIP (MAX / MIN without CLWH_PROJ_DENSE): a brick whose table entry cannot beat the
//                            running extreme -- max <= best for MAX, min >= best for MIN -- is stepped over without reading it.  A tie
//                            cannot move t_extreme (the first sample that attains the extreme wins and the walk runs front to back), so
//                            the result is bit-identical to the dense walk.
#include "view_device.hpp"

namespace clvr {

// ------------------------------------------------------------------------------------------------
// k_proj_repack: a block turns a 64 x 8 x 8 box of the caller's x-fastest image (eight bricks side by side, whole 128-byte lines of each
// row) into brick order.  The box is read once with coalesced 16-byte loads into LDS (the staging of k_repack, scene_kernels.hip); every
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
      a.table[brick_row + (size_t)bx] = pack_min_max((int)lo - 32768, 32767 - (int)hi);
    }
  }
}

enum : int { PROJ_MAX = CLWH_PROJ_MAX, PROJ_MIN = CLWH_PROJ_MIN, PROJ_MEAN = CLWH_PROJ_MEAN };

template <int MODE, bool SKIP>
__global__ __launch_bounds__(64) void k_projection(const ProjArgs a) {
  uint32_t x, y;
  view_pixel(a.fr, x, y);
  const ProjRay r = camera_ray(a.cam, a.vol, a.fr, x, y);

  constexpr int kNone = MODE == PROJ_MAX ? -32769 : 32768;  // beyond int16: no sample yet
  int best = kNone;
  float best_t = __builtin_nanf("");
  long long sum = 0;
  int count = 0;
  int k, kb;
  if (proj_kept_range(r, a.cam.k_cap, k, kb)) {
    walk_bricks(
        r, a.vol, k, kb, a.cam.k_cap, NeverSkip{},
        [&](size_t brick) {
          if constexpr (SKIP) {
            const uint32_t mm = a.vol.table[brick];
            return MODE == PROJ_MAX ? table_max(mm) <= best : table_min(mm) >= best;
          } else {
            return false;
          }
        },
        [&](size_t brick, int k0, int k_end) {
          const int16_t *__restrict__ b = a.vol.bricks + (brick << 9);
          for (int j = k0; j < k_end; ++j) {
            float tj;
            const f3 q = proj_sample(r, j, tj);
            const int v = b[VolumePacked::inner_index((unsigned)(int)q.x, (unsigned)(int)q.y, (unsigned)(int)q.z)];
            if constexpr (MODE == PROJ_MEAN) {
              sum += v;
              count += 1;
            } else {
              const bool better = MODE == PROJ_MAX ? v > best : v < best;  // strict: the first sample attaining the extreme keeps its t
              best_t = better ? tj : best_t;
              best = better ? v : best;
            }
          }
          return false;
        });
  }
  float value;
  if constexpr (MODE == PROJ_MEAN) {
    value = count > 0 ? (float)((double)sum / (double)count) : __builtin_nanf("");
    best_t = __builtin_nanf("");
  } else {
    value = best != kNone ? (float)best : __builtin_nanf("");
  }
  const size_t o = store_frame(a.fr, x, y, window_grey(value, a.window_center, a.window_width));
  store_optional(a.values, o, value);
  store_optional(a.t_extreme, o, best_t);
}

hipError_t launch_proj_repack(const ProjRepackArgs &a, hipStream_t s) {
  const dim3 grid((unsigned)((a.X + kProjRepackX - 1) / kProjRepackX), (unsigned)a.NBY, (unsigned)a.NBZ);
  hipLaunchKernelGGL(k_proj_repack, grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_projection(const ProjArgs &a, int mode, bool dense, hipStream_t s) {
  const dim3 grid((unsigned)a.fr.num_tiles), block(64);
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
