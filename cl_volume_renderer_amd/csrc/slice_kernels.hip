// slice_kernels.hip -- oblique slices and thick slabs of the volume's TRILINEAR field (clwh_render_slice): multi-planar reformatting.
// Pixel (x, y) of the region owns a ray of its own, o = (origin + x * du) + y * dv, all rays parallel along `normal`; sample k sits at
// o + normal * ((float)k * step), 0 <= k < slab_samples.  The kept-sample rule, the bricked int16 copy of the volume and the brick walk
// are the projections' (projection_device.hpp with t_near = 0 and no t_far); a sample's value is the isosurface's fixed-point field S
// (trilinear_device.hpp), so MAX / MIN compare exact integers and MEAN sums them in int64.
//
//   k_slice<MODE, SKIP>  one wave per 8x8 pixel tile, tiles in XCD-contiguous order (as k_projection), one lane per pixel.  A thin
//                        slice (slab_samples == 1) tests sample 0 and reads it: no range search.  A slab walks the lane's kept range
//                        brick by brick.  SKIP (MAX / MIN without CLWH_SLICE_DENSE): a brick whose dilated maximum cannot beat the
//                        running extreme -- dmax * 2^24 <= best for MAX, dmin * 2^24 >= best for MIN -- is stepped over unread, and
//                        with SliceArgs::use_coarse a whole cell of 4^3 bricks by one exit search.  Every sample whose voxel lies in
//                        the brick has dmin * 2^24 <= S <= dmax * 2^24 (the isosurface's proof), and a sample that only equals the
//                        extreme moves neither `best` nor k_ext (the first sample that attains it wins, and the walk runs in
//                        increasing k): the bytes are the dense walk's.
#include <climits>

#include "trilinear_device.hpp"

namespace clvr {

enum : int { SLICE_MAX = CLWH_SLICE_MAX, SLICE_MIN = CLWH_SLICE_MIN, SLICE_MEAN = CLWH_SLICE_MEAN };

template <int MODE, bool SKIP>
__global__ __launch_bounds__(64) void k_slice(const SliceArgs a) {
  const uint32_t slot = xcd_contiguous_slot(blockIdx.x, (uint32_t)a.num_tiles);
  const uint32_t tx = slot % (uint32_t)a.tiles_x, ty = slot / (uint32_t)a.tiles_x;
  const uint32_t lane = threadIdx.x;
  const uint32_t x = tx * 8u + (lane & 7u), y = ty * 8u + (lane >> 3);

  const float fx = (float)x, fy = (float)y;
  const f3 o = f3{(a.origin[0] + fx * a.du[0]) + fy * a.dv[0], (a.origin[1] + fx * a.du[1]) + fy * a.dv[1],
                  (a.origin[2] + fx * a.du[2]) + fy * a.dv[2]};
  const ProjRay r{o, f3{a.normal[0], a.normal[1], a.normal[2]}, a.step, 0.0f, INFINITY, (float)a.X, (float)a.Y, (float)a.Z};
  const FieldVolume fv{a.bricks, a.X, a.Y, a.Z, a.NBX, a.NBY};

  constexpr long long kNone = MODE == SLICE_MAX ? LLONG_MIN : LLONG_MAX;  // beyond |S| <= 2^39: no sample yet, and no brick is skipped
  long long best = kNone, sum = 0;
  int k_ext = 0, count = 0;
  if (a.slab_samples == 1) {  // a thin slice: sample 0 alone
    float t;
    const f3 p = proj_sample(r, 0, t);
    if (p.x >= 0.0f && p.x < r.dx && p.y >= 0.0f && p.y < r.dy && p.z >= 0.0f && p.z < r.dz) {
      best = sum = iso_field(fv, p);
      count = 1;
    }
  } else {
    int k, kb;
    if (proj_kept_range(r, a.slab_samples, k, kb)) {
      while (k <= kb) {  // one brick per iteration, in increasing k
        float t;
        const f3 p = proj_sample(r, k, t);  // kept: 0 <= p < dim, so the conversions are floors
        const unsigned bx = (unsigned)(int)p.x >> 3, by = (unsigned)(int)p.y >> 3, bz = (unsigned)(int)p.z >> 3;
        if constexpr (SKIP) {
          if (a.use_coarse) {  // a whole cell of 4^3 bricks that cannot change the extreme: one exit search
            const uint32_t cm = a.coarse[((size_t)(bz >> 2) * (size_t)a.CNY + (size_t)(by >> 2)) * (size_t)a.CNX + (size_t)(bx >> 2)];
            const long long bound = (long long)(MODE == SLICE_MAX ? (int16_t)(cm >> 16) : (int16_t)(cm & 0xFFFFu)) * 16777216ll;
            if (MODE == SLICE_MAX ? bound <= best : bound >= best) {
              k = iso_cell_exit(r, k, kb, bx >> 2, by >> 2, bz >> 2, a.slab_samples);
              continue;
            }
          }
        }
        const int k_end = proj_brick_exit(r, k, kb, bx, by, bz, a.slab_samples);
        bool skip = false;
        if constexpr (SKIP) {
          const uint32_t mm = a.dilated[((size_t)bz * (size_t)a.NBY + (size_t)by) * (size_t)a.NBX + (size_t)bx];
          const long long bound = (long long)(MODE == SLICE_MAX ? (int16_t)(mm >> 16) : (int16_t)(mm & 0xFFFFu)) * 16777216ll;
          skip = MODE == SLICE_MAX ? bound <= best : bound >= best;
        }
        if (!skip) {
          for (int j = k; j < k_end; ++j) {
            float tj;
            const f3 q = proj_sample(r, j, tj);
            const long long S = iso_field(fv, q);
            if constexpr (MODE == SLICE_MEAN) {
              sum += S;
              count += 1;
            } else if (MODE == SLICE_MAX ? S > best : S < best) {  // strict: the first sample attaining the extreme keeps its k
              best = S;
              k_ext = j;
            }
          }
        }
        k = k_end;
      }
    }
  }
  float value = __builtin_nanf(""), t_ext = __builtin_nanf("");
  if constexpr (MODE == SLICE_MEAN) {
    if (count > 0) value = (float)((double)sum / ((double)count * 16777216.0));  // |sum| <= 2^52: exact in binary64
  } else if (best != kNone) {
    value = (float)(double)best * 5.9604644775390625e-08f;  // one rounding of an integer exact in binary64, then an exact scaling
    t_ext = (float)k_ext * a.step;
  }
  uint32_t px = 0u;  // no kept sample: (0, 0, 0, 0)
  if (value == value) {
    const float u = ((value - a.window_center) / a.window_width + 0.5f) * 255.0f + 0.5f;
    const uint32_t grey = (uint32_t)(int)fminf(fmaxf(u, 0.0f), 255.0f);
    px = grey * 0x010101u | 0xFF000000u;
  }
  a.frame[(size_t)y * (size_t)a.frame_w + x] = px;
  const size_t out = (size_t)y * (size_t)a.launch_w + x;
  if (a.values) a.values[out] = value;
  if (a.t_extreme) a.t_extreme[out] = t_ext;
}

hipError_t launch_slice(const SliceArgs &a, int mode, bool dense, hipStream_t s) {
  const dim3 grid((unsigned)a.num_tiles), block(64);
  if (mode == SLICE_MEAN)
    hipLaunchKernelGGL((k_slice<SLICE_MEAN, false>), grid, block, 0, s, a);
  else if (mode == SLICE_MAX && dense)
    hipLaunchKernelGGL((k_slice<SLICE_MAX, false>), grid, block, 0, s, a);
  else if (mode == SLICE_MAX)
    hipLaunchKernelGGL((k_slice<SLICE_MAX, true>), grid, block, 0, s, a);
  else if (dense)
    hipLaunchKernelGGL((k_slice<SLICE_MIN, false>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((k_slice<SLICE_MIN, true>), grid, block, 0, s, a);
  return hipGetLastError();
}

}  // namespace clvr
