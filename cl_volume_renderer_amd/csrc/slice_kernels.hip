// slice_kernels.hip -- oblique slices and thick slabs of the volume's TRILINEAR field (clwh_render_slice): multi-planar reformatting.
// Pixel (x, y) of the region owns a ray of its own, o = (origin + x * du) + y * dv, all rays parallel along `normal`; sample k sits at
// o + normal * ((float)k * step), 0 <= k < slab_samples.  The kept-sample rule and the brick walk are the views' (view_device.hpp, with t_near = 0
// and no t_far), the bricked int16 copy of the volume is k_proj_repack's; a sample's value is the isosurface's fixed-point field S
// (trilinear_device.hpp), so MAX / MIN compare exact integers and MEAN sums them in int64.
//
//   k_slice<MODE, SKIP>  one wave per 8x8 pixel tile (view_pixel), one lane per pixel.  A thin
//                        slice (slab_samples == 1) tests sample 0 and reads it: no range search.  A slab walks the lane's kept range
//                        brick by brick (walk_bricks).  SKIP (MAX / MIN without CLWH_SLICE_DENSE): a brick whose dilated maximum cannot beat the
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
  uint32_t x, y;
  view_pixel(a.fr, x, y);
  const float fx = (float)x, fy = (float)y;
  const f3 o = f3{(a.origin[0] + fx * a.du[0]) + fy * a.dv[0], (a.origin[1] + fx * a.du[1]) + fy * a.dv[1],
                  (a.origin[2] + fx * a.du[2]) + fy * a.dv[2]};
  const ProjRay r{o, f3{a.normal[0], a.normal[1], a.normal[2]}, a.step, 0.0f, INFINITY, (float)a.vol.X, (float)a.vol.Y, (float)a.vol.Z};

  constexpr long long kNone = MODE == SLICE_MAX ? LLONG_MIN : LLONG_MAX;  // beyond |S| <= 2^39: no sample yet, and no brick is skipped
  long long best = kNone, sum = 0;
  int k_ext = 0, count = 0;
  // a cell of 4^3 bricks or a brick whose dilated {min, max} cannot change the extreme
  const auto cannot_beat = [&](uint32_t mm) {
    const long long bound = (long long)(MODE == SLICE_MAX ? table_max(mm) : table_min(mm)) * 16777216ll;
    return MODE == SLICE_MAX ? bound <= best : bound >= best;
  };
  if (a.slab_samples == 1) {  // a thin slice: sample 0 alone
    float t;
    const f3 p = proj_sample(r, 0, t);
    if (p.x >= 0.0f && p.x < r.dx && p.y >= 0.0f && p.y < r.dy && p.z >= 0.0f && p.z < r.dz) {
      best = sum = iso_field(a.vol, p);
      count = 1;
    }
  } else {
    int k, kb;
    if (proj_kept_range(r, a.slab_samples, k, kb)) {
      walk_bricks(
          r, a.vol, k, kb, a.slab_samples,
          [&](size_t cell) {
            if constexpr (SKIP) return a.use_coarse && cannot_beat(a.vol.coarse[cell]);
            else return false;
          },
          [&](size_t brick) {
            if constexpr (SKIP) return cannot_beat(a.vol.dilated[brick]);
            else return false;
          },
          [&](size_t, int k0, int k_end) {
            for (int j = k0; j < k_end; ++j) {
              float tj;
              const f3 q = proj_sample(r, j, tj);
              const long long S = iso_field(a.vol, q);
              if constexpr (MODE == SLICE_MEAN) {
                sum += S;
                count += 1;
              } else {
                const bool better = MODE == SLICE_MAX ? S > best : S < best;  // strict: the first sample attaining the extreme keeps its k
                k_ext = better ? j : k_ext;
                best = better ? S : best;
              }
            }
            return false;
          });
    }
  }
  float value = __builtin_nanf(""), t_ext = __builtin_nanf("");
  if constexpr (MODE == SLICE_MEAN) {
    if (count > 0) value = (float)((double)sum / ((double)count * 16777216.0));  // |sum| <= 2^52: exact in binary64
  } else if (best != kNone) {
    value = (float)(double)best * 5.9604644775390625e-08f;  // one rounding of an integer exact in binary64, then an exact scaling
    t_ext = (float)k_ext * a.step;
  }
  const size_t out = store_frame(a.fr, x, y, window_grey(value, a.window_center, a.window_width));
  store_optional(a.values, out, value);
  store_optional(a.t_extreme, out, t_ext);
}

hipError_t launch_slice(const SliceArgs &a, int mode, bool dense, hipStream_t s) {
  const dim3 grid((unsigned)a.fr.num_tiles), block(64);
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
