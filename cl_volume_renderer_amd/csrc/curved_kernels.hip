// curved_kernels.hip -- the straightened curved planar reformat (clwh_render_curved) and the section profile of a mask along a curve
// (clwh_curve_profile), gfx950.  Both read `rows`: nine floats per station of the curve -- origin[3], du[3], normal[3] in voxel space --
// staged by the host into a buffer of the context (clwh_views.hip).
//
//   k_curved<MODE, SKIP>  clwh_render_slice's pixel with a frame of its own per image row: pixel (x, y) owns the ray o = origin_y +
//                        (float)x * du_y along normal_y, and from there on the kernel is k_slice word for word (slice_kernels.hip):
//                        one wave per 8x8 pixel tile (view_pixel), one lane per pixel, a thin view reads sample 0 without a range
//                        search, a slab walks its kept range brick by brick (walk_bricks), and SKIP steps over bricks and cells of 4^3
//                        bricks whose dilated {min, max} cannot beat the running extreme.  The proof of the skip rule is per ray and
//                        nowhere uses that the rays of a wave are parallel.  A tile's eight rows are 72 floats; each lane reads its
//                        row's nine with plain loads (eight lanes share an address; DESIGN.md, section 4, has the compiled code).
//                        No LDS, no atomics, no scratch memory.
//
//   k_curve_profile<CONNECTED>  one wave per station, lane x (< width) owns column x of the station's grid of width x slab_samples
//                        samples: a 64-bit word whose bit k says "sample (x, k) is kept and its voxel's bit is set in the mask".
//                        Without CONNECTED the section is all set samples.  With it the section R is flooded from the centre samples:
//                        a round fills, inside every lane's word, the runs of set bits that hold a bit of R (fill_runs: O(1) by carry
//                        propagation), then takes the bits of the lanes x - 1 and x + 1 that are set here too; the rounds end when a
//                        wave-wide vote sees no lane change.
//     It terminates, with the right set.  R starts as a subset of the set samples S and only ever gains bits of S that are 4-neighbours
//     (along k: the runs; along x: the two neighbour lanes) of bits it holds, so R never leaves the union of the components of S that
//     hold a centre sample.  R is monotone and bounded by the 4096 bits of a section, and a round that is not the last adds at least
//     one bit: at most 4096 rounds.  When a round changes nothing, every set 4-neighbour of a bit of R is in R: R is closed under
//     the neighbourhood, so it is that whole union.
//                        The record is popcounts and wave sums; lane 0 stores its 16 bytes with one vector store.  No LDS, no atomics.
#include <climits>

#include "trilinear_device.hpp"

namespace clvr {

namespace {

enum : int { CURVED_MAX = CLWH_SLICE_MAX, CURVED_MIN = CLWH_SLICE_MIN, CURVED_MEAN = CLWH_SLICE_MEAN };
typedef unsigned long long u64;

// station y's origin[3], du[3], normal[3]
struct CurveRow {
  f3 origin, du, normal;
};
__device__ __forceinline__ CurveRow curve_row(const float *__restrict__ rows, uint32_t y) {
  const float *__restrict__ r = rows + (size_t)y * 9u;
  return CurveRow{f3{r[0], r[1], r[2]}, f3{r[3], r[4], r[5]}, f3{r[6], r[7], r[8]}};
}
// o = origin + (float)x * du: per component one multiply, then one add
__device__ __forceinline__ f3 curve_origin(const CurveRow &c, uint32_t x) {
  const float fx = (float)x;
  return f3{c.origin.x + fx * c.du.x, c.origin.y + fx * c.du.y, c.origin.z + fx * c.du.z};
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off);
  return v;
}
__device__ __forceinline__ u64 lane_word(u64 v, int lane) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, lane), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), lane);
  return (u64)lo | ((u64)hi << 32);
}
// r (a subset of s) with every run of set bits of s filled upwards from its lowest bit of r: s + r carries from that bit to the run's
// end and stops at the clear bit above it, so the bits of s that the sum flipped are the run's bits from there on, except the bits of r
// above it, which took a carry and kept their 1
__device__ __forceinline__ u64 fill_up(u64 s, u64 r) { return ((s ^ (s + r)) & s) | r; }
// ... and both ways: every run of s that holds a bit of r, whole
__device__ __forceinline__ u64 fill_runs(u64 s, u64 r) { return fill_up(s, r) | __brevll(fill_up(__brevll(s), __brevll(r))); }

}  // namespace

template <int MODE, bool SKIP>
__global__ __launch_bounds__(64) void k_curved(const CurvedArgs a) {
  uint32_t x, y;
  view_pixel(a.fr, x, y);
  const CurveRow row = curve_row(a.rows, y);
  const ProjRay r{curve_origin(row, x), row.normal, a.step, 0.0f, INFINITY, (float)a.vol.X, (float)a.vol.Y, (float)a.vol.Z};

  constexpr long long kNone = MODE == CURVED_MAX ? LLONG_MIN : LLONG_MAX;  // beyond |S| <= 2^39: no sample yet, and no brick is skipped
  long long best = kNone, sum = 0;
  int k_ext = 0, count = 0;
  // a cell of 4^3 bricks or a brick whose dilated {min, max} cannot change the extreme
  const auto cannot_beat = [&](uint32_t mm) {
    const long long bound = (long long)(MODE == CURVED_MAX ? table_max(mm) : table_min(mm)) * 16777216ll;
    return MODE == CURVED_MAX ? bound <= best : bound >= best;
  };
  if (a.slab_samples == 1) {  // a thin view: sample 0 alone
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
              if constexpr (MODE == CURVED_MEAN) {
                sum += S;
                count += 1;
              } else {
                const bool better = MODE == CURVED_MAX ? S > best : S < best;  // strict: the first sample attaining the extreme keeps its k
                k_ext = better ? j : k_ext;
                best = better ? S : best;
              }
            }
            return false;
          });
    }
  }
  float value = __builtin_nanf(""), t_ext = __builtin_nanf("");
  if constexpr (MODE == CURVED_MEAN) {
    if (count > 0) value = (float)((double)sum / ((double)count * 16777216.0));  // |sum| <= 2^52: exact in binary64
  } else if (best != kNone) {
    value = (float)(double)best * 5.9604644775390625e-08f;  // one rounding of an integer exact in binary64, then an exact scaling
    t_ext = (float)k_ext * a.step;
  }
  const size_t out = store_frame(a.fr, x, y, window_grey(value, a.window_center, a.window_width));
  store_optional(a.values, out, value);
  store_optional(a.t_extreme, out, t_ext);
}

hipError_t launch_curved(const CurvedArgs &a, int mode, bool dense, hipStream_t s) {
  const dim3 grid((unsigned)a.fr.num_tiles), block(64);
  if (mode == CURVED_MEAN)
    hipLaunchKernelGGL((k_curved<CURVED_MEAN, false>), grid, block, 0, s, a);
  else if (mode == CURVED_MAX && dense)
    hipLaunchKernelGGL((k_curved<CURVED_MAX, false>), grid, block, 0, s, a);
  else if (mode == CURVED_MAX)
    hipLaunchKernelGGL((k_curved<CURVED_MAX, true>), grid, block, 0, s, a);
  else if (dense)
    hipLaunchKernelGGL((k_curved<CURVED_MIN, false>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((k_curved<CURVED_MIN, true>), grid, block, 0, s, a);
  return hipGetLastError();
}

template <bool CONNECTED>
__global__ __launch_bounds__(64) void k_curve_profile(const CurveProfileArgs a) {
  const uint32_t y = blockIdx.x, x = threadIdx.x;  // the grid is n_rows blocks of one wave
  const int n = a.slab_samples, w = a.width;
  u64 set = 0ull;
  if ((int)x < w) {
    const CurveRow row = curve_row(a.rows, y);
    const ProjRay r{curve_origin(row, x), row.normal, a.step, 0.0f, INFINITY, (float)a.X, (float)a.Y, (float)a.Z};
    for (int k = 0; k < n; ++k) {
      float t;
      const f3 p = proj_sample(r, k, t);
      if (p.x >= 0.0f && p.x < r.dx && p.y >= 0.0f && p.y < r.dy && p.z >= 0.0f && p.z < r.dz) {  // kept: the conversions are floors
        const uint32_t vx = (uint32_t)(int)p.x, vy = (uint32_t)(int)p.y, vz = (uint32_t)(int)p.z;
        const u64 word = a.mask[((size_t)vz * (size_t)a.Y + (size_t)vy) * (size_t)a.W64 + (size_t)(vx >> 6)];
        set |= ((word >> (vx & 63u)) & 1ull) << k;
      }
    }
  }
  u64 section = set;
  if constexpr (CONNECTED) {
    const bool centre_x = (int)x == (w - 1) / 2 || (int)x == w / 2;
    u64 reach = centre_x ? set & ((1ull << ((n - 1) / 2)) | (1ull << (n / 2))) : 0ull;
    const int lane = (int)x;
    bool changed;
    do {
      u64 next = fill_runs(set, reach);
      const u64 left = lane_word(next, lane > 0 ? lane - 1 : lane), right = lane_word(next, lane < 63 ? lane + 1 : lane);
      next |= (left | right) & set;
      changed = next != reach;
      reach = next;
    } while (__any(changed));
    section = reach;
  }
  const uint32_t count = (uint32_t)__popcll(section);
  uint32_t sum_k = 0u;
  for (u64 rest = section; rest != 0ull; rest &= rest - 1ull) sum_k += (uint32_t)__builtin_ctzll(rest);
  const bool edge_x = x == 0u || (int)x == w - 1;
  const uint32_t border = (uint32_t)__popcll(edge_x ? section : section & (1ull | (1ull << (n - 1))));
  const uint4 record = make_uint4(wave_sum(count), wave_sum(x * count), wave_sum(sum_k), wave_sum(border));
  if (x == 0u) reinterpret_cast<uint4 *>(a.records)[y] = record;
}

hipError_t launch_curve_profile(const CurveProfileArgs &a, bool connected, hipStream_t s) {
  const dim3 grid(a.n_rows), block(64);
  if (connected)
    hipLaunchKernelGGL((k_curve_profile<true>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((k_curve_profile<false>), grid, block, 0, s, a);
  return hipGetLastError();
}

}  // namespace clvr
