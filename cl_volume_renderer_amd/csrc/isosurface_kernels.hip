// isosurface_kernels.hip -- the first position along a camera ray where the TRILINEAR field of the volume reaches a value, with its
// depth, normal and headlight shading (clwh_render_isosurface).  The sample set and the brick walk are the views' (view_device.hpp), the bricked
// int16 copy of the volume is k_proj_repack's.  The field is the contract's fixed-point one (include/clwh.h): per axis
// an 8-bit weight, the 8 corners combined in integers, S = value * 2^24 exactly -- so the hit decision S >= T holds whatever the order
// of evaluation, and the result can be tested bit for bit.
//
//   k_iso_dilate             the derived data: per 8^3 brick the {min, max} over the brick dilated by one voxel (10^3 voxels, clamped at
//                            the volume's faces), read from the bricked copy; one wave per brick.
//   k_iso_coarse             the same pair per cell of 4^3 bricks, from k_iso_dilate's table (stored behind it).
//   k_isosurface<BELOW, SKIP> one wave per 8x8 pixel tile (view_pixel); each lane walks its ray's kept range brick by brick
//                            (walk_bricks) and ends at the first inside sample.  SKIP (without CLWH_ISO_DENSE): a brick
//                            whose dilated {min, max} cannot reach T is stepped over unread.  A sample whose voxel floor(p) = v lies in
//                            the brick has i0 in {v - 1, v} per axis, so its clamped corners lie in the dilated box, and S is a
//                            combination of their values with non-negative integer weights summing to 2^24: dmin * 2^24 <= S <=
//                            dmax * 2^24, hence the bytes are the dense walk's.  The walk asks the cell of 4^3 bricks first: its pair
//                            bounds every brick in it, so a cell that cannot reach T is left by ONE exit search (measured: 1.25-1.55x
//                            on the surface from outside, 3.2-3.5x where every brick is skipped).  Refinement and the
//                            normal run once per hit lane, after the march.
//
// The field itself (iso_field) is in trilinear_device.hpp, shared with k_slice.
#include "trilinear_device.hpp"

namespace clvr {

// ------------------------------------------------------------------------------------------------
// k_iso_dilate
__global__ __launch_bounds__(256) void k_iso_dilate(const int16_t *__restrict__ bricks, int X, int Y, int Z, int NBX, int NBY, int NBZ,
                                                    uint32_t *__restrict__ dilated) {
  const size_t n_bricks = (size_t)NBX * (size_t)NBY * (size_t)NBZ;
  const size_t brick = (size_t)blockIdx.x * 4u + (threadIdx.x >> 6);  // uniform over the wave
  if (brick >= n_bricks) return;
  const unsigned lane = threadIdx.x & 63u;
  const int bx = (int)(brick % (size_t)NBX), by = (int)((brick / (size_t)NBX) % (size_t)NBY), bz = (int)(brick / ((size_t)NBX * (size_t)NBY));
  uint32_t lo = 0xFFFFFFFFu, hi = 0xFFFFFFFFu;  // unsigned minima of v + 32768 and 32767 - v (the wave minimum is unsigned)
  for (unsigned i = lane; i < 1000u; i += 64u) {
    const int hx = (int)(i % 10u), hy = (int)((i / 10u) % 10u), hz = (int)(i / 100u);
    // a coordinate clamped into the volume names a voxel of the dilated, clamped box again: duplicates do not move a minimum
    const int x = min(max(bx * 8 - 1 + hx, 0), X - 1), y = min(max(by * 8 - 1 + hy, 0), Y - 1), z = min(max(bz * 8 - 1 + hz, 0), Z - 1);
    const int v = bricks[VolumePacked::record_index(x, y, z, NBX, NBY)];
    lo = min(lo, (uint32_t)(v + 32768));
    hi = min(hi, (uint32_t)(32767 - v));
  }
  lo = wave_min_u32(lo);
  hi = wave_min_u32(hi);
  if (lane == 0u) dilated[brick] = pack_min_max((int)lo - 32768, 32767 - (int)hi);
}

// k_iso_coarse: the second level -- per cell of 4^3 bricks (32^3 voxels) the {min, max} over its bricks' dilated entries, i.e. over the
// union of their dilated boxes; one thread per cell
__global__ __launch_bounds__(256) void k_iso_coarse(const uint32_t *__restrict__ dilated, int NBX, int NBY, int NBZ, uint32_t *__restrict__ coarse) {
  const int CNX = (NBX + 3) / 4, CNY = (NBY + 3) / 4, CNZ = (NBZ + 3) / 4;
  const size_t cell = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (cell >= (size_t)CNX * CNY * CNZ) return;
  const int cx = (int)(cell % (size_t)CNX), cy = (int)((cell / (size_t)CNX) % (size_t)CNY), cz = (int)(cell / ((size_t)CNX * CNY));
  int lo = 32767, hi = -32768;
  for (int z = cz * 4; z < min(cz * 4 + 4, NBZ); ++z)
    for (int y = cy * 4; y < min(cy * 4 + 4, NBY); ++y)
      for (int x = cx * 4; x < min(cx * 4 + 4, NBX); ++x) {
        const uint32_t mm = dilated[((size_t)z * NBY + y) * NBX + x];
        lo = min(lo, table_min(mm));
        hi = max(hi, table_max(mm));
      }
  coarse[cell] = pack_min_max(lo, hi);
}

template <bool BELOW>
__device__ __forceinline__ bool iso_inside(long long S, long long T) { return BELOW ? S <= T : S >= T; }

// G at p: the corners' clamped central differences under the corners' weights (once per hit lane)
__device__ __forceinline__ void iso_gradient(const ViewVolume &v, const IsoCell c, long long &Gx, long long &Gy, long long &Gz) {
  Gx = Gy = Gz = 0;
  for (int corner = 0; corner < 8; ++corner) {
    const int ox = corner & 1, oy = (corner >> 1) & 1, oz = corner >> 2;
    const int x = min(max(c.ix + ox, 0), v.X - 1), y = min(max(c.iy + oy, 0), v.Y - 1), z = min(max(c.iz + oz, 0), v.Z - 1);
    const int w = (ox ? c.wx : 256 - c.wx) * (oy ? c.wy : 256 - c.wy) * (oz ? c.wz : 256 - c.wz);  // <= 2^24
    int dx, dy, dz;
    central_difference(v, x, y, z, dx, dy, dz);
    Gx += (long long)w * (long long)dx;
    Gy += (long long)w * (long long)dy;
    Gz += (long long)w * (long long)dz;
  }
}

template <bool BELOW, bool SKIP>
__global__ __launch_bounds__(64) void k_isosurface(const IsoArgs a) {
  uint32_t x, y;
  view_pixel(a.fr, x, y);
  const ProjRay r = camera_ray(a.cam, a.vol, a.fr, x, y);
  const long long T = a.threshold;
  // a cell of 4^3 bricks or a brick whose dilated {min, max} cannot reach T
  const auto unreachable = [&](uint32_t mm) { return BELOW ? table_min(mm) > a.skip_bound : table_max(mm) < a.skip_bound; };

  bool hit = false;
  int k_hit = 0, k_first = 0;
  long long S_hit = 0;
  int k, kb;
  if (proj_kept_range(r, a.cam.k_cap, k, kb)) {
    k_first = k;
    hit = walk_bricks(
        r, a.vol, k, kb, a.cam.k_cap,
        [&](size_t cell) {
          if constexpr (SKIP) return unreachable(a.vol.coarse[cell]);
          else return false;
        },
        [&](size_t brick) {
          if constexpr (SKIP) return unreachable(a.vol.dilated[brick]);
          else return false;
        },
        [&](size_t, int k0, int k_end) {
          for (int j = k0; j < k_end; ++j) {
            float tj;
            const f3 q = proj_sample(r, j, tj);
            const long long S = iso_field(a.vol, q);
            if (iso_inside<BELOW>(S, T)) {
              k_hit = j;
              S_hit = S;
              return true;
            }
          }
          return false;
        });
  }

  uint32_t px = 0u;  // a miss: (0, 0, 0, 0)
  float t_hit = __builtin_nanf("");
  float4 nrm = float4{t_hit, t_hit, t_hit, t_hit};
  if (hit) {
    float hi = (float)k_hit * r.h;
    if (k_hit > k_first) {  // k_hit - 1 is kept and outside
      float lo = (float)(k_hit - 1) * r.h;
      for (int i = 0; i < a.refine; ++i) {
        const float m = lo + (hi - lo) * 0.5f;
        const f3 p = f3{r.o.x + r.d.x * m, r.o.y + r.d.y * m, r.o.z + r.d.z * m};  // between two kept samples: inside the volume
        const long long S = iso_field(a.vol, p);
        if (iso_inside<BELOW>(S, T)) {
          hi = m;
          S_hit = S;
        } else {
          lo = m;
        }
      }
    }
    t_hit = hi;
    const f3 p = f3{r.o.x + r.d.x * t_hit, r.o.y + r.d.y * t_hit, r.o.z + r.d.z * t_hit};
    long long Gx, Gy, Gz;
    iso_gradient(a.vol, iso_cell(p), Gx, Gy, Gz);
    const float gx = (float)(double)Gx, gy = (float)(double)Gy, gz = (float)(double)Gz;  // exact in binary64: one rounding
    const float l2 = length2(gx, gy, gz);
    float s = 1.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f;
    if (l2 > 0.0f) {
      const float len = sqrtf(l2);
      nx = gx / len;
      ny = gy / len;
      nz = gz / len;
      s = headlight(gx, gy, gz, len, r.d, a.ambient);
    }
    px = quantise_unorm8(a.color[0] * s) | (quantise_unorm8(a.color[1] * s) << 8) | (quantise_unorm8(a.color[2] * s) << 16) | 0xFF000000u;
    nrm = float4{canonical_nan(nx), canonical_nan(ny), canonical_nan(nz), (float)(double)S_hit * 5.9604644775390625e-08f};
  }
  const size_t o = store_frame(a.fr, x, y, px);
  store_optional(a.t_hit, o, t_hit);
  store_optional(a.normal, o, nrm);
}

hipError_t launch_iso_dilate(const ViewVolume &v, uint32_t *dilated, hipStream_t s) {
  const size_t n_bricks = (size_t)v.NBX * (size_t)v.NBY * (size_t)v.NBZ;
  hipLaunchKernelGGL(k_iso_dilate, dim3((unsigned)((n_bricks + 3u) / 4u)), dim3(256), 0, s, v.bricks, v.X, v.Y, v.Z, v.NBX, v.NBY, v.NBZ, dilated);
  const size_t n_cells = (size_t)v.CNX * (size_t)v.CNY * (size_t)((v.NBZ + 3) / 4);
  hipLaunchKernelGGL(k_iso_coarse, dim3((unsigned)((n_cells + 255u) / 256u)), dim3(256), 0, s, dilated, v.NBX, v.NBY, v.NBZ, dilated + n_bricks);
  return hipGetLastError();
}

hipError_t launch_isosurface(const IsoArgs &a, bool below, bool dense, hipStream_t s) {
  const dim3 grid((unsigned)a.fr.num_tiles), block(64);
  if (below && dense)
    hipLaunchKernelGGL((k_isosurface<true, false>), grid, block, 0, s, a);
  else if (below)
    hipLaunchKernelGGL((k_isosurface<true, true>), grid, block, 0, s, a);
  else if (dense)
    hipLaunchKernelGGL((k_isosurface<false, false>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((k_isosurface<false, true>), grid, block, 0, s, a);
  return hipGetLastError();
}

}  // namespace clvr
