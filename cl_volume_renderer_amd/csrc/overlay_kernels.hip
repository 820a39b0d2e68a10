// overlay_kernels.hip -- a mask or a labelling drawn over a frame a view has written (clwh_overlay_slice, clwh_overlay_camera), and the
// id under every pixel.  The region is a caller's buffer: grow's bit rows (word(v) = the bit) or uint32[Z][Y][X] (word(v) = the word);
// id(v) = word(v) if id_lo <= word(v) <= id_hi, else 0.  A pixel's ray is the slice's or the projection's, its kept-sample rule and the
// brick walk are the views' (view_device.hpp, unchanged); ID(x, y) is the id of the first kept sample whose id is not 0, K(x, y) that
// sample's index.
//
//   k_region_occupancy<KIND>  one word per 8^3 brick of the region and one per cell of 4^3 bricks: 1 iff a voxel in it has a nonzero
//                             id.  One wave per run of eight bricks along x (64 voxels): of a mask a lane reads one 64-bit word, a row
//                             of the eight bricks, with the bits at x >= X masked off; of a labelling a lane reads one voxel column
//                             through the 64 rows, so that a wave's load is 256 contiguous bytes.  The cells' words are zero on entry
//                             and OR-ed into.  Built per call, for the camera's rays only (the slice call walks densely: DESIGN.md).
//   k_region_ids<RAY, KIND, SKIP>
//                             one lane per pixel of the PADDED grid (width + 2) x (height + 2), pixel (gx - 1, gy - 1): the launched
//                             region and the one-pixel halo the outline rule reads, so no ray is marched five times.  Writes {ID, K}.
//                             SKIP (camera rays without CLWH_OVERLAY_DENSE): a brick or cell whose occupancy word is 0 is stepped
//                             over unread -- no sample in it has an id, so the first hit is the dense walk's.
//   k_overlay_blend           one wave per 8x8 tile of the region (view_pixel), one lane per pixel: reads the pixel's and its four
//                             neighbours' ids, blends the palette's colour into the frame in integers, stores ids and t_first.
#include "view_device.hpp"

namespace clvr {

enum : int { REGION_MASK = CLWH_REGION_MASK, REGION_LABELS = CLWH_REGION_LABELS };
enum : int { RAY_PLANE = 0, RAY_CAMERA = 1 };

// the filtered id of voxel (x, y, z), 0 <= x < X and so on
template <int KIND>
__device__ __forceinline__ uint32_t region_id(const OverlayArgs &a, int x, int y, int z) {
  const size_t row = (size_t)z * (size_t)a.vol.Y + (size_t)y;
  uint32_t word;
  if constexpr (KIND == REGION_MASK)
    word = (uint32_t)(a.mask[row * (size_t)a.W64 + ((size_t)x >> 6)] >> (x & 63)) & 1u;
  else
    word = a.labels[row * (size_t)a.vol.X + (size_t)x];
  return word >= a.id_lo && word <= a.id_hi ? word : 0u;
}

template <int KIND>
__global__ __launch_bounds__(64) void k_region_occupancy(const OverlayArgs a, uint32_t *bricks, uint32_t *cells) {
  const uint32_t W64 = (uint32_t)a.W64, run = blockIdx.x;  // run (bz * NBY + by) * W64 + wx: the bricks 8 * wx .. 8 * wx + 7 of a row of bricks
  const int wx = (int)(run % W64), by = (int)(run / W64 % (uint32_t)a.vol.NBY), bz = (int)(run / (W64 * (uint32_t)a.vol.NBY));
  const uint32_t lane = threadIdx.x;
  uint32_t occupied = 0u;  // bit j: brick 8 * wx + j holds a nonzero id (the same in every lane)
  if constexpr (KIND == REGION_MASK) {
    // a lane takes a row (y, z) of the slab of bricks: one 64-bit word of it, whose byte j is brick j's; bits at x >= X are not the region's
    const int y = by * 8 + (int)(lane & 7u), z = bz * 8 + (int)(lane >> 3);
    unsigned long long word = 0ull;
    if (y < a.vol.Y && z < a.vol.Z && a.id_lo == 1u) {  // a set bit is the word 1 (id_hi >= id_lo)
      word = a.mask[((size_t)z * (size_t)a.vol.Y + (size_t)y) * (size_t)W64 + (size_t)wx];
      const int valid = a.vol.X - wx * 64;  // >= 1
      if (valid < 64) word &= (1ull << valid) - 1ull;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) occupied |= (__ballot(((word >> (8 * j)) & 0xFFull) != 0ull) != 0ull ? 1u : 0u) << j;
  } else {
    // a lane takes a voxel column x of the run and the slab's 64 rows in turn: every load of the wave is 256 contiguous bytes
    const int x = wx * 64 + (int)lane;
    bool any = false;
    if (x < a.vol.X) {
      const int z_end = min(bz * 8 + 8, a.vol.Z);
      for (int z = bz * 8; z < z_end; ++z) {
        uint32_t ids[8];  // eight loads in flight; a row past the volume's face repeats the last one
#pragma unroll
        for (int j = 0; j < 8; ++j) ids[j] = region_id<KIND>(a, x, min(by * 8 + j, a.vol.Y - 1), z);
#pragma unroll
        for (int j = 0; j < 8; ++j) any |= ids[j] != 0u;
      }
    }
    const unsigned long long columns = __ballot(any);
#pragma unroll
    for (int j = 0; j < 8; ++j) occupied |= (((columns >> (8 * j)) & 0xFFull) != 0ull ? 1u : 0u) << j;
  }
  const int bx = wx * 8 + (int)lane;
  if (lane < 8u && bx < a.vol.NBX) {
    const uint32_t holds = (occupied >> lane) & 1u;
    bricks[brick_index(a.vol, bx, by, bz)] = holds;
    if (holds) atomicOr(&cells[cell_index(a.vol, bx >> 2, by >> 2, bz >> 2)], 1u);
  }
}

template <int RAY, int KIND, bool SKIP>
__global__ __launch_bounds__(64) void k_region_ids(const OverlayArgs a) {
  const int gx = (int)(blockIdx.x * 8u + (threadIdx.x & 7u)), gy = (int)(blockIdx.y * 8u + (threadIdx.x >> 3));
  const int padded_w = a.fr.launch_w + 2;
  if (gx >= padded_w || gy >= a.fr.launch_h + 2) return;
  const int x = gx - 1, y = gy - 1;  // -1 .. launch_w, -1 .. launch_h

  ProjRay r;
  int k_cap;
  if constexpr (RAY == RAY_PLANE) {
    const float fx = (float)x, fy = (float)y;
    const f3 o = f3{(a.origin[0] + fx * a.du[0]) + fy * a.dv[0], (a.origin[1] + fx * a.du[1]) + fy * a.dv[1],
                    (a.origin[2] + fx * a.du[2]) + fy * a.dv[2]};
    r = ProjRay{o, f3{a.normal[0], a.normal[1], a.normal[2]}, a.step, 0.0f, INFINITY, (float)a.vol.X, (float)a.vol.Y, (float)a.vol.Z};
    k_cap = a.slab_samples;
  } else {
    const Ray ray = generate_ray(f3{a.cam.cam_pos[0], a.cam.cam_pos[1], a.cam.cam_pos[2]}, f3{a.cam.cam_dir[0], a.cam.cam_dir[1], a.cam.cam_dir[2]},
                                 x, y, a.fr.frame_w, a.fr.frame_h);
    r = ProjRay{ray.origin, ray.direction, a.cam.step, a.cam.t_near, a.cam.t_far, (float)a.vol.X, (float)a.vol.Y, (float)a.vol.Z};
    k_cap = a.cam.k_cap;
  }

  uint32_t id = 0u;
  int k_hit = 0;
  const auto id_at = [&](int j) {
    float tj;
    const f3 q = proj_sample(r, j, tj);  // kept: 0 <= q < dim, so the conversions are floors
    return region_id<KIND>(a, (int)q.x, (int)q.y, (int)q.z);
  };
  if (RAY == RAY_PLANE && k_cap == 1) {  // a thin slice: sample 0 alone
    float t;
    const f3 p = proj_sample(r, 0, t);
    if (p.x >= 0.0f && p.x < r.dx && p.y >= 0.0f && p.y < r.dy && p.z >= 0.0f && p.z < r.dz) id = id_at(0);
  } else {
    int k, kb;
    if (proj_kept_range(r, k_cap, k, kb)) {
      walk_bricks(
          r, a.vol, k, kb, k_cap,
          [&](size_t cell) {
            if constexpr (SKIP) return a.occ_cells[cell] == 0u;
            else return false;
          },
          [&](size_t brick) {
            if constexpr (SKIP) return a.occ_bricks[brick] == 0u;
            else return false;
          },
          [&](size_t, int k0, int k_end) {
            for (int j = k0; j < k_end; ++j) {
              const uint32_t w = id_at(j);
              if (w != 0u) {
                id = w;
                k_hit = j;
                return true;
              }
            }
            return false;
          });
    }
  }
  a.pixel_ids[(size_t)gy * (size_t)padded_w + (size_t)gx] = uint2{id, (uint32_t)k_hit};
}

// (c * (255 - a) + d * a + 127) / 255 for bytes c, d, a: at most 255 * 255 + 127
__device__ __forceinline__ uint32_t mix8(uint32_t c, uint32_t d, uint32_t a) { return (c * (255u - a) + d * a + 127u) / 255u; }

__global__ __launch_bounds__(64) void k_overlay_blend(const OverlayArgs a) {
  uint32_t x, y;
  view_pixel(a.fr, x, y);
  const size_t padded_w = (size_t)a.fr.launch_w + 2u;
  const uint2 *__restrict__ centre = a.pixel_ids + ((size_t)y + 1u) * padded_w + ((size_t)x + 1u);
  const uint32_t id = centre->x;
  const bool outline = id != 0u && (centre[-1].x != id || centre[1].x != id || (centre - padded_w)->x != id || (centre + padded_w)->x != id);

  const bool paint_outline = (a.flags & CLWH_OVERLAY_OUTLINE) != 0 && outline;
  const bool paint_fill = !paint_outline && (a.flags & CLWH_OVERLAY_FILL) != 0 && id != 0u;
  if (paint_outline || paint_fill) {
    const uint32_t col = a.palette[(id - 1u) % a.n_colours];
    const uint32_t al = ((col >> 24) * (paint_outline ? a.outline_alpha : a.fill_alpha) + 127u) / 255u;
    uint32_t *px = a.fr.frame + (size_t)y * (size_t)a.fr.frame_w + x;
    const uint32_t in = *px, in_a = in >> 24;
    *px = mix8(in & 255u, col & 255u, al) | mix8((in >> 8) & 255u, (col >> 8) & 255u, al) << 8 |
          mix8((in >> 16) & 255u, (col >> 16) & 255u, al) << 16 | (in_a + ((255u - in_a) * al + 127u) / 255u) << 24;
  }
  const size_t out = (size_t)y * (size_t)a.fr.launch_w + x;
  store_optional(a.ids, out, id);
  store_optional(a.t_first, out, id != 0u ? (float)(int)centre->y * a.step : __builtin_nanf(""));
}

hipError_t launch_region_occupancy(const OverlayArgs &a, uint32_t *bricks, uint32_t *cells, size_t n_cells, hipStream_t s) {
  hipError_t e = hipMemsetAsync(cells, 0, n_cells * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  const dim3 grid((unsigned)((size_t)a.W64 * a.vol.NBY * a.vol.NBZ)), block(64);  // (at most X * Y * Z / 64 + ... < 2^31 runs)
  if (a.kind == REGION_MASK)
    hipLaunchKernelGGL((k_region_occupancy<REGION_MASK>), grid, block, 0, s, a, bricks, cells);
  else
    hipLaunchKernelGGL((k_region_occupancy<REGION_LABELS>), grid, block, 0, s, a, bricks, cells);
  return hipGetLastError();
}

template <int RAY, int KIND, bool SKIP>
static void launch_ids(const OverlayArgs &a, hipStream_t s) {
  const dim3 grid(((unsigned)a.fr.launch_w + 2u + 7u) / 8u, ((unsigned)a.fr.launch_h + 2u + 7u) / 8u), block(64);
  hipLaunchKernelGGL((k_region_ids<RAY, KIND, SKIP>), grid, block, 0, s, a);
}

// `skip`: the camera's rays step over empty bricks by a.occ_bricks / a.occ_cells; the plane's rays always walk densely
hipError_t launch_overlay(const OverlayArgs &a, bool camera, bool skip, hipStream_t s) {
  const bool mask = a.kind == REGION_MASK;
  if (!camera) mask ? launch_ids<RAY_PLANE, REGION_MASK, false>(a, s) : launch_ids<RAY_PLANE, REGION_LABELS, false>(a, s);
  else if (skip) mask ? launch_ids<RAY_CAMERA, REGION_MASK, true>(a, s) : launch_ids<RAY_CAMERA, REGION_LABELS, true>(a, s);
  else mask ? launch_ids<RAY_CAMERA, REGION_MASK, false>(a, s) : launch_ids<RAY_CAMERA, REGION_LABELS, false>(a, s);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_overlay_blend, dim3((unsigned)a.fr.num_tiles), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace clvr
