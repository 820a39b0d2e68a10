// primary_kernels.hip -- the kernels of the `render` pass with one lane per pixel or per primary hit: k_primary and k_ao (CLWH_SHADE_AO)
#include "bounce_device.hpp"

namespace clvr {

// k_primary: ray_marching.cl:152-186 up to (and including) the first march_to_next_event of
// compute_light (:33), plus the hit's normal (:42).  One wave = one 8x8 pixel tile.
template <bool USE_GRAD>
__global__ __launch_bounds__(64) void k_primary(const RenderArgs a) {
  const uint32_t slot = xcd_contiguous_slot(blockIdx.x, a.num_tile_slots);
  int tx, ty;
  if (!tile_from_slot(a, slot, tx, ty)) return;
  const uint32_t lane = threadIdx.x;
  const uint32_t x = (uint32_t)tx * 8u + (lane & 7u);
  const uint32_t y = (uint32_t)ty * 8u + (lane >> 3);
  const uint32_t pslot = slot * 64u + lane;

  const VolumePacked vol = make_volume(a);
  const f3 cam_o = f3{a.cam_pos[0], a.cam_pos[1], a.cam_pos[2]};
  const f3 cam_d = f3{a.cam_dir[0], a.cam_dir[1], a.cam_dir[2]};
  const Ray vray = generate_ray(cam_o, cam_d, (int)x, (int)y, a.frame_w, a.frame_h);
  const float dx = (float)a.X, dy = (float)a.Y, dz = (float)a.Z;

  bool cut_ok;
  f3 cut_point;
  if (!(within(vray.origin.x, dx) && within(vray.origin.y, dy) && within(vray.origin.z, dz))) {
    cut_ok = cut_box(dx, dy, dz, vray, cut_point);
  } else {
    cut_ok = true;
    cut_point = vray.origin;
  }

  bool hit = false;
  Ray current_ray{cut_point, vray.direction};
  uint32_t current_color = 0u;
  // (tried in round 3: the exit-certificate table on the camera ray at its entry point -- "no event in the box towards the octant's
  // corner" would make the pixel a miss without a march.  From the default pose that box nearly always holds the object: 0.100 ms with
  // and without, tools/ab_list.sh; not kept.  Also without effect: the certified fast environment lookup for the miss pixels (0.100 /
  // 0.100 ms).  Without the hit counter's atomic -- one returning atomic per wave with a hit, all on one address -- the kernel takes
  // 0.089 ms: the rest is the marches, four generations of waves deep)
  if (cut_ok) {
    int ev;
    current_ray = march_to_next_event<USE_GRAD>(vol, a.tf, current_ray, ev, current_color);
    hit = (ev == EV_HIT);
  }

  // wave-level compaction of the hits: one atomic per wave, prefix of the ballot per lane
  const unsigned long long hit_mask = __ballot(hit);
  uint32_t base = 0u;
  if (hit_mask != 0ull) {
    const int leader = __ffsll((long long)hit_mask) - 1;
    if ((int)lane == leader) base = atomicAdd(&a.counters[CTR_HITS], (uint32_t)__popcll(hit_mask));
    base = __shfl(base, leader);
  }

  // the coarse grid of the hull-certificate search below, once per wave that has a hit (the block is one wave)
  constexpr int kHullCoarse = kHullGrid / 4;
  __shared__ float4 hull_coarse[kHullCoarse * kHullCoarse];
  if (a.hull != nullptr && hit_mask != 0ull) {
    for (int c = (int)lane; c < kHullCoarse * kHullCoarse; c += 64)
      hull_coarse[c] = a.hull[((c / kHullCoarse) * 4 + 2) * kHullGrid + (c % kHullCoarse) * 4 + 2];
    __syncthreads();
  }

  int64_t raw_entry = -1;
  if (hit) {
    const uint32_t h = base + prefix_count(hit_mask);
    const f3 normal = -normalize3(gradient_nn(vol, current_ray.origin));
    raw_entry = cache_entry_of(a.X, a.Z, current_ray.origin);
    int64_t entry = raw_entry;
    if (a.mode == CLWH_ACCUM_VOXEL_CACHE && !(entry >= 0 && entry < a.cache_entries)) entry = -2;
    uint4 q0, q1, q2, q3;
    q0.x = __float_as_uint(current_ray.origin.x); q0.y = __float_as_uint(current_ray.origin.y);
    q0.z = __float_as_uint(current_ray.origin.z); q0.w = __float_as_uint(current_ray.direction.x);
    q1.x = __float_as_uint(current_ray.direction.y); q1.y = __float_as_uint(current_ray.direction.z);
    q1.z = __float_as_uint(normal.x); q1.w = __float_as_uint(normal.y);
    q2.x = __float_as_uint(normal.z); q2.y = current_color;
    q2.z = (uint32_t)((uint64_t)entry & 0xFFFFFFFFull); q2.w = (uint32_t)((uint64_t)entry >> 32);
    // start certificate (k_start_*, scene_kernels.hip): both distribution rays of every sample start from P = (origin + direction) +
    // normal * 2, formed with k_bounce's own operations; the table byte of P's voxel travels with the hit (three unsigned compares:
    // has P a voxel?  see k_bounce's step loop)
    uint32_t start_free = 0u;
    if (a.start_free) {
      const f3 p = (current_ray.origin + current_ray.direction) + normal * 2.0f;
      if (__float_as_uint(p.x) < __float_as_uint(dx) && __float_as_uint(p.y) < __float_as_uint(dy) && __float_as_uint(p.z) < __float_as_uint(dz))
        start_free = a.start_free[((size_t)(int)p.z * (size_t)a.Y + (size_t)(int)p.y) * (size_t)a.X + (size_t)(int)p.x];
    }
    // hull certificate (k_hull_*, scene_kernels.hip): a plane of the support table with the same P in front of it, by the largest margin
    // m = n_k . P - h_k the search finds -- every 4th cell of the octahedral grid in both directions first (the wave's copy in LDS,
    // above), then the 7 x 7 cells around the best of those.  The margin is concave in an unnormalised normal, so the second look
    // rarely misses the best plane, and any plane with m >= 0 is a valid one.  (The hit's own normal is a poor guide: central
    // differences on a voxelised surface are a dozen degrees off, and a plane that far from the tangent stands voxels behind P.)
    // The code lives beside the hit record, not in it.
    if (a.hull) {
      const f3 p = (current_ray.origin + current_ray.direction) + normal * 2.0f;
      float best = -INFINITY;  // (a NaN in P: every comparison fails, no plane)
      int bc = 0;
#pragma unroll 4
      for (int c = 0; c < kHullCoarse * kHullCoarse; ++c) {
        const float4 e = hull_coarse[c];
        const float m = ((e.x * p.x + e.y * p.y) + e.z * p.z) - e.w;
        if (m > best) { best = m; bc = c; }
      }
      int bi = (bc % kHullCoarse) * 4 + 2, bj = (bc / kHullCoarse) * 4 + 2;
      uint32_t code = 0u;
      float margin = best;
      const int i0 = bi, j0 = bj;
#pragma unroll 1
      for (int dj = -3; dj <= 3; ++dj)  // (rolled: unrolled, the forty-nine gathers cost the kernel three of its eight waves)
        for (int di = -3; di <= 3; ++di) {
          const int i = min(max(i0 + di, 0), kHullGrid - 1), j = min(max(j0 + dj, 0), kHullGrid - 1);
          const float4 e = a.hull[j * kHullGrid + i];
          const float m = ((e.x * p.x + e.y * p.y) + e.z * p.z) - e.w;
          if (m >= margin) { margin = m; bi = i; bj = j; }
        }
      // bits 0-12: 1 + the plane's index; bits 16-31: the margin in 1/256 voxels, rounded down (k_bounce needs its sign only)
      if (margin >= 0.0f) code = ((uint32_t)(bj * kHullGrid + bi) + 1u) | ((uint32_t)fminf(floorf(margin * 256.0f), 65535.0f) << 16);
      a.hull_codes[h] = code;
      // the second word: the same plane even when P lies up to kHullDeferDeficit behind it, with the signed margin
      // rounded down on a grid of 1 / kHullMarginScale (k_bounce grants a march once it has got in front); 0: a NaN in P (margin stays
      // -inf: the comparison fails), or no plane that near
      if (a.hull_planes) {
        uint32_t word = 0u;
        if (margin >= -kHullDeferDeficit) {
          const int q = (int)fminf(floorf(margin * (float)kHullMarginScale), 127.0f);  // (at least -kHullDeferDeficit * kHullMarginScale >= -128)
          word = ((uint32_t)(bj * kHullGrid + bi) + 1u) | (((uint32_t)q & 0xFFu) << 16);
        }
        a.hull_planes[h] = word;
      }
    }
    q3.x = x | (y << 16); q3.y = pslot; q3.z = start_free; q3.w = 0u;
    uint4 *dst = reinterpret_cast<uint4 *>(&a.hits[h]);
    dst[0] = q0; dst[1] = q1; dst[2] = q2; dst[3] = q3;
    a.pix_slot[pslot] = PIX_HIT | h;
  } else {
    // miss: environment colour of the camera ray (ray_marching.cl:172-178, 188-195)
    const uint32_t e = sample_environment_map(a.env, a.env_w, a.env_h, vray.direction);
    a.pix_slot[pslot] = e & 0x00FFFFFFu;
  }
  if (a.hit_index_out) a.hit_index_out[(size_t)y * (size_t)a.launch_w + x] = raw_entry;
}

// k_ao: compute_ao (ray_marching.cl:104-149) for every primary hit, the launch's passes one after the other in the
// hit's own lane.  The cache entry is one 32-bit word per voxel, samples | occluded << 16 (the reference's 2-ushort view,
// utility.cl:123-159).  The reference updates it with a plain read-modify-write that races between pixels sharing a
// voxel; here the sample is claimed and the occlusion recorded with integer atomics, i.e. the pixels are serialised,
// which is one legal outcome of that race and independent of the order while the count stays below the cap of 100.
template <bool USE_GRAD>
__global__ __launch_bounds__(256) void k_ao(const RenderArgs a) {
  const uint32_t n_hits = a.n_hits_on_device ? a.counters[CTR_HITS] : a.n_hits;
  const uint32_t h = blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= n_hits) return;
  const VolumePacked vol = make_volume(a);
  const uint4 *src = reinterpret_cast<const uint4 *>(&a.hits[h]);
  const uint4 q0 = src[0], q1 = src[1], q2 = src[2], q3 = src[3];
  const f3 hit_origin = f3{__uint_as_float(q0.x), __uint_as_float(q0.y), __uint_as_float(q0.z)};
  const f3 hit_direction = f3{__uint_as_float(q0.w), __uint_as_float(q1.x), __uint_as_float(q1.y)};
  const f3 normal = f3{__uint_as_float(q1.z), __uint_as_float(q1.w), __uint_as_float(q2.x)};
  const int64_t entry = (int64_t)(((uint64_t)q2.w << 32) | (uint64_t)q2.z);
  const uint32_t gx = q3.x & 0xFFFFu, gy = q3.x >> 16;
  if (entry < 0) return;  // outside the allocation: nothing is recorded
  uint32_t *word = a.cache + entry;
  for (int s = 0; s < a.n_seeds; ++s) {
    // `if (buffer_value.x < 100) buffer_value.x += 1`: claim a sample, give it back if the cap was already reached
    const uint32_t old = atomicAdd(word, 1u);
    uint32_t granted = 1u, occluded = 0u;
    if ((old & 0xFFFFu) >= 100u) {
      atomicSub(word, 1u);
      granted = 0u;
    } else {
      // ray_bounce (utility_ray.cl:100-103), seven unclassified steps, then the occlusion march
      Ray r{hit_origin + hit_direction, hemisphere_direction(gx, gy, normal, a.seeds[s])};
      for (int k = 0; k < 7; ++k) {
        const int sd = (int)(vol.step_i(f2i(r.origin.x), f2i(r.origin.y), f2i(r.origin.z)) & 0x7Fu);
        r.origin = r.origin + r.direction * cl_max((float)sd, 0.5f);
      }
      int ev;
      uint32_t color = 0u;
      march_to_next_event<USE_GRAD>(vol, a.tf, r, ev, color);
      if (ev == EV_HIT) {
        atomicAdd(word, 0x10000u);
        occluded = 1u;
      }
    }
    if (a.contrib_out) {
      uint32_t *q = a.contrib_out + ((size_t)gy * (size_t)a.launch_w + gx) * 4;
      q[0] = occluded; q[1] = 0u; q[2] = 0u; q[3] = granted;
    }
  }
}

hipError_t launch_primary(const RenderArgs &a, hipStream_t s) {
  if (a.tf.uses_gradient)
    hipLaunchKernelGGL(k_primary<true>, dim3(a.num_tile_slots), dim3(64), 0, s, a);
  else
    hipLaunchKernelGGL(k_primary<false>, dim3(a.num_tile_slots), dim3(64), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_ao(const RenderArgs &a, hipStream_t s) {
  if (a.n_hits == 0) return hipSuccess;
  const dim3 grid((a.n_hits + 255u) / 256u), block(256);
  if (a.tf.uses_gradient) hipLaunchKernelGGL(k_ao<true>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(k_ao<false>, grid, block, 0, s, a);
  return hipGetLastError();
}

}  // namespace clvr
