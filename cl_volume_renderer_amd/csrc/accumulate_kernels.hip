// accumulate_kernels.hip -- where the samples of the `render` pass end up: k_commit, the planned voxel-cache launches, k_env_fixup, the resolves
#include "bounce_device.hpp"

namespace clvr {

// fold one launch's per-hit deltas into the float4 accumulation buffer (one lane per hit = per pixel)
__global__ __launch_bounds__(256) void k_commit(const RenderArgs a) {
  const uint32_t h = blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= (a.n_hits_on_device ? a.counters[CTR_HITS] : a.n_hits)) return;
  const unsigned long long d = a.delta[h];
  if (d == 0ull) return;
  a.delta[h] = 0ull;  // ready for the next launch: the host never clears the deltas (it does not know how many there are)
  const uint32_t pslot = a.hits[h].pslot;
  float4 acc = a.accum[pslot];
  // integer-valued floats below 2^24: exact
  acc.x += (float)(uint32_t)(d & 0xFFFFull);
  acc.y += (float)(uint32_t)((d >> 16) & 0xFFFFull);
  acc.z += (float)(uint32_t)((d >> 32) & 0xFFFFull);
  acc.w += (float)(uint32_t)(d >> 48);
  a.accum[pslot] = acc;
}

// Planned voxel-cache launches.  The reference takes a token per sample with an atomic on the voxel's entry and adds the sample with
// two more (utility.cl:20-54).  With the seeds of a launch fused, the 64 samples of a pixel -- and those of every other pixel that hit
// the same voxel -- do that to ONE 8-byte entry at the same time: 17.2 ms for the launch that takes 3.9 ms in image space.  Which
// samples get a voxel's remaining tokens is unspecified in the reference (whoever reaches the atomic first); how many is not:
// min(requests, 256 - count).  So the tokens are dealt out before the launch: the camera's hits are grouped by voxel once (a stable
// sort of their cache entries), k_vox_grant walks each group and gives hit after hit as many of the launch's seeds as the voxel has
// tokens left, adds the tokens to the entry's count, and the launch runs without a single atomic on the cache: a granted sample
// accumulates into its hit's 64-bit delta like an image-space sample, and k_commit_voxel adds each hit's sum to its voxel with two
// atomics per hit instead of three per sample.  Counts are exact, entries below the cap equal the reference's bit for bit.
__global__ __launch_bounds__(256) void k_vox_keys(const RenderArgs a, int64_t *__restrict__ keys, uint32_t *__restrict__ iota, uint32_t n) {
  const uint32_t h = blockIdx.x * 256u + threadIdx.x;
  if (h >= n) return;
  int64_t key = kVoxKeyNone;
  if (h < a.counters[CTR_HITS]) {
    const HitRec &r = a.hits[h];
    const int64_t e = (int64_t)(((uint64_t)(uint32_t)r.entry_hi << 32) | (uint64_t)(uint32_t)r.entry_lo);
    key = e >= 0 ? e : kVoxKeyInvalid;
  }
  keys[h] = key;
  iota[h] = h;
}

// one lane per sorted position; the lane at the head of a voxel's group deals the launch's tokens to the group's hits, in hit order
__global__ __launch_bounds__(256) void k_vox_grant(const RenderArgs a, const int64_t *__restrict__ keys, const uint32_t *__restrict__ order,
                                                   uint32_t n, uint32_t *__restrict__ grants) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const int64_t e = keys[i];
  if (e >= kVoxKeyInvalid) {
    if (e == kVoxKeyInvalid) grants[order[i]] = 0u;  // the hit lies outside the cache: never a token
    return;
  }
  if (i > 0u && keys[i - 1] == e) return;
  uint32_t *word1 = a.cache + 2 * e + 1;
  const uint32_t w1 = *word1;
  const uint32_t count = w1 >> 16;
  uint32_t remaining = count < 256u ? 256u - count : 0u, dealt = 0u;
  for (uint32_t j = i; j < n && keys[j] == e; ++j) {
    const uint32_t g = min((uint32_t)a.n_seeds, remaining);
    grants[order[j]] = g;
    remaining -= g;
    dealt += g;
  }
  *word1 = w1 + (dealt << 16);  // the tokens (utility.cl:28-31); the sums follow in k_commit_voxel
}

__global__ __launch_bounds__(256) void k_commit_voxel(const RenderArgs a) {
  const uint32_t h = blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= (a.n_hits_on_device ? a.counters[CTR_HITS] : a.n_hits)) return;
  const unsigned long long d = a.delta[h];
  if (d == 0ull) return;
  a.delta[h] = 0ull;
  const HitRec &r = a.hits[h];
  const int64_t e = (int64_t)(((uint64_t)(uint32_t)r.entry_hi << 32) | (uint64_t)(uint32_t)r.entry_lo);
  // <= 256 contributions of <= 255 per voxel in total: no lane carries (the count was added by k_vox_grant)
  atomicAdd(a.cache + 2 * e, (uint32_t)(d & 0xFFFFull) | ((uint32_t)((d >> 16) & 0xFFFFull) << 16));
  atomicAdd(a.cache + 2 * e + 1, (uint32_t)((d >> 32) & 0xFFFFull));
}

// k_env_fixup: one lane per fix-up record; exact lookups, then the reference's arithmetic in its order
template <int MODE>
__global__ __launch_bounds__(256) void k_env_fixup(const RenderArgs a) {
  uint32_t n = a.counters[CTR_FIXUPS];
  if (n > a.fixup_capacity) n = a.fixup_capacity;
  for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
    const uint32_t *rec = a.fixups + (size_t)k * kFixupDwords;
    const uint32_t hit = rec[0];
    const int64_t entry = (int64_t)(((uint64_t)rec[2] << 32) | (uint64_t)rec[1]);
    const uint32_t gx = rec[3] & 0xFFFFu, gy = rec[3] >> 16;
    uint32_t bv_r = rec[4], bv_g = rec[5], bv_b = rec[6];
    const uint32_t npend = rec[7];
    for (uint32_t q = 0; q < npend && q < 2u; ++q) {
      const uint32_t *e = rec + 8 + 7 * q;
      const float p_r = __uint_as_float(e[0]), p_g = __uint_as_float(e[1]), p_b = __uint_as_float(e[2]);
      const float factor = __uint_as_float(e[3]);
      const f3 d = f3{__uint_as_float(e[4]), __uint_as_float(e[5]), __uint_as_float(e[6])};
      const uint32_t light = sample_environment_map(a.env, a.env_w, a.env_h, d);
      bv_r = f2u((float)bv_r + p_r * (float)(light & 255u) * factor / 1.0f);
      bv_g = f2u((float)bv_g + p_g * (float)((light >> 8) & 255u) * factor / 1.0f);
      bv_b = f2u((float)bv_b + p_b * (float)((light >> 16) & 255u) * factor / 1.0f);
    }
    finish_item<MODE>(a, entry, hit, gx, gy, bv_r, bv_g, bv_b);
  }
}

// resolve: every pixel of this rank reads its accumulator after the whole pass (ray_marching.cl:82-99)
__global__ __launch_bounds__(64) void k_resolve(const RenderArgs a) {
  const uint32_t slot = blockIdx.x;
  int tx, ty;
  if (!tile_from_slot(a, slot, tx, ty)) return;
  const uint32_t lane = threadIdx.x;
  const uint32_t x = (uint32_t)tx * 8u + (lane & 7u);
  const uint32_t y = (uint32_t)ty * 8u + (lane >> 3);
  if (x >= (uint32_t)a.frame_w || y >= (uint32_t)a.frame_h) return;
  const uint32_t pslot = slot * 64u + lane;
  const uint32_t ps = a.pix_slot[pslot];
  uint32_t out;
  if (!(ps & PIX_HIT)) {
    out = (ps & 0x00FFFFFFu) | (200u << 24);  // miss: environment colour, alpha 200
  } else if (a.shading == CLWH_SHADE_AO) {
    // compute_ao's return value (ray_marching.cl:145-148): {v, v, v} with v = (100 - occluded) * 2; shown with alpha 1
    const HitRec &h = a.hits[ps & ~PIX_HIT];
    const int64_t e = (int64_t)(((uint64_t)(uint32_t)h.entry_hi << 32) | (uint64_t)(uint32_t)h.entry_lo);
    const uint32_t v = e < 0 ? 200u : (100u - (a.cache[e] >> 16)) * 2u;
    out = v | (v << 8) | (v << 16) | (1u << 24);
  } else if (a.mode == CLWH_ACCUM_VOXEL_CACHE) {
    const HitRec &h = a.hits[ps & ~PIX_HIT];
    const int64_t e = (int64_t)(((uint64_t)(uint32_t)h.entry_hi << 32) | (uint64_t)(uint32_t)h.entry_lo);
    if (e < 0) {
      out = 1u << 24;
    } else {
      const uint2 w = *reinterpret_cast<const uint2 *>(a.cache + e * 2);
      out = tone_map_rgba8(w.x & 0xFFFFu, w.x >> 16, w.y & 0xFFFFu, w.y >> 16);
    }
  } else {
    const float4 acc = a.accum[pslot];
    out = tone_map_rgba8((uint32_t)acc.x, (uint32_t)acc.y, (uint32_t)acc.z, (uint32_t)acc.w);
  }
  a.frame[(size_t)y * a.frame_w + x] = out;
}

// gathered image-space accumulation (all ranks' tile-major buffers back to back) -> RGBA8 frame
__global__ __launch_bounds__(64) void k_accum_resolve(const RenderArgs a, const float4 *__restrict__ accum_all) {
  const int tx = (int)(blockIdx.x % (unsigned)a.tiles_x), ty = (int)(blockIdx.x / (unsigned)a.tiles_x);
  const int owner = (tx + ty) % a.tile_world;
  const size_t slot = (size_t)ty * a.tiles_per_row + (size_t)(tx / a.tile_world);
  const size_t per_rank = (size_t)a.tiles_y * a.tiles_per_row * 64u;
  const uint32_t lane = threadIdx.x;
  const float4 acc = accum_all[(size_t)owner * per_rank + slot * 64u + lane];
  const uint32_t x = (uint32_t)tx * 8u + (lane & 7u), y = (uint32_t)ty * 8u + (lane >> 3);
  if (x >= (uint32_t)a.frame_w || y >= (uint32_t)a.frame_h) return;
  uint32_t out;
  if (acc.w == 0.0f) {
    const f3 cam_o = f3{a.cam_pos[0], a.cam_pos[1], a.cam_pos[2]};
    const f3 cam_d = f3{a.cam_dir[0], a.cam_dir[1], a.cam_dir[2]};
    const Ray vray = generate_ray(cam_o, cam_d, (int)x, (int)y, a.frame_w, a.frame_h);
    const uint32_t e = sample_environment_map(a.env, a.env_w, a.env_h, vray.direction);
    out = (e & 0x00FFFFFFu) | (200u << 24);
  } else {
    out = tone_map_rgba8((uint32_t)acc.x, (uint32_t)acc.y, (uint32_t)acc.z, (uint32_t)acc.w);
  }
  a.frame[(size_t)y * a.frame_w + x] = out;
}

// The multi-GPU form of the same resolve: a rank resolves ITS tiles to RGBA8 first (tile-major, the slot order of its
// accumulation buffer), the ranks exchange 4 bytes per pixel instead of 16, and k_frame_from_tiles puts the tiles in place.
__global__ __launch_bounds__(64) void k_accum_resolve_tiles(const RenderArgs a, const float4 *__restrict__ accum, uint32_t *__restrict__ tiles_out) {
  const uint32_t slot = blockIdx.x, lane = threadIdx.x;
  int tx, ty;
  const bool exists = tile_from_slot(a, slot, tx, ty);  // the last slots of a row may lie beyond the frame
  const uint32_t x = (uint32_t)tx * 8u + (lane & 7u), y = (uint32_t)ty * 8u + (lane >> 3);
  uint32_t out = 0u;
  if (exists && x < (uint32_t)a.frame_w && y < (uint32_t)a.frame_h) {
    const float4 acc = accum[(size_t)slot * 64u + lane];
    if (acc.w == 0.0f) {
      const f3 cam_o = f3{a.cam_pos[0], a.cam_pos[1], a.cam_pos[2]};
      const f3 cam_d = f3{a.cam_dir[0], a.cam_dir[1], a.cam_dir[2]};
      const Ray vray = generate_ray(cam_o, cam_d, (int)x, (int)y, a.frame_w, a.frame_h);
      const uint32_t e = sample_environment_map(a.env, a.env_w, a.env_h, vray.direction);
      out = (e & 0x00FFFFFFu) | (200u << 24);
    } else {
      out = tone_map_rgba8((uint32_t)acc.x, (uint32_t)acc.y, (uint32_t)acc.z, (uint32_t)acc.w);
    }
  }
  tiles_out[(size_t)slot * 64u + lane] = out;
}

__global__ __launch_bounds__(64) void k_frame_from_tiles(const RenderArgs a, const uint32_t *__restrict__ tiles_all) {
  const int tx = (int)(blockIdx.x % (unsigned)a.tiles_x), ty = (int)(blockIdx.x / (unsigned)a.tiles_x);
  const int owner = (tx + ty) % a.tile_world;
  const size_t slot = (size_t)ty * a.tiles_per_row + (size_t)(tx / a.tile_world);
  const size_t per_rank = (size_t)a.tiles_y * a.tiles_per_row * 64u;
  const uint32_t lane = threadIdx.x;
  const uint32_t x = (uint32_t)tx * 8u + (lane & 7u), y = (uint32_t)ty * 8u + (lane >> 3);
  if (x >= (uint32_t)a.frame_w || y >= (uint32_t)a.frame_h) return;
  a.frame[(size_t)y * a.frame_w + x] = tiles_all[(size_t)owner * per_rank + slot * 64u + lane];
}

// finish the samples whose environment lookups the fast path could not certify
hipError_t launch_env_fixup(const RenderArgs &a, hipStream_t s) {
  if ((uint64_t)a.n_hits * (uint64_t)a.n_seeds == 0) return hipSuccess;  // n_hits is the pixel count when the real one is on the device
  // (the record count is on the device: a grid-stride loop; a 64-seed launch leaves tens of thousands of records of binary64 work:
  // 47.6 us on 64 blocks, 19.6 on 256, 20.2 on 1024)
  const unsigned blocks = a.n_seeds > 1 ? 256u : 64u;
  if (a.mode == CLWH_ACCUM_VOXEL_CACHE)
    hipLaunchKernelGGL(k_env_fixup<CLWH_ACCUM_VOXEL_CACHE>, dim3(blocks), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(k_env_fixup<CLWH_ACCUM_IMAGE_SPACE>, dim3(blocks), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_commit(const RenderArgs &a, hipStream_t s) {
  if (a.n_hits == 0 || a.mode != CLWH_ACCUM_IMAGE_SPACE) return hipSuccess;
  hipLaunchKernelGGL(k_commit, dim3((a.n_hits + 255u) / 256u), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_vox_keys(const RenderArgs &a, int64_t *keys, uint32_t *iota, uint32_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_vox_keys, dim3((n + 255u) / 256u), dim3(256), 0, s, a, keys, iota, n);
  return hipGetLastError();
}
hipError_t launch_vox_grant(const RenderArgs &a, const int64_t *sorted_keys, const uint32_t *order, uint32_t n, uint32_t *grants, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_vox_grant, dim3((n + 255u) / 256u), dim3(256), 0, s, a, sorted_keys, order, n, grants);
  return hipGetLastError();
}
hipError_t launch_commit_voxel(const RenderArgs &a, hipStream_t s) {
  if (a.n_hits == 0) return hipSuccess;
  hipLaunchKernelGGL(k_commit_voxel, dim3((a.n_hits + 255u) / 256u), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_resolve(const RenderArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_resolve, dim3(a.num_tile_slots), dim3(64), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_accum_resolve_tiles(const RenderArgs &a, const float4 *accum, uint32_t *tiles_out, hipStream_t s) {
  hipLaunchKernelGGL(k_accum_resolve_tiles, dim3((uint32_t)(a.tiles_y * a.tiles_per_row)), dim3(64), 0, s, a, accum, tiles_out);
  return hipGetLastError();
}
hipError_t launch_frame_from_tiles(const RenderArgs &a, const uint32_t *tiles_all, hipStream_t s) {
  hipLaunchKernelGGL(k_frame_from_tiles, dim3((uint32_t)(a.tiles_x * a.tiles_y)), dim3(64), 0, s, a, tiles_all);
  return hipGetLastError();
}
hipError_t launch_accum_resolve(const RenderArgs &a, const float4 *accum_all, hipStream_t s) {
  hipLaunchKernelGGL(k_accum_resolve, dim3((uint32_t)(a.tiles_x * a.tiles_y)), dim3(64), 0, s, a, accum_all);
  return hipGetLastError();
}

}  // namespace clvr
