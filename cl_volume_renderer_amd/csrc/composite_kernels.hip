// composite_kernels.hip -- direct volume rendering: emission-absorption compositing of a camera ray's kept samples, front to back,
// through a colour/opacity table (clwh_render_composite).  The sample set, the bricked int16 copy of the volume and the brick walk
// are the projections' (projection_device.hpp, k_proj_repack); the arithmetic per sample is the contract's (include/clwh.h), in
// float32 without contraction, so the result can be tested bit for bit.
//
//   k_comp_prefix            the table's derived data: prefix[i] = number of entries j <= i with a > 0.  The entries a brick's voxels
//                            can map to are the index range [clamp(min - lut_first), clamp(max - lut_first)] (clamping is monotone),
//                            and prefix[hi] - prefix[lo - 1] == 0 says that none of them contributes.
//   k_composite<SHADE, SKIP> one wave per 8x8 pixel tile, tiles in XCD-contiguous order (as k_projection); each lane walks its ray's
//                            kept range brick by brick and stops at the first sample that takes A to alpha_stop.  SKIP (without
//                            CLWH_COMP_DENSE): a brick none of whose possible entries has a > 0 is stepped over without reading it --
//                            every sample in it is a no-op by step 1 of the contract, so the bytes are the dense walk's.  SHADE: six
//                            more voxels (clamped central differences, possibly in neighbouring bricks) for contributing samples only.
#include "projection_device.hpp"

namespace clvr {

constexpr unsigned kCompPrefixThreads = 1024;
__global__ __launch_bounds__(kCompPrefixThreads) void k_comp_prefix(const float4 *__restrict__ lut, int32_t lut_len, uint32_t *__restrict__ prefix) {
  __shared__ uint32_t s_sum[kCompPrefixThreads];
  const unsigned tid = threadIdx.x;
  const int chunk = (lut_len + (int)kCompPrefixThreads - 1) / (int)kCompPrefixThreads;  // consecutive entries per thread, <= 64
  const int i0 = (int)tid * chunk, i1 = min(i0 + chunk, lut_len);
  uint32_t mine = 0u;
  for (int i = i0; i < i1; ++i) mine += lut[i].w > 0.0f ? 1u : 0u;
  s_sum[tid] = mine;
  __syncthreads();
  for (unsigned s = 1u; s < kCompPrefixThreads; s <<= 1) {  // inclusive scan of the per-thread counts
    const uint32_t add = tid >= s ? s_sum[tid - s] : 0u;
    __syncthreads();
    s_sum[tid] += add;
    __syncthreads();
  }
  uint32_t run = s_sum[tid] - mine;
  for (int i = i0; i < i1; ++i) {
    run += lut[i].w > 0.0f ? 1u : 0u;
    prefix[i] = run;
  }
}

__device__ __forceinline__ int comp_lut_index(int v, int lut_first, int lut_len) { return min(max(v - lut_first, 0), lut_len - 1); }
__device__ __forceinline__ uint32_t comp_quantise(float x) { return (uint32_t)(int)fminf(fmaxf(x * 255.0f + 0.5f, 0.0f), 255.0f); }
// IEEE 754 leaves a NaN's sign and payload to the implementation; the contract stores every NaN as 0x7FC00000
__device__ __forceinline__ float comp_canonical(float x) { return x == x ? x : __builtin_nanf(""); }

template <bool SHADE, bool SKIP>
__global__ __launch_bounds__(64) void k_composite(const CompArgs a) {
  const uint32_t slot = xcd_contiguous_slot(blockIdx.x, (uint32_t)a.num_tiles);
  const uint32_t tx = slot % (uint32_t)a.tiles_x, ty = slot / (uint32_t)a.tiles_x;
  const uint32_t lane = threadIdx.x;
  const uint32_t x = tx * 8u + (lane & 7u), y = ty * 8u + (lane >> 3);

  const f3 cam_o = f3{a.cam_pos[0], a.cam_pos[1], a.cam_pos[2]};
  const f3 cam_d = f3{a.cam_dir[0], a.cam_dir[1], a.cam_dir[2]};
  const Ray ray = generate_ray(cam_o, cam_d, (int)x, (int)y, a.frame_w, a.frame_h);
  const ProjRay r{ray.origin, ray.direction, a.step, a.t_near, a.t_far, (float)a.X, (float)a.Y, (float)a.Z};

  float cr = 0.0f, cg = 0.0f, cb = 0.0f, A = 0.0f;
  float t_first = __builtin_nanf(""), t_stop = __builtin_nanf("");
  bool any = false;
  int k, kb;
  if (proj_kept_range(r, a.k_cap, k, kb)) {
    bool stopped = false;
    while (k <= kb && !stopped) {  // one brick per iteration, front to back
      float t;
      const f3 p = proj_sample(r, k, t);  // kept: 0 <= p < dim, so the conversions are floors
      const unsigned bx = (unsigned)(int)p.x >> 3, by = (unsigned)(int)p.y >> 3, bz = (unsigned)(int)p.z >> 3;
      const size_t brick = ((size_t)bz * (size_t)a.NBY + (size_t)by) * (size_t)a.NBX + (size_t)bx;
      const int k_end = proj_brick_exit(r, k, kb, bx, by, bz, a.k_cap);
      bool skip = false;
      if constexpr (SKIP) {
        const uint32_t mm = a.table[brick];
        const int lo = comp_lut_index((int)(int16_t)(mm & 0xFFFFu), a.lut_first, a.lut_len);
        const int hi = comp_lut_index((int)(int16_t)(mm >> 16), a.lut_first, a.lut_len);
        skip = a.prefix[hi] == (lo > 0 ? a.prefix[lo - 1] : 0u);
      }
      if (!skip) {
        const int16_t *__restrict__ b = a.bricks + (brick << 9);
        for (int j = k; j < k_end; ++j) {
          float tj;
          const f3 q = proj_sample(r, j, tj);
          const unsigned ux = (unsigned)(int)q.x, uy = (unsigned)(int)q.y, uz = (unsigned)(int)q.z;
          const int v = b[VolumePacked::inner_index(ux, uy, uz)];
          const float4 e = a.lut[comp_lut_index(v, a.lut_first, a.lut_len)];
          if (!(e.w > 0.0f)) continue;  // (also NaN) the sample changes nothing
          float er = e.x, eg = e.y, eb = e.z;
          if constexpr (SHADE) {
            const int ix = (int)ux, iy = (int)uy, iz = (int)uz;
            const int xm = max(ix - 1, 0), xp = min(ix + 1, a.X - 1), ym = max(iy - 1, 0), yp = min(iy + 1, a.Y - 1);
            const int zm = max(iz - 1, 0), zp = min(iz + 1, a.Z - 1);
            const int16_t *__restrict__ vb = a.bricks;
            const float gx = (float)((int)vb[VolumePacked::record_index(xp, iy, iz, a.NBX, a.NBY)] - (int)vb[VolumePacked::record_index(xm, iy, iz, a.NBX, a.NBY)]);
            const float gy = (float)((int)vb[VolumePacked::record_index(ix, yp, iz, a.NBX, a.NBY)] - (int)vb[VolumePacked::record_index(ix, ym, iz, a.NBX, a.NBY)]);
            const float gz = (float)((int)vb[VolumePacked::record_index(ix, iy, zp, a.NBX, a.NBY)] - (int)vb[VolumePacked::record_index(ix, iy, zm, a.NBX, a.NBY)]);
            const float l2 = (gx * gx + gy * gy) + gz * gz;
            float s = 1.0f;
            if (l2 > 0.0f) {
              const float c = fabsf((gx * r.d.x + gy * r.d.y) + gz * r.d.z) / sqrtf(l2);
              s = a.ambient + (1.0f - a.ambient) * fminf(c, 1.0f);
            }
            er = er * s;
            eg = eg * s;
            eb = eb * s;
          }
          const float w = (1.0f - A) * e.w;
          cr = cr + w * er;
          cg = cg + w * eg;
          cb = cb + w * eb;
          A = A + w;
          if (!any) {
            any = true;
            t_first = tj;
          }
          if (A >= a.alpha_stop) {
            t_stop = tj;
            stopped = true;
            break;
          }
        }
      }
      k = k_end;
    }
  }
  a.frame[(size_t)y * (size_t)a.frame_w + x] = comp_quantise(cr) | (comp_quantise(cg) << 8) | (comp_quantise(cb) << 16) | (comp_quantise(A) << 24);
  const size_t o = (size_t)y * (size_t)a.launch_w + x;
  if (a.rgba) a.rgba[o] = float4{comp_canonical(cr), comp_canonical(cg), comp_canonical(cb), comp_canonical(A)};
  if (a.t_first) a.t_first[o] = t_first;
  if (a.t_stop) a.t_stop[o] = t_stop;
}

hipError_t launch_comp_prefix(const float4 *lut, int32_t lut_len, uint32_t *prefix, hipStream_t s) {
  hipLaunchKernelGGL(k_comp_prefix, dim3(1), dim3(kCompPrefixThreads), 0, s, lut, lut_len, prefix);
  return hipGetLastError();
}

hipError_t launch_composite(const CompArgs &a, bool shade, bool dense, hipStream_t s) {
  const dim3 grid((unsigned)a.num_tiles), block(64);
  if (shade && dense)
    hipLaunchKernelGGL((k_composite<true, false>), grid, block, 0, s, a);
  else if (shade)
    hipLaunchKernelGGL((k_composite<true, true>), grid, block, 0, s, a);
  else if (dense)
    hipLaunchKernelGGL((k_composite<false, false>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((k_composite<false, true>), grid, block, 0, s, a);
  return hipGetLastError();
}

}  // namespace clvr
