// composite_kernels.hip -- direct volume rendering: emission-absorption compositing of a camera ray's kept samples, front to back,
// through a colour/opacity table (clwh_render_composite).  The sample set and the brick walk are the views' (view_device.hpp), the
// bricked int16 copy of the volume is k_proj_repack's; the arithmetic per sample is the contract's (include/clwh.h), in
// float32 without contraction, so the result can be tested bit for bit.
//
//   k_comp_prefix            the table's derived data: prefix[i] = number of entries j <= i with a > 0.  The entries a brick's voxels
//                            can map to are the index range [clamp(min - lut_first), clamp(max - lut_first)] (clamping is monotone),
//                            and prefix[hi] - prefix[lo - 1] == 0 says that none of them contributes.
//   k_composite<SHADE, SKIP> one wave per 8x8 pixel tile (view_pixel); each lane walks its ray's kept range brick by brick
//                            (walk_bricks) and stops at the first sample that takes A to alpha_stop.  SKIP (without
//                            CLWH_COMP_DENSE): a brick none of whose possible entries has a > 0 is stepped over without reading it --
//                            every sample in it is a no-op by step 1 of the contract, so the bytes are the dense walk's.  SHADE: six
//                            more voxels (clamped central differences, possibly in neighbouring bricks) for contributing samples only.
#include "view_device.hpp"

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
template <bool SHADE, bool SKIP>
__global__ __launch_bounds__(64) void k_composite(const CompArgs a) {
  uint32_t x, y;
  view_pixel(a.fr, x, y);
  const ProjRay r = camera_ray(a.cam, a.vol, a.fr, x, y);

  float cr = 0.0f, cg = 0.0f, cb = 0.0f, A = 0.0f;
  float t_first = __builtin_nanf(""), t_stop = __builtin_nanf("");
  bool any = false;
  int k, kb;
  if (proj_kept_range(r, a.cam.k_cap, k, kb)) {
    walk_bricks(
        r, a.vol, k, kb, a.cam.k_cap, NeverSkip{},
        [&](size_t brick) {
          if constexpr (SKIP) {
            const uint32_t mm = a.vol.table[brick];
            const int lo = comp_lut_index(table_min(mm), a.lut_first, a.lut_len);
            const int hi = comp_lut_index(table_max(mm), a.lut_first, a.lut_len);
            return a.prefix[hi] == (lo > 0 ? a.prefix[lo - 1] : 0u);
          } else {
            return false;
          }
        },
        [&](size_t brick, int k0, int k_end) {
          const int16_t *__restrict__ b = a.vol.bricks + (brick << 9);
          for (int j = k0; j < k_end; ++j) {
            float tj;
            const f3 q = proj_sample(r, j, tj);
            const unsigned ux = (unsigned)(int)q.x, uy = (unsigned)(int)q.y, uz = (unsigned)(int)q.z;
            const int v = b[VolumePacked::inner_index(ux, uy, uz)];
            const float4 e = a.lut[comp_lut_index(v, a.lut_first, a.lut_len)];
            if (!(e.w > 0.0f)) continue;  // (also NaN) the sample changes nothing
            float er = e.x, eg = e.y, eb = e.z;
            if constexpr (SHADE) {
              int dx, dy, dz;
              central_difference(a.vol, (int)ux, (int)uy, (int)uz, dx, dy, dz);
              const float gx = (float)dx, gy = (float)dy, gz = (float)dz;
              const float l2 = length2(gx, gy, gz);
              const float s = l2 > 0.0f ? headlight(gx, gy, gz, sqrtf(l2), r.d, a.ambient) : 1.0f;
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
              return true;
            }
          }
          return false;
        });
  }
  const size_t o = store_frame(a.fr, x, y, quantise_unorm8(cr) | (quantise_unorm8(cg) << 8) | (quantise_unorm8(cb) << 16) | (quantise_unorm8(A) << 24));
  store_optional(a.rgba, o, float4{canonical_nan(cr), canonical_nan(cg), canonical_nan(cb), canonical_nan(A)});
  store_optional(a.t_first, o, t_first);
  store_optional(a.t_stop, o, t_stop);
}

hipError_t launch_comp_prefix(const float4 *lut, int32_t lut_len, uint32_t *prefix, hipStream_t s) {
  hipLaunchKernelGGL(k_comp_prefix, dim3(1), dim3(kCompPrefixThreads), 0, s, lut, lut_len, prefix);
  return hipGetLastError();
}

hipError_t launch_composite(const CompArgs &a, bool shade, bool dense, hipStream_t s) {
  const dim3 grid((unsigned)a.fr.num_tiles), block(64);
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
