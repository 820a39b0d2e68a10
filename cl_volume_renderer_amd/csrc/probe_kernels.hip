// probe_kernels.hip -- the render path's device functions, one by one: clwh_debug_device_probe (include/clwh.h).
//
// One lane per record calls the product function named by `which` with the record's words as arguments and stores what it
// returns.  The functions are the ones k_primary / k_bounce / k_resolve call, included from the product headers and left as
// they are; this file holds no arithmetic of its own.  tests/test_gpu_device_functions.py compares every word with the
// oracle (or, for the plain arithmetic, with numpy's binary32 operations in the order written).  The C entry, with its
// checks of handles and sizes, stands with the other diagnostics in clwh_render.hip.
#include "bounce_device.hpp"

namespace clvr {

// words per record, index = enum clwh_probe
__host__ __device__ __forceinline__ ProbeShape probe_shape_of(int which) {
  switch (which) {
    case CLWH_PROBE_ARITH: return {6u, 12u};
    case CLWH_PROBE_HASH: return {1u, 1u};
    case CLWH_PROBE_HEMISPHERE: return {7u, 6u};
    case CLWH_PROBE_RAY: return {10u, 3u};
    case CLWH_PROBE_CUT: return {6u, 4u};
    case CLWH_PROBE_ENV_EXACT: return {3u, 1u};
    case CLWH_PROBE_ENV_FAST: return {3u, 2u};
    case CLWH_PROBE_ENV_APPROX: return {3u, 2u};
    case CLWH_PROBE_TONE: return {4u, 1u};
    case CLWH_PROBE_TAPS: return {3u, 3u};
    case CLWH_PROBE_HULL: return {5u, 5u};
    default: return {0u, 0u};
  }
}

struct ProbeParams {
  int32_t v[4];
};

__device__ __forceinline__ f3 f3_at(const uint32_t *r) {
  return f3{__uint_as_float(r[0]), __uint_as_float(r[1]), __uint_as_float(r[2])};
}
__device__ __forceinline__ void put_f3(uint32_t *o, f3 v) {
  o[0] = __float_as_uint(v.x);
  o[1] = __float_as_uint(v.y);
  o[2] = __float_as_uint(v.z);
}

__global__ __launch_bounds__(256) void k_debug_device_probe(int which, const uint32_t *__restrict__ in, uint64_t n,
                                                            uint32_t *__restrict__ out, const uint32_t *__restrict__ aux,
                                                            ProbeParams params) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const ProbeShape shape = probe_shape_of(which);
  const uint32_t *r = in + i * shape.in_words;
  uint32_t *o = out + i * shape.out_words;
  switch (which) {
    case CLWH_PROBE_ARITH: {
      const f3 a = f3_at(r), b = f3_at(r + 3);
      o[0] = __float_as_uint(a.x / b.x);
      o[1] = __float_as_uint(sqrtf(a.x));
      o[2] = __float_as_uint(dot3(a, b));
      o[3] = __float_as_uint(length3(a));
      put_f3(o + 4, normalize3(a));
      put_f3(o + 7, cross3(a, b));
      o[10] = __float_as_uint(cl_min(a.x, b.x));
      o[11] = __float_as_uint(cl_max(a.x, b.x));
      break;
    }
    case CLWH_PROBE_HASH: o[0] = hash_u32(r[0]); break;
    case CLWH_PROBE_HEMISPHERE: {
      const f3 normal = f3_at(r + 2);
      const int seed = (int)r[5];
      put_f3(o, hemisphere_reflective(r[0], r[1], normal, seed, __uint_as_float(r[6])));
      put_f3(o + 3, hemisphere_direction(r[0], r[1], normal, seed));
      break;
    }
    case CLWH_PROBE_RAY: {
      const Ray ray = generate_ray(f3_at(r), f3_at(r + 3), (int)r[6], (int)r[7], (int)r[8], (int)r[9]);
      put_f3(o, ray.direction);
      break;
    }
    case CLWH_PROBE_CUT: {
      f3 point;
      const bool hit = cut_box((float)params.v[0], (float)params.v[1], (float)params.v[2], Ray{f3_at(r), f3_at(r + 3)}, point);
      o[0] = hit ? 1u : 0u;
      put_f3(o + 1, point);
      break;
    }
    case CLWH_PROBE_ENV_EXACT: o[0] = sample_environment_map(aux, params.v[0], params.v[1], f3_at(r)); break;
    case CLWH_PROBE_ENV_FAST: {
      uint32_t texel = 0xFFFFFFFFu;
      const bool decided = sample_environment_map_fast(aux, params.v[0], params.v[1], f3_at(r), texel);
      o[0] = decided ? 1u : 0u;
      o[1] = decided ? texel : 0xFFFFFFFFu;
      break;
    }
    case CLWH_PROBE_ENV_APPROX:
      o[0] = __float_as_uint(atan2_approx(__uint_as_float(r[0]), __uint_as_float(r[1])));
      o[1] = __float_as_uint(asin_approx(__uint_as_float(r[2])));
      break;
    case CLWH_PROBE_TONE: o[0] = tone_map_rgba8(r[0], r[1], r[2], r[3]); break;
    case CLWH_PROBE_TAPS: {
      const f3 p = f3_at(r);
      const int64_t e = cache_entry_of(params.v[0], params.v[1], p);
      o[0] = taps_are_voxel_neighbours(p) ? 1u : 0u;
      o[1] = (uint32_t)((uint64_t)e & 0xFFFFFFFFu);
      o[2] = (uint32_t)((uint64_t)e >> 32);
      break;
    }
    case CLWH_PROBE_HULL: {
      const f3 n = hull_direction(r[0]);
      const float scale = __uint_as_float(r[1]);
      put_f3(o, n);
      o[3] = hull_cell(f3{n.x * scale, n.y * scale, n.z * scale});
      o[4] = hull_cell(f3_at(r + 2));
      break;
    }
    default: break;
  }
}

ProbeShape probe_shape(int which) { return probe_shape_of(which); }

hipError_t launch_device_probe(int which, const uint32_t *in, uint64_t n, uint32_t *out, const uint32_t *aux, const int32_t params[4], hipStream_t s) {
  ProbeParams p;
  for (int k = 0; k < 4; ++k) p.v[k] = params[k];
  hipLaunchKernelGGL(k_debug_device_probe, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, s, which, in, n, out, aux, p);
  return hipGetLastError();
}

}  // namespace clvr
