// sdf_layer_kernels.hip -- the reference's two signed-distance-field kernels, gfx950: what clwh_launch.hip dispatches when a caller
// runs the reference's own host loop kernel by kernel.
//
// What is computed follows opencl_kernels/signed_distance_field.cl (:6-54 create_base_image,
// :56-87 neightbour_distance_calc, :89-112 create_signed_distance_field) and the host loop of
// app/signed_distance_field.cpp:7-35.  v0: one thread per voxel on x-fastest rows (coalesced byte
// loads/stores along x), per-wave aggregation of the progress counter (one atomic per wave instead
// of one per voxel), and a device-side early-out chain so the fused build needs no host round trip
// per layer.
#include "sdf_device.hpp"

namespace clvr {

// create_base_image: -1 inside an event region, +1 outside; times max_iterations where the 8 clamped
// CORNER neighbours agree with the centre
template <bool USE_GRAD>
__global__ __launch_bounds__(256) void k_sdf_base(const SdfArgs a) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = blockIdx.y;
  const int z = blockIdx.z;
  if (x >= a.X) return;
  const VolumeIntLinear v{a.volume, a.X, a.Y, a.Z};
  const bool e = event_at<USE_GRAD>(v, a.tf, a.cls_in, x, y, z);
  bool homogenous = true;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int3 n = corner_neighbour(c, x, y, z, a.X, a.Y, a.Z);
    homogenous &= (event_at<USE_GRAD>(v, a.tf, a.cls_in, n.x, n.y, n.z) == e);
  }
  int r = e ? -1 : 1;
  if (homogenous) r *= a.max_iterations;
  const size_t i = ((size_t)z * (size_t)a.Y + (size_t)y) * (size_t)a.X + (size_t)x;
  a.ping[i] = (int8_t)r;
  a.pong[i] = (int8_t)r;
}

// one propagation layer
__global__ __launch_bounds__(256) void k_sdf_layer(const SdfArgs a) {
  const int it = a.iteration;
  if (a.done) {
    // fused build: layer `it` runs only while the reference's host loop would still be running:
    // it stops after the first ODD layer whose counter stayed 0 (signed_distance_field.cpp:29-31)
    const bool stop = it > 1 && (a.done[it - 1] != 0 || (((it - 1) & 1) && a.counters[it - 1] == 0));
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) a.done[it] = stop ? 1 : 0;
    if (stop) return;
  }
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = blockIdx.y;
  const int z = blockIdx.z;
  bool wrote = false;
  if (x < a.X) {
    const int8_t *__restrict__ in = a.ping;
    const size_t row = ((size_t)z * (size_t)a.Y + (size_t)y) * (size_t)a.X;
    int local_value = in[row + x];
    int abs_value = abs(local_value);
    if (abs_value >= it) {
      if (abs_value > it) {
        int neighbour_distance = 127, abs_added = 0, added = 0;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const int3 n = corner_neighbour(c, x, y, z, a.X, a.Y, a.Z);
          const int nv = in[((size_t)n.z * (size_t)a.Y + (size_t)n.y) * (size_t)a.X + (size_t)n.x];
          const int t = (int)(int8_t)abs(nv);
          abs_added += t;
          added += nv;
          neighbour_distance = min(neighbour_distance, t);
        }
        if (abs(added) != abs_added) neighbour_distance = 0;
        if (neighbour_distance != 0 && neighbour_distance == it) {
          abs_value = it + 1;
          local_value = local_value < 0 ? -abs_value : abs_value;
        }
      }
      if (abs_value < a.max_iterations) {
        a.pong[row + x] = (int8_t)local_value;
        wrote = true;
      }
    }
  }
  // atomic_inc(add_buffer) per written voxel -> one add per wave
  const unsigned long long m = __ballot(wrote);
  if (m != 0ull && (threadIdx.x & 63u) == (unsigned)__ffsll((long long)m) - 1u) {
    const int n = __popcll(m);
    if (a.counter_out) atomicAdd(a.counter_out, n);
    if (a.counters) atomicAdd(a.counters + it, n);
  }
}

hipError_t launch_sdf_base(const SdfArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(a.tf.uses_gradient ? k_sdf_base<true> : k_sdf_base<false>, row_grid(a.X, a.Y, a.Z), dim3(row_block(a.X)), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_sdf_layer(const SdfArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_sdf_layer, row_grid(a.X, a.Y, a.Z), dim3(row_block(a.X)), 0, s, a);
  return hipGetLastError();
}

}  // namespace clvr
