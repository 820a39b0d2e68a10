// mask_device.hpp -- what the kernel files of the mask operations share (grow, label, distance, geodesic, region statistics): the launch
// helpers, the load of eight voxels, and the classification of the admissible image A (value window, box, row padding) that grow and
// label both build, each with its own stores.
#pragma once

#include "clwh_internal.hpp"

namespace clvr {

namespace {

inline unsigned blocks_for(size_t threads) { return (unsigned)((threads + 255u) / 256u); }
// rows of a multiple of 8 elements in a 16-byte aligned array: a lane may take 8 voxels (or 4 + 4 labels) with 16-byte loads
inline bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0u; }
inline bool rows_of_8(const void *p, int32_t X) { return (X % 8) == 0 && aligned16(p); }

// the eight voxels of one 16-byte load
__device__ __forceinline__ void load8(const int16_t *p, int (&v)[8]) {
  const uint4 q = *reinterpret_cast<const uint4 *>(p);
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int h = 0; h < 8; ++h) v[h] = (int)(int16_t)(w[h >> 1] >> (16 * (h & 1)));
}

// The two classifiers of A.  Args is GrowArgs or LabelArgs: of it they read the volume pointer, X, Y, W64, the window lo .. hi and the
// box.  `id` is the lane's place in the padded bit image, checked by the caller; x0 (x), y, z are the voxels it stands for.
template <class Args>
__device__ __forceinline__ bool in_window_and_box(const Args &a, int v, int x) {
  return v >= a.lo && v <= a.hi && x >= a.box_lo[0] && x < a.box_hi[0];
}
template <class Args>
__device__ __forceinline__ bool in_box_yz(const Args &a, int y, int z) {
  return y >= a.box_lo[1] && y < a.box_hi[1] && z >= a.box_lo[2] && z < a.box_hi[2];
}
// rows of 8: lane `id` owns byte `id` of A and classifies the 8 voxels of one 16-byte load (k_sdfbit_events8's shape); the bytes at
// x0 >= X are the padding and are zero
template <class Args>
__device__ __forceinline__ uint32_t admissible_byte(const Args &a, size_t id, int &x0, int &y, int &z) {
  const size_t bytes_per_row = (size_t)a.W64 * 8u, row = id / bytes_per_row;
  x0 = (int)(id - row * bytes_per_row) * 8;
  z = (int)(row / (size_t)a.Y);
  y = (int)(row - (size_t)z * (size_t)a.Y);
  uint32_t bits = 0u;
  if (x0 < a.X && in_box_yz(a, y, z)) {  // X is a multiple of 8: all eight exist
    int v[8];
    load8(a.volume + row * (size_t)a.X + (size_t)x0, v);
#pragma unroll
    for (int h = 0; h < 8; ++h) bits |= in_window_and_box(a, v[h], x0 + h) ? (1u << h) : 0u;
  }
  return bits;
}
// any row length or alignment: lane `id` is voxel x of the padded row, a wave a 64-bit word of A (k_sdfbit_events' shape); the
// caller's ballot of the answers is the word
template <class Args>
__device__ __forceinline__ bool admissible_voxel(const Args &a, size_t id, int &x, int &y, int &z) {
  const size_t padded = (size_t)a.W64 * 64u, row = id / padded;
  // (the coordinates in locals, handed out at the end, and the box spelt out: this spelling leaves k_label_admissible's ISA as it
  // was; through the references or through in_box_yz it took two VGPRs or six instructions more)
  const int vx = (int)(id - row * padded);
  const int vz = (int)(row / (size_t)a.Y), vy = (int)(row - (size_t)vz * (size_t)a.Y);
  bool in = false;
  if (vx < a.X && vy >= a.box_lo[1] && vy < a.box_hi[1] && vz >= a.box_lo[2] && vz < a.box_hi[2])
    in = in_window_and_box(a, (int)a.volume[row * (size_t)a.X + (size_t)vx], vx);
  x = vx;
  y = vy;
  z = vz;
  return in;
}

}  // namespace

}  // namespace clvr
