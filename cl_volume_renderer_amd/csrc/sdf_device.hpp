// sdf_device.hpp -- what the signed-distance-field builders share on the device: the event test (sdf_layer_kernels.hip,
// sdf_front_kernels.hip, sdf_bits_kernels.hip), the clamped corner neighbourhood, and for the two files of the bit-parallel build
// (sdf_bits_kernels.hip, sdf_bits_layers_kernels.hip) the row / unit mapping, the region constants, the wake stamps and the phase timer.
#pragma once
#include "render_device.hpp"

namespace clvr {

struct VolumeIntLinear {
  const int16_t *__restrict__ vol;
  int X, Y, Z;
  // read_imagei(volume, int4): out of range -> border 0
  __device__ __forceinline__ int at(int x, int y, int z) const {
    if ((unsigned)x >= (unsigned)X || (unsigned)y >= (unsigned)Y || (unsigned)z >= (unsigned)Z) return 0;
    return vol[((size_t)z * (size_t)Y + (size_t)y) * (size_t)X + (size_t)x];
  }
};

template <bool USE_GRAD>
__device__ __forceinline__ bool event_at(const VolumeIntLinear &v, const TfDev &tf, const uint8_t *cls_in, int x, int y, int z) {
  if (cls_in) return cls_in[((size_t)z * (size_t)v.Y + (size_t)y) * (size_t)v.X + (size_t)x] != 0;  // opaque TF (tf_jit.cpp)
  const int value = v.at(x, y, z);
  int gradient = 0;
  if (USE_GRAD) {
    const float dx = (float)(v.at(x + 1, y, z) - v.at(x - 1, y, z));
    const float dy = (float)(v.at(x, y + 1, z) - v.at(x, y - 1, z));
    const float dz = (float)(v.at(x, y, z + 1) - v.at(x, y, z - 1));
    gradient = (int)(short)f2i(sqrtf((dx * dx + dy * dy) + dz * dz));
  }
  uint32_t color = 0u;
  return tf_eval(tf, value, gradient, color);
}

// One coordinate of a corner neighbour: a step up or down, clamped to the volume (signed_distance_field.cl:72).  The eight corner
// neighbours of a voxel are the combinations over x, y, z: corner c steps up along x / y / z where bit 0 / 1 / 2 of c is set.
__device__ __forceinline__ int corner_step(int v, bool up, int n) { return min(max(v + (up ? 1 : -1), 0), n - 1); }
__device__ __forceinline__ int3 corner_neighbour(int c, int x, int y, int z, int X, int Y, int Z) {
  return int3{corner_step(x, c & 1, X), corner_step(y, c & 2, Y), corner_step(z, c & 4, Z)};
}

// bits of a row shifted to x - 1 and x + 1 with the reference's clamp (signed_distance_field.cl:72): the neighbour of
// x = 0 at x - 1 is x = 0 itself, the neighbour of x = X - 1 at x + 1 is itself -- `both` = bits at either neighbour
__device__ __forceinline__ uint32_t sdfbit_x_neighbours(uint32_t prev, uint32_t cur, uint32_t next, uint32_t clampfix) {
  return ((cur << 1) | (prev >> 31)) | ((cur >> 1) | (next << 31)) | (cur & clampfix);
}

// (row, unit) of a thread for kernels that work on `units` items per (y, z) row: blockIdx.x counts groups of rows
// (rows_per_block = 256 / units when a row has fewer than 256 units), blockIdx.y chunks of 256 units within a row
__device__ __forceinline__ bool sdfbit_row_unit(uint32_t units, size_t n_rows, size_t &row, uint32_t &unit) {
  if (units >= 256u) {
    row = blockIdx.x;
    unit = blockIdx.y * 256u + threadIdx.x;
  } else {
    const uint32_t rows_per_block = 256u / units, r = threadIdx.x / units;
    row = (size_t)blockIdx.x * rows_per_block + r;
    unit = threadIdx.x - r * units;
    if (r >= rows_per_block) return false;
  }
  return row < n_rows && unit < units;
}
inline dim3 sdfbit_row_grid(uint32_t units, size_t n_rows) {
  if (units >= 256u) return dim3((unsigned)n_rows, (units + 255u) / 256u);
  const uint32_t rows_per_block = 256u / units;
  return dim3((unsigned)((n_rows + rows_per_block - 1u) / rows_per_block), 1u);
}

constexpr int kBitCoreY = 48, kBitHalo = 8, kBitRows = 4;  // a wave = 64 rows along y (48 core + 2 x 8 halo) x 4 rows along z
// a block = NW waves (8 or 16) = NW strips of 4 z-rows: region z = 4 NW, core z = 4 NW - 16 (SdfBitArgs::core_z)

// block state: 0 = no reached voxel in the core, 1 = some, 2 = all (just now: the other bit buffer is not complete yet), 3 = all, both buffers.
// A region with reached voxels wakes the EMPTY regions among its 26 neighbours whose core lies within 8 voxels (Chebyshev; a corner move
// changes every coordinate by at most one) of the box around its reached voxels: lane q < 27 stamps neighbour q for the launch `stamp - 1`.
// No loads: the list kernel then needs one byte per region instead of up to 27 dependent state / box reads.
__device__ __forceinline__ void sdfbit_wake_neighbours(const SdfBitArgs &a, int bx, int by, int bz, int x0, int x1, int y0, int y1, int z0, int z1,
                                                       unsigned q, uint8_t stamp) {
  if (q >= 27u) return;
  const int nx = bx + (int)(q % 3u) - 1, ny = by + (int)((q / 3u) % 3u) - 1, nz = bz + (int)(q / 9u) - 1;
  if (nx < 0 || ny < 0 || nz < 0 || nx >= a.BX || ny >= a.BY || nz >= a.BZ) return;
  const int cx0 = nx * 64, cx1 = min(cx0 + 63, a.X - 1), cy0 = ny * kBitCoreY, cy1 = min(cy0 + kBitCoreY - 1, a.Y - 1), cz0 = nz * a.core_z,
            cz1 = min(cz0 + a.core_z - 1, a.Z - 1);
  const int rx0 = bx * 64 + x0, rx1 = bx * 64 + x1, ry0 = by * kBitCoreY + y0, ry1 = by * kBitCoreY + y1, rz0 = bz * a.core_z + z0, rz1 = bz * a.core_z + z1;
  const int gx = max(max(rx0 - cx1, cx0 - rx1), 0), gy = max(max(ry0 - cy1, cy0 - ry1), 0), gz = max(max(rz0 - cz1, cz0 - rz1), 0);
  if (gx <= kBitHalo && gy <= kBitHalo && gz <= kBitHalo) a.wake[((size_t)nz * a.BY + ny) * a.BX + nx] = stamp;
}

// Per-phase times of a region visit in k_sdfbit_layers (-DCLVR_SDFBIT_TIMING, experiment builds: clwh_sdf.hip prints them).  One lane
// of the block (a core lane of a core strip) stamps wall_clock64 at the phase boundaries and adds the differences to SdfBitArgs::timing:
// [0] visits, [1..5] fetch / load / steps / store+values / tail, [6] interior visits.  In a product build the struct is empty and so is
// every method.  (`Args`: SdfBitArgs has its `timing` member in the experiment build only.)
template <bool ON> struct SdfBitProbeT;
template <> struct SdfBitProbeT<false> {
  __device__ explicit SdfBitProbeT(unsigned) {}
  __device__ void mark(int) {}
  __device__ void mark_after_wait(int) {}
  template <class Args> __device__ void flush(const Args &, bool) {}
};
template <> struct SdfBitProbeT<true> {
  const bool probe;
  unsigned long long t[5];
  __device__ __forceinline__ explicit SdfBitProbeT(unsigned tid) : probe(tid == 64u * 2u + 8u) { t[0] = wall_clock64(); }
  __device__ __forceinline__ void mark(int k) { t[k] = wall_clock64(); }
  // the phase ends when the probe lane's loads, stores and atomics have completed
  __device__ __forceinline__ void mark_after_wait(int k) { if (probe) __builtin_amdgcn_s_waitcnt(0); t[k] = wall_clock64(); }
  template <class Args> __device__ __forceinline__ void flush(const Args &a, bool interior) {
    if (probe) {
      atomicAdd(&a.timing[0], 1ull); atomicAdd(&a.timing[1], t[1] - t[0]); atomicAdd(&a.timing[2], t[2] - t[1]); atomicAdd(&a.timing[3], t[3] - t[2]);
      atomicAdd(&a.timing[4], t[4] - t[3]); atomicAdd(&a.timing[5], wall_clock64() - t[4]); atomicAdd(&a.timing[6], interior ? 1ull : 0ull);
    }
  }
};
#ifdef CLVR_SDFBIT_TIMING
using SdfBitProbe = SdfBitProbeT<true>;
#else
using SdfBitProbe = SdfBitProbeT<false>;
#endif

}  // namespace clvr
