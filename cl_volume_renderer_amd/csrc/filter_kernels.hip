// filter_kernels.hip -- the volume filters of clwh_volume_filter (median, grey min / max, exact integer smoothing), gfx950.  The
// definition is in include/clwh.h: a box of offsets |dx| <= rx, |dy| <= ry, |dz| <= rz, every tap read at the coordinate clamped to the
// volume, integers only.
//   k_filter_median<RX, RY, RZ> (radii 0 or 1): a block owns a tile of 64 x 8 x 8 voxels, loads it with a one-voxel halo into LDS
//   (clamped coordinates; 16-byte loads where the volume's rows allow) and a lane selects the medians of two x-neighbouring voxels at
//   once, the taps packed as short2 (.x: the even voxel's, .y: its right neighbour's): forgetful selection over packed min / max, all
//   indices known at compile time.  n = 27, 9 or 3 taps: start with n / 2 + 2 of them, drop the smallest and the largest, take the
//   next tap in; with three left the middle one is the median.
//   k_filter_line_x<KIND> and k_filter_line_yz<KIND> (KIND: min, max, smooth; radius 1 .. 16 at run time): one pass along one axis.
//   Both give a lane eight consecutive outputs of its line and slide the eight-value window over the 2r + 1 offsets: per offset one
//   new value from LDS, eight min / max / multiply-adds, the weight a broadcast LDS read.  The x pass keeps a row segment of 512
//   voxels and 16 on either side in LDS per wave; in the y and z passes a lane owns an x column (a wave's loads and stores are 64
//   consecutive voxels), walks a segment of its line eight steps at a time and keeps the last 16, 32 or 64 values it loaded (by the
//   radius) in LDS slots of its own.
// What has to hold, and why.
//   Bounds.  Every global read is at clamp(coordinate, 0, dim - 1) per axis, or a 16-byte load of a chunk that is tested to lie inside
//   its row; every store is tested against X and against the end of the line's segment.  LDS indices: the median's tile is
//   kMedTileZ + 2 by kMedTileY + 2 rows of kMedPitch shorts and a lane reads shorts 6 + 2 lx .. 11 + 2 lx, lx < 32, of rows
//   0 .. tile + 1; the x pass reads shorts 16 + 8 lane - r .. 16 + 8 lane + r + 8 < kLineXPitch; the yz ring is indexed & (RING - 1).
//   Source and destination.  No launch reads what it writes, except its lane's own voxel (the mask select reads V(p) and writes
//   out(p), in that order, in the lane that owns p): the host routes in-place calls through scratch (clwh_filter.hip).
//   The sums.  |sum| <= 4096 * 32768 = 2^27 and the rounding adds 2048: int32.  The shift is arithmetic.
//   Wave-private LDS.  The x pass' row segment belongs to one wave and the yz ring's slots to one lane; the block's barriers order
//   the x pass' writes before its reads, the ring needs none.
#include "mask_device.hpp"

namespace clvr {

namespace {

typedef short flt_short2 __attribute__((ext_vector_type(2)));

constexpr int kMedTileX = 64, kMedTileY = 8, kMedTileZ = 8;
constexpr int kMedPitch = 80;  // shorts per LDS row: 7 unused, x0 - 1 at 7, the tile's 64 voxels from 8 (16-byte aligned), x0 + 64 at 72, 7 unused
constexpr int kMedRows = (kMedTileY + 2) * (kMedTileZ + 2);

constexpr int kLineXSeg = 512;                  // voxels of a row a wave takes: eight per lane
constexpr int kLineXPitch = kLineXSeg + 2 * 16 + 8;  // 16 before, 16 after, and 8 the last window slides into and never uses

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// eight voxels from x .. x + 7 of a row: one 16-byte load where the row allows and the chunk lies inside, else clamped single loads
__device__ __forceinline__ uint4 load_chunk(const int16_t *row, int x, int X, bool wide) {
  if (wide && x >= 0 && x + 8 <= X) return *reinterpret_cast<const uint4 *>(row + x);
  uint32_t w[4];
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    const uint32_t lo = (uint16_t)row[clampi(x + 2 * h, X - 1)], hi = (uint16_t)row[clampi(x + 2 * h + 1, X - 1)];
    w[h] = lo | (hi << 16);
  }
  return uint4{w[0], w[1], w[2], w[3]};
}

// ---- median

__device__ __forceinline__ void cex(flt_short2 &a, flt_short2 &b) {  // a = min, b = max; packed 16-bit, no saturation
  const flt_short2 lo = __builtin_elementwise_min(a, b), hi = __builtin_elementwise_max(a, b);
  a = lo;
  b = hi;
}
// the smallest of a[LO .. HI - 1] to a[LO] and the largest to a[HI - 1]; the rest stay a multiset
template <int LO, int HI, int N>
__device__ __forceinline__ void min_max_to_ends(flt_short2 (&a)[N]) {
  constexpr int M = HI - LO, H = M / 2;
#pragma unroll
  for (int i = 0; i < H; ++i) cex(a[LO + i], a[HI - 1 - i]);  // the low half holds the minimum, the high half the maximum
#pragma unroll
  for (int i = 1; i < H; ++i) cex(a[LO], a[LO + i]);
#pragma unroll
  for (int i = 1; i < H; ++i) cex(a[HI - 1 - i], a[HI - 1]);
  if constexpr ((M & 1) != 0) {  // the middle element was in neither half
    cex(a[LO], a[LO + H]);
    cex(a[LO + H], a[HI - 1]);
  }
}
// forgetful selection: a[0 .. S - 1] hold the first S = n / 2 + 2 taps, tap[S ..] come in one by one in place of the minimum
template <int M, int NEXT, int NTAPS, int S>
__device__ __forceinline__ flt_short2 forget(flt_short2 (&a)[S], const flt_short2 (&tap)[NTAPS]) {
  min_max_to_ends<0, M, S>(a);
  if constexpr (M == 3) {
    return a[1];
  } else {
    a[0] = tap[NEXT];  // the minimum goes, the maximum is left behind at a[M - 1]
    return forget<M - 1, NEXT + 1, NTAPS, S>(a, tap);
  }
}
template <int NTAPS>
__device__ __forceinline__ flt_short2 median_of(const flt_short2 (&tap)[NTAPS]) {
  if constexpr (NTAPS == 1) {
    return tap[0];
  } else {
    constexpr int S = NTAPS / 2 + 2;
    flt_short2 a[S];
#pragma unroll
    for (int i = 0; i < S; ++i) a[i] = tap[i];
    return forget<S, S, NTAPS, S>(a, tap);
  }
}

}  // namespace

template <int RX, int RY, int RZ>
__global__ __launch_bounds__(256) void k_filter_median(const FilterArgs a) {
  __shared__ __attribute__((aligned(16))) int16_t tile[kMedRows * kMedPitch];
  const int tid = (int)threadIdx.x;
  const size_t TX = (size_t)((a.X + kMedTileX - 1) / kMedTileX), TY = (size_t)((a.Y + kMedTileY - 1) / kMedTileY),
               TZ = (size_t)((a.Z + kMedTileZ - 1) / kMedTileZ), tiles = TX * TY * TZ;
  for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int x0 = (int)(t % TX) * kMedTileX, y0 = (int)((t / TX) % TY) * kMedTileY, z0 = (int)(t / (TX * TY)) * kMedTileZ;
    // the tile's rows in chunks of eight voxels, then the two halo voxels of every row
    for (int i = tid; i < kMedRows * (kMedTileX / 8); i += 256) {
      const int row = i / (kMedTileX / 8), c = i - row * (kMedTileX / 8);
      const int gy = clampi(y0 + row % (kMedTileY + 2) - 1, a.Y - 1), gz = clampi(z0 + row / (kMedTileY + 2) - 1, a.Z - 1);
      const int16_t *src_row = a.src + ((size_t)gz * (size_t)a.Y + (size_t)gy) * (size_t)a.X;
      *reinterpret_cast<uint4 *>(&tile[row * kMedPitch + 8 + 8 * c]) = load_chunk(src_row, x0 + 8 * c, a.X, a.wide_src != 0);
    }
    for (int i = tid; i < kMedRows * 2; i += 256) {
      const int row = i >> 1, right = i & 1;
      const int gy = clampi(y0 + row % (kMedTileY + 2) - 1, a.Y - 1), gz = clampi(z0 + row / (kMedTileY + 2) - 1, a.Z - 1);
      const int gx = clampi(right ? x0 + kMedTileX : x0 - 1, a.X - 1);
      tile[row * kMedPitch + (right ? 8 + kMedTileX : 7)] = a.src[((size_t)gz * (size_t)a.Y + (size_t)gy) * (size_t)a.X + (size_t)gx];
    }
    __syncthreads();
    const int lx = tid & 31, ly = tid >> 5;
    const int px = x0 + 2 * lx, py = y0 + ly;
    if (px < a.X && py < a.Y) {
#pragma unroll 1
      for (int lz = 0; lz < kMedTileZ; ++lz) {
        const int pz = z0 + lz;
        if (pz >= a.Z) break;
        constexpr int NT = (2 * RX + 1) * (2 * RY + 1) * (2 * RZ + 1);
        flt_short2 tap[NT];
        int n = 0;
#pragma unroll
        for (int dz = -RZ; dz <= RZ; ++dz)
#pragma unroll
          for (int dy = -RY; dy <= RY; ++dy) {
            // shorts 6 + 2 lx .. 11 + 2 lx of the row: voxels px - 2 .. px + 3 as three aligned dwords
            const flt_short2 *q = reinterpret_cast<const flt_short2 *>(&tile[((lz + 1 + dz) * (kMedTileY + 2) + ly + 1 + dy) * kMedPitch + 6 + 2 * lx]);
            const flt_short2 q1 = q[1];
            if constexpr (RX != 0) {
              const flt_short2 q0 = q[0], q2 = q[2];
              tap[n++] = flt_short2{q0.y, q1.x};  // x - 1 of either voxel
              tap[n++] = q1;
              tap[n++] = flt_short2{q1.y, q2.x};  // x + 1 of either voxel
            } else {
              tap[n++] = q1;
            }
          }
        const flt_short2 m = median_of<NT>(tap);
        const size_t idx = ((size_t)pz * (size_t)a.Y + (size_t)py) * (size_t)a.X + (size_t)px;
        short o0 = m.x, o1 = m.y;
        if (a.mask) {
          const size_t mrow = ((size_t)pz * (size_t)a.Y + (size_t)py) * (size_t)a.W64 * 8u;
          if (((a.mask[mrow + (size_t)(px >> 3)] >> (px & 7)) & 1u) == 0u) o0 = a.orig[idx];
          if (px + 1 < a.X && ((a.mask[mrow + (size_t)((px + 1) >> 3)] >> ((px + 1) & 7)) & 1u) == 0u) o1 = a.orig[idx + 1u];
        }
        a.dst[idx] = o0;
        if (px + 1 < a.X) a.dst[idx + 1u] = o1;
      }
    }
    __syncthreads();  // the next tile overwrites the LDS
  }
}

namespace {

// ---- line passes

template <int KIND>
__device__ __forceinline__ int line_start() {
  return KIND == CLWH_FILTER_MIN ? 32767 : KIND == CLWH_FILTER_MAX ? -32768 : 2048;
}
template <int KIND>
__device__ __forceinline__ int line_step(int acc, int w, int v) {
  if constexpr (KIND == CLWH_FILTER_MIN) return min(acc, v);
  else if constexpr (KIND == CLWH_FILTER_MAX) return max(acc, v);
  else return acc + w * v;
}
template <int KIND>
__device__ __forceinline__ int line_end(int acc) {
  return KIND == CLWH_FILTER_SMOOTH ? (acc >> 12) : acc;
}
// the weights by |offset|, as ints in LDS (a broadcast read per offset)
__device__ __forceinline__ void stage_weights(const FilterArgs &a, int *wl) {
  if (threadIdx.x <= (unsigned)a.r) wl[threadIdx.x] = (int)a.w[threadIdx.x];
}

}  // namespace

// One pass along x.  A wave takes a segment of kLineXSeg voxels of one row (wave w of the block: row 4 * group + w).
template <int KIND>
__global__ __launch_bounds__(256) void k_filter_line_x(const FilterArgs a) {
  __shared__ __attribute__((aligned(16))) int16_t seg[4][kLineXPitch];
  __shared__ int wl[CLWH_FILTER_MAX_RADIUS + 1];
  stage_weights(a, wl);
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, r = a.r;
  const size_t rows = (size_t)a.Y * (size_t)a.Z, groups = (rows + 3u) / 4u, segs = (size_t)((a.X + kLineXSeg - 1) / kLineXSeg);
  for (size_t u = blockIdx.x; u < groups * segs; u += gridDim.x) {
    const size_t row = (u / segs) * 4u + (size_t)wave;
    const int x0 = (int)(u % segs) * kLineXSeg;
    const bool live = row < rows;
    if (live) {
      const int16_t *src_row = a.src + row * (size_t)a.X;
      // chunk c holds voxels x0 - 16 + 8 c ..: the lane's own (c = lane + 2) and, in lanes 0 .. 3, the two on either side
      *reinterpret_cast<uint4 *>(&seg[wave][8 * (lane + 2)]) = load_chunk(src_row, x0 + 8 * lane, a.X, a.wide_src != 0);
      if (lane < 4) {
        const int c = lane < 2 ? lane : 64 + lane;
        *reinterpret_cast<uint4 *>(&seg[wave][8 * c]) = load_chunk(src_row, x0 - 16 + 8 * c, a.X, a.wide_src != 0);
      }
    }
    __syncthreads();
    const int px = x0 + 8 * lane;
    if (live && px < a.X) {
      const int16_t *win = &seg[wave][16 + 8 * lane - r];
      int v[8], acc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        v[j] = win[j];
        acc[j] = line_start<KIND>();
      }
      for (int k = 0; k <= 2 * r; ++k) {
        const int w = wl[k < r ? r - k : k - r];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = line_step<KIND>(acc[j], w, v[j]);
#pragma unroll
        for (int j = 0; j < 7; ++j) v[j] = v[j + 1];
        v[7] = win[k + 8];
      }
      uint32_t keep = 0xFFu;  // the voxels that take the filtered value
      const size_t idx = row * (size_t)a.X + (size_t)px;
      if (a.mask) keep = a.mask[row * (size_t)a.W64 * 8u + (size_t)(px >> 3)];
      if (px + 8 <= a.X && a.wide_dst && (!a.mask || a.wide_orig)) {
        uint32_t o[4];
        if (a.mask) {
          const uint4 q = *reinterpret_cast<const uint4 *>(a.orig + idx);
          o[0] = q.x, o[1] = q.y, o[2] = q.z, o[3] = q.w;
        }
#pragma unroll
        for (int h = 0; h < 4; ++h) {
          const uint32_t f = ((uint32_t)line_end<KIND>(acc[2 * h]) & 0xFFFFu) | ((uint32_t)line_end<KIND>(acc[2 * h + 1]) << 16);
          const uint32_t sel = (((keep >> (2 * h)) & 1u) ? 0x0000FFFFu : 0u) | (((keep >> (2 * h + 1)) & 1u) ? 0xFFFF0000u : 0u);
          o[h] = a.mask ? ((f & sel) | (o[h] & ~sel)) : f;
        }
        *reinterpret_cast<uint4 *>(a.dst + idx) = uint4{o[0], o[1], o[2], o[3]};
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (px + j < a.X) a.dst[idx + (size_t)j] = ((keep >> j) & 1u) ? (int16_t)line_end<KIND>(acc[j]) : a.orig[idx + (size_t)j];
      }
    }
    __syncthreads();  // the next unit overwrites the segment
  }
}

// One pass along y (axis 1) or z (axis 2).  A lane owns column `col` of a plane: the line's elements are `cols` voxels apart.
//   y: planes = Z, cols = X, n = Y;  z: planes = 1, cols = X * Y, n = Z.
// A unit is 256 neighbouring columns and a segment of kLineSeg outputs of their lines.  Ring slot i & (RING - 1) holds line element
// s - r + i (clamped), s the segment's first output; outputs 8 c .. 8 c + 7 read i = 8 c .. 8 c + 7 + 2 r.  With pre = 2 r rounded up to
// a multiple of 8, elements 0 .. pre + 7 are in the ring before the first outputs, and chunk c loads elements pre + 8 (c + 1) .. + 7
// into registers BEFORE it computes (the loads fly during the arithmetic; what bounds a pass is bytes in flight) and puts them into
// the ring after: they take the slots of i = 8 c .. 8 c + 7 at the earliest, which chunk c has read by then.  So RING >= pre + 8:
// 16 slots for r <= 4, 32 for r <= 12, 64 above (ring_slots), and the LDS a block holds falls with them.
constexpr int kLineSeg = 128;
constexpr int ring_slots(int r) { return r <= 4 ? 16 : r <= 12 ? 32 : 64; }
template <int KIND, int RING>
__global__ __launch_bounds__(256) void k_filter_line_yz(const FilterArgs a) {
  __shared__ int16_t ring[RING * 256];
  __shared__ int wl[CLWH_FILTER_MAX_RADIUS + 1];
  stage_weights(a, wl);
  __syncthreads();
  const int tid = (int)threadIdx.x, r = a.r;
  const bool along_y = a.axis == 1;
  const size_t planes = along_y ? (size_t)a.Z : 1u, cols = along_y ? (size_t)a.X : (size_t)a.X * (size_t)a.Y;
  const int n = along_y ? a.Y : a.Z;
  const size_t col_blocks = (cols + 255u) / 256u, segs = (size_t)((n + kLineSeg - 1) / kLineSeg);
  const int pre = (2 * r + 7) & ~7;
  for (size_t u = blockIdx.x; u < planes * col_blocks * segs; u += gridDim.x) {
    const size_t plane = u / (col_blocks * segs), rest = u - plane * (col_blocks * segs);
    const size_t col = (rest / segs) * 256u + (size_t)tid;
    const int s = (int)(rest % segs) * kLineSeg, e = min(s + kLineSeg, n);
    if (col >= cols) continue;  // (no barrier below: the ring's slots are the lane's own)
    const int16_t *line = a.src + plane * cols * (size_t)n + col;
    int16_t *slot = &ring[tid];
    for (int i = 0; i < pre + 8; i += 8) {
      int16_t got[8];
#pragma unroll
      for (int h = 0; h < 8; ++h) got[h] = line[(size_t)clampi(s - r + i + h, n - 1) * cols];
#pragma unroll
      for (int h = 0; h < 8; ++h) slot[((i + h) & (RING - 1)) * 256] = got[h];
    }
    // where the lane's outputs are in the mask's rows: x, and the row of line element t is row0 + t * row_step
    const size_t x = along_y ? col : col % (size_t)a.X;
    const size_t row0 = along_y ? plane * (size_t)n : col / (size_t)a.X, row_step = along_y ? 1u : (size_t)a.Y;
    for (int c = 0; s + 8 * c < e; ++c) {
      const int i0 = 8 * c;
      const bool more = s + i0 + 8 < e;  // (the same for every lane of the block)
      int16_t got[8];
      if (more) {
#pragma unroll
        for (int h = 0; h < 8; ++h) got[h] = line[(size_t)clampi(s - r + pre + i0 + 8 + h, n - 1) * cols];
      }
      int v[8], acc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        v[j] = slot[((i0 + j) & (RING - 1)) * 256];
        acc[j] = line_start<KIND>();
      }
      for (int k = 0; k <= 2 * r; ++k) {
        const int w = wl[k < r ? r - k : k - r];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = line_step<KIND>(acc[j], w, v[j]);
#pragma unroll
        for (int j = 0; j < 7; ++j) v[j] = v[j + 1];
        v[7] = slot[((i0 + k + 8) & (RING - 1)) * 256];  // (the last one is not used)
      }
      if (more) {
#pragma unroll
        for (int h = 0; h < 8; ++h) slot[((pre + i0 + 8 + h) & (RING - 1)) * 256] = got[h];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int t = s + i0 + j;
        if (t < e) {
          const size_t idx = plane * cols * (size_t)n + (size_t)t * cols + col;
          int16_t o = (int16_t)line_end<KIND>(acc[j]);
          if (a.mask && ((a.mask[(row0 + (size_t)t * row_step) * (size_t)a.W64 * 8u + (x >> 3)] >> (x & 7u)) & 1u) == 0u) o = a.orig[idx];
          a.dst[idx] = o;
        }
      }
    }
  }
}

namespace {
// every kernel strides over its units: a grid is never larger than 2^31 - 1 blocks
unsigned grid_for(size_t units) { return (unsigned)(units < 0x7FFFFFFFull ? (units ? units : 1u) : 0x7FFFFFFFull); }
}  // namespace

hipError_t launch_filter_median(const FilterArgs &a, int rx, int ry, int rz, hipStream_t s) {
  const size_t tiles = (size_t)((a.X + kMedTileX - 1) / kMedTileX) * (size_t)((a.Y + kMedTileY - 1) / kMedTileY) *
                       (size_t)((a.Z + kMedTileZ - 1) / kMedTileZ);
  void (*k)(const FilterArgs) = nullptr;
  switch (rx | ry << 1 | rz << 2) {
    case 1: k = k_filter_median<1, 0, 0>; break;
    case 2: k = k_filter_median<0, 1, 0>; break;
    case 3: k = k_filter_median<1, 1, 0>; break;
    case 4: k = k_filter_median<0, 0, 1>; break;
    case 5: k = k_filter_median<1, 0, 1>; break;
    case 6: k = k_filter_median<0, 1, 1>; break;
    case 7: k = k_filter_median<1, 1, 1>; break;
    default: return hipErrorInvalidValue;  // all radii 0: the host copies
  }
  hipLaunchKernelGGL(k, dim3(grid_for(tiles)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_filter_line(const FilterArgs &a, int kind, hipStream_t s) {
  void (*k)(const FilterArgs) = nullptr;
  size_t units;
  if (a.axis == 0) {
    k = kind == CLWH_FILTER_MIN ? k_filter_line_x<CLWH_FILTER_MIN> : kind == CLWH_FILTER_MAX ? k_filter_line_x<CLWH_FILTER_MAX> : k_filter_line_x<CLWH_FILTER_SMOOTH>;
    units = (((size_t)a.Y * (size_t)a.Z + 3u) / 4u) * (size_t)((a.X + kLineXSeg - 1) / kLineXSeg);
  } else {
    const int ring = ring_slots(a.r);
    if (kind == CLWH_FILTER_MIN) k = ring == 16 ? k_filter_line_yz<CLWH_FILTER_MIN, 16> : ring == 32 ? k_filter_line_yz<CLWH_FILTER_MIN, 32> : k_filter_line_yz<CLWH_FILTER_MIN, 64>;
    else if (kind == CLWH_FILTER_MAX) k = ring == 16 ? k_filter_line_yz<CLWH_FILTER_MAX, 16> : ring == 32 ? k_filter_line_yz<CLWH_FILTER_MAX, 32> : k_filter_line_yz<CLWH_FILTER_MAX, 64>;
    else k = ring == 16 ? k_filter_line_yz<CLWH_FILTER_SMOOTH, 16> : ring == 32 ? k_filter_line_yz<CLWH_FILTER_SMOOTH, 32> : k_filter_line_yz<CLWH_FILTER_SMOOTH, 64>;
    const size_t cols = a.axis == 1 ? (size_t)a.X : (size_t)a.X * (size_t)a.Y, planes = a.axis == 1 ? (size_t)a.Z : 1u;
    const int n = a.axis == 1 ? a.Y : a.Z;
    units = planes * ((cols + 255u) / 256u) * (size_t)((n + kLineSeg - 1) / kLineSeg);
  }
  hipLaunchKernelGGL(k, dim3(grid_for(units)), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace clvr
