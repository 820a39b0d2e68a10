// scene_kernels.hip -- what the `render` pass derives from the scene: step bytes and hit records (k_repack), the exit-certificate table (k_macro_*), the start-certificate table (k_start_*), the hull-certificate table (k_hull_*)
#include "bounce_device.hpp"

namespace clvr {

// volume + SDF + transfer function -> bricked step bytes + hit records (packed_volume.hpp).
// A block turns a 64 x 8 x 8 box of the caller's x-fastest images (eight bricks side by side: whole 128-byte lines of the volume; with
// 32 voxels two blocks -- on two XCDs -- each fetched every line: 1.7 GB read for 0.4 GB of images at 512^3) into brick order: the box
// and its one-voxel halo are read ONCE with coalesced loads (a wave reads 64 consecutive voxels of a row) and staged
// in LDS; the central differences and the class come from there; every wave then writes whole 4x4x4 sub-bricks (512
// contiguous bytes of hit records, 64 of step bytes).  The first version let each wave gather its sub-brick's rows and
// the six taps straight from global memory: 8-byte pieces of 128-byte lines, 2.1 GB fetched for a 0.27 GB volume.
#ifndef CLVR_REPACK_X
#define CLVR_REPACK_X 64
#endif
constexpr int kRepackX = CLVR_REPACK_X;  // voxels per block along x (32 or 64)
constexpr int kRepackPitch = kRepackX + 16;  // LDS row: 7 unused shorts, x0 - 1, the box's voxels from a 16-byte aligned offset, one voxel beyond, padding
constexpr int kRepackX0 = 8;        // index of voxel x0 in a row
__global__ __launch_bounds__(256) void k_repack(const RepackArgs a) {
  __shared__ __attribute__((aligned(16))) int16_t s_val[10][10][kRepackPitch];  // [z][y][kRepackX0 + lx], lx = -1 .. 32: values with halo
  __shared__ __attribute__((aligned(16))) int8_t s_sdf[8][8][kRepackX];
  const int x0 = (int)blockIdx.x * kRepackX, y0 = (int)blockIdx.y * 8, z0 = (int)blockIdx.z * 8;
  const unsigned tid = threadIdx.x;
  if ((a.X & 15) == 0 && x0 + kRepackX <= a.X && ((reinterpret_cast<uintptr_t>(a.volume) | reinterpret_cast<uintptr_t>(a.sdf)) & 15u) == 0u) {
    // rows of a multiple of 16 voxels, box inside the volume along x: a lane moves 16 bytes (the staging loop below spent more
    // instructions on its per-voxel index arithmetic than the classification that follows)
    constexpr unsigned kChunks = kRepackX / 8;  // 16-byte pieces of a row of values
    for (unsigned i = tid; i < 10u * 10u * kChunks; i += 256u) {
      const unsigned row = i / kChunks, c = i % kChunks;
      const int ry = (int)(row % 10u), rz = (int)(row / 10u);
      const int y = y0 - 1 + ry, z = z0 - 1 + rz;
      uint4 v = uint4{0u, 0u, 0u, 0u};  // border texel (utility_filter.cl:2-35 reads with CLK_ADDRESS_CLAMP: 0 outside)
      int16_t left = 0, right = 0;
      if ((unsigned)y < (unsigned)a.Y && (unsigned)z < (unsigned)a.Z) {
        const int16_t *src = a.volume + ((size_t)z * (size_t)a.Y + (size_t)y) * (size_t)a.X + (size_t)x0;
        v = *reinterpret_cast<const uint4 *>(src + 8 * c);
        if (c == 0u && x0 > 0) left = src[-1];
        if (c == kChunks - 1u && x0 + kRepackX < a.X) right = src[kRepackX];
      }
      *reinterpret_cast<uint4 *>(&s_val[rz][ry][kRepackX0 + 8 * (int)c]) = v;
      if (c == 0u) s_val[rz][ry][kRepackX0 - 1] = left;
      if (c == kChunks - 1u) s_val[rz][ry][kRepackX0 + kRepackX] = right;
    }
    constexpr unsigned kSdfChunks = kRepackX / 16;  // 16-byte pieces of a row of SDF bytes
    for (unsigned i = tid; i < 8u * 8u * kSdfChunks; i += 256u) {
      const unsigned row = i / kSdfChunks, c = i % kSdfChunks;
      const int ry = (int)(row & 7u), rz = (int)(row >> 3);
      const int y = y0 + ry, z = z0 + rz;
      uint4 v = uint4{0u, 0u, 0u, 0u};
      if (y < a.Y && z < a.Z) v = *reinterpret_cast<const uint4 *>(a.sdf + ((size_t)z * (size_t)a.Y + (size_t)y) * (size_t)a.X + (size_t)x0 + 16u * c);
      *reinterpret_cast<uint4 *>(&s_sdf[rz][ry][16 * (int)c]) = v;
    }
  } else {
    constexpr unsigned kRX = kRepackX + 2;
    for (unsigned i = tid; i < 10u * 10u * kRX; i += 256u) {
      const int rx = (int)(i % kRX), ry = (int)((i / kRX) % 10u), rz = (int)(i / (10u * kRX));
      const int x = x0 - 1 + rx, y = y0 - 1 + ry, z = z0 - 1 + rz;
      int16_t v = 0;
      if ((unsigned)x < (unsigned)a.X && (unsigned)y < (unsigned)a.Y && (unsigned)z < (unsigned)a.Z)
        v = a.volume[((size_t)z * (size_t)a.Y + (size_t)y) * (size_t)a.X + (size_t)x];
      s_val[rz][ry][kRepackX0 - 1 + rx] = v;
    }
    for (unsigned i = tid; i < 8u * 8u * (unsigned)kRepackX; i += 256u) {
      const int rx = (int)(i % (unsigned)kRepackX), ry = (int)((i / (unsigned)kRepackX) % 8u), rz = (int)(i / (8u * (unsigned)kRepackX));
      const int x = x0 + rx, y = y0 + ry, z = z0 + rz;
      int8_t v = 0;
      if (x < a.X && y < a.Y && z < a.Z) v = a.sdf[((size_t)z * (size_t)a.Y + (size_t)y) * (size_t)a.X + (size_t)x];
      s_sdf[rz][ry][rx] = v;
    }
  }
  __syncthreads();
  const unsigned wave = tid >> 6, lane = tid & 63u;
  const size_t brick_row = ((size_t)blockIdx.z * (size_t)a.NBY + (size_t)blockIdx.y) * (size_t)a.NBX;
  // A wave writes the sub-bricks `wave` and `wave + 4` of the block's bricks: the lane's place inside the sub-brick is worked out twice, not
  // once per brick, and the rule table is walked without a per-lane `break` (a divergent loop exit costs more than the two rules it skips).
  for (unsigned half = 0u; half < 2u; ++half) {
   const unsigned sub = wave + 4u * half;
   unsigned ix, iy, iz;
   VolumePacked::inner_coords(sub * 64u + lane, ix, iy, iz);
   const int ly = (int)iy, lz = (int)iz, y = y0 + ly, z = z0 + lz;
   for (unsigned bq = 0u; bq < (unsigned)(kRepackX / 8); ++bq) {
    const int bx = (int)blockIdx.x * (kRepackX / 8) + (int)bq;
    if (bx >= a.NBX) break;
    const int lx = (int)(bq * 8u + ix);
    const int x = x0 + lx;
    uint2 r = uint2{0u, 0u};
    uint8_t q = 0u;
    bool record_read = false;  // can a march ever read this voxel's hit record?
    uint32_t free_min = 255u;  // for the exit certificates: 0 = this voxel may be an event / has no positive SDF value
    if (x < a.X && y < a.Y && z < a.Z) {
      const int cx = kRepackX0 + lx;
      const int value = s_val[lz + 1][ly + 1][cx];
      const int sd = s_sdf[lz][ly][lx];
      // central differences at the voxel's integer position, border 0 (utility_filter.cl:2-35)
      const int dx = s_val[lz + 1][ly + 1][cx + 1] - s_val[lz + 1][ly + 1][cx - 1];
      const int dy = s_val[lz + 1][ly + 2][cx] - s_val[lz + 1][ly][cx];
      const int dz = s_val[lz + 2][ly + 1][cx] - s_val[lz][ly + 1][cx];
      int gradient = 0;
      if (a.tf.uses_gradient) {
        const float gx = (float)dx, gy = (float)dy, gz = (float)dz;
        gradient = (int)(short)f2i(sqrtf((gx * gx + gy * gy) + gz * gz));  // |gradient| to short, as at the call (utility_ray.cl:134)
      }
      // class = 1 + index of the first matching rule; a terminal rule (`return (cond);`) ends the evaluation
      unsigned cls = a.cls_in ? a.cls_in[((size_t)z * (size_t)a.Y + (size_t)y) * (size_t)a.X + (size_t)x] : 0u;
      // `maybe`: could this voxel be an event for SOME gradient?  (A rule that reads `gradient` is evaluated literally, with
      // other taps, at the rare positions whose +-1 taps are not the voxel's neighbours: its value window alone decides here.)
      bool maybe = cls != 0u, decided = a.cls_in != nullptr;
      for (int k = 0; k < a.tf.n; ++k) {  // (wave-uniform trip count; `decided` lanes only ride along)
        const TfRuleDev &rule = a.tf.rules[k];
        const bool in_window = value >= rule.v_lo && value <= rule.v_hi;
        bool m = in_window;
        if (rule.flags & TF_USE_GRADIENT) m = m && gradient >= rule.g_lo && gradient <= rule.g_hi;
        maybe = maybe || (!decided && in_window);
        if (!decided && m && cls == 0u) cls = (unsigned)k + 1u;
        decided = decided || m || (rule.flags & TF_TERMINAL) != 0;
      }
      r = VolumePacked::pack_hit(dx, dy, dz, cls);
      q = (uint8_t)((cls ? 0x80u : 0u) | (uint32_t)(sd > 0 ? sd : 0));
      free_min = (maybe || sd <= 0) ? 0u : (uint32_t)sd;
      record_read = maybe;  // (cls != 0 implies maybe)
    }
    const size_t out = ((brick_row + (size_t)bx) << 9) + sub * 64u + lane;
    // A hit record is read at Hit positions only -- the rule colour and the normal's gradient of a voxel whose class is not 0
    // (render_device.hpp: hit_color, hit_gradient_and_color, gradient_nn; positions with irregular taps and the border never use it).
    // Sub-bricks without such a voxel -- nine in ten on CT-like data -- keep whatever their 512 bytes held: two thirds of what this
    // kernel wrote (8 of 12 bytes per voxel) was never read.
    if (__ballot(record_read) != 0ull) a.grec[out] = r;
    a.stepb[out] = q;
    free_min = wave_min_u32(free_min);
    if (lane == 0u) atomicMin(&a.brick_min[brick_row + (size_t)bx], free_min);  // eight sub-bricks per brick
   }
  }
}

// Exit-certificate table (certify_exit below).  One entry per macro cell (16^3 voxels up to 512^3, growing with the volume:
// macro_cell_shift in clwh_internal.hpp) and direction octant o
// (o = [d.x < 0] | [d.y < 0] << 1 | [d.z < 0] << 2): a march that starts anywhere in the cell with a direction of that
// octant stays in the box between the cell and the volume corner the octant heads for.  The entry is an upper bound of
// the number of steps such a march takes until it leaves the volume, or 255 if the box is not free.
// Step 1: m = the smallest "free value" over the cell's bricks -- 0 if a voxel there may be an event or has an SDF value below
// kCertMinStep, else the smallest SDF value; all eight octant entries start as m.  (Round 2 also took the bricks AROUND the cell, "because
// the real march is off the ideal line by its roundings".  It is, but the proof never needed the line: a march's coordinates are monotone
// in binary32 as well -- adding a product of the direction's sign never moves a coordinate the other way -- so every position it visits
// lies in the box between its cell and the octant's corner exactly, whatever the roundings.  Without the dilation the instrumented
// oracle saves 6.58 instead of 5.79 step fetches per item, 7.68 with certificates tried from a step length of 8, and still counts zero
// wrong certificates: profiles/r03_exit_certificate_finer_estimate.txt.)
__global__ __launch_bounds__(256) void k_macro_table(const uint32_t *__restrict__ brick_min, int NBX, int NBY, int NBZ,
                                                     uint2 *__restrict__ macro, int MNX, int MNY, int MNZ, int shift) {
  const int c = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (c >= MNX * MNY * MNZ) return;
  const int cx = c % MNX, cy = (c / MNX) % MNY, cz = c / (MNX * MNY);
  uint32_t m = 255u;
  const int bpc = 1 << (shift - 3);  // bricks per cell and axis
  for (int bz = cz * bpc; bz <= min(cz * bpc + bpc - 1, NBZ - 1); ++bz)
    for (int by = cy * bpc; by <= min(cy * bpc + bpc - 1, NBY - 1); ++by)
      for (int bx = cx * bpc; bx <= min(cx * bpc + bpc - 1, NBX - 1); ++bx)
        m = min(m, brick_min[((size_t)bz * (size_t)NBY + (size_t)by) * (size_t)NBX + (size_t)bx]);
  if (m < kCertMinStep) m = 0u;
  m *= 0x01010101u;
  macro[c] = make_uint2(m, m);
}

// per-byte minimum of two packed octant entries
__device__ __forceinline__ uint2 min_bytes(uint2 a, uint2 b) {
  uint2 r;
  r.x = r.y = 0u;
  for (int k = 0; k < 32; k += 8) {
    r.x |= min((a.x >> k) & 0xFFu, (b.x >> k) & 0xFFu) << k;
    r.y |= min((a.y >> k) & 0xFFu, (b.y >> k) & 0xFFu) << k;
  }
  return r;
}
// Step 2, once per axis: octant entry o of a cell becomes the minimum over the cells from here to the end of the line in
// o's direction along this axis -- after the three passes, the minimum over the whole box.  One thread per line.
__global__ __launch_bounds__(64) void k_macro_octants(uint2 *__restrict__ macro, int MNX, int MNY, int MNZ, int axis) {
  const int n[3] = {MNX, MNY, MNZ};
  const int len = n[axis], u_n = n[(axis + 1) % 3], v_n = n[(axis + 2) % 3];
  const int line = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (line >= u_n * v_n) return;
  int c[3];
  c[(axis + 1) % 3] = line % u_n;
  c[(axis + 2) % 3] = line / u_n;
  // bytes of the octants that run towards coordinate 0 on this axis (octant o is byte o of the 8-byte entry)
  const uint2 neg = axis == 0 ? make_uint2(0xFF00FF00u, 0xFF00FF00u) : (axis == 1 ? make_uint2(0xFFFF0000u, 0xFFFF0000u) : make_uint2(0u, 0xFFFFFFFFu));
  auto at = [&](int i) -> uint2 & {
    c[axis] = i;
    return macro[((size_t)c[2] * (size_t)MNY + (size_t)c[1]) * (size_t)MNX + (size_t)c[0]];
  };
  uint2 run = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
  for (int i = len - 1; i >= 0; --i) {  // positive direction: accumulate from the far end backwards
    const uint2 v = at(i);
    run = min_bytes(run, v);
    at(i) = make_uint2((v.x & neg.x) | (run.x & ~neg.x), (v.y & neg.y) | (run.y & ~neg.y));
  }
  run = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
  for (int i = 0; i < len; ++i) {  // negative direction: from coordinate 0 forwards
    const uint2 v = at(i);
    run = min_bytes(run, v);
    at(i) = make_uint2((v.x & ~neg.x) | (run.x & neg.x), (v.y & ~neg.y) | (run.y & neg.y));
  }
}
// Step 3: the table keeps the box MINIMUM per octant (0 = the box is not free: no certificate).  Round 2 turned it into a step count
// right here -- box diagonal / minimum + 5 -- because the diagonal is the longest path inside the box; the ray's own distance to the
// face it leaves through is shorter and costs a dozen instructions in certify_exit: 5.79 instead of 5.16 step fetches saved per item
// on the instrumented oracle (tools/exit_certificate.py --variants --finer, profiles/r03_exit_certificate_finer_estimate.txt).
__global__ __launch_bounds__(256) void k_macro_bounds(uint2 *__restrict__ macro, int MNX, int MNY, int MNZ) {
  const int c = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (c >= MNX * MNY * MNZ) return;
  const uint2 v = macro[c];
  uint2 r = make_uint2(0u, 0u);
  for (int o = 0; o < 8; ++o) {
    uint32_t m = ((o < 4 ? v.x : v.y) >> ((o & 3) * 8)) & 0xFFu;
    if (m == 255u) m = 0u;  // (a box without any brick: never the case for a cell inside the volume)
    if (o < 4) r.x |= m << (o * 8); else r.y |= m << ((o - 4) * 8);
  }
  macro[c] = r;
}
// Step 4: a refusing entry says how long to stay away.  For a cell c whose box towards octant o is not free, g = the number of cells
// one must advance along the octant's diagonal until the box is free or the volume ends.  The box of any cell at Chebyshev offset
// <= m from c in the octant's direction contains the box of c + m diagonal, so no cell with every offset below g has a free box: a
// march refused at c cannot get a certificate before one of its coordinates has advanced g - 1 whole cells (k_bounce stays off the
// table that long).  The entry becomes kCertRefused | min(g, 127); certify_exit reads every such value as "not free", so the hint can
// only change WHEN a look-up is made.  (In place: an entry is free before and after, or refusing before -- 0 -- and after -- bit 7
// set --, so a thread that reads a neighbour's entry sees the same answer either way.)
__global__ __launch_bounds__(256) void k_macro_hints(uint2 *__restrict__ macro, int MNX, int MNY, int MNZ) {
  const int c = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (c >= MNX * MNY * MNZ) return;
  const int cx = c % MNX, cy = (c / MNX) % MNY, cz = c / (MNX * MNY);
  const uint8_t *bytes = reinterpret_cast<const uint8_t *>(macro);
  const uint2 v = macro[c];
  uint2 r = v;
  for (int o = 0; o < 8; ++o) {
    const uint32_t m = ((o < 4 ? v.x : v.y) >> ((o & 3) * 8)) & 0xFFu;
    if (m != 0u && !(m & kCertRefused)) continue;  // free
    const int sx = (o & 1) ? -1 : 1, sy = (o & 2) ? -1 : 1, sz = (o & 4) ? -1 : 1;
    uint32_t g = 1u;
    for (; g < 127u; ++g) {
      const int x = cx + sx * (int)g, y = cy + sy * (int)g, z = cz + sz * (int)g;
      if ((unsigned)x >= (unsigned)MNX || (unsigned)y >= (unsigned)MNY || (unsigned)z >= (unsigned)MNZ) break;
      const uint32_t n = bytes[((((size_t)z * (size_t)MNY + (size_t)y) * (size_t)MNX + (size_t)x) << 3) | (size_t)o];
      if (n != 0u && !(n & kCertRefused)) break;
    }
    const uint32_t e = kCertRefused | g;
    if (o < 4) r.x = (r.x & ~(0xFFu << (o * 8))) | (e << (o * 8)); else r.y = (r.y & ~(0xFFu << ((o - 4) * 8))) | (e << ((o - 4) * 8));
  }
  macro[c] = r;
}

hipError_t launch_repack(const RepackArgs &a, hipStream_t s) {
  const dim3 grid(((unsigned)a.NBX + (unsigned)(kRepackX / 8) - 1u) / (unsigned)(kRepackX / 8), (unsigned)a.NBY, (unsigned)a.NBZ);  // every dimension far below the 2^32 work-item limit
  hipLaunchKernelGGL(k_repack, grid, dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_macro_table(const uint32_t *brick_min, int NBX, int NBY, int NBZ, uint8_t *macro8, int X, int Y, int Z, int shift, hipStream_t s) {
  const int M = 1 << shift;
  const int MNX = (X + M - 1) >> shift, MNY = (Y + M - 1) >> shift, MNZ = (Z + M - 1) >> shift;
  uint2 *macro = reinterpret_cast<uint2 *>(macro8);
  const unsigned n = (unsigned)(MNX * MNY * MNZ);
  hipLaunchKernelGGL(k_macro_table, dim3((n + 255u) / 256u), dim3(256), 0, s, brick_min, NBX, NBY, NBZ, macro, MNX, MNY, MNZ, shift);
  const int lines[3] = {MNY * MNZ, MNZ * MNX, MNX * MNY};
  for (int axis = 0; axis < 3; ++axis)
    hipLaunchKernelGGL(k_macro_octants, dim3(((unsigned)lines[axis] + 63u) / 64u), dim3(64), 0, s, macro, MNX, MNY, MNZ, axis);
  hipLaunchKernelGGL(k_macro_bounds, dim3((n + 255u) / 256u), dim3(256), 0, s, macro, MNX, MNY, MNZ);
  hipLaunchKernelGGL(k_macro_hints, dim3((n + 255u) / 256u), dim3(256), 0, s, macro, MNX, MNY, MNZ);
  return hipGetLastError();
}

// ---- start certificates: a per-voxel, per-octant "free from here" table (k_primary copies a hit's byte into its record, k_bounce ends
// a first leg before its first fetch: render_kernels.hip).  One byte per voxel, x fastest; bit o (certify_exit's octant numbering) is
// set when no voxel of the axis-aligned box from this voxel (inclusive) to the volume corner octant o heads for may be an event (step
// byte bit 7).  Three separable passes extend "an event lies that way" along x, y and z, each in both directions.

// The certificate's step bound (start_cert_dmin, clwh_internal.hpp) needs steps that grow with the distance from the events, which is
// a property of the caller's SDF image, not of the table.  It is checked on the step bytes themselves: a voxel with a step value of 0
// or 1 must be an event or (value 1) touch one (Chebyshev distance 1); a voxel with a larger value s must have s >= min(cap, 1 + the
// smallest value among its eight corner neighbours, clamped to the volume as the SDF build clamps them), cap = start_cert_cap.  By
// induction over m: every voxel m >= 1 away from all voxels that touch an event has a value of at least min(cap, m + 1).  The
// converged SDF of the volume passes; one built with fewer layers, or any other image, clears `regular` and the table stays 0.
__global__ __launch_bounds__(256) void k_start_regular(const uint8_t *__restrict__ stepb, int X, int Y, int Z, int NBX, int NBY, unsigned cap, uint32_t *regular) {
  const unsigned brick = blockIdx.x;
  const int bx = (int)(brick % (unsigned)NBX), by = (int)((brick / (unsigned)NBX) % (unsigned)NBY), bz = (int)(brick / (unsigned)(NBX * NBY));
  auto at = [&](int x, int y, int z) -> unsigned { return stepb[VolumePacked::record_index(x, y, z, NBX, NBY)]; };
  bool ok = true;
  for (unsigned inner = threadIdx.x; inner < 512u; inner += 256u) {
    unsigned ix, iy, iz;
    VolumePacked::inner_coords(inner, ix, iy, iz);
    const int x = bx * 8 + (int)ix, y = by * 8 + (int)iy, z = bz * 8 + (int)iz;
    if (x >= X || y >= Y || z >= Z) continue;
    const unsigned q = stepb[((size_t)brick << 9) + inner], s = q & 0x7Fu;
    if (s >= 2u) {
      unsigned m = 127u;
      for (int c = 0; c < 8; ++c)
        m = min(m, at(min(max(x + ((c & 1) ? 1 : -1), 0), X - 1), min(max(y + ((c & 2) ? 1 : -1), 0), Y - 1), min(max(z + ((c & 4) ? 1 : -1), 0), Z - 1)) & 0x7Fu);
      ok = ok && s >= min(cap, m + 1u);
    } else {
      bool touches = false;
      for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
          for (int dx = -1; dx <= 1; ++dx)
            touches = touches || (at(min(max(x + dx, 0), X - 1), min(max(y + dy, 0), Y - 1), min(max(z + dz, 0), Z - 1)) & 0x80u) != 0u;
      ok = ok && touches && (s == 1u || (q & 0x80u) != 0u);
    }
  }
  if (!ok) *regular = 0u;
}
// x: a wave per row finds the row's first and last event voxel; bits of the octants that head for x = X - 1 (even o) are set behind the
// last one, those of the octants that head for x = 0 before the first.  A block takes the 4 x 4 rows of a row of sub-bricks.
__global__ __launch_bounds__(256) void k_start_rows(const uint8_t *__restrict__ stepb, uint8_t *__restrict__ table, int2 *__restrict__ ends, int X, int Y, int Z, int NBX, int NBY) {
  const int lane = (int)(threadIdx.x & 63u), y = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (y >= Y) return;
  for (int k = 0; k < 4; ++k) {
    const int z = (int)blockIdx.y * 4 + k;
    if (z >= Z) break;
    int first = X, last = -1;
    for (int x0 = 0; x0 < X; x0 += 64) {
      const int x = x0 + lane;
      const unsigned long long ev = __ballot(x < X && (stepb[VolumePacked::record_index(min(x, X - 1), y, z, NBX, NBY)] & 0x80u) != 0u);
      if (ev != 0ull) {
        if (first == X) first = x0 + __ffsll((long long)ev) - 1;
        last = x0 + 63 - __clzll((long long)ev);
      }
    }
    uint8_t *row = table + ((size_t)z * (size_t)Y + (size_t)y) * (size_t)X;
    for (int x = lane; x < X; x += 64) row[x] = (uint8_t)((x > last ? 0x55u : 0u) | (x < first ? 0xAAu : 0u));
    if (ends != nullptr && lane == 0) ends[(size_t)z * (size_t)Y + (size_t)y] = make_int2(first, last);  // for k_hull_support
  }
}
// y (axis 1) and z (axis 2): one thread per line, neighbouring threads neighbouring x.  A bit survives only if it is set in every voxel
// from here to the end of the line in its octant's direction.  The last pass clears everything when the step bytes are not `regular`.
__global__ __launch_bounds__(256) void k_start_scan(uint8_t *__restrict__ table, int X, int Y, int Z, int axis, const uint32_t *regular) {
  const int x = (int)(blockIdx.x * blockDim.x + threadIdx.x), other = (int)blockIdx.y;
  if (x >= X) return;
  const int len = axis == 1 ? Y : Z;
  const size_t stride = axis == 1 ? (size_t)X : (size_t)X * (size_t)Y;
  uint8_t *line = table + (axis == 1 ? (size_t)other * (size_t)Y * (size_t)X : (size_t)other * (size_t)X) + (size_t)x;
  const unsigned up = axis == 1 ? 0x33u : 0x0Fu;  // the octants that head for the line's far end
  const unsigned keep = (regular == nullptr || *regular != 0u) ? 0xFFu : 0u;
  unsigned run = 0xFFu;
  for (int i = len - 1; i >= 0; --i) {
    const unsigned v = line[(size_t)i * stride];
    run &= v;
    line[(size_t)i * stride] = (uint8_t)((v & ~up) | (run & up));
  }
  run = 0xFFu;
  for (int i = 0; i < len; ++i) {
    const unsigned v = line[(size_t)i * stride];
    run &= v;
    line[(size_t)i * stride] = (uint8_t)(((v & up) | (run & ~up)) & keep);
  }
}
hipError_t launch_start_table(const uint8_t *stepb, uint8_t *table, uint32_t *regular, int2 *ends, int X, int Y, int Z, int NBX, int NBY, int NBZ, hipStream_t s) {
  hipError_t e = hipMemsetAsync(regular, 1, sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_start_regular, dim3((unsigned)(NBX * NBY * NBZ)), dim3(256), 0, s, stepb, X, Y, Z, NBX, NBY, (unsigned)start_cert_cap(X, Y, Z), regular);
  hipLaunchKernelGGL(k_start_rows, dim3(((unsigned)Y + 3u) / 4u, ((unsigned)Z + 3u) / 4u), dim3(256), 0, s, stepb, table, ends, X, Y, Z, NBX, NBY);
  hipLaunchKernelGGL(k_start_scan, dim3(((unsigned)X + 255u) / 256u, (unsigned)Z), dim3(256), 0, s, table, X, Y, Z, 1, (const uint32_t *)nullptr);
  hipLaunchKernelGGL(k_start_scan, dim3(((unsigned)X + 255u) / 256u, (unsigned)Y), dim3(256), 0, s, table, X, Y, Z, 2, (const uint32_t *)regular);
  return hipGetLastError();
}

// ---- hull certificates: the support table of the event voxels (k_primary picks a plane per hit, k_bounce ends a first leg that heads
// away from it: render_kernels.hip).  Entry k = {n_k, h_k}: n_k = hull_direction(k), h_k an upper bound of n_k . c over the eight
// corners c of every event voxel (step byte bit 7).  Along a row of voxels n_k . c is largest at the row's first or its last event
// voxel, which k_start_rows has found already: a thread takes one direction over kHullRows rows, an ordered-integer atomic maximum
// joins the row groups, and k_hull_finish adds the corner term and the slack (clwh_internal.hpp).  Step bytes that are not `regular`
// (k_start_regular), or without any event, leave h_k = +inf: no point is in front of such a plane.
constexpr int kHullRows = 512;
__device__ __forceinline__ uint32_t ordered_bits(float v) {
  const uint32_t b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__global__ __launch_bounds__(256) void k_hull_support(const int2 *__restrict__ ends, int Y, int n_rows, uint32_t *__restrict__ best_out) {
  const unsigned k = blockIdx.x * 256u + threadIdx.x;
  const f3 n = hull_direction(k);
  const int r0 = (int)blockIdx.y * kHullRows, r1 = min(r0 + kHullRows, n_rows);
  float best = -INFINITY;
  for (int r = r0; r < r1; ++r) {  // (wave-uniform: the row's ends arrive by scalar loads)
    const int2 e = ends[r];
    if (e.y < 0) continue;
    const float yz = n.y * (float)(r % Y) + n.z * (float)(r / Y);
    best = fmaxf(best, yz + fmaxf(n.x * (float)e.x, n.x * (float)e.y));
  }
  if (best > -INFINITY) atomicMax(&best_out[4u * k + 3u], ordered_bits(best));  // the entry's fourth word
}
__global__ __launch_bounds__(256) void k_hull_finish(const uint32_t *__restrict__ regular, float4 *__restrict__ hull, float *__restrict__ hull_h) {
  const unsigned k = blockIdx.x * 256u + threadIdx.x;
  const f3 n = hull_direction(k);
  const uint32_t o = reinterpret_cast<const uint32_t *>(hull)[4u * k + 3u];  // k_hull_support's maximum, 0: no event voxel
  const uint32_t b = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o;
  float h = INFINITY;
  if (o != 0u && *regular != 0u) h = (__uint_as_float(b) + ((fmaxf(n.x, 0.0f) + fmaxf(n.y, 0.0f)) + fmaxf(n.z, 0.0f))) + kHullSlack;
  hull[k] = make_float4(n.x, n.y, n.z, h);
  hull_h[k] = h;  // the same bits, alone: 16 KB that k_bounce's tilted-plane test reads (render_kernels.hip)
}
hipError_t launch_hull_table(const int2 *ends, const uint32_t *regular, float4 *hull, float *hull_h, int X, int Y, int Z, hipStream_t s) {
  (void)X;
  const hipError_t e = hipMemsetAsync(hull, 0, (size_t)kHullPlanes * sizeof(float4), s);
  if (e != hipSuccess) return e;
  const int n_rows = Y * Z;  // (below 2^31: kHullMaxDim)
  // the running maxima sit in the entries' fourth words (stride 4 words)
  hipLaunchKernelGGL(k_hull_support, dim3((unsigned)kHullPlanes / 256u, ((unsigned)n_rows + (unsigned)kHullRows - 1u) / (unsigned)kHullRows), dim3(256), 0, s, ends, Y, n_rows,
                     reinterpret_cast<uint32_t *>(hull));
  hipLaunchKernelGGL(k_hull_finish, dim3((unsigned)kHullPlanes / 256u), dim3(256), 0, s, regular, hull, hull_h);
  return hipGetLastError();
}

}  // namespace clvr
