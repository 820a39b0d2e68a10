// trilinear_device.hpp -- the fixed-point TRILINEAR field of the bricked int16 copy of the volume, shared by the kernels that
// interpolate it: k_isosurface (isosurface_kernels.hip) and k_slice (slice_kernels.hip).  The field is the contract's (include/clwh.h,
// clwh_render_isosurface): per axis an 8-bit weight, the 8 corners combined in integers, S = value * 2^24 exactly -- so a comparison
// of two S holds whatever the order of evaluation, and the result can be tested bit for bit.
//
// The sampler (iso_field) is the hot path: 8 two-byte gathers per sample.  A sample's 2x2x2 cell lies inside one 4^3 sub-brick -- one
// 128-byte line -- unless an axis sits at offset 3 of its sub-brick (58 % of the cells do); the eight indices are formed from per-axis
// terms without a branch (iso_corners).  The x and y stages of the blend fit int32 (|.| <= 2^31 is reached only by -32768 everywhere);
// the z stage is one 64-bit multiply-add.
#pragma once

#include "view_device.hpp"

namespace clvr {

// ------------------------------------------------------------------------------------------------
// the field
struct IsoCell {
  int ix, iy, iz;  // i0 per axis (-1 .. dim - 1), before clamping
  int wx, wy, wz;  // weights of the upper corners, 0 .. 255
};
__device__ __forceinline__ void iso_axis(float p, int &i0, int &w) {
  const float q = p - 0.5f, f = floorf(q);
  i0 = (int)f;
  w = min((int)((q - f) * 256.0f), 255);
}
__device__ __forceinline__ IsoCell iso_cell(const f3 p) {
  IsoCell c;
  iso_axis(p.x, c.ix, c.wx);
  iso_axis(p.y, c.iy, c.wy);
  iso_axis(p.z, c.iz, c.wz);
  return c;
}
struct IsoCorners {
  int v000, v100, v010, v110, v001, v101, v011, v111;
};
// the 8 corner values of a cell
__device__ __forceinline__ IsoCorners iso_corners(const ViewVolume &a, const IsoCell &c) {
  const int16_t *__restrict__ vb = a.bricks;
  IsoCorners v;
  // The brick index is separable (packed_volume.hpp): brick number = bx + by + bz, in-brick offset = ix | iy | iz, with per-axis terms.
  // Six terms per axis pair and one add + one or per corner serve every cell alike -- clamped, straddling or inside one sub-brick --
  // so the wave never diverges here (measured against a lean path for cells inside one 4^3 sub-brick plus eight record_index calls
  // for the rest: the wave nearly always held lanes of both kinds and paid for both).
  const unsigned x0 = (unsigned)max(c.ix, 0), x1 = (unsigned)min(c.ix + 1, a.X - 1), y0 = (unsigned)max(c.iy, 0), y1 = (unsigned)min(c.iy + 1, a.Y - 1);
  const unsigned z0 = (unsigned)max(c.iz, 0), z1 = (unsigned)min(c.iz + 1, a.Z - 1);
  const unsigned nbx = (unsigned)a.NBX, nbxy = (unsigned)a.NBX * (unsigned)a.NBY;
  const unsigned bx0 = x0 >> 3, bx1 = x1 >> 3, by0 = (y0 >> 3) * nbx, by1 = (y1 >> 3) * nbx, bz0 = (z0 >> 3) * nbxy, bz1 = (z1 >> 3) * nbxy;
  const unsigned ix0 = VolumePacked::inner_index(x0, 0u, 0u), ix1 = VolumePacked::inner_index(x1, 0u, 0u);
  const unsigned iy0 = VolumePacked::inner_index(0u, y0, 0u), iy1 = VolumePacked::inner_index(0u, y1, 0u);
  const unsigned iz0 = VolumePacked::inner_index(0u, 0u, z0), iz1 = VolumePacked::inner_index(0u, 0u, z1);
  const unsigned b00 = by0 + bz0, b10 = by1 + bz0, b01 = by0 + bz1, b11 = by1 + bz1;
  const unsigned i00 = iy0 | iz0, i10 = iy1 | iz0, i01 = iy0 | iz1, i11 = iy1 | iz1;
  v.v000 = vb[((size_t)(bx0 + b00) << 9) + (ix0 | i00)]; v.v100 = vb[((size_t)(bx1 + b00) << 9) + (ix1 | i00)];
  v.v010 = vb[((size_t)(bx0 + b10) << 9) + (ix0 | i10)]; v.v110 = vb[((size_t)(bx1 + b10) << 9) + (ix1 | i10)];
  v.v001 = vb[((size_t)(bx0 + b01) << 9) + (ix0 | i01)]; v.v101 = vb[((size_t)(bx1 + b01) << 9) + (ix1 | i01)];
  v.v011 = vb[((size_t)(bx0 + b11) << 9) + (ix0 | i11)]; v.v111 = vb[((size_t)(bx1 + b11) << 9) + (ix1 | i11)];
  return v;
}
// S from the corners and the weights
__device__ __forceinline__ long long iso_blend(const IsoCorners &v, const IsoCell &c) {
  const int ux = 256 - c.wx, uy = 256 - c.wy;
  const int a00 = v.v000 * ux + v.v100 * c.wx, a10 = v.v010 * ux + v.v110 * c.wx;  // |.| <= 2^23
  const int a01 = v.v001 * ux + v.v101 * c.wx, a11 = v.v011 * ux + v.v111 * c.wx;
  const int b0 = a00 * uy + a10 * c.wy, b1 = a01 * uy + a11 * c.wy;                // |.| <= 2^31, reached only as -2^31
  return (long long)b0 * (long long)(256 - c.wz) + (long long)b1 * (long long)c.wz;
}
// S(p) for a position inside the volume
__device__ __forceinline__ long long iso_field(const ViewVolume &a, const f3 p) {
  const IsoCell c = iso_cell(p);
  return iso_blend(iso_corners(a, c), c);
}

}  // namespace clvr
