// view_device.hpp -- what the kernels that read the bricked int16 copy of the volume share (k_projection, k_composite, k_isosurface,
// k_slice and the mesher): the {min, max} tables' words, a lane's pixel and camera ray, the exact sample set of a ray, the
// brick-by-brick walk over it (walk_bricks), and the stores and shading of the image views.
//
// The contract (include/clwh.h) is exact so that it can be tested bit for bit: sample k of a pixel's ray sits at t_k = (float)k * h,
// p_k = o + d * t_k (per component one multiply, then one add; the library is built without contraction), and is KEPT iff
// t_near <= t_k <= t_far and 0 <= p_k.c < dim_c on all three axes; its value is the voxel at floor(p_k).
//
// Why the kernels may bound loops by boxes: float multiply and add are monotone, so each coordinate of p_k is monotone in k (and t_k
// too).  Every condition of "kept" therefore switches at most once along the ray, and the kept samples of a ray form ONE contiguous
// range of k; so do the kept samples inside any axis-aligned box, such as an 8^3 brick, and once the march has left a brick it never
// comes back to it.  Box intersections in float only give a starting guess for a search; the exact per-sample test decides every
// boundary (first_false below), so the sample set is the dense loop's whatever the guess.
#pragma once

#include "render_device.hpp"

namespace clvr {

// ------------------------------------------------------------------------------------------------
// the exact sample test
struct ProjRay {
  f3 o, d;
  float h, t_near, t_far;
  float dx, dy, dz;  // volume dims
};

__device__ __forceinline__ f3 proj_sample(const ProjRay &r, int k, float &t) {
  t = (float)k * r.h;
  return f3{r.o.x + r.d.x * t, r.o.y + r.d.y * t, r.o.z + r.d.z * t};
}
// "kept" split into the conditions that can only switch from false to true as k grows (rising) and those that can only switch from
// true to false (falling): kept(k) = rising(k) && falling(k), so the kept range is [first rising k, last falling k].  An axis the ray
// does not move along (d.c == +-0, or NaN) keeps p.c == o.c while t is finite: its test is falling (an infinite t makes it NaN).
__device__ __forceinline__ bool axis_rising(float p, float d, float dim) { return d > 0.0f ? p >= 0.0f : (d < 0.0f ? p < dim : true); }
__device__ __forceinline__ bool axis_falling(float p, float d, float dim) {
  return d > 0.0f ? p < dim : (d < 0.0f ? p >= 0.0f : (p >= 0.0f && p < dim));
}
__device__ __forceinline__ bool proj_rising(const ProjRay &r, int k) {
  float t;
  const f3 p = proj_sample(r, k, t);
  return t >= r.t_near && axis_rising(p.x, r.d.x, r.dx) && axis_rising(p.y, r.d.y, r.dy) && axis_rising(p.z, r.d.z, r.dz);
}
__device__ __forceinline__ bool proj_falling(const ProjRay &r, int k) {
  float t;
  const f3 p = proj_sample(r, k, t);
  return t <= r.t_far && axis_falling(p.x, r.d.x, r.dx) && axis_falling(p.y, r.d.y, r.dy) && axis_falling(p.z, r.d.z, r.dz);
}

// The smallest k in (lo, hi] with pred(k) false, given pred(lo) true and pred true-then-false on [lo, hi]; hi + 1 if there is none.
// `guess` (a float estimate of the answer) only decides where the search starts: gallop away from it, then bisect.
template <class Pred>
__device__ __forceinline__ int first_false(int lo, int hi, int guess, Pred pred) {
  int f = hi + 1;  // pred is false at f, or f lies past the range
  const int g = guess <= lo ? lo + 1 : (guess > f ? f : guess);
  if (g < f && pred(g)) {
    lo = g;
    for (int s = 1; lo + s < f; s <<= 1) {
      if (!pred(lo + s)) { f = lo + s; break; }
      lo += s;
    }
  } else {
    f = g;
    for (int s = 1; f - s > lo; s <<= 1) {
      if (pred(f - s)) { lo = f - s; break; }
      f -= s;
    }
  }
  while (f - lo > 1) {
    const int m = lo + ((f - lo) >> 1);
    if (pred(m)) lo = m; else f = m;
  }
  return f;
}

// a float sample index as a search start in [0, cap] (NaN -> 0)
__device__ __forceinline__ int index_guess(float kf, int cap) { return (int)fminf(fmaxf(kf, 0.0f), (float)cap); }

// the ray's kept range [ka, kb]; false if it is empty
__device__ __forceinline__ bool proj_kept_range(const ProjRay &r, int k_cap, int &ka, int &kb) {
  float te = r.t_near, tx = r.t_far;  // slab estimate of the entry and exit
  const float dv[3] = {r.d.x, r.d.y, r.d.z}, ov[3] = {r.o.x, r.o.y, r.o.z}, dim[3] = {r.dx, r.dy, r.dz};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (dv[c] != 0.0f) {
      const float a = (0.0f - ov[c]) / dv[c], b = (dim[c] - ov[c]) / dv[c];
      te = fmaxf(te, fminf(a, b));
      tx = fminf(tx, fmaxf(a, b));
    }
  }
  if (!proj_falling(r, 0)) return false;
  kb = first_false(0, k_cap - 1, index_guess(floorf(tx / r.h) + 1.0f, k_cap), [&](int k) { return proj_falling(r, k); }) - 1;
  ka = proj_rising(r, 0) ? 0 : first_false(0, kb, index_guess(ceilf(te / r.h), k_cap), [&](int k) { return !proj_rising(r, k); });
  return ka <= kb;
}

// ------------------------------------------------------------------------------------------------
// the {min, max} tables (ViewVolume::table, dilated, coarse): one word per brick or cell
__device__ __forceinline__ int table_min(uint32_t mm) { return (int)(int16_t)(mm & 0xFFFFu); }
__device__ __forceinline__ int table_max(uint32_t mm) { return (int)(int16_t)(mm >> 16); }
__device__ __forceinline__ uint32_t pack_min_max(int lo, int hi) { return (uint32_t)(uint16_t)lo | ((uint32_t)(uint16_t)hi << 16); }
template <class I>
__device__ __forceinline__ size_t brick_index(const ViewVolume &v, I bx, I by, I bz) {
  return ((size_t)bz * (size_t)v.NBY + (size_t)by) * (size_t)v.NBX + (size_t)bx;
}
template <class I>
__device__ __forceinline__ size_t cell_index(const ViewVolume &v, I cx, I cy, I cz) {
  return ((size_t)cz * (size_t)v.CNY + (size_t)cy) * (size_t)v.CNX + (size_t)cx;
}

// ------------------------------------------------------------------------------------------------
// the brick walk
// The exit search: kept sample k lies in box (bx, by, bz) of 2^SHIFT voxels per axis (3: a brick, 5: a cell of 4^3 bricks); the first
// sample of (k, kb] outside that box, kb + 1 if there is none.  Where the ray leaves the box is the guess; the exact per-sample test
// decides.
template <int SHIFT>
__device__ __forceinline__ int box_exit(const ProjRay &r, int k, int kb, unsigned bx, unsigned by, unsigned bz, int k_cap) {
  constexpr unsigned kEdge = 1u << SHIFT;
  float tb = INFINITY;
  if (r.d.x != 0.0f) tb = fminf(tb, ((float)((bx + (r.d.x > 0.0f ? 1u : 0u)) * kEdge) - r.o.x) / r.d.x);
  if (r.d.y != 0.0f) tb = fminf(tb, ((float)((by + (r.d.y > 0.0f ? 1u : 0u)) * kEdge) - r.o.y) / r.d.y);
  if (r.d.z != 0.0f) tb = fminf(tb, ((float)((bz + (r.d.z > 0.0f ? 1u : 0u)) * kEdge) - r.o.z) / r.d.z);
  return first_false(k, kb, index_guess(floorf(tb / r.h) + 1.0f, k_cap), [&](int j) {
    float tj;
    const f3 q = proj_sample(r, j, tj);
    return ((unsigned)(int)q.x >> SHIFT) == bx && ((unsigned)(int)q.y >> SHIFT) == by && ((unsigned)(int)q.z >> SHIFT) == bz;
  });
}

// The kept range [k, kb] of a ray (proj_kept_range), one brick per iteration, front to back.  cell_skip(cell) and brick_skip(brick)
// say "step over unread" for the cell of 4^3 bricks and for the brick that hold sample k (indices into ViewVolume::coarse and
// ::table / ::dilated); the cell is asked before the brick's exit search, the brick after it.  visit(brick, k, k_end) runs the
// kernel's loop over the samples [k, k_end) of the brick and returns true to end the ray; the walk returns whether a visit did.
template <class CellSkip, class BrickSkip, class Visit>
__device__ __forceinline__ bool walk_bricks(const ProjRay &r, const ViewVolume &v, int k, int kb, int k_cap, CellSkip cell_skip,
                                            BrickSkip brick_skip, Visit visit) {
  bool ended = false;
  while (k <= kb && !ended) {
    float t;
    const f3 p = proj_sample(r, k, t);  // kept: 0 <= p < dim, so the conversions are floors
    const unsigned bx = (unsigned)(int)p.x >> 3, by = (unsigned)(int)p.y >> 3, bz = (unsigned)(int)p.z >> 3;
    if (cell_skip(cell_index(v, bx >> 2, by >> 2, bz >> 2))) {  // one exit search for up to ~55 voxels of ray
      k = box_exit<5>(r, k, kb, bx >> 2, by >> 2, bz >> 2, k_cap);
      continue;
    }
    const int k_end = box_exit<3>(r, k, kb, bx, by, bz, k_cap);
    const size_t brick = brick_index(v, bx, by, bz);
    if (!brick_skip(brick)) ended = visit(brick, k, k_end);
    k = k_end;
  }
  return ended;
}
// the test of a walk that reads every cell or brick
struct NeverSkip {
  __device__ __forceinline__ bool operator()(size_t) const { return false; }
};

// ------------------------------------------------------------------------------------------------
// a lane's pixel, its camera ray and its outputs
// one wave per 8x8 pixel tile, tiles in XCD-contiguous order (as k_primary, primary_kernels.hip), one lane per pixel
__device__ __forceinline__ void view_pixel(const ViewFrame &f, uint32_t &x, uint32_t &y) {
  const uint32_t slot = xcd_contiguous_slot(blockIdx.x, (uint32_t)f.num_tiles);
  const uint32_t tx = slot % (uint32_t)f.tiles_x, ty = slot / (uint32_t)f.tiles_x;
  const uint32_t lane = threadIdx.x;
  x = tx * 8u + (lane & 7u);
  y = ty * 8u + (lane >> 3);
}
__device__ __forceinline__ ProjRay camera_ray(const ViewCamera &c, const ViewVolume &v, const ViewFrame &f, uint32_t x, uint32_t y) {
  const f3 cam_o = f3{c.cam_pos[0], c.cam_pos[1], c.cam_pos[2]};
  const f3 cam_d = f3{c.cam_dir[0], c.cam_dir[1], c.cam_dir[2]};
  const Ray ray = generate_ray(cam_o, cam_d, (int)x, (int)y, f.frame_w, f.frame_h);
  return ProjRay{ray.origin, ray.direction, c.step, c.t_near, c.t_far, (float)v.X, (float)v.Y, (float)v.Z};
}
// the pixel into the frame; returns its index in the optional outputs, which are row-major over the launched region
__device__ __forceinline__ size_t store_frame(const ViewFrame &f, uint32_t x, uint32_t y, uint32_t px) {
  f.frame[(size_t)y * (size_t)f.frame_w + x] = px;
  return (size_t)y * (size_t)f.launch_w + x;
}
template <class T>
__device__ __forceinline__ void store_optional(T *out, size_t o, const T &value) {
  if (out) out[o] = value;
}

__device__ __forceinline__ uint32_t quantise_unorm8(float x) { return (uint32_t)(int)fminf(fmaxf(x * 255.0f + 0.5f, 0.0f), 255.0f); }
// IEEE 754 leaves a NaN's sign and payload to the implementation; the contract stores every NaN as 0x7FC00000
__device__ __forceinline__ float canonical_nan(float x) { return x == x ? x : __builtin_nanf(""); }
// a value through the grey window; no kept sample (NaN): (0, 0, 0, 0)
__device__ __forceinline__ uint32_t window_grey(float value, float center, float width) {
  uint32_t px = 0u;
  if (value == value) {
    const float u = ((value - center) / width + 0.5f) * 255.0f + 0.5f;
    px = (uint32_t)(int)fminf(fmaxf(u, 0.0f), 255.0f) * 0x010101u | 0xFF000000u;
  }
  return px;
}

// ------------------------------------------------------------------------------------------------
// shading
// the central differences at voxel (x, y, z), each neighbour clamped into the volume
__device__ __forceinline__ void central_difference(const ViewVolume &v, int x, int y, int z, int &gx, int &gy, int &gz) {
  const int16_t *__restrict__ vb = v.bricks;
  const auto at = [&](int i, int j, int k) { return (int)vb[VolumePacked::record_index(i, j, k, v.NBX, v.NBY)]; };
  gx = at(min(x + 1, v.X - 1), y, z) - at(max(x - 1, 0), y, z);
  gy = at(x, min(y + 1, v.Y - 1), z) - at(x, max(y - 1, 0), z);
  gz = at(x, y, min(z + 1, v.Z - 1)) - at(x, y, max(z - 1, 0));
}
__device__ __forceinline__ float length2(float gx, float gy, float gz) { return (gx * gx + gy * gy) + gz * gz; }
// the two-sided headlight factor of a gradient g with |g| = len > 0 seen along d
__device__ __forceinline__ float headlight(float gx, float gy, float gz, float len, const f3 &d, float ambient) {
  const float c = fabsf((gx * d.x + gy * d.y) + gz * d.z) / len;
  return ambient + (1.0f - ambient) * fminf(c, 1.0f);
}

}  // namespace clvr
