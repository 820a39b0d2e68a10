// projection_device.hpp -- the exact sample set of a camera ray and the brick-by-brick walk over it, shared by the kernels that march
// the bricked int16 copy of the volume: k_projection (projection_kernels.hip) and k_composite (composite_kernels.hip).
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

// The brick walk's exit search: kept sample k lies in brick (bx, by, bz); the first sample of (k, kb] outside that brick, kb + 1 if
// there is none.  Where the ray leaves the brick's box is the guess; the exact per-sample test decides.
__device__ __forceinline__ int proj_brick_exit(const ProjRay &r, int k, int kb, unsigned bx, unsigned by, unsigned bz, int k_cap) {
  float tb = INFINITY;
  if (r.d.x != 0.0f) tb = fminf(tb, ((float)((bx + (r.d.x > 0.0f ? 1u : 0u)) * 8u) - r.o.x) / r.d.x);
  if (r.d.y != 0.0f) tb = fminf(tb, ((float)((by + (r.d.y > 0.0f ? 1u : 0u)) * 8u) - r.o.y) / r.d.y);
  if (r.d.z != 0.0f) tb = fminf(tb, ((float)((bz + (r.d.z > 0.0f ? 1u : 0u)) * 8u) - r.o.z) / r.d.z);
  return first_false(k, kb, index_guess(floorf(tb / r.h) + 1.0f, k_cap), [&](int j) {
    float tj;
    const f3 q = proj_sample(r, j, tj);
    return ((unsigned)(int)q.x >> 3) == bx && ((unsigned)(int)q.y >> 3) == by && ((unsigned)(int)q.z >> 3) == bz;
  });
}

}  // namespace clvr
