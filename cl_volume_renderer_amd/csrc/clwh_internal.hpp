// clwh_internal.hpp -- what the host runtime and the HIP kernels share: argument structs and launcher prototypes.
// Host-only types (contexts, memory objects, owners of device memory) are in clwh_host.hpp.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/clwh.h"

namespace clvr {

// ---- transfer function as a kernel argument (uniform -> SGPRs / scalar cache)
struct TfRuleDev {
  int32_t v_lo, v_hi, g_lo, g_hi;
  uint32_t flags;   // bit0 use_gradient, bit1 writes_color, bit2 terminal
  uint32_t color;   // r | g<<8 | b<<16 | a<<24
};
struct TfDev {
  int32_t n;
  int32_t uses_gradient;
  int32_t literal_gradient_taps;  // 1: always take the reference's 7-fetch step (test knob CLWH_TUNE_LITERAL_GRADIENT)
  int32_t opaque;                 // 1: classes come from a hiprtc-compiled is_event_gen (tf_jit.cpp); rules hold only colours
  int32_t border_class;           // class of the border texel (value 0) for gradient-free rule tables: 1 + index of the first rule that
                                  // contains 0, or 0.  read_imagei returns 0 outside the volume, and a position with a NaN coordinate
                                  // or a coordinate == dimension is not 'exited' (utility_ray.cl:112-117): it classifies as value 0
  TfRuleDev rules[CLWH_TF_MAX_RULES];
};

enum : uint32_t { TF_USE_GRADIENT = 1u, TF_WRITES_COLOR = 2u, TF_TERMINAL = 4u };

// ---- render pass arguments
// One hit record = one 64-byte line: what compute_light needs to start the sample's bounce paths.
struct HitRec {
  float origin[3];     // hit_information.origin (position of the primary Hit event)
  float direction[3];  // hit_information.direction (the camera ray's direction)
  float normal[3];     // -normalize(gradient) at the hit (ray_marching.cl:42)
  uint32_t color;      // transfer-function colour of the hit: r | g<<8 | b<<16 | roughness<<24
  int32_t entry_lo;    // voxel-cache entry (y-major), or -2 when the entry lies outside the cache
  int32_t entry_hi;
  uint32_t xy;         // global pixel: x | y<<16  (feeds the per-pixel RNG, utility_sampling.cl:41)
  uint32_t pslot;      // tile-major pixel slot of this rank (accumulation / scratch index)
  uint32_t start_free; // bits 0-7: the start-certificate byte at the voxel the hit's distribution rays start from (k_primary), else 0
  uint32_t pad;
};
static_assert(sizeof(HitRec) == 64, "HitRec must be one 64-byte line");

enum : uint32_t { PIX_HIT = 0x80000000u };  // pix_slot: PIX_HIT | hit index, else the miss colour (rgb)

// format of the exit-certificate table, shared by its builder (scene_kernels.hip) and its reader (certify_exit, bounce_device.hpp)
constexpr uint32_t kCertMinStep = 2u;     // a box whose smallest SDF value is below this counts as not free
constexpr uint32_t kCertRefused = 0x80u;  // bit 7 of an entry: the box is not free (box minima are SDF values, at most 127)

// slots of RenderArgs::counters (cleared per camera from CTR_HITS on, per launch behind it)
enum : uint32_t {
  CTR_HITS = 0, CTR_FIXUPS = 2,  // primary hits of this camera (k_primary); fix-up records of this launch
  // -DCLVR_BOUNCE_STATS builds: scheduling statistics (BounceStats, bounce_device.hpp), sums over the launch's waves
  CTR_STEP_ITERS = 8, CTR_STEP_LANES, CTR_EVENT_PHASES, CTR_EVENT_LANES, CTR_REFILLS, CTR_REFILL_LANES,
  CTR_EV_KIND,     // four slots: start / exit / hit / none
  CTR_CERT_PHASES = CTR_EV_KIND + 4, CTR_CERT_LANES, CTR_CERT_GRANTED,
  CTR_SWAPS, CTR_STEP_IDLE,  // k_bounce2 only: swap points; k_bounce only: idle lanes, summed over the step iterations
  CTR_START_TRIED, CTR_START_GRANTED, CTR_START_WRONG,  // k_bounce only: start certificates (first legs of long launches); wrong: see BounceStats
  CTR_HULL_TRIED, CTR_HULL_GRANTED, CTR_HULL_BOTH, CTR_HULL_WRONG,  // k_bounce only: hull certificates; both: legs either proof grants
  CTR_STATS_END,
  CTR_QUEUE_STRIDE = 32,  // head of unit queue q: slot CTR_QUEUE_STRIDE * (q + 1), every head on its own 128-byte line
  // k_bounce only, behind the last queue head: tried / granted / wrong of the hull certificates item 13 added, three slots per class --
  // first legs granted after a few literal steps, rebounds granted at once, rebounds granted after a few literal steps
  CTR_HULL_DEFER = CTR_QUEUE_STRIDE * 9, CTR_HULL_DEFER_END = CTR_HULL_DEFER + 9,
  // ... and of the tilted planes item 14 adds, four classes: first legs at once / after a few literal steps, rebounds at once / after a few;
  // then one slot: armed lanes that covered their path too late and went back to marching without a look-up
  CTR_HULL_TILT = CTR_HULL_DEFER_END, CTR_HULL_TILT_END = CTR_HULL_TILT + 13,
};
struct RenderArgs {
  int32_t X, Y, Z;
  const uint2 *grec;       // bricked hit records {gx, gy, gz, class} (packed_volume.hpp)
  const uint8_t *stepb;    // bricked per-step bytes (packed_volume.hpp)
  const int16_t *volume_lin;  // the caller's images (x fastest): literal taps of the rare paths
  const int8_t *sdf_lin;
  // exit certificates (bounce_device.hpp, certify_exit): eight bytes per macro cell of 16^3 voxels; byte o: the smallest SDF value in
  // the box a march from this cell in direction octant o crosses until it leaves the volume (1..127), or, when the box is not free,
  // 0x80 | the number of cells along the octant's diagonal until it is (k_macro_hints)
  const uint8_t *macro;
  int32_t MNX, MNY, MNZ, macro_shift;  // cells per axis, log2 of the cell's edge in voxels
  int32_t cert_min_step;   // a march asks for a certificate once its next step is at least this long; 0 = certificates off
  int32_t cert_min_lanes;  // ... and the wave looks them up once this many lanes wait for one (launch_bounce sets it)
  int32_t cert_hint;       // 1: a refused march stays off the table for the distance the refusing entry names (k_macro_hints)
  // start certificates (k_start_* in scene_kernels.hip): one byte per voxel, x fastest; bit o: no voxel of the box from this voxel to the
  // volume corner of octant o may be an event.  k_primary copies the byte of a hit's start voxel into the hit record; nullptr: not built
  const uint8_t *start_free;
  float start_cert_dmin;   // a first leg is granted its certificate only if min |direction component| is at least this (start_cert_dmin below)
  // hull certificates (k_hull_* in scene_kernels.hip): kHullPlanes entries {n_k, h_k}, every corner of every event voxel has n_k . c <= h_k.
  // k_primary stores per hit (hull_codes, beside the hit records) 1 + the index of a plane the hit's start point lies in front of,
  // 0: none; nullptr: not built
  const float4 *hull;
  uint32_t *hull_codes;
  float hull_delta0;       // a first leg with such a plane is granted if direction . n_k is at least this (hull_cert_delta0 below)
  // ... and (hull_planes, a second word per hit) 1 + the index of the best plane the search found even when the start point lies up to
  // kHullDeferDeficit BEHIND it, with the signed margin in bits 16-23 (k_primary; clwh_debug_hull_planes); nullptr: CLWH_TUNE_HULL_DEFER=0, or no table
  uint32_t *hull_planes;
  float hull_defer_delta0;  // a march that gets in front of such a plane within J steps (kHullDeferSteps; kHullTiltSteps with hull_h) is granted there if direction . n_k is at least this
  // ... and the table's h_k alone (kHullPlanes floats, k_hull_finish): a march that neither rule above grants or arms asks the plane whose
  // normal is the hit's plane normal tilted towards its own direction; nullptr: CLWH_TUNE_HULL_TILT=0, no hull_planes, or no table
  const float *hull_h;
  float hull_tilt_target;   // t: the tilt aims at direction . n' = t = hull_defer_delta0 + kHullTiltMargin
  float hull_tilt_gain;     // t / sqrt(1 - t^2)
  int32_t NBX, NBY;
  const uint32_t *env;     // RGBA8 packed, row-major
  int32_t env_w, env_h;
  uint32_t *cache;         // voxel cache as 2 x u32 per entry
  int64_t cache_entries;   // entries that may be indexed
  uint32_t *frame;         // RGBA8 packed, row-major, frame_w x frame_h
  int32_t frame_w, frame_h;
  int32_t launch_w, launch_h;
  int32_t tiles_x, tiles_y, tiles_per_row;  // 8x8 pixel tiles; tiles_per_row = ceil(tiles_x / world)
  int32_t tile_rank, tile_world;
  float cam_pos[3];
  float cam_dir[3];
  int32_t mode;            // clwh_accum_mode
  float4 *accum;           // tile-major float4 per pixel slot (mode 1)
  unsigned long long *delta;  // mode 1 (and planned voxel-cache launches): this launch's packed sums per hit (see finish_item / k_commit)
  // planned voxel-cache launches (several seeds fused into one launch, clwh_render): the tokens of the launch are dealt out BEFORE it
  // runs -- grants[h] = how many of the launch's seeds hit h may trace (the first grants[h] of them) -- instead of three atomics per
  // sample on a cache entry that all the seeds and pixels of a voxel hammer at the same time; nullptr: the reference's own
  // token-per-sample protocol (utility.cl:20-36)
  const uint32_t *grants;
  uint32_t *pix_slot;      // tile-major, per pixel: PIX_HIT | hit index, or the miss colour
  HitRec *hits;            // compacted primary hits of this camera
  uint32_t *counters;      // the CTR_* slots above
  uint32_t *fixups;        // 128-byte records of samples whose env lookup needs the exact route
  uint32_t fixup_capacity;
  uint32_t *sticky_flags;  // [0] fix-up overflow (outside the per-launch reset range: survives until the host reads it)
  uint32_t n_hits;         // host copy of counters[CTR_HITS], or an upper bound of it when n_hits_on_device
  uint32_t n_hits_estimate;  // the likely count (the count itself once known): picks the scheduling class of the launch
  int32_t n_hits_on_device;  // 1: kernels read the hit count from counters[CTR_HITS] (no host round trip after k_primary)
  int32_t shading;         // clwh_shading
  int64_t *hit_index_out;  // optional, row-major over launch_w x launch_h
  uint32_t *contrib_out;   // optional, row-major uint32[4] (single seed)
  uint32_t num_tile_slots; // tile slots of this rank
  int32_t n_seeds;
  int32_t seeds[CLWH_MAX_SEEDS];
  // scheduling knobs of k_bounce (defaults in clwh_host.hpp, Tuning; CLWH_TUNE_* override for experiments)
  int32_t step_min_lanes;    // keep stepping while at least this many lanes march
  int32_t refill_min_lanes;  // idle lanes fetch new items once this many are idle (64: only an empty wave refills)
  int32_t force_long_launch; // tests: schedule every launch like a long one (thresholds 16 / 16, exit certificates)
  int32_t bounce_rays;       // 2: long launches run k_bounce2, two rays per lane (CLWH_TUNE_BOUNCE_RAYS; the round-3 experiment)
  uint32_t bounce_max_blocks;  // persistent grid size (256-thread blocks)
  int32_t unit_group;          // chunks per queue group (see k_bounce refill)
  int32_t unit_block_log2;     // 2^n consecutive chunks go to the same queue
  int32_t unit_queues;         // number of unit queues (1..8)
  int32_t unit_affinity;       // 0: the wave's XCD picks its home queue (default); 1: wave number; 2: queue 0 (experiments)
  TfDev tf;
  // k_bounce: 1 = a wave reserves its next unit when it starts on the current one (the atomic's answer is there when it is wanted);
  // 0 = it asks when it needs one.  In: -1 = launch_bounce decides (0: measured), CLWH_TUNE_UNIT_AHEAD forces 0 / 1
  int32_t unit_ahead;  // (behind the table: every older field keeps its place in the argument segment)
};

// ---- repack arguments (volume + sdf + TF -> step bytes + hit records)
struct RepackArgs {
  const int16_t *volume;
  const int8_t *sdf;
  int32_t X, Y, Z;
  int32_t NBX, NBY, NBZ;
  uint2 *grec;
  uint8_t *stepb;
  uint32_t *brick_min;     // per brick: 0 if a voxel may be an event or has a non-positive SDF value, else the smallest SDF value
  const uint8_t *cls_in;   // opaque TF: class byte per voxel (linear), computed by the JIT classifier
  TfDev tf;
};

// ---- SDF build arguments
struct SdfArgs {
  const int16_t *volume;
  int32_t X, Y, Z;
  int8_t *ping;
  int8_t *pong;
  int32_t max_iterations;
  int32_t iteration;
  int32_t *counters;   // [layer] write counts
  int32_t *done;       // [layer] early-out chain (fused build only; nullptr for the generic launch)
  int32_t *counter_out;  // generic launch: the caller's `add_buffer`
  const uint8_t *cls_in; // opaque TF: class byte per voxel (linear)
  TfDev tf;
};

// host-side launchers implemented in the .hip files
hipError_t launch_repack(const RepackArgs &a, hipStream_t s);
// log2 of the macro cell's edge: 16 voxels up to 512^3, then growing with the volume so that the table (8 B per cell) stays at a
// few hundred KB, resident in every L2 -- at 2048^3 cells of 16^3 would make it 16 MiB and every look-up a miss of its own
inline int macro_cell_shift(int X, int Y, int Z, int forced) {
  if (forced >= 3 && forced <= 8) return forced;  // CLWH_TUNE_MACRO_SHIFT (tests, experiments; 3: a cell is one brick)
  // 16-voxel cells while the table stays L2-sized (512^3: 33^3 cells x 8 octants = 0.3 MB); beyond that 32-voxel cells up to 2048^3 (65^3
  // cells, 2.2 MB: measured 28.3-28.5 ms per launch against 29.2-29.3 with 64-voxel cells and 29.2-30.2 with 16-voxel cells), then larger
  auto cells = [&](int sh) { return (int64_t)((X >> sh) + 1) * ((Y >> sh) + 1) * ((Z >> sh) + 1); };
  int shift = 4;
  if (cells(4) > 40000) {
    shift = 5;
    while (shift < 8 && cells(shift) > 300000) ++shift;
  }
  return shift;
}
hipError_t launch_macro_table(const uint32_t *brick_min, int NBX, int NBY, int NBZ, uint8_t *macro, int X, int Y, int Z, int shift, hipStream_t s);
// The start-certificate table of scene_kernels.hip: `regular` (one word) and `table` (X * Y * Z bytes) are written.
// `ends` (optional): Y * Z int2, a row's first and last event voxel (X, -1: none) for the hull table
hipError_t launch_start_table(const uint8_t *stepb, uint8_t *table, uint32_t *regular, int2 *ends, int X, int Y, int Z, int NBX, int NBY, int NBZ, hipStream_t s);
// The largest step value the start certificate's bound counts on: the SDF build's layer count, min(127, largest dimension / 2)
// (signed_distance_field.cpp), at which its values saturate.
inline int start_cert_cap(int X, int Y, int Z) {
  const int longest = X > Y ? (X > Z ? X : Z) : (Y > Z ? Y : Z);
  return longest / 2 < 127 ? longest / 2 : 127;
}
// The smallest min |direction component| (a multiple of 1/64) with which a first leg that holds a start certificate is PROVEN to leave
// the volume within its 70 steps.  The leg's box -- from its start voxel to the volume corner its octant heads for -- holds no event
// voxel, every one of its positions lies in that box (a march's coordinates are monotone in binary32), and the table is only built
// from step bytes for which k_start_regular has checked that a voxel m >= 1 voxels (Chebyshev) from the nearest voxel that touches an
// event has a step of at least min(cap, m + 1), cap = start_cert_cap, and every voxel that is no event a step of at least 1 (what
// the converged SDF, min(D + 1, cap) with D the corner-neighbour distance to the nearest non-homogeneous voxel, gives: every
// non-homogeneous voxel touches an event voxel).  After a path of length t every coordinate has moved at least t * dmin away from the
// box's three inner faces, so the voxel is at least floor(t * dmin) - 2 voxels from each of them (one voxel for the start position's
// fraction, one for the accumulated rounding of at most 70 additions), all voxels that close are in the box and hence no events, and
// the step taken there is at least max(1, min(cap, floor(t * dmin) - 2)).  The bound grows with t and the real steps are no shorter,
// so by induction the real path is at least as long as this recurrence's after every step.  Once t exceeds sqrt(3) * (largest
// dimension + 1) the largest direction component (at least (1 - 2^-20) / sqrt(3) for a normalised direction) has carried its
// coordinate out of the volume.  That has to happen within 70 - 5 steps: the 5 are certify_exit's reserve (a coordinate exactly on
// the far face, the strictness of exited_volume).  The result is never below 1/64, far above the 2^-10 under which a ray can crawl
// along the far face (certify_exit); 2 = no direction qualifies.
inline float start_cert_dmin(int X, int Y, int Z) {
  const double longest = (double)(X > Y ? (X > Z ? X : Z) : (Y > Z ? Y : Z));
  const double reach = 1.7320508075688772 * (longest + 1.0), cap = (double)start_cert_cap(X, Y, Z);
  for (int k = 1; k <= 64; ++k) {
    const double dmin = (double)k / 64.0;
    double t = 0.0;  // (integers throughout: exact)
    for (int step = 0; step < 70 - 5 && t <= reach; ++step) {
      const double m = (double)(long long)(t * dmin) - 2.0;
      const double bound = m > cap ? cap : m;
      t += bound < 1.0 ? 1.0 : bound;
    }
    if (t > reach) return (float)dmin;
  }
  return 2.0f;
}
// ---- hull certificates: the support table of the event voxels over a fixed set of directions (k_hull_*, scene_kernels.hip)
constexpr int kHullGrid = 64;                           // the directions: the cell centres of an octahedral grid of 64 x 64 (hull_direction, bounce_device.hpp)
constexpr int kHullPlanes = kHullGrid * kHullGrid;
// Every stored h_k is the binary32 maximum of n_k . c over the corners plus this slack.  It covers, with room to spare: the roundings
// of that maximum and of k_primary's n_k . P (each below 2^-10 for coordinates up to kHullMaxDim), the march's own roundings (70
// additions, half an ulp of a coordinate below 2^11 each, on three axes: below 2^-5), and n_k being 2^-22 off unit length.  So a
// start point with n_k . P - h_k >= 0 in binary32 is, in the reals, more than 2^-5 in front of the plane: the bound's m0 is 0.
constexpr float kHullSlack = 0.0625f;
constexpr int kHullMaxDim = 2048;                       // no table for a longer volume
// The smallest direction . n_k (a multiple of 1/64) with which a first leg that starts in front of plane k (margin m0 = 0 after the
// slack) is PROVEN to leave the volume within its 70 steps.  Every event voxel lies behind the plane; after a path t the position is at
// least t * delta0 in front of it (the direction is constant, the roundings are in the slack), hence at least that far, Euclidean, from
// every point of every event voxel, and its voxel at least floor(t * delta0 / sqrt(3)) - 2 voxels (Chebyshev) from every event voxel.
// By the regularity of the step bytes (k_start_regular; the table is only built from bytes that pass) the step taken there is at least
// min(cap, that distance) and never below 1: no voxel in front of the plane is an event.  The bound grows with t and the real steps
// are no shorter, so the real path is at least the recurrence's after every step; once t exceeds sqrt(3) * (largest dimension + 1) the
// largest direction component has carried its coordinate out of the volume.  70 - 5 steps: certify_exit's reserve.  2 = none qualifies.
inline float hull_cert_delta0(int X, int Y, int Z) {
  const double longest = (double)(X > Y ? (X > Z ? X : Z) : (Y > Z ? Y : Z));
  const double reach = 1.7320508075688772 * (longest + 1.0), cap = (double)start_cert_cap(X, Y, Z);
  for (int k = 1; k <= 64; ++k) {
    const double delta0 = (double)k / 64.0;
    double t = 0.0;
    for (int step = 0; step < 70 - 5 && t <= reach; ++step) {
      const double m = (double)(long long)(t * delta0 / 1.7320508075688772) - 2.0;
      const double bound = m > cap ? cap : m;
      t += bound < 1.0 ? 1.0 : bound;
    }
    if (t > reach) return (float)delta0;
  }
  return 2.0f;
}
// Deferred grants and rebounds.  The theorem above asks nothing of where a march comes from: a position in front of
// plane k, a constant direction with d . n_k >= delta0, and `budget` steps left carry the march out of the volume if the recurrence gets
// there in budget - 5 steps.  k_bounce applies it to every march of fresh budget 70 that starts from a bounce (never to the
// continuation of a march that ran out of steps), first legs and rebounds from secondary hits alike:
//   start   the march's first position, (hit position + incoming direction) + 2 * the bounce's normal, in binary32;
//   P       the first legs' start point, rebuilt from the lane's copy of the hit with k_primary's own operations (origin + direction, then
//           + normal * 2: the same bits);
//   m_q     the margin k_primary stored for P against plane k, rounded DOWN to a multiple of 1 / kHullMarginScale (hull_planes);
//   m       = m_q + n_k . (start - P), the march's own margin.  For a first leg start == P bit for bit and m == m_q.
// (a) m >= 0 and d . n_k >= hull_cert_delta0: the theorem as it stands, granted before the first step.
// (b) 0 < -m <= kHullDeferDeficit and d . n_k >= hull_defer_delta0: the lane marches literally and counts its path in the low field of
//     `march` (one add of the step byte's value per step; the step itself is max(value, 0.5), so the count never exceeds the path).
//     Once the count reaches ceil(-m / d . n_k) the position is start + t * d with t * (d . n_k) >= -m: in front of the plane.  If no
//     event has ended the march and it has taken at most kHullDeferSteps steps, at least 70 - kHullDeferSteps are left, and the
//     theorem holds with hull_defer_delta0, the same recurrence over 70 - 5 - kHullDeferSteps steps.  A lane that gets there later
//     drops the claim and asks the macro-cell table like any other.
// Rounding budget of m, in voxels, for coordinates up to kHullMaxDim = 2^11 (differences and partial sums below 2^13, half an ulp
// at most 2^-12): m_q is rounded down, which only errs to the safe side; P is bit-identical to k_primary's, whose own n_k . P and the
// table's maximum are in kHullSlack already (2 x 2^-10); the three subtractions start - P (3 x 2^-12, times |n| <= 1), three
// products, two additions and the addition of m_q (6 x 2^-12): below 2^-9 + 2^-10 in all.  ceil(-m / d . n_k) is taken from a reciprocal
// good to 2^-22 and widened by 2^-19: it never falls below the quotient.  kHullSlack = 2^-4 has to hold 2 x 2^-10 (support and n_k . P),
// 2^-5 (the march's 70 additions -- a deferred grant's literal steps are among them), 2^-10 (|n_k| off by 2^-22 at 2^12) and now 3 x 2^-10:
// 2^-5 + 6 x 2^-10 < 0.038 of 0.0625.  It fits; the slack is not touched and no guard is subtracted.
// The direction guards are item 12's: no NaN, min |component| >= 2^-10.  A NaN in start or P makes m a NaN, which fails both tests.
constexpr int kHullDeferSteps = 3;            // J: the most literal steps a march may have taken when a deferred grant fires
constexpr float kHullDeferDeficit = 1.5f;     // D: planes further than this in front of the start point are not worth waiting for
constexpr int kHullMarginScale = 16;          // the stored margin's grid: 1/16 voxel, eight bits signed (-8 .. +7.9375, clamped)
inline float hull_defer_delta0(int X, int Y, int Z, int J = kHullDeferSteps) {
  const double longest = (double)(X > Y ? (X > Z ? X : Z) : (Y > Z ? Y : Z));
  const double reach = 1.7320508075688772 * (longest + 1.0), cap = (double)start_cert_cap(X, Y, Z);
  for (int k = 1; k <= 64; ++k) {
    const double delta0 = (double)k / 64.0;
    double t = 0.0;
    for (int step = 0; step < 70 - 5 - J && t <= reach; ++step) {
      const double m = (double)(long long)(t * delta0 / 1.7320508075688772) - 2.0;
      const double bound = m > cap ? cap : m;
      t += bound < 1.0 ? 1.0 : bound;
    }
    if (t > reach) return (float)delta0;
  }
  return 2.0f;
}
// Tilted planes.  The theorem asks nothing of WHICH plane of the table a march names either: every corner of every
// event voxel lies behind every plane k (n_k . c <= h_k - kHullSlack, k_hull_*), so a position in front of plane k', a constant direction
// with d . n_k' >= delta and 70 - J steps left carry the march out of the volume exactly as in items 12 and 13.  A march of fresh budget
// 70 that starts from a bounce and that the hit's own plane neither grants nor arms picks k' in closed form:
//   n0   the hit's plane normal n_k (hull_direction of the hit's word; a hit without a word: the bounce's own normal),
//   c    = d . n0,  t = hull_defer_delta0(J) + kHullTiltMargin,  lambda = 0 if c >= t, else -c + sqrt(1 - c^2) * t / sqrt(1 - t^2),
//   n'   = n0 + lambda d: the vector of the plane spanned by n0 and d with d . n' / |n'| = t that is nearest n0,
//   k'   = hull_cell(n'), the octahedral cell n' falls in (bounce_device.hpp).
// None of this is part of the proof -- ANY cell is safe, a NaN included (hull_cell clamps it into the table); only the yield depends on
// it.  The proof starts at the two numbers formed from k' itself, with the operations of items 12 and 13:
//   dn'  = d . n_k',  n_k' = hull_direction(k'), the same bits as in the table's builder;
//   M'   = n_k' . start - h_k', start the march's first position in binary32, h_k' read from the table (hull_h).
// (a) M' >= 0 and dn' >= hull_cert_delta0: granted before the first step.
// (b) M' < 0, dn' >= hull_defer_delta0(J) and need = ceil(-M' / dn') <= kHullTiltPath: armed exactly as item 13 arms (kArmed, the low field
//     of `march` at kCertReady - need); the certificate phase fires the grant if at most J steps were taken.  After a counted path >= need
//     the position is start + t d with t dn' >= -M': in front of plane k'.  No deficit limit D; the path limit is no part of the proof
//     either: an armed lane cannot ask the macro-cell table before it has counted its path, so the path has to end in the near field.
// The step loop compares against ONE J per launch (a constant picked by the wave-uniform flag), so with the rule on item 13's armed
// marches take kHullTiltSteps and its delta as well.
// Rounding budget of M' against kHullSlack = 2^-4: n_k' . start is k_primary's n_k . P with another k -- coordinates below 2^11 + 3, three
// products and two additions of half an ulp (2^-13) each, the subtraction of h_k' one more: below 2^-10, the share the slack already
// reserves for "k_primary's n_k . P"; the table's maximum 2^-10; the march's 70 additions 2^-5 (the literal steps before a deferred grant
// are among them); |n_k'| off by 2^-22 at 2^12: 2^-10.  Item 13's relative margin (3 x 2^-10) is not used on this path.  2^-5 + 3 x 2^-10
// < 0.035 of 0.0625: it fits, the slack is not touched and no guard is subtracted.  need comes from a reciprocal good to 2^-22, widened
// by 2^-19: never below the quotient.  Direction guards as in items 12 and 13: no NaN, min |component| >= 2^-10; a NaN in start or in
// h_k' (+inf: no event voxel, or step bytes that are not regular) makes M' a NaN or -inf, which fails (a) and (b).
constexpr int kHullTiltSteps = 16;                // J with tilted planes (tools/hull_tilt.py; 12 / 16 / 20 on the GPU: profiles/bounce_hull_tilt_ab.txt)
constexpr float kHullTiltMargin = 0.0625f;        // the tilt aims this far above delta(J), so that the cell's own normal still qualifies
constexpr int kHullTiltPath = 48;                 // P: the longest path a tilted plane may ask a march to count before its grant
// `ends`: scratch of Y * Z int2 (k_start_rows leaves a row's first and last event voxel there); `hull`: kHullPlanes float4;
// `hull_h`: kHullPlanes floats, the entries' h_k alone
hipError_t launch_hull_table(const int2 *ends, const uint32_t *regular, float4 *hull, float *hull_h, int X, int Y, int Z, hipStream_t s);
constexpr uint64_t kStartTableBudget = 2ull << 30;  // bytes (= voxels): larger volumes get no start certificates
hipError_t launch_primary(const RenderArgs &a, hipStream_t s);
hipError_t launch_bounce(const RenderArgs &a, hipStream_t s);
// the bounce kernel's queue arithmetic needs ceil(hits / 64) x seeds below 2^24 (64 seeds: 16.7 M hit pixels); udivmod24
inline bool bounce_queues_fit(uint32_t n_hits, int32_t unit_block_log2, int32_t n_seeds) {
  return (uint64_t)(((n_hits + 63u) >> 6) + 8u * (1u << unit_block_log2)) * (uint64_t)n_seeds < (1ull << 24);
}
hipError_t launch_env_fixup(const RenderArgs &a, hipStream_t s);
hipError_t launch_commit(const RenderArgs &a, hipStream_t s);
// planned voxel-cache launches: sort keys of the camera's hits (their cache entries), the token deal of one launch, the launch's sums into the cache
constexpr int64_t kVoxKeyInvalid = (int64_t)1 << 38;  // a hit whose entry lies outside the cache; kVoxKeyNone: no such hit (padding)
constexpr int64_t kVoxKeyNone = ((int64_t)1 << 38) + 1;
hipError_t launch_vox_keys(const RenderArgs &a, int64_t *keys, uint32_t *iota, uint32_t n, hipStream_t s);
hipError_t launch_vox_grant(const RenderArgs &a, const int64_t *sorted_keys, const uint32_t *order, uint32_t n, uint32_t *grants, hipStream_t s);
hipError_t launch_commit_voxel(const RenderArgs &a, hipStream_t s);
// stable radix sort of (entry, position) pairs on bits [0, end_bit) (exchange_kernels.hip: the one translation unit with rocPRIM)
hipError_t sort_entry_pairs(void *temp, size_t &temp_bytes, const int64_t *keys_in, int64_t *keys_out, const uint32_t *vals_in,
                            uint32_t *vals_out, size_t n, unsigned end_bit, hipStream_t s);
hipError_t launch_resolve(const RenderArgs &a, hipStream_t s);
hipError_t launch_ao(const RenderArgs &a, hipStream_t s);
hipError_t launch_accum_resolve(const RenderArgs &a, const float4 *accum_all, hipStream_t s);
hipError_t launch_accum_resolve_tiles(const RenderArgs &a, const float4 *accum, uint32_t *tiles_out, hipStream_t s);
hipError_t launch_frame_from_tiles(const RenderArgs &a, const uint32_t *tiles_all, hipStream_t s);
// clwh_debug_device_probe (probe_kernels.hip): words per record of probe `which` ({0, 0}: no such probe), and its launch
struct ProbeShape {
  uint32_t in_words, out_words;
};
ProbeShape probe_shape(int which);
hipError_t launch_device_probe(int which, const uint32_t *in, uint64_t n, uint32_t *out, const uint32_t *aux, const int32_t params[4], hipStream_t s);
// ---- fused SDF build: one breadth-first layer over the active 8x8x8 tiles (sdf_front_kernels.hip)
struct SdfFrontArgs {
  int8_t *sdf;
  int32_t X, Y, Z;
  int32_t TX, TY, TZ;         // 8x8x8 tiles per axis
  const uint8_t *flags_cur;   // tiles that settled voxels in the previous layer (or hold |v| == 1 for layer 1)
  uint8_t *flags_next;        // tiles that settle voxels in this layer
  uint8_t *flags_clear;       // third buffer, zeroed here for the layer after next
  uint8_t *tile_done;         // 1: every voxel of the tile is settled, the tile is never visited again
  int32_t iteration;
  int32_t max_iterations;
  int32_t *counters;          // [i] != 0: layer i settled a voxel to a value < max_iterations; [0] != 0: some |v| == 1
};

// ---- fused SDF build, bit-parallel (sdf_bits_kernels.hip, sdf_bits_layers_kernels.hip): one bit per voxel, eight layers per launch
struct SdfBitArgs {
  int8_t *sdf;
  const uint32_t *ev;      // event bit per voxel, rows of WP 32-bit words
  const uint32_t *r_in;    // reached set after r0 layers
  uint32_t *r_out;         // reached set after r0 + steps layers (core rows of the active blocks)
  uint8_t *state;          // per block of sdfbit_block_grid: 0 empty, 1 some, 2 complete (just now), 3 complete in both buffers
  uint8_t *wake;           // per block: launch index + 1 for which a neighbour's reached voxels came within 8 voxels of its core
  int32_t launch;          // index of this launch (8 layers each)
  int32_t *presence;       // [D] != 0: some voxel lies D corner moves from the nearest seed; [0]: a seed exists
  int32_t X, Y, Z, WP;
  int32_t BX, BY, BZ, core_z;  // blocks of 64 x 48 x core_z voxels (sdfbit_block_grid)
  int32_t r0, steps;       // steps <= 8
  uint32_t *planes;        // seven bit planes of the layer index (8 launch + layer-in-launch + 1, 1..127) of every voxel a layer reached,
                           // each tiled like the reached sets; OR-ed in by the launches, expanded to bytes ONCE by k_sdfbit_expand
  size_t plane_words;      // words per plane
  uint32_t *list;          // blocks that can change in this launch (k_sdfbit_list)
  uint32_t *list_count;    // their number; list_head: the persistent grid's queue position
  uint32_t *list_head;
#ifdef CLVR_SDFBIT_TIMING
  unsigned long long *timing;  // tools/ builds only: per-phase sums of wall_clock64 ticks over all regions
#endif
};
void sdfbit_block_grid(int X, int Y, int Z, int waves, int32_t *BX, int32_t *BY, int32_t *BZ, int32_t *core_z);  // blocks of 64 x 48 x (4 waves - 16) voxels
hipError_t launch_sdfbit_events(const SdfArgs &a, uint32_t *ev, int32_t WP, hipStream_t s);
hipError_t launch_sdfbit_seed(const SdfBitArgs &a, hipStream_t s);                                // seeds into a.r_out
hipError_t launch_sdfbit_expand(const SdfBitArgs &a, const uint32_t *reached, int32_t max_iterations, hipStream_t s);  // bit planes + final reached set -> a.sdf
hipError_t launch_sdfbit_state(const SdfBitArgs &a, hipStream_t s);                              // block states of a.r_in
hipError_t launch_sdfbit_layers(const SdfBitArgs &a, int waves, unsigned grid_blocks, bool rec_in_lds, hipStream_t s);

// block and grid of the kernels that give a thread one voxel of an x-row (k_sdf_base, k_sdf_layer, k_apply_clip): blockIdx = (row chunk, y, z)
inline unsigned row_block(int X) { return X <= 64 ? 64u : (X <= 128 ? 128u : 256u); }
inline dim3 row_grid(int X, int Y, int Z) { return dim3(((unsigned)X + row_block(X) - 1u) / row_block(X), (unsigned)Y, (unsigned)Z); }
hipError_t launch_sdf_base(const SdfArgs &a, hipStream_t s);
hipError_t launch_sdf_base_front(const SdfArgs &a, uint8_t *flags, int32_t TX, int32_t TY, hipStream_t s);
hipError_t launch_sdf_front(const SdfFrontArgs &a, hipStream_t s);
hipError_t launch_sdf_layer(const SdfArgs &a, hipStream_t s);
hipError_t launch_fetch_stats(const int16_t *vol, int X, int Y, int Z, int32_t *stats, hipStream_t s);
hipError_t launch_tf_sort_values(const int16_t *vol, int X, int Y, int Z, uint32_t *frame, int width, int height,
                                 float min_v, float max_v, float min_g, float max_g, hipStream_t s);
hipError_t launch_tf_flush_color_frame(uint32_t *color_frame, int fw, int fh, const int32_t *frame, const int32_t *lookup,
                                       int lookup_len, hipStream_t s);
hipError_t launch_bilateral_filter(const int16_t *src, int X, int Y, int Z, int16_t *dst, const float *weights, hipStream_t s);
hipError_t launch_apply_clip(const int16_t *src, int SX, int SY, int SZ, int16_t *dst, int DX, int DY, int DZ,
                             const uint32_t *start, const uint32_t *len, hipStream_t s);

// ---- the views of the bricked volume (clwh_views.hip, clwh_mesh.hip): intensity projections, compositing, the isosurface, slices and
// the isosurface mesh.  Their kernel arguments are composed of three blocks (plain members: memset and pass-by-value stay valid).

// The derived data every view reads.  `bricks`: the caller's S16 image in brick order (packed_volume.hpp inner_index, one 4^3 sub-brick
// = one 128-byte line), NBX * NBY * NBZ * 512 voxels.  `table`: per 8^3 brick (uint16)min | (uint16)max << 16 over its real voxels.
// Both are built by k_proj_repack (ensure_projection_data).  `dilated`: the same pair over the voxels within one voxel of the brick
// (clamped at the volume's faces); `coarse`, stored behind it: the pair per cell of 4^3 bricks (CNX x CNY x ceil(NBZ / 4) cells).
// Both are built by k_iso_dilate / k_iso_coarse and nullptr until ensure_dilated_table has run.
struct ViewVolume {
  const int16_t *bricks;
  const uint32_t *table, *dilated, *coarse;
  int32_t X, Y, Z, NBX, NBY, NBZ, CNX, CNY;
};
// where an image view writes: one wave per 8x8 pixel tile of the launched region
struct ViewFrame {
  uint32_t *frame;        // RGBA8 packed, row-major, frame_w x frame_h
  int32_t frame_w, frame_h;
  int32_t launch_w, launch_h, tiles_x, num_tiles;
};
// the camera and the march along its rays
struct ViewCamera {
  float cam_pos[3], cam_dir[3];
  float step, t_near, t_far;
  int32_t k_cap;          // every kept sample has k < k_cap (view_march_ok checks the camera distance / step)
};

// ---- intensity projections (projection_kernels.hip)
struct ProjRepackArgs {
  const int16_t *volume;  // the caller's image, x fastest
  int32_t X, Y, Z, NBX, NBY, NBZ;
  int16_t *bricks;        // ViewVolume::bricks
  uint32_t *table;        // ViewVolume::table
};
struct ProjArgs {
  ViewVolume vol;
  ViewFrame fr;
  ViewCamera cam;
  float window_center, window_width;
  float *values;          // optional, row-major launch_w x launch_h
  float *t_extreme;       // optional, same
};
hipError_t launch_proj_repack(const ProjRepackArgs &a, hipStream_t s);
hipError_t launch_projection(const ProjArgs &a, int mode, bool dense, hipStream_t s);

// ---- compositing through a colour/opacity table (composite_kernels.hip): beside the volume the table's prefix count of entries with
// a > 0, built by k_comp_prefix
struct CompArgs {
  ViewVolume vol;
  ViewFrame fr;
  ViewCamera cam;
  const float4 *lut;      // lut_len entries (r, g, b, a), 16-byte aligned
  const uint32_t *prefix; // prefix[i] = number of entries j <= i with a > 0
  int32_t lut_first, lut_len;
  float alpha_stop, ambient;
  float4 *rgba;           // optional, row-major launch_w x launch_h
  float *t_first;         // optional, same
  float *t_stop;          // optional, same
};
hipError_t launch_comp_prefix(const float4 *lut, int32_t lut_len, uint32_t *prefix, hipStream_t s);
hipError_t launch_composite(const CompArgs &a, bool shade, bool dense, hipStream_t s);

// ---- isosurface of the trilinear field (isosurface_kernels.hip)
struct IsoArgs {
  ViewVolume vol;
  ViewFrame fr;
  ViewCamera cam;
  int64_t threshold;       // T = floor(iso * 2^24)
  int32_t skip_bound;      // a brick is stepped over iff dmax < skip_bound (ceil(T / 2^24)), BELOW: iff dmin > skip_bound (floor(T / 2^24))
  int32_t refine;
  float color[3], ambient;
  float *t_hit;            // optional, row-major launch_w x launch_h
  float4 *normal;          // optional, same
};
// `dilated` receives v.NBX * v.NBY * v.NBZ entries followed by the cells' (ViewVolume::coarse)
hipError_t launch_iso_dilate(const ViewVolume &v, uint32_t *dilated, hipStream_t s);
hipError_t launch_isosurface(const IsoArgs &a, bool below, bool dense, hipStream_t s);

// ---- oblique slices and thick slabs of the trilinear field (slice_kernels.hip): parallel rays with one origin per pixel; MAX / MIN may
// step over bricks (and cells of 4^3 bricks) by the dilated tables, which stay nullptr when the launch cannot skip (MEAN,
// CLWH_SLICE_DENSE)
struct SliceArgs {
  ViewVolume vol;
  ViewFrame fr;
  int32_t use_coarse;      // 1: ask the cell of 4^3 bricks first (Tuning::slice_coarse)
  float origin[3], du[3], dv[3], normal[3];
  float step;
  float window_center, window_width;
  int32_t slab_samples;    // 1 .. 8192: the sample indices' cap
  float *values;           // optional, row-major launch_w x launch_h
  float *t_extreme;        // optional, same
};
hipError_t launch_slice(const SliceArgs &a, int mode, bool dense, hipStream_t s);

// ---- the curved reformat and the section profile along a curve (curved_kernels.hip).  `rows`: nine floats per station -- origin[3],
// du[3], normal[3] in voxel space -- in the context's buffer (CurveScratch), launch_h rows for the view and n_rows for the profile.
// The view is the slice with a frame per image row; its dilated tables stay nullptr when the launch cannot skip.
struct CurvedArgs {
  ViewVolume vol;
  ViewFrame fr;
  int32_t use_coarse;      // as SliceArgs
  const float *rows;
  float step;
  float window_center, window_width;
  int32_t slab_samples;    // 1 .. 8192: the sample indices' cap
  float *values;           // optional, row-major launch_w x launch_h
  float *t_extreme;        // optional, same
};
hipError_t launch_curved(const CurvedArgs &a, int mode, bool dense, hipStream_t s);
struct CurveProfileArgs {
  const unsigned long long *mask;  // grow's layout: W64 64-bit words per row of X voxels
  int32_t X, Y, Z, W64;
  const float *rows;
  uint32_t n_rows;         // the grid: one wave per station
  int32_t width, slab_samples;  // 1 .. 64 each: lanes and bits of a lane's word
  float step;
  uint32_t *records;       // n_rows x {count, sum_x, sum_k, border}, 16-byte aligned
};
hipError_t launch_curve_profile(const CurveProfileArgs &a, bool connected, hipStream_t s);

// ---- the isosurface as an indexed triangle mesh (mesh_kernels.hip): marching tetrahedra, one block per 8^3 brick; without
// CLWH_MESH_DENSE the dilated table says which bricks the surface can touch
struct MeshArgs {
  ViewVolume vol;          // `dilated` is read when `skip` is set
  uint64_t n_bricks;       // NBX * NBY * NBZ: the grid of every launch
  int32_t lo[3], hi[3];    // the box in grid points, lo < hi <= dim - 1 on every axis
  int64_t threshold;       // T = floor(iso * 2^24)
  int32_t in_bound;        // V is inside iff V >= in_bound (ceil(T / 2^24)), below: iff V <= in_bound (floor(T / 2^24))
  int32_t below, skip;
  // three columns of n_bricks + 1 words each: vertices, triangles, "has a vertex" per brick, the last word 0 -- `counts` as k_mesh_count
  // writes them, `bases` their exclusive scans (so the last word of a column is its total)
  uint64_t *counts;
  const uint64_t *bases;
  uint32_t *points;        // per brick with a vertex (slot = bases[2][brick]) 512 words: edge mask | rank << 8 per grid point
  float *positions;        // [n_vertices][3]
  float *normals;          // optional, same
  uint64_t *keys;          // optional, [n_vertices]
  uint32_t *triangles;     // optional, [n_triangles][3]
};
hipError_t launch_mesh_count(const MeshArgs &a, hipStream_t s);
hipError_t launch_mesh_scan(void *temp, size_t &temp_bytes, const uint64_t *counts, uint64_t *bases, size_t n, hipStream_t s);
hipError_t launch_mesh_fill(const MeshArgs &a, hipStream_t s);  // k_mesh_vertices, then k_mesh_triangles if `triangles` is given

// ---- seeded region growing and masked volumes (grow_kernels.hip; host side clwh_grow.hip).  Bit images (the mask R, the admissible
// image A) hold a row of the volume as W64 = ceil(X / 64) 64-bit words, row (z * Y + y); the volume is cut into tiles of 64 x 16 x 16
// voxels, tile (tx, ty, tz) at (tz * TY + ty) * TX + tx: one word of each of its 256 rows.
constexpr int kGrowBatch = 8;  // rounds enqueued between two reads of the device's counters: {listed, ticket} x 8 = the 64 pinned bytes
// the tile worklist of a search that runs in rounds (grow's and the geodesic maps'; the protocol is in tile_work_device.hpp)
struct TileWork {
  int32_t TX, TY, TZ;          // the grid of tiles
  int32_t dense;               // CLWH_GROW_DENSE, CLWH_GEO_DENSE: one stamped tile lists them all
  uint32_t *stamps;            // per tile: the round (1, 2, ...) in which it is to be visited
  uint32_t *list;              // the tiles of the round being run
  uint32_t *counters;          // kGrowBatch x {tiles listed, ticket}
};
// k_tile_list (tile_work_kernels.hip) into counters[2 * slot]; launch_tile_round, its one caller, asks for the error behind both launches
void enqueue_tile_list(const TileWork &w, uint32_t round, int slot, hipStream_t s);
struct GrowDeviceResult {      // what k_grow_reduce accumulates (grow_result_identity: the start values)
  unsigned long long count, sum, sum_sq;  // sum: int64 in two's complement
  int32_t vmin, vmax;
  uint32_t lo[3], hi[3];       // hi inclusive here
};
struct GrowArgs {
  const int16_t *volume;       // the caller's image, x fastest
  unsigned long long *mask;    // R
  unsigned long long *adm;     // A
  int32_t X, Y, Z, W64;
  int32_t lo, hi;              // the window
  int32_t box_lo[3], box_hi[3];
  int32_t conn26, from_mask;
  TileWork tiles;
  const uint32_t *seeds;       // device copy, uint32[n_seeds][3]
  uint32_t n_seeds;
  GrowDeviceResult *result;
};
hipError_t launch_grow_admissible(const GrowArgs &a, hipStream_t s);  // A; mask &= A or mask = 0; stamps of the tiles that hold a bit
hipError_t launch_grow_seeds(const GrowArgs &a, hipStream_t s);
hipError_t launch_grow_round(const GrowArgs &a, uint32_t round, int slot, hipStream_t s);  // k_tile_list + k_grow_round, counters[2 * slot]
hipError_t launch_grow_reduce(const GrowArgs &a, hipStream_t s);
hipError_t launch_apply_mask(const int16_t *in, int16_t *out, const unsigned long long *mask, int32_t X, int32_t Y, int32_t Z, int32_t W64,
                             int32_t fill, int32_t invert, hipStream_t s);

// ---- connected-component labelling and rank selections (label_kernels.hip; host side clwh_label.hip), over grow's bit rows
struct LabelRecord {           // clwh_label_component, as the kernels write it
  unsigned long long count;
  uint32_t first[3], lo[3], hi[3];  // hi exclusive
  uint32_t reserved;
};
struct LabelArgs {
  const int16_t *volume;       // the caller's image, x fastest
  const unsigned long long *mask;  // CLWH_LABEL_FROM_MASK: the caller's mask, read only; else null
  unsigned long long *adm;     // A
  uint32_t *labels;            // the caller's buffer: the runs' parent words until the last kernel writes every word
  int32_t X, Y, Z, W64;
  int32_t lo, hi;              // the window
  int32_t box_lo[3], box_hi[3];
  int32_t conn26;
  unsigned long long *counters;  // {roots, admissible voxels, slots handed out}
  unsigned long long *keys_in, *keys_out;  // ~count << 32 | first, per component
  uint32_t n_roots;            // known to the host after launch_label_classes
  uint32_t n_records;          // min(n_roots, component_capacity), 0 without a table
  LabelRecord *records;
};
hipError_t launch_label_classes(const LabelArgs &a, hipStream_t s);  // A, runs, unions, flatten; counters[0], [1]
hipError_t launch_label_keys(const LabelArgs &a, hipStream_t s);     // keys_in
hipError_t launch_label_sort(void *temp, size_t &temp_bytes, const LabelArgs &a, hipStream_t s);  // keys_in -> keys_out
hipError_t launch_label_ranks(const LabelArgs &a, hipStream_t s);    // the table, every word of labels
hipError_t launch_labels_to_mask(const uint32_t *labels, unsigned long long *mask, int32_t X, int32_t Y, int32_t Z, int32_t W64, uint32_t rank_lo,
                                 uint32_t rank_hi, hipStream_t s);

// ---- distance maps of masks, ball morphology and mask algebra (distance_kernels.hip; host side clwh_distance.hip), over grow's bit rows
struct DistArgs {
  int32_t X, Y, Z, W64;
  uint32_t weight[3];          // wx, wy, wz >= 1
  unsigned long long cap;      // values above it become NONE; ~0ull: no cap
};
hipError_t launch_dist_rows(const DistArgs &a, const unsigned long long *mask, uint32_t *out, int32_t flip, hipStream_t s);  // along x, from the bits
hipError_t launch_dist_lines(const DistArgs &a, const uint32_t *src, uint32_t *dst, int32_t along_z, hipStream_t s);       // along y or z; src != dst
// the same pass by two linear scans per line; `stack`: a map's worth of words, dst holds the other half of the stack meanwhile
hipError_t launch_dist_lines_scan(const DistArgs &a, const uint32_t *src, uint32_t *dst, uint32_t *stack, int32_t along_z, hipStream_t s);
// the pass along z with the comparison instead of the map: bit = (value <= cap) != invert, padding clean
hipError_t launch_dist_lines_bits(const DistArgs &a, const uint32_t *src, unsigned long long *bits, int32_t invert, hipStream_t s);
hipError_t launch_mask_combine(const unsigned long long *a, const unsigned long long *b, unsigned long long *out, int32_t X, int32_t Y,
                               int32_t Z, int32_t W64, int32_t op, hipStream_t s);

// ---- topology-preserving thinning and the list of a mask's voxels (thin_kernels.hip; host side clwh_thin.hip), over grow's bit rows
// and grow's tiles of 64 x 16 x 16 voxels.  The counters' words: count_in (two words), then per iteration of a batch {tiles listed,
// voxels deleted}.
constexpr int kThinBatch = 4;  // iterations enqueued between two reads of the device's counters
struct ThinArgs {
  unsigned long long *mask;           // M: the caller's mask_out, thinned in place
  const unsigned long long *anchors;  // or nullptr
  unsigned long long *cand;           // C of the current iteration
  uint32_t *stamps;                   // per tile: the last iteration that listed it
  uint32_t *list;                     // the tiles that hold a candidate
  uint32_t *counters;                 // 2 + 2 * kThinBatch words
  int32_t X, Y, Z, W64;
  int32_t TX, TY, TZ;
  int32_t dense, keep_ends;
};
hipError_t launch_thin_begin(const ThinArgs &a, const unsigned long long *mask_in, hipStream_t s);  // M = mask_in without padding; count_in
// one iteration in batch slot `slot`: C and the list, then the eight sub-passes; `iteration` (1, 2, ...) is the tiles' stamp
hipError_t launch_thin_iteration(const ThinArgs &a, uint32_t iteration, int slot, hipStream_t s);
struct PointsArgs {
  const unsigned long long *mask;
  const uint32_t *map;                // or nullptr
  uint32_t *counts, *bases;           // per 64-bit word of the mask, and one more
  uint32_t *points, *values;
  int32_t X, Y, Z, W64;
};
hipError_t launch_points_count(const PointsArgs &a, hipStream_t s);
hipError_t launch_points_scan(void *temp, size_t &temp_bytes, const uint32_t *counts, uint32_t *bases, size_t n, hipStream_t s);
hipError_t launch_points_fill(const PointsArgs &a, hipStream_t s);

// ---- volume filters: median, grey min / max, exact integer smoothing (filter_kernels.hip; host side clwh_filter.hip).  One launch is
// the whole median or one line pass; `last` passes select by the mask and read the unfiltered volume at its clear bits.
struct FilterArgs {
  const int16_t *src;   // what the launch filters; never dst
  int16_t *dst;
  const int16_t *orig;  // V, read where the mask's bit is clear (with a mask only); may be dst
  const uint8_t *mask;  // grow's layout as bytes, or nullptr: every voxel takes the filtered value
  int32_t X, Y, Z, W64;
  int32_t axis, r;      // line passes: 0, 1, 2 and the radius along it, 1 .. CLWH_FILTER_MAX_RADIUS
  int32_t wide_src, wide_dst, wide_orig;  // rows_of_8 of the three arrays
  uint16_t w[CLWH_FILTER_MAX_RADIUS + 1];  // SMOOTH: the axis' weights by |offset|
};
hipError_t launch_filter_median(const FilterArgs &a, int rx, int ry, int rz, hipStream_t s);  // radii 0 or 1, not all 0
hipError_t launch_filter_line(const FilterArgs &a, int kind, hipStream_t s);                  // kind: CLWH_FILTER_MIN, _MAX or _SMOOTH

// ---- geodesic distance maps and nearest-seed territories inside a mask, and the path behind a distance (geodesic_kernels.hip; host
// side clwh_geodesic.hip).  The working keys (dist << 32 | id) are a packed array of one 64-bit word per voxel, [z][y][x] without
// padding; the volume is cut into tiles of kGeoTileX x kGeoTileY x kGeoTileZ voxels, tile (tx, ty, tz) at (tz * TY + ty) * TX + tx; rounds are grow's.
// The tile's core; a block of 256 threads owns it, a thread the column along z at its (x, y).  16 x 16 x 8 is what was measured best
// (DESIGN.md, section 4); the macros are there so that tools/time_geodesic.py can time another build of the library against it.
#ifndef CLVR_GEO_TILE_X
#define CLVR_GEO_TILE_X 16
#define CLVR_GEO_TILE_Y 16
#define CLVR_GEO_TILE_Z 8
#endif
constexpr int kGeoTileX = CLVR_GEO_TILE_X, kGeoTileY = CLVR_GEO_TILE_Y, kGeoTileZ = CLVR_GEO_TILE_Z;
static_assert(kGeoTileX * kGeoTileY == 256 && kGeoTileZ >= 1 && kGeoTileZ <= 32, "a thread per column, a bit per voxel of it");
struct GeoDeviceResult {       // what k_geo_finish accumulates, zero on entry
  unsigned long long reached;
  uint32_t max_dist, reserved;
};
struct GeoArgs {
  const uint8_t *domain;       // grow's bit rows, read only
  const uint32_t *seed_labels; // CLWH_GEO_FROM_LABELS: the caller's words; else null
  unsigned long long *keys;    // scratch, one per voxel
  uint32_t *dist, *labels;     // the caller's maps; either may be null
  int32_t X, Y, Z, W64;
  uint32_t w_face[3], w_edge[3], w_corner;  // the edge's index is the axis that does not change
  uint32_t cap;                // <= 0xFFFF0000
  int32_t conn26;
  TileWork tiles;
  const uint32_t *seeds;       // device copy, uint32[n_seeds][4] = x, y, z, id
  uint32_t n_seeds;
  GeoDeviceResult *result;
};
struct GeoTraceResult {
  unsigned long long n_points;
  uint32_t broken, reserved;   // broken: no direction qualified at a point with dist > 0
};
struct GeoTraceArgs {
  const uint32_t *dist, *labels;  // labels may be null
  uint32_t *points;            // [capacity][3]
  unsigned long long capacity;
  int32_t X, Y, Z;
  int32_t target[3];
  uint32_t w_face[3], w_edge[3], w_corner;
  int32_t conn26;
  GeoTraceResult *result;
};
hipError_t launch_geo_init(const GeoArgs &a, hipStream_t s);  // every key, the listed seeds, the stamps of the tiles that hold a seed
hipError_t launch_geo_round(const GeoArgs &a, uint32_t round, int slot, hipStream_t s);  // k_tile_list + k_geo_round, counters[2 * slot]
hipError_t launch_geo_finish(const GeoArgs &a, hipStream_t s);  // dist, labels, *result
hipError_t launch_geo_trace(const GeoTraceArgs &a, hipStream_t s);

// ---- shortest paths through a cost field, the path behind such a distance, and the cost field from a table (costpath_kernels.hip; host
// side clwh_costpath.hip).  The keys, the tiles and the rounds are the geodesic's; `g` holds what the two share, with the direction
// multipliers (1 .. 255) in the weights' fields, a cap <= 0xFF000000 and a domain that may be null.
struct CostArgs {
  GeoArgs g;
  const uint16_t *cost;        // [z][y][x], read only; 0 is a wall
};
struct CostTraceArgs {
  GeoTraceArgs g;
  const uint16_t *cost;
};
struct CostFieldArgs {
  const uint32_t *words;       // CLWH_COST_SRC_U32
  const int16_t *volume;       // CLWH_COST_SRC_VALUE, CLWH_COST_SRC_GRADIENT
  const uint8_t *domain;       // grow's bit rows, or null
  const uint16_t *table;       // device copy, n entries
  uint16_t *cost;
  long long lo;
  int32_t X, Y, Z, W64;
  uint32_t n, shift;
  int32_t kind;                // clwh_cost_source
};
hipError_t launch_cost_init(const CostArgs &a, hipStream_t s);   // every key, the listed seeds, the stamps of the tiles that hold a seed
hipError_t launch_cost_round(const CostArgs &a, uint32_t round, int slot, hipStream_t s);  // k_tile_list + k_cost_round, counters[2 * slot]
hipError_t launch_cost_trace(const CostTraceArgs &a, hipStream_t s);
hipError_t launch_cost_field(const CostFieldArgs &a, hipStream_t s);

// ---- seeded watershed of a cost field (watershed_kernels.hip; host side clwh_watershed.hip).  The tiles and the rounds are the
// geodesic's; its 8 bytes of scratch per voxel hold two arrays of uint32, [z][y][x] without padding: the states (M << 16 | L, all ones
// where nothing has arrived or can) and the working labels (id - 1, all ones for none).  Phase 1 (the states) and phase 2 (the labels)
// run over one worklist with a set of stamps each.
struct WsDeviceResult {        // what k_ws_finish accumulates, zero on entry
  unsigned long long reached;
  uint32_t max_level, reserved;
};
struct WsArgs {
  const uint16_t *cost;        // [z][y][x], read only; 0 is a wall
  const uint8_t *domain;       // grow's bit rows, read only, or null
  const uint32_t *seed_labels; // CLWH_GEO_FROM_LABELS: the caller's words; else null
  uint32_t *state, *wlab;      // scratch, one word per voxel each
  uint32_t *level, *labels;    // the caller's maps; either may be null
  int32_t X, Y, Z, W64;
  uint32_t plateau_cap;        // <= 65534
  uint32_t level_cap;          // <= 65535
  int32_t conn26;
  TileWork tiles;              // the phase being run: stamps is stamps_level or stamps_label
  uint32_t *stamps_level, *stamps_label;
  const uint32_t *seeds;       // device copy, uint32[n_seeds][4] = x, y, z, id
  uint32_t n_seeds;
  WsDeviceResult *result;
};
hipError_t launch_ws_init(const WsArgs &a, hipStream_t s);   // both arrays, the listed seeds, both phases' stamps of the tiles that hold a seed
hipError_t launch_ws_level_round(const WsArgs &a, uint32_t round, int slot, hipStream_t s);  // k_tile_list + k_ws_level_round, counters[2 * slot]
hipError_t launch_ws_label_round(const WsArgs &a, uint32_t round, int slot, hipStream_t s);  // k_tile_list + k_ws_label_round
hipError_t launch_ws_finish(const WsArgs &a, hipStream_t s);  // level, labels, *result

// ---- exact statistics of a mask's region and of every rank of a labelling (region_stats_kernels.hip; host side clwh_region_stats.hip).
// Records are accumulated in place, in clwh_region_stats' layout: launch_stats_init sets the identities (extremes, bbox_lo), the sums'
// kernels add with vector atomics, launch_stats_finish writes the empty record where nothing was added and makes bbox_hi exclusive.
struct MaskStatsArgs {
  const int16_t *volume;       // the caller's image, x fastest
  const uint8_t *mask;         // grow's bit rows, read only
  int32_t X, Y, Z, W64;
  clwh_region_stats *result;   // one record
  unsigned long long *tails;   // {hist_below, hist_above}, zero on entry
  unsigned long long *hist;    // n_bins words, zero on entry; nullptr: no histogram
  int32_t hist_lo;
  uint32_t bin_width, n_bins;
};
struct LabelStatsArgs {
  const int16_t *volume;
  const uint32_t *labels;      // [z][y][x]
  int32_t X, Y, Z;
  uint32_t capacity;           // ranks 1 .. capacity have a record
  int32_t mode;                // Tuning::label_stats: 0 as built; 1, 2: the experiments it was timed against
  clwh_region_stats *stats;
};
hipError_t launch_stats_init(clwh_region_stats *stats, uint32_t n, hipStream_t s);
hipError_t launch_stats_finish(clwh_region_stats *stats, uint32_t n, hipStream_t s);
hipError_t launch_mask_stats(const MaskStatsArgs &a, hipStream_t s);
hipError_t launch_label_stats(const LabelStatsArgs &a, hipStream_t s);

// ---- overlays of a mask or a labelling on a slice's or a camera view's frame (overlay_kernels.hip; host side clwh_views.hip).  The walk
// needs of `vol` only the dims and the brick and cell counts; its pointers stay nullptr.
struct OverlayArgs {
  ViewVolume vol;
  ViewFrame fr;
  ViewCamera cam;              // the camera call's rays
  float origin[3], du[3], dv[3], normal[3];  // the plane call's
  float step;                  // of either ray kind
  int32_t slab_samples;        // the plane call's cap of the sample indices
  int32_t kind;                // clwh_region_kind
  const unsigned long long *mask;  // CLWH_REGION_MASK: grow's bit rows
  const uint32_t *labels;      // CLWH_REGION_LABELS: [z][y][x]
  int32_t W64;
  uint32_t id_lo, id_hi;
  const uint32_t *occ_bricks, *occ_cells;  // 1: holds a nonzero filtered id; nullptr when the walk is dense (always for the plane)
  uint2 *pixel_ids;            // scratch: {ID, K} per pixel of the padded grid (launch_w + 2) x (launch_h + 2), pixel (-1, -1) first
  const uint32_t *palette;     // n_colours packed RGBA8 words
  uint32_t n_colours;
  int32_t flags;               // clwh_overlay_flags
  uint32_t fill_alpha, outline_alpha;
  uint32_t *ids;               // optional, row-major launch_w x launch_h
  float *t_first;              // optional, same
};
// `cells` (n_cells words) is cleared, then every word of `bricks` (NBX * NBY * NBZ) and of `cells` is written
hipError_t launch_region_occupancy(const OverlayArgs &a, uint32_t *bricks, uint32_t *cells, size_t n_cells, hipStream_t s);
// k_region_ids into a.pixel_ids, then k_overlay_blend
hipError_t launch_overlay(const OverlayArgs &a, bool camera, bool skip, hipStream_t s);

}  // namespace clvr
