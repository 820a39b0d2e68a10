// clwh_host.hpp -- host-only side of libclwhip.so: the opaque handles of include/clwh.h, the owners of their device
// memory and events, and the helpers the runtime's files share (clwh_context.hip: contexts, memory objects, timing, transfer
// functions; clwh_render.hip; clwh_sdf.hip; clwh_launch.hip: clwh_kernel_get / clwh_launch; clwh_views.hip: projections, compositing, isosurfaces, slices, curved reformats, section profiles and overlays; clwh_mesh.hip: the
// isosurface mesh; clwh_grow.hip: region growing and masked volumes; clwh_label.hip: component labelling;
// clwh_distance.hip: distance maps of masks, ball morphology and mask algebra; clwh_geodesic.hip: geodesic maps and paths; clwh_costpath.hip: the same through a cost field; clwh_watershed.hip: the seeded watershed of a cost field; clwh_thin.hip: thinning and the list of a mask's voxels; clwh_filter.hip: the volume filters; clwh_region_stats.hip: statistics of masks and labels).
// No kernel needs this header.
#pragma once

#include <atomic>
#include <deque>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "clwh_internal.hpp"

namespace clvr {

// a failed HIP call: remembered for clwh_last_hip_error(), mapped to a status
void note_hip_error(hipError_t e);
inline int hip_failed(hipError_t e) {
  note_hip_error(e);
  return e == hipErrorOutOfMemory ? CLWH_ERR_OUT_OF_MEMORY : CLWH_ERR_HIP;
}
#define HIP_TRY(expr)                                   \
  do {                                                  \
    hipError_t _e = (expr);                             \
    if (_e != hipSuccess) return clvr::hip_failed(_e);  \
  } while (0)
// the same for a call that returns a status of its own
#define CLWH_TRY(expr)                \
  do {                                \
    int _rc = (expr);                 \
    if (_rc != CLWH_OK) return _rc;   \
  } while (0)

// ---- owners: what they hold goes with them
struct NoCopy {
  NoCopy() = default;
  NoCopy(const NoCopy &) = delete;
  NoCopy &operator=(const NoCopy &) = delete;
};

struct DeviceBuffer : NoCopy {
  void *ptr = nullptr;
  size_t bytes = 0;
  ~DeviceBuffer() { if (ptr) (void)hipFree(ptr); }
  template <class T>
  T *as() const { return static_cast<T *>(ptr); }
  void *release() {  // hands the allocation to the caller
    void *p = ptr;
    ptr = nullptr;
    bytes = 0;
    return p;
  }
  // nothing if large enough; else the stream's work on the old memory is waited for, the memory freed and `need` bytes
  // allocated (contents undefined).  *reallocated tells callers whose derived state lives in or depends on the allocation.
  int reserve(hipStream_t stream, size_t need, bool *reallocated = nullptr) {
    if (reallocated) *reallocated = bytes < need;
    if (bytes >= need) return CLWH_OK;
    if (ptr) {
      HIP_TRY(hipStreamSynchronize(stream));
      HIP_TRY(hipFree(ptr));
      (void)release();
    }
    HIP_TRY(hipMalloc(&ptr, need));
    bytes = need;
    return CLWH_OK;
  }
};

struct Event : NoCopy {
  hipEvent_t ev = nullptr;
  ~Event() { if (ev) (void)hipEventDestroy(ev); }
  int ensure(unsigned flags) {  // created on first use
    if (!ev) HIP_TRY(hipEventCreateWithFlags(&ev, flags));
    return CLWH_OK;
  }
};

struct PinnedWord : NoCopy {  // one page-locked 64-byte line the device copies a word into
  uint32_t *ptr = nullptr;
  ~PinnedWord() { if (ptr) (void)hipHostFree(ptr); }
  int ensure() {
    if (!ptr) HIP_TRY(hipHostMalloc((void **)&ptr, 64, hipHostMallocDefault));
    return CLWH_OK;
  }
};

// hiprtc fallback for TF source outside the rule grammar (tf_jit.cpp)
int tf_jit_compile(const char *user_source, std::vector<char> &code, std::string &log);
struct JitTf {
  std::string source;
  std::vector<char> code;
  hipModule_t module = nullptr;
  hipFunction_t classify = nullptr;
};

// ---- derived scene data (step bytes + hit records + per-brick minima + exit-certificate table + start-certificate table + hull-certificate table), ONE copy per device however many
// contexts (frame lanes, callers) render the same (volume content, SDF content, transfer function): contexts hold it by
// shared_ptr and find it in a process-wide registry (clwh_render.hip); the memory goes when the last context lets go of it.
struct PackedScene {
  int device = 0;
  DeviceBuffer data;
  const void *vol = nullptr, *sdf = nullptr;
  uint64_t vol_ver = 0, sdf_ver = 0;
  TfDev tf{};
  std::string tf_identity;   // opaque (hiprtc) transfer functions: the source text -- two sources may share a palette
  int32_t macro_shift = 0;
  bool start_table = false;  // the allocation ends with the start-certificate table (one byte per voxel)
  bool hull_table = false;   // ... followed by the hull-certificate table and its scratch
  int32_t dims[3] = {0, 0, 0};  // of the volume (the macro table's place in `data` follows from them)
  uint64_t generation = 0;   // process-wide unique id of this content (part of the primary-hit key)
  Event ready;               // recorded on the building stream after the last build kernel; adopters make their stream wait for it
  bool stale = false;        // clwh_ctx_invalidate_derived: nobody adopts it any more
  ~PackedScene();            // waits for the whole device before the members let go
};

// content version of a device allocation, shared by every clwh_mem that names the same device pointer (the owner and all
// wraps): a push, a rebuild or clwh_mem_mark_dirty through ANY of them is seen by all
struct VersionCell {
  std::atomic<uint64_t> v{0};
};

// ---- the members of a context, one per concern; each owns its buffers and the key that says what they hold

// CLWH_TUNE_*: read once, when the context is created (tuning_from_environment)
struct Tuning {
  // measured on MI355X (round 1, git history: profiles/r01_tune_*.txt): a wave that runs its 64 samples to completion with
  // steps and events in separate wave-wide phases beats mid-flight refills (12.5 vs 7.6 Gsamples/s)
  int32_t step_min_lanes = 0;    // 0: chosen per launch (launch_bounce)
  int32_t refill_min_lanes = 0;  // 0: chosen per launch (launch_bounce)
  int32_t macro_shift = 0;       // CLWH_TUNE_MACRO_SHIFT: 4..8 forces the macro cell's edge to 2^n voxels (0: by volume size)
  int32_t bounce_rays = 1;       // CLWH_TUNE_BOUNCE_RAYS=2: k_bounce2 for long launches
  int32_t force_long_launch = 0; // CLWH_TUNE_LONG_LAUNCH=1: every launch is scheduled like a long one (the parity tests use it)
  int32_t literal_gradient = 0;
  int32_t unit_block_log2 = 4;
  int32_t unit_group = 1, unit_affinity = 0, unit_queues = 8;
  int32_t unit_ahead = -1;     // CLWH_TUNE_UNIT_AHEAD=0/1: k_bounce's waves reserve their next unit a pass ahead: never / always (-1: launch_bounce decides -- never)
  int32_t cert_hint = 1;       // CLWH_TUNE_CERT_HINT=0: a refused march asks again at its next long step, whatever the refusing entry says
  int32_t start_cert = 1;      // CLWH_TUNE_START_CERT=0: no start-certificate table (a byte per voxel), first legs march from their first step
  int32_t hull_cert = 1;       // CLWH_TUNE_HULL_CERT=0: no hull-certificate table, no plane search in k_primary, no test in k_bounce
  int32_t hull_defer = 1;      // CLWH_TUNE_HULL_DEFER=0: hull certificates for first legs that start in front of their plane only
  int32_t hull_tilt = 1;       // CLWH_TUNE_HULL_TILT=0: no tilted planes, armed marches keep kHullDeferSteps
  int32_t cert_min_step = -1;  // CLWH_TUNE_CERT: 0 = exit certificates off; -1 = by volume size (12 at 512^3, 24 at 1024^3, 48 at 2048^3:
                               // the best of the sweeps in profiles/r02_sweep_k_bounce_lds_state.txt)
  uint32_t bounce_max_blocks = 2048;  // CLWH_TUNE_BLOCKS
  int32_t sdfbit_waves = 8;    // CLWH_TUNE_SDFBIT_WAVES: 8 or 16 waves per block of the bit-parallel build
  int32_t sdfbit_grid = 512;   // CLWH_TUNE_SDFBIT_GRID: its persistent grid
  int32_t sdfbit_rec_lds = 0;  // CLWH_TUNE_SDFBIT_REC=lds: the layer records in LDS, three blocks of eight waves per CU (grid x 3 / 2)
  int32_t sdf_front = 0;       // CLWH_TUNE_SDF=front: the byte-front build (one launch per layer) instead of the bit-parallel one
  int32_t dist_lines = 0;      // CLWH_TUNE_DIST_LINES=search: clwh_mask_distance's passes along y and z by the outward search (2) instead of the two linear scans (0, 1)
  int32_t label_stats = 0;     // CLWH_TUNE_LABEL_STATS=item: clwh_label_statistics' lanes hand their part on after every eight voxels (1); =direct: parts go
                               // to memory, not through the block's table (2).  Both lost; same bytes either way
  int32_t slice_coarse = 1;    // CLWH_TUNE_SLICE_COARSE=0: k_slice's skipping walk asks the bricks' table only, not the cells of 4^3 bricks
};
Tuning tuning_from_environment();

// per-camera primary hits (derived data, rebuilt when the key changes)
struct PrimaryHits {
  struct Key {
    float cam_pos[3], cam_dir[3];
    int32_t frame_w, frame_h, launch_w, launch_h, tile_rank, tile_world;
    int64_t cache_entries;
    int32_t mode, shading;
    uint64_t packed_generation;
    // miss pixels keep the environment colour of their camera ray: the env map's identity and content are part of the key
    const void *env;
    uint64_t env_version;
    int32_t env_w, env_h;
  } key{};
  bool valid = false;  // cleared by clwh_ctx_invalidate_derived (scene or camera)
  DeviceBuffer pix_slot, hits;
  DeviceBuffer hull_codes;    // a word per hit: its hull-certificate plane (k_primary), when the scene has the table
  DeviceBuffer hull_planes;   // a second word per hit: that plane with its signed margin (hull_defer)
  uint32_t n_hits = 0;
  bool n_hits_known = false;  // false: the count of this camera's hits is only on the device so far
  // the count travels to the host behind the camera's k_primary without anybody waiting for it: a 4-byte copy into page-locked
  // memory + an event; later launches of the same camera pick it up once the event has completed (hipEventQuery)
  PinnedWord host_n_hits;
  Event n_hits_event;
  bool n_hits_in_flight = false;
  uint32_t last_known_n_hits = 0;  // of any earlier camera of this context (0: none yet): sizes work buffers while the count is unknown
};

// work buffers of one pass
struct PassScratch {
  static constexpr size_t kCounters = CTR_QUEUE_STRIDE * 10;  // the first line, eight queue heads, and a line of statistics (CTR_HULL_DEFER, CTR_HULL_TILT)
  DeviceBuffer counters;      // kCounters x u32 on the device
  DeviceBuffer fixups, delta;
  DeviceBuffer sticky_flags;  // [0] fix-up buffer overflow: set by kernels, cleared only when the host has read it
  bool fixup_overflow_pending = false;
};

// planned voxel-cache launches: the camera's hits grouped by voxel (sorted once per camera), this launch's grants
struct VoxelPlan {
  DeviceBuffer plan;   // keys_in | keys_sorted (int64 each) | iota | order | grants (u32 each), n_capacity elements each
  DeviceBuffer temp;
  bool valid = false;  // cleared by a new camera (k_primary ran) and by a plan buffer that moved
  uint32_t n = 0;      // elements sorted (the hit count, or its bound when the plan was made)
};

// hiprtc-compiled transfer functions, by source text; and the class bytes of the current (volume, source)
struct TfClasses {
  std::map<std::string, std::shared_ptr<JitTf>> cache;
  DeviceBuffer cls;
  DeviceBuffer palette;  // CLWH_TF_MAX_RULES keys + 1 error word
  const void *vol = nullptr;  // nullptr: nothing valid
  uint64_t vol_ver = 0;
  std::string source;
  TfDev tf{};
};

struct SdfScratch {
  DeviceBuffer counters;  // 160 ints: settled voxels per layer
  DeviceBuffer flags;     // 4 x tiles bytes (current / next / being cleared / done)
  DeviceBuffer bits;      // bit-parallel build: event bits, two reached-set buffers, block states
#ifdef CLVR_SDFBIT_TIMING
  DeviceBuffer timing;    // tools/ builds only: per-phase sums of wall_clock64 ticks over all regions
#endif
};

// a tile worklist's scratch (tile_work_begin): per tile the round it is to be visited in and its place in the round's list, behind them
// the round counters and the caller's result; the copied seeds; and the pinned line the counters and the result travel to the host in
struct TileScratch {
  DeviceBuffer tiles, seeds;
  PinnedWord host;
};

// clwh_segment_grow's scratch: the admissible bit image (one bit per voxel in the mask's layout) and the worklist of its tiles of
// 64 x 16 x 16 voxels.  Every call rewrites what it reads, so nothing here outlives a call: only the allocations are kept, and they go
// with the context.
struct GrowScratch {
  DeviceBuffer admissible;
  TileScratch work;
};

// clwh_segment_label's scratch: the admissible bit image; the components' sort keys (in | out) and the sort's work space; the three
// counters and the pinned line two of them travel to the host in.  Every call rewrites what it reads: only the allocations are kept.
struct LabelScratch {
  DeviceBuffer admissible, keys, temp, counters;
  PinnedWord host;
};

// clwh_mask_distance's and clwh_mask_morph's scratch: two maps of 4 bytes per voxel (a pass along an axis reads one map and writes
// another: the distance call's are the caller's buffer and map_a, with the scans' stack in map_b; a morphology step's are map_a and
// map_b) and, for OPEN and CLOSE, the mask between the two steps.  Every call rewrites what it reads: only the allocations are kept.
struct DistanceScratch {
  DeviceBuffer map_a, map_b, bits;
};

// clwh_mask_geodesic's and clwh_geodesic_trace's scratch: the packed keys (8 bytes per voxel) and the worklist of their tiles of
// 16 x 16 x 8 voxels, whose pinned line the trace's result travels in too.  Every call rewrites what it reads: only the allocations
// are kept.  clwh_watershed reuses both: the keys' bytes as two uint32 arrays, the worklist with a second word per tile.
struct GeodesicScratch {
  DeviceBuffer keys, trace;  // trace: clwh_geodesic_trace's count and verdict
  TileScratch work;
};

// clwh_cost_from_field's scratch: the table on the device and the page-locked copy it travels from (the call does not wait, and the
// caller's table need not outlive it), 65536 entries each; `copied` is recorded behind the copy, and the next call waits for it -- not
// for the stream -- before it overwrites the page-locked copy.  clwh_cost_geodesic and clwh_cost_trace use the geodesic's scratch.
struct CostScratch {
  DeviceBuffer table;
  uint16_t *host = nullptr;
  Event copied;
  bool in_flight = false;
  ~CostScratch() { if (host) (void)hipHostFree(host); }
};

// clwh_render_curved's and clwh_curve_profile's scratch: the curve's rows on the device and the page-locked copy they travel from, under
// clwh_cost_from_field's discipline: `copied` is recorded behind the copy, and the next call waits for it -- not for the stream --
// before it overwrites the page-locked copy; the device buffer is rewritten in stream order.
struct CurveScratch {
  DeviceBuffer rows;
  float *host = nullptr;
  size_t host_bytes = 0;
  Event copied;
  bool in_flight = false;
  ~CurveScratch() { if (host) (void)hipHostFree(host); }
};

// clwh_mask_thin's scratch: the candidate bits C (one bit per voxel in the mask's layout) and the tiles' worklist, of which it uses the
// stamps, the list and the counters' line.  clwh_mask_points': the per-word counts and their scan, and the scan's work space.  Every call
// rewrites what it reads: only the allocations are kept.
struct ThinScratch {
  DeviceBuffer candidates, counts, temp;
  TileScratch work;
};

// clwh_volume_filter's scratch: at most two int16 copies of the volume, between the passes and for the in-place case.  Every call
// rewrites what it reads: only the allocations are kept.
struct FilterScratch {
  DeviceBuffer a, b;
};

// clwh_mask_statistics' scratch: the one record the blocks add to, with the histogram's two tails behind it (a clwh_mask_stats_result).
// Every call rewrites what it reads: only the allocation is kept.
struct RegionStatsScratch {
  DeviceBuffer result;
};

// clwh_overlay_slice's and clwh_overlay_camera's scratch: {ID, K} per pixel of the region and its one-pixel halo, and the occupancy words of
// the region's bricks and cells.  Every call rewrites what it reads: only the allocations are kept.
struct OverlayScratch {
  DeviceBuffer pixel_ids, occupancy;
};

// intensity projections and compositing: the volume in brick order + the per-brick {min, max} table (one allocation, per context,
// shared by clwh_render_projection and clwh_render_composite), and the key of the content it was built from (device pointer, shared
// content version, dims).  Beside it the derived data of compositing's colour/opacity table: the prefix count of entries with
// a > 0, keyed the same way (device pointer, shared content version, length).
struct ProjectionData {
  DeviceBuffer data;
  bool valid = false;  // cleared by clwh_ctx_invalidate_derived (projection)
  const void *vol = nullptr;
  uint64_t vol_ver = 0;
  size_t dims[3] = {0, 0, 0};
  // clwh_render_isosurface and clwh_render_slice (MAX / MIN without CLWH_SLICE_DENSE) only: the {min, max} table of the bricks dilated
  // by one voxel (and of the cells of 4^3 bricks behind it), built from `data` by the first such call after `data` was (re)built --
  // valid only while `valid` is and for the same key
  DeviceBuffer dilated;
  bool dilated_valid = false;  // cleared whenever `data` is rebuilt and by clwh_ctx_invalidate_derived (projection)
  // clwh_mesh_isosurface only: its scratch (per-brick counts and their scans, the scan's work space, the point table of the bricks with
  // a vertex).  Every call rewrites what it reads, so nothing here outlives a call: only the allocations are kept
  DeviceBuffer mesh_counts, mesh_temp, mesh_points;
  DeviceBuffer lut_prefix;
  bool lut_valid = false;  // cleared by clwh_ctx_invalidate_derived (projection)
  const void *lut = nullptr;
  uint64_t lut_ver = 0;
  int32_t lut_len = 0;
};

// timing: one HIP event pair per timed region, recorded on the context's stream and read back (without a sync per pass) by
// clwh_ctx_timing_read; pairs are created once and reused after every read
struct LaunchTimers {
  struct Pair {
    Event begin, end;
    int which = 0;  // enum clwh_timer
  };
  bool enabled = false;
  std::deque<Pair> pairs;  // (a deque: pairs are made in place and never move)
  size_t used = 0;
};

}  // namespace clvr

// ---- opaque handle layouts
struct clwh_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  clvr::Event handoff;  // clwh_ctx_acquire_from / clwh_ctx_release_to
  clvr::Tuning tune;
  clvr::PrimaryHits primary;
  clvr::PassScratch pass;
  clvr::VoxelPlan vox;
  clvr::TfClasses classes;
  clvr::SdfScratch sdf;
  clvr::GrowScratch grow;
  clvr::LabelScratch label;
  clvr::DistanceScratch distance;
  clvr::GeodesicScratch geodesic;
  clvr::CostScratch cost;
  clvr::CurveScratch curve;
  clvr::RegionStatsScratch region_stats;
  clvr::ThinScratch thin;
  clvr::FilterScratch filter;
  clvr::OverlayScratch overlay;
  clvr::ProjectionData proj;
  clvr::DeviceBuffer bilateral_weights;  // 13 x 17 tap weights of the bilateral volume filter (built on first use)
  // derived packed volume: hit records (8 B per voxel of the brick grid), the step bytes (1 B), the per-brick minima (4 B per
  // brick), the macro-cell table -- shared with every other context of the device that renders the same scene
  std::shared_ptr<clvr::PackedScene> scene;
  clvr::LaunchTimers timers;
};

struct clwh_mem {
  clwh_ctx *ctx = nullptr;
  void *dptr = nullptr;
  size_t bytes = 0;
  bool owned = false;
  bool is_image = false;
  size_t dims[3] = {1, 1, 1};
  int channels = 1;
  int elem_kind = CLWH_ELEM_U8;
  int flags = 0;
  std::shared_ptr<clvr::VersionCell> cell;  // shared with every other clwh_mem of the same device pointer
  uint64_t version() const { return cell ? cell->v.load(std::memory_order_relaxed) : 0; }
};

enum clwh_kernel_id {
  CLWH_K_EMPTY = 0,
  CLWH_K_RENDER,
  CLWH_K_SDF_BASE,
  CLWH_K_SDF_LAYER,
  CLWH_K_BUFFER_RESET,
  CLWH_K_FETCH_STATS,
  CLWH_K_APPLY_CLIP,
  CLWH_K_TF_SORT_VALUES,
  CLWH_K_TF_FLUSH_COLOR_FRAME,
  CLWH_K_BILATERAL_FILTER
};

struct clwh_kernel {
  clwh_ctx *ctx = nullptr;
  int id = CLWH_K_EMPTY;
  clwh_tf tf{};
  bool has_tf = false;
  std::shared_ptr<clvr::JitTf> jit;  // set when the source is outside the rule grammar
};

// a new content version for the object's device memory (seen through every clwh_mem that names the same pointer)
void clwh_touch(clwh_mem *m);

namespace clvr {

inline void touch(clwh_mem *m) { clwh_touch(m); }

// a render may have overflowed its fix-up buffer; read and reported at the next synchronisation point (clwh_context.hip)
int check_device_flags(clwh_ctx *ctx);

// ---- transfer functions (clwh_context.hip)
void tf_to_dev(const clwh_tf &tf, TfDev &d);
int jit_for_source(clwh_ctx *ctx, const char *source, std::shared_ptr<JitTf> &out);
// class byte per voxel + colour palette of an opaque TF for `volume`; cached per (volume content, source)
int ensure_classes(clwh_ctx *ctx, const std::shared_ptr<JitTf> &jit, const clwh_mem *volume, TfDev &tf_out, const uint8_t **cls_out);
// the table of a kernel's transfer function, whichever way it was compiled
inline int kernel_tf(clwh_kernel *k, const clwh_mem *volume, TfDev &tf_out, const uint8_t **cls_out) {
  if (k->jit) return ensure_classes(k->ctx, k->jit, volume, tf_out, cls_out);
  tf_to_dev(k->tf, tf_out);
  return CLWH_OK;
}

// ---- argument checks every entry point shares
inline bool is_image(const clwh_mem *m, int dims_n, int channels, int elem_kind) {
  if (!m || !m->is_image || m->channels != channels || m->elem_kind != elem_kind) return false;
  if (dims_n == 2) return m->dims[2] == 1;
  return true;
}
// an output of the mesher, a mask: a plain device buffer (clwh_mem_create / clwh_mem_wrap), not an image
inline bool is_plain_buffer(const clwh_mem *m) { return m && m->dptr && !m->is_image; }
inline bool same_dims(const clwh_mem *a, const clwh_mem *b) {
  return a->dims[0] == b->dims[0] && a->dims[1] == b->dims[1] && a->dims[2] == b->dims[2];
}
// a launch region is a whole number of 8x8 pixel tiles
inline bool launch_size_ok(uint32_t w, uint32_t h) { return w != 0 && h != 0 && (w % 8) == 0 && (h % 8) == 0; }
// kernels with one block row per (y, z): the grid's y and z extents are 16-bit
inline bool fits_grid_yz(const clwh_mem *m) { return m->dims[1] <= 65535 && m->dims[2] <= 65535; }
// kernels index voxels with int32 coordinates
inline bool dims_fit_int32(const clwh_mem *m) { return m->dims[0] <= 0x7fffffffu && m->dims[1] <= 0x7fffffffu && m->dims[2] <= 0x7fffffffu; }
inline void env_into_args(RenderArgs &a, const clwh_mem *env) {
  a.env = (const uint32_t *)env->dptr;
  a.env_w = (int32_t)env->dims[0];
  a.env_h = (int32_t)env->dims[1];
}
// -- the mask operations' (grow, label, distance, geodesic, region statistics)
// a mask handle the kernels can use: a plain device buffer whose rows are aligned 64-bit words
inline bool mask_ok(const clwh_mem *m) { return is_plain_buffer(m) && ((uintptr_t)m->dptr & 7u) == 0u; }
// a buffer of 32-bit words: labels, distances, path points
inline bool words_ok(const clwh_mem *m) { return is_plain_buffer(m) && ((uintptr_t)m->dptr & 3u) == 0u; }
// the S16 volume the kernels read or write: an image with memory and no empty axis
inline bool volume_ok(const clwh_mem *m) {
  return is_image(m, 3, 1, CLWH_ELEM_S16) && m->dptr && m->dims[0] != 0 && m->dims[1] != 0 && m->dims[2] != 0;
}
// voxels are numbered in 31 bits: no dim zero, each below 2^31, X * Y * Z <= 2^31 - 1 (by division: the product may not fit)
inline bool voxels_fit_31_bits(uint64_t X, uint64_t Y, uint64_t Z) {
  if (X == 0 || Y == 0 || Z == 0 || X > 0x7FFFFFFFu || Y > 0x7FFFFFFFu || Z > 0x7FFFFFFFu) return false;
  return X * Y <= 0x7FFFFFFFull && Z <= 0x7FFFFFFFull / (X * Y);
}
// 64-bit words per row of a mask; whether the buffer holds the whole mask (dims below 2^31 each; compared by division: the product
// may not fit)
inline size_t mask_w64(uint64_t X) { return (size_t)((X + 63u) / 64u); }
inline bool mask_fits(uint64_t X, uint64_t Y, uint64_t Z, const clwh_mem *mask) { return mask->bytes / (mask_w64(X) * 8u) >= Y * Z; }
// grow's and label's admissible set: the value window lo <= hi within int16, and the box in voxels, box_hi all zero = the whole
// volume, lo <= hi <= dim on every axis.  False: CLWH_ERR_INVALID_VALUE.  `empty`: nothing is admissible
struct ResolvedBox {
  uint64_t lo[3], hi[3];
  bool empty;
};
inline bool resolve_window_and_box(int32_t lo, int32_t hi, const uint32_t *box_lo, const uint32_t *box_hi, const clwh_mem *vol, ResolvedBox &b) {
  if (!(lo >= -32768 && lo <= hi && hi <= 32767)) return false;
  const bool whole = (box_hi[0] | box_hi[1] | box_hi[2]) == 0u;
  for (int q = 0; q < 3; ++q) {
    b.lo[q] = box_lo[q];
    b.hi[q] = whole ? (uint64_t)vol->dims[q] : (uint64_t)box_hi[q];
    if (!(b.lo[q] <= b.hi[q] && b.hi[q] <= (uint64_t)vol->dims[q])) return false;
  }
  b.empty = b.lo[0] == b.hi[0] || b.lo[1] == b.hi[1] || b.lo[2] == b.hi[2];
  return true;
}
// ... and their answer when nothing is admissible: the output all zero, written when the call returns
inline int clear_and_wait(clwh_ctx *ctx, void *out, size_t bytes) {
  HIP_TRY(hipMemsetAsync(out, 0, bytes, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return CLWH_OK;
}

// ---- the tile worklist on the host (TileWork; the protocol is in tile_work_device.hpp).  The caller has set w's TX, TY, TZ and dense.
// One allocation: stamps | list | counters | result, the counters on a 64-byte line of their own and `result_bytes` for the caller
// behind them (*result); the seeds' copy and the pinned line beside it.  The stamps are cleared.
inline int tile_work_begin(clwh_ctx *ctx, TileScratch &g, TileWork &w, size_t seed_bytes, size_t result_bytes, void **result) {
  const size_t tile_words = ((size_t)w.TX * (size_t)w.TY * (size_t)w.TZ + 15u) & ~(size_t)15u;
  CLWH_TRY(g.tiles.reserve(ctx->stream, (2u * tile_words + 2u * (size_t)kGrowBatch) * sizeof(uint32_t) + result_bytes));
  CLWH_TRY(g.seeds.reserve(ctx->stream, seed_bytes > 16u ? seed_bytes : 16u));
  CLWH_TRY(g.host.ensure());
  w.stamps = g.tiles.as<uint32_t>();
  w.list = w.stamps + tile_words;
  w.counters = w.list + tile_words;
  *result = w.counters + 2 * kGrowBatch;
  HIP_TRY(hipMemsetAsync(w.stamps, 0, tile_words * sizeof(uint32_t), ctx->stream));
  return CLWH_OK;
}
// Rounds until one lists no tile, eight to a batch: the pinned line holds eight {listed, ticket} pairs, and a batch that turns out to
// be longer than the search costs its empty rounds one word read per block.  `enqueue_round(round, slot)` returns a hipError_t.
// *rounds: the rounds that listed a tile; once they reach `cap` (the caller's bound, which only keeps a defect from spinning) the
// answer is CLWH_ERR_INTERNAL_OVERFLOW.
template <class F>
int tile_work_run(clwh_ctx *ctx, TileScratch &g, const TileWork &w, uint64_t cap, F &&enqueue_round, uint64_t *rounds) {
  *rounds = 0;
  for (uint32_t round = 1;; round += (uint32_t)kGrowBatch) {
    HIP_TRY(hipMemsetAsync(w.counters, 0, 2u * (size_t)kGrowBatch * sizeof(uint32_t), ctx->stream));
    for (int slot = 0; slot < kGrowBatch; ++slot) HIP_TRY(enqueue_round(round + (uint32_t)slot, slot));
    HIP_TRY(hipMemcpyAsync(g.host.ptr, w.counters, 2u * (size_t)kGrowBatch * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int slot = 0; slot < kGrowBatch; ++slot) *rounds += g.host.ptr[2 * slot] != 0u;
    if (g.host.ptr[2 * (kGrowBatch - 1)] == 0u) return CLWH_OK;  // the batch's last round listed nothing: converged
    if (*rounds >= cap) return CLWH_ERR_INTERNAL_OVERFLOW;
  }
}

// ---- the derived data the views and the mesher share (clwh_views.hip): the bricked copy of `volume` and its {min, max} table, which
// also sets v's dims and grids; then, for the callers that may skip by them, the dilated and cell tables
int ensure_projection_data(clwh_ctx *ctx, const clwh_mem *volume, ViewVolume &v);
int ensure_dilated_table(clwh_ctx *ctx, ViewVolume &v);

// ---- a timed region: `launches` (a callable returning hipError_t) between a (begin, end) event pair of timer `which`;
// with timing off it is `launches` and nothing else -- no event is created or recorded
int timed_begin(clwh_ctx *ctx, int which, hipEvent_t *end);
template <class F>
int timed(clwh_ctx *ctx, int which, F &&launches) {
  hipEvent_t end = nullptr;
  CLWH_TRY(timed_begin(ctx, which, &end));
  HIP_TRY(launches());
  if (end) HIP_TRY(hipEventRecord(end, ctx->stream));
  return CLWH_OK;
}

}  // namespace clvr
