// clwh_render.hip -- clwh_render on the host: the registry of derived scene data, the camera's primary hits, one pass;
// and the entry points that resolve an image-space accumulation.  The kernels: {scene,primary,render,accumulate}_kernels.hip.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>

#include "clwh_host.hpp"

using namespace clvr;

// ------------------------------------------------------------------------------------------------
// the per-device registry of derived scene data (PackedScene, clwh_host.hpp)

static std::mutex g_scenes_mutex;  // contexts may live on different host threads
static std::vector<std::weak_ptr<PackedScene>> g_packed_scenes;
static std::atomic<uint64_t> g_packed_generation{0};

PackedScene::~PackedScene() {
  // the last context let go; another context that dropped its reference earlier may still have kernels in flight on its
  // own stream that read this memory
  (void)hipSetDevice(device);
  (void)hipDeviceSynchronize();
}

// layout of a PackedScene's allocation
struct PackedLayout {
  int X, Y, Z, NBX, NBY, NBZ, mshift, MNX, MNY, MNZ;
  size_t records, n_bricks, off_stepb, off_brick_min, off_macro, off_start, off_hull_ends, off_hull, off_hull_h, bytes;
  bool start_table;  // the start-certificate table is part of the allocation
  bool hull_table;   // ... and behind it the hull-certificate table with its scratch (the rows' first and last event voxels) and, last, its h_k alone
};
// Start certificates (k_start_*, scene_kernels.hip) are built for tables the step byte decides alone (no rule reads `gradient`), under
// which the border texel is no event (the other exit certificates are off there too), for volumes whose table fits the budget (and the
// build's grids), unless CLWH_TUNE_START_CERT=0.
static bool wants_start_table(const Tuning &t, const TfDev &tf, const clwh_mem *volume) {
  return t.start_cert != 0 && tf.uses_gradient == 0 && tf.border_class == 0 && fits_grid_yz(volume) &&
         (uint64_t)volume->dims[0] * volume->dims[1] * volume->dims[2] <= kStartTableBudget;
}
// Hull certificates (k_hull_*) are built where start certificates are (the same proof obligations), for volumes of at most
// kHullMaxDim voxels along every axis, unless CLWH_TUNE_HULL_CERT=0.
static bool wants_hull_table(const Tuning &t, const TfDev &tf, const clwh_mem *volume) {
  return t.hull_cert != 0 && wants_start_table(t, tf, volume) && volume->dims[0] <= (size_t)kHullMaxDim && volume->dims[1] <= (size_t)kHullMaxDim &&
         volume->dims[2] <= (size_t)kHullMaxDim;
}
// tilted planes: the tilt's target and gain as bind_scene hands them to k_bounce
static void hull_tilt_target(float delta, float &target, float &gain) {
  const double t = std::min((double)delta + (double)kHullTiltMargin, 0.984375);  // (delta = 2, none qualifies: any target will do)
  target = (float)t;
  gain = (float)(t / std::sqrt(1.0 - t * t));
}

static PackedLayout packed_layout(const clwh_mem *volume, int forced_macro_shift, bool start_table, bool hull_table) {
  PackedLayout L;
  L.X = (int)volume->dims[0]; L.Y = (int)volume->dims[1]; L.Z = (int)volume->dims[2];
  L.NBX = (L.X + 7) / 8; L.NBY = (L.Y + 7) / 8; L.NBZ = (L.Z + 7) / 8;
  L.records = (size_t)L.NBX * L.NBY * L.NBZ * 512u;
  L.n_bricks = (size_t)L.NBX * L.NBY * L.NBZ;
  L.mshift = macro_cell_shift(L.X, L.Y, L.Z, forced_macro_shift);  // macro cells of the exit certificates
  const int mcell = 1 << L.mshift;
  L.MNX = (L.X + mcell - 1) >> L.mshift; L.MNY = (L.Y + mcell - 1) >> L.mshift; L.MNZ = (L.Z + mcell - 1) >> L.mshift;
  // hit records, the per-step bytes, the per-brick minima (u32, 16-byte aligned), the macro-cell table
  L.off_stepb = L.records * sizeof(uint2);
  L.off_brick_min = (L.records * (sizeof(uint2) + 1u) + 15u) & ~(size_t)15u;
  L.off_macro = (L.off_brick_min + L.n_bricks * sizeof(uint32_t) + 15u) & ~(size_t)15u;
  L.off_start = (L.off_macro + (size_t)L.MNX * L.MNY * L.MNZ * 8u + 15u) & ~(size_t)15u;  // eight octant entries per cell
  // the start-certificate table: 16 bytes for the `regular` word, then one byte per voxel, x fastest
  L.start_table = start_table;
  L.off_hull_ends = (L.off_start + (start_table ? 16u + (size_t)L.X * L.Y * L.Z : 0u) + 15u) & ~(size_t)15u;
  L.hull_table = hull_table;
  L.off_hull = L.off_hull_ends + (hull_table ? (size_t)L.Y * L.Z * sizeof(int2) : 0u);  // (a multiple of 8; float4 loads need 16)
  L.off_hull = (L.off_hull + 15u) & ~(size_t)15u;
  L.off_hull_h = L.off_hull + (size_t)kHullPlanes * sizeof(float4);
  L.bytes = hull_table ? L.off_hull_h + (size_t)kHullPlanes * sizeof(float) : L.off_start + (start_table ? 16u + (size_t)L.X * L.Y * L.Z : 0u);
  return L;
}

static bool packed_matches(const PackedScene &p, int device, const PackedLayout &L, const clwh_mem *volume, const clwh_mem *sdf,
                           const TfDev &tf, const std::string &tf_identity) {
  return !p.stale && p.device == device && p.data.bytes == L.bytes && p.macro_shift == L.mshift && p.start_table == L.start_table && p.hull_table == L.hull_table && p.vol == volume->dptr &&
         p.sdf == sdf->dptr && p.vol_ver == volume->version() && p.sdf_ver == sdf->version() &&
         !std::memcmp(&p.tf, &tf, sizeof tf) && p.tf_identity == tf_identity;
}

// the bricked step bytes + hit records (packed_volume.hpp) of (volume, SDF, TF), laid out as L: the context's own entry if it
// still matches, else the entry another context of this device has built (its stream's work is ordered behind the build by an
// event), else built here on the context's stream
static int ensure_packed(clwh_ctx *ctx, const PackedLayout &L, const clwh_mem *volume, const clwh_mem *sdf, const TfDev &tf,
                         const uint8_t *cls_in, const std::string &tf_identity) {
  if (ctx->scene && packed_matches(*ctx->scene, ctx->device, L, volume, sdf, tf, tf_identity)) return CLWH_OK;
  std::shared_ptr<PackedScene> entry;
  {
    std::lock_guard<std::mutex> lock(g_scenes_mutex);
    for (auto it = g_packed_scenes.begin(); it != g_packed_scenes.end();) {
      std::shared_ptr<PackedScene> live = it->lock();
      if (!live) { it = g_packed_scenes.erase(it); continue; }
      if (!entry && packed_matches(*live, ctx->device, L, volume, sdf, tf, tf_identity)) entry = live;
      ++it;
    }
  }
  if (entry) {
    ctx->scene.reset();  // (frees the old entry if this context was its last holder)
    HIP_TRY(hipStreamWaitEvent(ctx->stream, entry->ready.ev, 0));
    ctx->scene = entry;
    return CLWH_OK;
  }
  // build.  A context that is the only holder of an entry of the right size rebuilds in place (a transfer-function flush
  // does not free and allocate 9 bytes per voxel); the stream orders the rebuild behind the kernels that still read it.
  if (ctx->scene && ctx->scene.use_count() == 1 && ctx->scene->data.bytes == L.bytes) {
    entry = ctx->scene;
  } else {
    ctx->scene.reset();
    entry = std::make_shared<PackedScene>();
    entry->device = ctx->device;
    CLWH_TRY(entry->data.reserve(ctx->stream, L.bytes));
    CLWH_TRY(entry->ready.ensure(hipEventDisableTiming));
  }
  ctx->scene.reset();
  {
    std::lock_guard<std::mutex> lock(g_scenes_mutex);
    entry->stale = true;  // not adoptable until described below
  }
  uint8_t *data = entry->data.as<uint8_t>();
  RepackArgs r;
  std::memset(&r, 0, sizeof r);
  r.volume = (const int16_t *)volume->dptr;
  r.sdf = (const int8_t *)sdf->dptr;
  r.X = L.X; r.Y = L.Y; r.Z = L.Z;
  r.NBX = L.NBX; r.NBY = L.NBY; r.NBZ = L.NBZ;
  r.grec = reinterpret_cast<uint2 *>(data);
  r.stepb = data + L.off_stepb;
  r.brick_min = reinterpret_cast<uint32_t *>(data + L.off_brick_min);
  HIP_TRY(hipMemsetAsync(r.brick_min, 0xFF, L.n_bricks * sizeof(uint32_t), ctx->stream));
  r.cls_in = cls_in;
  r.tf = tf;
  CLWH_TRY(timed(ctx, CLWH_TIMER_REPACK, [&] {
    const hipError_t e = launch_repack(r, ctx->stream);
    if (e != hipSuccess) return e;
    return launch_macro_table(r.brick_min, L.NBX, L.NBY, L.NBZ, data + L.off_macro, L.X, L.Y, L.Z, L.mshift, ctx->stream);
  }));
  if (L.start_table)
    CLWH_TRY(timed(ctx, CLWH_TIMER_REPACK, [&] {
      int2 *ends = L.hull_table ? reinterpret_cast<int2 *>(data + L.off_hull_ends) : nullptr;
      const hipError_t e = launch_start_table(r.stepb, data + L.off_start + 16u, reinterpret_cast<uint32_t *>(data + L.off_start), ends, L.X, L.Y, L.Z, L.NBX, L.NBY, L.NBZ, ctx->stream);
      if (e != hipSuccess || !L.hull_table) return e;
      return launch_hull_table(ends, reinterpret_cast<const uint32_t *>(data + L.off_start), reinterpret_cast<float4 *>(data + L.off_hull), reinterpret_cast<float *>(data + L.off_hull_h), L.X, L.Y, L.Z, ctx->stream);
    }));
  HIP_TRY(hipEventRecord(entry->ready.ev, ctx->stream));
  ctx->scene = entry;
  {
    std::lock_guard<std::mutex> lock(g_scenes_mutex);
    entry->vol = volume->dptr;
    entry->sdf = sdf->dptr;
    entry->vol_ver = volume->version();
    entry->sdf_ver = sdf->version();
    entry->tf = tf;
    entry->tf_identity = tf_identity;
    entry->macro_shift = L.mshift;
    entry->start_table = L.start_table;
    entry->hull_table = L.hull_table;
    entry->dims[0] = L.X; entry->dims[1] = L.Y; entry->dims[2] = L.Z;
    entry->generation = ++g_packed_generation;
    entry->stale = false;
    bool listed = false;
    for (auto &w : g_packed_scenes)
      if (w.lock() == entry) listed = true;
    if (!listed) g_packed_scenes.push_back(entry);
  }
  return CLWH_OK;
}

// ------------------------------------------------------------------------------------------------
// clwh_render, stage by stage

// fill the parts of RenderArgs that describe the frame / tile partition / camera
static void describe_frame(RenderArgs &a, int32_t launch_w, int32_t launch_h, int32_t frame_w, int32_t frame_h,
                           int32_t rank, int32_t world, const float cam_pos[3], const float cam_dir[3]) {
  a.launch_w = launch_w;
  a.launch_h = launch_h;
  a.frame_w = frame_w;
  a.frame_h = frame_h;
  a.tiles_x = launch_w / 8;
  a.tiles_y = launch_h / 8;
  a.tile_rank = rank;
  a.tile_world = world;
  a.tiles_per_row = (a.tiles_x + world - 1) / world;
  a.num_tile_slots = (uint32_t)a.tiles_y * (uint32_t)a.tiles_per_row;
  for (int q = 0; q < 3; ++q) {
    a.cam_pos[q] = cam_pos[q];
    a.cam_dir[q] = cam_dir[q];
  }
}

static size_t pixel_slots(const RenderArgs &a) { return (size_t)a.num_tile_slots * 64u; }
static size_t launch_pixels(const RenderArgs &a) { return (size_t)a.launch_w * (size_t)a.launch_h; }
// a voxel-cache launch of several seeds: its tokens are dealt out before it runs (plan_voxel_grants)
static bool is_planned(const RenderArgs &a) { return a.mode == CLWH_ACCUM_VOXEL_CACHE && a.n_seeds > 1; }

// stage 1: what can be refused by looking at the descriptor alone
static int validate_desc(const clwh_render_desc *d) {
  if (!is_image(d->volume, 3, 1, CLWH_ELEM_S16) || !is_image(d->sdf, 3, 1, CLWH_ELEM_S8) ||
      !is_image(d->env, 2, 4, CLWH_ELEM_U8))
    return CLWH_ERR_BAD_ARGS;
  if (d->frame && !is_image(d->frame, 2, 4, CLWH_ELEM_U8)) return CLWH_ERR_BAD_ARGS;
  if (!same_dims(d->volume, d->sdf)) return CLWH_ERR_SIZE_MISMATCH;
  if (!launch_size_ok(d->width, d->height)) return CLWH_ERR_BAD_NDRANGE;
  if (d->width > 65535u || d->height > 65535u) return CLWH_ERR_BAD_NDRANGE;  // pixel ids are packed x | y << 16
  if (d->env->dims[0] > 32768u || d->env->dims[1] > 32768u) return CLWH_ERR_INVALID_VALUE;  // env_fast.hpp bracket
  if (!dims_fit_int32(d->volume)) return CLWH_ERR_INVALID_VALUE;
  const int world = d->tile_world < 1 ? 1 : d->tile_world;
  if (d->tile_rank < 0 || d->tile_rank >= world) return CLWH_ERR_INVALID_VALUE;
  if (d->n_seeds < 0 || d->n_seeds > CLWH_MAX_SEEDS) return CLWH_ERR_INVALID_VALUE;
  if (d->n_seeds > 1 && d->contrib) return CLWH_ERR_BAD_ARGS;  // per-pixel contribution output: one seed
  if (d->shading != CLWH_SHADE_LIGHT && d->shading != CLWH_SHADE_AO) return CLWH_ERR_INVALID_VALUE;
  if (d->shading == CLWH_SHADE_AO && d->accum_mode != CLWH_ACCUM_VOXEL_CACHE) return CLWH_ERR_BAD_ARGS;  // compute_ao lives in buffer_volume
  return CLWH_OK;
}

// stage 2: frame, camera, accumulation target, optional outputs, seeds and the scheduling knobs into the arguments
static int describe_launch(const clwh_ctx *ctx, const clwh_render_desc *d, RenderArgs &a) {
  std::memset(&a, 0, sizeof a);
  a.X = (int32_t)d->volume->dims[0];
  a.Y = (int32_t)d->volume->dims[1];
  a.Z = (int32_t)d->volume->dims[2];
  env_into_args(a, d->env);
  // get_image_width/height(frame): the frame IMAGE's dims (the reference allocates 2048x1024 whatever
  // the launch size); without a frame, the launch size
  const int32_t fw = d->frame ? (int32_t)d->frame->dims[0] : (int32_t)d->width;
  const int32_t fh = d->frame ? (int32_t)d->frame->dims[1] : (int32_t)d->height;
  const int world = d->tile_world < 1 ? 1 : d->tile_world;
  describe_frame(a, (int32_t)d->width, (int32_t)d->height, fw, fh, d->tile_rank, world, d->cam_pos, d->cam_dir);
  a.frame = d->frame ? (uint32_t *)d->frame->dptr : nullptr;
  a.mode = d->accum_mode;
  a.shading = d->shading;
  if (a.mode == CLWH_ACCUM_VOXEL_CACHE) {
    if (!d->buffer_volume || d->buffer_volume->bytes < 8) return CLWH_ERR_BAD_ARGS;
    a.cache = (uint32_t *)d->buffer_volume->dptr;
    // compute_light: 4 ushorts per voxel (utility.cl:21); compute_ao: 2 ushorts per voxel (utility.cl:127)
    a.cache_entries = (int64_t)(d->buffer_volume->bytes / (d->shading == CLWH_SHADE_AO ? 4 : 8));
  } else if (a.mode == CLWH_ACCUM_IMAGE_SPACE) {
    const int64_t need = clwh_accum_len(d->width, d->height, world) * 16;
    if (!d->accum || (int64_t)d->accum->bytes < need) return CLWH_ERR_BAD_ARGS;
    a.accum = (float4 *)d->accum->dptr;
  } else {
    return CLWH_ERR_INVALID_VALUE;
  }
  if (d->hit_index) {
    if (d->hit_index->bytes < launch_pixels(a) * 8) return CLWH_ERR_SIZE_MISMATCH;
    a.hit_index_out = (int64_t *)d->hit_index->dptr;
  }
  if (d->contrib) {
    if (d->contrib->bytes < launch_pixels(a) * 16) return CLWH_ERR_SIZE_MISMATCH;
    a.contrib_out = (uint32_t *)d->contrib->dptr;
  }
  if (d->n_seeds > 0) {
    a.n_seeds = d->n_seeds;
    for (int q = 0; q < d->n_seeds; ++q) a.seeds[q] = d->seeds[q];
  } else {
    a.n_seeds = 1;
    a.seeds[0] = d->seed;
  }
  const Tuning &t = ctx->tune;
  a.step_min_lanes = t.step_min_lanes;
  a.refill_min_lanes = t.refill_min_lanes;
  a.force_long_launch = t.force_long_launch;
  a.bounce_rays = t.bounce_rays;
  a.bounce_max_blocks = t.bounce_max_blocks;
  a.unit_group = t.unit_group;
  a.unit_block_log2 = t.unit_block_log2;
  a.unit_affinity = t.unit_affinity;
  a.unit_queues = t.unit_queues;
  a.unit_ahead = t.unit_ahead;
  a.cert_hint = t.cert_hint;
  a.start_cert_dmin = start_cert_dmin(a.X, a.Y, a.Z);
  a.hull_delta0 = hull_cert_delta0(a.X, a.Y, a.Z);
  a.hull_defer_delta0 = hull_defer_delta0(a.X, a.Y, a.Z);
  return CLWH_OK;
}

// stage 3: the transfer function's table and the derived scene data of (volume, SDF, table)
static int bind_scene(clwh_kernel *k, const clwh_render_desc *d, RenderArgs &a) {
  clwh_ctx *ctx = k->ctx;
  const uint8_t *cls_in = nullptr;
  CLWH_TRY(kernel_tf(k, d->volume, a.tf, &cls_in));
  a.tf.literal_gradient_taps = ctx->tune.literal_gradient;
  const PackedLayout L = packed_layout(d->volume, ctx->tune.macro_shift, wants_start_table(ctx->tune, a.tf, d->volume), wants_hull_table(ctx->tune, a.tf, d->volume));
  CLWH_TRY(ensure_packed(ctx, L, d->volume, d->sdf, a.tf, cls_in, k->jit ? k->jit->source : std::string()));
  const uint8_t *packed = ctx->scene->data.as<uint8_t>();
  a.grec = reinterpret_cast<const uint2 *>(packed);
  a.NBX = L.NBX;
  a.NBY = L.NBY;
  a.stepb = packed + L.off_stepb;
  a.volume_lin = (const int16_t *)d->volume->dptr;
  a.sdf_lin = (const int8_t *)d->sdf->dptr;
  a.macro = packed + L.off_macro;
  a.start_free = L.start_table ? packed + L.off_start + 16u : nullptr;
  a.hull = L.hull_table ? reinterpret_cast<const float4 *>(packed + L.off_hull) : nullptr;
  // tilted planes ride on item 13's armed counter and its layout of the lane's word: no hull_planes, no tilt
  a.hull_h = L.hull_table && ctx->tune.hull_defer != 0 && ctx->tune.hull_tilt != 0 ? reinterpret_cast<const float *>(packed + L.off_hull_h) : nullptr;
  if (a.hull_h) {
    a.hull_defer_delta0 = hull_defer_delta0(a.X, a.Y, a.Z, kHullTiltSteps);  // k_bounce's one J for every armed march
    hull_tilt_target(a.hull_defer_delta0, a.hull_tilt_target, a.hull_tilt_gain);
  }
  a.macro_shift = L.mshift;
  a.MNX = L.MNX; a.MNY = L.MNY; a.MNZ = L.MNZ;
  // An exit certificate proves "this march leaves the volume without a Hit"; a position with a coordinate == dimension or NaN
  // reads the border texel (value 0), so tables under which value 0 can be an event keep marching literally.
  bool zero_may_hit = a.tf.border_class != 0;
  for (int q = 0; q < a.tf.n && a.tf.uses_gradient && !a.tf.opaque; ++q)
    if (a.tf.rules[q].v_lo <= 0 && 0 <= a.tf.rules[q].v_hi) zero_may_hit = true;
  const int cert_auto = a.macro_shift < 4 ? 12 >> (4 - a.macro_shift) : std::min(12 << (a.macro_shift - 4), 48);  // re-swept in round 3 with the stronger certificates: 8 / 12 / 16 -> 3.69 / 3.59 / 3.6-3.9 ms
  a.cert_min_step = zero_may_hit ? 0 : (ctx->tune.cert_min_step >= 0 ? ctx->tune.cert_min_step : cert_auto);
  return CLWH_OK;
}

// stage 4: primary hits of this camera, rebuilt only when something they depend on changed
static int ensure_primary_hits(clwh_ctx *ctx, const clwh_render_desc *d, RenderArgs &a) {
  PrimaryHits &p = ctx->primary;
  PassScratch &s = ctx->pass;
  const size_t slots = pixel_slots(a);
  CLWH_TRY(p.pix_slot.reserve(ctx->stream, slots * sizeof(uint32_t)));
  CLWH_TRY(p.hits.reserve(ctx->stream, slots * sizeof(HitRec)));
  if (a.hull) CLWH_TRY(p.hull_codes.reserve(ctx->stream, slots * sizeof(uint32_t)));
  const bool defer = a.hull && ctx->tune.hull_defer != 0;
  if (defer) CLWH_TRY(p.hull_planes.reserve(ctx->stream, slots * sizeof(uint32_t)));
  CLWH_TRY(s.counters.reserve(ctx->stream, PassScratch::kCounters * sizeof(uint32_t)));
  bool fresh_flags = false;
  CLWH_TRY(s.sticky_flags.reserve(ctx->stream, 64, &fresh_flags));
  if (fresh_flags) HIP_TRY(hipMemsetAsync(s.sticky_flags.ptr, 0, 64, ctx->stream));
  a.sticky_flags = s.sticky_flags.as<uint32_t>();
  a.pix_slot = p.pix_slot.as<uint32_t>();
  a.hits = p.hits.as<HitRec>();
  a.hull_codes = a.hull ? p.hull_codes.as<uint32_t>() : nullptr;
  a.hull_planes = defer ? p.hull_planes.as<uint32_t>() : nullptr;
  a.counters = s.counters.as<uint32_t>();

  PrimaryHits::Key key;
  std::memset(&key, 0, sizeof key);
  for (int q = 0; q < 3; ++q) {
    key.cam_pos[q] = a.cam_pos[q];
    key.cam_dir[q] = a.cam_dir[q];
  }
  key.frame_w = a.frame_w; key.frame_h = a.frame_h;
  key.launch_w = a.launch_w; key.launch_h = a.launch_h;
  key.tile_rank = a.tile_rank; key.tile_world = a.tile_world;
  key.cache_entries = a.cache_entries;
  key.mode = a.mode;
  key.shading = a.shading;
  key.packed_generation = ctx->scene->generation;
  key.env = d->env->dptr;
  key.env_version = d->env->version();
  key.env_w = a.env_w; key.env_h = a.env_h;
  if (p.valid && std::memcmp(&key, &p.key, sizeof key) == 0 && !a.hit_index_out) return CLWH_OK;
  p.valid = false;
  HIP_TRY(hipMemsetAsync(a.counters, 0, PassScratch::kCounters * sizeof(uint32_t), ctx->stream));
  CLWH_TRY(timed(ctx, CLWH_TIMER_PRIMARY, [&] { return launch_primary(a, ctx->stream); }));
  // the camera's hit count follows on the stream into page-locked memory; nobody waits for it
  CLWH_TRY(p.host_n_hits.ensure());
  CLWH_TRY(p.n_hits_event.ensure(hipEventDisableTiming));
  HIP_TRY(hipMemcpyAsync(p.host_n_hits.ptr, a.counters + CTR_HITS, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipEventRecord(p.n_hits_event.ev, ctx->stream));
  p.n_hits_in_flight = true;
  ctx->vox.valid = false;
  p.n_hits_known = false;
  p.key = key;
  p.valid = true;
  return CLWH_OK;
}

// stage 5: the hit count, or what stands in for it.
// No host round trip per camera (the reference's queue is one in-order queue without a readback between camera and pass,
// app/renderer.cpp:145-150).  The kernels read the hit count from counters[CTR_HITS] themselves; the host only needs a bound of it
// for grid and buffer sizes, and uses the real count as soon as the copy above has arrived by itself.
static int pick_up_hit_count(clwh_ctx *ctx, RenderArgs &a) {
  PrimaryHits &p = ctx->primary;
  if (p.n_hits_in_flight && !p.n_hits_known) {
    if (hipEventQuery(p.n_hits_event.ev) == hipSuccess) {
      p.n_hits = *p.host_n_hits.ptr;
      p.n_hits_known = true;
      p.n_hits_in_flight = false;
      p.last_known_n_hits = p.n_hits;
    } else {
      (void)hipGetLastError();  // hipErrorNotReady is an answer, not a failure: keep it out of the launches' error checks
    }
  }
  const size_t slots = pixel_slots(a);
  a.n_hits_on_device = !p.n_hits_known;
  a.n_hits = p.n_hits_known ? p.n_hits : (uint32_t)std::min<size_t>(slots, 0xFFFFFFFFu);  // else: upper bound
  // what the count is LIKELY to be, for the scheduling class of the launch and the size of the fix-up buffer: the count itself, else
  // twice the last camera's (a camera move rarely doubles the hit pixels), never below a quarter of the pixels
  a.n_hits_estimate = a.n_hits;
  if (!p.n_hits_known && p.last_known_n_hits != 0)
    a.n_hits_estimate = (uint32_t)std::min<uint64_t>(a.n_hits, std::max<uint64_t>(2ull * p.last_known_n_hits, slots / 4u));
  if (!bounce_queues_fit(a.n_hits, ctx->tune.unit_block_log2, a.n_seeds)) return CLWH_ERR_INVALID_VALUE;
  return CLWH_OK;
}

// stage 6a: the pass's work buffers
static int size_pass_buffers(clwh_ctx *ctx, RenderArgs &a) {
  PassScratch &s = ctx->pass;
  // fix-up records for environment lookups the fast path cannot certify.  Expected rate: 4e-6 x (0.16 w + 0.32 h) per lookup, at
  // most two lookups per item (0.5 % at 4096x2048, 4 % at the 32768 limit); room for three times that, never less than 1/64 of the
  // items -- of the ESTIMATED item count while the camera's hit count is still on its way (an overflow is reported, not silent)
  const double rate = std::min(1.0, std::max(1.0 / 64.0, 3.0 * 8.0e-6 * (0.16 * a.env_w + 0.32 * a.env_h)));
  const size_t fix_cap = std::max<size_t>((size_t)((double)a.n_hits_estimate * (double)a.n_seeds * rate), 4096u);
  CLWH_TRY(s.fixups.reserve(ctx->stream, fix_cap * 128u));
  a.fixups = s.fixups.as<uint32_t>();
  a.fixup_capacity = (uint32_t)std::min<size_t>(s.fixups.bytes / 128u, 0x7fffffffu);
  if (a.mode == CLWH_ACCUM_IMAGE_SPACE || is_planned(a)) {
    // one 64-bit delta per hit; k_commit folds a launch's deltas into the accumulator and leaves them zero for the next launch
    bool fresh = false;
    CLWH_TRY(s.delta.reserve(ctx->stream, std::max<size_t>(pixel_slots(a), 1) * sizeof(unsigned long long), &fresh));
    a.delta = s.delta.as<unsigned long long>();
    if (fresh) HIP_TRY(hipMemsetAsync(s.delta.ptr, 0, s.delta.bytes, ctx->stream));
  }
  return CLWH_OK;
}

// stage 6b: a voxel-cache launch of several seeds deals its tokens out beforehand (accumulate_kernels.hip "planned voxel-cache
// launches"); one seed per launch -- the reference's call pattern, and the per-pixel contribution output of the parity tests --
// keeps the reference's token-per-sample protocol
static int plan_voxel_grants(clwh_ctx *ctx, RenderArgs &a) {
  if (!is_planned(a)) return CLWH_OK;
  VoxelPlan &v = ctx->vox;
  // keys_in | keys_sorted (int64) | iota | order | grants (u32), `cap` elements each; sorted once per camera
  constexpr size_t kPerElement = 2 * sizeof(int64_t) + 3 * sizeof(uint32_t);
  bool moved = false;
  CLWH_TRY(v.plan.reserve(ctx->stream, pixel_slots(a) * kPerElement, &moved));
  if (moved) v.valid = false;
  const size_t have = v.plan.bytes / kPerElement;
  int64_t *keys_in = v.plan.as<int64_t>(), *keys = keys_in + have;
  uint32_t *iota = reinterpret_cast<uint32_t *>(keys + have), *order = iota + have, *grants = order + have;
  if (!v.valid) {
    const uint32_t n = a.n_hits;  // the count, or its bound (then the tail sorts behind every real hit)
    HIP_TRY(launch_vox_keys(a, keys_in, iota, n, ctx->stream));
    size_t need = 0;
    HIP_TRY(sort_entry_pairs(nullptr, need, keys_in, keys, iota, order, n, 39u, ctx->stream));
    CLWH_TRY(v.temp.reserve(ctx->stream, std::max<size_t>(need, 16)));
    size_t tb = v.temp.bytes;
    HIP_TRY(sort_entry_pairs(v.temp.ptr, tb, keys_in, keys, iota, order, n, 39u, ctx->stream));
    v.valid = true;
    v.n = n;
  }
  HIP_TRY(launch_vox_grant(a, keys, order, v.n, grants, ctx->stream));
  a.grants = grants;
  return CLWH_OK;
}

#ifdef CLVR_BOUNCE_STATS  // experiment builds only (CLVR_EXTRA_HIPCC_FLAGS=-DCLVR_BOUNCE_STATS): scheduling statistics of the launch
static int print_bounce_stats(clwh_ctx *ctx, const RenderArgs &a) {
  uint32_t h[CTR_HULL_TILT_END];
  HIP_TRY(hipMemcpyAsync(h, a.counters, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  auto per = [&](int sum, int n) { return h[n] ? (double)h[sum] / h[n] : 0.0; };
  std::fprintf(stderr, "[bounce stats] items=%llu step_iters=%u avg_march_lanes=%.2f event_phases=%u avg_event_lanes=%.2f "
               "refills=%u avg_refill=%.2f events start/exit/hit/none=%u/%u/%u/%u cert_phases=%u avg_cert_lanes=%.2f cert_granted=%u\n",
               (unsigned long long)h[CTR_HITS] * (unsigned long long)a.n_seeds, h[CTR_STEP_ITERS], per(CTR_STEP_LANES, CTR_STEP_ITERS),
               h[CTR_EVENT_PHASES], per(CTR_EVENT_LANES, CTR_EVENT_PHASES), h[CTR_REFILLS], per(CTR_REFILL_LANES, CTR_REFILLS), h[CTR_EV_KIND],
               h[CTR_EV_KIND + 1], h[CTR_EV_KIND + 2], h[CTR_EV_KIND + 3], h[CTR_CERT_PHASES], per(CTR_CERT_LANES, CTR_CERT_PHASES), h[CTR_CERT_GRANTED]);
  if (h[CTR_SWAPS]) std::fprintf(stderr, "[bounce stats] two rays per lane: %u swap points\n", h[CTR_SWAPS]);
  std::fprintf(stderr, "[bounce stats] per step iteration: avg_idle_lanes=%.2f (lane sum %u)\n", per(CTR_STEP_IDLE, CTR_STEP_ITERS), h[CTR_STEP_IDLE]);
  // -DCLVR_BOUNCE_STATS=2 takes the start certificates as the product build does; any other value marches a granted leg all the same and checks it
  std::fprintf(stderr, "[bounce stats] lane_steps=%u event_lanes=%u start certificates (%s) tried/granted/wrong=%u/%u/%u dmin=%.6f\n", h[CTR_STEP_LANES],
               h[CTR_EVENT_LANES], (CLVR_BOUNCE_STATS + 0) == 2 ? "taken" : "verified: marched literally", h[CTR_START_TRIED], h[CTR_START_GRANTED],
               h[CTR_START_WRONG], (double)a.start_cert_dmin);
  std::fprintf(stderr, "[bounce stats] hull certificates tried/granted/wrong=%u/%u/%u, of the granted the octant proof grants %u; either proof grants %u first legs; delta0=%.6f\n",
               h[CTR_HULL_TRIED], h[CTR_HULL_GRANTED], h[CTR_HULL_WRONG], h[CTR_HULL_BOTH], h[CTR_START_GRANTED] + h[CTR_HULL_GRANTED] - h[CTR_HULL_BOTH],
               (double)a.hull_delta0);
  const uint32_t *m = h + CTR_HULL_DEFER;
  std::fprintf(stderr, "[bounce stats] hull certificates tried/granted/wrong: first legs deferred=%u/%u/%u rebounds at once=%u/%u/%u rebounds deferred=%u/%u/%u; "
               "J=%d D=%.4g defer_delta0=%.6f; look-ups=%u\n", m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], m[8], a.hull_h ? kHullTiltSteps : kHullDeferSteps, (double)kHullDeferDeficit,
               (double)a.hull_defer_delta0, h[CTR_CERT_LANES] - ((CLVR_BOUNCE_STATS + 0) == 2 ? m[1] + m[7] + h[CTR_HULL_TILT + 4] + h[CTR_HULL_TILT + 10] : 0u) - h[CTR_HULL_TILT + 12]);
  const uint32_t *t = h + CTR_HULL_TILT;
  std::fprintf(stderr, "[bounce stats] tilted planes (%s) tried/granted/wrong: first legs at once=%u/%u/%u first legs deferred=%u/%u/%u rebounds at once=%u/%u/%u "
               "rebounds deferred=%u/%u/%u; armed lanes that got there late and were sent back without a look-up=%u; target=%.6f\n", a.hull_h ? "on" : "off", t[0], t[1], t[2], t[3], t[4], t[5],
               t[6], t[7], t[8], t[9], t[10], t[11], t[12], (double)a.hull_tilt_target);
  return CLWH_OK;
}
#endif

// stage 6c: the pass -- every (hit, seed) item
static int run_pass(clwh_ctx *ctx, const RenderArgs &a) {
  CLWH_TRY(timed(ctx, CLWH_TIMER_BOUNCE, [&] { return launch_bounce(a, ctx->stream); }));
#ifdef CLVR_BOUNCE_STATS
  CLWH_TRY(print_bounce_stats(ctx, a));
#endif
  CLWH_TRY(timed(ctx, CLWH_TIMER_FIXUP, [&] {
    hipError_t e = launch_env_fixup(a, ctx->stream);
    if (e == hipSuccess) e = launch_commit(a, ctx->stream);
    if (e == hipSuccess && is_planned(a)) e = launch_commit_voxel(a, ctx->stream);
    return e;
  }));
  ctx->pass.fixup_overflow_pending = true;
  return CLWH_OK;
}

extern "C" {

int64_t clwh_cache_len(uint32_t X, uint32_t Y, uint32_t Z) {
  return ((int64_t)X * Z * Y + (int64_t)X * Z + X + 1) * 4;
}

int64_t clwh_accum_len(uint32_t width, uint32_t height, int32_t tile_world) {
  if (tile_world < 1) tile_world = 1;
  const int64_t tiles_x = width / 8, tiles_y = height / 8;
  const int64_t tiles_per_row = (tiles_x + tile_world - 1) / tile_world;
  return tiles_y * tiles_per_row * 64;
}

int clwh_render(clwh_kernel *k, const clwh_render_desc *d) {
  if (!k || !d || k->id != CLWH_K_RENDER || !k->has_tf) return CLWH_ERR_INVALID_VALUE;
  clwh_ctx *ctx = k->ctx;
  RenderArgs a;
  CLWH_TRY(validate_desc(d));
  CLWH_TRY(describe_launch(ctx, d, a));
  HIP_TRY(hipSetDevice(ctx->device));
  CLWH_TRY(bind_scene(k, d, a));
  CLWH_TRY(ensure_primary_hits(ctx, d, a));
  CLWH_TRY(pick_up_hit_count(ctx, a));

  HIP_TRY(hipMemsetAsync(a.counters + CTR_HITS + 1, 0, (PassScratch::kCounters - CTR_HITS - 1) * sizeof(uint32_t), ctx->stream));
  if (a.contrib_out) HIP_TRY(hipMemsetAsync(a.contrib_out, 0, launch_pixels(a) * 16, ctx->stream));  // misses contribute nothing

  if (d->resolve_only) {
    if (!a.frame) return CLWH_ERR_BAD_ARGS;
  } else if (d->shading == CLWH_SHADE_AO) {
    // ambient occlusion (compute_ao, ray_marching.cl:104-149): one lane per hit, its passes one after the other
    CLWH_TRY(timed(ctx, CLWH_TIMER_AO, [&] { return launch_ao(a, ctx->stream); }));
  } else {
    CLWH_TRY(size_pass_buffers(ctx, a));
    CLWH_TRY(plan_voxel_grants(ctx, a));
    CLWH_TRY(run_pass(ctx, a));
  }
  if ((d->write_frame || d->resolve_only) && a.frame)
    CLWH_TRY(timed(ctx, CLWH_TIMER_RESOLVE, [&] { return launch_resolve(a, ctx->stream); }));
  if (d->frame) touch(d->frame);
  return CLWH_OK;
}

// ---- image-space accumulation: the ranks' tiles into a frame

int clwh_accum_resolve(clwh_ctx *ctx, clwh_mem *accum_all, int32_t tile_world, uint32_t width, uint32_t height,
                       clwh_mem *frame, clwh_mem *env, const float cam_pos[3], const float cam_dir[3]) {
  if (!ctx || !accum_all || !frame || !env || !cam_pos || !cam_dir || tile_world < 1) return CLWH_ERR_INVALID_VALUE;
  if (!is_image(frame, 2, 4, CLWH_ELEM_U8) || !is_image(env, 2, 4, CLWH_ELEM_U8)) return CLWH_ERR_BAD_ARGS;
  if (!launch_size_ok(width, height)) return CLWH_ERR_BAD_NDRANGE;
  const int64_t need = clwh_accum_len(width, height, tile_world) * 16 * tile_world;
  if ((int64_t)accum_all->bytes < need) return CLWH_ERR_SIZE_MISMATCH;
  RenderArgs a;
  std::memset(&a, 0, sizeof a);
  describe_frame(a, (int32_t)width, (int32_t)height, (int32_t)frame->dims[0], (int32_t)frame->dims[1], 0, tile_world,
                 cam_pos, cam_dir);
  a.frame = (uint32_t *)frame->dptr;
  env_into_args(a, env);
  HIP_TRY(hipSetDevice(ctx->device));
  CLWH_TRY(timed(ctx, CLWH_TIMER_RESOLVE, [&] { return launch_accum_resolve(a, (const float4 *)accum_all->dptr, ctx->stream); }));
  touch(frame);
  return CLWH_OK;
}

int clwh_accum_resolve_tiles(clwh_ctx *ctx, clwh_mem *accum, int32_t tile_rank, int32_t tile_world, uint32_t width, uint32_t height,
                             clwh_mem *tiles_rgba8, clwh_mem *env, const float cam_pos[3], const float cam_dir[3]) {
  if (!ctx || !accum || !tiles_rgba8 || !env || !cam_pos || !cam_dir || tile_world < 1 || tile_rank < 0 || tile_rank >= tile_world)
    return CLWH_ERR_INVALID_VALUE;
  if (!is_image(env, 2, 4, CLWH_ELEM_U8)) return CLWH_ERR_BAD_ARGS;
  if (!launch_size_ok(width, height)) return CLWH_ERR_BAD_NDRANGE;
  const int64_t n = clwh_accum_len(width, height, tile_world);
  if ((int64_t)accum->bytes < n * 16 || (int64_t)tiles_rgba8->bytes < n * 4) return CLWH_ERR_SIZE_MISMATCH;
  RenderArgs a;
  std::memset(&a, 0, sizeof a);
  describe_frame(a, (int32_t)width, (int32_t)height, (int32_t)width, (int32_t)height, tile_rank, tile_world, cam_pos, cam_dir);
  env_into_args(a, env);
  HIP_TRY(hipSetDevice(ctx->device));
  CLWH_TRY(timed(ctx, CLWH_TIMER_RESOLVE, [&] {
    return launch_accum_resolve_tiles(a, (const float4 *)accum->dptr, (uint32_t *)tiles_rgba8->dptr, ctx->stream);
  }));
  touch(tiles_rgba8);
  return CLWH_OK;
}

int clwh_frame_from_tiles(clwh_ctx *ctx, clwh_mem *tiles_all, int32_t tile_world, uint32_t width, uint32_t height, clwh_mem *frame) {
  if (!ctx || !tiles_all || !frame || tile_world < 1) return CLWH_ERR_INVALID_VALUE;
  if (!is_image(frame, 2, 4, CLWH_ELEM_U8)) return CLWH_ERR_BAD_ARGS;
  if (!launch_size_ok(width, height)) return CLWH_ERR_BAD_NDRANGE;
  if ((int64_t)tiles_all->bytes < clwh_accum_len(width, height, tile_world) * 4 * tile_world) return CLWH_ERR_SIZE_MISMATCH;
  const float zero[3] = {0.0f, 0.0f, 0.0f};
  RenderArgs a;
  std::memset(&a, 0, sizeof a);
  describe_frame(a, (int32_t)width, (int32_t)height, (int32_t)frame->dims[0], (int32_t)frame->dims[1], 0, tile_world, zero, zero);
  a.frame = (uint32_t *)frame->dptr;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(launch_frame_from_tiles(a, (const uint32_t *)tiles_all->dptr, ctx->stream));
  touch(frame);
  return CLWH_OK;
}

// ---- what a caller may know about the derived data

int clwh_ctx_invalidate_derived(clwh_ctx *ctx, int what) {
  if (!ctx) return CLWH_ERR_INVALID_VALUE;
  if ((what & CLWH_DERIVED_SCENE) && ctx->scene) {
    // this context rebuilds at its next render and nobody adopts the old copy any more; contexts that already share it keep it
    // until their own key changes (memory rewritten behind the shim's back is what clwh_mem_mark_dirty is for: every alias sees it)
    {
      std::lock_guard<std::mutex> lock(g_scenes_mutex);
      ctx->scene->stale = true;
    }
    if (ctx->scene.use_count() > 1) ctx->scene.reset();  // the only holder keeps the allocation and rebuilds in place
  }
  if (what & (CLWH_DERIVED_SCENE | CLWH_DERIVED_CAMERA)) ctx->primary.valid = false;
  if (what & CLWH_DERIVED_PROJECTION) ctx->proj.valid = ctx->proj.lut_valid = ctx->proj.dilated_valid = false;
  return CLWH_OK;
}

int clwh_ctx_scene_info(clwh_ctx *ctx, uint64_t *scene_id, uint64_t *bytes, int32_t *holders) {
  if (!ctx) return CLWH_ERR_INVALID_VALUE;
  std::lock_guard<std::mutex> lock(g_scenes_mutex);
  if (scene_id) *scene_id = ctx->scene ? ctx->scene->generation : 0;
  if (bytes) *bytes = ctx->scene ? ctx->scene->data.bytes : 0;
  if (holders) *holders = ctx->scene ? (int32_t)ctx->scene.use_count() : 0;
  return CLWH_OK;
}

int clwh_debug_device_probe(clwh_ctx *ctx, int32_t which, clwh_mem *in, uint64_t n, clwh_mem *out, clwh_mem *aux, const int32_t params[4]) {
  if (!ctx || !in || !out || !params) return CLWH_ERR_INVALID_VALUE;
  const ProbeShape shape = probe_shape(which);
  if (shape.in_words == 0u) return CLWH_ERR_INVALID_VALUE;
  const bool env = which == CLWH_PROBE_ENV_EXACT || which == CLWH_PROBE_ENV_FAST;
  if (env && (!aux || params[0] < 1 || params[1] < 1)) return CLWH_ERR_INVALID_VALUE;
  if (n >= (1ull << 31) || in->bytes < n * shape.in_words * 4u || out->bytes < n * shape.out_words * 4u) return CLWH_ERR_SIZE_MISMATCH;
  // the samplers clamp the texel they choose to [0, w) x [0, h): the image must hold that many words
  if (env && aux->bytes < (uint64_t)params[0] * (uint64_t)params[1] * 4u) return CLWH_ERR_SIZE_MISMATCH;
  if (n == 0) return CLWH_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(launch_device_probe(which, (const uint32_t *)in->dptr, n, (uint32_t *)out->dptr, env ? (const uint32_t *)aux->dptr : nullptr, params, ctx->stream));
  return CLWH_OK;
}

// the layout of the context's derived scene data
static PackedLayout scene_layout(clwh_ctx *ctx) {
  std::lock_guard<std::mutex> lock(g_scenes_mutex);
  clwh_mem shape{};
  for (int q = 0; q < 3; ++q) shape.dims[q] = (size_t)ctx->scene->dims[q];
  return packed_layout(&shape, ctx->scene->macro_shift, ctx->scene->start_table, ctx->scene->hull_table);
}

int clwh_debug_macro_table(clwh_ctx *ctx, void *host_out, uint64_t capacity, int32_t info_out[4]) {
  if (!ctx || !info_out) return CLWH_ERR_INVALID_VALUE;
  if (!ctx->scene) return CLWH_ERR_BAD_ARGS;  // nothing rendered yet (or the derived data was dropped)
  const PackedLayout L = scene_layout(ctx);
  info_out[0] = L.MNX; info_out[1] = L.MNY; info_out[2] = L.MNZ; info_out[3] = L.mshift;
  const size_t bytes = (size_t)L.MNX * L.MNY * L.MNZ * 8u;
  if (!host_out) return CLWH_OK;  // the size alone
  if (capacity < bytes || ctx->scene->data.bytes != L.bytes) return CLWH_ERR_SIZE_MISMATCH;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMemcpyAsync(host_out, ctx->scene->data.as<uint8_t>() + L.off_macro, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return CLWH_OK;
}

int clwh_debug_packed_scene(clwh_ctx *ctx, int32_t which, void *host_out, uint64_t capacity, int32_t info_out[4]) {
  if (!ctx || !info_out) return CLWH_ERR_INVALID_VALUE;
  if (which != CLWH_SCENE_HIT_RECORDS && which != CLWH_SCENE_STEP_BYTES && which != CLWH_SCENE_BRICK_MIN) return CLWH_ERR_INVALID_VALUE;
  if (!ctx->scene) return CLWH_ERR_BAD_ARGS;  // nothing rendered yet (or the derived data was dropped)
  const PackedLayout L = scene_layout(ctx);
  info_out[0] = L.NBX; info_out[1] = L.NBY; info_out[2] = L.NBZ; info_out[3] = 0;
  if (!host_out) return CLWH_OK;  // the size alone
  const size_t offset = which == CLWH_SCENE_HIT_RECORDS ? 0u : (which == CLWH_SCENE_STEP_BYTES ? L.off_stepb : L.off_brick_min);
  const size_t bytes = which == CLWH_SCENE_HIT_RECORDS ? L.records * sizeof(uint2) : (which == CLWH_SCENE_STEP_BYTES ? L.records : L.n_bricks * sizeof(uint32_t));
  if (capacity < bytes || ctx->scene->data.bytes != L.bytes) return CLWH_ERR_SIZE_MISMATCH;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMemcpyAsync(host_out, ctx->scene->data.as<uint8_t>() + offset, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return CLWH_OK;
}

int clwh_debug_view_data(clwh_ctx *ctx, int32_t which, void *host_out, uint64_t capacity, int32_t info_out[4]) {
  if (!ctx || !info_out) return CLWH_ERR_INVALID_VALUE;
  if (which != CLWH_VIEW_BRICKS && which != CLWH_VIEW_TABLE && which != CLWH_VIEW_DILATED && which != CLWH_VIEW_COARSE) return CLWH_ERR_INVALID_VALUE;
  const ProjectionData &p = ctx->proj;
  if (!p.valid) return CLWH_ERR_BAD_ARGS;  // no view rendered yet (or the derived data was dropped)
  const size_t NBX = (p.dims[0] + 7) / 8, NBY = (p.dims[1] + 7) / 8, NBZ = (p.dims[2] + 7) / 8;
  const size_t n_bricks = NBX * NBY * NBZ, n_cells = ((NBX + 3) / 4) * ((NBY + 3) / 4) * ((NBZ + 3) / 4);
  info_out[0] = (int32_t)NBX; info_out[1] = (int32_t)NBY; info_out[2] = (int32_t)NBZ; info_out[3] = (int32_t)n_cells;
  const bool second_level = which == CLWH_VIEW_DILATED || which == CLWH_VIEW_COARSE;
  // the bricked copy alone (ensure_projection_data): the dilated and the coarse table do not exist, whatever the buffer holds
  if (second_level && !p.dilated_valid) return CLWH_ERR_BAD_ARGS;
  if (!host_out) return CLWH_OK;  // the size alone
  const size_t off_table = n_bricks * 512u * sizeof(int16_t);
  const DeviceBuffer &from = second_level ? p.dilated : p.data;
  const size_t offset = which == CLWH_VIEW_TABLE ? off_table : (which == CLWH_VIEW_COARSE ? n_bricks * sizeof(uint32_t) : 0u);
  const size_t bytes = which == CLWH_VIEW_BRICKS ? off_table : (which == CLWH_VIEW_COARSE ? n_cells : n_bricks) * sizeof(uint32_t);
  if (capacity < bytes || from.bytes < offset + bytes) return CLWH_ERR_SIZE_MISMATCH;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMemcpyAsync(host_out, from.as<uint8_t>() + offset, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return CLWH_OK;
}

int clwh_debug_start_table(clwh_ctx *ctx, void *host_out, uint64_t capacity, int32_t info_out[4]) {
  if (!ctx || !info_out) return CLWH_ERR_INVALID_VALUE;
  if (!ctx->scene) return CLWH_ERR_BAD_ARGS;  // nothing rendered yet (or the derived data was dropped)
  const PackedLayout L = scene_layout(ctx);
  info_out[0] = L.X; info_out[1] = L.Y; info_out[2] = L.Z; info_out[3] = L.start_table ? 1 : 0;
  if (!host_out || !L.start_table) return CLWH_OK;  // the size alone; or there is no table
  const size_t bytes = (size_t)L.X * L.Y * L.Z;
  if (capacity < bytes || ctx->scene->data.bytes != L.bytes) return CLWH_ERR_SIZE_MISMATCH;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMemcpyAsync(host_out, ctx->scene->data.as<uint8_t>() + L.off_start + 16u, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return CLWH_OK;
}

int clwh_debug_start_cert_dmin(int32_t X, int32_t Y, int32_t Z, float *dmin_out) {
  if (!dmin_out || X < 1 || Y < 1 || Z < 1) return CLWH_ERR_INVALID_VALUE;
  *dmin_out = start_cert_dmin(X, Y, Z);
  return CLWH_OK;
}

int clwh_debug_hull_table(clwh_ctx *ctx, void *host_out, uint64_t capacity, int32_t info_out[4]) {
  if (!ctx || !info_out) return CLWH_ERR_INVALID_VALUE;
  if (!ctx->scene) return CLWH_ERR_BAD_ARGS;  // nothing rendered yet (or the derived data was dropped)
  const PackedLayout L = scene_layout(ctx);
  info_out[0] = kHullGrid; info_out[1] = kHullPlanes; info_out[2] = 0; info_out[3] = L.hull_table ? 1 : 0;
  if (!host_out || !L.hull_table) return CLWH_OK;  // the size alone; or there is no table
  const size_t bytes = (size_t)kHullPlanes * sizeof(float4);
  if (capacity < bytes || ctx->scene->data.bytes != L.bytes) return CLWH_ERR_SIZE_MISMATCH;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMemcpyAsync(host_out, ctx->scene->data.as<uint8_t>() + L.off_hull, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return CLWH_OK;
}

int clwh_debug_hull_cert_bound(int32_t X, int32_t Y, int32_t Z, float out[2]) {
  if (!out || X < 1 || Y < 1 || Z < 1) return CLWH_ERR_INVALID_VALUE;
  out[0] = hull_cert_delta0(X, Y, Z);
  out[1] = kHullSlack;
  return CLWH_OK;
}

int clwh_debug_hull_defer_bound(int32_t X, int32_t Y, int32_t Z, float out[4]) {
  if (!out || X < 1 || Y < 1 || Z < 1) return CLWH_ERR_INVALID_VALUE;
  out[0] = hull_defer_delta0(X, Y, Z);
  out[1] = (float)kHullDeferSteps;
  out[2] = kHullDeferDeficit;
  out[3] = (float)kHullMarginScale;
  return CLWH_OK;
}

int clwh_debug_hull_tilt_bound(int32_t X, int32_t Y, int32_t Z, float out[6]) {
  if (!out || X < 1 || Y < 1 || Z < 1) return CLWH_ERR_INVALID_VALUE;
  out[0] = hull_defer_delta0(X, Y, Z, kHullTiltSteps);
  out[1] = (float)kHullTiltSteps;
  out[2] = (float)kHullTiltPath;
  out[3] = kHullTiltMargin;
  hull_tilt_target(out[0], out[4], out[5]);
  return CLWH_OK;
}

int clwh_debug_hull_h(clwh_ctx *ctx, void *host_out, uint64_t capacity, int32_t info_out[4]) {
  if (!ctx || !info_out) return CLWH_ERR_INVALID_VALUE;
  if (!ctx->scene) return CLWH_ERR_BAD_ARGS;  // nothing rendered yet (or the derived data was dropped)
  const PackedLayout L = scene_layout(ctx);
  info_out[0] = kHullGrid; info_out[1] = kHullPlanes; info_out[2] = 0; info_out[3] = L.hull_table ? 1 : 0;
  if (!host_out || !L.hull_table) return CLWH_OK;  // the size alone; or there is no table
  const size_t bytes = (size_t)kHullPlanes * sizeof(float);
  if (capacity < bytes || ctx->scene->data.bytes != L.bytes) return CLWH_ERR_SIZE_MISMATCH;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMemcpyAsync(host_out, ctx->scene->data.as<uint8_t>() + L.off_hull_h, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return CLWH_OK;
}

int clwh_debug_hull_planes(clwh_ctx *ctx, void *host_out, uint64_t capacity, uint32_t *n_hits_out) {
  if (!ctx || !n_hits_out) return CLWH_ERR_INVALID_VALUE;
  PrimaryHits &p = ctx->primary;
  if (!p.valid || !p.hits.ptr || !ctx->pass.counters.ptr) return CLWH_ERR_BAD_ARGS;  // no camera rendered yet
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMemcpyAsync(n_hits_out, ctx->pass.counters.as<uint32_t>() + CTR_HITS, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (!host_out) return CLWH_OK;  // the count alone
  const bool built = ctx->scene && ctx->scene->hull_table && ctx->tune.hull_defer != 0 && p.hull_planes.ptr;
  const size_t bytes = (size_t)*n_hits_out * sizeof(uint32_t);
  if (capacity < bytes || (built && p.hull_planes.bytes < bytes)) return CLWH_ERR_SIZE_MISMATCH;
  if (!built) { std::memset(host_out, 0, bytes); return CLWH_OK;}  // no table, or CLWH_TUNE_HULL_DEFER=0: no hit has the word
  HIP_TRY(hipMemcpyAsync(host_out, p.hull_planes.ptr, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return CLWH_OK;
}

int clwh_debug_hull_codes(clwh_ctx *ctx, void *host_out, uint64_t capacity, uint32_t *n_hits_out) {
  if (!ctx || !n_hits_out) return CLWH_ERR_INVALID_VALUE;
  PrimaryHits &p = ctx->primary;
  if (!p.valid || !p.hits.ptr || !ctx->pass.counters.ptr) return CLWH_ERR_BAD_ARGS;  // no camera rendered yet
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMemcpyAsync(n_hits_out, ctx->pass.counters.as<uint32_t>() + CTR_HITS, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (!host_out) return CLWH_OK;  // the count alone
  const bool built = ctx->scene && ctx->scene->hull_table && p.hull_codes.ptr;
  const size_t bytes = (size_t)*n_hits_out * sizeof(uint32_t);
  if (capacity < bytes || (built && p.hull_codes.bytes < bytes)) return CLWH_ERR_SIZE_MISMATCH;
  if (!built) { std::memset(host_out, 0, bytes); return CLWH_OK; }  // no table: no hit has a plane
  HIP_TRY(hipMemcpyAsync(host_out, p.hull_codes.ptr, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return CLWH_OK;
}

int clwh_debug_hit_records(clwh_ctx *ctx, void *host_out, uint64_t capacity, uint32_t *n_hits_out) {
  if (!ctx || !n_hits_out) return CLWH_ERR_INVALID_VALUE;
  PrimaryHits &p = ctx->primary;
  if (!p.valid || !p.hits.ptr || !ctx->pass.counters.ptr) return CLWH_ERR_BAD_ARGS;  // no camera rendered yet
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMemcpyAsync(n_hits_out, ctx->pass.counters.as<uint32_t>() + CTR_HITS, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (!host_out) return CLWH_OK;  // the count alone
  const size_t bytes = (size_t)*n_hits_out * sizeof(HitRec);
  if (capacity < bytes || p.hits.bytes < bytes) return CLWH_ERR_SIZE_MISMATCH;
  HIP_TRY(hipMemcpyAsync(host_out, p.hits.ptr, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return CLWH_OK;
}

}  // extern "C"
