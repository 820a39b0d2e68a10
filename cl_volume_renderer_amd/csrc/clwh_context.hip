// clwh_context.hip -- host side of libclwhip.so: the C ABI declared in include/clwh.h.
//
// Replaces the reference's opencl_wrapper (clw_context / clw_vector / clw_image / clw_function)
// with a thin layer over the HIP runtime: one in-order stream per context, hipMalloc'ed objects,
// a registry of precompiled gfx950 kernels keyed by the reference's (file, entry) names, and the
// transfer-function source parsed into a launch-time table instead of being JIT-compiled.
//
// This file: contexts, memory objects, timing, transfer-function tables, diagnostics (the other files: clwh_host.hpp).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>

#include "clwh_host.hpp"

using namespace clvr;

static thread_local int g_last_hip_error = 0;
void clvr::note_hip_error(hipError_t e) { g_last_hip_error = (int)e; }

// Content versions are drawn from one process-wide counter, so (device pointer, version) identifies a
// content uniquely even when an object is released and another one is allocated at the same address.
// The version lives in a cell shared by every clwh_mem of the same device pointer (the owner and its wraps in
// other contexts): whoever rewrites the memory -- a push, clwh_sdf_build, clwh_mem_mark_dirty -- is seen by all of
// them, so no context keeps rendering from derived data of the old content.
static std::atomic<uint64_t> g_content_version{0};
static std::mutex g_cells_mutex;  // contexts may live on different host threads
static std::map<const void *, std::weak_ptr<VersionCell>> g_version_cells;
void clwh_touch(clwh_mem *m) { m->cell->v.store(++g_content_version, std::memory_order_relaxed); }

static std::shared_ptr<VersionCell> version_cell_of(const void *dptr) {
  std::lock_guard<std::mutex> lock(g_cells_mutex);
  auto it = g_version_cells.find(dptr);
  if (it != g_version_cells.end())
    if (auto live = it->second.lock()) return live;
  auto cell = std::make_shared<VersionCell>();
  g_version_cells[dptr] = cell;
  if (g_version_cells.size() > 4096) {  // forget the cells nobody holds any more
    for (auto i = g_version_cells.begin(); i != g_version_cells.end();)
      i = i->second.expired() ? g_version_cells.erase(i) : std::next(i);
  }
  return cell;
}

static size_t elem_size(int kind) {
  switch (kind) {
    case CLWH_ELEM_S8: case CLWH_ELEM_U8: return 1;
    case CLWH_ELEM_S16: case CLWH_ELEM_U16: return 2;
    case CLWH_ELEM_S32: case CLWH_ELEM_U32: case CLWH_ELEM_F32: return 4;
    default: return 0;
  }
}

// ------------------------------------------------------------------------------------------------
// transfer functions

void clvr::tf_to_dev(const clwh_tf &tf, TfDev &d) {
  std::memset(&d, 0, sizeof d);
  d.n = tf.n;
  for (int k = 0; k < tf.n; ++k) {
    const clwh_tf_rule &r = tf.rules[k];
    TfRuleDev &o = d.rules[k];
    o.v_lo = r.v_lo; o.v_hi = r.v_hi; o.g_lo = r.g_lo; o.g_hi = r.g_hi;
    o.flags = (r.use_gradient ? TF_USE_GRADIENT : 0u) | (r.writes_color ? TF_WRITES_COLOR : 0u) |
              (r.terminal ? TF_TERMINAL : 0u);
    o.color = ((uint32_t)r.color[0] & 255u) | (((uint32_t)r.color[1] & 255u) << 8) |
              (((uint32_t)r.color[2] & 255u) << 16) | (((uint32_t)r.color[3] & 255u) << 24);
    if (r.use_gradient) d.uses_gradient = 1;
  }
  // the border texel's class (see TfDev::border_class); tables that read `gradient` classify such positions literally
  for (int k = 0; k < tf.n && !d.uses_gradient; ++k) {
    const clwh_tf_rule &r = tf.rules[k];
    if (r.v_lo <= 0 && 0 <= r.v_hi) { d.border_class = k + 1; break; }
    if (r.terminal) break;
  }
}

// ---- hiprtc fallback (tf_jit.cpp): compile once per source text and context
int clvr::jit_for_source(clwh_ctx *ctx, const char *source, std::shared_ptr<JitTf> &out) {
  auto it = ctx->classes.cache.find(source);
  if (it != ctx->classes.cache.end()) {
    out = it->second;
    return CLWH_OK;
  }
  auto j = std::make_shared<JitTf>();
  j->source = source;
  std::string log;
  const int rc = tf_jit_compile(source, j->code, log);
  if (rc != CLWH_OK) {
    if (!log.empty()) std::fprintf(stderr, "clwhip: transfer-function source is neither in the rule grammar nor compilable:\n%s\n", log.c_str());
    return rc;
  }
  ctx->classes.cache[source] = j;
  out = j;
  return CLWH_OK;
}

int clvr::ensure_classes(clwh_ctx *ctx, const std::shared_ptr<JitTf> &jit, const clwh_mem *volume, TfDev &tf_out, const uint8_t **cls_out) {
  TfClasses &c = ctx->classes;
  if (c.cls.ptr && c.vol == volume->dptr && c.vol_ver == volume->version() && c.source == jit->source) {
    tf_out = c.tf;
    *cls_out = c.cls.as<uint8_t>();
    return CLWH_OK;
  }
  if (!jit->module) {
    HIP_TRY(hipModuleLoadData(&jit->module, jit->code.data()));
    HIP_TRY(hipModuleGetFunction(&jit->classify, jit->module, "clvr_tf_classify"));
  }
  const size_t voxels = volume->dims[0] * volume->dims[1] * volume->dims[2];
  CLWH_TRY(c.cls.reserve(ctx->stream, voxels));
  constexpr int kColors = CLWH_TF_MAX_RULES;
  CLWH_TRY(c.palette.reserve(ctx->stream, (kColors + 2) * sizeof(unsigned long long)));  // colours, error word, border class
  unsigned long long *palette = c.palette.as<unsigned long long>();
  HIP_TRY(hipMemsetAsync(palette, 0xFF, kColors * sizeof(unsigned long long), ctx->stream));
  HIP_TRY(hipMemsetAsync(palette + kColors, 0, 2 * sizeof(unsigned long long), ctx->stream));
  const void *vol = volume->dptr;
  int X = (int)volume->dims[0], Y = (int)volume->dims[1], Z = (int)volume->dims[2], max_colors = kColors;
  unsigned char *cls = c.cls.as<unsigned char>();
  int *error = reinterpret_cast<int *>(palette + kColors);
  int *border = reinterpret_cast<int *>(palette + kColors + 1);
  void *args[] = {&vol, &X, &Y, &Z, &cls, &palette, &max_colors, &error, &border};
  const size_t blocks = std::min<size_t>((voxels + 255u) / 256u, (size_t)1u << 23);  // the classifier strides over the rest
  HIP_TRY(hipModuleLaunchKernel(jit->classify, (unsigned)blocks, 1, 1, 256, 1, 1, 0, ctx->stream, args, nullptr));
  unsigned long long host[kColors + 2];
  HIP_TRY(hipMemcpyAsync(host, palette, sizeof host, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  c.vol = nullptr;  // invalid until fully built
  if ((int)(host[kColors] & 0xFFFFFFFFull) != 0) return CLWH_ERR_TF_UNSUPPORTED;  // more distinct colours than the table holds
  TfDev t;
  std::memset(&t, 0, sizeof t);
  t.opaque = 1;
  for (int k = 0; k < kColors && host[k] != ~0ull; ++k) {
    t.rules[k].flags = (host[k] >> 32) & 1ull ? TF_WRITES_COLOR : 0u;
    t.rules[k].color = (uint32_t)(host[k] & 0xFFFFFFFFull);
    t.n = k + 1;
  }
  t.border_class = (int32_t)(host[kColors + 1] & 0xFFull);  // is_event_gen(0, 0): the border texel (TfDev::border_class)
  c.tf = t;
  c.vol = volume->dptr;
  c.vol_ver = volume->version();
  c.source = jit->source;
  tf_out = t;
  *cls_out = cls;
  return CLWH_OK;
}

// ------------------------------------------------------------------------------------------------
// context

Tuning clvr::tuning_from_environment() {
  Tuning t;
  auto clamped = [](const char *e, int lo, int hi) { return std::max(lo, std::min(hi, std::atoi(e))); };
  if (const char *e = std::getenv("CLWH_TUNE_STEP")) t.step_min_lanes = clamped(e, 0, 64);
  if (const char *e = std::getenv("CLWH_TUNE_REFILL")) t.refill_min_lanes = clamped(e, 0, 64);
  if (const char *e = std::getenv("CLWH_TUNE_LITERAL_GRADIENT")) t.literal_gradient = std::atoi(e) != 0;
  if (const char *e = std::getenv("CLWH_TUNE_AFFINITY")) t.unit_affinity = std::atoi(e);
  if (const char *e = std::getenv("CLWH_TUNE_QUEUES")) t.unit_queues = clamped(e, 1, 8);
  if (const char *e = std::getenv("CLWH_TUNE_GROUP")) t.unit_group = std::max(1, std::atoi(e));
  if (const char *e = std::getenv("CLWH_TUNE_CHUNK_BLOCK_LOG2")) t.unit_block_log2 = clamped(e, 0, 8);
  if (const char *e = std::getenv("CLWH_TUNE_UNIT_AHEAD")) t.unit_ahead = std::atoi(e) != 0;
  if (const char *e = std::getenv("CLWH_TUNE_BLOCKS")) t.bounce_max_blocks = (uint32_t)std::max(1, std::atoi(e));
  if (const char *e = std::getenv("CLWH_TUNE_MACRO_SHIFT")) t.macro_shift = std::atoi(e);
  if (const char *e = std::getenv("CLWH_TUNE_LONG_LAUNCH")) t.force_long_launch = std::atoi(e) != 0;
  if (const char *e = std::getenv("CLWH_TUNE_BOUNCE_RAYS")) t.bounce_rays = std::atoi(e) == 2 ? 2 : 1;
  if (const char *e = std::getenv("CLWH_TUNE_SDF")) t.sdf_front = std::strcmp(e, "front") == 0;
  if (const char *e = std::getenv("CLWH_TUNE_DIST_LINES")) t.dist_lines = std::strcmp(e, "scan") == 0 ? 1 : std::strcmp(e, "search") == 0 ? 2 : 0;
  if (const char *e = std::getenv("CLWH_TUNE_LABEL_STATS")) t.label_stats = std::strcmp(e, "item") == 0 ? 1 : std::strcmp(e, "direct") == 0 ? 2 : 0;
  if (const char *e = std::getenv("CLWH_TUNE_SLICE_COARSE")) t.slice_coarse = std::atoi(e) != 0;
  if (const char *e = std::getenv("CLWH_TUNE_SDFBIT_WAVES")) t.sdfbit_waves = std::atoi(e) == 16 ? 16 : 8;
  if (const char *e = std::getenv("CLWH_TUNE_SDFBIT_GRID")) t.sdfbit_grid = std::max(1, std::atoi(e));
  if (const char *e = std::getenv("CLWH_TUNE_SDFBIT_REC")) t.sdfbit_rec_lds = std::strcmp(e, "lds") == 0 ? 1 : 0;
  if (const char *e = std::getenv("CLWH_TUNE_CERT")) t.cert_min_step = clamped(e, 0, 127);
  if (const char *e = std::getenv("CLWH_TUNE_CERT_HINT")) t.cert_hint = std::atoi(e) != 0;
  if (const char *e = std::getenv("CLWH_TUNE_START_CERT")) t.start_cert = std::atoi(e) != 0;
  if (const char *e = std::getenv("CLWH_TUNE_HULL_CERT")) t.hull_cert = std::atoi(e) != 0;
  if (const char *e = std::getenv("CLWH_TUNE_HULL_DEFER")) t.hull_defer = std::atoi(e) != 0;
  if (const char *e = std::getenv("CLWH_TUNE_HULL_TILT")) t.hull_tilt = std::atoi(e) != 0;
  return t;
}

int clvr::check_device_flags(clwh_ctx *ctx) {
  PassScratch &p = ctx->pass;
  if (!p.fixup_overflow_pending || !p.sticky_flags.ptr) return CLWH_OK;
  uint32_t flag = 0;
  HIP_TRY(hipMemcpyAsync(&flag, p.sticky_flags.ptr, sizeof flag, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  p.fixup_overflow_pending = false;
  if (!flag) return CLWH_OK;
  // the flag is sticky on the device (no render resets it): cleared here, once it has been reported
  HIP_TRY(hipMemsetAsync(p.sticky_flags.ptr, 0, sizeof(uint32_t), ctx->stream));
  return CLWH_ERR_INTERNAL_OVERFLOW;
}

// the next (begin, end) pair of the context's timers, `begin` recorded; *end stays null when timing is off
int clvr::timed_begin(clwh_ctx *ctx, int which, hipEvent_t *end) {
  LaunchTimers &t = ctx->timers;
  if (!t.enabled) return CLWH_OK;
  if (t.used == t.pairs.size()) {
    LaunchTimers::Pair &fresh = t.pairs.emplace_back();
    int rc = fresh.begin.ensure(hipEventDefault);
    if (rc == CLWH_OK) rc = fresh.end.ensure(hipEventDefault);
    if (rc != CLWH_OK) {
      t.pairs.pop_back();  // (a pair that fails half-way lets go of its first event)
      return rc;
    }
  }
  LaunchTimers::Pair &p = t.pairs[t.used++];
  p.which = which;
  HIP_TRY(hipEventRecord(p.begin.ev, ctx->stream));
  *end = p.end.ev;
  return CLWH_OK;
}

static int order_streams(clwh_ctx *ctx, hipStream_t first, hipStream_t then) {
  HIP_TRY(hipSetDevice(ctx->device));
  CLWH_TRY(ctx->handoff.ensure(hipEventDisableTiming));
  HIP_TRY(hipEventRecord(ctx->handoff.ev, first));
  HIP_TRY(hipStreamWaitEvent(then, ctx->handoff.ev, 0));
  return CLWH_OK;
}

extern "C" {

int clwh_ctx_create_on_stream(int device, void *hip_stream, clwh_ctx **out) {
  if (!out) return CLWH_ERR_INVALID_VALUE;
  *out = nullptr;
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) {
    note_hip_error(e);
    return CLWH_ERR_NO_DEVICE;
  }
  if (device < 0 || device >= count) return CLWH_ERR_NO_DEVICE;
  HIP_TRY(hipSetDevice(device));
  clwh_ctx *c = new (std::nothrow) clwh_ctx();
  if (!c) return CLWH_ERR_OUT_OF_MEMORY;
  c->device = device;
  c->stream = (hipStream_t)hip_stream;
  c->own_stream = false;
  c->tune = tuning_from_environment();
  *out = c;
  return CLWH_OK;
}

int clwh_ctx_create(int device, clwh_ctx **out) {
  CLWH_TRY(clwh_ctx_create_on_stream(device, nullptr, out));
  hipStream_t s;
  hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
  if (e != hipSuccess) {
    note_hip_error(e);
    delete *out;
    *out = nullptr;
    return CLWH_ERR_HIP;
  }
  (*out)->stream = s;
  (*out)->own_stream = true;
  return CLWH_OK;
}

// the members free what they own; what is left here is what only the context as a whole can do
int clwh_ctx_destroy(clwh_ctx *ctx) {
  if (!ctx) return CLWH_ERR_INVALID_VALUE;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  for (auto &kv : ctx->classes.cache)
    if (kv.second->module) (void)hipModuleUnload(kv.second->module);
  ctx->scene.reset();
  const hipStream_t owned = ctx->own_stream ? ctx->stream : nullptr;
  delete ctx;
  if (owned) (void)hipStreamDestroy(owned);
  return CLWH_OK;
}

int clwh_ctx_finish(clwh_ctx *ctx) {
  if (!ctx) return CLWH_ERR_INVALID_VALUE;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return check_device_flags(ctx);
}

int clwh_ctx_acquire_from(clwh_ctx *ctx, void *hip_stream) {
  if (!ctx) return CLWH_ERR_INVALID_VALUE;
  return order_streams(ctx, (hipStream_t)hip_stream, ctx->stream);
}

int clwh_ctx_release_to(clwh_ctx *ctx, void *hip_stream) {
  if (!ctx) return CLWH_ERR_INVALID_VALUE;
  return order_streams(ctx, ctx->stream, (hipStream_t)hip_stream);
}

void *clwh_ctx_stream(clwh_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }
int clwh_ctx_device(clwh_ctx *ctx) { return ctx ? ctx->device : -1; }

int clwh_ctx_set_timing(clwh_ctx *ctx, int enabled) {
  if (!ctx) return CLWH_ERR_INVALID_VALUE;
  ctx->timers.enabled = enabled != 0;
  ctx->timers.used = 0;
  return CLWH_OK;
}

int clwh_ctx_timing_read_all(clwh_ctx *ctx, float *ms, int32_t *launches, int32_t n) {
  if (!ctx || !ms || !launches || n <= 0) return CLWH_ERR_INVALID_VALUE;
  for (int k = 0; k < n; ++k) { ms[k] = 0.0f; launches[k] = 0; }
  HIP_TRY(hipSetDevice(ctx->device));
  LaunchTimers &timers = ctx->timers;
  for (size_t i = 0; i < timers.used; ++i) {
    const LaunchTimers::Pair &p = timers.pairs[i];
    HIP_TRY(hipEventSynchronize(p.end.ev));
    float t = 0.0f;
    HIP_TRY(hipEventElapsedTime(&t, p.begin.ev, p.end.ev));
    if (p.which >= 0 && p.which < n) { ms[p.which] += t; launches[p.which] += 1; }
  }
  timers.used = 0;
  return CLWH_OK;
}

int clwh_ctx_timing_read(clwh_ctx *ctx, float *total_ms, int32_t *launches) {
  if (!ctx || !total_ms || !launches) return CLWH_ERR_INVALID_VALUE;
  float ms[CLWH_TIMER_COUNT];
  int32_t n[CLWH_TIMER_COUNT];
  const int rc = clwh_ctx_timing_read_all(ctx, ms, n, CLWH_TIMER_COUNT);
  *total_ms = ms[CLWH_TIMER_BOUNCE];
  *launches = n[CLWH_TIMER_BOUNCE];
  return rc;
}

// ------------------------------------------------------------------------------------------------
// memory objects

static int mem_new(clwh_ctx *ctx, void *dptr, size_t bytes, bool owned, clwh_mem **out) {
  clwh_mem *m = new (std::nothrow) clwh_mem();
  if (!m) return CLWH_ERR_OUT_OF_MEMORY;
  m->ctx = ctx;
  m->dptr = dptr;
  m->bytes = bytes;
  m->owned = owned;
  m->cell = version_cell_of(dptr);
  // a new version also for a wrap of memory another clwh_mem already names: the caller may have rewritten it since, and
  // the address may have been reused by its allocator -- the owner's derived data is rebuilt once per wrap
  touch(m);
  *out = m;
  return CLWH_OK;
}

int clwh_mem_create(clwh_ctx *ctx, size_t bytes, int flags, clwh_mem **out) {
  if (!ctx || !out || bytes == 0) return CLWH_ERR_INVALID_VALUE;
  *out = nullptr;
  HIP_TRY(hipSetDevice(ctx->device));
  DeviceBuffer fresh;
  CLWH_TRY(fresh.reserve(ctx->stream, bytes));
  CLWH_TRY(mem_new(ctx, fresh.ptr, bytes, true, out));
  (void)fresh.release();  // the clwh_mem owns it from here (clwh_mem_release)
  (*out)->flags = flags;
  return CLWH_OK;
}

int clwh_mem_wrap(clwh_ctx *ctx, void *device_ptr, size_t bytes, clwh_mem **out) {
  if (!ctx || !out || !device_ptr || bytes == 0) return CLWH_ERR_INVALID_VALUE;
  *out = nullptr;
  return mem_new(ctx, device_ptr, bytes, false, out);
}

static bool image_format_ok(int channels, int elem_kind) {
  return elem_size(elem_kind) != 0 && (channels == 1 || channels == 2 || channels == 4);
}

static int image_describe(clwh_mem *m, const size_t dims[3], int channels, int elem_kind) {
  if (!image_format_ok(channels, elem_kind)) return CLWH_ERR_INVALID_VALUE;
  m->is_image = true;
  for (int k = 0; k < 3; ++k) m->dims[k] = dims[k];
  m->channels = channels;
  m->elem_kind = elem_kind;
  return CLWH_OK;
}

// an extent of 0 counts as 1
static void image_dims(const size_t in[3], size_t d[3]) {
  for (int k = 0; k < 3; ++k) d[k] = in[k] == 0 ? 1 : in[k];
}

int clwh_image_create(clwh_ctx *ctx, const size_t dims[3], int channels, int elem_kind, int flags, clwh_mem **out) {
  if (!ctx || !out || !dims) return CLWH_ERR_INVALID_VALUE;
  *out = nullptr;
  if (!image_format_ok(channels, elem_kind)) return CLWH_ERR_INVALID_VALUE;
  size_t d[3];
  image_dims(dims, d);
  // clw_image.hpp:45-58: width must exceed 1
  if (!(d[0] > 1)) return CLWH_ERR_INVALID_VALUE;
  const size_t bytes = d[0] * d[1] * d[2] * (size_t)channels * elem_size(elem_kind);
  CLWH_TRY(clwh_mem_create(ctx, bytes, flags, out));
  return image_describe(*out, d, channels, elem_kind);
}

int clwh_image_wrap(clwh_ctx *ctx, void *device_ptr, const size_t dims[3], int channels, int elem_kind, clwh_mem **out) {
  if (!ctx || !out || !dims || !device_ptr) return CLWH_ERR_INVALID_VALUE;
  *out = nullptr;
  const size_t es = elem_size(elem_kind);
  if (es == 0) return CLWH_ERR_INVALID_VALUE;
  size_t d[3];
  image_dims(dims, d);
  CLWH_TRY(mem_new(ctx, device_ptr, d[0] * d[1] * d[2] * (size_t)channels * es, false, out));
  const int rc = image_describe(*out, d, channels, elem_kind);
  if (rc != CLWH_OK) {
    delete *out;
    *out = nullptr;
  }
  return rc;
}

int clwh_mem_push(clwh_ctx *ctx, clwh_mem *mem, const void *host, size_t bytes) {
  if (!ctx || !mem || !host) return CLWH_ERR_INVALID_VALUE;
  if (bytes != mem->bytes) return CLWH_ERR_SIZE_MISMATCH;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMemcpyAsync(mem->dptr, host, bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  touch(mem);
  return CLWH_OK;
}

int clwh_mem_pull(clwh_ctx *ctx, clwh_mem *mem, void *host, size_t bytes) {
  if (!ctx || !mem || !host) return CLWH_ERR_INVALID_VALUE;
  if (bytes != mem->bytes) return CLWH_ERR_SIZE_MISMATCH;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMemcpyAsync(host, mem->dptr, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return check_device_flags(ctx);
}

int clwh_mem_release(clwh_mem *mem) {
  if (!mem) return CLWH_ERR_INVALID_VALUE;
  int rc = CLWH_OK;
  if (mem->owned && mem->dptr) {
    (void)hipSetDevice(mem->ctx->device);
    (void)hipStreamSynchronize(mem->ctx->stream);
    hipError_t e = hipFree(mem->dptr);
    if (e != hipSuccess) {
      note_hip_error(e);
      rc = CLWH_ERR_HIP;
    }
  }
  delete mem;
  return rc;
}

int clwh_host_register(void *host, size_t bytes) {
  if (!host || bytes == 0) return CLWH_ERR_INVALID_VALUE;
  HIP_TRY(hipHostRegister(host, bytes, hipHostRegisterDefault));
  return CLWH_OK;
}

int clwh_host_unregister(void *host) {
  if (!host) return CLWH_ERR_INVALID_VALUE;
  HIP_TRY(hipHostUnregister(host));
  return CLWH_OK;
}

void *clwh_mem_device_ptr(clwh_mem *mem) { return mem ? mem->dptr : nullptr; }
size_t clwh_mem_size(clwh_mem *mem) { return mem ? mem->bytes : 0; }
int clwh_mem_mark_dirty(clwh_mem *mem) {
  if (!mem) return CLWH_ERR_INVALID_VALUE;
  touch(mem);
  return CLWH_OK;
}

int clwh_buffer_reset(clwh_ctx *ctx, clwh_mem *buffer_volume) {
  if (!ctx || !buffer_volume) return CLWH_ERR_INVALID_VALUE;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMemsetAsync(buffer_volume->dptr, 0, buffer_volume->bytes, ctx->stream));
  touch(buffer_volume);
  return CLWH_OK;
}

// ------------------------------------------------------------------------------------------------
// diagnostics

const char *clwh_strerror(int status) {
  switch (status) {
    case CLWH_OK: return "CLWH_OK";
    case CLWH_ERR_INVALID_VALUE: return "CLWH_ERR_INVALID_VALUE";
    case CLWH_ERR_NO_DEVICE: return "CLWH_ERR_NO_DEVICE";
    case CLWH_ERR_OUT_OF_MEMORY: return "CLWH_ERR_OUT_OF_MEMORY";
    case CLWH_ERR_HIP: return "CLWH_ERR_HIP";
    case CLWH_ERR_UNKNOWN_KERNEL: return "CLWH_ERR_UNKNOWN_KERNEL";
    case CLWH_ERR_TF_UNSUPPORTED: return "CLWH_ERR_TF_UNSUPPORTED";
    case CLWH_ERR_BAD_ARGS: return "CLWH_ERR_BAD_ARGS";
    case CLWH_ERR_BAD_NDRANGE: return "CLWH_ERR_BAD_NDRANGE";
    case CLWH_ERR_SIZE_MISMATCH: return "CLWH_ERR_SIZE_MISMATCH";
    case CLWH_ERR_INTERNAL_OVERFLOW: return "CLWH_ERR_INTERNAL_OVERFLOW";
    default: return "CLWH_ERR_UNKNOWN";
  }
}

int clwh_last_hip_error(void) { return g_last_hip_error; }
const char *clwh_version(void) { return "clwhip 0.1 (gfx950)"; }

}  // extern "C"
