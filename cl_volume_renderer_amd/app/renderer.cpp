#include "renderer.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <set>

#include <clwh.h>

#include "common_defines.hpp"

// Mirrors the sequencing of the reference's app/renderer.cpp; what differs is below the clw_* API:
// no JIT on flush, the SDF build is one call, and the frame the caller receives is resolved after the
// pass instead of being read from the cache while other work-items still add to it.

renderer::renderer(clw_context &c)
    : ctx(c),
      render_func(ctx, "empty.cl", "empty"),
      frame(ctx, std::vector<unsigned char>((size_t)SCREEN_WIDTH * SCREEN_HEIGHT * 4), {SCREEN_WIDTH, SCREEN_HEIGHT, 1}),
      buffer_volume(ctx, std::vector<unsigned short>(8 * 4)),
      tfframe(ctx, std::vector<unsigned char>(2 * 2 * 4), {2, 2, 1}),
      composite_lut(ctx, std::vector<float>(4)),
      region_mask(ctx, std::vector<uint32_t>(2)),
      held_mask(ctx, std::vector<uint32_t>(2)),
      region_labels(ctx, std::vector<uint32_t>(1)),
      region_dist(ctx, std::vector<uint32_t>(1)),
      region_cost(ctx, std::vector<uint16_t>(1)),
      overlay_palette(ctx, std::vector<uint32_t>(overlay_colours()), true),
      sdf(ctx) {}

void renderer::image_set(const reference_volume *rv, const env_map *map) {
  volume = rv;
  emap = map;
}

void renderer::next_event_code_set(const std::string cl_code) { local_cl_code = cl_code; }

// reference :25-43 -- (re)allocate + zero the voxel cache, rebuild the render function and the SDF
void renderer::flush_changes() {
  const auto dims = volume->get_volume_size();
  // the reference allocates X*Y*Z*4 ushorts and can index one row past it (opencl_kernels/utility.cl:21
  // with utility_ray.cl:112-117); the padded length keeps that access inside the buffer
  const size_t cache_len = (size_t)clwh_cache_len((uint32_t)dims[0], (uint32_t)dims[1], (uint32_t)dims[2]);
  if (buffer_volume.size() != cache_len)
    buffer_volume = clw_vector<unsigned short>(ctx, std::vector<unsigned short>(cache_len), false);

  auto buffer_reset = clw_function(ctx, "buffer_reset.cl", "buffer_reset");
  buffer_reset.execute(volume->get_volume_size_evenness(4), {4, 4, 4}, volume->get_reference_volume(), buffer_volume);

  render_func = clw_function(ctx, "ray_marching.cl", "render", local_cl_code);
  sdf = signed_distance_field(ctx, *volume, local_cl_code);
}

// reference :131-158 -- one sample per pixel with a fresh std::rand() seed, then a blocking readback
void *renderer::render_frame(struct ui_state &state, bool &frame_changed) {
  frame_changed = false;
  if (!state.cam_changed && !state.path_changed) return &frame[0];

  Position3D vec(state.direction_look[0], state.direction_look[1], 0.0, {1.0, 0.0, 0.0});
  const int random_seed = std::rand();

  render_func.execute({(size_t)state.width, (size_t)state.height, 1}, {8, 8, 1}, frame, volume->get_reference_volume(),
                      sdf.get_sdf_buffer(), emap->get_buffer(), buffer_volume, state.position.val[0],
                      state.position.val[1], state.position.val[2], vec.val[0], vec.val[1], vec.val[2], random_seed);
  frame.pull();

  state.cam_changed = false;
  state.path_changed = false;
  frame_changed = true;
  return &frame[0];
}

void renderer::render_frame_device(struct ui_state &state, const clw_foreign_memory &target, int passes) {
  if (!state.cam_changed && !state.path_changed) return;
  Position3D vec(state.direction_look[0], state.direction_look[1], 0.0, {1.0, 0.0, 0.0});
  clwh_render_desc d{};
  d.frame = target.get_device_reference();
  d.volume = volume->get_reference_volume().get_device_reference();
  d.sdf = sdf.get_sdf_buffer().get_device_reference();
  d.env = emap->get_buffer().get_device_reference();
  d.buffer_volume = buffer_volume.get_device_reference();
  for (int q = 0; q < 3; ++q) {
    d.cam_pos[q] = (float)state.position.val[q];
    d.cam_dir[q] = (float)vec.val[q];
  }
  d.width = (uint32_t)state.width;
  d.height = (uint32_t)state.height;
  d.accum_mode = CLWH_ACCUM_VOXEL_CACHE;
  d.tile_world = 1;
  d.write_frame = 1;
  passes = std::max(1, std::min(passes, CLWH_MAX_SEEDS));
  d.n_seeds = passes;
  for (int k = 0; k < passes; ++k) d.seeds[k] = std::rand();  // the seeds `passes` render_frame calls would have drawn
  target.acquire();
  clw_fail_hard_on_error(clwh_render(render_func.get_kernel(), &d));
  target.release();
  state.cam_changed = false;
  state.path_changed = false;
}

// what the view descriptors share: the frame, the volume and the launched region (every view) ...
template <class Desc>
static void fill_region(Desc &d, const clw_image<unsigned char, 4> &frame, const reference_volume &volume, const struct ui_state &state) {
  d.frame = frame.get_device_reference();
  d.volume = volume.get_reference_volume().get_device_reference();
  d.width = (uint32_t)state.width;
  d.height = (uint32_t)state.height;
}
// ... and the camera of `state` with the whole ray as the slab (the camera views)
template <class Desc>
static void fill_view(Desc &d, const clw_image<unsigned char, 4> &frame, const reference_volume &volume, const struct ui_state &state) {
  fill_region(d, frame, volume, state);
  Position3D vec(state.direction_look[0], state.direction_look[1], 0.0, {1.0, 0.0, 0.0});
  for (int q = 0; q < 3; ++q) {
    d.cam_pos[q] = (float)state.position.val[q];
    d.cam_dir[q] = (float)vec.val[q];
  }
  d.t_near = 0.0f;
  d.t_far = INFINITY;
}

void *renderer::render_projection(struct ui_state &state, int mode, float center, float width, float step) {
  clwh_projection_desc d{};
  fill_view(d, frame, *volume, state);
  d.mode = mode;
  d.step = step;
  d.window_center = center;
  d.window_width = width;
  clw_fail_hard_on_error(clwh_render_projection(ctx.get_handle(), &d));
  frame.pull();
  return &frame[0];
}

void *renderer::render_composite(struct ui_state &state, const std::vector<float> &lut, int lut_first, int lut_len, float step,
                                 float alpha_stop, int flags, float ambient) {
  if (lut_len < 1 || lut.size() < (size_t)lut_len * 4) clw_fail_hard_on_error(CLWH_ERR_SIZE_MISMATCH);
  // a new table only when the contents changed: the push gives the device memory a new content version, which rebuilds the
  // library's derived prefix table
  const bool same = composite_lut.size() == lut.size() && std::memcmp(&composite_lut[0], lut.data(), lut.size() * sizeof(float)) == 0;
  if (!same || !composite_lut_pushed) {
    composite_lut = clw_vector<float>(ctx, std::vector<float>(lut), true);
    composite_lut_pushed = true;
  }
  clwh_composite_desc d{};
  fill_view(d, frame, *volume, state);
  d.flags = flags;
  d.step = step;
  d.lut = composite_lut.get_device_reference();
  d.lut_first = lut_first;
  d.lut_len = lut_len;
  d.alpha_stop = alpha_stop;
  d.ambient = ambient;
  clw_fail_hard_on_error(clwh_render_composite(ctx.get_handle(), &d));
  frame.pull();
  return &frame[0];
}

void *renderer::render_isosurface(struct ui_state &state, float iso, int flags, float step, int refine, float ambient, float red,
                                  float green, float blue) {
  clwh_isosurface_desc d{};
  fill_view(d, frame, *volume, state);
  d.flags = flags;
  d.step = step;
  d.iso = iso;
  d.refine = refine;
  d.color[0] = red;
  d.color[1] = green;
  d.color[2] = blue;
  d.ambient = ambient;
  clw_fail_hard_on_error(clwh_render_isosurface(ctx.get_handle(), &d));
  frame.pull();
  return &frame[0];
}

void renderer::slice_plane(const size_t dims[3], int orientation, float position, int width, int height, int slab_samples, float step,
                           float origin[3], float du[3], float dv[3], float normal[3]) {
  static const int axes[3][3] = {{0, 1, 2}, {0, 2, 1}, {1, 2, 0}};  // (axis of du, axis of dv, axis of the normal)
  const int iu = axes[orientation][0], iv = axes[orientation][1], iw = axes[orientation][2];
  const double a = (double)dims[iu], b = (double)dims[iv];
  const double s = std::max(a / (double)width, b / (double)height);
  double o[3] = {0.0, 0.0, 0.0};
  o[iu] = a / 2.0 + (0.5 - (double)width / 2.0) * s;
  o[iv] = b / 2.0 + (0.5 - (double)height / 2.0) * s;
  o[iw] = (double)position + 0.5 - (double)(slab_samples - 1) * (double)step / 2.0;
  for (int q = 0; q < 3; ++q) {
    origin[q] = (float)o[q];
    du[q] = dv[q] = normal[q] = 0.0f;
  }
  du[iu] = dv[iv] = (float)s;
  normal[iw] = 1.0f;
}

void *renderer::render_slice(struct ui_state &state, int orientation, float position, int mode, int slab_samples, float step, float center,
                             float width, int flags) {
  if (orientation < SLICE_AXIAL || orientation > SLICE_SAGITTAL || state.width < 1 || state.height < 1) clw_fail_hard_on_error(CLWH_ERR_INVALID_VALUE);
  clwh_slice_desc d{};
  fill_region(d, frame, *volume, state);
  const auto &size = volume->get_volume_size();
  const size_t dims[3] = {size[0], size[1], size[2]};
  slice_plane(dims, orientation, position, state.width, state.height, slab_samples, step, d.origin, d.du, d.dv, d.normal);
  d.mode = mode;
  d.flags = flags;
  d.slab_samples = slab_samples;
  d.step = step;
  d.window_center = center;
  d.window_width = width;
  clw_fail_hard_on_error(clwh_render_slice(ctx.get_handle(), &d));
  frame.pull();
  return &frame[0];
}

// scene.curve_frames, operation for operation (binary64, + - * / and sqrt in the same order; the library is built without contraction)
namespace {
struct vec3 {
  double v[3];
  double &operator[](int q) { return v[q]; }
  double operator[](int q) const { return v[q]; }
};
inline double dot3(const vec3 &a, const vec3 &b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
inline vec3 unit3(const vec3 &a) {
  const double n = std::sqrt(dot3(a, a));
  if (n == 0.0) clw_fail_hard_on_error(CLWH_ERR_INVALID_VALUE);
  return vec3{{a[0] / n, a[1] / n, a[2] / n}};
}
inline vec3 minus3(const vec3 &a, const vec3 &b) { return vec3{{a[0] - b[0], a[1] - b[1], a[2] - b[2]}}; }
// a - k * b
inline vec3 less3(const vec3 &a, double k, const vec3 &b) { return vec3{{a[0] - k * b[0], a[1] - k * b[1], a[2] - k * b[2]}}; }
}  // namespace

renderer::curve_frame_set renderer::curve_frames(const std::vector<double> &points, const double spacing[3], int width, double pixel_mm,
                                                 double station_mm, int smooth_passes, double angle, int slab_samples, double step_mm) {
  if (step_mm == 0.0) step_mm = pixel_mm;
  const size_t m = points.size() / 3;
  if (m < 2 || !(pixel_mm > 0.0 && station_mm > 0.0 && step_mm > 0.0 && spacing[0] > 0.0 && spacing[1] > 0.0 && spacing[2] > 0.0))
    clw_fail_hard_on_error(CLWH_ERR_INVALID_VALUE);
  std::vector<vec3> q(m);
  for (size_t i = 0; i < m; ++i) {
    if (i > 0 && points[3 * i] == points[3 * i - 3] && points[3 * i + 1] == points[3 * i - 2] && points[3 * i + 2] == points[3 * i - 1])
      clw_fail_hard_on_error(CLWH_ERR_INVALID_VALUE);
    for (int c = 0; c < 3; ++c) q[i][c] = (points[3 * i + c] + 0.5) * spacing[c];
  }
  for (int pass = 0; pass < smooth_passes; ++pass) {
    std::vector<vec3> next(q);
    for (size_t i = 1; i + 1 < m; ++i)
      for (int c = 0; c < 3; ++c) next[i][c] = ((q[i - 1][c] + 2.0 * q[i][c]) + q[i + 1][c]) / 4.0;
    q.swap(next);
  }
  std::vector<double> L(m, 0.0);
  for (size_t i = 0; i + 1 < m; ++i) {
    const vec3 d = minus3(q[i + 1], q[i]);
    L[i + 1] = L[i] + std::sqrt(dot3(d, d));
  }
  curve_frame_set out;
  const size_t n = (size_t)std::floor(L[m - 1] / station_mm) + 1;
  if (n < 2) clw_fail_hard_on_error(CLWH_ERR_INVALID_VALUE);
  out.n = n;
  out.s_mm.resize(n);
  std::vector<vec3> C(n), T(n), U(n);
  size_t i = 0;  // the last segment (i <= m - 2) whose L_i <= s_j: the stations come in increasing order
  for (size_t j = 0; j < n; ++j) {
    const double s = (double)j * station_mm;
    out.s_mm[j] = s;
    while (i < m - 2 && L[i + 1] <= s) ++i;
    const double span = L[i + 1] - L[i];
    const double f = span > 0.0 ? (s - L[i]) / span : 0.0;
    for (int c = 0; c < 3; ++c) C[j][c] = q[i][c] + f * (q[i + 1][c] - q[i][c]);
  }
  for (size_t j = 0; j < n; ++j) T[j] = unit3(minus3(C[std::min(j + 1, n - 1)], C[j > 0 ? j - 1 : 0]));
  int axis = 0;
  for (int c = 1; c < 3; ++c)
    if (std::fabs(T[0][c]) < std::fabs(T[0][axis])) axis = c;
  vec3 e{{0.0, 0.0, 0.0}};
  e[axis] = 1.0;
  U[0] = unit3(less3(e, dot3(e, T[0]), T[0]));
  for (size_t j = 0; j + 1 < n; ++j) {
    const vec3 v1 = minus3(C[j + 1], C[j]);
    const double c1 = dot3(v1, v1);
    if (c1 == 0.0) clw_fail_hard_on_error(CLWH_ERR_INVALID_VALUE);
    const vec3 rL = less3(U[j], (2.0 / c1) * dot3(v1, U[j]), v1);
    const vec3 tL = less3(T[j], (2.0 / c1) * dot3(v1, T[j]), v1);
    const vec3 v2 = minus3(T[j + 1], tL);
    const double c2 = dot3(v2, v2);
    const vec3 r = c2 == 0.0 ? rL : less3(rL, (2.0 / c2) * dot3(v2, rL), v2);
    U[j + 1] = unit3(less3(r, dot3(r, T[j + 1]), T[j + 1]));
  }
  const double co = std::cos(angle), si = std::sin(angle);
  const double hw = (double)(width - 1) / 2.0, hk = ((double)(slab_samples - 1) / 2.0) * step_mm;
  const size_t H = (n + 7) / 8 * 8;
  out.rows.assign(H * 9, 0.0f);
  for (size_t j = n; j < H; ++j) out.rows[9 * j] = out.rows[9 * j + 1] = out.rows[9 * j + 2] = -1.0f;  // padding: no kept sample
  for (size_t j = 0; j < n; ++j) {
    const vec3 &t = T[j], &u = U[j];
    const vec3 w{{t[1] * u[2] - t[2] * u[1], t[2] * u[0] - t[0] * u[2], t[0] * u[1] - t[1] * u[0]}};
    for (int c = 0; c < 3; ++c) {
      const double a = co * u[c] + si * w[c], nn = (-si) * u[c] + co * w[c];
      const double du = (a * pixel_mm) / spacing[c], normal = nn / spacing[c];
      out.rows[9 * j + c] = (float)((C[j][c] / spacing[c] - hw * du) - hk * normal);
      out.rows[9 * j + 3 + c] = (float)du;
      out.rows[9 * j + 6 + c] = (float)normal;
    }
  }
  return out;
}

void *renderer::render_curved(struct ui_state &, const curve_frame_set &frames, int width, int mode, int slab_samples, float step, float center,
                              float window_width, int flags) {
  const size_t H = frames.rows.size() / 9;
  if (H < 1 || H > (size_t)SCREEN_HEIGHT || width < 1 || width > SCREEN_WIDTH) clw_fail_hard_on_error(CLWH_ERR_INVALID_VALUE);
  clwh_curved_desc d{};
  d.frame = frame.get_device_reference();
  d.volume = volume->get_reference_volume().get_device_reference();
  d.rows = frames.rows.data();
  d.width = (uint32_t)width;
  d.height = (uint32_t)H;
  d.mode = mode;
  d.flags = flags;
  d.slab_samples = slab_samples;
  d.step = step;
  d.window_center = center;
  d.window_width = window_width;
  clw_fail_hard_on_error(clwh_render_curved(ctx.get_handle(), &d));
  frame.pull();
  return &frame[0];
}

renderer::profile_summary renderer::vessel_profile(struct ui_state &, const std::vector<uint32_t> &points, double pixel_mm, int window, bool connected) {
  const auto &size = volume->get_volume_size();
  if (region_mask.size() != 2 * ((size[0] + 63) / 64) * size[1] * size[2]) clw_fail_hard_on_error(CLWH_ERR_SIZE_MISMATCH);  // no mask
  const auto &sizes = volume->get_voxel_sizes();
  const double spacing[3] = {(double)sizes[0], (double)sizes[1], (double)sizes[2]};
  const curve_frame_set frames = curve_frames(std::vector<double>(points.begin(), points.end()), spacing, window, pixel_mm, pixel_mm, 8, 0.0, window, pixel_mm);
  profile_summary out;
  out.s_mm = frames.s_mm;
  clw_vector<uint32_t> table(ctx, std::vector<uint32_t>(frames.n * 4), false);
  clwh_curve_profile_desc d{};
  d.mask = region_mask.get_device_reference();
  for (int q = 0; q < 3; ++q) d.dims[q] = (uint32_t)size[q];
  d.rows = frames.rows.data();
  d.n_rows = (uint32_t)frames.n;
  d.width = (uint32_t)window;
  d.slab_samples = window;
  d.step = (float)pixel_mm;
  d.flags = connected ? CLWH_PROFILE_CONNECTED : 0;
  d.records = table.get_device_reference();
  clw_fail_hard_on_error(clwh_curve_profile(ctx.get_handle(), &d));
  table.pull();  // (waits for the stream)
  out.records.resize(frames.n);
  std::memcpy(out.records.data(), &table[0], frames.n * sizeof(clwh_section_record));
  for (const clwh_section_record &r : out.records) {  // scene.profile_measures
    const double area = (double)r.count * pixel_mm * pixel_mm;
    out.area_mm2.push_back(area);
    out.diameter_mm.push_back(2.0 * std::sqrt(area / 3.141592653589793));
    out.cut.push_back(r.border > 0 ? 1 : 0);
  }
  return out;
}

const std::vector<uint32_t> &renderer::overlay_colours() {
  static const uint8_t rgb[20][3] = {{230, 25, 75},   {60, 180, 75},   {255, 225, 25}, {0, 130, 200},   {245, 130, 48},
                                     {145, 30, 180},  {70, 240, 240},  {240, 50, 230}, {210, 245, 60},  {255, 140, 170},
                                     {0, 128, 128},   {220, 190, 255}, {170, 110, 40}, {255, 250, 200}, {128, 0, 0},
                                     {170, 255, 195}, {128, 128, 0},   {200, 160, 120}, {0, 0, 128},    {128, 128, 128}};
  static const std::vector<uint32_t> words = [] {
    std::vector<uint32_t> w;
    for (const auto &c : rgb) w.push_back((uint32_t)c[0] | (uint32_t)c[1] << 8 | (uint32_t)c[2] << 16 | 255u << 24);
    return w;
  }();
  return words;
}

// what the two overlay descriptors share: the frame and the launched region, the chosen region buffer, the palette and the style
template <class Desc>
void renderer::fill_overlay(Desc &d, const struct ui_state &state, int source, const overlay_style &style) {
  const auto &size = volume->get_volume_size();
  const size_t mask_words = 2 * ((size[0] + 63) / 64) * size[1] * size[2];
  const clw_vector<uint32_t> *buffer = nullptr;
  if (source == OVERLAY_REGION_MASK && region_mask.size() == mask_words) buffer = &region_mask;
  if (source == OVERLAY_HELD_MASK && held_mask.size() == mask_words) buffer = &held_mask;
  if (source == OVERLAY_LABELS && region_labels.size() == (size_t)size[0] * size[1] * size[2]) buffer = &region_labels;
  if (!buffer) clw_fail_hard_on_error(source < OVERLAY_REGION_MASK || source > OVERLAY_LABELS ? CLWH_ERR_INVALID_VALUE : CLWH_ERR_SIZE_MISMATCH);  // nothing grown, held or labelled
  d.frame = frame.get_device_reference();
  d.width = (uint32_t)state.width;
  d.height = (uint32_t)state.height;
  d.region.buffer = buffer->get_device_reference();
  d.region.kind = source == OVERLAY_LABELS ? CLWH_REGION_LABELS : CLWH_REGION_MASK;
  for (int q = 0; q < 3; ++q) d.region.dims[q] = (uint32_t)size[q];
  d.region.id_lo = style.id_lo;
  d.region.id_hi = style.id_hi;
  d.paint.palette = overlay_palette.get_device_reference();
  d.paint.n_colours = (uint32_t)overlay_palette.size();
  d.paint.flags = style.flags;
  d.paint.fill_alpha = style.fill_alpha;
  d.paint.outline_alpha = style.outline_alpha;
}

void *renderer::overlay_slice(struct ui_state &state, int source, int orientation, float position, int slab_samples, float step,
                              const overlay_style &style) {
  if (orientation < SLICE_AXIAL || orientation > SLICE_SAGITTAL || state.width < 1 || state.height < 1) clw_fail_hard_on_error(CLWH_ERR_INVALID_VALUE);
  clwh_overlay_slice_desc d{};
  fill_overlay(d, state, source, style);
  const auto &size = volume->get_volume_size();
  const size_t dims[3] = {size[0], size[1], size[2]};
  slice_plane(dims, orientation, position, state.width, state.height, slab_samples, step, d.origin, d.du, d.dv, d.normal);
  d.slab_samples = slab_samples;
  d.step = step;
  clw_fail_hard_on_error(clwh_overlay_slice(ctx.get_handle(), &d));
  frame.pull();
  return &frame[0];
}

void *renderer::overlay_camera(struct ui_state &state, int source, float step, const overlay_style &style) {
  clwh_overlay_camera_desc d{};
  fill_overlay(d, state, source, style);
  Position3D vec(state.direction_look[0], state.direction_look[1], 0.0, {1.0, 0.0, 0.0});
  for (int q = 0; q < 3; ++q) {
    d.cam_pos[q] = (float)state.position.val[q];
    d.cam_dir[q] = (float)vec.val[q];
  }
  d.step = step;
  d.t_near = 0.0f;
  d.t_far = INFINITY;
  clw_fail_hard_on_error(clwh_overlay_camera(ctx.get_handle(), &d));
  frame.pull();
  return &frame[0];
}

mesh_data renderer::extract_mesh(struct ui_state &, float iso, int flags) {
  mesh_data out;
  uint64_t nv = 0, nt = 0;
  clwh_mesh_desc d{};
  d.volume = volume->get_reference_volume().get_device_reference();
  d.iso = iso;
  d.flags = flags;
  d.n_vertices = &nv;
  d.n_triangles = &nt;
  clw_fail_hard_on_error(clwh_mesh_isosurface(ctx.get_handle(), &d));  // counts only
  if (nv == 0) return out;
  clw_vector<float> positions(ctx, std::vector<float>((size_t)nv * 3)), normals(ctx, std::vector<float>((size_t)nv * 3));
  clw_vector<uint64_t> keys(ctx, std::vector<uint64_t>((size_t)nv));
  clw_vector<uint32_t> triangles(ctx, std::vector<uint32_t>((size_t)nt * 3));
  d.positions = positions.get_device_reference();
  d.normals = normals.get_device_reference();
  d.keys = keys.get_device_reference();
  d.triangles = triangles.get_device_reference();
  d.vertex_capacity = nv;
  d.triangle_capacity = nt;
  clw_fail_hard_on_error(clwh_mesh_isosurface(ctx.get_handle(), &d));
  positions.pull();
  normals.pull();
  keys.pull();
  triangles.pull();
  out.positions.assign(&positions[0], &positions[0] + positions.size());
  out.normals.assign(&normals[0], &normals[0] + normals.size());
  out.keys.assign(&keys[0], &keys[0] + keys.size());
  out.triangles.assign(&triangles[0], &triangles[0] + triangles.size());
  return out;
}

clwh_grow_result renderer::grow_region(struct ui_state &, const std::vector<uint32_t> &seeds, int lo, int hi, int flags) {
  const auto &size = volume->get_volume_size();
  const size_t words = 2 * ((size[0] + 63) / 64) * size[1] * size[2];  // the mask layout of clwh_segment_grow
  if (region_mask.size() != words) {
    if (flags & CLWH_GROW_FROM_MASK) clw_fail_hard_on_error(CLWH_ERR_SIZE_MISMATCH);  // no mask of this volume to continue from
    region_mask = clw_vector<uint32_t>(ctx, std::vector<uint32_t>(words), false);
  }
  clwh_grow_result result{};
  clwh_grow_desc d{};
  d.volume = volume->get_reference_volume().get_device_reference();
  d.mask = region_mask.get_device_reference();
  d.lo = lo;
  d.hi = hi;
  d.flags = flags;
  d.n_seeds = (uint32_t)(seeds.size() / 3);
  d.seeds = seeds.data();
  d.result = &result;
  clw_fail_hard_on_error(clwh_segment_grow(ctx.get_handle(), &d));
  return result;
}

void renderer::apply_mask(struct ui_state &, int fill, int flags) {
  clwh_apply_mask_desc d{};
  d.volume_in = d.volume_out = volume->get_reference_volume().get_device_reference();
  d.mask = region_mask.get_device_reference();
  d.fill = fill;
  d.flags = flags;
  clw_fail_hard_on_error(clwh_volume_apply_mask(ctx.get_handle(), &d));
}

void renderer::filter_volume(struct ui_state &, int kind, const uint32_t radius[3], const std::array<std::vector<uint16_t>, 3> *weights, bool masked) {
  clwh_filter_desc d{};
  d.volume_in = d.volume_out = volume->get_reference_volume().get_device_reference();
  if (masked) {
    const auto &size = volume->get_volume_size();
    if (region_mask.size() != 2 * ((size[0] + 63) / 64) * size[1] * size[2]) clw_fail_hard_on_error(CLWH_ERR_SIZE_MISMATCH);  // no mask
    d.mask = region_mask.get_device_reference();
  }
  d.kind = kind;
  for (int q = 0; q < 3; ++q) {
    d.radius[q] = radius[q];
    if (weights) {
      if ((*weights)[q].size() != (size_t)radius[q] + 1u) clw_fail_hard_on_error(CLWH_ERR_INVALID_VALUE);
      d.weights[q] = (*weights)[q].data();
    }
  }
  clw_fail_hard_on_error(clwh_volume_filter(ctx.get_handle(), &d));
}

std::array<std::vector<uint16_t>, 3> renderer::gaussian_weights(double sigma_mm, const double spacing[3]) {
  std::array<std::vector<uint16_t>, 3> out;
  for (int c = 0; c < 3; ++c) {
    const double s = sigma_mm / spacing[c];
    if (!(s > 0.0)) {
      out[c] = {4096};
      continue;
    }
    const int r = std::min(16, std::max(1, (int)std::ceil(3.0 * s)));
    std::vector<double> g((size_t)r + 1u);
    for (int k = 0; k <= r; ++k) g[(size_t)k] = std::exp(-(double)(k * k) / (2.0 * s * s));
    double n = g[0];
    for (int k = 1; k <= r; ++k) n += 2.0 * g[(size_t)k];
    std::vector<uint16_t> w((size_t)r + 1u);
    int rest = 4096;
    for (int k = 1; k <= r; ++k) {
      w[(size_t)k] = (uint16_t)std::floor(4096.0 * g[(size_t)k] / n + 0.5);
      rest -= 2 * (int)w[(size_t)k];
    }
    w[0] = (uint16_t)rest;
    out[c] = w;
  }
  return out;
}

renderer::component_summary renderer::label_components(struct ui_state &, int lo, int hi, int flags, unsigned top_k) {
  const auto &size = volume->get_volume_size();
  const size_t voxels = (size_t)size[0] * size[1] * size[2], mask_words = 2 * ((size[0] + 63) / 64) * size[1] * size[2];
  if ((flags & CLWH_LABEL_FROM_MASK) && region_mask.size() != mask_words) clw_fail_hard_on_error(CLWH_ERR_SIZE_MISMATCH);  // no mask to split
  if (region_labels.size() != voxels) region_labels = clw_vector<uint32_t>(ctx, std::vector<uint32_t>(voxels), false);
  constexpr size_t record_words = sizeof(clwh_label_component) / sizeof(uint32_t);
  clw_vector<uint32_t> table(ctx, std::vector<uint32_t>(std::max<size_t>(top_k, 1) * record_words), false);
  clwh_label_result result{};
  clwh_label_desc d{};
  d.volume = volume->get_reference_volume().get_device_reference();
  d.labels = region_labels.get_device_reference();
  d.components = table.get_device_reference();
  d.component_capacity = top_k;
  d.mask = (flags & CLWH_LABEL_FROM_MASK) ? region_mask.get_device_reference() : nullptr;
  d.lo = lo;
  d.hi = hi;
  d.flags = flags;
  d.result = &result;
  clw_fail_hard_on_error(clwh_segment_label(ctx.get_handle(), &d));
  component_summary out;
  out.n_components = result.n_components;
  out.n_voxels = result.n_voxels;
  out.top.resize((size_t)std::min<uint64_t>(result.n_components, top_k));
  if (!out.top.empty()) {
    table.pull();
    std::memcpy(out.top.data(), &table[0], out.top.size() * sizeof(clwh_label_component));
  }
  return out;
}

void renderer::select_components(struct ui_state &, uint32_t rank_lo, uint32_t rank_hi) {
  const auto &size = volume->get_volume_size();
  const size_t words = 2 * ((size[0] + 63) / 64) * size[1] * size[2];
  if (region_labels.size() != (size_t)size[0] * size[1] * size[2]) clw_fail_hard_on_error(CLWH_ERR_SIZE_MISMATCH);  // nothing was labelled
  if (region_mask.size() != words) region_mask = clw_vector<uint32_t>(ctx, std::vector<uint32_t>(words), false);
  clwh_labels_to_mask_desc d{};
  d.labels = region_labels.get_device_reference();
  d.mask = region_mask.get_device_reference();
  for (int q = 0; q < 3; ++q) d.dims[q] = (uint32_t)size[q];
  d.rank_lo = rank_lo;
  d.rank_hi = rank_hi;
  clw_fail_hard_on_error(clwh_labels_to_mask(ctx.get_handle(), &d));
}

void renderer::mask_weights(uint32_t weight[3]) const {
  const auto &sizes = volume->get_voxel_sizes();
  for (int q = 0; q < 3; ++q) {
    const double s = (double)sizes[q] * 16.0;
    weight[q] = (uint32_t)std::max(1.0, std::nearbyint(s * s));  // round to nearest, halves to even, like Python's round
  }
}

uint32_t renderer::mask_radius_sq(float radius) {
  const double r = (double)radius * 16.0;
  return (uint32_t)std::min(std::floor(r * r), 4294967295.0);
}

std::vector<uint32_t> renderer::distance_map(struct ui_state &, bool to_clear, uint32_t cap) {
  const auto &size = volume->get_volume_size();
  if (region_mask.size() != 2 * ((size[0] + 63) / 64) * size[1] * size[2]) clw_fail_hard_on_error(CLWH_ERR_SIZE_MISMATCH);  // no mask
  clw_vector<uint32_t> map(ctx, std::vector<uint32_t>(size[0] * size[1] * size[2]), false);
  clwh_distance_desc d{};
  d.mask = region_mask.get_device_reference();
  d.dist = map.get_device_reference();
  for (int q = 0; q < 3; ++q) d.dims[q] = (uint32_t)size[q];
  mask_weights(d.weight);
  d.cap = cap;
  d.flags = to_clear ? CLWH_DIST_TO_CLEAR : 0;
  clw_fail_hard_on_error(clwh_mask_distance(ctx.get_handle(), &d));
  map.pull();
  return std::vector<uint32_t>(&map[0], &map[0] + map.size());
}

renderer::morph_summary renderer::morph_mask(struct ui_state &, int op, float radius) {
  const auto &size = volume->get_volume_size();
  if (region_mask.size() != 2 * ((size[0] + 63) / 64) * size[1] * size[2]) clw_fail_hard_on_error(CLWH_ERR_SIZE_MISMATCH);  // no mask
  morph_summary out;
  out.op = op;
  out.radius_sq = mask_radius_sq(radius);
  mask_weights(out.weight);
  clwh_morph_desc d{};
  d.mask_in = d.mask_out = region_mask.get_device_reference();
  for (int q = 0; q < 3; ++q) {
    d.dims[q] = (uint32_t)size[q];
    d.weight[q] = out.weight[q];
  }
  d.radius_sq = out.radius_sq;
  d.op = op;
  clw_fail_hard_on_error(clwh_mask_morph(ctx.get_handle(), &d));
  region_mask.pull();  // (padding is clean: every set bit is a voxel)
  for (size_t i = 0; i < region_mask.size(); ++i) out.count += (uint64_t)__builtin_popcount(region_mask[i]);
  return out;
}

renderer::thin_summary renderer::thin_mask(struct ui_state &, bool keep_ends, uint32_t max_iterations) {
  const auto &size = volume->get_volume_size();
  if (region_mask.size() != 2 * ((size[0] + 63) / 64) * size[1] * size[2]) clw_fail_hard_on_error(CLWH_ERR_SIZE_MISMATCH);  // no mask
  clwh_thin_result res{};
  clwh_thin_desc d{};
  d.mask_in = d.mask_out = region_mask.get_device_reference();
  for (int q = 0; q < 3; ++q) d.dims[q] = (uint32_t)size[q];
  d.flags = keep_ends ? CLWH_THIN_KEEP_ENDS : 0;
  d.max_iterations = max_iterations;
  d.result = &res;
  clw_fail_hard_on_error(clwh_mask_thin(ctx.get_handle(), &d));
  region_mask.pull();  // (the host's copy follows the device's, as after morph_mask)
  thin_summary out;
  out.count_in = res.count_in;
  out.count_out = res.count_out;
  out.deleted = res.deleted;
  out.iterations = res.iterations;
  return out;
}

std::vector<uint32_t> renderer::mask_points(struct ui_state &) {
  const auto &size = volume->get_volume_size();
  if (region_mask.size() != 2 * ((size[0] + 63) / 64) * size[1] * size[2]) clw_fail_hard_on_error(CLWH_ERR_SIZE_MISMATCH);  // no mask
  uint64_t n = 0;
  clwh_mask_points_desc d{};
  d.mask = region_mask.get_device_reference();
  for (int q = 0; q < 3; ++q) d.dims[q] = (uint32_t)size[q];
  d.n_points = &n;
  clw_fail_hard_on_error(clwh_mask_points(ctx.get_handle(), &d));  // the counting call
  if (n == 0) return {};
  clw_vector<uint32_t> points(ctx, std::vector<uint32_t>(4 * (size_t)n), false);
  d.points = points.get_device_reference();
  d.capacity = n;
  clw_fail_hard_on_error(clwh_mask_points(ctx.get_handle(), &d));
  points.pull();
  std::vector<uint32_t> out(4 * (size_t)n);
  for (size_t i = 0; i < out.size(); ++i) out[i] = points[i];
  return out;
}

void renderer::hold_mask(struct ui_state &) {
  const auto &size = volume->get_volume_size();
  if (region_mask.size() != 2 * ((size[0] + 63) / 64) * size[1] * size[2]) clw_fail_hard_on_error(CLWH_ERR_SIZE_MISMATCH);  // no mask
  if (held_mask.size() != region_mask.size()) held_mask = clw_vector<uint32_t>(ctx, std::vector<uint32_t>(region_mask.size()), false);
  clwh_mask_combine_desc d{};
  d.a = d.b = region_mask.get_device_reference();  // region AND region: the copy, with clean padding
  d.out = held_mask.get_device_reference();
  for (int q = 0; q < 3; ++q) d.dims[q] = (uint32_t)size[q];
  d.op = CLWH_MASK_AND;
  clw_fail_hard_on_error(clwh_mask_combine(ctx.get_handle(), &d));
}

void renderer::combine_masks(struct ui_state &, int op) {
  const auto &size = volume->get_volume_size();
  if (region_mask.size() != 2 * ((size[0] + 63) / 64) * size[1] * size[2]) clw_fail_hard_on_error(CLWH_ERR_SIZE_MISMATCH);  // no mask
  if (op != CLWH_MASK_NOT && held_mask.size() != region_mask.size()) clw_fail_hard_on_error(CLWH_ERR_SIZE_MISMATCH);   // nothing held
  clwh_mask_combine_desc d{};
  d.a = d.out = region_mask.get_device_reference();
  d.b = op != CLWH_MASK_NOT ? held_mask.get_device_reference() : nullptr;
  for (int q = 0; q < 3; ++q) d.dims[q] = (uint32_t)size[q];
  d.op = op;
  clw_fail_hard_on_error(clwh_mask_combine(ctx.get_handle(), &d));
}

void renderer::geodesic_weights(uint32_t face[3], uint32_t edge[3], uint32_t *corner) const {
  const auto &sizes = volume->get_voxel_sizes();
  double s[3];
  for (int q = 0; q < 3; ++q) s[q] = (double)sizes[q] * 16.0;
  const auto cost = [](double length) { return (uint32_t)std::min(65535.0, std::max(1.0, std::nearbyint(length))); };
  for (int q = 0; q < 3; ++q) {
    face[q] = cost(s[q]);
    edge[q] = cost(std::sqrt(s[(q + 1) % 3] * s[(q + 1) % 3] + s[(q + 2) % 3] * s[(q + 2) % 3]));
  }
  *corner = cost(std::sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]));
}

renderer::geodesic_summary renderer::geodesic_map(struct ui_state &, const std::vector<uint32_t> &seeds, int flags, uint32_t cap) {
  const auto &size = volume->get_volume_size();
  const size_t voxels = (size_t)size[0] * size[1] * size[2];
  if (region_mask.size() != 2 * ((size[0] + 63) / 64) * size[1] * size[2]) clw_fail_hard_on_error(CLWH_ERR_SIZE_MISMATCH);  // no mask
  if (region_labels.size() != voxels) region_labels = clw_vector<uint32_t>(ctx, std::vector<uint32_t>(voxels), false);
  if (region_dist.size() != voxels) region_dist = clw_vector<uint32_t>(ctx, std::vector<uint32_t>(voxels), false);
  geodesic_summary out;
  clwh_geodesic_desc d{};
  d.domain = region_mask.get_device_reference();
  d.dist = region_dist.get_device_reference();
  d.labels = region_labels.get_device_reference();
  for (int q = 0; q < 3; ++q) d.dims[q] = (uint32_t)size[q];
  geodesic_weights(d.weight_face, d.weight_edge, &d.weight_corner);
  d.cap = cap;
  d.flags = flags & ~CLWH_GEO_FROM_LABELS;
  d.n_seeds = (uint32_t)(seeds.size() / 4);
  d.seeds = seeds.data();
  d.result = &out.result;
  clw_fail_hard_on_error(clwh_mask_geodesic(ctx.get_handle(), &d));
  region_dist.pull();
  out.dist.assign(&region_dist[0], &region_dist[0] + voxels);
  return out;
}

std::vector<uint32_t> renderer::trace_path(struct ui_state &, const uint32_t target[3], int flags) {
  const auto &size = volume->get_volume_size();
  const size_t voxels = (size_t)size[0] * size[1] * size[2];
  if (region_dist.size() != voxels || region_labels.size() != voxels) clw_fail_hard_on_error(CLWH_ERR_SIZE_MISMATCH);  // no map
  uint64_t n = 0;
  clwh_geodesic_trace_desc d{};
  d.dist = region_dist.get_device_reference();
  d.labels = region_labels.get_device_reference();
  for (int q = 0; q < 3; ++q) {
    d.dims[q] = (uint32_t)size[q];
    d.target[q] = target[q];
  }
  geodesic_weights(d.weight_face, d.weight_edge, &d.weight_corner);
  d.flags = flags & CLWH_GEO_26;
  d.n_points = &n;
  clw_fail_hard_on_error(clwh_geodesic_trace(ctx.get_handle(), &d));  // the count; then the points
  if (n == 0) return {};
  clw_vector<uint32_t> points(ctx, std::vector<uint32_t>((size_t)n * 3), false);
  d.points = points.get_device_reference();
  d.capacity = n;
  clw_fail_hard_on_error(clwh_geodesic_trace(ctx.get_handle(), &d));
  points.pull();
  return std::vector<uint32_t>(&points[0], &points[0] + points.size());
}

renderer::split_summary renderer::split_mask(struct ui_state &, float radius, int flags) {
  const auto &size = volume->get_volume_size();
  const size_t voxels = (size_t)size[0] * size[1] * size[2], mask_words = 2 * ((size[0] + 63) / 64) * size[1] * size[2];
  if (region_mask.size() != mask_words) clw_fail_hard_on_error(CLWH_ERR_SIZE_MISMATCH);  // no mask
  if (region_labels.size() != voxels) region_labels = clw_vector<uint32_t>(ctx, std::vector<uint32_t>(voxels), false);
  split_summary out;
  out.radius_sq = mask_radius_sq(radius);
  mask_weights(out.weight);
  clw_vector<uint32_t> eroded(ctx, std::vector<uint32_t>(mask_words), false);
  clwh_morph_desc m{};
  m.mask_in = region_mask.get_device_reference();
  m.mask_out = eroded.get_device_reference();
  for (int q = 0; q < 3; ++q) {
    m.dims[q] = (uint32_t)size[q];
    m.weight[q] = out.weight[q];
  }
  m.radius_sq = out.radius_sq;
  m.op = CLWH_MORPH_ERODE;
  clw_fail_hard_on_error(clwh_mask_morph(ctx.get_handle(), &m));
  // the pieces of the eroded mask alone: every value is inside the full window
  clwh_label_result pieces{};
  clwh_label_desc l{};
  l.volume = volume->get_reference_volume().get_device_reference();
  l.labels = region_labels.get_device_reference();
  l.mask = eroded.get_device_reference();
  l.lo = -32768;
  l.hi = 32767;
  l.flags = CLWH_LABEL_FROM_MASK | ((flags & CLWH_GEO_26) ? CLWH_LABEL_26 : 0);
  l.result = &pieces;
  clw_fail_hard_on_error(clwh_segment_label(ctx.get_handle(), &l));
  out.n_parts = pieces.n_components;
  if (out.n_parts == 0) return out;  // nothing survived: every label is 0
  clwh_geodesic_result grown{};
  clwh_geodesic_desc d{};
  d.domain = region_mask.get_device_reference();
  d.seed_labels = d.labels = region_labels.get_device_reference();  // in place
  for (int q = 0; q < 3; ++q) d.dims[q] = (uint32_t)size[q], d.weight_face[q] = d.weight_edge[q] = 1;
  d.weight_corner = 1;
  d.cap = CLWH_DIST_NONE;
  d.flags = CLWH_GEO_FROM_LABELS | (flags & CLWH_GEO_26);
  d.result = &grown;
  clw_fail_hard_on_error(clwh_mask_geodesic(ctx.get_handle(), &d));
  return out;
}

void renderer::cost_multipliers(uint32_t face[3], uint32_t edge[3], uint32_t *corner) const {
  const auto &sizes = volume->get_voxel_sizes();
  double s[3];
  for (int q = 0; q < 3; ++q) s[q] = (double)sizes[q] * 10.0;
  const auto mult = [](double length) {
    const double m = std::max(1.0, std::nearbyint(length));
    if (m > 255.0) clw_fail_hard_on_error(CLWH_ERR_INVALID_VALUE);  // voxels too unequal for a multiplier of 8 bits
    return (uint32_t)m;
  };
  for (int q = 0; q < 3; ++q) {
    face[q] = mult(s[q]);
    edge[q] = mult(std::sqrt(s[(q + 1) % 3] * s[(q + 1) % 3] + s[(q + 2) % 3] * s[(q + 2) % 3]));
  }
  *corner = mult(std::sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]));
}

std::vector<uint16_t> renderer::centerline_cost_table(uint32_t r_sq_max, uint32_t sharpness) {
  if (r_sq_max < 1 || r_sq_max > 65535 || sharpness > 65534) clw_fail_hard_on_error(CLWH_ERR_INVALID_VALUE);
  std::vector<uint16_t> table((size_t)r_sq_max + 1);
  const uint64_t r = r_sq_max;  // sharpness * r^2 < 2^48
  for (uint64_t d = 0; d <= r; ++d) table[d] = (uint16_t)(1 + ((uint64_t)sharpness * (r - d) * (r - d)) / (r * r));
  return table;
}

void renderer::cost_field(struct ui_state &, int source, const std::vector<uint16_t> &table, int64_t lo, uint32_t shift, bool masked) {
  const auto &size = volume->get_volume_size();
  const size_t voxels = (size_t)size[0] * size[1] * size[2];
  const bool have_mask = region_mask.size() == 2 * ((size[0] + 63) / 64) * size[1] * size[2];
  if ((masked || source == COST_FROM_DEPTH) && !have_mask) clw_fail_hard_on_error(CLWH_ERR_SIZE_MISMATCH);  // no mask
  if (region_cost.size() != voxels) region_cost = clw_vector<uint16_t>(ctx, std::vector<uint16_t>(voxels), false);
  clw_vector<uint32_t> depth(ctx, std::vector<uint32_t>(source == COST_FROM_DEPTH ? voxels : 1), false);
  clwh_cost_field_desc d{};
  if (source == COST_FROM_DEPTH) {
    clwh_distance_desc m{};
    m.mask = region_mask.get_device_reference();
    m.dist = depth.get_device_reference();
    for (int q = 0; q < 3; ++q) m.dims[q] = (uint32_t)size[q];
    mask_weights(m.weight);
    m.cap = CLWH_DIST_NONE;
    m.flags = CLWH_DIST_TO_CLEAR;
    clw_fail_hard_on_error(clwh_mask_distance(ctx.get_handle(), &m));
    d.source = depth.get_device_reference();
    d.kind = CLWH_COST_SRC_U32;
  } else {
    d.source = volume->get_reference_volume().get_device_reference();
    d.kind = source == COST_FROM_VALUE ? CLWH_COST_SRC_VALUE : CLWH_COST_SRC_GRADIENT;
  }
  d.domain = masked ? region_mask.get_device_reference() : nullptr;
  d.cost = region_cost.get_device_reference();
  d.table = table.data();
  d.lo = lo;
  for (int q = 0; q < 3; ++q) d.dims[q] = (uint32_t)size[q];
  d.n = (uint32_t)table.size();
  d.shift = shift;
  clw_fail_hard_on_error(clwh_cost_from_field(ctx.get_handle(), &d));
}

renderer::geodesic_summary renderer::cost_geodesic(struct ui_state &, const std::vector<uint32_t> &seeds, int flags, uint32_t cap) {
  const auto &size = volume->get_volume_size();
  const size_t voxels = (size_t)size[0] * size[1] * size[2];
  if (region_cost.size() != voxels) clw_fail_hard_on_error(CLWH_ERR_SIZE_MISMATCH);  // no cost
  if (region_labels.size() != voxels) region_labels = clw_vector<uint32_t>(ctx, std::vector<uint32_t>(voxels), false);
  if (region_dist.size() != voxels) region_dist = clw_vector<uint32_t>(ctx, std::vector<uint32_t>(voxels), false);
  geodesic_summary out;
  clwh_cost_geodesic_desc d{};
  d.cost = region_cost.get_device_reference();
  d.dist = region_dist.get_device_reference();
  d.labels = region_labels.get_device_reference();
  for (int q = 0; q < 3; ++q) d.dims[q] = (uint32_t)size[q];
  cost_multipliers(d.mult_face, d.mult_edge, &d.mult_corner);
  d.cap = cap;
  d.flags = flags & ~CLWH_GEO_FROM_LABELS;
  d.n_seeds = (uint32_t)(seeds.size() / 4);
  d.seeds = seeds.data();
  d.result = &out.result;
  clw_fail_hard_on_error(clwh_cost_geodesic(ctx.get_handle(), &d));
  region_dist.pull();
  out.dist.assign(&region_dist[0], &region_dist[0] + voxels);
  return out;
}

std::vector<uint16_t> renderer::watershed_gradient_table(uint32_t g_max, uint32_t *shift) {
  if (g_max < 1 || g_max > 2u * 65535u) clw_fail_hard_on_error(CLWH_ERR_INVALID_VALUE);
  const uint64_t g_sq = (uint64_t)g_max * g_max;
  uint32_t s = 0;
  while ((g_sq >> s) >= 65536u) ++s;
  std::vector<uint16_t> table((size_t)(g_sq >> s) + 1);
  uint64_t root = 0;  // isqrt(i << s), which never falls as i grows
  for (uint64_t i = 0; i < table.size(); ++i) {
    while ((root + 1) * (root + 1) <= (i << s)) ++root;
    table[i] = (uint16_t)(1 + std::min<uint64_t>(65534, root));
  }
  *shift = s;
  return table;
}

renderer::watershed_summary renderer::watershed(struct ui_state &, const std::vector<uint32_t> &seeds, int flags, uint32_t plateau_cap,
                                                uint32_t level_cap, bool pull_labels) {
  const auto &size = volume->get_volume_size();
  const size_t voxels = (size_t)size[0] * size[1] * size[2];
  if (region_cost.size() != voxels) clw_fail_hard_on_error(CLWH_ERR_SIZE_MISMATCH);  // no cost
  if (region_labels.size() != voxels) region_labels = clw_vector<uint32_t>(ctx, std::vector<uint32_t>(voxels), false);
  if (region_dist.size() != voxels) region_dist = clw_vector<uint32_t>(ctx, std::vector<uint32_t>(voxels), false);
  watershed_summary out;
  clwh_watershed_desc d{};
  d.cost = region_cost.get_device_reference();
  d.level = region_dist.get_device_reference();
  d.labels = region_labels.get_device_reference();
  for (int q = 0; q < 3; ++q) d.dims[q] = (uint32_t)size[q];
  d.plateau_cap = plateau_cap;
  d.level_cap = level_cap;
  d.flags = flags & ~CLWH_GEO_FROM_LABELS;
  d.n_seeds = (uint32_t)(seeds.size() / 4);
  d.seeds = seeds.data();
  d.result = &out.result;
  clw_fail_hard_on_error(clwh_watershed(ctx.get_handle(), &d));
  region_dist.pull();
  out.level.assign(&region_dist[0], &region_dist[0] + voxels);
  if (pull_labels) {
    region_labels.pull();
    out.labels.assign(&region_labels[0], &region_labels[0] + voxels);
  }
  return out;
}

renderer::watershed_summary renderer::watershed_edges(struct ui_state &state, const std::vector<uint32_t> &seeds, int flags, uint32_t g_max,
                                                      uint32_t plateau_cap, bool pull_labels) {
  uint32_t shift = 0;
  const std::vector<uint16_t> table = watershed_gradient_table(g_max, &shift);
  cost_field(state, COST_FROM_GRADIENT, table, 0, shift, false);
  return watershed(state, seeds, flags, plateau_cap, CLWH_WATERSHED_LEVEL_MAX, pull_labels);
}

std::vector<uint32_t> renderer::trace_cost_path(struct ui_state &, const uint32_t target[3], int flags) {
  const auto &size = volume->get_volume_size();
  const size_t voxels = (size_t)size[0] * size[1] * size[2];
  if (region_cost.size() != voxels || region_dist.size() != voxels || region_labels.size() != voxels)
    clw_fail_hard_on_error(CLWH_ERR_SIZE_MISMATCH);  // no map
  uint64_t n = 0;
  clwh_cost_trace_desc d{};
  d.cost = region_cost.get_device_reference();
  d.dist = region_dist.get_device_reference();
  d.labels = region_labels.get_device_reference();
  for (int q = 0; q < 3; ++q) {
    d.dims[q] = (uint32_t)size[q];
    d.target[q] = target[q];
  }
  cost_multipliers(d.mult_face, d.mult_edge, &d.mult_corner);
  d.flags = flags & CLWH_GEO_26;
  d.n_points = &n;
  clw_fail_hard_on_error(clwh_cost_trace(ctx.get_handle(), &d));  // the count; then the points
  if (n == 0) return {};
  clw_vector<uint32_t> points(ctx, std::vector<uint32_t>((size_t)n * 3), false);
  d.points = points.get_device_reference();
  d.capacity = n;
  clw_fail_hard_on_error(clwh_cost_trace(ctx.get_handle(), &d));
  points.pull();
  return std::vector<uint32_t>(&points[0], &points[0] + points.size());
}

std::vector<uint32_t> renderer::centerline(struct ui_state &state, const uint32_t start[3], const uint32_t end[3], int flags, float max_radius,
                                           uint32_t sharpness) {
  const auto &size = volume->get_volume_size();
  for (int q = 0; q < 3; ++q)
    if (start[q] >= size[q] || end[q] >= size[q]) clw_fail_hard_on_error(CLWH_ERR_INVALID_VALUE);
  uint32_t r_sq_max = 1;
  if (max_radius > 0.0f) {
    r_sq_max = std::max(1u, mask_radius_sq(max_radius));
  } else {  // the deepest voxel of the region, on the host
    const std::vector<uint32_t> depth = distance_map(state, true);
    region_mask.pull();
    const size_t words_per_row = 2 * ((size[0] + 63) / 64);
    for (size_t row = 0; row < (size_t)size[1] * size[2]; ++row)
      for (size_t x = 0; x < size[0]; ++x)
        if (((region_mask[row * words_per_row + (x >> 5)] >> (x & 31)) & 1u) && depth[row * size[0] + x] != CLWH_DIST_NONE)
          r_sq_max = std::max(r_sq_max, depth[row * size[0] + x]);
  }
  uint32_t shift = 0;  // scene.centerline_shift: the depths within the table's 65535
  while ((r_sq_max >> shift) > 65535u) ++shift;
  cost_field(state, COST_FROM_DEPTH, centerline_cost_table(r_sq_max >> shift, sharpness), 0, shift, true);
  cost_geodesic(state, {start[0], start[1], start[2], 1u}, flags & (CLWH_GEO_26 | CLWH_GEO_DENSE));
  return trace_cost_path(state, end, flags);
}

clwh_mask_stats_result renderer::measure_mask(struct ui_state &, int hist_lo, int bin_width, int n_bins, std::vector<uint64_t> *hist) {
  const auto &size = volume->get_volume_size();
  if (region_mask.size() != 2 * ((size[0] + 63) / 64) * size[1] * size[2]) clw_fail_hard_on_error(CLWH_ERR_SIZE_MISMATCH);  // no mask
  const bool with_hist = n_bins > 0 && hist != nullptr;
  clw_vector<uint32_t> bins(ctx, std::vector<uint32_t>(with_hist ? 2 * (size_t)n_bins : 2), false);  // uint64 words, as pairs
  clwh_mask_stats_result result{};
  clwh_mask_stats_desc d{};
  d.volume = volume->get_reference_volume().get_device_reference();
  d.mask = region_mask.get_device_reference();
  if (with_hist) {
    d.hist = bins.get_device_reference();
    d.hist_lo = hist_lo;
    d.bin_width = bin_width;
    d.n_bins = n_bins;
  }
  d.result = &result;
  clw_fail_hard_on_error(clwh_mask_statistics(ctx.get_handle(), &d));
  if (with_hist) {
    bins.pull();
    hist->resize((size_t)n_bins);
    std::memcpy(hist->data(), &bins[0], (size_t)n_bins * sizeof(uint64_t));
  }
  return result;
}

std::vector<clwh_region_stats> renderer::measure_labels(struct ui_state &, unsigned capacity) {
  const auto &size = volume->get_volume_size();
  if (region_labels.size() != (size_t)size[0] * size[1] * size[2]) clw_fail_hard_on_error(CLWH_ERR_SIZE_MISMATCH);  // nothing was labelled
  constexpr size_t record_words = sizeof(clwh_region_stats) / sizeof(uint32_t);
  clw_vector<uint32_t> table(ctx, std::vector<uint32_t>(std::max<size_t>(capacity, 1) * record_words), false);
  clwh_label_stats_desc d{};
  d.volume = volume->get_reference_volume().get_device_reference();
  d.labels = region_labels.get_device_reference();
  d.stats = table.get_device_reference();
  d.capacity = capacity;
  clw_fail_hard_on_error(clwh_label_statistics(ctx.get_handle(), &d));
  table.pull();  // (waits for the stream)
  std::vector<clwh_region_stats> out(capacity);
  if (capacity) std::memcpy(out.data(), &table[0], (size_t)capacity * sizeof(clwh_region_stats));
  return out;
}

// (the host is little-endian, like every target of the library: the arrays go out as they lie in memory)
bool write_ply(const std::string &path, const mesh_data &mesh) {
  const size_t nv = mesh.positions.size() / 3, nt = mesh.triangles.size() / 3;
  if (mesh.normals.size() != mesh.positions.size()) return false;
  std::ofstream f(path, std::ios::binary);
  f << "ply\nformat binary_little_endian 1.0\nelement vertex " << nv
    << "\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\nelement face " << nt
    << "\nproperty list uchar uint vertex_indices\nend_header\n";
  std::vector<char> body(nv * 24 + nt * 13);
  for (size_t i = 0; i < nv; ++i) {
    std::memcpy(&body[i * 24], &mesh.positions[i * 3], 12);
    std::memcpy(&body[i * 24 + 12], &mesh.normals[i * 3], 12);
  }
  for (size_t i = 0; i < nt; ++i) {
    body[nv * 24 + i * 13] = 3;
    std::memcpy(&body[nv * 24 + i * 13 + 1], &mesh.triangles[i * 3], 12);
  }
  f.write(body.data(), (std::streamsize)body.size());
  f.flush();
  return f.good();
}

// reference :45-124 -- the 2-D (value, |gradient|) histogram texture of the transfer-function editor:
// bin the volume, quantise the counts on the host so that small counts stay distinguishable, rank the
// distinct counts, colour each bin by its rank.  (The reference declares render_tf(width, height) and
// defines render_tf(height, width); both call sites pass 500 x 500.)
void *renderer::render_tf(const unsigned int height, const unsigned int width) {
  tfframe = clw_image<unsigned char, 4>(ctx, std::vector<unsigned char>((size_t)height * width * 4), {width, height, 1});

  clw_vector<unsigned int> bins(ctx, std::vector<unsigned int>((size_t)width * height, 0));
  bins.push();
  const Volume_Stats stats = volume->get_volume_stats();
  clw_function sort_values(ctx, "histogram.cl", "tf_sort_values");
  sort_values.execute(volume->get_volume_size_evenness(8), {4, 4, 4}, volume->get_reference_volume(), bins, width, height,
                      stats.min_v, stats.max_v, stats.min_g, stats.max_g);
  bins.pull();

  // round every count down to its two leading decimal digits and collect the distinct results
  std::set<int> distinct;
  for (size_t i = 0; i < bins.size(); ++i) {
    const int value = (int)bins[i];
    if (value == 0) continue;
    const int unit = std::max((int)std::pow(10, std::floor(std::log10(value)) - 1), 1);
    const int corrected = (int)(std::floor(value / unit) * unit);
    bins[i] = (unsigned int)corrected;
    distinct.insert(corrected);
  }
  bins.push();

  if (distinct.empty()) {
    std::cout << "Warning, histogram does not contain non-zero entries.\n";
  } else {
    clw_vector<int> ranks(ctx, std::vector<int>(distinct.begin(), distinct.end()));
    ranks.push();
    clw_function flush_colors(ctx, "histogram.cl", "tf_flush_color_frame");
    flush_colors.execute({evenness((unsigned)tfframe.get_dimensions()[0], 16), evenness((unsigned)tfframe.get_dimensions()[1], 16), 1},
                         {16, 16, 1}, tfframe, bins, ranks, (int)ranks.size());
  }
  tfframe.pull();
  return &tfframe[0];
}
