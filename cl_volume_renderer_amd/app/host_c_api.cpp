// host_c_api.cpp -- a small extern "C" facade over the C++ host mirror (renderer, reference_volume,
// env_map, signed_distance_field) so that pytest can drive the very call sequence the SDL/ImGui
// application performs (reference app/ui.cpp:170-199, 296) without SDL.  Test / tooling entry points;
// the product ABI is include/clwh.h.
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "hdre_loader.hpp"
#include "nrrd_loader.hpp"
#include "renderer.hpp"
#include "tf_part.hpp"

struct clvr_host {
  clw_context ctx;
  renderer rend;
  std::unique_ptr<volume_block> block;
  std::unique_ptr<reference_volume> rv;
  std::unique_ptr<env_map> emap;
  ui_state state;
  mesh_data mesh;  // of the last clvr_host_extract_mesh
  clvr_host() : rend(ctx), state{"", true, 0, 0, Position3D(0, 0, 0), {0.f, 0.f}, true} {}
};

extern "C" {

clvr_host *clvr_host_create(void) { return new clvr_host(); }
void clvr_host_destroy(clvr_host *h) { delete h; }

// nrrd_loader::load_file + reference_volume + hdre_loader + env_map + image_set  (ui.cpp:182-194)
void clvr_host_load(clvr_host *h, const short *voxels, unsigned X, unsigned Y, unsigned Z, const unsigned char *env_rgba,
                    unsigned env_w, unsigned env_h) {
  h->rv.reset();  // release the old device images before allocating the new ones
  h->block.reset(new volume_block(std::vector<short>(voxels, voxels + (size_t)X * Y * Z), X, Y, Z, 1.f, 1.f, 1.f));
  h->rv.reset(new reference_volume(h->ctx, h->block.get()));
  h->rv->set_value_clip({-2000, 3000});
  h->rv->set_gradient_clip({0, 4000});
  image em;
  em.m_pixels.assign(env_rgba, env_rgba + (size_t)env_w * env_h * 4);
  em.m_width = env_w;
  em.m_height = env_h;
  h->emap.reset(new env_map(h->ctx, em));
  h->rend.image_set(h->rv.get(), h->emap.get());
}

// flush_tf + flush_changes  (ui.cpp:195-197)
void clvr_host_flush(clvr_host *h, const char *cl_code) {
  h->rend.next_event_code_set(cl_code);
  h->rend.flush_changes();
}

// one iteration of the ui::run loop body that matters here (ui.cpp:296)
const void *clvr_host_render_frame(clvr_host *h, const float pos[3], const float look[2], int width, int height,
                                   int cam_changed, int *frame_changed) {
  h->state.position = Position3D(pos[0], pos[1], pos[2]);
  h->state.direction_look[0] = look[0];
  h->state.direction_look[1] = look[1];
  h->state.width = width;
  h->state.height = height;
  h->state.cam_changed = cam_changed != 0;
  bool changed = false;
  void *p = h->rend.render_frame(h->state, changed);
  if (frame_changed) *frame_changed = changed ? 1 : 0;
  return p;
}

// the same iteration with the display hand-off instead of the readback: the frame goes into `device_frame`
// (frame_w x frame_h RGBA8 device memory of the caller, read on `stream`), `passes` seeds in one launch
void clvr_host_render_frame_device(clvr_host *h, const float pos[3], const float look[2], int width, int height,
                                   int cam_changed, void *device_frame, unsigned frame_w, unsigned frame_h, void *stream,
                                   int passes) {
  h->state.position = Position3D(pos[0], pos[1], pos[2]);
  h->state.direction_look[0] = look[0];
  h->state.direction_look[1] = look[1];
  h->state.width = width;
  h->state.height = height;
  h->state.cam_changed = cam_changed != 0;
  h->state.path_changed = true;
  clw_foreign_memory target(h->ctx, device_frame, frame_w, frame_h, stream);
  h->rend.render_frame_device(h->state, target, passes);
}

// renderer::render_projection from the same camera arguments as clvr_host_render_frame: the RGBA8 frame (SCREEN_WIDTH x SCREEN_HEIGHT)
const void *clvr_host_render_projection(clvr_host *h, const float pos[3], const float look[2], int width, int height, int mode,
                                        float center, float window_width, float step) {
  h->state.position = Position3D(pos[0], pos[1], pos[2]);
  h->state.direction_look[0] = look[0];
  h->state.direction_look[1] = look[1];
  h->state.width = width;
  h->state.height = height;
  return h->rend.render_projection(h->state, mode, center, window_width, step);
}

// renderer::render_composite from the same camera arguments: lut = float32[lut_len][4]; the RGBA8 frame (SCREEN_WIDTH x SCREEN_HEIGHT)
const void *clvr_host_render_composite(clvr_host *h, const float pos[3], const float look[2], int width, int height, const float *lut,
                                       int lut_first, int lut_len, float step, float alpha_stop, int flags, float ambient) {
  h->state.position = Position3D(pos[0], pos[1], pos[2]);
  h->state.direction_look[0] = look[0];
  h->state.direction_look[1] = look[1];
  h->state.width = width;
  h->state.height = height;
  const std::vector<float> table(lut, lut + (size_t)(lut_len > 0 ? lut_len : 0) * 4);
  return h->rend.render_composite(h->state, table, lut_first, lut_len, step, alpha_stop, flags, ambient);
}
// renderer::render_isosurface from the same camera arguments: color = float[3]; the RGBA8 frame (SCREEN_WIDTH x SCREEN_HEIGHT)
const void *clvr_host_render_isosurface(clvr_host *h, const float pos[3], const float look[2], int width, int height, float iso,
                                        int flags, float step, int refine, float ambient, const float color[3]) {
  h->state.position = Position3D(pos[0], pos[1], pos[2]);
  h->state.direction_look[0] = look[0];
  h->state.direction_look[1] = look[1];
  h->state.width = width;
  h->state.height = height;
  return h->rend.render_isosurface(h->state, iso, flags, step, refine, ambient, color[0], color[1], color[2]);
}
// renderer::render_slice for a region of width x height pixels (no camera): orientation 0 axial, 1 coronal, 2 sagittal; the RGBA8
// frame (SCREEN_WIDTH x SCREEN_HEIGHT)
const void *clvr_host_render_slice(clvr_host *h, int width, int height, int orientation, float position, int mode, int slab_samples,
                                   float step, float center, float window_width, int flags) {
  h->state.width = width;
  h->state.height = height;
  return h->rend.render_slice(h->state, orientation, position, mode, slab_samples, step, center, window_width, flags);
}
// renderer::extract_mesh: the counts, and pointers to the host's copy of the arrays (float[n][3], float[n][3], uint64[n], uint32[m][3]),
// valid until the next call or clvr_host_destroy
void clvr_host_extract_mesh(clvr_host *h, float iso, int flags, unsigned long long *n_vertices, unsigned long long *n_triangles,
                            const float **positions, const float **normals, const unsigned long long **keys, const unsigned **triangles) {
  h->mesh = h->rend.extract_mesh(h->state, iso, flags);
  *n_vertices = h->mesh.keys.size();
  *n_triangles = h->mesh.triangles.size() / 3;
  *positions = h->mesh.positions.data();
  *normals = h->mesh.normals.data();
  *keys = reinterpret_cast<const unsigned long long *>(h->mesh.keys.data());
  *triangles = h->mesh.triangles.data();
}
// write_ply of that mesh; 1 on success
int clvr_host_write_mesh_ply(clvr_host *h, const char *path) { return write_ply(path, h->mesh) ? 1 : 0; }
// renderer::grow_region from n_seeds (x, y, z) triples: the statistics go to *result (a clwh_grow_result); the mask stays on the device
void clvr_host_grow_region(clvr_host *h, const unsigned *seeds, unsigned n_seeds, int lo, int hi, int flags, void *result) {
  const std::vector<uint32_t> list(seeds, seeds + (size_t)n_seeds * 3);
  const clwh_grow_result r = h->rend.grow_region(h->state, list, lo, hi, flags);
  std::memcpy(result, &r, sizeof r);
}
// renderer::apply_mask: the last grown mask applied to the renderer's volume in place
void clvr_host_apply_mask(clvr_host *h, int fill, int flags) { h->rend.apply_mask(h->state, fill, flags); }
// renderer::filter_volume: the renderer's volume filtered in place; kind = clwh_filter_kind, SMOOTH with renderer::gaussian_weights of
// sigma_mm and the volume's voxel sizes (its radii are returned in radius), masked != 0: only inside the last mask.  With `out` the
// device's volume is read back into it (X * Y * Z shorts)
void clvr_host_filter_volume(clvr_host *h, int kind, unsigned radius[3], double sigma_mm, int masked, short *out) {
  if (kind == CLWH_FILTER_SMOOTH) {
    const auto &sizes = h->rv->get_voxel_sizes();
    const double spacing[3] = {(double)sizes[0], (double)sizes[1], (double)sizes[2]};
    const std::array<std::vector<uint16_t>, 3> w = renderer::gaussian_weights(sigma_mm, spacing);
    for (int q = 0; q < 3; ++q) radius[q] = (unsigned)w[q].size() - 1u;
    h->rend.filter_volume(h->state, kind, radius, &w, masked != 0);
  } else {
    h->rend.filter_volume(h->state, kind, radius, nullptr, masked != 0);
  }
  if (out) {
    clwh_mem *m = h->rv->get_reference_volume().get_device_reference();
    const auto &size = h->rv->get_volume_size();
    clw_fail_hard_on_error(clwh_mem_pull(h->ctx.get_handle(), m, out, size[0] * size[1] * size[2] * sizeof(short)));
  }
}
// renderer::label_components: *n_components and *n_voxels, and up to top_k records (clwh_label_component, 48 bytes each) into
// `records`; returns how many were written.  The labels stay on the device
unsigned clvr_host_label_components(clvr_host *h, int lo, int hi, int flags, unsigned top_k, unsigned long long *n_components,
                                    unsigned long long *n_voxels, void *records) {
  const renderer::component_summary s = h->rend.label_components(h->state, lo, hi, flags, top_k);
  *n_components = s.n_components;
  *n_voxels = s.n_voxels;
  if (!s.top.empty()) std::memcpy(records, s.top.data(), s.top.size() * sizeof(clwh_label_component));
  return (unsigned)s.top.size();
}
// renderer::select_components: ranks rank_lo .. rank_hi of the last labelling become the mask clvr_host_apply_mask applies
void clvr_host_select_components(clvr_host *h, unsigned rank_lo, unsigned rank_hi) { h->rend.select_components(h->state, rank_lo, rank_hi); }
// the voxel sizes relative to x that renderer::mask_weights reads (clvr_host_load sets 1, 1, 1)
void clvr_host_set_voxel_sizes(clvr_host *h, const float sizes[3]) { h->rv->set_voxel_sizes({sizes[0], sizes[1], sizes[2]}); }
// renderer::distance_map of the region mask into out[Z][Y][X]
void clvr_host_distance_map(clvr_host *h, int to_clear, unsigned cap, unsigned *out) {
  const std::vector<uint32_t> map = h->rend.distance_map(h->state, to_clear != 0, cap);
  std::memcpy(out, map.data(), map.size() * sizeof(uint32_t));
}
// renderer::morph_mask: the region mask morphed in place by a ball of `radius` x-voxels; out = {radius_sq, wx, wy, wz}; returns the
// new region's voxel count
unsigned long long clvr_host_morph_mask(clvr_host *h, int op, float radius, unsigned out[4]) {
  const renderer::morph_summary s = h->rend.morph_mask(h->state, op, radius);
  out[0] = s.radius_sq;
  for (int q = 0; q < 3; ++q) out[1 + q] = s.weight[q];
  return s.count;
}
// renderer::hold_mask / combine_masks: region = region op held
void clvr_host_hold_mask(clvr_host *h) { h->rend.hold_mask(h->state); }
void clvr_host_combine_masks(clvr_host *h, int op) { h->rend.combine_masks(h->state, op); }
// renderer::thin_mask: the region mask thinned in place; result = {count_in, count_out, deleted, iterations}
void clvr_host_thin_mask(clvr_host *h, int keep_ends, unsigned max_iterations, unsigned long long result[4]) {
  const renderer::thin_summary s = h->rend.thin_mask(h->state, keep_ends != 0, max_iterations);
  result[0] = s.count_in;
  result[1] = s.count_out;
  result[2] = s.deleted;
  result[3] = s.iterations;
}
// renderer::mask_points of the region mask: returns the number of points, and writes the first min(n, capacity) (x, y, z, n26)
// quadruples to out (NULL with capacity 0: the count alone)
unsigned long long clvr_host_mask_points(clvr_host *h, unsigned *out, unsigned long long capacity) {
  const std::vector<uint32_t> p = h->rend.mask_points(h->state);
  const size_t n = p.size() / 4u, take = n < capacity ? n : (size_t)capacity;
  if (out && take) std::memcpy(out, p.data(), take * 4u * sizeof(uint32_t));
  return n;
}
// renderer::geodesic_map of the region mask from n_seeds (x, y, z, id) quadruples into out[Z][Y][X]; result = {reached, max_dist}
void clvr_host_geodesic_map(clvr_host *h, const unsigned *seeds, unsigned n_seeds, int flags, unsigned cap, unsigned *out,
                            unsigned long long result[2]) {
  const renderer::geodesic_summary s = h->rend.geodesic_map(h->state, std::vector<uint32_t>(seeds, seeds + 4u * n_seeds), flags, cap);
  std::memcpy(out, s.dist.data(), s.dist.size() * sizeof(uint32_t));
  result[0] = s.result.reached;
  result[1] = s.result.max_dist;
}
// renderer::trace_path from `target` over the last geodesic map: up to `capacity` (x, y, z) triples into out; returns the true count
unsigned long long clvr_host_trace_path(clvr_host *h, const unsigned target[3], int flags, unsigned *out, unsigned long long capacity) {
  const std::vector<uint32_t> points = h->rend.trace_path(h->state, target, flags);
  std::memcpy(out, points.data(), std::min<size_t>(points.size(), (size_t)capacity * 3) * sizeof(uint32_t));
  return points.size() / 3;
}
// renderer::centerline from `start` to `end` inside the region mask: up to `capacity` (x, y, z) triples into out, `end` first; returns
// the true count
unsigned long long clvr_host_centerline(clvr_host *h, const unsigned start[3], const unsigned end[3], int flags, float max_radius,
                                        unsigned sharpness, unsigned *out, unsigned long long capacity) {
  const std::vector<uint32_t> points = h->rend.centerline(h->state, start, end, flags, max_radius, sharpness);
  std::memcpy(out, points.data(), std::min<size_t>(points.size(), (size_t)capacity * 3) * sizeof(uint32_t));
  return points.size() / 3;
}
// renderer::watershed_gradient_table: up to `capacity` entries into out and the shift that goes with them; returns the table's length
unsigned clvr_host_watershed_table(unsigned g_max, unsigned short *out, unsigned capacity, unsigned *shift) {
  const std::vector<uint16_t> table = renderer::watershed_gradient_table(g_max, shift);
  std::memcpy(out, table.data(), std::min<size_t>(table.size(), capacity) * sizeof(uint16_t));
  return (unsigned)table.size();
}
// renderer::watershed_edges from n_seeds (x, y, z, id) quadruples: labels[Z][Y][X] and level[Z][Y][X] (either may be null), *max_level;
// returns the voxels reached
unsigned long long clvr_host_watershed_edges(clvr_host *h, const unsigned *seeds, unsigned n_seeds, int flags, unsigned g_max, unsigned plateau_cap,
                                             unsigned *labels, unsigned *level, unsigned *max_level) {
  const renderer::watershed_summary s =
      h->rend.watershed_edges(h->state, std::vector<uint32_t>(seeds, seeds + 4u * n_seeds), flags, g_max, plateau_cap, labels != nullptr);
  if (labels) std::memcpy(labels, s.labels.data(), s.labels.size() * sizeof(uint32_t));
  if (level) std::memcpy(level, s.level.data(), s.level.size() * sizeof(uint32_t));
  *max_level = s.result.max_level;
  return s.result.reached;
}

// renderer::curve_frames of n_points (x, y, z) triples of doubles: up to `capacity` rows of nine floats into rows_out and as many
// stations' s_mm as fit `capacity` into s_out (either may be null); *n_out = the stations; returns the rows (n rounded up to 8)
unsigned long long clvr_host_curve_frames(const double *points, unsigned long long n_points, const double spacing[3], int width, double pixel_mm,
                                          double station_mm, int smooth_passes, double angle, int slab_samples, double step_mm, float *rows_out,
                                          double *s_out, unsigned long long capacity, unsigned long long *n_out) {
  const renderer::curve_frame_set f = renderer::curve_frames(std::vector<double>(points, points + 3 * n_points), spacing, width, pixel_mm,
                                                             station_mm, smooth_passes, angle, slab_samples, step_mm);
  const size_t H = f.rows.size() / 9;
  if (rows_out) std::memcpy(rows_out, f.rows.data(), std::min<size_t>(H, (size_t)capacity) * 9 * sizeof(float));
  if (s_out) std::memcpy(s_out, f.s_mm.data(), std::min<size_t>(f.n, (size_t)capacity) * sizeof(double));
  *n_out = f.n;
  return H;
}
// renderer::render_curved along n_points (x, y, z) voxels with curve_frames' rows (the volume's voxel sizes as mm, station_mm =
// pixel_mm, step_mm = step): the RGBA8 frame (SCREEN_WIDTH x SCREEN_HEIGHT), the reformat in its first `width` columns
const void *clvr_host_render_curved(clvr_host *h, const unsigned *points, unsigned long long n_points, int width, double pixel_mm, int mode,
                                    int slab_samples, float step, float center, float window_width, int flags) {
  const auto &sizes = h->rv->get_voxel_sizes();
  const double spacing[3] = {(double)sizes[0], (double)sizes[1], (double)sizes[2]};
  const renderer::curve_frame_set f = renderer::curve_frames(std::vector<double>(points, points + 3 * n_points), spacing, width, pixel_mm, pixel_mm,
                                                             8, 0.0, slab_samples, (double)step);
  return h->rend.render_curved(h->state, f, width, mode, slab_samples, step, center, window_width, flags);
}
// renderer::vessel_profile of the region mask along n_points (x, y, z) voxels: up to `capacity` records (16 bytes each), areas and
// diameters; returns the stations
unsigned long long clvr_host_vessel_profile(clvr_host *h, const unsigned *points, unsigned long long n_points, double pixel_mm, int window,
                                            int connected, void *records, double *area_mm2, double *diameter_mm, unsigned long long capacity) {
  const renderer::profile_summary s = h->rend.vessel_profile(h->state, std::vector<uint32_t>(points, points + 3 * n_points), pixel_mm, window, connected != 0);
  const size_t k = std::min<size_t>(s.records.size(), (size_t)capacity);
  std::memcpy(records, s.records.data(), k * sizeof(clwh_section_record));
  std::memcpy(area_mm2, s.area_mm2.data(), k * sizeof(double));
  std::memcpy(diameter_mm, s.diameter_mm.data(), k * sizeof(double));
  return s.records.size();
}

// renderer::split_mask: the region split into parts that become the labelling; out = {radius_sq, wx, wy, wz}; returns the number of parts
unsigned long long clvr_host_split_mask(clvr_host *h, float radius, int flags, unsigned out[4]) {
  const renderer::split_summary s = h->rend.split_mask(h->state, radius, flags);
  out[0] = s.radius_sq;
  for (int q = 0; q < 3; ++q) out[1 + q] = s.weight[q];
  return s.n_parts;
}
// renderer::measure_mask: the region mask's record into *out (a clwh_mask_stats_result, 120 bytes); n_bins > 0: its histogram into hist
void clvr_host_measure_mask(clvr_host *h, int hist_lo, int bin_width, int n_bins, unsigned long long *hist, void *out) {
  std::vector<uint64_t> bins;
  const clwh_mask_stats_result r = h->rend.measure_mask(h->state, hist_lo, bin_width, n_bins, n_bins > 0 ? &bins : nullptr);
  if (n_bins > 0) std::memcpy(hist, bins.data(), bins.size() * sizeof(uint64_t));
  std::memcpy(out, &r, sizeof r);
}
// renderer::measure_labels: the records of ranks 1 .. capacity of the last labelling into out (104 bytes each)
void clvr_host_measure_labels(clvr_host *h, unsigned capacity, void *out) {
  const std::vector<clwh_region_stats> table = h->rend.measure_labels(h->state, capacity);
  std::memcpy(out, table.data(), table.size() * sizeof(clwh_region_stats));
}
// renderer::overlay_slice over the frame clvr_host_render_slice wrote, with the same region and plane: source 0 the region mask, 1 the
// held mask, 2 the last labelling; the RGBA8 frame (SCREEN_WIDTH x SCREEN_HEIGHT)
const void *clvr_host_overlay_slice(clvr_host *h, int width, int height, int source, int orientation, float position, int slab_samples,
                                    float step, int flags, unsigned fill_alpha, unsigned outline_alpha, unsigned id_lo, unsigned id_hi) {
  h->state.width = width;
  h->state.height = height;
  renderer::overlay_style style;
  style.flags = flags;
  style.fill_alpha = fill_alpha;
  style.outline_alpha = outline_alpha;
  style.id_lo = id_lo;
  style.id_hi = id_hi;
  return h->rend.overlay_slice(h->state, source, orientation, position, slab_samples, step, style);
}
// renderer::overlay_camera over the frame a camera view wrote, from the same camera arguments as clvr_host_render_projection
const void *clvr_host_overlay_camera(clvr_host *h, const float pos[3], const float look[2], int width, int height, int source, float step,
                                     int flags, unsigned fill_alpha, unsigned outline_alpha, unsigned id_lo, unsigned id_hi) {
  h->state.position = Position3D(pos[0], pos[1], pos[2]);
  h->state.direction_look[0] = look[0];
  h->state.direction_look[1] = look[1];
  h->state.width = width;
  h->state.height = height;
  renderer::overlay_style style;
  style.flags = flags;
  style.fill_alpha = fill_alpha;
  style.outline_alpha = outline_alpha;
  style.id_lo = id_lo;
  style.id_hi = id_hi;
  return h->rend.overlay_camera(h->state, source, step, style);
}
// tf_composite_lut for a list of rectangles {min_v, max_v, min_g, max_g, r, g, b, a} into out[lut_len][4] (no device involved)
void clvr_host_tf_composite_lut(const float *rects, int n, int lut_first, int lut_len, float opacity, float *out) {
  std::vector<tf_selection *> sel;
  for (int i = 0; i < n; ++i) {
    auto *r = new tf_rect_selection((unsigned)i, rects[i * 8 + 0], rects[i * 8 + 1], rects[i * 8 + 2], rects[i * 8 + 3]);
    for (int c = 0; c < 4; ++c) r->color[c] = rects[i * 8 + 4 + c];
    sel.push_back(r);
  }
  const std::vector<float> lut = tf_composite_lut(sel, lut_first, lut_len, opacity);
  for (auto *s : sel) delete s;
  if (!lut.empty()) std::memcpy(out, lut.data(), lut.size() * sizeof(float));
}

size_t clvr_host_cache_len(clvr_host *h) { return h->rend.voxel_cache().size(); }
void clvr_host_pull_cache(clvr_host *h, unsigned short *out) {
  auto &c = h->rend.voxel_cache();
  c.pull();
  std::memcpy(out, &c[0], c.size() * sizeof(unsigned short));
}
size_t clvr_host_sdf_len(clvr_host *h) { return h->rend.distance_field().get_sdf_buffer().size(); }
void clvr_host_pull_sdf(clvr_host *h, signed char *out) {
  auto &s = h->rend.distance_field().get_sdf_buffer();
  s.pull();
  std::memcpy(out, &s[0], s.size());
}
// reference_volume statistics (fetch_stats at construction) and clipping (apply_clip)
void clvr_host_volume_stats(clvr_host *h, float out[4]) {
  const Volume_Stats s = h->rv->get_volume_stats();
  out[0] = s.min_v; out[1] = s.max_v; out[2] = s.min_g; out[3] = s.max_g;
}
void clvr_host_set_clipping(clvr_host *h, const unsigned lo[3], const unsigned hi[3]) {
  h->rv->set_clipping({lo[0], lo[1], lo[2]}, {hi[0], hi[1], hi[2]});
}
// the "Apply Filter" checkbox (ui.cpp:274-275)
void clvr_host_filter(clvr_host *h) { h->rv->filter(); }
// _create_tf (ui.cpp:151-158): the transfer-function editor's histogram texture, RGBA8, width x height
const void *clvr_host_render_tf(clvr_host *h, unsigned width, unsigned height) { return h->rend.render_tf(width, height); }
// nrrd_loader::load_file probe (no device involved): dims, voxel count, sum of all voxels
long long clvr_host_nrrd_probe(const char *path, unsigned dims[3], long long *checksum) {
  nrrd_loader loader;
  volume_block b = loader.load_file(path);
  dims[0] = b.m_voxel_count_x; dims[1] = b.m_voxel_count_y; dims[2] = b.m_voxel_count_z;
  long long sum = 0;
  for (short v : b.m_voxels) sum += v;
  *checksum = sum;
  return (long long)b.m_voxels.size();
}
// nrrd_loader::load_file, whole result (no device involved): counts, voxel sizes, voxels
long long clvr_host_nrrd_load(const char *path, unsigned counts[3], float sizes[3], short *out, long long cap_voxels) {
  nrrd_loader loader;
  volume_block b = loader.load_file(path);
  counts[0] = b.m_voxel_count_x; counts[1] = b.m_voxel_count_y; counts[2] = b.m_voxel_count_z;
  sizes[0] = b.m_voxel_size_x; sizes[1] = b.m_voxel_size_y; sizes[2] = b.m_voxel_size_z;
  const long long n = (long long)b.m_voxels.size();
  if (n > cap_voxels) return -n;
  std::memcpy(out, b.m_voxels.data(), (size_t)n * sizeof(short));
  return n;
}
// hdre_loader::load_file probe (no device involved): decodes into `out` (w*h*4 bytes) when it is large enough
long long clvr_host_hdr_probe(const char *path, unsigned dims[2], unsigned char *out, long long out_bytes) {
  hdre_loader loader;
  image im = loader.load_file(path);
  dims[0] = im.m_width; dims[1] = im.m_height;
  if ((long long)im.m_pixels.size() <= out_bytes) std::memcpy(out, im.m_pixels.data(), im.m_pixels.size());
  return (long long)im.m_pixels.size();
}
// ui::flush_tf string for a list of rectangles {min_v, max_v, min_g, max_g, r, g, b, a} (no device involved)
long long clvr_host_tf_source(const float *rects, int n, const float stats[4], char *out, long long out_bytes) {
  std::vector<tf_selection *> sel;
  for (int i = 0; i < n; ++i) {
    auto *r = new tf_rect_selection((unsigned)i, rects[i * 8 + 0], rects[i * 8 + 1], rects[i * 8 + 2], rects[i * 8 + 3]);
    for (int c = 0; c < 4; ++c) r->color[c] = rects[i * 8 + 4 + c];
    sel.push_back(r);
  }
  Volume_Stats st;
  st.min_v = stats[0]; st.max_v = stats[1]; st.min_g = stats[2]; st.max_g = stats[3];
  const std::string code = tf_generate_source(st, sel);
  for (auto *s : sel) delete s;
  if ((long long)code.size() + 1 <= out_bytes) std::memcpy(out, code.c_str(), code.size() + 1);
  return (long long)code.size();
}
int clvr_host_sdf_layers(clvr_host *h) { return h->rend.distance_field().layers(); }
void clvr_host_camera_direction(float alpha, float beta, float out[3]) {
  Position3D v(alpha, beta, 0.0, {1.0, 0.0, 0.0});
  out[0] = v.val[0]; out[1] = v.val[1]; out[2] = v.val[2];
}

}  // extern "C"
