// renderer.hpp -- the renderer the SDL/ImGui application talks to: same class name, base class and
// public methods as the reference's app/renderer.hpp:10-29, so `ui::run(&renderer)` is a drop-in.
#pragma once
#include <array>
#include <cstdint>
#include <string>
#include <vector>

#include <clw_context.hpp>
#include <clw_foreign_memory.hpp>
#include <clw_function.hpp>
#include <clw_image.hpp>
#include <clw_vector.hpp>

#include "signed_distance_field.hpp"
#include "ui.hpp"

// renderer::extract_mesh's result: the isosurface as an indexed triangle mesh in voxel space (clwh_mesh_isosurface)
struct mesh_data {
  std::vector<float> positions, normals;  // three per vertex
  std::vector<uint64_t> keys;             // one per vertex: the grid edge it sits on
  std::vector<uint32_t> triangles;        // three vertex indices per triangle, counter-clockwise seen from outside
};
// binary little-endian PLY (vertex x y z nx ny nz float, face uchar uint list): the bytes of scene.write_ply.  false: the file could
// not be written
bool write_ply(const std::string &path, const mesh_data &mesh);

// how renderer::overlay_slice and overlay_camera draw a region
struct overlay_style {
  int flags = CLWH_OVERLAY_FILL | CLWH_OVERLAY_OUTLINE;  // | CLWH_OVERLAY_DENSE
  uint32_t fill_alpha = 96, outline_alpha = 255;
  uint32_t id_lo = 1, id_hi = 0xFFFFFFFFu;  // the ranks drawn
};

class renderer : public frame_emitter {
 public:
  explicit renderer(clw_context &ctx);
  void image_set(const reference_volume *rv, const env_map *map) override;
  void flush_changes() override;
  void *render_frame(struct ui_state &state, bool &frame_changed) override;
  void *render_tf(const unsigned int width, const unsigned int height) override;
  void next_event_code_set(const std::string cl_code) override;

  // not in the reference: the display hand-off without the host readback.  Same pass as
  // render_frame, but the frame is written into the display's own device memory (`target`: a mapped GL buffer,
  // see clw_foreign_memory.hpp) and ordered before the display stream's next work by an event -- no pull(), no
  // 8 MiB over PCIe per frame, no host synchronisation.  `passes` > 1 batches that many std::rand() seeds into
  // ONE launch while the camera stands still (same cache as `passes` consecutive render_frame calls below the
  // token cap).
  void render_frame_device(struct ui_state &state, const clw_foreign_memory &target, int passes = 1);

  // not in the reference: a maximum / minimum / mean intensity projection of the volume (mode = CLWH_PROJ_MAX / MIN / MEAN) without a
  // transfer function, from render_frame's camera into the same frame image, so that it lines up with the path-traced frame pixel for
  // pixel (a preview while the path tracer converges).  `center` / `width` window the value to grey; `step` is the sample spacing in
  // voxels.  Pulls the frame and returns its host copy.
  void *render_projection(struct ui_state &state, int mode, float center, float width, float step = 0.5f);

  // not in the reference: direct volume rendering -- the samples of every camera ray composited front to back through the
  // colour/opacity table `lut` (float32[lut_len][4], entry 0 = voxel value lut_first; tf_composite_lut makes one from the editor's
  // selections), converged after this one launch.  Same camera and frame image as render_frame, so it lines up with the path-traced
  // frame pixel for pixel.  flags: CLWH_COMP_DENSE | CLWH_COMP_SHADE (`ambient` is read with the latter).  The table is pushed when
  // it differs from the last call's.  Pulls the frame (premultiplied RGBA8) and returns its host copy.
  void *render_composite(struct ui_state &state, const std::vector<float> &lut, int lut_first, int lut_len, float step = 0.5f,
                         float alpha_stop = 0.95f, int flags = 0, float ambient = 0.3f);

  // not in the reference: the isosurface of the volume's trilinear field at value `iso` (with CLWH_ISO_BELOW: the first position at or
  // below it), shaded by a two-sided headlight in `color`, after one launch.  Same camera and frame image as render_frame, so it lines
  // up with the path-traced frame pixel for pixel.  `refine`: bisection steps between the last outside and the first inside sample.
  // flags: CLWH_ISO_DENSE | CLWH_ISO_BELOW.  Pulls the frame (a miss is 0, 0, 0, 0) and returns its host copy.
  void *render_isosurface(struct ui_state &state, float iso, int flags = 0, float step = 0.5f, int refine = 8, float ambient = 0.3f,
                          float red = 1.0f, float green = 1.0f, float blue = 1.0f);

  // not in the reference: a slice of the volume's trilinear field on the axial, coronal or sagittal plane at `position` (voxel centres
  // along the plane's normal), or the maximum / minimum / mean (mode = CLWH_SLICE_MAX / MIN / MEAN) of a slab of `slab_samples` planes
  // `step` voxels apart centred on it: multi-planar reformatting.  The plane is slice_plane's for the launched region (state.width x
  // state.height); `center` / `width` window the value to grey.  flags: CLWH_SLICE_DENSE.  Pulls the frame (a pixel outside the volume
  // is 0, 0, 0, 0) and returns its host copy.
  enum slice_orientation { SLICE_AXIAL = 0, SLICE_CORONAL = 1, SLICE_SAGITTAL = 2 };
  void *render_slice(struct ui_state &state, int orientation, float position, int mode = 0, int slab_samples = 1, float step = 0.5f,
                     float center = 0.0f, float width = 4000.0f, int flags = 0);
  // the plane of a volume of `dims` voxels for a region of width x height pixels: normal +z with x right and y up (axial), normal +y
  // with x and z (coronal), normal +x with y and z (sagittal); one pixel spacing for both axes, the smallest at which the volume's
  // cross-section fits the region, centred in it; the slab centred on `position`.  Computed in double, rounded once.
  static void slice_plane(const size_t dims[3], int orientation, float position, int width, int height, int slab_samples, float step,
                          float origin[3], float du[3], float dv[3], float normal[3]);

  // not in the reference: the straightened curved reformat along a path and the vessel's section profile (clwh_render_curved /
  // clwh_curve_profile).  curve_frames: scene.curve_frames restated operation for operation -- the ONE place where a path (x, y, z
  // triples in voxels, in the order given) becomes the float rows both calls read; bit-identical to the Python one.  step_mm 0 means
  // pixel_mm.  render_curved: the reformat of `frames` into the region width x (rows of `frames`) of the frame image, row y the line
  // across the curve at station y; mode, slab, step, window and flags as render_slice.  Pulls the frame and returns its host copy.
  // vessel_profile: the stenosis curve of the region mask along `points` (as centerline returns them), with the volume's voxel sizes
  // as millimetres: sections of window x window samples pixel_mm apart perpendicular to the curve, one clwh_curve_profile call, and
  // scene.profile_measures' area and equivalent diameter per station.  Waits for the device.
  struct curve_frame_set {
    std::vector<float> rows;    // [H][9]: origin, du, normal; H = n rounded up to a multiple of 8, the padding rows transparent
    std::vector<double> s_mm;   // [n]: the stations' arc length
    size_t n = 0;
  };
  static curve_frame_set curve_frames(const std::vector<double> &points, const double spacing[3], int width, double pixel_mm, double station_mm,
                                      int smooth_passes = 8, double angle = 0.0, int slab_samples = 1, double step_mm = 0.0);
  void *render_curved(struct ui_state &state, const curve_frame_set &frames, int width, int mode = 0, int slab_samples = 1, float step = 0.5f,
                      float center = 0.0f, float window_width = 4000.0f, int flags = 0);
  struct profile_summary {
    std::vector<clwh_section_record> records;
    std::vector<double> s_mm, area_mm2, diameter_mm;
    std::vector<uint8_t> cut;   // border > 0: the window cut the section
  };
  profile_summary vessel_profile(struct ui_state &state, const std::vector<uint32_t> &points, double pixel_mm, int window = 64, bool connected = true);

  // not in the reference: the isosurface of the volume's grid at value `iso` as a triangle mesh (marching tetrahedra on the voxel
  // centres; flags: CLWH_MESH_DENSE | CLWH_MESH_BELOW): one counting call, buffers of that size, the filling call, the readback.
  // Unlike the views it waits for the device; no camera takes part (`state` is not read).
  mesh_data extract_mesh(struct ui_state &state, float iso, int flags = 0);

  // not in the reference: seeded region growing (clwh_segment_grow) on the volume the views show: the connected set of voxels with
  // lo <= value <= hi that hangs together with `seeds` (x, y, z triples in voxels) under 6-connectivity, with CLWH_GROW_26 under
  // 26-connectivity (flags: CLWH_GROW_26 | CLWH_GROW_FROM_MASK | CLWH_GROW_DENSE; FROM_MASK continues from the last mask).  The mask
  // stays on the device for apply_mask; the statistics come back.  Waits for the device; no camera takes part (`state` is not read).
  clwh_grow_result grow_region(struct ui_state &state, const std::vector<uint32_t> &seeds, int lo, int hi, int flags = 0);
  // ... and the last grown mask applied to the volume in place (clwh_volume_apply_mask): voxels outside the region become `fill`, with
  // CLWH_MASK_INVERT those inside.  Every view, the mesh and -- after the next flush_changes -- the path tracer then show the masked
  // volume.  The host copy of the volume keeps the loaded values.
  void apply_mask(struct ui_state &state, int fill = -32768, int flags = 0);
  // not in the reference: the volume filtered in place (clwh_volume_filter) before it is segmented: kind = CLWH_FILTER_MEDIAN (radii 0
  // or 1), CLWH_FILTER_MIN / CLWH_FILTER_MAX (grey erosion / dilation by the box, radii up to 16) or CLWH_FILTER_SMOOTH with `weights`
  // (radius[c] = weights[c].size() - 1); the edge is replicated.  masked: only the voxels of the region mask change.  Like apply_mask it
  // rewrites the device's volume, every view shows the result, and the host copy keeps the loaded values.  gaussian_weights is
  // scene.gaussian_weights bit for bit: s = sigma_mm / spacing[c]; s <= 0 gives {4096}; r = min(16, max(1, ceil(3 s))),
  // g_k = exp(-k^2 / (2 s^2)), n = g_0 + 2 sum g_k, w_k = floor(4096 g_k / n + 0.5) for k >= 1, w_0 = 4096 - 2 sum w_k.
  void filter_volume(struct ui_state &state, int kind, const uint32_t radius[3], const std::array<std::vector<uint16_t>, 3> *weights = nullptr,
                     bool masked = false);
  static std::array<std::vector<uint16_t>, 3> gaussian_weights(double sigma_mm, const double spacing[3]);

  // not in the reference: all connected components of the window lo <= value <= hi at once (clwh_segment_label; flags: CLWH_LABEL_26 |
  // CLWH_LABEL_FROM_MASK, the latter splits the last mask into its parts), ranked by descending voxel count: their number, the
  // admissible total and the records of the `top_k` largest.  The labels stay on the device for select_components.  Waits for the
  // device; no camera takes part (`state` is not read).
  struct component_summary {
    uint64_t n_components = 0, n_voxels = 0;
    std::vector<clwh_label_component> top;  // min(n_components, top_k) records, rank 1 first
  };
  component_summary label_components(struct ui_state &state, int lo, int hi, int flags = 0, unsigned top_k = 8);
  // ... and the components of ranks rank_lo .. rank_hi of the last labelling as the region mask (clwh_labels_to_mask), for apply_mask
  void select_components(struct ui_state &state, uint32_t rank_lo, uint32_t rank_hi);

  // not in the reference: distances, ball morphology and algebra of the region mask (clwh_mask_distance / clwh_mask_morph /
  // clwh_mask_combine), whoever made it: grow_region, select_components or these.  Lengths are counted in 1/16 of an x-voxel: the
  // weight of an axis is round((voxel size relative to x * 16)^2), at least 1, from the volume block's voxel sizes, and a radius r
  // in x-voxels is radius_sq = floor((r * 16)^2); this rounding is the only place where float spacing becomes integers.  No camera
  // takes part (`state` is not read).
  void mask_weights(uint32_t weight[3]) const;
  static uint32_t mask_radius_sq(float radius);
  // the exact squared distance of every voxel to the nearest voxel of the region (to_clear: to the nearest voxel outside it) in that
  // unit, uint32 [z][y][x], CLWH_DIST_NONE where there is none or the distance is above cap.  Waits for the device: the map comes back.
  std::vector<uint32_t> distance_map(struct ui_state &state, bool to_clear = false, uint32_t cap = CLWH_DIST_NONE);
  // the region dilated, eroded, opened or closed (clwh_morph_op) in place by a ball of `radius` x-voxels; the volume's border does
  // not erode.  Returns what was asked of the library and the number of voxels of the new region (the mask is pulled and counted).
  struct morph_summary {
    int op = 0;
    uint32_t radius_sq = 0, weight[3] = {1, 1, 1};
    uint64_t count = 0;
  };
  morph_summary morph_mask(struct ui_state &state, int op, float radius);
  // hold_mask keeps a copy of the region mask on the device; combine_masks replaces the region by (region op held), clwh_mask_op
  // (CLWH_MASK_NOT: the complement of the region within the volume, nothing need be held): "the grown region with its margin,
  // without the bone" is grow, hold, morph_mask(DILATE), combine_masks(ANDNOT).
  void hold_mask(struct ui_state &state);
  void combine_masks(struct ui_state &state, int op);
  // not in the reference: the region thinned in place to its skeleton without a change of its parts, cavities or tunnels
  // (clwh_mask_thin; keep_ends: the tips of branches stay, a curve skeleton; outside the volume is background, unlike morph_mask).
  // All four numbers are exact and functions of the region alone.  mask_points: the region's voxels in ascending flat index as
  // (x, y, z, n26) quadruples, n26 the number of set 26-neighbours (clwh_mask_points); the skeleton's graph is built from them in
  // Python (scene.skeleton_graph).  Both wait for the device.
  struct thin_summary {
    uint64_t count_in = 0, count_out = 0, deleted = 0;
    uint32_t iterations = 0;
  };
  thin_summary thin_mask(struct ui_state &state, bool keep_ends = true, uint32_t max_iterations = 0);
  std::vector<uint32_t> mask_points(struct ui_state &state);

  // not in the reference: shortest paths THROUGH the region mask (clwh_mask_geodesic / clwh_geodesic_trace).  geodesic_weights: the
  // step costs in mask_weights' unit, the Euclidean length of each step in 1/16 of an x-voxel, rounded, within 1 .. 65535 (face per
  // axis, edge per axis left unchanged, corner).  geodesic_map: the distance of every voxel of the region to the nearest of `seeds`
  // ((x, y, z, id) quadruples, id >= 1) inside it, uint32 [z][y][x], CLWH_DIST_NONE elsewhere and above cap; the id of that seed (the
  // smallest among equals) goes to the labelling select_components, measure_labels and the overlays read, and both maps stay on the
  // device for trace_path.  flags: CLWH_GEO_26 | CLWH_GEO_DENSE.  trace_path: the (x, y, z) triples of the shortest path from
  // `target` back to its seed, target first, inside the target's territory; empty for a voxel nothing reached; with the flags of the
  // map's call.  No camera takes part (`state` is not read); all three wait for the device.
  void geodesic_weights(uint32_t face[3], uint32_t edge[3], uint32_t *corner) const;
  struct geodesic_summary {
    clwh_geodesic_result result{};
    std::vector<uint32_t> dist;
  };
  geodesic_summary geodesic_map(struct ui_state &state, const std::vector<uint32_t> &seeds, int flags = 0, uint32_t cap = CLWH_DIST_NONE);
  std::vector<uint32_t> trace_path(struct ui_state &state, const uint32_t target[3], int flags = 0);
  // a region whose parts touch, split: the region is eroded by a ball of `radius` x-voxels (morph_mask's) until the bridges break, the
  // pieces that survive are ranked largest first (label_components' order), and they grow back inside the region, every voxel going
  // to the piece that reaches it first in unit steps (flags: CLWH_GEO_26), ties to the smaller rank.  The parts become the labelling
  // (rank = part); the region mask is unchanged.  A part that vanishes under the erosion leaves its voxels with label 0 unless a
  // surviving part reaches them.
  struct split_summary {
    uint64_t n_parts = 0;
    uint32_t radius_sq = 0, weight[3] = {1, 1, 1};
  };
  split_summary split_mask(struct ui_state &state, float radius, int flags = 0);

  // not in the reference: cheapest paths through a COST FIELD (clwh_cost_from_field / clwh_cost_geodesic / clwh_cost_trace), where a
  // step into a voxel costs the direction's multiplier times that voxel's cost.  cost_multipliers: the Euclidean length of each step
  // in 1/10 of an x-voxel, rounded (the 10 / 14 / 17 chamfer for cubic voxels), which must stay within 1 .. 255.  cost_field: the
  // cost on the device from `table` (1 .. 65536 entries) indexed by clamp((s - lo) >> shift): s is the region's depth map (the exact
  // squared distance to the nearest voxel outside the region, in mask_weights' unit), the volume's value or its squared gradient;
  // `masked`: 0 outside the region mask.  cost_geodesic: geodesic_map over that cost (a masked cost is a wall outside the region),
  // whose maps trace_cost_path then reads.  centerline: the four steps at once, from the voxel `start` to the voxel `end` inside the
  // region: the depth map, the table centerline_cost_table over it (scene.centerline_cost_table's integers; max_radius in x-voxels
  // is the largest radius of interest, 0 takes the depth map's largest value on the host: for small volumes), the cost geodesic from
  // `start` and the path from `end`: (x, y, z) triples, `end` first; empty if either lies outside the region.  All wait for the device.
  enum cost_source { COST_FROM_DEPTH = 0, COST_FROM_VALUE = 1, COST_FROM_GRADIENT = 2 };
  void cost_multipliers(uint32_t face[3], uint32_t edge[3], uint32_t *corner) const;
  static std::vector<uint16_t> centerline_cost_table(uint32_t r_sq_max, uint32_t sharpness = 100);
  void cost_field(struct ui_state &state, int source, const std::vector<uint16_t> &table, int64_t lo = 0, uint32_t shift = 0, bool masked = true);
  geodesic_summary cost_geodesic(struct ui_state &state, const std::vector<uint32_t> &seeds, int flags = 0, uint32_t cap = CLWH_DIST_NONE);
  std::vector<uint32_t> trace_cost_path(struct ui_state &state, const uint32_t target[3], int flags = 0);
  std::vector<uint32_t> centerline(struct ui_state &state, const uint32_t start[3], const uint32_t end[3], int flags = CLWH_GEO_26,
                                   float max_radius = 0.0f, uint32_t sharpness = 100);

  // not in the reference: the seeded watershed of the cost field (clwh_watershed), beside cost_geodesic: every seed ((x, y, z, id)
  // quadruples, id >= 1) floods its basin over cost_field's cost, and two floods meet on the ridge between them, however far either
  // seed lies from it.  The id of the seed whose flood reaches a voxel goes to the labelling select_components, measure_labels and
  // the overlays read; the levels (M << 16 | L, CLWH_DIST_NONE where nothing arrives) come back.  flags: CLWH_GEO_26 |
  // CLWH_GEO_DENSE.  watershed_gradient_table: scene.watershed_gradient_table's integers, 1 + the gradient's length clamped at
  // g_max, with the shift that goes with it.  pull_labels: the labelling comes back too (for small volumes).  watershed_edges: the two at once from clicks, over the unmasked gradient cost.
  struct watershed_summary {
    clwh_watershed_result result{};
    std::vector<uint32_t> level, labels;  // labels: with pull_labels only
  };
  static std::vector<uint16_t> watershed_gradient_table(uint32_t g_max, uint32_t *shift);
  watershed_summary watershed(struct ui_state &state, const std::vector<uint32_t> &seeds, int flags = 0,
                              uint32_t plateau_cap = CLWH_WATERSHED_PLATEAU_MAX, uint32_t level_cap = CLWH_WATERSHED_LEVEL_MAX,
                              bool pull_labels = false);
  watershed_summary watershed_edges(struct ui_state &state, const std::vector<uint32_t> &seeds, int flags = 0, uint32_t g_max = 4096,
                                    uint32_t plateau_cap = CLWH_WATERSHED_PLATEAU_MAX, bool pull_labels = false);

  // not in the reference: measuring (clwh_mask_statistics / clwh_label_statistics) on the volume the views show.  measure_mask: the
  // exact record of the region mask, whoever made it (count, sum, sum of squares, extremes, centroid numerators, bounding box, faces
  // per axis inside the volume and on its border), and with n_bins > 0 the histogram of its values, n_bins bins of bin_width from
  // hist_lo on, into *hist, the voxels under and over the range in the result.  Measure BEFORE apply_mask if the region is to be
  // removed: the record is of the volume as it is on the device.  measure_labels: one record per rank 1 .. capacity of the last
  // labelling (the zero record for a rank nobody has).  Both wait for the device; no camera takes part (`state` is not read).
  // region_measures in scene.py shows how the integers become millimetres.
  clwh_mask_stats_result measure_mask(struct ui_state &state, int hist_lo = 0, int bin_width = 0, int n_bins = 0,
                                      std::vector<uint64_t> *hist = nullptr);
  std::vector<clwh_region_stats> measure_labels(struct ui_state &state, unsigned capacity);

  // not in the reference: the region drawn over the frame the last view wrote (clwh_overlay_slice / clwh_overlay_camera): coloured,
  // half-transparent areas with an outline, in place of rewriting the volume with apply_mask.  `source`: the region mask (grow_region,
  // select_components, morph_mask, combine_masks), hold_mask's copy of it, or the last labelling, whose rank r gets colour
  // overlay_colours()[(r - 1) % 20].  overlay_slice takes render_slice's orientation, position, slab and step and draws with the
  // same plane; overlay_camera draws with the camera of `state`, the one of render_projection, render_composite, render_isosurface
  // and the path-traced frame.  The region is seen through whatever the view shows in front of it.  Both pull the frame and return
  // its host copy.
  enum overlay_source { OVERLAY_REGION_MASK = 0, OVERLAY_HELD_MASK = 1, OVERLAY_LABELS = 2 };
  typedef ::overlay_style overlay_style;
  void *overlay_slice(struct ui_state &state, int source, int orientation, float position, int slab_samples = 1, float step = 0.5f,
                      const overlay_style &style = overlay_style());
  void *overlay_camera(struct ui_state &state, int source, float step = 0.5f, const overlay_style &style = overlay_style());
  // the table of scene.overlay_palette: 20 well-separated opaque colours as packed RGBA8 words
  static const std::vector<uint32_t> &overlay_colours();

  // not in the reference: read-only access for tests and headless tools
  clw_vector<unsigned short> &voxel_cache() { return buffer_volume; }
  signed_distance_field &distance_field() { return sdf; }

 private:
  clw_context &ctx;
  clw_function render_func;
  clw_image<unsigned char, 4> frame;         // RGBA8 frame the caller blits
  clw_vector<unsigned short> buffer_volume;  // world-space radiance cache, 4 x u16 per voxel
  clw_image<unsigned char, 4> tfframe;
  clw_vector<float> composite_lut;           // render_composite's table on the device (host copy = the last one pushed)
  bool composite_lut_pushed = false;
  clw_vector<uint32_t> region_mask;          // grow_region's mask on the device (never pulled: the host side only sizes it)
  clw_vector<uint32_t> held_mask;            // hold_mask's copy of region_mask (never pulled)
  clw_vector<uint32_t> region_labels;        // label_components' ranks on the device, one word per voxel (never pulled)
  clw_vector<uint32_t> region_dist;          // geodesic_map's distances on the device, for trace_path
  clw_vector<uint16_t> region_cost;          // cost_field's cost on the device (never pulled)
  clw_vector<uint32_t> overlay_palette;      // overlay_colours() on the device, pushed once, by the constructor
  template <class Desc>
  void fill_overlay(Desc &d, const struct ui_state &state, int source, const overlay_style &style);
  const reference_volume *volume = nullptr;  // borrowed
  const env_map *emap = nullptr;             // borrowed
  signed_distance_field sdf;
  std::string local_cl_code;
};
