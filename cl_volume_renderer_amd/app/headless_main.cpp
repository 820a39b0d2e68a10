// headless_main.cpp -- the reference application's start-up and frame loop without the window:
// main (app/main.cpp:8-18) + the parts of ui::run that drive the frame_emitter (app/ui.cpp:170-199, 296).
// Usage: clvr_headless [--filter=median[,2d]|min=R|max=R|gauss=SIGMA_MM]... [--grow=X,Y,Z,LO,HI[,26][,dilate=R | erode=R | open=R | close=R][,split=R][,skeleton[=ends|kernel]][,centerline=X,Y,Z][,profile][,measure][,keep|remove][,fill=V][,show[=fill|outline|both]] | --components=LO,HI[,26][,largest=K | min=N][,dilate=R | erode=R | open=R | close=R][,split=R][,skeleton[=ends|kernel]][,measure][,keep|remove][,fill=V][,show[=fill|outline|both]] | --watershed=X:Y:Z,X:Y:Z[,...][,26][,gmax=G][,plateau=N][,show[=fill|outline|both] | keep=ID | remove=ID][,fill=V]] [--projection=max|min|mean | --composite | --composite=shaded | --isosurface=VALUE[,below] | --slice=axial|coronal|sagittal[,POSITION][,slab=N][,max|min|mean] | --curved[=WINDOW_MM][,angle=DEG][,slab=N][,max|min|mean] | --mesh=VALUE[,below]] <volume.nrrd> <env.hdr> [frames=16] [width=1920] [height=1080] [out.ppm]
// Prints one JSON line with the frame time and a checksum of the last frame.  --projection: the frames are intensity projections of
// the volume (renderer::render_projection, window centre 0 and width 4000, step 0.5) instead of path-traced passes.
// --composite: the frames are composited through the colour/opacity table of the default selection (renderer::render_composite: tf_composite_lut with lut_first -1024, 4096 entries, opacity 0.05; step 0.5, alpha_stop 0.95,
// ambient 0.3 when shaded).
// --isosurface=VALUE[,below]: the frames show the isosurface of the trilinear field at VALUE (renderer::render_isosurface: step 0.5,
// 8 refinement steps, white, ambient 0.3; ",below": the first position at or below VALUE).
// --slice=ORIENTATION[,POSITION][,slab=N][,max|min|mean]: the frames show the axial, coronal or sagittal plane of the trilinear field
// at POSITION (voxel centres along the plane's normal; default: the middle of the volume), or the maximum / minimum / mean of a slab
// of N planes 0.5 voxels apart centred on it (renderer::render_slice: window centre 0 and width 4000; default max).
// --mesh=VALUE[,below]: no frames; the isosurface of the volume's grid at VALUE is extracted as a triangle mesh (renderer::extract_mesh)
// and written to the `out` argument as a binary PLY.  frames, width and height are ignored; the JSON line has the counts.
// --grow=X,Y,Z,LO,HI[,26][,dilate=R | erode=R | open=R | close=R][,split=R][,skeleton[=ends|kernel]][,centerline=X,Y,Z][,profile][,measure][,keep|remove][,fill=V]: before anything is rendered or extracted, the connected set of voxels with
// LO <= value <= HI around voxel (X, Y, Z) is grown (renderer::grow_region; ",26": 26-connectivity) and applied to the volume in place
// (renderer::apply_mask): "keep" (default) sets every other voxel to V, "remove" sets the region itself to V (default -32768).  One
// JSON line has the region's count, bounding box, mean and extremes.  Goes with any one view option, with --mesh, and with none: the
// view, the mesh or the path-traced frames then show the masked volume.
// --components=LO,HI[,26][,largest=K | min=N][,dilate=R | erode=R | open=R | close=R][,split=R][,skeleton[=ends|kernel]][,measure][,keep|remove][,fill=V]: where --grow runs, all connected components of the window are
// labelled (renderer::label_components), the K largest or those of at least N voxels (default: all) become the mask
// (renderer::select_components) and are applied in place like --grow's region.  One JSON line has n_components, n_voxels, the selected
// rank range ([0, 0]: none) and count / first / bbox of up to the 8 largest.  --grow and --components exclude each other.
// dilate=R | erode=R | open=R | close=R, an item of --grow and of --components: the mask is dilated, eroded, opened or closed by a ball
// of R x-voxels (renderer::morph_mask: lengths in 1/16 x-voxel, the axes weighted by the file's voxel sizes) before it is applied; the
// JSON line then ends with "morph": {"op", "radius_sq", "weight", "count"}, count being the voxels of the mask that is applied.
// skeleton[=ends|kernel], an item of --grow and of --components: the mask that is applied or shown (after every other item has read it)
// is thinned to its skeleton without a change of its parts, cavities or tunnels (renderer::thin_mask; ends, the default: the tips of
// branches stay; kernel: only loops and cavities hold anything).  One more JSON line: {"skeleton": {"mode", "count_in", "count_out",
// "iterations", "ends", "junction_voxels"}}, ends and junction_voxels being the skeleton's voxels with one and with three or more
// neighbours among their 26 (renderer::mask_points).  With show the skeleton is overlaid instead of the mask.  The graph is built in
// Python (scene.skeleton_graph).
// split=R, an item of --grow and of --components: the mask (after any morphology item) is split into the parts that an erosion by a
// ball of R x-voxels (erode='s convention) separates: eroded, the pieces ranked largest first, and grown back inside the mask, every
// voxel to the piece that reaches it first (renderer::split_mask).  One JSON line {"split": {"radius_sq", "weight", "connectivity",
// "parts", "counts"}}, counts being the voxels of up to the 8 largest parts (renderer::measure_labels), follows the item's other
// lines; the mask that is applied is unchanged.  With show, the parts are coloured by their id.
// centerline=X,Y,Z, an item of --grow: the centreline of the mask that is applied (after any morphology) from the grow seed to the voxel
// (X, Y, Z), by the cheapest path through a cost that is low in the middle of the structure and high at its wall, 26 neighbours
// (renderer::centerline).  One JSON line {"centerline": {"from", "to", "points"}} follows the item's other lines, and with an `out`
// argument the points are written beside it, to <out>.centerline.txt, one "x y z" line each, the seed first.  An end outside the
// mask gives 0 points.  The three numbers follow the item's name, so the item takes three fields of the list.
// profile, an item of --grow that needs centerline=: the section profile of the mask along that centreline (renderer::vessel_profile:
// sections of 64 x 64 samples a quarter of the smallest voxel size apart, the part connected to the curve).  One JSON line
// {"profile": {"s_mm": [...], "area_mm2": [...], "diameter_mm": [...], "cut": [...]}} with one entry per station, the seed first,
// follows the centreline's.
// --curved[=WINDOW_MM][,angle=DEG][,slab=N][,max|min|mean]: needs --grow=...,centerline=X,Y,Z; the frames show the straightened curved
// reformat of the volume along that centreline in place of the other views (renderer::render_curved): row y of the frame is the line of
// WINDOW_MM (default 32) across the curve at station y, the seed first, pixels and stations WINDOW_MM / width apart, turned by DEG
// about the curve; thin, or the maximum / minimum / mean of a slab of N samples half a pixel apart (window centre 0 and width 4000;
// default max).  Rows beyond the curve's end stay transparent; a curve longer than `height` stations is cut there.
// measure, an item of --grow and of --components: a second JSON line with the exact record (renderer::measure_mask: count, sum, sum_sq,
// min, max, sum_pos, bbox, faces, border_faces) of the mask that is applied, after any morphology and before the volume is changed:
// {"measure": {...}}; for --components {"measure_components": [...]}, the records (renderer::measure_labels) of the selected ranks,
// rank 1 first, at most 256 of them, and with a morphology item also "measure": the record of the morphed mask.
// show[=fill|outline|both] (default both), an item of --grow and of --components: the volume is NOT rewritten; the region is drawn over
// every frame of the chosen view instead (renderer::overlay_slice with --slice's plane, renderer::overlay_camera with the camera of
// --projection, --composite and --isosurface): half-transparent colour, an outline, or both.  --components colours every selected
// component by its rank (with a morphology item: the morphed mask, in one colour).  The JSON lines say "mode": "show" and
// "overlay": "fill" | "outline" | "both".  show excludes keep, remove and fill=, and needs one of those four views.
// --watershed=X:Y:Z,X:Y:Z[,...][,26][,gmax=G][,plateau=N][,show[=fill|outline|both] | keep=ID | remove=ID][,fill=V]: where --grow runs, the
// volume is divided among the clicks (X:Y:Z each, ids 1, 2, ... in order) by the seeded watershed of its gradient
// (renderer::watershed_edges: the cost is 1 + the gradient's length clamped at G, default 4096; plateau_cap N, default 65534; ",26":
// 26 neighbours): every click floods its basin, and two floods meet on the edge between them.  One JSON line {"watershed": {"seeds",
// "connectivity", "gmax", "plateau", "mode", "fill", "reached", "max_level", "counts"}}, counts being the voxels of every id
// (renderer::measure_labels).  show draws the labelling over the view like --components' (a colour per id); keep=ID / remove=ID make
// the territory of one click the mask (renderer::select_components) and apply it like --grow's region; with none of the three the
// volume is left as it is.  --watershed excludes --grow and --components.
// --filter=median[,2d] | min=R | max=R | gauss=SIGMA_MM, repeatable: the loaded volume is filtered in place (renderer::filter_volume)
// before any view, --grow, --components, --watershed or --mesh sees it, one filter per option in the order given: the 3 x 3 x 3
// median (",2d": 3 x 3 in the slice), the grey minimum / maximum over a box of R voxels (0 .. 16) on every side, or the exact integer
// Gaussian of SIGMA_MM (renderer::gaussian_weights with the file's voxel sizes: anisotropic voxels get a radius per axis).  The edge
// is replicated.  One JSON line each: {"filter": {"kind", "radius": [rx, ry, rz]}}.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include <clwh.h>

#include "common_defines.hpp"
#include "hdre_loader.hpp"
#include "nrrd_loader.hpp"
#include "renderer.hpp"
#include "tf_part.hpp"

int main(int argc_in, char const *argv_in[]) {
  int projection = -1;  // clwh_projection, or -1: path-traced frames
  int composite = -1;   // 0: plain, 1: shaded, or -1
  bool isosurface = false, iso_below = false;
  float iso_value = 0.0f;
  int slice = -1;  // renderer::slice_orientation, or -1
  int slice_mode = CLWH_SLICE_MAX, slice_slab = 1;
  bool slice_centred = true;
  float slice_position = 0.0f;
  bool mesh = false, mesh_below = false;
  float mesh_value = 0.0f;
  bool grow = false, grow_remove = false;
  uint32_t grow_seed[3] = {0, 0, 0};
  int grow_lo = 0, grow_hi = 0, grow_flags = 0, grow_fill = -32768;
  bool comps = false, comps_remove = false;
  int comps_lo = 0, comps_hi = 0, comps_flags = 0, comps_fill = -32768;
  long long comps_largest = -1, comps_min = -1;
  int morph_op = -1;  // clwh_morph_op of the dilate= | erode= | open= | close= item, or -1
  float morph_radius = 0.0f;
  bool measure = false;  // the measure item
  float split_radius = -1.0f;  // the split= item's erosion radius in x-voxels, or -1
  bool centerline = false;     // the centerline= item of --grow
  uint32_t centerline_end[3] = {0, 0, 0};
  bool profile = false;        // the profile item of --grow
  bool curved = false;         // --curved
  float curved_window = 32.0f, curved_angle = 0.0f;
  int curved_mode = CLWH_SLICE_MAX, curved_slab = 1;
  bool shed = false;           // --watershed
  std::vector<uint32_t> shed_seeds;  // (x, y, z, id) quadruples
  int shed_flags = 0, shed_fill = -32768;
  long shed_gmax = 4096, shed_plateau = CLWH_WATERSHED_PLATEAU_MAX, shed_keep = -1, shed_remove = -1;
  struct filter_spec {
    int kind;         // clwh_filter_kind
    uint32_t radius;  // min, max
    bool flat;        // median,2d
    double sigma;     // gauss
  };
  std::vector<filter_spec> filters;  // --filter, in the order given
  int show = -1;         // the show item: CLWH_OVERLAY_FILL | CLWH_OVERLAY_OUTLINE, or -1
  bool rewrites = false; // a keep, remove or fill= item
  // whether `v` is the show item; *ok is cleared if its style is unknown
  const auto show_item = [&](const std::string &v, bool *ok) {
    if (v != "show" && v.rfind("show=", 0) != 0) return false;
    const std::string style = v == "show" ? "both" : v.substr(5);
    show = style == "fill" ? CLWH_OVERLAY_FILL : style == "outline" ? CLWH_OVERLAY_OUTLINE : CLWH_OVERLAY_FILL | CLWH_OVERLAY_OUTLINE;
    *ok = *ok && (style == "fill" || style == "outline" || style == "both");
    return true;
  };
  // whether `v` is that item; *ok is cleared if its radius is not a number >= 0
  const auto morph_item = [&](const std::string &v, bool *ok) {
    static const char *const names[4] = {"dilate=", "erode=", "open=", "close="};
    for (int op = 0; op < 4; ++op) {
      const std::string name = names[op];
      if (v.rfind(name, 0) != 0) continue;
      char *end = nullptr;
      const float radius = std::strtof(v.c_str() + name.size(), &end);
      *ok = *ok && v.size() > name.size() && *end == '\0' && radius >= 0.0f && radius <= 4095.0f && morph_op < 0;
      morph_op = op;
      morph_radius = radius;
      return true;
    }
    return false;
  };
  int skeleton = -1;  // the skeleton item: 1 = ends (CLWH_THIN_KEEP_ENDS), 0 = kernel, or -1
  const auto skeleton_item = [&](const std::string &v, bool *ok) {
    if (v != "skeleton" && v.rfind("skeleton=", 0) != 0) return false;
    const std::string mode = v == "skeleton" ? "ends" : v.substr(9);
    *ok = *ok && (mode == "ends" || mode == "kernel") && skeleton < 0;
    skeleton = mode == "ends" ? 1 : 0;
    return true;
  };
  // whether `v` is the split= item; *ok is cleared if its radius is not a number >= 0
  const auto split_item = [&](const std::string &v, bool *ok) {
    if (v.rfind("split=", 0) != 0) return false;
    char *end = nullptr;
    const float radius = std::strtof(v.c_str() + 6, &end);
    *ok = *ok && v.size() > 6 && *end == '\0' && radius >= 0.0f && radius <= 4095.0f && split_radius < 0.0f;
    split_radius = radius;
    return true;
  };
  static const char *const kCompsUsage = "(--components=LO,HI[,26][,largest=K | min=N][,dilate=R | erode=R | open=R | close=R][,split=R][,skeleton[=ends|kernel]][,measure][,keep|remove][,fill=V][,show[=fill|outline|both]])";
  static const char *const kGrowUsage = "(--grow=X,Y,Z,LO,HI[,26][,dilate=R | erode=R | open=R | close=R][,split=R][,skeleton[=ends|kernel]][,centerline=X,Y,Z][,profile][,measure][,keep|remove][,fill=V][,show[=fill|outline|both]])";
  static const char *const kShedUsage = "(--watershed=X:Y:Z,X:Y:Z[,...][,26][,gmax=G][,plateau=N][,show[=fill|outline|both] | keep=ID | remove=ID][,fill=V])";
  static const char *const kCurvedUsage = "(--curved[=WINDOW_MM][,angle=DEG][,slab=N][,max|min|mean], with --grow=...,centerline=X,Y,Z)";
  static const char *const kSliceUsage = "(--slice=axial|coronal|sagittal[,POSITION][,slab=N][,max|min|mean])";
  std::vector<const char *> args{argv_in[0]};
  for (int i = 1; i < argc_in; ++i) {
    const std::string a = argv_in[i];
    if (a.rfind("--filter", 0) == 0) {
      const std::string v = a.size() > 9 && a[8] == '=' ? a.substr(9) : "";
      filter_spec f{CLWH_FILTER_MEDIAN, 1u, false, 0.0};
      char *end = nullptr;
      bool ok = true;
      if (v == "median" || v == "median,2d") {
        f.flat = v != "median";
      } else if (v.rfind("min=", 0) == 0 || v.rfind("max=", 0) == 0) {
        const long n = std::strtol(v.c_str() + 4, &end, 10);
        ok = v.size() > 4 && *end == '\0' && n >= 0 && n <= CLWH_FILTER_MAX_RADIUS;
        f.kind = v[1] == 'i' ? CLWH_FILTER_MIN : CLWH_FILTER_MAX;
        f.radius = (uint32_t)n;
      } else if (v.rfind("gauss=", 0) == 0) {
        f.sigma = std::strtod(v.c_str() + 6, &end);
        ok = v.size() > 6 && *end == '\0' && std::isfinite(f.sigma) && f.sigma >= 0.0;
        f.kind = CLWH_FILTER_SMOOTH;
      } else {
        ok = false;
      }
      if (!ok) {
        std::cout << "Unknown option '" << a << "' (--filter=median[,2d]|min=R|max=R|gauss=SIGMA_MM)\n";
        return 1;
      }
      filters.push_back(f);
    } else if (a.rfind("--projection=", 0) == 0) {
      const std::string m = a.substr(13);
      projection = m == "max" ? CLWH_PROJ_MAX : m == "min" ? CLWH_PROJ_MIN : m == "mean" ? CLWH_PROJ_MEAN : -2;
      if (projection == -2) {
        std::cout << "Unknown projection '" << m << "' (max, min or mean)\n";
        return 1;
      }
    } else if (a == "--composite" || a == "--composite=plain") {
      composite = 0;
    } else if (a == "--composite=shaded") {
      composite = 1;
    } else if (a.rfind("--composite", 0) == 0) {
      std::cout << "Unknown option '" << a << "' (--composite or --composite=shaded)\n";
      return 1;
    } else if (a.rfind("--isosurface=", 0) == 0) {
      std::string v = a.substr(13);
      const size_t comma = v.find(',');
      if (comma != std::string::npos) {
        if (v.substr(comma + 1) != "below") {
          std::cout << "Unknown option '" << a << "' (--isosurface=VALUE or --isosurface=VALUE,below)\n";
          return 1;
        }
        iso_below = true;
        v = v.substr(0, comma);
      }
      char *end = nullptr;
      iso_value = std::strtof(v.c_str(), &end);
      if (v.empty() || *end != '\0' || !std::isfinite(iso_value)) {
        std::cout << "Bad isosurface value '" << v << "'\n";
        return 1;
      }
      isosurface = true;
    } else if (a.rfind("--isosurface", 0) == 0) {
      std::cout << "Unknown option '" << a << "' (--isosurface=VALUE or --isosurface=VALUE,below)\n";
      return 1;
    } else if (a.rfind("--mesh=", 0) == 0) {
      std::string v = a.substr(7);
      const size_t comma = v.find(',');
      if (comma != std::string::npos) {
        if (v.substr(comma + 1) != "below") {
          std::cout << "Unknown option '" << a << "' (--mesh=VALUE or --mesh=VALUE,below)\n";
          return 1;
        }
        mesh_below = true;
        v = v.substr(0, comma);
      }
      char *end = nullptr;
      mesh_value = std::strtof(v.c_str(), &end);
      if (v.empty() || *end != '\0' || !std::isfinite(mesh_value)) {
        std::cout << "Bad mesh value '" << v << "'\n";
        return 1;
      }
      mesh = true;
    } else if (a.rfind("--mesh", 0) == 0) {
      std::cout << "Unknown option '" << a << "' (--mesh=VALUE or --mesh=VALUE,below)\n";
      return 1;
    } else if (a.rfind("--grow=", 0) == 0) {
      std::string rest = a.substr(7);
      bool ok = true;
      int field = 0;
      for (; ok && (field == 0 || !rest.empty()); ++field) {
        const size_t comma = rest.find(',');
        const std::string v = rest.substr(0, comma);
        rest = comma == std::string::npos ? "" : rest.substr(comma + 1);
        if (comma != std::string::npos && rest.empty()) ok = false;  // a trailing comma
        char *end = nullptr;
        if (field < 5) {
          const long long n = std::strtoll(v.c_str(), &end, 10);
          ok = ok && !v.empty() && *end == '\0';
          if (field < 3) {
            ok = ok && n >= 0 && n <= 0x7fffffffLL;
            grow_seed[field] = (uint32_t)n;
          } else {
            ok = ok && n >= -32768 && n <= 32767;
            (field == 3 ? grow_lo : grow_hi) = (int)n;
          }
        } else if (v == "26") {
          grow_flags |= CLWH_GROW_26;
        } else if (morph_item(v, &ok)) {
        } else if (split_item(v, &ok)) {
        } else if (skeleton_item(v, &ok)) {
        } else if (v.rfind("centerline=", 0) == 0) {  // X here, Y and Z in the next two fields
          ok = ok && !centerline;
          centerline = true;
          std::string number = v.substr(11);
          for (int q = 0; q < 3 && ok; ++q) {
            if (q > 0) {
              const size_t next = rest.find(',');
              number = rest.substr(0, next);
              ok = !rest.empty() && !(next != std::string::npos && next + 1 == rest.size());
              rest = next == std::string::npos ? "" : rest.substr(next + 1);
            }
            const long long n = std::strtoll(number.c_str(), &end, 10);
            ok = ok && !number.empty() && *end == '\0' && n >= 0 && n <= 0x7fffffffLL;
            centerline_end[q] = (uint32_t)n;
          }
        } else if (v == "profile") {
          profile = true;
        } else if (v == "measure") {
          measure = true;
        } else if (show_item(v, &ok)) {
        } else if (v == "keep" || v == "remove") {
          grow_remove = v == "remove";
          rewrites = true;
        } else if (v.rfind("fill=", 0) == 0) {
          rewrites = true;
          const long n = std::strtol(v.c_str() + 5, &end, 10);
          ok = ok && v.size() > 5 && *end == '\0' && n >= -32768 && n <= 32767;
          grow_fill = (int)n;
        } else {
          ok = false;
        }
      }
      if (!ok || field < 5 || grow_lo > grow_hi || (show >= 0 && rewrites) || (profile && !centerline)) {
        std::cout << "Unknown option '" << a << "' " << kGrowUsage << "\n";
        return 1;
      }
      grow = true;
    } else if (a.rfind("--grow", 0) == 0) {
      std::cout << "Unknown option '" << a << "' " << kGrowUsage << "\n";
      return 1;
    } else if (a.rfind("--components=", 0) == 0) {
      std::string rest = a.substr(13);
      bool ok = true;
      int field = 0;
      for (; ok && (field == 0 || !rest.empty()); ++field) {
        const size_t comma = rest.find(',');
        const std::string v = rest.substr(0, comma);
        rest = comma == std::string::npos ? "" : rest.substr(comma + 1);
        if (comma != std::string::npos && rest.empty()) ok = false;  // a trailing comma
        char *end = nullptr;
        if (field < 2) {
          const long long n = std::strtoll(v.c_str(), &end, 10);
          ok = ok && !v.empty() && *end == '\0' && n >= -32768 && n <= 32767;
          (field == 0 ? comps_lo : comps_hi) = (int)n;
        } else if (v == "26") {
          comps_flags |= CLWH_LABEL_26;
        } else if (morph_item(v, &ok)) {
        } else if (split_item(v, &ok)) {
        } else if (skeleton_item(v, &ok)) {
        } else if (v == "measure") {
          measure = true;
        } else if (show_item(v, &ok)) {
        } else if (v == "keep" || v == "remove") {
          comps_remove = v == "remove";
          rewrites = true;
        } else if (v.rfind("fill=", 0) == 0) {
          rewrites = true;
          const long n = std::strtol(v.c_str() + 5, &end, 10);
          ok = ok && v.size() > 5 && *end == '\0' && n >= -32768 && n <= 32767;
          comps_fill = (int)n;
        } else if (v.rfind("largest=", 0) == 0) {
          comps_largest = std::strtoll(v.c_str() + 8, &end, 10);
          ok = ok && v.size() > 8 && *end == '\0' && comps_largest >= 1 && comps_largest <= 0x7fffffffLL;
        } else if (v.rfind("min=", 0) == 0) {
          comps_min = std::strtoll(v.c_str() + 4, &end, 10);
          ok = ok && v.size() > 4 && *end == '\0' && comps_min >= 1 && comps_min <= 0x7fffffffLL;
        } else {
          ok = false;
        }
      }
      if (!ok || field < 2 || comps_lo > comps_hi || (comps_largest >= 0 && comps_min >= 0) || (show >= 0 && rewrites)) {
        std::cout << "Unknown option '" << a << "' " << kCompsUsage << "\n";
        return 1;
      }
      comps = true;
    } else if (a.rfind("--components", 0) == 0) {
      std::cout << "Unknown option '" << a << "' " << kCompsUsage << "\n";
      return 1;
    } else if (a.rfind("--watershed=", 0) == 0) {
      std::string rest = a.substr(12);
      bool ok = true;
      for (int field = 0; ok && (field == 0 || !rest.empty()); ++field) {
        const size_t comma = rest.find(',');
        const std::string v = rest.substr(0, comma);
        rest = comma == std::string::npos ? "" : rest.substr(comma + 1);
        if (comma != std::string::npos && rest.empty()) ok = false;  // a trailing comma
        char *end = nullptr;
        if (v.find(':') != std::string::npos) {  // a click: they come first
          uint32_t at[3] = {0, 0, 0};
          const char *p = v.c_str();
          for (int q = 0; ok && q < 3; ++q) {
            const long long n = std::strtoll(p, &end, 10);
            ok = end != p && *p != '-' && *p != '+' && n >= 0 && n <= 0x7fffffffLL && *end == (q < 2 ? ':' : '\0');
            at[q] = (uint32_t)n;
            p = end + 1;
          }
          ok = ok && (size_t)field == shed_seeds.size() / 4 && shed_seeds.size() / 4 < CLWH_GROW_MAX_SEEDS;
          shed_seeds.insert(shed_seeds.end(), {at[0], at[1], at[2], (uint32_t)(shed_seeds.size() / 4 + 1)});
        } else if (v == "26") {
          shed_flags |= CLWH_GEO_26;
        } else if (show_item(v, &ok)) {
        } else if (v.rfind("gmax=", 0) == 0) {
          shed_gmax = std::strtol(v.c_str() + 5, &end, 10);
          ok = ok && v.size() > 5 && *end == '\0' && shed_gmax >= 1 && shed_gmax <= 2 * 65535;
        } else if (v.rfind("plateau=", 0) == 0) {
          shed_plateau = std::strtol(v.c_str() + 8, &end, 10);
          ok = ok && v.size() > 8 && *end == '\0' && shed_plateau >= 0 && shed_plateau <= (long)CLWH_WATERSHED_PLATEAU_MAX;
        } else if (v.rfind("keep=", 0) == 0) {
          shed_keep = std::strtol(v.c_str() + 5, &end, 10);
          ok = ok && v.size() > 5 && *end == '\0' && shed_keep >= 1;
          rewrites = true;
        } else if (v.rfind("remove=", 0) == 0) {
          shed_remove = std::strtol(v.c_str() + 7, &end, 10);
          ok = ok && v.size() > 7 && *end == '\0' && shed_remove >= 1;
          rewrites = true;
        } else if (v.rfind("fill=", 0) == 0) {
          const long n = std::strtol(v.c_str() + 5, &end, 10);
          ok = ok && v.size() > 5 && *end == '\0' && n >= -32768 && n <= 32767;
          shed_fill = (int)n;
        } else {
          ok = false;
        }
      }
      const long n_ids = (long)(shed_seeds.size() / 4);
      if (!ok || n_ids < 1 || (shed_keep >= 0 && shed_remove >= 0) || (show >= 0 && rewrites) || shed_keep > n_ids || shed_remove > n_ids ||
          (shed_fill != -32768 && !rewrites)) {
        std::cout << "Unknown option '" << a << "' " << kShedUsage << "\n";
        return 1;
      }
      shed = true;
    } else if (a.rfind("--watershed", 0) == 0) {
      std::cout << "Unknown option '" << a << "' " << kShedUsage << "\n";
      return 1;
    } else if (a.rfind("--slice=", 0) == 0) {
      std::string rest = a.substr(8);
      bool ok = true;
      for (int field = 0; ok && (field == 0 || !rest.empty()); ++field) {
        const size_t comma = rest.find(',');
        const std::string v = rest.substr(0, comma);
        rest = comma == std::string::npos ? "" : rest.substr(comma + 1);
        if (comma != std::string::npos && rest.empty()) ok = false;  // a trailing comma
        char *end = nullptr;
        if (field == 0) {
          slice = v == "axial" ? renderer::SLICE_AXIAL : v == "coronal" ? renderer::SLICE_CORONAL : v == "sagittal" ? renderer::SLICE_SAGITTAL : -1;
          ok = ok && slice >= 0;
        } else if (v == "max" || v == "min" || v == "mean") {
          slice_mode = v == "max" ? CLWH_SLICE_MAX : v == "min" ? CLWH_SLICE_MIN : CLWH_SLICE_MEAN;
        } else if (v.rfind("slab=", 0) == 0) {
          const long n = std::strtol(v.c_str() + 5, &end, 10);
          ok = ok && v.size() > 5 && *end == '\0' && n >= 1 && n <= 8192;
          slice_slab = (int)n;
        } else {
          slice_position = std::strtof(v.c_str(), &end);
          ok = ok && !v.empty() && *end == '\0' && std::isfinite(slice_position);
          slice_centred = false;
        }
      }
      if (!ok) {
        std::cout << "Unknown option '" << a << "' " << kSliceUsage << "\n";
        return 1;
      }
    } else if (a.rfind("--slice", 0) == 0) {
      std::cout << "Unknown option '" << a << "' " << kSliceUsage << "\n";
      return 1;
    } else if (a == "--curved" || a.rfind("--curved=", 0) == 0) {
      std::string rest = a == "--curved" ? "" : a.substr(9);
      bool ok = a == "--curved" || !rest.empty();
      for (int field = 0; ok && !rest.empty(); ++field) {
        const size_t comma = rest.find(',');
        const std::string v = rest.substr(0, comma);
        rest = comma == std::string::npos ? "" : rest.substr(comma + 1);
        if (comma != std::string::npos && rest.empty()) ok = false;  // a trailing comma
        char *end = nullptr;
        if (v == "max" || v == "min" || v == "mean") {
          curved_mode = v == "max" ? CLWH_SLICE_MAX : v == "min" ? CLWH_SLICE_MIN : CLWH_SLICE_MEAN;
        } else if (v.rfind("slab=", 0) == 0) {
          const long n = std::strtol(v.c_str() + 5, &end, 10);
          ok = ok && v.size() > 5 && *end == '\0' && n >= 1 && n <= 8192;
          curved_slab = (int)n;
        } else if (v.rfind("angle=", 0) == 0) {
          curved_angle = std::strtof(v.c_str() + 6, &end);
          ok = ok && v.size() > 6 && *end == '\0' && std::isfinite(curved_angle);
        } else {
          curved_window = std::strtof(v.c_str(), &end);
          ok = ok && field == 0 && !v.empty() && *end == '\0' && std::isfinite(curved_window) && curved_window > 0.0f;
        }
      }
      if (!ok) {
        std::cout << "Unknown option '" << a << "' " << kCurvedUsage << "\n";
        return 1;
      }
      curved = true;
    } else if (a.rfind("--curved", 0) == 0) {
      std::cout << "Unknown option '" << a << "' " << kCurvedUsage << "\n";
      return 1;
    } else {
      args.push_back(argv_in[i]);
    }
  }
  if (grow && comps) {
    std::cout << "--grow and --components exclude each other\n";
    return 1;
  }
  if (shed && (grow || comps)) {
    std::cout << "--watershed excludes --grow and --components\n";
    return 1;
  }
  if (show >= 0 && projection < 0 && composite < 0 && !isosurface && slice < 0) {
    std::cout << "show needs --projection, --composite, --isosurface or --slice " << (shed ? kShedUsage : grow ? kGrowUsage : kCompsUsage) << "\n";
    return 1;
  }
  if (curved && (projection >= 0 || composite >= 0 || isosurface || slice >= 0 || mesh)) {
    std::cout << "--curved excludes --projection, --composite, --isosurface, --slice and --mesh\n";
    return 1;
  }
  if (curved && !(grow && centerline)) {
    std::cout << "--curved needs --grow with a centerline= item " << kCurvedUsage << "\n";
    return 1;
  }
  if (mesh && (projection >= 0 || composite >= 0 || isosurface || slice >= 0)) {
    std::cout << "--mesh excludes --projection, --composite, --isosurface and --slice\n";
    return 1;
  }
  if (slice >= 0 && (projection >= 0 || composite >= 0 || isosurface)) {
    std::cout << "--slice excludes --projection, --composite and --isosurface\n";
    return 1;
  }
  if (projection >= 0 && composite >= 0) {
    std::cout << "--projection and --composite exclude each other\n";
    return 1;
  }
  if (isosurface && (projection >= 0 || composite >= 0)) {
    std::cout << "--isosurface excludes --projection and --composite\n";
    return 1;
  }
  const int argc = (int)args.size();
  char const *const *argv = args.data();
  if (argc < 3) {
    std::cout << "Usage: " << argv[0] << " [--filter=median[,2d]|min=R|max=R|gauss=SIGMA_MM]... [--grow=X,Y,Z,LO,HI[,26][,dilate=R | erode=R | open=R | close=R][,split=R][,skeleton[=ends|kernel]][,centerline=X,Y,Z][,profile][,measure][,keep|remove][,fill=V][,show[=fill|outline|both]] | --components=LO,HI[,26][,largest=K | min=N][,dilate=R | erode=R | open=R | close=R][,split=R][,skeleton[=ends|kernel]][,measure][,keep|remove][,fill=V][,show[=fill|outline|both]] | --watershed=X:Y:Z,X:Y:Z[,...][,26][,gmax=G][,plateau=N][,show[=fill|outline|both] | keep=ID | remove=ID][,fill=V]] [--projection=max|min|mean | --composite[=shaded] | --isosurface=VALUE[,below] | --slice=axial|coronal|sagittal[,POSITION][,slab=N][,max|min|mean] | --curved[=WINDOW_MM][,angle=DEG][,slab=N][,max|min|mean] | --mesh=VALUE[,below]] <path to nrrd file> <path to envmap> [frames] [width] [height] [out.ppm]\n";
    return 1;
  }
  const int frames = argc > 3 ? std::atoi(argv[3]) : 16;
  const int width = argc > 4 ? std::atoi(argv[4]) : 1920;
  const int height = argc > 5 ? std::atoi(argv[5]) : 1080;

  static const char *const kMorphNames[4] = {"dilate", "erode", "open", "close"};
  const auto print_record = [](const clwh_region_stats &s) {
    std::printf("{\"count\": %llu, \"sum\": %lld, \"sum_sq\": %llu, \"min\": %d, \"max\": %d, \"sum_pos\": [%llu, %llu, %llu], "
                "\"bbox_lo\": [%u, %u, %u], \"bbox_hi\": [%u, %u, %u], \"faces\": [%u, %u, %u], \"border_faces\": [%u, %u, %u]}",
                (unsigned long long)s.count, (long long)s.sum, (unsigned long long)s.sum_sq, s.vmin, s.vmax, (unsigned long long)s.sum_pos[0],
                (unsigned long long)s.sum_pos[1], (unsigned long long)s.sum_pos[2], s.bbox_lo[0], s.bbox_lo[1], s.bbox_lo[2], s.bbox_hi[0],
                s.bbox_hi[1], s.bbox_hi[2], s.faces[0], s.faces[1], s.faces[2], s.border_faces[0], s.border_faces[1], s.border_faces[2]);
  };
  clw_context ctx;
  renderer r(ctx);
  frame_emitter *emitter = &r;

  nrrd_loader vloader;
  volume_block v = vloader.load_file(argv[1]);
  reference_volume rv(ctx, &v);
  rv.set_value_clip({-2000, 3000});
  rv.set_gradient_clip({0, 4000});
  hdre_loader iloader;
  image em = iloader.load_file(argv[2]);
  env_map emap(ctx, em);
  emitter->image_set(&rv, &emap);

  {  // --filter: before anything reads the volume
    ui_state none{argv[1], true, height, width, Position3D(0, 0, 0), {0.f, 0.f}, true};
    for (const filter_spec &f : filters) {
      uint32_t radius[3] = {f.radius, f.radius, f.radius};
      if (f.kind == CLWH_FILTER_MEDIAN) radius[2] = f.flat ? 0u : 1u;
      if (f.kind == CLWH_FILTER_SMOOTH) {
        const auto &sizes = rv.get_voxel_sizes();
        const double spacing[3] = {(double)sizes[0], (double)sizes[1], (double)sizes[2]};
        const std::array<std::vector<uint16_t>, 3> w = renderer::gaussian_weights(f.sigma, spacing);
        for (int q = 0; q < 3; ++q) radius[q] = (uint32_t)w[q].size() - 1u;
        r.filter_volume(none, f.kind, radius, &w);
      } else {
        r.filter_volume(none, f.kind, radius);
      }
      static const char *const kFilterNames[4] = {"median", "min", "max", "gauss"};
      std::printf("{\"filter\": {\"kind\": \"%s\", \"radius\": [%u, %u, %u]}}\n", kFilterNames[f.kind], radius[0], radius[1], radius[2]);
    }
  }

  int show_source = renderer::OVERLAY_REGION_MASK;  // what the show item draws
  renderer::overlay_style show_style;
  if (show >= 0) show_style.flags = show;
  static const char *const kShowNames[4] = {"", "fill", "outline", "both"};

  // the split= item: the mask (after any morphology) is split into the parts that an erosion by R separates (renderer::split_mask);
  // one JSON line with their number and the voxel counts of up to the 8 largest; with show, the parts are coloured by their id
  std::string split_line;  // printed behind the item's own lines
  const auto split = [&](ui_state &none, bool conn26) {
    const renderer::split_summary s = r.split_mask(none, split_radius, conn26 ? CLWH_GEO_26 : 0);
    std::vector<uint64_t> counts;
    if (s.n_parts > 0)
      for (const clwh_region_stats &rec : r.measure_labels(none, (unsigned)std::min<uint64_t>(s.n_parts, 65536))) counts.push_back(rec.count);
    std::sort(counts.begin(), counts.end(), [](uint64_t a, uint64_t b) { return a > b; });
    counts.resize(std::min<size_t>(counts.size(), 8));
    split_line = "{\"split\": {\"radius_sq\": " + std::to_string(s.radius_sq) + ", \"weight\": [" + std::to_string(s.weight[0]) + ", " +
                 std::to_string(s.weight[1]) + ", " + std::to_string(s.weight[2]) + "], \"connectivity\": " + (conn26 ? "26" : "6") +
                 ", \"parts\": " + std::to_string(s.n_parts) + ", \"counts\": [";
    for (size_t k = 0; k < counts.size(); ++k) split_line += (k ? ", " : "") + std::to_string(counts[k]);
    split_line += "]}}\n";
    if (show >= 0 && s.n_parts > 0) {
      show_source = renderer::OVERLAY_LABELS;
      show_style.id_hi = (uint32_t)std::min<uint64_t>(s.n_parts, 0xFFFFFFFFull);
    }
  };

  // the skeleton item: the mask is thinned in place, last of all the items that read it; with show it is what is drawn
  std::string skeleton_line;
  const auto thin = [&](ui_state &none) {
    const renderer::thin_summary t = r.thin_mask(none, skeleton == 1);
    const std::vector<uint32_t> points = r.mask_points(none);
    uint64_t ends = 0, junctions = 0;
    for (size_t k = 3; k < points.size(); k += 4) {
      ends += points[k] == 1u;
      junctions += points[k] >= 3u;
    }
    skeleton_line = std::string("{\"skeleton\": {\"mode\": \"") + (skeleton == 1 ? "ends" : "kernel") + "\", \"count_in\": " + std::to_string(t.count_in) +
                    ", \"count_out\": " + std::to_string(t.count_out) + ", \"iterations\": " + std::to_string(t.iterations) +
                    ", \"ends\": " + std::to_string(ends) + ", \"junction_voxels\": " + std::to_string(junctions) + "}}\n";
    show_source = renderer::OVERLAY_REGION_MASK;
  };

  std::vector<uint32_t> curve;  // the centreline from the seed to its end: what --curved unrolls
  if (grow) {  // first: everything below sees the masked volume
    const auto &size = rv.get_volume_size();
    for (int q = 0; q < 3; ++q)
      if (grow_seed[q] >= size[q]) {
        std::cout << "The --grow seed (" << grow_seed[0] << ", " << grow_seed[1] << ", " << grow_seed[2] << ") lies outside the volume\n";
        return 1;
      }
    ui_state none{argv[1], true, height, width, Position3D(0, 0, 0), {0.f, 0.f}, true};
    const clwh_grow_result g = r.grow_region(none, {grow_seed[0], grow_seed[1], grow_seed[2]}, grow_lo, grow_hi, grow_flags);
    renderer::morph_summary m;
    if (morph_op >= 0) m = r.morph_mask(none, morph_op, morph_radius);
    clwh_mask_stats_result measured{};
    if (measure) measured = r.measure_mask(none);  // of the volume as loaded: before the mask changes it
    if (split_radius >= 0.0f) split(none, (grow_flags & CLWH_GROW_26) != 0);
    std::vector<uint32_t> line;  // the centerline= item: from its end back to the seed
    if (centerline) {
      for (int q = 0; q < 3; ++q)
        if (centerline_end[q] >= size[q]) {
          std::cout << "The centerline end (" << centerline_end[0] << ", " << centerline_end[1] << ", " << centerline_end[2] << ") lies outside the volume\n";
          return 1;
        }
      line = r.centerline(none, grow_seed, centerline_end);
      if (argc > 6) {
        std::ofstream file(std::string(argv[6]) + ".centerline.txt");
        for (size_t k = line.size() / 3; k-- > 0;) file << line[3 * k] << ' ' << line[3 * k + 1] << ' ' << line[3 * k + 2] << '\n';
      }
    }
    for (size_t k = line.size() / 3; k-- > 0;) curve.insert(curve.end(), line.begin() + 3 * k, line.begin() + 3 * k + 3);
    renderer::profile_summary sections;
    if (profile && curve.size() >= 6) {
      const auto &sizes = rv.get_voxel_sizes();
      sections = r.vessel_profile(none, curve, (double)std::min(sizes[0], std::min(sizes[1], sizes[2])) / 4.0);
    }
    if (skeleton >= 0) thin(none);
    if (show < 0) r.apply_mask(none, grow_fill, grow_remove ? CLWH_MASK_INVERT : 0);
    std::printf("{\"grow\": [%u, %u, %u], \"window\": [%d, %d], \"connectivity\": %d, \"mode\": \"%s\", \"fill\": %d, \"count\": %llu, "
                "\"bbox_lo\": [%u, %u, %u], \"bbox_hi\": [%u, %u, %u], \"mean\": %.6f, \"min\": %d, \"max\": %d",
                grow_seed[0], grow_seed[1], grow_seed[2], grow_lo, grow_hi, (grow_flags & CLWH_GROW_26) ? 26 : 6, show >= 0 ? "show" : grow_remove ? "remove" : "keep",
                grow_fill, (unsigned long long)g.count, g.bbox_lo[0], g.bbox_lo[1], g.bbox_lo[2], g.bbox_hi[0], g.bbox_hi[1], g.bbox_hi[2],
                g.count ? (double)g.sum / (double)g.count : 0.0, g.vmin, g.vmax);
    if (morph_op >= 0)
      std::printf(", \"morph\": {\"op\": \"%s\", \"radius_sq\": %u, \"weight\": [%u, %u, %u], \"count\": %llu}", kMorphNames[morph_op], m.radius_sq,
                  m.weight[0], m.weight[1], m.weight[2], (unsigned long long)m.count);
    std::printf("}\n");
    if (measure) {
      std::printf("{\"measure\": ");
      print_record(measured.stats);
      std::printf("}\n");
    }
    std::printf("%s%s", split_line.c_str(), skeleton_line.c_str());
    if (centerline)
      std::printf("{\"centerline\": {\"from\": [%u, %u, %u], \"to\": [%u, %u, %u], \"points\": %llu}}\n", grow_seed[0], grow_seed[1], grow_seed[2],
                  centerline_end[0], centerline_end[1], centerline_end[2], (unsigned long long)(line.size() / 3));
    if (profile) {
      const auto list = [](const char *name, const std::vector<double> &v, const char *tail) {
        std::printf("\"%s\": [", name);
        for (size_t k = 0; k < v.size(); ++k) std::printf("%s%.6f", k ? ", " : "", v[k]);
        std::printf("]%s", tail);
      };
      std::printf("{\"profile\": {");
      list("s_mm", sections.s_mm, ", ");
      list("area_mm2", sections.area_mm2, ", ");
      list("diameter_mm", sections.diameter_mm, ", ");
      std::printf("\"cut\": [");
      for (size_t k = 0; k < sections.cut.size(); ++k) std::printf("%s%s", k ? ", " : "", sections.cut[k] ? "true" : "false");
      std::printf("]}}\n");
    }
  }

  if (comps) {  // like --grow: everything below sees the masked volume
    ui_state none{argv[1], true, height, width, Position3D(0, 0, 0), {0.f, 0.f}, true};
    renderer::component_summary c = r.label_components(none, comps_lo, comps_hi, comps_flags, 8);
    uint64_t keep = c.n_components;  // the selected ranks are 1 .. keep
    if (comps_largest >= 0) keep = std::min<uint64_t>(keep, (uint64_t)comps_largest);
    if (comps_min >= 0) {
      // "at least N voxels" is a prefix of the ranks; if the eight records do not show its end, the whole table does
      renderer::component_summary all;
      const bool undecided = c.top.size() < c.n_components && !c.top.empty() && c.top.back().count >= (uint64_t)comps_min;
      if (undecided) all = r.label_components(none, comps_lo, comps_hi, comps_flags, (unsigned)c.n_components);
      const std::vector<clwh_label_component> &table = undecided ? all.top : c.top;
      keep = 0;
      while (keep < table.size() && table[keep].count >= (uint64_t)comps_min) ++keep;
    }
    // (no component selected: a rank nobody has gives the empty mask)
    if (keep > 0) r.select_components(none, 1, (uint32_t)keep);
    else r.select_components(none, (uint32_t)c.n_components + 1u, (uint32_t)c.n_components + 1u);
    renderer::morph_summary m;
    if (morph_op >= 0) m = r.morph_mask(none, morph_op, morph_radius);
    std::vector<clwh_region_stats> measured;
    clwh_mask_stats_result measured_mask{};
    if (measure && keep > 0) measured = r.measure_labels(none, (unsigned)std::min<uint64_t>(keep, 256));  // before the mask changes the volume
    if (measure && morph_op >= 0) measured_mask = r.measure_mask(none);  // the morphed mask is no longer the union of the ranks
    if (split_radius >= 0.0f) split(none, (comps_flags & CLWH_LABEL_26) != 0);  // (replaces the labelling: after it was measured)
    if (skeleton >= 0) thin(none);
    if (show < 0) r.apply_mask(none, comps_fill, comps_remove ? CLWH_MASK_INVERT : 0);
    if (show >= 0 && morph_op < 0 && keep > 0 && split_radius < 0.0f && skeleton < 0) {  // the labelling itself: a colour per rank (else the mask, which may be empty or morphed)
      show_source = renderer::OVERLAY_LABELS;
      show_style.id_hi = (uint32_t)keep;
    }
    std::printf("{\"components\": [%d, %d], \"connectivity\": %d, \"mode\": \"%s\", \"fill\": %d, \"n_components\": %llu, \"n_voxels\": %llu, "
                "\"selected\": [%u, %llu], \"largest\": [",
                comps_lo, comps_hi, (comps_flags & CLWH_LABEL_26) ? 26 : 6, show >= 0 ? "show" : comps_remove ? "remove" : "keep", comps_fill,
                (unsigned long long)c.n_components, (unsigned long long)c.n_voxels, keep > 0 ? 1u : 0u, (unsigned long long)keep);
    for (size_t k = 0; k < c.top.size(); ++k) {
      const clwh_label_component &t = c.top[k];
      std::printf("%s{\"count\": %llu, \"first\": [%u, %u, %u], \"bbox_lo\": [%u, %u, %u], \"bbox_hi\": [%u, %u, %u]}", k ? ", " : "",
                  (unsigned long long)t.count, t.first[0], t.first[1], t.first[2], t.bbox_lo[0], t.bbox_lo[1], t.bbox_lo[2], t.bbox_hi[0],
                  t.bbox_hi[1], t.bbox_hi[2]);
    }
    std::printf("]");
    if (morph_op >= 0)
      std::printf(", \"morph\": {\"op\": \"%s\", \"radius_sq\": %u, \"weight\": [%u, %u, %u], \"count\": %llu}", kMorphNames[morph_op], m.radius_sq,
                  m.weight[0], m.weight[1], m.weight[2], (unsigned long long)m.count);
    std::printf("}\n");
    if (measure) {
      std::printf("{\"measure_components\": [");
      for (size_t k = 0; k < measured.size(); ++k) {
        if (k) std::printf(", ");
        print_record(measured[k]);
      }
      std::printf("]");
      if (morph_op >= 0) {
        std::printf(", \"measure\": ");
        print_record(measured_mask.stats);
      }
      std::printf("}\n");
    }
    std::printf("%s%s", split_line.c_str(), skeleton_line.c_str());
  }

  if (shed) {  // like --grow: everything below sees the volume as this leaves it
    const auto &size = rv.get_volume_size();
    for (size_t k = 0; k < shed_seeds.size(); k += 4)
      for (int q = 0; q < 3; ++q)
        if (shed_seeds[k + q] >= size[q]) {
          std::cout << "The --watershed seed (" << shed_seeds[k] << ", " << shed_seeds[k + 1] << ", " << shed_seeds[k + 2] << ") lies outside the volume\n";
          return 1;
        }
    ui_state none{argv[1], true, height, width, Position3D(0, 0, 0), {0.f, 0.f}, true};
    const uint32_t n_ids = (uint32_t)(shed_seeds.size() / 4);
    const renderer::watershed_summary w = r.watershed_edges(none, shed_seeds, shed_flags, (uint32_t)shed_gmax, (uint32_t)shed_plateau);
    const std::vector<clwh_region_stats> records = r.measure_labels(none, n_ids);  // of the volume as loaded
    if (shed_keep >= 0 || shed_remove >= 0) {
      const uint32_t id = (uint32_t)(shed_keep >= 0 ? shed_keep : shed_remove);
      r.select_components(none, id, id);
      r.apply_mask(none, shed_fill, shed_remove >= 0 ? CLWH_MASK_INVERT : 0);
    }
    if (show >= 0) {
      show_source = renderer::OVERLAY_LABELS;
      show_style.id_hi = n_ids;
    }
    std::printf("{\"watershed\": {\"seeds\": %u, \"connectivity\": %d, \"gmax\": %ld, \"plateau\": %ld, \"mode\": \"%s\", \"fill\": %d, "
                "\"reached\": %llu, \"max_level\": %u, \"counts\": [",
                n_ids, (shed_flags & CLWH_GEO_26) ? 26 : 6, shed_gmax, shed_plateau,
                show >= 0 ? "show" : shed_keep >= 0 ? "keep" : shed_remove >= 0 ? "remove" : "none", shed_fill,
                (unsigned long long)w.result.reached, w.result.max_level);
    for (size_t k = 0; k < records.size(); ++k) std::printf("%s%llu", k ? ", " : "", (unsigned long long)records[k].count);
    std::printf("]}}\n");
  }

  if (mesh) {  // geometry, not frames: no transfer function, no distance field, no camera
    ui_state none{argv[1], true, height, width, Position3D(0, 0, 0), {0.f, 0.f}, true};
    const auto m0 = std::chrono::steady_clock::now();
    const mesh_data m = r.extract_mesh(none, mesh_value, mesh_below ? CLWH_MESH_BELOW : 0);
    const double mesh_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - m0).count();
    if (argc > 6 && !write_ply(argv[6], m)) {
      std::cout << "Cannot write '" << argv[6] << "'\n";
      return 1;
    }
    std::printf("{\"mesh\": %s, \"below\": %s, \"vertices\": %llu, \"triangles\": %llu, \"seconds\": %.6f}\n", std::to_string(mesh_value).c_str(),
                mesh_below ? "true" : "false", (unsigned long long)m.keys.size(), (unsigned long long)(m.triangles.size() / 3), mesh_seconds);
    return 0;
  }

  std::vector<tf_selection *> selection{new tf_rect_selection(0, 500.f, 1200.f, 0.0f, 4000.f)};
  emitter->next_event_code_set(tf_generate_source(rv.get_volume_stats(), selection));
  emitter->flush_changes();

  const int lut_first = -1024, lut_len = 4096;
  const std::vector<float> lut = tf_composite_lut(selection, lut_first, lut_len, 0.05f);

  ui_state state{argv[1], true, height, width, Position3D(-200, 200, -200), {0.9f, 6.183f}, true};
  const double scale = rv.get_volume_size()[0] / 512.0;  // the default camera is placed for a 512^3 volume
  state.position = Position3D(-200 * scale, 200 * scale, -200 * scale);
  const unsigned char *frame = nullptr;
  if (slice >= 0 && slice_centred) {  // the middle of the volume along the plane's normal
    static const int kNormalAxis[3] = {2, 1, 0};
    slice_position = (float)(((double)rv.get_volume_size()[kNormalAxis[slice]] - 1.0) / 2.0);
  }
  // renderer::render_frame seeds every pass from std::rand() and the application never calls srand
  // (app/renderer.cpp:142).  The ROCm runtime draws from rand() while it initialises, so the sequence is put
  // back to the never-seeded state here to make the frames reproducible (1804289383, 846930886, ...).
  renderer::curve_frame_set curve_rows;  // --curved: `height` rows, the curve's stations first
  if (curved) {
    if (curve.size() < 6) {
      std::cout << "--curved: the centreline is empty\n";
      return 1;
    }
    const auto &sizes = rv.get_voxel_sizes();
    const double spacing[3] = {(double)sizes[0], (double)sizes[1], (double)sizes[2]};
    const double pixel_mm = (double)curved_window / (double)std::max(width, 1);
    curve_rows = renderer::curve_frames(std::vector<double>(curve.begin(), curve.end()), spacing, width, pixel_mm, pixel_mm, 8,
                                        (double)curved_angle * 3.141592653589793 / 180.0, curved_slab, pixel_mm / 2.0);
    const size_t have = curve_rows.rows.size() / 9, want = (size_t)std::max(height, 0);
    curve_rows.rows.resize(want * 9, 0.0f);
    for (size_t j = have; j < want; ++j) curve_rows.rows[9 * j] = curve_rows.rows[9 * j + 1] = curve_rows.rows[9 * j + 2] = -1.0f;
    curve_rows.n = std::min(curve_rows.n, want);
  }
  std::srand(1);
  const auto t0 = std::chrono::steady_clock::now();
  for (int f = 0; f < frames; ++f) {
    bool changed = false;
    state.cam_changed = true;  // progressive refinement: keep sampling the same view
    if (curved)
      frame = static_cast<const unsigned char *>(r.render_curved(state, curve_rows, width, curved_mode, curved_slab,
                                                                 (float)((double)curved_window / (double)width / 2.0), 0.0f, 4000.0f));
    else if (slice >= 0)
      frame = static_cast<const unsigned char *>(r.render_slice(state, slice, slice_position, slice_mode, slice_slab, 0.5f, 0.0f, 4000.0f));
    else if (isosurface)
      frame = static_cast<const unsigned char *>(r.render_isosurface(state, iso_value, iso_below ? CLWH_ISO_BELOW : 0));
    else if (composite >= 0)
      frame = static_cast<const unsigned char *>(
          r.render_composite(state, lut, lut_first, lut_len, 0.5f, 0.95f, composite == 1 ? CLWH_COMP_SHADE : 0, 0.3f));
    else if (projection >= 0)
      frame = static_cast<const unsigned char *>(r.render_projection(state, projection, 0.0f, 4000.0f));
    else
      frame = static_cast<const unsigned char *>(emitter->render_frame(state, changed));
    if (show >= 0 && slice >= 0)
      frame = static_cast<const unsigned char *>(r.overlay_slice(state, show_source, slice, slice_position, slice_slab, 0.5f, show_style));
    else if (show >= 0)
      frame = static_cast<const unsigned char *>(r.overlay_camera(state, show_source, 0.5f, show_style));
  }
  const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

  std::uint64_t checksum = 1469598103934665603ull;  // FNV-1a over the launched region of the frame
  for (int y = 0; y < height; ++y)
    for (int x = 0; x < width * 4; ++x) {
      checksum ^= frame[(size_t)y * SCREEN_WIDTH * 4 + x];
      checksum *= 1099511628211ull;
    }
  if (argc > 6) {
    std::ofstream ppm(argv[6], std::ios::binary);
    ppm << "P6\n" << width << " " << height << "\n255\n";
    for (int y = height - 1; y >= 0; --y)  // row 0 is the bottom of the screen
      for (int x = 0; x < width; ++x) ppm.write(reinterpret_cast<const char *>(frame + ((size_t)y * SCREEN_WIDTH + x) * 4), 3);
  }
  static const char *const kProjectionNames[] = {"max", "min", "mean"};
  static const char *const kSliceNames[] = {"axial", "coronal", "sagittal"};
  std::printf("{\"frames\": %d, \"width\": %d, \"height\": %d, \"seconds\": %.6f, \"ms_per_frame\": %.4f, \"frame_fnv1a\": \"%016llx\"%s%s%s%s%s%s%s%s%s%s%s%s}\n",
              frames, width, height, seconds, seconds * 1e3 / frames, (unsigned long long)checksum,
              projection >= 0 ? ", \"projection\": \"" : "", projection >= 0 ? kProjectionNames[projection] : "", projection >= 0 ? "\"" : "",
              composite >= 0 ? ", \"composite\": \"" : "", composite >= 0 ? (composite == 1 ? "shaded" : "plain") : "", composite >= 0 ? "\"" : "",
              isosurface ? (", \"isosurface\": " + std::to_string(iso_value) + ", \"below\": " + (iso_below ? "true" : "false")).c_str() : "",
              slice >= 0 ? (std::string(", \"slice\": \"") + kSliceNames[slice] + "\", \"position\": " + std::to_string(slice_position) +
                            ", \"slab\": " + std::to_string(slice_slab) + ", \"mode\": \"" + kProjectionNames[slice_mode] + "\"").c_str() : "",
              curved ? (std::string(", \"curved\": {\"window_mm\": ") + std::to_string(curved_window) + ", \"angle\": " + std::to_string(curved_angle) +
                        ", \"slab\": " + std::to_string(curved_slab) + ", \"mode\": \"" + kProjectionNames[curved_mode] +
                        "\", \"stations\": " + std::to_string(curve_rows.n) + "}").c_str() : "",
              show >= 0 ? ", \"overlay\": \"" : "", show >= 0 ? kShowNames[show] : "", show >= 0 ? "\"" : "");
  for (tf_selection *s : selection) delete s;
  return 0;
}
