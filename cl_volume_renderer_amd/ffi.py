"""ctypes binding of the product's C ABI (include/clwh.h, libclwhip.so).

There is no CPU fallback: if the HIP library is missing or a call fails, this raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# CLWH_LIBRARY: another build of the same library (tools/ experiments: timing probes, tuning variants)
LIB_PATH = os.environ.get("CLWH_LIBRARY") or os.path.join(_HERE, "libclwhip.so")

OK = 0
ELEM_S8, ELEM_S16, ELEM_S32, ELEM_U8, ELEM_U16, ELEM_U32, ELEM_F32 = range(7)
ARG_MEM, ARG_I32, ARG_U32, ARG_F32, ARG_I64, ARG_U64, ARG_F64 = range(7)
ACCUM_VOXEL_CACHE, ACCUM_IMAGE_SPACE = 0, 1
DERIVED_SCENE, DERIVED_CAMERA, DERIVED_PROJECTION = 1, 2, 4
PROJ_MAX, PROJ_MIN, PROJ_MEAN = 0, 1, 2
PROJ_DENSE = 1
COMP_DENSE, COMP_SHADE = 1, 2
ISO_DENSE, ISO_BELOW = 1, 2
SLICE_MAX, SLICE_MIN, SLICE_MEAN = 0, 1, 2
SLICE_DENSE = 1
CURVED_DENSE = 1
PROFILE_CONNECTED = 1
MESH_DENSE, MESH_BELOW = 1, 2
GROW_26, GROW_FROM_MASK, GROW_DENSE = 1, 2, 4
GROW_MAX_SEEDS = 65536
LABEL_26, LABEL_FROM_MASK = 1, 2
DIST_NONE = 0xFFFFFFFF
DIST_TO_CLEAR = 1
GEO_26, GEO_FROM_LABELS, GEO_DENSE = 1, 2, 4
GEO_CAP_MAX = 0xFFFF0000
COST_CAP_MAX = 0xFF000000
COST_SRC_U32, COST_SRC_VALUE, COST_SRC_GRADIENT = 0, 1, 2
WATERSHED_PLATEAU_MAX, WATERSHED_LEVEL_MAX = 65534, 65535
MORPH_DILATE, MORPH_ERODE, MORPH_OPEN, MORPH_CLOSE = 0, 1, 2, 3
MASK_AND, MASK_OR, MASK_XOR, MASK_ANDNOT, MASK_NOT = 0, 1, 2, 3, 4
MASK_INVERT = 1
THIN_KEEP_ENDS, THIN_DENSE = 1, 2
FILTER_MEDIAN, FILTER_MIN, FILTER_MAX, FILTER_SMOOTH = 0, 1, 2, 3
FILTER_MAX_RADIUS, FILTER_WEIGHT_SUM = 16, 4096
REGION_MASK, REGION_LABELS = 0, 1
OVERLAY_FILL, OVERLAY_OUTLINE, OVERLAY_DENSE = 1, 2, 4
SHADE_LIGHT, SHADE_AO = 0, 1
(PROBE_ARITH, PROBE_HASH, PROBE_HEMISPHERE, PROBE_RAY, PROBE_CUT, PROBE_ENV_EXACT, PROBE_ENV_FAST, PROBE_ENV_APPROX, PROBE_TONE,
 PROBE_TAPS, PROBE_HULL) = range(11)
# clwh_debug_device_probe: (words per input record, words per output record) of each probe
PROBE_WORDS = ((6, 12), (1, 1), (7, 6), (10, 3), (6, 4), (3, 1), (3, 2), (3, 2), (4, 1), (3, 3), (5, 5))
SCENE_HIT_RECORDS, SCENE_STEP_BYTES, SCENE_BRICK_MIN = range(3)            # clwh_debug_packed_scene
VIEW_BRICKS, VIEW_TABLE, VIEW_DILATED, VIEW_COARSE = range(4)               # clwh_debug_view_data
TIMERS = ("bounce", "primary", "fixup", "resolve", "repack", "ao")
MAX_SEEDS = 64
TF_MAX_RULES = 16

_ELEM_OF_DTYPE = {
    np.dtype(np.int8): ELEM_S8, np.dtype(np.int16): ELEM_S16, np.dtype(np.int32): ELEM_S32,
    np.dtype(np.uint8): ELEM_U8, np.dtype(np.uint16): ELEM_U16, np.dtype(np.uint32): ELEM_U32,
    np.dtype(np.float32): ELEM_F32,
}


class ClwhError(RuntimeError):
    def __init__(self, status, where):
        self.status = status
        name = lib().clwh_strerror(status).decode()
        super().__init__("%s failed: %s (hip error %d)" % (where, name, lib().clwh_last_hip_error()))


class _ArgValue(C.Union):
    _fields_ = [("mem", C.c_void_p), ("i32", C.c_int32), ("u32", C.c_uint32), ("f32", C.c_float),
                ("i64", C.c_int64), ("u64", C.c_uint64), ("f64", C.c_double)]


class Arg(C.Structure):
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("v", _ArgValue)]


class TfRule(C.Structure):
    _fields_ = [("v_lo", C.c_int32), ("v_hi", C.c_int32), ("g_lo", C.c_int32), ("g_hi", C.c_int32),
                ("use_gradient", C.c_int32), ("writes_color", C.c_int32), ("terminal", C.c_int32),
                ("color", C.c_int32 * 4)]


class Tf(C.Structure):
    _fields_ = [("n", C.c_int32), ("rules", TfRule * TF_MAX_RULES)]

    def as_tuples(self):
        return [(r.v_lo, r.v_hi, r.g_lo, r.g_hi, r.use_gradient, r.writes_color, r.terminal, tuple(r.color))
                for r in list(self.rules)[: self.n]]


class RenderDesc(C.Structure):
    _fields_ = [
        ("frame", C.c_void_p), ("volume", C.c_void_p), ("sdf", C.c_void_p), ("env", C.c_void_p),
        ("buffer_volume", C.c_void_p),
        ("cam_pos", C.c_float * 3), ("cam_dir", C.c_float * 3), ("seed", C.c_int32),
        ("width", C.c_uint32), ("height", C.c_uint32),
        ("accum_mode", C.c_int32), ("accum", C.c_void_p),
        ("tile_rank", C.c_int32), ("tile_world", C.c_int32),
        ("write_frame", C.c_int32),
        ("hit_index", C.c_void_p), ("contrib", C.c_void_p),
        ("n_seeds", C.c_int32), ("seeds", C.c_int32 * 64),
        ("shading", C.c_int32), ("resolve_only", C.c_int32),
    ]


class ProjectionDesc(C.Structure):
    _fields_ = [
        ("frame", C.c_void_p), ("volume", C.c_void_p),
        ("cam_pos", C.c_float * 3), ("cam_dir", C.c_float * 3),
        ("width", C.c_uint32), ("height", C.c_uint32),
        ("mode", C.c_int32), ("flags", C.c_int32),
        ("step", C.c_float), ("t_near", C.c_float), ("t_far", C.c_float),
        ("window_center", C.c_float), ("window_width", C.c_float),
        ("values", C.c_void_p), ("t_extreme", C.c_void_p),
    ]


class CompositeDesc(C.Structure):
    _fields_ = [
        ("frame", C.c_void_p), ("volume", C.c_void_p),
        ("cam_pos", C.c_float * 3), ("cam_dir", C.c_float * 3),
        ("width", C.c_uint32), ("height", C.c_uint32),
        ("flags", C.c_int32),
        ("step", C.c_float), ("t_near", C.c_float), ("t_far", C.c_float),
        ("lut", C.c_void_p), ("lut_first", C.c_int32), ("lut_len", C.c_int32),
        ("alpha_stop", C.c_float), ("ambient", C.c_float),
        ("rgba", C.c_void_p), ("t_first", C.c_void_p), ("t_stop", C.c_void_p),
    ]


class IsosurfaceDesc(C.Structure):
    _fields_ = [
        ("frame", C.c_void_p), ("volume", C.c_void_p),
        ("cam_pos", C.c_float * 3), ("cam_dir", C.c_float * 3),
        ("width", C.c_uint32), ("height", C.c_uint32),
        ("flags", C.c_int32),
        ("step", C.c_float), ("t_near", C.c_float), ("t_far", C.c_float),
        ("iso", C.c_float), ("refine", C.c_int32),
        ("color", C.c_float * 3), ("ambient", C.c_float),
        ("t_hit", C.c_void_p), ("normal", C.c_void_p),
    ]


class SliceDesc(C.Structure):
    _fields_ = [
        ("frame", C.c_void_p), ("volume", C.c_void_p),
        ("origin", C.c_float * 3), ("du", C.c_float * 3), ("dv", C.c_float * 3), ("normal", C.c_float * 3),
        ("width", C.c_uint32), ("height", C.c_uint32),
        ("mode", C.c_int32), ("flags", C.c_int32),
        ("slab_samples", C.c_int32), ("step", C.c_float),
        ("window_center", C.c_float), ("window_width", C.c_float),
        ("values", C.c_void_p), ("t_extreme", C.c_void_p),
    ]


class CurvedDesc(C.Structure):
    _fields_ = [
        ("frame", C.c_void_p), ("volume", C.c_void_p),
        ("rows", C.c_void_p),
        ("width", C.c_uint32), ("height", C.c_uint32),
        ("mode", C.c_int32), ("flags", C.c_int32),
        ("slab_samples", C.c_int32), ("step", C.c_float),
        ("window_center", C.c_float), ("window_width", C.c_float),
        ("values", C.c_void_p), ("t_extreme", C.c_void_p),
    ]


class SectionRecord(C.Structure):
    _fields_ = [("count", C.c_uint32), ("sum_x", C.c_uint32), ("sum_k", C.c_uint32), ("border", C.c_uint32)]


# the same record as a numpy dtype (scene.SECTION_RECORD_DTYPE): what Context.curve_profile returns
SECTION_RECORD_DTYPE = np.dtype([("count", np.uint32), ("sum_x", np.uint32), ("sum_k", np.uint32), ("border", np.uint32)])
assert SECTION_RECORD_DTYPE.itemsize == C.sizeof(SectionRecord) == 16


class CurveProfileDesc(C.Structure):
    _fields_ = [
        ("mask", C.c_void_p),
        ("dims", C.c_uint32 * 3),
        ("rows", C.c_void_p),
        ("n_rows", C.c_uint32), ("width", C.c_uint32),
        ("slab_samples", C.c_int32), ("step", C.c_float),
        ("flags", C.c_int32),
        ("records", C.c_void_p),
    ]


class MeshDesc(C.Structure):
    _fields_ = [
        ("volume", C.c_void_p),
        ("iso", C.c_float), ("flags", C.c_int32),
        ("box_lo", C.c_uint32 * 3), ("box_hi", C.c_uint32 * 3),
        ("positions", C.c_void_p), ("normals", C.c_void_p), ("keys", C.c_void_p), ("triangles", C.c_void_p),
        ("vertex_capacity", C.c_uint64), ("triangle_capacity", C.c_uint64),
        ("n_vertices", C.POINTER(C.c_uint64)), ("n_triangles", C.POINTER(C.c_uint64)),
    ]


class GrowResult(C.Structure):
    _fields_ = [
        ("count", C.c_uint64),
        ("bbox_lo", C.c_uint32 * 3), ("bbox_hi", C.c_uint32 * 3),
        ("sum", C.c_int64), ("sum_sq", C.c_uint64),
        ("vmin", C.c_int32), ("vmax", C.c_int32),
        ("rounds", C.c_uint32), ("reserved", C.c_uint32),
    ]

    def as_dict(self):
        """the contract's fields (`rounds` is informational and left out)"""
        return {"count": int(self.count), "bbox_lo": tuple(self.bbox_lo), "bbox_hi": tuple(self.bbox_hi), "sum": int(self.sum),
                "sum_sq": int(self.sum_sq), "vmin": int(self.vmin), "vmax": int(self.vmax)}


class GrowDesc(C.Structure):
    _fields_ = [
        ("volume", C.c_void_p), ("mask", C.c_void_p),
        ("lo", C.c_int32), ("hi", C.c_int32), ("flags", C.c_int32),
        ("n_seeds", C.c_uint32), ("seeds", C.POINTER(C.c_uint32)),
        ("box_lo", C.c_uint32 * 3), ("box_hi", C.c_uint32 * 3),
        ("result", C.POINTER(GrowResult)),
    ]


class ApplyMaskDesc(C.Structure):
    _fields_ = [
        ("volume_in", C.c_void_p), ("volume_out", C.c_void_p), ("mask", C.c_void_p),
        ("fill", C.c_int32), ("flags", C.c_int32),
    ]


class FilterDesc(C.Structure):
    _fields_ = [
        ("volume_in", C.c_void_p), ("volume_out", C.c_void_p), ("mask", C.c_void_p),
        ("kind", C.c_int32), ("flags", C.c_int32), ("radius", C.c_uint32 * 3),
        ("weights", C.POINTER(C.c_uint16) * 3),
    ]


assert C.sizeof(FilterDesc) == 72


class LabelComponent(C.Structure):
    _fields_ = [
        ("count", C.c_uint64),
        ("first", C.c_uint32 * 3), ("bbox_lo", C.c_uint32 * 3), ("bbox_hi", C.c_uint32 * 3),
        ("reserved", C.c_uint32),
    ]

    def as_dict(self):
        return {"count": int(self.count), "first": tuple(self.first), "bbox_lo": tuple(self.bbox_lo), "bbox_hi": tuple(self.bbox_hi)}


# the same record as a numpy dtype: what Context.label_components returns the table in
LABEL_COMPONENT_DTYPE = np.dtype([("count", np.uint64), ("first", np.uint32, (3,)), ("bbox_lo", np.uint32, (3,)),
                                  ("bbox_hi", np.uint32, (3,)), ("reserved", np.uint32)])
assert LABEL_COMPONENT_DTYPE.itemsize == C.sizeof(LabelComponent) == 48


class LabelResult(C.Structure):
    _fields_ = [("n_components", C.c_uint64), ("n_voxels", C.c_uint64), ("passes", C.c_uint32), ("reserved", C.c_uint32)]

    def as_dict(self):
        """the contract's fields (`passes` is informational and left out)"""
        return {"n_components": int(self.n_components), "n_voxels": int(self.n_voxels)}


class LabelDesc(C.Structure):
    _fields_ = [
        ("volume", C.c_void_p), ("labels", C.c_void_p), ("components", C.c_void_p), ("component_capacity", C.c_uint64),
        ("mask", C.c_void_p),
        ("lo", C.c_int32), ("hi", C.c_int32), ("flags", C.c_int32),
        ("box_lo", C.c_uint32 * 3), ("box_hi", C.c_uint32 * 3),
        ("result", C.POINTER(LabelResult)),
    ]


class LabelsToMaskDesc(C.Structure):
    _fields_ = [("labels", C.c_void_p), ("mask", C.c_void_p), ("dims", C.c_uint32 * 3), ("rank_lo", C.c_uint32), ("rank_hi", C.c_uint32)]


class DistanceDesc(C.Structure):
    _fields_ = [("mask", C.c_void_p), ("dist", C.c_void_p), ("dims", C.c_uint32 * 3), ("weight", C.c_uint32 * 3), ("cap", C.c_uint32),
                ("flags", C.c_int32)]


class MorphDesc(C.Structure):
    _fields_ = [("mask_in", C.c_void_p), ("mask_out", C.c_void_p), ("dims", C.c_uint32 * 3), ("weight", C.c_uint32 * 3),
                ("radius_sq", C.c_uint32), ("op", C.c_int32), ("flags", C.c_int32)]


class GeodesicResult(C.Structure):
    _fields_ = [("reached", C.c_uint64), ("max_dist", C.c_uint32), ("rounds", C.c_uint32)]

    def as_dict(self):
        """the contract's fields (`rounds` is informational and left out)"""
        return {"reached": int(self.reached), "max_dist": int(self.max_dist)}


class GeodesicDesc(C.Structure):
    _fields_ = [
        ("domain", C.c_void_p), ("seed_labels", C.c_void_p), ("dist", C.c_void_p), ("labels", C.c_void_p),
        ("dims", C.c_uint32 * 3), ("weight_face", C.c_uint32 * 3), ("weight_edge", C.c_uint32 * 3), ("weight_corner", C.c_uint32),
        ("cap", C.c_uint32), ("flags", C.c_int32),
        ("n_seeds", C.c_uint32), ("seeds", C.POINTER(C.c_uint32)),
        ("result", C.POINTER(GeodesicResult)),
    ]


class GeodesicTraceDesc(C.Structure):
    _fields_ = [
        ("dist", C.c_void_p), ("labels", C.c_void_p), ("points", C.c_void_p), ("capacity", C.c_uint64),
        ("dims", C.c_uint32 * 3), ("weight_face", C.c_uint32 * 3), ("weight_edge", C.c_uint32 * 3), ("weight_corner", C.c_uint32),
        ("flags", C.c_int32), ("target", C.c_uint32 * 3),
        ("n_points", C.POINTER(C.c_uint64)),
    ]


assert C.sizeof(GeodesicDesc) == 104 and C.sizeof(GeodesicTraceDesc) == 96 and C.sizeof(GeodesicResult) == 16


class CostGeodesicDesc(C.Structure):
    _fields_ = [
        ("cost", C.c_void_p), ("domain", C.c_void_p), ("seed_labels", C.c_void_p), ("dist", C.c_void_p), ("labels", C.c_void_p),
        ("dims", C.c_uint32 * 3), ("mult_face", C.c_uint32 * 3), ("mult_edge", C.c_uint32 * 3), ("mult_corner", C.c_uint32),
        ("cap", C.c_uint32), ("flags", C.c_int32),
        ("n_seeds", C.c_uint32), ("seeds", C.POINTER(C.c_uint32)),
        ("result", C.POINTER(GeodesicResult)),
    ]


class CostTraceDesc(C.Structure):
    _fields_ = [
        ("cost", C.c_void_p), ("dist", C.c_void_p), ("labels", C.c_void_p), ("points", C.c_void_p), ("capacity", C.c_uint64),
        ("dims", C.c_uint32 * 3), ("mult_face", C.c_uint32 * 3), ("mult_edge", C.c_uint32 * 3), ("mult_corner", C.c_uint32),
        ("flags", C.c_int32), ("target", C.c_uint32 * 3),
        ("n_points", C.POINTER(C.c_uint64)),
    ]


class CostFieldDesc(C.Structure):
    _fields_ = [
        ("source", C.c_void_p), ("domain", C.c_void_p), ("cost", C.c_void_p), ("table", C.POINTER(C.c_uint16)),
        ("lo", C.c_int64), ("dims", C.c_uint32 * 3), ("n", C.c_uint32), ("shift", C.c_uint32), ("kind", C.c_int32), ("flags", C.c_int32),
    ]


assert C.sizeof(CostGeodesicDesc) == 112 and C.sizeof(CostTraceDesc) == 104 and C.sizeof(CostFieldDesc) == 72


class WatershedResult(C.Structure):
    _fields_ = [("reached", C.c_uint64), ("max_level", C.c_uint32), ("rounds", C.c_uint32)]

    def as_dict(self):
        """the contract's fields (`rounds` is informational and left out)"""
        return {"reached": int(self.reached), "max_level": int(self.max_level)}


class WatershedDesc(C.Structure):
    _fields_ = [
        ("cost", C.c_void_p), ("domain", C.c_void_p), ("seed_labels", C.c_void_p), ("level", C.c_void_p), ("labels", C.c_void_p),
        ("dims", C.c_uint32 * 3), ("plateau_cap", C.c_uint32), ("level_cap", C.c_uint32), ("flags", C.c_int32),
        ("n_seeds", C.c_uint32), ("seeds", C.POINTER(C.c_uint32)),
        ("result", C.POINTER(WatershedResult)),
    ]


assert C.sizeof(WatershedDesc) == 88 and C.sizeof(WatershedResult) == 16


class ThinResult(C.Structure):
    _fields_ = [("count_in", C.c_uint64), ("count_out", C.c_uint64), ("deleted", C.c_uint64), ("iterations", C.c_uint32),
                ("reserved", C.c_uint32)]

    def as_dict(self):
        """the contract's fields: all four are functions of the input"""
        return {"count_in": int(self.count_in), "count_out": int(self.count_out), "deleted": int(self.deleted),
                "iterations": int(self.iterations)}


class ThinDesc(C.Structure):
    _fields_ = [("mask_in", C.c_void_p), ("mask_out", C.c_void_p), ("anchors", C.c_void_p), ("dims", C.c_uint32 * 3),
                ("flags", C.c_int32), ("max_iterations", C.c_uint32), ("reserved", C.c_uint32), ("result", C.POINTER(ThinResult))]


class MaskPointsDesc(C.Structure):
    _fields_ = [("mask", C.c_void_p), ("points", C.c_void_p), ("map", C.c_void_p), ("values", C.c_void_p), ("dims", C.c_uint32 * 3),
                ("flags", C.c_int32), ("capacity", C.c_uint64), ("n_points", C.POINTER(C.c_uint64))]


assert C.sizeof(ThinDesc) == 56 and C.sizeof(ThinResult) == 32 and C.sizeof(MaskPointsDesc) == 64


class MaskCombineDesc(C.Structure):
    _fields_ = [("a", C.c_void_p), ("b", C.c_void_p), ("out", C.c_void_p), ("dims", C.c_uint32 * 3), ("op", C.c_int32)]


class RegionStats(C.Structure):
    _fields_ = [
        ("count", C.c_uint64), ("sum", C.c_int64), ("sum_sq", C.c_uint64),
        ("vmin", C.c_int32), ("vmax", C.c_int32),
        ("sum_pos", C.c_uint64 * 3),
        ("bbox_lo", C.c_uint32 * 3), ("bbox_hi", C.c_uint32 * 3),
        ("faces", C.c_uint32 * 3), ("border_faces", C.c_uint32 * 3),
    ]

    def as_dict(self):
        return {"count": int(self.count), "sum": int(self.sum), "sum_sq": int(self.sum_sq), "vmin": int(self.vmin), "vmax": int(self.vmax),
                "sum_pos": tuple(int(v) for v in self.sum_pos), "bbox_lo": tuple(self.bbox_lo), "bbox_hi": tuple(self.bbox_hi),
                "faces": tuple(self.faces), "border_faces": tuple(self.border_faces)}


# the same record as a numpy dtype (scene.REGION_STATS_DTYPE): what Context.label_statistics' table holds
REGION_STATS_DTYPE = np.dtype([("count", np.uint64), ("sum", np.int64), ("sum_sq", np.uint64), ("vmin", np.int32), ("vmax", np.int32),
                               ("sum_pos", np.uint64, (3,)), ("bbox_lo", np.uint32, (3,)), ("bbox_hi", np.uint32, (3,)),
                               ("faces", np.uint32, (3,)), ("border_faces", np.uint32, (3,))])
assert REGION_STATS_DTYPE.itemsize == C.sizeof(RegionStats) == 104
LABEL_STATS_MAX_CAPACITY = 1 << 24


class MaskStatsResult(C.Structure):
    _fields_ = [("stats", RegionStats), ("hist_below", C.c_uint64), ("hist_above", C.c_uint64)]


class MaskStatsDesc(C.Structure):
    _fields_ = [("volume", C.c_void_p), ("mask", C.c_void_p), ("hist", C.c_void_p), ("hist_lo", C.c_int32), ("bin_width", C.c_int32),
                ("n_bins", C.c_int32), ("flags", C.c_int32), ("result", C.POINTER(MaskStatsResult))]


class LabelStatsDesc(C.Structure):
    _fields_ = [("volume", C.c_void_p), ("labels", C.c_void_p), ("stats", C.c_void_p), ("capacity", C.c_uint64), ("flags", C.c_int32),
                ("reserved", C.c_int32)]


class OverlayRegion(C.Structure):
    _fields_ = [("buffer", C.c_void_p), ("kind", C.c_int32), ("dims", C.c_uint32 * 3), ("id_lo", C.c_uint32), ("id_hi", C.c_uint32)]


class OverlayPaint(C.Structure):
    _fields_ = [("palette", C.c_void_p), ("n_colours", C.c_uint32), ("flags", C.c_int32), ("fill_alpha", C.c_uint32),
                ("outline_alpha", C.c_uint32), ("ids", C.c_void_p), ("t_first", C.c_void_p)]


class OverlaySliceDesc(C.Structure):
    _fields_ = [
        ("frame", C.c_void_p), ("region", OverlayRegion), ("paint", OverlayPaint),
        ("origin", C.c_float * 3), ("du", C.c_float * 3), ("dv", C.c_float * 3), ("normal", C.c_float * 3),
        ("width", C.c_uint32), ("height", C.c_uint32),
        ("slab_samples", C.c_int32), ("step", C.c_float),
    ]


class OverlayCameraDesc(C.Structure):
    _fields_ = [
        ("frame", C.c_void_p), ("region", OverlayRegion), ("paint", OverlayPaint),
        ("cam_pos", C.c_float * 3), ("cam_dir", C.c_float * 3),
        ("width", C.c_uint32), ("height", C.c_uint32),
        ("step", C.c_float), ("t_near", C.c_float), ("t_far", C.c_float), ("reserved", C.c_int32),
    ]


# every symbol include/clwh.h declares: (name, restype, argtypes)
_SIZE3 = C.POINTER(C.c_size_t)
_PROTOTYPES = [
    ("clwh_ctx_create", C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    ("clwh_ctx_create_on_stream", C.c_int, [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    ("clwh_ctx_destroy", C.c_int, [C.c_void_p]),
    ("clwh_ctx_finish", C.c_int, [C.c_void_p]),
    ("clwh_ctx_stream", C.c_void_p, [C.c_void_p]),
    ("clwh_ctx_device", C.c_int, [C.c_void_p]),
    ("clwh_mem_create", C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p)]),
    ("clwh_mem_wrap", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    ("clwh_image_create", C.c_int, [C.c_void_p, _SIZE3, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    ("clwh_image_wrap", C.c_int, [C.c_void_p, C.c_void_p, _SIZE3, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    ("clwh_mem_push", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    ("clwh_mem_pull", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    ("clwh_mem_release", C.c_int, [C.c_void_p]),
    ("clwh_host_register", C.c_int, [C.c_void_p, C.c_size_t]),
    ("clwh_host_unregister", C.c_int, [C.c_void_p]),
    ("clwh_mem_device_ptr", C.c_void_p, [C.c_void_p]),
    ("clwh_mem_size", C.c_size_t, [C.c_void_p]),
    ("clwh_mem_mark_dirty", C.c_int, [C.c_void_p]),
    ("clwh_kernel_get", C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]),
    ("clwh_kernel_release", C.c_int, [C.c_void_p]),
    ("clwh_launch", C.c_int, [C.c_void_p, _SIZE3, _SIZE3, C.POINTER(Arg), C.c_int]),
    ("clwh_render", C.c_int, [C.c_void_p, C.POINTER(RenderDesc)]),
    ("clwh_cache_len", C.c_int64, [C.c_uint32, C.c_uint32, C.c_uint32]),
    ("clwh_accum_len", C.c_int64, [C.c_uint32, C.c_uint32, C.c_int32]),
    ("clwh_accum_resolve", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32, C.c_void_p,
                                     C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    ("clwh_accum_resolve_tiles", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_void_p,
                                           C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    ("clwh_frame_from_tiles", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32, C.c_void_p]),
    ("clwh_ctx_invalidate_derived", C.c_int, [C.c_void_p, C.c_int]),
    ("clwh_ctx_scene_info", C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]),
    ("clwh_render_projection", C.c_int, [C.c_void_p, C.POINTER(ProjectionDesc)]),
    ("clwh_render_composite", C.c_int, [C.c_void_p, C.POINTER(CompositeDesc)]),
    ("clwh_render_isosurface", C.c_int, [C.c_void_p, C.POINTER(IsosurfaceDesc)]),
    ("clwh_render_slice", C.c_int, [C.c_void_p, C.POINTER(SliceDesc)]),
    ("clwh_render_curved", C.c_int, [C.c_void_p, C.POINTER(CurvedDesc)]),
    ("clwh_curve_profile", C.c_int, [C.c_void_p, C.POINTER(CurveProfileDesc)]),
    ("clwh_mesh_isosurface", C.c_int, [C.c_void_p, C.POINTER(MeshDesc)]),
    ("clwh_segment_grow", C.c_int, [C.c_void_p, C.POINTER(GrowDesc)]),
    ("clwh_volume_apply_mask", C.c_int, [C.c_void_p, C.POINTER(ApplyMaskDesc)]),
    ("clwh_segment_label", C.c_int, [C.c_void_p, C.POINTER(LabelDesc)]),
    ("clwh_labels_to_mask", C.c_int, [C.c_void_p, C.POINTER(LabelsToMaskDesc)]),
    ("clwh_mask_distance", C.c_int, [C.c_void_p, C.POINTER(DistanceDesc)]),
    ("clwh_mask_morph", C.c_int, [C.c_void_p, C.POINTER(MorphDesc)]),
    ("clwh_mask_combine", C.c_int, [C.c_void_p, C.POINTER(MaskCombineDesc)]),
    ("clwh_volume_filter", C.c_int, [C.c_void_p, C.POINTER(FilterDesc)]),
    ("clwh_mask_thin", C.c_int, [C.c_void_p, C.POINTER(ThinDesc)]),
    ("clwh_mask_points", C.c_int, [C.c_void_p, C.POINTER(MaskPointsDesc)]),
    ("clwh_mask_geodesic", C.c_int, [C.c_void_p, C.POINTER(GeodesicDesc)]),
    ("clwh_geodesic_trace", C.c_int, [C.c_void_p, C.POINTER(GeodesicTraceDesc)]),
    ("clwh_cost_geodesic", C.c_int, [C.c_void_p, C.POINTER(CostGeodesicDesc)]),
    ("clwh_watershed", C.c_int, [C.c_void_p, C.POINTER(WatershedDesc)]),
    ("clwh_cost_trace", C.c_int, [C.c_void_p, C.POINTER(CostTraceDesc)]),
    ("clwh_cost_from_field", C.c_int, [C.c_void_p, C.POINTER(CostFieldDesc)]),
    ("clwh_mask_statistics", C.c_int, [C.c_void_p, C.POINTER(MaskStatsDesc)]),
    ("clwh_label_statistics", C.c_int, [C.c_void_p, C.POINTER(LabelStatsDesc)]),
    ("clwh_overlay_slice", C.c_int, [C.c_void_p, C.POINTER(OverlaySliceDesc)]),
    ("clwh_overlay_camera", C.c_int, [C.c_void_p, C.POINTER(OverlayCameraDesc)]),
    ("clwh_sdf_build", C.c_int, [C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int32)]),
    ("clwh_buffer_reset", C.c_int, [C.c_void_p, C.c_void_p]),
    ("clwh_cache_exchange_plan", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    ("clwh_cache_apply_contributions", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]),
    ("clwh_cache_exchange_plan_release", C.c_int, [C.c_void_p]),
    ("clwh_tf_parse", C.c_int, [C.c_char_p, C.POINTER(Tf)]),
    ("clwh_debug_float_conversions", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    ("clwh_debug_wave_min", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    ("clwh_debug_device_probe", C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]),
    ("clwh_debug_macro_table", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_int32)]),
    ("clwh_debug_packed_scene", C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.POINTER(C.c_int32)]),
    ("clwh_debug_view_data", C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.POINTER(C.c_int32)]),
    ("clwh_debug_start_table", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_int32)]),
    ("clwh_debug_start_cert_dmin", C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float)]),
    ("clwh_debug_hit_records", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32)]),
    ("clwh_debug_hull_table", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_int32)]),
    ("clwh_debug_hull_cert_bound", C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float)]),
    ("clwh_debug_hull_codes", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32)]),
    ("clwh_debug_hull_planes", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32)]),
    ("clwh_debug_hull_defer_bound", C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float)]),
    ("clwh_debug_hull_tilt_bound", C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float)]),
    ("clwh_debug_hull_h", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_int32)]),
    ("clwh_strerror", C.c_char_p, [C.c_int]),
    ("clwh_last_hip_error", C.c_int, []),
    ("clwh_version", C.c_char_p, []),
    ("clwh_ctx_acquire_from", C.c_int, [C.c_void_p, C.c_void_p]),
    ("clwh_ctx_release_to", C.c_int, [C.c_void_p, C.c_void_p]),
    ("clwh_ctx_set_timing", C.c_int, [C.c_void_p, C.c_int]),
    ("clwh_ctx_timing_read", C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32)]),
    ("clwh_ctx_timing_read_all", C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_int32]),
]
EXPORTED_SYMBOLS = [p[0] for p in _PROTOTYPES]

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libclwhip.so is missing (%s): build it with `python -m cl_volume_renderer_amd.build`; "
                "there is no CPU fallback for the product path" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, res, args in _PROTOTYPES:
            if not hasattr(L, name) and os.environ.get("CLWH_LIBRARY"):
                continue  # an older build named explicitly for an A/B timing run (tools/ab_bounce.sh)
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def _check(status, where):
    if status != OK:
        raise ClwhError(status, where)


def parse_tf(source: str) -> Tf:
    tf = Tf()
    _check(lib().clwh_tf_parse(source.encode(), C.byref(tf)), "clwh_tf_parse")
    return tf


def hull_cert_bound(X: int, Y: int, Z: int):
    """(delta0, slack): the smallest direction . n_k a hull certificate needs in an X x Y x Z volume (2.0: never granted), and the slack
    every entry of the hull table includes"""
    v = (C.c_float * 2)()
    _check(lib().clwh_debug_hull_cert_bound(X, Y, Z, v), "clwh_debug_hull_cert_bound")
    return float(v[0]), float(v[1])


def hull_defer_bound(X: int, Y: int, Z: int):
    """(delta0, J, D, scale): the smallest direction . n_k with which a march that got in front of its plane within J literal steps is
    granted in an X x Y x Z volume, the deficit limit D in voxels, and the grid of the stored margins (1 / scale voxels)"""
    v = (C.c_float * 4)()
    _check(lib().clwh_debug_hull_defer_bound(X, Y, Z, v), "clwh_debug_hull_defer_bound")
    return float(v[0]), int(v[1]), float(v[2]), int(v[3])


def hull_tilt_bound(X: int, Y: int, Z: int):
    """(delta, J, P, margin, target, gain) of the tilted planes: the bound over 70 - 5 - J steps, the J armed marches
    get with the rule on, the longest path a tilted plane may ask a march to count, and the tilt's target t = delta + margin with
    gain = t / sqrt(1 - t^2), as k_bounce gets them"""
    v = (C.c_float * 6)()
    _check(lib().clwh_debug_hull_tilt_bound(X, Y, Z, v), "clwh_debug_hull_tilt_bound")
    return float(v[0]), int(v[1]), int(v[2]), float(v[3]), float(v[4]), float(v[5])


def start_cert_dmin(X: int, Y: int, Z: int) -> float:
    """the smallest min |direction component| a start certificate needs in an X x Y x Z volume (2.0: never granted)"""
    v = C.c_float(0)
    _check(lib().clwh_debug_start_cert_dmin(X, Y, Z, C.byref(v)), "clwh_debug_start_cert_dmin")
    return float(v.value)


def cache_len(X, Y, Z) -> int:
    return int(lib().clwh_cache_len(X, Y, Z))


def accum_len(w, h, world=1) -> int:
    return int(lib().clwh_accum_len(w, h, world))


def _handle(mem):
    """the handle of an optional Mem"""
    return mem.h if mem is not None else None


def _fill_overlay(d, frame, source, kind, dims, palette, width, height, n_colours, flags, fill_alpha, outline_alpha, id_range, ids, t_first):
    """what the two overlay descriptors share"""
    d.frame = _handle(frame)
    d.region.buffer, d.region.kind = _handle(source), int(kind)
    for k in range(3):
        d.region.dims[k] = int(dims[k])
    d.region.id_lo, d.region.id_hi = int(id_range[0]), int(id_range[1])
    d.paint.palette = _handle(palette)
    d.paint.n_colours = int(n_colours if n_colours is not None else (palette.nbytes // 4 if palette is not None else 0))
    d.paint.flags, d.paint.fill_alpha, d.paint.outline_alpha = int(flags), int(fill_alpha), int(outline_alpha)
    d.paint.ids, d.paint.t_first = _handle(ids), _handle(t_first)
    d.width, d.height = int(width), int(height)


def _fill_view(d, frame, volume, cam_pos, cam_dir, width, height):
    """what the camera views' descriptors share"""
    d.frame, d.volume = frame.h, volume.h
    for k in range(3):
        d.cam_pos[k] = float(cam_pos[k])
        d.cam_dir[k] = float(cam_dir[k])
    d.width, d.height = int(width), int(height)


class Mem:
    def __init__(self, ctx, handle, nbytes, dtype=None, shape=None):
        self.ctx, self.h, self.nbytes, self.dtype, self.shape = ctx, C.c_void_p(handle), nbytes, dtype, shape

    def push(self, arr: np.ndarray):
        a = np.ascontiguousarray(arr)
        _check(lib().clwh_mem_push(self.ctx.h, self.h, a.ctypes.data, a.nbytes), "clwh_mem_push")

    def pull(self, dtype=None, shape=None) -> np.ndarray:
        dtype = np.dtype(dtype or self.dtype or np.uint8)
        out = np.empty(self.nbytes // dtype.itemsize, dtype=dtype)
        _check(lib().clwh_mem_pull(self.ctx.h, self.h, out.ctypes.data, out.nbytes), "clwh_mem_pull")
        shape = shape or self.shape
        return out.reshape(shape) if shape else out

    @property
    def device_ptr(self) -> int:
        return int(lib().clwh_mem_device_ptr(self.h) or 0)

    def release(self):
        if self.h:
            _check(lib().clwh_mem_release(self.h), "clwh_mem_release")
            self.h = None


class Kernel:
    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, C.c_void_p(handle)

    def launch(self, global_size, local_size, *args):
        g = (C.c_size_t * 3)(*(list(global_size) + [0, 0, 0])[:3])
        l = (C.c_size_t * 3)(*(list(local_size) + [0, 0, 0])[:3])
        arr = (Arg * max(len(args), 1))()
        for i, a in enumerate(args):
            if isinstance(a, Mem):
                arr[i].kind, arr[i].v.mem = ARG_MEM, a.h.value
            elif isinstance(a, (float, np.floating)):
                arr[i].kind, arr[i].v.f32 = ARG_F32, float(a)
            elif isinstance(a, np.unsignedinteger):
                arr[i].kind, arr[i].v.u32 = ARG_U32, int(a)
            elif isinstance(a, (int, np.integer)):
                arr[i].kind, arr[i].v.i32 = ARG_I32, int(a)
            else:
                raise TypeError("unsupported kernel argument %r" % (a,))
        _check(lib().clwh_launch(self.h, g, l, arr, len(args)), "clwh_launch")

    def render(self, *, frame, volume, sdf, env, cam_pos, cam_dir, seed, width, height, buffer_volume=None,
               accum=None, mode=ACCUM_VOXEL_CACHE, tile_rank=0, tile_world=1, write_frame=True,
               hit_index=None, contrib=None, seeds=None, shading=SHADE_LIGHT, resolve_only=False):
        d = RenderDesc()
        d.frame = frame.h if frame is not None else None
        d.volume, d.sdf, d.env = volume.h, sdf.h, env.h
        d.buffer_volume = buffer_volume.h if buffer_volume is not None else None
        for k in range(3):
            d.cam_pos[k] = float(cam_pos[k])
            d.cam_dir[k] = float(cam_dir[k])
        d.seed, d.width, d.height = int(seed), int(width), int(height)
        d.accum_mode = mode
        d.accum = accum.h if accum is not None else None
        d.tile_rank, d.tile_world = tile_rank, tile_world
        d.write_frame = 1 if write_frame else 0
        d.hit_index = hit_index.h if hit_index is not None else None
        d.contrib = contrib.h if contrib is not None else None
        d.shading = shading
        d.resolve_only = 1 if resolve_only else 0
        if seeds is not None:
            d.n_seeds = len(seeds)
            for i, sd in enumerate(seeds):
                d.seeds[i] = int(sd)
        _check(lib().clwh_render(self.h, C.byref(d)), "clwh_render")

    def release(self):
        if self.h:
            _check(lib().clwh_kernel_release(self.h), "clwh_kernel_release")
            self.h = None


class ExchangePlan:
    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, C.c_void_p(handle)

    def apply(self, buffer_volume: Mem, rgb: Mem, rgb_stride=3):
        """one pass's contributions (int32[n][rgb_stride], the plan's order) into the cache under the 256-token rule"""
        _check(lib().clwh_cache_apply_contributions(self.ctx.h, self.h, buffer_volume.h, rgb.h, rgb_stride),
               "clwh_cache_apply_contributions")

    def release(self):
        if self.h:
            _check(lib().clwh_cache_exchange_plan_release(self.h), "clwh_cache_exchange_plan_release")
            self.h = None


class Context:
    def __init__(self, device=0, stream=None):
        h = C.c_void_p()
        if stream is None:
            _check(lib().clwh_ctx_create(device, C.byref(h)), "clwh_ctx_create")
        else:
            _check(lib().clwh_ctx_create_on_stream(device, C.c_void_p(stream), C.byref(h)),
                   "clwh_ctx_create_on_stream")
        self.h = h

    def buffer(self, nbytes, dtype=None, shape=None) -> Mem:
        h = C.c_void_p()
        _check(lib().clwh_mem_create(self.h, nbytes, 0, C.byref(h)), "clwh_mem_create")
        return Mem(self, h.value, nbytes, dtype, shape)

    def buffer_from(self, arr: np.ndarray) -> Mem:
        a = np.ascontiguousarray(arr)
        m = self.buffer(a.nbytes, a.dtype, a.shape)
        m.push(a)
        return m

    def wrap(self, device_ptr: int, nbytes: int, dtype=None, shape=None) -> Mem:
        h = C.c_void_p()
        _check(lib().clwh_mem_wrap(self.h, C.c_void_p(device_ptr), nbytes, C.byref(h)), "clwh_mem_wrap")
        return Mem(self, h.value, nbytes, dtype, shape)

    def image(self, dims, channels, dtype, shape=None) -> Mem:
        dtype = np.dtype(dtype)
        d = (C.c_size_t * 3)(*(list(dims) + [1, 1, 1])[:3])
        h = C.c_void_p()
        _check(lib().clwh_image_create(self.h, d, channels, _ELEM_OF_DTYPE[dtype], 0, C.byref(h)),
               "clwh_image_create")
        n = int(np.prod([max(int(x), 1) for x in list(dims)[:3]])) * channels * dtype.itemsize
        return Mem(self, h.value, n, dtype, shape)

    def image_from(self, arr: np.ndarray, channels=1) -> Mem:
        """arr: [z][y][x] (3-D, 1 channel) or [h][w][c] (2-D, c channels)."""
        a = np.ascontiguousarray(arr)
        if channels == 1:
            dims = list(a.shape[::-1])
        else:
            assert a.shape[-1] == channels
            dims = list(a.shape[:-1][::-1])
        m = self.image(dims, channels, a.dtype, a.shape)
        m.push(a)
        return m

    def kernel(self, file: str, entry: str, prepend: str = "") -> Kernel:
        h = C.c_void_p()
        _check(lib().clwh_kernel_get(self.h, file.encode(), entry.encode(), prepend.encode(), C.byref(h)),
               "clwh_kernel_get")
        return Kernel(self, h.value)

    def sdf_build(self, volume: Mem, tf_source: str, sdf: Mem) -> int:
        n = C.c_int32(0)
        _check(lib().clwh_sdf_build(self.h, volume.h, tf_source.encode(), sdf.h, C.byref(n)), "clwh_sdf_build")
        return n.value

    def buffer_reset(self, buffer_volume: Mem):
        _check(lib().clwh_buffer_reset(self.h, buffer_volume.h), "clwh_buffer_reset")

    def exchange_plan(self, entries: Mem, n: int) -> "ExchangePlan":
        """group the listed cache entries (int64[n], (rank, pixel) order) by voxel: once per camera"""
        h = C.c_void_p()
        _check(lib().clwh_cache_exchange_plan(self.h, entries.h, int(n), C.byref(h)), "clwh_cache_exchange_plan")
        return ExchangePlan(self, h.value)

    def accum_resolve(self, accum_all: Mem, tile_world, width, height, frame: Mem, env: Mem, cam_pos, cam_dir):
        p = (C.c_float * 3)(*[float(x) for x in cam_pos])
        d = (C.c_float * 3)(*[float(x) for x in cam_dir])
        _check(lib().clwh_accum_resolve(self.h, accum_all.h, tile_world, width, height, frame.h, env.h, p, d),
               "clwh_accum_resolve")

    def accum_resolve_tiles(self, accum: Mem, tile_rank, tile_world, width, height, tiles_rgba8: Mem, env: Mem, cam_pos, cam_dir):
        """this rank's tiles -> RGBA8, tile-major (4 bytes per pixel to exchange instead of 16)"""
        p = (C.c_float * 3)(*[float(x) for x in cam_pos])
        d = (C.c_float * 3)(*[float(x) for x in cam_dir])
        _check(lib().clwh_accum_resolve_tiles(self.h, accum.h, tile_rank, tile_world, width, height, tiles_rgba8.h, env.h, p, d),
               "clwh_accum_resolve_tiles")

    def frame_from_tiles(self, tiles_all: Mem, tile_world, width, height, frame: Mem):
        _check(lib().clwh_frame_from_tiles(self.h, tiles_all.h, tile_world, width, height, frame.h), "clwh_frame_from_tiles")

    def invalidate_derived(self, scene=True, camera=True, projection=False):
        what = (DERIVED_SCENE if scene else 0) | (DERIVED_CAMERA if camera else 0) | (DERIVED_PROJECTION if projection else 0)
        _check(lib().clwh_ctx_invalidate_derived(self.h, what), "clwh_ctx_invalidate_derived")

    def render_projection(self, frame: Mem, volume: Mem, cam_pos, cam_dir, width, height, mode=PROJ_MAX, step=0.5,
                          window=(0.0, 1.0), t_near=0.0, t_far=float("inf"), values: Mem = None, t_extreme: Mem = None,
                          dense=False):
        """maximum / minimum / mean intensity projection of `volume` (S16) into `frame` (RGBA8) with clwh_render's camera rays;
        window = (center, width) maps the projected value to grey.  values / t_extreme: optional float32[height][width] buffers."""
        d = ProjectionDesc()
        _fill_view(d, frame, volume, cam_pos, cam_dir, width, height)
        d.mode, d.flags = int(mode), PROJ_DENSE if dense else 0
        d.step, d.t_near, d.t_far = float(step), float(t_near), float(t_far)
        d.window_center, d.window_width = float(window[0]), float(window[1])
        d.values = _handle(values)
        d.t_extreme = _handle(t_extreme)
        _check(lib().clwh_render_projection(self.h, C.byref(d)), "clwh_render_projection")

    def render_composite(self, frame: Mem, volume: Mem, cam_pos, cam_dir, width, height, lut: Mem, lut_first, lut_len=None, step=0.5,
                         alpha_stop=0.95, flags=0, ambient=0.3, t_near=0.0, t_far=float("inf"), rgba: Mem = None,
                         t_first: Mem = None, t_stop: Mem = None):
        """front-to-back compositing of `volume` (S16) through the colour/opacity table `lut` (float32[lut_len][4], entry 0 = voxel
        value lut_first) into `frame` (RGBA8, premultiplied) with clwh_render's camera rays.  flags: COMP_DENSE | COMP_SHADE.
        rgba / t_first / t_stop: optional float32 buffers over the launched region.  lut_len defaults to the whole buffer."""
        d = CompositeDesc()
        _fill_view(d, frame, volume, cam_pos, cam_dir, width, height)
        d.flags = int(flags)
        d.step, d.t_near, d.t_far = float(step), float(t_near), float(t_far)
        d.lut = _handle(lut)
        d.lut_first = int(lut_first)
        d.lut_len = int(lut_len if lut_len is not None else (lut.nbytes // 16 if lut is not None else 0))
        d.alpha_stop, d.ambient = float(alpha_stop), float(ambient)
        d.rgba = _handle(rgba)
        d.t_first = _handle(t_first)
        d.t_stop = _handle(t_stop)
        _check(lib().clwh_render_composite(self.h, C.byref(d)), "clwh_render_composite")

    def render_isosurface(self, frame: Mem, volume: Mem, cam_pos, cam_dir, width, height, iso, step=0.5, refine=8, flags=0,
                          color=(1.0, 1.0, 1.0), ambient=0.3, t_near=0.0, t_far=float("inf"), t_hit: Mem = None, normal: Mem = None):
        """the isosurface of the trilinear field of `volume` (S16) at value `iso` into `frame` (RGBA8), shaded by a two-sided
        headlight, with clwh_render's camera rays.  flags: ISO_DENSE | ISO_BELOW.  t_hit (float32[height][width]) / normal
        (float32[height][width][4] = n, value at the hit): optional buffers over the launched region."""
        d = IsosurfaceDesc()
        _fill_view(d, frame, volume, cam_pos, cam_dir, width, height)
        for k in range(3):
            d.color[k] = float(color[k])
        d.flags = int(flags)
        d.step, d.t_near, d.t_far = float(step), float(t_near), float(t_far)
        d.iso, d.refine, d.ambient = float(iso), int(refine), float(ambient)
        d.t_hit = _handle(t_hit)
        d.normal = _handle(normal)
        _check(lib().clwh_render_isosurface(self.h, C.byref(d)), "clwh_render_isosurface")

    def render_slice(self, frame: Mem, volume: Mem, origin, du, dv, normal, width, height, mode=SLICE_MAX, slab_samples=1, step=0.5,
                     window=(0.0, 1.0), flags=0, values: Mem = None, t_extreme: Mem = None):
        """a slice of the trilinear field of `volume` (S16) on the plane origin + x * du + y * dv (voxel space) into `frame` (RGBA8),
        or the maximum / minimum / mean over `slab_samples` planes `step` apart along `normal` (mode: SLICE_MAX / MIN / MEAN;
        scene.slice_plane makes axial, coronal and sagittal planes).  window = (center, width) maps the value to grey.  flags:
        SLICE_DENSE.  values / t_extreme: optional float32[height][width] buffers."""
        d = SliceDesc()
        d.frame, d.volume = frame.h, volume.h
        for k in range(3):
            d.origin[k], d.du[k], d.dv[k], d.normal[k] = float(origin[k]), float(du[k]), float(dv[k]), float(normal[k])
        d.width, d.height = int(width), int(height)
        d.mode, d.flags = int(mode), int(flags)
        d.slab_samples, d.step = int(slab_samples), float(step)
        d.window_center, d.window_width = float(window[0]), float(window[1])
        d.values = _handle(values)
        d.t_extreme = _handle(t_extreme)
        _check(lib().clwh_render_slice(self.h, C.byref(d)), "clwh_render_slice")

    def render_curved_raw(self, frame: Mem, volume: Mem, rows, width, height, mode=SLICE_MAX, slab_samples=1, step=0.5,
                          window=(0.0, 1.0), flags=0, values: Mem = None, t_extreme: Mem = None):
        """one clwh_render_curved call: its status; nothing is raised.  rows: float32 [height][9] on the host (origin, du, normal per
        image row), or None for a NULL pointer.  The library copies the rows before it returns."""
        d = CurvedDesc()
        d.frame, d.volume = _handle(frame), _handle(volume)
        r = None if rows is None else np.ascontiguousarray(rows, np.float32)
        d.rows = None if r is None else r.ctypes.data
        d.width, d.height = int(width), int(height)
        d.mode, d.flags = int(mode), int(flags)
        d.slab_samples, d.step = int(slab_samples), float(step)
        d.window_center, d.window_width = float(window[0]), float(window[1])
        d.values = _handle(values)
        d.t_extreme = _handle(t_extreme)
        return lib().clwh_render_curved(self.h, C.byref(d))

    def render_curved(self, frame: Mem, volume: Mem, rows, width, height, mode=SLICE_MAX, slab_samples=1, step=0.5,
                      window=(0.0, 1.0), flags=0, values: Mem = None, t_extreme: Mem = None):
        """the straightened curved reformat of `volume` (S16) into `frame` (RGBA8): image row y is the line origin_y + x * du_y of
        rows[y] (scene.curve_frames makes the rows of a centreline), thin or the maximum / minimum / mean over `slab_samples` samples
        `step` apart along normal_y.  Everything else as render_slice.  flags: CURVED_DENSE."""
        if rows is None or np.shape(rows) != (int(height), 9):
            raise ValueError("render_curved: rows must be float32 [height][9]")
        _check(self.render_curved_raw(frame, volume, rows, width, height, mode, slab_samples, step, window, flags, values, t_extreme),
               "clwh_render_curved")

    def curve_profile_raw(self, mask: Mem, dims, rows, n_rows, width, slab_samples, step, flags=0, records: Mem = None):
        """one clwh_curve_profile call: its status; nothing is raised.  rows: float32 [n_rows][9] on the host, or None for NULL."""
        d = CurveProfileDesc()
        d.mask, d.records = _handle(mask), _handle(records)
        for k in range(3):
            d.dims[k] = int(dims[k])
        r = None if rows is None else np.ascontiguousarray(rows, np.float32)
        d.rows = None if r is None else r.ctypes.data
        d.n_rows, d.width = int(n_rows), int(width)
        d.slab_samples, d.step, d.flags = int(slab_samples), float(step), int(flags)
        return lib().clwh_curve_profile(self.h, C.byref(d))

    def curve_profile(self, mask: Mem, dims, rows, width, slab_samples, step, connected=True) -> np.ndarray:
        """the section records of `mask` (grow's layout, dims = (X, Y, Z)) at the stations `rows` (float32 [n][9]): a structured array
        (SECTION_RECORD_DTYPE: count, sum_x, sum_k, border) of n records over a grid of width x slab_samples samples per station;
        connected: only the part of a section that is 4-connected to the grid's centre.  scene.profile_measures turns the records
        into areas and diameters.  The call waits for the device."""
        rows = np.ascontiguousarray(rows, np.float32)
        if rows.ndim != 2 or rows.shape[1] != 9 or rows.shape[0] < 1:
            raise ValueError("curve_profile: rows must be float32 [n][9], n >= 1")
        n = rows.shape[0]
        records = self.buffer(16 * n, SECTION_RECORD_DTYPE, (n,))
        try:
            _check(self.curve_profile_raw(mask, dims, rows, n, width, slab_samples, step, PROFILE_CONNECTED if connected else 0, records),
                   "clwh_curve_profile")
            return records.pull()
        finally:
            records.release()

    def vessel_profile(self, mask: Mem, dims, points, spacing, pixel_mm, window=64, connected=True, station_mm=None, smooth_passes=8,
                       angle=0.0):
        """the stenosis curve of the vessel `mask` along the path `points` (voxels, as Context.centerline returns them): a dictionary
        with s_mm (the stations' arc length) and, per station, area_mm2, diameter_mm, offset_mm (the section's centroid from the
        curve, across and along the section window) and cut (the window cut the section), beside the raw records.  The sections lie
        in the planes perpendicular to the curve: scene.curve_frames with slab_samples = width = window and step_mm = pixel_mm, one
        clwh_curve_profile call, scene.profile_measures.  station_mm defaults to pixel_mm.  The call waits for the device."""
        from . import scene

        station_mm = pixel_mm if station_mm is None else station_mm
        rows, s_mm, n = scene.curve_frames(points, spacing, window, pixel_mm=pixel_mm, station_mm=station_mm, smooth_passes=smooth_passes,
                                           angle=angle, slab_samples=window, step_mm=pixel_mm)
        records = self.curve_profile(mask, dims, rows[:n], window, window, pixel_mm, connected)
        out = scene.profile_measures(records, pixel_mm, pixel_mm, window, window)
        out["s_mm"], out["records"] = s_mm, records
        return out

    def overlay_slice_raw(self, frame: Mem, source: Mem, kind, dims, palette: Mem, origin, du, dv, normal, width, height, slab_samples=1,
                          step=0.5, flags=OVERLAY_FILL | OVERLAY_OUTLINE, fill_alpha=96, outline_alpha=255, id_range=(1, 0xFFFFFFFF),
                          n_colours=None, ids: Mem = None, t_first: Mem = None):
        """one clwh_overlay_slice call: its status; nothing is raised.  The region `source` (kind REGION_MASK: grow's mask layout,
        REGION_LABELS: uint32[Z][Y][X]; dims = (X, Y, Z)) drawn over `frame` with the rays of render_slice's plane; palette: packed
        RGBA8 words (n_colours defaults to the whole buffer).  ids (uint32) / t_first (float32): optional [height][width] buffers."""
        d = OverlaySliceDesc()
        _fill_overlay(d, frame, source, kind, dims, palette, width, height, n_colours, flags, fill_alpha, outline_alpha, id_range, ids, t_first)
        for k in range(3):
            d.origin[k], d.du[k], d.dv[k], d.normal[k] = float(origin[k]), float(du[k]), float(dv[k]), float(normal[k])
        d.slab_samples, d.step = int(slab_samples), float(step)
        return lib().clwh_overlay_slice(self.h, C.byref(d))

    def overlay_slice(self, *args, **kw):
        """overlay_slice_raw, raising on a status other than OK"""
        _check(self.overlay_slice_raw(*args, **kw), "clwh_overlay_slice")

    def overlay_camera_raw(self, frame: Mem, source: Mem, kind, dims, palette: Mem, cam_pos, cam_dir, width, height, step=0.5,
                           t_near=0.0, t_far=float("inf"), flags=OVERLAY_FILL | OVERLAY_OUTLINE, fill_alpha=96, outline_alpha=255,
                           id_range=(1, 0xFFFFFFFF), n_colours=None, ids: Mem = None, t_first: Mem = None):
        """one clwh_overlay_camera call: its status; nothing is raised.  As overlay_slice_raw with render_projection's camera rays:
        the first voxel of the region along each ray, whatever the volume shows in front of it."""
        d = OverlayCameraDesc()
        _fill_overlay(d, frame, source, kind, dims, palette, width, height, n_colours, flags, fill_alpha, outline_alpha, id_range, ids, t_first)
        for k in range(3):
            d.cam_pos[k], d.cam_dir[k] = float(cam_pos[k]), float(cam_dir[k])
        d.step, d.t_near, d.t_far = float(step), float(t_near), float(t_far)
        return lib().clwh_overlay_camera(self.h, C.byref(d))

    def overlay_camera(self, *args, **kw):
        """overlay_camera_raw, raising on a status other than OK"""
        _check(self.overlay_camera_raw(*args, **kw), "clwh_overlay_camera")

    def mesh_isosurface_raw(self, volume: Mem, iso, flags=0, box=None, positions: Mem = None, normals: Mem = None, keys: Mem = None,
                            triangles: Mem = None, vertex_capacity=0, triangle_capacity=0):
        """one clwh_mesh_isosurface call: (status, n_vertices, n_triangles); nothing is raised.  box = ((lo), (hi)) in grid points."""
        d = MeshDesc()
        nv, nt = C.c_uint64(0), C.c_uint64(0)
        d.volume = _handle(volume)
        d.iso, d.flags = float(iso), int(flags)
        if box is not None:
            for k in range(3):
                d.box_lo[k], d.box_hi[k] = int(box[0][k]), int(box[1][k])
        d.positions = _handle(positions)
        d.normals = _handle(normals)
        d.keys = _handle(keys)
        d.triangles = _handle(triangles)
        d.vertex_capacity, d.triangle_capacity = int(vertex_capacity), int(triangle_capacity)
        d.n_vertices, d.n_triangles = C.pointer(nv), C.pointer(nt)
        status = lib().clwh_mesh_isosurface(self.h, C.byref(d))
        return status, int(nv.value), int(nt.value)

    def mesh_isosurface(self, volume: Mem, iso, flags=0, box=None, normals=True, keys=False):
        """the isosurface of `volume` (S16) at `iso` as an indexed triangle mesh (marching tetrahedra on the voxel centres; positions
        in voxel space): (positions float32[n][3], normals float32[n][3] | None, triangles uint32[m][3], keys uint64[n] | None) as
        numpy arrays.  flags: MESH_DENSE | MESH_BELOW; box = ((lo), (hi)) in grid points, None = the whole volume.  One counting
        call, then the filling call; both wait for the device."""
        status, nv, nt = self.mesh_isosurface_raw(volume, iso, flags, box)
        _check(status, "clwh_mesh_isosurface")
        out_n = np.zeros((nv, 3), np.float32) if normals else None
        out_k = np.zeros((nv,), np.uint64) if keys else None
        if nv == 0:
            return np.zeros((0, 3), np.float32), out_n, np.zeros((0, 3), np.uint32), out_k
        bufs = [self.buffer(nv * 12, np.float32, (nv, 3)), self.buffer(nv * 12, np.float32, (nv, 3)) if normals else None,
                self.buffer(nv * 8, np.uint64, (nv,)) if keys else None, self.buffer(max(nt, 1) * 12, np.uint32, (max(nt, 1), 3))]
        try:
            status, _, _ = self.mesh_isosurface_raw(volume, iso, flags, box, bufs[0], bufs[1], bufs[2], bufs[3], nv, nt)
            _check(status, "clwh_mesh_isosurface")
            return (bufs[0].pull(), bufs[1].pull() if normals else None, bufs[3].pull()[:nt], bufs[2].pull() if keys else None)
        finally:
            for b in bufs:
                if b is not None:
                    b.release()

    def grow_region_raw(self, volume: Mem, seeds, lo, hi, flags=0, box=None, mask: Mem = None):
        """one clwh_segment_grow call: (status, GrowResult); nothing is raised.  seeds: rows of (x, y, z), or None."""
        d, res = GrowDesc(), GrowResult()
        d.volume, d.mask = _handle(volume), _handle(mask)
        d.lo, d.hi, d.flags = int(lo), int(hi), int(flags)
        if seeds is not None:
            s = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint32).reshape(-1, 3))
            d.n_seeds = len(s)
            d.seeds = s.ctypes.data_as(C.POINTER(C.c_uint32))
        if box is not None:
            for k in range(3):
                d.box_lo[k], d.box_hi[k] = int(box[0][k]), int(box[1][k])
        d.result = C.pointer(res)
        return lib().clwh_segment_grow(self.h, C.byref(d)), res

    def grow_region(self, volume: Mem, seeds, lo, hi, connectivity=6, box=None, mask: Mem = None, from_mask=False, dense=False):
        """the connected set of voxels of `volume` (S16) with lo <= value <= hi (inside box = ((lo), (hi)) in voxels, hi exclusive)
        that hangs together with `seeds` (rows of (x, y, z)) under 6- or 26-connectivity: (mask, GrowResult).  The mask is one bit per
        voxel in the layout scene.mask_pack / mask_unpack describe; it is allocated when none is given.  from_mask: the admissible
        bits of `mask` on entry are seeds too (seeds may then be empty or None).  dense: every tile in every round (tests, timing).
        The call waits for the device."""
        if connectivity not in (6, 26):
            raise ValueError("connectivity is 6 or 26")
        own = mask is None
        if own:
            from . import scene

            if volume.shape is None or len(volume.shape) != 3:
                raise ValueError("a volume without a [z][y][x] shape (a wrap): pass the mask buffer")
            X, Y, Z = volume.shape[::-1]
            n = scene.mask_words_per_row(X) * Y * Z
            mask = self.buffer(4 * n, np.uint32, (n,))
        flags = (GROW_26 if connectivity == 26 else 0) | (GROW_FROM_MASK if from_mask else 0) | (GROW_DENSE if dense else 0)
        status, res = self.grow_region_raw(volume, seeds, lo, hi, flags, box, mask)
        if status != OK and own:
            mask.release()
        _check(status, "clwh_segment_grow")
        return mask, res

    def apply_mask_raw(self, volume_in: Mem, mask: Mem, volume_out: Mem, fill=-32768, flags=0):
        """one clwh_volume_apply_mask call: its status; nothing is raised"""
        d = ApplyMaskDesc()
        d.volume_in, d.volume_out, d.mask = _handle(volume_in), _handle(volume_out), _handle(mask)
        d.fill, d.flags = int(fill), int(flags)
        return lib().clwh_volume_apply_mask(self.h, C.byref(d))

    def apply_mask(self, volume: Mem, mask: Mem, out: Mem = None, fill=-32768, invert=False):
        """out = volume where the mask's bit is set (invert: where it is clear), `fill` elsewhere; out=None: in place.  Counts as a
        rewrite of `out`: every view of it rebuilds its derived data at its next use."""
        _check(self.apply_mask_raw(volume, mask, out if out is not None else volume, fill, MASK_INVERT if invert else 0),
               "clwh_volume_apply_mask")

    def filter_volume_raw(self, volume_in: Mem, volume_out: Mem, kind, radius, weights=None, mask: Mem = None, flags=0):
        """one clwh_volume_filter call: its status; nothing is raised.  weights: None, or three sequences (an entry may be None: a NULL
        pointer) of uint16, tap 0 first"""
        d = FilterDesc()
        d.volume_in, d.volume_out, d.mask = _handle(volume_in), _handle(volume_out), _handle(mask)
        d.kind, d.flags = int(kind), int(flags)
        keep = []  # the arrays live until the call returns: it copies them
        for k in range(3):
            d.radius[k] = int(radius[k])
            if weights is not None and weights[k] is not None:
                w = np.ascontiguousarray(weights[k], np.uint16)
                keep.append(w)
                d.weights[k] = w.ctypes.data_as(C.POINTER(C.c_uint16))
        return lib().clwh_volume_filter(self.h, C.byref(d))

    def filter_volume(self, volume: Mem, kind, radius=(1, 1, 1), weights=None, mask: Mem = None, out: Mem = None):
        """`volume` filtered over the box |dx| <= rx, |dy| <= ry, |dz| <= rz with the edge replicated: FILTER_MEDIAN (radii 0 or 1),
        FILTER_MIN / FILTER_MAX (grey erosion / dilation, radii up to 16) or FILTER_SMOOTH (three exact integer passes x, y, z with
        `weights`, three uint16 arrays as scene.gaussian_weights / scene.binomial_weights return them; the radii are taken from their
        lengths).  With `mask` (grow's layout) only the voxels whose bit is set change.  out=None: in place.  Counts as a rewrite of
        `out`: every view of it rebuilds its derived data at its next use."""
        if kind == FILTER_SMOOTH and weights is not None:
            radius = tuple(len(w) - 1 for w in weights)
        _check(self.filter_volume_raw(volume, out if out is not None else volume, kind, radius, weights, mask), "clwh_volume_filter")

    def label_components_raw(self, volume: Mem, lo, hi, flags=0, box=None, mask: Mem = None, labels: Mem = None, components: Mem = None,
                             capacity=0):
        """one clwh_segment_label call: (status, LabelResult); nothing is raised"""
        d, res = LabelDesc(), LabelResult()
        d.volume, d.labels, d.components, d.mask = _handle(volume), _handle(labels), _handle(components), _handle(mask)
        d.component_capacity = int(capacity)
        d.lo, d.hi, d.flags = int(lo), int(hi), int(flags)
        if box is not None:
            for k in range(3):
                d.box_lo[k], d.box_hi[k] = int(box[0][k]), int(box[1][k])
        d.result = C.pointer(res)
        return lib().clwh_segment_label(self.h, C.byref(d)), res

    def label_components(self, volume: Mem, lo, hi, connectivity=6, box=None, mask: Mem = None, labels: Mem = None, capacity=256):
        """all connected components of the voxels of `volume` (S16) with lo <= value <= hi (inside box = ((lo), (hi)) in voxels, hi
        exclusive; with `mask`: only where its bit is set as well) under 6- or 26-connectivity, ranked by descending voxel count, ties
        by the earlier first voxel: (labels, LabelResult, table).  labels: uint32 [z][y][x] on the device, 0 or the component's rank;
        allocated when none is given.  table: the records of the min(n_components, capacity) largest as a structured numpy array
        (LABEL_COMPONENT_DTYPE).  The call waits for the device."""
        if connectivity not in (6, 26):
            raise ValueError("connectivity is 6 or 26")
        if volume.shape is None or len(volume.shape) != 3:
            raise ValueError("a volume without a [z][y][x] shape (a wrap): use label_components_raw")
        own = labels is None
        if own:
            labels = self.buffer(4 * int(np.prod(volume.shape)), np.uint32, tuple(volume.shape))
        capacity = int(capacity)
        table = self.buffer(max(capacity, 1) * 48, np.uint8)
        try:
            flags = (LABEL_26 if connectivity == 26 else 0) | (LABEL_FROM_MASK if mask is not None else 0)
            status, res = self.label_components_raw(volume, lo, hi, flags, box, mask, labels, table if capacity else None, capacity)
            if status != OK and own:
                labels.release()
            _check(status, "clwh_segment_label")
            n = min(int(res.n_components), capacity)
            records = table.pull(np.uint8)[:48 * n].view(LABEL_COMPONENT_DTYPE).copy() if n else np.zeros(0, LABEL_COMPONENT_DTYPE)
            return labels, res, records
        finally:
            table.release()

    def labels_to_mask_raw(self, labels: Mem, mask: Mem, dims, rank_lo, rank_hi):
        """one clwh_labels_to_mask call: its status; nothing is raised.  dims = (X, Y, Z)"""
        d = LabelsToMaskDesc()
        d.labels, d.mask = _handle(labels), _handle(mask)
        for k in range(3):
            d.dims[k] = int(dims[k])
        d.rank_lo, d.rank_hi = int(rank_lo), int(rank_hi)
        return lib().clwh_labels_to_mask(self.h, C.byref(d))

    def labels_to_mask(self, labels: Mem, dims, rank_lo, rank_hi, mask: Mem = None) -> Mem:
        """the components of ranks rank_lo .. rank_hi (both included) of `labels` (uint32 [z][y][x] of dims = (X, Y, Z)) as a mask in
        clwh_segment_grow's layout, allocated when none is given.  Ordered on the context's stream; does not wait."""
        own = mask is None
        if own:
            from . import scene

            n = scene.mask_words_per_row(int(dims[0])) * int(dims[1]) * int(dims[2])
            mask = self.buffer(4 * n, np.uint32, (n,))
        status = self.labels_to_mask_raw(labels, mask, dims, rank_lo, rank_hi)
        if status != OK and own:
            mask.release()
        _check(status, "clwh_labels_to_mask")
        return mask

    def keep_components(self, volume: Mem, lo, hi, largest=None, min_count=None, connectivity=6, box=None, mask: Mem = None, capacity=256):
        """the mask of the `largest` biggest components of the window, or of those with at least `min_count` voxels (exactly one of
        the two): (mask, LabelResult, number of components kept).  None kept: an empty mask.  min_count is decided from the table of
        the `capacity` largest; if that table is truncated and its last record still has min_count voxels, ValueError asks for a
        larger capacity."""
        if (largest is None) == (min_count is None):
            raise ValueError("exactly one of largest and min_count")
        labels, res, table = self.label_components(volume, lo, hi, connectivity, box, mask, capacity=capacity)
        try:
            n = int(res.n_components)
            if largest is not None:
                if int(largest) < 1:
                    raise ValueError("largest is at least 1")
                keep = min(n, int(largest))
            else:
                keep = int(np.count_nonzero(table["count"] >= int(min_count)))
                if keep == len(table) and len(table) < n:
                    raise ValueError("min_count=%d is not decided by the %d largest of %d components: pass a larger capacity"
                                     % (int(min_count), len(table), n))
            dims = volume.shape[::-1]
            # (no component kept: a rank nobody has gives the empty mask)
            out = self.labels_to_mask(labels, dims, 1 if keep else n + 1, keep if keep else n + 1)
            return out, res, keep
        finally:
            labels.release()

    def mask_distance_raw(self, mask: Mem, dist: Mem, dims, weights=(1, 1, 1), cap=DIST_NONE, flags=0):
        """one clwh_mask_distance call: its status; nothing is raised.  dims = (X, Y, Z), weights = (wx, wy, wz)"""
        d = DistanceDesc()
        d.mask, d.dist = _handle(mask), _handle(dist)
        for k in range(3):
            d.dims[k], d.weight[k] = int(dims[k]), int(weights[k])
        d.cap, d.flags = int(cap), int(flags)
        return lib().clwh_mask_distance(self.h, C.byref(d))

    def mask_distance(self, mask: Mem, dims, weights=(1, 1, 1), to_clear=False, cap=None, dist: Mem = None) -> Mem:
        """the exact squared distance of every voxel of a volume of dims = (X, Y, Z) to the nearest set voxel of `mask` (to_clear: to
        the nearest clear one), wx dx^2 + wy dy^2 + wz dz^2 in integers: uint32 [z][y][x] on the device, DIST_NONE where there is no
        such voxel or the distance is above `cap`; allocated when none is given.  Ordered on the context's stream; does not wait."""
        own = dist is None
        if own:
            shape = (int(dims[2]), int(dims[1]), int(dims[0]))
            dist = self.buffer(4 * int(np.prod(shape)), np.uint32, shape)
        status = self.mask_distance_raw(mask, dist, dims, weights, DIST_NONE if cap is None else cap, DIST_TO_CLEAR if to_clear else 0)
        if status != OK and own:
            dist.release()
        _check(status, "clwh_mask_distance")
        return dist

    def _new_mask(self, dims) -> Mem:
        from . import scene

        n = scene.mask_words_per_row(int(dims[0])) * int(dims[1]) * int(dims[2])
        return self.buffer(4 * n, np.uint32, (n,))

    def mask_morph_raw(self, mask_in: Mem, mask_out: Mem, dims, op, radius_sq, weights=(1, 1, 1), flags=0):
        """one clwh_mask_morph call: its status; nothing is raised"""
        d = MorphDesc()
        d.mask_in, d.mask_out = _handle(mask_in), _handle(mask_out)
        for k in range(3):
            d.dims[k], d.weight[k] = int(dims[k]), int(weights[k])
        d.radius_sq, d.op, d.flags = int(radius_sq), int(op), int(flags)
        return lib().clwh_mask_morph(self.h, C.byref(d))

    def mask_morph(self, mask: Mem, dims, op, radius_sq, weights=(1, 1, 1), out: Mem = None) -> Mem:
        """`mask` dilated, eroded, opened or closed (MORPH_*) by the ball wx dx^2 + wy dy^2 + wz dz^2 <= radius_sq
        (scene.mask_weights / scene.radius_sq turn voxel sizes and a radius into these integers); the volume's border does not erode.
        `out` may be `mask`; allocated when none is given.  Ordered on the context's stream; does not wait."""
        own = out is None
        if own:
            out = self._new_mask(dims)
        status = self.mask_morph_raw(mask, out, dims, op, radius_sq, weights)
        if status != OK and own:
            out.release()
        _check(status, "clwh_mask_morph")
        return out

    def mask_combine_raw(self, a: Mem, b: Mem, out: Mem, dims, op):
        """one clwh_mask_combine call: its status; nothing is raised"""
        d = MaskCombineDesc()
        d.a, d.b, d.out = _handle(a), _handle(b), _handle(out)
        for k in range(3):
            d.dims[k] = int(dims[k])
        d.op = int(op)
        return lib().clwh_mask_combine(self.h, C.byref(d))

    def mask_combine(self, a: Mem, b: Mem, op, dims, out: Mem = None) -> Mem:
        """a AND b, a OR b, a XOR b, a AND NOT b or NOT a (MASK_*; b may be None for MASK_NOT) of two masks of a volume of dims =
        (X, Y, Z), with clean padding; `out` may be `a` or `b`; allocated when none is given.  Does not wait."""
        own = out is None
        if own:
            out = self._new_mask(dims)
        status = self.mask_combine_raw(a, b, out, dims, op)
        if status != OK and own:
            out.release()
        _check(status, "clwh_mask_combine")
        return out

    def thin_mask_raw(self, mask_in: Mem, mask_out: Mem, dims, flags=0, anchors: Mem = None, max_iterations=0):
        """one clwh_mask_thin call: (status, ThinResult); nothing is raised"""
        d, res = ThinDesc(), ThinResult()
        d.mask_in, d.mask_out, d.anchors = _handle(mask_in), _handle(mask_out), _handle(anchors)
        for k in range(3):
            d.dims[k] = int(dims[k])
        d.flags, d.max_iterations = int(flags), int(max_iterations)
        d.result = C.pointer(res)
        return lib().clwh_mask_thin(self.h, C.byref(d)), res

    def thin_mask(self, mask: Mem, dims, keep_ends=True, anchors: Mem = None, max_iterations=0, out: Mem = None, dense=False):
        """the skeleton of `mask` (grow's layout, dims = (X, Y, Z)) by topology-preserving thinning: (mask, ThinResult).  Parts,
        cavities and tunnels are kept; keep_ends keeps the tips of branches (a curve skeleton), without it only `anchors` (a mask
        of voxels that are never deleted) and closed loops hold a branch.  Outside the volume is background.  `out` may be `mask`;
        allocated when none is given.  The call waits for the device."""
        own = out is None
        if own:
            out = self._new_mask(dims)
        status, res = self.thin_mask_raw(mask, out, dims, (THIN_KEEP_ENDS if keep_ends else 0) | (THIN_DENSE if dense else 0), anchors,
                                         max_iterations)
        if status != OK and own:
            out.release()
        _check(status, "clwh_mask_thin")
        return out, res

    def mask_points_raw(self, mask: Mem, dims, points: Mem = None, capacity=0, map: Mem = None, values: Mem = None, flags=0):
        """one clwh_mask_points call: (status, n_points); nothing is raised"""
        d = MaskPointsDesc()
        n = C.c_uint64(0)
        d.mask, d.points, d.map, d.values = _handle(mask), _handle(points), _handle(map), _handle(values)
        for k in range(3):
            d.dims[k] = int(dims[k])
        d.flags, d.capacity = int(flags), int(capacity)
        d.n_points = C.pointer(n)
        return lib().clwh_mask_points(self.h, C.byref(d)), int(n.value)

    def mask_points(self, mask: Mem, dims, map: Mem = None):
        """the set voxels of `mask` in ascending flat index: (points uint32[n][4] = x, y, z, n26, values uint32[n] | None) as numpy
        arrays; n26 is the number of set 26-neighbours, values the words of `map` (uint32 [z][y][x] on the device) at the voxels.
        One counting call, then the filling call; both wait for the device."""
        status, n = self.mask_points_raw(mask, dims)
        _check(status, "clwh_mask_points")
        if n == 0:
            return np.zeros((0, 4), np.uint32), (np.zeros((0,), np.uint32) if map is not None else None)
        points = self.buffer(16 * n, np.uint32, (n, 4))
        values = self.buffer(4 * n, np.uint32, (n,)) if map is not None else None
        try:
            status, _ = self.mask_points_raw(mask, dims, points, n, map, values)
            _check(status, "clwh_mask_points")
            return points.pull(), (values.pull() if values is not None else None)
        finally:
            points.release()
            if values is not None:
                values.release()

    def skeleton(self, mask: Mem, dims, spacing=(1, 1, 1), keep_ends=True, anchors: Mem = None):
        """the skeleton of `mask` as a graph: scene.skeleton_graph's dict (nodes, branches with their lengths in the unit of
        `spacing` and their mean and minimum radius), with "points" (uint32[n][4]) and "result" (ThinResult) beside.  Four steps: the
        depth map of the mask (mask_distance to the nearest clear voxel, weights scene.mask_weights(spacing)), thin_mask,
        mask_points sampling the depth, and the graph on the host.  The call waits for the device."""
        from . import scene

        depth = self.mask_distance(mask, dims, scene.mask_weights(spacing), to_clear=True)
        thin = None
        try:
            thin, res = self.thin_mask(mask, dims, keep_ends, anchors)
            points, depths = self.mask_points(thin, dims, depth)
        finally:
            depth.release()
            if thin is not None:
                thin.release()
        graph = scene.skeleton_graph(points[:, :3], points[:, 3], spacing, depths)
        graph["points"], graph["result"] = points, res
        return graph

    @staticmethod
    def _geodesic_weights(d, weights):
        """weights: None (all 1), (fx, fy, fz), or (face, edge, corner) as scene.geodesic_weights returns them"""
        face, edge, corner = (1, 1, 1), (1, 1, 1), 1
        if weights is not None:
            if len(weights) == 3 and np.ndim(weights[0]) == 1:
                face, edge, corner = weights
            else:
                face = weights
        for k in range(3):
            d.weight_face[k], d.weight_edge[k] = int(face[k]), int(edge[k])
        d.weight_corner = int(corner)

    def mask_geodesic_raw(self, domain: Mem, dims, seeds=None, seed_labels: Mem = None, flags=0, weights=None, cap=DIST_NONE,
                          dist: Mem = None, labels: Mem = None, result=True):
        """one clwh_mask_geodesic call: (status, GeodesicResult); nothing is raised.  seeds: rows of (x, y, z, id), or None.
        result=False passes a NULL result."""
        d, res = GeodesicDesc(), GeodesicResult()
        d.domain, d.seed_labels, d.dist, d.labels = _handle(domain), _handle(seed_labels), _handle(dist), _handle(labels)
        for k in range(3):
            d.dims[k] = int(dims[k])
        self._geodesic_weights(d, weights)
        d.cap, d.flags = int(cap), int(flags)
        if seeds is not None:
            s = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint32).reshape(-1, 4))
            d.n_seeds = len(s)
            d.seeds = s.ctypes.data_as(C.POINTER(C.c_uint32))
        if result:
            d.result = C.pointer(res)
        return lib().clwh_mask_geodesic(self.h, C.byref(d)), res

    def mask_geodesic(self, domain: Mem, dims, seeds=None, seed_labels: Mem = None, connectivity=6, weights=None, cap=None,
                      dist: Mem = None, labels: Mem = None, dense=False):
        """shortest paths inside the mask `domain` (grow's layout, dims = (X, Y, Z)) from labelled seeds: (dist, labels,
        GeodesicResult).  seeds: rows of (x, y, z, id), id >= 1; seed_labels: a uint32 [z][y][x] device buffer whose nonzero words
        inside the domain are seeds with that id as well.  dist: the length of the shortest path to the nearest seed, DIST_NONE
        outside the domain and where no seed reaches within `cap`; labels: the smallest id among the nearest seeds, 0 there.  Both
        are uint32 [z][y][x] on the device, allocated when none is given; `labels` may be `seed_labels`.  weights: None (every step
        costs 1), (fx, fy, fz), or (face, edge, corner) from scene.geodesic_weights.  dense: every tile in every round (tests,
        timing).  The call waits for the device."""
        if connectivity not in (6, 26):
            raise ValueError("connectivity is 6 or 26")
        shape = (int(dims[2]), int(dims[1]), int(dims[0]))
        own = [dist is None, labels is None]
        if own[0]:
            dist = self.buffer(4 * int(np.prod(shape)), np.uint32, shape)
        if own[1]:
            labels = self.buffer(4 * int(np.prod(shape)), np.uint32, shape)
        flags = (GEO_26 if connectivity == 26 else 0) | (GEO_FROM_LABELS if seed_labels is not None else 0) | (GEO_DENSE if dense else 0)
        status, res = self.mask_geodesic_raw(domain, dims, seeds, seed_labels, flags, weights, DIST_NONE if cap is None else cap,
                                             dist, labels)
        if status != OK:
            for mine, m in zip(own, (dist, labels)):
                if mine:
                    m.release()
        _check(status, "clwh_mask_geodesic")
        return dist, labels, res

    def geodesic_trace_raw(self, dist: Mem, dims, target, labels: Mem = None, flags=0, weights=None, points: Mem = None, capacity=0,
                           result=True):
        """one clwh_geodesic_trace call: (status, n_points); nothing is raised.  result=False passes a NULL n_points."""
        d, n = GeodesicTraceDesc(), C.c_uint64(0)
        d.dist, d.labels, d.points = _handle(dist), _handle(labels), _handle(points)
        d.capacity, d.flags = int(capacity), int(flags)
        for k in range(3):
            d.dims[k], d.target[k] = int(dims[k]), int(target[k])
        self._geodesic_weights(d, weights)
        if result:
            d.n_points = C.pointer(n)
        return lib().clwh_geodesic_trace(self.h, C.byref(d)), int(n.value)

    def geodesic_trace(self, dist: Mem, dims, target, labels: Mem = None, connectivity=6, weights=None, capacity=4096):
        """the shortest path behind mask_geodesic's `dist` from `target` = (x, y, z) back to a seed (inside the target's territory
        when `labels` is given), connectivity and weights as in that call: (points, n_points).  points: uint32 [n][3] = (x, y, z),
        target first, the first min(n_points, capacity) of them; n_points: the true count, 0 for an unreached target.  ClwhError
        for a map that mask_geodesic did not write.  The call waits for the device."""
        if connectivity not in (6, 26):
            raise ValueError("connectivity is 6 or 26")
        capacity = int(capacity)
        buf = self.buffer(max(capacity, 1) * 12, np.uint32)
        try:
            status, n = self.geodesic_trace_raw(dist, dims, target, labels, GEO_26 if connectivity == 26 else 0, weights, buf, capacity)
            _check(status, "clwh_geodesic_trace")
            k = min(n, capacity)
            return (buf.pull(np.uint32)[:3 * k].reshape(k, 3).copy() if k else np.zeros((0, 3), np.uint32)), n
        finally:
            buf.release()

    @staticmethod
    def _cost_multipliers(d, multipliers):
        """multipliers: None (all 1), (fx, fy, fz), or (face, edge, corner) as scene.geodesic_weights returns them"""
        face, edge, corner = (1, 1, 1), (1, 1, 1), 1
        if multipliers is not None:
            if len(multipliers) == 3 and np.ndim(multipliers[0]) == 1:
                face, edge, corner = multipliers
            else:
                face = multipliers
        for k in range(3):
            d.mult_face[k], d.mult_edge[k] = int(face[k]), int(edge[k])
        d.mult_corner = int(corner)

    def cost_from_field_raw(self, source: Mem, cost: Mem, dims, table, lo=0, shift=0, kind=COST_SRC_U32, domain: Mem = None, flags=0,
                            n=None):
        """one clwh_cost_from_field call: its status; nothing is raised.  table: uint16 entries, or None for a NULL table (then `n`
        says how many it claims)"""
        d = CostFieldDesc()
        d.source, d.domain, d.cost = _handle(source), _handle(domain), _handle(cost)
        if table is not None:
            t = np.ascontiguousarray(np.asarray(table, dtype=np.uint16).reshape(-1))
            d.table = t.ctypes.data_as(C.POINTER(C.c_uint16))
        d.n = int(n) if n is not None else (len(t) if table is not None else 0)
        d.lo, d.shift, d.kind, d.flags = int(lo), int(shift), int(kind), int(flags)
        for k in range(3):
            d.dims[k] = int(dims[k])
        return lib().clwh_cost_from_field(self.h, C.byref(d))

    def cost_from_field(self, source: Mem, dims, table, lo=0, shift=0, kind=COST_SRC_U32, domain: Mem = None, cost: Mem = None) -> Mem:
        """a cost field for cost_geodesic: cost(p) = table[clamp((s(p) - lo) >> shift, 0, len(table) - 1)], 0 where `domain` (a mask in
        grow's layout) is given and clear; uint16 [z][y][x] on the device, allocated when none is given.  kind: COST_SRC_U32 (`source`
        is a uint32 [z][y][x] buffer such as mask_distance's map, s its word), COST_SRC_VALUE (`source` is the S16 volume image, s its
        value) or COST_SRC_GRADIENT (the same image, s the squared length of its unscaled central differences).  table: 1 .. 65536
        uint16 entries.  Ordered on the context's stream; does not wait."""
        own = cost is None
        if own:
            shape = (int(dims[2]), int(dims[1]), int(dims[0]))
            cost = self.buffer(2 * int(np.prod(shape)), np.uint16, shape)
        status = self.cost_from_field_raw(source, cost, dims, table, lo, shift, kind, domain)
        if status != OK and own:
            cost.release()
        _check(status, "clwh_cost_from_field")
        return cost

    def cost_geodesic_raw(self, cost: Mem, dims, seeds=None, domain: Mem = None, seed_labels: Mem = None, flags=0, multipliers=None,
                          cap=DIST_NONE, dist: Mem = None, labels: Mem = None, result=True):
        """one clwh_cost_geodesic call: (status, GeodesicResult); nothing is raised.  seeds: rows of (x, y, z, id), or None.
        result=False passes a NULL result."""
        d, res = CostGeodesicDesc(), GeodesicResult()
        d.cost, d.domain, d.seed_labels, d.dist, d.labels = (_handle(m) for m in (cost, domain, seed_labels, dist, labels))
        for k in range(3):
            d.dims[k] = int(dims[k])
        self._cost_multipliers(d, multipliers)
        d.cap, d.flags = int(cap), int(flags)
        if seeds is not None:
            s = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint32).reshape(-1, 4))
            d.n_seeds = len(s)
            d.seeds = s.ctypes.data_as(C.POINTER(C.c_uint32))
        if result:
            d.result = C.pointer(res)
        return lib().clwh_cost_geodesic(self.h, C.byref(d)), res

    def cost_geodesic(self, cost: Mem, dims, seeds=None, domain: Mem = None, seed_labels: Mem = None, connectivity=6, multipliers=None,
                      cap=None, dist: Mem = None, labels: Mem = None, dense=False):
        """shortest paths through the cost field `cost` (uint16 [z][y][x] on the device, 0 = wall; cost_from_field makes one) from
        labelled seeds: (dist, labels, GeodesicResult), as mask_geodesic gives them.  A step INTO a voxel costs the direction's
        multiplier times that voxel's cost.  domain: an optional mask that restricts the paths further.  multipliers: None (all 1),
        (fx, fy, fz), or (face, edge, corner) from scene.geodesic_weights, each within 1 .. 255.  cap: at most COST_CAP_MAX; large costs
        over long paths can pass it, and the voxels behind count as unreached: scale the cost.  The call waits for the device."""
        if connectivity not in (6, 26):
            raise ValueError("connectivity is 6 or 26")
        shape = (int(dims[2]), int(dims[1]), int(dims[0]))
        own = [dist is None, labels is None]
        if own[0]:
            dist = self.buffer(4 * int(np.prod(shape)), np.uint32, shape)
        if own[1]:
            labels = self.buffer(4 * int(np.prod(shape)), np.uint32, shape)
        flags = (GEO_26 if connectivity == 26 else 0) | (GEO_FROM_LABELS if seed_labels is not None else 0) | (GEO_DENSE if dense else 0)
        status, res = self.cost_geodesic_raw(cost, dims, seeds, domain, seed_labels, flags, multipliers, DIST_NONE if cap is None else cap,
                                             dist, labels)
        if status != OK:
            for mine, m in zip(own, (dist, labels)):
                if mine:
                    m.release()
        _check(status, "clwh_cost_geodesic")
        return dist, labels, res

    def watershed_raw(self, cost: Mem, dims, seeds=None, domain: Mem = None, seed_labels: Mem = None, flags=0, plateau_cap=WATERSHED_PLATEAU_MAX,
                      level_cap=WATERSHED_LEVEL_MAX, labels: Mem = None, level: Mem = None, result=True):
        """one clwh_watershed call: (status, WatershedResult); nothing is raised.  seeds: rows of (x, y, z, id), or None.
        result=False passes a NULL result."""
        d, res = WatershedDesc(), WatershedResult()
        d.cost, d.domain, d.seed_labels, d.level, d.labels = (_handle(m) for m in (cost, domain, seed_labels, level, labels))
        for k in range(3):
            d.dims[k] = int(dims[k])
        d.plateau_cap, d.level_cap, d.flags = int(plateau_cap), int(level_cap), int(flags)
        if seeds is not None:
            s = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint32).reshape(-1, 4))
            d.n_seeds = len(s)
            d.seeds = s.ctypes.data_as(C.POINTER(C.c_uint32))
        if result:
            d.result = C.pointer(res)
        return lib().clwh_watershed(self.h, C.byref(d)), res

    def watershed(self, cost: Mem, dims, seeds=None, domain: Mem = None, seed_labels: Mem = None, connectivity=6,
                  plateau_cap=WATERSHED_PLATEAU_MAX, level_cap=WATERSHED_LEVEL_MAX, labels: Mem = None, level: Mem = None, dense=False):
        """the seeded watershed of the cost field `cost` (uint16 [z][y][x] on the device, 0 = wall; cost_from_field makes one): every
        seed floods its basin, and two floods meet on the ridge between them: (labels, level, WatershedResult).  labels: the id of the
        seed whose flood reaches the voxel, 0 where none does; level: M << 16 | L with M the height of the lowest pass from a seed and
        L the steps since that height was reached, saturating at plateau_cap (0: the pure max-cost watershed); DIST_NONE where not
        reached.  A voxel whose M would exceed level_cap is not reached.  seeds: rows of (x, y, z, id) and / or seed_labels (a uint32
        map whose nonzero words are seeds; `labels` may be the same buffer).  The call waits for the device."""
        if connectivity not in (6, 26):
            raise ValueError("connectivity is 6 or 26")
        shape = (int(dims[2]), int(dims[1]), int(dims[0]))
        own = [labels is None, level is None]
        if own[0]:
            labels = self.buffer(4 * int(np.prod(shape)), np.uint32, shape)
        if own[1]:
            level = self.buffer(4 * int(np.prod(shape)), np.uint32, shape)
        flags = (GEO_26 if connectivity == 26 else 0) | (GEO_FROM_LABELS if seed_labels is not None else 0) | (GEO_DENSE if dense else 0)
        status, res = self.watershed_raw(cost, dims, seeds, domain, seed_labels, flags, plateau_cap, level_cap, labels, level)
        if status != OK:
            for mine, m in zip(own, (labels, level)):
                if mine:
                    m.release()
        _check(status, "clwh_watershed")
        return labels, level, res

    def watershed_edges(self, volume: Mem, dims, seeds, domain: Mem = None, connectivity=6, g_max=4096, plateau_cap=WATERSHED_PLATEAU_MAX,
                        level_cap=WATERSHED_LEVEL_MAX, labels: Mem = None, level: Mem = None, dense=False):
        """the watershed of the volume's gradient from clicks: cost_from_field with COST_SRC_GRADIENT through
        scene.watershed_gradient_table(g_max) (cost = 1 + the gradient's length, clamped at g_max), then watershed.  The border between
        two seeds lies on the strongest edge that separates them.  (labels, level, WatershedResult)."""
        from .scene import watershed_gradient_table
        table, shift = watershed_gradient_table(g_max)
        cost = self.cost_from_field(volume, dims, table, 0, shift, COST_SRC_GRADIENT, domain)
        try:
            return self.watershed(cost, dims, seeds, domain, None, connectivity, plateau_cap, level_cap, labels, level, dense)
        finally:
            cost.release()

    def cost_trace_raw(self, cost: Mem, dist: Mem, dims, target, labels: Mem = None, flags=0, multipliers=None, points: Mem = None,
                       capacity=0, result=True):
        """one clwh_cost_trace call: (status, n_points); nothing is raised.  result=False passes a NULL n_points."""
        d, n = CostTraceDesc(), C.c_uint64(0)
        d.cost, d.dist, d.labels, d.points = _handle(cost), _handle(dist), _handle(labels), _handle(points)
        d.capacity, d.flags = int(capacity), int(flags)
        for k in range(3):
            d.dims[k], d.target[k] = int(dims[k]), int(target[k])
        self._cost_multipliers(d, multipliers)
        if result:
            d.n_points = C.pointer(n)
        return lib().clwh_cost_trace(self.h, C.byref(d)), int(n.value)

    def cost_trace(self, cost: Mem, dist: Mem, dims, target, labels: Mem = None, connectivity=6, multipliers=None, capacity=4096):
        """the cheapest path behind cost_geodesic's `dist` from `target` = (x, y, z) back to a seed, with the cost field, connectivity
        and multipliers of that call: (points, n_points) as geodesic_trace gives them.  The call waits for the device."""
        if connectivity not in (6, 26):
            raise ValueError("connectivity is 6 or 26")
        capacity = int(capacity)
        buf = self.buffer(max(capacity, 1) * 12, np.uint32)
        try:
            status, n = self.cost_trace_raw(cost, dist, dims, target, labels, GEO_26 if connectivity == 26 else 0, multipliers, buf, capacity)
            _check(status, "clwh_cost_trace")
            k = min(n, capacity)
            return (buf.pull(np.uint32)[:3 * k].reshape(k, 3).copy() if k else np.zeros((0, 3), np.uint32)), n
        finally:
            buf.release()

    def centerline(self, mask: Mem, dims, start, end, spacing=(1, 1, 1), connectivity=26, max_radius=None, sharpness=100, capacity=4096):
        """the centreline of the structure `mask` (grow's layout, dims = (X, Y, Z)) between the voxels `start` and `end`: (points,
        n_points), uint32 [n][3] = (x, y, z) from `end` back to `start`; scene.path_length measures it.  Four steps: the depth map d^2
        of the mask (mask_distance to the nearest clear voxel, weights scene.mask_weights(spacing)); the cost
        scene.centerline_cost_table over it (the depth shifted right by scene.centerline_shift so that the table has at most 65536
        entries), low in the middle and high at the wall, 0 outside the mask (cost_from_field);
        cost_geodesic from `start` with scene.geodesic_weights(spacing, 10) as multipliers; cost_trace from `end`.  max_radius: the
        largest radius of interest in the unit of `spacing`; deeper voxels all cost 1.  None pulls the depth map and takes its
        largest value inside the mask on the host: a convenience for small volumes; at full size pass the radius.  A start or end
        outside the mask gives n_points = 0.  capacity: the first guess of the path's length; a longer path is traced a second time.
        The call waits for the device."""
        from . import scene

        multipliers = scene.geodesic_weights(spacing, 10)
        if max(max(multipliers[0]), max(multipliers[1]), multipliers[2]) > 255:
            raise ValueError("centerline: a step's multiplier is above 255; use spacing relative to the smallest voxel size")
        weights = scene.mask_weights(spacing)
        X, Y, Z = (int(v) for v in dims)
        depth = self.mask_distance(mask, dims, weights, to_clear=True)
        cost = dist = None
        try:
            if max_radius is None:
                d = depth.pull().reshape(Z, Y, X)
                inside = scene.mask_unpack(mask.pull(np.uint32, (mask.nbytes // 4,)), dims) & (d != DIST_NONE)
                r_sq_max = int(d[inside].max()) if inside.any() else 1
            else:
                r_sq_max = scene.radius_sq(max_radius)
            shift = scene.centerline_shift(r_sq_max)
            table = scene.centerline_cost_table(max(r_sq_max, 1) >> shift, sharpness)
            cost = self.cost_from_field(depth, dims, table, 0, shift, COST_SRC_U32, mask)
            dist, labels, _ = self.cost_geodesic(cost, dims, [tuple(int(v) for v in start) + (1,)], None, None, connectivity, multipliers)
            labels.release()
            points, n = self.cost_trace(cost, dist, dims, end, None, connectivity, multipliers, capacity)
            if n > len(points):  # longer than the first guess: once more with room for all of it
                points, n = self.cost_trace(cost, dist, dims, end, None, connectivity, multipliers, n)
            return points, n
        finally:
            for m in (dist, cost, depth):
                if m is not None:
                    m.release()

    def split_mask(self, volume: Mem, mask: Mem, dims, radius_sq, weights=(1, 1, 1), connectivity=6):
        """a mask whose parts touch, split: (labels, number of parts).  Three steps: the mask is eroded by the ball of radius_sq
        (mask_morph's, with its `weights`) until the bridges break; the pieces that survive are labelled 1, 2, ... largest first
        (label_components over the eroded mask alone: `volume`, the S16 image the mask belongs to, is read with the full value
        window); and the pieces grow back inside the original mask, every voxel going to the piece that reaches it first
        (mask_geodesic with unit steps under `connectivity`, ties to the smaller label).  labels: uint32 [z][y][x] on the device.
        A part of the mask that vanishes under the erosion leaves its voxels unreached (label 0) unless a surviving part reaches
        them.  The call waits for the device."""
        eroded = self.mask_morph(mask, dims, MORPH_ERODE, radius_sq, weights)
        try:
            ranks, res, _ = self.label_components(volume, -32768, 32767, connectivity, mask=eroded, capacity=0)
        finally:
            eroded.release()
        n_parts = int(res.n_components)
        if n_parts == 0:  # nothing survived: label_components wrote 0 everywhere
            return ranks, 0
        status, _ = self.mask_geodesic_raw(mask, dims, None, ranks, GEO_FROM_LABELS | (GEO_26 if connectivity == 26 else 0), labels=ranks)
        if status != OK:
            ranks.release()
        _check(status, "clwh_mask_geodesic")
        return ranks, n_parts

    def mask_statistics_raw(self, volume: Mem, mask: Mem, hist: Mem = None, hist_lo=0, bin_width=0, n_bins=0, flags=0, result=True):
        """one clwh_mask_statistics call: (status, MaskStatsResult); nothing is raised.  result=False passes a NULL result."""
        d, res = MaskStatsDesc(), MaskStatsResult()
        d.volume, d.mask, d.hist = _handle(volume), _handle(mask), _handle(hist)
        d.hist_lo, d.bin_width, d.n_bins, d.flags = int(hist_lo), int(bin_width), int(n_bins), int(flags)
        if result:
            d.result = C.pointer(res)
        return lib().clwh_mask_statistics(self.h, C.byref(d)), res

    def mask_statistics(self, volume: Mem, mask: Mem, hist=None):
        """the exact record of the region of `volume` (S16) whose bits are set in `mask` (grow's layout, whoever made it): (RegionStats,
        histogram or None, below, above).  hist = (lo, width, n): n bins of `width` values from `lo` on, as a uint64 numpy array, with
        the counts of the region's voxels under and over the range.  scene.region_measures turns the record into volume, mean,
        centroid and area.  The call waits for the device."""
        table = None
        try:
            if hist is not None:
                lo, width, n = (int(v) for v in hist)
                table = self.buffer(8 * max(n, 1), np.uint64, (max(n, 1),))
                status, res = self.mask_statistics_raw(volume, mask, table, lo, width, n)
            else:
                status, res = self.mask_statistics_raw(volume, mask)
            _check(status, "clwh_mask_statistics")
            counts = table.pull()[:int(hist[2])].copy() if table is not None else None
            return res.stats, counts, int(res.hist_below), int(res.hist_above)
        finally:
            if table is not None:
                table.release()

    def label_statistics_raw(self, volume: Mem, labels: Mem, stats: Mem, capacity, flags=0):
        """one clwh_label_statistics call: its status; nothing is raised"""
        d = LabelStatsDesc()
        d.volume, d.labels, d.stats = _handle(volume), _handle(labels), _handle(stats)
        d.capacity, d.flags = int(capacity), int(flags)
        return lib().clwh_label_statistics(self.h, C.byref(d))

    def label_statistics(self, volume: Mem, labels: Mem, capacity, stats: Mem = None) -> Mem:
        """one record per rank 1 .. capacity of `labels` (uint32 [z][y][x]: clwh_segment_label's, or any words) over `volume`: the
        device table of `capacity` records, allocated when none is given; stats.pull() is a structured array (REGION_STATS_DTYPE),
        record k for rank k + 1, zero for a rank no voxel has.  Ordered on the context's stream; does not wait."""
        own = stats is None
        if own:
            stats = self.buffer(104 * max(int(capacity), 1), REGION_STATS_DTYPE, (max(int(capacity), 1),))
        status = self.label_statistics_raw(volume, labels, stats, capacity)
        if status != OK and own:
            stats.release()
        _check(status, "clwh_label_statistics")
        return stats

    def scene_info(self):
        """(id, bytes, holders) of the derived scene data this context renders from"""
        sid, nb, holders = C.c_uint64(0), C.c_uint64(0), C.c_int32(0)
        _check(lib().clwh_ctx_scene_info(self.h, C.byref(sid), C.byref(nb), C.byref(holders)), "clwh_ctx_scene_info")
        return int(sid.value), int(nb.value), int(holders.value)

    def device_probe(self, which, records: np.ndarray, params=(0, 0, 0, 0), aux: np.ndarray = None) -> np.ndarray:
        """clwh_debug_device_probe over `records` (uint32 [n][words in]; floats as their bits): uint32 [n][words out]"""
        w_in, w_out = PROBE_WORDS[which]
        rec = np.ascontiguousarray(records, dtype=np.uint32).reshape(-1, w_in)
        n = rec.shape[0]
        m_in, m_out = self.buffer_from(rec if n else np.zeros(1, np.uint32)), self.buffer(max(n, 1) * w_out * 4, np.uint32)
        m_aux = self.buffer_from(np.ascontiguousarray(aux, dtype=np.uint32)) if aux is not None else None
        try:
            _check(lib().clwh_debug_device_probe(self.h, which, m_in.h, C.c_uint64(n), m_out.h, m_aux.h if m_aux else None,
                                                 (C.c_int32 * 4)(*[int(v) for v in params])), "clwh_debug_device_probe")
            self.finish()
            return m_out.pull().reshape(-1, w_out)[:n]
        finally:
            for m in (m_in, m_out, m_aux):
                if m is not None:
                    m.release()

    def macro_table(self):
        """the exit-certificate table of the scene data this context rendered from last: (uint8 [cz][cy][cx][octant], log2 of the
        cell's edge); entries 1..127: the box is free, this is its smallest step value; 0x80 | g: not free, stay away g - 1 cells"""
        info = (C.c_int32 * 4)()
        _check(lib().clwh_debug_macro_table(self.h, None, C.c_uint64(0), info), "clwh_debug_macro_table")
        out = np.empty((info[2], info[1], info[0], 8), np.uint8)
        _check(lib().clwh_debug_macro_table(self.h, out.ctypes.data_as(C.c_void_p), C.c_uint64(out.nbytes), info), "clwh_debug_macro_table")
        return out, int(info[3])

    def packed_scene(self, which):
        """one of the arrays k_repack derived from the scene this context rendered from last, raw and in brick order
        (clwh_debug_packed_scene): SCENE_HIT_RECORDS uint32 [bricks][512][2], SCENE_STEP_BYTES uint8 [bricks][512], SCENE_BRICK_MIN
        uint32 [bricks]; and the bricks along (x, y, z)"""
        info = (C.c_int32 * 4)()
        _check(lib().clwh_debug_packed_scene(self.h, which, None, C.c_uint64(0), info), "clwh_debug_packed_scene")
        n = info[0] * info[1] * info[2]
        out = (np.empty((n, 512, 2), np.uint32) if which == SCENE_HIT_RECORDS else
               np.empty((n, 512), np.uint8) if which == SCENE_STEP_BYTES else np.empty(n, np.uint32))
        _check(lib().clwh_debug_packed_scene(self.h, which, out.ctypes.data_as(C.c_void_p), C.c_uint64(out.nbytes), info), "clwh_debug_packed_scene")
        return out, (int(info[0]), int(info[1]), int(info[2]))

    def view_data(self, which):
        """one of the arrays the views derive from the volume, as this context's last view call left them, raw (clwh_debug_view_data):
        VIEW_BRICKS int16 [bricks][512], VIEW_TABLE / VIEW_DILATED uint32 [bricks], VIEW_COARSE uint32 [cells]; and the bricks along
        (x, y, z).  Raises (status 7) for VIEW_DILATED / VIEW_COARSE while no call has built them."""
        info = (C.c_int32 * 4)()
        _check(lib().clwh_debug_view_data(self.h, which, None, C.c_uint64(0), info), "clwh_debug_view_data")
        n = info[0] * info[1] * info[2]
        out = np.empty((n, 512), np.int16) if which == VIEW_BRICKS else np.empty(info[3] if which == VIEW_COARSE else n, np.uint32)
        _check(lib().clwh_debug_view_data(self.h, which, out.ctypes.data_as(C.c_void_p), C.c_uint64(out.nbytes), info), "clwh_debug_view_data")
        return out, (int(info[0]), int(info[1]), int(info[2]))

    def start_table(self):
        """the start-certificate table of the scene data this context rendered from last: uint8 [z][y][x], bit o set = the box from
        the voxel to the volume corner of direction octant o holds no voxel that may be an event; None when it was not built"""
        info = (C.c_int32 * 4)()
        _check(lib().clwh_debug_start_table(self.h, None, C.c_uint64(0), info), "clwh_debug_start_table")
        if not info[3]:
            return None
        out = np.empty((info[2], info[1], info[0]), np.uint8)
        _check(lib().clwh_debug_start_table(self.h, out.ctypes.data_as(C.c_void_p), C.c_uint64(out.nbytes), info), "clwh_debug_start_table")
        return out

    def hull_table(self):
        """the hull-certificate table of the scene data this context rendered from last: float32 [planes][4] = unit normal n_k, h_k
        (every corner c of every event voxel has n_k . c <= h_k); None when it was not built"""
        info = (C.c_int32 * 4)()
        _check(lib().clwh_debug_hull_table(self.h, None, C.c_uint64(0), info), "clwh_debug_hull_table")
        if not info[3]:
            return None
        out = np.empty((info[1], 4), np.float32)
        _check(lib().clwh_debug_hull_table(self.h, out.ctypes.data_as(C.c_void_p), C.c_uint64(out.nbytes), info), "clwh_debug_hull_table")
        return out

    def hull_h(self):
        """the hull table's h_k alone, float32 [planes], as k_bounce's tilted-plane test reads them (clwh_debug_hull_h); None when the
        table was not built"""
        info = (C.c_int32 * 4)()
        _check(lib().clwh_debug_hull_h(self.h, None, C.c_uint64(0), info), "clwh_debug_hull_h")
        if not info[3]:
            return None
        out = np.empty(info[1], np.float32)
        _check(lib().clwh_debug_hull_h(self.h, out.ctypes.data_as(C.c_void_p), C.c_uint64(out.nbytes), info), "clwh_debug_hull_h")
        return out

    def hull_codes(self):
        """per hit of the camera this context rendered last (hit_records' order): uint32, 0 = no plane, else 1 + plane index in bits
        0-12 and the margin in 1/256 voxels (rounded down) in bits 16-31 (clwh_debug_hull_codes)"""
        n = C.c_uint32(0)
        _check(lib().clwh_debug_hull_codes(self.h, None, C.c_uint64(0), C.byref(n)), "clwh_debug_hull_codes")
        out = np.empty(int(n.value), np.uint32)
        _check(lib().clwh_debug_hull_codes(self.h, out.ctypes.data_as(C.c_void_p), C.c_uint64(out.nbytes), C.byref(n)), "clwh_debug_hull_codes")
        return out[:int(n.value)]

    def hull_planes(self):
        """per hit, hull_codes' order: uint32, 0 = no plane within D voxels, else 1 + plane index in bits 0-12 and the signed margin in
        1/16 voxels (rounded down, two's complement) in bits 16-23 (clwh_debug_hull_planes)"""
        n = C.c_uint32(0)
        _check(lib().clwh_debug_hull_planes(self.h, None, C.c_uint64(0), C.byref(n)), "clwh_debug_hull_planes")
        out = np.empty(int(n.value), np.uint32)
        _check(lib().clwh_debug_hull_planes(self.h, out.ctypes.data_as(C.c_void_p), C.c_uint64(out.nbytes), C.byref(n)), "clwh_debug_hull_planes")
        return out[:int(n.value)]

    def hit_records(self):
        """the hit records of the camera this context rendered last: uint32 [n_hits][16] (clwh_debug_hit_records)"""
        n = C.c_uint32(0)
        _check(lib().clwh_debug_hit_records(self.h, None, C.c_uint64(0), C.byref(n)), "clwh_debug_hit_records")
        out = np.empty((int(n.value), 16), np.uint32)
        _check(lib().clwh_debug_hit_records(self.h, out.ctypes.data_as(C.c_void_p), C.c_uint64(out.nbytes), C.byref(n)), "clwh_debug_hit_records")
        return out[:int(n.value)]

    def image_wrap(self, device_ptr: int, dims, channels, dtype, shape=None) -> Mem:
        """adopt device memory somebody else allocated (a graphics-interop mapping, a torch tensor) as an image"""
        dtype = np.dtype(dtype)
        d = (C.c_size_t * 3)(*(list(dims) + [1, 1, 1])[:3])
        h = C.c_void_p()
        _check(lib().clwh_image_wrap(self.h, C.c_void_p(device_ptr), d, channels, _ELEM_OF_DTYPE[dtype], C.byref(h)),
               "clwh_image_wrap")
        n = int(np.prod([max(int(x), 1) for x in list(dims)[:3]])) * channels * dtype.itemsize
        return Mem(self, h.value, n, dtype, shape)

    def acquire_from(self, stream: int):
        """the context's later work waits for what is queued on `stream` now (display done with the old frame)"""
        _check(lib().clwh_ctx_acquire_from(self.h, C.c_void_p(stream)), "clwh_ctx_acquire_from")

    def release_to(self, stream: int):
        """later work on `stream` waits for what is queued on the context's stream now (frame complete)"""
        _check(lib().clwh_ctx_release_to(self.h, C.c_void_p(stream)), "clwh_ctx_release_to")

    def finish(self):
        _check(lib().clwh_ctx_finish(self.h), "clwh_ctx_finish")

    def set_timing(self, enabled=True):
        _check(lib().clwh_ctx_set_timing(self.h, 1 if enabled else 0), "clwh_ctx_set_timing")

    def timing_read(self):
        """(total ms, launches) of the dominant render kernel since the last read (HIP events)."""
        ms, n = C.c_float(0), C.c_int32(0)
        _check(lib().clwh_ctx_timing_read(self.h, C.byref(ms), C.byref(n)), "clwh_ctx_timing_read")
        return float(ms.value), int(n.value)

    def timing_read_all(self):
        """{kernel: (total ms, launches)} per kernel of the render path since the last read (HIP events)."""
        n = len(TIMERS)
        ms, cnt = (C.c_float * n)(), (C.c_int32 * n)()
        _check(lib().clwh_ctx_timing_read_all(self.h, ms, cnt, n), "clwh_ctx_timing_read_all")
        return {name: (float(ms[i]), int(cnt[i])) for i, name in enumerate(TIMERS)}

    @property
    def stream(self) -> int:
        return int(lib().clwh_ctx_stream(self.h) or 0)

    def destroy(self):
        if self.h:
            _check(lib().clwh_ctx_destroy(self.h), "clwh_ctx_destroy")
            self.h = None
