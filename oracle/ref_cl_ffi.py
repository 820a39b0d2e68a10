"""ctypes binding of oracle/_ref/libref_cl_<tf>.so: the REFERENCE's own OpenCL C kernels compiled for the host
(oracle/ref/Makefile) behind the driver of oracle/ref/ref_cl_shim.cpp.

TEST INFRASTRUCTURE ONLY: used by tests/golden/make_ref_render_golden.py to record fixtures and by tests/test_ref_render.py to
check that the fixtures still follow from their recipe.  Nothing here reads the reference tree; where the library was not
built, available() is False.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
ELEM_I8, ELEM_I16, ELEM_RGBA8 = 0, 1, 2


def lib_path(tf_name: str) -> str:
    return os.path.join(_HERE, "_ref", "libref_cl_%s.so" % tf_name)


def available(tf_name: str) -> bool:
    return os.path.exists(lib_path(tf_name))


_libs = {}


def lib(tf_name: str):
    if tf_name not in _libs:
        L = C.CDLL(lib_path(tf_name))
        L.refcl_abi_status.restype = C.c_int
        if L.refcl_abi_status() != 0:
            raise RuntimeError("libref_cl_%s: ABI self-check failed at step %d" % (tf_name, L.refcl_abi_status()))
        L.refcl_out_of_range.restype = C.c_longlong
        L.refcl_exit_depths.restype = C.c_longlong
        L.refcl_exit_depths.argtypes = [C.c_void_p]
        L.refcl_image.restype = C.c_void_p
        L.refcl_image.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.refcl_image_free.argtypes = [C.c_void_p]
        L.refcl_render.restype = C.c_int
        L.refcl_render.argtypes = [C.c_void_p] * 5 + [C.c_longlong, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                      C.c_void_p]
        L.refcl_render_ao.restype = C.c_int
        L.refcl_render_ao.argtypes = [C.c_void_p] * 4 + [C.c_longlong, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.refcl_bilateral_filter.restype = C.c_int
        L.refcl_bilateral_filter.argtypes = [C.c_void_p] * 3
        L.refcl_fetch_stats.restype = C.c_int
        L.refcl_fetch_stats.argtypes = [C.c_void_p] * 3
        L.refcl_apply_clip.restype = C.c_int
        L.refcl_apply_clip.argtypes = [C.c_void_p] * 5
        L.refcl_tf_sort_values.restype = C.c_longlong
        L.refcl_tf_sort_values.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_float] * 4 + [C.c_void_p]
        L.refcl_buffer_reset.restype = C.c_int
        L.refcl_buffer_reset.argtypes = [C.c_void_p] * 3
        _libs[tf_name] = L
    return _libs[tf_name]


def _f3(v):
    return np.ascontiguousarray(v, dtype=np.float32)


class Image:
    """an image over a numpy array the caller keeps alive: [z][y][x] int8 / int16 or [y][x][4] uint8"""

    def __init__(self, L, array):
        self.L, self.array = L, array
        if array.dtype == np.uint8:
            h, w = array.shape[:2]
            self.h = L.refcl_image(w, h, 1, ELEM_RGBA8, array.ctypes.data)
        else:
            d, h, w = array.shape
            self.h = L.refcl_image(w, h, d, ELEM_I8 if array.dtype == np.int8 else ELEM_I16, array.ctypes.data)

    def __del__(self):
        self.L.refcl_image_free(self.h)


def _even(n, by=8):
    return (n + by - 1) // by * by


def _global(dims, global_size):
    g = global_size or [_even(dims[0]), _even(dims[1]), _even(dims[2])]  # get_volume_size_evenness(8), app/reference_volume.cpp:76
    return np.array(g, np.int32)


class Scene:
    """One render job on the reference's kernels, with the buffers of oracle.orc_ffi.Scene: cache, frame, hit_index, contrib
    (light) or shade (ambient occlusion).  Every launch runs the work-items one after the other, rows outer, x inner."""

    def __init__(self, tf_name, volume, sdf, env, frame_wh, launch_wh=None):
        self.L = lib(tf_name)
        self.volume = np.ascontiguousarray(volume, dtype=np.int16)
        self.sdf = np.ascontiguousarray(sdf, dtype=np.int8)
        self.env = np.ascontiguousarray(env, dtype=np.uint8)
        Z, Y, X = self.volume.shape
        self.frame_w, self.frame_h = frame_wh
        self.launch_w, self.launch_h = launch_wh or frame_wh
        self.cache = np.zeros((X * Z * Y + X * Z + X + 1) * 4, dtype=np.uint16)  # utility.cl:21 for the last voxel the march can name
        self.frame = np.zeros((self.frame_h, self.frame_w, 4), dtype=np.uint8)
        npx = self.launch_w * self.launch_h
        self.hit_index = np.full(npx, -1, dtype=np.int64)
        self.contrib = np.zeros((npx, 4), dtype=np.uint32)
        self.shade = np.zeros(npx, dtype=np.uint32)
        self._im = [Image(self.L, a) for a in (self.frame, self.volume, self.sdf, self.env)]

    def reset(self):
        """buffer_reset.cl over the volume's grid; the padding past the last voxel is never written by any kernel before it"""
        Z, Y, X = self.volume.shape
        rc = self.L.refcl_buffer_reset(self._im[1].h, self.cache.ctypes.data, _global((X, Y, Z), None).ctypes.data)
        assert rc == 0, rc

    def render(self, cam_pos, cam_dir, seed):
        p, d = _f3(cam_pos), _f3(cam_dir)
        f, v, s, e = (im.h for im in self._im)
        rc = self.L.refcl_render(f, v, s, e, self.cache.ctypes.data, self.cache.size, p.ctypes.data, d.ctypes.data, int(seed),
                                 self.launch_w, self.launch_h, self.hit_index.ctypes.data, self.contrib.ctypes.data)
        if rc != 0:
            raise RuntimeError("refcl_render failed: %d" % rc)
        depths = np.zeros(3, np.int64)
        odd = self.L.refcl_exit_depths(depths.ctypes.data)
        assert odd == 0, "the shim's path trace met %d calls it could not place" % odd
        self.exit_depths = depths  # paths of this launch that ended in Exit_volume with i = 8, 9, 10

    def render_ao(self, cam_pos, cam_dir, seed):
        p, d = _f3(cam_pos), _f3(cam_dir)
        f, v, s, _ = (im.h for im in self._im)
        rc = self.L.refcl_render_ao(f, v, s, self.cache.ctypes.data, self.cache.size, p.ctypes.data, d.ctypes.data, int(seed),
                                    self.launch_w, self.launch_h, self.shade.ctypes.data)
        if rc != 0:
            raise RuntimeError("refcl_render_ao failed: %d" % rc)


def bilateral_filter(volume, tf_name="default", global_size=None):
    L = lib(tf_name)
    v = np.ascontiguousarray(volume, dtype=np.int16)
    out = np.zeros_like(v)
    Z, Y, X = v.shape
    a, b = Image(L, v), Image(L, out)
    rc = L.refcl_bilateral_filter(a.h, b.h, _global((X, Y, Z), global_size).ctypes.data)
    assert rc == 0, rc
    return out


def fetch_stats(volume, init, tf_name="default", global_size=None):
    L = lib(tf_name)
    v = np.ascontiguousarray(volume, dtype=np.int16)
    stats = np.array(init, dtype=np.int32)
    Z, Y, X = v.shape
    a = Image(L, v)
    rc = L.refcl_fetch_stats(a.h, stats.ctypes.data, _global((X, Y, Z), global_size).ctypes.data)
    assert rc == 0, rc
    return stats


def apply_clip(volume, start, length, tf_name="default", before=None, global_size=None):
    """`before`: the destination image's content before the launch (its shape is the image's); zeros of `length` otherwise"""
    L = lib(tf_name)
    v = np.ascontiguousarray(volume, dtype=np.int16)
    out = np.zeros((length[2], length[1], length[0]), np.int16) if before is None else np.array(before, dtype=np.int16)
    b_start = np.array(start, np.uint32)
    b_end = np.array(list(length) + [4], np.uint32)
    a, b = Image(L, v), Image(L, out)
    g = np.array(global_size or out.shape[::-1], np.int32)
    rc = L.refcl_apply_clip(a.h, b.h, b_start.ctypes.data, b_end.ctypes.data, g.ctypes.data)
    assert rc == 0, rc
    return out


def tf_sort_values(volume, width, height, min_v, max_v, min_g, max_g, tf_name="default", global_size=None):
    """(frame[width * height] indexed x * height + y, number of increments that fell outside it and were dropped)"""
    L = lib(tf_name)
    v = np.ascontiguousarray(volume, dtype=np.int16)
    frame = np.zeros(width * height, np.uint32)
    Z, Y, X = v.shape
    a = Image(L, v)
    dropped = L.refcl_tf_sort_values(a.h, frame.ctypes.data, width, height, min_v, max_v, min_g, max_g,
                                     _global((X, Y, Z), global_size).ctypes.data)
    assert dropped >= 0, dropped
    return frame, int(dropped)
