"""What the GPU tests of the views share (test_gpu_projection, _composite, _isosurface, _slice, _mesh): bit patterns, camera
poses, each view's frame and outputs with their check, volumes as images, two volumes with constant regions, and the host mirror's library."""
import ctypes as C
import os

import numpy as np

from cl_volume_renderer_amd import scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def toward(pos, target):
    v = np.asarray(target, np.float64) - np.asarray(pos, np.float64)
    return (v / np.linalg.norm(v)).astype(F)


def image_of(ctx, vol):
    Z, Y, X = vol.shape
    if X > 1:
        return ctx.image_from(vol), None
    owner = ctx.buffer_from(vol)  # (clwh_image_create refuses a width of 1, as clw_image does; a wrap takes any dims)
    return ctx.image_wrap(owner.device_ptr, (X, Y, Z), 1, np.int16), owner


def pose(name, dims):
    X, Y, Z = dims
    n = max(dims)
    centre = np.array([(X - 1) / 2, (Y - 1) / 2, (Z - 1) / 2], F)
    if name == "default":  # (aimed at the centre when the default direction would miss a flat or tiny volume)
        pos, d = scene.default_camera(n)
        return pos, (d if X == Y == Z and n >= 8 else toward(pos, centre))
    if name == "close":  # scene.close_camera about the centre of a box that need not be a cube
        d = scene.camera_direction(0.9, 6.183)
        return (centre - d * F(0.6 * n)).astype(F), d
    return np.array([X * 0.45, Y * 0.55, Z * 0.5], F), scene.camera_direction(2.1, 0.4)


def plant_blocks(vol):
    """constant blocks on three faces of a random volume: a hit inside one has a zero gradient"""
    Z, Y, X = vol.shape
    vol[:6, :6, :6] = 32767
    vol[Z - 6:, Y - 6:, X - 6:] = -32768
    vol[Z // 2 - 3:Z // 2 + 3, :6, X - 6:] = 32767
    vol[:6, Y - 6:, :6] = -32768
    return vol


def quiet_phantom(n):
    """the phantom without its noise: constant regions, so that hits inside them have a zero gradient"""
    v = scene.phantom(n)
    return np.where(v < -500, -1000, np.where(v < 500, 40, 900)).astype(np.int16)


class Outputs:
    """a frame + the optional outputs of one view on one context; a subclass names the outputs and makes the call"""
    NAMES, FLOATS = (), ()  # the method's keyword per optional output, and its floats per pixel

    def __init__(self, ctx, frame_wh, region_wh):
        self.ctx, self.frame_wh, self.region_wh = ctx, frame_wh, region_wh
        fw, fh = frame_wh
        w, h = region_wh
        self.frame = ctx.image([fw, fh], 4, np.uint8, (fh, fw, 4))
        self.outputs = [ctx.buffer(w * h * 4 * n, np.float32, (h, w) if n == 1 else (h, w, n)) for n in self.FLOATS]

    def render(self, method, before, after=(), **kw):
        """method(frame, *before, region width, region height, *after, **kw, **outputs): (frame of the region, *outputs)"""
        fw, fh = self.frame_wh
        w, h = self.region_wh
        self.frame.push(np.full((fh, fw, 4), 7, np.uint8))  # pixels outside the region keep this
        method(self.frame, *before, w, h, *after, **kw, **dict(zip(self.NAMES, self.outputs)))
        frame = self.frame.pull()
        assert np.all(frame[h:] == 7) and np.all(frame[:, w:] == 7)
        return (frame[:h, :w],) + tuple(o.pull() for o in self.outputs)

    def release(self):
        for m in [self.frame] + self.outputs:
            m.release()

    @classmethod
    def check(cls, got, want, what=""):
        """the frame's bytes and every output's bit patterns (`want` may carry more behind them)"""
        assert np.array_equal(got[0], want[0]), "frame differs %s: %d pixels" % (what, int((got[0] != want[0]).any(axis=-1).sum()))
        for name, g, w in zip(cls.NAMES, got[1:], want[1:]):
            bad = bits(g) != bits(w)
            assert not bad.any(), "%s differs %s: %d values, first at %s" % (name, what, int(bad.sum()), tuple(np.argwhere(bad)[0]))


class Proj(Outputs):
    NAMES, FLOATS = ("values", "t_extreme"), (1, 1)

    def run(self, volume, pos, d, mode, dense=False, **kw):
        return self.render(self.ctx.render_projection, (volume, pos, d), mode=mode, dense=dense, **kw)


class Comp(Outputs):
    NAMES, FLOATS = ("rgba", "t_first", "t_stop"), (4, 1, 1)

    def run(self, volume, pos, d, lut, lut_first, **kw):
        return self.render(self.ctx.render_composite, (volume, pos, d), (lut, lut_first), **kw)


class Iso(Outputs):
    NAMES, FLOATS = ("t_hit", "normal"), (1, 4)

    def run(self, volume, pos, d, iso, **kw):
        return self.render(self.ctx.render_isosurface, (volume, pos, d), (iso,), **kw)


class Slice(Outputs):
    NAMES, FLOATS = ("values", "t_extreme"), (1, 1)

    def run(self, volume, case, mode, flags=0):
        c = case
        return self.render(self.ctx.render_slice, (volume, c["origin"], c["du"], c["dv"], c["normal"]), mode=mode,
                           slab_samples=c["n"], step=c["step"], window=c["window"], flags=flags)


def host_lib(**signatures):
    """libclvr_host.so with the calls every test makes declared, and `signatures`: name=(restype, argtypes) of the test's own"""
    L = C.CDLL(os.path.join(ROOT, "cl_volume_renderer_amd", "libclvr_host.so"))
    L.clvr_host_create.restype = C.c_void_p
    L.clvr_host_destroy.argtypes = [C.c_void_p]
    L.clvr_host_load.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_uint, C.c_uint]
    L.clvr_host_flush.argtypes = [C.c_void_p, C.c_char_p]
    for name, (restype, argtypes) in signatures.items():
        getattr(L, name).restype = restype
        getattr(L, name).argtypes = argtypes
    return L
