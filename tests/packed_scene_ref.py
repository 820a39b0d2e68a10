"""numpy restatement of the arrays the kernels derive from the scene, from their documented contracts (csrc/packed_volume.hpp's header
comment, csrc/clwh_internal.hpp's ViewVolume comment, DESIGN.md 2 "Semantics"), for the read-back tests of clwh_debug_packed_scene and
clwh_debug_view_data.  No GPU.

Brick order: a volume of X x Y x Z voxels is stored in NBX x NBY x NBZ bricks of 8^3 voxels, NB = ceil(dim / 8), a brick in eight 4^3
sub-bricks, x fastest inside a sub-brick; a brick's slots beyond the volume are padding.  Everything here is index arithmetic over
whole arrays: slot_index names the slot of every voxel, scatter() and gather() move an x-fastest array [z][y][x] into [brick][512]
and back.

Render side (k_repack): classes, `maybe`, step bytes, hit records and the per-brick free value from (volume, SDF, rules), rules being
orc_ffi.parse_tf(source).as_tuples() -- the parser the oracle renders with.  Views side (k_proj_repack, k_iso_dilate, k_iso_coarse):
the bricked copy and the three {min, max} tables."""
import numpy as np

from tests import isosurface_ref as ir

SLOTS = 512          # per brick
SUB_SLOTS = 64       # per 4^3 sub-brick: 64 consecutive slots


def brick_counts(dims):
    """(NBX, NBY, NBZ) of a volume of dims = (X, Y, Z)"""
    return tuple((int(n) + 7) // 8 for n in dims)


def slot_index(x, y, z, nbx, nby):
    """the slot of voxel (x, y, z): brick number * 512 + the offset inside the brick.  Bricks run x fastest; inside a brick the
    sub-brick (bit 2 of z, y, x) comes first, then z, y, x inside the sub-brick (two bits each)"""
    x, y, z = (np.asarray(v, np.int64) for v in (x, y, z))
    brick = ((z // 8) * nby + (y // 8)) * nbx + (x // 8)
    sub = ((z % 8) // 4) * 4 + ((y % 8) // 4) * 2 + ((x % 8) // 4)
    inside = (z % 4) * 16 + (y % 4) * 4 + (x % 4)
    return brick * SLOTS + sub * SUB_SLOTS + inside


def _voxel_slots(shape):
    Z, Y, X = shape
    nbx, nby, _ = brick_counts((X, Y, Z))
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    return slot_index(x, y, z, nbx, nby)


def scatter(a, fill=0):
    """a [z][y][x][...] -> [bricks][512][...] in brick order, padding slots = fill"""
    a = np.asarray(a)
    Z, Y, X = a.shape[:3]
    nb = brick_counts((X, Y, Z))
    out = np.full((nb[0] * nb[1] * nb[2] * SLOTS,) + a.shape[3:], fill, a.dtype)
    out[_voxel_slots((Z, Y, X)).reshape(-1)] = a.reshape((-1,) + a.shape[3:])
    return out.reshape((-1, SLOTS) + a.shape[3:])


def gather(bricked, dims):
    """[bricks][512][...] -> [z][y][x][...]: the real voxels' slots"""
    X, Y, Z = dims
    b = np.asarray(bricked)
    flat = b.reshape((-1,) + b.shape[2:])
    return flat[_voxel_slots((Z, Y, X))]


def real_slots(dims):
    """bool [bricks][512]: the slot holds a voxel of the volume"""
    X, Y, Z = dims
    return scatter(np.ones((Z, Y, X), bool), False)


# ---- render side

def central_differences(vol):
    """(gx, gy, gz) int32 [z][y][x]: V(p + e) - V(p - e) per axis, 0 outside the volume"""
    v = np.asarray(vol).astype(np.int32)
    p = np.pad(v, 1)
    c = slice(1, -1)
    return p[c, c, 2:] - p[c, c, :-2], p[c, 2:, c] - p[c, :-2, c], p[2:, c, c] - p[:-2, c, c]


def gradient_short(gx, gy, gz):
    """the `gradient` a rule reads: the binary32 length (gx^2 + gy^2) + gz^2, its square root, truncated to int, wrapped to short"""
    fx, fy, fz = (np.asarray(g).astype(np.float32) for g in (gx, gy, gz))
    length = np.sqrt((fx * fx + fy * fy) + fz * fz, dtype=np.float32)
    return length.astype(np.int32).astype(np.int16).astype(np.int32)


def classify(vol, rules):
    """(class uint8, maybe bool) [z][y][x] of a rule table (Tf.as_tuples()): class = 1 + the index of the first rule the voxel
    satisfies, 0 = none, a terminal rule ends the walk matched or not; maybe = class != 0, or the value lies in the value window of a
    rule the walk reaches (a rule that reads `gradient` may be evaluated with other taps than the voxel's own)"""
    value = np.asarray(vol).astype(np.int32)
    gradient = None
    if any(r[4] for r in rules):  # formed only when a rule reads it
        gradient = gradient_short(*central_differences(vol))
    cls = np.zeros(value.shape, np.uint8)
    maybe = np.zeros(value.shape, bool)
    walking = np.ones(value.shape, bool)  # the voxel's walk has not ended before this rule
    for k, (v_lo, v_hi, g_lo, g_hi, use_gradient, _writes, terminal, _color) in enumerate(rules):
        window = (value >= v_lo) & (value <= v_hi)
        match = window & (gradient >= g_lo) & (gradient <= g_hi) if use_gradient else window
        maybe |= walking & window
        cls[walking & match] = k + 1
        walking = walking & ~match
        if terminal:
            walking[:] = False
    return cls, maybe | (cls != 0)


def pack_record(gx, gy, gz, cls):
    """uint32 [...][2]: word 0 = gx[16:0] | gy[14:0] << 17, word 1 = gy[16:15] | gz[16:0] << 2 | class << 19"""
    ux, uy, uz = (np.asarray(g).astype(np.int64) & 0x1FFFF for g in (gx, gy, gz))
    c = np.asarray(cls).astype(np.int64) & 0xFF
    w0 = (ux | (uy << 17)) & 0xFFFFFFFF
    w1 = (uy >> 15) | (uz << 2) | (c << 19)
    return np.stack([w0, w1], axis=-1).astype(np.uint32)


def unpack_class(records):
    return (np.asarray(records)[..., 1] >> 19) & 0xFF


class PackedScene:
    """what k_repack must have written for (vol, sdf) under `rules` (Tf.as_tuples()) or, for a transfer function outside the rule
    grammar, under the per-voxel `classes` (then maybe = class != 0):
      cls, maybe    [z][y][x]
      stepb         uint8 [bricks][512]: 0x80 * [class != 0] | max(sdf, 0), padding 0
      grec          uint32 [bricks][512][2], padding (0, 0)
      brick_min     uint32 [bricks]: the smallest free value of the brick's real voxels, free = 0 if maybe or sdf <= 0 else sdf
      written       bool [bricks][8]: the sub-brick holds a `maybe` voxel -- its records are specified, the others are not"""

    def __init__(self, vol, sdf, rules=None, classes=None):
        vol = np.asarray(vol, np.int16)
        sdf = np.asarray(sdf, np.int8)
        assert vol.shape == sdf.shape and (rules is None) != (classes is None)
        Z, Y, X = vol.shape
        self.dims = (X, Y, Z)
        self.nb = brick_counts(self.dims)
        if classes is None:
            self.cls, self.maybe = classify(vol, rules)
        else:
            self.cls = np.asarray(classes, np.uint8)
            self.maybe = self.cls != 0
        step = np.maximum(sdf.astype(np.int32), 0)
        self.stepb = scatter((np.where(self.cls != 0, 0x80, 0) | step).astype(np.uint8), 0)
        self.grec = scatter(pack_record(*central_differences(vol), self.cls), 0)
        free = np.where(self.maybe | (sdf <= 0), 0, sdf.astype(np.int32))
        self.brick_min = scatter(free, 255).min(axis=1).astype(np.uint32)
        self.written = scatter(self.maybe, False).reshape(-1, 8, SUB_SLOTS).any(axis=2)

    def compared_slots(self):
        """bool [bricks][512]: the slots whose record is specified"""
        return np.repeat(self.written, SUB_SLOTS, axis=1)


# ---- views side

def pack_min_max(lo, hi):
    """(uint16)min | (uint16)max << 16"""
    return ((np.asarray(lo).astype(np.int64) & 0xFFFF) | ((np.asarray(hi).astype(np.int64) & 0xFFFF) << 16)).astype(np.uint32)


def _coarse(lo, hi):
    """per cell of 4^3 bricks the minimum of lo and the maximum of hi [NBZ][NBY][NBX], partial last cells included"""
    pad = [(0, -n % 4) for n in lo.shape]
    lo = np.pad(lo, pad, constant_values=1 << 20)
    hi = np.pad(hi, pad, constant_values=-(1 << 20))
    cz, cy, cx = (n // 4 for n in lo.shape)
    return lo.reshape(cz, 4, cy, 4, cx, 4).min(axis=(1, 3, 5)), hi.reshape(cz, 4, cy, 4, cx, 4).max(axis=(1, 3, 5))


class ViewData:
    """what the views' build kernels must have written for vol:
      bricks   int16 [bricks][512], padding 0
      table    uint32 [bricks]: min and max over the brick's real voxels
      dilated  uint32 [bricks]: over the brick grown by one voxel, clamped at the faces
      coarse   uint32 [cells]: per cell of 4^3 bricks over its bricks' dilated pairs, cells x fastest"""

    def __init__(self, vol):
        vol = np.asarray(vol, np.int16)
        Z, Y, X = vol.shape
        self.dims = (X, Y, Z)
        self.nb = brick_counts(self.dims)
        self.bricks = scatter(vol, 0)
        wide = vol.astype(np.int32)
        self.table = pack_min_max(scatter(wide, 1 << 20).min(axis=1), scatter(wide, -(1 << 20)).max(axis=1))
        dmin, dmax = ir.dilated_brick_bounds(vol)
        self.dilated = pack_min_max(dmin, dmax).reshape(-1)
        self.coarse = pack_min_max(*_coarse(dmin, dmax)).reshape(-1)
