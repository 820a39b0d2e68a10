"""-m gpu: the exit-certificate table says how long a refused march should stay away (csrc/scene_kernels.hip k_macro_hints;
k_bounce packs the distance beside its step budget; CLWH_TUNE_CERT_HINT=0 ignores it).

The table is read back through clwh_debug_macro_table and compared, cell by cell and octant by octant, with a numpy
restatement: a free entry is the smallest step value of its box; a refusing entry 0x80 | g has no free box at any Chebyshev
offset below g in the octant's direction, and the cell g along the diagonal is free or outside the volume.  The hint only
decides WHEN a look-up is made, so fused launches with the hint on and off, thresholds 4 and 12, cells of 8^3 and 16^3 voxels
must all give the bits of the passes one by one without certificates."""
import os

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests.gpu_util import GpuScene, look_at_centre
from tests.test_gpu_edge_cases import _parity

pytestmark = pytest.mark.gpu

TF = scene.tf_default_source()   # event: 500 <= value <= 1200, no gradient clause
REFUSED = 0x80


def _ctx(**env):
    env = {k: str(v) for k, v in env.items()}
    os.environ.update(env)
    try:
        return ffi.Context(0)
    finally:
        for k in env:
            del os.environ[k]


def _expected_free_boxes(vol, sdf, shift):
    """[octant][cz][cy][cx]: the smallest step value of the box between the cell and the corner the octant heads for, 0 = not free"""
    Z, Y, X = vol.shape
    edge = 1 << shift
    event = (vol >= 500) & (vol <= 1200)
    free = np.where(event | (sdf <= 0), 0, sdf.astype(np.int32))
    n = [(d + edge - 1) // edge for d in (Z, Y, X)]
    padded = np.full((n[0] * edge, n[1] * edge, n[2] * edge), 255, np.int32)   # beyond the volume: no voxel, no constraint
    padded[:Z, :Y, :X] = free
    cell = padded.reshape(n[0], edge, n[1], edge, n[2], edge).min(axis=(1, 3, 5))
    cell[cell < 2] = 0   # kCertMinStep
    out = np.empty((8,) + cell.shape, np.int32)
    for o in range(8):
        flips = [ax for ax, bit in ((2, 1), (1, 2), (0, 4)) if not (o & bit)]   # positive direction: accumulate from the far end
        b = np.flip(cell, flips) if flips else cell
        for ax in range(3):
            b = np.minimum.accumulate(b, axis=ax)
        out[o] = np.flip(b, flips) if flips else b
    return out


def _check_table(table, shift, vol, sdf):
    want = _expected_free_boxes(vol, sdf, shift)
    MNZ, MNY, MNX = want.shape[1:]
    assert table.shape == (MNZ, MNY, MNX, 8)
    refusing = 0
    for o in range(8):
        got = table[..., o].astype(np.int32)
        is_free = want[o] > 0
        assert np.array_equal(got[is_free], want[o][is_free]), "free entries: the box's smallest step value"
        assert np.all(got[~is_free] & REFUSED) and np.all(got[~is_free] & 0x7F), "refusing entries carry g >= 1"
        # look along the octant's direction as +x, +y, +z
        flips = [ax for ax, bit in ((2, 1), (1, 2), (0, 4)) if o & bit]
        F = np.flip(is_free, flips) if flips else is_free
        G = np.where(is_free, 0, got & 0x7F)
        G = np.flip(G, flips) if flips else G
        # near[m]: some cell at offsets 0..m on every axis has a free box
        near = [F.copy()]
        for _ in range(max(MNX, MNY, MNZ)):
            w = near[-1].copy()
            for ax in range(3):
                s = np.zeros_like(w)
                src = [slice(None)] * 3
                dst = [slice(None)] * 3
                src[ax], dst[ax] = slice(1, None), slice(0, -1)
                s[tuple(dst)] = w[tuple(src)]
                w |= s
            near.append(w)
        for cz, cy, cx in zip(*np.nonzero(~F)):
            g = int(G[cz, cy, cx])
            assert g < 127
            assert not near[g - 1][cz, cy, cx], "a free box nearer than the hint says"
            z, y, x = cz + g, cy + g, cx + g
            assert z - 1 < MNZ and y - 1 < MNY and x - 1 < MNX, "the diagonal left the volume before g cells"
            assert z >= MNZ or y >= MNY or x >= MNX or F[z, y, x], "the cell g along the diagonal is neither free nor outside"
            refusing += 1
    return refusing, int((want > 0).sum())


def _scene_volumes():
    ball = scene.phantom(64)
    rng = np.random.default_rng(3)
    odd = np.full((32, 80, 48), -900, np.int16)   # 48 x 80 x 32
    odd[6:20, 30:52, 10:30] = 900
    odd[26:32, 70:80, 40:48] = 1000   # a second object in the far corner
    odd += rng.integers(-20, 21, size=odd.shape, dtype=np.int16)
    return {"phantom64": ball, "48x80x32": odd}


@pytest.mark.parametrize("shift", [3, 4])
@pytest.mark.parametrize("name", ["phantom64", "48x80x32"])
def test_table_against_numpy(orc, name, shift):
    vol = _scene_volumes()[name]
    sdf, _, _ = orc.sdf_build(vol, orc.parse_tf(TF))
    ctx = _ctx(CLWH_TUNE_MACRO_SHIFT=shift)
    try:
        g = GpuScene(ctx, vol, sdf, scene.env_map(64, 32), TF, (16, 16))
        pos, d = look_at_centre(vol, [-20, 100, -30])
        g.render(pos, d, 1, debug=False)
        table, got_shift = ctx.macro_table()
        g.release()
    finally:
        ctx.destroy()
    assert got_shift == shift
    refusing, free = _check_table(table, shift, vol, sdf)
    assert refusing >= 50 and free >= 8   # both kinds of entry occur (the 16^3 cells of the phantom: only the corner cells' own octants are free)


def test_hint_changes_no_bit(gpu_ctx, orc):
    """64 seeds fused: hint on / off x threshold 4 / 12 x cells of 8^3 / 16^3 voxels, against 64 single-pass launches (short launches
    never ask for certificates)"""
    vol = scene.phantom(64)
    sdf, _, _ = orc.sdf_build(vol, orc.parse_tf(TF))
    env = scene.env_map(256, 128)
    pos, d = scene.default_camera(64)
    seeds = scene.glibc_rand(64)

    def run(ctx, fused):
        g = GpuScene(ctx, vol, sdf, env, TF, (96, 64))
        if fused:
            g.render(pos, d, None, mode=ffi.ACCUM_IMAGE_SPACE, seeds=seeds, debug=False)
        else:
            for s in seeds:
                g.render(pos, d, s, mode=ffi.ACCUM_IMAGE_SPACE, debug=False)
        out = (g.accum[0].pull(np.float32).copy(), g.frame.pull().copy())
        g.release()
        return out

    want = run(gpu_ctx, False)
    assert want[0].reshape(-1, 4)[:, 3].max() == 64.0
    for shift in (3, 4):
        for cert in (4, 12):
            for hint in (1, 0):
                ctx = _ctx(CLWH_TUNE_LONG_LAUNCH=1, CLWH_TUNE_MACRO_SHIFT=shift, CLWH_TUNE_CERT=cert, CLWH_TUNE_CERT_HINT=hint)
                try:
                    got = run(ctx, True)
                finally:
                    ctx.destroy()
                assert np.array_equal(got[0], want[0]), "accumulation (cells 2^%d, threshold %d, hint %d)" % (shift, cert, hint)
                assert np.array_equal(got[1], want[1]), "frame (cells 2^%d, threshold %d, hint %d)" % (shift, cert, hint)


@pytest.mark.parametrize("shift", [3, 4])
def test_nothing_free_and_everything_free(orc, shift):
    """an event voxel in every brick: no box is ever free, every entry refuses and g counts the cells to the end of the volume; no
    events at all: every entry is free.  Both render like the oracle (whose marches end after 70 steps) under long-launch scheduling
    with look-ups from a step length of 2."""
    ctx = _ctx(CLWH_TUNE_LONG_LAUNCH=1, CLWH_TUNE_MACRO_SHIFT=shift, CLWH_TUNE_CERT=2)
    try:
        lattice = np.full((48, 64, 56), -900, np.int16)
        for k in range(27):   # a 3^3 blob of event voxels in every brick
            lattice[2 + k // 9::8, 3 + k // 3 % 3::8, 1 + k % 3::8] = 900
        pos, d = look_at_centre(lattice, [-25, 90, -30])
        env = scene.env_map(64, 32)
        hits = _parity(orc, ctx, lattice, env, TF, (96, 64), pos, d, scene.glibc_rand(2), mode="image")
        assert hits > 300
        table, _ = ctx.macro_table()
        MNZ, MNY, MNX = table.shape[:3]
        cz, cy, cx = np.mgrid[0:MNZ, 0:MNY, 0:MNX]
        for o in range(8):
            to_end = np.minimum(np.minimum(cx + 1 if o & 1 else MNX - cx, cy + 1 if o & 2 else MNY - cy), cz + 1 if o & 4 else MNZ - cz)
            assert np.array_equal(table[..., o], (REFUSED | to_end).astype(np.uint8))
        empty = np.full((48, 64, 56), -900, np.int16)
        sdf, _, _ = orc.sdf_build(empty, orc.parse_tf(TF))
        assert _parity(orc, ctx, empty, env, TF, (96, 64), pos, d, scene.glibc_rand(2), mode="image") == 0
        table, _ = ctx.macro_table()
        assert not np.any(table & REFUSED)
        assert np.array_equal(table, np.broadcast_to(np.uint8(sdf.min()), table.shape))
    finally:
        ctx.destroy()
