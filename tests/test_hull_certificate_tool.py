"""tools/hull_certificate.py, the numpy restatement of the hull certificate, checked on the CPU: the support
table against brute force, the octahedral grid, the step bound, and that the convex scene of tests/test_gpu_hull_cert.py gives at
least one hit in three a plane by the restatement alone."""
import os
import sys

import numpy as np
import pytest

from cl_volume_renderer_amd import scene

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import hull_certificate as hc  # noqa: E402


@pytest.mark.parametrize("unit", [True, False])
def test_support_table_equals_brute_force(unit):
    rng = np.random.default_rng(5)
    event = rng.random((9, 7, 11)) < 0.05
    event[4, 3, 2:9] = True   # a row with several event voxels: only its ends count
    dirs = hc.oct_directions(8, unit)
    z, y, x = np.nonzero(event)
    corners = np.concatenate([np.stack([x + dx, y + dy, z + dz], axis=1) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)]).astype(np.float64)
    want = (corners @ dirs.T).max(axis=0)
    assert np.allclose(hc.support_table(event, dirs), want, rtol=0, atol=1e-12)
    assert np.all(np.isneginf(hc.support_table(np.zeros_like(event), dirs)))


def test_octahedral_grid():
    for G in (8, 32, 64):
        dirs = hc.oct_directions(G, unit=True)
        assert dirs.shape == (G * G, 3) and np.allclose(np.linalg.norm(dirs, axis=1), 1.0)
        i, j = hc.oct_cell(dirs, G)
        assert np.array_equal(j * G + i, np.arange(G * G)), "a cell's centre decodes to a direction of that cell"
        exact = hc.oct_directions(G, unit=False)
        assert np.array_equal(exact * G, np.round(exact * G)) and np.allclose(np.abs(exact).sum(axis=1), 1.0)
    # every direction is close to one of the grid: 64 x 64 cells leave less than 3 degrees
    v = np.random.default_rng(2).normal(size=(2000, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    assert (v @ hc.oct_directions(64).T).max(axis=1).min() > np.cos(np.radians(3.0))


def test_step_bound():
    d512 = hc.hull_delta0(512, 512, 512, 0.0)
    assert 0.1875 <= d512 <= 0.25   # the issue's hand estimate
    assert hc.hull_delta0(64, 64, 64, 0.0) <= d512 <= hc.hull_delta0(2048, 2048, 2048, 0.0) <= 1.0
    assert hc.hull_delta0(512, 512, 512, 4.0) <= d512   # a start further in front of the plane can only help
    assert hc.hull_steps_ok(512, 512, 512, d512, 0.0, 65) and not hc.hull_steps_ok(512, 512, 512, d512 - 1.0 / 64, 0.0, 65)


def _shell(n=64):
    c = (n - 1) / 2.0
    z, y, x = np.mgrid[0:n, 0:n, 0:n].astype(np.float32)
    r = np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2)
    vol = np.full((n, n, n), -1000, np.int16)
    vol[r < 0.42 * n] = 40
    vol[(r > 0.30 * n) & (r < 0.36 * n)] = 900
    return vol


def test_convex_scene_grants_one_hit_in_three_by_the_restatement_alone(orc):
    vol = _shell()
    sdf = orc.sdf_build(vol, orc.parse_tf(scene.tf_default_source()))[0]
    event = (vol >= 500) & (vol <= 1200)
    pos = np.array([-30.0, 80.0, -40.0], np.float32)
    d = np.array([32.0, 32.0, 32.0], np.float32) - pos
    d = (d / np.linalg.norm(d)).astype(np.float32)
    o, cd, normal = hc.primary_hits(vol, sdf, event, pos, d, 128, 96)
    assert len(o) > 300
    P = ((o + cd) + normal * np.float32(2.0)).astype(np.float32)
    dirs = hc.oct_directions(64)
    h = hc.support_table(event, dirs) + 0.0625 + 2.0 ** -9   # the device table's slack, at its largest
    k, m = hc.choose_plane(P, normal, dirs, h, 64, radius=None)
    assert 3 * np.count_nonzero(m >= 0) >= len(m), "%d of %d hits have a plane" % (np.count_nonzero(m >= 0), len(m))
    # every chosen plane has all event voxels behind it and the start point in front
    assert np.all((P[m >= 0].astype(np.float64) * dirs[k[m >= 0]]).sum(axis=1) > hc.support_table(event, dirs)[k[m >= 0]])
    # legs: with such a plane, four in five of the sampled hemisphere directions clear delta0 ... of the hits that have one
    legs = hc.sample_legs(normal, np.random.default_rng(3))
    delta0 = hc.hull_delta0(64, 64, 64, 0.0)
    granted = (m >= 0) & ((legs.astype(np.float64) * dirs[np.maximum(k, 0)]).sum(axis=1) >= delta0)
    assert np.count_nonzero(granted) >= 0.5 * np.count_nonzero(m >= 0)
