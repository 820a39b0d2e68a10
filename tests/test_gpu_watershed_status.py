"""clwh_watershed's exact status for every invalid call, in the order of kinds the header gives, and that nothing is written on any of
them; then that the same arguments without the defect are accepted, limits included."""
import ctypes as C

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests import watershed_ref as w

pytestmark = pytest.mark.gpu

INVALID_VALUE, SIZE_MISMATCH = 1, 9
PATTERN = 0xA5A5A5A5


def test_status_codes_and_nothing_written(gpu_ctx):
    ctx = gpu_ctx
    dims = X, Y, Z = (70, 12, 9)
    n, words = X * Y * Z, scene.mask_words_per_row(X) * Y * Z
    assert n % 2 == 0
    fill = lambda k: ctx.buffer_from(np.full(k, PATTERN, np.uint32))
    domain, short_domain = fill(words), fill(words - 1)
    cost, short_cost = fill(n // 2), fill(n // 2 - 1)  # 2 * n bytes exactly, and two bytes less
    level, labels, given, short_map = fill(n + 4), fill(n + 4), fill(n), fill(n - 1)
    as_image = ctx.image([4, 4, n // 16 + 1], 1, np.uint32)
    odd_domain = ctx.wrap(domain.device_ptr + 4, 4 * words - 4)
    odd_map = ctx.wrap(level.device_ptr + 2, 4 * n)
    odd_cost = ctx.wrap(level.device_ptr + 1, 2 * n)
    seeds = [(1, 2, 3, 4)]
    bad_dims = ((0, 12, 9), (70, 0, 9), (70, 12, 0), (1 << 31, 1, 1), (1 << 16, 1 << 15, 1))

    def ws(**kw):
        args = dict(cost=cost, dims=dims, seeds=seeds, domain=domain, seed_labels=None, flags=0, plateau_cap=w.PLATEAU_MAX,
                    level_cap=w.LEVEL_MAX, labels=labels, level=level)
        args.update(kw)
        return ctx.watershed_raw(**args)[0]

    L = ffi.lib()
    assert L.clwh_watershed(None, C.byref(ffi.WatershedDesc())) == INVALID_VALUE and L.clwh_watershed(ctx.h, None) == INVALID_VALUE
    cases = [ws(result=False)]
    cases += [ws(cost=bad) for bad in (None, as_image, odd_cost)]
    cases += [ws(domain=bad) for bad in (as_image, odd_domain)]
    cases += [ws(level=None, labels=None)]
    for bad in (as_image, odd_map):
        cases += [ws(level=bad), ws(labels=bad), ws(level=None, labels=bad), ws(level=bad, labels=None),
                  ws(seed_labels=bad, flags=ffi.GEO_FROM_LABELS)]
    cases += [ws(seed_labels=None, flags=ffi.GEO_FROM_LABELS)]
    cases += [ws(flags=8), ws(flags=-1), ws(flags=1 << 16)]
    cases += [ws(dims=bad) for bad in bad_dims]
    cases += [ws(plateau_cap=65535), ws(plateau_cap=1 << 16), ws(plateau_cap=0xFFFFFFFF)]
    cases += [ws(level_cap=65536), ws(level_cap=0xFFFFFFFF)]
    cases += [ws(seeds=[(1, 2, 3, 4)] * (ffi.GROW_MAX_SEEDS + 1)), ws(seeds=None), ws(seeds=[]), ws(seeds=None, seed_labels=given)]
    cases += [ws(seeds=[(1, 2, 3, 4), bad]) for bad in ((70, 2, 3, 4), (1, 12, 3, 4), (1, 2, 9, 4), (1, 2, 3, 0))]
    assert cases == [INVALID_VALUE] * len(cases), cases
    # n_seeds > 0 with NULL seeds
    d, res = ffi.WatershedDesc(), ffi.WatershedResult()
    d.cost, d.level, d.n_seeds, d.result, d.plateau_cap, d.level_cap = cost.h, level.h, 1, C.pointer(res), w.PLATEAU_MAX, w.LEVEL_MAX
    for k in range(3):
        d.dims[k] = dims[k]
    assert L.clwh_watershed(ctx.h, C.byref(d)) == INVALID_VALUE
    sizes = [ws(cost=short_cost), ws(domain=short_domain), ws(level=short_map), ws(labels=short_map),
             ws(seed_labels=short_map, flags=ffi.GEO_FROM_LABELS)]
    assert sizes == [SIZE_MISMATCH] * len(sizes), sizes
    # INVALID_VALUE before SIZE_MISMATCH, whichever argument carries it
    assert ws(cost=short_cost, plateau_cap=65535) == INVALID_VALUE and ws(domain=short_domain, seeds=[(1, 2, 3, 0)]) == INVALID_VALUE
    assert ws(level=short_map, level_cap=65536) == INVALID_VALUE and ws(labels=short_map, flags=8) == INVALID_VALUE
    for m in (domain, short_domain, cost, short_cost, level, labels, given, short_map):
        assert (m.pull(np.uint32, (m.nbytes // 4,)) == PATTERN).all()  # nothing was written
    # and the same arguments without the defect are accepted, limits included
    assert ws() == 0 and ws(plateau_cap=0, level_cap=0) == 0 and ws(flags=ffi.GEO_DENSE | ffi.GEO_26, level=None) == 0
    assert ws(domain=None, labels=None) == 0 and ws(seed_labels=as_image) == 0, "no domain; seed_labels ignored without the flag"
    assert ws(seeds=None, seed_labels=given, flags=ffi.GEO_FROM_LABELS) == 0
    assert (level.pull()[n:] == PATTERN).all() and (labels.pull()[n:] == PATTERN).all() and (domain.pull() == PATTERN).all()
    pattern_cost = np.full(n // 2, PATTERN, np.uint32).view(np.uint16).reshape(Z, Y, X)
    want = w.watershed(pattern_cost, None, 6, seed_labels=np.full((Z, Y, X), PATTERN, np.uint32),
                       domain=scene.mask_unpack(np.full(words, PATTERN, np.uint32), dims))
    assert np.array_equal(labels.pull()[:n].reshape(Z, Y, X), want[0]), "the pattern as cost, as domain and as labels"
    assert np.array_equal(level.pull()[:n].reshape(Z, Y, X), want[1])
    for x in (odd_cost, odd_map, odd_domain, as_image, short_map, given, labels, level, short_cost, cost, short_domain, domain):
        x.release()
