"""predict.tile_plan (the tile origins of sliced detection) and the host side
of the tile kernels' C ABI: known answers, the plan's properties over a sweep,
argument errors, and the status of bad calls.  No test here needs a GPU."""
import ctypes
import math
import os

import numpy as np
import pytest

import _tile_ref as R


def _axis(L, t, o):
    """The x origins of a one-row plan (the y axis is a single tile)."""
    from jabd_amd.predict import tile_plan
    p = tile_plan(32, L, tile=(32, t), overlap=(0, o))
    assert p.dtype == np.int32 and p.ndim == 2 and p.shape[1] == 2 and (p[:, 0] == 0).all()
    return p[:, 1].tolist()


def test_known_answers():
    assert _axis(160, 64, 16) == [0, 48, 96]
    assert _axis(96, 64, 16) == [0, 32]
    assert _axis(64, 64, 16) == [0]
    assert _axis(40, 64, 16) == [0]


def test_plan_is_row_major_and_takes_ints_for_pairs():
    from jabd_amd.predict import tile_plan
    p = tile_plan(96, 160, tile=(64, 64), overlap=(16, 16))
    assert p.tolist() == [[0, 0], [0, 48], [0, 96], [32, 0], [32, 48], [32, 96]]
    assert tile_plan(96, 160, tile=64, overlap=16).tolist() == p.tolist()
    assert p.tolist() == R.plan(96, 160, (64, 64), (16, 16)).tolist()
    # both axes have their own tile and overlap
    q = tile_plan(100, 300, tile=(64, 128), overlap=(8, 32))
    assert q.tolist() == R.plan(100, 300, (64, 128), (8, 32)).tolist()
    assert sorted(set(q[:, 0].tolist())) == [0, 36] and sorted(set(q[:, 1].tolist())) == [0, 96, 172]


def test_properties_over_a_sweep():
    n = 0
    for t in (32, 64, 96):
        for o in (0, 1, 16, 31, t - 1):
            for L in list(range(1, 3 * t + 2, 7)) + [t - 1, t, t + 1, 2 * t - o, 2 * t - o + 1]:
                org = _axis(L, t, o)
                assert org == R.axis_origins(L, t, o)
                assert org[0] == 0 and org == sorted(set(org))          # strictly ascending
                covered = np.zeros(L, bool)
                for x in org:
                    covered[max(x, 0):x + t] = True
                assert covered.all(), (L, t, o)
                assert all(b - a <= t - o for a, b in zip(org, org[1:])), (L, t, o)
                if L >= t:
                    assert org[-1] + t == L, (L, t, o)                  # flush with the edge
                else:
                    assert org == [0]
                n += 1
    assert n > 300


@pytest.mark.parametrize("kw", [
    {"tile": (48, 64)}, {"tile": (64, 40)}, {"tile": (0, 64)}, {"tile": (-32, 64)},
    {"tile": (64, 64, 64)}, {"tile": 63.5},
    {"overlap": (64, 0)}, {"overlap": (0, 64)}, {"overlap": (-1, 0)}, {"overlap": 100},
    {"overlap": (1, 2, 3)},
])
def test_argument_errors(kw):
    from jabd_amd.predict import tile_plan
    with pytest.raises(ValueError):
        tile_plan(100, 100, **{"tile": (64, 64), "overlap": (16, 16), **kw})


def test_bad_image_size_raises():
    from jabd_amd.predict import tile_plan
    for ih, iw in ((0, 10), (10, 0), (-1, 10)):
        with pytest.raises(ValueError):
            tile_plan(ih, iw, tile=(64, 64), overlap=(16, 16))


def test_new_names_are_declared_everywhere():
    from conftest import ROOT
    from jabd_amd import _lib, ops, predict
    header = open(os.path.join(ROOT, "include", "jabd.h")).read()
    h = _lib.lib()
    for name in ("jabd_tile_gather_f32", "jabd_tile_collect_workspace_size",
                 "jabd_tile_collect_f32"):
        assert name in _lib.SIGNATURES and name + "(" in header and hasattr(h, name)
    assert len(_lib.SIGNATURES["jabd_tile_gather_f32"]) == 12
    assert len(_lib.SIGNATURES["jabd_tile_collect_f32"]) == 17
    for mod, names in ((ops, ("tile_gather", "tile_collect")),
                       (predict, ("tile_plan", "detect_image_tiled"))):
        for name in names:
            assert callable(getattr(mod, name))


def test_bad_calls_return_einval_without_a_device():
    from jabd_amd import _lib
    h = _lib.lib()
    mean = (ctypes.c_float * 3)(104, 117, 123)
    mp = ctypes.cast(mean, ctypes.c_void_p)

    def gather(src_null=True, ih=8, iw=8, n=1, th=32, tw=32, m=mp):
        return h.jabd_tile_gather_f32(None, 0, ih, iw, None, n, th, tw, 84.0, m, None, None)
    for kw in ({}, {"ih": 0}, {"iw": -1}, {"n": -1}, {"th": 0}, {"tw": 0}, {"m": None},
               {"n": 1 << 31}):
        assert gather(**kw) == 1, kw
        assert "tile_gather" in _lib.last_error()
    assert gather(n=0) == 0                                  # launches nothing

    def collect(n=1, A=4, th=32, tw=32, ih=64, iw=64, border=1.0, cap=4, p=0):
        return h.jabd_tile_collect_f32(None, None, n, A, None, th, tw, ih, iw, border, None, cap,
                                       None, p, None, 0, None)
    for kw in ({}, {"n": -1}, {"A": -1}, {"th": 0}, {"tw": 0}, {"ih": 0}, {"iw": 0},
               {"border": math.nan}, {"cap": -1}, {"p": -1}, {"n": 65536}, {"A": 1 << 28},
               {"n": 0}, {"A": 0}):                          # null offsets even when empty
        assert collect(**kw) == 1, kw
        assert "tile_collect" in _lib.last_error()
    out = ctypes.c_size_t(0)
    assert h.jabd_tile_collect_workspace_size(3, 700, ctypes.byref(out)) == 0
    assert out.value >= 3 * 700 * 4 + 3 * 4
    assert h.jabd_tile_collect_workspace_size(-1, 700, ctypes.byref(out)) == 1
    assert h.jabd_tile_collect_workspace_size(3, -1, ctypes.byref(out)) == 1
    assert h.jabd_tile_collect_workspace_size(3, 700, None) == 1
