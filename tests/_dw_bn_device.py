"""Device harness of the depthwise / BatchNorm exact-data edge tests
(tests/test_dw_train_edges.py, tests/test_bn_train_edges.py): sentinel-tailed
output buffers, uploads, logged C-ABI calls, the equality and ulp checks, and
the per-module record of the worst distance observed.  Numpy references and
case tables: tests/_dw_bn_exact.py."""
import numpy as np
import torch

import _dw_bn_exact as E

TAIL = 64
SENTINEL = 12345.6789


def L():
    from jabd_amd import _lib
    return _lib


class Figures(dict):
    """name -> worst observed distance (ulp, or fraction of a bound) of one
    test module (each module keeps its own)."""

    def note(self, name, v):
        self[name] = max(self.get(name, 0.0), float(v))

    def report(self):
        print("worst observed:", {k: round(v, 3) for k, v in sorted(self.items())})


def scratch(n):
    """n floats the library may be handed in a call it must reject: device
    memory where there is a device, so that a wrongly accepted call cannot
    make a kernel read host memory."""
    return torch.zeros(n, dtype=torch.float32,
                       device="cuda:0" if torch.cuda.is_available() else "cpu")


class Out:
    """An output buffer: the body prefilled with NaN (or `init`), a sentinel tail."""

    def __init__(self, dev, *shape, init=None):
        self.shape = shape
        self.n = int(np.prod(shape))
        self.t = torch.full((self.n + TAIL,), float("nan"), dtype=torch.float32, device=dev)
        self.t[self.n:] = SENTINEL
        if init is not None:
            self.t[:self.n] = torch.from_numpy(np.asarray(init, dtype=np.float32).reshape(-1))

    @property
    def ptr(self):
        return self.t.data_ptr()

    def get(self, name, finite=True):
        tail = self.t[self.n:].cpu().numpy()
        assert np.all(tail == np.float32(SENTINEL)), f"{name}: sentinel tail overwritten"
        if finite is None:                           # a workspace: the tail only
            return None
        body = self.t[:self.n].cpu().numpy().reshape(self.shape)
        if finite:
            assert np.isfinite(body).all(), f"{name}: elements never written"
        return body.astype(np.float64)


def up(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def logged(fn, *args):
    lib = L()
    lib.launch_log_reset()
    lib.call(fn, *args)
    return [n for n, _ in lib.launch_log()]


def eq(name, cid, got, ref):
    assert got.shape == ref.shape, (cid, name, got.shape, ref.shape)
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        i = tuple(bad[0])
        raise AssertionError(f"{cid} {name}: {len(bad)} of {got.size} elements differ, first at "
                             f"{i}: got {got[i]!r}, exact value {ref[i]!r}")


def ulp(fig, name, cid, got, ref64, bar):
    dist = E.ulp_dist(got, ref64.astype(np.float32))
    fig.note(name, dist.max())
    assert dist.max() <= bar, f"{cid} {name}: {int(dist.max())} ulp from the fp64 value (bar {bar})"
