"""bench.py --dump-outputs: what dump_outputs writes (no GPU needed).

Small outputs are written whole in their own shape; outputs above
bench.DUMP_BYTES are written as the same seeded, ordered sample of
(image, anchor) rows of loc / conf / landm, identical from call to call and
within the byte budget."""
import numpy as np
import torch


def _outputs(B, A):
    g = torch.Generator().manual_seed(3)
    return tuple(torch.rand((B, A, k), generator=g) for k in (4, 2, 10))


def test_dump_outputs_whole(tmp_path):
    import bench
    out = _outputs(2, 37)
    bench.dump_outputs(out, str(tmp_path / "d"))
    for name, o in zip(("loc", "conf", "landm"), out):
        a = np.load(tmp_path / "d" / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == tuple(o.shape)
        np.testing.assert_array_equal(a, o.numpy())


def test_dump_outputs_sampled(tmp_path, monkeypatch):
    import bench
    assert bench.DUMP_BYTES <= 64 * 10**6
    monkeypatch.setattr(bench, "DUMP_BYTES", 64 * 25)      # 25 rows of 16 floats
    out = _outputs(3, 41)
    bench.dump_outputs(out, str(tmp_path / "a"))
    bench.dump_outputs(out, str(tmp_path / "b"))
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("loc", "conf", "landm")}
    assert sum(a.nbytes for a in got.values()) <= 64 * 25
    for n, a in got.items():
        assert a.dtype == np.float32 and a.shape[0] == 25
        np.testing.assert_array_equal(a, np.load(tmp_path / "b" / f"{n}.npy"))
    # the same rows of every output, in order: find them through loc
    flat = [o.numpy().reshape(3 * 41, -1) for o in out]
    rows = [int(np.flatnonzero((flat[0] == r).all(1))[0]) for r in got["loc"]]
    assert rows == sorted(set(rows))
    np.testing.assert_array_equal(got["conf"], flat[1][rows])
    np.testing.assert_array_equal(got["landm"], flat[2][rows])
