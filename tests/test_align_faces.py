"""ops.align_faces / jabd_align_faces_u8 against tests/_align_ref.py, by bytes,
crops and matrices alike.

The scene: six slots.  A 3 x 3 image without a face leads (offsets[0] ==
offsets[1]), images of 12 x 9 and 33 x 47 follow, then a 7 x 5 image without a
face between two that have faces, the 64 x 48 image, and an empty slot that
owns one face.  The odd image sizes put every pool offset off any alignment.
The faces: upscaled, half outside the image, rotated by 37 degrees, mirrored,
scaled down into each sub-sample count (2, 3, 4 and far below 1/4), and the
invalid ones: a NaN landmark, five equal landmarks, the face of the empty slot."""
import ctypes

import numpy as np
import pytest
import torch

import _align_ref as R

SIZES = [(3, 3), (12, 9), (33, 47), (7, 5), (64, 48)]
MEAN, STD = (100.0, 110.5, 127.5), (50.0, 64.0, 127.5)


def _scene(size, template):
    """(pool, desc, rows [11, 15], offsets) on the host for a crop size and
    template; the expected sub-sample counts per face."""
    rng = np.random.default_rng(11)
    images = [rng.integers(0, 256, (ih, iw, 3)).astype(np.uint8) for ih, iw in SIZES]
    desc, off = [], 0
    for im in images:
        desc.append((off, im.shape[0], im.shape[1]))
        off += im.size
    desc.append((0, 0, 0))                               # the empty slot
    pool = np.concatenate([im.reshape(-1) for im in images])
    q = R.default_template(size) if template is None else template
    mid = (size / 2.0, size / 2.0)

    def face(scale, deg, centre, mirror=False):
        lm = R.similar(q, scale, np.deg2rad(deg), centre, rng, 0.02 * size, mid)
        if mirror:
            lm[:, 0] = np.float32(2 * centre[0]) - lm[:, 0]
        return lm.reshape(10)
    per_image = [
        [],
        [face(2.5, 5, (4.3, 6.1)), face(1.2, -10, (8.5, 1.0))],          # upscaled; half outside
        [face(1.3, 37, (20.2, 15.7)), face(0.9, 12, (30.0, 20.0), True), face(0.7, -20, (24, 16))],
        [],
        [face(0.4, 8, (24, 30)), face(0.28, -5, (25, 33)), face(0.1, 3, (20, 30)),
         np.full(10, 17.5, np.float32)],
        [face(1.5, 0, (4, 4))],                                          # owned by the empty slot
    ]
    per_image[4].insert(2, per_image[4][0].copy())
    per_image[4][2][3] = np.nan
    counts = [len(f) for f in per_image]
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rows = np.zeros((int(offsets[-1]), 15), np.float32)
    rows[:, :5] = rng.uniform(0, 40, (rows.shape[0], 5)).astype(np.float32)
    rows[:, 5:] = np.concatenate([f for fs in per_image for f in fs]).reshape(-1, 10)
    return pool, np.array(desc, np.int64), rows, offsets


# (the mirrored set has no good fit without a reflection: its scale comes out small)
S_WANT = [1, 1, 1, 4, 2, 3, 4, 0, 4, 0, 0]


def _run(cuda, pool, desc, rows, offsets, cap, size, template, matrices=None, **kw):
    """ops.align_faces on `cap` rows (the scene's rows cut or padded with NaN
    rows) into buffers that hold a sentinel, and the restatement's answer."""
    from jabd_amd import ops
    padded = np.full((cap, 15), np.nan, np.float32)
    padded[:min(cap, len(rows))] = rows[:cap]
    out = kw.get("out", "u8")
    shape = (cap, size, size, 3) if out == "u8" else (cap, 3, size, size)
    c0 = (np.full(shape, 0xAB, np.uint8) if out == "u8" else np.full(shape, -7.25, np.float32))
    m0 = np.full((cap, 6), 123.0, np.float32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)   # noqa: E731
    crops = dev(c0)
    mats = dev(m0) if matrices is None else matrices
    got_c, got_m = ops.align_faces(dev(pool), dev(desc), dev(padded), dev(offsets), size=size,
                                   template=template, crops=crops, matrices=mats, **kw)
    assert got_c is crops
    want_c, want_m, ss = R.align_faces(pool, desc, padded, offsets, size, template, crops=c0,
                                       matrices=m0, **kw)
    return got_c.cpu().numpy(), None if got_m is None else got_m.cpu().numpy(), want_c, want_m, ss


CASES = [
    # size, template scale (None: the default), kwargs, launch tag
    (8, None, {}, 4),
    (7, None, {}, 1),
    (16, 0.85, {}, 4),
    (8, None, {"antialias": False}, 4),
    (16, None, {"out": "f32", "mean": MEAN, "std": STD, "bgr": True}, 4),
    (7, 0.85, {"out": "f32", "mean": 127.5, "std": 127.5}, 1),
]


@pytest.mark.gpu
@pytest.mark.parametrize("size,tscale,kw,tag", CASES)
def test_crops_and_matrices_are_the_restatement_bit_for_bit(cuda, size, tscale, kw, tag):
    from jabd_amd import _lib
    template = None
    if tscale is not None:       # a scaled template, about the crop's centre
        template = ((R.default_template(size) - np.float32(size / 2)) * np.float32(tscale)
                    + np.float32(size / 2)).astype(np.float32)
    pool, desc, rows, offsets = _scene(size, template)
    cap = len(rows) + 3                                  # more rows than faces
    _lib.launch_log_reset()
    got_c, got_m, want_c, want_m, ss = _run(cuda, pool, desc, rows, offsets, cap, size, template,
                                            **kw)
    assert _lib.launch_log() == [("align_faces", tag)]
    assert ss == (S_WANT if kw.get("antialias", True) else [min(s, 1) for s in S_WANT])
    bad = [r for r in range(cap) if got_c[r].tobytes() != want_c[r].tobytes()]
    assert not bad, f"crops of faces {bad} differ"
    assert got_m.tobytes() == want_m.tobytes()
    # the sentinel beyond the count survived, and the faces are not trivially empty
    n = len(rows)
    assert (got_m[n:] == 123.0).all() and (got_m[:n] != 123.0).all()
    if kw.get("out", "u8") == "u8":
        assert (got_c[n:] == 0xAB).all()
        assert all(got_c[r].any() for r in (0, 1, 2, 3, 4, 5, 6, 8))
        assert not got_c[[7, 9, 10]].any() and not got_m[[7, 9, 10]].any()
    else:
        assert (got_c[n:] == -7.25).all()
        m = np.broadcast_to(np.float32(kw["mean"]), (3,))
        s = np.broadcast_to(np.float32(kw["std"]), (3,))
        blank = ((np.float32(0) - m) / s)[:, None, None]
        assert all(np.array_equal(got_c[r], np.broadcast_to(blank, got_c[r].shape))
                   for r in (7, 9, 10))


@pytest.mark.gpu
def test_cap_below_the_count_and_no_matrices(cuda):
    pool, desc, rows, offsets = _scene(8, None)
    cap = len(rows) - 4
    got_c, got_m, want_c, want_m, ss = _run(cuda, pool, desc, rows, offsets, cap, 8, None)
    assert len(ss) == cap and got_c.tobytes() == want_c.tobytes()
    assert got_m.tobytes() == want_m.tobytes() and not (got_m == 123.0).any()
    none_c, none_m, _, _, _ = _run(cuda, pool, desc, rows, offsets, cap, 8, None, matrices=False)
    assert none_m is None and none_c.tobytes() == want_c.tobytes()


@pytest.mark.gpu
def test_defaults_allocate_and_a_second_run_and_a_graph_replay_agree(cuda):
    from jabd_amd import ops
    pool, desc, rows, offsets = _scene(16, None)
    dev = [torch.from_numpy(a).to(cuda) for a in (pool, desc, rows, offsets)]
    want_c, want_m, _ = R.align_faces(pool, desc, rows, offsets, 16)
    first = ops.align_faces(*dev, size=16)
    assert first[0].shape == (len(rows), 16, 16, 3) and first[0].dtype == torch.uint8
    assert first[1].shape == (len(rows), 6) and first[1].dtype == torch.float32
    assert first[0].cpu().numpy().tobytes() == want_c.tobytes()
    assert first[1].cpu().numpy().tobytes() == want_m.tobytes()
    assert np.array_equal(ops.align_template(16), R.default_template(16))
    crops = torch.zeros_like(first[0])
    mats = torch.zeros_like(first[1])
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        ops.align_faces(*dev, size=16, crops=crops, matrices=mats)
    torch.cuda.current_stream(cuda).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.align_faces(*dev, size=16, crops=crops, matrices=mats)
    crops.zero_()
    mats.zero_()
    graph.replay()
    assert crops.cpu().numpy().tobytes() == want_c.tobytes()
    assert mats.cpu().numpy().tobytes() == want_m.tobytes()


@pytest.mark.gpu
def test_nothing_to_do_launches_nothing(cuda):
    from jabd_amd import _lib, ops
    pool, desc, rows, offsets = _scene(8, None)
    dev = lambda a: torch.from_numpy(a).to(cuda)         # noqa: E731
    _lib.launch_log_reset()
    c, m = ops.align_faces(dev(pool), dev(desc), dev(rows[:0]), dev(offsets), size=8)
    assert c.shape == (0, 8, 8, 3) and m.shape == (0, 6)
    c, m = ops.align_faces(dev(pool), dev(desc[:0]), dev(rows), dev(offsets[:1]), size=8)
    assert c.shape == (len(rows), 8, 8, 3)
    assert _lib.launch_log() == []


@pytest.mark.gpu
def test_bad_arguments_are_einval_before_any_launch(cuda):
    from jabd_amd import _lib
    pool, desc, rows, offsets = _scene(8, None)
    t = [torch.from_numpy(a).to(cuda) for a in (pool, desc, rows, offsets)]
    crops = torch.zeros((len(rows), 8, 8, 3), dtype=torch.uint8, device=cuda)
    f3 = lambda *v: (ctypes.c_float * len(v))(*v)        # noqa: E731
    good = dict(template=f3(*R.default_template(8).reshape(10)), size=8, kind=0,
                mean=f3(0, 0, 0), std=f3(1, 1, 1))

    def call(**change):
        a = dict(good, **change)
        p = lambda x: ctypes.cast(x, ctypes.c_void_p)    # noqa: E731
        _lib.call("jabd_align_faces_u8", t[0].data_ptr(), t[0].numel(), t[1].data_ptr(),
                  t[1].shape[0], t[2].data_ptr(), t[3].data_ptr(), t[2].shape[0],
                  p(a["template"]), a["size"], 1, a["kind"], p(a["mean"]), p(a["std"]), 0,
                  crops.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    _lib.launch_log_reset()
    nan_t = list(R.default_template(8).reshape(10))
    nan_t[4] = float("nan")
    for change in ({"size": 0}, {"size": 1025}, {"kind": 2}, {"kind": -1},
                   {"std": f3(1, 0, 1)}, {"std": f3(1, 1, float("inf"))},
                   {"std": f3(float("nan"), 1, 1)}, {"template": f3(*nan_t)},
                   {"template": f3(*([float("inf")] + nan_t[1:4] + [1.0] + nan_t[5:]))}):
        with pytest.raises(RuntimeError, match=r"status 1\b"):
            call(**change)
    assert _lib.launch_log() == []
    call()                                               # the unchanged arguments pass
    assert _lib.launch_log() == [("align_faces", 4)]


def test_a_cpu_tensor_and_bad_host_arguments_are_rejected():
    from jabd_amd import ops
    pool, desc, rows, offsets = (torch.from_numpy(a) for a in _scene(8, None))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.align_faces(pool, desc, rows, offsets, size=8)
    for kw in ({"size": 0}, {"size": 1025}, {"out": "u16"}, {"std": 0.0},
               {"std": (1.0, float("nan"), 1.0)}, {"template": np.zeros((4, 2), np.float32)},
               {"template": np.full((5, 2), np.inf, np.float32)}):
        with pytest.raises(ValueError):
            ops._align_args("align_faces", **dict({"size": 8, "template": None, "out": "u8",
                                                   "mean": 127.5, "std": 127.5}, **kw))


@pytest.mark.gpu
def test_predict_align_faces_is_the_single_image_call(cuda):
    from jabd_amd import predict
    pool, desc, rows, offsets = _scene(8, None)
    off, ih, iw = (int(v) for v in desc[2])
    image = pool[off:off + 3 * ih * iw].reshape(ih, iw, 3)
    dets = rows[offsets[2]:offsets[3]]
    want_c, want_m, _ = R.align_faces(image.reshape(-1), [[0, ih, iw]], dets, [0, len(dets)], 8)
    crops, mats = predict.align_faces(image, dets, size=8, device=cuda)
    assert isinstance(crops, np.ndarray) and crops.dtype == np.uint8
    assert crops.tobytes() == want_c.tobytes() and mats.tobytes() == want_m.tobytes()
    f32, _ = predict.align_faces(image, dets, size=8, out="f32", mean=MEAN, std=STD, bgr=True,
                                 device=cuda)
    want_f, _, _ = R.align_faces(image.reshape(-1), [[0, ih, iw]], dets, [0, len(dets)], 8,
                                 out="f32", mean=MEAN, std=STD, bgr=True)
    assert f32.dtype == np.float32 and f32.tobytes() == want_f.tobytes()


def test_predict_align_faces_without_detections_needs_no_device():
    from jabd_amd import predict
    image = np.zeros((5, 4, 3), np.uint8)
    for dets in ([], np.zeros((0, 15), np.float32)):
        crops, mats = predict.align_faces(image, dets, size=7)
        assert crops.shape == (0, 7, 7, 3) and crops.dtype == np.uint8
        assert mats.shape == (0, 6) and mats.dtype == np.float32
    crops, _ = predict.align_faces(image, [], size=7, out="f32")
    assert crops.shape == (0, 3, 7, 7) and crops.dtype == np.float32
    with pytest.raises(TypeError):
        predict.align_faces(image.astype(np.float32), [])
    with pytest.raises(ValueError):
        predict.align_faces(image, np.zeros((2, 14), np.float32))
