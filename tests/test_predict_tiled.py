"""predict.detect_image_tiled: sliced detection with the on-device tile merge,
against detect_image (one tile, nothing filtered or merged) and against the
numpy oracle of tests/_tile_ref.py fed with the test's own gather -> forward ->
detect outputs in the call's chunking.  Every comparison is of bytes."""
import numpy as np
import pytest
import torch

import _tile_ref as R
import _vote_ref as V

# weights_init under these seeds on these images (see the asserts of each test
# for what the seeds were chosen to give; the figures are printed)
SEED_A, IMAGE_SEED_A = 1, 1
SEED_B, IMAGE_SEED_B = 1, 1
CONF, NMS_IOU = 0.5, 0.3
TILE, OVERLAP, BATCH = (64, 64), 16, 4
MEAN = (104.0, 117.0, 123.0)


def make_net(cuda, seed):
    from nets.retinaface_r import RetinaFace
    from nets.retinaface_training import weights_init
    from utils.config import cfg_mnet
    torch.manual_seed(seed)
    net = RetinaFace(cfg=cfg_mnet, mode="eval")
    weights_init(net)
    return net.eval().to(cuda), cfg_mnet


def make_image(seed, ih, iw):
    return np.random.default_rng(seed).integers(0, 256, (ih, iw, 3)).astype(np.uint8)


_NETS = {}


def _net(cuda, seed):
    if seed not in _NETS:
        _NETS[seed] = make_net(cuda, seed)
    return _NETS[seed]


def one_tile_case(cuda, seed, image_seed):
    """(want, got, margin): detect_image without letterbox on a 64 x 64 image,
    the tiled call with one 64 x 64 tile, and the smallest distance of a kept
    pair's pixel IoU from NMS_IOU."""
    from jabd_amd.predict import detect_image, detect_image_tiled
    net, cfg = _net(cuda, seed)
    image = make_image(image_seed, 64, 64)
    want = detect_image(net, image, (64, 64), cfg, confidence=CONF, nms_iou=NMS_IOU,
                        letterbox_image=False, device=cuda)
    got = detect_image_tiled(net, image, cfg, tile=TILE, overlap=OVERLAP, batch=1,
                             full_pass=False, confidence=CONF, nms_iou=NMS_IOU, device=cuda)
    margin = np.inf
    if len(want) > 1:
        iou = R.iou_pixels(want[:, :4]).astype(np.float64)
        off = ~np.eye(len(want), dtype=bool)
        margin = float(np.abs(iou[off] - NMS_IOU).min())
    return want, got, margin


def tiled_case(cuda, seed, image_seed, merge="nms"):
    """The call on a 96 x 160 image with its hooked merge input, and the oracle
    on the test's own stage outputs.  Returns a dict of everything compared."""
    from jabd_amd import functional as F
    from jabd_amd import ops
    from jabd_amd.predict import detect_image_tiled, tile_plan
    from oracle import prep_ref
    from utils.anchors import Anchors
    net, cfg = _net(cuda, seed)
    image = make_image(image_seed, 96, 160)
    seen = {}

    def hook(merged, offsets):
        seen["merged"], seen["offsets"] = merged.clone(), offsets.clone()
    got = detect_image_tiled(net, image, cfg, tile=TILE, overlap=OVERLAP, batch=BATCH,
                             full_pass=True, merge=merge, confidence=CONF, nms_iou=NMS_IOU,
                             device=cuda, _merged_hook=hook)
    # the oracle's input: the same stages by hand, in the same chunking
    plan = tile_plan(96, 160, TILE, OVERLAP)
    assert len(plan) == 6
    img = torch.from_numpy(image).to(cuda)
    pri = Anchors(cfg, image_size=TILE).get_anchors().to(cuda).float().contiguous()
    A = pri.shape[0]
    merged = np.zeros((7 * A, 15), np.float32)
    offsets = np.zeros(4, np.int64)
    filtered = 0

    def stage(x):
        with torch.no_grad(), F.split_k():
            out = net(x)
        rows, nk = ops.detect(*out, pri, cfg["variance"], CONF, NMS_IOU)
        return rows.cpu().numpy(), nk.cpu().numpy()
    for c in range(2):
        valid = plan[c * BATCH:(c + 1) * BATCH]
        padded = np.concatenate([valid, np.repeat(plan[-1:], BATCH - len(valid), 0)])
        x = ops.tile_gather(img, torch.from_numpy(padded).to(cuda), TILE, fill=84.0, mean=MEAN)
        rows, nk = stage(x)
        masks = R.collect(rows, nk, valid, TILE, (96, 160), 1.0, merged, offsets, c)
        filtered += sum(int((~m).sum()) for m in masks)
    rows, nk = stage(ops.letterbox(img.float(), (TILE[1], TILE[0]), mean=MEAN))
    k = int(nk[0])
    full = prep_ref.correct_rows(rows[0, :k], TILE, (96, 160), letterbox=True, to_pixels=True)
    merged[offsets[2]:offsets[2] + k] = full
    offsets[3] = offsets[2] + k
    return {"got": got, "merged": seen["merged"].cpu().numpy(),
            "offsets": seen["offsets"].cpu().tolist(), "ref_merged": merged,
            "ref_offsets": offsets.tolist(), "filtered": filtered, "dev": seen}


@pytest.mark.gpu
def test_one_tile_is_detect_image(cuda):
    want, got, margin = one_tile_case(cuda, SEED_A, IMAGE_SEED_A)
    print(f"one tile: {len(want)} rows, IoU margin {margin:.3e}")
    assert len(want) > 1
    # no kept pair sits where pixel and normalised IoU could round apart
    assert margin > 1e-4
    assert got.dtype == np.float32 and got.shape == want.shape
    assert got.tobytes() == want.tobytes()


@pytest.mark.gpu
def test_several_tiles_against_the_oracle(cuda):
    c = tiled_case(cuda, SEED_B, IMAGE_SEED_B)
    offsets = c["offsets"]
    n = offsets[-1]
    ref, _ = R.merge_nms(c["ref_merged"][:n], NMS_IOU, 750)
    print(f"tiled: offsets {offsets}, filtered {c['filtered']}, result rows {len(ref)}")
    assert len(offsets) == 4 and offsets[0] == 0
    assert all(b > a for a, b in zip(offsets, offsets[1:]))      # every pass found rows
    assert offsets == c["ref_offsets"]
    assert c["merged"].shape[0] >= n
    assert c["merged"][:n].tobytes() == c["ref_merged"][:n].tobytes()
    # the test shows something: the edge filter and the cross-tile merge removed rows
    assert c["filtered"] >= 1 and 0 < len(ref) < n
    got = c["got"]
    assert got.dtype == np.float32 and got.shape == ref.shape
    assert got.tobytes() == ref.tobytes()
    assert (np.diff(got[:, 4]) <= 0).all()                       # descending score
    assert np.isfinite(got).all() and got[:, 2].max() > 64       # image pixels, past one tile


@pytest.mark.gpu
def test_several_tiles_merged_by_voting(cuda):
    from jabd_amd import ops
    c = tiled_case(cuda, SEED_B, IMAGE_SEED_B, merge="vote")
    n = c["offsets"][-1]
    assert c["merged"][:n].tobytes() == c["ref_merged"][:n].tobytes()
    ref = V.vote(c["ref_merged"][:n], thresh=0.4, offset=1.0, max_out=750)
    print(f"vote: merged rows {n}, result rows {len(ref['seeds'])}, "
          f"max votes {ref['votes'].max()}, margin {ref['margin']:.3e}")
    assert (ref["votes"] >= 2).any() and 0 < len(ref["seeds"]) < n
    out, n_out, seed, votes = ops.box_vote(c["dev"]["merged"][None], 0.4, offset=1.0,
                                           n_valid=c["dev"]["offsets"][3:])
    k = int(n_out[0])
    got = c["got"]
    assert k == len(ref["seeds"]) == len(got)
    assert seed[0, :k].cpu().tolist() == ref["seeds"].tolist()
    assert votes[0, :k].cpu().tolist() == ref["votes"].tolist()
    assert got.tobytes() == out[0, :k].cpu().numpy().tobytes()
    assert got.tobytes() == ref["rows"].tobytes()


@pytest.mark.gpu
def test_one_graph_serves_every_image_and_the_call_synchronises_once(cuda, monkeypatch):
    """From the third call on the only host synchronisation is the read of the
    result count: one Tensor.item, no Tensor.cpu / tolist / nonzero, no stream,
    event or device synchronize.  An image of another size runs through the
    graphs the first image captured."""
    from jabd_amd.predict import detect_image_tiled
    net, cfg = _net(cuda, SEED_B)
    image = make_image(IMAGE_SEED_B, 96, 160)
    kw = dict(tile=TILE, overlap=OVERLAP, batch=BATCH, full_pass=True, confidence=CONF,
              nms_iou=NMS_IOU, device=cuda)
    detect_image_tiled(net, image, cfg, **kw)
    second = detect_image_tiled(net, image, cfg, **kw)
    graphs = list(net._jabd_graphs)
    assert any(key[0] == (BATCH, 3) + TILE for key in graphs)
    calls = []

    def count(owner, name):
        real = getattr(owner, name)

        def wrapped(*a, **k):
            calls.append(name)
            return real(*a, **k)
        monkeypatch.setattr(owner, name, wrapped)
    for name in ("item", "cpu", "tolist", "nonzero"):
        count(torch.Tensor, name)
    count(torch.cuda, "synchronize")
    count(torch.cuda.Stream, "synchronize")
    count(torch.cuda.Event, "synchronize")
    third = detect_image_tiled(net, image, cfg, **kw)
    monkeypatch.undo()
    assert calls == ["item"], calls
    assert len(third) > 0 and third.tobytes() == second.tobytes()
    other = detect_image_tiled(net, make_image(7, 64, 128), cfg, **kw)
    assert list(net._jabd_graphs) == graphs                      # no new entry
    assert isinstance(other, (list, np.ndarray))


def test_argument_errors():
    """Raised before any device work (no GPU needed)."""
    from jabd_amd.predict import detect_image_tiled
    from utils.config import cfg_mnet
    image = np.zeros((96, 160, 3), np.uint8)
    for kw in ({"nms_kind": "softnms"}, {"nms_kind": "softernms"}, {"nms_kind": "nope"},
               {"tile": (48, 64)}, {"tile": (64, 0)}, {"overlap": 64}, {"overlap": -1},
               {"overlap": (16, 64)}, {"merge": "soft"}, {"batch": 0},
               {"merge": "vote", "min_votes": 0}):
        with pytest.raises(ValueError):
            detect_image_tiled(None, image, cfg_mnet, **{"tile": (64, 64), "overlap": 16, **kw})
    with pytest.raises(ValueError):
        detect_image_tiled(None, np.zeros((96, 160), np.uint8), cfg_mnet, tile=(64, 64))
