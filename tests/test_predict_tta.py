"""predict.detect_image_tta: multi-scale / flip detection merged by box voting
on the device, against detect_image (one plain pass, nothing merged) and
against the numpy oracle of tests/_vote_ref.py on the merged rows the call
itself collected."""
import numpy as np
import pytest
import torch

import _vote_ref as V

# weights_init under this seed on this image: at confidence CONF one plain
# pass keeps 118 rows, and the three scales, plain and mirrored, 796 rows that
# vote down to 365, of which 213 have at least 2 votes and the largest 7 (the
# tests assert that there are rows to compare and merged clusters among them)
SEED, IMAGE_SEED, CONF = 1, 1, 0.5


@pytest.fixture(scope="module")
def setup(cuda):
    from nets.retinaface_r import RetinaFace
    from nets.retinaface_training import weights_init
    from utils.config import cfg_mnet
    torch.manual_seed(SEED)
    net = RetinaFace(cfg=cfg_mnet, mode="eval")
    weights_init(net)
    net = net.eval().to(cuda)
    image = np.random.default_rng(IMAGE_SEED).integers(0, 256, (96, 128, 3)).astype(np.uint8)
    return net, cfg_mnet, image


@pytest.mark.gpu
def test_one_plain_pass_without_merging_is_detect_image(cuda, setup):
    from jabd_amd.predict import detect_image, detect_image_tta
    net, cfg, image = setup
    want = detect_image(net, image, (96, 128), cfg, confidence=CONF, nms_iou=0.3,
                        letterbox_image=True, device=cuda)
    got = detect_image_tta(net, image, cfg, scales=(1.0,), flip=False, confidence=CONF,
                           nms_iou=0.3, vote_thres=2.0, device=cuda)
    assert len(want) > 1 and got.shape == want.shape and got.dtype == np.float32
    assert got[:, 4:].tobytes() == want[:, 4:].tobytes()        # order, scores, landmarks
    assert int(V.ulp_diff(got[:, :4], want[:, :4]).max()) <= 1


@pytest.mark.gpu
def test_three_scales_and_flip_against_the_oracle(cuda, setup):
    from jabd_amd import ops
    from jabd_amd.predict import detect_image_tta
    net, cfg, image = setup
    seen = {}

    def hook(merged, offsets):
        seen["merged"], seen["offsets"] = merged.clone(), offsets.clone()
    got = detect_image_tta(net, image, cfg, scales=(0.5, 1.0, 1.5), flip=True, confidence=CONF,
                           device=cuda, _merged_hook=hook)
    offsets = seen["offsets"].cpu().tolist()
    assert len(offsets) == 7 and offsets[0] == 0 and offsets == sorted(offsets)
    assert all(b > a for a, b in zip(offsets, offsets[1:]))       # every pass found rows
    n = offsets[-1]
    merged = seen["merged"].cpu().numpy()
    assert merged.shape[0] >= n
    ref = V.vote(merged[:n], thresh=0.4, offset=1.0, max_out=750)
    print(f"merged rows {n}, result rows {len(ref['seeds'])}, max votes {ref['votes'].max()}, "
          f"margin {ref['margin']:.3e}")
    assert (ref["votes"] >= 2).any()
    # the call's own voting step, with its seeds and votes
    out, n_out, seed, votes = ops.box_vote(seen["merged"][None], 0.4, offset=1.0,
                                           n_valid=seen["offsets"][6:])
    k = int(n_out[0])
    assert k == len(ref["seeds"]) == len(got)
    assert seed[0, :k].cpu().tolist() == ref["seeds"].tolist()
    assert votes[0, :k].cpu().tolist() == ref["votes"].tolist()
    assert got.tobytes() == out[0, :k].cpu().numpy().tobytes()
    assert got[:, 4:].tobytes() == ref["rows"][:, 4:].tobytes()
    assert int(V.ulp_diff(got[:, :4], ref["rows"][:, :4]).max()) <= 1
    # image pixels: the voted boxes of a 96 x 128 image lie around it
    assert np.isfinite(got).all() and got[:, 2].max() > 16 and got[:, :4].max() < 1000


@pytest.mark.gpu
def test_the_call_synchronises_once(cuda, setup, monkeypatch):
    """From the third call with one image size on (the first runs eagerly, the
    second captures the graphs), the only host synchronisation is the read of
    n_out: one Tensor.item, no Tensor.cpu / tolist / nonzero, no stream,
    event or device synchronize."""
    from jabd_amd.predict import detect_image_tta
    net, cfg, image = setup
    kw = dict(scales=(1.0, 1.5), flip=True, confidence=CONF, device=cuda)
    detect_image_tta(net, image, cfg, **kw)
    second = detect_image_tta(net, image, cfg, **kw)
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
    third = detect_image_tta(net, image, cfg, **kw)
    monkeypatch.undo()
    assert calls == ["item"], calls
    assert len(third) > 0 and third.tobytes() == second.tobytes()
