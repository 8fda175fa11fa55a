"""jabd_tile_gather_f32 through ops.tile_gather: the tile batch of an HWC
image, float32 or uint8, against the numpy restatement of tests/_tile_ref.py,
bytes equal (a pixel or the fill value minus the channel mean: one fp32
subtraction, nothing to tolerate)."""
import numpy as np
import pytest
import torch

import _tile_ref as R

MEAN = (104.0, 117.0, 123.0)


def _image(ih, iw, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, (ih, iw, 3)).astype(np.uint8)
    return (rng.random((ih, iw, 3)) * 255).astype(np.float32)     # fractional values


def _check(cuda, image, origins, tile, **kw):
    from jabd_amd import ops
    origins = np.asarray(origins, np.int32).reshape(-1, 2)
    got = ops.tile_gather(torch.from_numpy(image).to(cuda), torch.from_numpy(origins).to(cuda),
                          tile, **kw)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(origins), 3) + tuple(tile)
    want = R.gather(image, origins, tile, kw.get("fill", 84.0), kw.get("mean", MEAN))
    assert got.cpu().numpy().tobytes() == want.tobytes()
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
def test_plan_tiles_without_padding(cuda, dtype):
    """70 x 100 with 32 x 64 tiles: origins that are no multiples of 4 (the
    wide loads apply to some rows of a tile only), nothing padded."""
    from jabd_amd.predict import tile_plan
    plan = tile_plan(70, 100, tile=(32, 64), overlap=(5, 30))
    assert len(plan) > 2 and (plan % 4 != 0).any()
    assert plan[:, 0].max() + 32 == 70 and plan[:, 1].max() + 64 == 100
    image = _image(70, 100, dtype, 1)
    want = _check(cuda, image, plan, (32, 64))
    # the tiles are the image's own pixels: no fill value anywhere
    t = len(plan) - 1
    y0, x0 = plan[t]
    assert np.array_equal(want[t, 1], image[y0:y0 + 32, x0:x0 + 64, 1].astype(np.float32)
                          - np.float32(117))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
def test_tile_larger_than_the_image_is_padded(cuda, dtype):
    from jabd_amd.predict import tile_plan
    plan = tile_plan(40, 100, tile=(64, 64), overlap=(16, 16))
    assert plan.tolist() == [[0, 0], [0, 36]]
    want = _check(cuda, _image(40, 100, dtype, 2), plan, (64, 64))
    assert (want[:, 0, 40:] == np.float32(84 - 104)).all()        # the bottom rows are fill


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
def test_origins_outside_the_image_pad_all_four_sides(cuda, dtype):
    ih, iw = 37, 53
    image = _image(ih, iw, dtype, 3)
    origins = [(-5, -7), (ih - 3, iw - 3), (-40, 0), (0, iw), (-5, -8)]
    want = _check(cuda, image, origins, (32, 64), fill=7.5, mean=(1.0, 2.0, 3.0))
    assert (want[0, 0, :5] == np.float32(6.5)).all() and (want[0, 0, :, :7] == np.float32(6.5)).all()
    assert (want[1, 2, 3:] == np.float32(4.5)).all() and (want[1, 2, :, 3:] == np.float32(4.5)).all()
    assert (want[2] == np.array([6.5, 5.5, 4.5], np.float32)[:, None, None]).all()   # all outside
    # a tile that covers the whole image, with all four sides padded
    _check(cuda, image, [(-9, -6)], (64, 64))
    # a tile width that is no multiple of 4: the one-pixel form
    _check(cuda, image, [(-2, -3), (20, 30)], (9, 30))


@pytest.mark.gpu
def test_no_tiles_is_a_no_op(cuda):
    from jabd_amd import _lib, ops
    image = torch.from_numpy(_image(16, 16, np.uint8, 4)).to(cuda)
    _lib.launch_log_reset()
    got = ops.tile_gather(image, torch.empty((0, 2), dtype=torch.int32, device=cuda), (32, 32))
    assert tuple(got.shape) == (0, 3, 32, 32)
    assert _lib.launch_log() == []                               # nothing was launched
    org = torch.tensor([[0, 0], [-4, 4]], dtype=torch.int32, device=cuda)
    ops.tile_gather(image, org, (32, 32))
    assert _lib.launch_log() == [("tile_gather", 4)]
    ops.tile_gather(image, org, (32, 30))
    assert _lib.launch_log()[-1] == ("tile_gather", 1)           # the one-pixel form


@pytest.mark.gpu
def test_argument_errors(cuda):
    from jabd_amd import ops
    image = torch.zeros((8, 8, 3), device=cuda)
    org = torch.zeros((1, 2), dtype=torch.int32, device=cuda)
    with pytest.raises(TypeError):
        ops.tile_gather(image.double(), org, (32, 32))
    with pytest.raises(TypeError):
        ops.tile_gather(image, org.long(), (32, 32))
    with pytest.raises(ValueError):
        ops.tile_gather(image[:, :, :2], org, (32, 32))
    with pytest.raises(ValueError):
        ops.tile_gather(image, org.reshape(2), (32, 32))
    with pytest.raises(ValueError):
        ops.tile_gather(image, org, (0, 32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tile_gather(image.cpu(), org, (32, 32))
