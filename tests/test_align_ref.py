"""tests/_align_ref.py pinned on the CPU: the closed-form fit against an SVD
Umeyama, the sampling rules against cases whose result is known exactly, and
the whole restatement against a plain float64 warp.  The device is compared
with the restatement by bytes in tests/test_align_faces.py."""
import numpy as np
import pytest

import _align_ref as R

# a template whose coordinates and means are small dyadic numbers: every step
# of a fit to an integer-shifted, doubled or point-mirrored copy is exact
T8 = np.array([[2, 3], [6, 3], [4, 5], [2.5, 7], [5.5, 7]], np.float32)


def _image(ih, iw, seed=0, step=1):
    return (np.random.default_rng(seed).integers(0, 256 // step, (ih, iw, 3)) * step).astype(
        np.uint8)


_similar = R.similar


def _crop(image, lm, size, template, **kw):
    pool = image.reshape(-1)
    rows = np.zeros((1, 15), np.float32)
    rows[0, 5:] = np.asarray(lm, np.float32).reshape(10)
    crops, mats, ss = R.align_faces(pool, [[0, image.shape[0], image.shape[1]]], rows, [0, 1],
                                    size, template, **kw)
    return crops[0], mats[0], ss[0]


def test_closed_form_is_the_svd_umeyama():
    rng = np.random.default_rng(3)
    q = R.default_template(112)
    worst = 0.0
    for k in range(2000):
        scale = float(np.exp(rng.uniform(np.log(0.05), np.log(8.0))))
        lm = _similar(q, scale, rng.uniform(0, 2 * np.pi), rng.uniform(-4000, 4000, 2), rng, 3.0)
        if k % 4 == 0:                                   # a mirrored landmark set
            lm[:, 0] = np.float32(500.0) - lm[:, 0]
        f = R.fit(lm.reshape(10), q)
        assert f.s > 0
        det = 1.0 / (f.ia * f.ia + f.ib * f.ib)          # a*a + b*b
        a, b = f.ia * det, f.ib * det
        M = R.umeyama_svd(lm.astype(np.float64), q.astype(np.float64))
        c = np.hypot(M[0, 0], M[1, 0])
        lin = max(abs(a - M[0, 0]), abs(a - M[1, 1]), abs(b - M[1, 0]), abs(-b - M[0, 1])) / c
        tr = max(abs(f.tx - M[0, 2]), abs(f.ty - M[1, 2])) / max(abs(M[0, 2]), abs(M[1, 2]), 112.0)
        worst = max(worst, lin, tr)
        assert np.allclose(f.m, M.reshape(6), rtol=1e-6, atol=1e-4)
    print(f"worst relative difference {worst:.3g}")
    assert worst <= 1e-12


@pytest.mark.parametrize("template", [T8, None])
def test_an_integer_shift_is_a_pixel_copy(template):
    """With the default template the shifted landmarks round in float32, so the
    fitted scale is 1 only to ~1e-7: the sub-sample rule is switched off there,
    and the copy is exact after the rounding to uint8."""
    img = _image(21, 30, 1)
    q = R.default_template(8) if template is None else template
    crop, m, s = _crop(img, q + np.float32([9, 5]), 8, template, antialias=template is not None)
    assert s == 1
    assert np.array_equal(crop, img[5:13, 9:17])
    if template is not None:                             # exact all the way
        assert m.tolist() == [1.0, -0.0, -9.0, 0.0, 1.0, -5.0]


def test_a_half_turn_is_the_flipped_window():
    img = _image(21, 30, 2)
    crop, m, s = _crop(img, np.float32([20, 16]) - T8, 8, T8)
    assert s == 1 and m.tolist() == [-1.0, -0.0, 20.0, 0.0, -1.0, 16.0]
    # crop[y, x] = img[16 - y, 20 - x]
    assert np.array_equal(crop, img[9:17, 13:21][::-1, ::-1])


def test_a_2x_downscale_on_pixel_centres_is_the_box_mean():
    img = _image(24, 24, 3, step=4)                      # every 2 x 2 mean is an integer
    crop, m, s = _crop(img, T8 * np.float32(2) + np.float32(0.5), 8, T8)
    assert s == 2 and m.tolist() == [0.5, -0.0, -0.25, 0.0, 0.5, -0.25]
    box = img[:16, :16].astype(np.float64).reshape(8, 2, 8, 2, 3).mean((1, 3))
    assert np.array_equal(crop, box.astype(np.uint8))
    # a 4x downscale takes 4 x 4 sub-samples, which land on the 16 pixel centres too
    img = _image(40, 40, 3, step=16)
    crop, m, s = _crop(img, T8 * np.float32(4) + np.float32(1.5), 8, T8)
    assert s == 4 and m.tolist() == [0.25, -0.0, -0.375, 0.0, 0.25, -0.375]
    box = img[:32, :32].astype(np.float64).reshape(8, 4, 8, 4, 3).mean((1, 3))
    assert np.array_equal(crop, box.astype(np.uint8))
    # one sample per pixel sees only the four pixels in the middle of each block
    plain, _, s1 = _crop(img, T8 * np.float32(4) + np.float32(1.5), 8, T8, antialias=False)
    assert s1 == 1 and not np.array_equal(plain, crop)


def test_one_sample_crops_are_within_a_level_of_a_float64_warp():
    rng = np.random.default_rng(5)
    img = _image(40, 52, 4)
    q = R.default_template(16)
    for k in range(40):
        scale = float(np.exp(rng.uniform(np.log(0.2), np.log(4.0))))
        lm = _similar(q, scale, rng.uniform(0, 2 * np.pi), rng.uniform(15, 30, 2), rng, 0.4, (8, 8))
        crop, _, s = _crop(img, lm, 16, None, antialias=False)
        assert s == 1
        M = R.umeyama_svd(lm.astype(np.float64), q.astype(np.float64))
        want = R.warp_f64(img, M, 16)
        assert np.abs(crop.astype(np.float64) - want).max() <= 0.5 + 1e-3   # one level
        assert crop.max() > 0


def test_sub_sample_counts():
    q = R.default_template(16)
    got = {}
    for scale in (2.0, 1.1, 0.7, 0.51, 0.45, 0.34, 0.3, 0.26, 0.2, 0.01):
        lm = _similar(q, scale, 0.3, (50, 40))
        got[scale] = R.fit(lm.reshape(10), q).s
        assert R.fit(lm.reshape(10), q, antialias=False).s == 1
    assert got == {2.0: 1, 1.1: 1, 0.7: 2, 0.51: 2, 0.45: 3, 0.34: 3, 0.3: 4, 0.26: 4, 0.2: 4,
                   0.01: 4}


def test_taps_outside_the_image_read_zero():
    img = np.full((12, 10, 3), 200, np.uint8)
    crop, _, s = _crop(img, T8 + np.float32([-3, 8]), 8, T8)          # window x -3.., y 8..
    assert s == 1
    want = np.zeros((8, 8, 3), np.uint8)
    want[:4, 3:] = 200                                   # rows 8..11, columns 0..4
    assert np.array_equal(crop, want)
    # half a pixel in: the border pixel blends with the zero outside
    crop, _, _ = _crop(img, T8 + np.float32([-3.5, 8]), 8, T8)
    assert np.array_equal(crop[0, :, 0], [0, 0, 0, 100, 200, 200, 200, 200])
    # windows nowhere near the image
    for shift in ([500, 500], [1e6, -1e6]):
        crop, m, s = _crop(img, T8 + np.float32(shift), 8, T8)
        assert s == 1 and not crop.any()
    # source coordinates far beyond any int: still 0, no overflow on the way
    crop, m, s = _crop(img, T8 * np.float32(1e30), 8, T8)
    assert s == 4 and not crop.any() and 0.99e-30 < m[0] < 1.01e-30


def test_invalid_faces_give_a_zero_crop_and_matrix():
    img = _image(12, 10, 6)
    ok = T8 + np.float32([1, 2])
    nan = ok.copy()
    nan[2, 1] = np.nan
    inf = ok.copy()
    inf[0, 0] = np.inf
    same = np.tile(np.float32([4, 5]), (5, 1))           # S == 0
    # A == B == 0 with S > 0: landmarks that are no image of the template at all
    perp = np.float32([[0, 0], [0, 0], [0, 0], [1, 0], [-1, 0]])
    tmpl = np.float32([[1, 1], [-1, -1], [0, 0], [0, 5], [0, 5]])
    for lm, t in ((nan, T8), (inf, T8), (same, T8), (perp, tmpl)):
        crop, m, s = _crop(img, lm, 8, t)
        assert s == 0 and not crop.any() and m.tobytes() == bytes(24)
        f32, _, _ = _crop(img, lm, 8, t, out="f32", mean=(1.0, 2.0, 4.0), std=2.0)
        assert np.array_equal(f32, np.broadcast_to(np.float32([-0.5, -1, -2])[:, None, None],
                                                   (3, 8, 8)))
    # empty slots: no side, a negative side, bytes beyond the pool, a negative offset
    rows = np.zeros((1, 15), np.float32)
    rows[0, 5:] = ok.reshape(10)
    pool = img.reshape(-1)
    for desc in ([0, 0, 10], [0, 12, -1], [1, 12, 10], [-1, 12, 10], [0, 13, 10]):
        crops, mats, ss = R.align_faces(pool, [desc], rows, [0, 1], 8, T8)
        assert ss == [0] and not crops.any() and not mats.any()
    crops, mats, ss = R.align_faces(pool, [[0, 12, 10]], rows, [0, 1], 8, T8)
    assert ss == [1] and crops.any() and mats.any()


def test_float_output_layout_and_what_a_call_leaves_alone():
    img = _image(21, 30, 7)
    lm = T8 + np.float32([9, 5])
    f32, _, _ = _crop(img, lm, 8, T8, out="f32", mean=(10.0, 20.0, 30.0), std=(2.0, 4.0, 8.0),
                      bgr=True)
    win = img[5:13, 9:17].astype(np.float32)
    for k in range(3):
        want = (win[..., 2 - k] - np.float32((10, 20, 30)[k])) / np.float32((2, 4, 8)[k])
        assert np.array_equal(f32[k], want)
    # faces beyond the count keep what the buffers held; cap cuts the count
    rows = np.zeros((3, 15), np.float32)
    rows[:, 5:] = lm.reshape(10)
    before = np.full((3, 8, 8, 3), 7, np.uint8)
    crops, mats, ss = R.align_faces(img.reshape(-1), [[0, 21, 30]], rows, [0, 2], 8, T8,
                                    crops=before, matrices=np.full((3, 6), 9, np.float32))
    assert ss == [1, 1] and np.array_equal(crops[2], before[2]) and (mats[2] == 9).all()
    assert np.array_equal(crops[0], img[5:13, 9:17])
    crops, mats, ss = R.align_faces(img.reshape(-1), [[0, 21, 30]], rows, [0, 5], 8, T8)
    assert ss == [1, 1, 1]
