"""CPU tests of the conv-backward check itself (tests/_convgrad_ref.py): the
derived bounds pass a correct fp32 weight / data gradient (torch's own) on
every case of tests/test_conv_backward_dispatch.py and fail each seeded kernel
bug (a dropped pixel, a pixel counted twice, a tap read one column off, the
gate of the wrong image, a dropped data-gradient term), so they are neither too
tight nor too loose."""
import pytest
import torch
from torch.nn.grad import conv2d_input, conv2d_weight

import _convgrad_ref as G
from _convref import check


def _outside(mut, ref, E):
    return not check(mut, ref, E, "none")[0]


@pytest.mark.parametrize("name", sorted(G.WCASES))
def test_wgrad_bound_passes_fp32_and_fails_mutations(name):
    t = G.wtensors(name)
    x, dy, gate, ws, s, p = t["x"], t["dy"], t["gate"], t["wshape"], t["stride"], t["pad"]
    ref, E = G.wreference(name)
    ok, worst = check(conv2d_weight(G.gated(x, gate), ws, dy, s, p), ref, E, "none")
    print(f"{name}: torch fp32 at {worst:.4f} x tolerance")
    assert ok, f"torch fp32 conv2d_weight outside the bound: {worst:.3f} x tolerance"

    d = torch.float64
    xs, g = G.gated(x.to(d), gate), dy.to(d)
    B, _, OH, OW = dy.shape
    # (1) one dy pixel dropped, (2) that pixel counted twice: the middle pixel
    # of the last image
    cut = g.clone()
    cut[B - 1, :, OH // 2, OW // 2] = 0
    dropped = conv2d_weight(xs, ws, cut, s, p)
    assert _outside(dropped, ref, E), "a dropped dy pixel passes the bound"
    assert _outside(2 * ref - dropped, ref, E), "a pixel counted twice passes the bound"

    # (3) the centre tap read at iw + 1 (zero past the right edge); the centre,
    # because on a 1 x 3 input the outer taps of a 7x7 only ever see padding
    shifted = torch.zeros_like(xs)
    shifted[..., :-1] = xs[..., 1:]
    c = ws[2] // 2
    mut = ref.clone()
    mut[:, :, c, c] = conv2d_weight(shifted, ws, g, s, p)[:, :, c, c]
    assert _outside(mut, ref, E), "a tap read at iw + 1 passes the bound"

    # (4) the gate of image b applied to image b + 1
    if gate is not None:
        mut = conv2d_weight(G.gated(x.to(d), torch.roll(gate, 1, 0)), ws, g, s, p)
        assert _outside(mut, ref, E), "the gate of the previous image passes the bound"


@pytest.mark.parametrize("name", sorted(G.DCASES))
def test_dgrad_bound_passes_fp32_and_fails_mutations(name):
    t = G.dtensors(name)
    w, dy, xshape, s, p = t["w"], t["dy"], t["xshape"], t["stride"], t["pad"]
    ref, E = G.dreference(name)
    ok, worst = check(conv2d_input(xshape, w, dy, s, p), ref, E, "none")
    print(f"{name}: torch fp32 at {worst:.4f} x tolerance")
    assert ok, f"torch fp32 conv2d_input outside the bound: {worst:.3f} x tolerance"

    # one (n, kh, kw) term dropped at the last image's dx of largest magnitude:
    # the term of median magnitude among that output's terms
    d = torch.float64
    b = xshape[0] - 1
    ci, ih, iw = [int(v) for v in torch.unravel_index(torch.argmax(ref[b].abs()), ref.shape[1:])]
    terms = []
    for kh in range(w.shape[2]):
        for kw in range(w.shape[3]):
            oh, ow = ih + p - kh, iw + p - kw
            if oh % s or ow % s or not (0 <= oh // s < dy.shape[2] and 0 <= ow // s < dy.shape[3]):
                continue
            terms.append(w[:, ci, kh, kw].to(d) * dy[b, :, oh // s, ow // s].to(d))
    terms = torch.cat(terms)
    assert abs(float(terms.sum()) - float(ref[b, ci, ih, iw])) < 1e-9   # the terms are dx's
    nz = terms[terms != 0].abs().sort().values
    mut = ref.clone()
    mut[b, ci, ih, iw] -= float(nz[len(nz) // 2])
    assert _outside(mut, ref, E), "a dropped product term passes the bound"

    # an unwritten pixel: NaN in a NaN-filled dx (what the GPU test uses), 0 in a zeroed one
    for fill in (float("nan"), 0.0):
        mut = ref.clone()
        mut[b, :, ih, iw] = fill
        assert _outside(mut, ref, E), f"an unwritten pixel ({fill}) passes the bound"
