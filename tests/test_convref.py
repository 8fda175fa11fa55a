"""CPU tests of the operator-level conv check itself (tests/_convref.py) and
of the launch witness exports: the derived bound passes a correct fp32 conv
(torch's own) on every case of tests/test_conv_dispatch.py and fails each of
three seeded kernel bugs, so it is neither too tight nor too loose."""
import pytest
import torch
import torch.nn.functional as tF

import _convref as R


def test_launch_log_reset_then_count_is_zero():
    from jabd_amd import _lib
    h = _lib.lib()
    assert h.jabd_launch_log_reset() == 0
    assert h.jabd_launch_log_count() == 0
    assert _lib.launch_log() == []


def test_launch_log_out_of_range_is_null():
    from jabd_amd import _lib
    h = _lib.lib()
    h.jabd_launch_log_reset()
    for i in (0, 1, -1, 63, 64, 2 ** 31 - 1):
        assert h.jabd_launch_log_name(i) is None, i
        assert h.jabd_launch_log_tag(i) == 0, i


def _fp32(t):
    """The case in torch's fp32 CPU ops (separate gate multiply, convs, adds)."""
    x = t["x"] * t["gate"][:, :, None, None] if t["gate"] is not None else t["x"]
    z = tF.conv2d(x, t["w"], None, t["stride"], t["pad"])
    if t["x2"] is not None:
        v = R._x2_at(t["x2"], t["x2_stride"], z.shape[2], z.shape[3])
        z = z + tF.conv2d(v, t["w2"][:, :, None, None])
    if t["bias"] is not None:
        z = z + t["bias"][None, :, None, None]
    if t["res"] is not None:
        z = z + t["res"]
    if t["act"] == "relu":
        return tF.relu(z)
    if t["act"] == "leaky":
        return tF.leaky_relu(z, t["slope"])
    if t["act"] == "hswish":
        return tF.hardswish(z)
    return z


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_bound_passes_fp32_and_fails_mutations(name):
    t = R.tensors(name)
    z, y, E = R.reference(name)
    act, slope = t["act"], t["slope"]
    ok, worst = R.check(_fp32(t), y, E, act)
    assert ok, f"torch fp32 conv outside the bound: {worst:.3f} x tolerance"

    # (1) one product term dropped at one output: the last image's output with
    # the largest pre-activation value (so the activation passes it on with
    # slope >= 1), the term of median magnitude among its non-zero terms
    b = z.shape[0] - 1
    n, oh, ow = [int(v) for v in
                 torch.unravel_index(torch.argmax(z[b]), z.shape[1:])]
    terms = R.terms_at(t, b, n, oh, ow)
    extra = (float(t["bias"][n]) if t["bias"] is not None else 0.0) + \
        (float(t["res"][b, n, oh, ow]) if t["res"] is not None else 0.0)
    assert abs(float(terms.sum()) + extra - float(z[b, n, oh, ow])) < 1e-9   # the terms are z's
    nz = terms[terms != 0].abs().sort().values
    drop = float(nz[len(nz) // 2])
    mut = y.clone()
    mut[b, n, oh, ow] = R.act64(z[b, n, oh, ow] - drop, act, slope)
    assert not R.check(mut, y, E, act)[0], "a dropped product term passes the bound"

    # (2) the gate shifted by 4 channels (gated cases)
    if t["gate"] is not None:
        _, mut, _ = R.conv_ref64(t["x"], t["w"], t["bias"], t["stride"], t["pad"],
                                 torch.roll(t["gate"], 4, 1), t["x2"], t["w2"], t["x2_stride"],
                                 t["res"], act, slope)
        assert not R.check(mut, y, E, act)[0], "a gate shifted by 4 channels passes the bound"

    # (3) the last pixel of the last image left unwritten: NaN in a NaN-filled
    # output (what test_conv_dispatch uses), 0 in a zeroed one
    for fill in (float("nan"), 0.0):
        mut = y.clone()
        mut[-1, :, -1, -1] = fill
        assert not R.check(mut, y, E, act)[0], f"an unwritten pixel ({fill}) passes the bound"
