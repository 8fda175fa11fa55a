"""The conv query entry points against the entry points they size.

jabd_conv_workspace_size, jabd_conv1x1_bn_stats_nblk,
jabd_conv_bn_stats_part_floats and jabd_conv_bn_bwd_part_floats each say
whether (and with how large a buffer) a form of the conv serves a layer; the
caller allocates by the answer and then calls jabd_conv2d_nhwc_f32 (with the
split-K workspace), jabd_conv1x1_bn_stats_f32, jabd_conv_bn_stats_f32 or
jabd_conv_bn_bwd_sums_f32.  For every operator case of tests/_convref.py
(CASES, args as tests/test_conv_dispatch.py builds them) and every
data-gradient case of tests/_convgrad_ref.py (DCASES: the plain 1x1 forward
form over the transposed pack and the transposed forms, args as
tests/test_conv_backward_dispatch.py builds them) this asserts

 1. the four answers against the literal table below (split-K workspace and
    nblk as zero / non-zero, the part sizes exactly),
 2. that a non-zero answer means the matching entry point returns JABD_OK and
    leaves the table's launch witness (for the workspace: the split-K launch
    with split-K on, the plain tile kernel with it off), and
 3. that a zero answer means the matching entry point returns JABD_EINVAL
    and launches nothing (a zero workspace: the launch does not split).

The table was written from the dispatch code at the commit before the
classification was gathered into ConvLayer / conv_route (csrc/conv.hip) and
confirmed against that commit's library (JABD_LIB); it pins the queries
through any later reshuffle of the predicates.
"""
import pytest
import torch

import _convgrad_ref as G
import _convref as R
import test_conv_backward_dispatch as BD
import test_conv_dispatch as FD

EINVAL = 1
SPLITK = FD.SPLITK
STREAM_STATS = "conv1x1_stream_stats"
ST32, BB32, M32S = "conv1x1_m32 (BN statistics)", "conv1x1_m32 (BN backward sums)", "conv1x1_m32s"

# case -> (workspace != 0, nblk != 0, jabd_conv_bn_stats_part_floats,
#          jabd_conv_bn_bwd_part_floats, first launch of jabd_conv_bn_stats_f32,
#          first launch of jabd_conv_bn_bwd_sums_f32)
TABLE = {
    "a": (False, False, 0, 0, None, None),
    "a_b3": (False, False, 0, 0, None, None),
    "b_bias_leaky": (False, False, 0, 0, None, None),
    "b_none": (False, False, 1168, 0, ST32, None),
    "b_res": (False, False, 0, 0, None, None),
    "c": (True, False, 0, 0, None, None),
    "d": (False, False, 0, 0, None, None),
    "e160": (False, False, 0, 0, None, None),
    "e192": (False, False, 0, 0, None, None),
    "e224": (False, False, 0, 0, None, None),
    "f": (False, False, 0, 0, None, None),
    "g100_s1": (False, False, 0, 0, None, None),
    "g100_s1_gated": (False, False, 0, 0, None, None),
    "g100_s2": (False, False, 0, 0, None, None),
    "g96_s1": (False, False, 0, 0, None, None),
    "g96_s2": (False, False, 0, 0, None, None),
    "gemm_1x1s2_96_64": (False, False, 0, 0, None, None),
    "gemm_3x3s2_12_10": (False, False, 0, 0, None, None),
    "gemm_3x3s2_48_96": (False, False, 0, 0, None, None),
    "h": (True, False, 0, 0, None, None),
    "i": (True, False, 0, 0, None, None),
    "j": (True, False, 0, 0, None, None),
    "k": (True, False, 0, 0, None, None),
    "l": (True, False, 0, 0, None, None),
    "m": (True, False, 0, 0, None, None),
    "m32_3x3_128_64": (False, False, 0, 1024, None, BB32),
    "m32_3x3_64_64": (False, False, 0, 1280, None, BB32),
    "n": (True, False, 0, 0, None, None),
    "o": (False, False, 0, 0, None, None),
    "o1": (False, False, 0, 0, None, None),
    "o2": (False, False, 0, 0, None, None),
    "o3": (False, False, 0, 0, None, None),
    "o4": (False, False, 0, 0, None, None),
    "p": (False, False, 0, 0, None, None),
    "p_1x1_120_40": (False, False, 1248, 0, ST32, None),
    "p_m32_128_96": (False, False, 1280, 1280, ST32, BB32),
    "p_stream_64_16": (False, True, 896, 896, ST32, BB32),
    "ph_128_128_10x11": (False, False, 0, 0, None, None),
    "ph_128_128_11x10": (False, False, 0, 0, None, None),
    "ph_1x1_512_256": (False, False, 0, 0, None, None),
    "ph_64_64_10x11": (False, False, 0, 0, None, None),
    "ph_64_64_11x10": (False, False, 0, 0, None, None),
    "ph_64_64_h1": (False, False, 0, 0, None, None),
    "q": (False, False, 0, 0, None, None),
    "r": (False, False, 0, 0, None, None),
    "s": (False, False, 0, 0, None, None),
    "t": (False, False, 0, 0, None, None),
    "t3_40_40_64x17": (False, False, 0, 0, None, None),
    "t3_40_40_9x10": (False, False, 0, 0, None, None),
    "u": (False, False, 0, 0, None, None),
    "v": (False, True, 0, 0, None, None),
    "w": (False, False, 0, 0, None, None),
    "x": (False, False, 0, 0, None, None),
    "y": (False, False, 0, 0, None, None),
}


def _cdiv(a, b):
    return -(-a // b)


def _probe(cuda, aref):
    """The four queries of the args behind `aref` and what their entry points
    do, while the caller's buffers are alive.  Returns the table row."""
    from jabd_amd import _lib
    h = _lib.lib()
    a = aref._obj
    M, C = a.B * a.OH * a.OW, a.Cout
    st = BD._stream()
    ws = int(h.jabd_conv_workspace_size(aref))
    nblk = int(h.jabd_conv1x1_bn_stats_nblk(aref))
    nst = int(h.jabd_conv_bn_stats_part_floats(aref))
    nbb = int(h.jabd_conv_bn_bwd_part_floats(aref))
    # room for any form's partial rows, whatever the query said
    room = _cdiv(M, 8) * (C + 64) + 65536
    assert max(nblk * 2 * C, nst, nbb) <= room
    part = torch.empty(room, device=cuda)
    vec = [torch.ones(C + 64, device=cuda) for _ in range(4)]   # mean, invstd, gamma, beta / shift
    bnx = torch.zeros(M, C, device=cuda)                          # the BatchNorm's input rows

    def entry(fn, *args):
        _lib.launch_log_reset()
        status = int(getattr(h, fn)(aref, *args))
        log = _lib.launch_log()
        assert status in (0, EINVAL), f"{fn}: status {status}: {_lib.last_error()}"
        assert (status == 0) == bool(log), f"{fn}: status {status} with launches {log}"
        return status, (log[0] if log else None)

    s1, w1 = entry("jabd_conv1x1_bn_stats_f32", part.data_ptr(), nblk, vec[0].data_ptr(), st)
    s2, w2 = entry("jabd_conv_bn_stats_f32", part.data_ptr(), nst if nst else room,
                   vec[0].data_ptr(), vec[1].data_ptr(), None, None, 0.1, 1e-5, st)
    s3, w3 = entry("jabd_conv_bn_bwd_sums_f32", bnx.data_ptr(), C, vec[0].data_ptr(),
                   vec[1].data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(), 0, 0.0,
                   part.data_ptr(), nbb if nbb else room, st)
    torch.cuda.synchronize()
    _lib.launch_log_reset()
    assert (s1 == 0) == (nblk > 0) and (s2 == 0) == (nst > 0) and (s3 == 0) == (nbb > 0), \
        f"queries (nblk {nblk}, stats {nst}, bn-bwd {nbb}) vs entry statuses ({s1}, {s2}, {s3})"
    assert w1 is None or w1[0] == STREAM_STATS, w1
    return (ws > 0, nblk > 0, nst, nbb, w2 and w2[0], w3 and w3[0])


class _Spy:
    """Probes the args of the first jabd_conv2d_nhwc_f32 that passes through
    mod.call, just before the call itself."""

    def __init__(self, cuda, mod):
        self.cuda, self.mod, self.row = cuda, mod, None

    def __enter__(self):
        self.real = self.mod.call

        def call(fn, *args):
            if fn == "jabd_conv2d_nhwc_f32" and self.row is None:
                self.row = _probe(self.cuda, args[0])
            return self.real(fn, *args)

        self.mod.call = call
        return self

    def __exit__(self, *exc):
        self.mod.call = self.real


def _check_row(name, row):
    print(f'    "{name}": {row!r},')
    assert name in TABLE, f"{name}: no table row"
    assert row == TABLE[name], f"{name}: queries {row}, table {TABLE[name]}"
    assert row[4] in (None, ST32, M32S) and row[5] in (None, BB32, M32S)


def test_table_covers_the_cases():
    assert set(TABLE) == set(R.CASES) | set(G.DCASES)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_forward_queries(cuda, name):
    from jabd_amd import functional as F
    with _Spy(cuda, F) as spy:
        _, log, ws = FD._run(cuda, name, split=True)
    _check_row(name, spy.row)
    names = [n for n, _ in log]
    assert (ws > 0) == spy.row[0] == (SPLITK in names), (ws, log)
    if ws > 0:   # without the workspace the same layer takes the plain tile kernel
        _, log, _ = FD._run(cuda, name, split=False)
        assert [n for n, _ in log] == [FD.M32], log


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(G.DCASES))
def test_data_gradient_queries(cuda, name):
    from jabd_amd import _lib
    t = G.dtensors(name)
    with _Spy(cuda, _lib) as spy:
        _, log = BD.run_dgrad(cuda, t["w"], t["dy"], t["xshape"], t["stride"], t["pad"])
    _check_row(name, spy.row)
    # run_dgrad passes no workspace: never the split launch
    assert SPLITK not in [n for n, _ in log], log
