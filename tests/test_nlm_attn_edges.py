"""Parity of the two NLM attention families at the edges the model tests never
reach (references, inputs and case tables: tests/_attn_ref.py).

General-width core (csrc/nlm_attn.hip), called through the C ABI: every width
8..64, S in {1, 2, 3, 7, 33, 110, 160, 204, 205, 256}, ragged P, a peaked and
a monotone softmax (the online rescale on every bin), the dynamic-LDS path
over 64 KiB, lse == NULL and attn_check's rejections; ctx, lse, dq, pm, dsm,
and dK / dV after jabd_nlm_attn_dkv_f32, against fp64.  Every output buffer
carries a 64-float tail: the body is prefilled with NaN and must come back
finite, the tail with a sentinel and must come back bit-identical.

ch = 4 family (head.hip nlm_kv/pool/apply, nlm_train.hip nlm_bwd_*) through
NlmFn.apply and functional.nlm_fused(save=False): S < 4 (the "lane with no
bins" branch), S off the backward's 8-bin chunk, pixel counts at the 64 / 128 /
256 workgroup boundaries, non-square maps, C = 4 / 20 / 256, the backward's
LDS over 64 KiB (C = 1024), the standalone form, a peaked softmax, a strided
source, and the JABD_NLM_PX=1 / JABD_NLM_BWD_QUAD=1 forms in a fresh child
process (both are read once per process).

CPU self-checks (not marked gpu) prove inputs and bars sound first: for every
case an honest fp32 evaluation (torch on the CPU, and the numpy emulation of
the kernel's algorithm) stays within a quarter of the bar, the builders do what
their names say, the LDS byte counts are the kernels', and each planted defect
of the emulation is caught:
  no_rescale (accumulator not rescaled on a new max): rescale-monotone-ch40-S110
              and -ch64-S33 (ctx, dq, dsm, dk)
  lse_no_log (lse = m): lse, pm, dsm, dq, dk, dv of every peaked case with S > 1
              (named: width-peaked-ch40-S7, edges-peaked-ch40-S110-P257)
  short_loop (bin loop to S & ~3): S = 1, 2, 3 (nothing written), S = 7 and
              S = 110 (edges / width cases at ch = 40)

Worst error observed on the MI355X per group, next to its bar (no case is
within 2x of its bar):
  core, width sweep     ctx 2.6e-7 / 1e-5    lse 4.2e-7 / 1.43e-6 (normal, M = 3)
                        backward 1.2e-6 / 1.43e-5
  core, S / P edges     ctx 7.8e-7 / 1e-5    lse 1.4e-6 / 1.43e-5   backward 1.9e-6 / 1.43e-5
  core, online rescale  ctx 1.0e-6 / 1e-5    lse 1.2e-6 / 1.43e-5   backward 1.6e-6 / 1.43e-5
  core, LDS boundary    ctx 1.1e-6 / 1e-5    lse 2.0e-6 / 1.43e-5   backward 3.0e-6 / 1.43e-5
  ch = 4 (bar 1e-4)     small S 7.5e-7   pixel boundaries 1.1e-6   channel loops 1.3e-6
                        C = 1024 2.8e-6   standalone 3.8e-7   peaked 3.7e-6
  ch = 4 A/B children   JABD_NLM_PX=1 3.7e-6   JABD_NLM_BWD_QUAD=1 3.3e-6
"""
import os
import subprocess
import sys

import pytest
import torch

import _attn_ref as A
from _util import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jabd-joint-attention-based-detector-for-small-face-detection_amd", "csrc")
TAIL = 64
SENTINEL = 12345.6789

def _case(group, **kw):
    """The one case of CORE_CASES with these fields."""
    hits = [c for c in A.CORE_CASES if c.group == group
            and all(getattr(c, k) == v for k, v in kw.items())]
    assert len(hits) == 1, (group, kw, hits)
    return hits[0]


# --------------------------------------------------------------- CPU self-checks
@pytest.mark.parametrize("case", A.CORE_CASES + (A.CORE_LSE_NULL_CASE,), ids=A.core_id)
def test_core_case_is_benign_in_fp32(case):
    """Honest fp32 (torch CPU, and the emulation of the kernel's algorithm)
    stays within a quarter of every bar: a larger device error is the kernel's."""
    inp, ref = A.core_case_data(case)
    emu = A.core_emulate(inp)
    lg = inp["q"].double() @ inp["k"].double().transpose(1, 2)
    assert bool((emu["logits"].double() == lg).all()), "logits not exact in fp32"
    for what, got in (("torch-fp32", A.core_ref(inp, torch.float32)), ("emulation", emu)):
        for n, (e, bar) in A.core_errors(got, ref, inp).items():
            assert e <= bar / 4, f"{what} {n}: {e:.2e} > bar/4 = {bar / 4:.2e}"


def test_core_builders_do_what_they_say():
    kinds = set()
    for case in A.CORE_CASES:
        inp, ref = A.core_case_data(case)
        kinds.add(case.kind)
        target = A.NORMAL_LOGIT if case.kind == "normal" else A.PEAKED_LOGIT
        assert abs(ref["M"] - target) <= 0.02 * target, (A.core_id(case), ref["M"])
        if case.kind == "normal":
            assert ref["top"] <= 0.3, (A.core_id(case), ref["top"])
        elif case.kind == "peaked":
            assert ref["top"] >= 0.5, (A.core_id(case), ref["top"])
        else:
            resc = A.core_emulate(inp)["resc"]
            h = (case.P + 1) // 2
            assert resc[:, :h, :].all(), "first half: a new max on every bin"
            assert resc[:, h:, 0].all() and not resc[:, h:, 1:].any(), \
                "second half: a new max on the first bin only"
    assert kinds == {"normal", "peaked", "monotone"}


def _over(case, defect):
    """Names of the quantities whose bar the emulation with `defect` exceeds."""
    inp, ref = A.core_case_data(case)
    errs = A.core_errors(A.core_emulate(inp, defect=defect), ref, inp)
    return {n for n, (e, bar) in errs.items() if not e <= bar}


def test_planted_defects_are_caught():
    for case in (_case("rescale", S=110), _case("rescale", S=33)):
        assert {"ctx", "dq", "dsm", "dk"} <= _over(case, "no_rescale"), A.core_id(case)
    for case in A.CORE_CASES:
        if case.kind == "peaked" and case.S > 1:
            over = _over(case, "lse_no_log")
            assert {"lse", "pm", "dsm", "dq", "dk", "dv"} <= over, (A.core_id(case), over)
    for case in (_case("width", kind="peaked", ch=40), _case("edges", S=110, P=257)):
        assert "lse" in _over(case, "lse_no_log")
    for case in ([_case("edges", S=S, P=257) for S in (1, 2, 3, 110)]
                 + [_case("width", kind="peaked", ch=40), _case("width", kind="normal", ch=40)]):
        over = _over(case, "short_loop")
        assert {"ctx", "pm", "dv"} <= over, (A.core_id(case), over)
    assert not _over(_case("rescale", S=110), None)  # the honest emulation trips nothing


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return " ".join(f.read().split())


def test_tables_match_the_kernels_lds_formulas():
    """The byte counts the boundary cases rest on are the kernels' own: a
    change of the LDS layout fails here instead of moving the boundary away
    from the cases unnoticed."""
    attn = _src("nlm_attn.hip")
    assert attn.count("const size_t sm = (size_t)S * ch * 8;") == 2
    assert attn.count("if (sm > 65536)") == 2
    assert "JABD_REQUIRE((size_t)S * ch * 8 <= 160 * 1024" in attn
    assert "X(8) X(12) X(16) X(20) X(24) X(28) X(32) X(36) X(40) X(44) X(48) X(52) X(56) X(60) X(64)" in attn
    lds = {(c.ch, c.S): A.core_lds_bytes(c.S, c.ch) for c in A.CORE_CASES if c.group == "lds"}
    assert lds == {(40, 204): 65280, (40, 205): 65600, (64, 160): 81920, (64, 256): 131072}
    assert lds[(40, 204)] <= A.CORE_LDS_PLAIN < lds[(40, 205)]
    assert all(A.core_lds_bytes(c.S, c.ch) <= A.CORE_LDS_MAX
               for c in A.CORE_CASES + (A.CORE_LSE_NULL_CASE,))
    ch, S, _, _ = A.CORE_REJECT["lds"]
    assert A.core_lds_bytes(S, ch) > A.CORE_LDS_MAX >= A.core_lds_bytes(S - 1, ch)
    train = _src("nlm_train.hip")
    for text in ("constexpr int kNb = 8;", "constexpr int kNg = 256 / kNb;",
                 "constexpr int kNbP = 256 + 1;",
                 "const size_t smem = (2 * (size_t)C * CH + 2 * 256 * CH + 2 * (size_t)kNb * kNbP + "
                 "kNg * (size_t)kNb * 2 * CH) * 4;",
                 "if (smem > 64 * 1024)",
                 "const size_t smem = (2 * (size_t)S * CH + 2 * (size_t)C * CH + 4 * (size_t)S * 2 * CH) * 4;",
                 "JABD_REQUIRE(smem <= 64 * 1024, \"nlm_bwd_attn: LDS %zu > 64KiB\", smem);"):
        assert text in train, text
    big = [c for c in A.NLM4_CASES if c.group == "lds"]
    assert len(big) == 1 and big[0].C == 1024
    assert A.nlm4_bwd_lds_bytes(1024, A.nlm4_S(big[0])) == 65600 > 64 * 1024
    assert all(A.nlm4_bwd_lds_bytes(c.C, A.nlm4_S(c)) <= 64 * 1024
               for c in A.NLM4_CASES if c.C != 1024)
    # the lane-quad form holds every table case (C = 1024 at S = 5 takes 33 568 B);
    # its limit is met by NLM4_QUAD_OVER
    assert all(A.nlm4_bwd_lds_bytes(c.C, A.nlm4_S(c), quad=True) <= 64 * 1024
               for c in A.NLM4_CASES)
    assert A.nlm4_bwd_lds_bytes(A.NLM4_QUAD_OVER.C, A.nlm4_S(A.NLM4_QUAD_OVER), quad=True) == 65920


def test_nlm4_table_covers_its_edges():
    by = {}
    for c in A.NLM4_CASES:
        by.setdefault(c.group, []).append(c)
    assert sorted(A.nlm4_S(c) for c in by["smallS"]) == [1, 2, 3, 5, 9]
    assert sorted(c.h * c.w for c in by["pixels"]) == [1, 129, 192, 255, 256, 257]
    assert any(c.h != c.w for c in by["pixels"])
    assert sorted(c.C for c in by["channels"]) == [4, 20, 40, 256]
    assert all(not c.lateral and (c.hs, c.ws) == (c.h, c.w) for c in by["standalone"])
    assert len(by["peaked"]) == 3
    assert len(set(A.nlm4_id(c) for c in A.NLM4_CASES)) == len(A.NLM4_CASES)


@pytest.mark.parametrize("case", A.NLM4_CASES, ids=A.nlm4_id)
def test_nlm4_case_is_benign_in_fp32(case):
    """The oracle in torch-CPU fp32, and the fp32 emulation of the attention
    stage, stay within a quarter of the 1e-4 bar against fp64."""
    inp, ref = A.nlm4_case_data(case)
    for n, (e, bar) in A.nlm4_errors(case, A.nlm4_oracle(case, inp, torch.float32), ref).items():
        assert e <= bar / 4, f"torch-fp32 {n}: {e:.2e}"
    att = A.nlm4_attention_inputs(case, inp)
    a64, emu = A.core_ref(att), A.core_emulate(att)
    assert rel_err(emu["ctx"], a64["ctx"]) <= A.NLM4_TOL / 4
    _, _, M, top = A.nlm4_stats(case, inp)
    if case.peaked:
        assert abs(M - 30.0) <= 0.3 and top >= 0.5, (M, top)
        if A.nlm4_S(case) > 1:
            assert rel_err(emu["dq"], a64["dq"]) <= A.NLM4_TOL / 4


# ------------------------------------------------------------------- GPU: the core
def _tailed(n, dev):
    """n NaN floats followed by TAIL sentinel floats."""
    buf = torch.empty(n + TAIL, dtype=torch.float32, device=dev)
    buf[:n] = float("nan")
    buf[n:] = SENTINEL
    return buf


def _tail_intact(buf, n):
    want = torch.full((TAIL,), SENTINEL, dtype=torch.float32, device=buf.device)
    return bool(torch.equal(buf[n:].view(torch.int32), want.view(torch.int32)))


def _core_gpu(inp, dev, with_lse=True):
    """Forward, backward and the dkv reduction, as NlmAttnFn runs them, on
    tailed NaN-prefilled outputs.  Returns the outputs (bodies) and checks
    finiteness and tails."""
    from jabd_amd._lib import call, lib
    q, k, v, d = (inp[n].to(dev).contiguous() for n in ("q", "k", "v", "dctx"))
    B, P, ch = q.shape
    S = k.shape[1]
    shapes = {"ctx": (B, P, ch), "lse": (B, P), "dq": (B, P, ch), "pm": (B, S, P),
              "dsm": (B, S, P), "dk": (B, S, ch), "dv": (B, S, ch)}
    numel = {n: int(torch.Size(s).numel()) for n, s in shapes.items()}
    buf = {n: _tailed(numel[n], dev) for n in shapes}
    call("jabd_nlm_attn_fwd_f32", q.data_ptr(), k.data_ptr(), v.data_ptr(), B, P, S, ch,
         buf["ctx"].data_ptr(), buf["lse"].data_ptr() if with_lse else None, None)
    done = ["ctx"]
    if with_lse:
        ctx = buf["ctx"][:numel["ctx"]].clone()  # the saved forward output
        call("jabd_nlm_attn_bwd_f32", q.data_ptr(), k.data_ptr(), v.data_ptr(), ctx.data_ptr(),
             buf["lse"].data_ptr(), d.data_ptr(), B, P, S, ch, buf["dq"].data_ptr(),
             buf["pm"].data_ptr(), buf["dsm"].data_ptr(), None)
        nws = int(lib().jabd_nlm_attn_dkv_ws_floats(B, P, S, ch))
        ws = torch.empty(nws, dtype=torch.float32, device=dev)
        call("jabd_nlm_attn_dkv_f32", buf["dsm"].data_ptr(), buf["pm"].data_ptr(), q.data_ptr(),
             d.data_ptr(), B, P, S, ch, ws.data_ptr(), nws, buf["dk"].data_ptr(),
             buf["dv"].data_ptr(), None)
        done = list(shapes)
    torch.cuda.synchronize()
    out = {}
    for n in shapes:
        assert _tail_intact(buf[n], numel[n]), f"{n}: write past the end of the output"
        body = buf[n][:numel[n]]
        if n in done:
            assert bool(torch.isfinite(body).all()), f"{n}: unwritten or non-finite elements"
            out[n] = body.view(shapes[n]).cpu()
        else:
            assert bool(torch.isnan(body).all()), f"{n}: written without being asked for"
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", A.CORE_CASES, ids=A.core_id)
def test_core_parity(cuda, case):
    inp, ref = A.core_case_data(case)
    got = _core_gpu(inp, cuda)
    errs = A.core_errors(got, ref, inp)
    print(A.core_id(case), f"M={ref['M']:.1f}",
          " ".join(f"{n}={e:.2e}/{bar:.2e}" for n, (e, bar) in errs.items()))
    bad = {n: (e, bar) for n, (e, bar) in errs.items() if not e <= bar}
    assert not bad, f"{A.core_id(case)} (err, bar): {bad}"


@pytest.mark.gpu
def test_core_forward_without_lse(cuda):
    """lse == NULL: same ctx, bit for bit, and nothing else written."""
    inp, ref = A.core_case_data(A.CORE_LSE_NULL_CASE)
    with_lse = _core_gpu(inp, cuda)
    without = _core_gpu(inp, cuda, with_lse=False)
    assert set(without) == {"ctx"}
    assert torch.equal(with_lse["ctx"], without["ctx"])
    e, bar = A.core_errors(without, ref, inp, names=("ctx",))["ctx"]
    assert e <= bar, e


def _reject_calls(dev, ch, S, B, P, null=None):
    """The forward and the backward call at (B, P, S, ch) on generously sized
    buffers; `null` names one pointer passed as NULL.  Returns the outputs."""
    n_pix, n_bin = 2 * 257 * 68, 2 * 321 * 68
    t = {n: torch.ones(n_pix, device=dev) for n in ("q", "dctx", "ctx_in")}
    t.update({n: torch.ones(n_bin, device=dev) for n in ("k", "v")})
    t["lse_in"] = torch.ones(2 * 257, device=dev)
    outs = {"ctx": n_pix, "lse": 2 * 257, "dq": n_pix, "pm": 2 * 321 * 257, "dsm": 2 * 321 * 257}
    t.update({n: torch.full((m,), float("nan"), device=dev) for n, m in outs.items()})
    p = {n: (None if n == null else v.data_ptr()) for n, v in t.items()}
    fwd = ("jabd_nlm_attn_fwd_f32", p["q"], p["k"], p["v"], B, P, S, ch, p["ctx"], p["lse"], None)
    bwd = ("jabd_nlm_attn_bwd_f32", p["q"], p["k"], p["v"], p["ctx_in"], p["lse_in"], p["dctx"],
           B, P, S, ch, p["dq"], p["pm"], p["dsm"], None)
    return fwd, bwd, {n: t[n] for n in outs}


def _expect_rejected(call_args, outs):
    from jabd_amd._lib import call
    with pytest.raises(RuntimeError):
        call(*call_args)
    torch.cuda.synchronize()
    for n, v in outs.items():
        assert bool(torch.isnan(v).all()), f"{n} touched by a rejected call"


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(A.CORE_REJECT))
def test_core_rejects_bad_shapes(cuda, name):
    """attn_check: widths off the built list, K/V over 160 KiB, empty shapes —
    a RuntimeError from the host-side check, before any launch."""
    ch, S, B, P = A.CORE_REJECT[name]
    fwd, bwd, outs = _reject_calls(cuda, ch, S, B, P)
    _expect_rejected(fwd, outs)
    _expect_rejected(bwd, outs)


@pytest.mark.gpu
def test_core_rejects_null_pointers(cuda):
    for null in ("q", "k", "v", "ctx"):
        fwd, _, outs = _reject_calls(cuda, 40, 7, 2, 257, null=null)
        _expect_rejected(fwd, outs)
    for null in ("q", "k", "v", "ctx_in", "lse_in", "dctx", "dq", "pm", "dsm"):
        _, bwd, outs = _reject_calls(cuda, 40, 7, 2, 257, null=null)
        _expect_rejected(bwd, outs)


# ------------------------------------------------------------ GPU: the ch = 4 family
@pytest.mark.gpu
@pytest.mark.parametrize("case", A.NLM4_CASES, ids=A.nlm4_id)
def test_nlm4_parity(cuda, case):
    """out, dsrc, dlat and the eight parameter gradients of NlmFn against the
    fp64 oracle at 1e-4; eval output bit-equal to the training forward's."""
    A.nlm4_check(case, cuda)


@pytest.mark.gpu
def test_nlm4_strided_source(cuda):
    A.nlm4_strided_check(cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("var,flag", [("JABD_NLM_PX", "--px"), ("JABD_NLM_BWD_QUAD", "--quad")])
def test_nlm4_ab_form_in_a_fresh_process(cuda, var, flag):
    """The A/B forms are chosen by statics read once per process: one fresh
    child runs the whole ch = 4 table with the variable set, against the same
    oracle at the same bar, and stops at its first failure.  The table's
    C = 1024 case fits the lane-quad backward's 64 KiB (33 568 B at S = 5), so
    the --quad child runs it too and asserts the limit's RuntimeError on a
    shape that is over it (NLM4_QUAD_OVER)."""
    env = {k: v for k, v in os.environ.items() if k not in ("JABD_NLM_PX", "JABD_NLM_BWD_QUAD")}
    env[var] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_attn_ref.py"), flag],
                       env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, f"{var}=1 child exited {r.returncode}:\n{r.stdout[-6000:]}"
