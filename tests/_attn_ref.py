"""References, inputs and case tables for the NLM attention parity tests
(tests/test_nlm_attn_edges.py); no GPU needed to import or to self-check.

General-width core (csrc/nlm_attn.hip)
  core_ref(inp, dtype)  softmax(q K^T) V, lse, and through autograd dq / dK /
                        dV and the two S-major maps the backward kernel writes
                        (pm[b,s,p] = P, dsm[b,s,p] = P (dctx.V_s - dctx.ctx)).
                        float64 is the oracle, float32 the "honest torch" run.
  core_emulate(inp, defect=None)
                        fp32 numpy emulation of the kernel's own algorithm:
                        one pass with running max m and denominator l, the
                        accumulator rescaled when sc > m, lse = m + log l,
                        the backward via exp(s - lse).  defect= plants one of
                        DEFECTS so the self-checks can show the cases catch it.
  core_inputs(case)     seeded builders "normal" / "peaked" / "monotone".
  CORE_CASES            the table both the GPU tests and the CPU self-checks walk.
  core_bars / core_errors   the bars and the metric (see core_bars).

ch = 4 family (head.hip nlm_kv/pool/apply, nlm_train.hip nlm_bwd_*)
  NLM4_CASES, nlm4_inputs, nlm4_oracle (model_ref.nlm after F.interpolate
  (nearest), as test_train_ops.test_nlmfn_grads builds it), nlm4_gpu /
  nlm4_check (NlmFn.apply + functional.nlm_fused(save=False)), and the
  strided-source check.

`python tests/_attn_ref.py [--px | --quad]` runs the ch = 4 table on the GPU and
exits non-zero at the first failure: JABD_NLM_PX and JABD_NLM_BWD_QUAD are
read once per process, so the A/B forms are tested in a fresh child.
"""
import collections
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as tF

EPS = 2.0 ** -23
DEFECTS = ("no_rescale",     # (a) accumulator not rescaled on a new running max
           "lse_no_log",     # (b) lse = m, log l dropped
           "short_loop")     # (c) bin loops stop at S & ~3


def _rel(got, ref):
    """_util.rel_err: max|got - ref| / max|ref| (NaN / inf in got -> inf)."""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    if not bool(torch.isfinite(got).all()):
        return math.inf
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


# ------------------------------------------------------------ general-width core
CoreCase = collections.namedtuple("CoreCase", "group kind B P S ch seed")
CORE_WIDTHS = tuple(range(8, 65, 4))           # JABD_ATTN_WIDTHS
CORE_LDS_PLAIN = 65536                         # above: hipFuncSetAttribute path
CORE_LDS_MAX = 160 * 1024                      # attn_check's limit


def core_lds_bytes(S, ch):
    """Dynamic LDS of attn_fwd/bwd_kernel: K and V, S*ch floats each."""
    return 2 * S * ch * 4


# seeds of the "normal" cases (see core_inputs): draws whose mean top probability
# is under 0.3 with max|logit| = 3 (it runs 0.27 .. 0.33 over seeds at S = 7)
_NORMAL_SEED = {8: 108, 12: 2012, 16: 316, 20: 3820, 24: 924, 28: 228, 32: 2632, 36: 2836,
                40: 2540, 44: 344, 48: 2548, 52: 1952, 56: 1456, 60: 2860, 64: 3764}


def _core_cases():
    c = []
    for ch in CORE_WIDTHS:
        c.append(CoreCase("width", "normal", 2, 257, 7, ch, _NORMAL_SEED[ch]))
        c.append(CoreCase("width", "peaked", 2, 257, 7, ch, 100 + ch))
    for S in (1, 2, 3, 110):
        for P in (1, 255, 256, 257, 513):
            # P = 1: seeds at which one of the B pixels has two close logits; at most
            # seeds both rows are one-hot to 1e-13 and dsm / dq are rounding noise
            seed = {(2, 1): 314, (3, 1): 304, (110, 1): 302}.get((S, P), 200 + S + P)
            c.append(CoreCase("edges", "peaked", 2, P, S, 40, seed))
    c.append(CoreCase("rescale", "monotone", 2, 300, 110, 40, 301))
    c.append(CoreCase("rescale", "monotone", 2, 300, 33, 64, 302))
    for ch, S in ((40, 204), (40, 205), (64, 160), (64, 256)):
        c.append(CoreCase("lds", "peaked", 2, 300, S, ch, 400 + S))
        c.append(CoreCase("lds", "peaked", 3, 70, S, ch, 500 + S))
    return tuple(c)


CORE_CASES = _core_cases()
CORE_LSE_NULL_CASE = CoreCase("lse_null", "peaked", 2, 257, 7, 40, 140)
# (ch, S, B, P) that attn_check must refuse before any launch
CORE_REJECT = {"ch4": (4, 7, 2, 257), "ch6": (6, 7, 2, 257), "ch68": (68, 7, 2, 257),
               "lds": (64, 321, 2, 257), "B0": (40, 7, 0, 257), "P0": (40, 7, 2, 0),
               "S0": (40, 0, 2, 257)}


def core_id(c):
    return f"{c.group}-{c.kind}-ch{c.ch}-S{c.S}-P{c.P}-B{c.B}"


NORMAL_LOGIT = 3.0   # see core_inputs
MONO_KNOISE, MONO_QNOISE = 0.05, 0.02
PEAKED_LOGIT = 30.0


def _grid(t, bits):
    """Round to multiples of 2^-bits."""
    return torch.round(t * 2.0 ** bits) / 2.0 ** bits


def core_inputs(case):
    """q [B,P,ch], k / v [B,S,ch], dctx [B,P,ch] as fp32 CPU tensors.

    normal / peaked: randn, q scaled so that max|logit| (fp64) is 3 / 30.
    (normal: the width sweep's S = 7 leaves little room.  At a maximum of 4
    the mean top probability is 0.31 .. 0.40, not the flat softmax "normal"
    stands for; from 2.5 down the lse bar 4 * 2^-23 * M shrinks to where
    fp32's half ulp of lse alone is a fifth of it and no fp32 evaluation
    stays within a quarter.  At 3 the honest runs sit at 0.17 .. 0.21 of the
    bar and the top probability at 0.27 .. 0.33 by seed; _NORMAL_SEED picks
    draws under 0.3.)
    monotone: K_s = ((s+1)/S) u + 0.05 noise_s for a fixed unit vector u; the
    first half of the pixels has q = +a u + 0.02 noise (logits rise with s: the
    online softmax rescales on every bin), the second half q = -a u + 0.02
    noise (a new max on the first bin only); q is then scaled so that
    max|logit| is 30.  K's noise is taken orthogonal to u: along u it would be
    as large as the step a/S between two bins and break the order.  Its
    amplitude is 0.05, not 0.01: dq = sum_s dS_s K_s with sum_s dS_s = 0, so
    with nearly collinear K rows dq is what cancellation leaves, max|dq| is
    ~30x below its terms, and every fp32 evaluation (torch's included) sits
    at 0.25 .. 0.55 of the dq bar; at 0.05 the rows differ enough and the
    honest runs stay under 0.15 of it.

    q and K are then rounded to a grid (q 2^-8, K 2^-6; monotone K 2^-10) so
    that every product and partial sum of q . K_s fits fp32's 24 bits: the
    logits are exact in fp32 in any summation order, with or without FMA (the
    self-checks assert it).  Otherwise the rounding of a |logit| ~ 30 dot product alone
    (~ sqrt(ch) ulps of 30, ~5e-6) takes half of the lse / backward bar and an
    honest fp32 evaluation does not stay within a quarter of it; with exact
    logits whatever error the device shows is the softmax code's own.
    """
    B, P, S, ch = case.B, case.P, case.S, case.ch
    g = torch.Generator().manual_seed(case.seed)
    q = torch.randn(B, P, ch, generator=g).double()
    k = torch.randn(B, S, ch, generator=g).double()
    v = torch.randn(B, S, ch, generator=g)
    d = torch.randn(B, P, ch, generator=g)
    target = NORMAL_LOGIT if case.kind == "normal" else PEAKED_LOGIT
    qbits, kbits = 8, 6
    if case.kind == "monotone":
        u = torch.randn(ch, generator=g).double()
        u = (u / u.norm())
        nk = k - (k @ u)[..., None] * u
        ramp = (torch.arange(1, S + 1, dtype=torch.float64) / S)[None, :, None]
        k = ramp * u + MONO_KNOISE * nk
        sign = torch.ones(P, dtype=torch.float64)
        sign[(P + 1) // 2:] = -1.0
        q = 30.0 * sign[None, :, None] * u + MONO_QNOISE * q
        qbits, kbits = 8, 10
    elif case.kind not in ("normal", "peaked"):
        raise ValueError(case.kind)
    k = _grid(k, kbits)
    q = _grid(q * (target / float((q @ k.transpose(1, 2)).abs().max())), qbits)
    return {"q": q.float().contiguous(), "k": k.float().contiguous(), "v": v.contiguous(),
            "dctx": d.contiguous()}


def core_ref(inp, dtype=torch.float64):
    """The plain reference in `dtype` on the CPU (autograd for the backward)."""
    q, k, v = (inp[n].detach().clone().to(dtype).requires_grad_() for n in ("q", "k", "v"))
    d = inp["dctx"].to(dtype)
    lg = q @ k.transpose(1, 2)                 # [B, P, S]
    lg.retain_grad()
    pm = torch.softmax(lg, -1)
    ctx = pm @ v
    (ctx * d).sum().backward()
    return {"ctx": ctx.detach(), "lse": torch.logsumexp(lg.detach(), -1),
            "dq": q.grad, "dk": k.grad, "dv": v.grad,
            "pm": pm.detach().transpose(1, 2).contiguous(),
            "dsm": lg.grad.transpose(1, 2).contiguous(),
            "M": float(lg.detach().abs().max()),
            "top": float(pm.detach().max(-1)[0].mean())}


def _fma(a, b, c):
    """fmaf in numpy: the fp32 product is exact in fp64, one rounding of the sum
    to fp64 and one to fp32 (a double rounding, equal to fmaf's but for rare ties)."""
    return (a.astype(np.float64) * b + c).astype(np.float32)


def _dot2(a, b):
    """dot_lds: two fp32 FMA chains over the channels, added at the end."""
    ch = a.shape[-1]
    s0 = np.zeros(np.broadcast_shapes(a.shape[:-1], b.shape[:-1]), np.float32)
    s1 = s0.copy()
    for c in range(0, ch, 4):
        s0 = _fma(a[..., c], b[..., c], s0)
        s1 = _fma(a[..., c + 1], b[..., c + 1], s1)
        s0 = _fma(a[..., c + 2], b[..., c + 2], s0)
        s1 = _fma(a[..., c + 3], b[..., c + 3], s1)
    return s0 + s1


def core_emulate(inp, defect=None):
    """attn_fwd_kernel / attn_bwd_kernel / the dkv reduction step by step in
    fp32 numpy.  Also returns "resc" [B,P,S], whether bin s took the rescale
    branch for that pixel, and "logits" [B,P,S] as the kernel forms them."""
    if defect is not None and defect not in DEFECTS:
        raise ValueError(defect)
    f = np.float32
    q, k, v, d = (inp[n].numpy().astype(f) for n in ("q", "k", "v", "dctx"))
    B, P, ch = q.shape
    S = k.shape[1]
    Sl = (S & ~3) if defect == "short_loop" else S
    sc = _dot2(q[:, :, None, :], k[:, None, :, :])          # [B, P, S]
    m = np.full((B, P), -np.inf, f)
    l = np.zeros((B, P), f)
    acc = np.zeros((B, P, ch), f)
    resc = np.zeros((B, P, S), bool)
    with np.errstate(all="ignore"):
        for s in range(Sl):
            x = sc[:, :, s]
            up = x > m
            resc[:, :, s] = up
            corr = np.where(up, np.exp(m - x), f(1)).astype(f)
            l = l * corr
            if defect != "no_rescale":
                acc = acc * corr[..., None]
            m = np.where(up, x, m)
            e = np.exp(x - m).astype(f)
            l = l + e
            acc = _fma(e[..., None], v[:, None, s, :], acc)
        ctx = (acc * (f(1) / l)[..., None]).astype(f)
        lse = m if defect == "lse_no_log" else (m + np.log(l).astype(f)).astype(f)
        # backward
        D = np.zeros((B, P), f)
        for c in range(ch):
            D = _fma(d[..., c], ctx[..., c], D)
        dp = _dot2(d[:, :, None, :], v[:, None, :, :])
        pm = np.full((B, P, S), np.nan, f)      # bins the loop never visits stay unwritten
        dsm = pm.copy()
        pm[:, :, :Sl] = np.exp(sc[:, :, :Sl] - lse[..., None]).astype(f)
        dsm[:, :, :Sl] = pm[:, :, :Sl] * (dp[:, :, :Sl] - D[..., None])
        dq = np.zeros((B, P, ch), f)
        for s in range(Sl):
            dq = _fma(dsm[:, :, s, None], k[:, None, s, :], dq)
        pm_t = np.ascontiguousarray(pm.transpose(0, 2, 1))
        dsm_t = np.ascontiguousarray(dsm.transpose(0, 2, 1))
        dk = np.matmul(dsm_t, q).astype(f)
        dv = np.matmul(pm_t, d).astype(f)
    t = torch.from_numpy
    return {"ctx": t(ctx), "lse": t(np.ascontiguousarray(lse)), "dq": t(dq), "dk": t(dk),
            "dv": t(dv), "pm": t(pm_t), "dsm": t(dsm_t), "resc": resc, "logits": t(sc)}


CORE_FWD = ("ctx", "lse")
CORE_BWD = ("pm", "dsm", "dq", "dk", "dv")


def core_bars(M):
    """ctx: 1e-5 under rel_err (the bar test_nlm40_forward_and_gradients holds
    at ch = 40).  lse: absolute, 4 * 2^-23 * max(1, M), M = max|logit| of the
    fp64 reference.  Backward quantities: max(1e-5, 4 * 2^-23 * M) under
    rel_err: the backward forms P = exp(s - lse) with s recomputed in the
    forward's order, so P's relative error is the absolute rounding error of
    lse (half an ulp at magnitude <= M plus the log) ~ 2^-23 * M; the factor 4
    covers the S-term and P-term accumulations."""
    bwd = max(1e-5, 4 * EPS * M)
    b = {"ctx": 1e-5, "lse": 4 * EPS * max(1.0, M)}
    b.update({n: bwd for n in CORE_BWD})
    return b


def core_errors(got, ref, inp, names=CORE_FWD + CORE_BWD):
    """{name: (err, bar)}; the check is err <= bar.  lse: max abs error.  An
    output that is analytically zero (dq, dsm, dk at S = 1) is measured as
    max|got| / (max|dctx| max|V| max|K| ch) instead of the ratio to max|ref|."""
    bars = core_bars(ref["M"])
    S, ch = inp["k"].shape[1], inp["k"].shape[2]
    out = {}
    for n in names:
        g, r = torch.as_tensor(got[n]).double().cpu(), ref[n].double()
        assert g.shape == r.shape, (n, g.shape, r.shape)
        if not bool(torch.isfinite(g).all()):
            e = math.inf
        elif n == "lse":
            e = float((g - r).abs().max())
        elif S == 1 and n in ("dq", "dsm", "dk"):
            scale = float(inp["dctx"].abs().max() * inp["v"].abs().max() * inp["k"].abs().max()) * ch
            e = float(g.abs().max()) / scale
        else:
            e = _rel(g, r)
        out[n] = (e, bars[n])
    return out


_core_cache = {}


def core_case_data(case):
    """(inputs, fp64 reference) of a case, computed once and shared; callers
    must not modify them."""
    if case not in _core_cache:
        inp = core_inputs(case)
        _core_cache[case] = (inp, core_ref(inp, torch.float64))
    return _core_cache[case]


# ------------------------------------------------------------------ ch = 4 family
Nlm4Case = collections.namedtuple("Nlm4Case", "group C hs ws h w sizes lateral peaked seed")
NLM4_TOL = 1e-4          # TOL of test_train_ops.py, the per-op bar of this Function
NLM4_ORDER = ("n.f_query.weight", "n.f_query.bias", "n.f_key.weight", "n.f_key.bias",
              "n.f_value.weight", "n.f_value.bias", "n.W.weight", "n.W.bias")
PSP_FULL, PSP_SMALL = (1, 3, 6, 8), (1, 2)


def _nlm4_cases():
    c = []
    n = [0]

    def add(group, C, hs, ws, h, w, sizes, lateral=True, peaked=False):
        n[0] += 1
        c.append(Nlm4Case(group, C, hs, ws, h, w, tuple(sizes), lateral, peaked, 700 + n[0]))

    for sizes in ((1,), (1, 1), (1, 1, 1), (1, 2), (3,)):       # S = 1, 2, 3, 5, 9
        add("smallS", 40, 4, 4, 8, 8, sizes)
    add("pixels", 40, 1, 1, 1, 1, (1,))
    add("pixels", 40, 3, 26, 5, 51, PSP_SMALL)                   # 255 px
    add("pixels", 40, 8, 8, 16, 16, PSP_FULL)                    # 256 px
    add("pixels", 40, 1, 129, 1, 257, PSP_SMALL)                 # 257 px
    add("pixels", 40, 2, 22, 3, 43, PSP_SMALL)                   # 129 px
    add("pixels", 40, 2, 32, 3, 64, PSP_SMALL)                   # 192 px
    for C in (4, 20, 40, 256):
        add("channels", C, 4, 4, 8, 8, PSP_FULL)
    add("lds", 1024, 2, 3, 4, 5, PSP_SMALL)
    add("standalone", 40, 7, 9, 7, 9, PSP_FULL, lateral=False)
    add("standalone", 20, 1, 5, 1, 5, (1,), lateral=False)
    add("peaked", 40, 8, 8, 16, 16, PSP_FULL, peaked=True)
    add("peaked", 40, 4, 4, 8, 8, (3,), peaked=True)
    add("peaked", 1024, 2, 3, 4, 5, PSP_SMALL, peaked=True)
    return tuple(c)


NLM4_CASES = _nlm4_cases()
NLM4_B = 2
# over the lane-quad backward's 64 KiB of LDS (JABD_NLM_BWD_QUAD=1): S = 404
NLM4_QUAD_OVER = Nlm4Case("quad_limit", 40, 4, 4, 8, 8, (20, 2), True, False, 799)


def nlm4_id(c):
    s = "x".join(map(str, c.sizes))
    return (f"{c.group}-C{c.C}-{c.hs}x{c.ws}-{c.h}x{c.w}-psp{s}"
            + ("" if c.lateral else "-alone") + ("-peaked" if c.peaked else ""))


def nlm4_S(case):
    return sum(s * s for s in case.sizes)


def nlm4_bwd_lds_bytes(C, S, quad=False):
    """nlm_train.hip jabd_nlm_bwd_attn_f32: the 256-pixel kernel holds wW, wq,
    256 q and dctx rows, two 8-bin columns of 257 and the 32 x 8 x 8 partials;
    the lane-quad kernel K, V, wW, wq and 4 waves of S x 8 partials."""
    if quad:
        return (2 * S * 4 + 2 * C * 4 + 4 * S * 8) * 4
    return (2 * C * 4 + 2 * 256 * 4 + 2 * 8 * 257 + 32 * 8 * 8) * 4


def _nlm4_logit_max(P, up, sizes):
    from oracle import model_ref
    c = model_ref.Ctx({k: v.double() for k, v in P.items()})
    x = up.double()
    q = c.conv(x, "n.f_query").flatten(2).transpose(1, 2)
    k = model_ref.psp(c.conv(x, "n.f_key"), sizes)
    return q, k, float((q @ k).abs().max())


def nlm4_attention_inputs(case, inp):
    """The attention stage of the fp64 oracle as core-style fp32 inputs (q
    [B,P,4], K / V [B,S,4], dctx = W^T dy) for core_emulate / core_ref."""
    from oracle import model_ref
    up = (tF.interpolate(inp["src"], size=[case.h, case.w], mode="nearest")
          if case.lateral else inp["src"])
    q, k, _ = _nlm4_logit_max(inp["P"], up, case.sizes)
    c = model_ref.Ctx({n: v.double() for n, v in inp["P"].items()})
    v = model_ref.psp(c.conv(up.double(), "n.f_value"), case.sizes).transpose(1, 2)
    d = tF.conv2d(inp["dy"].double(), inp["P"]["n.W.weight"].double().transpose(0, 1))
    return {"q": q.float().contiguous(), "k": k.transpose(1, 2).float().contiguous(),
            "v": v.float().contiguous(),
            "dctx": d.flatten(2).transpose(1, 2).float().contiguous()}


def nlm4_inputs(case):
    """Seeded fp32 CPU inputs in the layout of test_nlmfn_grads (NCHW)."""
    C, B = case.C, NLM4_B
    g = torch.Generator().manual_seed(case.seed)
    src = torch.randn(B, C, case.hs, case.ws, generator=g)
    lat = torch.randn(B, C, case.h, case.w, generator=g) if case.lateral else None
    P = {"n.f_query.weight": torch.randn(4, C, 1, 1, generator=g) / C ** 0.5,
         "n.f_query.bias": 0.1 * torch.randn(4, generator=g),
         "n.f_key.weight": torch.randn(4, C, 1, 1, generator=g) / C ** 0.5,
         "n.f_key.bias": 0.1 * torch.randn(4, generator=g),
         "n.f_value.weight": torch.randn(4, C, 1, 1, generator=g) / C ** 0.5,
         "n.f_value.bias": 0.1 * torch.randn(4, generator=g),
         "n.W.weight": torch.randn(C, 4, 1, 1, generator=g) / 2,
         "n.W.bias": 0.1 * torch.randn(C, generator=g)}
    dy = torch.randn(B, C, case.h, case.w, generator=torch.Generator().manual_seed(8))
    if case.peaked:  # f_query / f_key scaled so that the fp64 oracle's max|logit| is 30
        up = tF.interpolate(src, size=[case.h, case.w], mode="nearest")
        t = math.sqrt(30.0 / _nlm4_logit_max(P, up, case.sizes)[2])
        for n in ("n.f_query.weight", "n.f_query.bias", "n.f_key.weight", "n.f_key.bias"):
            P[n] = (P[n].double() * t).float()
    return {"src": src, "lat": lat, "P": P, "dy": dy}


def nlm4_oracle(case, inp, dtype=torch.float64):
    """lateral + model_ref.nlm(nearest(src)) and every gradient, in `dtype`."""
    from oracle.model_ref import Ctx, nlm
    Pr = {k: v.detach().clone().to(dtype).requires_grad_() for k, v in inp["P"].items()}
    sr = inp["src"].detach().clone().to(dtype).requires_grad_()
    up = tF.interpolate(sr, size=[case.h, case.w], mode="nearest") if case.lateral else sr
    y = nlm(Ctx(Pr), up, "n.", case.sizes)
    lr = None
    if case.lateral:
        lr = inp["lat"].detach().clone().to(dtype).requires_grad_()
        y = lr + y
    (y * inp["dy"].to(dtype)).sum().backward()
    out = {"out": y.detach(), "dsrc": sr.grad}
    if lr is not None:
        out["dlat"] = lr.grad
    out.update({k: Pr[k].grad for k in NLM4_ORDER})
    return out


def nlm4_stats(case, inp):
    """q [B,P,4], K^T [B,4,S] of the fp64 oracle, max|logit|, mean top probability."""
    up = (tF.interpolate(inp["src"], size=[case.h, case.w], mode="nearest")
          if case.lateral else inp["src"])
    q, k, M = _nlm4_logit_max(inp["P"], up, case.sizes)
    return q, k, M, float(torch.softmax(q @ k, -1).max(-1)[0].mean())


def nlm4_zero_grads(case):
    """Gradients that are analytically zero: f_key.bias shifts every logit of a
    pixel equally (softmax-invariant); with only 1 x 1 PSP levels all K rows
    are the same global mean, the softmax is uniform whatever q is, and
    nothing reaches f_query or f_key at all."""
    z = {"n.f_key.bias"}
    if all(s == 1 for s in case.sizes):
        z |= {"n.f_query.weight", "n.f_query.bias", "n.f_key.weight"}
    return z


def nlm4_errors(case, got, ref):
    """{name: (err, bar)}, check err <= bar.  An analytically zero gradient is
    measured by its size against the largest fp64 gradient, as tests/test_train.py
    does for f_key.bias."""
    gmax = max(float(ref[k].abs().max()) for k in NLM4_ORDER)
    zero = nlm4_zero_grads(case)
    out = {}
    for n, r in ref.items():
        if n in zero:
            g = got[n].double().cpu()
            assert float(r.abs().max()) <= 1e-12 * gmax, (n, "not zero in fp64")
            e = float(g.abs().max()) / gmax if bool(torch.isfinite(g).all()) else math.inf
        else:
            e = _rel(got[n].cpu(), r)
        out[n] = (e, NLM4_TOL)
    return out


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def nlm4_gpu(case, inp, dev):
    """NlmFn.apply forward + backward, and functional.nlm_fused(save=False)
    for eval, whose output must be bit-equal to the training forward's."""
    from jabd_amd import functional as F
    from jabd_amd.train import NlmFn
    Pg = {k: torch.nn.Parameter(v.to(dev)) for k, v in inp["P"].items()}
    sg = _nhwc(inp["src"]).to(dev).requires_grad_()
    lg = _nhwc(inp["lat"]).to(dev).requires_grad_() if case.lateral else None
    yg = NlmFn.apply(sg, lg, *[Pg[k] for k in NLM4_ORDER], case.sizes)
    (yg * _nhwc(inp["dy"]).to(dev)).sum().backward()
    C = case.C
    W = tuple(Pg[k].detach().reshape(*s).contiguous() for k, s in zip(
        NLM4_ORDER, ((4, C), (4,), (4, C), (4,), (4, C), (4,), (C, 4), (C,))))
    ye = F.nlm_fused(sg.detach(), lg.detach() if lg is not None else None, W, case.sizes,
                     save=False)
    torch.cuda.synchronize()
    got = {"out": _nchw(yg.detach()), "dsrc": _nchw(sg.grad)}
    if lg is not None:
        got["dlat"] = _nchw(lg.grad)
    got.update({k: Pg[k].grad for k in NLM4_ORDER})
    return got, bool(torch.equal(ye, yg.detach()))


_nlm4_cache = {}


def nlm4_case_data(case):
    if case not in _nlm4_cache:
        inp = nlm4_inputs(case)
        _nlm4_cache[case] = (inp, nlm4_oracle(case, inp, torch.float64))
    return _nlm4_cache[case]


def nlm4_check(case, dev):
    """Run one case on the GPU; returns the worst (err, name), raises
    AssertionError naming every quantity over its bar."""
    inp, ref = nlm4_case_data(case)
    got, same = nlm4_gpu(case, inp, dev)
    errs = nlm4_errors(case, got, ref)
    print(nlm4_id(case), " ".join(f"{n.replace('n.', '')}={e:.2e}" for n, (e, _) in errs.items()))
    bad = {n: e for n, (e, b) in errs.items() if not e <= b}
    assert not bad, f"{nlm4_id(case)}: over {NLM4_TOL:g}: {bad}"
    assert same, f"{nlm4_id(case)}: eval output differs from the training forward's"
    return max((e, n) for n, (e, _) in errs.items())


def nlm4_strided_check(dev):
    """jabd_nlm_pool_f32 + jabd_nlm_apply_f32 on a C = 40 slice of a 48-channel
    NHWC buffer (src_ps = 48, offset 4 floats = 16 bytes): bit-equal to the
    contiguous call."""
    import ctypes
    from jabd_amd._lib import call
    B, C, Cb, off, hs, ws, h, w, sizes = 2, 40, 48, 4, 4, 6, 8, 11, (1, 3)
    S = sum(s * s for s in sizes)
    g = torch.Generator().manual_seed(48)
    buf = torch.randn(B, hs, ws, Cb, generator=g).to(dev)
    lat = torch.randn(B, h, w, C, generator=g).to(dev)
    wq, wk, wv = (torch.randn(4, C, generator=g).to(dev) / C ** 0.5 for _ in range(3))
    bq, bk, bv = (0.1 * torch.randn(4, generator=g).to(dev) for _ in range(3))
    wW, bW = torch.randn(C, 4, generator=g).to(dev) / 2, 0.1 * torch.randn(C, generator=g).to(dev)
    arr = (ctypes.c_int32 * len(sizes))(*sizes)
    outs = []
    for strided in (False, True):
        if strided:
            src, ptr, bs, ps = buf, buf.data_ptr() + 4 * off, hs * ws * Cb, Cb
        else:
            src = buf[..., off:off + C].contiguous()
            ptr, bs, ps = src.data_ptr(), hs * ws * C, C
        kp = torch.full((B, S, 4), float("nan"), device=dev)
        vp = torch.full((B, S, 4), float("nan"), device=dev)
        kv = torch.empty((B, hs * ws, 8), device=dev)
        out = torch.full((B, h, w, C), float("nan"), device=dev)
        call("jabd_nlm_pool_f32", ptr, bs, ps, B, hs, ws, C, h, w, wk.data_ptr(), bk.data_ptr(),
             wv.data_ptr(), bv.data_ptr(), 4, arr, len(sizes), kp.data_ptr(), vp.data_ptr(),
             kv.data_ptr(), None)
        call("jabd_nlm_apply_f32", ptr, bs, ps, B, hs, ws, C, h, w, wq.data_ptr(), bq.data_ptr(),
             kp.data_ptr(), vp.data_ptr(), S, 4, wW.data_ptr(), bW.data_ptr(), lat.data_ptr(),
             out.data_ptr(), None, None, None)
        torch.cuda.synchronize()
        outs.append((kp, vp, out))
        del src
    for a, b, n in zip(outs[0], outs[1], ("kpool", "vpool", "out")):
        assert bool(torch.isfinite(a).all()), n
        assert torch.equal(a, b), f"strided source: {n} differs from the contiguous call"


def nlm4_quad_limit_check(dev):
    """The lane-quad backward refuses a shape over its 64 KiB of LDS with a
    RuntimeError (a host-side check before the launch)."""
    case = NLM4_QUAD_OVER
    assert nlm4_bwd_lds_bytes(case.C, nlm4_S(case), quad=True) > 64 * 1024
    inp = nlm4_inputs(case)
    try:
        nlm4_gpu(case, inp, dev)
    except RuntimeError as e:
        assert "nlm_bwd_attn" in str(e), e
        return
    raise AssertionError("JABD_NLM_BWD_QUAD=1: no RuntimeError over 64 KiB of LDS")


def main(argv):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "jabd-joint-attention-based-detector-for-small-face-detection_amd")
    for p in (pkg, root):
        if p not in sys.path:
            sys.path.insert(0, p)
    quad = "--quad" in argv
    assert (os.environ.get("JABD_NLM_BWD_QUAD") == "1") == quad, "--quad goes with JABD_NLM_BWD_QUAD=1"
    assert (os.environ.get("JABD_NLM_PX") == "1") == ("--px" in argv), "--px goes with JABD_NLM_PX=1"
    if not torch.cuda.is_available():
        print("no HIP device")
        return 2
    dev = torch.device("cuda:0")
    worst = (0.0, "")
    try:
        for case in NLM4_CASES:
            e, n = nlm4_check(case, dev)
            worst = max(worst, (e, nlm4_id(case) + ":" + n))
        nlm4_strided_check(dev)
        if quad:
            nlm4_quad_limit_check(dev)
    except AssertionError as e:
        print("FAIL", e)
        return 1
    print(f"ok: {len(NLM4_CASES)} cases, worst rel_err {worst[0]:.2e} ({worst[1]}), bar {NLM4_TOL:g}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
