"""Float64 reference of the fused inference conv with a derived error bound,
and the operator-level cases of tests/test_conv_dispatch.py (shared with the
CPU test of the bound, tests/test_convref.py).

Everything here runs on the CPU; tensors are NCHW as in torch.

The bound.  A kernel computes act(sum_k x_k s_k w_k + bias + res) in fp32, in
some order (tiles, K stages, split-K partial sums).  For any order the
computed sum of K_tot products differs from the exact one by at most
gamma_K * sum_k |x_k s_k w_k| (Higham, Accuracy and Stability, (3.5)); the
gate multiply, the bias add, the residual add and the final rounding add one
unit roundoff each, so with u = 2^-24

    E = (K_tot + 8) * u * (sum_k |x_k s_k w_k| + |bias| + |res|)

bounds the error of the pre-activation value for every correct kernel
(gamma_n = n u / (1 - n u) < (n + 1) u for the K here).  An activation with
slope <= L scales that by L (hswish: 1.5 at x = 3; relu, leaky, none: 1) and
adds its own rounding, which csrc/common.h documents as within 2 ulp; the
check allows 4 ulp of the reference:

    |got - ref| <= L * E + 4 u |ref|.

No constant is measured.  A typical product term is about 1 / (K_tot^2 u)
times E, so for K_tot < 4000 a dropped or doubled term exceeds the bound.
"""
import torch
import torch.nn.functional as tF

U = 2.0 ** -24


def act64(z, act, slope=0.0):
    if act == "none":
        return z
    if act == "relu":
        return z.clamp_min(0)
    if act == "leaky":
        return torch.where(z > 0, z, z * slope)
    if act == "hswish":
        return z * ((z + 3).clamp(0, 6) / 6)
    raise ValueError(act)


def _x2_at(x2, x2_stride, OH, OW):
    """The second source at the output pixels: x2[..., oh * s, ow * s]."""
    return x2[:, :, ::x2_stride, ::x2_stride][:, :, :OH, :OW]


def conv_ref64(x, w, bias=None, stride=1, pad=0, gate=None, x2=None, w2=None, x2_stride=1,
               res=None, act="none", slope=0.0):
    """act(conv(x * gate[b, c], w) + x2 @ w2 + bias + res) in float64.

    x [B,Cin,H,W], w [Cout,Cin,KH,KW], bias [Cout], gate [B,Cin], x2
    [B,Cin2,H2,W2] taken at (oh * x2_stride, ow * x2_stride), w2 [Cout,Cin2],
    res [B,Cout,OH,OW]: the fp32 values the packed weights were built from.
    Returns (z, y, E): the pre-activation value, the output and the bound on
    the pre-activation error of an fp32 kernel (module docstring), float64."""
    d = torch.float64
    xs = x.to(d)
    if gate is not None:
        xs = xs * gate.to(d)[:, :, None, None]
    wd = w.to(d)
    z = tF.conv2d(xs, wd, None, stride, pad)
    mag = tF.conv2d(xs.abs(), wd.abs(), None, stride, pad)
    ktot = w.shape[1] * w.shape[2] * w.shape[3]
    if x2 is not None:
        OH, OW = z.shape[2], z.shape[3]
        v = _x2_at(x2.to(d), x2_stride, OH, OW)
        w2d = w2.to(d)[:, :, None, None]
        z = z + tF.conv2d(v, w2d)
        mag = mag + tF.conv2d(v.abs(), w2d.abs())
        ktot += w2.shape[1]
    if bias is not None:
        z = z + bias.to(d)[None, :, None, None]
        mag = mag + bias.to(d).abs()[None, :, None, None]
    if res is not None:
        z = z + res.to(d)
        mag = mag + res.to(d).abs()
    return z, act64(z, act, slope), (ktot + 8) * U * mag


def check(got, ref, E, act):
    """(ok, worst): whether |got - ref| <= L E + 4 u |ref| everywhere (a NaN
    fails) and the largest |got - ref| / that tolerance."""
    L = 1.5 if act == "hswish" else 1.0
    tol = L * E + 4 * U * ref.abs()
    err = (got.to(torch.float64) - ref).abs()
    ok = bool((err <= tol).all())
    worst = float((err / tol.clamp_min(1e-300)).nan_to_num(nan=float("inf")).max())
    return ok, worst


def terms_at(t, b, n, oh, ow):
    """The K_tot product terms x_k s_k w_k of output (b, n, oh, ow), float64."""
    d = torch.float64
    x, w = t["x"].to(d), t["w"].to(d)
    if t["gate"] is not None:
        x = x * t["gate"].to(d)[:, :, None, None]
    s, p = t["stride"], t["pad"]
    out = []
    for kh in range(w.shape[2]):
        for kw in range(w.shape[3]):
            ih, iw = oh * s - p + kh, ow * s - p + kw
            if 0 <= ih < x.shape[2] and 0 <= iw < x.shape[3]:
                out.append(x[b, :, ih, iw] * w[n, :, kh, kw])
    if t["x2"] is not None:
        xs = t["x2_stride"]
        out.append(t["x2"].to(d)[b, :, oh * xs, ow * xs] * t["w2"].to(d)[n])
    return torch.cat(out)


# --------------------------------------------------------------------------- the cases
# id -> dict(cin, cout, B, hw [input], k, stride, gate, bias, res, act, cin2, x2_stride,
#            gate_pad [floats the gate rows' pitch exceeds Cin by; 0: the test's default])
def _c(cin, cout, B, hw, k=1, stride=1, gate=False, bias=False, res=False, act="none", cin2=0,
       x2_stride=1, gate_pad=0):
    return dict(cin=cin, cout=cout, B=B, hw=hw, k=k, stride=stride, gate=gate, bias=bias, res=res,
                act=act, cin2=cin2, x2_stride=x2_stride, gate_pad=gate_pad)


CASES = {
    # conv1x1_m32 tile kernel, 1x1
    "a": _c(96, 96, 2, (5, 7), bias=True, act="relu"),
    "a_b3": _c(96, 96, 3, (5, 7), bias=True, act="relu"),   # batch invariance
    "b_none": _c(100, 100, 2, (5, 7)),
    "b_res": _c(100, 100, 2, (5, 7), res=True),
    "b_bias_leaky": _c(100, 100, 2, (5, 7), bias=True, act="leaky"),
    "c": _c(480, 112, 3, (9, 5), gate=True, bias=True, res=True, act="hswish"),
    "d": _c(96, 96, 2, (182, 181), gate=True, bias=True, act="relu"),
    "e160": _c(96, 160, 1, (6, 7), bias=True),
    "e192": _c(96, 192, 1, (6, 7), bias=True),
    "e224": _c(96, 224, 1, (6, 7), bias=True),
    "f": _c(96, 160, 2, (128, 128), gate=True, bias=True),
    "g96_s1": _c(96, 96, 2, (5, 7), bias=True, cin2=32),
    "g96_s2": _c(96, 96, 2, (5, 7), bias=True, cin2=32, x2_stride=2),
    "g100_s1": _c(100, 96, 2, (5, 7), bias=True, cin2=28),
    "g100_s2": _c(100, 96, 2, (5, 7), bias=True, cin2=28, x2_stride=2),
    "g100_s1_gated": _c(100, 96, 2, (5, 7), gate=True, bias=True, cin2=28),
    "h": _c(1056, 96, 2, (3, 5), gate=True, bias=True),
    # split-K (each also run with split-K off)
    "i": _c(1056, 128, 1, (4, 4), bias=True, res=True, act="relu"),
    "j": _c(64, 64, 1, (7, 9), k=3, bias=True),
    "k": _c(128, 128, 1, (9, 11), k=3, stride=2, bias=True),
    "l": _c(1056, 96, 2, (3, 5), gate=True, bias=True),
    # conv1x1_m32 k x k without split
    "m": _c(64, 64, 2, (5, 7), k=3, gate=True, bias=True, act="leaky"),
    "n": _c(32, 64, 2, (7, 6), k=3, stride=2, bias=True),
    # conv1x1 (the conv.hip fallback)
    "o1": _c(16, 16, 3, (33, 31), gate=True, bias=True, res=True, act="relu"),
    "o2": _c(64, 24, 3, (17, 23), gate=True, bias=True, act="relu", cin2=16),
    "o3": _c(200, 80, 3, (12, 13), gate=True, bias=True, res=True, act="hswish"),
    "o4": _c(240, 80, 3, (5, 9), gate=True, bias=True, act="hswish", cin2=40),
    "o": _c(256, 64, 2, (5, 7), bias=True, act="relu"),
    "p": _c(40, 120, 2, (5, 7), bias=True),
    "q": _c(64, 24, 2, (5, 7), gate=True, bias=True, cin2=16, x2_stride=2),
    "r": _c(16, 16, 2, (257, 255), gate=True, bias=True),
    # conv1x1_stream
    "s": _c(16, 16, 3, (4, 12), gate=True, bias=True, res=True),
    "t": _c(200, 80, 3, (4, 12), gate=True, bias=True, res=True, act="hswish"),
    "u": _c(240, 80, 3, (8, 6), gate=True, bias=True, act="hswish", cin2=40),
    "v": _c(40, 40, 3, (31, 7), bias=True),
    # conv_gemm
    "w": _c(10, 12, 2, (5, 7), k=3, bias=True, act="relu"),
    "x": _c(96, 32, 2, (5, 7), k=3, bias=True, res=True),
    "y": _c(40, 40, 2, (9, 11), k=3, stride=2, gate=True, bias=True, gate_pad=2),
}

SLOPE = 0.1  # LeakyReLU slope of the leaky cases

_CACHE = {}


def out_hw(c):
    pad = c["k"] // 2
    H, W = c["hw"]
    return (H + 2 * pad - c["k"]) // c["stride"] + 1, (W + 2 * pad - c["k"]) // c["stride"] + 1


def tensors(name, img=None):
    """The fp32 CPU operands of case `name` (seeded), cached and never
    modified; img: that one image of the batch alone (a bs1 run of it)."""
    c = CASES[name]
    full = _CACHE.get(name)
    if full is None:
        g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
        Bc, (H, W), k = c["B"], c["hw"], c["k"]
        OH, OW = out_hw(c)
        ktot = c["cin"] * k * k + c["cin2"]
        full = dict(stride=c["stride"], pad=k // 2, x2_stride=c["x2_stride"], act=c["act"],
                    slope=SLOPE if c["act"] == "leaky" else 0.0)
        full["x"] = torch.randn(Bc, c["cin"], H, W, generator=g)
        full["w"] = torch.randn(c["cout"], c["cin"], k, k, generator=g) / ktot ** 0.5
        full["bias"] = torch.randn(c["cout"], generator=g) * 0.5 if c["bias"] else None
        full["gate"] = torch.rand(Bc, c["cin"], generator=g) if c["gate"] else None
        full["x2"] = full["w2"] = None
        if c["cin2"]:
            s = c["x2_stride"]
            full["x2"] = torch.randn(Bc, c["cin2"], OH * s, OW * s, generator=g)
            full["w2"] = torch.randn(c["cout"], c["cin2"], generator=g) / ktot ** 0.5
        full["res"] = torch.randn(Bc, c["cout"], OH, OW, generator=g) if c["res"] else None
        _CACHE[name] = full
    if img is None:
        return full
    cut = dict(full)
    for key in ("x", "gate", "x2", "res"):
        if full[key] is not None:
            cut[key] = full[key][img:img + 1]
    return cut


def reference(name, img=None):
    """(z, y, E) of case `name` (conv_ref64 of tensors(name, img)), cached."""
    key = (name, img)
    if key not in _CACHE:
        t = tensors(name, img)
        _CACHE[key] = conv_ref64(t["x"], t["w"], t["bias"], t["stride"], t["pad"], t["gate"],
                                 t["x2"], t["w2"], t["x2_stride"], t["res"], t["act"], t["slope"])
    return _CACHE[key]
