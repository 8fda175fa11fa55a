"""Exact-data inputs, fp64 references, case tables, host-plan restatements and
planted defects for the depthwise / BatchNorm training-kernel edge tests
(tests/test_dw_train_edges.py, tests/test_bn_train_edges.py).

The method.  The kernels under test are linear, or piecewise linear with
relu / leaky(0.5).  Their inputs here are small nonzero integers (or dyadic
rationals with a known quantum q), so every product and every partial sum is
an integer multiple of q below 2^24 * q: fp32 arithmetic is then exact in any
order, with or without FMA contraction, and the device result must EQUAL the
fp64 reference.  One product dropped, counted twice or misplaced moves the
answer by at least q.  `assert_exact` is the condition that keeps this honest
(sum of absolute terms, in units of q, below 2^24 with ROOM to spare); it is
asserted on the CPU for every case before any device work.

Numpy only (no torch): the non-gpu self-checks and the gpu tests share these
references, and a child process can import the module on its own.
"""
import zlib
from collections import namedtuple

import numpy as np

TWO24 = float(1 << 24)
ROOM = 2.0            # every exactness condition holds with this factor to spare
ACT = {"none": 0, "relu": 1, "leaky": 2}
SLOPE = 0.5
KS = ((3, 1), (3, 2), (5, 1), (5, 2))
F32 = np.float32
F64 = np.float64


def cdiv(a, b):
    return -(-a // b)


def out_size(n, k, s):
    p = k // 2
    return (n + 2 * p - k) // s + 1


# ------------------------------------------------------------ host plans, restated
# Plain-Python restatements of the host code in csrc/train.hip and
# csrc/dwconv.hip.  The tests name every case's expected form from these, and
# compare them with the counts the library exports.
def bn_lanes(C):                     # BN reductions: lanes of a 256-thread block
    return min(C // 4, 256)


def bn_rows_pass(C):
    return 256 // bn_lanes(C)


def bn_rows_per_blk(M, C):
    rp = bn_rows_pass(C)
    per = cdiv(cdiv(M, 1024), rp) * rp
    return max(per, rp)


def bn_nblk(M, C):
    return cdiv(M, bn_rows_per_blk(M, C))


EW_ITERS = 8


def ew_lanes(C):                     # elementwise kernels and the depthwise gradients
    return min(C // 4, 64)


def ew_rows_pass(C):
    return 256 // ew_lanes(C)


def bn_sum_rp(C):
    rp = 1
    while rp * 2 * ew_lanes(C) <= 256:
        rp *= 2
    return rp


def bn_sum_rows(C):
    return bn_sum_rp(C) * EW_ITERS


def bn_sum_nblk(hw, C):
    rb = bn_sum_rows(C)
    return 0 if hw % rb else hw // rb


def dw_sp(C):                        # strips in flight per pass of the forward's workgroup
    return 256 // (C // 4)


def dw_strips_per_blk(B, OH, OW, C):
    sp = dw_sp(C)
    nstrip = OH * cdiv(OW, 4)
    per = cdiv(cdiv(nstrip * B, 2048), sp) * sp
    return max(per, sp)


def dw_nblk(B, OH, OW, C):
    return cdiv(OH * cdiv(OW, 4), dw_strips_per_blk(B, OH, OW, C))


Route = namedtuple("Route", "name PW R nch nbands nblk")


def _rows_plan(rows, budget):
    """want / R / nch of the row walkers: `budget` chunks for `rows` rows."""
    want = max(1, min(rows, budget))
    R = cdiv(rows, want)
    return R, cdiv(rows, R)


def dw_fwd_route(B, H, W, C, k, s, rows_on=True):
    """Form of the statistics forward (dwconv_stats in dwconv.hip)."""
    OH, OW = out_size(H, k, s), out_size(W, k, s)
    nblk = dw_nblk(B, OH, OW, C)
    if rows_on and k == 3:
        PW = 4 if s == 1 else 2
        nbands = cdiv(cdiv(OW, PW), dw_sp(C))
        if nbands <= nblk:
            R, nch = _rows_plan(OH, nblk // nbands)
            return Route("dwconv_stats_rows", PW, R, nch, nbands, nblk)
    return Route("dwconv_stats", 4, 0, 0, 0, nblk)


def dgbn_plan(B, H, W, C):
    groups = B * cdiv(cdiv(W, 8), ew_rows_pass(C)) * H
    spb = cdiv(groups, 8192)
    return cdiv(groups, spb), spb, groups


def dgbn_route(B, H, W, C, k, s, store_dz, rows_on=False):
    """Launch names of jabd_dw_dgrad_bn_bwd_f32 and the partials kernel's plan."""
    nblk, spb, _ = dgbn_plan(B, H, W, C)
    if rows_on and k == 3:
        PW = 4 if s == 1 else 8
        nbands = cdiv(cdiv(W, PW), ew_rows_pass(C))
        if B * nbands <= nblk:
            R, nch = _rows_plan(H, nblk // (B * nbands))
            names = ["dw_dgrad_bn_rows", "bn_bwd_final",
                     "bn_bwd_apply" if store_dz else "dw_dgrad_bn_rows_apply"]
            return names, Route(names[0], PW, R, nch, nbands, nblk)
    names = ["dw_dgrad_bn", "bn_bwd_final", "bn_bwd_apply" if store_dz else "dw_dgrad_bn_apply"]
    return names, Route(names[0], 8, spb, 0, 0, nblk)


def wgrad_route(B, H, W, C, k, s, rows_on=True):
    """Form of the depthwise weight gradient (dw_wgrad in train.hip); for the
    strip form R holds the items per block (`per`)."""
    OH, OW = out_size(H, k, s), out_size(W, k, s)
    rp = ew_rows_pass(C)
    if rows_on and k == 3:
        PW = 4 if s == 1 else 2
        nbands = cdiv(cdiv(OW, PW), rp)
        if B * nbands <= 1024:
            R, nch = _rows_plan(OH, 1024 // (B * nbands))
            return Route("dw_wgrad_rows", PW, R, nch, nbands, B * nbands * nch)
    PW = 8 if (k, s) == (3, 1) else 4
    items = B * OH * cdiv(cdiv(OW, PW), rp) * rp
    per = cdiv(cdiv(items, 1024), rp) * rp
    return Route("dw_wgrad", PW, per, 0, 0, cdiv(items, per))


# ------------------------------------------------------------ case tables
DwCase = namedtuple("DwCase", "group B H W C k s")


def dw_id(c):
    return f"{c.group}-B{c.B}-{c.H}x{c.W}-C{c.C}-k{c.k}s{c.s}"


CHAN_C = (4, 12, 72, 256, 260, 960)
CHAN_CASES = tuple(DwCase("chan", 2, 5, 9, C, k, s) for (k, s) in KS for C in CHAN_C)
CHAN_FWD_ONLY = tuple(DwCase("chan1024", 2, 5, 9, 1024, k, s) for (k, s) in KS)

# H and W over {1, 2, 3, 7, 8, 9, 17}: 20 maps in which every H value and every
# W value occurs at least twice, the five named ones included; crossed with
# C in {12, 256} and every (k, stride), so every value of one factor meets
# every value of each other factor.
SPATIAL_MAPS = ((1, 1), (1, 17), (17, 1), (2, 2), (8, 9),
                (1, 8), (2, 7), (2, 17), (3, 1), (3, 3), (3, 9), (7, 2), (7, 7), (7, 8),
                (8, 3), (8, 17), (9, 2), (9, 9), (9, 7), (17, 3))
SPATIAL_CASES = tuple(DwCase("spatial", 2, h, w, C, k, s)
                      for (k, s) in KS for C in (12, 256) for (h, w) in SPATIAL_MAPS)

# Row-chunk seams of dw_wgrad_rows_kernel: B = 512 and a one-band map give
# want = 2, R = ceil(OH / 2) = 1..5, the last chunk short for odd OH.
WG_ROWS_OH = (2, 3, 5, 7, 9)


def _wg_rows_cases():
    out = []
    for s in (1, 2):
        for oh in WG_ROWS_OH:
            h = oh if s == 1 else 2 * oh - (oh % 2)    # odd and even H at stride 2
            out.append(DwCase("wgrows", 512, h, 3, 12, 3, s))
        out.append(DwCase("wgrows", 512, 5 if s == 1 else 10, 9, 256, 3, s))
    return tuple(out)


WG_ROWS_CASES = _wg_rows_cases()


def _fwd_rows_cases():
    """For dw_rows_kernel the chunk plan follows the forward's block count, so
    the shapes are searched from the restated plan: per stride and R = 1..5 the
    smallest map with at least two chunks (a short last chunk where one exists)."""
    out = []
    for s in (1, 2):
        for R in (1, 2, 3, 4, 5):
            best = None
            for C in (960, 516, 256, 72, 12):
                for B in (1, 2, 3, 64, 512, 1025, 2049):
                    for H in range(1, 21):
                        for W in (3, 4, 8, 9):
                            n = B * H * W * C
                            if n > (1 << 23):
                                continue
                            r = dw_fwd_route(B, H, W, C, 3, s)
                            if r.name != "dwconv_stats_rows" or r.R != R or r.nch < 2:
                                continue
                            short = out_size(H, 3, s) % R != 0
                            key = (not short and R > 1, n)
                            if best is None or key < best[0]:
                                best = (key, DwCase("fwdrows", B, H, W, C, 3, s))
            if best is not None:
                out.append(best[1])
    return tuple(out)


FWD_ROWS_CASES = _fwd_rows_cases()


def _dg_rows_cases():
    """Row chunks of dw_dgrad_bn_rows_kernel (JABD_DW_DGRAD_ROWS=1), searched
    from the restated plan like the forward's: per stride, R = 1..5 over at
    least two chunks.  In the default build the same shapes run the strip form."""
    out = []
    for s in (1, 2):
        for R in (1, 2, 3, 4, 5):
            best = None
            for C in (256, 72, 12, 4):
                for B in (1, 2, 3, 512, 1025, 2049):
                    for H in range(1, 21):
                        for W in (3, 9, 17, 33, 65):
                            n = B * H * W * C
                            if n > (1 << 21):
                                continue
                            r = dgbn_route(B, H, W, C, 3, s, True, rows_on=True)[1]
                            if r.name != "dw_dgrad_bn_rows" or r.R != R or r.nch < 2:
                                continue
                            key = (H % R == 0 and R > 1, n)
                            if best is None or key < best[0]:
                                best = (key, DwCase("dgrows", B, H, W, C, 3, s))
            if best is not None:
                out.append(best[1])
    return tuple(out)


DG_ROWS_CASES = _dg_rows_cases()

# Form fallbacks of the default build.
WG_FALLBACK_CASES = tuple(DwCase("wgfall", 1025, 2, 3, 12, 3, s) for s in (1, 2))
FWD_FALLBACK_CASES = (DwCase("fwdfall", 2, 1, 16, 960, 3, 2), DwCase("fwdfall", 2, 2, 16, 960, 3, 2),
                      DwCase("fwdfall1", 1025, 1, 8, 516, 3, 1))  # 17 MB: the stride-1 fallback
# Block plans.
DGBN_SPB_CASES = tuple(DwCase("dgbnspb", 1025, 9, 3, 4, k, s) for (k, s) in KS)
WG_PER_CASES = tuple(DwCase("wgper", 1025, 2, 3, 256, 5, s) for s in (1, 2))

ALL_DW_CASES = (CHAN_CASES + CHAN_FWD_ONLY + SPATIAL_CASES + WG_ROWS_CASES + FWD_ROWS_CASES
                + DG_ROWS_CASES + WG_FALLBACK_CASES + FWD_FALLBACK_CASES + DGBN_SPB_CASES + WG_PER_CASES)

# Inference entry (jabd_dwconv_nhwc_f32): x and y are channel slices of wider buffers.
INFER_CASES = tuple(DwCase("infer", 2, 5, 9, C, k, s) for (k, s) in KS for C in (12, 260))


def case_act(c):
    """The activation a case uses where it is free to choose one."""
    return ("relu", "leaky", "none")[zlib.crc32(repr(tuple(c)).encode()) % 3]


# ------------------------------------------------------------ inputs
def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def ints(rng, shape, vals):
    return rng.choice(np.asarray(vals, dtype=F64), size=shape)


X_VALS = (-2, -1, 1, 2)
W_VALS = (-2, -1, 1, 2)
DY_VALS = (-3, -2, -1, 1, 2, 3)
BIAS_VALS = (-3, -2, -1, 1, 2, 3)

BnP = namedtuple("BnP", "mean invstd gamma beta")


def bn_params(rng, C, invstd=(0.5, 1.0), gamma=(-2.0, 2.0), beta=(-1.5, -0.5, 0.5, 1.5)):
    """Dyadic BatchNorm operands: integer mean, power-of-two invstd, gamma with
    invstd * gamma an integer, beta = integer + 0.5.  For integer x, xhat =
    (x - mean) * invstd and z = xhat * gamma + beta are exact, and z is an
    integer + 0.5: never on a kink."""
    return BnP(ints(rng, C, (-1, 0, 1)), ints(rng, C, invstd), ints(rng, C, gamma),
               ints(rng, C, beta))


def dw_data(c):
    rng = rng_for("dw", *c)
    OH, OW = out_size(c.H, c.k, c.s), out_size(c.W, c.k, c.s)
    return dict(x=ints(rng, (c.B, c.H, c.W, c.C), X_VALS), w=ints(rng, (c.k * c.k, c.C), W_VALS),
                dy=ints(rng, (c.B, OH, OW, c.C), DY_VALS), bias=ints(rng, c.C, BIAS_VALS),
                bn=bn_params(rng, c.C))


# ------------------------------------------------------------ arithmetic in a chosen order
class Summer:
    """How a reference adds: fp64 (the reference), or fp32 one term after the
    other, in the natural order or in a seeded random permutation of it."""

    def __init__(self, f32=False, seed=None):
        self.f32 = f32
        self.rng = None if seed is None else np.random.default_rng(seed)

    def taps(self, n, term):
        """sum_{i<n} term(i) elementwise (the terms of one output)."""
        order = range(n) if self.rng is None else self.rng.permutation(n)
        if not self.f32:
            acc = 0.0
            for i in range(n):
                acc = acc + term(i)
            return acc
        acc = None
        for i in order:
            t = term(int(i)).astype(F32)
            acc = t if acc is None else (acc + t).astype(F32)
        return acc.astype(F64)

    def rows(self, T):
        """Sum of T [N, C] over its rows (a reduction over pixels)."""
        if not self.f32:
            return T.sum(0)
        if self.rng is not None:
            T = T[self.rng.permutation(T.shape[0])]
        return np.cumsum(T.astype(F32), axis=0, dtype=F32)[-1].astype(F64)


REF = Summer()


def assert_exact(what, abs_sum, q=1.0):
    """The 2^24 condition: the sum of absolute terms of every output, in units
    of the quantum q, is below 2^24 / ROOM (so every partial sum, in any order,
    is an fp32 integer multiple of q)."""
    worst = float(np.max(abs_sum)) / q if np.size(abs_sum) else 0.0
    assert worst * ROOM < TWO24, f"{what}: sum|terms| / q = {worst:.3g} leaves no {ROOM}x room below 2^24"
    return worst


def assert_quantum(what, v, q):
    r = np.asarray(v) / q
    assert np.array_equal(r, np.round(r)), f"{what}: not a multiple of {q}"


# ------------------------------------------------------------ references
def act_f(z, act):
    if act == "relu":
        return np.maximum(z, 0.0)
    if act == "leaky":
        return np.where(z > 0, z, z * SLOPE)
    return z


def act_d(z, act):
    if act == "relu":
        return np.where(z > 0, 1.0, 0.0)
    if act == "leaky":
        return np.where(z > 0, 1.0, SLOPE)
    return np.ones_like(z)


def bn_xhat(x, bn):
    return (x - bn.mean) * bn.invstd


def bn_z(x, bn, res=None):
    z = bn_xhat(x, bn) * bn.gamma + bn.beta
    return z if res is None else z + res


class Taps:
    """Tap-shifted views of a zero-padded NHWC input: view(t)[b, oh, ow] =
    x[b, oh*s - pad + kh, ow*s - pad + kw] (0 outside), t = kh*k + kw."""

    def __init__(self, x, k, s, shift_tap=None):
        B, H, W, C = x.shape
        p = k // 2
        self.k, self.s, self.shift_tap = k, s, shift_tap
        self.OH, self.OW = out_size(H, k, s), out_size(W, k, s)
        self.xp = np.zeros((B, H + 2 * p + 1, W + 2 * p + 1, C))   # +1: room for defect (d)
        self.xp[:, p:p + H, p:p + W] = x

    def view(self, t):
        kh, kw = divmod(t, self.k)
        if t == self.shift_tap:
            kw += 1                                               # defect (d)
        s = self.s
        return self.xp[:, kh:kh + s * (self.OH - 1) + 1:s, kw:kw + s * (self.OW - 1) + 1:s]


def dgrad_term(dy, w, H, W, k, s, t, flip=False):
    """Tap t's contribution to dx [B, H, W, C]: dy[b, oh, ow] * w[t] lands on
    (oh*s - pad + kh, ow*s - pad + kw).  flip: defect (f), the stride-2 row
    parity test inverted (the tap reads the dy row of the other parity)."""
    B, OH, OW, C = dy.shape
    p = k // 2
    kh, kw = divmod(t, k)
    buf = np.zeros((B, H + 2 * p + 2, W + 2 * p + 2, C))
    r0 = kh + (1 if flip else 0)
    buf[:, r0:r0 + s * (OH - 1) + 1:s, kw:kw + s * (OW - 1) + 1:s] = dy * w[t]
    return buf[:, p:p + H, p:p + W]


def pixel_weights(shape, defect=None, PW=0, R=0, per=0):
    """[B, OH, OW, 1] multiplicity of each pixel in a reduction: 1, or the
    planted defects (a) drop the last column of every strip, (b) drop the first
    row of the second row chunk, (c) count the last row of the first block of
    `per` pixels twice."""
    B, OH, OW = shape
    wgt = np.ones((B, OH, OW, 1))
    if defect == "drop_col":
        wgt[:, :, PW - 1::PW] = 0.0
    elif defect == "drop_row":
        assert 0 < R < OH
        wgt[:, R] = 0.0
    elif defect == "dup_row":
        wgt.reshape(-1)[min(per, wgt.size) - 1] = 2.0
    return wgt


def dw_eval(c, d, sm=REF, defect=None, geom=None, want=None, act=None):
    """Every output of the depthwise training kernels for case c on data d, the
    sums taken by `sm`.  defect / geom: a planted defect and the kernel
    geometry it needs (PW, R, per).  want: restrict to these groups
    ("fwd", "fwdbn", "dgrad", "dgbn", "wgrad", "wgradbn").  act: the activation
    of the plain forward and of the fused BatchNorm backward (default: case_act)."""
    B, H, W, C, k, s = c.B, c.H, c.W, c.C, c.k, c.s
    kk = k * k
    OH, OW = out_size(H, k, s), out_size(W, k, s)
    act = act or case_act(c)
    geom = geom or {}
    want = want or ("fwd", "fwdbn", "dgrad", "dgbn", "wgrad", "wgradbn")
    x, w, dy, bias, bn = d["x"], d["w"], d["dy"], d["bias"], d["bn"]
    shift_tap = kk // 2 + 1 if defect == "shift_tap" else None
    red_def = defect if defect in ("drop_col", "drop_row", "dup_row") else None
    out = {}

    def skip(v):                                  # defect (e): channels 256.. never computed
        if defect == "skip_lane" and C > 256 and C % 256 == 4:
            v = v.copy()
            v[..., 256:] = np.nan
        return v

    def forward(xin, b, a, tag):
        tp = Taps(xin, k, s, shift_tap)
        nterm = kk + (1 if b is not None else 0)
        y = act_f(sm.taps(nterm, lambda i: tp.view(i) * w[i] if i < kk
                          else np.broadcast_to(b, tp.view(0).shape)), a)
        sh = y[0, 0, 0].copy()
        dd = (y - sh) * pixel_weights((B, OH, OW), red_def, **geom)
        out["y" + tag] = skip(y)
        out["shift" + tag] = skip(sh)
        out["S" + tag] = skip(sm.rows(dd.reshape(-1, C)))
        out["Q" + tag] = skip(sm.rows(((y - sh) * dd).reshape(-1, C)))

    if "fwd" in want:
        forward(x, bias, act, "")
    xa = act_f(bn_z(x, bn), "relu")               # the BN-input forms: relu(bn(x)) on load
    if "fwdbn" in want:
        forward(xa, None, "none", "b")
    if "dgrad" in want or "dgbn" in want:
        flip = defect == "flip_parity" and s == 2
        de = sm.taps(kk, lambda t: dgrad_term(dy, w, H, W, k, s, t, flip))
        if defect == "drop_col":
            de = de.copy()
            de[:, :, geom["PW"] - 1::geom["PW"]] = np.nan         # never stored
        out["dx"] = skip(de)
    if "dgbn" in want:
        xh = bn_xhat(x, bn)
        dz = de * act_d(bn_z(x, bn), act)
        wg = pixel_weights((B, H, W), defect if defect == "dup_row" else None, **geom)
        out["dz"] = skip(dz)
        out["dbeta"] = skip(sm.rows((dz * wg).reshape(-1, C)))
        out["dgamma"] = skip(sm.rows((dz * xh * wg).reshape(-1, C)))
    for key, xin in (("wgrad", x), ("wgradbn", xa)):
        if key in want:
            tp = Taps(xin, k, s, shift_tap)
            g = dy * pixel_weights((B, OH, OW), red_def, **geom)
            dw = np.stack([sm.rows((tp.view(t) * g).reshape(-1, C)) for t in range(kk)])
            out["dw" if key == "wgrad" else "dwb"] = skip(dw).T.copy()   # [C, kk]
    return out


ALL_GROUPS = ("fwd", "fwdbn", "dgrad", "dgbn", "wgrad", "wgradbn")
_GROUPS = {"chan": ALL_GROUPS, "spatial": ALL_GROUPS, "chan1024": ("fwd", "fwdbn"),
           "wgrows": ("wgrad", "wgradbn"), "fwdrows": ("fwd", "fwdbn"), "wgfall": ("wgrad",),
           "fwdfall": ("fwd", "fwdbn"), "fwdfall1": ("fwd",),   # (M = 8200: plain form only)
           "dgbnspb": ("dgbn",), "dgrows": ("dgbn",), "wgper": ("wgrad", "wgradbn"),
           "infer": ("fwd",)}


def case_groups(c):
    """The kernel families a case runs (dw_eval's `want`)."""
    return _GROUPS[c.group]


def dw_conditions(c, d, want=None):
    """The 2^24 condition of every exact output of dw_eval: {name: worst sum of
    absolute terms in units of its quantum}.  Plain operands are integers
    (q = 1); the BN-input taps relu(z), z = integer + 0.5, are multiples of
    0.5, dz under leaky(0.5) and xhat under invstd = 0.5 likewise."""
    B, H, W, C, k, s = c.B, c.H, c.W, c.C, c.k, c.s
    kk = k * k
    want = want or case_groups(c)
    x, w, dy, bias, bn = d["x"], d["w"], d["dy"], d["bias"], d["bn"]
    ref = dw_eval(c, d, want=want)
    res = {}
    xa = act_f(bn_z(x, bn), "relu")
    for nm in ("x", "w", "dy", "bias"):
        assert_quantum(nm, d[nm], 1.0)
        assert np.all(d[nm] != 0), nm
    assert_quantum("relu(bn(x))", xa, 0.5)
    assert not np.any(bn_z(x, bn) == 0.0), "a pre-activation on the kink"
    for tag, xin, q, b in (("", x, 1.0, bias), ("b", xa, 0.5, None)):
        tp = Taps(np.abs(xin), k, s)
        if "fwd" + ("bn" if tag else "") in want:
            ab = sum(tp.view(t) * np.abs(w[t]) for t in range(kk)) + (0 if b is None else np.abs(b))
            res["y" + tag] = assert_exact("y" + tag, ab, q)
            dd = ref["y" + tag] - ref["shift" + tag]
            res["S" + tag] = assert_exact("S" + tag, np.abs(dd).reshape(-1, C).sum(0), q)
            res["Q" + tag] = assert_exact("Q" + tag, (dd * dd).reshape(-1, C).sum(0), q * q)
        if "wgrad" + ("bn" if tag else "") in want:
            g = np.abs(dy)
            res["dw" + tag] = assert_exact(
                "dw" + tag, np.stack([(tp.view(t) * g).reshape(-1, C).sum(0) for t in range(kk)]), q)
    if "dgrad" in want or "dgbn" in want:
        ade = sum(dgrad_term(np.abs(dy), np.abs(w), H, W, k, s, t) for t in range(kk))
        res["dx"] = assert_exact("dx", ade)
    if "dgbn" in want:
        xh, dz = bn_xhat(x, bn), ref["dz"]
        assert_quantum("xhat", xh, 0.5)
        assert_quantum("dz", dz, 0.5)
        res["dbeta"] = assert_exact("dbeta", np.abs(dz).reshape(-1, C).sum(0), 0.5)
        res["dgamma"] = assert_exact("dgamma", np.abs(dz * xh).reshape(-1, C).sum(0), 0.25)
    return res


def bn_dx_ref(dz, xh, bn, sdz, sdzx, M):
    """dx of the BN backward in fp64 from the exact sums, and the elementwise
    bound on an fp32 evaluation of bn_bwd_apply_kernel's expression
        gamma * invstd * (dz - sdz / M - xhat * sdzx / M):
    1/M, the two products with it, xhat * a2, two subtractions, gamma * invstd
    and the final product are eight roundings of 2^-24 relative each, every
    one applied to a quantity no larger than the sum of the three magnitudes."""
    gi = bn.gamma * bn.invstd
    dx = gi * (dz - sdz / M - xh * sdzx / M)
    bound = 8.0 * 2.0 ** -24 * np.abs(gi) * (np.abs(dz) + np.abs(sdz) / M + np.abs(xh * sdzx) / M)
    return dx, bound


def bn_dx_f32(dz, xh, bn, sdz, sdzx, M):
    """bn_bwd_apply_kernel's expression evaluated in numpy fp32, op for op."""
    f = lambda v: np.asarray(v, dtype=F32)
    invM = F32(1.0) / F32(M)
    a1, a2 = f(sdz) * invM, f(sdzx) * invM
    return (f(bn.gamma) * f(bn.invstd)) * ((f(dz) - a1) - f(xh) * a2)


def ulp_dist(a, b):
    """Distance in fp32 units in the last place between a and b (rounded to fp32)."""
    def key(v):
        i = np.asarray(v, dtype=F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


# ------------------------------------------------------------ BatchNorm cases
BN_C = (4, 12, 72, 1024, 1028, 2048)


def bn_M_values(C):
    rp = bn_rows_pass(C)
    return tuple(sorted({2, max(rp - 1, 1), rp, rp + 1, 8 * rp + 1, 2053}))


BnCase = namedtuple("BnCase", "C M pad_ld")
BN_STATS_CASES = tuple(BnCase(C, M, p) for C in BN_C for M in bn_M_values(C) for p in (0, 8))


def bn_id(c):
    return "-".join(f"{k}{v}" for k, v in c._asdict().items())


BN_X_VALS = (-3, -2, -1, 1, 2, 3)
EPS = 1e-5


def bn_stats_data(c):
    rng = rng_for("bnstats", *c)
    x = ints(rng, (c.M, c.C), BN_X_VALS)
    x[:, 1] = 3.0                                 # a constant channel: var = 0 exactly
    return x


def bn_stats_sums(x, sm=REF, defect=None, per=0):
    """Shifted sums of bn_stats_part_kernel (shift = row 0)."""
    d = x - x[0]
    wgt = np.ones((x.shape[0], 1))
    if defect == "dup_row":           # the second block's: row 0 is the shift, its d is 0
        wgt[min(2 * per, x.shape[0]) - 1] = 2.0
    return sm.rows(d * wgt), sm.rows(d * d * wgt)


def bn_stats_ref(shift, S, Q, M, eps=EPS):
    """mean, invstd and the unbiased variance from the exact shifted sums, in
    bn_stats_final_kernel's fp64 expression (numpy longdouble where wider)."""
    L = np.longdouble
    ms = np.asarray(S, dtype=L) / L(M)
    var = np.maximum(np.asarray(Q, dtype=L) / L(M) - ms * ms, L(0))
    mean = np.asarray(shift, dtype=L) + ms
    invstd = L(1) / np.sqrt(var + L(F32(eps)))     # the ABI takes eps as a float
    unb = var * L(M) / L(M - 1) if M > 1 else var
    return mean.astype(F64), invstd.astype(F64), unb.astype(F64)


def running_ref(r0, new, momentum):
    """(1 - m) * r0 + m * new with the kernel's fp32 m and fp32 (1 - m), in fp64."""
    m = F32(momentum)
    return F64(F32(1.0) - m) * r0 + F64(m) * new


def running_start(mean):
    """Start values of the running mean with the sign of the batch mean, so
    the momentum blend adds two terms of one sign: no cancellation, and the
    2-ulp bar (1 ulp of the mean, the blend's own roundings) is meaningful."""
    return np.where(mean >= 0, 2.0, -2.0)


BnActCase = namedtuple("BnActCase", "C M act res yc0")


def _bn_act_cases():
    out = []
    for C in (12, 72, 260):
        full = 7 * ew_rows_pass(C)        # m0 + 7 * rows_pass < M is the "full block" test
        for i, M in enumerate((1, full, full + 1, 8 * ew_rows_pass(C) + 3)):
            for j, act in enumerate(("none", "relu", "leaky")):
                yc0 = 4 * ((i + j) % 2)               # res and no res at the same yc0:
                out.append(BnActCase(C, M, act, True, yc0))    # all four (res, yc0) pairs
                out.append(BnActCase(C, M, act, False, yc0))   # occur for every C
    return tuple(out)


BN_ACT_CASES = _bn_act_cases()

BnSumCase = namedtuple("BnSumCase", "C blocks act")
BN_SUM_CASES = tuple(BnSumCase(C, nb, act) for C in (12, 72, 256, 260)
                     for nb, act in ((1, "relu"), (3, "leaky"), (3, "none")))
BN_SUM_B = 3


def bn_act_data(key, M, C):
    rng = rng_for("bnact", *key)
    return dict(x=ints(rng, (M, C), BN_X_VALS), res=ints(rng, (M, C), X_VALS),
                bn=bn_params(rng, C, invstd=(0.5, 1.0, 2.0), gamma=(-4.0, -2.0, 2.0, 4.0)))


def bn_act_ref(d, act, res):
    return act_f(bn_z(d["x"], d["bn"], d["res"] if res else None), act)


BnBwdCase = namedtuple("BnBwdCase", "C M act res hw")   # hw = 0: no dy transform


def _bn_bwd_cases():
    out = []
    acts = ("relu", "leaky", "none")
    for ci, C in enumerate(BN_C):
        for mi, M in enumerate(bn_M_values(C)):
            out.append(BnBwdCase(C, M, acts[(ci + mi) % 3], (ci + mi) % 2 == 0, 0))
    # the dy transform: a thread's consecutive rows cross several images
    for C, M, hw in ((12, 2 * 85 * 3, 1), (12, 85 * 6, 3), (72, 64 * 9, 64), (1028, 192, 64),
                     (260, 9, 3), (2048, 12, 3)):
        assert M % hw == 0
        out.append(BnBwdCase(C, M, acts[M % 3], M % 2 == 0, hw))
    return tuple(out)


BN_BWD_CASES = _bn_bwd_cases()
BWD_DY_PAD, BWD_DYC0 = 8, 4          # lddy = C + 8, dy starts at column 4


def bn_bwd_data(c):
    rng = rng_for("bnbwd", *c)
    d = bn_act_data(("bwd",) + tuple(c), c.M, c.C)
    d["dy"] = ints(rng, (c.M, c.C), DY_VALS)
    if c.hw:
        nb = c.M // c.hw
        d["dys"] = ints(rng, (nb, c.C), (-2, -1, 1, 2))
        d["dya"] = ints(rng, (nb, c.C), (-1, 1))
    return d


def bn_bwd_eval(c, d, sm=REF, defect=None):
    """dz, the exact sums, and (fp64 only) dx with its bound."""
    bn = d["bn"]
    g = d["dy"]
    if c.hw:
        img = np.arange(c.M) // c.hw
        g = g * d["dys"][img] + d["dya"][img]
    xh = bn_xhat(d["x"], bn)
    z = bn_z(d["x"], bn, d["res"] if c.res else None)
    dz = g * act_d(z, c.act)
    wgt = np.ones((c.M, 1))
    if defect == "dup_row":
        wgt[min(bn_rows_per_blk(c.M, c.C), c.M) - 1] = 2.0
    out = dict(dz=dz, xh=xh, z=z, dbeta=sm.rows(dz * wgt), dgamma=sm.rows(dz * xh * wgt))
    if defect == "skip_lane" and c.C > 1024:
        out["dbeta"][1024:] = np.nan
        out["dgamma"][1024:] = np.nan
    return out


def bn_bwd_conditions(c, d):
    e = bn_bwd_eval(c, d)
    q = min(np.min(d["bn"].invstd), 1.0)          # xhat's quantum
    assert_quantum("xhat", e["xh"], q)
    assert_quantum("dz", e["dz"], 0.5)
    assert not np.any(e["z"] == 0.0), "a pre-activation on the kink"
    return dict(dbeta=assert_exact("dbeta", np.abs(e["dz"]).sum(0), 0.5),
                dgamma=assert_exact("dgamma", np.abs(e["dz"] * e["xh"]).sum(0), 0.5 * q))
