"""References, inputs, guarded buffers and case tables for the edge tests of the
kernels that write the detector's outputs (tests/test_head_writers_edges.py):
heads_kernel, heads_scatter_kernel and channel_sum_kernel (csrc/head.hip),
heads_gather_kernel (csrc/train.hip) and ssh_tail_heads_kernel (csrc/ssh.hip).
Test infrastructure only; everything here runs on the CPU.

Layout (nets/retinaface_r.py:335-343): a level's 32 head channels per position
are 8 bbox | 4 class | 20 landmark (engine.heads_pack's order); position p of
image b owns rows a_off + 2p and a_off + 2p + 1 of loc [B, A, 4], conf
[B, A, 2] and landm [B, A, 10].  write_level() is that as index arithmetic,
layout_permute() as the reference model's conv1x1 -> permute(0, 2, 3, 1) ->
view(B, -1, k) -> cat.

Guarded: an output buffer with at least GUARD_ROWS sentinel rows in front of
every owed range and behind it (in front of the first image, between a_off +
2 HW and the next image's a_off, behind the last image).  Owed rows start as
NaN and must come back finite; every other element must come back bit-identical.

*_emulate(): honest fp32 evaluations (torch on the CPU) that write through the
same write_level(), with one of DEFECTS planted on request, so the CPU
self-checks can show which cases catch which defect.
"""
import collections
import copy
import functools
import math

import torch
import torch.nn.functional as tF

U = 2.0 ** -24            # fp32 unit roundoff
GUARD_ROWS = 128          # two waves of positions
SENTINEL = 12345.6789
A_OFF_SMALL, A_OFF_BIG = 6, 130   # the positive even anchor offsets of the tables

# 4x the worst |torch-fp32 CPU softmax - fp64 softmax| over the exact fp32
# logits of every heads / scatter case (8.64e-8, 1.4 ulps of a probability in
# [0.5, 1)); test_softmax_term_is_four_times_the_measured_error re-measures it
SOFTMAX_R = 3.5e-7

HEAD_DEFECTS = ("swap_anchors",    # the position's two anchors exchanged
                "shift_rows",      # rows a_off + 2p + 2 (one position late)
                "wrong_pair")      # softmax over (c0, c2) and (c1, c3)
SSH_DEFECTS = ("u_outside",        # conv7X7_2 evaluated outside the image, not zero
               "halo1",            # only a 1-pixel t halo around the tile
               "frag12")           # conv7x7_3's head weights read at 20 + 12, not 20 + 10
CSUM_DEFECTS = ("drop_last_group",  # the last row group never added
                "floor_per")        # pixels per block floor(HW / nblk), not ceil


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    """randn drawn in float64 and rounded to float32.  torch's float32 normal
    sampler is vectorised differently per CPU (AVX2 / AVX-512) and its draws
    differ in the last bits from one machine to the next; the float64 one is
    scalar libm code.  The bars taken from an fp32 CPU evaluation of these
    inputs, and the checks against a quarter of them, need the same inputs
    everywhere."""
    return torch.randn(*shape, generator=g, dtype=torch.float64).float()


def _rand(g, *shape):
    return torch.rand(*shape, generator=g, dtype=torch.float64).float()


# ============================================================ guarded buffers
class Guarded:
    """[B, A, k] float32 on `dev` inside one flat allocation with GUARD_ROWS
    sentinel rows before and after; rows [a_off, a_off + n) of every image are
    owed (NaN), the rest sentinel.  .view is what the kernel gets."""

    def __init__(self, B, A, k, a_off, n, dev="cpu"):
        assert a_off >= 0 and n > 0 and A - (a_off + n) >= GUARD_ROWS
        self.B, self.A, self.k, self.a_off, self.n = B, A, k, a_off, n
        g = GUARD_ROWS
        self.rows = torch.full((g + B * A + g, k), SENTINEL, dtype=torch.float32, device=dev)
        self.view = self.rows[g:g + B * A].view(B, A, k)
        self.view[:, a_off:a_off + n] = float("nan")
        mask = torch.zeros(g + B * A + g, dtype=torch.bool)
        mask[g:g + B * A].view(B, A)[:, a_off:a_off + n] = True
        self.mask = mask

    def owed(self):
        return self.view[:, self.a_off:self.a_off + self.n]

    def problems(self, name):
        """[] when every owed element is finite and every other one still holds
        the sentinel's bits; else what is wrong and at which row (counted from
        image 0's row 0, so a negative row is in the front guard)."""
        rows = self.rows.detach().cpu()
        want = torch.full((self.k,), SENTINEL, dtype=torch.float32).view(torch.int32)
        touched = (rows.view(torch.int32) != want).any(1) & ~self.mask
        unwritten = (~torch.isfinite(rows)).any(1) & self.mask
        out = []
        for what, m in (("written outside its rows", touched),
                        ("owed but unwritten or non-finite", unwritten)):
            if bool(m.any()):
                first = int(m.nonzero()[0]) - GUARD_ROWS
                out.append(f"{name}: {int(m.sum())} rows {what}, first at image "
                           f"{first // self.A} row {first % self.A}")
        return out


def guarded_level(B, HW, a_off, dev="cpu"):
    """loc / conf / landm for one level of HW positions at a_off; A = a_off +
    2 HW + GUARD_ROWS, so every image ends in a guard."""
    A = a_off + 2 * HW + GUARD_ROWS
    return {n: Guarded(B, A, k, a_off, 2 * HW, dev) for n, k in (("loc", 4), ("conf", 2), ("landm", 10))}


def guarded_flat(rows, k, dev="cpu"):
    """A dense [rows, k] output with guards on both sides."""
    return Guarded(1, rows + GUARD_ROWS, k, 0, rows, dev)


# ==================================================================== layout
def level_rows(HW, a_off, defect=None):
    """rows[p, j]: the row of anchor j of position p."""
    p = torch.arange(HW).view(HW, 1)
    j = torch.arange(2).view(1, 2)
    if defect == "swap_anchors":
        j = 1 - j
    return a_off + 2 * p + j + (2 if defect == "shift_rows" else 0)


def pair_softmax(c, defect=None):
    """c [..., 4] = the class logits (a0c0, a0c1, a1c0, a1c1) of one position:
    F.softmax over each anchor's two."""
    p, dim = c.unflatten(-1, (2, 2)), (-2 if defect == "wrong_pair" else -1)
    if c.dtype == torch.float32:
        # the honest fp32 form, the same numbers on every CPU: exp through
        # float64 (correctly rounded), the subtract, add and divide in fp32
        e = torch.exp((p - p.amax(dim, keepdim=True)).double()).float()
        return (e / e.sum(dim, keepdim=True)).flatten(-2)
    return torch.softmax(p, dim).flatten(-2)


def write_level(o, loc, conf, landm, a_off, softmax, defect=None):
    """o [B, HW, 32] -> the level's rows of loc / conf / landm [B, A, k], by
    index arithmetic: row a_off + 2p + j gets loc o[4j : 4j + 4], conf
    o[8 + 2j : 10 + 2j], landm o[12 + 10j : 22 + 10j]."""
    B, HW, _ = o.shape
    rows = level_rows(HW, a_off, defect)
    cls = o[..., 8:12]
    if softmax:
        cls = pair_softmax(cls, defect)
    for j in range(2):
        r = rows[:, j]
        for i in range(4):
            loc[:, r, i] = o[:, :, 4 * j + i]
        for i in range(2):
            conf[:, r, i] = cls[:, :, 2 * j + i]
        for i in range(10):
            landm[:, r, i] = o[:, :, 12 + 10 * j + i]


def layout_index(o, softmax=False):
    """write_level into dense [B, 2 HW, k] tensors of o's dtype."""
    B, HW, _ = o.shape
    out = [torch.zeros(B, 2 * HW, k, dtype=o.dtype) for k in (4, 2, 10)]
    write_level(o, *out, 0, softmax)
    return dict(zip(("loc", "conf", "landm"), out))


def layout_permute(levels, softmax=False):
    """The reference model's form for a list of NCHW head maps [B, 32, h, w]:
    per head permute(0, 2, 3, 1).view(B, -1, k), cat over levels, softmax(-1)."""
    B = levels[0].shape[0]
    loc = torch.cat([o[:, 0:8].permute(0, 2, 3, 1).contiguous().view(B, -1, 4) for o in levels], 1)
    conf = torch.cat([o[:, 8:12].permute(0, 2, 3, 1).contiguous().view(B, -1, 2) for o in levels], 1)
    landm = torch.cat([o[:, 12:32].permute(0, 2, 3, 1).contiguous().view(B, -1, 10) for o in levels], 1)
    if softmax:
        conf = torch.softmax(conf, -1)
    return {"loc": loc, "conf": conf, "landm": landm}


def gather_rows(gl, gc, glm, HW, a_off):
    """The inverse of write_level: [B, A, k] x 3 -> [B, HW, 32]."""
    rows = level_rows(HW, a_off)
    parts = [g[:, rows[:, j]] for g in (gl, gc, glm) for j in range(2)]
    return torch.cat(parts, -1)


# ===================================================================== heads
HeadsCase = collections.namedtuple("HeadsCase", "name HW C B a_off softmax kind seed")
HEADS_HW = (1, 63, 64, 65, 255, 256, 257, 300, 400)
HEADS_C = (4, 36, 40, 64, 256)
VIEW_PS, VIEW_OFF, VIEW_EXTRA = 48, 4, 3   # the view case: 40 of 48 channels, 3 pixels past HW


def _heads_cases():
    c = []
    offs = (0, A_OFF_SMALL, A_OFF_BIG)
    for i, HW in enumerate(HEADS_HW):                     # every HW at C = 40
        c.append(HeadsCase(f"hw{HW}", HW, 40, (1, 3)[i % 2], offs[i % 3], i % 3 != 1, "plain", 10 + i))
    for i, (C, HW) in enumerate(((4, 65), (36, 257), (64, 63), (256, 300))):
        c.append(HeadsCase(f"c{C}-hw{HW}", HW, C, (3, 1)[i % 2], offs[(i + 1) % 3], i != 2, "plain", 30 + i))
    c.append(HeadsCase("view-hw257", 257, 40, 3, A_OFF_SMALL, True, "view", 40))
    c.append(HeadsCase("saturated-hw300", 300, 40, 3, 0, True, "saturated", 41))
    return tuple(c)


HEADS_CASES = _heads_cases()


def case_id(c):
    return c.name


@functools.lru_cache(maxsize=None)
def heads_inputs(case):
    """x [B, HW, C], W [32, C], b [32] as fp32 CPU tensors; read-only.
    saturated: positive x and class rows (+s w, -s w, +2s w, -2s w) with w > 0
    and s such that each anchor's two logits differ by more than 100 at every
    position (the truth is (1, 0, 1, 0); the pairs (c0, c2), (c1, c3) give
    (0, 0, 1, 1)).
    C = 4: x, W and b are rounded to multiples of 2^-5 / 2^-5 / 2^-10, so every
    product and partial sum is exact in fp32 in any order.  The bar is
    6 * 2^-24 * sum|terms| there and a plain fp32 sum of 4 rounded products and
    a bias reaches 2.7 of those 6 on some of a few thousand elements, over the
    quarter the self-checks ask for; with exact sums any device error at C = 4
    is a wrong operand, not rounding."""
    g = _gen(case.seed)
    x = _randn(g, case.B, case.HW, case.C)
    W = _randn(g, 32, case.C) / math.sqrt(case.C)
    b = 0.1 * _randn(g, 32)
    if case.kind == "saturated":
        x = x.abs() + 0.5
        w = (_rand(g, case.C) + 0.5) / case.C
        s = 101.0 / (2.0 * float((x.double() @ w.double()).min()))
        for n, f in ((8, 1.0), (9, -1.0), (10, 2.0), (11, -2.0)):
            W[n] = (f * s * w.double()).float()
    if case.C == 4:
        x, W, b = (torch.round(v * 2.0 ** k) / 2.0 ** k for v, k in ((x, 5), (W, 5), (b, 10)))
    return x.contiguous(), W.contiguous(), b.contiguous()


def heads_view_buffer(case, x):
    """x inside a [B, HW + 3, 48] buffer at channel 4, NaN everywhere else.
    Returns the buffer and (float offset of the view, x_bs, x_ps)."""
    buf = torch.full((case.B, case.HW + VIEW_EXTRA, VIEW_PS), float("nan"))
    buf[:, :case.HW, VIEW_OFF:VIEW_OFF + case.C] = x
    return buf, (VIEW_OFF, (case.HW + VIEW_EXTRA) * VIEW_PS, VIEW_PS)


def heads_logits(x, W, b, dtype=torch.float64):
    """o = x @ W.T + b in `dtype`, [B, HW, 32]."""
    return x.to(dtype) @ W.to(dtype).T + b.to(dtype)


@functools.lru_cache(maxsize=None)
def heads_ref(case):
    """fp64 reference rows [B, 2 HW, k] and the per-element bars.  Logits:
    (C + 2) 2^-24 (|b_n| + sum_c |W_nc x_c|), the worst case of an fp32 dot
    product of C terms plus a bias in any order, with or without FMA.
    Softmax: 0.25 (d0 + d1) + SOFTMAX_R, d the pair's two logit bars
    (|dp/dl| = p (1 - p) <= 1/4)."""
    x, W, b = heads_inputs(case)
    o = heads_logits(x, W, b)
    bound = (case.C + 2) * U * (x.double().abs() @ W.double().abs().T + b.double().abs())
    ref = layout_index(o, case.softmax)
    bar = layout_index(bound)
    if case.softmax:
        bar["conf"] = (0.25 * bar["conf"].sum(-1, keepdim=True) + SOFTMAX_R).expand(-1, -1, 2)
    return {"o": o, "ref": ref, "bar": bar}


def heads_emulate(case, defect=None):
    """Honest fp32: torch's x @ W.T + b on the CPU, written through
    write_level into guarded buffers."""
    x, W, b = heads_inputs(case)
    gl = guarded_level(case.B, case.HW, case.a_off)
    write_level(heads_logits(x, W, b, torch.float32), gl["loc"].view, gl["conf"].view,
                gl["landm"].view, case.a_off, case.softmax, defect)
    return gl


def bar_check(gl, ref, bar, frac=1.0):
    """Problems of guarded outputs against fp64 rows under per-element bars
    (scaled by frac); the worst err / bar ratio per tensor is returned too."""
    probs, worst = [], {}
    for n in ("loc", "conf", "landm"):
        probs += gl[n].problems(n)
        got = gl[n].owed().detach().cpu().double()
        err = (got - ref[n]).abs()
        ok = err <= frac * bar[n]              # False for NaN
        ratio = torch.where(torch.isfinite(err), err / bar[n], torch.full_like(err, math.inf))
        worst[n] = float(ratio.max())
        if not bool(ok.all()):
            i = int((~ok).flatten().nonzero()[0])
            probs.append(f"{n}: {int((~ok).sum())} elements over the bar, first flat index {i}: "
                         f"got {float(got.flatten()[i])!r} ref {float(ref[n].flatten()[i])!r} "
                         f"bar {frac * float(bar[n].flatten()[i]):.3e}")
    return probs, worst


# ------------------------------------------------------------------- scatter
ScatterCase = collections.namedtuple("ScatterCase", "name HW B a_off softmax kind seed")


def _scatter_cases():
    c = []
    offs = (A_OFF_SMALL, 0, A_OFF_BIG)
    kinds = ("plain", "saturated", "equal")
    for i, HW in enumerate(HEADS_HW):
        kind = kinds[i % 3]
        c.append(ScatterCase(f"{kind}-hw{HW}", HW, (3, 1)[i % 2], offs[i % 3],
                             kind != "plain" or i % 2 == 0, kind, 50 + i))
    return tuple(c)


SCATTER_CASES = _scatter_cases()


@functools.lru_cache(maxsize=None)
def scatter_inputs(case):
    """y [B, HW, 32] fp32.  saturated: each anchor's logits 150 / 120 apart;
    equal: each anchor's two logits the same number."""
    y = _randn(_gen(case.seed), case.B, case.HW, 32)
    if case.kind == "saturated":
        y[..., 8] = y[..., 9] + 150.0
        y[..., 10] = y[..., 11] - 120.0
    elif case.kind == "equal":
        y[..., 8] = y[..., 9]
        y[..., 10] = y[..., 11]
    return y.contiguous()


def scatter_check(case, gl):
    """loc / landm (and conf with the softmax off) bit-identical to y's
    slices; conf with the softmax on within SOFTMAX_R of fp64."""
    y = scatter_inputs(case)
    exact = layout_index(y)
    probs = []
    for n in ("loc", "conf", "landm"):
        probs += gl[n].problems(n)
        got = gl[n].owed().detach().cpu()
        if n == "conf" and case.softmax:
            ref = layout_index(y.double(), True)["conf"]
            err = (got.double() - ref).abs()
            if not bool((err <= SOFTMAX_R).all()):
                probs.append(f"conf: softmax off by {float(err.nan_to_num(math.inf).max()):.3e}")
        elif not torch.equal(got.view(torch.int32), exact[n].view(torch.int32)):
            probs.append(f"{n}: not bit-identical to y's slice")
    return probs


def scatter_emulate(case, defect=None):
    gl = guarded_level(case.B, case.HW, case.a_off)
    write_level(scatter_inputs(case), gl["loc"].view, gl["conf"].view, gl["landm"].view,
                case.a_off, case.softmax, defect)
    return gl


# -------------------------------------------------------------------- gather
GatherCase = collections.namedtuple("GatherCase", "name HW B a_off seed")
GATHER_CASES = tuple(GatherCase(f"hw{HW}", HW, (1, 3)[i % 2], (0, A_OFF_BIG, A_OFF_SMALL)[i % 3], 70 + i)
                     for i, HW in enumerate(HEADS_HW))
GATHER_TAIL = 14   # rows behind the level, so A > a_off + 2 HW


@functools.lru_cache(maxsize=None)
def gather_inputs(case):
    """d(loc), d(conf), d(landm) [B, A, k] with random values in every row, the
    level's and the others', and the expected [B, HW, 32]."""
    A = case.a_off + 2 * case.HW + GATHER_TAIL
    g = _gen(case.seed)
    gl, gc, glm = (_randn(g, case.B, A, k) for k in (4, 2, 10))
    return gl, gc, glm, gather_rows(gl, gc, glm, case.HW, case.a_off)


# ================================================================== SSH tail
SshCase = collections.namedtuple("SshCase", "name H W B view a_off softmax seed")
SSH_HW = ((1, 1), (3, 4), (7, 31), (8, 32), (9, 33), (17, 65), (20, 20), (1, 70), (40, 1))
SSH_TH, SSH_TW = 8, 32
SSH_REL_BAR = 2e-5      # tests/test_ssh_tail.py's bar, here per tensor and per image
# _util.elem_rel_err (floor 1e-2) per tensor and image: 4x the worst value a
# torch-fp32 CPU evaluation of the same graph (ssh_graph in float32: conv_taps,
# pair_softmax) gives against fp64 over SSH_CASES
# (the measured values are in test_head_writers_edges.py's docstring), rounded up
# in the second digit
SSH_ELEM_BAR = {"loc": 6.3e-5, "conf_logits": 5.2e-5, "conf_softmax": 2.7e-6, "landm": 5.3e-5}


def _ssh_cases():
    c = []
    offs = (0, A_OFF_SMALL, A_OFF_BIG)
    for i, (H, W) in enumerate(SSH_HW):
        c.append(SshCase(f"{H}x{W}", H, W, (1, 3)[i % 2], i % 2 == 1 or i >= 6, offs[i % 3],
                         i % 4 != 1, 90 + i))
    return tuple(c)


SSH_CASES = _ssh_cases()


def ssh_group(case, n):
    return n if n != "conf" else ("conf_softmax" if case.softmax else "conf_logits")


def _ssh_module(seed):
    """SSH(40, 40) after _util.init_for_parity, whose draws are made in float64
    here (see _randn) and rounded by its copy_ into the float32 parameters."""
    from _util import init_for_parity
    from nets.layers import SSH
    ssh = SSH(40, 40)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        init_for_parity(ssh, seed=seed)
    finally:
        torch.set_default_dtype(prev)
    assert all(p.dtype == torch.float32 for p in ssh.parameters())
    return ssh.eval()


@functools.lru_cache(maxsize=None)
def ssh_inputs(case):
    """The SSH(40, 40), the head weights (Wh [32, 40], bh), c33 = relu(randn)
    [B, H, W, 20] (what the level's first GEMM hands over) and t [B, H, W, 12]
    (10 channels of either sign + the 2 zero pad channels)."""
    g = _gen(case.seed)
    ssh = _ssh_module(case.seed)
    Wh = (_randn(g, 32, 40) / math.sqrt(40.0)).contiguous()
    bh = (0.1 * _randn(g, 32)).contiguous()
    c33 = torch.relu(_randn(g, case.B, case.H, case.W, 20)).contiguous()
    t = torch.zeros(case.B, case.H, case.W, 12)
    t[..., :10] = _randn(g, case.B, case.H, case.W, 10)
    return {"ssh": ssh, "Wh": Wh, "bh": bh, "c33": c33, "t": t}


def ssh_c33_buffer(case, c33):
    """c33 as the first 20 channels of a 32-channel tensor, the other 12 NaN."""
    buf = torch.full((case.B, case.H, case.W, 32), float("nan"))
    buf[..., :20] = c33
    return buf


def ssh_folded(ssh, dtype=torch.float64):
    """{name: (w [10, 10, 3, 3], b [10])} of conv5X5_2, conv7X7_2, conv7x7_3
    with the eval BatchNorm folded by hand in `dtype`."""
    out = {}
    for name in ("conv5X5_2", "conv7X7_2", "conv7x7_3"):
        conv, bn = getattr(ssh, name)[0], getattr(ssh, name)[1]
        # the square root through float64 (correctly rounded): torch's float32
        # sqrt is not the same bits on every CPU
        var = bn.running_var.to(dtype) + bn.eps
        s = bn.weight.detach().to(dtype) / torch.sqrt(var.double()).to(dtype)
        out[name] = (conv.weight.detach().to(dtype) * s[:, None, None, None],
                     bn.bias.detach().to(dtype) - bn.running_mean.to(dtype) * s)
    return out


def _nchw(a):
    return a.permute(0, 3, 1, 2).contiguous()


def conv_taps(x, w, b, pad=0):
    """conv2d (stride 1, zero padding) as bias + one product per (kh, kw,
    channel) added in that order, each a separate elementwise multiply and add.
    torch's conv2d and matmul pick their blocking and FMA use by thread count
    and CPU, and their fp32 results move by 15 % of their error with them;
    IEEE multiplies and adds give the same numbers everywhere, which bars taken
    from an fp32 evaluation need."""
    k = w.shape[-1]
    xp = tF.pad(x, (pad, pad, pad, pad))
    H, W = xp.shape[2] - k + 1, xp.shape[3] - k + 1
    out = b.view(1, -1, 1, 1).expand(x.shape[0], -1, H, W)
    for kh in range(k):
        for kw in range(k):
            xs = xp[:, :, kh:kh + H, kw:kw + W]
            for c in range(x.shape[1]):
                out = out + xs[:, c:c + 1] * w[:, c, kh, kw].view(1, -1, 1, 1)
    return out


def ssh_features(inp, dtype=torch.float64):
    """f = relu(cat[c33, c52, c73]) [B, 40, H, W] in `dtype`, BN folded by hand:
    u = leaky(conv3x3(t) + b72) and c73 = conv3x3(u) + b73, both zero padded."""
    fw = ssh_folded(inp["ssh"], dtype)
    t = _nchw(inp["t"][..., :10]).to(dtype)
    u = tF.leaky_relu(conv_taps(t, *fw["conv7X7_2"], pad=1), inp["ssh"].leaky)
    c52 = conv_taps(t, *fw["conv5X5_2"], pad=1)
    c73 = conv_taps(u, *fw["conv7x7_3"], pad=1)
    return torch.relu(torch.cat([_nchw(inp["c33"]).to(dtype), c52, c73], 1))


def ssh_graph(inp, dtype=torch.float64):
    """The tail + heads in `dtype`: o [B, 32, H, W]."""
    return conv_taps(ssh_features(inp, dtype), inp["Wh"].to(dtype).view(32, 40, 1, 1),
                     inp["bh"].to(dtype))


def ssh_graph_from_modules(inp):
    """The same feature map f from the SSH module's own submodules (torch's
    Conv2d / BatchNorm2d forwards of a .double().eval() copy, no folding)."""
    ssh = copy.deepcopy(inp["ssh"]).double().eval()

    def cb(name, x):
        seq = getattr(ssh, name)
        return torch.nn.BatchNorm2d.forward(seq[1], torch.nn.Conv2d.forward(seq[0], x))

    with torch.no_grad():
        t = _nchw(inp["t"][..., :10]).double()
        u = tF.leaky_relu(cb("conv7X7_2", t), ssh.leaky)
        return torch.relu(torch.cat([_nchw(inp["c33"]).double(), cb("conv5X5_2", t),
                                     cb("conv7x7_3", u)], 1))


@functools.lru_cache(maxsize=None)
def ssh_ref(case):
    """fp64 rows [B, 2 HW, k] of the case."""
    with torch.no_grad():
        o = ssh_graph(ssh_inputs(case))
    return layout_permute([o], case.softmax)


def _o_rows(o_nchw):
    B = o_nchw.shape[0]
    return o_nchw.permute(0, 2, 3, 1).reshape(B, -1, 32)


def ssh_emulate(case, defect=None):
    """Honest fp32 on the CPU into guarded buffers.  Without a defect it is
    ssh_graph in float32 (BN folded in float32, as the pack does).  With one
    (or "tiled", the same without a defect) it is evaluated as the kernel
    does, tile by tile: 8 x 32 outputs, t with a 2-pixel halo that is zero
    outside the image, u on the tile + 1 pixel and zero outside the image."""
    inp = ssh_inputs(case)
    with torch.no_grad():
        if defect is None:
            o = ssh_graph(inp, torch.float32)
        else:
            o = _ssh_tiled(case, inp, defect)
    gl = guarded_level(case.B, case.H * case.W, case.a_off)
    write_level(_o_rows(o), gl["loc"].view, gl["conf"].view, gl["landm"].view, case.a_off,
                case.softmax)
    return gl


def _ssh_tiled(case, inp, defect):
    assert defect in SSH_DEFECTS + ("tiled",)
    B, H, W = case.B, case.H, case.W
    fw = ssh_folded(inp["ssh"], torch.float32)
    Wh = inp["Wh"].clone()
    if defect == "frag12":
        k = torch.arange(10)
        Wh[:, 30 + k] = inp["Wh"][:, (32 + k).clamp(max=39)]
    t = _nchw(inp["t"][..., :10])
    c33 = _nchw(inp["c33"])
    o = torch.zeros(B, 32, H, W)
    for oy0 in range(0, H, SSH_TH):
        for ox0 in range(0, W, SSH_TW):
            r0 = torch.zeros(B, 10, SSH_TH + 4, SSH_TW + 4)
            ys, xs = torch.arange(oy0 - 2, oy0 + SSH_TH + 2), torch.arange(ox0 - 2, ox0 + SSH_TW + 2)
            yi, xi = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
            if defect == "halo1":
                yi[0] = yi[-1] = xi[0] = xi[-1] = False
            r0[:, :, yi.nonzero()[:, None, 0], xi.nonzero()[None, :, 0]] = \
                t[:, :, ys[yi][:, None], xs[xi][None, :]]
            r1 = tF.leaky_relu(conv_taps(r0, *fw["conv7X7_2"]), inp["ssh"].leaky)
            if defect != "u_outside":
                yo, xo = ys[1:-1], xs[1:-1]
                inside = ((yo >= 0) & (yo < H))[:, None] & ((xo >= 0) & (xo < W))[None, :]
                r1 = r1 * inside
            c52 = conv_taps(r0[:, :, 1:-1, 1:-1], *fw["conv5X5_2"])
            c73 = conv_taps(r1, *fw["conv7x7_3"])
            th, tw = min(SSH_TH, H - oy0), min(SSH_TW, W - ox0)
            f = torch.relu(torch.cat([c33[:, :, oy0:oy0 + th, ox0:ox0 + tw], c52[:, :, :th, :tw],
                                      c73[:, :, :th, :tw]], 1))
            o[:, :, oy0:oy0 + th, ox0:ox0 + tw] = conv_taps(f, Wh.view(32, 40, 1, 1), inp["bh"])
    return o


def ssh_errors(case, gl, ref):
    """Guard problems and {group: (worst max-norm relative error, worst
    _util.elem_rel_err)} over the images, each tensor on its own."""
    from _util import elem_rel_err, rel_err
    probs, errs = [], {}
    for n in ("loc", "conf", "landm"):
        probs += gl[n].problems(n)
        got = gl[n].owed().detach().cpu()
        rel = elem = 0.0
        for b in range(case.B):
            if not bool(torch.isfinite(got[b]).all()):
                rel = elem = math.inf
                continue
            rel = max(rel, rel_err(got[b], ref[n][b]))
            elem = max(elem, elem_rel_err(got[b], ref[n][b]))
        errs[ssh_group(case, n)] = (rel, elem)
    return probs, errs


def ssh_check(case, gl, frac=1.0):
    """Problems of guarded outputs against the fp64 rows: guards, max-norm
    relative error <= 2e-5, elem_rel_err <= SSH_ELEM_BAR (both scaled by frac)."""
    probs, errs = ssh_errors(case, gl, ssh_ref(case))
    for grp, (rel, elem) in errs.items():
        if not rel <= frac * SSH_REL_BAR:
            probs.append(f"{grp}: max-norm relative error {rel:.3e} > {frac * SSH_REL_BAR:.3e}")
        if not elem <= frac * SSH_ELEM_BAR[grp]:
            probs.append(f"{grp}: elem_rel_err {elem:.3e} > {frac * SSH_ELEM_BAR[grp]:.3e}")
    return probs, errs


# =============================================================== channel sum
CsumCase = collections.namedtuple("CsumCase", "name C HW nblk B view seed")
CSUM_C = (4, 16, 40, 72, 100, 200, 250, 256, 260, 480, 960)
CSUM_HW = (1, 63, 256, 1000)
CSUM_NBLK = (1, 3, 64)
CSUM_THREADS = 256
CSUM_VIEW_PS, CSUM_VIEW_OFF = 96, 8


def _csum_cases():
    # Blocks of a few pixels leave little room between an honest fp32 sum and a
    # quarter of n u sum|x|: 3 roundings against a quarter of 4 u at HW = 256,
    # nblk = 64 (not in the table), and at HW = 1000, nblk = 64 (16 pixels, the
    # last block 8) torch's fp32 sum reaches 0.29 of the bar on one of 61 440
    # elements at C = 960 but 0.15 at C = 72, which is the case kept.  C >= 256
    # meets nblk = 64 at HW = 63, where the 64th block must be zeros.
    shapes = ((4, 1000, 3, 2), (16, 63, 64, 1), (40, 256, 1, 3), (72, 1000, 64, 1),
              (100, 63, 3, 2), (200, 256, 3, 1), (250, 1, 64, 2), (256, 1000, 1, 1),
              (260, 63, 1, 2), (480, 1, 3, 1), (960, 256, 3, 2), (16, 1, 1, 1),
              (960, 63, 64, 1), (128, 63, 3, 1))
    c = [CsumCase(f"c{C}-hw{HW}-n{n}", C, HW, n, B, False, 110 + i)
         for i, (C, HW, n, B) in enumerate(shapes)]
    c.append(CsumCase("view-c72-hw63-n3", 72, 63, 3, 2, True, 130))
    return tuple(c)


CSUM_CASES = _csum_cases()


@functools.lru_cache(maxsize=None)
def csum_inputs(case):
    """x [B, HW, C] fp32, randn."""
    return _randn(_gen(case.seed), case.B, case.HW, case.C).contiguous()


def csum_view_buffer(case, x):
    """x inside a [B, HW, 96] buffer at channel 8, NaN in the other channels."""
    buf = torch.full((case.B, case.HW, CSUM_VIEW_PS), float("nan"))
    buf[..., CSUM_VIEW_OFF:CSUM_VIEW_OFF + case.C] = x
    return buf


def csum_blocks(HW, nblk, floor=False):
    """[(first pixel, one past the last)] per block, per = ceil(HW / nblk)."""
    per = HW // nblk if floor else -(-HW // nblk)
    return [(min(b * per, HW), min(b * per + per, HW)) for b in range(nblk)]


@functools.lru_cache(maxsize=None)
def csum_ref(case):
    """part [B, nblk, C] in fp64 and the bar n 2^-24 sum|x| (n pixels in the
    block's range): the worst case of an fp32 sum of n numbers in any order.
    A block past the end is an exact 0 with a bar of 0."""
    x = csum_inputs(case).double()
    ref = torch.zeros(case.B, case.nblk, case.C, dtype=torch.float64)
    bar = torch.zeros_like(ref)
    for i, (p0, p1) in enumerate(csum_blocks(case.HW, case.nblk)):
        ref[:, i] = x[:, p0:p1].sum(1)
        bar[:, i] = (p1 - p0) * U * x[:, p0:p1].abs().sum(1)
    return ref, bar


def csum_emulate(case, defect=None):
    """fp32 as the kernel maps it: kSumThreads / C row groups for C < 256 (one
    otherwise), group r sums pixels p0 + r, p0 + r + rows, ...; the groups are
    then added in order."""
    x = csum_inputs(case)
    rows = CSUM_THREADS // case.C if case.C < CSUM_THREADS else 1
    rows = max(rows, 1)
    g = guarded_flat(case.B * case.nblk, case.C)
    part = g.owed().view(case.B, case.nblk, case.C)
    for i, (p0, p1) in enumerate(csum_blocks(case.HW, case.nblk, floor=defect == "floor_per")):
        t = torch.zeros(case.B, case.C)
        for r in range(rows - 1 if defect == "drop_last_group" else rows):
            t = t + x[:, p0 + r:p1:rows].sum(1)
        part[:, i] = t
    return g


def csum_check(case, g, frac=1.0):
    ref, bar = csum_ref(case)
    probs = g.problems("part")
    got = g.owed().detach().cpu().double().view(case.B, case.nblk, case.C)
    err = (got - ref).abs()
    ok = err <= frac * bar
    if not bool(ok.all()):
        bad = (~ok).nonzero()[0].tolist()
        probs.append(f"part: {int((~ok).sum())} elements over the bar, first (b, blk, c) = {bad}: "
                     f"got {float(got[tuple(bad)])!r} ref {float(ref[tuple(bad)])!r} "
                     f"bar {frac * float(bar[tuple(bad)]):.3e}")
    ratio = torch.where(bar > 0, err / bar.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    return probs, float(ratio.nan_to_num(math.inf).max())


# ================================================================ softmax term
@functools.lru_cache(maxsize=None)
def softmax_fp32_worst():
    """Worst |torch-fp32 softmax - fp64 softmax| over the exact fp32 logits of
    every heads and scatter case."""
    worst = 0.0
    for case in HEADS_CASES:
        worst = max(worst, _torch_softmax_err(heads_ref(case)["o"][..., 8:12].float()))
    for case in SCATTER_CASES:
        worst = max(worst, _torch_softmax_err(scatter_inputs(case)[..., 8:12]))
    return worst


def _torch_softmax_err(lg):
    p = lg.unflatten(-1, (2, 2))
    return float((torch.softmax(p, -1).double() - torch.softmax(p.double(), -1)).abs().max())
