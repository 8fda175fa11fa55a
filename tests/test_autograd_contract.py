"""The autograd contract of every hand-written training node.

The parity tests drive each torch.autograd.Function one way: one forward,
one backward, every input requiring a gradient, a dense contiguous incoming
gradient, a plain chain.  This file drives every node the other legal ways
and pins what must not change:

  purity        a backward leaves the incoming gradient, the inputs, the saved
                activations and the forward output bit-unchanged;
  re-entrancy   two backwards over one retained graph return equal gradients;
  layout        a permuted, a [::2]-strided and a stride-0 incoming gradient
                give the gradients of their contiguous copies;
  frozen sets   with only the activation inputs, only the parameters, or all
                but one parameter requiring a gradient, the gradients that
                remain are those of the all-on run and a frozen leaf's .grad
                stays None;
  unused outs   a multi-output node whose loss uses one output gives what
                explicit zeros for the others give;
  reference     the all-on contiguous case against an fp64 torch restatement
                of the op (and its fp32 run): relative Frobenius error
                <= max(1e-4, 4 x the fp32 restatement's own error), the rule of
                tests/test_train.py, with the HIP forward's activation masks
                replayed (tests/_kinks.py).

"Equal" is torch.equal: the training kernels use no atomics (partials are
combined in a fixed order), so every node is bit-reproducible run to run.

ROWS has one row per node (more where a node has distinct paths), at the
smallest shape the node is already tested at; test_every_node_has_a_row
fails when a Function is added without one.

What the rows found when they were written: R50BlockFn failed re-entrancy
and layout in all three of its rows (its backward consumed the bn3 link
record, so any second backward over a graph raised KeyError 'rows'); the
other 22 nodes passed every row as they stood.  The link's other faults
(a second consumer, retain_grad) need a chain and live in
tests/test_train.py::test_train_r50_bn3_link.
"""
import collections
import inspect

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as tF

from _kinks import Kinks
from _util import init_for_parity
from oracle import model_ref

pytestmark = pytest.mark.gpu

NODE_MODULES = ("jabd_amd.train", "jabd_amd.modules", "jabd_amd.ops", "jabd_amd.parallel")


def _c2(t):   # NHWC -> NCHW view
    return t.permute(0, 3, 1, 2)


def _c4(t):   # NCHW -> NHWC view
    return t.permute(0, 2, 3, 1)


def _rand(g, *shape, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=g) * scale + shift


class Case:
    """leaves: name -> GPU leaf (requires_grad toggled by the checks);
    acts: names of the activation inputs (the rest are parameters);
    call(L) -> HIP output(s); ref(L) -> the same from CPU leaves of any dtype;
    zero: leaves whose gradient is analytically zero (rounding noise only)."""

    def __init__(self, node, leaves, acts, call, ref, zero=()):
        self.node, self.leaves, self.acts = node, leaves, tuple(acts)
        self.call, self.ref, self.zero = call, ref, set(zero)
        self.params = tuple(k for k in leaves if k not in self.acts)

    def run(self):
        o = self.call(self.leaves)
        return list(o) if isinstance(o, (tuple, list)) else [o]

    def require(self, on):
        for k, t in self.leaves.items():
            t.requires_grad_(k in on)
            t.grad = None


def _leaf(t, dev, param=False):
    t = t.to(dev)
    return nn.Parameter(t) if param else t.requires_grad_(True)


# ----------------------------------------------------------------------------- rows
def _conv(dev, cin, cout, k, h, bias):
    from jabd_amd.train import ConvFn
    g = torch.Generator().manual_seed(cin + k)
    L = collections.OrderedDict(
        x=_leaf(_rand(g, 2, h, h + 1, cin), dev),
        w=_leaf(_rand(g, cout, cin, k, k) / (cin * k * k) ** 0.5, dev, True))
    if bias:
        L["b"] = _leaf(_rand(g, cout) * 0.1, dev, True)
    return Case(ConvFn, L, ["x"],
                lambda L: ConvFn.apply(L["x"], L["w"], L.get("b"), 1, k // 2, False),
                lambda L: _c4(tF.conv2d(_c2(L["x"]), L["w"], L.get("b"), 1, k // 2)))


def _ecaconv(dev):
    from jabd_amd.train import EcaConvFn
    c, h = 40, 8
    ke = model_ref.eca_kernel_size(c)
    g = torch.Generator().manual_seed(c)
    L = collections.OrderedDict(
        x=_leaf(_rand(g, 2, h, h, c), dev), w1=_leaf(_rand(g, 1, 1, ke), dev, True),
        w=_leaf(_rand(g, c, c, 1, 1) / c ** 0.5, dev, True))

    def ref(L):
        x = _c2(L["x"])
        z = tF.conv1d(x.mean(dim=(2, 3)).unsqueeze(1), L["w1"], padding=(ke - 1) // 2).squeeze(1)
        return _c4(tF.conv2d(x * torch.sigmoid(z)[:, :, None, None], L["w"]))
    return Case(EcaConvFn, L, ["x"],
                lambda L: EcaConvFn.apply(L["x"], L["w1"], L["w"], 1, 0, "sigmoid"), ref)


def _bnact(dev, c, act, res):
    from jabd_amd.train import BnActFn
    g = torch.Generator().manual_seed(c)
    L = collections.OrderedDict(
        x=_leaf(_rand(g, 3, 5, 6, c, scale=2.0, shift=1.0), dev),
        gamma=_leaf(1 + 0.2 * _rand(g, c), dev, True), beta=_leaf(0.1 * _rand(g, c), dev, True))
    if res:
        L["res"] = _leaf(_rand(g, 3, 5, 6, c), dev)
    rm, rv = torch.zeros(c, device=dev), torch.ones(c, device=dev)

    def ref(L):
        z = tF.batch_norm(_c2(L["x"]), None, None, L["gamma"], L["beta"], True, 0.1, 1e-5)
        if res:
            z = z + _c2(L["res"])
        return _c4(model_ref.kink(z, act, 0.1))
    return Case(BnActFn, L, ["x", "res"] if res else ["x"],
                lambda L: BnActFn.apply(L["x"], L["gamma"], L["beta"], L.get("res"), rm, rv, act,
                                        0.1, 0.1, 1e-5), ref)


def _dwconv(dev, c, k, s, h):
    from jabd_amd.train import DwConvFn
    g = torch.Generator().manual_seed(c + k)
    L = collections.OrderedDict(x=_leaf(_rand(g, 2, h, h + 2, c), dev),
                                w=_leaf(_rand(g, c, 1, k, k) / k, dev, True))
    return Case(DwConvFn, L, ["x"], lambda L: DwConvFn.apply(L["x"], L["w"], s),
                lambda L: _c4(tF.conv2d(_c2(L["x"]), L["w"], None, s, k // 2, 1, c)))


_NLM_ORDER = ("f_query.weight", "f_query.bias", "f_key.weight", "f_key.bias", "f_value.weight",
              "f_value.bias", "W.weight", "W.bias")


def _nlm(dev):
    from jabd_amd.train import NlmFn
    C, hs, h = 40, 4, 8
    g = torch.Generator().manual_seed(C + h)
    L = collections.OrderedDict(src=_leaf(_rand(g, 2, hs, hs, C), dev),
                                lat=_leaf(_rand(g, 2, h, h, C), dev))
    for n in _NLM_ORDER:
        if n.endswith("bias"):
            t = 0.1 * _rand(g, C if n.startswith("W") else 4)
        elif n.startswith("W"):
            t = _rand(g, C, 4, 1, 1) / 2
        else:
            t = _rand(g, 4, C, 1, 1) / C ** 0.5
        L[n] = _leaf(t, dev, True)

    def ref(L):
        up = tF.interpolate(_c2(L["src"]), size=[h, h], mode="nearest")
        P = {"n." + n: L[n] for n in _NLM_ORDER}
        return L["lat"] + _c4(model_ref.nlm(model_ref.Ctx(P), up, "n."))
    return Case(NlmFn, L, ["src", "lat"],
                lambda L: NlmFn.apply(L["src"], L["lat"], *[L[n] for n in _NLM_ORDER],
                                      (1, 4, 8, 12)), ref, zero=["f_key.bias"])


def _upadd(dev):
    from jabd_amd.train import UpAddFn
    g = torch.Generator().manual_seed(1)
    L = collections.OrderedDict(src=_leaf(_rand(g, 2, 4, 4, 40), dev),
                                lat=_leaf(_rand(g, 2, 8, 8, 40), dev))
    return Case(UpAddFn, L, ["src", "lat"], lambda L: UpAddFn.apply(L["src"], L["lat"]),
                lambda L: L["lat"] + _c4(tF.interpolate(_c2(L["src"]), size=[8, 8],
                                                        mode="nearest")))


def _upsample(dev, mode):
    from jabd_amd.train import UpsampleFn
    g = torch.Generator().manual_seed(2)
    L = collections.OrderedDict(src=_leaf(_rand(g, 2, 5, 7, 8), dev))
    kw = {"mode": "nearest"} if mode == "nearest" else {"mode": "bicubic", "align_corners": True}
    return Case(UpsampleFn, L, ["src"], lambda L: UpsampleFn.apply(L["src"], 13, 9, mode),
                lambda L: _c4(tF.interpolate(_c2(L["src"]), size=[13, 9], **kw)))


def _add3(dev):
    from jabd_amd.train import Add3Fn
    g = torch.Generator().manual_seed(3)
    L = collections.OrderedDict((n, _leaf(_rand(g, 2, 5, 6, 8), dev)) for n in "abc")
    return Case(Add3Fn, L, "abc", lambda L: Add3Fn.apply(L["a"], L["b"], L["c"]),
                lambda L: L["a"] + L["b"] + L["c"])


def _nlmattn(dev):
    from jabd_amd.train import NlmAttnFn
    g = torch.Generator().manual_seed(4)
    L = collections.OrderedDict(q=_leaf(_rand(g, 2, 16, 16, 40, scale=0.3), dev),
                                kp=_leaf(_rand(g, 2, 110, 40), dev),
                                vp=_leaf(_rand(g, 2, 110, 40), dev))

    def ref(L):
        q = L["q"].reshape(2, 256, 40)
        sim = torch.softmax(q @ L["kp"].transpose(1, 2), -1)
        return (sim @ L["vp"]).reshape(2, 16, 16, 40)
    return Case(NlmAttnFn, L, ["q", "kp", "vp"],
                lambda L: NlmAttnFn.apply(L["q"], L["kp"], L["vp"]), ref)


def _sshtail(dev):
    from jabd_amd.train import SshTailFn
    g = torch.Generator().manual_seed(5)
    cs = (20, 12, 12)
    L = collections.OrderedDict()
    for n, c in zip("abc", cs):
        L[n] = _leaf(_rand(g, 2, 6, 7, c, scale=2.0, shift=0.5), dev)
    for n, c in zip("abc", cs):
        L["g" + n] = _leaf(1 + 0.2 * _rand(g, c), dev, True)
        L["b" + n] = _leaf(0.1 * _rand(g, c), dev, True)
    stats = [(torch.zeros(c, device=dev), torch.ones(c, device=dev), 0.1, 1e-5) for c in cs]

    def ref(L):
        z = [tF.batch_norm(_c2(L[n]), None, None, L["g" + n], L["b" + n], True, 0.1, 1e-5)
             for n in "abc"]
        return _c4(model_ref.kink(torch.cat(z, 1), "relu"))
    return Case(SshTailFn, L, "abc",
                lambda L: SshTailFn.apply(L["a"], L["b"], L["c"], L["ga"], L["ba"], L["gb"],
                                          L["bb"], L["gc"], L["bc"], stats), ref)


def _heads(dev):
    from jabd_amd.train import HeadsFn
    C = 40
    g = torch.Generator().manual_seed(C)
    L = collections.OrderedDict((f"f{i}", _leaf(_rand(g, 2, s, s, C), dev))
                                for i, s in enumerate((8, 4, 2)))
    for i in range(3):
        for kind, n in (("box", 8), ("cls", 4), ("lmk", 20)):
            L[f"{kind}{i}.w"] = _leaf(_rand(g, n, C, 1, 1) / C ** 0.5, dev, True)
            L[f"{kind}{i}.b"] = _leaf(0.1 * _rand(g, n), dev, True)
    wb = [f"{kind}{i}.{p}" for i in range(3) for kind in ("box", "cls", "lmk") for p in "wb"]

    def ref(L):
        outs = []
        for kind, k in (("box", 4), ("cls", 2), ("lmk", 10)):
            parts = [tF.conv2d(_c2(L[f"f{i}"]), L[f"{kind}{i}.w"], L[f"{kind}{i}.b"])
                     .permute(0, 2, 3, 1).reshape(2, -1, k) for i in range(3)]
            outs.append(torch.cat(parts, 1))
        return outs
    return Case(HeadsFn, L, ["f0", "f1", "f2"],
                lambda L: HeadsFn.apply(L["f0"], L["f1"], L["f2"], (None, None, None),
                                        *[L[n] for n in wb]), ref)


def _maxpool(dev):
    from jabd_amd.train import MaxPoolFn
    g = torch.Generator().manual_seed(6)
    L = collections.OrderedDict(x=_leaf(_rand(g, 2, 17, 23, 64), dev))
    return Case(MaxPoolFn, L, ["x"], lambda L: MaxPoolFn.apply(L["x"]),
                lambda L: _c4(model_ref.maxpool(_c2(L["x"]))))


def _pad(dev):
    from jabd_amd.train import PadFn
    g = torch.Generator().manual_seed(7)
    L = collections.OrderedDict(w0=_leaf(_rand(g, 10, 40, 3, 3), dev, True),
                                w1=_leaf(_rand(g, 10, 10, 3, 3), dev, True),
                                gamma=_leaf(_rand(g, 10), dev, True),
                                var=_leaf(_rand(g, 10).abs(), dev, True))
    spec = (((12, 40, 3, 3), 0.0), ((12, 12, 3, 3), 0.0), ((12,), 0.0), ((12,), 1.0))

    def ref(L):
        return [tF.pad(L["w0"], (0, 0, 0, 0, 0, 0, 0, 2)), tF.pad(L["w1"], (0, 0, 0, 0, 0, 2, 0, 2)),
                tF.pad(L["gamma"], (0, 2)), tF.pad(L["var"], (0, 2), value=1.0)]
    return Case(PadFn, L, [], lambda L: PadFn.apply(spec, *L.values()), ref)


def _fork(dev):
    from jabd_amd.train import ForkFn
    g = torch.Generator().manual_seed(8)
    L = collections.OrderedDict(x=_leaf(_rand(g, 2, 5, 6, 8), dev))
    return Case(ForkFn, L, ["x"], lambda L: ForkFn.apply(L["x"], 3),
                lambda L: [L["x"] * 1 for _ in range(3)])


def _module_case(node, dev, mod, used, x, call, ref, zero=()):
    """A row whose parameters live in an nn.Module: the leaves are the
    Parameters `used` (by their state_dict names) and the input x."""
    snap = {k: v.detach().clone() for k, v in mod.state_dict().items()}
    mod.to(dev).train()
    names = {id(p): k for k, p in mod.named_parameters()}
    L = collections.OrderedDict(x=_leaf(x, dev))
    for p in used:
        if p is not None:
            L[names[id(p)]] = p

    def run_ref(L):
        dt = L["x"].dtype
        P = {k: (v.clone().to(dt) if v.is_floating_point() else v.clone())
             for k, v in snap.items()}
        P.update({k: v for k, v in L.items() if k != "x"})
        return _c4(ref(model_ref.Ctx(P, True), _c2(L["x"])))
    return Case(node, L, ["x"], lambda L: call(mod, L["x"]), run_ref, zero)


MNV3_SPECS = {  # skip kind -> Block_eca spec (k, cin, exp, cout, act, se, stride)
    "identity": (5, 40, 120, 40, "relu", True, 1),
    "concat": (3, 80, 480, 112, "hswish", True, 1),
    "dw_concat": (3, 16, 64, 24, "relu", False, 2),
    "dw_residual": (3, 24, 72, 24, "relu", False, 2),
}


def _mnv3(dev, kind):
    import nets.mobilenetV3 as mv3
    from jabd_amd import train as T
    spec = MNV3_SPECS[kind]
    k, cin, exp, cout, act, se, stride = spec
    blk = init_for_parity(mv3.Block_eca(k, cin, exp, cout, nn.ReLU if act == "relu"
                                        else nn.Hardswish, se, stride), seed=cin)
    x = _rand(torch.Generator().manual_seed(cin), 2, 16, 16, cin)

    def call(m, x):
        y = T._mnv3_block(m, x)
        assert type(y.grad_fn).__name__.startswith("MNv3BlockFn") and \
            y.grad_fn.kind == kind, "the fused node of this skip kind"
        return y
    # a bias in front of a training-mode BatchNorm is removed by its batch mean
    zero = ["skip.1.bias", "skip.2.bias"] if kind == "dw_concat" else []
    return _module_case(T.MNv3BlockFn, dev, blk, T._block_params(blk), x, call,
                        lambda ctx, x: model_ref.block_eca(ctx, x, "", spec), zero)


def _r50_ref(ctx, x, pre, down, stride=1):
    o = model_ref.kink(ctx.bn(ctx.conv(x, pre + "conv1"), pre + "bn1"), "relu")
    o = model_ref.kink(ctx.bn(ctx.conv(o, pre + "conv2", stride, 1), pre + "bn2"), "relu")
    o = ctx.bn(ctx.conv(o, pre + "conv3"), pre + "bn3")
    idn = ctx.bn(ctx.conv(x, pre + "downsample.0", stride), pre + "downsample.1") if down else x
    return model_ref.kink(o + idn, "relu")


def _r50_layer1(n):
    """layer1.0 (1x1 downsample) .. layer1.<n-1> of torchvision's ResNet-50."""
    from jabd_amd import modules as M
    from nets.resnet_pytorch_r import Bottleneck, conv1x1
    blocks = [Bottleneck(64, 64, 1, M.ConvBNAct(conv1x1(64, 256), M.BatchNorm2d(256)))]
    blocks += [Bottleneck(256, 64) for _ in range(n - 1)]
    return init_for_parity(nn.Sequential(*blocks), seed=11)


def _r50(dev, which):
    """which: 0 / 1 = layer1.0 / layer1.1 alone (unlinked, as a direct caller
    gets them); "linked" = layer1.0 -> layer1.1 with the bn3 link taken."""
    from jabd_amd import train as T
    seq = _r50_layer1(2)
    g = torch.Generator().manual_seed(9)
    if which == "linked":
        def call(m, x):
            return T._r50_block(m[1], T._r50_block(m[0], x, link=True), link=True)
        return _module_case(T.R50BlockFn, dev, seq, T._r50_params(seq[0]) + T._r50_params(seq[1]),
                            _rand(g, 2, 8, 8, 64), call,
                            lambda ctx, x: _r50_ref(ctx, _r50_ref(ctx, x, "0.", True), "1.", False))
    blk = seq[which]
    return _module_case(T.R50BlockFn, dev, blk, T._r50_params(blk),
                        _rand(g, 2, 8, 8, 64 if which == 0 else 256),
                        lambda m, x: T._r50_block(m, x),
                        lambda ctx, x: _r50_ref(ctx, x, "", which == 0))


def _act(dev, act):
    from jabd_amd.modules import ActFn
    g = torch.Generator().manual_seed(8)
    L = collections.OrderedDict(x=_leaf(_rand(g, 2, 13, 9, 24, scale=4.0), dev))
    return Case(ActFn, L, ["x"], lambda L: ActFn.apply(L["x"], act, 0.1),
                lambda L: model_ref.kink(L["x"], act, 0.1))


def _adaptivepool(dev):
    from jabd_amd.modules import AdaptivePoolFn
    g = torch.Generator().manual_seed(10)
    sizes = (1, 3, 6, 8)
    L = collections.OrderedDict(x=_leaf(_rand(g, 2, 13, 17, 12), dev))
    return Case(AdaptivePoolFn, L, ["x"], lambda L: AdaptivePoolFn.apply(L["x"], sizes),
                lambda L: model_ref.psp(_c2(L["x"]), sizes).permute(0, 2, 1))


def _ecascale(dev, gate):
    from jabd_amd.modules import EcaScaleFn
    c = 40
    ke = model_ref.eca_kernel_size(c)
    g = torch.Generator().manual_seed(11)
    L = collections.OrderedDict(x=_leaf(_rand(g, 2, 8, 8, c, shift=0.3), dev),
                                w1=_leaf(_rand(g, 1, 1, ke) * 3, dev, True))
    return Case(EcaScaleFn, L, ["x"], lambda L: EcaScaleFn.apply(L["x"], L["w1"], gate),
                lambda L: _c4(model_ref.eca(model_ref.Ctx({"e.conv.weight": L["w1"]}),
                                            _c2(L["x"]), "e", gate)))


def _scale(dev):
    from jabd_amd.modules import ScaleFn
    g = torch.Generator().manual_seed(12)
    L = collections.OrderedDict(x=_leaf(_rand(g, 2, 9, 7, 24), dev),
                                s=_leaf(torch.rand(2, 24, 1, 1, generator=g), dev))
    return Case(ScaleFn, L, ["x", "s"], lambda L: ScaleFn.apply(L["x"], L["s"]),
                lambda L: L["x"] * L["s"].reshape(2, 1, 1, 24))


def _bicubic(dev):
    from jabd_amd.ops import UpsampleBicubicFn
    g = torch.Generator().manual_seed(20 * 31 + 40)
    L = collections.OrderedDict(x=_leaf(_rand(g, 2, 20, 20, 64), dev))
    return Case(UpsampleBicubicFn, L, ["x"], lambda L: UpsampleBicubicFn.apply(L["x"], 40, 40),
                lambda L: _c4(tF.interpolate(_c2(L["x"]), size=[40, 40], mode="bicubic",
                                             align_corners=True)))


def _beca(dev):
    from jabd_amd.ops import BecaFn
    g = torch.Generator().manual_seed(64 + 40)
    L = collections.OrderedDict(x=_leaf(_rand(g, 2, 40, 40, 64, scale=2.0, shift=0.5), dev),
                                w=_leaf(_rand(g, 3) * 3, dev, True))

    def ref(L):
        x = _c2(L["x"])
        y = (x - x.mean((2, 3), keepdim=True)).pow(2).mean((2, 3)).pow(0.5)
        y = tF.conv1d(y.unsqueeze(1), L["w"].view(1, 1, 3), padding=1).squeeze(1)
        return _c4(x * model_ref.kink(y, "hsigmoid")[:, :, None, None])
    return Case(BecaFn, L, ["x"], lambda L: BecaFn.apply(L["x"], L["w"]), ref)


def _weighted(dev):
    from jabd_amd.parallel import _WeightedLossFn
    L = collections.OrderedDict((n, _leaf(torch.tensor(v), dev))
                                for n, v in (("r", 1.25), ("c", 0.4), ("lm", 3.5)))
    return Case(_WeightedLossFn, L, ["r", "c", "lm"],
                lambda L: _WeightedLossFn.apply(L["r"], L["c"], L["lm"], 2.0),
                lambda L: 2.0 * L["r"] + L["c"] + L["lm"])


ROWS = {
    "ConvFn-16-64-1x1": lambda d: _conv(d, 16, 64, 1, 12, False),
    "ConvFn-40-40-3x3-bias": lambda d: _conv(d, 40, 40, 3, 9, True),
    "EcaConvFn": _ecaconv,
    "BnActFn-relu": lambda d: _bnact(d, 40, "relu", False),
    "BnActFn-hswish-res": lambda d: _bnact(d, 24, "hswish", True),
    "DwConvFn-64-3x3s2": lambda d: _dwconv(d, 64, 3, 2, 10),
    "DwConvFn-72-5x5s2": lambda d: _dwconv(d, 72, 5, 2, 11),
    "NlmFn": _nlm,
    "UpAddFn": _upadd,
    "UpsampleFn-nearest": lambda d: _upsample(d, "nearest"),
    "UpsampleFn-bicubic": lambda d: _upsample(d, "bicubic"),
    "Add3Fn": _add3,
    "NlmAttnFn": _nlmattn,
    "SshTailFn": _sshtail,
    "HeadsFn": _heads,
    "MaxPoolFn": _maxpool,
    "PadFn": _pad,
    "ForkFn": _fork,
    "MNv3BlockFn-identity": lambda d: _mnv3(d, "identity"),
    "MNv3BlockFn-concat": lambda d: _mnv3(d, "concat"),
    "MNv3BlockFn-dw_concat": lambda d: _mnv3(d, "dw_concat"),
    "MNv3BlockFn-dw_residual": lambda d: _mnv3(d, "dw_residual"),
    "R50BlockFn-layer1.0": lambda d: _r50(d, 0),
    "R50BlockFn-layer1.1": lambda d: _r50(d, 1),
    "R50BlockFn-layer1.0-1.1-linked": lambda d: _r50(d, "linked"),
    "ActFn-relu": lambda d: _act(d, "relu"),
    "ActFn-hswish": lambda d: _act(d, "hswish"),
    "AdaptivePoolFn": _adaptivepool,
    "EcaScaleFn-sigmoid": lambda d: _ecascale(d, "sigmoid"),
    "EcaScaleFn-hsigmoid": lambda d: _ecascale(d, "hsigmoid"),
    "ScaleFn": _scale,
    "UpsampleBicubicFn": _bicubic,
    "BecaFn": _beca,
    "_WeightedLossFn": _weighted,
}
MULTI_OUT = ("HeadsFn", "PadFn", "ForkFn")
# nodes whose backward needs shapes only
SAVE_NOTHING = ("UpAddFn", "UpsampleFn", "Add3Fn", "PadFn", "ForkFn", "AdaptivePoolFn",
                "UpsampleBicubicFn", "_WeightedLossFn")


# ----------------------------------------------------------------------------- helpers
def _node_classes():
    import importlib
    found = []
    for name in NODE_MODULES:
        mod = importlib.import_module(name)
        found += [c for _, c in inspect.getmembers(mod, inspect.isclass)
                  if issubclass(c, torch.autograd.Function) and c.__module__ == name]
    return found


def _seeds(outs, seed=13):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(o.shape, generator=g).to(o.device) for o in outs]


def _grads(case, outs, gs, retain=True):
    """{leaf name: gradient} of sum(out . g) for the leaves that require one."""
    names = [k for k, t in case.leaves.items() if t.requires_grad]
    pairs = [(o, g) for o, g in zip(outs, gs) if o.requires_grad and g is not None]
    res = torch.autograd.grad([o for o, _ in pairs], [case.leaves[k] for k in names],
                              [g for _, g in pairs], retain_graph=retain, allow_unused=True)
    return dict(zip(names, res))


def _assert_same(got, want, what):
    assert got.keys() == want.keys(), what
    for k in want:
        a, b = got[k], want[k]
        assert (a is None) == (b is None), f"{what}: {k} None-ness"
        if b is not None:
            assert a.shape == b.shape and torch.equal(a, b), \
                f"{what}: {k} differs, max |d| {float((a - b).abs().max()):.3e}"


def _tensors(obj, out):
    if isinstance(obj, torch.Tensor):
        out.append(obj)
    elif isinstance(obj, (tuple, list)):
        for o in obj:
            _tensors(o, out)
    elif isinstance(obj, dict):
        _tensors(list(obj.values()), out)


def _saved(outs):
    """Every tensor a backward may read that the test can reach: the nodes'
    saved tensors and the statistics / link records kept on their ctx."""
    found, seen, todo = [], set(), [o.grad_fn for o in outs if o.grad_fn is not None]
    while todo:
        fn = todo.pop()
        if fn is None or id(fn) in seen:
            continue
        seen.add(id(fn))
        if isinstance(fn, torch.autograd.function.BackwardCFunction):
            _tensors(list(fn.saved_tensors), found)
            for attr in ("st", "sts", "stats", "info", "prev"):
                _tensors(getattr(fn, attr, None), found)
        todo += [f for f, _ in fn.next_functions]
    return found


def _noncontiguous(g, how):
    if how == "permuted":   # made channel-first, then viewed channel-last
        perm = (0, g.dim() - 1) + tuple(range(1, g.dim() - 1))
        inv = sorted(range(g.dim()), key=lambda i: perm[i])
        return g.permute(perm).contiguous().permute(inv)
    big = torch.zeros((2 * g.shape[0],) + tuple(g.shape[1:]), device=g.device)
    big[::2] = g
    return big[::2]


def _fro(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.fixture(params=sorted(ROWS))
def case(request, cuda):
    return ROWS[request.param](cuda)


# ----------------------------------------------------------------------------- tests
def test_every_node_has_a_row(cuda):
    nodes = _node_classes()
    assert len(nodes) >= 23, [c.__name__ for c in nodes]
    covered = {ROWS[k](cuda).node for k in ROWS}
    missing = [c.__name__ for c in nodes if c not in covered]
    assert not missing, f"autograd nodes without a row in ROWS: {missing}"
    assert all(m in ROWS for m in MULTI_OUT)


def test_purity_and_reentrancy(case):
    case.require(case.leaves)
    outs = case.run()
    gs = _seeds(outs)
    saved = _saved(outs)
    assert saved or case.node.__name__ in SAVE_NOTHING, "no saved tensor found to watch"
    watched = [("gradient", t) for t in gs] + [("output", o) for o in outs] + \
        [("leaf " + k, t) for k, t in case.leaves.items()] + [("saved", t) for t in saved]
    before = [t.detach().clone() for _, t in watched]
    first = _grads(case, outs, gs)
    for (what, t), b in zip(watched, before):
        assert torch.equal(t.detach(), b), f"backward wrote into a {what} tensor"
    assert all(g is not None for g in first.values()), [k for k, g in first.items() if g is None]
    # (Add3Fn, UpAddFn, ForkFn and the linked R50BlockFn hand one gradient
    # tensor to several inputs, or the incoming one on: the clones above show
    # that nothing downstream of them wrote into it)
    second = _grads(case, outs, gs)
    _assert_same(second, first, "second backward over the retained graph")
    for (what, t), b in zip(watched, before):
        assert torch.equal(t.detach(), b), f"second backward wrote into a {what} tensor"


def test_gradient_layout(case):
    case.require(case.leaves)
    outs = case.run()
    gs = _seeds(outs)
    want = _grads(case, outs, gs)
    for how in ("permuted", "strided"):
        var = [_noncontiguous(g, how) if g.dim() >= (3 if how == "permuted" else 1) else g
               for g in gs]
        assert all(torch.equal(v, g) for v, g in zip(var, gs))
        if any(g.dim() >= 3 for g in gs):
            assert any(not v.is_contiguous() for v in var), how
        _assert_same(_grads(case, outs, var), want, f"{how} incoming gradient")
    flat = [torch.full((), 0.37, device=o.device).expand(o.shape) for o in outs]
    _assert_same(_grads(case, outs, flat), _grads(case, outs, [f.contiguous() for f in flat]),
                 "stride-0 incoming gradient")


def test_frozen_subsets(case):
    case.require(case.leaves)
    outs = case.run()
    gs = _seeds(outs)
    want = _grads(case, outs, gs, retain=False)
    every = list(case.leaves)
    settings = []
    if case.acts and case.params:
        settings += [set(case.acts), set(case.params)]
    if len(every) > 1:   # each parameter alone frozen (each input, where there are several)
        settings += [set(every) - {p} for p in case.params]
        settings += [set(every) - {a} for a in case.acts if len(case.acts) > 1]
    for on in settings:
        case.require(on)
        outs = case.run()
        pairs = [(o, g) for o, g in zip(outs, gs) if o.requires_grad]
        torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs])
        for k, t in case.leaves.items():
            if k in on:
                assert t.grad is not None, f"{sorted(on)} on: no gradient for {k}"
                assert torch.equal(t.grad, want[k]), f"{sorted(on)} on: {k} differs from all-on"
            else:
                assert t.grad is None, f"{sorted(on)} on: frozen {k} got a gradient"


@pytest.mark.parametrize("row", MULTI_OUT)
def test_unused_outputs(cuda, row):
    case = ROWS[row](cuda)
    case.require(case.leaves)
    outs = case.run()
    gs = _seeds(outs)
    for i in range(len(outs)):
        alone = _grads(case, outs, [g if j == i else None for j, g in enumerate(gs)])
        zeros = _grads(case, outs, [g if j == i else torch.zeros_like(g)
                                    for j, g in enumerate(gs)])
        for k in zeros:   # a leaf no used output depends on: None or exact zeros
            if alone[k] is None:
                assert not bool(zeros[k].any()), (i, k)
                alone[k] = zeros[k]
        _assert_same(alone, zeros, f"output {i} alone")


def test_reference(case):
    """All-on, contiguous: forward and every gradient against the fp64 torch
    restatement; per tensor relative Frobenius error <= max(1e-4, 4 x the
    fp32 restatement's error)."""
    case.require(case.leaves)
    kk = Kinks()
    with kk.record():
        outs = case.run()
    gs = _seeds(outs)
    got = _grads(case, outs, gs, retain=False)
    ref = {}
    for dt in (torch.float64, torch.float32):
        L = collections.OrderedDict((k, v.detach().cpu().to(dt).requires_grad_(True))
                                    for k, v in case.leaves.items())
        with kk.replay(dt):
            o = case.ref(L)
        o = list(o) if isinstance(o, (tuple, list)) else [o]
        assert not kk.unmatched, kk.unmatched
        gr = torch.autograd.grad(o, list(L.values()), [g.cpu().to(dt) for g in gs],
                                 allow_unused=True)
        ref[dt] = ([t.detach() for t in o], dict(zip(L, gr)))
    o64, g64 = ref[torch.float64]
    o32, g32 = ref[torch.float32]
    for i, (o, r, r32) in enumerate(zip(outs, o64, o32)):
        assert o.shape == r.shape
        e, e32 = _fro(o, r), _fro(r32, r)
        assert e <= max(1e-4, 4 * e32), f"output {i}: {e:.2e} (fp32 restatement {e32:.2e})"
    gmax = max(float(g.abs().max()) for g in g64.values() if g is not None)
    for k, r in g64.items():
        assert got[k] is not None and r is not None, k
        if k in case.zero:
            assert float(got[k].abs().max()) <= 1e-4 * gmax, k
            continue
        e, e32 = _fro(got[k], r), _fro(g32[k], r)
        assert e <= max(1e-4, 4 * e32), f"d{k}: {e:.2e} (fp32 restatement {e32:.2e})"
