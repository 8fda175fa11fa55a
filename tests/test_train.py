"""A9/A11 training parity: MultiBoxLoss (values, selection, gradients) and the
full detector backward (every parameter gradient, BN running stats) of the
HIP path against autograd through the oracle restatement (PyTorch-CPU fp32).
Tolerances: losses 1e-5 relative; gradients vs an fp64 oracle run with the
HIP forward's activation masks (tests/_kinks.py), per tensor relative
Frobenius error <= max(2e-3, 4x the mask-matched fp32 oracle's own error)."""
import pytest
import torch

from _kinks import Kinks
from _util import init_for_parity, rel_err
from oracle import box_ref, model_ref


def _targets(B, size, seed):
    from jabd_amd import synth
    return [torch.from_numpy(t) for t in synth.targets(B, size, seed=seed)]


@pytest.mark.gpu
def test_multibox_loss_parity(cuda):
    from nets.retinaface_training import MultiBoxLoss
    cfg = {"min_sizes": [[16, 32], [64, 128], [256, 512]], "steps": [8, 16, 32], "clip": False}
    pri = box_ref.anchors(cfg, (256, 256))
    B, A = 4, pri.shape[0]
    g = torch.Generator().manual_seed(3)
    loc = torch.randn(B, A, 4, generator=g)
    conf = torch.randn(B, A, 2, generator=g) * 2
    landm = torch.randn(B, A, 10, generator=g)
    tg = _targets(B, 256, 9)
    # oracle: match + loss + autograd
    lt, ct, lmt = box_ref.match_batch(tg, pri)
    leaves = [t.clone().requires_grad_(True) for t in (loc, conf, landm)]
    rl, rc, rlm, info = box_ref.multibox_loss(*leaves, lt, ct, lmt)
    (2.0 * rl + rc + rlm).backward()
    # HIP path
    crit = MultiBoxLoss(2, 0.35, 7, [0.1, 0.2], True)
    gl = [t.to(cuda).requires_grad_(True) for t in (loc, conf, landm)]
    l, c, lm = crit(tuple(gl), pri.to(cuda), [t.to(cuda) for t in tg])
    (2.0 * l + c + lm).backward()
    for got, ref in ((l, rl), (c, rc), (lm, rlm)):
        assert abs(float(got) - float(ref)) <= 1e-5 * max(1.0, abs(float(ref))), (got, ref)
    for g_, r_ in zip(gl, leaves):
        assert rel_err(g_.grad, r_.grad) < 1e-5


@pytest.mark.gpu
def test_multibox_diou_loss_parity(cuda):
    """The DIoU variant (nets/retinaface_training_DIOU.py:524-665): values 1e-5
    relative to the fp32 oracle; gradients (analytic DIoU backward in the kernel
    vs autograd through the oracle) relative Frobenius error < 1e-4 against an
    fp64 oracle run."""
    from nets.retinaface_training_DIOU import MultiBoxLoss
    cfg = {"min_sizes": [[16, 32], [64, 128], [256, 512]], "steps": [8, 16, 32], "clip": False}
    pri = box_ref.anchors(cfg, (256, 256))
    B, A = 4, pri.shape[0]
    g = torch.Generator().manual_seed(4)
    loc = torch.randn(B, A, 4, generator=g)
    conf = torch.randn(B, A, 2, generator=g) * 2
    landm = torch.randn(B, A, 10, generator=g)
    tg = _targets(B, 256, 11)
    lt, ct, lmt = box_ref.match_iou_batch(tg, pri)
    refs = {}
    for dt in (torch.float32, torch.float64):
        leaves = [t.clone().to(dt).requires_grad_(True) for t in (loc, conf, landm)]
        out = box_ref.multibox_loss(*leaves, lt.to(dt), ct, lmt.to(dt), diou=(pri, [0.1, 0.2]))
        (2.0 * out[0] + out[1] + out[2]).backward()
        refs[dt] = (out[:3], [t.grad for t in leaves])
    crit = MultiBoxLoss(2, 0.35, 7, [0.1, 0.2], True)
    gl = [t.to(cuda).requires_grad_(True) for t in (loc, conf, landm)]
    l, c, lm = crit(tuple(gl), pri.to(cuda), [t.to(cuda) for t in tg])
    (2.0 * l + c + lm).backward()
    for got, ref in zip((l, c, lm), refs[torch.float32][0]):
        assert abs(float(got) - float(ref)) <= 1e-5 * max(1.0, abs(float(ref))), (got, ref)
    assert float(l) > 0.0
    for g_, r_ in zip(gl, refs[torch.float64][1]):
        assert rel_err(g_.grad, r_) < 1e-4


def _oracle_grads(sd, fn, x, dtype, kk, wseed=5, frozen=None):
    """frozen: a name prefix ("body.") whose parameters are constants."""
    def leaf(k, v):
        return v.is_floating_point() and "running" not in k and \
            not (frozen is not None and k.startswith(frozen))
    P = {k: (v.clone().to(dtype).requires_grad_(True) if leaf(k, v)
             else (v.clone().to(dtype) if v.is_floating_point() else v.clone()))
         for k, v in sd.items()}
    g = torch.Generator().manual_seed(wseed)
    with kk.replay():
        ref = fn(P, x.to(dtype), "train", train_bn=True)
    assert not kk.unmatched, f"oracle kinks without a HIP tensor: {kk.unmatched[:5]}"
    wts = [torch.randn(r.shape, generator=g) for r in ref]
    sum(((r * w.to(dtype)).sum() for r, w in zip(ref, wts))).backward()
    grads = {k: p.grad for k, p in P.items()
             if isinstance(p, torch.Tensor) and p.requires_grad and p.grad is not None}
    return [r.detach() for r in ref], grads, P, wts


def _fro(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _train_compare(model, fn, x, cuda, tol=2e-3, frozen=None):
    """Gradients are judged per tensor against an fp64 run of the oracle
    whose activation masks (ReLU / LeakyReLU / Hardswish / Hardsigmoid
    regions, max-pool argmaxes) are the HIP forward's own (tests/_kinks.py):
    relative Frobenius error within max(tol, 4x the error of the equally
    mask-matched fp32 oracle run).  frozen: a parameter-name prefix set to
    requires_grad=False in the model (left so on return) and held constant in
    the oracle; those parameters must end without a gradient."""
    import re
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    kk = Kinks()
    m = model.to(cuda).train()
    cold = [k for k, q in m.named_parameters() if frozen is not None and k.startswith(frozen)]
    assert (frozen is None) == (not cold)
    for k, q in m.named_parameters():
        if k in cold:
            q.requires_grad_(False)
    with kk.record():
        out = m(x.to(cuda))
    ref64, g64, P64, wts = _oracle_grads(sd, fn, x, torch.float64, kk, frozen=frozen)
    ref32, g32, _, _ = _oracle_grads(sd, fn, x, torch.float32, kk, frozen=frozen)
    assert kk.matched > 20
    sum(((o * w.to(cuda)).sum() for o, w in zip(out, wts))).backward()
    for o, r, name in zip(out, ref64, ("loc", "conf", "landm")):
        e = rel_err(o.detach(), r)
        assert e < 1e-3, f"{name} forward rel err {e:.2e}"
    named = dict(m.named_parameters())
    assert not set(cold) & set(g64)
    for k in cold:
        assert named[k].grad is None, f"frozen {k} got a gradient"
    gmax = max(float(g.abs().max()) for g in g64.values())
    # Analytically-zero gradients (rounding noise in every path) are checked
    # for smallness: f_key.bias shifts all logits of a pixel equally
    # (softmax-invariant); a bias feeding conv->BN in training mode is removed
    # by that BN's batch mean.
    zero = re.compile(r"(f_key\.bias|skip\.2\.bias)$")
    rows = []
    for k, rg in g64.items():
        q = named[k]
        assert q.grad is not None, f"no HIP gradient for {k}"
        if zero.search(k) or (k.endswith("skip.1.bias")
                              and k.replace("skip.1.bias", "skip.3.weight") in g64):
            assert float(q.grad.abs().max()) <= 1e-4 * gmax, k
            continue
        rows.append((_fro(q.grad, rg), _fro(g32[k], rg), k))
    assert len(rows) > 50
    bad = [r for r in rows if r[0] > max(tol, 4 * r[1])]
    assert not bad, f"gradients off vs fp64 (hip, oracle-fp32, name): {sorted(bad)[-5:]}"
    for k, v in m.state_dict().items():
        if "running" in k:
            e = rel_err(v, P64[k])
            assert e < 1e-4, f"{k} running stat rel err {e:.2e}"


@pytest.mark.gpu
def test_train_backward_parity_mnv3(cuda):
    from nets.retinaface_r import RetinaFace
    from utils.config import cfg_mnet
    m = init_for_parity(RetinaFace(cfg=cfg_mnet, mode="train"), seed=4)
    x = torch.randn(2, 3, 96, 96, generator=torch.Generator().manual_seed(1)) * 50
    _train_compare(m, model_ref.retinaface_mnv3, x, cuda)


@pytest.mark.gpu
def test_train_backward_parity_r50(cuda):
    from nets.retinaface_eca_nonlocal import RetinaFace
    from utils.config import cfg_re50
    m = init_for_parity(RetinaFace(cfg=cfg_re50, mode="train"), seed=6)
    x = torch.randn(2, 3, 128, 128, generator=torch.Generator().manual_seed(2)) * 50
    from jabd_amd import train as T
    taken = T.LINKS_TAKEN[0]
    _train_compare(m, model_ref.retinaface_r50, x, cuda)
    # the default path takes every bn3 link of its single-consumer chains:
    # layer1.0 .. layer2.3 (6), layer3 (5), layer4 (2); fork() ends a chain
    assert T.LINKS_TAKEN[0] - taken == R50_LINKS


R50_LINKS = 13


def _freeze_unfreeze(kind):
    if kind == "mnv3":
        from nets.retinaface_r import RetinaFace
        from utils.config import cfg_mnet
        m = init_for_parity(RetinaFace(cfg=cfg_mnet, mode="train"), seed=4)
        x = torch.randn(2, 3, 96, 96, generator=torch.Generator().manual_seed(1)) * 50
        return m, x, model_ref.retinaface_mnv3
    from nets.retinaface_eca_nonlocal import RetinaFace
    from utils.config import cfg_re50
    m = init_for_parity(RetinaFace(cfg=cfg_re50, mode="train"), seed=6)
    x = torch.randn(2, 3, 128, 128, generator=torch.Generator().manual_seed(2)) * 50
    return m, x, model_ref.retinaface_r50


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["mnv3", "r50"])
def test_train_freeze_unfreeze(cuda, kind):
    """The reference's Freeze_Train schedule (train_mobilenetV3_r.py:490-524):
    the first epochs run with model.body's parameters at requires_grad=False
    and the model in train() mode, then the same model object is unfrozen.
    Frozen step: the head gradients against the fp64 oracle with the same
    leaves held constant, no body parameter gets a gradient, and the body's
    BatchNorm buffers still update (running statistics at 1e-4 against the
    oracle, num_batches_tracked + 1).  Then, unfrozen, the same object passes
    the unchanged full comparison (the pack cache and the R50 link records
    carry nothing over from the frozen step)."""
    from jabd_amd import train as T
    m, x, fn = _freeze_unfreeze(kind)
    before = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}

    def counted(steps):
        """Every BatchNorm whose running mean moved (all but the in-block SE
        modules, which Block_eca never runs) counted `steps` batches."""
        sd, n = m.state_dict(), 0
        for k in before:
            if k.endswith("num_batches_tracked"):
                ran = not torch.equal(sd[k.replace("num_batches_tracked", "running_mean")].cpu(),
                                      before[k.replace("num_batches_tracked", "running_mean")])
                assert int(sd[k]) == int(before[k]) + (steps if ran else 0), k
                n += ran and k.startswith("body.")
        return n
    taken = T.LINKS_TAKEN[0]
    _train_compare(m, fn, x, cuda, frozen="body.")
    assert T.LINKS_TAKEN[0] == taken          # no backward reaches a frozen body
    assert counted(1) > 40
    # Freeze_Train's second phase
    for p in m.body.parameters():
        p.requires_grad = True
    m.zero_grad()
    _train_compare(m, fn, x, cuda)
    if kind == "r50":
        assert T.LINKS_TAKEN[0] - taken == R50_LINKS
    assert counted(2) > 40


def _param_grads(m):
    return {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["mnv3", "r50"])
def test_train_grad_accumulation(cuda, kind):
    """Gradient accumulation over two different inputs without zero_grad, and
    over two graphs alive at once (forward A, forward B, backward A, backward
    B), against the fp32 sum of the two separately computed gradient sets.
    torch.equal: the training kernels use no atomics, so a backward is
    bit-reproducible, and .grad accumulation is one fp32 add per element."""
    m, xa, _ = _freeze_unfreeze(kind)
    m = m.to(cuda).train()
    xb = torch.randn(xa.shape, generator=torch.Generator().manual_seed(17)) * 50
    xa, xb = xa.to(cuda), xb.to(cuda)
    wts = None

    def loss(out):
        nonlocal wts
        if wts is None:
            g = torch.Generator().manual_seed(5)
            wts = [torch.randn(o.shape, generator=g).to(cuda) for o in out]
        return sum((o * w).sum() for o, w in zip(out, wts))

    single = []
    for x in (xa, xb):
        m.zero_grad()
        loss(m(x)).backward()
        single.append(_param_grads(m))
    # (every parameter the forward uses: not the in-block SE modules / the classifier)
    assert single[0].keys() == single[1].keys() and len(single[0]) > 200
    want = {k: single[0][k] + single[1][k] for k in single[0]}
    m.zero_grad()
    loss(m(xa)).backward()
    loss(m(xb)).backward()
    got = _param_grads(m)
    bad = [k for k in want if not torch.equal(got[k], want[k])]
    assert not bad, f"accumulated over two steps: {bad[:5]}"
    m.zero_grad()
    la, lb = loss(m(xa)), loss(m(xb))
    la.backward()
    lb.backward()
    got = _param_grads(m)
    bad = [k for k in want if not torch.equal(got[k], want[k])]
    assert not bad, f"two live graphs: {bad[:5]}"


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["mnv3", "r50"])
def test_train_forward_no_grad(cuda, kind):
    """A train-mode forward under torch.no_grad() (a validation pass that
    forgot eval(), or a BatchNorm re-estimation pass) computes the outputs of
    the grad-enabled forward and advances the running statistics the same."""
    import copy
    m, x, _ = _freeze_unfreeze(kind)
    m1 = m.to(cuda).train()
    m2 = copy.deepcopy(m1)
    init = {k: v.clone() for k, v in m1.state_dict().items()}
    x = x.to(cuda)
    out1 = m1(x)
    with torch.no_grad():
        out2 = m2(x)
    assert all(o.requires_grad for o in out1) and not any(o.requires_grad for o in out2)
    for a, b in zip(out1, out2):
        assert torch.equal(a.detach(), b)
    s1, s2 = m1.state_dict(), m2.state_dict()
    moved = 0
    for k in init:
        if "running" in k or k.endswith("num_batches_tracked"):
            assert torch.equal(s1[k], s2[k]), k
            moved += not torch.equal(s1[k], init[k])
    assert moved > 60     # (a module the forward never runs, the in-block SE, stays put)


@pytest.mark.gpu
def test_train_r50_blocks_parity(cuda):
    """Stem (7x7/2 conv on NCHW input, BN, ReLU, 3x3/2 max-pool) and
    bottlenecks layer1.0 (1x1 downsample), layer2.0 (stride-2 downsample),
    layer2.1 (identity residual) alone: every gradient vs fp64 autograd."""
    from jabd_amd import train as T
    from nets.retinaface_eca_nonlocal import RetinaFace
    from utils.config import cfg_re50
    m = init_for_parity(RetinaFace(cfg=cfg_re50, mode="train"), seed=11)
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(3)) * 50
    blocks = ("layer1.0.", "layer2.0.", "layer2.1.")
    sd = {k[5:]: v.clone() for k, v in m.state_dict().items() if k.startswith("body.")
          and (k.startswith("body.conv1") or k.startswith("body.bn1")
               or any(k.startswith("body." + b) for b in blocks))}

    def ref(dtype):
        P = {k: (v.to(dtype).requires_grad_(True) if v.is_floating_point() and "running" not in k
                 else (v.to(dtype) if v.is_floating_point() else v)) for k, v in sd.items()}
        ctx = model_ref.Ctx(P, True)
        with kk.replay():
            s = model_ref.kink(ctx.bn(ctx.conv(x.to(dtype), "conv1", 2, 3), "bn1"), "relu")
            s = model_ref.maxpool(s)
            for b in blocks:
                st = 2 if b == "layer2.0." else 1
                o = model_ref.kink(ctx.bn(ctx.conv(s, b + "conv1"), b + "bn1"), "relu")
                o = model_ref.kink(ctx.bn(ctx.conv(o, b + "conv2", st, 1), b + "bn2"), "relu")
                o = ctx.bn(ctx.conv(o, b + "conv3"), b + "bn3")
                idn = s if b == "layer2.1." else ctx.bn(ctx.conv(s, b + "downsample.0", st),
                                                         b + "downsample.1")
                s = model_ref.kink(o + idn, "relu")
        assert not kk.unmatched, kk.unmatched
        w = torch.randn(s.shape, generator=torch.Generator().manual_seed(8)).to(dtype)
        (s * w).sum().backward()
        return s.detach(), w, {k: p.grad for k, p in P.items()
                               if isinstance(p, torch.Tensor) and p.grad is not None}

    kk = Kinks()
    body = m.to(cuda).train().body
    with kk.record():
        s = T.bn_act(T.conv(x.to(cuda), body.conv1, 2, 3, nchw_in=True), body.bn1, "relu")
        s = T.MaxPoolFn.apply(s)
        for blk in (body.layer1[0], body.layer2[0], body.layer2[1]):
            s = T._r50_block(blk, s)
    y64, w, g64 = ref(torch.float64)
    _, _, g32 = ref(torch.float32)
    y = s.permute(0, 3, 1, 2)
    assert rel_err(y.detach(), y64) < 1e-4
    (y * w.float().to(cuda)).sum().backward()
    named = dict(body.named_parameters())
    bad = []
    for k, rg in g64.items():
        if k.endswith("conv1.bias"):
            continue
        e, e32 = _fro(named[k].grad, rg), _fro(g32[k], rg)
        if e > max(1e-4, 4 * e32):
            bad.append((e, e32, k))
    assert len(g64) > 30 and not bad, sorted(bad)[-5:]


@pytest.mark.gpu
def test_train_r50_bn3_link(cuda, monkeypatch):
    """bn3's backward taken from the next bottleneck's conv1 data gradient
    (jabd_conv_bn_bwd_sums_res_f32 writes dz = dout * [out > 0] and the
    BatchNorm sums; JABD_R50_BN3_LINK) against the unlinked form
    (jabd_bn_act_bwd_ex_f32 on dout) over layer1.0 (downsample) -> layer1.1
    -> layer1.2 -> layer2.0 (stride-2 downsample): the three links are
    taken, and every gradient and the input gradient agree to fp32
    reassociation (1e-5).

    The link hands a block dz in place of the true gradient of its output,
    so it is sound only while that output has one consumer and no observer.
    Every use below is judged, link on and link off, against an fp64
    restatement of the chain (model_ref.Ctx, the HIP forward's masks
    replayed): relative Frobenius error <= max(1e-4, 4 x the fp32
    restatement's error), and on against off <= 1e-5:
      plain   the chain, one backward: 3 links;
      (a)     a second backward over the retained graph: .grad is exactly
              twice the single backward's, 3 more links;
      (b)     layer1.1's output also feeds (out * w2).sum(), that consumer
              created before the next block (the engine adds its gradient
              into dz in place: same tensor, other values) and after it
              (another tensor arrives): the link into layer1.1 is refused;
      (c)     retain_grad() on that output in a linked chain (its producer of
              dz sees the request and writes the true gradient), and
              torch.autograd.grad(loss, out) in a chain built as a direct
              caller builds it, _r50_block(blk, x): both give the true
              gradient.  (A caller that passes link=True vouches that nothing
              observes the output; only _train_forward does.)"""
    from jabd_amd import train as T
    from nets.retinaface_eca_nonlocal import RetinaFace
    from utils.config import cfg_re50
    m = init_for_parity(RetinaFace(cfg=cfg_re50, mode="train"), seed=5)
    names = ("layer1.0.", "layer1.1.", "layer1.2.", "layer2.0.")
    sd = {k[5:]: v.clone() for k, v in m.state_dict().items()
          if any(k.startswith("body." + b) for b in names)}
    body = m.to(cuda).train().body
    blocks = (body.layer1[0], body.layer1[1], body.layer1[2], body.layer2[0])
    x0 = torch.randn(2, 37, 29, 64, generator=torch.Generator().manual_seed(4))
    g = torch.Generator().manual_seed(6)
    w = torch.randn(2, 19, 15, 512, generator=g)
    w2 = torch.randn(2, 37, 29, 256, generator=g)
    wg, w2g = w.to(cuda), w2.to(cuda)
    calls = []
    real = T._dgrad_1x1_res_bn3

    def spy(*a):
        r = real(*a)
        calls.append(r[1] is not None)
        return r
    monkeypatch.setattr(T, "_dgrad_1x1_res_bn3", spy)

    def chain(second=None, linked=True, watch=False):
        """-> (x, out of layer1.1, final out, the second consumer's loss)."""
        body.zero_grad()
        x = x0.to(cuda).requires_grad_(True)
        extra = None
        with T._BatchCounts():
            s = x
            for i, blk in enumerate(blocks):
                s = T._r50_block(blk, s, link=True) if linked else T._r50_block(blk, s)
                if i == 1:
                    mid = s
                    if watch:
                        mid.retain_grad()
                    if second == "before":
                        extra = (mid * w2g).sum()
        if second == "after":
            extra = (mid * w2g).sum()
        return x, mid, s, extra

    def grads(x):
        torch.cuda.synchronize()
        out = {k: p.grad.clone() for k, p in body.named_parameters() if p.grad is not None}
        out["x"] = x.grad.clone()
        return out

    def taken(fn):
        n = T.LINKS_TAKEN[0]
        r = fn()
        return r, T.LINKS_TAKEN[0] - n

    kk = Kinks()
    res = {}
    for link in (True, False):
        monkeypatch.setattr(T, "R50_BN3_LINK", link)
        r = res[link] = {}
        del calls[:]
        if link:
            with kk.record():
                x, mid, s, _ = chain()
        else:
            x, mid, s, _ = chain()
        loss = (s * wg).sum()
        _, n = taken(lambda: loss.backward(retain_graph=True))
        assert n == (3 if link else 0)
        assert calls == ([True, True, True] if link else []), calls
        r["out"], r["plain"] = s.detach().clone(), grads(x)
        _, n = taken(lambda: loss.backward())                     # (a)
        assert n == (3 if link else 0)
        twice = grads(x)
        assert all(torch.equal(twice[k], 2 * r["plain"][k]) for k in twice)
        for second in ("before", "after"):                        # (b)
            x, mid, s, extra = chain(second)
            _, n = taken(lambda: ((s * wg).sum() + extra).backward())
            assert n == (2 if link else 0), (second, n)
            r[second] = grads(x)
        x, mid, s, _ = chain(watch=True)                          # (c)
        _, n = taken(lambda: (s * wg).sum().backward())
        assert n == (2 if link else 0)
        r["retain_grad"] = mid.grad.clone()
        x, mid, s, _ = chain(linked=False)
        (r["autograd.grad"],), n = taken(lambda: torch.autograd.grad((s * wg).sum(), mid))
        assert n == 0

    def ref(dtype):
        P = {k: (v.to(dtype).requires_grad_(True) if v.is_floating_point() and "running" not in k
                 else (v.to(dtype) if v.is_floating_point() else v.clone())) for k, v in sd.items()}
        ctx = model_ref.Ctx(P, True)
        x = x0.permute(0, 3, 1, 2).to(dtype).requires_grad_(True)
        with kk.replay(dtype):
            s = x
            for i, b in enumerate(names):
                st = 2 if b == "layer2.0." else 1
                o = model_ref.kink(ctx.bn(ctx.conv(s, b + "conv1"), b + "bn1"), "relu")
                o = model_ref.kink(ctx.bn(ctx.conv(o, b + "conv2", st, 1), b + "bn2"), "relu")
                o = ctx.bn(ctx.conv(o, b + "conv3"), b + "bn3")
                idn = ctx.bn(ctx.conv(s, b + "downsample.0", st), b + "downsample.1") \
                    if b.endswith(".0.") else s
                s = model_ref.kink(o + idn, "relu")
                if i == 1:
                    mid = s
        assert not kk.unmatched, kk.unmatched
        keys = [k for k, p in P.items() if isinstance(p, torch.Tensor) and p.requires_grad]
        leaves = [P[k] for k in keys] + [x]
        main = (s * w.permute(0, 3, 1, 2).to(dtype)).sum()
        extra = (mid * w2.permute(0, 3, 1, 2).to(dtype)).sum()
        gm = torch.autograd.grad(main, leaves + [mid], retain_graph=True)
        gb = torch.autograd.grad(main + extra, leaves)
        nhwc = lambda t: t.permute(0, 2, 3, 1)   # noqa: E731
        plain = dict(zip(keys, gm[:-2]), x=nhwc(gm[-2]))
        return {"out": nhwc(s.detach()), "plain": plain, "mid": nhwc(gm[-1]),
                "second": dict(zip(keys, gb[:-1]), x=nhwc(gb[-1]))}

    r64, r32 = ref(torch.float64), ref(torch.float32)
    assert kk.matched >= 12

    def judge(got, want, want32, what):
        e, e32 = _fro(got, want), _fro(want32, want)
        assert e <= max(1e-4, 4 * e32), f"{what}: {e:.2e} (fp32 restatement {e32:.2e})"

    assert torch.equal(res[True]["out"], res[False]["out"])
    assert rel_err(res[True]["out"], r64["out"]) < 1e-4
    for link in (True, False):
        r = res[link]
        assert len(r["plain"]) == len(r64["plain"]) > 30
        for case, want in (("plain", "plain"), ("before", "second"), ("after", "second")):
            for k, v in r[case].items():
                judge(v, r64[want][k], r32[want][k], f"link {link} {case} {k}")
        for case in ("retain_grad", "autograd.grad"):
            judge(r[case], r64["mid"], r32["mid"], f"link {link} {case}")
    for case in ("plain", "before", "after"):
        bad = [(rel_err(res[True][case][k], v), case, k) for k, v in res[False][case].items()
               if rel_err(res[True][case][k], v) > 1e-5]
        assert not bad, sorted(bad)[-5:]
    for case in ("retain_grad", "autograd.grad"):
        assert rel_err(res[True][case], res[False][case]) <= 1e-5, case


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["mnv3", "r50"])
def test_train_head_parity(cuda, kind):
    """ECA -> FPN(+NLM) -> SSH -> heads sub-graph alone (backbone features as
    leaves), gradients vs the fp64 oracle."""
    from jabd_amd import train as T
    if kind == "mnv3":
        from nets.retinaface_r import RetinaFace
        from utils.config import cfg_mnet as cfg
        chans, names, nlm_name, leaky = (40, 80, 160), ("eca_40", "eca_80", "eca_160"), "fpn.nlm.", 0.1
    else:
        from nets.retinaface_eca_nonlocal import RetinaFace
        from utils.config import cfg_re50 as cfg
        chans, names, nlm_name, leaky = (512, 1024, 2048), ("eca_64", "eca_128", "eca_256"), "fpn.Nlm.", 0.0
    m = init_for_parity(RetinaFace(cfg=cfg, mode="train"), seed=9)
    g = torch.Generator().manual_seed(4)
    feats = [torch.randn(2, c, s, s, generator=g) for c, s in zip(chans, (16, 8, 4))]
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    kk = Kinks()
    mg = m.to(cuda).train()
    fg = [f.permute(0, 2, 3, 1).contiguous().to(cuda).requires_grad_() for f in feats]
    nlm = mg.fpn.nlm if kind == "mnv3" else mg.fpn.Nlm
    with kk.record():
        out = T._head(mg, fg, names, nlm)
    P = {k: (v.double().requires_grad_(True) if v.is_floating_point() and "running" not in k
             else (v.double() if v.is_floating_point() else v)) for k, v in sd.items()}
    fr = [f.double().requires_grad_() for f in feats]
    ctx = model_ref.Ctx(P, True)
    with kk.replay():
        fe = [model_ref.eca(ctx, f, n, "sigmoid") for f, n in zip(fr, names)]
        f3 = model_ref.fpn(ctx, fe, leaky, nlm_name)
        f3 = [model_ref.ssh(ctx, model_ref.eca(ctx, f3[i], "eca_fpn", "sigmoid"), f"ssh{i + 1}.",
                            leaky) for i in range(3)]
        ref = model_ref.heads(ctx, f3, "train")
    assert not kk.unmatched and kk.matched >= 12, (kk.matched, kk.unmatched)
    wts = [torch.randn(r.shape, generator=g, dtype=torch.float64) for r in ref]
    sum(((r * w).sum() for r, w in zip(ref, wts))).backward()
    sum(((o * w.float().to(cuda)).sum() for o, w in zip(out, wts))).backward()
    for o, r in zip(out, ref):
        assert rel_err(o.detach(), r.detach()) < 1e-3
    errs = [(rel_err(f.grad.permute(0, 3, 1, 2), r.grad), f"feat{i}") for i, (f, r) in
            enumerate(zip(fg, fr))]
    named = dict(mg.named_parameters())
    for k, p in P.items():
        if isinstance(p, torch.Tensor) and p.requires_grad and p.grad is not None:
            if k.endswith("f_key.bias"):
                continue
            errs.append((rel_err(named[k].grad, p.grad), k))
    errs.sort(reverse=True)
    assert errs[0][0] < 2e-3, errs[:6]
