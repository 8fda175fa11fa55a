"""jabd_expand_dw_select with a form that does not exist (3 and 4 were removed,
7 never existed) stores 0: the default kernel runs and computes what it
computes under select(0)."""
import pytest
import torch


@pytest.mark.gpu
def test_removed_forms_run_the_default_kernel(cuda):
    from jabd_amd import _lib
    from jabd_amd import functional as F
    k, cin, E, s = 3, 16, 16, 1
    B, H, W = 1, 1, 2
    g = torch.Generator().manual_seed(3)
    conv1 = torch.nn.Conv2d(cin, E, 1)
    with torch.no_grad():
        conv1.weight.copy_(torch.randn(conv1.weight.shape, generator=g) / cin ** 0.5)
        conv1.bias.copy_(0.3 * torch.randn(E, generator=g))
    pk = F.pack_conv(conv1.to(cuda))
    dw_w = (torch.randn(k * k, E, generator=g) / k).to(cuda)
    dw_b = (0.3 * torch.randn(E, generator=g)).to(cuda)
    x = torch.randn(B, H, W, cin, generator=g).to(cuda)
    select = _lib.lib().jabd_expand_dw_select
    try:
        select(0)
        want = F.expand_dw(x, pk, dw_w, dw_b, k, s, act="relu")
        for form in (3, 4, 7):
            select(form)
            _lib.launch_log_reset()
            got = F.expand_dw(x, pk, dw_w, dw_b, k, s, act="relu")
            assert _lib.launch_log() == [("expand_dw", 0)], (form, _lib.launch_log())
            assert select(0) == 0, form   # the form was stored as 0
            for a, b in zip(got, want):
                assert torch.equal(a, b), form
    finally:
        select(0)
