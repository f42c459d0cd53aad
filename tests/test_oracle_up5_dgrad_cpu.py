"""The oracle's two 16-bit contracts for the input gradient of the sub-pixel ("Upsample(2) + 5x5") layers (oracle.compute_dtype(up5_dgrad=)).

The default plan computes the interior of that gradient through the merged 3x3 phase filters, rounded to the 16-bit type, and the output
ring of width 2 through the rounded 5x5 (conv_fast16.hip dgrad16_t).  The deterministic plan runs the plain upsample + 5x5 convolution
with the rounded 5x5 everywhere.  The merged filters are sums of up to four taps, so their rounding differs from the taps' own.

Checked here: the default is "merged" and gives the same bits as the statement of that contract restated below (what the oracle computed
before the option existed); "plain" gives the same bits as _plain_conv on rounded weights with the rounded gradient; the two differ; the
forward and the weight gradient do not depend on the option."""
import pytest
import torch
import torch.nn.functional as F

from oracle import aclgan_oracle as O

B, CI, CO, H, W = 2, 32, 32, 6, 7       # channel counts that take the 16-bit kernels in all three passes


def _operands(seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, CI, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(CO, CI, 5, 5, generator=g, dtype=torch.float64) * 0.05
    b = torch.randn(CO, generator=g, dtype=torch.float64) * 0.1
    dy = torch.randn(B, CO, 2 * H, 2 * W, generator=g, dtype=torch.float64) * 1e-3
    return x, w, b, dy


def _run(x, w, b, dy):
    """forward and both gradients of one sub-pixel layer through the oracle's 16-bit conv"""
    xv = x.clone().requires_grad_(True)
    wv = w.clone().requires_grad_(True)
    y = O._ConvQ.apply(xv, wv, b, 1, 2, True, True, True, True)
    dx, dw = torch.autograd.grad(y, [xv, wv], dy)
    return y.detach(), dx, dw


def _merged_statement(x, w, dy):
    """the merged-filter contract as the oracle stated it before the option: ring through the rounded 5x5, interior per output phase
    through the rounded merged 3x3 filters, both against the rounded gradient"""
    xv = x.clone().requires_grad_(True)
    dyq = O._qg(dy)
    ring = torch.ones_like(dyq)
    ring[:, :, 2: 2 * H - 2, 2: 2 * W - 2] = 0
    tot = (O._plain_conv(xv, O._q(w), 1, 2, True) * (dyq * ring)).sum()
    for py in (0, 1):
        for px in (0, 1):
            tot = tot + (F.conv2d(xv, O._q(O._up5_merged(w, py, px))) * dyq[:, :, 2 + py: 2 * H - 2: 2, 2 + px: 2 * W - 2: 2]).sum()
    return torch.autograd.grad(tot, xv)[0]


def _plain_statement(x, w, dy):
    xv = x.clone().requires_grad_(True)
    return torch.autograd.grad(O._plain_conv(xv, O._q(w), 1, 2, True), xv, O._qg(dy))[0]


@pytest.mark.parametrize("dt,scale", [("bf16", 1.0), ("fp16", 65536.0)])
def test_up5_dgrad_contracts(dt, scale):
    x, w, b, dy = _operands(5)
    with O.compute_dtype(dt, loss_scale=scale):
        assert O._QUP5D == "merged"
        default = _run(x, w, b, dy)
        merged_ref = _merged_statement(x, w, dy)
        plain_ref = _plain_statement(x, w, dy)
    with O.compute_dtype(dt, loss_scale=scale, up5_dgrad="merged"):
        merged = _run(x, w, b, dy)
    with O.compute_dtype(dt, loss_scale=scale, up5_dgrad="plain"):
        assert O._QUP5D == "plain"
        plain = _run(x, w, b, dy)
    assert O._QUP5D == "merged"                                 # restored on exit
    # the default is the merged contract, bit for bit
    assert torch.equal(default[1], merged_ref)
    for a, c in zip(default, merged):
        assert torch.equal(a, c)
    # "plain" is the rounded 5x5 on the upsampled grid, bit for bit
    assert torch.equal(plain[1], plain_ref)
    # the two contracts differ (the merged filters round differently from their taps) -- by rounding only
    assert not torch.equal(plain[1], merged_ref)
    assert (plain[1] - merged_ref).abs().max() <= 0.05 * merged_ref.abs().max()
    # forward and weight gradient are the same in both plans
    assert torch.equal(plain[0], default[0]) and torch.equal(plain[2], default[2])


def test_up5_dgrad_rejects_unknown_plans():
    with pytest.raises(ValueError):
        O.compute_dtype("bf16", up5_dgrad="phases")
