"""The ring kernel of the fp32 input gradient (csrc/conv_ring.hip; tuning key dgrad_ring): reflection halo of the 3x3 and 4x4 stride-2 layers
whose interior runs through Winograd, and the band of the sub-pixel (upsample + 5x5) layers.  Every case goes through aclgan_conv2d_dgrad at
channel counts that send the interior through Winograd, so the ring launch is what adds the frame, and is compared with autograd of
oracle.conv_block (as tests/test_gpu_ops.py::test_conv_dgrad), over the whole dx and over the frame alone.
The maps are small, and at such sizes the cost model of the 4x4 stride-2 layers prefers the direct interior, whose split-K slices meet in
atomics (not reproducible run to run, so no bitwise statement about the interior could hold): the tests set wino_fused = 2, which takes
the fused Winograd kernel wherever the shape allows it, as the benchmarked shapes do by themselves."""
import ctypes as C

import pytest
import torch

from oracle import aclgan_oracle as O

pytestmark = pytest.mark.gpu

TOL = 2e-4      # tests/test_gpu_ops.py: fp32 on both sides, differences are summation order

# (B, Hi, Wi, Ci, Co, k, s, p, up)
CASES = [
    (2, 8, 8, 128, 128, 3, 1, 1, 0),       # 3x3: one tile block, all four sides and corners in one 64-row tile
    (1, 12, 20, 256, 128, 3, 1, 1, 0),     # 3x3: non-square map, ragged segments
    (2, 16, 16, 64, 128, 4, 2, 1, 0),      # 4x4 stride 2: parity-class lines of unequal length
    (1, 20, 12, 128, 256, 4, 2, 1, 0),
    (2, 8, 8, 128, 64, 5, 1, 2, 1),        # upsample + 5x5: the band and its corner squares, four phases
    (1, 12, 8, 256, 128, 5, 1, 2, 1),
]


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib
    return _lib


_REF = {}


def _reference(case):
    """(dy NHWC, w OHWI, dx of the oracle NCHW, accumulate base NHWC), computed once per case on the CPU and never written again"""
    if case not in _REF:
        from gpu_util import nhwc, ohwi
        B, Hi, Wi, Ci, Co, k, s, p, up = case
        g = torch.Generator().manual_seed(1)
        x = (torch.rand(B, Ci, Hi, Wi, generator=g) * 2 - 1).requires_grad_(True)
        w = torch.randn(Co, Ci, k, k, generator=g) / (Ci * k * k) ** 0.5
        b = torch.randn(Co, generator=g) * 0.1
        y = O.conv_block(x, w, b, s, p, "none", upsample=bool(up))
        dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(5))
        y.backward(dy)
        base = torch.randn(B, Hi, Wi, Ci, generator=torch.Generator().manual_seed(6))
        _REF[case] = (nhwc(dy), ohwi(w.detach()), x.grad.detach().clone(), base)
    return _REF[case]


def _frame(t_nchw):
    """the outer 3 rows and columns (everything else zeroed)"""
    f = t_nchw.clone()
    f[:, :, 3:-3, 3:-3] = 0
    return f


def _tune(L, key, value):
    prev = C.c_int(0)
    L.check(L.lib.aclgan_tuning(key, value, C.byref(prev)), "tuning")
    return prev.value


def _run(L, case, accumulate):
    from gpu_util import conv_desc, gpu_conv_dgrad
    B, Hi, Wi, Ci, Co, k, s, p, up = case
    dy, w, _, base = _reference(case)
    d = conv_desc(L, B, Hi, Wi, Ci, Co, k, s, p, up, "none")
    dx = gpu_conv_dgrad(L, d, dy.cuda(), w.cuda(), accumulate_into=base.clone().cuda() if accumulate else None)
    torch.cuda.synchronize()
    return dx.cpu()


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_dgrad_ring(L, case, accumulate):
    from gpu_util import deterministic_mode, nchw, rel_err
    _, _, ref, base = _reference(case)
    prev = _tune(L, b"dgrad_ring", 1)
    prev_fused = _tune(L, b"wino_fused", 2)
    try:
        with deterministic_mode(L, False):
            new = _run(L, case, accumulate)
            _tune(L, b"dgrad_ring", 0)
            old = _run(L, case, accumulate)
        got = nchw(new) - (nchw(base) if accumulate else 0)
        e_all, e_frame = rel_err(got, ref), rel_err(_frame(got), _frame(ref))
        ab = ((new.double() - old.double()).abs().max() / old.double().abs().max()).item()
        print("case %s accumulate %d: rel_err %.3g, frame %.3g, ring vs old launches %.3g" % (case, accumulate, e_all, e_frame, ab))
        assert e_all < TOL
        assert e_frame < TOL          # the frame alone: the interior must not dilute a ring error
        assert ab <= 1e-5             # only the order of the atomics differs
        assert torch.equal(new[:, 3:-3, 3:-3], old[:, 3:-3, 3:-3])      # the interior never sees the ring: bit for bit
        # the deterministic plan does not come through the ring kernel: same launches whatever the switch says, same bits call to call
        with deterministic_mode(L, True):
            counts, outs = [], []
            for ring in (1, 0, 1):
                _tune(L, b"dgrad_ring", ring)
                n0 = L.lib.aclgan_launch_count()
                outs.append(_run(L, case, accumulate))
                counts.append(L.lib.aclgan_launch_count() - n0)
            assert counts[0] == counts[1] == counts[2], counts
            assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
            assert rel_err(nchw(outs[0]) - (nchw(base) if accumulate else 0), ref) < TOL
    finally:
        _tune(L, b"wino_fused", prev_fused)
        _tune(L, b"dgrad_ring", prev)
