"""Convolution kernels at channel counts off the power-of-two lattice: 12, 48, 96, 160, 192, 320, 384, 768 -- a 128-wide N tile followed by a
partial one, three or more whole tiles, the tile shapes launch_wgrad_kc_any / launch_wgrad16_any fall through to -- and at 512, which no
operator test of the 3x3 / sub-pixel paths reached.  Method and bounds of tests/test_gpu_ops.py (fp32: the fp64 oracle on the same operands,
2e-4 max-abs / max|ref|, summation order only) and tests/test_gpu_ops16.py (16-bit: the fp64 oracle on the rounded operands, 2e-4; run
twice, same bits).  Every shape goes through every entry point whose own predicate admits it; ENTRY pins which those are, so a silently
narrowed predicate shows up.  Run with -s for the measured errors (profiles/arch_space.md)."""
import ctypes as C

import pytest
import torch

from oracle import aclgan_oracle as O
from gpu_util import conv_desc, deterministic_mode, gpu_conv_dgrad, gpu_conv_fwd, gpu_conv_wgrad, nchw, nhwc, ohwi, out_hw, rel_err

pytestmark = pytest.mark.gpu

TOL = 2e-4            # tests/test_gpu_ops.py: TOL; the largest K here is 16 * 768 = 12288
EXACT_TOL = 2e-4      # tests/test_gpu_ops16.py: EXACT_TOL
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib
    return _lib


# (B, Hi, Wi, Ci, Co, k, s, p, up, act)
F32_CASES = [
    (2, 12, 20, 48, 96, 4, 2, 1, 0, "lrelu"),      # dis.dim 48, layer 1
    (2, 16, 16, 96, 192, 4, 2, 1, 0, "lrelu"),     # dis.dim 96: 128-wide N tile + a partial one
    (1, 8, 8, 192, 384, 4, 2, 1, 0, "lrelu"),      # three whole 128-wide tiles; weight gradient on 128 x 64 tiles with Cin 192
    (2, 6, 10, 384, 768, 4, 2, 1, 0, "lrelu"),     # K = 16 * 384, split-K
    (2, 32, 32, 3, 96, 4, 2, 1, 0, "lrelu"),       # thin-input first layer, Cout != 64
    (2, 20, 28, 6, 48, 4, 2, 1, 0, "lrelu"),
    (2, 20, 28, 6, 12, 4, 2, 1, 0, "lrelu"),       # dis.dim 12
    (2, 4, 4, 768, 1, 1, 1, 0, 0, "none"),         # 1x1 head of dis.dim 96
    (3, 2, 2, 96, 1, 1, 1, 0, 0, "none"),
    (1, 8, 8, 512, 512, 3, 1, 1, 0, "none"),       # gen.dim 128 ResBlock
    (2, 8, 12, 512, 512, 3, 1, 1, 0, "relu"),
    (1, 16, 16, 512, 256, 5, 1, 2, 1, "none"),     # gen.dim 128 sub-pixel layer
    (2, 12, 20, 96, 192, 3, 1, 1, 0, "relu"),
    (2, 12, 20, 192, 96, 3, 1, 1, 0, "none"),
]
FWD16_CASES = [
    (2, 16, 16, 96, 192, 4, 2, 1, 0, "none"), (3, 12, 20, 160, 96, 3, 1, 1, 0, "none"), (2, 8, 8, 192, 384, 4, 2, 1, 0, "none"),
    (2, 8, 8, 384, 768, 4, 2, 1, 0, "none"), (2, 9, 13, 96, 96, 5, 1, 2, 1, "none"), (1, 10, 6, 96, 32, 3, 1, 1, 0, "none"),
]
WGRAD16_CASES = [
    (2, 16, 16, 192, 384, 4, 2, 1, 0, "none"),     # 128 x 64 tiles with Cin 192
    (2, 16, 16, 384, 192, 4, 2, 1, 0, "none"),     # 64 x 128 tiles with Cout 192
    (2, 12, 20, 192, 192, 3, 1, 1, 0, "none"),     # 64 x 64 tiles, three each way
    (2, 12, 20, 320, 64, 3, 1, 1, 0, "none"),      # 64 x 64 tiles, five along N
]
# case -> (aclgan_conv16_eligible forward / input gradient / weight gradient, aclgan_conv16s_ok forward / backward): the predicates' answers
# when this module was written (host code: the same without a GPU)
ENTRY = {
    F32_CASES[0]: ((0, 0, 0), (0, 0)), F32_CASES[1]: ((1, 1, 0), (0, 0)), F32_CASES[2]: ((1, 1, 1), (0, 1)), F32_CASES[3]: ((1, 1, 1), (0, 1)),
    F32_CASES[4]: ((0, 0, 0), (0, 0)), F32_CASES[5]: ((0, 0, 0), (0, 0)), F32_CASES[6]: ((0, 0, 0), (0, 0)), F32_CASES[7]: ((0, 0, 0), (0, 0)),
    F32_CASES[8]: ((0, 0, 0), (0, 0)), F32_CASES[9]: ((1, 1, 1), (0, 1)), F32_CASES[10]: ((1, 1, 1), (0, 1)), F32_CASES[11]: ((1, 1, 1), (0, 0)),
    F32_CASES[12]: ((1, 1, 0), (0, 0)), F32_CASES[13]: ((1, 1, 0), (0, 0)),
    FWD16_CASES[0]: ((1, 1, 0), (0, 0)), FWD16_CASES[1]: ((1, 1, 0), (0, 0)), FWD16_CASES[2]: ((1, 1, 1), (0, 1)),
    FWD16_CASES[3]: ((1, 1, 1), (0, 1)), FWD16_CASES[4]: ((1, 1, 0), (0, 0)), FWD16_CASES[5]: ((1, 1, 0), (0, 0)),
    WGRAD16_CASES[0]: ((1, 1, 1), (0, 1)), WGRAD16_CASES[1]: ((1, 1, 1), (0, 1)), WGRAD16_CASES[2]: ((1, 1, 1), (0, 1)),
    WGRAD16_CASES[3]: ((1, 1, 1), (0, 1)),
}


def _id(case):
    return "x".join(str(v) for v in case)


@pytest.mark.parametrize("case", list(ENTRY), ids=_id)
def test_entry_points_admit_what_they_admitted(L, case):
    d = conv_desc(L, *case)
    got = (tuple(L.lib.aclgan_conv16_eligible(C.byref(d), w) for w in (0, 1, 2)), tuple(L.lib.aclgan_conv16s_ok(C.byref(d), w) for w in (0, 1)))
    assert got == ENTRY[case]
    # a scratch size for exactly the eligible 16-bit passes
    for w, fn in enumerate((L.lib.aclgan_conv2d_fwd16_scratch_bytes, L.lib.aclgan_conv2d_dgrad16_scratch_bytes, L.lib.aclgan_conv2d_wgrad16_scratch_bytes)):
        assert got[0][w] or fn(C.byref(d)) == 0, (w, fn(C.byref(d)))
    assert (L.lib.aclgan_conv2d_dgrad16s_scratch_bytes(C.byref(d)) > 0) == bool(got[1][1])
    assert got[1][0] or L.lib.aclgan_conv2d_fwd16s_stats_chunk(C.byref(d)) == 0


_REF = {}


def _ref32(case):
    """operands and the fp64 oracle of one fp32 case, computed once: y (with the activation), dx and dw / db of the linear layer"""
    if case not in _REF:
        B, Hi, Wi, Ci, Co, k, s, p, up, act = case
        g = torch.Generator().manual_seed(17)
        x = torch.randn(B, Ci, Hi, Wi, generator=g)
        w = torch.randn(Co, Ci, k, k, generator=g) * (2.0 / (Ci * k * k)) ** 0.5
        b = torch.randn(Co, generator=g) * 0.1
        xd, wd, bd = (t.double().requires_grad_(True) for t in (x, w, b))
        with torch.no_grad():
            y = O.conv_block(xd, wd, bd, s, p, act, upsample=bool(up))
        y_lin = O.conv_block(xd, wd, bd, s, p, "none", upsample=bool(up))
        dy = torch.randn(y_lin.shape, generator=g)
        y_lin.backward(dy.double())
        base = torch.randn(B, Hi, Wi, Ci, generator=g)
        _REF[case] = dict(x=x, w=w, b=b, dy=dy, base=base, y=y, dx=xd.grad, dw=ohwi(wd.grad), db=bd.grad)
    return _REF[case]


def _check32(L, case, tag, errs, raw=None):
    """forward, input gradient plain and accumulating onto a nonzero base, weight and bias gradient through the general entry points, as the
    switches stand; raw[tag] = (the forward's output, its launch count)"""
    B, Hi, Wi, Ci, Co, k, s, p, up, act = case
    r = _ref32(case)
    d = conv_desc(L, B, Hi, Wi, Ci, Co, k, s, p, up, act)
    dn = conv_desc(L, B, Hi, Wi, Ci, Co, k, s, p, up, "none")
    xg, wg, bg, dyg = nhwc(r["x"]).cuda(), ohwi(r["w"]).cuda(), r["b"].cuda(), nhwc(r["dy"]).cuda()
    e = {}
    n0 = L.lib.aclgan_launch_count()
    y = gpu_conv_fwd(L, d, xg, wg, bg)
    if raw is not None:
        raw[tag] = (y, L.lib.aclgan_launch_count() - n0)
    e["fwd"] = rel_err(nchw(y), r["y"])
    e["dgrad"] = rel_err(nchw(gpu_conv_dgrad(L, dn, dyg, wg)), r["dx"])
    acc = gpu_conv_dgrad(L, dn, dyg, wg, accumulate_into=r["base"].clone().cuda())
    e["dgrad+="] = rel_err(nchw(acc), nchw(r["base"]).double() + r["dx"])
    dw, db = gpu_conv_wgrad(L, dn, xg, dyg)
    e["wgrad"] = rel_err(dw, r["dw"])
    e["bgrad"] = rel_err(db, r["db"])
    errs[tag] = e
    return e


@pytest.mark.parametrize("plan", ["default", "deterministic"])
@pytest.mark.parametrize("case", F32_CASES, ids=_id)
def test_conv_fp32(L, case, plan):
    B, Hi, Wi, Ci, Co, k, s, p, up, act = case
    errs = {}
    with deterministic_mode(L, plan == "deterministic"):
        _check32(L, case, "as shipped", errs)
        fused_modes = (k == 3 and up == 0) or (k == 4 and s == 2) or up == 1
        if fused_modes:
            # 3x3: the three-launch Winograd pipeline (0) and the fused kernel forced on every eligible shape (2); 4x4 stride 2: the direct
            # kernels (0) and the four parity phases of the fused kernel where its predicate holds (2); sub-pixel: its four phases likewise
            old_f = L.lib.aclgan_set_tuning(b"wino_fused", 0); old_w = L.lib.aclgan_set_tuning(b"wino_wgrad_fused", 0)
            assert old_f >= 0 and old_w >= 0
            raw = {}
            try:
                for v in (0, 2):
                    assert L.lib.aclgan_set_tuning(b"wino_fused", v) >= 0 and L.lib.aclgan_set_tuning(b"wino_wgrad_fused", v) >= 0
                    _check32(L, case, "wino_fused %d" % v, errs, raw)
            finally:
                L.lib.aclgan_set_tuning(b"wino_fused", old_f); L.lib.aclgan_set_tuning(b"wino_wgrad_fused", old_w)
            # the forced mode did reach the other kernel where the fused kernel's shape rule holds (csrc/conv_wino_fused.hip: K side a multiple
            # of 16, output side of 64; stride 2: an even map of 8 x 8 at least): other bits than the pipeline / the direct kernels gave, as
            # tests/test_gpu_ops.py asserts it for the stride-2 phases.  (The fused weight gradient takes only maps 16 wide and more,
            # wg_shape_ok: none of these shapes, so both settings run the same weight gradient.)
            (y0, n0), (y2, n2) = raw["wino_fused 0"], raw["wino_fused 2"]
            if Ci % 16 == 0 and Co % 64 == 0 and (k != 4 or (Hi % 2 == 0 and Wi % 2 == 0 and min(Hi, Wi) >= 8)):
                assert not torch.equal(y2, y0), "the forced mode did not take the fused kernel (launch counts %d and %d)" % (n2, n0)
        if k == 3 and up == 0:
            # the fused kernel's own entry point: runs where it is eligible, refuses with a message elsewhere
            r = _ref32(case)
            xg, wg, bg = nhwc(r["x"]).cuda(), ohwi(r["w"]).cuda(), r["b"].cuda()
            Uf = torch.empty(36 * Co * Ci, device="cuda")
            y = torch.full((B, Hi, Wi, Co), float("nan"), device="cuda")
            rc = L.lib.aclgan_winograd_filter_frag(L.ptr(wg), L.ptr(Uf), Co, Ci, 0, L.stream_ptr())
            if rc == 0:
                rc = L.lib.aclgan_conv3x3_winograd_fused(L.ptr(xg), L.ptr(Uf), L.ptr(bg), L.ptr(y), B, Hi, Wi, Ci, Co, L.ACT[act], 1, 0, None, L.stream_ptr())
            eligible = Hi % 4 == 0 and Wi % 4 == 0 and Ci % 16 == 0 and Co % 64 == 0
            assert (rc == 0) == eligible, (rc, L.last_error())
            if rc == 0:
                errs["entry point"] = {"fwd": rel_err(nchw(y), r["y"])}
            else:
                assert L.last_error()
    worst = {}
    for e in errs.values():
        for k_, v in e.items():
            worst[k_] = max(worst.get(k_, 0.0), v)
    print("ops_widths fp32 %-13s %-38s worst over %s:" % (plan, _id(case), " / ".join(errs)), {k_: "%.2e" % v for k_, v in worst.items()})
    bad = {(tag, k_): v for tag, e in errs.items() for k_, v in e.items() if not v < TOL}
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------------
# 16-bit: the exact-operand contract of tests/test_gpu_ops16.py
# ---------------------------------------------------------------------------------------------------------------------------------
def _rounded(t, dt):
    return t.to(TDT[dt]).float()


def _tensors16(case, seed, grid):
    B, Hi, Wi, Ci, Co, k, s, p, up, act = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Ci, Hi, Wi, generator=g)
    if grid:   # weights on a 1/8 grid in [-3/8, 3/8]: the sub-pixel path rounds the MERGED phase filters, sums of up to 4 stay exactly representable
        w = torch.randint(-3, 4, (Co, Ci, k, k), generator=g).float() / 8.0
    else:
        w = torch.randn(Co, Ci, k, k, generator=g) * (2.0 / (Ci * k * k)) ** 0.5
    b = torch.randn(Co, generator=g) * 0.1
    return x, w, b


def _packs(L, w_ohwi, dt):
    Co, kh, kw, Ci = w_ohwi.shape
    w16 = torch.empty(w_ohwi.numel(), dtype=torch.int16, device="cuda")
    w16t = torch.empty(w_ohwi.numel(), dtype=torch.int16, device="cuda")
    L.check(L.lib.aclgan_pack_weights16(L.ptr(w_ohwi), L.ptr(w16), L.ptr(w16t), Co, kh * kw, Ci, L.DTYPE[dt], L.stream_ptr()), "pack_weights16")
    return w16, w16t


def _scratch(nbytes):
    return torch.empty(nbytes // 4 + 64, device="cuda") if nbytes else None


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("case", FWD16_CASES, ids=_id)
def test_conv_fwd16_dgrad16(L, case, dt):
    B, Hi, Wi, Ci, Co, k, s, p, up, act = case
    d = conv_desc(L, B, Hi, Wi, Ci, Co, k, s, p, up, act)
    assert L.lib.aclgan_conv16_eligible(C.byref(d), 0) == 1 and L.lib.aclgan_conv16_eligible(C.byref(d), 1) == 1
    x, w, b = _tensors16(case, 0, grid=bool(up))
    xr = _rounded(x, dt).double().requires_grad_(True)
    exact = O.conv_block(xr, _rounded(w, dt).double(), b.double(), s, p, act, upsample=bool(up))
    dy = torch.randn(exact.shape, generator=torch.Generator().manual_seed(5))
    exact.backward(_rounded(dy, dt).double())
    wg, xg, bg, dyg = ohwi(w).cuda(), nhwc(x).cuda(), b.cuda(), nhwc(dy).cuda()
    w16, w16t = _packs(L, wg, dt)
    Ho, Wo = out_hw(Hi, Wi, k, s, p, up)
    scr = _scratch(L.lib.aclgan_conv2d_fwd16_scratch_bytes(C.byref(d)))
    ys = []
    for rep in range(2):
        y = torch.full((B, Ho, Wo, Co), float("nan"), device="cuda")
        L.check(L.lib.aclgan_conv2d_fwd16(C.byref(d), L.DTYPE[dt], L.ptr(xg), L.ptr(wg), L.ptr(w16), L.ptr(bg), L.ptr(y), L.ptr(scr), L.stream_ptr()), "conv2d_fwd16")
        ys.append(y)
    scr = _scratch(L.lib.aclgan_conv2d_dgrad16_scratch_bytes(C.byref(d)))
    base = torch.randn(B, Hi, Wi, Ci, generator=torch.Generator().manual_seed(6))
    with deterministic_mode(L, True):      # (the halo ring of the default plan is mirrored in with atomics: same bits only under the ordered plan)
        scr_det = _scratch(L.lib.aclgan_conv2d_dgrad16_scratch_bytes(C.byref(d)))      # (the ordered plan has a scratch size of its own)
        dxs = []
        for rep in range(2):
            dx = torch.full((B, Hi, Wi, Ci), float("nan"), device="cuda")
            L.check(L.lib.aclgan_conv2d_dgrad16(C.byref(d), L.DTYPE[dt], L.ptr(dyg), L.ptr(wg), L.ptr(w16t), L.ptr(dx), 0, L.ptr(scr_det), L.stream_ptr()), "conv2d_dgrad16")
            dxs.append(dx)
    dxd = torch.full((B, Hi, Wi, Ci), float("nan"), device="cuda")
    L.check(L.lib.aclgan_conv2d_dgrad16(C.byref(d), L.DTYPE[dt], L.ptr(dyg), L.ptr(wg), L.ptr(w16t), L.ptr(dxd), 0, L.ptr(scr), L.stream_ptr()), "conv2d_dgrad16")
    acc = base.clone().cuda()
    L.check(L.lib.aclgan_conv2d_dgrad16(C.byref(d), L.DTYPE[dt], L.ptr(dyg), L.ptr(wg), L.ptr(w16t), L.ptr(acc), 1, L.ptr(scr), L.stream_ptr()), "conv2d_dgrad16")
    e = {"fwd": rel_err(nchw(ys[0]), exact.detach()), "dgrad ordered": rel_err(nchw(dxs[0]), xr.grad), "dgrad": rel_err(nchw(dxd), xr.grad),
         "dgrad+=": rel_err(nchw(acc), nchw(base).double() + xr.grad)}
    print("ops_widths %s %-34s" % (dt, _id(case)), {k_: "%.2e" % v for k_, v in e.items()})
    bad = {k_: v for k_, v in e.items() if not v < EXACT_TOL}
    assert not bad, bad
    assert torch.equal(ys[0], ys[1]) and torch.equal(dxs[0], dxs[1])


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("case", WGRAD16_CASES, ids=_id)
def test_conv_wgrad16(L, case, dt):
    B, Hi, Wi, Ci, Co, k, s, p, up, act = case
    d = conv_desc(L, B, Hi, Wi, Ci, Co, k, s, p, up, "none")
    assert L.lib.aclgan_conv16_eligible(C.byref(d), 2) == 1
    x, w, b = _tensors16(case, 2, False)
    wr = w.double().requires_grad_(True); br = b.double().requires_grad_(True)
    y = O.conv_block(_rounded(x, dt).double(), wr, br, s, p, "none")
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(7))
    y.backward(_rounded(dy, dt).double())
    db_ref = dy.double().sum(dim=(0, 2, 3))      # the bias gradient is summed from the UNROUNDED fp32 dy
    scr = _scratch(L.lib.aclgan_conv2d_wgrad16_scratch_bytes(C.byref(d)))
    xg, dyg = nhwc(x).cuda(), nhwc(dy).cuda()
    outs = []
    for rep in range(2):
        dw = torch.zeros(Co, k, k, Ci, device="cuda"); db = torch.zeros(Co, device="cuda")
        L.check(L.lib.aclgan_conv2d_wgrad16(C.byref(d), L.DTYPE[dt], L.ptr(xg), L.ptr(dyg), L.ptr(dw), L.ptr(db), L.ptr(scr), L.stream_ptr()), "conv2d_wgrad16")
        outs.append((dw, db))
    e = {"wgrad": rel_err(outs[0][0], ohwi(wr.grad)), "bgrad": rel_err(outs[0][1], db_ref)}
    print("ops_widths %s %-34s" % (dt, _id(case)), {k_: "%.2e" % v for k_, v in e.items()})
    bad = {k_: v for k_, v in e.items() if not v < EXACT_TOL}
    assert not bad, bad
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("stx,stdy", [(1, 1), (1, 0), (0, 1)])
@pytest.mark.parametrize("case", WGRAD16_CASES, ids=_id)
def test_conv_wgrad16_any_storage(L, case, dt, stx, stdy):
    """tests/test_gpu_ops16s.py::test_conv_wgrad16_any_storage: either operand stored in the 16-bit dtype"""
    B, Hi, Wi, Ci, Co, k, s, p, up, act = case
    d = conv_desc(L, B, Hi, Wi, Ci, Co, k, s, p, up, "none")
    x, w, b = _tensors16(case, 2, False)
    wr = w.double().requires_grad_(True); br = b.double().requires_grad_(True)
    y = O.conv_block(_rounded(x, dt).double(), wr, br, s, p, "none")
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(7))
    y.backward(_rounded(dy, dt).double())
    code = L.DTYPE[dt]
    xg = nhwc(x).cuda(); dyg = nhwc(dy).cuda()
    xs = xg.to(TDT[dt]) if stx else xg
    dys = dyg.to(TDT[dt]) if stdy else dyg
    scr = _scratch(L.lib.aclgan_conv2d_wgrad16_scratch_bytes(C.byref(d)))
    outs = []
    for rep in range(2):
        dw = torch.zeros(Co, k, k, Ci, device="cuda"); db = torch.zeros(Co, device="cuda")
        L.check(L.lib.aclgan_conv2d_wgrad16_st(C.byref(d), code, L.ptr(xs), code if stx else 0, L.ptr(dys), code if stdy else 0, L.ptr(dw), L.ptr(db),
                                               L.ptr(scr), L.stream_ptr()), "conv2d_wgrad16_st")
        outs.append((dw, db))
    # bias gradient: summed from dy as stored (fp32 dy: unrounded; 16-bit dy: the rounded values, which is what br.grad saw)
    want_db = br.grad if stdy else dy.double().sum(dim=(0, 2, 3))
    e = {"wgrad": rel_err(outs[0][0], ohwi(wr.grad)), "bgrad": rel_err(outs[0][1], want_db)}
    print("ops_widths %s x16 %d dy16 %d %-30s" % (dt, stx, stdy, _id(case)), {k_: "%.2e" % v for k_, v in e.items()})
    bad = {k_: v for k_, v in e.items() if not v < EXACT_TOL}
    assert not bad, bad
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# (B, Hi, Wi, Ci, Co, k, s, p): the 16-bit-storage kernels (csrc/conv_glds16.hip) with three N tiles and more
S16_CASES = [
    (2, 64, 64, 64, 192, 3, 1, 1),       # forward: Co / 64 = 3 tiles of 64
    (3, 20, 28, 192, 384, 4, 2, 1),      # input gradient: N = Cin = 192, stride-2 parity classes, ragged M
    (7, 30, 34, 192, 64, 3, 1, 1),       # input gradient: three N tiles over the padded grid, ragged last tile
    (2, 16, 16, 320, 192, 1, 1, 0),      # 1x1: forward with Co 192, input gradient with Cin 320 (five tiles)
]
S16_ENTRY = {S16_CASES[0]: (1, 1, 128), S16_CASES[1]: (0, 1, 0), S16_CASES[2]: (0, 1, 0), S16_CASES[3]: (1, 1, 128)}      # conv16s_ok fwd / bwd, stats chunk
ULP = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}      # tests/test_gpu_ops16s.py


@pytest.fixture(params=[1, 4], ids=["tile128", "tilemax"])
def tile(request, L):
    old = L.lib.aclgan_set_tuning(b"glds_tile", request.param)
    assert old >= 0
    yield request.param
    L.lib.aclgan_set_tuning(b"glds_tile", old)


@pytest.fixture(params=[0, 1], ids=["fold", "direct"])
def direct(request, L):
    old = L.lib.aclgan_set_tuning(b"dgrad16s_direct", request.param)
    assert old >= 0
    yield request.param
    L.lib.aclgan_set_tuning(b"dgrad16s_direct", old)


def _desc16s(L, case, act="none"):
    B, Hi, Wi, Ci, Co, k, s, p = case
    return conv_desc(L, B, Hi, Wi, Ci, Co, k, s, p, 0, act)


def test_storage_kernels_admit_what_they_admitted(L):
    for case, want in S16_ENTRY.items():
        d = _desc16s(L, case)
        got = (L.lib.aclgan_conv16s_ok(C.byref(d), 0), L.lib.aclgan_conv16s_ok(C.byref(d), 1), L.lib.aclgan_conv2d_fwd16s_stats_chunk(C.byref(d)))
        assert got == want, (case, got)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("case", [c for c in S16_CASES if S16_ENTRY[c][0]], ids=_id)
def test_conv_fwd16s(L, case, dt, tile):
    """tests/test_gpu_ops16s.py::test_conv_fwd16s and ::test_conv_fwd16s_epilogue_statistics"""
    B, Hi, Wi, Ci, Co, k, s, p = case
    d = _desc16s(L, case, "lrelu")
    assert L.lib.aclgan_conv16s_ok(C.byref(d), 0) == 1
    x, w, b = _tensors16(case + (0, "none"), 0, False)
    wg, bg = ohwi(w).cuda(), b.cuda()
    x16 = nhwc(x).cuda().to(TDT[dt])
    w16, _ = _packs(L, wg, dt)
    Ho, Wo = out_hw(Hi, Wi, k, s, p, 0)
    exact = O.conv_block(_rounded(x, dt).double(), _rounded(w, dt).double(), b.double(), s, p, "lrelu")
    code = L.DTYPE[dt]
    y32 = torch.full((B, Ho, Wo, Co), float("nan"), device="cuda")
    L.check(L.lib.aclgan_conv2d_fwd16s(C.byref(d), code, L.ptr(x16), L.ptr(w16), L.ptr(bg), L.ptr(y32), 0, L.stream_ptr()), "conv2d_fwd16s")
    e = rel_err(nchw(y32), exact)
    print("ops_widths %s fwd16s tile %d %-30s %.2e" % (dt, tile, _id(case), e))
    assert e < EXACT_TOL
    y16 = torch.full((B, Ho, Wo, Co), float("nan"), device="cuda").to(TDT[dt])
    L.check(L.lib.aclgan_conv2d_fwd16s(C.byref(d), code, L.ptr(x16), L.ptr(w16), L.ptr(bg), L.ptr(y16), code, L.stream_ptr()), "conv2d_fwd16s")
    assert torch.equal(y16, y32.to(TDT[dt]))           # the 16-bit output IS the fp32 output rounded once
    y2 = torch.empty_like(y32)
    L.check(L.lib.aclgan_conv2d_fwd16s(C.byref(d), code, L.ptr(x16), L.ptr(w16), L.ptr(bg), L.ptr(y2), 0, L.stream_ptr()))
    assert torch.equal(y32, y2)
    R = L.lib.aclgan_conv2d_fwd16s_stats_chunk(C.byref(d))
    if R > 0:      # the epilogue statistics: (mean, M2) chunk partials of the outputs AS STORED
        M = B * Ho * Wo
        for yst, T_ in ((0, torch.float32), (code, TDT[dt])):
            y = torch.full((B, Ho, Wo, Co), float("nan"), device="cuda").to(T_)
            stats = torch.full((M // R, Co, 2), float("nan"), device="cuda")
            L.check(L.lib.aclgan_conv2d_fwd16s_stats(C.byref(d), code, L.ptr(x16), L.ptr(w16), L.ptr(bg), L.ptr(y), yst, L.ptr(stats), L.stream_ptr()), "fwd16s_stats")
            assert torch.equal(y, y16 if yst else y32)
            yc = y.double().reshape(M // R, R, Co)
            mean = yc.mean(1)
            m2 = ((yc - mean[:, None]) ** 2).sum(1)
            sd = yc.std().item()
            assert (stats[..., 0].double() - mean).abs().max().item() < 1e-5 * max(sd, 1e-3)
            assert ((stats[..., 1].double() - m2).abs() / m2.clamp_min(1e-6 * R * sd * sd)).max().item() < 1e-4


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("case", S16_CASES, ids=_id)
def test_conv_dgrad16s(L, case, dt, tile, direct):
    """tests/test_gpu_ops16s.py::test_conv_dgrad16s"""
    B, Hi, Wi, Ci, Co, k, s, p = case
    d = _desc16s(L, case)
    assert L.lib.aclgan_conv16s_ok(C.byref(d), 1) == 1
    x, w, b = _tensors16(case + (0, "none"), 1, False)
    xr = x.double().requires_grad_(True)
    y = O.conv_block(xr, _rounded(w, dt).double(), b.double(), s, p, "none")
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(5))
    y.backward(_rounded(dy, dt).double())
    code = L.DTYPE[dt]
    wg = ohwi(w).cuda()
    dy16 = nhwc(dy).cuda().to(TDT[dt])
    _, w16t = _packs(L, wg, dt)
    scr = _scratch(L.lib.aclgan_conv2d_dgrad16s_scratch_bytes(C.byref(d)))
    dx32 = torch.full((B, Hi, Wi, Ci), float("nan"), device="cuda")
    L.check(L.lib.aclgan_conv2d_dgrad16s(C.byref(d), code, L.ptr(dy16), L.ptr(w16t), L.ptr(dx32), 0, 0, L.ptr(scr), L.stream_ptr()), "conv2d_dgrad16s")
    e = rel_err(nchw(dx32), xr.grad)
    print("ops_widths %s dgrad16s tile %d direct %d %-30s %.2e" % (dt, tile, direct, _id(case), e))
    # the padded-grid partial sums are stored in the 16-bit dtype before the fold: exact to one rounding of the dtype
    assert e < 2 * ULP[dt]
    dx16 = torch.full((B, Hi, Wi, Ci), float("nan"), device="cuda").to(TDT[dt])
    L.check(L.lib.aclgan_conv2d_dgrad16s(C.byref(d), code, L.ptr(dy16), L.ptr(w16t), L.ptr(dx16), code, 0, L.ptr(scr), L.stream_ptr()), "conv2d_dgrad16s")
    assert torch.equal(dx16, dx32.to(TDT[dt]))
    base = torch.randn(B, Hi, Wi, Ci, generator=torch.Generator().manual_seed(6)).cuda().to(TDT[dt])
    acc = base.clone()
    L.check(L.lib.aclgan_conv2d_dgrad16s(C.byref(d), code, L.ptr(dy16), L.ptr(w16t), L.ptr(acc), code, 1, L.ptr(scr), L.stream_ptr()))
    assert torch.equal(acc, (base.float() + dx32).to(TDT[dt]))
    dx2 = torch.empty_like(dx32)
    L.check(L.lib.aclgan_conv2d_dgrad16s(C.byref(d), code, L.ptr(dy16), L.ptr(w16t), L.ptr(dx2), 0, 0, L.ptr(scr), L.stream_ptr()))
    assert torch.equal(dx32, dx2)


# ---------------------------------------------------------------------------------------------------------------------------------
# normalisation layers at 96 / 192 / 512 / 768 channels
# ---------------------------------------------------------------------------------------------------------------------------------
NORM_CASES = [("in", "relu", 2, 12, 20, 96, False), ("ln", "relu", 2, 8, 8, 192, False), ("adain", "none", 3, 8, 8, 512, True),
              ("ln", "relu", 1, 16, 16, 768, False)]
# The normalisation kernels fix each thread's channel quad by C being a power of two in [4, 1024] (csrc/elementwise.hip), and no admitted
# architecture asks for another width: the only normalised tensors are the generator's (gen.dim << k, gen.dim a power of two; the
# discriminators have no normalisation layer but the spectral norm of their weights).  96, 192 and 768 channels are therefore REFUSED by
# the operator -- an argument error before any launch, which is what the tests below assert for them -- and 512 runs the whole method.


def _pow2(n):
    return n & (n - 1) == 0


def _norm_refused(L, kind, act, B, HW, Cn, st16=None):
    """forward and backward entry points (st16: the storage variants with that dtype code) refuse C with a message and launch nothing"""
    t = torch.zeros(B * HW * Cn, device="cuda")
    st = torch.zeros(B * Cn, device="cuda")
    scr = torch.zeros(L.lib.aclgan_norm_scratch_bytes(B, HW, Cn) // 4 + 64, device="cuda")
    n0 = L.lib.aclgan_launch_count()
    K = L.NORM[kind]
    if st16 is None:
        rf = L.lib.aclgan_norm_fwd(K, L.ACT[act], B, HW, Cn, L.ptr(t), L.ptr(st), L.ptr(st), 0, None, L.ptr(t), L.ptr(st), L.ptr(st), L.ptr(scr), L.stream_ptr())
        mf = L.last_error()
        rb = L.lib.aclgan_norm_bwd(K, L.ACT[act], B, HW, Cn, L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(st), 0, L.ptr(st), L.ptr(st), L.ptr(t), L.ptr(st), L.ptr(st), None, 0,
                                   L.ptr(scr), L.stream_ptr())
        mb = L.last_error()
    else:
        stf = (C.c_int * 3)(st16, st16, st16); stb = (C.c_int * 6)(st16, st16, st16, st16, st16, 0)
        rf = L.lib.aclgan_norm_fwd_st(K, L.ACT[act], B, HW, Cn, L.ptr(t), L.ptr(st), L.ptr(st), 0, None, L.ptr(t), L.ptr(st), L.ptr(st), L.ptr(scr), stf, L.stream_ptr())
        mf = L.last_error()
        rb = L.lib.aclgan_norm_bwd_st(K, L.ACT[act], B, HW, Cn, L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(st), 0, L.ptr(st), L.ptr(st), L.ptr(t), L.ptr(st), L.ptr(st), None, 0,
                                      L.ptr(scr), stb, L.stream_ptr())
        mb = L.last_error()
    assert rf == -1 and rb == -1 and "C=%d must be a power of two" % Cn in mf and "C=%d must be a power of two" % Cn in mb, (rf, mf, rb, mb)
    assert L.lib.aclgan_launch_count() == n0
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0 and float(st.abs().max()) == 0.0


def _norm_ref(kind, act, x, w, b, res):
    y = O.instance_norm(x) if kind == "in" else (O.adain(x, w, b) if kind == "adain" else O.layer_norm_munit(x, w, b))
    y = O._act(y, act)
    return y + res if res is not None else y


@pytest.mark.parametrize("case", NORM_CASES, ids=_id)
def test_norm_fwd_bwd(L, case):
    """tests/test_gpu_ops.py::test_norm_fwd_bwd: method and bounds (forward and the residual gradient TOL, the other gradients 5 TOL), the
    reference in fp64"""
    kind, act, B, H, W, Cn, use_res = case
    if not _pow2(Cn):
        return _norm_refused(L, kind, act, B, H * W, Cn)
    g = torch.Generator().manual_seed(11)
    x32 = torch.randn(B, Cn, H, W, generator=g) * 1.7 + 0.4
    res32 = torch.randn(B, Cn, H, W, generator=g) if use_res else None
    x = x32.double().requires_grad_(True)
    res = res32.double().requires_grad_(True) if use_res else None
    if kind == "adain":
        ap32 = torch.randn(B, 3 * Cn, generator=g)      # a row-strided slice, like the MLP output
        ap = ap32.double().requires_grad_(True)
        w, b = ap[:, Cn:2 * Cn], ap[:, :Cn]
        wstride = 3 * Cn
    elif kind == "ln":
        w32 = torch.rand(Cn, generator=g); b32 = torch.randn(Cn, generator=g) * 0.1
        w = w32.double().requires_grad_(True); b = b32.double().requires_grad_(True)
        wstride = 0
    else:
        w = b = None
        wstride = 0
    y = _norm_ref(kind, act, x, w, b, res)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy.double())
    HW = H * W
    xg = nhwc(x32).cuda()
    resg = nhwc(res32).cuda() if use_res else None
    yg = torch.empty_like(xg)
    nstat = B if kind == "ln" else B * Cn
    mean = torch.empty(nstat, device="cuda"); rstd = torch.empty(nstat, device="cuda")
    scratch = torch.empty(L.lib.aclgan_norm_scratch_bytes(B, HW, Cn) // 4 + 16, device="cuda")
    if kind == "adain":
        apg = ap32.cuda()
        wptr, bptr = C.c_void_p(apg.data_ptr() + 4 * Cn), C.c_void_p(apg.data_ptr())
    elif kind == "ln":
        wg, bg = w32.cuda(), b32.cuda()
        wptr, bptr = L.ptr(wg), L.ptr(bg)
    else:
        wptr = bptr = None
    L.check(L.lib.aclgan_norm_fwd(L.NORM[kind], L.ACT[act], B, HW, Cn, L.ptr(xg), wptr, bptr, wstride, L.ptr(resg), L.ptr(yg),
                                  L.ptr(mean), L.ptr(rstd), L.ptr(scratch), L.stream_ptr()), "norm_fwd")
    e = {"fwd": (rel_err(nchw(yg), y.detach()), TOL)}
    dyg = nhwc(dy).cuda()
    dxg = torch.empty_like(xg)
    dresg = torch.full_like(xg, float("nan")) if use_res else None
    if kind == "adain":
        dap = torch.zeros(B, 3 * Cn, device="cuda")
        dwptr, dbptr = C.c_void_p(dap.data_ptr() + 4 * Cn), C.c_void_p(dap.data_ptr())
    elif kind == "ln":
        dwg = torch.zeros(Cn, device="cuda"); dbg = torch.zeros(Cn, device="cuda")
        dwptr, dbptr = L.ptr(dwg), L.ptr(dbg)
    else:
        dwptr = dbptr = None
    L.check(L.lib.aclgan_norm_bwd(L.NORM[kind], L.ACT[act], B, HW, Cn, L.ptr(xg), L.ptr(yg), L.ptr(dyg), wptr, wstride, L.ptr(mean),
                                  L.ptr(rstd), L.ptr(dxg), dwptr, dbptr, L.ptr(dresg), 0, L.ptr(scratch), L.stream_ptr()), "norm_bwd")
    e["dx"] = (rel_err(nchw(dxg), x.grad), 5 * TOL)
    if use_res:
        e["dres"] = (rel_err(nchw(dresg), res.grad), TOL)
    if kind == "adain":
        e["dparams"] = (rel_err(dap[:, :2 * Cn], ap.grad[:, :2 * Cn]), 5 * TOL)
        assert float(dap[:, 2 * Cn:].abs().max()) == 0.0
    if kind == "ln":
        e["dgamma"] = (rel_err(dwg, w.grad), 5 * TOL)
        e["dbeta"] = (rel_err(dbg, b.grad), 5 * TOL)
    print("ops_widths norm %-28s" % _id(case), {k_: "%.2e" % v[0] for k_, v in e.items()})
    bad = {k_: v for k_, v in e.items() if not v[0] < v[1]}
    assert not bad, bad


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("case", NORM_CASES, ids=_id)
def test_norm_on_16bit_storage(L, case, dt):
    """tests/test_gpu_ops16s.py::test_norm_on_16bit_storage: x, y, residual, dy, dx, dres stored in the 16-bit dtype == the fp32-storage kernels
    on the same (rounded) values, outputs rounded once; statistics and parameter gradients are fp32 in both"""
    kind, act, B, H, W, Cn, res = case
    HW = H * W
    code = L.DTYPE[dt]
    if not _pow2(Cn):
        return _norm_refused(L, kind, act, B, HW, Cn, code)
    g = torch.Generator().manual_seed(3)
    x = _rounded(torch.randn(B, HW, Cn, generator=g) * 2 + 0.5, dt).cuda()
    r = _rounded(torch.randn(B, HW, Cn, generator=g), dt).cuda() if res else None
    dy = _rounded(torch.randn(B, HW, Cn, generator=g), dt).cuda()
    K = L.NORM[kind]
    if kind == "adain":
        w = torch.randn(B, Cn, generator=g).cuda(); b = torch.randn(B, Cn, generator=g).cuda(); ws = Cn
    elif kind == "ln":
        w = torch.rand(Cn, generator=g).cuda(); b = torch.randn(Cn, generator=g).cuda(); ws = 0
    else:
        w = b = None; ws = 0
    nst = Cn * B if kind != "ln" else B
    scr = torch.empty(L.lib.aclgan_norm_scratch_bytes(B, HW, Cn) // 4 + 64, device="cuda")

    def run(st16):
        T_ = TDT[dt] if st16 else torch.float32
        s = code if st16 else 0
        xs, rs, dys = x.to(T_), (r.to(T_) if res else None), dy.to(T_)
        y = torch.empty(B, HW, Cn, device="cuda", dtype=T_)
        mean = torch.empty(nst, device="cuda"); rstd = torch.empty(nst, device="cuda")
        stf = (C.c_int * 3)(s, s, s)
        L.check(L.lib.aclgan_norm_fwd_st(K, L.ACT[act], B, HW, Cn, L.ptr(xs), L.ptr(w), L.ptr(b), ws, L.ptr(rs), L.ptr(y), L.ptr(mean), L.ptr(rstd),
                                         L.ptr(scr), stf, L.stream_ptr()), "norm_fwd_st")
        dx = torch.empty(B, HW, Cn, device="cuda", dtype=T_)
        dres = torch.empty(B, HW, Cn, device="cuda", dtype=T_) if res else None
        dw = torch.zeros_like(w) if w is not None else None
        dbb = torch.zeros_like(b) if b is not None else None
        stb = (C.c_int * 6)(s, s, s, s, s, 0)
        L.check(L.lib.aclgan_norm_bwd_st(K, L.ACT[act], B, HW, Cn, L.ptr(xs), L.ptr(y), L.ptr(dys), L.ptr(w), ws, L.ptr(mean), L.ptr(rstd), L.ptr(dx),
                                         L.ptr(dw), L.ptr(dbb), L.ptr(dres), 0, L.ptr(scr), stb, L.stream_ptr()), "norm_bwd_st")
        return y, mean, rstd, dx, dres, dw, dbb
    y32, m32, r32, dx32, dr32, dw32, db32 = run(False)
    y16, m16, r16, dx16, dr16, dw16, db16 = run(True)
    assert torch.equal(m16, m32) and torch.equal(r16, r32)
    assert torch.equal(y16, y32.to(TDT[dt]))
    e = rel_err(dx16.float(), dx32)
    print("ops_widths %s norm storage %-28s dx %.2e" % (dt, _id(case), e))
    assert e < 2 * ULP[dt]
    if res:
        assert torch.equal(dr16, dr32.to(TDT[dt]))
    if dw32 is not None:
        assert rel_err(dw16, dw32) < 1e-5 and rel_err(db16, db32) < 1e-5
