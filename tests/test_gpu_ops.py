"""Operator-level parity of the HIP kernels (through the C ABI) against the CPU oracle.
Run on the GPU box:  python -m pytest tests -m gpu"""
import ctypes as C

import pytest
import torch

from oracle import aclgan_oracle as O

pytestmark = pytest.mark.gpu

# fp32 on both sides (the MFMA path is an exact-fp32 fma chain): differences are summation order.
TOL = 2e-4


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib
    return _lib


# (B, Hi, Wi, Ci, Co, k, s, p, up, act)
CONV_CASES = [
    (2, 16, 20, 3, 64, 7, 1, 3, 0, "relu"),      # CE0 / SE0: Cin 3 (scalar gather path)
    (2, 16, 16, 64, 128, 4, 2, 1, 0, "none"),    # CE1
    (1, 16, 16, 128, 256, 4, 2, 1, 0, "relu"),   # CE2 / SE2
    (2, 8, 8, 256, 256, 3, 1, 1, 0, "none"),     # ResBlock conv (Winograd F(4x4,3x3) path: forward, dgrad interior, wgrad)
    (1, 12, 20, 64, 128, 3, 1, 1, 0, "relu"),    # Winograd: non-square map, Cin != Cout, activation in the output transform
    (3, 4, 8, 128, 64, 3, 1, 1, 0, "none"),      # Winograd: a single tile row, B = 3
    (2, 16, 16, 64, 64, 3, 1, 1, 0, "lrelu"),    # Winograd: smallest channel counts that take the path
    (2, 10, 12, 64, 64, 3, 1, 1, 0, "none"),     # 3x3 but H % 4 != 0: stays on the direct kernels
    (2, 8, 8, 256, 128, 5, 1, 2, 1, "none"),     # DU0: upsample folded into the gather
    (1, 16, 16, 128, 64, 5, 1, 2, 1, "none"),    # DU1
    (2, 9, 13, 32, 48, 5, 1, 2, 1, "relu"),      # upsample+5x5 on a ragged map (sub-pixel path: 4 phases + exact ring)
    (1, 4, 4, 16, 16, 5, 1, 2, 1, "none"),       # smallest map the sub-pixel path accepts (interior 2x2)
    (2, 16, 16, 64, 4, 7, 1, 3, 0, "tanh"),      # DO: Cout 4 (direct VALU kernels)
    (1, 40, 72, 64, 4, 7, 1, 3, 0, "tanh"),      # DO on a map that is not a multiple of the 8x32 tile
    (2, 12, 20, 32, 4, 7, 1, 3, 0, "none"),      # Cout 4 with Cin 32: direct forward, MFMA wgrad
    (2, 32, 32, 6, 64, 4, 2, 1, 0, "lrelu"),     # D first layer, 6-channel pair
    (2, 32, 32, 3, 64, 4, 2, 1, 0, "lrelu"),     # D first layer, 3 channels
    (2, 8, 8, 256, 512, 4, 2, 1, 0, "lrelu"),    # D last strided conv
    (2, 4, 4, 512, 1, 1, 1, 0, 0, "none"),       # D head 1x1, Cout 1
    (2, 8, 8, 8, 16, 3, 1, 1, 0, "relu"),        # reduced-width config
    (3, 12, 20, 16, 8, 4, 2, 1, 0, "lrelu"),     # ragged sizes
    (1, 2, 2, 16, 16, 4, 2, 1, 0, "lrelu"),      # smallest map the 3rd D scale reaches (64x64 input)
    (5, 9, 7, 12, 20, 3, 1, 1, 0, "none"),       # nothing a multiple of anything
    (3, 12, 20, 3, 64, 4, 2, 1, 0, "lrelu"),     # round 6: D first layer on a ragged map (thin-input kernels: 6 x 10 outputs, 7 x 11 class grid)
    (2, 66, 40, 6, 64, 4, 2, 1, 0, "lrelu"),     # ... 6-channel pair input, more than one tile in both directions, two tiles per workgroup
    (1, 128, 96, 3, 64, 4, 2, 1, 0, "none"),     # ... several tiles per workgroup (64 x 48 outputs)
    (2, 16, 16, 3, 16, 4, 2, 1, 0, "lrelu"),     # ... reduced width (Cout 16: forward on the general kernel, input gradient on the thin one)
    (2, 40, 72, 3, 64, 7, 1, 3, 0, "relu"),      # CE0 on a map of 5 x 3 tiles (pipelined tiles: 4 / 2 / 1 per workgroup by grid size)
]


def _case_tensors(case, seed=0):
    B, Hi, Wi, Ci, Co, k, s, p, up, act = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Ci, Hi, Wi, generator=g)
    w = torch.randn(Co, Ci, k, k, generator=g) * (2.0 / (Ci * k * k)) ** 0.5
    b = torch.randn(Co, generator=g) * 0.1
    return x, w, b


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_fwd(L, case):
    from gpu_util import conv_desc, gpu_conv_fwd, nhwc, nchw, ohwi, rel_err
    B, Hi, Wi, Ci, Co, k, s, p, up, act = case
    x, w, b = _case_tensors(case)
    ref = O.conv_block(x, w, b, s, p, act, upsample=bool(up))
    d = conv_desc(L, B, Hi, Wi, Ci, Co, k, s, p, up, act)
    y = gpu_conv_fwd(L, d, nhwc(x).cuda(), ohwi(w).cuda(), b.cuda())
    assert rel_err(nchw(y), ref) < TOL
    yn = gpu_conv_fwd(L, d, nhwc(x).cuda(), ohwi(w).cuda(), b.cuda(), naive=True)
    assert rel_err(nchw(yn), ref) < TOL
    if L.lib.aclgan_conv2d_fwd_scratch_bytes(C.byref(d)) and not L.lib.aclgan_get_deterministic():
        # the scratch-less variant of the same layer (exact gather instead of the sub-pixel path, fp32 atomics instead of
        # ordered split-K partials) must agree as well ...
        ye = gpu_conv_fwd(L, d, nhwc(x).cuda(), ohwi(w).cuda(), b.cuda(), ws=False)
        assert rel_err(nchw(ye), ref) < TOL
        # ... and WITH scratch the forward is reproducible bit for bit
        y2 = gpu_conv_fwd(L, d, nhwc(x).cuda(), ohwi(w).cuda(), b.cuda())
        assert torch.equal(y, y2)


WINO_X3_CASES = [CONV_CASES[3], CONV_CASES[4], CONV_CASES[5], CONV_CASES[6], CONV_CASES[8], CONV_CASES[9],
                 (2, 32, 32, 128, 128, 3, 1, 1, 0, "relu"), (1, 20, 24, 64, 192, 3, 1, 1, 0, "none")]


@pytest.mark.parametrize("case", WINO_X3_CASES)
def test_winograd_with_split_bf16_gemm_slices(L, case):
    """The option aclgan_set_tuning("wino_x3", 1) (csrc/gemm_bf16x3.hip: the GEMM slices of the fp32 Winograd pipeline as six bf16 x bf16
    products per multiply, operands split exactly into three bf16 planes by the transforms) is fp32 arithmetic: forward and input
    gradient agree with the oracle to the same tolerance as the fp32 MFMA slices, and with the fp32-slices result itself to fp32 rounding."""
    from gpu_util import conv_desc, gpu_conv_fwd, gpu_conv_dgrad, nhwc, nchw, ohwi, rel_err
    B, Hi, Wi, Ci, Co, k, s, p, up, act = case
    x, w, b = _case_tensors(case, 3)
    x.requires_grad_(True)
    ref = O.conv_block(x, w, b, s, p, act, upsample=bool(up))
    y_lin = O.conv_block(x, w, b, s, p, "none", upsample=bool(up))
    dy = torch.randn(y_lin.shape, generator=torch.Generator().manual_seed(5))
    y_lin.backward(dy)
    d = conv_desc(L, B, Hi, Wi, Ci, Co, k, s, p, up, act)
    dn = conv_desc(L, B, Hi, Wi, Ci, Co, k, s, p, up, "none")
    xg, wg, bg, dyg = nhwc(x.detach()).cuda(), ohwi(w).cuda(), b.cuda(), nhwc(dy).cuda()
    out = {}
    old = L.lib.aclgan_set_tuning(b"wino_x3", 0)
    try:
        for v in (0, 1):
            L.lib.aclgan_set_tuning(b"wino_x3", v)
            out[v] = (gpu_conv_fwd(L, d, xg, wg, bg), gpu_conv_dgrad(L, dn, dyg, wg))
    finally:
        L.lib.aclgan_set_tuning(b"wino_x3", old)
    for v in (0, 1):
        assert rel_err(nchw(out[v][0]), ref) < TOL
        assert rel_err(nchw(out[v][1]), x.grad) < TOL
    # the two GEMM implementations differ by fp32 rounding only (the transforms amplify it by the same ~1.5 digits either way)
    assert rel_err(out[1][0], out[0][0]) < 2e-5 and rel_err(out[1][1], out[0][1]) < 2e-5
    # and with both against the fp64 truth the split-bf16 result is no worse than 1.5x the fp32 MFMA one
    e0, e1 = rel_err(nchw(out[0][0]), ref.double()), rel_err(nchw(out[1][0]), ref.double())
    assert e1 <= 1.5 * e0 + 1e-6, (e0, e1)


@pytest.mark.parametrize("case", WINO_X3_CASES + [(2, 64, 64, 128, 128, 3, 1, 1, 0, "none"), (1, 16, 16, 128, 64, 5, 1, 2, 1, "none")])
def test_winograd_fused_kernel(L, case):
    """csrc/conv_wino_fused.hip (round 4): Winograd F(4x4,3x3) with the input transform, the 36 frequency GEMMs and the output transform in
    ONE launch -- the ResBlock convolutions and the four sub-pixel phases of the upsample + 5x5 layers, forward and input gradient.  The step
    takes it where its cost model says it pays (large grids); here it is FORCED (tuning mode 2) on every eligible shape, small and ragged
    ones included, and must agree with the oracle like the three-launch pipeline (mode 0) does, accumulate mode included."""
    from gpu_util import conv_desc, gpu_conv_fwd, gpu_conv_dgrad, nhwc, nchw, ohwi, rel_err
    B, Hi, Wi, Ci, Co, k, s, p, up, act = case
    x, w, b = _case_tensors(case, 7)
    x.requires_grad_(True)
    ref = O.conv_block(x, w, b, s, p, act, upsample=bool(up))
    y_lin = O.conv_block(x, w, b, s, p, "none", upsample=bool(up))
    dy = torch.randn(y_lin.shape, generator=torch.Generator().manual_seed(5))
    y_lin.backward(dy)
    d = conv_desc(L, B, Hi, Wi, Ci, Co, k, s, p, up, act)
    dn = conv_desc(L, B, Hi, Wi, Ci, Co, k, s, p, up, "none")
    xg, wg, bg, dyg = nhwc(x.detach()).cuda(), ohwi(w).cuda(), b.cuda(), nhwc(dy).cuda()
    base = torch.randn(B, Hi, Wi, Ci, generator=torch.Generator().manual_seed(6))
    out = {}
    old = L.lib.aclgan_set_tuning(b"wino_fused", 0)
    try:
        for v in (0, 2):
            L.lib.aclgan_set_tuning(b"wino_fused", v)
            n0 = L.lib.aclgan_launch_count()
            y = gpu_conv_fwd(L, d, xg, wg, bg)
            launches = L.lib.aclgan_launch_count() - n0
            out[v] = (y, gpu_conv_dgrad(L, dn, dyg, wg), gpu_conv_dgrad(L, dn, dyg, wg, accumulate_into=base.clone().cuda()), launches)
    finally:
        L.lib.aclgan_set_tuning(b"wino_fused", old)
    for v in (0, 2):
        assert rel_err(nchw(out[v][0]), ref) < TOL
        assert rel_err(nchw(out[v][1]), x.grad) < TOL
        assert rel_err(nchw(out[v][2]).cpu() - nchw(base), x.grad) < 5 * TOL
    if Co % 64 == 0 and Ci % 16 == 0:
        assert out[2][3] < out[0][3], "the forced mode did not take the fused kernel (launch counts %d vs %d)" % (out[2][3], out[0][3])
    # same arithmetic, different summation order
    assert rel_err(out[2][0], out[0][0]) < 5e-5 and rel_err(out[2][1], out[0][1]) < 5e-5
    if k == 3 and up == 0 and Hi % 4 == 0 and Wi % 4 == 0 and Ci % 16 == 0 and Co % 64 == 0:
        # the entry point itself (include/aclgan_hip.h: "reflect != 0: reflection padding") with any non-zero flag -- the launcher's
        # internal edge mode (2) and a negative value included -- pads by reflection
        Uf = torch.empty(36 * Co * Ci, device="cuda")
        L.check(L.lib.aclgan_winograd_filter_frag(L.ptr(wg), L.ptr(Uf), Co, Ci, 0, L.stream_ptr()), "winograd_filter_frag")
        for flag in (1, 2, -1):
            y = torch.full((B, Hi, Wi, Co), float("nan"), device="cuda")
            L.check(L.lib.aclgan_conv3x3_winograd_fused(L.ptr(xg), L.ptr(Uf), L.ptr(bg), L.ptr(y), B, Hi, Wi, Ci, Co, L.ACT[act], flag, 0, None,
                                                        L.stream_ptr()), "conv3x3_winograd_fused")
            assert rel_err(nchw(y), ref) < TOL, (flag, rel_err(nchw(y), ref))


S2K4_CASES = [
    (2, 16, 16, 64, 128, 4, 2, 1, 0, "none"),     # CE1 / SE1 / D layer 1 shape (reduced map)
    (1, 16, 16, 128, 256, 4, 2, 1, 0, "relu"),    # CE2 / SE2, activation in the epilogue
    (2, 8, 8, 256, 512, 4, 2, 1, 0, "lrelu"),     # D layer 3: one (half-empty) tile block per image
    (3, 12, 20, 64, 64, 4, 2, 1, 0, "lrelu"),     # 6 x 10 outputs: ragged last tiles in both directions, B = 3
    (1, 34, 18, 32, 64, 4, 2, 1, 0, "none"),      # 17 x 9 outputs (odd), Cin 32
    (2, 64, 64, 64, 128, 4, 2, 1, 0, "none"),     # several tile blocks per image (2 x 1 blocks of 8 x 4 tiles)
    (1, 72, 40, 128, 64, 4, 2, 1, 0, "none"),     # 36 x 20 outputs: 2 x 3 tile blocks, the last ones partly empty; Cin > Cout
]


@pytest.mark.parametrize("case", S2K4_CASES)
def test_stride2_layers_through_the_fused_winograd_kernel(L, case):
    """Round 6 (csrc/conv_wino_fused.hip, wino_fused_s2k4_*): ReflectionPad2d(1) + Conv2d(4x4, stride 2) (networks.py:41, 216-221, 236-241) as the
    four input-parity phases of the fused F(4x4,3x3) kernel -- forward (K loop over phase x Cin, edge replication in the parity views) and the
    interior of the input gradient (four grid phases writing the parity views of dx; the mirrored halo keeps its direct launch).  FORCED
    (tuning mode 2) on small and ragged maps, against the oracle and against the direct kernels (mode 0), accumulate mode included."""
    from gpu_util import conv_desc, gpu_conv_fwd, gpu_conv_dgrad, nhwc, nchw, ohwi, rel_err
    B, Hi, Wi, Ci, Co, k, s, p, up, act = case
    x, w, b = _case_tensors(case, 11)
    x.requires_grad_(True)
    ref = O.conv_block(x, w, b, s, p, act, upsample=False)
    y_lin = O.conv_block(x, w, b, s, p, "none", upsample=False)
    dy = torch.randn(y_lin.shape, generator=torch.Generator().manual_seed(5))
    y_lin.backward(dy)
    d = conv_desc(L, B, Hi, Wi, Ci, Co, k, s, p, up, act)
    dn = conv_desc(L, B, Hi, Wi, Ci, Co, k, s, p, up, "none")
    xg, wg, bg, dyg = nhwc(x.detach()).cuda(), ohwi(w).cuda(), b.cuda(), nhwc(dy).cuda()
    base = torch.randn(B, Hi, Wi, Ci, generator=torch.Generator().manual_seed(6))
    out = {}
    old = L.lib.aclgan_set_tuning(b"wino_fused", 0)
    try:
        for v in (0, 2):
            L.lib.aclgan_set_tuning(b"wino_fused", v)
            y = gpu_conv_fwd(L, d, xg, wg, bg)
            out[v] = (y, gpu_conv_dgrad(L, dn, dyg, wg), gpu_conv_dgrad(L, dn, dyg, wg, accumulate_into=base.clone().cuda()), gpu_conv_fwd(L, d, xg, wg, bg))
    finally:
        L.lib.aclgan_set_tuning(b"wino_fused", old)
    for v in (0, 2):
        assert rel_err(nchw(out[v][0]), ref) < TOL
        assert rel_err(nchw(out[v][1]), x.grad) < TOL
        assert rel_err(nchw(out[v][2]).cpu() - nchw(base), x.grad) < 5 * TOL
        assert torch.equal(out[v][0], out[v][3])          # the forward is reproducible bit for bit on either path
    # different arithmetic (so the forced mode did take the other kernel), same result to the transforms' rounding
    # (the input gradient's output channels are the layer's INPUT channels: Cin 32 stays on the direct kernel)
    assert not torch.equal(out[2][0], out[0][0]) and (L.lib.aclgan_get_deterministic() or Ci % 64 != 0 or not torch.equal(out[2][1], out[0][1]))
    assert rel_err(out[2][0], out[0][0]) < 5e-5 and rel_err(out[2][1], out[0][1]) < 5e-5


WGRAD_FUSED_CASES = [(1, 16, 16, 64, 64), (2, 16, 32, 64, 64), (1, 8, 32, 64, 128), (3, 20, 48, 64, 64), (7, 12, 16, 128, 64), (2, 64, 64, 256, 256), (5, 32, 32, 128, 128)]


@pytest.mark.parametrize("case", WGRAD_FUSED_CASES)
def test_winograd_wgrad_fused_kernel(L, case):
    """csrc/conv_wino_wgrad_fused.hip (round 4): the weight / bias gradient of the 3x3 ResBlock convolutions with both Winograd transforms done in
    registers on the way into the MFMAs (one kernel + one ordered finish launch instead of seven launches and 150 MB of planes).  Against the
    oracle's autograd (networks.py:297-310 Conv2dBlock, zero-initialised and NON-zero gradient buffers: the kernels accumulate), against the
    pipeline of conv_wino.hip, run to run bit-identical (ordered K slices); shapes with one strip per row (both image borders in one strip),
    a single group per K slice (the small shapes), K slices of unequal length (5 x 8 x 2 = 80 groups in 27 slices of 3, 3, .., 2), the step's shape."""
    from gpu_util import conv_desc, nhwc, ohwi, rel_err
    import ctypes as C
    B, H, W, Ci, Co = case
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, Ci, H, W, generator=g); dy = torch.randn(B, Co, H, W, generator=g)
    w = torch.zeros(Co, Ci, 3, 3, requires_grad=True); b = torch.zeros(Co, requires_grad=True)
    O.conv_block(x, w, b, 1, 1, "none").backward(dy)
    dw0 = torch.randn(Co, 3, 3, Ci, generator=g) * 0.1; db0 = torch.randn(Co, generator=g)
    d = conv_desc(L, B, H, W, Ci, Co, 3, 1, 1, 0, "none")
    xg, dyg = nhwc(x).cuda(), nhwc(dy).cuda()
    scratch = torch.empty(L.lib.aclgan_conv2d_wgrad_scratch_bytes(C.byref(d)) // 4 + 16, device="cuda")
    out = {}
    old = L.lib.aclgan_set_tuning(b"wino_wgrad_fused", 0)
    try:
        for v in (0, 2, 3):      # 3 = the fused kernel a second time
            L.lib.aclgan_set_tuning(b"wino_wgrad_fused", min(v, 2))
            dw, db = dw0.clone().cuda(), db0.clone().cuda()
            n0 = L.lib.aclgan_launch_count()
            L.check(L.lib.aclgan_conv2d_wgrad_ws(C.byref(d), L.ptr(xg), L.ptr(dyg), L.ptr(dw), L.ptr(db), L.ptr(scratch), L.stream_ptr()), "conv2d_wgrad_ws")
            out[v] = (dw.cpu() - dw0, db.cpu() - db0, L.lib.aclgan_launch_count() - n0, dw.cpu(), db.cpu())
    finally:
        L.lib.aclgan_set_tuning(b"wino_wgrad_fused", old)
    for v in (0, 2):
        assert rel_err(out[v][0], ohwi(w.grad)) < 5 * TOL and rel_err(out[v][1], b.grad) < 5 * TOL, (v, rel_err(out[v][0], ohwi(w.grad)), rel_err(out[v][1], b.grad))
    assert out[2][2] == 2, "the forced mode did not take the fused kernel (%d launches)" % out[2][2]
    assert torch.equal(out[2][3], out[3][3]) and torch.equal(out[2][4], out[3][4]), "the fused weight gradient is not reproducible run to run"
    if Ci % 64 == 0:      # (below that the mode-0 path is the direct kernel, not the Winograd pipeline)
        assert rel_err(out[2][0], out[0][0]) < 5e-5


STRESS_FWD_CASES = [(3, 20, 28, 64, 64, 3, 1, 1, 0, "relu"),      # ragged tile rows / columns, reflect padding
                    (2, 64, 64, 256, 256, 3, 1, 1, 0, "none"),    # the step's ResBlock shape (one workgroup per 8 x 4 tile block)
                    (1, 16, 16, 128, 64, 5, 1, 2, 1, "none")]     # sub-pixel phases: four grid phases forward, four K phases in the input gradient


@pytest.mark.parametrize("case", STRESS_FWD_CASES)
def test_winograd_fused_kernels_repeat_launch_stress(L, case):
    """Advisor (round 4): the two fused Winograd kernels carry hand-written MFMAs (`v_mfma` in VGPR form with "+v" operands) and, in the weight
    gradient, inline-asm LDS reads with manual s_waitcnt -- hazards the compiler cannot see, held by the placement of sched_barriers.  The
    round-4 race of exactly this kind (barriers publishing LDS-DMA copies) showed in 1 launch of 3 000.  So: thousands of back-to-back launches
    of the forced fused forward, the fused input gradient (accumulate mode off) and the fused weight gradient, each compared BITWISE with the
    first launch, with a busy second stream next to them (the side stream / lanes of the step change what shares a CU)."""
    from gpu_util import conv_desc, nhwc, ohwi
    import ctypes as C
    B, Hi, Wi, Ci, Co, k, s, p, up, act = case
    x, w, b = _case_tensors(case, 9)
    d = conv_desc(L, B, Hi, Wi, Ci, Co, k, s, p, up, act)
    dn = conv_desc(L, B, Hi, Wi, Ci, Co, k, s, p, up, "none")
    xg, wg, bg = nhwc(x).cuda(), ohwi(w).cuda(), b.cuda()
    Ho, Wo = (Hi << up), (Wi << up)
    dyg = torch.randn(B, Ho, Wo, Co, generator=torch.Generator().manual_seed(4)).cuda()
    fwd_scr = torch.empty(L.lib.aclgan_conv2d_fwd_scratch_bytes(C.byref(d)) // 4 + 16, device="cuda")
    dg_scr = torch.empty(L.lib.aclgan_conv2d_dgrad_scratch_bytes(C.byref(dn)) // 4 + 16, device="cuda")
    wg_scr = torch.empty(L.lib.aclgan_conv2d_wgrad_scratch_bytes(C.byref(dn)) // 4 + 16, device="cuda")
    N = 800
    busy = torch.cuda.Stream()
    noise = torch.randn(1 << 24, device="cuda")
    old_f = L.lib.aclgan_set_tuning(b"wino_fused", 2); old_w = L.lib.aclgan_set_tuning(b"wino_wgrad_fused", 2)
    try:
        st = L.stream_ptr()
        first = None
        bad = {"fwd": 0, "dgrad": 0, "wgrad": 0}
        for i in range(N):
            if i % 50 == 0:
                with torch.cuda.stream(busy):
                    noise.mul_(1.0001)          # a streaming kernel on another queue
            y = torch.empty(B, Ho, Wo, Co, device="cuda")
            L.check(L.lib.aclgan_conv2d_fwd_ws(C.byref(d), L.ptr(xg), L.ptr(wg), L.ptr(bg), L.ptr(y), L.ptr(fwd_scr), st), "fwd")
            dx = torch.empty(B, Hi, Wi, Ci, device="cuda")
            L.check(L.lib.aclgan_conv2d_dgrad(C.byref(dn), L.ptr(dyg), L.ptr(wg), L.ptr(dx), L.ptr(dg_scr), 0, st), "dgrad")
            cur = [y, dx]
            if up == 0:
                dw = torch.zeros(Co, k, k, Ci, device="cuda"); db = torch.zeros(Co, device="cuda")
                L.check(L.lib.aclgan_conv2d_wgrad_ws(C.byref(dn), L.ptr(xg), L.ptr(dyg), L.ptr(dw), L.ptr(db), L.ptr(wg_scr), st), "wgrad")
                cur += [dw, db]
            if first is None:
                first = cur
                continue
            bad["fwd"] += int(not torch.equal(cur[0], first[0]))
            # (the border of dx also receives the reflection halo / the sub-pixel ring through fp32 atomics in the default mode: the fused kernel's
            #  own output is the interior)
            bad["dgrad"] += int(not torch.equal(cur[1][:, 3:-3, 3:-3], first[1][:, 3:-3, 3:-3]))
            if up == 0:
                bad["wgrad"] += int(not (torch.equal(cur[2], first[2]) and torch.equal(cur[3], first[3])))
        torch.cuda.synchronize()
        assert bad == {"fwd": 0, "dgrad": 0, "wgrad": 0}, (case, bad, N)
    finally:
        L.lib.aclgan_set_tuning(b"wino_fused", old_f); L.lib.aclgan_set_tuning(b"wino_wgrad_fused", old_w)


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_dgrad(L, case):
    from gpu_util import conv_desc, gpu_conv_dgrad, nhwc, nchw, ohwi, rel_err
    B, Hi, Wi, Ci, Co, k, s, p, up, act = case
    x, w, b = _case_tensors(case, 1)
    x.requires_grad_(True)
    y = O.conv_block(x, w, b, s, p, "none", upsample=bool(up))
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(5))
    y.backward(dy)
    d = conv_desc(L, B, Hi, Wi, Ci, Co, k, s, p, up, "none")
    dx = gpu_conv_dgrad(L, d, nhwc(dy).cuda(), ohwi(w).cuda())
    assert rel_err(nchw(dx), x.grad) < TOL
    # accumulate mode: dx += on top of an existing gradient
    base = torch.randn(B, Hi, Wi, Ci, generator=torch.Generator().manual_seed(6))
    acc = gpu_conv_dgrad(L, d, nhwc(dy).cuda(), ohwi(w).cuda(), accumulate_into=base.clone().cuda())
    assert rel_err(nchw(acc).cpu() - nchw(base), x.grad) < 5 * TOL



@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_wgrad(L, case):
    from gpu_util import conv_desc, gpu_conv_wgrad, nhwc, ohwi, rel_err
    B, Hi, Wi, Ci, Co, k, s, p, up, act = case
    x, w, b = _case_tensors(case, 2)
    w.requires_grad_(True); b.requires_grad_(True)
    y = O.conv_block(x, w, b, s, p, "none", upsample=bool(up))
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(7))
    y.backward(dy)
    d = conv_desc(L, B, Hi, Wi, Ci, Co, k, s, p, up, "none")
    dw, db = gpu_conv_wgrad(L, d, nhwc(x).cuda(), nhwc(dy).cuda())
    assert rel_err(dw, ohwi(w.grad)) < TOL
    assert rel_err(db, b.grad) < TOL
    if Co % 64 == 0 and Ci % 64 == 0:
        # heavy layers: k-contiguous tiles + ordered slices (csrc/conv_fast.hip: conv_wgrad_kc_kernel) -- no atomics, so the
        # weight and bias gradients are reproducible bit for bit
        dw3, db3 = gpu_conv_wgrad(L, d, nhwc(x).cuda(), nhwc(dy).cuda())
        assert torch.equal(dw, dw3) and torch.equal(db, db3)
    if L.lib.aclgan_conv2d_wgrad_scratch_bytes(C.byref(d)) and not L.lib.aclgan_get_deterministic():   # the scratch-less variant of the same layer (exact gather / atomics) must agree
        dw2, db2 = gpu_conv_wgrad(L, d, nhwc(x).cuda(), nhwc(dy).cuda(), ws=False)
        assert rel_err(dw2, ohwi(w.grad)) < TOL and rel_err(db2, b.grad) < TOL


# thin-channel 7x7 layers (csrc/conv_small.hip): sizes around the kernels' internal boundaries -- 8x32 output tiles,
# 70-position column segments, 8- / 16-row bands of the weight-gradient kernel, the smallest legal map (7x7)
THIN_CASES = [(B, H, W, Ci, Co) for (Ci, Co) in ((3, 64), (64, 4), (4, 64), (64, 3))
              for (B, H, W) in ((1, 7, 7), (2, 9, 71), (1, 17, 70), (1, 33, 141), (3, 16, 69))]


@pytest.mark.parametrize("case", THIN_CASES)
def test_thin_7x7_layers_ragged(L, case):
    from gpu_util import conv_desc, gpu_conv_fwd, gpu_conv_dgrad, gpu_conv_wgrad, nhwc, nchw, ohwi, rel_err
    B, H, W, Ci, Co = case
    g = torch.Generator().manual_seed(H * 1000 + W + Ci)
    x = torch.randn(B, Ci, H, W, generator=g, requires_grad=True)
    w = (torch.randn(Co, Ci, 7, 7, generator=g) * (2.0 / (Ci * 49)) ** 0.5).requires_grad_(True)
    b = (torch.randn(Co, generator=g) * 0.1).requires_grad_(True)
    y = O.conv_block(x, w, b, 1, 3, "none")
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy)
    d = conv_desc(L, B, H, W, Ci, Co, 7, 1, 3, 0, "none")
    assert rel_err(nchw(gpu_conv_fwd(L, d, nhwc(x.detach()).cuda(), ohwi(w.detach()).cuda(), b.detach().cuda())), y.detach()) < TOL
    assert rel_err(nchw(gpu_conv_dgrad(L, d, nhwc(dy).cuda(), ohwi(w.detach()).cuda())), x.grad) < TOL
    # two-stage reduction through scratch / atomics (the scratch-less call refuses to run in deterministic mode)
    for ws in ((True,) if L.lib.aclgan_get_deterministic() else (True, False)):
        dw, db = gpu_conv_wgrad(L, d, nhwc(x.detach()).cuda(), nhwc(dy).cuda(), ws=ws)
        assert rel_err(dw, ohwi(w.grad)) < TOL and rel_err(db, b.grad) < TOL


def test_conv_linearity_full_size(L):
    """size-independent property at a BASELINE-sized layer (256x64x64 ResBlock conv, B=8):
    conv(a*x1 + x2) == a*conv(x1) + conv(x2) (bias off), and MFMA == naive kernel."""
    from gpu_util import conv_desc, gpu_conv_fwd
    g = torch.Generator(device="cuda").manual_seed(3)
    x1 = torch.randn(8, 64, 64, 256, device="cuda", generator=g)
    x2 = torch.randn(8, 64, 64, 256, device="cuda", generator=g)
    w = torch.randn(256, 3, 3, 256, device="cuda", generator=g) * 0.03
    d = conv_desc(L, 8, 64, 64, 256, 256, 3, 1, 1)
    yn = gpu_conv_fwd(L, d, x1, w, None, naive=True)
    # ws=False: the direct MFMA kernel (an exact fp32 fma chain);  ws=True: what the engine runs for this layer -- Winograd
    # F(4x4,3x3) (csrc/conv_wino.hip), whose transforms cost ~1.5 digits (measured 1.3e-5 against the fp64 truth)
    for ws, tol in ((False, 1e-5), (True, 1e-4)):
        y1 = gpu_conv_fwd(L, d, x1, w, None, ws=ws)
        y2 = gpu_conv_fwd(L, d, x2, w, None, ws=ws)
        y12 = gpu_conv_fwd(L, d, 0.5 * x1 + x2, w, None, ws=ws)
        assert ((y12 - (0.5 * y1 + y2)).abs().max() / y12.abs().max()).item() < tol
        assert ((y1 - yn).abs().max() / yn.abs().max()).item() < tol


NORM_CASES = [  # (kind, act, B, H, W, C, residual)
    ("in", "relu", 2, 16, 16, 64, False), ("in", "none", 2, 8, 8, 256, True), ("in", "relu", 1, 12, 20, 8, False),
    ("adain", "relu", 2, 8, 8, 256, False), ("adain", "none", 3, 8, 8, 16, True),
    ("ln", "relu", 2, 16, 16, 128, False), ("ln", "relu", 1, 32, 32, 64, False), ("ln", "relu", 3, 6, 10, 8, False),
    ("in", "relu", 2, 64, 64, 64, False),
    ("ln", "relu", 2, 4, 6, 512, False), ("in", "none", 1, 5, 7, 4, False), ("ln", "none", 2, 64, 64, 64, False),   # C > 256 / C = 4 / many chunks
    # round 6: 512 chunks per sample -- the LayerNorm statistics in 32 slices (stage 2 inside the apply kernel), the division-free InstanceNorm
    # finalize in two rounds of 16 partials per thread
    ("ln", "relu", 1, 128, 128, 128, False), ("in", "none", 1, 128, 128, 32, True),
]


def _norm_ref(kind, act, x, w, b, res):
    if kind == "in":
        y = O.instance_norm(x)
    elif kind == "adain":
        y = O.adain(x, w, b)
    else:
        y = O.layer_norm_munit(x, w, b)
    y = O._act(y, act)
    return y + res if res is not None else y


@pytest.mark.parametrize("case", NORM_CASES)
def test_norm_fwd_bwd(L, case):
    from gpu_util import nhwc, nchw, rel_err
    kind, act, B, H, W, Cn, use_res = case
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(B, Cn, H, W, generator=g) * 1.7 + 0.4).requires_grad_(True)
    res = torch.randn(B, Cn, H, W, generator=g).requires_grad_(True) if use_res else None
    if kind == "adain":
        ap = torch.randn(B, 3 * Cn, generator=g).requires_grad_(True)   # a row-strided slice, like the MLP output
        w, b = ap[:, Cn:2 * Cn], ap[:, :Cn]
        wstride = 3 * Cn
    elif kind == "ln":
        w = torch.rand(Cn, generator=g).requires_grad_(True)
        b = (torch.randn(Cn, generator=g) * 0.1).requires_grad_(True)
        wstride = 0
    else:
        w = b = None
        wstride = 0
    y = _norm_ref(kind, act, x, w, b, res)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy)

    HW = H * W
    xg = nhwc(x.detach()).cuda()
    resg = nhwc(res.detach()).cuda() if use_res else None
    yg = torch.empty_like(xg)
    nstat = B if kind == "ln" else B * Cn
    mean = torch.empty(nstat, device="cuda"); rstd = torch.empty(nstat, device="cuda")
    scratch = torch.empty(L.lib.aclgan_norm_scratch_bytes(B, HW, Cn) // 4 + 16, device="cuda")
    if kind == "adain":
        apg = ap.detach().cuda()
        wg, bg = apg[:, Cn:], apg[:, :Cn]       # views: pointer + row stride
        wptr, bptr = C.c_void_p(apg.data_ptr() + 4 * Cn), C.c_void_p(apg.data_ptr())
    elif kind == "ln":
        wg, bg = w.detach().cuda(), b.detach().cuda()
        wptr, bptr = L.ptr(wg), L.ptr(bg)
    else:
        wptr = bptr = None
    L.check(L.lib.aclgan_norm_fwd(L.NORM[kind], L.ACT[act], B, HW, Cn, L.ptr(xg), wptr, bptr, wstride, L.ptr(resg), L.ptr(yg),
                                  L.ptr(mean), L.ptr(rstd), L.ptr(scratch), L.stream_ptr()), "norm_fwd")
    assert rel_err(nchw(yg), y) < TOL

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
    assert rel_err(nchw(dxg), x.grad) < 5 * TOL
    if use_res:
        assert rel_err(nchw(dresg), res.grad) < TOL
    if kind == "adain":
        assert rel_err(dap[:, :2 * Cn], ap.grad[:, :2 * Cn]) < 5 * TOL
        assert float(dap[:, 2 * Cn:].abs().max()) == 0.0
    if kind == "ln":
        assert rel_err(dwg, w.grad) < 5 * TOL
        assert rel_err(dbg, b.grad) < 5 * TOL


# Conv2dBlock.forward as one operator (networks.py:365-371): (B, H, W, Ci, Co, k, norm, act, residual, statistics from the conv epilogue?)
BLOCK_CASES = [
    (2, 16, 16, 256, 256, 3, "in", "relu", False, True),      # ResBlock conv 1: Winograd output transform emits the IN statistics
    (2, 8, 12, 256, 256, 3, "in", "none", True, True),        # ResBlock conv 2 (+ residual), non-square map
    (3, 8, 8, 64, 128, 3, "adain", "relu", False, True),      # decoder ResBlock (AdaIN), Cin != Cout
    (1, 64, 64, 64, 64, 3, "ln", "relu", False, True),        # LN over the tile partials (256 tiles x 64 channels)
    (2, 10, 12, 64, 64, 3, "in", "relu", False, False),       # H % 4 != 0: direct kernel, separate statistics pass
    (2, 16, 16, 64, 128, 4, "in", "relu", False, "s2"),       # strided encoder conv: statistics from the epilogue where the fused kernel runs it
    (1, 24, 40, 128, 256, 4, "in", "relu", False, "s2"),      # ... non-square, 12 x 20 outputs (whole 4x4 tiles)
    (2, 12, 20, 64, 128, 4, "in", "relu", False, False),      # ... 6 x 10 outputs: not whole tiles -> separate statistics pass
]


@pytest.fixture(params=[0, 2], ids=["three-launch", "one-launch"])
def wino_mode(L, request):
    """the Winograd layers through the three-launch pipeline (tuning mode 0) and through the fused kernel on every eligible shape (mode 2);
    the default (mode 1) picks between them by grid size"""
    old = L.lib.aclgan_set_tuning(b"wino_fused", request.param)
    yield request.param
    L.lib.aclgan_set_tuning(b"wino_fused", old)


@pytest.mark.parametrize("case", BLOCK_CASES)
def test_conv_block_fwd(L, case, wino_mode):
    from gpu_util import conv_desc, nhwc, nchw, ohwi, rel_err
    B, H, W, Ci, Co, k, kind, act, use_res, expect_fused = case
    s, p = (2, 1) if k == 4 else (1, 1)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, Ci, H, W, generator=g)
    w = torch.randn(Co, Ci, k, k, generator=g) * (2.0 / (Ci * k * k)) ** 0.5
    b = torch.randn(Co, generator=g) * 0.1
    yc_ref = O.conv_block(x, w, b, s, p, "none")
    res = torch.randn(yc_ref.shape, generator=g) if use_res else None
    if kind == "adain":
        nw, nb = torch.rand(B, Co, generator=g) + 0.5, torch.randn(B, Co, generator=g) * 0.2
    elif kind == "ln":
        nw, nb = torch.rand(Co, generator=g), torch.randn(Co, generator=g) * 0.1
    else:
        nw = nb = None
    y_ref = _norm_ref(kind, act, yc_ref, nw, nb, res)

    d = conv_desc(L, B, H, W, Ci, Co, k, s, p, 0, "none")
    xg, wg, bg = nhwc(x).cuda(), ohwi(w).cuda(), b.cuda()
    nwg = nw.cuda() if nw is not None else None
    nbg = nb.cuda() if nb is not None else None
    resg = nhwc(res).cuda() if use_res else None
    Ho, Wo = yc_ref.shape[2], yc_ref.shape[3]
    yc = torch.empty(B, Ho, Wo, Co, device="cuda"); y = torch.empty_like(yc)
    nstat = B if kind == "ln" else B * Co
    mean = torch.empty(nstat, device="cuda"); rstd = torch.empty(nstat, device="cuda")
    scratch = torch.empty(L.lib.aclgan_conv2d_block_fwd_scratch_bytes(C.byref(d)) // 4 + 64, device="cuda")
    fused = C.c_int(-1)
    L.check(L.lib.aclgan_conv2d_block_fwd(C.byref(d), L.NORM[kind], L.ACT[act], L.ptr(xg), L.ptr(wg), L.ptr(bg), L.ptr(nwg), L.ptr(nbg),
                                          Co if kind == "adain" else 0, L.ptr(resg), L.ptr(yc), L.ptr(y), L.ptr(mean), L.ptr(rstd),
                                          L.ptr(scratch), C.byref(fused), L.stream_ptr()), "conv2d_block_fwd")
    if expect_fused == "s2":      # (round 6) the stride-2 layers take the fused kernel in forced mode (2); the default asks the cost model
        expect_fused = wino_mode == 2
    assert fused.value == int(expect_fused)
    assert rel_err(nchw(yc), yc_ref) < TOL
    assert rel_err(nchw(y), y_ref) < TOL
    # the statistics the block saved for the backward = those of the separate normalisation operator on the same conv output
    y2 = torch.empty_like(y); mean2 = torch.empty_like(mean); rstd2 = torch.empty_like(rstd)
    nscr = torch.empty(L.lib.aclgan_norm_scratch_bytes(B, Ho * Wo, Co) // 4 + 16, device="cuda")
    L.check(L.lib.aclgan_norm_fwd(L.NORM[kind], L.ACT[act], B, Ho * Wo, Co, L.ptr(yc), L.ptr(nwg), L.ptr(nbg), Co if kind == "adain" else 0,
                                  L.ptr(resg), L.ptr(y2), L.ptr(mean2), L.ptr(rstd2), L.ptr(nscr), L.stream_ptr()), "norm_fwd")
    assert rel_err(mean, mean2) < 1e-5 and rel_err(rstd, rstd2) < 1e-5
    assert rel_err(y, y2) < 1e-5


@pytest.mark.parametrize("shape", [(2, 6, 64, 64), (1, 3, 7, 9), (3, 3, 32, 32), (2, 6, 2, 2)])
def test_avgpool(L, shape):
    from gpu_util import nhwc, nchw, rel_err
    B, Cn, H, W = shape
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, Cn, H, W, generator=g).requires_grad_(True)
    y = O.avgpool3s2(x)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy)
    xg = nhwc(x.detach()).cuda()
    yg = torch.empty(B, y.shape[2], y.shape[3], Cn, device="cuda")
    L.check(L.lib.aclgan_avgpool3s2_fwd(B, H, W, Cn, L.ptr(xg), L.ptr(yg), L.stream_ptr()))
    assert rel_err(nchw(yg), y) < 1e-6
    dxg = torch.full_like(xg, float("nan"))
    dyg = nhwc(dy).cuda()   # named: a temporary could be freed and reused before the launch
    L.check(L.lib.aclgan_avgpool3s2_bwd(B, H, W, Cn, L.ptr(dyg), L.ptr(dxg), 0, L.stream_ptr()))
    assert rel_err(nchw(dxg), x.grad) < 1e-6


def test_adam_flat_matches_torch_adam(L):
    """3 steps of the fused kernel vs torch.optim.Adam(weight_decay=...) on the same grads (trainer.py:39-42)."""
    n = 100003
    g = torch.Generator().manual_seed(4)
    p0 = torch.randn(n, generator=g)
    p_ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p_ref], lr=1e-4, betas=(0.5, 0.999), weight_decay=1e-4)
    p = p0.clone().cuda(); m = torch.zeros(n, device="cuda"); v = torch.zeros(n, device="cuda")
    a = L.Adam(1e-4, 0.5, 0.999, 1e-8, 1e-4)
    for step in range(1, 4):
        grad = torch.randn(n, generator=g) * 0.01
        p_ref.grad = grad.clone()
        opt.step()
        gg = grad.cuda()
        L.check(L.lib.aclgan_adam_flat(L.ptr(p), L.ptr(gg), L.ptr(m), L.ptr(v), n, C.byref(a), step, L.stream_ptr()))
    assert (p.cpu() - p_ref.detach()).abs().max().item() < 2e-7


def test_layout_roundtrip(L):
    x = torch.randn(3, 5, 6, 7, device="cuda")
    y = torch.empty(3, 6, 7, 5, device="cuda"); z = torch.empty_like(x)
    L.check(L.lib.aclgan_nchw_to_nhwc(L.ptr(x), L.ptr(y), 3, 5, 6, 7, L.stream_ptr()))
    L.check(L.lib.aclgan_nhwc_to_nchw(L.ptr(y), L.ptr(z), 3, 5, 6, 7, L.stream_ptr()))
    assert torch.equal(y, x.permute(0, 2, 3, 1).contiguous()) and torch.equal(z, x)


def test_errors_are_reported_not_fatal(L):
    d = L.ConvDesc(1, 2, 2, 4, 4, 7, 1, 3, 0, 0)   # reflect pad 3 on a 2x2 map: torch raises too
    rc = L.lib.aclgan_conv2d_fwd(C.byref(d), None, None, None, None, None)
    assert rc == -1 and "reflect" in L.last_error()
