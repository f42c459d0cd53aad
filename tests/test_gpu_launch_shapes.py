"""Every convolution and normalisation layer of the benchmarked steps, at its own launch shape, against a float64 reference.

The operator tests (test_gpu_ops*.py, test_gpu_sweep.py) compare each kernel with the oracle elementwise at small shapes; the kernel a
layer gets and its launch grid depend on the shape (split-K and split_nwg in conv_fast.hip, glds_tile in conv_glds16.hip, the ordered
slices of conv_wgrad_kc_kernel, the tiles per workgroup of the thin-input kernels, the halo ring of the 3x3 input gradient, the LayerNorm
slices and finalize rounds), so the launches the benchmark times were largely not the ones tested.  At the benchmarked shapes the backward
kernels were seen only through the relative L2 of whole parameter gradients (test_gpu_fullsize.py), which hides an error confined to one
row, slice or tile seam.  This module closes that gap:

  * the launch table -- every distinct layer (B, Hi, Wi, Ci, Co, k, s, p, upsample, activation, norm, residual) the step executes for each
    single-GPU workload bench.py times -- is DERIVED from the oracle: the arguments of O.conv_block are recorded during one dis_update and
    one gen_update loss graph at B = 1 (on the meta device: shapes only), then the batch is scaled; the launches the engine makes at another
    batch (discriminator passes over concatenated batches) or outside conv_block (the 1x1 discriminator heads) are added explicitly;
  * fp32 layers: forward (aclgan_conv2d_fwd_ws; aclgan_conv2d_block_fwd for normalised layers, epilogue statistics and residual included),
    input gradient (aclgan_conv2d_dgrad, plain and accumulating onto a nonzero base), weight and bias gradient (aclgan_conv2d_wgrad_ws)
    against the oracle in float64 (torch on the GPU in fp64: MIOpen has no fp64 convolution, so this is torch's own im2col + GEMM,
    independent of the kernels under test): elementwise max-abs / max |ref| <= 2e-4, the bound of test_gpu_ops.py;
  * 16-bit layers (bf16 B = 8, fp16 B = 32): every 16-bit entry point the engine's own predicates (aclgan_conv16_eligible,
    aclgan_conv16s_ok) admit for the layer, with the default tile choices, under the exact-operand contract of test_gpu_ops16s.py;
  * every normalised layer through aclgan_norm_fwd_x / aclgan_norm_bwd_x, with the step's own operands: conv-epilogue statistics, the
    storage codes the engine uses at that layer, the fused scale / shift (ss) the backward rebuilds the activation mask from, and the
    deferred LayerNorm gamma / beta totals (sbc + aclgan_norm_bwd_ln_params);
  * the small operators (linear, MLP, global average pool, avgpool, losses) at the step's batch sizes and pixel counts.

Per-sample passes (forward, input gradient) are checked on samples 0, B // 2 and B - 1 while the kernel runs the whole batch; the weight
gradient sums over the batch, so its reference is the whole batch.  A failure names the workload, the mode, the layer (its parameter names),
the pass and the worst element with its position.  Run with -s for the table of worst errors.

Both plans of the library are checked (the `mode` parameter, ids "<workload>" and "<workload>-det"; the mode is set explicitly either way, so
the module means the same under ACLGAN_DETERMINISTIC=1).  The deterministic plan (aclgan_set_deterministic) replaces every fp32 atomic of the
default plan: padded-grid input gradients with an ordered fold, the Winograd ring stored on a zeroed grid, per-slice weight-gradient copies
added in order, ordered bias column sums, no split-K.  In that mode every scratch buffer is sized after the mode is set and filled with NaN
before the call, so a padded-grid position no launch writes (or a memset misses) shows in the output instead of a zero the allocator happened
to return; every backward pass runs a second time on scratch filled with +inf and must give the same bits.  Its one contract difference: the
16-bit input gradient of the sub-pixel layers is the plain rounded 5x5 (oracle compute_dtype(up5_dgrad="plain")), not the merged phase
filters of the default plan."""
import ctypes as C
import os
import time
from collections import OrderedDict

import pytest
import torch
import torch.nn.functional as F

from oracle import aclgan_oracle as O

pytestmark = pytest.mark.gpu

TOL = 2e-4                                   # test_gpu_ops.py (fp32: differences are summation order)
ULP = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the single-GPU workloads bench.py times: (name, yaml, image size, compute dtype, per-GPU batch)
WORKLOADS = [
    ("fp32_256_b8", "male2female.yaml", 256, "fp32", 8),      # headline (BASELINE configs[1])
    ("fp32_512_b4", "glasses_removal.yaml", 512, "fp32", 4),  # BASELINE configs[3]
    ("bf16_256_b8", "selfie2anime.yaml", 256, "bf16", 8),     # BASELINE configs[2], per GPU
    ("fp16_256_b32", "male2female.yaml", 256, "fp16", 32),    # BASELINE configs[4], per GPU
    ("fp32_256_b3", "male2female.yaml", 256, "fp32", 3),      # the reference's own batch (configs/male2female.yaml batch_size)
]
WL = {w[0]: w for w in WORKLOADS}

RESULTS = []          # (workload/mode, layer, pass, worst error, bound)
MODES = ("default", "det")


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib
    yield _lib
    if RESULTS:
        print("\nworst error per (workload, layer, pass) -- max |got - ref| / max |ref| unless noted; bit-identity checks: 0 = identical;"
              " mask checks: number of disagreeing signs")
        print("workload | layer | pass | worst | bound")
        for wl, lay, ps, err, bound in RESULTS:
            print("%s | %s | %s | %.2e | %.1e" % (wl, lay, ps, err, bound))


@pytest.fixture
def mode(L, request):
    """the library's plan for one test: "default" (mode 0, set explicitly) or "det"; the previous mode is restored afterwards"""
    from gpu_util import deterministic_mode
    with deterministic_mode(L, request.param == "det"):
        yield request.param


def _modes(values):
    """(value, mode) parameters: the default plan keeps the value's own id, the deterministic plan's id ends in -det"""
    return [pytest.param(v, m, id=str(v) if m == "default" else "%s-det" % v) for m in MODES for v in values]


def _det(L):
    return L.lib.aclgan_get_deterministic() == 1


# ----------------------------------------------------------------------------------------------------------------------------------
# 1. the launch table
# ----------------------------------------------------------------------------------------------------------------------------------
def _config(yaml_name):
    import yaml
    with open(os.path.join(ROOT, "configs", yaml_name)) as f:
        y = yaml.safe_load(f)
    cfg = O.default_config()
    for k in ("gen", "dis"):
        cfg[k].update({kk: y[k][kk] for kk in cfg[k] if kk in y[k]})
    for k in ("input_dim_a", "input_dim_b", "focus_loss", "alpha"):
        if k in y:
            cfg[k] = y[k]
    return cfg


_RECORDED = {}


def recorded_layers(yaml_name, S):
    """the O.conv_block calls of one dis_update and one gen_update loss graph at B = 1 (meta tensors: shapes only, no arithmetic)"""
    key = (yaml_name, S)
    if key in _RECORDED:
        return _RECORDED[key]
    cfg = _config(yaml_name)
    nets = {n: {k: t.to("meta") for k, t in P.items()} for n, P in O.test_nets(cfg, 0).items()}
    names = {id(t): "%s/%s" % (n, k[:-len(".weight")]) for n, P in nets.items() for k, t in P.items() if k.endswith(".weight")}
    x_a = torch.empty(1, cfg["input_dim_a"], S, S, device="meta")
    x_b = torch.empty(1, cfg["input_dim_a"], S, S, device="meta")
    z = [torch.empty(1, cfg["gen"]["style_dim"], 1, 1, device="meta") for _ in range(3)]
    rec = []
    orig = O.conv_block

    def recording(x, w, b, stride, pad, act="none", norm="none", norm_args=None, upsample=False, out16=True, g16=True, residual_follows=False):
        rec.append(dict(name=names[id(w)], B=x.shape[0], Hi=x.shape[2], Wi=x.shape[3], Ci=x.shape[1], Co=w.shape[0], k=w.shape[2], s=stride,
                        p=pad, up=int(bool(upsample)), act=act, norm=norm, res=bool(residual_follows), out16=bool(out16)))
        return orig(x, w, b, stride, pad, act, norm, norm_args, upsample, out16, g16, residual_follows)

    O.conv_block = recording
    try:
        with torch.no_grad():
            O.dis_losses(nets, x_a, x_b, z, cfg)
            O.gen_losses(nets, x_a, x_b, z, cfg)
    finally:
        O.conv_block = orig
    _RECORDED[key] = (cfg, rec)
    return cfg, rec


GEOM = ("B", "Hi", "Wi", "Ci", "Co", "k", "s", "p", "up", "act", "norm", "res")


def launch_table(wl):
    """distinct layers the engine launches for workload wl: OrderedDict geometry tuple -> dict(names, out16, why = reason of an added batch)"""
    name, yaml_name, S, dt, B = WL[wl]
    cfg, rec = recorded_layers(yaml_name, S)
    table = OrderedDict()

    def add(ent, batch, why=None):
        e = dict(ent, B=batch)
        key = tuple(e[k] for k in GEOM)
        t = table.setdefault(key, dict(names=[], out16=e["out16"], why=why))
        if e["name"] not in t["names"]:
            t["names"].append(e["name"])
    heads = OrderedDict()
    last = ".%d.conv" % (cfg["dis"]["n_layer"] - 1)
    for ent in rec:
        if not ent["name"].startswith("dis_"):
            add(ent, B)                       # generator passes run at the step's batch, one call per use
            continue
        # the discriminators run over JOINT batches (engine_graph.hip dis_lsgan): gen_update dis_B (B), dis_A (x_A_fake | x_A2_fake: 2B),
        # dis_2 (pair_A1 | pair_A2: 2B); dis_update dis_B (x_B_fake | x_b: 2B), dis_A (x_A_fake | x_A2_fake | x_a: 3B), dis_2 (2B).
        # The oracle calls every network once per input; dis_A / dis_B share their shapes, dis_2 differs in its first layer only.
        for m in ((2,) if ent["name"].startswith("dis_2") else (1, 2, 3)):
            add(ent, m * B, "joint discriminator batch")
            if ent["name"].endswith(last):
                # the 1x1 head of the scale (networks.py:45) on this layer's output: F.conv2d in the oracle, a conv_block launch in the engine
                Ho, Wo = _out_hw((1, ent["Hi"], ent["Wi"], ent["Ci"], ent["Co"], ent["k"], ent["s"], ent["p"], ent["up"]))
                heads.setdefault((m * B, Ho, Wo, ent["Co"], 1, 1, 1, 0, 0, "none", "none", False), []).append(ent["name"][:-len(last)] + ".%d" % cfg["dis"]["n_layer"])
    for key, nms in heads.items():
        table.setdefault(key, dict(names=sorted(set(nms)), out16=True, why="discriminator head"))
    return table


# distinct layers per workload: 15 generator layers at B, the discriminator's 12 strided convolutions + 3 heads at B, 2B and 3B, the
# three 6-channel first layers of dis_2 at 2B
TABLE_SIZE = 15 + 3 * 15 + 3


def _lname(g, ent):
    return "%s%s B=%d" % (ent["names"][0], " +%d" % (len(ent["names"]) - 1) if len(ent["names"]) > 1 else "", g[0])


def test_launch_table_is_complete():
    """the table of every workload has every layer, and the generator's recorded passes have the structure of the reference networks"""
    for wl, _, S, _, B in WORKLOADS:
        t = launch_table(wl)
        assert len(t) == TABLE_SIZE, (wl, len(t))
        kinds = {}
        for g in t:
            kinds[g[10]] = kinds.get(g[10], 0) + 1
        assert kinds == {"none": TABLE_SIZE - 9, "in": 5, "adain": 2, "ln": 2}, (wl, kinds)
        assert sum(1 for g in t if g[11]) == 2                          # the second convolution of the encoder / decoder ResBlocks
        assert {g[0] for g in t} == {B, 2 * B, 3 * B}
        assert max(g[1] for g in t) == S and sum(1 for g in t if g[8]) == 2
    _, rec = recorded_layers("male2female.yaml", 256)
    assert len(rec) == 336            # every conv_block call of the two loss graphs (generators and discriminators, full width)


# ----------------------------------------------------------------------------------------------------------------------------------
# helpers
# ----------------------------------------------------------------------------------------------------------------------------------
def _desc(L, g, act=None):
    B, Hi, Wi, Ci, Co, k, s, p, up, a, norm, res = g
    return L.ConvDesc(B, Hi, Wi, Ci, Co, k, s, p, up, L.ACT[a if act is None else act])


def _out_hw(g):
    B, Hi, Wi, Ci, Co, k, s, p, up = g[:9]
    return ((Hi << up) + 2 * p - k) // s + 1, ((Wi << up) + 2 * p - k) // s + 1


def _samples(B):
    return sorted({0, B // 2, B - 1})


def _scr(nbytes, fill=None):
    """scratch of nbytes (+ 256 bytes); fill: the value every element starts as (deterministic mode: NaN, +inf for a second run)"""
    n = int(nbytes) // 4 + 64
    return torch.empty(n, device="cuda") if fill is None else torch.full((n,), fill, device="cuda")


NAN, INF = float("nan"), float("inf")


def _where(idx, shape, what, rows=None):
    """position of the worst element (NHWC activation or OHWI weight; rows: batch index of each checked sample) and its coordinates in the
    implicit GEMM every convolution kernel here computes: an activation pixel is GEMM row m = (b H + y) W + x, so a wrong M tile of R rows
    shows as m // R; a weight entry is column (ky kw + kx) Ci + ci of row co.  Which kernel and tile the library chose is not visible
    through the C ABI; these coordinates and the distance from the border (reflection halo, sub-pixel ring) locate it for any of them."""
    pos = []
    for n in reversed(shape):
        pos.append(idx % n)
        idx //= n
    pos = pos[::-1]
    if what == "act" and len(pos) == 4:
        b, y, x, c = pos
        b = rows[b] if rows is not None else b
        H, W = shape[1], shape[2]
        ring = min(y, x, H - 1 - y, W - 1 - x)
        m = (b * H + y) * W + x
        return "(b, y, x, c) = (%d, %d, %d, %d) of %dx%d: %d pixels from the border, GEMM row m = %d (m // 128 = %d, m // 256 = %d), channel c // 64 = %d" % (
            b, y, x, c, H, W, ring, m, m // 128, m // 256, c // 64)
    if what == "w":
        co, ky, kx, ci = pos
        kk = (ky * shape[2] + kx) * shape[3] + ci
        return "(co, ky, kx, ci) = (%d, %d, %d, %d): GEMM column k = %d of %d (k // 64 = %d), row co // 64 = %d" % (
            co, ky, kx, ci, kk, shape[1] * shape[2] * shape[3], kk // 64, co // 64)
    return "index %s" % (tuple(pos),)


class Check:
    """collects the comparisons of one test; fails at the end with every offending (layer, pass)"""

    def __init__(self, wl, mode=None):
        self.wl, self.bad = wl if mode is None else "%s/%s" % (wl, mode), []

    def __call__(self, lay, ps, got, ref, bound, what="act", rows=None):
        got = got.detach().double()
        ref = ref.detach().double().to(got.device)
        d = (got - ref).abs()
        den = ref.abs().max().clamp_min(1e-30)
        err = (d.max() / den).item() if d.numel() else 0.0
        if not err == err:          # NaN somewhere in the output
            err = float("inf")
        RESULTS.append((self.wl, lay, ps, err, bound))
        if not err <= bound:
            idx = int(torch.nan_to_num(d, nan=float("inf")).reshape(-1).argmax())
            shape = list(got.shape)
            loc = _where(idx, shape, what, rows)
            self.bad.append("%s %s %s: %.3e > %.1e at %s" % (self.wl, lay, ps, err, bound, loc))
        return err

    def equal(self, lay, ps, a, b):
        ok = torch.equal(a, b)
        RESULTS.append((self.wl, lay, ps, 0.0 if ok else float("inf"), 0.0))
        if not ok:
            d = (a.double() - b.double()).abs()
            idx = int(torch.nan_to_num(d, nan=float("inf")).reshape(-1).argmax())
            self.bad.append("%s %s %s: not bit-identical, first worst at %s" % (self.wl, lay, ps, _where(idx, list(a.shape), "act" if a.dim() == 4 else "")))

    def count(self, lay, ps, n):
        RESULTS.append((self.wl, lay, ps, float(n), 0.0))
        if n:
            self.bad.append("%s %s %s: %d disagreements" % (self.wl, lay, ps, n))

    def done(self):
        assert not self.bad, "\n".join(self.bad)


def _nchw64(t):
    return t.permute(0, 3, 1, 2).double()


def _oihw64(w):
    return w.permute(0, 3, 1, 2).double()


def _tensors(g, seed, grid_w=False):
    """x (NHWC), w (OHWI), bias for layer geometry g, on the GPU"""
    B, Hi, Wi, Ci, Co, k, s, p, up = g[:9]
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(B, Hi, Wi, Ci, device="cuda", generator=gen)
    if grid_w:   # 1/8 grid times 2^-4: sums of up to four taps (the merged sub-pixel phase filters) stay exact in bf16 / fp16
        w = torch.randint(-3, 4, (Co, k, k, Ci), device="cuda", generator=gen).float() / 128.0
    else:
        w = torch.randn(Co, k, k, Ci, device="cuda", generator=gen) * (2.0 / (Ci * k * k)) ** 0.5
    b = torch.randn(Co, device="cuda", generator=gen) * 0.1
    return x, w, b, gen


def _ref_conv(x64, w64, b64, g, act="none"):
    B, Hi, Wi, Ci, Co, k, s, p, up = g[:9]
    return O.conv_block(x64, w64, b64, s, p, act, upsample=bool(up))


def _ref_wgrad(x, dy, w, g, chunk_bytes=2 << 30):
    """dw (OHWI), db over the whole batch in float64, chunked by samples"""
    B, Hi, Wi, Ci, Co, k, s, p, up = g[:9]
    w64 = _oihw64(w).requires_grad_(True)
    per = (x[0].numel() << (2 * up)) * k * k * 8 + x[0].numel() * 8
    n = max(1, min(B, chunk_bytes // max(per, 1)))
    dw = torch.zeros_like(w64)
    db = torch.zeros(Co, dtype=torch.float64, device="cuda")
    for i in range(0, B, n):
        xs = _nchw64(x[i:i + n])
        dys = _nchw64(dy[i:i + n])
        y = O._plain_conv(xs, w64, s, p, bool(up))
        dw += torch.autograd.grad(y, w64, dys)[0]
        db += dys.sum(dim=(0, 2, 3))
    return dw.permute(0, 2, 3, 1), db


def _ref_dgrad(dy_s, w64, g, xshape):
    B, Hi, Wi, Ci, Co, k, s, p, up = g[:9]
    xs = torch.zeros(xshape, dtype=torch.float64, device="cuda", requires_grad=True)
    y = O._plain_conv(xs, w64, s, p, bool(up))
    return torch.autograd.grad(y, xs, _nchw64(dy_s))[0].permute(0, 2, 3, 1)


# ----------------------------------------------------------------------------------------------------------------------------------
# norms (part 4): one normalised layer with the step's operands
# ----------------------------------------------------------------------------------------------------------------------------------
def _norm_params(kind, B, Co, gen):
    """AdaIN: two slices of a row-strided MLP output (bias | weight of one layer, networks.py:154-163); LN: gamma / beta"""
    if kind == "adain":
        width = 2 * Co * 4                  # 4 AdaIN layers per decoder at full width: 2048 bias + weight columns
        ap = torch.randn(B, width, device="cuda", generator=gen) * 0.3
        ap[:, 3 * Co:4 * Co] += 1.0         # layer 1: bias = columns [2C, 3C), weight = [3C, 4C)
        return ap, 2 * Co, 3 * Co, width
    if kind == "ln":
        return torch.cat([torch.rand(Co, device="cuda", generator=gen) + 0.5, torch.randn(Co, device="cuda", generator=gen) * 0.1]), Co, 0, 0
    return None, 0, 0, 0


def _norm_wb(kind, P, bcol, wcol, Co):
    if kind == "adain":
        return P[:, wcol:wcol + Co], P[:, bcol:bcol + Co]
    if kind == "ln":
        return P[:Co], P[Co:]
    return None, None


def _norm_ref64(kind, act, x64, w, b, res64, mask=None):
    """fp64 normalisation (+ activation with the KERNEL's sign decisions where given -- a pre-activation within rounding of zero must not
    decide the comparison) (+ residual), NCHW"""
    w = None if w is None else w.double()
    b = None if b is None else b.double()
    if kind == "in":
        y = O.instance_norm(x64)
    elif kind == "adain":
        y = O.adain(x64, w, b)
    else:
        y = O.layer_norm_munit(x64, w, b)
    if act in ("relu", "lrelu") and mask is not None:
        y = torch.where(mask, y, y * (0.0 if act == "relu" else 0.2))
    else:
        y = O._act(y, act)
    return y + res64 if res64 is not None else y


def check_norm_layer(L, chk, lay, g, xc, st, dt_code, gen, stats=None, chunk=0):
    """xc: the conv output as stored (NHWC, fp32 or 16-bit); st = (x, y, res, dy, dx, dres) storage codes as the engine picks them"""
    B, Ho, Wo, Co = xc.shape
    kind, act, use_res = g[10], g[9], g[11]
    HW = Ho * Wo
    K = L.NORM[kind]
    T = lambda code: TDT["bf16" if code == 1 else "fp16"] if code else torch.float32    # noqa: E731
    P, bcol, wcol, wstride = _norm_params(kind, B, Co, gen)
    w, b = _norm_wb(kind, P, bcol, wcol, Co)
    wptr = None if P is None else C.c_void_p(P.data_ptr() + 4 * (wcol if kind == "adain" else 0))
    bptr = None if P is None else C.c_void_p(P.data_ptr() + 4 * (bcol if kind == "adain" else Co))
    res = (torch.randn(B, Ho, Wo, Co, device="cuda", generator=gen)).to(T(st[2])) if use_res else None
    nst = B if kind == "ln" else B * Co
    scr = _scr(L.lib.aclgan_norm_scratch_bytes(B, HW, Co), NAN if _det(L) else None)
    stf = (C.c_int * 3)(st[0], st[1], st[2])

    def fwd(stats_, chunk_, ss_):
        y = torch.full((B, Ho, Wo, Co), float("nan"), device="cuda").to(T(st[1]))
        mean = torch.empty(nst, device="cuda"); rstd = torch.empty(nst, device="cuda")
        L.check(L.lib.aclgan_norm_fwd_x(K, L.ACT[act], B, HW, Co, L.ptr(xc), wptr, bptr, wstride, L.ptr(res), L.ptr(y), L.ptr(mean), L.ptr(rstd),
                                        L.ptr(scr), L.ptr(stats_), chunk_, stf, L.ptr(ss_), L.stream_ptr()), "norm_fwd_x")
        return y, mean, rstd
    ss = torch.full((2 * B * Co,), float("nan"), device="cuda") if act in ("relu", "lrelu") else None
    y, mean, rstd = fwd(stats, chunk, ss)
    y32 = y.float()
    x64 = _nchw64(xc.float())
    r64 = _nchw64(res.float()) if use_res else None
    # the kernel's activation mask: the sign of its own fmaf(x, scale, shift) (what the backward with ss recovers)
    mask = None
    if ss is not None:
        sc, sh = ss[:B * Co].view(B, 1, 1, Co).double(), ss[B * Co:].view(B, 1, 1, Co).double()
        mask = (xc.double() * sc + sh > 0).permute(0, 3, 1, 2)
    ref = _norm_ref64(kind, act, x64, w, b, r64, mask)
    if mask is not None:
        # ss itself: x * scale + shift is the fp64 pre-activation to fp32 accuracy, and its sign (the mask the reference above and the
        # backward with ss use) is the fp64 sign wherever the pre-activation is farther from zero than that accuracy
        pre = _norm_ref64(kind, "none", x64, w, b, None)
        chk(lay, "norm ss: x*scale+shift", (xc.double() * sc + sh), pre.permute(0, 2, 3, 1), TOL)
        clear = pre.abs() > 2 * TOL * pre.abs().max()
        chk.count(lay, "norm ss: mask vs fp64 sign", int((mask != (pre > 0))[clear].sum()))
    ytol = TOL + (ULP[{1: "bf16", 2: "fp16"}[st[1]]] if st[1] else 0.0)
    chk(lay, "norm fwd%s" % (" (conv stats)" if stats is not None else ""), y32, ref.permute(0, 2, 3, 1), ytol)
    if stats is not None:      # the statistics from the conv epilogue == those of the norm's own pass over the same stored values
        y2, mean2, rstd2 = fwd(None, 0, None)
        chk(lay, "norm mean/rstd vs own", torch.cat([mean, rstd]), torch.cat([mean2, rstd2]), 1e-5, what="")
    if st[1]:                  # a 16-bit y is the fp32 result rounded once (same statistics: no conv stats, all-fp32 storage otherwise)
        stf32 = (C.c_int * 3)(st[0], 0, st[2])
        ya = torch.empty(B, Ho, Wo, Co, device="cuda"); m3 = torch.empty(nst, device="cuda"); r3 = torch.empty(nst, device="cuda")
        yb = torch.empty(B, Ho, Wo, Co, device="cuda").to(T(st[1]))
        L.check(L.lib.aclgan_norm_fwd_x(K, L.ACT[act], B, HW, Co, L.ptr(xc), wptr, bptr, wstride, L.ptr(res), L.ptr(ya), L.ptr(m3), L.ptr(r3),
                                        L.ptr(scr), None, 0, stf32, None, L.stream_ptr()), "norm_fwd_x")
        L.check(L.lib.aclgan_norm_fwd_x(K, L.ACT[act], B, HW, Co, L.ptr(xc), wptr, bptr, wstride, L.ptr(res), L.ptr(yb), L.ptr(m3), L.ptr(r3),
                                        L.ptr(scr), None, 0, stf, None, L.stream_ptr()), "norm_fwd_x")
        chk.equal(lay, "norm fwd 16-bit y == fp32 rounded", yb, ya.to(T(st[1])))

    # backward: reference with the kernel's mask -- with ss the sign of its fmaf, without ss the sign of the stored y (a 16-bit y can round
    # a tiny positive pre-activation to zero: fp16 below 2^-25)
    dy = torch.randn(B, Ho, Wo, Co, device="cuda", generator=gen).to(T(st[3]))
    ymask = _nchw64(y32) > 0

    def bwd_ref(m):
        x64r = x64.clone().requires_grad_(True)
        Pr = P.double().requires_grad_(True) if P is not None else None
        wr, br = _norm_wb(kind, Pr, bcol, wcol, Co) if P is not None else (None, None)
        r64r = r64.clone().requires_grad_(True) if use_res else None
        yr = _norm_ref64(kind, act, x64r, wr, br, r64r, m)
        grads = torch.autograd.grad(yr, [t for t in (x64r, Pr, r64r) if t is not None], _nchw64(dy.float()))
        return grads[0].permute(0, 2, 3, 1), (grads[1] if P is not None else None), (grads[-1].permute(0, 2, 3, 1) if use_res else None)
    refs = {"ss": bwd_ref(mask if mask is not None else ymask)}
    refs["no ss"] = refs["sbc"] = refs["ss"]
    if mask is not None and not torch.equal(mask, ymask):
        refs["no ss"] = bwd_ref(ymask)
    stb = (C.c_int * 6)(st[0], st[1], st[3], st[4], st[5], 0)
    out = {}
    for variant in (("ss", "sbc") if kind == "ln" else ("ss",)) + ("no ss",):
        if variant != "no ss" and ss is None:
            continue
        dx = torch.full((B, Ho, Wo, Co), float("nan"), device="cuda").to(T(st[4]))
        dres = torch.full((B, Ho, Wo, Co), float("nan"), device="cuda").to(T(st[5])) if use_res else None
        dP = torch.zeros_like(P) if P is not None else None
        dwp = None if P is None else C.c_void_p(dP.data_ptr() + 4 * (wcol if kind == "adain" else 0))
        dbp = None if P is None else C.c_void_p(dP.data_ptr() + 4 * (bcol if kind == "adain" else Co))
        sbc = torch.full((B * Co * 2,), float("nan"), device="cuda") if variant == "sbc" else None
        L.check(L.lib.aclgan_norm_bwd_x(K, L.ACT[act], B, HW, Co, L.ptr(xc), L.ptr(y), L.ptr(dy), wptr, wstride, L.ptr(mean), L.ptr(rstd),
                                        L.ptr(dx), dwp, dbp, L.ptr(dres), 0, L.ptr(scr), stb, L.ptr(ss if variant != "no ss" else None),
                                        L.ptr(sbc), L.stream_ptr()), "norm_bwd_x")
        if variant == "sbc":
            assert float(dP.abs().max()) == 0.0, "norm_bwd_x with sbc_out must leave gamma / beta alone"
            L.check(L.lib.aclgan_norm_bwd_ln_params(L.ptr(sbc), B, Co, dwp, dbp, L.stream_ptr()), "norm_bwd_ln_params")
        out[variant] = (dx, dres, dP)
        gx, gP, gres = refs[variant]
        dxtol = 5 * TOL + (2 * ULP[{1: "bf16", 2: "fp16"}[st[4]]] if st[4] else 0.0)
        chk(lay, "norm bwd dx (%s)" % variant, dx.float(), gx, dxtol)
        if use_res:
            chk(lay, "norm bwd dres (%s)" % variant, dres.float(), gres, TOL + (ULP[{1: "bf16", 2: "fp16"}[st[5]]] if st[5] else 0.0))
        if kind == "adain":
            chk(lay, "norm bwd dw,db rows (%s)" % variant, dP[:, bcol:bcol + 2 * Co], gP[:, bcol:bcol + 2 * Co], 5 * TOL, what="")
            assert float(dP[:, :bcol].abs().max()) == 0.0 and float(dP[:, bcol + 2 * Co:].abs().max()) == 0.0
        elif kind == "ln":
            chk(lay, "norm bwd dgamma,dbeta (%s)" % variant, dP, gP, 5 * TOL, what="")
    if "no ss" in out and "ss" in out:
        # the mask from (x, ss) and the mask from the stored y: the same gradient, except where a positive pre-activation was stored as 0
        a, b_ = out["ss"][0].float(), out["no ss"][0].float()
        differ = (mask != ymask).permute(0, 2, 3, 1)
        assert bool((y32[differ] == 0).all()), (lay, "the two backward masks differ where y is not zero")
        chk(lay, "norm bwd ss vs no ss", torch.where(differ, 0.0, a), torch.where(differ, 0.0, b_),
            2 * ULP[{1: "bf16", 2: "fp16"}[st[4]]] if st[4] else 1e-5)
    if "sbc" in out:
        chk(lay, "norm bwd sbc vs direct", out["sbc"][2], out["ss"][2], 1e-6, what="")


# ----------------------------------------------------------------------------------------------------------------------------------
# 2. fp32 layers
# ----------------------------------------------------------------------------------------------------------------------------------
def check_fp32_layer(L, chk, g, ent, seed, passes=("fwd", "dgrad", "wgrad"), norm_storage=None, dt_code=0):
    B, Hi, Wi, Ci, Co, k, s, p, up, act, norm, use_res = g
    lay = _lname(g, ent)
    Ho, Wo = _out_hw(g)
    x, w, b, gen = _tensors(g, seed)
    S = _samples(B)
    w64, b64 = _oihw64(w), b.double()
    det = _det(L)
    fill = NAN if det else None
    if "fwd" in passes:
        d = _desc(L, g, act if norm == "none" else "none")
        if norm == "none":
            y = torch.full((B, Ho, Wo, Co), float("nan"), device="cuda")
            L.check(L.lib.aclgan_conv2d_fwd_ws(C.byref(d), L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(y), L.ptr(_scr(L.lib.aclgan_conv2d_fwd_scratch_bytes(C.byref(d)), fill)),
                                               L.stream_ptr()), "conv2d_fwd_ws")
            ref = _ref_conv(_nchw64(x[S]), w64, b64, g, act).permute(0, 2, 3, 1)
            chk(lay, "fwd", y[S], ref, TOL, rows=S)
        else:
            P, bcol, wcol, wstride = _norm_params(norm, B, Co, gen)
            nw, nb = _norm_wb(norm, P, bcol, wcol, Co)
            nwp = None if P is None else C.c_void_p(P.data_ptr() + 4 * (wcol if norm == "adain" else 0))
            nbp = None if P is None else C.c_void_p(P.data_ptr() + 4 * (bcol if norm == "adain" else Co))
            res = torch.randn(B, Ho, Wo, Co, device="cuda", generator=gen) if use_res else None
            yc = torch.full((B, Ho, Wo, Co), float("nan"), device="cuda"); y = torch.full_like(yc, float("nan"))
            nst = B if norm == "ln" else B * Co
            mean = torch.empty(nst, device="cuda"); rstd = torch.empty(nst, device="cuda")
            fused = C.c_int(-1)
            L.check(L.lib.aclgan_conv2d_block_fwd(C.byref(d), L.NORM[norm], L.ACT[act], L.ptr(x), L.ptr(w), L.ptr(b), nwp, nbp, wstride, L.ptr(res),
                                                  L.ptr(yc), L.ptr(y), L.ptr(mean), L.ptr(rstd),
                                                  L.ptr(_scr(L.lib.aclgan_conv2d_block_fwd_scratch_bytes(C.byref(d)), fill)), C.byref(fused), L.stream_ptr()),
                    "conv2d_block_fwd")
            ycr = _ref_conv(_nchw64(x[S]), w64, b64, g)
            chk(lay, "fwd conv", yc[S], ycr.permute(0, 2, 3, 1), TOL, rows=S)
            # the norm over the kernel's own conv output (the conv error is checked above; the norm is per sample)
            wS = nw[S] if norm == "adain" else nw
            bS = nb[S] if norm == "adain" else nb
            ref = _norm_ref64(norm, act, _nchw64(yc[S]), wS, bS, _nchw64(res[S]) if use_res else None)
            chk(lay, "fwd block%s" % (" (epilogue stats)" if fused.value else ""), y[S], ref.permute(0, 2, 3, 1), TOL, rows=S)
            if norm_storage is not None:
                check_norm_layer(L, chk, lay, g, yc, norm_storage, dt_code, gen)
    d = _desc(L, g)          # the engine's descriptor for the backward kernels (desc.act as in the forward of a norm-free layer)
    if norm != "none":
        d = _desc(L, g, "none")
    if "dgrad" in passes or "wgrad" in passes:
        dy = torch.randn(B, Ho, Wo, Co, device="cuda", generator=gen)
    if "dgrad" in passes:
        nb = L.lib.aclgan_conv2d_dgrad_scratch_bytes(C.byref(d))

        def dgrad(out, acc, fill_):
            scr = _scr(nb, fill_)
            L.check(L.lib.aclgan_conv2d_dgrad(C.byref(d), L.ptr(dy), L.ptr(w), L.ptr(out), L.ptr(scr), acc, L.stream_ptr()), "conv2d_dgrad")
            return out
        dx = dgrad(torch.full((B, Hi, Wi, Ci), NAN, device="cuda"), 0, fill)
        ref = _ref_dgrad(dy[S], w64, g, (len(S), Ci, Hi, Wi))
        chk(lay, "dgrad", dx[S], ref, TOL, rows=S)
        # accumulate (a tensor with two consumers, the ResBlock input): onto a nonzero base of the gradient's own magnitude
        base = torch.randn(B, Hi, Wi, Ci, device="cuda", generator=gen) * float(ref.abs().max())
        acc = dgrad(base.clone(), 1, fill)
        chk(lay, "dgrad accumulate", (acc[S].double() - base[S].double()), ref, TOL, rows=S)
        if det:       # a second run on scratch poisoned differently: the same bits
            chk.equal(lay, "dgrad det rerun", dgrad(torch.full((B, Hi, Wi, Ci), NAN, device="cuda"), 0, INF), dx)
            chk.equal(lay, "dgrad accumulate det rerun", dgrad(base.clone(), 1, INF), acc)
    if "wgrad" in passes:
        nb = L.lib.aclgan_conv2d_wgrad_scratch_bytes(C.byref(d))

        def wgrad(fill_):
            dw = torch.zeros(Co, k, k, Ci, device="cuda"); db = torch.zeros(Co, device="cuda")      # (the weight gradient accumulates)
            L.check(L.lib.aclgan_conv2d_wgrad_ws(C.byref(d), L.ptr(x), L.ptr(dy), L.ptr(dw), L.ptr(db), L.ptr(_scr(nb, fill_)), L.stream_ptr()),
                    "conv2d_wgrad_ws")
            return dw, db
        dw, db = wgrad(fill)
        rdw, rdb = _ref_wgrad(x, dy, w, g)
        chk(lay, "wgrad dw", dw, rdw, TOL, what="w")
        chk(lay, "wgrad db", db, rdb, TOL, what="")
        if det:
            dw2, db2 = wgrad(INF)
            chk.equal(lay, "wgrad dw det rerun", dw2, dw)
            chk.equal(lay, "wgrad db det rerun", db2, db)


@pytest.mark.parametrize("wl,mode", _modes(["fp32_256_b8", "fp32_512_b4", "fp32_256_b3"]), indirect=["mode"])
def test_fp32_layers_at_launch_shape(L, wl, mode):
    t0 = time.time()
    chk = Check(wl, mode)
    for i, (g, ent) in enumerate(launch_table(wl).items()):
        check_fp32_layer(L, chk, g, ent, 100 + i, norm_storage=(0, 0, 0, 0, 0, 0) if g[10] != "none" else None)
    torch.cuda.synchronize()
    print("\n%s/%s: %d layers in %.1f s" % (wl, mode, len(launch_table(wl)), time.time() - t0))
    chk.done()


# ----------------------------------------------------------------------------------------------------------------------------------
# 3. 16-bit layers
# ----------------------------------------------------------------------------------------------------------------------------------
def _packs(L, w, code):
    Co, kh, kw, Ci = w.shape
    w16 = torch.empty(w.numel(), dtype=torch.int16, device="cuda")
    w16t = torch.empty(w.numel(), dtype=torch.int16, device="cuda")
    L.check(L.lib.aclgan_pack_weights16(L.ptr(w), L.ptr(w16), L.ptr(w16t), Co, kh * kw, Ci, code, L.stream_ptr()), "pack_weights16")
    return w16, w16t


def _ref16(x, w, b, g, dt, dy=None, up5_dgrad="merged"):
    """the 16-bit compute contract in float64 (oracle _ConvQ: both operands rounded; the sub-pixel layers round the merged phase filters
    in the forward, and in the input gradient of the default plan -- up5_dgrad="plain": the rounded 5x5, the deterministic plan)"""
    B, Hi, Wi, Ci, Co, k, s, p, up = g[:9]
    with O.compute_dtype(dt, storage=False, up5_dgrad=up5_dgrad):
        xr = _nchw64(x).requires_grad_(dy is not None)
        wr = _oihw64(w).requires_grad_(dy is not None)
        y = O._ConvQ.apply(xr, wr, b.double(), s, p, bool(up), True, True, True)
        if dy is None:
            return y.permute(0, 2, 3, 1).detach()
        gx, gw = torch.autograd.grad(y, [xr, wr], _nchw64(dy.float()))
        return gx.permute(0, 2, 3, 1), gw.permute(0, 2, 3, 1)


def check_16bit_layer(L, chk, g, ent, dt, seed, last_dec_res):
    B, Hi, Wi, Ci, Co, k, s, p, up, act, norm, use_res = g
    code = L.DTYPE[dt]
    T = TDT[dt]
    lay = _lname(g, ent)
    Ho, Wo = _out_hw(g)
    d_f = _desc(L, g, act if norm == "none" else "none")
    d_b = _desc(L, g, act if norm == "none" else "none")
    f16, d16, w16 = (L.lib.aclgan_conv16_eligible(C.byref(d_f), i) == 1 for i in range(3))
    s_bwd = f16 and d16 and w16 and L.lib.aclgan_conv16s_ok(C.byref(d_b), 1) == 1
    s_fwd = f16 and L.lib.aclgan_conv16s_ok(C.byref(d_f), 0) == 1 and Ci % 64 == 0
    fp32_passes = tuple(ps for ps, ok in (("fwd", f16), ("dgrad", d16), ("wgrad", w16)) if not ok)
    # storage of this layer's tensors in the step (engine_graph.hip conv_block): activations of 64-multiple widths are 16-bit unless they feed an
    # fp32-only consumer (out16); the conv output in front of a norm and the gradients are 16-bit where the 16-bit-storage kernels run
    out_st = code if (Co % 64 == 0 and ent["out16"]) else 0
    x_st = code if Ci % 64 == 0 else 0
    co_st = code if (norm != "none" and s_bwd) else 0
    out_gst = out_st if not (norm == "ln" or last_dec_res) else 0          # (consumed by a sub-pixel layer: its input gradient is fp32)
    norm_st = (co_st, out_st, code if use_res else 0, out_gst, co_st, code if use_res else 0)
    if fp32_passes:
        check_fp32_layer(L, chk, g, ent, seed, fp32_passes, norm_st if "fwd" in fp32_passes and norm != "none" else None, code)
    if not (f16 or d16 or w16):
        return
    x, w, b, gen = _tensors(g, seed + 7, grid_w=bool(up))
    xq = x.to(T).float()                      # the operand values (a 16-bit x is the same numbers)
    S = _samples(B)
    det = _det(L)
    fill = NAN if det else None
    w16p, w16t = _packs(L, w, code)
    if f16:
        yref = _ref16(xq[S], w, b, g, dt)
        if norm == "none":
            yref = O._act(yref, act)
        x16 = x.to(T)
        if s_fwd:
            y32 = torch.full((B, Ho, Wo, Co), float("nan"), device="cuda")
            L.check(L.lib.aclgan_conv2d_fwd16s(C.byref(d_f), code, L.ptr(x16), L.ptr(w16p), L.ptr(b), L.ptr(y32), 0, L.stream_ptr()), "conv2d_fwd16s")
            chk(lay, "fwd16s", y32[S], yref, TOL, rows=S)
            y16 = torch.full((B, Ho, Wo, Co), float("nan"), device="cuda").to(T)
            L.check(L.lib.aclgan_conv2d_fwd16s(C.byref(d_f), code, L.ptr(x16), L.ptr(w16p), L.ptr(b), L.ptr(y16), code, L.stream_ptr()), "conv2d_fwd16s")
            chk.equal(lay, "fwd16s 16-bit y == fp32 rounded", y16, y32.to(T))
            if norm != "none":
                chunk = L.lib.aclgan_conv2d_fwd16s_stats_chunk(C.byref(d_f))      # (0: the step runs the norm's own statistics pass)
                yc = torch.full((B, Ho, Wo, Co), float("nan"), device="cuda").to(T if co_st else torch.float32)
                stats = torch.full((B * (Ho * Wo // max(chunk, 1)) * Co * 2,), float("nan"), device="cuda")
                L.check(L.lib.aclgan_conv2d_fwd16s_stats(C.byref(d_f), code, L.ptr(x16), L.ptr(w16p), L.ptr(b), L.ptr(yc), co_st, L.ptr(stats),
                                                         L.stream_ptr()), "conv2d_fwd16s_stats")
                chk.equal(lay, "fwd16s_stats y == fwd16s y", yc, y16 if co_st else y32)
                check_norm_layer(L, chk, lay, g, yc, norm_st, code, gen, stats if chunk else None, chunk)
        y = torch.full((B, Ho, Wo, Co), float("nan"), device="cuda")
        L.check(L.lib.aclgan_conv2d_fwd16_x16(C.byref(d_f), code, L.ptr(x16), L.ptr(w), L.ptr(w16p), L.ptr(b), L.ptr(y),
                                              L.ptr(_scr(L.lib.aclgan_conv2d_fwd16_scratch_bytes(C.byref(d_f)), fill)), L.stream_ptr()), "conv2d_fwd16_x16")
        chk(lay, "fwd16_x16", y[S], yref, TOL, rows=S)
        if Co % 64 == 0 and norm == "none" and ent["out16"]:      # a 16-bit y (the step's wide layers without a norm, where the LDS-DMA kernel does not run them) == y rounded
            yst = torch.full((B, Ho, Wo, Co), float("nan"), device="cuda").to(T)
            L.check(L.lib.aclgan_conv2d_fwd16_x16_st(C.byref(d_f), code, L.ptr(x16), L.ptr(w), L.ptr(w16p), L.ptr(b), L.ptr(yst), code,
                                                     L.ptr(_scr(L.lib.aclgan_conv2d_fwd16_scratch_bytes(C.byref(d_f)), fill)), L.stream_ptr()),
                    "conv2d_fwd16_x16_st")
            chk.equal(lay, "fwd16_x16 16-bit y == fp32 rounded", yst, y.to(T))
        if norm != "none" and not s_fwd:      # the step's norm reads this conv output (fp32, own statistics pass)
            check_norm_layer(L, chk, lay, g, y, norm_st, code, gen)
    if d16 or w16:
        dy = torch.randn(B, Ho, Wo, Co, device="cuda", generator=gen)
        dyq = dy.to(T).float()
    if d16:
        # the deterministic plan runs the sub-pixel layers as the plain upsample + 5x5 (conv_fast16.hip dgrad16_t): its own rounding contract
        gx, _ = _ref16(xq[S], w, b, g, dt, dyq[S], up5_dgrad="plain" if det else "merged")
        nb = L.lib.aclgan_conv2d_dgrad16_scratch_bytes(C.byref(d_b))
        if det:       # one writer per position of the padded gradient grid, then the fold: the scratch holds that whole grid
            Hp, Wp = (Hi << up) + 2 * p, (Wi << up) + 2 * p
            assert nb >= 4 * B * Hp * Wp * Ci, (chk.wl, lay, "dgrad16 scratch", nb, 4 * B * Hp * Wp * Ci)

        def dgrad16(out, acc, fill_):
            L.check(L.lib.aclgan_conv2d_dgrad16(C.byref(d_b), code, L.ptr(dyq), L.ptr(w), L.ptr(w16t), L.ptr(out), acc, L.ptr(_scr(nb + 256, fill_)),
                                                L.stream_ptr()), "conv2d_dgrad16")
            return out
        dx = dgrad16(torch.full((B, Hi, Wi, Ci), NAN, device="cuda"), 0, fill)
        chk(lay, "dgrad16", dx[S], gx, TOL, rows=S)
        base = torch.randn(B, Hi, Wi, Ci, device="cuda", generator=gen) * float(gx.abs().max())
        acc = dgrad16(base.clone(), 1, fill)
        chk(lay, "dgrad16 accumulate", acc[S].double() - base[S].double(), gx, TOL, rows=S)
        if det:
            chk.equal(lay, "dgrad16 det rerun", dgrad16(torch.full((B, Hi, Wi, Ci), NAN, device="cuda"), 0, INF), dx)
            chk.equal(lay, "dgrad16 accumulate det rerun", dgrad16(base.clone(), 1, INF), acc)
        if L.lib.aclgan_conv16s_ok(C.byref(d_b), 1):
            dy16 = dy.to(T)
            snb = L.lib.aclgan_conv2d_dgrad16s_scratch_bytes(C.byref(d_b))

            def dgrad16s(out, st_, acc_, fill_):
                L.check(L.lib.aclgan_conv2d_dgrad16s(C.byref(d_b), code, L.ptr(dy16), L.ptr(w16t), L.ptr(out), st_, acc_, L.ptr(_scr(snb, fill_)),
                                                     L.stream_ptr()), "conv2d_dgrad16s")
                return out
            dx32 = dgrad16s(torch.full((B, Hi, Wi, Ci), NAN, device="cuda"), 0, 0, fill)
            chk(lay, "dgrad16s", dx32[S], gx, 2 * ULP[dt], rows=S)
            dx16 = dgrad16s(torch.full((B, Hi, Wi, Ci), NAN, device="cuda").to(T), code, 0, fill)
            chk.equal(lay, "dgrad16s 16-bit dx == fp32 rounded", dx16, dx32.to(T))
            b16 = base.to(T)
            acc16 = dgrad16s(b16.clone(), code, 1, fill)
            chk.equal(lay, "dgrad16s accumulate 16-bit", acc16, (b16.float() + dx32).to(T))
            acc32 = dgrad16s(base.clone(), 0, 1, fill)
            chk(lay, "dgrad16s accumulate fp32", acc32[S].double() - base[S].double(), dx32[S], 1e-5, rows=S)
            if det:
                chk.equal(lay, "dgrad16s det rerun", dgrad16s(torch.full((B, Hi, Wi, Ci), NAN, device="cuda"), 0, 0, INF), dx32)
                chk.equal(lay, "dgrad16s 16-bit det rerun", dgrad16s(torch.full((B, Hi, Wi, Ci), NAN, device="cuda").to(T), code, 0, INF), dx16)
    if w16:
        dy_st = code if s_bwd else 0
        dyw = dy.to(T) if dy_st else dy
        xw = x.to(T) if x_st else x
        _, gw = _ref16(xq, w, b, g, dt, dyq)
        gdb = (dyq if dy_st else dy).double().sum(dim=(0, 1, 2))
        wnb = L.lib.aclgan_conv2d_wgrad16_scratch_bytes(C.byref(d_b))

        def wgrad16(fill_):
            dw = torch.zeros(Co, k, k, Ci, device="cuda"); db = torch.zeros(Co, device="cuda")      # (the weight gradient accumulates)
            L.check(L.lib.aclgan_conv2d_wgrad16_st(C.byref(d_b), code, L.ptr(xw), x_st, L.ptr(dyw), dy_st, L.ptr(dw), L.ptr(db),
                                                   L.ptr(_scr(wnb, fill_)), L.stream_ptr()), "conv2d_wgrad16_st")
            return dw, db
        dw, db = wgrad16(fill)
        chk(lay, "wgrad16 dw (x %s, dy %s)" % ("16" if x_st else "32", "16" if dy_st else "32"), dw, gw, TOL, what="w")
        chk(lay, "wgrad16 db", db, gdb, TOL, what="")
        if det:
            dw2, db2 = wgrad16(INF)
            chk.equal(lay, "wgrad16 dw det rerun", dw2, dw)
            chk.equal(lay, "wgrad16 db det rerun", db2, db)


@pytest.mark.parametrize("wl,mode", _modes(["bf16_256_b8", "fp16_256_b32"]), indirect=["mode"])
def test_16bit_layers_at_launch_shape(L, wl, mode):
    t0 = time.time()
    dt = WL[wl][3]
    _, _, _, _, B = WL[wl]
    cfg, _ = recorded_layers(WL[wl][1], WL[wl][2])
    last = "dec.model.0.model.%d.model.1.conv" % (cfg["gen"]["n_res"] - 1)
    chk = Check(wl, mode)
    for i, (g, ent) in enumerate(launch_table(wl).items()):
        check_16bit_layer(L, chk, g, ent, dt, 300 + i, any(n.endswith(last) for n in ent["names"]))
    torch.cuda.synchronize()
    print("\n%s/%s: %d layers in %.1f s" % (wl, mode, len(launch_table(wl)), time.time() - t0))
    chk.done()


# ----------------------------------------------------------------------------------------------------------------------------------
# 6. the remaining operators at the step's sizes
# ----------------------------------------------------------------------------------------------------------------------------------
def _rel64(a, b):
    a = a.detach().double(); b = b.detach().double().to(a.device)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


@pytest.mark.parametrize("B,mode", _modes([3, 4, 8, 32]), indirect=["mode"])
def test_dense_layers_at_step_batches(L, B, mode):
    """the style MLP (8 -> 256 -> 256 -> 4096, one fused launch), its linear layers forward / backward, the style head (256 -> 8).  The input
    gradient of the 256 -> 4096 layer combines O-slices with fp32 atomics in the default plan (dense.hip linear_dx, O >= 512), one slice in
    the deterministic plan"""
    chk = Check("B=%d" % B, mode)
    gen = torch.Generator(device="cuda").manual_seed(B)
    S, M, Oo = 8, 256, 4096
    mk = lambda o, i: (torch.randn(o, i, device="cuda", generator=gen) * (2.0 / i) ** 0.5, torch.randn(o, device="cuda", generator=gen) * 0.1)  # noqa: E731
    (w0, b0), (w1, b1), (w2, b2) = mk(M, S), mk(M, M), mk(Oo, M)
    s = torch.randn(B, S, device="cuda", generator=gen)
    m0 = torch.empty(B, M, device="cuda"); m1 = torch.empty(B, M, device="cuda"); ap = torch.empty(B, Oo, device="cuda")
    L.check(L.lib.aclgan_mlp3_fwd(B, S, M, Oo, L.ptr(s), L.ptr(w0), L.ptr(b0), L.ptr(w1), L.ptr(b1), L.ptr(w2), L.ptr(b2), L.ptr(m0), L.ptr(m1),
                                  L.ptr(ap), L.stream_ptr()), "mlp3_fwd")
    r0 = F.relu(F.linear(s.double(), w0.double(), b0.double()))
    r1 = F.relu(F.linear(r0, w1.double(), b1.double()))
    chk("mlp", "mlp3_fwd", ap, F.linear(r1, w2.double(), b2.double()), TOL, what="")
    chk("mlp", "mlp3_fwd hidden", torch.cat([m0, m1], 1), torch.cat([r0, r1], 1), TOL, what="")
    for (I, Oo_, act) in ((S, M, "relu"), (M, M, "relu"), (M, Oo, "none"), (256, 8, "none")):
        x = torch.randn(B, I, device="cuda", generator=gen)
        w, b = mk(Oo_, I)
        y = torch.empty(B, Oo_, device="cuda")
        L.check(L.lib.aclgan_linear_fwd(B, I, Oo_, L.ptr(x), L.ptr(w), L.ptr(b), L.ACT[act], L.ptr(y), L.stream_ptr()), "linear_fwd")
        xr = x.double().requires_grad_(True); wr = w.double().requires_grad_(True); br = b.double().requires_grad_(True)
        yl = F.linear(xr, wr, br)
        chk("linear %dx%d" % (I, Oo_), "fwd", y, F.relu(yl) if act == "relu" else yl, TOL, what="")
        dy = torch.randn(B, Oo_, device="cuda", generator=gen)
        yl.backward(torch.where(y > 0, dy, 0.0).double() if act == "relu" else dy.double())     # (the kernel's own ReLU mask)
        dx = torch.full((B, I), float("nan"), device="cuda"); dw = torch.zeros_like(w); db = torch.zeros_like(b)
        L.check(L.lib.aclgan_linear_bwd(B, I, Oo_, L.ptr(x), L.ptr(y), L.ptr(dy.clone()), L.ptr(w), L.ACT[act], L.ptr(dx), L.ptr(dw), L.ptr(db),
                                        L.stream_ptr()), "linear_bwd")
        chk("linear %dx%d" % (I, Oo_), "bwd dx", dx, xr.grad, TOL, what="")
        chk("linear %dx%d" % (I, Oo_), "bwd dw", dw, wr.grad, TOL, what="")
        chk("linear %dx%d" % (I, Oo_), "bwd db", db, br.grad, TOL, what="")
        if mode == "det":
            dx2 = torch.full((B, I), float("nan"), device="cuda"); dw2 = torch.zeros_like(w); db2 = torch.zeros_like(b)
            L.check(L.lib.aclgan_linear_bwd(B, I, Oo_, L.ptr(x), L.ptr(y), L.ptr(dy.clone()), L.ptr(w), L.ACT[act], L.ptr(dx2), L.ptr(dw2),
                                            L.ptr(db2), L.stream_ptr()), "linear_bwd")
            chk.equal("linear %dx%d" % (I, Oo_), "bwd dx,dw,db det rerun", torch.cat([dx2.flatten(), dw2.flatten(), db2]),
                      torch.cat([dx.flatten(), dw.flatten(), db]))
    chk.done()


@pytest.mark.parametrize("wl", ["fp32_256_b8", "fp32_512_b4", "fp16_256_b32", "fp32_256_b3"])
def test_pooling_at_step_shapes(L, wl):
    """global average pool of the style encoder (256 channels on S/16, both batches) and the discriminators' 3x3 / 2 average pool
    between scales (3- and 6-channel images at the joint batches)"""
    _, _, S, _, B = WL[wl]
    chk = Check(wl)
    gen = torch.Generator(device="cuda").manual_seed(S + B)
    HW, Cn = (S // 16) ** 2, 256
    x = torch.randn(B, HW, Cn, device="cuda", generator=gen)
    y = torch.empty(B, Cn, device="cuda")
    L.check(L.lib.aclgan_gap_fwd(B, HW, Cn, L.ptr(x), L.ptr(y), L.stream_ptr()), "gap_fwd")
    chk("gap %dx%d" % (HW, Cn), "fwd", y, x.double().mean(1), TOL, what="")
    dy = torch.randn(B, Cn, device="cuda", generator=gen)
    dx = torch.randn(B, HW, Cn, device="cuda", generator=gen)
    base = dx.clone()
    L.check(L.lib.aclgan_gap_bwd(B, HW, Cn, L.ptr(dy), L.ptr(dx), 1, L.stream_ptr()), "gap_bwd")
    chk("gap %dx%d" % (HW, Cn), "bwd accumulate", dx.double() - base.double(), (dy.double() / HW).unsqueeze(1).expand(B, HW, Cn), TOL, what="")
    for m, Cc in ((1, 3), (2, 3), (3, 3), (2, 6)):
        for H in (S, S // 2):
            xi = torch.randn(m * B, Cc, H, H, device="cuda", generator=gen)
            xn = xi.permute(0, 2, 3, 1).contiguous()
            Ho = (H - 1) // 2 + 1
            yp = torch.empty(m * B, Ho, Ho, Cc, device="cuda")
            L.check(L.lib.aclgan_avgpool3s2_fwd(m * B, H, H, Cc, L.ptr(xn), L.ptr(yp), L.stream_ptr()), "avgpool3s2_fwd")
            xr = xi.double().requires_grad_(True)
            yr = O.avgpool3s2(xr)
            chk("avgpool %dx%dx%d B=%d" % (H, H, Cc, m * B), "fwd", yp, yr.permute(0, 2, 3, 1), TOL)
            g = torch.randn(yr.shape, device="cuda", generator=gen, dtype=torch.float64)
            yr.backward(g)
            dxp = torch.full_like(xn, float("nan"))
            L.check(L.lib.aclgan_avgpool3s2_bwd(m * B, H, H, Cc, L.ptr(g.float().permute(0, 2, 3, 1).contiguous()), L.ptr(dxp), 0, L.stream_ptr()), "avgpool3s2_bwd")
            chk("avgpool %dx%dx%d B=%d" % (H, H, Cc, m * B), "bwd", dxp, xr.grad.permute(0, 2, 3, 1), TOL)
    chk.done()


@pytest.mark.parametrize("wl,mode", _modes(["fp32_256_b8", "fp32_512_b4", "fp16_256_b32", "fp32_256_b3"]), indirect=["mode"])
def test_losses_at_full_pixel_counts(L, wl, mode):
    """the L1 identity loss, the focus size / digit losses and one multi-term LSGAN launch at the step's pixel counts (up to 32 x 256^2): the
    multi-block finishes take more partials here than at the operator tests' sizes (the L1 loss: one workgroup in the deterministic plan)"""
    _, _, S, _, B = WL[wl]
    chk = Check(wl, mode)
    gen = torch.Generator(device="cuda").manual_seed(7 * S + B)
    npix = B * S * S
    # L1 (x_recon - x): 4-channel decoder output against the 3-channel image
    a = torch.randn(npix, 4, device="cuda", generator=gen); bb = torch.randn(npix, 3, device="cuda", generator=gen)
    slot = torch.zeros(1, device="cuda"); d_a = torch.full((npix, 4), float("nan"), device="cuda")
    L.check(L.lib.aclgan_l1_loss(L.ptr(a), 4, L.ptr(bb), npix, L.ptr(slot), L.ptr(d_a), 1.5, 0, L.stream_ptr()), "l1_loss")
    diff = a[:, :3].double() - bb.double()
    chk("l1 %d px" % npix, "loss", slot, diff.abs().mean().view(1), 1e-5, what="")
    chk("l1 %d px" % npix, "grad", d_a[:, :3], 1.5 * torch.sign(torch.where(diff == 0, 1.0, diff)) / (3 * npix), TOL, what="")
    assert float(d_a[:, 3].abs().max()) == 0.0
    # focus losses
    dec = torch.tanh(torch.randn(npix, 4, device="cuda", generator=gen) * 0.5 + 0.1)
    hp = dict(focus_upper=0.5, focus_lower=0.3, focus_delta=0.001, focus_epsilon=0.01)
    decr = dec.double().requires_grad_(True)
    size, digit = O.focus_losses(decr[:, 3], hp)
    scale = 0.025 / npix / 3
    (scale * (size + digit)).backward()
    scr = _scr(L.lib.aclgan_focus_loss_scratch_bytes(npix), NAN if mode == "det" else None)
    slots = torch.zeros(2, device="cuda"); d_dec = torch.zeros(npix, 4, device="cuda")
    L.check(L.lib.aclgan_focus_loss(L.ptr(dec), npix, 0.001, 0.5, 0.3, 0.01, scale, L.ptr(slots), C.c_void_p(slots.data_ptr() + 4), L.ptr(d_dec),
                                    L.ptr(scr), L.stream_ptr()), "focus_loss")
    chk("focus %d px" % npix, "size", slots[:1], size.detach().view(1), 1e-4, what="")
    chk("focus %d px" % npix, "digit", slots[1:], digit.detach().view(1), 1e-5, what="")
    chk("focus %d px" % npix, "grad", d_dec[:, 3], decr.grad[:, 3], TOL, what="")
    # LSGAN over the three scales of a joint discriminator batch (3B samples, two segments of targets 0 / 1 like dis_update's dis_A)
    maps = [torch.randn(3 * B, (S >> (4 + j)) ** 2, device="cuda", generator=gen) for j in range(3)]
    segs = [(0.0, 0.5, B), (0.0, 0.5, B), (1.0, 1.0, B)]
    terms = [(m[i * B:(i + 1) * B].reshape(-1), t, wgt) for m in maps for i, (t, wgt, _) in enumerate(segs)]
    lslot = torch.zeros(len(terms), device="cuda")
    grads = [torch.full_like(t[0], float("nan")) for t in terms]
    arr = lambda v: (C.c_void_p * len(v))(*v)   # noqa: E731
    L.check(L.lib.aclgan_lsgan_loss_multi(arr([t[0].data_ptr() for t in terms]), (C.c_int * len(terms))(*[t[0].numel() for t in terms]),
                                          (C.c_float * len(terms))(*[t[1] for t in terms]), (C.c_float * len(terms))(*[t[2] for t in terms]),
                                          arr([lslot.data_ptr() + 4 * i for i in range(len(terms))]), arr([gg.data_ptr() for gg in grads]),
                                          (C.c_float * len(terms))(*([0.2] * len(terms))), len(terms), L.stream_ptr()), "lsgan_loss_multi")
    for i, (o, t, wgt) in enumerate(terms):
        od = o.double()
        chk("lsgan term %d (%d values)" % (i, o.numel()), "loss", lslot[i:i + 1], (wgt * ((od - t) ** 2).mean()).view(1), 1e-5, what="")
        chk("lsgan term %d (%d values)" % (i, o.numel()), "grad", grads[i], 0.2 * wgt * 2 * (od - t) / o.numel(), TOL, what="")
    chk.done()
