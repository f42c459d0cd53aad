"""Gradient norm per group: readout, clipping and the non-finite guard on the GPU -- gradnorm_part_kernel / gradnorm_finish_kernel of
csrc/gradnorm.hip and the clipped Adam kernels of csrc/optimizer.hip against the fp64 model of tests/gradclip_ref.py.

  (1) the norm stage alone (aclgan_grad_clip_flat) at the edges of its decomposition, aligned and from a pointer offset by one float:
      relative error against the fp64 norm of the same fp32 buffer <= 1e-5 (the bound of this project's other fixed-order sums), the
      same bits twice, coefficient and counters as the model says, non-finite values at the ends and in the ragged tail.
  (2) clipped Adam through a real context, both groups: fp32 path, loss-scaled path, GEN with a bound average; ten steps whose norms
      alternate between 0.25 and 4 times max_norm.  The bound is measured, not fixed: torch's fp32 CPU clip_grad_norm_ + Adam against the
      same fp64 run, the kernel at most 2x worse per metric.
  (3) max_norm = inf changes no bit (context level and trainer level) and adds exactly the documented launches.
  (4) skips: a NaN gradient leaves everything bit-unchanged, later updates follow the model with the reduced bias-correction step and not
      the un-reduced one; beside a loss scale all eight floats of its state follow LossScaleModel.
  (5) full width, once per group: every element of p, m, v after three clipped fp32 steps and three loss-scaled ones.
  (6) trainer: the published norms, the per-group keys, save / resume, key off, graph replay.

Hyper-parameters cross the ABI as C floats: every side is fed the float-rounded values."""
import ctypes as C
import json
import math
import os
import warnings
from contextlib import contextmanager
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from gpu_util import deterministic_mode
from oracle import aclgan_oracle as O
from oracle import optimizer_oracle as M
from gradclip_ref import ClipModel, clip_rule, index_values, norm_f32

pytestmark = pytest.mark.gpu

FULL = (3, 6, 64, 256, 8, 4, 2, 4, 64, 4, 3)
SMALL = (3, 6, 8, 16, 8, 4, 2, 1, 8, 4, 3)        # 226 536 / 393 372 floats
B1, B2, EPS, WD, LR0 = 0.5, M.f32(0.999), M.f32(1e-8), M.f32(1e-4), M.f32(1e-4)
INF = float("inf")
NORM_BOUND = 1e-5
# the norm kernel's decomposition (csrc/gradnorm.hip): 16-byte loads x 256 threads; 2048 workgroups; four loads per thread and trip
WG, GRID_PASS, TRIP = 4 * 256, 2048 * 4 * 256, 4 * 2048 * 4 * 256


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib
    assert _lib.lib.aclgan_grad_clip_state_floats() == 8 + 2048
    return _lib


@pytest.fixture(scope="module")
def T(L):
    from aclgan_amd import trainer
    return trainer


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _new_state(L):
    return torch.zeros(L.lib.aclgan_grad_clip_state_floats(), device="cuda")


def _flat(L, g, max_norm, state):
    L.check(L.lib.aclgan_grad_clip_flat(L.ptr(g), g.numel(), max_norm, L.ptr(state), L.stream_ptr()), "grad_clip_flat")
    return state[:8].cpu().tolist()


# ---------------------------------------------------------------- (1) the norm stage at its edges
NORM_SIZES = [1, 3, 4, 5, 255, 256, 257, WG - 1, WG, WG + 1, GRID_PASS - 1, GRID_PASS, GRID_PASS + 1, TRIP - 1, TRIP, TRIP + 1]


@pytest.fixture(scope="module")
def norm_buffer():
    """one buffer of index values (magnitudes 1e-6 .. 1, mixed signs) all sizes and both alignments are cut from, and its fp64 squares' prefix sums"""
    buf = index_values(TRIP + 8, 3, -6.0, 0.0, device="cuda").float()
    assert buf.data_ptr() % 16 == 0
    return buf


def test_norm_stage_at_the_edges_of_its_decomposition(L, norm_buffer):
    worst, rows = 0.0, []
    for off in (0, 1):
        for n in NORM_SIZES:
            g = norm_buffer[off:off + n]
            assert g.data_ptr() % 16 == 4 * off
            want = float(g.double().pow(2).sum().sqrt())
            st = _new_state(L)
            a = _flat(L, g, INF, st)
            bits = st[:8 + 2048].clone()
            b = _flat(L, g, INF, st)
            rel = abs(a[0] - want) / want
            rows.append((off, n, a[0], want, rel))
            worst = max(worst, rel)
            print("    offset %d n %8d: norm %.9g fp64 %.12g rel %.2e" % rows[-1])
            assert rel <= NORM_BOUND, rows[-1]
            assert a[1:] == [1.0, 0, 0, 0, 0, 0, 0] and b == a and same_bits(st, bits), (off, n, a, b)
            # max_norm below the norm, above it, inf: coefficient and counters on one state, as the model says
            st = _new_state(L)
            lo, hi = M.f32(want / 2), M.f32(want * 2)
            s1 = _flat(L, g, lo, st); s2 = _flat(L, g, hi, st); s3 = _flat(L, g, INF, st); s4 = _flat(L, g, lo, st)
            c = clip_rule(a[0], lo)
            assert 0.49 < c < 0.51 and abs(s1[1] - c) <= 2.0 ** -23 * c, (s1, c)
            assert s1[2:4] == [1.0, 0.0] and s2[1:4] == [1.0, 1.0, 0.0] and s3[1:4] == [1.0, 1.0, 0.0] and s4[1:4] == [s1[1], 2.0, 0.0]
            assert s1[0] == s2[0] == s3[0] == s4[0] == a[0] and s4[4:] == [0, 0, 0, 0]
    print("(1) worst relative error of the norm over %d cases: %.3e (bound %.0e)" % (len(rows), worst, NORM_BOUND))
    out = os.environ.get("ACLGAN_GRADCLIP_PARITY_OUT")
    if out:      # (scripts/bench_gradclip.py's companion figure: profiles/gradclip_parity.json)
        json.dump({"bound": NORM_BOUND, "worst_relative_error": worst,
                   "cases": [{"offset_floats": r[0], "n": r[1], "norm": r[2], "fp64": r[3], "rel": r[4]} for r in rows]}, open(out, "w"), indent=1)


@pytest.mark.parametrize("off", [0, 1])
def test_norm_stage_non_finite_values_at_the_ends_and_in_the_ragged_tail(L, norm_buffer, off):
    head = (4 - off) % 4                        # scalar elements before the first 16-byte boundary
    n = head + GRID_PASS + 3 * WG + 2           # ... a grid-stride remainder and a scalar tail of two elements
    tail0 = head + 4 * ((n - head) // 4)
    assert tail0 < n
    g = norm_buffer[off:off + n].clone() if off == 0 else norm_buffer.clone()[off:off + n]
    assert g.data_ptr() % 16 == 4 * off
    for pos in (0, n - 1, tail0, head, GRID_PASS + head):
        for val in (float("nan"), INF, -INF):
            keep = float(g[pos])
            g[pos] = val
            st = _new_state(L)
            s = _flat(L, g, 1.0, st)
            assert not math.isfinite(s[0]) and s[1:4] == [0.0, 0.0, 1.0], (pos, val, s)
            s = _flat(L, g, INF, st)
            assert not math.isfinite(s[0]) and s[1:4] == [0.0, 0.0, 2.0], (pos, val, s)
            g[pos] = keep
            s = _flat(L, g, INF, st)
            assert math.isfinite(s[0]) and s[1:4] == [1.0, 0.0, 2.0], (pos, val, s)
    # a finite value whose square is no fp32 number: the norm is inf, the update would be skipped
    g[tail0] = 3e38
    s = _flat(L, g, 1.0, _new_state(L))
    assert s[0] == INF and s[1:4] == [0.0, 0.0, 1.0]


# ---------------------------------------------------------------- contexts
class _Ctx:
    """a context with caller-owned p / g / m / v for both groups; optionally the loss-scale state, clip states and the average"""

    def __init__(self, L, arch):
        self.L = L
        self.ctx = C.c_void_p()
        L.check(L.lib.aclgan_ctx_create(C.byref(L.Arch(*arch)), C.byref(self.ctx)), "ctx_create")
        self.n = [L.lib.aclgan_group_numel(self.ctx, grp) for grp in (0, 1)]
        self.p, self.g, self.m, self.v = ([torch.zeros(n, device="cuda") for n in self.n] for _ in range(4))
        for grp in (0, 1):
            L.check(L.lib.aclgan_bind_params(self.ctx, grp, L.ptr(self.p[grp]), L.ptr(self.g[grp]), L.ptr(self.m[grp]), L.ptr(self.v[grp])), "bind_params")
        self.state, self.clip, self.ema = None, [None, None], None

    def bind_scale(self, values):
        L = self.L
        if values is None:
            self.state = None
            L.check(L.lib.aclgan_bind_loss_scale(self.ctx, None), "unbind_loss_scale")
            return
        if self.state is None:
            self.state = torch.zeros(8, device="cuda")
            L.check(L.lib.aclgan_bind_loss_scale(self.ctx, L.ptr(self.state)), "bind_loss_scale")
        self.state.copy_(torch.tensor(values, dtype=torch.float32))

    def bind_clip(self, grp, max_norm):
        L = self.L
        self.clip[grp] = None if max_norm is None else _new_state(L)
        L.check(L.lib.aclgan_bind_grad_clip(self.ctx, grp, max_norm or 0.0, None if max_norm is None else L.ptr(self.clip[grp])), "bind_grad_clip")

    def bind_ema(self, on=True):
        L = self.L
        self.ema = self.p[0].clone() if on else None
        L.check(L.lib.aclgan_bind_ema(self.ctx, 0, L.ptr(self.ema) if on else None), "bind_ema")

    def step(self, grp, lr, step, decay=0.5):
        L = self.L
        adam = L.Adam(lr, B1, B2, EPS, WD)
        if grp == 0 and self.ema is not None:
            L.check(L.lib.aclgan_adam_step_ema(self.ctx, grp, C.byref(adam), step, decay, L.EMA_BLEND, L.stream_ptr()), "adam_step_ema")
        else:
            L.check(L.lib.aclgan_adam_step(self.ctx, grp, C.byref(adam), step, L.stream_ptr()), "adam_step")

    def clip_list(self, grp):
        return self.clip[grp][:8].cpu().tolist()


@contextmanager
def _context(L, arch):
    c = _Ctx(L, arch)
    try:
        yield c
    finally:
        torch.cuda.synchronize()
        L.lib.aclgan_ctx_destroy(c.ctx)


def _sign(n, gen):
    return torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()


def _p0(n, gen):
    return (10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 4 - 3) * _sign(n, gen)).float()


def _check_clip_state(got, model, tag):
    want = model.state
    if math.isfinite(want[0]):
        assert abs(got[0] - model.norm64) <= NORM_BOUND * model.norm64, (tag, got, model.norm64)
        assert abs(got[1] - want[1]) <= 2 * NORM_BOUND * want[1], (tag, got, want)
    else:
        assert not math.isfinite(got[0]) and got[1] == 0.0, (tag, got, want)
    assert got[2:4] == want[2:4] and got[4:] == [0, 0, 0, 0], (tag, got, want)


# ---------------------------------------------------------------- (2) clipped Adam against the fp64 model
SEQ_T, MAX_NORM = 10, 0.5
PATHS = (("fp32", None, False), ("S=2^16", 2.0 ** 16, False), ("fp32+ema", None, True))


def _seq_grads(n, seed):
    gen = torch.Generator().manual_seed(seed)
    p0 = _p0(n, gen)
    grads = []
    for t in range(1, SEQ_T + 1):
        u = torch.randn(n, generator=gen, dtype=torch.float64)
        grads.append(((0.25 if t % 2 else 4.0) * MAX_NORM * u / u.norm()).float())
    return p0, grads


@pytest.fixture(scope="module")
def parity(L):
    """runs (2) once: the rows and, per metric, torch-fp32's largest error over the cases; 2x that is the bound (4) and (5) use too"""
    rows = []
    with _context(L, SMALL) as c:
        for grp, gname in ((0, "gen"), (1, "dis")):
            n = c.n[grp]
            p0, grads = _seq_grads(n, 50 + grp)
            model = ClipModel(p0, B1, B2, EPS, WD, MAX_NORM, ema=p0)
            t32 = M.TorchAdam32(p0, B1, B2, EPS, WD)
            for t in range(1, SEQ_T + 1):
                assert model.step(grads[t - 1], LR0, t, decay=0.5)
                # far from the edge of the clip decision on the fp64 side: a factor 4 from max_norm, either way
                r = model.norm64 / MAX_NORM
                assert abs(r - (0.25 if t % 2 else 4.0)) < 1e-5 * r, (t, r)
                t32.p.grad = grads[t - 1].clone()
                torch.nn.utils.clip_grad_norm_([t32.p], MAX_NORM)
                t32.opt.param_groups[0]["lr"] = LR0
                t32.opt.step()
            assert model.state[2] == SEQ_T // 2 and model.state[3] == 0
            err32 = M.parity_metrics(t32.p, t32.m, t32.v, model.adam, LR0, SEQ_T)
            for tag, S, ema in PATHS:
                if ema and grp != 0:
                    continue
                c.p[grp].copy_(p0); c.m[grp].zero_(); c.v[grp].zero_()
                c.bind_scale(None if S is None else [S, 1.0 / S, 0, 0, 0, 0, 1e6, 0])
                c.bind_clip(grp, MAX_NORM)
                if ema:
                    c.bind_ema()
                for t in range(1, SEQ_T + 1):
                    c.g[grp].copy_(grads[t - 1] if S is None else grads[t - 1] * S)      # S * g is exact: S is a power of two
                    c.step(grp, LR0, t)
                e = M.parity_metrics(c.p[grp].cpu(), c.m[grp].cpu(), c.v[grp].cpu(), model.adam, LR0, SEQ_T)
                for k in M.METRICS:
                    rows.append((gname, tag, k, e[k], err32[k]))
                _check_clip_state(c.clip_list(grp), model, (gname, tag))
                if S is not None:
                    assert c.state.cpu().tolist() == [S, 1.0 / S, float(SEQ_T), 0, 0, 0, 1e6, S]
                if ema:
                    e64 = model.ema
                    ea = ((c.ema.cpu().double() - e64).abs() / (LR0 * 1e-6 + SEQ_T * M.EPS32 * e64.abs())).max().item()
                    rows.append((gname, tag, "ema", ea, err32["p"] + 2.0))
                    c.bind_ema(False)
                c.bind_clip(grp, None); c.bind_scale(None)
    bound = {k: 2 * max(r[4] for r in rows if r[2] == k) for k in M.METRICS}
    return SimpleNamespace(rows=rows, bound=bound)


def test_clipped_adam_ten_steps_within_twice_torch_fp32_error_of_the_fp64_model(parity):
    """the average: it is the blend of the p's, so p's error plus the blend's own two roundings per step (the fmaf and (1 - d) * p), in
    units of the p metric's denominator: bound err32[p] + 2, doubled like the others"""
    print("\n(2) %d steps, norms alternating 0.25 / 4 x max_norm %.2f; errors against the fp64 model" % (SEQ_T, MAX_NORM))
    print("  group path      metric      HIP          torch-fp32   ratio")
    bad = []
    for gname, tag, k, hip, ref in parity.rows:
        print("    %-3s %-9s %-6s %12.4e %12.4e %7.3f" % (gname, tag, k, hip, ref, hip / ref))
        assert ref > 0
        if not hip <= 2 * ref:
            bad.append((gname, tag, k, hip, ref))
    assert not bad, bad
    assert len(parity.rows) == 5 * 4 + 1


def _assert_under_bound(tag, p, m, v, ref, lr, T, bound):
    e = M.parity_metrics(p, m, v, ref, lr, T)
    print("    %s: " % tag + ", ".join("%s %.3e (bound %.3e)" % (k, e[k], bound[k]) for k in M.METRICS))
    bad = {k: (e[k], bound[k]) for k in M.METRICS if not e[k] <= bound[k]}
    assert not bad, (tag, bad)


class _Yardstick:
    """torch's fp32 CPU clip_grad_norm_ + Adam over the APPLIED updates of a sequence (torch counts its own steps, so its bias-correction
    step is the reduced one): what fp32 arithmetic costs against the fp64 model on these very inputs.  The `m` metric divides by the
    largest |g| an element has seen, which after one or two updates can be far below weight_decay * |p|: the bound of (2) does not carry
    over to other gradients, so (4) takes 2x torch's error on its own inputs where that is larger."""

    def __init__(self, p0, max_norm):
        self.t, self.max_norm = M.TorchAdam32(p0, B1, B2, EPS, WD), max_norm
        self.applied = 0

    def step(self, g_true, lr):
        self.t.p.grad = g_true.float().cpu().clone()
        if math.isfinite(self.max_norm):
            torch.nn.utils.clip_grad_norm_([self.t.p], self.max_norm)
        self.t.opt.param_groups[0]["lr"] = lr
        self.t.opt.step()
        self.applied += 1

    def bound(self, ref, lr, floor):
        e = M.parity_metrics(self.t.p, self.t.m, self.t.v, ref, lr, self.applied)
        return {k: max(floor[k], 2 * e[k]) for k in M.METRICS}


# ---------------------------------------------------------------- (3) monitor mode changes no bit
@pytest.mark.parametrize("scaled", [False, True], ids=["fp32", "scaled"])
def test_monitor_mode_is_bit_identical_to_a_twin_context_without_a_state(L, scaled):
    S = 2.0 ** 16
    with _context(L, SMALL) as a, _context(L, SMALL) as b:
        gen = torch.Generator().manual_seed(60)
        counts = {}
        for c in (a, b):
            if scaled:
                c.bind_scale([S, 1.0 / S, 0, 0, 0, 0, 0, 0])
        for grp in (0, 1):
            p0 = _p0(a.n[grp], gen)
            for c in (a, b):
                c.p[grp].copy_(p0)
            a.bind_clip(grp, INF)
        for c in (a, b):
            c.bind_ema()
        for t in range(1, 4):
            for grp in (0, 1):
                g = (10.0 ** (torch.rand(a.n[grp], generator=gen, dtype=torch.float64) * 6 - 6) * _sign(a.n[grp], gen)).float()
                for c in (a, b):
                    c.g[grp].copy_(g * S if scaled else g)
                    n0 = L.lib.aclgan_launch_count()
                    c.step(grp, LR0, t)
                    counts[c is a] = L.lib.aclgan_launch_count() - n0
                assert counts[True] - counts[False] == (1 if scaled else 2) and counts[False] == (3 if scaled else 1), counts
                for name in "pmv":
                    assert same_bits(getattr(a, name)[grp], getattr(b, name)[grp]), (t, grp, name)
            assert same_bits(a.ema, b.ema) and not same_bits(a.ema, a.p[0])
        for grp in (0, 1):
            st = a.clip_list(grp)
            assert math.isfinite(st[0]) and st[0] > 0 and st[1:] == [1.0, 0, 0, 0, 0, 0, 0]
        if scaled:
            assert same_bits(a.state, b.state)


@pytest.fixture(scope="module")
def fix():
    meta = json.load(open(os.path.join(GOLDEN, "step_reduced_64.json")))
    data = np.load(os.path.join(GOLDEN, "step_reduced_64.npz"))
    cfg = meta["config"]
    x_a, x_b = torch.from_numpy(data["x_a"]), torch.from_numpy(data["x_b"])
    z = [torch.from_numpy(data["z%d" % i]) for i in range(6)]
    assert tuple(x_a.shape) == (2, 3, 64, 64)
    return cfg, O.test_nets(cfg, 0), x_a, x_b, z


def _make(T, fix, dtype="fp32", hip_graph=None, **keys):
    cfg, nets = dict(fix[0], **keys), fix[1]
    tr = T.aclgan_Trainer(cfg, compute_dtype=dtype, deterministic=True, hip_graph=hip_graph)
    for name in O.OracleTrainer.NETS:
        getattr(tr, name).load_state_dict(nets[name], strict=False)
    return tr, cfg


def _iteration(tr, cfg, fix):
    _, _, x_a, x_b, z = fix
    tr.dis_update(x_a, x_b, cfg, z=z[:3])
    tr.gen_update(x_a, x_b, cfg, z=z[3:])


def _same_training_state(a, b, tag):
    for grp in (0, 1):
        for name in ("_param", "_m", "_v"):
            assert same_bits(getattr(a, name)[grp], getattr(b, name)[grp]), (tag, grp, name)


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_trainer_monitor_mode_changes_no_bit_and_adds_the_documented_launches(L, T, fix, dtype):
    with deterministic_mode(L, True):
        on, c_on = _make(T, fix, dtype, grad_clip=INF)
        off, c_off = _make(T, fix, dtype)
        # key off: nothing of the feature exists
        assert off._clip == [None, None] and off.grad_clip == (0.0, 0.0) and off.grad_clip_state() == {"gen": None, "dis": None}
        assert off.grad_norm_gen is off.loss_dis_total and off.grad_norm_dis is off.loss_dis_total
        launches = {}
        for it in range(3):
            for tr, cfg in ((on, c_on), (off, c_off)):
                n0 = L.lib.aclgan_launch_count()
                _iteration(tr, cfg, fix)
                launches[tr is on] = L.lib.aclgan_launch_count() - n0
            torch.cuda.synchronize()
            assert same_bits(on._losses, off._losses), it
            _same_training_state(on, off, it)
            # two Adam calls per iteration: part + finish more each without a loss scale, one more each under it (the part kernel replaces the scan)
            # (from the second iteration on: the first trainer to run also makes the library's one-time launches)
            assert it == 0 or launches[True] - launches[False] == (2 if dtype == "fp16" else 4), (it, launches)
        st = on.grad_clip_state()
        for k in ("gen", "dis"):
            assert st[k]["norm"] > 0 and math.isfinite(st[k]["norm"]) and (st[k]["coef"], st[k]["clipped"], st[k]["skipped"]) == (1.0, 0, 0)
        assert float(off.grad_norm_gen) == 0.0 and float(on.grad_norm_gen) == st["gen"]["norm"] and float(on.grad_norm_dis) == st["dis"]["norm"]
        assert on.grad_norm_gen.dim() == 0 and on.grad_norm_gen.data_ptr() != on._clip[0].data_ptr()
        assert " gnorm_G=" in on.grad_clip_log_text() and on.grad_clip_log_text().endswith(" skipped=0")


# ---------------------------------------------------------------- (4) skips
def test_a_nan_gradient_skips_and_later_updates_use_the_reduced_bias_correction_step(L, parity):
    with _context(L, SMALL) as c:
        gen = torch.Generator().manual_seed(61)
        c.bind_ema()
        for grp in (0, 1):
            n = c.n[grp]
            p0 = _p0(n, gen)
            c.p[grp].copy_(p0); c.m[grp].zero_(); c.v[grp].zero_()
            if grp == 0:
                c.ema.copy_(p0)
            c.bind_clip(grp, INF)
            good = ClipModel(p0, B1, B2, EPS, WD, INF, ema=p0)
            wrong = ClipModel(p0, B1, B2, EPS, WD, INF, count_skips=False)
            yard = _Yardstick(p0, INF)
            for t in range(1, 5):
                g = (10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 6 - 6) * _sign(n, gen)).float()
                if t == 1:
                    g[(0, n - 1)[grp]] = float("nan")
                c.g[grp].copy_(g)
                before = [x.clone() for x in (c.p[grp], c.m[grp], c.v[grp], c.ema)]
                c.step(grp, LR0, t)
                applied = good.step(g, LR0, t, decay=0.5)
                assert wrong.step(g, LR0, t) == applied == (t > 1)
                st = c.clip_list(grp)
                _check_clip_state(st, good, (grp, t))
                if not applied:
                    assert all(same_bits(x, y) for x, y in zip((c.p[grp], c.m[grp], c.v[grp], c.ema), before)) and st[3] == 1.0 and math.isnan(st[0])
                    continue
                assert good.bias_correction_step(t) == t - 1 and wrong.bias_correction_step(t) == t
                yard.step(g, LR0)
                bound = yard.bound(good.adam, LR0, parity.bound)
                _assert_under_bound("group %d host step %d" % (grp, t), c.p[grp], c.m[grp], c.v[grp], good.adam, LR0, t - 1, bound)
                if t == 2:      # the check can fail: the model with the un-reduced step is further away than the bound
                    apart = M.parity_metrics(wrong.adam.p, wrong.adam.m, wrong.adam.v, good.adam, LR0, 1)["p"]
                    mine = M.parity_metrics(c.p[grp], c.m[grp], c.v[grp], wrong.adam, LR0, 1)["p"]
                    print("    host step 2: un-reduced model vs reduced %.3e, kernel vs un-reduced %.3e (bound %.3e)" % (apart, mine, bound["p"]))
                    assert apart > bound["p"] and mine > bound["p"]
            if grp == 0:
                ea = ((c.ema.double().cpu() - good.ema).abs() / (LR0 * 1e-6 + 3 * M.EPS32 * good.ema.abs())).max().item()
                assert ea <= parity.bound["p"] + 4.0, ea


def test_beside_a_loss_scale_its_eight_floats_follow_the_model_and_overflows_leave_the_clip_counters(L, parity):
    events = ["clean", "+inf", "clean", "huge", "clean", "nan", "clipped", "-inf", "clean", "clean"]
    with _context(L, SMALL) as c:
        gen = torch.Generator().manual_seed(62)
        for grp in (0, 1):
            n = c.n[grp]
            p0 = _p0(n, gen)
            c.p[grp].copy_(p0); c.m[grp].zero_(); c.v[grp].zero_()
            ls = M.LossScaleModel(16.0, interval=3)
            c.bind_scale(ls.state)
            max_norm = 1.0
            c.bind_clip(grp, max_norm)
            model = ClipModel(p0, B1, B2, EPS, WD, max_norm, group=grp, loss_scale=ls)
            yard = _Yardstick(p0, max_norm)
            applied_n = 0
            for i, ev in enumerate(events):
                S = ls.state[0]
                u = torch.randn(n, generator=gen, dtype=torch.float64)
                g = ((4.0 if ev == "clipped" else 0.25) * max_norm * u / u.norm()).float() * S
                if ev in ("+inf", "-inf", "nan"):
                    g[(0, n - 1, n // 2)[i % 3]] = float(ev)
                elif ev == "huge":
                    g[n // 3] = 3e38        # finite: no overflow; (3e38 / S)^2 is no fp32 number: a clip-skip
                c.g[grp].copy_(g)
                before = [x.clone() for x in (c.p[grp], c.m[grp], c.v[grp])]
                clip_before = c.clip_list(grp)
                c.step(grp, LR0, i + 1)
                applied = model.step(g, LR0, i + 1)
                assert c.state.cpu().tolist() == ls.state, (grp, i, ev, c.state.cpu().tolist(), ls.state)
                st = c.clip_list(grp)
                _check_clip_state(st, model, (grp, i, ev))
                assert applied == (ev in ("clean", "clipped"))
                if applied:
                    applied_n += 1
                    assert model.bias_correction_step(i + 1) == applied_n
                    yard.step(g.double() / S, LR0)      # (exact: S is a power of two)
                    _assert_under_bound("group %d call %d (%s)" % (grp, i, ev), c.p[grp], c.m[grp], c.v[grp], model.adam, LR0, applied_n,
                                        yard.bound(model.adam, LR0, parity.bound))
                else:
                    assert all(same_bits(x, y) for x, y in zip((c.p[grp], c.m[grp], c.v[grp]), before)), (grp, i, ev)
                    if ev != "huge":
                        assert st[2:4] == clip_before[2:4]
                    else:
                        assert st[3] == clip_before[3] + 1 and ls.state[4 + grp] == model.ls.state[4 + grp]
            assert ls.state[4 + grp] == 3 and model.state[2:4] == [1.0, 1.0] and applied_n == 6
            c.bind_clip(grp, None); c.bind_scale(None)


# ---------------------------------------------------------------- (5) full width, once per group
@pytest.mark.parametrize("grp,gname", ((0, "gen"), (1, "dis")), ids=["gen", "dis"])
def test_full_width_every_element_three_clipped_fp32_and_three_clipped_scaled_steps(L, parity, grp, gname):
    other, S = 1 - grp, 2.0 ** 16
    with _context(L, FULL) as c:
        n = c.n[grp]
        assert n > TRIP and n % TRIP != 0 and n > 16384 * 256       # several trips of the norm kernel's grid and a ragged last one
        p0 = index_values(n, 1, -3, 1, device="cuda").float()
        c.p[grp].copy_(p0)
        for buf in (c.p, c.g, c.m, c.v):
            buf[other].uniform_(-1, 1)
        keep = [buf[other].clone() for buf in (c.p, c.g, c.m, c.v)]
        g1 = index_values(n, 101, -6, 0, device="cuda").float()
        max_norm = M.f32(0.25 * norm_f32(g1)[1])
        c.bind_clip(grp, max_norm)
        model = ClipModel(p0, B1, B2, EPS, WD, max_norm, group=grp)       # fp64 on the GPU: independent of the kernels under test
        for t in range(1, 7):
            if t == 4:
                model.ls = M.LossScaleModel(S)
                c.bind_scale(model.ls.state)
            g = g1 if t == 1 else index_values(n, 100 + t, -6, 0, device="cuda").float()
            buf = g if t < 4 else g * S
            c.g[grp].copy_(buf)
            c.step(grp, LR0, t)
            assert model.step(buf, LR0, t)
            assert 3.9 < model.norm64 / max_norm < 4.1               # clipped, far from the edge
            _check_clip_state(c.clip_list(grp), model, (gname, t))
            if t in (3, 6):
                _assert_under_bound("%s after step %d" % (gname, t), c.p[grp], c.m[grp], c.v[grp], model.adam, LR0, t, parity.bound)
        assert c.clip_list(grp)[2:4] == [6.0, 0.0]
        assert c.state.cpu().tolist() == [S, 1.0 / S, 3.0, 0, 0, 0, 0, S]
        for name, buf, k in zip("pgmv", (c.p, c.g, c.m, c.v), keep):
            assert torch.equal(buf[other], k), "the other group's %s buffer changed" % name
        assert int((c.v[grp] == 0).sum()) == 0


# ---------------------------------------------------------------- (6) trainer
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_trainer_publishes_the_norm_of_its_gradient_buffers_in_true_gradient_units(L, T, fix, dtype):
    with deterministic_mode(L, True):
        tr, cfg = _make(T, fix, dtype, grad_clip=INF)
        _, _, x_a, x_b, z = fix
        for which, grp in (("dis", 1), ("gen", 0)):
            getattr(tr, which + "_update")(x_a, x_b, cfg, z=z[:3] if which == "dis" else z[3:])
            torch.cuda.synchronize()
            want = float(tr._grad[grp].double().pow(2).sum().sqrt()) / tr.grad_scale(which)
            got = float(getattr(tr, "grad_norm_" + which))
            print("    %s %s: grad_norm %.9g, fp64 %.12g (scale %g)" % (dtype, which, got, want, tr.grad_scale(which)))
            assert want > 0 and abs(got - want) <= NORM_BOUND * want
        assert dtype != "fp16" or tr.loss_scale_state()["skipped_gen"] + tr.loss_scale_state()["skipped_dis"] == 0


def test_trainer_per_group_keys(L, T, fix):
    with deterministic_mode(L, True):
        tr, cfg = _make(T, fix, grad_clip=INF, grad_clip_gen=0)
        assert tr.grad_clip == (0.0, INF) and tr._clip[0] is None and tr._clip[1] is not None
        _iteration(tr, cfg, fix)
        st = tr.grad_clip_state()
        assert st["gen"] is None and st["dis"]["norm"] > 0 and st["dis"]["coef"] == 1.0
        assert float(tr.grad_norm_gen) == 0.0 and float(tr.grad_norm_dis) == st["dis"]["norm"]
        # a bound on the generators only, a quarter of the norm just seen on the same batch: that update is clipped
        probe, c0 = _make(T, fix, grad_clip=INF)
        _iteration(probe, c0, fix)
        bound = 0.25 * probe.grad_clip_state()["gen"]["norm"]
        tr2, cfg2 = _make(T, fix, grad_clip_gen=bound)
        assert tr2._clip[1] is None
        _iteration(tr2, cfg2, fix)
        st = tr2.grad_clip_state()
        assert st["dis"] is None and st["gen"]["clipped"] == 1 and 0.24 < st["gen"]["coef"] < 0.26
        assert same_bits(tr2._param[1], probe._param[1]) and not same_bits(tr2._param[0], probe._param[0])


def test_trainer_save_resume_restores_the_states_and_training_continues_bit_identically(L, T, fix, tmp_path):
    with deterministic_mode(L, True):
        keys = dict(grad_clip=1e-3)                       # far below every norm of this run: every update is clipped
        tr, cfg = _make(T, fix, **keys)
        twin, _ = _make(T, fix, **keys)
        off, c_off = _make(T, fix)
        for _ in range(2):
            for t_ in (tr, twin):
                _iteration(t_, cfg, fix)
            _iteration(off, c_off, fix)
        for t_ in (tr, twin):                             # one update of each group counted as skipped: part of the bias-correction step
            for grp in (0, 1):
                t_._clip[grp][3] = 1.0
        d_on, d_off = tmp_path / "on", tmp_path / "off"
        d_on.mkdir(); d_off.mkdir()
        tr.save(str(d_on), 1); off.save(str(d_off), 1)
        assert sorted(os.listdir(d_on)) == sorted(os.listdir(d_off)) == ["dis_00000002.pt", "gen_00000002.pt", "optimizer.pt"]
        sd, sd_off = torch.load(str(d_on / "optimizer.pt")), torch.load(str(d_off / "optimizer.pt"))
        assert list(sd_off.keys()) == ["gen", "dis"] and list(sd.keys()) == ["gen", "dis", "aclgan_grad_clip_state"]
        saved = sd["aclgan_grad_clip_state"]
        assert saved.shape == (2, 8) and saved.dtype == torch.float32
        for grp in (0, 1):
            assert same_bits(saved[grp], tr._clip[grp][:8].cpu()) and saved[grp].tolist()[1:4] != [0, 0, 0] and saved[grp][2] == 2 and saved[grp][3] == 1
        fresh = T.aclgan_Trainer(cfg, deterministic=True)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            assert fresh.resume(str(d_on), cfg) == 2
        for grp in (0, 1):
            assert same_bits(fresh._clip[grp][:8], tr._clip[grp][:8])
        for t_ in (fresh, twin):
            t_._sched_calls = 2
            _iteration(t_, cfg, fix)
        torch.cuda.synchronize()
        _same_training_state(fresh, twin, "after resume")
        assert fresh.grad_clip_state() == twin.grad_clip_state() and fresh.grad_clip_state()["gen"]["clipped"] == 3
        # the skipped count matters: the same continuation without it ends elsewhere
        other = T.aclgan_Trainer(cfg, deterministic=True)
        other.resume(str(d_on), cfg)
        other._clip[0][3] = 0.0
        other._sched_calls = 2
        _iteration(other, cfg, fix)
        assert not same_bits(other._param[0], twin._param[0])
        # a checkpoint written with the key off: a warning, the counters start at 0
        cold = T.aclgan_Trainer(cfg, deterministic=True)
        with pytest.warns(UserWarning, match="aclgan_grad_clip_state"):
            assert cold.resume(str(d_off), cfg) == 2
        assert all(float(t.abs().sum()) == 0.0 for t in cold._clip)
        # and a trainer with the key off resumes a checkpoint that has the extra key silently
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            off2 = T.aclgan_Trainer(c_off, deterministic=True)
            assert off2.resume(str(d_on), c_off) == 2 and off2._clip == [None, None]


def test_trainer_graph_replay_gives_the_bits_of_eager(L, T):
    """hip_graph=True: step 1 runs eagerly, step 2 captures, steps 3 and 4 replay (the setting of tests/test_gpu_graph.py at reduced width, a
    fresh batch per step); Adam, and with it the norm stage, is enqueued eagerly after every replay.  Every parameter, Adam buffer and
    the clip states equal the eager trainer's bit for bit.  The bound is far below every norm of the run: every update is clipped."""
    cfg = O.default_config()
    cfg["gen"].update(dim=16, mlp_dim=32, n_res=2)
    cfg["dis"].update(dim=16)
    cfg.update(display_size=1, focus_epsilon=0.5, grad_clip=1e-3)
    nets = O.test_nets(cfg, 0)
    g = torch.Generator().manual_seed(31)
    batches = [(torch.rand(2, 3, 64, 64, generator=g) * 2 - 1, torch.rand(2, 3, 64, 64, generator=g) * 2 - 1,
                [torch.randn(2, 8, 1, 1, generator=g) for _ in range(6)]) for _ in range(4)]

    def run(**kw):
        tr = T.aclgan_Trainer(cfg, deterministic=True, **kw)
        for name in O.OracleTrainer.NETS:
            getattr(tr, name).load_state_dict(nets[name], strict=False)
        states = []
        for x_a, x_b, z in batches:
            tr.dis_update(x_a, x_b, cfg, z=z[:3])
            tr.gen_update(x_a, x_b, cfg, z=z[3:])
            tr.update_learning_rate()
            states.append(tr.grad_clip_state())
        torch.cuda.synchronize()
        return tr, states

    with deterministic_mode(L, True):
        eager, se = run()
        graph, sg = run(hip_graph=True)
    assert graph.hip_graph, "capture fell back to eager execution"
    assert graph._graphs["gen"]["graph"] is not None and graph._graphs["dis"]["graph"] is not None
    assert se == sg, (se, sg)
    _same_training_state(eager, graph, "graph")
    assert se[-1]["gen"]["clipped"] == 4 and se[-1]["dis"]["clipped"] == 4 and se[-1]["gen"]["skipped"] == 0
