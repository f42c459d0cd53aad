"""aclgan_adam_step -- adam_kernel (plain and SCALED), grad_check_kernel and scale_update_kernel of csrc/optimizer.hip -- against the fp64
optimizer model of oracle/optimizer_oracle.py (itself checked on the CPU by tests/test_optimizer_oracle_cpu.py).

Everything goes through the C ABI with a real context: aclgan_ctx_create, aclgan_bind_params for both groups and, for the fp16 path,
aclgan_bind_loss_scale.  No workspace, no update: the caller owns the gradient buffer, so the tests write the gradients themselves.

  (a) numerics over 40 steps, both groups, fp32 path and loss-scaled path (S = 1, 2^16, 2^24): p, m and v against the fp64 model at
      three steps.  The bound is not fixed in advance: torch's own fp32 CPU torch.optim.Adam (what the reference runs) is measured
      against the same fp64 run with the same metrics, and the kernel may be at most 2x worse in each.
  (b) every element of the full-width groups (30 058 648 / 24 822 756 floats: 8 / 6 passes of the 16384 x 256 grid-stride loop with
      a ragged last one): values are functions of the index, three fp32-mode steps and three loss-scaled ones, all of p, m, v against
      fp64 (torch on the GPU), the other group's buffers bit-unchanged.
  (c) the non-finite scan at full size: one +inf / -inf / nan at the edges of the buffer, of the passes and of a tensor must skip the
      update; a finite 3e38 must not.
  (d) the loss-scale state machine over an interleaved gen / dis sequence: all eight floats equal LossScaleModel after every call,
      and p, m, v follow the fp64 model run with bias-correction step = number of APPLIED updates.
  (e) trainer level: growth, the scale the next update's buffers carry, what save() writes.

Hyper-parameters cross the ABI as C floats: every side (kernel, fp64 model, torch fp32) is fed the float-rounded values."""
import ctypes as C
import math
import time
from contextlib import contextmanager
from types import SimpleNamespace

import pytest
import torch

from oracle import aclgan_oracle as O
from oracle import optimizer_oracle as M

pytestmark = pytest.mark.gpu

FULL = (3, 6, 64, 256, 8, 4, 2, 4, 64, 4, 3)      # the default architecture (tests/test_abi_cpu.py)
SMALL = (3, 6, 8, 16, 8, 4, 2, 1, 8, 4, 3)        # reduced width: 226 536 / 393 372 floats
B1, B2, EPS, WD, LR0 = 0.5, M.f32(0.999), M.f32(1e-8), M.f32(1e-4), M.f32(1e-4)
PASS = 16384 * 256                                # elements one pass of the capped grid covers
GROUPS = ((0, "gen"), (1, "dis"))


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib
    t0 = time.time()
    yield _lib
    print("\ntests/test_gpu_optimizer.py wall time: %.1f s" % (time.time() - t0))


class _Ctx:
    """a context with caller-owned p / g / m / v for both groups (and optionally the loss-scale state) bound"""

    def __init__(self, L, arch):
        self.L = L
        self.ctx = C.c_void_p()
        L.check(L.lib.aclgan_ctx_create(C.byref(L.Arch(*arch)), C.byref(self.ctx)), "ctx_create")
        self.n = [L.lib.aclgan_group_numel(self.ctx, grp) for grp in (0, 1)]
        self.p, self.g, self.m, self.v = ([torch.zeros(n, device="cuda") for n in self.n] for _ in range(4))
        for grp in (0, 1):
            L.check(L.lib.aclgan_bind_params(self.ctx, grp, L.ptr(self.p[grp]), L.ptr(self.g[grp]), L.ptr(self.m[grp]), L.ptr(self.v[grp])), "bind_params")
        self.state = None

    def bind_state(self, values):
        L = self.L
        if values is None:
            self.state = None
            L.check(L.lib.aclgan_bind_loss_scale(self.ctx, None), "unbind_loss_scale")
            return
        if self.state is None:
            self.state = torch.zeros(8, device="cuda")
            L.check(L.lib.aclgan_bind_loss_scale(self.ctx, L.ptr(self.state)), "bind_loss_scale")
        self.state.copy_(torch.tensor(values, dtype=torch.float32))

    def state_list(self):
        return self.state.cpu().tolist()

    def step(self, grp, lr, step):
        L = self.L
        adam = L.Adam(lr, B1, B2, EPS, WD)
        L.check(L.lib.aclgan_adam_step(self.ctx, grp, C.byref(adam), step, L.stream_ptr()), "adam_step")

    def tensor_span(self, grp, index):
        L = self.L
        name = C.create_string_buffer(256); off = C.c_int64(); shp = (C.c_int * 4)(); nd = C.c_int()
        L.check(L.lib.aclgan_tensor_info(self.ctx, grp, index, name, 256, C.byref(off), shp, C.byref(nd)), "tensor_info")
        numel = 1
        for j in range(nd.value):
            numel *= shp[j]
        return name.value.decode(), off.value, numel


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


def _snapshot(a):
    return SimpleNamespace(p=a.p.clone(), m=a.m.clone(), v=a.v.clone(), gmax=a.gmax.clone(), gvmax=a.gvmax.clone())


# ---------------------------------------------------------------- (a) numerics over a long sequence
SEQ_T = 40
SEQ_CHECK = (7, 24, 40)
SEQ_LR_STEP = 20            # StepLR: lr halves after 20 scheduler calls, i.e. from step 21 on


def _seq_lr(t):             # lr of the t-th (1-based) update when the scheduler is stepped once after every update
    return M.f32(O.step_lr(LR0, 0.5, SEQ_LR_STEP, t - 1))


def _sequence_inputs(n, seed):
    """p0 over 1e-3 .. 1e1 and per-element gradient magnitudes over 1e-8 .. 1e2 (log-uniform, random signs; every step draws a factor
    in +-[0.25, 1]).  weight_decay * p spans 1e-7 .. 1e-3, so both `weight_decay * p >> g` and `g >> weight_decay * p` occur in bulk.
    sqrt(v) < eps needs |g + weight_decay * p| < 1e-8, which independent draws almost never give: every 16th element therefore has
    |p0| in [1, 1.5]e-3 and gradients -weight_decay * p0 * (1 - 0.06 u) (magnitude ~1e-7, inside the band), which leaves an effective
    gradient of ~6e-9 u.  (0.06, not less: the cancellation then costs fp32 about 1e-6 relative, the size of its other errors.)"""
    gen = torch.Generator().manual_seed(seed)
    p0 = (10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 4 - 3) * _sign(n, gen))
    mag = 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 10 - 8)
    idx = torch.arange(0, n, 16)
    p0[idx] = 1e-3 * (1 + 0.5 * torch.rand(idx.numel(), generator=gen, dtype=torch.float64)) * _sign(idx.numel(), gen)
    p0 = p0.float()
    grads = []
    for _ in range(SEQ_T):
        u = (0.25 + 0.75 * torch.rand(n, generator=gen, dtype=torch.float64)) * _sign(n, gen)
        g = mag * u
        g[idx] = -WD * p0[idx].double() * (1 - 0.06 * u[idx])
        grads.append(g.float())
    return p0, grads


@pytest.fixture(scope="module")
def parity(L):
    """runs (a) once; the rows and, per metric, torch-fp32's largest error over the cases: 2x that is the bound (b), (c), (d) use"""
    rows, regimes = [], []
    with _context(L, SMALL) as c:
        for grp, gname in GROUPS:
            n = c.n[grp]
            p0, grads = _sequence_inputs(n, 40 + grp)
            a64 = M.Adam64(p0, B1, B2, EPS, WD)
            t32 = M.TorchAdam32(p0, B1, B2, EPS, WD)
            ref, err32 = {}, {}
            for t in range(1, SEQ_T + 1):
                a64.step(grads[t - 1], _seq_lr(t)); t32.step(grads[t - 1], _seq_lr(t))
                if t in SEQ_CHECK:
                    ref[t] = _snapshot(a64)
                    err32[t] = M.parity_metrics(t32.p, t32.m, t32.v, ref[t], _seq_lr(t), t)
                    vhat = (ref[t].v / (1 - B2 ** t)).sqrt()
                    gl = grads[t - 1].double().abs(); wl = WD * ref[t].p.abs()
                    regimes.append((gname, t, n, int((vhat < EPS).sum()), int((wl > 10 * gl).sum()), int((gl > 10 * wl).sum())))
            for mode, S in (("fp32", None), ("scaled", 1.0), ("scaled", 2.0 ** 16), ("scaled", 2.0 ** 24)):
                c.p[grp].copy_(p0); c.m[grp].zero_(); c.v[grp].zero_()
                # growth interval 1e6: the scale stays put over the 40 clean updates
                c.bind_state(None if S is None else [S, 1.0 / S, 0, 0, 0, 0, 1e6, 0])
                for t in range(1, SEQ_T + 1):
                    c.g[grp].copy_(grads[t - 1] if S is None else grads[t - 1] * S)      # S * g is exact: S is a power of two, |S g| < 2^31
                    c.step(grp, _seq_lr(t), t)
                    if t in SEQ_CHECK:
                        e = M.parity_metrics(c.p[grp].cpu(), c.m[grp].cpu(), c.v[grp].cpu(), ref[t], _seq_lr(t), t)
                        for k in M.METRICS:
                            rows.append((gname, mode if S is None else "S=2^%d" % round(math.log2(S)), t, k, e[k], err32[t][k]))
                if S is not None:
                    st = c.state_list()
                    assert st == [S, 1.0 / S, float(SEQ_T), 0, 0, 0, 1e6, S], st
            c.bind_state(None)
    bound = {k: 2 * max(r[5] for r in rows if r[3] == k) for k in M.METRICS}
    return SimpleNamespace(rows=rows, regimes=regimes, bound=bound)


def test_adam_40_steps_p_m_v_within_twice_torch_fp32_error_of_the_fp64_model(parity):
    print("\n(a) %d steps, lr %.1e halved from step %d, betas (%.1f, %.3f), eps %.0e, weight_decay %.0e; errors against the fp64 model"
          % (SEQ_T, LR0, SEQ_LR_STEP + 1, B1, B2, EPS, WD))
    print("  regimes (elements at the checked step):  group step n | sqrt(v_hat) < eps | wd|p| > 10|g| | |g| > 10 wd|p|")
    for r in parity.regimes:
        print("    %-3s %3d %7d | %6d | %7d | %7d" % r)
        assert r[4] > 0 and r[5] > 0, r
    assert all(r[3] > 0 for r in parity.regimes if r[1] == SEQ_CHECK[0]), parity.regimes       # the eps regime is populated
    print("  group path    step metric      HIP          torch-fp32   ratio")
    bad = []
    for gname, mode, t, k, hip, ref in parity.rows:
        print("    %-3s %-7s %3d  %-6s %12.4e %12.4e %7.3f" % (gname, mode, t, k, hip, ref, hip / ref))
        assert ref > 0
        if not hip <= 2 * ref:
            bad.append((gname, mode, t, k, hip, ref))
    print("  bound carried to the other groups of this module (2 x torch-fp32's largest):", {k: "%.3e" % v for k, v in parity.bound.items()})
    assert not bad, bad


# ---------------------------------------------------------------- (b) every element of the benchmarked launches
def _index_values(n, salt, lo_exp, hi_exp):
    """a deterministic function of the element index: magnitudes 10^lo_exp .. 10^hi_exp, signs, no two neighbours alike (fp64, on the GPU)"""
    i = torch.arange(n, device="cuda", dtype=torch.int64)
    h = ((i + salt) * 2654435761) % 1048573
    s = (((i + 7 * salt) * 40503) % 65521) % 2
    mag = 10.0 ** (lo_exp + (hi_exp - lo_exp) * h.double() / 1048573.0)
    return mag * (2.0 * s.double() - 1.0)


def _assert_under_bound(tag, c, grp, ref, lr, T, bound):
    e = M.parity_metrics(c.p[grp], c.m[grp], c.v[grp], ref, lr, T)
    print("    %s: " % tag + ", ".join("%s %.3e (bound %.3e)" % (k, e[k], bound[k]) for k in M.METRICS))
    bad = {k: (e[k], bound[k]) for k in M.METRICS if not e[k] <= bound[k]}
    assert not bad, (tag, bad)


@pytest.mark.parametrize("grp,gname", GROUPS, ids=["gen", "dis"])
def test_full_width_every_element_of_p_m_v_three_fp32_and_three_scaled_steps(L, parity, grp, gname):
    other = 1 - grp
    S = 2.0 ** 16
    with _context(L, FULL) as c:
        n = c.n[grp]
        assert n > PASS and n % PASS != 0                     # several passes of the capped grid, a ragged last one
        print("\n(b) %s: %d elements = %d full passes of %d + %d" % (gname, n, n // PASS, PASS, n % PASS))
        p0 = _index_values(n, 1, -3, 1).float()
        c.p[grp].copy_(p0)
        for buf in (c.p, c.g, c.m, c.v):
            buf[other].uniform_(-1, 1)
        keep = [buf[other].clone() for buf in (c.p, c.g, c.m, c.v)]
        a64 = M.Adam64(p0, B1, B2, EPS, WD)                   # fp64 on the GPU: independent of the kernels under test
        for t in range(1, 7):
            if t == 4:
                c.bind_state([S, 1.0 / S, 0, 0, 0, 0, 0, 0])
            g = _index_values(n, 100 + t, -6, 0).float()
            c.g[grp].copy_(g if t < 4 else g * S)
            c.step(grp, LR0, t)
            a64.step(g, LR0, t=t)
            if t in (3, 6):
                _assert_under_bound("%s after step %d (%s)" % (gname, t, "fp32 path" if t == 3 else "loss-scaled path"), c, grp, a64, LR0, t, parity.bound)
        assert c.state_list() == [S, 1.0 / S, 3.0, 0, 0, 0, 0, S]
        for name, buf, k in zip("pgmv", (c.p, c.g, c.m, c.v), keep):
            assert torch.equal(buf[other], k), "the other group's %s buffer changed" % name
        # an element the launch never reached would still hold v = 0: none does
        assert int((c.v[grp] == 0).sum()) == 0


# ---------------------------------------------------------------- (c) the non-finite scan at full size
def _scan_positions(c, grp):
    n = c.n[grp]
    klast = (n - 1) // PASS
    name, off, numel = c.tensor_span(grp, L_count(c, grp) // 2)
    pos = [("0", 0), ("n-1", n - 1), ("pass*1-1", PASS - 1), ("pass*1", PASS), ("pass*%d-1" % klast, PASS * klast - 1), ("pass*%d" % klast, PASS * klast),
           ("ragged last pass", PASS * klast + (n - PASS * klast) // 2), ("first of " + name, off), ("last of " + name, off + numel - 1)]
    assert all(0 <= p < n for _, p in pos) and klast >= 2 and 0 < off and off + numel < n
    return pos


def L_count(c, grp):
    return c.L.lib.aclgan_tensor_count(c.ctx, grp)


@pytest.mark.parametrize("grp,gname", GROUPS, ids=["gen", "dis"])
def test_full_width_one_non_finite_gradient_anywhere_skips_the_update(L, parity, grp, gname):
    other = 1 - grp
    S = 2.0 ** 16
    preset = [S, 1.0 / S, 5, 0, 2, 3, 0, 123.0]
    with _context(L, FULL) as c:
        n = c.n[grp]
        gen = torch.Generator(device="cuda").manual_seed(70 + grp)
        for buf, lo, hi in ((c.p, -1, 1), (c.m, -1e-2, 1e-2), (c.v, 1e-6, 1e-3)):
            buf[grp].uniform_(lo, hi, generator=gen)
        p0, m0, v0 = c.p[grp].clone(), c.m[grp].clone(), c.v[grp].clone()
        g_clean = torch.empty(n, device="cuda").uniform_(-1e-2, 1e-2, generator=gen) * S
        positions = _scan_positions(c, grp)
        print("\n(c) %s, n = %d: scan positions" % (gname, n), positions)
        # control: the clean buffer is applied (the scan does not skip everything)
        c.g[grp].copy_(g_clean); c.bind_state(preset); c.step(grp, LR0, 10)
        model = M.LossScaleModel(S, clean=5, skipped=(2, 3), last=123.0)
        assert model.adam_step(grp, False) and c.state_list() == model.state
        assert int((c.p[grp] != p0).sum()) > 0.99 * n
        tried = 0
        for label, pos in positions:
            for val in (float("inf"), float("-inf"), float("nan")):
                c.p[grp].copy_(p0); c.m[grp].copy_(m0); c.v[grp].copy_(v0)
                c.g[grp].copy_(g_clean); c.g[grp][pos] = val
                c.bind_state(preset)
                c.step(grp, LR0, 10)
                model = M.LossScaleModel(S, clean=5, skipped=(2, 3), last=123.0)
                assert not model.adam_step(grp, True)
                want = [S / 2, 2.0 / S, 0, 0, 2 + (grp == 0), 3 + (grp == 1), 0, S]       # halved, clean 0, this group's counter, flag cleared, [7] the old S
                st = c.state_list()
                assert st == want == model.state, (label, pos, val, st, want)
                assert torch.equal(c.p[grp], p0) and torch.equal(c.m[grp], m0) and torch.equal(c.v[grp], v0), (label, pos, val)
                tried += 1
        print("    %d placements (9 positions x +inf, -inf, nan): every one skipped the update, left p, m, v bit-unchanged, halved S" % tried)
        assert tried == 27
        assert float(c.p[other].abs().max()) == 0.0 and float(c.m[other].abs().max()) == 0.0 and float(c.v[other].abs().max()) == 0.0


@pytest.mark.parametrize("grp,gname", GROUPS, ids=["gen", "dis"])
def test_full_width_a_huge_finite_gradient_is_applied_like_torch_fp32_adam(L, parity, grp, gname):
    """3e38 at S = 1 is finite: the update is NOT skipped.  Its square overflows fp32, so v = inf there and the parameter stays
    (m / inf = 0): torch's fp32 Adam -- the reference's optimizer -- does the same; documented, not changed."""
    with _context(L, FULL) as c:
        n = c.n[grp]
        gen = torch.Generator().manual_seed(80 + grp)
        p0 = torch.empty(n).uniform_(-1, 1, generator=gen)
        g = torch.empty(n).uniform_(-1e-2, 1e-2, generator=gen)
        pos = PASS * ((n - 1) // PASS) + 12345               # inside the ragged last pass
        g[pos] = 3e38
        c.p[grp].copy_(p0); c.g[grp].copy_(g)
        c.bind_state([1.0, 1.0, 0, 0, 0, 0, 0, 0])
        c.step(grp, LR0, 1)
        assert c.state_list() == [1.0, 1.0, 1.0, 0, 0, 0, 0, 1.0]          # clean, no skip
        t32 = M.TorchAdam32(p0, B1, B2, EPS, WD)
        t32.step(g, LR0)
        p, m, v = c.p[grp].cpu(), c.m[grp].cpu(), c.v[grp].cpu()
        tp, tm, tv = t32.p.detach(), t32.m, t32.v
        print("\n(c) %s huge finite gradient at %d: HIP p %r m %r v %r | torch fp32 p %r m %r v %r (p0 %r)"
              % (gname, pos, p[pos].item(), m[pos].item(), v[pos].item(), tp[pos].item(), tm[pos].item(), tv[pos].item(), p0[pos].item()))
        assert torch.isinf(tv[pos]) and tp[pos] == p0[pos]                  # the reference's behaviour
        assert torch.equal(torch.isinf(v), torch.isinf(tv)) and int(torch.isinf(v).sum()) == 1
        assert p[pos] == p0[pos] and abs(m[pos].item() - tm[pos].item()) <= 1e-6 * abs(tm[pos].item())
        assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(m).all()) and not bool(torch.isnan(v).any())
        # everything else: two fp32 evaluations of one step, each within its own error of fp64 -> apart by at most 1.5 x the bound of (a)
        ok = torch.ones(n, dtype=torch.bool); ok[pos] = False
        gv = (g.double() + WD * p0.double()).abs()
        ep = ((p.double() - tp.double()).abs() / (LR0 * 1e-6 + M.EPS32 * tp.double().abs()))[ok].max().item()
        ev = ((v.double() - tv.double()).abs() / tv.double().clamp_min(1e-300))[ok].max().item()
        em = ((m.double() - tm.double()).abs() / gv.clamp_min(1e-300))[ok].max().item()
        print("    other elements, HIP vs torch fp32: p %.3e v %.3e m_eff %.3e (1.5 x bound: %.3e %.3e %.3e)"
              % (ep, ev, em, 1.5 * parity.bound["p"], 1.5 * parity.bound["v"], 1.5 * parity.bound["m_eff"]))
        assert ep <= 1.5 * parity.bound["p"] and ev <= 1.5 * parity.bound["v"] and em <= 1.5 * parity.bound["m_eff"]


# ---------------------------------------------------------------- (d) state-machine trace
# (group, what the gradient buffer holds, presets applied to the caller-owned state before the call)
TRACE = [
    (1, "+inf", None), (1, None, None), (0, "nan", None), (1, "-inf", None), (0, None, None), (1, None, None), (0, "+inf", None), (0, None, None),
    (1, "nan", None),                                  # S is 1 here: the floor, 2 -> 1 -> 1
    (0, None, None), (1, None, None), (0, None, None),  # three clean updates of BOTH groups together: growth (interval 3)
    (1, None, None),
    (0, None, {0: 2.0 ** 23, 1: 2.0 ** -23, 2: 2.0}),   # 2^23 -> 2^24
    (1, None, {2: 2.0}),                                # the cap: 2^24 -> 2^24
    (1, "-inf", None),
    (0, None, {0: 65536.0, 1: 2.0 ** -16, 2: 1999.0, 6: 0.0}),      # interval 0 means 2000: the next clean update doubles
    (1, None, None),
]


def test_loss_scale_state_machine_trace_and_bias_correction_counts_applied_updates(L, parity):
    with _context(L, SMALL) as c:
        model = M.LossScaleModel(16.0, interval=3)
        c.bind_state(model.state)
        gen = torch.Generator().manual_seed(90)
        adam, host_step = [], [0, 0]
        for grp in (0, 1):
            p0 = (10.0 ** (torch.rand(c.n[grp], generator=gen, dtype=torch.float64) * 4 - 3) * _sign(c.n[grp], gen)).float()
            c.p[grp].copy_(p0)
            adam.append(M.Adam64(p0, B1, B2, EPS, WD))
        seen = set()
        pattern = {0: "", 1: ""}
        print("\n(d) call group buffer -> state[0..7]")
        for i, (grp, badval, preset) in enumerate(TRACE):
            if preset:
                for k, x in preset.items():
                    model.state[k] = float(x)
                c.bind_state(model.state)
            n = c.n[grp]
            S = model.state[0]
            lr = M.f32(LR0 * (0.5 if i >= 10 else 1.0))
            g = (10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 6 - 6) * _sign(n, gen)).float()
            c.g[grp].copy_(g * S)
            if badval is not None:
                c.g[grp][(0, n - 1, n // 2)[i % 3]] = float(badval)
            before = [b[grp].clone() for b in (c.p, c.m, c.v)]
            other = [b[1 - grp].clone() for b in (c.p, c.m, c.v)]
            host_step[grp] += 1
            c.step(grp, lr, host_step[grp])
            old = list(model.state)
            applied = model.adam_step(grp, badval is not None)
            st = c.state_list()
            print("    %2d %s %-5s %s" % (i, "gen" if grp == 0 else "dis", badval or "clean", st))
            assert st == model.state, (i, st, model.state)                 # small integers, powers of two and their reciprocals: exact
            assert all(torch.equal(b[1 - grp], o) for b, o in zip((c.p, c.m, c.v), other))
            pattern[grp] += "a" if applied else "s"
            if applied:
                t = model.bias_correction_step(grp, host_step[grp])
                assert t == adam[grp].applied + 1
                adam[grp].step(g, lr, t=t)
                _assert_under_bound("call %d, bias-correction step %d of host step %d" % (i, t, host_step[grp]), c, grp, adam[grp], lr, t, parity.bound)
            else:
                assert all(torch.equal(b[grp], o) for b, o in zip((c.p, c.m, c.v), before)), i
            # which rules of the contract this call exercised
            if not applied:
                seen.add("floor" if old[0] == 1.0 and st[0] == 1.0 else "halve")
            elif st[0] == 2 * old[0]:
                seen.add("default interval" if old[6] == 0 else "grow")
            elif old[0] == 2.0 ** 24 and old[2] + 1 >= old[6] > 0:
                seen.add("cap")
            assert st[7] == old[0] and st[1] == 1.0 / st[0] and st[3] == 0
        assert seen == {"floor", "halve", "grow", "default interval", "cap"}, seen
        assert pattern[0].startswith("sasa") and pattern[1].startswith("sasa"), pattern     # skip, apply, skip, apply per group
        assert model.state[4] == 2 and model.state[5] == 4


# ---------------------------------------------------------------- (e) trainer level
def test_trainer_growth_doubles_the_scale_the_next_buffers_carry_and_save_writes_the_state(L, tmp_path):
    from aclgan_amd import trainer as T
    cfg = O.default_config()
    cfg["gen"].update(dim=32, mlp_dim=32, n_res=1)
    cfg["dis"].update(dim=32)
    cfg["display_size"] = 1
    nets = O.test_nets(cfg, 2)
    g = torch.Generator().manual_seed(27)
    x_a = torch.rand(1, 3, 64, 64, generator=g) * 2 - 1
    x_b = torch.rand(1, 3, 64, 64, generator=g) * 2 - 1
    z = [torch.randn(1, 8, 1, 1, generator=g) for _ in range(6)]

    def make(interval):
        c = dict(cfg)
        if interval is not None:
            c["loss_scale_growth_interval"] = interval
        # deterministic plan: the two trainers below must make the same roundings (the default plan's fp32 atomics reorder sums run to run)
        tr = T.aclgan_Trainer(c, compute_dtype="fp16", deterministic=True)
        for name in O.OracleTrainer.NETS:
            getattr(tr, name).load_state_dict(nets[name], strict=False)
        return tr, c

    prev_det = L.lib.aclgan_get_deterministic()
    try:
        _trainer_growth_body(L, tmp_path, make, x_a, x_b, z)
    finally:
        L.check(L.lib.aclgan_set_deterministic(prev_det))


def _trainer_growth_body(L, tmp_path, make, x_a, x_b, z):
    tr, c2 = make(2)
    twin, ct = make(None)               # the same run with the default interval: its scale never moves
    S = 65536.0
    assert tr.grad_scale() == S
    for t_, c_ in ((tr, c2), (twin, ct)):
        t_.dis_update(x_a, x_b, c_, z=z[:3])
    assert tr._lscale.cpu().tolist() == [S, 1 / S, 1, 0, 0, 0, 2, S]
    for t_, c_ in ((tr, c2), (twin, ct)):
        t_.gen_update(x_a, x_b, c_, z=z[3:])
    torch.cuda.synchronize()
    # one dis update + one gen update = 2 clean updates: the scale doubles; the buffers of those two updates carried S
    assert tr._lscale.cpu().tolist() == [2 * S, 0.5 / S, 0, 0, 0, 0, 2, S]
    assert twin._lscale.cpu().tolist() == [S, 1 / S, 2, 0, 0, 0, 2000, S]
    assert tr.grad_scale("gen") == S and tr.grad_scale("dis") == S
    assert torch.equal(tr._param[0], twin._param[0]) and torch.equal(tr._param[1], twin._param[1])
    for t_, c_ in ((tr, c2), (twin, ct)):
        t_.dis_update(x_a, x_b, c_, z=z[:3])
    torch.cuda.synchronize()
    assert tr.grad_scale("dis") == 2 * S and tr.grad_scale() == 2 * S and twin.grad_scale("dis") == S and tr.grad_scale("gen") == S
    # ... and they really do: the same update from the same parameters at S and at 2 S (a power of two: the fp16 roundings coincide
    # except in the subnormal range)
    a, b = tr._grad[1].double(), twin._grad[1].double()
    rel = ((a - 2 * b).norm() / (2 * b).norm()).item()
    print("\n(e) gradient buffer at 2S against twice the buffer at S: relative L2 %.3e" % rel)
    assert float(b.norm()) > 0 and rel <= 1e-3
    assert tr._lscale.cpu().tolist() == [2 * S, 0.5 / S, 1, 0, 0, 0, 2, 2 * S]
    # a skipped generator update, then the checkpoint
    tr._lscale[0] = 2.0 ** 40; tr._lscale[1] = 2.0 ** -40
    tr.gen_update(x_a, x_b, c2, z=z[3:])
    torch.cuda.synchronize()
    live = tr._lscale.cpu().clone()
    assert live.tolist() == [2.0 ** 39, 2.0 ** -39, 0, 0, 1, 0, 2, 2.0 ** 40]
    tr.save(str(tmp_path), 0)
    sd = torch.load(str(tmp_path / "optimizer.pt"), map_location="cpu")
    assert torch.equal(sd["aclgan_loss_scale_state"], live) and sd["aclgan_loss_scale_state"].dtype == torch.float32
    applied = {"gen": 1, "dis": 2}
    skipped = {"gen": int(live[4]), "dis": int(live[5])}
    for key, grp in (("gen", 0), ("dis", 1)):
        steps = {float(s["step"]) for s in sd[key]["state"].values()}
        assert steps == {float(applied[key] + skipped[key])}, (key, steps)
        assert len(steps) == 1 and len(sd[key]["state"]) > 0
