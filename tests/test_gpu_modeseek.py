"""Mode-seeking regulariser of the generators on the GPU (csrc/modeseek.hip: modeseek_part_kernel / modeseek_grad_kernel; aclgan_modeseek,
aclgan_ctx_set_modeseek; config key ms_lambda):
  1. the operator against the fp64 model of tests/modeseek_ref.py at the edges of its decomposition, aligned and offset pointers, both
     accumulate modes, degenerate rows; two calls give identical bits;
  2. one fp32 gen_update with the key on against the same update with it off: the twelve losses keep their bits, out8 is the oracle's, and the
     DIFFERENCE of every generator gradient tensor is the oracle's gradient of the term (exactly zero under enc_style);
  3. 1 and 3 lanes, 4. graph replay, 5. key off / set and reset: the same bits;
  6. bf16 and fp16 updates against the fp32 oracle at the bounds of tests/test_gpu_step16.py; the fp16 loss scale cancels;
  7. train.py --synthetic prints the four fields and leaves losses.csv as it was.
Bounds: values 1e-5 relative (the bound of the sibling streaming reduction, tests/test_gpu_gradclip.py: NORM_BOUND), the per-image coefficient
1e-5 relative, the sign pattern exact; losses 1e-3 and per-tensor gradients 3e-2 + the 1e-5 gmax floor, both as tests/test_gpu_step.py states
them for its smooth fixtures (ltol, ETOL_SMOOTH)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import aclgan_oracle as O
from modeseek_ref import gen_losses_ms, ms_seeds, ms_value

pytestmark = pytest.mark.gpu

VALUE_BOUND = 1e-5          # tests/test_gpu_gradclip.py: NORM_BOUND
LTOL = 1e-3                 # tests/test_gpu_step.py: ltol of test_update_steps_match_reference
ETOL = 3e-2                 # tests/test_gpu_step.py: ETOL_SMOOTH (the un-frozen per-tensor bound; with its floor of 1e-5 * gmax)
# tests/test_gpu_step16.py: FTOL (forward tensors against the fp32 oracle) and GTOL (per-tensor gradients against the fp32 oracle, floor 1e-4 gmax)
FTOL16 = {"bf16": 6e-2, "fp16": 8e-3}
GTOL16 = {"bf16": 3e-1, "fp16": 1.2e-1}
# The weight of the difference test.  Chosen on the CPU with the fp32 oracle: on both fixtures below the gradient of (ms_B + ms_A) is 10 .. 10^4
# times the update's own gradient in every generator tensor outside enc_style (smallest ratio: 9.7, gen_AB dec.model.5.conv.bias of the plain
# fixture), so 1.0 -- the paper's value -- puts ||Delta_ref|| two orders above the 0.1 ||g_ref(0)|| the test asks for.
LAM = 1.0
FIXTURES = ("step_reduced_64_smooth", "step_reduced_64_plain")      # focus and plain configuration, reduced width, 64x64, B = 2
GEN = ("gen_AB", "gen_BA")


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def T(L):
    from aclgan_amd import trainer
    return trainer


def _record(key, value):
    """(scripts/bench_modeseek.py's companion figures: profiles/modeseek_parity.json)"""
    out = os.environ.get("ACLGAN_MODESEEK_PARITY_OUT")
    if not out:
        return
    doc = json.load(open(out)) if os.path.exists(out) else {}
    doc[key] = value
    json.dump(doc, open(out, "w"), indent=1)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------- (1) the operator
CHUNK = 4 * 512             # include/aclgan_hip.h: chunks per image = min(128, max(1, ceil((n / 4) / 512)))
SIZES = [1, 3, 4, 5, 255, 256, 257, CHUNK + 3, CHUNK + 4, 3 * 64 * 64]


def _op(L, a, b, u, u2, u_scale, weight, out4, da, db, acc, scratch, lscale=None):
    B, n = a.shape
    L.check(L.lib.aclgan_modeseek(L.ptr(a), L.ptr(b), B, n, L.ptr(u), L.ptr(u2), u.shape[1], u_scale, weight, L.ptr(lscale), L.ptr(out4), L.ptr(da), L.ptr(db),
                                  acc, L.ptr(scratch), L.stream_ptr()), "modeseek")


def test_operator_against_fp64(L):
    assert L.lib.aclgan_modeseek_scratch_bytes(1, CHUNK + 3) == 4 and L.lib.aclgan_modeseek_scratch_bytes(1, CHUNK + 4) == 8      # the chunk boundary
    g = torch.Generator().manual_seed(11)
    nmax = 3 * max(SIZES) + 8
    pool = [(torch.rand(nmax, generator=g) * 2 - 1).cuda() for _ in range(4)]      # a, b, da, db are cut from these at the offset under test
    assert all(p.data_ptr() % 16 == 0 for p in pool)
    worst = {"value": 0.0, "div": 0.0, "coef": 0.0}
    cases = 0
    for n in SIZES:
        for B in (1, 2, 3):
            for sd in (1, 8):
                u, u2 = torch.randn(B, sd, generator=g), torch.randn(B, sd, generator=g)
                if B >= 2:
                    u2[0] = u[0]                                  # one row with u == u'
                for offs in ((0, 0, 0, 0), (1, 1, 1, 1), (0, 1, 1, 0)):      # aligned; offset by one float together; apart (no common 16-byte boundary)
                    a = pool[0].clone()[offs[0]:offs[0] + B * n].view(B, n)
                    b = pool[1].clone()[offs[1]:offs[1] + B * n].view(B, n)
                    assert a.data_ptr() % 16 == 4 * offs[0] and b.data_ptr() % 16 == 4 * offs[1]
                    if B >= 2:
                        b[B - 1] = a[B - 1]                       # one image with I == I'
                    b[0, ::7] = a[0, ::7]                         # sign(0) = 0 inside an image
                    u_scale, lam = (0.5, 0.7) if sd == 8 else (1.0, 1.0)
                    ud, u2d = u.cuda(), u2.cuda()
                    vref, dref = ms_value(a.double().cpu(), b.double().cpu(), u_scale * u.double(), u_scale * u2.double())
                    _, _, kref = ms_seeds(a.double().cpu(), b.double().cpu(), u_scale * u.double(), u_scale * u2.double(), lam)
                    scratch = torch.zeros(L.lib.aclgan_modeseek_scratch_bytes(B, n) // 4, device="cuda")
                    sgn = torch.sign(a - b)
                    for acc in (0, 1):
                        da = (pool[2].clone()[offs[2]:offs[2] + B * n]).view(B, n)
                        db = (pool[3].clone()[offs[3]:offs[3] + B * n]).view(B, n)
                        assert da.data_ptr() % 16 == 4 * offs[2] and db.data_ptr() % 16 == 4 * offs[3]
                        da_in, db_in = da.clone(), db.clone()
                        out4 = torch.full((4,), 7.0, device="cuda")
                        _op(L, a, b, ud, u2d, u_scale, lam / B, out4, da, db, acc, scratch)
                        if acc == 0:
                            first = (out4.clone(), da.clone(), db.clone())
                            _op(L, a, b, ud, u2d, u_scale, lam / B, out4, da, db, acc, scratch)      # two calls: identical bits
                            assert same_bits(out4, first[0]) and same_bits(da, first[1]) and same_bits(db, first[2]), (n, B, sd, offs)
                            o = out4.cpu().tolist()
                            assert o[2:] == [0.0, 0.0]
                            rv = abs(o[0] - float(vref)) / max(abs(float(vref)), 1e-30) if float(vref) else abs(o[0])
                            rd = abs(o[1] - float(dref)) / max(abs(float(dref)), 1e-30) if float(dref) else abs(o[1])
                            worst["value"], worst["div"] = max(worst["value"], rv), max(worst["div"], rd)
                            assert rv <= VALUE_BOUND and rd <= VALUE_BOUND, (n, B, sd, offs, o, float(vref), float(dref))
                            # the gradient: -k_b sign(a - b) in da, its negative in db; k_b one float per image
                            assert torch.equal(torch.sign(da), -sgn * (kref.float().cuda() > 0).float()[:, None]), (n, B, sd, offs)
                            assert torch.equal(db, -da)
                            for i in range(B):
                                nz = da[i][sgn[i] != 0].abs()
                                if float(kref[i]) == 0 or nz.numel() == 0:
                                    assert float(da[i].abs().max()) == 0
                                    continue
                                assert float(nz.min()) == float(nz.max())
                                rk = abs(float(nz[0]) - float(kref[i])) / float(kref[i])
                                worst["coef"] = max(worst["coef"], rk)
                                assert rk <= VALUE_BOUND, (n, B, sd, offs, i, float(nz[0]), float(kref[i]))
                            plain = (da.clone(), db.clone())
                        else:
                            assert torch.equal(da, da_in + plain[0]) and torch.equal(db, db_in + plain[1]), (n, B, sd, offs)
                        cases += 1
                    # monitoring only: the same values, no gradient
                    out4m = torch.zeros(4, device="cuda")
                    _op(L, a, b, ud, u2d, u_scale, lam / B, out4m, None, None, 0, scratch)
                    assert same_bits(out4m, first[0])
    torch.cuda.synchronize()
    print("(1) %d cases: worst relative error value %.3e, div %.3e, coefficient %.3e (bound %.0e)" % (cases, worst["value"], worst["div"], worst["coef"], VALUE_BOUND))
    _record("operator", {"bound": VALUE_BOUND, "cases": cases, "worst_relative_error": worst})


def test_operator_loss_scale_multiplies_the_seeds_only(L):
    g = torch.Generator().manual_seed(12)
    a, b = (torch.rand(2, 300, generator=g) * 2 - 1).cuda(), (torch.rand(2, 300, generator=g) * 2 - 1).cuda()
    u, u2 = torch.randn(2, 8, generator=g).cuda(), torch.randn(2, 8, generator=g).cuda()
    scratch = torch.zeros(L.lib.aclgan_modeseek_scratch_bytes(2, 300) // 4, device="cuda")
    res = []
    for S in (None, 1024.0):
        ls = None if S is None else torch.tensor([S, 1 / S, 0, 0, 0, 0, 0, 0], device="cuda")
        out4, da, db = torch.zeros(4, device="cuda"), torch.zeros(2, 300, device="cuda"), torch.zeros(2, 300, device="cuda")
        _op(L, a, b, u, u2, 1.0, 0.5, out4, da, db, 0, scratch, ls)
        res.append((out4, da, db))
    assert same_bits(res[0][0], res[1][0])
    assert float(((res[1][1] / 1024.0 - res[0][1]).abs() / res[0][1].abs().clamp_min(1e-30)).max()) <= 2e-7      # a power of two: one rounding of k
    assert torch.equal(res[1][2], -res[1][1])


# ---------------------------------------------------------------- the updates: fixtures and the oracle's side, computed once
def _load(name):
    meta = json.load(open(os.path.join(GOLDEN, name + ".json")))
    data = np.load(os.path.join(GOLDEN, name + ".npz"))
    cfg = meta["config"]
    x_a, x_b = torch.from_numpy(data["x_a"]), torch.from_numpy(data["x_b"])
    z = [torch.from_numpy(data["z%d" % i]) for i in range(3, 6)]
    g = torch.Generator().manual_seed(407)
    z_ms = [torch.randn(x_a.shape[0], cfg["gen"]["style_dim"], 1, 1, generator=g) for _ in range(2)]
    return cfg, O.test_nets(cfg, 0), x_a, x_b, z, z_ms


_ORACLE = {}


def _oracle(fix):
    """fp32 oracle: the update's own gradient g0, the gradient of LAM * (ms_B + ms_A) alone (Delta_ref), and the four values"""
    if fix in _ORACLE:
        return _ORACLE[fix]
    cfg, nets0, x_a, x_b, z, z_ms = _load(fix)
    out = []
    for which in (0, 1):
        nets = {k: {n: t.detach().clone().requires_grad_(True) for n, t in v.items()} for k, v in nets0.items()}
        total, _, _, ms = gen_losses_ms(nets, x_a, x_b, z, z_ms, cfg)
        (total if which == 0 else LAM * (ms["ms_B"] + ms["ms_A"])).backward()
        out.append({(n, k): (t.grad if t.grad is not None else torch.zeros_like(t)) for n in GEN for k, t in nets[n].items()})
    _ORACLE[fix] = (out[0], out[1], {k: float(v.detach()) for k, v in ms.items()})
    return _ORACLE[fix]


def _make(T, cfg, nets, **kw):
    tr = T.aclgan_Trainer(cfg, **kw)
    for name in O.OracleTrainer.NETS:
        getattr(tr, name).load_state_dict(nets[name], strict=False)
    return tr


def _grads(tr):
    return {(n, k): g.contiguous().clone() for n in GEN for k, g in getattr(tr, n).named_grads()}


def _out8(tr):
    return {"ms_B": float(tr.loss_gen_ms_B), "div_B": float(tr.gen_diversity_B), "ms_A": float(tr.loss_gen_ms_A), "div_A": float(tr.gen_diversity_A)}


class _det:
    def __init__(self, L):
        self.L = L

    def __enter__(self):
        self.prev = self.L.lib.aclgan_get_deterministic()

    def __exit__(self, *a):
        self.L.check(self.L.lib.aclgan_set_deterministic(self.prev))


def _tune(L, key, value):
    prev = C.c_int()
    L.check(L.lib.aclgan_tuning(key, value, C.byref(prev)), "aclgan_tuning")
    return prev.value


# ---------------------------------------------------------------- (2) the difference of two updates
@pytest.mark.parametrize("fix", FIXTURES)
def test_update_difference_is_the_gradient_of_the_term(L, T, fix):
    cfg, nets, x_a, x_b, z, z_ms = _load(fix)
    assert x_a.shape == (2, 3, 64, 64)
    on = dict(cfg, ms_lambda=LAM)
    g0_ref, d_ref, ms_ref = _oracle(fix)
    with _det(L):
        tr0 = _make(T, cfg, nets, deterministic=True)
        tr0.gen_update(x_a, x_b, cfg, z=z)
        tr1 = _make(T, on, nets, deterministic=True)
        tr1.gen_update(x_a, x_b, on, z=z, z_ms=z_ms)
        torch.cuda.synchronize()
    assert tr0.ms_lambda == 0 and tr0._ms_out is None and tr1.ms_lambda == LAM
    # the original forward is untouched
    assert same_bits(tr0._losses[:12], tr1._losses[:12]), (tr0._losses[:12].tolist(), tr1._losses[:12].tolist())
    got = _out8(tr1)
    for k, v in ms_ref.items():
        print("    %s %s: hip %.7g oracle %.7g rel %.2e" % (fix, k, got[k], v, abs(got[k] - v) / max(1e-3, abs(v))))
    for k, v in ms_ref.items():
        assert abs(got[k] - v) <= LTOL * max(1e-3, abs(v)), (k, got[k], v)
    assert float(tr0.loss_gen_ms_A) == 0 and float(tr0.gen_diversity_B) == 0
    ga, gb = _grads(tr0), _grads(tr1)
    assert set(ga) == set(g0_ref)
    gmax = max(float(v.double().norm()) for v in d_ref.values())
    seen = []
    for key in sorted(ga):
        dh = gb[key].cpu().double() - ga[key].cpu().double()
        if key[1].startswith("enc_style."):      # s_2 and s_4 only feed the reconstructions
            assert float(d_ref[key].abs().max()) == 0 and same_bits(ga[key], gb[key]), key
            continue
        dr = d_ref[key].double()
        # the precondition, on the oracle's side: the term moves this tensor by at least a tenth of its gradient, fp32 cancellation in
        # g(lam) - g(0) then stays two orders below the bound
        assert float(dr.norm()) >= 0.1 * float(g0_ref[key].double().norm()), (key, float(dr.norm()), float(g0_ref[key].double().norm()))
        err = float((dh - dr).norm())
        seen.append((err / (float(dr.norm()) + 1e-5 * gmax / ETOL), key))
        assert err <= ETOL * float(dr.norm()) + 1e-5 * gmax, (key, err, float(dr.norm()))      # (tests/test_gpu_step.py: l2ok)
    seen.sort(reverse=True)
    print("(2) %s: worst ||Delta_hip - Delta_ref|| / ||Delta_ref|| over %d tensors:" % (fix, len(seen)), [("%.2e" % e, k) for e, k in seen[:3]])
    _record("update_difference_" + fix, {"lam": LAM, "bound": ETOL, "tensors": len(seen), "worst_ratio": seen[0][0], "worst_tensor": "/".join(seen[0][1]),
                                         "out8": got, "oracle": ms_ref})


# ---------------------------------------------------------------- (3) lanes
def test_lane_count_does_not_change_a_bit(L, T):
    cfg, nets, x_a, x_b, z, z_ms = _load(FIXTURES[0])
    on = dict(cfg, ms_lambda=LAM)
    prev = _tune(L, b"lanes", 1)
    res = []
    try:
        with _det(L):
            for lanes in (1, 3):
                _tune(L, b"lanes", lanes)
                tr = _make(T, on, nets, deterministic=True)
                tr.gen_update(x_a, x_b, on, z=z, z_ms=z_ms)
                torch.cuda.synchronize()
                res.append((tr._grad[0].clone(), tr._param[0].clone(), tr._ms_out.clone(), tr._losses.clone()))
    finally:
        _tune(L, b"lanes", prev)
    for a, b in zip(*res):
        assert same_bits(a, b)
    assert float(res[0][2][0]) > 0 and float(res[0][2][4]) > 0


# ---------------------------------------------------------------- (4) graph replay
def test_graph_replay_matches_eager(L, T):
    cfg, nets, x_a, x_b, z, _ = _load(FIXTURES[0])
    on = dict(cfg, ms_lambda=LAM)
    g = torch.Generator().manual_seed(408)
    zs = [[torch.randn(2, 8, 1, 1, generator=g) for _ in range(2)] for _ in range(3)]      # update 1 eager, 2 captures, 3 replays
    res = []
    with _det(L):
        for graph in (False, True):
            tr = _make(T, on, nets, deterministic=True, hip_graph=graph)
            outs = []
            for z_ms in zs:
                tr.gen_update(x_a, x_b, on, z=z, z_ms=z_ms)
                outs.append(tr._ms_out.clone())
            torch.cuda.synchronize()
            res.append((tr, outs, tr._param[0].clone(), tr._m[0].clone(), tr._v[0].clone()))
    tg = res[1][0]
    assert tg.hip_graph and tg._graphs["gen"]["graph"] is not None, "capture fell back to eager execution"
    for a, b in zip(res[0][1], res[1][1]):
        assert same_bits(a, b), (a.tolist(), b.tolist())
    assert not same_bits(res[0][1][1], res[0][1][2])          # fresh noise reached the replayed graph
    for i in (2, 3, 4):
        assert same_bits(res[0][i], res[1][i])


# ---------------------------------------------------------------- (5) key off; lambda set, then reset to 0
def test_key_off_and_reset_leave_no_trace(L, T):
    cfg, nets, x_a, x_b, z, _ = _load(FIXTURES[0])
    g = torch.Generator().manual_seed(409)
    zd = [torch.randn(2, 8, 1, 1, generator=g) for _ in range(3)]
    res = []
    with _det(L):
        for mode in ("never", "zero", "reset"):
            c = dict(cfg, ms_lambda=0) if mode == "zero" else cfg
            tr = _make(T, c, nets, deterministic=True)
            if mode == "reset":
                dev, out = torch.zeros(2, 2, 8, device="cuda"), torch.zeros(8, device="cuda")
                L.check(L.lib.aclgan_ctx_set_modeseek(tr._ctx, 1.0, L.ptr(dev), 4, L.ptr(out)))
                L.check(L.lib.aclgan_ctx_set_modeseek(tr._ctx, 0.0, L.ptr(dev), 4, L.ptr(out)))
            n0 = L.lib.aclgan_launch_count()
            for _ in range(2):
                tr.dis_update(x_a, x_b, c, z=zd)
                tr.gen_update(x_a, x_b, c, z=z)
            torch.cuda.synchronize()
            res.append([L.lib.aclgan_launch_count() - n0] + [t[grp].clone() for grp in (0, 1) for t in (tr._param, tr._m, tr._v)])
            assert tr._ms_out is None and not tr._ms_dev
    assert res[0][0] == res[1][0] == res[2][0]
    for other in res[1:]:
        for a, b in zip(res[0][1:], other[1:]):
            assert same_bits(a, b)
    # a gen_update whose rows do not match its batch is refused before anything is enqueued
    tr = _make(T, cfg, nets)
    dev, out = torch.zeros(2, 3, 8, device="cuda"), torch.zeros(8, device="cuda")
    L.check(L.lib.aclgan_ctx_set_modeseek(tr._ctx, 1.0, L.ptr(dev), 6, L.ptr(out)))
    n0 = L.lib.aclgan_launch_count()
    with pytest.raises(L.AclganError, match="mode-seeking noise rows"):
        tr.gen_update(x_a, x_b, cfg, z=z)
    tr.dis_update(x_a, x_b, cfg, z=zd)      # dis_update does not read them
    L.check(L.lib.aclgan_ctx_set_modeseek(tr._ctx, 0.0, None, 0, None))
    with pytest.raises(L.AclganError, match="z_ms"):
        tr.gen_update(x_a, x_b, cfg, z=z, z_ms=[zd[0], zd[1]])


# ---------------------------------------------------------------- (6) 16-bit compute
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_update_16bit(L, T, dt):
    fix = FIXTURES[0]
    cfg, nets, x_a, x_b, z, z_ms = _load(fix)
    on = dict(cfg, ms_lambda=LAM)
    g0_ref, d_ref, ms_ref = _oracle(fix)
    ref = {k: (g0_ref[k] + d_ref[k]).double() for k in g0_ref}
    gmax = max(float(v.norm()) for v in ref.values())

    def run(c):
        tr = _make(T, c, nets, compute_dtype=dt)
        S = tr.grad_scale()
        tr.gen_update(x_a, x_b, c, z=z, z_ms=z_ms)
        torch.cuda.synchronize()
        return tr, S, {k: v.cpu().double() / S for k, v in _grads(tr).items()}
    tr, S, got = run(on)
    assert S == (65536.0 if dt == "fp16" else 1.0)
    o8 = _out8(tr)
    for k, v in ms_ref.items():
        print("    %s %s: hip %.6g fp32 oracle %.6g rel %.2e" % (dt, k, o8[k], v, abs(o8[k] - v) / abs(v)))
    # dI is a mean over 12288 absolute differences of pixels that each sit within FTOL of the oracle's: the means, and their ratios to the
    # exactly known dz, carry at most that relative error
    for k, v in ms_ref.items():
        assert abs(o8[k] - v) <= FTOL16[dt] * abs(v), (k, o8[k], v)
    worst = sorted(((float((got[k] - ref[k]).norm()) / (float(ref[k].norm()) + 1e-4 * gmax), k) for k in ref), reverse=True)
    print("(6) %s worst gradient tensors vs the fp32 oracle (relative L2):" % dt, [("%.2e" % e, k) for e, k in worst[:4]])
    assert worst[0][0] <= GTOL16[dt], worst[:6]      # (tests/test_gpu_step16.py: test_step_gradients_16bit)
    if dt == "fp16":
        assert tr.loss_scale_state()["skipped_gen"] == 0
        tr2, S2, got2 = run(dict(on, loss_scale_init=2 * 65536.0))
        assert S2 == 2 * 65536.0 and tr2.loss_scale_state()["skipped_gen"] == 0
        w2 = max(float((got2[k] - got[k]).norm()) / (float(ref[k].norm()) + 1e-4 * gmax) for k in ref)
        print("    fp16: unscaled gradient at twice the loss scale against the first run, worst relative L2 %.2e" % w2)
        assert w2 <= GTOL16[dt]
        assert same_bits(tr2._ms_out, tr._ms_out)      # the values carry no scale


# ---------------------------------------------------------------- (7) train.py
def test_train_py_prints_the_four_fields(L, tmp_path):
    from test_gpu_visual import _tiny_config, _train
    out = str(tmp_path)
    r = _train(out, _tiny_config(image_save_iter=10000, image_display_iter=10000, snapshot_save_iter=10000, max_iter=3, ms_lambda=1.0))
    lines = [l for l in r.stdout.splitlines() if l.startswith("Iteration:")]
    assert len(lines) == 3 and "Iteration: 00000003/00000003" in lines[-1]
    for l in lines:
        fields = dict(f.split("=") for f in l.split() if "=" in f)
        assert all(k in fields for k in ("ms_A", "ms_B", "div_A", "div_B")), l
        assert all(np.isfinite(float(fields[k])) and float(fields[k]) > 0 for k in ("ms_A", "ms_B", "div_A", "div_B")), l
    rows = open(os.path.join(out, "logs", "tiny", "losses.csv")).read().splitlines()
    assert rows[0].split(",") == ["iteration"] + L.LOSS_NAMES and len(rows) == 4 and all(len(x.split(",")) == 17 for x in rows[1:])
