"""Adaptive dis_augment probability on the GPU (csrc/ada.hip: augment_gate_kernel / ada_sign_kernel / ada_fold_kernel; aclgan_ctx_set_ada;
config keys dis_augment_p / ada_target / ada_interval / ada_kimg): the gate, the sign statistic and the fold against the numpy model of
tests/ada_ref.py, then the trainer -- bits against a key-off twin at p = 1 and p = 0, the steered controller, the signal against the
discriminators' own forward, lanes and graph replay, checkpoints and the error paths.  Run on the GPU box: pytest -m gpu"""
import copy
import ctypes as C
import math
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import aclgan_oracle as O
from diffaug_ref import neutral_params
from gpu_util import deterministic_mode
import ada_ref as R

pytestmark = pytest.mark.gpu


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


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.int32)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the gate
# ---------------------------------------------------------------------------------------------------------------------------------
def test_gate_is_the_models_select_bit_for_bit(L):
    """n in {1, 5, 21, 257} (257: a second workgroup), every policy, p in {0, 0.25, 1} and a p equal to one of the uniforms: rows_eff holds the
    model's bits; p = 1 returns the rows, p = 0 the neutral values in the policy's columns.  rows hold a NaN and a -0.0: bits, not values"""
    g = torch.Generator().manual_seed(7)
    H, W = 48, 80
    for n in (1, 5, 21, 257):
        rows = torch.randn(n, 8, generator=g)
        rows[0, 0] = float("nan")
        rows[n // 2, 3] = -0.0
        u = torch.rand(n, 4, generator=g)
        rows_d, u_d = rows.cuda(), u.cuda()
        for policy in range(1, 8):
            on = [c for bit, cols in R.OPS if policy & bit for c in cols]
            for p in (0.0, 0.25, 1.0, float(u[n // 3, 1]), float(u[n - 1, 0])):
                state = torch.zeros(12)
                state[0] = p
                state_d = state.cuda()
                eff = torch.full((n, 8), 7.0, device="cuda")
                L.check(L.lib.aclgan_augment_gate(L.ptr(rows_d), L.ptr(u_d), L.ptr(state_d), n, H, W, policy, L.ptr(eff), L.stream_ptr()), "augment_gate")
                want = R.gate(rows.numpy(), u.numpy(), np.float32(p), H, W, policy)
                assert np.array_equal(_bits(eff), want.view(np.int32)), (n, policy, p)
                if p == 1.0:
                    assert np.array_equal(_bits(eff), _bits(rows))
                if p == 0.0:
                    assert np.array_equal(_bits(eff)[:, on], np.tile(R.neutral_row(H, W), (n, 1)).view(np.int32)[:, on])
                assert torch.equal(state_d.cpu(), state)      # the gate reads the state


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the sign statistic
# ---------------------------------------------------------------------------------------------------------------------------------
SIGN_SIZES = [1, 63, 64, 65, 1024, 2049]


def _sign_map(n, g):
    """values below 0.5, above 0.5 and exactly 0.5"""
    o = torch.rand(n, generator=g) * 2 - 0.5
    o[torch.rand(n, generator=g) < 0.2] = 0.5
    o[0] = 0.5 if n % 2 else 0.75
    return o


def _sign(L, maps, weights, acc):
    dev = [m.cuda() for m in maps]
    k = len(maps)
    L.check(L.lib.aclgan_ada_sign_multi((C.c_void_p * k)(*[m.data_ptr() for m in dev]), (C.c_int * k)(*[m.numel() for m in maps]),
                                        (C.c_float * k)(*weights), k, C.c_void_p(acc), L.stream_ptr()), "ada_sign_multi")
    torch.cuda.synchronize()


def test_sign_matches_fp64(L):
    """per map: q within 1e-6 of fp64 (a count of +-1 is exact, the division and the product round once each); 13 weighted terms (two
    launches) onto one pair: the fp32 model's bits"""
    g = torch.Generator().manual_seed(11)
    maps = [_sign_map(n, g) for n in SIGN_SIZES]
    for o in maps:
        assert (o < 0.5).any() or o.numel() == 1
        state = torch.zeros(12, device="cuda")
        _sign(L, [o], [1.0], state.data_ptr() + 32)
        got = state.cpu()
        want = R.sign_q(o.numpy())
        print("ada sign n=%d: q %.9g, fp64 %.9g" % (o.numel(), float(got[8]), want))
        assert abs(float(got[8]) - want) <= 1e-6 and float(got[9]) == 1.0
        assert float(got[:8].abs().max()) == 0 and float(got[10:].abs().max()) == 0
    assert any((o == 0.5).sum() > 1 and (o > 0.5).any() and (o < 0.5).any() for o in maps)
    many = [maps[i % len(maps)] for i in range(13)]
    weights = [0.5 if i % 3 else 1.0 for i in range(13)]
    state = torch.zeros(12, device="cuda")
    state[10:12] = torch.tensor([0.125, 2.0])
    _sign(L, many, weights, state.data_ptr() + 40)
    a, b = R.sign_acc((0.125, 2.0), [m.numpy() for m in many], weights)
    got = state.cpu().numpy()
    assert got[10:12].view(np.int32).tolist() == np.array([a, b], dtype=np.float32).view(np.int32).tolist()
    want = 0.125 + sum(w * R.sign_q(m.numpy()) for m, w in zip(many, weights))
    assert abs(float(got[10]) - want) <= 1e-6 * 13


def test_a_nan_map_leaves_p_and_r_t(L):
    state = R.new_state(0.3)
    state[R.R_T] = 0.1
    dev = torch.from_numpy(state.copy()).cuda()
    o = _sign_map(65, torch.Generator().manual_seed(1))
    o[40] = float("nan")
    _sign(L, [_sign_map(64, torch.Generator().manual_seed(2)), o], [1.0, 1.0], dev.data_ptr() + 32)
    assert math.isnan(float(dev[8])) and float(dev[9]) == 2.0
    L.check(L.lib.aclgan_ada_fold(L.ptr(dev), 0.6, 1, 0.5, L.stream_ptr()), "ada_fold")
    got = dev.cpu().numpy()
    state[8:10] = (np.nan, 2.0)
    want = R.fold(state, 0.6, 1, 0.5)
    assert got[R.P] == np.float32(0.3) and got[R.R_T] == np.float32(0.1) and math.isnan(got[R.R])
    assert np.array_equal(got.view(np.int32)[[0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11]], want.view(np.int32)[[0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11]])
    assert R.readout(got)["updates"] == 1 and R.readout(got)["adjustments"] == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the fold
# ---------------------------------------------------------------------------------------------------------------------------------
def test_fold_trajectory_matches_the_float32_model_bit_for_bit(L):
    """interval 2, step 0.4 from p = 0.5, target 0.6: up, clamped at 1, down twice, clamped at 0, and an interval that lands on the target
    exactly -- after every fold the twelve words of the state are the model's; then step 0 over two intervals leaves p bit-identical and
    still publishes r and r_t"""
    hi, lo = torch.full((8,), 0.9), torch.full((8,), 0.1)
    mixed = torch.tensor([0.9, 0.9, 0.9, 0.1])                       # q = 0.5
    third = torch.tensor([0.9, 0.9, 0.1])                            # q = 1/3: a rounded quotient
    updates = [(hi, hi), (hi, mixed), (hi, hi), (hi, hi), (lo, lo), (mixed, lo), (lo, third), (lo, lo), (lo, lo), (lo, lo), (lo, lo), (lo, lo)]
    target, interval, step = 0.6, 2, 0.4
    model = R.new_state(0.5)
    dev = torch.from_numpy(model.copy()).cuda()
    ps = []
    for a, b in updates:
        _sign(L, [a], [1.0], dev.data_ptr() + 32)
        _sign(L, [b], [0.5], dev.data_ptr() + 40)
        model[8:10] = R.sign_acc((0, 0), [a.numpy()], [1.0])
        model[10:12] = R.sign_acc((0, 0), [b.numpy()], [0.5])
        L.check(L.lib.aclgan_ada_fold(L.ptr(dev), target, interval, step, L.stream_ptr()), "ada_fold")
        model = R.fold(model, target, interval, step)
        assert np.array_equal(_bits(dev), model.view(np.int32)), (len(ps), dev.cpu().tolist(), model.tolist())
        ps.append(float(model[R.P]))
    f = np.float32
    assert ps[1] == float(f(0.5) + f(0.4)) and ps[3] == 1.0 and ps[5] == float(f(1.0) - f(0.4)) and ps[7] > 0 and ps[9] == 0.0 and ps[-1] == 0.0
    assert R.readout(model)["updates"] == 12 and R.readout(model)["adjustments"] == 6
    # r_t equal to the target: sgn(0) = 0, p stays, the interval still counts as an adjustment made
    dev[0] = 0.3
    model[0] = 0.3
    for _ in range(2):
        _sign(L, [mixed], [1.0], dev.data_ptr() + 32)
        model[8:10] = R.sign_acc((0, 0), [mixed.numpy()], [1.0])
        L.check(L.lib.aclgan_ada_fold(L.ptr(dev), 0.5, 2, step, L.stream_ptr()), "ada_fold")
        model = R.fold(model, 0.5, 2, step)
    assert np.array_equal(_bits(dev), model.view(np.int32)) and float(dev[0]) == float(f(0.3)) and float(dev[1]) == 0.5
    # a fixed probability
    p0 = _bits(dev)[0]
    for a in (hi, lo, hi, hi):
        _sign(L, [a], [1.0], dev.data_ptr() + 40)
        model[10:12] = R.sign_acc((0, 0), [a.numpy()], [1.0])
        L.check(L.lib.aclgan_ada_fold(L.ptr(dev), target, interval, 0.0, L.stream_ptr()), "ada_fold")
        model = R.fold(model, target, interval, 0.0)
        assert _bits(dev)[0] == p0 and np.array_equal(_bits(dev), model.view(np.int32))
    assert float(dev[R.R]) == 1.0 and float(dev[R.R_T]) == 1.0 and R.readout(model)["updates"] == 18


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the trainer
# ---------------------------------------------------------------------------------------------------------------------------------
POLICY = "color,translation,cutout"
HEADS = [(D, "cnns.%d.4." % s) for D in ("dis_A", "dis_B") for s in range(3)]


def _reduced(norm="none", dim=8):
    cfg = O.default_config()
    cfg["gen"].update(dim=dim, mlp_dim=2 * dim, n_res=2)
    cfg["dis"].update(dim=dim, norm=norm)
    cfg["display_size"] = 1
    cfg["focus_epsilon"] = 0.5
    if norm == "sn":
        from sn_nets import sn_test_nets
        return cfg, sn_test_nets(cfg, 0)
    return cfg, O.test_nets(cfg, 0)


def _cfg(cfg, policy=POLICY, **keys):
    out = copy.deepcopy(cfg)
    out["dis_augment"] = policy
    out.update(keys)
    return out


def _biased(nets, bias):
    """the bias of every scale's 1x1 head of dis_A and dis_B: every output of the real-side discriminators lies on one side of 0.5"""
    out = copy.deepcopy(nets)
    for D, pre in HEADS:
        out[D][pre + "bias"] = torch.full_like(out[D][pre + "bias"], bias)
    return out


def _batch(B, S, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 3, S, S, generator=g) * 2 - 1, torch.rand(B, 3, S, S, generator=g) * 2 - 1,
            [torch.randn(B, 8, 1, 1, generator=g) for _ in range(6)])


def _make(T, cfg, nets, **kw):
    tr = T.aclgan_Trainer(cfg, **kw)
    for name in O.OracleTrainer.NETS:
        getattr(tr, name).load_state_dict(nets[name], strict=False)
    return tr


def _same_weights(L, a, b):
    for grp in (L.GROUP_GEN, L.GROUP_DIS):
        for name, x, y in (("param", a._param, b._param), ("exp_avg", a._m, b._m), ("exp_avg_sq", a._v, b._v)):
            assert torch.equal(x[grp], y[grp]), (grp, name)


def test_p_one_is_the_key_absent_bit_for_bit(T, L):
    """dis_augment_p: 1.0 against the key absent, two dis + gen steps with the trainers' own draws: every parameter and Adam buffer holds the
    same bits (the gate copies every row: u < 1), the 16 losses too, and the monitor has run"""
    cfg, nets = _reduced()
    off_cfg, on_cfg = _cfg(cfg), _cfg(cfg, dis_augment_p=1.0)
    runs = []
    with deterministic_mode(L, True):
        for c in (off_cfg, on_cfg):
            torch.manual_seed(77)
            tr = _make(T, c, nets)
            losses = []
            for step in range(2):
                x_a, x_b, z = _batch(2, 64, 200 + step)
                tr.dis_update(x_a, x_b, c, z=z[:3])
                tr.gen_update(x_a, x_b, c, z=z[3:])
                losses.append([float(getattr(tr, n)) for n in L.LOSS_NAMES])
            torch.cuda.synchronize()
            runs.append((tr, losses))
    (off, loff), (on, lon) = runs
    assert loff == lon
    _same_weights(L, off, on)
    s = on.ada_state()
    assert s["p"] == 1.0 and s["updates"] == 2 and s["adjustments"] == 0 and s["r"] == -1.0 and off.ada is None
    with pytest.raises(L.AclganError, match="dis_augment_p"):
        off.ada_state()


def test_p_zero_is_the_key_absent_with_neutral_rows(T, L):
    cfg, nets = _reduced()
    off_cfg, on_cfg = _cfg(cfg), _cfg(cfg, dis_augment_p=0.0)
    runs = []
    with deterministic_mode(L, True):
        for c in (off_cfg, on_cfg):
            torch.manual_seed(78)
            tr = _make(T, c, nets)
            for step in range(2):
                x_a, x_b, z = _batch(2, 64, 210 + step)
                neutral = tr.ada is None
                tr.dis_update(x_a, x_b, c, z=z[:3], aug=neutral_params(14, 64, 64).float() if neutral else None)
                tr.gen_update(x_a, x_b, c, z=z[3:], aug=neutral_params(10, 64, 64).float() if neutral else None)
            torch.cuda.synchronize()
            runs.append(tr)
    _same_weights(L, runs[0], runs[1])
    assert runs[1].ada_state()["p"] == 0.0


@pytest.mark.parametrize("bias,moves", [(10.0, True), (-10.0, False)])
def test_controller_steered(T, L, bias, moves):
    """every head of dis_A and dis_B biased to +10: r == 1, and after ada_interval updates p == step exactly; biased to -10: r == -1, p stays 0"""
    cfg, nets = _reduced()
    c = _cfg(cfg, dis_augment_p="adaptive", ada_interval=3, ada_kimg=0.05)
    tr = _make(T, c, _biased(nets, bias))
    B = 2
    step = np.float32(3 * B / (0.05 * 1000.0))
    for i in range(3):
        s = tr.ada_state()
        assert s["p"] == 0.0 and s["updates"] == i and s["adjustments"] == 0
        x_a, x_b, z = _batch(B, 64, 220 + i)
        tr.dis_update(x_a, x_b, c, z=z[:3])
        assert tr.ada_state()["r"] == (1.0 if moves else -1.0)
    s = tr.ada_state()
    assert s == {"p": float(step) if moves else 0.0, "r_t": 1.0 if moves else -1.0, "r": 1.0 if moves else -1.0, "updates": 3, "adjustments": 1}
    assert set(s) == {"p", "r_t", "r", "updates", "adjustments"}
    assert tr.ada_log_text() == " ada_p=%.4g ada_rt=%.4g" % (s["p"], s["r_t"])
    tr.gen_update(x_a, x_b, c, z=z[3:])             # a gen_update gates by the same p and folds nothing
    assert tr.ada_state() == s


SIGNAL_SEED = 156      # picked with the fp32 oracle on the CPU: every real-side output of the fixture lies >= 2e-3 from 0.5


def _signal_nets(cfg, nets, x_a, x_b, K=1000.0, quantile=0.7):
    """head weights x K, head biases moved so that 0.5 cuts each real-side map at its 0.7 quantile (fp32 oracle, CPU): maps that straddle 0.5"""
    out = copy.deepcopy(nets)
    for D, x in (("dis_A", x_a), ("dis_B", x_b)):
        for s in range(3):
            out[D]["cnns.%d.4.weight" % s] = out[D]["cnns.%d.4.weight" % s] * K
        for s, o in enumerate(O.dis_forward(out[D], x, cfg["dis"])):
            v = o.flatten().sort().values
            i = min(v.numel() - 1, int(quantile * v.numel()))
            cut = float(v[i - 1] + v[i]) / 2 if i > 0 else float(v[0]) - 0.25
            out[D]["cnns.%d.4.bias" % s] = out[D]["cnns.%d.4.bias" % s] + (0.5 - cut)
    return out


def test_signal_is_the_statistic_of_the_discriminators_own_forward(T, L):
    """policy translation,cutout at p = 0: the first update's discriminators see the input bits, so r after the first dis_update is
    sum(w q) / sum(w) over the maps of dis_A.forward(x_a) and dis_B.forward(x_b) with the pre-update weights (w = 1 per scale)"""
    cfg, nets = _reduced()
    x_a, x_b, z = _batch(2, 64, SIGNAL_SEED)
    c = _cfg(cfg, policy="translation,cutout", dis_augment_p=0.0)
    tr = _make(T, c, _signal_nets(cfg, nets, x_a, x_b))
    outs = [o.cpu() for o in tr.dis_A.forward(x_a)] + [o.cpu() for o in tr.dis_B.forward(x_b)]
    margin = min(float((o - 0.5).abs().min()) for o in outs)
    qs = [R.sign_q(o.numpy()) for o in outs]
    print("ada signal fixture: margin %.3e, q per map %s" % (margin, qs))
    assert margin >= 1e-3, margin                                    # the precondition: asserted, not skipped
    assert len(set(qs)) > 1 and all(abs(q) < 1 for q in qs)          # maps that straddle 0.5
    want = sum(qs) / len(qs)
    tr.dis_update(x_a, x_b, c, z=z[:3])
    s = tr.ada_state()
    print("ada signal: r %.9g, from the forward %.9g" % (s["r"], want))
    assert abs(s["r"] - want) <= 1e-6
    assert s["updates"] == 1 and s["p"] == 0.0


@pytest.mark.parametrize("norm", ["none", "sn"])
def test_launch_counts(T, L, norm):
    """the second iteration of a key-on (p = 1) and a key-off trainer: gen_update launches one kernel more (the gate), dis_update the gate, the
    fold and one sign launch per discriminator pass that has a real-side term -- dis_A and dis_B, and under dis.norm sn dis_A's real side twice"""
    cfg, nets = _reduced(norm)
    counts = {}
    for key, c in (("off", _cfg(cfg)), ("on", _cfg(cfg, dis_augment_p=1.0))):
        tr = _make(T, c, nets)
        for step in range(2):
            x_a, x_b, z = _batch(2, 64, 260 + step)
            n0 = L.lib.aclgan_launch_count()
            tr.dis_update(x_a, x_b, c, z=z[:3])
            n1 = L.lib.aclgan_launch_count()
            tr.gen_update(x_a, x_b, c, z=z[3:])
            n2 = L.lib.aclgan_launch_count()
        torch.cuda.synchronize()
        counts[key] = (n1 - n0, n2 - n1)
    print("ada launches (dis, gen) dis.norm %s: off %s on %s" % (norm, counts["off"], counts["on"]))
    assert counts["on"][1] == counts["off"][1] + 1
    assert counts["on"][0] == counts["off"][0] + 1 + (3 if norm == "sn" else 2) + 1
    assert tr.ada_state()["updates"] == 2 and math.isfinite(tr.ada_state()["r"])


def _tune(L, key, value):
    prev = C.c_int()
    L.check(L.lib.aclgan_tuning(key, value, C.byref(prev)), "aclgan_tuning")
    return prev.value


def _run_steps(T, cfg, nets, steps=4, **kw):
    torch.manual_seed(79)
    tr = _make(T, cfg, nets, **kw)
    trace = []
    for step in range(steps):
        x_a, x_b, z = _batch(2, 64, 230 + step)
        tr.dis_update(x_a, x_b, cfg, z=z[:3])
        tr.gen_update(x_a, x_b, cfg, z=z[3:])
        trace.append((float(tr.loss_dis_total), float(tr.loss_gen_total), tuple(sorted(tr.ada_state().items()))))
    torch.cuda.synchronize()
    return tr, trace, {k: v.detach().clone() for k, v in tr.named_parameters()}


def _same_run(a, b):
    (ta, la, pa), (tb, lb, pb) = a, b
    assert la == lb, (la, lb)
    bad = [k for k in pa if not torch.equal(pa[k], pb[k])]
    assert not bad, bad[:6]
    assert np.array_equal(_bits(ta._ada), _bits(tb._ada))
    s = ta.ada_state()
    assert s["updates"] == len(la) and s["adjustments"] == len(la) // 2 and 0 < s["p"] < 1      # p moved during the run: the gate read it on the device


def _steered(T):
    cfg, nets = _reduced(dim=16)
    return _cfg(cfg, dis_augment_p="adaptive", ada_interval=2, ada_kimg=0.02), _biased(nets, 10.0)


def test_lane_count_does_not_change_a_bit(T, L):
    c, nets = _steered(T)
    prev = _tune(L, b"lanes", 1)
    try:
        with deterministic_mode(L, True):
            one = _run_steps(T, c, nets)
            _tune(L, b"lanes", 3)
            _same_run(one, _run_steps(T, c, nets))
    finally:
        _tune(L, b"lanes", prev)


def test_graph_replay_equals_eager(T, L):
    """hip_graph=True: step 1 runs eagerly, step 2 captures, steps 3 and 4 replay -- with a p that moved in between, read by the eager gate
    before every replay; losses, every parameter and the state's bits equal the eager trainer's"""
    c, nets = _steered(T)
    with deterministic_mode(L, True):
        eager = _run_steps(T, c, nets)
        graph = _run_steps(T, c, nets, hip_graph=True)
    tg = graph[0]
    assert tg.hip_graph, "capture fell back to eager execution"
    assert tg._graphs["gen"]["graph"] is not None and tg._graphs["dis"]["graph"] is not None
    assert tg._graphs["dis"]["key"][-4:] == (tg._ada.data_ptr(), 0.6, 2, 2 * 2 / (0.02 * 1000.0))
    _same_run(eager, graph)


def test_checkpoint_round_trip(T, L, tmp_path):
    """save() writes ada_%08d.pt beside gen_ / dis_ / optimizer.pt; resume() restores the state bit for bit and still picks the gen_ / dis_
    files; without the file it warns and p starts again; a key-off trainer writes no new file"""
    c, nets = _steered(T)
    tr = _make(T, c, nets)
    for step in range(3):
        x_a, x_b, z = _batch(2, 64, 240 + step)
        tr.dis_update(x_a, x_b, c, z=z[:3])
        tr.gen_update(x_a, x_b, c, z=z[3:])
    tr.save(str(tmp_path), 2)
    names = sorted(os.listdir(str(tmp_path)))
    assert names == ["ada_00000003.pt", "dis_00000003.pt", "gen_00000003.pt", "optimizer.pt"]
    sd = torch.load(os.path.join(str(tmp_path), "ada_00000003.pt"))
    assert (sd["target"], sd["interval"], sd["kimg"]) == (0.6, 2, 0.02) and sd["state"].shape == (12,)
    state = tr._ada.clone()
    s = tr.ada_state()
    assert s["updates"] == 3 and s["adjustments"] == 1 and s["p"] > 0 and float(state[3]) == 1.0      # an interval half open
    fresh = T.aclgan_Trainer(c)
    assert fresh.ada_state()["updates"] == 0
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        assert fresh.resume(str(tmp_path), c) == 3
    assert not [w for w in seen if "ada" in str(w.message)]
    assert np.array_equal(_bits(fresh._ada), _bits(state)) and fresh.ada_state() == s
    for k, v in tr.named_parameters():
        assert torch.equal(dict(fresh.named_parameters())[k], v), k
    other_cfg = dict(c, ada_interval=5)
    other = T.aclgan_Trainer(other_cfg)
    with pytest.warns(UserWarning, match="ada_target, ada_interval, ada_kimg"):
        assert other.resume(str(tmp_path), other_cfg) == 3
    assert np.array_equal(_bits(other._ada), _bits(state))
    os.remove(os.path.join(str(tmp_path), "ada_00000003.pt"))
    again = T.aclgan_Trainer(c)
    again._ada.fill_(0.5)
    with pytest.warns(UserWarning, match="ada_00000003.pt not found"):
        assert again.resume(str(tmp_path), c) == 3
    assert float(again._ada.abs().max()) == 0.0 and again.ada_state()["updates"] == 0
    plain_cfg = _cfg(_reduced(dim=16)[0])
    plain = T.aclgan_Trainer(plain_cfg)
    tr.save(str(tmp_path), 2)
    assert plain.resume(str(tmp_path), plain_cfg) == 3
    out = tmp_path / "plain"
    out.mkdir()
    plain.save(str(out), 2)
    assert sorted(os.listdir(str(out))) == ["dis_00000003.pt", "gen_00000003.pt", "optimizer.pt"]


def test_refusals_enqueue_nothing_and_leave_the_trainer_usable(T, L):
    cfg, nets = _reduced()
    c = _cfg(cfg, dis_augment_p=0.5)
    x_a, x_b, z = _batch(2, 64, 250)
    u = torch.rand(14, 4, generator=torch.Generator().manual_seed(4))
    with deterministic_mode(L, True):
        tr = _make(T, c, nets)
        n0 = L.lib.aclgan_launch_count()
        for args, word in (((1.5, 4, 0.0), "target"), ((float("nan"), 4, 0.0), "target"), ((0.6, 0, 0.0), "interval"), ((0.6, 4, -1.0), "step"),
                           ((0.6, 4, float("inf")), "step")):
            assert L.lib.aclgan_ctx_set_ada(tr._ctx, L.ptr(tr._ada), *args) == -1 and word in L.last_error()
        assert L.lib.aclgan_ada_fold(None, 0.6, 4, 0.0, L.stream_ptr()) == -1
        assert L.lib.aclgan_ada_fold(L.ptr(tr._ada), 0.6, 0, 0.0, L.stream_ptr()) == -1
        assert L.lib.aclgan_augment_gate(L.ptr(tr._ada), L.ptr(tr._ada), L.ptr(tr._ada), 1, 64, 64, 8, L.ptr(tr._losses), L.stream_ptr()) == -1
        for bad in (torch.rand(14, 3), torch.rand(13, 4), [0.5] * 14):
            with pytest.raises(L.AclganError, match="aug_u"):
                tr.dis_update(x_a, x_b, c, z=z[:3], aug_u=bad)
        assert L.lib.aclgan_launch_count() == n0
        for bad in ({"dis_augment_p": 1.5}, {"dis_augment_p": "adaptive", "ada_interval": 0}, {"dis_augment_p": 0.5, "dis_augment": ""},
                    {"dis_augment_p": 0.5, "dis_augment": "color,flip"}):
            with pytest.raises(L.AclganError):
                T.aclgan_Trainer(dict(c, **bad))
        with pytest.raises(L.AclganError, match="aug_u"):
            _make(T, _cfg(cfg), nets).dis_update(x_a, x_b, cfg, z=z[:3], aug_u=u)
        # the refused calls changed nothing: the trainer gives the bits of one that never saw them; explicit uniforms are what the gate applies
        torch.manual_seed(80)
        tr.dis_update(x_a, x_b, c, z=z[:3], aug_u=u)
        torch.manual_seed(80)
        fresh = _make(T, c, nets)
        fresh.dis_update(x_a, x_b, c, z=z[:3], aug_u=u)
        assert np.array_equal(_bits(tr._ada), _bits(fresh._ada)) and tr.ada_state()["updates"] == 1
        assert float(tr.loss_dis_total) == float(fresh.loss_dis_total)
        _same_weights(L, tr, fresh)
        rows, eff = tr._aug_dev[("dis", 14)].cpu().numpy(), tr._ada_dev[("dis", 14)][1].cpu().numpy()
        assert np.array_equal(eff.view(np.int32), R.gate(rows, u.numpy(), 0.5, 64, 64, 7).view(np.int32))
        assert not np.array_equal(eff, rows) and not np.array_equal(eff, np.tile(R.neutral_row(64, 64), (14, 1)))
