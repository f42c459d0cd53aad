"""Whole updates of the HIP path against the oracle at the nine architectures of tests/arch_space.py: every axis aclgan_ctx_create admits
moved off the value all other tests use (dis.dim 12 / 48 / 96, n_layer 1..3, num_scales 2 / 4 / 5, n_downsample 1 / 3, style_dim 5,
gen.dim 128).  The oracle is pinned to the reference at the same architectures by tests/test_oracle_arch_space_cpu.py.
Every bound is an existing bound of this project applied to a new architecture; each test names its origin.  Run with -s for the measured
errors (profiles/arch_space.md)."""
import copy
import json
import os

import pytest
import torch

from oracle import aclgan_oracle as O

import arch_space as A
from conftest import GOLDEN
from gpu_util import deterministic_mode
from lecam_ref import NETS as LC_NETS, class_means, fold, lecam_values, oracle_lsgan

pytestmark = pytest.mark.gpu

DIS_NETS, GEN_NETS = ("dis_A", "dis_B", "dis_2"), ("gen_AB", "gen_BA")
META = json.load(open(os.path.join(GOLDEN, "arch_space.json")))


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available()
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def T(L):
    from aclgan_amd import trainer
    return trainer


def _make(T, cfg, nets, **kw):
    tr = T.aclgan_Trainer(cfg, **kw)
    for name in O.OracleTrainer.NETS:
        getattr(tr, name).load_state_dict(nets[name], strict=False)
    return tr


def _rel(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


_ORACLE = {}


def _oracle(name):
    """the fp32 oracle of one architecture, computed once per module and left unchanged: config, weights, inputs, the forward tensors, and
    losses and gradients of one dis_update and one gen_update from the same weights"""
    if name not in _ORACLE:
        cfg = A.arch_config(name)
        nets = O.test_nets(cfg, A.NET_SEED)
        x_a, x_b, z = A.arch_inputs(name)
        with torch.no_grad():
            fw = dict(O.generator_forward(nets["gen_AB"], nets["gen_BA"], x_a, x_b, z[:3], cfg, with_recon=False))
            fw["dec_AB_c1_z1"] = O.decode(nets["gen_AB"], fw["c_1"], z[0], cfg["gen"])
            fw["dec_BA_c2_z2"] = O.decode(nets["gen_BA"], fw["c_2"], cfg["alpha"] * z[1], cfg["gen"])
            for s, o in enumerate(O.dis_forward(nets["dis_A"], fw["x_A_fake"], cfg["dis"])):
                fw["dis_A_xA_s%d" % s] = o
            for s, o in enumerate(O.dis_forward(nets["dis_2"], fw["pair_A2"], cfg["dis"])):
                fw["dis_2_pA2_s%d" % s] = o
        od = O.OracleTrainer(cfg, nets=nets); od.dis_update(x_a, x_b, z[:3], apply=False)
        og = O.OracleTrainer(cfg, nets=nets); og.gen_update(x_a, x_b, z[3:], apply=False)
        _ORACLE[name] = dict(cfg=cfg, nets=nets, x_a=x_a, x_b=x_b, z=z, fw=fw, od=od, og=og)
    return _ORACLE[name]


def _check_update(trd, trg, od, og, tag):
    """exactly the assertions of tests/test_gpu_step.py::test_non_square_odd_batch_step_matches_oracle: losses 1e-3 relative (5e-3 for the
    focus *_size losses), every parameter gradient within 3e-2 ||ref|| + 1e-5 gmax.  No tensor is skipped."""
    worst_l = 0.0
    for n, v in list(od.losses.items()) + list(og.losses.items()):
        got = float(getattr(trd if n.startswith("loss_dis") else trg, n))
        tol = 5e-3 if n.endswith("_size") else 1e-3
        worst_l = max(worst_l, abs(got - v) / max(1e-3, abs(v)) / tol)
        assert abs(got - v) <= tol * max(1e-3, abs(v)), (tag, n, got, v)
    worst = (0.0, None)
    for tr, orc, nets_ in ((trd, od, DIS_NETS), (trg, og, GEN_NETS)):
        gmax = max(float(t.grad.norm()) for n in nets_ for t in orc.nets[n].values() if t.grad is not None)
        seen = 0
        for n in nets_:
            for k, gr in getattr(tr, n).named_grads():
                ref = orc.nets[n][k].grad
                err = (gr.cpu().double() - ref.double()).norm().item()
                worst = max(worst, (err / (3e-2 * ref.double().norm().item() + 1e-5 * gmax), (n, k)))
                assert err <= 3e-2 * ref.double().norm().item() + 1e-5 * gmax, (tag, n, k, err)
                seen += 1
        assert seen == sum(1 for n in nets_ for k in orc.nets[n] if not O.is_sn_state(k)), (tag, seen)
    print("arch_space %-24s worst loss error / bound %.3f, worst gradient error / bound %.3f at %s" % (tag, worst_l, worst[0], worst[1]))


def _forward(tr, o):
    cfg, x_a, z = o["cfg"], o["x_a"].cuda(), [t.cuda() for t in o["z"]]
    out = {}
    out["c_1"], _ = tr.gen_AB.encode(x_a)
    out["c_2"], out["s_2"] = tr.gen_BA.encode(x_a)
    out["dec_AB_c1_z1"] = tr.gen_AB.decode(out["c_1"], z[0])
    out["dec_BA_c2_z2"] = tr.gen_BA.decode(out["c_2"], cfg["alpha"] * z[1])
    xB4, xA4 = out["dec_AB_c1_z1"], out["dec_BA_c2_z2"]
    out["x_B_fake"] = tr.focus_translation(xB4[:, :3], x_a, xB4[:, 3:])
    out["x_A_fake"] = tr.focus_translation(xA4[:, :3], x_a, xA4[:, 3:])
    out["c_3"], _ = tr.gen_BA.encode(out["x_B_fake"])
    xA24 = tr.gen_BA.decode(out["c_3"], z[2])
    out["x_A2_fake"] = tr.focus_translation(xA24[:, :3], out["x_B_fake"], xA24[:, 3:])
    dA = tr.dis_A(out["x_A_fake"])
    d2 = tr.dis_2(torch.cat((x_a, out["x_A2_fake"]), 1))
    assert len(dA) == len(d2) == cfg["dis"]["num_scales"]
    for s in range(len(dA)):
        out["dis_A_xA_s%d" % s] = dA[s]
        out["dis_2_pA2_s%d" % s] = d2[s]
    return out


def _grads(tr, nets_):
    return {(n, k): g.contiguous().clone() for n in nets_ for k, g in getattr(tr, n).named_grads()}


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) fp32, per architecture: forward tensors and both updates, default and deterministic plan
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(A.ARCHS))
def test_forward_matches_oracle_and_reference(T, name):
    """the tensors of tests/test_gpu_step.py::test_forward_matches_reference at its bound: _rel < 1e-3 against the fp32 oracle's tensor, and
    the norm within 1e-3 of the fp64 reference's (tests/golden/arch_space.json)"""
    o = _oracle(name)
    got = _forward(_make(T, o["cfg"], o["nets"]), o)
    stats = META[name]["fwd_stats"]
    assert sorted(got) == sorted(stats)
    worst = (0.0, None)
    for k, t in got.items():
        assert list(t.shape) == stats[k]["shape"], (name, k, t.shape)
        e = _rel(t, o["fw"][k])
        worst = max(worst, (e, k))
        assert e < 1e-3, (name, k, e)
        nrm = stats[k]["stats"][1]
        assert abs(float(t.double().norm()) - nrm) <= 1e-3 * nrm, (name, k)
    print("arch_space %-24s forward worst max-abs / max|ref| %.3e at %s" % (name, worst[0], worst[1]))


@pytest.mark.parametrize("name", list(A.ARCHS))
def test_updates_match_oracle(T, name):
    o = _oracle(name)
    trd = _make(T, o["cfg"], o["nets"]); trd.dis_update(o["x_a"], o["x_b"], o["cfg"], z=o["z"][:3])
    trg = _make(T, o["cfg"], o["nets"]); trg.gen_update(o["x_a"], o["x_b"], o["cfg"], z=o["z"][3:])
    _check_update(trd, trg, o["od"], o["og"], name)


@pytest.mark.parametrize("name", list(A.ARCHS))
def test_updates_match_oracle_deterministic_and_repeat_bit_for_bit(T, L, name):
    o = _oracle(name)
    prev = L.lib.aclgan_get_deterministic()
    try:
        runs = []
        for rep in range(2):
            trd = _make(T, o["cfg"], o["nets"], deterministic=True); trd.dis_update(o["x_a"], o["x_b"], o["cfg"], z=o["z"][:3])
            trg = _make(T, o["cfg"], o["nets"], deterministic=True); trg.gen_update(o["x_a"], o["x_b"], o["cfg"], z=o["z"][3:])
            assert trd.deterministic and trg.deterministic
            if rep == 0:
                _check_update(trd, trg, o["od"], o["og"], name + " deterministic")
            losses = {n: float(getattr(trd if n.startswith("loss_dis") else trg, n)) for n in list(o["od"].losses) + list(o["og"].losses)}
            runs.append((losses, _grads(trd, DIS_NETS), _grads(trg, GEN_NETS)))
    finally:
        L.check(L.lib.aclgan_set_deterministic(prev))
    (la, da, ga), (lb, db, gb) = runs
    assert la == lb, {k: (la[k], lb[k]) for k in la if la[k] != lb[k]}
    bad = [k for k in da if not torch.equal(da[k], db[k])] + [k for k in ga if not torch.equal(ga[k], gb[k])]
    assert not bad, (name, bad[:8])


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) 16-bit: forward tensors and losses against the fp32 oracle and the emulated contract
# ---------------------------------------------------------------------------------------------------------------------------------
# tests/test_gpu_step16.py's dtype-level bounds (its X2_DIST was measured at other architectures and is not used here)
from test_gpu_step16 import ETOL_F, ETOL_S2, FTOL, LTOL, LTOL_DIGIT, LTOL_SIZE  # noqa: E402

_EMULATED = {}


def _emulated(name, dt):
    """forward tensors of O.compute_dtype(dt), the CPU restatement of the 16-bit contract, once per (architecture, dtype)"""
    if (name, dt) not in _EMULATED:
        o = _oracle(name)
        with torch.no_grad(), O.compute_dtype(dt):
            _, _, fe = O.gen_losses(o["nets"], o["x_a"], o["x_b"], o["z"][3:], o["cfg"])
            fe = dict(fe)
            fe["dis_A"] = O.dis_forward(o["nets"]["dis_A"], fe["x_A_fake"], o["cfg"]["dis"])
        _EMULATED[(name, dt)] = fe
    return _EMULATED[(name, dt)]


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["dis48_l3_s2", "dis96", "gen128"])
def test_forward_and_losses_16bit(T, name, dt):
    """tests/test_gpu_step16.py::test_forward_and_losses_16bit at dis48_l3_s2 (the 48 -> 96 layer is ineligible, between 16-bit-stored
    neighbours), dis96 (96 -> 192 -> 384 on the 16-bit kernels) and gen128 (512-channel ResBlocks)"""
    o = _oracle(name)
    cfg, nets, x_a, x_b, z = o["cfg"], o["nets"], o["x_a"], o["x_b"], o["z"]
    with torch.no_grad():
        _, Lg, fw = O.gen_losses(nets, x_a, x_b, z[3:], cfg)
        _, Ld, _ = O.dis_losses(nets, x_a, x_b, z[:3], cfg)
        dA = O.dis_forward(nets["dis_A"], fw["x_A_fake"], cfg["dis"])
    fe = _emulated(name, dt)
    tr = _make(T, cfg, nets, compute_dtype=dt)
    xa = x_a.cuda()
    zz = [t.cuda() for t in z[3:]]
    worst, worst_e = {}, {}

    def chk(key, got):
        worst[key] = _rel(got, fw[key]); worst_e[key] = _rel(got, fe[key])

    c1, _ = tr.gen_AB.encode(xa); chk("c_1", c1)
    c2, s2 = tr.gen_BA.encode(xa); chk("c_2", c2); chk("s_2", s2)
    xB4 = tr.gen_AB.decode(c1, zz[0])
    xB = tr.focus_translation(xB4[:, :3], xa, xB4[:, 3:]); chk("x_B_fake", xB)
    chk("f_B", xB4[:, 3:])
    rec = tr.gen_BA.decode(c2, s2); chk("x_A_recon", rec[:, :3])
    c3, _ = tr.gen_BA.encode(xB); chk("c_3", c3)
    xA24 = tr.gen_BA.decode(c3, zz[2])
    xA2 = tr.focus_translation(xA24[:, :3], xB, xA24[:, 3:]); chk("x_A2_fake", xA2)
    xA4 = tr.gen_BA.decode(c2, cfg["alpha"] * zz[1])
    xA = tr.focus_translation(xA4[:, :3], xa, xA4[:, 3:])
    got_d = tr.dis_A(xA)
    assert len(got_d) == cfg["dis"]["num_scales"]
    for s, (g_, w_, e_) in enumerate(zip(got_d, dA, fe["dis_A"])):
        worst["dis_A_xA_s%d" % s] = _rel(g_, w_); worst_e["dis_A_xA_s%d" % s] = _rel(g_, e_)
    for what, d in (("fp32 oracle", worst), ("emulated contract", worst_e)):
        print("arch_space %s %s forward vs %s: worst %.2e at %s, s_2 %.2e" % (name, dt, what, max(d.values()), max(d, key=d.get), d["s_2"]))
    bad = {k: v for k, v in worst.items() if not v < (max(FTOL[dt], ETOL_F[dt]) if k == "x_A2_fake" else FTOL[dt])}
    assert not bad, bad
    bad = {k: v for k, v in worst_e.items() if not v < ETOL_F[dt]}
    assert not bad, ("emulated", bad)
    assert worst_e["s_2"] < ETOL_S2[dt], ("emulated s_2", worst_e["s_2"])
    tr.dis_update(x_a, x_b, cfg, z=z[:3])
    ld = {n: float(getattr(tr, n)) for n in Ld}
    tr2 = _make(T, cfg, nets, compute_dtype=dt)
    tr2.gen_update(x_a, x_b, cfg, z=z[3:])
    lg = {n: float(getattr(tr2, n)) for n in Lg}
    errs = {}
    for n, v in list(Ld.items()) + list(Lg.items()):
        v = float(v)
        got = ld[n] if n in ld else lg[n]
        tol = LTOL_SIZE[dt] if "_size" in n else (LTOL_DIGIT[dt] if "_digit" in n else LTOL[dt])
        errs[n] = (abs(got - v) / max(1e-3, abs(v)), tol, got, v)
    wk = max(errs, key=lambda k: errs[k][0] / errs[k][1])
    print("arch_space %s %s losses: worst error / bound %.3f at %s (%.2e)" % (name, dt, errs[wk][0] / errs[wk][1], wk, errs[wk][0]))
    bad = {k: e for k, e in errs.items() if not e[0] <= e[1]}
    assert not bad, bad


# per network group, masks and signs frozen, against the emulated contract
from test_gpu_maskfrozen import ETOL_FROZEN, _grad_errors, _hip_update_with_masks, _match, _per_net  # noqa: E402


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["dis48_l3_s2", "dis96", "gen128"])
def test_backward_parity_with_frozen_masks_16bit(T, L, name, dt):
    """tests/test_gpu_maskfrozen.py::test_backward_parity_with_frozen_masks_16bit at its bounds: the HIP update records the activation masks
    and loss signs it ran with, the emulated 16-bit contract replays the update with those, and every gradient tensor is compared per
    network group"""
    o = _oracle(name)
    cfg, nets, x_a, x_b, z = o["cfg"], o["nets"], o["x_a"], o["x_b"], o["z"]
    B = x_a.shape[0]
    scale = 65536.0 if dt == "fp16" else 1.0
    det = L.lib.aclgan_get_deterministic() == 1

    def contract():
        return O.compute_dtype(dt, loss_scale=scale, up5_dgrad="plain" if det else "merged")

    worst = {}
    for which, zs, nets_ in (("dis", slice(0, 3), DIS_NETS), ("gen", slice(3, 6), GEN_NETS)):
        tr = _make(T, cfg, nets, compute_dtype=dt)
        assert tr.grad_scale() == scale
        chunks, signs = _hip_update_with_masks(tr, which, x_a, x_b, cfg, z[zs], B, 1 << 28)
        assert chunks and len(signs) == (5 if which == "gen" else 0)
        if dt == "fp16":
            st = tr.loss_scale_state()
            assert st["skipped_gen"] == 0 and st["skipped_dis"] == 0 and st["scale"] == scale, (which, st)
        with contract(), O.act_masks() as rec, torch.no_grad():      # the oracle's own masks, from the loss graph alone
            (O.dis_losses if which == "dis" else O.gen_losses)(nets, x_a, x_b, z[zs], cfg)
        replay, flips, total, unmatched = _match(rec.recorded, chunks, stride=1)      # (every element: gen128 runs at B = 1, its coarsest masks hold 64)
        with contract(), O.act_masks(replay, dict(enumerate(signs))) as rec2:
            frozen = O.OracleTrainer(cfg, nets=nets)
            (frozen.dis_update if which == "dis" else frozen.gen_update)(x_a, x_b, z[zs], apply=False)
        assert len(rec2.recorded) == len(rec.recorded)
        errs = _grad_errors(tr, frozen, nets_, scale)
        print("arch_space %s %s %s_update: %d of %d oracle activations matched (%d recorded chunks), %d of %d mask elements differ; worst %.2e at %s"
              % (name, dt, which, len(replay), len(rec.recorded), len(chunks), flips, total, errs[0][0], errs[0][1:]))
        for key, e in _per_net(errs).items():
            kk = "dis" if key.startswith("dis") else "gen" + key[key.index("."):]
            worst[kk] = max(worst.get(kk, 0.0), e)
    print("arch_space %s %s frozen-mask worst per network group:" % (name, dt), {k: "%.2e" % v for k, v in worst.items()})
    bad = {k: v for k, v in worst.items() if v > ETOL_FROZEN[dt][k]}
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) features whose state is indexed by the architecture
# ---------------------------------------------------------------------------------------------------------------------------------
def _trainer_nets(tr):
    return {n: {k: v.detach().cpu().clone() for k, v in getattr(tr, n).state_dict().items()} for n in O.OracleTrainer.NETS}


def _batch(name, seed):
    return A.arch_inputs(name, seed)


@pytest.mark.parametrize("name", ["scales5_l2", "dis48_l3_s2"])
def test_lecam_three_updates_match_the_wrapped_oracle(T, L, monkeypatch, name):
    """tests/lecam_ref.py and the wrapped-oracle method of tests/test_gpu_lecam.py (test_dis_update_matches_the_wrapped_oracle for losses,
    lecam values and gradients: 1e-3 and 3e-2 ||ref|| + 1e-5 gmax; test_anchor_dynamics_over_three_updates for the anchors: 1e-5 of
    1 + |a|), over three chained updates from a fresh state: the copy, the fold and the live term, at 18 * num_scales state offsets"""
    o = _oracle(name)
    cfg = o["cfg"]
    S = cfg["dis"]["num_scales"]
    decay = 0.9
    cfgl = copy.deepcopy(cfg); cfgl.update(lecam_lambda=1.0, lecam_decay=decay, lecam_start=0)
    with deterministic_mode(L, True):
        tr = _make(T, cfgl, o["nets"])
        assert tr._lecam.numel() > 18 * S
        anchors = None
        for step in range(3):
            x_a, x_b, z = _batch(name, 70 + step)
            orc = O.OracleTrainer(cfg, nets=_trainer_nets(tr))
            with monkeypatch.context() as m:
                w = oracle_lsgan(O.lsgan, anchors, 1.0 if step else 0.0)
                m.setattr(O, "lsgan", w)
                orc.dis_update(x_a, x_b, z[:3], apply=False)
            rec = w.rec
            assert len(rec["means"]) == 8 and all(len(r) == S for r in rec["means"])
            tr.dis_update(x_a, x_b, cfgl, z=z[:3])
            assert tr.lecam_updates == step + 1
            want = dict(orc.losses)
            want.update({"loss_dis_lecam_" + D: v for D, v in lecam_values(rec).items()})
            for n, v in want.items():
                got = float(getattr(tr, n))
                assert abs(got - v) <= 1e-3 * max(1e-3, abs(v)), (name, step, n, got, v)
            gmax = max(float(t.grad.norm()) for n in DIS_NETS for t in orc.nets[n].values())
            worst = 0.0
            for n in DIS_NETS:
                for k, gr in getattr(tr, n).named_grads():
                    ref = orc.nets[n][k].grad
                    err = (gr.cpu().double() - ref.double()).norm().item()
                    worst = max(worst, err / (3e-2 * ref.double().norm().item() + 1e-5 * gmax))
                    assert err <= 3e-2 * ref.double().norm().item() + 1e-5 * gmax, (name, step, n, k, err)
            anchors = fold(anchors, class_means(rec), step, decay)
            got = tr.lecam_anchors()
            assert sorted(got) == sorted(LC_NETS)
            aworst = 0.0
            for D in LC_NETS:
                assert tuple(got[D].shape) == (S, 2)
                wt = torch.tensor(anchors[D], dtype=torch.float64)
                err = ((got[D].cpu().double() - wt).abs() / (1.0 + wt.abs())).max().item()
                aworst = max(aworst, err)
                assert err <= 1e-5, (name, step, D, got[D], wt)
            print("arch_space %-24s lecam update %d: gradient error / bound %.3f, anchors %.3e" % (name, step + 1, worst, aworst))


def _run_steps(T, cfg, nets, batches, **kw):
    tr = _make(T, cfg, nets, **kw)
    losses = []
    for x_a, x_b, z in batches:
        tr.dis_update(x_a, x_b, cfg, z=z[:3])
        tr.gen_update(x_a, x_b, cfg, z=z[3:])
        tr.update_learning_rate()
        losses.append((float(tr.loss_dis_total), float(tr.loss_gen_total)))
    torch.cuda.synchronize()
    return tr, losses, {k: v.detach().clone() for k, v in tr.named_parameters()}


@pytest.mark.parametrize("name", ["down3_style5", "scales5_l2"])
def test_graph_replay_matches_eager(T, L, name):
    """tests/test_gpu_graph.py::test_graph_replay_matches_eager: four steps (eager, capture, two replays), deterministic mode, bit for bit"""
    o = _oracle(name)
    batches = [_batch(name, 31 + i) for i in range(4)]
    prev = L.lib.aclgan_get_deterministic()
    try:
        te, le, pe = _run_steps(T, o["cfg"], o["nets"], batches, deterministic=True)
        tg, lg, pg = _run_steps(T, o["cfg"], o["nets"], batches, deterministic=True, hip_graph=True)
    finally:
        L.check(L.lib.aclgan_set_deterministic(prev))
    assert tg.hip_graph, "capture fell back to eager execution"
    assert tg._graphs["gen"]["graph"] is not None and tg._graphs["dis"]["graph"] is not None
    assert le == lg, (le, lg)
    bad = [k for k in pe if not torch.equal(pe[k], pg[k])]
    assert not bad, bad[:6]


@pytest.mark.parametrize("name", ["down3_style5", "scales4_l3"])
def test_checkpoint_round_trip_with_lecam(T, L, tmp_path, name):
    """save() / resume() with LeCam on: after resume one further dis_update and gen_update give the bits of the uninterrupted run"""
    o = _oracle(name)
    cfgl = copy.deepcopy(o["cfg"]); cfgl.update(lecam_lambda=1.0, lecam_decay=0.9, lecam_start=0)
    with deterministic_mode(L, True):
        tr = _make(T, cfgl, o["nets"])
        for step in range(2):
            x_a, x_b, z = _batch(name, 120 + step)
            tr.dis_update(x_a, x_b, cfgl, z=z[:3])
            tr.gen_update(x_a, x_b, cfgl, z=z[3:])
        tr.save(str(tmp_path), 1)
        assert sorted(os.listdir(str(tmp_path))) == ["dis_00000002.pt", "gen_00000002.pt", "lecam_00000002.pt", "optimizer.pt"]
        fresh = T.aclgan_Trainer(cfgl)
        assert fresh.resume(str(tmp_path), cfgl) == 2
        assert torch.equal(fresh._lecam, tr._lecam) and fresh.lecam_updates == 2
        x_a, x_b, z = _batch(name, 130)
        for t in (tr, fresh):
            t.dis_update(x_a, x_b, cfgl, z=z[:3])
            t.gen_update(x_a, x_b, cfgl, z=z[3:])
    assert torch.equal(fresh._lecam, tr._lecam) and fresh.lecam_updates == 3
    assert tuple(fresh.lecam_anchors()["2"].shape) == (cfgl["dis"]["num_scales"], 2)
    for n in ("loss_dis_total", "loss_gen_total"):
        assert float(getattr(tr, n)) == float(getattr(fresh, n)), n
    want = dict(tr.named_parameters())
    bad = [k for k, v in fresh.named_parameters() if not torch.equal(v, want[k])]
    assert not bad, bad[:6]


def _sn_case(name):
    from sn_nets import sn_test_nets
    o = _oracle(name)
    cfg = copy.deepcopy(o["cfg"]); cfg["dis"]["norm"] = "sn"
    return o, cfg, sn_test_nets(cfg, A.NET_SEED)


@pytest.mark.parametrize("name,layers", [("scales4_l3", 8), ("dis48_l3_s2", 4)])
def test_spectral_norm_updates_match_oracle(T, name, layers):
    """dis.norm sn with num_scales * (n_layer - 1) = 8 and 4 normalised layers per discriminator, one dis_update and one gen_update from
    sn_test_nets against the fp32 oracle at tests/test_gpu_spectral.py::_updates_match_reference's bounds: losses 1e-3 (5e-3 *_size), every
    gradient norm within 1e-2 (+ 1e-5 of the largest), u and v after the update within 1e-5; and elementwise as in _check_update"""
    o, cfg, nets = _sn_case(name)
    x_a, x_b, z = o["x_a"], o["x_b"], o["z"]
    od = O.OracleTrainer(cfg, nets=nets); od.dis_update(x_a, x_b, z[:3], apply=False)
    og = O.OracleTrainer(cfg, nets=nets); og.gen_update(x_a, x_b, z[3:], apply=False)
    trd = _make(T, cfg, nets); trd.dis_update(x_a, x_b, cfg, z=z[:3])
    trg = _make(T, cfg, nets); trg.gen_update(x_a, x_b, cfg, z=z[3:])
    assert len(trd._tensors[T.L.GROUP_SN_STATE]) == 3 * 2 * layers
    _check_update(trd, trg, od, og, name + " sn")
    for tr, orc, nets_ in ((trd, od, DIS_NETS), (trg, og, GEN_NETS)):
        gmax = max(float(t.grad.norm()) for n in nets_ for t in orc.nets[n].values() if t.grad is not None)
        for n in nets_:
            for k, gr in getattr(tr, n).named_grads():
                nrm = float(orc.nets[n][k].grad.double().norm())
                assert abs(float(gr.double().norm()) - nrm) <= 1e-2 * nrm + 1e-5 * gmax, (name, n, k)
        worst, seen = 0.0, 0
        for n in DIS_NETS:
            for k, v in getattr(tr, n).state_dict().items():
                if k.endswith(("weight_u", "weight_v")):
                    ref = orc.nets[n][k]
                    assert not torch.equal(ref, nets[n][k]), (n, k)      # (the call advanced it)
                    err = (v.cpu().double() - ref.double()).abs().max().item()
                    worst = max(worst, err)
                    seen += 1
                    assert err <= 1e-5, (name, n, k, err)
        assert seen == 3 * 2 * layers
        print("arch_space %-24s sn: u / v worst error %.3e over %d vectors" % (name, worst, seen))


def test_spectral_norm_without_normalised_layers_is_norm_none_bit_for_bit(T, L):
    """layer1: n_layer 1 leaves nothing to normalise; dis.norm sn then gives the bits of dis.norm none in deterministic mode"""
    o, cfg, nets = _sn_case("layer1")
    assert not [k for n in DIS_NETS for k in nets[n] if O.is_sn_state(k)]
    with deterministic_mode(L, True):
        out = []
        for c in (cfg, o["cfg"]):
            trd = _make(T, c, nets); trd.dis_update(o["x_a"], o["x_b"], c, z=o["z"][:3])
            trg = _make(T, c, nets); trg.gen_update(o["x_a"], o["x_b"], c, z=o["z"][3:])
            losses = {n: float(getattr(trd if n.startswith("loss_dis") else trg, n)) for n in list(o["od"].losses) + list(o["og"].losses)}
            out.append((losses, _grads(trd, DIS_NETS), _grads(trg, GEN_NETS), trd._param[1].clone(), trg._param[0].clone()))
    (la, da, ga, pda, pga), (lb, db, gb, pdb, pgb) = out
    assert la == lb
    assert not [k for k in da if not torch.equal(da[k], db[k])] and not [k for k in ga if not torch.equal(ga[k], gb[k])]
    assert torch.equal(pda, pdb) and torch.equal(pga, pgb)


# (dis.dim, n_layer, num_scales) -> (seed, separated biases, required LeakyReLU margin of the fp64 oracle): seeds chosen on the CPU as
# tests/test_gpu_r1.py chooses its reduced-width cases (measured margins 7.8e-5 and 2.9e-5), so that no fp32 chain takes another branch than
# the oracle.  dis_cfg(48, 2, 1) with that module's separated biases (factor 4, seed 0) is an ill-conditioned case of the operation itself:
# torch's own fp32 evaluation of the closed form (r1_ref.r1_closed_form on the CPU) is 7.4e-6 / 3.8e-6 from fp64 on the two weight gradients,
# above the bound (the library measured 1.1e-6 / 3.0e-6 there); with the plain fill torch's fp32 is at 8.1e-7 / 6.3e-7, like that module's cases.
R1_CASES = {(12, 3, 2): (5, False, 2e-5), (48, 2, 1): (21, False, 2e-5)}
from test_gpu_r1 import TOL as R1_TOL  # noqa: E402  (4 x that module's MEASURED_REL_ERR)


@pytest.mark.parametrize("case", list(R1_CASES), ids=lambda c: "dis%d_l%d_s%d" % c)
def test_r1_operator_matches_fp64(T, L, case):
    """aclgan_dis_r1 against the fp64 double backward of the definition (tests/r1_ref.py) on dis_A, B = 2, 64x64, at
    tests/test_gpu_r1.py::test_operator_matches_fp64's bound: P, grad_x and every weight gradient"""
    from gpu_util import rel_err
    from r1_ref import dis_cfg, r1_autograd, r1_closed_form, separated_biases
    dim, nl, ns = case
    seed, sep, need = R1_CASES[case]
    dcfg = dis_cfg(dim, nl, ns)
    P = O.seeded_fill(O.dis_param_shapes(3, dcfg), "gaussian", seed)
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(1000 + seed)) * 2 - 1
    if sep:
        P = separated_biases(P, x, dcfg, 4.0, seed)
    gamma = 10.0
    margin = r1_closed_form(P, x.double(), dcfg, gamma)[3]
    assert margin >= need, "precondition: LeakyReLU margin %.2e of the fp64 oracle < %.0e" % (margin, need)
    p_ref, G_ref, g_ref = r1_autograd(P, x.double(), dcfg, gamma)
    cfg = A.arch_config("dis12"); cfg["dis"].update(dim=dim, n_layer=nl, num_scales=ns)
    tr = T.aclgan_Trainer(cfg)
    tr.dis_A.load_state_dict(P, strict=False)
    xd = x.cuda().contiguous()
    nb = L.lib.aclgan_dis_r1_scratch_bytes(tr._ctx, L.NETS["dis_A"], 2, 64, 64)
    assert nb > 0, L.last_error()
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda")
    buf = tr._grad[L.GROUP_DIS]
    buf.fill_(1.5)
    for k, v in tr.dis_A.named_grads():
        if k.endswith("weight"):
            v.zero_()
    pen = torch.full((1,), float("nan"), device="cuda")
    gx = torch.full_like(xd, float("nan"))
    L.check(L.lib.aclgan_dis_r1(tr._ctx, L.NETS["dis_A"], L.ptr(xd), 2, 64, 64, gamma, L.ptr(pen), L.ptr(gx), L.ptr(scratch), L.stream_ptr()), "dis_r1")
    torch.cuda.synchronize()
    grads = {k: v.contiguous().clone() for k, v in tr.dis_A.named_grads()}
    errs = {"P": abs(float(pen) - float(p_ref)) / float(p_ref), "grad_x": rel_err(gx, G_ref)}
    for k, ref in g_ref.items():
        if k.endswith("weight"):
            assert float(ref.abs().max()) > 0
            errs[k] = rel_err(grads[k], ref)
        else:
            assert torch.equal(grads[k], torch.full_like(grads[k], 1.5)), k      # biases untouched
    assert len(errs) == 2 + ns * (nl + 1)
    for k, v in errs.items():
        print("arch_space r1 dis%d_l%d_s%d %-28s rel_err %.3e" % (dim, nl, ns, k, v))
    assert max(errs.values()) <= R1_TOL, {k: v for k, v in errs.items() if v > R1_TOL}


def test_diffaugment_updates_match_the_wrapped_oracle(T, monkeypatch):
    """scales5_l2 with dis_augment color,translation,cutout: both updates against the oracle with dis_forward wrapped by
    tests/diffaug_ref.py (GEN_BLOCKS / DIS_BLOCKS are per call, not per scale), at _check_update's bounds"""
    from diffaug_ref import DIS_BLOCKS, GEN_BLOCKS, oracle_dis_forward
    o = _oracle("scales5_l2")
    cfg = copy.deepcopy(o["cfg"]); cfg["dis_augment"] = "color,translation,cutout"
    policy = 7
    x_a, x_b, z = o["x_a"], o["x_b"], o["z"]
    B, _, H, W = x_a.shape
    aug_d = T.draw_augment_params(policy, 7 * B, H, W, torch.Generator().manual_seed(62))
    aug_g = T.draw_augment_params(policy, 5 * B, H, W, torch.Generator().manual_seed(63))
    orcs = []
    for upd, aug, blocks in (("dis", aug_d, DIS_BLOCKS), ("gen", aug_g, GEN_BLOCKS)):
        orc = O.OracleTrainer(o["cfg"], nets=o["nets"])
        with monkeypatch.context() as m:
            wf = oracle_dis_forward(O.dis_forward, aug, B, policy, blocks)
            m.setattr(O, "dis_forward", wf)
            (orc.dis_update if upd == "dis" else orc.gen_update)(x_a, x_b, z[:3] if upd == "dis" else z[3:], apply=False)
            assert len(wf.calls) == len(blocks)
        orcs.append(orc)
    assert orcs[0].losses != o["od"].losses      # (the rows change what the discriminators see)
    trd = _make(T, cfg, o["nets"]); trd.dis_update(x_a, x_b, cfg, z=z[:3], aug=aug_d)
    trg = _make(T, cfg, o["nets"]); trg.gen_update(x_a, x_b, cfg, z=z[3:], aug=aug_g)
    _check_update(trd, trg, orcs[0], orcs[1], "scales5_l2 diffaugment")


# ---------------------------------------------------------------------------------------------------------------------------------
# (d) refusals: argument checks, produced by the dry run before any launch
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_trainer_usable(T, L):
    def refused(tr, cfg, x_a, x_b, z, words, exc):
        n0 = L.lib.aclgan_launch_count()
        for upd in (tr.dis_update, tr.gen_update):
            with pytest.raises(exc) as e:
                upd(x_a, x_b, cfg, z=z)
            for w in words:
                assert w in str(e.value), (w, str(e.value))
        assert L.lib.aclgan_launch_count() == n0

    def usable(tr, cfg, x_a, x_b, z):
        tr.dis_update(x_a, x_b, cfg, z=z[:3])
        tr.gen_update(x_a, x_b, cfg, z=z[3:])
        assert torch.isfinite(tr.loss_dis_total).item() and torch.isfinite(tr.loss_gen_total).item()

    g = torch.Generator().manual_seed(5)

    def batch(B, H, W, sd):
        return (torch.rand(B, 3, H, W, generator=g) * 2 - 1, torch.rand(B, 3, H, W, generator=g) * 2 - 1,
                [torch.randn(B, sd, 1, 1, generator=g) for _ in range(6)])

    # dis.n_layer 5 given 64x64: scale 2 sees 16x16, its fifth layer a 1x1 map
    cfg = A.arch_config("dis12"); cfg["dis"].update(dim=8, n_layer=5)
    tr = T.aclgan_Trainer(cfg)
    x_a, x_b, z = batch(2, 64, 64, 8)
    refused(tr, cfg, x_a, x_b, z[:3], ("dis.n_layer 5", "H,W>=125"), L.AclganError)
    usable(tr, cfg, *batch(1, 128, 128, 8))
    # down3_style5 given 68x64: not a multiple of 2^n_downsample
    cfg = A.arch_config("down3_style5")
    tr = T.aclgan_Trainer(cfg)
    x_a, x_b, z = batch(2, 68, 64, 5)
    refused(tr, cfg, x_a, x_b, z[:3], ("multiples of 8",), L.AclganError)
    usable(tr, cfg, *batch(2, 64, 72, 5))
    # z of width 8 given to the style_dim 5 trainer
    x_a, x_b, z = batch(2, 64, 72, 8)
    refused(tr, cfg, x_a, x_b, z[:3], ("gen.style_dim 5",), L.AclganError)
    usable(tr, cfg, *batch(2, 64, 72, 5))
