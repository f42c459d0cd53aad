"""LeCam regularisation of the discriminators on the GPU (csrc/losses.hip: lsgan_lecam_batch_kernel / lecam_fold_kernel; aclgan_ctx_set_lecam;
config keys lecam_lambda / lecam_decay / lecam_start): the operator against fp64 numpy, dis_update against the fp32 oracle with its lsgan
wrapped (tests/lecam_ref.py), the anchor recurrence, the bits before the start, launch counts, lanes and graph replay, fp16, checkpoints
and the error paths.  Run on the GPU box: pytest -m gpu"""
import copy
import ctypes as C
import json
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import aclgan_oracle as O
from diffaug_ref import DIS_BLOCKS, GEN_BLOCKS, oracle_dis_forward
from gpu_util import deterministic_mode, rel_err
from lecam_ref import NETS, class_means, fold, lecam_values, oracle_lsgan

pytestmark = pytest.mark.gpu

# the bounds of the existing LSGAN operator test (tests/test_gpu_ops_misc.py::test_lsgan_loss) for the same quantities: a slot value to
# 1e-5 * max(1, |value|), the gradient map to the project's operator bound.  Measured worst on the MI355X: profiles/lecam_parity.json
SLOT_TOL = 1e-5
TOL = 2e-4
MEASURED = {}      # what this run measured, written to $ACLGAN_LECAM_PARITY_OUT (a JSON file) when that is set


def _record(key, value):
    MEASURED[key] = value
    out = os.environ.get("ACLGAN_LECAM_PARITY_OUT")
    if out:
        worst = {}      # per quantity, over the operator and fold cases recorded so far
        for k, v in MEASURED.items():
            if k.startswith(("operator", "fold")):
                for q, e in v.items():
                    worst[q] = max(worst.get(q, 0.0), e)
        doc = {"device": torch.cuda.get_device_name(0), "bounds": {"loss_slot / lecam_slot / sums / anchors": SLOT_TOL, "d_o": TOL},
               "worst": worst, "cases": MEASURED}
        with open(out, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)


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


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the operator
# ---------------------------------------------------------------------------------------------------------------------------------
S3 = 3
SIZES = [1, 255, 256, 257, 1000]
NTERMS = 13      # one more than LSGAN_MAX_TERMS: two launches


def _terms(seed):
    """13 maps of every size, targets 0 and 1, weights 0.5 and 1, spread over the (discriminator, scale, class) cells of a 3-scale state"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(NTERMS):
        n = SIZES[i % len(SIZES)]
        out.append(dict(o=torch.randn(n, generator=g) * 0.7 + 0.4, n=n, target=float(i % 2), weight=0.5 if (i // 2) % 2 else 1.0,
                        gscale=0.2 if i % 3 else 1.0, D=i % 3, s=(i // 3) % S3))
    out[12].update(D=0, s=0, weight=0.5)      # the cell of term 0 (weight 1), from the second launch: a weighted mean of two terms
    return out


def _fresh_state(seed, count):
    g = torch.Generator().manual_seed(seed)
    st = torch.zeros(18 * S3 + 4)
    st[:6 * S3] = torch.rand(6 * S3, generator=g)
    st[-1:].view(torch.int32).fill_(count)
    return st


def _arr(ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


def _run_operator(L, terms, state, slots, lam, start, with_grad, lscale):
    """aclgan_lsgan_lecam_multi on device copies; returns the gradient maps (or None)"""
    maps = [t["o"].cuda() for t in terms]
    grads = [torch.full((t["n"],), float("nan"), device="cuda") for t in terms] if with_grad else None
    n = len(terms)
    base = state.data_ptr()

    def cell(t, k):
        return (t["D"] * S3 + t["s"]) * 2 + k
    anchor = [base + 4 * cell(t, 1 - int(t["target"])) for t in terms]
    lecam = [base + 4 * (18 * S3 + t["D"]) for t in terms]
    stats = [base + 4 * (6 * S3 + 2 * cell(t, int(t["target"]))) for t in terms]
    L.check(L.lib.aclgan_lsgan_lecam_multi(
        _arr([m.data_ptr() for m in maps]), (C.c_int * n)(*[t["n"] for t in terms]), (C.c_float * n)(*[t["target"] for t in terms]),
        (C.c_float * n)(*[t["weight"] for t in terms]), _arr([slots.data_ptr() + 4 * t["D"] for t in terms]),
        _arr([gr.data_ptr() for gr in grads]) if with_grad else None, (C.c_float * n)(*[t["gscale"] for t in terms]),
        _arr(anchor), _arr(lecam), _arr(stats), n, lam, start, C.c_void_p(base + 4 * (18 * S3 + 3)), L.ptr(lscale), L.stream_ptr()),
        "lsgan_lecam_multi")
    torch.cuda.synchronize()
    return grads


def _numpy_operator(terms, state, slots, lam, start, scale):
    """fp64: (slots, state, gradient maps) after the call"""
    st = state.double().numpy().copy()
    count = int(state[-1:].view(torch.int32).item())
    sl = slots.double().numpy().copy()
    lam_eff = lam if count >= max(start, 1) else 0.0
    grads = []
    anchors = st[:6 * S3].copy()      # read before anything is written
    for t in terms:
        o = t["o"].double().numpy()
        k = int(t["target"])
        cell = (t["D"] * S3 + t["s"]) * 2
        a = anchors[cell + 1 - k]
        w = np.float64(np.float32(t["weight"]))
        gs = np.float64(np.float32(t["gscale"]))
        sl[t["D"]] += w * np.mean((o - k) ** 2)
        if count > 0:
            st[18 * S3 + t["D"]] += w * np.mean((o - a) ** 2)
        st[6 * S3 + 2 * (cell + k)] += w * np.mean(o)
        st[6 * S3 + 2 * (cell + k) + 1] += w
        grads.append(scale * gs * w * (2.0 / o.size) * ((o - k) + lam_eff * (o - a)))
    return sl, st, grads


@pytest.mark.parametrize("count,start", [(0, 0), (3, 5), (5, 5), (1, 0)])
@pytest.mark.parametrize("with_grad", [True, False])
@pytest.mark.parametrize("with_scale", [False, True])
def test_operator_matches_fp64(L, count, start, with_grad, with_scale):
    """13 terms (two launches), n in {1, 255, 256, 257, 1000}: loss slots, lecam slots, the statistics pairs and d_o against fp64 numpy;
    count 0 (no term, lecam slots stay 0), below the start, at the start, and start 0 (which means 1).  With lam_eff == 0 the loss slots
    and d_o are the bits of aclgan_lsgan_loss_multi."""
    lam = 0.7
    terms = _terms(11)
    state0 = _fresh_state(12, count)
    slots0 = torch.full((3,), 0.25)
    lscale = torch.tensor([1024.0], device="cuda") if with_scale else None
    state, slots = state0.cuda(), slots0.cuda()
    grads = _run_operator(L, terms, state, slots, lam, start, with_grad, lscale)
    rsl, rst, rgr = _numpy_operator(terms, state0, slots0, lam, start, 1024.0 if with_scale else 1.0)
    got_st = state.cpu().double().numpy()
    errs = {}
    errs["loss_slot"] = max(abs(float(slots[d]) - rsl[d]) / max(1.0, abs(rsl[d])) for d in range(3))
    errs["lecam_slot"] = max(abs(got_st[18 * S3 + d] - rst[18 * S3 + d]) / max(1.0, abs(rst[18 * S3 + d])) for d in range(3))
    errs["sums"] = max(abs(got_st[i] - rst[i]) / max(1.0, abs(rst[i])) for i in range(6 * S3, 18 * S3))
    if with_grad:
        errs["d_o"] = max(rel_err(gr, torch.from_numpy(r)) for gr, r in zip(grads, rgr))
    for k, v in errs.items():
        print("lecam operator count %d start %d grad %d scale %d: %-10s %.3e" % (count, start, with_grad, with_scale, k, v))
    _record("operator count=%d start=%d grad=%d scale=%d" % (count, start, with_grad, with_scale), errs)
    # the anchors and the count are not the term kernel's to write
    assert torch.equal(state[:6 * S3].cpu(), state0[:6 * S3]) and int(state[-1:].view(torch.int32).item()) == count
    if count == 0:
        assert float(state[18 * S3:18 * S3 + 3].abs().max()) == 0.0
    else:
        assert float(state[18 * S3:18 * S3 + 3].min()) > 0.0
    assert all(errs[k] <= SLOT_TOL for k in ("loss_slot", "lecam_slot", "sums")), errs
    assert not with_grad or errs["d_o"] < TOL, errs
    lam_eff = lam if count >= max(start, 1) else 0.0
    assert (lam_eff == 0.0) == ((count, start) in ((0, 0), (3, 5)))
    # against the plain operator: the same bits while the term is off, other bits (where the anchor is not the target) while it is on
    n = len(terms)
    maps = [t["o"].cuda() for t in terms]
    pslots = slots0.cuda()
    pgrads = [torch.full((t["n"],), float("nan"), device="cuda") for t in terms]
    gsc = [t["gscale"] * (1024.0 if with_scale else 1.0) for t in terms]      # (powers of two: the product is exact)
    L.check(L.lib.aclgan_lsgan_loss_multi(_arr([m.data_ptr() for m in maps]), (C.c_int * n)(*[t["n"] for t in terms]),
                                          (C.c_float * n)(*[t["target"] for t in terms]), (C.c_float * n)(*[t["weight"] for t in terms]),
                                          _arr([pslots.data_ptr() + 4 * t["D"] for t in terms]), _arr([gr.data_ptr() for gr in pgrads]),
                                          (C.c_float * n)(*gsc), n, L.stream_ptr()), "lsgan_loss_multi")
    torch.cuda.synchronize()
    assert torch.equal(pslots, slots), "the loss slots never see the term"
    if with_grad:
        same = [torch.equal(a, b) for a, b in zip(grads, pgrads)]
        assert all(same) if lam_eff == 0.0 else not any(same), same


def test_fold_matches_fp64_and_skips_a_non_finite_mean(L):
    """the fold on a caller-supplied state: copy at count 0, decay * a + (1 - decay) * m later, the sums zeroed, the count advanced; an inf
    planted in one map leaves that anchor -- and only that one -- as it was; a class without a term keeps its anchor"""
    decay = 0.9
    terms = _terms(21)
    for count in (0, 4):
        state0 = _fresh_state(22, count)
        planted = copy.deepcopy(terms)
        planted[4]["o"][0] = float("inf")
        state, slots = state0.cuda(), torch.zeros(3, device="cuda")
        _run_operator(L, planted, state, slots, 0.5, 0, False, None)
        _, rst, _ = _numpy_operator(terms, state0, torch.zeros(3), 0.5, 0, 1.0)
        L.check(L.lib.aclgan_lecam_fold(L.ptr(state), S3, decay, L.stream_ptr()), "lecam_fold")
        torch.cuda.synchronize()
        got = state.cpu()
        assert int(got[-1:].view(torch.int32).item()) == count + 1
        assert float(got[6 * S3:18 * S3].abs().max()) == 0.0
        bad_cell = (planted[4]["D"] * S3 + planted[4]["s"]) * 2 + int(planted[4]["target"])
        seen = set()
        worst = 0.0
        for t in terms:
            seen.add((t["D"] * S3 + t["s"]) * 2 + int(t["target"]))
        assert bad_cell in seen and len(seen) < 6 * S3
        for i in range(6 * S3):
            a0 = float(state0[i])
            if i == bad_cell or i not in seen:
                assert float(got[i]) == a0, (count, i)
                continue
            m = rst[6 * S3 + 2 * i] / rst[6 * S3 + 2 * i + 1]
            want = m if count == 0 else decay * a0 + (1 - decay) * m
            worst = max(worst, abs(float(got[i]) - want) / max(1.0, abs(want)))
        print("lecam fold count %d: worst anchor error %.3e" % (count, worst))
        _record("fold count=%d" % count, {"anchors": worst})
        assert worst <= SLOT_TOL


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. dis_update against the oracle
# ---------------------------------------------------------------------------------------------------------------------------------
DIS_NETS, GEN_NETS = ("dis_A", "dis_B", "dis_2"), ("gen_AB", "gen_BA")
ANCHORS = (0.2, 0.8)


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


def _lecam_cfg(cfg, lam=1.0, decay=0.99, start=0):
    out = copy.deepcopy(cfg)
    out.update(lecam_lambda=lam, lecam_decay=decay, lecam_start=start)
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


def _preset(tr, count=1):
    """anchors (0.2, 0.8) at every scale of every discriminator, `count` updates folded"""
    S = tr.arch.dis_num_scales
    a = tr._lecam[:6 * S].view(3, S, 2)
    a[..., 0] = ANCHORS[0]
    a[..., 1] = ANCHORS[1]
    tr._lecam[-1:].view(torch.int32).fill_(count)


def _oracle_dis(monkeypatch, cfg, nets, x_a, x_b, z, anchors, lam, aug=None, policy=0):
    """one dis_update of the fp32 oracle, lsgan wrapped (anchors / lam: lecam_ref.oracle_lsgan; lam None: unwrapped) and, with rows,
    dis_forward wrapped too"""
    orc = O.OracleTrainer(cfg, nets=nets)
    w = None
    with monkeypatch.context() as m:
        if lam is not None:
            w = oracle_lsgan(O.lsgan, anchors, lam)
            m.setattr(O, "lsgan", w)
        if aug is not None:
            wf = oracle_dis_forward(O.dis_forward, aug, x_a.shape[0], policy, DIS_BLOCKS)
            m.setattr(O, "dis_forward", wf)
        orc.dis_update(x_a, x_b, z[:3], apply=False)
        assert aug is None or len(wf.calls) == len(DIS_BLOCKS)
    assert w is None or len(w.rec["means"]) == 8
    return orc, (w.rec if w is not None else None)


def _check_dis(tr, orc, rec, tag):
    """the bounds of tests/test_gpu_diffaugment.py::_check_against_oracle for losses and gradients; the three lecam values as losses"""
    want = dict(orc.losses)
    if rec is not None:
        want.update({"loss_dis_lecam_" + D: v for D, v in lecam_values(rec).items()})
    for n, v in want.items():
        got = float(getattr(tr, n))
        print("%s %-26s gpu %+.6e oracle %+.6e" % (tag, n, got, v))
        assert abs(got - v) <= 1e-3 * max(1e-3, abs(v)), (tag, n, got, v)
    gmax = max(float(t.grad.norm()) for n in DIS_NETS for t in orc.nets[n].values() if t.grad is not None)
    worst = 0.0
    for n in DIS_NETS:
        for k, gr in getattr(tr, n).named_grads():
            ref = orc.nets[n][k].grad
            err = (gr.cpu().double() - ref.double()).norm().item()
            worst = max(worst, err / (ref.double().norm().item() + 1e-5 * gmax / 3e-2))
            assert err <= 3e-2 * ref.double().norm().item() + 1e-5 * gmax, (tag, n, k, err)
    print("%s dis worst gradient error / bound: %.3e" % (tag, worst / 3e-2))
    return worst / 3e-2


def _oracle_gen(monkeypatch, cfg, nets, x_a, x_b, z, aug=None, policy=0):
    """one gen_update of the fp32 oracle, lsgan as it is; with rows, dis_forward wrapped"""
    orc = O.OracleTrainer(cfg, nets=nets)
    with monkeypatch.context() as m:
        if aug is not None:
            wf = oracle_dis_forward(O.dis_forward, aug, x_a.shape[0], policy, GEN_BLOCKS)
            m.setattr(O, "dis_forward", wf)
        orc.gen_update(x_a, x_b, z[3:], apply=False)
        assert aug is None or len(wf.calls) == len(GEN_BLOCKS)
    return orc


def _check_gen(tr, orc, tag):
    """gen_update: the bounds of tests/test_gpu_diffaugment.py::_check_against_oracle for the twelve losses and the generator gradients"""
    for n, v in orc.losses.items():
        got = float(getattr(tr, n))
        print("%s %-26s gpu %+.6e oracle %+.6e" % (tag, n, got, v))
        assert abs(got - v) <= (5e-3 if n.endswith("_size") else 1e-3) * max(1e-3, abs(v)), (tag, n, got, v)
    gmax = max(float(t.grad.norm()) for n in GEN_NETS for t in orc.nets[n].values())
    worst = 0.0
    for n in GEN_NETS:
        for k, gr in getattr(tr, n).named_grads():
            ref = orc.nets[n][k].grad
            err = (gr.cpu().double() - ref.double()).norm().item()
            worst = max(worst, err / (ref.double().norm().item() + 1e-5 * gmax / 3e-2))
            assert err <= 3e-2 * ref.double().norm().item() + 1e-5 * gmax, (tag, n, k, err)
    print("%s gen worst gradient error / bound: %.3e" % (tag, worst / 3e-2))
    return worst / 3e-2


def _grad_change(a, b):
    num = sum(float((a.nets[n][k].grad.double() - b.nets[n][k].grad.double()).norm() ** 2) for n in DIS_NETS for k in a.nets[n]
              if a.nets[n][k].grad is not None) ** 0.5
    den = sum(float(b.nets[n][k].grad.double().norm() ** 2) for n in DIS_NETS for k in b.nets[n] if b.nets[n][k].grad is not None) ** 0.5
    return num / den


@pytest.mark.parametrize("case", ["none", "sn", "augment"])
def test_dis_update_matches_the_wrapped_oracle(T, L, monkeypatch, case):
    """reduced width, 64x64, B=2, anchors (0.2, 0.8), lam 1, start 0, count 1: the four discriminator losses, the three lecam values and every
    discriminator gradient against the fp32 oracle under the wrapper (with dis.norm sn; with dis_augment translation,cutout and both
    wrappers).  Asserted on the oracle: the term moves the gradient by >= 0.1 relative L2.  Control: a key-off trainer fails.  In every
    case a second key-on trainer with the same preset runs gen_update: its twelve losses and every generator gradient are the UNWRAPPED
    oracle's, and the state tensor keeps its bits -- the key does not reach gen_update."""
    cfg, nets = _reduced("sn" if case == "sn" else "none")
    B, S = 2, 64
    x_a, x_b, z = _batch(B, S, 61)
    aug, policy = None, 0
    if case == "augment":
        cfg["dis_augment"] = "translation,cutout"
        policy = 6
        aug = T.draw_augment_params(policy, 7 * B, S, S, torch.Generator().manual_seed(62))
    anchors = {D: [list(ANCHORS)] * cfg["dis"]["num_scales"] for D in NETS}
    off, _ = _oracle_dis(monkeypatch, cfg, nets, x_a, x_b, z, None, None, aug, policy)
    on, rec = _oracle_dis(monkeypatch, cfg, nets, x_a, x_b, z, anchors, 1.0, aug, policy)
    change = _grad_change(on, off)
    print("lecam %s: the term moves the oracle's discriminator gradient by %.3f (relative L2)" % (case, change))
    assert change >= 0.1
    assert on.losses == off.losses
    cfgl = _lecam_cfg(cfg)
    tr = _make(T, cfgl, nets)
    _preset(tr)
    tr.dis_update(x_a, x_b, cfgl, z=z[:3], aug=aug)
    assert tr.lecam_updates == 2
    worst = _check_dis(tr, on, rec, "lecam " + case)
    # gen_update on a second key-on trainer built from the fixture nets, the term live (count 1 >= start): the twelve generator losses and
    # every generator gradient are the UNWRAPPED oracle's -- the key does not reach gen_update -- and the state is not touched
    aug_g = T.draw_augment_params(policy, 5 * B, S, S, torch.Generator().manual_seed(63)) if case == "augment" else None
    og = _oracle_gen(monkeypatch, cfg, nets, x_a, x_b, z, aug_g, policy)
    trg = _make(T, cfgl, nets)
    _preset(trg)
    before = trg._lecam.clone()
    trg.gen_update(x_a, x_b, cfgl, z=z[3:], aug=aug_g)
    assert len(og.losses) == 12
    worst_g = _check_gen(trg, og, "lecam " + case)
    assert torch.equal(trg._lecam, before) and trg.lecam_updates == 1, "gen_update wrote the LeCam state"
    _record("update " + case, {"gradient error / bound": worst, "oracle gradient change": change, "gen_update gradient error / bound": worst_g})
    # control: the key off against the wrapped oracle fails the gradient comparison
    tro = _make(T, cfg, nets)
    tro.dis_update(x_a, x_b, cfg, z=z[:3], aug=aug)
    assert tro.lecam_updates == 0 and tro._lecam is None
    _check_dis(tro, off, None, "control " + case)
    with pytest.raises(AssertionError):
        _check_dis(tro, on, None, "control " + case + " against the wrapped oracle")


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. anchor dynamics
# ---------------------------------------------------------------------------------------------------------------------------------
def _trainer_nets(tr):
    return {n: {k: v.detach().cpu().clone() for k, v in getattr(tr, n).state_dict().items()} for n in O.OracleTrainer.NETS}


def _grads_of(tr):
    return {(n, k): gr.contiguous().clone() for n in DIS_NETS for k, gr in getattr(tr, n).named_grads()}


def test_anchor_dynamics_over_three_updates(T, L, monkeypatch):
    """three chained dis_updates from a fresh state, decay 0.9, start 0: after each the anchors are the recurrence applied to the means the
    oracle records AT THE TRAINER'S CURRENT PARAMETERS (copy, then decay * a + (1 - decay) * m) to 1e-5 absolute plus relative; the count
    goes 1, 2, 3; update 1 has lam_eff 0 -- its gradients are the bits of a key-off twin -- and update 2 has not"""
    cfg, nets = _reduced()
    decay = 0.9
    cfgl = _lecam_cfg(cfg, lam=1.0, decay=decay, start=0)
    B, S = 2, 64
    with deterministic_mode(L, True):
        tr, twin = _make(T, cfgl, nets), _make(T, cfg, nets)
        anchors = None
        worst = 0.0
        for step in range(3):
            x_a, x_b, z = _batch(B, S, 70 + step)
            now = _trainer_nets(tr)
            _, rec = _oracle_dis(monkeypatch, cfg, now, x_a, x_b, z, anchors, 1.0 if step else 0.0)
            tr.dis_update(x_a, x_b, cfgl, z=z[:3])
            twin.dis_update(x_a, x_b, cfg, z=z[:3])
            assert tr.lecam_updates == step + 1
            anchors = fold(anchors, class_means(rec), step, decay)
            got = tr.lecam_anchors()
            assert sorted(got) == sorted(NETS)
            for D in NETS:
                assert tuple(got[D].shape) == (cfg["dis"]["num_scales"], 2)
                want = torch.tensor(anchors[D], dtype=torch.float64)
                err = ((got[D].cpu().double() - want).abs() / (1.0 + want.abs())).max().item()
                worst = max(worst, err)
                print("lecam dynamics step %d dis_%s: anchors %s, error / (1 + |a|) %.3e" % (step + 1, D, got[D].flatten().tolist(), err))
                assert err <= 1e-5, (step, D, got[D], want)
            vals = lecam_values(rec)
            for D in NETS:
                v = float(getattr(tr, "loss_dis_lecam_" + D))
                assert (v == 0.0 and vals[D] == 0.0) if step == 0 else abs(v - vals[D]) <= 1e-3 * max(1e-3, abs(vals[D])), (step, D, v, vals[D])
            same = all(torch.equal(a, b) for a, b in zip(_grads_of(tr).values(), _grads_of(twin).values()))
            assert same == (step == 0), (step, same)
            if step == 0:
                assert float(tr.loss_dis_total) == float(twin.loss_dis_total)
    _record("dynamics", {"anchors": worst})


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. before the start
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_before_the_start_no_bit_differs(T, L, dtype):
    """lecam_start 10**9, deterministic mode, three dis + gen steps: parameters, Adam state and the 16 losses equal a key-off twin's bit for
    bit, and the anchors are tracked all the same"""
    cfg, nets = _reduced(dim=16)
    cfgl = _lecam_cfg(cfg, lam=1.0, start=10 ** 9)
    B, S = 2, 64
    with deterministic_mode(L, True):
        runs = []
        for c in (cfg, cfgl):
            tr = _make(T, c, nets, compute_dtype=dtype)
            losses = []
            for step in range(3):
                x_a, x_b, z = _batch(B, S, 80 + step)
                tr.dis_update(x_a, x_b, c, z=z[:3])
                tr.gen_update(x_a, x_b, c, z=z[3:])
                losses.append([float(getattr(tr, n)) for n in L.LOSS_NAMES])
            torch.cuda.synchronize()
            runs.append((tr, losses))
    (off, loff), (on, lon) = runs
    assert loff == lon
    for grp in (L.GROUP_GEN, L.GROUP_DIS):
        for name, a, b in (("param", off._param, on._param), ("exp_avg", off._m, on._m), ("exp_avg_sq", off._v, on._v)):
            assert torch.equal(a[grp], b[grp]), (grp, name)
    assert off.lecam_updates == 0 and on.lecam_updates == 3
    a = on.lecam_anchors()
    assert all(float(a[D].abs().min()) > 0 for D in NETS)
    assert all(float(getattr(on, "loss_dis_lecam_" + D)) > 0 for D in NETS)
    assert float(off.loss_dis_lecam_A) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. launches
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", ["none", "sn"])
def test_launch_counts(T, L, norm):
    """the second iteration of a key-on and a key-off trainer: gen_update launches the same number of kernels, dis_update exactly one more
    (the fold; the term kernel replaces the LSGAN kernel one for one)"""
    cfg, nets = _reduced(norm)
    cfgl = _lecam_cfg(cfg)
    B, S = 2, 64
    counts = {}
    for key, c in (("off", cfg), ("on", cfgl)):
        tr = _make(T, c, nets)
        for step in range(2):
            x_a, x_b, z = _batch(B, S, 90 + step)
            n0 = L.lib.aclgan_launch_count()
            tr.dis_update(x_a, x_b, c, z=z[:3])
            n1 = L.lib.aclgan_launch_count()
            tr.gen_update(x_a, x_b, c, z=z[3:])
            n2 = L.lib.aclgan_launch_count()
        torch.cuda.synchronize()
        counts[key] = (n1 - n0, n2 - n1)
    print("lecam launches (dis, gen) dis.norm %s: off %s on %s" % (norm, counts["off"], counts["on"]))
    assert counts["on"][1] == counts["off"][1]
    assert counts["on"][0] == counts["off"][0] + 1


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. lanes and graph replay
# ---------------------------------------------------------------------------------------------------------------------------------
def _tune(L, key, value):
    prev = C.c_int()
    L.check(L.lib.aclgan_tuning(key, value, C.byref(prev)), "aclgan_tuning")
    return prev.value


def _run_steps(T, cfg, nets, steps=4, **kw):
    tr = _make(T, cfg, nets, **kw)
    losses = []
    for step in range(steps):
        x_a, x_b, z = _batch(2, 64, 100 + step)
        tr.dis_update(x_a, x_b, cfg, z=z[:3])
        tr.gen_update(x_a, x_b, cfg, z=z[3:])
        losses.append((float(tr.loss_dis_total), float(tr.loss_gen_total), float(tr.loss_dis_lecam_A), float(tr.loss_dis_lecam_B),
                       float(tr.loss_dis_lecam_2)))
    torch.cuda.synchronize()
    return tr, losses, {k: v.detach().clone() for k, v in tr.named_parameters()}


def _same_run(a, b):
    (ta, la, pa), (tb, lb, pb) = a, b
    assert la == lb, (la, lb)
    bad = [k for k in pa if not torch.equal(pa[k], pb[k])]
    assert not bad, bad[:6]
    assert torch.equal(ta._lecam, tb._lecam)
    assert ta.lecam_updates == len(la) and float(ta._lecam[:6 * ta.arch.dis_num_scales].abs().min()) > 0
    assert len(set(la)) == len(la)


def test_lane_count_does_not_change_a_bit(T, L):
    cfg, nets = _reduced(dim=16)
    cfgl = _lecam_cfg(cfg, decay=0.9)
    prev = _tune(L, b"lanes", 1)
    try:
        with deterministic_mode(L, True):
            one = _run_steps(T, cfgl, nets, steps=3)
            _tune(L, b"lanes", 3)
            _same_run(one, _run_steps(T, cfgl, nets, steps=3))
    finally:
        _tune(L, b"lanes", prev)


def test_graph_replay_equals_eager(T, L):
    """hip_graph=True: step 1 runs eagerly, step 2 captures, steps 3 and 4 replay; losses, lecam values, every parameter and the state
    tensor (anchors, count) equal the eager trainer's bit for bit"""
    cfg, nets = _reduced(dim=16)
    cfgl = _lecam_cfg(cfg, decay=0.9)
    with deterministic_mode(L, True):
        eager = _run_steps(T, cfgl, nets)
        graph = _run_steps(T, cfgl, nets, hip_graph=True)
    tg = graph[0]
    assert tg.hip_graph, "capture fell back to eager execution"
    assert tg._graphs["gen"]["graph"] is not None and tg._graphs["dis"]["graph"] is not None
    assert tg._graphs["dis"]["key"][-4:] == (1.0, 0.9, 0, tg._lecam.data_ptr())
    _same_run(eager, graph)


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. fp16
# ---------------------------------------------------------------------------------------------------------------------------------
def test_fp16_gradients_carry_the_loss_scale_once(T, L):
    """anchors (0.2, 0.8), lam 1, count 1: the fp16 trainer's discriminator gradients divided by grad_scale("dis") against the fp32
    trainer's, per tensor in relative L2 within the fp16 bound of tests/test_gpu_step16.py::test_step_gradients_16bit (GTOL 1.2e-1, floor
    1e-4 of the largest tensor); the lecam values are reported without the scale"""
    cfg, nets = _reduced(dim=16)
    cfgl = _lecam_cfg(cfg)
    x_a, x_b, z = _batch(2, 64, 110)
    out = {}
    for dt in ("fp32", "fp16"):
        tr = _make(T, cfgl, nets, compute_dtype=dt)
        _preset(tr)
        tr.dis_update(x_a, x_b, cfgl, z=z[:3])
        out[dt] = (tr, tr.grad_scale("dis"), _grads_of(tr))
    (t32, s32, g32), (t16, s16, g16) = out["fp32"], out["fp16"]
    assert s32 == 1.0 and s16 == 65536.0
    gmax = max(float(v.double().norm()) for v in g32.values())
    worst = max((g16[k].double() / s16 - g32[k].double()).norm().item() / (g32[k].double().norm().item() + 1e-4 * gmax) for k in g32)
    print("lecam fp16 / S against fp32: worst relative L2 %.3e" % worst)
    _record("fp16", {"gradient relative L2": worst})
    assert worst <= 1.2e-1
    for D in NETS:
        a, b = float(getattr(t16, "loss_dis_lecam_" + D)), float(getattr(t32, "loss_dis_lecam_" + D))
        assert abs(a - b) <= 1e-2 * abs(b), (D, a, b)
    assert t16.loss_scale_state()["skipped_dis"] == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. checkpoints
# ---------------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip(T, L, tmp_path):
    """save() writes lecam_%08d.pt beside gen_ / dis_ / optimizer.pt; resume() restores anchors and count bit for bit and still picks the
    gen_ / dis_ files; without the file it warns and the anchors start again"""
    cfg, nets = _reduced()
    cfgl = _lecam_cfg(cfg, decay=0.9)
    tr = _make(T, cfgl, nets)
    for step in range(2):
        x_a, x_b, z = _batch(2, 64, 120 + step)
        tr.dis_update(x_a, x_b, cfgl, z=z[:3])
        tr.gen_update(x_a, x_b, cfgl, z=z[3:])
    tr.save(str(tmp_path), 1)
    names = sorted(os.listdir(str(tmp_path)))
    assert names == ["dis_00000002.pt", "gen_00000002.pt", "lecam_00000002.pt", "optimizer.pt"]
    assert not any(("gen" in n or "dis" in n) for n in names if n.startswith("lecam"))
    state = tr._lecam.clone()
    assert tr.lecam_updates == 2
    fresh = T.aclgan_Trainer(cfgl)
    assert fresh.lecam_updates == 0
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        assert fresh.resume(str(tmp_path), cfgl) == 2
    assert not [w for w in seen if "lecam" in str(w.message)]
    assert torch.equal(fresh._lecam, state) and fresh.lecam_updates == 2
    for k, v in tr.named_parameters():
        assert torch.equal(dict(fresh.named_parameters())[k], v), k
    # the resumed trainer continues like the original
    x_a, x_b, z = _batch(2, 64, 130)
    with deterministic_mode(L, True):
        tr.dis_update(x_a, x_b, cfgl, z=z[:3])
        fresh.dis_update(x_a, x_b, cfgl, z=z[:3])
    assert torch.equal(fresh._lecam, tr._lecam) and fresh.lecam_updates == 3
    # anchors saved under one lecam_decay continue under another only with a warning
    cfgd = _lecam_cfg(cfg, decay=0.5)
    other = T.aclgan_Trainer(cfgd)
    with pytest.warns(UserWarning, match="lecam_decay 0.9"):
        assert other.resume(str(tmp_path), cfgd) == 2
    assert torch.equal(other._lecam, state)
    os.remove(os.path.join(str(tmp_path), "lecam_00000002.pt"))
    again = T.aclgan_Trainer(cfgl)
    again._lecam.fill_(1.0)
    with pytest.warns(UserWarning, match="lecam_00000002.pt not found"):
        assert again.resume(str(tmp_path), cfgl) == 2
    assert again.lecam_updates == 0 and float(again._lecam.abs().max()) == 0.0
    # a key-off trainer resumes from a directory that holds the file, and writes none
    plain = T.aclgan_Trainer(cfg)
    tr.save(str(tmp_path), 1)
    assert plain.resume(str(tmp_path), cfg) == 2
    out = tmp_path / "plain"
    out.mkdir()
    plain.save(str(out), 1)
    assert sorted(os.listdir(str(out))) == ["dis_00000002.pt", "gen_00000002.pt", "optimizer.pt"]


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. errors
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing_and_leave_the_trainer_usable(T, L):
    cfg, nets = _reduced()
    cfgl = _lecam_cfg(cfg)
    x_a, x_b, z = _batch(2, 64, 140)
    with deterministic_mode(L, True):
        tr = _make(T, cfgl, nets)
        n0 = L.lib.aclgan_launch_count()
        for args, word in (((-1.0, 0.99, 0), "lambda"), ((float("nan"), 0.99, 0), "lambda"), ((float("inf"), 0.99, 0), "lambda"),
                           ((1.0, 1.0, 0), "decay"), ((1.0, -0.1, 0), "decay"), ((1.0, 0.99, -1), "start")):
            assert L.lib.aclgan_ctx_set_lecam(tr._ctx, args[0], args[1], args[2], L.ptr(tr._lecam)) == -1 and word in L.last_error()
            assert L.lib.aclgan_ctx_set_lecam(tr._ctx, args[0], args[1], args[2], None) == -1
        assert L.lib.aclgan_lecam_fold(None, 3, 0.9, L.stream_ptr()) == -1
        assert L.lib.aclgan_lecam_fold(L.ptr(tr._lecam), 3, 1.0, L.stream_ptr()) == -1
        assert L.lib.aclgan_launch_count() == n0
        for bad in ({"lecam_lambda": -1}, {"lecam_lambda": 1.0, "lecam_decay": 1.0}, {"lecam_lambda": 1.0, "lecam_start": -1}):
            with pytest.raises(L.AclganError):
                T.aclgan_Trainer(dict(cfg, **bad))
        with pytest.raises(L.AclganError, match="lecam_lambda"):
            _make(T, cfg, nets).lecam_anchors()
        # the refused calls changed nothing: the trainer gives the bits of one that never saw them
        tr.dis_update(x_a, x_b, cfgl, z=z[:3])
        fresh = _make(T, cfgl, nets)
        fresh.dis_update(x_a, x_b, cfgl, z=z[:3])
        assert torch.equal(tr._lecam, fresh._lecam) and tr.lecam_updates == 1
        assert all(torch.equal(a, b) for a, b in zip(_grads_of(tr).values(), _grads_of(fresh).values()))
        assert float(tr.loss_dis_total) == float(fresh.loss_dis_total)
