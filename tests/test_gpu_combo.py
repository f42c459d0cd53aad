"""The training keys switched on together, on the GPU, against the composed oracle of tests/combo_ref.py (its fixtures, stacks and the
oracle-side preconditions: tests/test_combo_cpu.py).  Stack A (limited data): dis_augment + dis_augment_p + lecam_lambda + ms_lambda + grad_clip +
ema_decay with dis.norm none and sn; stack B: r1_gamma (which refuses sn and dis_augment) + lecam_lambda + ms_lambda + grad_clip + ema_decay.
  1. one dis_update + adopting gen_update against the oracle, with a control per key;   2. adoption, 3. lanes, 4. graph replay change no bit;
  5. each key stays in its lane;   6. save / resume mid-run;   7. a non-finite batch with everything on;   8. bf16 and fp16.
Every bound is an existing one, cited where it is used.  Measured figures: profiles/combo_parity.json (ACLGAN_COMBO_PARITY_OUT=<file>).
Run on the GPU box: pytest -m gpu"""
import copy
import ctypes as C
import json
import math
import os

import pytest
import torch

from oracle import aclgan_oracle as O
import combo_ref as R
import lecam_ref
from gpu_util import deterministic_mode
from gradclip_ref import norm_f32

pytestmark = pytest.mark.gpu

LTOL, LTOL_SIZE = 1e-3, 5e-3      # tests/test_gpu_step.py: ltol of test_update_steps_match_reference (losses; the *_size losses)
ETOL, EFLOOR = 3e-2, 1e-5         # tests/test_gpu_step.py: ETOL_SMOOTH, per tensor ||got - ref|| <= ETOL ||ref|| + EFLOOR gmax (l2ok)
NORM_BOUND = 1e-5                 # tests/test_gpu_gradclip.py: NORM_BOUND (the streaming reductions)
ANCHOR_BOUND = 1e-5               # tests/test_gpu_lecam.py::test_anchor_dynamics_over_three_updates: |got - want| / (1 + |want|)
ADA_BOUND = 1e-6                  # tests/test_gpu_ada.py::test_signal_is_the_statistic_of_the_discriminators_own_forward
SIGN_MARGIN = 1e-3                # the same test's precondition
FTOL16 = {"bf16": 6e-2, "fp16": 8e-3}       # tests/test_gpu_step16.py: FTOL
GTOL16 = {"bf16": 3e-1, "fp16": 1.2e-1}     # tests/test_gpu_step16.py: GTOL (floor 1e-4 gmax)
LTOL16_DIGIT = {"bf16": 1.5e-2, "fp16": 1.2e-3}
LTOL16_SIZE = {"bf16": 1e-1, "fp16": 1.5e-2}      # tests/test_gpu_step16.py: LTOL_DIGIT, LTOL_SIZE (the focus losses against the fp32 oracle)
GEN, DIS = 0, 1


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
    out = os.environ.get("ACLGAN_COMBO_PARITY_OUT")
    if not out:
        return
    doc = {}
    if os.path.exists(out):
        with open(out) as f:
            doc = json.load(f)
    doc[key] = value
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


def _hits(L):
    v = C.c_longlong()
    L.check(L.lib.aclgan_tuning_get(b"enc_reuse_hits", C.byref(v)))
    return v.value


def _tune(L, key, value):
    prev = C.c_int()
    L.check(L.lib.aclgan_tuning(key, value, C.byref(prev)), "aclgan_tuning")
    return prev.value


def _make(T, cfg, nets, **kw):
    tr = T.aclgan_Trainer(cfg, **kw)
    for name in O.OracleTrainer.NETS:
        getattr(tr, name).load_state_dict(nets[name], strict=False)
    if tr._ema is not None:      # the average starts from the weights the run starts from
        tr.ema_reset()
    return tr


def _preset(tr, count=1):
    """anchors (0.2, 0.8) at every scale of every discriminator, `count` updates folded (tests/test_gpu_lecam.py)"""
    S = tr.arch.dis_num_scales
    a = tr._lecam[:6 * S].view(3, S, 2)
    a[..., 0] = R.ANCHORS[0]
    a[..., 1] = R.ANCHORS[1]
    tr._lecam[-1:].view(torch.int32).fill_(count)


def _trainer_nets(tr):
    return {n: {k: v.detach().cpu().clone() for k, v in getattr(tr, n).state_dict().items()} for n in O.OracleTrainer.NETS}


def _biased(nets, bias):
    """the bias of every scale's 1x1 head of dis_A and dis_B (tests/test_gpu_ada.py): the controller sees r = 1 and moves p every interval"""
    out = copy.deepcopy(nets)
    for D in ("dis_A", "dis_B"):
        for s in range(3):
            out[D]["cnns.%d.4.bias" % s] = torch.full_like(out[D]["cnns.%d.4.bias" % s], bias)
    return out


def _dev(b):
    """the iteration's images on the device, once: dis_update and gen_update then see the same tensor, and gen_update adopts"""
    if "x_a_dev" not in b:
        b["x_a_dev"], b["x_b_dev"] = b["x_a"].cuda(), b["x_b"].cuda()
    return b["x_a_dev"], b["x_b_dev"]


def _dis(tr, cfg, b):
    kw = {}
    if tr.augment:
        kw["aug"] = b["aug_d"]
    if tr._ada is not None:
        kw["aug_u"] = b["u_d"]
    x_a, x_b = _dev(b)
    tr.dis_update(x_a, x_b, cfg, z=b["z"][:3], **kw)


def _gen(tr, cfg, b):
    kw = {}
    if tr.augment:
        kw["aug"] = b["aug_g"]
    if tr._ada is not None:
        kw["aug_u"] = b["u_g"]
    if tr.ms_lambda > 0:
        kw["z_ms"] = b["z_ms"]
    x_a, x_b = _dev(b)
    tr.gen_update(x_a, x_b, cfg, z=b["z"][3:], **kw)


def _grads(tr, names, S=1.0):
    return {(n, k): g.contiguous().cpu().double() / S for n in names for k, g in getattr(tr, n).named_grads()}


def _state(tr, clip=True):
    """everything a run leaves behind, as clones"""
    s = {}
    for grp in (GEN, DIS):
        for name in ("_param", "_m", "_v"):
            s["%s%d" % (name, grp)] = getattr(tr, name)[grp].clone()
        if clip and tr._clip[grp] is not None:
            s["clip%d" % grp] = tr._clip[grp][:8].clone()      # the eight floats a checkpoint carries; the rest is the norm stage's scratch
    for name in ("_ema", "_lecam", "_ada", "_lscale"):
        if getattr(tr, name) is not None:
            s[name] = getattr(tr, name).clone()
    s["_sn_state"] = tr._sn_state.clone()
    return s


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _assert_same(a, b, tag, keys=None):
    keys = sorted(a) if keys is None else keys
    assert keys and set(keys) <= set(a) and set(keys) <= set(b), (tag, sorted(a), sorted(b))
    bad = [k for k in keys if a[k].shape != b[k].shape or not torch.equal(_bits(a[k]), _bits(b[k]))]
    assert not bad, (tag, bad)


def _values(tr):
    """the losses and the keys' extra values of the last iteration, as one tensor"""
    v = [tr._losses.clone()]
    if tr._ms_out is not None:
        v.append(tr._ms_out.clone())
    if tr._lecam is not None:
        s = 18 * tr.arch.dis_num_scales
        v.append(tr._lecam[s:s + 3].clone())
    if tr.r1_gamma > 0:
        v.append(torch.stack([tr.loss_dis_r1_A, tr.loss_dis_r1_B]))
    return torch.cat(v)


def _chain(T, cfg, nets, seeds, before=None, **kw):
    """`len(seeds)` chained iterations on explicit inputs; returns (trainer, state, per-iteration values)"""
    tr = _make(T, cfg, nets, deterministic=True, **kw)
    if before is not None:
        before(tr)
    vals = []
    for seed in seeds:
        b = R.batch(seed)
        _dis(tr, cfg, b)
        _gen(tr, cfg, b)
        vals.append(_values(tr))
    torch.cuda.synchronize()
    st = _state(tr)
    st["values"] = torch.stack(vals)
    return tr, st


def _adaptive(cfg):
    """stack A with the controller on and steered (with _biased nets): p moves by 0.2 after every second dis_update"""
    return R.with_keys(cfg, dis_augment_p="adaptive", ada_interval=2, ada_kimg=0.02)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. one iteration against the composed oracle
# ---------------------------------------------------------------------------------------------------------------------------------
def _check_losses(got, want, tag):
    for n, v in want.items():
        tol = LTOL_SIZE if n.endswith("_size") else LTOL
        print("    %s %-26s gpu %+.6e oracle %+.6e" % (tag, n, got[n], v))
        assert abs(got[n] - v) <= tol * max(1e-3, abs(v)), (tag, n, got[n], v)


def _grad_ratio(got, ref, tag):
    """the worst of ||got - ref|| / (ETOL ||ref|| + EFLOOR gmax) over the tensors, and its tensor; the two sides hold the same tensors"""
    assert set(got) == set(ref), (tag, sorted(set(got) ^ set(ref))[:6])
    gmax = max(float(t.double().norm()) for t in ref.values())
    worst = (0.0, None)
    for k in sorted(ref):
        r = ref[k].double()
        worst = max(worst, (float((got[k] - r).norm()) / (ETOL * float(r.norm()) + EFLOOR * gmax), k))
    return worst


def _check_grads(got, ref, tag):
    """per tensor ||got - ref|| <= ETOL ||ref|| + EFLOOR gmax; returns the worst error / bound"""
    worst, k = _grad_ratio(got, ref, tag)
    assert worst <= 1.0, (tag, k, worst)
    return worst


def _group_norm(ref):
    return sum(float(t.double().norm() ** 2) for t in ref.values()) ** 0.5


def _check_norm(got, buf, st, ref, tag):
    """a published grad_norm_* against gradclip_ref.norm_f32 of the trainer's own buffer `buf` (NORM_BOUND) and against the oracle gradient's
    norm (ETOL); `st` is the group's clip state after the update: clipped, not skipped"""
    own = norm_f32(buf)[0]
    want = _group_norm(ref)
    print("    %s grad_norm %.7g, of its buffer %.7g, of the oracle's gradient %.7g" % (tag, got, own, want))
    assert abs(got - own) <= NORM_BOUND * own, (tag, got, own)
    assert abs(got - want) <= ETOL * want, (tag, got, want)
    assert st["norm"] == got and st["clipped"] == 1 and st["skipped"] == 0 and 0 < st["coef"] < 1, (tag, st)


_ITER = {}


def _one_iteration(T, L, case):
    """the full-stack trainer's iteration and the oracle's, at the trainer's parameters before each update (computed once per case)"""
    if case in _ITER:
        return _ITER[case]
    cfg, nets, b = R.case(*case)
    tr = _make(T, cfg, nets)
    _preset(tr)
    h0 = _hits(L)
    nets_d = _trainer_nets(tr)
    _dis(tr, cfg, b)
    out = {"cfg": cfg, "nets_d": nets_d, "b": b, "tr": tr}
    out["losses_d"] = {n: float(getattr(tr, n)) for n in L.LOSS_NAMES[12:16]}
    out["lecam"] = {D: float(getattr(tr, "loss_dis_lecam_" + D)) for D in lecam_ref.NETS}
    out["r1"] = {"A": float(tr.loss_dis_r1_A), "B": float(tr.loss_dis_r1_B)}
    out["grads_d"] = _grads(tr, R.DIS_NETS)
    out["norm_d"] = (float(tr.grad_norm_dis), tr._grad[DIS].cpu(), tr.grad_clip_state()["dis"])
    out["anchors"] = {D: a.cpu().double() for D, a in tr.lecam_anchors().items()}
    out["ada"] = tr.ada_state() if tr._ada is not None else None
    out["nets_g"] = nets_g = _trainer_nets(tr)
    _gen(tr, cfg, b)
    torch.cuda.synchronize()
    out["hits"] = _hits(L) - h0
    out["losses_g"] = {n: float(getattr(tr, n)) for n in L.LOSS_NAMES[0:12]}
    out["ms"] = {"ms_B": float(tr.loss_gen_ms_B), "div_B": float(tr.gen_diversity_B), "ms_A": float(tr.loss_gen_ms_A), "div_A": float(tr.gen_diversity_A)}
    out["grads_g"] = _grads(tr, R.GEN_NETS)
    out["oracle"] = R.iteration(cfg, nets_d, nets_g, b)
    _ITER[case] = out
    return out


@pytest.mark.parametrize("case", R.CASES, ids=["-".join(c) for c in R.CASES])
def test_one_iteration_matches_the_composed_oracle(T, L, case):
    """dis_update, then gen_update on the same device tensors (it adopts the encodings: enc_reuse_hits moves by 2), anchors preset to (0.2, 0.8)
    with one update folded: the 16 losses, the lecam / mode-seeking / R1 values, every gradient tensor of both groups, both published norms,
    the anchors after the fold and ADA's r, each against the composed fp32 oracle evaluated at the trainer's parameters before that update"""
    tag = "-".join(case)
    it = _one_iteration(T, L, case)
    tr, orc, cfg = it["tr"], it["oracle"], it["cfg"]
    assert it["hits"] == 2, "gen_update did not adopt dis_update's encodings"
    od, og = orc["dis"], orc["gen"]
    assert od["calls"]["dis_forward"] == od["calls"]["lsgan"] == 8 and og["calls"]["dis_forward"] == 5
    # dis_update
    _check_losses(it["losses_d"], od["losses"], tag)
    _check_losses({"lecam_" + D: v for D, v in it["lecam"].items()}, {"lecam_" + D: v for D, v in od["lecam"].items()}, tag)
    if case[0] == "B":
        _check_losses({"r1_" + D: v for D, v in it["r1"].items()}, {"r1_" + D: v for D, v in od["r1"].items()}, tag)
        assert tr.r1_passes == 1
    worst_d = _check_grads(it["grads_d"], od["grads"], tag + " dis")
    # gen_update
    assert len(og["losses"]) == (12 if case[2] == "focus" else 6)
    _check_losses(it["losses_g"], og["losses"], tag)
    _check_losses(it["ms"], og["ms"], tag)
    worst_g = _check_grads(it["grads_g"], og["grads"], tag + " gen")
    print("combo %s: worst gradient error / bound dis %.3f gen %.3f" % (tag, worst_d, worst_g))
    # the norm stage behind the composed gradients: every update is clipped
    _check_norm(*it["norm_d"], od["grads"], tag + " dis")
    _check_norm(float(tr.grad_norm_gen), tr._grad[GEN].cpu(), tr.grad_clip_state()["gen"], og["grads"], tag + " gen")
    assert tr.ema_updates == 1 and not torch.equal(tr._ema, tr._param[GEN])
    # the anchors after the fold
    want_a = lecam_ref.fold(R.preset_anchors(cfg), od["class_means"], 1, cfg["lecam_decay"])
    worst_a = 0.0
    for D in lecam_ref.NETS:
        w = torch.tensor(want_a[D], dtype=torch.float64)
        err = float(((it["anchors"][D] - w).abs() / (1.0 + w.abs())).max())
        worst_a = max(worst_a, err)
        assert err <= ANCHOR_BOUND, (tag, D, it["anchors"][D], w)
    assert tr.lecam_updates == 2
    rec = {"gradient error / bound": {"dis": worst_d, "gen": worst_g}, "anchor error": worst_a}
    # ADA's signal with the gated augmentation applied
    if case[0] == "A":
        r, margin = R.sign_r(od["real_outs"])
        assert margin >= SIGN_MARGIN and abs(r) < 1, (tag, r, margin)      # the precondition, on the oracle's side
        print("    %s ada r %.9g oracle %.9g (margin %.3e)" % (tag, it["ada"]["r"], r, margin))
        assert abs(it["ada"]["r"] - r) <= ADA_BOUND, (tag, it["ada"], r)
        assert it["ada"]["updates"] == 1 and it["ada"]["p"] == 0.5
        rec["sign fixture"] = {"r": r, "margin": margin}
    else:
        assert it["ada"] is None
    _record("one_iteration " + tag, rec)


@pytest.mark.parametrize("case", R.CASES, ids=["-".join(c) for c in R.CASES])
def test_one_key_off_fails_the_comparison(T, L, case):
    """the control of test 1: the same update with one key of the stack off -- every key that acts on that update, in turn -- fails the
    gradient comparison against the full oracle; a gen_update control starts from the parameters the full trainer's gen_update started from"""
    tag = "-".join(case)
    it = _one_iteration(T, L, case)
    cfg, b, orc = it["cfg"], it["b"], it["oracle"]
    margins = {}
    for which, start, names in (("dis", it["nets_d"], R.DIS_NETS), ("gen", it["nets_g"], R.GEN_NETS)):
        for key in R.ACTS_ON[case[0]][which]:
            c = R.drop_key(cfg, key)
            tr = _make(T, c, start)
            if tr._lecam is not None:
                _preset(tr)
            (_dis if which == "dis" else _gen)(tr, c, b)
            worst, k = _grad_ratio(_grads(tr, names), orc[which]["grads"], "%s control without %s" % (tag, key))
            print("combo %s: %s_update without %s: worst gradient error / bound %.1f (%s)" % (tag, which, key, worst, k))
            margins["%s without %s" % (which, key)] = worst
            assert worst > 1.0, (tag, which, key, worst)
    _record("controls " + tag, margins)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. adoption, 3. lanes: no bit changes with the stack on
# ---------------------------------------------------------------------------------------------------------------------------------
SEEDS = (510, 511, 512, 513)


def _steered_case(norm="none", dim=8):
    cfg, nets, _ = R.case("A", norm, "focus", dim)
    return _adaptive(cfg), _biased(nets, 10.0)


@pytest.fixture(scope="module")
def chain_a(T, L):
    """stack A, adaptive and steered, three chained iterations in deterministic mode, adopting: the run tests 2, 5 and 7 compare against"""
    cfg, nets = _steered_case()
    with deterministic_mode(L, True):
        h0 = _hits(L)
        tr, st = _chain(T, cfg, nets, SEEDS[:3])
        hits = _hits(L) - h0
    return cfg, nets, tr, st, hits


def test_adoption_changes_no_bit(T, L, chain_a):
    """enc_reuse: false against the default over three chained iterations of stack A: every parameter, Adam buffer, the average, the lecam /
    ada / clip states and all values hold the same bits; the default run adopted in every gen_update, the other in none"""
    cfg, nets, tr, st, hits = chain_a
    assert hits == 6
    with deterministic_mode(L, True):
        h0 = _hits(L)
        tr2, st2 = _chain(T, R.with_keys(cfg, enc_reuse=False), nets, SEEDS[:3])
        assert _hits(L) == h0
    _assert_same(st, st2, "enc_reuse")
    s = tr.ada_state()
    assert s["updates"] == 3 and s["adjustments"] == 1 and 0 < s["p"] < 1      # p moved during the run
    for k in ("gen", "dis"):
        assert tr.grad_clip_state()[k]["clipped"] == 3 and tr.grad_clip_state()[k]["skipped"] == 0
    assert float(st["values"][:, [16, 17, 20, 21]].abs().min()) > 0                                     # ms_B, div_B, ms_A, div_A of every iteration
    assert tr.lecam_updates == 3 and float(st["values"][0, 24:].abs().max()) == 0 and float(st["values"][1:, 24:].min()) > 0      # no anchors in update 1


def test_lane_count_does_not_change_a_bit(T, L):
    cfg, nets = _steered_case()
    prev = _tune(L, b"lanes", 1)
    try:
        with deterministic_mode(L, True):
            _, one = _chain(T, cfg, nets, SEEDS[:2])
            _tune(L, b"lanes", 3)
            _, three = _chain(T, cfg, nets, SEEDS[:2])
    finally:
        _tune(L, b"lanes", prev)
    _assert_same(one, three, "lanes")


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. graph replay
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", ["none", "sn"])
def test_graph_replay_equals_eager(T, L, norm):
    """stack A, adaptive and steered, dim 16 and a fresh batch per step (the setting of tests/test_gpu_graph.py): step 1 runs eagerly, step 2
    captures, steps 3 and 4 replay with a p that moved after step 2; every state tensor and value equals the eager trainer's bit for bit"""
    cfg, nets = _steered_case(norm, dim=16)
    with deterministic_mode(L, True):
        te, eager = _chain(T, cfg, nets, SEEDS)
        tg, graph = _chain(T, cfg, nets, SEEDS, hip_graph=True)
    assert tg.hip_graph, "capture fell back to eager execution"
    assert tg._graphs["gen"]["graph"] is not None and tg._graphs["dis"]["graph"] is not None
    _assert_same(eager, graph, "graph " + norm)
    s = te.ada_state()
    assert s["updates"] == 4 and s["adjustments"] == 2 and 0 < s["p"] < 1
    assert len({tuple(v.tolist()) for v in eager["values"]}) == 4
    if norm == "sn":
        assert float(eager["_sn_state"].abs().max()) > 0


def _l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_graph_replay_stack_b_within_the_eager_order_spread(T, L):
    """stack B under hip_graph (tests/test_gpu_r1.py section 6): a replayed update zeroes the buffer itself, so the R1 pass follows it where the
    eager trainer runs the pass first.  With the eager order swapped too (_r1_after) the two agree bit for bit; in their own orders they differ
    by no more than 4 x the eager trainer's own spread between the two orders (the form of that module's ORDER_TOL).  The bound has no floor
    on purpose: where the two eager orders give the same bits -- a spread of exactly 0, which is what this shape gives in deterministic mode
    (profiles/combo_parity.json) -- the replayed run has to give them as well, and the test is then a bitwise one"""
    cfg, nets, _ = R.case("B", "none", "focus", 16)

    def after(tr):
        tr._r1_after = True
    with deterministic_mode(L, True):
        te, e = _chain(T, cfg, nets, SEEDS[:3])
        ta, a = _chain(T, cfg, nets, SEEDS[:3], before=after)
        tg, g = _chain(T, cfg, nets, SEEDS[:3], before=after, hip_graph=True)
    assert tg.hip_graph and tg._graphs["dis"]["graph"] is not None and tg._graphs["gen"]["graph"] is not None
    assert te.r1_passes == ta.r1_passes == tg.r1_passes == 3
    _assert_same(a, g, "graph B, same order")
    th_keys = ("_param0", "_param1", "_ema", "_lecam")
    spread = max(_l2(a[k], e[k]) for k in th_keys)
    with deterministic_mode(L, True):
        th, h = _chain(T, cfg, nets, SEEDS[:3], hip_graph=True)
    got = max(_l2(h[k], e[k]) for k in th_keys)
    print("combo stack B: hip_graph vs eager %.3e; eager order spread %.3e" % (got, spread))
    _record("graph stack B", {"graph_vs_eager": got, "eager_order_spread": spread})
    assert got <= 4 * spread


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. each key stays in its lane
# ---------------------------------------------------------------------------------------------------------------------------------
def _single(T, cfg, nets, b, which):
    """one update of a fresh trainer with preset anchors: (its gradient buffers, its values, its state)"""
    tr = _make(T, cfg, nets, deterministic=True)
    if tr._lecam is not None:
        _preset(tr)
    (_dis if which == "dis" else _gen)(tr, cfg, b)
    torch.cuda.synchronize()
    return {"grad0": tr._grad[GEN].clone(), "grad1": tr._grad[DIS].clone(), "losses": tr._losses.clone()}, _state(tr, clip=False), tr


def test_each_key_stays_in_its_lane(T, L, chain_a):
    """stack A in deterministic mode with one key dropped, bits against the full stack: ms_lambda leaves the first dis_update alone (gradients,
    losses, every state); lecam_lambda leaves a gen_update alone; grad_clip .inf in place of the bound leaves every gradient, loss and non-clip
    state of an update alone except what Adam wrote with the clipped step; ema_decay leaves the live parameters of a whole chained run alone"""
    cfg, nets, b = R.case("A", "none", "focus")
    with deterministic_mode(L, True):
        full = {w: _single(T, cfg, nets, b, w) for w in ("dis", "gen")}
        g, s, _ = _single(T, R.drop_key(cfg, "ms_lambda"), nets, b, "dis")
        _assert_same(full["dis"][0], g, "ms_lambda / dis_update")
        _assert_same(full["dis"][1], s, "ms_lambda / dis_update state")
        g, s, tr = _single(T, R.drop_key(cfg, "lecam_lambda"), nets, b, "gen")
        assert tr._lecam is None
        _assert_same(full["gen"][0], g, "lecam_lambda / gen_update")
        _assert_same({k: v for k, v in full["gen"][1].items() if k != "_lecam"}, s, "lecam_lambda / gen_update state")
        for which, grp in (("dis", DIS), ("gen", GEN)):
            g, s, tr = _single(T, R.with_keys(cfg, grad_clip=float("inf")), nets, b, which)
            _assert_same(full[which][0], g, "grad_clip inf / " + which)
            wrote = ["_param%d" % grp, "_m%d" % grp, "_v%d" % grp] + (["_ema"] if grp == GEN else [])
            _assert_same(full[which][1], s, "grad_clip inf / %s state" % which, [k for k in s if k not in wrote])
            assert not torch.equal(full[which][1]["_param%d" % grp], s["_param%d" % grp])      # the bound did clip
            st = tr.grad_clip_state()["gen" if grp == GEN else "dis"]
            assert st["coef"] == 1.0 and st["clipped"] == 0 and full[which][2].grad_clip_state()["gen" if grp == GEN else "dis"]["clipped"] == 1
        # ema_decay: the chained, adaptive run
        ccfg, cnets, _, st, _ = chain_a
        tr2, st2 = _chain(T, R.drop_key(ccfg, "ema_decay"), cnets, SEEDS[:3])
    assert tr2._ema is None and "_ema" in st
    _assert_same({k: v for k, v in st.items() if k != "_ema"}, st2, "ema_decay")


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. save / resume mid-run
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stack", ["A", "B"])
def test_save_resume_mid_run(T, L, tmp_path, stack):
    """two iterations, save, a cold trainer resumes, two more on explicit inputs: every state tensor and value equals the uninterrupted run's
    bit for bit -- lecam, ada, clip, the average and (stack B with r1_every 2: passes at the discriminator updates 1 and 3) the lazy-R1 count"""
    if stack == "A":
        cfg, nets = _steered_case()
    else:
        cfg, nets, _ = R.case("B", "none", "focus")
        cfg = R.with_keys(cfg, r1_every=2)
    with deterministic_mode(L, True):
        whole, want = _chain(T, cfg, nets, SEEDS)
        first, _ = _chain(T, cfg, nets, SEEDS[:2])
        first.save(str(tmp_path), 1)
        cold = T.aclgan_Trainer(cfg, deterministic=True)
        assert cold.resume(str(tmp_path), cfg) == 2
        _assert_same(_state(first), _state(cold), "resume " + stack)
        vals = []
        for seed in SEEDS[2:]:
            b = R.batch(seed)
            _dis(cold, cfg, b)
            _gen(cold, cfg, b)
            vals.append(_values(cold))
        torch.cuda.synchronize()
    got = _state(cold)
    got["values"] = torch.cat([want["values"][:2], torch.stack(vals)])
    _assert_same(want, got, "save / resume " + stack)
    assert cold._opt[DIS]["steps"] == whole._opt[DIS]["steps"] == 4 and cold._opt[GEN]["steps"] == 4
    if stack == "A":
        assert cold.ada_state() == whole.ada_state() and whole.ada_state()["adjustments"] == 2
    else:
        assert whole.r1_passes == 2 and cold.r1_passes == 1
    assert cold.grad_clip_state() == whole.grad_clip_state() and whole.grad_clip_state()["dis"]["clipped"] == 4


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. a non-finite batch with everything on
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_a_non_finite_batch_leaves_no_trace(T, L, dtype):
    """stack A (p fixed at 0.5), three iterations, one NaN pixel in x_a at iteration 2.  Both updates of that iteration are skipped -- by the
    clip stage in fp32, by the loss-scale machine in fp16 (the clip counters then stay) -- and parameters, Adam buffers, the average, the anchors
    and ADA's p and interval sums keep their bits across it.  Iteration 3 then gives, bit for bit, what a run of iterations 1 and 3 alone gives:
    tests/gradclip_ref.py's rule, bias-correction step = host step - skips, makes its Adam steps the same (fp16: that run's loss scale is halved by
    hand where the overflows halved it)"""
    cfg, nets, _ = R.case("A", "none", "focus") if dtype == "fp32" else R.case16()      # (fp16: the fixture that does not overflow by itself)
    batches = [R.batch(s) for s in SEEDS[:3]]
    batches[1]["x_a"][1, 2, 17, 40] = float("nan")
    keep = ("_param0", "_param1", "_m0", "_m1", "_v0", "_v1", "_ema")
    with deterministic_mode(L, True):
        tr = _make(T, cfg, nets, deterministic=True, compute_dtype=dtype)
        ref = _make(T, cfg, nets, deterministic=True, compute_dtype=dtype)
        for i, b in enumerate(batches):
            before = _state(tr)
            _dis(tr, cfg, b)
            _gen(tr, cfg, b)
            if i != 1:
                _dis(ref, cfg, b)
                _gen(ref, cfg, b)
                continue
            torch.cuda.synchronize()
            after = _state(tr)
            _assert_same(before, after, "across the NaN iteration (%s)" % dtype, list(keep))
            S = tr.arch.dis_num_scales
            assert torch.equal(_bits(before["_lecam"][:6 * S]), _bits(after["_lecam"][:6 * S])), "the anchors moved"
            assert torch.equal(_bits(before["_ada"][:4]), _bits(after["_ada"][:4])), "p, r_t or the interval sums moved"
            assert math.isnan(tr.ada_state()["r"]) and tr.ada_state()["updates"] == 2
            clip, ls = tr.grad_clip_state(), tr.loss_scale_state()
            if dtype == "fp32":
                assert clip["gen"]["skipped"] == clip["dis"]["skipped"] == 1 and clip["gen"]["coef"] == clip["dis"]["coef"] == 0.0
            else:
                assert clip["gen"]["skipped"] == clip["dis"]["skipped"] == 0 and ls["skipped_gen"] == ls["skipped_dis"] == 1
                assert ls["scale"] == 65536.0 / 4
                ref._lscale[0:2].copy_(tr._lscale[0:2])      # the scale and its reciprocal, as the two overflows left them
            assert clip["gen"]["clipped"] == clip["dis"]["clipped"] == 1
        torch.cuda.synchronize()
    assert tr._opt[GEN]["steps"] == 3 and ref._opt[GEN]["steps"] == 2
    got, want = _state(tr, clip=False), _state(ref, clip=False)
    _assert_same(got, want, "iteration 3 (%s)" % dtype, list(keep))
    S = tr.arch.dis_num_scales
    assert torch.equal(_bits(got["_lecam"][:6 * S]), _bits(want["_lecam"][:6 * S]))
    assert torch.equal(_bits(tr._losses), _bits(ref._losses)) and torch.equal(_bits(tr._ms_out), _bits(ref._ms_out))
    assert math.isfinite(float(tr.loss_gen_total)) and tr.grad_clip_state()["gen"]["clipped"] == 2


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. 16-bit compute
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_update_16bit(T, L, dt):
    """stack A on the 16-bit fixture (tests/combo_ref.py: case16), one iteration in bf16 and fp16 (loss scale 65536) against the fp32 composed
    oracle: the 16 losses within FTOL (LTOL_DIGIT / LTOL_SIZE for the focus losses), the lecam and mode-seeking values within FTOL (means over maps whose
    elements sit within FTOL of the oracle's), every gradient tensor within GTOL; grad_norm_* is in true gradient units;
    fp16 at twice the loss scale gives the same unscaled gradients, as tests/test_gpu_modeseek.py::test_update_16bit checks"""
    cfg, nets, b = R.case16()

    def run(c):
        tr = _make(T, c, nets, compute_dtype=dt)
        _preset(tr)
        nets_d = _trainer_nets(tr)
        Sd = tr.grad_scale("dis")
        _dis(tr, c, b)
        gd = _grads(tr, R.DIS_NETS, tr.grad_scale("dis"))
        lec = {D: float(getattr(tr, "loss_dis_lecam_" + D)) for D in lecam_ref.NETS}
        losses = {n: float(getattr(tr, n)) for n in L.LOSS_NAMES[12:16]}
        nd = float(tr.grad_norm_dis)
        nets_g = _trainer_nets(tr)
        _gen(tr, c, b)
        torch.cuda.synchronize()
        losses.update({n: float(getattr(tr, n)) for n in L.LOSS_NAMES[0:12]})
        gg = _grads(tr, R.GEN_NETS, tr.grad_scale("gen"))
        return tr, Sd, nets_d, nets_g, gd, gg, lec, nd, losses
    tr, S, nets_d, nets_g, gd, gg, lec, nd, losses = run(cfg)
    assert S == (65536.0 if dt == "fp16" else 1.0)
    orc = R.iteration(cfg, nets_d, nets_g, b)
    want = dict(orc["dis"]["losses"], **orc["gen"]["losses"])
    assert len(want) == 16
    errs = {}
    # the 16 losses, in true units.  The adversarial, identity and total losses at FTOL, like the lecam values below: they are the same means of
    # squares over discriminator maps.  tests/test_gpu_step16.py's LTOL (1e-3 / 1e-4) is a figure measured with the unscaled fill, whose
    # discriminator outputs barely depend on their input; on this fixture (weights x 10) the adversarial losses sit 1.8e-3 (bf16) and 2.4e-4
    # (fp16) from the fp32 oracle, the others within LTOL.  The ill-conditioned *_size / *_digit losses keep that module's bounds for them.
    for n, v in want.items():
        tol = LTOL16_SIZE[dt] if "_size" in n else (LTOL16_DIGIT[dt] if "_digit" in n else FTOL16[dt])
        errs[n] = (abs(losses[n] - v) / max(1e-3, abs(v)), tol, losses[n], v)
        print("    %s %-26s hip %+.6e fp32 oracle %+.6e rel %.2e (bound %.1e)" % (dt, n, losses[n], v, errs[n][0], tol))
    bad = {k: e for k, e in errs.items() if not e[0] <= e[1]}
    assert not bad, bad
    ms = {"ms_B": float(tr.loss_gen_ms_B), "div_B": float(tr.gen_diversity_B), "ms_A": float(tr.loss_gen_ms_A), "div_A": float(tr.gen_diversity_A)}
    for got, want in ((lec, orc["dis"]["lecam"]), (ms, orc["gen"]["ms"])):
        for k, v in want.items():
            print("    %s %s: hip %.6g fp32 oracle %.6g rel %.2e" % (dt, k, got[k], v, abs(got[k] - v) / abs(v)))
            assert abs(got[k] - v) <= FTOL16[dt] * abs(v), (k, got[k], v)
    worst = {}
    for name, got, ref, norm in (("dis", gd, orc["dis"]["grads"], nd), ("gen", gg, orc["gen"]["grads"], float(tr.grad_norm_gen))):
        gmax = max(float(t.double().norm()) for t in ref.values())
        assert all(bool(torch.isfinite(t).all()) for t in got.values()), (name, "non-finite gradients: the update overflowed")
        errs = sorted(((float((got[k] - ref[k].double()).norm()) / (float(ref[k].double().norm()) + 1e-4 * gmax), k) for k in ref), reverse=True)
        print("combo %s %s worst gradient tensors vs the fp32 oracle (relative L2):" % (dt, name), [("%.2e" % e, k) for e, k in errs[:3]])
        worst[name] = errs[0][0]
        assert errs[0][0] <= GTOL16[dt], errs[:6]      # (tests/test_gpu_step16.py: test_step_gradients_16bit)
        want = _group_norm(ref)
        assert abs(norm - want) <= GTOL16[dt] * want, (name, norm, want)      # true gradient units: no loss scale in it
    _record("16bit " + dt, {"gradient relative L2": worst})
    if dt == "fp16":
        st = tr.loss_scale_state()
        assert st["skipped_gen"] == 0 and st["skipped_dis"] == 0
        tr2, S2, _, _, gd2, gg2, _, nd2, _ = run(R.with_keys(cfg, loss_scale_init=2 * 65536.0))
        assert S2 == 2 * 65536.0 and tr2.loss_scale_state()["skipped_gen"] == 0 and tr2.loss_scale_state()["skipped_dis"] == 0
        for got2, got, ref in ((gd2, gd, orc["dis"]["grads"]), (gg2, gg, orc["gen"]["grads"])):
            gmax = max(float(t.double().norm()) for t in ref.values())
            w2 = max(float((got2[k] - got[k]).norm()) / (float(ref[k].double().norm()) + 1e-4 * gmax) for k in ref)
            assert w2 <= GTOL16[dt], w2
        assert abs(nd2 - nd) <= GTOL16[dt] * nd
