"""The composed oracle of tests/combo_ref.py on the CPU (no GPU, no library): with one key on it returns the bits of that key's own reference
path as its existing test builds it, with none the unwrapped oracle's; every wrapper is exhausted (no call index shifted); and the fixtures
of tests/test_gpu_combo.py see every key of their stack -- switching one off moves the gradient of the group it acts on by >= 0.1 relative
L2 with the other keys on, the clip bound lies below every norm, and no real-side discriminator output lies within 1e-3 of 0.5."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import aclgan_oracle as O
import ada_ref
import combo_ref as R
import lecam_ref
import r1_ref
from diffaug_ref import DIS_BLOCKS, GEN_BLOCKS, oracle_dis_forward
from modeseek_ref import gen_losses_ms

SENSITIVITY = 0.1
POLICY = 7


def _record(key, value):
    """(the oracle-side figures of profiles/combo_parity.json, beside what tests/test_gpu_combo.py writes)"""
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


@pytest.fixture(scope="module")
def plain():
    """the fixture with every key off, both dis.norm"""
    out = {}
    for norm in ("none", "sn"):
        cfg = R.base_config("focus", norm)
        out[norm] = (cfg, R.scaled_nets(cfg, scale=R.WEIGHT_SCALE[norm]), R.batch(R.BATCH_SEED))
    return out


def _same(got, orc, names):
    for n in names:
        for k, t in orc.nets[n].items():
            if not R.is_param(orc.hp, k):
                continue
            ref = t.grad if t.grad is not None else torch.zeros_like(t)
            assert torch.equal(got["grads"][(n, k)], ref), (n, k)
    assert sum(1 for n in names for k in orc.nets[n] if R.is_param(orc.hp, k)) == len(got["grads"])


def _own_path(cfg, nets, b, which, dis_forward=None, lsgan=None):
    """an update of the oracle as the per-key test modules build it: OracleTrainer with the module attributes replaced"""
    orc = O.OracleTrainer(cfg, nets=nets)
    attrs = {k: v for k, v in (("dis_forward", dis_forward), ("lsgan", lsgan)) if v is not None}
    with R.patched(**attrs):
        if which == "dis":
            orc.dis_update(b["x_a"], b["x_b"], b["z"][:3], apply=False)
        else:
            orc.gen_update(b["x_a"], b["x_b"], b["z"][3:], apply=False)
    return orc


@pytest.mark.parametrize("norm", ["none", "sn"])
def test_no_key_is_the_unwrapped_oracle(plain, norm):
    cfg, nets, b = plain[norm]
    before = (O.dis_forward, O.lsgan)
    got = R.iteration(cfg, nets, nets, b)
    assert (O.dis_forward, O.lsgan) == before
    for which, names in (("dis", R.DIS_NETS), ("gen", R.GEN_NETS)):
        orc = _own_path(cfg, nets, b, which)
        _same(got[which], orc, names)
        assert got[which]["losses"] == {k: v for k, v in orc.losses.items() if k in got[which]["losses"]} and got[which]["losses"]
    assert got["dis"]["lecam"] is None and got["dis"]["r1"] is None and got["gen"]["ms"] is None
    assert got["dis"]["calls"] == {"dis_forward": 8, "augment": None, "blocks": 8, "lsgan": 8}


@pytest.mark.parametrize("norm", ["none", "sn"])
@pytest.mark.parametrize("p", [None, 0.5])
def test_augmentation_alone_is_the_wrapped_dis_forward(plain, norm, p):
    """dis_augment (p None) and dis_augment with dis_augment_p: tests/test_gpu_diffaugment.py wraps dis_forward with the rows, tests/test_gpu_ada.py
    gates them with ada_ref.gate first"""
    base, nets, b = plain[norm]
    cfg = R.with_keys(base, dis_augment="color,translation,cutout", **({} if p is None else {"dis_augment_p": p}))
    got = R.iteration(cfg, nets, nets, b)
    for which, names, rows, u, blocks in (("dis", R.DIS_NETS, b["aug_d"], b["u_d"], DIS_BLOCKS), ("gen", R.GEN_NETS, b["aug_g"], b["u_g"], GEN_BLOCKS)):
        if p is not None:
            eff = ada_ref.gate(rows.numpy(), u.numpy(), np.float32(p), R.S, R.S, POLICY)
            assert not np.array_equal(eff, rows.numpy()) and not np.array_equal(eff, np.tile(ada_ref.neutral_row(R.S, R.S), (len(eff), 1)))
            rows = torch.from_numpy(eff)
        wf = oracle_dis_forward(O.dis_forward, rows, R.B, POLICY, blocks)
        orc = _own_path(base, nets, b, which, dis_forward=wf)
        assert len(wf.calls) == len(blocks)
        _same(got[which], orc, names)
        assert got[which]["calls"]["augment"] == got[which]["calls"]["dis_forward"] == len(blocks)
    plain_d = R.iteration(base, nets, nets, b, which=("dis",))["dis"]
    assert R.group_change(got["dis"]["grads"], plain_d["grads"]) >= SENSITIVITY


@pytest.mark.parametrize("count", [0, 1])
def test_lecam_alone_is_the_wrapped_lsgan(plain, count):
    """tests/test_gpu_lecam.py::_oracle_dis; count 0: no anchors yet, no term, the values 0"""
    base, nets, b = plain["none"]
    cfg = R.with_keys(base, lecam_lambda=1.0, lecam_start=0)
    anchors = R.preset_anchors(cfg)
    got = R.iteration(cfg, nets, nets, b, anchors=anchors, lecam_count=count)
    w = lecam_ref.oracle_lsgan(O.lsgan, anchors if count else None, 1.0 if count else 0.0)
    orc = _own_path(base, nets, b, "dis", lsgan=w)
    assert len(w.rec["means"]) == 8 and got["dis"]["calls"]["lsgan"] == 8
    _same(got["dis"], orc, R.DIS_NETS)
    assert got["dis"]["lecam"] == lecam_ref.lecam_values(w.rec) and got["dis"]["class_means"] == lecam_ref.class_means(w.rec)
    assert (sum(got["dis"]["lecam"].values()) > 0) == (count > 0)
    _same(got["gen"], _own_path(base, nets, b, "gen"), R.GEN_NETS)      # the key does not reach gen_update


def test_modeseek_alone_is_gen_losses_ms(plain):
    """tests/modeseek_ref.py::gen_losses_ms with ONE backward of total + lambda (ms_B + ms_A): its bits.  tests/test_gpu_modeseek.py::_oracle adds the
    gradients of two backward passes instead; the sums differ by fp32 rounding only (1e-5 of the group's norm, an fp32 sum of two terms)"""
    base, nets, b = plain["none"]
    cfg = R.with_keys(base, ms_lambda=R.MS_LAMBDA)
    got = R.iteration(cfg, nets, nets, b, which=("gen",))["gen"]
    parts = []
    for which in (0, 1, 2):
        orc = O.OracleTrainer(base, nets=nets)
        total, L, _, ms = gen_losses_ms(orc.nets, b["x_a"], b["x_b"], b["z"][3:], b["z_ms"], base)
        (total, R.MS_LAMBDA * (ms["ms_B"] + ms["ms_A"]), total + R.MS_LAMBDA * (ms["ms_B"] + ms["ms_A"]))[which].backward()
        parts.append(R._grads(orc, R.GEN_NETS))
    for k, t in parts[2].items():
        assert torch.equal(got["grads"][k], t), k
    two = {k: parts[0][k] + parts[1][k] for k in parts[0]}
    assert R.group_change(got["grads"], two) <= 1e-5
    assert got["ms"] == {k: float(v.detach()) for k, v in ms.items()} and got["losses"] == {k: float(v.detach()) for k, v in L.items()}
    assert R.group_change(got["grads"], parts[0]) >= SENSITIVITY


def test_r1_alone_adds_r1_autograd(plain):
    base, nets, b = plain["none"]
    cfg = R.with_keys(base, r1_gamma=R.R1_GAMMA, r1_every=2)
    got = R.iteration(cfg, nets, nets, b, which=("dis",))["dis"]
    orc = _own_path(base, nets, b, "dis")
    for D, x in (("dis_A", b["x_a"]), ("dis_B", b["x_b"])):
        pen, _, g = r1_ref.r1_autograd(nets[D], x, base["dis"], R.R1_GAMMA * 2)
        assert got["r1"][D[-1]] == float(pen) > 0
        for k, t in g.items():
            assert torch.equal(got["grads"][(D, k)], orc.nets[D][k].grad + t), (D, k)
    for k, t in orc.nets["dis_2"].items():
        assert torch.equal(got["grads"][("dis_2", k)], t.grad)
    skipped = R.dis_update(cfg, nets, b["x_a"], b["x_b"], b["z"][:3], r1=False)      # an update between two lazy passes
    _same(skipped, orc, R.DIS_NETS)


_FULL = {}


def _full(case):
    if case not in _FULL:
        cfg, nets, b = R.case16() if case[1] == "16bit" else R.case(*case)
        _FULL[case] = (cfg, nets, b, R.iteration(cfg, nets, nets, b))
    return _FULL[case]


@pytest.mark.parametrize("case", R.CASES + [("A", "16bit")], ids=["-".join(c) for c in R.CASES] + ["A-16bit"])
def test_every_key_of_a_stack_moves_the_gradient_of_its_group(case):
    """the fixtures of tests/test_gpu_combo.py, on the oracle alone: one key off, the others on, moves the gradient of the group the key acts
    on by >= 0.1 relative L2; the wrappers are exhausted; grad_clip's bound lies below both norms; the sign fixture keeps its margin"""
    cfg, nets, b, full = _full(case)
    seen = {}
    assert full["dis"]["calls"] == {"dis_forward": 8, "augment": 8 if case[0] == "A" else None, "blocks": 8, "lsgan": 8}
    assert full["gen"]["calls"] == {"dis_forward": 5, "augment": 5 if case[0] == "A" else None, "blocks": 5}
    for which in ("dis", "gen"):
        for key in R.ACTS_ON[case[0]][which]:
            off = R.iteration(R.drop_key(cfg, key), nets, nets, b, which=(which,))[which]
            change = R.group_change(full[which]["grads"], off["grads"])
            print("combo sensitivity %s %s without %-14s %.3f" % ("-".join(case), which, key, change))
            assert change >= SENSITIVITY, (case, which, key, change)
            seen["%s without %s" % (which, key)] = change
        norm = sum(float(t.double().norm() ** 2) for t in full[which]["grads"].values()) ** 0.5
        assert norm >= 50 * R.GRAD_CLIP, (case, which, norm)
    # the keys that must NOT reach the other update
    assert R.group_change(R.iteration(R.drop_key(cfg, "lecam_lambda"), nets, nets, b, which=("gen",))["gen"]["grads"], full["gen"]["grads"]) == 0
    assert R.group_change(R.iteration(R.drop_key(cfg, "ms_lambda"), nets, nets, b, which=("dis",))["dis"]["grads"], full["dis"]["grads"]) == 0
    r, margin = R.sign_r(full["dis"]["real_outs"])
    print("combo sign fixture %s: r %.6f margin %.3e" % ("-".join(case), r, margin))
    assert margin >= 1e-3 and abs(r) < 1      # maps on both sides of 0.5, none near it
    _record("oracle sensitivity " + "-".join(case), dict(seen, sign_r=r, sign_margin=margin))


def test_the_oracles_attributes_come_back_after_an_error(plain):
    base, nets, b = plain["none"]
    before = (O.dis_forward, O.lsgan)
    cfg = R.with_keys(base, dis_augment="color,translation,cutout")
    with pytest.raises(AssertionError, match="rows"):
        R.dis_update(cfg, nets, b["x_a"], b["x_b"], b["z"][:3], aug=b["aug_g"])      # 5 B rows where dis_update reads 7 B
    with pytest.raises(AssertionError):
        R.dis_update(cfg, nets, b["x_a"], b["x_b"][:, :2], b["z"][:3], aug=b["aug_d"])      # fails inside the patched region, at dis_B's real side
    assert (O.dis_forward, O.lsgan) == before
