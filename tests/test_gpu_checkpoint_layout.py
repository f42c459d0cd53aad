"""What save() writes and what resume() does when a sidecar state is absent, with the training keys of stack A on (tests/combo_ref.py: the
reduced-width fixture, B = 2, 64x64), in fp32 and fp16, against literals: the directory listing, every file's top-level keys, the shapes and
dtypes of the state tensors and of optimizer.pt's two extra keys, the text of every resume warning and the state each one restarts from.
And train.py's log-line suffix, log_suffix(), against the five terms it is made of, in their order.
Run on the GPU box: pytest -m gpu"""
import os
import warnings

import pytest
import torch

from oracle import aclgan_oracle as O
import combo_ref as R

pytestmark = pytest.mark.gpu

GEN, DIS = 0, 1
# the files of a checkpoint written at iterations = 0 and their top-level keys, sorted
PLAIN = {"dis_00000001.pt": ["2", "A", "B"], "gen_00000001.pt": ["AB", "BA"], "optimizer.pt": ["dis", "gen"]}
STACK_A = {"ada_00000001.pt": ["interval", "kimg", "state", "target"], "dis_00000001.pt": ["2", "A", "B"],
           "ema_00000001.pt": ["AB", "BA", "decay", "updates"], "gen_00000001.pt": ["AB", "BA"], "lecam_00000001.pt": ["decay", "state"],
           "optimizer.pt": ["aclgan_grad_clip_state", "dis", "gen"]}
NUM_SCALES = 3
LECAM_SHAPE = (18 * NUM_SCALES + 4,)      # include/aclgan_hip.h: aclgan_lecam_state_floats
ADA_SHAPE = (12,)                         # aclgan_ada_state_floats
CLIP_SHAPE = (2, 8)                       # row 0 gen, row 1 dis: the eight leading floats of a group's state
LOSS_SCALE_SHAPE = (8,)                   # aclgan_bind_loss_scale


@pytest.fixture(scope="module")
def T():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import aclgan_amd  # noqa: F401
    from aclgan_amd import trainer
    return trainer


def _iteration(T, cfg, nets, b, **kw):
    """a trainer at `nets` after one dis_update and one gen_update on the fixture's explicit inputs"""
    tr = T.aclgan_Trainer(cfg, **kw)
    for name in O.OracleTrainer.NETS:
        getattr(tr, name).load_state_dict(nets[name], strict=False)
    if tr._ema is not None:
        tr.ema_reset()
    x_a, x_b = b["x_a"].cuda(), b["x_b"].cuda()
    on = lambda d: {k: v for k, v in d.items() if v is not None}      # noqa: E731
    tr.dis_update(x_a, x_b, cfg, z=b["z"][:3], **on({"aug": b["aug_d"] if tr.augment else None, "aug_u": b["u_d"] if tr._ada is not None else None}))
    tr.gen_update(x_a, x_b, cfg, z=b["z"][3:], **on({"aug": b["aug_g"] if tr.augment else None, "aug_u": b["u_g"] if tr._ada is not None else None,
                                                     "z_ms": b["z_ms"] if tr.ms_lambda > 0 else None}))
    torch.cuda.synchronize()
    return tr


@pytest.fixture(scope="module")
def stack_a(T):
    cfg, nets, b = R.case("A", "none", "focus")
    return cfg, _iteration(T, cfg, nets, b)


def _listing(d):
    return {name: sorted(torch.load(os.path.join(d, name), map_location="cpu")) for name in sorted(os.listdir(d))}


def _check_stack_a_files(d, cfg, fp16):
    want = dict(STACK_A)
    if fp16:
        want["optimizer.pt"] = ["aclgan_grad_clip_state", "aclgan_loss_scale_state", "dis", "gen"]
    assert _listing(d) == want
    load = lambda name: torch.load(os.path.join(d, name), map_location="cpu")      # noqa: E731
    lecam, ada, ema, opt = load("lecam_00000001.pt"), load("ada_00000001.pt"), load("ema_00000001.pt"), load("optimizer.pt")
    assert tuple(lecam["state"].shape) == LECAM_SHAPE and lecam["state"].dtype == torch.float32 and lecam["state"].device.type == "cpu"
    assert lecam["decay"] == cfg["lecam_decay"] == 0.9
    assert tuple(ada["state"].shape) == ADA_SHAPE and ada["state"].dtype == torch.float32
    assert (ada["target"], ada["interval"], ada["kimg"]) == (0.6, 4, 500.0) and float(ada["state"][0]) == cfg["dis_augment_p"] == 0.5
    assert ema["updates"] == 1 and ema["decay"] == cfg["ema_decay"] == 0.9
    gen = load("gen_00000001.pt")
    for k in ("AB", "BA"):
        assert list(ema[k]) == list(gen[k]) and all(ema[k][n].shape == gen[k][n].shape and ema[k][n].dtype == gen[k][n].dtype for n in gen[k])
    clip = opt["aclgan_grad_clip_state"]
    assert tuple(clip.shape) == CLIP_SHAPE and clip.dtype == torch.float32
    if fp16:
        ls = opt["aclgan_loss_scale_state"]
        assert tuple(ls.shape) == LOSS_SCALE_SHAPE and ls.dtype == torch.float32
    assert sorted(opt["gen"]) == sorted(opt["dis"]) == ["param_groups", "state"]


def test_stack_a_checkpoint_fp32(T, stack_a, tmp_path):
    cfg, tr = stack_a
    tr.save(str(tmp_path), 0)
    _check_stack_a_files(str(tmp_path), cfg, fp16=False)


def test_stack_a_checkpoint_fp16(T, tmp_path):
    cfg, nets, b = R.case16()
    tr = _iteration(T, cfg, nets, b, compute_dtype="fp16")
    tr.save(str(tmp_path), 0)
    _check_stack_a_files(str(tmp_path), cfg, fp16=True)


def test_default_keys_write_no_sidecar_and_no_extra_key(T, tmp_path):
    cfg = R.base_config()
    tr = _iteration(T, cfg, R.scaled_nets(cfg), R.batch(R.BATCH_SEED))
    tr.save(str(tmp_path), 0)
    assert _listing(str(tmp_path)) == PLAIN
    assert tr.log_suffix() == ""


def test_resume_without_the_sidecars_warns_and_restarts_each_state(T, tmp_path):
    cfg, nets, b = R.case("A", "none", "focus")
    tr = _iteration(T, cfg, nets, b)      # (a trainer of its own: resume() restarts its states)
    d = str(tmp_path)
    tr.save(d, 0)
    for name in ("ema_00000001.pt", "lecam_00000001.pt", "ada_00000001.pt"):
        os.remove(os.path.join(d, name))
    opt = torch.load(os.path.join(d, "optimizer.pt"), map_location="cpu")
    del opt["aclgan_grad_clip_state"]
    torch.save(opt, os.path.join(d, "optimizer.pt"))
    # the states this trainer's two updates left are not the ones a restart gives
    assert tr.lecam_updates == 1 and float(tr._lecam.abs().sum()) > 0
    assert all(float(t[:4].abs().sum()) > 0 for t in tr._clip) and tr.grad_clip_state()["dis"]["clipped"] == 1
    assert not torch.equal(tr._ema, tr._param[GEN])
    assert tr.ada_state()["updates"] == 1
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        assert tr.resume(d, cfg) == 1
    texts = [str(w.message) for w in seen]
    want = ["aclgan_Trainer.resume: optimizer.pt holds no aclgan_grad_clip_state (written with grad_clip off); the clipped and skipped counts start at 0",
            "aclgan_Trainer.resume: %s not found; the averaged generator starts from the resumed weights" % os.path.join(d, "ema_00000001.pt"),
            "aclgan_Trainer.resume: %s not found; the LeCam anchors start again (the term acts after lecam_start more updates)"
            % os.path.join(d, "lecam_00000001.pt"),
            "aclgan_Trainer.resume: %s not found; the augmentation probability starts again at 0.5" % os.path.join(d, "ada_00000001.pt")]
    assert [t for t in texts if t.startswith("aclgan_Trainer.resume")] == want
    torch.cuda.synchronize()
    assert float(tr._lecam.abs().sum()) == 0 and tr.lecam_updates == 0
    assert tr._ada.cpu().tolist() == [0.5] + [0.0] * 11 and tr.ada_state()["p"] == 0.5
    assert all(float(t.abs().sum()) == 0 for t in tr._clip)
    assert tr.grad_clip_state() == {k: {"norm": 0.0, "coef": 0.0, "clipped": 0, "skipped": 0} for k in ("gen", "dis")}
    assert torch.equal(tr._ema, tr._param[GEN])
    assert tr._opt[GEN]["steps"] == tr._opt[DIS]["steps"] == 1


def test_log_suffix_stack_a(T, stack_a):
    """R1's term (absent in stack A), then the lecam, grad_clip, mode-seeking and ada texts, in train.py's order"""
    _, tr = stack_a
    got = tr.log_suffix()
    assert got == tr.lecam_log_text() + tr.grad_clip_log_text() + tr.modeseek_log_text() + tr.ada_log_text()
    assert got.startswith(" lecam_A=") and " gnorm_G=" in got and " ms_A=" in got and " ada_p=0.5 ada_rt=" in got and "r1_A" not in got
    assert got.index(" lecam_A=") < got.index(" gnorm_G=") < got.index(" ms_A=") < got.index(" ada_p=")


def test_log_suffix_stack_b_begins_with_the_r1_term(T):
    cfg, nets, b = R.case("B", "none", "focus")
    tr = _iteration(T, cfg, nets, b)
    assert tr.r1_passes == 1 and float(tr.loss_dis_r1_A) > 0
    r1 = " r1_A=%.4g r1_B=%.4g" % (float(tr.loss_dis_r1_A), float(tr.loss_dis_r1_B))
    assert tr.log_suffix() == r1 + tr.lecam_log_text() + tr.grad_clip_log_text() + tr.modeseek_log_text()
