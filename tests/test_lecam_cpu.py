"""LeCam regularisation of the discriminators (config keys lecam_lambda / lecam_decay / lecam_start; include/aclgan_hip.h:
aclgan_ctx_set_lecam) -- everything about it that needs no GPU: the config keys and what they refuse, the shipped configs, the exported
symbols and the header text, the launch-free queries, the argument checks, and the oracle wrapper of tests/lecam_ref.py against the
formulas written out in fp64."""
import ctypes as C
import glob
import os

import pytest
import torch
import yaml

from conftest import ROOT
from oracle import aclgan_oracle as O
from lecam_ref import CALLS, NETS, class_means, fold, lecam_values, oracle_lsgan


def _mods():
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib, trainer
    return _lib, trainer


def test_lecam_from_config():
    L, T = _mods()
    f = T.lecam_from_config
    assert "lecam_from_config" in T.__all__
    assert f({}) == (0.0, 0.99, 1000) and f({"lecam_lambda": 0}) == (0.0, 0.99, 1000)
    assert f({"lecam_lambda": 1, "lecam_decay": 0, "lecam_start": 0}) == (1.0, 0.0, 0)
    assert f({"lecam_lambda": 0.3, "lecam_decay": 0.5, "lecam_start": 7}) == (0.3, 0.5, 7)
    lam, decay, start = f({"lecam_lambda": 1})
    assert isinstance(lam, float) and isinstance(decay, float) and isinstance(start, int)
    for bad in (-1, -0.0001, float("nan"), float("inf"), 1e39, "0.3", None, True, [1.0]):
        with pytest.raises(L.AclganError, match="lecam_lambda"):
            f({"lecam_lambda": bad})
    for bad in (-0.1, 1, 1.0, 1.5, float("nan"), "0.99", None, True):
        with pytest.raises(L.AclganError, match="lecam_decay"):
            f({"lecam_lambda": 1.0, "lecam_decay": bad})
        with pytest.raises(L.AclganError, match="lecam_decay"):
            f({"lecam_decay": bad})                               # checked with the regulariser off too
    for bad in (-1, 1.0, 1000.0, "1000", None, True, 2 ** 31):
        with pytest.raises(L.AclganError, match="lecam_start"):
            f({"lecam_lambda": 1.0, "lecam_start": bad})
    # it composes with the other limited-data keys: nothing is refused
    assert f({"dis": {"norm": "sn"}, "dis_augment": "color", "r1_gamma": 0, "ema_decay": 0.999, "lecam_lambda": 2.0}) == (2.0, 0.99, 1000)


def test_shipped_configs():
    """only selfie2anime_lecam.yaml turns the key on, and it is selfie2anime.yaml plus the key"""
    L, T = _mods()
    shipped = sorted(glob.glob(os.path.join(ROOT, "configs", "*.yaml")))
    assert len(shipped) >= 7
    for path in shipped:
        cfg = yaml.safe_load(open(path))
        lam, decay, start = T.lecam_from_config(cfg)
        assert (lam > 0) == path.endswith("selfie2anime_lecam.yaml"), path
        assert (decay, start) == (0.99, 1000), path
    base = yaml.safe_load(open(os.path.join(ROOT, "configs", "selfie2anime.yaml")))
    lec = yaml.safe_load(open(os.path.join(ROOT, "configs", "selfie2anime_lecam.yaml")))
    assert lec.pop("lecam_lambda") == 0.3 and lec == base
    assert T.augment_from_config(lec) == 0 and T.r1_from_config(lec)[0] == 0 and T.ema_from_config(lec)[0] == 0
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "LeCam" in readme and "lecam_lambda" in readme and "nobody has measured" in readme.lower().replace("\n", " ")


def _ctx(L, scales=3, norm=0):
    a = L.Arch(3, 6, 8, 16, 8, 4, 2, 2, 8, 4, scales)
    ctx = C.c_void_p()
    L.check(L.lib.aclgan_ctx_create_dis_norm(C.byref(a), norm, C.byref(ctx)))
    return ctx


def test_symbols_header_and_state_size_without_gpu():
    L, _ = _mods()
    for name, nargs in (("aclgan_lecam_state_floats", 1), ("aclgan_ctx_set_lecam", 5), ("aclgan_lsgan_lecam_multi", 16), ("aclgan_lecam_fold", 4)):
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == nargs
        assert getattr(L.lib, name).argtypes is not None
    header = open(os.path.join(ROOT, "include", "aclgan_hip.h")).read()
    assert "size_t aclgan_lecam_state_floats(aclgan_ctx* ctx);" in header
    assert "int aclgan_ctx_set_lecam(aclgan_ctx* ctx, float lambda, float decay, int start, float* state);" in header
    assert "int aclgan_lsgan_lecam_multi(" in header and "int aclgan_lecam_fold(float* state, int num_scales, float decay, void* stream);" in header
    for text in ("lam_eff = lambda if count >= max(start, 1) else 0", "a non-finite m leaves a as it is", "18 S + 4 floats", "Tseng et al."):
        assert text in header, text
    n0 = L.lib.aclgan_launch_count()
    for scales in (1, 2, 3):
        ctx = _ctx(L, scales)
        assert L.lib.aclgan_lecam_state_floats(ctx) == 18 * scales + 4
        L.lib.aclgan_ctx_destroy(ctx)
    assert L.lib.aclgan_lecam_state_floats(None) == 0
    assert L.lib.aclgan_launch_count() == n0


def test_argument_checks_launch_nothing():
    """every refusal is ACLGAN_EINVAL with a message, made before anything is enqueued; a refused call leaves the context as it was"""
    L, _ = _mods()
    EINVAL = -1
    n0 = L.lib.aclgan_launch_count()
    ctx = _ctx(L)
    f = L.lib.aclgan_ctx_set_lecam
    fake = C.c_void_p(0x10000)
    assert f(None, 1.0, 0.99, 0, fake) == EINVAL
    for lam in (-1.0, -1e-30, float("nan"), float("inf"), -float("inf")):
        assert f(ctx, lam, 0.99, 0, fake) == EINVAL and "lambda" in L.last_error()
        assert f(ctx, lam, 0.99, 0, None) == EINVAL
    for decay in (-0.5, 1.0, 1.5, float("nan"), float("inf")):
        assert f(ctx, 1.0, decay, 0, fake) == EINVAL and "decay" in L.last_error()
    for start in (-1, -2 ** 31):
        assert f(ctx, 1.0, 0.99, start, fake) == EINVAL and "start" in L.last_error()
    assert f(ctx, 0.0, 0.0, 0, fake) == 0 and f(ctx, 1.0, 0.99, 10 ** 9, fake) == 0 and f(ctx, 1.0, 0.99, 0, None) == 0
    # the operators
    m = L.lib.aclgan_lsgan_lecam_multi
    arr = (C.c_void_p * 1)(0x10000)
    n = (C.c_int * 1)(4)
    fl = (C.c_float * 1)(1.0)
    ok = [arr, n, fl, fl, arr, arr, fl, arr, arr, arr, 1, 1.0, 0, fake, None, None]
    for i in (0, 1, 2, 3, 4, 6, 7, 8, 9, 13):      # a null array / a null count
        args = list(ok)
        args[i] = None
        assert m(*args) == EINVAL, i
    for i, v in ((10, 0), (10, 1025), (11, -1.0), (11, float("nan")), (11, float("inf")), (12, -1)):
        args = list(ok)
        args[i] = v
        assert m(*args) == EINVAL, (i, v)
    null = (C.c_void_p * 1)(None)
    for i in (0, 4, 7, 8, 9):                      # a null entry
        args = list(ok)
        args[i] = null
        assert m(*args) == EINVAL and "term 0" in L.last_error(), i
    args = list(ok)
    args[1] = (C.c_int * 1)(0)
    assert m(*args) == EINVAL
    g = L.lib.aclgan_lecam_fold
    assert g(None, 3, 0.9, None) == EINVAL and g(fake, 0, 0.9, None) == EINVAL
    for decay in (-0.1, 1.0, float("nan")):
        assert g(fake, 3, decay, None) == EINVAL and "decay" in L.last_error()
    L.lib.aclgan_ctx_destroy(ctx)
    assert L.lib.aclgan_launch_count() == n0


def test_dry_runs_count_the_fold():
    """with a state bound the algorithmic bytes of dis_update grow by the fold's (the state read and written once); gen_update's, the
    executed FLOPs and the workspace do not move; unbinding restores every figure"""
    L, _ = _mods()
    n0 = L.lib.aclgan_launch_count()
    ctx = _ctx(L)
    fake = C.c_void_p(0x10000)
    for grp in (0, 1):
        L.check(L.lib.aclgan_bind_params(ctx, grp, fake, fake, fake, fake))

    def q():
        ws, out = C.c_size_t(), []
        L.check(L.lib.aclgan_workspace_bytes(ctx, 2, 64, 64, C.byref(ws)))
        for which in (0, 1):
            v, w = C.c_double(), C.c_double()
            L.check(L.lib.aclgan_step_algorithmic_bytes(ctx, which, 2, 64, 64, C.byref(v)))
            L.check(L.lib.aclgan_step_executed_flops(ctx, which, 2, 64, 64, C.byref(w)))
            out += [v.value, w.value]
        return [ws.value] + out
    off = q()
    L.check(L.lib.aclgan_ctx_set_lecam(ctx, 1.0, 0.99, 0, fake))
    on = q()
    assert on[0] == off[0] and on[1] == off[1] and on[2] == off[2] and on[4] == off[4]
    assert on[3] - off[3] == 2 * 4 * (18 * 3 + 4)
    L.check(L.lib.aclgan_ctx_set_lecam(ctx, 1.0, 0.99, 0, None))
    assert q() == off
    L.lib.aclgan_ctx_destroy(ctx)
    assert L.lib.aclgan_launch_count() == n0


def _fake_outs(g, S=3, B=2):
    return [torch.randn(B, 1, 8 >> s, 6 >> s if (6 >> s) else 1, generator=g, dtype=torch.float64).requires_grad_(True) for s in range(S)]


def test_wrapper_is_the_formula_in_fp64():
    """eight calls in dis_losses' order on random fp64 maps: the values are lsgan's, the gradient of every map is
    w * (2/n) * [(o - t) + lam * (o - a[D][s][1 - t])], the recorded values and means are the sums written out, and the fold is the recurrence"""
    g = torch.Generator().manual_seed(5)
    anchors = {D: [[0.2 + 0.1 * s + 0.05 * i, 0.8 - 0.1 * s - 0.05 * i] for s in range(3)] for i, D in enumerate(NETS)}
    lam = 0.7
    w = oracle_lsgan(O.lsgan, anchors, lam)
    plain = []
    maps = []
    total = 0
    for D, cls, wt in CALLS:
        outs = _fake_outs(g)
        maps.append(outs)
        v = w(outs, float(cls))
        ref = O.lsgan([o.detach() for o in outs], float(cls))
        assert float(v.detach()) == float(ref)
        plain.append(float(ref))
        total = total + wt * v
    total.backward()
    with pytest.raises(AssertionError):
        w(maps[0], 0.0)                     # a ninth call
    want_vals = {D: 0.0 for D in NETS}
    for (D, cls, wt), outs in zip(CALLS, maps):
        for s, o in enumerate(outs):
            od = o.detach()
            a = anchors[D][s][1 - cls]
            ref = wt * (2.0 / od.numel()) * ((od - cls) + lam * (od - a))
            assert float((o.grad - ref).abs().max()) <= 1e-15
            want_vals[D] += wt * float(((od - a) ** 2).mean())
    got = lecam_values(w.rec)
    assert all(abs(got[D] - want_vals[D]) <= 1e-14 for D in NETS)
    means = class_means(w.rec)
    # dis_A: calls 0 and 2 are its fake side, 1 and 3 its real side, each at weight 0.5; dis_B / dis_2: one call per side
    for s in range(3):
        assert abs(means["A"][s][0] - 0.5 * (float(maps[0][s].detach().mean()) + float(maps[2][s].detach().mean()))) <= 1e-15
        assert abs(means["A"][s][1] - 0.5 * (float(maps[1][s].detach().mean()) + float(maps[3][s].detach().mean()))) <= 1e-15
        assert means["B"][s] == [float(maps[4][s].detach().mean()), float(maps[5][s].detach().mean())]
        assert means["2"][s] == [float(maps[6][s].detach().mean()), float(maps[7][s].detach().mean())]
    first = fold(None, means, 0, 0.9)
    assert first == means and first["A"] is not means["A"]
    second = fold(anchors, means, 1, 0.9)
    assert abs(second["B"][1][0] - (0.9 * anchors["B"][1][0] + 0.1 * means["B"][1][0])) <= 1e-16
    # count == 0: no anchors, no term -- the plain gradient, values 0, means still recorded
    w0 = oracle_lsgan(O.lsgan, None, lam)
    outs = _fake_outs(g)
    w0(outs, 0.0).backward()
    assert all(float((o.grad - 2.0 * o.detach() / o.numel()).abs().max()) <= 1e-16 for o in outs)
    assert w0.rec["terms"] == [[0.0, 0.0, 0.0]] and len(w0.rec["means"][0]) == 3


def test_wrapped_oracle_update_calls_lsgan_eight_times(monkeypatch):
    """reduced width, 64x64, B=2, lam 1, anchors (0.2, 0.8): the wrapper sits where dis_losses calls lsgan, the four discriminator losses
    do not move, and the discriminator gradient moves by far more than the 0.1 relative L2 the GPU test asks of its fixture"""
    cfg = O.default_config()
    cfg["gen"].update(dim=8, mlp_dim=16, n_res=1)
    cfg["dis"].update(dim=8)
    cfg["display_size"] = 1
    nets = O.test_nets(cfg, 0)
    g = torch.Generator().manual_seed(3)
    x_a, x_b = torch.rand(2, 3, 64, 64, generator=g) * 2 - 1, torch.rand(2, 3, 64, 64, generator=g) * 2 - 1
    z = [torch.randn(2, 8, 1, 1, generator=g) for _ in range(3)]
    off = O.OracleTrainer(cfg, nets=nets)
    off.dis_update(x_a, x_b, z, apply=False)
    on = O.OracleTrainer(cfg, nets=nets)
    anchors = {D: [[0.2, 0.8]] * cfg["dis"]["num_scales"] for D in NETS}
    with monkeypatch.context() as m:
        w = oracle_lsgan(O.lsgan, anchors, 1.0)
        m.setattr(O, "lsgan", w)
        on.dis_update(x_a, x_b, z, apply=False)
    assert len(w.rec["means"]) == 8
    assert on.losses == off.losses
    num = sum(float((a.grad.double() - b.grad.double()).norm() ** 2) for a, b in zip(on.dis_opt.params, off.dis_opt.params)) ** 0.5
    den = sum(float(b.grad.double().norm() ** 2) for b in off.dis_opt.params) ** 0.5
    print("relative L2 change of the discriminator gradient: %.3f" % (num / den))
    assert num / den >= 0.1
    assert all(v > 0 for v in lecam_values(w.rec).values())
