"""Gradient norm per group: readout, clipping and the non-finite guard (config keys grad_clip / grad_clip_gen / grad_clip_dis;
include/aclgan_hip.h: aclgan_bind_grad_clip) -- everything about it that needs no GPU: the config keys and what they refuse, the shipped
configs, the exported symbols, the argument checks, the traffic count, and the fp64 model of tests/gradclip_ref.py against
torch.nn.utils.clip_grad_norm_ + torch.optim.Adam in fp64 and against LossScaleModel."""
import ctypes as C
import glob
import math
import os

import pytest
import torch
import yaml

from conftest import ROOT
from oracle import optimizer_oracle as M
from gradclip_ref import ClipModel, clip_rule, norm_f32

INF = float("inf")


def _mods():
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib, trainer
    return _lib, trainer


def test_grad_clip_from_config():
    L, T = _mods()
    f = T.grad_clip_from_config
    assert "grad_clip_from_config" in T.__all__
    assert f({}) == (0.0, 0.0) and f({"grad_clip": 0}) == (0.0, 0.0)
    assert f({"grad_clip": 5}) == (5.0, 5.0) and f({"grad_clip": INF}) == (INF, INF)
    assert f({"grad_clip": 5, "grad_clip_gen": 0}) == (0.0, 5.0) and f({"grad_clip": 5, "grad_clip_dis": 0.5}) == (5.0, 0.5)
    assert f({"grad_clip_gen": INF}) == (INF, 0.0) and f({"grad_clip_dis": 2, "grad_clip_gen": 3}) == (3.0, 2.0)
    assert all(isinstance(v, float) for v in f({"grad_clip": 1}))
    assert yaml.safe_load("grad_clip: .inf")["grad_clip"] == INF
    for key in ("grad_clip", "grad_clip_gen", "grad_clip_dis"):
        for bad in (-1, -1e-9, -INF, float("nan"), 1e-50, "5", True, [1.0], None):
            with pytest.raises(L.AclganError, match=key + "="):
                f({key: bad})
    # it composes with the other keys: nothing is refused
    assert f({"dis": {"norm": "sn"}, "dis_augment": "color", "r1_gamma": 0, "lecam_lambda": 1.0, "ema_decay": 0.999, "grad_clip": 1.5}) == (1.5, 1.5)


def test_shipped_configs():
    """only selfie2anime_gradclip.yaml turns the key on (.inf: guard and readout, no bound), and it is selfie2anime.yaml plus the key"""
    L, T = _mods()
    shipped = sorted(glob.glob(os.path.join(ROOT, "configs", "*.yaml")))
    assert len(shipped) >= 8
    for path in shipped:
        want = (INF, INF) if path.endswith("selfie2anime_gradclip.yaml") else (0.0, 0.0)
        assert T.grad_clip_from_config(yaml.safe_load(open(path))) == want, path
    base = yaml.safe_load(open(os.path.join(ROOT, "configs", "selfie2anime.yaml")))
    gc = yaml.safe_load(open(os.path.join(ROOT, "configs", "selfie2anime_gradclip.yaml")))
    assert gc.pop("grad_clip") == INF and gc == base
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "grad_clip" in readme and "gnorm_G" in readme and "profiles/gradclip.json" in readme


def _ctx(L):
    a = L.Arch(3, 6, 8, 16, 8, 4, 2, 1, 8, 4, 3)
    ctx = C.c_void_p()
    L.check(L.lib.aclgan_ctx_create(C.byref(a), C.byref(ctx)))
    return ctx


def test_symbols_header_and_state_size_without_gpu():
    L, _ = _mods()
    for name, nargs in (("aclgan_grad_clip_state_floats", 0), ("aclgan_bind_grad_clip", 4), ("aclgan_grad_clip_flat", 5)):
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == nargs
        assert getattr(L.lib, name) is not None
    header = open(os.path.join(ROOT, "include", "aclgan_hip.h")).read()
    for text in ("size_t aclgan_grad_clip_state_floats(void);", "int aclgan_bind_grad_clip(aclgan_ctx* ctx, int group, float max_norm, float* state);",
                 "int aclgan_grad_clip_flat(const float* g, int64_t n, float max_norm, float* state, void* stream);",
                 "coef = min(1, max_norm / (norm + 1e-6))", "state[3] += 1"):
        assert text in header, text
    n0 = L.lib.aclgan_launch_count()
    assert L.lib.aclgan_grad_clip_state_floats() >= 8
    assert L.lib.aclgan_launch_count() == n0


def test_argument_checks_launch_nothing():
    """every refusal is ACLGAN_EINVAL with a message, made before anything is enqueued"""
    L, _ = _mods()
    EINVAL = -1
    n0 = L.lib.aclgan_launch_count()
    ctx = _ctx(L)
    f = L.lib.aclgan_bind_grad_clip
    fake = C.c_void_p(0x10000)
    assert f(None, 0, 1.0, fake) == EINVAL
    for grp in (-1, 2, 3):
        assert f(ctx, grp, 1.0, fake) == EINVAL and "group" in L.last_error()
        assert f(ctx, grp, 1.0, None) == EINVAL
    for grp in (0, 1):
        for bad in (float("nan"), 0.0, -0.0, -1.0, -1e-30, -INF):
            assert f(ctx, grp, bad, fake) == EINVAL and "max_norm" in L.last_error(), bad
        assert f(ctx, grp, 1.0, fake) == 0 and f(ctx, grp, INF, fake) == 0 and f(ctx, grp, 1e-30, fake) == 0
        assert f(ctx, grp, 1.0, None) == 0 and f(ctx, grp, 0.0, None) == 0      # unbinding does not look at max_norm
    g = L.lib.aclgan_grad_clip_flat
    assert g(None, 10, 1.0, fake, None) == EINVAL and g(fake, 10, 1.0, None, None) == EINVAL and g(fake, 0, 1.0, fake, None) == EINVAL
    assert g(C.c_void_p(0x10002), 10, 1.0, fake, None) == EINVAL
    for bad in (float("nan"), 0.0, -1.0, -INF):
        assert g(fake, 10, bad, fake, None) == EINVAL and "max_norm" in L.last_error()
    L.lib.aclgan_ctx_destroy(ctx)
    assert L.lib.aclgan_launch_count() == n0


def test_dry_runs_count_the_extra_read_of_the_gradients():
    """fp32 / bf16 path: + 4 B per parameter of a group with a bound state, that update only; under a bound loss scale the pass replaces
    the overflow scan, which the count has never included: nothing is added.  Unbinding restores every figure."""
    L, _ = _mods()
    n0 = L.lib.aclgan_launch_count()
    ctx = _ctx(L)
    fake = C.c_void_p(0x10000)
    for grp in (0, 1):
        L.check(L.lib.aclgan_bind_params(ctx, grp, fake, fake, fake, fake))
    numel = [L.lib.aclgan_group_numel(ctx, grp) for grp in (0, 1)]

    def q():
        out = []
        for which in (0, 1):
            v, w = C.c_double(), C.c_double()
            L.check(L.lib.aclgan_step_algorithmic_bytes(ctx, which, 2, 64, 64, C.byref(v)))
            L.check(L.lib.aclgan_step_executed_flops(ctx, which, 2, 64, 64, C.byref(w)))
            out += [v.value, w.value]
        return out
    off = q()
    for grp in (0, 1):
        L.check(L.lib.aclgan_bind_grad_clip(ctx, grp, INF, fake))
        on = q()
        assert on[2 * grp] - off[2 * grp] == 4.0 * numel[grp] and on[2 * (1 - grp)] == off[2 * (1 - grp)]
        assert on[1] == off[1] and on[3] == off[3]
        L.check(L.lib.aclgan_bind_loss_scale(ctx, fake))
        assert q() == off
        L.check(L.lib.aclgan_bind_loss_scale(ctx, None))
        L.check(L.lib.aclgan_bind_grad_clip(ctx, grp, 0.0, None))
        assert q() == off
    L.lib.aclgan_ctx_destroy(ctx)
    assert L.lib.aclgan_launch_count() == n0


# ---------------------------------------------------------------- the fp64 model
B1, B2, EPS, WD, LR = 0.5, 0.999, 1e-8, 1e-4, 1e-4


def test_model_follows_torch_clip_grad_norm_and_adam_in_fp64():
    """ten steps, gradient norms alternating between 0.25 and 4 times max_norm: clipped and unclipped steps"""
    n, max_norm = 500, 0.37
    gen = torch.Generator().manual_seed(5)
    p0 = torch.randn(n, generator=gen, dtype=torch.float64)
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD)
    mine = ClipModel(p0, B1, B2, EPS, WD, max_norm)
    clipped = 0
    for t in range(1, 11):
        u = torch.randn(n, generator=gen, dtype=torch.float64)
        r = 0.25 if t % 2 else 4.0
        g = r * max_norm * u / u.norm()
        ref.grad = g.clone()
        total = torch.nn.utils.clip_grad_norm_([ref], max_norm)
        opt.step()
        assert mine.step(g, LR, t)
        clipped += r > 1
        assert abs(mine.norm64 - float(total)) <= 1e-12 * float(total)
        assert mine.state[2] == clipped and mine.state[3] == 0
        assert (mine.state[1] == 1.0) == (r < 1) and abs(mine.state[1] - min(1.0, 1.0 / r)) < 1e-4
    st = opt.state[ref]
    rel_p = ((mine.adam.p - ref.detach()).abs() / (10 * LR)).max().item()      # of the distance ten steps can move a parameter
    rel_v = ((mine.adam.v - st["exp_avg_sq"]).abs() / st["exp_avg_sq"]).max().item()
    err_m = ((mine.adam.m - st["exp_avg"]).abs() / mine.adam.gvmax).max().item()
    print("clip model vs torch fp64: p %.2e, v %.2e, m %.2e" % (rel_p, rel_v, err_m))
    # (norm and coefficient are rounded to fp32, as the kernel rounds them: up to 2 * 2^-24 = 1.2e-7 relative on the clipped gradients, hence
    # twice that on v; m / sqrt(v) sees it only where clipped and unclipped steps mix)
    assert rel_p <= 1e-6 and rel_v <= 1e-6 and err_m <= 1e-6, (rel_p, rel_v, err_m)
    assert clipped == 5


def test_model_monitor_mode_is_plain_adam_and_never_clips():
    n = 100
    gen = torch.Generator().manual_seed(6)
    p0 = torch.randn(n, generator=gen, dtype=torch.float64)
    mine, plain = ClipModel(p0, B1, B2, EPS, WD, INF), M.Adam64(p0, B1, B2, EPS, WD)
    for t in range(1, 4):
        g = torch.randn(n, generator=gen, dtype=torch.float64) * 10.0 ** t
        assert mine.step(g, LR, t)
        plain.step(g, LR, t=t)
        assert mine.state[1:] == [1.0, 0.0, 0.0]
    assert torch.equal(mine.adam.p, plain.p) and torch.equal(mine.adam.m, plain.m) and torch.equal(mine.adam.v, plain.v)
    assert clip_rule(0.0, INF) == 1.0 and clip_rule(3e38, INF) == 1.0 and 0.4999 < clip_rule(2.0, 1.0) < 0.5


def test_model_skip_rule_beside_the_loss_scale_model():
    """interleaved sequence on one group under a loss scale: fp16 overflows are the loss-scale machine's (clip counters stay), a non-finite
    norm of finite gradients is the clip state's, and the bias-correction step excludes both"""
    n, S = 64, 2.0 ** 10
    gen = torch.Generator().manual_seed(7)
    p0 = torch.randn(n, generator=gen, dtype=torch.float64).float()
    ls, twin = M.LossScaleModel(S, interval=1e6), M.LossScaleModel(S, interval=1e6)
    mine = ClipModel(p0, B1, B2, EPS, WD, 1.0, group=1, loss_scale=ls)
    events = ["clean", "inf", "clean", "huge", "nan", "clean", "huge", "clean"]
    applied = host = 0
    for ev in events:
        g = (torch.randn(n, generator=gen, dtype=torch.float64) * 1e-2).float() * ls.state[0]
        if ev == "inf":
            g[3] = INF
        elif ev == "nan":
            g[n - 1] = float("nan")
        elif ev == "huge":
            g[5] = 3e38      # finite: no overflow for the loss-scale machine; (3e38 / S)^2 is no fp32 number: the norm is inf
        host += 1
        before = (mine.adam.p.clone(), list(mine.state))
        ok = mine.step(g, LR, host)
        twin.adam_step(1, ev in ("inf", "nan"))
        assert ls.state == twin.state
        assert ok == (ev == "clean")
        if ok:
            applied += 1
            assert mine.bias_correction_step(host) == applied == mine.adam.applied
        else:
            assert torch.equal(mine.adam.p, before[0]) and mine.state[1] == 0.0 and not math.isfinite(mine.state[0])
            assert mine.state[2] == before[1][2] and mine.state[3] == before[1][3] + (ev == "huge")
    assert ls.state[5] == 2 and ls.state[4] == 0 and mine.state[3] == 2 and applied == 4
    assert norm_f32(torch.tensor([3e38]))[0] == INF and norm_f32(torch.tensor([3.0, 4.0]))[0] == 5.0
