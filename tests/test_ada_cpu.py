"""Adaptive dis_augment probability (config keys dis_augment_p / ada_target / ada_interval / ada_kimg; include/aclgan_hip.h: aclgan_ctx_set_ada,
aclgan_augment_gate) -- everything about it that needs no GPU: the config keys and what they refuse, the shipped configs, the numpy model's own
invariants (tests/ada_ref.py), the exported symbols and the header text, the launch-free queries, the argument checks, and the third generator."""
import ctypes as C
import glob
import os
import types

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT
import ada_ref as R


def _mods():
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib, trainer
    return _lib, trainer


def test_ada_from_config():
    L, T = _mods()
    f = T.ada_from_config
    assert "ada_from_config" in T.__all__
    aug = {"dis_augment": "color,cutout"}
    assert f({}) is None and f(aug) is None
    assert f({"ada_target": "nonsense", "ada_interval": -3, "ada_kimg": 0}) is None          # read only with adaptive
    assert f(dict(aug, dis_augment_p=0.25)) == (0.25, False, 0.6, 4, 500.0)
    assert f(dict(aug, dis_augment_p=0)) == (0.0, False, 0.6, 4, 500.0) and f(dict(aug, dis_augment_p=1)) == (1.0, False, 0.6, 4, 500.0)
    assert f(dict(aug, dis_augment_p=0.5, ada_target="nonsense", ada_interval=-3)) == (0.5, False, 0.6, 4, 500.0)
    assert f(dict(aug, dis_augment_p="adaptive")) == (0.0, True, 0.6, 4, 500.0)              # ADA's defaults
    got = f(dict(aug, dis_augment_p="adaptive", ada_target=-0.25, ada_interval=1, ada_kimg=0.5))
    assert got == (0.0, True, -0.25, 1, 0.5)
    assert [type(v) for v in got] == [float, bool, float, int, float]
    assert f(dict(aug, dis_augment_p="adaptive", ada_target=1, ada_kimg=100))[2:] == (1.0, 4, 100.0)
    for bad in (-0.01, 1.01, float("nan"), float("inf"), True, False, None, "0.5", "adapt", [0.5]):
        with pytest.raises(L.AclganError, match="dis_augment_p"):
            f(dict(aug, dis_augment_p=bad))
    for bad in (-1.01, 1.5, float("nan"), float("inf"), True, "0.6", None):
        with pytest.raises(L.AclganError, match="ada_target"):
            f(dict(aug, dis_augment_p="adaptive", ada_target=bad))
    for bad in (0, -1, 4.0, True, "4", None, 2 ** 31):
        with pytest.raises(L.AclganError, match="ada_interval"):
            f(dict(aug, dis_augment_p="adaptive", ada_interval=bad))
    for bad in (0, -1, float("nan"), float("inf"), 1e39, True, "500", None):
        with pytest.raises(L.AclganError, match="ada_kimg"):
            f(dict(aug, dis_augment_p="adaptive", ada_kimg=bad))
    # the key needs something to apply, and the message says so
    for cfg in ({"dis_augment_p": 0.5}, {"dis_augment_p": "adaptive", "dis_augment": ""}, {"dis_augment_p": 0.0, "dis_augment": "  "}):
        with pytest.raises(L.AclganError, match="needs a non-empty dis_augment"):
            f(cfg)
    # new augmentation operations stay out of scope
    with pytest.raises(L.AclganError):
        f({"dis_augment_p": 0.5, "dis_augment": "color,flip"})


def test_every_shipped_config_leaves_the_key_out():
    L, T = _mods()
    shipped = sorted(glob.glob(os.path.join(ROOT, "configs", "*.yaml")))
    assert len(shipped) >= 7
    for path in shipped:
        cfg = yaml.safe_load(open(path))
        assert T.ada_from_config(cfg) is None, path
        assert not any(k in cfg for k in ("dis_augment_p", "ada_target", "ada_interval", "ada_kimg")), path
    readme = open(os.path.join(ROOT, "README.md")).read()
    flat = readme.lower().replace("\n", " ")
    assert "dis_augment_p: adaptive" in readme and "ada_target" in readme and "nobody has measured" in flat
    assert "per-rank batch" in flat and "drift apart" in flat


def test_model_invariants():
    g = np.random.default_rng(3)
    H, W, n = 20, 13, 64
    rows = g.standard_normal((n, 8)).astype(np.float32)
    u = g.random((n, 4)).astype(np.float32)
    neutral = R.neutral_row(H, W)
    assert neutral.tolist() == [0, 1, 1, 0, 0, W, H, 0]
    for policy in range(1, 8):
        on = [c for bit, cols in R.OPS if policy & bit for c in cols]
        off = [c for c in range(8) if c not in on]
        assert np.array_equal(R.gate(rows, u, 1.0, H, W, policy).view(np.int32), rows.view(np.int32))
        zero = R.gate(rows, u, 0.0, H, W, policy)
        assert np.array_equal(zero[:, off], rows[:, off]) and all(np.array_equal(zero[:, c], np.full(n, neutral[c])) for c in on)
        # strict comparison: a uniform equal to p leaves its operation off; every output element is an input element or a neutral value
        p = u[7, 0]
        mid = R.gate(rows, u, p, H, W, policy)
        if policy & 1:
            assert mid[7, 1] == 1 and np.array_equal(mid[u[:, 0] < p][:, :3], rows[u[:, 0] < p][:, :3])
        assert ((mid == rows) | (mid == neutral[None, :])).all()
    # the sign statistic: exact thirds, the boundary counts as nothing, one NaN poisons the mean
    o = np.array([0.2, 0.5, 0.9, 0.7, 0.5, 0.1], dtype=np.float32)
    assert R.sign_q(o) == 0.0 and R.sign_q(o[:4]) == 0.25 and R.sign_q(np.full(5, 0.5)) == 0.0
    assert np.isnan(R.sign_q(np.array([0.9, np.nan])))
    a, b = R.sign_acc((0, 0), [o[:4], np.ones(3)], [0.5, 1.0])
    assert (a, b) == (np.float32(1.125), np.float32(1.5))
    assert np.isnan(R.sign_acc((0, 0), [np.array([np.nan, 1.0])], [1.0])[0])
    # the fold: r into the interval, p moves when the interval closes, clamps at both ends, step 0 never moves it, a non-finite r is skipped
    s = R.new_state(0.0)
    step = np.float32(0.3)
    for i in range(8):
        s[R.PAIR_A:R.PAIR_A + 2] = (1.0, 1.0)
        s[R.PAIR_B:R.PAIR_B + 2] = (0.5, 1.0)           # r = 0.75 > 0.6
        s = R.fold(s, 0.6, 2, step)
        assert R.readout(s)["updates"] == i + 1 and R.readout(s)["r"] == 0.75 and not s[R.PAIR_A:].any()
    want = np.float32(0)
    for _ in range(3):
        want = want + step
    assert R.readout(s) == {"p": 1.0, "r_t": 0.75, "r": 0.75, "updates": 8, "adjustments": 4} and want < 1
    for i in range(8):
        s[R.PAIR_A:R.PAIR_A + 2] = (-1.0, 1.0)
        s = R.fold(s, 0.6, 2, step)
    assert R.readout(s)["p"] == 0.0 and R.readout(s)["r_t"] == -1.0
    fixed = R.new_state(0.37)
    for i in range(4):
        fixed[R.PAIR_B:R.PAIR_B + 2] = (1.0, 1.0)
        fixed = R.fold(fixed, 0.6, 2, 0.0)
    assert fixed[R.P] == np.float32(0.37) and R.readout(fixed)["r_t"] == 1.0 and R.readout(fixed)["adjustments"] == 2
    before = fixed.copy()
    fixed[R.PAIR_A:R.PAIR_A + 2] = (np.nan, 1.0)
    after = R.fold(fixed, 0.6, 1, 0.5)
    assert after[R.P] == before[R.P] and after[R.R_T] == before[R.R_T] and np.isnan(after[R.R]) and R.readout(after)["updates"] == 5
    assert R.readout(after)["adjustments"] == 2
    empty = R.fold(R.new_state(0.5), 0.6, 1, 0.5)        # an update without a term: 0 / 0
    assert empty[R.P] == 0.5 and np.isnan(empty[R.R])
    exact = R.new_state(0.25)
    exact[R.PAIR_A:R.PAIR_A + 2] = (0.5, 1.0)
    assert R.fold(exact, 0.5, 1, 0.125)[R.P] == 0.25     # r_t == target: sgn(0) = 0


def _ctx(L, scales=3, norm=0):
    a = L.Arch(3, 6, 8, 16, 8, 4, 2, 2, 8, 4, scales)
    ctx = C.c_void_p()
    L.check(L.lib.aclgan_ctx_create_dis_norm(C.byref(a), norm, C.byref(ctx)))
    return ctx


def test_symbols_header_and_state_size_without_gpu():
    L, _ = _mods()
    for name, nargs in (("aclgan_ada_state_floats", 0), ("aclgan_ctx_set_ada", 5), ("aclgan_augment_gate", 9), ("aclgan_ada_sign_multi", 6),
                        ("aclgan_ada_fold", 5)):
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == nargs
        assert getattr(L.lib, name).argtypes is not None
    header = open(os.path.join(ROOT, "include", "aclgan_hip.h")).read()
    for decl in ("size_t aclgan_ada_state_floats(void);",
                 "int aclgan_ctx_set_ada(aclgan_ctx* ctx, float* state, float target, int interval, float step);",
                 "int aclgan_augment_gate(const float* rows, const float* u, const float* state, int n, int H, int W, int policy, float* rows_eff, void* stream);",
                 "int aclgan_ada_sign_multi(const float* const* o, const int* n, const float* weight, int nterms, float* acc, void* stream);",
                 "int aclgan_ada_fold(float* state, float target, int interval, float step, void* stream);"):
        assert decl in header, decl
    for text in ("Karras et al.", "sgn(o - 0.5)", "p = clamp(p + sgn(r_t - target) * step, 0, 1)", "a non-finite r leaves p, r_t and the interval sum as they are",
                 "Slots 8 .. 11 extend the eight published slots", "dis_2 contributes nothing"):
        assert text in header, text
    n0 = L.lib.aclgan_launch_count()
    # the eight published slots and the documented extension: one (sum w q, sum w) pair per real-side discriminator
    assert L.lib.aclgan_ada_state_floats() == R.STATE_FLOATS == 12
    assert L.lib.aclgan_launch_count() == n0


def test_argument_checks_launch_nothing():
    """every refusal is ACLGAN_EINVAL with a message, made before anything is enqueued"""
    L, _ = _mods()
    EINVAL = -1
    n0 = L.lib.aclgan_launch_count()
    ctx = _ctx(L)
    fake, fake2 = C.c_void_p(0x10000), C.c_void_p(0x20000)
    f = L.lib.aclgan_ctx_set_ada
    assert f(None, fake, 0.6, 4, 0.0) == EINVAL
    for target in (-1.5, 1.0001, float("nan"), float("inf")):
        assert f(ctx, fake, target, 4, 0.0) == EINVAL and "target" in L.last_error()
    for interval in (0, -1, -2 ** 31):
        assert f(ctx, fake, 0.6, interval, 0.0) == EINVAL and "interval" in L.last_error()
    for step in (-1e-9, float("nan"), float("inf")):
        assert f(ctx, fake, 0.6, 4, step) == EINVAL and "step" in L.last_error()
        assert f(ctx, None, 0.6, 4, step) == EINVAL
    assert f(ctx, fake, -1.0, 1, 0.0) == 0 and f(ctx, fake, 1.0, 2 ** 31 - 1, 1.0) == 0 and f(ctx, None, 0.6, 4, 0.0) == 0
    g = L.lib.aclgan_augment_gate
    ok = [fake, fake, fake, 5, 64, 64, 7, fake2, None]
    for i in (0, 1, 2, 7):
        args = list(ok)
        args[i] = None
        assert g(*args) == EINVAL and "null" in L.last_error(), i
    for i, v in ((3, 0), (3, -1), (4, 0), (5, 0), (6, 0), (6, 8), (6, -1), (7, fake)):
        args = list(ok)
        args[i] = v
        assert g(*args) == EINVAL, (i, v)
    m = L.lib.aclgan_ada_sign_multi
    arr, n, w = (C.c_void_p * 1)(0x10000), (C.c_int * 1)(4), (C.c_float * 1)(1.0)
    ok = [arr, n, w, 1, fake, None]
    for i in (0, 1, 2, 4):
        args = list(ok)
        args[i] = None
        assert m(*args) == EINVAL, i
    for i, v in ((3, 0), (3, 1025), (0, (C.c_void_p * 1)(None)), (1, (C.c_int * 1)(0)), (2, (C.c_float * 1)(-1.0)), (2, (C.c_float * 1)(float("nan")))):
        args = list(ok)
        args[i] = v
        assert m(*args) == EINVAL, (i, v)
    h = L.lib.aclgan_ada_fold
    assert h(None, 0.6, 4, 0.0, None) == EINVAL
    for args in ((fake, 2.0, 4, 0.0), (fake, float("nan"), 4, 0.0), (fake, 0.6, 0, 0.0), (fake, 0.6, 4, -1.0), (fake, 0.6, 4, float("inf"))):
        assert h(*args, None) == EINVAL, args
    L.lib.aclgan_ctx_destroy(ctx)
    assert L.lib.aclgan_launch_count() == n0


@pytest.mark.parametrize("norm", [0, 4])
def test_dry_runs_count_the_new_launches(norm):
    """with a state bound the algorithmic bytes of dis_update grow by the sign launches' (every real-side map read once, the pair read and
    written) and the fold's (the state read and written once); gen_update's, the executed FLOPs and the workspace do not move; unbinding
    restores every figure.  dis.norm sn runs the real side of dis_A twice (one pass per reference call)."""
    L, _ = _mods()
    n0 = L.lib.aclgan_launch_count()
    ctx = _ctx(L, norm=norm)
    fake = C.c_void_p(0x10000)
    for grp in (0, 1):
        L.check(L.lib.aclgan_bind_params(ctx, grp, fake, fake, fake, fake))
    if norm:
        L.check(L.lib.aclgan_bind_sn_state(ctx, fake))

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
    L.check(L.lib.aclgan_ctx_set_ada(ctx, fake, 0.6, 4, 0.001))
    on = q()
    assert on[0] == off[0] and on[1] == off[1] and on[2] == off[2] and on[4] == off[4]
    # n_layer 4 at 64x64: the three scales' maps are 4x4, 2x2 and 1x1 per image, B = 2
    maps = 2 * (16 + 4 + 1)
    passes = 3 if norm else 2
    assert on[3] - off[3] == passes * (4 * maps + 16) + 2 * 4 * 12
    L.check(L.lib.aclgan_ctx_set_ada(ctx, None, 0.6, 4, 0.001))
    assert q() == off
    L.lib.aclgan_ctx_destroy(ctx)
    assert L.lib.aclgan_launch_count() == n0


def test_the_third_generator_moves_no_other_stream():
    """the gate's uniforms come from a generator seeded initial_seed() + rank + 0x0A08: with and without draws from it, the z stream (the
    default CPU generator) and the augmentation rows' stream (their own generator) give the same tensors"""
    L, T = _mods()
    assert (T.AUG_SEED_OFFSET, T.MS_SEED_OFFSET, T.ADA_SEED_OFFSET) == (0x0A06, 0x0A07, 0x0A08)
    Tr = T.aclgan_Trainer

    def run(with_u):
        torch.manual_seed(123)
        stub = types.SimpleNamespace(_adagen=None, _auggen=None, augment=7, _dist_world=lambda: 0)
        z, rows, us = [], [], []
        for _ in range(3):
            rows.append(Tr._draw_augment(stub, "dis", 2, 64, 64))
            if with_u:
                us.append(Tr._draw_aug_u(stub, 14))
            z.append(torch.randn(2, 8, 1, 1))
        return z, rows, us
    z0, rows0, _ = run(False)
    z1, rows1, us = run(True)
    assert all(torch.equal(a, b) for a, b in zip(z0 + rows0, z1 + rows1))
    assert all(u.shape == (14, 4) and u.dtype == torch.float32 and 0 <= float(u.min()) and float(u.max()) < 1 for u in us)
    assert not torch.equal(us[0], us[1])
    torch.manual_seed(123)
    want = torch.rand(14, 4, generator=torch.Generator().manual_seed(123 + 0x0A08))
    assert torch.equal(us[0], want)
