"""Differentiable augmentation of the discriminator inputs (config key dis_augment; include/aclgan_hip.h: aclgan_ctx_set_augment,
aclgan_diffaugment_fwd / _bwd) -- everything about it that needs no GPU: the config key, the parameter draws, the fp64 reference the GPU
tests compare against (tests/diffaug_ref.py), the exported symbols, the argument checks and the launch-free dry runs of the scheduler."""
import ctypes as C
import glob
import os

import pytest
import torch
import yaml

from conftest import ROOT
from diffaug_ref import diffaug_bwd_ref, diffaug_ref, neutral_params


def _mods():
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib, trainer
    return _lib, trainer


def test_augment_from_config():
    L, T = _mods()
    f = T.augment_from_config
    assert f({}) == 0 and f({"dis_augment": ""}) == 0 and f({"dis_augment": "  "}) == 0
    assert (f({"dis_augment": "color"}), f({"dis_augment": "translation"}), f({"dis_augment": "cutout"})) == (1, 2, 4)
    assert (L.AUG["color"], L.AUG["translation"], L.AUG["cutout"]) == (1, 2, 4)
    names = ("color", "translation", "cutout")
    for bits in range(8):
        sub = [n for i, n in enumerate(names) if bits >> i & 1]
        assert f({"dis_augment": ",".join(sub)}) == bits
        assert f({"dis_augment": ", ".join(reversed(sub))}) == bits
    for bad in ("colour", "color,flip", "color,color", "color,,cutout", ",", 7, None, True, ["color"]):
        with pytest.raises(L.AclganError):
            f({"dis_augment": bad})
    # every shipped config but the augmented one leaves it off; that one is selfie2anime.yaml plus the key
    shipped = sorted(glob.glob(os.path.join(ROOT, "configs", "*.yaml")))
    assert len(shipped) >= 5
    for path in shipped:
        want = 7 if path.endswith("selfie2anime_diffaug.yaml") else 0
        assert f(yaml.safe_load(open(path))) == want, path
    base = yaml.safe_load(open(os.path.join(ROOT, "configs", "selfie2anime.yaml")))
    aug = yaml.safe_load(open(os.path.join(ROOT, "configs", "selfie2anime_diffaug.yaml")))
    assert aug.pop("dis_augment") == "color,translation,cutout" and aug == base


def test_draw_augment_params():
    L, T = _mods()
    H, W, rows = 20, 13, 4000
    g = torch.Generator().manual_seed(5)
    p = T.draw_augment_params(7, rows, H, W, g)
    assert p.shape == (rows, 8) and p.dtype == torch.float32 and p.device.type == "cpu"
    b, s, c, tx, ty, cx, cy, pad = p.unbind(1)
    assert -0.5 <= b.min() < -0.45 and 0.45 < b.max() < 0.5
    assert 0 <= s.min() < 0.1 and 1.9 < s.max() < 2
    assert 0.5 <= c.min() < 0.55 and 1.45 < c.max() < 1.5
    for col in (tx, ty, cx, cy):
        assert torch.equal(col, col.round())
    sx, sy = int(W / 8 + 0.5), int(H / 8 + 0.5)      # 2, 3 (20 / 8 + 0.5 = 3.0)
    assert (sx, sy) == (2, 3)
    assert set(tx.tolist()) == set(range(-sx, sx + 1)) and set(ty.tolist()) == set(range(-sy, sy + 1))
    ch, cw = (H + 1) // 2, (W + 1) // 2              # 10, 7
    assert set(cy.tolist()) == set(o - ch // 2 for o in range(0, H + (1 - ch % 2)))      # oy in [0, 21)
    assert set(cx.tolist()) == set(o - cw // 2 for o in range(0, W + (1 - cw % 2)))      # ox in [0, 13)
    assert float(pad.abs().max()) == 0
    # operations that are off hold their neutral values, whatever else is on
    neutral = neutral_params(64, H, W)
    assert torch.equal(T.draw_augment_params(0, 64, H, W, g), neutral)
    for policy in range(1, 8):
        q = T.draw_augment_params(policy, 64, H, W, g)
        for bit, cols in ((1, (0, 1, 2)), (2, (3, 4)), (4, (5, 6))):
            same = all(torch.equal(q[:, k], neutral[:, k]) for k in cols)
            assert same == (not policy & bit), (policy, bit)
    # neutral rows are the identity of the reference under every policy
    x = torch.randn(3, 6, 9, 7, dtype=torch.float64)
    for policy in range(1, 8):
        assert (diffaug_ref(x, neutral_params(3, 9, 7), policy) - x).abs().max() < 1e-15
    # the same seed gives the same tensor
    a = T.draw_augment_params(7, 21, 64, 96, torch.Generator().manual_seed(11))
    assert torch.equal(a, T.draw_augment_params(7, 21, 64, 96, torch.Generator().manual_seed(11)))
    assert not torch.equal(a, T.draw_augment_params(7, 21, 64, 96, torch.Generator().manual_seed(12)))
    # the draws come from their own generator: the z stream (the default CPU generator, trainer.py:99-101) does not move
    torch.manual_seed(123)
    z0 = [torch.randn(3, 8, 1, 1) for _ in range(3)]
    torch.manual_seed(123)
    z1 = []
    for _ in range(3):
        T.draw_augment_params(7, 21, 64, 96, g)
        z1.append(torch.randn(3, 8, 1, 1))
    assert all(torch.equal(u, v) for u, v in zip(z0, z1))
    with pytest.raises(L.AclganError):
        T.draw_augment_params(8, 4, 8, 8, g)


def _extreme_rows(H, W):
    sx, sy, ch, cw = int(W / 8 + 0.5), int(H / 8 + 0.5), (H + 1) // 2, (W + 1) // 2
    return torch.tensor([[0.3, 0.0, 0.5, sx, sy, -(cw // 2), -(ch // 2), 0],
                         [-0.4, 1.7, 1.4, -sx, -sy, W - cw % 2 - cw // 2, H - ch % 2 - ch // 2, 0],
                         [0.1, 0.6, 0.5, 0, 0, W, H, 0]], dtype=torch.float64)


def test_reference_backward_is_the_adjoint():
    """the analytic backward the kernels implement == autograd of the forward formulas, fp64, 1e-12"""
    g = torch.Generator().manual_seed(3)
    for (N, Cc, H, W) in ((3, 3, 10, 7), (3, 6, 7, 9)):
        p = _extreme_rows(H, W)
        for policy in range(1, 8):
            x = torch.randn(N, Cc, H, W, generator=g, dtype=torch.float64, requires_grad=True)
            dy = torch.randn(N, Cc, H, W, generator=g, dtype=torch.float64)
            y = diffaug_ref(x, p, policy)
            y.backward(dy)
            ref = x.grad
            x, y = x.detach(), y.detach()
            got = diffaug_bwd_ref(dy, p, policy)
            assert (got - ref).abs().max() <= 1e-12 * ref.abs().max(), (N, Cc, policy)
            # and the forward does what its description says at the extremes: shifted-out borders and the rectangle are exactly zero
            if policy & 4:      # (row 0: the rectangle hangs over the top left corner)
                ch, cw = (H + 1) // 2, (W + 1) // 2
                assert float(y[0, :, :ch - ch // 2, :cw - cw // 2].abs().max()) == 0
            if policy == 4:
                assert torch.equal(y[0, :, ch - ch // 2:], x[0, :, ch - ch // 2:]) and torch.equal(y[2], x[2])
            if policy == 2:
                sx, sy = int(W / 8 + 0.5), int(H / 8 + 0.5)
                assert torch.equal(y[0, :, :H - sy, :W - sx], x[0, :, sy:, sx:]) and float(y[0, :, H - sy:].abs().max()) == 0


def test_new_symbols_are_exported_and_bound():
    L, _ = _mods()
    for name, nargs in (("aclgan_ctx_set_augment", 4), ("aclgan_diffaugment_scratch_bytes", 4), ("aclgan_diffaugment_fwd", 10),
                        ("aclgan_diffaugment_bwd", 11)):
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == nargs
        assert getattr(L.lib, name).argtypes is not None
    # partial sums: one float per (sample, group, slice of <= 1024 pixels up to 64 slices)
    sb = L.lib.aclgan_diffaugment_scratch_bytes
    assert sb(16, 256, 256, 3) == 16 * 64 * 4 and sb(16, 256, 256, 6) == 2 * 16 * 64 * 4 and sb(2, 7, 9, 6) == 2 * 2 * 4
    assert sb(2, 8, 8, 4) == 0


def test_operator_argument_checks_without_gpu():
    """bad arguments are codes with messages, and nothing is launched"""
    L, _ = _mods()
    n0 = L.lib.aclgan_launch_count()
    fake = C.c_void_p(0x10000)
    fake2 = C.c_void_p(0x20000)
    fwd, bwd = L.lib.aclgan_diffaugment_fwd, L.lib.aclgan_diffaugment_bwd
    for Cc in (1, 4, 9):
        assert fwd(2, 8, 8, Cc, 7, fake, fake, fake2, fake, None) == -1 and "C = %d" % Cc in L.last_error()
        assert bwd(2, 8, 8, Cc, 7, fake, fake, fake2, 0, fake, None) == -1
    for policy in (0, 8, -1):
        assert fwd(2, 8, 8, 3, policy, fake, fake, fake2, fake, None) == -1 and "policy" in L.last_error()
        assert bwd(2, 8, 8, 3, policy, fake, fake, fake2, 1, fake, None) == -1
    for args in ((None, fake, fake2), (fake, None, fake2), (fake, fake, None)):
        assert fwd(2, 8, 8, 6, 7, args[0], args[1], args[2], fake, None) == -1 and "null" in L.last_error()
        assert bwd(2, 8, 8, 6, 7, args[0], args[1], args[2], 0, fake, None) == -1
    assert fwd(2, 8, 8, 3, 1, fake, fake, fake2, None, None) == -1 and "scratch" in L.last_error()      # colour needs its partials
    assert fwd(2, 8, 8, 3, 6, fake, fake, fake, None, None) == -1 and "alias" in L.last_error()
    ctx = C.c_void_p()
    a = L.Arch(3, 6, 8, 16, 8, 4, 2, 2, 8, 4, 3)
    L.check(L.lib.aclgan_ctx_create(C.byref(a), C.byref(ctx)))
    assert L.lib.aclgan_ctx_set_augment(ctx, 8, None, 0) == -1 and "policy" in L.last_error()
    assert L.lib.aclgan_ctx_set_augment(ctx, -1, None, 0) == -1
    assert L.lib.aclgan_ctx_set_augment(None, 7, None, 0) == -1
    assert L.lib.aclgan_ctx_set_augment(ctx, 7, None, 0) == 0 and L.lib.aclgan_ctx_set_augment(ctx, 0, None, 0) == 0
    L.lib.aclgan_ctx_destroy(ctx)
    assert L.lib.aclgan_launch_count() == n0


@pytest.mark.parametrize("dtype", [0, 1])
def test_dry_runs_account_for_the_augmented_tensors(dtype):
    """policy 7 on a context, B=2 at 64x64, against policy 0: the workspace holds the augmented tensors and their gradients, the
    algorithmic bytes grow, the matrix-pipe FLOPs do not move -- and policy 0 again gives back exactly the first numbers"""
    L, _ = _mods()
    n0 = L.lib.aclgan_launch_count()
    B, S = 2, 64
    a = L.Arch(3, 6, 8, 16, 8, 4, 2, 2, 8, 4, 3)
    ctx = C.c_void_p()
    L.check(L.lib.aclgan_ctx_create(C.byref(a), C.byref(ctx)))
    L.check(L.lib.aclgan_set_compute_dtype(ctx, dtype))
    fake = C.c_void_p(0x10000)
    for grp in (0, 1):
        L.check(L.lib.aclgan_bind_params(ctx, grp, fake, fake, fake, fake))
        if dtype:
            L.check(L.lib.aclgan_bind_params16(ctx, grp, fake, fake))

    def q():
        ws = C.c_size_t()
        L.check(L.lib.aclgan_workspace_bytes(ctx, B, S, S, C.byref(ws)))
        out = {"ws": ws.value}
        for which in (0, 1):
            v = C.c_double()
            L.check(L.lib.aclgan_step_algorithmic_bytes(ctx, which, B, S, S, C.byref(v)))
            out["bytes%d" % which] = v.value
            L.check(L.lib.aclgan_step_executed_flops(ctx, which, B, S, S, C.byref(v)))
            out["flops%d" % which] = v.value
        return out
    off = q()
    L.check(L.lib.aclgan_ctx_set_augment(ctx, 7, None, 0))
    on = q()
    L.check(L.lib.aclgan_ctx_set_augment(ctx, 0, None, 0))
    assert q() == off
    # gen_update augments x_A_fake, x_A2_fake, x_B_fake (3 channels) and pair_A1, pair_A2 (6): 21 B H W floats, and as many of gradient;
    # dis_update 27 B H W floats (x_a and x_b too) without gradients -- fp32 in every compute dtype
    img = B * S * S * 4
    assert on["ws"] - off["ws"] >= 2 * 21 * img
    assert on["bytes0"] - off["bytes0"] == 2 * 2 * 21 * img      # forward and backward, each tensor read once and written once
    assert on["bytes1"] - off["bytes1"] == 2 * 27 * img
    assert on["flops0"] == off["flops0"] and on["flops1"] == off["flops1"]
    L.lib.aclgan_ctx_destroy(ctx)
    assert L.lib.aclgan_launch_count() == n0
