"""Mode-seeking regulariser of the generators (config key ms_lambda; include/aclgan_hip.h: aclgan_modeseek / aclgan_ctx_set_modeseek) --
everything about it that needs no GPU: the config key and what it refuses, the shipped configs, the exported symbols and the header text,
the argument checks, the launch-free queries, and the fp64 model of tests/modeseek_ref.py against the closed-form seeds."""
import ctypes as C
import glob
import os

import pytest
import torch
import yaml

from conftest import ROOT
from modeseek_ref import EPS, ms_seeds, ms_terms, ms_value


def _mods():
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib, trainer
    return _lib, trainer


def test_modeseek_from_config():
    L, T = _mods()
    f = T.modeseek_from_config
    assert "modeseek_from_config" in T.__all__
    assert f({}) == 0.0 and f({"ms_lambda": 0}) == 0.0 and f({"ms_lambda": 1}) == 1.0 and f({"ms_lambda": 0.25}) == 0.25
    assert isinstance(f({"ms_lambda": 1}), float)
    for bad in (-1, -0.0001, float("nan"), float("inf"), 1e39, "1.0", None, True, False, [1.0]):
        with pytest.raises(L.AclganError, match="ms_lambda"):
            f({"ms_lambda": bad})
    # it composes with every other key: nothing is refused
    assert f({"dis": {"norm": "sn"}, "dis_augment": "color", "r1_gamma": 0, "lecam_lambda": 1.0, "ema_decay": 0.999, "grad_clip": 1.5, "ms_lambda": 2.0}) == 2.0


def test_shipped_configs():
    """only selfie2anime_modeseek.yaml turns the key on, and it is selfie2anime.yaml plus the key"""
    L, T = _mods()
    shipped = sorted(glob.glob(os.path.join(ROOT, "configs", "*.yaml")))
    assert len(shipped) >= 8
    for path in shipped:
        cfg = yaml.safe_load(open(path))
        assert (T.modeseek_from_config(cfg) > 0) == path.endswith("selfie2anime_modeseek.yaml"), path
    base = yaml.safe_load(open(os.path.join(ROOT, "configs", "selfie2anime.yaml")))
    ms = yaml.safe_load(open(os.path.join(ROOT, "configs", "selfie2anime_modeseek.yaml")))
    assert ms.pop("ms_lambda") == 1.0 and ms == base
    assert T.augment_from_config(ms) == 0 and T.r1_from_config(ms)[0] == 0 and T.ema_from_config(ms)[0] == 0 and T.lecam_from_config(ms)[0] == 0
    readme = open(os.path.join(ROOT, "README.md")).read()
    flat = readme.lower().replace("\n", " ")
    assert "ms_lambda" in readme and "Mode-seeking" in readme and "nobody has measured" in flat and "grad_clip" in readme
    assert "modeseek.hip" in readme and "not stored in checkpoints" in flat
    assert "4g" in open(os.path.join(ROOT, "DESIGN.md")).read()


def _ctx(L):
    a = L.Arch(3, 6, 8, 16, 8, 4, 2, 2, 8, 4, 3)
    ctx = C.c_void_p()
    L.check(L.lib.aclgan_ctx_create_dis_norm(C.byref(a), 0, C.byref(ctx)))
    return ctx


def test_symbols_and_header():
    L, _ = _mods()
    for name, nargs in (("aclgan_modeseek_scratch_bytes", 2), ("aclgan_modeseek", 16), ("aclgan_ctx_set_modeseek", 5)):
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == nargs
        assert getattr(L.lib, name).argtypes is not None
    header = open(os.path.join(ROOT, "include", "aclgan_hip.h")).read()
    assert "size_t aclgan_modeseek_scratch_bytes(int B, int64_t n_per_image);" in header
    assert "int aclgan_ctx_set_modeseek(aclgan_ctx* ctx, float lambda, const float* z_extra, int rows, float* out8);" in header
    assert "int aclgan_modeseek(const float* a, const float* b, int B, int64_t n_per_image, const float* u, const float* u2, int style_dim, float u_scale," in header
    for text in ("ms_b = dz_b / (dI_b + eps * dz_b),  eps = 1e-5", "Mao et al.", "sign(0) = 0", "rows must be 2 B"):
        assert text in header, text
    # the decomposition the header documents: one partial per (image, chunk), chunks = min(128, max(1, ceil((n / 4) / 512)))
    n0 = L.lib.aclgan_launch_count()
    for B, n in ((1, 1), (1, 2051), (1, 2052), (3, 3 * 64 * 64), (8, 3 * 256 * 256), (2, 3 * 1024 * 1024)):
        chunks = min(128, max(1, -(-(n // 4) // 512)))
        assert L.lib.aclgan_modeseek_scratch_bytes(B, n) == 4 * B * chunks, (B, n)
    assert L.lib.aclgan_modeseek_scratch_bytes(0, 16) == 0 and L.lib.aclgan_modeseek_scratch_bytes(1, 0) == 0
    assert L.lib.aclgan_launch_count() == n0


def test_argument_checks_launch_nothing():
    """every refusal is ACLGAN_EINVAL with a message, made before anything is enqueued"""
    L, _ = _mods()
    EINVAL = -1
    n0 = L.lib.aclgan_launch_count()
    ctx = _ctx(L)
    f = L.lib.aclgan_ctx_set_modeseek
    fake = C.c_void_p(0x10000)
    assert f(None, 1.0, fake, 4, fake) == EINVAL
    for lam in (-1.0, -1e-30, float("nan"), float("inf"), -float("inf")):
        assert f(ctx, lam, fake, 4, fake) == EINVAL and "lambda" in L.last_error()
        assert f(ctx, lam, None, 0, None) == EINVAL
    assert f(ctx, 1.0, fake, -1, fake) == EINVAL and "rows" in L.last_error()
    assert f(ctx, 1.0, fake, 4, None) == EINVAL and "out8" in L.last_error()
    assert f(ctx, 1.0, fake, 4, fake) == 0 and f(ctx, 0.0, fake, 4, fake) == 0 and f(ctx, 1.0, None, 0, None) == 0 and f(ctx, 0.0, None, 0, None) == 0
    # the operator
    m = L.lib.aclgan_modeseek
    ok = [fake, fake, 2, 48, fake, fake, 8, 1.0, 0.5, None, fake, fake, fake, 0, fake, None]
    for i in (0, 1, 4, 5, 10, 14):                      # a null image / noise / output / scratch
        args = list(ok)
        args[i] = None
        assert m(*args) == EINVAL and "null" in L.last_error(), i
    for i, v in ((2, 0), (2, 65536), (3, 0), (6, 0), (8, -1.0), (8, float("nan")), (8, float("inf")), (7, float("nan")), (0, C.c_void_p(0x10002)), (11, C.c_void_p(0x10001))):
        args = list(ok)
        args[i] = v
        assert m(*args) == EINVAL, (i, v)
    L.lib.aclgan_ctx_destroy(ctx)
    assert L.lib.aclgan_launch_count() == n0


def test_dry_runs_count_the_two_passes():
    """with the feature on, gen_update's workspace, algorithmic bytes and executed FLOPs grow (two decoder passes, two blends, four launches);
    dis_update's do not move; switching it off again restores every figure of a context that was never configured"""
    L, _ = _mods()
    n0 = L.lib.aclgan_launch_count()
    ctx, never = _ctx(L), _ctx(L)
    fake = C.c_void_p(0x10000)
    for c in (ctx, never):
        for grp in (0, 1):
            L.check(L.lib.aclgan_bind_params(c, grp, fake, fake, fake, fake))

    def q(c):
        ws, out = C.c_size_t(), []
        L.check(L.lib.aclgan_workspace_bytes(c, 2, 64, 64, C.byref(ws)))
        for which in (0, 1):
            v, w = C.c_double(), C.c_double()
            L.check(L.lib.aclgan_step_algorithmic_bytes(c, which, 2, 64, 64, C.byref(v)))
            L.check(L.lib.aclgan_step_executed_flops(c, which, 2, 64, 64, C.byref(w)))
            out += [v.value, w.value]
        return [ws.value] + out
    off = q(ctx)
    assert off == q(never)
    L.check(L.lib.aclgan_ctx_set_modeseek(ctx, 1.0, fake, 0, fake))      # (rows is checked by the update, not by the queries)
    on = q(ctx)
    assert on[0] > off[0] and on[1] > off[1] and on[2] > off[2]
    assert on[3] == off[3] and on[4] == off[4]
    # the streaming kernels' own share: I, I' read twice, dI read and written, dI' written, per direction (fp32 images of N = 3 * 64 * 64, B = 2),
    # on top of two decoder passes that are counted like the update's other decoder passes
    assert on[1] - off[1] > 2 * 4 * 7 * 2 * 3 * 64 * 64
    L.check(L.lib.aclgan_ctx_set_modeseek(ctx, 0.0, fake, 4, fake))
    assert q(ctx) == off
    L.check(L.lib.aclgan_ctx_set_modeseek(ctx, 1.0, fake, 4, fake))
    L.check(L.lib.aclgan_ctx_set_modeseek(ctx, 1.0, None, 0, None))
    assert q(ctx) == off == q(never)
    L.lib.aclgan_ctx_destroy(ctx)
    L.lib.aclgan_ctx_destroy(never)
    assert L.lib.aclgan_launch_count() == n0


def _pair(B=4, shape=(3, 5, 7), sd=8, seed=0):
    g = torch.Generator().manual_seed(seed)
    I = (torch.rand(B, *shape, generator=g, dtype=torch.float64) * 2 - 1).requires_grad_(True)
    I2 = (torch.rand(B, *shape, generator=g, dtype=torch.float64) * 2 - 1).requires_grad_(True)
    u = torch.randn(B, sd, 1, 1, generator=g, dtype=torch.float64)
    u2 = torch.randn(B, sd, 1, 1, generator=g, dtype=torch.float64)
    return I, I2, u, u2


def test_autograd_gradient_is_the_closed_form():
    lam = 0.7
    I, I2, u, u2 = _pair()
    with torch.no_grad():
        I2[1, 0, 0, :3] = I[1, 0, 0, :3]            # sign(0) = 0
    ms, div = ms_value(I, I2, u, u2)
    (lam * ms).backward()
    gI, gI2, k = ms_seeds(I.detach(), I2.detach(), u, u2, lam)
    assert float((I.grad - gI).abs().max()) <= 1e-12 and float((I2.grad - gI2).abs().max()) <= 1e-12
    assert float(I.grad[1, 0, 0, :3].abs().max()) == 0.0
    # the definition written out
    dI = (I.detach() - I2.detach()).abs().flatten(1).mean(1)
    dz = (u - u2).abs().flatten(1).mean(1)
    assert abs(float(ms) - float((dz / (dI + EPS * dz)).mean())) <= 1e-12 and abs(float(div) - float((dI / dz).mean())) <= 1e-12
    assert float((k - lam / 4 * dz / (dI + EPS * dz) ** 2 / I[0].numel()).abs().max()) <= 1e-12
    # under a loss scale the seeds are S times these
    assert float((ms_seeds(I.detach(), I2.detach(), u, u2, lam, S=1024.0)[0] - 1024.0 * gI).abs().max()) <= 1e-9


def test_degenerate_rows_are_finite():
    """dz_b == 0 gives ms_b = div_b = 0 and no gradient; I == I' gives the finite value 1 / eps and no gradient (sign(0) = 0)"""
    I, I2, u, u2 = _pair()
    u2 = u2.clone()
    u2[0] = u[0]
    with torch.no_grad():
        I2[2] = I[2]
        I2[3] = I[3]
        u2[3] = u[3]                                 # both at once
    dI, dz, ms_b, div_b = ms_terms(I, I2, u, u2)
    assert float(dz[0]) == 0 and float(ms_b[0]) == 0 and float(div_b[0]) == 0
    assert float(dI[2]) == 0 and abs(float(ms_b[2]) - 1 / EPS) <= 1e-6 and float(div_b[2]) == 0
    assert float(ms_b[3]) == 0 and float(div_b[3]) == 0
    ms, div = ms_value(I, I2, u, u2)
    assert torch.isfinite(ms) and torch.isfinite(div)
    ms.backward()
    assert torch.isfinite(I.grad).all() and torch.isfinite(I2.grad).all()
    for b in (0, 2, 3):
        assert float(I.grad[b].abs().max()) == 0 and float(I2.grad[b].abs().max()) == 0
    assert float(I.grad[1].abs().max()) > 0
    gI, gI2, k = ms_seeds(I.detach(), I2.detach(), u, u2, 1.0)
    assert float((I.grad - gI).abs().max()) <= 1e-12 and torch.isfinite(k).all()


def test_batch_of_four_is_the_average_of_two_shards():
    """the per-image form: what makes a data-parallel run (each rank its equal shard, the gradient all-reduce averaging the ranks) one process
    on the joint batch"""
    lam = 1.3
    I, I2, u, u2 = _pair(B=4, seed=3)
    ms, div = ms_value(I, I2, u, u2)
    (lam * ms).backward()
    vals, divs, gI, gI2 = [], [], [], []
    for sl in (slice(0, 2), slice(2, 4)):
        a, b = I.detach()[sl].clone().requires_grad_(True), I2.detach()[sl].clone().requires_grad_(True)
        m, d = ms_value(a, b, u[sl], u2[sl])
        (lam * m).backward()
        vals.append(m.detach()); divs.append(d.detach()); gI.append(a.grad); gI2.append(b.grad)
    assert abs(float(ms) - float(sum(vals) / 2)) <= 1e-12 and abs(float(div) - float(sum(divs) / 2)) <= 1e-12
    # a rank's gradient is for ITS mean; the all-reduce averages the ranks: each shard's rows carry half their weight in the joint batch
    assert float((I.grad - torch.cat(gI) / 2).abs().max()) <= 1e-12 and float((I2.grad - torch.cat(gI2) / 2).abs().max()) <= 1e-12
