"""R1 gradient penalty on real images (config keys r1_gamma / r1_every; include/aclgan_hip.h: aclgan_dis_r1) -- everything about it that
needs no GPU: the closed form the library computes against the fp64 double backward of the definition (tests/r1_ref.py), the config keys
and what they refuse, the exported symbols, the launch-free scratch query and the argument checks."""
import ctypes as C
import glob
import os

import pytest
import torch
import yaml

from conftest import ROOT
from oracle import aclgan_oracle as O
from r1_ref import dis_cfg, r1_autograd, r1_closed_form, separated_biases


def _mods():
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib, trainer
    return _lib, trainer


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("case", [(8, 2, 2, 24, 40, 3), (4, 4, 3, 64, 64, 3), (4, 4, 3, 64, 64, 6)])
def test_closed_form_is_the_double_backward(case):
    """fp64, four seeds, B=2: P, G and every weight gradient of the closed form agree with autograd.grad(create_graph=True) through the
    oracle's dis_forward to 1e-12 (observed: 6e-16), and every bias gradient of both is exactly zero"""
    dim, nl, S, H, W, Cin = case
    dcfg = dis_cfg(dim, nl, S)
    worst = 0.0
    for seed in range(4):
        P = O.seeded_fill(O.dis_param_shapes(Cin, dcfg), "gaussian", seed)
        x = torch.rand(2, Cin, H, W, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 2 - 1
        p0, G0, g0 = r1_autograd(P, x, dcfg, 10.0)
        p1, G1, g1, margin = r1_closed_form(P, x, dcfg, 10.0)
        assert float(p0) > 0 and margin > 0
        errs = [abs(float(p1 - p0)) / float(p0), _rel(G1, G0)] + [_rel(g1[k], g0[k]) for k in g0 if k.endswith("weight")]
        worst = max(worst, max(errs))
        assert max(errs) <= 1e-12, (case, seed, errs)
        assert all(float(g0[k].abs().max()) > 0 for k in g0 if k.endswith("weight"))
        for k in g0:
            if k.endswith("bias"):
                assert float(g0[k].abs().max()) == 0 and float(g1[k].abs().max()) == 0, k
        # the loss scale is a factor of the gradients alone
        p2, _, g2, _ = r1_closed_form(P, x, dcfg, 10.0, scale=256.0)
        assert float(p2) == float(p1) and all(_rel(g2[k], 256.0 * g1[k]) <= 1e-14 for k in g1 if k.endswith("weight"))
    print("closed form vs double backward %s: worst rel_err %.2e" % (case, worst))


def test_separated_biases_keep_pre_activations_off_zero():
    """the fixture of the full-width GPU case, at a small width: biases of 4 x the layer's rms with a random sign per channel give a
    margin far above gaussian weights', both slopes occur, and the closed form still is the double backward"""
    dcfg = dis_cfg(8, 3, 2)
    P = O.seeded_fill(O.dis_param_shapes(3, dcfg), "gaussian", 1)
    x = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(1), dtype=torch.float64) * 2 - 1
    Q = separated_biases(P, x, dcfg, 4.0, 7)
    assert all(torch.equal(Q[k], P[k]) for k in P if k.endswith("weight"))
    _, _, _, m0 = r1_closed_form(P, x, dcfg, 1.0)
    p1, G1, g1, m1 = r1_closed_form(Q, x, dcfg, 1.0)
    assert m1 >= 1e-2 and m1 > 10 * m0       # (|z| >= 4 rms - |z without bias|: a 3.9-sigma tail still leaves 0.1 rms)
    signs = torch.cat([Q["cnns.0.%d.conv.bias" % l].sign() for l in range(3)])
    assert (signs > 0).any() and (signs < 0).any()
    p0, G0, g0 = r1_autograd(Q, x, dcfg, 1.0)
    assert _rel(G1, G0) <= 1e-12 and all(_rel(g1[k], g0[k]) <= 1e-12 for k in g0 if k.endswith("weight"))


def test_r1_from_config():
    L, T = _mods()
    f = T.r1_from_config
    assert "r1_from_config" in T.__all__
    assert f({}) == (0.0, 16) and f({"r1_gamma": 0}) == (0.0, 16) and f({"r1_gamma": 10}) == (10.0, 16)
    assert f({"r1_gamma": 0.5, "r1_every": 1}) == (0.5, 1) and f({"r1_every": 4}) == (0.0, 4)
    assert isinstance(f({"r1_gamma": 1})[0], float) and isinstance(f({"r1_gamma": 1.0, "r1_every": 3})[1], int)
    for bad in (-1, -0.0001, float("nan"), float("inf"), 1e39, "10", None, True, [1.0]):
        with pytest.raises(L.AclganError, match="r1_gamma"):
            f({"r1_gamma": bad})
    for bad in (0, -1, 1.0, 16.0, "16", None, True):
        with pytest.raises(L.AclganError, match="r1_every"):
            f({"r1_gamma": 1.0, "r1_every": bad})
        with pytest.raises(L.AclganError, match="r1_every"):
            f({"r1_every": bad})                              # checked with the penalty off too
    with pytest.raises(L.AclganError):
        f({"r1_gamma": 3e38, "r1_every": 16})                 # gamma * every is what the library gets
    # refusals: spectral normalisation and differentiable augmentation, only with the penalty on
    for extra, word in (({"dis": {"norm": "sn"}}, "sn"), ({"dis_augment": "color"}, "dis_augment")):
        assert f(dict(extra, r1_gamma=0)) == (0.0, 16)
        with pytest.raises(L.AclganError, match=word) as e:
            f(dict(extra, r1_gamma=1.0))
        assert "follow-up" in str(e.value)
    assert f({"dis": {"norm": "none"}, "dis_augment": "", "r1_gamma": 2.0}) == (2.0, 16)
    # the shipped configs: only male2female_r1.yaml turns it on, and it is male2female.yaml plus the key
    shipped = sorted(glob.glob(os.path.join(ROOT, "configs", "*.yaml")))
    for path in shipped:
        gamma, every = f(yaml.safe_load(open(path)))
        assert (gamma > 0) == path.endswith("male2female_r1.yaml"), path
    base = yaml.safe_load(open(os.path.join(ROOT, "configs", "male2female.yaml")))
    r1 = yaml.safe_load(open(os.path.join(ROOT, "configs", "male2female_r1.yaml")))
    assert r1.pop("r1_gamma") == 10.0 and r1 == base


def _ctx(L, norm=0, dim=4):
    a = L.Arch(3, 6, 8, 16, 8, 4, 2, 2, dim, 4, 3)
    ctx = C.c_void_p()
    L.check(L.lib.aclgan_ctx_create_dis_norm(C.byref(a), norm, C.byref(ctx)))
    return ctx


def test_symbols_and_scratch_query_without_gpu():
    L, _ = _mods()
    for name, nargs in (("aclgan_dis_r1_scratch_bytes", 5), ("aclgan_dis_r1", 11)):
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == nargs
        assert getattr(L.lib, name).argtypes is not None
    header = open(os.path.join(ROOT, "include", "aclgan_hip.h")).read()
    assert "size_t aclgan_dis_r1_scratch_bytes(aclgan_ctx* ctx, int net, int B, int H, int W);" in header
    assert "int aclgan_dis_r1(aclgan_ctx* ctx, int net, const float* x, int B, int H, int W, float gamma, float* penalty_slot, float* grad_x," in header
    assert "IN EVERY COMPUTE DTYPE" in header
    n0 = L.lib.aclgan_launch_count()
    ctx = _ctx(L)
    sb = L.lib.aclgan_dis_r1_scratch_bytes
    a = {net: sb(ctx, L.NETS[net], 2, 64, 64) for net in ("dis_A", "dis_B", "dis_2")}
    # at least: the image, G, every activation and every delta of the three scales, fp32
    acts = sum(2 * (64 >> s >> l) ** 2 * 4 * (1 << (l - 1)) for s in range(3) for l in range(1, 5))
    imgs = sum(2 * (64 >> s) ** 2 for s in range(3))
    assert a["dis_A"] == a["dis_B"] >= 4 * (2 * acts + 2 * 3 * imgs) and a["dis_2"] >= a["dis_A"] + 4 * 2 * 3 * imgs
    assert sb(ctx, L.NETS["dis_A"], 3, 64, 64) > a["dis_A"] and sb(ctx, L.NETS["dis_A"], 2, 64, 96) > a["dis_A"]
    assert sb(ctx, L.NETS["dis_A"], 2, 65, 67) > 0
    # what aclgan_dis_r1 would refuse sizes as 0: a generator, a null context, an image too small for the third scale, spectral norm
    assert sb(ctx, L.NETS["gen_AB"], 2, 64, 64) == 0 and sb(ctx, 5, 2, 64, 64) == 0 and sb(None, 2, 2, 64, 64) == 0
    assert sb(ctx, L.NETS["dis_A"], 0, 64, 64) == 0
    assert sb(ctx, L.NETS["dis_A"], 2, 61, 64) > 0            # 61 -> 31 -> 16 at the third scale -> 8, 4, 2: the last layer sees two rows
    assert sb(ctx, L.NETS["dis_A"], 2, 32, 64) == 0           # 32 -> 16 -> 8 -> 4, 2, 1: it would see one
    sn = _ctx(L, norm=L.NORM["sn"])
    assert sb(sn, L.NETS["dis_A"], 2, 64, 64) == 0
    L.lib.aclgan_ctx_destroy(sn)
    L.lib.aclgan_ctx_destroy(ctx)
    assert L.lib.aclgan_launch_count() == n0


def test_argument_checks_launch_nothing():
    """every refusal is a code with a message, made before anything is enqueued"""
    L, _ = _mods()
    n0 = L.lib.aclgan_launch_count()
    f = L.lib.aclgan_dis_r1
    fake, fake2, fake3 = C.c_void_p(0x10000), C.c_void_p(0x20000), C.c_void_p(0x30000)
    A = L.NETS["dis_A"]
    ctx = _ctx(L)
    EINVAL, EUNSUPPORTED = -1, -2
    # unbound parameters
    assert f(ctx, A, fake, 2, 64, 64, 1.0, fake2, None, fake3, None) == EINVAL and "bind" in L.last_error()
    for grp in (0, 1):
        L.check(L.lib.aclgan_bind_params(ctx, grp, fake, fake, fake, fake))
    for net in (L.NETS["gen_AB"], L.NETS["gen_BA"], 5, -1):
        assert f(ctx, net, fake, 2, 64, 64, 1.0, fake2, None, fake3, None) == EINVAL and "discriminator" in L.last_error()
    assert f(None, A, fake, 2, 64, 64, 1.0, fake2, None, fake3, None) == EINVAL
    for gamma in (-1.0, float("nan"), float("inf"), -float("inf")):
        assert f(ctx, A, fake, 2, 64, 64, gamma, fake2, None, fake3, None) == EINVAL and "gamma" in L.last_error()
    for args in ((None, fake2, fake3), (fake, None, fake3), (fake, fake2, None)):
        assert f(ctx, A, args[0], 2, 64, 64, 1.0, args[1], None, args[2], None) == EINVAL and "null" in L.last_error()
    for (B, H, W) in ((0, 64, 64), (-1, 64, 64), (2, 16, 64), (2, 64, 16), (2, 0, 64), (70000, 64, 64)):
        assert f(ctx, A, fake, B, H, W, 1.0, fake2, None, fake3, None) == EINVAL, (B, H, W)
    assert f(ctx, A, fake, 2, 16, 64, 1.0, fake2, None, fake3, None) == EINVAL and "too small" in L.last_error()
    L.lib.aclgan_ctx_destroy(ctx)
    sn = _ctx(L, norm=L.NORM["sn"])
    for grp in (0, 1):
        L.check(L.lib.aclgan_bind_params(sn, grp, fake, fake, fake, fake))
    assert f(sn, A, fake, 2, 64, 64, 1.0, fake2, None, fake3, None) == EUNSUPPORTED and "sn" in L.last_error()
    assert f(sn, L.NETS["gen_AB"], fake, 2, 64, 64, 1.0, fake2, None, fake3, None) == EINVAL      # no discriminator: EINVAL comes first
    L.lib.aclgan_ctx_destroy(sn)
    assert L.lib.aclgan_launch_count() == n0


def test_queries_of_an_update_do_not_count_the_pass():
    """the pass is no part of an update: the workspace, the algorithmic bytes and the executed FLOPs of dis_update are the context's own,
    whatever the trainer's keys say (there is nothing on the context to set)"""
    L, _ = _mods()
    ctx = _ctx(L, dim=8)
    fake = C.c_void_p(0x10000)
    for grp in (0, 1):
        L.check(L.lib.aclgan_bind_params(ctx, grp, fake, fake, fake, fake))

    def q():
        ws, v, w = C.c_size_t(), C.c_double(), C.c_double()
        L.check(L.lib.aclgan_workspace_bytes(ctx, 2, 64, 64, C.byref(ws)))
        L.check(L.lib.aclgan_step_algorithmic_bytes(ctx, 1, 2, 64, 64, C.byref(v)))
        L.check(L.lib.aclgan_step_executed_flops(ctx, 1, 2, 64, 64, C.byref(w)))
        return ws.value, v.value, w.value
    before = q()
    assert L.lib.aclgan_dis_r1_scratch_bytes(ctx, L.NETS["dis_A"], 2, 64, 64) > 0
    assert q() == before
    L.lib.aclgan_ctx_destroy(ctx)
