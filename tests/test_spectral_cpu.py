"""Spectral normalisation (dis.norm: sn) without a GPU: an fp64 numpy restatement of the reference's power iteration
(SpectralNorm._update_u_v, one iteration per forward call) replays the discriminator calls of dis_update and gen_update in the
reference's order from the fixture's initial u / v / W_bar, and must reproduce the sigma of every call and u / v afterwards
(tests/golden/make_golden_sn.py).  This pins the call order the library must follow (dis_A sees x_A_fake, x_a, x_A2_fake, x_a in
dis_update) and the v ordering of the state_dict (Ci kh kw, OIHW)."""
import json
import os

import numpy as np
import pytest

from conftest import ROOT

GOLD = os.path.join(ROOT, "tests", "golden")
FIX = "step_reduced_64_sn_smooth"
DIS = ("dis_A", "dis_B", "dis_2")
# forward calls per discriminator and update (trainer.py:136-139, 283-286)
CALLS = {"dis": {"dis_A": 4, "dis_B": 2, "dis_2": 2}, "gen": {"dis_A": 2, "dis_B": 1, "dis_2": 2}}


def _load():
    meta = json.load(open(os.path.join(GOLD, FIX + ".json")))
    data = np.load(os.path.join(GOLD, FIX + ".npz"))
    return meta, data


def _sn_layers(meta, net):
    """(prefix, W_bar as Co x (Ci kh kw), u, v) of every SN layer of `net` in the fixture's initial state, in (scale, layer) order"""
    from sn_nets import sn_test_nets
    sd = sn_test_nets(meta["config"], meta["seed"])[net]
    keys = sorted({k[:-len("weight_bar")] for k in sd if k.endswith(".module.weight_bar")},
                  key=lambda p: tuple(int(x) for x in p.split(".")[1:3]))
    out = []
    for p in keys:
        w = sd[p + "weight_bar"].double().numpy()
        out.append((p, w.reshape(w.shape[0], -1), sd[p + "weight_u"].double().numpy().copy(), sd[p + "weight_v"].double().numpy().copy()))
    return out


def l2n(x):
    return x / (np.linalg.norm(x) + 1e-12)


def power_iteration(w, u):
    v = l2n(w.T @ u)
    u = l2n(w @ v)
    return u, v, float(u @ (w @ v))


@pytest.mark.parametrize("which", ["dis", "gen"])
def test_sigma_sequence_and_uv_follow_the_reference_call_order(which):
    meta, data = _load()
    sig_ref = meta["sigma_%s" % which]
    for net in DIS:
        layers = _sn_layers(meta, net)
        assert len(layers) == 9
        assert len(sig_ref[net]) == CALLS[which][net]
        for call in range(CALLS[which][net]):
            for i, (p, w, u, v) in enumerate(layers):
                u, v, s = power_iteration(w, u)
                layers[i] = (p, w, u, v)
                assert abs(s - sig_ref[net][call][i]) <= 1e-9 * abs(s), (net, call, p, s, sig_ref[net][call][i])
        for p, w, u, v in layers:
            np.testing.assert_allclose(u, data["uv_%s/%s/%sweight_u" % (which, net, p)], rtol=0, atol=1e-6)
            np.testing.assert_allclose(v, data["uv_%s/%s/%sweight_v" % (which, net, p)], rtol=0, atol=1e-6)


def test_sn_state_dict_layout():
    """state_dict_keys_sn.txt (the full-width reference): per SN layer bias, weight_u, weight_v, weight_bar in that order, no weight key,
    u of Co and v of Ci kh kw elements; the first 4x4 layer and the 1x1 head are plain convolutions"""
    lines = [l.split() for l in open(os.path.join(GOLD, "state_dict_keys_sn.txt")).read().splitlines()]
    dis = [(n, k, s) for n, k, s in lines if n == "dis_A"]
    sn = [(k, s) for _, k, s in dis if ".module." in k]
    assert len(sn) == 4 * 9
    for i in range(0, len(sn), 4):
        names = [k.rsplit(".", 1)[1] for k, _ in sn[i:i + 4]]
        assert names == ["bias", "weight_u", "weight_v", "weight_bar"], names
        co, ci, kh, kw = (int(x) for x in sn[i + 3][1].split("x"))
        assert sn[i + 1][1] == str(co) and sn[i + 2][1] == str(ci * kh * kw)
    assert sum(int(np.prod([int(x) for x in s.split("x")])) for k, s in sn if k.endswith("weight_bar")) == 3 * (128 * 1024 + 256 * 2048 + 512 * 4096)
    assert not any(k.endswith(".weight") and ".module." in k for _, k, _ in dis)
    assert ("dis_A", "cnns.0.0.conv.weight", "64x3x4x4") in [tuple(l) for l in lines]
    assert ("dis_A", "cnns.0.4.weight", "1x512x1x1") in [tuple(l) for l in lines]


def test_config_selects_spectral_norm_and_other_norms_still_raise():
    import yaml
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib as L
    from aclgan_amd.trainer import arch_from_config, dis_norm_from_config
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "male2female_sn.yaml")))
    base = yaml.safe_load(open(os.path.join(ROOT, "configs", "male2female.yaml")))
    assert {k: v for k, v in cfg.items() if k != "dis"} == {k: v for k, v in base.items() if k != "dis"}
    assert {k: v for k, v in cfg["dis"].items() if k != "norm"} == {k: v for k, v in base["dis"].items() if k != "norm"}
    assert dis_norm_from_config(cfg) == L.NORM["sn"] and dis_norm_from_config(base) == 0
    arch_from_config(cfg)
    for norm in ("in", "ln", "bn", "adain"):
        bad = dict(cfg, dis=dict(cfg["dis"], norm=norm))
        with pytest.raises(L.AclganError):
            arch_from_config(bad)
    with pytest.raises(L.AclganError):
        arch_from_config(dict(cfg, dis=dict(cfg["dis"], gan_type="nsgan")))


def test_library_tensor_table_under_spectral_norm_without_gpu():
    """the C ABI's layout under ACLGAN_NORM_SN: the discriminator group lists bias, weight_bar of every SN layer (the reference's
    dis_opt order), the SN-state group weight_u / weight_v; keys and shapes match the reference's state_dict"""
    import ctypes as C
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib as L
    a = L.Arch(3, 6, 64, 256, 8, 4, 2, 4, 64, 4, 3)
    ref = {}
    for n, k, s in (l.split() for l in open(os.path.join(GOLD, "state_dict_keys_sn.txt")).read().splitlines()):
        ref["%s/%s" % (n, k)] = tuple(int(x) for x in s.split("x"))
    ctx = C.c_void_p()
    L.check(L.lib.aclgan_ctx_create_dis_norm(C.byref(a), L.NORM["sn"], C.byref(ctx)))
    try:
        name = C.create_string_buffer(256)
        off = C.c_int64(); shp = (C.c_int * 4)(); nd = C.c_int()
        got = {}
        for grp in (L.GROUP_DIS, L.GROUP_SN_STATE):
            keys = []
            for i in range(L.lib.aclgan_tensor_count(ctx, grp)):
                L.check(L.lib.aclgan_tensor_info(ctx, grp, i, name, 256, C.byref(off), shp, C.byref(nd)))
                keys.append(name.value.decode())
                got[keys[-1]] = tuple(shp[j] for j in range(nd.value))
            if grp == L.GROUP_DIS:
                sn = [k for k in keys if ".module." in k]
                assert len(sn) == 2 * 27 and all(sn[i].endswith("bias") and sn[i + 1].endswith("weight_bar") for i in range(0, len(sn), 2))
            else:
                assert len(keys) == 2 * 27
        assert L.lib.aclgan_group_numel(ctx, L.GROUP_SN_STATE) == 3 * 3 * (128 + 1024 + 256 + 2048 + 512 + 4096)
        dis_ref = {k: v for k, v in ref.items() if k.startswith("dis")}
        assert got == dis_ref, set(got) ^ set(dis_ref)
    finally:
        L.lib.aclgan_ctx_destroy(ctx)
    with pytest.raises(L.AclganError):
        L.check(L.lib.aclgan_ctx_create_dis_norm(C.byref(a), L.NORM["in"], C.byref(ctx)))


@pytest.mark.parametrize("dtype", [0, 1])
def test_dry_run_counts_and_sizes_the_spectral_norm_work_without_gpu(dtype):
    """a launch-free dry run of the scheduler under SN: the step's workspace need, executed FLOPs and algorithmic bytes exceed the
    none-norm step's (weight slots, per-call gradient scratch, the split discriminator passes, the power iterations and folds)"""
    import ctypes as C
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib as L
    a = L.Arch(3, 6, 64, 256, 8, 4, 2, 4, 64, 4, 3)
    fake = C.c_void_p(0x10000)

    def measure(norm):
        ctx = C.c_void_p()
        L.check(L.lib.aclgan_ctx_create_dis_norm(C.byref(a), norm, C.byref(ctx)))
        L.check(L.lib.aclgan_set_compute_dtype(ctx, dtype))
        for grp in (0, 1):
            L.check(L.lib.aclgan_bind_params(ctx, grp, fake, fake, fake, fake))
            if dtype:
                L.check(L.lib.aclgan_bind_params16(ctx, grp, fake, fake))
        out = []
        for which in (0, 1):
            ws, f, b = C.c_size_t(), C.c_double(), C.c_double()
            L.check(L.lib.aclgan_workspace_bytes(ctx, 8, 256, 256, C.byref(ws)) if which == 0 else 0)
            L.check(L.lib.aclgan_step_executed_flops(ctx, which, 8, 256, 256, C.byref(f)))
            L.check(L.lib.aclgan_step_algorithmic_bytes(ctx, which, 8, 256, 256, C.byref(b)))
            out.append((ws.value, f.value, b.value))
        fw = C.c_size_t()
        L.check(L.lib.aclgan_forward_workspace_bytes(ctx, 8, 256, 256, C.byref(fw)))
        L.lib.aclgan_ctx_destroy(ctx)
        return out, fw.value

    none, fw0 = measure(0)
    sn, fw1 = measure(L.NORM["sn"])
    n_weights = 3 * (128 * 1024 + 256 * 2048 + 512 * 4096)        # SN weights per discriminator (8.26 M)
    assert sn[0][0] > none[0][0] + 5 * n_weights * 4                  # dis_update: 8 calls x (slot + gradient scratch)
    assert fw1 >= fw0                                                 # (the generator passes dominate the forward-only arena here)
    for which, calls in ((0, 5), (1, 8)):                             # discriminator calls per update (each: power iteration (+ fold))
        assert sn[which][1] > none[which][1]
        assert sn[which][2] - none[which][2] > calls * n_weights * 4 * 3
    assert L.lib.aclgan_launch_count() == 0
