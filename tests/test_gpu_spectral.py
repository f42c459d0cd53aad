"""Spectrally normalised discriminators (dis.norm: sn; reference networks.py:360-361, 538-600) on the MI355X.

  * the power-iteration and fold kernels (csrc/spectral.hip) against fp64 at the 9 matrices of the shipped width;
  * one dis_update / gen_update and three chained steps against the fp64 reference fixture (tests/golden/make_golden_sn.py):
    losses, gradient norms, u / v after each update, the parameters after Adam;
  * the checkpoint surface: keys / shapes, save -> resume, a checkpoint written by the reference;
  * lanes: 1, 2, 3 lanes bitwise equal in deterministic mode;
  * bf16 at 64x64 B=2 against the fixture; 256x256 B=8 fp32 / bf16 stays finite with sigma > 0 and |u| = 1;
  * both updates at the reduced and at the shipped width (step_full_64_sn_smooth);
  * the kernels at their tiling edges (row-chunk, column-tile and element-block tails, a 16-layer block table) and the ABI's refusals;
  * frozen-mask parity against the fp64 oracle's spectral norm at 256x256 (fp32 B=8 default plan with 3 lanes and deterministic,
    bf16 B=8 and fp16 B=32 against the emulated 16-bit contract) and at 64x64 B=2.  Measured worst relative L2 per network group:
    fp32 B=8 dis 3.4e-6, gen 4.1e-5 (both plans); bf16 B=8 dis 3.5e-3, gen 1.4e-2; fp16 B=32 dis 4.6e-4, gen 2.0e-3; u / v 1.3e-7.
    No weight_bar tensor needed a bound of its own.
Run on the GPU box: pytest -m gpu"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FIX = "step_reduced_64_sn_smooth"
FIX_FULL = "step_full_64_sn_smooth"      # the shipped width
DIS = ("dis_A", "dis_B", "dis_2")
NETS = ("gen_AB", "gen_BA") + DIS
# the SN matrices of one discriminator at the shipped width (dis.dim 64, n_layer 4, 3 scales): Co x (Ci kh kw)
SHIPPED = [(128, 1024), (256, 2048), (512, 4096)] * 3


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available()
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def T(L):
    from aclgan_amd import trainer
    return trainer


def _load(fix=FIX):
    meta = json.load(open(os.path.join(GOLDEN, fix + ".json")))
    data = np.load(os.path.join(GOLDEN, fix + ".npz"))
    return meta, data


def _make(T, cfg, data, fix=FIX, **kw):
    """a trainer in the fixture's initial state (tests/sn_nets.py; `data` is the fixture, whose config and seed name it)"""
    from sn_nets import sn_test_nets
    meta = json.load(open(os.path.join(GOLDEN, fix + ".json")))
    assert meta["config"] == cfg
    nets = sn_test_nets(cfg, meta["seed"])
    tr = T.aclgan_Trainer(cfg, **kw)
    for n in NETS:
        getattr(tr, n).load_state_dict(nets[n], strict=False)     # (the generators' AdaIN running statistics are not in the test fill)
    for n in DIS:      # ... but every discriminator tensor is, u and v included
        assert set(nets[n]) == set(getattr(tr, n).state_dict()), n
    return tr


def _inputs(data):
    return torch.from_numpy(data["x_a"]), torch.from_numpy(data["x_b"]), [torch.from_numpy(data["z%d" % i]) for i in range(6)]


def _nrel(a, b):
    a = torch.as_tensor(a).detach().double().cpu().flatten(); b = torch.as_tensor(b).detach().double().cpu().flatten()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


# ---------------------------------------------------------------------------------------------------------------------------
# kernels vs fp64
# ---------------------------------------------------------------------------------------------------------------------------
def _packed(seed, shapes):
    g = torch.Generator().manual_seed(seed)
    ws, us = [], []
    for co, k in shapes:
        b = 1.0 / np.sqrt(k)      # nn.Conv2d's default (kaiming-uniform, a = sqrt 5) range
        ws.append((torch.rand(co, k, generator=g, dtype=torch.float64) * 2 - 1) * b)
        u = torch.randn(co, generator=g, dtype=torch.float64)
        us.append(u / u.norm())
    return [w.float().double() for w in ws], [u.float().double() for u in us]


def _pi64(w, u):
    v = w.t() @ u; v = v / (v.norm() + 1e-12)
    u = w @ v; u = u / (u.norm() + 1e-12)
    return u, v, u @ (w @ v)


@pytest.mark.parametrize("iters", [1, 5])
@pytest.mark.parametrize("cin", [3, 6])
def test_power_iteration_kernel_matches_fp64(L, iters, cin):
    """the 9 SN matrices of a discriminator at the shipped width (the same for dis_A / dis_B, Cin 3, and dis_2, Cin 6: the first layer is
    not normalised); u, v, sigma to 1e-5 relative and W / sigma to 1e-6 relative after 1 and 5 consecutive calls"""
    n = len(SHIPPED)
    ws, us = _packed(100 + cin, SHIPPED)
    co = (C.c_int * n)(*[s[0] for s in SHIPPED]); kk = (C.c_int * n)(*[s[1] for s in SHIPPED])
    dev = torch.device("cuda")
    w = torch.cat([x.flatten() for x in ws]).float().to(dev)
    u = torch.cat(us).float().to(dev)
    v = torch.zeros(sum(s[1] for s in SHIPPED), device=dev)
    wn = torch.empty_like(w)
    sig = torch.zeros(n, device=dev)
    scr = torch.empty(L.lib.aclgan_sn_scratch_bytes(n, co, kk), dtype=torch.uint8, device=dev)
    st = L.stream_ptr()
    u64 = list(us)
    for _ in range(iters):
        L.check(L.lib.aclgan_sn_power_iteration(n, co, kk, L.ptr(w), L.ptr(u), L.ptr(v), L.ptr(wn), L.ptr(sig), L.ptr(scr), st))
        res = [_pi64(ws[l], u64[l]) for l in range(n)]
        u64 = [r[0] for r in res]
    torch.cuda.synchronize()
    uo = vo = wo = 0
    for l, (c_, k_) in enumerate(SHIPPED):
        ur, vr, sr = res[l]
        assert _nrel(u[uo:uo + c_], ur) <= 1e-5, (l, _nrel(u[uo:uo + c_], ur))
        assert _nrel(v[vo:vo + k_], vr) <= 1e-5, (l, _nrel(v[vo:vo + k_], vr))
        assert abs(float(sig[l]) - float(sr)) <= 1e-5 * float(sr), (l, float(sig[l]), float(sr))
        assert _nrel(wn[wo:wo + c_ * k_], ws[l].flatten() / sr) <= 1e-6, (l, _nrel(wn[wo:wo + c_ * k_], ws[l].flatten() / sr))
        uo += c_; vo += k_; wo += c_ * k_


def test_fold_kernel_matches_fp64_autograd(L):
    """grad += G / sigma - (<G, W> / sigma^2) u v^T == d/dW <G, W / sigma(W)> with sigma(W) = u . (W v), u and v constant (fp64 autograd),
    accumulated onto an existing gradient, at the shipped matrices with random G; 1e-5 relative"""
    n = len(SHIPPED)
    ws, us = _packed(7, SHIPPED)
    co = (C.c_int * n)(*[s[0] for s in SHIPPED]); kk = (C.c_int * n)(*[s[1] for s in SHIPPED])
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(8)
    Gs = [torch.randn(c_, k_, generator=g, dtype=torch.float64).float().double() for c_, k_ in SHIPPED]
    base = [torch.randn(c_, k_, generator=g, dtype=torch.float64).float().double() * 0.1 for c_, k_ in SHIPPED]
    w = torch.cat([x.flatten() for x in ws]).float().to(dev)
    u = torch.cat(us).float().to(dev)
    v = torch.zeros(sum(s[1] for s in SHIPPED), device=dev)
    wn = torch.empty_like(w); sig = torch.zeros(n, device=dev)
    scr = torch.empty(L.lib.aclgan_sn_scratch_bytes(n, co, kk), dtype=torch.uint8, device=dev)
    st = L.stream_ptr()
    L.check(L.lib.aclgan_sn_power_iteration(n, co, kk, L.ptr(w), L.ptr(u), L.ptr(v), L.ptr(wn), L.ptr(sig), L.ptr(scr), st))
    G = torch.cat([x.flatten() for x in Gs]).float().to(dev)
    grad = torch.cat([x.flatten() for x in base]).float().to(dev)
    L.check(L.lib.aclgan_sn_fold(n, co, kk, L.ptr(w), L.ptr(G), L.ptr(u), L.ptr(v), L.ptr(sig), L.ptr(grad), L.ptr(scr), st))
    torch.cuda.synchronize()
    uo = vo = wo = 0
    for l, (c_, k_) in enumerate(SHIPPED):
        ul = u[uo:uo + c_].double().cpu(); vl = v[vo:vo + k_].double().cpu()
        W = ws[l].clone().requires_grad_(True)
        s = ul @ (W @ vl)
        (Gs[l] * (W / s)).sum().backward()
        ref = base[l] + W.grad
        got = grad[wo:wo + c_ * k_].view(c_, k_)
        assert _nrel(got - base[l].float().to(dev), W.grad) <= 1e-5, (l, _nrel(got - base[l].float().to(dev), W.grad))
        assert _nrel(got, ref) <= 1e-5
        uo += c_; vo += k_; wo += c_ * k_


# ---------------------------------------------------------------------------------------------------------------------------
# updates vs the fp64 reference fixture
# ---------------------------------------------------------------------------------------------------------------------------
def _uv_check(tr, data, prefix, tol):
    for net in DIS:
        sd = getattr(tr, net).state_dict()
        for k, v in sd.items():
            if k.endswith(("weight_u", "weight_v")):
                ref = torch.from_numpy(data["%s/%s/%s" % (prefix, net, k)])
                err = (v.cpu().double() - ref.double()).abs().max().item()
                assert err <= tol, (prefix, net, k, err)


def _grads(tr, nets):
    return {(n, k): g.contiguous().clone() for n in nets for k, g in getattr(tr, n).named_grads()}


def _check_losses(tr, ref, ltol, size_tol, digit_tol=None):
    for n, v in ref.items():
        got = float(getattr(tr, n))
        tol = size_tol if n.endswith("_size") else (digit_tol if (digit_tol and n.endswith("_digit")) else ltol)
        assert np.isfinite(got) and abs(got - v) <= tol * max(1e-3, abs(v)), (n, got, v)


def _check_grad_norms(meta, gd, gg, gtol, floor=None):
    """every gradient tensor's norm within gtol of the fixture's, plus 1e-5 of the largest norm; floor: instead within
    gtol (nrm + floor x the largest norm) -- tests/test_gpu_step16.py's 16-bit bound, see _bf16_update_matches_reference"""
    gmax = max(v[1] for v in meta["grad_stats"].values())
    seen, worst = 0, (0.0, None)
    for key, (s, nrm, mx) in meta["grad_stats"].items():
        upd, net, k = key.split("/", 2)
        g = (gd if upd == "dis_update" else gg)[(net, k)]
        got = float(g.double().norm())
        bound = gtol * nrm + 1e-5 * gmax if floor is None else gtol * (nrm + floor * gmax)
        worst = max(worst, (abs(got - nrm) / bound, key))
        assert abs(got - nrm) <= bound, (key, got, nrm, bound)
        seen += 1
    print("gradient norms: worst error / bound %.2f (%s)" % worst)
    assert seen == len(gd) + len(gg)


def test_updates_match_reference(T):
    """dis_update and gen_update, each from the fixture's initial state, vs the fp64 reference: the 16 losses (1e-3; the
    'size' losses 5e-3, as tests/test_gpu_step.py), every gradient tensor's norm (1e-2), u and v after each update (1e-5), the
    discriminator parameters after Adam"""
    _updates_match_reference(T, FIX)


def test_updates_match_reference_full_width(T):
    """the same at the shipped width (step_full_64_sn_smooth: the 9 SN matrices of male2female_sn.yaml, 128 x 1024 .. 512 x 4096)"""
    _updates_match_reference(T, FIX_FULL)


def _updates_match_reference(T, fix):
    meta, data = _load(fix)
    cfg = meta["config"]
    x_a, x_b, z = _inputs(data)
    trd = _make(T, cfg, data, fix)
    trd.dis_update(x_a, x_b, cfg, z=z[:3])
    gd = _grads(trd, DIS)
    trg = _make(T, cfg, data, fix)
    trg.gen_update(x_a, x_b, cfg, z=z[3:6])
    gg = _grads(trg, ("gen_AB", "gen_BA"))
    torch.cuda.synchronize()
    _check_losses(trd, {k: v for k, v in meta["losses"].items() if k.startswith("loss_dis")}, 1e-3, 5e-3)
    _check_losses(trg, {k: v for k, v in meta["losses"].items() if not k.startswith("loss_dis")}, 1e-3, 5e-3)
    _check_grad_norms(meta, gd, gg, 1e-2)
    _uv_check(trd, data, "uv_dis", 1e-5)
    _uv_check(trg, data, "uv_gen", 1e-5)
    lr = cfg["lr"]
    for net in DIS:
        for k, p in getattr(trd, net).named_parameters():
            s, nrm, mx = meta["param_stats_after_dis"]["%s/%s" % (net, k)]
            pd = p.detach().double().flatten()
            got = float(pd.norm())
            # Adam's first step moves every element by lr * g / (|g| + eps) ~ lr * sign(g): an element whose gradient is within the
            # implementations' difference of 0 may step the other way, 2 lr off.  The gradients agree to ~1e-2 in norm (above; the
            # ReLU-mask lottery of tests/test_gpu_step.py), and in the deepest SN layers the two terms of the fold, G / sigma and
            # <G, W> / sigma^2 u v^T, nearly cancel for many elements -- so every element whose gradient is below 3e-2 of the tensor's
            # rms may contribute 2 lr |p_i| / |p| to the norm (measured: 4.7e-5 on a weight_bar of norm 3.6)
            g = gd[(net, k)].double().flatten().cpu()
            amb = g.abs() <= 3e-2 * g.pow(2).mean().sqrt()
            slack = 2 * lr * float(pd.cpu()[amb].abs().sum()) / max(nrm, 1e-12)
            assert abs(got - nrm) <= 1e-5 * max(1.0, nrm) + 4 * lr * mx / max(nrm, 1e-12) + slack, (net, k, got, nrm, slack)


def test_three_chained_steps_match_reference(T):
    """three dis -> gen steps in the train.py order on the updated weights: every loss of every step, u and v at the end"""
    meta, data = _load()
    cfg = meta["config"]
    x_a, x_b, z = _inputs(data)
    tr = _make(T, cfg, data)
    for step, ref in enumerate(meta["seq_losses"]):
        tr.dis_update(x_a, x_b, cfg, z=z[:3])
        tr.gen_update(x_a, x_b, cfg, z=z[3:6])
        torch.cuda.synchronize()
        # (Adam turns gradient rounding into O(lr) parameter noise from the first step on: looser than a single update)
        _check_losses(tr, ref, 2e-3 * (step + 1), 2e-2 * (step + 1))
    # u / v follow W_bar, which after Adam carries O(lr) = 1e-4 noise per element (a gradient within rounding of 0 may step either way),
    # amplified by the small spectral gap of these nearly random matrices (one power iteration per call is far from converged):
    # measured up to 1.3e-3 after three steps, while every loss of every step holds the bounds above
    _uv_check(tr, data, "seq_uv", 1e-2)


def test_bf16_update_matches_reference(T):
    """compute dtype bf16 (16-bit MFMA operands, the normalised weights packed from W_bar / sigma each call) at 64x64 B=2 vs the fp64
    fixture, with the 16-bit bounds of tests/test_gpu_step16.py"""
    _bf16_update_matches_reference(T, FIX)


def test_bf16_update_matches_reference_full_width(T):
    """the same at the shipped width.  Gradient norms within GTOL (nrm + 1e-4 x the largest norm), the bound of
    tests/test_gpu_step16.py::test_step_gradients_16bit: the conv biases in front of an instance norm have a gradient of 0 in exact
    arithmetic (the fixture's norms are 1e-17), but under bf16 the gradient of their stored 16-bit conv output is rounded before it is
    summed (oracle.conv_block: _StoreQ), so what the library returns is the sum of B H W rounding errors -- at this width up to 1.1e-5 of
    the largest gradient norm, just above the reduced fixture's floor of 1e-5"""
    _bf16_update_matches_reference(T, FIX_FULL, floor=1e-4)


def _bf16_update_matches_reference(T, fix, floor=None):
    from test_gpu_step16 import LTOL, LTOL_DIGIT, LTOL_SIZE, GTOL
    meta, data = _load(fix)
    cfg = meta["config"]
    x_a, x_b, z = _inputs(data)
    trd = _make(T, cfg, data, fix, compute_dtype="bf16")
    trd.dis_update(x_a, x_b, cfg, z=z[:3])
    gd = _grads(trd, DIS)
    trg = _make(T, cfg, data, fix, compute_dtype="bf16")
    trg.gen_update(x_a, x_b, cfg, z=z[3:6])
    gg = _grads(trg, ("gen_AB", "gen_BA"))
    torch.cuda.synchronize()
    _check_losses(trd, {k: v for k, v in meta["losses"].items() if k.startswith("loss_dis")}, LTOL["bf16"], LTOL_SIZE["bf16"])
    _check_losses(trg, {k: v for k, v in meta["losses"].items() if not k.startswith("loss_dis")}, LTOL["bf16"], LTOL_SIZE["bf16"],
                  LTOL_DIGIT["bf16"])
    _check_grad_norms(meta, gd, gg, GTOL["bf16"], floor)
    # the power iteration runs on the fp32 master weights whatever the compute dtype
    _uv_check(trd, data, "uv_dis", 1e-5)
    _uv_check(trg, data, "uv_gen", 1e-5)


def test_forward_only_call_advances_u_and_v(T):
    """MsImageDis.forward (aclgan_dis_forward) runs one power iteration per call, like the reference's forward in eval mode"""
    meta, data = _load()
    cfg = meta["config"]
    x_a, _, _ = _inputs(data)
    tr = _make(T, cfg, data)
    tr.dis_A(x_a)
    tr.dis_A(x_a)
    torch.cuda.synchronize()
    # two calls = the first two dis_A calls of gen_update (the power iteration does not depend on the input)
    sd = tr.dis_A.state_dict()
    for k, v in sd.items():
        if k.endswith(("weight_u", "weight_v")):
            ref = torch.from_numpy(data["uv_gen/dis_A/%s" % k])
            assert (v.cpu().double() - ref.double()).abs().max().item() <= 1e-5, k


# ---------------------------------------------------------------------------------------------------------------------------
# checkpoint surface
# ---------------------------------------------------------------------------------------------------------------------------
def test_state_dict_keys_and_save_resume(T, tmp_path):
    import yaml
    from conftest import ROOT
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "male2female_sn.yaml")))
    cfg["display_size"] = 1
    tr = T.aclgan_Trainer(cfg)
    want = {}
    for line in open(os.path.join(GOLDEN, "state_dict_keys_sn.txt")):
        net, key, shp = line.split()
        want.setdefault(net, []).append((key, tuple(int(s) for s in shp.split("x"))))
    for net in NETS:
        assert [(k, tuple(v.shape)) for k, v in getattr(tr, net).state_dict().items()] == want[net], net
    # initialisation (networks.py:567-574, utils.py:277): weight_bar kaiming-uniform(a = sqrt 5), bias U(+-1/sqrt fan_in), |u| = |v| = 1
    sd = tr.dis_B.state_dict()
    w = sd["cnns.0.3.conv.module.weight_bar"]
    bound = 1.0 / np.sqrt(w[0].numel())
    assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.95 * bound
    assert float(sd["cnns.0.3.conv.module.bias"].abs().max()) <= bound
    assert abs(float(sd["cnns.1.2.conv.module.weight_u"].norm()) - 1) < 1e-5 and abs(float(sd["cnns.1.2.conv.module.weight_v"].norm()) - 1) < 1e-5

    # save -> resume round trip, exact, at the fixture's reduced width after one step
    meta, data = _load()
    rcfg = meta["config"]
    x_a, x_b, z = _inputs(data)
    tr = _make(T, rcfg, data)
    tr.dis_update(x_a, x_b, rcfg, z=z[:3])
    tr.gen_update(x_a, x_b, rcfg, z=z[3:6])
    tr.save(str(tmp_path), 41)
    tr2 = T.aclgan_Trainer(rcfg)
    assert tr2.resume(str(tmp_path), rcfg) == 42
    for net in NETS:
        a, b = getattr(tr, net).state_dict(), getattr(tr2, net).state_dict()
        assert list(a) == list(b)
        for k in a:
            assert torch.equal(a[k].cpu(), b[k].cpu()), (net, k)
    for grp in (0, 1):
        assert torch.equal(tr._m[grp], tr2._m[grp]) and torch.equal(tr._v[grp], tr2._v[grp])
    opt = torch.load(os.path.join(tmp_path, "optimizer.pt"), map_location="cpu")
    # dis_opt holds bias then weight_bar of an SN layer, never u / v (requires_grad False)
    dis_params = [(n, k) for n in DIS for k, _ in getattr(tr, n).named_parameters()]
    assert len(opt["dis"]["param_groups"][0]["params"]) == len(dis_params)
    assert not any(k.endswith(("weight_u", "weight_v")) for _, k in dis_params)
    i = dis_params.index(("dis_A", "cnns.0.1.conv.module.bias"))
    assert dis_params[i + 1] == ("dis_A", "cnns.0.1.conv.module.weight_bar")
    assert tuple(opt["dis"]["state"][i + 1]["exp_avg"].shape) == tuple(tr.dis_A.state_dict()["cnns.0.1.conv.module.weight_bar"].shape)


def test_resume_from_reference_written_checkpoint(T, tmp_path):
    """tests/golden/ckpt_reference_reduced_sn: written by the reference's trainer.save with dis.norm: sn (reduced width, one SN layer per
    scale, after one dis_update); loads (u, v, weight_bar, the Adam state in dis_opt order) and the next dis_update reproduces the
    reference's loss"""
    import shutil
    src = os.path.join(GOLDEN, "ckpt_reference_reduced_sn")
    exp = json.load(open(os.path.join(src, "expect.json")))
    for f in exp["files"]:
        shutil.copy(os.path.join(src, f), tmp_path)
    cfg = exp["config"]
    tr = T.aclgan_Trainer(cfg)
    assert tr.resume(str(tmp_path), cfg) == 7
    assert tr._opt[1]["steps"] == 1 and tr._opt[0]["steps"] == 0
    ref_dis = torch.load(os.path.join(src, "dis_00000007.pt"), map_location="cpu")
    for k, v in tr.dis_2.state_dict().items():
        assert torch.equal(v.cpu(), ref_dis["2"][k]), k
    ref_opt = torch.load(os.path.join(src, "optimizer.pt"), map_location="cpu")
    idx = [k for k, _ in tr.dis_A.named_parameters()].index("cnns.1.1.conv.module.weight_bar")
    e = tr.dis_A._entries[idx]
    assert torch.equal(tr.dis_A._view(e, tr._m[1]).cpu(), ref_opt["dis"]["state"][idx]["exp_avg"])
    assert torch.equal(tr.dis_A._view(tr.dis_A._entries[idx - 1], tr._v[1]).cpu(), ref_opt["dis"]["state"][idx - 1]["exp_avg_sq"])
    from test_gpu_step import _load as load_plain
    pdata = load_plain("step_reduced_64")[1]
    x_a, x_b = torch.from_numpy(pdata["x_a"]), torch.from_numpy(pdata["x_b"])
    z = [torch.from_numpy(pdata["z%d" % i]) for i in range(3)]
    tr.dis_update(x_a, x_b, cfg, z=z)
    assert abs(float(tr.loss_dis_total) - exp["loss_dis_total_after_resume"]) <= 2e-3 * exp["loss_dis_total_after_resume"]


# ---------------------------------------------------------------------------------------------------------------------------
# lanes, full size
# ---------------------------------------------------------------------------------------------------------------------------
def _tune(L, key, value):
    prev = C.c_int()
    L.check(L.lib.aclgan_tuning(key, value, C.byref(prev)), "aclgan_tuning")
    return prev.value


def test_lane_count_does_not_change_a_bit(L, T):
    """deterministic mode: losses, every gradient, u and v of dis_update + gen_update with 2 and 3 lanes == 1 lane, bitwise"""
    from gpu_util import deterministic_mode
    meta, data = _load()
    cfg = meta["config"]
    x_a, x_b, z = _inputs(data)

    def run():
        out = {}
        for which in ("dis", "gen"):
            tr = _make(T, cfg, data)
            getattr(tr, which + "_update")(x_a, x_b, cfg, z=z[:3] if which == "dis" else z[3:6])
            torch.cuda.synchronize()
            losses = {n: float(getattr(tr, n)) for n in L.LOSS_NAMES}
            g = {k: v.cpu() for k, v in _grads(tr, DIS if which == "dis" else ("gen_AB", "gen_BA")).items()}
            out[which] = (losses, g, tr._sn_state.cpu().clone())
        return out

    prev = _tune(L, b"lanes", 1)
    try:
        with deterministic_mode(L, True):
            one = run()
            for lanes in (2, 3):
                _tune(L, b"lanes", lanes)
                other = run()
                for which in ("dis", "gen"):
                    assert one[which][0] == other[which][0], (lanes, which)
                    diff = [k for k in one[which][1] if not torch.equal(one[which][1][k], other[which][1][k])]
                    assert not diff, (lanes, which, diff[:6])
                    assert torch.equal(one[which][2], other[which][2]), (lanes, which)
    finally:
        _tune(L, b"lanes", prev)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_full_size_chained_steps_stay_finite(T, dtype):
    """the shipped SN configuration at 256x256 B=8: three chained steps; every loss and gradient finite, every sigma > 0, |u| = 1 +- 1e-5"""
    import yaml
    from conftest import ROOT
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "male2female_sn.yaml")))
    cfg["display_size"] = 1
    torch.manual_seed(3)
    tr = T.aclgan_Trainer(cfg, compute_dtype=dtype)
    g = torch.Generator().manual_seed(4)
    x_a = torch.rand(8, 3, 256, 256, generator=g) * 2 - 1
    x_b = torch.rand(8, 3, 256, 256, generator=g) * 2 - 1
    for _ in range(3):
        tr.dis_update(x_a, x_b, cfg)
        tr.gen_update(x_a, x_b, cfg)
    torch.cuda.synchronize()
    for n in T.L.LOSS_NAMES:
        assert np.isfinite(float(getattr(tr, n))), n
    for grp in (0, 1):
        assert torch.isfinite(tr._grad[grp]).all() and torch.isfinite(tr._param[grp]).all()
    for net in DIS:
        sd = getattr(tr, net).state_dict()
        for k, v in sd.items():
            if k.endswith("weight_bar"):
                pre = k[:-len("weight_bar")]
                u, vv = sd[pre + "weight_u"].double(), sd[pre + "weight_v"].double()
                assert abs(float(u.norm()) - 1) <= 1e-5, (net, k)
                sigma = float(u @ (v.double().reshape(v.shape[0], -1) @ vv))
                assert sigma > 0 and np.isfinite(sigma), (net, k, sigma)


# ---------------------------------------------------------------------------------------------------------------------------
# kernel edges: the tilings of csrc/spectral.hip are row chunks of 8 (column partials), column tiles of 1024 floats, element blocks of
# 8192 floats (W / sigma, the fold) and a block table of up to 16 layers; the shipped shapes divide all of them evenly
# ---------------------------------------------------------------------------------------------------------------------------
# Co in {1, 3, 5, 13} (a row chunk's tail) with small and large K, K in {4, 16, 1020, 1028, 4100} (column-tile tails: 1020 = 255 float4,
# 1028 and 4100 one float4 past a tile); (13, 4100) is 13325 float4, not a multiple of the 2048 of an element block
EDGE_GROUPS = [[(co, k) for k in (4, 16, 1020, 1028, 4100)] for co in (1, 3, 5, 13)]
# 16 layers of mixed sizes in one call: every block-table seam, tails next to full tiles, a shipped matrix in the middle
EDGE_16 = [(1, 4), (3, 1028), (128, 1024), (5, 4100), (13, 16), (9, 2052), (7, 1020), (1, 4100),
           (64, 64), (9, 12), (2, 8), (256, 2048), (33, 1028), (3, 4), (17, 8196), (5, 1020)]


def _nan_scratch(L, n, co, kk):
    nb = L.lib.aclgan_sn_scratch_bytes(n, co, kk)
    assert nb > 0 and nb % 4 == 0
    return torch.full((nb // 4,), float("nan"), device="cuda")


def _edge_run(L, shapes, iters, seed):
    """`iters` power iterations, then the fold onto a nonzero base, every scratch, output and v NaN-filled before each call.
    Returns the device results and the fp64 inputs."""
    n = len(shapes)
    ws, us = _packed(seed, shapes)
    g = torch.Generator().manual_seed(seed + 1)
    Gs = [torch.randn(c_, k_, generator=g, dtype=torch.float64).float().double() for c_, k_ in shapes]
    base = [torch.randn(c_, k_, generator=g, dtype=torch.float64).float().double() * 0.1 for c_, k_ in shapes]
    co = (C.c_int * n)(*[s[0] for s in shapes]); kk = (C.c_int * n)(*[s[1] for s in shapes])
    dev = torch.device("cuda")
    w = torch.cat([x.flatten() for x in ws]).float().to(dev)
    u = torch.cat(us).float().to(dev)
    v = torch.full((sum(s[1] for s in shapes),), float("nan"), device=dev)
    wn = torch.full_like(w, float("nan"))
    sig = torch.full((n,), float("nan"), device=dev)
    st = L.stream_ptr()
    for _ in range(iters):
        scr = _nan_scratch(L, n, co, kk)
        L.check(L.lib.aclgan_sn_power_iteration(n, co, kk, L.ptr(w), L.ptr(u), L.ptr(v), L.ptr(wn), L.ptr(sig), L.ptr(scr), st))
    G = torch.cat([x.flatten() for x in Gs]).float().to(dev)
    grad = torch.cat([x.flatten() for x in base]).float().to(dev)
    scr = _nan_scratch(L, n, co, kk)
    L.check(L.lib.aclgan_sn_fold(n, co, kk, L.ptr(w), L.ptr(G), L.ptr(u), L.ptr(v), L.ptr(sig), L.ptr(grad), L.ptr(scr), st))
    torch.cuda.synchronize()
    return dict(u=u.cpu(), v=v.cpu(), wn=wn.cpu(), sig=sig.cpu(), grad=grad.cpu()), (ws, us, Gs, base)


def _edge_check(shapes, out, ref, iters):
    ws, us, Gs, base = ref
    uo = vo = wo = 0
    worst = {"u": 0.0, "v": 0.0, "sigma": 0.0, "wn": 0.0, "fold": 0.0}
    for l, (c_, k_) in enumerate(shapes):
        u64 = us[l]
        for _ in range(iters):
            ur, vr, sr = _pi64(ws[l], u64)
            u64 = ur
        e = {"u": _nrel(out["u"][uo:uo + c_], ur), "v": _nrel(out["v"][vo:vo + k_], vr),
             "sigma": abs(float(out["sig"][l]) - float(sr)) / float(sr), "wn": _nrel(out["wn"][wo:wo + c_ * k_], ws[l].flatten() / sr)}
        # the fold, fp64 autograd with the kernel's own u / v (d/dW <G, W / sigma(W)>, sigma = u . (W v)), onto the base
        ul = out["u"][uo:uo + c_].double(); vl = out["v"][vo:vo + k_].double()
        W = ws[l].clone().requires_grad_(True)
        (Gs[l] * (W / (ul @ (W @ vl)))).sum().backward()
        e["fold"] = _nrel(out["grad"][wo:wo + c_ * k_].view(c_, k_).double() - base[l], W.grad)
        for key, val in e.items():
            worst[key] = max(worst[key], val)
            assert val <= 1e-5, (l, (c_, k_), iters, key, val)
        uo += c_; vo += k_; wo += c_ * k_
    return worst


@pytest.mark.parametrize("iters", [1, 5])
@pytest.mark.parametrize("group", range(len(EDGE_GROUPS) + 1), ids=["co1", "co3", "co5", "co13", "16layers"])
def test_kernels_at_tiling_edges_match_fp64(L, iters, group):
    """the power iteration (u, v, sigma, W / sigma) after 1 and 5 calls and the fold onto a nonzero base, against fp64, at row-chunk,
    column-tile and element-block tails and across a full 16-layer block table: 1e-5 relative.  Scratch, outputs and v start as NaN, so
    a read of anything the kernels did not write shows.  A second run gives the same bits."""
    shapes = EDGE_GROUPS[group] if group < len(EDGE_GROUPS) else EDGE_16
    out, ref = _edge_run(L, shapes, iters, 200 + group)
    for key, t in out.items():
        assert torch.isfinite(t).all(), key
    worst = _edge_check(shapes, out, ref, iters)
    print("spectral kernels %s, %d iteration(s): worst relative error %s" % (shapes, iters, {k: "%.1e" % v for k, v in worst.items()}))
    again, _ = _edge_run(L, shapes, iters, 200 + group)
    for key in out:
        assert torch.equal(out[key], again[key]), key


def test_abi_rejects_bad_layer_tables(L):
    """n = 0, n = 17 (SN_MAX_LAYERS is 16) and K % 4 != 0 are refused before anything is launched; n = 16 is accepted"""
    dev = torch.device("cuda")
    buf = torch.zeros(1 << 20, device=dev)
    p = L.ptr(buf)
    st = L.stream_ptr()

    def tables(shapes):
        n = len(shapes)
        return n, (C.c_int * max(1, n))(*[s[0] for s in shapes]), (C.c_int * max(1, n))(*[s[1] for s in shapes])

    for shapes in ([], [(2, 4)] * 17, [(2, 6)], [(3, 4), (5, 18)], [(0, 4)]):
        n, co, kk = tables(shapes)
        assert L.lib.aclgan_sn_scratch_bytes(n, co, kk) == 0, shapes
        assert L.lib.aclgan_sn_power_iteration(n, co, kk, p, p, p, p, p, p, st) != 0, shapes
        assert L.lib.aclgan_sn_fold(n, co, kk, p, p, p, p, p, p, p, st) != 0, shapes
    torch.cuda.synchronize()
    assert torch.equal(buf, torch.zeros_like(buf))
    n, co, kk = tables([(2, 4)] * 16)
    assert L.lib.aclgan_sn_scratch_bytes(n, co, kk) > 0


# ---------------------------------------------------------------------------------------------------------------------------
# frozen-mask parity at the shipped width (tests/test_gpu_maskfrozen.py's flow with dis.norm sn)
# ---------------------------------------------------------------------------------------------------------------------------
def _sn_frozen_checks(res, bounds):
    """every recorded chunk taken by exactly one oracle activation (dis_update: the generator passes are forward-only, nothing recorded),
    u / v after each update within 1e-5 of the oracle's, and per-network gradient bounds"""
    from test_gpu_maskfrozen import _per_net
    for which in ("dis", "gen"):
        r = res[which]
        assert r["used"].count(1) == r["chunks"] == r["matched"], (which, r["chunks"], r["matched"], r["used"].count(0), r["unmatched"][:6])
        assert r["matched"] >= (0.3 if which == "dis" else 0.9) * r["acts"], (which, r["matched"], r["acts"])
        assert r["uv"] <= 1e-5, (which, r["uv"])
        worst = _per_net(r["frozen"])
        print("SN %s_update worst relative L2 per network: %s" % (which, {k: "%.2e" % v for k, v in worst.items()}))
        group = lambda key: "dis" if key.startswith("dis") else "gen" + key[key.index("."):]      # noqa: E731  (ETOL_FROZEN's keys)
        bad = {k: v for k, v in worst.items() if v > (bounds[group(k)] if isinstance(bounds, dict) else bounds)}
        assert not bad, (which, bad, r["frozen"][:6])
        # the SN tensors themselves are in the comparison: weight_bar (through the fold) and the SN biases of every discriminator
        if which == "dis":
            keys = {k for _, n, k in r["frozen"]}
            assert any(k.endswith("conv.module.weight_bar") for k in keys) and any(k.endswith("conv.module.bias") for k in keys)


@pytest.fixture()
def lanes3(L):
    prev = _tune(L, b"lanes", 3)
    try:
        yield
    finally:
        _tune(L, b"lanes", prev)


@pytest.mark.parametrize("det", [False, True], ids=["default-plan-3-lanes", "deterministic"])
def test_sn_backward_parity_with_frozen_masks_fp32_benchmarked_batch(L, T, lanes3, det):
    """male2female_sn.yaml's networks at 256x256 B=8 (default plan with 3 lanes, and deterministic mode): every gradient tensor of both
    updates -- weight_bar through the fold, the SN biases, the generator gradients through the four frozen SN discriminator calls --
    within 1e-3 relative L2 of the fp32 oracle run with the update's own masks"""
    from gpu_util import deterministic_mode
    from test_gpu_maskfrozen import _frozen_and_free
    from test_gpu_maskfrozen import _mask_capture_bytes
    with deterministic_mode(L, det):
        res = _frozen_and_free(T, None, 8, 256, 37, cap_bytes=_mask_capture_bytes(T, 8, 256, 37, sn=True), free=False, sn=True)
    _sn_frozen_checks(res, 1e-3)


@pytest.mark.parametrize("dt,B", [("bf16", 8), ("fp16", 32)])
def test_sn_backward_parity_with_frozen_masks_16bit_benchmarked_batch(L, T, lanes3, dt, B):
    """bf16 B=8 / fp16 B=32 against the emulated 16-bit contract (the quantised weight is q(W_bar / sigma)), four distinct samples
    repeated, with the bounds of tests/test_gpu_maskfrozen.py (ETOL_FROZEN_BATCH, never above ETOL_FROZEN)"""
    from test_gpu_maskfrozen import ETOL_FROZEN, ETOL_FROZEN_BATCH, _frozen_and_free, _mask_capture_bytes
    res = _frozen_and_free(T, dt, B, 256, 37, cap_bytes=_mask_capture_bytes(T, B, 256, 37, dt, sn=True), d=4, sn=True)
    bounds = {k: min(ETOL_FROZEN_BATCH[dt][k], ETOL_FROZEN[dt][k]) for k in ETOL_FROZEN[dt]}
    _sn_frozen_checks(res, bounds)


def test_sn_backward_parity_with_frozen_masks_fp32_small(L, T):
    """the same flow at 64x64 B=2 (full width, the library's default plan and lanes): quick, and already at 1e-3 -- a fold that uses
    another call's u / v or loses one call's contribution moves the weight_bar gradients by 1e-2 and more"""
    from test_gpu_maskfrozen import _frozen_and_free
    res = _frozen_and_free(T, None, 2, 64, 38, sn=True)
    _sn_frozen_checks(res, 1e-3)
