"""Differentiable augmentation of the discriminator inputs on the GPU (csrc/augment.hip, aclgan_ctx_set_augment, config key dis_augment):
the operator against the fp64 reference of tests/diffaug_ref.py, both updates against the fp32 oracle with its dis_forward wrapped,
neutral rows changing no bit, lanes and graph replay, and the error paths.  Run on the GPU box: pytest -m gpu"""
import copy
import ctypes as C

import pytest
import torch

from oracle import aclgan_oracle as O
from diffaug_ref import DIS_BLOCKS, GEN_BLOCKS, diffaug_bwd_ref, diffaug_ref, neutral_params, oracle_dis_forward
from gpu_util import deterministic_mode, nchw, nhwc, rel_err

pytestmark = pytest.mark.gpu

TOL = 2e-4      # the project's operator bound (tests/test_gpu_ops_misc.py)


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def T(L):
    from aclgan_amd import trainer
    return trainer


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the operator
# ---------------------------------------------------------------------------------------------------------------------------------
def _extreme_rows(H, W):
    """shifts of +-Sx, +-Sy; the rectangle over each corner and fully outside; saturation 0, contrast 0.5"""
    sx, sy, ch, cw = int(W / 8 + 0.5), int(H / 8 + 0.5), (H + 1) // 2, (W + 1) // 2
    x0, x1, y0, y1 = -(cw // 2), W - cw % 2 - cw // 2, -(ch // 2), H - ch % 2 - ch // 2      # the ends of draw_augment_params' ranges
    return torch.tensor([[0.3, 0.0, 0.5, sx, sy, x0, y0, 0],
                         [-0.4, 1.7, 1.4, -sx, -sy, x1, y1, 0],
                         [0.2, 0.0, 1.0, sx, -sy, x1, y0, 0],
                         [-0.1, 1.0, 0.5, -sx, sy, x0, y1, 0],
                         [0.5, 2.0, 0.5, 0, 0, W, H, 0],
                         [-0.5, 0.0, 0.5, sx, 0, W, 0, 0]], dtype=torch.float32)


def _gpu_op(L, x, p, policy, dy=None, dx=None):
    """forward (dy None) or backward (into dx when given: accumulate) of the operator on NHWC device tensors"""
    N, H, W, Cc = x.shape if dy is None else dy.shape
    nb = L.lib.aclgan_diffaugment_scratch_bytes(N, H, W, Cc)
    scratch = torch.empty(nb // 4 + 16, device="cuda")
    if dy is None:
        y = torch.full_like(x, float("nan"))
        L.check(L.lib.aclgan_diffaugment_fwd(N, H, W, Cc, policy, L.ptr(x), L.ptr(p), L.ptr(y), L.ptr(scratch), L.stream_ptr()), "diffaugment_fwd")
        return y
    acc = dx is not None
    if not acc:
        dx = torch.full_like(dy, float("nan"))
    L.check(L.lib.aclgan_diffaugment_bwd(N, H, W, Cc, policy, L.ptr(dy), L.ptr(p), L.ptr(dx), 1 if acc else 0, L.ptr(scratch), L.stream_ptr()),
            "diffaugment_bwd")
    return dx


@pytest.mark.parametrize("shape", [(5, 3, 20, 12), (4, 6, 10, 16), (2, 6, 7, 9), (3, 3, 64, 96)])
def test_operator_matches_fp64(L, T, shape):
    """all 7 policies, random rows and the extreme ones: forward, backward (overwrite and accumulate) against fp64; two calls give the same
    bits; without the colour bit, no shift and the rectangle outside the frame, the output IS the input"""
    N, Cc, H, W = shape
    g = torch.Generator().manual_seed(100 + H)
    ext = _extreme_rows(H, W)
    sets = [T.draw_augment_params(7, N, H, W, g)]
    for k in range(0, len(ext), N):
        sets.append(torch.cat([ext[k:k + N], T.draw_augment_params(7, N, H, W, g)])[:N])
    x = torch.randn(N, Cc, H, W, generator=g)
    dy = torch.randn(N, Cc, H, W, generator=g)
    dx0 = torch.randn(N, Cc, H, W, generator=g)
    xd, dyd = nhwc(x).cuda(), nhwc(dy).cuda()
    worst = {"fwd": 0.0, "bwd": 0.0, "acc": 0.0}
    for policy in range(1, 8):
        for p in sets:
            pd = p.cuda()
            ref_y = diffaug_ref(x.double(), p.double(), policy)
            ref_dx = diffaug_bwd_ref(dy.double(), p.double(), policy)
            y = _gpu_op(L, xd, pd, policy)
            dx = _gpu_op(L, None, pd, policy, dy=dyd)
            dxa = _gpu_op(L, None, pd, policy, dy=dyd, dx=nhwc(dx0).cuda())
            assert torch.equal(y, _gpu_op(L, xd, pd, policy)) and torch.equal(dx, _gpu_op(L, None, pd, policy, dy=dyd)), (policy, "not reproducible")
            e = (rel_err(nchw(y), ref_y), rel_err(nchw(dx), ref_dx), rel_err(nchw(dxa), ref_dx + dx0.double()))
            worst = {k: max(worst[k], v) for k, v in zip(worst, e)}
            assert max(e) < TOL, (shape, policy, e)
            if not policy & 1:      # a masked gather: every output element is 0 or the bits of an input element
                ys = nchw(y).cpu()
                assert torch.equal(ys, diffaug_ref(x, p, policy))
    print("diffaugment %s worst rel_err fwd %.2e bwd %.2e bwd+acc %.2e" % (shape, worst["fwd"], worst["bwd"], worst["acc"]))
    neutral = neutral_params(N, H, W).cuda()
    for policy in (2, 4, 6):
        assert torch.equal(_gpu_op(L, xd, neutral, policy), xd)
        assert torch.equal(_gpu_op(L, None, neutral, policy, dy=dyd), dyd)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. both updates against the oracle
# ---------------------------------------------------------------------------------------------------------------------------------
def _make(T, cfg, nets, **kw):
    tr = T.aclgan_Trainer(cfg, **kw)
    for name in O.OracleTrainer.NETS:
        getattr(tr, name).load_state_dict(nets[name], strict=False)
    return tr


DIS_NETS, GEN_NETS = ("dis_A", "dis_B", "dis_2"), ("gen_AB", "gen_BA")


def _oracle_step(monkeypatch, cfg, nets, x_a, x_b, z, aug_d, aug_g, B):
    """(dis-update oracle, gen-update oracle) with dis_forward wrapped when rows are given"""
    orig = O.dis_forward
    out = []
    for which, aug, blocks in (("dis", aug_d, DIS_BLOCKS), ("gen", aug_g, GEN_BLOCKS)):
        orc = O.OracleTrainer(cfg, nets=nets)
        with monkeypatch.context() as m:
            w = None
            if aug is not None:
                w = oracle_dis_forward(orig, aug, B, 7, blocks)
                m.setattr(O, "dis_forward", w)
            if which == "dis":
                orc.dis_update(x_a, x_b, z[:3], apply=False)
            else:
                orc.gen_update(x_a, x_b, z[3:], apply=False)
            assert w is None or len(w.calls) == len(blocks)
        out.append(orc)
    return out


def _check_against_oracle(trd, trg, od, og, tag):
    """the bounds of tests/test_gpu_step.py::test_non_square_odd_batch_step_matches_oracle"""
    for n, v in list(od.losses.items()) + list(og.losses.items()):
        got = float(getattr(trd if n.startswith("loss_dis") else trg, n))
        print("%s %-26s gpu %+.6e oracle %+.6e" % (tag, n, got, v))
        assert abs(got - v) <= (5e-3 if n.endswith("_size") else 1e-3) * max(1e-3, abs(v)), (tag, n, got, v)
    for tr, orc, nets_ in ((trd, od, DIS_NETS), (trg, og, GEN_NETS)):
        gmax = max(float(t.grad.norm()) for n in nets_ for t in orc.nets[n].values())
        worst = 0.0
        for n in nets_:
            for k, gr in getattr(tr, n).named_grads():
                ref = orc.nets[n][k].grad
                err = (gr.cpu().double() - ref.double()).norm().item()
                worst = max(worst, err / (ref.double().norm().item() + 1e-5 * gmax / 3e-2))
                assert err <= 3e-2 * ref.double().norm().item() + 1e-5 * gmax, (tag, n, k, err)
        print("%s %s worst gradient error / bound: %.3f" % (tag, nets_[0][:3], worst / 3e-2))


def test_updates_match_the_oracle_with_wrapped_dis_forward(T, monkeypatch):
    """B=3, 64x96, reduced width, policy 7 with explicit rows: losses and every gradient tensor of dis_update and gen_update against the fp32
    oracle whose dis_forward augments its input with the row block of its call.  The discriminator weights are 10 x the fixture's
    gaussian(0.02) fill: at the fill's own scale the discriminator outputs barely depend on their input and the test would pass without
    the feature -- the sensitivity is asserted.  Control: the same nets and inputs with the key off against the unwrapped oracle."""
    cfg = O.default_config()
    cfg["gen"].update(dim=8, mlp_dim=16, n_res=2)
    cfg["dis"].update(dim=8)
    cfg["display_size"] = 1
    cfg["focus_epsilon"] = 0.5
    nets = O.test_nets(cfg, 4)
    for n in DIS_NETS:
        nets[n] = {k: (v * 10 if k.endswith("weight") else v) for k, v in nets[n].items()}
    B, H, W = 3, 64, 96
    g = torch.Generator().manual_seed(9)
    x_a = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    x_b = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    z = [torch.randn(B, 8, 1, 1, generator=g) for _ in range(6)]
    # (the rows: a seed at which the oracle-against-oracle sensitivity below holds with room -- losses >= 9e-2, gradients >= 0.16.  The
    #  gradient of a scalar head bias is one number, and at some draws the augmented and the plain one nearly coincide)
    ga = torch.Generator().manual_seed(2)
    aug_d = T.draw_augment_params(7, 7 * B, H, W, ga)
    aug_g = T.draw_augment_params(7, 5 * B, H, W, ga)
    od0, og0 = _oracle_step(monkeypatch, cfg, nets, x_a, x_b, z, None, None, B)
    od, og = _oracle_step(monkeypatch, cfg, nets, x_a, x_b, z, aug_d, aug_g, B)
    # the fixture sees the augmentation: every adversarial / discriminator loss and every discriminator gradient moves
    for n in list(od.losses) + list(og.losses):
        if "adv" in n or "dis" in n:
            a, b = (od if n.startswith("loss_dis") else og).losses[n], (od0 if n.startswith("loss_dis") else og0).losses[n]
            assert abs(a - b) >= 5e-2 * abs(b), ("insensitive loss", n, a, b)
    for n in DIS_NETS:
        for k, t in od.nets[n].items():
            ref = od0.nets[n][k].grad.double()
            assert (t.grad.double() - ref).norm() >= 0.1 * ref.norm(), ("insensitive gradient", n, k)
    # control: key off, unwrapped oracle
    trd = _make(T, cfg, nets); trd.dis_update(x_a, x_b, cfg, z=z[:3])
    trg = _make(T, cfg, nets); trg.gen_update(x_a, x_b, cfg, z=z[3:])
    assert trd.augment == 0
    _check_against_oracle(trd, trg, od0, og0, "control")
    # the feature
    cfga = copy.deepcopy(cfg)
    cfga["dis_augment"] = "color,translation,cutout"
    trd = _make(T, cfga, nets); trd.dis_update(x_a, x_b, cfga, z=z[:3], aug=aug_d)
    trg = _make(T, cfga, nets); trg.gen_update(x_a, x_b, cfga, z=z[3:], aug=aug_g)
    assert trd.augment == 7
    _check_against_oracle(trd, trg, od, og, "augment")


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. neutral geometry changes no bit
# ---------------------------------------------------------------------------------------------------------------------------------
def _reduced(norm="none"):
    cfg = O.default_config()
    cfg["gen"].update(dim=16, mlp_dim=32, n_res=2)
    cfg["dis"].update(dim=16, norm=norm)
    cfg["display_size"] = 1
    cfg["focus_epsilon"] = 0.5
    if norm == "sn":
        from sn_nets import sn_test_nets
        return cfg, sn_test_nets(cfg, 0)
    return cfg, O.test_nets(cfg, 0)


def _batch(B, S, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 3, S, S, generator=g) * 2 - 1, torch.rand(B, 3, S, S, generator=g) * 2 - 1,
            [torch.randn(B, 8, 1, 1, generator=g) for _ in range(6)])


def _both_updates(T, L, cfg, nets, x_a, x_b, z, aug_d=None, aug_g=None, **kw):
    """dis_update then gen_update, each on a fresh trainer: ({loss: value}, {(net, key): gradient}) per update"""
    out = {}
    for which in ("dis", "gen"):
        tr = _make(T, cfg, nets, **kw)
        if which == "dis":
            tr.dis_update(x_a, x_b, cfg, z=z[:3], aug=aug_d); names = DIS_NETS
        else:
            tr.gen_update(x_a, x_b, cfg, z=z[3:], aug=aug_g); names = GEN_NETS
        torch.cuda.synchronize()
        lnames = L.LOSS_NAMES[12:16] if which == "dis" else L.LOSS_NAMES[0:12]
        out[which] = ({n: float(getattr(tr, n)) for n in lnames},
                      {(n, k): gr.contiguous().clone() for n in names for k, gr in getattr(tr, n).named_grads()})
    return out


def _same(a, b):
    for which in ("dis", "gen"):
        la, ga = a[which]; lb, gb = b[which]
        assert la and ga
        assert la == lb, (which, {k: (la[k], lb[k]) for k in la if la[k] != lb[k]})
        diff = [k for k in ga if not torch.equal(ga[k], gb[k])]
        assert not diff, (which, len(diff), diff[:8])


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("norm", ["none", "sn"])
def test_neutral_geometry_changes_no_bit(T, L, norm, dtype):
    """deterministic mode, policy translation|cutout with neutral rows: the augmented tensors are copies, so losses and all gradients of
    both updates equal those of a trainer with the key off bit for bit -- the wiring (joint batches, views, one pass per call under sn,
    the fp32 tensors of the 16-bit modes) with no tolerance at all"""
    cfg, nets = _reduced(norm)
    B, S = 2, 64
    x_a, x_b, z = _batch(B, S, 41)
    cfga = copy.deepcopy(cfg)
    cfga["dis_augment"] = "translation,cutout"
    with deterministic_mode(L, True):
        off = _both_updates(T, L, cfg, nets, x_a, x_b, z, compute_dtype=dtype)
        on = _both_updates(T, L, cfga, nets, x_a, x_b, z, neutral_params(7 * B, S, S), neutral_params(5 * B, S, S), compute_dtype=dtype)
    _same(off, on)
    assert any(float(t.abs().max()) > 0 for t in off["gen"][1].values())


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. lanes and graph
# ---------------------------------------------------------------------------------------------------------------------------------
def _tune(L, key, value):
    prev = C.c_int()
    L.check(L.lib.aclgan_tuning(key, value, C.byref(prev)), "aclgan_tuning")
    return prev.value


def test_lane_count_does_not_change_a_bit_with_augmentation(T, L):
    cfg, nets = _reduced()
    cfg["dis_augment"] = "color,translation,cutout"
    B, S = 2, 64
    x_a, x_b, z = _batch(B, S, 42)
    g = torch.Generator().manual_seed(43)
    aug_d, aug_g = T.draw_augment_params(7, 7 * B, S, S, g), T.draw_augment_params(7, 5 * B, S, S, g)
    prev = _tune(L, b"lanes", 1)
    try:
        with deterministic_mode(L, True):
            one = _both_updates(T, L, cfg, nets, x_a, x_b, z, aug_d, aug_g)
            _tune(L, b"lanes", 3)
            _same(one, _both_updates(T, L, cfg, nets, x_a, x_b, z, aug_d, aug_g))
    finally:
        _tune(L, b"lanes", prev)


def test_graph_replay_reads_fresh_rows(T, L):
    """hip_graph=True: step 1 runs eagerly, step 2 captures, steps 3 and 4 replay -- with different rows every step; losses and every
    parameter equal the eager trainer's bit for bit (a replay that read stale rows would not)"""
    cfg, nets = _reduced()
    cfg["dis_augment"] = "color,translation,cutout"
    B, S = 2, 64
    g = torch.Generator().manual_seed(44)
    batches = [_batch(B, S, 50 + i) + (T.draw_augment_params(7, 7 * B, S, S, g), T.draw_augment_params(7, 5 * B, S, S, g)) for i in range(4)]

    def run(**kw):
        tr = _make(T, cfg, nets, **kw)
        losses = []
        for x_a, x_b, z, aug_d, aug_g in batches:
            tr.dis_update(x_a, x_b, cfg, z=z[:3], aug=aug_d)
            tr.gen_update(x_a, x_b, cfg, z=z[3:], aug=aug_g)
            losses.append((float(tr.loss_dis_total), float(tr.loss_gen_total)))
        torch.cuda.synchronize()
        return tr, losses, {k: v.detach().clone() for k, v in tr.named_parameters()}
    with deterministic_mode(L, True):
        te, le, pe = run()
        tg, lg, pg = run(hip_graph=True)
    assert tg.hip_graph, "capture fell back to eager execution"
    assert tg._graphs["gen"]["graph"] is not None and tg._graphs["dis"]["graph"] is not None
    assert le == lg, (le, lg)
    bad = [k for k in pe if not torch.equal(pe[k], pg[k])]
    assert not bad, bad[:6]
    assert len(set(le)) == len(le)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. errors
# ---------------------------------------------------------------------------------------------------------------------------------
def test_wrong_rows_and_missing_params_are_refused(T, L):
    cfg, nets = _reduced()
    cfg["dis_augment"] = "color,cutout"
    B, S = 2, 64
    x_a, x_b, z = _batch(B, S, 45)
    g = torch.Generator().manual_seed(46)
    aug_d, aug_g = T.draw_augment_params(5, 7 * B, S, S, g), T.draw_augment_params(5, 5 * B, S, S, g)
    with deterministic_mode(L, True):
        tr = _make(T, cfg, nets)
        n0 = L.lib.aclgan_launch_count()
        with pytest.raises(L.AclganError, match="%d augmentation rows" % (7 * B)):
            tr.dis_update(x_a, x_b, cfg, z=z[:3], aug=aug_g)             # 5 B rows where dis_update reads 7 B
        with pytest.raises(L.AclganError, match="%d augmentation rows" % (5 * B)):
            tr.gen_update(x_a, x_b, cfg, z=z[3:], aug=aug_d)
        with pytest.raises(L.AclganError):
            tr.gen_update(x_a, x_b, cfg, z=z[3:], aug=aug_g[:, :7])      # not (rows, 8)
        # the policy without its rows: refused by the library, before anything is enqueued
        L.check(L.lib.aclgan_ctx_set_augment(tr._ctx, 5, None, 5 * B))
        zz = torch.stack([t.reshape(B, 8) for t in z[3:]]).cuda().contiguous()
        xa, xb = x_a.cuda(), x_b.cuda()
        hpc = T.hparams_from_config(cfg)
        n1 = L.lib.aclgan_launch_count()
        with pytest.raises(L.AclganError, match="params = NULL"):
            L.check(L.lib.aclgan_gen_update(tr._ctx, L.ptr(xa), L.ptr(xb), L.ptr(zz), B, S, S, C.byref(hpc), L.ptr(tr._losses), L.stream_ptr()), "gen_update")
        assert L.lib.aclgan_launch_count() == n1
        # the trainer is usable afterwards, and gives the bits of one that never saw an error
        tr.dis_update(x_a, x_b, cfg, z=z[:3], aug=aug_d)
        got = {k: gr.contiguous().clone() for n in DIS_NETS for k, gr in ((n + "." + k, v) for k, v in getattr(tr, n).named_grads())}
        fresh = _make(T, cfg, nets)
        fresh.dis_update(x_a, x_b, cfg, z=z[:3], aug=aug_d)
        want = {k: gr.contiguous().clone() for n in DIS_NETS for k, gr in ((n + "." + k, v) for k, v in getattr(fresh, n).named_grads())}
        assert float(tr.loss_dis_total) == float(fresh.loss_dis_total)
        assert not [k for k in want if not torch.equal(want[k], got[k])]
        assert n0 < L.lib.aclgan_launch_count()
    plain, _ = _reduced()
    with pytest.raises(L.AclganError, match="dis_augment"):
        _make(T, plain, nets).gen_update(x_a, x_b, plain, z=z[3:], aug=aug_g)
