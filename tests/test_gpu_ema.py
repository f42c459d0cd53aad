"""The averaged generator on the GPU.

Operator level (the EMA instantiations of adam_kernel, csrc/optimizer.hip, through aclgan_adam_flat_ema and, for the loss-scaled path,
a context with aclgan_bind_loss_scale + aclgan_bind_ema + aclgan_adam_step_ema):
  p, m, v bit-identical to the launch without the average; the average against its formula in fp64 from the same fp32 inputs; copy mode
  (also over a non-finite old average); a skipped fp16 update leaves everything untouched.
  Sizes: 16384 * 256 + 77 floats (one full pass of the capped grid, a second, ragged one) and the full-width generator group
  (30 058 648 floats: 7 passes and a ragged eighth).

The bound of the blend, per element: ema = fma(d, ema_old, fl((1 - d) * p_new)) has two fp32 roundings, the product and the fused result,
each at most 2^-24 of a magnitude no larger than max(|ema_old|, |p_new|) (the result is a convex combination of the two); the test allows
twice their sum, 2^-22 * max(|ema_old|, |p_new|).  Over k blended updates the trainer-level recurrence may collect k times that.

Trainer level (the reduced architecture of tests/golden/step_reduced_64.json, 64x64, B = 2): training is bit-identical with the average
on and off; the copy-then-blend recurrence; sample() from the average equals a plain sample() of a trainer that holds the average as
its live weights (fp32 and bf16); checkpoints; a skipped fp16 update."""
import ctypes as C
import json
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import aclgan_oracle as O
from conftest import GOLDEN
from gpu_util import deterministic_mode

pytestmark = pytest.mark.gpu

N_FLAT = 16384 * 256 + 77
FULL = (3, 6, 64, 256, 8, 4, 2, 4, 64, 4, 3)
B1, B2, EPS, WD, LR = 0.5, 0.999, 1e-8, 1e-4, 1e-4
EPS_BLEND = 2.0 ** -22


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


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _inputs(n, seed):
    """p over 1e-3 .. 1, gradients over 1e-6 .. 1, Adam state as after a few updates, an old average near p (all random signs)"""
    g = torch.Generator().manual_seed(seed)

    def mag(lo, hi):
        return 10.0 ** (torch.rand(n, generator=g) * (hi - lo) + lo)

    def sign():
        return torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    p = mag(-3, 0) * sign()
    grad = mag(-6, 0) * sign()
    m = 0.5 * grad * torch.rand(n, generator=g)
    v = (grad * grad) * 0.001 * torch.rand(n, generator=g)
    ema = p * (1 + 0.1 * (torch.rand(n, generator=g) - 0.5)) + 1e-3 * (torch.rand(n, generator=g) - 0.5)
    return {k: t.float().cuda() for k, t in dict(p=p, g=grad, m=m, v=v, ema=ema).items()}


@pytest.fixture(scope="module")
def flat():
    return _inputs(N_FLAT, 1234)      # read-only: every test clones what a launch overwrites


def _adam(L):
    return L.Adam(LR, B1, B2, EPS, WD)


def _plain(L, x, step):
    p, m, v = x["p"].clone(), x["m"].clone(), x["v"].clone()
    L.check(L.lib.aclgan_adam_flat(L.ptr(p), L.ptr(x["g"]), L.ptr(m), L.ptr(v), p.numel(), C.byref(_adam(L)), step, L.stream_ptr()), "adam_flat")
    return p, m, v


def _with_ema(L, x, step, decay, mode, ema0=None):
    p, m, v = x["p"].clone(), x["m"].clone(), x["v"].clone()
    ema = (x["ema"] if ema0 is None else ema0).clone()
    L.check(L.lib.aclgan_adam_flat_ema(L.ptr(p), L.ptr(x["g"]), L.ptr(m), L.ptr(v), L.ptr(ema), p.numel(), C.byref(_adam(L)), step, decay, mode,
                                       L.stream_ptr()), "adam_flat_ema")
    return p, m, v, ema


def _blend_excess(ema_new, ema_old, p_new, decay):
    """max over the elements of |ema_new - fp64 formula| / (2^-22 max(|ema_old|, |p_new|)): <= 1 passes.  The formula takes what the kernel
    takes: float32(d), and 1 - float32(d) evaluated in fp32 (exact for d >= 0.5)"""
    d32 = np.float32(decay)
    one_minus = np.float32(1.0) - d32
    ref = float(d32) * ema_old.double() + float(one_minus) * p_new.double()
    bound = EPS_BLEND * torch.maximum(ema_old.abs(), p_new.abs()).double()
    assert float(bound.min()) > 0
    return float(((ema_new.double() - ref).abs() / bound).max())


# ---------------------------------------------------------------- operator level
@pytest.mark.parametrize("step", [1, 7])
@pytest.mark.parametrize("mode", ["copy", "blend"])
def test_p_m_v_are_bit_identical_to_the_launch_without_the_average(L, flat, mode, step):
    assert N_FLAT % 256 != 0 and N_FLAT > 16384 * 256
    want = _plain(L, flat, step)
    got = _with_ema(L, flat, step, 0.999, L.EMA_BLEND if mode == "blend" else L.EMA_COPY)
    torch.cuda.synchronize()
    for name, a, b in zip("pmv", got, want):
        assert same_bits(a, b), name
    assert not same_bits(want[0], flat["p"])      # (an update happened)


@pytest.mark.parametrize("decay", [0.5, 0.999])
def test_blend_meets_the_two_rounding_bound(L, flat, decay):
    p, _, _, ema = _with_ema(L, flat, 7, decay, L.EMA_BLEND)
    excess = _blend_excess(ema, flat["ema"], p, decay)
    print("\nblend d=%g: max |ema - fp64| / (2^-22 max(|ema_old|, |p_new|)) = %.3f" % (decay, excess))
    assert excess <= 1.0
    assert not same_bits(ema, flat["ema"]) and not same_bits(ema, p)


def test_copy_mode_writes_p_new_also_over_a_non_finite_average(L, flat):
    p, _, _, ema = _with_ema(L, flat, 1, 0.999, L.EMA_COPY)
    assert same_bits(ema, p)
    bad = flat["ema"].clone()
    bad[0::3] = float("nan"); bad[1::3] = float("inf"); bad[2::7] = float("-inf")
    bad[-1] = float("nan"); bad[16384 * 256 - 1] = float("inf"); bad[16384 * 256] = float("nan")
    p2, _, _, ema2 = _with_ema(L, flat, 1, 0.999, L.EMA_COPY, ema0=bad)
    assert same_bits(p2, p) and same_bits(ema2, p)
    assert bool(torch.isfinite(ema2).all())


def test_loss_scaled_variant_blends_and_a_skipped_update_touches_nothing(L):
    ctx = C.c_void_p()
    L.check(L.lib.aclgan_ctx_create(C.byref(L.Arch(*FULL)), C.byref(ctx)), "ctx_create")
    try:
        n = L.lib.aclgan_group_numel(ctx, L.GROUP_GEN)
        assert n % 256 != 0 and n > 16384 * 256
        S = 65536.0
        x = _inputs(n, 99)
        x["g"] = x["g"] * S                       # the buffer carries S * g
        p, m, v, ema = (x[k].clone() for k in ("p", "m", "v", "ema"))
        state = torch.tensor([S, 1.0 / S, 0, 0, 0, 0, 0, 0], dtype=torch.float32, device="cuda")
        L.check(L.lib.aclgan_bind_params(ctx, L.GROUP_GEN, L.ptr(p), L.ptr(x["g"]), L.ptr(m), L.ptr(v)), "bind_params")
        L.check(L.lib.aclgan_bind_loss_scale(ctx, L.ptr(state)), "bind_loss_scale")
        L.check(L.lib.aclgan_bind_ema(ctx, L.GROUP_GEN, L.ptr(ema)), "bind_ema")
        adam = _adam(L)
        # finite gradients: the update is applied, the average blends
        L.check(L.lib.aclgan_adam_step_ema(ctx, L.GROUP_GEN, C.byref(adam), 3, 0.999, L.EMA_BLEND, L.stream_ptr()), "adam_step_ema")
        assert state.cpu().tolist() == [S, 1.0 / S, 1, 0, 0, 0, 0, S]
        excess = _blend_excess(ema, x["ema"], p, 0.999)
        print("\nloss-scaled blend: max |ema - fp64| / bound = %.3f" % excess)
        assert excess <= 1.0 and not same_bits(p, x["p"])
        # ... and p, m, v are what aclgan_adam_step gives from the same state
        p1, m1, v1 = x["p"].clone(), x["m"].clone(), x["v"].clone()
        state.copy_(torch.tensor([S, 1.0 / S, 0, 0, 0, 0, 0, 0]))
        L.check(L.lib.aclgan_bind_params(ctx, L.GROUP_GEN, L.ptr(p1), L.ptr(x["g"]), L.ptr(m1), L.ptr(v1)), "bind_params")
        L.check(L.lib.aclgan_adam_step(ctx, L.GROUP_GEN, C.byref(adam), 3, L.stream_ptr()), "adam_step")
        assert same_bits(p1, p) and same_bits(m1, m) and same_bits(v1, v)
        # one non-finite gradient, in the ragged tail of the last pass: nothing moves, the skip is counted
        L.check(L.lib.aclgan_bind_params(ctx, L.GROUP_GEN, L.ptr(p), L.ptr(x["g"]), L.ptr(m), L.ptr(v)), "bind_params")
        before = [t.clone() for t in (p, m, v, ema)]
        x["g"][n - 1] = float("inf")
        L.check(L.lib.aclgan_adam_step_ema(ctx, L.GROUP_GEN, C.byref(adam), 4, 0.999, L.EMA_BLEND, L.stream_ptr()), "adam_step_ema")
        L.check(L.lib.aclgan_adam_step_ema(ctx, L.GROUP_GEN, C.byref(adam), 5, 0.999, L.EMA_COPY, L.stream_ptr()), "adam_step_ema")
        assert state.cpu().tolist() == [S / 4, 4.0 / S, 0, 0, 2, 0, 0, S / 2]
        for name, a, b in zip(("p", "m", "v", "ema"), (p, m, v, ema), before):
            assert same_bits(a, b), name
    finally:
        torch.cuda.synchronize()
        L.lib.aclgan_ctx_destroy(ctx)


# ---------------------------------------------------------------- trainer level
@pytest.fixture(scope="module")
def fix():
    meta = json.load(open(os.path.join(GOLDEN, "step_reduced_64.json")))
    data = np.load(os.path.join(GOLDEN, "step_reduced_64.npz"))
    cfg = meta["config"]
    x_a, x_b = torch.from_numpy(data["x_a"]), torch.from_numpy(data["x_b"])
    z = [torch.from_numpy(data["z%d" % i]) for i in range(6)]
    assert tuple(x_a.shape) == (2, 3, 64, 64) and cfg["display_size"] == 2
    return cfg, O.test_nets(cfg, 0), x_a, x_b, z


def _make(T, fix, dtype="fp32", **keys):
    cfg, nets = dict(fix[0], **keys), fix[1]
    tr = T.aclgan_Trainer(cfg, compute_dtype=dtype, deterministic=True)
    for name in O.OracleTrainer.NETS:
        getattr(tr, name).load_state_dict(nets[name], strict=False)
    if tr._ema is not None:
        tr.ema_reset()      # the average was taken from the initialisation: start it from the weights just loaded
        assert same_bits(tr._ema, tr._param[0])
    return tr, cfg


def _iteration(tr, cfg, fix):
    _, _, x_a, x_b, z = fix
    tr.dis_update(x_a, x_b, cfg, z=z[:3])
    tr.gen_update(x_a, x_b, cfg, z=z[3:])


def test_training_is_bit_identical_with_the_average_on_and_off(L, T, fix):
    with deterministic_mode(L, True):
        on, c_on = _make(T, fix, ema_decay=0.5)
        off, c_off = _make(T, fix)
        assert off._ema is None and on._ema is not None
        for it in range(2):
            _iteration(on, c_on, fix); _iteration(off, c_off, fix)
            torch.cuda.synchronize()
            assert same_bits(on._losses, off._losses), it
            for grp in (0, 1):
                for name in ("_param", "_m", "_v"):
                    assert same_bits(getattr(on, name)[grp], getattr(off, name)[grp]), (it, grp, name)
        assert float(off._losses.abs().sum()) > 0 and not same_bits(on._ema, on._param[0])
        assert on.ema_updates == 2


def test_average_follows_copy_then_blend_over_four_generator_updates(L, T, fix):
    with deterministic_mode(L, True):
        tr, cfg = _make(T, fix, ema_decay=0.5, ema_start=1)
        _, _, x_a, x_b, z = fix
        ps = []
        for _ in range(4):
            tr.gen_update(x_a, x_b, cfg, z=z[3:])
            ps.append(tr._param[0].clone())
        ref = ps[0].double()                                  # update 1 <= ema_start: copy
        for p in ps[1:]:
            ref = 0.5 * ref + 0.5 * p.double()                # updates 2 .. 4: blend
        k = 3
        bound = k * EPS_BLEND * torch.stack([p.abs() for p in ps]).max(0).values.double()
        err = (tr._ema.double() - ref).abs()
        live = bound > 0                                      # (alignment padding between tensors stays exactly zero)
        print("\nrecurrence: max err / bound = %.3f over %d elements" % (float((err[live] / bound[live]).max()), int(live.sum())))
        assert bool((err <= bound).all())
        assert not same_bits(tr._ema, tr._param[0]) and float((tr._ema - tr._param[0]).abs().max()) > 0
        assert tr.ema_updates == 4


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_forward_reads_the_average_inside_the_context_manager_and_updates_never_do(L, T, fix, dtype):
    _, _, x_a, x_b, z = fix
    with deterministic_mode(L, True):
        a, cfg = _make(T, fix, dtype, ema_decay=0.5)
        twin, _ = _make(T, fix, dtype, ema_decay=0.5)
        _iteration(a, cfg, fix); _iteration(twin, cfg, fix)
        assert same_bits(a._param[0], twin._param[0]) and same_bits(a._ema, twin._ema) and not same_bits(a._ema, a._param[0])
        plain, _ = _make(T, fix, dtype)
        sd = a.ema_state_dict()
        assert list(sd["AB"].keys()) == list(a.gen_AB.state_dict().keys()) and list(sd["BA"].keys()) == list(a.gen_BA.state_dict().keys())
        assert all(v.shape == w.shape for v, w in zip(sd["AB"].values(), a.gen_AB.state_dict().values()))
        plain.gen_AB.load_state_dict(sd["AB"]); plain.gen_BA.load_state_dict(sd["BA"])
        assert same_bits(plain._param[0], a._ema)
        plain.z_1, plain.z_2, plain.z_3 = a.z_1, a.z_2, a.z_3
        before = a.sample(x_a, x_b)
        with a.ema_weights():
            inside = a.sample(x_a, x_b)
        want = plain.sample(x_a, x_b)
        assert len(inside) == len(want) == 9
        for i, (u, w) in enumerate(zip(inside, want)):
            assert same_bits(u, w), i
        assert any(not same_bits(u, w) for u, w in zip(inside[1:], before[1:]))      # the average is not the live generator
        for i, (u, w) in enumerate(zip(a.sample(x_a, x_b, ema=True), want)):
            assert same_bits(u, w), i
        # the live selection is back: after a normal exit, and after an exception
        for i, (u, w) in enumerate(zip(a.sample(x_a, x_b), before)):
            assert same_bits(u, w), i
        with pytest.raises(ZeroDivisionError):
            with a.ema_weights():
                1 / 0
        for i, (u, w) in enumerate(zip(a.sample(x_a, x_b), before)):
            assert same_bits(u, w), i
        # an update inside the context manager reads (and writes) the live weights
        with a.ema_weights():
            a.gen_update(x_a, x_b, cfg, z=z[3:])
        twin.gen_update(x_a, x_b, cfg, z=z[3:])
        torch.cuda.synchronize()
        assert same_bits(a._param[0], twin._param[0]) and same_bits(a._ema, twin._ema) and same_bits(a._losses, twin._losses)
        with pytest.raises(L.AclganError):
            with plain.ema_weights():
                pass
        with pytest.raises(L.AclganError):
            plain.sample(x_a, x_b, ema=True)
        with pytest.raises(L.AclganError):
            plain.ema_state_dict()


def test_checkpoints_carry_the_average_under_a_name_resume_does_not_mistake(L, T, fix, tmp_path):
    with deterministic_mode(L, True):
        tr, cfg = _make(T, fix, ema_decay=0.5)
        off, c_off = _make(T, fix)
        for _ in range(2):
            _iteration(tr, cfg, fix); _iteration(off, c_off, fix)
        d_on, d_off = tmp_path / "on", tmp_path / "off"
        d_on.mkdir(); d_off.mkdir()
        tr.save(str(d_on), 41); off.save(str(d_off), 41)
        assert sorted(os.listdir(d_off)) == ["dis_00000042.pt", "gen_00000042.pt", "optimizer.pt"]
        assert sorted(os.listdir(d_on)) == ["dis_00000042.pt", "ema_00000042.pt", "gen_00000042.pt", "optimizer.pt"]
        assert tr._get_model_list(str(d_on), "gen") == str(d_on / "gen_00000042.pt")
        assert tr._get_model_list(str(d_on), "dis") == str(d_on / "dis_00000042.pt")
        # the three files of a run without the average hold what they hold today
        for name in ("gen_00000042.pt", "dis_00000042.pt"):
            x, y = torch.load(str(d_on / name)), torch.load(str(d_off / name))
            assert list(x.keys()) == list(y.keys())
            for net in x:
                assert list(x[net].keys()) == list(y[net].keys()) and all(torch.equal(x[net][k], y[net][k]) for k in x[net]), (name, net)
        x, y = torch.load(str(d_on / "optimizer.pt")), torch.load(str(d_off / "optimizer.pt"))
        assert list(x.keys()) == list(y.keys()) == ["gen", "dis"]
        for grp in x:
            assert x[grp]["param_groups"] == y[grp]["param_groups"] and list(x[grp]["state"].keys()) == list(y[grp]["state"].keys())
            for i in x[grp]["state"]:
                assert all(torch.equal(x[grp]["state"][i][k], y[grp]["state"][i][k]) for k in ("step", "exp_avg", "exp_avg_sq")), (grp, i)
        sd = torch.load(str(d_on / "ema_00000042.pt"))
        assert set(sd.keys()) == {"AB", "BA", "updates", "decay"} and sd["updates"] == 2 and sd["decay"] == 0.5
        assert list(sd["AB"].keys()) == list(tr.gen_AB.state_dict().keys())
        # a fresh trainer resumes the average bitwise, and the update count
        fresh = T.aclgan_Trainer(cfg, deterministic=True)
        assert fresh.resume(str(d_on), cfg) == 42
        assert same_bits(fresh._ema, tr._ema) and same_bits(fresh._param[0], tr._param[0]) and fresh.ema_updates == 2
        assert not same_bits(fresh._ema, fresh._param[0])
        # without the file the average starts from the resumed weights, with a warning
        os.remove(str(d_on / "ema_00000042.pt"))
        fresh2 = T.aclgan_Trainer(cfg, deterministic=True)
        with pytest.warns(UserWarning, match="ema_00000042.pt"):
            assert fresh2.resume(str(d_on), cfg) == 42
        assert same_bits(fresh2._param[0], tr._param[0]) and same_bits(fresh2._ema, fresh2._param[0])
        # a trainer without the average resumes the same directory silently
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            off2 = T.aclgan_Trainer(c_off, deterministic=True)
            assert off2.resume(str(d_on), c_off) == 42 and off2._ema is None


def test_skipped_fp16_update_leaves_the_average_untouched(L, T, fix):
    _, _, x_a, x_b, z = fix
    with deterministic_mode(L, True):
        tr, cfg = _make(T, fix, "fp16", ema_decay=0.5, loss_scale_init=2.0 ** 60)
        tr._ema.mul_(1.25)      # an average that is not the live weights: a copy or a blend would show
        ema0, p0 = tr._ema.clone(), tr._param[0].clone()
        tr.gen_update(x_a, x_b, cfg, z=z[3:])
        torch.cuda.synchronize()
        assert tr.loss_scale_state()["skipped_gen"] == 1
        assert same_bits(tr._ema, ema0) and same_bits(tr._param[0], p0)
        assert tr.ema_updates == 1      # (Adam's step counts skipped updates, as before)
