"""R1 gradient penalty on real images on the GPU (csrc/r1.hip: aclgan_dis_r1; config keys r1_gamma / r1_every): the operator against the
fp64 double backward of the definition (tests/r1_ref.py), reproducibility, the trainer's placement, schedule and reporting, the key
switched off, graph replay, the forced single-rank RCCL path and the error paths.  Run on the GPU box: pytest -m gpu"""
import functools
import json
import os

import pytest
import torch

from oracle import aclgan_oracle as O
from gpu_util import deterministic_mode, rel_err
from r1_ref import dis_cfg, r1_autograd, r1_closed_form, separated_biases

pytestmark = pytest.mark.gpu

# Worst rel_err (max |got - ref| / max |ref| per tensor) of P, grad_x and every weight-gradient tensor against the fp64 oracle, measured on
# the MI355X (profiles/r1_parity.json): reduced width 6.1e-7 (64x64 B=2), 5.9e-7 (64x96), 4.7e-7 (B=3), 5.9e-7 (dis_2); full width 7.0e-7;
# the trainer 5.8e-7 in fp32, bf16 and fp16 alike (the pass is fp32).  MEASURED_REL_ERR is the worst of them; the bound is 4 x that, for
# the run-to-run variation of the non-deterministic accumulation order.  (For scale: the mask-frozen update gradients of
# tests/test_gpu_maskfrozen.py agree to 1.3e-5.)
MEASURED_REL_ERR = 7.1e-7
TOL = None if MEASURED_REL_ERR is None else 4 * MEASURED_REL_ERR
# hip_graph=True against the eager run after 3 iterations (relative L2 of the discriminators' parameter and gradient buffers): the eager
# run's own spread when the pass runs after the update instead of before it (the order a replayed update has), measured on the MI355X in
# deterministic mode (profiles/r1_parity.json: "order_spread"): 0.0 -- every weight tensor receives one sum from the pass and one from
# the update, and an fp32 addition commutes.  The bound is 4 x that: the same bits.
MEASURED_ORDER_SPREAD = 0.0
ORDER_TOL = None if MEASURED_ORDER_SPREAD is None else 4 * MEASURED_ORDER_SPREAD

GAMMA = 10.0
# At the fixture's gaussian(0.02) weights the gradient of the penalty is 1e-8 of the adversarial one: where both have to carry weight
# (graph replay against the eager run) gamma is raised until they are of one order.
GAMMA_BIG = 1e8
MEASURED = {}      # what this run measured, written to $ACLGAN_R1_PARITY_OUT (a JSON file) when that is set


def _record(key, value):
    MEASURED[key] = value
    out = os.environ.get("ACLGAN_R1_PARITY_OUT")
    if out:
        with open(out, "w") as f:
            json.dump(MEASURED, f, indent=1, sort_keys=True)


def _check(tag, errs):
    """print every figure, record the worst, then assert the bound"""
    worst = max(errs.values())
    for k, v in errs.items():
        print("%s %-28s rel_err %.3e" % (tag, k, v))
    _record(tag, {"worst": worst, "tensor": max(errs, key=errs.get)})
    assert TOL is not None, "no measured bound yet: run on the MI355X, fill MEASURED_REL_ERR (this run's worst: %.3e)" % worst
    assert worst <= TOL, (tag, {k: v for k, v in errs.items() if v > TOL})


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


def _cfg(dis_dim=4, **keys):
    cfg = O.default_config()
    cfg["gen"].update(dim=8, mlp_dim=16, n_res=1)
    cfg["dis"].update(dim=dis_dim)
    cfg["display_size"] = 1
    cfg.update(keys)
    return cfg


def _make(T, cfg, nets, **kw):
    tr = T.aclgan_Trainer(cfg, **kw)
    for name in O.OracleTrainer.NETS:
        getattr(tr, name).load_state_dict(nets[name], strict=False)
    return tr


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the operator against fp64
# ---------------------------------------------------------------------------------------------------------------------------------
# name -> (dis.dim, net, B, H, W, seed, separated biases, required margin).  The seeds were picked on the CPU so that the smallest
# |z| / rms(z of its layer) over all LeakyReLU inputs of the fp64 oracle meets the margin (reduced width: 1.4e-4, 8.5e-5, 3.8e-5, 2.1e-4;
# full width with biases of 4 x the layer's rms and a random sign per channel: 1.4e-2): no fp32 chain takes another branch than the oracle.
CASES = {
    "reduced_64x64_b2": (4, "dis_A", 2, 64, 64, 4, False, 2e-5),
    "reduced_64x96_b2": (4, "dis_A", 2, 64, 96, 1, False, 2e-5),
    "reduced_64x64_b3": (4, "dis_B", 3, 64, 64, 2, False, 2e-5),
    "reduced_dis2_64x64_b2": (4, "dis_2", 2, 64, 64, 4, False, 2e-5),
    "full_64x64_b2": (64, "dis_A", 2, 64, 64, 0, True, 1e-4),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(dcfg, fp32 parameters, fp32 images, fp64 oracle (P, G, grads)) of a case, computed once"""
    dim, net, B, H, W, seed, sep, need = CASES[name]
    Cin = 6 if net == "dis_2" else 3
    dcfg = dis_cfg(dim, 4, 3)
    P = O.seeded_fill(O.dis_param_shapes(Cin, dcfg), "gaussian", seed)
    x = torch.rand(B, Cin, H, W, generator=torch.Generator().manual_seed(1000 + seed)) * 2 - 1
    if sep:
        P = separated_biases(P, x, dcfg, 4.0, seed)
    margin = r1_closed_form(P, x.double(), dcfg, GAMMA)[3]
    assert margin >= need, "precondition: LeakyReLU margin %.2e of the fp64 oracle < %.0e (%s)" % (margin, need, name)
    ref = r1_autograd(P, x.double(), dcfg, GAMMA)
    return dcfg, P, x, ref


def _run_op(L, tr, net, x, gamma, want_gx=True, sentinel=1.5, zero=True):
    """aclgan_dis_r1 on the trainer's context: (P, grad_x, {key: gradient}, gradient buffer).  The buffer is filled with `sentinel` except the
    weight tensors of `net`, which are zeroed."""
    B, Cin, H, W = x.shape
    xd = x.cuda().contiguous()
    nb = L.lib.aclgan_dis_r1_scratch_bytes(tr._ctx, L.NETS[net], B, H, W)
    assert nb > 0, L.last_error()
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda")
    buf = tr._grad[L.GROUP_DIS]
    if zero:
        buf.fill_(sentinel)
        for k, v in getattr(tr, net).named_grads():
            if k.endswith("weight"):
                v.zero_()
    pen = torch.full((1,), float("nan"), device="cuda")
    gx = torch.full_like(xd, float("nan")) if want_gx else None
    L.check(L.lib.aclgan_dis_r1(tr._ctx, L.NETS[net], L.ptr(xd), B, H, W, gamma, L.ptr(pen), L.ptr(gx), L.ptr(scratch), L.stream_ptr()), "dis_r1")
    torch.cuda.synchronize()
    grads = {k: v.contiguous().clone() for k, v in getattr(tr, net).named_grads()}
    return pen[0].clone(), gx, grads, buf.clone()


@functools.lru_cache(maxsize=None)
def _op_trainer(dim):
    from aclgan_amd import trainer as T
    return T.aclgan_Trainer(_cfg(dim))


@pytest.mark.parametrize("name", list(CASES))
def test_operator_matches_fp64(L, name):
    dim, net, B, H, W, seed, sep, need = CASES[name]
    dcfg, P, x, (p_ref, G_ref, g_ref) = _case(name)
    tr = _op_trainer(dim)
    getattr(tr, net).load_state_dict(P, strict=False)
    pen, gx, grads, buf = _run_op(L, tr, net, x, GAMMA)
    errs = {"P": abs(float(pen) - float(p_ref)) / float(p_ref), "grad_x": rel_err(gx, G_ref)}
    for k, ref in g_ref.items():
        if k.endswith("weight"):
            assert float(ref.abs().max()) > 0
            errs[k] = rel_err(grads[k], ref)
    # everything but the weight tensors of this network is untouched bit for bit: its biases, the other discriminators
    mask = torch.ones_like(buf, dtype=torch.bool)
    for e in getattr(tr, net)._entries:
        if e["key"].endswith("weight"):
            mask[e["offset"]: e["offset"] + e["numel"]] = False
    assert torch.equal(buf[mask], torch.full_like(buf[mask], 1.5))
    for k, g in grads.items():
        if k.endswith("bias"):
            assert torch.equal(g, torch.full_like(g, 1.5)), k
    _check(name, errs)


def test_penalty_scales_with_gamma_and_accumulates(L):
    """gamma 0: P = 0 and nothing is added; a second call without zeroing adds the same gradient again; no grad_x is fine"""
    name = "reduced_64x64_b2"
    dim, net, B, H, W, seed, sep, need = CASES[name]
    dcfg, P, x, (p_ref, G_ref, g_ref) = _case(name)
    tr = _op_trainer(dim)
    getattr(tr, net).load_state_dict(P, strict=False)
    pen0, gx0, grads0, _ = _run_op(L, tr, net, x, 0.0)
    assert float(pen0) == 0.0 and all(float(g.abs().max()) == 0 for k, g in grads0.items() if k.endswith("weight"))
    assert rel_err(gx0, G_ref) <= 1e-4        # G does not depend on gamma
    pen1, _, g1, _ = _run_op(L, tr, net, x, GAMMA, want_gx=False)
    pen2, _, g2, _ = _run_op(L, tr, net, x, GAMMA, want_gx=False, zero=False)
    assert float(pen1) > 0 and abs(float(pen2) - float(pen1)) <= 1e-5 * float(pen1)
    for k in g1:
        if k.endswith("weight"):
            assert rel_err(g2[k], 2 * g1[k]) <= 1e-4, k


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. deterministic mode
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["reduced_64x96_b2", "full_64x64_b2"])
def test_deterministic_mode_repeats_every_bit(L, name):
    dim, net, B, H, W, seed, sep, need = CASES[name]
    dcfg, P, x, ref = _case(name)
    with deterministic_mode(L, True):
        tr = _op_trainer(dim)
        getattr(tr, net).load_state_dict(P, strict=False)
        a = _run_op(L, tr, net, x, GAMMA)
        b = _run_op(L, tr, net, x, GAMMA)
    assert float(a[0]) == float(b[0]) and float(a[0]) > 0
    assert torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])
    assert rel_err(a[1], ref[1]) <= 1e-4


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the trainer: the buffer holds the penalty alone
# ---------------------------------------------------------------------------------------------------------------------------------
TRAINER_SEED = 1      # margins of the fp64 oracle: 1.7e-4 (dis_A on x_a), 1.3e-4 (dis_B on x_b)


def _trainer_batch(B=2, S=64, seed=TRAINER_SEED):
    g = torch.Generator().manual_seed(2000 + seed)
    x_a = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    x_b = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    z = [torch.randn(B, 8, 1, 1, generator=g) for _ in range(6)]
    return x_a, x_b, z


@functools.lru_cache(maxsize=None)
def _trainer_ref():
    cfg = _cfg()
    nets = O.test_nets(cfg, TRAINER_SEED)
    x_a, x_b, z = _trainer_batch()
    out = {}
    for net, x in (("dis_A", x_a), ("dis_B", x_b)):
        margin = r1_closed_form(nets[net], x.double(), cfg["dis"], GAMMA)[3]
        assert margin >= 2e-5, (net, margin)
        out[net] = r1_autograd(nets[net], x.double(), cfg["dis"], GAMMA)
    return out


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_trainer_buffer_holds_the_penalty_alone(T, L, dtype):
    """gan_w = gan_cw = 0 and r1_every 1: the LSGAN seeds are zero, so after dis_update the DIS gradient buffer is the penalty's gradient --
    dis_A on x_a, dis_B on x_b with gamma, dis_2 all zero -- in every compute dtype (the pass is fp32); fp16 carries grad_scale("dis")"""
    cfg = _cfg(gan_w=0.0, gan_cw=0.0, r1_gamma=GAMMA, r1_every=1)
    nets = O.test_nets(cfg, TRAINER_SEED)
    x_a, x_b, z = _trainer_batch()
    ref = _trainer_ref()
    tr = _make(T, cfg, nets, compute_dtype=dtype)
    assert (tr.r1_gamma, tr.r1_every, tr.r1_passes) == (GAMMA, 1, 0) and float(tr.loss_dis_r1_A) == 0 and float(tr.loss_dis_r1_B) == 0
    tr.dis_update(x_a, x_b, cfg, z=z[:3])
    torch.cuda.synchronize()
    assert tr.r1_passes == 1
    scale = tr.grad_scale("dis")
    assert (scale > 1) == (dtype == "fp16")
    errs = {}
    for net, pub in (("dis_A", tr.loss_dis_r1_A), ("dis_B", tr.loss_dis_r1_B)):
        p_ref, _, g_ref = ref[net]
        assert pub.dim() == 0
        errs[net + ".P"] = abs(float(pub) - float(p_ref)) / float(p_ref)
        for k, g in getattr(tr, net).named_grads():
            if k.endswith("weight"):
                errs[net + "." + k] = rel_err(g / scale, g_ref[k])
            else:
                assert float(g.abs().max()) == 0, (net, k)
    assert all(float(g.abs().max()) == 0 for _, g in tr.dis_2.named_grads())
    assert float(tr.loss_dis_total) == 0.0      # the 16 reference losses do not hold the penalty
    _check("trainer_" + dtype, errs)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. schedule
# ---------------------------------------------------------------------------------------------------------------------------------
def test_schedule_and_resume(T, L, tmp_path):
    """r1_every 4: passes at the discriminator updates 1, 5 and 9 only -- r1_passes, and the library's launch counter against a twin without
    the key -- and a trainer resumed after update 6 continues the phase (next pass at update 9)"""
    cfg = _cfg(r1_gamma=GAMMA, r1_every=4)
    off = _cfg()
    nets = O.test_nets(cfg, 0)
    x_a, x_b, z = _trainer_batch(seed=7)
    on_t, off_t = _make(T, cfg, nets), _make(T, off, nets)
    extra, passes = [], []
    for i in range(10):
        d = []
        for tr, c in ((on_t, cfg), (off_t, off)):
            n0 = L.lib.aclgan_launch_count()
            tr.dis_update(x_a, x_b, c, z=z[:3])
            d.append(L.lib.aclgan_launch_count() - n0)
        extra.append(d[0] - d[1]); passes.append(on_t.r1_passes)
        if i == 5:
            on_t.save(str(tmp_path), 5)
    torch.cuda.synchronize()
    assert passes == [1, 1, 1, 1, 2, 2, 2, 2, 3, 3], passes
    assert extra[0] > 0 and extra == [extra[0] if i % 4 == 0 else 0 for i in range(10)], extra
    assert off_t.r1_passes == 0 and off_t._r1_pen is None and off_t._r1_scratch is None
    assert float(on_t.loss_dis_r1_A) > 0 and float(on_t.loss_dis_r1_B) > 0
    res = T.aclgan_Trainer(cfg)
    assert res.resume(str(tmp_path), cfg) == 6 and res._opt[L.GROUP_DIS]["steps"] == 6
    seen = []
    for i in range(4):      # updates 7 .. 10
        res.dis_update(x_a, x_b, cfg, z=z[:3])
        seen.append(res.r1_passes)
    assert seen == [0, 0, 1, 1], seen


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. key off
# ---------------------------------------------------------------------------------------------------------------------------------
def _iterate(L, tr, cfg, batches):
    n0 = L.lib.aclgan_launch_count()
    losses = []
    for x_a, x_b, z in batches:
        tr.dis_update(x_a, x_b, cfg, z=z[:3])
        tr.gen_update(x_a, x_b, cfg, z=z[3:])
        losses.append(tr._losses.clone())
    torch.cuda.synchronize()
    state = {"param%d" % g: tr._param[g].clone() for g in (0, 1)}
    state.update({"m%d" % g: tr._m[g].clone() for g in (0, 1)})
    state.update({"v%d" % g: tr._v[g].clone() for g in (0, 1)})
    state["grad1"] = tr._grad[1].clone()
    return state, torch.stack(losses), L.lib.aclgan_launch_count() - n0


def test_key_off_changes_nothing(T, L):
    """deterministic mode, 3 D+G iterations: r1_gamma 0 (with an r1_every) gives the parameters, Adam state and 16 losses of a trainer built
    without the keys, bit for bit, with the same number of launches and no buffer"""
    plain = _cfg()
    zero = _cfg(r1_gamma=0.0, r1_every=2)
    nets = O.test_nets(plain, 0)
    batches = [_trainer_batch(seed=20 + i) for i in range(3)]
    with deterministic_mode(L, True):
        a, la, na = _iterate(L, _make(T, plain, nets), plain, batches)
        tz = _make(T, zero, nets)
        b, lb, nb = _iterate(L, tz, zero, batches)
    assert na == nb
    assert torch.equal(la, lb)
    assert not [k for k in a if not torch.equal(a[k], b[k])]
    assert tz.r1_passes == 0 and tz._r1_pen is None and tz._r1_scratch is None and float(tz.loss_dis_r1_A) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. hip_graph
# ---------------------------------------------------------------------------------------------------------------------------------
def _l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_graph_replay_runs_the_pass_after_the_update(T, L):
    """r1_every 1, 3 iterations, deterministic mode.  A replayed update has zeroed the buffer itself, so the pass follows it where the
    eager trainer runs the pass first: with the eager trainer's order swapped too (_r1_after) the two agree bit for bit; in their own
    orders they agree within the eager trainer's own spread between the two orders"""
    cfg = _cfg(r1_gamma=GAMMA_BIG, r1_every=1)
    nets = O.test_nets(cfg, 0)
    batches = [_trainer_batch(seed=30 + i) for i in range(3)]

    def run(after, **kw):
        tr = _make(T, cfg, nets, **kw)
        tr._r1_after = after
        out = _iterate(L, tr, cfg, batches)
        return tr, out
    with deterministic_mode(L, True):
        plain, _, _ = _iterate(L, _make(T, _cfg(), nets), _cfg(), batches)
        te, (e, le, _) = run(False)
        ta, (a, la_, _) = run(True)
        tg, (g, lg, _) = run(True, hip_graph=True)
        th, (h, lh, _) = run(False, hip_graph=True)
    assert tg.hip_graph and tg._graphs["dis"]["graph"] is not None and th._graphs["dis"]["graph"] is not None
    assert te.r1_passes == ta.r1_passes == tg.r1_passes == th.r1_passes == 3
    # the same order: the same bits
    assert torch.equal(la_, lg) and not [k for k in a if not torch.equal(a[k], g[k])]
    assert float(tg.loss_dis_r1_A) == float(ta.loss_dis_r1_A) > 0
    # their own orders: within the spread of the order
    spread = max(_l2(a["param1"], e["param1"]), _l2(a["grad1"], e["grad1"]))
    got = max(_l2(h["param1"], e["param1"]), _l2(h["grad1"], e["grad1"]))
    weight = _l2(e["grad1"], plain["grad1"])      # what the penalty moves: far above the bound, or the comparison would show nothing
    print("hip_graph vs eager %.3e; eager order spread %.3e; with vs without the penalty %.3e" % (got, spread, weight))
    assert weight > 0.05
    _record("order_spread", {"eager_before_vs_after": spread, "graph_vs_eager": got, "with_vs_without_penalty": weight})
    assert ORDER_TOL is not None, "no measured bound yet: fill MEASURED_ORDER_SPREAD (this run: %.3e)" % spread
    assert got <= ORDER_TOL and spread <= ORDER_TOL


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. the forced single-rank RCCL path
# ---------------------------------------------------------------------------------------------------------------------------------
def test_data_parallel_world1_matches_the_plain_trainer(T, L):
    """RCCL world size 1 forced (as tests/test_gpu_ddp.py does): the pass runs before the update, the bucket callbacks of the update fire
    after the last writer, and the reduced gradient buffer equals the non-distributed trainer's"""
    import torch.distributed as dist
    cfg = _cfg(gan_w=0.0, gan_cw=0.0, r1_gamma=GAMMA, r1_every=1)      # (the buffer holds the penalty alone, as in test 3)
    nets = O.test_nets(cfg, 0)
    x_a, x_b, z = _trainer_batch(seed=40)

    def run(tr):
        tr.dis_update(x_a, x_b, cfg, z=z[:3])
        torch.cuda.synchronize()
        return tr._grad[1].clone(), tr._losses.clone(), float(tr.loss_dis_r1_A), float(tr.loss_dis_r1_B)
    with deterministic_mode(L, True):
        ref = run(_make(T, cfg, nets))
        pen_off = run(_make(T, _cfg(gan_w=0.0, gan_cw=0.0), nets))
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ["MASTER_PORT"] = str(28600 + os.getpid() % 300)
        os.environ["ACLGAN_BENCH_FORCE_DIST"] = "1"
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        try:
            tr = _make(T, cfg, nets)
            assert tr._reducer is not None
            got = run(tr)
            nbk = (tr._grad[1].numel() + tr._reducer.bucket_elems - 1) // tr._reducer.bucket_elems
            assert sorted(tr._reducer.order) == list(range(nbk))
        finally:
            os.environ.pop("ACLGAN_BENCH_FORCE_DIST", None)
            dist.destroy_process_group()
    assert got[2] == ref[2] > 0 and got[3] == ref[3] > 0
    for a, b in zip(got[:2], ref[:2]):      # (the bound of tests/test_gpu_ddp.py::test_trainer_data_parallel_world1)
        assert (a - b).abs().max().item() <= 2e-5 * max(1e-6, b.abs().max().item())
    # and the penalty is what was reduced: without the key the buffer is all zero
    assert ref[0].abs().max().item() > 0 and pen_off[0].abs().max().item() == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. error paths
# ---------------------------------------------------------------------------------------------------------------------------------
def test_errors_are_refused_before_any_launch(T, L):
    cfg = _cfg()
    tr = T.aclgan_Trainer(cfg)
    x = torch.rand(2, 3, 64, 64, device="cuda")
    pen = torch.zeros(1, device="cuda")
    scratch = torch.empty(L.lib.aclgan_dis_r1_scratch_bytes(tr._ctx, L.NETS["dis_A"], 2, 64, 64), dtype=torch.uint8, device="cuda")
    f = L.lib.aclgan_dis_r1
    torch.cuda.synchronize()
    before = tr._grad[1].clone()
    n0 = L.lib.aclgan_launch_count()
    A, st = L.NETS["dis_A"], L.stream_ptr()
    assert f(tr._ctx, L.NETS["gen_AB"], L.ptr(x), 2, 64, 64, 1.0, L.ptr(pen), None, L.ptr(scratch), st) == -1
    assert f(tr._ctx, A, None, 2, 64, 64, 1.0, L.ptr(pen), None, L.ptr(scratch), st) == -1
    assert f(tr._ctx, A, L.ptr(x), 2, 64, 64, 1.0, None, None, L.ptr(scratch), st) == -1
    assert f(tr._ctx, A, L.ptr(x), 2, 64, 64, 1.0, L.ptr(pen), None, None, st) == -1
    assert f(tr._ctx, A, L.ptr(x), 2, 64, 64, -1.0, L.ptr(pen), None, L.ptr(scratch), st) == -1
    assert f(tr._ctx, A, L.ptr(x), 2, 64, 64, float("nan"), L.ptr(pen), None, L.ptr(scratch), st) == -1
    assert f(tr._ctx, A, L.ptr(x), 2, 16, 16, 1.0, L.ptr(pen), None, L.ptr(scratch), st) == -1 and "too small" in L.last_error()
    sn = T.aclgan_Trainer(_cfg(**{"dis": dict(cfg["dis"], norm="sn")}))
    assert f(sn._ctx, A, L.ptr(x), 2, 64, 64, 1.0, L.ptr(pen), None, L.ptr(scratch), st) == -2
    assert L.lib.aclgan_dis_r1_scratch_bytes(sn._ctx, A, 2, 64, 64) == 0
    assert L.lib.aclgan_launch_count() == n0
    torch.cuda.synchronize()
    assert torch.equal(tr._grad[1], before) and float(pen) == 0
    for bad in ({"dis": dict(cfg["dis"], norm="sn"), "r1_gamma": 1.0}, {"dis_augment": "color", "r1_gamma": 1.0}, {"r1_gamma": -1.0},
                {"r1_gamma": 1.0, "r1_every": 0}):
        with pytest.raises(L.AclganError):
            T.aclgan_Trainer(_cfg(**bad))
    assert L.lib.aclgan_launch_count() == n0
