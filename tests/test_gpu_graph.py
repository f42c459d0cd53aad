"""HIP-graph replay of the update launch sequence (aclgan_Trainer(hip_graph=True), SURVEY section 7 step 7 "static launch
sequence"): the same kernels in the same order, so a graph-replayed run must reproduce the eager run -- bitwise in deterministic
mode, to summation-order accuracy otherwise.  The reference has no counterpart (eager PyTorch)."""
import pytest
import torch

from oracle import aclgan_oracle as O

pytestmark = pytest.mark.gpu


def _run(T, cfg, nets, batches, **kw):
    tr = T.aclgan_Trainer(cfg, **kw)
    for name in O.OracleTrainer.NETS:
        getattr(tr, name).load_state_dict(nets[name], strict=False)
    losses = []
    for x_a, x_b, z in batches:
        tr.dis_update(x_a, x_b, cfg, z=z[:3])
        tr.gen_update(x_a, x_b, cfg, z=z[3:])
        tr.update_learning_rate()
        losses.append((float(tr.loss_dis_total), float(tr.loss_gen_total)))
    torch.cuda.synchronize()
    params = {k: v.detach().clone() for k, v in tr.named_parameters()}
    return tr, losses, params


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_graph_replay_matches_eager(dtype):
    assert torch.cuda.is_available()
    import aclgan_amd  # noqa: F401
    from aclgan_amd import trainer as T, _lib as L
    cfg = O.default_config()
    cfg["display_size"] = 1
    cfg["focus_epsilon"] = 0.5
    nets = O.test_nets(cfg, 0)
    g = torch.Generator().manual_seed(31)
    B, S = 2, 64
    batches = [(torch.rand(B, 3, S, S, generator=g) * 2 - 1, torch.rand(B, 3, S, S, generator=g) * 2 - 1,
                [torch.randn(B, 8, 1, 1, generator=g) for _ in range(6)]) for _ in range(4)]     # step 1 eager, 2 captures, 3-4 replay
    prev = L.lib.aclgan_get_deterministic()
    try:
        te, le, pe = _run(T, cfg, nets, batches, compute_dtype=dtype, deterministic=True)
        tg, lg, pg = _run(T, cfg, nets, batches, compute_dtype=dtype, deterministic=True, hip_graph=True)
    finally:
        L.check(L.lib.aclgan_set_deterministic(prev))
    assert tg.hip_graph, "capture fell back to eager execution"
    assert tg._graphs["gen"]["graph"] is not None and tg._graphs["dis"]["graph"] is not None
    assert le == lg, (le, lg)
    bad = [k for k in pe if not torch.equal(pe[k], pg[k])]
    assert not bad, bad[:6]
    # a different batch size re-captures instead of replaying a stale graph
    x_a, x_b, z = batches[0]
    tg.dis_update(x_a[:1], x_b[:1], cfg, z=[t[:1] for t in z[:3]])
    assert torch.isfinite(tg.loss_dis_total).item()


def test_graph_replay_flat_buffers_reduced_width_repeated_batch():
    """default keys, gen / dis dim 8, the SAME batch every step, deterministic: the flat gradient, parameter and Adam buffers of both groups
    (alignment floats included) and the 16 losses equal the eager trainer's bit for bit after every update of four iterations -- two of
    them replays.  From its second replay on a captured hipMemsetAsync (the update's zero-fill of the gradient buffer, the first node of
    the graph) used to fill the buffer with a non-zero 8-byte pattern; named_parameters() above is too coarse a view to pin that down to
    its first update, and the alignment floats behind the 1-float head biases, which nothing but the zero-fill writes, show it alone"""
    assert torch.cuda.is_available()
    import aclgan_amd  # noqa: F401
    from aclgan_amd import trainer as T, _lib as L
    cfg = O.default_config()
    cfg["gen"].update(dim=8, mlp_dim=16, n_res=2); cfg["dis"].update(dim=8)
    cfg["display_size"] = 1
    cfg["focus_epsilon"] = 0.5
    nets = O.test_nets(cfg, 4)
    g = torch.Generator().manual_seed(33)
    B, S = 2, 64
    x_a, x_b = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).cuda(), (torch.rand(B, 3, S, S, generator=g) * 2 - 1).cuda()
    z = [torch.randn(B, 8, 1, 1, generator=g) for _ in range(6)]

    def make(**kw):
        tr = T.aclgan_Trainer(cfg, deterministic=True, **kw)
        for name in O.OracleTrainer.NETS:
            getattr(tr, name).load_state_dict(nets[name], strict=False)
        return tr

    def bits(t):
        return t.view(torch.int32)
    prev = L.lib.aclgan_get_deterministic()
    try:
        te, tg = make(), make(hip_graph=True)
        start = te._param[1].clone()
        for it in range(4):
            for which in ("dis", "gen"):
                for tr in (te, tg):
                    if which == "dis":
                        tr.dis_update(x_a, x_b, cfg, z=z[:3])
                    else:
                        tr.gen_update(x_a, x_b, cfg, z=z[3:])
                torch.cuda.synchronize()
                bad = ["%s[%d]" % (nm, grp) for grp in (0, 1) for nm in ("_grad", "_param", "_m", "_v")
                       if not torch.equal(bits(getattr(te, nm)[grp]), bits(getattr(tg, nm)[grp]))]
                if not torch.equal(bits(te._losses), bits(tg._losses)):
                    bad.append("_losses")
                assert not bad, ("iteration %d, %s_update" % (it + 1, which), bad)
    finally:
        L.check(L.lib.aclgan_set_deterministic(prev))
    assert tg.hip_graph, "capture fell back to eager execution"
    assert tg._graphs["gen"]["graph"] is not None and tg._graphs["dis"]["graph"] is not None
    assert not torch.equal(te._param[1], start)      # the run moved the parameters


def test_graph_replay_matches_eager_sn():
    """dis.norm sn (one pass per discriminator call, the fold as the last writer of the weight_bar gradients): graph replay == eager
    bit for bit in deterministic mode over the 4 steps -- losses, every parameter and the power-iteration state u / v"""
    assert torch.cuda.is_available()
    import aclgan_amd  # noqa: F401
    from aclgan_amd import trainer as T, _lib as L
    from sn_nets import sn_test_nets
    cfg = O.default_config()
    cfg["gen"].update(dim=16, mlp_dim=32, n_res=2); cfg["dis"].update(dim=16, norm="sn")
    cfg["display_size"] = 1
    cfg["focus_epsilon"] = 0.5
    nets = sn_test_nets(cfg, 0)
    g = torch.Generator().manual_seed(32)
    B, S = 2, 64
    batches = [(torch.rand(B, 3, S, S, generator=g) * 2 - 1, torch.rand(B, 3, S, S, generator=g) * 2 - 1,
                [torch.randn(B, 8, 1, 1, generator=g) for _ in range(6)]) for _ in range(4)]
    prev = L.lib.aclgan_get_deterministic()
    try:
        te, le, pe = _run(T, cfg, nets, batches, deterministic=True)
        tg, lg, pg = _run(T, cfg, nets, batches, deterministic=True, hip_graph=True)
    finally:
        L.check(L.lib.aclgan_set_deterministic(prev))
    assert tg.hip_graph, "capture fell back to eager execution"
    assert tg._graphs["gen"]["graph"] is not None and tg._graphs["dis"]["graph"] is not None
    assert le == lg, (le, lg)
    bad = [k for k in pe if not torch.equal(pe[k], pg[k])]
    assert not bad, bad[:6]
    assert torch.equal(te._sn_state, tg._sn_state)
    # u / v moved: 4 steps = 4 x (dis_update + gen_update) calls of every discriminator
    assert not torch.equal(te.dis_A.state_dict()["cnns.0.1.conv.module.weight_u"].cpu(), nets["dis_A"]["cnns.0.1.conv.module.weight_u"])
