"""The optimizer model the GPU tests check aclgan_adam_step against (oracle/optimizer_oracle.py) is itself checked here, without a GPU:
the fp64 Adam against torch.optim.Adam in fp64, the loss-scale state model against a transition table written by hand from the
contract in include/aclgan_hip.h (aclgan_bind_loss_scale)."""
import torch

from oracle import aclgan_oracle as O
from oracle import optimizer_oracle as M


def _inputs(n, steps, seed):
    g = torch.Generator().manual_seed(seed)
    p0 = (torch.rand(n, generator=g, dtype=torch.float64) * 4 - 3).exp().mul(torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0))
    mag = 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 10 - 8)
    grads = [mag * (torch.rand(n, generator=g, dtype=torch.float64) * 2 - 1) for _ in range(steps)]
    return p0, grads


def test_fp64_adam_equals_torch_adam_in_fp64_over_40_steps_with_weight_decay_and_an_lr_change():
    n, T = 4099, 40
    p0, grads = _inputs(n, T, 11)
    b1, b2, eps, wd = 0.5, 0.999, 1e-8, 1e-4
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=1e-4, betas=(b1, b2), eps=eps, weight_decay=wd)
    mine = M.Adam64(p0, b1, b2, eps, wd)
    for t in range(1, T + 1):
        lr = O.step_lr(1e-4, 0.5, 25, t - 1)          # StepLR: halves after 25 scheduler calls
        assert lr == (1e-4 if t <= 25 else 5e-5)
        opt.param_groups[0]["lr"] = lr
        ref.grad = grads[t - 1].clone()
        opt.step()
        mine.step(grads[t - 1], lr, t=t)
    st = opt.state[ref]
    assert int(float(st["step"])) == T and mine.applied == T
    rel_p = ((mine.p - ref.detach()).abs() / ref.detach().abs()).max().item()
    rel_v = ((mine.v - st["exp_avg_sq"]).abs() / st["exp_avg_sq"]).max().item()
    err_m = ((mine.m - st["exp_avg"]).abs() / mine.gvmax).max().item()      # m cancels: normalised by what went into it
    print("fp64 model vs torch.optim.Adam fp64: p %.2e, v %.2e (relative), m %.2e (of the largest effective gradient)" % (rel_p, rel_v, err_m))
    assert rel_p <= 1e-12 and rel_v <= 1e-12 and err_m <= 1e-12, (rel_p, rel_v, err_m)
    assert (mine.p - p0).abs().max().item() > 1e-4                      # the parameters did move


def test_explicit_bias_correction_step_is_what_separates_a_skipped_update():
    """the first applied update moves a parameter by lr with step 1, by 0.9426 lr with step 2 and 0.9892 lr with step 3 (beta 0.5 / 0.999,
    no decay, |g| >> eps): the figures the GPU tests rely on to tell the two apart"""
    g = torch.full((4,), 0.25, dtype=torch.float64)
    for t, want in ((1, 1.0), (2, 0.9426), (3, 0.9892)):
        a = M.Adam64(torch.ones(4, dtype=torch.float64), 0.5, 0.999, 1e-8, 0.0)
        a.step(g, 1e-4, t=t)
        moved = ((1.0 - a.p) / 1e-4).max().item()
        assert abs(moved - want) < 1e-4, (t, moved)


def test_torch_fp32_adam_wrapper_follows_the_fp64_model():
    p0, grads = _inputs(1000, 5, 12)
    p0 = p0.float()
    b1, b2, eps, wd = 0.5, M.f32(0.999), M.f32(1e-8), M.f32(1e-4)
    a64 = M.Adam64(p0, b1, b2, eps, wd)
    a32 = M.TorchAdam32(p0, b1, b2, eps, wd)
    for t in range(5):
        g = grads[t].float()
        a64.step(g, M.f32(1e-4)); a32.step(g, M.f32(1e-4))
    e = M.parity_metrics(a32.p, a32.m, a32.v, a64, M.f32(1e-4), 5)
    print("torch fp32 vs fp64 after 5 steps:", e)
    assert set(e) == set(M.METRICS)
    assert 0 < e["p"] < 10 and 0 < e["v"] < 1e-5 and 0 < e["m"] and 0 < e["m_eff"] < 1e-5, e
    # the metrics see a wrong bias-correction step at once
    bad = M.Adam64(p0, b1, b2, eps, wd)
    bad.step(grads[0].float(), M.f32(1e-4), t=2)
    good = M.Adam64(p0, b1, b2, eps, wd)
    good.step(grads[0].float(), M.f32(1e-4), t=1)
    # (5.7 % of lr against lr * 1e-6 + 2^-23 |p| with |p| >= e^-3: about 950, where fp32 arithmetic costs a few units)
    assert M.parity_metrics(bad.p, bad.m, bad.v, good, M.f32(1e-4), 1)["p"] > 100 * e["p"]


# (group, grads non-finite) -> the eight floats afterwards, written out by hand from the header:
# [0] S  [1] 1/S  [2] clean updates  [3] flag  [4],[5] skipped gen, dis  [6] interval  [7] S of the update just made
TABLE_INTERVAL_3 = [
    # start: S = 8, interval 3
    ((0, False), [8.0, 1 / 8, 1, 0, 0, 0, 3, 8.0]),
    ((1, False), [8.0, 1 / 8, 2, 0, 0, 0, 3, 8.0]),        # the clean counter is shared by the groups ...
    ((0, False), [16.0, 1 / 16, 0, 0, 0, 0, 3, 8.0]),      # ... third clean update: doubles, counter restarts, [7] keeps the OLD scale
    ((1, True), [8.0, 1 / 8, 0, 0, 0, 1, 3, 16.0]),        # overflow in dis: halves, only dis's skip counter moves
    ((1, False), [8.0, 1 / 8, 1, 0, 0, 1, 3, 8.0]),
    ((0, True), [4.0, 1 / 4, 0, 0, 1, 1, 3, 8.0]),         # overflow in gen: clean counter back to 0, gen's own counter
    ((0, True), [2.0, 1 / 2, 0, 0, 2, 1, 3, 4.0]),
    ((1, True), [1.0, 1.0, 0, 0, 2, 2, 3, 2.0]),
    ((1, True), [1.0, 1.0, 0, 0, 2, 3, 3, 1.0]),           # the floor: 2 -> 1 -> 1, the skip still counts
    ((0, False), [1.0, 1.0, 1, 0, 2, 3, 3, 1.0]),
    ((0, False), [1.0, 1.0, 2, 0, 2, 3, 3, 1.0]),
    ((1, False), [2.0, 0.5, 0, 0, 2, 3, 3, 1.0]),
]


def _run_table(model, table):
    for i, ((grp, bad), want) in enumerate(table):
        applied = model.adam_step(grp, bad)
        assert applied == (not bad)
        assert model.state == [float(x) for x in want], (i, model.state, want)


def test_loss_scale_model_reproduces_the_hand_written_transition_table():
    m = M.LossScaleModel(8.0, interval=3)
    assert m.state == [8.0, 0.125, 0, 0, 0, 0, 3.0, 0]
    _run_table(m, TABLE_INTERVAL_3)
    # bias-correction step = host step - that group's skips: gen made 6 calls, 2 skipped; dis 6 calls, 3 skipped
    assert m.bias_correction_step(0, 6) == 4 and m.bias_correction_step(1, 6) == 3


def test_loss_scale_model_cap_and_default_interval():
    m = M.LossScaleModel(2.0 ** 23, interval=1)
    _run_table(m, [((0, False), [2.0 ** 24, 2.0 ** -24, 0, 0, 0, 0, 1, 2.0 ** 23]),
                   ((1, False), [2.0 ** 24, 2.0 ** -24, 0, 0, 0, 0, 1, 2.0 ** 24]),      # the cap: 2^23 -> 2^24 -> 2^24
                   ((1, True), [2.0 ** 23, 2.0 ** -23, 0, 0, 0, 1, 1, 2.0 ** 24])])
    # interval 0 means 2000: 1998 clean updates do nothing, the 2000th doubles
    m = M.LossScaleModel(65536.0, interval=0, clean=1998)
    _run_table(m, [((0, False), [65536.0, 2.0 ** -16, 1999, 0, 0, 0, 0, 65536.0]),
                   ((1, False), [131072.0, 2.0 ** -17, 0, 0, 0, 0, 0, 65536.0]),
                   ((0, False), [131072.0, 2.0 ** -17, 1, 0, 0, 0, 0, 131072.0])])
    # 1 / S is the fp32 quotient for a scale that is not a power of two
    m = M.LossScaleModel(3.0, interval=5)
    m.adam_step(0, False)
    assert m.state[1] == M.f32(1.0 / 3.0) and m.state[1] != 1.0 / 3.0
