"""BASELINE.json configs[2] (bf16) and configs[4] (fp16 + loss scaling): the training step with the heavy convolutions
on the 16-bit matrix cores.

The reference is fp32-only, so there is no reference behaviour to match bit for bit.  Two checks, same weights / inputs / z:

  (1) against the EMULATED CONTRACT: oracle/aclgan_oracle.py::compute_dtype restates, on the CPU, exactly what the 16-bit
      path promises (both GEMM operands of every eligible convolution rounded to the 16-bit type, fp32 accumulation,
      merged phase filters rounded in the sub-pixel layers, gradients rounded at the loss scale they carry, everything
      else fp32).  Two implementations of the SAME contract still drift apart: a pre-rounding difference of 1e-7 (fp32
      summation order) flips the 16-bit rounding of a few values, each flip is a 2^-9 (2^-12) relative kick, and after a
      handful of layers every value carries quantisation-level noise -- so deep tensors agree with the emulation only
      ~1.5x better than with the fp32 oracle, while shallow ones (style code s_2: five convolutions) agree ~30x better:
      s_2 <= 5e-4 / 1e-4 is the sharp step-level check; kernel-level exactness is tests/test_gpu_ops16.py (2e-4).
  (2) against the fp32 ORACLE: the stated precision of the reduced-precision configs,

                              forward tensors   losses (adv, idt, totals | focus digit | focus size)   gradients (per-tensor
        bf16  (8-bit mantissa)     6e-2          1e-3 | 1.5e-2 | 6e-2                                   relative L2, smooth
        fp16  (11-bit mantissa)    8e-3          1e-4 | 6e-4   | 1.5e-2                                 fixture)  3e-1 / 1.2e-1

      The gradient figures are a property of the contract, not of the kernels: the CPU emulation sits at the same
      distance from the fp32 oracle (0.226 for bf16 on the worst tensor, gen_AB enc_content.model.1.conv.weight --
      ReLU masks of ~25 stacked layers flip when activations move by 2^-9).

fp16 runs under dynamic loss scaling: gradient buffers carry S*g, Adam divides by S on the device, an overflowing
update is skipped and halves S -- both behaviours are tested.
"""
import os

import numpy as np
import pytest
import torch

from oracle import aclgan_oracle as O

pytestmark = pytest.mark.gpu

FTOL = {"bf16": 6e-2, "fp16": 8e-3}
LTOL = {"bf16": 1e-3, "fp16": 1e-4}         # adversarial / identity / total losses (measured worst 2.1e-4 / 1.5e-5)
LTOL_DIGIT = {"bf16": 1.5e-2, "fp16": 1.2e-3}   # sum 1/(|m-.5|+0.01): ill-conditioned in the mask values (measured over the round-3 builds: up to 8.5e-3 / 6.3e-4)
LTOL_SIZE = {"bf16": 1e-1, "fp16": 1.5e-2}    # relu(sum(m - upper))^2 near its threshold: a difference of two large sums, squared (measured over the round-3 builds: up to 4.8e-2 / 8.1e-3)
GTOL = {"bf16": 3e-1, "fp16": 1.2e-1}
# vs the emulated contract.  The deepest tensor (x_A2_fake: encode -> decode -> encode -> decode, ~60 roundings deep) is chaotic in the
# LAST BIT of anything upstream: between two builds of this round that differ only in the association order of the epilogue statistics it
# measured 3.9e-2 .. 5.6e-2 (bf16) and 4.9e-3 .. 6.4e-3 (fp16); the shallow tensors (c_1 8e-3, s_2 below, discriminator outputs 4e-3) are stable
ETOL_F = {"bf16": 8e-2, "fp16": 1e-2}
ETOL_S2 = {"bf16": 5e-4, "fp16": 2e-4}     # the shallow tensor s_2 vs the emulated contract (measured 1.3e-4 / 1.05e-4 with 16-bit storage: the pool averages rounded values)
ETOL_G = {"bf16": 2.5e-1, "fp16": 1e-1}    # measured worst 2.08e-1 / 7.75e-2 with 16-bit activation / gradient storage (stable to 3 digits over five builds)
SCALE = {"bf16": 1.0, "fp16": 65536.0}


@pytest.fixture(scope="module")
def T():
    assert torch.cuda.is_available()
    import aclgan_amd  # noqa: F401
    from aclgan_amd import trainer
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    return trainer


def _make(T, cfg, nets, dt):
    tr = T.aclgan_Trainer(cfg, compute_dtype=dt)
    for name in O.OracleTrainer.NETS:
        getattr(tr, name).load_state_dict(nets[name], strict=False)
    return tr


def _rel(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _dist(a, b):
    """(p99, mean) of |a - b| / max |b|: the distribution beside _rel's maximum -- a subtly wrong 16-bit kernel shifts the bulk of the
    elements, which one outlier pixel's max-abs bound cannot show"""
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    e = ((a - b).abs() / b.abs().max().clamp_min(1e-30)).flatten()
    return torch.quantile(e.float(), 0.99).item(), e.mean().item()


# x_A2_fake against the fp32 oracle: (p99, mean) of |got - ref| / max |ref|, bounds = 2x the value measured on the MI355X.  Keys: (dtype, image
# size) for test_forward_and_losses_16bit (B = 2), (dtype, batch) for test_16bit_at_its_per_gpu_batch (256x256).  Measured:
#   bf16  64x64 2.28e-2 / 5.58e-3,  256x256 2.42e-2 / 6.50e-3,  B=8  2.73e-2 / 7.28e-3
#   fp16  64x64 2.81e-3 / 7.00e-4,  256x256 3.06e-3 / 8.21e-4,  B=32 2.59e-3 / 6.94e-4
X2_DIST = {("bf16", 64): (4.6e-2, 1.12e-2), ("bf16", 256): (4.9e-2, 1.3e-2), ("bf16", 8): (5.5e-2, 1.5e-2),
           ("fp16", 64): (5.7e-3, 1.4e-3), ("fp16", 256): (6.2e-3, 1.65e-3), ("fp16", 32): (5.2e-3, 1.4e-3)}


def _inputs(B, S, seed):
    g = torch.Generator().manual_seed(seed)
    x_a = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    x_b = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    z = [torch.randn(B, 8, 1, 1, generator=g) for _ in range(6)]
    return x_a, x_b, z


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("B,S", [(2, 64), (2, 256)])
def test_forward_and_losses_16bit(T, dt, B, S):
    cfg = O.default_config()
    cfg["display_size"] = 1
    nets = O.test_nets(cfg, 0)
    x_a, x_b, z = _inputs(B, S, 21)
    tr = _make(T, cfg, nets, dt)
    with torch.no_grad():
        _, Lg, fw = O.gen_losses(nets, x_a, x_b, z[3:], cfg)
        _, Ld, _ = O.dis_losses(nets, x_a, x_b, z[:3], cfg)
        dA = O.dis_forward(nets["dis_A"], fw["x_A_fake"], cfg["dis"])
        with O.compute_dtype(dt):
            _, _, fe = O.gen_losses(nets, x_a, x_b, z[3:], cfg)
            dAe = O.dis_forward(nets["dis_A"], fe["x_A_fake"], cfg["dis"])
    xa = x_a.cuda()
    zz = [t.cuda() for t in z[3:]]
    worst, worst_e = {}, {}

    def chk(name, got, key=None):
        worst[name] = _rel(got, fw[key or name]); worst_e[name] = _rel(got, fe[key or name])

    c1, _ = tr.gen_AB.encode(xa); chk("c_1", c1)
    c2, s2 = tr.gen_BA.encode(xa); chk("c_2", c2); chk("s_2", s2)
    xB4 = tr.gen_AB.decode(c1, zz[0])
    xB = tr.focus_translation(xB4[:, :3], xa, xB4[:, 3:]); chk("x_B_fake", xB)
    chk("f_B", xB4[:, 3:])
    rec = tr.gen_BA.decode(c2, s2); chk("x_A_recon", rec[:, :3])
    c3, _ = tr.gen_BA.encode(xB); chk("c_3", c3)
    xA24 = tr.gen_BA.decode(c3, zz[2])
    xA2 = tr.focus_translation(xA24[:, :3], xB, xA24[:, 3:]); chk("x_A2_fake", xA2)
    xA4 = tr.gen_BA.decode(c2, cfg["alpha"] * zz[1])
    xA = tr.focus_translation(xA4[:, :3], xa, xA4[:, 3:])
    for s, (g_, w_, e_) in enumerate(zip(tr.dis_A(xA), dA, dAe)):
        worst["dis_A_xA_s%d" % s] = _rel(g_, w_); worst_e["dis_A_xA_s%d" % s] = _rel(g_, e_)
    print("%s forward max-abs rel errors vs fp32 oracle @%dx%d B=%d:" % (dt, S, S, B), {k: "%.2e" % v for k, v in worst.items()})
    print("%s forward max-abs rel errors vs emulated contract:" % dt, {k: "%.2e" % v for k, v in worst_e.items()})
    # x_A2_fake is two encode -> decode round trips deep (~60 roundings): like the B=8 test below it gets the emulated-contract bound against the
    # fp32 oracle too.  Its MAX-abs error over 2 x 3 x 256 x 256 values moves with the summation order of the fp32 statistics upstream: 5.5e-2
    # (rounds 5-6) -> 6.0e-2 when the LayerNorm partials started to be combined in 64 slices (round 6), 4.7e-2 against the emulated contract.
    bad = {k: v for k, v in worst.items() if not v < (max(FTOL[dt], ETOL_F[dt]) if k == "x_A2_fake" else FTOL[dt])}
    assert not bad, bad
    p99, mean = _dist(xA2, fw["x_A2_fake"])
    print("%s x_A2_fake @%dx%d B=%d vs the fp32 oracle: p99 %.3e, mean %.3e (relative absolute error)" % (dt, S, S, B, p99, mean))
    assert p99 <= X2_DIST[(dt, S)][0] and mean <= X2_DIST[(dt, S)][1], (p99, mean, X2_DIST[(dt, S)])
    bad = {k: v for k, v in worst_e.items() if not v < ETOL_F[dt]}
    assert not bad, ("emulated", bad)
    assert worst_e["s_2"] < ETOL_S2[dt], ("emulated s_2", worst_e["s_2"])
    tr.dis_update(x_a, x_b, cfg, z=z[:3])
    ld = {n: float(getattr(tr, n)) for n in Ld}
    tr2 = _make(T, cfg, nets, dt)
    tr2.gen_update(x_a, x_b, cfg, z=z[3:])
    lg = {n: float(getattr(tr2, n)) for n in Lg}
    errs = {}
    for n, v in list(Ld.items()) + list(Lg.items()):
        v = float(v)
        got = ld[n] if n in ld else lg[n]
        tol = LTOL_SIZE[dt] if "_size" in n else (LTOL_DIGIT[dt] if "_digit" in n else LTOL[dt])
        errs[n] = (abs(got - v) / max(1e-3, abs(v)), tol, got, v)
    print("%s loss rel errors:" % dt, {k: "%.2e" % e[0] for k, e in errs.items()})
    bad = {k: e for k, e in errs.items() if not e[0] <= e[1]}
    assert not bad, bad


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_step_gradients_16bit(T, dt):
    cfg = O.default_config()
    cfg["display_size"] = 1
    cfg["focus_epsilon"] = 0.5      # smooth fixture
    nets = O.test_nets(cfg, 0)
    x_a, x_b, z = _inputs(2, 128, 22)
    trd = _make(T, cfg, nets, dt); sd = trd.grad_scale(); trd.dis_update(x_a, x_b, cfg, z=z[:3])
    trg = _make(T, cfg, nets, dt); sg = trg.grad_scale(); trg.gen_update(x_a, x_b, cfg, z=z[3:])
    assert (sd == 65536.0 and sg == 65536.0) if dt == "fp16" else (sd == 1.0 and sg == 1.0)
    od = O.OracleTrainer(cfg, nets=nets); od.dis_update(x_a, x_b, z[:3], apply=False)
    og = O.OracleTrainer(cfg, nets=nets); og.gen_update(x_a, x_b, z[3:], apply=False)
    with O.compute_dtype(dt, loss_scale=SCALE[dt]):
        ed = O.OracleTrainer(cfg, nets=nets); ed.dis_update(x_a, x_b, z[:3], apply=False)
        eg = O.OracleTrainer(cfg, nets=nets); eg.gen_update(x_a, x_b, z[3:], apply=False)
    worst, worst_e = [], []
    for tr, orc, emu, nets_, S in ((trd, od, ed, ("dis_A", "dis_B", "dis_2"), sd), (trg, og, eg, ("gen_AB", "gen_BA"), sg)):
        gmax = max(float(t.grad.norm()) for n in nets_ for t in orc.nets[n].values())
        for n in nets_:
            for k, gr in getattr(tr, n).named_grads():
                got = gr.cpu().double() / S
                for lst, ref in ((worst, orc.nets[n][k].grad.double()), (worst_e, emu.nets[n][k].grad.double())):
                    lst.append(((got - ref).norm().item() / (ref.norm().item() + 1e-4 * gmax), n, k))
    worst.sort(reverse=True); worst_e.sort(reverse=True)
    print("%s worst gradient tensors vs fp32 oracle (relative L2):" % dt, [("%.2e" % e, n, k) for e, n, k in worst[:6]])
    print("%s worst gradient tensors vs emulated contract:" % dt, [("%.2e" % e, n, k) for e, n, k in worst_e[:6]])
    assert worst[0][0] <= GTOL[dt], worst[:6]
    assert worst_e[0][0] <= ETOL_G[dt], ("emulated", worst_e[:6])
    if dt == "fp16":
        st = trg.loss_scale_state()
        assert st["skipped_gen"] == 0 and st["clean_updates"] == 1 and st["scale"] == 65536.0
    # the optimizer step itself: parameters move like the fp32 oracle's Adam step (first step = lr * sign(g) elementwise,
    # so compare the well-determined part: elements whose |g| is not tiny)
    og2 = O.OracleTrainer(cfg, nets=nets); og2.gen_update(x_a, x_b, z[3:], apply=True)
    k = "dec.model.0.model.0.model.0.conv.weight"
    p_new = dict(trg.gen_AB.named_parameters())[k].cpu()
    ref_new = og2.nets["gen_AB"][k].detach()
    g = og.nets["gen_AB"][k].grad
    mask = g.abs() > g.abs().mean()
    agree = ((p_new - nets["gen_AB"][k]).sign() == (ref_new - nets["gen_AB"][k]).sign())[mask].float().mean().item()
    assert agree > 0.97, agree
    assert (p_new - nets["gen_AB"][k]).abs().max().item() <= 1.01 * cfg["lr"]


def test_fp16_overflow_skips_the_update_and_halves_the_scale(T):
    cfg = O.default_config()
    cfg["gen"].update(dim=32, mlp_dim=32, n_res=1)
    cfg["dis"].update(dim=32)
    cfg["display_size"] = 1
    cfg["loss_scale_init"] = 2.0 ** 40          # every conv gradient overflows fp16 -> inf / nan in the weight gradients
    nets = O.test_nets(cfg, 2)
    x_a, x_b, z = _inputs(1, 64, 23)
    tr = _make(T, cfg, nets, "fp16")
    p0 = tr._param[1].clone(); m0 = tr._m[1].clone()
    tr.dis_update(x_a, x_b, cfg, z=z[:3])
    torch.cuda.synchronize()
    st = tr.loss_scale_state()
    assert st["skipped_dis"] == 1 and st["scale"] == 2.0 ** 39 and st["clean_updates"] == 0
    assert torch.equal(tr._param[1], p0) and torch.equal(tr._m[1], m0)      # no update, no moment pollution
    assert np.isfinite(float(tr.loss_dis_total))                            # the reported losses are unscaled and finite
    # bring the scale down and check a normal update goes through with bias-correction step 1 (the skip is not counted)
    tr._lscale[0] = 1024.0; tr._lscale[1] = 1.0 / 1024.0
    tr.dis_update(x_a, x_b, cfg, z=z[:3])
    st = tr.loss_scale_state()
    assert st["skipped_dis"] == 1 and st["clean_updates"] == 1 and st["scale"] == 1024.0
    d = (tr._param[1] - p0).abs().max().item()
    assert 0 < d <= 1.01 * cfg["lr"]            # |first Adam step| <= lr holds only if bias correction used step = 1
    # ... which the line above cannot tell: with betas (0.5, 0.999) a first applied update computed with step 2 moves a parameter by
    # 0.9426 lr (step 3: 0.9892 lr), inside that bound.  The discriminating checks: some parameter moves by (nearly) the full lr, and
    # p, m, v equal the fp64 model (oracle/optimizer_oracle.py) run with bias-correction step 1 on the gradients the buffer holds,
    # within twice the error torch's own fp32 Adam has on the same inputs (the bound of tests/test_gpu_optimizer.py).
    assert d >= 0.97 * cfg["lr"], d
    from oracle import optimizer_oracle as M
    S = tr.grad_scale("dis")
    assert S == 1024.0
    g = (tr._grad[1] / S).cpu()
    o = tr._opt[1]
    hyper = [M.f32(o[k]) for k in ("beta1", "beta2", "eps", "weight_decay")]
    lr = M.f32(cfg["lr"])
    a64 = M.Adam64(p0.cpu(), *hyper); a64.step(g, lr, t=1)
    t32 = M.TorchAdam32(p0.cpu(), *hyper); t32.step(g, lr)
    e_ref = M.parity_metrics(t32.p, t32.m, t32.v, a64, lr, 1)
    e_hip = M.parity_metrics(tr._param[1].cpu(), tr._m[1].cpu(), tr._v[1].cpu(), a64, lr, 1)
    print("first applied update after the skip vs the fp64 model with step 1: HIP", e_hip, "torch fp32", e_ref)
    bad = {k: (e_hip[k], e_ref[k]) for k in M.METRICS if not e_hip[k] <= 2 * e_ref[k]}
    assert not bad, bad


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_full_size_step_properties_16bit(T, dt):
    """configs[2] / [4] per-GPU shape (256x256, B=8, full width): losses finite and close to the fp32 build's, the two
    optimizers stay separate, Adam's first step moves every parameter by at most lr."""
    cfg = O.default_config()
    cfg["display_size"] = 1
    torch.manual_seed(3)
    tr = T.aclgan_Trainer(cfg, compute_dtype=dt)
    torch.manual_seed(3)
    tr32 = T.aclgan_Trainer(cfg)
    assert torch.equal(tr._param[0], tr32._param[0])
    x_a, x_b, z = _inputs(8, 256, 24)
    gen0 = tr._param[0].clone(); dis0 = tr._param[1].clone()
    tr.gen_update(x_a, x_b, cfg, z=z[3:]); tr32.gen_update(x_a, x_b, cfg, z=z[3:])
    torch.cuda.synchronize()
    for n in ["loss_gen_adv_A", "loss_gen_adv_B", "loss_gen_adv_2", "loss_idt_A", "loss_idt_B"]:
        a, b = float(getattr(tr, n)), float(getattr(tr32, n))
        assert np.isfinite(a) and abs(a - b) <= 10 * LTOL[dt] * max(1e-3, abs(b)), (n, a, b)
    assert torch.equal(tr._param[1], dis0)
    d = (tr._param[0] - gen0).abs().max().item()
    assert 0 < d <= 1.01 * cfg["lr"]
    gen1 = tr._param[0].clone()
    tr.dis_update(x_a, x_b, cfg, z=z[:3])
    torch.cuda.synchronize()
    assert torch.equal(tr._param[0], gen1)
    assert 0 < (tr._param[1] - dis0).abs().max().item() <= 1.01 * cfg["lr"]
    assert np.isfinite(float(tr.loss_dis_total))


@pytest.mark.parametrize("dt,B,NS", [("fp16", 32, 4), ("bf16", 8, 2)], ids=["fp16_b32", "bf16_b8"])
def test_16bit_at_its_per_gpu_batch(T, dt, B, NS):
    """BASELINE configs[4] / configs[2] at their real per-GPU workloads (round 5: bf16 B = 64 / 8 GPUs = 8 as well -- until now the bf16 build
    at this shape was only compared with the repo's own fp32 build).
    fp16 MFMA + dynamic loss scaling, 256x256, B = 256 / 8 GPUs = 32
    (different split-K plans and a ~4x arena compared with the B=8 test above).
      * forward parity against the fp32 ORACLE on a 4-sample subset: every normalisation on the path is per sample, so samples
        0..3 of the B=32 HIP forward must match the oracle run on those four samples alone, within the fp16 bounds stated above;
      * the step's own fused loss kernels at B=32 against a recomputation from the B=32 public-API forward (L1 identity loss,
        the LSGAN generator terms): 1e-4;
      * losses finite, loss scale untouched (no overflow at B=32), the two optimizers stay separate, |first Adam step| <= lr."""
    cfg = O.default_config()
    cfg["display_size"] = 1
    nets = O.test_nets(cfg, 0)
    S = 256
    x_a, x_b, z = _inputs(B, S, 25)
    tr = _make(T, cfg, nets, dt)
    xa = x_a.cuda()
    zz = [t.cuda() for t in z[3:]]
    # ---- HIP forward at B=32 through the public surface ----
    c1, _ = tr.gen_AB.encode(xa)
    c2, s2 = tr.gen_BA.encode(xa)
    xB4 = tr.gen_AB.decode(c1, zz[0])
    xB = tr.focus_translation(xB4[:, :3], xa, xB4[:, 3:])
    xA4 = tr.gen_BA.decode(c2, cfg["alpha"] * zz[1])
    xA = tr.focus_translation(xA4[:, :3], xa, xA4[:, 3:])
    rec = tr.gen_BA.decode(c2, s2)
    c3, _ = tr.gen_BA.encode(xB)
    xA24 = tr.gen_BA.decode(c3, zz[2])
    xA2 = tr.focus_translation(xA24[:, :3], xB, xA24[:, 3:])
    dB = tr.dis_B(xB)
    dA = tr.dis_A(torch.cat((xA, xA2)))
    d2 = tr.dis_2(torch.cat((torch.cat((xa, xA), 1), torch.cat((xa, xA2), 1))))
    # ---- fp32 oracle on samples 0..3 ----
    with torch.no_grad():
        _, _, fw = O.gen_losses(nets, x_a[:NS], x_b[:NS], [t[:NS] for t in z[3:]], cfg)
        dAo = O.dis_forward(nets["dis_A"], fw["x_A_fake"], cfg["dis"])
    worst = {}
    for name, got in (("c_1", c1), ("c_2", c2), ("s_2", s2), ("x_B_fake", xB), ("x_A_fake", xA), ("x_A_recon", rec[:, :3]), ("c_3", c3),
                      ("x_A2_fake", xA2), ("f_B", xB4[:, 3:])):
        worst[name] = _rel(got[:NS], fw[name])
    for s_, (g_, w_) in enumerate(zip(dA, dAo)):
        worst["dis_A_xA_s%d" % s_] = _rel(g_[:NS], w_)
    print("%s B=%d forward max-abs rel errors vs the fp32 oracle on samples 0..%d:" % (dt, B, NS - 1), {k: "%.2e" % v for k, v in worst.items()})
    # x_A2_fake is two encode -> decode round trips deep (~60 roundings): its MAX-abs error over 2 x 3 x 256 x 256 values measured 6.1e-2 at
    # bf16 B=8 (round 5), every other tensor <= 3.9e-2; it gets the bound the docstring above states for it against the emulated contract
    bad = {k: v for k, v in worst.items() if not v < (max(FTOL[dt], ETOL_F[dt]) if k == "x_A2_fake" else FTOL[dt])}
    assert not bad, bad
    p99, mean = _dist(xA2[:NS], fw["x_A2_fake"])
    print("%s B=%d x_A2_fake vs the fp32 oracle on samples 0..%d: p99 %.3e, mean %.3e (relative absolute error)" % (dt, B, NS - 1, p99, mean))
    assert p99 <= X2_DIST[(dt, B)][0] and mean <= X2_DIST[(dt, B)][1], (p99, mean, X2_DIST[(dt, B)])
    # ---- the update at B=32 ----
    gen0 = tr._param[0].clone(); dis0 = tr._param[1].clone()
    assert tr.grad_scale() == SCALE[dt]
    tr.gen_update(x_a, x_b, cfg, z=z[3:])
    torch.cuda.synchronize()
    want = {"loss_idt_A": (rec[:, :3] - xa).abs().mean().item(),
            "loss_gen_adv_B": sum(((o - 1) ** 2).mean().item() for o in dB),
            "loss_gen_adv_A": sum(0.5 * ((o[:B] - 1) ** 2).mean().item() + 0.5 * ((o[B:] - 1) ** 2).mean().item() for o in dA),
            "loss_gen_adv_2": sum(((o[:B] - 1) ** 2).mean().item() + (o[B:] ** 2).mean().item() for o in d2)}
    # (the public-API forward feeds fp32 copies of the 16-bit tensors through different kernels than the step: same values, another summation
    #  order, and in bf16 a rounding flip is a 2^-9 kick -- hence 2e-3 there; fp16 measured <= 1.5e-5)
    ltol = 1e-4 if dt == "fp16" else 2e-3
    for n, v in want.items():
        got = float(getattr(tr, n))
        print("  %s B=%d %s: step %.6f, recomputed from the public-API forward %.6f" % (dt, B, n, got, v))
        assert np.isfinite(got) and abs(got - v) <= ltol * max(1e-3, abs(v)), (n, got, v)
    if dt == "fp16":
        st = tr.loss_scale_state()
        assert st["skipped_gen"] == 0 and st["scale"] == 65536.0 and st["clean_updates"] == 1, st
    assert tr.grad_scale() == SCALE[dt]
    assert torch.equal(tr._param[1], dis0)
    d = (tr._param[0] - gen0).abs().max().item()
    assert 0 < d <= 1.01 * cfg["lr"]
    gen1 = tr._param[0].clone()
    tr.dis_update(x_a, x_b, cfg, z=z[:3])
    torch.cuda.synchronize()
    assert torch.equal(tr._param[0], gen1)
    assert 0 < (tr._param[1] - dis0).abs().max().item() <= 1.01 * cfg["lr"]
    assert np.isfinite(float(tr.loss_dis_total)) and (dt != "fp16" or tr.loss_scale_state()["skipped_dis"] == 0)


# Measured on the MI355X (round 5, three builds): worst relative deviation of loss_gen_total / loss_dis_total from the fp32 HIP run over the 20
# iterations -- bf16 1.1e-1 (iteration 14) / 3.1e-2 .. 5.0e-2; the loss itself falls from 5.85 to 3.63 (gen) and 6.59 to 3.16 (dis) on the way
# (lr x 10), so the 16-bit runs follow the same descent with a lag of about one iteration at worst.  Bands = ~2x the measured worst.
# fp16: 3.3e-2 on loss_dis_total at iteration 19 (5.8e-4 over the first five): the two updates chase each other, a difference of one rounding is amplified from
# iteration to iteration whatever the precision -- the FIRST iterations show the precision, the whole run only that nothing blows up.
# Final build, default (atomics) mode: whole run bf16 1.5e-1 (gen) / 8.5e-2 (dis), fp16 2.5e-2 / 2.6e-2; first five iterations bf16 2.8e-3 / 7.4e-4, fp16 9.0e-4 / 5.9e-4.
# The test runs the three trainers in DETERMINISTIC mode so that its numbers do not move from run to run (the late deviations are an amplification of single
# roundings: with fp32 atomics in the path they changed by 40 % between two builds).  Deterministic mode, final build: whole run bf16 1.17e-1 / 3.65e-2,
# fp16 1.45e-2 / 3.17e-2; first five iterations bf16 2.5e-3 / 6.5e-4, fp16 7.6e-4 / 5.4e-4.
TRACK_BAND = {"bf16": {"loss_gen_total": 3.5e-1, "loss_dis_total": 3.5e-1}, "fp16": {"loss_gen_total": 1e-1, "loss_dis_total": 1e-1}}
TRACK_EARLY = {"bf16": 2e-2, "fp16": 5e-3}          # first five iterations: the precision of the dtype (measured 2.8e-3 / 9.0e-4)


def test_loss_trajectory_16bit_first_five_iterations_at_dtype_precision_and_no_blow_up_over_twenty(T):
    """Twenty chained iterations (dis_update, gen_update, update_learning_rate; reduced width, fixed batches and noise, lr x 10 so that the
    parameters move): the bf16 and fp16 HIP trainers follow the fp32 HIP trainer -- loss_gen_total and loss_dis_total of every iteration
    within a stated band over the whole run and at precision level over the first five iterations (only fp32 had chained-step and loop tests before).  fp16 runs under its
    dynamic loss scaling and must not skip an update on the way."""
    cfg = O.default_config()
    cfg["gen"].update(dim=32, mlp_dim=64, n_res=2); cfg["dis"].update(dim=32)
    cfg["display_size"] = 1
    cfg["focus_epsilon"] = 0.5
    cfg["lr"] = 10 * cfg["lr"]
    nets = O.test_nets(cfg, 4)
    NIT = 20
    batches = [_inputs(2, 64, 100 + i % 3) for i in range(NIT)]          # three batches in rotation, their own noise
    traj = {}
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib as L
    prev_det = L.lib.aclgan_get_deterministic()
    for dt in ("fp32", "bf16", "fp16"):
        tr = T.aclgan_Trainer(cfg, compute_dtype=dt, deterministic=True)
        for name in O.OracleTrainer.NETS:
            getattr(tr, name).load_state_dict(nets[name], strict=False)
        rows = []
        for it in range(NIT):
            x_a, x_b, z = batches[it]
            tr.dis_update(x_a, x_b, cfg, z=z[:3]); tr.gen_update(x_a, x_b, cfg, z=z[3:]); tr.update_learning_rate()
            rows.append((float(tr.loss_gen_total), float(tr.loss_dis_total)))
        traj[dt] = rows
        if dt == "fp16":
            st = tr.loss_scale_state()
            assert st["skipped_gen"] == 0 and st["skipped_dis"] == 0, st
    L.check(L.lib.aclgan_set_deterministic(prev_det))
    # the losses must actually move over the run (otherwise "tracks" says nothing)
    g0, g1 = traj["fp32"][0][0], traj["fp32"][-1][0]
    d0, d1 = traj["fp32"][0][1], traj["fp32"][-1][1]
    print("fp32 trajectory: loss_gen_total %.4f -> %.4f, loss_dis_total %.4f -> %.4f" % (g0, g1, d0, d1))
    assert abs(d1 - d0) > 1e-2 * abs(d0)
    failures = []
    for dt in ("bf16", "fp16"):
        worst = {"loss_gen_total": (0.0, -1), "loss_dis_total": (0.0, -1)}
        for it in range(NIT):
            for j, name in enumerate(("loss_gen_total", "loss_dis_total")):
                ref = traj["fp32"][it][j]; got = traj[dt][it][j]
                assert np.isfinite(got)
                dev = abs(got - ref) / max(1e-3, abs(ref))
                if dev > worst[name][0]:
                    worst[name] = (dev, it)
        print("%s vs fp32 over %d iterations, worst relative deviation (iteration):" % (dt, NIT), {k: ("%.2e" % v[0], v[1]) for k, v in worst.items()})
        failures += [(dt, name, dev, it) for name, (dev, it) in worst.items() if not dev <= TRACK_BAND[dt][name]]
        # no divergence: the deviation over the last five iterations is not an order of magnitude above the first five
        for j, name in enumerate(("loss_gen_total", "loss_dis_total")):
            early = max(abs(traj[dt][it][j] - traj["fp32"][it][j]) / max(1e-3, abs(traj["fp32"][it][j])) for it in range(5))
            late = max(abs(traj[dt][it][j] - traj["fp32"][it][j]) / max(1e-3, abs(traj["fp32"][it][j])) for it in range(NIT - 5, NIT))
            print("  %s %s: worst deviation over iterations 0-4 %.2e, over iterations %d-%d %.2e" % (dt, name, early, NIT - 5, NIT - 1, late))
            if not early <= TRACK_EARLY[dt]:
                failures.append((dt, name, "first five iterations", early))
    assert not failures, failures


def test_fp16_loss_scale_state_survives_a_checkpoint(T, tmp_path):
    """save() / resume() carry the dynamic loss-scale state (scale, clean counter, skipped-update counts): after a resume Adam's
    bias-correction step and the live scale continue where they were, and grad_scale() reports the scale the LAST update ran with
    even after that update halved it."""
    cfg = O.default_config()
    cfg["gen"].update(dim=32, mlp_dim=32, n_res=1)
    cfg["dis"].update(dim=32)
    cfg["display_size"] = 1
    cfg["loss_scale_init"] = 2.0 ** 40
    nets = O.test_nets(cfg, 2)
    x_a, x_b, z = _inputs(1, 64, 26)
    tr = _make(T, cfg, nets, "fp16")
    tr.dis_update(x_a, x_b, cfg, z=z[:3])             # overflows: skipped, scale halves
    torch.cuda.synchronize()
    assert tr.loss_scale_state()["scale"] == 2.0 ** 39 and tr.grad_scale() == 2.0 ** 40      # the buffers of that update carry 2^40
    assert tr.grad_scale("dis") == 2.0 ** 40 and tr.grad_scale("gen") == 2.0 ** 39           # (gen not updated yet: the live scale)
    tr.gen_update(x_a, x_b, cfg, z=z[3:])              # runs at 2^39 (overflows again): per group, not one shared slot
    torch.cuda.synchronize()
    assert tr.grad_scale("gen") == 2.0 ** 39 and tr.grad_scale("dis") == 2.0 ** 40 and tr.grad_scale() == 2.0 ** 39
    live = tr.loss_scale_state()["scale"]
    assert live == 2.0 ** 38, live
    tr.save(str(tmp_path), 0)
    tr2 = T.aclgan_Trainer(cfg, compute_dtype="fp16")
    tr2.resume(str(tmp_path), cfg)
    a, b = tr.loss_scale_state(), tr2.loss_scale_state()
    assert a == b and b["skipped_dis"] == 1 and b["skipped_gen"] == 1 and b["scale"] == live, (a, b)
