"""The repeated-batch construction behind the 16-bit frozen-mask cases at the benchmarked batches (tests/test_gpu_maskfrozen.py).

The HIP update runs at the full batch B, made of d distinct samples (x_a, x_b, z), each repeated k = B / d times; the oracle runs the d
distinct samples only.  Every normalisation is per sample, the LSGAN and L1 losses are batch means (the discriminators' joint batches
included) and the focus digit term is divided by B.  The one term that couples samples is the focus size term,
relu(sum(m - u))^2 * delta / (H W B 3): over k copies the sum is k times the d-sample sum, so the term is k times the d-sample term with
the same delta.  Hence, in exact arithmetic, the B-row loss with focus_delta = delta and the d-row loss with focus_delta = k delta are the
same function of the parameters, and so are their gradients.

Under the emulated 16-bit contract each copy carries 1/k of the per-sample activation gradient; with the loss scale S / k in the d-row
oracle against S in the B-row update, every value rounded to 16 bits is the same number (fp16 underflow into subnormals included).

Checked here at a reduced width and a 64x64 map: in float64 every parameter gradient agrees to 1e-12; under the 16-bit emulation what is
left is fp32 summation order.  The forward-only loss graph under torch.no_grad() records the same activation masks and sign decisions as
the full update, so the GPU cases may use it for mask matching instead of a second full oracle update."""
import copy

import pytest
import torch

from oracle import aclgan_oracle as O

D_SAMPLES = 4


def arrangement_faults(bmap, d):
    """what is wrong with a batch map (position -> distinct sample) for the repeated-batch construction; [] = fine.  A kernel that reads
    the wrong sample should usually read different data: every sample k times, not i % d, no cyclic shift (the half swap included)
    maps the arrangement onto itself, and the first and last positions hold different samples."""
    B = len(bmap)
    out = []
    if B % d or sorted(bmap) != sorted(list(range(d)) * (B // d)):
        out.append("not every sample %d times" % (B // d))
    if bmap == [i % d for i in range(B)]:
        out.append("i % d")
    for s in range(1, B):
        if bmap[s:] + bmap[:s] == bmap:
            out.append("invariant under a cyclic shift by %d" % s)
            break
    if bmap[0] == bmap[-1]:
        out.append("first and last position hold the same sample")
    return out


def batch_map(B, d=D_SAMPLES, seed=0):
    """a fixed, seeded, non-periodic arrangement of d samples over B positions (the first seeded permutation without faults)"""
    g = torch.Generator().manual_seed(seed)
    while True:
        bmap = [int(p) % d for p in torch.randperm(B, generator=g)]
        if not arrangement_faults(bmap, d):
            return bmap


def repeat_batch(x_a, x_b, z, bmap):
    """the B-row inputs: row i holds distinct sample bmap[i] (x_a, x_b and every z alike)"""
    idx = torch.tensor(bmap)
    return x_a[idx].contiguous(), x_b[idx].contiguous(), [t[idx].contiguous() for t in z]


def rescaled_config(cfg, k):
    """the d-sample oracle's config: focus_delta * k (the focus size term over k copies is k times the d-sample term)"""
    c = copy.deepcopy(cfg)
    c["focus_delta"] = cfg["focus_delta"] * k
    return c


def rescaled_loss_scale(S, k):
    """the d-sample oracle's loss scale: each copy carries 1 / k of the per-sample gradient at S"""
    return S / k


def _setup(dtype=torch.float32):
    cfg = O.default_config()
    cfg["gen"].update(dim=16, mlp_dim=16, n_res=1); cfg["dis"].update(dim=16)     # dim 16: 64-channel layers, so the 16-bit storage runs
    cfg["display_size"] = 1; cfg["focus_epsilon"] = 0.5
    nets = {n: {k: t.to(dtype) for k, t in p.items()} for n, p in O.test_nets(cfg, 0).items()}
    g = torch.Generator().manual_seed(5)
    x_a = (torch.rand(D_SAMPLES, 3, 64, 64, generator=g) * 2 - 1).to(dtype)
    x_b = (torch.rand(D_SAMPLES, 3, 64, 64, generator=g) * 2 - 1).to(dtype)
    z = [torch.randn(D_SAMPLES, 8, 1, 1, generator=g).to(dtype) for _ in range(6)]
    return cfg, nets, x_a, x_b, z


_GROUPS = (("dis", 0, ("dis_A", "dis_B", "dis_2")), ("gen", 3, ("gen_AB", "gen_BA")))


def _grads(cfg, nets, x_a, x_b, zz, which, names, ctx=None):
    orc = O.OracleTrainer(cfg, nets=nets)
    if ctx is None:
        getattr(orc, which + "_update")(x_a, x_b, zz, apply=False)
    else:
        with ctx:
            getattr(orc, which + "_update")(x_a, x_b, zz, apply=False)
    return {(n, k): t.grad.double() for n in names for k, t in orc.nets[n].items() if t.grad is not None}


def _worst(got, want, floor):
    """worst relative L2 over the tensors whose reference norm is >= floor * the largest one (biases in front of Instance / AdaIN norms are
    exactly zero in exact arithmetic)"""
    gmax = max(t.norm().item() for t in want.values())
    errs = [((got[k] - w).norm().item() / w.norm().item(), k) for k, w in want.items() if w.norm().item() >= floor * gmax]
    assert len(errs) >= 0.8 * len(want)
    return max(errs)


@pytest.mark.parametrize("B", [8, 32])
def test_arrangement(B):
    bmap = batch_map(B)
    assert arrangement_faults(bmap, D_SAMPLES) == [], bmap
    assert bmap == batch_map(B)      # fixed
    k = B // D_SAMPLES
    assert all(bmap.count(j) == k for j in range(D_SAMPLES))
    assert bmap[B // 2:] + bmap[:B // 2] != bmap and bmap[0] != bmap[-1] and bmap != [i % D_SAMPLES for i in range(B)]
    # (the checker itself: i % d is periodic, a half-repeated map is invariant under the half swap)
    assert arrangement_faults([i % D_SAMPLES for i in range(B)], D_SAMPLES)
    assert arrangement_faults(bmap[:B // 2] * 2, D_SAMPLES)


@pytest.mark.parametrize("k", [2, 8])
def test_repeated_batch_gradients_match_in_float64(k):
    """B = k d rows with focus_delta against d rows with focus_delta * k: every parameter gradient of both updates to 1e-12 relative L2"""
    cfg, nets, x_a, x_b, z = _setup(torch.float64)
    xr_a, xr_b, zr = repeat_batch(x_a, x_b, z, batch_map(k * D_SAMPLES))
    cfg_d = rescaled_config(cfg, k)
    assert cfg_d["focus_delta"] == k * cfg["focus_delta"] and cfg["focus_delta"] == O.default_config()["focus_delta"]
    for which, z0, names in _GROUPS:
        got = _grads(cfg, nets, xr_a, xr_b, zr[z0:z0 + 3], which, names)
        want = _grads(cfg_d, nets, x_a, x_b, z[z0:z0 + 3], which, names)
        e, key = _worst(got, want, 1e-6)
        print("float64 k=%d %s_update: worst relative L2 %.2e %s" % (k, which, e, key))
        assert e <= 1e-12, (which, e, key)
    # ... and the construction is not vacuous: the un-rescaled focus_delta gives another generator gradient
    got = _grads(cfg, nets, xr_a, xr_b, zr[3:], "gen", ("gen_AB", "gen_BA"))
    want = _grads(cfg, nets, x_a, x_b, z[3:], "gen", ("gen_AB", "gen_BA"))
    assert _worst(got, want, 1e-6)[0] > 1e-9


# fp32 summation order only: the B-row and d-row batch sums differ in the last fp32 bit, which flips the 16-bit rounding of a few values,
# and the flips compound through the generator's stacked layers.  Worst relative L2 over the tensors (measured: dis_update 6.0e-7 bf16 /
# 1.5e-6 fp16, gen_update 1.8e-3 bf16 / 2.9e-4 fp16, both on enc_content.model.0), bounds ~3x that; the GPU cases' ETOL_FROZEN is >= 17x above
RTOL_16 = {"bf16": {"dis": 1e-5, "gen": 5e-3}, "fp16": {"dis": 1e-5, "gen": 1e-3}}


@pytest.mark.parametrize("dt,k", [("bf16", 2), ("fp16", 8)])
def test_repeated_batch_gradients_match_under_16bit_emulation(dt, k):
    """compute_dtype(dt, S) over the B = k d rows against compute_dtype(dt, S / k) over the d rows, S as the HIP update (bf16 1, fp16
    65536): the gradients (unscaled, as the emulation returns them) agree up to fp32 summation order"""
    cfg, nets, x_a, x_b, z = _setup()
    S = 65536.0 if dt == "fp16" else 1.0
    xr_a, xr_b, zr = repeat_batch(x_a, x_b, z, batch_map(k * D_SAMPLES))
    cfg_d = rescaled_config(cfg, k)
    for which, z0, names in _GROUPS:
        got = _grads(cfg, nets, xr_a, xr_b, zr[z0:z0 + 3], which, names, O.compute_dtype(dt, loss_scale=S))
        want = _grads(cfg_d, nets, x_a, x_b, z[z0:z0 + 3], which, names, O.compute_dtype(dt, loss_scale=rescaled_loss_scale(S, k)))
        e, key = _worst(got, want, 1e-3)
        print("%s k=%d %s_update: worst relative L2 %.2e %s" % (dt, k, which, e, key))
        assert e <= RTOL_16[dt][which], (dt, which, e, key)


@pytest.mark.parametrize("dt", [None, "fp16"])
def test_forward_only_loss_graph_records_the_update_masks(dt):
    """the loss graph alone under torch.no_grad() inside act_masks() records the same activation masks and sign decisions, in the same
    order, as the full oracle update"""
    cfg, nets, x_a, x_b, z = _setup()
    for which, z0, _ in _GROUPS:
        zz = z[z0:z0 + 3]
        ctx = O.compute_dtype(dt, loss_scale=8192.0) if dt else O.compute_dtype("fp32")
        with ctx, O.act_masks() as full:
            getattr(O.OracleTrainer(cfg, nets=nets), which + "_update")(x_a, x_b, zz, apply=False)
        with ctx, O.act_masks() as fwd, torch.no_grad():
            (O.gen_losses if which == "gen" else O.dis_losses)(nets, x_a, x_b, zz, cfg)
        assert len(full.recorded) > 10 and len(fwd.recorded) == len(full.recorded), (which, len(fwd.recorded), len(full.recorded))
        assert all(torch.equal(a, b) for a, b in zip(fwd.recorded, full.recorded)), which
        assert len(fwd.signs) == len(full.signs) == (5 if which == "gen" else 0)
        assert all(torch.equal(a, b) for a, b in zip(fwd.signs, full.signs)), which
