"""Backward parity with the activation masks HELD FIXED (round 6).

The step-level gradient tests (tests/test_gpu_fullsize.py: every gradient tensor within 1e-2 relative L2 of the fp32 oracle, measured
5 - 6e-3) cannot tell a sloppy backward kernel from the "mask lottery": two correct fp32 implementations take different branches of a
ReLU / LeakyReLU wherever a pre-activation lies within forward rounding (~1e-5) of zero, and every flipped element moves all upstream
gradients.  Here the lottery is taken out: the HIP update records the masks it ran with (aclgan_debug_capture_masks: output > 0 of every
Conv2dBlock it back-propagates through, plus the step's two other sign decisions: |m - 0.5| of the focus digit losses and |x_recon - x| of
the identity losses), the oracle's autograd replays the same update with THOSE masks in place of its own (oracle.act_masks), and what is left is the error of the backward kernels themselves (summation order, Winograd transforms, atomics):

    fp32   every gradient tensor <= 1e-3 relative L2 -- measured 1.3e-5 (gen_update) / 2.5e-6 (dis_update) at 256x256 B=2, against 7.2e-3 /
           4.3e-4 un-frozen in the same run: 398 of 2.5e8 mask elements and ONE of 1.2e6 loss signs differed; at the benchmarked B=8 (the
           stride-2 parity phases at the benchmark's own grids) 1.56e-5 (gen_update, p99 1.56e-5, mean 6.6e-6) / 2.4e-6 (dis_update) against
           7.6e-3 / 5.5e-4 un-frozen.  A stride-2 input-gradient phase that drops its last 16 channels of K moves the first-layer gradients
           behind it (enc_content / enc_style model.0, the discriminators' cnns.0.0) to 0.4 - 0.5, at B=2 and at B=8 alike
    bf16 / fp16 against the EMULATED 16-bit contract (oracle.compute_dtype) with the masks frozen: per network bounds below, at 128x128 B=2
           and at the benchmarked 256x256 bf16 B=8 / fp16 B=32, where the batch is four distinct samples repeated (the oracle runs the four;
           tests/test_oracle_repeat_batch_cpu.py) and the copies of a sample must record identical masks.

Blocks are matched between the two implementations by CONTENT, not by order (the engine builds the passes of an update in its lane order
and runs the discriminators on joint batches): a recorded mask (split into the update's batch-sized chunks) belongs to the oracle
activation of the same shape it agrees with on >= 99 % of the elements -- unrelated passes agree on ~50 %."""
import ctypes as C
import gc
import os

import pytest
import torch

from oracle import aclgan_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    assert torch.cuda.is_available()
    import aclgan_amd  # noqa: F401
    from aclgan_amd import trainer
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    return trainer


def _make(T, cfg, nets, dt=None):
    tr = T.aclgan_Trainer(cfg, compute_dtype=dt) if dt else T.aclgan_Trainer(cfg)
    for name in O.OracleTrainer.NETS:
        getattr(tr, name).load_state_dict(nets[name], strict=False)
    return tr


def _inputs(B, S, seed):
    g = torch.Generator().manual_seed(seed)
    x_a = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    x_b = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    z = [torch.randn(B, 8, 1, 1, generator=g) for _ in range(6)]
    return x_a, x_b, z


def _by_sample(m, bmap):
    """m: (B, ...) bool on the device; bmap: position -> distinct sample (the repeated-batch construction, test_oracle_repeat_batch_cpu.py).
    Returns the (d, ...) mask the copies of each sample agree on by majority (a tie takes the first copy) and how many elements of the
    copies differ from it"""
    d = max(bmap) + 1
    rows, ndiff = [], 0
    for j in range(d):
        cp = m[[i for i, s in enumerate(bmap) if s == j]]
        n = cp.sum(0, dtype=torch.int32) * 2
        maj = (n > cp.shape[0]) | ((n == cp.shape[0]) & cp[0])
        ndiff += int((cp != maj).sum())
        rows.append(maj)
    return torch.stack(rows), ndiff


def _hip_update_with_masks(tr, which, x_a, x_b, cfg, z, B, cap_bytes, used=None, bmap=None):
    """run one update with the mask recording on; returns the masks as NCHW bool CPU tensors in batch-sized chunks.
    used: a one-element list -- only measure the bytes the recording took (end of the last mask), nothing is copied back.
    bmap: the batch is made of repeated samples (position -> distinct sample): every chunk and sign decision is reduced to one row per
    distinct sample (_by_sample), and a third value lists the recorded masks whose copies disagree, as (index, act, (b, h, w, c), elements)"""
    from aclgan_amd import _lib as L
    buf = torch.zeros(cap_bytes, dtype=torch.uint8, device="cuda")
    L.check(L.lib.aclgan_debug_capture_masks(tr._ctx, L.ptr(buf), cap_bytes), "debug_capture_masks")
    disagree = []

    def rows(m, i, act, dims):
        if bmap is None:
            return m.cpu()
        r, n = _by_sample(m, bmap)
        if n:
            disagree.append((i, act, dims, n))
        return r.cpu()

    try:
        (tr.dis_update if which == "dis" else tr.gen_update)(x_a, x_b, cfg, z=z)
        torch.cuda.synchronize()
        chunks, signs = [], []
        dims = (C.c_int * 4)(); off = C.c_longlong(); act = C.c_int()
        for i in range(L.lib.aclgan_debug_mask_count(tr._ctx)):
            L.check(L.lib.aclgan_debug_mask_info(tr._ctx, i, dims, C.byref(off), C.byref(act)), "debug_mask_info")
            b, h, w, c = list(dims)
            if used is not None:
                used[0] = max(used[0], off.value + b * h * w * c)
                continue
            m = buf[off.value: off.value + b * h * w * c].view(b, h, w, c).permute(0, 3, 1, 2).bool()
            if act.value == 100:        # sign of a focus mask's (m - 0.5): channel 3 of the decoder output (2 m - 1)
                signs.append(rows(m[:, 3:4], i, act.value, (b, h, w, c)).contiguous())
            elif act.value == 101:      # sign of (x_recon - x) of an identity loss
                signs.append(rows(m, i, act.value, (b, h, w, c)).contiguous())
            else:
                assert b % B == 0, (b, B)
                chunks.extend(rows(m[j:j + B], i, act.value, (b, h, w, c)) for j in range(0, b, B))
    finally:
        L.check(L.lib.aclgan_debug_capture_masks(tr._ctx, None, 0), "debug_capture_masks(off)")
    return (chunks, signs, disagree) if bmap is not None else (chunks, signs)


def _match(recorded, chunks, exclusive=False, stride=13):
    """replay dictionary {oracle activation index: the HIP mask of the same block}; also the flip statistics.
    exclusive (spectral norm: every reference discriminator call is a pass of its own): each recorded chunk serves one oracle activation,
    and among the chunks that agree with it on >= 99 % the first one not yet taken wins -- the two real dis_A calls of dis_update see the
    same x_a with different sigmas, so their masks agree on nearly every element, and the engine runs one network's calls in the
    reference's order.  used[j]: how many oracle activations took chunk j.
    stride: the agreement is measured on every stride-th element; 1 where masks are small (a 1 x 1 x 64 mask of a coarse discriminator scale at
    B = 1 leaves 5 samples at the default stride, and unrelated passes then agree on all of them by chance)"""
    by_shape = {}
    for j, ch in enumerate(chunks):
        by_shape.setdefault(tuple(ch.shape), []).append(j)
    replay, flips, total, unmatched = {}, 0, 0, []
    used = [0] * len(chunks)
    for i, own in enumerate(recorded):
        cands = by_shape.get(tuple(own.shape), [])
        best, best_agree = None, 0.0
        sub = own.flatten()[::stride]
        for j in cands:
            if exclusive and used[j]:
                continue
            a = (chunks[j].flatten()[::stride] == sub).float().mean().item()
            if exclusive and a >= 0.99:
                best, best_agree = j, a
                break
            if a > best_agree:
                best, best_agree = j, a
        if best is not None and best_agree >= 0.99:
            replay[i] = chunks[best]
            used[best] += 1
            flips += int((chunks[best] != own).sum()); total += own.numel()
        else:
            unmatched.append((i, tuple(own.shape), round(best_agree, 3)))
    return (replay, flips, total, unmatched, used) if exclusive else (replay, flips, total, unmatched)


def _grad_errors(tr, orc, nets_, scale=1.0, floor=1e-3):
    gmax = max(float(t.grad.norm()) for n in nets_ for t in orc.nets[n].values() if t.grad is not None)     # (SN u / v: no gradient)
    out = []
    for n in nets_:
        for k, gr in getattr(tr, n).named_grads():
            ref = orc.nets[n][k].grad.double()
            rn = ref.norm().item()
            if rn >= floor * gmax:       # (tensors that are exactly zero in exact arithmetic -- biases in front of Instance / AdaIN norms -- are the fullsize test's business)
                out.append(((gr.cpu().double() / scale - ref).norm().item() / rn, n, k))
    out.sort(reverse=True)
    return out


def _frozen_and_free(T, dt, B, S, seed, forced=False, cap_bytes=None, d=None, rerun=False, free=True, sn=False):
    """forced: every eligible convolution through the one-launch Winograd kernel (tuning wino_fused = 2): at B = 2 the cost models keep the
    4x4 stride-2 layers and the small grids on the direct kernels / the pipeline, so the default run does not reach those kernels.
    The library's plan (default / deterministic) is whatever the caller set; the oracle follows it (_frozen_and_free_impl)"""
    from aclgan_amd import _lib as L
    old = L.lib.aclgan_set_tuning(b"wino_fused", 2) if forced else None
    try:
        return _frozen_and_free_impl(T, dt, B, S, seed, cap_bytes, d, rerun, free, sn)
    finally:
        if forced:
            L.lib.aclgan_set_tuning(b"wino_fused", old)


def _sn_copy(nets):
    """the oracle advances SN u / v in place: every oracle run starts from a copy of the initial state"""
    return {k: {n: t.clone() for n, t in v.items()} for k, v in nets.items()}


def _frozen_and_free_impl(T, dt, B, S, seed, cap_bytes=None, d=None, rerun=False, free=True, sn=False):
    """d: the HIP update runs at batch B made of d distinct samples, each B / d times (the repeated-batch construction of
    tests/test_oracle_repeat_batch_cpu.py), and the oracle runs the d samples alone with focus_delta * k and the loss scale / k.  Its
    own masks then come from the loss graph alone under no_grad (the same activation list, test_forward_only_loss_graph_records_the_
    update_masks), so there is no masks-free gradient figure.
    In deterministic mode the oracle emulates that plan's 16-bit contract: the input gradient of the sub-pixel layers through the rounded
    5x5 (compute_dtype(up5_dgrad="plain")) -- every other pass computes the same contract in both plans.
    rerun: a second trainer from the same state runs the same update (mask recording on, as in the first); res[which]["rerun_differ"] lists
    the gradient tensors whose bits differ from the first run's.
    free = False: no masks-free gradient figure either -- the oracle's own masks come from the forward-only loss graph, as with d
    sn: dis.norm sn with the seeded SN state of tests/sn_nets.py; recorded chunks are matched exclusively (_match), res[which] also holds
    "used" (oracle activations per recorded chunk) and "uv" (max |u - u_oracle|, |v - v_oracle| over every SN layer after the update)"""
    from test_oracle_repeat_batch_cpu import batch_map, repeat_batch, rescaled_config, rescaled_loss_scale
    from aclgan_amd import _lib as L
    det = L.lib.aclgan_get_deterministic() == 1
    cfg = O.default_config()
    cfg["display_size"] = 1
    cfg["focus_epsilon"] = 0.5      # smooth fixture (tests/golden/make_golden.py: the default 0.01 has a sign discontinuity of 1e4 at m = 0.5)
    if sn:
        from sn_nets import sn_test_nets
        cfg["dis"]["norm"] = "sn"
        nets = sn_test_nets(cfg, 0)
    else:
        nets = O.test_nets(cfg, 0)
    onets = _sn_copy if sn else (lambda n: n)
    scale = 65536.0 if dt == "fp16" else 1.0
    if d is None:
        x_a, x_b, z = _inputs(B, S, seed)
        hx_a, hx_b, hz, bmap, ocfg, oscale = x_a, x_b, z, None, cfg, scale
    else:
        k = B // d
        x_a, x_b, z = _inputs(d, S, seed)
        bmap = batch_map(B, d)
        hx_a, hx_b, hz = repeat_batch(x_a, x_b, z, bmap)
        ocfg, oscale = rescaled_config(cfg, k), rescaled_loss_scale(scale, k)

    class ctx:      # the oracle under the build's arithmetic contract (plain fp32, or the emulated 16-bit contract)
        def __enter__(self):
            self.c = O.compute_dtype(dt, loss_scale=oscale, up5_dgrad="plain" if det else "merged") if dt else None
            return self.c.__enter__() if self.c else None

        def __exit__(self, *a):
            return self.c.__exit__(*a) if self.c else None

    res = {}
    for which, zs, nets_ in (("dis", slice(0, 3), ("dis_A", "dis_B", "dis_2")), ("gen", slice(3, 6), ("gen_AB", "gen_BA"))):
        zz = z[zs]
        tr = _make(T, cfg, nets, dt)
        assert tr.deterministic == det
        if dt:
            assert tr.grad_scale() == scale
        cap = cap_bytes[which] if cap_bytes else (2 << 30 if S >= 256 else 1 << 29)
        out = _hip_update_with_masks(tr, which, hx_a, hx_b, cfg, hz[zs], B, cap, bmap=bmap)
        chunks, signs = out[:2]
        disagree = out[2] if bmap is not None else []
        assert chunks, "nothing recorded"
        assert len(signs) == (5 if which == "gen" else 0), len(signs)      # focus B, A, A2 + identity A, B: the oracle's call order (gen_losses)
        if dt == "fp16":
            st = tr.loss_scale_state()
            assert st["skipped_gen"] == 0 and st["skipped_dis"] == 0 and st["scale"] == scale and st["clean_updates"] == 1, (which, st)
            assert tr.grad_scale() == scale
        with ctx(), O.act_masks() as rec:                    # the oracle with its OWN masks
            orc_free = O.OracleTrainer(ocfg, nets=nets)
            if bmap is None and free:
                (orc_free.dis_update if which == "dis" else orc_free.gen_update)(x_a, x_b, zz, apply=False)
            else:
                with torch.no_grad():
                    (O.dis_losses if which == "dis" else O.gen_losses)(onets(nets), x_a, x_b, zz, ocfg)
        if sn:
            replay, flips, total, unmatched, used = _match(rec.recorded, chunks, exclusive=True)
        else:
            replay, flips, total, unmatched = _match(rec.recorded, chunks)
        sflips = sum(int((a != b).sum()) for a, b in zip(signs, rec.signs))
        with ctx(), O.act_masks(replay, dict(enumerate(signs))) as rec2:             # ... and with the masks / signs of the HIP update
            frozen = O.OracleTrainer(ocfg, nets=nets)
            (frozen.dis_update if which == "dis" else frozen.gen_update)(x_a, x_b, zz, apply=False)
        assert len(rec2.recorded) == len(rec.recorded)
        e_frozen = _grad_errors(tr, frozen, nets_, scale)
        e_free = _grad_errors(tr, orc_free, nets_, scale) if bmap is None and free else None
        print("%s %s_update @%dx%d B=%d%s: %d of %d oracle activations matched to a recorded mask (%d recorded chunks), %d of %d mask elements differ (%.2e)"
              % (dt or "fp32", which, S, S, B, "" if bmap is None else " (%d distinct samples, batch map %s)" % (d, bmap), len(replay),
                 len(rec.recorded), len(chunks), flips, total, flips / max(1, total)))
        if bmap is not None:
            print("   copies of a sample that recorded another mask element than their majority: %d elements in %d recorded masks %s"
                  % (sum(n for *_, n in disagree), len(disagree), disagree[:8]))
        print("   sign decisions of the focus digit / identity losses that differ: %d of %d" % (sflips, sum(a.numel() for a in signs)))
        print("   unmatched oracle activations (no gradient passes through them in the HIP update):", unmatched[:8], "..." if len(unmatched) > 8 else "")
        print("   worst gradient tensors, masks FROZEN:", [("%.2e" % e, n, k) for e, n, k in e_frozen[:4]])
        if e_free is not None:
            print("   worst gradient tensors, masks free  :", [("%.2e" % e, n, k) for e, n, k in e_free[:4]])
        ef = torch.tensor([e for e, _, _ in e_frozen], dtype=torch.float64)
        print("   masks FROZEN over all %d gradient tensors: p99 %.2e, mean %.2e" % (len(ef), torch.quantile(ef, 0.99).item(), ef.mean().item()))
        res[which] = dict(frozen=e_frozen, free=e_free, matched=len(replay), acts=len(rec.recorded), unmatched=unmatched, disagree=disagree)
        if sn:
            uv = 0.0
            for n in ("dis_A", "dis_B", "dis_2"):
                for k, t in getattr(tr, n).state_dict().items():
                    if O.is_sn_state(k):
                        uv = max(uv, (t.cpu().double() - frozen.nets[n][k].double()).abs().max().item())
            res[which].update(used=used, chunks=len(chunks), uv=uv)
            print("   SN: recorded chunks taken by 0 / 1 / >1 oracle activations: %d / %d / %d; max |u, v - oracle| %.2e"
                  % (used.count(0), used.count(1), sum(1 for x in used if x > 1), uv))
        if rerun:
            first = {(n, k): g.detach().clone() for n in nets_ for k, g in getattr(tr, n).named_grads()}
            del tr
            gc.collect()      # (a trainer's arena is released when its reference cycles are)
            tr2 = _make(T, cfg, nets, dt)
            _hip_update_with_masks(tr2, which, hx_a, hx_b, cfg, hz[zs], B, cap, used=[0])
            res[which]["rerun_differ"] = [key for key, g in first.items() if not torch.equal(dict(getattr(tr2, key[0]).named_grads())[key[1]], g)]
            print("   second update from the same state: %d of %d gradient tensors differ in their bits" % (len(res[which]["rerun_differ"]), len(first)))
            del tr2, first
    return res


def _per_net(errs):
    out = {}
    for e, n, k in errs:
        key = n if n.startswith("dis") else n + (".enc" if k.startswith("enc_") else ".dec")
        out[key] = max(out.get(key, 0.0), e)
    return out


@pytest.mark.parametrize("forced", [False, True], ids=["default-paths", "fused-winograd-forced"])
def test_backward_parity_with_frozen_masks_fp32(T, forced):
    """256x256 B=2, full width: with the HIP update's own ReLU / LeakyReLU masks replayed by the oracle every gradient tensor agrees to 1e-3
    relative L2 (the bound of tests/test_gpu_fullsize.py on the un-frozen comparison stays 1e-2).  Second case: the one-launch Winograd kernel
    FORCED on every eligible layer -- the 3x3 ResBlock layers, the sub-pixel phases and (round 6) the four parity phases of the 4x4 stride-2
    layers, forward and input gradient -- the kernels the benchmarked batch runs but B = 2 would not reach."""
    res = _frozen_and_free(T, None, 2, 256, 31, forced=forced)
    for which in ("dis", "gen"):
        r = res[which]
        # every activation a gradient passes through was matched (dis_update: the generator pass is forward-only in the HIP update)
        assert r["matched"] >= (0.3 if which == "dis" else 0.9) * r["acts"], (which, r["matched"], r["acts"], r["unmatched"][:6])
        assert r["frozen"][0][0] <= 1e-3, (which, r["frozen"][:6])       # (measured 1.3e-5 / 2.5e-6: the bound of the review; 1e-4 would hold)
        assert r["free"][0][0] <= 1e-2, (which, r["free"][:6])


def _executed_flops(tr, which, B, S, s2k4):
    """aclgan_step_executed_flops (a dry run of the launchers' own path predicates) with the stride-2 Winograd phases on / off"""
    from aclgan_amd import _lib as L
    prev, v = C.c_int(), C.c_double()
    L.check(L.lib.aclgan_tuning(b"wino_s2k4", s2k4, C.byref(prev)), "tuning")
    try:
        L.check(L.lib.aclgan_step_executed_flops(tr._ctx, 0 if which == "gen" else 1, B, S, S, C.byref(v)), "step_executed_flops")
    finally:
        L.check(L.lib.aclgan_tuning(b"wino_s2k4", prev.value, None), "tuning")
    return v.value


def _stride2_reached(T, cases):
    """{(which, B): (FLOPs with the stride-2 phases, without)} at 256x256 on the full-width network, default lanes and paths"""
    cfg = O.default_config()
    cfg["display_size"] = 1
    tr = T.aclgan_Trainer(cfg)
    out = {}
    for which, B in cases:
        out[(which, B)] = (_executed_flops(tr, which, B, 256, 1), _executed_flops(tr, which, B, 256, 0))
        print("%s_update @256x256 B=%d executed matrix FLOPs, stride-2 phases on / off: %.4e / %.4e" % ((which, B) + out[(which, B)]))
    return out


def test_frozen_mask_cases_reach_the_stride2_phases(T):
    """the 4x4 stride-2 layers' parity phases (wino_fused_s2k4_ok's cost model): at the benchmarked B = 8 both updates take them (forward and
    input gradient of CE1/CE2/SE1/SE2, the discriminators' layers 1-2, the input gradient of SE3); at B = 2 the generator update already
    takes the input-gradient phases of CE1 / SE1, which the default-paths case above runs.  Path on = fewer executed FLOPs."""
    fl = _stride2_reached(T, (("dis", 8), ("gen", 8), ("gen", 2)))
    for key, (on, off) in fl.items():
        assert on < off, (key, on, off)


def _mask_capture_bytes(T, B, S, seed, dt=None, sn=False):
    """mask-recording buffer for an update at batch B under compute dtype dt: the bytes the same update takes at B = 2
    (aclgan_debug_mask_info's offsets; every recorded mask is a multiple of the batch), scaled by B / 2, plus 10 % and 64 MB of margin.
    sn: with spectrally normalised discriminators (one pass per reference call: dis_update records the real dis_A branch twice)"""
    cfg = O.default_config()
    cfg["display_size"] = 1
    cfg["focus_epsilon"] = 0.5
    if sn:
        from sn_nets import sn_test_nets
        cfg["dis"]["norm"] = "sn"
        nets = sn_test_nets(cfg, 0)
    else:
        nets = O.test_nets(cfg, 0)
    x_a, x_b, z = _inputs(2, S, seed)
    out = {}
    for which, zz in (("dis", z[:3]), ("gen", z[3:])):
        used = [0]
        _hip_update_with_masks(_make(T, cfg, nets, dt), which, x_a, x_b, cfg, zz, 2, 2 << 30, used=used)
        assert used[0] > 0
        out[which] = int(used[0] * B / 2 * 1.1) + (64 << 20)
    return out


def test_backward_parity_with_frozen_masks_fp32_benchmarked_batch(T):
    """256x256 B=8, fp32, default paths and lanes: the benchmarked schedule.  The B = 2 cases above leave most of the stride-2 parity phases
    to the cost model's direct kernels; here they run at the grids and splits the benchmark uses (test_frozen_mask_cases_reach_the_stride2_phases).
    With the HIP update's own masks replayed by the oracle every gradient tensor agrees to 1e-3 relative L2, the bound of the B = 2 cases;
    the masks-free figure is printed beside it (tests/test_gpu_fullsize.py holds that one to 1e-2)."""
    cap = _mask_capture_bytes(T, 8, 256, 33)
    res = _frozen_and_free(T, None, 8, 256, 33, cap_bytes=cap)
    for which in ("dis", "gen"):
        r = res[which]
        assert r["matched"] >= (0.3 if which == "dis" else 0.9) * r["acts"], (which, r["matched"], r["acts"], r["unmatched"][:6])
        assert r["frozen"][0][0] <= 1e-3, (which, r["frozen"][:6])


def _sample_oracle(nets, cfg, x_a, z1, z2, z3):
    """sample()'s nine outputs (trainer.py:179-245, focus branch) from the fp32 oracle"""
    gc = cfg["gen"]
    AB, BA = nets["gen_AB"], nets["gen_BA"]
    want = [[] for _ in range(9)]
    with torch.no_grad():
        for i in range(x_a.size(0)):
            xa = x_a[i:i + 1]
            c1, s1 = O.content_encode(BA, xa, gc), O.style_encode(BA, xa, gc)
            o = O.decode(BA, c1, z1[i:i + 1], gc); a_fake = O.focus_translation(o[:, :3], xa, o[:, 3:]); m_a = o[:, 3:]
            o = O.decode(BA, c1, s1, gc); a_rec, m_rec = o[:, :3], o[:, 3:]
            o = O.decode(AB, O.content_encode(AB, xa, gc), z2[i:i + 1], gc); b_fake = O.focus_translation(o[:, :3], xa, o[:, 3:]); m_b = o[:, 3:]
            o = O.decode(BA, O.content_encode(BA, b_fake, gc), z3[i:i + 1], gc); a2 = O.focus_translation(o[:, :3], b_fake, o[:, 3:])
            for lst, t in zip(want, (xa, a_fake, m_a, b_fake, m_b, a2, o[:, 3:], a_rec, m_rec)):
                lst.append(t)
    return [torch.cat(w) for w in want]


def test_forward_arena_follows_tuning_changes(T):
    """sample() at 256x256 B=2 (full width), then tuning wino_fused = 2 and sample() again.  sample() runs per image, so its forward-only
    arena is sized for B = 1; mode 2 sends every eligible 4x4 stride-2 layer to the parity phases, whose filter-transform scratch grows that
    arena (measured by the dry run: 357.6 -> 431.0 MB).  A forward-only arena is valid for one tuning epoch, like a training arena: the
    second call must size and bind again, and both calls must match the oracle at the bound of tests/test_gpu_step.py's sample test."""
    from aclgan_amd import _lib as L
    cfg = O.default_config()
    cfg["display_size"] = 2
    nets = O.test_nets(cfg, 0)
    tr = _make(T, cfg, nets)
    g = torch.Generator().manual_seed(37)
    x_a = torch.rand(2, 3, 256, 256, generator=g) * 2 - 1
    x_b = torch.rand(2, 3, 256, 256, generator=g) * 2 - 1

    def fwd_bytes():
        v = C.c_size_t()
        L.check(L.lib.aclgan_forward_workspace_bytes(tr._ctx, 1, 256, 256, C.byref(v)), "forward_workspace_bytes")
        return v.value

    def rel(a, b):
        a = a.detach().double().cpu(); b = b.detach().double().cpu()
        return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()

    want = None
    prev = C.c_int()
    before = fwd_bytes()
    outs = [tr.sample(x_a, x_b)]
    assert tr._ws_shape[3] is False and tr._ws.numel() >= before
    L.check(L.lib.aclgan_tuning(b"wino_fused", 2, C.byref(prev)), "tuning")
    try:
        after = fwd_bytes()
        print("forward-only workspace @256x256 B=1: %d bytes, %d with wino_fused = 2" % (before, after))
        assert after > before, (before, after)
        outs.append(tr.sample(x_a, x_b))
        torch.cuda.synchronize()
        assert tr._ws.numel() >= after
    finally:
        L.check(L.lib.aclgan_tuning(b"wino_fused", prev.value, None), "tuning")
    want = _sample_oracle(nets, cfg, x_a, tr.z_1.cpu(), tr.z_2.cpu(), tr.z_3.cpu())
    for run, out in enumerate(outs):
        errs = [rel(got, w) for got, w in zip(out, want)]
        print("sample() run %d max-abs rel errors vs the oracle:" % run, ["%.2e" % e for e in errs])
        assert max(errs) < 1e-3, (run, errs)


def test_forward_workspace_does_not_depend_on_the_mode(T):
    """the forward-only arena (trainer._ensure_workspace(forward_only=True), what sample() binds) is cached per tuning epoch, and
    aclgan_set_deterministic does not start a new epoch -- so a mode change must not change what a forward needs.  It does not: the forward
    kernels' scratch (split-K partials, Winograd and sub-pixel buffers, 16-bit merged filters) is sized for the default plan's largest need
    whatever the mode.  Pinned at the five single-GPU workloads bench.py times, at their batch and at sample()'s B = 1"""
    from aclgan_amd import _lib as L
    from gpu_util import deterministic_mode
    from test_gpu_launch_shapes import WORKLOADS, _config
    for wl, yaml_name, S, dt, B in WORKLOADS:
        tr = T.aclgan_Trainer(_config(yaml_name), compute_dtype=dt)
        need = {}
        for det in (False, True):
            with deterministic_mode(L, det):
                for b in (1, B):
                    v = C.c_size_t()
                    L.check(L.lib.aclgan_forward_workspace_bytes(tr._ctx, b, S, S, C.byref(v)), "forward_workspace_bytes")
                    need[(det, b)] = v.value
        print("%s forward-only workspace, default / deterministic: B=1 %d / %d bytes, B=%d %d / %d bytes"
              % (wl, need[(False, 1)], need[(True, 1)], B, need[(False, B)], need[(True, B)]))
        for b in (1, B):
            assert need[(False, b)] > 0 and need[(False, b)] == need[(True, b)], (wl, b, need)
        del tr


# 16-bit: bounds per network group <= 2x the measured value, masks and signs frozen, against the emulated contract.  Measured (round 6,
# profiles/r06_experiments.md): bf16 dis 7.8e-3, gen.dec 1.82e-2, gen.enc 1.63e-2 (un-frozen: 5.6e-2 / 1.96e-1); fp16 dis 9.2e-4, gen.dec
# 2.4e-3, gen.enc 2.2e-3 (un-frozen: 2.0e-2 / 7.0e-2) -- what remains is the rounding-flip noise of the 16-bit values themselves
# (tests/test_gpu_step16.py docstring), 10x below the un-frozen figures the round-5 bounds (3e-1 / 1.2e-1) had to admit.
ETOL_FROZEN = {
    "bf16": {"dis": 1.5e-2, "gen.dec": 3e-2, "gen.enc": 3e-2},
    "fp16": {"dis": 2e-3, "gen.dec": 5e-3, "gen.enc": 5e-3},
}


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_backward_parity_with_frozen_masks_16bit(T, dt):
    """the same construction for the 16-bit paths against the emulated contract (128x128 B=2 as tests/test_gpu_step16.py::test_step_gradients_16bit):
    with the masks frozen the remaining distance is rounding-flip noise of the 16-bit values themselves, held per network."""
    res = _frozen_and_free(T, dt, 2, 128, 32)
    worst = {}
    for which in ("dis", "gen"):
        for key, e in _per_net(res[which]["frozen"]).items():
            kk = "dis" if key.startswith("dis") else "gen" + key[key.index("."):]
            worst[kk] = max(worst.get(kk, 0.0), e)
    print("%s frozen-mask worst per network group:" % dt, {k: "%.2e" % v for k, v in worst.items()})
    bad = {k: v for k, v in worst.items() if v > ETOL_FROZEN[dt][k]}
    assert not bad, bad


# the benchmarked 16-bit batches (bench.py: bf16 256x256 B=8, fp16 256x256 B=32), built from D_SAMPLES distinct samples.  Per network group
# worst relative L2 against the emulated contract, bounds <= 2x the value measured on the MI355X and never above ETOL_FROZEN.  Measured:
#   bf16 B=8   dis 3.64e-3, gen.enc 1.58e-2, gen.dec 1.50e-2 (p99 over the generator's tensors 1.57e-2, mean 6.3e-3)
#   fp16 B=32  dis 4.49e-4, gen.enc 2.45e-3, gen.dec 2.36e-3 (p99 2.43e-3, mean 1.0e-3)
# bf16 gen sits at half of ETOL_FROZEN, as the 128x128 B=2 case does (1.63e-2 / 1.82e-2 above): the rounding-flip noise floor of the
# 8-bit mantissa, spread evenly over the generator's tensors rather than on one layer.  Two CPU emulations of the same contract that differ
# only in fp32 summation order already drift apart by 1.8e-3 at 1/4 width (tests/test_oracle_repeat_batch_cpu.py::RTOL_16).  2x the
# bf16 generator figures would exceed ETOL_FROZEN, so those two bounds are ETOL_FROZEN itself.
ETOL_FROZEN_BATCH = {
    "bf16": {"dis": 7e-3, "gen.dec": 3e-2, "gen.enc": 3e-2},
    "fp16": {"dis": 9e-4, "gen.dec": 4.7e-3, "gen.enc": 4.9e-3},
}
COPY_DISAGREE = {"bf16": 0, "fp16": 0}      # mask / sign elements where a copy of a sample differs from its copies' majority (measured: none)


@pytest.mark.parametrize("dt,B", [("bf16", 8), ("fp16", 32)], ids=["bf16_b8", "fp16_b32"])
def test_backward_parity_with_frozen_masks_16bit_benchmarked_batch(T, dt, B):
    """256x256 at the benchmarked per-GPU batch, full width, default paths, lanes and mode: the split-M / split-K plans, the storage codes
    between layers, the fold / finish kernels and the discriminators' joint batches (2B, 3B) that bench.py times.  The batch is D_SAMPLES = 4
    distinct samples, each B / 4 times in a fixed non-periodic arrangement, and the oracle runs the four alone with focus_delta and the loss
    scale rescaled (tests/test_oracle_repeat_batch_cpu.py proves that identity).  The copies of a sample must record the same masks -- the
    forward does not depend on where a sample sits in the batch -- and with those masks frozen every network group stays within
    ETOL_FROZEN_BATCH; fp16: neither update overflowed, the scale is 65536 and the one update counts as clean."""
    from test_oracle_repeat_batch_cpu import D_SAMPLES
    cap = _mask_capture_bytes(T, B, 256, 34, dt)
    res = _frozen_and_free(T, dt, B, 256, 34, cap_bytes=cap, d=D_SAMPLES)
    worst, ndis = {}, 0
    for which in ("dis", "gen"):
        r = res[which]
        assert r["matched"] >= (0.3 if which == "dis" else 0.9) * r["acts"], (which, r["matched"], r["acts"], r["unmatched"][:6])
        ndis += sum(n for *_, n in r["disagree"])
        for key, e in _per_net(r["frozen"]).items():
            kk = "dis" if key.startswith("dis") else "gen" + key[key.index("."):]
            worst[kk] = max(worst.get(kk, 0.0), e)
    print("%s B=%d frozen-mask worst per network group:" % (dt, B), {k: "%.2e" % v for k, v in worst.items()},
          "copy-disagreeing mask elements: %d" % ndis)
    assert ndis <= COPY_DISAGREE[dt], (ndis, res["dis"]["disagree"][:8], res["gen"]["disagree"][:8])
    bad = {k: v for k, v in worst.items() if v > min(ETOL_FROZEN_BATCH[dt][k], ETOL_FROZEN[dt][k])}
    assert not bad, bad


# Deterministic mode (aclgan_set_deterministic) at the benchmarked batches: the ordered plan -- padded-grid input gradients and folds, the
# Winograd ring on a zeroed grid, per-slice weight-gradient copies, ordered bias column sums, no split-K -- through the same construction, the
# same bounds (1e-3 fp32, ETOL_FROZEN_BATCH 16-bit), the oracle under the contract that plan computes.  A second update from the same state
# must give the same bits.  The fp32 case skips the masks-free oracle gradients (not asserted here; the default-mode case prints them): its
# oracle masks come from the forward-only loss graph.  (bf16 B=8 is left to the default-mode case above: the suite's time budget.)
@pytest.mark.parametrize("dt,B", [(None, 8), ("fp16", 32)], ids=["fp32_b8", "fp16_b32"])
def test_backward_parity_with_frozen_masks_deterministic_benchmarked_batch(T, dt, B):
    from aclgan_amd import _lib as L
    from gpu_util import deterministic_mode
    from test_oracle_repeat_batch_cpu import D_SAMPLES
    with deterministic_mode(L, True):
        if dt is None:
            cap = _mask_capture_bytes(T, 8, 256, 33)
            res = _frozen_and_free(T, None, 8, 256, 33, cap_bytes=cap, rerun=True, free=False)
        else:
            cap = _mask_capture_bytes(T, B, 256, 34, dt)
            res = _frozen_and_free(T, dt, B, 256, 34, cap_bytes=cap, d=D_SAMPLES, rerun=True)
    worst, ndis = {}, 0
    for which in ("dis", "gen"):
        r = res[which]
        assert r["matched"] >= (0.3 if which == "dis" else 0.9) * r["acts"], (which, r["matched"], r["acts"], r["unmatched"][:6])
        assert not r["rerun_differ"], (which, "a second deterministic update gave other bits", r["rerun_differ"][:8])
        ndis += sum(n for *_, n in r["disagree"])
        for key, e in _per_net(r["frozen"]).items():
            kk = "dis" if key.startswith("dis") else "gen" + key[key.index("."):]
            worst[kk] = max(worst.get(kk, 0.0), e)
    print("deterministic %s B=%d frozen-mask worst per network group:" % (dt or "fp32", B), {k: "%.2e" % v for k, v in worst.items()},
          "copy-disagreeing mask elements: %d" % ndis)
    if dt is None:
        for which in ("dis", "gen"):
            assert res[which]["frozen"][0][0] <= 1e-3, (which, res[which]["frozen"][:6])
    else:
        assert ndis <= COPY_DISAGREE[dt], (ndis, res["dis"]["disagree"][:8], res["gen"]["disagree"][:8])
        bad = {k: v for k, v in worst.items() if v > min(ETOL_FROZEN_BATCH[dt][k], ETOL_FROZEN[dt][k])}
        assert not bad, bad
