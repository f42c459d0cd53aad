"""What the gradient-norm stage (grad_clip / aclgan_bind_grad_clip) costs, at the full-width GEN and DIS groups of the male2female config.
Per group, over the same flat buffers, each figure the time of one call from stream events around `--reps` back-to-back calls:
    copy             a device-to-device copy of the gradient buffer (4 B read + 4 B written per parameter): the rate the bytes are held against
    norm             aclgan_grad_clip_flat: gradnorm_part_kernel + gradnorm_finish_kernel (4 B / parameter read)
    adam_fp32        aclgan_adam_step without a state (adam_kernel)                 adam_fp32_clip   with one: part, finish, adam_kernel<CLIP>
    adam_fp16        aclgan_adam_step under a loss scale: grad_check_kernel, adam_kernel<SCALED>, scale_update_kernel
    adam_fp16_clip   the same with a state: part, finish, adam_kernel<SCALED, CLIP>, scale_update_kernel
adam_fp16_clip - adam_fp16 is the norm stage against the scan it replaces (part + finish - grad_check_kernel): the other two launches are
the same work.  The variants are measured in turn, `--rounds` times; reported: median and range over the rounds.
--step: one dis + gen step of the trainer at 256x256, B = 8, fp32 and bf16, grad_clip off against grad_clip: .inf.
One JSON line on stdout; --out writes the same line to a file."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def events_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def summary(t, scale=1.0, nd=2):
    return {"median": round(statistics.median(t) * scale, nd), "min": round(min(t) * scale, nd), "max": round(max(t) * scale, nd)}


def overlap(a, b):
    return a["min"] <= b["max"] and b["min"] <= a["max"]


def group_variants(L, ctx, grp, n, cfg):
    gen = torch.Generator(device="cuda").manual_seed(grp)
    p = torch.randn(n, device="cuda", generator=gen) * 0.05
    g = torch.randn(n, device="cuda", generator=gen) * 1e-3
    m, v, tmp = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), torch.empty(n, device="cuda")
    clip = torch.zeros(L.lib.aclgan_grad_clip_state_floats(), device="cuda")
    scale = torch.tensor([1.0, 1.0, 0, 0, 0, 0, 1e9, 0], device="cuda")      # S = 1: the same buffer serves both paths
    L.check(L.lib.aclgan_bind_params(ctx, grp, L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v)), "bind_params")
    adam = L.Adam(float(cfg["lr"]), float(cfg["beta1"]), float(cfg["beta2"]), 1e-8, float(cfg["weight_decay"]))
    st = L.stream_ptr()
    inf = float("inf")

    def step(scaled, clipped):
        def fn():
            L.check(L.lib.aclgan_bind_loss_scale(ctx, L.ptr(scale) if scaled else None), "bind_loss_scale")
            L.check(L.lib.aclgan_bind_grad_clip(ctx, grp, inf, L.ptr(clip) if clipped else None), "bind_grad_clip")
            L.check(L.lib.aclgan_adam_step(ctx, grp, C.byref(adam), 1000, st), "adam_step")
        return fn

    def norm():
        L.check(L.lib.aclgan_grad_clip_flat(L.ptr(g), n, inf, L.ptr(clip), st), "grad_clip_flat")

    keep = (p, g, m, v, tmp, clip, scale)
    return keep, [("copy", lambda: tmp.copy_(g)), ("norm", norm), ("adam_fp32", step(False, False)), ("adam_fp32_clip", step(False, True)),
                  ("adam_fp16", step(True, False)), ("adam_fp16_clip", step(True, True))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=os.path.join(ROOT, "configs", "male2female.yaml"))
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step", action="store_true", help="also time one dis + gen step of the trainer with the key off and on")
    ap.add_argument("--step-reps", type=int, default=10)
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    opts = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU timing of a device path"
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib as L
    from aclgan_amd.trainer import aclgan_Trainer, arch_from_config
    cfg = yaml.safe_load(open(opts.config))
    out = {"what": "gradient norm stage and clipped Adam, per call", "config": os.path.basename(opts.config), "reps": opts.reps,
           "rounds": opts.rounds, "device": torch.cuda.get_device_name(0)}
    ctx = C.c_void_p()
    L.check(L.lib.aclgan_ctx_create(C.byref(arch_from_config(cfg)), C.byref(ctx)), "ctx_create")
    for grp, gname in ((L.GROUP_GEN, "gen"), (L.GROUP_DIS, "dis")):
        n = L.lib.aclgan_group_numel(ctx, grp)
        keep, variants = group_variants(L, ctx, grp, n, cfg)
        times = {name: [] for name, _ in variants}
        for _ in range(opts.rounds):
            for name, fn in variants:
                times[name].append(events_ms(fn, opts.reps))
        assert bool(torch.isfinite(keep[0]).all())
        r = {name: summary(times[name], 1e3) for name, _ in variants}      # microseconds
        spread = max(x["max"] - x["min"] for x in r.values())
        copy_rate = 8.0 * n / (r["copy"]["median"] * 1e-6)      # bytes moved per second by the copy
        r.update(numel=n, gradient_bytes=4 * n, copy_tb_per_s=round(copy_rate / 1e12, 3),
                 norm_us_at_the_copy_rate=round(4.0 * n / copy_rate * 1e6, 2),
                 norm_tb_per_s_at_median=round(4.0 * n / (r["norm"]["median"] * 1e-6) / 1e12, 3),
                 norm_stage_minus_scan_us=round(r["adam_fp16_clip"]["median"] - r["adam_fp16"]["median"], 2),
                 fp16_ranges_overlap=overlap(r["adam_fp16_clip"], r["adam_fp16"]),
                 adam_fp32_clip_minus_adam_fp32_us=round(r["adam_fp32_clip"]["median"] - r["adam_fp32"]["median"], 2),
                 largest_round_to_round_spread_us=round(spread, 2))
        out[gname] = r
        del keep, variants
    L.lib.aclgan_ctx_destroy(ctx)

    if opts.step:
        B, S = 8, 256
        c0 = dict(cfg, display_size=1)
        g = torch.Generator().manual_seed(0)
        x_a = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).cuda()
        x_b = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).cuda()
        variants = []
        for dtype in ("fp32", "bf16"):
            for tag, keys in (("off", {}), ("on", {"grad_clip": float("inf")})):
                c = dict(c0, **keys)
                torch.manual_seed(1)
                tr = aclgan_Trainer(c, compute_dtype=dtype)

                def fn(tr=tr, c=c):
                    tr.dis_update(x_a, x_b, c)
                    tr.gen_update(x_a, x_b, c)
                variants.append(("%s_%s" % (dtype, tag), fn, tr))
        times = {name: [] for name, _, _ in variants}
        for _ in range(opts.step_rounds):
            for name, fn, _ in variants:
                times[name].append(events_ms(fn, opts.step_reps))
        r = {name: summary(times[name], 1.0, 3) for name, _, _ in variants}      # milliseconds
        for dtype in ("fp32", "bf16"):
            r[dtype + "_on_minus_off"] = round(r[dtype + "_on"]["median"] - r[dtype + "_off"]["median"], 3)
            r[dtype + "_ranges_overlap"] = overlap(r[dtype + "_on"], r[dtype + "_off"])
        r["grad_clip_state"] = {name: tr.grad_clip_state() for name, _, tr in variants if name.endswith("_on")}
        out["step_ms_256_b8"] = r
    line = json.dumps(out)
    print(line)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
