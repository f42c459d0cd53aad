"""What the averaged generator costs per generator update (male2female config: the full-width generator group, 30 058 648 floats).
Three ways to run the generator's Adam launch, over the same flat buffers:
    adam            aclgan_adam_flat: p, g, m, v read, p, m, v written (28 B / parameter) -- a run without ema_decay
    adam_ema        aclgan_adam_flat_ema, blend mode: the average read and written by the same launch (36 B / parameter)
    adam_then_lerp  aclgan_adam_flat followed by torch.Tensor.lerp_ over the average and p (28 + 12 B / parameter): what the fusion replaces
Each figure is the time of one update from stream events around `--reps` back-to-back updates, after a warm-up; the three are measured in
turn, `--rounds` times, so that whatever else the machine is doing lands on all of them alike.  Reported: the median and the range over
the rounds, and bytes / median.  One JSON line on stdout; --out writes the same line to a file."""
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


def events_ms(fn, reps, warm=5):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=os.path.join(ROOT, "configs", "male2female.yaml"))
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--decay", type=float, default=0.999)
    ap.add_argument("--out", default=None)
    opts = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU timing of a device path"
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib as L
    from aclgan_amd.trainer import arch_from_config
    cfg = yaml.safe_load(open(opts.config))
    ctx = C.c_void_p()
    L.check(L.lib.aclgan_ctx_create(C.byref(arch_from_config(cfg)), C.byref(ctx)), "ctx_create")
    n = L.lib.aclgan_group_numel(ctx, L.GROUP_GEN)
    L.lib.aclgan_ctx_destroy(ctx)
    gen = torch.Generator(device="cuda").manual_seed(0)
    p = torch.randn(n, device="cuda", generator=gen) * 0.05
    g = torch.randn(n, device="cuda", generator=gen) * 1e-3
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    ema = p.clone()
    adam = L.Adam(float(cfg["lr"]), float(cfg["beta1"]), float(cfg["beta2"]), 1e-8, float(cfg["weight_decay"]))
    st = L.stream_ptr()
    step = 1000      # (a fixed bias correction: the time does not depend on it, and the buffers stay finite over any number of repetitions)

    def adam_only():
        L.check(L.lib.aclgan_adam_flat(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), n, C.byref(adam), step, st), "adam_flat")

    def adam_ema():
        L.check(L.lib.aclgan_adam_flat_ema(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), L.ptr(ema), n, C.byref(adam), step, opts.decay, L.EMA_BLEND, st), "adam_flat_ema")

    def adam_then_lerp():
        adam_only()
        ema.lerp_(p, 1.0 - opts.decay)

    variants = (("adam", adam_only, 28), ("adam_ema", adam_ema, 36), ("adam_then_lerp", adam_then_lerp, 40))
    times = {name: [] for name, _, _ in variants}
    for _ in range(opts.rounds):
        for name, fn, _ in variants:
            times[name].append(events_ms(fn, opts.reps))
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(ema).all())
    out = {"what": "generator Adam launch, per update", "config": os.path.basename(opts.config), "numel": n, "decay": opts.decay,
           "reps": opts.reps, "rounds": opts.rounds, "device": torch.cuda.get_device_name(0)}
    for name, _, nbytes in variants:
        t = times[name]
        med = statistics.median(t)
        out[name] = {"median_us": round(med * 1e3, 2), "min_us": round(min(t) * 1e3, 2), "max_us": round(max(t) * 1e3, 2),
                     "bytes_per_parameter": nbytes, "tb_per_s_at_median": round(nbytes * n / (med * 1e-3) / 1e12, 3)}
    out["adam_ema_over_adam"] = round(out["adam_ema"]["median_us"] / out["adam"]["median_us"], 4)
    out["adam_ema_over_adam_by_bytes"] = round(36 / 28, 4)
    out["adam_ema_over_adam_then_lerp"] = round(out["adam_ema"]["median_us"] / out["adam_then_lerp"]["median_us"], 4)
    # the fused launch is "not slower" when its slowest round is no slower than the separate pair's fastest, or at least the medians say so
    out["fused_not_slower_than_separate"] = out["adam_ema"]["median_us"] <= out["adam_then_lerp"]["median_us"]
    out["fused_max_below_separate_min"] = out["adam_ema"]["max_us"] <= out["adam_then_lerp"]["min_us"]
    line = json.dumps(out)
    print(line)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
