"""What the LeCam regulariser (config keys lecam_lambda / lecam_decay / lecam_start; aclgan_ctx_set_lecam) costs at 256x256, B=8
(male2female config, full width).
    dis_update  one eager dis_update (zero_grad, update, Adam) in ms, fp32 and bf16, with the key off and on (lecam_start 0: the term acts)
    step        one dis_update + gen_update in ms, the same four variants
    kernels     (--kernel-trace FILE: the *_kernel_trace.csv of `rocprofv3 --kernel-trace -- python scripts/bench_lecam.py --updates-only 20`)
                time per dis_update of lsgan_batch_kernel (key off), lsgan_lecam_batch_kernel and lecam_fold_kernel (key on)
Eight trainers, timed in turn: every figure is the median over `--rounds` alternating rounds (range given too).  One JSON line on stdout;
--out writes it to a file."""
import argparse
import csv
import json
import os
import statistics
import sys

import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("lsgan_batch_kernel", "lsgan_lecam_batch_kernel", "lecam_fold_kernel")


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


def summary(t, scale=1.0, nd=3):
    return {"median": round(statistics.median(t) * scale, nd), "min": round(min(t) * scale, nd), "max": round(max(t) * scale, nd)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=os.path.join(ROOT, "configs", "male2female.yaml"))
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10, help="updates / steps per timing")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lam", type=float, default=0.3)
    ap.add_argument("--updates-only", type=int, default=0, help="run that many fp32 dis_updates with the key off, then on, and nothing else (for rocprofv3 --kernel-trace)")
    ap.add_argument("--kernel-trace", default=None, help="kernel trace CSV of an --updates-only run")
    ap.add_argument("--out", default=None)
    opts = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU timing of a device path"
    import aclgan_amd  # noqa: F401
    from aclgan_amd.trainer import aclgan_Trainer
    B, S = opts.batch, opts.size
    cfg = yaml.safe_load(open(opts.config))
    cfg["display_size"] = 1
    on_keys = {"lecam_lambda": opts.lam, "lecam_start": 0}
    g = torch.Generator().manual_seed(0)
    x_a = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).cuda()
    x_b = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).cuda()

    if opts.updates_only:
        for keys in ({}, on_keys):
            c = dict(cfg, **keys)
            tr = aclgan_Trainer(c)
            for _ in range(opts.updates_only):
                tr.dis_update(x_a, x_b, c)
            torch.cuda.synchronize()
        print(json.dumps({"dis_updates_per_variant": opts.updates_only}))
        return

    out = {"what": "lecam_lambda at %dx%d B=%d" % (S, S, B), "config": os.path.basename(opts.config), "rounds": opts.rounds,
           "reps_per_timing": opts.reps, "lecam_lambda": opts.lam, "device": torch.cuda.get_device_name(0)}
    variants = []
    for dtype in ("fp32", "bf16"):
        for tag, keys in (("off", {}), ("on", on_keys)):
            c = dict(cfg, **keys)
            for what in ("dis_update", "step"):
                torch.manual_seed(1)
                tr = aclgan_Trainer(c, compute_dtype=dtype)

                def fn(tr=tr, c=c, what=what):
                    tr.dis_update(x_a, x_b, c)
                    if what == "step":
                        tr.gen_update(x_a, x_b, c)
                variants.append(("%s_%s_%s" % (what, dtype, tag), fn))
    times = {name: [] for name, _ in variants}
    for _ in range(opts.rounds):
        for name, fn in variants:
            times[name].append(events_ms(fn, opts.reps, warm=3))
    for what in ("dis_update", "step"):
        r = {name[len(what) + 1:]: summary(times[name]) for name, _ in variants if name.startswith(what + "_")}
        for dtype in ("fp32", "bf16"):
            r[dtype + "_on_minus_off"] = round(r[dtype + "_on"]["median"] - r[dtype + "_off"]["median"], 3)
            r[dtype + "_ranges_overlap"] = r[dtype + "_on"]["min"] <= r[dtype + "_off"]["max"] and r[dtype + "_off"]["min"] <= r[dtype + "_on"]["max"]
        out[what + "_ms"] = r

    if opts.kernel_trace:
        tot, calls = {}, {}
        with open(opts.kernel_trace) as f:
            for row in csv.DictReader(f):
                name = row["Kernel_Name"].split("(")[0].split("<")[0].replace("void ", "").replace("aclgan::", "")
                if name in KERNELS:
                    tot[name] = tot.get(name, 0) + int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
                    calls[name] = calls.get(name, 0) + 1
        nupd = max(1, calls.get("lecam_fold_kernel", 1))      # (the fold: one launch per key-on dis_update; the trace holds as many key-off ones)
        out["kernels"] = {name: {"us_per_dis_update": round(tot[name] / nupd / 1e3, 2), "launches_per_dis_update": round(calls[name] / nupd, 2),
                                 "us_per_launch": round(tot[name] / calls[name] / 1e3, 2)} for name in sorted(tot)}
    line = json.dumps(out)
    print(line)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
