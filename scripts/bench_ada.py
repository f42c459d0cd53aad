"""What the adaptive augmentation probability (config keys dis_augment_p / ada_*; aclgan_ctx_set_ada, aclgan_augment_gate) costs at 256x256,
B=8 (male2female config, full width).
    step        one dis_update + gen_update in ms, fp32 and bf16, with `dis_augment: color,translation,cutout` alone ("off") and with
                `dis_augment_p: adaptive` added ("on")
    kernels     (--kernel-trace FILE: the *_kernel_trace.csv of `rocprofv3 --kernel-trace -- python scripts/bench_ada.py --updates-only 20`)
                time per step of augment_gate_kernel, ada_sign_kernel and ada_fold_kernel
Four trainers, timed in turn: every figure is the median over `--rounds` alternating rounds (range given too).  One JSON line on stdout;
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

KERNELS = ("augment_gate_kernel", "ada_sign_kernel", "ada_fold_kernel")
POLICY = "color,translation,cutout"


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
    ap.add_argument("--reps", type=int, default=10, help="steps per timing")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--updates-only", type=int, default=0, help="run that many fp32 dis + gen steps with the key on and nothing else (for rocprofv3 --kernel-trace)")
    ap.add_argument("--kernel-trace", default=None, help="kernel trace CSV of an --updates-only run")
    ap.add_argument("--out", default=None)
    opts = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU timing of a device path"
    import aclgan_amd  # noqa: F401
    from aclgan_amd.trainer import aclgan_Trainer
    B, S = opts.batch, opts.size
    cfg = yaml.safe_load(open(opts.config))
    cfg["display_size"] = 1
    cfg["dis_augment"] = POLICY
    on_keys = {"dis_augment_p": "adaptive"}
    g = torch.Generator().manual_seed(0)
    x_a = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).cuda()
    x_b = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).cuda()

    if opts.updates_only:
        c = dict(cfg, **on_keys)
        tr = aclgan_Trainer(c)
        for _ in range(opts.updates_only):
            tr.dis_update(x_a, x_b, c)
            tr.gen_update(x_a, x_b, c)
        torch.cuda.synchronize()
        print(json.dumps({"steps": opts.updates_only, "ada_state": tr.ada_state()}))
        return

    out = {"what": "dis_augment_p: adaptive at %dx%d B=%d" % (S, S, B), "config": os.path.basename(opts.config), "dis_augment": POLICY,
           "rounds": opts.rounds, "reps_per_timing": opts.reps, "device": torch.cuda.get_device_name(0)}
    variants, trainers = [], {}
    for dtype in ("fp32", "bf16"):
        for tag, keys in (("off", {}), ("on", on_keys)):
            c = dict(cfg, **keys)
            torch.manual_seed(1)
            tr = aclgan_Trainer(c, compute_dtype=dtype)
            trainers["%s_%s" % (dtype, tag)] = tr

            def fn(tr=tr, c=c):
                tr.dis_update(x_a, x_b, c)
                tr.gen_update(x_a, x_b, c)
            variants.append(("%s_%s" % (dtype, tag), fn))
    times = {name: [] for name, _ in variants}
    for _ in range(opts.rounds):
        for name, fn in variants:
            times[name].append(events_ms(fn, opts.reps, warm=3))
    r = {name: summary(times[name]) for name, _ in variants}
    for dtype in ("fp32", "bf16"):
        r[dtype + "_on_minus_off"] = round(r[dtype + "_on"]["median"] - r[dtype + "_off"]["median"], 3)
        r[dtype + "_ranges_overlap"] = r[dtype + "_on"]["min"] <= r[dtype + "_off"]["max"] and r[dtype + "_off"]["min"] <= r[dtype + "_on"]["max"]
    out["step_ms"] = r
    out["ada_state_after"] = {k: tr.ada_state() for k, tr in trainers.items() if k.endswith("_on")}

    if opts.kernel_trace:
        dur = {}
        with open(opts.kernel_trace) as f:
            for row in csv.DictReader(f):
                name = row["Kernel_Name"].split("(")[0].split("<")[0].replace("void ", "").replace("aclgan::", "")
                if name in KERNELS:
                    dur.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
        nstep = max(1, len(dur.get("ada_fold_kernel", [0])))      # (the fold: one launch per dis_update, so per step)
        # (mean and median both: a few launches many times the median carry most of a single-workgroup kernel's total)
        out["kernels"] = {name: {"us_per_step": round(sum(v) / nstep, 2), "launches_per_step": round(len(v) / nstep, 2),
                                 "us_per_launch_mean": round(sum(v) / len(v), 2), "us_per_launch": summary(v, nd=2)} for name, v in sorted(dur.items())}
    line = json.dumps(out)
    print(line)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
