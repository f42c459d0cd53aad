"""What the mode-seeking regulariser (config key ms_lambda; aclgan_ctx_set_modeseek) costs at 256x256, B=8 (male2female config, full width).
    gen_update  one eager gen_update (zero_grad, update, Adam) in ms, fp32 and bf16, with the key off and on
    step        one dis_update + gen_update in ms, the same four variants
    operator    aclgan_modeseek (part + grad, accumulating into both gradients) on one direction's tensors, B x 3 x S x S fp32, against a
                device-to-device copy of one such tensor timed in the same rounds.  The two launches move 8 tensors' worth of bytes (I, I' read
                twice; dI, dI' read and written), the copy 2: `copy_rate_us` is those bytes at the copy's rate
    kernels     (--kernel-trace FILE: the *_kernel_trace.csv of `rocprofv3 --kernel-trace -- python scripts/bench_modeseek.py --updates-only 20`)
                time per launch of modeseek_part_kernel / modeseek_grad_kernel inside a gen_update and the queues they ran on
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

KERNELS = ("modeseek_part_kernel", "modeseek_grad_kernel")


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
    ap.add_argument("--lam", type=float, default=1.0)
    ap.add_argument("--updates-only", type=int, default=0, help="run that many fp32 gen_updates with the key on and nothing else (for rocprofv3 --kernel-trace)")
    ap.add_argument("--kernel-trace", default=None, help="kernel trace CSV of an --updates-only run")
    ap.add_argument("--out", default=None)
    opts = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU timing of a device path"
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib as L
    from aclgan_amd.trainer import aclgan_Trainer
    B, S = opts.batch, opts.size
    cfg = yaml.safe_load(open(opts.config))
    cfg["display_size"] = 1
    on_keys = {"ms_lambda": opts.lam}
    g = torch.Generator().manual_seed(0)
    x_a = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).cuda()
    x_b = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).cuda()

    if opts.updates_only:
        c = dict(cfg, **on_keys)
        tr = aclgan_Trainer(c)
        for _ in range(opts.updates_only):
            tr.gen_update(x_a, x_b, c)
        torch.cuda.synchronize()
        print(json.dumps({"gen_updates": opts.updates_only}))
        return

    out = {"what": "ms_lambda at %dx%d B=%d" % (S, S, B), "config": os.path.basename(opts.config), "rounds": opts.rounds,
           "reps_per_timing": opts.reps, "ms_lambda": opts.lam, "device": torch.cuda.get_device_name(0)}
    variants = []
    for dtype in ("fp32", "bf16"):
        for tag, keys in (("off", {}), ("on", on_keys)):
            c = dict(cfg, **keys)
            for what in ("gen_update", "step"):
                torch.manual_seed(1)
                tr = aclgan_Trainer(c, compute_dtype=dtype)

                def fn(tr=tr, c=c, what=what):
                    if what == "step":
                        tr.dis_update(x_a, x_b, c)
                    tr.gen_update(x_a, x_b, c)
                variants.append(("%s_%s_%s" % (what, dtype, tag), fn))
    # the operator on one direction's tensors, and the copy it is measured against
    n = 3 * S * S
    a, b = x_a.reshape(B, n).clone(), x_b.reshape(B, n).clone()
    da, db, dst = torch.zeros(B, n, device="cuda"), torch.zeros(B, n, device="cuda"), torch.empty(B, n, device="cuda")
    u, u2 = torch.randn(B, 8, generator=g).cuda(), torch.randn(B, 8, generator=g).cuda()
    out4 = torch.zeros(4, device="cuda")
    scratch = torch.zeros(L.lib.aclgan_modeseek_scratch_bytes(B, n) // 4, device="cuda")
    st = L.stream_ptr()

    def op():
        L.check(L.lib.aclgan_modeseek(L.ptr(a), L.ptr(b), B, n, L.ptr(u), L.ptr(u2), 8, 1.0, 1e-6 / B, None, L.ptr(out4), L.ptr(da), L.ptr(db), 1, L.ptr(scratch), st))
    variants += [("operator", op), ("copy", lambda: dst.copy_(a))]
    times = {name: [] for name, _ in variants}
    for _ in range(opts.rounds):
        for name, fn in variants:
            times[name].append(events_ms(fn, 200 if name in ("operator", "copy") else opts.reps, warm=3))
    for what in ("gen_update", "step"):
        r = {name[len(what) + 1:]: summary(times[name]) for name, _ in variants if name.startswith(what + "_")}
        for dtype in ("fp32", "bf16"):
            r[dtype + "_on_minus_off"] = round(r[dtype + "_on"]["median"] - r[dtype + "_off"]["median"], 3)
            r[dtype + "_ranges_overlap"] = r[dtype + "_on"]["min"] <= r[dtype + "_off"]["max"] and r[dtype + "_off"]["min"] <= r[dtype + "_on"]["max"]
        out[what + "_ms"] = r
    op_us, copy_us = summary(times["operator"], 1e3, 2), summary(times["copy"], 1e3, 2)
    out["operator"] = {"tensor_bytes": 4 * B * n, "part_plus_grad_us": op_us, "copy_us": copy_us, "tensors_moved": 8,
                       "copy_rate_us": round(copy_us["median"] * 4, 2), "copy_rate_over_measured": round(copy_us["median"] * 4 / op_us["median"], 3),
                       "copy_TB_per_s": round(2 * 4 * B * n / copy_us["median"] / 1e6, 2)}

    if opts.kernel_trace:
        tot, calls, queues = {}, {}, {}
        with open(opts.kernel_trace) as f:
            for row in csv.DictReader(f):
                name = row["Kernel_Name"].split("(")[0].split("<")[0].replace("void ", "").replace("aclgan::", "")
                if name in KERNELS:
                    tot[name] = tot.get(name, 0) + int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
                    calls[name] = calls.get(name, 0) + 1
                    q = row.get("Queue_Id", "?")
                    queues.setdefault(name, {})
                    queues[name][q] = queues[name].get(q, 0) + 1
        out["kernels"] = {name: {"us_per_launch": round(tot[name] / calls[name] / 1e3, 2), "launches": calls[name], "launches_by_queue": queues[name]}
                          for name in sorted(tot)}
    line = json.dumps(out)
    print(line)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
