"""What the R1 gradient penalty (config keys r1_gamma / r1_every; aclgan_dis_r1) costs at 256x256, B=8 (male2female config, full width).
    pass      one aclgan_dis_r1 call per discriminator (dis_A, dis_B; stream events), on an fp32 and on a bf16 context -- the pass itself is
              fp32 in both -- next to one eager dis_update (zero_grad, update, Adam) of the same trainer with the key off
    step      one dis_update + gen_update in ms, fp32 and bf16, with the key off, with r1_every 1 and with r1_every 16 (16 steps per
              timing, so that every timing holds one pass): six trainers, timed in turn
    copy      a device-to-device hipMemcpyAsync of the largest activation of the pass (the first conv block's output): the yardstick for
              the streaming kernels
    kernels   (--kernel-trace FILE: the *_kernel_trace.csv of `rocprofv3 --kernel-trace -- python scripts/bench_r1.py --pass-only 20`)
              time per pass of each new streaming kernel against the bytes it moves (inputs read once, outputs written once) at the copy's rate
Every figure is the median over `--rounds` alternating rounds (range given too).  One JSON line on stdout; --out writes it to a file."""
import argparse
import csv
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


def summary(t, scale=1.0, nd=3):
    return {"median": round(statistics.median(t) * scale, nd), "min": round(min(t) * scale, nd), "max": round(max(t) * scale, nd)}


def kernel_bytes(arch, B, S, Cin=3):
    """bytes each new streaming kernel moves in ONE pass: {kernel: bytes}"""
    out = {"r1_seed_kernel": 0, "r1_slope_mul_kernel": 0, "r1_sqnorm_kernel": 4 * B * S * S * Cin, "r1_finalize_kernel": 8 * B * S * S * Cin,
           "r1_head_part_kernel": 0}
    h = S
    for s in range(arch.dis_num_scales):
        hi, co = h, arch.dis_dim
        for l in range(1, arch.dis_n_layer + 1):
            hi = (hi + 2 - 4) // 2 + 1
            e = 4 * B * hi * hi * co
            out["r1_slope_mul_kernel"] += 3 * e * (2 if l < arch.dis_n_layer else 1)      # backward chain (not the last layer) and adjoint chain
            if l == arch.dis_n_layer:
                out["r1_seed_kernel"] += 2 * e
                out["r1_head_part_kernel"] += e
            co *= 2
        h = (h - 1) // 2 + 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=os.path.join(ROOT, "configs", "male2female.yaml"))
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10, help="passes / dis_updates per timing")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--gamma", type=float, default=10.0)
    ap.add_argument("--pass-only", type=int, default=0, help="run that many passes per discriminator and nothing else (for rocprofv3 --kernel-trace)")
    ap.add_argument("--kernel-trace", default=None, help="kernel trace CSV of a --pass-only run")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    opts = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU timing of a device path"
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib as L
    from aclgan_amd.trainer import aclgan_Trainer
    B, S = opts.batch, opts.size
    cfg = yaml.safe_load(open(opts.config))
    cfg["display_size"] = 1
    g = torch.Generator().manual_seed(0)
    x_a = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).cuda()
    x_b = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).cuda()
    st = L.stream_ptr()

    def pass_fn(tr):
        nb = max(L.lib.aclgan_dis_r1_scratch_bytes(tr._ctx, n.net_id, B, S, S) for n in (tr.dis_A, tr.dis_B))
        scratch = torch.empty(nb, dtype=torch.uint8, device="cuda")
        pen = torch.zeros(2, device="cuda")

        def run():
            for i, (net, x) in enumerate(((tr.dis_A, x_a), (tr.dis_B, x_b))):
                L.check(L.lib.aclgan_dis_r1(tr._ctx, net.net_id, L.ptr(x), B, S, S, opts.gamma, C.c_void_p(pen.data_ptr() + 4 * i), None,
                                            L.ptr(scratch), st), "dis_r1")
        return run, nb

    if opts.pass_only:
        tr = aclgan_Trainer(cfg)
        run, _ = pass_fn(tr)
        for _ in range(opts.pass_only):
            run()
        torch.cuda.synchronize()
        print(json.dumps({"passes": opts.pass_only}))
        return

    out = {"what": "r1_gamma at %dx%d B=%d" % (S, S, B), "config": os.path.basename(opts.config), "rounds": opts.rounds,
           "reps_per_timing": opts.reps, "device": torch.cuda.get_device_name(0)}
    # ---- the pass and a dis_update ----
    timed, trainers = [], {}
    for dtype in ("fp32", "bf16"):
        torch.manual_seed(1)
        tr = trainers[dtype] = aclgan_Trainer(cfg, compute_dtype=dtype)
        run, nb = pass_fn(tr)
        out.setdefault("scratch_mb", round(nb / 1e6, 1))
        timed.append((dtype + "_pass_both_nets", run))
        timed.append((dtype + "_dis_update", lambda tr=tr: tr.dis_update(x_a, x_b, cfg)))
    # ---- the copy ----
    a = trainers["fp32"].arch
    big = torch.empty(B * (S // 2) * (S // 2) * a.dis_dim, device="cuda")
    dst = torch.empty_like(big)
    hip = C.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int

    def copy():
        rc = hip.hipMemcpyAsync(dst.data_ptr(), big.data_ptr(), big.numel() * 4, 3, st)      # 3 = hipMemcpyDeviceToDevice
        assert rc == 0, rc
    timed.append(("copy", copy))
    t = {name: [] for name, _ in timed}
    for _ in range(opts.rounds):
        for name, fn in timed:
            t[name].append(events_ms(fn, 100 if name == "copy" else opts.reps, warm=2))
    out["pass_ms"] = {name: summary(t[name]) for name, _ in timed if name != "copy"}
    copy_us = summary(t["copy"], 1e3, 2)
    rate = 2 * big.numel() * 4 / (copy_us["median"] * 1e-6)
    out["copy"] = {"tensor_mb": round(big.numel() * 4 / 1e6, 2), "us": copy_us, "tb_per_s": round(rate / 1e12, 3)}
    for dtype in ("fp32", "bf16"):
        out["pass_ms"][dtype + "_pass_over_dis_update"] = round(out["pass_ms"][dtype + "_pass_both_nets"]["median"] / out["pass_ms"][dtype + "_dis_update"]["median"], 3)
    del trainers, timed

    # ---- the step ----
    if not opts.no_step:
        variants = []
        for dtype in ("fp32", "bf16"):
            for tag, keys in (("off", {}), ("every1", {"r1_gamma": opts.gamma, "r1_every": 1}), ("every16", {"r1_gamma": opts.gamma, "r1_every": 16})):
                c = dict(cfg)
                c.update(keys)
                torch.manual_seed(1)
                tr = aclgan_Trainer(c, compute_dtype=dtype)

                def step(tr=tr, c=c):
                    tr.dis_update(x_a, x_b, c)
                    tr.gen_update(x_a, x_b, c)
                variants.append(("%s_%s" % (dtype, tag), step))
        times = {name: [] for name, _ in variants}
        for _ in range(opts.rounds):
            for name, fn in variants:
                times[name].append(events_ms(fn, 16, warm=16))      # (16 + 16 steps: the phase of r1_every 16 is the same in every timing)
        out["step_ms"] = {name: summary(times[name]) for name, _ in variants}
        for dtype in ("fp32", "bf16"):
            for tag in ("every1", "every16"):
                out["step_ms"]["%s_%s_minus_off" % (dtype, tag)] = round(out["step_ms"]["%s_%s" % (dtype, tag)]["median"] - out["step_ms"][dtype + "_off"]["median"], 3)

    # ---- the streaming kernels, from a kernel trace ----
    if opts.kernel_trace:
        tot, calls = {}, {}
        with open(opts.kernel_trace) as f:
            for row in csv.DictReader(f):
                name = row["Kernel_Name"].split("(")[0].split("<")[0].replace("void ", "").replace("aclgan::", "")
                if name.startswith("r1_"):
                    tot[name] = tot.get(name, 0) + int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
                    calls[name] = calls.get(name, 0) + 1
        npass = max(1, calls.get("r1_finalize_kernel", 1))      # (finalize: one launch per aclgan_dis_r1 call)
        nbytes = kernel_bytes(a, B, S)
        ks = {}
        for name in sorted(tot):
            us = tot[name] / npass / 1e3
            r = {"us_per_call": round(us, 2), "launches_per_call": calls[name] // npass}
            if name in nbytes:
                r["mb_per_call"] = round(nbytes[name] / 1e6, 2)
                r["us_at_copy_rate"] = round(nbytes[name] / rate * 1e6, 2)
                r["over_copy"] = round(us / (nbytes[name] / rate * 1e6), 2)
            ks[name] = r
        out["kernels"] = ks
    line = json.dumps(out)
    print(line)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
