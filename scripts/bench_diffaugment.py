"""What differentiable augmentation of the discriminator inputs (config key dis_augment) costs at 256x256, B=8 (male2female config, full width).
    step      one dis_update + gen_update in ms, fp32 and bf16, with the key off and with color,translation,cutout (fresh rows every
              update, drawn and uploaded by the trainer as in a training run): four trainers, timed in turn
    operator  aclgan_diffaugment_fwd / _bwd alone at the step's shapes (N=16 C=3: the joint dis_A batch of gen_update; N=16 C=6: the joint
              pair batch), policy 7 and policy 6 (no colour: one launch), with stream events
    copy      a device-to-device hipMemcpyAsync of the same tensor, timed in the same rounds: it moves the bytes the apply kernel moves
              (one read, one write), so it is the yardstick; with the colour bit the operator reads its input twice (the ordered partial
              sums, then the apply)
Every figure is the median over `--rounds` alternating rounds (range given too).  One JSON line on stdout; --out writes it to a file."""
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


def summary(t, scale=1.0, nd=3):
    return {"median": round(statistics.median(t) * scale, nd), "min": round(min(t) * scale, nd), "max": round(max(t) * scale, nd)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=os.path.join(ROOT, "configs", "male2female.yaml"))
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=4, help="updates pairs per timing")
    ap.add_argument("--reps", type=int, default=200, help="operator launches per timing")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    opts = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU timing of a device path"
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib as L
    from aclgan_amd.trainer import aclgan_Trainer, draw_augment_params
    B, S = opts.batch, opts.size
    out = {"what": "dis_augment at %dx%d B=%d" % (S, S, B), "config": os.path.basename(opts.config), "rounds": opts.rounds,
           "steps_per_timing": opts.steps, "reps_per_timing": opts.reps, "device": torch.cuda.get_device_name(0)}

    # ---- the step ----
    cfg = yaml.safe_load(open(opts.config))
    cfg["display_size"] = 1
    g = torch.Generator().manual_seed(0)
    x_a = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).cuda()
    x_b = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).cuda()
    variants = []
    for dtype in ("fp32", "bf16"):
        for key in ("", "color,translation,cutout"):
            c = dict(cfg)
            c["dis_augment"] = key
            torch.manual_seed(1)
            tr = aclgan_Trainer(c, compute_dtype=dtype)

            def step(tr=tr, c=c):
                tr.dis_update(x_a, x_b, c)
                tr.gen_update(x_a, x_b, c)
            variants.append(("%s_%s" % (dtype, "aug" if key else "off"), step))
    times = {name: [] for name, _ in variants}
    for _ in range(opts.rounds):
        for name, fn in variants:
            times[name].append(events_ms(fn, opts.steps, warm=2))
    out["step_ms"] = {name: summary(times[name]) for name, _ in variants}
    for dtype in ("fp32", "bf16"):
        a, o = out["step_ms"][dtype + "_aug"], out["step_ms"][dtype + "_off"]
        out["step_ms"][dtype + "_aug_minus_off"] = round(a["median"] - o["median"], 3)

    # ---- the operator and the copy ----
    hip = C.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    st = L.stream_ptr()
    N = 2 * B
    ops = {}
    for Cc in (3, 6):
        gen = torch.Generator(device="cuda").manual_seed(Cc)
        x = torch.randn(N, S, S, Cc, device="cuda", generator=gen)
        y = torch.empty_like(x)
        p = draw_augment_params(7, N, S, S, g).cuda()
        scratch = torch.empty(L.lib.aclgan_diffaugment_scratch_bytes(N, S, S, Cc) // 4 + 16, device="cuda")
        nbytes = x.numel() * 4

        def fwd(policy, x=x, y=y, p=p, scratch=scratch, Cc=Cc):
            L.check(L.lib.aclgan_diffaugment_fwd(N, S, S, Cc, policy, L.ptr(x), L.ptr(p), L.ptr(y), L.ptr(scratch), st), "diffaugment_fwd")

        def bwd(policy, x=x, y=y, p=p, scratch=scratch, Cc=Cc):
            L.check(L.lib.aclgan_diffaugment_bwd(N, S, S, Cc, policy, L.ptr(x), L.ptr(p), L.ptr(y), 0, L.ptr(scratch), st), "diffaugment_bwd")

        def copy(x=x, y=y, nbytes=nbytes):
            rc = hip.hipMemcpyAsync(y.data_ptr(), x.data_ptr(), nbytes, 3, st)      # 3 = hipMemcpyDeviceToDevice
            assert rc == 0, rc
        ov = (("fwd_p7", lambda fwd=fwd: fwd(7)), ("bwd_p7", lambda bwd=bwd: bwd(7)), ("fwd_p6", lambda fwd=fwd: fwd(6)),
              ("bwd_p6", lambda bwd=bwd: bwd(6)), ("copy", copy))
        t = {name: [] for name, _ in ov}
        for _ in range(opts.rounds):
            for name, fn in ov:
                t[name].append(events_ms(fn, opts.reps, warm=5))
        r = {"tensor_mb": round(nbytes / 1e6, 2)}
        for name, _ in ov:
            r[name + "_us"] = summary(t[name], 1e3, 2)
        for name in ("fwd_p7", "bwd_p7", "fwd_p6", "bwd_p6"):
            r[name + "_over_copy"] = round(r[name + "_us"]["median"] / r["copy_us"]["median"], 3)
        r["copy_tb_per_s"] = round(2 * nbytes / (r["copy_us"]["median"] * 1e-6) / 1e12, 3)
        ops["N%d_C%d" % (N, Cc)] = r
    out["operator"] = ops
    line = json.dumps(out)
    print(line)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
