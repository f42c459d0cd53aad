"""What one image_save_iter event of train.py costs (male2female config: 256x256, display_size 16, full-width generators), split into
    sample()            display_size per-image forwards (trainer.py:179-245)
    grid                csrc/grid.hip: min / max + compose, the 9 float tensors -> uint8 [9*256][16*256][3] on the device
    D2H                 the bytes to the host
    JPEG                Pillow's encoder on the host
and, for comparison, the host path the grid kernel replaces (the arithmetic of test.py:save_image applied to the whole tuple):
    torch.cat of the expanded floats on the device, D2H of the floats, clamp / normalise / *255 + 0.5 / uint8 on the CPU.
Device parts are timed with stream events over repeated launches after a warm-up, host parts with a host clock after a device
synchronise.  One JSON line on stdout; --out writes the same line to a file."""
import argparse
import json
import os
import sys
import tempfile
import time

import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def events_ms(fn, reps, warm=2):
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


def host_ms(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=os.path.join(ROOT, "configs", "male2female.yaml"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    opts = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU timing of a device path"
    import aclgan_amd  # noqa: F401
    from aclgan_amd import visual
    from aclgan_amd.trainer import aclgan_Trainer
    from PIL import Image
    cfg = yaml.safe_load(open(opts.config))
    n, H, W = cfg["display_size"], cfg["crop_image_height"], cfg["crop_image_width"]
    torch.manual_seed(0)
    tr = aclgan_Trainer(cfg, device="cuda:0")
    g = torch.Generator().manual_seed(1)
    x_a, x_b = ((torch.rand(n, 3, H, W, generator=g) * 2 - 1).cuda() for _ in range(2))

    res = {"config": os.path.basename(opts.config), "display_size": n, "H": H, "W": W, "reps": opts.reps}
    res["sample_ms"] = events_ms(lambda: tr.sample(x_a, x_b), opts.reps, warm=1)
    outs = tr.sample(x_a, x_b)
    res["tensors"] = len(outs)
    res["float_bytes"] = sum(t.numel() * 4 for t in outs)
    res["grid_ms"] = events_ms(lambda: visual.image_grid(outs, n), 50, warm=3)
    grid = visual.image_grid(outs, n)
    res["picture_bytes"] = grid.numel()
    res["grid_d2h_ms"] = host_ms(lambda: grid.cpu(), opts.reps)
    arr = grid.cpu().numpy()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "p.jpg")
        res["jpeg_encode_ms"] = host_ms(lambda: Image.fromarray(arr).save(path), opts.reps)
        res["jpeg_bytes"] = os.path.getsize(path)

    # the host path: floats leave the device, the CPU normalises
    def cat():
        return torch.cat([t.expand(-1, 3, -1, -1) for t in outs], 0)
    res["host_path_cat_ms"] = events_ms(cat, 20)
    floats = cat()
    res["host_path_float_bytes"] = floats.numel() * 4
    res["host_path_d2h_ms"] = host_ms(lambda: floats.cpu(), opts.reps)
    cpu = floats.cpu()

    def normalise():
        t = cpu.clone()
        lo, hi = float(t.min()), float(t.max())
        t = (t.clamp(lo, hi) - lo) / (hi - lo + 1e-5)
        return t.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)
    res["host_path_normalise_ms"] = host_ms(normalise, opts.reps)
    res["host_path_cpu_threads"] = torch.get_num_threads()
    res["device_path_total_ms"] = res["grid_ms"] + res["grid_d2h_ms"]
    res["host_path_total_ms"] = res["host_path_cat_ms"] + res["host_path_d2h_ms"] + res["host_path_normalise_ms"]
    res["event_total_ms"] = res["sample_ms"] + res["grid_ms"] + res["grid_d2h_ms"] + res["jpeg_encode_ms"]
    line = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()})
    print(line)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
