"""What translating a test folder costs (test_batch.py's core, acl-gan_amd/translate.py): full-width configs/male2female.yaml with random
weights, N synthetic 256x256 JPEGs in a temporary folder.

  images/s        the parent commit's only way -- an in-process loop of test.load_image -> test.translate -> test.save_image at batch 1 --
                  against translate_folder at batch_size 1, 8 and 32: medians of alternating rounds
  stages          one batch split into host decode, upload + transform, forward (encode + decode), finish (csrc/finish.hip), device->host
                  copy of the bytes, Pillow's encodes
  kernel rate     the two finishing launches against a device-to-device copy with the same memory traffic (the bytes the launches read
                  and write), timed in the same rounds
  key-off check   with --parent ROOT (a built checkout of the previous commit): bench.py alternating between this tree and that one, three
                  runs each -- no training path is touched, the ranges must overlap

Device parts are timed with stream events over repeated launches after a warm-up, host parts and whole runs with a host clock around work
that ends in a device synchronise.  Writes profiles/translate_folder.json (--out) and prints the same JSON."""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BENCH_ARGS = ["--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--no-other-configs", "--no-launch-floor"]


def bench_py(root):
    r = subprocess.run([sys.executable, "bench.py"] + BENCH_ARGS, cwd=root, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError("bench.py failed in %s: %s" % (root, r.stderr[-2000:]))
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    return {"images_per_s": d["value"], "ms_per_step": d["ms_per_step"]}


def key_off_check(parent, runs=3):
    this, prev = [], []
    for k in range(runs):
        this.append(bench_py(ROOT))
        prev.append(bench_py(parent))
        print("key-off run %d: this %s previous %s" % (k, this[-1], prev[-1]), file=sys.stderr, flush=True)
    lo = lambda v: min(x["images_per_s"] for x in v)
    hi = lambda v: max(x["images_per_s"] for x in v)
    return {"command": "bench.py " + " ".join(BENCH_ARGS) + ", alternating this / previous", "this_build": this, "previous_build": prev,
            "ranges_overlap": lo(this) <= hi(prev) and lo(prev) <= hi(this)}


def write(res, out):
    def rnd(v):
        if isinstance(v, float):
            return round(v, 4)
        if isinstance(v, dict):
            return {k: rnd(x) for k, x in v.items()}
        if isinstance(v, list):
            return [rnd(x) for x in v]
        return v
    text = json.dumps(rnd(res), indent=1, sort_keys=True)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=os.path.join(ROOT, "configs", "male2female.yaml"))
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch_sizes", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--stage_batch", type=int, default=8)
    ap.add_argument("--parent", default=None, help="a built checkout of the previous commit: adds the bench.py key-off check")
    ap.add_argument("--key_off_only", action="store_true", help="only the bench.py check, merged into an existing --out file")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "translate_folder.json"))
    opts = ap.parse_args()

    res = {"config": os.path.basename(opts.config), "images": opts.images, "rounds": opts.rounds}
    if opts.key_off_only:
        if os.path.exists(opts.out):
            res = json.load(open(opts.out))
        res["bench_py_key_off"] = key_off_check(opts.parent)
        write(res, opts.out)
        return
    if opts.parent:                       # first: child processes, before this one opens the GPU
        res["bench_py_key_off"] = key_off_check(opts.parent)

    import numpy as np
    import torch
    import yaml
    from PIL import Image
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU timing of a device path"
    import aclgan_amd  # noqa: F401
    from aclgan_amd import translate as TR
    from aclgan_amd.data import GpuBatchTransform, default_loader
    from aclgan_amd.trainer import aclgan_Trainer
    import importlib.util
    spec = importlib.util.spec_from_file_location("aclgan_test_script_bench", os.path.join(ROOT, "test.py"))
    test_py = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(test_py)

    cfg = yaml.safe_load(open(opts.config))
    torch.manual_seed(0)
    tr = aclgan_Trainer(cfg, device="cuda:0")
    new_size, sd = cfg["new_size"], cfg["gen"]["style_dim"]
    H = W = 256
    tmp = tempfile.mkdtemp(prefix="translate_bench_")
    try:
        src = os.path.join(tmp, "in")
        os.makedirs(src)
        rng = np.random.RandomState(0)
        yy, xx = np.mgrid[0:H, 0:W]
        for i in range(opts.images):      # smooth pictures with noise: JPEG sizes and encode times of photographs, not of flat colour or white noise
            base = np.stack([(xx + 3 * i) % 256, (yy * 2 + 7 * i) % 256, ((xx + yy) // 2 + i) % 256], -1)
            Image.fromarray(((base + rng.randint(0, 24, (H, W, 3))) % 256).astype(np.uint8)).save(os.path.join(src, "img%04d.jpg" % i), quality=90)
        files = TR.list_files(src, 0)

        def loop_batch_1(out):
            """test.py's functions, one image at a time: what a user of the parent commit had (without its process start per image)"""
            styles = torch.randn(len(files), 1, sd, 1, 1)
            for i, p in enumerate(files):
                image = test_py.load_image(p, new_size).cuda()
                (outputs, mask, _), = test_py.translate(tr, image, styles[i].cuda(), a2b=True)
                test_py.save_image(outputs, os.path.join(out, "_00_bar", os.path.basename(p)))
                if mask is not None:
                    test_py.save_image(mask, os.path.join(out, "_00_mask", os.path.basename(p)))
                test_py.save_image(image, os.path.join(out, "input%03d.jpg" % i))

        def timed(fn):
            out = os.path.join(tmp, "out")
            shutil.rmtree(out, ignore_errors=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(out)
            torch.cuda.synchronize()
            return opts.images / (time.perf_counter() - t0)

        variants = [("loop_batch_1", loop_batch_1)]
        for bs in opts.batch_sizes:
            variants.append(("translate_folder_b%d" % bs, lambda out, bs=bs: TR.translate_folder(tr, cfg, src, out, batch_size=bs, max_images=0)))
        for _, fn in variants:            # warm-up: code objects, workspaces, pinned buffers of every shape the timed rounds use
            timed(fn)
        rates = {name: [] for name, _ in variants}
        for _ in range(opts.rounds):      # alternating rounds
            for name, fn in variants:
                rates[name].append(timed(fn))
                print("%s: %.1f images/s" % (name, rates[name][-1]), file=sys.stderr, flush=True)
        res["images_per_s"] = {k: {"median": statistics.median(v), "rounds": v} for k, v in rates.items()}
        base = res["images_per_s"]["loop_batch_1"]["median"]
        res["ratio_to_loop_batch_1"] = {k: v["median"] / base for k, v in res["images_per_s"].items()}

        # ---- stages of one batch ----
        B = opts.stage_batch
        focus = tr.focus_lam > 0

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

        st = {"batch": B, "cpu_threads_for_encodes": min(TR.MAX_WORKERS, max(4, 2 * B))}
        st["decode_ms_per_image_one_thread"] = host_ms(lambda: [default_loader(p) for p in files[:B]], 3) / B
        pil = [default_loader(p) for p in files[:B]]
        tf = GpuBatchTransform(new_size, None, None, train=False, crop=False, device=tr.device)
        st["upload_transform_ms"] = host_ms(lambda: tf(pil), 10)
        images = tf(pil)
        styles = torch.randn(B, 1, sd, 1, 1).cuda()
        gen = tr.gen_AB
        st["forward_ms"] = events_ms(lambda: gen.decode(gen.encode(images)[0], styles[:, 0]), 10)
        dec = gen.decode(gen.encode(images)[0], styles[:, 0])
        names = ["bar", "mask", "input"] if focus else ["bar", "input"]
        buf = torch.empty(len(names), B, H, W, 3, dtype=torch.uint8, device=tr.device)
        out = {n: buf[k] for k, n in enumerate(names)}
        fdec = dec if focus else dec[:, :3]
        st["finish_ms"] = events_ms(lambda: TR.finish_u8(fdec, images, outputs=names, out=out), 50, warm=3)
        st["d2h_ms"] = host_ms(lambda: TR._to_host(buf), 10)
        host = TR._to_host(buf).numpy()
        enc = os.path.join(tmp, "enc")
        os.makedirs(enc)
        st["encode_ms_per_image_one_thread"] = host_ms(
            lambda: [Image.fromarray(host[k, i]).save(os.path.join(enc, "%d_%d.jpg" % (k, i))) for k in range(len(names)) for i in range(B)], 3) / B
        st["files_per_image"] = len(names)
        res["stages"] = st

        # ---- kernel rate against a copy with the same traffic, same rounds ----
        planes = (7 + 1 + 3) if focus else (3 + 3)          # fp32 planes read per image by each of the two launches
        kr = {}
        for Bk in sorted(set([B, max(opts.batch_sizes)])):
            d = (torch.rand(Bk, dec.shape[1], H, W, device=tr.device) * 2 - 1)
            x = (torch.rand(Bk, 3, H, W, device=tr.device) * 2 - 1)
            fd = d if focus else d[:, :3]
            ob = torch.empty(len(names), Bk, H, W, 3, dtype=torch.uint8, device=tr.device)
            o = {n: ob[k] for k, n in enumerate(names)}
            traffic = Bk * H * W * (2 * planes * 4 + 3 * len(names))
            a, b = torch.empty(traffic // 2, dtype=torch.uint8, device=tr.device), torch.empty(traffic // 2, dtype=torch.uint8, device=tr.device)
            f_ms, c_ms = [], []
            for _ in range(opts.rounds):
                f_ms.append(events_ms(lambda: TR.finish_u8(fd, x, outputs=names, out=o), 50, warm=3))
                c_ms.append(events_ms(lambda: b.copy_(a), 50, warm=3))
            fm, cm = statistics.median(f_ms), statistics.median(c_ms)
            kr["B%d" % Bk] = {"traffic_bytes": traffic, "finish_ms": fm, "copy_same_traffic_ms": cm, "finish_over_copy": fm / cm,
                              "finish_GB_per_s": traffic / fm / 1e6, "copy_GB_per_s": traffic / cm / 1e6, "finish_ms_rounds": f_ms, "copy_ms_rounds": c_ms}
        res["finish_kernels_vs_copy"] = kr
    finally:
        shutil.rmtree(tmp, ignore_errors=True)

    write(res, opts.out)


if __name__ == "__main__":
    main()
