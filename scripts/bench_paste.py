"""What translating photographs at their own size costs (translate_photos.py --fit pad / --full_size; acl-gan_amd/translate.py, csrc/paste.hip):
full-width configs/male2female.yaml with random weights.

  paste kernel    N sources of 3000x4000 (H x W) pasted from a 256x341 net output in 256x344 planes, bar and mask in one launch, against a
                  device-to-device copy of the same bytes (source read, pictures written, the valid region of the net planes read), timed in
                  the same alternating rounds
  crop            fit: pad without full_size finishes strided (oh, ow) views, which torch copies dense: finish_u8 of the views against
                  finish_u8 of dense tensors of the same shape, and the pad launch itself
  images/s        translate_folder over synthetic 1024x768 JPEGs (256x341 after Resize(256): refused without fit: pad) -- net-size pictures
                  with fit: pad, and full-size pictures -- medians of alternating rounds
  stages          one full-size batch split into host decode, upload + transform, pad, forward (encode + decode), paste, device->host copy
                  of the bytes, Pillow's encodes

Device parts are timed with stream events over repeated launches after a warm-up, host parts and whole runs with a host clock around work
that ends in a device synchronise.  Writes profiles/paste_fullsize.json (--out) and prints the same JSON."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write(res, out):
    def rnd(v):
        if isinstance(v, float):
            return round(v, 4)
        if isinstance(v, dict):
            return {k: rnd(x) for k, x in v.items()}
        if isinstance(v, (list, tuple)):
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
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch_sizes", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--stage_batch", type=int, default=8)
    ap.add_argument("--kernel_sources", type=int, default=8)
    ap.add_argument("--kernel_source_size", type=int, nargs=2, default=[3000, 4000], help="H W")
    ap.add_argument("--folder_source_size", type=int, nargs=2, default=[768, 1024], help="H W")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paste_fullsize.json"))
    opts = ap.parse_args()

    import numpy as np
    import torch
    import yaml
    from PIL import Image
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU timing of a device path"
    import aclgan_amd  # noqa: F401
    from aclgan_amd import translate as TR
    from aclgan_amd.data import GpuBatchTransform, default_loader, resized_size
    from aclgan_amd.trainer import aclgan_Trainer

    cfg = yaml.safe_load(open(opts.config))
    torch.manual_seed(0)
    tr = aclgan_Trainer(cfg, device="cuda:0")
    dev = tr.device
    new_size, sd, M = cfg["new_size"], cfg["gen"]["style_dim"], 2 ** cfg["gen"]["n_downsample"]
    focus = tr.focus_lam > 0
    per = 2 if focus else 1
    res = {"config": os.path.basename(opts.config), "images": opts.images, "rounds": opts.rounds}

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

    # ---- the paste kernel against a copy of the same bytes, same rounds ----
    Hs, Ws = opts.kernel_source_size
    ow, oh = resized_size(Ws, Hs, new_size)
    PH, PW = TR.padded_shape((oh, ow), M)
    n = opts.kernel_sources
    g = torch.Generator(device=dev).manual_seed(1)
    dec = torch.tanh(torch.randn(n, 4 if focus else 3, PH, PW, device=dev, generator=g) * 1.5)
    x = torch.rand(n, 3, PH, PW, device=dev, generator=g) * 2 - 1
    src = torch.randint(0, 256, (n * Hs * Ws * 3,), device=dev, dtype=torch.uint8, generator=g)
    plan = TR.paste_plan([(k * Hs * Ws * 3, Hs, Ws) for k in range(n)], dev)
    names = ["bar", "mask"] if focus else ["bar"]
    ob = torch.empty(len(names), plan["total"], dtype=torch.uint8, device=dev)
    o = {nm: ob[k] for k, nm in enumerate(names)}
    planes = (7 if focus else 6) * oh * ow * 4 * n
    traffic = src.numel() + ob.numel() + planes
    a, b = torch.empty(traffic // 2, dtype=torch.uint8, device=dev), torch.empty(traffic // 2, dtype=torch.uint8, device=dev)
    p_ms, c_ms = [], []
    for _ in range(opts.rounds):
        p_ms.append(events_ms(lambda: TR.paste_u8(dec, x, (oh, ow), src, plan, outputs=names, out=o), 20, warm=3))
        c_ms.append(events_ms(lambda: b.copy_(a), 20, warm=3))
    pm, cm = statistics.median(p_ms), statistics.median(c_ms)
    res["paste_kernel_vs_copy"] = {
        "sources": n, "source_hw": [Hs, Ws], "valid_hw": [oh, ow], "plane_hw": [PH, PW], "pictures": names,
        "source_bytes_read": src.numel(), "picture_bytes_written": ob.numel(), "net_plane_bytes_read": planes, "traffic_bytes": traffic,
        "paste_ms": pm, "copy_same_traffic_ms": cm, "paste_over_copy": pm / cm, "paste_GB_per_s": traffic / pm / 1e6,
        "copy_GB_per_s": traffic / cm / 1e6, "output_megapixels_per_ms": n * Hs * Ws / pm / 1e6, "paste_ms_rounds": p_ms, "copy_ms_rounds": c_ms}
    del a, b, src, ob, o
    torch.cuda.empty_cache()

    # ---- what the crop of fit: pad costs: finish_u8 of strided views (copied dense) against dense tensors of the same shape ----
    B = opts.stage_batch
    fdec = dec[:B] if focus else dec[:B, :3]
    dd, xd = fdec[:, :, :oh, :ow].contiguous(), x[:B, :, :oh, :ow].contiguous()
    fnames = ["bar", "mask", "input"] if focus else ["bar", "input"]
    fb = torch.empty(len(fnames), B, oh, ow, 3, dtype=torch.uint8, device=dev)
    fo = {nm: fb[k] for k, nm in enumerate(fnames)}
    v_ms, d_ms, pad_ms = [], [], []
    for _ in range(opts.rounds):
        v_ms.append(events_ms(lambda: TR.finish_u8(fdec[:, :, :oh, :ow], x[:B, :, :oh, :ow], outputs=fnames, out=fo), 50, warm=3))
        d_ms.append(events_ms(lambda: TR.finish_u8(dd, xd, outputs=fnames, out=fo), 50, warm=3))
        pad_ms.append(events_ms(lambda: TR.reflect_pad(xd, M), 50, warm=3))
    res["crop_cost"] = {"batch": B, "valid_hw": [oh, ow], "plane_hw": [PH, PW], "finish_of_views_ms": statistics.median(v_ms),
                        "finish_of_dense_ms": statistics.median(d_ms), "crop_copies_ms": statistics.median(v_ms) - statistics.median(d_ms),
                        "copied_bytes_read_and_written": 2 * (dd.numel() + xd.numel()) * 4, "reflect_pad_ms": statistics.median(pad_ms),
                        "finish_of_views_ms_rounds": v_ms, "finish_of_dense_ms_rounds": d_ms, "reflect_pad_ms_rounds": pad_ms}
    del dec, x, dd, xd, fb, fo
    torch.cuda.empty_cache()

    # ---- the folder ----
    FH, FW = opts.folder_source_size
    tmp = tempfile.mkdtemp(prefix="paste_bench_")
    try:
        srcdir = os.path.join(tmp, "in")
        os.makedirs(srcdir)
        rng = np.random.RandomState(0)
        yy, xx = np.mgrid[0:FH, 0:FW]
        for i in range(opts.images):      # smooth pictures with noise: JPEG sizes and encode times of photographs, not of flat colour or white noise
            base = np.stack([(xx // 3 + 3 * i) % 256, (yy // 2 + 7 * i) % 256, ((xx + yy) // 6 + i) % 256], -1)
            Image.fromarray(((base + rng.randint(0, 24, (FH, FW, 3))) % 256).astype(np.uint8)).save(os.path.join(srcdir, "img%04d.jpg" % i), quality=90)
        files = TR.list_files(srcdir, 0)
        fow, foh = resized_size(FW, FH, new_size)
        res["folder"] = {"source_hw": [FH, FW], "resized_hw": [foh, fow], "net_hw": list(TR.padded_shape((foh, fow), M))}

        def timed(fn):
            out = os.path.join(tmp, "out")
            shutil.rmtree(out, ignore_errors=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(out)
            torch.cuda.synchronize()
            return opts.images / (time.perf_counter() - t0)

        variants = []
        for bs in opts.batch_sizes:
            variants.append(("fit_pad_net_size_b%d" % bs, lambda out, bs=bs: TR.translate_folder(tr, cfg, srcdir, out, batch_size=bs, max_images=0, fit="pad")))
            variants.append(("fit_pad_full_size_b%d" % bs,
                             lambda out, bs=bs: TR.translate_folder(tr, cfg, srcdir, out, batch_size=bs, max_images=0, fit="pad", full_size=True)))
        for _, fn in variants:            # warm-up: code objects, workspaces, pinned buffers of every shape the timed rounds use
            timed(fn)
        rates = {name: [] for name, _ in variants}
        for _ in range(opts.rounds):      # alternating rounds
            for name, fn in variants:
                rates[name].append(timed(fn))
                print("%s: %.1f images/s" % (name, rates[name][-1]), file=sys.stderr, flush=True)
        res["images_per_s"] = {k: {"median": statistics.median(v), "rounds": v} for k, v in rates.items()}

        # ---- stages of one full-size batch ----
        st = {"batch": B, "cpu_threads_for_encodes": min(TR.MAX_WORKERS, max(4, 2 * B))}
        st["decode_ms_per_image_one_thread"] = host_ms(lambda: [default_loader(p).load() for p in files[:B]], 3) / B
        pil = [default_loader(p) for p in files[:B]]
        tf = GpuBatchTransform(new_size, None, None, train=False, crop=False, device=dev)
        st["upload_transform_ms"] = host_ms(lambda: tf.launch(tf.stage(pil)), 10)
        staged = tf.stage(pil)
        images = tf.launch(staged)
        st["pad_ms"] = events_ms(lambda: TR.reflect_pad(images, M), 50, warm=3)
        padded = TR.reflect_pad(images, M)
        styles = torch.randn(B, 1, sd, 1, 1).cuda()
        gen = tr.gen_AB
        st["forward_ms"] = events_ms(lambda: gen.decode(gen.encode(padded)[0], styles[:, 0]), 10)
        fd = gen.decode(gen.encode(padded)[0], styles[:, 0])
        fd = fd if focus else fd[:, :3]
        sources = tf.sources(staged)
        fplan = TR.paste_plan(sources[1], dev)
        pb = torch.empty(per, fplan["total"], dtype=torch.uint8, device=dev)
        po = {nm: pb[k] for k, nm in enumerate(names)}
        st["paste_ms"] = events_ms(lambda: TR.paste_u8(fd, padded, (foh, fow), sources[0], fplan, outputs=names, out=po), 50, warm=3)
        st["paste_plan_ms"] = host_ms(lambda: TR.paste_plan(sources[1], dev), 10)
        st["d2h_ms"] = host_ms(lambda: TR._to_host(pb), 10)
        st["d2h_bytes"] = pb.numel()
        host = TR._to_host(pb).numpy()
        enc = os.path.join(tmp, "enc")
        os.makedirs(enc)

        def encodes():
            for k in range(B):
                off = fplan["offsets"][k]
                for q in range(per):
                    Image.fromarray(host[q, off:off + FH * FW * 3].reshape(FH, FW, 3)).save(os.path.join(enc, "%d_%d.jpg" % (q, k)))
                Image.fromarray(np.asarray(pil[k], dtype=np.uint8)).save(os.path.join(enc, "in_%d.jpg" % k))
        st["encode_ms_per_image_one_thread"] = host_ms(encodes, 3) / B
        st["files_per_image"] = per + 1
        res["stages_full_size"] = st
    finally:
        shutil.rmtree(tmp, ignore_errors=True)

    write(res, opts.out)


if __name__ == "__main__":
    main()
