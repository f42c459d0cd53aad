"""What guided-filter upsampling of the edit costs (translate_photos.py --full_size --detail guided; acl-gan_amd/translate.py: guided_u8,
csrc/guided.hip): full-width configs/male2female.yaml with random weights, the conventions of scripts/bench_paste.py.

  apply launch    N sources of 3000x4000 (H x W) from the coefficient planes of a 256x341 net output, bar and mask in one launch, against
                  paste_kernel (paste_u8) on the same decoder outputs, sources and output buffers, and against a device-to-device copy of
                  the same bytes (source read, pictures written, the coefficient planes read) -- all three timed in the same alternating rounds
  coefficients    the two launches of the coefficient stage alone, at the default radius and at the widest
  images/s        translate_folder over bench_paste.py's synthetic 1024x768 JPEGs, fit: pad and full size, detail: guided against detail:
                  bilinear -- medians of alternating rounds, the ranges reported

Device parts are timed with stream events over repeated launches after a warm-up, whole runs with a host clock around work that ends in a
device synchronise.  Writes profiles/guided_fullsize.json (--out) and prints the same JSON."""
import argparse
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_paste import write  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=os.path.join(ROOT, "configs", "male2female.yaml"))
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch_sizes", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--kernel_sources", type=int, default=8)
    ap.add_argument("--kernel_source_size", type=int, nargs=2, default=[3000, 4000], help="H W")
    ap.add_argument("--folder_source_size", type=int, nargs=2, default=[768, 1024], help="H W")
    ap.add_argument("--radius", type=int, default=4)
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--no_folder", action="store_true", help="the device timings only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided_fullsize.json"))
    opts = ap.parse_args()

    import numpy as np
    import torch
    import yaml
    from PIL import Image
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU timing of a device path"
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib as L
    from aclgan_amd import translate as TR
    from aclgan_amd.data import resized_size

    cfg = yaml.safe_load(open(opts.config))
    new_size, M = cfg["new_size"], 2 ** cfg["gen"]["n_downsample"]
    focus = cfg["focus_loss"] > 0
    dev = torch.device("cuda:0")
    res = {"config": os.path.basename(opts.config), "images": opts.images, "rounds": opts.rounds, "radius": opts.radius, "eps": opts.eps}

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

    def med(v):
        return {"median": statistics.median(v), "min": min(v), "max": max(v), "rounds": v}

    # ---- the apply launch against paste_kernel and a copy of the same bytes, same rounds ----
    Hs, Ws = opts.kernel_source_size
    ow, oh = resized_size(Ws, Hs, new_size)
    PH, PW = TR.padded_shape((oh, ow), M)
    n = opts.kernel_sources
    g = torch.Generator(device=dev).manual_seed(1)
    Cd, planes = (4, 7) if focus else (3, 6)
    dec = torch.tanh(torch.randn(n, Cd, PH, PW, device=dev, generator=g) * 1.5)
    x = torch.rand(n, 3, PH, PW, device=dev, generator=g) * 2 - 1
    src = torch.randint(0, 256, (n * Hs * Ws * 3,), device=dev, dtype=torch.uint8, generator=g)
    plan = TR.paste_plan([(k * Hs * Ws * 3, Hs, Ws) for k in range(n)], dev)
    names = ["bar", "mask"] if focus else ["bar"]
    ob = torch.empty(len(names), plan["total"], dtype=torch.uint8, device=dev)
    o = {nm: ob[k] for k, nm in enumerate(names)}
    coef = torch.empty(n, planes, oh, ow, device=dev)
    scratch = torch.empty(L.lib.aclgan_translate_guided_scratch_bytes(n, oh, ow, 16), dtype=torch.uint8, device=dev)

    def coefficients(radius):
        L.check(L.lib.aclgan_translate_guided_coef(L.ptr(dec), dec.stride(0), Cd, L.ptr(x), x.stride(0), n, oh, ow, PH, PW, radius, opts.eps,
                                                   L.ptr(coef), L.ptr(scratch), L.stream_ptr(dev)), "translate_guided_coef")

    def apply():
        L.check(L.lib.aclgan_translate_guided_paste_u8(L.ptr(coef), planes, n, oh, ow, L.ptr(src), src.numel(), plan["descs"], L.ptr(plan["dev"]),
                                                       L.ptr(o["bar"]), L.ptr(o.get("mask")), plan["total"], L.stream_ptr(dev)),
                "translate_guided_paste_u8")

    coefficients(opts.radius)
    plane_bytes = coef.numel() * 4
    traffic = src.numel() + ob.numel() + plane_bytes
    a, b = torch.empty(traffic // 2, dtype=torch.uint8, device=dev), torch.empty(traffic // 2, dtype=torch.uint8, device=dev)
    g_ms, p_ms, c_ms, k_ms, k16_ms = [], [], [], [], []
    for _ in range(opts.rounds):
        g_ms.append(events_ms(apply, 20))
        p_ms.append(events_ms(lambda: TR.paste_u8(dec, x, (oh, ow), src, plan, outputs=names, out=o), 20))
        c_ms.append(events_ms(lambda: b.copy_(a), 20))
        k_ms.append(events_ms(lambda: coefficients(opts.radius), 50))
        k16_ms.append(events_ms(lambda: coefficients(16), 50))
    gm, pm, cm = statistics.median(g_ms), statistics.median(p_ms), statistics.median(c_ms)
    res["apply_vs_paste_vs_copy"] = {
        "sources": n, "source_hw": [Hs, Ws], "valid_hw": [oh, ow], "plane_hw": [PH, PW], "pictures": names, "coefficient_planes": planes,
        "source_bytes_read": src.numel(), "picture_bytes_written": ob.numel(), "coefficient_bytes_read": plane_bytes, "traffic_bytes": traffic,
        "guided_apply_ms": med(g_ms), "paste_kernel_ms": med(p_ms), "copy_same_traffic_ms": med(c_ms),
        "guided_over_paste": gm / pm, "guided_over_copy": gm / cm, "paste_over_copy": pm / cm,
        "guided_GB_per_s": traffic / gm / 1e6, "output_megapixels_per_ms": n * Hs * Ws / gm / 1e6}
    res["coefficient_stage"] = {"images": n, "valid_hw": [oh, ow], "launches": 2, "scratch_bytes": L.lib.aclgan_translate_guided_scratch_bytes(n, oh, ow, opts.radius),
                                "radius_%d_ms" % opts.radius: med(k_ms), "radius_16_ms": med(k16_ms)}
    del a, b, src, ob, o, dec, x, coef, scratch
    torch.cuda.empty_cache()

    # ---- the folder ----
    if not opts.no_folder:
        from aclgan_amd.trainer import aclgan_Trainer
        torch.manual_seed(0)
        tr = aclgan_Trainer(cfg, device="cuda:0")
        FH, FW = opts.folder_source_size
        tmp = tempfile.mkdtemp(prefix="guided_bench_")
        try:
            srcdir = os.path.join(tmp, "in")
            os.makedirs(srcdir)
            rng = np.random.RandomState(0)
            yy, xx = np.mgrid[0:FH, 0:FW]
            for i in range(opts.images):      # bench_paste.py's pictures
                base = np.stack([(xx // 3 + 3 * i) % 256, (yy // 2 + 7 * i) % 256, ((xx + yy) // 6 + i) % 256], -1)
                Image.fromarray(((base + rng.randint(0, 24, (FH, FW, 3))) % 256).astype(np.uint8)).save(os.path.join(srcdir, "img%04d.jpg" % i), quality=90)
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
                for detail in ("bilinear", "guided"):
                    variants.append(("full_size_%s_b%d" % (detail, bs), lambda out, bs=bs, detail=detail: TR.translate_folder(
                        tr, cfg, srcdir, out, batch_size=bs, max_images=0, fit="pad", full_size=True, detail=detail, guided_radius=opts.radius,
                        guided_eps=opts.eps)))
            for _, fn in variants:            # warm-up: code objects, workspaces, pinned buffers of every shape the timed rounds use
                timed(fn)
            rates = {name: [] for name, _ in variants}
            for _ in range(opts.rounds):      # alternating rounds
                for name, fn in variants:
                    rates[name].append(timed(fn))
                    print("%s: %.1f images/s" % (name, rates[name][-1]), file=sys.stderr, flush=True)
            res["images_per_s"] = {k: med(v) for k, v in rates.items()}
        finally:
            shutil.rmtree(tmp, ignore_errors=True)

    write(res, opts.out)


if __name__ == "__main__":
    main()
