"""Fingerprint of what a build decides and produces, as one JSON document: run it in two trees and diff the output.
  --dry   no GPU: the launch-free entry points (workspace sizes, algorithmic bytes, executed FLOPs, bucket schedules, per-layer scratch sizes and
          16-bit eligibility) over architectures x dis.norm x dtype x lanes x deterministic x buckets x shapes, in a child without ACLGAN_* variables
  --gpu   the full-width network at 64x64 B=2 (the smallest shape that takes the Winograd, sub-pixel, parity, thin-channel and 16-bit-storage
          kernels), seeded: sha256 of the losses and of each group's gradients in deterministic mode, and the launch count of each update"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ARCHS = {"full": (64, 256, 64, 4), "r8": (8, 16, 8, 3), "r16": (16, 32, 16, 4)}      # gen.dim, gen.mlp_dim, dis.dim, gen.output_dim
SHAPES = [(1, 64, 64), (2, 128, 64), (8, 256, 256), (4, 512, 512)]


def config(arch):
    import yaml
    from oracle import aclgan_oracle as O
    with open(os.path.join(ROOT, "configs", "male2female.yaml")) as f:
        y = yaml.safe_load(f)
    cfg = O.default_config()
    for k in ("gen", "dis"):
        cfg[k].update({kk: y[k][kk] for kk in cfg[k] if kk in y[k]})
    cfg.update({k: y[k] for k in ("input_dim_a", "input_dim_b", "focus_loss", "alpha") if k in y})
    gd, md, dd, od = ARCHS[arch]
    cfg["gen"].update(dim=gd, mlp_dim=md, output_dim=od)
    cfg["dis"].update(dim=dd)
    return cfg


def layers(cfg, B, H, W):
    """distinct convolution layers of one dis_update + gen_update, from the oracle's conv_block calls on meta tensors (tests/test_gpu_launch_shapes.py):
    generator layers at B, discriminator layers at the joint batches B, 2B, 3B, and the 1x1 head of every discriminator scale"""
    import torch
    from oracle import aclgan_oracle as O
    od = cfg["gen"]["output_dim"]      # (the oracle's loss graph needs the focus channel: recorded at 4 output channels, the image layer put back to od)
    cfg = dict(cfg, gen=dict(cfg["gen"], output_dim=4))
    nets = {n: {k: t.to("meta") for k, t in P.items()} for n, P in O.test_nets(cfg, 0).items()}
    dis = {id(t) for n, P in nets.items() if n.startswith("dis_") for t in P.values()}
    x = torch.empty(1, cfg["input_dim_a"], H, W, device="meta")
    z = [torch.empty(1, cfg["gen"]["style_dim"], 1, 1, device="meta") for _ in range(3)]
    out, orig = set(), O.conv_block

    def recording(x, w, b, stride, pad, act="none", *a, **k):
        up = int(bool(k.get("upsample", a[2] if len(a) > 2 else False)))
        for m in ((1, 2, 3) if id(w) in dis else (1,)):
            out.add((m * B, x.shape[2], x.shape[3], x.shape[1], w.shape[0], w.shape[2], stride, pad, up, act))
            if id(w) in dis and w.shape[0] == cfg["dis"]["dim"] << (cfg["dis"]["n_layer"] - 1):
                out.add((m * B, ((x.shape[2] << up) + 2 * pad - w.shape[2]) // stride + 1, ((x.shape[3] << up) + 2 * pad - w.shape[2]) // stride + 1,
                         w.shape[0], 1, 1, 1, 0, 0, "none"))
        return orig(x, w, b, stride, pad, act, *a, **k)
    O.conv_block = recording
    try:
        with torch.no_grad():
            O.dis_losses(nets, x, x, z, cfg)
            O.gen_losses(nets, x, x, z, cfg)
    finally:
        O.conv_block = orig
    return sorted(g[:4] + (od,) + g[5:] if g[4] == 4 and g[5] == 7 else g for g in out)


def dry():
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib as L
    from aclgan_amd.trainer import arch_from_config
    lib, fake, doc = L.lib, C.c_void_p(0x10000), {"steps": {}, "layers": {}}
    conv_sizes = sorted(n for n, (_, args) in L.SIGNATURES.items() if n.startswith("aclgan_conv2d_") and n.endswith("scratch_bytes") and len(args) == 1)
    for arch in ARCHS:
        cfg = config(arch)
        a = arch_from_config(cfg)
        for det in (0, 1):
            lib.aclgan_set_deterministic(det)
            for (B, H, W) in SHAPES:
                for g in layers(cfg, B, H, W):
                    d = L.ConvDesc(*g[:9], L.ACT[g[9]])
                    doc["layers"]["det%d %s" % (det, list(g))] = [getattr(lib, n)(C.byref(d)) for n in conv_sizes] + \
                        [lib.aclgan_conv16_eligible(C.byref(d), w) for w in (0, 1, 2)] + [lib.aclgan_conv16s_ok(C.byref(d), w) for w in (0, 1)]
            for norm in ("none", "sn"):
                for dt in (0, 1, 2):
                    ctx = C.c_void_p()
                    L.check(lib.aclgan_ctx_create_dis_norm(C.byref(a), L.NORM[norm], C.byref(ctx)))
                    L.check(lib.aclgan_set_compute_dtype(ctx, dt))
                    for grp in (0, 1):
                        L.check(lib.aclgan_bind_params(ctx, grp, fake, fake, fake, fake))
                        if dt:
                            L.check(lib.aclgan_bind_params16(ctx, grp, fake, fake))
                    for lanes in (1, 2, 3):
                        L.check(lib.aclgan_tuning(b"lanes", lanes, None))
                        for bucket in (0, 1 << 16):
                            rcb = lib.aclgan_set_grad_buckets(ctx, bucket, L.BUCKET_FN(), None)
                            for (B, H, W) in SHAPES:
                                ws, fw, v, row = C.c_size_t(), C.c_size_t(), C.c_double(), [rcb]
                                row += [lib.aclgan_workspace_bytes(ctx, B, H, W, C.byref(ws)), ws.value]
                                row += [lib.aclgan_forward_workspace_bytes(ctx, B, H, W, C.byref(fw)), fw.value]
                                for fn in (lib.aclgan_step_algorithmic_bytes, lib.aclgan_step_executed_flops):
                                    for which in (0, 1):
                                        row += [fn(ctx, which, B, H, W, C.byref(v)), repr(v.value)]
                                for grp in (0, 1):
                                    order, cnt = (C.c_int * 65536)(), C.c_int()
                                    row += [lib.aclgan_bucket_schedule(ctx, grp, B, H, W, 0, order, 65536, C.byref(cnt)), list(order[:max(cnt.value, 0)])]
                                doc["steps"]["%s %s dt%d lanes%d det%d bucket%d %s" % (arch, norm, dt, lanes, det, bucket, [B, H, W])] = row
                    lib.aclgan_ctx_destroy(ctx)
    lib.aclgan_set_deterministic(0)
    assert lib.aclgan_launch_count() == 0, "a dry run launched a kernel"
    return doc


def gpu():
    import torch
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib as L
    from aclgan_amd.trainer import aclgan_Trainer
    from oracle import aclgan_oracle as O
    cfg, doc = config("full"), {}
    nets = O.test_nets(cfg, 0)
    g = torch.Generator().manual_seed(0)
    x_a, x_b = (torch.rand(2, 3, 64, 64, generator=g) * 2 - 1 for _ in range(2))
    z = [torch.randn(2, cfg["gen"]["style_dim"], 1, 1, generator=g) for _ in range(6)]
    sha = lambda t: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
    for dt in ("fp32", "bf16", "fp16"):
        for det, lanes in ((1, 3), (1, 1), (0, 3), (0, 1)):
            L.check(L.lib.aclgan_tuning(b"lanes", lanes, None))
            tr = aclgan_Trainer(cfg, device="cuda:0", compute_dtype=dt, deterministic=bool(det))
            for n in O.OracleTrainer.NETS:
                getattr(tr, n).load_state_dict(nets[n], strict=False)
            for which, grp, zz in (("dis", L.GROUP_DIS, z[:3]), ("gen", L.GROUP_GEN, z[3:])):
                n0 = L.lib.aclgan_launch_count()
                getattr(tr, which + "_update")(x_a, x_b, cfg, z=zz)
                torch.cuda.synchronize()
                key = "%s %s_update det%d lanes%d" % (dt, which, det, lanes)
                doc[key + " launches"] = L.lib.aclgan_launch_count() - n0
                if det and lanes == 3:
                    doc[key + " sha256"] = {"losses": sha(tr._losses), "grad": sha(tr._grad[grp])}
            del tr
    return doc


if __name__ == "__main__":
    if "--child" in sys.argv:
        print(json.dumps(dry(), sort_keys=True, indent=0))
    elif "--dry" in sys.argv:      # (a switch is latched on its first read: a child with every ACLGAN_* variable stripped)
        env = {k: v for k, v in os.environ.items() if not k.startswith("ACLGAN_")}
        sys.exit(subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env).returncode)
    elif "--gpu" in sys.argv:
        print(json.dumps(gpu(), sort_keys=True, indent=0))
    else:
        sys.exit(__doc__)
