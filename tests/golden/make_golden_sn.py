#!/usr/bin/env python3
"""Generate the spectral-norm golden fixtures (dis.norm: sn) in this directory by IMPORTING THE REFERENCE on CPU.

Run only in the build container (needs the reference tree, like make_golden.py, whose shims and helpers this
script imports):
    python tests/golden/make_golden_sn.py

Written (data only -- no reference source travels):
  step_reduced_64_sn_smooth.{json,npz}     reduced width, 64x64, B=2, focus_epsilon 0.5, float64 reference;
  step_full_64_sn_smooth.{json,npz}        the same at the shipped width (dis.dim 64: SN matrices up to 512 x 4096, gen.dim 64):
      npz: x_a, x_b, z0..z5 (the initial state is tests/sn_nets.py: sn_test_nets(config, seed)),
           uv_dis/<net>/<key>, uv_gen/<net>/<key>   weight_u / weight_v after that update (each from init),
           seq_uv/<net>/<key>    weight_u / weight_v after the three chained steps (reduced width only)
      json: config, losses (16), grad_stats (sum, norm, max of every gradient of both updates), param_stats_after_dis
            (the discriminator parameters after dis_update + Adam), sigma sequences per update ("sigma_dis" / "sigma_gen": one list per
            discriminator, one entry per forward call, each the sigma of its SN layers in (scale, layer) order, recovered
            from module.weight after the call), seq_losses (three chained dis -> gen steps, train.py order)
  state_dict_keys_sn.txt                     keys and shapes of the full-width SN trainer
  ckpt_reference_reduced_sn/                 a checkpoint written by the reference (reduced width, two layers per discriminator
                                             scale, after one dis_update) and expect.json: its config and the next dis_update's
                                             loss_dis_total (float32 reference)
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (shims + the reference modules)

sys.path.insert(0, os.path.dirname(HERE))
from sn_nets import sn_test_nets  # noqa: E402  (the seeded initial state, rebuilt by the tests without the reference)

ref_trainer, ref_networks = G.ref_trainer, G.ref_networks
NETS = ("gen_AB", "gen_BA", "dis_A", "dis_B", "dis_2")
DIS = ("dis_A", "dis_B", "dis_2")


def sn_config(reduced=True):
    cfg = G.reduced_config() if reduced else G.base_config()
    cfg["dis"]["norm"] = "sn"
    return cfg


class SigmaLog:
    """records sigma = <W_bar, W> / <W, W> of every SpectralNorm forward (module.weight = W_bar / sigma after the call)"""

    def __init__(self, tr):
        self.names = {}
        for net in DIS:
            for k, m in getattr(tr, net).named_modules():
                if isinstance(m, ref_networks.SpectralNorm):
                    self.names[id(m)] = (net, k)
        self.log = []
        self._orig = ref_networks.SpectralNorm.forward

    def __enter__(self):
        log, names, orig = self.log, self.names, self._orig

        def fwd(m, *a):
            out = orig(m, *a)
            w, wb = m.module.weight.detach().double(), m.module.weight_bar.detach().double()
            log.append((names[id(m)], float((wb * w).sum() / (w * w).sum())))
            return out
        ref_networks.SpectralNorm.forward = fwd
        return self

    def __exit__(self, *exc):
        ref_networks.SpectralNorm.forward = self._orig

    def per_call(self, nlayers):
        """{net: [[sigma of each SN layer] per forward call]} (consecutive records of one net = one call)"""
        out = {n: [] for n in DIS}
        cur = {n: [] for n in DIS}
        for (net, _), s in self.log:
            cur[net].append(s)
            if len(cur[net]) == nlayers:
                out[net].append(cur[net])
                cur[net] = []
        assert all(not v for v in cur.values())
        return out


def uv(tr, prefix, out):
    for net in DIS:
        for k, v in getattr(tr, net).state_dict().items():
            if k.endswith(("weight_u", "weight_v")):
                out["%s/%s/%s" % (prefix, net, k)] = v.detach().float().numpy().copy()


def run_sn_fixture(cfg, B, H, W, seed, fname, seq_uv=True):
    dd = torch.float64
    init = sn_test_nets(cfg, seed)
    x_a, x_b, z = G.seeded_inputs(B, H, W, seed)
    xa, xb, zd = x_a.to(dd), x_b.to(dd), [t.to(dd) for t in z]
    out = {"x_a": x_a.numpy(), "x_b": x_b.numpy()}
    for i, t in enumerate(z):
        out["z%d" % i] = t.numpy()
    nl = (cfg["dis"]["n_layer"] - 1) * cfg["dis"]["num_scales"]
    meta = {"config": cfg, "B": B, "H": H, "W": W, "seed": seed, "dtype": "float64 reference", "losses": {}, "grad_stats": {},
            "sigma_dis": {}, "sigma_gen": {}, "seq_losses": [], "param_stats_after_dis": {}}

    def fresh():
        tr = ref_trainer.aclgan_Trainer(cfg)
        for n in NETS:
            mod = getattr(tr, n)
            sd = mod.state_dict()
            for k, v in init[n].items():
                assert sd[k].shape == v.shape, (n, k, sd[k].shape, v.shape)
                sd[k] = v.clone()
            mod.load_state_dict(sd)
        return tr.double()

    tr = fresh()
    with SigmaLog(tr) as sl, G.RandnQueue(zd[:3]):
        tr.dis_update(xa, xb, cfg)
    meta["sigma_dis"] = sl.per_call(nl)
    for n in G.LOSS_NAMES_DIS:
        meta["losses"][n] = float(getattr(tr, n).detach())
    for net in DIS:
        for k, p in getattr(tr, net).named_parameters():
            if p.grad is None:
                continue
            meta["grad_stats"]["dis_update/%s/%s" % (net, k)] = G.tstats(p.grad)
            meta["param_stats_after_dis"]["%s/%s" % (net, k)] = G.tstats(p)
    uv(tr, "uv_dis", out)

    tr = fresh()
    with SigmaLog(tr) as sl, G.RandnQueue(zd[3:6]):
        tr.gen_update(xa, xb, cfg)
    meta["sigma_gen"] = sl.per_call(nl)
    for n in G.LOSS_NAMES_GEN:
        if hasattr(tr, n):
            meta["losses"][n] = float(getattr(tr, n).detach())
    for net in ("gen_AB", "gen_BA"):
        for k, p in getattr(tr, net).named_parameters():
            meta["grad_stats"]["gen_update/%s/%s" % (net, k)] = G.tstats(p.grad)
    uv(tr, "uv_gen", out)

    # three chained steps in the train.py order (dis, then gen on the updated weights), the same batch and noise each step
    tr = fresh()
    for _ in range(3):
        with G.RandnQueue(zd[:3]):
            tr.dis_update(xa, xb, cfg)
        with G.RandnQueue(zd[3:6]):
            tr.gen_update(xa, xb, cfg)
        meta["seq_losses"].append({n: float(getattr(tr, n).detach()) for n in G.LOSS_NAMES_DIS + G.LOSS_NAMES_GEN if hasattr(tr, n)})
    if seq_uv:      # (the full-width fixture leaves them out: 300 KB of float32 that would bring its npz to the 1 MiB file limit)
        uv(tr, "seq_uv", out)

    np.savez_compressed(os.path.join(HERE, fname + ".npz"), **out)
    json.dump(meta, open(os.path.join(HERE, fname + ".json"), "w"), indent=1, sort_keys=True)
    print("%s: losses %s" % (fname, {k: round(v, 5) for k, v in meta["losses"].items()}))


def key_list_sn():
    tr = ref_trainer.aclgan_Trainer(sn_config(reduced=False))
    lines = []
    for name in NETS:
        for k, v in getattr(tr, name).state_dict().items():
            lines.append("%s %s %s" % (name, k, "x".join(str(s) for s in v.shape)))
    open(os.path.join(HERE, "state_dict_keys_sn.txt"), "w").write("\n".join(lines) + "\n")


def checkpoint_config():
    """the reduced width with two layers per discriminator scale (one SN layer each): the checkpoint stays small"""
    cfg = sn_config()
    cfg["dis"]["n_layer"] = 2
    return cfg


def checkpoint_fixture_sn():
    """laid out like ckpt_reference_reduced (make_golden.checkpoint_fixture), with dis.norm: sn, after one dis_update (the Adam state of
    dis_opt -- bias then weight_bar of every SN layer -- is populated, gen_opt's is empty: the files stay small)"""
    cfg = checkpoint_config()
    torch.manual_seed(5)
    tr = ref_trainer.aclgan_Trainer(cfg)
    x_a, x_b, z = G.seeded_inputs(2, 64, 64, 1)
    with G.RandnQueue(z[:3]):
        tr.dis_update(x_a, x_b, cfg)
    d = os.path.join(HERE, "ckpt_reference_reduced_sn")
    os.makedirs(d, exist_ok=True)
    tr.save(d, 6)
    files = sorted(os.listdir(d))
    with G.RandnQueue(z[:3]):
        tr.dis_update(x_a, x_b, cfg)
    meta = {"config": cfg, "loss_dis_total_after_resume": float(tr.loss_dis_total.detach()), "files": files}
    json.dump(meta, open(os.path.join(d, "expect.json"), "w"), indent=1)
    print("SN checkpoint fixture:", meta)


if __name__ == "__main__":
    # python make_golden_sn.py [keys] [reduced] [full] [ckpt]   (no argument: all of them)
    which = set(sys.argv[1:]) or {"keys", "reduced", "full", "ckpt"}
    if "keys" in which:
        key_list_sn()
    if "reduced" in which:
        smooth = sn_config(); smooth["focus_epsilon"] = 0.5
        run_sn_fixture(smooth, 2, 64, 64, 11, "step_reduced_64_sn_smooth")
    if "full" in which:
        smooth = sn_config(reduced=False); smooth["focus_epsilon"] = 0.5
        run_sn_fixture(smooth, 2, 64, 64, 12, "step_full_64_sn_smooth", seq_uv=False)
    if "ckpt" in which:
        checkpoint_fixture_sn()
    print("spectral-norm fixtures written to", HERE)
