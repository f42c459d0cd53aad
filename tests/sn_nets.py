"""The seeded initial state of the spectral-norm fixtures (tests/golden/make_golden_sn.py) and of the tests that replay them.

The reference is not needed to rebuild it: every tensor comes from the oracle's seeded test fill (oracle.test_nets of the same
configuration with dis.norm none), the weight / bias of each spectrally normalised layer become its `conv.module.weight_bar` /
`conv.module.bias`, and `weight_u` / `weight_v` are drawn from N(0, 1) with a seeded generator and l2-normalised
(networks.py:571-574).  Keys and layouts are the reference's state_dict (v in (ci, kh, kw) order)."""
import copy

import torch

from oracle import aclgan_oracle as O


def sn_test_nets(cfg, seed):
    plain = copy.deepcopy(cfg)
    plain["dis"]["norm"] = "none"
    nets = O.test_nets(plain, seed)
    n_layer = int(cfg["dis"]["n_layer"])
    g = torch.Generator().manual_seed(1000 + seed)
    out = {}
    for name, sd in nets.items():
        if not name.startswith("dis"):
            out[name] = dict(sd)
            continue
        new = {}
        for k in sorted(sd, key=lambda k: (k.split(".")[:3], not k.endswith("bias"))):
            p = k.split(".")
            if len(p) == 5 and p[3] == "conv" and 0 < int(p[2]) < n_layer:
                pre = "cnns.%s.%s.conv.module." % (p[1], p[2])
                if p[4] == "bias":
                    new[pre + "bias"] = sd[k]
                else:
                    w = sd[k]
                    u = torch.randn(w.shape[0], generator=g, dtype=torch.float64)
                    v = torch.randn(w[0].numel(), generator=g, dtype=torch.float64)
                    new[pre + "weight_u"] = (u / (u.norm() + 1e-12)).float()
                    new[pre + "weight_v"] = (v / (v.norm() + 1e-12)).float()
                    new[pre + "weight_bar"] = w
            else:
                new[k] = sd[k]
        out[name] = new
    return out
