"""The nine architectures beside the default one that the arch-space tests build (tests/test_oracle_arch_space_cpu.py,
tests/test_arch_space_cpu.py, tests/test_gpu_arch_space.py) and tests/golden/make_golden.py pins to the reference: every
axis aclgan_ctx_create admits moved off the value all other tests use.  Data and seeded inputs only."""
import torch

from oracle import aclgan_oracle as O

# name -> (gen: dim, mlp_dim, style_dim, n_downsample, n_res), (dis: dim, n_layer, num_scales), (B, H, W)
ARCHS = {
    "dis12": ((8, 16, 8, 2, 1), (12, 4, 3), (2, 64, 64)),
    "dis48_l3_s2": ((8, 16, 8, 2, 1), (48, 3, 2), (3, 64, 96)),
    "dis96": ((8, 16, 8, 2, 1), (96, 4, 3), (2, 64, 64)),
    "down1": ((16, 24, 8, 1, 1), (8, 4, 3), (2, 66, 70)),
    "down3_style5": ((8, 20, 5, 3, 2), (8, 4, 3), (2, 64, 72)),
    "scales5_l2": ((8, 16, 8, 2, 1), (8, 2, 5), (2, 64, 64)),
    "scales4_l3": ((8, 16, 8, 2, 1), (8, 3, 4), (2, 64, 64)),
    "layer1": ((8, 16, 8, 2, 1), (20, 1, 4), (2, 64, 64)),
    "gen128": ((128, 64, 8, 2, 1), (8, 4, 3), (1, 64, 64)),
}
NET_SEED, INPUT_SEED = 3, 9


def arch_config(name, base=None):
    (gd, md, sd, nd, nr), (dd, nl, ns), _ = ARCHS[name]
    cfg = O.default_config() if base is None else base
    cfg["gen"].update(dim=gd, mlp_dim=md, style_dim=sd, n_downsample=nd, n_res=nr)
    cfg["dis"].update(dim=dd, n_layer=nl, num_scales=ns)
    cfg["display_size"] = 1
    cfg["focus_epsilon"] = 0.5
    return cfg


def arch_shape(name):
    return ARCHS[name][2]


def arch_inputs(name, seed=INPUT_SEED):
    """x_a, x_b and six style codes of the architecture's own style_dim, from one seeded generator"""
    B, H, W = ARCHS[name][2]
    sd = ARCHS[name][0][2]
    g = torch.Generator().manual_seed(seed)
    x_a = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    x_b = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    z = [torch.randn(B, sd, 1, 1, generator=g) for _ in range(6)]
    return x_a, x_b, z
