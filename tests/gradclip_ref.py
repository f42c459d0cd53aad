"""fp64 model of an optimizer step with a gradient-clip state bound (include/aclgan_hip.h: aclgan_bind_grad_clip), written around
oracle.optimizer_oracle.Adam64 and LossScaleModel.  The rule, once:

  norm   = sqrtf(sum_i (g_i / S)^2), g the buffer as the device holds it, S the bound loss scale or 1
  fp16 overflow (some g_i non-finite under a loss scale): the loss-scale machine skips, halves and counts; clip = [norm, 0, same, same]
  norm not finite otherwise: a clip-skip, nothing written; clip = [norm, 0, same, skipped + 1]
  else   coef = min(1, max_norm / (norm + 1e-6)); clipped += coef < 1; Adam with g / S * coef (weight decay after the clip)
  bias-correction step = host step - loss-scale skips of the group - clip skips of the group

Not a test module: tests/test_gradclip_cpu.py checks it against torch, tests/test_gpu_gradclip.py checks the kernels against it."""
import math

import numpy as np
import torch

from oracle import optimizer_oracle as M


def index_values(n, salt, lo_exp=-6.0, hi_exp=0.0, device="cpu"):
    """a deterministic function of the element index: magnitudes 10^lo_exp .. 10^hi_exp, mixed signs (fp64)"""
    i = torch.arange(n, device=device, dtype=torch.int64)
    h = ((i + salt) * 2654435761) % 1048573
    s = (((i + 7 * salt) * 40503) % 65521) % 2
    return 10.0 ** (lo_exp + (hi_exp - lo_exp) * h.double() / 1048573.0) * (2.0 * s.double() - 1.0)


def norm_f32(g, inv=1.0):
    """sqrtf of the fp32-rounded sum of squares, the sum itself in fp64: (norm as a Python float, the fp64 norm)"""
    n2 = float((g.double() * inv).pow(2).sum())
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.sqrt(np.float32(n2))), (math.sqrt(n2) if math.isfinite(n2) else n2)


def clip_rule(norm, max_norm):
    """coef of a finite norm in fp32 arithmetic, torch's formula"""
    with np.errstate(over="ignore", divide="ignore"):
        return float(min(np.float32(1.0), np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6))))


class ClipModel:
    """one group: Adam64 + the four leading floats of the clip state (+ optionally the average), driven by step(buffer, lr, host_step)"""

    def __init__(self, p0, b1, b2, eps, wd, max_norm, group=0, loss_scale=None, ema=None, count_skips=True):
        self.adam = M.Adam64(p0, b1, b2, eps, wd)
        self.max_norm, self.group, self.ls = float(max_norm), group, loss_scale
        self.state = [0.0, 0.0, 0.0, 0.0]
        self.ema = None if ema is None else ema.detach().double().clone()
        self.count_skips = count_skips      # False: the WRONG model whose bias correction ignores the clip skips (tests show the kernels differ from it)
        self.norm64 = 0.0

    def bias_correction_step(self, host_step):
        ls_skips = int(self.ls.state[4 + self.group]) if self.ls is not None else 0
        return host_step - ls_skips - (int(self.state[3]) if self.count_skips else 0)

    def step(self, gbuf, lr, host_step, decay=None, blend=True):
        """returns True when the update is applied"""
        inv = self.ls.state[1] if self.ls is not None else 1.0
        norm, self.norm64 = norm_f32(gbuf, inv)
        self.state[0] = norm
        overflow = self.ls is not None and not bool(torch.isfinite(gbuf).all())
        if self.ls is not None:
            self.ls.adam_step(self.group, overflow)
        if overflow or not math.isfinite(norm):
            self.state[1] = 0.0
            if not overflow:
                self.state[3] += 1.0
            return False
        coef = clip_rule(norm, self.max_norm)
        self.state[1] = coef
        if coef < 1.0:
            self.state[2] += 1.0
        # (the loss-scale model has already counted this call: an applied update leaves the skip counts as they were)
        self.adam.step(gbuf.double() * inv * coef, lr, t=self.bias_correction_step(host_step))
        if self.ema is not None:
            self.ema = decay * self.ema + (1.0 - decay) * self.adam.p if blend else self.adam.p.clone()
        return True
