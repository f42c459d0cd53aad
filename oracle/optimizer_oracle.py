"""fp64 model of the optimizer step (aclgan_adam_step, include/aclgan_hip.h): torch.optim.Adam as the reference configures it
(trainer.py:39-42: L2 weight decay added to the gradient, betas (0.5, 0.999), eps 1e-8 outside the square root) and the fp16
dynamic loss-scale state machine of aclgan_bind_loss_scale.

Written from the reference's optimizer semantics and from the contract in the header, not from the kernels: the tests compare
the kernels with THIS, and tests/test_optimizer_oracle_cpu.py compares this with torch.optim.Adam in fp64 and with a transition
table written by hand, so that the checker is itself checked on a machine without a GPU.

  Adam64          AdamState (oracle/aclgan_oracle.py) on fp64 copies of one flat buffer, bias-correction step passed explicitly
  TorchAdam32     torch's own fp32 torch.optim.Adam on the same inputs: the optimizer the reference runs, used as the yardstick
                  of what fp32 arithmetic costs against the fp64 run
  parity_metrics  the three error figures both are measured with (no element excluded)
  LossScaleModel  the eight state floats over a sequence of adam_step(group, grads_nonfinite) events
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from .aclgan_oracle import AdamState

EPS32 = 2.0 ** -23
SCALE_MAX = 2.0 ** 24
DEFAULT_GROWTH_INTERVAL = 2000.0


def f32(x: float) -> float:
    """the value a C float holds for x, as a Python float: the hyper-parameters cross the C ABI as floats (aclgan_adam), so every
    side of a comparison is fed the rounded value"""
    return float(np.float32(x))


class Adam64:
    """torch.optim.Adam semantics in fp64 over one flat buffer.  p0, and every g passed to step(), may be fp32 tensors on any
    device; they are converted exactly.  `gmax` / `gvmax` keep each element's largest |g| and |g + weight_decay * p| over the
    sequence (normalisers of the first-moment error, which cancels)."""

    def __init__(self, p0: torch.Tensor, beta1: float, beta2: float, eps: float, weight_decay: float,
                 m0: Optional[torch.Tensor] = None, v0: Optional[torch.Tensor] = None):
        self.p = p0.detach().double().clone()
        self.st = AdamState([self.p], 0.0, beta1, beta2, weight_decay, eps)
        if m0 is not None:
            self.st.m[0].copy_(m0.double())
        if v0 is not None:
            self.st.v[0].copy_(v0.double())
        self.gmax = torch.zeros_like(self.p)
        self.gvmax = torch.zeros_like(self.p)
        self.applied = 0

    @property
    def m(self):
        return self.st.m[0]

    @property
    def v(self):
        return self.st.v[0]

    def step(self, g: torch.Tensor, lr: float, t: Optional[int] = None):
        """one APPLIED update with bias-correction step t (default: the number of applied updates, this one included)"""
        g = g.detach().double()
        self.applied += 1
        self.gmax = torch.maximum(self.gmax, g.abs())
        self.gvmax = torch.maximum(self.gvmax, (g + self.st.wd * self.p).abs())
        self.st.step([g], lr=lr, t=self.applied if t is None else t)


class TorchAdam32:
    """torch.optim.Adam in fp32 on the CPU over one flat buffer (weight_decay = classic L2, amsgrad off)"""

    def __init__(self, p0: torch.Tensor, beta1: float, beta2: float, eps: float, weight_decay: float):
        self.p = p0.detach().float().cpu().clone().requires_grad_(True)
        self.opt = torch.optim.Adam([self.p], lr=1.0, betas=(beta1, beta2), eps=eps, weight_decay=weight_decay)

    def step(self, g: torch.Tensor, lr: float):
        self.opt.param_groups[0]["lr"] = lr
        self.p.grad = g.detach().float().cpu().clone()
        self.opt.step()

    @property
    def m(self):
        return self.opt.state[self.p]["exp_avg"]

    @property
    def v(self):
        return self.opt.state[self.p]["exp_avg_sq"]


def parity_metrics(p: torch.Tensor, m: torch.Tensor, v: torch.Tensor, ref: Adam64, lr: float, T: int) -> Dict[str, float]:
    """Errors of an fp32 (p, m, v) against the fp64 run `ref` after T applied updates, maxima over ALL elements:
      p      |p - p64| / (lr * 1e-6 + T * 2^-23 * |p64|)     (one rounding of p per step, plus the step itself at 1e-6 of lr)
      v      |v - v64| / v64                                  (a sum of non-negative terms: relative error is meaningful everywhere)
      m      |m - m64| / max_t |g_t|                          (m cancels: its error scales with what went in, not with what is left)
      m_eff  |m - m64| / max_t |g_t + weight_decay * p_t|     (the same with the decay term counted in)"""
    dev = ref.p.device
    p = p.detach().to(dev).double(); m = m.detach().to(dev).double(); v = v.detach().to(dev).double()
    tiny = 1e-300
    out = {
        "p": ((p - ref.p).abs() / (lr * 1e-6 + T * EPS32 * ref.p.abs())).max().item(),
        "v": torch.where(ref.v > 0, (v - ref.v).abs() / ref.v.clamp_min(tiny), v.abs() * 1e300).max().item(),
        "m": ((m - ref.m).abs() / ref.gmax.clamp_min(tiny)).max().item(),
        "m_eff": ((m - ref.m).abs() / ref.gvmax.clamp_min(tiny)).max().item(),
    }
    return out


METRICS = ("p", "v", "m", "m_eff")


class LossScaleModel:
    """The eight floats of aclgan_bind_loss_scale, driven by adam_step(group, grads_nonfinite):

      state[7] <- S (the scale this update's gradient buffers carry)
      non-finite gradients:  S <- max(S / 2, 1), clean <- 0, skipped[group] += 1, the update is NOT applied
      otherwise:             clean += 1; clean >= interval (0 means 2000): S <- min(2 S, 2^24), clean <- 0
      state[1] <- 1 / S (fp32), state[3] <- 0

    The clean counter is shared by both groups; the skip counters are per group.  The bias-correction step of an applied update
    is the host's step count minus that group's skips."""

    def __init__(self, scale: float, interval: float = 0.0, clean: float = 0.0, skipped=(0.0, 0.0), last: float = 0.0):
        self.state: List[float] = [float(scale), f32(1.0 / scale), float(clean), 0.0, float(skipped[0]), float(skipped[1]), float(interval), float(last)]

    def adam_step(self, group: int, grads_nonfinite: bool) -> bool:
        """returns True when the update is applied"""
        s = self.state
        s[7] = s[0]
        if grads_nonfinite:
            s[0] = max(s[0] / 2.0, 1.0)
            s[2] = 0.0
            s[4 + group] += 1.0
        else:
            s[2] += 1.0
            if s[2] >= (s[6] if s[6] > 0 else DEFAULT_GROWTH_INTERVAL):
                s[0] = min(2.0 * s[0], SCALE_MAX)
                s[2] = 0.0
        s[1] = float(np.float32(1.0) / np.float32(s[0]))
        s[3] = 0.0
        return not grads_nonfinite

    def bias_correction_step(self, group: int, host_step: int) -> int:
        return host_step - int(self.state[4 + group])
