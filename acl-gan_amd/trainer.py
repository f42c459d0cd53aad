"""aclgan_Trainer -- drop-in counterpart of the reference's trainer.aclgan_Trainer
(reference trainer.py:14-331) running on libaclgan_hip.so.

Same constructor argument (the YAML dict), same methods (gen_update / dis_update / sample /
update_learning_rate / save / resume), same ``loss_*`` attributes (0-d tensors), same attribute
names for the five networks, same checkpoint file names / dict keys / state_dict key names
(OIHW fp32 weights on disk; the OHWI <-> OIHW repack happens here, at the boundary).

PyTorch's role: device memory (flat parameter / gradient / Adam-state buffers, workspace),
the current stream, torch.save/torch.load, torch.distributed.  All arithmetic of the step is in
the HIP library; if it is missing the import of this package fails -- there is no fallback.
"""
import ctypes as C
import math
import os
from collections import OrderedDict
from contextlib import contextmanager

import torch

from . import _lib as L

__all__ = ["aclgan_Trainer", "AdaINGen", "MsImageDis", "ada_from_config", "arch_from_config", "augment_from_config", "dis_norm_from_config", "draw_augment_params",
           "ema_from_config", "grad_clip_from_config", "hparams_from_config", "lecam_from_config", "modeseek_from_config", "r1_from_config"]

DIS_NORMS = ("none", "sn")    # dis.norm values the library implements (sn: SpectralNorm, networks.py:360-361,538-600)


def dis_norm_from_config(hp):
    """dis.norm as the library's ACLGAN_NORM_* code (none -> 0, sn -> ACLGAN_NORM_SN)"""
    norm = hp["dis"].get("norm", "none")
    if norm not in DIS_NORMS:
        raise L.AclganError("dis.norm=%r unsupported (implemented: %s)" % (norm, ", ".join(DIS_NORMS)))
    return L.NORM[norm]


def arch_from_config(hp):
    g, d = hp["gen"], hp["dis"]
    for key, want in (("activ", "relu"), ("pad_type", "reflect")):
        if g.get(key, want) != want:
            raise L.AclganError("gen.%s=%r unsupported (only %r is reached by the shipped config)" % (key, g.get(key), want))
    for key, want in (("activ", "lrelu"), ("pad_type", "reflect"), ("gan_type", "lsgan")):
        if d.get(key, want) != want:
            raise L.AclganError("dis.%s=%r unsupported (only %r is reached by the shipped config)" % (key, d.get(key), want))
    dis_norm_from_config(hp)
    return L.Arch(int(hp["input_dim_a"]), int(hp["input_dim_b"]), int(g["dim"]), int(g["mlp_dim"]), int(g["style_dim"]),
                  int(g["output_dim"]), int(g["n_downsample"]), int(g["n_res"]), int(d["dim"]), int(d["n_layer"]),
                  int(d["num_scales"]))


def ema_from_config(hp):
    """The averaged generator's keys (not in the reference) as (decay, start, display):
    ema_decay   float in [0, 1), default 0 = off: no buffer, no extra call, the launches of a run without the keys;
    ema_start   int >= 0, default 0: the generator updates 1 .. ema_start copy the weights into the average, later ones blend;
    ema_display bool, default false: train.py's pictures are sampled from the average (needs ema_decay > 0)."""
    decay, start, display = hp.get("ema_decay", 0), hp.get("ema_start", 0), hp.get("ema_display", False)
    if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not (0 <= decay and C.c_float(decay).value < 1):
        raise L.AclganError("ema_decay=%r: expected a number in [0, 1) (0 switches the averaged generator off)" % (decay,))
    if isinstance(start, bool) or not isinstance(start, int) or start < 0:
        raise L.AclganError("ema_start=%r: expected an integer >= 0" % (start,))
    if not isinstance(display, bool):
        raise L.AclganError("ema_display=%r: expected true or false" % (display,))
    if display and not decay > 0:
        raise L.AclganError("ema_display: true needs ema_decay > 0 (there is no averaged generator to sample from)")
    return float(decay), start, display


def augment_from_config(hp):
    """dis_augment (not in the reference): a comma-separated subset of color,translation,cutout -- the differentiable augmentation every
    discriminator input of both updates goes through (Zhao et al. 2020) -- as the library's ACLGAN_AUG_* policy bits.  Default "" = 0 = off:
    no buffer, no extra library call, the launches of a run without the key."""
    v = hp.get("dis_augment", "")
    if not isinstance(v, str):
        raise L.AclganError("dis_augment=%r: expected a string, a comma-separated subset of %s" % (v, ",".join(L.AUG)))
    policy = 0
    if v.strip() == "":
        return policy
    for name in (t.strip() for t in v.split(",")):
        if name not in L.AUG or policy & L.AUG[name]:
            raise L.AclganError("dis_augment=%r: %r is %s (expected a comma-separated subset of %s)"
                                % (v, name, "named twice" if name in L.AUG else "unknown", ",".join(L.AUG)))
        policy |= L.AUG[name]
    return policy


def r1_from_config(hp):
    """The R1 gradient penalty's keys (not in the reference; Mescheder et al. 2018, in StyleGAN2's lazy form) as (gamma, every):
    r1_gamma  float >= 0, default 0 = off: no buffer, no library call, the launches and bits of a run without the keys;
    r1_every  int >= 1, default 16: the pass runs on every r1_every-th discriminator update, with gamma * r1_every.
    The penalty gamma/2 E||grad_x D(x)||^2 is taken on the real batches: dis_A on x_a, dis_B on x_b (dis_2 never sees a real image).
    Refused with r1_gamma > 0: dis.norm sn (the pass does not fold through sigma) and dis_augment (the pass does not wrap the augmentation)."""
    gamma, every = hp.get("r1_gamma", 0), hp.get("r1_every", 16)
    if isinstance(gamma, bool) or not isinstance(gamma, (int, float)) or not (0 <= gamma and math.isfinite(C.c_float(gamma).value)):
        raise L.AclganError("r1_gamma=%r: expected a finite number >= 0 (0 switches the R1 penalty off)" % (gamma,))
    if isinstance(every, bool) or not isinstance(every, int) or every < 1:
        raise L.AclganError("r1_every=%r: expected an integer >= 1" % (every,))
    if gamma > 0 and not math.isfinite(C.c_float(gamma * every).value):
        raise L.AclganError("r1_gamma * r1_every = %r is no finite fp32 number" % (gamma * every,))
    if gamma > 0 and hp.get("dis", {}).get("norm", "none") == "sn":
        raise L.AclganError("r1_gamma > 0 with dis.norm: sn is not implemented (follow-up: fold the penalty through sigma and the "
                            "power-iteration state); use dis.norm: none")
    if gamma > 0 and augment_from_config(hp):
        raise L.AclganError("r1_gamma > 0 with dis_augment is not implemented (follow-up: aclgan_diffaugment_fwd / _bwd around the R1 pass, "
                            "the penalty through the affine augmentation); leave one of the two keys out")
    return float(gamma), every


def lecam_from_config(hp):
    """The LeCam regulariser's keys (not in the reference; Tseng et al. 2021, eq. 7, two-sided, on the LSGAN outputs) as (lambda, decay, start):
    lecam_lambda  float >= 0, default 0 = off: no buffer, no library call, the launches and bits of a run without the keys;
    lecam_decay   float in [0, 1), default 0.99: the decay of the two anchors per discriminator and scale (mean D on real, mean D on fake);
    lecam_start   int >= 0, default 1000: the anchors are tracked from the first discriminator update, the term acts from update start + 1 on
                  (never on the first: it has no anchors yet).
    The defaults are this project's choice; nobody has measured which values suit these datasets (README).  It composes with dis.norm sn,
    dis_augment, r1_gamma and ema_decay: it only looks at discriminator outputs."""
    lam, decay, start = hp.get("lecam_lambda", 0), hp.get("lecam_decay", 0.99), hp.get("lecam_start", 1000)
    if isinstance(lam, bool) or not isinstance(lam, (int, float)) or not (0 <= lam and math.isfinite(C.c_float(lam).value)):
        raise L.AclganError("lecam_lambda=%r: expected a finite number >= 0 (0 switches the LeCam regulariser off)" % (lam,))
    if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not (0 <= decay and C.c_float(decay).value < 1):
        raise L.AclganError("lecam_decay=%r: expected a number in [0, 1)" % (decay,))
    if isinstance(start, bool) or not isinstance(start, int) or not 0 <= start < 2 ** 31:
        raise L.AclganError("lecam_start=%r: expected an integer >= 0 (below 2**31)" % (start,))
    return float(lam), float(decay), start


def ada_from_config(hp):
    """The adaptive-augmentation keys (not in the reference; Karras et al. 2020, "Training GANs with Limited Data", ADA; README / DESIGN.md
    section 4h) as None (dis_augment_p absent: no buffer, no library call, the launches and bits of a run without the keys) or
    (p0, adaptive, target, interval, kimg):
    dis_augment_p  a number in [0, 1]: every operation of dis_augment is applied to a discriminator input with that fixed probability, and the
                   overfitting signal r is monitored; or the string adaptive: p starts at 0 and is steered towards r = ada_target.
                   It needs a non-empty dis_augment.
    ada_target     number in [-1, 1], default 0.6     |
    ada_interval   int >= 1, default 4 dis updates    |  read only with adaptive (a fixed p closes its monitoring intervals at the defaults)
    ada_kimg       number > 0, default 500            |  p moves by ada_interval * B / (ada_kimg * 1000) per interval
    The three defaults are ADA's; nobody has measured which values suit these datasets (README)."""
    if "dis_augment_p" not in hp:
        return None
    v = hp["dis_augment_p"]
    adaptive = isinstance(v, str) and v.strip() == "adaptive"
    if not adaptive and (isinstance(v, bool) or not isinstance(v, (int, float)) or not (0 <= v <= 1)):
        raise L.AclganError("dis_augment_p=%r: expected a number in [0, 1] or the string adaptive" % (v,))
    if not augment_from_config(hp):
        raise L.AclganError("dis_augment_p=%r needs a non-empty dis_augment (a comma-separated subset of %s): there is nothing to apply with "
                            "that probability" % (v, ",".join(L.AUG)))
    target, interval, kimg = 0.6, 4, 500.0
    if adaptive:
        target, interval, kimg = hp.get("ada_target", target), hp.get("ada_interval", interval), hp.get("ada_kimg", kimg)
        if isinstance(target, bool) or not isinstance(target, (int, float)) or not (-1 <= target <= 1):
            raise L.AclganError("ada_target=%r: expected a number in [-1, 1]" % (target,))
        if isinstance(interval, bool) or not isinstance(interval, int) or not 1 <= interval < 2 ** 31:
            raise L.AclganError("ada_interval=%r: expected an integer >= 1 (below 2**31)" % (interval,))
        if isinstance(kimg, bool) or not isinstance(kimg, (int, float)) or not (kimg > 0 and math.isfinite(C.c_float(kimg).value)):
            raise L.AclganError("ada_kimg=%r: expected a finite number > 0" % (kimg,))
    return (0.0 if adaptive else float(v)), adaptive, float(target), interval, float(kimg)


def modeseek_from_config(hp):
    """The mode-seeking regulariser's key (not in the reference; Mao et al. 2019, "Mode Seeking GANs", per image; README / DESIGN.md section 4g):
    ms_lambda  float >= 0, default 0 = off: no buffer, no library call, the launches and bits of a run without the key.
    With it gen_update decodes c_1 and c_2 once more with fresh noise and the objective gains ms_lambda * (loss_gen_ms_B + loss_gen_ms_A),
    ms = mean over the batch of dz / (dI + 1e-5 dz).  The paper uses 1 throughout; nobody has measured which value suits these datasets.
    It composes with every other key: it never touches the discriminators or the finished gradient buffer.  grad_clip is its companion
    (the term grows like dz / dI^2 where two samples nearly coincide)."""
    lam = hp.get("ms_lambda", 0)
    if isinstance(lam, bool) or not isinstance(lam, (int, float)) or not (0 <= lam and math.isfinite(C.c_float(lam).value)):
        raise L.AclganError("ms_lambda=%r: expected a finite number >= 0 (0 switches the mode-seeking regulariser off)" % (lam,))
    return float(lam)


def grad_clip_from_config(hp):
    """The gradient-norm keys (not in the reference; torch.nn.utils.clip_grad_norm_ per optimizer group, on the device) as (gen, dis), the
    max_norm of each group, 0 = off:
    grad_clip      number > 0 or .inf, default 0 = off: no buffer, no library call, the launches and bits of a run without the keys.  Both groups.
                   .inf is monitor and guard: the norms are read out, nothing is clipped, an update with a non-finite norm is skipped;
    grad_clip_gen  optional override for the generators' group (0 switches that group off);
    grad_clip_dis  likewise for the discriminators' group.
    No bound is shipped: nobody has measured which suits these datasets (README: read the logged norms first).  It composes with dis.norm sn,
    dis_augment, r1_gamma, lecam_lambda, ema_decay, hip_graph and data-parallel runs: it only looks at the finished gradient buffer."""
    out = []
    for key in ("grad_clip", "grad_clip_gen", "grad_clip_dis"):
        if key not in hp:
            out.append(None if key != "grad_clip" else 0.0)
            continue
        v = hp[key]
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not (v >= 0) or (v > 0 and not C.c_float(v).value > 0):
            raise L.AclganError("%s=%r: expected a number > 0 or .inf (0 switches the gradient norm, the clip and the guard off)" % (key, v))
        out.append(float(v))
    both, gen, dis = out
    return (both if gen is None else gen, both if dis is None else dis)


AUG_SEED_OFFSET = 0x0A06           # the augmentation generator's seed = torch.initial_seed() + rank + this
MS_SEED_OFFSET = 0x0A07            # the mode-seeking noise generator's seed = torch.initial_seed() + rank + this
ADA_SEED_OFFSET = 0x0A08           # the gate's uniforms' generator's seed = torch.initial_seed() + rank + this


def draw_augment_params(policy, rows, H, W, generator=None):
    """(rows, 8) fp32 CPU tensor of augmentation parameters (b, s, c, tx, ty, cx, cy, 0), one row per discriminator input image, with
    DiffAugment's distributions (include/aclgan_hip.h: aclgan_diffaugment_fwd for what the columns do):
      color        b = U[0,1) - 0.5 (brightness), s = 2 U[0,1) (saturation), c = U[0,1) + 0.5 (contrast)
      translation  tx uniform on the integers [-Sx, Sx], Sx = int(W/8 + 0.5); ty likewise with H
      cutout       a (ch, cw) = ((H+1)//2, (W+1)//2) rectangle; oy uniform on the integers [0, H + (1 - ch % 2)), cy = oy - ch//2; cx likewise
    The columns of an operation that policy leaves out hold its neutral values: 0, 1, 1; 0, 0; a rectangle outside the frame (cx = W, cy = H).
    Draw order: b, s, c, tx, ty, cx, cy, each for all rows at once and only for the operations that are on."""
    if not (isinstance(policy, int) and 0 <= policy <= 7) or rows < 0 or H < 1 or W < 1:
        raise L.AclganError("draw_augment_params: bad arguments (policy %r, rows %r, H %r, W %r)" % (policy, rows, H, W))
    p = torch.zeros(rows, 8, dtype=torch.float32)
    p[:, 1] = 1.0
    p[:, 2] = 1.0
    p[:, 5] = float(W)
    p[:, 6] = float(H)
    g = generator
    if policy & L.AUG["color"]:
        p[:, 0] = torch.rand(rows, generator=g) - 0.5
        p[:, 1] = torch.rand(rows, generator=g) * 2.0
        p[:, 2] = torch.rand(rows, generator=g) + 0.5
    if policy & L.AUG["translation"]:
        sx, sy = int(W / 8 + 0.5), int(H / 8 + 0.5)
        p[:, 3] = torch.randint(-sx, sx + 1, (rows,), generator=g).float()
        p[:, 4] = torch.randint(-sy, sy + 1, (rows,), generator=g).float()
    if policy & L.AUG["cutout"]:
        ch, cw = (H + 1) // 2, (W + 1) // 2
        p[:, 5] = (torch.randint(0, W + (1 - cw % 2), (rows,), generator=g) - cw // 2).float()
        p[:, 6] = (torch.randint(0, H + (1 - ch % 2), (rows,), generator=g) - ch // 2).float()
    return p


def hparams_from_config(hp):
    """The per-call hyper-parameters gen_update / dis_update read (trainer.py:93-97,142-144,164,288-290)."""
    return L.HParams(float(hp["gan_w"]), float(hp["gan_cw"]), float(hp["recon_x_w"]), float(hp["focus_loss"]),
                     float(hp["focus_delta"]), float(hp["focus_upper"]), float(hp["focus_lower"]),
                     float(hp["focus_epsilon"]), float(hp.get("alpha", 1)))


class _Net:
    """A view of one network's tensors inside the flat group buffers, with the reference's
    state_dict surface."""

    def __init__(self, trainer, name):
        self._t = trainer
        self.name = name
        self.net_id = L.NETS[name]
        self.group = L.GROUP_GEN if name.startswith("gen") else L.GROUP_DIS
        self._entries = [e for e in trainer._tensors[self.group] if e["net"] == name]

    # ---- tensor access ----
    def _view(self, e, buf):
        flat = buf[e["offset"]: e["offset"] + e["numel"]]
        shp = e["shape"]
        if len(shp) == 4:   # OHWI in memory -> OIHW view (what the reference stores)
            co, ci, kh, kw = shp
            return flat.view(co, kh, kw, ci).permute(0, 3, 1, 2)
        return flat.view(*shp)

    def _named_views(self, buf):
        for e in self._entries:
            yield e["key"], self._view(e, buf)

    def named_parameters(self):
        return self._named_views(self._t._param[self.group])

    def named_grads(self):
        for e in self._entries:
            yield e["key"], self._view(e, self._t._grad[self.group])

    def parameters(self):
        return [p for _, p in self.named_parameters()]

    def state_dict(self):
        return self._state_dict_of(self._t._param[self.group])

    def _state_dict_of(self, buf):
        """the reference's state_dict with the parameters read from `buf` (the group's flat parameter buffer, or the generators' average)"""
        sd = OrderedDict()
        params = OrderedDict((k, v.contiguous().clone()) for k, v in self._named_views(buf))
        bufs = self._buffers()
        # reference ordering: per module, parameters then buffers
        for k in self._t._ref_key_order(self.name, list(params.keys()), list(bufs.keys())):
            sd[k] = params[k] if k in params else bufs[k]
        return sd

    def _buffers(self):
        return OrderedDict()

    def load_state_dict(self, sd, strict=True):
        self._t._carry_epoch += 1
        mine = OrderedDict(self.named_parameters())
        missing = [k for k in mine if k not in sd]
        unexpected = [k for k in sd if k not in mine and k not in self._buffers()]
        if strict and (missing or unexpected):
            raise L.AclganError("load_state_dict(%s): missing %s unexpected %s" % (self.name, missing, unexpected))
        with torch.no_grad():
            for k, v in mine.items():
                if k in sd:
                    src = sd[k].to(device=v.device, dtype=torch.float32)
                    if tuple(src.shape) != tuple(v.shape):
                        raise L.AclganError("load_state_dict(%s): shape mismatch for %s: %s vs %s" % (self.name, k, tuple(src.shape), tuple(v.shape)))
                    v.copy_(src)
        for k in self._buffers():
            if k in sd:
                self._load_buffer(k, sd[k])

    def _load_buffer(self, key, value):
        self._t._dummy_buffers[self.name][key] = value.detach().clone().cpu()

    def cuda(self, *a, **k):
        return self

    def eval(self):
        return self

    def train(self, mode=True):
        return self


class AdaINGen(_Net):
    """reference networks.py:112-171 -- encode / decode on the HIP forward path."""

    def _buffers(self):
        return self._t._dummy_buffers[self.name]

    def encode(self, images):
        t = self._t
        images = images.to(t.device, torch.float32).contiguous()
        B, Cin, H, W = images.shape
        a = t.arch
        q = 1 << a.gen_n_downsample
        content = torch.empty(B, a.gen_dim * q, H // q, W // q, device=t.device)
        style = torch.empty(B, a.gen_style_dim, 1, 1, device=t.device)
        with torch.cuda.device(t.device):
            t._ensure_workspace(B, H, W, forward_only=True)
            L.check(L.lib.aclgan_gen_encode(t._ctx, self.net_id, L.ptr(images), B, H, W, L.ptr(content), L.ptr(style), t._st()), "gen_encode")
        return content, style

    def decode(self, content, style):
        t = self._t
        content = content.to(t.device, torch.float32).contiguous()
        style = style.to(t.device, torch.float32).contiguous()
        B, Cc, h, w = content.shape
        a = t.arch
        q = 1 << a.gen_n_downsample
        out = torch.empty(B, a.gen_output_dim, h * q, w * q, device=t.device)
        with torch.cuda.device(t.device):
            t._ensure_workspace(B, h * q, w * q, forward_only=True)
            L.check(L.lib.aclgan_gen_decode(t._ctx, self.net_id, L.ptr(content), L.ptr(style), B, h, w, L.ptr(out), t._st()), "gen_decode")
        return out

    def forward(self, images):
        content, style = self.encode(images)
        return self.decode(content, style)

    __call__ = forward


class MsImageDis(_Net):
    """reference networks.py:21-106 -- forward (list of per-scale maps) on the HIP path.  Under dis.norm: sn every forward call runs one
    power iteration of the spectrally normalised layers (u / v advance, networks.py:547-559), as the reference's does."""

    def _sn_entries(self):
        return [e for e in self._t._tensors.get(L.GROUP_SN_STATE, []) if e["net"] == self.name]

    def _sn_view(self, e):
        """weight_u as stored; weight_v permuted from the library's (kh, kw, ci) column order to the reference's (ci, kh, kw)"""
        flat = self._t._sn_state[e["offset"]: e["offset"] + e["numel"]]
        if e["key"].endswith("weight_v"):
            ci, kh, kw = e["vshape"]
            return flat.view(kh, kw, ci).permute(2, 0, 1).reshape(-1)
        return flat

    def _buffers(self):
        return OrderedDict((e["key"], self._sn_view(e).clone()) for e in self._sn_entries())

    def load_state_dict(self, sd, strict=True):
        missing = [e["key"] for e in self._sn_entries() if e["key"] not in sd]
        if strict and missing:
            raise L.AclganError("load_state_dict(%s): missing %s" % (self.name, missing))
        super().load_state_dict(sd, strict=strict)

    def _load_buffer(self, key, value):
        e = next(e for e in self._sn_entries() if e["key"] == key)
        src = value.detach().to(device=self._t.device, dtype=torch.float32).reshape(-1)
        if src.numel() != e["numel"]:
            raise L.AclganError("load_state_dict(%s): shape mismatch for %s: %s vs (%d,)" % (self.name, key, tuple(value.shape), e["numel"]))
        if key.endswith("weight_v"):
            ci, kh, kw = e["vshape"]
            src = src.view(ci, kh, kw).permute(1, 2, 0).reshape(-1)
        with torch.no_grad():
            self._t._sn_state[e["offset"]: e["offset"] + e["numel"]].copy_(src)

    def forward(self, x):
        t = self._t
        x = x.to(t.device, torch.float32).contiguous()
        B, Cin, H, W = x.shape
        a = t.arch
        outs = []
        h, w = H, W
        for s in range(a.dis_num_scales):
            hs, ws = h, w
            for _ in range(a.dis_n_layer):
                hs, ws = (hs + 2 - 4) // 2 + 1, (ws + 2 - 4) // 2 + 1
            outs.append(torch.empty(B, 1, hs, ws, device=t.device))
            h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        arr = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        with torch.cuda.device(t.device):
            t._ensure_workspace(B, H, W, forward_only=True)
            L.check(L.lib.aclgan_dis_forward(t._ctx, self.net_id, L.ptr(x), B, H, W, arr, t._st()), "dis_forward")
        return outs

    __call__ = forward


class aclgan_Trainer:
    """See module docstring.  Extra (optional) arguments over the reference: ``device``; and
    ``z=(z_1, z_2, z_3)`` on the update calls for seed-independent parity tests (by default z is
    drawn from the CPU generator exactly like trainer.py:99-101)."""

    def __init__(self, hyperparameters, device=None, compute_dtype=None, deterministic=None, hip_graph=None):
        if not torch.cuda.is_available():
            raise L.AclganError("aclgan_Trainer needs an MI355X (torch.cuda.is_available() is False); there is no CPU fallback")
        hp = hyperparameters
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        self.arch = arch_from_config(hp)
        self._ema_decay, self._ema_start, self.ema_display = ema_from_config(hp)
        self.augment = augment_from_config(hp)      # ACLGAN_AUG_* bits of dis_augment (0: off)
        # R1 penalty on the real batches (r1_gamma > 0): the device float[2] of the penalties and the pass's scratch are made by the first pass
        self.r1_gamma, self.r1_every = r1_from_config(hp)
        self.r1_passes = 0
        self._r1_pen = self._r1_scratch = None
        self._r1_after = False
        # compute dtype of the heavy convolutions (not in the reference, which is fp32 only): "fp32" | "bf16" | "fp16"
        self.compute_dtype = str(compute_dtype or hp.get("compute_dtype", "fp32"))
        if self.compute_dtype not in L.DTYPE:
            raise L.AclganError("compute_dtype=%r: expected one of %s" % (self.compute_dtype, sorted(L.DTYPE)))
        # deterministic=True (or config key "deterministic", or ACLGAN_DETERMINISTIC=1): every reduction takes an ordered path and a step
        # is reproducible bit for bit run to run (include/aclgan_hip.h: aclgan_set_deterministic).  Process-wide, like
        # torch.use_deterministic_algorithms; must be chosen before the workspaces are sized, i.e. here.
        det = deterministic if deterministic is not None else hp.get("deterministic", None)
        if det is not None:
            L.check(L.lib.aclgan_set_deterministic(1 if det else 0), "set_deterministic")
        self.deterministic = bool(L.lib.aclgan_get_deterministic())
        # hip_graph=True (or config key "hip_graph", or ACLGAN_GRAPH=1): the launch sequence of an update (zero_grad + forward +
        # losses + backward, ~1 000-2 000 kernels) is captured once per (shape, hyper-parameters, workspace) into a HIP graph and
        # replayed; Adam stays a separate launch (its step count is a kernel argument).  Same kernels in the same order: same
        # results.  Pays when the step is launch-bound (small batches / images); off by default.
        hg = hip_graph if hip_graph is not None else hp.get("hip_graph", os.environ.get("ACLGAN_GRAPH", "0") not in ("", "0"))
        self.hip_graph = bool(hg)
        self._graphs = {}
        self._ctx = C.c_void_p()
        L.check(L.lib.aclgan_ctx_create_dis_norm(C.byref(self.arch), dis_norm_from_config(hp), C.byref(self._ctx)), "ctx_create")
        L.check(L.lib.aclgan_set_compute_dtype(self._ctx, L.DTYPE[self.compute_dtype]), "set_compute_dtype")
        # dis_augment: the policy goes on the context before the first workspace query (the augmented tensors live in the arena); the rows
        # of an update are bound just before it (_bind_augment).  They come from a CPU generator of their own (seed: initial_seed() + rank +
        # AUG_SEED_OFFSET), so the z stream of a run is the same with and without augmentation; its state is not part of a checkpoint.
        self._auggen = None
        self._aug_dev = {}
        if self.augment:
            L.check(L.lib.aclgan_ctx_set_augment(self._ctx, self.augment, None, 0), "ctx_set_augment")
        # LeCam regulariser (lecam_lambda > 0): anchors, per-update sums, the three published values and the update count in ONE persistent
        # device tensor the context reads and writes stream-ordered (include/aclgan_hip.h: aclgan_ctx_set_lecam) -- a replayed graph too
        self.lecam_lambda, self.lecam_decay, self.lecam_start = lecam_from_config(hp)
        self._lecam = None
        if self.lecam_lambda > 0:
            self._lecam = torch.zeros(L.lib.aclgan_lecam_state_floats(self._ctx), dtype=torch.float32, device=self.device)
            L.check(L.lib.aclgan_ctx_set_lecam(self._ctx, self.lecam_lambda, self.lecam_decay, self.lecam_start, L.ptr(self._lecam)), "ctx_set_lecam")
        # adaptive augmentation probability (dis_augment_p): p, the overfitting signal and the controller's counters in ONE persistent device
        # tensor (include/aclgan_hip.h: aclgan_ctx_set_ada) that the gate reads before an update and dis_update folds -- no host synchronisation,
        # a replayed graph included.  The gate's uniforms come from a third CPU generator of the trainer's own (seed: initial_seed() + rank +
        # ADA_SEED_OFFSET), so the augmentation rows and the z of a run are the same with and without the key; its state is not part of a
        # checkpoint.  The context is given the controller's parameters before every update (_bind_ada: the step depends on the batch size)
        self.ada = ada_from_config(hp)
        self._ada = self._adagen = None
        self._ada_dev = {}
        self._ada_bound = None
        if self.ada is not None:
            self._ada = torch.zeros(L.lib.aclgan_ada_state_floats(), dtype=torch.float32, device=self.device)
            self._ada[0] = self.ada[0]
        # mode-seeking regulariser (ms_lambda > 0): z_4, z_5 of an update come from a CPU generator of the trainer's own (seed: initial_seed() +
        # rank + MS_SEED_OFFSET), so the z and the augmentation rows of a run are the same with and without the key; its state is not part of a
        # checkpoint.  They are copied into a persistent device tensor per batch size (a replayed graph reads the address it captured) and bound
        # just before the update (_bind_modeseek); the eight values of an update land in _ms_out.  Off: no tensor, no call
        self.ms_lambda = modeseek_from_config(hp)
        self._msgen = None
        self._ms_dev = {}
        self._ms_out = torch.zeros(8, dtype=torch.float32, device=self.device) if self.ms_lambda > 0 else None
        if self.ms_lambda > 0:
            # on the context before the first workspace query, like the augmentation policy (the two extra passes live in the arena).  rows = 0:
            # no update accepts this binding, so the placeholder address is never read
            L.check(L.lib.aclgan_ctx_set_modeseek(self._ctx, self.ms_lambda, L.ptr(self._ms_out), 0, L.ptr(self._ms_out)), "ctx_set_modeseek")
        # the lane scheduler's streams first, before anything else of this process creates one (the rank-0 broadcast below initialises the process
        # group's communicator and its stream): HIP binds streams to hardware queues in creation order (include/aclgan_hip.h, aclgan_warm_streams)
        if os.environ.get("ACLGAN_WARM_STREAMS", "1") not in ("", "0"):
            with torch.cuda.device(self.device):
                L.check(L.lib.aclgan_warm_streams(0), "warm_streams")
        if self.hip_graph:      # (a captured update runs on one lane with a parameter-gradient stream of its own: created here, outside any capture)
            with torch.cuda.device(self.device):
                L.check(L.lib.aclgan_ctx_enable_capture(self._ctx), "ctx_enable_capture")
        self.style_dim = hp["gen"]["style_dim"]
        self.alpha = hp["alpha"]
        self.focus_lam = hp["focus_loss"]
        self._hp = hp
        # ---- flat buffers (one contiguous param / grad / exp_avg / exp_avg_sq per optimizer) ----
        self._tensors, self._param, self._grad, self._m, self._v = {}, {}, {}, {}, {}
        self._w16, self._w16t = {}, {}
        for grp in (L.GROUP_GEN, L.GROUP_DIS):
            n = L.lib.aclgan_group_numel(self._ctx, grp)
            ents = []
            name = C.create_string_buffer(256)
            off = C.c_int64(); shp = (C.c_int * 4)(); nd = C.c_int()
            for i in range(L.lib.aclgan_tensor_count(self._ctx, grp)):
                L.check(L.lib.aclgan_tensor_info(self._ctx, grp, i, name, 256, C.byref(off), shp, C.byref(nd)))
                full = name.value.decode()
                net, key = full.split("/", 1)
                shape = tuple(shp[j] for j in range(nd.value))
                ents.append(dict(net=net, key=key, offset=off.value, shape=shape, numel=int(math.prod(shape))))
            self._tensors[grp] = ents
            self._param[grp] = torch.zeros(n, device=self.device)
            self._grad[grp] = torch.zeros(n, device=self.device)
            self._m[grp] = torch.zeros(n, device=self.device)
            self._v[grp] = torch.zeros(n, device=self.device)
            L.check(L.lib.aclgan_bind_params(self._ctx, grp, L.ptr(self._param[grp]), L.ptr(self._grad[grp]),
                                             L.ptr(self._m[grp]), L.ptr(self._v[grp])), "bind_params")
            if self.compute_dtype != "fp32":   # 16-bit weight packs, refreshed by the library from the fp32 master copy
                self._w16[grp] = torch.zeros(n, dtype=torch.int16, device=self.device)
                self._w16t[grp] = torch.zeros(n, dtype=torch.int16, device=self.device)
                L.check(L.lib.aclgan_bind_params16(self._ctx, grp, L.ptr(self._w16[grp]), L.ptr(self._w16t[grp])), "bind_params16")
        # spectral norm (dis.norm: sn): u / v of every normalised layer, one flat buffer outside Adam, the gradients and the buckets
        ents = []
        for i in range(L.lib.aclgan_tensor_count(self._ctx, L.GROUP_SN_STATE)):
            L.check(L.lib.aclgan_tensor_info(self._ctx, L.GROUP_SN_STATE, i, name, 256, C.byref(off), shp, C.byref(nd)))
            net, key = name.value.decode().split("/", 1)
            ents.append(dict(net=net, key=key, offset=off.value, shape=(shp[0],), numel=shp[0]))
        for e in ents:     # weight_v: the (ci, kh, kw) of the weight_bar it belongs to
            if e["key"].endswith("weight_v"):
                bar = next(t for t in self._tensors[L.GROUP_DIS] if t["net"] == e["net"] and t["key"] == e["key"][:-len("weight_v")] + "weight_bar")
                e["vshape"] = bar["shape"][1:]
        self._tensors[L.GROUP_SN_STATE] = ents
        self._sn_state = torch.zeros(max(1, L.lib.aclgan_group_numel(self._ctx, L.GROUP_SN_STATE)), device=self.device)
        L.check(L.lib.aclgan_bind_sn_state(self._ctx, L.ptr(self._sn_state)), "bind_sn_state")
        d = self.arch.gen_dim << self.arch.gen_n_downsample
        self._dummy_buffers = {}
        for net in ("gen_AB", "gen_BA"):   # AdaIN running_mean/var: never used, but in the state_dict (networks.py:488-489)
            b = OrderedDict()
            for r in range(self.arch.gen_n_res):
                for j in range(2):
                    b["dec.model.0.model.%d.model.%d.norm.running_mean" % (r, j)] = torch.zeros(d)
                    b["dec.model.0.model.%d.model.%d.norm.running_var" % (r, j)] = torch.ones(d)
            self._dummy_buffers[net] = b
        self.gen_AB, self.gen_BA = AdaINGen(self, "gen_AB"), AdaINGen(self, "gen_BA")
        self.dis_A, self.dis_B, self.dis_2 = MsImageDis(self, "dis_A"), MsImageDis(self, "dis_B"), MsImageDis(self, "dis_2")
        # fixed display noise (trainer.py:30-32)
        ds = int(hp["display_size"])
        self.z_1 = torch.randn(ds, self.style_dim, 1, 1).to(self.device)
        self.z_2 = torch.randn(ds, self.style_dim, 1, 1).to(self.device)
        self.z_3 = torch.randn(ds, self.style_dim, 1, 1).to(self.device)
        # optimizers (trainer.py:34-44): Adam + StepLR, one per group
        self._opt = {grp: dict(lr=float(hp["lr"]), beta1=float(hp["beta1"]), beta2=float(hp["beta2"]), eps=1e-8,
                               weight_decay=float(hp["weight_decay"]), steps=0) for grp in (L.GROUP_GEN, L.GROUP_DIS)}
        self._sched_calls = 0
        # weight init (trainer.py:48-52, utils.py:274-294)
        self._init_weights(hp.get("init", "kaiming"))
        self._ws = None
        self._ws_shape = None
        self._losses = torch.zeros(len(L.LOSS_NAMES), device=self.device)
        for n in L.LOSS_NAMES:
            setattr(self, n, torch.zeros((), device=self.device))
        # the penalties of the last R1 pass: 0 before the first (the zero a loss starts as: no tensor of their own while the key is off)
        self.loss_dis_r1_A = self.loss_dis_r1_B = self.loss_dis_total
        # ... and the LeCam values of the last dis_update, w * mean((D - anchor of the other side)^2) summed per discriminator, without lambda
        self.loss_dis_lecam_A = self.loss_dis_lecam_B = self.loss_dis_lecam_2 = self.loss_dis_total
        # ... and the mode-seeking values of the last gen_update (without lambda) with the collapse readout mean(dI / dz): it tends to 0 when z is ignored
        self.loss_gen_ms_A = self.loss_gen_ms_B = self.gen_diversity_A = self.gen_diversity_B = self.loss_dis_total
        self._zgen = None
        # fp16: dynamic loss scaling, state resident on the device (include/aclgan_hip.h: aclgan_bind_loss_scale)
        self._lscale = None
        if self.compute_dtype == "fp16":
            s0 = float(hp.get("loss_scale_init", 65536.0))
            self._lscale = torch.tensor([s0, 1.0 / s0, 0, 0, 0, 0, float(hp.get("loss_scale_growth_interval", 2000)), 0],
                                        dtype=torch.float32, device=self.device)
            L.check(L.lib.aclgan_bind_loss_scale(self._ctx, L.ptr(self._lscale)), "bind_loss_scale")
        # the scale each group's gradient buffers carry: a device-side copy of the live scale taken when that group's update starts
        # (grad_scale(grp)); the two groups are updated at different live scales whenever one of them overflowed in between
        self._gscale = None if self._lscale is None else torch.zeros(2, dtype=torch.float32, device=self.device)
        self._last_grp = None
        # gradient norm / clip / guard (grad_clip*): per group one persistent device tensor the optimizer step reads and writes stream-ordered
        # (include/aclgan_hip.h: aclgan_bind_grad_clip).  Off: no tensor, no call; the two readouts stay the zero a loss starts as
        self.grad_clip = grad_clip_from_config(hp)
        self._clip = [None, None]
        self.grad_norm_gen = self.grad_norm_dis = self.loss_dis_total
        for grp in (L.GROUP_GEN, L.GROUP_DIS):
            if self.grad_clip[grp] > 0:
                self._clip[grp] = torch.zeros(L.lib.aclgan_grad_clip_state_floats(), dtype=torch.float32, device=self.device)
                L.check(L.lib.aclgan_bind_grad_clip(self._ctx, grp, self.grad_clip[grp], L.ptr(self._clip[grp])), "bind_grad_clip")
        self._ema = None
        self._fwd_ema = False
        # content encodings of x_a carried from a dis_update into the gen_update that follows it (_carry_state): the x_a tensor of the last
        # eager dis_update (held, so that its storage cannot be handed to another tensor) and what must not change before gen_update adopts
        self._carry = None
        self._carry_epoch = 0
        self.enc_reuse = bool(hp.get("enc_reuse", True))
        self._setup_data_parallel()
        # averaged generator (ema_decay > 0): one more flat buffer beside the generator group's, starting from this replica's weights
        # (initialised and, data-parallel, already rank 0's); the generator's Adam launch keeps it up to date (aclgan_adam_step_ema)
        if self._ema_decay > 0:
            self._ema = self._param[L.GROUP_GEN].clone()
            L.check(L.lib.aclgan_bind_ema(self._ctx, L.GROUP_GEN, L.ptr(self._ema)), "bind_ema")

    def __del__(self):
        try:
            if getattr(self, "_ctx", None):
                L.lib.aclgan_ctx_destroy(self._ctx)
                self._ctx = None
        except Exception:
            pass

    # ---- plumbing: the nn.Module surface of the reference class (trainer.py:14) that callers can reach ----
    NETS = ("gen_AB", "gen_BA", "dis_A", "dis_B", "dis_2")

    def state_dict(self):
        """the reference trainer's own state_dict(): '<net>.<key>' for the five networks, in registration order
        (254 entries: tests/golden/state_dict_keys.txt)"""
        sd = OrderedDict()
        for n in self.NETS:
            for k, v in getattr(self, n).state_dict().items():
                sd[n + "." + k] = v
        return sd

    def load_state_dict(self, sd, strict=True):
        self._carry_epoch += 1
        known = set()
        for n in self.NETS:
            sub = OrderedDict((k[len(n) + 1:], v) for k, v in sd.items() if k.startswith(n + "."))
            known.update(n + "." + k for k in sub)
            getattr(self, n).load_state_dict(sub, strict=strict)
        extra = [k for k in sd if k not in known]
        if strict and extra:
            raise L.AclganError("load_state_dict: unexpected keys %s" % extra[:5])

    def named_parameters(self):
        for n in self.NETS:
            for k, v in getattr(self, n).named_parameters():
                yield n + "." + k, v

    def parameters(self):
        return [p for _, p in self.named_parameters()]

    def zero_grad(self):
        for grp in (L.GROUP_GEN, L.GROUP_DIS):
            self._grad[grp].zero_()

    def to(self, *a, **k):
        return self

    def cuda(self, *a, **k):
        return self

    def eval(self):
        return self

    def train(self, mode=True):
        return self

    def _ref_key_order(self, net, pkeys, bkeys):
        # AdaIN blocks: norm buffers precede the conv parameters of the same Conv2dBlock
        out = []
        for k in pkeys:
            if k.endswith("conv.weight") and k.startswith("dec.model.0."):
                pre = k[: -len("conv.weight")]
                out += [pre + "norm.running_mean", pre + "norm.running_var"]
            if k.endswith(".module.weight_bar"):     # SpectralNorm registers u, v, then bar after the conv's bias (networks.py:577-579)
                pre = k[: -len("weight_bar")]
                out += [pre + "weight_u", pre + "weight_v"]
            out.append(k)
        assert set(out) == set(pkeys) | set(bkeys), (set(out) ^ (set(pkeys) | set(bkeys)))
        return out

    def _init_weights(self, kind):
        for grp, nets in ((L.GROUP_GEN, (self.gen_AB, self.gen_BA)), (L.GROUP_DIS, (self.dis_A, self.dis_B, self.dis_2))):
            for net in nets:
                for key, v in net.named_parameters():
                    if ".module." in key:
                        # spectrally normalised conv: weights_init skips it (no `weight` attribute after the wrap, utils.py:277), so
                        # nn.Conv2d's own initialisation stays: kaiming-uniform(a=sqrt 5) weight, bias ~ U(+-1/sqrt(fan_in))
                        if key.endswith("weight_bar"):
                            v.copy_(torch.nn.init.kaiming_uniform_(torch.empty(tuple(v.shape)), a=math.sqrt(5.0)).to(self.device))
                        else:
                            bar = next(e for e in net._entries if e["key"] == key[: -len("bias")] + "weight_bar")
                            fan_in = int(math.prod(bar["shape"][1:]))
                            b = 1.0 / math.sqrt(fan_in)
                            v.copy_(torch.empty(tuple(v.shape)).uniform_(-b, b).to(self.device))
                    elif key.endswith(".weight"):
                        fan_in = int(math.prod(v.shape[1:]))
                        if grp == L.GROUP_DIS or kind == "gaussian":
                            w = torch.randn(tuple(v.shape)) * 0.02
                        elif kind == "kaiming":
                            w = torch.randn(tuple(v.shape)) * math.sqrt(2.0 / fan_in)
                        elif kind == "xavier":
                            fan_out = v.shape[0] * int(math.prod(v.shape[2:]))
                            w = torch.randn(tuple(v.shape)) * math.sqrt(2.0) * math.sqrt(2.0 / (fan_in + fan_out))
                        elif kind == "orthogonal":     # utils.py:285-286
                            w = torch.nn.init.orthogonal_(torch.empty(tuple(v.shape)), gain=math.sqrt(2.0))
                        elif kind == "default":        # utils.py:287-288: nn.Conv2d / nn.Linear's own reset_parameters() stays
                            w = torch.nn.init.kaiming_uniform_(torch.empty(tuple(v.shape)), a=math.sqrt(5.0))
                        else:
                            raise L.AclganError("Unsupported initialization: %s" % kind)
                        v.copy_(w.to(self.device))
                    elif key.endswith(".gamma"):
                        v.copy_(torch.rand(tuple(v.shape)).to(self.device))   # networks.py:517
                    else:
                        v.zero_()
        # u, v ~ N(0, 1), l2-normalised (networks.py:571-574)
        for e in self._tensors[L.GROUP_SN_STATE]:
            x = torch.randn(e["numel"], dtype=torch.float64)
            self._sn_state[e["offset"]: e["offset"] + e["numel"]].copy_((x / (x.norm() + 1e-12)).float().to(self.device))

    def _st(self):
        """the current stream of THIS trainer's device (not of torch's current device)"""
        return L.stream_ptr(self.device)

    def _ensure_workspace(self, B, H, W, forward_only=False):
        """Bind an arena large enough for one update (or, forward_only, for one encode / decode / discriminator
        forward: inference must not inherit the training step's shape constraints or its arena size)."""
        key = (B, H, W)
        have = self._ws_shape
        # (an update's need depends on the library's tuning switches -- lanes, batched transforms, kernel choices -- and so does a
        #  forward's: the 4x4 stride-2 Winograd scratch follows wino_fused / wino_s2k4.  The cached size is valid for one tuning epoch;
        #  after aclgan_tuning the next call sizes and binds again instead of failing with ACLGAN_ENOMEM)
        ep = C.c_longlong()
        L.check(L.lib.aclgan_tuning_get(b"epoch", C.byref(ep)), "tuning_get")
        if have is not None and have[0] >= B and have[1:3] == (H, W) and have[4] == ep.value and (forward_only or have[3]):
            return
        need = C.c_size_t()
        if forward_only:
            L.check(L.lib.aclgan_forward_workspace_bytes(self._ctx, B, H, W, C.byref(need)), "forward_workspace_bytes")
        else:
            L.check(L.lib.aclgan_workspace_bytes(self._ctx, B, H, W, C.byref(need)), "workspace_bytes")
        if self._ws is None or self._ws.numel() < need.value:
            self._ws = None
            try:
                self._ws = torch.empty(need.value, dtype=torch.uint8, device=self.device)
            except torch.OutOfMemoryError:
                # arenas of trainers that are garbage but not yet collected (reference cycles through the bucket callbacks), and blocks
                # the caching allocator keeps reserved: release both and try once more before giving up
                import gc
                gc.collect(); torch.cuda.empty_cache()
                self._ws = torch.empty(need.value, dtype=torch.uint8, device=self.device)
        L.check(L.lib.aclgan_bind_workspace(self._ctx, L.ptr(self._ws), self._ws.numel()), "bind_workspace")
        self._ws_shape = key + (not forward_only, ep.value)

    def loss_scale_state(self):
        """fp16 only: {'scale', 'clean_updates', 'skipped_gen', 'skipped_dis'} (one device->host copy)."""
        if self._lscale is None:
            return None
        v = self._lscale.cpu().tolist()
        return {"scale": v[0], "clean_updates": int(v[2]), "skipped_gen": int(v[4]), "skipped_dis": int(v[5])}

    def grad_clip_state(self):
        """{'gen': {...}, 'dis': {...}} with 'norm' and 'coef' of the group's last update (true-gradient units; coef 0: it was skipped) and the
        counts 'clipped' / 'skipped' (skipped: for a non-finite norm; fp16 overflows are counted by loss_scale_state()).  None for a group
        whose key is off.  One device->host copy, only when asked."""
        on = [t[:4] for t in self._clip if t is not None]
        vals = torch.stack(on).cpu().tolist() if on else []
        out = {}
        for name, t in zip(("gen", "dis"), self._clip):
            v = vals.pop(0) if t is not None else None
            out[name] = None if v is None else {"norm": v[0], "coef": v[1], "clipped": int(v[2]), "skipped": int(v[3])}
        return out

    def grad_clip_log_text(self):
        """train.py's log-line suffix: both groups' last norms and the updates skipped so far (a group whose key is off shows nan / 0)"""
        s = self.grad_clip_state()
        norm = lambda k: s[k]["norm"] if s[k] else float("nan")      # noqa: E731
        return " gnorm_G=%.4g gnorm_D=%.4g skipped=%d" % (norm("gen"), norm("dis"), sum(v["skipped"] for v in s.values() if v))

    def grad_scale(self, grp=None):
        """the factor a group's gradient buffers carry.  fp32 / bf16: 1.  fp16: the loss scale that group's last update ran with --
        the generator's and the discriminators' buffers differ whenever an overflow halved (or a clean run doubled) the live scale
        between the two updates.  grp: "gen" / "dis" (or GROUP_GEN / GROUP_DIS); None -> the group updated last.  A group that has not
        been updated yet reports the live scale (its buffers are zero).  One device->host copy, only when asked."""
        if self._lscale is None:
            return 1.0
        if grp is None:
            grp = self._last_grp
        elif isinstance(grp, str):
            grp = {"gen": L.GROUP_GEN, "dis": L.GROUP_DIS}[grp]
        live = float(self._lscale[0].item())
        if grp is None:
            return live
        own = float(self._gscale[grp].item())
        return own if own > 0 else live

    def _carry_state(self, x_a):
        """What a gen_update may adopt the preceding dis_update's content encodings of x_a under (include/aclgan_hip.h:
        aclgan_ctx_carry_encodings): the same x_a storage that no torch operation has written since, generator parameters and 16-bit packs
        that no torch operation has written since (load_state_dict, a broadcast), and no weight swap or resume in between.  The library
        checks its own side (Adam on the generators, binds, shape, dtype, workspace).  torch cannot see a loader that refills the buffer
        behind x_a without going through a tensor operation: such a caller turns the reuse off (config key enc_reuse: false, or the library's tuning key enc_reuse 0)."""
        g = L.GROUP_GEN
        packs = tuple((t.data_ptr(), t._version) for t in (self._w16.get(g), self._w16t.get(g)) if t is not None)
        return (x_a.data_ptr(), tuple(x_a.shape), x_a._version, self._param[g].data_ptr(), self._param[g]._version, packs, self._carry_epoch)

    def _draw_z(self, B):
        # three draws from the CPU generator, in the reference's order (trainer.py:99-101); data-parallel ranks use
        # their own generator (seed + rank) so that shards do not share noise
        return [torch.randn(B, self.style_dim, 1, 1, generator=self._zgen) for _ in range(3)]

    def _current_lr(self, hp):
        if hp.get("lr_policy", "constant") == "step":   # StepLR (utils.py:263-271)
            return float(hp["lr"]) * float(hp["gamma"]) ** (self._sched_calls // int(hp["step_size"]))
        return float(hp["lr"])

    def _publish_losses(self, lo, hi):
        # fresh 0-d tensors per update, like the reference (trainer.py:136-165): a caller may keep them across steps
        vals = self._losses[lo:hi].clone()
        for i in range(lo, hi):
            setattr(self, L.LOSS_NAMES[i], vals[i - lo])

    def _draw_augment(self, which, B, H, W):
        """a fresh draw of this update's augmentation rows from the trainer's own CPU generator"""
        if self._auggen is None:
            import torch.distributed as dist
            rank = dist.get_rank() if self._dist_world() else 0
            self._auggen = torch.Generator().manual_seed((torch.initial_seed() + rank + AUG_SEED_OFFSET) % (1 << 63))
        return draw_augment_params(self.augment, (5 if which == "gen" else 7) * B, H, W, self._auggen)

    def _bind_augment(self, which, aug):
        """This update's augmentation rows into the persistent device tensor of (update, row count) the context reads them from
        (persistent: a replayed graph reads the address it was captured with).  Returns that tensor."""
        if not (isinstance(aug, torch.Tensor) and aug.dim() == 2 and aug.shape[1] == 8):
            raise L.AclganError("aug: expected a (rows, 8) tensor of augmentation parameters (draw_augment_params)")
        key = (which, aug.shape[0])
        dev = self._aug_dev.get(key)
        if dev is None:
            dev = self._aug_dev[key] = torch.zeros(aug.shape[0], 8, dtype=torch.float32, device=self.device)
        dev.copy_(aug.to(torch.float32))
        L.check(L.lib.aclgan_ctx_set_augment(self._ctx, self.augment, L.ptr(dev), dev.shape[0]), "ctx_set_augment")
        return dev

    def _draw_aug_u(self, rows):
        """a fresh draw of this update's gate uniforms, (rows, 4) in [0, 1) (column 3 unused), from the trainer's third CPU generator"""
        if self._adagen is None:
            import torch.distributed as dist
            rank = dist.get_rank() if self._dist_world() else 0
            self._adagen = torch.Generator().manual_seed((torch.initial_seed() + rank + ADA_SEED_OFFSET) % (1 << 63))
        return torch.rand(rows, 4, generator=self._adagen)

    def _bind_ada(self, B):
        """The controller's parameters onto the context: step = ada_interval * B / (ada_kimg * 1000) with B this update's (per-rank) batch,
        0 for a fixed p.  Returns what a captured graph holds as kernel arguments."""
        _, adaptive, target, interval, kimg = self.ada
        step = interval * B / (kimg * 1000.0) if adaptive else 0.0
        key = (self._ada.data_ptr(), target, interval, step)
        if key != self._ada_bound:
            L.check(L.lib.aclgan_ctx_set_ada(self._ctx, L.ptr(self._ada), target, interval, step), "ctx_set_ada")
            self._ada_bound = key
        return key

    def _gate_augment(self, which, aug_dev, aug_u, H, W):
        """The gate (aclgan_augment_gate), eagerly on the update's stream: this update's rows and uniforms and the p of the moment, read on the
        device, into the persistent effective rows of (update, row count), which the context then reads instead of the rows.  Returns that tensor."""
        rows = aug_dev.shape[0]
        key = (which, rows)
        ent = self._ada_dev.get(key)
        if ent is None:
            ent = self._ada_dev[key] = (torch.zeros(rows, 4, dtype=torch.float32, device=self.device),
                                        torch.zeros(rows, 8, dtype=torch.float32, device=self.device))
        u_dev, eff = ent
        u_dev.copy_(aug_u.to(torch.float32))
        L.check(L.lib.aclgan_augment_gate(L.ptr(aug_dev), L.ptr(u_dev), L.ptr(self._ada), rows, H, W, self.augment, L.ptr(eff), self._st()), "augment_gate")
        L.check(L.lib.aclgan_ctx_set_augment(self._ctx, self.augment, L.ptr(eff), rows), "ctx_set_augment")
        return eff

    def _draw_z_ms(self, B):
        """a fresh draw of this gen_update's (z_4, z_5) from the trainer's own CPU generator"""
        if self._msgen is None:
            import torch.distributed as dist
            rank = dist.get_rank() if self._dist_world() else 0
            self._msgen = torch.Generator().manual_seed((torch.initial_seed() + rank + MS_SEED_OFFSET) % (1 << 63))
        return [torch.randn(B, self.style_dim, 1, 1, generator=self._msgen) for _ in range(2)]

    def _bind_modeseek(self, z_ms, B):
        """This update's (z_4, z_5) into the persistent device tensor of its batch size, which the context reads them from.  Returns that tensor."""
        if len(z_ms) != 2 or any((not isinstance(t, torch.Tensor)) or t.numel() != B * self.style_dim for t in z_ms):
            raise L.AclganError("z_ms: expected two (B, gen.style_dim %d, 1, 1) tensors (z_4, z_5) for B = %d" % (self.style_dim, B))
        dev = self._ms_dev.get(B)
        if dev is None:
            dev = self._ms_dev[B] = torch.zeros(2, B, self.style_dim, dtype=torch.float32, device=self.device)
        dev.copy_(torch.stack([t.reshape(B, self.style_dim).to(torch.float32) for t in z_ms]))
        L.check(L.lib.aclgan_ctx_set_modeseek(self._ctx, self.ms_lambda, L.ptr(dev), 2 * B, L.ptr(self._ms_out)), "ctx_set_modeseek")
        return dev

    def _update(self, which, x_a, x_b, hp, z, aug=None, z_ms=None, aug_u=None):
        grp = L.GROUP_GEN if which == "gen" else L.GROUP_DIS
        x_a = x_a.to(self.device, torch.float32).contiguous()
        x_b = x_b.to(self.device, torch.float32).contiguous()
        B, Cc, H, W = x_a.shape
        if x_b.shape != x_a.shape or Cc != 3:
            raise L.AclganError("x_a / x_b must both be (B,3,H,W); got %s and %s" % (tuple(x_a.shape), tuple(x_b.shape)))
        if aug is not None and not self.augment:
            raise L.AclganError("aug given, but this trainer was built without dis_augment")
        if aug_u is not None:      # (refused here, before a generator moves or anything is copied)
            if self._ada is None:
                raise L.AclganError("aug_u given, but this trainer was built without dis_augment_p")
            rows = aug.shape[0] if isinstance(aug, torch.Tensor) and aug.dim() == 2 else (5 if which == "gen" else 7) * B
            if not (isinstance(aug_u, torch.Tensor) and tuple(aug_u.shape) == (rows, 4)):
                raise L.AclganError("aug_u: expected a (%d, 4) tensor of uniforms in [0, 1), one row per augmentation row" % rows)
        if self.augment and aug is None:      # (host work: before the copies below, which wait for the device)
            aug = self._draw_augment(which, B, H, W)
        if self._ada is not None and aug_u is None:
            aug_u = self._draw_aug_u((5 if which == "gen" else 7) * B)
        ms = which == "gen" and self.ms_lambda > 0
        if z_ms is not None and not ms:
            raise L.AclganError("z_ms given, but this is no gen_update of a trainer built with ms_lambda > 0")
        if ms and z_ms is None:
            z_ms = self._draw_z_ms(B)
        if z is None:
            z = self._draw_z(B)
        if any(t.numel() != B * self.style_dim for t in z):      # (refused here, by name, before anything is copied or enqueued)
            raise L.AclganError("z: expected (B, gen.style_dim %d, 1, 1) tensors for B = %d; got %s"
                                % (self.style_dim, B, [tuple(t.shape) for t in z]))
        zz = torch.stack([t.reshape(B, self.style_dim).to(torch.float32) for t in z]).to(self.device).contiguous()
        hpc = hparams_from_config(hp)
        with torch.cuda.device(self.device):
            aug_dev = self._bind_augment(which, aug) if self.augment else None
            ada_key = None
            if self._ada is not None:      # p of the moment onto this update's rows, before the update (under hip_graph: before the replay)
                ada_key = self._bind_ada(B)
                aug_dev = self._gate_augment(which, aug_dev, aug_u, H, W)
            ms_dev = self._bind_modeseek(z_ms, B) if ms else None
            det_now = bool(L.lib.aclgan_get_deterministic())
            if det_now != self.deterministic:      # the process-wide mode changed under us: scratch sizes depend on it
                self.deterministic = det_now
                self._ws_shape = None
                self._graphs = {}
            self._ensure_workspace(B, H, W)
            st = self._st()
            if self._gscale is not None:      # fp16: this update's gradients carry the scale that is live NOW (stream-ordered copy, no sync)
                self._gscale[grp:grp + 1].copy_(self._lscale[0:1])
                self._last_grp = grp
            fn = L.lib.aclgan_gen_update if which == "gen" else L.lib.aclgan_dis_update
            # lazy R1: on the discriminator updates whose count BEFORE the update is a multiple of r1_every (the count is saved and resumed)
            r1 = which == "dis" and self.r1_gamma > 0 and self._opt[grp]["steps"] % self.r1_every == 0
            if self.hip_graph and self._reducer is None and self._run_graph(which, grp, fn, x_a, x_b, zz, B, H, W, hpc, aug_dev, ms_dev, ada_key):
                # zero_grad + update replayed from the captured graph; the pass is not captured: eagerly after it, before Adam
                if r1:
                    self._r1_pass(x_a, x_b, B, H, W, st)
            else:
                L.check(L.lib.aclgan_zero_grad(self._ctx, grp, st), "zero_grad")   # opt.zero_grad() (trainer.py:91,248)
                if self._reducer is not None:
                    self._reducer.begin(grp)
                # before the update: its bucket callbacks then fire after the last writer of every bucket.  (_r1_after, single process only: after
                # it, the order a replayed update has -- tests measure what the order of the two accumulations is worth)
                after = self._r1_after and self._reducer is None
                if r1 and not after:
                    self._r1_pass(x_a, x_b, B, H, W, st)
                # an eager dis_update keeps its content encodings of x_a; the gen_update after it adopts them if nothing changed (_carry_state)
                kept, self._carry, carry = self._carry, None, L.CARRY_OFF
                if self.enc_reuse and not self.hip_graph:
                    if which == "dis":
                        self._carry, carry = (x_a, self._carry_state(x_a)), L.CARRY_KEEP
                    elif kept is not None and kept[0] is x_a and kept[1] == self._carry_state(x_a):
                        carry = L.CARRY_ADOPT
                L.check(L.lib.aclgan_ctx_carry_encodings(self._ctx, carry), "ctx_carry_encodings")
                L.check(fn(self._ctx, L.ptr(x_a), L.ptr(x_b), L.ptr(zz), B, H, W, C.byref(hpc), L.ptr(self._losses), st), which + "_update")
                if r1 and after:
                    self._r1_pass(x_a, x_b, B, H, W, st)
            if getattr(self, "_sync_error", None) is not None:
                raise self._sync_error
            self._allreduce_grads(grp)
            o = self._opt[grp]
            o["steps"] += 1
            adam = L.Adam(self._current_lr(self._hp), o["beta1"], o["beta2"], o["eps"], o["weight_decay"])
            if grp == L.GROUP_GEN and self._ema is not None:      # opt.step() with the average as one more stream of the same launch
                mode = L.EMA_COPY if o["steps"] <= self._ema_start else L.EMA_BLEND
                L.check(L.lib.aclgan_adam_step_ema(self._ctx, grp, C.byref(adam), o["steps"], self._ema_decay, mode, st), "adam_step_ema")
            else:
                L.check(L.lib.aclgan_adam_step(self._ctx, grp, C.byref(adam), o["steps"], st), "adam_step")   # opt.step()
        if self._clip[grp] is not None:      # a fresh 0-d tensor per update, like the losses
            setattr(self, "grad_norm_gen" if which == "gen" else "grad_norm_dis", self._clip[grp][0].clone())
        if which == "gen":
            self._publish_losses(0, 12)
            if ms:      # fresh 0-d tensors per update, like the losses
                vals = self._ms_out.clone()
                self.loss_gen_ms_B, self.gen_diversity_B, self.loss_gen_ms_A, self.gen_diversity_A = vals[0], vals[1], vals[4], vals[5]
        else:
            self._publish_losses(12, 16)
            if self._lecam is not None:
                s = 18 * self.arch.dis_num_scales
                vals = self._lecam[s:s + 3].clone()
                self.loss_dis_lecam_A, self.loss_dis_lecam_B, self.loss_dis_lecam_2 = vals[0], vals[1], vals[2]

    def _r1_pass(self, x_a, x_b, B, H, W, st):
        """aclgan_dis_r1 on (dis_A, x_a) and (dis_B, x_b) with gamma * r1_every, into the zeroed (or just written) DIS gradient buffer, on the
        update's stream.  Under fp16 the library multiplies by the live loss scale, the one this update's gradients carry (grad_scale)."""
        if self._r1_pen is None:
            self._r1_pen = torch.zeros(2, device=self.device)
        need = 0
        for net in (self.dis_A, self.dis_B):
            nb = L.lib.aclgan_dis_r1_scratch_bytes(self._ctx, net.net_id, B, H, W)
            if not nb:
                raise L.AclganError("dis_r1_scratch_bytes(%s, %d, %d, %d): %s" % (net.name, B, H, W, L.last_error()))
            need = max(need, nb)
        if self._r1_scratch is None or self._r1_scratch.numel() < need:
            self._r1_scratch = None
            self._r1_scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
        gamma = self.r1_gamma * self.r1_every
        for i, (net, x) in enumerate(((self.dis_A, x_a), (self.dis_B, x_b))):
            L.check(L.lib.aclgan_dis_r1(self._ctx, net.net_id, L.ptr(x), B, H, W, gamma, C.c_void_p(self._r1_pen.data_ptr() + 4 * i), None,
                                        L.ptr(self._r1_scratch), st), "dis_r1(%s)" % net.name)
        self.r1_passes += 1
        vals = self._r1_pen.clone()      # fresh 0-d tensors per pass, like the losses of an update
        self.loss_dis_r1_A, self.loss_dis_r1_B = vals[0], vals[1]

    # ---- HIP-graph replay of an update (opt-in, see __init__) ----
    def _run_graph(self, which, grp, fn, x_a, x_b, zz, B, H, W, hpc, aug_dev=None, ms_dev=None, ada_key=None):
        """True: the update ran as a graph replay.  False: run it eagerly (first call of a new key -- it also performs the
        library's one-time initialisation outside any capture -- or capture is unavailable)."""
        key = (B, H, W, bytes(hpc), self._ws.data_ptr(), self._ws.numel(), self.compute_dtype, self.deterministic)
        if self.augment:      # (the captured kernels read the policy and the address of the rows; the rows themselves are refilled before every replay)
            key += (self.augment, aug_dev.data_ptr(), aug_dev.shape[0])
        if self._lecam is not None:      # (lambda, decay and start are kernel arguments of the captured launches, the state's address too)
            key += (self.lecam_lambda, self.lecam_decay, self.lecam_start, self._lecam.data_ptr())
        if ms_dev is not None:      # (lambda is a kernel argument of the captured launches; the noise rows are refilled before every replay)
            key += (self.ms_lambda, ms_dev.data_ptr(), self._ms_out.data_ptr())
        if ada_key is not None:     # (the state's address, target, interval and step are kernel arguments of the captured sign and fold launches)
            key += ada_key
        ent = self._graphs.get(which)
        if ent is None or ent["key"] != key:
            self._graphs[which] = {"key": key, "graph": None}
            return False
        if ent["graph"] is None:
            try:
                sx_a, sx_b, szz = torch.empty_like(x_a), torch.empty_like(x_b), torch.empty_like(zz)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    st = self._st()      # the capture stream
                    L.check(L.lib.aclgan_zero_grad(self._ctx, grp, st), "zero_grad (capture)")
                    L.check(fn(self._ctx, L.ptr(sx_a), L.ptr(sx_b), L.ptr(szz), B, H, W, C.byref(hpc), L.ptr(self._losses), st), which + "_update (capture)")
                ent.update(graph=g, x_a=sx_a, x_b=sx_b, zz=szz)
            except Exception as e:      # capture unsupported here: say so once and stay eager
                import warnings
                warnings.warn("aclgan_Trainer: HIP-graph capture failed (%r); running eagerly" % (e,))
                self.hip_graph = False
                self._graphs = {}
                return False
        ent["x_a"].copy_(x_a); ent["x_b"].copy_(x_b); ent["zz"].copy_(zz)
        ent["graph"].replay()
        return True

    # ---- data parallelism (not in the reference): one process per GPU, full replicas ----
    def _dist_world(self):
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return 0
        if dist.get_world_size() == 1 and os.environ.get("ACLGAN_BENCH_FORCE_DIST") != "1":
            return 0
        return dist.get_world_size()

    def _setup_data_parallel(self):
        """Called at the end of __init__ and resume(): replicas must START identical, whatever each rank's RNG did --
        broadcast rank 0's parameters and Adam state; then hook the engine's bucket callback so that each gradient
        bucket's all-reduce starts while the rest of the backward is still running (ddp.BucketReducer).
        z noise: every rank draws its own shard's z from a generator seeded with initial_seed() + rank."""
        self._reducer = None
        self._exposed_events, self._exposed_ms = [], 0.0
        world = self._dist_world()
        if not world:
            return
        import torch.distributed as dist
        from .ddp import BucketReducer, broadcast_flat
        for grp in (L.GROUP_GEN, L.GROUP_DIS):
            for buf in (self._param[grp], self._m[grp], self._v[grp]):
                broadcast_flat(buf)
        if self._ema is not None:
            broadcast_flat(self._ema)
        if self._tensors[L.GROUP_SN_STATE]:
            broadcast_flat(self._sn_state)   # spectral norm's u / v (not parameters, but every replica must start from the same)
        if self._lecam is not None:
            # LeCam anchors: every rank starts from rank 0's (here and after resume()), then keeps its own -- each rank sees its own shard,
            # the anchors are not all-reduced; the parameter gradients are, as before
            broadcast_flat(self._lecam)
        if self._ada is not None:
            # p and the controller's counters: every rank starts from rank 0's (here and after resume()), then keeps its own -- each rank
            # steers by the signal of its own shard, which is not all-reduced: the ranks may drift apart in p
            broadcast_flat(self._ada)
        steps = torch.tensor([self._opt[0]["steps"], self._opt[1]["steps"], self._sched_calls], dtype=torch.int64, device=self.device)
        dist.broadcast(steps, 0)
        self._opt[0]["steps"], self._opt[1]["steps"], self._sched_calls = (int(v) for v in steps.tolist())
        self._zgen = torch.Generator().manual_seed(torch.initial_seed() + dist.get_rank())
        if os.environ.get("ACLGAN_DDP_OVERLAP", "1") != "0":
            self._reducer = BucketReducer(self._ctx, lambda g: self._grad[g], world)
        if self.hip_graph:
            # HIP-graph replay is single-GPU only: the bucket callbacks and the forward sync point are host code that starts
            # collectives from inside the update, which a captured graph cannot replay -- say so instead of silently ignoring the option
            import warnings
            warnings.warn("aclgan_Trainer: hip_graph=True is ignored in data-parallel runs (world size %d): updates run eagerly" % world)
            self.hip_graph = False
        # optional: the reference's global-batch semantics of the focus losses (config key ddp_global_focus / env
        # ACLGAN_DDP_GLOBAL_FOCUS=1): the 6 mask sums are all-reduced at a forward sync point of gen_update
        if self._hp.get("ddp_global_focus", False) or os.environ.get("ACLGAN_DDP_GLOBAL_FOCUS") == "1":
            def on_sync(user, ptr, n):
                try:
                    off = int(ptr) - self._ws.data_ptr()
                    t = self._ws[off: off + 4 * n].view(torch.float32)
                    dist.all_reduce(t, op=dist.ReduceOp.SUM)      # stream-ordered: the compute stream waits for it, the host does not
                except BaseException as e:   # noqa: BLE001  (must not unwind through the C frames)
                    self._sync_error = e
            self._sync_error = None
            self._sync_cb = L.SYNC_FN(on_sync)
            L.check(L.lib.aclgan_set_forward_sync(self._ctx, self._sync_cb, None, world), "set_forward_sync")

    def _allreduce_grads(self, grp):
        """Average the flat gradient buffer over ranks with RCCL before Adam.  With the bucket reducer the collectives
        were started from inside the backward (overlap) and are only waited for here; ACLGAN_DDP_OVERLAP=0 selects the
        plain post-backward bucketed all-reduce.  No-op when torch.distributed is not initialised."""
        world = self._dist_world()
        if not world:
            return
        # GPU-side exposure of the exchange: the compute stream does nothing between these two events except wait for the
        # collectives, so their distance is the part of the all-reduce that was NOT hidden behind the backward
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
        if self._reducer is not None:
            self._reducer.finish(grp)
        else:
            from .ddp import allreduce_flat
            allreduce_flat(self._grad[grp], world)
        ev[1].record()
        self._exposed_events.append(ev)
        if len(self._exposed_events) > 4096:
            self.allreduce_exposed_ms()

    def allreduce_exposed_ms(self, reset=True):
        """total milliseconds the compute stream spent waiting for gradient collectives since the last call (synchronises)"""
        torch.cuda.synchronize(self.device)
        self._exposed_ms += sum(a.elapsed_time(b) for a, b in self._exposed_events)
        self._exposed_events = []
        v = self._exposed_ms
        if reset:
            self._exposed_ms = 0.0
        return v

    # ---- the hot path (trainer.py:90-170, 247-293) ----
    def gen_update(self, x_a, x_b, hyperparameters, z=None, aug=None, z_ms=None, aug_u=None):
        """aug (tests): this update's (5 B, 8) augmentation rows instead of a draw (dis_augment; include/aclgan_hip.h: aclgan_ctx_set_augment);
        z_ms (tests): this update's (z_4, z_5) instead of a draw (ms_lambda; include/aclgan_hip.h: aclgan_ctx_set_modeseek);
        aug_u (tests): this update's (5 B, 4) gate uniforms instead of a draw (dis_augment_p; include/aclgan_hip.h: aclgan_augment_gate)"""
        self._update("gen", x_a, x_b, hyperparameters, z, aug, z_ms, aug_u)

    def modeseek_log_text(self):
        """train.py's log-line suffix: the two mode-seeking values of the last gen_update and the two collapse readouts"""
        return " ms_A=%.4g ms_B=%.4g div_A=%.4g div_B=%.4g" % (float(self.loss_gen_ms_A), float(self.loss_gen_ms_B), float(self.gen_diversity_A),
                                                               float(self.gen_diversity_B))

    def dis_update(self, x_a, x_b, hyperparameters, z=None, aug=None, aug_u=None):
        """aug (tests): this update's (7 B, 8) augmentation rows instead of a draw; aug_u (tests): its (7 B, 4) gate uniforms instead of a draw"""
        self._update("dis", x_a, x_b, hyperparameters, z, aug, aug_u=aug_u)

    # ---- adaptive augmentation probability (dis_augment_p; not in the reference) ----
    def ada_state(self):
        """{'p', 'r_t', 'r', 'updates', 'adjustments'} of the device state in one device-to-host copy: the probability the next gate reads, the
        mean overfitting signal of the last closed interval, the signal of the last dis_update, the dis_updates folded and the intervals closed
        with a finite r_t (include/aclgan_hip.h: aclgan_ctx_set_ada)"""
        if self._ada is None:
            raise L.AclganError("ada_state(): the adaptive augmentation probability is off (set dis_augment_p)")
        t = self._ada.cpu()
        n = t.view(torch.int32)
        return {"p": float(t[0]), "r_t": float(t[1]), "r": float(t[6]), "updates": int(n[4]), "adjustments": int(n[5])}

    def ada_log_text(self):
        """train.py's log-line suffix: p and the last closed interval's r_t"""
        s = self.ada_state()
        return " ada_p=%.4g ada_rt=%.4g" % (s["p"], s["r_t"])

    def update_learning_rate(self):   # trainer.py:295-299, called every iteration (train.py:101)
        self._sched_calls += 1

    def focus_translation(self, x_fg, x_bg, x_focus):
        """trainer.py:85-88 for sample() / test.py, on NCHW tensors, through the library's blend kernel.  x_fg / x_focus may
        be channel slices of one decoder output (only the batch stride has to be regular)."""
        B, Cc, H, W = x_fg.shape
        if Cc != 3 or x_focus.shape[1] != 1 or tuple(x_bg.shape) != (B, 3, H, W):
            raise L.AclganError("focus_translation: expected (B,3,H,W), (B,3,H,W), (B,1,H,W)")

        def dense(t):   # each sample's C*H*W block contiguous; any batch stride
            t = t.to(self.device, torch.float32)
            ok = t.stride(3) == 1 and t.stride(2) == W and t.stride(1) == H * W
            return t if ok else t.contiguous()
        fg, bg, fo = dense(x_fg), dense(x_bg), dense(x_focus)
        out = torch.empty(B, 3, H, W, device=self.device)
        with torch.cuda.device(self.device):
            L.check(L.lib.aclgan_focus_translation_nchw(L.ptr(fg), fg.stride(0), L.ptr(bg), bg.stride(0), L.ptr(fo), fo.stride(0),
                                                        L.ptr(out), B, H * W, self._st()), "focus_translation")
        return out

    # ---- averaged generator (ema_decay > 0; not in the reference) ----
    @property
    def ema_updates(self):
        """generator updates so far (Adam's step count; skipped fp16 updates included): the first ema_start of them copy, the rest blend"""
        return self._opt[L.GROUP_GEN]["steps"]

    def _require_ema(self, what):
        if self._ema is None:
            raise L.AclganError("%s: the averaged generator is off (set ema_decay in (0, 1))" % what)

    @contextmanager
    def ema_weights(self):
        """Inside the block gen_AB / gen_BA .encode / .decode -- and so sample() and test.py's translate() -- read the averaged weights;
        the updates keep reading (and writing) the live ones.  The previous selection comes back on exit, also on an exception."""
        self._require_ema("ema_weights()")
        prev = self._fwd_ema
        self._select_forward_weights(True)
        try:
            yield self
        finally:
            self._select_forward_weights(prev)

    def _select_forward_weights(self, ema):
        self._carry_epoch += 1
        L.check(L.lib.aclgan_set_forward_weights(self._ctx, L.WEIGHTS_EMA if ema else L.WEIGHTS_LIVE), "set_forward_weights")
        self._fwd_ema = ema

    def ema_state_dict(self):
        """{'AB', 'BA'}: the averaged generators in the layout of gen_AB.state_dict() / gen_BA.state_dict() (what a gen_*.pt holds)"""
        self._require_ema("ema_state_dict()")
        return {"AB": self.gen_AB._state_dict_of(self._ema), "BA": self.gen_BA._state_dict_of(self._ema)}

    def ema_reset(self):
        """start the average again from the live weights"""
        self._require_ema("ema_reset()")
        self._ema.copy_(self._param[L.GROUP_GEN])

    # ---- LeCam regulariser (lecam_lambda > 0; not in the reference) ----
    @property
    def lecam_updates(self):
        """discriminator updates folded into the anchors so far (the device's count; one device->host copy); 0 while the key is off"""
        if self._lecam is None:
            return 0
        return int(self._lecam[-1:].view(torch.int32).item())

    def lecam_anchors(self):
        """{'A', 'B', '2'}: per discriminator a (num_scales, 2) tensor (copies), [s][0] the moving average of its mean output on the fake side,
        [s][1] on the real side (dis_2: pair_A1 / pair_A2).  The two drift apart when a discriminator memorises its real images."""
        if self._lecam is None:
            raise L.AclganError("lecam_anchors(): the LeCam regulariser is off (set lecam_lambda > 0)")
        S = self.arch.dis_num_scales
        a = self._lecam[:6 * S].clone().view(3, S, 2)
        return {"A": a[0], "B": a[1], "2": a[2]}

    def lecam_log_text(self):
        """train.py's log-line suffix: the three values of the last dis_update and the first scale's anchors"""
        a = self.lecam_anchors()
        return (" lecam_A=%.4g lecam_B=%.4g lecam_2=%.4g" % (float(self.loss_dis_lecam_A), float(self.loss_dis_lecam_B), float(self.loss_dis_lecam_2)) +
                "".join(" D_real_%s=%.4g D_fake_%s=%.4g" % (k, float(a[k][0, 1]), k, float(a[k][0, 0])) for k in ("A", "B", "2")))

    def sample(self, x_a, x_b, ema=False):
        """trainer.py:179-245: per-image eval forward; returns the reference's 9-tuple (focus branch) or 7-tuple (focus_loss == 0).
        ema=True: from the averaged generators (ema_weights())."""
        if ema:
            with self.ema_weights():
                return self.sample(x_a, x_b)
        x_a = x_a.to(self.device, torch.float32)
        x_b = x_b.to(self.device, torch.float32)
        if not (self.focus_lam > 0):
            return self._sample_plain(x_a, x_b)
        X_A, X_B, A_fake, B_fake, A2_fake, m_A, m_B, m_A2, m_rec, A_rec = [], [], [], [], [], [], [], [], [], []
        for i in range(x_a.size(0)):
            xa = x_a[i].unsqueeze(0)
            X_A.append(xa); X_B.append(x_b[i].unsqueeze(0))
            c_1, s_1 = self.gen_BA.encode(xa)
            img, mask = self.gen_BA.decode(c_1, self.z_1[i].unsqueeze(0)).split(3, 1)
            A_fake.append(self.focus_translation(img, xa, mask)); m_A.append(mask)
            img, mask = self.gen_BA.decode(c_1, s_1).split(3, 1)
            A_rec.append(img); m_rec.append(mask)
            c_2, _ = self.gen_AB.encode(xa)
            xb_img, mask = self.gen_AB.decode(c_2, self.z_2[i].unsqueeze(0)).split(3, 1)
            xb_img = self.focus_translation(xb_img, xa, mask)
            B_fake.append(xb_img); m_B.append(mask)
            c_3, _ = self.gen_BA.encode(xb_img)
            img, mask = self.gen_BA.decode(c_3, self.z_3[i].unsqueeze(0)).split(3, 1)
            A2_fake.append(self.focus_translation(img, xb_img, mask)); m_A2.append(mask)
        cat = torch.cat
        return (cat(X_A), cat(A_fake), cat(m_A), cat(B_fake), cat(m_B), cat(A2_fake), cat(m_A2), cat(A_rec), cat(m_rec))

    def _sample_plain(self, x_a, x_b):
        """trainer.py:216-230,238-245 (non-focus configuration).  Faithful to the reference including its quirk at :228-229: the B
        reconstruction encodes the WHOLE batch x_b inside the per-image loop, so x_B_recon comes back as B copies of the batch."""
        X_A, X_B, A_fake, B_fake, A2_fake, A_rec, B_rec = [], [], [], [], [], [], []
        for i in range(x_a.size(0)):
            xa = x_a[i].unsqueeze(0)
            X_A.append(xa); X_B.append(x_b[i].unsqueeze(0))
            c_1, s_1 = self.gen_BA.encode(xa)
            A_fake.append(self.gen_BA.decode(c_1, self.z_1[i].unsqueeze(0)))
            A_rec.append(self.gen_BA.decode(c_1, s_1))
            c_2, _ = self.gen_AB.encode(xa)
            x_B1 = self.gen_AB.decode(c_2, self.z_2[i].unsqueeze(0))
            B_fake.append(x_B1)
            c_3, _ = self.gen_BA.encode(x_B1)
            A2_fake.append(self.gen_BA.decode(c_3, self.z_3[i].unsqueeze(0)))
            c_4, s_4 = self.gen_AB.encode(x_b)
            B_rec.append(self.gen_AB.decode(c_4, s_4))
        cat = torch.cat
        return (cat(X_A), cat(A_fake), cat(B_fake), cat(A2_fake), cat(A_rec), cat(X_B), cat(B_rec))

    # ---- checkpoints (trainer.py:301-331, utils.py:211-220) ----
    def _opt_state_dict(self, grp):
        """torch.optim.Adam.state_dict() layout so that the reference can load optimizer.pt."""
        o = self._opt[grp]
        state = {}
        nets = (self.gen_AB, self.gen_BA) if grp == L.GROUP_GEN else (self.dis_A, self.dis_B, self.dis_2)
        idx = 0
        for net in nets:
            for e in net._entries:
                if o["steps"] > 0:
                    state[idx] = {"step": torch.tensor(float(o["steps"])),
                                  "exp_avg": net._view(e, self._m[grp]).contiguous().clone(),
                                  "exp_avg_sq": net._view(e, self._v[grp]).contiguous().clone()}
                idx += 1
        pg = {"lr": self._current_lr(self._hp), "betas": (o["beta1"], o["beta2"]), "eps": o["eps"], "weight_decay": o["weight_decay"],
              "amsgrad": False, "initial_lr": float(self._hp["lr"]), "params": list(range(idx))}
        return {"state": state, "param_groups": [pg]}

    def _load_opt_state_dict(self, grp, sd):
        o = self._opt[grp]
        nets = (self.gen_AB, self.gen_BA) if grp == L.GROUP_GEN else (self.dis_A, self.dis_B, self.dis_2)
        idx = 0
        steps = 0
        with torch.no_grad():
            for net in nets:
                for e in net._entries:
                    st = sd["state"].get(idx)
                    if st is not None:
                        net._view(e, self._m[grp]).copy_(st["exp_avg"].to(self.device))
                        net._view(e, self._v[grp]).copy_(st["exp_avg_sq"].to(self.device))
                        steps = int(float(st["step"]))
                    idx += 1
        o["steps"] = steps
        pg = sd["param_groups"][0]
        o.update(beta1=float(pg["betas"][0]), beta2=float(pg["betas"][1]), eps=float(pg["eps"]), weight_decay=float(pg["weight_decay"]))

    def save(self, snapshot_dir, iterations):
        gen_name = os.path.join(snapshot_dir, "gen_%08d.pt" % (iterations + 1))
        dis_name = os.path.join(snapshot_dir, "dis_%08d.pt" % (iterations + 1))
        opt_name = os.path.join(snapshot_dir, "optimizer.pt")
        cpu = lambda sd: OrderedDict((k, v.cpu()) for k, v in sd.items())  # noqa: E731
        torch.save({"AB": cpu(self.gen_AB.state_dict()), "BA": cpu(self.gen_BA.state_dict())}, gen_name)
        torch.save({"A": cpu(self.dis_A.state_dict()), "B": cpu(self.dis_B.state_dict()), "2": cpu(self.dis_2.state_dict())}, dis_name)
        opt = {"gen": self._opt_state_dict(L.GROUP_GEN), "dis": self._opt_state_dict(L.GROUP_DIS)}
        if self._lscale is not None:
            # fp16 only (an extra key the reference's loader ignores: trainer.py:313-316 reads 'gen' / 'dis'): the dynamic loss-scale state --
            # live scale, clean-update counter and the SKIPPED-update counts Adam's bias-correction step excludes.  Adam's per-tensor
            # 'step' above counts applied + skipped updates (the reference's own counter semantics: one per optimizer.step() call).
            opt["aclgan_loss_scale_state"] = self._lscale.cpu().clone()
        if any(t is not None for t in self._clip):
            # another extra key: the eight leading floats of both groups' clip states (row 0 gen, row 1 dis; zeros for a group that is off).
            # [3], the updates skipped for a non-finite norm, is part of Adam's bias-correction step like the loss scale's skip counts
            opt["aclgan_grad_clip_state"] = torch.stack([torch.zeros(8) if t is None else t[:8].cpu() for t in self._clip])
        torch.save(opt, opt_name)
        if self._ema is not None:
            # the averaged generators, loadable wherever a gen_*.pt is (test.py --checkpoint).  The name holds neither "gen" nor "dis":
            # _get_model_list (and the reference's, utils.py:211-220) matches by substring and takes the last name in sorted order
            sd = self.ema_state_dict()
            torch.save({"AB": cpu(sd["AB"]), "BA": cpu(sd["BA"]), "updates": self.ema_updates, "decay": self._ema_decay},
                       os.path.join(snapshot_dir, "ema_%08d.pt" % (iterations + 1)))
        if self._lecam is not None:
            # the LeCam state as the device holds it (anchors, the count's four bytes).  The name holds neither "gen" nor "dis" either
            # (decay: resume() warns when the resuming run's differs)
            torch.save({"state": self._lecam.cpu().clone(), "decay": self.lecam_decay}, os.path.join(snapshot_dir, "lecam_%08d.pt" % (iterations + 1)))
        if self._ada is not None:
            # the state as the device holds it (p, the open interval, the counters' four bytes) and the controller's three parameters.  The
            # name holds neither "gen" nor "dis" either
            torch.save({"state": self._ada.cpu().clone(), "target": self.ada[2], "interval": self.ada[3], "kimg": self.ada[4]},
                       os.path.join(snapshot_dir, "ada_%08d.pt" % (iterations + 1)))

    @staticmethod
    def _get_model_list(dirname, key):   # utils.py:211-220
        if not os.path.exists(dirname):
            return None
        models = sorted(os.path.join(dirname, f) for f in os.listdir(dirname)
                        if os.path.isfile(os.path.join(dirname, f)) and key in f and ".pt" in f)
        return models[-1] if models else None

    def resume(self, checkpoint_dir, hyperparameters):
        last = self._get_model_list(checkpoint_dir, "gen")
        sd = torch.load(last, map_location="cpu")
        self.gen_AB.load_state_dict(sd["AB"]); self.gen_BA.load_state_dict(sd["BA"])
        iterations = int(last[-11:-3])
        last = self._get_model_list(checkpoint_dir, "dis")
        sd = torch.load(last, map_location="cpu")
        self.dis_A.load_state_dict(sd["A"]); self.dis_B.load_state_dict(sd["B"]); self.dis_2.load_state_dict(sd["2"])
        sd = torch.load(os.path.join(checkpoint_dir, "optimizer.pt"), map_location="cpu")
        self._load_opt_state_dict(L.GROUP_DIS, sd["dis"]); self._load_opt_state_dict(L.GROUP_GEN, sd["gen"])
        if self._lscale is not None and "aclgan_loss_scale_state" in sd:      # fp16: resume the loss scale and the skipped-update counts
            self._lscale.copy_(sd["aclgan_loss_scale_state"].to(self.device, torch.float32))
        if any(t is not None for t in self._clip):
            if "aclgan_grad_clip_state" in sd:
                for t, row in zip(self._clip, sd["aclgan_grad_clip_state"]):
                    if t is not None:
                        t[:8].copy_(row.to(self.device, torch.float32))
            else:
                import warnings
                warnings.warn("aclgan_Trainer.resume: optimizer.pt holds no aclgan_grad_clip_state (written with grad_clip off); the clipped and "
                              "skipped counts start at 0")
                for t in self._clip:
                    if t is not None:
                        t.zero_()
        # get_scheduler(..., iterations) (trainer.py:318-320, utils.py:263-271) builds StepLR(last_epoch=iterations).  The reference
        # pins torch 1.2.0 (acl-gan.yaml), whose _LRScheduler.__init__ ends with self.step(last_epoch): the scheduler resumes AT
        # last_epoch = iterations and (closed-form get_lr of that version) lr = lr0 * gamma ** (iterations // step_size).  torch >= 1.4
        # calls self.step() instead and would resume one epoch later (iterations + 1) -- the pinned version is the one mirrored here
        # (ACLGAN_RESUME_SCHED_PLUS1=1 selects the torch >= 1.4 behaviour).
        self._sched_calls = iterations + (1 if os.environ.get("ACLGAN_RESUME_SCHED_PLUS1") == "1" else 0)
        if self._ema is not None:
            ema_name = os.path.join(checkpoint_dir, "ema_%08d.pt" % iterations)
            if os.path.isfile(ema_name):
                sd = torch.load(ema_name, map_location="cpu")
                with torch.no_grad():
                    for net, key in ((self.gen_AB, "AB"), (self.gen_BA, "BA")):
                        for k, v in net._named_views(self._ema):
                            v.copy_(sd[key][k].to(device=self.device, dtype=torch.float32))
            else:
                import warnings
                warnings.warn("aclgan_Trainer.resume: %s not found; the averaged generator starts from the resumed weights" % ema_name)
                self.ema_reset()
        if self._lecam is not None:
            lecam_name = os.path.join(checkpoint_dir, "lecam_%08d.pt" % iterations)
            if os.path.isfile(lecam_name):
                sd = torch.load(lecam_name, map_location="cpu")
                if tuple(sd["state"].shape) != tuple(self._lecam.shape):
                    raise L.AclganError("resume: %s holds %d floats, dis.num_scales %d needs %d" % (lecam_name, sd["state"].numel(),
                                                                                                   self.arch.dis_num_scales, self._lecam.numel()))
                self._lecam.copy_(sd["state"].to(self.device, torch.float32))
                if float(sd.get("decay", self.lecam_decay)) != self.lecam_decay:
                    import warnings
                    warnings.warn("aclgan_Trainer.resume: %s was written with lecam_decay %r, this run uses %r; the saved anchors continue under "
                                  "the new decay" % (lecam_name, sd["decay"], self.lecam_decay))
            else:
                import warnings
                warnings.warn("aclgan_Trainer.resume: %s not found; the LeCam anchors start again (the term acts after lecam_start more updates)" % lecam_name)
                self._lecam.zero_()
        if self._ada is not None:
            import warnings
            ada_name = os.path.join(checkpoint_dir, "ada_%08d.pt" % iterations)
            if os.path.isfile(ada_name):
                sd = torch.load(ada_name, map_location="cpu")
                if tuple(sd["state"].shape) != tuple(self._ada.shape):
                    raise L.AclganError("resume: %s holds %d floats, the state has %d" % (ada_name, sd["state"].numel(), self._ada.numel()))
                self._ada.copy_(sd["state"].to(self.device, torch.float32))
                if not self.ada[1]:      # a fixed probability is the configured one, whatever the file says; the monitor's counters continue
                    self._ada[0] = self.ada[0]
                saved = (sd.get("target"), sd.get("interval"), sd.get("kimg"))
                if saved != tuple(self.ada[2:]):
                    warnings.warn("aclgan_Trainer.resume: %s was written with (ada_target, ada_interval, ada_kimg) = %r, this run uses %r; the saved "
                                  "p and interval continue under the new parameters" % (ada_name, saved, tuple(self.ada[2:])))
            else:
                warnings.warn("aclgan_Trainer.resume: %s not found; the augmentation probability starts again at %g" % (ada_name, self.ada[0]))
                self._ada.zero_()
                self._ada[0] = self.ada[0]
        self._hp = hyperparameters
        self._setup_data_parallel()
        print("Resume from iteration %d" % iterations)
        return iterations
