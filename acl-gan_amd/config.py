"""The YAML dict of a run as validated values: one *_from_config per group of keys (aclgan_amd.trainer exports them).  Nothing touches the device."""
import ctypes as C
import math

from . import _lib as L

__all__ = ["DIS_NORMS", "ada_from_config", "arch_from_config", "augment_from_config", "dis_norm_from_config", "ema_from_config",
           "grad_clip_from_config", "hparams_from_config", "lecam_from_config", "modeseek_from_config", "r1_from_config"]

DIS_NORMS = ("none", "sn")    # dis.norm values the library implements (sn: SpectralNorm, networks.py:360-361,538-600)
_f32 = lambda v: C.c_float(v).value                              # noqa: E731  (the fp32 the library will see)
_finite_from_0 = lambda v: 0 <= v and math.isfinite(_f32(v))     # noqa: E731  ([0, inf) as fp32)
_decay = lambda v: 0 <= v and _f32(v) < 1                        # noqa: E731  ([0, 1) as fp32)


def _is_number(v, in_range):      # (the tests every key repeats: a number, no bool, in its range ...)
    return not isinstance(v, bool) and isinstance(v, (int, float)) and bool(in_range(v))


def _is_integer(v, lo, below=None):      # (... or an integer, no bool, in its range)
    return not isinstance(v, bool) and isinstance(v, int) and lo <= v and (below is None or v < below)


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
    return L.Arch(int(hp["input_dim_a"]), int(hp["input_dim_b"]), int(g["dim"]), int(g["mlp_dim"]), int(g["style_dim"]), int(g["output_dim"]),
                  int(g["n_downsample"]), int(g["n_res"]), int(d["dim"]), int(d["n_layer"]), int(d["num_scales"]))


def ema_from_config(hp):
    """The averaged generator's keys (not in the reference) as (decay, start, display):
    ema_decay   float in [0, 1), default 0 = off: no buffer, no extra call, the launches of a run without the keys;
    ema_start   int >= 0, default 0: the generator updates 1 .. ema_start copy the weights into the average, later ones blend;
    ema_display bool, default false: train.py's pictures are sampled from the average (needs ema_decay > 0)."""
    decay, start, display = hp.get("ema_decay", 0), hp.get("ema_start", 0), hp.get("ema_display", False)
    if not _is_number(decay, _decay):
        raise L.AclganError("ema_decay=%r: expected a number in [0, 1) (0 switches the averaged generator off)" % (decay,))
    if not _is_integer(start, 0):
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
    if not _is_number(gamma, _finite_from_0):
        raise L.AclganError("r1_gamma=%r: expected a finite number >= 0 (0 switches the R1 penalty off)" % (gamma,))
    if not _is_integer(every, 1):
        raise L.AclganError("r1_every=%r: expected an integer >= 1" % (every,))
    if gamma > 0 and not math.isfinite(_f32(gamma * every)):
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
    if not _is_number(lam, _finite_from_0):
        raise L.AclganError("lecam_lambda=%r: expected a finite number >= 0 (0 switches the LeCam regulariser off)" % (lam,))
    if not _is_number(decay, _decay):
        raise L.AclganError("lecam_decay=%r: expected a number in [0, 1)" % (decay,))
    if not _is_integer(start, 0, 2 ** 31):
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
    if not adaptive and not _is_number(v, lambda v: 0 <= v <= 1):
        raise L.AclganError("dis_augment_p=%r: expected a number in [0, 1] or the string adaptive" % (v,))
    if not augment_from_config(hp):
        raise L.AclganError("dis_augment_p=%r needs a non-empty dis_augment (a comma-separated subset of %s): there is nothing to apply with "
                            "that probability" % (v, ",".join(L.AUG)))
    target, interval, kimg = 0.6, 4, 500.0
    if adaptive:
        target, interval, kimg = hp.get("ada_target", target), hp.get("ada_interval", interval), hp.get("ada_kimg", kimg)
        if not _is_number(target, lambda v: -1 <= v <= 1):
            raise L.AclganError("ada_target=%r: expected a number in [-1, 1]" % (target,))
        if not _is_integer(interval, 1, 2 ** 31):
            raise L.AclganError("ada_interval=%r: expected an integer >= 1 (below 2**31)" % (interval,))
        if not _is_number(kimg, lambda v: v > 0 and math.isfinite(_f32(v))):
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
    if not _is_number(lam, _finite_from_0):
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
        if not _is_number(v, lambda v: v >= 0 and (v == 0 or _f32(v) > 0)):      # (a positive number must stay positive as fp32)
            raise L.AclganError("%s=%r: expected a number > 0 or .inf (0 switches the gradient norm, the clip and the guard off)" % (key, v))
        out.append(float(v))
    both, gen, dis = out
    return (both if gen is None else gen, both if dis is None else dis)


def hparams_from_config(hp):
    """The per-call hyper-parameters gen_update / dis_update read (trainer.py:93-97,142-144,164,288-290)."""
    return L.HParams(float(hp["gan_w"]), float(hp["gan_cw"]), float(hp["recon_x_w"]), float(hp["focus_loss"]), float(hp["focus_delta"]),
                     float(hp["focus_upper"]), float(hp["focus_lower"]), float(hp["focus_epsilon"]), float(hp.get("alpha", 1)))
