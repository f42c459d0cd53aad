"""aclgan_Trainer -- drop-in counterpart of the reference's trainer.aclgan_Trainer (reference trainer.py:14-331) running on libaclgan_hip.so.

Same constructor argument (the YAML dict), same methods (gen_update / dis_update / sample / update_learning_rate / save / resume), same
``loss_*`` attributes (0-d tensors), same attribute names for the five networks, same checkpoint file names / dict keys / state_dict key
names (OIHW fp32 weights on disk; the OHWI <-> OIHW repack happens in nets.py, at the boundary).

PyTorch's role: device memory (flat parameter / gradient / Adam-state buffers, workspace), the current stream, torch.save/torch.load,
torch.distributed.  All arithmetic of the step is in the HIP library; if it is missing the import of this package fails -- there is no fallback.
Here: the constructor, the update path, the readouts, sample().  Beside it: config.py, nets.py, checkpoint.py (save / resume), ddp.py.
"""
import ctypes as C
import gc
import os
import warnings
from collections import OrderedDict
from contextlib import contextmanager

import torch
import torch.distributed as dist

from . import _lib as L, config
from .checkpoint import Checkpoints
from .config import *  # noqa: F401,F403  (its __all__: DIS_NORMS and every *_from_config)
from .ddp import DataParallel
from .nets import AdaINGen, MsImageDis, adain_dummy_buffers, init_weights, tensor_table

__all__ = ["aclgan_Trainer", "AdaINGen", "MsImageDis", "draw_augment_params"] + config.__all__

AUG_SEED_OFFSET = 0x0A06           # the augmentation generator's seed = torch.initial_seed() + rank + this
MS_SEED_OFFSET = 0x0A07            # the mode-seeking noise generator's seed = torch.initial_seed() + rank + this
ADA_SEED_OFFSET = 0x0A08           # the gate's uniforms' generator's seed = torch.initial_seed() + rank + this


def _own_generator(t, attr, offset):
    """The CPU generator trainer t keeps for itself in t.<attr>, made at its first draw and seeded torch.initial_seed() + rank + offset as
    they are THEN: the z stream of a run and the other private streams are the same with and without the key that draws from this one; its
    state is not part of a checkpoint.  (A function on attribute names, no method: tests call the _draw_* methods on a stub without methods.)"""
    g = getattr(t, attr)
    if g is None:
        rank = dist.get_rank() if t._dist_world() else 0
        g = torch.Generator().manual_seed((torch.initial_seed() + rank + offset) % (1 << 63))
        setattr(t, attr, g)
    return g


def update_rows(which, B):
    """the discriminator input images of one update at batch B: one augmentation row (and one row of gate uniforms) each"""
    return (5 if which == "gen" else 7) * B


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
    p[:, 1:3] = 1.0
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


class aclgan_Trainer(Checkpoints, DataParallel):
    """See module docstring.  Extra (optional) arguments over the reference: ``device``; and ``z=(z_1, z_2, z_3)`` on the update calls for
    seed-independent parity tests (by default z is drawn from the CPU generator exactly like trainer.py:99-101)."""

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
        self.r1_passes, self._r1_after = 0, False
        self._r1_pen = self._r1_scratch = None
        # compute dtype of the heavy convolutions (not in the reference, which is fp32 only): "fp32" | "bf16" | "fp16"
        self.compute_dtype = str(compute_dtype or hp.get("compute_dtype", "fp32"))
        if self.compute_dtype not in L.DTYPE:
            raise L.AclganError("compute_dtype=%r: expected one of %s" % (self.compute_dtype, sorted(L.DTYPE)))
        # deterministic=True (or config key "deterministic", or ACLGAN_DETERMINISTIC=1): every reduction takes an ordered path and a step is reproducible
        # bit for bit (include/aclgan_hip.h: aclgan_set_deterministic).  Process-wide; must be chosen before the workspaces are sized, i.e. here.
        det = deterministic if deterministic is not None else hp.get("deterministic", None)
        if det is not None:
            L.check(L.lib.aclgan_set_deterministic(1 if det else 0), "set_deterministic")
        self.deterministic = bool(L.lib.aclgan_get_deterministic())
        # hip_graph=True (or config key "hip_graph", or ACLGAN_GRAPH=1): the launch sequence of an update (zero_grad + forward + losses + backward,
        # ~1 000-2 000 kernels) is captured once per (shape, hyper-parameters, workspace) into a HIP graph and replayed; Adam stays a separate launch
        # (its step count is a kernel argument).  Same kernels, same order, same results.  Pays when the step is launch-bound; off by default.
        hg = hip_graph if hip_graph is not None else hp.get("hip_graph", os.environ.get("ACLGAN_GRAPH", "0") not in ("", "0"))
        self.hip_graph, self._graphs = bool(hg), {}
        self._ctx = C.c_void_p()
        L.check(L.lib.aclgan_ctx_create_dis_norm(C.byref(self.arch), dis_norm_from_config(hp), C.byref(self._ctx)), "ctx_create")
        L.check(L.lib.aclgan_set_compute_dtype(self._ctx, L.DTYPE[self.compute_dtype]), "set_compute_dtype")
        # dis_augment: the policy goes on the context before the first workspace query (the augmented tensors live in the arena); the rows
        # of an update are bound just before it (_bind_augment).  They come from a CPU generator of the trainer's own (_own_generator)
        self._auggen, self._aug_dev = None, {}
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
        # a replayed graph included.  The gate's uniforms come from a third CPU generator of the trainer's own.  The context is given the
        # controller's parameters before every update (_bind_ada: the step depends on the batch size)
        self.ada = ada_from_config(hp)
        self._ada = self._adagen = self._ada_bound = None
        self._ada_dev = {}
        if self.ada is not None:
            self._ada = torch.zeros(L.lib.aclgan_ada_state_floats(), dtype=torch.float32, device=self.device)
            self._ada[0] = self.ada[0]
        # mode-seeking regulariser (ms_lambda > 0): z_4, z_5 of an update come from a CPU generator of the trainer's own, are copied into a
        # persistent device tensor per batch size and bound just before the update (_bind_modeseek); the eight values of an update land in
        # _ms_out.  Off: no tensor, no call
        self.ms_lambda = modeseek_from_config(hp)
        self._msgen, self._ms_dev = None, {}
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
            self._tensors[grp] = tensor_table(self._ctx, grp)
            self._param[grp], self._grad[grp], self._m[grp], self._v[grp] = (torch.zeros(n, device=self.device) for _ in range(4))
            L.check(L.lib.aclgan_bind_params(self._ctx, grp, L.ptr(self._param[grp]), L.ptr(self._grad[grp]),
                                             L.ptr(self._m[grp]), L.ptr(self._v[grp])), "bind_params")
            if self.compute_dtype != "fp32":   # 16-bit weight packs, refreshed by the library from the fp32 master copy
                self._w16[grp], self._w16t[grp] = (torch.zeros(n, dtype=torch.int16, device=self.device) for _ in range(2))
                L.check(L.lib.aclgan_bind_params16(self._ctx, grp, L.ptr(self._w16[grp]), L.ptr(self._w16t[grp])), "bind_params16")
        # spectral norm (dis.norm: sn): u / v of every normalised layer, one flat buffer outside Adam, the gradients and the buckets
        self._tensors[L.GROUP_SN_STATE] = tensor_table(self._ctx, L.GROUP_SN_STATE)
        for e in self._tensors[L.GROUP_SN_STATE]:     # weight_v: the (ci, kh, kw) of the weight_bar it belongs to
            if e["key"].endswith("weight_v"):
                bar = next(t for t in self._tensors[L.GROUP_DIS] if t["net"] == e["net"] and t["key"] == e["key"][:-len("weight_v")] + "weight_bar")
                e["vshape"] = bar["shape"][1:]
        self._sn_state = torch.zeros(max(1, L.lib.aclgan_group_numel(self._ctx, L.GROUP_SN_STATE)), device=self.device)
        L.check(L.lib.aclgan_bind_sn_state(self._ctx, L.ptr(self._sn_state)), "bind_sn_state")
        self._dummy_buffers = adain_dummy_buffers(self.arch)
        self.gen_AB, self.gen_BA = AdaINGen(self, "gen_AB"), AdaINGen(self, "gen_BA")
        self.dis_A, self.dis_B, self.dis_2 = MsImageDis(self, "dis_A"), MsImageDis(self, "dis_B"), MsImageDis(self, "dis_2")
        # fixed display noise (trainer.py:30-32)
        ds = int(hp["display_size"])
        self.z_1, self.z_2, self.z_3 = (torch.randn(ds, self.style_dim, 1, 1).to(self.device) for _ in range(3))
        # optimizers (trainer.py:34-44): Adam + StepLR, one per group
        self._opt = {grp: dict(lr=float(hp["lr"]), beta1=float(hp["beta1"]), beta2=float(hp["beta2"]), eps=1e-8,
                               weight_decay=float(hp["weight_decay"]), steps=0) for grp in (L.GROUP_GEN, L.GROUP_DIS)}
        self._sched_calls = 0
        # weight init (trainer.py:48-52, utils.py:274-294)
        init_weights(self, hp.get("init", "kaiming"))
        self._ws = self._ws_shape = None
        self._losses = torch.zeros(len(L.LOSS_NAMES), device=self.device)
        for n in L.LOSS_NAMES:
            setattr(self, n, torch.zeros((), device=self.device))
        for n in self.KEY_READOUTS:      # (the zero a loss starts as: no tensor of their own while their key is off)
            setattr(self, n, self.loss_dis_total)
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
        for grp in (L.GROUP_GEN, L.GROUP_DIS):
            if self.grad_clip[grp] > 0:
                self._clip[grp] = torch.zeros(L.lib.aclgan_grad_clip_state_floats(), dtype=torch.float32, device=self.device)
                L.check(L.lib.aclgan_bind_grad_clip(self._ctx, grp, self.grad_clip[grp], L.ptr(self._clip[grp])), "bind_grad_clip")
        self._ema, self._fwd_ema = None, False
        # content encodings of x_a carried from a dis_update into the gen_update that follows it (_carry_state): the x_a tensor of the last
        # eager dis_update (held, so that its storage cannot be handed to another tensor) and what must not change before gen_update adopts
        self._carry, self._carry_epoch = None, 0
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
    # the readouts of the training keys, 0-d tensors like the 16 losses (R1, LeCam and mode-seeking values without their factor)
    KEY_READOUTS = ("loss_dis_r1_A", "loss_dis_r1_B", "loss_dis_lecam_A", "loss_dis_lecam_B", "loss_dis_lecam_2",
                    "loss_gen_ms_A", "loss_gen_ms_B", "gen_diversity_A", "gen_diversity_B", "grad_norm_gen", "grad_norm_dis")

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

    def to(self, *a, **k):      # (and cuda / eval / train: there is nothing to move or to switch)
        return self
    cuda = eval = train = to

    def _st(self):
        """the current stream of THIS trainer's device (not of torch's current device)"""
        return L.stream_ptr(self.device)

    def _ensure_workspace(self, B, H, W, forward_only=False):
        """Bind an arena large enough for one update (or, forward_only, for one encode / decode / discriminator
        forward: inference must not inherit the training step's shape constraints or its arena size)."""
        key, have = (B, H, W), self._ws_shape
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

    def log_suffix(self):
        """what train.py's log line adds to the reference's four losses, for the keys that are on, in this order (none: ""); not in losses.csv"""
        return ((" r1_A=%.4g r1_B=%.4g" % (float(self.loss_dis_r1_A), float(self.loss_dis_r1_B)) if self.r1_gamma > 0 else "") +
                (self.lecam_log_text() if self.lecam_lambda > 0 else "") +
                (self.grad_clip_log_text() if max(self.grad_clip) > 0 else "") +
                (self.modeseek_log_text() if self.ms_lambda > 0 else "") +
                (self.ada_log_text() if self.ada is not None else ""))

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
        # the reference's three draws, in its order (trainer.py:99-101); data-parallel ranks use their own generator: shards do not share noise
        return [torch.randn(B, self.style_dim, 1, 1, generator=self._zgen) for _ in range(3)]

    def _current_lr(self, hp):
        if hp.get("lr_policy", "constant") == "step":   # StepLR (utils.py:263-271)
            return float(hp["lr"]) * float(hp["gamma"]) ** (self._sched_calls // int(hp["step_size"]))
        return float(hp["lr"])

    def _draw_augment(self, which, B, H, W):
        """a fresh draw of this update's augmentation rows from the trainer's own CPU generator"""
        return draw_augment_params(self.augment, update_rows(which, B), H, W, _own_generator(self, "_auggen", AUG_SEED_OFFSET))

    def _draw_aug_u(self, rows):
        """a fresh draw of this update's gate uniforms, (rows, 4) in [0, 1) (column 3 unused), from the trainer's third CPU generator"""
        return torch.rand(rows, 4, generator=_own_generator(self, "_adagen", ADA_SEED_OFFSET))

    def _draw_z_ms(self, B):
        """a fresh draw of this gen_update's (z_4, z_5) from the trainer's own CPU generator"""
        g = _own_generator(self, "_msgen", MS_SEED_OFFSET)
        return [torch.randn(B, self.style_dim, 1, 1, generator=g) for _ in range(2)]

    def _staged(self, store, key, *shapes):
        """store[key]: zeroed fp32 device tensors of `shapes` (one shape: the tensor itself, as tests read it), made on first use and kept"""
        if key not in store:
            made = tuple(torch.zeros(*shape, dtype=torch.float32, device=self.device) for shape in shapes)
            store[key] = made[0] if len(made) == 1 else made
        return store[key]

    # ---- a key's inputs of one update (_bind_keys).  _bind_ada / _bind_modeseek return their piece of the graph key; the rows' is the tensor finally read ----
    def _bind_augment(self, which, aug):
        """This update's augmentation rows into the persistent device tensor of (update, row count) the context reads them from.  Returns that tensor."""
        if not (isinstance(aug, torch.Tensor) and aug.dim() == 2 and aug.shape[1] == 8):
            raise L.AclganError("aug: expected a (rows, 8) tensor of augmentation parameters (draw_augment_params)")
        dev = self._staged(self._aug_dev, (which, aug.shape[0]), (aug.shape[0], 8))
        dev.copy_(aug.to(torch.float32))
        L.check(L.lib.aclgan_ctx_set_augment(self._ctx, self.augment, L.ptr(dev), dev.shape[0]), "ctx_set_augment")
        return dev

    def _bind_ada(self, B):
        """The controller's parameters onto the context: step = ada_interval * B / (ada_kimg * 1000) with B this update's (per-rank) batch,
        0 for a fixed p.  (The state's address, target, interval and step are kernel arguments of the captured sign and fold launches.)"""
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
        u_dev, eff = self._staged(self._ada_dev, (which, rows), (rows, 4), (rows, 8))
        u_dev.copy_(aug_u.to(torch.float32))
        L.check(L.lib.aclgan_augment_gate(L.ptr(aug_dev), L.ptr(u_dev), L.ptr(self._ada), rows, H, W, self.augment, L.ptr(eff), self._st()), "augment_gate")
        L.check(L.lib.aclgan_ctx_set_augment(self._ctx, self.augment, L.ptr(eff), rows), "ctx_set_augment")
        return eff

    def _bind_modeseek(self, z_ms, B):
        """This update's (z_4, z_5) into the persistent device tensor of its batch size, which the context reads them from.  (lambda is a kernel
        argument of the captured launches; the noise rows are refilled before every replay.)"""
        if len(z_ms) != 2 or any((not isinstance(t, torch.Tensor)) or t.numel() != B * self.style_dim for t in z_ms):
            raise L.AclganError("z_ms: expected two (B, gen.style_dim %d, 1, 1) tensors (z_4, z_5) for B = %d" % (self.style_dim, B))
        dev = self._staged(self._ms_dev, B, (2, B, self.style_dim))
        dev.copy_(torch.stack([t.reshape(B, self.style_dim).to(torch.float32) for t in z_ms]))
        L.check(L.lib.aclgan_ctx_set_modeseek(self._ctx, self.ms_lambda, L.ptr(dev), 2 * B, L.ptr(self._ms_out)), "ctx_set_modeseek")
        return (self.ms_lambda, dev.data_ptr(), self._ms_out.data_ptr())

    def _bind_keys(self, which, B, H, W, aug, aug_u, z_ms):
        """Stage 2 of an update: every key's inputs onto the device and the context, the gate enqueued.  Returns the keys' part of the graph key"""
        key, ada_key = (), ()
        if self.augment:
            rows = self._bind_augment(which, aug)
            if self._ada is not None:      # p of the moment onto this update's rows, before the update (under hip_graph: before the replay)
                ada_key = self._bind_ada(B)
                rows = self._gate_augment(which, rows, aug_u, H, W)
            # (the captured kernels read the policy and the address of the rows; the rows themselves are refilled before every replay)
            key += (self.augment, rows.data_ptr(), rows.shape[0])
        if self._lecam is not None:      # (lambda, decay and start are kernel arguments of the captured launches, the state's address too)
            key += (self.lecam_lambda, self.lecam_decay, self.lecam_start, self._lecam.data_ptr())
        if z_ms is not None:
            key += self._bind_modeseek(z_ms, B)
        return key + ada_key

    def _host_inputs(self, which, x_a, x_b, z, aug, z_ms, aug_u):
        """Stage 1 of an update: the arguments checked, in this order, then what the caller left out drawn.  aug, aug_u, z_ms: None where a key is off"""
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
            rows = aug.shape[0] if isinstance(aug, torch.Tensor) and aug.dim() == 2 else update_rows(which, B)
            if not (isinstance(aug_u, torch.Tensor) and tuple(aug_u.shape) == (rows, 4)):
                raise L.AclganError("aug_u: expected a (%d, 4) tensor of uniforms in [0, 1), one row per augmentation row" % rows)
        if self.augment and aug is None:      # (host work: before the copies below, which wait for the device)
            aug = self._draw_augment(which, B, H, W)
        if self._ada is not None and aug_u is None:
            aug_u = self._draw_aug_u(update_rows(which, B))
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
        return x_a, x_b, zz, aug, aug_u, z_ms

    def _launch(self, which, grp, x_a, x_b, zz, hpc, keys, st):
        """Stage 3 of an update: zero_grad, the update and, when it is due, the R1 pass -- replayed from the captured graph or eagerly"""
        B, _, H, W = x_a.shape
        fn = L.lib.aclgan_gen_update if which == "gen" else L.lib.aclgan_dis_update
        # lazy R1: on the discriminator updates whose count BEFORE the update is a multiple of r1_every (the count is saved and resumed)
        r1 = which == "dis" and self.r1_gamma > 0 and self._opt[grp]["steps"] % self.r1_every == 0
        if self.hip_graph and self._reducer is None and self._run_graph(which, grp, fn, x_a, x_b, zz, B, H, W, hpc, keys):
            # zero_grad + update replayed from the captured graph; the pass is not captured: eagerly after it, before Adam
            if r1:
                self._r1_pass(x_a, x_b, B, H, W, st)
            return
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

    def _optimizer_step(self, grp, st):
        """Stage 4 of an update: the gradient exchange of a data-parallel run, then Adam (with the average as one more stream of the same launch)"""
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

    def _publish(self, src, names):
        """fresh 0-d tensors per update, like the reference (trainer.py:136-165): one clone of src, attribute names[i] = its element i (None: none)"""
        vals = src.clone()
        for i, n in enumerate(names):
            if n is not None:
                setattr(self, n, vals[i])

    def _publish_update(self, which, grp, ms):
        """Stage 5 of an update: its readouts (the R1 pass publishes its own two: it does not run on every update)"""
        if self._clip[grp] is not None:
            self._publish(self._clip[grp][0:1], ("grad_norm_gen" if which == "gen" else "grad_norm_dis",))
        if which == "gen":
            self._publish(self._losses[0:12], L.LOSS_NAMES[0:12])
            if ms:
                self._publish(self._ms_out, ("loss_gen_ms_B", "gen_diversity_B", None, None, "loss_gen_ms_A", "gen_diversity_A"))
        else:
            self._publish(self._losses[12:16], L.LOSS_NAMES[12:16])
            if self._lecam is not None:
                s = 18 * self.arch.dis_num_scales
                self._publish(self._lecam[s:s + 3], ("loss_dis_lecam_A", "loss_dis_lecam_B", "loss_dis_lecam_2"))

    def _update(self, which, x_a, x_b, hp, z, aug=None, z_ms=None, aug_u=None):
        grp = L.GROUP_GEN if which == "gen" else L.GROUP_DIS
        x_a, x_b, zz, aug, aug_u, z_ms = self._host_inputs(which, x_a, x_b, z, aug, z_ms, aug_u)
        B, _, H, W = x_a.shape
        hpc = hparams_from_config(hp)
        with torch.cuda.device(self.device):
            keys = self._bind_keys(which, B, H, W, aug, aug_u, z_ms)
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
            self._launch(which, grp, x_a, x_b, zz, hpc, keys, st)
            self._optimizer_step(grp, st)
        self._publish_update(which, grp, z_ms is not None)

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
        self._publish(self._r1_pen, ("loss_dis_r1_A", "loss_dis_r1_B"))

    # ---- HIP-graph replay of an update (opt-in, see __init__) ----
    def _run_graph(self, which, grp, fn, x_a, x_b, zz, B, H, W, hpc, keys=()):
        """True: the update ran as a graph replay.  False: run it eagerly (first call of a new key, which also performs the library's one-time
        initialisation outside any capture, or capture is unavailable)"""
        key = (B, H, W, bytes(hpc), self._ws.data_ptr(), self._ws.numel(), self.compute_dtype, self.deterministic) + tuple(keys)
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
                warnings.warn("aclgan_Trainer: HIP-graph capture failed (%r); running eagerly" % (e,))
                self.hip_graph = False
                self._graphs = {}
                return False
        ent["x_a"].copy_(x_a); ent["x_b"].copy_(x_b); ent["zz"].copy_(zz)
        ent["graph"].replay()
        return True

    # ---- the hot path (trainer.py:90-170, 247-293) ----
    def gen_update(self, x_a, x_b, hyperparameters, z=None, aug=None, z_ms=None, aug_u=None):
        """aug (tests): this update's (5 B, 8) augmentation rows instead of a draw (dis_augment; include/aclgan_hip.h: aclgan_ctx_set_augment);
        z_ms (tests): this update's (z_4, z_5) instead of a draw (ms_lambda; include/aclgan_hip.h: aclgan_ctx_set_modeseek);
        aug_u (tests): this update's (5 B, 4) gate uniforms instead of a draw (dis_augment_p; include/aclgan_hip.h: aclgan_augment_gate)"""
        self._update("gen", x_a, x_b, hyperparameters, z, aug, z_ms, aug_u)

    def modeseek_log_text(self):
        """train.py's log-line suffix: the two mode-seeking values of the last gen_update and the two collapse readouts"""
        return " ms_A=%.4g ms_B=%.4g div_A=%.4g div_B=%.4g" % tuple(map(float, (self.loss_gen_ms_A, self.loss_gen_ms_B, self.gen_diversity_A, self.gen_diversity_B)))

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
