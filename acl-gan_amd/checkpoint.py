"""Checkpoints of the trainer (trainer.py:301-331, utils.py:211-220): gen_%08d.pt {AB, BA}, dis_%08d.pt {A, B, 2} and optimizer.pt {gen, dis}
in torch.optim.Adam's layout, all loadable by the reference -- and, beside them, the state of every training key that has some."""
import os
import warnings
from collections import OrderedDict, namedtuple

import torch

from . import _lib as L

# One state beside the networks' and Adam's.  where: its key in optimizer.pt (_opt_extras) or the stem of its own file <stem>_%08d.pt (_file_states: a
# name with neither "gen" nor "dis" in it, _get_model_list matches by substring); payload(): what save() writes; load(saved, name): take it; when the
# checkpoint holds none, resume() warns `absent % name` (None: silent) and calls restart() (None: the state stays as built)
Sidecar = namedtuple("Sidecar", "where payload load restart absent")
_cpu = lambda sd: OrderedDict((k, v.cpu()) for k, v in sd.items())      # noqa: E731


def _copy_state(dst, sd, name, needs):
    if tuple(sd["state"].shape) != tuple(dst.shape):
        raise L.AclganError("resume: %s holds %d floats, %s" % (name, sd["state"].numel(), needs))
    dst.copy_(sd["state"].to(dst.device, torch.float32))


def _opt_extras(t):
    """the extra keys of optimizer.pt (the reference's loader ignores them: trainer.py:313-316 reads 'gen' / 'dis') for what is on in trainer t"""
    out = []
    if t._lscale is not None:      # fp16: live scale, clean-update counter and the SKIPPED-update counts Adam's bias-correction step excludes
        out.append(Sidecar("aclgan_loss_scale_state", lambda: t._lscale.cpu().clone(), lambda v, name: t._lscale.copy_(v.to(t.device, torch.float32)),
                           None, None))
    clips = [c for c in t._clip if c is not None]
    if clips:
        # the eight leading floats of both groups' clip states (row 0 gen, row 1 dis; zeros for a group that is off).  [3], the updates
        # skipped for a non-finite norm, is part of Adam's bias-correction step like the loss scale's skip counts
        out.append(Sidecar("aclgan_grad_clip_state", lambda: torch.stack([torch.zeros(8) if c is None else c[:8].cpu() for c in t._clip]),
                           lambda rows, name: [c[:8].copy_(r.to(t.device, torch.float32)) for c, r in zip(t._clip, rows) if c is not None],
                           lambda: [c.zero_() for c in clips], "aclgan_Trainer.resume: %s holds no aclgan_grad_clip_state (written with grad_clip "
                           "off); the clipped and skipped counts start at 0"))
    return out


def _file_states(t):
    """the states with a file of their own for what is on in trainer t, in the order save() writes and resume() reads them"""
    out = []
    if t._ema is not None:      # the averaged generators, loadable wherever a gen_*.pt is (test.py --checkpoint)
        def load_ema(sd, name):
            with torch.no_grad():
                for net, key in ((t.gen_AB, "AB"), (t.gen_BA, "BA")):
                    for k, v in net._named_views(t._ema):
                        v.copy_(sd[key][k].to(device=t.device, dtype=torch.float32))
        out.append(Sidecar("ema", lambda: dict({k: _cpu(v) for k, v in t.ema_state_dict().items()}, updates=t.ema_updates, decay=t._ema_decay),
                           load_ema, t.ema_reset, "aclgan_Trainer.resume: %s not found; the averaged generator starts from the resumed weights"))
    if t._lecam is not None:      # the state as the device holds it (anchors, the count's four bytes), and the decay it was written under
        def load_lecam(sd, name):
            _copy_state(t._lecam, sd, name, "dis.num_scales %d needs %d" % (t.arch.dis_num_scales, t._lecam.numel()))
            if float(sd.get("decay", t.lecam_decay)) != t.lecam_decay:
                warnings.warn("aclgan_Trainer.resume: %s was written with lecam_decay %r, this run uses %r; the saved anchors continue under "
                              "the new decay" % (name, sd["decay"], t.lecam_decay))
        out.append(Sidecar("lecam", lambda: {"state": t._lecam.cpu().clone(), "decay": t.lecam_decay}, load_lecam, t._lecam.zero_,
                           "aclgan_Trainer.resume: %s not found; the LeCam anchors start again (the term acts after lecam_start more updates)"))
    if t._ada is not None:      # the state as the device holds it (p, the open interval, the counters' four bytes) and the controller's parameters
        def load_ada(sd, name):
            _copy_state(t._ada, sd, name, "the state has %d" % t._ada.numel())
            if not t.ada[1]:      # a fixed probability is the configured one, whatever the file says; the monitor's counters continue
                t._ada[0] = t.ada[0]
            saved = (sd.get("target"), sd.get("interval"), sd.get("kimg"))
            if saved != tuple(t.ada[2:]):
                warnings.warn("aclgan_Trainer.resume: %s was written with (ada_target, ada_interval, ada_kimg) = %r, this run uses %r; the saved "
                              "p and interval continue under the new parameters" % (name, saved, tuple(t.ada[2:])))

        def restart_ada():
            t._ada.zero_()
            t._ada[0] = t.ada[0]
        out.append(Sidecar("ada", lambda: {"state": t._ada.cpu().clone(), "target": t.ada[2], "interval": t.ada[3], "kimg": t.ada[4]}, load_ada,
                           restart_ada, "aclgan_Trainer.resume: %%s not found; the augmentation probability starts again at %g" % t.ada[0]))
    return out


class Checkpoints:
    """save / resume of aclgan_Trainer (a base class of it: the methods read the trainer's own attributes)"""

    def _opt_entries(self, grp):
        """(index, net, table entry) of every tensor of a group, in the order of the reference optimizer's params"""
        nets = (self.gen_AB, self.gen_BA) if grp == L.GROUP_GEN else (self.dis_A, self.dis_B, self.dis_2)
        return enumerate((net, e) for net in nets for e in net._entries)

    def _opt_state_dict(self, grp):
        """torch.optim.Adam.state_dict() layout so that the reference can load optimizer.pt."""
        o = self._opt[grp]
        state, count = {}, 0
        for idx, (net, e) in self._opt_entries(grp):
            count += 1
            if o["steps"] > 0:
                state[idx] = {"step": torch.tensor(float(o["steps"])),
                              "exp_avg": net._view(e, self._m[grp]).contiguous().clone(),
                              "exp_avg_sq": net._view(e, self._v[grp]).contiguous().clone()}
        pg = {"lr": self._current_lr(self._hp), "betas": (o["beta1"], o["beta2"]), "eps": o["eps"], "weight_decay": o["weight_decay"],
              "amsgrad": False, "initial_lr": float(self._hp["lr"]), "params": list(range(count))}
        return {"state": state, "param_groups": [pg]}

    def _load_opt_state_dict(self, grp, sd):
        o = self._opt[grp]
        steps = 0
        with torch.no_grad():
            for idx, (net, e) in self._opt_entries(grp):
                st = sd["state"].get(idx)
                if st is not None:
                    net._view(e, self._m[grp]).copy_(st["exp_avg"].to(self.device))
                    net._view(e, self._v[grp]).copy_(st["exp_avg_sq"].to(self.device))
                    steps = int(float(st["step"]))
        o["steps"] = steps
        pg = sd["param_groups"][0]
        o.update(beta1=float(pg["betas"][0]), beta2=float(pg["betas"][1]), eps=float(pg["eps"]), weight_decay=float(pg["weight_decay"]))

    def save(self, snapshot_dir, iterations):
        name = lambda stem: os.path.join(snapshot_dir, "%s_%08d.pt" % (stem, iterations + 1))      # noqa: E731
        torch.save({"AB": _cpu(self.gen_AB.state_dict()), "BA": _cpu(self.gen_BA.state_dict())}, name("gen"))
        torch.save({"A": _cpu(self.dis_A.state_dict()), "B": _cpu(self.dis_B.state_dict()), "2": _cpu(self.dis_2.state_dict())}, name("dis"))
        opt = {"gen": self._opt_state_dict(L.GROUP_GEN), "dis": self._opt_state_dict(L.GROUP_DIS)}
        opt.update((s.where, s.payload()) for s in _opt_extras(self))
        torch.save(opt, os.path.join(snapshot_dir, "optimizer.pt"))
        for s in _file_states(self):
            torch.save(s.payload(), name(s.where))

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
        opt = torch.load(os.path.join(checkpoint_dir, "optimizer.pt"), map_location="cpu")
        self._load_opt_state_dict(L.GROUP_DIS, opt["dis"]); self._load_opt_state_dict(L.GROUP_GEN, opt["gen"])
        found = [(s, opt.get(s.where), "optimizer.pt") for s in _opt_extras(self)]
        # get_scheduler(..., iterations) (trainer.py:318-320, utils.py:263-271) builds StepLR(last_epoch=iterations).  The reference
        # pins torch 1.2.0 (acl-gan.yaml), whose _LRScheduler.__init__ ends with self.step(last_epoch): the scheduler resumes AT
        # last_epoch = iterations and (closed-form get_lr of that version) lr = lr0 * gamma ** (iterations // step_size).  torch >= 1.4
        # calls self.step() instead and would resume one epoch later (iterations + 1) -- the pinned version is the one mirrored here
        # (ACLGAN_RESUME_SCHED_PLUS1=1 selects the torch >= 1.4 behaviour).
        self._sched_calls = iterations + (1 if os.environ.get("ACLGAN_RESUME_SCHED_PLUS1") == "1" else 0)
        for s in _file_states(self):
            name = os.path.join(checkpoint_dir, "%s_%08d.pt" % (s.where, iterations))
            found.append((s, torch.load(name, map_location="cpu") if os.path.isfile(name) else None, name))
        for s, saved, name in found:      # (a file is read before the state listed ahead of it is taken: nothing of the trainer depends on that)
            if saved is not None:
                s.load(saved, name)
                continue
            if s.absent:
                warnings.warn(s.absent % name)
            if s.restart:
                s.restart()
        self._hp = hyperparameters
        self._setup_data_parallel()
        print("Resume from iteration %d" % iterations)
        return iterations
