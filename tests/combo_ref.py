"""The composed oracle of the training keys for the tests (tests/test_combo_cpu.py, tests/test_gpu_combo.py): ONE dis_update / gen_update of the
fp32 oracle with several keys on at once.  Nothing is restated here -- every key keeps the reference module its own tests use:
  dis_augment        diffaug_ref.oracle_dis_forward around oracle.dis_forward, the rows gated by ada_ref.gate when a p is given (dis_augment_p)
  lecam_lambda       lecam_ref.oracle_lsgan around oracle.lsgan (dis_update only; lam_eff and the anchors of count 0 as the header states them)
  ms_lambda          modeseek_ref.gen_losses_ms on top of oracle.gen_losses, which calls the wrapped dis_forward
  r1_gamma           r1_ref.r1_autograd on (dis_A, x_a) and (dis_B, x_b) with gamma * r1_every, added to the discriminator gradients
grad_clip and ema_decay act on the finished gradient buffer: gradclip_ref models them, the tests apply it to what this module returns.
The module attributes of the oracle are replaced for the duration of one update and restored on every path (patched).
Not a test module.  case() builds the shared reduced-width fixtures of the two test modules."""
import copy
from collections import OrderedDict
from contextlib import contextmanager

import numpy as np
import torch

from oracle import aclgan_oracle as O
import ada_ref
import lecam_ref
import r1_ref
from diffaug_ref import DIS_BLOCKS, GEN_BLOCKS, oracle_dis_forward
from modeseek_ref import gen_losses_ms

DIS_NETS, GEN_NETS = ("dis_A", "dis_B", "dis_2"), ("gen_AB", "gen_BA")
AUG_BITS = {"color": 1, "translation": 2, "cutout": 4}
REAL_CALLS = ((1, "A", 0.5), (3, "A", 0.5), (5, "B", 1.0))      # oracle.dis_losses: the dis_forward calls on x_a, x_a, x_b and the weight of their lsgan term


def policy_of(cfg):
    v = cfg.get("dis_augment", "")
    return sum(AUG_BITS[t.strip()] for t in v.split(",")) if v.strip() else 0


@contextmanager
def patched(**attrs):
    """oracle.aclgan_oracle.<name> = value for the body; the previous attributes come back on every path"""
    prev = {k: getattr(O, k) for k in attrs}
    try:
        for k, v in attrs.items():
            setattr(O, k, v)
        yield
    finally:
        for k, v in prev.items():
            setattr(O, k, v)


def _recording(inner):
    """dis_forward that keeps the outputs of every call, in call order (outermost: it sees what the discriminator returned for the augmented input)"""
    outs = []

    def wrapper(P, x, dcfg):
        o = inner(P, x, dcfg)
        outs.append([t.detach().clone() for t in o])
        return o
    wrapper.outs = outs
    return wrapper


def effective_rows(cfg, aug, aug_u, p, H, W):
    """the rows an update applies: the rows themselves, or under dis_augment_p the gate's select with p as float32"""
    if aug is None or p is None:
        return aug
    eff = ada_ref.gate(aug.numpy(), aug_u.numpy(), np.float32(p), H, W, policy_of(cfg))
    return torch.from_numpy(eff)


def _dis_forward_for(cfg, aug, aug_u, p, x_a, blocks):
    policy = policy_of(cfg)
    inner, wf = O.dis_forward, None
    if policy:
        assert aug is not None and aug.shape[0] == (max(blocks) + 1) * x_a.shape[0], "dis_augment needs this update's rows"
        rows = effective_rows(cfg, aug, aug_u, p, x_a.shape[2], x_a.shape[3])
        inner = wf = oracle_dis_forward(O.dis_forward, rows, x_a.shape[0], policy, blocks)
    return _recording(inner), wf


def is_param(cfg, key):
    """a tensor an optimizer owns: not the power-iteration state, not the generators' unused AdaIN running statistics"""
    return not O.is_sn_state(key) and key not in O.gen_buffer_shapes(cfg["gen"])


def _grads(orc, names):
    return OrderedDict(((n, k), (t.grad.detach().clone() if t.grad is not None else torch.zeros_like(t)))
                       for n in names for k, t in orc.nets[n].items() if is_param(orc.hp, k))


def dis_update(cfg, nets, x_a, x_b, z, aug=None, aug_u=None, p=None, anchors=None, lecam_count=0, r1=None):
    """one dis_update at `nets`.  z = (z_1, z_2, z_3); aug (7 B, 8) rows, aug_u (7 B, 4) uniforms and p under dis_augment / dis_augment_p;
    anchors {'A','B','2'} -> per scale (fake, real) and lecam_count (the updates folded so far) under lecam_lambda; r1: whether the pass runs on
    this update (default: whenever r1_gamma > 0)."""
    orc = O.OracleTrainer(cfg, nets=nets)
    rec_f, wf = _dis_forward_for(cfg, aug, aug_u, p, x_a, DIS_BLOCKS)
    attrs, wl = {"dis_forward": rec_f}, None
    lam = float(cfg.get("lecam_lambda", 0))
    if lam > 0:
        lam_eff = lam if lecam_count >= max(int(cfg.get("lecam_start", 1000)), 1) else 0.0
        wl = lecam_ref.oracle_lsgan(O.lsgan, anchors if lecam_count > 0 else None, lam_eff)
        attrs["lsgan"] = wl
    else:      # the call count only: the value and the graph of every call are the oracle's own
        seen, orig = [], O.lsgan

        def counted(outs, target):
            seen.append(float(target))
            return orig(outs, target)
        attrs["lsgan"] = counted
    with patched(**attrs):
        orc.dis_update(x_a, x_b, list(z), apply=False)
    out = {"losses": dict(orc.losses), "grads": _grads(orc, DIS_NETS),
           "calls": {"dis_forward": len(rec_f.outs), "augment": None if wf is None else len(wf.calls), "blocks": len(DIS_BLOCKS),
                     "lsgan": len(wl.rec["means"]) if wl is not None else len(seen)},
           "real_outs": [(D, w, rec_f.outs[k]) for k, D, w in REAL_CALLS], "lecam": None, "class_means": None, "r1": None}
    if wl is not None:
        out["lecam"] = lecam_ref.lecam_values(wl.rec)
        out["class_means"] = lecam_ref.class_means(wl.rec)
    gamma = float(cfg.get("r1_gamma", 0))
    if gamma > 0 and (r1 is None or r1):
        out["r1"] = {}
        for D, x in (("dis_A", x_a), ("dis_B", x_b)):
            pen, _, g = r1_ref.r1_autograd(nets[D], x, cfg["dis"], gamma * int(cfg.get("r1_every", 16)))
            out["r1"][D[-1]] = float(pen)
            for k, t in g.items():
                out["grads"][(D, k)] = out["grads"][(D, k)] + t
    return out


def gen_update(cfg, nets, x_a, x_b, z, aug=None, aug_u=None, p=None, z_ms=None):
    """one gen_update at `nets`.  z = (z_1, z_2, z_3); aug (5 B, 8), aug_u (5 B, 4), p as above; z_ms = (z_4, z_5) under ms_lambda"""
    orc = O.OracleTrainer(cfg, nets=nets)
    rec_f, wf = _dis_forward_for(cfg, aug, aug_u, p, x_a, GEN_BLOCKS)
    lam = float(cfg.get("ms_lambda", 0))
    ms = None
    with patched(dis_forward=rec_f):
        if lam > 0:
            total, L, _, terms = gen_losses_ms(orc.nets, x_a, x_b, list(z), z_ms, cfg)
            (total + lam * (terms["ms_B"] + terms["ms_A"])).backward()
            losses = {k: float(v.detach()) for k, v in L.items()}
            ms = {k: float(v.detach()) for k, v in terms.items()}
        else:
            orc.gen_update(x_a, x_b, list(z), apply=False)
            losses = dict(orc.losses)
    return {"losses": losses, "grads": _grads(orc, GEN_NETS), "ms": ms,
            "calls": {"dis_forward": len(rec_f.outs), "augment": None if wf is None else len(wf.calls), "blocks": len(GEN_BLOCKS)}}


def sign_r(real_outs):
    """the overfitting signal of one dis_update: sum(w q) / sum(w) over the real-side maps (ada_ref.sign_q per map), and the smallest |o - 0.5|"""
    num = den = 0.0
    margin = float("inf")
    for _, w, maps in real_outs:
        for o in maps:
            num += w * ada_ref.sign_q(o.numpy())
            den += w
            margin = min(margin, float((o - 0.5).abs().min()))
    return num / den, margin


def group_change(a, b):
    """relative L2 distance of two gradient dicts over the whole group: ||a - b|| / ||b||"""
    num = sum(float((a[k].double() - b[k].double()).norm() ** 2) for k in b) ** 0.5
    return num / sum(float(b[k].double().norm() ** 2) for k in b) ** 0.5


# ---------------------------------------------------------------------------------------------------------------------------------
# the shared fixture
# ---------------------------------------------------------------------------------------------------------------------------------
B, S = 2, 64
ANCHORS = (0.2, 0.8)
# Chosen with the fp32 oracle on the CPU (tests/test_combo_cpu.py asserts what they are chosen for): per unit of lambda the mode-seeking term
# moves the generator gradient of these fixtures by 0.01 .. 0.04 relative L2, so 32 keeps it above 0.1 in every case; R1 at gamma 10 moves the
# discriminator gradient by 0.11, so 40; every gradient norm of the fixtures lies above 50, so a bound of 1 clips every update.
MS_LAMBDA = 32.0
R1_GAMMA = 40.0
GRAD_CLIP = 1.0
STACK_A = dict(dis_augment="color,translation,cutout", dis_augment_p=0.5, lecam_lambda=1.0, lecam_start=0, lecam_decay=0.9, ms_lambda=MS_LAMBDA,
               grad_clip=GRAD_CLIP, ema_decay=0.9)
STACK_B = dict(r1_gamma=R1_GAMMA, r1_every=1, lecam_lambda=1.0, lecam_start=0, lecam_decay=0.9, ms_lambda=MS_LAMBDA, grad_clip=GRAD_CLIP, ema_decay=0.9)
STACKS = {"A": STACK_A, "B": STACK_B}
# (stack, dis.norm, configuration).  R1 refuses dis.norm sn and dis_augment, so stack B has no sn twin
CASES = [("A", "none", "focus"), ("A", "none", "plain"), ("A", "sn", "focus"), ("A", "sn", "plain"), ("B", "none", "focus"), ("B", "none", "plain")]
# the discriminators' weight scale per dis.norm.  Under sn the layers 1 .. 3 of every scale are normalised whatever their scale, only the first
# layer and the 1x1 head keep it: x 75 there gives the adversarial gradients the weight x 10 gives them without normalisation
WEIGHT_SCALE = {"none": 10.0, "sn": 75.0}
BATCH_SEED = 500
# which keys act on which update: (key, the keys to drop with it).  Dropping dis_augment_p leaves the rows ungated
ACTS_ON = {"A": {"dis": ("dis_augment", "dis_augment_p", "lecam_lambda"), "gen": ("dis_augment", "dis_augment_p", "ms_lambda")},
           "B": {"dis": ("r1_gamma", "lecam_lambda"), "gen": ("ms_lambda",)}}


def base_config(kind="focus", norm="none", dim=8):
    """reduced width; kind 'focus' (the default configuration) or 'plain' (focus_loss 0, gen.output_dim 3)"""
    cfg = O.default_config()
    cfg["gen"].update(dim=dim, mlp_dim=2 * dim, n_res=2)
    cfg["dis"].update(dim=dim, n_layer=4, num_scales=3, norm=norm)
    cfg["display_size"] = 1
    cfg["focus_epsilon"] = 0.5
    if kind == "plain":
        cfg["focus_loss"] = 0
        cfg["gen"]["output_dim"] = 3
    return cfg


def scaled_nets(cfg, seed=4, scale=10.0):
    """oracle.test_nets (sn: its twin) with the discriminators' *weight tensors x scale: at the fill's own scale the discriminator outputs
    barely depend on their input (tests/test_gpu_diffaugment.py)"""
    if cfg["dis"].get("norm", "none") == "sn":
        from sn_nets import sn_test_nets
        nets = sn_test_nets(cfg, seed)
    else:
        nets = O.test_nets(cfg, seed)
    for n in DIS_NETS:
        nets[n] = {k: (v * scale if k.endswith("weight") else v) for k, v in nets[n].items()}
    return nets


def draw_rows(rows, H, W, g):
    """(rows, 8) augmentation rows of policy 7 with DiffAugment's ranges, from a torch generator (explicit inputs of both sides of a comparison)"""
    p = torch.zeros(rows, 8)
    p[:, 0] = torch.rand(rows, generator=g) - 0.5
    p[:, 1] = torch.rand(rows, generator=g) * 2.0
    p[:, 2] = torch.rand(rows, generator=g) + 0.5
    p[:, 3] = torch.randint(-(W // 8), W // 8 + 1, (rows,), generator=g).float()
    p[:, 4] = torch.randint(-(H // 8), H // 8 + 1, (rows,), generator=g).float()
    p[:, 5] = (torch.randint(0, W + 1, (rows,), generator=g) - W // 4).float()
    p[:, 6] = (torch.randint(0, H + 1, (rows,), generator=g) - H // 4).float()
    return p


def batch(seed, style_dim=8):
    """everything one iteration reads: x_a, x_b, z (6), the rows and uniforms of both updates, z_ms"""
    g = torch.Generator().manual_seed(seed)
    x_a = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    x_b = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    z = [torch.randn(B, style_dim, 1, 1, generator=g) for _ in range(6)]
    out = dict(x_a=x_a, x_b=x_b, z=z, aug_d=draw_rows(7 * B, S, S, g), aug_g=draw_rows(5 * B, S, S, g),
               u_d=torch.rand(7 * B, 4, generator=g), u_g=torch.rand(5 * B, 4, generator=g),
               z_ms=[torch.randn(B, style_dim, 1, 1, generator=g) for _ in range(2)])
    return out


def case(stack, norm, kind, dim=8):
    """(config with the stack's keys, nets, the iteration's inputs) of one of CASES"""
    cfg = with_keys(base_config(kind, norm, dim), **STACKS[stack])
    return cfg, scaled_nets(cfg, scale=WEIGHT_SCALE[norm]), batch(BATCH_SEED)


# the 16-bit fixture.  At fp16's loss scale of 65536 the x 10 fixture overflows in both updates -- measured with every key off too: its
# discriminator outputs reach |o| = 10 -- so the 1x1 heads keep a tenth of it (|o| < 2).  The adversarial gradient of the generators shrinks with
# them; ms_lambda 4 and a second noise pair a quarter as far away keep the mode-seeking term from drowning it (tests/test_combo_cpu.py)
HEAD16, MS_LAMBDA16, ZMS16 = 0.1, 4.0, 0.25


def case16():
    cfg, nets, b = case("A", "none", "focus")
    cfg["ms_lambda"] = MS_LAMBDA16
    for D in DIS_NETS:
        for s in range(cfg["dis"]["num_scales"]):
            k = "cnns.%d.%d.weight" % (s, cfg["dis"]["n_layer"])
            nets[D][k] = nets[D][k] * HEAD16
    b["z_ms"] = [t * ZMS16 for t in b["z_ms"]]
    return cfg, nets, b


def drop_key(cfg, key):
    """the config with one key of its stack off (dis_augment takes dis_augment_p with it)"""
    return without(cfg, *(("dis_augment", "dis_augment_p") if key == "dis_augment" else (key,)))


def iteration(cfg, nets_d, nets_g, b, p=None, anchors=None, lecam_count=1, which=("dis", "gen")):
    """the composed oracle on one iteration's inputs: dis_update at nets_d, gen_update at nets_g, each with the inputs its config's keys read"""
    aug = policy_of(cfg) != 0
    p = (cfg.get("dis_augment_p") if p is None else p) if aug else None
    out = {}
    if "dis" in which:
        out["dis"] = dis_update(cfg, nets_d, b["x_a"], b["x_b"], b["z"][:3], aug=b["aug_d"] if aug else None, aug_u=b["u_d"] if p is not None else None,
                                p=p, anchors=anchors if anchors is not None else preset_anchors(cfg), lecam_count=lecam_count)
    if "gen" in which:
        out["gen"] = gen_update(cfg, nets_g, b["x_a"], b["x_b"], b["z"][3:], aug=b["aug_g"] if aug else None, aug_u=b["u_g"] if p is not None else None,
                                p=p, z_ms=b["z_ms"])
    return out


def preset_anchors(cfg):
    return {D: [list(ANCHORS) for _ in range(cfg["dis"]["num_scales"])] for D in lecam_ref.NETS}


def with_keys(cfg, **keys):
    out = copy.deepcopy(cfg)
    out.update(keys)
    return out


def without(cfg, *names):
    out = copy.deepcopy(cfg)
    for n in names:
        out.pop(n, None)
    return out
