"""The fp32 oracle against the fp64 reference at the nine architectures of tests/arch_space.py (tests/golden/arch_space.json, written by
tests/golden/make_golden.py): the oracle is the yardstick of tests/test_gpu_arch_space.py, and tests/golden/step_*.json pin it only at the
default and reduced default architectures.  Tolerances: those of tests/test_oracle_golden.py for its smooth step fixtures.  CPU only."""
import json
import os

import pytest
import torch

from oracle import aclgan_oracle as O

import arch_space as A
from conftest import GOLDEN

META = json.load(open(os.path.join(GOLDEN, "arch_space.json")))


def test_fixture_lists_the_architectures():
    assert list(META) == list(A.ARCHS)
    for name, rec in META.items():
        cfg = A.arch_config(name)
        assert rec["config"]["gen"] == cfg["gen"] and rec["config"]["dis"] == cfg["dis"], name
        assert (rec["B"], rec["H"], rec["W"]) == A.arch_shape(name)
        assert (rec["net_seed"], rec["input_seed"], rec["config"]["focus_epsilon"]) == (A.NET_SEED, A.INPUT_SEED, 0.5)
        assert len([k for k in rec["fwd_stats"] if k.startswith("dis_A_xA_s")]) == cfg["dis"]["num_scales"]
        assert rec["fwd_stats"]["s_2"]["shape"] == [rec["B"], cfg["gen"]["style_dim"], 1, 1]


def _close(t, triple, rel):
    s, n, m = triple
    t = t.double()
    return abs(float(t.norm()) - n) <= rel * max(1.0, n) and abs(float(t.sum()) - s) <= 100 * rel * max(1.0, n) and \
        abs(float(t.abs().max()) - m) <= rel * max(1.0, m)


@pytest.mark.parametrize("name", list(A.ARCHS))
def test_seeded_inputs_and_weights_are_the_fixture_s(name):
    rec = META[name]
    x_a, x_b, z = A.arch_inputs(name)
    for k, t in [("x_a", x_a), ("x_b", x_b)] + [("z%d" % i, t) for i, t in enumerate(z)]:
        assert _close(t, rec["input_stats"][k], 1e-9), k
    nets = O.test_nets(A.arch_config(name), A.NET_SEED)
    assert sorted(rec["param_stats_initial"]) == sorted(nets)
    for net, rows in rec["param_stats_initial"].items():      # (one triple per parameter, in parameters() order)
        assert len(rows) == len(nets[net]), net
        for (k, t), (sm, nrm) in zip(nets[net].items(), rows):      # (a checksum of the seeded fill, stored to 8 digits)
            assert abs(float(t.double().norm()) - nrm) <= 1e-6 * max(1.0, nrm) and abs(float(t.double().sum()) - sm) <= 1e-4 * max(1.0, nrm), (net, k)


@pytest.mark.parametrize("name", list(A.ARCHS))
def test_step_fp32_within_fp32_noise(name):
    """losses 1e-4 rel (focus 'size' losses 1e-2), gradient norms 3e-3 rel + 1e-6 of the largest: test_oracle_golden's smooth bounds"""
    rec = META[name]
    cfg = A.arch_config(name)
    nets = O.test_nets(cfg, A.NET_SEED)
    x_a, x_b, z = A.arch_inputs(name)
    od = O.OracleTrainer(cfg, nets=nets)
    od.dis_update(x_a, x_b, z[:3], apply=False)
    losses = dict(od.losses)
    grads = {("dis_update", n, k): t.grad.clone() for n in ("dis_A", "dis_B", "dis_2") for k, t in od.nets[n].items()}
    og = O.OracleTrainer(cfg, nets=nets)
    og.gen_update(x_a, x_b, z[3:], apply=False)
    losses.update(og.losses)
    grads.update({("gen_update", n, k): t.grad for n in ("gen_AB", "gen_BA") for k, t in og.nets[n].items()})
    assert sorted(losses) == sorted(rec["losses"])
    for n, v in rec["losses"].items():
        tol = 1e-2 if n.endswith("_size") else 1e-4
        assert abs(losses[n] - v) <= tol * max(1e-3, abs(v)), (n, losses[n], v)
    assert sorted(rec["grad_stats"]) == sorted(nets)
    gmax = max(nrm for rows in rec["grad_stats"].values() for nrm in rows)
    for net, rows in rec["grad_stats"].items():
        upd = "dis_update" if net.startswith("dis") else "gen_update"
        assert len(rows) == len(nets[net]), net
        for k, nrm in zip(nets[net], rows):
            assert nrm > 0, (net, k)      # (no parameter of any of the nine has an all-zero gradient: the GPU test skips none)
            g = grads[(upd, net, k)]
            assert abs(float(g.double().norm()) - nrm) <= 3e-3 * nrm + 1e-6 * gmax, (net, k, float(g.norm()), nrm)


@pytest.mark.parametrize("name", list(A.ARCHS))
def test_forward_tensors_fp32(name):
    """every forward tensor's shape, and its norm and max|.| to 1e-4 (test_oracle_golden.test_forward_tensors_fp32's bound, on the triples)"""
    rec = META[name]
    cfg = A.arch_config(name)
    nets = O.test_nets(cfg, A.NET_SEED)
    x_a, x_b, z = A.arch_inputs(name)
    with torch.no_grad():
        fw = dict(O.generator_forward(nets["gen_AB"], nets["gen_BA"], x_a, x_b, z[:3], cfg, with_recon=False))
        fw["dec_AB_c1_z1"] = O.decode(nets["gen_AB"], fw["c_1"], z[0], cfg["gen"])
        fw["dec_BA_c2_z2"] = O.decode(nets["gen_BA"], fw["c_2"], cfg["alpha"] * z[1], cfg["gen"])
        dA = O.dis_forward(nets["dis_A"], fw["x_A_fake"], cfg["dis"])
        d2 = O.dis_forward(nets["dis_2"], torch.cat((x_a, fw["x_A2_fake"]), 1), cfg["dis"])
    assert len(dA) == len(d2) == cfg["dis"]["num_scales"]
    for s in range(len(dA)):
        fw["dis_A_xA_s%d" % s] = dA[s]
        fw["dis_2_pA2_s%d" % s] = d2[s]
    for k, ent in rec["fwd_stats"].items():
        t = fw[k]
        s, nrm, mx = ent["stats"]
        assert list(t.shape) == ent["shape"], k
        assert abs(float(t.double().norm()) - nrm) <= 1e-4 * max(1.0, nrm), (k, float(t.norm()), nrm)
        assert abs(float(t.abs().max()) - mx) <= 1e-4 * max(1.0, mx), k
