"""The oracle's spectral norm (oracle/aclgan_oracle.py: dis.norm sn) replayed in float64 against the reference's SN fixtures
(tests/golden/make_golden_sn.py): the reduced width and the shipped width (9 SN matrices per discriminator, up to 512 x 4096).
CPU only.

Every bound is at least as tight as tests/test_oracle_golden.py's float64 bounds.  Measured (x86, torch 2.10):
  losses                       reduced 7.4e-15, full 2.3e-16 relative
  gradients (sum, norm, max)   reduced 6.8e-12, full 8.4e-12 of (norm + 1e-6 max norm): the worst are the conv biases in front of an
                               instance norm, whose gradient is rounding noise around 0; every weight_bar 1.3e-14 or less
  per-call sigma               reduced 3.5e-16, full 3.2e-16 relative
  u / v after each update      reduced 3.0e-8, full 1.3e-8 absolute (the fixture stores them in float32)
"""
import json
import os

import numpy as np
import pytest
import torch

from oracle import aclgan_oracle as O

from conftest import GOLDEN

DIS = ("dis_A", "dis_B", "dis_2")
FIXTURES = ["step_reduced_64_sn_smooth", "step_full_64_sn_smooth"]


def _load(name):
    return json.load(open(os.path.join(GOLDEN, name + ".json"))), np.load(os.path.join(GOLDEN, name + ".npz"))


def _nets(meta, dd=torch.float64):
    from sn_nets import sn_test_nets
    return {k: {n: t.to(dd) for n, t in v.items()} for k, v in sn_test_nets(meta["config"], meta["seed"]).items()}


def _inputs(data, dd=torch.float64):
    T = lambda a: torch.from_numpy(np.asarray(a)).to(dd)  # noqa: E731
    return T(data["x_a"]), T(data["x_b"]), [T(data["z%d" % i]) for i in range(6)]


def _per_net(log, orc):
    """sn_sigmas records -> {net: [[sigma per SN layer] per call]}"""
    ids = {id(orc.nets[n]): n for n in DIS}
    out = {n: [] for n in DIS}
    for pid, sig in log.calls:
        out[ids[pid]].append(sig)
    return out


@pytest.fixture(scope="module", params=FIXTURES)
def replay(request):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    meta, data = _load(request.param)
    x_a, x_b, z = _inputs(data)
    nets = _nets(meta)
    orc_d = O.OracleTrainer(meta["config"], nets=nets)
    with O.sn_sigmas() as ld:
        orc_d.dis_update(x_a, x_b, z[:3])
    orc_g = O.OracleTrainer(meta["config"], nets=nets)
    with O.sn_sigmas() as lg:
        orc_g.gen_update(x_a, x_b, z[3:6])
    return request.param, meta, data, orc_d, orc_g, _per_net(ld, orc_d), _per_net(lg, orc_g)


def test_sn_state_dict_keys_match_reference():
    """dis_param_shapes with dis.norm sn: the reference's keys, shapes and order (bias, weight_u, weight_v, weight_bar per SN layer)"""
    want = {}
    for line in open(os.path.join(GOLDEN, "state_dict_keys_sn.txt")):
        net, key, shp = line.split()
        want.setdefault(net, []).append((key, tuple(int(s) for s in shp.split("x"))))
    meta, _ = _load("step_full_64_sn_smooth")
    cfg = meta["config"]
    assert cfg["dis"]["norm"] == "sn" and cfg["dis"]["dim"] == 64
    for net, cin in (("dis_A", 3), ("dis_B", 3), ("dis_2", 6)):
        assert list(O.dis_param_shapes(cin, cfg["dis"]).items()) == want[net], net
    # the fixture's initial state (tests/sn_nets.py) holds exactly those tensors
    nets = _nets(meta)
    for net in DIS:
        assert {k: tuple(v.shape) for k, v in nets[net].items()} == dict(want[net]), net


def test_full_width_fixture_pins_the_shipped_sn_matrices():
    """the GPU tests that replay step_full_64_sn_smooth rely on the 9 SN layers per discriminator of the shipped width"""
    meta, _ = _load("step_full_64_sn_smooth")
    shapes = [(s[0], int(np.prod(s[1:]))) for k, s in O.dis_param_shapes(3, meta["config"]["dis"]).items() if k.endswith("weight_bar")]
    assert shapes == [(128, 1024), (256, 2048), (512, 4096)] * 3
    assert all(len(calls[0]) == 9 for calls in meta["sigma_dis"].values())


def test_sn_losses(replay):
    name, meta, _, orc_d, orc_g, _, _ = replay
    losses = dict(orc_d.losses)
    losses.update(orc_g.losses)
    assert len(meta["losses"]) == 16
    for n, v in meta["losses"].items():
        assert abs(losses[n] - v) <= 1e-9 * max(1.0, abs(v)), (name, n, losses[n], v)


def test_sn_gradient_stats(replay):
    """every gradient of both updates: sum, norm and max, 1e-8 relative to the tensor's norm (+1e-12 of the largest norm: the biases
    in front of an instance norm have a gradient of pure rounding noise)"""
    name, meta, _, orc_d, orc_g, _, _ = replay
    gmax = max(v[1] for v in meta["grad_stats"].values())
    seen = 0
    for key, ref in meta["grad_stats"].items():
        upd, net, k = key.split("/", 2)
        g = (orc_d if upd == "dis_update" else orc_g).nets[net][k].grad
        got = (float(g.sum()), float(g.norm()), float(g.abs().max()))
        for a, b in zip(got, ref):
            assert abs(a - b) <= 1e-8 * ref[1] + 1e-12 * gmax, (name, key, got, ref)
        seen += 1
    # every discriminator parameter of dis_update, u / v excluded, and every generator parameter of gen_update
    want = sum(1 for n in DIS for k in orc_d.nets[n] if not O.is_sn_state(k)) + sum(len(orc_g.nets[n]) for n in ("gen_AB", "gen_BA"))
    assert seen == want


def test_sn_per_call_sigmas(replay):
    """one power iteration per discriminator call, in the reference's call order: dis_update calls dis_A 4 times (fake, real, fake,
    real), dis_B and dis_2 twice; gen_update calls dis_A and dis_2 twice and dis_B once"""
    name, meta, _, _, _, sd, sg = replay
    for ours, ref, counts in ((sd, meta["sigma_dis"], (4, 2, 2)), (sg, meta["sigma_gen"], (2, 1, 2))):
        for net, cnt in zip(DIS, counts):
            assert len(ours[net]) == len(ref[net]) == cnt, (name, net)
            for a, b in zip(ours[net], ref[net]):
                assert len(a) == len(b)
                assert np.allclose(a, b, rtol=1e-12, atol=0), (name, net, a, b)


def test_sn_u_v_after_each_update(replay):
    name, _, data, orc_d, orc_g, _, _ = replay
    for prefix, orc in (("uv_dis", orc_d), ("uv_gen", orc_g)):
        n = 0
        for net in DIS:
            for k, t in orc.nets[net].items():
                if O.is_sn_state(k):
                    ref = torch.from_numpy(data["%s/%s/%s" % (prefix, net, k)]).double()
                    assert (t - ref).abs().max().item() <= 1e-7, (name, prefix, net, k)    # float32 storage of unit vectors
                    assert not t.requires_grad
                    n += 1
        assert n == 2 * sum(1 for net in DIS for k in orc.nets[net] if k.endswith("weight_bar"))


def test_sn_params_after_dis_adam(replay):
    """the discriminator parameters after dis_update + Adam (u / v are not in dis_opt)"""
    name, meta, _, orc_d, _, _, _ = replay
    assert set(meta["param_stats_after_dis"]) == {"%s/%s" % (n, k) for n in DIS for k in orc_d.nets[n] if not O.is_sn_state(k)}
    for key, (s, nrm, mx) in meta["param_stats_after_dis"].items():
        net, k = key.split("/", 1)
        p = orc_d.nets[net][k].detach()
        assert abs(float(p.sum()) - s) <= 1e-9 * max(1.0, nrm), (name, key)
        assert abs(float(p.norm()) - nrm) <= 1e-9 * max(1.0, nrm), (name, key)


@pytest.mark.parametrize("name", FIXTURES)
def test_sn_three_chained_steps(name):
    """three dis -> gen steps in the train.py order, u / v carried from call to call: every loss of every step"""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    meta, data = _load(name)
    x_a, x_b, z = _inputs(data)
    orc = O.OracleTrainer(meta["config"], nets=_nets(meta))
    for step, ref in enumerate(meta["seq_losses"]):
        orc.dis_update(x_a, x_b, z[:3])
        orc.gen_update(x_a, x_b, z[3:6])
        for n, v in ref.items():
            assert abs(orc.losses[n] - v) <= 1e-9 * max(1.0, abs(v)), (name, step, n, orc.losses[n], v)
    if "seq_uv/dis_A/cnns.0.1.conv.module.weight_u" in data.files:
        for net in DIS:
            for k, t in orc.nets[net].items():
                if O.is_sn_state(k):
                    assert (t - torch.from_numpy(data["seq_uv/%s/%s" % (net, k)]).double()).abs().max().item() <= 1e-7, (net, k)


def test_sn_backward_reads_the_last_calls_u_v():
    """the reference's quirk, restated: u / v are replaced through .data after autograd saved them, so d sigma / d W_bar of EVERY call
    is u v^T of the last call (a backward with each call's own u / v misses the reduced fixture's weight_bar gradients by up to 1.8e-2)"""
    torch.manual_seed(0)
    P = {"m.weight_bar": torch.randn(6, 2, 2, 2, dtype=torch.float64, requires_grad=True),
         "m.weight_u": torch.randn(6, dtype=torch.float64), "m.weight_v": torch.randn(8, dtype=torch.float64)}
    _, s1 = O.spectral_norm_weight(P, "m.")
    u1, v1 = P["m.weight_u"].clone(), P["m.weight_v"].clone()
    _, s2 = O.spectral_norm_weight(P, "m.")
    u2, v2 = P["m.weight_u"].clone(), P["m.weight_v"].clone()
    assert float(s1.detach()) == float(u1 @ (P["m.weight_bar"].detach().reshape(6, -1) @ v1))      # the forward value is the call's own
    g, = torch.autograd.grad(s1, P["m.weight_bar"])
    assert torch.allclose(g.reshape(6, -1), torch.outer(u2, v2), rtol=0, atol=1e-15)
    assert (g.reshape(6, -1) - torch.outer(u1, v1)).abs().max().item() > 1e-3
