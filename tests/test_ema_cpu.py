"""The averaged generator (ema_decay / ema_start / ema_display) without a GPU: the config keys, and the host half of the C ABI --
aclgan_bind_ema, aclgan_set_forward_weights, aclgan_adam_step_ema, aclgan_adam_flat_ema argument checks and the traffic count --
on a context with fake device pointers (nothing is launched: tests/test_abi_cpu.py does the same)."""
import ctypes as C
import os

import pytest

from conftest import ROOT


def _lib():
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib
    return _lib


def test_ema_from_config_defaults_are_off_and_bad_values_raise():
    L = _lib()
    from aclgan_amd.trainer import ema_from_config
    assert ema_from_config({}) == (0.0, 0, False)
    assert ema_from_config({"ema_decay": 0}) == (0.0, 0, False)
    assert ema_from_config({"ema_decay": 0.999, "ema_start": 100, "ema_display": True}) == (0.999, 100, True)
    assert ema_from_config({"ema_decay": 0.5, "ema_start": 0}) == (0.5, 0, False)
    for bad in (1.0, 1, 1.5, -0.1, -1, "0.9", None, True, float("nan"), 1 - 1e-12):      # (1 - 1e-12 is 1.0 as the C float the kernel gets)
        with pytest.raises(L.AclganError):
            ema_from_config({"ema_decay": bad})
    for bad in (-1, 1.5, "3", None, True):
        with pytest.raises(L.AclganError):
            ema_from_config({"ema_decay": 0.9, "ema_start": bad})
    for bad in (1, "yes", None):
        with pytest.raises(L.AclganError):
            ema_from_config({"ema_decay": 0.9, "ema_display": bad})
    with pytest.raises(L.AclganError):      # nothing to display
        ema_from_config({"ema_display": True})


def test_shipped_configs_leave_the_average_off():
    import yaml
    from aclgan_amd.trainer import ema_from_config
    for name in ("male2female", "male2female_sn", "selfie2anime", "glasses_removal"):
        cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", name + ".yaml")))
        assert ema_from_config(cfg) == (0.0, 0, False), name


@pytest.fixture()
def ctx():
    L = _lib()
    a = L.Arch(3, 6, 64, 256, 8, 4, 2, 4, 64, 4, 3)
    c = C.c_void_p()
    L.check(L.lib.aclgan_ctx_create(C.byref(a), C.byref(c)))
    fake = C.c_void_p(0x10000)      # device pointers are never dereferenced on the host
    for grp in (0, 1):
        L.check(L.lib.aclgan_bind_params(c, grp, fake, fake, fake, fake))
    yield L, c
    L.lib.aclgan_ctx_destroy(c)


def test_average_binds_to_the_generator_group_only(ctx):
    L, c = ctx
    fake = C.c_void_p(0x20000)
    assert L.lib.aclgan_bind_ema(c, L.GROUP_DIS, fake) == -1
    assert "generator" in L.last_error()
    assert L.lib.aclgan_bind_ema(c, L.GROUP_SN_STATE, fake) == -1
    assert L.lib.aclgan_bind_ema(None, L.GROUP_GEN, fake) == -1
    assert L.lib.aclgan_bind_ema(c, L.GROUP_GEN, fake) == 0
    assert L.lib.aclgan_bind_ema(c, L.GROUP_GEN, None) == 0      # unbind


def test_forward_weights_switch_needs_a_bound_average(ctx):
    L, c = ctx
    fake = C.c_void_p(0x20000)
    assert L.lib.aclgan_set_forward_weights(c, L.WEIGHTS_LIVE) == 0
    assert L.lib.aclgan_set_forward_weights(c, L.WEIGHTS_EMA) == -1
    assert "aclgan_bind_ema" in L.last_error()
    assert L.lib.aclgan_set_forward_weights(c, 2) == -1
    L.check(L.lib.aclgan_bind_ema(c, L.GROUP_GEN, fake))
    assert L.lib.aclgan_set_forward_weights(c, L.WEIGHTS_EMA) == 0
    # unbinding falls back to the live weights: the selection cannot outlive the buffer
    L.check(L.lib.aclgan_bind_ema(c, L.GROUP_GEN, None))
    assert L.lib.aclgan_set_forward_weights(c, L.WEIGHTS_EMA) == -1
    # the dry runs go through the same weight accessors whatever the switch says
    L.check(L.lib.aclgan_bind_ema(c, L.GROUP_GEN, fake))
    L.check(L.lib.aclgan_set_forward_weights(c, L.WEIGHTS_EMA))
    need = C.c_size_t()
    L.check(L.lib.aclgan_forward_workspace_bytes(c, 1, 64, 64, C.byref(need)))
    assert need.value > 0
    assert L.lib.aclgan_launch_count() == 0


def test_traffic_count_grows_by_eight_bytes_per_generator_parameter(ctx):
    L, c = ctx

    def q(which):
        v = C.c_double()
        L.check(L.lib.aclgan_step_algorithmic_bytes(c, which, 2, 64, 64, C.byref(v)))
        return v.value
    gen0, dis0 = q(0), q(1)
    L.check(L.lib.aclgan_bind_ema(c, L.GROUP_GEN, C.c_void_p(0x20000)))
    n = L.lib.aclgan_group_numel(c, L.GROUP_GEN)
    assert n >= 30058648
    assert q(0) - gen0 == 8.0 * n      # (both figures are integers far below 2^53: the difference is exact)
    assert q(1) == dis0
    L.check(L.lib.aclgan_bind_ema(c, L.GROUP_GEN, None))
    assert q(0) == gen0 and q(1) == dis0
    assert L.lib.aclgan_launch_count() == 0


def test_ema_adam_argument_checks_return_codes_before_any_launch(ctx):
    L, c = ctx
    fake = C.c_void_p(0x10000)
    adam = L.Adam(1e-4, 0.5, 0.999, 1e-8, 1e-4)
    st = C.c_void_p(0)
    # context level: a bound average, the generator group
    assert L.lib.aclgan_adam_step_ema(c, L.GROUP_GEN, C.byref(adam), 1, 0.5, L.EMA_BLEND, st) == -1
    assert "aclgan_bind_ema" in L.last_error()
    L.check(L.lib.aclgan_bind_ema(c, L.GROUP_GEN, C.c_void_p(0x20000)))
    assert L.lib.aclgan_adam_step_ema(c, L.GROUP_DIS, C.byref(adam), 1, 0.5, L.EMA_BLEND, st) == -1
    for decay, mode in ((1.0, L.EMA_BLEND), (-0.5, L.EMA_BLEND), (float("nan"), L.EMA_BLEND), (0.5, 2), (0.5, -1)):
        assert L.lib.aclgan_adam_step_ema(c, L.GROUP_GEN, C.byref(adam), 1, decay, mode, st) == -1, (decay, mode)
        assert L.lib.aclgan_adam_flat_ema(fake, fake, fake, fake, fake, 1000, C.byref(adam), 1, decay, mode, st) == -1, (decay, mode)
    assert L.lib.aclgan_adam_flat_ema(fake, fake, fake, fake, None, 1000, C.byref(adam), 1, 0.5, L.EMA_BLEND, st) == -1
    assert L.lib.aclgan_adam_flat_ema(fake, fake, fake, fake, fake, 1000, C.byref(adam), 0, 0.5, L.EMA_BLEND, st) == -1      # step >= 1
    assert L.lib.aclgan_launch_count() == 0
