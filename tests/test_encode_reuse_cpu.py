"""Content encodings of x_a carried from dis_update into gen_update (aclgan_ctx_carry_encodings), the host half without a GPU: the new
symbol in the header and in the ctypes table, the tuning keys, the argument checks, and the dry runs -- a workspace sized with the reuse on
holds the carry region on top of what it held before, and the executed-work figures do not move until a real gen_update has adopted.
Fake device pointers, nothing is launched (tests/test_ema_cpu.py does the same)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT


def _lib():
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib
    return _lib


@pytest.fixture()
def ctx():
    L = _lib()
    a = L.Arch(3, 6, 16, 32, 8, 4, 2, 2, 16, 4, 3)      # the reduced-width fixture network of the GPU tests
    c = C.c_void_p()
    L.check(L.lib.aclgan_ctx_create(C.byref(a), C.byref(c)))
    fake = C.c_void_p(0x10000)      # device pointers are never dereferenced on the host
    for grp in (0, 1):
        L.check(L.lib.aclgan_bind_params(c, grp, fake, fake, fake, fake))
    prev = C.c_int()
    L.check(L.lib.aclgan_tuning(b"enc_reuse", 1, C.byref(prev)))
    yield L, c
    L.check(L.lib.aclgan_tuning(b"enc_reuse", prev.value, None))
    L.lib.aclgan_ctx_destroy(c)


def _ws(L, c, B, H, W):
    v = C.c_size_t()
    L.check(L.lib.aclgan_workspace_bytes(c, B, H, W, C.byref(v)), "workspace_bytes")
    return v.value


def test_header_and_ctypes_table_agree_on_the_new_symbol():
    L = _lib()
    header = open(os.path.join(ROOT, "include", "aclgan_hip.h")).read()
    assert re.search(r"^int aclgan_ctx_carry_encodings\(aclgan_ctx\* ctx, int mode\);", header, re.M)
    assert L.SIGNATURES["aclgan_ctx_carry_encodings"] == (C.c_int, [C.c_void_p, C.c_int])
    for name, value in (("OFF", 0), ("KEEP", 1), ("ADOPT", 2)):
        assert re.search(r"^#define ACLGAN_CARRY_%s %d$" % (name, value), header, re.M), name
        assert getattr(L, "CARRY_" + name) == value


def test_switch_registry_lists_enc_reuse_and_the_hit_counter_is_read_only(ctx):
    L, c = ctx
    v = C.c_longlong(-7)
    L.check(L.lib.aclgan_tuning_get(b"enc_reuse", C.byref(v)))
    assert v.value == 1
    prev = C.c_int(-7)
    L.check(L.lib.aclgan_tuning(b"enc_reuse", 0, C.byref(prev)))
    L.check(L.lib.aclgan_tuning_get(b"enc_reuse", C.byref(v)))
    assert (prev.value, v.value) == (1, 0)
    L.check(L.lib.aclgan_tuning(b"enc_reuse", 5, None))      # a boolean: nonzero -> 1
    L.check(L.lib.aclgan_tuning_get(b"enc_reuse", C.byref(v)))
    assert v.value == 1
    L.check(L.lib.aclgan_tuning_get(b"enc_reuse_hits", C.byref(v)))
    assert v.value >= 0                                        # (passes adopted so far in this process)
    assert L.lib.aclgan_tuning(b"enc_reuse_hits", 3, None) == -1 and "unknown key" in L.last_error()


def test_carry_mode_argument_checks(ctx):
    L, c = ctx
    for mode in (L.CARRY_KEEP, L.CARRY_ADOPT, L.CARRY_OFF):
        assert L.lib.aclgan_ctx_carry_encodings(c, mode) == 0
    assert L.lib.aclgan_ctx_carry_encodings(c, 3) == -1 and "ACLGAN_CARRY" in L.last_error()
    assert L.lib.aclgan_ctx_carry_encodings(c, -1) == -1
    assert L.lib.aclgan_ctx_carry_encodings(None, L.CARRY_KEEP) == -1


@pytest.mark.parametrize("shape", [(2, 64, 64), (1, 64, 96), (3, 128, 64)])
def test_workspace_with_carry_armed_is_not_smaller(ctx, shape):
    L, c = ctx
    B, H, W = shape
    launches = L.lib.aclgan_launch_count()
    L.check(L.lib.aclgan_tuning(b"enc_reuse", 0, None))
    L.check(L.lib.aclgan_ctx_carry_encodings(c, L.CARRY_OFF))
    off = _ws(L, c, B, H, W)
    L.check(L.lib.aclgan_tuning(b"enc_reuse", 1, None))
    L.check(L.lib.aclgan_ctx_carry_encodings(c, L.CARRY_KEEP))
    keep = _ws(L, c, B, H, W)
    L.check(L.lib.aclgan_ctx_carry_encodings(c, L.CARRY_ADOPT))
    adopt = _ws(L, c, B, H, W)
    assert keep >= off and adopt == keep
    # (the size is the larger of the two updates' needs: the carried tensors leave the keeping dis_update's stack for the carry region, and
    #  gen_update, the larger of the two, sheds two passes when it adopts -- the total may not grow at all)
    # and a workspace of exactly that size passes the library's own check, one byte less does not
    fake = C.c_void_p(0x40000)
    L.check(L.lib.aclgan_bind_workspace(c, fake, keep))
    assert L.lib.aclgan_check_workspace(c, B, H, W) == 0, L.last_error()
    L.check(L.lib.aclgan_bind_workspace(c, fake, keep - 1))
    assert L.lib.aclgan_check_workspace(c, B, H, W) == -4 and "too small" in L.last_error()
    assert L.lib.aclgan_launch_count() == launches


def test_dry_run_figures_do_not_move_before_a_real_adoption(ctx):
    """aclgan_step_executed_flops / aclgan_step_algorithmic_bytes mirror the last REAL call of the update: arming alone changes nothing"""
    L, c = ctx

    def q(fn, which):
        v = C.c_double()
        L.check(fn(c, which, 2, 64, 64, C.byref(v)))
        return v.value
    before = [q(L.lib.aclgan_step_executed_flops, w) for w in (0, 1)] + [q(L.lib.aclgan_step_algorithmic_bytes, w) for w in (0, 1)]
    L.check(L.lib.aclgan_ctx_carry_encodings(c, L.CARRY_ADOPT))
    after = [q(L.lib.aclgan_step_executed_flops, w) for w in (0, 1)] + [q(L.lib.aclgan_step_algorithmic_bytes, w) for w in (0, 1)]
    assert before == after and all(x > 0 for x in before)
