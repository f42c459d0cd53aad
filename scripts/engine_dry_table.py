#!/usr/bin/env python3
"""Everything the step engine computes without a GPU, as one sorted JSON table: run it on two builds and compare the outputs byte for byte.

No GPU, no torch: ctypes through aclgan_amd._lib with fake non-null device pointers (a dry run never dereferences one), as
tests/test_abi_cpu.py does.  Per cell of the grid (architecture x dis_norm x dtype x augment policy x LeCam x shape x lanes x deterministic x
enc_reuse, gradient buckets of 2^20 elements): return code and value of aclgan_workspace_bytes, aclgan_forward_workspace_bytes,
aclgan_step_algorithmic_bytes and aclgan_step_executed_flops (both updates), the aclgan_bucket_schedule order of both groups (fire = 0; and
fire = 1 with a recording callback bound: what it was called with, and that no other dry run calls it), and
the parameter layout (aclgan_tensor_count / aclgan_tensor_info: the lists are printed once under "layouts", a cell names its own by hash).
Then the refused shapes with their error texts, and aclgan_launch_count() at exit (0)."""
import ctypes as C
import hashlib
import itertools
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aclgan_amd  # noqa: E402,F401
from aclgan_amd import _lib as L  # noqa: E402

FAKE = C.c_void_p(0x10000)
ARCHS = {"full": (3, 6, 64, 256, 8, 4, 2, 4, 64, 4, 3), "reduced": (3, 6, 8, 16, 8, 4, 2, 2, 8, 2, 3), "full_out3": (3, 6, 64, 256, 8, 3, 2, 4, 64, 4, 3)}
SHAPES = ((1, 64), (2, 64), (3, 256), (8, 256))
BUCKET = 1 << 20
FIRED = []
RECORD = L.BUCKET_FN(lambda user, group, bucket, off, n: FIRED.append([group, bucket, off, n]))


def make_ctx(arch, dis_norm, dtype, aug, lecam, B):
    ctx = C.c_void_p()
    a = L.Arch(*ARCHS[arch])
    L.check(L.lib.aclgan_ctx_create_dis_norm(C.byref(a), dis_norm, C.byref(ctx)))
    if dis_norm:
        L.check(L.lib.aclgan_bind_sn_state(ctx, FAKE))
    L.check(L.lib.aclgan_set_compute_dtype(ctx, dtype))
    for grp in (0, 1):
        L.check(L.lib.aclgan_bind_params(ctx, grp, FAKE, FAKE, FAKE, FAKE))
        if dtype:
            L.check(L.lib.aclgan_bind_params16(ctx, grp, FAKE, FAKE))
    L.check(L.lib.aclgan_ctx_set_augment(ctx, aug, FAKE if aug else None, 7 * B if aug else 0))
    if lecam:
        L.check(L.lib.aclgan_ctx_set_lecam(ctx, 1.0, 0.99, 0, FAKE))
    L.check(L.lib.aclgan_set_grad_buckets(ctx, BUCKET, RECORD, None))
    return ctx


def layout(ctx):
    out = []
    name = C.create_string_buffer(256); off = C.c_int64(); shp = (C.c_int * 4)(); nd = C.c_int()
    for grp in (0, 1, 2):
        n = L.lib.aclgan_tensor_count(ctx, grp)
        rows = []
        for i in range(n):
            rc = L.lib.aclgan_tensor_info(ctx, grp, i, name, 256, C.byref(off), shp, C.byref(nd))
            rows.append([rc, name.value.decode(), off.value, list(shp), nd.value])
        out.append({"count": n, "numel": L.lib.aclgan_group_numel(ctx, grp), "tensors": rows})
    return out


def sizes(ctx, B, S):
    r = {}
    del FIRED[:]
    v = C.c_size_t()
    rc = L.lib.aclgan_workspace_bytes(ctx, B, S, S, C.byref(v)); r["workspace_bytes"] = [rc, v.value if rc == 0 else L.last_error()]
    v = C.c_size_t()
    rc = L.lib.aclgan_forward_workspace_bytes(ctx, B, S, S, C.byref(v)); r["forward_workspace_bytes"] = [rc, v.value if rc == 0 else L.last_error()]
    for which in (0, 1):
        d = C.c_double()
        rc = L.lib.aclgan_step_algorithmic_bytes(ctx, which, B, S, S, C.byref(d)); r["algorithmic_bytes_%d" % which] = [rc, repr(d.value) if rc == 0 else L.last_error()]
        d = C.c_double()
        rc = L.lib.aclgan_step_executed_flops(ctx, which, B, S, S, C.byref(d)); r["executed_flops_%d" % which] = [rc, repr(d.value) if rc == 0 else L.last_error()]
    order = (C.c_int * 8192)(); cnt = C.c_int()
    for grp in (0, 1):
        rc = L.lib.aclgan_bucket_schedule(ctx, grp, B, S, S, 0, order, 8192, C.byref(cnt))
        r["bucket_schedule_%d" % grp] = [rc, [order[i] for i in range(cnt.value)] if rc == 0 else L.last_error()]
    r["fired_without_fire"] = list(FIRED)      # (no dry run but aclgan_bucket_schedule(fire = 1) calls the callback)
    for grp in (0, 1):
        del FIRED[:]
        rc = L.lib.aclgan_bucket_schedule(ctx, grp, B, S, S, 1, order, 8192, C.byref(cnt))
        r["bucket_fired_%d" % grp] = [rc, hashlib.sha256(json.dumps(FIRED).encode()).hexdigest(), len(FIRED)]
    return r


def main():
    table = {"cells": {}, "layouts": {}, "refused": {}}
    grid = itertools.product(ARCHS, (0, L.NORM["sn"]), (0, 1, 2), (0, 7), (0, 1), SHAPES, (1, 3), (0, 1), (0, 1))
    for arch, dis_norm, dtype, aug, lecam, (B, S), lanes, determ, reuse in grid:
        L.check(L.lib.aclgan_tuning(b"lanes", lanes, None))
        L.check(L.lib.aclgan_tuning(b"enc_reuse", reuse, None))
        L.lib.aclgan_set_deterministic(determ)
        ctx = make_ctx(arch, dis_norm, dtype, aug, lecam, B)
        cell = sizes(ctx, B, S)
        lay = layout(ctx)
        h = hashlib.sha256(json.dumps(lay, sort_keys=True).encode()).hexdigest()
        table["layouts"][h] = lay
        cell["layout"] = h
        table["cells"]["%s norm%d dtype%d aug%d lecam%d B%d S%d lanes%d determ%d reuse%d" % (arch, dis_norm, dtype, aug, lecam, B, S, lanes, determ, reuse)] = cell
        L.lib.aclgan_ctx_destroy(ctx)
    L.lib.aclgan_set_deterministic(0)
    for B, S in ((1, 32), (2, 66)):
        ctx = make_ctx("full", 0, 0, 0, 0, B)
        table["refused"]["B%d S%d" % (B, S)] = sizes(ctx, B, S)
        L.lib.aclgan_ctx_destroy(ctx)
    table["launch_count"] = L.lib.aclgan_launch_count()
    print(json.dumps(table, sort_keys=True, indent=1))
    return 0 if table["launch_count"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
