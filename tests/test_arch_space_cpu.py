"""Launch-free contract of the architecture space aclgan_ctx_create admits, on the nine architectures of tests/arch_space.py: what create
refuses, that every dry run (workspace, forward workspace, executed FLOPs, algorithmic bytes, bucket schedule) sizes every architecture in
every compute dtype with one and three lanes, that exactly the reported workspace passes aclgan_check_workspace, that the flat parameter
layout is the oracle's, and that an image too small for the architecture is refused up front by the config key that asks for more.
Each check drives libaclgan_hip.so in a fresh child process (tests/test_switches_cpu.py does the same): no GPU, no launch."""
import json
import os
import subprocess
import sys

from oracle import aclgan_oracle as O

import arch_space as A
from conftest import ROOT

LIB = os.path.join(ROOT, "acl-gan_amd", "libaclgan_hip.so")

CHILD = r'''
import ctypes as C, json, sys
L = C.CDLL(sys.argv[1])
L.aclgan_last_error.restype = C.c_char_p
L.aclgan_launch_count.restype = C.c_longlong
L.aclgan_group_numel.restype = C.c_int64
ARCH_FIELDS = ("input_dim_a", "input_dim_b", "gen_dim", "gen_mlp_dim", "gen_style_dim", "gen_output_dim", "gen_n_downsample", "gen_n_res",
               "dis_dim", "dis_n_layer", "dis_num_scales")
class Arch(C.Structure):
    _fields_ = [(n, C.c_int) for n in ARCH_FIELDS]
NONE, SN, ENOMEM = 0, 4, -4
FAKE = C.c_void_p(0x10000)      # device pointers are never dereferenced on the host
def err():
    return L.aclgan_last_error().decode()
def arch(gen, dis):
    gd, md, sd, nd, nr = gen
    dd, nl, ns = dis
    return Arch(3, 6, gd, md, sd, 4, nd, nr, dd, nl, ns)
def create(gen, dis, norm=NONE):
    ctx = C.c_void_p()
    rc = L.aclgan_ctx_create_dis_norm(C.byref(arch(gen, dis)), norm, C.byref(ctx))
    return rc, ctx
def bound(gen, dis, dtype=0):
    rc, ctx = create(gen, dis)
    assert rc == 0, err()
    assert L.aclgan_set_compute_dtype(ctx, dtype) == 0
    for grp in (0, 1):
        assert L.aclgan_bind_params(ctx, grp, FAKE, FAKE, FAKE, FAKE) == 0
        if dtype:
            assert L.aclgan_bind_params16(ctx, grp, FAKE, FAKE) == 0
    return ctx
def ws_bytes(ctx, B, H, W):
    ws = C.c_size_t()
    return L.aclgan_workspace_bytes(ctx, B, H, W, C.byref(ws)), ws.value
cases = json.load(open(sys.argv[2]))
out = {}
exec(sys.argv[3])
assert L.aclgan_launch_count() == 0
print(json.dumps(out))
'''


def _child(code, tmp_path, cases=None):
    f = tmp_path / "cases.json"
    f.write_text(json.dumps(cases if cases is not None else {}))
    e = {k: v for k, v in os.environ.items() if not k.startswith("ACLGAN_")}
    p = subprocess.run([sys.executable, "-c", CHILD, LIB, str(f), code], env=e, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def _cases():
    return {name: {"gen": list(g), "dis": list(d), "shape": list(s)} for name, (g, d, s) in A.ARCHS.items()}


def test_create_refusals(tmp_path):
    """gen.dim 12 and 3, dis.dim 6 and 2, every layer count 0, the mlp / style widths 0, and spectral norm with more than 16 normalised
    layers per discriminator: an error code and a message, no context"""
    base_g, base_d = [8, 16, 8, 2, 1], [8, 4, 3]
    bad = {"gen.dim 12": ([12, 16, 8, 2, 1], base_d, 0), "gen.dim 3": ([3, 16, 8, 2, 1], base_d, 0),
           "dis.dim 6": (base_g, [6, 4, 3], 0), "dis.dim 2": (base_g, [2, 4, 3], 0),
           "gen.n_downsample 0": ([8, 16, 8, 0, 1], base_d, 0), "gen.n_res 0": ([8, 16, 8, 2, 0], base_d, 0),
           "dis.n_layer 0": (base_g, [8, 0, 3], 0), "dis.num_scales 0": (base_g, [8, 4, 0], 0),
           "gen.mlp_dim 0": ([8, 0, 8, 2, 1], base_d, 0), "gen.style_dim 0": ([8, 16, 0, 2, 1], base_d, 0),
           "sn 17 layers": (base_g, [8, 2, 17], 4), "sn 3 x 6 layers": (base_g, [8, 7, 3], 4)}
    good = {"sn 16 layers": (base_g, [8, 2, 16], 4), "sn 4 x 4 layers": (base_g, [8, 5, 4], 4), "none 17 layers": (base_g, [8, 2, 17], 0)}
    code = r'''
for k, (g, d, norm) in cases["bad"].items():
    rc, ctx = create(g, d, norm)
    out[k] = [rc, err(), bool(ctx.value)]
for k, (g, d, norm) in cases["good"].items():
    rc, ctx = create(g, d, norm)
    assert rc == 0 and ctx.value, (k, err())
    L.aclgan_ctx_destroy(ctx)
'''
    got = _child(code, tmp_path, {"bad": bad, "good": good})
    assert sorted(got) == sorted(bad)
    for k, (rc, msg, made) in got.items():
        assert rc == -1 and msg and not made, (k, rc, msg)
    for k, word in (("gen.dim 12", "gen.dim"), ("gen.dim 3", "gen.dim"), ("dis.dim 6", "dis.dim"), ("dis.dim 2", "dis.dim"),
                    ("dis.n_layer 0", "layer counts"), ("gen.style_dim 0", "mlp/style"), ("sn 17 layers", "spectral norm"),
                    ("sn 3 x 6 layers", "spectral norm")):
        assert word in got[k][1], (k, got[k][1])


def test_every_architecture_sizes_in_every_dtype_and_lane_count(tmp_path):
    code = r'''
prev = C.c_int()
for name, c in cases.items():
    B, H, W = c["shape"]
    for dtype in (0, 1, 2):
        ctx = bound(c["gen"], c["dis"], dtype)
        for lanes in (1, 3):
            assert L.aclgan_tuning(b"lanes", lanes, C.byref(prev)) == 0
            rc, ws = ws_bytes(ctx, B, H, W)
            assert rc == 0 and ws > 0, (name, dtype, lanes, err())
            fw = C.c_size_t()
            assert L.aclgan_forward_workspace_bytes(ctx, B, H, W, C.byref(fw)) == 0 and 0 < fw.value <= ws, (name, dtype, lanes, err())
            rec = {"ws": ws, "fw": fw.value}
            for which in (0, 1):
                v = C.c_double()
                assert L.aclgan_step_executed_flops(ctx, which, B, H, W, C.byref(v)) == 0 and v.value > 0, (name, dtype, lanes, which, err())
                rec["flops%d" % which] = v.value
                assert L.aclgan_step_algorithmic_bytes(ctx, which, B, H, W, C.byref(v)) == 0 and v.value > 0, (name, dtype, lanes, which, err())
                rec["bytes%d" % which] = v.value
            assert L.aclgan_set_grad_buckets(ctx, C.c_int64(1 << 12), None, None) == 0, err()
            order = (C.c_int * 65536)(); cnt = C.c_int()
            for grp in (0, 1):
                assert L.aclgan_bucket_schedule(ctx, grp, B, H, W, 0, order, 65536, C.byref(cnt)) == 0, (name, dtype, lanes, grp, err())
                n = L.aclgan_group_numel(ctx, grp)
                want = (n + (1 << 12) - 1) >> 12
                assert sorted(order[:cnt.value]) == list(range(want)), (name, dtype, lanes, grp, cnt.value, want)
            assert L.aclgan_set_grad_buckets(ctx, C.c_int64(0), None, None) == 0
            # exactly the reported bytes pass, one byte less is refused -- before anything is enqueued
            assert L.aclgan_bind_workspace(ctx, C.c_void_p(0x100000), C.c_size_t(ws)) == 0
            assert L.aclgan_check_workspace(ctx, B, H, W) == 0, (name, dtype, lanes, err())
            assert L.aclgan_bind_workspace(ctx, C.c_void_p(0x100000), C.c_size_t(ws - 1)) == 0
            assert L.aclgan_check_workspace(ctx, B, H, W) == ENOMEM and "too small" in err(), (name, dtype, lanes, err())
            out["%s/%d/%d" % (name, dtype, lanes)] = rec
        L.aclgan_ctx_destroy(ctx)
'''
    got = _child(code, tmp_path, _cases())
    assert len(got) == len(A.ARCHS) * 3 * 2
    for name in A.ARCHS:
        f32 = got["%s/0/3" % name]
        assert 16 << 20 < f32["ws"] < 4 << 30, (name, f32["ws"])      # 29 MiB (the 8-wide ones) .. 3.3 GiB (gen128)
        for dt in (1, 2):      # 16-bit storage moves fewer bytes than fp32, never more
            assert got["%s/%d/3" % (name, dt)]["bytes0"] <= f32["bytes0"] and got["%s/%d/3" % (name, dt)]["bytes1"] <= f32["bytes1"], name


def test_flat_parameter_layout_is_the_oracle_s(tmp_path):
    code = r'''
for name, c in cases.items():
    rc, ctx = create(c["gen"], c["dis"])
    assert rc == 0, err()
    nm = C.create_string_buffer(256); off = C.c_int64(); shp = (C.c_int * 4)(); nd = C.c_int()
    out[name] = []
    for grp in (0, 1):
        rows = []
        for i in range(L.aclgan_tensor_count(ctx, grp)):
            assert L.aclgan_tensor_info(ctx, grp, i, nm, 256, C.byref(off), shp, C.byref(nd)) == 0, err()
            rows.append([nm.value.decode(), [shp[j] for j in range(nd.value)], off.value])
        out[name].append(rows)
    L.aclgan_ctx_destroy(ctx)
'''
    got = _child(code, tmp_path, _cases())
    for name in A.ARCHS:
        cfg = A.arch_config(name)
        gs = O.gen_param_shapes(3, cfg["gen"])
        want_gen = [("%s/%s" % (n, k), list(s)) for n in ("gen_AB", "gen_BA") for k, s in gs.items()]
        want_dis = [("%s/%s" % (n, k), list(s)) for n, ci in (("dis_A", 3), ("dis_B", 3), ("dis_2", 6))
                    for k, s in O.dis_param_shapes(ci, cfg["dis"]).items()]
        for rows, want in zip(got[name], (want_gen, want_dis)):
            assert [(r[0], r[1]) for r in rows] == want, name
            end = 0
            for _, shape, off in rows:      # disjoint, in order
                assert off >= end and off % 4 == 0, (name, off, end)
                numel = 1
                for s in shape:
                    numel *= s
                end = off + numel


def test_too_small_an_image_is_refused_by_the_key_that_needs_more(tmp_path):
    """A 4x4 stride-2 layer reflect-pads a map of 2 at least and halves it, the pyramid halves with ceil: scale s needs ceil(H / 2^s) >=
    2^n_layer, i.e. H >= (2^n_layer - 1) 2^(num_scales-1) + 1; the ResBlocks need H >= 2^(n_downsample+1).  Refused in the dry run, with the
    key and the minimum in the message; the same context then sizes a valid shape.  The 64 minimum of the default architecture stays."""
    g, d = [8, 16, 8, 2, 1], [8, 4, 3]
    rows = {
        "n_layer 5 at 64x64": (g, [8, 5, 3], (2, 64, 64), (2, 128, 128)),
        "n_layer 5 at 64x96": (g, [8, 5, 3], (2, 64, 96), (2, 128, 128)),
        "n_layer 5 at 124x128": (g, [8, 5, 3], (1, 124, 128), (1, 128, 128)),      # minimum 31 * 4 + 1 = 125 (and a multiple of 4: 128)
        "num_scales 4 at 64x64": (g, [8, 4, 4], (2, 64, 64), (2, 128, 128)),
        "num_scales 4 at 96x120": (g, [8, 4, 4], (2, 96, 120), (2, 124, 124)),      # minimum 15 * 8 + 1 = 121
        "n_downsample 6 at 64x64": ([8, 16, 8, 6, 1], d, (2, 64, 64), (1, 128, 128)),
        "H = 68 with n_downsample 3": ([8, 20, 5, 3, 2], d, (2, 68, 64), (2, 64, 72)),
        "default at 60x64": (g, d, (2, 60, 64), (2, 64, 64)),
        "default at 64x62": (g, d, (2, 64, 62), (2, 64, 64)),
    }
    code = r'''
for k, (g, d, bad, good) in cases.items():
    ctx = bound(g, d)
    rc, ws = ws_bytes(ctx, *bad)
    msg = err()
    v = C.c_double()
    rc2 = [L.aclgan_step_algorithmic_bytes(ctx, which, bad[0], bad[1], bad[2], C.byref(v)) for which in (0, 1)]
    assert L.aclgan_bind_workspace(ctx, C.c_void_p(0x100000), C.c_size_t(1 << 40)) == 0
    rc3 = L.aclgan_check_workspace(ctx, *bad)
    assert L.aclgan_launch_count() == 0
    rcg, wsg = ws_bytes(ctx, *good)
    assert rcg == 0 and wsg > 0, (k, err())
    assert L.aclgan_check_workspace(ctx, *good) == 0, (k, err())
    out[k] = [rc, msg, rc2, rc3]
    L.aclgan_ctx_destroy(ctx)
# forward-only encode does not need the size to round-trip through the decoder
ctx = bound([8, 20, 5, 3, 2], [8, 4, 3])
fw = C.c_size_t()
assert L.aclgan_forward_workspace_bytes(ctx, 2, 68, 64, C.byref(fw)) == 0 and fw.value > 0, err()
L.aclgan_ctx_destroy(ctx)
'''
    got = _child(code, tmp_path, rows)
    for k, (rc, msg, rc2, rc3) in got.items():
        assert rc == -1 and rc2 == [-1, -1] and rc3 == -1, (k, rc, rc2, rc3, msg)
    for k, words in (("n_layer 5 at 64x64", ("dis.n_layer 5", "H,W>=125")), ("n_layer 5 at 64x96", ("dis.n_layer 5", "H,W>=125")),
                     ("n_layer 5 at 124x128", ("dis.n_layer 5", "H,W>=125")),
                     ("num_scales 4 at 64x64", ("dis.num_scales 4", "H,W>=121")), ("num_scales 4 at 96x120", ("dis.num_scales 4", "H,W>=121")),
                     ("n_downsample 6 at 64x64", ("gen.n_downsample 6", "H,W>=128")),
                     ("H = 68 with n_downsample 3", ("multiples of 8",)),
                     ("default at 60x64", ("H,W>=64",)), ("default at 64x62", ("H,W>=64",))):
        for w in words:
            assert w in got[k][1], (k, got[k][1])
        assert "reflect pad 1 >= input size" not in got[k][1], (k, got[k][1])      # (not whichever convolution first trips)
