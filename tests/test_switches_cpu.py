"""CPU-only checks of the switch table (acl-gan_amd/csrc/switches.hip): every switch's default, how its environment variable is parsed,
the twelve run-time settable keys of aclgan_tuning, and that the table, the sources and DESIGN.md section 6 list the same variables.
Each check loads libaclgan_hip.so in a fresh child process with its own environment (a switch is latched on its first read)."""
import json
import os
import re
import subprocess
import sys

from conftest import ROOT

LIB = os.path.join(ROOT, "acl-gan_amd", "libaclgan_hip.so")
CSRC = os.path.join(ROOT, "acl-gan_amd", "csrc")

# key -> (environment variable or None, default)
SWITCHES = {
    "lanes": ("ACLGAN_LANES", 3), "u_batch": ("ACLGAN_U_BATCH", 1), "norm_mask": ("ACLGAN_NORM_MASK", 1),
    "mlp_fused": ("ACLGAN_MLP_FUSED", 1), "fault_at": (None, -1), "glds_tile": ("ACLGAN_GLDS_TILE", 0), "wino_x3": ("ACLGAN_WINO_X3", 0),
    "wino_fused": ("ACLGAN_WINO_FUSED", 1), "wino_wgrad_fused": ("ACLGAN_WINO_WGRAD_FUSED", 1), "wino_s2k4": ("ACLGAN_NOWINOS2", 1),
    "dgrad16s_direct": ("ACLGAN_DGRAD16S_DIRECT", 0), "fwd16_patch": ("ACLGAN_FWD16_PATCH", 1),
    "deterministic": ("ACLGAN_DETERMINISTIC", 0), "nofast": ("ACLGAN_NOFAST", 0), "noup5": ("ACLGAN_NOUP5", 0),
    "split_nwg": ("ACLGAN_SPLIT_NWG", 256), "nowgkc": ("ACLGAN_NOWGKC", 0), "noup5dgrad": ("ACLGAN_NOUP5DGRAD", 0),
    "nostatfuse": ("ACLGAN_NOSTATFUSE", 0), "nokeepv": ("ACLGAN_NOKEEPV", 0), "nodirect": ("ACLGAN_NODIRECT", 0),
    "nowgrad16s": ("ACLGAN_NOWGRAD16S", 0), "wgrad16s_minpix": ("ACLGAN_WGRAD16S_MINPIX", 64),
    "noglds16": ("ACLGAN_NOGLDS16", 0), "nosmall": ("ACLGAN_NOSMALL", 0), "nothin": ("ACLGAN_NOTHIN", 0),
    "nowino": ("ACLGAN_NOWINO", 0), "nowinoup5": ("ACLGAN_NOWINOUP5", 0), "wino_vec": ("ACLGAN_WINO_VEC", 2),
    "wino_vec3": ("ACLGAN_WINO_VEC3", 2), "roctx": ("ACLGAN_ROCTX", 0), "noucache": ("ACLGAN_NOUCACHE", 0), "act16": ("ACLGAN_ACT16", 1),
    "co16": ("ACLGAN_CO16", 1), "side_stream": ("ACLGAN_SIDE_STREAM", 1), "keepv_budget_gb": ("ACLGAN_KEEPV_BUDGET_GB", 64),
}
SETTABLE = ["lanes", "u_batch", "norm_mask", "mlp_fused", "fault_at", "glds_tile", "wino_x3", "wino_fused", "wino_wgrad_fused", "wino_s2k4",
            "dgrad16s_direct", "fwd16_patch"]
# retired experiments: no longer keys of the library
RETIRED = ["mergedhalo", "up5_bandfold", "gemm_var", "glds_spec", "glds_nbuf", "bigtile", "tile16", "halo_tile", "halo_split", "side_prio",
           "lane_prio", "capture_lanes", "nosingletap", "thinin2", "prefill_lane"]

_BOOL = [("1", 1), ("3", 1), ("0", 0), ("", 0)]              # nonzero -> 1 (atoi: "" is 0)
_ON_UNLESS_0 = [("0", 0), ("", 0), ("2", 1)]                 # default 1, off when the variable reads as 0
_MODE = [("0", 0), ("2", 2), ("19", 1), ("18", 18), ("-1", 1), ("3", 1)]      # low four bits 0..2 (bits 4..: ablation builds), else 1
# key -> [(variable text, value read back)], from the library's parsing of each variable
PARSE = {
    "lanes": [("2", 2), ("0", 1), ("7", 3), ("", 3)],
    "u_batch": [("0", 0), ("5", 1), ("", 1)], "norm_mask": [("0", 0), ("5", 1), ("", 1)], "mlp_fused": [("0", 0), ("5", 1), ("", 1)],
    "glds_tile": [("3", 3), ("9", 9), ("-5", 0)],
    "wino_x3": _BOOL, "wino_fused": _MODE, "fwd16_patch": _MODE,
    "wino_wgrad_fused": [("0", 0), ("2", 2), ("3", 1), ("-1", 1)],
    "wino_s2k4": [("1", 0), ("5", 0), ("0", 1)],
    "dgrad16s_direct": _BOOL, "deterministic": _BOOL, "nofast": _BOOL, "noup5": _BOOL,
    "split_nwg": [("128", 128), ("", 0)],
    "nowgkc": _BOOL, "noup5dgrad": _BOOL,
    "nostatfuse": _BOOL, "nokeepv": _BOOL, "nodirect": _BOOL,
    "nowgrad16s": _BOOL, "wgrad16s_minpix": [("100000", 100000), ("", 0)], "noglds16": _BOOL,
    "nosmall": _BOOL, "nothin": _BOOL,
    "nowino": _BOOL, "nowinoup5": _BOOL,
    "wino_vec": [("1", 1), ("4", 4), ("3", 2), ("8", 2), ("-2", 2)], "wino_vec3": [("1", 1), ("4", 4), ("3", 2), ("0", 2)],
    "roctx": _BOOL,
    "noucache": _BOOL, "act16": _ON_UNLESS_0, "co16": _ON_UNLESS_0, "side_stream": _ON_UNLESS_0,
    "keepv_budget_gb": [("128", 128), ("2.9", 2), ("0.5", 0)],      # (read back truncated; the engine uses the real value)
}
# key -> [(value given to aclgan_tuning, value read back)]
SET = {
    "lanes": [(0, 1), (2, 2), (9, 3)], "u_batch": [(0, 0), (5, 1)], "norm_mask": [(0, 0), (5, 1)], "mlp_fused": [(0, 0), (5, 1)],
    "fault_at": [(7, 7), (-1, -1)], "glds_tile": [(3, 3), (-2, 0)], "wino_x3": [(1, 1), (0, 0)],
    "wino_fused": [(2, 2), (19, 1), (18, 18), (-1, 1)], "wino_wgrad_fused": [(2, 2), (3, 1), (0, 0)],
    "wino_s2k4": [(0, 0), (5, 1)], "dgrad16s_direct": [(4, 1), (0, 0)], "fwd16_patch": [(2, 2), (3, 1), (0, 0)],
}

CHILD = r'''
import ctypes as C, json, os, sys
L = C.CDLL(sys.argv[1])
L.aclgan_last_error.restype = C.c_char_p
def get(key):
    v = C.c_longlong(12345)
    rc = L.aclgan_tuning_get(key.encode(), C.byref(v))
    return v.value if rc == 0 else None
def tune(key, value):
    prev = C.c_int(12345)
    rc = L.aclgan_tuning(key.encode(), value, C.byref(prev))
    return rc, prev.value, L.aclgan_last_error().decode()
out = {}
exec(sys.argv[2])
print(json.dumps(out))
'''


def _child(code, env=None):
    e = {k: v for k, v in os.environ.items() if not k.startswith("ACLGAN_")}
    e.update(env or {})
    p = subprocess.run([sys.executable, "-c", CHILD, LIB, code], env=e, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_defaults_without_environment():
    got = _child("out.update({k: get(k) for k in %r})" % sorted(SWITCHES))
    assert got == {k: d for k, (_, d) in SWITCHES.items()}


def test_environment_parsing():
    assert set(PARSE) == {k for k, (var, _) in SWITCHES.items() if var}
    for i in range(max(len(c) for c in PARSE.values())):
        env = {SWITCHES[k][0]: c[i][0] for k, c in PARSE.items() if i < len(c)}
        want = {k: c[i][1] for k, c in PARSE.items() if i < len(c)}
        got = _child("out.update({k: get(k) for k in %r})" % sorted(want), env)
        assert got == want, (env, {k: (got[k], want[k]) for k in want if got[k] != want[k]})


def test_latched_on_first_read():
    """a variable set before a switch's first read is seen (os.environ after the library is loaded); later changes are not"""
    got = _child("os.environ['ACLGAN_NOWINO'] = '1'; out['a'] = get('nowino'); os.environ['ACLGAN_NOWINO'] = '0'; out['b'] = get('nowino')")
    assert got == {"a": 1, "b": 1}


def test_setters_epoch_and_read_only_keys():
    code = r'''
ep = lambda: get("epoch")
for key, cases in %r.items():
    for value, want in cases:
        e0, old = ep(), get(key)
        rc, prev, _ = tune(key, value)
        assert rc == 0 and prev == old, (key, value, rc, prev, old)
        assert get(key) == want and get(key) == want, (key, value, get(key), want)
        assert ep() == e0 + 1, (key, value, e0, ep())
    assert L.aclgan_set_tuning(key.encode(), cases[0][0]) == cases[-1][1] and get(key) == cases[0][1]
for key in %r:
    e0, old = ep(), get(key)
    rc, prev, err = tune(key, 1 - old)
    assert rc == -1 and prev == 12345 and "read-only" in err and get(key) == old and ep() == e0, (key, rc, prev, err)
    assert L.aclgan_set_tuning(key.encode(), 1) == -1 and get(key) == old and ep() == e0
e0 = ep()
rc, prev, err = tune("no such key", 1)
assert rc == -1 and prev == 12345 and "unknown key" in err and ep() == e0
assert get("no such key") is None
for key in %r:      # a retired experiment is an unknown key: a script that still sets it fails instead of measuring the default
    e0 = ep()
    rc, prev, err = tune(key, 1)
    assert rc == -1 and prev == 12345 and "unknown key '" + key + "'" in err and ep() == e0, (key, rc, prev, err)
    assert get(key) is None and "unknown key '" + key + "'" in L.aclgan_last_error().decode(), key
assert L.aclgan_set_deterministic(1) == 0 and get("deterministic") == 1 and L.aclgan_get_deterministic() == 1
assert L.aclgan_set_deterministic(0) == 0 and get("deterministic") == 0 and L.aclgan_get_deterministic() == 0 and ep() == e0
out["ok"] = 1
''' % (SET, sorted(set(SWITCHES) - set(SETTABLE)), RETIRED)
    assert sorted(SET) == sorted(SETTABLE)
    assert _child(code) == {"ok": 1}


def test_getenv_only_in_the_switch_table():
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h")) and name != "switches.hip":
            src = open(os.path.join(CSRC, name)).read()
            assert "getenv" not in src, name


def test_design_table_lists_every_variable_of_the_switch_table():
    table = set(re.findall(r'"(ACLGAN_[A-Z0-9_]+)"', open(os.path.join(CSRC, "switches.hip")).read()))
    assert table == {var for var, _ in SWITCHES.values() if var}
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"\n\| key \| variable \|.*?\n\n", design, re.S)
    assert m, "DESIGN.md: switch table not found"
    rows = re.findall(r"^\| `([a-z0-9_]+)` \| (?:`(ACLGAN_[A-Z0-9_]+)`|--) \|", m.group(0), re.M)
    assert sorted(k for k, _ in rows) == sorted(SWITCHES)
    assert {v for _, v in rows if v} == table
