#!/usr/bin/env python3
"""Record what the Adam launches compute, bit for bit, as sha256 digests: tests/golden/adam_bits_parent.json.

Run on the MI355X AT THE COMMIT WHOSE RESULTS ARE TO BE KEPT (the parent of a change to csrc/optimizer.hip), with the library built:
    python tests/golden/make_adam_bits.py [--out FILE]
tests/test_gpu_adam_bits.py replays the same cases (run_flat / run_small / run_full below) and compares the digests.  The kernels and
csrc/gradnorm.hip use no atomics: two runs write the same file.

Everything goes through the C ABI.  Inputs come from numpy.random.RandomState(seed): host-generated, the same at every commit; magnitudes
2^e (1 + u) with e spread over +-20 binades, random signs.  One digest per call (digest() below: the sha256 of the sha256 of each
tensor's bytes), over -- in this order -- p, m, v of the updated buffer, the average where bound, the eight loss-scale floats and the
clip state where bound, then the buffers of the group the call does not update (p, g, m, v; run_small and run_full), which must not
move.

  flat/...   aclgan_adam_flat, aclgan_adam_flat_ema (copy and blend): n = 1, 255, 257, 1000 x step = 1, 2, 1000
  small/...  a context of the reduced architecture (226 536 / 393 372 floats, both ragged against 256): {no loss scale, loss scale} x
             {no clip, clip with a finite max_norm (coefficient < 1), clip with max_norm = +inf} x {no average, blend, copy}; five calls
             per group (the average belongs to the generator group; variants with one update that group only).  Call 3 carries an event
             that skips the update -- under a loss scale one +inf gradient element, with a clip state alone finite gradients whose norm
             is not finite -- so that calls 4 and 5 take the bias correction of step - skipped on the device.  Asserted: the skip
             counter went up.
  full/...   the default architecture: the generator group (30 058 648 floats: eight trips of the 16384 x 256 grid-stride loop, the
             last one ragged) under loss scale + clip + blend, two calls; the discriminator group plain, two calls."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for d in (ROOT, os.path.dirname(HERE)):
    if d not in sys.path:
        sys.path.insert(0, d)
from test_gpu_optimizer import B1, B2, EPS, FULL, LR0, SMALL, WD, _Ctx  # noqa: E402

FIXTURE = os.path.join(HERE, "adam_bits_parent.json")
INF = float("inf")
S0 = 65536.0
FLAT_SIZES, FLAT_STEPS = (1, 255, 257, 1000), (1, 2, 1000)
SCALES, CLIPS, EMAS = ("noscale", "scale"), ("noclip", "clipfinite", "clipinf"), ("noema", "blend", "copy")
DECAY = 0.999


def values(rs, n, nonneg=False):
    """fp32 values 2^e (1 + u), e over [-20, 20), random signs (or none), put together from one draw of 32 random bits per element:
    sign | exponent field 107 + (8 bits scaled to 0 .. 39) | 23 mantissa bits"""
    bits = rs.randint(0, 2 ** 32, n, dtype=np.uint32)
    expo = ((((bits >> np.uint32(23)) & np.uint32(0xFF)) * np.uint32(40)) >> np.uint32(8)) + np.uint32(107)
    sign = np.uint32(0) if nonneg else bits & np.uint32(0x80000000)
    return torch.from_numpy((sign | (expo << np.uint32(23)) | (bits & np.uint32(0x7FFFFF))).view(np.float32))


def digest(*tensors):
    """sha256 over the tensors' own sha256 digests, in order (one thread per tensor: hashlib releases the GIL)"""
    arrays = [t.detach().cpu().contiguous().numpy() for t in tensors]
    with ThreadPoolExecutor(8) as pool:
        parts = list(pool.map(lambda a: hashlib.sha256(a.data).hexdigest(), arrays))
    return hashlib.sha256("".join(parts).encode()).hexdigest()


def run_flat(L):
    out = {}
    adam = L.Adam(LR0, B1, B2, EPS, WD)
    for n in FLAT_SIZES:
        rs = np.random.RandomState(1000 + n)
        p0, g, m0, v0, e0 = values(rs, n), values(rs, n), values(rs, n), values(rs, n, nonneg=True), values(rs, n)
        for step in FLAT_STEPS:
            for entry in ("plain", "copy", "blend"):
                p, gd, m, v, ema = (t.cuda() for t in (p0, g, m0, v0, e0))
                if entry == "plain":
                    L.check(L.lib.aclgan_adam_flat(L.ptr(p), L.ptr(gd), L.ptr(m), L.ptr(v), n, C.byref(adam), step, L.stream_ptr()), "adam_flat")
                else:
                    mode = L.EMA_COPY if entry == "copy" else L.EMA_BLEND
                    L.check(L.lib.aclgan_adam_flat_ema(L.ptr(p), L.ptr(gd), L.ptr(m), L.ptr(v), L.ptr(ema), n, C.byref(adam), step, DECAY, mode,
                                                       L.stream_ptr()), "adam_flat_ema")
                torch.cuda.synchronize()
                assert torch.equal(gd.cpu(), g)
                out["flat/%s/n%d/step%d" % (entry, n, step)] = [digest(p, m, v, *([] if entry == "plain" else [ema]))]
    return out


class _BitsCtx(_Ctx):
    """_Ctx with the clip states and the average of tests/test_gpu_gradclip.py's and tests/test_gpu_ema.py's binding calls"""

    def __init__(self, L, arch):
        super().__init__(L, arch)
        self.clip, self.ema = [None, None], None

    def bind_clip(self, grp, max_norm):
        L = self.L
        self.clip[grp] = torch.zeros(L.lib.aclgan_grad_clip_state_floats(), device="cuda")
        L.check(L.lib.aclgan_bind_grad_clip(self.ctx, grp, max_norm, L.ptr(self.clip[grp])), "bind_grad_clip")

    def bind_ema(self, ema):
        L = self.L
        self.ema = ema.cuda()
        L.check(L.lib.aclgan_bind_ema(self.ctx, L.GROUP_GEN, L.ptr(self.ema)), "bind_ema")

    def step(self, grp, step, mode=None):
        L = self.L
        adam = L.Adam(LR0, B1, B2, EPS, WD)
        if mode is None:
            L.check(L.lib.aclgan_adam_step(self.ctx, grp, C.byref(adam), step, L.stream_ptr()), "adam_step")
        else:
            L.check(L.lib.aclgan_adam_step_ema(self.ctx, grp, C.byref(adam), step, DECAY, mode, L.stream_ptr()), "adam_step_ema")
        torch.cuda.synchronize()

    def other_buffers(self, grp):
        return [buf[1 - grp] for buf in (self.p, self.g, self.m, self.v)]

    def call_digest(self, grp):
        own = [self.p[grp], self.m[grp], self.v[grp]] + [t for t in (self.ema if grp == 0 else None, self.state, self.clip[grp]) if t is not None]
        return digest(*(own + self.other_buffers(grp)))

    def close(self):
        torch.cuda.synchronize()
        self.L.lib.aclgan_ctx_destroy(self.ctx)


def _sequence(L, arch, seed, scale, clip, ema, groups, calls, event_call):
    """`calls` updates of each group of `groups`, interleaved; one digest per call"""
    c = _BitsCtx(L, arch)
    try:
        # one host draw per sequence; every buffer is a rotation of it (exact, on the device): 30 M values take the host half a second each
        base = values(np.random.RandomState(seed), max(c.n)).cuda()

        def take(k, n):
            return torch.roll(base, 1009 * k)[:n]
        for grp in (0, 1):
            c.p[grp].copy_(take(1 + grp, c.n[grp]))
            c.g[grp].copy_(take(3 + grp, c.n[grp]))      # (the group a call does not update keeps what it holds)
        if scale == "scale":
            c.bind_state([S0, 1.0 / S0, 0, 0, 0, 0, 2, 0])      # growth interval 2: the scale moves during the sequence
        max_norm = {"noclip": None, "clipfinite": 1.0, "clipinf": INF}[clip]
        if max_norm is not None:
            for grp in groups:
                c.bind_clip(grp, max_norm)
        if ema != "noema":
            c.bind_ema(take(5, c.n[0]).clone())
        mode = {"noema": None, "blend": L.EMA_BLEND, "copy": L.EMA_COPY}[ema]
        out = {g_: [] for g_ in groups}
        for call in range(1, calls + 1):
            for grp in groups:
                g = take(10 + 2 * call + grp, c.n[grp]) * (S0 if scale == "scale" else 1.0)
                skips = call == event_call and (scale == "scale" or max_norm is not None)
                if skips:
                    g[c.n[grp] // 3] = INF if scale == "scale" else 3e38
                c.g[grp].copy_(g)
                keep = [t.clone() for t in c.other_buffers(grp)]
                c.step(grp, call, mode if grp == 0 else None)
                assert all(torch.equal(a, b) for a, b in zip(c.other_buffers(grp), keep)), "the other group's buffers moved"
                skipped = float(event_call is not None and call >= event_call)      # what the skip counter must show
                if scale == "scale":
                    assert c.state_list()[4 + grp] == skipped, (call, c.state_list())
                elif max_norm is not None:
                    coef, _, count = c.clip[grp][1:4].cpu().tolist()
                    assert count == skipped, (call, count)
                    assert coef == 0.0 if skips else (coef < 1.0) == (clip == "clipfinite"), (call, coef)
                out[grp].append(c.call_digest(grp))
        return out
    finally:
        c.close()


def run_small(L):
    out = {}
    for i, scale in enumerate(SCALES):
        for j, clip in enumerate(CLIPS):
            for k, ema in enumerate(EMAS):
                groups = (0, 1) if ema == "noema" else (0,)
                r = _sequence(L, SMALL, 2000 + 100 * i + 10 * j + k, scale, clip, ema, groups, calls=5, event_call=3)
                for grp in groups:
                    out["small/%s+%s+%s/%s" % (scale, clip, ema, ("gen", "dis")[grp])] = r[grp]
    return out


def run_full(L):
    out = {}
    r = _sequence(L, FULL, 3000, "scale", "clipfinite", "blend", (0,), calls=2, event_call=None)
    out["full/scale+clipfinite+blend/gen"] = r[0]
    r = _sequence(L, FULL, 3001, "noscale", "noclip", "noema", (1,), calls=2, event_call=None)
    out["full/noscale+noclip+noema/dis"] = r[1]
    return out


def load_lib():
    assert torch.cuda.is_available(), "needs the MI355X"
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib
    return _lib


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    L = load_lib()
    cases = {}
    for run in (run_flat, run_small, run_full):
        cases.update(run(L))
    with open(args.out, "w") as f:
        json.dump(cases, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%s: %d cases, %d digests -> %s" % (L.LIB_PATH, len(cases), sum(len(v) for v in cases.values()), args.out))
