"""CPU model of csrc/guided.hip (include/aclgan_hip.h: aclgan_translate_guided_coef, aclgan_translate_guided_paste_u8) in numpy: ONE array
operation per rounded operation of the rule, evaluated in fp32 (what the kernels are held to bit for bit and byte for byte in
tests/test_gpu_guided.py) or, with dt=np.float64, the same rule in fp64 (tests/test_guided_cpu.py bounds the difference of the two).
The sampling rule, the residual and the cases are those of tests/paste_ref.py.  scene() / quality_case(): the pictures of the quality test."""
import numpy as np

from paste_ref import SHAPES, _bilinear, axis, case, residual  # noqa: F401  (SHAPES and case: re-exported for the tests)


def _taps_inside(n, radius):
    i = np.arange(n)
    return np.minimum(i + radius, n - 1) - np.maximum(i - radius, 0) + 1


def _running(v, radius, ax):
    """((0 + v[k - radius]) + v[k - radius + 1]) + ... + v[k + radius] along axis `ax`, ascending; taps outside the plane are left out"""
    v = np.moveaxis(v, ax, -1)
    n = v.shape[-1]
    acc = np.zeros_like(v)
    for k in range(-radius, radius + 1):
        lo, hi = max(0, -k), min(n, n - k)                 # the outputs whose tap k lies inside
        if lo < hi:
            acc[..., lo:hi] = acc[..., lo:hi] + v[..., lo + k:hi + k]
    return np.moveaxis(acc, -1, ax)


def box_mean(v, radius):
    """v (..., oh, ow): the row sums h in ascending j, their column sums s in ascending i, s / fp(ny * nx)"""
    oh, ow = v.shape[-2:]
    h = _running(v, radius, -1)
    s = _running(h, radius, -2)
    n = (_taps_inside(oh, radius)[:, None] * _taps_inside(ow, radius)[None, :]).astype(v.dtype)
    return s / n


def coefficients(dec, x, valid, radius, eps, dt=np.float32):
    """steps 1-4: dec (3 or 4, PH, PW), x (3, PH, PW) -> A (3, oh, ow), Bq (3, oh, ow), m (oh, ow)"""
    oh, ow = valid
    r, m = residual(dec, x, valid, dt)
    xs = np.asarray(x, np.float32)[:, :oh, :ow].astype(dt)
    s = xs + dt(1)
    g = s * dt(0.5)
    gg = g * g
    gr = g * r
    Mg, Mr, Mgg, Mgr = box_mean(g, radius), box_mean(r, radius), box_mean(gg, radius), box_mean(gr, radius)
    sq = Mg * Mg
    d = Mgg - sq
    var = np.maximum(d, dt(0))
    pr = Mg * Mr
    cov = Mgr - pr
    den = var + dt(eps)
    a = cov / den
    t = a * Mg
    b = Mr - t
    return box_mean(a, radius), box_mean(b, radius), m


def planes(dec, x, valid, radius, eps, dt=np.float32):
    """the coefficient planes as aclgan_translate_guided_coef lays them out: (7, oh, ow) = A_0..2, Bq_0..2, m -- (6, oh, ow) without a focus plane"""
    A, Bq, m = coefficients(dec, x, valid, radius, eps, dt)
    return np.concatenate([A, Bq] + ([m[None]] if np.asarray(dec).shape[0] == 4 else []))


def guided(dec, x, valid, source, radius=4, eps=1e-3, dt=np.float32):
    """One image.  source (Hs, Ws, 3) uint8 -> (bar, mask), each (Hs, Ws, 3) uint8"""
    source = np.asarray(source, np.uint8)
    Hs, Ws = source.shape[:2]
    A, Bq, m = coefficients(dec, x, valid, radius, eps, dt)
    yy, xx = axis(valid[0], Hs, dt), axis(valid[1], Ws, dt)
    Au = _bilinear(A, yy, xx)                              # (3, Hs, Ws)
    Bu = _bilinear(Bq, yy, xx)
    byte = source.transpose(2, 0, 1).astype(dt)
    G = byte * dt(1 / 255)
    E = Au * G
    E = E + Bu
    t = E * dt(255)
    v = byte + t
    v = v + dt(0.5)
    bar = np.clip(v, dt(0), dt(255)).astype(np.uint8).transpose(1, 2, 0)
    M = _bilinear(m, yy, xx)
    t = M * dt(255)
    v = t + dt(0.5)
    mask = np.clip(v, dt(0), dt(255)).astype(np.uint8)
    return np.ascontiguousarray(bar), np.ascontiguousarray(np.repeat(mask[:, :, None], 3, 2))


# ---- the pictures of the quality test ----
ALPHA = np.array([0.6, 0.8, 0.5])
BETA = np.array([0.25, 0.05, 0.3])


def scene(Hs, Ws, seed, noise=3):
    """a deterministic piecewise-constant picture (Hs, Ws, 3) uint8: rectangles of flat colour over a flat ground, plus `noise` levels of
    uniform noise either way -- edges and texture above the net's resolution"""
    rng = np.random.RandomState(7000 + seed)
    img = np.empty((Hs, Ws, 3), np.float64)
    img[:] = rng.randint(40, 216, 3)
    for _ in range(12):
        y0, x0 = rng.randint(0, Hs), rng.randint(0, Ws)
        h, w = rng.randint(Hs // 8 + 1, Hs // 2 + 2), rng.randint(Ws // 8 + 1, Ws // 2 + 2)
        img[y0:y0 + h, x0:x0 + w] = rng.randint(20, 236, 3)
    img += rng.randint(-noise, noise + 1, (Hs, Ws, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def quality_case(valid, factor, seed):
    """an affine edit under an open mask: the source is `factor` times the net region, x its block mean, fg = ALPHA_c x + BETA_c in [0, 1]
    units, f = 1.  Returns (dec (4, oh, ow), x (3, oh, ow), source, target): target = clip(ALPHA source + 255 BETA), the edit at full size"""
    oh, ow = valid
    source = scene(oh * factor, ow * factor, seed)
    x01 = source.reshape(oh, factor, ow, factor, 3).mean((1, 3)).transpose(2, 0, 1) / 255.0
    fg01 = ALPHA[:, None, None] * x01 + BETA[:, None, None]
    dec = np.concatenate([fg01 * 2 - 1, np.ones((1, oh, ow))]).astype(np.float32)
    x = (x01 * 2 - 1).astype(np.float32)
    target = np.clip(ALPHA * source.astype(np.float64) + 255 * BETA, 0, 255)
    return dec, x, source, target
