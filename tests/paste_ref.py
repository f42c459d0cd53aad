"""CPU model of csrc/paste.hip (include/aclgan_hip.h: aclgan_translate_pad, aclgan_translate_paste_u8) in numpy: ONE array operation per
rounded operation of the rule, evaluated in fp32 (what the kernels are held to byte for byte in tests/test_gpu_paste.py) or, with
dt=np.float64, the same rule in fp64 (tests/test_paste_cpu.py bounds the difference of the two)."""
import numpy as np


def padded_shape(shape, multiple):
    return tuple(-(-n // multiple) * multiple for n in shape)


def reflect_index(n, padded):
    """source index of every padded position: i < n is i, i >= n is 2 (n - 1) - i"""
    i = np.arange(padded)
    return np.where(i < n, i, 2 * (n - 1) - i)


def reflect_pad(x, multiple):
    """x (..., oh, ow) -> (..., PH, PW): rows added at the bottom, columns at the right, by reflection without the edge; values copied"""
    oh, ow = x.shape[-2:]
    PH, PW = padded_shape((oh, ow), multiple)
    assert oh >= multiple and ow >= multiple
    return np.ascontiguousarray(x[..., reflect_index(oh, PH), :][..., reflect_index(ow, PW)])


def axis(n_in, n_out, dt=np.float32):
    """(i0, i1, w) of every output index of one axis"""
    scale = np.asarray(n_in, dt) / np.asarray(n_out, dt)
    c = np.arange(n_out).astype(dt) + dt(0.5)
    s = c * scale
    s = s - dt(0.5)
    s = np.maximum(s, dt(0))
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    w = s - i0.astype(dt)
    return i0, i1, w


def residual(dec, x, valid, dt=np.float32):
    """dec (3 or 4, PH, PW), x (3, PH, PW) -> r (3, oh, ow), m (oh, ow): the valid region only"""
    oh, ow = valid
    dec = np.asarray(dec, np.float32)[:, :oh, :ow].astype(dt)
    x = np.asarray(x, np.float32)[:, :oh, :ow].astype(dt)
    if dec.shape[0] == 4:
        s = dec[3] + dt(1)
        m = s * dt(0.5)
    else:
        m = np.ones((oh, ow), dt)
    diff = dec[:3] - x
    h = diff * dt(0.5)
    return m[None] * h, m


def _bilinear(v, yy, xx):
    """v (..., oh, ow) sampled at the taps; every product and sum rounded on its own, in the header's association"""
    (y0, y1, wy), (x0, x1, wx) = yy, xx
    uy, ux = (wy.dtype.type(1) - wy)[:, None], wx.dtype.type(1) - wx
    wy = wy[:, None]
    r0, r1 = v[..., y0, :], v[..., y1, :]
    a = ux * r0[..., x0]
    b = wx * r0[..., x1]
    top = a + b
    c = ux * r1[..., x0]
    d = wx * r1[..., x1]
    bot = c + d
    e = uy * top
    f = wy * bot
    return e + f


def paste(dec, x, valid, source, dt=np.float32):
    """One image.  source (Hs, Ws, 3) uint8 -> (bar, mask), each (Hs, Ws, 3) uint8"""
    source = np.asarray(source, np.uint8)
    Hs, Ws = source.shape[:2]
    r, m = residual(dec, x, valid, dt)
    yy, xx = axis(valid[0], Hs, dt), axis(valid[1], Ws, dt)
    R = _bilinear(r, yy, xx)                               # (3, Hs, Ws)
    t = R * dt(255)
    v = source.transpose(2, 0, 1).astype(dt) + t
    v = v + dt(0.5)
    bar = np.clip(v, dt(0), dt(255)).astype(np.uint8).transpose(1, 2, 0)
    M = _bilinear(m, yy, xx)
    t = M * dt(255)
    v = t + dt(0.5)
    mask = np.clip(v, dt(0), dt(255)).astype(np.uint8)
    return np.ascontiguousarray(bar), np.ascontiguousarray(np.repeat(mask[:, :, None], 3, 2))


# (oh, ow | PH, PW | Hs, Ws): the smallest shapes that reach every branch -- identity, non-integer up-scale, large ratio, down-scale,
# ragged with padding, degenerate source, the clamp of i1 on both axes
SHAPES = [((4, 4), (4, 4), (4, 4)), ((5, 7), (8, 8), (13, 29)), ((4, 4), (4, 4), (64, 61)), ((8, 12), (8, 12), (3, 5)),
          ((16, 22), (16, 24), (21, 30)), ((6, 5), (8, 8), (1, 1)), ((4, 8), (4, 8), (37, 9))]


def case(shape, channels, seed=0):
    """random tanh decoder outputs, a net input in [-1, 1] and source bytes for one entry of SHAPES: (dec, x, valid, source)"""
    valid, (PH, PW), (Hs, Ws) = shape
    rng = np.random.RandomState(1000 * seed + 100 * PH + 10 * Ws + channels)
    dec = np.tanh(rng.randn(channels, PH, PW) * 1.5).astype(np.float32)
    x = (rng.rand(3, PH, PW) * 2 - 1).astype(np.float32)
    source = rng.randint(0, 256, (Hs, Ws, 3)).astype(np.uint8)
    return dec, x, valid, source
