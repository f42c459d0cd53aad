"""numpy model of the adaptive augmentation probability (include/aclgan_hip.h: aclgan_ctx_set_ada, aclgan_augment_gate): the gate as a select,
the sign statistic in fp64 and as the library accumulates it in fp32, and the fold as the sequence of fp32 operations the header writes out.
Everything here is exact arithmetic on a handful of numbers, so the GPU tests compare bits."""
import numpy as np

F = np.float32
STATE_FLOATS = 12
P, R_T, ISUM, ICOUNT, UPDATES, ADJUSTMENTS, R, PAIR_A, PAIR_B = 0, 1, 2, 3, 4, 5, 6, 8, 10
OPS = ((1, (0, 1, 2)), (2, (3, 4)), (4, (5, 6)))      # (policy bit, columns) of color, translation, cutout -- the order of u's columns


def neutral_row(H, W):
    """the values draw_augment_params documents for an operation that is off"""
    return np.array([0, 1, 1, 0, 0, W, H, 0], dtype=F)


def gate(rows, u, p, H, W, policy):
    """rows (n, 8), u (n, 4) float32, p a float32: the effective rows"""
    rows, u, p = np.asarray(rows, dtype=F), np.asarray(u, dtype=F), F(p)
    out = rows.copy()
    neutral = neutral_row(H, W)
    for k, (bit, cols) in enumerate(OPS):
        if not policy & bit:
            continue
        off = ~(u[:, k] < p)
        for c in cols:
            out[off, c] = neutral[c]
    return out


def sign_q(o):
    """mean(sgn(o - 0.5)) in fp64, sgn(0) = 0; NaN when o holds one"""
    o = np.asarray(o, dtype=np.float64).ravel()
    if np.isnan(o).any():
        return float("nan")
    return (float((o > 0.5).sum()) - float((o < 0.5).sum())) / o.size


def sign_acc(pair, maps, weights):
    """the library's accumulation of (sum w q, sum w) in fp32, terms in order: q = fp32(count) / fp32(n), one rounding"""
    a, b = F(pair[0]), F(pair[1])
    for o, w in zip(maps, weights):
        o = np.asarray(o, dtype=F).ravel()
        if np.isnan(o).any():
            q = F("nan")
        else:
            d = o - F(0.5)
            q = F(int((d > 0).sum()) - int((d < 0).sum())) / F(o.size)
        a = a + F(w) * q
        b = b + F(w)
    return a, b


def new_state(p=0.0):
    s = np.zeros(STATE_FLOATS, dtype=F)
    s[P] = p
    return s


def fold(state, target, interval, step):
    """one ada_fold on a (12,) float32 state: returns the new state"""
    s = np.array(state, dtype=F)
    n = s.view(np.int32)
    target, step = F(target), F(step)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = (s[PAIR_A] + s[PAIR_B]) / (s[PAIR_A + 1] + s[PAIR_B + 1])
    s[PAIR_A:PAIR_B + 2] = 0
    s[R] = r
    if np.isfinite(r):
        s[ISUM] = s[ISUM] + r
        s[ICOUNT] = s[ICOUNT] + F(1)
    n[UPDATES] += 1
    if n[UPDATES] % interval:
        return s
    if s[ICOUNT] > 0:
        rt = s[ISUM] / s[ICOUNT]
        s[R_T] = rt
        d = step if rt > target else -step if rt < target else F(0)
        if d != 0:
            s[P] = min(max(s[P] + d, F(0)), F(1))
        n[ADJUSTMENTS] += 1
    s[ISUM] = 0
    s[ICOUNT] = 0
    return s


def readout(state):
    s = np.asarray(state, dtype=F)
    n = s.view(np.int32)
    return {"p": float(s[P]), "r_t": float(s[R_T]), "r": float(s[R]), "updates": int(n[UPDATES]), "adjustments": int(n[ADJUSTMENTS])}
