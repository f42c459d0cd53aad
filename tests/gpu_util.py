"""helpers for the -m gpu tests: layout conversion and thin wrappers over the C ABI."""
import ctypes as C
from contextlib import contextmanager

import torch


def nhwc(t):   # NCHW -> NHWC contiguous
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):   # NHWC -> NCHW contiguous
    return t.permute(0, 3, 1, 2).contiguous()


def ohwi(w):   # OIHW -> OHWI contiguous
    return w.permute(0, 2, 3, 1).contiguous()


def oihw(w):
    return w.permute(0, 3, 1, 2).contiguous()


def rel_err(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


@contextmanager
def deterministic_mode(L, on):
    """the library's process-wide deterministic switch set to `on` for the body and restored to its previous value afterwards (1 when the
    whole suite runs under ACLGAN_DETERMINISTIC=1); on = False sets mode 0 explicitly"""
    prev = L.lib.aclgan_get_deterministic()
    L.check(L.lib.aclgan_set_deterministic(1 if on else 0))
    assert L.lib.aclgan_get_deterministic() == (1 if on else 0)
    try:
        yield
    finally:
        L.check(L.lib.aclgan_set_deterministic(prev))


def conv_desc(L, B, Hi, Wi, Ci, Co, k, s, p, up=0, act="none"):
    return L.ConvDesc(B, Hi, Wi, Ci, Co, k, s, p, up, L.ACT[act])


def out_hw(Hi, Wi, k, s, p, up):
    Hu, Wu = Hi << up, Wi << up
    return (Hu + 2 * p - k) // s + 1, (Wu + 2 * p - k) // s + 1


def gpu_conv_fwd(L, d, x_nhwc, w_ohwi, bias, naive=False, ws=True):
    Ho, Wo = out_hw(d.Hi, d.Wi, d.k, d.stride, d.pad, d.upsample)
    y = torch.empty(d.B, Ho, Wo, d.Co, device="cuda")
    if naive:
        L.check(L.lib.aclgan_conv2d_fwd_naive(C.byref(d), L.ptr(x_nhwc), L.ptr(w_ohwi), L.ptr(bias), L.ptr(y), L.stream_ptr()), "conv2d_fwd_naive")
        return y
    nb = L.lib.aclgan_conv2d_fwd_scratch_bytes(C.byref(d))
    if nb and ws:
        scratch = torch.empty(nb // 4 + 16, device="cuda")
        L.check(L.lib.aclgan_conv2d_fwd_ws(C.byref(d), L.ptr(x_nhwc), L.ptr(w_ohwi), L.ptr(bias), L.ptr(y), L.ptr(scratch), L.stream_ptr()), "conv2d_fwd_ws")
    else:
        L.check(L.lib.aclgan_conv2d_fwd(C.byref(d), L.ptr(x_nhwc), L.ptr(w_ohwi), L.ptr(bias), L.ptr(y), L.stream_ptr()), "conv2d_fwd")
    return y


def gpu_conv_dgrad(L, d, dy_nhwc, w_ohwi, accumulate_into=None):
    nb = L.lib.aclgan_conv2d_dgrad_scratch_bytes(C.byref(d))
    scratch = torch.empty(nb // 4 + 16, device="cuda")
    if accumulate_into is None:
        dx = torch.full((d.B, d.Hi, d.Wi, d.Ci), float("nan"), device="cuda")
        acc = 0
    else:
        dx = accumulate_into
        acc = 1
    L.check(L.lib.aclgan_conv2d_dgrad(C.byref(d), L.ptr(dy_nhwc), L.ptr(w_ohwi), L.ptr(dx), L.ptr(scratch), acc, L.stream_ptr()), "conv2d_dgrad")
    return dx


def gpu_conv_wgrad(L, d, x_nhwc, dy_nhwc, ws=True):
    dw = torch.zeros(d.Co, d.k, d.k, d.Ci, device="cuda")
    db = torch.zeros(d.Co, device="cuda")
    nb = L.lib.aclgan_conv2d_wgrad_scratch_bytes(C.byref(d))
    if nb and ws:
        scratch = torch.empty(nb // 4 + 16, device="cuda")
        L.check(L.lib.aclgan_conv2d_wgrad_ws(C.byref(d), L.ptr(x_nhwc), L.ptr(dy_nhwc), L.ptr(dw), L.ptr(db), L.ptr(scratch), L.stream_ptr()), "conv2d_wgrad_ws")
    else:
        L.check(L.lib.aclgan_conv2d_wgrad(C.byref(d), L.ptr(x_nhwc), L.ptr(dy_nhwc), L.ptr(dw), L.ptr(db), L.stream_ptr()), "conv2d_wgrad")
    return dw, db
