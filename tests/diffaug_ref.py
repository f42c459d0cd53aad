"""The reference of the differentiable augmentation (include/aclgan_hip.h: aclgan_diffaugment_fwd) for the tests: a small torch function
on NCHW tensors that restates the operator's formulas in the dtype of its input (fp64 for the operator tests, fp32 inside the fp32
oracle); autograd supplies its backward.  diffaug_bwd_ref is the analytic adjoint the kernels implement, kept here so that the CPU suite
checks it against autograd.  oracle_dis_forward wraps the oracle's module-level dis_forward for the step-level tests.

x (N, C, H, W) with C in {3, 6} (6: two 3-channel images sharing one row); p (N, 8) = (b, s, c, tx, ty, cx, cy, 0);
policy bits color 1, translation 2, cutout 4; order colour, translation, cutout."""
import torch

COLOR, TRANSLATION, CUTOUT = 1, 2, 4


def _geometry(p, policy, H, W):
    N = p.shape[0]
    z = torch.zeros(N, dtype=torch.long)
    tx = p[:, 3].round().long() if policy & TRANSLATION else z
    ty = p[:, 4].round().long() if policy & TRANSLATION else z
    cx = p[:, 5].round().long() if policy & CUTOUT else z + W
    cy = p[:, 6].round().long() if policy & CUTOUT else z + H
    return tx, ty, cx, cy


def _cut_mask(cx, cy, H, W):
    """(N, 1, H, W) bool: True outside the rectangle"""
    i = torch.arange(H).view(1, H, 1)
    j = torch.arange(W).view(1, 1, W)
    cy, cx = cy.view(-1, 1, 1), cx.view(-1, 1, 1)
    inside = (i >= cy) & (i < cy + (H + 1) // 2) & (j >= cx) & (j < cx + (W + 1) // 2)
    return (~inside).unsqueeze(1)


def _shift(w, dy, dx):
    """out[n, :, i, j] = w[n, :, i + dy[n], j + dx[n]] inside the frame, else 0"""
    N, C, H, W = w.shape
    ii = torch.arange(H).view(1, H, 1) + dy.view(N, 1, 1)
    jj = torch.arange(W).view(1, 1, W) + dx.view(N, 1, 1)
    valid = ((ii >= 0) & (ii < H) & (jj >= 0) & (jj < W)).unsqueeze(1)
    n = torch.arange(N).view(N, 1, 1)
    out = w[n, :, ii.clamp(0, H - 1), jj.clamp(0, W - 1)]      # (N, H, W, C)
    return out.permute(0, 3, 1, 2) * valid.to(w.dtype)


def diffaug_ref(x, p, policy):
    N, C, H, W = x.shape
    assert C in (3, 6) and p.shape == (N, 8) and 1 <= policy <= 7
    w = x
    if policy & COLOR:
        b, s, c = (p[:, k].to(x.dtype).view(N, 1, 1, 1, 1) for k in range(3))
        u = x.reshape(N, C // 3, 3, H, W) + b
        pm = u.mean(2, keepdim=True)
        v = (u - pm) * s + pm
        m = v.mean((2, 3, 4), keepdim=True)
        w = ((v - m) * c + m).reshape(N, C, H, W)
    tx, ty, cx, cy = _geometry(p, policy, H, W)
    y = _shift(w, ty, tx) if policy & TRANSLATION else w
    if policy & CUTOUT:
        y = y * _cut_mask(cx, cy, H, W).to(x.dtype)
    return y


def diffaug_bwd_ref(dy, p, policy):
    """the exact adjoint, written out: g = dy outside the rectangle; dw[i][j] = g[i - ty][j - tx]; dv = c dw + (1 - c) mean_{c,h,w}(dw) per
    group; dx = s dv + (1 - s) mean_c(dv) per pixel"""
    N, C, H, W = dy.shape
    tx, ty, cx, cy = _geometry(p, policy, H, W)
    g = dy * _cut_mask(cx, cy, H, W).to(dy.dtype) if policy & CUTOUT else dy
    dw = _shift(g, -ty, -tx) if policy & TRANSLATION else g
    if not policy & COLOR:
        return dw
    s, c = (p[:, k].to(dy.dtype).view(N, 1, 1, 1, 1) for k in (1, 2))
    dw = dw.reshape(N, C // 3, 3, H, W)
    dv = c * dw + (1 - c) * dw.mean((2, 3, 4), keepdim=True)
    return (s * dv + (1 - s) * dv.mean(2, keepdim=True)).reshape(N, C, H, W)


def neutral_params(rows, H, W):
    """rows that change nothing under any policy: b 0, s 1, c 1, no shift, the rectangle outside the frame"""
    p = torch.zeros(rows, 8)
    p[:, 1] = 1.0
    p[:, 2] = 1.0
    p[:, 5] = float(W)
    p[:, 6] = float(H)
    return p


GEN_BLOCKS = [0, 1, 2, 3, 4]               # oracle.gen_losses: dis_forward call index -> block of the 5 B rows
DIS_BLOCKS = [0, 2, 1, 2, 3, 4, 5, 6]      # oracle.dis_losses: the real x_a block serves both of its calls


def oracle_dis_forward(orig, aug, B, policy, blocks):
    """a replacement for oracle.aclgan_oracle.dis_forward (monkeypatch.setattr(O, "dis_forward", ...)) for ONE update: its k-th call
    augments its input with the rows of block blocks[k] before it runs the discriminator"""
    calls = []

    def wrapper(P, x, dcfg):
        k = len(calls)
        calls.append(k)
        rows = aug[blocks[k] * B:(blocks[k] + 1) * B]
        return orig(P, diffaug_ref(x, rows, policy), dcfg)
    wrapper.calls = calls
    return wrapper
