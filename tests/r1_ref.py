"""Reference of the R1 gradient penalty (include/aclgan_hip.h: aclgan_dis_r1), shared by tests/test_r1_cpu.py and
tests/test_gpu_r1.py.

For one un-normalised MsImageDis D with outputs out_s (B,1,h_s,w_s) on a real batch x:
    s_b = sum_s mean_pixels(out_s[b]),   G = d(sum_b s_b)/dx,   P = gamma/2 * (1/B) * sum_b ||G[b]||^2

r1_autograd     the definition: double backward through the oracle's dis_forward
r1_closed_form  what the library computes: D is piecewise linear in x, so dP/dW is three chains of first-order operators
dis_cfg         a dis: block of the given width, depth and number of scales
"""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from oracle import aclgan_oracle as O


def dis_cfg(dim, n_layer, num_scales):
    d = dict(O.default_config()["dis"])
    d.update(dim=dim, n_layer=n_layer, num_scales=num_scales, norm="none")
    return d


def r1_autograd(P, x, dcfg, gamma):
    """(P, G, {key: dP/dparam}) in the dtype of x, by autograd.grad(..., create_graph=True) through oracle.aclgan_oracle.dis_forward.
    A parameter the penalty does not depend on (every bias) gets exact zeros."""
    Pd = OrderedDict((k, v.detach().to(x.dtype).clone().requires_grad_(True)) for k, v in P.items())
    xr = x.detach().clone().requires_grad_(True)
    outs = O.dis_forward(Pd, xr, dcfg)
    s = sum(o.mean(dim=(1, 2, 3)).sum() for o in outs)
    (G,) = torch.autograd.grad(s, xr, create_graph=True)
    pen = 0.5 * gamma * (G ** 2).sum() / x.shape[0]
    gr = torch.autograd.grad(pen, list(Pd.values()), allow_unused=True)
    grads = OrderedDict((k, torch.zeros_like(v) if g is None else g.detach()) for (k, v), g in zip(Pd.items(), gr))
    return pen.detach(), G.detach(), grads


def _adjoint(fn, like, gy):
    """A^T gy of the LINEAR map fn at an input shaped like `like` (first-order autograd of a linear operator: exact, no graph kept)"""
    z = torch.zeros_like(like).requires_grad_(True)
    with torch.enable_grad():
        (g,) = torch.autograd.grad(fn(z), z, gy)
    return g


def _conv(h, w, b=None):
    """reflect pad 1 + 4x4 stride-2 convolution (networks.py:41, 366)"""
    return F.conv2d(F.pad(h, (1, 1, 1, 1), mode="reflect"), w, b, stride=2)


def r1_closed_form(P, x, dcfg, gamma, scale=1.0):
    """The closed form in torch, in the dtype of x.  Returns (P, G, {key: scale * dP/dparam}, margin); margin = the smallest
    |z| / rms(z of its layer) over all LeakyReLU inputs z -- how far the nearest activation is from changing its branch.
      forward   a_l = lrelu(W_l * pad(a_{l-1}) + b_l), m_l = 1 where a_l > 0 else 0.2, a_0 = x pooled s times
      backward  delta_n = m_n w_f / (h_s w_s);  g_{l-1} = dgrad(W_l, delta_l);  delta_{l-1} = m_{l-1} g_{l-1};  G = sum_s (AvgPool^T)^s g_0^s
      adjoint   Hd = (scale gamma / B) G;  h_0 = Hd pooled s times;  u_l = W_l * pad(h_{l-1});  dW_l += wgrad(h_{l-1}, delta_l);  h_l = m_l u_l;
                dw_f[c] += sum_{b,p} h_n[b,p,c] / (h_s w_s);  bias gradients: zero"""
    with torch.no_grad():
        P = OrderedDict((k, v.detach().to(x.dtype)) for k, v in P.items())
        B, nl, S = x.shape[0], dcfg["n_layer"], dcfg["num_scales"]
        grads = OrderedDict((k, torch.zeros_like(v)) for k, v in P.items())
        xs, margin = [x], float("inf")
        for s in range(1, S):
            xs.append(O.avgpool3s2(xs[-1]))
        masks, deltas, g0 = [], [], []
        for s in range(S):
            a, m_s, in_s = xs[s], [], []
            for l in range(nl):
                in_s.append(a)
                z = _conv(a, P["cnns.%d.%d.conv.weight" % (s, l)], P["cnns.%d.%d.conv.bias" % (s, l)])
                margin = min(margin, float(z.abs().min() / z.pow(2).mean().sqrt()))
                a = F.leaky_relu(z, 0.2)
                m_s.append(torch.where(a > 0, torch.ones_like(a), torch.full_like(a, 0.2)))
            hw = a.shape[2] * a.shape[3]
            g = P["cnns.%d.%d.weight" % (s, nl)].reshape(1, -1, 1, 1).expand_as(a) / hw
            d_s = [None] * nl
            for l in range(nl - 1, -1, -1):
                d_s[l] = m_s[l] * g
                w = P["cnns.%d.%d.conv.weight" % (s, l)]
                g = _adjoint(lambda t: _conv(t, w), in_s[l], d_s[l])
            masks.append(m_s); deltas.append(d_s); g0.append(g)
        G = g0[S - 1]
        for s in range(S - 2, -1, -1):
            G = g0[s] + _adjoint(O.avgpool3s2, xs[s], G)
        pen = 0.5 * gamma * (G ** 2).sum() / B
        h0 = [(scale * gamma / B) * G]
        for s in range(1, S):
            h0.append(O.avgpool3s2(h0[-1]))
        for s in range(S):
            h = h0[s]
            for l in range(nl):
                key = "cnns.%d.%d.conv.weight" % (s, l)
                w = P[key]
                grads[key] += torch.nn.grad.conv2d_weight(F.pad(h, (1, 1, 1, 1), mode="reflect"), w.shape, deltas[s][l], stride=2)
                h = masks[s][l] * _conv(h, w)
            grads["cnns.%d.%d.weight" % (s, nl)] += (h.sum(dim=(0, 2, 3)) / (h.shape[2] * h.shape[3])).reshape(1, -1, 1, 1)
        return pen, G, grads, margin


def separated_biases(P, x, dcfg, factor, seed):
    """A copy of P whose conv biases have magnitude factor x the rms of their layer's bias-free pre-activation, with a random sign per
    channel (layer by layer, each layer seeing the biased layers before it): pre-activations then keep away from zero at any width, and
    both LeakyReLU slopes occur (per channel).  The 1x1 heads keep their bias."""
    g = torch.Generator().manual_seed(seed)
    Q = OrderedDict((k, v.detach().clone()) for k, v in P.items())
    with torch.no_grad():
        xs = x.double()
        for s in range(dcfg["num_scales"]):
            a = xs
            for l in range(dcfg["n_layer"]):
                w = Q["cnns.%d.%d.conv.weight" % (s, l)].double()
                z = _conv(a, w)
                sign = torch.randint(0, 2, (w.shape[0],), generator=g).double() * 2 - 1
                b = factor * z.pow(2).mean().sqrt() * sign
                Q["cnns.%d.%d.conv.bias" % (s, l)] = b.to(P["cnns.%d.%d.conv.bias" % (s, l)].dtype)
                a = F.leaky_relu(z + b.reshape(1, -1, 1, 1), 0.2)
            xs = O.avgpool3s2(xs)
    return Q
