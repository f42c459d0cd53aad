"""The five networks as the reference's callers see them: views into the trainer's flat group buffers with the reference's state_dict surface
(OIHW fp32 on disk; the OHWI <-> OIHW repack happens here), encode / decode / forward on the HIP forward path, and what only they need."""
import ctypes as C
import math
from collections import OrderedDict

import torch

from . import _lib as L

def tensor_table(ctx, grp):
    """aclgan_tensor_info of every tensor of a group: dicts of net, key, offset (elements into the flat buffer), shape (SN state: a vector), numel"""
    ents = []
    name = C.create_string_buffer(256)
    off, shp, nd = C.c_int64(), (C.c_int * 4)(), C.c_int()
    for i in range(L.lib.aclgan_tensor_count(ctx, grp)):
        L.check(L.lib.aclgan_tensor_info(ctx, grp, i, name, 256, C.byref(off), shp, C.byref(nd)))
        net, key = name.value.decode().split("/", 1)
        shape = (shp[0],) if grp == L.GROUP_SN_STATE else tuple(shp[j] for j in range(nd.value))
        ents.append(dict(net=net, key=key, offset=off.value, shape=shape, numel=int(math.prod(shape))))
    return ents


def adain_dummy_buffers(arch):
    """AdaIN running_mean / running_var of both generators: never used, but in the state_dict (networks.py:488-489)"""
    d = arch.gen_dim << arch.gen_n_downsample
    out = {}
    for net in ("gen_AB", "gen_BA"):
        b = OrderedDict()
        for r in range(arch.gen_n_res):
            for j in range(2):
                b["dec.model.0.model.%d.model.%d.norm.running_mean" % (r, j)] = torch.zeros(d)
                b["dec.model.0.model.%d.model.%d.norm.running_var" % (r, j)] = torch.ones(d)
        out[net] = b
    return out


def _ref_key_order(pkeys, bkeys):
    """the reference's state_dict order.  AdaIN blocks: norm buffers precede the conv parameters of the same Conv2dBlock"""
    out = []
    for k in pkeys:
        if k.endswith("conv.weight") and k.startswith("dec.model.0."):
            pre = k[: -len("conv.weight")]
            out += [pre + "norm.running_mean", pre + "norm.running_var"]
        if k.endswith(".module.weight_bar"):     # SpectralNorm registers u, v, then bar after the conv's bias (networks.py:577-579)
            pre = k[: -len("weight_bar")]
            out += [pre + "weight_u", pre + "weight_v"]
        out.append(k)
    assert set(out) == set(pkeys) | set(bkeys), (set(out) ^ (set(pkeys) | set(bkeys)))
    return out


def init_weights(t, kind):
    """weight init of trainer t's networks (trainer.py:48-52, utils.py:274-294), then the SN state, from torch's global CPU generator in this order"""
    for grp, nets in ((L.GROUP_GEN, (t.gen_AB, t.gen_BA)), (L.GROUP_DIS, (t.dis_A, t.dis_B, t.dis_2))):
        for net in nets:
            for key, v in net.named_parameters():
                if ".module." in key:
                    # spectrally normalised conv: weights_init skips it (no `weight` attribute after the wrap, utils.py:277), so
                    # nn.Conv2d's own initialisation stays: kaiming-uniform(a=sqrt 5) weight, bias ~ U(+-1/sqrt(fan_in))
                    if key.endswith("weight_bar"):
                        v.copy_(torch.nn.init.kaiming_uniform_(torch.empty(tuple(v.shape)), a=math.sqrt(5.0)).to(t.device))
                    else:
                        bar = next(e for e in net._entries if e["key"] == key[: -len("bias")] + "weight_bar")
                        fan_in = int(math.prod(bar["shape"][1:]))
                        b = 1.0 / math.sqrt(fan_in)
                        v.copy_(torch.empty(tuple(v.shape)).uniform_(-b, b).to(t.device))
                elif key.endswith(".weight"):
                    fan_in = int(math.prod(v.shape[1:]))
                    if grp == L.GROUP_DIS or kind == "gaussian":
                        w = torch.randn(tuple(v.shape)) * 0.02
                    elif kind == "kaiming":
                        w = torch.randn(tuple(v.shape)) * math.sqrt(2.0 / fan_in)
                    elif kind == "xavier":
                        fan_out = v.shape[0] * int(math.prod(v.shape[2:]))
                        w = torch.randn(tuple(v.shape)) * math.sqrt(2.0) * math.sqrt(2.0 / (fan_in + fan_out))
                    elif kind == "orthogonal":     # utils.py:285-286
                        w = torch.nn.init.orthogonal_(torch.empty(tuple(v.shape)), gain=math.sqrt(2.0))
                    elif kind == "default":        # utils.py:287-288: nn.Conv2d / nn.Linear's own reset_parameters() stays
                        w = torch.nn.init.kaiming_uniform_(torch.empty(tuple(v.shape)), a=math.sqrt(5.0))
                    else:
                        raise L.AclganError("Unsupported initialization: %s" % kind)
                    v.copy_(w.to(t.device))
                elif key.endswith(".gamma"):
                    v.copy_(torch.rand(tuple(v.shape)).to(t.device))   # networks.py:517
                else:
                    v.zero_()
    # u, v ~ N(0, 1), l2-normalised (networks.py:571-574)
    for e in t._tensors[L.GROUP_SN_STATE]:
        x = torch.randn(e["numel"], dtype=torch.float64)
        t._sn_state[e["offset"]: e["offset"] + e["numel"]].copy_((x / (x.norm() + 1e-12)).float().to(t.device))


class _Net:
    """A view of one network's tensors inside the flat group buffers, with the reference's state_dict surface."""

    def __init__(self, trainer, name):
        self._t = trainer
        self.name = name
        self.net_id = L.NETS[name]
        self.group = L.GROUP_GEN if name.startswith("gen") else L.GROUP_DIS
        self._entries = [e for e in trainer._tensors[self.group] if e["net"] == name]

    # ---- tensor access ----
    def _view(self, e, buf):
        flat = buf[e["offset"]: e["offset"] + e["numel"]]
        shp = e["shape"]
        if len(shp) == 4:   # OHWI in memory -> OIHW view (what the reference stores)
            co, ci, kh, kw = shp
            return flat.view(co, kh, kw, ci).permute(0, 3, 1, 2)
        return flat.view(*shp)

    def _named_views(self, buf):
        for e in self._entries:
            yield e["key"], self._view(e, buf)

    def named_parameters(self):
        return self._named_views(self._t._param[self.group])

    def named_grads(self):
        return self._named_views(self._t._grad[self.group])

    def parameters(self):
        return [p for _, p in self.named_parameters()]

    def state_dict(self):
        return self._state_dict_of(self._t._param[self.group])

    def _state_dict_of(self, buf):
        """the reference's state_dict with the parameters read from `buf` (the group's flat parameter buffer, or the generators' average)"""
        sd = OrderedDict()
        params = OrderedDict((k, v.contiguous().clone()) for k, v in self._named_views(buf))
        bufs = self._buffers()
        for k in _ref_key_order(list(params.keys()), list(bufs.keys())):
            sd[k] = params[k] if k in params else bufs[k]
        return sd

    def _buffers(self):
        return OrderedDict()

    def load_state_dict(self, sd, strict=True):
        self._t._carry_epoch += 1
        mine = OrderedDict(self.named_parameters())
        missing = [k for k in mine if k not in sd]
        unexpected = [k for k in sd if k not in mine and k not in self._buffers()]
        if strict and (missing or unexpected):
            raise L.AclganError("load_state_dict(%s): missing %s unexpected %s" % (self.name, missing, unexpected))
        with torch.no_grad():
            for k, v in mine.items():
                if k in sd:
                    src = sd[k].to(device=v.device, dtype=torch.float32)
                    if tuple(src.shape) != tuple(v.shape):
                        raise L.AclganError("load_state_dict(%s): shape mismatch for %s: %s vs %s" % (self.name, k, tuple(src.shape), tuple(v.shape)))
                    v.copy_(src)
        for k in self._buffers():
            if k in sd:
                self._load_buffer(k, sd[k])

    def _load_buffer(self, key, value):
        self._t._dummy_buffers[self.name][key] = value.detach().clone().cpu()

    def cuda(self, *a, **k):      # (and eval / train: there is nothing to move or to switch)
        return self
    eval = train = cuda


class AdaINGen(_Net):
    """reference networks.py:112-171 -- encode / decode on the HIP forward path."""

    def _buffers(self):
        return self._t._dummy_buffers[self.name]

    def encode(self, images):
        t = self._t
        images = images.to(t.device, torch.float32).contiguous()
        B, Cin, H, W = images.shape
        a = t.arch
        q = 1 << a.gen_n_downsample
        content = torch.empty(B, a.gen_dim * q, H // q, W // q, device=t.device)
        style = torch.empty(B, a.gen_style_dim, 1, 1, device=t.device)
        with torch.cuda.device(t.device):
            t._ensure_workspace(B, H, W, forward_only=True)
            L.check(L.lib.aclgan_gen_encode(t._ctx, self.net_id, L.ptr(images), B, H, W, L.ptr(content), L.ptr(style), t._st()), "gen_encode")
        return content, style

    def decode(self, content, style):
        t = self._t
        content = content.to(t.device, torch.float32).contiguous()
        style = style.to(t.device, torch.float32).contiguous()
        B, Cc, h, w = content.shape
        a = t.arch
        q = 1 << a.gen_n_downsample
        out = torch.empty(B, a.gen_output_dim, h * q, w * q, device=t.device)
        with torch.cuda.device(t.device):
            t._ensure_workspace(B, h * q, w * q, forward_only=True)
            L.check(L.lib.aclgan_gen_decode(t._ctx, self.net_id, L.ptr(content), L.ptr(style), B, h, w, L.ptr(out), t._st()), "gen_decode")
        return out

    def forward(self, images):
        content, style = self.encode(images)
        return self.decode(content, style)

    __call__ = forward


class MsImageDis(_Net):
    """reference networks.py:21-106 -- forward (list of per-scale maps) on the HIP path.  Under dis.norm: sn every forward call runs one
    power iteration of the spectrally normalised layers (u / v advance, networks.py:547-559), as the reference's does."""

    def _sn_entries(self):
        return [e for e in self._t._tensors.get(L.GROUP_SN_STATE, []) if e["net"] == self.name]

    def _sn_view(self, e):
        """weight_u as stored; weight_v permuted from the library's (kh, kw, ci) column order to the reference's (ci, kh, kw)"""
        flat = self._t._sn_state[e["offset"]: e["offset"] + e["numel"]]
        if e["key"].endswith("weight_v"):
            ci, kh, kw = e["vshape"]
            return flat.view(kh, kw, ci).permute(2, 0, 1).reshape(-1)
        return flat

    def _buffers(self):
        return OrderedDict((e["key"], self._sn_view(e).clone()) for e in self._sn_entries())

    def load_state_dict(self, sd, strict=True):
        missing = [e["key"] for e in self._sn_entries() if e["key"] not in sd]
        if strict and missing:
            raise L.AclganError("load_state_dict(%s): missing %s" % (self.name, missing))
        super().load_state_dict(sd, strict=strict)

    def _load_buffer(self, key, value):
        e = next(e for e in self._sn_entries() if e["key"] == key)
        src = value.detach().to(device=self._t.device, dtype=torch.float32).reshape(-1)
        if src.numel() != e["numel"]:
            raise L.AclganError("load_state_dict(%s): shape mismatch for %s: %s vs (%d,)" % (self.name, key, tuple(value.shape), e["numel"]))
        if key.endswith("weight_v"):
            ci, kh, kw = e["vshape"]
            src = src.view(ci, kh, kw).permute(1, 2, 0).reshape(-1)
        with torch.no_grad():
            self._t._sn_state[e["offset"]: e["offset"] + e["numel"]].copy_(src)

    def forward(self, x):
        t = self._t
        x = x.to(t.device, torch.float32).contiguous()
        B, Cin, H, W = x.shape
        a = t.arch
        outs = []
        h, w = H, W
        for s in range(a.dis_num_scales):
            hs, ws = h, w
            for _ in range(a.dis_n_layer):
                hs, ws = (hs + 2 - 4) // 2 + 1, (ws + 2 - 4) // 2 + 1
            outs.append(torch.empty(B, 1, hs, ws, device=t.device))
            h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        arr = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        with torch.cuda.device(t.device):
            t._ensure_workspace(B, H, W, forward_only=True)
            L.check(L.lib.aclgan_dis_forward(t._ctx, self.net_id, L.ptr(x), B, H, W, arr, t._st()), "dis_forward")
        return outs

    __call__ = forward
