"""Guided-filter upsampling of the edit (acl-gan_amd/translate.py: guided_u8; csrc/guided.hip; translate_photos.py --detail guided): what needs
no GPU.

(a) a closed mask returns the source bytes, and the mask picture is the paste's, on the fp32 model tests/guided_ref.py -- the model
    tests/test_gpu_guided.py holds the kernels to;
(b) the fp32 model against the same rule in fp64: at most one level per byte, on at most 1 % of the bytes.  Every product of the chain is of
    size <= a few, eps >= 1e-4 keeps a's denominator away from the cancellation in var, and the result is scaled by 255: the fp32 error is
    orders of magnitude below one level, so a difference is a flip at a rounding boundary;
(c) the point of the feature: under an open mask and an edit that is an affine function of the input, the guided bytes are at most half as
    far from the edit at full resolution as the bilinear paste's;
(d) the argument checks of the three entry points, which return before any launch, and the device paths' refusal of host tensors;
(e) the switches: translate_folder's forward gets detail='guided' only when asked, 'guided' without full_size is refused, and
    translate_photos.py lists and checks the three flags."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import guided_ref as G
import paste_ref as P

import aclgan_amd  # noqa: F401
from aclgan_amd import _lib as L
from aclgan_amd import translate as TR

IDS = lambda s: "%dx%d_to_%dx%d" % (s[0] + s[2])
RADII = [1, 2, 5]                           # 5 is wider than the 4x4 regions: the window is the whole region


# ---- (a) ----
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("channels", [4, 3])
@pytest.mark.parametrize("shape", G.SHAPES, ids=IDS)
def test_closed_mask_returns_the_source(shape, channels, radius):
    dec, x, valid, source = G.case(shape, channels)
    if channels == 4:
        dec[3] = -1.0                       # f = -1: m = 0 everywhere
    else:
        dec[:3] = x                         # no focus plane: m = 1, and the edit itself is nothing
    A, Bq, _ = G.coefficients(dec, x, valid, radius, 1e-3)
    assert not A.any() and not Bq.any()     # r = 0: cov = 0, a = 0, b = 0
    bar, mask = G.guided(dec, x, valid, source, radius, 1e-3)
    assert np.array_equal(bar, source)
    assert np.array_equal(mask, P.paste(dec, x, valid, source)[1])
    assert np.all(mask == (0 if channels == 4 else 255))


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("shape", G.SHAPES, ids=IDS)
def test_mask_bytes_are_the_pastes(shape, radius):
    dec, x, valid, source = G.case(shape, 4)
    assert np.array_equal(G.guided(dec, x, valid, source, radius, 1e-3)[1], P.paste(dec, x, valid, source)[1])


def test_box_mean_is_the_clipped_window_mean():
    """the model's box against a direct clipped-window mean in fp64 (where the order of summation does not show at this tolerance)"""
    rng = np.random.RandomState(3)
    v = rng.rand(2, 9, 13)
    for radius in (1, 3, 16):
        got = G.box_mean(v, radius)
        for i in (0, 4, 8):
            for j in (0, 6, 12):
                w = v[:, max(i - radius, 0):i + radius + 1, max(j - radius, 0):j + radius + 1]
                assert np.allclose(got[:, i, j], w.mean((1, 2)), rtol=1e-13, atol=0)


# ---- (b) ----
def _count(a, b):
    d = np.abs(a.astype(np.int32) - b.astype(np.int32))
    return d.size, int((d != 0).sum()), int(d.max())


@pytest.mark.parametrize("radius", RADII)
def test_fp32_model_within_one_level_of_fp64(radius):
    total = ndiff = worst = 0
    for shape in G.SHAPES:
        for channels in (3, 4):
            dec, x, valid, source = G.case(shape, channels, seed=1)
            b32, m32 = G.guided(dec, x, valid, source, radius, 1e-3, np.float32)
            b64, m64 = G.guided(dec, x, valid, source, radius, 1e-3, np.float64)
            for a, b in ((b32, b64), (m32[:, :, 0], m64[:, :, 0])):
                n, nd, w = _count(a, b)
                total, ndiff, worst = total + n, ndiff + nd, max(worst, w)
    print("fp32 / fp64 model, radius %d: %d of %d bytes differ, largest difference %d" % (radius, ndiff, total, worst))
    assert total == 42208 and worst <= 1 and ndiff <= total // 100


def test_fp32_model_within_one_level_of_fp64_on_smooth_guides():
    """a guide with little variance -- a linear ramp with unit noise -- is where a = cov / (var + eps) is least well conditioned"""
    total = ndiff = worst = 0
    oh, ow, factor = 16, 24, 4
    for seed in range(4):
        rng = np.random.RandomState(50 + seed)
        ramp = 60 + 120 * (np.arange(ow * factor)[None, :, None] + np.arange(oh * factor)[:, None, None]) / (ow * factor + oh * factor)
        source = np.clip(ramp + rng.randint(-1, 2, (oh * factor, ow * factor, 3)), 0, 255).astype(np.uint8)
        x = (source.reshape(oh, factor, ow, factor, 3).mean((1, 3)).transpose(2, 0, 1) / 255.0 * 2 - 1).astype(np.float32)
        dec = np.tanh(rng.randn(4, oh, ow) * 1.5).astype(np.float32)
        b32, _ = G.guided(dec, x, (oh, ow), source, 2, 1e-4, np.float32)
        b64, _ = G.guided(dec, x, (oh, ow), source, 2, 1e-4, np.float64)
        n, nd, w = _count(b32, b64)
        total, ndiff, worst = total + n, ndiff + nd, max(worst, w)
    print("fp32 / fp64 model, smooth guides: %d of %d bytes differ, largest difference %d" % (ndiff, total, worst))
    assert total == 73728 and worst <= 1 and ndiff <= total // 100


# ---- (c) ----
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("radius", [2, 4])
@pytest.mark.parametrize("factor", [4, 8])
@pytest.mark.parametrize("valid", [(16, 24), (32, 40)], ids=lambda v: "%dx%d" % v)
def test_guided_halves_the_error_of_the_bilinear_paste(valid, factor, radius, seed):
    dec, x, source, target = G.quality_case(valid, factor, seed)
    guided, _ = G.guided(dec, x, valid, source, radius, 1e-3)
    pasted, _ = P.paste(dec, x, valid, source)
    eg, ep = np.abs(guided - target).mean(), np.abs(pasted - target).mean()
    print("mean absolute error in levels: guided %.3f, bilinear %.3f, ratio %.3f" % (eg, ep, eg / ep))
    assert eg <= 0.5 * ep


# ---- (d) ----
def test_scratch_query_needs_no_gpu():
    f = L.lib.aclgan_translate_guided_scratch_bytes
    assert f(2, 5, 7, 4) == 2 * 6 * 5 * 7 * 4
    assert f(8, 256, 341, 16) == 8 * 6 * 256 * 341 * 4
    for bad in ((0, 5, 7, 4), (2, 0, 7, 4), (2, 5, -1, 4), (2, 5, 7, 0), (2, 5, 7, 17), (1 << 20, 5, 7, 4), (2, 1 << 15, 1 << 15, 4)):
        assert f(*bad) == 0, bad


def test_coef_argument_checks_return_before_any_launch():
    f = L.lib.aclgan_translate_guided_coef
    p = C.c_void_p(0x1000)             # never dereferenced: every call below is refused by the checks in front of the launches
    ok = dict(dec=p, dec_bs=4 * 64, ch=4, x=p, x_bs=3 * 64, B=2, oh=5, ow=7, PH=8, PW=8, radius=4, eps=1e-3, coef=p, scratch=p)

    def call(**over):
        a = dict(ok, **over)
        return f(a["dec"], a["dec_bs"], a["ch"], a["x"], a["x_bs"], a["B"], a["oh"], a["ow"], a["PH"], a["PW"], a["radius"], a["eps"], a["coef"],
                 a["scratch"], None)

    for what, over in (("null dec", dict(dec=None)), ("null x", dict(x=None)), ("null coef", dict(coef=None)), ("null scratch", dict(scratch=None)),
                       ("2 channels", dict(ch=2)), ("5 channels", dict(ch=5)), ("B = 0", dict(B=0)), ("B too large", dict(B=1 << 20)),
                       ("oh = 0", dict(oh=0)), ("ow < 0", dict(ow=-1)), ("PH below oh", dict(PH=4)), ("PW below ow", dict(PW=4)),
                       ("planes too large", dict(PH=1 << 15, PW=1 << 15)), ("negative dec stride", dict(dec_bs=-4)),
                       ("negative x stride", dict(x_bs=-4)), ("radius 0", dict(radius=0)), ("radius -1", dict(radius=-1)), ("radius 17", dict(radius=17)),
                       ("eps 0", dict(eps=0.0)), ("eps below 1e-6", dict(eps=5e-7)), ("eps above 1", dict(eps=1.5)), ("eps negative", dict(eps=-1e-3)),
                       ("eps NaN", dict(eps=float("nan")))):
        assert call(**over) == -1, what                    # ACLGAN_EINVAL
        assert "translate_guided_coef" in L.last_error(), what


def test_paste_argument_checks_return_before_any_launch():
    f = L.lib.aclgan_translate_guided_paste_u8
    p = C.c_void_p(0x1000)             # never dereferenced
    sizes = [(13, 29), (1, 1)]

    def descs(src_off=(0, 1131), out_off=(0, 1131), sz=sizes):
        d = (L.PasteDesc * 2)()
        for k in range(2):
            d[k].src_offset, d[k].out_offset, d[k].src_h, d[k].src_w = src_off[k], out_off[k], sz[k][0], sz[k][1]
        return d

    ok = dict(coef=p, planes=7, B=2, oh=5, ow=7, src=p, src_bytes=1134, dh=descs(), dd=p, bar=p, mask=p, out_bytes=1134)

    def call(**over):
        a = dict(ok, **over)
        return f(a["coef"], a["planes"], a["B"], a["oh"], a["ow"], a["src"], a["src_bytes"], a["dh"], a["dd"], a["bar"], a["mask"], a["out_bytes"], None)

    for what, over in (("null coef", dict(coef=None)), ("null src", dict(src=None)), ("null host descriptors", dict(dh=None)),
                       ("null device descriptors", dict(dd=None)), ("no output", dict(bar=None, mask=None)), ("5 planes", dict(planes=5)),
                       ("8 planes", dict(planes=8)), ("mask from 6 planes", dict(planes=6)), ("mask alone from 6 planes", dict(planes=6, bar=None)),
                       ("B = 0", dict(B=0)), ("B too large", dict(B=1 << 20)), ("oh = 0", dict(oh=0)), ("ow < 0", dict(ow=-1)),
                       ("region too large", dict(oh=1 << 15, ow=1 << 15)),
                       ("source size 0", dict(dh=descs(sz=[(13, 29), (0, 1)]))), ("source too large", dict(dh=descs(sz=[(13, 29), (1 << 23, 1)]))),
                       ("negative source offset", dict(dh=descs(src_off=(-1, 1131)))), ("source past the buffer", dict(src_bytes=1133)),
                       ("source offset past the buffer", dict(dh=descs(src_off=(4, 1132)))), ("outputs overlap", dict(dh=descs(out_off=(0, 1130)))),
                       ("outputs do not ascend", dict(dh=descs(out_off=(3, 0)), out_bytes=4096)), ("negative output offset", dict(dh=descs(out_off=(-3, 1131)))),
                       ("output past the buffer", dict(out_bytes=1133))):
        assert call(**over) == -1, what                    # ACLGAN_EINVAL
        assert "translate_guided_paste_u8" in L.last_error(), what


def test_device_paths_refuse_host_tensors():
    with pytest.raises(L.AclganError, match="no CPU path"):
        TR.guided_u8(torch.zeros(1, 4, 8, 8), torch.zeros(1, 3, 8, 8), (5, 7), torch.zeros(3, dtype=torch.uint8), None)


# ---- (e) ----
class _Stub:
    """the device halves of translate_folder on the CPU, recording what the forward was given (full_size: the transform in its halves)"""

    def __init__(self):
        self.calls = []

    def __call__(self, images):
        return self.launch(self.stage(images))

    def stage(self, images):
        return [np.asarray(im, dtype=np.uint8).copy() for im in images]

    def launch(self, st):
        return torch.stack([torch.from_numpy(a).permute(2, 0, 1).float().div(255.0) for a in st])

    def sources(self, st):
        offs = np.cumsum([0] + [a.size for a in st])
        return torch.from_numpy(np.concatenate([a.reshape(-1) for a in st])), [(int(o), a.shape[0], a.shape[1]) for o, a in zip(offs, st)]

    def forward(self, trainer, images, styles, a2b, with_input, **kw):
        B, _, H, W = images.shape
        self.calls.append({"shape": (B, H, W), "with_input": with_input, "kw": kw})
        res = {"dec": [torch.zeros(B, 4, H, W)], "images": images}
        if "sources" in kw:
            sizes = [(h, w) for _, h, w in kw["sources"][1]]
            offs = np.cumsum([0] + [h * w * 3 for h, w in sizes])
            res.update(bytes=torch.zeros(2, int(offs[-1]), dtype=torch.uint8), sizes=sizes, offsets=[int(o) for o in offs[:-1]])
        else:
            res["bytes"] = torch.zeros(2 + (1 if with_input else 0), B, H, W, 3, dtype=torch.uint8)
        return res


def test_folder_passes_detail_on_only_when_asked(tmp_path):
    from PIL import Image
    src = os.path.join(tmp_path, "in")
    os.makedirs(src)
    for name, (w, h) in (("fine.png", (64, 64)), ("odd.png", (64, 50))):
        Image.fromarray(np.zeros((h, w, 3), np.uint8)).save(os.path.join(src, name))
    cfg = {"gen": {"n_downsample": 2, "style_dim": 8}, "focus_loss": 1, "new_size": None}
    run = lambda stub, out, **kw: TR.translate_folder(None, cfg, src, os.path.join(tmp_path, out), forward=stub.forward, transform=stub, **kw)

    stub = _Stub()
    run(stub, "o0", fit="pad", full_size=True, detail="guided")
    assert [sorted(c["kw"]) for c in stub.calls] == [["detail", "guided_eps", "guided_radius", "multiple", "sources"]] * 2
    assert all(c["kw"]["detail"] == "guided" and c["kw"]["guided_radius"] == 4 and c["kw"]["guided_eps"] == 1e-3 for c in stub.calls)
    with Image.open(os.path.join(tmp_path, "o0", "_00_bar", "odd.png")) as im:
        assert im.size == (64, 50)
    stub = _Stub()
    run(stub, "o1", fit="pad", full_size=True, detail="guided", guided_radius=2, guided_eps=1e-2)
    assert all(c["kw"]["guided_radius"] == 2 and c["kw"]["guided_eps"] == 1e-2 for c in stub.calls) and len(stub.calls) == 2

    for kw in ({}, {"detail": "bilinear"}):                 # the default, spelt out or not: nothing new reaches the forward
        stub = _Stub()
        run(stub, "o2", fit="pad", full_size=True, **kw)
        assert [sorted(c["kw"]) for c in stub.calls] == [["multiple", "sources"]] * 2
        stub = _Stub()
        run(stub, "o3", fit="pad", **kw)
        assert [c["kw"] for c in stub.calls] == [{"multiple": 4}] * 2
        stub = _Stub()
        run(stub, "o4", max_images=1, **kw)
        assert [c["kw"] for c in stub.calls] == [{}]


def test_guided_without_full_size_is_refused_with_the_reason(tmp_path):
    from PIL import Image
    src = os.path.join(tmp_path, "in")
    os.makedirs(src)
    Image.fromarray(np.zeros((64, 64, 3), np.uint8)).save(os.path.join(src, "fine.png"))
    cfg = {"gen": {"n_downsample": 2, "style_dim": 8}, "focus_loss": 1, "new_size": None}
    stub = _Stub()
    for kw in ({}, {"fit": "pad"}):
        with pytest.raises(L.AclganError, match="needs full_size.*nothing to upsample"):
            TR.translate_folder(None, cfg, src, os.path.join(tmp_path, "o"), forward=stub.forward, transform=stub, detail="guided", **kw)
    with pytest.raises(L.AclganError, match="detail must be one of"):
        TR.translate_folder(None, cfg, src, os.path.join(tmp_path, "o"), forward=stub.forward, transform=stub, full_size=True, detail="bicubic")
    assert stub.calls == [] and not os.path.exists(os.path.join(tmp_path, "o"))
    with pytest.raises(L.AclganError, match="nothing to upsample"):         # translate_batch itself: refused before anything touches the trainer
        TR.translate_batch(None, torch.zeros(1, 3, 8, 8), torch.zeros(1, 1, 8, 1, 1), detail="guided")
    with pytest.raises(L.AclganError, match="detail must be one of"):
        TR.translate_batch(None, torch.zeros(1, 3, 8, 8), torch.zeros(1, 1, 8, 1, 1), detail="bicubic")


def test_script_lists_the_detail_flags():
    script = os.path.join(ROOT, "translate_photos.py")
    r = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--detail", "bilinear", "guided", "--guided_radius", "--guided_eps", "--fit", "--full_size"):
        assert flag in r.stdout, flag
    r = subprocess.run([sys.executable, script, "--detail", "bicubic"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--detail" in r.stderr and "invalid choice" in r.stderr
    r = subprocess.run([sys.executable, script, "--fit", "pad", "--detail", "guided"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "nothing to upsample" in r.stderr
    r = subprocess.run([sys.executable, script, "--fit", "pad", "--full_size", "--detail", "guided", "--guided_radius", "2", "--guided_eps", "1e-2"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--config is required" in r.stderr           # the flags parse; the run stops at the missing paths
