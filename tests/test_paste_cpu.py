"""Photographs at their own size (acl-gan_amd/translate.py, csrc/paste.hip, translate_photos.py --fit pad / --full_size): what needs no GPU.

(a) the properties that follow from the rule, on the fp32 model tests/paste_ref.py -- the model tests/test_gpu_paste.py holds the kernels to;
(b) the fp32 model against the same rule in fp64: at most one level per byte.  The fp32 chain's error (a few ulp of values of size <= 1,
    times 255: ~1e-4 of a level) is orders of magnitude below one level, so the only possible difference is a flip at a rounding boundary;
(c) the planning: fit='pad' admits what the default refuses, the default's message is unchanged, a side below the multiple is refused;
(d) the argument checks of aclgan_translate_pad / aclgan_translate_paste_u8, which return before any launch;
(e) translate_photos.py's flags: test_batch.py's and the two switches."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import paste_ref as P

import aclgan_amd  # noqa: F401
from aclgan_amd import _lib as L
from aclgan_amd import translate as TR


# ---- (a) ----
@pytest.mark.parametrize("channels", [4, 3])
@pytest.mark.parametrize("shape", P.SHAPES, ids=lambda s: "%dx%d_to_%dx%d" % (s[0] + s[2]))
def test_closed_mask_returns_the_source(shape, channels):
    dec, x, valid, source = P.case(shape, channels)
    if channels == 4:
        dec[3] = -1.0                       # f = -1: m = 0 everywhere
    else:
        dec[:3] = x                         # no focus plane: m = 1, and the edit itself is nothing
    bar, mask = P.paste(dec, x, valid, source)
    assert np.array_equal(bar, source)
    assert np.all(mask == (0 if channels == 4 else 255))


@pytest.mark.parametrize("channels", [4, 3])
def test_identity_size_is_source_plus_residual(channels):
    shape = ((16, 22), (16, 24), (16, 22))
    dec, x, valid, source = P.case(shape, channels)
    (y0, y1, wy), (x0, x1, wx) = P.axis(16, 16), P.axis(22, 22)
    assert np.array_equal(y0, np.arange(16)) and np.all(wy == 0) and np.array_equal(x0, np.arange(22)) and np.all(wx == 0)
    r, m = P.residual(dec, x, valid)
    want = np.clip(source.transpose(2, 0, 1).astype(np.float32) + r * np.float32(255) + np.float32(0.5), 0, 255).astype(np.uint8)
    bar, mask = P.paste(dec, x, valid, source)
    assert np.array_equal(bar, want.transpose(1, 2, 0))
    assert np.array_equal(mask[:, :, 0], np.clip(m * np.float32(255) + np.float32(0.5), 0, 255).astype(np.uint8))


def test_pixels_the_edit_leaves_alone_keep_their_bytes():
    """a residual that is zero at the four taps of a pixel returns that pixel's source byte, whatever its neighbours do"""
    dec, x, valid, source = P.case(P.SHAPES[1], 4)
    dec[3, :, :4] = -1.0                    # the mask is closed over the left columns of the net picture
    bar, _ = P.paste(dec, x, valid, source)
    x0, x1, _ = P.axis(valid[1], source.shape[1])
    untouched = x1 < 4
    assert untouched.any() and not untouched.all()
    assert np.array_equal(bar[:, untouched], source[:, untouched]) and not np.array_equal(bar, source)


def test_model_reflect_pad():
    x = np.arange(2 * 5 * 7, dtype=np.float32).reshape(2, 5, 7)
    p = P.reflect_pad(x, 4)
    assert p.shape == (2, 8, 8) and np.array_equal(p[:, :5, :7], x)
    assert np.array_equal(p[:, 5], p[:, 3]) and np.array_equal(p[:, 6], p[:, 2]) and np.array_equal(p[:, 7], p[:, 1])
    assert np.array_equal(p[:, :, 7], p[:, :, 5])
    ref = torch.nn.functional.pad(torch.from_numpy(x)[None], (0, 1, 0, 3), mode="reflect")[0].numpy()
    assert np.array_equal(p, ref)
    assert P.reflect_pad(x[:, :4, :4], 4).shape == (2, 4, 4)


# ---- (b) ----
def test_fp32_model_within_one_level_of_fp64():
    total = ndiff = worst = 0
    for shape in P.SHAPES:
        dec, x, valid, source = P.case(shape, 4, seed=1)
        b32, m32 = P.paste(dec, x, valid, source, np.float32)
        b64, m64 = P.paste(dec, x, valid, source, np.float64)
        for a, b in ((b32, b64), (m32[:, :, 0], m64[:, :, 0])):
            d = np.abs(a.astype(np.int32) - b.astype(np.int32))
            total += d.size
            ndiff += int((d != 0).sum())
            worst = max(worst, int(d.max()))
    print("fp32 / fp64 model: %d of %d bytes differ, largest difference %d" % (ndiff, total, worst))
    assert total == 21104 and worst <= 1


# ---- (c) ----
def _sizes(table):
    return lambda path: table[path]


def test_plan_pad_admits_what_the_default_refuses():
    table = {"fine.png": (64, 64), "odd.png": (64, 50)}           # (width, height); no Resize: 50x64 (H x W) as it is
    files = list(table)
    with pytest.raises(L.AclganError, match=r"odd\.png is 50x64 .*multiples of 4"):
        TR.plan_batches(files, None, 4, 8, size_of=_sizes(table))
    plan = TR.plan_batches(files, None, 4, 8, size_of=_sizes(table), fit="pad")
    assert plan == [[(0, "fine.png", (64, 64), (64, 64))], [(1, "odd.png", (50, 64), (52, 64))]]
    assert TR.plan_batches(["fine.png"], None, 4, 8, size_of=_sizes(table)) == [[(0, "fine.png", (64, 64), (64, 64))]]
    # batches form on the resized shape: two ragged files of one shape share a batch
    table = {"a.png": (30, 21), "b.png": (60, 42), "c.png": (16, 16)}
    plan = TR.plan_batches(list(table), 16, 4, 8, size_of=_sizes(table), fit="pad")
    assert [[e[2:] for e in b] for b in plan] == [[((16, 22), (16, 24)), ((16, 22), (16, 24))], [((16, 16), (16, 16))]]
    with pytest.raises(L.AclganError, match="fit must be one of"):
        TR.plan_batches(list(table), 16, 4, 8, size_of=_sizes(table), fit="crop")


def test_plan_pad_refuses_a_side_below_the_multiple_by_name():
    table = {"ok.png": (40, 9), "thin.png": (40, 3)}
    with pytest.raises(L.AclganError, match=r"thin\.png is 3x40 .*at least 4 pixels a side"):
        TR.plan_batches(list(table), None, 4, 8, size_of=_sizes(table), fit="pad")
    assert TR.plan_batches(["ok.png"], None, 4, 8, size_of=_sizes(table), fit="pad")[0][0][3] == (12, 40)


class _Stub:
    """the device halves of translate_folder on the CPU, recording what the forward was given"""

    def __init__(self):
        self.calls = []

    def transform(self, images):
        return torch.stack([torch.from_numpy(np.asarray(im, dtype=np.uint8).copy()).permute(2, 0, 1).float().div(255.0) for im in images])

    def forward(self, trainer, images, styles, a2b, with_input, **kw):
        B, _, H, W = images.shape
        self.calls.append({"shape": (B, H, W), "with_input": with_input, "kw": kw})
        return {"bytes": torch.zeros(2 + (1 if with_input else 0), B, H, W, 3, dtype=torch.uint8), "dec": [torch.zeros(B, 4, H, W)], "images": images}


def test_folder_passes_the_switches_on_and_keeps_the_default_call(tmp_path):
    from PIL import Image
    src = os.path.join(tmp_path, "in")
    os.makedirs(src)
    for name, (w, h) in (("fine.png", (64, 64)), ("odd.png", (64, 50))):
        Image.fromarray(np.zeros((h, w, 3), np.uint8)).save(os.path.join(src, name))
    cfg = {"gen": {"n_downsample": 2, "style_dim": 8}, "focus_loss": 1, "new_size": None}
    stub = _Stub()
    with pytest.raises(L.AclganError, match=r"odd\.png is 50x64 .*multiples of 4"):
        TR.translate_folder(None, cfg, src, os.path.join(tmp_path, "o0"), forward=stub.forward, transform=stub.transform)
    with pytest.raises(L.AclganError, match=r"odd\.png is 50x64 .*multiples of 4"):            # full_size alone still refuses ragged shapes
        TR.translate_folder(None, cfg, src, os.path.join(tmp_path, "o0"), forward=stub.forward, transform=stub.transform, full_size=True)
    assert stub.calls == [] and not os.path.exists(os.path.join(tmp_path, "o0"))
    rec = TR.translate_folder(None, cfg, src, os.path.join(tmp_path, "o1"), forward=stub.forward, transform=stub.transform, fit="pad")
    assert [s for _, s, _ in rec] == [(64, 64), (50, 64)]
    assert [c["kw"] for c in stub.calls] == [{"multiple": 4}, {"multiple": 4}] and [c["shape"] for c in stub.calls] == [(1, 64, 64), (1, 50, 64)]
    with Image.open(os.path.join(tmp_path, "o1", "_00_bar", "odd.png")) as im:
        assert im.size == (64, 50)
    stub = _Stub()
    TR.translate_folder(None, cfg, src, os.path.join(tmp_path, "o2"), max_images=1, forward=stub.forward, transform=stub.transform)
    assert [c["kw"] for c in stub.calls] == [{}]                    # switches off: the call of before, no keyword
    with pytest.raises(L.AclganError, match="stage"):               # full_size reads the staged sources: a bare callable cannot give them
        TR.translate_folder(None, cfg, src, os.path.join(tmp_path, "o3"), max_images=1, forward=stub.forward, transform=stub.transform, full_size=True)


# ---- (d) ----
def test_pad_argument_checks_return_before_any_launch():
    f = L.lib.aclgan_translate_pad
    p = C.c_void_p(0x1000)             # never dereferenced: every call below is refused by the checks in front of the launch
    ok = dict(src=p, bs=3 * 35, B=2, C=3, oh=5, ow=7, M=4, dst=p)

    def call(**over):
        a = dict(ok, **over)
        return f(a["src"], a["bs"], a["B"], a["C"], a["oh"], a["ow"], a["M"], a["dst"], None)

    for what, over in (("null src", dict(src=None)), ("null dst", dict(dst=None)), ("B = 0", dict(B=0)), ("C = 0", dict(C=0)), ("oh = 0", dict(oh=0)),
                       ("ow < 0", dict(ow=-7)), ("multiple = 0", dict(M=0)), ("height below the multiple", dict(oh=3)),
                       ("width below the multiple", dict(ow=7, M=8, oh=8)), ("negative stride", dict(bs=-1)), ("too many planes", dict(B=30000)),
                       ("too large", dict(oh=1 << 15, ow=1 << 15))):
        assert call(**over) == -1, what                    # ACLGAN_EINVAL
        assert "translate_pad" in L.last_error(), what


def test_paste_argument_checks_return_before_any_launch():
    f = L.lib.aclgan_translate_paste_u8
    p = C.c_void_p(0x1000)             # never dereferenced
    sizes = [(13, 29), (1, 1)]

    def descs(src_off=(0, 1131), out_off=(0, 1131), sz=sizes):
        d = (L.PasteDesc * 2)()
        for k in range(2):
            d[k].src_offset, d[k].out_offset, d[k].src_h, d[k].src_w = src_off[k], out_off[k], sz[k][0], sz[k][1]
        return d

    ok = dict(dec=p, dec_bs=4 * 64, ch=4, x=p, x_bs=3 * 64, B=2, oh=5, ow=7, PH=8, PW=8, src=p, src_bytes=1134, dh=descs(), dd=p, bar=p, mask=p,
              out_bytes=1134)

    def call(**over):
        a = dict(ok, **over)
        return f(a["dec"], a["dec_bs"], a["ch"], a["x"], a["x_bs"], a["B"], a["oh"], a["ow"], a["PH"], a["PW"], a["src"], a["src_bytes"], a["dh"],
                 a["dd"], a["bar"], a["mask"], a["out_bytes"], None)

    for what, over in (("null dec", dict(dec=None)), ("null x", dict(x=None)), ("null src", dict(src=None)), ("null host descriptors", dict(dh=None)),
                       ("null device descriptors", dict(dd=None)), ("no output", dict(bar=None, mask=None)), ("2 channels", dict(ch=2)),
                       ("5 channels", dict(ch=5)), ("B = 0", dict(B=0)), ("B too large", dict(B=1 << 20)), ("oh = 0", dict(oh=0)), ("ow < 0", dict(ow=-1)),
                       ("PH below oh", dict(PH=4)), ("PW below ow", dict(PW=4)), ("planes too large", dict(PH=1 << 15, PW=1 << 15)),
                       ("negative dec stride", dict(dec_bs=-4)), ("negative x stride", dict(x_bs=-4)),
                       ("source size 0", dict(dh=descs(sz=[(13, 29), (0, 1)]))), ("source too large", dict(dh=descs(sz=[(13, 29), (1 << 23, 1)]))),
                       ("negative source offset", dict(dh=descs(src_off=(-1, 1131)))), ("source past the buffer", dict(src_bytes=1133)),
                       ("source offset past the buffer", dict(dh=descs(src_off=(4, 1132)))), ("outputs overlap", dict(dh=descs(out_off=(0, 1130)))),
                       ("outputs do not ascend", dict(dh=descs(out_off=(3, 0)), out_bytes=4096)), ("negative output offset", dict(dh=descs(out_off=(-3, 1131)))),
                       ("output past the buffer", dict(out_bytes=1133))):
        assert call(**over) == -1, what                    # ACLGAN_EINVAL
        assert "translate_paste_u8" in L.last_error(), what


def test_device_paths_refuse_host_tensors():
    with pytest.raises(L.AclganError, match="no CPU path"):
        TR.reflect_pad(torch.zeros(1, 3, 5, 7), 4)
    with pytest.raises(L.AclganError, match="no CPU path"):
        TR.paste_u8(torch.zeros(1, 4, 8, 8), torch.zeros(1, 3, 8, 8), (5, 7), torch.zeros(3, dtype=torch.uint8), None)


# ---- (e) ----
def test_script_lists_the_new_flags():
    """translate_photos.py: every flag of test_batch.py (whose file stays as it is) and the two switches"""
    script = os.path.join(ROOT, "translate_photos.py")
    r = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--fit", "refuse", "pad", "--full_size", "--config", "--input_folder", "--output_folder", "--checkpoint", "--a2b", "--seed",
                 "--num_style", "--synchronized", "--output_only", "--batch_size", "--max_images"):
        assert flag in r.stdout, flag
    r = subprocess.run([sys.executable, script, "--fit", "stretch"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--fit" in r.stderr
    r = subprocess.run([sys.executable, script, "--fit", "pad", "--full_size"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--config is required" in r.stderr           # both switches parse; the run stops at the missing paths
