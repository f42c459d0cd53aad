"""Folder translation (acl-gan_amd/translate.py, csrc/finish.hip, test_batch.py): everything that needs no GPU.

(a) tests/translate_ref.py -- the model the kernels are held to byte for byte in tests/test_gpu_translate_batch.py -- against the host path
    the project already ships: test.focus_translation -> (o + 1) / 2 -> test.save_image, through a PNG (lossless);
(b) the folder driver's planning with stub device halves: order, grouping, cap, paths, style draws, refusals;
(c) the argument checks of aclgan_translate_finish_u8, which return before any launch;
(d) test_batch.py's flags."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import translate_ref as R

import aclgan_amd  # noqa: F401
from aclgan_amd import _lib as L
from aclgan_amd import translate as TR

test_py = R.test_script()


# ---- (a) ----
def _boundary_values():
    """values whose normalised, scaled result falls on or next to k and k + 0.5 (where truncation after + 0.5 changes the byte), in [-1, 1]"""
    k = torch.arange(0, 511, dtype=torch.float32) / 510          # k / 255 and (k + 0.5) / 255 in [0, 1]
    v = torch.cat([k, torch.nextafter(k, torch.tensor(2.0)), torch.nextafter(k, torch.tensor(-2.0))]).clamp(0, 1)
    return v * 2 - 1


def _cases():
    g = torch.Generator().manual_seed(7)
    rnd = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    cases = [("random 4ch", rnd(2, 4, 9, 13), rnd(2, 3, 9, 13)),
             ("random 3ch", rnd(2, 3, 9, 13), rnd(2, 3, 9, 13)),
             ("wide range", rnd(1, 4, 8, 8) * 37, rnd(1, 3, 8, 8) * 0.001),
             ("constant", torch.full((1, 4, 5, 6), 0.25), torch.full((1, 3, 5, 6), -0.75))]
    b = _boundary_values()
    n = b.numel()                                                 # 1533 = 3 * 511 = 7 * 219
    cases.append(("boundaries 4ch", torch.cat([b.view(1, 3, 7, 73), b[:511].view(1, 1, 7, 73)], 1), b.flip(0).view(1, 3, 7, 73)))
    cases.append(("boundaries 3ch", b.view(1, 3, 7, 73), b.view(1, 3, 7, 73)))
    assert n == 1533
    return cases


def _host_path_bytes(t, path):
    from PIL import Image
    test_py.save_image(t, path)
    return torch.from_numpy(np.asarray(Image.open(path)).copy())


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c[0].replace(" ", "_"))
def test_model_equals_the_shipped_host_path(case, tmp_path):
    name, dec, bg = case
    got = R.ref_finish_u8(dec, bg)
    path = os.path.join(tmp_path, "p.png")
    for i in range(dec.shape[0]):
        d, x = dec[i:i + 1], bg[i:i + 1]
        if dec.shape[1] == 4:
            img, mask = d.split(3, 1)
            bar = (test_py.focus_translation(img, x, mask) + 1) / 2.0
            assert torch.equal(got["mask"][i], _host_path_bytes(mask.expand(-1, 3, -1, -1), path)), name
        else:
            assert "mask" not in got
            bar = (d[:, :3] + 1) / 2.0
        assert torch.equal(got["bar"][i], _host_path_bytes(bar, path)), name
        assert torch.equal(got["input"][i], _host_path_bytes(x, path)), name
    if name == "constant":         # hi == lo: (x - lo) / 1e-5 = 0 everywhere
        assert all(int(v.max()) == 0 for v in got.values())
    if name.startswith("boundaries"):
        assert len(torch.unique(got["input"])) == 256


def test_model_ranges_are_per_image_and_per_picture():
    g = torch.Generator().manual_seed(8)
    dec = torch.rand(3, 4, 6, 10, generator=g) * 2 - 1
    bg = torch.rand(3, 3, 6, 10, generator=g) * 2 - 1
    scale = torch.tensor([1e-3, 1.0, 50.0]).view(3, 1, 1, 1)
    both = R.ref_finish_u8(dec * scale, bg * scale)
    for i in range(3):
        alone = R.ref_finish_u8(dec[i:i + 1] * scale[i], bg[i:i + 1] * scale[i])
        for n in ("bar", "mask", "input"):
            assert torch.equal(both[n][i], alone[n][0])
            assert int(both[n][i].min()) == 0 and int(both[n][i].max()) >= 240


# ---- (b) ----
class _Stub:
    """the device halves of translate_folder on the CPU: a host transform and a forward that records what it was given"""

    def __init__(self, new_size, focus):
        self.new_size, self.focus, self.calls = new_size, focus, []

    def transform(self, images):
        import numpy as _np
        ts = []
        for im in images:
            im = test_py.resize_smaller_edge(im, self.new_size)
            ts.append(torch.from_numpy(_np.asarray(im, dtype=_np.uint8).copy()).permute(2, 0, 1).float().div(255.0))
        return torch.stack(ts)

    def forward(self, trainer, images, styles, a2b, with_input):
        B, _, H, W = images.shape
        S = styles.shape[1]
        P = S * (2 if self.focus else 1) + (1 if with_input else 0)
        self.calls.append({"shape": (B, H, W), "styles": styles.clone(), "a2b": a2b})
        buf = torch.empty(P, B, H, W, 3, dtype=torch.uint8)
        for p in range(P):
            for k in range(B):
                buf[p, k] = 10 * p + k
        return {"bytes": buf, "dec": [torch.zeros(B, 4 if self.focus else 3, H, W) for _ in range(S)], "images": images}


def _config(focus=True, new_size=48):
    return {"gen": {"n_downsample": 2, "style_dim": 8}, "focus_loss": 1 if focus else 0, "new_size": new_size}


SIZES = [("a0.png", 128, 96), ("a1.png", 128, 96), ("b0.png", 64, 64), ("c0.png", 128, 96), ("c1.png", 128, 96), ("c2.png", 128, 96),
         ("d0.jpg", 64, 64)]          # (name, width, height): Resize(48) -> 48x64 (H x W) and 48x48


def _folder(tmp_path, sizes=SIZES):
    from PIL import Image
    src = os.path.join(tmp_path, "in")
    os.makedirs(src)
    rng = np.random.RandomState(3)
    for name, w, h in sizes:
        Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(os.path.join(src, name))
    return src


def _run(tmp_path, src, name, focus=True, **kw):
    stub = _Stub(kw.pop("new_size", 48), focus)
    out = os.path.join(tmp_path, name)
    cfg = _config(focus, stub.new_size)
    rec = TR.translate_folder(None, cfg, src, out, forward=stub.forward, transform=stub.transform, **kw)
    return rec, stub, out


def test_folder_order_grouping_and_cap(tmp_path):
    src = _folder(tmp_path)
    rec, stub, _ = _run(tmp_path, src, "o1", batch_size=2)
    assert [os.path.basename(p) for p, _, _ in rec] == [s[0] for s in SIZES]
    assert [s for _, s, _ in rec] == [(48, 64), (48, 64), (48, 48), (48, 64), (48, 64), (48, 64), (48, 48)]
    # a0 a1 | b0 (shape change) | c0 c1 (full) | c2 | d0 (shape change)
    assert [b for _, _, b in rec] == [0, 0, 1, 2, 2, 3, 4]
    assert [c["shape"] for c in stub.calls] == [(2, 48, 64), (1, 48, 48), (2, 48, 64), (1, 48, 64), (1, 48, 48)]
    rec, stub, _ = _run(tmp_path, src, "o2", batch_size=5)
    assert [b for _, _, b in rec] == [0, 0, 1, 2, 2, 2, 3]
    rec, stub, _ = _run(tmp_path, src, "o3", batch_size=2, max_images=4)
    assert [os.path.basename(p) for p, _, _ in rec] == ["a0.png", "a1.png", "b0.png", "c0.png"]
    rec, _, _ = _run(tmp_path, src, "o4", batch_size=2, max_images=0)
    assert len(rec) == len(SIZES)
    assert all(c["a2b"] is True for c in stub.calls)
    rec, stub, _ = _run(tmp_path, src, "o5", batch_size=3, a2b=False)
    assert all(c["a2b"] is False for c in stub.calls)


@pytest.mark.parametrize("focus", [True, False], ids=["focus", "plain"])
def test_folder_output_paths_two_styles(tmp_path, focus):
    from PIL import Image
    src = _folder(tmp_path)
    _, _, out = _run(tmp_path, src, "out", focus=focus, batch_size=2, num_style=2)
    dirs = ["_00_bar", "_01_bar"] + (["_00_mask", "_01_mask"] if focus else [])
    inputs = ["input%03d.jpg" % i for i in range(len(SIZES))]
    assert sorted(os.listdir(out)) == sorted(dirs + inputs)
    for d in dirs:
        assert sorted(os.listdir(os.path.join(out, d))) == sorted(s[0] for s in SIZES)
    per = 2 if focus else 1
    # the stub's bytes: picture p of batch element k holds 10 p + k; c1.png is element 1 of its batch
    for j in range(2):
        assert int(np.asarray(Image.open(os.path.join(out, "_%02d_bar" % j, "c1.png")))[0, 0, 0]) == 10 * (j * per) + 1
        if focus:
            assert int(np.asarray(Image.open(os.path.join(out, "_%02d_mask" % j, "c1.png")))[0, 0, 0]) == 10 * (j * per + 1) + 1
    with Image.open(os.path.join(out, "_01_bar", "a0.png")) as im:
        assert im.size == (64, 48) and im.format == "PNG"
    with Image.open(os.path.join(out, "_00_bar", "d0.jpg")) as im:
        assert im.size == (48, 48) and im.format == "JPEG"
    with Image.open(os.path.join(out, "input002.jpg")) as im:
        assert im.size == (48, 48) and im.format == "JPEG"
    _, _, out = _run(tmp_path, src, "out_only", focus=focus, batch_size=2, num_style=1, output_only=True)
    assert sorted(os.listdir(out)) == (["_00_bar", "_00_mask"] if focus else ["_00_bar"])


@pytest.mark.parametrize("batch_size", [1, 2, 5])
def test_folder_styles_equal_a_per_image_loop(tmp_path, batch_size):
    src = _folder(tmp_path)
    S, sd, n = 2, 8, len(SIZES)
    torch.manual_seed(5)
    fixed = torch.randn(S * 3, sd, 1, 1)
    want = []
    for _ in range(n):
        s = torch.randn(S * 3, sd, 1, 1) * 2
        want.append(torch.stack([s[j * 3] for j in range(S)]))
    torch.manual_seed(5)
    _, stub, _ = _run(tmp_path, src, "a", batch_size=batch_size, num_style=S)
    got = torch.cat([c["styles"] for c in stub.calls])
    assert tuple(got.shape) == (n, S, sd, 1, 1) and torch.equal(got, torch.stack(want))
    torch.manual_seed(5)
    _, stub, _ = _run(tmp_path, src, "b", batch_size=batch_size, num_style=S, synchronized=True)
    got = torch.cat([c["styles"] for c in stub.calls])
    assert torch.equal(got, torch.stack([(fixed * 2)[0::3]] * n))


def test_folder_refusals(tmp_path):
    src = _folder(tmp_path, [("fine.png", 64, 64), ("odd.png", 64, 50)])
    stub = _Stub(48, True)
    cfg = _config(True)
    del cfg["new_size"]
    cfg.update(new_size_a=48, new_size_b=50)      # a2b reads new_size_a, as test.py does
    rec = TR.translate_folder(None, cfg, src, os.path.join(tmp_path, "fine"), max_images=1, forward=stub.forward, transform=stub.transform)
    assert [s for _, s, _ in rec] == [(48, 48)]
    stub = _Stub(None, True)
    with pytest.raises(L.AclganError, match=r"odd\.png is 50x64 .*multiples of 4"):      # no Resize: 50 x 64 as it is, under n_downsample 2
        TR.translate_folder(None, _config(True, None), src, os.path.join(tmp_path, "o"), forward=stub.forward, transform=stub.transform)
    assert stub.calls == [] and not os.path.exists(os.path.join(tmp_path, "o"))      # refused before anything ran or was written
    empty = os.path.join(tmp_path, "empty")
    os.makedirs(empty)
    open(os.path.join(empty, "notes.txt"), "w").close()
    with pytest.raises(L.AclganError, match="no images"):
        TR.translate_folder(None, _config(), empty, os.path.join(tmp_path, "o"), forward=stub.forward, transform=stub.transform)
    with pytest.raises(L.AclganError, match="no images"):
        TR.translate_folder(None, _config(), os.path.join(tmp_path, "missing"), os.path.join(tmp_path, "o"), forward=stub.forward,
                            transform=stub.transform)
    with pytest.raises(L.AclganError, match="batch_size"):
        TR.translate_folder(None, _config(), src, os.path.join(tmp_path, "o"), batch_size=0, forward=stub.forward, transform=stub.transform)


# ---- (c) ----
def test_finish_argument_checks_return_before_any_launch():
    f = L.lib.aclgan_translate_finish_u8
    p = C.c_void_p(0x1000)             # never dereferenced: every call below is refused by the checks in front of the launches
    ok = dict(dec=p, dec_bs=4 * 64, ch=4, bg=p, bg_bs=3 * 64, B=2, H=8, W=8, bar=p, mask=p, inp=p, scratch=p)

    def call(**over):
        a = dict(ok, **over)
        return f(a["dec"], a["dec_bs"], a["ch"], a["bg"], a["bg_bs"], a["B"], a["H"], a["W"], a["bar"], a["mask"], a["inp"], a["scratch"], None)

    for what, over in (("null dec", dict(dec=None)), ("null scratch", dict(scratch=None)), ("no output", dict(bar=None, mask=None, inp=None)),
                       ("2 channels", dict(ch=2)), ("5 channels", dict(ch=5)), ("4 channels without bg", dict(bg=None, inp=None)),
                       ("input picture without bg", dict(ch=3, bg=None, mask=None)), ("mask without a focus channel", dict(ch=3)),
                       ("H = 0", dict(H=0)), ("W < 0", dict(W=-3)), ("B = 0", dict(B=0)), ("B too large", dict(B=1 << 20)),
                       ("H W too large", dict(H=1 << 15, W=1 << 15)), ("negative stride", dict(dec_bs=-4))):
        assert call(**over) == -1, what                    # ACLGAN_EINVAL
        assert "translate_finish_u8" in L.last_error(), what
    assert L.lib.aclgan_translate_finish_scratch_bytes(4) == 4 * 6 * 4
    assert L.lib.aclgan_translate_finish_scratch_bytes(0) == 0


def test_finish_u8_refuses_host_tensors():
    with pytest.raises(L.AclganError, match="no CPU path"):
        TR.finish_u8(torch.zeros(1, 4, 8, 8), torch.zeros(1, 3, 8, 8))


# ---- (d) ----
def test_script_lists_the_reference_flags():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "test_batch.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--config", "--input_folder", "--output_folder", "--checkpoint", "--a2b", "--seed", "--num_style", "--synchronized",
                 "--output_only", "--output_path", "--trainer", "--compute_IS", "--compute_CIS", "--batch_size", "--max_images"):
        assert flag in r.stdout, flag
    r = subprocess.run([sys.executable, os.path.join(ROOT, "test_batch.py"), "--compute_IS"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "Inception" in r.stderr
