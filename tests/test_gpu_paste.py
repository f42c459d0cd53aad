"""Photographs at their own size on the GPU (csrc/paste.hip through acl-gan_amd/translate.py; translate_photos.py --fit pad / --full_size).  -m gpu

The kernels' bytes must EQUAL the fp32 model tests/paste_ref.py -- no tolerance, no excluded case or pixel; the padded floats must equal
the model bit for bit.  Every byte comparison prints the number of differing bytes and their largest difference before it asserts."""
import os

import numpy as np
import pytest
import torch

from oracle import aclgan_oracle as O
import paste_ref as P
import translate_ref as R

pytestmark = pytest.mark.gpu

IDS = lambda s: "%dx%d_in_%dx%d_to_%dx%d" % (s[0] + s[1] + s[2])


@pytest.fixture(scope="module")
def TR():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import aclgan_amd  # noqa: F401
    from aclgan_amd import translate
    return translate


def _same_bytes(got, want, what):
    got = np.asarray(got.cpu() if torch.is_tensor(got) else got)
    want = np.asarray(want)
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.shape, want.shape)
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print("%s: %d of %d bytes differ, largest difference %d" % (what, int((diff != 0).sum()), diff.size, int(diff.max()) if diff.size else 0))
    assert np.array_equal(got, want), what


def _stage(sources, lead=0):
    """the sources packed one after the other behind `lead` bytes, as GpuBatchTransform.stage packs them: (device buffer, [(offset, h, w)])"""
    parts, desc, off = [np.full(lead, 77, np.uint8)], [], lead
    for s in sources:
        desc.append((off, s.shape[0], s.shape[1]))
        parts.append(s.reshape(-1))
        off += s.size
    return torch.from_numpy(np.concatenate(parts)).cuda(), desc


def _run(TR, dec, x, valid, sources, lead=0, outputs=("bar", "mask")):
    """paste_u8 of a batch (dec, x: device tensors) -> per image {name: (Hs, Ws, 3) array}"""
    src, desc = _stage(sources, lead)
    plan = TR.paste_plan(desc, dec.device)
    got = TR.paste_u8(dec, x, valid, src, plan, outputs=outputs)
    torch.cuda.synchronize()
    res = []
    for k, (h, w) in enumerate(plan["sizes"]):
        o = plan["offsets"][k]
        res.append({n: got[n][o:o + h * w * 3].cpu().numpy().reshape(h, w, 3) for n in outputs})
    return res


# ---- 1. the paste kernel: bytes exact ----
@pytest.mark.parametrize("channels", [4, 3])
@pytest.mark.parametrize("shape", P.SHAPES, ids=IDS)
def test_paste_bytes_equal_the_model(TR, shape, channels):
    dec, x, valid, source = P.case(shape, channels)
    want_bar, want_mask = P.paste(dec, x, valid, source)
    for lead in (0, 1):                              # a row may start at any byte: both parities of the first one
        got, = _run(TR, torch.from_numpy(dec)[None].cuda(), torch.from_numpy(x)[None].cuda(), valid, [source], lead)
        _same_bytes(got["bar"], want_bar, "bar lead %d" % lead)
        _same_bytes(got["mask"], want_mask, "mask lead %d" % lead)
    only, = _run(TR, torch.from_numpy(dec)[None].cuda(), torch.from_numpy(x)[None].cuda(), valid, [source], outputs=("bar",))
    _same_bytes(only["bar"], want_bar, "bar alone")


def _batch_of_three(channels):
    """three images of equal (oh, ow) = (16, 22) in (16, 24) planes and three source sizes"""
    shapes = [((16, 22), (16, 24), hw) for hw in ((21, 30), (42, 60), (7, 101))]
    cases = [P.case(s, channels, seed=k + 1) for k, s in enumerate(shapes)]
    dec = torch.from_numpy(np.stack([c[0] for c in cases]))
    x = torch.from_numpy(np.stack([c[1] for c in cases]))
    return dec, x, (16, 22), [c[3] for c in cases]


@pytest.mark.parametrize("channels", [4, 3])
def test_image_bytes_do_not_depend_on_the_batch(TR, channels):
    dec, x, valid, sources = _batch_of_three(channels)
    both = _run(TR, dec.cuda(), x.cuda(), valid, sources)
    for i in range(3):
        alone, = _run(TR, dec[i:i + 1].cuda(), x[i:i + 1].cuda(), valid, sources[i:i + 1])
        want = P.paste(dec[i].numpy(), x[i].numpy(), valid, sources[i])
        for n, w in zip(("bar", "mask"), want):
            _same_bytes(alone[n], both[i][n], "image %d %s alone / in the batch" % (i, n))
            _same_bytes(both[i][n], w, "image %d %s against the model" % (i, n))


def test_paste_batch_and_channel_slices_without_a_copy(TR):
    """dec a batch slice [::2] of a larger tensor, x a channel slice, and 3 of 4 decoder channels: read through their strides"""
    from aclgan_amd import visual
    dec, x, valid, sources = _batch_of_three(4)
    big = torch.zeros(6, 4, 16, 24)
    big[::2] = dec
    big[1::2] = dec.flip(0)
    wide = torch.zeros(3, 4, 16, 24)
    wide[:, 1:4] = x
    big, wide = big.cuda(), wide.cuda()
    d, g = big[::2], wide[:, 1:4]
    assert not d.is_contiguous() and not g.is_contiguous()
    assert visual._dense(d).data_ptr() == d.data_ptr() and visual._dense(g).data_ptr() == g.data_ptr()
    got = _run(TR, d, g, valid, sources)
    plain = _run(TR, d[:, :3], g, valid, sources)
    for i in range(3):
        for n, w in zip(("bar", "mask"), P.paste(dec[i].numpy(), x[i].numpy(), valid, sources[i])):
            _same_bytes(got[i][n], w, "slices image %d %s" % (i, n))
        for n, w in zip(("bar", "mask"), P.paste(dec[i, :3].numpy(), x[i].numpy(), valid, sources[i])):
            _same_bytes(plain[i][n], w, "slices, 3 of 4 channels, image %d %s" % (i, n))


# ---- 2. closed mask ----
@pytest.mark.parametrize("shape", P.SHAPES, ids=IDS)
def test_closed_mask_returns_the_source_bytes(TR, shape):
    dec, x, valid, source = P.case(shape, 4)
    dec[3] = -1.0
    got, = _run(TR, torch.from_numpy(dec)[None].cuda(), torch.from_numpy(x)[None].cuda(), valid, [source], lead=3)
    _same_bytes(got["bar"], source, "bar under a closed mask")
    assert int(got["mask"].max()) == 0


# ---- 3. the pad kernel: bits exact ----
@pytest.mark.parametrize("shape", [(5, 7), (16, 22), (55, 16), (8, 12)], ids=lambda s: "%dx%d" % s)
def test_pad_bits_equal_the_model(TR, shape):
    oh, ow = shape
    rng = np.random.RandomState(oh * 100 + ow)
    x = (rng.rand(3, 3, oh, ow) * 2 - 1).astype(np.float32)
    x.view(np.uint32)[0, 0, 0, :3] = (0x7fc00001, 0xff800000, 0x80000000)      # a NaN with a payload, -Inf, -0: copied, not computed with
    want = P.reflect_pad(x, 4)
    assert want.shape[2:] == {(5, 7): (8, 8), (16, 22): (16, 24), (55, 16): (56, 16), (8, 12): (8, 12)}[shape]
    got = TR.reflect_pad(torch.from_numpy(x).cuda(), 4)
    assert tuple(got.shape) == want.shape and got.is_contiguous()
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    wide = torch.zeros(3, 4, oh, ow)
    wide[:, 1:4] = torch.from_numpy(x)
    sl = TR.reflect_pad(wide.cuda()[:, 1:4][::2], 4)                            # a channel slice of every other image: read through its stride
    assert np.array_equal(sl.cpu().numpy().view(np.uint32), want[::2].view(np.uint32))
    one = TR.reflect_pad(torch.from_numpy(x[:1, :1]).cuda(), 4)
    assert np.array_equal(one.cpu().numpy().view(np.uint32), want[:1, :1].view(np.uint32))


# ---- 4. the folder, end to end ----
FILES = [("p0.png", 30, 21), ("p1.png", 60, 42), ("q0.png", 16, 16), ("r0.png", 9, 31)]      # (name, width, height)
RESIZED = {"p0.png": (16, 22), "p1.png": (16, 22), "q0.png": (16, 16), "r0.png": (55, 16)}    # after Resize(16), H x W
NET = {"p0.png": (16, 24), "p1.png": (16, 24), "q0.png": (16, 16), "r0.png": (56, 16)}


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    from PIL import Image
    src = str(tmp_path_factory.mktemp("paste_in"))
    yy, xx = np.mgrid[0:64, 0:64]
    rng = np.random.RandomState(6)
    for k, (name, w, h) in enumerate(FILES):
        base = np.stack([(xx[:h, :w] * (7 + k)) % 256, (yy[:h, :w] * 5 + 30 * k) % 256, ((xx[:h, :w] + yy[:h, :w]) * 3) % 256], -1)
        Image.fromarray(((base + rng.randint(0, 40, (h, w, 3))) % 256).astype(np.uint8)).save(os.path.join(src, name))
    return src


@pytest.fixture(scope="module")
def folder_trainer(TR):
    from aclgan_amd import trainer as T
    cfg = O.default_config()
    cfg["gen"].update(dim=8, mlp_dim=16, n_res=1)
    cfg["dis"].update(dim=8)
    cfg["display_size"] = 2
    cfg["new_size"] = 16
    assert cfg["gen"]["n_downsample"] == 2 and cfg["focus_loss"] > 0
    tr = T.aclgan_Trainer(cfg)
    nets = O.test_nets(cfg, 6)
    for name in O.OracleTrainer.NETS:
        getattr(tr, name).load_state_dict(nets[name], strict=False)
    return tr, cfg


def _png(path):
    from PIL import Image
    with Image.open(path) as im:
        assert im.format == "PNG" and im.mode == "RGB"
        return np.asarray(im).copy()


def _tree(root):
    """{relative path: file bytes} of everything under root"""
    out = {}
    for d, _, names in os.walk(root):
        for n in names:
            p = os.path.join(d, n)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


@pytest.fixture(scope="module")
def runs(TR, folder, folder_trainer, tmp_path_factory):
    """every folder run the tests below compare, once: {(mode, batch_size): (records, floats, output folder)}"""
    tr, cfg = folder_trainer
    base = str(tmp_path_factory.mktemp("paste_out"))
    res = {}
    for mode, kw in (("full", dict(fit="pad", full_size=True)), ("pad", dict(fit="pad"))):
        for bs in (3, 1):
            out = os.path.join(base, "%s_b%d" % (mode, bs))
            torch.manual_seed(3)
            rec, floats = TR.translate_folder(tr, cfg, folder, out, a2b=True, num_style=2, batch_size=bs, keep_float=True, **kw)
            res[(mode, bs)] = (rec, floats, out)
    return res


def _check_records(rec, floats, bs):
    names = [f[0] for f in FILES]
    assert [os.path.basename(p) for p, _, _ in rec] == names
    assert [s for _, s, _ in rec] == [RESIZED[n] for n in names]
    assert [b for _, _, b in rec] == ([0, 0, 1, 2] if bs == 3 else [0, 1, 2, 3])      # p0 and p1 share a batch
    for p, _, _ in rec:
        n, f = os.path.basename(p), floats[p]
        assert f["valid"] == RESIZED[n] and tuple(f["input"].shape) == (3,) + NET[n] and all(tuple(d.shape) == (4,) + NET[n] for d in f["dec"])


def test_folder_full_size_against_the_model(folder, runs):
    from PIL import Image
    rec, floats, out = runs[("full", 3)]
    _check_records(rec, floats, 3)
    assert sorted(os.listdir(out)) == sorted(["_00_bar", "_00_mask", "_01_bar", "_01_mask"] + ["input%03d.jpg" % i for i in range(4)])
    for i, (path, _, _) in enumerate(rec):
        name, f = os.path.basename(path), floats[path]
        source = _png(path)
        assert source.shape == (FILES[i][2], FILES[i][1], 3)
        for j in range(2):
            want = P.paste(f["dec"][j].numpy(), f["input"].numpy(), f["valid"], source)
            for kind, w in zip(("bar", "mask"), want):
                got = _png(os.path.join(out, "_%02d_%s" % (j, kind), name))
                _same_bytes(got, w, "%s style %d %s" % (name, j, kind))
        assert not torch.equal(f["dec"][0], f["dec"][1])
        with Image.open(os.path.join(out, "input%03d.jpg" % i)) as im:      # the decoded source, at its own size
            assert im.format == "JPEG" and im.size == (FILES[i][1], FILES[i][2])
    # the padding is what the header says: the net input is the reflect pad of its own valid region
    f = floats[rec[0][0]]
    oh, ow = f["valid"]
    assert np.array_equal(f["input"].numpy().view(np.uint32), P.reflect_pad(f["input"].numpy()[:, :oh, :ow], 4).view(np.uint32))


def test_folder_pad_alone_writes_the_crop_of_the_existing_rule(runs):
    from PIL import Image
    rec, floats, out = runs[("pad", 3)]
    _check_records(rec, floats, 3)
    for i, (path, (oh, ow), _) in enumerate(rec):
        name, f = os.path.basename(path), floats[path]
        for j in range(2):
            want = R.ref_finish_u8(f["dec"][j][None, :, :oh, :ow], f["input"][None, :, :oh, :ow])
            for kind in ("bar", "mask"):
                got = _png(os.path.join(out, "_%02d_%s" % (j, kind), name))
                _same_bytes(got, want[kind][0].numpy(), "%s style %d %s" % (name, j, kind))
        with Image.open(os.path.join(out, "input%03d.jpg" % i)) as im:
            assert im.format == "JPEG" and im.size == (ow, oh)


@pytest.mark.parametrize("mode", ["full", "pad"])
def test_folder_files_do_not_depend_on_the_batch_size(runs, mode):
    a, b = _tree(runs[(mode, 3)][2]), _tree(runs[(mode, 1)][2])
    _check_records(runs[(mode, 1)][0], runs[(mode, 1)][1], 1)
    assert sorted(a) == sorted(b) and len(a) == 4 * 5
    differ = [n for n in sorted(a) if a[n] != b[n]]
    print("%s: %d of %d files differ between batch_size 3 and 1 %s" % (mode, len(differ), len(a), differ))
    assert not differ


def test_folder_refuses_ragged_files_without_fit_pad(TR, folder, folder_trainer, tmp_path):
    from aclgan_amd import _lib as L
    tr, cfg = folder_trainer
    for kw in ({}, {"full_size": True}):
        out = os.path.join(tmp_path, "o")
        with pytest.raises(L.AclganError, match=r"p0\.png is 16x22 .*multiples of 4"):
            TR.translate_folder(tr, cfg, folder, out, **kw)
        assert not os.path.exists(out)
