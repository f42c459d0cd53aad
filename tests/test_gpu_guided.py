"""Guided-filter upsampling of the edit on the GPU (csrc/guided.hip through acl-gan_amd/translate.py: guided_u8; translate_folder(detail=
'guided')).  -m gpu

The coefficient planes must equal the fp32 model tests/guided_ref.py bit for bit, and the bytes must EQUAL it -- no tolerance, no excluded
case or pixel.  Every comparison prints the number of differing elements and their largest difference before it asserts."""
import os

import numpy as np
import pytest
import torch

from oracle import aclgan_oracle as O
import guided_ref as G
import paste_ref as P

pytestmark = pytest.mark.gpu

IDS = lambda s: "%dx%d_in_%dx%d_to_%dx%d" % (s[0] + s[1] + s[2])
RADII = [1, 2, 5]                           # 5 is wider than the 4x4 regions: the window is the whole region
EPS = 1e-3


@pytest.fixture(scope="module")
def TR():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import aclgan_amd  # noqa: F401
    from aclgan_amd import translate
    assert hasattr(translate, "guided_u8")
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


def _run(TR, dec, x, valid, sources, radius, lead=0, outputs=("bar", "mask"), eps=EPS):
    """guided_u8 of a batch (dec, x: device tensors) -> per image {name: (Hs, Ws, 3) array}"""
    src, desc = _stage(sources, lead)
    plan = TR.paste_plan(desc, dec.device)
    got = TR.guided_u8(dec, x, valid, src, plan, radius=radius, eps=eps, outputs=outputs)
    torch.cuda.synchronize()
    res = []
    for k, (h, w) in enumerate(plan["sizes"]):
        o = plan["offsets"][k]
        res.append({n: got[n][o:o + h * w * 3].cpu().numpy().reshape(h, w, 3) for n in outputs})
    return res


def _coef(dec, x, valid, radius, eps=EPS):
    """aclgan_translate_guided_coef of a dense batch -> host array (B, 7 | 6, oh, ow)"""
    from aclgan_amd import _lib as L
    B, Cd, PH, PW = dec.shape
    oh, ow = valid
    coef = torch.full((B, 7 if Cd == 4 else 6, oh, ow), float("nan"), device=dec.device)
    scratch = torch.empty(L.lib.aclgan_translate_guided_scratch_bytes(B, oh, ow, radius), dtype=torch.uint8, device=dec.device)
    L.check(L.lib.aclgan_translate_guided_coef(L.ptr(dec), dec.stride(0), Cd, L.ptr(x), x.stride(0), B, oh, ow, PH, PW, radius, eps, L.ptr(coef),
                                               L.ptr(scratch), L.stream_ptr(dec.device)), "translate_guided_coef")
    torch.cuda.synchronize()
    return coef.cpu().numpy()


# ---- 1. the coefficient planes: bits exact ----
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("channels", [4, 3])
@pytest.mark.parametrize("shape", G.SHAPES, ids=IDS)
def test_coefficient_planes_equal_the_model_bit_for_bit(TR, shape, channels, radius):
    dec, x, valid, _ = G.case(shape, channels)
    want = G.planes(dec, x, valid, radius, EPS)
    got = _coef(torch.from_numpy(dec)[None].cuda(), torch.from_numpy(x)[None].cuda(), valid, radius)[0]
    assert got.shape == want.shape and want.dtype == np.float32
    differ = got.view(np.uint32) != want.view(np.uint32)
    print("coefficient planes: %d of %d floats differ, largest difference %g" % (int(differ.sum()), differ.size, float(np.abs(got - want).max())))
    assert not differ.any()


def test_coefficient_planes_across_tiles_and_at_the_widest_window(TR):
    """a region of several 16 x 32 tiles with ragged edges, at radius 16 (the halo spans more than a tile) and at the default"""
    rng = np.random.RandomState(11)
    valid, (PH, PW) = (37, 70), (40, 72)
    dec = np.tanh(rng.randn(2, 4, PH, PW) * 1.5).astype(np.float32)
    x = (rng.rand(2, 3, PH, PW) * 2 - 1).astype(np.float32)
    for radius, eps in ((16, 1e-6), (4, EPS), (1, 1.0)):
        got = _coef(torch.from_numpy(dec).cuda(), torch.from_numpy(x).cuda(), valid, radius, eps)
        for i in range(2):
            want = G.planes(dec[i], x[i], valid, radius, eps)
            differ = got[i].view(np.uint32) != want.view(np.uint32)
            print("radius %d image %d: %d of %d floats differ" % (radius, i, int(differ.sum()), differ.size))
            assert not differ.any()


# ---- 2. the bytes: exact ----
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("channels", [4, 3])
@pytest.mark.parametrize("shape", G.SHAPES, ids=IDS)
def test_guided_bytes_equal_the_model(TR, shape, channels, radius):
    dec, x, valid, source = G.case(shape, channels)
    want_bar, want_mask = G.guided(dec, x, valid, source, radius, EPS)
    outputs = ("bar", "mask") if channels == 4 else ("bar",)       # no m plane without a focus plane: the mask picture is refused
    d, g = torch.from_numpy(dec)[None].cuda(), torch.from_numpy(x)[None].cuda()
    for lead in (0, 1):                              # a row may start at any byte: both parities of the first one
        got, = _run(TR, d, g, valid, [source], radius, lead, outputs)
        _same_bytes(got["bar"], want_bar, "bar lead %d" % lead)
        if channels == 4:
            _same_bytes(got["mask"], want_mask, "mask lead %d" % lead)
            _same_bytes(got["mask"], P.paste(dec, x, valid, source)[1], "mask against the paste's")
    if channels == 4:
        only, = _run(TR, d, g, valid, [source], radius, outputs=("bar",))
        _same_bytes(only["bar"], want_bar, "bar alone")
        only, = _run(TR, d, g, valid, [source], radius, outputs=("mask",))
        _same_bytes(only["mask"], want_mask, "mask alone")
    else:
        from aclgan_amd import _lib as L
        with pytest.raises(L.AclganError, match="m plane"):
            _run(TR, d, g, valid, [source], radius, outputs=("bar", "mask"))


def _batch_of_three(channels):
    """three images of equal (oh, ow) = (16, 22) in (16, 24) planes; source widths 30, 61, 101 behind a lead of 1: with 3 bytes a pixel the
    rows of the three start at every phase of a dword"""
    shapes = [((16, 22), (16, 24), hw) for hw in ((21, 30), (42, 61), (7, 101))]
    cases = [G.case(s, channels, seed=k + 1) for k, s in enumerate(shapes)]
    dec = torch.from_numpy(np.stack([c[0] for c in cases]))
    x = torch.from_numpy(np.stack([c[1] for c in cases]))
    return dec, x, (16, 22), [c[3] for c in cases]


@pytest.mark.parametrize("channels", [4, 3])
def test_image_bytes_do_not_depend_on_the_batch(TR, channels):
    dec, x, valid, sources = _batch_of_three(channels)
    names = ("bar", "mask") if channels == 4 else ("bar",)
    starts, off = set(), 1
    for s in sources:
        starts |= {(off + y * s.shape[1] * 3) % 4 for y in range(s.shape[0])}
        off += s.size
    assert starts == {0, 1, 2, 3}
    both = _run(TR, dec.cuda(), x.cuda(), valid, sources, 2, lead=1, outputs=names)
    for i in range(3):
        alone, = _run(TR, dec[i:i + 1].cuda(), x[i:i + 1].cuda(), valid, sources[i:i + 1], 2, outputs=names)
        want = G.guided(dec[i].numpy(), x[i].numpy(), valid, sources[i], 2, EPS)
        for n, w in zip(names, want):
            _same_bytes(alone[n], both[i][n], "image %d %s alone / in the batch" % (i, n))
            _same_bytes(both[i][n], w, "image %d %s against the model" % (i, n))


def test_guided_batch_and_channel_slices_without_a_copy(TR):
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
    got = _run(TR, d, g, valid, sources, 2)
    plain = _run(TR, d[:, :3], g, valid, sources, 2, outputs=("bar",))
    for i in range(3):
        for n, w in zip(("bar", "mask"), G.guided(dec[i].numpy(), x[i].numpy(), valid, sources[i], 2, EPS)):
            _same_bytes(got[i][n], w, "slices image %d %s" % (i, n))
        _same_bytes(plain[i]["bar"], G.guided(dec[i, :3].numpy(), x[i].numpy(), valid, sources[i], 2, EPS)[0], "slices, 3 of 4 channels, image %d" % i)


# ---- 3. closed mask ----
@pytest.mark.parametrize("radius", [1, 5])
@pytest.mark.parametrize("shape", G.SHAPES, ids=IDS)
def test_closed_mask_returns_the_source_bytes(TR, shape, radius):
    dec, x, valid, source = G.case(shape, 4)
    dec[3] = -1.0
    got, = _run(TR, torch.from_numpy(dec)[None].cuda(), torch.from_numpy(x)[None].cuda(), valid, [source], radius, lead=3)
    _same_bytes(got["bar"], source, "bar under a closed mask")
    assert int(got["mask"].max()) == 0


# ---- 4. the folder, end to end ----
FILES = [("p0.png", 30, 21), ("p1.png", 60, 42), ("q0.png", 16, 16), ("r0.png", 9, 31)]      # (name, width, height)
RADIUS = 2


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    from PIL import Image
    src = str(tmp_path_factory.mktemp("guided_in"))
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
    """every folder run the tests below compare, once: {name: (records, floats, output folder)}"""
    tr, cfg = folder_trainer
    base = str(tmp_path_factory.mktemp("guided_out"))
    res = {}
    for name, kw in (("guided_b3", dict(detail="guided", guided_radius=RADIUS, batch_size=3)),
                     ("guided_b1", dict(detail="guided", guided_radius=RADIUS, batch_size=1)),
                     ("bilinear_b3", dict(detail="bilinear", batch_size=3)), ("default_b3", dict(batch_size=3))):
        out = os.path.join(base, name)
        torch.manual_seed(3)
        rec, floats = TR.translate_folder(tr, cfg, folder, out, a2b=True, num_style=2, keep_float=True, fit="pad", full_size=True, **kw)
        res[name] = (rec, floats, out)
    return res


def test_folder_guided_against_the_model(folder, runs):
    rec, floats, out = runs["guided_b3"]
    assert [os.path.basename(p) for p, _, _ in rec] == [f[0] for f in FILES] and [b for _, _, b in rec] == [0, 0, 1, 2]
    assert sorted(os.listdir(out)) == sorted(["_00_bar", "_00_mask", "_01_bar", "_01_mask"] + ["input%03d.jpg" % i for i in range(4)])
    changed = 0
    for i, (path, _, _) in enumerate(rec):
        name, f = os.path.basename(path), floats[path]
        source = _png(path)
        assert source.shape == (FILES[i][2], FILES[i][1], 3)
        for j in range(2):
            want = G.guided(f["dec"][j].numpy(), f["input"].numpy(), f["valid"], source, RADIUS, EPS)
            for kind, w in zip(("bar", "mask"), want):
                got = _png(os.path.join(out, "_%02d_%s" % (j, kind), name))
                _same_bytes(got, w, "%s style %d %s" % (name, j, kind))
            changed += int((want[0] != P.paste(f["dec"][j].numpy(), f["input"].numpy(), f["valid"], source)[0]).sum())
    assert changed > 0                               # (the comparison means something: the bilinear paste's bytes are others)


def test_folder_guided_files_do_not_depend_on_the_batch_size(runs):
    a, b = _tree(runs["guided_b3"][2]), _tree(runs["guided_b1"][2])
    assert [r[2] for r in runs["guided_b1"][0]] == [0, 1, 2, 3]
    assert sorted(a) == sorted(b) and len(a) == 4 * 5
    differ = [n for n in sorted(a) if a[n] != b[n]]
    print("%d of %d files differ between batch_size 3 and 1 %s" % (len(differ), len(a), differ))
    assert not differ


def test_folder_detail_bilinear_is_the_run_without_the_keyword(runs):
    a, b = _tree(runs["bilinear_b3"][2]), _tree(runs["default_b3"][2])
    assert sorted(a) == sorted(b) and len(a) == 4 * 5
    differ = [n for n in sorted(a) if a[n] != b[n]]
    print("%d of %d files differ between detail='bilinear' and no keyword %s" % (len(differ), len(a), differ))
    assert not differ
    g = _tree(runs["guided_b3"][2])
    assert any(g[n] != a[n] for n in a if "_bar" in n) and all(g[n] == a[n] for n in a if "_bar" not in n)     # masks and inputs: the paste's
