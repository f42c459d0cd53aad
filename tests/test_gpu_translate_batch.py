"""Folder translation on the GPU (csrc/finish.hip through acl-gan_amd/translate.py, test_batch.py's core).  -m gpu

The kernels' bytes must EQUAL tests/translate_ref.py (pinned to test.py's host path in tests/test_translate_batch_cpu.py) -- no tolerance,
no excluded case or pixel.  Every byte comparison prints the number of differing bytes and their largest difference before it asserts.
The floats of the batched forward are held to the oracle at the bound tests/test_gpu_step.py::test_inference_shapes_and_sample_values
uses for the same calls (_rel < 1e-3)."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

from oracle import aclgan_oracle as O
from conftest import GOLDEN
from gpu_util import deterministic_mode
import translate_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 3, 5), (3, 8, 8), (2, 17, 23), (3, 61, 67), (3, 64, 64), (1, 64, 84)]


@pytest.fixture(scope="module")
def TR():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import aclgan_amd  # noqa: F401
    from aclgan_amd import translate
    return translate


@pytest.fixture(scope="module")
def T(TR):
    from aclgan_amd import trainer
    return trainer


def _rel(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _same_bytes(got, want, what):
    got = got.cpu()
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(want.shape), (what, got.shape, want.shape)
    diff = (got.to(torch.int32) - want.to(torch.int32)).abs()
    print("%s: %d of %d bytes differ, largest difference %d" % (what, int((diff != 0).sum()), diff.numel(), int(diff.max())))
    assert torch.equal(got, want), what


def _subsets(channels):
    names = ("bar", "mask", "input") if channels == 4 else ("bar", "input")
    return [list(c) for r in range(1, len(names) + 1) for c in itertools.combinations(names, r)]


def _check_all_subsets(TR, dec, bg, what):
    """finish_u8 of every subset of the pictures against ONE evaluation of the model"""
    want = R.ref_finish_u8(dec, bg)
    for sub in _subsets(dec.shape[1]):
        got = TR.finish_u8(dec, bg, outputs=sub)
        assert sorted(got) == sorted(sub)
        for n in sub:
            _same_bytes(got[n], want[n], "%s %s of %s" % (what, n, "+".join(sub)))
    # the default: every picture the arguments allow; without the images only what needs none
    assert sorted(TR.finish_u8(dec, bg)) == sorted(want)
    if dec.shape[1] == 3:
        _same_bytes(TR.finish_u8(dec)["bar"], want["bar"], what + " bar without images")


# ---- 1. bytes exact ----
@pytest.mark.parametrize("channels", [4, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d_%dx%d" % s)
def test_finish_bytes_equal_the_model(TR, shape, channels):
    B, H, W = shape
    g = torch.Generator().manual_seed(1000 * B + 10 * H + W + channels)
    dec = (torch.rand(B, channels, H, W, generator=g) * 2 - 1).cuda()
    bg = (torch.rand(B, 3, H, W, generator=g) * 2 - 1).cuda()
    _check_all_subsets(TR, dec, bg, "B=%d %dx%d C=%d" % (B, H, W, channels))


def test_finish_bytes_constant_image_and_placed_extremes(TR):
    g = torch.Generator().manual_seed(5)
    dec = (torch.rand(3, 4, 16, 20, generator=g) * 2 - 1).cuda()
    bg = (torch.rand(3, 3, 16, 20, generator=g) * 2 - 1).cuda()
    dec[1] = 0.25                   # image 1 constant in every picture (hi == lo: all bytes 0), its neighbours not
    bg[1] = -0.75
    dec[0, 3, 15, 19] = 1.0         # extremes in a plane's last element, and ties with them
    dec[0, 3, 0, 0:4] = -1.0
    bg[2, 2, 15, 16:20] = 1.0
    bg[2, 0, 7, 3] = -1.0
    _check_all_subsets(TR, dec, bg, "constant image 1")
    out = TR.finish_u8(dec, bg)
    assert all(int(out[n][1].max()) == 0 for n in out) and all(int(out[n][0].max()) == 255 for n in ("mask",))
    assert out["mask"][0, 15, 19].tolist() == [255, 255, 255] and out["mask"][0, 0, 0].tolist() == [0, 0, 0]
    _check_all_subsets(TR, torch.full((2, 3, 8, 8), 0.5).cuda(), torch.full((2, 3, 8, 8), -1.0).cuda(), "constant 3 channels")


@pytest.mark.parametrize("shape", [(3, 8, 8), (2, 17, 23)], ids=["aligned", "unaligned"])
def test_finish_bytes_batch_and_channel_slices_without_a_copy(TR, shape):
    """dec a batch slice [::2] of a larger tensor, bg a channel slice: 16-byte aligned planes (8x8) and planes that are not (17x23)"""
    from aclgan_amd import visual
    B, H, W = shape
    g = torch.Generator().manual_seed(9)
    big = (torch.rand(2 * B, 4, H, W, generator=g) * 2 - 1).cuda()
    wide = (torch.rand(B, 4, H, W, generator=g) * 2 - 1).cuda()
    dec, bg = big[::2], wide[:, 1:4]
    assert not dec.is_contiguous() and not bg.is_contiguous()
    assert visual._dense(dec).data_ptr() == dec.data_ptr() and visual._dense(bg).data_ptr() == bg.data_ptr()
    _check_all_subsets(TR, dec, bg, "slices %dx%d" % (H, W))
    _check_all_subsets(TR, big[1::2, :3], bg, "slices %dx%d, 3 of 4 channels" % (H, W))
    # a layout that is NOT dense per image is copied, not misread
    cl = wide.contiguous(memory_format=torch.channels_last)
    _check_all_subsets(TR, cl, bg, "channels_last %dx%d" % (H, W))


# ---- 2. independence ----
def test_image_bytes_do_not_depend_on_the_batch(TR):
    g = torch.Generator().manual_seed(21)
    scale = torch.tensor([1e-3, 1.0, 50.0]).view(3, 1, 1, 1)
    for H, W in ((64, 84), (17, 23)):
        dec = ((torch.rand(3, 4, H, W, generator=g) * 2 - 1) * scale).cuda()
        bg = ((torch.rand(3, 3, H, W, generator=g) * 2 - 1) * scale).cuda()
        both = TR.finish_u8(dec, bg)
        for i in range(3):
            alone = TR.finish_u8(dec[i:i + 1], bg[i:i + 1])
            for n in ("bar", "mask", "input"):
                _same_bytes(alone[n][0], both[n][i].cpu(), "image %d %s alone / in the batch, %dx%d" % (i, n, H, W))
                assert int(both[n][i].min()) == 0 and int(both[n][i].max()) >= 240      # its own range, not the batch's


# ---- 3. floats of the batched forward ----
def _reduced(plain):
    if plain:
        cfg = json.load(open(os.path.join(GOLDEN, "step_reduced_64_plain.json")))["config"]
    else:
        cfg = O.default_config()
        cfg["gen"].update(dim=8, mlp_dim=16, n_res=1)
        cfg["dis"].update(dim=8)
        cfg["display_size"] = 2
    return cfg


def _make(T, cfg, nets, **kw):
    tr = T.aclgan_Trainer(cfg, **kw)
    for name in O.OracleTrainer.NETS:
        getattr(tr, name).load_state_dict(nets[name], strict=False)
    return tr


@pytest.mark.parametrize("a2b", [True, False], ids=["a2b", "b2a"])
@pytest.mark.parametrize("plain", [False, True], ids=["focus", "plain"])
def test_translate_batch_floats_against_the_oracle(TR, T, plain, a2b):
    cfg = _reduced(plain)
    nets = O.test_nets(cfg, 6)
    tr = _make(T, cfg, nets)
    gc = cfg["gen"]
    g = torch.Generator().manual_seed(31)
    x = torch.rand(3, 3, 64, 84, generator=g) * 2 - 1
    styles = torch.randn(3, 2, gc["style_dim"], 1, 1, generator=g)
    res = TR.translate_batch(tr, x, styles, a2b=a2b)
    P = nets["gen_AB" if a2b else "gen_BA"]
    content = O.content_encode(P, x, gc)
    assert len(res["dec"]) == 2 and tr._ws_shape[3] is False
    for j in range(2):
        want = O.decode(P, content, styles[:, j], gc)
        assert tuple(res["dec"][j].shape) == tuple(want.shape) == (3, gc["output_dim"], 64, 84)
        err = _rel(res["dec"][j], want)
        print("style %d: rel %.3g" % (j, err))
        assert err < 1e-3
        # and the pictures are the model's, from the floats the forward returned
        dec = res["dec"][j] if tr.focus_lam > 0 else res["dec"][j][:, :3]
        ref = R.ref_finish_u8(dec, x)
        _same_bytes(res["bar"][j], ref["bar"], "bar %d" % j)
        if tr.focus_lam > 0:
            _same_bytes(res["mask"][j], ref["mask"], "mask %d" % j)
        else:
            assert res["mask"] is None
    _same_bytes(res["input"], R.ref_finish_u8(res["dec"][0], x)["input"], "input")
    per = 2 if tr.focus_lam > 0 else 1
    assert tuple(res["bytes"].shape) == (2 * per + 1, 3, 64, 84, 3) and res["bar"][1].data_ptr() == res["bytes"][per].data_ptr()
    # the styles are per image: image 1 with image 0's style rows is another picture
    swapped = styles.clone()
    swapped[1] = styles[0]
    other = TR.translate_batch(tr, x, swapped, a2b=a2b, with_input=False)
    assert other["input"] is None and tuple(other["bytes"].shape) == (2 * per, 3, 64, 84, 3)
    assert torch.equal(other["dec"][0][0], res["dec"][0][0]) and not torch.equal(other["dec"][0][1], res["dec"][0][1])


# ---- 4. / 5. the folder, end to end ----
FILES = [("a0.png", 128, 96), ("a1.png", 128, 96), ("b0.png", 64, 64), ("c0.png", 128, 96), ("d0.png", 64, 64)]      # (name, width, height)


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    from PIL import Image
    src = str(tmp_path_factory.mktemp("translate_in"))
    yy, xx = np.mgrid[0:256, 0:256]
    rng = np.random.RandomState(4)
    for k, (name, w, h) in enumerate(FILES):      # smooth pictures with some noise: resampling and blending see more than flat colours
        base = np.stack([(xx[:h, :w] * (k + 1)) % 256, (yy[:h, :w] * 2 + 30 * k) % 256, ((xx[:h, :w] + yy[:h, :w]) // 2) % 256], -1)
        Image.fromarray(((base + rng.randint(0, 40, (h, w, 3))) % 256).astype(np.uint8)).save(os.path.join(src, name))
    return src


@pytest.fixture(scope="module")
def folder_trainer(T):
    cfg = _reduced(False)
    cfg["new_size"] = 48
    return _make(T, cfg, O.test_nets(cfg, 6)), cfg


def _png(path):
    from PIL import Image
    with Image.open(path) as im:
        assert im.format == "PNG" and im.mode == "RGB"
        return torch.from_numpy(np.asarray(im).copy())


def test_folder_end_to_end_against_the_model(TR, folder, folder_trainer, tmp_path):
    from PIL import Image
    tr, cfg = folder_trainer
    out = os.path.join(tmp_path, "out")
    torch.manual_seed(3)
    rec, floats = TR.translate_folder(tr, cfg, folder, out, a2b=True, num_style=2, batch_size=2, keep_float=True)
    names = [f[0] for f in FILES]
    assert [os.path.basename(p) for p, _, _ in rec] == names
    assert [s for _, s, _ in rec] == [(48, 64), (48, 64), (48, 48), (48, 64), (48, 48)]
    assert [b for _, _, b in rec] == [0, 0, 1, 2, 3]                      # a shape change closes the batch of two
    assert sorted(os.listdir(out)) == sorted(["_00_bar", "_00_mask", "_01_bar", "_01_mask"] + ["input%03d.jpg" % i for i in range(5)])
    for i, (path, (H, W), _) in enumerate(rec):
        f = floats[path]
        assert len(f["dec"]) == 2 and tuple(f["dec"][0].shape) == (4, H, W) and tuple(f["input"].shape) == (3, H, W)
        for j in range(2):
            want = R.ref_finish_u8(f["dec"][j][None], f["input"][None])
            for kind in ("bar", "mask"):
                d = os.path.join(out, "_%02d_%s" % (j, kind))
                assert sorted(os.listdir(d)) == sorted(names)
                got = _png(os.path.join(d, names[i]))
                assert tuple(got.shape) == (H, W, 3)
                _same_bytes(got, want[kind][0], "%s style %d %s" % (names[i], j, kind))
        with Image.open(os.path.join(out, "input%03d.jpg" % i)) as im:
            assert im.format == "JPEG" and im.size == (W, H)
        assert not torch.equal(f["dec"][0], f["dec"][1])                  # two styles, two pictures
    assert tr._ws_shape[3] is False                                       # forward-only workspace


def test_folder_batch_1_files_equal_the_single_image_script(TR, folder, folder_trainer, tmp_path):
    """batch_size 1 against test.py's own path, file by file: load_image -> translate -> save_image.  The forward is bit-reproducible and
    the device input pipeline bit-identical to Pillow's, so the files are compared byte for byte."""
    test_py = R.test_script()
    tr, cfg = folder_trainer
    S, n = 2, len(FILES)
    out, ref = os.path.join(tmp_path, "out"), os.path.join(tmp_path, "ref")
    for a2b in (True, False):
        torch.manual_seed(11)
        TR.translate_folder(tr, cfg, folder, out, a2b=a2b, num_style=S, batch_size=1)
        torch.manual_seed(11)
        styles = TR.draw_styles(n, S, cfg["gen"]["style_dim"])             # the same draws, explicit
        ndiff = 0
        for i, (name, _, _) in enumerate(FILES):
            image = test_py.load_image(os.path.join(folder, name), cfg["new_size"]).cuda()
            outs = test_py.translate(tr, image, styles[i].cuda(), a2b=a2b)
            pairs = [(os.path.join(out, "input%03d.jpg" % i), image, "input.jpg")]
            for j, (outputs, outputs_mask, _) in enumerate(outs):
                pairs.append((os.path.join(out, "_%02d_bar" % j, name), outputs, "bar%d.png" % j))
                pairs.append((os.path.join(out, "_%02d_mask" % j, name), outputs_mask, "mask%d.png" % j))
            for got_path, t, ref_name in pairs:
                want_path = os.path.join(ref, ref_name)
                test_py.save_image(t, want_path)
                same = open(got_path, "rb").read() == open(want_path, "rb").read()
                if not same and ref_name.endswith(".png"):
                    d = (_png(got_path).int() - _png(want_path).int()).abs()
                    print("%s %s a2b=%s: %d pixels differ, largest difference %d" % (name, ref_name, a2b, int((d != 0).sum()), int(d.max())))
                ndiff += not same
        print("a2b=%s: %d of %d files differ from test.py's" % (a2b, ndiff, n * (2 * S + 1)))
        assert ndiff == 0


# ---- 6. weights and state ----
@pytest.fixture(scope="module")
def fix():
    meta = json.load(open(os.path.join(GOLDEN, "step_reduced_64.json")))
    data = np.load(os.path.join(GOLDEN, "step_reduced_64.npz"))
    cfg = meta["config"]
    x_a, x_b = torch.from_numpy(data["x_a"]), torch.from_numpy(data["x_b"])
    z = [torch.from_numpy(data["z%d" % i]) for i in range(6)]
    return cfg, O.test_nets(cfg, 0), x_a, x_b, z


def test_translate_reads_the_average_inside_ema_weights_only(TR, T, fix):
    from aclgan_amd import _lib as L
    cfg, nets, x_a, x_b, z = fix
    cfg = dict(cfg, ema_decay=0.5)
    with deterministic_mode(L, True):
        tr = _make(T, cfg, nets, deterministic=True)
        tr.ema_reset()
        for _ in range(2):
            tr.dis_update(x_a, x_b, cfg, z=z[:3])
            tr.gen_update(x_a, x_b, cfg, z=z[3:])
        assert not torch.equal(tr._ema, tr._param[0])
        styles = torch.randn(2, 1, cfg["gen"]["style_dim"], 1, 1, generator=torch.Generator().manual_seed(2))
        live = TR.translate_batch(tr, x_a, styles)
        with tr.ema_weights():
            avg = TR.translate_batch(tr, x_a, styles)
        again = TR.translate_batch(tr, x_a, styles)
        assert not torch.equal(avg["dec"][0], live["dec"][0]) and not torch.equal(avg["bytes"], live["bytes"])
        assert torch.equal(again["dec"][0], live["dec"][0]) and torch.equal(again["bytes"], live["bytes"])
        # the average as the live weights of another trainer gives the same floats and bytes
        plain = _make(T, dict(fix[0]), nets, deterministic=True)
        sd = tr.ema_state_dict()
        plain.gen_AB.load_state_dict(sd["AB"]); plain.gen_BA.load_state_dict(sd["BA"])
        twin = TR.translate_batch(plain, x_a, styles)
        assert torch.equal(twin["dec"][0], avg["dec"][0]) and torch.equal(twin["bytes"], avg["bytes"])


def test_folder_translation_leaves_training_alone(TR, T, fix, folder, tmp_path):
    """dis_update, [translate_folder], gen_update, dis_update, gen_update: the same losses and weights with and without the call between a
    dis_update and the gen_update that adopts its content encodings (forward-only workspace, carried encodings, weight selection)"""
    from aclgan_amd import _lib as L
    cfg, nets, x_a, x_b, z = fix
    cfg = dict(cfg, new_size=48)
    with deterministic_mode(L, True):
        losses = []
        for translate in (False, True):
            tr = _make(T, cfg, nets, deterministic=True)
            xa, xb = x_a.cuda(), x_b.cuda()
            seq = []
            tr.dis_update(xa, xb, cfg, z=z[:3]); seq.append(tr._losses.clone())
            if translate:
                rec = TR.translate_folder(tr, cfg, folder, os.path.join(tmp_path, "o"), num_style=1, batch_size=2)
                assert len(rec) == len(FILES)
            tr.gen_update(xa, xb, cfg, z=z[3:]); seq.append(tr._losses.clone())
            tr.dis_update(xa, xb, cfg, z=z[:3]); seq.append(tr._losses.clone())
            tr.gen_update(xa, xb, cfg, z=z[3:]); seq.append(tr._losses.clone())
            torch.cuda.synchronize()
            losses.append((seq, tr._param[0].clone(), tr._param[1].clone()))
        (a, ga, da), (b, gb, db) = losses
        for k, (u, v) in enumerate(zip(a, b)):
            assert torch.equal(u, v), (k, u, v)
        assert float(a[-1].abs().sum()) > 0 and torch.equal(ga, gb) and torch.equal(da, db)
