"""Sample pictures on the device (csrc/grid.hip through acl-gan_amd/visual.py) and the files train.py writes from them.  -m gpu

The kernel's bytes must EQUAL ref_grid_u8 (tests/test_visual_cpu.py: the reference's rule restated in fp32 on the CPU) -- no tolerance,
no excluded pixels.  Every comparison prints the number of differing bytes and their largest difference before it asserts."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT
from test_visual_cpu import ref_grid_u8

pytestmark = pytest.mark.gpu

NINE = (3, 3, 1, 3, 1, 3, 1, 3, 1)      # channels of sample()'s tuple, focus branch (trainer.py:233-235)
SEVEN = (3,) * 7                        # non-focus branch (trainer.py:243-245)


def _visual():
    import aclgan_amd  # noqa: F401
    from aclgan_amd import visual
    return visual


def _tuple(channels, n, H, W, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [((torch.rand(n, c, H, W, generator=g) * 2 - 1) * scale).cuda() for c in channels]


def _assert_same_bytes(tensors, nrow, what):
    got = _visual().image_grid(tensors, nrow).cpu()
    want = ref_grid_u8([t.cpu() for t in tensors], nrow)
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(want.shape), (got.shape, want.shape)
    diff = (got.to(torch.int32) - want.to(torch.int32)).abs()
    print("%s: %d of %d bytes differ, largest difference %d" % (what, int((diff != 0).sum()), diff.numel(), int(diff.max())))
    assert torch.equal(got, want)
    return got


@pytest.mark.parametrize("channels", [NINE, SEVEN], ids=["focus9", "plain7"])
def test_grid_bytes_sample_tuple_64(channels):
    ts = _tuple(channels, 2, 64, 64, seed=1)
    g = _assert_same_bytes(ts, 2, "random 64x64 n=2")
    assert tuple(g.shape) == (len(channels) * 64, 2 * 64, 3)
    # values exactly at the extremes: the global lo / hi live in different tensors, one of them a 1-channel mask (its bytes: 0 / 255 in
    # all three channels), and every tensor holds values that tie with them
    ts = _tuple(channels, 2, 64, 64, seed=2)
    last = len(channels) - 1
    ts[1][1, 2, 63, 63] = -1.0
    ts[last][0, 0, 0, 0] = 1.0
    for t in ts:
        t[0, 0, 5, 4:12] = -1.0
        t[1, 0, 6, 60:64] = 1.0
    g = _assert_same_bytes(ts, 2, "extremes placed 64x64 n=2")
    assert g[last * 64, 0, 0].item() == 255 and (channels[last] == 3 or g[last * 64, 0].tolist() == [255, 255, 255])
    assert g[1 * 64 + 63, 64 + 63, 2].item() == 0
    # a tuple whose range is far from [-1, 1], and a nearly constant one (hi - lo of the order of the 1e-5 in the divisor)
    _assert_same_bytes(_tuple(channels, 2, 64, 64, seed=3, scale=41.0), 2, "scale 41")
    ts = [0.25 + t * 4e-6 for t in _tuple(channels, 2, 64, 64, seed=4)]
    _assert_same_bytes(ts, 2, "range 8e-6 around 0.25")
    _assert_same_bytes([torch.full_like(t, -0.75) for t in ts], 2, "constant")


def test_grid_bytes_256_display_16():
    ts = _tuple(NINE, 16, 256, 256, seed=5)
    ts[2][7, 0, 100, 100] = -1.0
    ts[5][15, 1, 255, 255] = 1.0
    g = _assert_same_bytes(ts, 16, "256x256 n=16 nrow=16")
    assert tuple(g.shape) == (9 * 256, 16 * 256, 3)


@pytest.mark.parametrize("shape", [(5, 7, (3, 2), (3, 1), 4), (6, 8, (4, 1), (1, 3), 3), (3, 4, (1,), (3,), 8), (9, 13, (2, 2, 3), (1, 3, 1), 7)],
                         ids=["5x7_N5_nrow4", "6x8_N5_nrow3", "3x4_N1_nrow8", "9x13_N7_nrow7"])
def test_grid_bytes_ragged(shape):
    """H != W, W no multiple of 4 (no 16-byte loads, no 12-byte stores), N no multiple of nrow (zero-filled cells), N < nrow"""
    H, W, ns, cs, nrow = shape
    g = torch.Generator().manual_seed(H * 100 + W)
    ts = [(torch.rand(n, c, H, W, generator=g) * 2 - 1).cuda() for n, c in zip(ns, cs)]
    out = _assert_same_bytes(ts, nrow, "ragged %dx%d" % (H, W))
    N = sum(ns)
    cols = min(nrow, N)
    rows = -(-N // cols)
    assert tuple(out.shape) == (rows * H, cols * W, 3)
    if rows * cols > N:
        assert int(out[(rows - 1) * H:, (N % cols) * W:].max()) == 0


def test_grid_bytes_batch_strided_channel_slices():
    """dec[:, :3] / dec[:, 3:] of one (B, 4, H, W) decoder output, as sample() produces them: passed as they are (no copy)"""
    V = _visual()
    g = torch.Generator().manual_seed(11)
    for H, W in ((32, 32), (5, 7)):      # 16-byte aligned slices, and slices that are not
        dec = (torch.rand(4, 4, H, W, generator=g) * 2 - 1).cuda()
        x = (torch.rand(4, 3, H, W, generator=g) * 2 - 1).cuda()
        img, mask = dec.split(3, 1)
        assert not img.is_contiguous() and V._dense(img).data_ptr() == img.data_ptr() and V._dense(mask).data_ptr() == mask.data_ptr()
        _assert_same_bytes([x, img, mask], 4, "channel slices %dx%d" % (H, W))
        _assert_same_bytes([x[:2], img[:2], mask[:2]], 2, "channel slices, first two images %dx%d" % (H, W))
    # a layout that is NOT dense per image (channels_last) is copied, not misread
    cl = (torch.rand(2, 3, 8, 8, generator=g) * 2 - 1).cuda().contiguous(memory_format=torch.channels_last)
    _assert_same_bytes([cl], 2, "channels_last input")


def test_grid_on_a_side_stream_and_nonfinite_input_does_not_fault():
    V = _visual()
    ts = _tuple(NINE, 2, 64, 64, seed=12)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    got = V.image_grid(ts, 2, stream=st)
    st.synchronize()
    assert torch.equal(got.cpu(), ref_grid_u8([t.cpu() for t in ts], 2))
    ts[0][0, 0, 0, 0] = float("nan")
    ts[3][1, 2, 1, 1] = float("inf")
    out = V.image_grid(ts, 2)
    torch.cuda.synchronize()             # the pixel values are unspecified; the launch completes
    assert tuple(out.shape) == (9 * 64, 128, 3)


def test_write_2images_jpeg_equals_pillow_on_the_reference_bytes(tmp_path):
    from PIL import Image
    V = _visual()
    K, H, W, display = len(NINE), 64, 64, 2
    ts = _tuple(NINE, 3, H, W, seed=13)                            # one image more than is displayed: sliced like utils.py:117
    V.write_2images(ts, display, str(tmp_path), "train_current")
    path = os.path.join(tmp_path, "gen_a2b_train_current.jpg")
    got = np.asarray(Image.open(path))
    ref = ref_grid_u8([t[:display].cpu() for t in ts], display).numpy()
    Image.fromarray(ref).save(os.path.join(tmp_path, "ref.jpg"))
    want = np.asarray(Image.open(os.path.join(tmp_path, "ref.jpg")))
    assert got.shape == (K * H, display * W, 3)
    assert np.array_equal(got, want)


# ---- train.py ----
def _tiny_config(**over):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "male2female.yaml")))      # the tiny config of tests/test_gpu_sweep.py
    cfg["gen"].update(dim=8, mlp_dim=16, n_res=1)
    cfg["dis"].update(dim=8)
    cfg.update(batch_size=2, crop_image_height=64, crop_image_width=64, display_size=2, snapshot_save_iter=2, max_iter=3)
    cfg.update(over)
    return cfg


def _train(out, cfg, *extra, env=None):
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "tiny.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--config", path, "--output_path", str(out), "--synthetic", *extra],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    return r


def test_train_py_writes_pictures_index_and_loss_log(tmp_path):
    from PIL import Image
    V = _visual()
    from aclgan_amd import _lib as L
    out = str(tmp_path)
    r = _train(out, _tiny_config(image_save_iter=2, image_display_iter=1, max_iter=3))
    assert "Iteration: 00000003/00000003" in r.stdout and "Finish training" in r.stdout
    run = os.path.join(out, "outputs", "tiny")
    assert sorted(os.listdir(os.path.join(run, "images"))) == ["gen_a2b_test_00000002.jpg", "gen_a2b_train_00000002.jpg", "gen_a2b_train_current.jpg"]
    for name in os.listdir(os.path.join(run, "images")):
        with Image.open(os.path.join(run, "images", name)) as im:
            assert im.size == (2 * 64, 9 * 64) and im.mode == "RGB", (name, im.size)      # 9 rows x display_size columns of 64x64
    want = os.path.join(out, "want.html")
    V.write_html(want, 2, 2, "images")
    assert open(os.path.join(run, "index.html")).read() == open(want).read().replace("want.html", "index.html")
    lines = open(os.path.join(out, "logs", "tiny", "losses.csv")).read().splitlines()
    assert lines[0].split(",") == ["iteration"] + L.LOSS_NAMES
    assert [int(l.split(",")[0]) for l in lines[1:]] == [1, 2, 3] and all(len(l.split(",")) == 17 for l in lines[1:])
    assert all(np.isfinite([float(v) for v in l.split(",")[1:]]).all() for l in lines[1:])


def test_pictures_do_not_disturb_training(tmp_path):
    """Deterministic mode; one two-iteration run, its output tree copied, then the SAME resumed command on both copies -- one with both
    picture cadences out of reach, one with sample() and the display-image fetch between the updates of every iteration (a fresh
    process initialises its weights from an unseeded generator, so both runs start from one checkpoint).  The final weights must be
    bit-identical: pictures leave the generators that training reads, and the training arenas, alone."""
    env = dict(os.environ, ACLGAN_DETERMINISTIC="1")
    off = dict(image_save_iter=10000, image_display_iter=10000)
    a, b = os.path.join(tmp_path, "a"), os.path.join(tmp_path, "b")
    _train(a, _tiny_config(max_iter=2, **off), env=env)
    shutil.copytree(a, b)
    _train(a, _tiny_config(**off), "--resume", "--max_iter", "5", env=env)
    _train(b, _tiny_config(image_save_iter=2, image_display_iter=1), "--resume", "--max_iter", "5", env=env)
    assert not os.path.exists(os.path.join(a, "outputs", "tiny", "images"))
    assert sorted(os.listdir(os.path.join(b, "outputs", "tiny", "images"))) == ["gen_a2b_test_00000004.jpg", "gen_a2b_train_00000004.jpg",
                                                                                "gen_a2b_train_current.jpg"]
    n = 0
    for name in ("gen_00000005.pt", "dis_00000005.pt"):
        sa = torch.load(os.path.join(a, "outputs", "tiny", "checkpoints", name), map_location="cpu")
        sb = torch.load(os.path.join(b, "outputs", "tiny", "checkpoints", name), map_location="cpu")
        assert sa.keys() == sb.keys()
        for net in sa:
            assert sa[net].keys() == sb[net].keys()
            for k in sa[net]:
                assert torch.equal(sa[net][k], sb[net][k]), (name, net, k)
                n += 1
    assert n > 50
