"""Sample pictures, HTML index and loss log (acl-gan_amd/visual.py): everything that needs no GPU.

ref_grid_u8 below is the yardstick the device kernel (csrc/grid.hip) is held to byte for byte in tests/test_gpu_visual.py: a plain
fp32 torch restatement of what the reference does to the tuple trainer.sample() returns (utils.py:115-119) under the torchvision
0.4.0 its acl-gan.yaml pins.  Here it is checked against hand-computed cases and against an independent numpy evaluation."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, GOLDEN


def ref_grid_u8(tensors, nrow):
    """uint8 (rows*H, cols*W, 3) of utils.py:116-119 on the CPU, operation by operation:

      utils.py:116      images.expand(-1, 3, -1, -1)
      utils.py:117      torch.cat(..., 0)
      torchvision/utils.py make_grid(tensor, nrow, padding=0, normalize=True, range=None, scale_each=False, pad_value=0):
          tensor = tensor.clone()
          norm_range(tensor, None) -> norm_ip(tensor, float(t.min()), float(t.max())):
              img.clamp_(min=min, max=max); img.add_(-min).div_(max - min + 1e-5)
          (min / max are Python floats: `max - min + 1e-5` is evaluated in double and becomes an fp32 scalar in div_)
          xmaps = min(nrow, nmaps); ymaps = int(math.ceil(float(nmaps) / xmaps)); grid = tensor.new_full(..., pad_value)
          image k -> grid[:, y*H:(y+1)*H, x*W:(x+1)*W] for y in range(ymaps) for x in range(xmaps), stopping at nmaps
      torchvision/utils.py save_image(grid, nrow=1): make_grid returns a single 3-channel image unchanged, then
          grid.mul_(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to('cpu', torch.uint8)
    """
    t = torch.cat([x.detach().to("cpu", torch.float32).expand(-1, 3, -1, -1) for x in tensors], 0).clone()
    lo, hi = float(t.min()), float(t.max())
    t.clamp_(min=lo, max=hi)
    t.add_(-lo).div_(hi - lo + 1e-5)
    nmaps, _, H, W = t.shape
    xmaps = min(nrow, nmaps)
    ymaps = int(math.ceil(float(nmaps) / xmaps))
    grid = t.new_full((3, H * ymaps, W * xmaps), 0)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= nmaps:
                break
            grid.narrow(1, y * H, H).narrow(2, x * W, W).copy_(t[k])
            k += 1
    return grid.mul_(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).contiguous()


def _numpy_grid_u8(tensors, nrow):
    """the same rule with numpy's fp32 arithmetic (every operation separately rounded, true division), written independently"""
    imgs = np.concatenate([np.repeat(x.numpy(), 3 // x.shape[1], axis=1) for x in tensors], 0).astype(np.float32)
    lo, hi = np.float32(imgs.min()), np.float32(imgs.max())
    d = np.float32(float(hi) - float(lo) + 1e-5)
    v = (np.clip(imgs, lo, hi) - lo) / d
    v = np.clip(v * np.float32(255) + np.float32(0.5), 0, 255).astype(np.uint8)      # numpy does not fuse; float -> uint8 truncates
    N, _, H, W = imgs.shape
    cols = min(nrow, N)
    rows = -(-N // cols)
    out = np.zeros((rows * H, cols * W, 3), np.uint8)
    for n in range(N):
        r, c = divmod(n, cols)
        out[r * H:(r + 1) * H, c * W:(c + 1) * W] = v[n].transpose(1, 2, 0)
    return out


def _visual():
    import aclgan_amd  # noqa: F401
    from aclgan_amd import visual
    return visual


# ---- the yardstick against hand-computed cases ----
def test_ref_grid_truncation_and_divisor_epsilon():
    # lo = -1, hi = 1, d = fp32(2.00001): 0 -> 1 / 2.00001 * 255 + 0.5 = 127.9994 -> 127 (truncated, not rounded); 1 -> 255.4987 -> clamp 255
    x = torch.tensor([-1.0, 0.0, 1.0]).view(3, 1, 1, 1)
    assert ref_grid_u8([x], 3)[0, :, 0].tolist() == [0, 127, 255]
    # hi - lo = 1e-5 is as large as the 1e-5 of the divisor: the top value lands on 0.5 -> 127.5 + 0.5 = 128, not 255
    x = torch.tensor([0.0, 1e-5]).view(2, 1, 1, 1)
    assert ref_grid_u8([x], 2)[0, :, 0].tolist() == [0, 128]


def test_ref_grid_one_channel_expands_to_three():
    gray = torch.tensor([-1.0, 1.0]).view(1, 1, 1, 2)
    rgb = torch.tensor([[-1.0, 0.0], [0.0, 1.0], [1.0, -1.0]]).view(1, 3, 1, 2)
    g = ref_grid_u8([gray, rgb], 2)
    assert tuple(g.shape) == (1, 4, 3) and g.dtype == torch.uint8
    assert g[0].tolist() == [[0, 0, 0], [255, 255, 255],           # the gray image: three equal channels
                             [0, 127, 255], [127, 255, 0]]         # the colour image: HWC order


def test_ref_grid_cell_order_and_empty_cells():
    # five constant 2x3 images with values 0..4: lo = 0, hi = 4, d = 4.00001 -> n / 4.00001 * 255 + 0.5 = 0.5, 64.25, 127.9997, 191.75, 255.4994
    imgs = [torch.full((1, 3, 2, 3), float(n)) for n in range(3)] + [torch.full((2, 1, 2, 3), 3.0)]
    imgs[3][1] = 4.0
    g = ref_grid_u8(imgs, 3)                                      # N = 5 is no multiple of nrow: cols 3, rows 2, the last cell empty
    assert tuple(g.shape) == (4, 9, 3)
    want = np.kron(np.array([[0, 64, 127], [191, 255, 0]], np.uint8), np.ones((2, 3), np.uint8))
    for ch in range(3):
        assert np.array_equal(g[:, :, ch].numpy(), want)
    g = ref_grid_u8(imgs[:2], 8)                                  # N < nrow: one row of N cells
    assert tuple(g.shape) == (2, 6, 3)
    assert np.array_equal(g[:, :, 0].numpy(), np.kron(np.array([[0, 255]], np.uint8), np.ones((2, 3), np.uint8)))   # (hi = 1: 1 / 1.00001 * 255 + 0.5 = 255.497)


def test_ref_grid_constant_input_is_black():
    g = ref_grid_u8([torch.full((2, 3, 4, 4), 0.3), torch.full((2, 1, 4, 4), 0.3)], 2)
    assert tuple(g.shape) == (8, 8, 3) and int(g.max()) == 0      # (x - lo) = 0 over the 1e-5 the divisor keeps


def test_ref_grid_agrees_with_numpy_fp32():
    g = torch.Generator().manual_seed(7)
    for shapes, nrow in (([(2, 3, 8, 8), (2, 1, 8, 8), (2, 3, 8, 8)], 2), ([(5, 3, 5, 7), (2, 1, 5, 7)], 4), ([(3, 1, 16, 12)], 16)):
        for scale in (1.0, 1e-3, 37.0):
            ts = [(torch.rand(s, generator=g) * 2 - 1) * scale for s in shapes]
            assert np.array_equal(ref_grid_u8(ts, nrow).numpy(), _numpy_grid_u8(ts, nrow))


# ---- index.html ----
def test_write_html_matches_the_reference_file(tmp_path):
    """tests/golden/index_reference.html is what the reference's utils.write_html wrote for (index.html, 30000, 10000, 'images')
    (tests/golden/make_golden_visual.py)"""
    V = _visual()
    path = os.path.join(tmp_path, "index.html")
    V.write_html(path, 30000, 10000, "images")
    got, want = open(path).read(), open(os.path.join(GOLDEN, "index_reference.html")).read()
    assert got == want
    # three saved iterations, newest first; the b2a pictures are linked although nothing writes them
    order = [got.index("gen_a2b_test_%08d.jpg" % j) for j in (30000, 20000, 10000)]
    assert order == sorted(order) and "gen_b2a_train_00010000.jpg" in got and "gen_a2b_test_00000000.jpg" not in got


def test_write_html_before_the_first_saved_iteration(tmp_path):
    V = _visual()
    path = os.path.join(tmp_path, "run.html")
    V.write_html(path, 3, 10, "pics", all_size=640)
    txt = open(path).read()
    assert "Experiment name = run.html" in txt and "_test_" not in txt
    assert txt.count('<img src="pics/gen_a2b_train_current.jpg" style="width:640px">') == 1


# ---- cadence ----
def test_image_due_follows_the_reference_cadence():
    import aclgan_amd  # noqa: F401
    from aclgan_amd.train_loop import image_due
    from oracle import aclgan_oracle as O
    cfg = O.default_config()
    assert "image_save_iter" not in cfg and "image_display_iter" not in cfg      # a missing key means never
    assert not any(image_due(i, cfg, k) for i in range(50) for k in ("image_save_iter", "image_display_iter"))
    for never in (0, -1, None):
        assert not any(image_due(i, {"image_save_iter": never}, "image_save_iter") for i in range(50))
    cfg = {"image_save_iter": 10, "image_display_iter": 4}
    assert [i for i in range(40) if image_due(i, cfg, "image_save_iter")] == [9, 19, 29, 39]          # (iterations + 1) % n == 0, train.py:83
    assert [i for i in range(12) if image_due(i, cfg, "image_display_iter")] == [3, 7, 11]            # train.py:92


# ---- loss log ----
def test_loss_log_header_once_and_append_on_reopen(tmp_path):
    V = _visual()
    from aclgan_amd import _lib as L
    path = os.path.join(tmp_path, "logs", "tiny", "losses.csv")
    vals = torch.arange(16, dtype=torch.float32) / 3 + 1e-7
    log = V.LossLog(path)
    log.append(1, vals.tolist())
    log.append(2, (vals * 2).tolist())
    log.close()
    log = V.LossLog(path)                                          # a resumed run
    log.append(3, (vals * 3).tolist())
    log.close()
    lines = open(path).read().splitlines()
    assert len(lines) == 4
    assert lines[0].split(",") == ["iteration"] + L.LOSS_NAMES and len(L.LOSS_NAMES) == 16
    assert sum(l.startswith("iteration") for l in lines) == 1
    for i, line in enumerate(lines[1:], 1):
        f = line.split(",")
        assert len(f) == 17 and int(f[0]) == i
        assert torch.equal(torch.tensor([float(v) for v in f[1:]], dtype=torch.float64).to(torch.float32), vals * i)    # fp32 values round-trip
    with pytest.raises(ValueError):
        V.LossLog(path).append(4, [0.0] * 15)


# ---- C ABI argument checks (return before anything is launched) ----
def test_image_grid_rejects_bad_arguments_without_gpu():
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib as L
    assert L.lib.aclgan_image_grid_scratch_bytes() >= 8
    fake = 4096                                                    # never dereferenced: every call below fails validation first

    def call(srcs, H=4, W=4, nrow=2, out=fake, scratch=fake):
        arr = (L.GridSrc * max(1, len(srcs)))(*[L.GridSrc(*s) for s in srcs])
        return L.lib.aclgan_image_grid_u8(arr if srcs else None, len(srcs), H, W, nrow, C.c_void_p(out), C.c_void_p(scratch), None)

    assert call([(fake, 48, 1, 2)]) == -1 and "channels" in L.last_error()
    assert call([(fake, 48, 1, 3), (None, 16, 1, 1)]) == -1 and "null" in L.last_error()
    assert call([(fake, 48, 1, 3)], H=0) == -1 and call([(fake, 48, 1, 3)], W=-2) == -1 and call([(fake, 48, 1, 3)], nrow=0) == -1
    assert call([(fake, 48, 1, 3)], out=None) == -1 and call([(fake, 48, 1, 3)], scratch=None) == -1
    assert call([]) == -1
    assert call([(fake, 48, 0, 3)]) == -1
    assert call([(fake, 48, 1, 3)] * (L.GRID_MAX_SRCS + 1)) == -1
    with pytest.raises(L.AclganError):
        _visual().image_grid([torch.zeros(1, 3, 4, 4)], 1)         # a CPU tensor: there is no host path
