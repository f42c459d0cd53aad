"""fp32 CPU model of the finishing rule of csrc/finish.hip (include/aclgan_hip.h: aclgan_translate_finish_u8), written with torch CPU
operators, one operator per rounding.  tests/test_translate_batch_cpu.py pins it to the host path the project already ships
(test.focus_translation -> (o + 1) / 2 -> test.save_image); the GPU tests compare the kernels' bytes with it, exactly."""
import importlib.util
import os

import torch


def test_script():
    """the repository's test.py as a module (its name collides with a package of the standard library: loaded from its path)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("aclgan_test_script_translate", os.path.join(root, "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


test_script.__test__ = False


def unit(x):
    return (x + 1) / 2


def ref_bar(dec, bg):
    """(B, 3, H, W) floats of the 'bar' picture: test.py's blend chain with a focus channel, (dec + 1) / 2 without"""
    dec = dec.detach().float().cpu()
    if dec.shape[1] == 3:
        return unit(dec)
    bg = bg.detach().float().cpu()
    fg, f = dec[:, :3], dec[:, 3:]
    m = unit(f).expand(-1, 3, -1, -1)
    a = unit(fg)
    b = unit(bg)
    am = a * m
    n = 1 - m
    bn = b * n
    t = am + bn
    o = t * 2 - 1
    return unit(o)


def ref_bytes(pic):
    """save_image(padding=0, normalize=True) of ONE (3, H, W) picture -> (H, W, 3) uint8"""
    pic = pic.detach().float().cpu()
    lo, hi = float(pic.min()), float(pic.max())
    d = torch.tensor(hi - lo + 1e-5, dtype=torch.float64).to(torch.float32)      # the double sum, rounded to fp32 once
    c = pic.clamp(lo, hi)
    q = (c - lo) / d
    v = q * 255
    r = v + 0.5
    return r.clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()


def ref_finish_u8(dec, bg=None, outputs=None):
    """{name: (B, H, W, 3) uint8} for the pictures of `outputs` (default: all that the arguments allow), every image with its own range"""
    dec = dec.detach().float().cpu()
    if outputs is None:
        outputs = [n for n in ("bar", "mask", "input") if (n != "mask" or dec.shape[1] == 4) and (n != "input" or bg is not None)]
    pics = {}
    if "bar" in outputs:
        pics["bar"] = ref_bar(dec, bg)
    if "mask" in outputs:
        pics["mask"] = dec[:, 3:].expand(-1, 3, -1, -1)
    if "input" in outputs:
        pics["input"] = bg.detach().float().cpu()
    return {n: torch.stack([ref_bytes(p[i]) for i in range(p.shape[0])]) for n, p in pics.items()}
