"""Translating a folder of test images in batches (the counterpart of the reference's test_batch.py; its loop is lines 105-194).

finish_u8         decoder outputs + input images of a batch -> the byte pictures that get written, on the device (csrc/finish.hip through
                  aclgan_translate_finish_u8: focus blend, one value range per picture per image, normalisation, rounding to bytes)
reflect_pad       fit: pad -- a batch whose shape is no multiple of 2 ** n_downsample, padded at the bottom and the right (csrc/paste.hip)
paste_u8          full_size -- the edit of a batch pasted onto every image's own source pixels, at the source's size (csrc/paste.hip)
guided_u8         full_size, detail: guided -- the same pictures with the photograph's own detail inside the edit: a local affine model of
                  the edit fitted at net resolution, upsampled and evaluated on the source pixels (csrc/guided.hip)
translate_batch   one encode of the batch, one decode per style column, finish_u8, paste_u8 or guided_u8; every byte of the batch in ONE
                  device buffer
translate_folder  the driver: file order, grouping by shape, style draws, output paths, one device->host copy per batch, Pillow encodes in a
                  thread pool while the next batch is decoded and translated

PyTorch does the plumbing only: allocations, views, the host copies.  What the reference computes per image at batch 1 -- and test.py with
it -- is computed here per batch; with batch_size 1 the written files are byte-identical to test.py's load_image -> translate -> save_image.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib as L
from .data import GpuBatchTransform, ImageFolder, default_loader, resized_size
from .visual import _dense

PICTURES = ("bar", "mask", "input")
MAX_WORKERS = 16


def finish_u8(dec, images=None, outputs=None, out=None, stream=None):
    """dec (B, 4 or 3, H, W): decoder outputs (or a 3-channel slice of them), images (B, 3, H, W): what was translated -- device fp32
    tensors; any batch stride passes without a copy (batch slices, channel slices), as in visual.image_grid.
    outputs: which of 'bar', 'mask', 'input' to make (default: all that the arguments allow: 'mask' needs 4 channels, 'input' the images).
    out: optional dict of preallocated contiguous (B, H, W, 3) uint8 device tensors to write into (views of one buffer: translate_batch).
    Returns {name: uint8 (B, H, W, 3)} on dec's device; include/aclgan_hip.h states the rule.  Nothing is synchronised."""
    dev = dec.device
    if dev.type != "cuda":
        raise L.AclganError("finish_u8: tensors must be on the GPU (got %s); there is no CPU path" % dev)
    if dec.dim() != 4 or dec.shape[1] not in (3, 4) or dec.shape[0] < 1:
        raise L.AclganError("finish_u8: expected a (B, 3 or 4, H, W) decoder output, got %s" % (tuple(dec.shape),))
    B, Cd, H, W = dec.shape
    if images is not None and (tuple(images.shape) != (B, 3, H, W) or images.device != dev):
        raise L.AclganError("finish_u8: expected (%d, 3, %d, %d) images on %s, got %s on %s" % (B, H, W, dev, tuple(images.shape), images.device))
    if outputs is None:
        outputs = [n for n in PICTURES if (n != "mask" or Cd == 4) and (n != "input" or images is not None)]
    outputs = list(outputs)
    if not outputs or any(n not in PICTURES for n in outputs):
        raise L.AclganError("finish_u8: outputs must be a non-empty subset of %s, got %s" % (PICTURES, outputs))
    with torch.cuda.device(dev), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
        d = _dense(dec)                  # (kept alive until the launches are enqueued; the caching allocator is stream-ordered)
        g = _dense(images) if images is not None else None
        res = {}
        for n in outputs:
            t = out[n] if out is not None else torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev)
            if tuple(t.shape) != (B, H, W, 3) or t.dtype != torch.uint8 or t.device != dev or not t.is_contiguous():
                raise L.AclganError("finish_u8: out[%r] must be a contiguous (%d, %d, %d, 3) uint8 tensor on %s" % (n, B, H, W, dev))
            res[n] = t
        scratch = torch.empty(L.lib.aclgan_translate_finish_scratch_bytes(B), dtype=torch.uint8, device=dev)
        L.check(L.lib.aclgan_translate_finish_u8(L.ptr(d), d.stride(0) if B > 1 else 0, Cd, L.ptr(g), g.stride(0) if g is not None and B > 1 else 0,
                                                 B, H, W, L.ptr(res.get("bar")), L.ptr(res.get("mask")), L.ptr(res.get("input")),
                                                 L.ptr(scratch), L.stream_ptr(dev)), "translate_finish_u8")
    return res


def padded_shape(shape, multiple):
    """(PH, PW): each side of (oh, ow) rounded up to the next multiple"""
    return tuple(-(-n // multiple) * multiple for n in shape)


def reflect_pad(images, multiple, stream=None):
    """images (B, C, oh, ow) device fp32 -> (B, C, PH, PW), PH / PW the next multiples of `multiple`: rows added at the bottom and columns at
    the right by reflection without the edge, copied bit for bit (include/aclgan_hip.h: aclgan_translate_pad).  A side below `multiple` is
    an error.  One launch, also for a shape that is aligned already (a plain copy).  Nothing is synchronised."""
    dev = images.device
    if dev.type != "cuda":
        raise L.AclganError("reflect_pad: tensors must be on the GPU (got %s); there is no CPU path" % dev)
    if images.dim() != 4 or images.shape[0] < 1:
        raise L.AclganError("reflect_pad: expected (B, C, H, W) images, got %s" % (tuple(images.shape),))
    B, Cn, oh, ow = images.shape
    with torch.cuda.device(dev), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
        s = _dense(images)
        PH, PW = padded_shape((oh, ow), multiple) if multiple >= 1 else (oh, ow)
        out = torch.empty(B, Cn, PH, PW, dtype=torch.float32, device=dev)
        L.check(L.lib.aclgan_translate_pad(L.ptr(s), s.stride(0) if B > 1 else 0, B, Cn, oh, ow, multiple, L.ptr(out), L.stream_ptr(dev)), "translate_pad")
    return out


def paste_plan(sources, device):
    """sources: per image (byte offset of its HWC RGB uint8 pixels in the staged buffer, src_h, src_w).  Packs the pictures of the batch one
    after the other and returns the descriptors of aclgan_translate_paste_u8 on the host and on `device`:
    {'descs', 'dev', 'offsets': [byte offset of image k's picture], 'sizes': [(src_h, src_w)], 'total': bytes of one picture kind}"""
    n = len(sources)
    descs = (L.PasteDesc * n)()
    offsets, sizes, off = [], [], 0
    for k, (so, h, w) in enumerate(sources):
        d = descs[k]
        d.src_offset, d.out_offset, d.src_h, d.src_w = int(so), off, int(h), int(w)
        offsets.append(off)
        sizes.append((int(h), int(w)))
        off += int(h) * int(w) * 3
    host = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8)
    if torch.device(device).type == "cuda":                # pinned: the copy is asynchronous, as the staging upload of the pixels is
        host = host.pin_memory()
    dev = host.to(device, non_blocking=True)
    return {"descs": descs, "dev": dev, "offsets": offsets, "sizes": sizes, "total": off}


def paste_u8(dec, x, valid, src, plan, outputs=("bar", "mask"), out=None, stream=None):
    """The edit at every image's own size (include/aclgan_hip.h: aclgan_translate_paste_u8).  dec (B, 4 or 3, PH, PW) decoder outputs and
    x (B, 3, PH, PW) the net input, device fp32 (batch and channel slices pass without a copy, as in finish_u8); valid = (oh, ow): the
    region of them that is the resized source; src: the 1-D uint8 device buffer the sources were staged in (GpuBatchTransform.stage);
    plan: paste_plan() of the batch.  out: optional dict of preallocated contiguous 1-D uint8 device tensors of plan['total'] bytes.
    Returns {name: uint8 (total,)}: image k's (src_h, src_w, 3) picture starts at plan['offsets'][k].  Nothing is synchronised."""
    dev = dec.device
    if dev.type != "cuda":
        raise L.AclganError("paste_u8: tensors must be on the GPU (got %s); there is no CPU path" % dev)
    if dec.dim() != 4 or dec.shape[1] not in (3, 4) or dec.shape[0] < 1:
        raise L.AclganError("paste_u8: expected a (B, 3 or 4, H, W) decoder output, got %s" % (tuple(dec.shape),))
    B, Cd, PH, PW = dec.shape
    if tuple(x.shape) != (B, 3, PH, PW) or x.device != dev:
        raise L.AclganError("paste_u8: expected (%d, 3, %d, %d) net inputs on %s, got %s on %s" % (B, PH, PW, dev, tuple(x.shape), x.device))
    oh, ow = valid
    if len(plan["sizes"]) != B or src.dtype != torch.uint8 or src.dim() != 1 or src.device != dev or not src.is_contiguous():
        raise L.AclganError("paste_u8: expected %d staged sources in a contiguous 1-D uint8 buffer on %s" % (B, dev))
    outputs = list(outputs)
    if not outputs or any(n not in ("bar", "mask") for n in outputs):
        raise L.AclganError("paste_u8: outputs must be a non-empty subset of ('bar', 'mask'), got %s" % (outputs,))
    with torch.cuda.device(dev), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
        d, g = _dense(dec), _dense(x)
        res = {}
        for n in outputs:
            t = out[n] if out is not None else torch.empty(plan["total"], dtype=torch.uint8, device=dev)
            if tuple(t.shape) != (plan["total"],) or t.dtype != torch.uint8 or t.device != dev or not t.is_contiguous():
                raise L.AclganError("paste_u8: out[%r] must be a contiguous (%d,) uint8 tensor on %s" % (n, plan["total"], dev))
            res[n] = t
        L.check(L.lib.aclgan_translate_paste_u8(L.ptr(d), d.stride(0) if B > 1 else 0, Cd, L.ptr(g), g.stride(0) if B > 1 else 0, B, oh, ow, PH, PW,
                                                L.ptr(src), src.numel(), plan["descs"], L.ptr(plan["dev"]), L.ptr(res.get("bar")),
                                                L.ptr(res.get("mask")), plan["total"], L.stream_ptr(dev)), "translate_paste_u8")
    return res


DETAILS = ("bilinear", "guided")
GUIDED_RADIUS, GUIDED_EPS = 4, 1e-3          # this project's choice: nobody has measured which values suit the datasets


def guided_u8(dec, x, valid, src, plan, radius=GUIDED_RADIUS, eps=GUIDED_EPS, outputs=("bar", "mask"), out=None, stream=None):
    """paste_u8's pictures by guided-filter upsampling (include/aclgan_hip.h: aclgan_translate_guided_coef, aclgan_translate_guided_paste_u8):
    per window of radius `radius` and per channel an affine model of the residual in the net input is fitted at net resolution
    (regularised by eps), its smoothed coefficients are upsampled and evaluated on the source bytes.  Arguments, outputs and layout are
    paste_u8's; radius is an integer in [1, 16], eps lies in [1e-6, 1].  The coefficient planes (B, 7 or 6, oh, ow) and the scratch are
    allocated here; three launches.  Nothing is synchronised."""
    dev = dec.device
    if dev.type != "cuda":
        raise L.AclganError("guided_u8: tensors must be on the GPU (got %s); there is no CPU path" % dev)
    if dec.dim() != 4 or dec.shape[1] not in (3, 4) or dec.shape[0] < 1:
        raise L.AclganError("guided_u8: expected a (B, 3 or 4, H, W) decoder output, got %s" % (tuple(dec.shape),))
    B, Cd, PH, PW = dec.shape
    if tuple(x.shape) != (B, 3, PH, PW) or x.device != dev:
        raise L.AclganError("guided_u8: expected (%d, 3, %d, %d) net inputs on %s, got %s on %s" % (B, PH, PW, dev, tuple(x.shape), x.device))
    oh, ow = valid
    if len(plan["sizes"]) != B or src.dtype != torch.uint8 or src.dim() != 1 or src.device != dev or not src.is_contiguous():
        raise L.AclganError("guided_u8: expected %d staged sources in a contiguous 1-D uint8 buffer on %s" % (B, dev))
    outputs = list(outputs)
    if not outputs or any(n not in ("bar", "mask") for n in outputs):
        raise L.AclganError("guided_u8: outputs must be a non-empty subset of ('bar', 'mask'), got %s" % (outputs,))
    if "mask" in outputs and Cd == 3:
        raise L.AclganError("guided_u8: the mask picture needs the m plane, which a 3-channel decoder output does not give")
    if int(radius) != radius:
        raise L.AclganError("guided_u8: radius must be an integer, got %r" % (radius,))
    radius, planes = int(radius), 7 if Cd == 4 else 6
    with torch.cuda.device(dev), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
        d, g = _dense(dec), _dense(x)
        res = {}
        for n in outputs:
            t = out[n] if out is not None else torch.empty(plan["total"], dtype=torch.uint8, device=dev)
            if tuple(t.shape) != (plan["total"],) or t.dtype != torch.uint8 or t.device != dev or not t.is_contiguous():
                raise L.AclganError("guided_u8: out[%r] must be a contiguous (%d,) uint8 tensor on %s" % (n, plan["total"], dev))
            res[n] = t
        coef = torch.empty(B, planes, max(oh, 0), max(ow, 0), dtype=torch.float32, device=dev)
        scratch = torch.empty(max(L.lib.aclgan_translate_guided_scratch_bytes(B, oh, ow, radius), 4), dtype=torch.uint8, device=dev)
        L.check(L.lib.aclgan_translate_guided_coef(L.ptr(d), d.stride(0) if B > 1 else 0, Cd, L.ptr(g), g.stride(0) if B > 1 else 0, B, oh, ow, PH, PW,
                                                   radius, eps, L.ptr(coef), L.ptr(scratch), L.stream_ptr(dev)), "translate_guided_coef")
        L.check(L.lib.aclgan_translate_guided_paste_u8(L.ptr(coef), planes, B, oh, ow, L.ptr(src), src.numel(), plan["descs"], L.ptr(plan["dev"]),
                                                       L.ptr(res.get("bar")), L.ptr(res.get("mask")), plan["total"], L.stream_ptr(dev)),
                "translate_guided_paste_u8")
    return res


def translate_batch(trainer, images, styles, a2b=True, with_input=True, multiple=None, sources=None, detail=None, guided_radius=GUIDED_RADIUS,
                    guided_eps=GUIDED_EPS):
    """reference test_batch.py:115,137-142 for a whole batch: ONE encode of images (B, 3, H, W), one decode per style column of styles
    (B, S, style_dim, 1, 1) -- every image has its own style rows -- and the pictures of all of them through finish_u8.
    Reads the weights trainer.ema_weights() selects, as encode / decode do.
    multiple (fit: pad): the images are reflect_pad()ded to multiples of it in front of the generators, and the pictures are finish_u8 of the
    top-left (H, W) crop of the decoder output and of the net input -- strided views, which finish_u8 copies dense.
    sources (full_size): (the staged uint8 device buffer, [(byte offset, src_h, src_w) per image]) -- bar and mask come from paste_u8 at
    every image's own source size instead, packed; there is no input picture.  Returns a dict:
      dec     list of S raw decoder outputs (B, output_dim, PH, PW): the net's shape, (H, W) unless padded
      images  the net input (B, 3, PH, PW) on the device;  valid  (H, W)
      bar     list of S uint8 (B, H, W, 3);  mask  the same when the configuration has a focus channel, else None
      input   uint8 (B, H, W, 3), or None without with_input
      bytes   the one uint8 device buffer (P, B, H, W, 3) all of those are views of, P = S (x 2 with masks) (+ 1 with the input)
    with sources: bar / mask are lists of S uint8 (T,), bytes is (P, T), input None, and 'offsets' / 'sizes' say where image k's
    (src_h, src_w, 3) picture lies in each.
    detail (with sources only): None or 'bilinear' -- paste_u8 -- or 'guided' -- guided_u8(radius=guided_radius, eps=guided_eps)."""
    if detail not in (None,) + DETAILS:
        raise L.AclganError("translate_batch: detail must be one of %s, got %r" % (DETAILS, detail))
    if detail == "guided" and sources is None:
        raise L.AclganError("translate_batch: detail='guided' upsamples the edit to the staged sources' size; without sources there is nothing to upsample")
    gen = trainer.gen_AB if a2b else trainer.gen_BA
    focus = trainer.focus_lam > 0
    images = images.to(trainer.device, torch.float32)
    if images.dim() != 4 or images.shape[1] != 3:
        raise L.AclganError("translate_batch: expected (B, 3, H, W) images, got %s" % (tuple(images.shape),))
    B, _, H, W = images.shape
    if styles.dim() != 5 or styles.shape[0] != B or styles.shape[1] < 1:
        raise L.AclganError("translate_batch: expected (%d, S, style_dim, 1, 1) styles, got %s" % (B, tuple(styles.shape)))
    S = styles.shape[1]
    styles = styles.to(trainer.device, torch.float32)
    padded = multiple is not None and padded_shape((H, W), multiple) != (H, W)
    with torch.no_grad():
        if padded:
            images = reflect_pad(images, multiple)
        content, _ = gen.encode(images)
        per = 2 if focus else 1
        if sources is not None:
            if len(sources[1]) != B:
                raise L.AclganError("translate_batch: %d staged sources for %d images" % (len(sources[1]), B))
            plan = paste_plan(sources[1], trainer.device)
            buf = torch.empty(S * per, plan["total"], dtype=torch.uint8, device=trainer.device)
            res = {"dec": [], "images": images, "valid": (H, W), "bar": [], "mask": [] if focus else None, "input": None, "bytes": buf,
                   "offsets": plan["offsets"], "sizes": plan["sizes"]}
        else:
            buf = torch.empty(S * per + (1 if with_input else 0), B, H, W, 3, dtype=torch.uint8, device=trainer.device)
            res = {"dec": [], "images": images, "valid": (H, W), "bar": [], "mask": [] if focus else None,
                   "input": buf[S * per] if with_input else None, "bytes": buf}
        for j in range(S):
            dec = gen.decode(content, styles[:, j])
            out = {"bar": buf[j * per]}
            if focus:
                out["mask"] = buf[j * per + 1]
            fdec = dec if focus else dec[:, :3]                                              # (test.py: outputs[:, :3] without a focus loss)
            if sources is not None and detail == "guided":
                guided_u8(fdec, images, (H, W), sources[0], plan, radius=guided_radius, eps=guided_eps, outputs=list(out), out=out)
            elif sources is not None:
                paste_u8(fdec, images, (H, W), sources[0], plan, outputs=list(out), out=out)
            else:
                if with_input and j == 0:
                    out["input"] = res["input"]
                if padded:
                    finish_u8(fdec[:, :, :H, :W], images[:, :, :H, :W], outputs=list(out), out=out)
                else:
                    finish_u8(fdec, images, outputs=list(out), out=out)
            res["dec"].append(dec)
            res["bar"].append(out["bar"])
            if focus:
                res["mask"].append(out["mask"])
    return res


# ---- the folder driver ----
def list_files(input_folder, max_images=3000):
    """ImageFolder's files in its (sorted) order, the first max_images of them (the reference stops at 3000; 0: no cap)"""
    try:
        files = ImageFolder(input_folder).imgs
    except (RuntimeError, AssertionError) as e:
        raise L.AclganError("translate_folder: no images to translate in %s (%s)" % (input_folder, str(e).splitlines()[0]))
    return files[:max_images] if max_images and max_images > 0 else files


def image_size(path):
    """(width, height) from the file's header, without decoding it"""
    from PIL import Image
    with Image.open(path) as im:
        return im.size


FITS = ("refuse", "pad")


def plan_batches(files, new_size, multiple, batch_size, size_of=image_size, fit="refuse"):
    """Consecutive files of equal resized shape form a batch of at most batch_size; a change of shape closes the batch.  Raises before
    anything runs for a file whose resized H or W is no multiple of `multiple` (2 ** gen.n_downsample: the decoder would return another size
    than the encoder was given, and the blend with the input would fail) -- unless fit is 'pad': then the net input is the resized shape
    with each side rounded up to the next multiple, and only a side below `multiple` is refused (reflection would need more than the image
    holds).  Returns a list of batches, each a list of (index, path, (H, W), (PH, PW)): the resized shape and the net's."""
    if batch_size < 1:
        raise L.AclganError("translate_folder: batch_size must be positive, got %d" % batch_size)
    if fit not in FITS:
        raise L.AclganError("translate_folder: fit must be one of %s, got %r" % (FITS, fit))
    batches, cur = [], []
    for i, path in enumerate(files):
        w, h = size_of(path)
        ow, oh = resized_size(w, h, new_size)
        if fit == "pad":
            if oh < multiple or ow < multiple:
                raise L.AclganError("translate_folder: %s is %dx%d (H x W) after Resize(%s); padding by reflection to multiples of %d needs "
                                    "at least %d pixels a side" % (path, oh, ow, new_size, multiple, multiple))
        elif oh % multiple or ow % multiple:
            raise L.AclganError("translate_folder: %s is %dx%d (H x W) after Resize(%s); the generators take multiples of %d"
                                % (path, oh, ow, new_size, multiple))
        if cur and (cur[0][2] != (oh, ow) or len(cur) == batch_size):
            batches.append(cur)
            cur = []
        cur.append((i, path, (oh, ow), padded_shape((oh, ow), multiple)))
    if cur:
        batches.append(cur)
    return batches


def draw_styles(n_images, num_style, style_dim, synchronized=False):
    """The reference's draws in its order, from torch's CPU default generator (test_batch.py:105,117): style_fixed = randn(3 num_style, ...)
    first, then -- unless synchronized -- one randn(3 num_style, ...) per image in folder order; every draw times 2, style j = row 3 j (the
    rows 3 j + 1 and 3 j + 2 feed the cycle passes that are not run).  Returns (n_images, num_style, style_dim, 1, 1) on the host: the
    values depend on the folder order only, never on how the images are grouped into batches."""
    fixed = torch.randn(num_style * 3, style_dim, 1, 1)
    rows = []
    for _ in range(n_images):
        s = fixed if synchronized else torch.randn(num_style * 3, style_dim, 1, 1)
        rows.append((s * 2)[0::3])
    return torch.stack(rows) if rows else torch.empty(0, num_style, style_dim, 1, 1)


def output_paths(output_folder, path, index, num_style, focus, output_only=False):
    """the files one input produces (test_batch.py:161-163,181,194): {'bar': [S paths], 'mask': [S paths] or None, 'input': path or None}"""
    base = os.path.basename(path)
    return {"bar": [os.path.join(output_folder, "_%02d_bar" % j, base) for j in range(num_style)],
            "mask": [os.path.join(output_folder, "_%02d_mask" % j, base) for j in range(num_style)] if focus else None,
            "input": None if output_only else os.path.join(output_folder, "input%03d.jpg" % index)}


def _save(arr, path):
    from PIL import Image
    Image.fromarray(arr).save(path)          # the format follows the extension, as in torchvision's save_image


def _save_source(im, path):
    _save(np.asarray(im, dtype=np.uint8), path)     # a decoded image (PIL or array) as the host array it is


def _to_host(t):
    """one copy of a batch's bytes into pinned memory; the caller's stream has finished when it returns"""
    if not t.is_cuda:
        return t
    host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    host.copy_(t, non_blocking=True)
    torch.cuda.current_stream(t.device).synchronize()
    return host


def translate_folder(trainer, config, input_folder, output_folder, a2b=True, num_style=1, synchronized=False, output_only=False,
                     batch_size=8, max_images=3000, keep_float=False, forward=None, transform=None, fit="refuse", full_size=False,
                     detail="bilinear", guided_radius=GUIDED_RADIUS, guided_eps=GUIDED_EPS):
    """The reference's test_batch.py loop.  Per input file <out>/_%02d_bar/<basename> for every style, <out>/_%02d_mask/<basename> when
    focus_loss > 0, <out>/input%03d.jpg unless output_only.  The passes whose saves the reference has commented out (_hat, _til) are not run.
    forward(trainer, images, styles, a2b, with_input) / transform(list of decoded images): the device halves (translate_batch and
    GpuBatchTransform(new_size, train=False, crop=False)); replaceable, so that the planning can be checked where there is no GPU.
    fit: 'refuse' (a resized shape that is no multiple of 2 ** n_downsample raises by name) or 'pad' (it is padded by reflection in front of
    the generators and the pictures are the crop; forward is given multiple=).  full_size: bar and mask are written at every source file's
    own decoded size -- the edit pasted onto the source pixels -- and input%03d.jpg is the decoded source; the transform is then used
    through its stage() / launch() halves and forward is given sources=transform.sources(staged state).  With both off the calls
    are exactly those above.
    detail: how the edit reaches the source's size under full_size -- 'bilinear' (the residual interpolated: paste_u8; forward is given no
    further keyword) or 'guided' (guided_u8 with guided_radius and guided_eps: forward is given detail=, guided_radius=, guided_eps=).
    'guided' without full_size is refused: the pictures are then written at the net's size, and there is nothing to upsample.
    Returns a list of (path, (H, W), batch index) records in folder order, (H, W) the resized shape; with keep_float (for tests) a pair of
    that list and {path: {'dec': [S tensors (C, PH, PW)], 'input': (3, PH, PW), 'valid': (H, W)}} on the host, (PH, PW) the net's shape."""
    gen_cfg = config["gen"]
    focus = config["focus_loss"] > 0
    if "new_size" in config:
        new_size = config["new_size"]
    else:
        new_size = config["new_size_a"] if a2b else config["new_size_b"]
    if num_style < 1:
        raise L.AclganError("translate_folder: num_style must be positive, got %d" % num_style)
    if detail not in DETAILS:
        raise L.AclganError("translate_folder: detail must be one of %s, got %r" % (DETAILS, detail))
    if detail == "guided" and not full_size:
        raise L.AclganError("translate_folder: detail='guided' needs full_size: without it the pictures are written at the net's size, "
                            "and there is nothing to upsample")
    files = list_files(input_folder, max_images)
    multiple = 2 ** gen_cfg["n_downsample"]
    batches = plan_batches(files, new_size, multiple, batch_size, fit=fit)
    styles = draw_styles(len(files), num_style, gen_cfg["style_dim"], synchronized)
    if forward is None:
        forward = translate_batch
    if transform is None:
        transform = GpuBatchTransform(new_size, None, None, train=False, crop=False, device=trainer.device)
    paths = [output_paths(output_folder, p, i, num_style, focus, output_only) for i, p in enumerate(files)]
    for d in sorted({os.path.dirname(q) for o in paths for q in o["bar"] + (o["mask"] or []) + ([o["input"]] if o["input"] else [])}):
        os.makedirs(d, exist_ok=True)

    records, floats, pending = [], {}, []
    pool = ThreadPoolExecutor(max_workers=min(MAX_WORKERS, max(4, 2 * batch_size)))
    try:
        decode = lambda b: [pool.submit(default_loader, p) for _, p, _, _ in batches[b]]
        nxt = decode(0)
        extra = {"multiple": multiple} if fit == "pad" else {}
        if detail == "guided":
            extra.update(detail="guided", guided_radius=guided_radius, guided_eps=guided_eps)
        for b, batch in enumerate(batches):
            cur = nxt
            nxt = decode(b + 1) if b + 1 < len(batches) else None      # the decode of batch b+1 overlaps everything below
            idx = [i for i, _, _, _ in batch]
            decoded = [f.result() for f in cur]
            if full_size:
                if not all(hasattr(transform, n) for n in ("stage", "launch", "sources")):
                    raise L.AclganError("translate_folder: full_size needs a transform with stage(), launch() and sources() (GpuBatchTransform)")
                st = transform.stage(decoded)                           # the one upload: the paste reads the bytes the resize kernel reads
                images = transform.launch(st)
                extra["sources"] = transform.sources(st)
                res = forward(trainer, images, styles[idx], a2b, False, **extra)
            else:
                images = transform(decoded)
                res = forward(trainer, images, styles[idx], a2b, not output_only, **extra)
            host = _to_host(res["bytes"]).numpy()                       # (P, B, H, W, 3): the one device->host copy of this batch
            if full_size:                                               # (P, T): every picture at its source's size, packed
                sizes = [(h, w) for _, h, w in extra["sources"][1]]
                if host.ndim != 2 or list(res["sizes"]) != sizes:
                    raise L.AclganError("translate_folder: batch %d came back as %s for sources of %s" % (b, res.get("sizes"), sizes))
            elif tuple(host.shape[2:4]) != batch[0][2]:
                raise L.AclganError("translate_folder: batch %d came back as %s for %s images" % (b, tuple(host.shape[2:4]), batch[0][2]))
            for f in pending:                                           # the encodes of batch b-1 ran during this batch's forward
                f.result()
            pending = []
            per = 2 if focus else 1
            for k, (i, path, shape, _) in enumerate(batch):
                o = paths[i]
                if full_size:
                    (hs, ws), off = sizes[k], res["offsets"][k]
                    pic = lambda p: host[p, off:off + hs * ws * 3].reshape(hs, ws, 3)
                else:
                    pic = lambda p: host[p, k]
                for j in range(num_style):
                    pending.append(pool.submit(_save, pic(j * per), o["bar"][j]))
                    if focus:
                        pending.append(pool.submit(_save, pic(j * per + 1), o["mask"][j]))
                if o["input"]:
                    if full_size:                                       # the decoded source as it is, from the host array
                        pending.append(pool.submit(_save_source, decoded[k], o["input"]))
                    else:
                        pending.append(pool.submit(_save, pic(num_style * per), o["input"]))
                records.append((path, shape, b))
                if keep_float:
                    floats[path] = {"dec": [d[k].detach().cpu() for d in res["dec"]], "input": res["images"][k].detach().cpu(),
                                    "valid": tuple(res.get("valid", shape))}
        for f in pending:
            f.result()
    finally:
        pool.shutdown(wait=True)
    return (records, floats) if keep_float else records
