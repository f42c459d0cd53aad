"""The files a long run is judged from (reference train.py:78-95, utils.py:115-178): sample picture grids, the HTML index
over them and the loss log.

image_grid / write_2images   the tuple trainer.sample() returns -> ONE uint8 picture on the device (csrc/grid.hip through
                             aclgan_image_grid_u8: global min / max, normalisation, grid layout, rounding to bytes), one
                             device->host copy of the bytes, Pillow's JPEG encoder on the host
write_html                   index.html, the same text the reference writes for the same arguments
LossLog                      logs/<model>/losses.csv: the 16 values of _lib.LOSS_NAMES per logged iteration (the reference
                             feeds the same members to a tensorboardX SummaryWriter; no event files are written here)
"""
import os

import torch

from . import _lib as L


def _dense(t):
    """fp32, every image's C*H*W block contiguous, any batch stride (channel slices of a decoder output pass as they are)"""
    t = t.to(torch.float32)
    _, _, H, W = t.shape
    ok = t.stride(3) == 1 and t.stride(2) == W and t.stride(1) == H * W and t.stride(0) >= 0
    return t if ok else t.contiguous()


def image_grid(tensors, nrow, stream=None):
    """utils.py:116-119 (expand to 3 channels, cat, torchvision 0.4.0 make_grid(nrow=nrow, padding=0, normalize=True),
    save_image's conversion to bytes) on the device.

    tensors: (n_k, C_k, H, W) device tensors, C_k in {1, 3}, equal H and W: the tuple trainer.sample() returns.
    Returns torch.uint8 (rows*H, cols*W, 3) on the tensors' device, cols = min(nrow, N), rows = ceil(N / cols).
    stream: the torch.cuda.Stream to launch on (default: the current stream of that device).  Nothing is synchronised."""
    tensors = [t for t in tensors if t.numel() > 0]
    if not tensors:
        raise L.AclganError("image_grid: no images")
    dev = tensors[0].device
    if dev.type != "cuda":
        raise L.AclganError("image_grid: tensors must be on the GPU (got %s); there is no CPU path" % dev)
    H, W = tensors[0].shape[-2:]
    for t in tensors:
        if t.dim() != 4 or t.device != dev or tuple(t.shape[-2:]) != (H, W):
            raise L.AclganError("image_grid: expected (n, C, %d, %d) tensors on %s, got %s on %s" % (H, W, dev, tuple(t.shape), t.device))
    if len(tensors) > L.GRID_MAX_SRCS:
        raise L.AclganError("image_grid: %d tensors (at most %d)" % (len(tensors), L.GRID_MAX_SRCS))
    if int(nrow) <= 0:
        raise L.AclganError("image_grid: nrow must be positive")
    with torch.cuda.device(dev), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
        srcs = [_dense(t) for t in tensors]       # (kept alive until the launches are enqueued; the caching allocator is stream-ordered)
        N = sum(t.shape[0] for t in srcs)
        cols = min(int(nrow), N)
        rows = (N + cols - 1) // cols
        out = torch.empty(rows * H, cols * W, 3, dtype=torch.uint8, device=dev)
        scratch = torch.empty(L.lib.aclgan_image_grid_scratch_bytes(), dtype=torch.uint8, device=dev)
        arr = (L.GridSrc * len(srcs))(*[L.GridSrc(t.data_ptr(), t.stride(0) if t.shape[0] > 1 else 0, t.shape[0], t.shape[1]) for t in srcs])
        L.check(L.lib.aclgan_image_grid_u8(arr, len(srcs), H, W, int(nrow), L.ptr(out), L.ptr(scratch), L.stream_ptr(dev)), "image_grid_u8")
    return out


def write_2images(image_outputs, display_image_num, image_directory, postfix):
    """utils.py:122-124: the first display_image_num images of every tensor, one tensor per row, as
    <image_directory>/gen_a2b_<postfix>.jpg.  One device->host copy (the bytes); the encoder call is torchvision's own
    (Image.fromarray(ndarr).save(filename))."""
    from PIL import Image
    grid = image_grid([images[:display_image_num] for images in image_outputs], display_image_num)
    os.makedirs(image_directory, exist_ok=True)
    Image.fromarray(grid.cpu().numpy()).save("%s/gen_a2b_%s.jpg" % (image_directory, postfix))


def display_stack(dataset, display_size):
    """train.py:44-47: the first display_size transformed samples of a loader's dataset, stacked.  The transform draws its flip and
    crop from Python's global `random` (data.py GpuBatchTransform.draw); its state is put back, so that a run with pictures reads
    the same random stream during training as a run without."""
    import random
    state = random.getstate()
    try:
        return torch.stack([dataset[i] for i in range(display_size)])
    finally:
        random.setstate(state)


def write_html(filename, iterations, image_save_iterations, image_directory, all_size=1536):
    """utils.py:139-171: index.html -- the two 'current' pictures, then for every saved iteration from the newest down the
    a2b / b2a test and train pictures.  The b2a files are linked although nothing writes them, as in the reference."""
    def row(it, name):
        path = "%s/%s" % (image_directory, name)
        return ("<h3>iteration [%d] (%s)</h3>" % (it, path.split("/")[-1]) +
                "\n        <p><a href=\"%s\">\n          <img src=\"%s\" style=\"width:%dpx\">\n        </a><br>\n        <p>\n        " % (path, path, all_size))
    head = ("\n    <!DOCTYPE html>\n    <html>\n    <head>\n      <title>Experiment name = %s</title>\n"
            "      <meta http-equiv=\"refresh\" content=\"30\">\n    </head>\n    <body>\n    " % os.path.basename(filename))
    parts = [head, "<h3>current</h3>"]
    parts += [row(iterations, "gen_%s_train_current.jpg" % d) for d in ("a2b", "b2a")]
    saved = [j for j in range(iterations, image_save_iterations - 1, -1) if j % image_save_iterations == 0]
    parts += [row(j, "gen_%s_%s_%08d.jpg" % (d, split, j)) for j in saved for split in ("test", "train") for d in ("a2b", "b2a")]
    parts.append("</body></html>")
    with open(filename, "w") as f:
        f.write("".join(parts))


class LossLog:
    """CSV of the losses: a header (`iteration` and the 16 names of _lib.LOSS_NAMES), then one line per logged iteration.  An existing
    file is appended to and keeps its header, so a resumed run continues the log of the run it resumes.  Every line is flushed: a
    killed run keeps what it logged."""

    def __init__(self, path):
        self.path = path
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        fresh = not os.path.exists(path) or os.path.getsize(path) == 0
        self._f = open(path, "a")
        if fresh:
            self._f.write(",".join(["iteration"] + L.LOSS_NAMES) + "\n")
            self._f.flush()

    def append(self, iteration, values):
        """iteration: the 1-based count the reference logs under (iterations + 1); values: the 16 losses in LOSS_NAMES order (the
        host copy of trainer._losses).  %.9g round-trips fp32."""
        values = [float(v) for v in values]
        if len(values) != len(L.LOSS_NAMES):
            raise ValueError("LossLog.append: %d values for %d losses" % (len(values), len(L.LOSS_NAMES)))
        self._f.write(",".join(["%d" % iteration] + ["%.9g" % v for v in values]) + "\n")
        self._f.flush()

    def close(self):
        self._f.close()
