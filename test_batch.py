#!/usr/bin/env python3
"""test_batch.py -- counterpart of the reference's folder inference script on the MI355X-native generators: translates every image of
--input_folder and writes, per input and per style j,

  <output_folder>/_%02d_bar/<basename>    the translated image, blended with the input through the focus mask
  <output_folder>/_%02d_mask/<basename>   the focus mask (configurations with focus_loss > 0)
  <output_folder>/input%03d.jpg           the resized input (unless --output_only)

These are the files FID / KID are computed on.  What runs where: image decode and the JPEG / PNG encoders stay on the host (thread pool);
Resize / ToTensor / Normalize, encode(), decode(), the focus blend and save_image's normalisation to bytes run on the device for a whole
batch at a time (acl-gan_amd/translate.py, csrc/finish.hip); one device->host copy of the bytes per batch.  With --batch_size 1 the files
are byte-identical to what test.py writes for the same image and style.

The reference's cycle passes (_hat, _til), whose saves it has commented out, are not run.  --compute_IS / --compute_CIS need a pretrained
Inception network that is neither shipped nor ported: they exit with a message.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

DEFAULT_BATCH_SIZE = 32      # the fastest of 1 / 8 / 32 measured (profiles/translate_folder.json)


def parser():
    ap = argparse.ArgumentParser(description="translate a folder of images in batches")
    ap.add_argument("--config", type=str, help="net configuration")
    ap.add_argument("--input_folder", type=str, help="input image folder")
    ap.add_argument("--output_folder", type=str, help="output image folder")
    ap.add_argument("--checkpoint", type=str, help="checkpoint of autoencoders (gen_XXXXXXXX.pt or ema_XXXXXXXX.pt)")
    ap.add_argument("--a2b", type=int, default=1, help="1 for a2b and 0 for b2a")
    ap.add_argument("--seed", type=int, default=1, help="random seed")
    ap.add_argument("--num_style", type=int, default=1, help="number of styles to sample")
    ap.add_argument("--synchronized", action="store_true", help="whether use synchronized style code or not")
    ap.add_argument("--output_only", action="store_true", help="whether only save the output images or also save the input images")
    ap.add_argument("--output_path", type=str, default=".", help="path for logs, checkpoints, and VGG model weight")
    ap.add_argument("--trainer", type=str, default="aclgan", help="aclgan")
    ap.add_argument("--compute_IS", action="store_true", help="not supported: no Inception network is available")
    ap.add_argument("--compute_CIS", action="store_true", help="not supported: no Inception network is available")
    ap.add_argument("--batch_size", type=int, default=DEFAULT_BATCH_SIZE, help="images of equal size translated together")
    ap.add_argument("--max_images", type=int, default=3000, help="translate the first N images of the folder (0: all)")
    return ap


def main(argv=None):
    opts = parser().parse_args(argv)
    if opts.trainer != "aclgan":
        sys.exit("Only support aclgan")
    if opts.compute_IS or opts.compute_CIS:
        sys.exit("--compute_IS / --compute_CIS: no pretrained Inception network is available or ported; compute the scores on the written files")
    for name in ("config", "input_folder", "output_folder", "checkpoint"):
        if getattr(opts, name) is None:
            sys.exit("--%s is required" % name)

    import torch
    import yaml
    import aclgan_amd  # noqa: F401
    from aclgan_amd.trainer import aclgan_Trainer
    from aclgan_amd.translate import translate_folder

    torch.manual_seed(opts.seed)
    with open(opts.config) as f:
        config = yaml.safe_load(f)
    trainer = aclgan_Trainer(config)
    state_dict = torch.load(opts.checkpoint, map_location="cpu")      # {'AB': ..., 'BA': ...}
    trainer.gen_AB.load_state_dict(state_dict["AB"])
    trainer.gen_BA.load_state_dict(state_dict["BA"])
    trainer.cuda()
    trainer.eval()
    records = translate_folder(trainer, config, opts.input_folder, opts.output_folder, a2b=bool(opts.a2b), num_style=opts.num_style,
                               synchronized=opts.synchronized, output_only=opts.output_only, batch_size=opts.batch_size,
                               max_images=opts.max_images)
    torch.cuda.synchronize()
    print("translated %d images in %d batches -> %s" % (len(records), records[-1][2] + 1, opts.output_folder))


if __name__ == "__main__":
    main()
