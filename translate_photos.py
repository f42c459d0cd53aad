#!/usr/bin/env python3
"""translate_photos.py -- test_batch.py for photographs: the same flags, the same files, plus the two switches that let a folder of
pictures of any shape through and return the edit at each picture's own size (acl-gan_amd/translate.py, csrc/paste.hip, csrc/guided.hip):

  --fit refuse|pad   a resized shape that is no multiple of 2 ** n_downsample: refused by name as in test_batch.py (default), or padded by
                     reflection in front of the generators, the written pictures cropped back to the resized shape
  --full_size        <output_folder>/_%02d_bar and _%02d_mask at each source file's own decoded size -- the edit added onto the source
                     pixels -- and input%03d.jpg as the decoded source
  --detail bilinear|guided   with --full_size: the edit interpolated bilinearly to the source's size (default), or upsampled by a guided
                     filter, so that the photograph's own detail passes through the edit; --guided_radius R (1..16, default 4) and
                     --guided_eps E (1e-6..1, default 1e-3) are its window and its regulariser

With neither switch the run is test_batch.py's, file for file.  --full_size without --fit pad still refuses ragged shapes; --detail guided
without --full_size is refused: at net size there is nothing to upsample.
"""
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import test_batch  # noqa: E402  (the folder script: its flags are this script's)


def parser():
    ap = test_batch.parser()
    ap.description = "translate a folder of photographs in batches"
    ap.add_argument("--fit", type=str, default="refuse", choices=("refuse", "pad"),
                    help="a resized shape that is no multiple of 2 ** n_downsample: refuse the file by name, or pad it by reflection and crop the pictures")
    ap.add_argument("--full_size", action="store_true",
                    help="write _bar and _mask at each source file's own size: the edit pasted onto the source pixels (input%%03d.jpg: the source)")
    ap.add_argument("--detail", type=str, default="bilinear", choices=("bilinear", "guided"),
                    help="with --full_size: interpolate the edit bilinearly to the source's size, or upsample it by a guided filter that keeps the "
                         "photograph's own detail inside the edit")
    ap.add_argument("--guided_radius", type=int, default=4, help="--detail guided: window radius at net resolution, 1 to 16")
    ap.add_argument("--guided_eps", type=float, default=1e-3, help="--detail guided: regulariser of the local model, 1e-6 to 1")
    return ap


def main(argv=None):
    opts = parser().parse_args(argv)
    if opts.trainer != "aclgan":
        sys.exit("Only support aclgan")
    if opts.compute_IS or opts.compute_CIS:
        sys.exit("--compute_IS / --compute_CIS: no pretrained Inception network is available or ported; compute the scores on the written files")
    if opts.detail == "guided" and not opts.full_size:
        sys.exit("--detail guided needs --full_size: at net size there is nothing to upsample")
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
                               max_images=opts.max_images, fit=opts.fit, full_size=opts.full_size, detail=opts.detail,
                               guided_radius=opts.guided_radius, guided_eps=opts.guided_eps)
    torch.cuda.synchronize()
    print("translated %d images in %d batches -> %s" % (len(records), records[-1][2] + 1, opts.output_folder))


if __name__ == "__main__":
    main()
