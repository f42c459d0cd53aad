#!/usr/bin/env python3
"""Generate tests/golden/index_reference.html by calling THE REFERENCE's own utils.write_html.

    python tests/golden/make_golden_visual.py <path to the reference checkout>

The fixture is a file the reference wrote (data only, no reference source travels): index.html as train.py:90 produces it after
iteration 30000 with image_save_iter 10000 and the picture directory 'images'.  acl-gan_amd/visual.py:write_html must write the
same text for the same arguments (tests/test_visual_cpu.py).

The reference's utils.py imports torchvision at module level; the same empty stub modules as in make_golden.py stand in for it
(write_html touches none of it).
"""
import os
import shutil
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))

ITERATIONS, IMAGE_SAVE_ITER, IMAGE_DIRECTORY = 30000, 10000, "images"


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "utils.py")):
        sys.exit(__doc__)
    for m in ["torchvision", "torchvision.transforms", "torchvision.utils", "torchvision.models", "torchvision.datasets"]:
        sys.modules[m] = types.ModuleType(m)
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    sys.modules["torchvision"].utils = sys.modules["torchvision.utils"]
    sys.modules["torchvision"].models = sys.modules["torchvision.models"]
    sys.path.insert(0, sys.argv[1])
    import utils as ref_utils      # the reference
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "index.html")      # the title carries the file's base name (utils.py:160)
        ref_utils.write_html(path, ITERATIONS, IMAGE_SAVE_ITER, IMAGE_DIRECTORY)
        shutil.copyfile(path, os.path.join(HERE, "index_reference.html"))
    print("wrote", os.path.join(HERE, "index_reference.html"))


if __name__ == "__main__":
    main()
