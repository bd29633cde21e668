"""The half- and quarter-size folders of a scene: the files of the reference's src/preprocessing/resize_images.py, from
gaussianhaircut_amd.ground_truth (HIP kernels on a ROCm device; --fused 0: the same fixed-point arithmetic composed from torch
integer operations, any device).  Both give Pillow's bicubic bytes.

    python tools/resize_images.py --data_path DATA

Reads DATA/images/NAME.*, DATA/masks/{hair,body}/NAME.png and, where it exists, DATA/masks/face/NAME.png; the names come from
DATA/iqa_filtered_names.pkl when that file exists, else from the images directory.  A frame whose hair and face masks overlap on
more than 0.1 of the body mask's pixels is skipped (and said so), as the reference skips it.  Writes, each resized from the
original: images_2/, images_4/, masks_2/{hair,body}/, masks_4/{hair,body}/, all under the image's file name.  An RGBA image
is refused: Pillow premultiplies alpha there, which is not built."""
import argparse
import os
import pickle
import sys

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussianhaircut_amd import ground_truth as gt  # noqa: E402

FACTORS = (2, 4)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data_path", required=True)
    ap.add_argument("--fused", type=int, default=1, help="0: the torch-composed comparator")
    ap.add_argument("--device", default=None, help="default: cuda:0 when there is one")
    a = ap.parse_args(argv)
    data = a.data_path
    dev = torch.device(a.device if a.device else ("cuda:0" if torch.cuda.is_available() else "cpu"))
    if dev.type != "cuda" and a.fused:
        ap.error("the kernels need a ROCm device; pass --fused 0 for the torch-composed form")
    names_file = os.path.join(data, "iqa_filtered_names.pkl")
    if os.path.exists(names_file):
        with open(names_file, "rb") as f:
            names = pickle.load(f)
    else:
        names = os.listdir(os.path.join(data, "images"))
    for f in FACTORS:
        for sub in ("images_%d" % f, "masks_%d/hair" % f, "masks_%d/body" % f):
            os.makedirs(os.path.join(data, sub), exist_ok=True)
    written = 0
    for name in names:
        base = name.split(".")[0]
        img = np.array(Image.open(os.path.join(data, "images", name)))
        hair = np.array(Image.open(os.path.join(data, "masks", "hair", base + ".png")))
        body = np.array(Image.open(os.path.join(data, "masks", "body", base + ".png")))
        face_path = os.path.join(data, "masks", "face", base + ".png")
        if os.path.exists(face_path) and gt.frame_is_skipped(hair, body, np.asarray(Image.open(face_path))):
            print("Skipping frame %s" % name)
            continue
        pyr = gt.resize_pyramid(*(np.ascontiguousarray(x) for x in (img, hair, body)), factors=FACTORS, fused=bool(a.fused), device=dev)
        for f, (i, h, b) in pyr.items():
            Image.fromarray(i).save(os.path.join(data, "images_%d" % f, name))
            Image.fromarray(h).save(os.path.join(data, "masks_%d" % f, "hair", name))
            Image.fromarray(b).save(os.path.join(data, "masks_%d" % f, "body", name))
        written += 1
    return written


if __name__ == "__main__":
    print("wrote the folders of %d frames" % main())
