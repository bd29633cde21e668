"""Orientation maps of a directory of images: the files of the reference's src/preprocessing/calc_orientation_maps.py, from
gaussianhaircut_amd.orientation (HIP kernels on a ROCm device; --torch: the PyTorch-composed form, any device).

    python tools/orientation_maps.py --img_path DATA/images_2 --mask_path DATA/masks_2/hair --out_dir DATA/orientations_2

Per image NAME.* it writes, as the reference does:
    angles/NAME.png         deg as uint8
    vars/NAME.npy           the variance as float16
    filtered_imgs/NAME.png  (f - min) / (max - min) * 255 of the difference of Gaussians, truncated to uint8
    vis_imgs/NAME.png       the four-colour wheel times the hair mask; the reference writes it with cv2.imwrite, which takes the
                            array as B, G, R, so the file's red and blue are swapped against the array -- kept
Without --mask_path the wheel is not masked.  --orient_dir / --conf_dir / --filtered_img_dir / --vis_img_dir override the four
directories one by one (the reference's argument names)."""
import argparse
import os
import sys

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussianhaircut_amd import orientation as ori  # noqa: E402


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--img_path", required=True)
    ap.add_argument("--mask_path", default=None)
    ap.add_argument("--out_dir", default=None)
    ap.add_argument("--orient_dir", default=None)
    ap.add_argument("--conf_dir", default=None)
    ap.add_argument("--filtered_img_dir", default=None)
    ap.add_argument("--vis_img_dir", default=None)
    ap.add_argument("--dog_low", type=float, default=0.4)
    ap.add_argument("--dog_high", type=float, default=10.0)
    ap.add_argument("--num_filters", type=int, default=180)
    ap.add_argument("--patch_size", type=int, default=64, help="of the --torch form; changes no value")
    ap.add_argument("--torch", action="store_true", help="the PyTorch-composed form (fused=False)")
    ap.add_argument("--device", default=None, help="default: cuda:0 when there is one")
    a = ap.parse_args(argv)
    dirs = {}
    for key, sub in (("orient_dir", "angles"), ("conf_dir", "vars"), ("filtered_img_dir", "filtered_imgs"), ("vis_img_dir", "vis_imgs")):
        d = getattr(a, key) or (os.path.join(a.out_dir, sub) if a.out_dir else None)
        if d is None:
            ap.error("--out_dir or --%s is needed" % key)
        os.makedirs(d, exist_ok=True)
        dirs[key] = d
    dev = torch.device(a.device if a.device else ("cuda:0" if torch.cuda.is_available() else "cpu"))
    if dev.type != "cuda" and not a.torch:
        ap.error("the kernels need a ROCm device; pass --torch for the PyTorch-composed form")
    bank = ori.gabor_bank(a.num_filters)
    names = sorted(os.listdir(a.mask_path if a.mask_path else a.img_path))
    for name in names:
        base = name.split(".")[0]
        img = np.array(Image.open(os.path.join(a.img_path, name)))
        if img.ndim == 3:
            img = img[:, :, :3]
        m = ori.orientation_maps(torch.from_numpy(np.ascontiguousarray(img)).to(dev), a.dog_low, a.dog_high, bank=bank,
                                 fused=not a.torch, patch_size=a.patch_size)
        deg, var = m.deg.cpu().numpy(), m.var.cpu().numpy()
        if a.mask_path:
            mask = np.asarray(Image.open(os.path.join(a.mask_path, name))) / 255.
            if mask.ndim == 3:
                mask = mask[:, :, 0]
        else:
            mask = np.ones(deg.shape)
        Image.fromarray(deg).save(os.path.join(dirs["orient_dir"], base + ".png"))
        np.save(os.path.join(dirs["conf_dir"], base + ".npy"), var.astype(np.float16))
        Image.fromarray(ori.filtered_to_u8(m.filtered)).save(os.path.join(dirs["filtered_img_dir"], base + ".png"))
        Image.fromarray(np.ascontiguousarray(ori.vis_orientation(deg, mask)[:, :, ::-1])).save(os.path.join(dirs["vis_img_dir"], base + ".png"))
    return len(names)


if __name__ == "__main__":
    print("wrote the maps of %d images" % main())
