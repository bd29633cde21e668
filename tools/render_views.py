"""Render a set of views and write the seven products of the reference's render_set (src/render_gaussians.py:31-68) in its
directory layout:

    <model_path>/<name>/ours_<iteration>/{renders,hair_masks,head_masks,orients,orients_vis,orient_confs_vis}/<view>.png
    <model_path>/<name>/ours_<iteration>/orient_confs/<view>.pth

The 8-bit images come from gaussianhaircut_amd.evaluation.render_products (one kernel launch and one device-to-host copy per
view) and are written with PIL; single-channel products are replicated to RGB at write time, so the files hold what
torchvision's save_image writes for a one-channel tensor.  The .pth file is the float [1,H,W] tensor the reference saves.

    python tools/render_views.py --model_path OUT --ply point_cloud.ply --views 16 --width 1920 --height 1080
    python tools/render_views.py --model_path OUT --config tiny --views 4          # a synthetic model of utils.synthetic

Cameras are the ring of scene.cameras.ring_cameras (this package has no dataset reader); a script with its own cameras calls
``write_products`` below with them.  ``--torch`` runs the PyTorch-composed comparator instead of the kernels."""
import argparse
import os
import sys

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussianhaircut_amd import evaluation as ev  # noqa: E402
from gaussianhaircut_amd.scene.cameras import ring_cameras  # noqa: E402
from gaussianhaircut_amd.scene.gaussian_model import GaussianModel  # noqa: E402
from gaussianhaircut_amd.utils import synthetic as syn  # noqa: E402

DIRS = dict(render="renders", hair_mask="hair_masks", head_mask="head_masks", orient="orients", orient_vis="orients_vis",
            orient_conf="orient_confs", orient_conf_vis="orient_confs_vis")


def write_products(model_path, name, iteration, products, scene_suffix=""):
    """products: the iterator of evaluation.render_products.  Returns the number of views written."""
    base = os.path.join(model_path, "%s%s" % (name, scene_suffix), "ours_{}".format(iteration))
    for d in DIRS.values():
        os.makedirs(os.path.join(base, d), exist_ok=True)
    n = 0
    for idx, p in enumerate(products):
        stem = os.path.basename(str(p.get("name") or "%05d" % idx)).split(".")[0]
        for k in ev.PRODUCTS:
            a = p[k]
            if a.ndim == 2:
                a = np.repeat(a[:, :, None], 3, axis=2)
            Image.fromarray(a, "RGB").save(os.path.join(base, DIRS[k], stem + ".png"))
        torch.save(torch.from_numpy(np.array(p["orient_conf"]))[None], os.path.join(base, DIRS["orient_conf"], stem + ".pth"))
        n += 1
    return n


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model_path", required=True)
    ap.add_argument("--ply")
    ap.add_argument("--config", default="tiny", choices=sorted(syn.CONFIGS))
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--width", type=int)
    ap.add_argument("--height", type=int)
    ap.add_argument("--name", default="test")
    ap.add_argument("--iteration", type=int, default=0)
    ap.add_argument("--scene_suffix", default="")
    ap.add_argument("--white_background", action="store_true")
    ap.add_argument("--torch", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    spec = syn.CONFIGS[a.config]
    if a.ply:
        model = GaussianModel(3)
        model.load_ply(a.ply, device=dev)
    else:
        model = syn.make_model(spec, dev)
    W, H = a.width or spec.W, a.height or spec.H
    cams = ring_cameras(a.views, W, H, device=dev)
    for k, cam in enumerate(cams):
        cam.image_name = "%05d" % k
    bg = torch.tensor(([1, 1, 1] if a.white_background else [0, 0, 0]) + [0, 0, 0, 0, 0, 0, 100], dtype=torch.float32, device=dev)
    n = write_products(a.model_path, a.name, a.iteration, ev.render_products(model, cams, bg, fused=not a.torch, copy=False),
                       a.scene_suffix)
    print("wrote %d views under %s" % (n, os.path.join(a.model_path, a.name + a.scene_suffix, "ours_%d" % a.iteration)))


if __name__ == "__main__":
    main()
