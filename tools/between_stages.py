"""The three steps the reference's run.sh takes between its training stages, on the reference's directory layout:

    python tools/between_stages.py crop   --model_path M --path_to_data D [--iter 30000]
        M/point_cloud/iteration_N/raw_point_cloud.ply -> M/point_cloud_cropped/iteration_N/point_cloud.ply (+ raw_), D/scale.pickle
    python tools/between_stages.py filter --model_path M --mesh HEAD.obj [--iter 30000] [--probe reference]
        M/point_cloud_cropped/iteration_N/raw_point_cloud.ply -> M/point_cloud_filtered/iteration_N/point_cloud.ply (+ raw_)
    python tools/between_stages.py export --points P.npy|P.pkl --mesh HEAD.obj --out_dir DIR [--iter 30000]
        strand points [S, L, 3] -> DIR/N_strands.pkl, DIR/N_strands.ply

(src/preprocessing/scale_scene_into_sphere.py, filter_flame_intersections.py, export_strands.py.)  The containment runs in HIP on
cuda:0; --composed evaluates the PyTorch-composed form instead (any device, slow)."""
import argparse
import os
import pickle
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussianhaircut_amd import between_stages as bs  # noqa: E402
from gaussianhaircut_amd.mesh import HeadMesh  # noqa: E402
from gaussianhaircut_amd.scene.gaussian_model import GaussianModel  # noqa: E402


def _load(path, sh_degree, device):
    m = GaussianModel(sh_degree)
    m.load_ply(path, device=device)
    return m


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("step", choices=["crop", "filter", "export"])
    ap.add_argument("--model_path")
    ap.add_argument("--path_to_data")
    ap.add_argument("--mesh")
    ap.add_argument("--points")
    ap.add_argument("--out_dir")
    ap.add_argument("--iter", type=int, default=30_000)
    ap.add_argument("--sh_degree", type=int, default=3)
    ap.add_argument("--probe", default="reference", choices=["reference", "ellipsoid", "axis_scaled"])
    ap.add_argument("--composed", action="store_true")
    ap.add_argument("--device", default=None)
    a = ap.parse_args(argv)
    fused = not a.composed
    dev = torch.device(a.device or ("cuda:0" if fused else "cpu"))
    it = "iteration_%d" % a.iter
    if a.step == "crop":
        m = _load(os.path.join(a.model_path, "point_cloud", it, "raw_point_cloud.ply"), a.sh_degree, dev)
        tr, s = bs.hair_sphere(m)
        keep = bs.crop_to_sphere(m, tr, s)
        m.save_ply(os.path.join(a.model_path, "point_cloud_cropped", it, "point_cloud.ply"))
        d = bs.write_scale_pickle(os.path.join(a.path_to_data, "scale.pickle"), tr, s)
        print("crop: kept %d of %d Gaussians; %s" % (int(keep.sum()), keep.numel(), d))
    elif a.step == "filter":
        m = _load(os.path.join(a.model_path, "point_cloud_cropped", it, "raw_point_cloud.ply"), a.sh_degree, dev)
        keep = bs.filter_head_intersections(m, HeadMesh.from_obj(a.mesh), probe=a.probe, fused=fused)
        m.save_ply(os.path.join(a.model_path, "point_cloud_filtered", it, "point_cloud.ply"))
        print("filter: kept %d of %d Gaussians" % (int(keep.sum()), keep.numel()))
    else:
        if a.points.endswith(".npy"):
            p = np.load(a.points)
        else:
            with open(a.points, "rb") as f:
                p = np.asarray(pickle.load(f))
        p = torch.from_numpy(np.ascontiguousarray(p, np.float32)).to(dev)
        kept, keep = bs.prune_strands(p, HeadMesh.from_obj(a.mesh), fused=fused)
        print("Pruning %d strands that intersect the head mesh" % int((~keep).sum()))
        print("export: %s %s" % bs.export_strands(kept, a.out_dir, a.iter))


if __name__ == "__main__":
    main()
