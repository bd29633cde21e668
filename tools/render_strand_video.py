"""The last step of the reference's run.sh (src/postprocessing/render_video.py) without Blender: the frames of a camera path
around the exported strands and the head mesh, drawn by gaussianhaircut_amd.strand_view (csrc/ghr_strandview.h).

    python tools/render_strand_video.py --strands 10000_strands.pkl --mesh mesh_final.obj --cameras 30000_matrices.pkl \
        --size 1080x1920 --out blender

writes OUT/results/%06d.png (Pillow; no video is encoded).  --strands is what between_stages.export_strands writes: the pickled
[S, L, 3] array, or the PLY of its points with --strand_length L.  --cameras is the reference's *_matrices.pkl: name -> 4 x 4,
used as transpose(0, 1)[:3, :4] as the script does; names that are frame numbers are the key frames.  The key cameras are brought
to the pixels of --size as visibility.views_from_projections does, then strand_view.camera_path interpolates them.
--composed takes the PyTorch-composed comparator instead of the HIP kernels (any device; slow).
--shadows adds self-shadowing (a deep opacity map of the light's view): by default the light follows the camera and
the map is made per frame; with --world-light X Y Z the light is that world vector (towards the light) for the whole path and ONE
map is made and reused."""
import argparse
import os
import pickle
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussianhaircut_amd import strand_view as sv  # noqa: E402
from gaussianhaircut_amd import visibility as vis  # noqa: E402
from gaussianhaircut_amd.mesh import read_obj  # noqa: E402
from gaussianhaircut_amd.scene import ply_io  # noqa: E402


def load_strands(path, strand_length):
    if path.endswith(".pkl"):
        with open(path, "rb") as fh:
            p = pickle.load(fh)
        p = p.detach().cpu().numpy() if isinstance(p, torch.Tensor) else np.asarray(p)
        return np.ascontiguousarray(p, np.float32).reshape(p.shape[0], -1, 3)
    _, v = ply_io.read_ply_vertices(path)
    xyz = np.stack([np.asarray(v[c], np.float32) for c in ("x", "y", "z")], 1)
    if strand_length < 2 or len(xyz) % strand_length:
        raise SystemExit("--strand_length %d does not divide the %d points of %s" % (strand_length, len(xyz), path))
    return np.ascontiguousarray(xyz.reshape(-1, strand_length, 3))


def load_key_cameras(path, H, W):
    """frame number -> 3 x 4 float64 pixel matrix"""
    with open(path, "rb") as fh:
        cams = pickle.load(fh)
    keys = {}
    for name, P in cams.items():
        if not str(name).isdigit():
            continue
        P = P.detach().cpu().numpy() if isinstance(P, torch.Tensor) else np.asarray(P)
        M, _, _ = vis.views_from_projections({"k": np.asarray(P, np.float64).T[:3, :4]}, {"k": (H, W)})["k"]
        keys[int(name)] = M.astype(np.float64).reshape(3, 4)
    if len(keys) < 2:
        raise SystemExit("%s holds fewer than two cameras named by a frame number" % path)
    return keys


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--strands", required=True)
    ap.add_argument("--strand_length", type=int, default=100)
    ap.add_argument("--mesh", default=None)
    ap.add_argument("--cameras", required=True)
    ap.add_argument("--size", default="1080x1920", help="HxW")
    ap.add_argument("--out", default=".")
    ap.add_argument("--speed_up", type=int, default=4)
    ap.add_argument("--max_frames", type=int, default=200)
    ap.add_argument("--supersample", type=int, default=2, choices=(1, 2, 4))
    ap.add_argument("--mode", default="kajiya", choices=sorted(sv.MODES))
    ap.add_argument("--half_width", type=float, default=0.75)
    ap.add_argument("--head_bias", type=float, default=0.0)
    ap.add_argument("--composed", action="store_true")
    ap.add_argument("--shadows", action="store_true")
    ap.add_argument("--world-light", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"))
    ap.add_argument("--shadow_size", type=int, default=sv.SHADOW_SIZE)
    ap.add_argument("--device", default=None)
    a = ap.parse_args(argv)
    from PIL import Image
    H, W = (int(x) for x in a.size.lower().split("x"))
    points = load_strands(a.strands, a.strand_length)
    mesh = read_obj(a.mesh) if a.mesh else None
    path = sv.camera_path(load_key_cameras(a.cameras, H, W), speed_up=a.speed_up, max_frames=a.max_frames)
    dev = torch.device(a.device if a.device else ("cpu" if a.composed else "cuda:0"))
    pts = torch.from_numpy(points).to(dev)
    out = os.path.join(a.out, "results")
    os.makedirs(out, exist_ok=True)
    if a.world_light is not None and not a.shadows:
        raise SystemExit("--world-light needs --shadows")
    kw, shadows = {}, a.shadows
    if a.world_light is not None:
        kw["light"] = np.asarray(a.world_light, np.float64) / np.linalg.norm(a.world_light)
        Ml, Hl, Wl, _ = sv.light_view(pts, mesh, light=kw["light"], size=a.shadow_size)
        shadows = sv.strand_shadow_map(pts, Ml, Hl, Wl, mesh=mesh, fused=not a.composed, device=dev)
    for n, P in enumerate(path):
        pic = sv.render_strands(pts, (P.astype(np.float32).reshape(12), H, W), mesh=mesh, mode=a.mode, supersample=a.supersample,
                                half_width=a.half_width, head_bias=a.head_bias, fused=not a.composed, device=dev, shadows=shadows,
                                shadow_size=a.shadow_size, **kw)
        Image.fromarray(pic.cpu().numpy()).save(os.path.join(out, "%06d.png" % n))
    print("render_strand_video: %d frames of %d x %d (%d strands of %d points%s%s) in %s"
          % (len(path), H, W, points.shape[0], points.shape[1], ", composed" if a.composed else "", ", shadows" if a.shadows else "", out))
    return len(path)


if __name__ == "__main__":
    main()
