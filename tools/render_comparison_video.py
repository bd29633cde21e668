"""The frames of the reference's comparison video (run.sh, "VISUALIZATIONS": render_strands.py --interpolate_cameras and
src/postprocessing/concat_video.py) -- photograph | strand render | Gaussian render -- without ffmpeg: PNGs in, PNGs out.

    python tools/render_comparison_video.py path --model_path OUT --ply point_cloud.ply --cameras cameras.json --iteration 30000
    python tools/render_comparison_video.py frames --renders OUT/train/ours_30000/renders --preview blender/results \
        --gt frames --out OUT

``path`` renders the model along the camera path scene.interpolated_cameras makes of the key cameras (evaluation.render_products,
the 8-bit ``render`` product) and writes <model_path>/train/ours_<iteration>/renders/%06d.png, named by frame number as the
reference names them.  --cameras is the ``cameras.json`` a trained model's directory holds (a list of {img_name, width, height,
position, rotation, fx, fy}: the camera-to-world pose and the focal lengths in pixels); entries whose img_name is not a frame
number are skipped.  --width / --height render at another size with the keys' fields of view.  A script that holds a strand model
calls ``render_path`` below with ``gaussians_hair``; this package has no checkpoint reader for it.

``frames`` assembles one frame per PNG of --renders, in the order of their names (gaussianhaircut_amd.comparison):
the strand render of the same name in --preview (Blender's results) or, where the names differ, of the same position in name
order (tools/render_strand_video.py's results), RGB or RGBA, and the photograph '%06d' % (int(NAME) - 1) of --gt (.png or .jpg), as the script pairs them.  Writes
<out>/frames/%06d.png, numbered by position.  --composed takes the PyTorch-composed comparator instead of the HIP kernels (any
device).  No video is encoded."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussianhaircut_amd import comparison as cmp  # noqa: E402
from gaussianhaircut_amd import evaluation as ev  # noqa: E402
from gaussianhaircut_amd.scene.cameras import Camera, interpolated_cameras  # noqa: E402


def load_key_cameras(path, width=None, height=None):
    """cameras.json -> Cameras on the host, one per entry named by a frame number"""
    with open(path) as fh:
        entries = json.load(fh)
    keys = []
    for e in entries:
        name = os.path.splitext(os.path.basename(str(e["img_name"])))[0]
        if not name.isdigit():
            continue
        c2w_R, pos = np.asarray(e["rotation"], np.float64), np.asarray(e["position"], np.float64)
        w, h = int(e["width"]), int(e["height"])
        fovx, fovy = 2 * np.arctan(w / (2 * float(e["fx"]))), 2 * np.arctan(h / (2 * float(e["fy"])))
        keys.append(Camera(c2w_R, -c2w_R.T @ pos, fovx, fovy, width or w, height or h, image_name=name))
    if len(keys) < 2:
        raise SystemExit("%s holds fewer than two cameras named by a frame number" % path)
    return keys


def render_path(gaussians, keys, background, out_dir, gaussians_hair=None, speed_up=4, max_frames=300, frame_offset=0, fused=None):
    """Writes the ``render`` product of every path camera to out_dir/<image_name>.png; returns their number."""
    from PIL import Image
    os.makedirs(out_dir, exist_ok=True)
    cams = interpolated_cameras(keys, speed_up=speed_up, max_frames=max_frames, frame_offset=frame_offset, device=background.device)
    n = 0
    for p in ev.render_products(gaussians, cams, background, gaussians_hair=gaussians_hair, fused=fused, copy=False):
        Image.fromarray(p["render"], "RGB").save(os.path.join(out_dir, "%s.png" % p["name"]))
        n += 1
    return n


def _pngs(d):
    return sorted(f for f in os.listdir(d) if f.lower().endswith(".png"))


def _read(path):
    from PIL import Image
    im = Image.open(path)
    if im.mode not in ("RGB", "RGBA"):
        im = im.convert("RGBA" if "A" in im.mode or "transparency" in im.info else "RGB")
    return np.array(im)


def _photograph(d, name):
    for ext in (".png", ".jpg", ".jpeg", ".PNG", ".JPG"):
        p = os.path.join(d, name + ext)
        if os.path.exists(p):
            return _read(p)[:, :, :3]
    raise SystemExit("no photograph %s.png / .jpg in %s" % (name, d))


def assemble_frames(renders_dir, preview_dir, gt_dir, out_dir, out_short=720, fused=None, device=None):
    """Returns the number of frames written to out_dir/frames."""
    from PIL import Image
    renders, previews = _pngs(renders_dir), _pngs(preview_dir)
    if all(r in previews for r in renders):      # Blender's results carry the renders' names, as the script expects
        previews = renders
    elif len(previews) < len(renders):           # tools/render_strand_video.py numbers its frames by position
        raise SystemExit("%d renders in %s, but %d strand renders in %s" % (len(renders), renders_dir, len(previews), preview_dir))
    out = os.path.join(out_dir, "frames")
    os.makedirs(out, exist_ok=True)
    gts = (_photograph(gt_dir, "%06d" % (int(os.path.splitext(r)[0]) - 1)) for r in renders)
    pvs = (_read(os.path.join(preview_dir, p)) for p in previews)
    rds = (_read(os.path.join(renders_dir, r))[:, :, :3] for r in renders)
    n = 0
    for n, frame in enumerate(cmp.comparison_frames(gts, pvs, rds, out_short=out_short, fused=fused, device=device), 1):
        Image.fromarray(frame, "RGB").save(os.path.join(out, "%06d.png" % (n - 1)))
    return n


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("path")
    p.add_argument("--model_path", required=True)
    p.add_argument("--ply", required=True)
    p.add_argument("--cameras", required=True)
    p.add_argument("--iteration", type=int, default=30000)
    p.add_argument("--width", type=int)
    p.add_argument("--height", type=int)
    p.add_argument("--speed_up", type=int, default=4)
    p.add_argument("--max_frames", type=int, default=300)
    p.add_argument("--frame_offset", type=int, default=0)
    p.add_argument("--white_background", action="store_true")
    p.add_argument("--composed", action="store_true")
    f = sub.add_parser("frames")
    f.add_argument("--renders", required=True)
    f.add_argument("--preview", required=True)
    f.add_argument("--gt", required=True)
    f.add_argument("--out", default=".")
    f.add_argument("--out_short", type=int, default=720)
    f.add_argument("--composed", action="store_true")
    f.add_argument("--device", default=None)
    a = ap.parse_args(argv)
    if a.cmd == "path":
        from gaussianhaircut_amd.scene.gaussian_model import GaussianModel
        dev = torch.device("cuda:0")   # rendering is ROCm-only; --composed composes the products from torch operations
        model = GaussianModel(3)
        model.load_ply(a.ply, device=dev)
        bg = torch.tensor(([1, 1, 1] if a.white_background else [0, 0, 0]) + [0, 0, 0, 0, 0, 0, 100], dtype=torch.float32, device=dev)
        out = os.path.join(a.model_path, "train", "ours_%d" % a.iteration, "renders")
        n = render_path(model, load_key_cameras(a.cameras, a.width, a.height), bg, out, speed_up=a.speed_up, max_frames=a.max_frames,
                        frame_offset=a.frame_offset, fused=not a.composed)
        print("render_comparison_video: %d path renders in %s" % (n, out))
        return n
    dev = torch.device(a.device if a.device else ("cpu" if a.composed else "cuda:0"))
    n = assemble_frames(a.renders, a.preview, a.gt, a.out, a.out_short, fused=not a.composed, device=dev)
    print("render_comparison_video: %d frames in %s%s" % (n, os.path.join(a.out, "frames"), ", composed" if a.composed else ""))
    return n


if __name__ == "__main__":
    main()
