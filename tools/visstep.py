"""Time of the head-mesh visibility pass (gaussianhaircut_amd.visibility), HIP kernels against the PyTorch-composed form, in ONE
process on one GPU:

    python tools/visstep.py > profiles/head_visibility.txt

The mesh is a UV sphere of 9976 faces (116 x 44: the face count of the reference's head mesh, which is not redistributable),
radius 1, seen by 64 ring cameras at radius 4 with synthetic blob masks.  Forms: fused (ghr_vis_view: seven launches and one fill
per view) and composed (brute force over all faces in pixel chunks + max_pool2d + unique).  The composed form is timed over its
first VISSTEP_COMPOSED_VIEWS views (default 4) and reported per view, because a full pass of it takes minutes at the larger
sizes; the fused form runs all 64.  Each figure is the device time between two events around a pass, after a warm-up of every
form; the forms alternate and every round is printed.  The floor beside the figures is derived, not measured."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussianhaircut_amd import visibility as vis  # noqa: E402
from gaussianhaircut_amd.scene.cameras import ring_cameras  # noqa: E402
from tests import mesh_cases as mc  # noqa: E402

HBM_BPS = 6.29e12  # measured float4 copy rate of the part (8.0e12 spec)


def blob_masks(n, H, W, seed=0):
    rng = np.random.default_rng(seed)
    ii, jj = np.mgrid[0:H, 0:W]
    out = []
    for _ in range(n):
        planes = []
        for r0 in (0.33, 0.22):      # a body blob and a smaller hair blob above its middle
            ci, cj, r = H * rng.uniform(0.35, 0.65), W * rng.uniform(0.4, 0.6), r0 * min(H, W) * rng.uniform(0.8, 1.2)
            planes.append(np.where((ii - ci + (r0 < 0.3) * 0.2 * H) ** 2 + (jj - cj) ** 2 <= r * r, 255, 0).astype(np.uint8))
        out.append(tuple(planes))
    return out


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    assert torch.cuda.is_available(), "visstep needs a ROCm GPU (a CPU run measures nothing)"
    dev = torch.device("cuda:0")
    n_views = int(os.environ.get("VISSTEP_VIEWS", 64))
    n_cmp = int(os.environ.get("VISSTEP_COMPOSED_VIEWS", 4))
    sizes = [tuple(int(x) for x in s.split("x")) for s in os.environ.get("VISSTEP_SIZES", "256x256,512x512,1080x1920").split(",")]
    rounds = 3
    v, f = mc.uv_sphere(116, 44)
    print("VISSTEP mesh vertices=%d faces=%d views=%d (composed form over the first %d)" % (len(v), len(f), n_views, n_cmp))
    for H, W in sizes:
        cams = ring_cameras(n_views, W, H, radius=4.0)
        views = [vis.view_matrix_from_camera(c) for c in cams]
        masks = [tuple(torch.from_numpy(p).to(dev) for p in m) for m in blob_masks(n_views, H, W)]
        forms = {"fused": lambda: vis.vertex_visibility((v, f), views, masks, fused=True, device=dev),
                 "composed": lambda: vis.vertex_visibility((v, f), views[:n_cmp], masks[:n_cmp], fused=False, device=dev)}
        a = vis.vertex_visibility((v, f), views[:n_cmp], masks[:n_cmp], fused=True, device=dev)
        b = forms["composed"]()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2])), "the forms disagree"
        cnt, cnt_head, _ = forms["fused"]()
        mask = vis.visible_vertex_mask(cnt, cnt_head, n_views)
        print("VISSTEP %dx%d: forms equal on %d views; seen by >= 1 view: %d vertices, through the head: %d, cut mask: %d of %d"
              % (H, W, n_cmp, int((cnt > 0).sum()), int((cnt_head > 0).sum()), int(mask.sum()), len(v)))
        best = {}
        for rd in range(rounds):
            for name, fn in forms.items():
                per_view = timed(fn) / (n_views if name == "fused" else n_cmp)
                best[name] = min(best.get(name, per_view), per_view)
                print("VISSTEP round %d %dx%d %-8s %.4f ms per view" % (rd, H, W, name, per_view))
        # derived: 4 B written and 2 B read per pixel, 108 B per face (nine screen floats and three q) once
        floor = (6.0 * H * W + 108.0 * len(f)) / HBM_BPS * 1e3
        print("VISSTEP %dx%d floor (derived: traffic at the measured copy rate) %.5f ms per view; fused %.4f, composed %.4f ms per "
              "view; fused / composed = %.4f" % (H, W, floor, best["fused"], best["composed"], best["fused"] / best["composed"]))


if __name__ == "__main__":
    main()
