"""Golden of the evaluation pass: the REFERENCE's own ``src/utils/image_utils.py`` (psnr, vis_orient) and
``src/utils/loss_utils.py`` (l1_loss, or_loss, ssim) on the CPU, composed as ``training_report``
(``src/train_gaussians.py:254-277``), ``src/metrics.py:71-78`` and ``render_set`` (``src/render_gaussians.py:52-68``) compose them,
over random packed [10,H,W] renders and ground truths, in float32 and -- the same calls on float64 tensors -- in float64.

Two things are restated here rather than imported: the orientation angle of ``src/gaussian_renderer/__init__.py:102-105`` (that
module cannot be imported without the rasterizer extension) and the one-line quantisation of torchvision's ``save_image``,
``mul(255).add_(0.5).clamp_(0, 255).to(uint8)`` (torchvision is not installed where this runs).

Cases: (H, W) = (5, 7), (23, 37), (48, 64); then, at (23, 37), one whose orientation weights are all zero and one whose render
equals its ground truth.  Colours are spread beyond [0, 1], masks lie in [-0.1, 1.1], confidences are positive.  Writes
``reference_eval_golden.npz`` (data only): inputs, the five metrics in both precisions, and the float64 product values before
quantisation (from which a test derives the expected levels and which elements sit on a rounding edge).

    python -m tests.golden.make_reference_eval_golden      # needs the reference checkout
"""
import importlib.util
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

REF = "/root/reference/src"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_eval_golden.npz")
SHAPES = ((5, 7), (23, 37), (48, 64))
METRICS = ("l1", "ce", "or", "psnr", "ssim")
PRODUCTS = ("render", "hair_mask", "head_mask", "orient", "orient_vis", "orient_conf_vis", "orient_conf")


def _load(name):
    spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(REF, "utils", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_inputs(H, W, seed):
    g = np.random.default_rng(seed)
    packed = np.empty((10, H, W), np.float32)
    packed[0:3] = g.uniform(-0.3, 1.3, (3, H, W))
    packed[3:5] = g.uniform(-0.1, 1.1, (2, H, W))
    packed[5:8] = g.standard_normal((3, H, W))
    packed[8] = np.minimum(np.exp(0.5 * g.standard_normal((H, W))), 4.0)
    packed[9] = g.uniform(1.0, 6.0, (H, W))
    gt = dict(gt_image=g.uniform(-0.3, 1.3, (3, H, W)).astype(np.float32),
              gt_mask=g.uniform(-0.1, 1.1, (2, H, W)).astype(np.float32),
              gt_angle=g.uniform(-0.05, 1.05, (1, H, W)).astype(np.float32),
              gt_conf=np.exp(0.5 * g.standard_normal((1, H, W))).astype(np.float32))
    return dict(packed=packed, **gt)


def orient_angle(cov2d):
    dir2d = F.normalize(cov2d[:2], dim=0)
    mirror = torch.where(dir2d[[0]] < 0, -torch.ones_like(dir2d[[0]]), torch.ones_like(dir2d[[0]]))
    return torch.acos(dir2d[[1]].clamp(-1 + 1e-3, 1 - 1e-3) * mirror) / math.pi


def reference_metrics(iu, lu, c, dtype):
    t = {k: torch.from_numpy(v).to(dtype) for k, v in c.items()}
    image, mask = torch.clamp(t["packed"][0:3], 0.0, 1.0), torch.clamp(t["packed"][3:5], 0.0, 1.0)
    angle = torch.clamp(orient_angle(t["packed"][5:8]), 0.0, 1.0)
    gt_image, gt_mask = torch.clamp(t["gt_image"], 0.0, 1.0), torch.clamp(t["gt_mask"], 0.0, 1.0)
    gt_angle = torch.clamp(t["gt_angle"], 0.0, 1.0)
    with np.errstate(all="ignore"):
        return np.array([lu.l1_loss(image, gt_image).mean().double().item(),
                         lu.l1_loss(mask, gt_mask).mean().double().item(),
                         lu.or_loss(angle, gt_angle, mask=gt_mask[:1], weight=t["gt_conf"]).mean().double().item(),
                         iu.psnr(image, gt_image).mean().double().item(),
                         lu.ssim(image, gt_image).double().item()], np.float64)


def reference_products(iu, packed, dtype):
    p = torch.from_numpy(packed).to(dtype)
    image, hair_mask, head_mask = p[0:3], p[3:4], p[4:5]
    angle = orient_angle(p[5:8])
    orient_conf = p[8:9] * hair_mask
    vals = dict(render=image, hair_mask=hair_mask, head_mask=head_mask, orient=angle * hair_mask,
                orient_vis=iu.vis_orient(angle, hair_mask), orient_conf_vis=iu.vis_orient(angle, 1 - 1 / (orient_conf + 1)),
                orient_conf=orient_conf)
    return {k: v.numpy() for k, v in vals.items()}


def save_image_levels(v):
    """torchvision.utils.save_image's quantisation, restated (see the module docstring); CHW in, CHW out"""
    return torch.from_numpy(np.asarray(v)).mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).numpy()


def main():
    iu, lu = _load("image_utils"), _load("loss_utils")
    cases = [make_inputs(H, W, 100 + i) for i, (H, W) in enumerate(SHAPES)]
    zero_w = dict(cases[1])
    zero_w["gt_conf"] = np.zeros_like(zero_w["gt_conf"])
    same = dict(cases[1])
    same["gt_image"], same["gt_mask"] = same["packed"][0:3].copy(), same["packed"][3:5].copy()
    cases += [zero_w, same]
    out = {"n_cases": np.int64(len(cases)), "n_product_cases": np.int64(len(SHAPES))}
    worst = 0
    for i, c in enumerate(cases):
        for k, v in c.items():
            if i < len(SHAPES) or k != "packed":    # the two special cases share case 1's render
                out["c%d/%s" % (i, k)] = v
        out["c%d/ref32" % i] = reference_metrics(iu, lu, c, torch.float32)
        out["c%d/ref64" % i] = reference_metrics(iu, lu, c, torch.float64)
        print(i, c["packed"].shape[1:], dict(zip(METRICS, out["c%d/ref64" % i])), np.abs(out["c%d/ref32" % i] - out["c%d/ref64" % i]))
        if i < len(SHAPES):
            p32, p64 = reference_products(iu, c["packed"], torch.float32), reference_products(iu, c["packed"], torch.float64)
            for k in PRODUCTS:
                out["c%d/prod64/%s" % (i, k)] = p64[k]
                if k != "orient_conf":
                    d = save_image_levels(p32[k]) != save_image_levels(p64[k])
                    frag = np.abs(p64[k] * 255 + 0.5 - np.round(p64[k] * 255 + 0.5)) < 0.01
                    print("   %-16s fp32 / fp64 levels differ at %d elements (%d of them off a rounding edge), %.2f %% on an edge"
                          % (k, d.sum(), (d & ~frag).sum(), 100 * frag.mean()))
                    worst = max(worst, (d & ~frag).sum())
    assert worst == 0
    np.savez(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
