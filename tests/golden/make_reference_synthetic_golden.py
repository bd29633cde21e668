"""Golden of the synthetic ground truth: the REFERENCE's own ``loadCam`` (src/utils/camera_utils.py:29-84) and ``Camera``
(src/scene/cameras.py) with ``load_synthetic_rgba`` / ``load_synthetic_geom`` -- imported at run time from the read-only checkout
and called unmodified on the CPU, with the stand-ins of make_reference_loader_golden.py -- over small views written as files in
the layout the reference reads.

    python -m tests.golden.make_reference_synthetic_golden      # needs the reference checkout and Pillow

Per view (w x h; a 37 x 53, b 64 x 64, d 16 x 20, the loader golden's own ``make_view`` for the photograph's side) a temporary
directory holds ``images_2/<name>.png``, ``masks_2/{hair,body}``, ``orientations_2/{angles,vars}`` and, as render_gaussians.py
writes them, ``<model>/train_cropped/ours_30000/{renders,head_masks,hair_masks,orients}/<name>.png`` and
``orient_confs/<name>.pth``.  The single-channel products are written with Pillow as RGB with three equal channels (what
torchvision's save_image writes for one channel), the confidence with ``torch.save`` of a float [1,H,W] tensor.

The rendered side (``make_synth``): the render is noise with every third row from {0, 255}; the masks are soft discs with bytes
127 and 128 planted (the two sides of ``binarize_masks``); the ``orients`` bytes are random over 0 ... 255 with 0, 180, 200 and
255 planted (``/ 255`` against ``/ 180`` and against a clamp); the confidence is positive with zeros and a few values of 1e6.

CASES: (view, resolution, binarize_masks, white_background, load_synthetic_rgba, load_synthetic_geom) -- ``-r 1 | 2 | 4`` and a
width of 33 on the 16 x 20 view (an upscale), both mask modes, both backgrounds, the three flag combinations.  Per case ``k``:
``k/size`` = (w, h) and the reference camera's ``image``, ``mask``, ``angle``, ``conf``.  Where the confidence (geom) or the
variance (files) is resized, ``k/plane_dist`` = ``|torch32 - f64|`` of that plane: F.interpolate in float32 against
``bilinear64`` of the loader golden's generator -- the distance the tests' bar for a resized plane is built from.  Numeric arrays
only; nothing of the reference is copied.  ``pillow``: the version the bytes were read with."""
import os
import sys
import tempfile
import types

import numpy as np
import torch

from tests.golden import make_reference_loader_golden as mk

REF = mk.REF
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "reference_synthetic_golden.npz")
ITERATION = 30000
VIEWS = {k: mk.VIEWS[k] for k in ("a", "b", "d")}
BOTH, RGBA, GEOM = (1, 1), (1, 0), (0, 1)
CASES = (("a", 1, 0, 0) + BOTH, ("a", 1, 1, 1) + BOTH, ("a", 1, 0, 1) + BOTH, ("a", 1, 1, 0) + BOTH,
         ("a", 2, 0, 0) + BOTH, ("a", 2, 1, 1) + BOTH, ("a", 4, 0, 0) + BOTH,
         ("b", 1, 0, 0) + BOTH, ("b", 2, 1, 0) + BOTH, ("b", 4, 0, 1) + BOTH,
         ("d", 33, 0, 0) + BOTH, ("d", 33, 1, 1) + BOTH,
         ("a", 1, 0, 0) + RGBA, ("a", 2, 1, 1) + RGBA, ("d", 33, 0, 1) + RGBA,
         ("a", 1, 0, 0) + GEOM, ("a", 2, 0, 1) + GEOM, ("b", 4, 1, 0) + GEOM, ("d", 33, 0, 0) + GEOM)
SYNTH_NAMES = ("render", "head", "hair", "orient", "conf")
DIRS = dict(render="renders", head="head_masks", hair="hair_masks", orient="orients")


def make_synth(w, h, seed):
    g = np.random.default_rng(1000 + seed)
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    render = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
    render[1::3] = g.choice(np.array([0, 255], np.uint8), render[1::3].shape)

    def disc(cx, cy, r):
        d = np.hypot(x - cx * w, y - cy * h) / (r * max(min(w, h), 8))
        m = np.clip((1.2 - d) * 255, 0, 255) + 20 * g.standard_normal((h, w))
        return np.clip(m, 0, 255).astype(np.uint8)
    hair, head = disc(0.45, 0.4, 0.4), disc(0.5, 0.5, 0.75)
    hair.reshape(-1)[2:: 7][:8] = 127
    hair.reshape(-1)[5:: 7][:8] = 128
    head.reshape(-1)[1:: 5][:8] = 128
    head.reshape(-1)[3:: 5][:8] = 127
    orient = g.integers(0, 256, (h, w)).astype(np.uint8)
    for i, b in enumerate((0, 180, 200, 255)):
        orient.reshape(-1)[i:: 11][:6] = b
    conf = (g.random((h, w)) ** 2 * 40).astype(np.float32)
    conf.reshape(-1)[:: 13] = 0
    conf.reshape(-1)[4:: 97][:5] = 1e6
    return dict(render=render, head=head, hair=hair, orient=orient, conf=conf)


def rgb3(a):
    return np.repeat(a[:, :, None], 3, axis=2)


def main():
    import PIL
    from PIL import Image
    assert os.path.isdir(REF), "needs the reference checkout"
    mk._patch_cuda_factories()
    for name, attrs in (("easydict", dict(EasyDict=dict)), ("cv2", {})):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
    sys.path.insert(0, REF)
    for m in [k for k in sys.modules if k in ("utils", "scene") or k.startswith(("utils.", "scene."))]:
        del sys.modules[m]
    sys.modules["scene"] = types.ModuleType("scene")
    sys.modules["scene"].__path__ = []
    mk._load("scene.cameras", os.path.join(REF, "scene", "cameras.py"))
    cu = mk._load("ref_camera_utils", os.path.join(REF, "utils", "camera_utils.py"))

    out = {"pillow": np.array(PIL.__version__), "n_cases": np.array(len(CASES)),
           "cases": np.array([[ord(c[0])] + list(c[1:]) for c in CASES], np.int64)}
    photo = {k: mk.make_view(*v) for k, v in VIEWS.items()}
    synth = {k: make_synth(*v) for k, v in VIEWS.items()}
    for k in VIEWS:
        for n in ("image", "hair", "body", "angle", "var"):
            out["view/%s/%s" % (k, n)] = photo[k][n]
        for n in SYNTH_NAMES:
            out["synth/%s/%s" % (k, n)] = synth[k][n]
    with tempfile.TemporaryDirectory() as tmp:
        model = os.path.join(tmp, "model")
        base = os.path.join(model, "train_cropped", "ours_%d" % ITERATION)
        for sub in ("images_2", "masks_2/hair", "masks_2/body", "orientations_2/angles", "orientations_2/vars"):
            os.makedirs(os.path.join(tmp, sub))
        for sub in list(DIRS.values()) + ["orient_confs"]:
            os.makedirs(os.path.join(base, sub))
        for k in VIEWS:
            v, s = photo[k], synth[k]
            Image.fromarray(v["image"]).save(os.path.join(tmp, "images_2", k + ".png"))
            Image.fromarray(v["hair"]).save(os.path.join(tmp, "masks_2/hair", k + ".png"))
            Image.fromarray(v["body"]).save(os.path.join(tmp, "masks_2/body", k + ".png"))
            Image.fromarray(v["angle"]).save(os.path.join(tmp, "orientations_2/angles", k + ".png"))
            np.save(os.path.join(tmp, "orientations_2/vars", k + ".npy"), v["var"])
            Image.fromarray(s["render"], "RGB").save(os.path.join(base, "renders", k + ".png"))
            for n in ("head", "hair", "orient"):
                Image.fromarray(rgb3(s[n]), "RGB").save(os.path.join(base, DIRS[n], k + ".png"))
            torch.save(torch.from_numpy(s["conf"])[None], os.path.join(base, "orient_confs", k + ".pth"))
        for i, (k, r, binarize, white, rgba, geom) in enumerate(CASES):
            path = os.path.join(tmp, "images_2", k + ".png")
            pil = Image.open(path)
            info = types.SimpleNamespace(image=pil, image_path=path, uid=i, R=np.eye(3), T=np.zeros(3), FovX=0.7, FovY=0.7,
                                         width=pil.size[0], height=pil.size[1], image_name=k)
            args = types.SimpleNamespace(resolution=r, binarize_masks=bool(binarize), white_background=bool(white), data_device="cpu",
                                         trainable_cameras=False, use_barf=False, trainable_intrinsics=False, model_path=model,
                                         iteration_data=ITERATION, load_synthetic_rgba=bool(rgba), load_synthetic_geom=bool(geom))
            cam = cu.loadCam(args, i, info, 1.0)
            w, h = cam.image_width, cam.image_height
            tag = "%d/" % i
            out[tag + "size"] = np.array([w, h], np.int64)
            for n, t in (("image", cam.original_image), ("mask", cam.original_mask), ("angle", cam.original_orient_angle),
                         ("conf", cam.original_orient_conf)):
                assert t.dtype == torch.float32
                out[tag + n] = t.numpy().copy()
            assert torch.equal(cam.original_mask[0:1], cam.original_mask_hair) and torch.equal(cam.original_mask[1:2], cam.original_mask_body)
            src = synth[k]["conf"] if geom else photo[k]["var"]
            if (w, h) != pil.size:
                p32 = torch.nn.functional.interpolate(torch.from_numpy(src).float()[None, None], size=(h, w), mode="bilinear")[0, 0].numpy()
                out[tag + "plane_dist"] = np.abs(p32 - mk.bilinear64(src, w, h)).astype(np.float32)
                if geom:
                    assert np.array_equal(p32, out[tag + "conf"][0]), "the resized plane is not what loadCam's conf is"
            elif geom:
                assert np.array_equal(src, out[tag + "conf"][0]), "F.interpolate at equal size changed a finite plane"
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(out), "arrays; Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
