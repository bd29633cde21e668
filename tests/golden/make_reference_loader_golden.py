"""Golden of the ground-truth loader: the REFERENCE's own ``loadCam`` (src/utils/camera_utils.py:29-84, with ``PILtoTorch`` of
src/utils/general_utils.py and ``Camera`` of src/scene/cameras.py behind it) and its ``src/preprocessing/resize_images.py`` --
imported at run time from the read-only checkout and called unmodified on the CPU -- over small synthetic views written as
files in the layout the reference reads.

    python -m tests.golden.make_reference_loader_golden      # needs the reference checkout and Pillow

As in make_reference_camera_bank_golden.py: ``.cuda()`` and ``device="cuda"`` are redirected to the CPU, ``easydict`` is an empty
stand-in, ``scene.cameras`` is loaded by file path under a stand-in ``scene`` package (the package's ``__init__`` pulls
plyfile); ``cv2`` is an empty stand-in too (resize_images.py imports it and does not use it).

Views (w x h), written to a temporary directory as ``images_2/<name>.png``, ``masks_2/{hair,body}/<name>.png``,
``orientations_2/angles/<name>.png`` and ``orientations_2/vars/<name>.npy`` (float16):
  a  37 x 53   odd sizes; ``-r 2`` and ``-r 4`` round to (18, 26) and (9, 13) by Python's rounding, ``-r 8`` to (5, 7)
  b  64 x 64   ``-r 8`` to (8, 8), an exact ``/ 2``, ``-r 4``
  c  1700 x 2  ``-r -1``: the 1.6K rule
  d  16 x 20   a width of 33: an upscale to (33, 41), five taps
The image is textured noise with every third row drawn from {0, 255} (the bicubic lobes saturate); the masks are soft discs with
noise, with bytes 127 and 128 planted (the two sides of ``binarize_masks``); the angle is random in 0 ... 179 with a few bytes
above 180 (the clamp); the variance is positive float16 with zeros (conf = 1e7).

CASES: (view, resolution, binarize_masks, white_background).  Per case ``k``: ``k/size`` = (w, h) of the result and the
reference camera's ``image``, ``mask``, ``angle``, ``conf`` (``original_mask_hair`` / ``_body`` are asserted here to be the
two planes of ``mask``); and of the variance alone ``k/var32`` (F.interpolate in float32, as loadCam calls it) and ``k/var_dist``
= ``|var32 - var64|``, var64 the same blend in double from the float32 source coordinates (``bilinear64`` below, also what the
tests call) -- the distance the tests' bar for a resized variance is built from.  Where the size changes, PILtoTorch's resized
bytes are stored as ``k/image_u8`` etc. (what ``resize_u8`` must reproduce).  SIZE_CASES: (view, resolution, resolution_scale)
with the size loadCam arrived at, ``sizes`` = rows of (orig_w, orig_h, resolution, w, h) and ``size_scales``.

resize_images.py runs on views a and b (``images/``, ``masks/{hair,body,face}``; b's face mask covers its hair, so the script
skips it) plus the two ``Image.resize(..., Image.BICUBIC)`` calls on b directly: ``pyr/<view>/<factor>/{image,hair,body}``,
``pyr/skipped``.  Numeric arrays only; nothing of the reference is copied.  ``pillow``: the version the bytes were recorded with."""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

REF = "/root/reference/src"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "reference_loader_golden.npz")
VIEWS = {"a": (37, 53, 1), "b": (64, 64, 2), "c": (1700, 2, 3), "d": (16, 20, 4)}   # w, h, seed
CASES = (("a", 1, 0, 0), ("a", 1, 1, 1),
         ("a", 2, 0, 0), ("a", 2, 1, 0), ("a", 2, 0, 1), ("a", 2, 1, 1),
         ("a", 4, 0, 0), ("a", 8, 0, 0), ("a", 20, 0, 0), ("a", 4, 1, 1),
         ("b", 8, 0, 0), ("b", 2, 1, 1), ("b", 4, 0, 1),
         ("c", -1, 0, 0), ("d", 33, 0, 0))
# sizes alone: (view, resolution, resolution_scale)
SIZE_CASES = (("a", -1, 1.0), ("b", -1, 1.0), ("b", 1, 1.0), ("a", 30, 1.0), ("a", 2, 2.0), ("b", 4, 0.5), ("c", 2, 1.0), ("c", -1, 0.5),
              ("d", 2, 1.0), ("a", 1, 3.0), ("c", 1600, 1.0), ("b", 63, 1.0))


def make_view(w, h, seed):
    g = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    image = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
    image[::3] = g.choice(np.array([0, 255], np.uint8), image[::3].shape)

    def disc(cx, cy, r):
        d = np.hypot(x - cx * w, y - cy * h) / (r * max(min(w, h), 8))
        m = np.clip((1.2 - d) * 255, 0, 255) + 20 * g.standard_normal((h, w))
        return np.clip(m, 0, 255).astype(np.uint8)
    hair, body, face = disc(0.5, 0.35, 0.45), disc(0.5, 0.5, 0.8), disc(0.5, 0.6, 0.1)
    hair.reshape(-1)[:: 7][:8] = 127
    hair.reshape(-1)[3:: 7][:8] = 128
    body.reshape(-1)[1:: 5][:8] = 128
    body.reshape(-1)[2:: 5][:8] = 127
    angle = g.integers(0, 180, (h, w)).astype(np.uint8)
    angle.reshape(-1)[:: 11][:6] = 200
    var = (g.random((h, w)) ** 2 * 2.5).astype(np.float16)
    var.reshape(-1)[:: 13] = 0
    return dict(image=image, hair=hair, body=body, face=face, angle=angle, var=var)


def lerp_coords32(in_size, out_size):
    """F.interpolate(align_corners=False)'s source cell along one axis with float32 arithmetic: (i0, i1, lambda float32)"""
    scale = np.float32(in_size) / np.float32(out_size)
    src = scale * (np.arange(out_size, dtype=np.float32) + np.float32(0.5)) - np.float32(0.5)
    src = np.maximum(src, np.float32(0))
    i0 = np.minimum(src.astype(np.int64), in_size - 1)
    i1 = i0 + (i0 < in_size - 1)
    lam = np.clip(src - i0.astype(np.float32), np.float32(0), np.float32(1))
    assert src.dtype == lam.dtype == np.float32
    return i0, i1, lam


def bilinear64(var, w, h):
    """hy (hx a + lx b) + ly (hx c + lx d) in double, the weights the float32 ones of ``lerp_coords32`` (hx = 1 - lx in float32)"""
    v = np.asarray(var).astype(np.float64)
    x0, x1, lx = lerp_coords32(v.shape[1], w)
    y0, y1, ly = lerp_coords32(v.shape[0], h)
    hx, hy = (np.float32(1) - lx).astype(np.float64)[None, :], (np.float32(1) - ly).astype(np.float64)[:, None]
    lx, ly = lx.astype(np.float64)[None, :], ly.astype(np.float64)[:, None]
    return hy * (hx * v[y0][:, x0] + lx * v[y0][:, x1]) + ly * (hx * v[y1][:, x0] + lx * v[y1][:, x1])


def _patch_cuda_factories():
    def wrap(fn):
        def inner(*a, **k):
            if str(k.get("device", "")).startswith("cuda"):
                k["device"] = "cpu"
            return fn(*a, **k)
        return inner
    for name in ("zeros", "ones", "arange", "tensor", "empty", "full", "eye"):
        setattr(torch, name, wrap(getattr(torch, name)))
    torch.Tensor.cuda = lambda self, *a, **k: self


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    import PIL
    from PIL import Image
    assert os.path.isdir(REF), "needs the reference checkout"
    _patch_cuda_factories()
    for name, attrs in (("easydict", dict(EasyDict=dict)), ("cv2", {})):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
    sys.path.insert(0, REF)
    for m in [k for k in sys.modules if k in ("utils", "scene") or k.startswith(("utils.", "scene."))]:
        del sys.modules[m]
    sys.modules["scene"] = types.ModuleType("scene")
    sys.modules["scene"].__path__ = []
    _load("scene.cameras", os.path.join(REF, "scene", "cameras.py"))
    cu = _load("ref_camera_utils", os.path.join(REF, "utils", "camera_utils.py"))
    ri = _load("ref_resize_images", os.path.join(REF, "preprocessing", "resize_images.py"))

    out = {"pillow": np.array(PIL.__version__), "n_cases": np.array(len(CASES)),
           "cases": np.array([[ord(v), r, b, wb] for v, r, b, wb in CASES], np.int64)}
    views = {k: make_view(*v) for k, v in VIEWS.items()}
    for k, v in views.items():
        for n, a in v.items():
            out["view/%s/%s" % (k, n)] = a
    worst = 0.0
    with tempfile.TemporaryDirectory() as tmp:
        for sub in ("images_2", "masks_2/hair", "masks_2/body", "orientations_2/angles", "orientations_2/vars"):
            os.makedirs(os.path.join(tmp, sub))
        for k, v in views.items():
            Image.fromarray(v["image"]).save(os.path.join(tmp, "images_2", k + ".png"))
            Image.fromarray(v["hair"]).save(os.path.join(tmp, "masks_2/hair", k + ".png"))
            Image.fromarray(v["body"]).save(os.path.join(tmp, "masks_2/body", k + ".png"))
            Image.fromarray(v["angle"]).save(os.path.join(tmp, "orientations_2/angles", k + ".png"))
            np.save(os.path.join(tmp, "orientations_2/vars", k + ".npy"), v["var"])
        for i, (k, r, binarize, white) in enumerate(CASES):
            path = os.path.join(tmp, "images_2", k + ".png")
            pil = Image.open(path)
            info = types.SimpleNamespace(image=pil, image_path=path, uid=i, R=np.eye(3), T=np.zeros(3), FovX=0.7, FovY=0.7,
                                         width=pil.size[0], height=pil.size[1], image_name=k)
            args = types.SimpleNamespace(resolution=r, binarize_masks=bool(binarize), white_background=bool(white), data_device="cpu",
                                         trainable_cameras=False, use_barf=False, trainable_intrinsics=False)
            cam = cu.loadCam(args, i, info, 1.0)
            w, h = cam.image_width, cam.image_height
            tag = "%d/" % i
            out[tag + "size"] = np.array([w, h], np.int64)
            for n, t in (("image", cam.original_image), ("mask", cam.original_mask), ("angle", cam.original_orient_angle),
                         ("conf", cam.original_orient_conf)):
                assert t.dtype == torch.float32
                out[tag + n] = t.numpy().copy()
            assert torch.equal(cam.original_mask[0:1], cam.original_mask_hair) and torch.equal(cam.original_mask[1:2], cam.original_mask_body)
            v = views[k]
            if (w, h) != pil.size:
                for n in ("image", "hair", "body", "angle"):   # PILtoTorch's resize, alone
                    out[tag + n + "_u8"] = np.array(Image.fromarray(v[n]).resize((w, h)))
            var32 = torch.nn.functional.interpolate(torch.from_numpy(v["var"]).float()[None, None], size=(h, w), mode="bilinear")[0, 0].numpy()
            var64 = bilinear64(v["var"], w, h)
            out[tag + "var32"], out[tag + "var_dist"] = var32, np.abs(var32 - var64).astype(np.float32)
            worst = max(worst, float(np.abs(var32 - var64).max() / max(float(v["var"].max()), 1e-30)))
            conf = (1 / ((torch.from_numpy(var32) / np.pi ** 2) ** 2 + 1e-7)).numpy()
            assert np.array_equal(conf, out[tag + "conf"][0]), "the stored var32 is not what loadCam's conf came from"
        rows = []
        for k, r, rs in SIZE_CASES:
            path = os.path.join(tmp, "images_2", k + ".png")
            pil = Image.open(path)
            info = types.SimpleNamespace(image=pil, image_path=path, uid=0, R=np.eye(3), T=np.zeros(3), FovX=0.7, FovY=0.7,
                                         width=pil.size[0], height=pil.size[1], image_name=k)
            args = types.SimpleNamespace(resolution=r, binarize_masks=False, white_background=False, data_device="cpu",
                                         trainable_cameras=False, use_barf=False, trainable_intrinsics=False)
            cam = cu.loadCam(args, 0, info, rs)
            rows.append([pil.size[0], pil.size[1], r, cam.image_width, cam.image_height])
        out["sizes"], out["size_scales"] = np.array(rows, np.int64), np.array([rs for _, _, rs in SIZE_CASES])

        # resize_images.py on views a and b
        data = os.path.join(tmp, "data")
        for sub in ("images", "masks/hair", "masks/body", "masks/face"):
            os.makedirs(os.path.join(data, sub))
        face_b = views["b"]["hair"].copy()   # b: the face covers the hair -> skipped
        out["view/b/face_skip"] = face_b
        for k, face in (("a", views["a"]["face"]), ("b", face_b)):
            Image.fromarray(views[k]["image"]).save(os.path.join(data, "images", k + ".png"))
            Image.fromarray(views[k]["hair"]).save(os.path.join(data, "masks/hair", k + ".png"))
            Image.fromarray(views[k]["body"]).save(os.path.join(data, "masks/body", k + ".png"))
            Image.fromarray(face).save(os.path.join(data, "masks/face", k + ".png"))
        ri.main(types.SimpleNamespace(data_path=data))
        skipped = []
        for k in ("a", "b"):
            if not os.path.exists(os.path.join(data, "images_2", k + ".png")):
                skipped.append(k)
                continue
            for f in (2, 4):
                out["pyr/%s/%d/image" % (k, f)] = np.array(Image.open(os.path.join(data, "images_%d" % f, k + ".png")))
                out["pyr/%s/%d/hair" % (k, f)] = np.array(Image.open(os.path.join(data, "masks_%d/hair" % f, k + ".png")))
                out["pyr/%s/%d/body" % (k, f)] = np.array(Image.open(os.path.join(data, "masks_%d/body" % f, k + ".png")))
        assert skipped == ["b"], skipped
        out["pyr/skipped"] = np.array([ord(s) for s in skipped], np.int64)
        w, h = VIEWS["b"][:2]
        for f in (2, 4):   # the script's two calls on b directly
            for n in ("image", "hair", "body"):
                out["pyr/b/%d/%s" % (f, n)] = np.array(Image.fromarray(views["b"][n]).resize((w // f, h // f), Image.BICUBIC))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(out), "arrays; Pillow", PIL.__version__)
    print("F.interpolate's float32 against the double blend: worst %.3g of max|v|" % worst)


if __name__ == "__main__":
    main()
