"""Golden of the orientation maps: the REFERENCE's own ``src/preprocessing/calc_orientation_maps.py`` -- imported at run time,
its ``generate_gabor_filters`` and ``calc_orients`` called unmodified on the CPU (``.cuda()`` patched to the identity) -- over
textured synthetic images, plus a float64 restatement of the per-pixel arithmetic that says which pixels the reference's own
float32 run decides.

Two functions are restated here rather than imported, because scikit-image is not installed where this runs:
``skimage.filters.gabor_kernel`` and ``skimage.filters.difference_of_gaussians`` (the latter over
``scipy.ndimage.gaussian_filter``, which is installed), both from scikit-image's definitions.  ``cv2`` and
``torchvision.transforms`` are empty stand-ins: the two functions called here do not use them.

Images: ``img = clip(stack(base * (0.9, 0.7, 0.5)) + 0.05 N(0, 1), 0, 1) * 255`` as uint8 with
``base = 0.5 + 0.3 sin(2 pi 0.2 (x cos a + y sin a))``, ``a = 0.6 + 0.8 sin(x / 23) + 0.5 cos(y / 17)``,
``numpy.random.default_rng(seed)`` -- textured everywhere: on flat regions the reference's output is rounding noise.

Cases (H, W, seed): (5, 7, 6) smaller than the 17-tap window and the DoG's radius 40; (16, 17, 7); (33, 47, 0); (70, 90, 1);
and (33, 47, 0) again with patch size 32, which must give the same maps.

Per case: the image, the reference's float64 DoG plane and its float32 narrowing, the reference's ``deg`` and ``var``, and the
float64 restatement ``k64``, ``var64`` with the relative margin ``m = (F1 - F2) / F1`` of the two largest float64 responses.  A
pixel is *undecided* when ``m < 1e-5``.  Asserted here about the reference's float32 run: ``deg == k64`` on every decided pixel;
undecided pixels are at most 3 % of a case; ``|var32 - var64| <= 3e-6 max(var64)`` on decided pixels.

    python -m tests.golden.make_reference_orient_golden      # needs the reference checkout
"""
import importlib.util
import math
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

REF = "/root/reference/src/preprocessing/calc_orientation_maps.py"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_orient_golden.npz")
CASES = ((5, 7, 6), (16, 17, 7), (33, 47, 0), (70, 90, 1))
PATCH_CASE, PATCH_SIZE = 2, 32
DEFAULTS = dict(dog_low=0.4, dog_high=10, num_frequencies=1, num_filters=180, num_sigmas_x=1, num_sigmas_y=1, num_offsets=1,
                patch_size=64)
MARGIN, UNDECIDED_SHARE, VAR_REL = 1e-5, 0.03, 3e-6


def make_image(H, W, seed):
    g = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    a = 0.6 + 0.8 * np.sin(x / 23) + 0.5 * np.cos(y / 17)
    base = 0.5 + 0.3 * np.sin(2 * np.pi * 0.2 * (x * np.cos(a) + y * np.sin(a)))
    img = np.stack([base * 0.9, base * 0.7, base * 0.5], -1) + 0.05 * g.standard_normal((H, W, 3))
    return (np.clip(img, 0, 1) * 255).astype(np.uint8)


def gabor_kernel(frequency, theta=0, bandwidth=1, sigma_x=None, sigma_y=None, n_stds=3, offset=0, dtype=np.complex128):
    """skimage.filters.gabor_kernel, restated (see the module docstring)"""
    if sigma_x is None:
        sigma_x = math.sqrt(math.log(2) / 2) * (2 ** bandwidth + 1) / (2 ** bandwidth - 1) / (math.pi * frequency)
    if sigma_y is None:
        sigma_y = sigma_x
    ct, st = math.cos(theta), math.sin(theta)
    x0 = math.ceil(max(abs(n_stds * sigma_x * ct), abs(n_stds * sigma_y * st), 1))
    y0 = math.ceil(max(abs(n_stds * sigma_y * ct), abs(n_stds * sigma_x * st), 1))
    y, x = np.meshgrid(np.arange(-y0, y0 + 1), np.arange(-x0, x0 + 1), indexing="ij", sparse=True)
    rotx = x * ct + y * st
    roty = -x * st + y * ct
    g = np.empty(roty.shape, dtype=dtype)
    np.exp(-0.5 * (rotx ** 2 / sigma_x ** 2 + roty ** 2 / sigma_y ** 2), out=g)
    g /= 2 * math.pi * sigma_x * sigma_y
    g *= np.exp(1j * (2 * math.pi * frequency * rotx + offset))
    return g


def difference_of_gaussians(image, low_sigma, high_sigma=None):
    """skimage.filters.difference_of_gaussians on a float64 image with its defaults (mode 'nearest', truncate 4.0), restated"""
    from scipy import ndimage as ndi
    image = np.asarray(image, np.float64)
    if high_sigma is None:
        high_sigma = low_sigma * 1.6
    im1 = ndi.gaussian_filter(image, low_sigma, mode="nearest", cval=0, truncate=4.0)
    im2 = ndi.gaussian_filter(image, high_sigma, mode="nearest", cval=0, truncate=4.0)
    return im1 - im2


def load_reference():
    """the reference's module with the stand-ins in place of what is not installed"""
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    if "skimage" not in sys.modules:
        sk = stub("skimage")
        sk.filters = stub("skimage.filters", gabor_kernel=gabor_kernel, difference_of_gaussians=difference_of_gaussians)
    for name in ("cv2", "torchvision"):
        if name not in sys.modules:
            stub(name)
    if "torchvision.transforms" not in sys.modules:
        sys.modules["torchvision"].transforms = stub("torchvision.transforms", Resize=None, InterpolationMode=None)
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    spec = importlib.util.spec_from_file_location("ref_calc_orientation_maps", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def restate64(plane32, weights32, thetas):
    """responses, pick, variance and margin in float64 from the float32 plane and the float32 bank (the operands the reference's
    convolution sees); returns (F64 [F,H,W], k64, var64, margin)"""
    K = weights32.shape[-1]
    x = F.pad(torch.from_numpy(plane32).double(), (K // 2,) * 4)
    F64 = F.conv2d(x[None, None], torch.from_numpy(weights32).double()[:, None])[0].abs().numpy()
    n = F64.shape[0]
    k64 = F64.argmax(0)
    top = np.sort(F64, axis=0)[-2:] if n > 1 else np.stack([np.zeros_like(F64[0]), F64[0]])
    with np.errstate(invalid="ignore", divide="ignore"):
        margin = np.where(top[1] > 0, (top[1] - top[0]) / top[1], 0.0)
    o = k64 / n * math.pi
    th = np.asarray(thetas, np.float64)[:, None, None]
    d = np.minimum(np.abs(o[None] - th), np.minimum(np.abs(o[None] - th - math.pi), np.abs(o[None] - th + math.pi)))
    var64 = (d ** 2 * F64).sum(0) / np.maximum(F64.sum(0), 1e-12)
    return F64, k64, var64, margin


def main():
    ref = load_reference()
    kernel, thetas = ref.generate_gabor_filters(DEFAULTS["num_frequencies"], DEFAULTS["num_filters"], DEFAULTS["num_sigmas_x"],
                                                DEFAULTS["num_sigmas_y"], DEFAULTS["num_offsets"])
    bank = kernel.weight.data[:, 0].numpy().copy()
    assert bank.dtype == np.float32 and bank.shape == (180, 17, 17), bank.shape
    print("bank", bank.shape, "non-zero taps %.1f %%" % (100 * (bank != 0).mean()))
    out = {"bank": bank, "thetas": np.asarray(thetas, np.float64), "n_cases": np.int64(len(CASES)),
           "cases": np.asarray(CASES, np.int64), "patch_case": np.int64(PATCH_CASE)}
    for i, (H, W, seed) in enumerate(CASES):
        img = make_image(H, W, seed)
        deg, var, dog64 = ref.calc_orients(img, **DEFAULTS)
        if i == PATCH_CASE:
            deg_p, var_p, _ = ref.calc_orients(img, **dict(DEFAULTS, patch_size=PATCH_SIZE))
            assert np.array_equal(deg_p, deg) and np.array_equal(var_p, var), "the patch size changed the reference's maps"
        dog32 = torch.from_numpy(dog64).float().numpy()
        _, k64, var64, margin = restate64(dog32, bank, thetas)
        decided = margin >= MARGIN
        share = 1.0 - decided.mean()
        dv = np.abs(var.astype(np.float64) - var64)[decided].max() / var64.max()
        print("case %d (%d, %d, seed %d): undecided %.2f %%, deg != k64 at %d decided pixels, |var32 - var64| / max(var64) = %.3g"
              % (i, H, W, seed, 100 * share, int((deg != k64)[decided].sum()), dv))
        assert (deg == k64)[decided].all()
        assert share <= UNDECIDED_SHARE
        assert dv <= VAR_REL
        out.update({"c%d/image" % i: img, "c%d/dog64" % i: dog64, "c%d/dog32" % i: dog32, "c%d/deg" % i: deg.astype(np.uint8),
                    "c%d/var" % i: var.astype(np.float32), "c%d/k64" % i: k64.astype(np.uint8), "c%d/var64" % i: var64,
                    "c%d/margin" % i: margin})
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
