"""The synthetic ground truth of the strand stages (gaussianhaircut_amd.ground_truth: ground_truth_from_render,
synthetic_view_ground_truth) against the files it replaces, and its time, on one GPU:

    python tools/render_views.py --model_path OUT --config tiny --views 4 --name train --scene_suffix _cropped --iteration 30000
    python tools/synthstep.py check --model_path OUT --config tiny --views 4 --iteration 30000 --scene_suffix _cropped
    python tools/synthstep.py time                  # writes profiles/synthetic_ground_truth.txt

``check`` reads ``<model_path>/<name><scene_suffix>/ours_<iteration>/{renders,head_masks,hair_masks,orients}/<view>.png`` and
``orient_confs/<view>.pth`` as the reference's loadCam does (Pillow and torch.load -- here and only here; the package needs
neither), builds the ground truth through ``synthetic_view_ground_truth``, renders the same model and cameras again (the model
arguments are those of tools/render_views.py) and reports, per plane, whether ``ground_truth_from_render`` of the fresh render is
the same bits.  Exit status 0 when every plane of every view is.

``time``: four forms of one view's ground truth from a packed [10,H,W] render that is already on the device, alternated in one
process over three rounds; per round and form the MEDIAN device time between two events around one call, over 20 calls after 3
warm-up calls (form c, which crosses the host, is timed on the host clock around a device synchronise).
  a  ground_truth_from_render: the direct launch
  b  products + assembly on the device: two launches (ghr_eval_products, ghr_gt_assemble with the / 255 table)
  c  products, device to host, host to device, synthetic_view_ground_truth: the file route without the files
  d  the torch-composed comparator on the device (fused=False)
The floor is DERIVED, not measured: 60 B per pixel (eight planes read, seven written) at 8 TB/s."""
import argparse
import datetime
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussianhaircut_amd import evaluation as ev  # noqa: E402
from gaussianhaircut_amd import ground_truth as gt  # noqa: E402

PLANES = ("original_image", "original_mask", "original_orient_angle", "original_orient_conf")
DIRS = dict(render="renders", head_mask="head_masks", hair_mask="hair_masks", orient="orients", orient_conf="orient_confs")
SIZES = ((1080, 1920), (2160, 3840))   # w x h: a portrait view at the // 2 the reference trains on, and at full size
WARMUP, CALLS, ROUNDS = 3, 20, 3
PEAK_BW = 8e12
BYTES_PER_PIXEL = 60


def read_view(base, stem):
    """the five files of one view as loadCam opens them: uint8 [H,W,3] arrays and the float [1,H,W] plane"""
    from PIL import Image
    out = {k: np.array(Image.open(os.path.join(base, DIRS[k], stem + ".png"))) for k in ("render", "head_mask", "hair_mask", "orient")}
    out["orient_conf"] = torch.load(os.path.join(base, DIRS["orient_conf"], stem + ".pth")).float().numpy()
    return out


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def check(a):
    from gaussianhaircut_amd.scene.cameras import ring_cameras
    from gaussianhaircut_amd.scene.gaussian_model import GaussianModel
    from gaussianhaircut_amd.utils import synthetic as syn
    dev = torch.device("cuda:0")
    spec = syn.CONFIGS[a.config]
    if a.ply:
        model = GaussianModel(3)
        model.load_ply(a.ply, device=dev)
    else:
        model = syn.make_model(spec, dev)
    W, H = a.width or spec.W, a.height or spec.H
    cams = ring_cameras(a.views, W, H, device=dev)
    bg = torch.tensor(([1, 1, 1] if a.white_background else [0, 0, 0]) + [0, 0, 0, 0, 0, 0, 100], dtype=torch.float32, device=dev)
    base = os.path.join(a.model_path, "%s%s" % (a.name, a.scene_suffix), "ours_{}".format(a.iteration))
    bad = 0
    for k, cam in enumerate(cams):
        stem = "%05d" % k
        f = read_view(base, stem)
        from_files = gt.synthetic_view_ground_truth(*(torch.from_numpy(f[n]).to(dev) for n in ("render", "head_mask", "hair_mask", "orient",
                                                                                                "orient_conf")),
                                                    white_background=a.white_background, binarize_masks=a.binarize_masks)
        with torch.no_grad():
            packed = ev._render_view(cam, model, None, ev._default_pipe(), bg).renders_packed
        direct = gt.ground_truth_from_render(packed, white_background=a.white_background, binarize_masks=a.binarize_masks)
        for name in PLANES:
            x, y = getattr(from_files, name), getattr(direct, name)
            same = same_bits(x, y)
            bad += not same
            print("SYNTHSTEP check view %s %-22s %s" % (stem, name, "equal bit for bit" if same else
                                                         "DIFFERS at %d of %d elements" % (int((x != y).sum()), x.numel())))
    print("SYNTHSTEP check: %d views under %s, %s" % (len(cams), base, "every plane equal bit for bit" if not bad else "%d planes differ" % bad))
    return 1 if bad else 0


def make_packed(w, h, dev, seed=0):
    """a packed render's value ranges without a scene: colours and masks a little outside [0, 1], directions of any sign, positive
    confidence"""
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(10, h, w, generator=g) * 1.2 - 0.1
    p[5:8] = torch.randn(3, h, w, generator=g)
    p[8] = torch.rand(h, w, generator=g) ** 2 * 40
    return p.to(dev)


def median_event_ms(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(CALLS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def median_host_ms(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def form_b(packed):
    img, hair, head, orient, conf = gt.core_products_fused(packed)
    o = gt._assemble_launch(img, hair, head, orient, None, False, False, False, None, 255)
    return o[0], o[1], o[2], conf[None]


def form_c(packed):
    _, H, W = packed.shape
    p = ev.split_product_block(ev.products_fused(packed).cpu().numpy(), W, H, copy=False)
    dev = packed.device
    return gt.synthetic_view_ground_truth(*(torch.from_numpy(p[n]).to(dev) for n in ("render", "head_mask", "hair_mask", "orient", "orient_conf")))


def timing(a):
    dev = torch.device("cuda:0")
    arch = getattr(torch.cuda.get_device_properties(dev), "gcnArchName", "")
    lines = ["# tools/synthstep.py time, %s %s, one process, %s" % (torch.cuda.get_device_name(dev), arch, datetime.date.today().isoformat()),
             "SYNTHSTEP one view's ground truth from a packed [10,H,W] render on the device; per round the median of %d calls after "
             "%d warm-up calls; device events (form c: host clock around a synchronise)" % (CALLS, WARMUP)]
    for w, h in SIZES:
        packed = make_packed(w, h, dev)
        tag = "SYNTHSTEP %4d x %-4d" % (w, h)
        forms = (("a  direct launch", lambda: gt.ground_truth_from_render(packed), median_event_ms),
                 ("b  products + assembly on the device", lambda: form_b(packed), median_event_ms),
                 ("c  products, D2H, H2D, synthetic_view_ground_truth", lambda: form_c(packed), median_host_ms),
                 ("d  torch comparator on the device", lambda: gt.ground_truth_from_render(packed, fused=False), median_event_ms))
        ra, rb, rc = forms[0][1](), forms[1][1](), forms[2][1]()
        lines.append("%s forms a, b and c agree bit for bit on all four tensors: %s"
                     % (tag, all(same_bits(x, y) and same_bits(x, z) for x, y, z in zip(ra[:4], rb, rc[:4]))))
        res = {}
        for rnd in range(ROUNDS):
            for name, fn, clock in forms:
                med, lo, hi = clock(fn)
                res.setdefault(name, []).append(med)
                lines.append("%s round %d  %-52s median %9.4f ms  (min %9.4f, max %9.4f)" % (tag, rnd + 1, name, med, lo, hi))
        floor_ms = BYTES_PER_PIXEL * w * h / PEAK_BW * 1e3
        best = {n: min(v) for n, v in res.items()}
        fa = best[forms[0][0]]
        lines.append("%s DERIVED floor: %d B per pixel = %.1f MB at %.0f TB/s = %.4f ms; form a's best round reaches %.1f %% of it"
                     % (tag, BYTES_PER_PIXEL, BYTES_PER_PIXEL * w * h / 1e6, PEAK_BW / 1e12, floor_ms, 100 * floor_ms / fa))
        for name, _, _ in forms[1:]:
            lines.append("%s form a is %.2fx the speed of form %s (best rounds: %.4f against %.4f ms)"
                         % (tag, best[name] / fa, name.split()[0], fa, best[name]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


def main(argv=None):
    from gaussianhaircut_amd.utils import synthetic as syn
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    c = sub.add_parser("check")
    c.add_argument("--model_path", required=True)
    c.add_argument("--iteration", type=int, required=True)
    c.add_argument("--scene_suffix", default="_cropped")
    c.add_argument("--name", default="train")
    c.add_argument("--ply")
    c.add_argument("--config", default="tiny", choices=sorted(syn.CONFIGS))
    c.add_argument("--views", type=int, default=16)
    c.add_argument("--width", type=int)
    c.add_argument("--height", type=int)
    c.add_argument("--white_background", action="store_true")
    c.add_argument("--binarize_masks", action="store_true")
    t = sub.add_parser("time")
    t.add_argument("--out", default=os.path.join(ROOT, "profiles", "synthetic_ground_truth.txt"))
    a = ap.parse_args(argv)
    return check(a) if a.cmd == "check" else timing(a)


if __name__ == "__main__":
    sys.exit(main())
