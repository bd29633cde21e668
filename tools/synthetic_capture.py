"""Synthetic captures of a known groom (gaussianhaircut_amd.synthetic_capture) as a scene on disk, and their time.

    python tools/synthetic_capture.py write --out SCENE [--strands groom.npy] [--mesh head.obj] [--views 8] [--size 256x256]
    python tools/synthetic_capture.py check --scene SCENE
    python tools/synthetic_capture.py time > profiles/synthetic_capture.txt

``write``: a groom [S, L, 3] (``.npy``; default: strands grown from a unit sphere), a head mesh (``.obj``; default: that sphere)
and a ring of cameras become a scene directory in the layout the reference's trainers read for its dataset type "Synthetic" after
``preprocess_synthetic_scene.py``: ``images/%04d.png``, ``masks/hair/``, ``masks/body/``, ``orientations/angles/%04d.png``,
``orientations/vars/%04d.npy`` (float16, as ``calc_orientation_maps.py`` saves them), ``flame_fitting/stage_3/mesh_final.obj``,
``projection.npy`` ([n, 4, 4] float64: ``K [R | t]`` per view at TWICE the written size, because ``readSyntheticSceneInfo`` halves
the intrinsics) and the groom itself as ``strands_gt.npy``.  ``check`` reads such a scene back -- the cameras through
``visibility.decompose_projection`` --, captures it afresh, asks every byte to be equal and attaches the ground truth to cameras
made from the files.  ``--composed`` runs the PyTorch form on the CPU.  ``time`` is the measurement of README.md's paragraph.
PIL is used here only, never in the library."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussianhaircut_amd import _lib  # noqa: E402
from gaussianhaircut_amd import ground_truth as gt  # noqa: E402
from gaussianhaircut_amd import strand_view as sv  # noqa: E402
from gaussianhaircut_amd import synthetic_capture as cap  # noqa: E402
from gaussianhaircut_amd import visibility as vis  # noqa: E402
from gaussianhaircut_amd.scene.cameras import Camera, ring_cameras  # noqa: E402

HBM_BPS = 6.29e12  # the measured float4 copy rate README.md's floors use
DIRS = ("images", "masks/hair", "masks/body", "orientations/angles", "orientations/vars", "flame_fitting/stage_3")


def uv_sphere(n_lon, n_lat, radius=1.0):
    """(vertices float32 [V, 3], faces int32 [F, 3]) of a closed UV sphere: 2 n_lon (n_lat - 1) faces"""
    v = [[0.0, radius, 0.0]]
    for a in range(1, n_lat):
        th = np.pi * a / n_lat
        for b in range(n_lon):
            ph = 2 * np.pi * b / n_lon
            v.append([radius * np.sin(th) * np.cos(ph), radius * np.cos(th), radius * np.sin(th) * np.sin(ph)])
    v.append([0.0, -radius, 0.0])
    f, last = [], len(v) - 1
    ring = lambda a, b: 1 + (a - 1) * n_lon + b % n_lon  # noqa: E731
    for b in range(n_lon):
        f.append([0, ring(1, b + 1), ring(1, b)])
        f.append([last, ring(n_lat - 1, b), ring(n_lat - 1, b + 1)])
        for a in range(1, n_lat - 1):
            f.append([ring(a, b), ring(a, b + 1), ring(a + 1, b + 1)])
            f.append([ring(a, b), ring(a + 1, b + 1), ring(a + 1, b)])
    return np.array(v, np.float32), np.array(f, np.int32)


def grown_hair(S, L, seed, radius=1.0):
    """S strands of L points that grow outwards from the sphere with a curl, their roots on it"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(S, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    side = np.cross(d, rng.normal(size=(S, 3)))
    side /= np.linalg.norm(side, axis=1, keepdims=True)
    u = np.linspace(0.0, 1.0, L)[None, :, None]
    length = rng.uniform(0.3, 0.9, (S, 1, 1))
    p = d[:, None] * (radius + length * u) + side[:, None] * (0.25 * length * np.sin(5.0 * u + rng.uniform(0, 6, (S, 1, 1))) * u)
    return np.ascontiguousarray(p.astype(np.float32))


def read_obj(path):
    v, f = [], []
    with open(path) as fh:
        for line in fh:
            p = line.split()
            if p and p[0] == "v":
                v.append([float(x) for x in p[1:4]])
            elif p and p[0] == "f":
                f.append([int(x.split("/")[0]) - 1 for x in p[1:4]])
    return np.array(v, np.float32).reshape(-1, 3), np.array(f, np.int32).reshape(-1, 3)


def write_obj(path, v, f):
    with open(path, "w") as fh:
        fh.write("".join("v %.9g %.9g %.9g\n" % tuple(p) for p in v) + "".join("f %d %d %d\n" % tuple(t + 1) for t in f))


def projection_of(M, H, W):
    """[4, 4] float64: K [R | t] of the view at twice its size (fx, fy, cx, cy doubled)"""
    K, R, t = vis.decompose_projection(np.asarray(M, np.float64).reshape(3, 4))
    K2 = K.copy()
    K2[:2] *= 2.0
    P = np.eye(4)
    P[:3] = K2 @ np.concatenate([R, t[:, None]], 1)
    return P


def view_of(P, H, W):
    """(M float32 [12], K, R, t) of a stored projection at the written size: the intrinsics halved"""
    K, R, t = vis.decompose_projection(np.asarray(P, np.float64)[:3, :4])
    K = K.copy()
    K[:2] /= 2.0
    return vis.view_matrix(K, R, t), K, R, t


def _capture(points, M, H, W, mesh, a, dev):
    return cap.capture_view(points, (M, H, W), mesh=mesh, supersample=a.supersample, half_width=a.half_width, var_floor=a.var_floor,
                            shadows=a.shadows, fused=not a.composed, device=dev)


def _device(a):
    return torch.device("cpu" if a.composed else "cuda:0")


def write(a):
    from PIL import Image
    H, W = (int(x) for x in a.size.split("x"))
    v, f = read_obj(a.mesh) if a.mesh else uv_sphere(24, 10)
    points = np.load(a.strands).astype(np.float32) if a.strands else grown_hair(a.default_strands, 24, 1)
    for d in DIRS:
        os.makedirs(os.path.join(a.out, d), exist_ok=True)
    write_obj(os.path.join(a.out, "flame_fitting/stage_3/mesh_final.obj"), v, f)
    np.save(os.path.join(a.out, "strands_gt.npy"), points)
    cams = ring_cameras(a.views, W, H, radius=a.radius, fovy_deg=a.fovy)
    P = np.stack([projection_of(vis.view_matrix_from_camera(c)[0], H, W) for c in cams])
    np.save(os.path.join(a.out, "projection.npy"), P)
    dev = _device(a)
    for k in range(a.views):
        M = view_of(P[k], H, W)[0]       # the view a reader of the file gets, not the camera's own: they differ by a rounding
        cv = _capture(points, M, H, W, (v, f), a, dev)
        name = "%04d" % k
        Image.fromarray(cv.image.cpu().numpy()).save(os.path.join(a.out, "images", name + ".png"))
        Image.fromarray(cv.mask_hair.cpu().numpy()).save(os.path.join(a.out, "masks/hair", name + ".png"))
        Image.fromarray(cv.mask_body.cpu().numpy()).save(os.path.join(a.out, "masks/body", name + ".png"))
        Image.fromarray(cv.angle.cpu().numpy()).save(os.path.join(a.out, "orientations/angles", name + ".png"))
        np.save(os.path.join(a.out, "orientations/vars", name + ".npy"), cv.var.cpu().numpy().astype(np.float16))
    print("synthetic_capture: wrote %d views of %d x %d (h x w), %d strands of %d points, %d faces to %s"
          % (a.views, H, W, points.shape[0], points.shape[1], len(f), a.out))
    return a.views


def check(a):
    from PIL import Image
    P = np.load(os.path.join(a.scene, "projection.npy"))
    points = np.load(os.path.join(a.scene, "strands_gt.npy"))
    v, f = read_obj(os.path.join(a.scene, "flame_fitting/stage_3/mesh_final.obj"))
    dev = _device(a)
    cams = []
    for k in range(len(P)):
        name = "%04d" % k
        files = dict(image=np.asarray(Image.open(os.path.join(a.scene, "images", name + ".png"))),
                     mask_hair=np.asarray(Image.open(os.path.join(a.scene, "masks/hair", name + ".png"))),
                     mask_body=np.asarray(Image.open(os.path.join(a.scene, "masks/body", name + ".png"))),
                     angle=np.asarray(Image.open(os.path.join(a.scene, "orientations/angles", name + ".png"))),
                     var=np.load(os.path.join(a.scene, "orientations/vars", name + ".npy")))
        H, W = files["image"].shape[:2]
        M, K, R, t = view_of(P[k], H, W)
        cv = _capture(points, M, H, W, (v, f), a, dev)
        for key in ("image", "mask_hair", "mask_body", "angle"):
            if not np.array_equal(getattr(cv, key).cpu().numpy(), files[key]):
                raise SystemExit("synthetic_capture check: view %s: %s differs from a fresh capture" % (name, key))
        if cv.var.cpu().numpy().astype(np.float16).tobytes() != files["var"].tobytes():
            raise SystemExit("synthetic_capture check: view %s: var differs from a fresh capture" % name)
        cam = Camera(R.T, t, 2 * np.arctan(W / 2.0 / K[0, 0]), 2 * np.arctan(H / 2.0 / K[1, 1]), W, H, image_name=name)
        gt.attach_ground_truth([cam], [{k_: torch.from_numpy(np.array(x)).to(dev) for k_, x in files.items()}])
        cams.append(cam)
    print("synthetic_capture: %d views of %s equal a fresh capture byte for byte; ground truth attached" % (len(P), a.scene))
    return cams


def _timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def time_(a):
    assert torch.cuda.is_available(), "synthetic_capture time needs a ROCm GPU (a CPU run measures nothing)"
    dev = torch.device("cuda:0")
    H, W = (int(x) for x in a.size.split("x"))
    S, L, s, r = a.strands_n, a.points_n, a.supersample, a.half_width
    v, f = uv_sphere(116, 44)            # 9976 faces: the face count of tools/strandviewstep.py's sphere
    pts = torch.from_numpy(grown_hair(S, L, 1)).to(dev)
    vd, fd = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    fl = 1.6 * min(H, W) / 2.0
    K = np.array([[fl, 0, W / 2.0], [0, fl, H / 2.0], [0, 0, 1.0]])
    eye = np.array([3.4 * np.sin(0.4), 0.35, 3.4 * np.cos(0.4)])
    z = -eye / np.linalg.norm(eye)
    x = np.cross(z, [0.0, 1.0, 0.0])
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    M = vis.view_matrix(K, R, -R @ eye)
    print("SYNTHCAPTURE strands=%d points=%d faces=%d %dx%d supersample=%d half_width=%g" % (S, L, len(f), H, W, s, r))
    Ms, rs = sv.supersampled(M, r, s)
    seg, _, face, _ = sv.rasterize_strands(pts, Ms, s * H, s * W, mesh=(vd, fd), half_width=rs, device=dev)
    fused = cap._maps_fused(pts, Ms, H, W, s, len(f), seg, face, vis.NEAR, 0.0)
    composed = cap._maps_torch(pts, Ms, H, W, s, len(f), seg, face, vis.NEAR, 0.0)
    assert all(torch.equal(x, y) for x, y in zip(fused[:3], composed[:3])) and \
        torch.equal(fused[3].view(torch.int32), composed[3].view(torch.int32)), "the forms disagree"
    print("SYNTHCAPTURE the launch and the composed maps are equal (three byte planes and the bits of var); hair subsamples %d, head "
          "subsamples %d of %d; pixels with hair %d of %d" % (int((seg >= 0).sum()), int((face >= 0).sum()), seg.numel(),
                                                              int((fused[0] > 0).sum()), H * W))
    outs = [torch.empty((H, W), dtype=torch.uint8, device=dev) for _ in range(3)] + [torch.empty((H, W), dtype=torch.float32, device=dev)]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    Mc, T = sv._mc(Ms), cap._table(dev)

    def launch():
        _lib.check(_lib.lib().ghr_strandview_capture(stream, S, L, ptr(pts), ctypes.byref(Mc), float(vis.NEAR), H, W, s, len(f), ptr(seg),
                                                     ptr(face), ptr(T), 0.0, *[ptr(t) for t in outs]))
    forms = {"capture": lambda: cap.capture_view(pts, (M, H, W), mesh=(vd, fd), supersample=s, half_width=r, device=dev),
             "render": lambda: sv.render_strands(pts, (M, H, W), mesh=(vd, fd), supersample=s, half_width=r, device=dev),
             "launch": launch,
             "composed": lambda: cap._maps_torch(pts, Ms, H, W, s, len(f), seg, face, vis.NEAR, 0.0)}
    for fn in forms.values():
        fn()
    best = {}
    for rd in range(3):
        for name, fn in forms.items():
            ms = _timed(fn)
            best[name] = min(best.get(name, ms), ms)
            print("SYNTHCAPTURE round %d %-8s %.4f ms" % (rd, name, ms))
    n = s * s
    traffic = (8.0 * n + 7.0) * H * W
    floor = traffic / HBM_BPS * 1e3
    print("SYNTHCAPTURE floor (DERIVED: %d B read and 7 B written per output pixel, %.0f MB, at the measured copy rate) %.4f ms"
          % (8 * n, traffic / 1e6, floor))
    print("SYNTHCAPTURE MEASURED best of three: capture_view %.4f ms (render_strands at the same arguments %.4f), the new launch alone "
          "%.4f ms = %.3f of the derived floor's rate, its composed form %.4f ms; launch / composed = %.5f"
          % (best["capture"], best["render"], best["launch"], floor / best["launch"], best["composed"], best["launch"] / best["composed"]))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    for name in ("write", "check", "time"):
        p = sub.add_parser(name)
        p.add_argument("--supersample", type=int, default=4)
        p.add_argument("--half_width", type=float, default=0.75)
        p.add_argument("--var_floor", type=float, default=0.0)
        p.add_argument("--shadows", action="store_true")
        p.add_argument("--composed", action="store_true", help="the PyTorch form on the CPU")
        if name == "write":
            p.add_argument("--out", required=True)
            p.add_argument("--strands", help="[S, L, 3] .npy (default: strands grown from the sphere)")
            p.add_argument("--default_strands", type=int, default=400)
            p.add_argument("--mesh", help=".obj (default: a UV sphere)")
            p.add_argument("--views", type=int, default=8)
            p.add_argument("--size", default="256x256", help="HxW")
            p.add_argument("--radius", type=float, default=4.0)
            p.add_argument("--fovy", type=float, default=40.0)
        elif name == "check":
            p.add_argument("--scene", required=True)
        else:
            p.add_argument("--size", default="1080x1920", help="HxW")
            p.add_argument("--strands_n", type=int, default=30000)
            p.add_argument("--points_n", type=int, default=100)
    a = ap.parse_args(argv)
    return {"write": write, "check": check, "time": time_}[a.cmd](a)


if __name__ == "__main__":
    main()
