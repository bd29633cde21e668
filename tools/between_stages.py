"""The steps the reference's run.sh takes between its training stages, on the reference's directory layout:

    python tools/between_stages.py crop   --model_path M --path_to_data D [--iter 30000]
        M/point_cloud/iteration_N/raw_point_cloud.ply -> M/point_cloud_cropped/iteration_N/point_cloud.ply (+ raw_), D/scale.pickle
    python tools/between_stages.py filter --model_path M --mesh HEAD.obj [--iter 30000] [--probe reference]
        M/point_cloud_cropped/iteration_N/raw_point_cloud.ply -> M/point_cloud_filtered/iteration_N/point_cloud.ply (+ raw_)
    python tools/between_stages.py export --points P.npy|P.pkl --mesh HEAD.obj --out_dir DIR [--iter 30000]
        strand points [S, L, 3] -> DIR/N_strands.pkl, DIR/N_strands.ply
    python tools/between_stages.py split  --points P.npy|P.pkl --mesh HEAD.obj --out_dir DIR [--scalp SCALP.obj] [--max_root_dist 0.1]
        strand points [S, L, 3] -> DIR/N_strands.pkl, DIR/N_strands.ply: strands cut where they enter the head, the pieces after a
        cut re-rooted on the scalp mesh when it is given and nearer than --max_root_dist (dropped otherwise)
    python tools/between_stages.py scalp  --mesh HEAD.obj --cams CAMS.pkl --path_to_data D --out_dir FLAME_DIR
                                          --scalp_idx I --scalp_faces F --scalp_uvs UV [--seam_pairs SEAMS.json]
        D/masks_2/{body,hair}/<view>.png -> FLAME_DIR/scalp_data/{scalp.obj, cut_scalp_verts.pickle, dif_mask.png, vis/<view>.jpg}
        CAMS.pkl: the reference's cameras pickle (view -> 4 x 4 projection, stored transposed), or a pickle of a list of this
        package's cameras (their image_name names the masks).  I, F, UV: the scalp template's vertex indices into the head mesh,
        its faces and its UV map, each a .npy, .pkl or .pth file; SEAMS.json: {"groups": [[...], ...]}, scalp vertices kept or cut
        together.

    python tools/between_stages.py grow   --ply STAGE1.ply | --model_path M  --scalp SCALP.obj --out_dir DIR [--scalp_uvs UV]
                                          [--num_strands 30000] [--strand_length 100] [--radius R] [--step_length H] [--max_steps 400]
                                          [--mesh HEAD.obj [--avoid [--margin M]]] [--seed 0] [--smooth ITER]
        the hair Gaussians of a stage-1 model (default M/point_cloud_filtered/iteration_N/point_cloud.ply) -> an initial groom grown
        from roots sampled on the scalp along its normals (strand_growing.grow_strands): DIR/N_strands.pkl,
        DIR/N_strands.ply, DIR/N_strands_rgb.npy.  --mesh prunes the strands that run inside the head; with --avoid the trace itself
        keeps every step at least M off the head (default M: the step length).  Without --scalp_uvs the scalp's two
        widest coordinates stand in for its UV map (only the roots' normals are used, not their tangents).  --smooth ITER runs ITER
        Adam steps on the strand shape term alone (stretch, bend, neighbour coherence) over the groom before export;
        the term knows no mesh, so with --avoid the points it moved inside the margin are counted and printed.

    python tools/between_stages.py upsample --points GUIDES.npy|GUIDES.pkl --scalp SCALP.obj --out_dir DIR --count 150000
                                            [--scalp_uvs UV] [--seed 0] [--radius R] [--tau 0.5 | --no_gate] [--mesh HEAD.obj]
                                            [--features RGB.npy] [--with_guides]
        guide strands [G, L, 3] -> a denser groom (strand_upsampling.upsample_strands): --count child roots and
        their frames drawn on the scalp (strand_generator.sample_roots), every child a blend of its 4 nearest guides in scalp-local
        frames, gated by shape similarity at --tau; the guides' own frames are those of the scalp faces nearest to their roots
        (strand_upsampling.frames_at).  The scalp's UVs come from --scalp_uvs, else from the obj's `vt` records (the first one a
        vertex is used with), else its two widest coordinates stand in.  --radius leaves a child without a guide that near out;
        --mesh prunes the children that run inside the head.  DIR/N_strands.pkl, DIR/N_strands.ply (--with_guides: the guides
        first), and DIR/N_strands_rgb.npy when --features [G, F] is given.

(src/preprocessing/scale_scene_into_sphere.py, filter_flame_intersections.py, export_strands.py,
extract_non_visible_head_scalp.py.)  Containment and visibility run in HIP on cuda:0; --composed evaluates the PyTorch-composed
forms instead (any device, slow)."""
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


def _load_array(path):
    if path.endswith(".npy"):
        return np.load(path)
    if path.endswith((".pth", ".pt")):
        return torch.load(path, map_location="cpu").numpy()
    with open(path, "rb") as f:
        return np.asarray(pickle.load(f))


def _scalp(a, fused, dev):
    from PIL import Image
    from gaussianhaircut_amd import visibility as vis
    from gaussianhaircut_amd.mesh import read_obj
    v, f = read_obj(a.mesh)
    with open(a.cams, "rb") as fh:
        cams = pickle.load(fh)
    read = lambda kind, name: np.asarray(Image.open(os.path.join(a.path_to_data, "masks_2", kind, "%s.png" % name)).convert("L"))  # noqa: E731
    if isinstance(cams, dict):
        names = list(cams)
        masks = [(read("body", n), read("hair", n)) for n in names]
        P = {n: (cams[n].T if isinstance(cams[n], np.ndarray) else cams[n].transpose(0, 1)) for n in names}
        by_name = vis.views_from_projections(P, {n: m[0].shape for n, m in zip(names, masks)})
        views = [by_name[n] for n in names]
    else:
        names = [c.image_name for c in cams]
        views = [vis.view_matrix_from_camera(c) for c in cams]
        masks = [(read("body", n), read("hair", n)) for n in names]
    cnt, cnt_head, planes = vis.vertex_visibility((v, f), views, masks, fused=fused, device=dev)
    vertex_mask = vis.visible_vertex_mask(cnt, cnt_head, len(views), a.prob_thr, a.n_views_thr)
    idx, sf, uv = _load_array(a.scalp_idx), _load_array(a.scalp_faces), _load_array(a.scalp_uvs)
    seams = bs.load_seam_pairs(a.seam_pairs) if a.seam_pairs else []
    kept, faces = bs.cut_scalp(vertex_mask, idx, sf, seams)
    dif = bs.scalp_uv_mask(uv.reshape(-1, 2)[kept], faces, fused=fused, device=dev)
    out = bs.write_scalp_data(a.out_dir, v[np.asarray(idx).reshape(-1)], kept, faces, dict(zip(names, planes)), dif)
    print("scalp: %d views; %d of %d head vertices marked; kept %d of %d scalp vertices, %d of %d faces -> %s"
          % (len(views), int(vertex_mask.sum()), len(v), len(kept), len(np.asarray(idx).reshape(-1)), len(faces), len(sf.reshape(-1, 3)), out))


def _grow(a, fused, dev):
    from gaussianhaircut_amd import strand_generator as sgen
    from gaussianhaircut_amd import strand_growing as sg
    from gaussianhaircut_amd.mesh import read_obj
    ply = a.ply or os.path.join(a.model_path, "point_cloud_filtered", "iteration_%d" % a.iter, "point_cloud.ply")
    field = sg.HairField.from_model(_load(ply, a.sh_degree, dev), a.label_threshold)
    v, f = read_obj(a.scalp)
    v, f = torch.as_tensor(np.asarray(v, np.float32)), torch.as_tensor(np.asarray(f, np.int64))
    if a.scalp_uvs:
        uv = torch.as_tensor(np.asarray(_load_array(a.scalp_uvs), np.float32)).reshape(-1, 2)
    else:
        wide = torch.argsort(v.max(0).values - v.min(0).values, descending=True)[:2].sort().values
        uv = v[:, wide]
    roots = sgen.sample_roots(v, f, uv, a.num_strands, generator=torch.Generator().manual_seed(a.seed))
    normals = roots["local2world"][:, :, 2].contiguous()
    out = sg.grow_strands(field, roots["origins"].to(dev), normals.to(dev), L=a.strand_length, radius=a.radius, step=a.step_length,
                          max_steps=a.max_steps, mesh=HeadMesh.from_obj(a.mesh) if a.mesh else None, fused=fused, avoid=a.avoid,
                          margin=a.margin)
    print("grow: %d hair Gaussians, radius %.5g, step %.5g, rho_min %.5g; kept %d of %d strands (steps: median %d, longest %d)"
          % (field.P, out["radius"], out["step"], out["rho_min"], int(out["keep"].sum()), a.num_strands,
             int(out["steps"].float().median()), int(out["steps"].max())))
    if a.avoid:
        stop = torch.bincount(out["stop"].long().cpu(), minlength=3).tolist()
        print("grow: margin %.5g; contact steps per strand: median %d, most %d; stopped: %d out of steps, %d coasted out, %d head-on"
              % (out["margin"], int(out["contacts"].float().median()), int(out["contacts"].max()), stop[0], stop[1], stop[2]))
    points = out["points"]
    if a.smooth > 0 and points.shape[0] > 0:
        from gaussianhaircut_amd import strand_shape as ss
        shape = ss.StrandShape(points[:, :1], points[:, 1:] - points[:, :-1], fused=fused)
        before = shape.terms(points[:, 1:] - points[:, :-1]).tolist()
        points = ss.smooth_polylines(points, a.smooth, fused=fused, shape=shape)
        after = shape.terms(points[:, 1:] - points[:, :-1]).tolist()
        print("smooth: %d Adam steps on the shape term; stretch %.4g -> %.4g, bend %.4g -> %.4g, coherence %.4g -> %.4g"
              % (a.smooth, before[0], after[0], before[1], after[1], before[2], after[2]))
        if a.avoid:  # the term knows no mesh: say what it undid of the guarded trace
            from gaussianhaircut_amd.mesh import signed_distance
            sd = signed_distance(points[:, 1:].reshape(-1, 3), HeadMesh.from_obj(a.mesh), fused=fused)
            print("smooth: %d of %d free points are now nearer to the head than the margin %.5g"
                  % (int((sd < out["margin"]).sum()), sd.numel(), out["margin"]))
    print("export: %s %s" % bs.export_strands(points, a.out_dir, a.iter))
    np.save(os.path.join(a.out_dir, "%s_strands_rgb.npy" % a.iter), out["rgb"].cpu().numpy())


def _obj_uvs(path, num_vertices):
    """[V, 2] from an obj's `vt` records through its faces' `v/vt` corners (the first one a vertex is used with), or None"""
    vts, uv = [], {}
    with open(path, "r") as fh:
        for line in fh:
            tok = line.split()
            if not tok:
                continue
            if tok[0] == "vt":
                vts.append([float(tok[1]), float(tok[2])])
            elif tok[0] == "f":
                for t in tok[1:]:
                    part = t.split("/")
                    if len(part) > 1 and part[1]:
                        a, b = int(part[0]), int(part[1])
                        uv.setdefault(a - 1 if a > 0 else num_vertices + a, b - 1 if b > 0 else len(vts) + b)
    if not vts or len(uv) < num_vertices:
        return None
    return np.asarray([vts[uv[i]] for i in range(num_vertices)], np.float32)


def _upsample(a, fused, dev):
    from gaussianhaircut_amd import strand_generator as sgen
    from gaussianhaircut_amd import strand_upsampling as su
    from gaussianhaircut_amd.mesh import read_obj
    guides = torch.from_numpy(np.ascontiguousarray(_load_array(a.points), np.float32)).to(dev)
    v_np, f_np = read_obj(a.scalp)
    v, f = torch.as_tensor(np.asarray(v_np, np.float32)), torch.as_tensor(np.asarray(f_np, np.int64))
    uv = np.asarray(_load_array(a.scalp_uvs), np.float32).reshape(-1, 2) if a.scalp_uvs else _obj_uvs(a.scalp, len(v_np))
    if uv is None:
        wide = torch.argsort(v.max(0).values - v.min(0).values, descending=True)[:2].sort().values
        uv = v[:, wide]
    uv = torch.as_tensor(uv)
    roots = sgen.sample_roots(v, f, uv, a.count, generator=torch.Generator().manual_seed(a.seed))
    guide_frames = su.frames_at(HeadMesh(v_np, f_np), sgen.scalp_frames(v, f, uv), guides[:, 0], fused=fused)
    feats = torch.from_numpy(np.ascontiguousarray(_load_array(a.features), np.float32)).to(dev) if a.features else None
    out = su.upsample_strands(guides, guide_frames, roots["origins"].to(dev), roots["local2world"].to(dev), features=feats,
                              radius=a.radius, tau=None if a.no_gate else a.tau, mesh=HeadMesh.from_obj(a.mesh) if a.mesh else None,
                              fused=fused)
    keep = out["keep"]
    used = (out["weights"][out["valid"]] > 0).sum(1).float()
    print("upsample: %d guides of %d points, %d children; eps2 %.5g; %d without a guide in reach, %d pruned by the head; kept %d "
          "(guides carrying weight per child: mean %.2f)"
          % (guides.shape[0], guides.shape[1], a.count, out["eps2"], int((~out["valid"]).sum()), int((out["valid"] & ~keep).sum()),
             int(keep.sum()), float(used.mean()) if used.numel() else 0.0))
    points = out["points"][keep]
    if a.with_guides:
        points = torch.cat([guides, points])
    print("export: %s %s" % bs.export_strands(points, a.out_dir, a.iter))
    if feats is not None:
        rgb = out["features"][keep]
        np.save(os.path.join(a.out_dir, "%s_strands_rgb.npy" % a.iter), (torch.cat([feats.reshape(guides.shape[0], -1), rgb]) if a.with_guides else rgb).cpu().numpy())


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("step", choices=["crop", "filter", "export", "split", "scalp", "grow", "upsample"])
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
    ap.add_argument("--cams")
    ap.add_argument("--scalp_idx")
    ap.add_argument("--scalp_faces")
    ap.add_argument("--scalp_uvs")
    ap.add_argument("--seam_pairs")
    ap.add_argument("--scalp")
    ap.add_argument("--max_root_dist", type=float, default=0.1)
    ap.add_argument("--prob_thr", type=float, default=0.5)
    ap.add_argument("--n_views_thr", type=float, default=0.1)
    ap.add_argument("--ply")
    ap.add_argument("--num_strands", type=int, default=30_000)
    ap.add_argument("--strand_length", type=int, default=100)
    ap.add_argument("--radius", type=float, default=None)
    ap.add_argument("--step_length", type=float, default=None)
    ap.add_argument("--max_steps", type=int, default=400)
    ap.add_argument("--label_threshold", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--avoid", action="store_true")
    ap.add_argument("--margin", type=float, default=None)
    ap.add_argument("--smooth", type=int, default=0)
    ap.add_argument("--count", type=int, default=150_000)
    ap.add_argument("--tau", type=float, default=0.5)
    ap.add_argument("--no_gate", action="store_true")
    ap.add_argument("--features")
    ap.add_argument("--with_guides", action="store_true")
    a = ap.parse_args(argv)
    fused = not a.composed
    dev = torch.device(a.device or ("cuda:0" if fused else "cpu"))
    it = "iteration_%d" % a.iter
    if a.step == "scalp":
        _scalp(a, fused, dev)
    elif a.step == "grow":
        _grow(a, fused, dev)
    elif a.step == "upsample":
        _upsample(a, fused, dev)
    elif a.step == "crop":
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
    elif a.step == "split":
        p = torch.from_numpy(np.ascontiguousarray(_load_array(a.points), np.float32)).to(dev)
        pieces, source = bs.split_strands(p, HeadMesh.from_obj(a.mesh), HeadMesh.from_obj(a.scalp) if a.scalp else None,
                                          max_root_dist=a.max_root_dist, fused=fused)
        print("split: %d strands -> %d pieces of %d strands" % (p.shape[0], pieces.shape[0], int(torch.unique(source).numel())))
        print("export: %s %s" % bs.export_strands(pieces, a.out_dir, a.iter))
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
