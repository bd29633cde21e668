"""Is a point inside the head mesh (csrc/ghr_mesh.h): what the steps between the training stages ask of
``pysdf.SDF(vertices, faces)(points) < 0`` -- only ever the sign.

``HeadMesh(vertices, faces)`` builds the per-axis grids once on the host (``ghr_mesh_grid_build``, deterministic) and keeps a
copy per device.  ``contains`` / ``probes_outside`` launch the HIP kernels (``fused=True``, ROCm tensors only: there is no CPU
path) or evaluate the PyTorch-composed comparator (``fused=False``, any device): the same float32 expressions in the same
operand order, brute force over all faces in chunks -- the grid changes which faces are looked at, never the answer.

The definition of "inside" is this package's own (three axis rays with exact, complementary edge predicates, majority of the
three parities); on a closed mesh, away from the surface, it agrees with every sound definition, pysdf's included.

``closest_point`` / ``signed_distance`` (csrc/ghr_meshdist.h) add the magnitude: the closest point of the mesh, its
squared distance and its face by a definition of our own (three clamped edge candidates and a clamped interior candidate per
face in float32, the smallest ``d``, the lowest face index among equals), the sign from ``contains``.  The triangle blob (faces in
Morton order, blocks of 64 with their boxes) is built on first use and kept per device.  The module-level ``signed_distance`` is
differentiable in the points.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib

PROBES = {"reference": _lib.PROBE_REFERENCE, "ellipsoid": _lib.PROBE_REFERENCE, "axis_scaled": _lib.PROBE_AXIS_SCALED}

# pytorch3d's level-0 ``ico_sphere`` (quoted from memory to the four digits it tabulates; not a dependency): the one table of
# the probe directions, in the order of ghr::mesh_ico_vertex (csrc/ghr_mesh.h), which generates the same twelve.
_A, _B = 0.5257, 0.8507
ICO_VERTS = ((-_A, _B, 0.0), (_A, _B, 0.0), (-_A, -_B, 0.0), (_A, -_B, 0.0),
             (0.0, -_A, _B), (0.0, _A, _B), (0.0, -_A, -_B), (0.0, _A, -_B),
             (_B, 0.0, -_A), (_B, 0.0, _A), (-_B, 0.0, -_A), (-_B, 0.0, _A))


def read_obj(path: str):
    """``v`` / ``f`` lines of a Wavefront OBJ: vertices [V,3] float32, faces [F,3] int32.  Indices may be ``a``, ``a/b``, ``a//c`` or
    ``a/b/c`` (the first is taken) and negative (relative to the vertices read so far); polygons are fanned from their first
    corner."""
    verts, faces = [], []
    with open(path, "r") as fh:
        for line in fh:
            tok = line.split()
            if not tok:
                continue
            if tok[0] == "v":
                verts.append([float(tok[1]), float(tok[2]), float(tok[3])])
            elif tok[0] == "f":
                idx = []
                for t in tok[1:]:
                    i = int(t.split("/")[0])
                    idx.append(i - 1 if i > 0 else len(verts) + i)
                for k in range(1, len(idx) - 1):
                    faces.append([idx[0], idx[k], idx[k + 1]])
    return (np.asarray(verts, np.float32).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3))


def _launch_env(t):
    from .diff_gaussian_rasterization import _on_device, _ptr, _stream
    return _on_device(t.device), _ptr, _stream


class HeadMesh:
    def __init__(self, vertices, faces, grid: int = 0):
        """``grid``: cells per side of each axis' grid; 0 takes ceil(sqrt(F)) (at most 256)."""
        v = vertices.detach().cpu().numpy() if isinstance(vertices, torch.Tensor) else np.asarray(vertices)
        f = faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else np.asarray(faces)
        self.vertices = np.ascontiguousarray(v, np.float32).reshape(-1, 3)
        self.faces = np.ascontiguousarray(f, np.int32).reshape(-1, 3)
        L = _lib.lib()
        nv, nf = len(self.vertices), len(self.faces)
        self.header = _lib.MeshGrid()
        _lib.check(L.ghr_mesh_grid_sizes(nv, self.vertices.ctypes.data, nf, self.faces.ctypes.data, int(grid),
                                         ctypes.byref(self.header)))
        nbytes = int(self.header.bytes)
        self._blob = torch.empty(nbytes, dtype=torch.uint8)  # (torch's allocations are 64-B aligned)
        _lib.check(L.ghr_mesh_grid_build(nv, self.vertices.ctypes.data, nf, self.faces.ctypes.data, int(grid),
                                         self._blob.data_ptr(), nbytes))
        ctypes.memmove(ctypes.byref(self.header), self._blob.data_ptr(), ctypes.sizeof(self.header))
        self._dev = {}
        self._cmp = {}
        self._tris_header = None  # the closest-point tables: built on first use
        self._tris_blob = None
        self._tris_dev = {}
        self._tris_cmp = {}

    @classmethod
    def from_obj(cls, path: str, grid: int = 0):
        return cls(*read_obj(path), grid=grid)

    # ------------------------------------------------------------------ the grid
    @property
    def grid(self) -> int:
        return int(self.header.G)

    def grid_blob(self) -> np.ndarray:
        """The host copy of the tables, bytes (tests compare it with the host simulator's)."""
        return self._blob.numpy()

    def grid_stats(self):
        """Per axis: (mean, max) length of the cell lists."""
        cells = self.grid * self.grid
        return [(self.header.list_total[a] / cells, int(self.header.list_max[a])) for a in range(3)]

    def _tables(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = self._blob.to(device)
        return self._dev[key]

    # ------------------------------------------------------------------ fused
    def _contains_fused(self, pts, return_crossings):
        if not pts.is_cuda:
            raise RuntimeError("HeadMesh.contains(fused=True) needs a tensor on a ROCm device: the kernels have no CPU path "
                               "(fused=False is the PyTorch form)")
        Q = pts.shape[0]
        inside = torch.empty(Q, dtype=torch.uint8, device=pts.device)
        cross = torch.empty((Q, 3), dtype=torch.int32, device=pts.device) if return_crossings else None
        guard, _ptr, _stream = _launch_env(pts)
        with guard:
            tab = self._tables(pts.device)
            _lib.check(_lib.lib().ghr_mesh_contains(_stream(), ctypes.byref(self.header), _ptr(tab), Q, _ptr(pts), _ptr(inside),
                                                    _ptr(cross) if return_crossings else None))
        return inside.bool(), cross

    def _probes_fused(self, xyz, scaling, rotation, mode):
        if not xyz.is_cuda:
            raise RuntimeError("HeadMesh.probes_outside(fused=True) needs tensors on a ROCm device: the kernels have no CPU path "
                               "(fused=False is the PyTorch form)")
        P = xyz.shape[0]
        out = torch.empty(P, dtype=torch.uint8, device=xyz.device)
        guard, _ptr, _stream = _launch_env(xyz)
        with guard:
            tab = self._tables(xyz.device)
            _lib.check(_lib.lib().ghr_gaussian_probe_outside(_stream(), ctypes.byref(self.header), _ptr(tab), P, _ptr(xyz),
                                                             _ptr(scaling), _ptr(rotation), mode, _ptr(out)))
        return out.bool()

    # ------------------------------------------------------------------ composed
    def _comparator_tables(self, device):
        """Per axis the projected vertices, heights, direction bits and never-counts flags of every face, as tensors."""
        key = str(device)
        if key in self._cmp:
            return self._cmp[key]
        v, f = self.vertices, self.faces
        rep = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])
        axes = []
        for a in range(3):
            U, V = (a + 1) % 3, (a + 2) % 3
            pu, pv, ph = [[v[f[:, k], c] for k in range(3)] for c in (U, V, a)]
            never = rep | ((pu[1] - pu[0]) * (pv[2] - pv[0]) - (pv[1] - pv[0]) * (pu[2] - pu[0]) == 0)  # float32, as mesh_flat
            flip = [f[:, k] > f[:, (k + 1) % 3] for k in range(3)]
            t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)  # noqa: E731
            axes.append(dict(pu=[t(x) for x in pu], pv=[t(x) for x in pv], ph=[t(x) for x in ph], never=t(never),
                             flip=[t(x) for x in flip]))
        used = v[f.reshape(-1)] if len(f) else np.zeros((0, 3), np.float32)
        lo = torch.from_numpy(used.min(0) if len(f) else np.ones(3, np.float32)).to(device)
        hi = torch.from_numpy(used.max(0) if len(f) else -np.ones(3, np.float32)).to(device)
        self._cmp[key] = (axes, lo, hi)
        return self._cmp[key]

    def _contains_torch(self, pts, chunk_elems: int = 1 << 22):
        axes, lo, hi = self._comparator_tables(pts.device)
        Q, F = pts.shape[0], len(self.faces)
        cross = torch.zeros((Q, 3), dtype=torch.int32, device=pts.device)
        if Q and F:
            ok = ((pts >= lo) & (pts <= hi)).all(dim=1)  # (a NaN fails both comparisons)
            idx = ok.nonzero(as_tuple=True)[0]
            chunk = max(1, chunk_elems // F)
            for a in range(3):
                U, V = (a + 1) % 3, (a + 2) % 3
                t = axes[a]
                ulo, uhi = torch.minimum(torch.minimum(t["pu"][0], t["pu"][1]), t["pu"][2]), torch.maximum(torch.maximum(t["pu"][0], t["pu"][1]), t["pu"][2])
                vlo, vhi = torch.minimum(torch.minimum(t["pv"][0], t["pv"][1]), t["pv"][2]), torch.maximum(torch.maximum(t["pv"][0], t["pv"][1]), t["pv"][2])
                for s in range(0, int(idx.numel()), chunk):
                    ii = idx[s:s + chunk]
                    pu, pv, ph = pts[ii, U][:, None], pts[ii, V][:, None], pts[ii, a][:, None]
                    side, e = [], []
                    for k in range(3):
                        k1 = (k + 1) % 3
                        flip = t["flip"][k]
                        au, av = torch.where(flip, t["pu"][k1], t["pu"][k]), torch.where(flip, t["pv"][k1], t["pv"][k])
                        bu, bv = torch.where(flip, t["pu"][k], t["pu"][k1]), torch.where(flip, t["pv"][k], t["pv"][k1])
                        dx, dy = bu - au, bv - av
                        E = dx * (pv - av) - dy * (pu - au)
                        left = (E > 0) | ((E == 0) & ((dy < 0) | ((dy == 0) & (dx > 0))))
                        side.append(left != flip)
                        e.append(torch.where(flip, -E, E))
                    height = ((e[1] * t["ph"][0] + e[2] * t["ph"][1]) + e[0] * t["ph"][2]) / ((e[0] + e[1]) + e[2])
                    in_box = (pu >= ulo) & (pu <= uhi) & (pv >= vlo) & (pv <= vhi)
                    crossed = ~t["never"] & in_box & (side[0] == side[1]) & (side[1] == side[2]) & (height > ph)
                    cross[ii, a] = crossed.sum(dim=1, dtype=torch.int32)
        return ((cross & 1).sum(dim=1) >= 2), cross


    # ------------------------------------------------------------------ closest point (csrc/ghr_meshdist.h)
    def tris_blob(self) -> np.ndarray:
        """The host copy of the closest-point tables, bytes (built on first use; tests compare it with the host simulator's)."""
        if self._tris_blob is None:
            L = _lib.lib()
            nv, nf = len(self.vertices), len(self.faces)
            h = _lib.MeshTris()
            _lib.check(L.ghr_mesh_tris_sizes(nv, self.vertices.ctypes.data, nf, self.faces.ctypes.data, ctypes.byref(h)))
            nbytes = int(h.bytes)
            blob = torch.empty(nbytes, dtype=torch.uint8)
            _lib.check(L.ghr_mesh_tris_build(nv, self.vertices.ctypes.data, nf, self.faces.ctypes.data, blob.data_ptr(), nbytes))
            ctypes.memmove(ctypes.byref(h), blob.data_ptr(), ctypes.sizeof(h))
            self._tris_header, self._tris_blob = h, blob
        return self._tris_blob.numpy()

    def _tris_tables(self, device):
        """(the blob, the key bounds [6]) on ``device``."""
        key = str(device)
        if key not in self._tris_dev:
            self.tris_blob()
            h = self._tris_header
            bounds = torch.tensor(list(h.lo) + list(h.hi), dtype=torch.float32)
            self._tris_dev[key] = (self._tris_blob.to(device), bounds.to(device))
        return self._tris_dev[key]

    def _closest_fused(self, pts):
        if not pts.is_cuda:
            raise RuntimeError("HeadMesh.closest_point(fused=True) needs a tensor on a ROCm device: the kernels have no CPU path "
                               "(fused=False is the PyTorch form)")
        from .simple_knn import _C as _knn
        Q = pts.shape[0]
        dist2 = torch.empty(Q, dtype=torch.float32, device=pts.device)
        face = torch.empty(Q, dtype=torch.int32, device=pts.device)
        point = torch.empty((Q, 3), dtype=torch.float32, device=pts.device)
        if Q == 0:
            return dist2, face, point
        guard, _ptr, _stream = _launch_env(pts)
        with guard:
            blob, bounds = self._tris_tables(pts.device)
            srt = _knn.sort_keys(_knn.keys(pts, bounds))
            _lib.check(_lib.lib().ghr_mesh_closest(_stream(), ctypes.byref(self._tris_header), _ptr(blob), Q, _ptr(pts),
                                                   _ptr(srt.indices), _ptr(srt.values), _ptr(dist2), _ptr(face), _ptr(point)))
        return dist2, face, point

    def _closest_tables(self, device):
        """A, B, C of every face (its vertices in vertex-index order), per component, as tensors [1, F]."""
        key = str(device)
        if key not in self._tris_cmp:
            fs = np.sort(self.faces, axis=1)
            self._tris_cmp[key] = [[torch.from_numpy(np.ascontiguousarray(self.vertices[fs[:, k], c])).to(device)[None, :]
                                    for c in range(3)] for k in range(3)]
        return self._tris_cmp[key]

    def _closest_torch(self, pts, chunk_elems: int = 1 << 20):
        F = len(self.faces)
        if F == 0:
            raise ValueError("HeadMesh.closest_point: the mesh has no faces")
        A, B, C = self._closest_tables(pts.device)
        Q = pts.shape[0]
        dist2 = torch.full((Q,), float("inf"), dtype=torch.float32, device=pts.device)
        face = torch.full((Q,), -1, dtype=torch.int32, device=pts.device)
        point = pts.clone()
        idx = (pts.abs() <= torch.finfo(torch.float32).max).all(dim=1).nonzero(as_tuple=True)[0]  # (a NaN fails the comparison)
        rows = max(1, chunk_elems // F)
        ar = torch.arange(F, device=pts.device)
        for s in range(0, int(idx.numel()), rows):
            ii = idx[s:s + rows]
            q = [pts[ii, c][:, None] for c in range(3)]
            d, c = _md_face(A, B, C, q)
            mn = d.min(dim=1, keepdim=True).values
            w = torch.where(d == mn, ar[None, :], F).min(dim=1).values  # the lowest face index among equal d
            dist2[ii] = d.gather(1, w[:, None])[:, 0]
            face[ii] = w.to(torch.int32)
            point[ii] = torch.stack([c[k].expand_as(d).gather(1, w[:, None])[:, 0] for k in range(3)], dim=1)
        return dist2, face, point

    @torch.no_grad()
    def closest_point(self, points, fused: bool = True):
        """points [..., 3] -> (dist2 [...] float32: the squared distance to the mesh, face [...] int32: the face that holds the
        closest point -- the lowest index among the faces at that distance --, point [..., 3]) by the definition at the top of
        csrc/ghr_meshdist.h.  A point with a non-finite coordinate gets (+inf, -1, itself).  ``fused=False``: the PyTorch-composed
        comparator, brute force over all faces in chunks, the same float32 expressions in the same order (any device)."""
        shape = tuple(points.shape[:-1])
        assert points.shape[-1] == 3, points.shape
        pts = points.detach().reshape(-1, 3).float().contiguous()
        dist2, face, point = self._closest_fused(pts) if fused else self._closest_torch(pts)
        return dist2.reshape(shape), face.reshape(shape), point.reshape(shape + (3,))

    def signed_distance(self, points, fused: bool = True):
        """[...]: ``inside ? -sqrtf(dist2) : sqrtf(dist2)`` with ``inside`` from ``contains`` -- NEGATIVE INSIDE the mesh, positive
        outside (pysdf's SDF has the opposite sign).  +inf for a point with a non-finite coordinate.  Differentiable in the
        points (see the module-level ``signed_distance``)."""
        return signed_distance(points, self, fused=fused)

    # ------------------------------------------------------------------ public
    @torch.no_grad()
    def contains(self, points, fused: bool = True, return_crossings: bool = False):
        """bool [...] for points [..., 3]: inside the mesh.  ``return_crossings``: also the three axes' crossing counts, int32
        [..., 3].  A point with a non-finite coordinate or outside the mesh's bounding box is outside."""
        shape = tuple(points.shape[:-1])
        assert points.shape[-1] == 3, points.shape
        pts = points.detach().reshape(-1, 3).float().contiguous()
        inside, cross = self._contains_fused(pts, return_crossings) if fused else self._contains_torch(pts)
        inside = inside.reshape(shape)
        return (inside, cross.reshape(shape + (3,))) if return_crossings else inside

    @staticmethod
    def probe_points(xyz, scaling, rotation, probe: str = "reference"):
        """The twelve probes of every Gaussian, [P, 12, 3] (the composed form: the fused kernel never stores them).
        ``reference``: the points of the reference's filter script, ``v @ (diag(3 s) @ build_rotation(q)) + xyz`` -- as its
        ``build_rotation`` returns the TRANSPOSE of the rotation matrix R, these are ``R diag(3 s) v + xyz``, the points of the
        3-sigma ellipsoid (``ellipsoid`` is accepted as a second name).  ``axis_scaled``: ``diag(3 s) R^T v + xyz``, the inverse
        rotation followed by a scale along the world axes."""
        mode = PROBES[probe]
        r = rotation.float()
        # sqrtf's correctly rounded float32 root: through float64 (53 >= 2 x 24 + 2 bits: the second rounding is innocuous),
        # because torch's own float32 sqrt is not correctly rounded on every backend
        n = torch.sqrt((((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]) + r[:, 3] * r[:, 3]).double()).float()
        w, x, y, z = (r[:, i] / n for i in range(4))
        R = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
             [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
             [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
        s3 = [scaling[:, i].float() * 3 for i in range(3)]
        ico = torch.tensor(ICO_VERTS, dtype=torch.float32, device=xyz.device)
        out = torch.empty((xyz.shape[0], 12, 3), dtype=torch.float32, device=xyz.device)
        for k in range(12):
            v = ico[k]
            for j in range(3):
                if mode == _lib.PROBE_REFERENCE:
                    out[:, k, j] = ((v[0] * (s3[0] * R[j][0]) + v[1] * (s3[1] * R[j][1])) + v[2] * (s3[2] * R[j][2])) + xyz[:, j]
                else:
                    out[:, k, j] = s3[j] * ((v[0] * R[0][j] + v[1] * R[1][j]) + v[2] * R[2][j]) + xyz[:, j]
        return out

    @torch.no_grad()
    def probes_outside(self, xyz, scaling, rotation, probe: str = "reference", fused: bool = True, fused_contains=None):
        """bool [P]: all twelve probes of the Gaussian are outside the mesh.  ``scaling`` is the ACTIVATED scale, ``rotation`` the
        raw quaternion.  ``fused=False`` is the composed form: the probes built in PyTorch, ``contains`` (``fused_contains``:
        with the kernel or the comparator; default: the comparator on the CPU, the kernel on a ROCm device), ``.all(1)``."""
        if probe not in PROBES:
            raise ValueError("probe must be one of %s, got %r" % (sorted(PROBES), probe))
        xyz, scaling, rotation = (t.detach().float().contiguous() for t in (xyz, scaling, rotation))
        assert xyz.shape[1:] == (3,) and scaling.shape == xyz.shape and rotation.shape == (xyz.shape[0], 4)
        if fused:
            return self._probes_fused(xyz, scaling, rotation, PROBES[probe])
        pts = self.probe_points(xyz, scaling, rotation, probe)
        if fused_contains is None:
            fused_contains = xyz.is_cuda
        return ~self.contains(pts, fused=fused_contains).any(dim=1)


# ---- closest point: the composed candidates (the expressions of csrc/ghr_meshdist.h, operand for operand) ---------------------
def _md_sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _md_dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _md_cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _md_clamp(x, lo, hi):
    t = torch.where(x > lo, x, lo)
    return torch.where(t < hi, t, hi)


def _md_edge(P0, P1, q):
    e, w = _md_sub(P1, P0), _md_sub(q, P0)
    ee, ew = _md_dot(e, e), _md_dot(e, w)
    zero, one = torch.zeros((), dtype=ew.dtype, device=ew.device), torch.ones((), dtype=ew.dtype, device=ew.device)
    t = torch.where(ee > 0, _md_clamp(ew / ee, zero, one), zero)
    c = [torch.where(t == 1, P1[k], P0[k] + t * e[k]) for k in range(3)]
    c = [_md_clamp(c[k], torch.minimum(P0[k], P1[k]), torch.maximum(P0[k], P1[k])) for k in range(3)]
    r = _md_sub(c, q)
    return _md_dot(r, r), c


def _md_face(A, B, C, q):
    """d [Q, F] and the closest point (three [Q, F]) of every (query, face) pair; A, B, C: three [1, F] each, q: three [Q, 1]."""
    d, best = _md_edge(A, B, q)
    for P0, P1 in ((A, C), (B, C)):
        dk, p = _md_edge(P0, P1, q)
        take = dk < d
        d = torch.where(take, dk, d)
        best = [torch.where(take, p[k], best[k]) for k in range(3)]
    ab, ac = _md_sub(B, A), _md_sub(C, A)
    n = _md_cross(ab, ac)
    nn = _md_dot(n, n)
    s0 = _md_dot(_md_cross(_md_sub(C, B), _md_sub(q, B)), n)
    s1 = _md_dot(_md_cross(_md_sub(A, C), _md_sub(q, C)), n)
    s2 = _md_dot(_md_cross(ab, _md_sub(q, A)), n)
    accepted = (nn > 0) & (s0 >= 0) & (s1 >= 0) & (s2 >= 0)
    k = torch.where(nn > 0, _md_dot(n, _md_sub(q, A)) / nn, torch.zeros((), dtype=nn.dtype, device=nn.device))
    p = [q[i] - k * n[i] for i in range(3)]
    p = [_md_clamp(p[i], torch.minimum(torch.minimum(A[i], B[i]), C[i]), torch.maximum(torch.maximum(A[i], B[i]), C[i]))
         for i in range(3)]
    r = _md_sub(p, q)
    dk = _md_dot(r, r)
    take = accepted & (dk < d)
    d = torch.where(take, dk, d)
    best = [torch.where(take, p[i], best[i]) for i in range(3)]
    return d, best


def _sqrt32(d):
    """sqrtf's correctly rounded float32 root (through float64, as ``probe_points``)."""
    return torch.sqrt(d.double()).float()


class _SignedDistance(torch.autograd.Function):
    """points [Q, 3] -> sd [Q].  Backward: ``t = g sign``, ``t ((q - c) / sqrtf(d))`` per component, 0 where ``d == 0`` or the point
    was not finite -- the closest point and the sign are constants of the step (the gradient of a distance field), one thread per
    point in HIP (``fused``) or the same expressions composed."""

    @staticmethod
    def forward(ctx, pts, mesh, fused):
        dist2, _, closest = mesh.closest_point(pts, fused=fused)
        inside = mesh.contains(pts, fused=fused)
        root = _sqrt32(dist2)
        ctx.save_for_backward(pts, closest, dist2, inside)
        ctx.fused = fused
        return torch.where(inside, -root, root)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        pts, closest, dist2, inside = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        if ctx.fused:
            Q = pts.shape[0]
            d_pts = torch.empty_like(pts)
            if Q:
                guard, _ptr, _stream = _launch_env(pts)
                in8 = inside.to(torch.uint8)
                with guard:
                    _lib.check(_lib.lib().ghr_mesh_distance_backward(_stream(), Q, _ptr(pts), _ptr(closest), _ptr(dist2), _ptr(in8),
                                                                     _ptr(g), _ptr(d_pts)))
            return d_pts, None, None
        fmax = torch.finfo(torch.float32).max
        live = (dist2 > 0) & (dist2 <= fmax) & (pts.abs() <= fmax).all(dim=1)
        t = g * torch.where(inside, -torch.ones_like(g), torch.ones_like(g))
        root = torch.where(live, _sqrt32(dist2), torch.ones_like(dist2))
        d_pts = t[:, None] * ((pts - closest) / root[:, None])
        return torch.where(live[:, None], d_pts, torch.zeros_like(d_pts)), None, None


def signed_distance(points, mesh: HeadMesh, fused: bool = True):
    """[...] for points [..., 3]: the signed distance to ``mesh``, ``inside ? -sqrtf(d) : sqrtf(d)`` with ``d`` from
    ``mesh.closest_point`` and ``inside`` from ``mesh.contains`` -- NEGATIVE INSIDE (pysdf's ``SDF`` is positive inside: the
    opposite sign).  Differentiable in ``points`` only: the gradient is ``sign (q - c) / sqrtf(d)``, the unit vector from the
    closest point ``c``, 0 where ``d == 0`` or the point is not finite.  ``fused=True`` needs a ROCm tensor (HIP forward and
    backward); ``fused=False`` is the PyTorch-composed comparator on any device."""
    assert points.shape[-1] == 3, points.shape
    if fused and not points.is_cuda:
        raise RuntimeError("signed_distance(fused=True) needs a tensor on a ROCm device: the kernels have no CPU path "
                           "(fused=False is the PyTorch form)")
    shape = tuple(points.shape[:-1])
    pts = points.reshape(-1, 3).float().contiguous()
    return _SignedDistance.apply(pts, mesh, bool(fused)).reshape(shape)
