"""chamfer_distance, knn_points and strand_geometry (gaussianhaircut_amd/utils/loss_chamfer_utils.py, nearest.py, evaluation.py;
DESIGN.md 8j) without a GPU.

 1. tests/golden/reference_chamfer_golden.npz is the REFERENCE'S OWN chamfer_distance in float64 (make_reference_chamfer_golden.py)
    for thirteen argument combinations.  The composed form (fused=False) on CPU tensors:
      in float64  every returned value and every gradient (x, y, both normals) within 256 * 2^-53 of the tensor's largest
                  magnitude: the two are the same formulas in another order, a sum of at most 227 terms per element;
      in float32  indices exact (equal per-point values imply them; they are also compared through the weights), every per-point
                  distance within 6 * 2^-24 relative (dx: 1 rounding, squared: 2 + 1, two additions: 2 -- the golden's inputs are
                  the same float32 values), every normals term within 16 * 2^-24 absolute per unit of weight (dot and both norms
                  of three terms each, cos <= 1), and a reduced value within (16 + 2 (P + N)) * 2^-24 * R, R the same reduction of
                  the terms' magnitudes (distances, weights and 1 - |cos| are non-negative, so R is the value itself; for the
                  normals term R is the reduction of the weights alone): a sum of n terms adds at most n * 2^-24 * sum |term|,
                  and the divisor of the weighted mean is such a sum again.
    The weights returned are the caller's tensors, multiplied in place; the error texts match.
 2. the comparator on the tie cases (and every other cloud kind, small shapes) against the stated rule by a numpy loop.
 3. the C ABI: the four symbols declared, exported and bound; ghr_nn.h listed; ABI 20; every refusal answered before a device is
    touched.
 4. strand_geometry on a hand-made pair whose precision and recall are known fractions."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from gaussianhaircut_amd import _lib, evaluation, nearest
from gaussianhaircut_amd.utils.loss_chamfer_utils import chamfer_distance
from tests import chamfer_cases as cc
from tests import helpers as hp

U24, U53 = 2.0 ** -24, 2.0 ** -53
NAMES = ("ghr_nn_workspace_size", "ghr_nn_search", "ghr_chamfer_point", "ghr_chamfer_point_backward")


@pytest.fixture(scope="module")
def golden():
    return cc.load_golden()


def _inputs(golden):
    return {k[3:]: torch.from_numpy(v) for k, v in golden.items() if k.startswith("in/")}


def _run(name, golden, dtype):
    uses, extra = cc.GOLDEN_CASES[name]
    kw = cc.golden_kwargs(uses, _inputs(golden), dtype)
    res = chamfer_distance(**kw, **extra, fused=False)
    return kw, res


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
def test_golden_inputs_are_the_recipe(golden):
    for k, v in cc.golden_inputs().items():
        assert np.array_equal(golden["in/" + k], v.numpy()), k


@pytest.mark.parametrize("name", sorted(cc.GOLDEN_CASES))
def test_composed_form_in_float64_equals_the_reference_golden(name, golden):
    kw, res = _run(name, golden, torch.float64)
    cc.scalar_of(res).backward()
    seen = 0
    for term, pair in zip(("dist", "normals", "features", "weights"), res):
        for side, v in zip("xy", pair):
            key = "%s/%s_%s" % (name, term, side)
            assert (v is None) == (key not in golden), key
            if v is not None:
                want = golden[key]
                # (the tensor of ones made for x_weights when only y_weights is given is float32 whatever the inputs are)
                assert v.shape == want.shape and (v.dtype == torch.float64 or key == "y_weights_only/weights_x"), key
                err = float(np.abs(v.detach().double().numpy() - want).max())
                assert err <= 256 * U53 * max(float(np.abs(want).max()), 1e-300), (key, err)
                seen += 1
    for k in ("x", "y", "x_normals", "y_normals"):
        key = "%s/d_%s" % (name, k)
        assert (k in kw and kw[k].grad is not None) == (key in golden), key
        if key in golden:
            err = float(np.abs(kw[k].grad.numpy() - golden[key]).max())
            assert err <= 256 * U53 * float(np.abs(golden[key]).max()), (key, err)
            seen += 1
    assert seen >= 3


@pytest.mark.parametrize("name", sorted(cc.GOLDEN_CASES))
def test_composed_form_in_float32_is_within_the_derived_bounds_of_the_golden(name, golden):
    uses, extra = cc.GOLDEN_CASES[name]
    kw, res = _run(name, golden, torch.float32)
    pr, br = extra.get("point_reduction", "mean"), extra.get("batch_reduction", "mean")
    N = cc.GOLDEN_N
    for side, P, li in (("x", cc.GOLDEN_P1, 0), ("y", cc.GOLDEN_P2, 1)):
        if "%s/dist_%s" % (name, side) not in golden:
            continue
        lengths = np.array(cc.GOLDEN_LENGTHS[li] if "l" in uses else (P,) * N, dtype=np.float64)
        wkey = "%s/weights_%s" % (name, side)
        w = golden[wkey] if wkey in golden else None
        if w is not None:   # products of float32 values taken at the same indices: one rounding for x's, and y's multiplies
            got_w = res[3]["xy".index(side)].numpy().astype(np.float64)   # by x's rounded products: two; 3 covers the u^2 term
            assert np.all(np.abs(got_w - w) <= 3 * U24 * np.abs(w)), wkey
        unit = np.ones((N, P)) if w is None else w.copy()
        unit = unit * (np.arange(P)[None, :] < lengths[:, None])
        K = (16 + 2 * (P + N)) if pr is not None else 16
        for term, absolute in (("dist", False), ("normals", True)):
            key = "%s/%s_%s" % (name, term, side)
            if key not in golden:
                continue
            want = golden[key]
            got = res[("dist", "normals").index(term)]["xy".index(side)].detach().numpy().astype(np.float64)
            if pr is None:
                scale = unit if absolute else np.abs(want)
            else:
                scale = cc.reduce64(unit, w, lengths, pr, br) if absolute else np.abs(want)
            err = np.abs(got - want)
            print(key, "max err / bound:", float((err / np.maximum(K * U24 * scale, 1e-300)).max()))
            assert np.all(err <= K * U24 * scale), key


def test_indices_equal_the_golden_through_the_per_point_values(golden):
    """per_point returns the unreduced distances: float32 equals float64 within 6 ulps only if every index is the golden's (the
    two nearest candidates are at least 1e-5 apart, relative); the gathered weights of 'weights' say the same."""
    _, res = _run("per_point", golden, torch.float32)
    for side, v in zip("xy", res[0]):
        want = golden["per_point/dist_" + side]
        assert np.all(np.abs(v.detach().numpy().astype(np.float64) - want) <= 6 * U24 * np.abs(want))
    inp = _inputs(golden)
    nn = nearest.knn_points(inp["x"], inp["y"], fused=False)
    assert nn.idx.dtype == torch.int64 and nn.idx.shape == (cc.GOLDEN_N, cc.GOLDEN_P1, 1) and nn.knn is None
    w = golden["weights/weights_x"] / inp["x_weights"].double().numpy()          # = y_weights[idx], to rounding
    gathered = nearest.knn_gather(inp["y_weights"][:, :, None], nn.idx)[:, :, 0, 0].double().numpy()
    assert np.all(np.abs(w - gathered) <= 4 * U53 * np.abs(w))


def test_weights_are_multiplied_in_place_and_returned(golden):
    kw, res = _run("weights", golden, torch.float32)
    assert res[3][0] is kw["x_weights"] and res[3][1] is kw["y_weights"]
    inp = _inputs(golden)
    assert not torch.equal(kw["x_weights"], inp["x_weights"]) and not torch.equal(kw["y_weights"], inp["y_weights"])
    kw, res = _run("y_weights_only", golden, torch.float32)
    assert res[3][1] is kw["y_weights"] and torch.equal(kw["y_weights"], inp["y_weights"])   # nothing to multiply it by
    assert res[3][0].shape == (cc.GOLDEN_N, cc.GOLDEN_P1) and res[3][0].dtype == torch.float32


def test_error_texts(golden):
    inp = _inputs(golden)
    for name, (uses, extra) in cc.GOLDEN_ERRORS.items():
        kind, text = golden[name + "/error"]
        with pytest.raises(ValueError if kind == "ValueError" else TypeError) as e:
            chamfer_distance(**cc.golden_kwargs(uses, inp, torch.float32), **extra, fused=False)
        assert str(e.value) == text, name
    x, y = inp["x"], inp["y"]
    for kw, text in ((dict(batch_reduction="max"), 'batch_reduction must be one of ["mean", "sum"] or None'),
                     (dict(point_reduction="max"), 'point_reduction must be one of ["mean", "sum"] or None'),
                     (dict(point_reduction=None), "Batch reduction must be None if point_reduction is None"),
                     (dict(norm=3), "Support for 1 or 2 norm."),
                     (dict(x_lengths=torch.tensor([1])), "Expected lengths to be of shape (N,)"),
                     (dict(x_lengths=torch.tensor([1, 98])), "A length value was too long"),
                     (dict(x_normals=torch.zeros(3), y_normals=inp["y_normals"]), "Expected normals to be of shape (N, P, 3"),
                     (dict(x_weights=torch.ones(2, 3)), "x_weights must be of shape (N, P1)."),
                     (dict(y_weights=torch.ones(2, 3)), "y_weights must be of shape (N, P2)."),
                     (dict(x_weights=-torch.ones(2, 97)), "x_weights cannot be negative."),
                     (dict(y_weights=-torch.ones(2, 130)), "y_weights cannot be negative.")):
        with pytest.raises(ValueError) as e:
            chamfer_distance(x, y, **kw, fused=False)
        assert str(e.value) == text
    for bad, text in ((x[0], "Expected points to be of shape (N, P, D)"),
                      ([1.0], "The input pointclouds should be either Pointclouds objects or torch.Tensor of shape "
                              "(minibatch, num_points, 3).")):
        with pytest.raises(ValueError) as e:
            chamfer_distance(bad, y, fused=False)
        assert str(e.value) == text
    with pytest.raises(ValueError) as e:
        chamfer_distance(x, y[:, :, :2], fused=False)
    assert str(e.value) == "y does not have the correct shape."
    Pointclouds = type("Pointclouds", (), {})
    with pytest.raises(TypeError, match="pytorch3d is not a dependency"):
        chamfer_distance(Pointclouds(), y)
    with pytest.raises(NotImplementedError, match="K == 1"):
        nearest.knn_points(x, y, K=2)
    with pytest.raises(ValueError, match="fused=True"):
        nearest.knn_points(x, y, fused=True)      # CPU tensors: HIP does not apply
    with pytest.raises(ValueError, match="fused=True"):
        chamfer_distance(x, y, fused=True)


def test_reference_import_line_resolves_with_the_package_on_the_path():
    import importlib
    import sys
    pkg = os.path.join(hp.ROOT, "gaussianhaircut_amd")
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "utils" or k.startswith("utils.")}
    sys.path.insert(0, pkg)
    try:
        mod = importlib.import_module("utils.loss_chamfer_utils")
        assert callable(mod.chamfer_distance)
    finally:
        sys.path.remove(pkg)
        for k in [k for k in sys.modules if k == "utils" or k.startswith("utils.")]:
            del sys.modules[k]
        sys.modules.update(saved)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cc.KINDS)
def test_comparator_follows_the_stated_rule_on_the_small_shapes(kind):
    ties = 0
    for Px, Py in cc.SMALL_SHAPES:
        c = cc.cloud(kind, Px, Py)
        for norm in (1, 2):
            d, i = nearest.nearest_composed(c["x"], c["y"], norm)
            wd, wi = cc.brute_rule(c["x"], c["y"], norm)
            assert np.array_equal(i.numpy(), wi), (kind, Px, Py, norm)
            assert np.array_equal(d.numpy().view(np.int32), wd.view(np.int32)), (kind, Px, Py, norm)
        if c["idx"] is not None:
            assert torch.equal(i, c["idx"]) and float(d.abs().max()) == 0.0
        if kind == "lattice" and Py >= 63:
            full = nearest._pair_dist(c["y"][None] - c["x"][:, None], 2)
            ties += int(((full == full.min(-1, keepdim=True).values).sum(-1) > 1).sum())
    if kind == "lattice":
        assert ties > 100      # the case does what it is for: exact ties, decided by the index


def test_lengths_padding_any_dimension_and_dtype():
    g = torch.Generator().manual_seed(5)
    p1, p2 = torch.rand(2, 9, 4, generator=g, dtype=torch.float64), torch.rand(2, 7, 4, generator=g, dtype=torch.float64)
    l1, l2 = torch.tensor([9, 4]), torch.tensor([3, 7])
    nn = nearest.knn_points(p1, p2, l1, l2, norm=1)
    assert nn.dists.dtype == torch.float64 and nn.dists.shape == (2, 9, 1)
    assert float(nn.dists[1, 4:].abs().max()) == 0.0 and int(nn.idx[1, 4:].max()) == 0 and int(nn.idx[0].max()) < 3
    want = (p2[0, None, :3] - p1[0, :, None]).abs().sum(-1).min(-1).values
    assert torch.allclose(nn.dists[0, :, 0], want, rtol=1e-15, atol=0)
    out = nearest.knn_gather(p2, nn.idx, l2)
    assert out.shape == (2, 9, 1, 4) and torch.equal(out[0, :, 0], p2[0][nn.idx[0, :, 0]])
    empty = nearest.knn_points(p1, p2, l1, torch.tensor([0, 7]))
    assert float(empty.dists[0].abs().max()) == 0.0 and int(empty.idx[0].max()) == 0


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
def test_c_abi_symbols_are_declared_and_exported():
    L = _lib.lib()
    with open(os.path.join(hp.ROOT, "include", "ghr.h")) as fh:
        hdr = fh.read()
    with open(os.path.join(_lib.CSRC, "ghr_capi.hip")) as fh:
        capi = fh.read()
    new = set(re.findall(r"\bint (ghr_(?:nn|chamfer)_\w+)\(", hdr))
    assert new == set(NAMES)
    assert set(re.findall(r"^int (ghr_(?:nn|chamfer)_\w+)\(", capi, re.M)) - {"ghr_nn_read_counters"} == new   # (a -D build's own)
    for n in NAMES:
        assert n in _lib.EXPORTS and hasattr(L, n) and getattr(L, n).argtypes, n
    assert not hasattr(L, "ghr_nn_read_counters")          # the counter lives in measurement builds only
    assert L.ghr_abi_version() == 20 == _lib.ABI_VERSION and "#define GHR_ABI_VERSION 20" in hdr
    assert "ghr_nn.h" in _lib.HEADERS and os.path.exists(os.path.join(_lib.CSRC, "ghr_nn.h"))


def test_c_abi_refusals_launch_nothing():
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused before anything is enqueued
    INV, BIG = _lib.GHR_E_INVALID, 2 ** 31

    def size(Px=5, Py=7, out=True):
        b = ctypes.c_size_t(0)
        return L.ghr_nn_workspace_size(Px, Py, ctypes.byref(b) if out else None)

    def search(Px=5, Py=7, norm=2, **kw):
        names = ("x", "order_x", "keys_x", "y", "order_y", "keys_y", "ws", "dist", "idx")
        a = dict(dict.fromkeys(names, fake), **kw)
        return L.ghr_nn_search(None, Px, a["x"], a["order_x"], a["keys_x"], Py, a["y"], a["order_y"], a["keys_y"], norm, a["ws"],
                               a["dist"], a["idx"])

    def point(Px=5, Py=7, **kw):
        names = ("idx", "xn", "yn", "yw", "term", "weight")
        a = dict(dict.fromkeys(names, fake), **kw)
        return L.ghr_chamfer_point(None, Px, Py, a["idx"], a["xn"], a["yn"], 1, a["yw"], a["term"], a["weight"])

    def back(Px=5, Py=7, norm=2, **kw):
        names = ("x", "y", "idx", "start", "members", "g_dist", "xn", "yn", "g_cos", "d_x", "d_y", "d_xn", "d_yn")
        a = dict(dict.fromkeys(names, fake), **kw)
        return L.ghr_chamfer_point_backward(None, Px, Py, norm, a["x"], a["y"], a["idx"], a["start"], a["members"], a["g_dist"],
                                            a["xn"], a["yn"], 1, a["g_cos"], a["d_x"], a["d_y"], a["d_xn"], a["d_yn"])

    sizes = [(dict(Px=BIG), b"Px must be in [0, 2^31)"), (dict(Px=-1), b"Px must be"), (dict(Py=BIG), b"Py must be in [0, 2^31)"),
             (dict(Py=-1), b"Py must be"), (dict(Py=0), b"Py == 0")]
    table = ((size, sizes + [(dict(out=False), b"bytes is NULL")]),
             (search, sizes + [(dict(norm=0), b"norm must be 1 or 2"), (dict(norm=3), b"norm must be 1 or 2")] +
              [({k: None}, b"NULL") for k in ("x", "order_x", "keys_x", "y", "order_y", "keys_y", "ws", "dist", "idx")]),
             (point, sizes + [(dict(idx=None), b"idx is NULL"), (dict(xn=None), b"all three or none"), (dict(term=None), b"all three or none"),
                              (dict(yw=None), b"both or neither"), (dict(xn=None, yn=None, term=None, yw=None, weight=None), b"nothing to compute")]),
             (back, sizes + [(dict(norm=4), b"norm must be 1 or 2"), (dict(idx=None), b"NULL"), (dict(start=None), b"NULL"),
                             (dict(members=None), b"NULL"), (dict(g_dist=None, g_cos=None), b"nothing to compute"),
                             (dict(x=None), b"g_dist needs"), (dict(d_y=None), b"g_dist needs"), (dict(g_dist=None), b"without g_dist"),
                             (dict(yn=None), b"g_cos needs"), (dict(d_xn=None), b"g_cos needs"), (dict(g_cos=None), b"without g_cos")]))
    for fn, cases in table:
        for kw, words in cases:
            assert fn(**kw) == INV, (fn.__name__, kw)
            msg = L.ghr_last_error()
            assert words in msg and msg.startswith(b"ghr_"), (fn.__name__, kw, msg)
    assert size() == _lib.GHR_OK and search(Px=0) == _lib.GHR_OK and point(Px=0) == _lib.GHR_OK   # empty: nothing to do
    assert _lib.nn_workspace_size(0, 1) > 0 and _lib.nn_workspace_size(2 ** 31 - 1, 2 ** 31 - 1) > 2 * 16 * (2 ** 31 - 1)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
def test_strand_geometry_on_a_hand_made_pair():
    """Four predicted strands of one segment along x, midpoints at (0.5, k, 0); four ground-truth strands: the first two the same
    segments moved by 0.1 in z, the third moved by 0.1 and turned by 45 degrees in the plane, the fourth 5 away.  Within 0.2 and
    30 degrees: predictions 0 and 1 (precision 2 / 4); ground truth 0 and 1 (recall 2 / 4).  Within 0.2 and 60 degrees the third
    pair joins (3 / 4 both).  Within 10: prediction 3 at (0.5, 3, 0) finds ground truth 2 at distance sqrt(1.01), turned by 45,
    and ground truth 3 (at y = 8) finds prediction 3 at distance 5, parallel -- so 30 degrees give precision 2 / 4 and recall
    3 / 4, and 60 degrees 4 / 4 both."""
    def seg(mid, ang):
        d = 0.5 * torch.tensor([np.cos(np.deg2rad(ang)), np.sin(np.deg2rad(ang)), 0.0], dtype=torch.float32)
        m = torch.tensor(mid, dtype=torch.float32)
        return torch.stack((m - d, m + d))

    pred = torch.stack([seg((0.5, float(k), 0.0), 0.0) for k in range(4)])
    gt = torch.stack([seg((0.5, 0.0, 0.1), 0.0), seg((0.5, 1.0, 0.1), 180.0), seg((0.5, 2.0, 0.1), 45.0), seg((0.5, 8.0, 0.0), 0.0)])
    r = evaluation.strand_geometry(pred, gt, [0.2, 10.0], [30.0, 60.0], fused=False)
    assert r["thresholds"] == [(0.2, 30.0), (0.2, 60.0), (10.0, 30.0), (10.0, 60.0)]
    assert r["precision"] == [0.5, 0.75, 0.5, 1.0] and r["recall"] == [0.5, 0.75, 0.75, 1.0]
    assert r["fscore"][0] == 0.5 and r["fscore"][1] == 0.75 and r["fscore"][3] == 1.0
    assert abs(r["fscore"][2] - 2 * 0.5 * 0.75 / 1.25) < 1e-15
    assert abs(r["chamfer_pred_to_gt"] - (3 * 0.01 + 1.01) / 4) < 1e-6 and abs(r["chamfer_gt_to_pred"] - (3 * 0.01 + 25.0) / 4) < 1e-5
    assert abs(r["direction_pred_to_gt"] - 2 * (1 - np.cos(np.pi / 4)) / 4) < 1e-6
    assert abs(r["direction_gt_to_pred"] - (1 - np.cos(np.pi / 4)) / 4) < 1e-6
    with pytest.raises(ValueError, match="L >= 2"):
        evaluation.strand_geometry(pred[:, :1], gt, [0.1], [10.0], fused=False)
