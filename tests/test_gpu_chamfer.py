"""The cross-cloud nearest-neighbour search, the chamfer point terms and their backward (csrc/ghr_nn.h, gaussianhaircut_amd/
nearest.py, utils/loss_chamfer_utils.py, evaluation.strand_geometry) on the MI355X against the PyTorch-composed
comparator on the same device, for every cloud kind and every (Px, Py) of tests/chamfer_cases.py -- no case is left out.

u = 2^-24.  Per case:
  dist          bit for bit (the same fp32 expression, no contraction), norm 1 and norm 2;
  idx           exactly equal (the comparator takes the lowest index explicitly); 'duplicates' also against its known answer;
  d_x           bit for bit (elementwise);
  cosine term   within 24 u absolute: in either form cos carries at most ~12 roundings (a dot and two squared norms of three terms,
                two square roots, a product and a quotient or two quotients), each relative to a quantity that is at most 1 after
                the division, and 1 - |cos| adds one;
  d_x_normals   within 64 u |g| / |a| per element: the gradient is (g / |a|) (b^ - cos a^), both terms at most 1 in magnitude and
                each within 16 roundings in either form, so 32 u absolute per form before the scale;
  d_y           against the SAME fp32 products summed in float64, within (n_j - 1) u sum |product|, n_j the list length;
  d_y_normals   against the float64 evaluation of the formula, within sum_i 64 u |g_i| / |b| (the products, as for d_x_normals)
                plus (n_j - 1) u sum |product|;
  lists         their lengths sum to Px, every member's idx is the list's owner, members ascend within a list;
  schedule      permuting x permutes dist, idx, d_x and the cosine term with equal bits; permuting y leaves dist's bits, maps idx
                through the permutation on the tie-free kinds and equals the comparator on the permuted cloud (the lowest index in
                the NEW numbering, i.e. of the caller's original order) on the tie kinds;
  twice         two runs of forward and backward give equal bits everywhere.
Then: lengths shorter than the padded size; chamfer_distance(fused=True) against fused=False for the golden's argument
combinations; strand_geometry fused against composed with equal counts."""
import numpy as np
import pytest
import torch

from gaussianhaircut_amd import evaluation, nearest
from gaussianhaircut_amd.utils.loss_chamfer_utils import chamfer_distance
from tests import chamfer_cases as cc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24


def _bits(a, b, what):
    assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape, what
    bad = a.view(torch.int32) != b.view(torch.int32)
    assert not bool(bad.any()), (what, int(bad.sum()), a[bad][:4].tolist(), b[bad][:4].tolist())


def _hip(x, y, xn, yn, g_d, g_c, norm=2, abs_cosine=True):
    """forward and backward of the HIP form -> dict of detached tensors"""
    x, y, xn, yn = (t.detach().clone().requires_grad_(True) for t in (x, y, xn, yn))
    d, i = nearest._NearestHip.apply(x, y, norm)
    term = nearest._CosineHip.apply(xn, yn, i.to(torch.int32), abs_cosine)
    torch.autograd.backward((d, term), (g_d, g_c))
    return dict(dist=d.detach(), idx=i, term=term.detach(), d_x=x.grad, d_y=y.grad, d_xn=xn.grad, d_yn=yn.grad)


def _composed(x, y, xn, yn, g_d, g_c, norm=2, abs_cosine=True):
    x, y, xn, yn = (t.detach().clone().requires_grad_(True) for t in (x, y, xn, yn))
    d, i = nearest.nearest_composed(x, y, norm)
    term = nearest.cosine_term_composed(xn, yn[i], abs_cosine)
    torch.autograd.backward((d, term), (g_d, g_c))
    return dict(dist=d.detach(), idx=i, term=term.detach(), d_x=x.grad, d_y=y.grad, d_xn=xn.grad, d_yn=yn.grad)


def _cos_grad64(a, b, g, abs_cosine=True):
    """float64: gradient of g (1 - |cos|) w.r.t. a and b, per pair"""
    a, b, g = a.double(), b.double(), g.double()
    na, nb = a.norm(dim=1, keepdim=True), b.norm(dim=1, keepdim=True)
    c = (a * b).sum(1, keepdim=True) / (na * nb)
    gc = -(torch.sign(c) if abs_cosine else 1.0) * g[:, None]
    return gc * (b / (na * nb) - c * a / (na * na)), gc * (a / (na * nb) - c * b / (nb * nb))


@pytest.mark.parametrize("Px,Py", cc.SHAPES, ids=["%dx%d" % s for s in cc.SHAPES])
@pytest.mark.parametrize("kind", cc.KINDS)
def test_hip_equals_the_comparator(kind, Px, Py):
    c = cc.cloud(kind, Px, Py)
    x, y = c["x"].to(DEV), c["y"].to(DEV)
    xn, yn = cc.normals_for(Px, 1).to(DEV), cc.normals_for(Py, 2).to(DEV)
    g = torch.Generator().manual_seed(Px * 3 + Py)
    g_d, g_c = torch.randn(Px, generator=g).to(DEV), torch.randn(Px, generator=g).to(DEV)

    # norm 1: the search alone
    d1, i1 = nearest.search_hip(x, y, 1)
    r1, j1 = nearest.nearest_composed(x, y, 1)
    assert torch.equal(i1.long(), j1), (kind, Px, Py, "idx, norm 1", int((i1.long() != j1).sum()))
    _bits(d1, r1, "dist, norm 1")

    h, r = _hip(x, y, xn, yn, g_d, g_c), _composed(x, y, xn, yn, g_d, g_c)
    idx = h["idx"]
    assert idx.dtype == torch.int64 and int(idx.min()) >= 0 and int(idx.max()) < Py
    assert torch.equal(idx, r["idx"]), (kind, Px, Py, "idx", int((idx != r["idx"]).sum()))
    if c["idx"] is not None:
        assert torch.equal(idx.cpu(), c["idx"]) and float(h["dist"].abs().max()) == 0.0
    _bits(h["dist"], r["dist"], "dist")
    _bits(h["d_x"], r["d_x"], "d_x")
    err = float((h["term"] - r["term"]).abs().max())
    assert err <= 24 * U, ("cosine term", err / U)
    na, nb = xn.norm(dim=1, keepdim=True), yn.norm(dim=1, keepdim=True)
    bound_xn = 64 * U * g_c.abs()[:, None] / na
    assert bool(((h["d_xn"] - r["d_xn"]).abs() <= bound_xn).all()), "d_x_normals"

    # the lists
    start, members = nearest.inverted_lists(idx.to(torch.int32), Py)
    counts = start[1:] - start[:-1]
    assert int(start[0]) == 0 and int(start[-1]) == Px and int(counts.sum()) == Px and bool((counts >= 0).all())
    owner = torch.repeat_interleave(torch.arange(Py, device=DEV), counts)
    assert torch.equal(idx[members], owner)
    same = owner[1:] == owner[:-1]
    assert bool((members[1:][same] > members[:-1][same]).all())

    # d_y: the same fp32 products, summed in float64
    diff = y[idx] - x
    t = g_d[:, None] * diff
    p = (t + t).double()
    want = torch.zeros(Py, 3, dtype=torch.float64, device=DEV).index_add_(0, idx, p)
    mag = torch.zeros(Py, 3, dtype=torch.float64, device=DEV).index_add_(0, idx, p.abs())
    n1 = (counts - 1).clamp(min=0).double()[:, None]
    assert bool(((h["d_y"].double() - want).abs() <= n1 * U * mag).all()), "d_y"
    assert float(h["d_y"][counts == 0].abs().max() if bool((counts == 0).any()) else 0.0) == 0.0
    # d_y_normals
    _, db = _cos_grad64(xn, yn[idx], g_c)
    want = torch.zeros(Py, 3, dtype=torch.float64, device=DEV).index_add_(0, idx, db)
    mag = torch.zeros(Py, 3, dtype=torch.float64, device=DEV).index_add_(0, idx, db.abs())
    each = torch.zeros(Py, 1, dtype=torch.float64, device=DEV).index_add_(0, idx, (64 * U * g_c.abs()[:, None] / nb[idx]).double())
    assert bool(((h["d_yn"].double() - want).abs() <= each + n1 * U * mag).all()), "d_y_normals"

    # twice
    h2 = _hip(x, y, xn, yn, g_d, g_c)
    for k in ("dist", "term", "d_x", "d_y", "d_xn", "d_yn"):
        _bits(h[k], h2[k], "second run: " + k)
    assert torch.equal(h2["idx"], idx)

    # permuted x
    px = torch.randperm(Px, generator=g).to(DEV)
    hp = _hip(x[px].contiguous(), y, xn[px].contiguous(), yn, g_d[px], g_c[px])
    assert torch.equal(hp["idx"], idx[px])
    for k in ("dist", "term", "d_x", "d_xn"):
        _bits(hp[k], h[k][px], "permuted x: " + k)
    # permuted y
    py = torch.randperm(Py, generator=g).to(DEV)
    yp = y[py].contiguous()
    dp, ip = nearest.search_hip(x, yp, 2)
    _bits(dp, h["dist"], "permuted y: dist")
    if kind in cc.TIE_KINDS:
        assert torch.equal(ip.long(), nearest.nearest_composed(x, yp, 2)[1])
    else:
        assert torch.equal(py[ip.long()], idx)


def test_signed_cosine_and_l1_backward():
    c = cc.cloud("uniform", 4097, 65)
    x, y = c["x"].to(DEV), c["y"].to(DEV)
    xn, yn = cc.normals_for(4097, 3).to(DEV), cc.normals_for(65, 4).to(DEV)
    g = torch.Generator().manual_seed(9)
    g_d, g_c = torch.randn(4097, generator=g).to(DEV), torch.randn(4097, generator=g).to(DEV)
    h, r = _hip(x, y, xn, yn, g_d, g_c, 1, False), _composed(x, y, xn, yn, g_d, g_c, 1, False)
    assert torch.equal(h["idx"], r["idx"])
    _bits(h["dist"], r["dist"], "dist")
    _bits(h["d_x"], r["d_x"], "d_x, norm 1")
    assert float((h["term"] - r["term"]).abs().max()) <= 24 * U
    idx = h["idx"]
    p = (g_d[:, None] * torch.sign(y[idx] - x)).double()                 # +-g or 0: sums of these in float64 are exact here
    want = torch.zeros(65, 3, dtype=torch.float64, device=DEV).index_add_(0, idx, p)
    mag = torch.zeros(65, 3, dtype=torch.float64, device=DEV).index_add_(0, idx, p.abs())
    n1 = (torch.bincount(idx, minlength=65) - 1).clamp(min=0).double()[:, None]
    assert bool(((h["d_y"].double() - want).abs() <= n1 * U * mag).all())
    da, db = _cos_grad64(xn, yn[idx], g_c, False)
    assert bool(((h["d_xn"].double() - da).abs() <= 64 * U * g_c.abs()[:, None] / xn.norm(dim=1, keepdim=True)).all())
    want = torch.zeros(65, 3, dtype=torch.float64, device=DEV).index_add_(0, idx, db)
    mag = torch.zeros(65, 3, dtype=torch.float64, device=DEV).index_add_(0, idx, db.abs())
    each = torch.zeros(65, 1, dtype=torch.float64, device=DEV).index_add_(0, idx, (64 * U * g_c.abs()[:, None] / yn.norm(dim=1, keepdim=True)[idx]).double())
    assert bool(((h["d_yn"].double() - want).abs() <= each + n1 * U * mag).all())


def test_lengths_shorter_than_the_padded_size():
    g = torch.Generator().manual_seed(11)
    p1, p2 = torch.rand(3, 200, 3, generator=g).to(DEV), torch.rand(3, 150, 3, generator=g).to(DEV)
    l1, l2 = torch.tensor([200, 65, 1], device=DEV), torch.tensor([64, 150, 0], device=DEV)
    for norm in (1, 2):
        a = nearest.knn_points(p1.clone().requires_grad_(True), p2, l1, l2, norm=norm, fused=True)
        b = nearest.knn_points(p1, p2, l1, l2, norm=norm, fused=False)
        assert a.dists.shape == (3, 200, 1) and a.idx.dtype == torch.int64 and a.knn is None
        assert torch.equal(a.idx, b.idx)
        _bits(a.dists.detach(), b.dists, "dists")
        assert float(a.dists.detach()[1, 65:].abs().max()) == 0.0 and int(a.idx[1, 65:].max()) == 0 and int(a.idx[0].max()) < 64
        assert float(a.dists.detach()[2].abs().max()) == 0.0 and int(a.idx[2].max()) == 0          # an empty second cloud
    with pytest.raises(ValueError, match="fused=True"):
        nearest.knn_points(p1.double(), p2.double(), fused=True)
    with pytest.raises(ValueError, match="fused=True"):
        nearest.knn_points(p1[:, :, :2], p2[:, :, :2], fused=True)
    assert nearest.knn_points(p1.double(), p2.double()).dists.dtype == torch.float64      # fused=None: the comparator


@pytest.mark.parametrize("name", sorted(cc.GOLDEN_CASES))
def test_chamfer_distance_fused_equals_composed(name):
    """Distances are the same bits, so their reductions (the same torch operations on the same values) are too.  The normals term
    differs by at most 24 u per point, so a reduction of it by at most 24 u R, R the same reduction of the weights alone; one more
    unit of the value for the order of the last roundings.  Gradients: an element is its own product plus the sum over a list of at
    most n members; each product is within 64 u of its magnitude in either form and the sums add (n + 1) u sum |product|, so the
    two forms differ by at most (n + 1) (n + 66) u pmax, pmax the largest gradient element of the composed form taken one direction
    at a time (there every element of the query side is a single product)."""
    uses, extra = cc.GOLDEN_CASES[name]
    inp = {k[3:]: torch.from_numpy(v) for k, v in cc.load_golden().items() if k.startswith("in/")}
    runs = []
    for fused in (True, False):
        kw = cc.golden_kwargs(uses, inp, torch.float32, device=DEV)
        res = chamfer_distance(**kw, **extra, fused=fused)
        cc.scalar_of(res).backward()
        runs.append((kw, res))
    (kf, rf), (kc, rc) = runs
    if "w" in uses:
        assert rf[3][0] is kf["x_weights"] and rf[3][1] is kf["y_weights"]
    pr, br = extra.get("point_reduction", "mean"), extra.get("batch_reduction", "mean")
    for slot, (a, b) in enumerate(zip(rf, rc)):
        for side, (va, vb) in enumerate(zip(a, b)):
            assert (va is None) == (vb is None)
            if va is None:
                continue
            if slot != 1:
                assert torch.equal(va, vb), (name, slot, side)
                continue
            P = (cc.GOLDEN_P1, cc.GOLDEN_P2)[side]
            lengths = np.array(cc.GOLDEN_LENGTHS[side] if "l" in uses else (P,) * cc.GOLDEN_N, dtype=np.float64)
            w = rc[3][side].double().cpu().numpy() if rc[3][side] is not None else None
            unit = (np.ones((cc.GOLDEN_N, P)) if w is None else w) * (np.arange(P)[None, :] < lengths[:, None])
            R = cc.reduce64(unit, w, lengths, pr, br)
            err = (va.detach() - vb.detach()).abs().double().cpu().numpy()
            assert np.all(err <= 24 * U * R + U * np.abs(vb.detach().double().cpu().numpy())), (name, "normals", side)
    # gradients
    n, pmax = 1, 0.0
    for swap in (False, True):
        kw = cc.golden_kwargs(uses, inp, torch.float32, device=DEV)
        if swap:
            kw = {(("y" + k[1:]) if k[0] == "x" else ("x" + k[1:])): v for k, v in kw.items()}
        one = dict(extra, single_directional=True)
        res = chamfer_distance(**kw, **one, fused=False)
        cc.scalar_of(res).backward()
        pmax = max([pmax] + [float(kw[k].grad.abs().max()) for k in ("x", "x_normals") if k in kw and kw[k].grad is not None])
        idx = nearest.knn_points(kw["x"].detach(), kw["y"].detach(), kw.get("x_lengths"), kw.get("y_lengths"),
                                 norm=extra.get("norm", 2), fused=False).idx
        n = max(n, int(torch.stack([torch.bincount(i.flatten(), minlength=1).max() for i in idx]).max()))
    if "w" in uses or "v" in uses:
        pmax *= 5.0   # weights lie in [0.25, 1.25]: the second direction's carry one more factor than a single run's, over their sum
    for k in ("x", "y", "x_normals", "y_normals"):
        if k in kc and kc[k].grad is not None:
            err = float((kf[k].grad - kc[k].grad).abs().max())
            print(name, k, "err %.3e bound %.3e" % (err, (n + 1) * (n + 66) * U * pmax))
            assert err <= (n + 1) * (n + 66) * U * pmax, (name, k)


def test_strand_geometry_fused_equals_composed():
    g = torch.Generator().manual_seed(21)
    roots = torch.rand(300, 1, 3, generator=g) * 0.2
    steps = torch.nn.functional.normalize(torch.randn(300, 1, 3, generator=g), dim=2) * 0.01 + torch.randn(300, 19, 3, generator=g) * 0.002
    gt = (roots + torch.cumsum(torch.cat((torch.zeros(300, 1, 3), steps), 1), 1)).to(DEV)
    pred = (gt[:257, :17] + torch.randn(257, 17, 3, generator=g).to(DEV) * 0.003).contiguous()
    a = evaluation.strand_geometry(pred, gt, [0.002, 0.005, 0.02], [10.0, 30.0, 80.0], fused=True)
    b = evaluation.strand_geometry(pred, gt, [0.002, 0.005, 0.02], [10.0, 30.0, 80.0], fused=False)
    assert a["thresholds"] == b["thresholds"] and len(a["thresholds"]) == 9
    assert a["precision"] == b["precision"] and a["recall"] == b["recall"] and a["fscore"] == b["fscore"]   # equal counts
    assert 0.0 <= min(a["precision"]) < max(a["precision"]) <= 1.0 and 0.0 <= min(a["recall"]) < max(a["recall"]) <= 1.0
    assert a["chamfer_pred_to_gt"] == b["chamfer_pred_to_gt"] and a["chamfer_gt_to_pred"] == b["chamfer_gt_to_pred"]
    for k in ("direction_pred_to_gt", "direction_gt_to_pred"):
        assert abs(a[k] - b[k]) <= 24 * U
