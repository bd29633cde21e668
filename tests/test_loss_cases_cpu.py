"""The per-pixel loss tests' own ground (tests/loss_cases.py), on the CPU: the shape table says what its rows claim, the
inputs keep clear of the orientation term's kinks, the reference run in float32 sits about two orders inside every bar the
kernels are held to, and the split-group gradient criterion rejects what the whole-plane one lets through."""
import numpy as np
import pytest
import torch

from tests import loss_cases as lc


def test_shape_table_is_well_formed():
    assert len(set(lc.ALL_SHAPES)) == len(lc.ALL_SHAPES)
    assert set(lc.MARCH_GEOMETRY) == set(lc.MARCH_SHAPES) | {(20, 36)} and set(lc.TILE_GEOMETRY) == set(lc.TILE_SHAPES)
    assert set(lc.SEGMENT_SHAPES) <= set(lc.MARCH_GEOMETRY)
    for (H, W), want in lc.MARCH_GEOMETRY.items():
        assert W % 4 == 0 and H * W < 2 ** 30                     # what the host asks of the marching form
        nst = (W + 31) // 32
        got = (nst, 8 * ((nst + 7) // 8), (H + 31) // 32, H - 32 * ((H - 1) // 32), W - 32 * (nst - 1))
        assert got == want, ((H, W), got, want)
    for (H, W), want in lc.TILE_GEOMETRY.items():
        assert W % 4 != 0                                         # only the tile form can take it
        tx, ty = (W + 31) // 32, (H + 15) // 16
        got = (tx, ty, W - 32 * (tx - 1), H - 16 * (ty - 1))
        assert got == want, ((H, W), got, want)
    # the rows of the table, in numbers
    assert min(H for H, _ in lc.MARCH_SHAPES) == 1 and min(W for _, W in lc.MARCH_SHAPES) == 4
    assert any(H <= 5 for H, _ in lc.MARCH_SHAPES) and any(H == 8 and W < 32 for H, W in lc.MARCH_SHAPES)
    assert lc.MARCH_GEOMETRY[(9, 260)][:2] == (9, 16)             # nine strips on sixteen grid columns: strips 2 per XCD, gaps
    assert (20 + 7) // 8 == 3 and 20 - 16 == 4                    # (20, 36) at 8 rows per segment: three, the last half a pass
    assert len(lc.WEIGHTS) == 5 and lc.WEIGHTS[0] == (0.8, 0.2, 0.2, 0.1)
    assert [w.index(1.0) for w in lc.ONE_HOT] == [0, 1, 2, 3] and all(sum(w) == 1.0 for w in lc.ONE_HOT)


@pytest.mark.parametrize("H,W", lc.ALL_SHAPES)
def test_make_case_leaves_no_pixel_near_a_kink(H, W):
    c = lc.make_case(H, W)
    assert c["renders"].shape == (10, H, W) and c["renders"].dtype == torch.float32
    for k, n in (("gt_image", 3), ("gt_mask", 2), ("gt_angle", 1), ("gt_oconf", 1)):
        assert c[k].shape == (n, H, W) and c[k].dtype == torch.float32 and c[k].is_contiguous()
    assert not bool(lc.near_kink(c).any())
    ordinary = ~c["special"]
    assert not bool(lc.kink_distance_mask(c["renders"], c["gt_angle"])[ordinary].any())
    assert c["replaced"] <= 0.25                                   # the inputs stay what they were meant to be
    assert set(c["gt_mask"].unique().tolist()) <= {0.0, 1.0} and float(c["gt_oconf"].min()) >= 0.05
    assert bool(c["gt_mask"][0].any()) and bool(c["gt_mask"][1].any())   # neither term is masked away everywhere
    assert int(c["special"].sum()) == (H // 6) * W if H >= 6 else not bool(c["special"].any())
    sp = c["special"]
    assert float(c["renders"][5:7][:, sp].abs().sum()) == 0.0 and float(c["renders"][8][sp].abs().sum()) == 0.0
    assert float(c["renders"][8][ordinary].min()) >= 0.05
    again = lc.make_case(H, W)
    assert all(torch.equal(c[k], again[k]) for k in ("renders", "gt_image", "gt_mask", "gt_angle", "gt_oconf", "special"))


@pytest.mark.parametrize("mask_colours", [True, False])
@pytest.mark.parametrize("H,W", lc.ALL_SHAPES)
def test_float32_reference_sits_inside_every_bar(H, W, mask_colours):
    """The same composed form in float32 against float64: measured at most 5.0e-6 of a group's maximum in any gradient
    (bar 2e-4) and 2.0e-7 in the value (bar 5e-6) over the table and the five weight vectors; held here to a twentieth of
    each bar."""
    c = lc.make_case(H, W)
    for w in lc.WEIGHTS:
        ref = lc.reference64(c, w, mask_colours)
        loss32, terms32, grad32 = lc.composed(c, w, mask_colours, torch.float32)
        ev = lc.check_value(loss32, ref["loss"], ("float32", H, W, w))
        eg = lc.check_grad(grad32, ref["grad"], c["special"], ("float32", H, W, w))
        assert ev <= lc.VALUE_BAR / 20 and eg <= lc.GRAD_BAR / 20, (H, W, w, ev, eg)
        e32 = lc.float32_error(c, w, mask_colours)
        assert e32 and max(e32.values()) == pytest.approx(eg, rel=1e-12)   # the same figure, group by group
        assert np.isfinite(ref["grad"]).all() and all(np.isfinite(ref["terms"]))
    assert ref["mu2"].shape == ref["e22"].shape == (3, H, W)
    assert (ref["e22"] >= ref["mu2"] ** 2 - 1e-12).all()           # a variance


def test_reference_terms_add_up_and_a_nan_orientation_term_is_dropped():
    c = lc.make_case(9, 32)
    blended = lc.reference64(c, lc.BLENDED, True)
    hot = [lc.reference64(c, w, True) for w in lc.ONE_HOT]
    assert blended["loss"] == pytest.approx(sum(wi * h["loss"] for wi, h in zip(lc.BLENDED, hot)), rel=1e-14)
    assert [h["loss"] for h in hot] == list(blended["terms"])
    assert not hot[0]["grad"][3:].any() and not hot[2]["grad"][:3].any() and not hot[2]["grad"][5:].any()
    assert not hot[3]["grad"][:5].any() and hot[3]["grad"][5:7].any() and hot[3]["grad"][8].any()
    assert not blended["grad"][7].any() and not blended["grad"][9].any()
    c["gt_oconf"] = torch.zeros_like(c["gt_oconf"])               # weight.sum() == 0 -> 0 / 0
    dropped = lc.reference64(c, lc.BLENDED, True)
    assert dropped["terms"][3] == 0.0 and not dropped["grad"][5:].any()
    assert dropped["terms"][:3] == blended["terms"][:3] and np.array_equal(dropped["grad"][:5], blended["grad"][:5])


def test_split_groups_reject_what_the_whole_plane_criterion_accepts():
    """A confidence gradient that is 1 % off at every ordinary pixel.  Over the whole plane the scale is the special pixels'
    1 / 1e-7, so 2e-4 of it is two thousand times an ordinary value: the old criterion cannot see the error."""
    H, W = 33, 64
    c = lc.make_case(H, W)
    ref = lc.reference64(c, lc.BLENDED, True)["grad"]
    sp = c["special"].numpy()
    conf = np.abs(ref[8])
    assert conf[sp].max() > 1000 * conf[~sp].max() > 0             # the two populations of gap 2
    off = ref.copy()
    off[8][~sp] *= 1.01
    assert lc.check_grad_whole_plane(ref, ref) and lc.check_grad_whole_plane(off, ref)
    lc.check_grad(ref, ref, sp)
    with pytest.raises(AssertionError, match="conf"):
        lc.check_grad(off, ref, sp, "perturbed")
    # the other things check_grad is there to refuse
    for plane, value in ((7, 1e-30), (0, float("nan"))):
        broken = ref.copy()
        broken[plane, H - 1, W - 1] = value
        with pytest.raises(AssertionError):
            lc.check_grad(broken, ref, sp)
    with pytest.raises(AssertionError):
        lc.check_value(1.0 + 1e-5, 1.0)
    lc.check_value(1.0 + 4e-6, 1.0)
