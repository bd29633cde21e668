"""The reference side of tests/test_gpu_projection_shapes.py, checked without a GPU: for every case of tests/projection_cases.py
the float64 arbiter alone has the properties the device comparison relies on -- otherwise a wrong slab tail could hide behind a
gradient that is zero anyway, or a planted row could take another branch than the one it was built for."""
import numpy as np
import pytest
import torch

from tests import projection_cases as pc

IDS = [c.name for c in pc.SHAPES]


def test_the_shapes_cover_every_tail_row_width_and_owner():
    Ps = {c.P for c in pc.SHAPES}
    assert Ps >= {1, 2, 3, 63, 64, 65, 127, 129, 255, 256, 257, 513}
    assert {c.max_deg for c in pc.SHAPES} == {0, 1, 2, 3}
    assert {(c.max_deg, c.active) for c in pc.SHAPES} >= {(3, 1), (2, 0), (3, 3), (1, 1), (2, 2)}
    for K_deg in (1, 3):  # K = 4 and K = 16: rows of 9 and 45 floats, both 1 mod 4
        for blk in (64, 256):  # backward wave (slab_dma, slab_out), forward workgroup (slab_load / slab_to_lds)
            rem = {((c.P % blk or blk) * 3 * ((c.max_deg + 1) ** 2 - 1)) % 4 for c in pc.SHAPES if c.max_deg == K_deg}
            assert rem >= {1, 2, 3}, (K_deg, blk, rem)
    # the fused update (slab_out_adam) runs on the owned cases only
    rem = {((c.P % 64 or 64) * 3 * ((c.max_deg + 1) ** 2 - 1)) % 4 for c in pc.OWNED}
    assert rem >= {0, 1, 2, 3}, rem
    assert {c.P for c in pc.OWNED} >= {63, 64, 65, 257} and {c.max_deg for c in pc.OWNED} == {1, 3}
    assert {(c.W, c.H) for c in pc.SHAPES} == {(64, 48), (70, 37)}
    assert [pc.BY_NAME[n].P for n in pc.CAMERA_CASES] == [1, 63, 64, 65, 129, 257]


@pytest.mark.parametrize("name", IDS)
def test_reference_alone_has_what_the_device_comparison_relies_on(name):
    """`Every visible Gaussian has a non-zero last features_rest row` is asserted for every CONTRIBUTING one: a Gaussian some
    weighted pixel composited.  The planted opacity -12 row never passes alpha >= 1/255, and a random row may lie behind opaque
    neighbours; at least 95 % of the visible rows contribute.  What the tails need is pinned exactly: the model's last three
    rows contribute, with every channel of their last active coefficient non-zero, and in the cases of one to three Gaussians
    every row does.  Prints how far the float32 oracle chain itself lies from float64 in units of the row criterion: the
    device test's bar carries three times that distance, a fixed 1e-4 would not."""
    from tests.projection_shared import row_unit
    case = pc.BY_NAME[name]
    a = pc.arbiter_cached(name)
    g64, g32 = a["g64"], a["g32"]
    P = case.P
    assert a["named"].mean() <= 0.05, a["named"].mean()
    for k in g64:
        assert np.isfinite(g64[k]).all() and np.isfinite(g32[k]).all(), k
    vis = a["radii"] > 0
    assert np.array_equal(vis, a["keep"])
    assert vis.mean() >= 0.9, vis.mean()     # nearly every Gaussian is visible
    # a Gaussian CONTRIBUTES when some weighted pixel composited it (the opacity -12 row and rows hidden behind others do not)
    dc = g64["_features_dc"].reshape(P, 3)
    contrib = vis & (np.abs(dc).max(axis=1) > 0)
    assert contrib.sum() >= 0.95 * vis.sum() - 1
    if not pc.planted(case):
        assert contrib.all(), contrib
    own = {k: float((np.abs(g32[k] - g64[k]).reshape(P, -1) / row_unit(g64[k])).max()) for k in pc.PARAMS
           if g64[k].size and np.abs(g64[k]).max() > 0}
    print(name, "oracle32 chain vs float64 in units of the row criterion:", {k: round(v, 3) for k, v in own.items()})
    first_off, n_rows = pc.last_coeff_rows(case)
    rest = g64["_features_rest"].reshape(P, n_rows, 3)
    if n_rows:
        # exact zeros above the active degree, in both precisions
        assert not rest[:, first_off:].any() and not g32["_features_rest"].reshape(P, n_rows, 3)[:, first_off:].any()
    if n_rows and first_off:
        last = rest[:, first_off - 1]
        assert (np.abs(last[contrib]).max(axis=1) > 0).all()
        # the model's last rows are what a wrong tail corrupts: they contribute, every channel of the last active coefficient
        tail_rows = list(range(max(0, P - 3), P))
        assert contrib[tail_rows].all(), contrib[tail_rows]
        if case.active == case.max_deg:
            assert (last[tail_rows] != 0).all(), last[tail_rows]
    if not pc.planted(case):
        return
    # ---- planted rows
    for k in pc.PARAMS:
        assert not g64[k][pc.ROW_BEHIND].any() and not g32[k][pc.ROW_BEHIND].any(), k     # culled: exact zeros everywhere
    assert not vis[pc.ROW_BEHIND]
    others = [r for r in range(pc.N_PLANTED) if r != pc.ROW_BEHIND]
    assert vis[others].all(), a["radii"][:pc.N_PLANTED]
    for r in (pc.ROW_CLAMP_X, pc.ROW_CLAMP_Y, pc.ROW_CUT, pc.ROW_Q3, pc.ROW_QSMALL, pc.ROW_OP_HI, pc.ROW_TIE):
        assert contrib[r], r
        assert np.abs(g64["_rotation"][r]).max() > 0 and np.abs(g64["_xyz"][r]).max() > 0, r
    cut = dc[pc.ROW_CUT]
    assert cut[0] == 0.0 and cut[1] != 0.0 and cut[2] != 0.0, cut
    assert g32["_features_dc"].reshape(P, 3)[pc.ROW_CUT, 0] == 0.0
    if n_rows and first_off:
        rc = rest[pc.ROW_CUT, :first_off]
        assert not rc[:, 0].any() and rc[:, 1:].any()
    margins = pc.branch_margins(case)
    for what, m in margins.items():
        assert m >= 1e-3, (what, m)
    # the clamp rows lie outside the frame (their ellipse reaches in): pixel mean beyond the last column / row
    assert a["means2d"][pc.ROW_CLAMP_X, 0] > case.W and 0 <= a["means2d"][pc.ROW_CLAMP_X, 1] < case.H
    assert a["means2d"][pc.ROW_CLAMP_Y, 1] > case.H and 0 <= a["means2d"][pc.ROW_CLAMP_Y, 0] < case.W
    assert a["means2d"][pc.ROW_CLAMP_X, 0] - a["radii"][pc.ROW_CLAMP_X] < case.W - 1
    assert a["means2d"][pc.ROW_CLAMP_Y, 1] - a["radii"][pc.ROW_CLAMP_Y] < case.H - 1
    # the tie: both precisions take the FIRST of the two equal longest axes (gaussian_model.py:384-388)
    for dtype in (torch.float32, torch.float64):
        s = pc.build_model(case, "cpu", owned=False).get_scaling.detach().to(dtype)[pc.ROW_TIE]
        assert s[0] == s[1] and s[0] > s[2]
        assert int(s[None].argsort(dim=-1, descending=True)[0, 0]) == 0
    assert np.abs(g64["_scaling"][pc.ROW_TIE]).max() > 0


@pytest.mark.parametrize("name", pc.CAMERA_CASES)
def test_camera_arbiter_has_gradients_where_the_projection_reads_the_camera(name):
    a = pc.arbiter_cached(name, True)
    v = a["g64"]["view_direct"]
    # column 3 of the view matrix is never read by the projection: exact zeros on the direct path (the leaf's total also
    # collects the path through the inverse behind camera_center, which is not zero there)
    assert v.shape == (4, 4) and not v[:, 3].any() and not a["g32"]["view_direct"][:, 3].any()
    assert (v[:, :3] != 0).all() and a["g64"]["FoVx"] != 0 and a["g64"]["FoVy"] != 0
    assert (a["g64"]["world_view_transform"][:, :3] != 0).all()
    # the model's gradients do not depend on whether the camera is a leaf (double rounding of a differently ordered graph)
    b = pc.arbiter_cached(name)
    for k in pc.PARAMS:
        assert np.allclose(a["g64"][k], b["g64"][k], rtol=1e-9, atol=1e-9 * np.abs(b["g64"][k]).max(initial=0.0)), k


@pytest.mark.parametrize("name", [c.name for c in pc.OWNED])
def test_the_two_ring_views_of_the_owned_cases_name_few_pixels_and_reach_the_last_rows(name):
    case = pc.BY_NAME[name]
    first_off, n_rows = pc.last_coeff_rows(case)
    total = 0.0
    for index in (0, 1):
        a = pc.arbiter_cached(name, False, index)
        assert a["named"].mean() <= 0.05
        total = total + a["g64"]["_features_rest"].reshape(case.P, n_rows, 3)[:, first_off - 1]
    assert (total[max(0, case.P - 3):] != 0).all()   # the summed gradient of the last rows' last coefficient: every channel
