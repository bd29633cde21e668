"""`-m gpu`: the fused loss kernels (csrc/ghr_loss.h: forward, ground-truth window moments, backward; tile form and marching
form of each) per pixel against the float64 reference of tests/loss_cases.py, at the shapes where their spatial logic -- tiles,
halos, strips, row batches, segment hand-over, clamped addresses -- takes another turn.  The table and the reason for each
entry are in tests/loss_cases.py; in short

  marching form (W % 4 == 0): (1, 4) one row, one float4, every row batch but one outside the image; (3, 8), (5, 12) no
  taller than the window radius; (8, 28) exactly one pass, a strip under 32 columns whose right halo is inside the aligned
  window but outside the image; (9, 32) one row into a second pass, right halo all outside; (11, 36) a second strip of one
  float4 with a real left halo; (32, 64) exactly one segment, two full strips; (33, 64) a second segment of one row whose
  ten rows above are the other segment's (the L1 term's `own` test); (40, 68) a second segment of one pass, three strips, the
  last of one float4; (9, 260) nine strips on a grid padded to 16 (empty strips in the strip-to-XCD remap); (20, 36) at 8
  rows per segment three segments, the last of half a pass.
  tile form: (1, 1); (6, 5) smaller than the window; (10, 11) about its size; (16, 33) a second tile of one column;
  (17, 31) a second tile row of one row; (26, 42) exactly a tile plus its halo.

Every launch goes through `run()` below, straight to the C ABI.  Every output buffer (maps [9, H, W], sums, stats
[2, 3, H, W], the packed gradient [10, H, W] with planes 7 and 9 handed over as the two zero planes, the loss) has a guard of
64 floats on either side; payload and guards start as NaN.  After each call the guards are still the same NaN bit for bit,
every element the kernel owns is finite, and of `sums` exactly the slots of the form the host should have picked were written
(the rest is still NaN): a kernel that skips a pixel, writes outside its planes or runs in the other form than expected is
caught whatever the allocator handed out.  Every comparison is per element against float64 or bit for bit between two forms
of one kernel; no pixel is left out of any."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import loss_cases as lc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD = 64
UP = float(np.float32(0.37))   # dL/dloss handed to the backward kernels
LOSS_AUX = 8                   # floats in front of the slots of `sums` (GHR_LOSS_AUX)
INPUTS = ("renders", "gt_image", "gt_mask", "gt_angle", "gt_oconf")


class Guarded:
    """a float32 device buffer of `shape` between two guards, all NaN"""

    def __init__(self, *shape):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV)
        self.t = self.buf[GUARD:GUARD + n].view(*shape)
        bits = self.buf.view(torch.int32)
        self.nan_bits = int(bits[0])                   # one NaN pattern throughout, whichever the fill chose
        assert self.t.data_ptr() % 16 == 0 and bool(torch.isnan(self.buf).all()) and bool((bits == self.nan_bits).all())

    def ptr(self, plane=0):
        return ctypes.c_void_p(self.t.data_ptr() + 4 * plane * self.t[0].numel()) if plane else ctypes.c_void_p(self.t.data_ptr())

    def check(self, what, owned=None):
        """guards untouched; the owned elements (default: all) finite, the others still NaN"""
        bits = self.buf.view(torch.int32)
        assert bool((bits[:GUARD] == self.nan_bits).all()), (what, "wrote in front of the buffer")
        assert bool((bits[-GUARD:] == self.nan_bits).all()), (what, "wrote behind the buffer")
        flat = self.t.reshape(-1)
        if owned is None:
            bad = ~torch.isfinite(flat)
            assert not bool(bad.any()), (what, "not written / not finite at", bad.nonzero()[:4].flatten().tolist())
        else:
            assert bool(torch.isfinite(flat[owned]).all()), (what, "an owned slot was not written")
            assert bool((flat.view(torch.int32)[~owned] == self.nan_bits).all()), (what, "wrote a slot it does not own")


def to_dev(c, unaligned=False):
    """the case's inputs on the device; `unaligned`: every base 4 bytes past a 16-byte boundary"""
    d = {}
    for k in INPUTS:
        v = c[k]
        if unaligned:
            buf = torch.empty(v.numel() + 1, dtype=torch.float32, device=DEV)
            d[k] = buf[1:].view(v.shape)
            d[k].copy_(v)
            assert d[k].data_ptr() % 16 == 4
        else:
            d[k] = v.to(DEV).contiguous()
            assert d[k].data_ptr() % 16 == 0
    return d


def _seg(env, name):
    v = int(env.get(name, "0") or 0)
    return (v if v > 0 else 32) + 7 & ~7


def expected_slots(H, W, marching, seg):
    return 3 * ((W + 31) // 32) * ((H + seg - 1) // seg if marching else (H + 15) // 16)


def run(d, H, W, w, mask_colours=True, cached=False, marching=None):
    """ghr_loss_gt_stats (always: its output is checked either way; handed to the forward when `cached`), ghr_loss_forward,
    ghr_loss_backward on guarded NaN-filled buffers.  `marching`: the form the host is expected to pick (default: from W and
    the environment, for aligned inputs).  Returns host copies."""
    from gaussianhaircut_amd import _lib
    L = _lib.lib()
    if marching is None:
        marching = W % 4 == 0 and "GHR_LOSS_SCALAR" not in os.environ
    n = H * W
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    r = d["renders"]
    off = lambda t, plane: ctypes.c_void_p(t.data_ptr() + 4 * plane * n)
    a = _lib.LossArgs()
    a.W, a.H = W, H
    a.image, a.mask, a.dir2d, a.orient_conf = off(r, 0), off(r, 3), off(r, 5), off(r, 8)
    a.gt_image, a.gt_mask = off(d["gt_image"], 0), off(d["gt_mask"], 0)
    a.gt_orient_angle, a.gt_orient_conf = off(d["gt_angle"], 0), off(d["gt_oconf"], 0)
    a.w_l1, a.w_ssim, a.w_mask, a.w_orient = [float(x) for x in w]
    a.unmasked_colours = int(not mask_colours)
    a.gt_stats = None
    what = (H, W, tuple(w), mask_colours, cached, "marching" if marching else "tile")

    stats = Guarded(2, 3, H, W)
    _lib.check(L.ghr_loss_gt_stats(stream, ctypes.byref(a), stats.ptr()))
    torch.cuda.synchronize()
    stats.check(what + ("gt_stats",))

    maps, loss = Guarded(9, H, W), Guarded(1)
    n_sums = _lib.loss_sums_floats(W, H)
    sums = Guarded(n_sums)
    n_slots = expected_slots(H, W, marching, _seg(os.environ, "GHR_LOSS_SEG_F"))
    assert LOSS_AUX + 5 * n_slots <= n_sums
    owned = torch.zeros(n_sums, dtype=torch.bool, device=DEV)
    owned[:2] = True                                   # {sum of the orientation weights, NaN flag}
    owned[LOSS_AUX:LOSS_AUX + 5 * n_slots] = True      # [term][slot]
    if cached:
        a.gt_stats = stats.ptr()
    _lib.check(L.ghr_loss_forward(stream, ctypes.byref(a), maps.ptr(), sums.ptr(), loss.ptr()))
    torch.cuda.synchronize()
    for g, o, name in ((maps, None, "maps"), (sums, owned, "sums"), (loss, None, "loss"), (stats, None, "gt_stats after forward")):
        g.check(what + (name,), o)

    grad = Guarded(10, H, W)
    gl = torch.tensor([UP], dtype=torch.float32, device=DEV)
    a.gt_stats = None
    _lib.check(L.ghr_loss_backward(stream, ctypes.byref(a), maps.ptr(), sums.ptr(), ctypes.c_void_p(gl.data_ptr()),
                                   grad.ptr(0), grad.ptr(3), grad.ptr(5), grad.ptr(8), grad.ptr(7), grad.ptr(9)))
    torch.cuda.synchronize()
    grad.check(what + ("grad",))
    maps.check(what + ("maps after backward",))
    sums.check(what + ("sums after backward",), owned)
    return dict(loss=float(loss.t[0]), maps=maps.t.cpu().numpy(), stats=stats.t.cpu().numpy(), grad=grad.t.cpu().numpy())


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def same_bits(a, b, what):
    assert np.array_equal(bits(a), bits(b)), (what, "differs at", np.argwhere(bits(a) != bits(b))[:4].tolist())


def compare_forms(a, b, what, orient_planes_exact=False):
    """two forms of the same kernels: maps, cached moments and the gradient planes 0-4, 7, 9 the same bits; the loss within
    2e-6 relative and planes 5, 6, 8 within 3e-7 of their maximum (they carry 1 / sum(weights), a sum whose last bit depends
    on the order of its partial sums) -- or, where that order is the same too, the same bits as well"""
    same_bits(a["maps"], b["maps"], what + ("maps",))
    same_bits(a["stats"], b["stats"], what + ("moments",))
    for p in (0, 1, 2, 3, 4, 7, 9):
        same_bits(a["grad"][p], b["grad"][p], what + ("gradient plane %d" % p,))
    assert abs(a["loss"] - b["loss"]) <= 2e-6 * abs(a["loss"]), (what, a["loss"], b["loss"])
    for p in (5, 6, 8):
        if orient_planes_exact:
            same_bits(a["grad"][p], b["grad"][p], what + ("gradient plane %d" % p,))
        else:
            err, top = np.abs(a["grad"][p] - b["grad"][p]).max(), np.abs(a["grad"][p]).max()
            print("%s plane %d: %.3g of its maximum" % (what, p, err / top if top else 0.0))
            assert err <= 3e-7 * top, (what, p, err, top)


def test_the_guards_catch_a_stray_write():
    g = Guarded(3, 5)
    g.t.fill_(1.0)
    g.check("in place")
    for i in (GUARD - 1, GUARD + 15):
        g.buf[i] = 0.0
        with pytest.raises(AssertionError, match="wrote"):
            g.check("stray")
        g.buf[i] = float("nan")
    g.t[1, 2] = float("nan")
    with pytest.raises(AssertionError, match="not written"):
        g.check("skipped")


@pytest.mark.parametrize("mask_colours", [True, False])
@pytest.mark.parametrize("H,W", lc.MARCH_SHAPES + lc.TILE_SHAPES)
def test_each_form_matches_float64_per_pixel(H, W, mask_colours):
    """the form the host picks for the shape; ground-truth moments cached or not; the blended weights and the four one-hot
    vectors (each term's value on its own)"""
    c = lc.make_case(H, W)
    d = to_dev(c)
    for cached in (False, True):
        for w in lc.WEIGHTS:
            ref = lc.reference64(c, w, mask_colours)
            out = run(d, H, W, w, mask_colours, cached)
            what = (H, W, w, mask_colours, cached)
            ev = lc.check_value(out["loss"], ref["loss"], what)
            eg = lc.check_grad(out["grad"], ref["grad"] * UP, c["special"].numpy(), what)
            es = max(np.abs(out["stats"][0] - ref["mu2"]).max(), np.abs(out["stats"][1] - ref["e22"]).max())
            print("%s value %.3g of %.3g, gradient %.3g of %.3g, moments %.3g of %.3g" %
                  (what, ev, lc.VALUE_BAR, eg, lc.GRAD_BAR, es, lc.STATS_ATOL))
            assert es <= lc.STATS_ATOL, (what, es)


@pytest.mark.parametrize("H,W", lc.MARCH_SHAPES)
def test_marching_and_tile_forms_agree_bit_for_bit(H, W, monkeypatch):
    c = lc.make_case(H, W)
    d = to_dev(c)
    for mask_colours in (True, False):
        for cached in (False, True):
            monkeypatch.delenv("GHR_LOSS_SCALAR", raising=False)
            march = run(d, H, W, lc.BLENDED, mask_colours, cached)
            monkeypatch.setenv("GHR_LOSS_SCALAR", "1")
            tile = run(d, H, W, lc.BLENDED, mask_colours, cached)
            compare_forms(tile, march, (H, W, mask_colours, cached))


def test_an_unaligned_base_takes_the_tile_form(monkeypatch):
    """(33, 64) at a base 4 bytes off a 16-byte boundary: the tile form (the slots of `sums` it writes say so), the same bits
    per pixel as the aligned run -- all of them against the aligned tile run, and against the aligned marching run all but the
    last bit of the orientation term's normaliser"""
    H, W = 33, 64
    c = lc.make_case(H, W)
    monkeypatch.delenv("GHR_LOSS_SCALAR", raising=False)
    assert expected_slots(H, W, True, 32) != expected_slots(H, W, False, 32)
    for cached in (False, True):
        march = run(to_dev(c), H, W, lc.BLENDED, True, cached, marching=True)
        off = run(to_dev(c, unaligned=True), H, W, lc.BLENDED, True, cached, marching=False)
        compare_forms(off, march, (H, W, "unaligned against marching", cached))
        monkeypatch.setenv("GHR_LOSS_SCALAR", "1")
        tile = run(to_dev(c), H, W, lc.BLENDED, True, cached, marching=False)
        monkeypatch.delenv("GHR_LOSS_SCALAR")
        compare_forms(off, tile, (H, W, "unaligned against tile", cached), orient_planes_exact=True)
        assert off["loss"] == tile["loss"]
        ref = lc.reference64(c, lc.BLENDED, True)
        lc.check_value(off["loss"], ref["loss"], "unaligned")
        lc.check_grad(off["grad"], ref["grad"] * UP, c["special"].numpy(), "unaligned")


@pytest.mark.parametrize("H,W", lc.SEGMENT_SHAPES)
def test_segment_length_changes_no_per_pixel_output(H, W, monkeypatch):
    """GHR_LOSS_SEG_F / GHR_LOSS_SEG_B at 8 and 16 rows against the default 32: where a strip is handed from one wave to the
    next moves, what a pixel gets does not.  (20, 36) at 8: three segments, the last of half a pass.

    maps, moments and every gradient plane are the same bits -- with one exception that is arithmetic, not placement.
    Planes 5, 6 and 8 carry 1 / sum(gt_oconf), and that sum is folded from one partial sum per wave of the FORWARD kernel:
    another forward segment length groups the same float32 additions differently.  Restating the kernels' order of
    additions (per lane down the strip, the DPP wave sum, k_loss_finalize) in numpy float32 on these very inputs gives a
    normaliser one unit in the last place apart between 32, 16 and 8 rows at (20, 36) (bits ...343, ...344, ...342) and
    between 32 and 16 at (40, 68), and the same bits at (33, 64).  So where GHR_LOSS_SEG_F differs from the default those
    three planes are held, group by group, to four times the error of the composed form run in float32 against float64 at
    this case (tests/loss_cases.float32_error; 6e-8 .. 1.4e-6 of a group's maximum here) instead of to identity; a group
    whose values are all zero stays exactly zero.  With the forward segments unchanged (GHR_LOSS_SEG_B alone) all ten
    planes are the same bits."""
    c = lc.make_case(H, W)
    d = to_dev(c)
    special = c["special"].numpy()
    e32 = lc.float32_error(c, lc.BLENDED, True)
    for name in ("GHR_LOSS_SCALAR", "GHR_LOSS_SEG_F", "GHR_LOSS_SEG_B"):
        monkeypatch.delenv(name, raising=False)
    base = {cached: run(d, H, W, lc.BLENDED, True, cached) for cached in (False, True)}
    for seg_f in (None, 8, 16):
        for seg_b in (None, 8, 16):
            if seg_f is None and seg_b is None:
                continue
            for name, v in (("GHR_LOSS_SEG_F", seg_f), ("GHR_LOSS_SEG_B", seg_b)):
                if v is None:
                    monkeypatch.delenv(name, raising=False)
                else:
                    monkeypatch.setenv(name, str(v))
            for cached in (False, True):
                out, ref = run(d, H, W, lc.BLENDED, True, cached), base[cached]
                what = (H, W, "segments", seg_f, seg_b, cached)
                same_bits(out["maps"], ref["maps"], what + ("maps",))
                same_bits(out["stats"], ref["stats"], what + ("moments",))
                for p in (0, 1, 2, 3, 4, 7, 9) + ((5, 6, 8) if seg_f is None else ()):
                    same_bits(out["grad"][p], ref["grad"][p], what + ("gradient plane %d" % p,))
                assert abs(out["loss"] - ref["loss"]) <= 2e-6 * abs(ref["loss"]), what
                if seg_f is None:
                    continue
                for group, planes in (("dir", [5, 6]), ("conf", [8])):
                    for kind, sel in (("ordinary", ~special), ("special", special)):
                        x, y = out["grad"][planes][:, sel].astype(np.float64), ref["grad"][planes][:, sel].astype(np.float64)
                        if (group, kind) not in e32:
                            assert not x.any() and not y.any(), what + (group, kind)
                            continue
                        err, scale = np.abs(x - y).max(), np.abs(y).max()
                        print("%s %s %s: %.3g of the maximum, bar %.3g" % (what, group, kind, err / scale, 4 * e32[(group, kind)]))
                        assert err <= 4 * e32[(group, kind)] * scale, what + (group, kind, err / scale, 4 * e32[(group, kind)])


@pytest.mark.parametrize("H,W", [(9, 32), (6, 5)])
def test_zero_orientation_weight_and_no_orientation_term(H, W):
    """w_orient = 0, and gt_oconf all zero (sum of weights 0 -> a NaN term, which is dropped): planes 5-9 exactly zero, a
    finite loss equal to the reference's"""
    c = lc.make_case(H, W)
    w0 = lc.BLENDED[:3] + (0.0,)
    empty = dict(c, gt_oconf=torch.zeros_like(c["gt_oconf"]))
    for case, w in ((c, w0), (empty, lc.BLENDED), (empty, w0)):
        ref = lc.reference64(case, w, True)
        assert ref["terms"][3] == 0.0 or w[3] == 0.0
        for cached in (False, True):
            out = run(to_dev(case), H, W, w, True, cached)
            assert not bits(out["grad"][5:]).any() and np.isfinite(out["loss"]), (H, W, w, cached, "planes 5-9")
            lc.check_value(out["loss"], ref["loss"], (H, W, w, cached))
            lc.check_grad(out["grad"], ref["grad"] * UP, c["special"].numpy(), (H, W, w, cached))
