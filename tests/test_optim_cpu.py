"""Host logic of gaussianhaircut_amd.optim that needs no GPU: the ZeRO-1 range plan and the argument checks."""
import pytest
import torch

from gaussianhaircut_amd import _lib
from gaussianhaircut_amd.optim import FusedAdam, _zero_grad_mode


def test_shard_plan_covers_every_range_once_and_keeps_slices_aligned():
    plan = [(0, 3_000_000, "sum"), (3_000_000, 25_500_000, ("rest", 500_000, 15, 3)), (25_500_000, 30_500_123, "sum"),
            (30_500_123, 30_500_200, "none")]
    for G in (1, 2, 3, 8):
        out = FusedAdam._shard_plan(plan, G)
        # same cover, same order, nothing overlapping
        assert out[0][0] == 0 and out[-1][1] == plan[-1][1]
        assert all(a[1] == b[0] for a, b in zip(out, out[1:]))
        for a, b, how in out:
            if how == "shard":
                assert (b - a) % (G * 256) == 0 and b > a      # every rank's slice is a whole number of 1-KiB pieces
            elif how == "sum":
                assert b - a < G * 256 or G == 0                # only the tail that does not divide stays replicated
        kept = [(a, b, h) for a, b, h in out if h not in ("shard", "sum")]
        assert kept == [p for p in plan if p[2] not in ("sum",)]
        assert sum(b - a for a, b, h in out if h in ("shard", "sum")) == sum(b - a for a, b, h in plan if h == "sum")


def test_zero_grad_argument_is_validated():
    assert _zero_grad_mode(True) == (True, False) and _zero_grad_mode(False) == (False, False)
    assert _zero_grad_mode("defer") == (False, True)
    for bad in ("true", "Defer", "", "zero"):
        with pytest.raises(ValueError):
            _zero_grad_mode(bad)


def _model_shaped_optimizer(P, act=None, gather=False):
    """A FusedAdam over the groups of GaussianModel.param_groups at P Gaussians (meta tensors: only the plan is built)."""
    widths = [("xyz", (3,)), ("f_dc", (1, 3)), ("f_rest", (15, 3)), ("opacity", (1,)), ("label", (1,)),
              ("scaling", (3,)), ("rotation", (4,)), ("orient_conf", (1,))]
    o = object.__new__(FusedAdam)
    o.param_groups = [dict(name=n, lr=1e-3, params=[torch.empty((P,) + w, device="meta")]) for n, w in widths]
    o.flat_param = torch.empty(61 * P, device="meta")
    o.active_rest_coeffs = act
    o._views = dict(gather=True) if gather else None
    return o


@pytest.mark.parametrize("P", [64 * 99, 500_000, 2001])  # tiny_strands, cfg3, and a P whose f_dc starts off a float4
def test_shard_plan_of_the_real_reduce_plans_for_1_to_8_ranks(P):
    """FusedAdam._shard_plan on the four-chunk plans step_chunked builds: every SH degree (a plain "sum" plan, packed
    ("rest", ...) and "none" f_rest ranges), with and without the gathered view ranges, G = 1..8."""
    for act, gather in [(None, False), (15, False), (8, False), (3, False), (0, False), (None, True), (3, True)]:
        plan = _model_shaped_optimizer(P, act, gather)._reduce_plan(4)
        assert plan[0][0] == 0 and plan[-1][1] == 61 * P
        assert any(how == "sum" for _, _, how in plan)
        for G in range(1, 9):
            out = FusedAdam._shard_plan(plan, G)
            assert out[0][0] == 0 and out[-1][1] == 61 * P, (act, gather, G)
            assert all(x[1] == y[0] for x, y in zip(out, out[1:])), (act, gather, G)  # in order, no gap, no overlap
            assert all(b > a for a, b, _ in out)
            assert [x for x in out if x[2] not in ("shard", "sum")] == [x for x in plan if x[2] != "sum"]
            # every "sum" range of the input is one shard part (if it is long enough) followed by one tail (if any)
            i = 0
            for a, b, how in plan:
                if how != "sum":
                    assert out[i] == (a, b, how)
                    i += 1
                    continue
                main = (b - a) // (G * 256) * (G * 256)
                parts = out[i:i + (main > 0) + (main < b - a)]
                i += len(parts)
                assert parts[0][0] == a and parts[-1][1] == b, (a, b, parts)
                for pa, pb, ph in parts:
                    if ph == "shard":
                        L = (pb - pa) // G
                        assert (pb - pa) % (G * 256) == 0 and pb - pa >= G * 256
                        # every rank's slice start (and the tail's) is on a float4 whenever the range start is
                        assert all((pa + r * L) % 4 == 0 for r in range(G + 1)) or a % 4 != 0
                    else:
                        assert ph == "sum" and pb - pa < G * 256 and pa == a + main, (pa, pb, ph)
                        assert pa % 4 == 0 or a % 4 != 0
            assert i == len(out)


# ---- the hand-off of one training view's direct backward to the optimizer (FusedAdam.open_view / close_view) -------------------
def _cpu_optimizer(P=5):
    """A FusedAdam made by hand over CPU tensors, model-shaped (K = 16): the host-side protocol runs, nothing is launched."""
    widths = [("xyz", (3,)), ("f_dc", (1, 3)), ("f_rest", (15, 3)), ("opacity", (1,)), ("label", (1,)),
              ("scaling", (3,)), ("rotation", (4,)), ("orient_conf", (1,))]
    o = object.__new__(FusedAdam)
    o.param_groups = [dict(name=n, lr=1e-3, params=[torch.nn.Parameter(torch.zeros((P,) + w))]) for n, w in widths]
    o.betas, o.eps, o.nan_guard, o.direct_grads = (0.9, 0.999), 1e-15, True, True
    o.flat_param, o.flat_grad, o.exp_avg, o.exp_avg_sq = (torch.zeros(61 * P) for _ in range(4))
    o.state_dev = torch.zeros(_lib.ADAM_STATE, dtype=torch.int32)
    o._set_ends()
    o._mark_zero()
    return o


def _flag_name(o, ptr):
    words = {o.state_dev.data_ptr() + 4: "state_dev[1]"}
    if o._fuse is not None:
        words.update({o._fuse["flags"].data_ptr() + 4 * i: "fuse%d" % i for i in (0, 1)})
    return words[ptr.value]


def _run_views(o, V, fuse):
    """The views of a step that is open on the optimizer: one (check_overflow, adam_fuse set, accumulate, slot of d_rgb,
    fold, flag word) per view, and the ``accumulate`` of every fold the hand-off asked for (the caller's to execute: taken as
    arguments here, as the native path does)."""
    rows, folds = [], []
    for i in range(V):
        h = o.open_view(fuse and i == V - 1, torch.full((3,), float(i)))
        slot = None
        if h.d_rgb is not None:
            v = o._views
            slot, rem = divmod(h.d_rgb.value - v["buf"].data_ptr(), 4 * v["stride"])
            assert rem == 0 and v["buf"][slot, 3 * v["P"]: 3 * v["P"] + 3].tolist() == [float(i)] * 3
        rows.append((h.check_overflow, h.adam_fuse is not None, h.accumulate, slot, h.fold, _flag_name(o, h.nan_flag)))
        if h.fold:
            folds.append(_lib.ShFoldArgs.from_address(o.fold_own_views_args()).accumulate)
        assert h.wait_event is None
        o.close_view(h)
    return rows, folds


def _step(o, V, fuse, gather=False):
    """One training step on the optimizer's host state, opened as trainer._open_step opens it and ended as the update ends
    it (the fused step's end, or what step(zero_grad="defer") does around its kernel)."""
    o.end_factored_views()
    if V >= (3 if fuse else 2):
        o.begin_factored_views(V, gather=gather, sh_degree=3)
    if fuse:
        assert o.can_fuse_step()
        o.begin_fused_step()
    rows, folds = _run_views(o, V, fuse)
    assert o.direct_backwards == V
    if fuse:
        assert o.fused_update_launched and o.end_fused_step()
    else:
        o._begin_update("defer", False)
        o._after_step(False, True)
    assert o.direct_backwards == 0
    return rows, folds


_F, _T = False, True
_HAND_OFF_TABLE = {  # (V, fuse): (check_overflow, adam_fuse, accumulate, slot, fold) of every view
    (1, False): [(_F, _F, 0, None, _F)],
    (1, True): [(_T, _T, 0, None, _F)],
    (2, False): [(_F, _F, 0, 0, _F), (_F, _F, 1, 1, _F)],
    (2, True): [(_T, _F, 0, None, _F), (_T, _T, 1, None, _F)],
    (3, False): [(_F, _F, 0, 0, _F), (_F, _F, 1, 1, _F), (_F, _F, 1, 2, _F)],
    (3, True): [(_T, _F, 0, 0, _F), (_T, _F, 1, 1, _F), (_T, _T, 1, None, _T)],
}


@pytest.mark.parametrize("V,fuse", sorted(_HAND_OFF_TABLE))
def test_view_hand_off_table_over_two_consecutive_steps(V, fuse):
    """What FusedAdam.open_view tells the views of a V-view step, with the update carried by the last backward or as the
    separate pass: the same in two consecutive steps, except that the fused steps alternate between their two flag words."""
    o = _cpu_optimizer()
    for step in (0, 1):
        rows, folds = _step(o, V, fuse)
        flag = "fuse%d" % step if fuse else "state_dev[1]"
        assert rows == [r + (flag,) for r in _HAND_OFF_TABLE[V, fuse]], (step, rows)
        assert folds == ([0] if (V, fuse) == (3, True) else []), (step, folds)  # (into a buffer that holds nothing: assigned)
        assert o.fused_steps == (step + 1 if fuse else 0)


def test_view_hand_off_edge_cases():
    # gathered slots: filled in order, never folded by the rank itself
    o = _cpu_optimizer()
    rows, folds = _step(o, 2, False, gather=True)
    assert [r[2:5] for r in rows] == [(0, 0, _F), (1, 1, _F)] and folds == []
    assert o._views["next"] == 2 and o.fold_own_views_args() is None
    # somebody touched the gradient buffer before the step: the first view adds, and so does the fold
    o = _cpu_optimizer()
    o.flat_grad.add_(0)
    rows, folds = _step(o, 3, True)
    assert [r[2] for r in rows] == [1, 1, 1] and folds == [1] and rows[2][4]
    # a fused 3-view step that is aborted (a capacity guess overflowed) and redone without the fused update
    o = _cpu_optimizer()
    _step(o, 3, True)
    o.abort_step(fused_update_undone=True)
    assert (o.fused_steps, o.direct_backwards, o._views["next"]) == (0, 0, 0)
    rows, folds = _run_views(o, 3, False)
    assert rows == [r + ("state_dev[1]",) for r in _HAND_OFF_TABLE[3, False]] and folds == []
    # a deferred buffer written in place by somebody else
    o = _cpu_optimizer()
    _step(o, 1, False)
    o.flat_grad.add_(0)
    with pytest.raises(RuntimeError, match="written in place while its contents were undefined"):
        o.open_view(False, torch.zeros(3))
    # more views than slots
    o = _cpu_optimizer()
    o.begin_factored_views(1, gather=False, sh_degree=3)
    o.close_view(o.open_view(False, torch.zeros(3)))
    with pytest.raises(RuntimeError, match="more backward passes than view slots"):
        o.open_view(False, torch.zeros(3))


def test_concurrent_views_hand_each_other_the_event_behind_their_accumulating_kernels():
    o = _cpu_optimizer()
    first, second = object(), object()
    o.set_concurrent(True)
    h = o.open_view(False, torch.zeros(3))
    assert h.wait_event is None
    o.close_view(h, first)
    h = o.open_view(False, torch.zeros(3))
    assert h.wait_event is first
    o.close_view(h, second)
    o.set_concurrent(False)
    assert not o.concurrent and o.open_view(False, torch.zeros(3)).wait_event is None
    o._begin_update("defer", False)
    assert o._acc_event is None
