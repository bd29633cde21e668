"""Host logic of gaussianhaircut_amd.optim that needs no GPU: the ZeRO-1 range plan and the argument checks."""
import pytest
import torch

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
