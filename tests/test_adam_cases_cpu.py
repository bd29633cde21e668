"""The ground of the optimizer's per-element tests (tests/adam_cases.py), on the CPU: the threshold table is the sources',
the float64 model is torch.optim.Adam in float64 (a lagging group included), the host simulator's adam_update meets the bar,
the bar's constants are what the composed fp32 form measures, and every case sits where it claims to."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import adam_cases as ac
from tests import helpers as hp

CSRC = os.path.join(hp.ROOT, "gaussianhaircut_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_threshold_table_is_the_sources():
    adam, host = _src("ghr_adam.h"), _src("ghr_capi.hip")
    t = ac.THRESHOLDS
    assert re.search(r"^#define GHR_ADAM_MAX_GROUPS %d$" % t["GHR_ADAM_MAX_GROUPS"], adam, flags=re.M)
    assert re.search(r"^#define GHR_ADAM_BLOCKS %d$" % t["GHR_ADAM_BLOCKS"], host, flags=re.M)
    # the 256-thread block: launch bounds, strides and launches
    for kernel in ("k_adam_nan_flag", "k_adam", "k_adam_v4", "k_adam_fused_finish", "k_relay_rows"):
        assert re.search(r"__launch_bounds__\(%d\) %s\(" % (t["BLOCK"], kernel), adam), kernel
        assert re.search(r"ghr::%s, dim3\([^;]*\), dim3\(%d\)," % (kernel, t["BLOCK"]), host), kernel
    assert len(re.findall(r"\+= \(long long\)gridDim\.x \* (\d+)\)", adam)) == 5
    assert set(re.findall(r"\+= \(long long\)gridDim\.x \* (\d+)\)", adam)) == {str(t["BLOCK"])}
    assert len(re.findall(r"\(long long\)blockIdx\.x \* %d \+ threadIdx\.x" % t["BLOCK"], adam)) == 5
    # four elements per thread: quads of the v4 kernel and of the finish
    assert "const long long n4 = (a.n - a.begin) >> 2;" in adam and "const long long i = a.begin + %d * q;" % t["VEC"] in adam
    assert "const long long n4 = n >> 2;" in adam and "threadIdx.x < (n & 3)" in adam
    assert "const long long n4 = (count + 3) / %d;" % t["VEC"] in host
    # the grid caps: literals of the launches
    cap = r"const int blocks = \(int\)\(\(count \+ 255\) / 256 < (\d+) \? \(count \+ 255\) / 256 : (\d+)\);"
    found = re.findall(cap, host)
    assert found == [(str(t["ADAM_GRID"]),) * 2] * 2                       # adam_step_range (k_adam and its scan), ghr_adam_nan_scan
    assert "ghr::k_adam_nan_flag, dim3(blocks), dim3(256)" in host and "ghr::k_adam, dim3(blocks), dim3(256)" in host
    assert "const long long cap4 = GHR_ADAM_BLOCKS;" in host
    assert "const int blocks = (int)(blocks_ll < %d ? blocks_ll : %d);" % ((t["RELAY_GRID"],) * 2) in host
    assert "ghr::k_adam_fused_finish, dim3(%d), dim3(256)" % t["FINISH_GRID"] in host
    assert re.search(r"^#define GHR_ADAM_STATE %d\b" % ac.STATE_WORDS, open(os.path.join(hp.ROOT, "include", "ghr.h")).read(),
                     flags=re.M)
    assert (ac.SCALAR_TRIP, ac.FINISH_TRIP, ac.RELAY_TRIP, ac.V4_TRIP) == (1048576, 1048576, 4194304, 67108864)


def _torch_adam64(p, g, m, v, t, lr):
    """torch.optim.Adam in float64 on one tensor whose own step count stands at t - 1."""
    q = torch.nn.Parameter(torch.from_numpy(p.astype(np.float64)))
    opt = torch.optim.Adam([q], lr=float(np.float32(lr)), betas=(ac.BETA1, ac.BETA2), eps=float(np.float32(ac.EPS)))
    opt.state[q] = dict(step=torch.tensor(float(t - 1)), exp_avg=torch.from_numpy(m.astype(np.float64)),
                        exp_avg_sq=torch.from_numpy(v.astype(np.float64)))
    q.grad = torch.from_numpy(g.astype(np.float64))
    opt.step()
    st = opt.state[q]
    assert float(st["step"]) == t
    return q.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


@pytest.mark.parametrize("step_count", ac.STEP_COUNTS)
def test_model_step_is_torch_adam_in_float64(step_count):
    case = ac.GROUPS_CASE
    inp = ac.make_inputs(case)
    ends = case["ends"]
    state = ac.make_state(step_count, len(ends))
    skip = ac.SKIP_MASKS[1]
    ref = ac.model_step(inp["p"], inp["g"], inp["m"], inp["v"], ends, ac.LRS, state, skip_mask=skip, zero_grad=1)
    assert not ref["g"].any()
    lagging = 0
    lo = 0
    for gi, end in enumerate(ends):
        sl = slice(lo, end)
        lo = end
        if (skip >> gi) & 1:     # a parameter without a gradient: torch passes it by
            for k in ("p", "m", "v"):
                assert np.array_equal(ref[k][sl], inp[k][sl].astype(np.float64)) and not ref["moved"][sl].any()
            continue
        t = step_count + 1 - int(state[2 + gi])     # a separate optimizer per group: its step count lags by the group's own
        lagging += int(state[2 + gi] > 0)
        want = _torch_adam64(inp["p"][sl], inp["g"][sl], inp["m"][sl], inp["v"][sl], t, ac.LRS[gi])
        # in the bar's own scales (m' cancels where g is close to -9 m), at float64's precision: 1e-6 u = 6e-14
        d = ac.distances(dict(zip("pmv", want)), {k: ref[k][sl] for k in "pmv"}, {k: inp[k][sl] for k in inp})
        assert max(d.values()) < 1e-6, (gi, d)
        assert ref["moved"][sl].all()
    assert lagging >= (8 if step_count else 0)


def test_nothing_moves_under_the_flag_in_a_skipped_group_or_outside_the_range():
    case = ac.GROUPS_CASE
    inp = ac.make_inputs(case)
    state = ac.make_state(6, 16)
    a = (inp["p"], inp["g"], inp["m"], inp["v"], case["ends"], ac.LRS, state)
    up = ac.model_step(*a, flag=1, zero_grad=1)
    assert not up["moved"].any() and not up["g"].any() and all(np.array_equal(up[k], inp[k].astype(np.float64)) for k in "pmv")
    part = ac.model_step(*a, skip_mask=1 << 7, begin=5, count=2000, zero_grad=1)
    want = np.zeros(case["n"], bool)
    want[5:8] = True
    want[1031:2005] = True
    assert np.array_equal(part["moved"], want)
    assert np.array_equal(part["g"][:5], inp["g"][:5]) and np.array_equal(part["g"][2005:], inp["g"][2005:])
    assert not part["g"][5:2005].any()
    for k in "pmv":
        assert np.array_equal(part[k][~want], inp[k][~want].astype(np.float64))
        assert (part[k][want] != inp[k][want]).mean() > 0.5
    keep = ac.model_step(*a, zero_grad=0)
    assert np.array_equal(keep["g"], inp["g"])
    assert list(ac.model_state(state, 0b101, 16, 0)[:5]) == [7, 0, state[2] + 1, state[3], state[4] + 1]
    assert list(ac.model_state(state, 0b101, 16, 1)[:5]) == [6, 0, state[2], state[3], state[4]]
    assert np.array_equal(ac.model_state(state, 0b101, 16, 0, finish=False), state)


def test_inputs_are_normal_fp32_numbers_of_the_stated_kind():
    tiny = np.finfo(np.float32).tiny
    for case in ac.ALL_STEP_CASES[-2:]:
        inp = ac.make_inputs(case)
        for k, x in inp.items():
            assert x.dtype == np.float32 and x.shape == (case["n"],) and np.isfinite(x).all()
            assert ((x == 0) | (np.abs(x) >= tiny)).all(), k
        g = np.abs(inp["g"])
        assert 0.08 < (g == 0).mean() < 0.17
        decade = np.floor(np.log10(g[g > 0].astype(np.float64) * (1 + 1e-6))).astype(int)   # (fp32(1e-8) lies below 1e-8)
        assert set(decade.tolist()) == set(range(ac.K_MIN, ac.K_MAX + 1))
        assert (inp["v"] >= 0).all() and (inp["v"] == 0).mean() < 0.01 and (np.abs(inp["p"]) >= 2.0 ** -6).all()
        again = ac.make_inputs(case, np.arange(case["n"], dtype=np.int64)[7:19])
        assert all(np.array_equal(again[k], inp[k][7:19]) for k in inp)      # a value depends on index and seed only
    t = ac.make_inputs(ac.GROUPS_CASE, torch.arange(ac.N_GROUPS, dtype=torch.int64))
    ref = ac.make_inputs(ac.GROUPS_CASE)
    assert all(np.array_equal(t[k].numpy(), ref[k]) for k in ref)            # and the torch path fills the same bits


def test_bar_constants_are_what_the_composed_form_measures():
    worst = ac.measure_composed()
    print("composed fp32 form against model_step, worst distance in u:", worst)
    for k in ("m", "v", "p"):
        assert np.isfinite(worst[k]) and worst[k] < ac.BAR_CAP, (k, worst[k])
        assert ac.MEASURED[k] - 0.05 <= worst[k] <= ac.MEASURED[k], (k, worst[k], ac.MEASURED[k])
        assert ac.BAR[k] == 3.0 * ac.MEASURED[k]


def test_host_simulator_adam_update_meets_the_bar():
    sim = hp.HostSim().L
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    worst = dict(m=0.0, v=0.0, p=0.0)
    for case in (ac.GROUPS_CASE, dict(n=50000, ends=(50000,), seed=5)):
        inp = ac.make_inputs(case)
        ends = case["ends"]
        for sc in ac.STEP_COUNTS:
            state = ac.make_state(sc, len(ends))
            ref = ac.model_step(inp["p"], inp["g"], inp["m"], inp["v"], ends, ac.LRS, state, zero_grad=0)
            got = {k: inp[k].copy() for k in "pmv"}
            for gi, a, b in ac.group_slices(ends, 0, case["n"], 0):
                p, g, m, v = (x[a:b].copy() for x in (inp["p"], inp["g"], inp["m"], inp["v"]))   # updated in place
                sim.ghrsim_adam(b - a, ptr(p), ptr(g), ptr(m), ptr(v), ctypes.c_float(ac.LRS[gi]), ctypes.c_double(ac.BETA1),
                                ctypes.c_double(ac.BETA2), ctypes.c_float(ac.EPS), sc + 1 - int(state[2 + gi]))
                got["p"][a:b], got["m"][a:b], got["v"][a:b] = p, m, v
            d = ac.distances(got, ref, inp)
            worst = {k: max(worst[k], d[k]) for k in worst}
    print("host simulator against model_step, worst distance in u:", worst)
    for k in worst:
        assert worst[k] <= ac.BAR[k], (k, worst[k])


def test_the_bar_rejects_a_wrong_step_number_and_a_wrong_group():
    case = ac.GROUPS_CASE
    inp = ac.make_inputs(case)
    state = ac.make_state(6, 16)
    ref = ac.model_step(inp["p"], inp["g"], inp["m"], inp["v"], case["ends"], ac.LRS, state, zero_grad=0)
    sl = slice(8, 1031)                                       # group 7
    args = [inp[k][sl] for k in ("p", "g", "m", "v")]
    part = lambda d: {k: d[k][sl] for k in d if k != "moved"}
    t = 7 - int(state[2 + 7])
    assert state[2 + 7] > 0
    right = dict(zip("pmv", ac.composed_step(*args, t, ac.LRS[7])))
    d = ac.distances(right, part(ref), part(inp))
    assert all(d[k] <= ac.BAR[k] for k in d)
    no_lag = dict(zip("pmv", ac.composed_step(*args, 7, ac.LRS[7])))
    other = dict(zip("pmv", ac.composed_step(*args, t, ac.LRS[8])))
    for wrong in (no_lag, other):
        d = ac.distances(wrong, part(ref), part(inp))
        assert d["p"] > 100 * ac.BAR["p"] and d["m"] <= ac.BAR["m"] and d["v"] <= ac.BAR["v"]
    # a gradient of +-inf is not a NaN: the model's outputs there are inf, inf and NaN, and same_class tells them apart
    g = inp["g"].copy()
    g[[3, 2000]] = np.inf, -np.inf
    r = ac.model_step(inp["p"], g, inp["m"], inp["v"], case["ends"], ac.LRS, state)
    assert r["m"][3] == np.inf and r["m"][2000] == -np.inf and r["v"][3] == np.inf and np.isnan(r["p"][[3, 2000]]).all()
    assert np.isfinite(np.delete(r["p"], [3, 2000])).all()
    assert ac.same_class(r["m"].astype(np.float32), r["m"]) and not ac.same_class(-r["m"], r["m"])
    assert not ac.same_class(np.where(np.isnan(r["p"]), np.inf, r["p"]), r["p"])


def test_step_cases_sit_where_they_claim_to():
    t = ac.THRESHOLDS
    assert ac.SINGLE_N == (1, 2, 3, 4, 5) and [n // t["VEC"] for n in ac.SINGLE_N] == [0, 0, 0, 1, 1]
    ends = ac.ENDS_GROUPS
    assert len(ends) == t["GHR_ADAM_MAX_GROUPS"] == 16 and ends[-1] == ac.N_GROUPS == 4099 and list(ends) == sorted(set(ends))
    assert ends[:9] == (1, 2, 3, 5, 6, 7, 8, 1031, 1032)
    assert {e % 4 for e in ends} == {0, 1, 2, 3}
    q = ac.quad_groups(ends, 0, ac.N_GROUPS)
    assert q.size == 1024 and q[0] == 4 and q[1] == 4 and q[512] == 3 and (q == 2).sum() >= 3 and (q == 1).sum() > 1000
    sizes = np.diff((0,) + ends)
    assert (sizes == 1).sum() >= 8
    assert ends[14] == 4097 and 4096 < ends[14] < ac.N_GROUPS          # the v4 tail (4096 .. 4098) lies in two groups
    m1, m2 = ac.SKIP_MASKS[1], ac.SKIP_MASKS[2]
    assert m1 & 1 and m1 >> 15 & 1 and m1 >> 1 & 1 and not m1 >> 2 & 1 and m1 >> 5 & 1 and not m1 >> 4 & 1
    assert m2 >> 7 & 1 and sizes[7] > 1000 and m2 >> 14 & 1            # whole quads inside a skipped group; a skipped tail element
    for sc in ac.STEP_COUNTS:
        lag = ac.lags(sc, 16)
        assert max(lag) <= sc and (sc == 0 or len(set(lag)) >= min(sc, 6))
        assert (ac.make_state(sc, 3)[5:] == 77).all()
    # ranges: every (begin % 4, count % 4), inside one group and across many; one group exactly; empty ones
    inside = [(b, c) for b, c in ac.RANGES if 8 <= b and 0 < c and b + c <= 1031 and (b, c) != (8, 1023)]
    across = [(b, c) for b, c in ac.RANGES if b < 4 and b + c > 2051]
    for part in (inside, across):
        assert {(b % 4, c % 4) for b, c in part} >= {(i, j) for i in range(4) for j in range(4)}
    assert (8, 1023) in ac.RANGES and (ends[6], ends[7]) == (8, 1031) and (1031, 1) in ac.RANGES and (2050, 1) in ac.RANGES
    assert sum(c == 0 for _, c in ac.RANGES) == 3 and (0, ac.N_GROUPS) in ac.RANGES
    assert all(b + c <= ac.N_GROUPS for b, c in ac.RANGES)
    # the stride cases
    s = ac.STRIDE_SCALAR
    assert s["n"] - ac.SCALAR_TRIP == 256 + 3 and s["ends"] == (ac.SCALAR_TRIP - 1, ac.SCALAR_TRIP + 1, s["n"])
    assert (s["n"] + 255) // 256 > t["ADAM_GRID"] and s["n"] % 4 == 3
    v = ac.STRIDE_V4
    assert v["n"] - ac.V4_TRIP == 1024 + 3 and v["n"] % 4 == 3 and v["ends"][-1] == v["n"]
    assert ((v["n"] + 3) // 4 + 255) // 256 > t["GHR_ADAM_BLOCKS"] and v["ends"][0] < ac.V4_TRIP < v["ends"][1]
    assert ac.quad_groups((3, 6, 8), 0, 8).tolist() == [2, 2]
    n = s["n"]
    assert ac.NAN_AT == dict(first=0, last=n - 1, v4_tail=n - 2, second_trip=1048576 + 5, none=None)
    assert ac.NAN_AT["v4_tail"] >= (n // 4) * 4 and ac.NAN_AT["second_trip"] >= ac.SCALAR_TRIP
    assert ac.SCAN_COUNTS == (1, 63, 64, 65, 256, 257, 1048576, 1048577)
    assert ac.FINISH_N == (1, 3, 4, 5, 1048576, 1048579, 2098181) and ac.FINISH_N[-1] == 2 * ac.FINISH_TRIP + 1029
    assert ac.FINISH_N[-1] % 4 == 1 and ac.FINISH_N[-1] // 4 > 2 * t["FINISH_GRID"] * t["BLOCK"]


def test_relay_cases_sit_where_they_claim_to_and_the_model_is_the_stated_gather():
    assert set(ac.WIDTHS) == {1, 8, 16} and all(len(w) == g for g, w in ac.WIDTHS.items())
    assert set(ac.WIDTHS[16]) == {1, 3, 4, 45} and sum(ac.WIDTHS[8]) == 61
    big = ac.RELAY_BIG
    assert sum(ac.WIDTHS[big["groups"]]) * big["P_new"] == 4194421 == ac.RELAY_TRIP + 117
    for g in (8, 16):     # (300, 257): no group of the new layout ends on a workgroup's edge
        assert all(e % 256 for e in np.cumsum(ac.WIDTHS[g]) * 257)
    assert {(1, 1), (5, 3), (300, 257)} <= set(ac.RELAY_ROWS) and any(a < b for a, b in ac.RELAY_ROWS)
    for mode in ac.CHILD_MODES:
        c = ac.relay_case(16, 300, 257, mode, 3)
        assert len(set(c["take"].tolist())) < 257 and 0 < c["fresh"].sum() < 257
        outs = ac.model_relay(c["widths"], 300, 257, c["take"], c["fresh"], c["child"], c["overrides"], c["p_in"], c["m_in"],
                              c["v_in"])
        assert all(o.shape == (c["n_new"],) and o.dtype == np.float32 for o in outs)
        if mode == "null":
            assert c["child"] is None and c["overrides"] is None
        else:
            assert [o is not None for o in c["overrides"]] == [True] + [False] * 14 + [True]
            assert ((c["child"] >= 0).sum() > 50) == (mode == "two_groups")
        # the loop the comment above RelayArgs states, element by element
        off_old = off_new = 0
        for gi, w in enumerate(c["widths"]):
            for r in (0, 1, 128, 255, 256):
                src = off_old + c["take"][r] * w
                ch = -1 if c["child"] is None else c["child"][r]
                for col in range(w):
                    want = c["overrides"][gi][ch, col] if ch >= 0 and c["overrides"][gi] is not None else c["p_in"][src + col]
                    assert outs[0][off_new + r * w + col] == want
                    assert outs[1][off_new + r * w + col] == (0 if c["fresh"][r] else c["m_in"][src + col])
                    assert outs[2][off_new + r * w + col] == (0 if c["fresh"][r] else c["v_in"][src + col])
            off_old += w * 300
            off_new += w * 257
        if mode == "two_groups":
            assert (outs[0] >= 1000).sum() == (c["child"] >= 0).sum() * (c["widths"][0] + c["widths"][15])
    outs, state, nxt = ac.model_finish(1, ac.make_state(6, 8), [np.ones(3)] * 3, [np.zeros(3)] * 3)
    assert all((o == 1).all() for o in outs) and state[0] == 6 and nxt == 0
    outs, state, nxt = ac.model_finish(0, ac.make_state(6, 8), [np.ones(3)] * 3, [np.zeros(3)] * 3)
    assert all((o == 0).all() for o in outs) and state[0] == 7 and nxt == 0
