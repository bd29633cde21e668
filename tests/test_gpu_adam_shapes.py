"""`-m gpu`: the kernels of csrc/ghr_adam.h through the C ABI, per element against the float64 model of tests/adam_cases.py:
every form of the step (in place, a range, a range out of place) on both kernels (the scalar one forced by GHR_ADAM_SCALAR
and by base pointers 4 bytes off a 16-B boundary), group ends at every residue mod 4, skipped and lagging groups, ranges at
every (begin % 4, count % 4), the grid-stride loops' second trips, the NaN guard, scan and mark, the re-lay of a
densification event and the finish of a fused step.  Every device buffer is a payload between two guards; what must not
change is compared by bits."""
import ctypes

import numpy as np
import pytest
import torch

from gaussianhaircut_amd import _lib
from tests import adam_cases as ac

pytestmark = pytest.mark.gpu

GUARD_B = 256                # bytes on either side of every payload (keeps the allocation's 16-B alignment)
FILL = 0xA5
KERNELS = ("v4", "scalar_env", "scalar_off")
WORST = dict(m=0.0, v=0.0, p=0.0)        # the kernels' worst distance from the model over everything this module ran
_INPUTS = {}


def _dev():
    return torch.device("cuda:0")


def _poison(n):
    return np.full(n, np.nan, np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


class Buf:
    """a payload (numpy array or device tensor, any dtype) between two guards of FILL bytes; `off`: bytes the payload is
    shifted by (4: off the 16-B alignment the vector kernel needs)"""

    def __init__(self, payload, off=0):
        t = (payload if isinstance(payload, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(payload))).reshape(-1)
        self.nbytes = t.numel() * t.element_size()
        self.lo = GUARD_B + off
        self.buf = torch.full((self.lo + self.nbytes + GUARD_B,), FILL, dtype=torch.uint8, device=_dev())
        self.t = self.buf[self.lo:self.lo + self.nbytes].view(t.dtype) if t.numel() else torch.zeros(0, dtype=t.dtype, device=_dev())
        self.t.copy_(t)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + self.lo)

    def dev(self):
        """the payload on the device, after the guards were found intact"""
        torch.cuda.synchronize()
        assert bool((self.buf[:self.lo] == FILL).all()), "the guard below the payload was written"
        assert bool((self.buf[self.lo + self.nbytes:] == FILL).all()), "the guard above the payload was written"
        return self.t

    def get(self):
        return self.dev().cpu().numpy().copy()


def _inputs(case):
    key = (case["n"], case["seed"])
    if key not in _INPUTS:
        _INPUTS[key] = ac.make_inputs(case)
    return {k: v.copy() for k, v in _INPUTS[key].items()}


def _tables(ends):
    return (ctypes.c_int64 * len(ends))(*ends), (ctypes.c_float * len(ends))(*ac.LRS[:len(ends)])


def _select(monkeypatch, kernel):
    if kernel == "scalar_env":
        monkeypatch.setenv("GHR_ADAM_SCALAR", "1")
    else:
        monkeypatch.delenv("GHR_ADAM_SCALAR", raising=False)
    return 4 if kernel == "scalar_off" else 0


def call_step(monkeypatch, kernel, form, inp, ends, state, skip_mask=0, begin=0, count=None, nan_guard=0, zero_grad=1, last=1,
              nan_mark=0, flag_word=None):
    """One call of ghr_adam_step ("step"), ghr_adam_step_range ("range") or ghr_adam_step_range_to ("range_to"; flag_word:
    the value of a flag word of its own, None: state[1] is the flag) on fresh guarded buffers; everything read back."""
    L = _lib.lib()
    off = _select(monkeypatch, kernel)
    n, G = inp["p"].size, len(ends)
    count = n - begin if count is None else count
    ends_c, lrs_c = _tables(ends)
    b = {k: Buf(inp[k], off) for k in "pgmv"}
    sb = Buf(np.asarray(state, np.int32))
    tail = (G, ends_c, lrs_c, ac.BETA1, ac.BETA2, ac.EPS)
    res = {}
    if form == "step":
        assert begin == 0 and count == n
        rc = L.ghr_adam_step(None, n, b["p"].ptr, b["g"].ptr, b["m"].ptr, b["v"].ptr, sb.ptr, *tail, nan_guard, zero_grad, skip_mask)
    elif form == "range":
        rc = L.ghr_adam_step_range(None, n, begin, count, b["p"].ptr, b["g"].ptr, b["m"].ptr, b["v"].ptr, sb.ptr, *tail, nan_guard,
                                   zero_grad, last, skip_mask)
    else:
        outs = {k: Buf(_poison(n), off) for k in "pmv"}
        fw = None if flag_word is None else Buf(np.array([flag_word], np.int32))
        rc = L.ghr_adam_step_range_to(None, n, begin, count, b["p"].ptr, b["m"].ptr, b["v"].ptr, outs["p"].ptr, b["g"].ptr,
                                      outs["m"].ptr, outs["v"].ptr, sb.ptr, None if fw is None else fw.ptr, nan_mark, *tail,
                                      zero_grad, skip_mask)
    _lib.check(rc)
    if form == "range_to":
        for k in "pmv":
            assert _same_bits(b[k].get(), inp[k]), "the `in` set was written"
            res[k] = outs[k].get()
        res["flag_word"] = None if fw is None else int(fw.get()[0])
    else:
        for k in "pmv":
            res[k] = b[k].get()
    res["g"], res["state"] = b["g"].get(), sb.get()
    return res


def check_step(res, inp, ref, state_after, form, begin, count, what):
    """Untouched and copied elements, the gradient and the state words by bits; the moved elements under the bar."""
    moved = ref["moved"]
    in_range = np.zeros(moved.size, bool)
    in_range[begin:begin + count] = True
    for k in "pmv":
        if form == "range_to":
            assert np.isnan(res[k][~in_range]).all() and _same_bits(res[k][~in_range], _poison(int((~in_range).sum()))), \
                (what, k, "written outside the range")
            assert _same_bits(res[k][in_range & ~moved], inp[k][in_range & ~moved]), (what, k, "not copied")
        else:
            assert _same_bits(res[k][~moved], inp[k][~moved]), (what, k, "an element that takes no update changed")
        assert ac.same_class(res[k][moved], ref[k][moved]), (what, k, "non-finite class")
    assert _same_bits(res["g"], ref["g"]), (what, "gradient")
    assert np.array_equal(res["state"], state_after), (what, res["state"], state_after)
    d = ac.distances({k: res[k][moved] for k in "pmv"}, {k: ref[k][moved] for k in "pmv"}, {k: inp[k][moved] for k in inp})
    for k in d:
        assert d[k] <= ac.BAR[k], (what, k, d[k], ac.BAR[k])
        WORST[k] = max(WORST[k], d[k])
    return d


def _three_kernels(monkeypatch, form, inp, ends, state, what, vector_applies=True, **kw):
    """The call on the vector kernel and on the scalar one forced both ways: all three checked, and the same bits."""
    n = inp["p"].size
    begin = kw.get("begin", 0)
    count = kw.get("count", None)
    count = n - begin if count is None else count
    flag_word = kw.get("flag_word")
    flag = flag_word if flag_word is not None else int(state[1])
    ref = ac.model_step(inp["p"], inp["g"], inp["m"], inp["v"], ends, ac.LRS, state, kw.get("skip_mask", 0), flag, begin, count,
                        ac.BETA1, ac.BETA2, ac.EPS, kw.get("zero_grad", 1))
    finish = form == "step" or (form == "range" and kw.get("last", 1) != 0)
    after = ac.model_state(state, kw.get("skip_mask", 0), len(ends), int(state[1]), finish=finish)
    runs = []
    for kernel in KERNELS:
        res = call_step(monkeypatch, kernel, form, inp, ends, state, **kw)
        check_step(res, inp, ref, after, form, begin, count, (what, kernel))
        if form == "range_to":
            assert res["flag_word"] == flag_word, (what, kernel, "the flag word")
        runs.append(res)
    for other in runs[1:]:
        for k in ("p", "m", "v", "g"):
            assert _same_bits(runs[0][k], other[k]), (what, k, "scalar and vector kernel differ")
    return ref


# ---- the step, small ------------------------------------------------------------------------------------------------------------
def test_step_in_place_single_groups_and_sixteen_groups(monkeypatch):
    n_calls = 0
    for case in [ac.single_case(n) for n in ac.SINGLE_N] + [ac.GROUPS_CASE]:
        inp, ends = _inputs(case), case["ends"]
        small = len(ends) == 1
        for sc in ((6,) if small else ac.STEP_COUNTS):
            for mask in ((0, 1) if small else ac.SKIP_MASKS):
                for zero_grad in (0, 1):
                    for flag in (0, 1):
                        for nan_guard in (0, 1, 2):
                            state = ac.make_state(sc, len(ends), flag)
                            ref = _three_kernels(monkeypatch, "step", inp, ends, state,
                                                 (case["n"], sc, mask, zero_grad, flag, nan_guard), skip_mask=mask,
                                                 nan_guard=nan_guard, zero_grad=zero_grad)
                            assert ref["moved"].any() == (not flag and not (small and mask))
                            n_calls += 3
    print("in place: %d calls, worst distance so far (u): %s" % (n_calls, WORST))


def test_step_range_at_every_begin_and_count_residue(monkeypatch):
    case = ac.GROUPS_CASE
    inp, ends = _inputs(case), case["ends"]
    i = 0
    for begin, count in ac.RANGES:
        for zero_grad in (0, 1):
            for flag in (0, 1):
                whole = (begin, count) == (0, case["n"])
                for nan_guard in ((0, 1, 2) if whole else ((0, 2)[i % 2],)):
                    sc, mask, last = ac.STEP_COUNTS[i % 3], ac.SKIP_MASKS[(i // 3) % 3], (i // 2) % 2
                    state = ac.make_state(sc, len(ends), flag)
                    _three_kernels(monkeypatch, "range", inp, ends, state, (begin, count, zero_grad, flag, nan_guard, sc, mask, last),
                                   skip_mask=mask, begin=begin, count=count, nan_guard=nan_guard, zero_grad=zero_grad, last=last)
                    i += 1
    print("ranges in place: %d configurations, worst distance so far (u): %s" % (i, WORST))


def test_step_range_out_of_place_at_every_begin_and_count_residue(monkeypatch):
    case = ac.GROUPS_CASE
    inp, ends = _inputs(case), case["ends"]
    i = 0
    for begin, count in ac.RANGES:
        for zero_grad in (0, 1):
            for flag in (0, 1):
                sc, mask, nan_mark = ac.STEP_COUNTS[i % 3], ac.SKIP_MASKS[(i // 3) % 3], (i // 2) % 2
                own_word = bool(nan_mark) or i % 3 != 0          # else: state[1] is the flag (flag == NULL)
                state = ac.make_state(sc, len(ends), 0 if own_word else flag)
                _three_kernels(monkeypatch, "range_to", inp, ends, state, (begin, count, zero_grad, flag, nan_mark, sc, mask, own_word),
                               skip_mask=mask, begin=begin, count=count, zero_grad=zero_grad, nan_mark=nan_mark,
                               flag_word=flag if own_word else None)
                i += 1
    print("ranges out of place: %d configurations, worst distance so far (u): %s" % (i, WORST))


def test_infinite_gradient_is_not_a_nan(monkeypatch):
    """g = +-inf: the guard stays down (the step is taken, the counter advances, a flag word of its own stays 0) and m', v',
    p' are of the model's class there -- +-inf, inf, NaN -- and within the bar everywhere else."""
    case = ac.GROUPS_CASE
    inp, ends = _inputs(case), case["ends"]
    inp["g"][[3, 2000, 4098]] = np.inf, -np.inf, np.inf
    state = ac.make_state(6, len(ends))
    ref = _three_kernels(monkeypatch, "step", inp, ends, state, "inf, scanning guard", nan_guard=1)
    assert np.isnan(ref["p"][[3, 2000, 4098]]).all() and np.isinf(ref["m"][[3, 2000, 4098]]).all() and ref["moved"].all()
    _three_kernels(monkeypatch, "range_to", inp, ends, state, "inf, nan_mark", nan_mark=1, flag_word=0)


# ---- the step, second trips ----------------------------------------------------------------------------------------------------------
def test_scalar_kernel_takes_a_second_trip(monkeypatch):
    """n = 4096 * 256 + 259 with group ends on either side of the first trip's end: k_adam's grid-stride loop (and the
    scan's) goes round again; against the model per element, and the vector kernel gives the same bits."""
    case = ac.STRIDE_SCALAR
    inp, ends = _inputs(case), case["ends"]
    state = ac.make_state(6, len(ends))
    ref = ac.model_step(inp["p"], inp["g"], inp["m"], inp["v"], ends, ac.LRS, state)
    after = ac.model_state(state, 0, len(ends), 0)
    runs = {}
    for kernel in ("scalar_env", "v4"):
        runs[kernel] = call_step(monkeypatch, kernel, "step", inp, ends, state, nan_guard=1)
        d = check_step(runs[kernel], inp, ref, after, "step", 0, case["n"], kernel)
        print("second trip of %s: distance (u) %s" % (kernel, d))
    for k in ("p", "m", "v", "g"):
        assert _same_bits(runs["v4"][k], runs["scalar_env"][k]), k


def test_vector_kernel_takes_a_second_trip(monkeypatch):
    """n = 65536 * 1024 + 1027, in place: k_adam_v4's loop goes round again (so does the scan's, 64 times).  Inputs and the
    float64 model on the device; only the worst distance and the mismatch counts come back."""
    case = ac.STRIDE_V4
    n, ends = case["n"], case["ends"]
    L = _lib.lib()
    inp = ac.make_inputs(case, torch.arange(n, dtype=torch.int64, device=_dev()))
    state = ac.make_state(6, len(ends))
    ends_c, lrs_c = _tables(ends)
    runs = {}
    for kernel in ("v4", "scalar_env"):
        _select(monkeypatch, kernel)
        b = {k: Buf(inp[k]) for k in "pgmv"}
        sb = Buf(state)
        _lib.check(L.ghr_adam_step(None, n, b["p"].ptr, b["g"].ptr, b["m"].ptr, b["v"].ptr, sb.ptr, len(ends), ends_c, lrs_c, ac.BETA1,
                                   ac.BETA2, ac.EPS, 1, 1, 0))
        runs[kernel] = dict({k: b[k].dev() for k in "pgmv"}, state=sb.get())
        assert np.array_equal(runs[kernel]["state"], ac.model_state(state, 0, len(ends), 0))
        assert int(torch.count_nonzero(runs[kernel]["g"].view(torch.int32))) == 0
    for k in "pmv":
        assert torch.equal(runs["v4"][k].view(torch.int32), runs["scalar_env"][k].view(torch.int32)), k
    got = runs["v4"]
    worst = dict(m=0.0, v=0.0, p=0.0)
    chunk = 1 << 24
    for gi, a, b_ in ac.group_slices(ends, 0, n, 0):
        t = int(state[0]) + 1 - int(state[2 + gi])
        for lo in range(a, b_, chunk):
            sl = slice(lo, min(lo + chunk, b_))
            part = {k: inp[k][sl] for k in "pgmv"}
            rp, rm, rv = ac.update64(*[part[k].double() for k in "pgmv"], t, ac.LRS[gi], ac.BETA1, ac.BETA2, ac.EPS)
            assert bool(torch.isfinite(rp).all()) and all(bool(torch.isfinite(got[k][sl]).all()) for k in "pmv")
            d = ac.distances({k: got[k][sl] for k in "pmv"}, dict(p=rp, m=rm, v=rv), part)
            worst = {k: max(worst[k], d[k]) for k in worst}
    print("second trip of v4, %d elements: distance (u) %s" % (n, worst))
    for k in worst:
        assert worst[k] <= ac.BAR[k], (k, worst[k])
        WORST[k] = max(WORST[k], worst[k])


# ---- NaN: guard, mark, scan ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", list(ac.NAN_AT))
def test_scanning_guard_finds_one_nan_wherever_it_is(where, monkeypatch):
    """nan_guard = 1 on n = 4096 * 256 + 259: nothing moves, state[0] stays, state[1] ends 0, the gradient is cleared --
    for a NaN in the first element, the last, the vector kernel's tail and the scan's second trip; none: the step is taken."""
    case = ac.STRIDE_SCALAR
    inp, ends = _inputs(case), case["ends"]
    at = ac.NAN_AT[where]
    if at is not None:
        inp["g"][at] = np.nan
    state = ac.make_state(6, len(ends))
    for kernel in ("v4", "scalar_env"):
        for zero_grad in (1, 0):
            res = call_step(monkeypatch, kernel, "step", inp, ends, state, nan_guard=1, zero_grad=zero_grad)
            assert res["state"][1] == 0 and np.array_equal(res["state"][2:], state[2:])
            assert _same_bits(res["g"], np.zeros_like(inp["g"]) if zero_grad else inp["g"])
            if at is None:
                assert res["state"][0] == 7 and not any((res[k] == inp[k]).all() for k in "pmv")
            else:
                assert res["state"][0] == 6, (where, kernel, "the step counter advanced")
                for k in "pmv":
                    assert _same_bits(res[k], inp[k]), (where, kernel, k, "moved under a NaN")


def test_nan_mark_rises_only_for_a_nan_inside_the_range(monkeypatch):
    case = ac.GROUPS_CASE
    ends = case["ends"]
    state = ac.make_state(6, len(ends))
    for begin, count in ((0, 4099), (100, 43), (101, 42), (8, 1023), (1031, 1), (4096, 3), (3, 5), (2, 2057)):
        spots = [(begin, 1), (begin + count - 1, 1), (begin + count // 2, 1)]
        spots += [(begin - 1, 0)] if begin > 0 else []
        spots += [(begin + count, 0)] if begin + count < case["n"] else []
        for at, want in spots + [(None, 0)]:
            inp = _inputs(case)
            if at is not None:
                inp["g"][at] = np.nan
            for kernel in KERNELS:
                res = call_step(monkeypatch, kernel, "range_to", inp, ends, state, begin=begin, count=count, nan_mark=1,
                                zero_grad=0, flag_word=0)
                assert res["flag_word"] == want, (begin, count, at, kernel)
                assert np.array_equal(res["state"], state) and _same_bits(res["g"], inp["g"])
    # without nan_mark the word is left alone, NaN or not; a word that is up stays up
    inp = _inputs(case)
    inp["g"][150] = np.nan
    for kernel in KERNELS:
        assert call_step(monkeypatch, kernel, "range_to", inp, ends, state, begin=100, count=100, flag_word=0)["flag_word"] == 0
        assert call_step(monkeypatch, kernel, "range_to", inp, ends, state, begin=100, count=100, nan_mark=1,
                         flag_word=1)["flag_word"] == 1


@pytest.mark.parametrize("count", ac.SCAN_COUNTS)
def test_nan_scan_alone(count):
    """ghr_adam_nan_scan: state[1] |= any(isnan(g[0 .. count))), the other words untouched.  The element after the scanned
    ones IS a NaN: a scan one element too far raises the word in the clean cases."""
    L = _lib.lib()
    g = (1.0 + np.arange(count + 1) % 1021).astype(np.float32)
    g[count] = np.nan
    state = (100 + np.arange(ac.STATE_WORDS)).astype(np.int32)
    for at, before, want in ((None, 0, 0), (count - 1, 0, 1), (0, 0, 1), (None, 1, 1), (count - 1, 1, 1)):
        gg, st = g.copy(), state.copy()
        if at is not None:
            gg[at] = np.nan
        st[1] = before
        gb, sb = Buf(gg), Buf(st)
        _lib.check(L.ghr_adam_nan_scan(None, gb.ptr, count, sb.ptr))
        got = sb.get()
        assert got[1] == want, (count, at, before, int(got[1]))
        st[1] = want
        assert np.array_equal(got, st), "another state word changed"
        assert _same_bits(gb.get(), gg)
    gb, sb = Buf(g), Buf(state)       # an empty scan is a no-op
    _lib.check(L.ghr_adam_nan_scan(None, gb.ptr, 0, sb.ptr))
    assert np.array_equal(sb.get(), state)


# ---- ghr_adam_relay_rows ----------------------------------------------------------------------------------------------------------
def call_relay(c):
    L = _lib.lib()
    G = len(c["widths"])
    take, fresh = Buf(c["take"]), Buf(c["fresh"])
    child = None if c["child"] is None else Buf(c["child"])
    ovr, keep = (ctypes.c_void_p * G)(), []
    for gi, o in enumerate(c["overrides"] or []):
        if o is not None:
            keep.append(Buf(o))
            ovr[gi] = keep[-1].ptr.value
    ins = [Buf(c[k]) for k in ("p_in", "m_in", "v_in")]
    outs = [Buf(_poison(c["n_new"])) for _ in range(3)]
    rc = L.ghr_adam_relay_rows(None, G, (ctypes.c_int32 * G)(*c["widths"]), c["P_old"], c["P_new"], take.ptr, fresh.ptr,
                               None if child is None else child.ptr, ctypes.cast(ovr, ctypes.c_void_p) if keep else None,
                               *[x.ptr for x in ins], *[x.ptr for x in outs])
    _lib.check(rc)
    got = [x.get() for x in outs]
    for x, k in zip(ins, ("p_in", "m_in", "v_in")):
        assert _same_bits(x.get(), c[k])
    for x in keep + [take, fresh] + ([child] if child is not None else []):
        x.dev()
    return got


def check_relay(c, what):
    got = call_relay(c)
    want = ac.model_relay(c["widths"], c["P_old"], c["P_new"], c["take"], c["fresh"], c["child"], c["overrides"], c["p_in"],
                          c["m_in"], c["v_in"])
    for name, a, b in zip("pmv", got, want):
        bad = np.nonzero(_bits(a) != _bits(b))[0]
        assert bad.size == 0, (what, name, bad.size, "first at", int(bad[0]), float(a[bad[0]]), float(b[bad[0]]))


@pytest.mark.parametrize("child_mode", ac.CHILD_MODES)
@pytest.mark.parametrize("groups", sorted(ac.WIDTHS))
def test_relay_rows_is_the_stated_gather(groups, child_mode):
    for i, (P_old, P_new) in enumerate(ac.RELAY_ROWS):
        check_relay(ac.relay_case(groups, P_old, P_new, child_mode, 10 * groups + i), (groups, child_mode, P_old, P_new))
    # an empty result: OK, and nothing is written
    c = ac.relay_case(groups, 5, 0, child_mode, 7)
    assert c["n_new"] == 0
    c["n_new"] = 64                  # output buffers that must keep their poison
    got = call_relay(c)
    assert all(_same_bits(g, _poison(64)) for g in got)


def test_relay_rows_takes_a_second_trip():
    """61 floats per row, 68 761 new rows: 4 194 421 elements, 117 past what 16 384 workgroups cover in one trip."""
    big = ac.RELAY_BIG
    c = ac.relay_case(big["groups"], big["P_old"], big["P_new"], "two_groups", 99)
    assert c["n_new"] == ac.RELAY_TRIP + 117
    check_relay(c, "second trip")


# ---- ghr_adam_fused_finish ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ac.FINISH_N)
def test_fused_finish_copies_under_the_flag_and_keeps_the_books(n):
    L = _lib.lib()
    idx = torch.arange(n, device=_dev())
    ins_t = [((idx % 8191).float() / 8192.0 + k).contiguous() for k in (1.0, 10.0, 20.0)]
    ends_c, lrs_c = _tables((n,))
    state = ac.make_state(6, 8)
    for flag in (0, 1):
        ins, outs = [Buf(t) for t in ins_t], [Buf(torch.full((n,), float("nan"), device=_dev())) for _ in range(3)]
        sb, fb = Buf(state), Buf(np.array([flag, 55], np.int32))
        af = _lib.AdamFuse()
        af.n = n
        af.p_in, af.m_in, af.v_in = (x.ptr.value for x in ins)
        af.p_out, af.m_out, af.v_out = (x.ptr.value for x in outs)
        af.state, af.flag, af.flag_next = sb.ptr.value, fb.ptr.value, fb.ptr.value + 4
        af.n_groups, af.group_end_host, af.lr_host = 1, ctypes.addressof(ends_c), ctypes.addressof(lrs_c)
        af.beta1, af.beta2, af.eps = ac.BETA1, ac.BETA2, ac.EPS
        _lib.check(L.ghr_adam_fused_finish(None, ctypes.byref(af)))
        _, want_state, want_next = ac.model_finish(flag, state, [0, 0, 0], [1, 1, 1])   # (the buffers are compared on the device)
        assert np.array_equal(sb.get(), want_state) and want_state[0] == 7 - flag
        assert list(fb.get()) == [flag, want_next], "flag word / flag_next"
        for i, o, src in zip(ins, outs, ins_t):
            assert torch.equal(i.dev().view(torch.int32), src.view(torch.int32)), "the `in` set was written"
            got = o.dev().view(torch.int32)
            if flag:
                bad = int((got != src.view(torch.int32)).sum())
                assert bad == 0, (n, bad, "elements not copied")
            else:
                assert bool((got == 0x7FC00000).all()), (n, "the `out` set lost its poison")


def test_zz_report_the_worst_distance():
    """(runs last in the module) the kernels' own worst distance from the model, for tests/adam_cases.KERNEL_MEASURED"""
    print("kernels against model_step, worst distance in u:", WORST)
    for k in WORST:
        assert WORST[k] <= ac.BAR[k]
