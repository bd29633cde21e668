"""Cases, thresholds and a plain float64 model of csrc/ghr_adam.h (k_adam, k_adam_v4, k_adam_nan_flag, k_adam_finish,
k_adam_fused_finish, k_relay_rows) for tests/test_adam_cases_cpu.py (the cases' own ground, on the CPU) and
tests/test_gpu_adam_shapes.py (the kernels through the C ABI, per element, between guards).

Nothing here calls project kernel code.  ``model_step`` is ONE kernel call in float64 from the same fp32 inputs (not a
float64 chain carried across steps); ``model_relay`` is the gather the comment above RelayArgs states; ``model_finish`` the
books of k_adam_fused_finish.  The grid caps the stride cases sit on are kept in ``THRESHOLDS``; the CPU test reads the
literals and ``#define``s out of ghr_adam.h and ghr_capi.hip and compares, so a changed cap fails there instead of moving a
boundary out of the cases.

Inputs (``make_inputs``) are seeded by an integer hash of the element index (the same code runs on numpy arrays and on
device tensors, so the 67 M-element case is filled where it is used): gradients of magnitude 10^k, k in -8 .. 3, with exact
zeros mixed in; the moments come from HISTORY fp32 steps started at zero, as in training (a large m over a tiny v would only
amplify rounding); every value is zero or a normal fp32 number.

The per-element bar, in units of u = 2^-24:
    |m' - ref| <= A_M u (|m| + (1 - beta1) |g|)      |v' - ref| <= A_V u |ref|      |p' - ref| <= A_P u (|ref| + |ref - p|)
The constants are three times the worst distance of the COMPOSED fp32 form (the operations of torch's _single_tensor_adam
in its order, numpy float32) from ``model_step`` over ALL_STEP_CASES below at every step count of the tests -- every step
case but the 67 M-element one, which is the same generator at more indices (tests/test_adam_cases_cpu.py measures it again
and compares); the margin is for the device's divide and square root and for another association of the same products.
    composed form, worst distance (CPU):   m 2.79 u    v 3.51 u    p 2.32 u        (MEASURED)
    the bars:                              m 8.37 u    v 10.53 u   p 6.96 u        (BAR)
    kernels on the MI355X, worst distance: m 2.87 u    v 3.58 u    p 2.32 u        (KERNEL_MEASURED)
The kernels' figures up to 1 048 835 elements are the composed form's to the last digit printed (m 2.79, v 3.51, p 2.32:
the library is built with -ffp-contract=off, divide and square root are correctly rounded); 2.87 and 3.58 are elements of
the 67 M case.  The fp32 casts of 1 - beta1 and beta2 alone are worth up to 1 u of these."""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24

# ---- launch shapes (names as in the sources where they have one) --------------------------------------------------------
THRESHOLDS = dict(
    ADAM_GRID=4096,              # k_adam, k_adam_nan_flag: workgroups at most (literal in ghr_capi.hip)
    FINISH_GRID=1024,            # k_adam_fused_finish: workgroups, always (literal)
    RELAY_GRID=16384,            # k_relay_rows: workgroups at most (literal)
    GHR_ADAM_BLOCKS=65536,       # k_adam_v4: workgroups at most
    BLOCK=256,                   # threads of a workgroup, every kernel here
    VEC=4,                       # elements per thread and trip in k_adam_v4 and k_adam_fused_finish
    GHR_ADAM_MAX_GROUPS=16,
)
SCALAR_TRIP = THRESHOLDS["ADAM_GRID"] * THRESHOLDS["BLOCK"]                           # 1 048 576 elements
FINISH_TRIP = THRESHOLDS["FINISH_GRID"] * THRESHOLDS["BLOCK"] * THRESHOLDS["VEC"]     # 1 048 576
RELAY_TRIP = THRESHOLDS["RELAY_GRID"] * THRESHOLDS["BLOCK"]                           # 4 194 304
V4_TRIP = THRESHOLDS["GHR_ADAM_BLOCKS"] * THRESHOLDS["BLOCK"] * THRESHOLDS["VEC"]     # 67 108 864
STATE_WORDS = 2 + THRESHOLDS["GHR_ADAM_MAX_GROUPS"]

BETA1, BETA2, EPS = 0.9, 0.999, 1e-15
MEASURED = dict(m=2.79, v=3.51, p=2.32)         # composed fp32 form against model_step, worst over ALL_STEP_CASES, in u
BAR = {k: 3.0 * x for k, x in MEASURED.items()}
KERNEL_MEASURED = dict(m=2.87, v=3.58, p=2.32)   # the kernels' own worst distance on the MI355X (tests/test_gpu_adam_shapes.py)
BAR_CAP = 16.0                                   # a measured constant beyond this is a finding, not a bar


# ---- inputs -----------------------------------------------------------------------------------------------------------------
HISTORY = 3                                      # fp32 steps from zero moments before the step under test
K_MIN, K_MAX = -8, 3
_POW10 = [10.0 ** k for k in range(K_MIN, K_MAX + 1)]
_M32 = 0xFFFFFFFF


def _hash(idx, salt):
    """32 well-mixed bits per index (an int64 numpy array or torch tensor; wrap-around products are fine in both)."""
    x = (idx + (salt * 0x9E3779B1 & _M32)) & _M32
    x = ((x ^ (x >> 16)) * 0x7FEB352D) & _M32
    x = ((x ^ (x >> 15)) * 0x846CA68B) & _M32
    return x ^ (x >> 16)


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _f64(x):
    if _is_torch(x):
        import torch
        return x.to(torch.float64)
    return x.astype(np.float64)


def _f32(x):
    if _is_torch(x):
        import torch
        return x.to(torch.float32)
    return x.astype(np.float32)


def _take(table, k):
    if _is_torch(k):
        import torch
        return torch.tensor(table, dtype=torch.float64, device=k.device)[k]
    return np.asarray(table, np.float64)[k]


def gradient(idx, seed, step):
    """fp32 gradient of the elements `idx` at history step `step`: sign * (1 + j / 256) * 10^k, one in eight exactly zero.
    k stays within a decade of the element's own level, like a parameter's gradient over neighbouring iterations."""
    base = _hash(idx, 3 * seed + 1) % (K_MAX - K_MIN + 1)
    h = _hash(idx, 1000003 * (step + 1) + seed)
    k = base + (h >> 3) % 3 - 1
    k = (k + abs(k)) // 2                                       # max(k, 0)
    top = K_MAX - K_MIN
    k = top - ((top - k) + abs(top - k)) // 2                   # min(k, top)
    mag = (1.0 + _f64((h >> 8) & 0xFF) / 256.0) * _take(_POW10, k)
    sign = 1.0 - 2.0 * _f64((h >> 5) & 1)
    live = _f64((h & 7) != 0)
    return _f32(sign * mag * live)


def parameter(idx, seed):
    """fp32 parameter values in +-[2^-6, 4)."""
    h = _hash(idx, 7 * seed + 5)
    mag = (1.0 + _f64(h & 0xFFFF) / 65536.0) * _take([2.0 ** e for e in range(-6, 2)], (h >> 16) & 7)
    return _f32((1.0 - 2.0 * _f64((h >> 20) & 1)) * mag)


def make_inputs(case, idx=None):
    """dict(p, g, m, v) of fp32 arrays for a case (a dict with `n` and `seed`).  `idx`: the int64 element indices, a numpy
    array (default: all n) or a device tensor -- the values depend on the index and the seed only."""
    if idx is None:
        idx = np.arange(case["n"], dtype=np.int64)
    seed = case["seed"]
    w1 = float(np.float32(1.0 - BETA1))
    w2 = float(np.float32(1.0 - BETA2))
    b2 = float(np.float32(BETA2))
    if not _is_torch(idx):
        w1, w2, b2 = np.float32(w1), np.float32(w2), np.float32(b2)
    m = v = None
    for s in range(HISTORY):
        g = gradient(idx, seed, s)
        m = g * w1 if m is None else m + (g - m) * w1
        v = g * g * w2 if v is None else v * b2 + g * g * w2
    return dict(p=parameter(idx, seed), g=gradient(idx, seed, HISTORY), m=m, v=v)


# ---- the model ----------------------------------------------------------------------------------------------------------------
def update64(p, g, m, v, t, lr, beta1, beta2, eps):
    """Adam's update of float64 arrays (numpy or torch) at step number t; lr and eps as the fp32 values the kernel gets."""
    lr, eps = float(np.float32(lr)), float(np.float32(eps))
    m1 = m + (g - m) * (1.0 - beta1)
    v1 = beta2 * v + (1.0 - beta2) * g * g
    p1 = p - lr / (1.0 - beta1 ** t) * m1 / (v1 ** 0.5 / (1.0 - beta2 ** t) ** 0.5 + eps)
    return p1, m1, v1


def group_slices(ends, begin, count, skip_mask):
    """[(group, lo, hi)] of the parts of [begin, begin + count) that lie in a group not named in skip_mask."""
    out, lo = [], 0
    for gi, end in enumerate(ends):
        a, b = max(lo, begin), min(int(end), begin + count)
        if a < b and not (skip_mask >> gi) & 1:
            out.append((gi, a, b))
        lo = int(end)
    return out


def model_step(p, g, m, v, ends, lrs, state, skip_mask=0, flag=0, begin=0, count=None, beta1=BETA1, beta2=BETA2, eps=EPS,
               zero_grad=1):
    """One call of ghr_adam_step / _range / _range_to from fp32 inputs: float64 p, m, v (the inputs, exactly, where nothing
    moves: a group of skip_mask, a raised flag, outside the range), the fp32 gradient afterwards, and the mask of moved
    elements.  `state`: the GHR_ADAM_STATE words at entry; group g is at its step state[0] + 1 - state[2 + g]."""
    n = p.size
    count = n - begin if count is None else count
    assert 0 <= begin and begin + count <= n and int(ends[-1]) == n and len(ends) <= THRESHOLDS["GHR_ADAM_MAX_GROUPS"]
    P, M, V = (np.asarray(x, np.float32).astype(np.float64) for x in (p, m, v))
    G = np.asarray(g, np.float32).copy()
    moved = np.zeros(n, bool)
    if not flag:
        with np.errstate(all="ignore"):
            for gi, a, b in group_slices(ends, begin, count, skip_mask):
                t = int(state[0]) + 1 - int(state[2 + gi])
                assert t >= 1
                P[a:b], M[a:b], V[a:b] = update64(P[a:b], G[a:b].astype(np.float64), M[a:b], V[a:b], t, lrs[gi], beta1, beta2,
                                                  eps)
                moved[a:b] = True
    if zero_grad:
        G[begin:begin + count] = 0.0
    return dict(p=P, m=M, v=V, g=G, moved=moved)


def model_state(state, skip_mask, n_groups, flag, finish=True):
    """The state words after the call: k_adam_finish (ghr_adam_step, or ghr_adam_step_range with last != 0) advances the
    counter and the lag of the groups that sat out unless the flag (state[1], as it stands after a scanning guard) is up,
    and clears it."""
    s = np.asarray(state, np.int32).copy()
    if finish:
        if not flag:
            s[0] += 1
            for gi in range(n_groups):
                if (skip_mask >> gi) & 1:
                    s[2 + gi] += 1
        s[1] = 0
    return s


def composed_step(p, g, m, v, t, lr, beta1=BETA1, beta2=BETA2, eps=EPS):
    """torch/optim/adam.py, _single_tensor_adam, operation by operation in numpy float32 (Python scalars enter an fp32
    tensor operation as fp32; the bias corrections are Python doubles):
        exp_avg.lerp_(grad, 1 - beta1); exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
        denom = (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps); param.addcdiv_(exp_avg, denom, value=-step_size)"""
    f = np.float32
    p, g, m, v = (np.asarray(x, f) for x in (p, g, m, v))
    with np.errstate(all="ignore"):
        m1 = m + f(1.0 - beta1) * (g - m)
        v1 = v * f(beta2) + f(1.0 - beta2) * g * g
        step_size = float(f(lr)) / (1.0 - beta1 ** t)
        denom = np.sqrt(v1) / f((1.0 - beta2 ** t) ** 0.5) + f(eps)
        p1 = p + f(-step_size) * (m1 / denom)
    assert p1.dtype == f and m1.dtype == f and v1.dtype == f
    return p1, m1, v1


def distances(got, ref, inp):
    """Worst distance, in u of the bar's scales, of fp32 results `got` (dict p, m, v) from the float64 `ref` over the elements
    where the reference is finite -- numpy arrays or torch tensors.  An error at zero scale is infinitely far."""
    out = {}
    p, g, m = _f64(inp["p"]), _f64(inp["g"]), _f64(inp["m"])
    with np.errstate(all="ignore"):
        scales = dict(m=abs(m) + (1.0 - BETA1) * abs(g), v=abs(ref["v"]), p=abs(ref["p"]) + abs(ref["p"] - p))
    for k in ("m", "v", "p"):
        sc = scales[k]
        with np.errstate(all="ignore"):
            err = abs(_f64(got[k]) - ref[k])
            fin = (ref[k] - ref[k]) == 0
            d = err / (U * sc)
        bad = fin & (sc == 0) & (err != 0)
        use = fin & (sc > 0)
        if _is_torch(d):
            import torch
            worst = float(torch.where(use, d, torch.zeros_like(d)).max()) if d.numel() else 0.0
        else:
            worst = float(np.where(use, np.nan_to_num(d), 0.0).max()) if d.size else 0.0
        out[k] = float("inf") if bool(bad.any()) else worst
    return out


def same_class(got, ref):
    """Where the reference is not finite the result has its class: NaN, +inf or -inf; elsewhere it is finite."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return bool((np.isnan(got) == np.isnan(ref)).all() and (np.isposinf(got) == np.isposinf(ref)).all() and
                (np.isneginf(got) == np.isneginf(ref)).all())


# ---- ghr_adam_relay_rows ----------------------------------------------------------------------------------------------------------
def model_relay(widths, P_old, P_new, take, fresh, child, overrides, p_in, m_in, v_in):
    """p_out[g][r] = overrides[g][child[r]] if overrides[g] is not None and child is not None and child[r] >= 0 else
    p_in[g][take[r]];  m_out / v_out[g][r] = 0 if fresh[r] else m_in / v_in[g][take[r]] -- group-major in both layouts."""
    take = np.asarray(take, np.int64)[:P_new]
    fresh = np.asarray(fresh)[:P_new] != 0
    outs = [[], [], []]
    off = 0
    for gi, w in enumerate(widths):
        rows = [np.asarray(x, np.float32)[off:off + w * P_old].reshape(P_old, w)[take] for x in (p_in, m_in, v_in)]
        ov = overrides[gi] if overrides is not None else None
        if ov is not None and child is not None:
            ch = np.asarray(child, np.int64)[:P_new]
            rows[0] = np.where((ch >= 0)[:, None], np.asarray(ov, np.float32).reshape(-1, w)[np.maximum(ch, 0)], rows[0])
        for k in (1, 2):
            rows[k] = np.where(fresh[:, None], np.float32(0.0), rows[k])
        for k in range(3):
            outs[k].append(np.ascontiguousarray(rows[k], np.float32).reshape(-1))
        off += w * P_old
    return tuple(np.concatenate(o) if o else np.zeros(0, np.float32) for o in outs)


WIDTHS = {1: (3,), 8: (3, 3, 4, 1, 1, 1, 3, 45), 16: (1, 3, 4, 45, 1, 1, 3, 4, 1, 45, 3, 1, 4, 1, 3, 1)}
RELAY_ROWS = ((1, 1), (5, 3), (3, 5), (300, 257), (257, 300))        # (P_old, P_new): shrinking and growing
RELAY_BIG = dict(groups=8, P_old=70000, P_new=68761)                 # 61 * 68 761 = 4 194 421 elements: RELAY_TRIP + 117
CHILD_MODES = ("null", "two_groups", "all_minus_one")


def relay_case(groups, P_old, P_new, child_mode, seed):
    """Inputs of one re-lay: take with repeats (and, where P_old allows, rows nobody takes), mixed fresh, child as named:
    "null" (no child array, no overrides), "two_groups" (children on about a third of the rows, override rows for the first
    and the last group only: the others take the gathered row where child >= 0), "all_minus_one" (overrides on those two
    groups, but no row is a child)."""
    rng = np.random.default_rng(seed)
    widths = WIDTHS[groups]
    n_old = sum(widths) * P_old
    take = rng.integers(0, P_old, P_new).astype(np.int64)
    if P_new > 1:
        take[-1] = take[0]                                    # a repeat whatever the draw
    fresh = (rng.random(P_new) < 0.4).astype(np.uint8)
    child, overrides = None, None
    if child_mode != "null":
        is_child = rng.random(P_new) < 0.35 if child_mode == "two_groups" else np.zeros(P_new, bool)
        if child_mode == "two_groups" and P_new:
            is_child[P_new - 1] = True
        n_children = int(is_child.sum())
        child = np.full(P_new, -1, np.int64)
        child[is_child] = rng.permutation(n_children)
        overrides = [None] * groups
        for gi in sorted({0, groups - 1}):
            overrides[gi] = (1000.0 + rng.random((max(n_children, 1), widths[gi]))).astype(np.float32)
    bufs = [(k * 10.0 + 1.0 + np.arange(n_old) % 8191 / 8192.0).astype(np.float32) for k in range(3)]
    return dict(widths=widths, P_old=P_old, P_new=P_new, take=take, fresh=fresh, child=child, overrides=overrides,
                p_in=bufs[0], m_in=bufs[1], v_in=bufs[2], n_new=sum(widths) * P_new)


# ---- ghr_adam_fused_finish ----------------------------------------------------------------------------------------------------------
FINISH_N = (1, 3, 4, 5, FINISH_TRIP, FINISH_TRIP + 3, 2 * FINISH_TRIP + 1029)


def model_finish(flag, state, ins, outs):
    """(outs after, state after, flag_next after): out := in for p, m, v when the flag is up, else the counter advances;
    the other flag word is cleared either way, the flag word itself is never written."""
    s = np.asarray(state, np.int32).copy()
    if not flag:
        s[0] += 1
    return tuple(np.asarray(i if flag else o).copy() for i, o in zip(ins, outs)), s, 0


# ---- the step cases -----------------------------------------------------------------------------------------------------------------
LRS = (1.6e-4, 2.5e-3, 1.25e-4, 0.05, 1e-3, 5e-3, 7e-5, 1e-2, 3e-4, 2e-5, 0.02, 6e-4, 1.6e-6, 4e-3, 9e-4, 1.1e-3)
SINGLE_N = (1, 2, 3, 4, 5)                                       # below 4 only the tail of k_adam_v4 runs
N_GROUPS = 4099
# every residue mod 4; quads 0 and 1 touch four groups each; one-element groups; 16 groups; the v4 tail spans an end
ENDS_GROUPS = (1, 2, 3, 5, 6, 7, 8, 1031, 1032, 2050, 2051, 3000, 3001, 4094, 4097, 4099)   # quad 512 touches three
SKIP_MASKS = (0, (1 << 0) | (1 << 1) | (1 << 5) | (1 << 15), (1 << 7) | (1 << 9) | (1 << 14))
STEP_COUNTS = (0, 6, 29999)                                      # state[0]


def lags(step_count, n_groups):
    """state[2 + g]: a different number of sat-out steps per group, none beyond the counter."""
    return [min(step_count, (5 * g + 1) % 13) for g in range(n_groups)]


def make_state(step_count, n_groups, flag=0):
    s = np.full(STATE_WORDS, 0, np.int32)
    s[0], s[1] = step_count, flag
    s[2:2 + n_groups] = lags(step_count, n_groups)
    s[2 + n_groups:] = 77                                            # words of groups that do not exist: never read or written
    return s


RANGES = tuple((100 + b, 40 + c) for b in range(4) for c in range(4)) + \
    tuple((b, 2056 + c) for b in range(4) for c in range(4)) + \
    ((8, 1023), (1031, 1), (2050, 1), (512, 0), (0, 0), (4099, 0), (0, 4099), (4096, 3), (4097, 2), (3, 5), (1, 1))

STRIDE_SCALAR = dict(n=SCALAR_TRIP + 256 + 3, ends=(SCALAR_TRIP - 1, SCALAR_TRIP + 1, SCALAR_TRIP + 256 + 3), seed=31)
STRIDE_V4 = dict(n=V4_TRIP + 1024 + 3, ends=(V4_TRIP - 1, V4_TRIP + 2, V4_TRIP + 1024 + 3), seed=37)
NAN_AT = dict(first=0, last=STRIDE_SCALAR["n"] - 1, v4_tail=STRIDE_SCALAR["n"] - 2, second_trip=SCALAR_TRIP + 5, none=None)
SCAN_COUNTS = (1, 63, 64, 65, 256, 257, SCALAR_TRIP, SCALAR_TRIP + 1)


def single_case(n):
    return dict(n=n, ends=(n,), seed=100 + n)


GROUPS_CASE = dict(n=N_GROUPS, ends=ENDS_GROUPS, seed=17)
ALL_STEP_CASES = tuple(single_case(n) for n in SINGLE_N) + (GROUPS_CASE, STRIDE_SCALAR)


def quad_groups(ends, begin, n):
    """Per whole quad of k_adam_v4 over [begin, n): how many groups its four elements lie in."""
    idx = begin + np.arange(((n - begin) // 4) * 4)
    grp = np.searchsorted(np.asarray(ends[:-1]), idx, side="right")
    q = grp.reshape(-1, 4)
    return np.array([len(set(r)) for r in q]) if q.size else np.zeros(0, int)


def measure_composed(cases=ALL_STEP_CASES):
    """Worst distance of the composed fp32 form from model_step over the cases, every step count and group lag of the
    tests: dict(m, v, p) in u."""
    worst = dict(m=0.0, v=0.0, p=0.0)
    for case in cases:
        inp = make_inputs(case)
        ends = case["ends"]
        for sc in STEP_COUNTS:
            state = make_state(sc, len(ends))
            ref = model_step(inp["p"], inp["g"], inp["m"], inp["v"], ends, LRS, state, zero_grad=0)
            got = {k: np.empty_like(inp[k]) for k in ("p", "m", "v")}
            for gi, a, b in group_slices(ends, 0, case["n"], 0):
                t = sc + 1 - int(state[2 + gi])
                got["p"][a:b], got["m"][a:b], got["v"][a:b] = composed_step(inp["p"][a:b], inp["g"][a:b], inp["m"][a:b],
                                                                          inp["v"][a:b], t, LRS[gi])
            d = distances(got, ref, inp)
            worst = {k: max(worst[k], d[k]) for k in worst}
    return worst
