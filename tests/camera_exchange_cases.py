"""The cases and the numpy model of the camera bank's gradient exchange (``CameraBank.exchange_gradients``: pack, gather, merge),
shared by the CPU (gloo) and the GPU (C ABI) tests.

A case is, per rank, a gradient buffer ``grads [N, width]`` and its marks ``touched [N]``.  The row patterns, cycled over the rows:
touched by no rank, by one rank (a different one from row to row), by two ranks, by all ranks; one rank of G >= 3 touches nothing
at all.  Touched rows carry ``-0.0`` and, in one row, a NaN; UNtouched rows of every local buffer carry stale values, a stale NaN
among them, which must not travel."""
import numpy as np


def make_case(N, G, width, seed=0, nan_row=True):
    rng = np.random.default_rng(1000 * N + 10 * G + width + seed)
    grads = rng.standard_normal((G, N, width)).astype(np.float32)
    touched = np.zeros((G, N), dtype=np.int32)
    idle = G - 1 if G >= 3 else None  # a rank that touched nothing
    busy = [q for q in range(G) if q != idle]
    for r in range(N):
        kind = r % 4
        if kind == 1:
            touched[busy[(r // 4) % len(busy)], r] = 1
        elif kind == 2:
            for q in (busy[(r // 4) % len(busy)], busy[(r // 4 + 1) % len(busy)]):
                touched[q, r] = 1
        elif kind == 3:
            touched[busy, r] = 1
    # -0.0 in touched rows (assigned as it is by a lone rank; -0.0 + -0.0 stays -0.0)
    grads[:, :, 1] = np.where(touched != 0, np.float32(-0.0), grads[:, :, 1])
    # stale contents of untouched rows, a NaN among them
    stale = touched == 0
    grads[:, :, 0] = np.where(stale, np.float32(np.nan), grads[:, :, 0])
    grads[:, :, 2] = np.where(stale, np.float32(7.5), grads[:, :, 2])
    if nan_row and N >= 2:
        r = 1 if N < 6 else 5  # a row that one rank alone touched
        q = int(np.argmax(touched[:, r]))
        grads[q, r, 3] = np.nan
    return grads, touched


def pack_model(grads, touched):
    """message [N, width + 1] of one rank"""
    N, W = grads.shape
    msg = np.zeros((N, W + 1), dtype=np.float32)
    t = touched != 0
    msg[t, :W] = grads[t]
    msg[t, W] = 1.0
    return msg


def merge_model(gathered, grads, touched):
    """(grads, touched) of a rank after the merge of ``gathered [G, N, width + 1]``: float32 sums in ascending rank order"""
    G, N, W1 = gathered.shape
    W = W1 - 1
    g, t = grads.copy(), touched.copy()
    for r in range(N):
        first = True
        for q in range(G):
            if gathered[q, r, W] == 0:
                continue
            with np.errstate(invalid="ignore"):
                g[r] = gathered[q, r, :W] if first else (g[r] + gathered[q, r, :W]).astype(np.float32)
            first = False
        if not first:
            t[r] = 1
    return g, t


def same_bits(a, b):
    """equal bit patterns (so -0.0 is not 0.0); a NaN equals a NaN whatever its payload"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float32:
        return bool((a == b).all())
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
