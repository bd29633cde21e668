"""`-m gpu`: ``k_cam_pack`` / ``k_cam_merge`` through the C ABI (``ghr_camera_pack_row_message``, ``ghr_camera_merge_ranks``) into
poisoned, guarded buffers against the numpy model of tests/camera_exchange_cases.py, exact.  The gather is simulated by stacking
the ranks' messages in one process: no process group."""
import ctypes

import numpy as np
import pytest
import torch

from gaussianhaircut_amd import _lib
from gaussianhaircut_amd.scene.cameras import merge_ranks_torch, pack_row_message_torch
from tests.camera_exchange_cases import make_case, merge_model, pack_model, same_bits

pytestmark = pytest.mark.gpu

GUARD = 64          # floats / ints in front of and behind every buffer the kernels write
POISON = -12345.5


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _guarded(payload, dev):
    """(whole buffer, the payload's view) with GUARD poisoned elements on both sides"""
    flat = torch.from_numpy(np.ascontiguousarray(payload)).reshape(-1)
    poison = POISON if flat.dtype == torch.float32 else -77
    whole = torch.full((flat.numel() + 2 * GUARD,), poison, dtype=flat.dtype, device=dev)
    whole[GUARD:GUARD + flat.numel()] = flat.to(dev)
    return whole, whole[GUARD:GUARD + flat.numel()].view(*payload.shape)


def _guards_intact(whole):
    poison = POISON if whole.dtype == torch.float32 else -77
    return bool((whole[:GUARD] == poison).all()) and bool((whole[-GUARD:] == poison).all())


@pytest.mark.parametrize("width", [8, 11])
@pytest.mark.parametrize("G", [1, 2, 3, 8])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_pack_and_merge_equal_the_numpy_model(N, G, width):
    dev = torch.device("cuda:0")
    L = _lib.lib()
    grads, touched = make_case(N, G, width)
    messages = []
    for q in range(G):
        g, t = torch.from_numpy(grads[q]).to(dev), torch.from_numpy(touched[q]).to(dev)
        whole, msg = _guarded(np.full((N, width + 1), POISON, dtype=np.float32), dev)
        _lib.check(L.ghr_camera_pack_row_message(_stream(dev), N, width, _p(g), width, _p(t), _p(msg)))
        torch.cuda.synchronize()
        want = pack_model(grads[q], touched[q])
        assert same_bits(msg.cpu().numpy(), want), ("pack", N, G, width, q)
        assert _guards_intact(whole)
        assert not np.isnan(want[touched[q] == 0]).any()  # (the stale NaN of an untouched row did not travel)
        assert same_bits(pack_row_message_torch(g, t, torch.full_like(msg, POISON)).cpu().numpy(), want)  # the torch form, too
        messages.append(want)
    gathered = np.stack(messages)
    gathered_dev = torch.from_numpy(gathered).to(dev)
    for q in range(G):  # every rank merges into ITS buffers and ends with the same rows wherever a rank touched one
        want_g, want_t = merge_model(gathered, grads[q], touched[q])
        whole_g, g = _guarded(grads[q], dev)
        whole_t, t = _guarded(touched[q], dev)
        g2, t2 = g.clone(), t.clone()
        _lib.check(L.ghr_camera_merge_ranks(_stream(dev), N, width, G, _p(gathered_dev), _p(g), width, _p(t)))
        torch.cuda.synchronize()
        assert same_bits(g.cpu().numpy(), want_g), ("merge", N, G, width, q)
        assert (t.cpu().numpy() == want_t).all()
        assert _guards_intact(whole_g) and _guards_intact(whole_t)
        merge_ranks_torch(gathered_dev, g2, t2)
        assert same_bits(g2.cpu().numpy(), want_g) and (t2.cpu().numpy() == want_t).all()
        any_touched = touched.any(axis=0)
        assert (want_t[any_touched] == 1).all() and same_bits(want_g[~any_touched], grads[q][~any_touched])
        if q:
            assert same_bits(want_g[any_touched], first_g[any_touched])
        else:
            first_g = want_g
    # a row that one rank alone touched keeps that rank's bits, its -0.0 included
    lone = np.flatnonzero(touched.sum(axis=0) == 1)
    for r in lone:
        q = int(np.argmax(touched[:, r]))
        assert same_bits(first_g[r], grads[q, r])
    if N >= 2:
        assert np.isnan(first_g).any() and np.signbit(first_g[lone[0], 1])


def test_a_wider_gradient_stride_is_honoured():
    """grads rows `stride` floats apart: the floats between the rows are neither read into the message nor written by the merge"""
    dev = torch.device("cuda:0")
    L = _lib.lib()
    N, G, width, stride = 65, 3, 8, 13
    grads, touched = make_case(N, G, width)
    msgs = np.stack([pack_model(grads[q], touched[q]) for q in range(G)])
    wide = np.full((N, stride), POISON, dtype=np.float32)
    wide[:, :width] = grads[0]
    g, t = torch.from_numpy(wide).to(dev), torch.from_numpy(touched[0]).to(dev)
    msg = torch.empty(N, width + 1, device=dev)
    _lib.check(L.ghr_camera_pack_row_message(_stream(dev), N, width, _p(g), stride, _p(t), _p(msg)))
    assert same_bits(msg.cpu().numpy(), msgs[0])
    _lib.check(L.ghr_camera_merge_ranks(_stream(dev), N, width, G, _p(torch.from_numpy(msgs).to(dev)), _p(g), stride, _p(t)))
    torch.cuda.synchronize()
    want_g, want_t = merge_model(msgs, grads[0], touched[0])
    got = g.cpu().numpy()
    assert same_bits(got[:, :width], want_g) and (got[:, width:] == POISON).all() and (t.cpu().numpy() == want_t).all()
