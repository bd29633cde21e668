"""A replicated camera bank on more than one rank (``CameraBank.replicate`` / ``exchange_gradients``): gloo, world sizes 2 and 3,
``fused=False``, CPU tensors.  (a) bank level: hand-set gradient rows per rank, then ``step()``; (b) step level on the CPU oracle
path: one step equals a one-rank step over the same views bit for bit, replicas stay bit-identical; (c) the opt-in."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from gaussianhaircut_amd.parallel import FlatGradBucket
from gaussianhaircut_amd.scene.cameras import CameraBank, ring_cameras
from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams
from gaussianhaircut_amd.trainer import make_ground_truth, training_step
from gaussianhaircut_amd.utils import synthetic as syn
from tests.camera_exchange_cases import make_case, merge_model, pack_model, same_bits
from tests.oracle_backend import oracle_rasterizer
from tests.dist_helpers import collect
from tests.dist_helpers import free_port as _free_port

SPEC = syn.CONFIGS["tiny"]
N_BANK = 9                      # cameras of the bank-level case: every row pattern at least twice
DEAL = {3: [(0, 2), (2, 4), (4, 5)], 2: [(0, 2), (2, 3)]}   # 5 ring cameras dealt 2 + 2 + 1 and 2 + 1: one rank has fewer views
STEPS = 4
# bank-level steps: (seed, a NaN in a touched row?)
BANK_STEPS = [(0, False), (1, True), (2, False)]


def _bank_np(bank):
    return {k: getattr(bank, k).detach().cpu().numpy().copy() for k in ("params", "exp_avg", "exp_avg_sq", "steps")}


def _same_bank(a, b):
    return all(same_bits(a[k], b[k]) for k in ("params", "exp_avg", "exp_avg_sq", "steps"))


def _level_bank(use_barf, opt):
    return CameraBank(ring_cameras(N_BANK, 8, 8), use_barf=use_barf, fused=False).training_setup(opt)


def _scene():
    """the 5 ring cameras of the `tiny` config with ground truth, a model and a bank over them"""
    opt = OptimizationParams()
    cams = ring_cameras(5, SPEC.W, SPEC.H)
    gt = syn.make_model(SPEC)
    with torch.no_grad():
        gt._features_dc.add_(0.3)
    make_ground_truth(gt, cams, syn.background())
    model = syn.make_model(SPEC)
    model.training_setup(opt)
    bank = CameraBank(cams, use_barf=True, fused=False).training_setup(opt)
    return opt, model, bank


def _model_np(model):
    return [p.detach().numpy().copy() for p in model.leaf_parameters()]


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = {}
    opt = OptimizationParams()
    # ---- (c) the opt-in
    plain = CameraBank(ring_cameras(3, 8, 8), use_barf=True, fused=False).training_setup(opt)
    try:
        training_step(None, [plain[0]], None, opt, 1, camera_bank=plain)
        out["unreplicated"] = "no error"
    except NotImplementedError:
        out["unreplicated"] = "NotImplementedError"
    try:
        CameraBank(ring_cameras(3 + (rank == 1), 8, 8), use_barf=True, fused=False).replicate()
        out["counts"] = "no error"
    except ValueError as e:
        out["counts"] = "ValueError: %s" % e
    try:
        plain.exchange_gradients()
        out["exchange_unreplicated"] = "no error"
    except RuntimeError:
        out["exchange_unreplicated"] = "RuntimeError"
    # ---- (a) bank level
    for use_barf in (True, False):
        bank = _level_bank(use_barf, opt)
        if rank:  # (replicate() brings rank 0's state)
            with torch.no_grad():
                bank.params.add_(0.25 * rank)
                bank.exp_avg.add_(1.0)
                bank.steps.add_(3)
        assert bank.replicate() is bank
        trace = [_bank_np(bank)]
        for it, (seed, nan_row) in enumerate(BANK_STEPS):
            grads, touched = make_case(N_BANK, world, bank.width, seed=seed, nan_row=nan_row)
            bank.grads.copy_(torch.from_numpy(grads[rank]))
            bank.touched.copy_(torch.from_numpy(touched[rank]))
            bank.step(it + 1)
            assert not bank.touched.any()
            trace.append(_bank_np(bank))
        # from iterations_cam on step() returns before any collective -- on every rank alike
        bank.step(bank.iterations_cam)
        out["level_%d" % use_barf] = trace
    # ---- (b) step level on the CPU oracle path
    with oracle_rasterizer():
        opt, model, bank = _scene()
        bank.replicate()
        bucket = FlatGradBucket(model.leaf_parameters())
        lo, hi = DEAL[world][rank]
        mine = [bank[i] for i in range(lo, hi)]
        n_global = DEAL[world][-1][1]
        trace = []
        for it in range(1, STEPS + 1):
            training_step(model, mine, syn.background(), opt, it, bucket=bucket, global_views=n_global, camera_bank=bank)
            trace.append((_bank_np(bank), _model_np(model)))
        out["steps"] = trace
    out["rank"] = rank
    q.put(out)
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module", params=[2, 3])
def ranks(request):
    """the workers' results at one world size, computed once for the tests below"""
    world = request.param
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = collect(q, procs, world, timeout=500)  # (fails as soon as a worker has died)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    return world, res


@pytest.mark.timeout(900)
def test_the_opt_in(ranks):
    world, res = ranks
    for r in res:
        assert r["unreplicated"] == "NotImplementedError"
        assert r["counts"].startswith("ValueError") and "number of cameras" in r["counts"], r["counts"]
        assert r["exchange_unreplicated"] == "RuntimeError"


@pytest.mark.timeout(900)
@pytest.mark.parametrize("use_barf", [True, False])
def test_bank_level_steps_equal_one_bank_filled_by_the_rank_ordered_rule(ranks, use_barf):
    world, res = ranks
    traces = [r["level_%d" % use_barf] for r in res]
    for t in traces[1:]:  # every rank ends every step with identical params / moments / steps
        assert len(t) == len(traces[0]) and all(_same_bank(a, b) for a, b in zip(traces[0], t))
    opt = OptimizationParams()
    one = _level_bank(use_barf, opt)
    assert _same_bank(_bank_np(one), traces[0][0])  # rank 0's state was broadcast
    for it, (seed, nan_row) in enumerate(BANK_STEPS):
        grads, touched = make_case(N_BANK, world, one.width, seed=seed, nan_row=nan_row)
        gathered = np.stack([pack_model(grads[q], touched[q]) for q in range(world)])
        g, t = merge_model(gathered, grads[0], touched[0])
        assert nan_row == bool(np.isnan(g[t != 0]).any())
        assert np.isnan(grads[0][touched[0] == 0]).any()       # a stale NaN in an UNtouched row of the local buffer ...
        assert not np.isnan(gathered[0][touched[0] == 0]).any()  # ... does not travel
        before = _bank_np(one)
        one.grads.copy_(torch.from_numpy(g))
        one.touched.copy_(torch.from_numpy(t))
        one.step(it + 1)
        after = _bank_np(one)
        assert _same_bank(after, traces[0][it + 1]), (world, use_barf, it)
        untouched = touched.sum(axis=0) == 0
        assert untouched.any() and (~untouched).any()
        for k in after:  # rows no rank touched are unchanged; a NaN step is skipped altogether
            rows = slice(None) if nan_row else untouched
            assert same_bits(after[k][rows], before[k][rows])
        if not nan_row:
            assert (after["steps"][~untouched] == before["steps"][~untouched] + 1).all()
            assert (after["params"][~untouched] != before["params"][~untouched]).any(axis=1).all()


@pytest.mark.timeout(900)
def test_step_level_one_step_equals_one_rank_and_replicas_stay_identical(ranks):
    world, res = ranks
    traces = [r["steps"] for r in res]
    for t in traces[1:]:  # the replicas, Gaussians and bank, after every one of the 4 steps
        for (bank_a, model_a), (bank_b, model_b) in zip(traces[0], t):
            assert _same_bank(bank_a, bank_b)
            assert all(same_bits(x, y) for x, y in zip(model_a, model_b))
    n_global = DEAL[world][-1][1]
    with oracle_rasterizer():
        opt, model, bank = _scene()
        init = _bank_np(bank)
        bucket = FlatGradBucket(model.leaf_parameters())
        training_step(model, [bank[i] for i in range(n_global)], syn.background(), opt, 1, bucket=bucket, global_views=n_global,
                      camera_bank=bank)
    one = _bank_np(bank)
    assert _same_bank(one, traces[0][0][0]), world
    assert one["steps"].tolist() == [1] * n_global + [0] * (5 - n_global)
    assert (one["params"][:n_global] != init["params"][:n_global]).any(axis=1).all()
    last = traces[0][-1][0]
    assert last["steps"].tolist() == [STEPS] * n_global + [0] * (5 - n_global) and np.isfinite(last["params"]).all()
