"""`-m gpu`: a replicated, fused camera bank on TWO ranks that share cuda:0, gloo carrying the collectives (spawned as
tests/test_gpu_dist_shared.py spawns its ranks: three processes in all, one step stream each): ``k_cam_pack`` and ``k_cam_merge``
around the gather inside ``CameraBank.step``.  4 cameras; the two views of a step dealt 1 + 1, and 2 + 0 (a rank without a view).
  * the bank after one step is bit-equal to one rank's over the same two views,
  * the replicas -- Gaussians and bank -- are bit-identical after 4 steps, the last at ``iteration == iterations_cam`` (no
    collective of the bank's any more, on every rank alike)."""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests.dist_helpers import collect, free_port, fresh_model, scene_cameras

pytestmark = pytest.mark.gpu

CAMERAS, STEPS, ITERATIONS_CAM = 4, 4, 4
DEALS = {"1+1": [(0, 1), (1, 2)], "2+0": [(0, 2), (2, 2)]}


def _bank_and_model(dev):
    from gaussianhaircut_amd import _lib
    from gaussianhaircut_amd.scene.cameras import CameraBank
    _lib.lib().ghr_set_deterministic(1)  # runs are compared bit for bit: the gradient walk's atomics must be ordered
    cams, bg = scene_cameras(dev, CAMERAS)
    model, opt = fresh_model(dev, 3)
    opt.iterations_cam = ITERATIONS_CAM
    bank = CameraBank(cams, use_barf=True, device=dev).training_setup(opt)
    assert bank.fused
    return model, bank, bg, opt


def _bank_state(bank):
    """numpy: what a worker puts into the queue must not be a tensor (those travel as handles to the sender's memory)"""
    return {k: getattr(bank, k).detach().cpu().numpy().copy() for k in ("params", "exp_avg", "exp_avg_sq", "steps", "touched")}


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _worker(rank, world, port, q, deal):
    import torch.distributed as dist
    from gaussianhaircut_amd.parallel import param_checksum
    from gaussianhaircut_amd.trainer import training_step
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    model, bank, bg, opt = _bank_and_model(dev)
    if rank:  # (replicate() brings rank 0's state)
        with torch.no_grad():
            bank.params.add_(0.125)
    bank.replicate()
    lo, hi = DEALS[deal][rank]
    mine = [bank[i] for i in range(lo, hi)]
    trace = []
    for it in range(1, STEPS + 1):
        training_step(model, mine, bg, opt, it, global_views=2, views_per_rank=max(b - a for a, b in DEALS[deal]),
                      camera_bank=bank, streams=1)
        torch.cuda.synchronize()
        trace.append((_bank_state(bank), param_checksum(model.leaf_parameters())))
    q.put(dict(rank=rank, trace=trace))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(900)
@pytest.mark.parametrize("deal", ["1+1", "2+0"])
def test_two_ranks_step_one_replicated_bank(deal):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, deal)) for r in range(2)]
    for p in procs:
        p.start()
    res = collect(q, procs, 2, timeout=600)
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    a, b = res[0]["trace"], res[1]["trace"]
    for it, ((bank_a, sum_a), (bank_b, sum_b)) in enumerate(zip(a, b)):
        assert sum_a == sum_b, ("replicas diverged", deal, it)
        for k in bank_a:
            assert _same(bank_a[k], bank_b[k]), (deal, it, k)
        assert not bank_a["touched"].any()
    assert a[-1][0]["steps"].tolist() == [ITERATIONS_CAM - 1] * 2 + [0] * 2
    for k in ("params", "exp_avg", "exp_avg_sq", "steps"):  # the step at iterations_cam moved no camera
        assert _same(a[-1][0][k], a[-2][0][k]), k
    # one rank over the same two views
    from gaussianhaircut_amd.trainer import training_step
    dev = torch.device("cuda:0")
    model, bank, bg, opt = _bank_and_model(dev)
    init = bank.params.detach().cpu().numpy().copy()
    training_step(model, [bank[0], bank[1]], bg, opt, 1, global_views=2, camera_bank=bank, streams=1, fuse_adam=False)
    torch.cuda.synchronize()
    one = _bank_state(bank)
    for k in one:
        assert _same(one[k], a[0][0][k]), (deal, k, one[k], a[0][0][k])
    assert (one["params"][:2] != init[:2]).any(axis=1).all() and _same(one["params"][2:], init[2:])
    assert bool(np.isfinite(a[-1][0]["params"]).all())
