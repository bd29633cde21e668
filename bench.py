#!/usr/bin/env python
"""bench.py -- the measured hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W        (N > 1 without a launcher: bench.py starts the N ranks itself)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
           bench.py --gpus N --steps K --warmup W
    options: --full (everything below `grad_steps_per_sec`), --dump-outputs DIR (the last timed step's results as .npy,
             from a bit-reproducible replay of the timed path)

A plain run sets up, settles, warms up, times the K steps, writes --dump-outputs if asked and prints the headline fields
(metric ... grad_steps_per_sec, config).  `--full` then goes on with everything else in the same line.

HEADLINE (the one JSON line, rank 0): BASELINE.json configs[2] exactly -- one gradient step of the reference's stage-1
loop shape (src/train_gaussians.py:96-181, no densification) on ONE 1920x1080 view of the 500k strand-aligned model per
GPU: render() (fused HIP projection + rasterizer forward), the four stage-1 losses incl. the orientation term
(lambda_dorient = 0.1, run.sh:112-115), backward (HIP loss / rasterizer / projection backward), [one flat sum of the
Gaussian gradients over RCCL when N > 1], Adam.  Inputs are resident in HBM.  The steps draw their views in turn from 16
ring cameras per GPU (the reference draws a random training camera per iteration, train_gaussians.py:103-105).  Weak
scaling: one view per GPU per step at every N (a global step covers N views).
  value               = sum over the timed steps' views of P_vis / elapsed: Gaussians per second through the whole step,
                        P_vis = Gaussians of the model that pass the cull of the view (radii > 0), NOT the model size
  grad_steps_per_sec  = 1 / t_step
--full only:
  roofline            : k_render_bwd_cells = K8 (the dominant kernel): SURVEY 8(d) algorithmic bytes / HIP-event duration on the
                        launch stream over solo passes cycling over the same cameras, against 8 TB/s HBM; `traffic` from the
                        committed rocprofv3 FETCH_SIZE / WRITE_SIZE passes (profiles/).
  repeat_ms_per_step  : the same K steps once more, straight behind the timed ones -- a diagnostic, never used for `value`
Further blocks of the same line (N = 1 unless noted), each named for what it measures.  Blocks timed over steps run TWO timed
passes and report the faster one (`ms_per_step_passes` lists both): they exist to be compared with the headline, a pass lasts
7-40 ms, and the boxes of this pool stall a process for a few milliseconds now and then (`host_gc`: it is not Python's
collector):
  fixed_camera_step   : the headline step on camera 0 only (what rounds 1-5 timed)
  config4_shard       : BASELINE configs[3]'s per-GPU shard -- 4 views per GPU per step, same model (every N)
  config5_2M          : BASELINE configs[4]'s model (2M strand Gaussians), one view per step: step time, K8 time and fraction
  dropin_trainable_camera_step : the configs[2] step with camera parameters that require grad (the reference's default run)
  strand_stage        : one iteration of the strand stage (render_hair, 3.07 M Gaussians), fused vs generic projection
  op_only             : SURVEY 8(d)(i), the rasterizer op ALONE (GaussianRasterizer autograd op, mode A), cfg2
                        (BASELINE configs[1], 100k blobs) and cfg3 (500k strands): Gaussians / (t_fwd + t_bwd), and the
                        whole backward (K8 + per-Gaussian epilogue) against B_bwd = 140 P + 132 R + 48 N + 8 T
  cpu_baseline        : the CPU oracle (oracle/ghr_oracle.c, OpenMP; pinned to the reference's CUDA) on the SAME scope as
                        op_only.cfg3: rasterizer forward + backward of one view, Gaussians / (t_fwd + t_bwd)
"""
from __future__ import annotations

import argparse
import ctypes
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6.3 TB/s is the measured copy ceiling


def _free_port() -> int:
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as so:
        so.bind(("127.0.0.1", 0))
        return int(so.getsockname()[1])


def relaunch_command(n: int, argv):
    """`python bench.py --gpus N` started WITHOUT torchrun: the command that runs N ranks of this script on this node."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr",
            "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + list(argv)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="cfg3", choices=["cfg1", "cfg2", "cfg3", "cfg5", "tiny"])
    ap.add_argument("--views-per-gpu", type=int, default=1,
                    help="views per GPU per global step of the headline; 1 = BASELINE.json configs[2]")
    ap.add_argument("--shard-views", type=int, default=4,
                    help="views per GPU per step of the config4_shard block (BASELINE.json configs[3]: 32 views on 8 GPUs); 0 = skip")
    ap.add_argument("--cameras", type=int, default=16,
                    help="training cameras per GPU the steps draw from in turn (the reference draws a random camera per "
                         "iteration, train_gaussians.py:103-105); 1 = every step renders the same view")
    ap.add_argument("--streams", type=int, default=None,
                    help="HIP streams the views of a step alternate on (default: trainer's choice, 2; 1 = one stream, "
                         "the setting per-kernel rocprof averages should be taken with)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-op-only", action="store_true")
    ap.add_argument("--no-2m", action="store_true", help="skip the config5_2M block (BASELINE configs[4]'s model, N = 1)")
    ap.add_argument("--no-camera-block", action="store_true", help="skip the dropin_trainable_camera_step block (N = 1)")
    ap.add_argument("--no-strand-block", action="store_true", help="skip the strand_stage block (render_hair at the reference's size, N = 1)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run everything else the line can carry: repeat, solo kernel times and "
                         "roofline, replica check, the side blocks (each --no-* above skips one), op_only, cpu_baseline, "
                         "host_gc; off: the line holds the headline alone")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed to DIR/<name>.npy (rank 0), from a replay of the same "
                         "steps with the gradient walk's additions in a fixed order: the same every run (see dump_outputs)")
    args = ap.parse_args()

    # `--gpus N` without a launcher: become the launcher (one process per GPU, ranks over RCCL), never a silent 1-rank run.
    # The ranks run as child processes; this one only waits for them (it never touches the GPU).
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        import subprocess
        cmd = relaunch_command(args.gpus, sys.argv[1:])
        sys.stderr.write("bench.py: --gpus %d without torchrun; launching %s\n" % (args.gpus, " ".join(cmd[1:10]) + " ..."))
        sys.stderr.flush()
        sys.exit(subprocess.call(cmd))

    from gaussianhaircut_amd import _lib
    from gaussianhaircut_amd import diff_gaussian_rasterization as dgr
    from gaussianhaircut_amd.parallel import env_world, init_distributed
    from gaussianhaircut_amd.scene.cameras import TrainableCamera, ring_cameras
    from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams
    from gaussianhaircut_amd.trainer import make_ground_truth, training_step
    from gaussianhaircut_amd.utils import synthetic as syn

    env_rank, _, env_n = env_world()
    if env_n != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d (launch with torch.distributed.run --nproc-per-node %d, or "
                         "without a launcher: bench.py starts the ranks itself)" % (args.gpus, env_n, args.gpus))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a ROCm GPU (the HIP path has no CPU fallback) [rank %d of %d]" % (env_rank, env_n))
    # GHR_BENCH_BACKEND=gloo + GHR_BENCH_SHARE_GPU=1: functional check of the N > 1 path on a box with fewer GPUs than
    # ranks (ranks share devices, the gradient all-reduce goes through gloo); never a performance number
    share = os.environ.get("GHR_BENCH_SHARE_GPU") == "1"
    if torch.cuda.device_count() < env_n and not share:
        raise SystemExit("bench.py: --gpus %d but only %d device(s) visible (GHR_BENCH_SHARE_GPU=1 lets ranks share a device "
                         "for a functional check)" % (env_n, torch.cuda.device_count()))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if share:
        local_rank %= torch.cuda.device_count()
        torch.cuda.set_device(local_rank)
    rank, world = init_distributed(backend=os.environ.get("GHR_BENCH_BACKEND") or None)
    assert world == args.gpus
    backend = dist.get_backend() if (world > 1 and dist.is_initialized()) else None
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    L = _lib.lib()

    spec = syn.CONFIGS[args.workload]
    V = args.views_per_gpu
    VS = max(args.shard_views, 0)
    NC = max(args.cameras, V, VS, 1)
    global_views = V * world
    opt = OptimizationParams()
    opt.lambda_dorient = 0.1  # the reference's stage-1 command line (run.sh:112-115)
    bg = syn.background(dev)
    from gaussianhaircut_amd import trainer as _tr
    from gaussianhaircut_amd.gaussian_renderer import render as _render

    def build_scene(spec_, n_cams, cls=None):
        """model replica (identical on every rank: CPU-seeded) + this rank's training cameras with synthetic ground truth"""
        model_ = syn.make_model(spec_, dev)
        ring = ring_cameras(n_cams * world, spec_.W, spec_.H, device=dev, cls=cls)  # camera 0 == the SURVEY front camera
        pool_ = ring[rank::world][:n_cams]
        with torch.no_grad():
            gt = syn.make_model(spec_, dev)
            g = torch.Generator(device="cpu").manual_seed(202)
            gt._xyz.add_((0.002 * torch.randn(gt._xyz.shape, generator=g)).to(dev))
            gt._features_dc.add_((0.05 * torch.randn(gt._features_dc.shape, generator=g)).to(dev))
            make_ground_truth(gt, pool_, bg)
            del gt
            # ... and what a data loader would hand over with them: the SSIM window moments of every camera's ground truth
            # (constants of a training view, trainer._gt_stats: 2 x 3 planes per camera, computed once)
            for c in pool_:
                _tr._gt_stats(c, c.original_image, c.original_mask, True)
        model_.training_setup(opt)  # FusedAdam on ROCm: flat params / grads / moments
        torch.cuda.synchronize()
        return model_, pool_

    def sync_all():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def max_over_ranks(x: float) -> float:
        if world == 1:
            return x
        t = torch.tensor([x], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    # Full collections of Python's cyclic garbage collector that fall into a timed region, with their duration, go into the line
    # (`host_gc`).  Round 6 looked for the cause of sporadic slow side blocks (one run in five: 2.8 - 3.7 ms where the others
    # read 2.0 - 2.3) here first: twelve runs, not one collection inside a timed region -- and gc.collect() + gc.freeze() in
    # front of the regions made the headline WORSE (0.70 -> 0.72 - 0.86 in three runs of six: profiles/r06r), so nothing of
    # the kind is done.  The disturbances are the box's (they hit whatever block is running, for ~0.1 s).
    import gc as _gc
    gc_log = {"gen2_collections": 0, "gen2_ms": 0.0, "longest_ms": 0.0, "_t": 0.0, "timed": False}

    def _gc_cb(phase, info):
        if info.get("generation") != 2 or not gc_log.get("timed"):
            return
        if phase == "start":
            gc_log["_t"] = time.perf_counter()
        else:
            dt_ = 1e3 * (time.perf_counter() - gc_log["_t"])
            gc_log["gen2_collections"] += 1
            gc_log["gen2_ms"] += dt_
            gc_log["longest_ms"] = max(gc_log["longest_ms"], dt_)
    if args.full:
        _gc.callbacks.append(_gc_cb)

    def timed_steps(model_, pool_, v, n_warm, n_steps, it0=0, gv=None, after_step=None):
        """n_warm untimed + n_steps timed gradient steps; step i renders cameras (i v + j) mod len(pool), j < v.
        Returns (seconds for the timed steps, max over ranks; the camera indices of every timed step)."""
        def views(i):
            return [(i * v + j) % len(pool_) for j in range(v)]

        def one(i):
            training_step(model_, [pool_[c] for c in views(i)], bg, opt, it0 + i + 1, global_views=gv or v * world,
                          streams=args.streams)
            if after_step is not None:
                after_step([pool_[c] for c in views(i)])
        for i in range(n_warm):
            one(i)
        sync_all()
        gc_log["timed"] = True
        t0 = time.perf_counter()
        for i in range(n_steps):
            one(n_warm + i)
        sync_all()
        dt_timed = time.perf_counter() - t0
        gc_log["timed"] = False
        return max_over_ranks(dt_timed), [views(n_warm + i) for i in range(n_steps)]

    def timed_steps_2(model_, pool_, v, n_warm, n_steps, it0=0, **kw):
        """For the SIDE blocks: two timed passes of n_steps, the faster one returned, both listed (ms per step).  A pass of ten or
        twenty steps lasts 7-40 ms and the boxes of this pool stall a process for 3-4 ms every now and then (not this process'
        doing: DESIGN.md 7a); a side block exists to be compared with the headline, and a stalled pass compares the box with
        itself.  The headline is timed ONCE, K steps, as the contract says (its repeat is printed beside it, never used)."""
        a, ua = timed_steps(model_, pool_, v, n_warm, n_steps, it0=it0, **kw)
        b, ub = timed_steps(model_, pool_, v, 0, n_steps, it0=it0 + n_warm + n_steps, **kw)
        passes = [round(1e3 * a / n_steps, 4), round(1e3 * b / n_steps, 4)]
        return (a, ua, passes) if a <= b else (b, ub, passes)

    def visible(model_, cams_):
        with torch.no_grad():
            return [int((_render(c, model_, _tr.PIPE, bg)["radii"] > 0).sum().item()) for c in cams_]

    def solo_kernel_times(model_, cams_, n_pass, gv):
        """HIP events around the two render kernels, recorded by the library on the launch stream.  In the timed steps the
        kernels of two views may share the GPU (two streams), so a kernel's wall time there is not a property of the kernel;
        here view after view runs alone: render + loss + backward, no optimizer step (the accumulated gradients are
        dropped afterwards).  Pass i renders cams_[i mod len]; returns per pass (fwd ms, bwd ms, R of the view)."""
        evs = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(n_pass)]
        for quad in evs:
            for e in quad:
                e.record()  # materialise the hipEvent_t
        torch.cuda.synchronize()
        Rs = []
        for i, q in enumerate([None, None] + evs):
            if q is not None:
                L.ghr_set_profile_events(*[ctypes.c_void_p(e.cuda_event) for e in q])
            cam = cams_[max(i - 2, 0) % len(cams_)]
            pkg = _render(cam, model_, _tr.PIPE, bg)
            loss = _tr.view_loss(pkg, cam, opt, scale=1.0 / gv)
            loss.backward()
            if q is not None:
                Rs.append(int(pkg.count))
        L.ghr_set_profile_events(None, None, None, None)
        torch.cuda.synchronize()
        model_.optimizer._direct_backwards = 0
        model_.optimizer.zero()
        model_.optimizer.state_dev[1:2].zero_()
        torch.cuda.synchronize()
        return [(q[0].elapsed_time(q[1]), q[2].elapsed_time(q[3]), r) for q, r in zip(evs, Rs)]

    # ---- headline: BASELINE configs[2] -----------------------------------------------------------------------------------
    model, pool = build_scene(spec, NC)
    K, Wm = args.steps, args.warmup
    L.ghr_set_profile_events(None, None, None, None)
    # settle (setup, untimed, like the ground-truth renders above): every camera of the pool is stepped through three times, so
    # that the allocator's pools, the capacity guess, the clocks and -- on a fresh box -- the page cache behind the host's launch
    # path are those of a running training loop when the W warm-up steps begin (the first process on a fresh box once read
    # 0.84 ms for a step whose kernels sum to 0.70: profiles/r06e)
    n_settle = 3 * len(pool)
    timed_steps(model, pool, V, n_settle, 0)
    elapsed, used = timed_steps(model, pool, V, Wm, K, it0=n_settle)
    ms_per_step = 1e3 * elapsed / K
    fused_steps = getattr(model.optimizer, "fused_steps", 0)
    if args.dump_outputs:
        # The timed steps add each gradient line's contributions in the GPU's scheduling order (as the reference's atomicAdd
        # does), and Adam turns last-bit differences of near-cancelled gradients into whole steps: the parameters of two runs
        # part within a few steps.  What is dumped is the same path replayed from the same seeded start -- a fresh scene, the
        # same settle, warm-up and timed steps on the same cameras and iterations -- with those additions in a fixed order
        # (ghr_set_deterministic: bit-reproducible), so that two runs, and two builds, can be compared output for output.
        model_d, pool_d = build_scene(spec, NC)
        prev_det = L.ghr_set_deterministic(1)
        try:
            for it0, n in ((0, n_settle), (n_settle, Wm + K)):  # (timed_steps: settle, then warm-up + timed steps)
                for i in range(n):
                    loss_d = training_step(model_d, [pool_d[(i * V + j) % len(pool_d)] for j in range(V)], bg, opt,
                                           it0 + i + 1, global_views=V * world, streams=args.streams)
            sync_all()
        finally:
            L.ghr_set_deterministic(prev_det)
        if rank == 0:
            dump_outputs(args.dump_outputs, model_d, loss_d)
        del model_d, pool_d, loss_d
        torch.cuda.empty_cache()

    P_model = spec.P
    # Gaussians that pass the cull of a view (radii > 0): what the rasterizer actually carries through forward and
    # backward.  Outside the timed region; summed over the views the timed steps rendered.
    P_vis = visible(model, pool)
    p_sum = torch.tensor([float(sum(P_vis[c] for vs in used for c in vs))], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(p_sum)
    value = float(p_sum.item()) / elapsed

    out = {
        "metric": "gaussians_per_sec_grad_step_500k_strands_1080p", "value": round(value, 1), "unit": "Gaussians/s",
        "n_gpus": world, "steps": K, "warmup": Wm, "ms_per_step": round(ms_per_step, 4), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": "BASELINE configs[2]: %s, %d Gaussians (%s) in the model, %d view(s) per GPU per gradient step "
                               "at %dx%d, drawn in turn from %d ring cameras per GPU (all ground truth resident): render + 4 "
                               "stage-1 losses (L1, SSIM, mask, orientation 0.1) + backward%s + Adam" %
                   (spec.name, P_model, spec.kind, V, spec.W, spec.H, len(pool),
                    " + gradient sum over %d ranks (backend %s%s)" % (world, backend, " = RCCL" if backend == "nccl" else "")
                    if world > 1 else ""),
                   "views_per_gpu": V, "global_views": global_views, "parallelism": "view-dp%d" % world,
                   "backend": backend, "cameras_per_gpu": len(pool), "settle_steps_before_warmup": n_settle,
                   "optimizer": ("Adam applied by the step's last k_project_bwd (ghr_adam_fuse): %d of the %d timed + warm-up steps"
                                 % (fused_steps - n_settle, K + Wm)) if fused_steps
                   else "separate k_adam_v4 pass",
                   "P_model": P_model, "P_visible_per_camera": P_vis,
                   "value_is": "sum over the timed steps' views of the Gaussians that pass the cull / elapsed time"},
        "grad_steps_per_sec": round(K / elapsed, 3),
    }
    if not args.full:  # the headline is all a plain run measures
        if rank == 0:
            print(json.dumps(out), flush=True)
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return

    # ---- --full: everything below adds to the same line ------------------------------------------------------------------
    # (a diagnostic only, printed as `repeat_ms_per_step`: the same K steps once more, straight behind the timed ones.  `value`
    # and `ms_per_step` are the FIRST K steps whatever this says; two numbers far apart mean the box stalled the process in one
    # of the two 14-ms windows)
    elapsed_rep, _ = timed_steps(model, pool, V, 0, K, it0=n_settle + Wm + K)

    N_pix = spec.W * spec.H
    T_tiles = ((spec.W + 15) // 16) * ((spec.H + 15) // 16)
    n_ev = max(K, 10, len(pool))
    solo = solo_kernel_times(model, pool, n_ev, global_views)
    # K8's share of B_bwd = per instance 68 B read + 64 B gradient payload, per pixel 48 B, ranges 8 B/tile
    bytes_bwd = [132 * r + 48 * N_pix + 8 * T_tiles for _, _, r in solo]
    bytes_fwd = [68 * r + 48 * N_pix + 8 * T_tiles for _, _, r in solo]
    fwd_avg, bwd_avg = sum(s_[0] for s_ in solo) / len(solo), sum(s_[1] for s_ in solo) / len(solo)
    bytes_bwd_kernel, bytes_fwd_kernel = sum(bytes_bwd) / len(solo), sum(bytes_fwd) / len(solo)
    achieved = bytes_bwd_kernel / (bwd_avg * 1e-3) / 1e9 if bwd_avg > 0 else 0.0
    per_cam = {}
    for i, (f_, b_, r_) in enumerate(solo):
        per_cam.setdefault(i % len(pool), []).append((b_, r_))
    cam0 = per_cam.get(0, [(bwd_avg, 0)])
    cam0_ms, cam0_R = sum(x[0] for x in cam0) / len(cam0), cam0[0][1]

    replicas_identical = None
    if world > 1:
        # identical reduced gradients + identical Adam => the replicas must still be bit-identical
        bits = model.optimizer.flat_param.view(torch.int32).to(torch.int64)
        ck = torch.stack([bits.sum(), (bits * (torch.arange(bits.numel(), device=dev) % 8191 + 1)).sum()])
        lo, hi = ck.clone(), ck.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        replicas_identical = bool(torch.equal(lo, hi))

    traffic, traffic_src, traffic_stale = None, None, None
    pmc_file = os.path.join(ROOT, "profiles", "pmc_k_render_bwd.json")
    if os.path.exists(pmc_file):
        whole = {}
        try:
            whole = json.load(open(pmc_file))
            rec = whole.get(args.workload, whole if args.workload == "cfg3" and "hbm_bytes_per_launch" in whole else {})
            traffic, traffic_src = rec.get("hbm_bytes_per_launch"), rec.get("source")
        except Exception:
            traffic = None
        # the counters were taken from a particular build of the kernel: the record carries the hash of its sources
        # (tools/k8_source_hash.py, written by the profiling script) and a figure taken from other sources says so.  Its own
        # try: a failure here must not drop a traffic figure that was read successfully
        try:
            import importlib.util
            hs = importlib.util.spec_from_file_location("k8_source_hash", os.path.join(ROOT, "tools", "k8_source_hash.py"))
            hm = importlib.util.module_from_spec(hs)
            hs.loader.exec_module(hm)
            traffic_stale = whole.get("k8_source_sha256") != hm.k8_source_hash()
        except Exception:
            traffic_stale = None
    roofline = {"kernel": "k_render_bwd_cells (K8)", "bound": "hbm", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS,
                "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": traffic,
                "traffic_source": traffic_src, "traffic_stale": traffic_stale,
                "algorithmic_bytes_per_launch": int(bytes_bwd_kernel), "avg_kernel_ms": round(bwd_avg, 4),
                "camera0": {"avg_kernel_ms": round(cam0_ms, 4), "num_rendered": cam0_R,
                            "frac": round((132 * cam0_R + 48 * N_pix + 8 * T_tiles) / (cam0_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5)
                            if cam0_ms > 0 else None,
                            "note": "the SURVEY front camera alone (what rounds 1-5 quoted, and the view `traffic` was counted on)"},
                "note": "gradient walk NOT bound by HBM bandwidth: it issues one 64-B line atomic per (cell, splat) hit and the L2 "
                        "retires ~17 G of them per second (profiles/r04k: 2.96 M hits = 0.174 ms on this workload; four more "
                        "per chunk cost 2.7x), with the wave's issue chain (~0.17 ms) and the chunk arithmetic (0.117 ms of "
                        "VALU) right behind; every L2 atomic is written through to HBM, hence traffic > algorithmic bytes; "
                        "the zero-fill of the gradient lines is the forward render kernel's last act; DESIGN.md 10 / 11); "
                        "algorithmic bytes 132 R + 48 N + 8 T per SURVEY.md 8(d) with R, N, T of each measured view (mean over "
                        "the passes); kernel duration from HIP events the library records around the kernel on its launch "
                        "stream, %d solo passes cycling over this rank's %d training cameras" % (n_ev, len(pool))}

    out["config"]["num_rendered_per_camera"] = [per_cam[c][0][1] for c in sorted(per_cam)]
    out.update({
        "kernels_ms": {"k_render_fwd": round(fwd_avg, 4), "k_render_bwd": round(bwd_avg, 4),
                       "k_render_fwd_hbm_frac": round(bytes_fwd_kernel / (fwd_avg * 1e-3) / 1e9 / HBM_PEAK_GBS, 5)
                       if fwd_avg > 0 else None},
        "roofline": roofline,
        "repeat_ms_per_step": round(1e3 * elapsed_rep / K, 4),
    })
    if replicas_identical is not None:
        out["replicas_identical"] = replicas_identical

    # ---- the same step on ONE camera (what rounds 1-5 timed): the per-camera caches -- ground-truth SSIM moments, the
    # capacity guess, the image-workspace lease -- all hit every step there; the headline above proves them across cameras
    if len(pool) > 1:
        e1, _, p1 = timed_steps_2(model, pool[:1], V, 3, K, it0=Wm + K)
        out["fixed_camera_step"] = {"ms_per_step": round(1e3 * e1 / K, 4), "ms_per_step_passes": p1, "steps": K,
                                    "headline_over_fixed": round(ms_per_step / (1e3 * e1 / K), 4)}

    # ---- ... and with the stage-1 loop's per-iteration densification statistics (train_gaussians.py:161-165: every iteration
    # below densify_until_iter, half of a run) kept by k_project_bwd itself
    if world == 1 and len(pool) > 1:
        def stats_steps(n_warm, n_steps, it0):
            for i in range(n_warm + n_steps):
                if i == n_warm:
                    sync_all()
                    t_ = time.perf_counter()
                training_step(model, [pool[(i * V + j) % len(pool)] for j in range(V)], bg, opt, it0 + i + 1,
                              global_views=V * world, streams=args.streams, densify_stats=True)
            sync_all()
            return time.perf_counter() - t_
        e2a, e2b = stats_steps(3, K, Wm + 3 * K + 6), stats_steps(0, K, Wm + 4 * K + 9)
        e2 = min(e2a, e2b)
        out["densify_stats_step"] = {"ms_per_step": round(1e3 * e2 / K, 4),
                                     "ms_per_step_passes": [round(1e3 * e2a / K, 4), round(1e3 * e2b / K, 4)], "steps": K,
                                     "over_headline_us": round(1e3 * (1e3 * e2 / K - ms_per_step), 2),
                                     "seen_fraction": round(float((model.denom > 0).float().mean().item()), 4)}

    # ---- BASELINE configs[3]'s per-GPU shard: VS views per GPU per global step (every N; same model, continues training)
    if VS > 0 and VS != V:
        K4 = max(5, K // 2)
        # (two timed passes, the faster one reported and both listed: a side block of ten steps lasts 25 ms, and one run in five
        # a disturbance of the box -- not of this process: `host_gc` -- lands in one of them; the HEADLINE above is K steps, once)
        dt4, used4, passes4 = timed_steps_2(model, pool, VS, 5, K4, it0=Wm + 5 * K + 12)
        dt4 /= K4
        pv4 = torch.tensor([float(sum(P_vis[c] for vs in used4 for c in vs)) / K4], dtype=torch.float64, device=dev)
        if world > 1:
            dist.all_reduce(pv4)
        out["config4_shard"] = {"workload": "BASELINE configs[3] shard: %d views per GPU per gradient step (%d global)" %
                                            (VS, VS * world), "steps": K4, "ms_per_step": round(1e3 * dt4, 4),
                                "ms_per_step_passes": passes4,
                                "gaussians_per_sec": round(float(pv4.item()) / dt4, 1),
                                "grad_steps_per_sec": round(1.0 / dt4, 3)}
    # ---- N > 1: what the scaling curve is made of (VERDICT r2 next #6b).  Measured with HIP events on this rank's
    # stream, max over ranks; outside the timed regions above (the buffers hold zeros: the values do not matter).
    if world > 1 or os.environ.get("GHR_FORCE_COLLECTIVES") == "1":
        o = model.optimizer
        o.active_rest_coeffs = (int(model.active_sh_degree) + 1) ** 2 - 1
        msg = sum((b - a) for a, b, how in o._reduce_plan(4) if how == "sum") + \
            sum(how[1] * how[3] * 3 for a, b, how in o._reduce_plan(4) if isinstance(how, tuple))

        def timed(fn, n=7):
            ts = []
            for _ in range(n):
                torch.cuda.synchronize()
                if world > 1:
                    dist.barrier()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
            ts.sort()
            t = torch.tensor([ts[len(ts) // 2]], dtype=torch.float64, device=dev)
            if world > 1:
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return float(t.item())

        # (the timing lambdas run ~40 optimizer passes over zero gradients -- moments decay, the step counter advances: the
        # optimizer is put back afterwards so that what follows sees the state the timed steps left)
        o.sync_moments()
        snap = [t.detach().clone() for t in (o.flat_param, o.exp_avg, o.exp_avg_sq, o.state_dev)]
        ar_ms = timed(lambda: o.all_reduce())                                      # the gradient message alone
        adam_ms = timed(lambda: o.step_chunked(chunks=4, zero_grad=True, reduce=False))  # the local update alone
        both_ms = timed(lambda: o.step_chunked(chunks=4, zero_grad=True, reduce=True, shard=False))  # replicated update
        zero_ms = timed(lambda: o.step_chunked(chunks=4, zero_grad=True, reduce=True, shard=True))   # ZeRO-1, as in the step
        from gaussianhaircut_amd.optim import FusedAdam as _FA
        Gw, rk = (dist.get_world_size(), dist.get_rank()) if dist.is_initialized() else (1, 0)
        shards = [(a, b) for a, b, how in _FA._shard_plan(o._reduce_plan(4), Gw) if how == "shard"]

        def rs():
            for a, b in shards:
                L = (b - a) // Gw
                dist.reduce_scatter_tensor(o.flat_grad[a + rk * L: a + (rk + 1) * L], o.flat_grad[a:b])

        def ag():
            for a, b in shards:
                L = (b - a) // Gw
                dist.all_gather_into_tensor(o.flat_param[a:b], o.flat_param[a + rk * L: a + (rk + 1) * L])
        rs_ms, ag_ms = (timed(rs), timed(ag)) if dist.is_initialized() else (None, None)
        # the headline step's message since ABI 19: SH gradients as per-view dL/d(rgb) tables (all-gather) + the other 13
        # floats per Gaussian summed; what the step does with V views per rank when V x ranks <= FACTORED_SH_MAX_VIEWS
        from gaussianhaircut_amd import optim as _optim
        fact = None
        if _optim.FACTORED_SH_REDUCE and o.can_factor_views() and V * Gw <= _optim.FACTORED_SH_MAX_VIEWS:
            def factored_step(shard_):
                o.begin_factored_views(V)
                o._views["next"] = V  # (as if V backward passes had filled the slots: zero tables, like the zero gradients)
                try:
                    o.step_chunked(chunks=4, zero_grad=True, reduce=True, shard=shard_)
                finally:
                    o.end_factored_views()
            o.begin_factored_views(V)
            buf = o._views["buf"]
            o.end_factored_views()
            gathered = torch.empty((Gw * buf.shape[0], buf.shape[1]), dtype=torch.float32, device=dev)
            gather_ms = timed(lambda: dist.all_gather_into_tensor(gathered, buf)) if dist.is_initialized() else None
            o.begin_factored_views(V)
            rebuild_ms = timed(lambda: o._rebuild_sh_from_views(gathered))
            plan_f = o._reduce_plan(4)
            o.end_factored_views()
            fact = {"views_per_rank": V, "views_gathered": V * Gw,
                    "all_gather_bytes_per_rank": int(4 * buf.numel()),
                    "summed_floats_per_gaussian": round(sum(b - a for a, b, how in plan_f if how == "sum") / max(int(model.get_xyz.shape[0]), 1), 2),
                    "all_gather_ms": round(gather_ms, 4) if gather_ms is not None else None,
                    "rebuild_ms": round(rebuild_ms, 4),
                    "step_chunked_replicated_ms": round(timed(lambda: factored_step(False)), 4),
                    "step_chunked_sharded_ms": round(timed(lambda: factored_step(True)), 4),
                    "bytes_on_wire_per_gpu_ring": int((Gw - 1) / Gw * Gw * 4 * buf.numel() +
                                                      2 * (Gw - 1) / Gw * 4 * sum(b - a for a, b, how in plan_f if how == "sum"))}
        o.sync_moments()
        for dst, src in zip((o.flat_param, o.exp_avg, o.exp_avg_sq, o.state_dev), snap):
            dst.copy_(src)
        o.zero()
        G = max(world, 1)
        shard = out.get("config4_shard")
        out["scaling_breakdown"] = {
            "figure": "config4_shard.gaussians_per_sec (BASELINE configs[3]: %d views per GPU per step, weak scaling): "
                      "divide by N x the N = 1 run's config4_shard.gaussians_per_sec; the headline `value` is the "
                      "1-view-per-GPU step of configs[2], whose weak-scaling ceiling is set by the 244 B per Gaussian "
                      "gradient message (DESIGN.md 6)" % VS,
            "config4_shard_gaussians_per_sec": shard["gaussians_per_sec"] if shard else None,
            "config4_shard_ms_per_step": shard["ms_per_step"] if shard else None,
            "headline_ms_per_step": round(ms_per_step, 4),
            "all_reduce_ms": round(ar_ms, 4), "adam_ms": round(adam_ms, 4), "all_reduce_plus_adam_chunked_ms": round(both_ms, 4),
            "reduce_scatter_ms": round(rs_ms, 4) if rs_ms is not None else None,
            "all_gather_ms": round(ag_ms, 4) if ag_ms is not None else None,
            "reduce_scatter_adam_slice_all_gather_chunked_ms": round(zero_ms, 4),
            # what the chunked forms hide: (collective alone + Adam alone) - (the two interleaved chunk by chunk).  The collective
            # itself cannot start before the step's LAST view has added its gradients (every element of the buffer is a sum
            # over the rank's views): only the optimizer pass, not the backward pass, can run under it
            "overlap_hidden_ms": round(max(0.0, ar_ms + adam_ms - both_ms), 4),
            "overlap_hidden_ms_sharded": round(max(0.0, (rs_ms or 0.0) + (ag_ms or 0.0) + adam_ms / G - zero_ms), 4)
            if rs_ms is not None and ag_ms is not None else None,
            "optimizer": "sharded update (FusedAdam.step_chunked(shard=True), the communication pattern of ZeRO-1; moments stay "
                         "allocated in full): each rank updates 1 / N of every reduced range",
            "message_bytes": int(4 * msg), "bytes_on_wire_per_gpu_ring": int(2 * (G - 1) / G * 4 * msg),
            "bus_bandwidth_GBps": round(2 * (G - 1) / G * 4 * msg / (ar_ms * 1e-3) / 1e9, 2) if ar_ms > 0 and G > 1 else None,
            "factored_sh_message": fact,
            "backend": dist.get_backend() if dist.is_initialized() else None, "replicas_identical": replicas_identical,
            "note": "HIP events on the rank's stream, median of 7, max over ranks; no curve is computed here (the driver "
                    "divides the per-N lines)"}

    # ---- BASELINE configs[4]'s model: 2M strand Gaussians ("after densify / clone"), one 1080p view per step, N = 1 -------------
    if world == 1 and not args.no_2m and args.workload == "cfg3":
        spec5 = syn.CONFIGS["cfg5"]
        m5, pool5 = build_scene(spec5, 1)
        K5 = 10
        e5, _, passes5 = timed_steps_2(m5, pool5, 1, 8, K5)
        solo5 = solo_kernel_times(m5, pool5, 10, 1)
        b5 = sum(s_[1] for s_ in solo5) / len(solo5)
        f5 = sum(s_[0] for s_ in solo5) / len(solo5)
        R5 = solo5[0][2]
        pv5 = visible(m5, pool5)[0]
        by5 = 132 * R5 + 48 * N_pix + 8 * T_tiles
        out["config5_2M"] = {"workload": "BASELINE configs[4] model: %s, %d Gaussians, 1 view %dx%d per gradient step (render + 4 "
                                         "losses + backward + Adam), 1 GPU" % (spec5.name, spec5.P, spec5.W, spec5.H),
                             "steps": K5, "ms_per_step": round(1e3 * e5 / K5, 4), "ms_per_step_passes": passes5,
                             "P_visible": pv5, "num_rendered": R5,
                             "gaussians_per_sec": round(pv5 / (e5 / K5), 1),
                             "k_render_fwd_ms": round(f5, 4), "k_render_bwd_ms": round(b5, 4),
                             "k_render_bwd_algorithmic_bytes": by5,
                             "k_render_bwd_hbm_frac": round(by5 / (b5 * 1e-3) / 1e9 / HBM_PEAK_GBS, 5) if b5 > 0 else None}
        del m5, pool5
        torch.cuda.empty_cache()

    # ---- the reference's DEFAULT run trains its cameras (src/arguments/__init__.py:61-62, run.sh:112-115): the same configs[2]
    # step with camera parameters that require grad -- the fused path returns the camera gradients itself (ABI 17), N = 1
    if world == 1 and not args.no_camera_block:
        import copy
        blk = {"workload": "BASELINE configs[2] step with trainable cameras: the fused projection backward also reduces dL/d(world_view_"
                           "transform, full_proj_transform, camera_center, tan FoV) (k_project_bwd<CAM> + k_cam_fold)"}
        # (a) the five camera tensors themselves are leaves that require grad: the cost of the kernels alone
        leaf_pool = []
        for c in pool:
            c2 = copy.copy(c)
            for n in ("world_view_transform", "full_proj_transform", "camera_center", "FoVx", "FoVy"):
                setattr(c2, n, getattr(c, n).detach().clone().requires_grad_(True))
            leaf_pool.append(c2)

        def drop_cam_grads(cams_):
            for c in cams_:
                for n in ("world_view_transform", "full_proj_transform", "camera_center", "FoVx", "FoVy"):
                    getattr(c, n).grad = None
        ea, _, pa = timed_steps_2(model, leaf_pool, V, 3, K, it0=10_000, after_step=drop_cam_grads)
        blk["leaf_camera_tensors"] = {"ms_per_step": round(1e3 * ea / K, 4), "ms_per_step_passes": pa,
                                      "over_headline": round(1e3 * ea / K / ms_per_step, 4)}
        # (b) pose / FoV residuals as parameters (scene.cameras.TrainableCamera: the reference's ortho-6D + translation + FoV
        # residuals, cameras.py:85-117), composed with PyTorch ops under autograd, stepped by an Adam of their own after the
        # Gaussians' (train_gaussians.py:45-60,183-196: three groups, eps 1e-15)
        mC, poolC = build_scene(spec, NC, cls=TrainableCamera)
        cam_opt = torch.optim.Adam([{"params": [c._rotation_res for c in poolC], "lr": 0.001, "name": "rotation"},
                                    {"params": [c._translation_res for c in poolC], "lr": 0.0016, "name": "translation"},
                                    {"params": [c._fov_res for c in poolC], "lr": 0.001, "name": "fov"}], lr=0.0, eps=1e-15)

        def cam_step(_cams):
            cam_opt.step()
            cam_opt.zero_grad(set_to_none=True)
        eb, _, pb = timed_steps_2(mC, poolC, V, 3, K, after_step=cam_step)
        blk["residual_parameters"] = {"ms_per_step": round(1e3 * eb / K, 4), "ms_per_step_passes": pb,
                                      "over_headline": round(1e3 * eb / K / ms_per_step, 4),
                                      "camera_moved": bool(poolC[0]._translation_res.detach().abs().max().item() > 0),
                                      "note": "camera matrices composed from the residuals by ~40 small PyTorch kernels per view "
                                              "(forward + autograd) and a torch.optim.Adam over the camera parameters: camera-"
                                              "side work outside the hot path (cameras.py is out of scope, DESIGN.md 8)"}
        out["dropin_trainable_camera_step"] = blk
        del mC, poolC
        torch.cuda.empty_cache()

    # ---- the strand stage (src/train_strands.py:98-160; reference size: 30 000 strands x 99 segments + the frozen head): one
    # iteration = rebuild the strand Gaussians, render_hair (two fused segments of one rasterizer state), the strand-stage loss,
    # backward to the strand parameters, Adam -- fused against the generic PyTorch projection path, N = 1
    if world == 1 and not args.no_strand_block and args.workload == "cfg3":
        from gaussianhaircut_amd.gaussian_renderer import render_hair
        from gaussianhaircut_amd.scene.gaussian_model_strands import GaussianModelStrands
        from gaussianhaircut_amd.trainer import strand_training_step
        from types import SimpleNamespace
        torch.cuda.empty_cache()
        S, n_seg, n_head = 30_000, 99, 100_000
        head = syn.make_model(spec, dev)
        with torch.no_grad():
            head._label[:n_head] = -4.0
            head._label[n_head:] = 4.0
        head.precompute_head()
        g = torch.Generator().manual_seed(9)
        unit = torch.nn.functional.normalize
        origins = unit(torch.randn(S, 1, 3, generator=g), dim=-1)
        dirs = torch.randn(S, n_seg, 3, generator=g) * 0.003 + unit(torch.randn(S, 1, 3, generator=g), dim=-1) * 0.01
        feats = torch.randn(S * n_seg, 16, 3, generator=g) * 0.1
        hair = GaussianModelStrands(3).create_from_strands(origins.to(dev), dirs.to(dev), feats.to(dev))
        hcam = pool[0]
        sopt = OptimizationParams()
        sopt.lambda_dorient, sopt.lambda_dmask = 0.1, 0.1  # run.sh:177
        fusedp, genericp = SimpleNamespace(debug=False, fused_projection=True), SimpleNamespace(debug=False, fused_projection=False)
        saved_gt = (hcam.original_image, hcam.original_mask, hcam.original_orient_angle, hcam.original_orient_conf)
        with torch.no_grad():
            hair.initialize_gaussians_hair()
            hp_ = render_hair(hcam, head, hair, fusedp, bg)
            hcam.original_image, hcam.original_mask = hp_["render"].clamp(0, 1).detach(), hp_["mask"].clamp(0, 1).detach()
            hcam.original_orient_angle = hp_["orient_angle"].detach()
            hcam.original_orient_conf = torch.ones_like(hp_["orient_conf"]).detach()
            hair._dirs.mul_(1.02)  # (train towards the unperturbed strands)
        hair.training_setup(sopt)

        def strand_ms(pipe_, n_warm, n_it):
            for i in range(n_warm + n_it):
                if i == n_warm:
                    torch.cuda.synchronize()
                    gc_log["timed"] = True
                    t_ = time.perf_counter()
                strand_training_step(head, hair, [hcam], bg, sopt, i + 1, pipe=pipe_)
            torch.cuda.synchronize()
            dt_ = time.perf_counter() - t_
            gc_log["timed"] = False
            return 1e3 * dt_ / n_it
        f_ms = strand_ms(fusedp, 4, 12)
        g_ms = strand_ms(genericp, 1, 3)
        out["strand_stage"] = {"workload": "train_strands.py iteration shape: %d strands x %d segments + %d frozen head Gaussians = %d "
                                           "Gaussians, 1 view %dx%d: initialize_gaussians_hair + render_hair + strand-stage loss + "
                                           "backward + Adam" % (S, n_seg, n_head, S * n_seg + n_head, spec.W, spec.H),
                               "ms_per_iteration_fused": round(f_ms, 3), "ms_per_iteration_generic_projection": round(g_ms, 2),
                               "generic_over_fused": round(g_ms / f_ms, 1)}
        (hcam.original_image, hcam.original_mask, hcam.original_orient_angle, hcam.original_orient_conf) = saved_gt
        del head, hair
        torch.cuda.empty_cache()

    if rank == 0 and world == 1:
        if not args.no_op_only:
            out["op_only"] = {c: op_only_bench(dev, c, iters=50 if c == "cfg2" else 30) for c in ("cfg2", "cfg3")}
        if not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline("cfg3")
    out["host_gc"] = {"full_collections_inside_timed_regions": gc_log["gen2_collections"],
                      "ms_in_all": round(gc_log["gen2_ms"], 2), "longest_ms": round(gc_log["longest_ms"], 2)}
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


DUMP_ROWS = 1 << 17  # Gaussians sampled by dump_outputs: 61 floats each, 32 MB in all
DUMP_SEED = 20260


def dump_outputs(dirname, model, loss):
    """What a caller of the timed path holds after its last timed step, as DIR/<name>.npy (float32): ``loss`` (what
    training_step returned) and the eight parameter tensors of the model after that step's Adam update (main() hands it
    the model of its bit-reproducible replay of the timed steps).  The parameters
    are sampled: the same DUMP_ROWS Gaussians of the model, chosen by a CPU generator seeded with DUMP_SEED, in
    ascending index order (all of them when the model is smaller)."""
    import numpy as np
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    os.makedirs(dirname, exist_ok=True)
    params = {"xyz": model._xyz, "features_dc": model._features_dc, "features_rest": model._features_rest,
              "opacity": model._opacity, "label": model._label, "scaling": model._scaling, "rotation": model._rotation,
              "orient_conf": model._orient_conf}
    P = int(model._xyz.shape[0])
    g = torch.Generator(device="cpu").manual_seed(DUMP_SEED)
    rows = torch.randperm(P, generator=g)[:DUMP_ROWS].sort().values if P > DUMP_ROWS else torch.arange(P)
    for name, t in params.items():
        a = t.detach().index_select(0, rows.to(t.device)).float().cpu().numpy()
        np.save(os.path.join(dirname, name + ".npy"), a)
    np.save(os.path.join(dirname, "loss.npy"), np.asarray(loss.detach().float().cpu().numpy(), dtype=np.float32))


def op_only_bench(dev, cfg="cfg2", iters=50, warm=10):  # 10 warm-up + 50 timed, median and p10 / p90
    """Rasterizer op alone -- the product's GaussianRasterizer autograd op (mode A: conic + colours precomputed, what
    render() hands it), forward and backward: BASELINE.json configs[1], Gaussians / (t_fwd + t_bwd)."""
    from gaussianhaircut_amd import diff_gaussian_rasterization as dgr
    from gaussianhaircut_amd.utils import synthetic as syn
    spec = syn.CONFIGS[cfg]
    ri = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in syn.raster_inputs(spec).items()}
    dL = (syn.grad_image(spec, 101) * (spec.H * spec.W)).to(dev).contiguous()
    rs = dgr.GaussianRasterizationSettings(image_height=spec.H, image_width=spec.W, tanfovx=ri["tanfovx"],
                                           tanfovy=ri["tanfovy"], bg=ri["bg"], scale_modifier=1.0,
                                           viewmatrix=ri["viewmatrix"], projmatrix=ri["projmatrix"], sh_degree=3,
                                           campos=ri["campos"], prefiltered=True, debug=False)
    rast = dgr.GaussianRasterizer(rs)
    leaves = {k: ri[k].clone().requires_grad_(True) for k in ("means3D", "means2D", "colors", "opacities", "conic")}
    # One event triple per iteration, read back after the loop: the host is not stalled between iterations (a training
    # loop is not either), so the Python work of call i+1 -- argument structs, workspace tensors -- is done while the GPU
    # is still busy with the backward of call i.  The forward's own blocking read of num_rendered stays where it is.
    def run(n_it, sync_each):
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(n_it + warm)]
        for i in range(n_it + warm):
            for t in leaves.values():
                t.grad = None
            e = ev[i]
            e[0].record()
            color, radii = rast(means3D=leaves["means3D"], means2D=leaves["means2D"], shs=None,
                                colors_precomp=leaves["colors"], opacities=leaves["opacities"], cov3D_precomp=ri["cov3D"],
                                conic_precomp=leaves["conic"])
            e[1].record()
            torch.autograd.backward(color, grad_tensors=dL)
            e[2].record()
            if sync_each:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        f = sorted(e[0].elapsed_time(e[1]) for e in ev[warm:])
        b = sorted(e[1].elapsed_time(e[2]) for e in ev[warm:])
        return f, b
    tf, tb = run(iters, False)
    mf, mb = tf[len(tf) // 2], tb[len(tb) // 2]
    # ... and with the host waiting for the GPU after every iteration (how rounds 1-2 and a cold single call measure: the
    # Python work of a call is then NOT hidden behind the previous backward)
    sf, sb = run(max(iters // 2, 10), True)
    pct = lambda v, q: round(v[min(len(v) - 1, int(q * len(v)))], 4)
    R = dgr.LAST_STATS["num_rendered"]
    P, N, T = ri["P"], spec.W * spec.H, ((spec.W + 15) // 16) * ((spec.H + 15) // 16)
    b_fwd, b_bwd = 92 * P + 112 * R + 48 * N + 16 * T, 140 * P + 132 * R + 48 * N + 8 * T
    return {"workload": spec.name, "P": ri["P"], "num_rendered": R, "fwd_ms": round(mf, 4),
            "bwd_ms": round(mb, 4), "gaussians_per_sec_fwd_bwd": round(ri["P"] / ((mf + mb) * 1e-3), 1),
            "whole_forward_hbm_frac": round(b_fwd / (mf * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
            "whole_backward_hbm_frac": round(b_bwd / (mb * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
            "algorithmic_bytes": {"B_fwd = 92 P + 112 R + 48 N + 16 T": b_fwd, "B_bwd = 140 P + 132 R + 48 N + 8 T": b_bwd},
            "fwd_ms_p10_p90": [pct(tf, 0.1), pct(tf, 0.9)], "bwd_ms_p10_p90": [pct(tb, 0.1), pct(tb, 0.9)],
            "fwd_ms_host_sync_every_iter": round(sf[len(sf) // 2], 4), "bwd_ms_host_sync_every_iter": round(sb[len(sb) // 2], 4),
            "iters": iters, "warmup": warm,
            "note": "GaussianRasterizer op (autograd, workspace allocation and the num_rendered read included); HIP events per "
                    "iteration, no host synchronisation between iterations"}


def cpu_baseline(cfg="cfg3"):
    """The oracle (CPU restatement of the reference's CUDA semantics, pinned to outputs of the reference's own rasterizer;
    'port') on the same scope as op_only[cfg]: rasterizer forward + backward of one view, mode A."""
    import oracle
    from gaussianhaircut_amd.utils import synthetic as syn
    from tests import helpers as hp
    spec = syn.CONFIGS[cfg]
    ri = syn.raster_inputs(spec, "cpu")
    dL = syn.grad_image(spec, 101).numpy() * (spec.H * spec.W)
    best = None
    for _ in range(3):  # bounded sample: three passes over one view (~1 s each on a 128-core host), best pass reported
        t0 = time.perf_counter()
        out_o, radii_o, st = hp.oracle_forward(oracle, ri, "A")
        t1 = time.perf_counter()
        hp.oracle_backward(oracle, st, ri, dL, "A")
        t2 = time.perf_counter()
        if best is None or t2 - t0 < best[2] - best[0]:
            best = (t0, t1, t2)
    t0, t1, t2 = best
    return {"value": round(ri["P"] / (t2 - t0), 1), "unit": "Gaussians/s", "cores": oracle.num_threads(), "kind": "port",
            "sample": "1 view of %s (P = %d Gaussians handed to the op), best of 3 passes, rasterizer fwd (%.2f s) + bwd "
                      "(%.2f s): the scope of op_only.%s" % (spec.name, ri["P"], t1 - t0, t2 - t1, cfg)}


if __name__ == "__main__":
    main()
