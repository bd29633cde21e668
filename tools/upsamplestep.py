"""Time of groom upsampling (gaussianhaircut_amd.strand_upsampling; csrc/ghr_upsample.h), HIP against the
PyTorch-composed form, in ONE process on one GPU:

    python tools/upsamplestep.py [out-file, default profiles/strand_upsampling.txt]

The workload: 30 000 guides of 100 points grown on the 9976-face UV sphere (tools/synthetic_capture.py's grown_hair), their frames
those of the sphere's faces nearest to their roots (frames_at); 150 000 children drawn on the sphere by sample_roots; 3 features.
  search    ghr_upsample_neighbours alone (guide_neighbours)
  blend     ghr_upsample_blend alone (upsample_strands with the table handed over and eps2 given)
  whole     upsample_strands as a caller uses it: default eps2 (a nearest_roots over the guides), search, blend
  composed  the PyTorch form on the first UPSAMPLESTEP_SLICE children against all guides; scaled to all children it is printed as
            EXTRAPOLATED (both its parts are linear in the children)
The forms alternate in one call, three rounds; each figure is the device time between two events, the median of the rounds.  The
floors beside the figures are DERIVED, not measured, and no time is a pass/fail condition."""
import importlib.util
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussianhaircut_amd import strand_generator as sgen  # noqa: E402
from gaussianhaircut_amd import strand_upsampling as su  # noqa: E402
from gaussianhaircut_amd.mesh import HeadMesh  # noqa: E402

ROUNDS = 3
HBM = 6.29e12                        # bytes per second, the figure the other floors use
LANE_RATE = 256 * 4 * 16 * 2.4e9     # fp32 vector operations per second: 256 CUs x 4 SIMDs x 16 lanes a clock at 2.4 GHz
OPS_PER_PAIR = 8                     # three subtractions, three multiplies, two additions; the compare and insert are left out


def timed(fn, n=1):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def scene(G, L, N, dev):
    spec = importlib.util.spec_from_file_location("synthetic_capture_tool", os.path.join(ROOT, "tools", "synthetic_capture.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    v, f = tool.uv_sphere(116, 44)
    uv = np.stack([np.arctan2(v[:, 2], v[:, 0]) / (2 * np.pi) + 0.5, np.arccos(np.clip(v[:, 1], -1, 1)) / np.pi], 1).astype(np.float32)
    vt, ft, uvt = torch.from_numpy(v), torch.from_numpy(f.astype(np.int64)), torch.from_numpy(uv)
    guides = torch.from_numpy(tool.grown_hair(G, L, 1)).to(dev)
    roots = sgen.sample_roots(vt, ft, uvt, N, generator=torch.Generator().manual_seed(4))
    frames = su.frames_at(HeadMesh(v, f), sgen.scalp_frames(vt, ft, uvt), guides[:, 0])
    feats = torch.rand(G, 3, generator=torch.Generator().manual_seed(5)).to(dev)
    return guides, frames, roots["origins"].to(dev).contiguous(), roots["local2world"].to(dev).contiguous(), feats


def main():
    assert torch.cuda.is_available(), "upsamplestep needs a ROCm GPU (a CPU run measures nothing)"
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "strand_upsampling.txt")
    dev = torch.device("cuda:0")
    G, L = int(os.environ.get("UPSAMPLESTEP_GUIDES", 30000)), int(os.environ.get("UPSAMPLESTEP_POINTS", 100))
    N, SL = int(os.environ.get("UPSAMPLESTEP_CHILDREN", 150000)), int(os.environ.get("UPSAMPLESTEP_SLICE", 4096))
    SL = min(SL, N)
    gp, gM, co, cM, gf = scene(G, L, N, dev)
    groots = gp[:, 0].contiguous()
    med = statistics.median
    fmt = lambda xs: " / ".join("%.3f" % x for x in xs)  # noqa: E731
    spread = lambda xs: (max(xs) - min(xs)) / med(xs) * 100  # noqa: E731
    lines = ["groom upsampling: %d guides x %d points, %d children, 3 features, tau %.2f, no radius" % (G, L, N, su.TAU),
             "device: %s, torch %s; device time between two events, %d alternating rounds" % (torch.cuda.get_device_name(0), torch.__version__, ROUNDS)]
    eps2 = su.default_eps2(groots)
    table = su.guide_neighbours(groots, co)
    full = su.upsample_strands(gp, gM, co, cM, features=gf, eps2=eps2, neighbours=table)
    part = su.upsample_strands(gp, gM, co[:SL], cM[:SL], features=gf, eps2=eps2, fused=False)
    same = torch.equal(part["nbr"], table[0][:SL])
    used = (full["weights"] > 0).sum(1).float()
    lines.append("MEASURED: eps2 %.5g; guides carrying weight per child: mean %.2f; children gated down to one guide: %d of %d"
                 % (eps2, float(used.mean()), int((used == 1).sum()), N))
    lines.append("MEASURED: on the first %d children the HIP search and the composed one give %s table; points differ by at most %.3g "
                 "(strands reach %.3g from the centre), weights by %.3g"
                 % (SL, "the same" if same else "a DIFFERENT", float((part["points"] - full["points"][:SL]).abs().max()),
                    float(full["points"].norm(dim=-1).max()), float((part["weights"] - full["weights"][:SL]).abs().max())))
    assert same
    forms = {"search fused": (lambda: su.guide_neighbours(groots, co), 2, 1.0),
             "blend fused": (lambda: su.upsample_strands(gp, gM, co, cM, features=gf, eps2=eps2, neighbours=table), 10, 1.0),
             "whole fused": (lambda: su.upsample_strands(gp, gM, co, cM, features=gf), 2, 1.0),
             "search composed": (lambda: su.guide_neighbours(groots, co[:SL], fused=False), 1, N / SL),
             "blend composed": (lambda: su.upsample_strands(gp, gM, co[:SL], cM[:SL], features=gf, eps2=eps2,
                                                            neighbours=(table[0][:SL], table[1][:SL]), fused=False), 1, N / SL)}
    rounds = {k: [] for k in forms}
    for fn, _, _ in forms.values():
        fn()
    for _ in range(ROUNDS):
        for k, (fn, n, _) in forms.items():
            rounds[k].append(timed(fn, n))
    for k, (_, _, scale) in forms.items():
        if scale == 1.0:
            lines.append("MEASURED: %-16s median %.3f ms   rounds %s   spread %.1f %%" % (k, med(rounds[k]), fmt(rounds[k]), spread(rounds[k])))
        else:
            lines.append("MEASURED: %-16s median %.3f ms on %d children   rounds %s   spread %.1f %%   EXTRAPOLATED to %d children: %.1f ms"
                         % (k, med(rounds[k]), SL, fmt(rounds[k]), spread(rounds[k]), N, med(rounds[k]) * scale))
    s_f, b_f = med(rounds["search fused"]), med(rounds["blend fused"])
    lines.append("EXTRAPOLATED composed / MEASURED fused: search %.0fx, blend %.0fx"
                 % (med(rounds["search composed"]) * N / SL / s_f, med(rounds["blend composed"]) * N / SL / b_f))
    pairs = float(G) * N
    floor_s = pairs * OPS_PER_PAIR / LANE_RATE * 1e3
    wr = 12.0 * N * L + 4.0 * N * (4 + 3) + N
    rd = 4 * 12.0 * N * L
    lines.append("DERIVED search floor: %.2f G pairs x %d lane operations at %.1f T lane operations/s = %.3f ms; the search runs at %.0f %% of it"
                 % (pairs / 1e9, OPS_PER_PAIR, LANE_RATE / 1e12, floor_s, floor_s / s_f * 100))
    lines.append("DERIVED blend floors at %.2f TB/s: %.1f MB written = %.4f ms if only the writes reach HBM (the %.1f MB of guide rows are "
                 "mostly served from cache); %.4f ms if each of the four guide rows a child reads (%.1f MB) came from HBM too.  The blend "
                 "runs at %.0f %% of the first and %.0f %% of the second."
                 % (HBM / 1e12, wr / 1e6, wr / HBM * 1e3, 12.0 * G * L / 1e6, (wr + rd) / HBM * 1e3, rd / 1e6, wr / HBM * 1e3 / b_f * 100,
                    (wr + rd) / HBM * 1e3 / b_f * 100))
    lines.append("NOT MEASURED: the blend with the guide rows kept in registers between its two passes; any size but this one; the "
                 "composed form on all children (its [N, 4, L, 3] gather is %.0f MB)." % (4 * 12.0 * N * L / 1e6))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
