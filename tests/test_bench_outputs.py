"""bench.py's plain / --full split and --dump-outputs, as far as they go without a GPU: the options exist, and the dump is a
fixed float32 sample of the model's parameters plus the step's loss, the same rows on every call, within 64 MB at the
headline's model size."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = ("xyz", "features_dc", "features_rest", "opacity", "label", "scaling", "rotation", "orient_conf")


def _bench():
    sys.path.insert(0, ROOT)
    try:
        import bench
    finally:
        sys.path.remove(ROOT)
    return bench


def test_bench_has_full_and_dump_outputs_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout and "--dump-outputs DIR" in r.stdout


def test_dump_outputs_is_a_fixed_float32_sample(tmp_path, monkeypatch):
    from gaussianhaircut_amd.utils import synthetic as syn
    bench = _bench()
    # the headline's model (cfg3, 500k Gaussians): 61 floats per sampled Gaussian
    assert bench.DUMP_ROWS * 61 * 4 <= 64 << 20
    model = syn.make_model(syn.CONFIGS["tiny"], "cpu")
    P = int(model._xyz.shape[0])
    monkeypatch.setattr(bench, "DUMP_ROWS", P // 4)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, model, torch.tensor(0.5))
    bench.dump_outputs(b, model, torch.tensor(0.5))
    assert sorted(os.listdir(a)) == sorted([n + ".npy" for n in PARAMS + ("loss",)])
    for name in PARAMS + ("loss",):
        x, y = np.load(os.path.join(a, name + ".npy")), np.load(os.path.join(b, name + ".npy"))
        assert x.dtype == np.float32 and np.array_equal(x, y), name
    assert float(np.load(os.path.join(a, "loss.npy"))) == 0.5
    xyz = np.load(os.path.join(a, "xyz.npy"))
    full = model._xyz.detach().numpy()
    assert xyz.shape == (P // 4, 3)
    # rows of the model, each once, in ascending order
    idx = [int(np.flatnonzero((full == r).all(1))[0]) for r in xyz]
    assert idx == sorted(set(idx))
    # a model no larger than the sample is written whole
    monkeypatch.setattr(bench, "DUMP_ROWS", P)
    bench.dump_outputs(str(tmp_path / "c"), model, torch.tensor(0.5))
    assert np.array_equal(np.load(str(tmp_path / "c" / "xyz.npy")), full)
