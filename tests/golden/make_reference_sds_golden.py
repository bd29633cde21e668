"""Generates tests/golden/reference_sds_golden.npz by running THE REFERENCE'S OWN ``initialize_gaussians_hair`` with
``use_sds = True`` (src/scene/gaussian_model_strands.py:435-515, read-only, imported from /root/reference/src) on the CPU.  Run
once in the build container (the reference does not exist where the GPU tests run; the committed .npz is what the tests read):

    python tests/golden/make_reference_sds_golden.py

The module's imports are stubbed and ``__init__`` bypassed as in make_reference_golden.py.  Stand-ins, all seeded:
``strands_encoder`` = tanh(flatten(p) @ W); ``strands_generator`` = a namespace with ``scale_decoder``, ``diffusion_input = 32``,
``diffuse_mask = None``, ``sample_density`` and ``model_ema.loss_wo_logvar`` = ((texture - T0)^2).mean(dim=(1, 2, 3)), which also
captures the texture.  The method hard-codes device="cuda" in ``torch.randint`` and ``torch.linspace``: inside this script only,
both are redirected to the CPU, and ``randint`` returns randperm(S)[:1000] -- no strand twice, so the reference's unstable sort
decides nothing.  Its literals force N = 1000, n = 99, G >= 32.  Inputs: tests/sds_cases.py ``recipe`` (S = 1200).

What is stored (float32 run), whole: the inputs (uvs, local2world, origins, dirs, W, T0, idx), the texture, the loss and d_dirs --
its 1000 drawn rows; the script asserts that every other row is zero.  The arrays go into five files, none above 1 MiB:
reference_sds_golden.npz (everything small), reference_sds_golden_dirs_{a,b}.npz (the strands' halves) and
reference_sds_golden_ddirs_{a,b}.npz (the halves of the drawn rows of d_dirs, in the order of idx).  The float64 run of the same
method is printed next to it.  Nothing from the reference is copied into the repository -- only numeric outputs.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference/src"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import sds_cases as sc  # noqa: E402


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _run(ref_gms, inp, W, T0, idx, scale, dtype):
    cast = lambda t: t.to(dtype)  # noqa: E731
    m = object.__new__(ref_gms.GaussianModelCurves)
    m.setup_functions()
    m.active_sh_degree = m.max_sh_degree = 3
    m.pts_origins = cast(inp["origins"])
    m._dirs = cast(inp["dirs"]).clone().requires_grad_(True)
    m.scale, m.use_sds = 1e-3, True
    m.num_strands = inp["dirs"].shape[0]
    m.uvs, m.local2world = cast(inp["uvs"]), cast(inp["local2world"])
    m.strands_encoder = lambda p: torch.tanh(p.flatten(1) @ cast(W))
    seen = {}

    def loss_wo_logvar(texture, noise, sigma, mask=None, unet_cond=None):
        seen["texture"] = texture.detach().clone()
        return ((texture - cast(T0)) ** 2).mean(dim=(1, 2, 3)), None, None
    m.strands_generator = types.SimpleNamespace(
        scale_decoder=scale, diffusion_input=sc.GOLDEN["G"], diffuse_mask=None,
        sample_density=lambda shape, device=None: torch.ones(shape[0], dtype=dtype),
        model_ema=types.SimpleNamespace(loss_wo_logvar=loss_wo_logvar))
    real_randint, real_linspace = torch.randint, torch.linspace
    torch.randint = lambda low, high, size, device=None: idx.clone()
    torch.linspace = lambda start, end, steps, device=None: real_linspace(start, end, steps).to(dtype)
    try:
        m.initialize_gaussians_hair()
    finally:
        torch.randint, torch.linspace = real_randint, real_linspace
    m.Lsds.backward()
    return seen["texture"], m.Lsds.detach(), m._dirs.grad.detach()


def main():
    assert os.path.isdir(REF), "run in the build container (needs /root/reference)"
    sys.modules["plyfile"] = types.SimpleNamespace(PlyData=None, PlyElement=None)
    knn, knn_c = types.ModuleType("simple_knn"), types.ModuleType("simple_knn._C")
    knn_c.distCUDA2 = None
    sys.modules["simple_knn"], sys.modules["simple_knn._C"] = knn, knn_c
    sys.path.insert(0, REF)
    for m in [k for k in sys.modules if k == "utils" or k.startswith("utils.")]:
        del sys.modules[m]
    for name in ("trimesh", "pysdf", "src", "src.hair_networks", "src.hair_networks.optimizable_textured_strands",
                 "src.hair_networks.strand_prior"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["pysdf"].SDF = None
    sys.modules["src.hair_networks.optimizable_textured_strands"].OptimizableTexturedStrands = None
    sys.modules["src.hair_networks.strand_prior"].Decoder = None
    sys.modules["src.hair_networks.strand_prior"].Encoder = None
    ref_gms = _load("ref_gaussian_model_strands", os.path.join(REF, "scene", "gaussian_model_strands.py"))

    G = sc.GOLDEN
    inp = sc.recipe(G["S"], G["n"], G["seed"])
    W = sc.encoder_weights(G["n"], G["C"], G["seed"])
    T0 = sc.target_texture(G["C"], G["G"], G["seed"])
    idx = torch.randperm(G["S"], generator=torch.Generator().manual_seed(G["seed"] + 3))[:G["N"]]
    tex, loss, dd = _run(ref_gms, inp, W, T0, idx, G["scale"], torch.float32)
    tex64, loss64, dd64 = _run(ref_gms, inp, W, T0, idx, G["scale"], torch.float64)
    print("loss fp32 %.7f / float64 %.7f; texture within %.2e; d_dirs within %.2e of a maximum of %.3g" % (
        float(loss), float(loss64), float((tex - tex64).abs().max()), float((dd - dd64).abs().max()), float(dd64.abs().max())))
    rows = dd[idx]
    rest = torch.ones(G["S"], dtype=torch.bool)
    rest[idx] = False
    assert float(dd[rest].abs().max()) == 0.0 and len(set(idx.tolist())) == G["N"]
    small = dict(uvs=inp["uvs"], local2world=inp["local2world"], origins=inp["origins"], W=W, T0=T0, idx=idx, texture=tex, loss=loss)
    half_s, half_n = G["S"] // 2, G["N"] // 2
    files = {"": small, "_dirs_a": dict(dirs=inp["dirs"][:half_s]), "_dirs_b": dict(dirs=inp["dirs"][half_s:]),
             "_ddirs_a": dict(d_dirs_rows=rows[:half_n]), "_ddirs_b": dict(d_dirs_rows=rows[half_n:])}
    for tag, arrays in files.items():
        path = os.path.join(HERE, "reference_sds_golden%s.npz" % tag)
        np.savez_compressed(path, **{k: v.numpy() for k, v in arrays.items()})
        print("wrote", path, os.path.getsize(path) // 1024, "KiB")
        assert os.path.getsize(path) < (1 << 20)

if __name__ == "__main__":
    main()
