"""Build-time guard for the kernels that walk a tile's list (csrc/ghr_tilelists.h's tl_walk: k_vis_raster, k_sv_raster, k_sv_layers) and
for the shadowed shade (csrc/ghr_strandview.h): k_sv_layers keeps its front plane and its four counters in registers across two
walks, the rasters their winner, and k_sv_shade_shadowed gathers a texel's counts into registers -- none may get a private segment (an
array the compiler could not promote, or a spill).  Reads the kernel descriptors of the device code cross-compiled to assembly (no
GPU needed), as tests/test_kernel_resources.py does."""
import pytest

from tests.test_kernel_resources import _descriptors


@pytest.mark.parametrize("kernel,vgprs,lds", [("k_sv_layers", 64, 2 * 128 * 16), ("k_sv_shade_shadowed", 128, 0),
                                              ("k_vis_raster", 64, 3 * 64 * 16 + 64 * 4), ("k_sv_raster", 64, 2 * 128 * 16 + 128 * 4)])
def test_shadow_kernels_compile_without_scratch_or_spills(kernel, vgprs, lds):
    meta = _descriptors()
    ks = [v for k, v in meta.items() if kernel in k]
    assert len(ks) == 1, (kernel, [k for k in meta if kernel in k])
    k = ks[0]
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["vgpr_count"] <= vgprs, k                   # the walks: eight waves per SIMD; the shade: four
    assert k["group_segment_fixed_size"] == lds, k       # the staged records and their ids (k_sv_layers keeps no ids)
