"""Build-time guard for the kernel of csrc/ghr_grow.h: no scratch, no vector spills, the LDS of ONE tile per wave (the field walk's
points and payload, then the mesh search's records, in the same 3 x 64 float4), registers within four waves per SIMD, and a name
that holds no other kernel's name.  Cross-compiles the device code to assembly (no GPU needed); the counts are in DESIGN.md 8t."""
import re

from tests.test_kernel_resources import _descriptors

KERNEL = "k_grow_guarded"
LDS = 4 * 3 * 64 * 16   # GHR_FIELD_WAVES waves x one shared tile of 3 x 64 float4


def _mine(meta):
    return {k: v for k, v in meta.items() if KERNEL in k}


def test_grow_kernel_compiles_without_scratch_or_vector_spills_and_within_its_budget():
    mine = _mine(_descriptors())
    assert len(mine) == 1, list(mine)
    (name, k), = mine.items()
    print(name, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (name, k)
    assert k["group_segment_fixed_size"] == LDS, (name, k)
    assert k["vgpr_count"] <= 128, (name, k)       # four waves per SIMD
    assert k["max_flat_workgroup_size"] == 256 and k["wavefront_size"] == 64, (name, k)


def test_grow_kernel_name_holds_no_other_kernels_name():
    """the resource tests pick kernels by substring of the mangled name (argument types included): the new name must contain no
    other kernel's name, nor "meshdist", and be contained in none"""
    meta = _descriptors()
    (mine,) = _mine(meta)
    assert re.search(r"k_[a-z0-9_]+", mine).group(0) == KERNEL
    assert "meshdist" not in mine and "GrowArgs" in mine
    for other in meta:
        if other == mine:
            continue
        name = re.search(r"k_[a-z0-9_]+", other)  # the kernel's own name inside the mangled one
        assert name is not None and name.group(0) not in mine, (mine, other)
        assert KERNEL not in other, other
    for sub in ("k_field_pack", "k_field_query", "k_field_trace", "k_strands_resample"):
        assert sub not in mine
