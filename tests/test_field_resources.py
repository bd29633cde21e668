"""Build-time guard for the four kernels of csrc/ghr_field.h: no scratch, no vector spills, the LDS of two tiles per wave (the
block's points and its payload) from the code object's metadata, registers within eight waves per SIMD, and names that hold no
other kernel's name.  Cross-compiles the device code to assembly (no GPU needed); the counts themselves are in DESIGN.md 8s."""
import re

from tests.test_kernel_resources import _descriptors

KERNELS = ("k_field_pack", "k_field_query", "k_field_trace", "k_strands_resample")
WALKS = ("k_field_query", "k_field_trace")
LDS = 4 * 3 * 64 * 16   # GHR_FIELD_WAVES waves x (64 points + 2 x 64 payload) float4


def _mine(meta):
    return {k: v for k, v in meta.items() if any(n in k for n in KERNELS)}


def test_field_kernels_compile_without_scratch_or_spills_and_within_their_budgets():
    mine = _mine(_descriptors())
    assert len(mine) == len(KERNELS), list(mine)
    for name, k in sorted(mine.items()):
        print(name, k)
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        walk = any(w in name for w in WALKS)
        assert k["group_segment_fixed_size"] == (LDS if walk else 0), (name, k)
        assert k["vgpr_count"] <= 64, (name, k)      # eight waves per SIMD: a strand's whole state stays in registers


def test_field_kernel_names_hold_no_other_kernels_name():
    """tests/test_kernel_resources.py picks kernels by substring: a new name must not contain an existing one (or be contained)."""
    meta = _descriptors()
    mine = _mine(meta)
    own = [re.search(r"k_[a-z0-9_]+", m).group(0) for m in mine]
    assert sorted(own) == sorted(KERNELS), own
    for m in mine:
        for other in meta:
            if other in mine:
                continue
            name = re.search(r"k_[a-z0-9_]+", other)  # the kernel's own name inside the mangled one
            assert name is not None and name.group(0) not in m, (m, other)
            assert not any(o in other for o in own), (other, own)
