"""Build-time guard for the eight kernels of csrc/ghr_guides.h: no scratch, no vector spills, no LDS.  Cross-compiles the device
code to assembly (no GPU needed); the register counts are reported in DESIGN.md 8q, not pinned here."""
import re

from tests.test_kernel_resources import _descriptors

KERNELS = ("k_gd_knn", "k_gd_start", "k_gd_fill", "k_gd_lists", "k_gd_blend", "k_gd_dalpha", "k_gd_gather", "k_gd_bwd_v")


def _mine(meta):
    return {k: v for k, v in meta.items() if "k_gd_" in k}


def test_guides_kernels_compile_without_scratch_or_vector_spills():
    mine = _mine(_descriptors())
    assert len(mine) == len(KERNELS), list(mine)
    for name, k in sorted(mine.items()):
        print(name, k)
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (name, k)
        assert k["group_segment_fixed_size"] == 0, (name, k)


def test_guides_kernel_names_hold_no_other_kernels_name():
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
