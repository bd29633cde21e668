"""Build-time guard for the HAAR blend's kernels: both instantiations (texels, drawn roots) of the five kernels of csrc/ghr_haar.h
and the three list kernels of csrc/ghr_guides.h: no scratch, no vector spills, no LDS.  Cross-compiles the device code to assembly
(no GPU needed); the register counts are reported in DESIGN.md 8q, not pinned here."""
import re

from tests.test_kernel_resources import _descriptors

SHARED = ("k_haar_knn", "k_haar_blend", "k_haar_dalpha", "k_haar_gather", "k_haar_bwd_v")
POLICIES = ("HaarTexels", "HaarRoots")
KERNELS = SHARED + ("k_gd_start", "k_gd_fill", "k_gd_lists")


def _mine(meta):
    return {k: v for k, v in meta.items() if "k_gd_" in k or "k_haar_" in k}


def test_guides_kernels_compile_without_scratch_or_vector_spills():
    mine = _mine(_descriptors())
    assert len(mine) == len(SHARED) * len(POLICIES) + 3, list(mine)
    for name in SHARED:
        for policy in POLICIES:
            assert sum(1 for m in mine if name in m and policy in m) == 1, (name, policy, list(mine))
    for name, k in sorted(mine.items()):
        print(name, k)
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (name, k)
        assert k["group_segment_fixed_size"] == 0, (name, k)


def test_guides_kernel_names_hold_no_other_kernels_name():
    """tests/test_kernel_resources.py picks kernels by substring: a new name must not contain an existing one (or be contained)."""
    meta = _descriptors()
    mine = _mine(meta)
    own = [re.search(r"k_[a-z0-9_]+", m).group(0) for m in mine]
    assert sorted(own) == sorted(SHARED * len(POLICIES) + KERNELS[len(SHARED):]), own
    for m in mine:
        for other in meta:
            if other in mine:
                continue
            name = re.search(r"k_[a-z0-9_]+", other)  # the kernel's own name inside the mangled one
            assert name is not None and name.group(0) not in m, (m, other)
            assert not any(o in other for o in own), (other, own)
