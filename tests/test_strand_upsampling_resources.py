"""Build-time guard for the kernels of csrc/ghr_upsample.h: no scratch, no vector spills, the LDS that was planned (one tile of 256
guide roots in k_ups_near, none in k_ups_blend), registers within eight waves per SIMD, workgroups of 256 in waves of 64, and names
that hold no other kernel's name.  Cross-compiles the device code to assembly (no GPU needed); the counts are in DESIGN.md 8v."""
import re

from tests.test_kernel_resources import _descriptors

KERNELS = {
    # name: (LDS bytes, threads per workgroup, most VGPRs)
    "k_ups_near": (3 * 256 * 4, 256, 64),   # 512 / 64 = eight waves per SIMD
    "k_ups_blend": (0, 256, 64),
}


def _mine(meta, kernel):
    return {k: v for k, v in meta.items() if kernel in k}


def test_upsampling_kernels_compile_without_scratch_or_vector_spills_and_within_their_budget():
    meta = _descriptors()
    for kernel, (lds, threads, vgprs) in KERNELS.items():
        mine = _mine(meta, kernel)
        assert len(mine) == 1, (kernel, list(mine))
        (name, k), = mine.items()
        print(name, k)
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (name, k)
        assert k["group_segment_fixed_size"] == lds, (name, k)
        assert k["vgpr_count"] <= vgprs, (name, k)
        assert k["max_flat_workgroup_size"] == threads and k["wavefront_size"] == 64, (name, k)


def test_upsampling_kernel_names_hold_no_other_kernels_name():
    """the resource tests pick kernels by substring of the mangled name (argument types included): a new name must contain no other
    kernel's name and be contained in none"""
    meta = _descriptors()
    for kernel in KERNELS:
        (mine,) = _mine(meta, kernel)
        assert re.search(r"k_[a-z0-9_]+", mine).group(0) == kernel
        for other in meta:
            if other == mine:
                continue
            name = re.search(r"k_[a-z0-9_]+", other)  # the kernel's own name inside the mangled one
            assert name is not None and name.group(0) not in mine, (mine, other)
            assert kernel not in other, other
