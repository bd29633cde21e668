"""Build-time guard for the five kernels of csrc/ghr_texstrands.h: no scratch, no vector spills, and LDS only in k_ts_texgrad --
exactly its 64 x 193 float tile (64 texels x 192 channels a pass, rows padded by one float against bank conflicts).  Cross-compiles
the device code to assembly (no GPU needed); the register counts are reported in DESIGN.md 8p, not pinned here."""
import re

from tests.test_kernel_resources import _descriptors

KERNELS = ("k_ts_fetch", "k_ts_positions", "k_ts_texgrad", "k_ts_world_bwd", "k_ts_world")


def _mine(meta):
    return {k: v for k, v in meta.items() if "k_ts_" in k}


def test_texstrands_kernels_compile_without_scratch_or_vector_spills():
    mine = _mine(_descriptors())
    assert len(mine) == len(KERNELS), list(mine)
    for name, k in sorted(mine.items()):
        print(name, k)
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (name, k)
        want_lds = 64 * 193 * 4 if "k_ts_texgrad" in name else 0
        assert k["group_segment_fixed_size"] == want_lds, (name, k)


def test_texstrands_kernel_names_hold_no_other_kernels_name():
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
