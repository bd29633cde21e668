"""Build-time guard for the two kernels of csrc/ghr_meshdist.h: no scratch, no vector spills (the search keeps a lane's state --
best d, face, point -- and a face's candidates in registers through the walk), and the search's LDS is exactly the four waves'
private tiles of 64 records of 48 B.  Cross-compiles the device code to assembly (no GPU needed); the register counts are
reported in DESIGN.md 8o, not pinned here."""
import re

from tests.test_kernel_resources import _descriptors


def _one(meta, sub):
    ks = {k: v for k, v in meta.items() if sub in k}
    assert len(ks) == 1, (sub, list(ks))
    return next(iter(ks.values()))


def test_mesh_distance_kernels_compile_without_scratch_or_vector_spills():
    meta = _descriptors()
    search, bwd = _one(meta, "k_meshdist_search"), _one(meta, "k_meshdist_bwd")
    print("k_meshdist_search:", search)
    print("k_meshdist_bwd:", bwd)
    for k in (search, bwd):
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, k
    assert search["group_segment_fixed_size"] == 4 * 64 * 48, search
    assert bwd["group_segment_fixed_size"] == 0, bwd


def test_mesh_distance_kernel_names_hold_no_other_kernels_name():
    """tests/test_kernel_resources.py picks kernels by substring: a new name must not contain an existing one (or be contained)."""
    meta = _descriptors()
    mine = [k for k in meta if "meshdist" in k]
    assert len(mine) == 2, mine
    for m in mine:
        for other in meta:
            if other in mine:
                continue
            name = re.search(r"k_[a-z0-9_]+", other)  # the kernel's own name inside the mangled one
            assert name is not None and name.group(0) not in m, (m, other)
