"""Build-time guard for the capture kernel (csrc/ghr_capture.h: k_sv_capture): a thread keeps the sums, the best scores and the bins
of its four pixels in registers and a row of subsamples as one vector -- no instantiation may get a private segment (an array the
compiler could not promote, or a spill), and the only LDS is the staged table.  Reads the kernel descriptors of the device code
cross-compiled to assembly (no GPU needed), as tests/test_strand_shadow_resources.py does."""
from tests.test_kernel_resources import _descriptors


def test_capture_kernel_compiles_without_scratch_or_spills():
    meta = _descriptors()
    ks = {k: v for k, v in meta.items() if "k_sv_capture" in k}
    assert len(ks) == 5, sorted(ks)                            # s = 4 and 2 with and without row loads, s = 1
    for name, k in ks.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["vgpr_count"] <= 64, (name, k)                # eight waves per SIMD: the loads of a quad's rows are its latency
        assert k["group_segment_fixed_size"] == 2 * 180 * 4, (name, k)   # the table [180][2] and nothing else
