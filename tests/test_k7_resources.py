"""Build-time guard for the occupancy k_render_fwd (csrc/ghr_render_fwd.h) is tuned for: six workgroups of four waves per CU.

The kernel is bound by instruction issue and hides its LDS latency behind the other waves of its SIMD; it sits right at two
occupancy steps -- 80 VGPRs (512 / 6, granule 8) and a sixth of the CU's 160 KiB of LDS (the record planes take 24.6 KB, the
per-cell hit lists 2 KB) -- and one register or one more LDS array over either costs a sixth of its waves without any test of
results noticing.  Both instantiations (the list walk and the mask walk behind GHR_K7_WALK=mask) must meet it, without
scratch: a spill is a memory access inside the step loop.  Cross-compiles the device code to assembly (no GPU needed) and
reads the kernel descriptors, as tests/test_kernel_resources.py does.

The LDS step is finer than 160 KiB / 6 = 27,306 B says: the CU hands its LDS out in 128 granules of 1280 B, a workgroup gets
whole granules, six workgroups fit with 21 granules each = 26,880 B.  Measured (profiles/k7_hit_lists_ab.txt): the list walk
at 26,960 B ran with 16 % fewer cycles per wave than the mask walk and in the same kernel time -- five workgroups per CU;
at 26,720 B it is 7-10 % faster."""
from tests.test_kernel_resources import _descriptors

LDS_GRANULE = 1280          # bytes; 128 of them per CU
LDS_GRANULES_FOR_SIX = 21   # 128 // 6


def test_every_render_fwd_instantiation_holds_six_workgroups_per_cu():
    meta = _descriptors()
    k7 = {k: v for k, v in meta.items() if "k_render_fwd" in k}
    assert len(k7) == 2, list(k7)   # <true>: hit lists, <false>: mask walk
    for name, k in k7.items():
        assert k["private_segment_fixed_size"] == 0, (name, k)
        assert k["vgpr_spill_count"] == 0, (name, k)
        assert k["vgpr_count"] <= 80, (name, k)
        assert k["group_segment_fixed_size"] <= 27306, (name, k)
        assert -(-k["group_segment_fixed_size"] // LDS_GRANULE) <= LDS_GRANULES_FOR_SIX, (name, k)
