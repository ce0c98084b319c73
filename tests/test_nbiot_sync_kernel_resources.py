"""Compile-time resources of the NB-IoT synchronisation kernels (csrc/nbiot_sync.hip): none uses scratch memory or spills, and the static LDS of
each stays within the bound phy_hip.h states for the module (12 288 bytes; the slide kernels 4 256, the others 4 096)."""
import os

import pytest

from test_kernel_resources import HIPCC, _remarks

LDS_BOUND = 12288
KERNELS = ("nbiot_npss_slide_kernel", "nbiot_npss_comb_kernel", "nbiot_npss_decide_kernel", "nbiot_nsss_slide_kernel", "nbiot_nsss_prod_kernel",
           "nbiot_nsss_decide_kernel", "nbiot_track_reset_kernel", "nbiot_track_set_cfo_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_nbiot_kernels_use_no_scratch_and_little_lds():
    res = _remarks("nbiot_sync.hip")
    for name in KERNELS:
        hit = [k for k in res if name in k]
        assert len(hit) == 1, (name, sorted(res))
    assert len(res) == len(KERNELS), sorted(res)
    for k, r in res.items():
        assert r.get("ScratchSize [bytes/lane]", 0) == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
        assert r.get("LDS Size [bytes/block]", 0) <= LDS_BOUND, (k, r)
        if "slide_kernel" in k:
            assert r["LDS Size [bytes/block]"] <= 4256, (k, r)
        elif "prod_kernel" not in k:
            assert r.get("LDS Size [bytes/block]", 0) <= 4096, (k, r)
    prod = [r for k, r in res.items() if "nbiot_nsss_prod_kernel" in k][0]
    print("nbiot_nsss_prod_kernel:", prod)
    assert prod["LDS Size [bytes/block]"] == 2 * 12 * 64 * 8
