"""The synchronisation kernels under the rule of tests/test_kernel_resources.py: they exist, use no scratch memory and spill nothing, and their
static LDS stays under the documented bound. sync_corr_kernel's replica and input tile are dynamic LDS, (2 N + 255) cf32 = 34 808 bytes at
N = 2048, on top of the 2 KB counted here: 40 KB with everything, the bound phy_hip.h states. sync_decide_kernel holds one symbol of 2048
samples (16 KB) and 6 KB of reduction and SSS buffers."""
import os

import pytest

from test_kernel_resources import HIPCC, _remarks

LDS_BOUND = {"sync_cp_kernel": 2 * 1024, "sync_corr_kernel": 2 * 1024, "sync_decide_kernel": 24 * 1024, "cfo_correct_kernel": 0}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_sync_kernels_use_no_scratch():
    kernels = _remarks("sync.hip")
    assert (2 * 2048 + 255) * 8 + LDS_BOUND["sync_corr_kernel"] <= 40 * 1024
    for want, bound in LDS_BOUND.items():
        hit = [k for k in kernels if want in k]
        assert len(hit) == 1, (want, sorted(kernels))
        r = kernels[hit[0]]
        assert r.get("ScratchSize [bytes/lane]", 0) == 0 and r.get("VGPRs Spill", 0) == 0, (want, r)
        assert r["LDS Size [bytes/block]"] <= bound, (want, r)
