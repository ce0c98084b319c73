"""The kernels of sync.hip under the rule of tests/test_meas_kernel_resources.py, with the tracked call's in: every body exists once per
instance - the stateless sync_*_kernel and the track_*_kernel of srslte_hip_sync_track_batch -, no kernel uses scratch memory or spills a
vector register, and the static LDS stays under the bound phy_hip.h states (the correlation kernels add (2 N + 255) cf32 of
dynamic LDS, 34 808 bytes at N = 2048: 40 KB with everything). The two SSS trials of track_decide_kernel run one after the other in the LDS
of one: it holds what sync_decide_kernel holds, one symbol of 2048 samples (16 KB) and 6 KB of reduction and SSS buffers."""
import os

import pytest

from test_kernel_resources import HIPCC, _remarks

LDS_BOUND = {"sync_cp_kernel": 2 * 1024, "sync_corr_kernel": 2 * 1024, "sync_decide_kernel": 24 * 1024, "cfo_correct_kernel": 0,
             "track_cp_kernel": 2 * 1024, "track_corr_kernel": 2 * 1024, "track_decide_kernel": 24 * 1024, "track_reset_kernel": 0,
             "track_copy_cfo_kernel": 0}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_sync_and_track_kernels_use_no_scratch():
    kernels = _remarks("sync.hip")
    for corr in ("sync_corr_kernel", "track_corr_kernel"):
        assert (2 * 2048 + 255) * 8 + LDS_BOUND[corr] <= 40 * 1024
    for want, bound in LDS_BOUND.items():
        hit = [k for k in kernels if want in k]
        assert len(hit) == 1, (want, sorted(kernels))
        r = kernels[hit[0]]
        assert r.get("ScratchSize [bytes/lane]", 0) == 0 and r.get("VGPRs Spill", 0) == 0, (want, r)
        assert r["LDS Size [bytes/block]"] <= bound, (want, r)
    assert len(kernels) == len(LDS_BOUND), sorted(kernels)
    assert kernels[[k for k in kernels if "track_decide_kernel" in k][0]]["LDS Size [bytes/block]"] == \
        kernels[[k for k in kernels if "sync_decide_kernel" in k][0]]["LDS Size [bytes/block]"]
