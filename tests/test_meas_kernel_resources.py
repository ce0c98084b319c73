"""The measurement kernels under the rule of tests/test_kernel_resources.py: each exists once, uses no scratch memory and spills nothing, and
its static LDS stays under the bound phy_hip.h states. The row passes in fft.hip are templates over the OFDM plans: every instance of the
fused inverse row pass is held to the same rule (their LDS is dynamic, (N + N / 16 + 2) cf32 = 17 424 bytes at N = 2048)."""
import os

import pytest

from test_kernel_resources import HIPCC, _remarks

LDS_BOUND = {"meas_fill_kernel": 0, "meas_scale_kernel": 0, "meas_col_fwd_kernel": 0, "meas_col_inv_kernel": 2 * 1024, "meas_decide_kernel": 0,
             "meas_sf_kernel": 1024, "meas_finish_kernel": 0}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_meas_kernels_use_no_scratch():
    kernels = _remarks("meas.hip")
    for want, bound in LDS_BOUND.items():
        hit = [k for k in kernels if want in k]
        assert len(hit) == 1, (want, sorted(kernels))
        r = kernels[hit[0]]
        assert r.get("ScratchSize [bytes/lane]", 0) == 0 and r.get("VGPRs Spill", 0) == 0, (want, r)
        assert r["LDS Size [bytes/block]"] <= bound, (want, r)
    assert len(kernels) == len(LDS_BOUND), sorted(kernels)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_fused_inverse_row_pass_uses_no_scratch():
    rows = {k: r for k, r in _remarks("fft.hip").items() if "dft_rows30_mulconj_kernel" in k}
    assert len(rows) == 9, sorted(rows)  # the eight fixed plans of the OFDM sizes and the generic one
    assert (2048 + 2048 // 16 + 2) * 8 == 17424
    for k, r in rows.items():
        assert r.get("ScratchSize [bytes/lane]", 0) == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
        assert r["LDS Size [bytes/block]"] == 0, (k, r)  # static; the transform's buffer is dynamic
