"""Compile-time resource check of csrc/srs.hip (the check of tests/test_kernel_resources.py, whose file list is fixed): both SRS kernels exist
and neither uses scratch memory or spills."""
import os

import pytest

from test_kernel_resources import HIPCC, _remarks


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_srs_kernels_use_no_scratch():
    kernels = _remarks("srs.hip")
    names = sorted(kernels)
    assert any("srs_rx_kernel" in k for k in names) and any("srs_tx_kernel" in k for k in names), names
    for k, r in kernels.items():
        assert r.get("ScratchSize [bytes/lane]", 0) == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (k, r)
