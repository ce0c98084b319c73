"""Compile-time resource check of csrc/pucch.hip (the check of tests/test_kernel_resources.py, whose file list is fixed): no kernel may use
scratch memory or spill."""
import os

import pytest

from test_kernel_resources import HIPCC, _remarks


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_pucch_kernels_use_no_scratch():
    kernels = _remarks("pucch.hip")
    names = sorted(kernels)
    assert any("ul_pucch_rx_kernel" in k for k in names) and any("ul_pucch_tx_kernel" in k for k in names), names
    for k, r in kernels.items():
        assert r.get("ScratchSize [bytes/lane]", 0) == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
