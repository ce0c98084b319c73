"""Compile-time resource check of csrc/csi.hip (the check of tests/test_kernel_resources.py, whose file list is fixed): the one kernel uses
no scratch, the LDS of its four wave partials only, and a register count that leaves the SIMDs to the decoder's wavefronts."""
import os

import pytest

from test_kernel_resources import HIPCC, _remarks


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_csi_kernel_resources():
    kernels = _remarks("csi.hip")
    assert len(kernels) == 1 and "csi_kernel" in list(kernels)[0], sorted(kernels)
    for k, r in kernels.items():
        assert r.get("ScratchSize [bytes/lane]", 0) == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
        # 4 waves x 8 floats; an index into the record once moved it to LDS (64 bytes a lane, 16 KB a block)
        assert r["LDS Size [bytes/block]"] <= 128, (k, r)
        assert r["VGPRs"] <= 96 and r.get("AGPRs", 0) == 0, (k, r)
