"""The channel emulator's kernels under the rule of tests/test_kernel_resources.py: no scratch memory, no spills (the per-tap amplitudes live in
a device table and the launch geometry is only read, because a by-value argument struct that is indexed dynamically or written moves to scratch)."""
import os

import pytest

from test_kernel_resources import HIPCC, _remarks


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_channel_kernels_use_no_scratch():
    kernels = _remarks("channel.hip")
    names = " ".join(kernels)
    for want in ["ch_fading_kernelILi%dEE" % n for n in (64, 128, 256, 512, 1024)] + ["ch_output_kernel", "ch_carry_kernel"]:
        assert want in names, (want, sorted(kernels))
    for k, r in kernels.items():
        assert r.get("ScratchSize [bytes/lane]", 0) == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
        assert r["LDS Size [bytes/block]"] <= 3 * 8 * 1024 + 128, (k, r)  # three N-point buffers and the tap coefficients at N = 1024
