"""Compile-time resources of the sc16 instances of the two OFDM kernels (fft.hip) beside their cf32 twins: none spills or uses scratch, none
reaches fewer waves per SIMD than its twin (so none needs more registers than the twin's occupancy allows), and there is one per fixed plan:
eight receive, eight receive with the half-carrier shift, eight transmit. The kernels' LDS is dynamic and sized by the plan alone."""
import os
import re

import pytest

from test_kernel_resources import HIPCC, _remarks


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_sc16_instances_fit_their_cf32_twins():
    res = _remarks("fft.hip")
    inst = {}
    for k in res:  # mangled: ofdm_rx_kernel<R0, R1, R2, FMT, SC16_SHIFT> / ofdm_tx_kernel<R0, R1, R2, FMT>
        m = re.search(r"(ofdm_[rt]x)_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E(?:Lb([01])E)?E", k)
        if m:
            inst[(m.group(1), tuple(int(v) for v in m.group(2, 3, 4)), int(m.group(5)), m.group(6) == "1")] = res[k]
    sc16 = {k: r for k, r in inst.items() if k[2] == 1}
    assert len(sc16) == 24 and all(k[1] != (0, 0, 0) for k in sc16), sorted(sc16)
    for (kern, plan, _, shift), r in sorted(sc16.items()):
        twin = inst[(kern, plan, 0, False)]
        print(kern, plan, "shift" if shift else "", "sc16", r, "cf32", twin)
        assert r.get("ScratchSize [bytes/lane]", 0) == 0 and r.get("VGPRs Spill", 0) == 0, (kern, plan, shift, r)
        assert r["Occupancy [waves/SIMD]"] >= twin["Occupancy [waves/SIMD]"], (kern, plan, shift, r, twin)
        assert r.get("AGPRs", 0) == 0 and r.get("LDS Size [bytes/block]", 0) == twin.get("LDS Size [bytes/block]", 0)
