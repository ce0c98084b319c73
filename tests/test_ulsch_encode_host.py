"""The uplink transmit hook of the link-time drop-in without a GPU: the library exports the device call and its debugging accessor (phy_hip.h),
the reference's srslte_ulsch_encode on top of it and the counter of served calls (srslte_compat.h), and what that function reads and writes of
the reference's structs - the (position, type) list in srslte_sch_t, the transmit soft buffer, the UCI values - lies in the compat header as in
the reference's headers: against the stored numbers of tests/golden/ref_abi_ulsch_enc.json (tests/gen_golden_ulsch_enc_abi.py) and, where they
are present, against the headers themselves. The structs of the PUSCH configuration are held by tests/test_ulsch_host.py."""
import ctypes
import json
import os

from _libs import HIP_SO, REF_INC, ROOT, struct_layout
from ulsch_enc_abi import FIELDS, INCLUDES


def test_the_uplink_transmit_entry_points_are_exported():
    lib = ctypes.CDLL(HIP_SO)
    missing = [n for n in ("srslte_hip_ulsch_encode", "srslte_hip_ulsch_enc_debug", "srslte_ulsch_encode", "srslte_hip_compat_stats_ul_tx") if not hasattr(lib, n)]
    assert not missing, missing


def test_position_list_soft_buffer_and_uci_value_layouts_match_the_reference():
    ours = struct_layout(FIELDS, ["srslte_hip/srslte_compat.h"], [os.path.join(ROOT, "include")])
    with open(os.path.join(ROOT, "tests", "golden", "ref_abi_ulsch_enc.json")) as f:
        stored = json.load(f)["layouts"]
    assert set(stored) == set(ours) and len(ours) == len(FIELDS) + sum(len(v) for v in FIELDS.values())
    assert ours == stored
    # the list holds 57600 pairs of two 32-bit words, directly in front of the turbo encoder's two fields
    assert ours["srslte_uci_bit_t"] == 8 and ours["srslte_sch_t.encoder"] - ours["srslte_sch_t.ack_ri_bits"] == 57600 * 8
    if os.path.isdir(REF_INC):
        assert struct_layout(FIELDS, INCLUDES, [REF_INC]) == ours


def test_null_arguments_are_refused_without_a_device():
    """what needs no object: NULL arguments of the three entries, which the counter of served calls does not see"""
    lib = ctypes.CDLL(HIP_SO)
    buf = (ctypes.c_uint8 * 4096)()
    before, after = (ctypes.c_ulonglong * 2)(), (ctypes.c_ulonglong * 2)()
    lib.srslte_hip_compat_stats_ul_tx(before)
    assert lib.srslte_hip_ulsch_encode(None, buf, buf, None, None, buf, buf) == -2
    assert lib.srslte_hip_ulsch_enc_debug(None, buf, 0) == -2
    assert lib.srslte_ulsch_encode(None, buf, buf, buf, None, buf) == -2
    lib.srslte_hip_compat_stats_ul_tx(after)
    assert list(after) == list(before)
