"""The uplink receive hook of the link-time drop-in without a GPU: the library exports the device call (phy_hip.h), the reference's
srslte_ulsch_decode on top of it and the counter of served calls (srslte_compat.h), and every struct that function reads or writes lies in the
compat header as in the reference's headers: against the stored numbers of tests/golden/ref_abi_ulsch.json (tests/gen_golden_ulsch_abi.py) and,
where they are present, against the headers themselves."""
import ctypes
import json
import os

from _libs import HIP_SO, REF_INC, ROOT, struct_layout
from ulsch_abi import FIELDS, INCLUDES


def test_the_uplink_entry_points_are_exported():
    lib = ctypes.CDLL(HIP_SO)
    missing = [n for n in ("srslte_hip_ulsch_decode", "srslte_hip_ulsch_debug_g", "srslte_ulsch_decode", "srslte_hip_compat_stats_ul") if not hasattr(lib, n)]
    assert not missing, missing


def test_pusch_and_uci_struct_layouts_match_the_reference():
    ours = struct_layout(FIELDS, ["srslte_hip/srslte_compat.h"], [os.path.join(ROOT, "include")])
    with open(os.path.join(ROOT, "tests", "golden", "ref_abi_ulsch.json")) as f:
        stored = json.load(f)["layouts"]
    assert set(stored) == set(ours) and len(ours) == len(FIELDS) + sum(len(v) for v in FIELDS.values())
    assert ours == stored
    if os.path.isdir(REF_INC):
        assert struct_layout(FIELDS, INCLUDES, [REF_INC]) == ours
