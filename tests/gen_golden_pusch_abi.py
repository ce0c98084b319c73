"""Writes tests/golden/ref_abi_pusch.json: sizeof / offsetof of the reference structs srslte_pusch_decode takes (tests/pusch_decode_abi.py), taken
from the reference's headers with gcc. Numbers only. Run where the reference tree exists:

    python tests/gen_golden_pusch_abi.py
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _libs import REF_INC, ROOT, struct_layout  # noqa: E402
from pusch_decode_abi import FIELDS, INCLUDES  # noqa: E402

if __name__ == "__main__":
    if not os.path.isdir(REF_INC):
        sys.exit("the reference headers are not here")
    out = os.path.join(ROOT, "tests", "golden", "ref_abi_pusch.json")
    with open(out, "w") as f:
        json.dump({"layouts": struct_layout(FIELDS, INCLUDES, [REF_INC])}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(out)
