"""CPU-side checks of the two-codeword transmit calls (srslte_hip_dl_tx_batch_grants2 / _ctrl / _full): the symbols are declared and exported,
the host mirror's structure has the header's size, null arguments are refused without a device, and the one new kernel - cross-compiled for
gfx950 - uses no scratch, no LDS and no AGPRs (the check of tests/test_kernel_resources.py, whose file list is fixed)."""
import ctypes as C
import importlib
import os
import re
import shutil
import subprocess

import pytest

from _libs import HIP_SO, ROOT
from test_kernel_resources import HIPCC, _remarks

NAMES = ("srslte_hip_dl_tx_batch_grants2", "srslte_hip_dl_tx_batch_grants2_ctrl", "srslte_hip_dl_tx_batch_grants2_full")
needs_lib = pytest.mark.skipif(not os.path.exists(HIP_SO), reason="libsrslte_phy_hip.so not built (run __graft_entry__.build())")


@needs_lib
def test_grants2_symbols_are_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srslte_hip", "phy_hip.h")).read(), flags=re.S)
    lib = C.CDLL(HIP_SO)
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, hdr), n
        assert hasattr(lib, n), n
    assert re.search(r"typedef struct \{[^}]*srslte_hip_dl_grant2_t\s+grant;[^}]*\}\s*srslte_hip_dl_tx_grant2_t;", hdr)


@needs_lib
def test_grants2_reject_null_arguments_without_gpu():
    lib = C.CDLL(HIP_SO)
    vp, u32 = C.c_void_p, C.c_uint32
    lib.srslte_hip_dl_tx_batch_grants2.argtypes = [vp, vp, u32, u32, u32, vp, u32, vp, vp]
    assert lib.srslte_hip_dl_tx_batch_grants2(None, None, 0, 0, 1, None, 0, None, None) == -2
    for n in NAMES[1:]:
        fn = getattr(lib, n)
        fn.argtypes = [vp, vp, u32, u32, u32, vp, u32, vp, vp, vp, vp]
        assert fn(None, None, 0, 0, 1, None, 0, None, None, None, None) == -2, n


@pytest.mark.skipif(not (shutil.which("gcc") or shutil.which("cc")), reason="no C compiler")
def test_host_mirror_struct_has_the_headers_size(tmp_path):
    """sizeof(srslte_hip_dl_tx_grant2_t) and the offset of its grant, compiled from the header, against the ctypes DlTxGrant2."""
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "srslte_hip/phy_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(srslte_hip_dl_tx_grant2_t), offsetof(srslte_hip_dl_tx_grant2_t, grant), '
                   'sizeof(srslte_hip_dl_grant2_t)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call([shutil.which("gcc") or shutil.which("cc"), "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, off, inner = (int(v) for v in subprocess.check_output([str(exe)], text=True).split())
    hp = importlib.import_module("srslte-emane_amd")
    assert C.sizeof(hp.DlTxGrant2) == size and hp.DlTxGrant2.grant.offset == off and C.sizeof(hp.DlGrant2) == inner


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_mod2_kernel_resources():
    """One thread per symbol, select by value: no scratch, no spills, no LDS (the transmit-diversity kernels beside it keep their d[4] there),
    no AGPRs, and few enough registers for eight waves a SIMD."""
    kernels = {k: r for k, r in _remarks("pdsch.hip").items() if "pdsch_tx_mod2_grants_kernel" in k}
    assert len(kernels) == 1, sorted(kernels)
    for k, r in kernels.items():
        assert r.get("ScratchSize [bytes/lane]", 0) == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
        assert r["LDS Size [bytes/block]"] == 0 and r.get("AGPRs", 0) == 0, (k, r)
        assert r["VGPRs"] <= 64 and r["Occupancy [waves/SIMD]"] == 8, (k, r)
