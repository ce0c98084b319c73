"""The transmit hook of the link-time drop-in, linked: the reference's own srslte_pdsch_encode (lib/src/phy/phch/pdsch.c in
oracle/_ref/hip/libsrslte_upper.a; pdsch.c:1032 calls srslte_dlsch_encode2) over this library, once with the archive's own sch.o serving that call
(upstream's loop: one srslte_tcod_encode_lut round trip per code block) and once with the call wrapped to the library's srslte_dlsch_encode2
(-Wl,--wrap, INTEGRATION.md 1: one device call per transport block). tests/sch_encode_dropin_driver.c, compiled here with gcc as
tests/test_gpu_meas.py compiles its driver. The two builds must produce the same resource grids - 25 PRB / tbs 4008 16QAM with rv 0 and 2, 100 PRB /
tbs 75376 64QAM - and the library's counter of served srslte_dlsch_encode2 calls must say which path each took."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from _libs import ROOT

CSRC = os.path.join(ROOT, "srslte-emane_amd", "csrc")
HIP_REF = os.path.join(ROOT, "oracle", "_ref", "hip")
WRAP = ["-DWRAPPED", "-Wl,--wrap=srslte_dlsch_encode2", "-Wl,--wrap=srslte_dlsch_encode"]

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(os.path.join(HIP_REF, "libsrslte_upper.a")), reason="oracle/_ref/hip/libsrslte_upper.a not built")]


def build(d, name, extra):
    exe = os.path.join(d, name)
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-I" + os.path.join(ROOT, "include")] + extra + [os.path.join(ROOT, "tests", "sch_encode_dropin_driver.c"), "-o", exe,
                           os.path.join(HIP_REF, "libsrslte_upper.a"), "-L" + CSRC, "-lsrslte_phy_hip", "-Wl,-rpath," + CSRC, "-Wl,-rpath,/opt/rocm/lib",
                           "-lstdc++", "-lm", "-lpthread", "-ldl"])
    return exe


def run(exe, out):
    r = subprocess.run([exe, "grid", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    tb = int(re.search(r"transport_blocks=(\d+)", r.stdout).group(1))
    st = [int(x) for x in re.search(r"stats: (\d+) (\d+) (\d+) (\d+)", r.stdout).groups()]
    print(r.stdout)
    return tb, st, np.fromfile(out, np.complex64)


def test_wrapped_and_plain_builds_transmit_the_same_grids():
    with tempfile.TemporaryDirectory() as d:
        tb_p, st_p, grid_p = run(build(d, "plain", []), os.path.join(d, "plain.grid"))
        tb_w, st_w, grid_w = run(build(d, "wrapped", WRAP), os.path.join(d, "wrapped.grid"))
    assert tb_p == tb_w == 6
    assert grid_p.size == 14 * 12 * (4 * 25 + 2 * 100) and np.any(grid_p != 0)
    assert grid_p.tobytes() == grid_w.tobytes()
    assert st_p[3] == 0, "the plain build reached the library's srslte_dlsch_encode2: %s" % st_p
    assert st_w[3] == tb_w, "the wrapped build did not: %s" % st_w
    assert st_w[0] < st_p[0], "one stream wait per transport block against one per code block: %s / %s" % (st_w, st_p)
