"""The uplink receive hook of the link-time drop-in, linked: the reference's own srslte_pusch_encode / srslte_pusch_decode (lib/src/phy/phch/pusch.c
in oracle/_ref/hip/libsrslte_upper.a; pusch.c:503 calls srslte_ulsch_decode) over this library on an identity channel, once with the archive's own
sch.o serving that call (upstream's path: UCI and de-interleaver on the host, one srslte_tdec_iteration round trip per code block and pass) and
once with the call wrapped to the library's srslte_ulsch_decode (-Wl,--wrap, INTEGRATION.md 1: one device call per transport block).
tests/ulsch_dropin_driver.c, compiled here with gcc as tests/test_gpu_sch_encode_dropin.py compiles its driver: 6 PRB QPSK with ACK + CQI,
25 PRB 16QAM tbs 15264 with rv 0 (which cannot decode alone) then 2, 100 PRB 64QAM tbs 75376. The two builds must decode the same bytes and UCI values, the library's counter of
served srslte_ulsch_decode calls must say which path each took, and the wrapped build must wait for a stream less often."""
import os
import re
import subprocess
import tempfile

import pytest

from _libs import ROOT

CSRC = os.path.join(ROOT, "srslte-emane_amd", "csrc")
HIP_REF = os.path.join(ROOT, "oracle", "_ref", "hip")
WRAP = ["-DWRAPPED", "-Wl,--wrap=srslte_ulsch_decode"]

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(os.path.join(HIP_REF, "libsrslte_upper.a")), reason="oracle/_ref/hip/libsrslte_upper.a not built")]


def build(d, name, extra):
    exe = os.path.join(d, name)
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-I" + os.path.join(ROOT, "include")] + extra + [os.path.join(ROOT, "tests", "ulsch_dropin_driver.c"), "-o", exe,
                           os.path.join(HIP_REF, "libsrslte_upper.a"), "-L" + CSRC, "-lsrslte_phy_hip", "-Wl,-rpath," + CSRC, "-Wl,-rpath,/opt/rocm/lib",
                           "-lstdc++", "-lm", "-lpthread", "-ldl"])
    return exe


def run(exe, out):
    r = subprocess.run([exe, "run", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    n = int(re.search(r"decodes=(\d+)", r.stdout).group(1))
    st = [int(x) for x in re.search(r"stats: (\d+) (\d+) (\d+) (\d+)", r.stdout).groups()]
    ul = [int(x) for x in re.search(r"stats_ul: (\d+) (\d+)", r.stdout).groups()]
    print(r.stdout)
    with open(out, "rb") as f:
        return n, st, ul, f.read()


def test_wrapped_and_plain_builds_decode_the_same():
    with tempfile.TemporaryDirectory() as d:
        n_p, st_p, ul_p, out_p = run(build(d, "plain", []), os.path.join(d, "plain.out"))
        n_w, st_w, ul_w, out_w = run(build(d, "wrapped", WRAP), os.path.join(d, "wrapped.out"))
    assert n_p == n_w == 4
    assert len(out_p) == 4 * 8 + (600 + 2 * 15264 + 75376) // 8 and out_p == out_w  # the driver itself holds the bytes to what was sent
    assert ul_p == [0, 0], "the plain build reached the library's srslte_ulsch_decode: %s" % ul_p
    assert ul_w[0] == n_w, "the wrapped build did not: %s" % ul_w
    assert st_w[2] == 0 and st_p[2] > 0, "single-block decoder calls: none through the hook, upstream's loop without it: %s / %s" % (st_w, st_p)
    assert st_w[0] + ul_w[1] < st_p[0] + ul_p[1], "stream waits, the hook's own included: %s %s / %s %s" % (st_w, ul_w, st_p, ul_p)
