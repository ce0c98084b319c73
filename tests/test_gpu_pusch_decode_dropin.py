"""The PUSCH receiver's hook of the link-time drop-in, linked: the reference's own srslte_pusch_encode / srslte_pusch_decode (lib/src/phy/phch/pusch.c
in oracle/_ref/hip/libsrslte_upper.a) over this library on an identity channel, in three builds of tests/pusch_decode_dropin_driver.c, compiled
here with gcc as tests/test_gpu_ulsch_dropin.py compiles its driver: plain (the archive's pusch.o and sch.o), with srslte_ulsch_decode handed to
the library (the path before this hook: three visits of the library per PUSCH) and with -Wl,--wrap=srslte_pusch_decode (one
device call per PUSCH). 6 PRB QPSK with ACK + CQI, 25 PRB 16QAM tbs 15264 with rv 0 (which cannot decode alone) then 2, 100 PRB 64QAM tbs 75376,
and the 6-PRB case on an 8-bit object, which the forwarders hand back to upstream. All three must write the same bytes, UCI values and CRC flags;
the counters say which path each took."""
import os
import re
import subprocess
import tempfile

import pytest

from _libs import ROOT

CSRC = os.path.join(ROOT, "srslte-emane_amd", "csrc")
HIP_REF = os.path.join(ROOT, "oracle", "_ref", "hip")
COUNT = ["-Wl,--wrap=srslte_dft_precoding", "-Wl,--wrap=srslte_demod_soft_demodulate_s", "-Wl,--wrap=srslte_ulsch_decode"]
BUILDS = {"plain": [], "ulsch": ["-DHOOK_ULSCH"], "pusch": ["-DHOOK_PUSCH", "-Wl,--wrap=srslte_pusch_decode"]}

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(os.path.join(HIP_REF, "libsrslte_upper.a")), reason="oracle/_ref/hip/libsrslte_upper.a not built")]


def build(d, name):
    exe = os.path.join(d, name)
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-I" + os.path.join(ROOT, "include")] + COUNT + BUILDS[name] +
                          [os.path.join(ROOT, "tests", "pusch_decode_dropin_driver.c"), "-o", exe, os.path.join(HIP_REF, "libsrslte_upper.a"), "-L" + CSRC,
                           "-lsrslte_phy_hip", "-Wl,-rpath," + CSRC, "-Wl,-rpath,/opt/rocm/lib", "-lstdc++", "-lm", "-lpthread", "-ldl"])
    return exe


def run(exe, out):
    r = subprocess.run([exe, "run", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    print(r.stdout)
    dec = [dict(zip(("crc", "waits", "dft", "demod", "ulsch", "served"), map(int, m)))
           for m in re.findall(r"dec \d+ crc (\d) waits (\d+) dft (\d+) demod (\d+) ulsch (\d+) served (\d+)", r.stdout)]
    pu = [int(x) for x in re.search(r"stats_pusch: (\d+) (\d+)", r.stdout).groups()]
    ul = [int(x) for x in re.search(r"stats_ul: (\d+) (\d+)", r.stdout).groups()]
    with open(out, "rb") as f:
        return dec, ul, pu, f.read()


def test_the_three_builds_decode_the_same_and_the_counters_name_their_paths():
    with tempfile.TemporaryDirectory() as d:
        res = {name: run(build(d, name), os.path.join(d, name + ".out")) for name in BUILDS}
    (dec_p, ul_p, pu_p, out_p), (dec_u, ul_u, pu_u, out_u), (dec_h, ul_h, pu_h, out_h) = res["plain"], res["ulsch"], res["pusch"]
    # decodes 0 .. 4: 6 PRB, 25 PRB rv 0, rv 2, 100 PRB, 6 PRB on the 8-bit object
    assert len(dec_p) == len(dec_u) == len(dec_h) == 5
    assert len(out_p) == 5 * 8 + (600 + 2 * 15264 + 75376 + 600) // 8  # the driver itself holds the bytes to what was sent
    assert out_p == out_u == out_h, "bytes, UCI values or CRC flags differ between the builds"
    assert [x["crc"] for x in dec_h[:4]] == [1, 0, 1, 1]
    # which path each took
    assert pu_p == [0, 0] and ul_p == [0, 0] and all(x["ulsch"] == 1 and x["dft"] == 1 and x["demod"] == 1 for x in dec_p[:4]), (dec_p, ul_p, pu_p)
    assert pu_u == [0, 0] and ul_u[0] == 4 and all(x["ulsch"] == 1 and x["dft"] == 1 and x["demod"] == 1 for x in dec_u[:4]), (dec_u, ul_u, pu_u)
    assert pu_h[0] == 4 and ul_h == [0, 0], (pu_h, ul_h)
    for x in dec_h[:4]:  # served, and no separate entry into the transform, the demapper or the UL-SCH call
        assert (x["served"], x["dft"], x["demod"], x["ulsch"]) == (1, 0, 0, 0), dec_h
    # stream waits, every counter of the library together: one per served call where every block passed; the failed rv 0 fetches its soft buffers
    assert [x["waits"] for x in dec_h[:4]] == [1, 2, 1, 1], dec_h
    # fewer than through the UL-SCH hook, which never waits more often than upstream's loop (one block decoded in one pass costs both one visit)
    assert all(h["waits"] < u["waits"] <= p["waits"] for h, u, p in zip(dec_h[:4], dec_u[:4], dec_p[:4])), (dec_h, dec_u, dec_p)
    # the fallback: an 8-bit srslte_pusch_t goes back to upstream's function through the forwarder and decodes as the plain build does
    assert dec_h[4]["served"] == 0 and dec_h[4]["ulsch"] == 1 and dec_h[4]["dft"] == 1, dec_h[4]
    assert dec_h[4] == dict(dec_p[4], served=0) and pu_h[1] == sum(x["waits"] for x in dec_h[:4])
