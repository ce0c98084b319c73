"""The link-time drop-in of INTEGRATION.md §1, performed: the reference's OWN test programs, compiled from /root/reference where they lie
together with the reference's lib/src/phy minus the translation units this library replaces, and linked against libsrslte_phy_hip.so
instead of those translation units and of FFTW (recipe: oracle/ref_hip.mk -> oracle/_ref/hip/, prebuilt binaries travel to the GPU box).
Each runs as a fresh child process with the arguments of the reference's CTest registration and must exit 0, i.e. reach what the
reference's test asserts - through srslte_ue_dl_* / srslte_enb_dl_* / srslte_pdsch_* / srslte_sch_* code that is the reference's, calling
srslte_ofdm_*, srslte_dft_*, srslte_chest_dl_*, srslte_demod_soft_*, srslte_tcod_*, srslte_tdec_*, srslte_cbsegm* that are ours."""
import os
import re
import subprocess

import pytest

from _libs import ORACLE_DIR
from refdrv import IQ_DIR

pytestmark = pytest.mark.gpu
BIN = os.path.join(ORACLE_DIR, "_ref", "hip")
need_bin = pytest.mark.skipif(not os.path.exists(os.path.join(BIN, "phy_dl_test")), reason="oracle/_ref/hip not built (needs /root/reference at build time)")
OUT = os.path.join(os.path.dirname(ORACLE_DIR), "gpurun_out")


def run(prog, args, timeout=600, env=None):
    r = subprocess.run([os.path.join(BIN, prog)] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout,
                       env=dict(os.environ, **env) if env else None)
    return r.returncode, r.stdout.decode(errors="replace")


CASES = [
    # lib/src/phy/dft/test/CMakeLists.txt:28-32
    ("ofdm_test", []), ("ofdm_test", ["-e"]), ("ofdm_test", ["-n", "6"]), ("ofdm_test", ["-e", "-n", "6"]),
    # lib/src/phy/utils/test/CMakeLists.txt:28-34
    ("dft_test", []), ("dft_test", ["-b"]), ("dft_test", ["-m"]), ("dft_test", ["-n"]), ("dft_test", ["-b", "-d"]), ("dft_test", ["-N", "255"]),
    ("dft_test", ["-N", "255", "-b", "-d"]),
    # lib/src/phy/fec/test/CMakeLists.txt:44-51
    ("turbodecoder_test", ["-n", "100", "-s", "1", "-l", "504", "-e", "1.0", "-t"]), ("turbodecoder_test", ["-n", "100", "-s", "1", "-l", "504", "-e", "2.0", "-t"]),
    ("turbodecoder_test", ["-n", "100", "-s", "1", "-l", "6144", "-e", "1.5", "-t"]), ("turbodecoder_test", ["-n", "1", "-s", "1", "-k", "-e", "0.5"]),
    # :35-36 - the reference's rate matcher over this library's srslte_cbsegm_* tables
    ("rm_turbo_test", ["-e", "1920"]), ("rm_turbo_test", ["-e", "8192"]),
    # lib/src/phy/ch_estimation/test/CMakeLists.txt:28-34
    ("chest_test_dl", ["-c", "0"]), ("chest_test_dl", ["-c", "1"]), ("chest_test_dl", ["-c", "2"]), ("chest_test_dl", ["-c", "0", "-r", "50"]),
    ("chest_test_dl", ["-c", "1", "-r", "50"]), ("chest_test_dl", ["-c", "2", "-r", "50"]),
    # :47-49 - the reference's chest_ul.c over this library's srslte_chest_average_pilots / _estimate_noise_pilots / filter taps
    ("chest_test_ul", ["-c", "0", "-r", "50"]), ("chest_test_ul", ["-c", "1", "-r", "50"]), ("chest_test_ul", ["-c", "2", "-r", "50"]),
    # lib/src/phy/modem/test/CMakeLists.txt:28-38
    ("modem_test", ["-n", "1024", "-m", "1"]), ("modem_test", ["-n", "1024", "-m", "2"]), ("modem_test", ["-n", "1024", "-m", "4"]),
    ("modem_test", ["-n", "1008", "-m", "6"]), ("modem_test", ["-n", "1024", "-m", "8"]),
    ("soft_demod_test", ["-n", "1024", "-m", "2"]), ("soft_demod_test", ["-n", "1008", "-m", "6"]), ("soft_demod_test", ["-n", "1024", "-m", "8"]),
    # lib/src/phy/phch/test/CMakeLists.txt:97-116 (grid level, TM1 / TM2), a few of the 143
    ("pdsch_test", ["-m", "10", "-n", "50", "-r", "1"]), ("pdsch_test", ["-m", "20", "-n", "100"]), ("pdsch_test", ["-n", "100"]),
    ("pdsch_test", ["-x", "1", "-a", "2", "-n", "25"]), ("pdsch_test", ["-x", "2", "-a", "2", "-n", "50"]), ("pdsch_test", ["-x", "3", "-a", "2", "-t", "0", "-n", "25"]),
    ("pusch_test", ["-n", "50", "-L", "50", "-m", "20"]),
    # :206-208 - PMCH over the MBSFN (extended-CP) OFDM modulator / demodulator and the decoder
    ("pmch_test", ["-m", "6", "-n", "50"]), ("pmch_test", ["-m", "15", "-n", "100"]), ("pmch_test", ["-m", "25", "-n", "100"]),
    # lib/src/phy/sync/test/CMakeLists.txt:69-77 - the reference's PSS / SSS search (FFT convolutions on srslte_dft_*) on subframes from srslte_ofdm_tx_*
    ("sync_test", ["-o", "100", "-c", "501"]), ("sync_test", ["-o", "400", "-c", "2"]), ("sync_test", ["-o", "100", "-e", "-c", "150"]),
    ("sync_test", ["-o", "400", "-e", "-c", "151"]), ("sync_test", ["-o", "100", "-p", "50", "-c", "501"]), ("sync_test", ["-o", "400", "-p", "50", "-c", "500"]),
    ("sync_test", ["-o", "100", "-e", "-p", "50", "-c", "133"]), ("sync_test", ["-o", "400", "-e", "-p", "50", "-c", "123"]),
    # lib/src/phy/phch/test/CMakeLists.txt:28-88 - the control channels' own tests: the reference's code over this library's srslte_chest_dl_res_*
    # and CRS functions (the channels themselves are outside the path)
    ("pbch_test", ["-p", "1", "-n", "6", "-c", "100"]), ("pbch_test", ["-p", "2", "-n", "6", "-c", "100"]), ("pbch_test", ["-p", "4", "-n", "6", "-c", "100"]),
    ("pbch_test", ["-p", "1", "-n", "50", "-c", "50"]), ("pbch_test", ["-p", "2", "-n", "50", "-c", "50"]), ("pbch_test", ["-p", "4", "-n", "50", "-c", "50"]),
    ("pcfich_test", ["-p", "1", "-n", "6"]), ("pcfich_test", ["-p", "2", "-n", "6"]), ("pcfich_test", ["-p", "4", "-n", "6"]),
    ("pcfich_test", ["-p", "1", "-n", "10"]), ("pcfich_test", ["-p", "2", "-n", "10"]), ("pcfich_test", ["-p", "4", "-n", "10"]),
    ("phich_test", ["-p", "1", "-n", "6"]), ("phich_test", ["-p", "2", "-n", "6"]), ("phich_test", ["-p", "4", "-n", "6", "-g", "1/6"]),
    ("phich_test", ["-p", "1", "-n", "6", "-e"]), ("phich_test", ["-p", "2", "-n", "6", "-e", "-l"]), ("phich_test", ["-p", "4", "-n", "6", "-e", "-l", "-g", "2"]),
    ("phich_test", ["-p", "1", "-n", "10", "-e"]), ("phich_test", ["-p", "2", "-n", "10", "-g", "2"]), ("phich_test", ["-p", "4", "-n", "10", "-e", "-l", "-g", "1/2"]),
    ("pdcch_test", ["-n", "6"]), ("pdcch_test", ["-n", "15"]), ("pdcch_test", ["-n", "25"]), ("pdcch_test", ["-n", "50"]), ("pdcch_test", ["-n", "75"]),
    ("pdcch_test", ["-n", "100"]), ("pdcch_test", ["-n", "6", "-p", "2"]), ("pdcch_test", ["-n", "15", "-p", "2"]), ("pdcch_test", ["-n", "25", "-p", "2"]),
    ("pdcch_test", ["-n", "50", "-p", "2"]), ("pdcch_test", ["-n", "75", "-p", "2"]), ("pdcch_test", ["-n", "100", "-p", "2"]),
    # lib/src/phy/phch/test/CMakeLists.txt:335-364 - the reference's PRACH generator and detector (prach.c) over srslte_dft_*: 839- / 139-point
    # Zadoff-Chu transforms and the long (I)FFTs of every bandwidth, formats 0-3, root sequences, zero-correlation zones, several preambles at once
    ("prach_test", []), ("prach_test", ["-n", "15"]), ("prach_test", ["-n", "25"]), ("prach_test", ["-n", "50"]), ("prach_test", ["-n", "75"]),
    ("prach_test", ["-n", "100"]), ("prach_test", ["-f", "0"]), ("prach_test", ["-f", "1"]), ("prach_test", ["-f", "2"]), ("prach_test", ["-f", "3"]),
    ("prach_test", ["-r", "1"]), ("prach_test", ["-r", "2"]), ("prach_test", ["-r", "3"]), ("prach_test", ["-z", "0"]), ("prach_test", ["-z", "2"]),
    ("prach_test", ["-z", "3"]), ("prach_test_multi", []), ("prach_test_multi", ["-n", "32"]), ("prach_test_multi", ["-n", "16"]),
    ("prach_test_multi", ["-n", "8"]), ("prach_test_multi", ["-n", "4"]),
    # :325-326 - PUCCH: the reference's chest_ul.c / pucch.c over this library's pilot averaging, noise estimation and filter taps (chest_common.c)
    ("pucch_test", []), ("pucch_test", ["-q"]),
    # lib/test/phy/CMakeLists.txt: the whole chain eNB -> UE, all four transmission modes go through our OFDM / estimator / decoder
    ("phy_dl_test", ["-p", "6", "-t", "1", "-m", "7"]), ("phy_dl_test", ["-p", "25", "-t", "2", "-m", "21"]), ("phy_dl_test", ["-p", "50", "-t", "4", "-m", "14"]),
    ("phy_dl_test", ["-p", "25", "-t", "4", "-m", "28"]), ("phy_dl_test", ["-p", "100", "-t", "1", "-q", "-m", "27"]),
    ("phy_dl_test", ["-p", "15", "-t", "1", "-m", "28"]), ("phy_dl_test", ["-p", "75", "-t", "2", "-m", "14"]),
]
# Not in the list: phy_dl_test -t 3 (TM3, large-delay CDD). It fails here with every code block KO, and the failing link is the
# reference's own srslte_predecoding_type(..., SRSLTE_TXSCHEME_CDD, ...), which no translation unit of ours replaces: as compiled in this
# image (gcc 11.4, the reference's -Ofast) its two sign masks come out as one constant (oracle/ref.mk, tests/test_oracle_vs_ref.py::
# test_reference_cdd_predecoder_on_a_noise_free_channel). test_tm3_with_the_reference_predecoder_as_written below runs the same test program
# with that ONE unit of the reference compiled with -fsigned-zeros: TM3 then passes through this library's OFDM, estimator and decoder.
TM3_CASES = [["-p", "25", "-t", "3", "-m", "14"], ["-p", "50", "-t", "3", "-m", "21"], ["-p", "100", "-t", "3", "-m", "28"], ["-p", "6", "-t", "3", "-m", "7"],
             ["-p", "75", "-t", "3", "-q", "-m", "27"]]


@pytest.mark.skipif(not os.path.exists(os.path.join(BIN, "phy_dl_test_sz")), reason="oracle/_ref/hip/phy_dl_test_sz not built")
@pytest.mark.parametrize("args", TM3_CASES, ids=[" ".join(a) for a in TM3_CASES])
def test_tm3_with_the_reference_predecoder_as_written(args):
    """lib/test/phy/CMakeLists.txt:33-54 runs TM3 at every bandwidth. The drop-in build of phy_dl_test whose only difference is
    -fsigned-zeros on the reference's mimo/precoding.c (oracle/ref_hip.mk: phy_dl_test_sz) passes them: what fails in `phy_dl_test -t 3` is
    the reference's predecoder as this image's compiler builds it, not what libsrslte_phy_hip.so serves."""
    rc, out = run("phy_dl_test_sz", args)
    assert rc == 0, out[-3000:]


@need_bin
@pytest.mark.parametrize("prog,args", CASES, ids=[" ".join([c[0]] + c[1]) for c in CASES])
def test_reference_ctest(prog, args):
    rc, out = run(prog, args)
    assert rc == 0, out[-3000:]


@need_bin
def test_whole_default_ctest_matrix_of_pdsch_test_and_pusch_test():
    """Every pdsch_test line of lib/src/phy/phch/test/CMakeLists.txt:97-200 (76: TM1-4, one and two codewords, every codebook index, codeword
    swap, 256QAM, six bandwidths; their argument lists are in tests/golden/ctest_pdsch_test_args.json) and the default pusch_test loops of
    :248-316 (36: with and without HARQ-ACK and a wide-band CQI report). scripts/dropin_full_matrix.py runs these plus the 241 phy_dl_test
    invocations of lib/test/phy/CMakeLists.txt:27-58 (profiles/r03/dropin_full_ctest_matrix.txt: 353 of 353 exit 0)."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import dropin_full_matrix
    rows = [r for r in dropin_full_matrix.matrix() if r[0] in ("pdsch_test", "pusch_test")]
    assert len(rows) == 76 + 36
    bad = []
    for prog, args in rows:
        rc, out = run(prog, args)
        if rc != 0:
            bad.append((prog, args, rc, out[-300:]))
    assert not bad, bad


@need_bin
def test_recorded_iq_ctests():
    """lib/src/phy/phch/test/CMakeLists.txt:233-238: the reference's file tests on its own captures (tests/golden/iq/)."""
    for prog, args, name in (("pbch_file_test", [], "signal.1.92M.dat"), ("pcfich_file_test", ["-c", "150", "-n", "50", "-p", "2"], "signal.10M.dat"),
                             ("phich_file_test", ["-c", "150", "-n", "50", "-p", "2"], "signal.10M.dat"),
                             ("pdcch_file_test", ["-c", "1", "-f", "3", "-n", "6", "-p", "1"], "signal.1.92M.amar.dat"),
                             ("pdsch_pdcch_file_test", ["-c", "1", "-f", "3", "-n", "6", "-p", "1"], "signal.1.92M.amar.dat"),
                             ("pmch_file_test", [], "pmch_100prbs_MCS2_SR0.bin")):
        rc, out = run(prog, args + ["-i", os.path.join(IQ_DIR, name)])
        assert rc == 0, prog + "\n" + out[-3000:]
        if prog == "pmch_file_test":
            assert "PMCH Decoded OK!" in out
        if prog == "pdsch_pdcch_file_test":
            assert "PDSCH Decoded OK!" in out


@need_bin
def test_phy_dl_test_headline_and_latency():
    """phy_dl_test -t 1 -p 100 -m 28 (TBS 75376, 13 code blocks of K = 5824): exit 0 = every transport block decoded, EVM and
    soft bits as the test demands. Its own timing print gives the latency of one subframe through the synchronous single-call API
    (srslte_ue_dl_decode_fft_estimate + srslte_pdsch_decode, host pointers in and out); recorded under gpurun_out/ for DESIGN.md - a printed
    figure, not a bound: a shared or slower box must not turn correct results red. What the bound stood for is checked structurally, from the
    library's own counters (SRSLTE_HIP_STATS): every transport block went through ONE device call (srslte_dlsch_decode2) and the UE path never
    fell back to a round trip per code block and pass (srslte_tdec_run_all / _iteration: 13 x up to 6 calls per subframe)."""
    rc, out = run("phy_dl_test", ["-p", "100", "-t", "1", "-m", "28"], timeout=900, env={"SRSLTE_HIP_STATS": "1"})
    assert rc == 0, out[-3000:]
    assert "BLER:   0.0%" in out
    m = re.search(r"UE:\s+([0-9.]+)\s+([0-9.]+)", out)
    assert m
    granted_mbps, processed = float(m.group(1)), float(m.group(2))
    us = granted_mbps * 1000.0 / processed if processed > 0 else float("inf")  # granted = bits per subframe / 1000 ; processed = bits per us
    os.makedirs(os.path.join(OUT, "r4"), exist_ok=True)
    with open(os.path.join(OUT, "r4", "dropin_phy_dl_test_100prb_mcs28.txt"), "w") as f:
        f.write(out[-1500:] + "\nUE receive path through the single-call API (srslte_dlsch_decode2 on the device, oracle/ref_hip.mk SCH_ON_DEVICE=1): "
                "%.0f us per subframe\n" % us)
    print("phy_dl_test -p 100 -m 28 through the drop-in: %.0f us per subframe (UE side)" % us)
    st = re.search(r"\[srslte_hip\] stats: stream_waits=(\d+) dlsch_decode2=(\d+) tdec_single_block_calls=(\d+)", out)
    assert st, out[-1500:]
    waits, decode2, single = (int(x) for x in st.groups())
    assert decode2 >= 1 and single == 0, "the drop-in's UE path fell back to a round trip per code block and pass: %s" % st.group(0)


@need_bin
def test_registered_log_handler_receives_diagnostics():
    """srslte_phy_log_register_handler (utils/phy_logger.c:37-52): with the library linked next to the reference's phy_logger.c its
    diagnostics go to the registered callback like the reference's ERROR() does (debug.h:75-89). oracle/dropin_log_test.c."""
    rc, out = run("dropin_log_test", [])
    assert rc == 0, out


@need_bin
def test_objects_built_at_max_prb_follow_the_cell():
    """srsue builds its objects once for the widest cell and resizes them when it learns the real one (cc_worker.cc:74,79): oracle/
    dropin_resize_test.c builds srslte_enb_dl / _ue_dl / _ue_ul / _enb_ul at SRSLTE_MAX_PRB and moves them through eight cells (6 to 100 PRB,
    1 and 2 ports, extended CP) with their set_cell calls, which resize this library's OFDM objects and estimator. On every cell each DCI is
    found and every PDSCH and PUSCH transport block arrives byte for byte."""
    rc, out = run("dropin_resize_test", [], timeout=300)
    cells = re.findall(r"^cell id=\d+ prb=(\d+) ports=(\d) cp=(\w+): (\w+)", out, re.M)
    assert rc == 0 and len(cells) == 8 and all(c[3] == "ok" for c in cells), out
    assert {c[0] for c in cells} >= {"6", "15", "25", "50", "75", "100"} and {c[1] for c in cells} == {"1", "2"} and "ext" in {c[2] for c in cells}
