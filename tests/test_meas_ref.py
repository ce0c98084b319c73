"""The restatement of tests/meas_ref.py itself (no device): its 10 frequency-domain replica grids against the reference's
srslte_refsignal_cs_put_sf + srslte_pss_put_slot + srslte_sss_put_slot, its FFT search against a direct-sum correlation, and whole rows
against planted captures."""
import ctypes as C

import numpy as np
import pytest

import meas_ref as mr
from _libs import RefCell, RefDlSfCfg, aligned, p, ref
from test_refsignal_helpers import RefSignal


@pytest.mark.skipif(ref() is None, reason="the reference build is absent")
@pytest.mark.parametrize("prb,cid", [(6, 0), (15, 301), (25, 150), (100, 503)])
def test_replica_grids_are_the_reference_put_functions(prb, cid):
    from dl_bcast_ref import _R
    R = _R()
    R.srslte_refsignal_cs_set_cell.argtypes = [C.c_void_p, RefCell]
    R.srslte_sss_generate.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    q = RefSignal()
    assert R.srslte_refsignal_cs_init(C.byref(q), 110) == 0
    assert R.srslte_refsignal_cs_set_cell(C.byref(q), RefCell(prb, 2, cid, 0, 0, 0, 0)) == 0
    pss, s0, s5 = aligned(62, np.complex64), aligned(62, np.float32), aligned(62, np.float32)
    assert R.srslte_pss_generate(pss.ctypes.data, cid % 3) == 0
    R.srslte_sss_generate(s0.ctypes.data, s5.ctypes.data, cid)
    want = mr.replica_grids(cid, prb)
    for i in range(10):
        g = aligned(14 * 12 * prb, np.complex64)
        g[:] = 0
        if i in (0, 5):
            R.srslte_pss_put_slot(pss.ctypes.data, g.ctypes.data, prb, 0)
            R.srslte_sss_put_slot((s5 if i else s0).ctypes.data, g.ctypes.data, prb, 0)
        sf = RefDlSfCfg()
        sf.tti = i
        for port in range(2):
            assert R.srslte_refsignal_cs_put_sf(C.byref(q), C.byref(sf), port, p(g)) == 0
        got = g.reshape(14, 12 * prb)
        assert np.array_equal(got != 0, want[i] != 0), i
        assert np.abs(got - want[i]).max() <= 2e-7, i


def test_replicas_have_the_power_set_cell_gives_them():
    """8 nof_prb CRS values of port 0 and as many of port 1 per subframe, each carrying 1 / (8 nof_prb) through an un-normalised N-point
    modulator: the body samples of subframe 1 hold 16 nof_prb N / (8 nof_prb)^2 = 2 N / (8 nof_prb) of energy."""
    for prb, N in ((6, 128), (25, 384), (100, 2048)):
        s = mr.replicas(7, prb, N)
        assert s.shape == (10, 15 * N)
        cp0, cp1 = mr.cp_len(N, 160), mr.cp_len(N, 144)
        body = sum(np.sum(np.abs(s[1, cp0 + (N + cp1) * l + (cp0 - cp1 if l >= 7 else 0):][:N]) ** 2) for l in mr.CRS_SYMBOLS)
        assert body == pytest.approx(2.0 * N / (8 * prb), rel=1e-9)


def test_fft_search_is_the_direct_sum_correlation():
    N, L = 128, 1920
    rng = np.random.default_rng(5)
    x = mr.capture([dict(id=33, start_sf=0, delay=700)], 6, N, 2, rng)
    seq0 = mr.replicas(33, 6, N)[0]
    a, b = mr.correlate_fft(x, seq0), mr.correlate_direct(x, seq0)
    assert a.shape == b.shape == (L,)
    assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
    assert int(np.argmax(np.abs(a))) == 700


@pytest.mark.parametrize("prb,nof_sf", [(6, 5), (15, 5), (6, 12)])
def test_planted_cells_come_out_where_they_were_planted(prb, nof_sf):
    N = mr.symbol_sz(prb)
    L = 15 * N
    rng = np.random.default_rng(prb * 100 + nof_sf)
    cells = [dict(id=150, start_sf=8, delay=L // 3, amp=1.0, cfo_hz=300.0), dict(id=29, start_sf=0, delay=0, amp=0.7, cfo_hz=-200.0)]
    x = mr.capture(cells, prb, N, nof_sf, rng)
    for c in cells:
        o = mr.run_one(x, nof_sf, c["id"], prb)
        idx = mr.planted_index(c, N, nof_sf)
        assert idx is not None and o["found"] == 1 and o["peak_index"] == idx, (c, o)
        assert o["sf_idx"] == (20 - idx // L) % 10 and o["nof_sf"] == (nof_sf if c["delay"] == 0 else nof_sf - 1)
        assert abs(o["cfo_Hz"] - c["cfo_hz"]) < 60.0
        assert o["margins"]["threshold"] > 0.2 and o["margins"]["peak"] > 0.2
    strong, weak = (mr.run_one(x, nof_sf, c["id"], prb) for c in cells)
    assert 2.0 < strong["rsrp_dBfs"] - weak["rsrp_dBfs"] < 4.2  # 20 log10(1 / 0.7) = 3.1 dB
    o = mr.run_one(x, nof_sf, 151, prb)  # the strong cell's neighbour id is not there
    assert o["found"] == 0 and o["peak_index"] == mr.UINT32_MAX and np.isnan(o["rsrp_dBfs"]) and np.isnan(o["cfo_Hz"])
