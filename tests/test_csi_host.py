"""UE CSI feedback on the host (no GPU): the NumPy restatement of the measurement (tests/csi_ref.py) against the reference library, which
pins the sampling rule of the reference's compiled (AVX) build; the host report helpers against cqi.c; the decision function the kernel's
deciding lane runs; the two report generators against a line-by-line restatement of ue_dl.c:802-928.

Bounds: the project's scalar rule: 1e-4 relative for linear values, 1e-3 absolute for dB."""
import ctypes as C
import importlib
import itertools

import numpy as np
import pytest

import csi_ref as R
from _libs import p, ref

pkg = importlib.import_module("srslte-emane_amd")
needs_ref = pytest.mark.skipif(ref() is None, reason="oracle/_ref/libsrslte_ref.so is not built")
REL, DB = 1e-4, 1e-3

CASES = [(prb, cp, cond, snr) for prb in (6, 25, 50, 100) for cp in (True, False) for cond in ("well", "ill", "ortho") for snr in (-5, 5, 15, 25, 35)]


def _noise(ce, snr_db):
    return float(np.mean(np.abs(ce) ** 2) * 2 * 10 ** (-snr_db / 10))


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - b) / np.abs(b)))


@needs_ref
def test_restatement_matches_the_reference_on_drawn_channels():
    rng = np.random.default_rng(2026)
    worst = [0.0, 0.0, 0.0]
    for prb, cp, cond, snr in CASES:
        ce = R.draw_ce(rng, prb, cp, cond)
        noise = _noise(ce, snr)
        N = ce.shape[-1]
        r = R.Ref(ref(), ce, noise, prb, cp)
        m = R.measure(ce, noise, snr)
        # the same sample set by construction: _gen steps 24 up to nof_symbols, 96 floor(N / 96) / 24 = 4 floor(N / 96) samples
        g1, g2 = r.gen(1, 96 * (N // 96)), r.gen(2, 96 * (N // 96))
        e = [_rel(m["sinr_1l"], g1[1]), _rel(m["sinr_2l"], g2[1]), abs(float(m["cn_db"]) - float(r.cn()))]
        worst = [max(a, b) for a, b in zip(worst, e)]
        assert e[0] <= REL and e[1] <= REL and e[2] <= DB, (prb, cp, cond, snr, e)
    print("worst: 1 layer %.2e, 2 layers %.2e relative, cn %.2e dB" % tuple(worst))


@needs_ref
@pytest.mark.parametrize("cp", [True, False])
def test_dispatch_follows_the_avx_sample_count_not_gen_at_N(cp):
    """6 PRB: N = 1008 (864 extended): 4 floor(N / 96) = 40 (36) samples in the compiled dispatch, ceil(N / 24) = 42 (36) in _gen at N. The
    one-layer variant has no approximation in it, so it tells the sample sets apart: the dispatch with N equals _gen at 96 floor(N / 96)
    and, where the counts differ, not _gen at N."""
    rng = np.random.default_rng(7)
    for prb in (6, 15, 25, 100):
        ce = R.draw_ce(rng, prb, cp, "well", ripple=0.5)
        N = ce.shape[-1]
        noise = _noise(ce, 10)
        r = R.Ref(ref(), ce, noise, prb, cp)
        d, g_cut, g_all = r.dispatch(1, N)[1], r.gen(1, 96 * (N // 96))[1], r.gen(1, N)[1]
        assert _rel(d, g_cut) <= 1e-5, (prb, _rel(d, g_cut))
        n_pmi, n_cn = R.nof_samples(N)
        if n_pmi != n_cn:
            assert _rel(d, g_all) > 1e-3, (prb, _rel(d, g_all))
        # and the restatement uses the dispatch's count
        assert _rel(R.measure(ce, noise, 10)["sinr_1l"], d) <= REL
    assert R.nof_samples(1008) == (40, 42) and R.nof_samples(864) == (36, 36) and R.nof_samples(16800) == (700, 700)


def test_sample_counts_of_the_library_without_gpu():
    L = pkg.lib()
    for prb, cp in itertools.product((6, 15, 25, 50, 75, 100, 110), (True, False)):
        h = L.srslte_hip_csi_create(prb, 2, 2, 1 if cp else 0)
        assert h
        a, b = C.c_uint32(), C.c_uint32()
        assert L.srslte_hip_csi_nof_samples(h, C.byref(a), C.byref(b)) == 0
        assert (a.value, b.value) == R.nof_samples((14 if cp else 12) * 12 * prb)
        L.srslte_hip_csi_destroy(h)


def test_create_and_batch_refuse_without_gpu():
    L = pkg.lib()
    for args in ((25, 4, 2, 1), (25, 3, 2, 1), (25, 0, 2, 1), (25, 2, 3, 1), (25, 2, 0, 1), (5, 2, 2, 1), (111, 2, 2, 1)):
        assert L.srslte_hip_csi_create(*args) is None, args
    h = L.srslte_hip_csi_create(25, 2, 2, 1)
    one = C.create_string_buffer(64)
    for a in ((None, one, one, 1, one), (h, None, one, 1, one), (h, one, None, 1, one), (h, one, one, 1, None)):
        assert L.srslte_hip_csi_batch(*a, None) == -2
    assert L.srslte_hip_csi_set_snr_to_cqi_offset(None, 0.0) == -2 and L.srslte_hip_csi_set_snr_to_cqi_offset(h, float("nan")) == -2
    assert L.srslte_hip_csi_nof_samples(None, None, None) == -2
    assert L.srslte_hip_dl_rx_csi_batch(None, 1, one, None) == -2 and L.srslte_hip_dl_rx_set_snr_to_cqi_offset(None, 0.0) == -2
    assert L.srslte_hip_csi_decide(None, 1, 1, 1.0, 0.0, 0.0, 2, None) == -2
    L.srslte_hip_csi_destroy(h)
    L.srslte_hip_csi_destroy(None)


@needs_ref
def test_cqi_from_snr_matches_the_reference():
    for snr in list(np.arange(-10, 40, 0.05, dtype=np.float32)) + [float(t) for t in R.CQI_TO_SNR] + [float(np.nextafter(t, np.float32(-100))) for t in R.CQI_TO_SNR] + \
            [float("-inf"), float("inf")]:
        want = R.ref_cqi_from_snr(ref(), snr)
        assert pkg.cqi_from_snr(snr) == want == R.cqi_from_snr(snr), snr
    assert pkg.cqi_from_snr(float("nan")) == 0


def test_decisions_of_the_deciding_lane():
    """srslte_hip_csi_decide is the function lane 0 of the kernel runs. Sums are chosen so that every quotient is exact."""
    n, noise = 64, 0.5
    lin = lambda db: 10.0 ** (db / 10.0)

    def sums(s1, s2, cn):
        return [v * noise * n for v in s1] + [v * n for v in s2] + [cn * n]

    # the strict maximum from 0: the first of two equal entries wins, nothing positive keeps pmi 0
    r = pkg.csi_decide(sums([2, 4, 4, 1], [3, 3], 5.0), n, n, noise, 10.0)
    assert (r.pmi_1l, r.pmi_2l) == (1, 0) and list(r.sinr_1l) == [2, 4, 4, 1] and list(r.sinr_2l) == [3, 3]
    r = pkg.csi_decide(sums([0, -1, 0, -2], [-1, 0], 5.0), n, n, noise, 10.0)
    assert (r.pmi_1l, r.pmi_2l) == (0, 0)
    # cn < 17.0f, strictly: 17 exactly is rank one
    assert [pkg.csi_decide(sums([1, 1, 1, 1], [1, 1], c), n, n, noise, 0.0).ri_cn for c in (16.5, 17.0, 17.5)] == [1, 0, 0]
    assert pkg.csi_decide(sums([1, 1, 1, 1], [1, 1], 17.0), n, n, noise, 0.0).cn_db == 17.0
    # select_ri_pmi: two layers win by more than 0.1 dB ...
    r = pkg.csi_decide(sums([lin(10), 1, 1, 1], [1, lin(10.5)], 5.0), n, n, noise, 0.0)
    assert (r.ri, r.pmi) == (1, 1) and abs(r.sinr_db - 10.5) < 1e-4
    r = pkg.csi_decide(sums([lin(10), 1, 1, 1], [1, lin(10.05)], 5.0), n, n, noise, 0.0)
    assert (r.ri, r.pmi) == (0, 0) and abs(r.sinr_db - 10.0) < 1e-4
    # ... or by being above 20 dB although one layer is better still (the "> 20.0" clause)
    r = pkg.csi_decide(sums([1, 1, lin(30), 1], [lin(21), 1], 5.0), n, n, noise, 0.0)
    assert (r.ri, r.pmi) == (1, 0) and abs(r.sinr_db - 21.0) < 1e-4 and r.cqi_sinr == R.cqi_from_snr(21.0) == 10
    r = pkg.csi_decide(sums([1, 1, lin(30), 1], [lin(19), 1], 5.0), n, n, noise, 0.0)
    assert (r.ri, r.pmi) == (0, 2) and r.cqi_sinr == 15
    # the offset moves both CQIs, one antenna measures one layer only
    r = pkg.csi_decide(sums([lin(10), 1, 1, 1], [1, lin(25)], 5.0), n, n, noise, 3.9, 2.2, 1)
    assert (r.ri, r.pmi, r.ri_cn, r.cn_db, list(r.sinr_2l)) == (0, 0, 0, 0.0, [0, 0])
    assert r.cqi_sinr == R.cqi_from_snr(12.2) and r.cqi_wideband == R.cqi_from_snr(np.float32(3.9) + np.float32(2.2)) == 3
    # against the restatement's rule on drawn values
    rng = np.random.default_rng(3)
    for _ in range(300):
        s1, s2 = rng.uniform(0.1, 300, 4).astype(np.float32), rng.uniform(0.1, 300, 2).astype(np.float32)
        r = pkg.csi_decide(sums(s1, s2, 3.0), n, n, noise, 0.0)
        p1, p2 = int(np.argmax(r.sinr_1l)), int(np.argmax(r.sinr_2l))
        want = R.select_ri_pmi(lambda ri: (p2, np.array(r.sinr_2l, np.float32)) if ri else (p1, np.array(r.sinr_1l, np.float32)), 2)
        assert (r.ri, r.pmi) == want[:2] and abs(r.sinr_db - want[2]) < 1e-4


CFGS = [(t, pmi, four, rank, lab, L, N) for t in range(4) for pmi in (0, 1) for four in (0, 1) for rank in (0, 1) for lab in (0, 1) for L, N in ((0, 0), (3, 7), (11, 13))]


@needs_ref
def test_cqi_size_and_pack_match_the_reference():
    lib = ref()
    rng = np.random.default_rng(5)
    for t, pmi, four, rank, lab, L, N in CFGS:
        for enable in (1, 0):
            cfg = pkg.CqiCfg(t, enable, pmi, four, rank, lab, L, N)
            v = pkg.CqiValue(*[int(x) for x in rng.integers(0, [16, 8, 16, 16, 4, 1 << 26, 16, 1 << 26])])
            if t == 2:
                v.subband_diff_cqi &= 3  # a uint8 in the reference, two bits wide
            rc, rv = R.to_ref(cfg, v)
            assert pkg.cqi_size(cfg) == lib.srslte_cqi_size(C.byref(rc)), (t, pmi, four, rank, lab, L, N, enable)
            want = np.zeros(128, np.uint8)
            n_ref = lib.srslte_cqi_value_pack(C.byref(rc), C.byref(rv), p(want))
            n, bits = pkg.cqi_value_pack(cfg, v)
            assert n == n_ref and np.array_equal(bits, want[:64]) and not want[64:].any(), (t, pmi, four, rank, lab, L, N)
    assert pkg.cqi_size(pkg.CqiCfg(7, 1, 0, 0, 0, 0, 0, 0)) == -1
    assert pkg.cqi_value_pack(pkg.CqiCfg(3, 1, 1, 0, 1, 0, 0, 14), pkg.CqiValue())[0] == -2
    assert pkg.lib().srslte_hip_cqi_size(None) == -2 and pkg.lib().srslte_hip_cqi_value_pack(None, None, None) == -2


@needs_ref
@pytest.mark.parametrize("tdd", [False, True])
def test_periodic_schedule_matches_the_reference(tdd):
    lib = ref()
    lib.srslte_cqi_periodic_send.restype = C.c_bool
    lib.srslte_cqi_periodic_ri_send.restype = C.c_bool
    ft = 1 if tdd else 0
    ri_list = [0, 1, 5, 160, 161, 200, 321, 322, 400, 482, 483, 643, 644, 804, 805, 965, 966, 1023]
    for I in range(1024):
        rc = R.RefCqiReportCfg(True, False, I, 0, True, False, 0, 0, 0)
        for tti in list(range(40)) + [10239 - k for k in range(3)]:
            assert pkg.cqi_periodic_send(I, tti, tdd) == lib.srslte_cqi_periodic_send(C.byref(rc), C.c_uint32(tti), C.c_int(ft)), (I, tti)
        for I_ri in (ri_list if I % 7 == 0 or I < 20 else ri_list[:4]):
            rc.ri_idx = I_ri
            for tti in range(40):
                assert pkg.cqi_periodic_ri_send(I, I_ri, tti, tdd) == lib.srslte_cqi_periodic_ri_send(C.byref(rc), C.c_uint32(tti), C.c_int(ft)), (I, I_ri, tti)


@needs_ref
def test_no_subbands_matches_the_reference():
    for prb in range(0, 112):
        assert pkg.cqi_hl_get_no_subbands(prb) == ref().srslte_cqi_hl_get_no_subbands(C.c_int(prb)) == R.no_subbands(prb), prb


def _csi(rng, nof_ports=2, nof_rx=2):
    r = pkg.CsiRes()
    if nof_ports == 2:
        r.pmi_1l, r.pmi_2l = int(rng.integers(0, 4)), int(rng.integers(0, 2))
        r.ri_cn = int(rng.integers(0, 2))
        r.ri = int(rng.integers(0, 2)) if nof_rx == 2 else 0
        r.pmi = r.pmi_2l if r.ri else r.pmi_1l
        r.sinr_db = float(rng.uniform(-5, 35))
    return r


def _same(u, out, where):
    got = (out.cqi.type, bool(out.cqi.data_enable), bool(out.cqi.pmi_present), bool(out.cqi.four_antenna_ports), bool(out.cqi.rank_is_not_one), out.cqi.N,
           out.ri_len, out.ri, out.value.wideband_cqi, out.value.pmi, out.value.subband_cqi, out.value.subband_label, out.value.subband_diff_cqi,
           out.value.wideband_cqi_cw1, out.value.subband_diff_cqi_cw1)
    want = (u.type, u.data_enable, u.pmi_present, u.four_antenna_ports, u.rank_is_not_one, u.N, u.ri_len, u.ri, u.wideband_cqi, u.pmi, u.subband_cqi,
            u.subband_label, u.subband_diff_cqi, u.wideband_cqi_cw1, u.subband_diff_cqi_cw1)
    assert got == want, (where, got, want)
    # the row: srslte_cqi_size bits of srslte_cqi_value_pack
    cfg = pkg.CqiCfg(u.type, int(u.data_enable), int(u.pmi_present), int(u.four_antenna_ports), int(u.rank_is_not_one), 0, 0, u.N)
    assert out.cqi_len == max(0, pkg.cqi_size(cfg)), where
    bits = pkg.cqi_value_pack(cfg, out.value)[1] if u.data_enable else np.zeros(64, np.uint8)
    assert np.array_equal(np.frombuffer(bytes(out.cqi_bits), np.uint8), bits), where


def test_gen_cqi_aperiodic_follows_ue_dl_branch_for_branch():
    rng = np.random.default_rng(11)
    for tm, ports, rx, mode, prb, last_ri in itertools.product((1, 2, 3, 4), (1, 2), (1, 2), (30, 31), (6, 7, 8, 25, 50, 100), (0, 1)):
        for rep in range(4):
            csi = _csi(rng, ports, rx)
            off = float(rng.uniform(-3, 3))
            q = R.Ue(csi, tm, prb, ports, rx, last_ri=last_ri, aperiodic_mode=mode, snr_to_cqi_offset=off)
            cfg = pkg.CsiReportCfg(tm, prb, ports, rx, 0, 1, 1, 0, 0, 0, mode, off, last_ri)
            wb = int(rng.integers(0, 16))
            u = R.gen_cqi_aperiodic(q, wb)
            rc, out = pkg.csi_gen_cqi_aperiodic(csi, cfg, wb)
            assert rc == 0
            _same(u, out, (tm, ports, rx, mode, prb, last_ri))
            assert cfg.last_ri == q.last_ri
    assert pkg.csi_gen_cqi_aperiodic(pkg.CsiRes(), pkg.CsiReportCfg(4, 25, 2, 2, 0, 1, 1, 0, 0, 0, 12, 0.0, 0), 0)[0] == -2
    assert pkg.csi_gen_cqi_aperiodic(pkg.CsiRes(), pkg.CsiReportCfg(4, 110, 2, 2, 0, 1, 1, 0, 0, 0, 31, 0.0, 0), 0)[0] == 0
    two = pkg.CsiRes()
    two.ri = 1
    assert pkg.csi_gen_cqi_aperiodic(two, pkg.CsiReportCfg(4, 110, 2, 2, 0, 1, 1, 0, 0, 0, 31, 0.0, 0), 0)[0] == -2  # 65 bits
    L = pkg.lib()
    assert L.srslte_hip_csi_gen_cqi_aperiodic(None, None, 0, None) == -2 and L.srslte_hip_csi_gen_cqi_periodic(None, None, 0, 0, None) == -2


def test_gen_cqi_periodic_follows_ue_dl_branch_for_branch():
    rng = np.random.default_rng(12)
    send = (pkg.cqi_periodic_send, pkg.cqi_periodic_ri_send)
    seen = set()
    for tm, ports, rx, sub, conf, ri_present, tdd in itertools.product((1, 2, 3, 4), (1, 2), (1, 2), (0, 1), (1, 0), (1, 0), (False, True)):
        last_ri = int(rng.integers(0, 2))
        q = R.Ue(None, tm, 25, ports, rx, last_ri=last_ri, tdd=tdd, periodic_configured=bool(conf), ri_idx_present=bool(ri_present), I_cqi_pmi=3, I_ri=161,
                 format_is_subband=bool(sub), send=send)
        cfg = pkg.CsiReportCfg(tm, 25, ports, rx, 1 if tdd else 0, conf, ri_present, 3, 161, sub, 31, 0.0, last_ri)
        for tti in range(40):  # the state (last_ri) runs through the TTIs on both sides
            csi = _csi(rng, ports, rx)
            q.csi = csi
            wb = int(rng.integers(0, 16))
            u = R.gen_cqi_periodic(q, wb, tti)
            rc, out = pkg.csi_gen_cqi_periodic(csi, cfg, wb, tti)
            assert rc == 0
            _same(u, out, (tm, ports, rx, sub, conf, ri_present, tdd, tti))
            assert cfg.last_ri == q.last_ri
            seen.add((u.ri_len, u.data_enable, u.type, u.pmi_present, u.rank_is_not_one))
    # RI report, nothing, subband, wideband without PMI, wideband with PMI at rank one and above
    assert {(1, False, 0, False, False), (0, False, 0, False, False), (0, True, 1, False, False), (0, True, 0, False, False), (0, True, 0, True, False),
            (0, True, 0, True, True)} <= seen


def test_periodic_rank_is_not_one_comes_from_last_ri_not_from_the_measurement():
    """ue_dl.c:833: a wideband report between two RI reports describes the rank last REPORTED."""
    csi = pkg.CsiRes()
    csi.ri, csi.pmi, csi.pmi_1l, csi.pmi_2l = 1, 1, 2, 1
    cfg = pkg.CsiReportCfg(4, 25, 2, 2, 0, 1, 0, 0, 0, 0, 31, 0.0, 0)  # I_cqi_pmi 0: every second TTI; no RI reports
    rc, out = pkg.csi_gen_cqi_periodic(csi, cfg, 9, 0)
    assert rc == 0 and out.cqi.rank_is_not_one == 0 and out.value.pmi == 2 and out.cqi_len == 6 and cfg.last_ri == 0
    assert list(out.cqi_bits[:6]) == [1, 0, 0, 1, 1, 0]
    cfg.last_ri = 1
    csi.ri = 0
    rc, out = pkg.csi_gen_cqi_periodic(csi, cfg, 9, 2)
    assert out.cqi.rank_is_not_one == 1 and out.value.pmi == 1 and out.cqi_len == 8 and list(out.cqi_bits[:8]) == [1, 0, 0, 1, 0, 0, 0, 1]
    assert pkg.csi_gen_cqi_periodic(csi, cfg, 9, 1)[1].cqi_len == 0
