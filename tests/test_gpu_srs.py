"""The SRS on the device (srslte_hip_srs_tx_put, srslte_hip_srs_rx_batch, srslte_hip_ul_rx_batch_grants_pucch_srs): transmitted grids against
tests/golden/srs.npz (recorded from the reference's refsignal_ul.c), the sounding receiver against its float64 model of tests/srs_ref.py on
random grids - per fixture case, and at every legal block count J with three occupancies, three input scales and guarded output rows -, two
end-to-end scenes with gains, delays and noise (five UEs near the cell's timing; four with a 30 dB spread at the edge of the ta_us range on an
asymmetric comb), the grants pipeline with a PUSCH, a PUCCH and two SRS in one shortened subframe and, reduced, on 6, 50 (extended CP) and 100
PRB, one object holding ten sequence tables, refusals, and calls queued on one stream."""
import ctypes as C
import importlib

import numpy as np
import pytest

from gen_golden_srs import CASES
from srs_ref import E2E, E2E_HARD, M_SRS_B, bw_table_idx, case_cfg, case_ue, e2e_channel, e2e_truth, golden, rx_model, scene_channel

pkg = importlib.import_module("srslte-emane_amd")
pytestmark = pytest.mark.gpu

TA_SCALE = 2 * np.pi * 16 * 15e3 * 1e-6  # radians between neighbouring blocks per microsecond


def _srs(c, max_srs):
    return pkg.Srs(c["nof_prb"], c["cell_id"], c["bw_cfg"], max_srs=max_srs, subframe_config=c["subframe_config"], cp_ext=c["cp_ext"],
                   group_hopping_en=c["gh"], sequence_hopping_en=c["sh"], delta_ss=c["delta_ss"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_tx_put_matches_the_reference(name):
    """Every TTI of the case in one call of two subframes (the entry in the second), on a grid pre-filled with a sentinel: the SRS REs hold the
    recorded values bit for bit - the device copies the host generator's table, which the host test pins bit for bit - and nothing else changed."""
    c, g = CASES[name], golden()
    q = _srs(c, 1)
    rng = np.random.default_rng(11)
    for i, tti in enumerate(c["ttis"]):
        bg = (rng.normal(size=(2, q.grid_len)) + 1j * rng.normal(size=(2, q.grid_len))).astype(np.complex64)
        rc, got = q.put(bg, tti - 1, [case_ue(c, sf=1)])
        assert rc == 0
        idx = g[name + ".put_idx"][i]
        assert np.array_equal(got[1][idx].view(np.uint32), g[name + ".put_val"][i].view(np.uint32)), (name, tti)
        mask = np.ones(bg.shape, bool)
        mask[1][idx] = False
        assert np.array_equal(got[mask].view(np.uint32), bg[mask].view(np.uint32)), (name, tti)
    q.free()


def _check_against_model(res, ce, m, s=1.0):
    """s: the scale of the input the model was given (a unit-power grid times s); the one absolute bar, on h_j, scales with it."""
    J = m["ce"].size
    assert res.nof_ce == J
    assert np.abs(ce[:J] - m["ce"]).max() <= 1e-5 * s
    assert abs(res.rsrp - m["rsrp"]) <= 1e-4 * m["rsrp"]
    if m["nof_free"] == 0:
        assert res.noise_estimate == 0 and np.isnan(res.snr) and np.isnan(res.snr_db) and res.noise_estimate_dbm == -np.inf
    else:
        assert abs(res.noise_estimate - m["noise_estimate"]) <= 1e-4 * m["noise_estimate"]
        # the three derived figures from the device's own rsrp and noise_estimate, as chest_ul.c:317-321 derives them
        assert res.snr == pytest.approx(res.rsrp / res.noise_estimate, rel=1e-6)
        assert res.snr_db == pytest.approx(10 * np.log10(res.snr), abs=1e-4)
        assert res.noise_estimate_dbm == pytest.approx(10 * np.log10(res.noise_estimate) + 30, abs=1e-4)
    # ta_us through sum h_{j+1} conj(h_j): every h within 1e-5 moves the sum by at most 1e-5 sum (|h_j| + |h_{j+1}|); the angle then moves by at most
    # that over |sum| (a chord on the unit circle), and ta_us itself is a float (ulp 2.4e-7 us at 2 us)
    a = np.abs(m["ce"])
    slack = 1e-5 * s * float(np.sum(a[1:] + a[:-1])) / abs(m["corr"]) + 1e-6
    assert abs(np.exp(-1j * res.ta_us * TA_SCALE) - m["corr"] / abs(m["corr"])) <= slack
    assert abs(res.ta_us) <= 1e6 / (2 * 16 * 15e3) + 1e-3


@pytest.mark.parametrize("name", sorted(CASES))
def test_rx_matches_the_model_on_random_grids(name):
    """Random unit-power grids of three subframes; requests in the first and in the LAST subframe of the batch, with no other UE, with some, and
    with all eight cyclic shifts taken (no free bin: noise 0, snr NaN). p6_bw7 is J = 3, p100_bw0_B0 J = 72 (two wavefronts)."""
    c, g = CASES[name], golden()
    rng = np.random.default_rng(21)
    nof_sf, tti = 3, c["ttis"][0]
    q = _srs(c, 6)
    grid = ((rng.normal(size=(nof_sf, q.grid_len)) + 1j * rng.normal(size=(nof_sf, q.grid_len))) / np.sqrt(2)).astype(np.complex64)
    tti0 = tti  # subframe 0 is the case's first recorded TTI, the last subframe TTI tti0 + 2
    ues = [case_ue(c, sf=sf, cs_used=cs) for sf in (0, nof_sf - 1) for cs in (0, 0x5A, 0xFF)]
    rc, res, ce = q.rx(grid, tti0, ues)
    assert rc == 0
    cfg = case_cfg(c)
    for ue, r_, ce_ in zip(ues, res, ce):
        t = tti0 + ue.sf
        k0, M = pkg.srs_k0(cfg, ue, t), pkg.srs_M_sc(cfg, ue)
        if ue.sf == 0:  # the fixture's own position and sequence at the recorded TTI, the host generator's (pinned to the fixture) elsewhere
            assert (q.grid_len - 12 * c["nof_prb"]) + k0 == int(g[name + ".put_idx"][0][0])
            seq = g[name + ".gen"][0][0]
        else:
            seq = pkg.srs_gen(cfg, ue, t % 10)[0]
        y = grid[ue.sf].reshape(-1, 12 * c["nof_prb"])[-1][k0 + 2 * np.arange(M)]
        m = rx_model(y, seq, ue.n_srs, ue.cs_used)
        assert (m["nof_free"] == 0) == (ue.cs_used == 0xFF)
        _check_against_model(r_, ce_, m)
    assert {r_.nof_ce for r_ in res} == {int(g[name + ".M_sc"]) // 8}
    q.free()


# J = M_sc / 8 = 3 m_SRS / 4 -> (nof_prb, bw_cfg) with m_SRS,0 = 4 J / 3 (B = 0): every value the tables allow. 45-60 fill the first wavefront
# almost and leave the second idle, 72 alone crosses into it.
J_CELLS = {3: (6, 7), 6: (25, 6), 9: (15, 5), 12: (25, 4), 15: (25, 3), 18: (25, 2), 24: (50, 4), 27: (50, 3), 30: (50, 2), 36: (50, 0), 45: (100, 5),
           48: (100, 4), 54: (100, 3), 60: (100, 2), 72: (100, 0)}


def test_j_cells_are_every_block_count_of_the_tables():
    assert {3 * m // 4 for t in M_SRS_B for row in t for m in row} == set(J_CELLS)
    assert all(M_SRS_B[bw_table_idx(P)][0][bw] * 3 == 4 * J for J, (P, bw) in J_CELLS.items())


@pytest.mark.parametrize("J", sorted(J_CELLS))
def test_rx_matches_the_model_at_every_block_count(J):
    """A random grid of two subframes at scales 2^-10, 1 and 2^10 (exact in float), three requests in each subframe: no other UE, the asymmetric
    occupancy 0x16, all eight shifts. Against the model at the file's bars (h_j 1e-5 times the scale, rsrp and noise 1e-4 relative). Against the
    unit-scale device result: a power of two scales every product and sum of the kernel exactly, so h_j times s bit for bit, rsrp and noise times
    s^2 (1e-4 relative), snr and ta_us - ratios of exactly scaled numbers - and nof_ce the same bits. The outputs are pre-filled with 0x5A and two
    rows longer than the call: h_j from J on, and both guard rows of ce and of the records, keep the fill (at J = 72 a row is full and the next
    begins at once)."""
    P, bw = J_CELLS[J]
    q = pkg.Srs(P, 90 + J, bw, max_srs=6)
    cfg, tti0, nof_sf = q.cfg, 7, 2
    rng = np.random.default_rng(100 + J)
    grid = ((rng.normal(size=(nof_sf, q.grid_len)) + 1j * rng.normal(size=(nof_sf, q.grid_len))) / np.sqrt(2)).astype(np.complex64)
    ues = [pkg.SrsUe.make(sf, n_srs=(3 + 2 * i + 5 * sf) % 8, k_tc=(sf + i) % 2, cs_used=cs) for sf in range(nof_sf) for i, cs in enumerate((0, 0x16, 0xFF))]
    n, unit = len(ues), None
    for s in (1.0, 2.0 ** -10, 2.0 ** 10):
        gs = (grid * np.float32(s)).astype(np.complex64)
        dg, dr, dc = pkg.DevBuf.from_host(gs), pkg.DevBuf(C.sizeof(pkg.SrsRes) * (n + 2)), pkg.DevBuf(8 * pkg.SRS_MAX_CE * (n + 2))
        for d in (dr, dc):
            pkg.lib().srslte_hip_memset(d.ptr, 0x5A, d.nbytes)
        assert q.rx_device(dg.ptr, tti0, nof_sf, ues, dr.ptr, dc.ptr) == 0
        pkg.sync()
        res, ce = pkg.Srs.read(dr, dc, n + 2)
        raw_ce = ce.view(np.uint8).reshape(n + 2, pkg.SRS_MAX_CE, 8)
        assert (raw_ce[:n, J:] == 0x5A).all() and (raw_ce[n:] == 0x5A).all() and not (raw_ce[:n, :J] == 0x5A).all(axis=2).any()
        assert all(bytes(r_) == b"\x5a" * C.sizeof(pkg.SrsRes) for r_ in res[n:])
        for ue, r_, ce_ in zip(ues, res, ce):
            t = tti0 + ue.sf
            k0, M = pkg.srs_k0(cfg, ue, t), pkg.srs_M_sc(cfg, ue)
            assert M == 8 * J
            y = gs[ue.sf].reshape(-1, 12 * P)[-1][k0 + 2 * np.arange(M)]
            m = rx_model(y, pkg.srs_gen(cfg, ue, t % 10)[0], ue.n_srs, ue.cs_used)
            assert m["nof_free"] == {0: 7, 0x16: 7 - bin(0x16 & ~(1 << ue.n_srs)).count("1"), 0xFF: 0}[ue.cs_used]
            _check_against_model(r_, ce_, m, s)
        if unit is None:
            unit = (res, ce.copy())
            continue
        for a, b, ca, cb in zip(unit[0][:n], res, unit[1], ce):
            assert np.array_equal((ca[:J] * np.float32(s)).view(np.uint32), cb[:J].view(np.uint32))
            assert abs(b.rsrp - a.rsrp * s * s) <= 1e-4 * a.rsrp * s * s and abs(b.noise_estimate - a.noise_estimate * s * s) <= 1e-4 * a.noise_estimate * s * s
            same = lambda x, y_: np.float32(x).view(np.uint32) == np.float32(y_).view(np.uint32)
            assert same(a.ta_us, b.ta_us) and same(a.snr, b.snr) and a.nof_ce == b.nof_ce == J
    q.free()


def test_rx_leaves_the_rest_of_a_ce_row_alone():
    c = CASES["p6_bw7"]
    q = _srs(c, 2)
    grid = np.ones((1, q.grid_len), np.complex64)
    ues = [case_ue(c), case_ue(c)]
    dg, dr, dc = pkg.DevBuf.from_host(grid), pkg.DevBuf(C.sizeof(pkg.SrsRes) * 2), pkg.DevBuf(8 * pkg.SRS_MAX_CE * 2)
    pkg.lib().srslte_hip_memset(dc.ptr, 0x5A, dc.nbytes)
    assert q.rx_device(dg.ptr, c["ttis"][0], 1, ues, dr.ptr, dc.ptr) == 0
    pkg.sync()
    raw = dc.to_host(np.uint8).reshape(2, pkg.SRS_MAX_CE, 8)
    assert (raw[:, 3:] == 0x5A).all() and not (raw[:, :3] == 0x5A).all()
    q.free()


def test_end_to_end_five_ues():
    """tests/srs_ref.py E2E: each UE's SRS from srslte_hip_srs_tx_put on its own grid, gain and delay (a phase ramp over the subcarriers) applied
    per UE, the five summed, complex white noise of variance sigma^2 added, then srslte_hip_srs_rx_batch with the comb's shifts in cs_used.
    h_j within 5 sigma / sqrt(8) of gain times ramp at the block's centre, ta_us within 0.1 us of the delay (from the 0.52 us timing-advance step),
    noise_estimate within 5 / sqrt(J |F|) of sigma^2. The model alone stays inside the same bounds (checked here too, before the device)."""
    P, s2 = E2E["nof_prb"], E2E["sigma2"]
    q = pkg.Srs(P, E2E["cell_id"], E2E["bw_cfg"], max_srs=8)
    cfg, tti = q.cfg, 4
    ues = [pkg.SrsUe.make(0, n_srs=u["n_srs"], k_tc=u["k_tc"], cs_used=0b01010101 if u["k_tc"] == 0 else 0b1) for u in E2E["ues"]]
    tx = []
    for ue in ues:  # a put writes, it does not add: each UE its own grid, the air sums them
        rc, g = q.put(np.zeros((1, q.grid_len), np.complex64), tti, [ue])
        assert rc == 0 and np.count_nonzero(g) == pkg.srs_M_sc(cfg, ue)
        tx.append(g[0][-12 * P:])
    grid = np.zeros((1, q.grid_len), np.complex64)
    grid[0][-12 * P:] = e2e_channel(tx)
    rc, res, ce = q.rx(grid, tti, ues)
    assert rc == 0
    for u, ue, r_, ce_ in zip(E2E["ues"], ues, res, ce):
        k0, M = pkg.srs_k0(cfg, ue, tti), pkg.srs_M_sc(cfg, ue)
        J, nfree = M // 8, 4 if u["k_tc"] == 0 else 7
        assert J == 36 and r_.nof_ce == J
        truth = e2e_truth(u, k0, J)
        m = rx_model(grid[0][-12 * P:][k0 + 2 * np.arange(M)], pkg.srs_gen(cfg, ue, tti % 10)[0], ue.n_srs, ue.cs_used)
        for h, ta, noise in ((m["ce"], m["ta_us"], m["noise_estimate"]), (ce_[:J], r_.ta_us, r_.noise_estimate)):
            assert np.abs(h - truth).max() <= 5 * np.sqrt(s2) / np.sqrt(8)
            assert abs(ta - u["tau_us"]) <= 0.1
            assert abs(noise - s2) <= 5 / np.sqrt(J * nfree) * s2
    q.free()


def test_end_to_end_asymmetric_comb_strong_and_weak():
    """tests/srs_ref.py E2E_HARD, built as test_end_to_end_five_ues: comb 0 carries shifts 0, 1, 3 (cs_used 0b1011) with gains 1.0, 0.1, 3.0 at
    +1.9, 0, -1.9 us, comb 1 one UE of gain 0.5 at +1.9 us; sigma^2 0.09, noise seed 8. The bounds have that test's form plus the leakage the
    float64 model shows on the noise-free scene (half a bin of delay is no longer orthogonal to the other shifts over 8 REs):
      h_j             within L_h + 5 sigma / sqrt(8) of gain times ramp at the block centre, L_h = max_j |h_j - truth| of the noise-free model:
                      L_h = 0.685, 0.680, 1.041, 0.152 for the four UEs, so bounds 1.215, 1.211, 1.572, 0.683; the model is at 0.747, 0.785,
                      1.104, 0.295. The 0.1-gain UE is NOT recovered - the leakage into its bin is 0.68, seven times its gain: that is the
                      estimator (an 8-RE block DFT), and the device has to show the same leakage, which the 1e-5 comparison with the model
                      below holds it to.
      noise_estimate  within 5 sigma^2 / sqrt(J |F|) + L_n of sigma^2, L_n the noise-free model's noise_estimate (7.541 on comb 0, 0.148 on comb
                      1: bounds 7.575 and 0.176; the model is at 7.413 and 0.146 off). The product of leakage and noise, which this form leaves
                      out, has a standard deviation of sqrt(2 L_n sigma^2 / (J |F|)) = 0.087 on comb 0: the bound holds for this noise seed and
                      for 7, 9, 10, not for every seed (11 misses by 0.08).
      ta_us           the sign of the delay for the three UEs at +-1.9 us, and within |ta_0 - tau| + asin(d / |corr_0|) / (2 pi 16 15e3 us) of
                      it, with ta_0, corr_0, h_0 of the noise-free model and d = 5 sqrt(sigma_h^2 sum_j (|h_0,j|^2 + |h_0,j+1|^2) + (J - 1)
                      sigma_h^4), sigma_h^2 = sigma^2 / 8 the noise on one h_j: 5 sigma of what noise adds to sum h_j+1 conj(h_j). Bounds 0.19,
                      2.15 (no statement: the weak UE's sum is leakage), 0.042, 0.25 us; the model is 0.088, 1.97, 0.000, 0.005 us off.
    The model is checked against all three first, then the device against the same bounds and against the model at the file's bars."""
    S = E2E_HARD
    P, s2 = S["nof_prb"], S["sigma2"]
    q = pkg.Srs(P, S["cell_id"], S["bw_cfg"], max_srs=8)
    cfg, tti = q.cfg, 4
    ues = [pkg.SrsUe.make(0, n_srs=u["n_srs"], k_tc=u["k_tc"], cs_used=u["cs_used"]) for u in S["ues"]]
    tx = []
    for ue in ues:
        rc, g = q.put(np.zeros((1, q.grid_len), np.complex64), tti, [ue])
        assert rc == 0 and np.count_nonzero(g) == pkg.srs_M_sc(cfg, ue)
        tx.append(g[0][-12 * P:])
    clean = scene_channel(S, tx, noise=False)
    grid = np.zeros((1, q.grid_len), np.complex64)
    grid[0][-12 * P:] = scene_channel(S, tx, seed=8)
    rc, res, ce = q.rx(grid, tti, ues)
    assert rc == 0
    for u, ue, r_, ce_ in zip(S["ues"], ues, res, ce):
        k0, M = pkg.srs_k0(cfg, ue, tti), pkg.srs_M_sc(cfg, ue)
        J, nfree = M // 8, 5 if u["k_tc"] == 0 else 7
        assert J == 36 and r_.nof_ce == J
        truth, seq, sel = e2e_truth(u, k0, J), pkg.srs_gen(cfg, ue, tti % 10)[0], k0 + 2 * np.arange(M)
        m0 = rx_model(clean[sel], seq, ue.n_srs, ue.cs_used)
        m = rx_model(grid[0][-12 * P:][sel], seq, ue.n_srs, ue.cs_used)
        assert m["nof_free"] == nfree
        bound_h = np.abs(m0["ce"] - truth).max() + 5 * np.sqrt(s2) / np.sqrt(8)
        bound_n = 5 / np.sqrt(J * nfree) * s2 + m0["noise_estimate"]
        a2, sh2 = np.abs(m0["ce"]) ** 2, s2 / 8
        d = 5 * np.sqrt(sh2 * np.sum(a2[1:] + a2[:-1]) + (J - 1) * sh2 * sh2)
        bound_ta = abs(m0["ta_us"] - u["tau_us"]) + (np.arcsin(d / abs(m0["corr"])) / TA_SCALE if d < abs(m0["corr"]) else np.inf)
        print("n_srs %d: bounds h %.3f noise %.3f ta %.3f" % (ue.n_srs, bound_h, bound_n, bound_ta))
        for who, h, ta, noise in (("model", m["ce"], m["ta_us"], m["noise_estimate"]), ("device", ce_[:J], r_.ta_us, r_.noise_estimate)):
            print("  %s: h %.3f noise %.3f ta %.3f" % (who, np.abs(h - truth).max(), abs(noise - s2), abs(ta - u["tau_us"])))
            assert np.abs(h - truth).max() <= bound_h
            assert abs(noise - s2) <= bound_n
            assert abs(ta - u["tau_us"]) <= bound_ta
            if u["tau_us"]:
                assert np.sign(ta) == np.sign(u["tau_us"]) and bound_ta < abs(u["tau_us"])
        _check_against_model(r_, ce_, m)
    q.free()


def test_pipeline_with_pusch_pucch_and_two_srs():
    """One shortened PUSCH, one shortened PUCCH and two SRS (two cyclic shifts of one comb) in one subframe, summed in the time domain: the
    transport block and the PUCCH result of _grants_pucch_srs are those of _grants_pucch on the same samples, the SRS results those of
    srslte_hip_srs_rx_batch on the grid of a stand-alone demodulation; then the entry with either object NULL."""
    prb, nsf, cell_id, tti0 = 25, 2, 77, 230
    rng = np.random.default_rng(5)
    grant = pkg.UlGrant.make(1, 0x400, 10, 10, 1, 1544, n_dmrs=3)
    data = rng.integers(0, 256, 1544 // 8, dtype=np.uint8)
    utx = pkg.UlTx(cell_id, prb, 0x400, 1, 1544, 10, 10, 0, nsf, shortened=True, max_grants=1)
    iq = utx.encode_grants([data], tti0, nsf, [grant]).reshape(nsf, -1)
    utx.free()
    kw = dict(delta_pucch_shift=2, N_cs=0, n_rb_2=1, N_pucch_1=1, threshold_format1=0.8, threshold_data_valid_format1a=0.9, threshold_data_valid_format2=0.5)
    req = pkg.PucchReq.make(1, 0x46, ack_len=2, ncce=3, shortened=True)
    ctx = pkg.UlCtrlTx(prb, cell_id, max_pucch=1, **kw)
    srs = pkg.Srs(prb, cell_id, 2, max_srs=2)  # m_SRS,0 = 24: PRB 0-23, across the PUSCH's PRBs (10-19) and one of the PUCCH's
    ues = [pkg.SrsUe.make(1, n_srs=1, k_tc=1, cs_used=0b1010), pkg.SrsUe.make(1, n_srs=3, k_tc=1, cs_used=0b1010)]
    ofdm = pkg.Ofdm(prb, True, rx=False)
    ofdm.set_freq_shift(0.5)
    rc, g = ctx.put(np.zeros((nsf, ctx.grid_len), np.complex64), tti0, [pkg.PucchTx.make(req, ack=(1, 0))])
    assert rc == 0
    iq = iq + ofdm.tx_sf(g)
    for ue in ues:
        rc, g = srs.put(np.zeros((nsf, srs.grid_len), np.complex64), tti0, [ue])
        assert rc == 0
        iq = iq + ofdm.tx_sf(g)
    iq = iq.astype(np.complex64)
    ctrl = pkg.UlCtrl(prb, cell_id, max_pucch=1, **kw)
    rx1 = pkg.UlRx(cell_id, prb, 0x400, 1, 1544, 10, 10, 0, 6, nsf, shortened=True, max_grants=1)
    rx2 = pkg.UlRx(cell_id, prb, 0x400, 1, 1544, 10, 10, 0, 6, nsf, shortened=True, max_grants=1)
    rc, tb1, ok1, p1 = rx1.decode_grants_pucch(iq, tti0, [grant], ctrl, [req])
    assert rc == 0
    rc, tb2, ok2, p2, sres, sce = rx2.decode_grants_pucch_srs(iq, tti0, [grant], ctrl, [req], srs, ues)
    assert rc == 0 and ok1.all() and np.array_equal(ok1, ok2)
    n = grant.tbs // 8 + 3
    assert np.array_equal(tb1[0][:n], tb2[0][:n]) and np.array_equal(tb2[0][:grant.tbs // 8], data)
    assert bytes(p1[0]) == bytes(p2[0]) and p2[0].detected == 1 and list(p2[0].ack) == [1, 0]
    rxo = pkg.Ofdm(prb, True, rx=True)
    rxo.set_freq_shift(-0.5)
    rc, alone, ace = srs.rx(rxo.rx_sf(iq), tti0, ues)
    assert rc == 0
    for a, b, ca, cb in zip(alone, sres, ace, sce):
        assert bytes(a) == bytes(b) and np.array_equal(ca[:a.nof_ce].view(np.uint32), cb[:a.nof_ce].view(np.uint32))
        assert a.snr > 100 and abs(a.ta_us) < 0.05 and a.nof_ce == 18  # a clean flat channel: the SRS is there, alone in its bin
    # either object NULL: the other's results stay, the PUSCH's too; the existing entry point is the srs = NULL case
    rc, tb3, ok3, p3, s3, _ = rx2.decode_grants_pucch_srs(iq, tti0, [grant], ctrl, [req], None, [])
    assert rc == 0 and ok3.all() and np.array_equal(tb3[0][:n], tb1[0][:n]) and bytes(p3[0]) == bytes(p1[0])
    rc, tb4, ok4, _, s4, c4 = rx2.decode_grants_pucch_srs(iq, tti0, [grant], None, [], srs, ues)
    assert rc == 0 and ok4.all() and np.array_equal(tb4[0][:n], tb1[0][:n]) and all(bytes(a) == bytes(b) for a, b in zip(s4, alone))
    rc, _, _, _, s5, _ = rx2.decode_grants_pucch_srs(iq, tti0, [], None, [], srs, ues)  # no grants: the demodulation and the SRS batch alone
    assert rc == 0 and all(bytes(a) == bytes(b) for a, b in zip(s5, alone))
    # an SRS object of another cell, and a bad entry, are refused before anything is queued
    other = pkg.Srs(prb, cell_id + 1, 2, max_srs=2)
    assert rx2.decode_grants_pucch_srs(iq, tti0, [grant], ctrl, [req], other, ues)[0] == -2
    assert rx2.decode_grants_pucch_srs(iq, tti0, [grant], ctrl, [req], srs, [pkg.SrsUe.make(2)])[0] == -2
    for o in (ctx, srs, other, ofdm, rxo, ctrl, rx1, rx2):
        o.free()


# nof_prb, cp_ext, bw_cfg, J, the PUSCH (L_prb, n_prb, tbs; QPSK): shapes the UL tests run on such cells
PIPE_CELLS = [(6, False, 7, 3, (6, 0, 808)), (50, True, 3, 27, (6, 12, 808)), (100, False, 0, 72, (10, 10, 1544))]


@pytest.mark.parametrize("prb,cp_ext,bw_cfg,J,pusch", PIPE_CELLS)
def test_pipeline_on_other_cells(prb, cp_ext, bw_cfg, J, pusch):
    """test_pipeline_with_pusch_pucch_and_two_srs reduced, on the smallest cell, on an extended-CP cell (nsym = 12 in the position of the SRS) and
    with J = 72 inside the pipeline: three subframes, a shortened PUSCH in each, two SRS (two shifts of one comb) in subframe 0 and two in
    subframe 2, no PUCCH. The transport blocks are those of _grants_pucch on the same samples, the SRS records and ce those of
    srslte_hip_srs_rx_batch on a stand-alone demodulation, byte for byte."""
    nsf, cell_id, tti0 = 3, 77, 238  # subframe 2 is TTI 240: row 0 of the sequence tables after row 8
    L, n0, tbs = pusch
    rng = np.random.default_rng(50 + prb)
    grants = [pkg.UlGrant.make(sf, 0x400, L, n0, 1, tbs, n_dmrs=(3 + sf) % 8) for sf in range(nsf)]
    datas = [rng.integers(0, 256, tbs // 8, dtype=np.uint8) for _ in range(nsf)]
    utx = pkg.UlTx(cell_id, prb, 0x400, 1, tbs, L, n0, 0, nsf, shortened=True, max_grants=nsf, cp_ext=cp_ext)
    iq = utx.encode_grants(datas, tti0, nsf, grants).reshape(nsf, -1)
    utx.free()
    srs = pkg.Srs(prb, cell_id, bw_cfg, max_srs=4, cp_ext=cp_ext)
    ues = [pkg.SrsUe.make(sf, n_srs=n, k_tc=sf // 2, cs_used=0b100010) for sf in (0, 2) for n in (1, 5)]
    ofdm = pkg.Ofdm(prb, not cp_ext, rx=False)
    ofdm.set_freq_shift(0.5)
    for ue in ues:
        rc, g = srs.put(np.zeros((nsf, srs.grid_len), np.complex64), tti0, [ue])
        assert rc == 0
        iq = iq + ofdm.tx_sf(g)
    iq = iq.astype(np.complex64)
    ctrl = pkg.UlCtrl(prb, cell_id, max_pucch=1, cp_ext=cp_ext, delta_pucch_shift=2, N_cs=0, n_rb_2=1, N_pucch_1=1)
    rx1 = pkg.UlRx(cell_id, prb, 0x400, 1, tbs, L, n0, 0, 6, nsf, shortened=True, max_grants=nsf, cp_ext=cp_ext)
    rx2 = pkg.UlRx(cell_id, prb, 0x400, 1, tbs, L, n0, 0, 6, nsf, shortened=True, max_grants=nsf, cp_ext=cp_ext)
    rc, tb1, ok1, _ = rx1.decode_grants_pucch(iq, tti0, grants, ctrl, [])
    assert rc == 0
    rc, tb2, ok2, _, sres, sce = rx2.decode_grants_pucch_srs(iq, tti0, grants, None, [], srs, ues)
    assert rc == 0 and ok1.all() and np.array_equal(ok1, ok2)
    for p_ in range(nsf):
        assert np.array_equal(tb1[p_][:tbs // 8 + 3], tb2[p_][:tbs // 8 + 3]) and np.array_equal(tb2[p_][:tbs // 8], datas[p_])
    rxo = pkg.Ofdm(prb, not cp_ext, rx=True)
    rxo.set_freq_shift(-0.5)
    rc, alone, ace = srs.rx(rxo.rx_sf(iq), tti0, ues)
    assert rc == 0
    for a, b, ca, cb in zip(alone, sres, ace, sce):
        assert bytes(a) == bytes(b) and np.array_equal(ca[:a.nof_ce].view(np.uint32), cb[:a.nof_ce].view(np.uint32))
        assert a.snr > 100 and abs(a.ta_us) < 0.05 and a.nof_ce == J  # a clean flat channel: the SRS is there, alone in its bin
    for o in (srs, ofdm, rxo, ctrl, rx1, rx2):
        o.free()


def test_one_object_holds_many_tables():
    """One object on 100 PRB (bw_cfg 0: M_sc 576, 288, 144, 24 at B 0-3), one put and one receive call of 14 entries over three subframes that
    need ten (M_sc, n_srs) tables and three rows (tti % 10) of them, in an order that is not the tables'. No two entries share an RE. The put
    writes srslte_hip_srs_gen at srslte_hip_srs_k0 and nothing else; the receiver reads |h_j| = 1 and rsrp = 1 from those grids; and the same two
    calls again on the same object - every table a cache hit - give the same bytes."""
    P, tti0, nsf = 100, 8, 3  # rows 8, 9, 0
    # sf, B, n_rrc, n_srs, k_tc: a comb of a subframe holds one B 0 entry, or entries whose n_rrc put them in different parts of the band
    spec = [(0, 0, 0, 5, 0), (0, 1, 0, 2, 1), (0, 1, 12, 7, 1), (1, 1, 12, 2, 0), (1, 2, 0, 1, 0), (1, 2, 6, 4, 0), (1, 0, 0, 0, 1), (2, 3, 0, 3, 0),
            (2, 3, 1, 6, 0), (2, 3, 23, 3, 0), (2, 2, 12, 4, 0), (2, 1, 0, 7, 1), (2, 2, 18, 0, 1), (2, 3, 13, 5, 1)]
    spec = [spec[i] for i in np.random.default_rng(6).permutation(len(spec))]
    ues = [pkg.SrsUe.make(sf, B=B, b_hop=3, n_rrc=n_rrc, n_srs=n, k_tc=k, cs_used=1 << n) for (sf, B, n_rrc, n, k) in spec]
    q = pkg.Srs(P, 311, 0, max_srs=len(ues), group_hopping_en=True)
    cfg = q.cfg
    tables = [(pkg.srs_M_sc(cfg, ue), ue.n_srs) for ue in ues]
    assert len(set(tables)) == 10 and len({t[0] for t in tables}) == 4 and tables != sorted(tables) and len(ues) >= 12
    rng = np.random.default_rng(61)
    bg = (rng.normal(size=(nsf, q.grid_len)) + 1j * rng.normal(size=(nsf, q.grid_len))).astype(np.complex64)
    want, taken = bg.copy(), np.zeros(bg.shape, bool)
    for ue in ues:
        idx = 13 * 12 * P + pkg.srs_k0(cfg, ue, tti0 + ue.sf) + 2 * np.arange(pkg.srs_M_sc(cfg, ue))
        assert not taken[ue.sf][idx].any()
        taken[ue.sf][idx] = True
        want[ue.sf][idx] = pkg.srs_gen(cfg, ue, (tti0 + ue.sf) % 10)[0]
    outs = []
    for _ in range(2):
        rc, got = q.put(bg, tti0, ues)
        assert rc == 0 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        rc, res, ce = q.rx(got, tti0, ues)
        assert rc == 0
        for ue, r_, ce_ in zip(ues, res, ce):
            J = pkg.srs_M_sc(cfg, ue) // 8
            assert r_.nof_ce == J and np.abs(np.abs(ce_[:J]) - 1).max() <= 1e-4 and abs(r_.rsrp - 1) <= 1e-4
        outs.append((got, [bytes(r_) for r_ in res], [ce_[:r_.nof_ce].copy() for r_, ce_ in zip(res, ce)]))
    assert np.array_equal(outs[0][0].view(np.uint32), outs[1][0].view(np.uint32)) and outs[0][1] == outs[1][1]
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(outs[0][2], outs[1][2]))
    q.free()


def test_refusals_and_calls_on_one_stream():
    L = pkg.lib()
    for cfg in (pkg.srs_cfg(6, 1, 0, max_srs=2), pkg.srs_cfg(50, 1, 0, tdd=True, max_srs=2), pkg.srs_cfg(50, 1, 8, max_srs=2),
                pkg.srs_cfg(50, 1, 0, subframe_config=15, max_srs=2), pkg.srs_cfg(5, 1, 7, max_srs=2), pkg.srs_cfg(111, 1, 7, max_srs=2)):
        assert L.srslte_hip_srs_create(C.byref(cfg)) is None
    c = CASES["p50_bw0_B3_hop"]
    q = _srs(c, 2)
    grid = np.zeros((2, q.grid_len), np.complex64)
    dg = pkg.DevBuf.from_host(grid)
    dr, dc = pkg.DevBuf(C.sizeof(pkg.SrsRes) * 4), pkg.DevBuf(8 * pkg.SRS_MAX_CE * 4)
    for d in (dr, dc):
        L.srslte_hip_memset(d.ptr, 0x5A, d.nbytes)
    mk, ok = pkg.SrsUe.make, case_ue(c)
    for ue in (mk(0, B=4), mk(0, b_hop=4), mk(0, n_srs=8), mk(0, k_tc=2), mk(0, I_srs=637), mk(0, n_rrc=24), mk(2)):
        assert q.rx_device(dg.ptr, 0, 2, [ok, ue], dr.ptr, dc.ptr) == -2
        assert q.put_device(dg.ptr, 0, 2, [ok, ue]) == -2
    assert q.rx_device(dg.ptr, 0, 2, [ok, ok, ok], dr.ptr, dc.ptr) == -2 and q.put_device(dg.ptr, 0, 2, [ok, ok, ok]) == -2  # nof > max_srs
    pkg.sync()
    assert (dr.to_host(np.uint8) == 0x5A).all() and (dc.to_host(np.uint8) == 0x5A).all() and not dg.to_host(np.complex64).any()  # nothing was queued
    q.free()
    # two put calls and two receive calls on one stream, nothing read in between: the descriptors of the first must survive the second's
    rng = np.random.default_rng(31)
    q = _srs(c, 4)
    st = L.srslte_hip_stream_create()
    lists = [[case_ue(c, sf=0), mk(1, B=1, b_hop=0, n_srs=2, k_tc=0, n_rrc=9)], [mk(0, B=2, b_hop=3, n_srs=6, k_tc=1, n_rrc=20), case_ue(c, sf=1, cs_used=0x21)]]
    ttis = [c["ttis"][3], c["ttis"][7] - 1]
    bgs = [(rng.normal(size=(2, q.grid_len)) + 1j * rng.normal(size=(2, q.grid_len))).astype(np.complex64) for _ in range(2)]
    dgs = [pkg.DevBuf.from_host(b) for b in bgs]
    outs = [(pkg.DevBuf(C.sizeof(pkg.SrsRes) * 2), pkg.DevBuf(8 * pkg.SRS_MAX_CE * 2)) for _ in range(2)]
    for k in range(2):
        assert q.put_device(dgs[k].ptr, ttis[k], 2, lists[k], st) == 0
    for k in range(2):
        assert q.rx_device(dgs[k].ptr, ttis[k], 2, lists[k], outs[k][0].ptr, outs[k][1].ptr, st) == 0
    L.srslte_hip_stream_sync(st)
    for k in range(2):
        rc, one = q.put(bgs[k], ttis[k], lists[k])
        assert rc == 0 and np.array_equal(dgs[k].to_host(np.complex64).view(np.uint32), one.ravel().view(np.uint32))
        rc, res, ce = q.rx(one, ttis[k], lists[k])
        got, gce = pkg.Srs.read(outs[k][0], outs[k][1], 2)
        for a, b, ca, cb in zip(res, got, ce, gce):
            assert rc == 0 and bytes(a) == bytes(b) and np.array_equal(ca[:a.nof_ce].view(np.uint32), cb[:a.nof_ce].view(np.uint32))
            assert abs(a.rsrp - 1) < 1e-4  # the receiver reads what the transmitter put: |h_j| = 1
    L.srslte_hip_stream_destroy(st)
    q.free()
