"""The SRS on the device (srslte_hip_srs_tx_put, srslte_hip_srs_rx_batch, srslte_hip_ul_rx_batch_grants_pucch_srs): transmitted grids against
tests/golden/srs.npz (recorded from the reference's refsignal_ul.c), the sounding receiver against its float64 model of tests/srs_ref.py on
random grids, an end-to-end scene of five UEs with gains, delays and noise, the grants pipeline with a PUSCH, a PUCCH and two SRS in one
shortened subframe, refusals, and calls queued on one stream."""
import ctypes as C
import importlib

import numpy as np
import pytest

from gen_golden_srs import CASES
from srs_ref import E2E, case_cfg, case_ue, e2e_channel, e2e_truth, golden, rx_model

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


def _check_against_model(res, ce, m):
    J = m["ce"].size
    assert res.nof_ce == J
    assert np.abs(ce[:J] - m["ce"]).max() <= 1e-5
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
    slack = 1e-5 * float(np.sum(a[1:] + a[:-1])) / abs(m["corr"]) + 1e-6
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


def test_refusals_and_calls_on_one_stream():
    L = pkg._bind_srs(pkg.lib())
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
