"""UE CSI feedback on the device (srslte_hip_csi_batch, srslte_hip_dl_rx_csi_batch) against the reference's own functions run on the device's
own estimates and noise figures, copied back.

Bounds. One-layer SINRs, cn_db and the two-layer SINRs against the reference's _gen text: the project's scalar rule, 1e-4 relative for
linear values and 1e-3 absolute for dB. Two-layer SINRs against the reference's compiled dispatch (AVX, two _mm256_rcp_ps steps): twice the
distance between the reference's own two variants, _gen and the dispatch, measured on the test's inputs on the CPU - measured: 3.2e-4 relative
on the drawn cases and 4.4e-4 on the estimator's own estimates (low SNR, where 1 / den - 1 amplifies the approximation), so the bound is
6.4e-4 / 8.8e-4; the test computes it from its inputs every time, per group of cases. The device measured 4.4e-4 against the dispatch. Decisions (pmi_1l, pmi_2l, ri_cn, ri, pmi, cqi_sinr, cqi_wideband) equal those of the dispatching
reference; a case may be set aside only where the reference's own margin lies inside that bound (_margin_inside below), at most 2 % of the cases."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest

import csi_ref as R
from _libs import ref

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(ref() is None, reason="oracle/_ref/libsrslte_ref.so is not built")]
REL, DB = 1e-4, 1e-3
GROUPS = [(prb, cp) for prb in (6, 25, 50, 100) for cp in (True, False)]
DRAWS = [(cond, snr, rep) for cond in ("well", "ill") for snr in (-5, 5, 15, 25, 35) for rep in range(3)]


@pytest.fixture(scope="module")
def hp():
    return importlib.import_module("srslte-emane_amd")


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - b) / np.abs(b)))


def _draw(prb, cp):
    rng = np.random.default_rng(4100 + prb + (0 if cp else 1))
    ces, noises, snrs = [], [], []
    for cond, snr, rep in DRAWS:
        ce = R.draw_ce(rng, prb, cp, cond)
        ces.append(ce)
        noises.append(np.float32(np.mean(np.abs(ce) ** 2) * 2 * 10 ** (-snr / 10)))
        snrs.append(np.float32(snr + rng.uniform(-0.5, 0.5)))
    return np.stack(ces), np.array(noises, np.float32), np.array(snrs, np.float32)


def _margin_inside(r, bound):
    """True where a decision of the reference hangs on less than the two-layer SINR bound (or, for cn, the dB rule)."""
    db = 10 * math.log10(1 + bound) + DB
    s1 = np.sort(np.asarray(r["d1"][1], np.float64))[::-1]
    s2 = np.sort(np.asarray(r["d2"][1], np.float64))[::-1]
    if s1[0] - s1[1] <= bound * s1[0] or s2[0] - s2[1] <= bound * s2[0]:
        return True
    db1, db2 = 10 * math.log10(s1[0]), 10 * math.log10(s2[0])
    if abs(db2 - db1 - 0.1) <= 2 * db or abs(db2 - 20.0) <= db or abs(float(r["cn"]) - 17.0) <= DB:
        return True
    return any(abs(v + r["offset"] - float(t)) <= db for v in (db1, db2) for t in R.CQI_TO_SNR)


def _check_group(recs, ces, noises, snrs, prb, cp, offset, stats):
    N = ces.shape[-1]
    cut = 96 * (N // 96)
    refs = []
    for b in range(len(recs)):
        r = R.Ref(ref(), ces[b], noises[b], prb, cp)
        refs.append(dict(g1=r.gen(1, cut), g2=r.gen(2, cut), d1=r.dispatch(1, N), d2=r.dispatch(2, N), cn=r.cn(), sel=r.select_ri_pmi(), offset=offset))
    dist = max(_rel(x["d2"][1], x["g2"][1]) for x in refs)  # the reference's two variants against each other, on these inputs
    bound = 2 * dist
    stats["dist"] = max(stats.get("dist", 0.0), dist)
    for b, (o, x) in enumerate(zip(recs, refs)):
        where = (prb, cp, DRAWS[b] if len(recs) == len(DRAWS) else b)
        e1, e2, ec = _rel(list(o.sinr_1l), x["g1"][1]), _rel(list(o.sinr_2l), x["g2"][1]), abs(o.cn_db - float(x["cn"]))
        ea = _rel(list(o.sinr_2l), x["d2"][1])
        stats["e"] = [max(a, c) for a, c in zip(stats.get("e", [0, 0, 0, 0]), (e1, e2, ec, ea))]
        assert e1 <= REL and e2 <= REL and ec <= DB, (where, e1, e2, ec)
        assert ea <= bound, (where, ea, bound)
        ri, pmi, sinr_db = x["sel"]
        want = (x["d1"][0], x["d2"][0], 1 if x["cn"] < np.float32(17.0) else 0, ri, pmi, R.cqi_from_snr(np.float32(sinr_db) + np.float32(offset)),
                R.cqi_from_snr(np.float32(snrs[b]) + np.float32(offset)))
        got = (o.pmi_1l, o.pmi_2l, o.ri_cn, o.ri, o.pmi, o.cqi_sinr, o.cqi_wideband)
        stats["n"] = stats.get("n", 0) + 1
        if got != want and _margin_inside(x, bound):
            stats["aside"] = stats.get("aside", 0) + 1
            continue
        assert got == want, (where, got, want)
        assert abs(o.sinr_db - float(sinr_db)) <= 10 * math.log10(1 + bound) + DB and o.reserved == 0, where


def test_csi_batch_parity_and_decisions_on_drawn_estimates(hp):
    stats = {}
    for prb, cp in GROUPS:
        ces, noises, snrs = _draw(prb, cp)
        offset = 0.0 if prb != 25 else 1.5
        q = hp.Csi(prb, 2, 2, cp)
        assert q.set_snr_to_cqi_offset(offset) == 0
        rc, recs = q.batch(ces, noises, snrs)
        assert rc == 0
        rc, again = q.batch(ces, noises, snrs)  # the fixed-order reduction: the same bits on every run
        assert rc == 0 and all(bytes(a) == bytes(b) for a, b in zip(recs, again))
        _check_group(recs, ces, noises, snrs, prb, cp, offset, stats)
        q.free()
    print("cases %d, set aside %d; _gen vs dispatch (two layers) %.3e; device: 1l %.2e 2l %.2e rel, cn %.2e dB vs _gen, 2l %.2e vs dispatch"
          % (stats["n"], stats.get("aside", 0), stats["dist"], *stats["e"]))
    assert stats.get("aside", 0) <= 0.02 * stats["n"], stats


def test_rank_rule_variants_on_drawn_estimates(hp):
    """No device call: this only establishes, on the NumPy restatement, that the cases the parity test above draws cover both outcomes of
    every rank rule - two layers chosen by the "> 20.0" clause alone and not at all, cn on either side of 17. The device's decisions on these
    cases are compared with the reference's in test_csi_batch_parity_and_decisions_on_drawn_estimates; the rules themselves are pinned
    exactly through the host entry of the kernel's decision function (tests/test_csi_host.py::test_decisions_of_the_deciding_lane)."""
    seen = set()
    for prb, cp in GROUPS[:4]:
        ces, noises, snrs = _draw(prb, cp)
        for b in range(len(ces)):
            m = R.measure(ces[b], noises[b], snrs[b])
            d1, d2 = 10 * math.log10(m["sinr_1l"][m["pmi_1l"]]), 10 * math.log10(m["sinr_2l"][m["pmi_2l"]])
            seen.add(("ri", m["ri"], d2 > d1 + 0.1, d2 > 20.0))
            seen.add(("cn", m["ri_cn"]))
    assert {("ri", 1, False, True), ("ri", 0, False, False), ("cn", 0), ("cn", 1)} <= seen, seen


@pytest.mark.parametrize("nof_ports,nof_rx", [(1, 1), (1, 2), (2, 1)])
def test_csi_batch_other_antenna_counts(hp, nof_ports, nof_rx):
    rng = np.random.default_rng(9)
    prb, N = 25, 14 * 12 * 25
    ce = (rng.standard_normal((3, nof_ports, nof_rx, N)) + 1j * rng.standard_normal((3, nof_ports, nof_rx, N))).astype(np.complex64)
    q = hp.Csi(prb, nof_ports, nof_rx)
    rc, recs = q.batch(ce, [0.1, 0.2, 0.3], [3.0, 12.0, 30.0])
    assert rc == 0
    for b, o in enumerate(recs):
        if nof_ports == 1:  # select_pmi does nothing on a single-port cell
            assert bytes(o) == bytes(64)
            continue
        full = np.zeros((2, 2, N), np.complex64)
        full[:, 0] = ce[b, :, 0]
        m = R.measure(full, [0.1, 0.2, 0.3][b], [3.0, 12.0, 30.0][b], nof_rx=1)
        assert _rel(list(o.sinr_1l), m["sinr_1l"]) <= REL and o.pmi_1l == m["pmi_1l"]
        assert (o.ri, o.pmi, o.ri_cn, o.cn_db, o.pmi_2l, list(o.sinr_2l)) == (0, m["pmi_1l"], 0, 0.0, 0, [0.0, 0.0])
        assert o.cqi_wideband == R.cqi_from_snr([3.0, 12.0, 30.0][b]) and abs(o.sinr_db - m["sinr_db"]) <= DB
    q.free()


def _chest(hp):
    hc = hp.ChestDlCfg()
    hc.filter_coef[0], hc.filter_coef[1] = 4.0, 1.0
    return hc


@pytest.mark.parametrize("prb,scheme,pmi,tbs,tbs2,snr", [(25, "mux", 1, 4008, 2216, 9.0), (25, None, 0, 4008, 0, 6.0), (100, "mux", 0, 30576, 30576, 18.0),
                                                         (6, "mux", 2, 328, 0, 3.0)])
def test_dl_rx_csi_batch_measures_the_pipelines_own_estimates(hp, prb, scheme, pmi, tbs, tbs2, snr):
    """After a TM4 batch and after a transmit-diversity batch: srslte_hip_dl_rx_csi_batch equals srslte_hip_csi_batch on the stage-2 buffers
    of the same call bit for bit, and both match the reference on those estimates (made by the estimator from lte_sim 2x2 signals)."""
    from lte_sim import DlConfig, make_subframe, make_subframe_mimo
    nsf, tti0, cid = 4, 3, 7
    mod = 2 if prb > 6 else 1
    cfg = DlConfig(prb, cid, mod, tbs, cfi=1, nof_rx=2, nof_ports=2, tx_scheme=scheme, pmi=pmi, mod2=mod if tbs2 else None, tbs2=tbs2)
    rng = np.random.default_rng(500 + prb)
    make = make_subframe_mimo if scheme else make_subframe
    iq = [make(cfg, tti0 + b, rng, snr_db=snr, amp=0.2)[0] for b in range(nsf)]
    rx = hp.DlRx(cid, prb, 1, 0x1234, mod, tbs, 6, nsf, True, _chest(hp), nof_rx=2, nof_ports=2, tx_scheme=2 if scheme else 0, pmi=pmi, mod2=mod if tbs2 else 0,
                 tbs2=tbs2)
    one = hp.DevBuf(64 * nsf)
    assert hp.lib().srslte_hip_dl_rx_csi_batch(rx.h, 1, one.ptr, None) == -2  # no batch has run
    rx.decode(np.stack(iq), tti0)
    rc, recs = rx.csi(nsf)
    assert rc == 0
    assert hp.lib().srslte_hip_dl_rx_csi_batch(rx.h, nsf + 1, one.ptr, None) == -2 and hp.lib().srslte_hip_dl_rx_csi_batch(rx.h, nsf, None, None) == -2
    assert hp.lib().srslte_hip_dl_rx_csi_batch(rx.h, 0, one.ptr, None) == -2
    L = hp.lib()
    q = hp.Csi(prb, 2, 2)
    dout = hp.DevBuf(64 * nsf)
    assert q.run_device(L.srslte_hip_dl_rx_debug_buffer(rx.h, 1), L.srslte_hip_dl_rx_debug_buffer(rx.h, 2), nsf, dout.ptr) == 0
    hp.sync()
    assert bytes(dout.to_host(np.uint8)) == b"".join(bytes(r) for r in recs)
    N = 14 * 12 * prb
    ces = rx.debug(1, np.complex64, nsf * 4 * N).reshape(nsf, 2, 2, N)
    res = rx.debug(2, np.float32, nsf * 10).reshape(nsf, 10)
    stats = {}
    _check_group(recs, ces, res[:, 0], res[:, 2], prb, True, 0.0, stats)
    assert stats.get("aside", 0) == 0, stats
    # a shorter measurement of the same batch, and an offset
    rc, part = rx.csi(2, snr_to_cqi_offset=2.0)
    assert rc == 0 and [list(p.sinr_1l) for p in part] == [list(r.sinr_1l) for r in recs[:2]]
    assert [p.cqi_wideband for p in part] == [R.cqi_from_snr(np.float32(res[b, 2]) + np.float32(2.0)) for b in range(2)]
    q.free()
    rx.free()


def test_refusals_queue_nothing(hp):
    L = hp.lib()
    assert L.srslte_hip_csi_create(25, 4, 2, 1) is None
    q = hp.Csi(25)
    d = hp.DevBuf(64)
    before = d.to_host(np.uint8).copy()
    for a in ((None, d.ptr, d.ptr, 1, d.ptr), (q.h, None, d.ptr, 1, d.ptr), (q.h, d.ptr, None, 1, d.ptr), (q.h, d.ptr, d.ptr, 1, None)):
        assert L.srslte_hip_csi_batch(*a, None) == -2
    hp.sync()
    assert np.array_equal(d.to_host(np.uint8), before)
    rx4 = hp.DlRx(7, 25, 1, 0x1234, 2, 4008, 6, 2, True, _chest(hp), nof_rx=2, nof_ports=4)
    from lte_sim import DlConfig, make_subframe
    cfg = DlConfig(25, 7, 2, 4008, nof_rx=2, nof_ports=4)
    rng = np.random.default_rng(1)
    rx4.decode(np.stack([make_subframe(cfg, b, rng, snr_db=10.0)[0] for b in range(2)]), 0)
    assert L.srslte_hip_dl_rx_csi_batch(rx4.h, 2, d.ptr, None) == -2  # 4 ports
    hp.sync()
    assert np.array_equal(d.to_host(np.uint8), before)
    rx4.free()
    q.free()


def _tm4_iq(cfg, tti, rng, H, snr_db, amp=0.2):
    """One TM4 subframe of lte_sim (coding, precoding with cfg.pmi, RE mapping, CRS) over the flat 2x2 channel H[antenna][port] with one delay per
    antenna, so that the phase between the two ports - what the codebook entry has to match - is the same on every subcarrier.
    Returns (iq [2][sf_len], [payload])."""
    from lte_sim import OrcOfdm, make_subframe_mimo, oracle
    from _libs import p
    orc = oracle()
    k = {}
    _, data = make_subframe_mimo(cfg, tti, rng, snr_db=None, amp=amp, keep=k)
    sf_idx = tti % 10
    tx = []
    for port in range(2):
        g = np.zeros(cfg.grid_len, np.complex64)
        g[k["idx"]] = k["y"][port]
        orc.orc_crs_put_sf(C.byref(cfg.cell), sf_idx, port, p(g))
        tx.append(g)
    q = OrcOfdm()
    orc.orc_ofdm_init(C.byref(q), cfg.nof_prb, cfg.cp_norm)
    q.normalize = True
    kk = (np.arange(cfg.grid_len) % cfg.nre) - cfg.nre / 2
    sigma = np.sqrt(amp * amp * cfg.nre / cfg.N / 2) * 10 ** (-snr_db / 20)
    out = []
    for a in range(2):
        rxg = (tx[0] * H[a][0] + tx[1] * H[a][1]) * np.exp(-2j * np.pi * kk * (0.6 + 0.5 * a) / cfg.N)
        rxg = np.ascontiguousarray(rxg.astype(np.complex64))
        iq = np.zeros(cfg.sf_len, np.complex64)
        orc.orc_ofdm_tx_sf(C.byref(q), p(rxg), p(iq))
        iq = iq * np.float32(amp) + (sigma * (rng.standard_normal(cfg.sf_len) + 1j * rng.standard_normal(cfg.sf_len))).astype(np.complex64)
        out.append(iq.astype(np.complex64))
    return np.stack(out), data


def _ref_unpack(cqi_cfg, bits):
    """srslte_cqi_value_unpack of the reference on a received bit row -> RefCqiValue"""
    rc = R.RefCqiCfg(bool(cqi_cfg.data_enable), False, bool(cqi_cfg.pmi_present), bool(cqi_cfg.four_antenna_ports), bool(cqi_cfg.rank_is_not_one),
                     bool(cqi_cfg.subband_label_2_bits), cqi_cfg.L, cqi_cfg.N, cqi_cfg.type, 0)
    buf = np.zeros(128, np.uint8)
    buf[:len(bits)] = bits
    v = R.RefCqiValue()
    n = ref().srslte_cqi_value_unpack(C.byref(rc), buf.ctypes.data_as(C.c_void_p), C.byref(v))
    return n, v


@pytest.mark.parametrize("prb,mod,tbs", [(25, 2, 4008), (100, 3, 30576)])
def test_closed_loop_pmi_and_ri_through_pusch_and_pucch(hp, prb, mod, tbs):
    """TM4 downlink over a fixed 2x2 channel whose two ports arrive theta apart on both antennas (plus a tenth of a second path, so rank one
    is 20 dB ahead): the precoder [1, e^(j theta)] / sqrt(2) adds them up - entry 0 for theta = 0, entry 2 for pi / 2 - and the opposite entry
    cancels them. The UE pipeline decodes a batch sent with the OPPOSITE entry (blocks fail) and measures; the host helpers make the aperiodic
    mode 31 report and the periodic wideband + PMI report; they travel through srslte_hip_ul_tx_batch_uci_cqi -> the eNB PUSCH receiver and
    through PUCCH format 2 -> srslte_hip_ul_ctrl_pucch_batch, are unpacked by the reference's srslte_cqi_value_unpack, and the next downlink
    batch, sent with the reported PMI and RI, decodes with every block passing. Rotating theta moves the reported entry to the one the
    reference picks on the same estimates."""
    from lte_sim import DlConfig
    cid, rnti, nsf, tti0, snr = 7, 0x1234, 2, 4, 12.0
    N = 14 * 12 * prb
    for theta, expect in ((0.0, 0), (np.pi / 2, 2)):
        rng = np.random.default_rng(900 + prb + expect)
        H = np.outer([1.0, 0.8 * np.exp(0.9j)], [1.0, np.exp(-1j * theta)]) + 0.1 * np.array([[0.6 * np.exp(2.0j), -0.7], [0.5j, 0.8 * np.exp(-1.1j)]])
        wrong = {0: 1, 2: 3}[expect]
        cfg0 = DlConfig(prb, cid, mod, tbs, cfi=1, nof_rx=2, nof_ports=2, tx_scheme="mux", pmi=wrong, tbs2=0)
        iq0 = [_tm4_iq(cfg0, tti0 + b, rng, H, snr)[0] for b in range(nsf)]
        rx0 = hp.DlRx(cid, prb, 1, rnti, mod, tbs, 6, nsf, True, _chest(hp), nof_rx=2, nof_ports=2, tx_scheme=2, pmi=wrong)
        _, ok0 = rx0.decode(np.stack(iq0), tti0)
        assert not ok0.any(), "the cancelling precoder should not decode"
        rc, recs = rx0.csi(nsf)
        assert rc == 0
        ces = rx0.debug(1, np.complex64, nsf * 4 * N).reshape(nsf, 2, 2, N)
        res = rx0.debug(2, np.float32, nsf * 10).reshape(nsf, 10)
        rx0.free()
        for b in range(nsf):  # the entry the reference picks on the same estimates
            r = R.Ref(ref(), ces[b], res[b, 0], prb)
            ri_ref, pmi_ref, _ = r.select_ri_pmi()
            assert (recs[b].ri, recs[b].pmi) == (ri_ref, pmi_ref) == (0, expect), (theta, b, recs[b].ri, recs[b].pmi, ri_ref, pmi_ref)
        # aperiodic mode 31 on the PUSCH
        rep = hp.CsiReportCfg(4, prb, 2, 2, 0, 1, 0, 0, 0, 0, 31, 0.0, 1)
        outs = []
        for b in range(nsf):
            rc, out = hp.csi_gen_cqi_aperiodic(recs[b], rep, recs[b].cqi_wideband)
            assert rc == 0 and out.ri_len == 1 and out.ri == 0 and rep.last_ri == 0
            outs.append(out)
        clen = outs[0].cqi_len
        assert clen == 4 + 2 * hp.cqi_hl_get_no_subbands(prb) + 2 and all(o.cqi_len == clen for o in outs)
        L_prb, n_prb, ul_tbs = 12, 2, 1000
        kw = dict(ri_len=1, I_offset_ri=6, cqi_len=clen, I_offset_cqi=6)
        utx = hp.UlTx(cid, prb, rnti, 1, ul_tbs, L_prb, n_prb, 3, nsf, **kw)
        urx = hp.UlRx(cid, prb, rnti, 1, ul_tbs, L_prb, n_prb, 3, 6, nsf, **kw)
        ul_data = rng.integers(0, 256, (nsf, ul_tbs // 8), dtype=np.uint8)
        bits = np.array([list(o.cqi_bits[:clen]) for o in outs], np.uint8)
        ul_iq = utx.encode(ul_data, tti0 + 4, ri=np.array([[o.ri] for o in outs], np.uint8), cqi=bits)
        ul_tb, ul_ok = urx.decode(ul_iq, tti0 + 4)
        got_bits, got_crc = urx.cqi()
        assert ul_ok.all() and np.array_equal(ul_tb[:, :ul_tbs // 8], ul_data) and got_crc.all() and np.array_equal(got_bits, bits)
        assert np.array_equal(urx.ri()[:, 0], [o.ri for o in outs])
        utx.free()
        urx.free()
        reported = []
        for b in range(nsf):
            n, v = _ref_unpack(outs[b].cqi, got_bits[b])
            assert n == clen and v.subband_hl.pmi == expect and v.subband_hl.wideband_cqi_cw0 == outs[b].value.wideband_cqi == recs[b].cqi_sinr
            assert v.subband_hl.subband_diff_cqi_cw0 == 0
            reported.append(int(v.subband_hl.pmi))
        # periodic wideband + PMI on PUCCH format 2: I_cqi_pmi 0 reports in even TTIs
        per = hp.CsiReportCfg(4, prb, 2, 2, 0, 1, 0, 0, 0, 0, 31, 0.0, rep.last_ri)
        txs, reqs, pouts = [], [], []
        for b in range(nsf):
            rc, out = hp.csi_gen_cqi_periodic(recs[b], per, recs[b].cqi_wideband, tti0 + b)
            assert rc == 0 and out.cqi_len == (6 if (tti0 + b) % 2 == 0 else 0)
            if out.cqi_len:
                req = hp.PucchReq.make(b, rnti, cqi_len=out.cqi_len, n_pucch_2=3, noise_estimate=0.1)
                reqs.append(req), txs.append(hp.PucchTx.make(req, cqi=list(out.cqi_bits[:out.cqi_len]))), pouts.append((b, out))
        assert len(reqs) == 1
        ptx, prx = hp.UlCtrlTx(prb, cid, max_pucch=nsf), hp.UlCtrl(prb, cid, max_pucch=nsf)
        rc, grid = ptx.put(np.zeros((nsf, N), np.complex64), tti0, txs)
        assert rc == 0
        rc, pres = prx.batch(grid, tti0, reqs)
        assert rc == 0
        for (b, out), pr in zip(pouts, pres):
            assert pr.detected and list(pr.cqi[:6]) == list(out.cqi_bits[:6])
            n, v = _ref_unpack(out.cqi, list(pr.cqi[:6]))
            # srslte_cqi_value_unpack reads all six bits of a wideband + PMI report and returns 4 whatever it read (cqi.c:207)
            assert n == 4 and v.wideband.pmi == expect == recs[b].pmi_1l and v.wideband.wideband_cqi == recs[b].cqi_wideband
        ptx.free()
        prx.free()
        # the next downlink batch with what the eNB read: RI 0 -> one layer, the reported entry
        assert reported == [expect] * nsf
        cfg1 = DlConfig(prb, cid, mod, tbs, cfi=1, nof_rx=2, nof_ports=2, tx_scheme="mux", pmi=reported[0], tbs2=0)
        sent = [_tm4_iq(cfg1, tti0 + 8 + b, rng, H, snr) for b in range(nsf)]
        rx1 = hp.DlRx(cid, prb, 1, rnti, mod, tbs, 6, nsf, True, _chest(hp), nof_rx=2, nof_ports=2, tx_scheme=2, pmi=reported[0])
        tb1, ok1 = rx1.decode(np.stack([s[0] for s in sent]), tti0 + 8)
        assert ok1.all(), (theta, ok1)
        for b in range(nsf):
            assert np.array_equal(tb1[b][:tbs // 8], sent[b][1][0])
        rx1.free()
