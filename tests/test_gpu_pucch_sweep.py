"""PUCCH on the device over every resource index: srslte_hip_ul_ctrl_tx_put_pucch and srslte_hip_ul_ctrl_pucch_batch at every in-band n_pucch of the
five sweep cells of tests/gen_golden_pucch.py (n_oc 2, every PRB pair to the innermost, both sides of c N_cs / delta and of 12 n_rb_2, the band
edge), against RefUlCtrl (pinned to the reference's own pucch.c by tests/test_pucch_golden.py) and against the recorded grids themselves; a full
RB of UEs in one subframe; the format-2 RNTI range; and the fused grants pipeline with PUCCHs at n_oc 2 beside a PUSCH. One device call per
(cell, family, case), never one per index."""
import collections
import ctypes as C

import numpy as np
import pytest

from _libs import ref
from pucch_sweep import (NAMES, SWEEP_CELLS, SWEEP_SNRS, al, cfg_of, golden, kw, last_in_band, pkg, rec_grid, rec_tx, ref_of, sweep_scene, threshold)
from test_gpu_ul_ctrl import KINDS, _compare
from ul_ctrl_ref import F1, F1A, F1B, F2, F2A, F2B, RefUlCtrl

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(ref() is None, reason="oracle/_ref/libsrslte_ref.so is not built")]
INVALID = -2  # SRSLTE_ERROR_INVALID_INPUTS
assert len(KINDS) == 7  # pucch_sweep.F1_KINDS / F2_KINDS split these seven (cqi_ack with and without simul_cqi_ack)


def _tx_of(rng, spec, family, n, shortened, k):
    """The k-th variant of a family on n_pucch = n in subframe n: 1, 1a and 1b with every ACK value; 2, 2a / 2b with drawn reports and RIs."""
    mk, N1 = pkg.PucchReq.make, spec[7]
    if family == 1:
        fmt, ack = [(F1, (0, 0)), (F1A, (0, 0)), (F1A, (1, 0)), (F1B, (0, 0)), (F1B, (0, 1)), (F1B, (1, 0)), (F1B, (1, 1))][k % 7]
        if fmt == F1:
            return fmt, pkg.PucchTx.make(mk(n, 0x46 + n, sr_tti=True, n_pucch_sr=n, shortened=shortened), sr=1)
        return fmt, pkg.PucchTx.make(mk(n, 0x46 + n, ack_len=fmt, ncce=n - N1, shortened=shortened), ack=ack)
    ack_len, use_ri = [(0, False), (1, False), (2, False), (0, True), (2, True), (1, True)][k % 6]
    ack = (int(rng.integers(0, 2)), int(rng.integers(0, 2)))
    ln = int(rng.integers(1, 13))
    q = mk(n, 0x46 + n, ack_len=ack_len, cqi_len=0 if use_ri else ln, ri_len=1 if use_ri else 0, n_pucch_2=n, simul_cqi_ack=True, shortened=shortened)
    fmt = F2 if ack_len == 0 else (F2B if ack_len == 2 or spec[2] else F2A)
    return fmt, pkg.PucchTx.make(q, ack=ack, ri=int(rng.integers(0, 2)), cqi=[int(b) for b in rng.integers(0, 2, ln)])


@pytest.mark.parametrize("name", NAMES)
def test_put_pucch_at_every_index(name):
    """One put_pucch call per (family, shortened) writes every in-band index, one PUCCH per subframe, into a random background: within 1e-5 of
    RefUlCtrl.encode, every other RE bit-identical."""
    spec = SWEEP_CELLS[name]
    R = ref_of(spec)
    rng = np.random.default_rng(4000 + NAMES.index(name))
    seen = set()
    for family in (1, 2):
        nof = last_in_band(spec, family) + 1
        tx = pkg.UlCtrlTx(spec[0], spec[1], max_pucch=nof, **kw(spec))
        for shortened in (False, True):
            tti0 = int(rng.integers(0, 10240))
            bg = (rng.normal(size=(nof, R.glen)) + 1j * rng.normal(size=(nof, R.glen))).astype(np.complex64)
            want, txs = bg.copy(), []
            for n in range(nof):
                fmt, t = _tx_of(rng, spec, family, n, shortened, n + n // 7)
                g = al(want[n])
                assert R.encode(g, tti0 + n, t) == fmt
                want[n] = g
                txs.append(t)
                seen.add(fmt)
            rc, got = tx.put(bg, tti0, txs)
            assert rc == 0
            err = np.abs(got - want).max(axis=1)
            assert err.max() < 1e-5, (family, shortened, int(err.argmax()), float(err.max()))
            touched = want.view(np.uint64) != bg.view(np.uint64)
            assert touched.sum(axis=1).min() >= 84 + 24
            assert np.array_equal(got.view(np.uint64)[~touched], bg.view(np.uint64)[~touched]), (family, shortened)
        tx.free()
    assert seen == ({F1, F1A, F1B, F2, F2B} if spec[2] else {F1, F1A, F1B, F2, F2A, F2B})


@pytest.mark.parametrize("name", NAMES)
def test_put_pucch_matches_recorded_grids(name):
    """The full-signal records through one put_pucch call on zeroed grids: the REs of srslte_pucch_encode + srslte_refsignal_dmrs_pucch_put and
    no others, values within 1e-5 of the reference's own."""
    g, spec = golden(), SWEEP_CELLS[name]
    meta = g[name + ".rec_meta"]
    glen = (12 if spec[2] else 14) * 12 * spec[0]
    tx = pkg.UlCtrlTx(spec[0], spec[1], max_pucch=len(meta), **kw(spec))
    # subframe k of a call is TTI tti0 + k and the signal depends on the TTI through tti % 10 alone: record i goes to a subframe of its own
    # with that residue, so one call writes them all
    sfs, txs = [], []
    for i, m in enumerate(meta):
        sf = int(m[2]) % 10
        while sf in sfs:
            sf += 10
        sfs.append(sf)
        txs.append(rec_tx(spec, m, g[name + ".rec_uci"][i], sf=sf))
    rc, got = tx.put(np.zeros((max(sfs) + 1, glen), np.complex64), 0, txs)
    assert rc == 0
    for i, sf in enumerate(sfs):
        want, idx = rec_grid(g, name, i, glen)
        assert np.array_equal(np.flatnonzero(got[sf]), idx), i
        assert np.abs(got[sf] - want).max() < 1e-5, (i, int(meta[i][0]), int(meta[i][1]))
    assert not np.delete(got, sfs, axis=0).any()
    tx.free()


@pytest.mark.parametrize("name", NAMES)
def test_receive_at_every_index(name):
    """Every in-band index of both families, one UE per subframe, the seven request kinds cycled (the SR retry on a high HARQ-ACK resource
    among them), at 30 dB and 0 dB: every decision and the correlation equal RefUlCtrl.decode's. Decisions the reference itself takes within 1e-4
    of a threshold or a tie are set aside (at most 1 % by tests/test_pucch_golden.py), as are format-2 LLRs one step apart: 2 % in all."""
    spec = SWEEP_CELLS[name]
    total, excl, R = 0, collections.Counter(), None
    for family in (1, 2):
        rx = pkg.UlCtrl(spec[0], spec[1], max_pucch=last_in_band(spec, family) + 1, **kw(spec))
        for snr in SWEEP_SNRS:
            R, reqs, grid, tti0 = sweep_scene(name, family, snr, R)
            rc, got = rx.batch(grid, tti0, reqs)
            assert rc == 0
            _compare(R, grid, tti0, reqs, got, rx.debug(1, len(reqs)), rx.debug(0, len(reqs)), excl)
            if family == 1:  # an SR TTI whose SR resource stayed empty: the retry found the UE on the swept HARQ-ACK resource, high ones included
                retried = [g.n_pucch for q, g in zip(reqs, got) if q.sr_tti and q.ack_len and q.ncce + spec[7] == q.sf and not g.sr and g.n_pucch == q.sf]
                assert retried and max(retried) > last_in_band(spec, 1) - 40
            else:
                assert all(g.n_pucch == q.sf for q, g in zip(reqs, got))
            total += len(reqs)
        rx.free()
    print("%s: %d requests, set aside %s" % (name, total, dict(excl)))
    assert total == 2 * (last_in_band(spec, 1) + last_in_band(spec, 2) + 2)
    assert sum(excl.values()) <= total // 50 and excl["llr"] <= 2, (total, dict(excl))


def full_rb_scene(name):
    """Every resource of one format-1 PRB pair active in the same subframe, with drawn ACK bits (1b and 1a alternating): at the first m past
    the mixed RB, the next one (the slots' PRBs swapped) and the innermost in-band m, each noise-free and at 10 dB -> R, reqs, txs, grid, the RB's
    resources and the thresholds."""
    spec = SWEEP_CELLS[name]
    P, _, ext, _, D, Ncs, nrb2, N1 = spec
    per, m0 = (2 if ext else 3) * 12 // D, nrb2 + (Ncs + 7) // 8
    # K UEs of equal power on one RB: a UE's share of the received energy is 1 / K, its normalised correlation about 1 / sqrt(K) at best.
    # Half of that is the detection threshold here; under the 0.8 of the other tests the reference finds nobody in a full RB
    th = dict(threshold_format1=0.5 / np.sqrt(per), threshold_data_valid_format1a=0.5 / np.sqrt(per))
    R = RefUlCtrl(cfg_of(spec, **th))
    rng = np.random.default_rng(9000 + NAMES.index(name))
    cases = [(m, snr) for m in (m0, m0 + 1, 2 * P - 1) for snr in (None, 10.0)]
    reqs, txs, grid = [], [], np.zeros((len(cases), R.glen), np.complex64)
    for sf, (m, snr) in enumerate(cases):
        base = threshold(spec) + (m - m0) * per
        noise = 0.0 if snr is None else 10 ** (-snr / 10)
        for j in range(per):
            q = pkg.PucchReq.make(sf, 0x100 + j, ack_len=2 - j % 2, ncce=base + j - N1, noise_estimate=noise)
            t = pkg.PucchTx.make(q, ack=(int(rng.integers(0, 2)), int(rng.integers(0, 2))))
            g = al(np.zeros(R.glen, np.complex64))
            R.encode(g, 700 + sf, t)
            grid[sf] += g
            reqs.append(q)
            txs.append(t)
        if snr is not None:
            grid[sf] += (rng.normal(0, np.sqrt(noise / 2), R.glen) + 1j * rng.normal(0, np.sqrt(noise / 2), R.glen)).astype(np.complex64)
    return R, reqs, txs, grid, per, th


@pytest.mark.parametrize("name", ["S1", "S2", "S4"])
def test_receive_a_full_rb(name):
    """36, 18 and 24 UEs on one PRB pair: every request equals RefUlCtrl.decode on the same grid (the reference's decisions, not the bits sent:
    its 3-tap filter does not separate cyclic shifts), and in the noise-free subframes every n_oc class has a UE found with its bits."""
    spec = SWEEP_CELLS[name]
    R, reqs, txs, grid, per, th = full_rb_scene(name)
    assert per == {"S1": 36, "S2": 18, "S4": 24}[name] and len(reqs) == 6 * per
    rx = pkg.UlCtrl(spec[0], spec[1], max_pucch=len(reqs), **kw(spec, **th))
    rc, got = rx.batch(grid, 700, reqs)
    assert rc == 0
    excl = collections.Counter()
    _compare(R, grid, 700, reqs, got, rx.debug(1, len(reqs)), rx.debug(0, len(reqs)), excl)
    rx.free()
    assert sum(excl.values()) <= len(reqs) // 50, dict(excl)
    n_oc = golden()[name + ".f1_state"][:, 0, 0, 0, 1]
    found = collections.Counter()
    for q, t, g in zip(reqs, txs, got):
        if q.noise_estimate == 0.0 and g.detected and list(g.ack)[:q.ack_len] == list(t.ack)[:q.ack_len]:
            found[int(n_oc[g.n_pucch])] += 1
    assert set(found) == ({0, 1} if spec[2] else {0, 1, 2}), dict(found)


@pytest.mark.parametrize("name", NAMES)
def test_band_edge(name):
    """The last in-band index of each family is accepted by put_pucch and pucch_batch; the first one out of band is refused with
    SRSLTE_ERROR_INVALID_INPUTS before anything is written, as is an SR TTI request whose HARQ-ACK retry resource is out of band."""
    spec = SWEEP_CELLS[name]
    mk, N1 = pkg.PucchReq.make, spec[7]
    tx = pkg.UlCtrlTx(spec[0], spec[1], max_pucch=2, **kw(spec))
    rx = pkg.UlCtrl(spec[0], spec[1], max_pucch=2, **kw(spec))
    rng = np.random.default_rng(11)
    bg = (rng.normal(size=(1, rx.grid_len)) + 1j * rng.normal(size=(1, rx.grid_len))).astype(np.complex64)
    dres = pkg.DevBuf(C.sizeof(pkg.PucchRes) * 2)
    for family in (1, 2):
        last = last_in_band(spec, family)
        assert golden()["%s.f%d_prb" % (name, family)].shape[0] == last + 2  # the reference's own band edge
        req = (lambda n, **a: mk(0, 0x46, ack_len=1, ncce=n - N1, **a)) if family == 1 else (lambda n, **a: mk(0, 0x46, cqi_len=4, n_pucch_2=n, **a))
        good, bad = req(last), req(last + 1)
        rc, got = tx.put(bg, 0, [pkg.PucchTx.make(good, ack=(1, 0), cqi=[1, 0, 1, 1])])
        # 1a and 2 with their DMRS fill their PRB in every symbol of the subframe
        assert rc == 0 and np.count_nonzero(got.view(np.uint64) != bg.view(np.uint64)) == (12 if spec[2] else 14) * 12
        rc, got = tx.put(bg, 0, [pkg.PucchTx.make(good, ack=(1, 0), cqi=[1, 0, 1, 1]), pkg.PucchTx.make(bad, ack=(1, 0), cqi=[1, 0, 1, 1])])
        assert rc == INVALID and np.array_equal(got.view(np.uint64), bg.view(np.uint64))
        dg = pkg.DevBuf.from_host(bg)
        pkg.lib().srslte_hip_memset(dres.ptr, 0x5A, dres.nbytes)
        assert rx.run_device(dg.ptr, 0, 1, [good, bad], dres.ptr) == INVALID
        if family == 1:  # the SR resource in band, the HARQ-ACK resource of the retry not; and the other way round
            assert rx.run_device(dg.ptr, 0, 1, [mk(0, 0x46, ack_len=1, ncce=last + 1 - N1, sr_tti=True, n_pucch_sr=last)], dres.ptr) == INVALID
            assert rx.run_device(dg.ptr, 0, 1, [mk(0, 0x46, ack_len=1, ncce=last - N1, sr_tti=True, n_pucch_sr=last + 1)], dres.ptr) == INVALID
        pkg.sync()
        assert (dres.to_host(np.uint8) == 0x5A).all()
        rc, res = rx.batch(got, 0, [good, req(last, sr_tti=True, n_pucch_sr=last) if family == 1 else good])
        assert rc == 0 and [r.n_pucch for r in res] == [last, last]
    tx.free()
    rx.free()


def test_format2_rnti_range():
    """The C-RNTI range of get_user_sequence (pucch.c:214-236): 0x000B and 0xFFF2 are served, and with cell 503 and subframe 9 beside 0xFFF2 the
    scrambling word comes from a c_init with its high bits set: the transmitted QPSK quadrants are the reference's own, and the recorded grids
    decode to the reference's own bits. 0x000A and 0xFFF3 are refused on both sides."""
    name, g = "S1", golden()
    spec = SWEEP_CELLS[name]
    meta = g[name + ".rec_meta"]
    rows = {int(m[4]): i for i, m in enumerate(meta) if int(m[0]) >= F2 and int(m[4]) in (0x000B, 0xFFF2)}
    assert set(rows) == {0x000B, 0xFFF2} and int(meta[rows[0xFFF2]][2]) % 10 == 9 and spec[1] == 503
    R = ref_of(spec)
    tx = pkg.UlCtrlTx(spec[0], spec[1], max_pucch=1, **kw(spec))
    rx = pkg.UlCtrl(spec[0], spec[1], max_pucch=1, **kw(spec))
    for rnti, i in sorted(rows.items()):
        tti = int(meta[i][2])
        t = rec_tx(spec, meta[i], g[name + ".rec_uci"][i])
        want, idx = rec_grid(g, name, i, R.glen)
        rc, got = tx.put(np.zeros((1, R.glen), np.complex64), tti, [t])
        assert rc == 0 and np.abs(got[0] - want).max() < 1e-5, hex(rnti)
        data = g[name + ".enc_idx"][i, :120]
        ph = got[0][data] / want[data]  # d(i) of both sides is one of four quadrants: the same bits leave a phase error, other bits a quadrant's
        assert np.abs(ph - 1).max() < 1e-4, hex(rnti)
        q = t.req
        q.noise_estimate = 0.0
        # the recorded grid itself. A clean QPSK symbol's LLR is 100.0 before the truncation to int16, so where the reference has 100 an
        # ulp in the equaliser or in sincosf leaves 99: every LLR within one step of the reference's (a wrong scrambling bit is 200 away), the
        # correlation within 20 steps of 1 / 2000, and every decision and bit the reference's own
        rc, res = rx.batch(want[None], tti, [q])
        assert rc == 0
        ref_dec, dec, r = R.decode(al(want), tti, q), g[name + ".dec"][i], res[0]
        assert np.abs(rx.debug(1, 1)[0].astype(int) - ref_dec["llr"].astype(int)).max() <= 1, hex(rnti)
        assert abs(r.correlation - float(g[name + ".dec_corr"][i])) <= 20 / 2000 + 1e-6, (hex(rnti), r.correlation)
        assert (r.format, r.n_pucch, r.detected, list(r.ack), r.ack_valid, r.cqi_crc) == \
               (int(meta[i][0]), int(meta[i][1]), int(dec[0]), [int(dec[1]), int(dec[2])], int(dec[3]), int(dec[4])), hex(rnti)
        assert list(r.cqi) == dec[8:].tolist() and list(r.cqi)[:q.cqi_len] == g[name + ".rec_uci"][i, 3:3 + q.cqi_len].tolist(), hex(rnti)
        # and off the steps, at 30 dB: the correlation and the LLRs themselves, by the rules of the other receive tests
        rng = np.random.default_rng(rnti)
        noisy = (want + rng.normal(0, np.sqrt(0.5e-3), R.glen) + 1j * rng.normal(0, np.sqrt(0.5e-3), R.glen)).astype(np.complex64)[None]
        rc, res = rx.batch(noisy, tti, [q])
        assert rc == 0
        excl = collections.Counter()
        _compare(R, noisy, tti, [q], res, rx.debug(1, 1), rx.debug(0, 1), excl)
        assert not excl["tie"] and not excl["threshold"] and list(res[0].cqi) == dec[8:].tolist(), (hex(rnti), dict(excl))
    dres = pkg.DevBuf(C.sizeof(pkg.PucchRes))
    pkg.lib().srslte_hip_memset(dres.ptr, 0x5A, dres.nbytes)
    dg = pkg.DevBuf.from_host(np.zeros((1, R.glen), np.complex64))
    for rnti in (0x000A, 0xFFF3):
        q = pkg.PucchReq.make(0, rnti, cqi_len=4, n_pucch_2=5)
        assert rx.run_device(dg.ptr, 9, 1, [q], dres.ptr) == INVALID
        assert tx.put_device(dg.ptr, 9, 1, [pkg.PucchTx.make(q, cqi=[1, 0, 1, 1])]) == INVALID
    pkg.sync()
    assert (dres.to_host(np.uint8) == 0x5A).all() and not dg.to_host(np.complex64).any()
    tx.free()
    rx.free()


def test_grants_pipeline_with_pucch_at_n_oc_2():
    """srslte_hip_ul_rx_batch_grants_pucch on S5 with a PUSCH on PRBs 8-17: PUCCHs at n_oc 2 on the outermost PRB pair and on the innermost m
    whose PRBs (6 and 18) clear the PUSCH, and a format 2 on the same PRB pair in the other slots (m = 12): byte for byte the stand-alone pucch_batch results."""
    name = "S5"
    spec = SWEEP_CELLS[name]
    P, cell_id, nsf, tti0 = spec[0], spec[1], 2, 4321
    rng = np.random.default_rng(78)
    grants, datas = [], []
    for b in range(nsf):
        grants.append(pkg.UlGrant.make(b, 0x400, 10, 8, 1, 1544, n_dmrs=b))
        datas.append(rng.integers(0, 256, 1544 // 8, dtype=np.uint8))
    utx = pkg.UlTx(cell_id, P, 0x1234, 1, 1544, 10, 8, 0, nsf, max_grants=len(grants))
    iq = utx.encode_grants(datas, tti0, nsf, grants).reshape(nsf, -1)
    utx.free()
    m0, per, thr = spec[6] + (spec[5] + 7) // 8, 3 * 12 // spec[4], threshold(spec)
    m_in = 13  # m / 2 = 6 and nof_prb - 1 - m / 2 = 18: the last m whose two PRBs lie outside 8..17
    n_oc = golden()[name + ".f1_state"][:, 0, :, 0, 1]
    f1 = [[thr + (m - m0) * per + j for j in range(per) if 2 in n_oc[thr + (m - m0) * per + j]][:2] for m in (m0, m_in)]
    f1 = f1[0] + f1[1]
    assert len(f1) == 4 and [int(golden()[name + ".f1_prb"][n, 0]) for n in f1] == [2, 2, 18, 18]
    txs, reqs = [], []
    for sf in range(nsf):
        for k, n in enumerate(f1):
            q = pkg.PucchReq.make(sf, 0x50 + k, ack_len=1 + k % 2, ncce=n - spec[7])
            txs.append(pkg.PucchTx.make(q, ack=(int(rng.integers(0, 2)), int(rng.integers(0, 2)))))
            reqs.append(q)
        q = pkg.PucchReq.make(sf, 0x60, cqi_len=7, ack_len=1, simul_cqi_ack=True, n_pucch_2=12 * (m_in - 1) + 5 + sf)
        txs.append(pkg.PucchTx.make(q, ack=(1, 0), cqi=[int(b) for b in rng.integers(0, 2, 7)]))
        reqs.append(q)
    nue = len(f1) + 1
    ctx = pkg.UlCtrlTx(P, cell_id, max_pucch=len(txs), **kw(spec))
    ofdm = pkg.Ofdm(P, True, rx=False)
    ofdm.set_freq_shift(0.5)
    for k in range(nue):  # each UE its own grids: a put writes, the air adds
        rc, ue_grid = ctx.put(np.zeros((nsf, 14 * 12 * P), np.complex64), tti0, txs[k::nue])
        assert rc == 0
        iq = (iq + ofdm.tx_sf(ue_grid)).astype(np.complex64)
    ctrl = pkg.UlCtrl(P, cell_id, max_pucch=len(reqs), **kw(spec, threshold_data_valid_format2=0.5))
    rx1 = pkg.UlRx(cell_id, P, 0x1234, 1, 1544, 10, 8, 0, 6, nsf, max_grants=len(grants))
    rc, tb, ok, pres = rx1.decode_grants_pucch(iq, tti0, grants, ctrl, reqs)
    assert rc == 0 and ok.all() and all(np.array_equal(tb[p][:1544 // 8], datas[p]) for p in range(len(grants)))
    rxo = pkg.Ofdm(P, True, rx=True)
    rxo.set_freq_shift(-0.5)
    rc, alone = ctrl.batch(rxo.rx_sf(iq), tti0, reqs)
    assert rc == 0
    for a, b in zip(alone, pres):
        assert bytes(a) == bytes(b)
    for t, q, r in zip(txs, reqs, pres):  # UEs that share an RB are not separated by the reference's estimator: the lone format 2 is
        if q.cqi_len:
            assert r.detected == 1 and r.format == F2A and r.cqi_crc == 1 and list(r.ack)[:1] == [1] and list(r.cqi)[:7] == list(t.cqi)[:7]
    for o in (ctrl, ctx, rx1, ofdm, rxo):
        o.free()
