"""PUCCH formats 1-2b on the device (srslte_hip_ul_ctrl_tx_put_pucch, srslte_hip_ul_ctrl_pucch_batch, srslte_hip_ul_rx_batch_grants_pucch)
against the reference chain of tests/ul_ctrl_ref.py: transmitted grids, every decision of srslte_enb_ul_get_pucch over drawn requests with
AWGN, the SR retry, the grants pipeline with PUCCHs beside PUSCHs, a device round trip through the SC-FDMA modulator, refusals and calls
queued on one stream."""
import collections
import ctypes as C
import importlib

import numpy as np
import pytest

from _libs import aligned, ref
from ul_ctrl_ref import F1, F1A, F1B, F2, F2A, F2B, RefUlCtrl, select

pkg = importlib.import_module("srslte-emane_amd")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(ref() is None, reason="oracle/_ref/libsrslte_ref.so is not built")]

# (nof_prb, cell_id, cp_ext, group hopping, delta_pucch_shift, N_cs, n_rb_2, N_pucch_1)
CELLS = [(6, 1, False, False, 1, 0, 1, 0), (25, 200, True, True, 2, 4, 2, 3), (50, 150, False, True, 3, 6, 2, 1), (100, 5, False, False, 2, 6, 3, 2),
         (75, 301, True, False, 1, 7, 1, 5)]
TH = dict(threshold_format1=0.8, threshold_data_valid_format1a=0.9, threshold_data_valid_format2=1.5)


def _kw(spec, **extra):
    P, cid, ext, gh, D, Ncs, nrb2, N1 = spec
    return dict(cp_ext=ext, group_hopping_en=gh, delta_pucch_shift=D, N_cs=Ncs, n_rb_2=nrb2, N_pucch_1=N1, **dict(TH, **extra))


def _ref(spec):
    return RefUlCtrl(pkg.ul_ctrl_cfg(spec[0], spec[1], **_kw(spec)))


def _draw_ue(rng, sf, k, kind, spec, shortened, rnti):
    """A UE k of subframe sf: (the eNB's PucchReq, the UE's PucchTx or None when it sends nothing)."""
    N1 = spec[7]
    ack = (int(rng.integers(0, 2)), int(rng.integers(0, 2)))
    cqi_len = int(rng.integers(1, 13))
    cqi = [int(b) for b in rng.integers(0, 2, cqi_len)]
    base = dict(ncce=2 * k, n_pucch_sr=N1 + 2 * k + 1, n_pucch_2=k + int(rng.integers(0, 2)) * 12 * spec[6], shortened=shortened)
    mk = lambda **a: pkg.PucchReq.make(sf, rnti, **dict(base, **a))  # noqa: E731
    if kind == "sr":         # SR TTI, SR sent (or not)
        sent = rng.random() < 0.7
        return mk(sr_tti=True), (pkg.PucchTx.make(mk(sr_tti=True), sr=1) if sent else None)
    if kind == "ack":        # 1 or 2 HARQ-ACK bits, sometimes in an SR TTI with a positive SR
        n, srv = int(rng.integers(1, 3)), int(rng.random() < 0.3)
        return mk(ack_len=n, sr_tti=bool(srv or rng.random() < 0.3)), pkg.PucchTx.make(mk(ack_len=n, sr_tti=bool(srv)), ack=ack, sr=srv)
    if kind == "cqi":
        return mk(cqi_len=cqi_len), pkg.PucchTx.make(mk(cqi_len=cqi_len), cqi=cqi)
    if kind == "ri":
        return mk(ri_len=1), pkg.PucchTx.make(mk(ri_len=1), ri=ack[0])
    if kind == "cqi_ack":    # 2a / 2b with simul_cqi_ack, or the drop to 1a / 1b without it
        n, simul = int(rng.integers(1, 3)), bool(rng.random() < 0.7)
        q = mk(ack_len=n, cqi_len=cqi_len, simul_cqi_ack=simul)
        return q, pkg.PucchTx.make(q, ack=ack, cqi=cqi)
    if kind == "ri_ack":
        n = int(rng.integers(1, 3))
        q = mk(ack_len=n, ri_len=1)
        return q, pkg.PucchTx.make(q, ack=ack, ri=int(rng.integers(0, 2)))
    q = mk(ack_len=int(rng.integers(1, 3)))  # "dtx": a HARQ-ACK expected, nothing sent
    return q, None


KINDS = ["sr", "ack", "cqi", "ri", "cqi_ack", "ri_ack", "dtx"]


def _scene(spec, rng, nof_sf, per_sf, snr_db, tti0):
    """Requests, UE transmissions and the received grids [nof_sf][glen] (the restated encoder, unit channel, AWGN)."""
    R = _ref(spec)
    reqs, txs, grid = [], [], np.zeros((nof_sf, R.glen), np.complex64)
    for sf in range(nof_sf):
        shortened = bool(rng.random() < 0.3)
        for k in range(per_sf):
            q, t = _draw_ue(rng, sf, k, KINDS[int(rng.integers(0, len(KINDS)))], spec, shortened, 0x46 + 16 * sf + k)
            reqs.append(q)
            if t is not None:
                g = aligned(R.glen, np.complex64)
                R.encode(g, tti0 + sf, t)
                grid[sf] += g
                txs.append(t)
    noise = np.float32(10 ** (-snr_db / 10))
    grid += (rng.normal(0, np.sqrt(noise / 2), grid.shape) + 1j * rng.normal(0, np.sqrt(noise / 2), grid.shape)).astype(np.complex64)
    for q in reqs:
        q.noise_estimate = float(noise) * float(rng.choice([0.0, 0.5, 1.0]))
    return R, reqs, txs, grid


def _near(x, th, eps=1e-4):
    return abs(float(x) - float(th)) < eps


def _excluded(R, grid_sf, tti, q, want, got_llr):
    """Why a decision is set aside (None: it is compared): the reference takes it within 1e-4 of a threshold ("threshold") or of a tie between
    hypotheses ("tie"), or a format-2 LLR sits on a truncation step that the few-ulp difference of the equaliser moved by one ("llr")."""
    c, fmt, corr = R.cfg, want["format"], want["corr"]
    if fmt < F2:
        hyp = sorted(want["hyp"], reverse=True)
        if len(hyp) > 1 and hyp[0] - hyp[1] < 1e-4:
            return "tie"
        if _near(corr, c.threshold_format1) or _near(corr, c.threshold_data_valid_format1a):
            return "threshold"
        return None
    if not np.array_equal(got_llr, want["llr"]):
        d = got_llr.astype(int) - want["llr"].astype(int)
        assert np.abs(d).max() <= 1 and np.count_nonzero(d) <= 2, (got_llr, want["llr"])
        return "llr"
    if _near(corr, c.threshold_data_valid_format2):
        return "threshold"
    if fmt in (F2A, F2B):  # the DMRS hypotheses' |sum| within 1e-4 (relative) of each other
        idx = R.dmrs_re(fmt, want["n_pucch"])
        x = []
        for h in range(2 if fmt == F2A else 4):
            r = R.dmrs(fmt, want["n_pucch"], tti, (h % 2, h // 2))
            x.append(abs(np.sum(grid_sf[idx].astype(np.complex128) * np.conj(r))))
        x = sorted(x, reverse=True)
        if x[0] - x[1] < 1e-4 * max(x[0], 1e-12):
            return "tie"
    return None


def _compare(R, grid, tti0, reqs, got, llrs, zs, excl):
    for i, q in enumerate(reqs):
        want, g = R.decode(_al(grid[q.sf]), tti0 + q.sf, q), got[i]
        assert (g.format, g.n_pucch) == (want["format"], want["n_pucch"]), (i, q.sf, g.format, want["format"], g.n_pucch, want["n_pucch"])
        nre = want["z"].size
        assert np.abs(zs[i][:nre] - want["z"]).max() <= 1e-3 * max(1.0, np.abs(want["z"]).max()), i
        why = _excluded(R, grid[q.sf], tti0 + q.sf, q, want, llrs[i])
        if why:
            excl[why] += 1
            continue
        if want["format"] >= F2:
            assert g.correlation == pytest.approx(float(want["corr"]), abs=1e-6), i
        else:
            assert abs(g.correlation - float(want["corr"])) < 1e-4, (i, g.correlation, want["corr"])
        assert (g.detected, g.sr, list(g.ack), g.ack_valid, list(g.cqi), g.cqi_crc, g.ri) == \
               (want["detected"], want["sr"], want["ack"], want["ack_valid"], want["cqi"], want["cqi_crc"], want["ri"]), (i, want["format"])


def _al(x):
    a = aligned(x.size, np.complex64)
    a[:] = x
    return a


@pytest.mark.parametrize("idx", range(len(CELLS)))
def test_put_pucch_matches_reference_encoder(idx):
    """Every format, both CPs, shortened or not, group hopping on / off; two PUCCHs on distinct PRBs in some subframes, shared PRBs across
    subframes; a random background that must stay as it was outside the PUCCHs' REs."""
    spec = CELLS[idx]
    rng = np.random.default_rng(300 + idx)
    R = _ref(spec)
    nof_sf, tti0 = 20, int(rng.integers(0, 10240))
    tx = pkg.UlCtrlTx(spec[0], spec[1], max_pucch=64, **_kw(spec))
    txs, want = [], (rng.normal(size=(nof_sf, R.glen)) + 1j * rng.normal(size=(nof_sf, R.glen))).astype(np.complex64)
    bg = want.copy()
    seen = set()
    for sf in range(nof_sf):
        sh = bool(sf % 3 == 1)
        kinds = ["ack", "sr"] if sf % 2 else ["cqi", "cqi_ack", "ri", "ri_ack"]
        t = None
        while t is None:
            q, t = _draw_ue(rng, sf, 0, kinds[int(rng.integers(0, len(kinds)))], spec, sh, 0x100 + sf)
        if sf % 2:  # format 1 family only: m >= n_rb_2 ...
            ue = [t]
            if sf % 4 == 1:  # ... beside a format 2 with n_pucch_2 < 12 n_rb_2 (m < n_rb_2): distinct PRBs
                q2 = pkg.PucchReq.make(sf, 0x200 + sf, cqi_len=int(rng.integers(1, 13)), n_pucch_2=int(rng.integers(0, 12 * spec[6])), shortened=sh)
                ue.append(pkg.PucchTx.make(q2, cqi=[int(b) for b in rng.integers(0, 2, q2.cqi_len)]))
        else:
            ue = [pkg.PucchTx.make(t.req, ack=tuple(t.ack), sr=t.sr, ri=t.ri, cqi=list(t.cqi)[:t.req.cqi_len])]
            ue[0].req.n_pucch_2 = int(rng.integers(0, 12 * spec[6] + 24))
        for u in ue:
            g = _al(want[sf])
            seen.add(R.encode(g, tti0 + sf, u))
            want[sf] = g
            txs.append(u)
    rc, got = tx.put(bg, tti0, txs)
    assert rc == 0
    assert np.abs(got - want).max() < 1e-5
    touched = np.abs(want - bg) > 0
    assert np.array_equal(got[~touched].view(np.uint32), bg[~touched].view(np.uint32))
    assert seen >= {F1A, F1B, F2}
    tx.free()


def test_put_pucch_every_format_both_cps():
    """One PUCCH of each format (2a only on the normal CP, as get_format selects it), shortened and not, on both CPs."""
    for spec in (CELLS[0], CELLS[1]):
        R = _ref(spec)
        tx = pkg.UlCtrlTx(spec[0], spec[1], max_pucch=16, **_kw(spec))
        mk = lambda sf, **a: pkg.PucchReq.make(sf, 0x77, ncce=1, n_pucch_sr=7, n_pucch_2=3, **a)  # noqa: E731
        cases = [pkg.PucchTx.make(mk(0, sr_tti=True), sr=1), pkg.PucchTx.make(mk(1, ack_len=1), ack=(1, 0)),
                 pkg.PucchTx.make(mk(2, ack_len=2, shortened=True), ack=(0, 1)), pkg.PucchTx.make(mk(3, cqi_len=11), cqi=[1, 0] * 5 + [1]),
                 pkg.PucchTx.make(mk(4, cqi_len=4, ack_len=1, simul_cqi_ack=True), ack=(1, 0), cqi=[1, 1, 0, 1]),
                 pkg.PucchTx.make(mk(5, cqi_len=4, ack_len=2, simul_cqi_ack=True, shortened=True), ack=(1, 1), cqi=[0, 1, 0, 1])]
        want = np.zeros((6, R.glen), np.complex64)
        fmts = []
        for sf, t in enumerate(cases):
            g = _al(want[sf])
            fmts.append(R.encode(g, 7 + sf, t))
            want[sf] = g
        assert fmts == ([F1, F1A, F1B, F2, F2B, F2B] if spec[2] else [F1, F1A, F1B, F2, F2A, F2B])
        rc, got = tx.put(np.zeros_like(want), 7, cases)
        assert rc == 0 and np.abs(got - want).max() < 1e-5
        tx.free()


@pytest.mark.parametrize("idx", range(len(CELLS)))
def test_receive_matches_reference_chain(idx):
    """Drawn requests of every kind (SR with and without ACK, 1 / 2 ACK bits, CQI of 1-12 bits, RI, reports with ACK with and without
    simul_cqi_ack, absent PUCCHs) over n_pucch on both sides of c N_cs / delta and 12 n_rb_2, at several SNRs: every decision and the
    correlation equal the reference chain's; decisions at a threshold or a tie, and format-2 LLRs an ulp moved, are set aside and counted."""
    spec = CELLS[idx]
    rng = np.random.default_rng(500 + idx)
    total, excl = 0, collections.Counter()
    for snr in (30.0, 6.0, 0.0, -6.0):
        tti0 = int(rng.integers(0, 10240))
        R, reqs, _, grid = _scene(spec, rng, 10, 5, snr, tti0)
        rx = pkg.UlCtrl(spec[0], spec[1], max_pucch=len(reqs), **_kw(spec))
        rc, got = rx.batch(grid, tti0, reqs)
        assert rc == 0
        _compare(R, grid, tti0, reqs, got, rx.debug(1, len(reqs)), rx.debug(0, len(reqs)), excl)
        total += len(reqs)
        rx.free()
    print("cell %d: %d requests, set aside %s" % (idx, total, dict(excl)))
    # measured on an MI355X: one of the 1000 requests of the five cells set aside (an LLR moved by one); 2 % leaves room, not a hiding place
    assert total >= 200 and sum(excl.values()) <= total // 50 and excl["llr"] <= 2, (total, dict(excl))


def test_sr_retry_on_the_ack_resource():
    """An SR TTI with HARQ-ACK where only the ACK resource carries energy: not found on n_pucch_sr, decoded again on ncce + N_pucch_1."""
    spec = CELLS[2]
    R = _ref(spec)
    rx = pkg.UlCtrl(spec[0], spec[1], max_pucch=4, **_kw(spec))
    reqs, grid = [], np.zeros((4, R.glen), np.complex64)
    for sf, (n, ack) in enumerate([(1, (1, 0)), (2, (0, 1)), (1, (0, 0)), (2, (1, 1))]):
        ue = pkg.PucchTx.make(pkg.PucchReq.make(sf, 0x60 + sf, ack_len=n, ncce=4 + sf, n_pucch_sr=20 + sf), ack=ack)
        g = _al(grid[sf])
        R.encode(g, 40 + sf, ue)
        grid[sf] = g
        reqs.append(pkg.PucchReq.make(sf, 0x60 + sf, ack_len=n, ncce=4 + sf, sr_tti=True, n_pucch_sr=20 + sf))
    rc, got = rx.batch(grid, 40, reqs)
    assert rc == 0
    for sf, g in enumerate(got):
        want = R.decode(_al(grid[sf]), 40 + sf, reqs[sf])
        assert g.sr == 0 and g.detected == 1 and g.n_pucch == 4 + sf + spec[7] and g.format == (F1A if reqs[sf].ack_len == 1 else F1B)
        assert list(g.ack) == want["ack"] and want["n_pucch"] == g.n_pucch
        assert list(g.ack)[:reqs[sf].ack_len] == list([(1, 0), (0, 1), (0, 0), (1, 1)][sf][:reqs[sf].ack_len])
    rx.free()


def _pusch_scene(prb, nsf, rng):
    grants, datas = [], []
    for b in range(nsf):
        for u in range(2):
            L, n0, mod, tbs = [(10, 10, 1, 1544), (12, 25, 2, 4008)][u]
            grants.append(pkg.UlGrant.make(b, 0x400 + u, L, n0, mod, tbs, n_dmrs=(u + b) % 8))
            datas.append(rng.integers(0, 256, tbs // 8, dtype=np.uint8))
    return grants, datas


def test_grants_pipeline_and_round_trip():
    """put_pucch -> SC-FDMA with the UL half-carrier shift, added to PUSCHs from srslte_hip_ul_tx_batch_grants -> _grants_pucch: the PUSCH
    outputs equal srslte_hip_ul_rx_batch_grants' byte for byte, the PUCCH results equal the stand-alone call on the pipeline's grid, every
    UCI comes back noise-free; then a PUCCH-only batch."""
    prb, nsf, cell_id, tti0 = 50, 8, 150, 1234
    spec = (prb, cell_id, False, True, 2, 4, 2, 1)
    rng = np.random.default_rng(77)
    grants, datas = _pusch_scene(prb, nsf, rng)
    utx = pkg.UlTx(cell_id, prb, 0x1234, 1, 4008, 6, 0, 0, nsf, max_grants=len(grants))
    iq = utx.encode_grants(datas, tti0, nsf, grants).reshape(nsf, -1)
    utx.free()
    txs, reqs = [], []
    for sf in range(nsf):
        for k, kind in enumerate(["sr", "ack", "cqi", "cqi_ack", "ri"]):
            q, t = None, None
            while t is None:
                q, t = _draw_ue(rng, sf, k, kind, spec, False, 0x46 + 8 * sf + k)
            q.sr_tti = 1 if kind == "sr" else q.sr_tti
            # one PRB pair per UE, away from the PUSCHs: the reference's estimate (a 3-tap filter, no despreading over the 12 cyclic shifts)
            # does not separate PUCCHs that share a PRB, so neither can a receiver that equals it
            res = {"sr": (0, 0, 0), "ack": (6 - spec[7], 24, 0), "cqi": (0, 0, 0), "cqi_ack": (42 - spec[7], 60, 12), "ri": (0, 0, 72)}[kind]
            for r in (q, t.req):
                r.ncce, r.n_pucch_sr, r.n_pucch_2 = res
            txs.append(t)
            reqs.append(q)
    ctx = pkg.UlCtrlTx(prb, cell_id, max_pucch=len(txs), **_kw(spec))
    ofdm = pkg.Ofdm(prb, True, rx=False)
    ofdm.set_freq_shift(0.5)
    for k in range(5):  # each UE its own grids (a put writes, it does not add): UE k of every subframe in one call, the air sums them
        rc, ue_grid = ctx.put(np.zeros((nsf, 14 * 12 * prb), np.complex64), tti0, txs[k::5])
        assert rc == 0
        iq = (iq + ofdm.tx_sf(ue_grid)).astype(np.complex64)
    ctrl = pkg.UlCtrl(prb, cell_id, max_pucch=len(reqs), **_kw(spec, threshold_data_valid_format2=0.5))  # a clean report correlates 1.0
    rx1 = pkg.UlRx(cell_id, prb, 0x1234, 1, 4008, 6, 0, 0, 6, nsf, max_grants=len(grants))
    rx2 = pkg.UlRx(cell_id, prb, 0x1234, 1, 4008, 6, 0, 0, 6, nsf, max_grants=len(grants))
    tb1, ok1 = rx1.decode_grants(iq, tti0, grants)
    rc, tb2, ok2, pres = rx2.decode_grants_pucch(iq, tti0, grants, ctrl, reqs)
    assert rc == 0 and np.array_equal(ok1, ok2) and ok1.all()
    for p, g in enumerate(grants):  # the bytes the call writes (tbs / 8 + 3 per row; the rest of a row is the buffer's own)
        assert np.array_equal(tb1[p][:g.tbs // 8 + 3], tb2[p][:g.tbs // 8 + 3]), p
    for p, g in enumerate(grants):
        assert np.array_equal(tb2[p][:g.tbs // 8], datas[p])
    rxo = pkg.Ofdm(prb, True, rx=True)
    rxo.set_freq_shift(-0.5)
    g_rx = rxo.rx_sf(iq)
    rc, alone = ctrl.batch(g_rx, tti0, reqs)
    assert rc == 0
    for a, b in zip(alone, pres):
        assert bytes(a) == bytes(b)
    for t, q, r in zip(txs, reqs, pres):
        assert r.detected == 1 and r.format == select(False, spec[7], q, q.sr_tti)[0], (r.format, q.ack_len, q.cqi_len)
        if q.sr_tti:
            assert r.sr == t.sr
        n = q.ack_len
        assert list(r.ack)[:n] == list(t.ack)[:n], (list(r.ack), list(t.ack), r.format)
        if r.format >= F2:
            assert r.cqi_crc == 1
            if q.ri_len:
                assert r.ri == t.ri
            elif q.cqi_len and (q.simul_cqi_ack or not q.ack_len):
                assert list(r.cqi)[:q.cqi_len] == list(t.cqi)[:q.cqi_len]
    # a PUCCH-only batch
    rc, _, _, only = rx2.decode_grants_pucch(iq, tti0, [], ctrl, reqs)
    assert rc == 0 and all(bytes(a) == bytes(b) for a, b in zip(only, pres))
    for o in (ctrl, ctx, rx1, rx2, ofdm, rxo):
        o.free()


def test_refusals_and_calls_on_one_stream():
    spec = CELLS[3]
    P = spec[0]
    assert pkg.lib().srslte_hip_ul_ctrl_create(C.byref(pkg.ul_ctrl_cfg(P, 5, tdd=True, max_pucch=4))) is None
    assert pkg.lib().srslte_hip_ul_ctrl_create(C.byref(pkg.ul_ctrl_cfg(P, 5, delta_pucch_shift=2, N_cs=3, max_pucch=4))) is None
    assert pkg.lib().srslte_hip_ul_ctrl_create(C.byref(pkg.ul_ctrl_cfg(P, 5, delta_pucch_shift=0, max_pucch=4))) is None
    rx = pkg.UlCtrl(P, spec[1], max_pucch=4, **_kw(spec))
    grid = np.zeros((2, rx.grid_len), np.complex64)
    mk = pkg.PucchReq.make
    bad = [mk(0, 0x46, ack_len=3), mk(0, 0x46, cqi_len=13), mk(0, 0x46, cqi_len=4, ri_len=1), mk(0, 0x46, ri_len=2), mk(0, 0x46),
           mk(0, 0x46, cqi_len=4, n_pucch_2=12 * 2 * P), mk(0, 0x46, ack_len=1, ncce=10000), mk(0, 0x46, sr_tti=True, ack_len=1, ncce=10000),
           mk(2, 0x46, ack_len=1), mk(0, 0x0A, cqi_len=4), mk(0, 0xFFF3, ack_len=1, ri_len=1)]
    dres = pkg.DevBuf(C.sizeof(pkg.PucchRes) * 8)
    pkg.lib().srslte_hip_memset(dres.ptr, 0x5A, dres.nbytes)
    dg = pkg.DevBuf.from_host(grid)
    for q in bad:
        assert rx.run_device(dg.ptr, 0, 2, [mk(0, 0x46, ack_len=1), q], dres.ptr) == -2, (q.ack_len, q.cqi_len, q.ri_len, q.sf)
    assert rx.run_device(dg.ptr, 0, 2, [mk(0, 0x46, ack_len=1)] * 5, dres.ptr) == -2  # nof > max_pucch
    pkg.sync()
    assert (dres.to_host(np.uint8) == 0x5A).all()  # nothing was queued
    assert rx.run_device(dg.ptr, 0, 2, [mk(0, 0x0A, ack_len=1)], dres.ptr) == 0  # format 1 needs no scrambling sequence: any RNTI
    utx = pkg.UlCtrlTx(P, spec[1], max_pucch=2, **_kw(spec))
    assert utx.put_device(dg.ptr, 0, 2, [pkg.PucchTx.make(mk(0, 0x0A, cqi_len=4), cqi=[1, 0, 1, 1])]) == -2
    assert utx.put_device(dg.ptr, 0, 2, [pkg.PucchTx.make(mk(0, 0x46, ack_len=3))]) == -2
    pkg.sync()
    utx.free()
    # three calls on one stream, results read once at the end, equal to the calls made one by one
    rng = np.random.default_rng(9)
    R, reqs, _, g3 = _scene(spec, rng, 3, 4, 10.0, 100)
    st = pkg.lib().srslte_hip_stream_create()
    rx3 = pkg.UlCtrl(P, spec[1], max_pucch=len(reqs), **_kw(spec))
    bufs = [pkg.DevBuf.from_host(g3) for _ in range(3)]
    outs = [pkg.DevBuf(C.sizeof(pkg.PucchRes) * len(reqs)) for _ in range(3)]
    for k in range(3):
        assert rx3.run_device(bufs[k].ptr, 100 + 10 * k, 3, reqs, outs[k].ptr, st) == 0
    pkg.lib().srslte_hip_stream_sync(st)
    for k in range(3):
        rc, one = rx3.batch(g3, 100 + 10 * k, reqs)
        assert rc == 0 and outs[k].to_host(np.uint8).tobytes() == b"".join(bytes(x) for x in one)
    pkg.lib().srslte_hip_stream_destroy(st)
    # the pipeline refuses a control object of another cell before queuing anything
    other = pkg.UlCtrl(P, spec[1] + 1, max_pucch=4, **_kw(spec))
    urx = pkg.UlRx(spec[1], P, 0x1234, 1, 1544, 6, 0, 0, 6, 2, max_grants=2)
    rc, _, _, _ = urx.decode_grants_pucch(np.zeros((2, urx.sf_len), np.complex64), 0, [], other, [mk(0, 0x46, ack_len=1)])
    assert rc == -2
    for o in (rx, rx3, other, urx):
        o.free()


def test_decision_rules_on_ties():
    """The tie and threshold rules themselves. On an empty grid every RM word correlates 0 and the first (word 0) wins; every 2a / 2b DMRS
    hypothesis sums to 0 and the last wins (chest_ul.c's >=); a format 1 whose correlation equals threshold_format1 is detected (>=), a 1a one
    is not (>)."""
    spec = CELLS[2]
    rx = pkg.UlCtrl(spec[0], spec[1], max_pucch=8, **_kw(spec))
    mk = pkg.PucchReq.make
    reqs = [mk(0, 0x50, cqi_len=12, n_pucch_2=3, noise_estimate=0.1), mk(0, 0x51, cqi_len=5, ack_len=1, simul_cqi_ack=True, n_pucch_2=5, noise_estimate=0.1),
            mk(0, 0x52, cqi_len=5, ack_len=2, simul_cqi_ack=True, n_pucch_2=7, noise_estimate=0.1), mk(0, 0x53, ri_len=1, ack_len=2, n_pucch_2=9, noise_estimate=0.1)]
    rc, got = rx.batch(np.zeros((1, rx.grid_len), np.complex64), 0, reqs)
    assert rc == 0
    assert [list(g.cqi) for g in got] == [[0] * 13] * 4 and all(g.correlation == 0 for g in got)
    assert [g.format for g in got] == [F2, F2A, F2B, F2B]
    assert list(got[1].ack) == [1, 0] and list(got[2].ack) == [1, 1] and list(got[3].ack) == [1, 1] and got[3].ri == 0
    rx.free()
    # a threshold equal to the device's own correlation
    R = _ref(spec)
    g = _al(np.zeros(R.glen, np.complex64))
    q1, q1a = mk(0, 0x60, sr_tti=True, n_pucch_sr=3, noise_estimate=0.3), mk(0, 0x61, ack_len=1, ncce=5, noise_estimate=0.3)
    R.encode(g, 0, pkg.PucchTx.make(q1, sr=1))
    R.encode(g, 0, pkg.PucchTx.make(q1a, ack=(1, 0)))
    grid = (np.asarray(g) + np.random.default_rng(3).normal(0, 0.3, g.size).astype(np.float32)).astype(np.complex64)[None]
    probe = pkg.UlCtrl(spec[0], spec[1], max_pucch=2, **_kw(spec))
    rc, c = probe.batch(grid, 0, [q1, q1a])
    assert rc == 0
    probe.free()
    for k, (q, want) in enumerate(((q1, 1), (q1a, 0))):
        at = pkg.UlCtrl(spec[0], spec[1], max_pucch=1, **_kw(spec, threshold_format1=c[k].correlation))
        rc, r = at.batch(grid, 0, [q])
        assert rc == 0 and r[0].correlation == c[k].correlation and r[0].detected == want, (k, r[0].correlation)
        at.free()
