"""A capture of exact zeros, and non-finite symbols, through the kernels of the shared-channel receivers (silent_cases.py says what such a
capture is and why the reference's answer is that of its x86 build; test_silent_oracle.py pins the oracle on these inputs and records its
answers). Integer outputs are compared exactly; the only tolerances are those of finite float figures of the estimator records.

Conversions each test reaches:
  test_demappers_nonfinite        demod_dev::rne / trunc_i behind srslte_hip_demod_soft_demodulate{,_s,_b}_batch: vector bodies, scalar tails and
                                  the casts of BPSK / 256QAM, every modulation, a NaN-only call, a live row beside a non-finite one
  test_chest_*_zero_row           the estimator records of an all-zero grid (no conversion: NaN / infinities in the float figures)
  test_silent_dl[...]             pdsch_demod_kernel (and its two-antenna, two-port and PMCH forms) -> demod_s / demod_b; with csi: csi_apply in
                                  the rate de-matcher (weight -32768, (int16) NaN = 0 in the tail); the soft buffer, compact layout included
  test_silent_ul[...]             pusch_demod_kernel -> demod_s; the 25-PRB shape runs six passes and fails
The pipelines' decoders are judged by the oracle's decoder on the DEVICE's own LLRs (and gains), so that what is compared exactly does not
depend on the last bit of the FFT: LLR view against the oracle chain on the silent rows, everything behind it against the oracle's
rate de-matcher + turbo decoder + CRC fed with the LLR view."""
import ctypes as C
import importlib

import numpy as np
import pytest

from _libs import OrcCell, OrcChestCfg, OrcChestRes, OrcChestUlRes, OrcUlDmrs, OrcUlDmrsCfg, oracle, p
from lte_sim import PmchConfig
from silent_cases import (DL_SHAPES, NONFINITE, UL_SHAPES, DlPipe, UlPipe, check_against_oracle, dl_grants_views, dl_ragged_cfgs, nan_symbols,
                          random_payload, row_of, same_floats, same_row, symbol_set, ul_ragged_cfgs)

pytestmark = pytest.mark.gpu
KIND_DT = {"f": np.float32, "s": np.int16, "b": np.int8}


@pytest.fixture(scope="module")
def hp():
    return importlib.import_module("srslte-emane_amd")


# ------------------------------------------------------------------------------------------------------------------------ B1 demappers
def _orc_demod(mod, x, kind):
    qm = 1 if mod == 0 else 2 * mod
    out = np.zeros(len(x) * qm, KIND_DT[kind])
    assert getattr(oracle(), "orc_demod_soft_" + kind)(mod, p(np.ascontiguousarray(x)), p(out), len(x)) == 0
    return out


@pytest.mark.parametrize("nsym", [7, 16, 33])
@pytest.mark.parametrize("mod", [0, 1, 2, 3, 4])
def test_demappers_nonfinite(hp, mod, nsym):
    """One launch of eleven calls: symbol_set() from each of its eight start offsets (every value in every lane of a group), a live row, a
    call of NaN only, the live row again. nsym 7: all scalar tail for the 8-symbol steps, body + tail for the 4-symbol ones; 16: all body;
    33: body + tail. Against the oracle call by call; the live rows equal what the live row gives in a launch of its own."""
    rng = np.random.default_rng(10 * mod + nsym)
    live = ((rng.standard_normal(nsym) + 1j * rng.standard_normal(nsym)) * 0.7).astype(np.complex64)
    calls = [symbol_set(nsym, s) for s in range(len(NONFINITE))] + [live, nan_symbols(nsym), live]
    x = np.stack(calls)
    for kind in ("f", "s", "b"):
        rc, llr = hp.demod_soft_demodulate(mod, x, kind, len(calls))
        assert rc == 0
        rc, alone = hp.demod_soft_demodulate(mod, live, kind, 1)
        assert rc == 0
        for c, s in enumerate(calls):
            want = _orc_demod(mod, s, kind)
            if kind == "f":
                same_floats(llr[c], want, 1e-6, (mod, nsym, c))
            else:
                assert np.array_equal(llr[c], want), (mod, nsym, kind, c, llr[c], want)
        for c in (8, 10):
            assert llr[c].tobytes() == alone[0].tobytes(), (mod, nsym, kind, c)


# ---------------------------------------------------------------------------------------------------------------- B3 estimator records
def _rows_012_vs_02(run, grids):
    """run(grids [n][...]) -> list of per-row byte strings; the live rows of [live, zero, live] against those of [live, live]"""
    three, two = run(grids), run(grids[[0, 2]])
    assert three[0] == two[0] and three[2] == two[1]


def _chest_case(prb, cid, sf_idx, rng, snr_db=20):
    """test_gpu_parity's stimulus: random REs and the CRS through a smooth channel, plus noise"""
    nre, n = 12 * prb, 14 * 12 * prb
    cell = OrcCell(cid, prb, 1, True)
    g = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.7).astype(np.complex64)
    oracle().orc_crs_put_sf(C.byref(cell), sf_idx, 0, p(g))
    k, l = np.arange(n) % nre, np.arange(n) // nre
    h = ((3 + np.sin(k / 40.0)) * np.exp(1j * (k / 100.0 + 0.1 * l))).astype(np.complex64)
    sig = 10 ** (-snr_db / 20)
    return cell, (g * h + sig * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


def test_chest_dl_zero_row(hp):
    """test_chest_dl's 6-PRB case (cell 1, Gauss filter 4 / 1) on [live, all-zero, live]: the zero row's estimates and record against the
    oracle's field by field (NaN matches NaN, infinities with their sign, finite figures to 1e-4 relative / 1e-3 for the dB figures); the
    live rows byte-identical to a batch without the zero row."""
    prb, cid, tti0 = 6, 1, 8
    rng = np.random.default_rng(prb * 1000 + cid)
    cell = None
    grids = []
    for b in range(3):
        cell, g = _chest_case(prb, cid, (tti0 + b) % 10, rng)
        grids.append(g)
    grids[1] = np.zeros_like(grids[1])
    grids = np.stack(grids)
    hc, oc = hp.ChestDlCfg(), OrcChestCfg()
    hc.filter_coef[0], hc.filter_coef[1] = 4.0, 1.0
    oc.filter_coef[0], oc.filter_coef[1] = 4.0, 1.0
    est = hp.ChestDl(cid, prb)
    ce, res = est.estimate(grids, tti0, hc)
    ref, rres = np.zeros(14 * 12 * prb, np.complex64), OrcChestRes()
    assert oracle().orc_chest_dl(C.byref(cell), (tti0 + 1) % 10, C.byref(oc), p(grids[1]), p(ref), C.byref(rres)) == 0
    assert rres.noise_estimate == 0.0 and np.isnan(rres.snr_db)  # the oracle's answer on a silent grid, as test_silent_oracle records it
    same_floats(ce[1].view(np.float32), ref.view(np.float32), 1e-4, "ce")
    for name in ("noise_estimate", "rsrp", "rsrq", "cfo"):
        same_floats(res[name][1], getattr(rres, name), 1e-4, name)
    for name in ("noise_estimate_dbm", "snr_db", "rsrp_dbm", "rsrq_db", "rssi_dbm"):
        same_floats(res[name][1], getattr(rres, name), 1e-3, name)

    def run(g):
        # tti0 + 2 stays the third grid's TTI: the two-row batch is two calls of one row
        if len(g) == 3:
            ce_, res_ = est.estimate(g, tti0, hc)
            return [ce_[b].tobytes() + b"".join(res_[k][b].tobytes() for k in sorted(res_)) for b in range(3)]
        out = []
        for row, t in zip(g, (tti0, tti0 + 2)):
            ce_, res_ = est.estimate(row[None], t, hc)
            out.append(ce_[0].tobytes() + b"".join(res_[k][0].tobytes() for k in sorted(res_)))
        return out
    _rows_012_vs_02(run, grids)
    est.free()


def test_chest_ul_zero_row(hp):
    """test_chest_ul_pusch_batch's 6-PRB case (cell 3, L = 6) on [live, all-zero, live], as test_chest_dl_zero_row."""
    cell_id, prb, L, n_prb = 3, 6, 6, 0
    rng = np.random.default_rng(cell_id + prb + L)
    cs, ds, gh, sh, n_dmrs, tti0 = 4, 11, True, True, 2, 7
    q = hp.ChestUl(cell_id, prb, cs, ds, gh, sh)
    o, cfg = OrcUlDmrs(), OrcUlDmrsCfg(cs, ds, gh, sh)
    oracle().orc_ul_dmrs_init(C.byref(o), cell_id)
    nre, ng = 12 * prb, 14 * 12 * prb
    grids, refs = np.zeros((3, ng), np.complex64), []
    for b in range(3):
        r = np.zeros(2 * 12 * L, np.complex64)
        assert oracle().orc_ul_dmrs_pusch_gen(C.byref(o), C.byref(cfg), L, (tti0 + b) % 10, n_dmrs, p(r)) == 0
        g = (0.5 * (rng.standard_normal(ng) + 1j * rng.standard_normal(ng))).astype(np.complex64)
        k = np.arange(12 * L)
        h = ((1.0 + 0.5 * np.cos(k / 25.0 + b)) * np.exp(1j * (b + k / 120.0))).astype(np.complex64)
        for s_, sym in enumerate((3, 10)):
            g[sym * nre + 12 * n_prb: sym * nre + 12 * (n_prb + L)] = r[s_ * 12 * L:(s_ + 1) * 12 * L] * h
        grids[b] = g
        refs.append(r)
    grids[1] = 0
    rc, ce, res = q.estimate_pusch(grids, tti0, L, n_prb, n_dmrs)
    assert rc == 0
    ce_o, ores = np.zeros(ng, np.complex64), OrcChestUlRes()
    assert oracle().orc_chest_ul_pusch(p(refs[1]), prb, L, n_prb, p(np.ascontiguousarray(grids[1])), p(ce_o), C.byref(ores)) == 0
    assert ores.noise_estimate == 0.0
    same_floats(ce[1].view(np.float32), ce_o.view(np.float32), 1e-4, "ce")
    for j, nm in enumerate(("noise_estimate", "noise_estimate_dbm", "snr", "snr_db")):
        same_floats(res[1, j], getattr(ores, nm), 1e-4, nm)

    def run(g):
        if len(g) == 3:
            _, ce_, res_ = q.estimate_pusch(g, tti0, L, n_prb, n_dmrs)
            return [ce_[b].tobytes() + res_[b].tobytes() for b in range(3)]
        out = []
        for row, t in zip(g, (tti0, tti0 + 2)):
            _, ce_, res_ = q.estimate_pusch(row[None], t, L, n_prb, n_dmrs)
            out.append(ce_[0].tobytes() + res_[0].tobytes())
        return out
    _rows_012_vs_02(run, grids)
    q.free()


# ------------------------------------------------------------------------------------------------------------------ D the pipelines
def _rows(P, rx, res, n, tti0):
    """the rows of ONE call's result"""
    return [row_of(P, rx, res, b, n, tti0) for b in range(n)]


def _silent_pipeline(P, harq_compact_off=False):
    rng = np.random.default_rng(77)
    t0 = P.tti0
    l0, d0 = P.live(t0, rng)
    l2, d2 = P.live(t0 + 2, rng)
    iq = np.stack([l0, P.silent, l2])
    rx = P.rx(3)
    # 1. live, silent, live
    rows = _rows(P, rx, P.decode(rx, iq, t0), 3, t0)
    llr, gains = P.oracle_front(P.silent, t0 + 1)
    assert np.array_equal(rows[1][2], llr), ("silent LLRs", np.unique(rows[1][2], return_counts=True), np.unique(llr, return_counts=True))
    if P.csi:
        assert np.array_equal(rows[1][3], gains) and not gains.any()
    silent_ok, silent_it, silent_cb = check_against_oracle(P, rows[1], t0 + 1, P.new_harq(), what="silent row")
    assert not silent_ok
    for b, d in ((0, d0), (2, d2)):
        fresh = P.rx(1)
        same_row(rows[b], _rows(P, fresh, P.decode(fresh, iq[b:b + 1], t0 + b), 1, t0 + b)[0], "live row %d against a fresh object" % b)
        fresh.free()
        assert rows[b][1][0] == 1 and np.array_equal(rows[b][0][:len(d)], d) and (rows[b][5] == 1).all(), b
        check_against_oracle(P, rows[b], t0 + b, P.new_harq(), what="live row %d" % b)
    # 2. HARQ after silence: rv 0 on silence (row 0) beside a live first transmission (row 1), then rv 2 of real payloads on both. Every
    # call is made once per object. `off`: created with the compact layout off. `blind`: a compact object none of whose views is read
    # between the two calls - reading the soft-buffer view expands the compact slots, so only on this object does the rv 2 call itself
    # expand the slots that hold the silent pattern, in place, before it combines.
    off = P.rx(2, compact=False) if harq_compact_off else None
    blind = P.rx(2) if harq_compact_off else None
    l1, d1 = P.live(t0 + 1, rng)
    h = [P.new_harq(), P.new_harq()]
    first = np.stack([P.silent, l1])
    rows = _rows(P, rx, P.decode_harq(rx, first, t0, 0, True), 2, t0)
    if off is not None:
        assert rx.parity_compact() and not off.parity_compact()
        for b, r in enumerate(_rows(P, off, P.decode_harq(off, first, t0, 0, True), 2, t0)):
            same_row(rows[b], r, "rv 0 against the whole layout, row %d" % b)
        first_blind = P.decode_harq(blind, first, t0, 0, True)
        assert blind.parity_compact()
        for x, y in zip(first_blind, (np.stack([r[0] for r in rows]), np.concatenate([r[1] for r in rows]))):
            assert np.array_equal(x, y), "rv 0 on the object whose views are not read"
    for b in range(2):
        check_against_oracle(P, rows[b], t0 + b, h[b], 0, True, "harq rv 0 row %d" % b)
    t1 = t0 + 10
    da = random_payload(P.cfg.tbs, rng)
    second = np.stack([P.live(t1, rng, rv=2, data=da)[0], P.live(t1 + 1, rng, rv=2, data=d1)[0]])
    rows = _rows(P, rx, P.decode_harq(rx, second, t1, 2, False), 2, t1)
    if off is not None:
        assert not rx.parity_compact()
        for b, r in enumerate(_rows(P, off, P.decode_harq(off, second, t1, 2, False), 2, t1)):
            same_row(rows[b], r, "rv 2 against the whole layout, row %d" % b)
        off.free()
        res = P.decode_harq(blind, second, t1, 2, False)  # expands its compact slots here
        assert not blind.parity_compact()
        for b, r in enumerate(_rows(P, blind, res, 2, t1)):
            same_row(rows[b], r, "rv 2 with the slots expanded by the call itself, row %d" % b)
        blind.free()
    for b in range(2):
        ok, it, _ = check_against_oracle(P, rows[b], t1 + b, h[b], 2, False, "harq rv 2 row %d" % b)
        if b == 0:  # blocks whose CRC passed on silence are skipped (pass count 0); the others are decoded on top of the silent pattern
            assert np.array_equal(it == 0, silent_cb != 0), (it, silent_cb)
    # 3. a live batch on the same object equals a fresh object's
    iq[1] = l1
    fresh = P.rx(3)
    a, b_ = P.decode(rx, iq, t0), P.decode(fresh, iq, t0)
    for x, y in zip(_rows(P, rx, a, 3, t0), _rows(P, fresh, b_, 3, t0)):
        same_row(x, y, "live batch after silence")
    assert a[1].all()
    rx.free()
    fresh.free()


DL_CASES = {"K352": ("K352", {}), "K832": ("K832", {}), "C2": ("C2", {}), "llr8": ("K832", {"llr8": True}), "csi": ("K352", {"csi": True}),
            "csi8": ("K352", {"csi": True, "llr8": True}), "rx2": ("K352", {"nof_rx": 2}), "ports2": ("K352", {"nof_ports": 2})}


@pytest.mark.parametrize("case", list(DL_CASES))
def test_silent_dl(hp, case):
    """srslte_hip_dl_rx_batch / _batch_harq: the three shapes, 8-bit LLRs, the CSI weighting (16- and 8-bit), two receive antennas, two
    ports. K832 and C2 use the compact parity layout: their HARQ calls are also compared with an object created with the layout off, and
    with a compact object whose views are not read between rv 0 and rv 2 (the compact slots holding the -32768 pattern are expanded in place
    by its rv 2 call)."""
    name, kw = DL_CASES[case]
    mk, tti0 = DL_SHAPES[name]
    _silent_pipeline(DlPipe(hp, mk(**kw), tti0), harq_compact_off=case in ("K832", "C2"))


@pytest.mark.parametrize("name", list(UL_SHAPES))
def test_silent_ul(hp, name):
    """srslte_hip_ul_rx_batch / _batch_harq. On the 25-PRB shape the silent row runs six passes, its block CRC fails and non-zero bytes are
    delivered; the retransmission is then wrap-added onto the -32768 / +-32516 pattern and decoded."""
    _silent_pipeline(UlPipe(hp, UL_SHAPES[name](), 4))


def test_silent_pmch(hp):
    """test_gpu_pmch's 6-PRB case (the MBSFN estimate and pmch_cp's RE mapping in front of the same demapper); no HARQ entry point is
    exercised on a PMCH object beyond what _silent_pipeline does on every object."""
    cfg = PmchConfig(6, 1, 1, 1, 488, cfi=2, non_mbsfn_region=2, nof_rx=1, cp_ext=True)
    cfg.Qm_sch = cfg.Qm
    _silent_pipeline(DlPipe(hp, cfg, 1, pmch=True))


def test_silent_grants_dl(hp):
    """srslte_hip_dl_rx_batch_grants on silent_cases.DL_RAGGED (K = 352, 832, C = 2 x 4992, 800: every body of the mixed decoder launch)
    with each subframe silent in turn, the three steps of _silent_pipeline with per-grant rv / new_data:
    1. rv 0: the silent row's LLRs are the oracle chain's; every row's verdict, bytes, pass counts, block flags and soft buffer are those of
       the oracle's back end on the row's own LLRs; the live rows equal what a fresh object gives for them alone;
    2. rv 2, new_data = 0, clean, a real payload in the silent position: again the oracle's back end with the soft buffers it kept - the
       silent blocks passed their CRC and are skipped, the verdict stays 0;
    3. the live batch on the same object equals the fresh objects' rows."""
    from lte_sim import make_subframe
    cfgs = dl_ragged_cfgs()
    n = len(cfgs)
    pipes = [DlPipe(None, c, 4) for c in cfgs]
    tbs_max = max(c.tbs for c in cfgs)
    hc = hp.ChestDlCfg()
    hc.filter_coef[0], hc.filter_coef[1] = 4.0, 1.0
    rng = np.random.default_rng(21)
    data = [random_payload(c.tbs, rng) for c in cfgs]
    live = np.stack([make_subframe(c, 4 + b, rng, amp=0.1, data=data[b])[0] for b, c in enumerate(cfgs)])

    def run(rx, iq, tti0, cf, rv=0, new=True):
        gr = [hp.DlGrant.make(50, 1, c.tbs, c.rnti, cfi=3, rv=rv, new_data=new, prb_mask=c.prb_mask) for c in cf]
        rc, tb, ok = rx.decode_grants(iq, tti0, gr)
        assert rc == 0
        views = dl_grants_views(rx, cf, tti0)
        return [[tb[b][:c.tbs // 8 + 3].copy(), ok[b:b + 1].copy()] + views[b] for b, c in enumerate(cf)]

    rx = hp.DlRx(150, 50, 3, 0, 1, tbs_max, 6, n, True, hc)
    alone = []
    for b in range(n):
        fresh = hp.DlRx(150, 50, 3, 0, 1, tbs_max, 6, n, True, hc)
        alone.append(run(fresh, live[b:b + 1], 4 + b, cfgs[b:b + 1])[0])
        assert alone[b][1][0] == 1
        fresh.free()
    for pos in range(n):
        iq = live.copy()
        iq[pos] = 0
        rows = run(rx, iq, 4, cfgs)
        llr, _ = pipes[pos].oracle_front(iq[pos], 4 + pos)
        assert np.array_equal(rows[pos][2], llr) and llr.min() == -32768, pos
        h = [P.new_harq() for P in pipes]
        for b in range(n):
            ok, _, cb = check_against_oracle(pipes[b], rows[b], 4 + b, h[b], 0, True, ("rv 0", pos, b))
            assert ok == (b != pos) and cb.all(), (pos, b)
            if b != pos:
                same_row(rows[b], alone[b], "silent subframe %d, live row %d" % (pos, b))
        d2 = list(data)
        d2[pos] = random_payload(cfgs[pos].tbs, rng)
        second = np.stack([make_subframe(c, 14 + b, rng, amp=0.1, rv=2, data=d2[b])[0] for b, c in enumerate(cfgs)])
        rows = run(rx, second, 14, cfgs, 2, False)
        for b in range(n):
            ok, it, _ = check_against_oracle(pipes[b], rows[b], 14 + b, h[b], 2, False, ("rv 2", pos, b))
            assert not ok and not it.any(), (pos, b, it)
        for x, y in zip(run(rx, live, 4, cfgs), alone):
            same_row(x, y, "live batch after silence in subframe %d" % pos)
    rx.free()


def test_silent_grants_ul(hp):
    """srslte_hip_ul_rx_batch_grants on silent_cases.UL_RAGGED, each subframe silent in turn, the same three steps. The grants mode of the
    PUSCH receiver exposes its LLR rows and pass counts only (views 22, 23): verdict, bytes and pass counts are compared with the oracle's
    back end on the row's own LLRs, block flags and soft buffer are not. The silent 16QAM and 64QAM rows fail their block CRCs after six
    passes, so their rv 2 is wrap-added onto the silent pattern and decoded: what it delivers shows the soft buffer."""
    from lte_sim import make_ul_subframe
    cfgs = ul_ragged_cfgs()
    n = len(cfgs)
    pipes = [UlPipe(None, c, 7) for c in cfgs]
    rng = np.random.default_rng(22)
    data = [random_payload(c.tbs, rng) for c in cfgs]
    live = np.stack([make_ul_subframe(c, 7 + b, rng, amp=0.1, data=data[b])[0] for b, c in enumerate(cfgs)])
    stride = (12 * 12 * 25 * 8 + 15) & ~15

    def run(rx, iq, tti0, cf, rv=0, new=True):
        gr = [hp.UlGrant.make(b, c.rnti, c.L_prb, c.n_prb, c.mod, c.tbs, n_dmrs=c.n_dmrs, rv=rv, new_data=new) for b, c in enumerate(cf)]
        tb, ok = rx.decode_grants(iq, tti0, gr)
        m = len(gr)
        e, it = rx.debug(22, np.int16, m * stride).reshape(m, stride), rx.debug(23, np.uint32, m * 2).reshape(m, 2)
        return [[tb[b][:c.tbs // 8 + 3].copy(), ok[b:b + 1].copy(), e[b][:c.nbits].copy(), it[b][:c.seg.C].copy()] for b, c in enumerate(cf)]

    def judge(P, row, tti, harq, rv, new, what):
        tb, ok, it, _ = P.oracle_back(row[2], None, tti, harq, rv, new)
        assert bool(row[1][0]) == ok and np.array_equal(row[3], it), (what, row[1], ok, row[3], it)
        if it.any():
            assert np.array_equal(row[0], tb), (what, "bytes")
        return ok, it

    def mk():
        return hp.UlRx(11, 25, 0x1234, 1, 7992, 6, 0, 0, 6, n, 2, 5, True, False, max_grants=n)

    rx = mk()
    alone = []
    for b in range(n):
        fresh = mk()
        alone.append(run(fresh, live[b:b + 1], 7 + b, cfgs[b:b + 1])[0])
        assert alone[b][1][0] == 1
        fresh.free()
    decoded_on_silence = 0
    for pos in range(n):
        iq = live.copy()
        iq[pos] = 0
        rows = run(rx, iq, 7, cfgs)
        assert np.array_equal(rows[pos][2], pipes[pos].oracle_front(iq[pos], 7 + pos)[0]) and rows[pos][2].min() == -32768, pos
        h = [P.new_harq() for P in pipes]
        for b in range(n):
            ok, _ = judge(pipes[b], rows[b], 7 + b, h[b], 0, True, ("rv 0", pos, b))
            assert ok == (b != pos), (pos, b)
            if b != pos:
                same_row(rows[b], alone[b], "silent subframe %d, live row %d" % (pos, b))
        d2 = list(data)
        d2[pos] = random_payload(cfgs[pos].tbs, rng)
        second = np.stack([make_ul_subframe(c, 17 + b, rng, amp=0.1, rv=2, data=d2[b])[0] for b, c in enumerate(cfgs)])
        rows = run(rx, second, 17, cfgs, 2, False)
        for b in range(n):
            ok, it = judge(pipes[b], rows[b], 17 + b, h[b], 2, False, ("rv 2", pos, b))
            decoded_on_silence += int(b == pos and it.any())
        for x, y in zip(run(rx, live, 7, cfgs), alone):
            same_row(x, y, "live batch after silence in subframe %d" % pos)
    assert decoded_on_silence >= 2
    rx.free()
