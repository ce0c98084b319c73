"""The core objects' memory (csrc/dev_buf.hpp in tdec.hip, chest.hip and fft.hip) and the turbo decoder's per-call options (TdecOpts), as
test_gpu_object_lifecycle.py and test_gpu_pipeline_lifecycle.py do it for the modules built on them, at the smallest shapes each path has.

Create / use / destroy, three times in a row per kind; the kinds are chosen so that every part an object makes on first use (the widened
LLRs of the 8-bit fall-back, the 16-window tables, the estimator's per-antenna records, an MBSFN area's pilots, a grant's DMRS, the
frequency-shift table) is there at destroy in one kind and absent in another. Each use is compared as test_gpu_parity.py compares that
module: decoder bytes, pass counts and CRC flags bit-exact against the oracle on the same LLRs, estimates and transforms at its bounds.

Modes interleaved on one object: a run of the decoder depends on its own options only, so a direct-assembly call, a HARQ call with skip
flags and a grants call give on one object what each gives on a fresh one. Then the configurations the decoder refuses."""
import ctypes as C
import importlib

import numpy as np
import pytest

from _libs import OrcCell, OrcChestCfg, OrcChestRes, OrcChestUlRes, OrcOfdm, OrcUlDmrs, OrcUlDmrsCfg, hip, opaque, oracle, p, ref
from lte_sim import DlConfig, OrcHarq, make_subframe, oracle_rx
from test_gpu_object_lifecycle import need_ref
from test_gpu_parity import _chest_case, assert_close_c
from test_gpu_pipeline_lifecycle import _chest

pkg = importlib.import_module("srslte-emane_amd")
pytestmark = pytest.mark.gpu

P, CELL = 6, 1
vp, u32 = C.c_void_p, C.c_uint32


# ---------------------------------------------------------------- turbo decoder
TDEC_MAX_K, NCB, NIT = 2112, 3, 6  # three blocks: the last wavefront of the two-blocks-per-wavefront kernels is half filled


def _coded_blocks(K, seed, scale, dtype):
    """NCB noise-free blocks of length K with CRC24B attached (the early stop fires), as LLRs +-scale in the plain [s p0 p1] layout."""
    rng = np.random.default_rng(seed)
    llr = np.zeros((NCB, 3 * K + 12), dtype)
    for i in range(NCB):
        payload = rng.integers(0, 256, (K - 24) // 8, dtype=np.uint8)
        crc = oracle().orc_crc_bytes(0x1800063, 24, p(payload), K - 24)
        bits = np.unpackbits(np.concatenate([payload, np.array([crc >> 16, (crc >> 8) & 255, crc & 255], np.uint8)]))
        rc, enc = pkg.tcod_encode(bits, K)
        assert rc == 0
        llr[i] = scale * (2 * enc[0].astype(np.int32) - 1)
    return llr


def _tdec_same_as_oracle(dec, K, llr8, seed=0):
    llr = _coded_blocks(K, 100 * K + seed, 20 if llr8 else 100, np.int8 if llr8 else np.int16)
    rc, out, iters, ok = dec.run_all(llr, K, NIT, crc_poly=pkg.CRC24B, crc_nbits=K, llr8=llr8)
    assert rc == 0
    run = oracle().orc_tdec_run_8bit if llr8 else oracle().orc_tdec_run
    for i in range(NCB):
        per = np.zeros((NIT, K // 8), np.uint8)
        assert run(p(llr[i]), False, K, NIT, None, p(per)) == 0
        n, good = 0, False
        while n < NIT and not good:
            good = oracle().orc_crc_bytes(0x1800063, 24, p(per[n]), K) == 0
            n += 1
        assert iters[i] == n and bool(ok[i]) == good and np.array_equal(out[i], per[n - 1]), (K, llr8, i, iters[i], n, ok[i], good)
    assert ok.all() and (iters < NIT).all()  # noise free: every block stops early


def _use_tdec(K, llr8):
    dec = pkg.Tdec(TDEC_MAX_K, NCB)
    _tdec_same_as_oracle(dec, K, llr8)
    dec.free()


# ---------------------------------------------------------------- downlink estimator
def _chest_cfgs(**kw):
    hc, oc = pkg.ChestDlCfg(), OrcChestCfg()
    hc.filter_coef[0], hc.filter_coef[1] = oc.filter_coef[0], oc.filter_coef[1] = 4.0, 1.0
    for k, v in kw.items():
        setattr(hc, k, 1 if v is True else v)
        setattr(oc, k, v)
    return hc, oc


def _last_raw(est):
    L = pkg.lib()
    L.srslte_hip_chest_dl_last_raw.restype, L.srslte_hip_chest_dl_last_raw.argtypes = vp, [vp]
    return L.srslte_hip_chest_dl_last_raw(est.h)


def _use_chest_dl_one_port():
    """One port, one antenna, no result record asked for: the per-(port, antenna) records are never made."""
    rng, tti0, nsf = np.random.default_rng(201), 8, 2
    cases = [_chest_case(P, CELL, (tti0 + b) % 10, rng) for b in range(nsf)]
    grids = np.stack([g for _, g in cases])
    hc, oc = _chest_cfgs()
    est = pkg.ChestDl(CELL, P)
    dg, dce = pkg.DevBuf.from_host(grids), pkg.DevBuf(grids.nbytes)
    assert pkg.lib().srslte_hip_chest_dl_estimate_batch(est.h, C.byref(hc), tti0, dg.ptr, dce.ptr, None, nsf, None) == 0
    pkg.sync()
    ce = dce.to_host(np.complex64).reshape(nsf, -1)
    for b in range(nsf):
        want, res = np.zeros(14 * 12 * P, np.complex64), OrcChestRes()
        assert oracle().orc_chest_dl(C.byref(cases[b][0]), (tti0 + b) % 10, C.byref(oc), p(grids[b]), p(want), C.byref(res)) == 0
        assert_close_c(ce[b], want, "ce sf %d" % b)
    assert _last_raw(est) is None
    est.free()


def _use_chest_dl_two_ports(grow):
    """Two ports, two antennas: the records are made by the first call; with grow, a second call of twice the subframes replaces them."""
    orc = oracle()
    orc.orc_chest_dl_ports_state.argtypes = [vp, u32, vp, u32, vp, vp, vp, vp, vp]
    rng, npt, nrx = np.random.default_rng(202), 2, 2
    nre, n = 12 * P, 14 * 12 * P
    cell, est = OrcCell(CELL, P, npt, True), pkg.ChestDl(CELL, P, npt)
    hc, oc = _chest_cfgs()
    k, l = np.arange(n) % nre, np.arange(n) // nre
    assert _last_raw(est) is None
    for tti0, nsf in ((8, 2), (3, 4))[:2 if grow else 1]:
        grids = np.zeros((nsf, nrx, n), np.complex64)
        for b in range(nsf):
            g = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.7).astype(np.complex64)
            for pp in range(npt):
                orc.orc_crs_put_sf(C.byref(cell), (tti0 + b) % 10, pp, p(g))
            for a in range(nrx):
                h = ((3 + np.sin(k / 40.0 + a)) * np.exp(1j * (k / 100.0 + 0.1 * l + a))).astype(np.complex64)
                grids[b, a] = (g * h + 0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
        rc, ce, res, raw = est.estimate_multi(grids, tti0, hc, nrx)
        assert rc == 0 and _last_raw(est) is not None
        for b in range(nsf):
            ce2, ores = [np.zeros(n, np.complex64) for _ in range(npt * nrx)], OrcChestRes()
            gl = [np.ascontiguousarray(grids[b, a]) for a in range(nrx)]
            gp, cp = (vp * nrx)(*[x.ctypes.data for x in gl]), (vp * (npt * nrx))(*[c.ctypes.data for c in ce2])
            assert orc.orc_chest_dl_ports_state(C.byref(cell), (tti0 + b) % 10, C.byref(oc), nrx, gp, cp, C.byref(ores), None, p(np.zeros(16, np.float32))) == 0
            for pt in range(npt):
                for a in range(nrx):
                    assert_close_c(ce[b, pt, a], ce2[pt * nrx + a], "ce call at %d sf %d port %d ant %d" % (tti0, b, pt, a))
            for name in ("noise_estimate", "rsrp", "rsrq"):
                x, y = float(res[name][b]), float(getattr(ores, name))
                assert abs(x - y) <= 1e-4 * abs(y) + 1e-9, (name, tti0, b, x, y)
    est.free()


def _use_chest_dl_mbsfn():
    """An extended-CP cell with the pilots of two MBSFN areas, one estimate in each."""
    orc = oracle()
    orc.orc_chest_dl_mbsfn.argtypes = [vp, u32, vp, u32, u32, vp, vp, vp]
    rng, tti0, nsf = np.random.default_rng(203), 1, 2
    nre, n = 12 * P, 12 * 12 * P
    cell, est = OrcCell(CELL, P, 1, False), pkg.ChestDl(CELL, P, 1, cp_norm=False)
    L = pkg.lib()
    L.srslte_hip_chest_dl_mbsfn_pilots.restype, L.srslte_hip_chest_dl_mbsfn_pilots.argtypes = vp, [vp, C.c_uint16]
    k, l = np.arange(n) % nre, np.arange(n) // nre
    h = ((3 + np.sin(k / 40.0)) * np.exp(1j * (k / 100.0 + 0.1 * l))).astype(np.complex64)
    for area in (1, 255):
        hc, oc = _chest_cfgs(interpolate_subframe=True)
        hc.mbsfn_area_id = area
        assert L.srslte_hip_chest_dl_mbsfn_pilots(est.h, area) is None
        assert est.set_mbsfn_area_id(area) == 0 and L.srslte_hip_chest_dl_mbsfn_pilots(est.h, area) is not None
        grids = np.zeros((nsf, 1, n), np.complex64)
        for b in range(nsf):
            g = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.7).astype(np.complex64)
            assert orc.orc_mbsfn_put_sf(C.byref(cell), tti0 + b, 0, area, p(g)) == 0
            grids[b, 0] = (g * h + 0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
        rc, ce, noise = est.estimate_mbsfn(grids, tti0, hc)
        assert rc == 0
        for b in range(nsf):
            want, nz = np.zeros(n, np.complex64), C.c_float(0)
            assert orc.orc_chest_dl_mbsfn(C.byref(cell), tti0 + b, C.byref(oc), area, 0, p(np.ascontiguousarray(grids[b, 0])), p(want), C.byref(nz)) == 0
            assert_close_c(ce[b, 0, 0], want, "ce area %d sf %d" % (area, b))
            assert abs(noise[b, 0, 0] - nz.value) <= 1e-4 * nz.value, (area, b, noise[b, 0, 0], nz.value)
    est.free()


# ---------------------------------------------------------------- uplink estimator
def _use_chest_ul():
    """estimate_pusch for (L_prb, n_dmrs) = (1, 0), (2, 3) and (1, 0) again: the object's DMRS table is replaced twice."""
    rng, tti0, nsf, n_prb = np.random.default_rng(204), 7, 2, 1
    q = pkg.ChestUl(CELL, P, 4, 11, True, False)
    o, cfg = OrcUlDmrs(), OrcUlDmrsCfg(4, 11, True, False)
    oracle().orc_ul_dmrs_init(C.byref(o), CELL)
    nre, ng = 12 * P, 14 * 12 * P
    for L, n_dmrs in ((1, 0), (2, 3), (1, 0)):
        grids, refs = np.zeros((nsf, ng), np.complex64), []
        for b in range(nsf):
            r = np.zeros(2 * 12 * L, np.complex64)
            assert oracle().orc_ul_dmrs_pusch_gen(C.byref(o), C.byref(cfg), L, (tti0 + b) % 10, n_dmrs, p(r)) == 0
            g = (0.5 * (rng.standard_normal(ng) + 1j * rng.standard_normal(ng))).astype(np.complex64)
            k = np.arange(12 * L)
            h = ((1.0 + 0.5 * np.cos(k / 25.0 + b)) * np.exp(1j * (b + k / 120.0))).astype(np.complex64)
            for s_, sym in enumerate((3, 10)):
                g[sym * nre + 12 * n_prb: sym * nre + 12 * (n_prb + L)] = r[s_ * 12 * L:(s_ + 1) * 12 * L] * h
            grids[b] = g + (0.02 + 0.05 * b) * (rng.standard_normal(ng) + 1j * rng.standard_normal(ng))
            refs.append(r)
        rc, ce, res = q.estimate_pusch(grids, tti0, L, n_prb, n_dmrs)
        assert rc == 0
        for b in range(nsf):
            ce_o, ores = np.zeros(ng, np.complex64), OrcChestUlRes()
            assert oracle().orc_chest_ul_pusch(p(refs[b]), P, L, n_prb, p(np.ascontiguousarray(grids[b])), p(ce_o), C.byref(ores)) == 0
            assert_close_c(ce[b], ce_o, "ce L %d sf %d" % (L, b))
            for j, nm in enumerate(("noise_estimate", "noise_estimate_dbm", "snr", "snr_db")):
                x = getattr(ores, nm)
                assert abs(res[b, j] - x) <= 1e-4 * abs(x) + 1e-5, (L, nm, res[b, j], x)
    q.free()


# ---------------------------------------------------------------- OFDM
def _use_ofdm(shifts):
    """Modulator and demodulator of one subframe; shifts: the frequency shifts set one after the other before the transforms, the last one in force."""
    rng, q = np.random.default_rng(205), OrcOfdm()
    assert oracle().orc_ofdm_init(C.byref(q), P, True) == 0
    q.normalize, q.exact = True, True
    tx, rx = pkg.Ofdm(P, True, rx=False), pkg.Ofdm(P, True, rx=True)
    for o in (tx, rx):
        o.set_normalize(True)
        for s in shifts:
            o.set_freq_shift(s)
    if shifts:
        q.freq_shift, q.freq_shift_f = True, shifts[-1]
    grid = (rng.standard_normal((1, 14 * 12 * P)) + 1j * rng.standard_normal((1, 14 * 12 * P))).astype(np.complex64)
    t_ref = np.zeros(q.sf_sz, np.complex64)
    oracle().orc_ofdm_tx_sf(C.byref(q), p(grid[0]), p(t_ref))
    assert_close_c(tx.tx_sf(grid)[0], t_ref, "ofdm_tx %s" % (shifts,))
    time_in = (rng.standard_normal((1, q.sf_sz)) + 1j * rng.standard_normal((1, q.sf_sz))).astype(np.complex64)
    g_ref = np.zeros(14 * 12 * P, np.complex64)
    oracle().orc_ofdm_rx_sf(C.byref(q), p(time_in[0]), p(g_ref))
    assert_close_c(rx.rx_sf(time_in)[0], g_ref, "ofdm_rx %s" % (shifts,))
    tx.free()
    rx.free()


USES = {"tdec_k40_unwindowed": lambda: _use_tdec(40, False), "tdec_k408_8_windows": lambda: _use_tdec(408, False),
        "tdec_k816_pair": lambda: _use_tdec(816, False), "tdec_8bit_k408_widened": lambda: _use_tdec(408, True),
        "tdec_8bit_k816_sse8": lambda: _use_tdec(816, True), "tdec_8bit_k2112_avx8": lambda: _use_tdec(2112, True),
        "chest_dl_one_port": _use_chest_dl_one_port, "chest_dl_two_ports_two_antennas": lambda: _use_chest_dl_two_ports(False),
        "chest_dl_two_ports_records_grow": lambda: _use_chest_dl_two_ports(True), "chest_dl_extended_cp_two_mbsfn_areas": _use_chest_dl_mbsfn,
        "chest_ul_three_grants": _use_chest_ul, "ofdm": lambda: _use_ofdm(()), "ofdm_freq_shift_set_twice": lambda: _use_ofdm((0.5, -0.5))}


@pytest.mark.parametrize("kind", sorted(USES))
def test_create_use_destroy_three_times(kind):
    for _ in range(3):
        USES[kind]()


# ---------------------------------------------------------------- modes interleaved on one object
MOD, TBS, CFI = 1, 792, 1  # QPSK; 792 + 24 = 816: one code block of the smallest length the 16-window decoder takes
NB = TBS // 8


def _dl_cfg(rnti=0x1234):
    return DlConfig(P, CELL, MOD, TBS, cfi=CFI, rnti=rnti)


def _dl_rx():
    return pkg.DlRx(CELL, P, CFI, 0x1234, MOD, TBS, 6, 1, True, _chest())


def _fixed_direct(rx, rng, tti, harq):
    """New data through the fixed-grant call, whose decoder assembles the transport block itself -> (transport block bytes, flag)."""
    cfg = _dl_cfg()
    iq, data = make_subframe(cfg, tti, rng)
    r = oracle_rx(cfg, iq, tti, harq=harq, rv=0, new_data=True)
    tb, ok = rx.decode(iq[None], tti)
    assert r["ok"] and ok[0] == 1 and np.array_equal(tb[0], r["tb"]) and np.array_equal(tb[0][:NB], data), tti
    assert np.array_equal(rx.debug(6, np.uint32, 1), r["iters"])
    return data, tb[0].tobytes() + ok.tobytes()


def test_dl_rx_direct_harq_direct_on_one_object():
    """One fixed-grant receiver of a single K = 816 block (TBS 792, no table entry), on 6 PRB with QPSK: the smallest cell and modulation there
    are, and the oracle chain alone decodes it noise free in one pass there (subframes other than 0 and 5 carry 828 PDSCH symbols, 1656 bits
    for the 2460 coded ones; checked on the CPU). (a) new data, assembled by the decoder; (b) the same data again with rv 2 and new_data = 0,
    which runs with skip flags and the assembly kernel - the block was acknowledged in (a), so it is not decoded again and, as in the oracle
    (sch.c:404-410), not delivered; (c) new data again, assembled by the decoder: each as the oracle's chain with one soft buffer, (c) also
    byte for byte what a fresh object gives for the same call."""
    rng, cfg, rx, harq = np.random.default_rng(301), _dl_cfg(), _dl_rx(), None
    harq = OrcHarq(cfg)
    data, _ = _fixed_direct(rx, rng, 3, harq)
    iq, _ = make_subframe(cfg, 4, rng, rv=2, data=data)
    r = oracle_rx(cfg, iq, 4, harq=harq, rv=2, new_data=False)
    tb, ok = rx.decode_harq(iq[None], 4, 2, False)
    assert bool(ok[0]) == r["ok"] and np.array_equal(rx.debug(6, np.uint32, 1), r["iters"]) and r["iters"][0] == 0
    state = rng.bit_generator.state
    _, got = _fixed_direct(rx, rng, 6, harq)
    fresh = _dl_rx()
    rng.bit_generator.state = state
    _, want = _fixed_direct(fresh, rng, 6, OrcHarq(cfg))
    assert got == want
    rx.free()
    fresh.free()


def test_dl_rx_grants_fixed_grants_on_one_object():
    """A grants call (the decoders assemble a ragged batch: block counts per slot, the CRC24A tables of K = 816), a fixed-grant call (the
    one-length assembly) and a grants call again on one receiver, different payloads and RNTIs: each as the oracle's chain."""
    rng, rx = np.random.default_rng(302), _dl_rx()
    for n, (tti, rnti) in enumerate(((3, 0x77), (4, None), (6, 0x78))):
        if rnti is None:
            _fixed_direct(rx, rng, tti, None)
            continue
        cfg = _dl_cfg(rnti)
        iq, data = make_subframe(cfg, tti, rng)
        r = oracle_rx(cfg, iq, tti)
        rc, tb, ok = rx.decode_grants(iq[None], tti, [pkg.DlGrant.make(P, MOD, TBS, rnti, cfi=CFI)])
        assert rc == 0 and r["ok"] and ok[0] == 1 and np.array_equal(tb[0], r["tb"]) and np.array_equal(tb[0][:NB], data), n
    rx.free()


@need_ref
def test_single_call_resume_then_another_length_on_one_object():
    """srslte_tdec_new_cb and two srslte_tdec_iteration calls (the second continues the first's pass), then srslte_tdec_new_cb for another
    length and srslte_tdec_run_all on the same srslte_tdec_t: what the reference's decoder gives for the same calls."""
    H, R, rng = hip(), ref(), np.random.default_rng(303)
    outs = []
    for L in (H, R):
        tdec = opaque(1 << 16)
        assert L.srslte_tdec_init(tdec, 6144) == 0
        L.srslte_tdec_force_not_sb(tdec)
        outs.append((L, tdec, []))
    for K, resume in ((816, True), (408, False)):
        bits = rng.integers(0, 2, K).astype(np.uint8)
        rc, enc = pkg.tcod_encode(bits, K)
        assert rc == 0
        llr = (100 * ((2.0 * enc[0] - 1) + 0.9 * rng.standard_normal(3 * K + 12))).astype(np.int16)
        for L, tdec, got in outs:
            out = np.zeros(K // 8, np.uint8)
            assert L.srslte_tdec_new_cb(tdec, K) == 0
            if resume:
                for it in range(2):
                    L.srslte_tdec_iteration(tdec, p(llr), p(out))
                    got.append((out.tobytes(), L.srslte_tdec_get_nof_iterations(tdec)))
            else:
                assert L.srslte_tdec_run_all(tdec, p(llr), p(out), 4, K) == 0
                got.append((out.tobytes(), L.srslte_tdec_get_nof_iterations(tdec)))
    assert outs[0][2] == outs[1][2] and [n for _, n in outs[0][2]] == [1, 2, 4]
    assert outs[0][2][0][0] != outs[0][2][1][0]  # at this noise the second pass still changes bits
    for L, tdec, _ in outs:
        L.srslte_tdec_free(tdec)


# ---------------------------------------------------------------- refused configurations
def test_invalid_configurations_are_refused():
    """A block length below 40 or above 6144, no blocks; then a run with a length above the object's and one that is no interleaver size: after
    each the same object - or, after a refused create, a fresh one - decodes K = 40."""
    for bad in ((39, 1), (6145, 1), (40, 0)):
        with pytest.raises(RuntimeError):
            pkg.Tdec(*bad)
        dec = pkg.Tdec(40, NCB)
        _tdec_same_as_oracle(dec, 40, False, seed=1)
        dec.free()
    dec = pkg.Tdec(TDEC_MAX_K, NCB)
    for K in (2176, 41):
        rc, *_ = dec.run_all(np.zeros((1, 3 * K + 12), np.int16), K, 1)
        assert rc == pkg.SRSLTE_ERROR, K
        _tdec_same_as_oracle(dec, 40, False, seed=K)
    dec.free()
