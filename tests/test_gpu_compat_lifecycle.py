"""Lifetimes in the single-call API (csrc/compat.cpp over csrc/compat_link.hpp): every object is created, used and freed three times and
gives the same bytes each time; srslte_tcod_encode_lut's three zero-copy regions come from one reservation whatever state the thread's
arena is in; a call still waits for its stream exactly once; host threads that end take their stream, arena and stages with them and the
next thread starts from nothing. Round 1 of every object is held to the oracle, the reference or the golden data the way
tests/test_gpu_compat.py, test_gpu_sch_host.py and test_gpu_ulsch_decode.py hold it. The error paths (a device call that fails half way) are
not provoked here: tests/test_compat_link_sanitizer.py walks them on the CPU. srslte_dlsch_encode2 has no case here: with one in this file,
tests/test_gpu_sch_encode_host.py, which runs later in the same process, ended in a segmentation fault whose cause was not found, so the
function, its thread's encoder object and its tests are as they were."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

from _libs import OrcCell, OrcChestCfg, OrcChestRes, OrcOfdm, RefCell, RefChestRes, RefDlSfCfg, acopy, aligned, hip, make_crc, opaque, oracle, p, ref
from test_gpu_compat import DftPlan, close

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(ref() is None, reason="oracle/_ref/libsrslte_ref.so not built")
HERE = os.path.dirname(os.path.abspath(__file__))


def cplx(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def three_rounds(one_round):
    """one_round(first) -> bytes-comparable arrays; `first`: hold them to the reference. Rounds 2 and 3 are byte-equal to round 1"""
    r1 = one_round(True)
    for k in (2, 3):
        rk = one_round(False)
        assert len(rk) == len(r1)
        for i, (a, b) in enumerate(zip(r1, rk)):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), ("round", k, "output", i)


def in_thread(fn):
    """fn() on a host thread of its own that ends before this returns -> its result"""
    box = {}

    def run():
        try:
            box["r"] = fn()
        except BaseException as e:  # noqa: B036 - handed to the caller's thread
            box["e"] = e
    t = threading.Thread(target=run)
    t.start()
    t.join()
    if "e" in box:
        raise box["e"]
    return box["r"]


# ---------------------------------------------------------------------------------------------------- create, use, free: three times
@pytest.mark.parametrize("kind", ["c", "r", "guru"])
def test_dft_plan_three_rounds(kind):
    L, rng, N = hip(), np.random.default_rng(1), 128
    x = aligned(256, np.complex64)
    x[:] = cplx(rng, 256)
    xr = rng.standard_normal(256).astype(np.float32)

    def one_round(first):
        pl, outs = DftPlan(), []
        y = aligned(256, np.complex64)
        yr = np.zeros(256, np.float32)
        if kind == "guru":
            assert L.srslte_dft_plan_guru_c(C.byref(pl), N, 0, p(x), p(y), 1, 1, 1, N, N) == 0
        else:
            assert (L.srslte_dft_plan_c if kind == "c" else L.srslte_dft_plan_r)(C.byref(pl), N, 0) == 0
        for n in (N, 2 * N, N):  # as planned, replanned up, replanned down again
            if n != pl.size:
                if kind == "guru":
                    assert L.srslte_dft_replan_guru_c(C.byref(pl), n, p(x), p(y), 1, 1, 1, n, n) == 0
                else:
                    assert (L.srslte_dft_replan_c if kind == "c" else L.srslte_dft_replan_r)(C.byref(pl), n) == 0
            assert pl.size == n
            y[:] = 0
            if kind == "guru":
                L.srslte_dft_run_guru_c(C.byref(pl))
            elif kind == "c":
                L.srslte_dft_run_c(C.byref(pl), p(x), p(y))
            else:
                L.srslte_dft_run_r(C.byref(pl), p(xr), p(yr))
            out = yr[:n].copy() if kind == "r" else y[:n].copy()
            if first:
                refo = np.zeros(n, np.float32 if kind == "r" else np.complex64)
                if kind == "r":
                    oracle().orc_dft_r2hc(p(xr), p(refo), n, 1)
                else:
                    oracle().orc_dft_exact(p(np.ascontiguousarray(x[:n])), p(refo), n, 1)
                assert close(out, refo), (kind, n)
            outs.append(out)
        L.srslte_dft_plan_free(C.byref(pl))
        assert pl.size == 0 and not pl.p
        return outs
    three_rounds(one_round)


def test_ofdm_objects_three_rounds():
    L, rng, prb = hip(), np.random.default_rng(2), 6
    N = L.srslte_symbol_sz(prb)
    nre, sf = 14 * 12 * prb, 15 * N
    g = cplx(rng, nre)

    def one_round(first):
        grid_in, time_buf, grid_out = aligned(2 * nre, np.float32), aligned(2 * sf, np.float32), aligned(2 * nre, np.float32)
        tx, rx, outs = opaque(4096), opaque(4096), []
        assert L.srslte_ofdm_tx_init(tx, 0, p(grid_in), p(time_buf), prb) == 0 and L.srslte_ofdm_rx_init(rx, 0, p(time_buf), p(grid_out), prb) == 0
        for again in (False, True):  # the second pass after a set_prb, which frees and rebuilds the state
            if again:
                assert L.srslte_ofdm_tx_set_prb(tx, 0, prb) == 0 and L.srslte_ofdm_rx_set_prb(rx, 0, prb) == 0
            L.srslte_ofdm_set_normalize(tx, True)
            L.srslte_ofdm_set_normalize(rx, True)
            grid_in.view(np.complex64)[:] = g
            L.srslte_ofdm_tx_sf(tx)
            t = time_buf.view(np.complex64).copy()
            L.srslte_ofdm_rx_sf(rx)
            outs += [t, grid_out.view(np.complex64).copy()]
            if first:
                q = OrcOfdm()
                assert oracle().orc_ofdm_init_sz(C.byref(q), prb, N, True) == 0
                q.normalize = True
                ref_t = np.zeros(sf, np.complex64)
                oracle().orc_ofdm_tx_sf(C.byref(q), p(g), p(ref_t))
                assert close(t, ref_t) and np.mean(np.abs(outs[-1] - g) ** 2) < 1e-9
        L.srslte_ofdm_tx_free(tx)
        L.srslte_ofdm_rx_free(rx)
        return outs
    three_rounds(one_round)


def test_dft_precoding_three_rounds():
    L, rng = hip(), np.random.default_rng(3)
    x = cplx(rng, 12 * 12)

    def one_round(first):
        q, y = opaque(1 << 16), np.zeros_like(x)
        assert L.srslte_dft_precoding_init_tx(q, 6) == 0
        assert L.srslte_dft_precoding(q, p(x), p(y), 1, 12) == 0
        if first:
            refo = np.zeros_like(x)
            oracle().orc_dft_precoding(p(x), p(refo), 1, 12, 1, True)
            assert close(y, refo)
        L.srslte_dft_precoding_free(q)
        return [y]
    three_rounds(one_round)


@pytest.mark.parametrize("K", [40, 6144])
@pytest.mark.parametrize("llr8", [False, True])
def test_tdec_three_rounds(K, llr8):
    L, rng = hip(), np.random.default_rng(K + llr8)
    bits, enc = rng.integers(0, 2, K).astype(np.uint8), np.zeros(3 * K + 12, np.uint8)
    oracle().orc_tcod_encode_bits(p(bits), p(enc), K)
    if llr8:
        llr = (20 * ((2.0 * enc - 1) + 0.8 * rng.standard_normal(enc.shape))).clip(-128, 127).astype(np.int8)
    else:
        llr = (100 * ((2.0 * enc - 1) + 0.9 * rng.standard_normal(enc.shape))).astype(np.int16)

    def one_round(first):
        tdec, out = opaque(1 << 16), np.zeros(K // 8, np.uint8)
        assert L.srslte_tdec_init(tdec, 6144) == 0
        L.srslte_tdec_force_not_sb(tdec)
        assert (L.srslte_tdec_run_all_8bit if llr8 else L.srslte_tdec_run_all)(tdec, p(llr), p(out), 4, K) == 0
        if first:
            refo = np.zeros(K // 8, np.uint8)
            (oracle().orc_tdec_run_8bit if llr8 else oracle().orc_tdec_run)(p(llr), False, K, 4, p(refo), None)
            assert np.array_equal(out, refo) and L.srslte_tdec_get_nof_iterations(tdec) == 4
        L.srslte_tdec_free(tdec)
        return [out]
    three_rounds(one_round)


def chest_case(rng, cid, prb, sf_idx):
    n, nre = 14 * 12 * prb, 12 * prb
    cell = OrcCell(cid, prb, 1, True)
    g = (cplx(rng, n) * 0.7).astype(np.complex64)
    oracle().orc_crs_put_sf(C.byref(cell), sf_idx, 0, p(g))
    k, l = np.arange(n) % nre, np.arange(n) // nre
    grid = acopy((g * ((3 + np.sin(k / 40.0)) * np.exp(1j * (k / 100.0 + 0.1 * l))) + 0.05 * rng.standard_normal(n)).astype(np.complex64).view(np.float32))
    return cell, grid, n


def chest_estimate(L, est, res, grid, sf_idx):
    sf = RefDlSfCfg()
    sf.tti = 10 + sf_idx
    inp = (C.c_void_p * 4)(grid.ctypes.data, 0, 0, 0)
    return L.srslte_chest_dl_estimate(est, C.byref(sf), inp, C.byref(res))


def test_chest_dl_three_rounds():
    """6 PRB / 1 port / 1 antenna, then set_cell to 15 PRB and back: each set_cell destroys and rebuilds the device estimator"""
    L, rng, cid, sf_idx = hip(), np.random.default_rng(5), 2, 4
    cases = {prb: chest_case(rng, cid, prb, sf_idx) for prb in (6, 15)}

    def one_round(first):
        est, res, outs = opaque(1 << 16), RefChestRes(), []
        assert L.srslte_chest_dl_init(est, 15, 1) == 0 and L.srslte_chest_dl_res_init(C.byref(res), 15) == 0
        for prb in (6, 15, 6):
            cell, grid, n = cases[prb]
            assert L.srslte_chest_dl_set_cell(est, RefCell(prb, 1, cid, 0, 0, 0, 0)) == 0
            assert chest_estimate(L, est, res, grid, sf_idx) == 0
            ce = np.ctypeslib.as_array(C.cast(res.ce[0][0], C.POINTER(C.c_float)), (2 * n,)).view(np.complex64).copy()
            outs += [ce, np.float32([res.noise_estimate, res.snr_db, res.rsrp_dbm, res.rsrq_db, res.rssi_dbm])]
            if first:
                refo, rres, oc = np.zeros(n, np.complex64), OrcChestRes(), OrcChestCfg()
                assert oracle().orc_chest_dl(C.byref(cell), sf_idx, C.byref(oc), p(grid), p(refo), C.byref(rres)) == 0
                assert close(ce, refo)
                assert abs(res.noise_estimate - rres.noise_estimate) <= 1e-4 * rres.noise_estimate and abs(res.snr_db - rres.snr_db) < 1e-3
                assert abs(res.rsrp_dbm - rres.rsrp_dbm) < 1e-3 and np.isnan(res.sync_error)
        L.srslte_chest_dl_res_free(C.byref(res))
        L.srslte_chest_dl_free(est)
        return outs
    three_rounds(one_round)


@needs_ref
def test_dlsch_decode2_three_rounds():
    """6 PRB QPSK tbs 328, then 25 PRB 16QAM tbs 4008 on the same srslte_sch_t: the transport-block decoder behind it is made again"""
    from lte_sim import OrcSchCfg
    from test_gpu_sch_host import Side, hip_seg
    H, R, orc, rng = hip(), ref(), oracle(), np.random.default_rng(6)
    blocks = []
    for prb, tbs, mod, nre in ((6, 328, 1, 600), (25, 4008, 2, 3000)):
        nbits, data = nre * 2 * mod, rng.integers(0, 256, tbs // 8, dtype=np.uint8)
        sch, bits = OrcSchCfg(tbs, nbits, 2 * mod, 0, 4), np.zeros(nbits, np.uint8)
        assert orc.orc_dlsch_encode(C.byref(sch), p(data), p(bits)) == 0
        e = np.clip(np.round(100.0 * ((2.0 * bits - 1) + 0.5 * rng.standard_normal(nbits))), -32000, 32000).astype(np.int16)
        blocks.append((prb, tbs, mod, nbits, data, e))

    def grant(side, tbs, mod, nbits):
        """a new transport block on the side's srslte_sch_t and soft buffer"""
        for f, v in (("mod", mod), ("tbs", tbs), ("nof_bits", nbits)):
            o = side.tb0 + side.Ly["srslte_ra_tb_t." + f]
            side.g[o:o + 4].view(np.uint32)[0] = v
        side.set(0, 1)
        R.srslte_softbuffer_rx_reset(side.sb)

    def one_round(first):
        outs = []
        sides = [Side(True, 25, 328, 1, 1200, False, 4)] + ([Side(False, 25, 328, 1, 1200, False, 4)] if first else [])
        for prb, tbs, mod, nbits, data, e in blocks:
            K, C_ = hip_seg(tbs)
            got = []
            for s in sides:
                grant(s, tbs, mod, nbits)
                out = np.zeros(tbs // 8 + 64, np.uint8)
                rc = s.decode(e.copy(), out, 1)
                crc, _, _, tbc = s.soft(C_, 3 * (K + 32) + 12)
                got.append((rc, out, crc, tbc))
            rc, out, crc, tbc = got[0]
            outs += [np.int32([rc, tbc]), out, crc]
            if first:
                rc_r, out_r, crc_r, tbc_r = got[1]
                assert rc == rc_r == 0 and np.array_equal(out[:tbs // 8 + 3], out_r[:tbs // 8 + 3]) and np.array_equal(crc, crc_r) and tbc == tbc_r
                assert np.array_equal(out[:tbs // 8], data)
        for s in sides:
            R.srslte_softbuffer_rx_free(s.sb)
        H.srslte_tdec_free(C.c_void_p(C.addressof(sides[0].q) + sides[0].Ly["srslte_sch_t.decoder"]))
        return outs
    three_rounds(one_round)


@needs_ref
def test_ulsch_decode_three_rounds():
    """6 PRB QPSK tbs 1544, then tbs 6200 on the same srslte_sch_t (the object is made again for the larger block)"""
    import test_gpu_ulsch_decode as U
    shapes = [U.Shape(6, U.QPSK, 12, 1544), U.Shape(6, U.QPSK, 12, 6200)]
    sent = [U.transmit(sh, 0, U.payload(sh.tbs), U.CLEAN, 7 + i) for i, sh in enumerate(shapes)]

    def one_round(first):
        mine, outs = U.Rx(True), []
        theirs = U.Rx(False) if first else None
        for sh, (llr, c_seq) in zip(shapes, sent):
            ref().srslte_softbuffer_rx_reset(mine.sb)
            m = mine.decode(sh, 0, llr, c_seq)
            if first:
                ref().srslte_softbuffer_rx_reset(theirs.sb)
                U.same(m, theirs.decode(sh, 0, llr, c_seq), sh, ("tbs", sh.tbs))
                U.same_soft(mine, theirs, sh, ("tbs", sh.tbs))
            outs += [np.int32([m["rc"], m["K_segm"]]), m["data"], m["g"]]
        mine.free()
        if first:
            theirs.free()
        return outs
    three_rounds(one_round)


# ---------------------------------------------------------------------------------------------------- srslte_tcod_encode_lut: one reservation
def lut_golden(L):
    """every case of tests/golden/tcod_lut.npz (cblen_idx 0 .. 187, last_cb and crc_cb on and off) on the calling thread"""
    g = np.load(os.path.join(HERE, "golden", "tcod_lut.npz"))
    tcod = opaque(64)
    assert L.srslte_tcod_init(tcod, 6144) == 0
    seen = set()
    for n in range(6):
        idx, K, with_cb, last, tb_init, tb_final = (int(v) for v in g["meta_%d" % n])
        buf, par = g["in_%d" % n].copy(), np.zeros(K // 4 + 2, np.uint8)
        crc_tb, crc_cb = make_crc(0x1864CFB, 24), make_crc(0x1800063, 24)
        crc_tb.crcinit = tb_init
        assert L.srslte_tcod_encode_lut(tcod, C.byref(crc_tb), C.byref(crc_cb) if with_cb else None, p(buf), p(par), idx, bool(last)) == 3 * K + 12
        assert np.array_equal(buf, g["sys_%d" % n]) and np.array_equal(par[: K // 4 + 1], g["par_%d" % n]) and crc_tb.crcinit == tb_final, n
        seen |= {("idx", idx), ("cb", with_cb), ("last", last)}
    assert {("idx", 0), ("idx", 187), ("cb", 0), ("cb", 1), ("last", 0), ("last", 1)} <= seen
    L.srslte_tcod_free(tcod)
    return True


def test_tcod_encode_lut_on_a_fresh_and_on_a_large_arena():
    L = hip()

    def body():
        assert lut_golden(L)  # the thread's first use of its arena: the reservation makes it
        prb = 100             # a 100 PRB subframe makes the arena large and leaves it empty
        N = L.srslte_symbol_sz(prb)
        t, g = aligned(2 * 15 * N, np.float32), aligned(2 * 14 * 12 * prb, np.float32)
        rx = opaque(4096)
        assert L.srslte_ofdm_rx_init(rx, 0, p(t), p(g), prb) == 0
        t[:] = np.random.default_rng(8).standard_normal(t.size).astype(np.float32)  # the init clears the bound input buffer
        L.srslte_ofdm_rx_sf(rx)
        assert np.abs(g).max() > 0
        assert lut_golden(L)
        L.srslte_ofdm_rx_free(rx)
        return True
    assert in_thread(body)


# ---------------------------------------------------------------------------------------------------- one stream wait per call
def waits(L):
    out = (C.c_ulonglong * 4)()
    L.srslte_hip_compat_stats(out)
    return out[0]


def test_one_stream_wait_per_call():
    """[0] of srslte_hip_compat_stats grows by exactly one per call once the thread's arena and the objects' stages have their size. The whole
    test runs on a thread of its own, so no other thread's calls are counted in between."""
    L, rng = hip(), np.random.default_rng(9)

    def body():
        K, prb = 6144, 6
        sym, llr16 = cplx(rng, 300), np.zeros(2 * 300, np.int16)
        tcod, tdec = opaque(64), opaque(1 << 16)
        assert L.srslte_tcod_init(tcod, 6144) == 0 and L.srslte_tdec_init(tdec, 6144) == 0
        L.srslte_tdec_force_not_sb(tdec)  # the plain 3K + 12 input layout
        bits, enc = rng.integers(0, 2, K).astype(np.uint8), np.zeros(3 * K + 12, np.uint8)
        g = np.load(os.path.join(HERE, "golden", "tcod_lut.npz"))
        llr, dec = (100 * (2.0 * rng.integers(0, 2, 3 * K + 12) - 1)).astype(np.int16), np.zeros(K // 8, np.uint8)
        pl, x, y = DftPlan(), cplx(rng, 128), np.zeros(128, np.complex64)
        assert L.srslte_dft_plan_c(C.byref(pl), 128, 0) == 0
        N = L.srslte_symbol_sz(prb)
        t, grid = aligned(2 * 15 * N, np.float32), aligned(2 * 14 * 12 * prb, np.float32)
        rx = opaque(4096)
        assert L.srslte_ofdm_rx_init(rx, 0, p(t), p(grid), prb) == 0
        est, res = opaque(1 << 16), RefChestRes()
        assert L.srslte_chest_dl_init(est, prb, 1) == 0 and L.srslte_chest_dl_set_cell(est, RefCell(prb, 1, 1, 0, 0, 0, 0)) == 0
        assert L.srslte_chest_dl_res_init(C.byref(res), prb) == 0
        _, cgrid, _ = chest_case(rng, 1, prb, 1)

        def lut():
            buf, par, crc_tb = g["in_5"].copy(), np.zeros(6144 // 4 + 2, np.uint8), make_crc(0x1864CFB, 24)
            return L.srslte_tcod_encode_lut(tcod, C.byref(crc_tb), None, p(buf), p(par), 187, False) == 3 * 6144 + 12
        calls = {"srslte_demod_soft_demodulate_s": lambda: L.srslte_demod_soft_demodulate_s(1, p(sym), p(llr16), 300) == 0,
                 "srslte_tcod_encode": lambda: L.srslte_tcod_encode(tcod, p(bits), p(enc), K) == 0,
                 "srslte_tcod_encode_lut": lut,
                 "srslte_tdec_run_all": lambda: L.srslte_tdec_run_all(tdec, p(llr), p(dec), 2, K) == 0,
                 "srslte_dft_run_c": lambda: L.srslte_dft_run_c(C.byref(pl), p(x), p(y)) is None,
                 "srslte_ofdm_rx_sf": lambda: L.srslte_ofdm_rx_sf(rx) is None,
                 "srslte_chest_dl_estimate": lambda: chest_estimate(L, est, res, cgrid, 1) == 0}
        L.srslte_dft_run_c.restype = L.srslte_ofdm_rx_sf.restype = None
        for name, call in calls.items():  # warm-up: the arena and the stages grow here
            assert call(), name
        counts = {}
        for name, call in calls.items():
            w0 = waits(L)
            assert call(), name
            counts[name] = waits(L) - w0
        L.srslte_chest_dl_res_free(C.byref(res))
        L.srslte_chest_dl_free(est)
        L.srslte_ofdm_rx_free(rx)
        L.srslte_dft_plan_free(C.byref(pl))
        L.srslte_tdec_free(tdec)
        L.srslte_tcod_free(tcod)
        return counts
    counts = in_thread(body)
    print("stream waits per call:", counts)
    assert counts == {name: 1 for name in counts} and len(counts) == 7, counts


# ---------------------------------------------------------------------------------------------------- worker threads that end
def test_worker_threads_that_end():
    """three times: a thread runs the demapper, srslte_tcod_encode and srslte_chest_average_pilots and ends; the main thread then makes the
    same calls and gets the same bytes. (srslte_dlsch_encode2 is not among the calls: see the module's note.)"""
    L, rng = hip(), np.random.default_rng(10)
    K, nref, nsym, flen = 512, 50, 4, 5
    sym, bits, pilots = cplx(rng, 300), rng.integers(0, 2, K).astype(np.uint8), cplx(rng, nref * nsym)
    filt = np.float32([1, 2, 3, 2, 1]) / 9
    L.srslte_chest_average_pilots.restype = None

    def calls():
        llr, enc, avg = np.zeros(4 * 300, np.int16), np.zeros(3 * K + 12, np.uint8), np.zeros(nref * nsym, np.complex64)
        tcod = opaque(64)
        assert L.srslte_tcod_init(tcod, 6144) == 0
        assert L.srslte_demod_soft_demodulate_s(2, p(sym), p(llr), 300) == 0
        assert L.srslte_tcod_encode(tcod, p(bits), p(enc), K) == 0
        L.srslte_chest_average_pilots(p(pilots), p(avg), p(filt), nref, nsym, flen)
        L.srslte_tcod_free(tcod)
        return [llr, enc, avg]
    first = None
    for k in range(3):
        a, b = in_thread(calls), calls()
        first = first or a
        for i, (u, v, w) in enumerate(zip(a, b, first)):
            assert u.tobytes() == v.tobytes() == w.tobytes(), ("round", k, "output", i)
    refo = np.zeros(3 * K + 12, np.uint8)
    oracle().orc_tcod_encode_bits(p(bits), p(refo), K)
    assert np.array_equal(first[1], refo) and np.abs(first[0]).max() > 0 and np.abs(first[2]).max() > 0
