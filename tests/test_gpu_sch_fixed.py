"""The transport-block back end the fixed-grant pipelines share (SchRxFixed / SchTxFixed, sch_fixed.inc and pusch_tx.inc): every branch of it on
the smallest shapes that reach it, and that a call depends on its arguments alone. Inputs are noise-free, so every expectation is exact: all CRC
flags 1, the bytes those that were sent; there is no tolerance anywhere in this file.

Shapes ((prb, mod, tbs) of the existing cases; the CPU oracle decodes each of them in one pass):
  short  6 PRB, QPSK, TBS 328:             K = 352 <= 800: the unwindowed decoder and tb_crc_kernel                 (test_gpu_mimo CASES)
  win1   6 PRB, extended CP, QPSK, TBS 808: one windowed block, K = 832                                             (test_gpu_parity_compact)
  c2     50 PRB, CFI 3, QPSK, TBS 9912:    C = 2, K = 4992 = 78 * 64; 6300 / 6156 LLRs per block on subframes 4 / 5, below E_lim(4992) = 7182:
                                           the compact parity layout (16QAM as in test_gpu_mimo would hand a block twice that)
  UL     15 PRB, L = 3, QPSK, TBS 328 (K = 352) and 25 PRB, L = 10, 16QAM, TBS 4008 (K = 4032)                      (test_gpu_ul_harq)
A batch is TTIs 4, 5 (1, 2 for win1, whose subframe 5 carries fewer bits than K): two subframe classes, more than one workgroup per kernel."""
import ctypes as C
import importlib

import numpy as np
import pytest

from lte_sim import DlConfig, UlConfig, make_subframe, make_subframe_mimo, make_ul_subframe

pytestmark = pytest.mark.gpu

AMP = 0.1
DL = {"short": (lambda l8: DlConfig(6, 1, 1, 328, cfi=3, llr8=l8), 4), "win1": (lambda l8: DlConfig(6, 7, 1, 808, cfi=3, cp_ext=True, llr8=l8), 1),
      "c2": (lambda l8: DlConfig(50, 150, 1, 9912, cfi=3, llr8=l8), 4)}
UL = {"short": lambda: UlConfig(15, 11, 1, 328, 3, 12, n_dmrs=3, cyclic_shift=2, delta_ss=5),
      "win1": lambda: UlConfig(25, 11, 2, 4008, 10, 5, n_dmrs=3, cyclic_shift=2, delta_ss=5)}
NSF = 2


@pytest.fixture(scope="module")
def hp():
    return importlib.import_module("srslte-emane_amd")


def _dl_rx(hp, cfg, nsf=NSF):
    hc = hp.ChestDlCfg()
    hc.filter_coef[0], hc.filter_coef[1] = 4.0, 1.0
    return hp.DlRx(cfg.cell_id, cfg.nof_prb, cfg.cfi, cfg.rnti, cfg.mod, cfg.tbs, 6, nsf, True, hc, llr_8bit=cfg.llr8, cp_ext=cfg.cp_ext)


def _ul_rx(hp, cfg, nsf=NSF):
    return hp.UlRx(cfg.cell_id, cfg.nof_prb, cfg.rnti, cfg.mod, cfg.tbs, cfg.L_prb, cfg.n_prb, 3, 6, nsf, 2, 5)


def _dl_iq(cfg, tti0, seed, rv=0, data=None, nsf=NSF):
    rng = np.random.default_rng(seed)
    iq, dat = zip(*[make_subframe(cfg, tti0 + b, rng, amp=AMP, rv=rv, data=None if data is None else data[b]) for b in range(nsf)])
    return np.stack(iq), list(dat)


def _ul_iq(cfg, tti0, seed, rv=0, data=None, nsf=NSF):
    rng = np.random.default_rng(seed)
    iq, dat = zip(*[make_ul_subframe(cfg, tti0 + b, rng, amp=AMP, rv=rv, data=None if data is None else data[b]) for b in range(nsf)])
    return np.stack(iq), list(dat)


def _sent(tb, ok, data, tbs):
    assert ok.all(), ok
    for b, d in enumerate(data):
        assert np.array_equal(tb[b][:tbs // 8], d), b


@pytest.mark.parametrize("name,llr8", [("short", False), ("short", True), ("win1", False), ("win1", True), ("c2", False)])
def test_dl_back_end_branches(hp, name, llr8):
    mk, tti0 = DL[name]
    cfg = mk(llr8)
    assert (cfg.seg.C, cfg.seg.K1) == {"short": (1, 352), "win1": (1, 832), "c2": (2, 4992)}[name]
    iq, data = _dl_iq(cfg, tti0, 11)
    rx = _dl_rx(hp, cfg)
    tb, ok = rx.decode(iq, tti0)
    _sent(tb, ok, data, cfg.tbs)
    assert (rx.debug(6, np.uint32, NSF * cfg.seg.C) == 1).all() and rx.debug(7, np.uint8, NSF * cfg.seg.C).all()
    assert rx.parity_compact() == (name != "short" and not llr8)  # K % 64 == 0, the 16-window 16-bit decoder, few enough LLRs per block
    rx.free()


@pytest.mark.parametrize("name", ["short", "win1"])
def test_ul_back_end_branches(hp, name):
    cfg = UL[name]()
    assert (cfg.seg.C, cfg.seg.K1) == {"short": (1, 352), "win1": (1, 4032)}[name]
    iq, data = _ul_iq(cfg, 4, 12)
    rx = _ul_rx(hp, cfg)
    tb, ok = rx.decode(iq, 4)
    _sent(tb, ok, data, cfg.tbs)
    assert (rx.debug(6, np.uint32, NSF * cfg.seg.C) == 1).all() and rx.debug(7, np.uint8, NSF * cfg.seg.C).all()
    rx.free()


HARQ_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p)


def _refused(hp, fn, rx, din, nof_sf, rv):
    fn = HARQ_FN(C.cast(fn, C.c_void_p).value)  # a prototype of this test's own: the library object's stays as the wrappers declared it
    assert fn(rx.h, din.ptr, 4, nof_sf, rv, 1, rx.d_tb.ptr, rx.tb_stride, rx.d_ok.ptr, None) == hp.SRSLTE_ERROR_INVALID_INPUTS, (nof_sf, rv)


def _grid_call(hp, rx, grid, tti0, rows):
    """srslte_hip_dl_rx_grid_batch on [nof_sf][...] grids -> (tb rows, ok) of `rows` transport-block rows"""
    x = np.ascontiguousarray(grid, np.complex64)
    din = hp.DevBuf.from_host(x)
    assert hp.lib().srslte_hip_dl_rx_grid_batch(rx.h, din.ptr, tti0, x.shape[0], rx.d_tb.ptr, rx.tb_stride, rx.d_ok.ptr, None) == hp.SRSLTE_SUCCESS
    hp.sync()
    return rx.d_tb.to_host(np.uint8).reshape(-1, rx.tb_stride)[:rows], rx.d_ok.to_host(np.uint8)[:rows]


def _grid_rows(r, kind, cfg):
    """the rows of _grid_call in the order of a decode() result"""
    tb, ok = r
    if kind == "dl2":
        return [tb[:NSF, :328 // 8 + 3], tb[NSF:, :328 // 8 + 3], ok[:NSF], ok[NSF:]]
    return [tb[:, :cfg.tbs // 8 + 3], ok]


def _same(a, b, what):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x, y), what


@pytest.mark.parametrize("kind", ["dl", "ul", "dl2"])
def test_calls_carry_no_state(hp, kind):
    """decode(x); a retransmission of other data; the grid entry point on x's grids; two refused calls; decode(x) again. The last call gives what
    the first gave and what a fresh object gives - bytes, flags, pass counts, and the layout the rate de-matcher chose: nothing of the HARQ call,
    the caller's grids or the refused arguments stays in the object."""
    tti0 = 1 if kind == "dl" else 4
    L = hp.lib()
    if kind == "dl":  # win1: the compact parity layout is part of what a call chooses
        cfg = DL["win1"][0](False)
        mk = lambda: _dl_rx(hp, cfg)
        x, data = _dl_iq(cfg, tti0, 21)
        y, _ = _dl_iq(cfg, tti0, 22, rv=2)
        nC, glen = cfg.seg.C, 12 * 12 * cfg.nof_prb
    elif kind == "ul":
        cfg = UL["win1"]()
        mk = lambda: _ul_rx(hp, cfg)
        x, data = _ul_iq(cfg, tti0, 21)
        y, _ = _ul_iq(cfg, tti0, 22, rv=1)
        nC = cfg.seg.C
    else:  # the smallest two-codeword case of test_gpu_mimo: 6 PRB, CDD, QPSK / QPSK, TBS 328 / 328
        cfg = DlConfig(6, 1, 1, 328, cfi=3, nof_rx=2, nof_ports=2, tx_scheme="cdd", pmi=0, mod2=1, tbs2=328)
        hc = hp.ChestDlCfg()
        hc.filter_coef[0], hc.filter_coef[1] = 4.0, 1.0
        mk = lambda: hp.DlRx(1, 6, 3, 0x1234, 1, 328, 6, NSF, True, hc, nof_rx=2, nof_ports=2, tx_scheme=3, pmi=0, mod2=1, tbs2=328)
        rng = np.random.default_rng(21)
        x, data = zip(*[make_subframe_mimo(cfg, tti0 + b, rng, amp=0.2) for b in range(NSF)])
        y = np.stack([make_subframe_mimo(cfg, tti0 + b, rng, amp=0.2, rv=(2, 0))[0] for b in range(NSF)])
        x, nC, glen = np.stack(x), 1, 2 * 14 * 12 * 6

    def state(rx):
        its = [rx.debug(100 * c + 6, np.uint32, NSF * nC) for c in range(2 if kind == "dl2" else 1)]
        return its + ([rx.parity_compact()] if kind != "ul" else [])

    def flat(r):  # (tb, ok), each a list per codeword on the two-codeword object
        return list(r[0]) + list(r[1]) if kind == "dl2" else [r[0], r[1]]

    rx, fresh = mk(), mk()
    first = flat(rx.decode(x, tti0)) + state(rx)
    if kind == "dl2":
        for cw in range(2):
            _sent(first[cw], first[2 + cw], [d[cw] for d in data], 328)
    else:
        _sent(first[0], first[1], data, cfg.tbs)
    din = hp.DevBuf.from_host(np.ascontiguousarray(x, np.complex64))
    if kind == "ul":
        rx.decode_harq(y, tti0, 1, False)
        for nof_sf, rv in ((NSF, 4), (NSF + 1, 0)):
            _refused(hp, L.srslte_hip_ul_rx_batch_harq, rx, din, nof_sf, rv)
    else:
        grid = rx.debug(0, np.complex64, NSF * glen).reshape(NSF, glen)  # the grids stage 0 made of x
        if kind == "dl":
            rx.decode_harq(y, tti0, 2, False)
            assert not rx.parity_compact()
        else:
            rx.decode_harq2(y, tti0, (2, 0), (False, True))
        _same(_grid_rows(_grid_call(hp, rx, grid, tti0, 2 * NSF if kind == "dl2" else NSF), kind, cfg), first[:4 if kind == "dl2" else 2], "grid")
        for nof_sf, rv in ((NSF, 4), (NSF + 1, 0)):
            _refused(hp, L.srslte_hip_dl_rx_batch_harq, rx, din, nof_sf, rv)
    last = flat(rx.decode(x, tti0)) + state(rx)
    _same(last, first, "first")
    _same(last, flat(fresh.decode(x, tti0)) + state(fresh), "fresh")
    rx.free()
    fresh.free()


def test_second_codeword_views(hp):
    """Debug views 100 + n are the second codeword's own buffers: symbols, LLRs, soft buffers, pass counts, block CRC flags, bytes; it has no
    grids or estimates of its own."""
    cfg = DlConfig(6, 1, 1, 328, cfi=3, nof_rx=2, nof_ports=2, tx_scheme="cdd", pmi=0, mod2=1, tbs2=328)
    hc = hp.ChestDlCfg()
    hc.filter_coef[0], hc.filter_coef[1] = 4.0, 1.0
    rx = hp.DlRx(1, 6, 3, 0x1234, 1, 328, 6, NSF, True, hc, nof_rx=2, nof_ports=2, tx_scheme=3, pmi=0, mod2=1, tbs2=328)
    rx.keep_symbols()
    rng = np.random.default_rng(31)
    iq, data = zip(*[make_subframe_mimo(cfg, 4 + b, rng, amp=0.2) for b in range(NSF)])
    tb, ok = rx.decode(np.stack(iq), 4)
    for cw in range(2):
        _sent(tb[cw], ok[cw], [d[cw] for d in data], 328)
    view = hp.lib().srslte_hip_dl_rx_debug_buffer
    ptrs = {n: view(rx.h, 100 + n) for n in range(9)}
    assert all(ptrs[n] for n in range(3, 9)), ptrs
    assert not ptrs[0] and not ptrs[1]
    assert len({ptrs[n] for n in range(3, 9)} | {view(rx.h, n) for n in range(3, 9)}) == 12  # its own, not the first codeword's
    flags = rx.debug(107, np.uint8, NSF * cfg.segs[1].C).reshape(NSF, -1)
    rows = rx.d_ok.to_host(np.uint8)[NSF:2 * NSF]  # rows nof_sf .. 2 nof_sf - 1 of tb_ok
    assert np.array_equal(flags.all(axis=1), rows != 0) and np.array_equal(rows, ok[1])
    rx.free()


@pytest.mark.parametrize("direction", ["dl", "ul"])
def test_tx_rv_tables_on_first_use(hp, direction):
    """Redundancy versions 0, 2, 0, 3, 2 on one transmit object: every output equals, byte for byte, that of a fresh object asked for that rv
    alone - a table made on first use is the table of its rv, and making one leaves the others alone."""
    mk = (lambda: hp.DlTx(1, 6, 3, 0x1234, 1, 328, NSF)) if direction == "dl" else (lambda: hp.UlTx(11, 15, 0x1234, 1, 328, 3, 12, 3, NSF, 2, 5))
    data = np.random.default_rng(41).integers(0, 256, (NSF, 328 // 8), dtype=np.uint8)
    alone = {}
    for rv in (0, 2, 3):
        tx = mk()
        alone[rv] = tx.encode(data, 4, rv=rv).copy()
        tx.free()
    assert not np.array_equal(alone[0], alone[2]) and not np.array_equal(alone[2], alone[3])
    tx = mk()
    for rv in (0, 2, 0, 3, 2):
        assert np.array_equal(tx.encode(data, 4, rv=rv).view(np.uint8), alone[rv].view(np.uint8)), rv
    tx.free()
