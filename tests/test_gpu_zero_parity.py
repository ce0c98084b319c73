"""The verdict `par_rx == par_tx && par_rx` (sch.c:482) at every place the library implements it: a transport block whose CRC24A is zero is
reported as failed although every code-block CRC passes and the bytes are those that were sent. Both constructions of such a block
(silent_cases.zero_parity_payload: all zero; random bytes followed by their own CRC24A) go in one batch with a random payload of the same
shape: verdicts 0, 0, 1, bytes those sent, one pass per block, every block flag 1 - what the oracle says (test_silent_oracle.py records it,
and each row is checked against the oracle's back end on the row's own LLRs). Inputs are noise-free; nothing here has a tolerance.

The test ids name the verdict site the case is judged by (read from the code; the sites were not switched off one at a time):
  tb_crc_kernel            fixed-grant DL (16- and 8-bit) and UL, K = 352: the unwindowed decoder, whose bytes tb_crc_kernel assembles and judges
  tdec_pair_direct         fixed-grant DL, K = 832 and C = 2, K = 4992 with the compact parity layout: the direct assembly of tdec_pair_kernel;
                           -whole: the same shapes on an object created with SRSLTE_HIP_PARITY_COMPACT=0
  win8bit-sse8 / -avx8     fixed-grant DL with 8-bit LLRs at K = 832 / K = 4992: the 8-bit windowed bodies
  tb_asm_kernel-ul-K4032   the PUSCH receiver never assembles directly: its windowed block's verdict is tb_asm_kernel's
  pmch                     test_gpu_pmch's 6-PRB case
  harq-*                   srslte_hip_*_rx_batch_harq: rv 0 new data is judged as the same shape above (K352: tb_crc_kernel, K832 / C2: the
                           direct assembly, UL: tb_asm_kernel); rv 2 with new_data = 0 decodes nothing, and the verdict is 0 for every row -
                           the random one too, by the no-block-decoded rule, so this call does not tell the parity term apart
  two_codewords            test_gpu_sch_fixed's 6-PRB CDD object: codeword 0 zero-parity beside a random codeword 1, then swapped
  grants-dl / grants-ul    a ragged batch, one grant per subframe, the zero-parity payload in each position in turn: K = 352 (generic body of
                           the mixed launch), K = 800 (8-window body: its one-block verdict `ok && par_nz`), K = 832 / 4032 and two blocks
                           (pair body, tdec_tb_fold); -bytes: SRSLTE_HIP_GRANTS_TB_DIRECT=0, the fallback tb_crc_bytes_kernel
  tdec_tb_stored_block     grants mode, a retransmission of a two-block transport block one of whose blocks passed earlier
  dlsch_decode2            compat.cpp / sch_host.inc: srslte_dlsch_decode2 through test_gpu_sch_host.py's harness, one and two blocks
The library exports no srslte_ulsch_decode (its PUSCH receiver is srslte_hip_ul_rx_*), so there is no such case."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

from _libs import OrcSchCfg, oracle, p, ref
from lte_sim import DlConfig, PmchConfig, make_subframe, make_subframe_mimo, make_ul_subframe, oracle_rx, oracle_ul_rx
from silent_cases import (DL_CK, DL_SHAPES, UL_CK, UL_SHAPES, DlPipe, UlPipe, blur_symbols, check_against_oracle, crc24a, dl_grants_views,
                          dl_ragged_cfgs, random_payload, row_of, ul_ragged_cfgs, zero_parity_payload)

pytestmark = pytest.mark.gpu
HOWS = ("zeros", "crc", "random")


@pytest.fixture(scope="module")
def hp():
    return importlib.import_module("srslte-emane_amd")


def _payloads(tbs, rng, hows=HOWS):
    return [random_payload(tbs, rng) if h == "random" else zero_parity_payload(tbs, h, rng) for h in hows]


def _pipe(hp, site):
    if site == "pmch":
        cfg = PmchConfig(6, 1, 1, 1, 488, cfi=2, non_mbsfn_region=2, nof_rx=1, cp_ext=True)
        cfg.Qm_sch = cfg.Qm
        return DlPipe(hp, cfg, 1, pmch=True), True, (1, 512)
    kind, name, llr8, compact = {"tb_crc_kernel-dl": ("dl", "K352", False, True), "tb_crc_kernel-dl8": ("dl", "K352", True, True),
                                 "tb_crc_kernel-ul": ("ul", "K352", False, True),
                                 "tdec_pair_direct-K832": ("dl", "K832", False, True), "tdec_pair_direct-C2": ("dl", "C2", False, True),
                                 "tdec_pair_direct-K832-whole": ("dl", "K832", False, False), "tdec_pair_direct-C2-whole": ("dl", "C2", False, False),
                                 "win8bit-sse8-K832": ("dl", "K832", True, True), "win8bit-avx8-K4992": ("dl", "C2", True, True),
                                 "tb_asm_kernel-ul-K4032": ("ul", "K4032", False, True)}[site]
    if kind == "ul":
        return UlPipe(hp, UL_SHAPES[name](), 4), compact, UL_CK[name]
    mk, tti0 = DL_SHAPES[name]
    return DlPipe(hp, mk(llr8=llr8), tti0), compact, DL_CK[name]


FIXED = ["tb_crc_kernel-dl", "tb_crc_kernel-dl8", "tb_crc_kernel-ul", "tdec_pair_direct-K832", "tdec_pair_direct-C2", "tdec_pair_direct-K832-whole",
         "tdec_pair_direct-C2-whole", "win8bit-sse8-K832", "win8bit-avx8-K4992", "tb_asm_kernel-ul-K4032", "pmch"]


def _expect(P, rows, data):
    for b, (how, d) in enumerate(zip(HOWS, data)):
        tb, ok, it, cb = rows[b][0], rows[b][1][0], rows[b][5], rows[b][6]
        assert ok == (1 if how == "random" else 0), (how, ok)
        assert np.array_equal(tb[:len(d)], d), how
        assert tb[len(d):len(d) + 3].any() == (how == "random"), (how, tb[len(d):len(d) + 3])
        assert (it == 1).all() and cb.all(), (how, it, cb)


@pytest.mark.parametrize("site", FIXED)
def test_fixed_grant_verdict(hp, site):
    P, compact, ck = _pipe(hp, site)
    assert (P.C, P.K) == ck
    rng = np.random.default_rng(len(site))
    data = _payloads(P.cfg.tbs, rng)
    iq = np.stack([P.live(P.tti0 + b, rng, data=d)[0] for b, d in enumerate(data)])
    rx = P.rx(3, compact=compact)
    res = P.decode(rx, iq, P.tti0)
    if site.startswith("tdec_pair_direct"):
        assert rx.parity_compact() == compact
    rows = [row_of(P, rx, res, b, 3, P.tti0) for b in range(3)]
    _expect(P, rows, data)
    for b in range(3):
        check_against_oracle(P, rows[b], P.tti0 + b, P.new_harq(), what=(site, HOWS[b]))
    rx.free()


@pytest.mark.parametrize("site", ["harq-K352", "harq-K832", "harq-C2", "harq-ul-K4032"])
def test_harq_entry_point_verdict(hp, site):
    name = site.split("-")[-1]
    P = UlPipe(hp, UL_SHAPES[name](), 4) if "-ul-" in site else DlPipe(hp, DL_SHAPES[name][0](), DL_SHAPES[name][1])
    rng = np.random.default_rng(len(site))
    data = _payloads(P.cfg.tbs, rng)
    rx = P.rx(3)
    h = [P.new_harq() for _ in range(3)]
    for rv, new, t0 in ((0, True, P.tti0), (2, False, P.tti0 + 10)):
        iq = np.stack([P.live(t0 + b, rng, rv=rv, data=d)[0] for b, d in enumerate(data)])
        res = P.decode_harq(rx, iq, t0, rv, new)
        rows = [row_of(P, rx, res, b, 3, t0) for b in range(3)]
        if rv == 0:
            _expect(P, rows, data)
        else:  # nothing is decoded again, every flag stays, and every verdict is 0: also the random block's, whose retransmission is a
            # duplicate the MAC would not ask for (upstream's answer to it, sch.c:392-414,:482, as the oracle has it)
            for b in range(3):
                assert rows[b][1][0] == 0 and (rows[b][5] == 0).all() and rows[b][6].all(), (site, b, rows[b][1], rows[b][5], rows[b][6])
        for b in range(3):
            check_against_oracle(P, rows[b], t0 + b, h[b], rv, new, what=(site, rv, HOWS[b]))
    rx.free()


def test_two_codewords(hp):
    """rows: (codeword 0, codeword 1) = (zeros, random), (crc, random), then swapped: the two verdict rows are independent"""
    cfg = DlConfig(6, 1, 1, 328, cfi=3, nof_rx=2, nof_ports=2, tx_scheme="cdd", pmi=0, mod2=1, tbs2=328)
    hc = hp.ChestDlCfg()
    hc.filter_coef[0], hc.filter_coef[1] = 4.0, 1.0
    rx = hp.DlRx(1, 6, 3, 0x1234, 1, 328, 6, 2, True, hc, nof_rx=2, nof_ports=2, tx_scheme=3, pmi=0, mod2=1, tbs2=328)
    rng = np.random.default_rng(3)
    for swap in (False, True):
        z = _payloads(328, rng, ("zeros", "crc"))
        r = [random_payload(328, rng) for _ in range(2)]
        data = [[r[b], z[b]] if swap else [z[b], r[b]] for b in range(2)]
        iq = np.stack([make_subframe_mimo(cfg, 4 + b, rng, amp=0.2, data=data[b])[0] for b in range(2)])
        tb, ok = rx.decode(iq, 4)
        zc, rc = (1, 0) if swap else (0, 1)
        assert not ok[zc].any() and ok[rc].all(), (swap, ok)
        for cw in range(2):
            for b in range(2):
                assert np.array_equal(tb[cw][b][:41], data[b][cw]), (swap, cw, b)
                assert tb[cw][b][41:44].any() == (cw == rc), (swap, cw, b)
            assert (rx.debug(100 * cw + 6, np.uint32, 2) == 1).all() and rx.debug(100 * cw + 7, np.uint8, 2).all(), (swap, cw)
    rx.free()


class _Env:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = os.environ.pop(self.name, None)
        if self.value is not None:
            os.environ[self.name] = self.value

    def __exit__(self, *a):
        os.environ.pop(self.name, None)
        if self.old is not None:
            os.environ[self.name] = self.old


@pytest.mark.parametrize("site", ["grants-dl", "grants-dl-bytes", "grants-dl8"])
def test_dl_grants_verdict(hp, site):
    """silent_cases.DL_RAGGED (50 PRB, CFI 3, QPSK): K = 352 on 3 PRBs (the generic body of the mixed launch), K = 832 on 7 PRBs (the pair
    body), C = 2, K = 4992 on the full band, K = 800 on 6 PRBs (the 8-window body, whose one-block verdict is tdec.hip's `ok && par_nz`), one
    per subframe; the zero-parity payload (the two constructions in turn) in each position."""
    llr8 = site.endswith("8")
    cfgs = dl_ragged_cfgs(llr8)
    n = len(cfgs)
    hc = hp.ChestDlCfg()
    hc.filter_coef[0], hc.filter_coef[1] = 4.0, 1.0
    rng = np.random.default_rng(len(site))
    with _Env("SRSLTE_HIP_GRANTS_TB_DIRECT", "0" if site.endswith("bytes") else None):  # read when the grants mode is set up
        rx = hp.DlRx(150, 50, 3, 0, 1, max(c.tbs for c in cfgs), 6, n, True, hc, llr_8bit=llr8)
        grants = [hp.DlGrant.make(50, 1, c.tbs, c.rnti, cfi=3, prb_mask=c.prb_mask) for c in cfgs]
        for pos in range(n):
            for how in ("zeros", "crc"):
                data = [zero_parity_payload(c.tbs, how, rng) if b == pos else random_payload(c.tbs, rng) for b, c in enumerate(cfgs)]
                iq = np.stack([make_subframe(c, 4 + b, rng, amp=0.1, data=data[b])[0] for b, c in enumerate(cfgs)])
                rc, tb, ok = rx.decode_grants(iq, 4, grants)
                assert rc == 0 and ok.tolist() == [0 if b == pos else 1 for b in range(n)], (pos, how, ok)
                it, cb = rx.debug(13, np.uint32, n * 2).reshape(n, 2), rx.debug(14, np.uint8, n * 2).reshape(n, 2)
                for b, c in enumerate(cfgs):
                    nb = c.tbs // 8
                    assert np.array_equal(tb[b][:nb], data[b]) and tb[b][nb:nb + 3].any() == (b != pos), (pos, how, b)
                    assert (it[b, :c.seg.C] == 1).all() and cb[b, :c.seg.C].all(), (pos, how, b, it, cb)
                    r = oracle_rx(c, iq[b], 4 + b)
                    assert bool(ok[b]) == r["ok"] and np.array_equal(tb[b][:nb + 3], r["tb"]), (pos, how, b)
        rx.free()


def test_ul_grants_verdict(hp):
    """silent_cases.UL_RAGGED (25 PRB): K = 352, K = 4032 (16QAM), C = 2 x K = 4032 (64QAM), K = 800 (the 8-window body), one PUSCH per
    subframe; the zero-parity payload in each position."""
    cfgs = ul_ragged_cfgs()
    n = len(cfgs)
    grants = [hp.UlGrant.make(b, c.rnti, c.L_prb, c.n_prb, c.mod, c.tbs, n_dmrs=c.n_dmrs) for b, c in enumerate(cfgs)]
    rx = hp.UlRx(11, 25, 0x1234, 1, 7992, 6, 0, 0, 6, n, 2, 5, True, False, max_grants=n)
    rng = np.random.default_rng(8)
    for pos in range(n):
        for how in ("zeros", "crc"):
            data = [zero_parity_payload(c.tbs, how, rng) if b == pos else random_payload(c.tbs, rng) for b, c in enumerate(cfgs)]
            iq = np.stack([make_ul_subframe(c, 7 + b, rng, amp=0.1, data=data[b])[0] for b, c in enumerate(cfgs)])
            tb, ok = rx.decode_grants(iq, 7, grants)
            assert ok.tolist() == [0 if b == pos else 1 for b in range(n)], (pos, how, ok)
            it = rx.debug(23, np.uint32, n * 2).reshape(n, 2)
            for b, c in enumerate(cfgs):
                nb = c.tbs // 8
                assert np.array_equal(tb[b][:nb], data[b]) and tb[b][nb:nb + 3].any() == (b != pos), (pos, how, b)
                assert (it[b, :c.seg.C] == 1).all(), (pos, how, b, it)
                r = oracle_ul_rx(c, iq[b], 7 + b)
                assert bool(ok[b]) == r["ok"] and np.array_equal(tb[b][:nb + 3], r["tb"]), (pos, how, b)
    rx.free()


@pytest.mark.parametrize("site", ["tdec_tb_stored_block", "tdec_tb_stored_block-bytes"])
def test_grants_harq_verdict_with_a_stored_block(hp, site):
    """tdec_tb_stored_block (tdec.hip): in the grants mode a retransmission whose transport block has a block that passed earlier folds that
    block's kept bytes into the verdict. Three subframes, each a two-block grant (C = 2, K = 4992): the payloads are two zero-parity blocks
    (random bytes + their CRC24A, two draws) and a random one. rv 0: the OFDM symbols that carry most of block 0 are blurred with another
    payload's (silent_cases.blur_symbols), so block 0 fails and block 1 passes. rv 2, new_data = 0, clean: block 0 is decoded on top of what
    rv 0 left, block 1 is skipped as stored - verdicts 0, 0, 1 and the bytes those sent. Every call is also judged by the oracle's back
    end with its soft buffer on the device's own LLRs. -bytes: SRSLTE_HIP_GRANTS_TB_DIRECT=0, where tb_crc_bytes_kernel judges instead."""
    cfg = dl_ragged_cfgs()[2]
    cfgs = [DlConfig(50, 150, 1, cfg.tbs, cfi=3, rnti=0x100 + b) for b in range(3)]
    pipes = [DlPipe(None, c, 4) for c in cfgs]
    hc = hp.ChestDlCfg()
    hc.filter_coef[0], hc.filter_coef[1] = 4.0, 1.0
    rng = np.random.default_rng(12)
    data = [zero_parity_payload(cfg.tbs, "crc", rng), zero_parity_payload(cfg.tbs, "crc", rng), random_payload(cfg.tbs, rng)]
    with _Env("SRSLTE_HIP_GRANTS_TB_DIRECT", "0" if site.endswith("bytes") else None):
        rx = hp.DlRx(150, 50, 3, 0, 1, cfg.tbs, 6, 3, True, hc)
        h = [P.new_harq() for P in pipes]
        for rv, new, t0 in ((0, True, 4), (2, False, 14)):
            iq = [make_subframe(c, t0 + b, rng, amp=0.1, rv=rv, data=data[b])[0] for b, c in enumerate(cfgs)]
            if rv == 0:  # symbols 3 .. 6 hold 2200 of block 0's 3150 REs
                iq = [blur_symbols(c, x, make_subframe(c, t0 + b, rng, amp=0.1, data=random_payload(c.tbs, rng))[0], (3, 4, 5, 6)) for b, (c, x) in enumerate(zip(cfgs, iq))]
            grants = [hp.DlGrant.make(50, 1, c.tbs, c.rnti, cfi=3, rv=rv, new_data=new) for c in cfgs]
            rc, tb, ok = rx.decode_grants(np.stack(iq), t0, grants)
            assert rc == 0
            views = dl_grants_views(rx, cfgs, t0)
            for b, P in enumerate(pipes):
                row = [tb[b][:cfg.tbs // 8 + 3].copy(), ok[b:b + 1].copy()] + views[b]
                o_ok, it, cb = check_against_oracle(P, row, t0 + b, h[b], rv, new, what=(site, rv, b))
                if rv == 0:
                    assert not o_ok and it[0] == 6 and it[1] == 1 and cb.tolist() == [0, 1], (b, it, cb)
                else:
                    assert it[0] >= 1 and it[1] == 0 and cb.all(), (b, it, cb)
                    assert ok[b] == (1 if b == 2 else 0), (site, b, ok)
                    assert np.array_equal(tb[b][:cfg.tbs // 8], data[b]) and tb[b][cfg.tbs // 8:cfg.tbs // 8 + 3].any() == (b == 2), (site, b)
        rx.free()


def _own_side(Side, prb, tbs, nbits, llr8):
    """test_gpu_sch_host's Side for this library, set up without the reference's srslte_crc_init / srslte_softbuffer_rx_init: the CRC tables
    from _libs.make_crc, a zeroed srslte_softbuffer_rx_t built here (softbuffer.h:37-43: max_cb, buffer_f, data, cb_crc, tb_crc)."""
    from _libs import hip, make_crc, opaque
    from test_gpu_sch_host import layout
    Ly, H = layout(), hip()
    s = Side.__new__(Side)
    s.mine, s.R, s.H, s.Ly = True, None, H, Ly
    s.q = opaque(Ly["srslte_sch_t"] + 256)
    assert H.srslte_tdec_init(C.c_void_p(C.addressof(s.q) + Ly["srslte_sch_t.decoder"]), 6144) == 0
    for field, poly in (("crc_tb", 0x1864CFB), ("crc_cb", 0x1800063)):
        h = make_crc(poly, 24)
        C.memmove(C.addressof(s.q) + Ly["srslte_sch_t." + field], C.addressof(h), C.sizeof(h))
    qb = np.frombuffer(s.q, np.uint8)
    qb[Ly["srslte_sch_t.max_iterations"]:Ly["srslte_sch_t.max_iterations"] + 4].view(np.uint32)[0] = 4
    qb[Ly["srslte_sch_t.llr_is_8bit"]] = 1 if llr8 else 0
    ncb = 32
    s.keep = [np.zeros((ncb, 18600), np.int16), np.zeros((ncb, 768), np.uint8), np.zeros(ncb, np.uint8)]
    s.keep += [np.array([s.keep[0][c].ctypes.data for c in range(ncb)], np.uint64), np.array([s.keep[1][c].ctypes.data for c in range(ncb)], np.uint64)]
    s.sb = opaque(Ly["srslte_softbuffer_rx_t"] + 64)
    sbb = np.frombuffer(s.sb, np.uint8)
    sbb[Ly["srslte_softbuffer_rx_t.max_cb"]:][:4].view(np.uint32)[0] = ncb
    for field, arr in (("buffer_f", s.keep[3]), ("data", s.keep[4]), ("cb_crc", s.keep[2])):
        sbb[Ly["srslte_softbuffer_rx_t." + field]:][:8].view(np.uint64)[0] = arr.ctypes.data
    s.cfg = opaque(Ly["srslte_pdsch_cfg_t"] + 64)
    g = np.frombuffer(s.cfg, np.uint8)
    tb0 = Ly["srslte_pdsch_cfg_t.grant"] + Ly["srslte_pdsch_grant_t.tb"]
    for fld, v in (("mod", 1), ("tbs", tbs), ("rv", 0), ("nof_bits", nbits), ("cw_idx", 0)):
        g[tb0 + Ly["srslte_ra_tb_t." + fld]:][:4].view(np.uint32)[0] = v
    g[tb0 + Ly["srslte_ra_tb_t.enabled"]] = 1
    s.tb0, s.g = tb0, g
    g[Ly["srslte_pdsch_cfg_t.softbuffers"]:][:8].view(np.uint64)[0] = C.addressof(s.sb)
    return s


@pytest.mark.parametrize("prb,tbs,nre,llr8", [(6, 328, 684, False), (50, 9912, 6300, False), (50, 9912, 6300, True)])
def test_dlsch_decode2_verdict(prb, tbs, nre, llr8):
    """srslte_dlsch_decode2 of the library on clean LLRs: SRSLTE_ERROR for both zero-parity blocks, SRSLTE_SUCCESS for the random one, the bytes
    those sent, every block's CRC flag set in the soft buffer - on objects set up here (_own_side: needs no reference build), on the harness's
    own, and beside the reference's srslte_dlsch_decode2 where oracle/_ref is built."""
    from test_gpu_sch_host import Side, hip_seg
    orc, rng = oracle(), np.random.default_rng(tbs)
    nbits = nre * 2
    K, C_ = hip_seg(tbs)
    for how, data in zip(HOWS, _payloads(tbs, rng)):
        assert (crc24a(data, tbs) == 0) == (how != "random")
        sch = OrcSchCfg(tbs, nbits, 2, 0, 4)
        bits = np.zeros(nbits, np.uint8)
        assert orc.orc_dlsch_encode(C.byref(sch), p(data), p(bits)) == 0
        e = ((2 * bits.astype(np.int16) - 1) * (20 if llr8 else 100)).astype(np.int8 if llr8 else np.int16)
        for mine in (None, True, False) if ref() is not None else (None,):
            s = _own_side(Side, prb, tbs, nbits, llr8) if mine is None else Side(mine, prb, tbs, 1, nbits, llr8, 4)
            s.set(0, 1)
            out = np.zeros(tbs // 8 + 64, np.uint8)
            rc = s.decode(e.copy(), out, 1)
            assert rc == (0 if how == "random" else -1), (how, mine, rc)
            assert np.array_equal(out[:tbs // 8], data) and out[tbs // 8:tbs // 8 + 3].any() == (how == "random"), (how, mine)
            assert s.soft(C_, 16)[0].all(), (how, mine)
