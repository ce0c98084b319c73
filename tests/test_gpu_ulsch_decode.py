"""srslte_ulsch_decode served by the library (one device call per PUSCH transport block, include/srslte_hip/srslte_compat.h) against the
reference's own srslte_ulsch_decode (oracle/_ref/libsrslte_ref.so, sch.c:991-1066) on the same descrambled LLRs and the same c_seq.

Inputs are made with the reference's own functions as pusch.c:366-403 and :482-499 use them: srslte_ulsch_encode, the PUSCH Gold sequence,
scrambling, the placeholder / repetition bits, the modulator, AWGN from a seeded numpy generator, srslte_demod_soft_demodulate_s, descrambling.
Compared, all exactly: the return code, data with its three CRC bytes and a guard behind them, every field of uci_data the function writes
(scheduling_request untouched), cfg->K_segm and rank_is_not_one, avg_iterations, the whole srslte_softbuffer_rx_t, and the de-interleaved
stream g (srslte_hip_ulsch_debug_g against the reference's g_bits over nof_bits).

Noise: sigma is the standard deviation per real dimension of the unit-power constellation. CLEAN = 0.02 is error-free for every shape. The
failing level of each shape was chosen on the CPU with the reference alone (the smallest of 0.05, 0.10, 0.15 .. 0.95 at which a block fails at rv 0 while
the sequence rv 0, 2, 3, 1 on one soft buffer still recovers the block by the last transmission); the test checks both properties again, with
the reference alone, before it compares. Struct layouts are ctypes mirrors of this repository's compat header, which tests/test_ulsch_host.py
holds against the reference's.

The error-free channel gives large LLRs, and the reports of 6prb_64qam and the tbs = 0 cases are repeated until the reference's int16 sums
wrap: its int16 quantiser in front of the Viterbi decoder and its 16-lane int16 correlation then decide, and the library follows both."""
import ctypes as C
import os

import numpy as np
import pytest

from _libs import ROOT, hip, opaque, p, ref, struct_layout

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(ref() is None, reason="oracle/_ref/libsrslte_ref.so not built")]
QPSK, QAM16, QAM64 = 1, 2, 3
WIDEBAND, SUBBAND_HL = 0, 3
CLEAN, GUARD, FILL = 0.02, 64, 0xA5
_cache = {}


class RaTb(C.Structure):
    _fields_ = [("mod", C.c_int), ("tbs", C.c_int), ("rv", C.c_int), ("nof_bits", C.c_uint32), ("cw_idx", C.c_uint32), ("enabled", C.c_bool), ("mcs_idx", C.c_uint32)]


class Grant(C.Structure):
    _fields_ = [("is_from_rar", C.c_bool), ("L_prb", C.c_uint32), ("n_prb", C.c_uint32 * 2), ("n_prb_tilde", C.c_uint32 * 2), ("freq_hopping", C.c_uint32),
                ("nof_re", C.c_uint32), ("nof_symb", C.c_uint32), ("tb", RaTb), ("last_tb", RaTb), ("n_dmrs", C.c_uint32)]


class CqiCfg(C.Structure):
    _fields_ = [("data_enable", C.c_bool), ("ri_present", C.c_bool), ("pmi_present", C.c_bool), ("four_antenna_ports", C.c_bool), ("rank_is_not_one", C.c_bool),
                ("subband_label_2_bits", C.c_bool), ("L", C.c_uint32), ("N", C.c_uint32), ("type", C.c_int), ("ri_len", C.c_uint32)]


class AckCfg(C.Structure):
    _fields_ = [("pending_tb", C.c_bool * 2), ("nof_acks", C.c_uint32), ("ncce", C.c_uint32 * 9), ("N_bundle", C.c_uint32), ("tdd_ack_M", C.c_uint32),
                ("tdd_ack_m", C.c_uint32), ("tdd_is_multiplex", C.c_bool), ("tpc_for_pucch", C.c_uint32), ("grant_cc_idx", C.c_uint32)]


class UciCfg(C.Structure):
    _fields_ = [("ack", AckCfg * 5), ("cqi", CqiCfg), ("is_scheduling_request_tti", C.c_bool)]


class Offsets(C.Structure):
    _fields_ = [("I_offset_cqi", C.c_uint32), ("I_offset_ri", C.c_uint32), ("I_offset_ack", C.c_uint32)]


class PuschCfg(C.Structure):
    _fields_ = [("rnti", C.c_uint16), ("uci_cfg", UciCfg), ("uci_offset", Offsets), ("grant", Grant), ("max_nof_iterations", C.c_uint32), ("last_O_cqi", C.c_uint32),
                ("K_segm", C.c_uint32), ("current_tx_nb", C.c_uint32), ("csi_enable", C.c_bool), ("enable_64qam", C.c_bool), ("softbuffers", C.c_void_p),
                ("meas_time_en", C.c_bool), ("meas_time_value", C.c_uint32)]


class HlSubband(C.Structure):
    _fields_ = [("wideband_cqi_cw0", C.c_uint8), ("subband_diff_cqi_cw0", C.c_uint32), ("wideband_cqi_cw1", C.c_uint8), ("subband_diff_cqi_cw1", C.c_uint32),
                ("pmi", C.c_uint32)]


class Wideband(C.Structure):
    _fields_ = [("wideband_cqi", C.c_uint8), ("spatial_diff_cqi", C.c_uint8), ("pmi", C.c_uint8)]


class CqiUnion(C.Union):
    _fields_ = [("wideband", Wideband), ("subband_hl", HlSubband)]


class CqiValue(C.Structure):
    _anonymous_ = ("u",)
    _fields_ = [("u", CqiUnion), ("data_crc", C.c_bool)]


class AckValue(C.Structure):
    _fields_ = [("ack_value", C.c_uint8 * 10), ("valid", C.c_bool)]


class UciValue(C.Structure):
    _fields_ = [("scheduling_request", C.c_bool), ("cqi", CqiValue), ("ack", AckValue), ("ri", C.c_uint8)]


def layout():
    if not _cache:
        _cache.update(struct_layout({"srslte_sch_t": ["max_iterations", "avg_iterations", "llr_is_8bit", "ack_ri_bits", "decoder", "crc_tb", "crc_cb"],
                                     "srslte_softbuffer_rx_t": ["max_cb", "buffer_f", "data", "cb_crc", "tb_crc"], "srslte_pusch_cfg_t": ["softbuffers", "K_segm"],
                                     "srslte_uci_value_t": ["ri"], "srslte_cqi_value_t": ["data_crc"]}, ["srslte_hip/srslte_compat.h"], [os.path.join(ROOT, "include")]))
        Ly = _cache
        assert C.sizeof(PuschCfg) == Ly["srslte_pusch_cfg_t"] and PuschCfg.softbuffers.offset == Ly["srslte_pusch_cfg_t.softbuffers"] and PuschCfg.K_segm.offset == Ly["srslte_pusch_cfg_t.K_segm"]
        assert C.sizeof(UciValue) == Ly["srslte_uci_value_t"] and UciValue.ri.offset == Ly["srslte_uci_value_t.ri"] and CqiValue.data_crc.offset == Ly["srslte_cqi_value_t.data_crc"]
    return _cache


def seg(tbs):
    class Seg(C.Structure):
        _fields_ = [(n, C.c_uint32) for n in ("F", "C", "K1", "K2", "K1_idx", "K2_idx", "C1", "C2", "tbs")]
    s = Seg()
    assert hip().srslte_cbsegm(C.byref(s), tbs) == 0
    return s


class Shape:
    """one PUSCH: allocation, modulation, transport block and UCI configuration. ack: list of bits; ri: None or (ri_len, value);
    cqi: None, ("wb", value) - 4 bits - or ("hl", N, pmi_present, value): 4 + 2N bits per codeword"""

    def __init__(self, L_prb, mod, nsymb, tbs, ack=(), ri=None, cqi=None, I=(9, 6, 6)):
        self.L_prb, self.mod, self.nsymb, self.tbs, self.ack, self.ri, self.cqi, self.I = L_prb, mod, nsymb, tbs, list(ack), ri, cqi, I
        self.Qm = 2 * mod
        self.nof_re = 12 * L_prb * nsymb
        self.nbits = self.nof_re * self.Qm

    def cfg(self, rv, ri_for_rank=None):
        c = PuschCfg()
        c.rnti = 0x1234
        g = c.grant
        g.L_prb, g.nof_re, g.nof_symb = self.L_prb, self.nof_re, self.nsymb
        g.tb.mod, g.tb.tbs, g.tb.rv, g.tb.nof_bits, g.tb.enabled = self.mod, self.tbs, rv, self.nbits, True
        c.uci_offset.I_offset_ack, c.uci_offset.I_offset_ri, c.uci_offset.I_offset_cqi = self.I
        c.uci_cfg.ack[0].nof_acks = min(len(self.ack), 2)
        c.uci_cfg.ack[1].nof_acks = len(self.ack) - min(len(self.ack), 2)  # srslte_uci_cfg_total_ack sums the carriers
        q = c.uci_cfg.cqi
        if self.ri:
            q.ri_len = self.ri[0]
        if self.cqi:
            q.data_enable = True
            if self.cqi[0] == "wb":
                q.type = WIDEBAND
            else:
                q.type, q.N, q.pmi_present, q.ri_present = SUBBAND_HL, self.cqi[1], self.cqi[2], self.ri is not None
                if ri_for_rank is not None:  # the transmitter packs with the rank it reports
                    q.rank_is_not_one = ri_for_rank > 0
        c.enable_64qam = True
        return c

    def uci_tx(self):
        u = UciValue()
        for i, b in enumerate(self.ack):
            u.ack.ack_value[i] = b
        if self.ri:
            u.ri = self.ri[1]
        if self.cqi and self.cqi[0] == "wb":
            u.cqi.wideband.wideband_cqi = self.cqi[1]
        elif self.cqi:
            v = self.cqi[3]
            u.cqi.subband_hl.wideband_cqi_cw0, u.cqi.subband_hl.subband_diff_cqi_cw0 = v & 15, (v * 2654435761 >> 7) & ((1 << 2 * self.cqi[1]) - 1)
            u.cqi.subband_hl.wideband_cqi_cw1, u.cqi.subband_hl.subband_diff_cqi_cw1 = (v >> 4) & 15, (v * 40503 >> 3) & ((1 << 2 * self.cqi[1]) - 1)
            u.cqi.subband_hl.pmi = 1
        return u


def tx_side():
    if "tx" not in _cache:
        Ly, R = layout(), ref()
        q = opaque(Ly["srslte_sch_t"] + 256)
        assert R.srslte_sch_init(q) == 0
        sb = opaque(64)
        assert R.srslte_softbuffer_tx_init(sb, 100) == 0
        tabs = {}
        for mod in (QPSK, QAM16, QAM64):
            tabs[mod] = opaque(4096)
            assert R.srslte_modem_table_lte(tabs[mod], mod) == 0
            R.srslte_modem_table_bytes(tabs[mod])
        _cache["tx"] = (q, sb, tabs)
    return _cache["tx"]


def transmit(sh, rv, data, sigma, seed, tti=3, cell_id=1):
    """-> (descrambled int16 LLRs [nbits], c_seq [nbits]) of one transmission, made as pusch.c:366-403 and :482-499 do"""
    Ly, R = layout(), ref()
    q, sb, tabs = tx_side()
    if rv == 0:
        R.srslte_softbuffer_tx_reset(sb)
    cfg = sh.cfg(rv, sh.ri[1] if sh.ri else 0)
    cfg.softbuffers = C.addressof(sb)
    uci = sh.uci_tx()
    g, qb = np.zeros(sh.nbits // 8 + 64, np.uint8), np.zeros(sh.nbits // 8 + 64, np.uint8)
    R.srslte_ulsch_encode.argtypes = [C.c_void_p] * 6
    n_uci = R.srslte_ulsch_encode(q, C.byref(cfg), p(data), C.byref(uci), p(g), p(qb))
    assert n_uci >= 0, n_uci
    seq = opaque(64)
    assert R.srslte_sequence_pusch(seq, C.c_uint16(0x1234), 2 * (tti % 10), cell_id, sh.nbits) == 0
    R.srslte_scrambling_bytes(seq, p(qb), sh.nbits)
    pos = np.frombuffer(q, np.uint32, 2 * n_uci, Ly["srslte_sch_t.ack_ri_bits"]).reshape(n_uci, 2)
    for position, typ in pos.tolist():  # pusch.c:384-400
        if typ == 3:
            qb[position // 8] |= 1 << (7 - position % 8)
        elif typ == 2 and position > 1:
            bit = qb[(position - 1) // 8] & (1 << (7 - (position - 1) % 8))
            if bit:
                qb[position // 8] |= 1 << (7 - position % 8)
            else:
                qb[position // 8] &= 0xff ^ (1 << (7 - position % 8))
    d = np.zeros(sh.nof_re, np.complex64)
    R.srslte_mod_modulate_bytes(tabs[sh.mod], p(qb), p(d), sh.nbits)
    rng = np.random.default_rng(seed)
    d = (d + sigma * (rng.standard_normal(sh.nof_re) + 1j * rng.standard_normal(sh.nof_re))).astype(np.complex64)
    llr = np.zeros(sh.nbits + 64, np.int16)
    R.srslte_demod_soft_demodulate_s(sh.mod, p(d), p(llr), sh.nof_re)
    R.srslte_scrambling_s_offset(seq, p(llr), 0, sh.nbits)
    c_seq = np.ctypeslib.as_array((C.c_uint8 * sh.nbits).from_address(C.cast(seq, C.POINTER(C.c_void_p))[0])).copy()
    R.srslte_sequence_free(seq)
    return llr[:sh.nbits].copy(), c_seq


class Rx:
    """one srslte_sch_t + srslte_softbuffer_rx_t; `mine`: decoder object and srslte_ulsch_decode are this library's"""

    def __init__(self, mine, max_it=4):
        Ly, R, H = layout(), ref(), hip()
        self.mine, self.Ly = mine, Ly
        self.q = opaque(Ly["srslte_sch_t"] + 256)
        if mine:
            assert H.srslte_tdec_init(C.c_void_p(C.addressof(self.q) + Ly["srslte_sch_t.decoder"]), 6144) == 0
            assert R.srslte_crc_init(C.c_void_p(C.addressof(self.q) + Ly["srslte_sch_t.crc_tb"]), 0x1864CFB, 24) == 0
            assert R.srslte_crc_init(C.c_void_p(C.addressof(self.q) + Ly["srslte_sch_t.crc_cb"]), 0x1800063, 24) == 0
        else:
            assert R.srslte_sch_init(self.q) == 0
        self.qb = np.frombuffer(self.q, np.uint8)
        self.qb[Ly["srslte_sch_t.max_iterations"]:][:4].view(np.uint32)[0] = max_it
        self.sb = opaque(Ly["srslte_softbuffer_rx_t"] + 64)
        assert R.srslte_softbuffer_rx_init(self.sb, 100) == 0
        R.srslte_softbuffer_rx_reset(self.sb)

    def free(self):
        ref().srslte_softbuffer_rx_free(self.sb)
        if self.mine:
            hip().srslte_tdec_free(C.c_void_p(C.addressof(self.q) + self.Ly["srslte_sch_t.decoder"]))
        # the reference's object is left alone: srslte_sch_free frees the process-wide rate-matching tables (sch.c:150-151), which the
        # transmitter's srslte_sch_t of tx_side() goes on using

    def decode(self, sh, rv, llr, c_seq, uci_in=None, sb=None):
        """-> dict of everything the call returns or writes"""
        fn = (hip() if self.mine else ref()).srslte_ulsch_decode
        fn.argtypes = [C.c_void_p] * 7
        cfg = sh.cfg(rv)
        cfg.softbuffers = C.addressof(sb if sb is not None else self.sb)
        ubuf = (C.c_uint8 * (C.sizeof(UciValue) + 16))()  # the reference writes a byte behind ri when ri_len = 2 (uci.c:784): room for it
        C.memset(ubuf, 0x33, len(ubuf))
        uci = UciValue.from_buffer(ubuf)
        if uci_in is not None:
            uci.ri = uci_in
        qq, gg, cs = llr.copy(), np.zeros(sh.nbits + 64, np.int16), c_seq.copy()
        out = np.full(sh.tbs // 8 + 3 + GUARD, FILL, np.uint8)
        rc = fn(self.q, C.byref(cfg), p(qq), p(gg), p(cs), p(out), C.byref(uci))
        if self.mine and rc != -2:
            gg = np.zeros(sh.nbits + 64, np.int16)
            assert hip().srslte_hip_ulsch_debug_g(sch_handle(self), p(gg), sh.nbits) == 0
        u = bytes(uci)
        return {"rc": rc, "data": out, "ack": list(uci.ack.ack_value), "ack_valid_byte": u[UciValue.ack.offset + 10], "ri": uci.ri, "sr": u[0],
                "cqi": u[UciValue.cqi.offset:UciValue.cqi.offset + C.sizeof(CqiValue)] if sh.cqi else None, "K_segm": cfg.K_segm,
                "rank": bool(cfg.uci_cfg.cqi.rank_is_not_one), "avg_it": float(self.qb[self.Ly["srslte_sch_t.avg_iterations"]:][:4].view(np.float32)[0]),
                "g": gg[:sh.nbits]}

    def soft(self, C_, n, sb=None):
        sbb, L = np.frombuffer(sb if sb is not None else self.sb, np.uint8), self.Ly

        def ptr(f):
            return int(sbb[L["srslte_softbuffer_rx_t." + f]:][:8].view(np.uint64)[0])
        crc = np.ctypeslib.as_array((C.c_uint8 * C_).from_address(ptr("cb_crc"))).copy()
        bf = [np.ctypeslib.as_array((C.c_int16 * n).from_address(int(np.ctypeslib.as_array((C.c_uint64 * C_).from_address(ptr("buffer_f")))[c]))).copy() for c in range(C_)]
        dt = [np.ctypeslib.as_array((C.c_uint8 * 768).from_address(int(np.ctypeslib.as_array((C.c_uint64 * C_).from_address(ptr("data")))[c]))).copy() for c in range(C_)]
        return crc, bf, dt, int(sbb[L["srslte_softbuffer_rx_t.tb_crc"]])


def sch_handle(rx):
    """the srslte_hip_sch_t behind q->decoder.dec16_hdlr[0] is not public: srslte_hip_ulsch_debug_g goes through a tiny accessor of the library"""
    H = hip()
    H.srslte_hip_compat_sch_of.restype = C.c_void_p
    H.srslte_hip_compat_sch_of.argtypes = [C.c_void_p]
    H.srslte_hip_ulsch_debug_g.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    return H.srslte_hip_compat_sch_of(C.c_void_p(C.addressof(rx.q)))


def stats_ul():
    out = (C.c_ulonglong * 2)()
    hip().srslte_hip_compat_stats_ul(out)
    return out[0], out[1]


def same(m, r, sh, what):
    assert m["rc"] == r["rc"], (what, m["rc"], r["rc"])
    for k in ("ack", "ack_valid_byte", "ri", "sr", "cqi", "K_segm", "rank", "avg_it"):
        assert m[k] == r[k], (what, k, m[k], r[k])
    assert m["sr"] == 0x33 and m["ack_valid_byte"] == 0x33
    assert np.array_equal(m["data"], r["data"]), (what, "data", np.nonzero(m["data"] != r["data"])[0][:8].tolist())
    # the last block lands with its own 24 CRC bits behind the transport block's (decode_tb_cb copies K / 8 bytes per block): the guard starts there
    assert np.all(m["data"][sh.tbs // 8 + 6:] == FILL) or sh.tbs == 0
    d = np.nonzero(m["g"] != r["g"])[0]
    assert d.size == 0, (what, "g", d.size, d[:8].tolist(), m["g"][d[:8]].tolist(), r["g"][d[:8]].tolist())


def same_soft(mine, theirs, sh, what, sb_m=None, sb_r=None):
    if sh.tbs == 0:
        return None
    s = seg(sh.tbs)
    H = hip()  # the meaningful length: the decoder's window layout where it has sub-blocks, the plain 3K + 12 otherwise
    n = H.srslte_hip_tdec_input_len(s.K1, 1 if H.srslte_hip_tdec_autoimp_get_subblocks(s.K1) else 0)
    (crc_m, bf_m, dt_m, tb_m), (crc_r, bf_r, dt_r, tb_r) = mine.soft(s.C, n, sb_m), theirs.soft(s.C, n, sb_r)
    assert np.array_equal(crc_m, crc_r) and tb_m == tb_r, (what, crc_m, crc_r, tb_m, tb_r)
    rlen = (s.K1 - (24 if s.C > 1 else 0)) // 8
    for c in range(s.C):
        if crc_r[c]:
            if not tb_r:
                assert np.array_equal(dt_m[c][:rlen], dt_r[c][:rlen]), (what, "stored bytes", c)
        else:
            d = np.nonzero(bf_m[c] != bf_r[c])[0]
            assert d.size == 0, (what, "buffer_f", c, d.size, d[:8].tolist())
    return crc_r


def payload(tbs, seed=0):
    return np.random.default_rng(tbs + seed).integers(0, 256, max(tbs, 8) // 8 + 64, dtype=np.uint8)


HL_LONG = ("hl", 8, False, 0x5A)  # 4 + 16 = 20 bits: rate de-matching, tail-biting Viterbi and CRC8
S6 = dict(L_prb=6, mod=QAM16, nsymb=12, tbs=6200)
# name -> (shape, failing sigma). The shapes are the smallest that reach each branch.
CASES = {
    # Q'_ack = min(ceil(1 x 144 x 15.875 / 40), 4 x 12) = 48: every one of the 12 rows, from the bottom up
    "1prb_qpsk_ack1": (Shape(1, QPSK, 12, 40, ack=[1]), 0.95),
    "2prb_16qam_12symb": (Shape(2, QAM16, 12, 600, ack=[1, 0], ri=(1, 1)), 0.30),
    "2prb_16qam_11symb": (Shape(2, QAM16, 11, 600, ack=[1, 0], ri=(1, 1)), 0.25),
    "2prb_16qam_10symb": (Shape(2, QAM16, 10, 600, ack=[0, 1], ri=(1, 0)), 0.25),
    "6prb_qpsk": (Shape(6, QPSK, 12, 6200), None),
    "6prb_16qam": (Shape(**S6, cqi=HL_LONG), 0.05),
    "6prb_64qam": (Shape(6, QAM64, 12, 6200, ack=[0, 1], cqi=HL_LONG), 0.05),
    "100prb_64qam": (Shape(100, QAM64, 12, 75376), 0.10),
    "none": (Shape(**S6), 0.05),
    "ack1": (Shape(**S6, ack=[1]), 0.05),
    "ack2": (Shape(**S6, ack=[1, 0]), 0.05),
    "ack3": (Shape(**S6, ack=[1, 0, 1]), 0.05),
    "ri": (Shape(**S6, ri=(1, 1)), 0.05),
    "ri_qpsk": (Shape(6, QPSK, 12, 1544, ri=(1, 1)), 0.35),  # Qm = 2: g[0] is the flipped p1 LLR of the RI symbol in the last column
    "ri2": (Shape(**S6, ri=(2, 1)), 0.05),
    "ack2_ri": (Shape(**S6, ack=[0, 1], ri=(1, 0)), 0.05),
    "cqi_wb": (Shape(**S6, cqi=("wb", 11)), 0.05),
    "cqi_long": (Shape(**S6, cqi=HL_LONG), 0.05),
    "ack_ri_cqi": (Shape(**S6, ack=[1, 1], ri=(1, 1), cqi=HL_LONG), None),
    "ri_sizes_the_report": (Shape(**S6, ack=[1], ri=(1, 1), cqi=("hl", 8, True, 0xC3)), 0.05),  # 20 bits at rank 1, 41 above: the size follows the decoded RI
    "cqi_only": (Shape(6, QAM16, 12, 0, cqi=HL_LONG), None),
    "cqi_only_wb_ack": (Shape(6, QAM16, 12, 0, ack=[1], cqi=("wb", 7)), None),
    "cqi_only_ack2_ri": (Shape(6, QPSK, 12, 0, ack=[1, 0], ri=(1, 1), cqi=HL_LONG), None),
}


# four transmissions never carry these two (QPSK: 6912 LLRs for 6224 bits; 16QAM with ACK, RI and a long report in the way): the reference
# decodes them at no noise level, so they are compared over the four transmissions of the error-free channel only
NEVER = ("6prb_qpsk", "ack_ri_cqi")


def pair(max_it=4):
    return Rx(True, max_it), Rx(False, max_it)


def run_sequence(name, sigma, seed0):
    """rv 0, 2, 3, 1 on one soft buffer per side until the reference decodes: every transmission compared -> the reference's return codes"""
    sh = CASES[name][0]
    data = payload(sh.tbs)
    mine, theirs = pair()
    rank_wait = 1 if name == "ri_sizes_the_report" else 0
    rcs = []
    for k, rv in enumerate((0, 2, 3, 1) if sh.tbs else (0,)):
        llr, c_seq = transmit(sh, rv, data, sigma, seed0 + k)
        w0 = stats_ul()
        r = theirs.decode(sh, rv, llr, c_seq)
        m = mine.decode(sh, rv, llr, c_seq)
        w1 = stats_ul()
        same(m, r, sh, (name, rv))
        crc = same_soft(mine, theirs, sh, (name, rv))
        rcs.append(r["rc"])
        block_failed = crc is not None and not crc.all()
        assert (w1[0] - w0[0], w1[1] - w0[1] - rank_wait) == (1, 2 if block_failed else 1), (name, rv, "one wait, two when a block failed", w1, w0, crc)
        if sh.tbs == 0:
            assert r["rc"] > 0  # the last Q' it computed
        if len(sh.ack) in (1, 2) and sigma == CLEAN:
            assert r["ack"][:len(sh.ack)] == sh.ack
        elif sh.ack and sigma == CLEAN:
            assert r["ack"][0] == 0  # three bits and more: no decision, the sum stays 0
        if sh.ri and sh.ri[0] == 1 and sigma == CLEAN:
            assert r["ri"] == sh.ri[1]
        if r["rc"] == 0:
            assert np.array_equal(r["data"][:sh.tbs // 8], data[:sh.tbs // 8])
            break
    mine.free(), theirs.free()
    return rcs


@pytest.mark.parametrize("name", list(CASES))
def test_error_free_channel_matches_the_reference(name):
    """CLEAN over the transmissions the shape needs (at 6 PRB a tbs of 6200 does not fit one transmission at any modulation)"""
    rcs = run_sequence(name, CLEAN, 1)
    if name not in NEVER:
        assert rcs[-1] >= 0, rcs


@pytest.mark.parametrize("name", [n for n in CASES if CASES[n][1] is not None])
def test_harq_sequence_matches_the_reference(name):
    rcs = run_sequence(name, CASES[name][1], 100)
    assert rcs[0] == -1, "the chosen level must fail a block at rv 0 (reference alone): %s" % rcs
    assert rcs[-1] == 0, "and the sequence must recover it (reference alone): %s" % rcs


def test_long_report_with_a_failed_crc8():
    """sigma 1.2 on the 6-PRB 16QAM shape: the reference's CRC8 over the 20-bit report fails (checked here): data_crc false, the report zeros"""
    sh = Shape(**S6, cqi=HL_LONG)
    llr, c_seq = transmit(sh, 0, payload(sh.tbs), 1.2, 7)
    mine, theirs = pair()
    m, r = mine.decode(sh, 0, llr, c_seq), theirs.decode(sh, 0, llr, c_seq)
    assert r["cqi"][CqiValue.data_crc.offset] == 0, "raise sigma: the reference's CRC8 passed"
    same(m, r, sh, "crc8")
    same_soft(mine, theirs, sh, "crc8")
    mine.free(), theirs.free()


@pytest.mark.parametrize("first_mine", [True, False])
def test_soft_buffers_cross_between_the_library_and_the_reference(first_mine):
    sh, sigma = CASES["cqi_long"]
    data = payload(sh.tbs)
    mine, theirs = pair()
    a, b = (mine, theirs) if first_mine else (theirs, mine)
    other_a, other_b = (theirs, mine) if first_mine else (mine, theirs)
    # two soft buffers walk the same sequence; each is decoded into by one side at rv 0 and by the other at rv 2
    llr0, cs0 = transmit(sh, 0, data, sigma, 100)
    ra, rb = a.decode(sh, 0, llr0, cs0, sb=mine.sb), other_a.decode(sh, 0, llr0, cs0, sb=theirs.sb)
    same(*((ra, rb) if first_mine else (rb, ra)), sh, "rv0")
    assert ra["rc"] == -1
    same_soft(mine, theirs, sh, "rv0")
    llr2, cs2 = transmit(sh, 2, data, sigma, 101)
    rb2, ra2 = b.decode(sh, 2, llr2, cs2, sb=mine.sb), other_b.decode(sh, 2, llr2, cs2, sb=theirs.sb)
    same(*((ra2, rb2) if first_mine else (rb2, ra2)), sh, "rv2")
    same_soft(mine, theirs, sh, "rv2")
    mine.free(), theirs.free()


def test_refusals_on_a_live_object_write_nothing():
    sh = CASES["1prb_qpsk_ack1"][0]
    llr, c_seq = transmit(sh, 0, payload(sh.tbs), CLEAN, 1)
    mine = Rx(True)
    assert mine.decode(sh, 0, llr, c_seq)["rc"] == 0
    w0 = stats_ul()
    bad = []
    x = Shape(**S6, ack=[1]); x.mod = 4; bad.append(("256QAM", x, False))
    x = Shape(**S6, ack=[1]); x.mod = 0; bad.append(("BPSK", x, False))
    x = Shape(6, QAM16, 12, 6208, ack=[1]); bad.append(("filler bits / two block sizes", x, False))
    x = Shape(**S6, ack=[1]); x.nbits -= 4; bad.append(("nof_bits", x, False))
    bad.append(("8-bit LLRs", Shape(**S6, ack=[1]), True))
    for what, x, l8 in bad:
        mine.qb[mine.Ly["srslte_sch_t.llr_is_8bit"]] = 1 if l8 else 0
        mine.soft_before = mine.soft(2, 3 * (3136 + 32) + 12)
        r = mine.decode(x, 0, np.resize(llr, x.nbits + 8), np.resize(c_seq, x.nbits + 8))
        assert r["rc"] == -2, (what, r["rc"])
        assert np.all(r["data"] == FILL) and r["ack"] == [0x33] * 10 and r["ri"] == 0x33 and r["sr"] == 0x33, what
        after = mine.soft(2, 3 * (3136 + 32) + 12)
        assert all(np.array_equal(a, b) for a, b in zip(mine.soft_before[1], after[1])) and np.array_equal(mine.soft_before[0], after[0]), what
    mine.qb[mine.Ly["srslte_sch_t.llr_is_8bit"]] = 0
    assert stats_ul() == w0
    ref().srslte_softbuffer_rx_reset(mine.sb)
    assert mine.decode(sh, 0, llr, c_seq)["rc"] == 0  # and the object still serves
    mine.free()


def test_the_object_grows_when_a_larger_block_follows():
    mine, theirs = pair()
    for name in ("1prb_qpsk_ack1", "ri_qpsk", "100prb_64qam", "2prb_16qam_11symb"):
        sh = CASES[name][0]
        data = payload(sh.tbs)
        for s in (mine, theirs):
            ref().srslte_softbuffer_rx_reset(s.sb)
        llr, c_seq = transmit(sh, 0, data, CLEAN, 1)
        m, r = mine.decode(sh, 0, llr, c_seq), theirs.decode(sh, 0, llr, c_seq)
        same(m, r, sh, name)
        assert r["rc"] == 0
    mine.free(), theirs.free()
