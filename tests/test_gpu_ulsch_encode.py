"""srslte_ulsch_encode served by the library (one device call per PUSCH transport block, include/srslte_hip/srslte_compat.h) against the
reference's own srslte_ulsch_encode (oracle/_ref/libsrslte_ref.so, sch.c:1068-1210) on the same configuration, payload and UCI values.

Both sides get a zeroed g_bits, a q_bits filled with 0xA5 and a guard behind it. Compared, all exactly: the return code, q_bits and its guard, g
over its defined bits - the host copy and the device's own words (srslte_hip_ulsch_enc_debug) -, q->ack_ri_bits[0 .. ret) as (position, type)
pairs, cfg->K_segm and every circular buffer of the srslte_softbuffer_tx_t over its 3K + 12 bits. Each served call must count as one call and
one stream wait. The shapes are the smallest that reach each branch; struct layouts are the ctypes mirrors of test_gpu_ulsch_decode.py, which
tests/test_ulsch_host.py and tests/test_ulsch_encode_host.py hold against the reference's headers.

A 2-bit ACK at I_offset_ack 15 does not saturate Q' at 4 M_sc: index 15 is the reserved entry of 36.213 Table 8.6.3-1, which both sides
answer with -1. That call is compared among the refusals; index 14 (beta 126), the largest offset there is, is the case that saturates."""
import ctypes as C
import math

import numpy as np
import pytest

from _libs import hip, opaque, p, ref
from test_gpu_ulsch_decode import HL_LONG, QAM16, QAM64, QPSK, S6, Shape, layout, payload, seg

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(ref() is None, reason="oracle/_ref/libsrslte_ref.so not built")]
GUARD, FILL = 64, 0xA5
RI_COLS = {True: (1, 4, 7, 10), False: (0, 3, 5, 8)}

CASES = {
    "1prb_qpsk_k40": Shape(1, QPSK, 12, 16),
    # Q'_ack = min(ceil(2 x 144 x 126 / 40), 4 x 12) = 48: every row of the four ACK columns
    "1prb_qpsk_ack2_saturated": Shape(1, QPSK, 12, 16, ack=[1, 0], I=(14, 6, 6)),
    "6prb_qpsk_ack1_wb": Shape(6, QPSK, 12, 1544, ack=[1], cqi=("wb", 11)),  # 4 bits: the (32, O) block code
    # 20 bits: CRC8 and the convolutional code; a 1-bit ACK and RI at Qm = 6: value, repetition, four placeholders
    "6prb_64qam_11symb": Shape(6, QAM64, 11, 6200, ack=[1], ri=(1, 1), cqi=HL_LONG),
    "2prb_16qam_10symb": Shape(2, QAM16, 10, 600, ack=[0, 1], ri=(1, 0)),
    "2prb_16qam_9symb": Shape(2, QAM16, 9, 600, ack=[1, 0], ri=(1, 1), cqi=("wb", 5)),
    # C = 3; Q'_cqi = ceil(26 x 3600 x 1.125 / 15360) = 7 symbols of 4 bits end inside a byte, and G' = 3600 - 7 is no multiple of 3 (asserted below)
    "25prb_16qam_c3": Shape(25, QAM16, 12, 15264, cqi=("hl", 7, False, 0x3C), I=(9, 6, 2)),
    "cqi_only_ack2_ri": Shape(6, QPSK, 12, 0, ack=[1, 0], ri=(1, 1), cqi=HL_LONG),
    "ack3": Shape(**S6, ack=[1, 0, 1]),
    "ack10": Shape(**S6, ack=[1, 0, 1, 1, 0, 0, 1, 0, 1, 1]),
    "ri2": Shape(**S6, ri=(2, 1)),
    "ri2_zero_ack2_qpsk": Shape(6, QPSK, 12, 1544, ack=[1, 1], ri=(2, 0)),
    "100prb_64qam": Shape(100, QAM64, 12, 75376, ack=[1, 0], ri=(1, 1)),
}
HARQ = ("6prb_64qam_11symb", "25prb_16qam_c3")


def stats_ul_tx():
    out = (C.c_ulonglong * 2)()
    hip().srslte_hip_compat_stats_ul_tx(out)
    return out[0], out[1]


class SoftTx:
    """a srslte_softbuffer_tx_t of the reference's allocator (softbuffer.c), which either side encodes into or out of"""

    def __init__(self):
        self.sb = opaque(64)
        assert ref().srslte_softbuffer_tx_init(self.sb, 100) == 0
        ref().srslte_softbuffer_tx_reset(self.sb)
        self.max_cb = int(np.frombuffer(self.sb, np.uint32, 1, 0)[0])  # what the allocator made (16): free() walks that many

    def free(self):
        ref().srslte_softbuffer_tx_free(self.sb)

    def blocks(self, n_cb, K):
        """-> the n_cb circular buffers over their 3K + 12 bits (the rest of the last byte masked)"""
        ptrs = np.ctypeslib.as_array((C.c_uint64 * n_cb).from_address(int(np.frombuffer(self.sb, np.uint64, 1, 8)[0])))
        nb = 3 * K + 12
        out = []
        for c in range(n_cb):
            b = np.ctypeslib.as_array((C.c_uint8 * ((nb + 7) // 8)).from_address(int(ptrs[c]))).copy()
            if nb % 8:
                b[-1] &= 0xff00 >> (nb % 8) & 0xff
            out.append(b)
        return out

    def fill(self, n_cb, K, value):
        ptrs = np.ctypeslib.as_array((C.c_uint64 * n_cb).from_address(int(np.frombuffer(self.sb, np.uint64, 1, 8)[0])))
        for c in range(n_cb):
            C.memset(int(ptrs[c]), value, (3 * K + 12 + 7) // 8)


class Tx:
    """one srslte_sch_t; `mine`: srslte_ulsch_encode is this library's, which needs nothing of the struct but its ack_ri_bits"""

    def __init__(self, mine):
        self.mine, self.Ly = mine, layout()
        self.q = opaque(self.Ly["srslte_sch_t"] + 256)
        if not mine:
            assert ref().srslte_sch_init(self.q) == 0
        # the reference's object is never freed: srslte_sch_free frees the process-wide rate-matching tables (sch.c:150-151)

    def pos(self, n):
        return np.frombuffer(self.q, np.uint32, 2 * n, self.Ly["srslte_sch_t.ack_ri_bits"]).reshape(n, 2).copy()

    def encode(self, sh, rv, data, soft, cfg_edit=None, with_g=True):
        """-> dict of everything the call returns or writes. data None: a retransmission without the payload"""
        fn = (hip() if self.mine else ref()).srslte_ulsch_encode
        fn.argtypes = [C.c_void_p] * 6
        cfg = sh.cfg(rv, sh.ri[1] if sh.ri else 0)
        cfg.softbuffers = C.addressof(soft.sb) if soft is not None else None
        if cfg_edit:
            cfg_edit(cfg)
        uci = sh.uci_tx()
        g = np.zeros(sh.nbits // 8 + GUARD, np.uint8)
        qb = np.full(sh.nbits // 8 + GUARD, FILL, np.uint8)
        w0 = stats_ul_tx()
        rc = fn(self.q, C.byref(cfg), p(data) if data is not None else None, C.byref(uci), p(g) if with_g else None, p(qb))
        w1 = stats_ul_tx()
        out = {"rc": rc, "q": qb, "g": g, "K_segm": cfg.K_segm, "pos": self.pos(max(rc, 0)), "served": (w1[0] - w0[0], w1[1] - w0[1])}
        if self.mine and rc >= 0:
            H = hip()
            H.srslte_hip_compat_sch_enc.restype = C.c_void_p
            H.srslte_hip_ulsch_enc_debug.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
            n_ri = sum(1 for position, _ in out["pos"].tolist() if position // (sh.nbits // sh.nsymb) in RI_COLS[sh.nsymb > 10])
            words = np.zeros((sh.nbits - n_ri + 31) // 32, np.uint32)
            assert H.srslte_hip_ulsch_enc_debug(H.srslte_hip_compat_sch_enc(), p(words), words.size) == 0
            out["g_dev"] = words.view(np.uint8)
        return out


def defined_g(sh, r):
    """the bits of g the call defines: (H' - Q'_ri) Qm, Q'_ri Qm being the entries of ack_ri_bits that lie in the RI columns"""
    n_ri = sum(1 for position, _ in r["pos"].tolist() if position // (sh.nbits // sh.nsymb) in RI_COLS[sh.nsymb > 10])
    return sh.nbits - n_ri


def masked(a, nbits):
    b = a[:(nbits + 7) // 8].copy()
    if nbits % 8:
        b[-1] &= 0xff00 >> (nbits % 8) & 0xff
    return b


def same(m, r, sh, what):
    assert m["rc"] == r["rc"], (what, m["rc"], r["rc"])
    assert r["rc"] >= 0, (what, r["rc"])
    assert m["served"] == (1, 1) and r["served"] == (0, 0), (what, "one call, one stream wait", m["served"], r["served"])
    assert m["K_segm"] == r["K_segm"], (what, m["K_segm"], r["K_segm"])
    d = np.nonzero(m["q"] != r["q"])[0]
    assert d.size == 0, (what, "q_bits", d.size, d[:8].tolist(), m["q"][d[:8]].tolist(), r["q"][d[:8]].tolist())
    assert np.all(m["q"][sh.nbits // 8:] == FILL), (what, "guard")
    n = defined_g(sh, r)
    for k in ("g", "g_dev"):
        a, b = masked(m[k], n), masked(r["g"], n)
        d = np.nonzero(a != b)[0]
        assert d.size == 0, (what, k, n, d.size, d[:8].tolist(), a[d[:8]].tolist(), b[d[:8]].tolist())
    assert np.all(m["g"][(n + 7) // 8:] == 0), (what, "g behind its bits")
    assert np.array_equal(m["pos"], r["pos"]), (what, "ack_ri_bits", m["rc"], np.nonzero(m["pos"] != r["pos"])[0][:8].tolist())


def same_soft(sm, sr, sh, what):
    if sh.tbs == 0:
        return
    s = seg(sh.tbs)
    for c, (a, b) in enumerate(zip(sm.blocks(s.C, s.K1), sr.blocks(s.C, s.K1))):
        d = np.nonzero(a != b)[0]
        assert d.size == 0, (what, "buffer_b", c, d.size, d[:8].tolist())


@pytest.fixture(scope="module")
def sides():
    return Tx(True), Tx(False)


@pytest.mark.parametrize("name", list(CASES))
def test_first_transmission_matches_the_reference(sides, name):
    sh = CASES[name]
    mine, theirs = sides
    sm, sr = SoftTx(), SoftTx()
    data = payload(sh.tbs)
    r = theirs.encode(sh, 0, data, sr)
    m = mine.encode(sh, 0, data, sm)
    same(m, r, sh, name)
    same_soft(sm, sr, sh, name)
    if sh.ack or sh.ri:
        assert r["rc"] > 0
    sm.free(), sr.free()


def test_the_shapes_reach_what_they_are_chosen_for(sides):
    """with the reference alone: the saturated Q'_ack, the report that ends inside a byte in front of three unequal blocks, the repetition and
    placeholder types, the block code of a long ACK"""
    _, theirs = sides
    sr = SoftTx()
    sh = CASES["1prb_qpsk_ack2_saturated"]
    assert theirs.encode(sh, 0, payload(sh.tbs), sr)["rc"] == 4 * 12 * sh.Qm
    sh = CASES["25prb_16qam_c3"]
    s = seg(sh.tbs)
    O = 4 + 2 * 7
    Qp_cqi = math.ceil(float(np.float32(O + 8) * np.float32(sh.nof_re) * np.float32(1.125) / np.float32(s.C * s.K1)))  # uci.c:276, I_offset_cqi 2
    assert s.C == 3 and (Qp_cqi * sh.Qm) % 8 != 0 and (sh.nof_re - Qp_cqi) % s.C != 0, (s.C, Qp_cqi)
    sh = CASES["6prb_64qam_11symb"]
    types = set(theirs.encode(sh, 0, payload(sh.tbs), sr)["pos"][:, 1].tolist())
    assert {2, 3} <= types, types
    assert seg(CASES["1prb_qpsk_k40"].tbs).K1 == 40 and seg(CASES["100prb_64qam"].tbs).C == 13
    sr.free()


@pytest.mark.parametrize("name", HARQ)
def test_rv_sequence_on_one_soft_buffer(sides, name):
    """rv 0, 2, 3, 1: the retransmissions without the payload read the circular buffers rv 0 left and nothing else"""
    sh = CASES[name]
    mine, theirs = sides
    sm, sr = SoftTx(), SoftTx()
    data = payload(sh.tbs)
    for rv in (0, 2, 3, 1):
        r = theirs.encode(sh, rv, data if rv == 0 else None, sr)
        m = mine.encode(sh, rv, data if rv == 0 else None, sm)
        same(m, r, sh, (name, rv))
        same_soft(sm, sr, sh, (name, rv))
    # with the payload given again the retransmission still depends on the buffers alone
    r, m = theirs.encode(sh, 2, data, sr), mine.encode(sh, 2, payload(sh.tbs, 1), sm)
    same(m, r, sh, (name, "rv 2 with another payload"))
    sm.free(), sr.free()


@pytest.mark.parametrize("name", HARQ)
def test_soft_buffers_cross_between_the_library_and_the_reference(sides, name):
    """two soft buffers walk rv 0, 2, 3: a is written by the library and read by the reference, b the other way round, then swapped again"""
    sh = CASES[name]
    mine, theirs = sides
    a, b = SoftTx(), SoftTx()
    data = payload(sh.tbs)
    same(mine.encode(sh, 0, data, a), theirs.encode(sh, 0, data, b), sh, (name, "rv 0"))
    same_soft(a, b, sh, (name, "rv 0"))
    same(mine.encode(sh, 2, None, b), theirs.encode(sh, 2, None, a), sh, (name, "rv 2, crossed"))
    same(mine.encode(sh, 3, None, a), theirs.encode(sh, 3, None, b), sh, (name, "rv 3, back"))
    same_soft(a, b, sh, (name, "after"))
    a.free(), b.free()


def test_g_bits_may_be_null(sides):
    sh = CASES["6prb_qpsk_ack1_wb"]
    mine, theirs = sides
    sm, sr = SoftTx(), SoftTx()
    data = payload(sh.tbs)
    r, m = theirs.encode(sh, 0, data, sr), mine.encode(sh, 0, data, sm, with_g=False)
    m["g"] = m["g_dev"].copy()
    m["g"] = np.concatenate([masked(m["g"], defined_g(sh, r)), np.zeros(8, np.uint8)])
    same(m, r, sh, "g_bits NULL")
    sm.free(), sr.free()


def test_refusals_write_nothing(sides):
    mine, theirs = sides
    base = dict(L_prb=6, mod=QPSK, nsymb=12, tbs=6200)  # C = 2, K = 3136
    good = Shape(**base, ack=[1])
    soft = SoftTx()
    data = payload(6264)
    assert mine.encode(good, 0, data, soft)["rc"] > 0
    w0 = stats_ul_tx()

    def edit(**kw):
        def f(cfg):
            for k, v in kw.items():
                o = cfg
                path = k.split("__")
                for part in path[:-1]:
                    o = getattr(o, part)
                    o = o[0] if part == "ack" else o
                setattr(o, path[-1], v)
        return f

    def shape(**kw):
        x = Shape(**{**base, **{k: v for k, v in kw.items() if k in ("L_prb", "mod", "nsymb", "tbs", "ack", "ri", "cqi", "I")}})
        for k, v in kw.items():
            if k in ("set_mod", "set_nbits"):
                setattr(x, k[4:], v)
        return x

    big_report = Shape(1, QPSK, 12, 16, cqi=HL_LONG, I=(9, 6, 15))  # Q'_cqi = min(ceil(28 x 144 x 6.25 / 40), 144): nothing left for the block
    bad = [  # what, shape, rv, data, soft, edit, expected, the reference returns the same
        ("256QAM", shape(ack=[1], set_mod=4), 0, data, soft, None, -2, False),
        ("BPSK", shape(ack=[1], set_mod=0), 0, data, soft, None, -2, False),
        ("filler bits", shape(tbs=4016, ack=[1]), 0, data, soft, None, -1, True),
        ("two block sizes", shape(tbs=6264, ack=[1]), 0, data, soft, None, -2, False),
        ("nof_bits", shape(ack=[1], set_nbits=good.nbits - 8), 0, data, soft, None, -2, False),
        ("nof_symb 8", shape(nsymb=8, ack=[1]), 0, data, soft, None, -2, False),
        ("ri_len 3", shape(ri=(3, 1)), 0, data, soft, None, -2, False),
        ("11 ACK bits", good, 0, data, soft, edit(uci_cfg__ack__nof_acks=11), -2, False),
        ("I_offset_cqi 16", good, 0, data, soft, edit(uci_offset__I_offset_cqi=16), -2, False),
        ("reserved beta: I_offset_ack 15", Shape(1, QPSK, 12, 16, ack=[1, 0], I=(15, 6, 6)), 0, data, soft, None, -1, True),
        ("reserved beta of the report", shape(cqi=("wb", 3), I=(9, 6, 1)), 0, data, soft, None, -1, True),
        ("tbs 0 without a report", shape(tbs=0, ack=[1]), 0, data, soft, None, -2, False),
        ("the report takes every symbol", big_report, 0, data, soft, None, -2, False),
        ("TDD bundling", good, 0, data, soft, edit(uci_cfg__ack__N_bundle=2), -2, False),
        ("no payload at rv 0", good, 0, None, soft, None, -2, False),
        ("rv 4", good, 4, data, soft, None, -2, False),
        ("no soft buffer", good, 0, data, None, None, -2, True),
        ("a soft buffer of one block", good, 0, data, soft, edit_max_cb(soft, 1), -1, True),
    ]
    for what, x, rv, d, sb, ed, expected, ref_too in bad:
        soft.fill(2, 3136, 0x5C)
        C.memset(C.addressof(mine.q) + mine.Ly["srslte_sch_t.ack_ri_bits"], 0x77, 64)
        m = mine.encode(x, rv, d, sb, ed)
        restore_max_cb(soft)
        assert m["rc"] == expected, (what, m["rc"])
        assert np.all(m["q"] == FILL) and not m["g"].any(), (what, "q_bits / g_bits written")
        assert all(np.all(b[:-1] == 0x5C) for b in soft.blocks(2, 3136)), (what, "buffer_b written")
        assert np.all(np.frombuffer(mine.q, np.uint8, 64, mine.Ly["srslte_sch_t.ack_ri_bits"]) == 0x77), (what, "ack_ri_bits written")
        if ref_too:
            sr = SoftTx() if sb is not None else None
            r = theirs.encode(x, rv, d, sr, ed if not what.startswith("a soft buffer") else edit_max_cb_cfg(1))
            assert r["rc"] == expected, (what, "the reference", r["rc"])
            if sr is not None:
                restore_max_cb(sr)
                sr.free()
    assert stats_ul_tx() == w0
    ref().srslte_softbuffer_tx_reset(soft.sb)
    ours, sr = mine.encode(good, 0, data, soft), SoftTx()
    same(ours, theirs.encode(good, 0, data, sr), good, "the object still serves")
    soft.free(), sr.free()


def edit_max_cb(soft, n):
    """shrinks the library side's soft buffer to n blocks for the next call (restore_max_cb puts back what the allocator made)"""
    def f(cfg):
        np.frombuffer(soft.sb, np.uint32, 1, 0)[0] = n
    return f


def edit_max_cb_cfg(n):
    def f(cfg):
        C.cast(cfg.softbuffers, C.POINTER(C.c_uint32))[0] = n
    return f


def restore_max_cb(soft):
    np.frombuffer(soft.sb, np.uint32, 1, 0)[0] = soft.max_cb


def test_the_object_grows_when_a_larger_block_follows(sides):
    mine, theirs = sides
    for name in ("1prb_qpsk_k40", "6prb_64qam_11symb", "100prb_64qam", "2prb_16qam_9symb"):
        sh = CASES[name]
        sm, sr = SoftTx(), SoftTx()
        data = payload(sh.tbs)
        same(mine.encode(sh, 0, data, sm), theirs.encode(sh, 0, data, sr), sh, name)
        same_soft(sm, sr, sh, name)
        sm.free(), sr.free()
