"""srslte_dlsch_encode2 served by the library (one device call per transport block, include/srslte_hip/srslte_compat.h) against the reference's
own srslte_dlsch_encode2 (oracle/_ref/libsrslte_ref.so, sch.c:549-575 -> encode_tb_off :183-289) on the same transport block: return code,
the packed e_bits, the bytes behind them and - after rv 0 - the 3K + 12 bits of every circular buffer of the srslte_softbuffer_tx_t, through
the HARQ sequence rv 0, 2, 3, 1 on ONE soft buffer; soft buffers handed from one side to the other between transmissions; the refusals; the
calling thread's encoder object growing and shrinking; the library's own counter. Struct layouts come from this repository's compat header,
which tests/test_sch_encode_host.py and tests/test_abi_layout.py hold against the reference's."""
import ctypes as C
import importlib
import os
import threading

import numpy as np
import pytest

from _libs import ROOT, hip, opaque, p, ref, struct_layout

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(ref() is None, reason="oracle/_ref/libsrslte_ref.so not built")]
_cache = {}
GUARD, FILL = 64, 0xA5
QPSK, QAM16, QAM64, QAM256 = 1, 2, 3, 4

# (tbs, mod, Nl, nof_bits): the smallest cases that reach each branch
CASES = [(328, QPSK, 1, 1200),          # one block of K = 352, no CB CRC; E = 1200 > 3K + 12 = 1068: the selection wraps
         (6200, QPSK, 1, 3002),         # C = 2, K = 3136; E = 1500 / 1502: gamma = 1, block 1 starts at bit 4 of a byte, the last byte is partial
         (6200, QPSK, 2, 6012),         # Qm Nl = 4; E = 3004 / 3008
         (6200, QAM16, 1, 19212),       # E = 9604 / 9608 > 9420: wrap and an unaligned block start together
         (12216, QAM64, 1, 6 * 2001),   # C = 2 at K = 6144, the largest block
         (75376, QAM64, 1, 6 * 14580),  # 20 MHz MCS 28: C = 13, K = 5824
         (97896, QAM256, 1, 8 * 14230)]  # C = 16, the most a 110-PRB soft buffer holds


def layout():
    if not _cache:
        _cache.update(struct_layout({"srslte_sch_t": ["encoder", "crc_tb", "crc_cb"], "srslte_pdsch_cfg_t": ["grant", "softbuffers"],
                                     "srslte_pdsch_grant_t": ["tb", "nof_tb"], "srslte_ra_tb_t": ["mod", "tbs", "rv", "nof_bits", "cw_idx", "enabled"],
                                     "srslte_softbuffer_tx_t": ["max_cb", "buffer_b"]}, ["srslte_hip/srslte_compat.h"], [os.path.join(ROOT, "include")]))
    return _cache


def seg(tbs):
    class Seg(C.Structure):
        _fields_ = [(n, C.c_uint32) for n in ("F", "C", "K1", "K2", "K1_idx", "K2_idx", "C1", "C2", "tbs")]
    s = Seg()
    assert hip().srslte_cbsegm(C.byref(s), tbs) == 0
    return s


def sch(mine):
    """a srslte_sch_t; `mine`: what srslte_sch_init leaves with the replaced translation units - the library's encoder, the reference's CRC tables"""
    key = "sch_mine" if mine else "sch_ref"
    if key not in _cache:
        Ly, R, H = layout(), ref(), hip()
        q = opaque(Ly["srslte_sch_t"] + 256)
        if mine:
            assert H.srslte_tcod_init(C.c_void_p(C.addressof(q) + Ly["srslte_sch_t.encoder"]), 6144) == 0
            assert R.srslte_crc_init(C.c_void_p(C.addressof(q) + Ly["srslte_sch_t.crc_tb"]), 0x1864CFB, 24) == 0
            assert R.srslte_crc_init(C.c_void_p(C.addressof(q) + Ly["srslte_sch_t.crc_cb"]), 0x1800063, 24) == 0
        else:
            assert R.srslte_sch_init(q) == 0
        _cache[key] = q
    return _cache[key]


class Harq:
    """one srslte_softbuffer_tx_t (the reference's init + reset) and a srslte_pdsch_cfg_t that points at it; either side encodes into it"""

    def __init__(self, prb, tbs, mod, nbits, Nl=1):
        Ly, R = layout(), ref()
        self.Ly, self.nbits, self.Nl = Ly, nbits, Nl
        self.sb = opaque(Ly["srslte_softbuffer_tx_t"] + 64)
        assert R.srslte_softbuffer_tx_init(self.sb, prb) == 0
        R.srslte_softbuffer_tx_reset(self.sb)
        self.cfg = opaque(Ly["srslte_pdsch_cfg_t"] + 64)
        self.g = np.frombuffer(self.cfg, np.uint8)
        self.tb0 = Ly["srslte_pdsch_cfg_t.grant"] + Ly["srslte_pdsch_grant_t.tb"]
        for f, v in (("mod", mod), ("tbs", tbs), ("rv", 0), ("nof_bits", nbits), ("cw_idx", 0)):
            self.u32(self.tb0 + Ly["srslte_ra_tb_t." + f], v)
        self.g[self.tb0 + Ly["srslte_ra_tb_t.enabled"]] = 1
        self.u32(Ly["srslte_pdsch_cfg_t.grant"] + Ly["srslte_pdsch_grant_t.nof_tb"], 1)  # Nl = 2 where nof_layers != nof_tb (sch.c:552-556)
        o = Ly["srslte_pdsch_cfg_t.softbuffers"]
        self.g[o:o + 8].view(np.uint64)[0] = C.addressof(self.sb)

    def u32(self, o, v):
        self.g[o:o + 4].view(np.uint32)[0] = v

    def encode(self, mine, rv, data, entry="srslte_dlsch_encode2"):
        """-> (return code, the whole e buffer: ceil(nbits / 8) bytes and the guard)"""
        self.u32(self.tb0 + self.Ly["srslte_ra_tb_t.rv"], rv)
        e = np.full((self.nbits + 7) // 8 + GUARD, FILL, np.uint8)
        fn = getattr(hip() if mine else ref(), entry)
        if entry == "srslte_dlsch_encode2":
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32]
            rc = fn(sch(mine), self.cfg, None if data is None else p(data), p(e), 0, 2 if self.Nl == 2 else 1)
        else:
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            rc = fn(sch(mine), self.cfg, None if data is None else p(data), p(e))
        return rc, e

    def max_cb(self):
        return int(np.frombuffer(self.sb, np.uint8)[self.Ly["srslte_softbuffer_tx_t.max_cb"]:][:4].view(np.uint32)[0])

    def w(self, c, nbytes):
        """a view of the first bytes of circular buffer c"""
        o = self.Ly["srslte_softbuffer_tx_t.buffer_b"]
        arr = int(np.frombuffer(self.sb, np.uint8)[o:o + 8].view(np.uint64)[0])
        return np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(int((C.c_uint64 * (c + 1)).from_address(arr)[c])))

    def free(self):
        ref().srslte_softbuffer_tx_free(self.sb)


def bits(e, n):
    return np.unpackbits(e[:(n + 7) // 8])[:n]


def same_e(a, b, nbits, what):
    (rc_a, e_a), (rc_b, e_b) = a, b
    assert rc_a == rc_b, (what, rc_a, rc_b)
    d = np.nonzero(bits(e_a, nbits) != bits(e_b, nbits))[0]
    assert d.size == 0, (what, d.size, d[:12].tolist())
    for e in (e_a, e_b):
        assert np.all(e[(nbits + 7) // 8:] == FILL), (what, "bytes behind e_bits were written")


def payload(tbs, seed=0):
    return np.random.default_rng(tbs + seed).integers(0, 256, tbs // 8 + 64, dtype=np.uint8)


@pytest.mark.parametrize("tbs,mod,Nl,nbits", CASES)
def test_dlsch_encode2_vs_reference_with_harq(tbs, mod, Nl, nbits):
    s, data = seg(tbs), payload(tbs)
    K, C_ = s.K1, s.C
    assert s.F == 0 and s.C2 == 0
    mine, theirs = Harq(110, tbs, mod, nbits, Nl), Harq(110, tbs, mod, nbits, Nl)
    for rv in (0, 2, 3, 1):
        m, r = mine.encode(True, rv, data), theirs.encode(False, rv, data)
        assert r[0] == 0
        same_e(m, r, nbits, ("rv", rv))
        if rv == 0:
            for c in range(C_):  # the circular buffers: 3K + 12 bits each, the rest of the last byte is not defined
                d = np.nonzero(bits(mine.w(c, 2400), 3 * K + 12) != bits(theirs.w(c, 2400), 3 * K + 12))[0]
                assert d.size == 0, ("circular buffer", c, d.size, d[:12].tolist())
        else:  # a retransmission depends on the soft buffer alone
            same_e(mine.encode(True, rv, None), r, nbits, ("rv without data", rv))
            same_e(theirs.encode(False, rv, None), r, nbits, ("reference, rv without data", rv))
    mine.free()
    theirs.free()


@pytest.mark.parametrize("tbs,mod,Nl,nbits", CASES)
def test_soft_buffers_pass_between_the_library_and_the_reference(tbs, mod, Nl, nbits):
    data = payload(tbs, 1)
    ours_first, theirs_first, theirs = (Harq(110, tbs, mod, nbits, Nl) for _ in range(3))
    assert theirs.encode(False, 0, data)[0] == 0
    want = theirs.encode(False, 2, None)
    assert want[0] == 0
    assert ours_first.encode(True, 0, data)[0] == 0
    same_e(ours_first.encode(False, 2, None), want, nbits, "rv 0 by the library, rv 2 by the reference")
    assert theirs_first.encode(False, 0, data)[0] == 0
    same_e(theirs_first.encode(True, 2, None), want, nbits, "rv 0 by the reference, rv 2 by the library")
    for h in (ours_first, theirs_first, theirs):
        h.free()


def test_dlsch_encode_is_encode2_of_codeword_0_on_one_layer():
    tbs, mod, _, nbits = CASES[1]
    data = payload(tbs, 2)
    a, b = Harq(110, tbs, mod, nbits), Harq(110, tbs, mod, nbits)
    same_e(a.encode(True, 0, data, "srslte_dlsch_encode"), b.encode(True, 0, data), nbits, "srslte_dlsch_encode")
    assert np.array_equal(a.w(1, 1177), b.w(1, 1177))
    a.free()
    b.free()


def stats():
    out = (C.c_ulonglong * 4)()
    hip().srslte_hip_compat_stats(out)
    return list(out)


def test_refusals_leave_the_buffers_alone_and_are_not_counted():
    served = stats()[3]

    def refused(h, rv, data, want, C_=2):
        for c in range(min(C_, h.max_cb())):
            h.w(c, 2400)[:] = 0x5A
        rc, e = h.encode(True, rv, data)
        assert rc == want, (rc, want)
        assert np.all(e == FILL)
        assert all(np.all(h.w(c, 2400) == 0x5A) for c in range(min(C_, h.max_cb())))

    data = payload(6200)
    h = Harq(110, 4016, QPSK, 3000)  # filler bits: upstream's refusal (sch.c:194-197)
    assert seg(4016).F > 0
    refused(h, 0, data, -1)
    rc, e = h.encode(False, 0, data)
    assert rc == -1 and np.all(e == FILL)
    h.free()
    h = Harq(110, 6136, QPSK, 3000)  # two block lengths without filler bits: this library's refusal
    assert seg(6136).C2 > 0 and seg(6136).F == 0
    refused(h, 0, data, -2)
    h.free()
    h = Harq(110, 6200, QPSK, 3002)
    refused(h, 4, data, -2)
    refused(h, 0, None, -2)
    h.free()
    h = Harq(6, 6200, QPSK, 3002)  # a soft buffer of fewer blocks than the transport block has
    assert h.max_cb() < 2
    refused(h, 0, data, -1)
    assert h.encode(False, 0, data)[0] == -1
    h.free()
    h = Harq(110, 0, QPSK, 3002)  # no transport block: success, nothing written
    for d in (data, None):
        h.w(0, 2400)[:] = 0x5A
        rc, e = h.encode(True, 0, d)
        assert rc == 0 and np.all(e == FILL) and np.all(h.w(0, 2400) == 0x5A)
    h.free()
    assert stats()[3] == served


def test_operator_interface_refusals():
    pkg = importlib.import_module("srslte-emane_amd")
    enc = pkg.SchEnc(6200, 4000)
    data = payload(6200)[:6200 // 8]
    w = [np.full(2400, 0x5A, np.uint8) for _ in range(2)]
    ok = dict(data=data, tbs=6200, mod=QPSK, Nl=1, rv=0, nof_e_bits=3002)
    for change in (dict(mod=0), dict(mod=5), dict(Nl=0), dict(Nl=3), dict(rv=4), dict(tbs=6204, data=payload(6208)), dict(tbs=6712, data=payload(6712)),
                   dict(nof_e_bits=0), dict(nof_e_bits=4001), dict(data=None), dict(tbs=6136)):
        rc, e = enc.encode(buffer_b=w, **dict(ok, **change))
        assert rc == -2 and e is None and all(np.all(x == 0x5A) for x in w), change
    rc, e = enc.encode(buffer_b=w, **dict(ok, tbs=4016))
    assert rc == -1 and e is None and all(np.all(x == 0x5A) for x in w)
    rc, e = enc.encode(buffer_b=w, **dict(ok, tbs=0))
    assert rc == 0 and e is None and all(np.all(x == 0x5A) for x in w)
    rc, e = enc.encode(buffer_b=w, **ok)
    ref_h = Harq(110, 6200, QPSK, 3002)
    want = ref_h.encode(False, 0, payload(6200))
    assert rc == 0 and want[0] == 0 and np.array_equal(e, bits(want[1], 3002))
    assert all(np.array_equal(bits(w[c], 3 * 3136 + 12), bits(ref_h.w(c, 2400), 3 * 3136 + 12)) for c in range(2))
    ref_h.free()
    enc.free()
    for bad in ((0, 100), (104, 0)):
        with pytest.raises(RuntimeError):
            pkg.SchEnc(*bad)


def sizes_in_turn(errors):
    """small, large, small on the calling thread: its encoder object is made, replaced by a larger one, and used below its size"""
    try:
        before = stats()[3]
        for tbs, mod, Nl, nbits in (CASES[0], CASES[5], CASES[0]):
            data = payload(tbs, 3)
            a, b = Harq(110, tbs, mod, nbits, Nl), Harq(110, tbs, mod, nbits, Nl)
            for rv in (0, 2):
                same_e(a.encode(True, rv, data), b.encode(False, rv, data), nbits, (tbs, rv))
            a.free()
            b.free()
        if threading.current_thread() is threading.main_thread():
            assert stats()[3] == before + 6  # the counter: every call the device served, no other
    except BaseException as ex:  # noqa: B902 - handed to the test's own thread
        errors.append(ex)


def test_the_thread_s_encoder_object_grows_and_is_reused_and_calls_are_counted():
    errors = []
    sizes_in_turn(errors)
    assert not errors, errors
    t = threading.Thread(target=sizes_in_turn, args=(errors,))
    t.start()
    t.join()
    assert not errors, errors
