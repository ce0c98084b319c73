"""srslte_hip_pusch_decode (phy_hip.h) and the exported srslte_pusch_decode on top of it (srslte_compat_pusch.h), through the C ABI: one PUSCH's grid
and channel estimates from the host, one visit of the device. Cases, stimulus and expectation: tests/pusch_decode_cases.py (lte_sim's oracle).

Held to the oracle: the descrambled LLRs through the debug accessor within 1 LSB on at most 1e-3 of them - the bound tests/test_gpu_ul_grants.py and
test_gpu_ul_harq.py hold the batched pipeline to -, and exactly: the CRC verdict, the transport block's bytes, the ACK / RI decisions, the report's
bits and its CRC flag, the three Q', the flags of every code block and the soft buffers of the blocks that failed. Stream waits: one per call when
every block passes, a second for the soft buffers of failed blocks, one more where the decoded rank sizes the report."""
import ctypes as C
import os

import numpy as np
import pytest

from _libs import ROOT, hip, make_crc, oracle, p, struct_layout
from pusch_decode_abi import FIELDS, UlschRes, pusch_cfg
from pusch_decode_cases import CASES, MAX_ITER, expect, ul_config
from test_gpu_ulsch_decode import CqiValue, PuschCfg, UciValue

pytestmark = pytest.mark.gpu
SB_LEN, FILL = 18600, 0x33  # SOFTBUFFER_SIZE (softbuffer.h:50)
_ly = {}


def H():
    h = hip()
    h.srslte_hip_sch_create.restype = C.c_void_p
    h.srslte_hip_sch_create.argtypes = [C.c_uint32, C.c_uint32, C.c_int]
    h.srslte_hip_sch_destroy.argtypes = [C.c_void_p]
    h.srslte_hip_pusch_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float] + [C.c_void_p] * 6
    h.srslte_hip_pusch_debug_q.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    h.srslte_pusch_decode.argtypes = [C.c_void_p] * 6
    h.srslte_hip_compat_sch_of.restype = C.c_void_p
    h.srslte_hip_compat_sch_of.argtypes = [C.c_void_p]
    return h


def crc24a(d, nbits):
    return int(oracle().orc_crc_bytes(0x1864CFB, 24, p(np.ascontiguousarray(d, np.uint8)), nbits))


def llr_close(mine, theirs, what):
    diff = np.abs(mine.astype(np.int32) - theirs.astype(np.int32))
    print(what, "LLRs: max diff", int(diff.max()), "differing", int((diff != 0).sum()), "of", diff.size)
    assert diff.max() <= 1 and (diff != 0).sum() <= 1e-3 * diff.size, (what, int(diff.max()), int((diff != 0).sum()), diff.size)


class Soft:
    """the arrays of a srslte_softbuffer_rx_t for C blocks, and the array of pointers the device call takes"""

    def __init__(self, nblk):
        self.f = np.zeros((max(nblk, 1), SB_LEN), np.int16)
        self.crc = np.zeros(max(nblk, 1), np.uint8)
        self.data = np.zeros((max(nblk, 1), 768), np.uint8)
        self.ptrs = (C.c_void_p * max(nblk, 1))(*[self.f[c].ctypes.data for c in range(max(nblk, 1))])


class Dev:
    """a srslte_hip_sch_t and one soft buffer, driven as compat.cpp drives them (tb_begin / tb_finish, sch.c:312-412,:461-488)"""

    def __init__(self, max_tbs, max_e, nblk, l8=0):
        self.h = H().srslte_hip_sch_create(max_tbs, max_e, l8)
        assert self.h
        self.sb = Soft(nblk)

    def free(self):
        H().srslte_hip_sch_destroy(self.h)

    def decode(self, c, grid, ce, noise, seg):
        nblk, K = seg.C, seg.K1
        was = self.sb.crc.copy()
        crc, byt, passes, res = self.sb.crc.copy(), np.zeros((max(nblk, 1), 768), np.uint8), C.c_uint32(0xffffffff), UlschRes()
        g, e = np.ascontiguousarray(grid, np.complex64), np.ascontiguousarray(ce, np.complex64)
        rc = H().srslte_hip_pusch_decode(self.h, p(g), p(e), noise, C.byref(c), self.sb.ptrs if nblk else None, p(crc) if nblk else None, p(byt) if nblk else None,
                                         C.byref(passes), C.byref(res))
        out = {"rc": rc, "res": res, "passes": passes.value}
        if rc or nblk == 0:
            return out
        tbs, rlen = c.sch.tbs, (K if nblk == 1 else K - 24) // 8
        tb = np.zeros(tbs // 8 + 3 + K // 8, np.uint8)
        for b in range(nblk):  # decode_tb_cb: a block's K / 8 bytes land where its payload goes, the next block overwrites its CRC
            tb[b * rlen:b * rlen + (rlen if was[b] else K // 8)] = self.sb.data[b][:rlen] if was[b] else byt[b][:K // 8]
        self.sb.crc[:nblk] = crc[:nblk]
        ok = bool(crc[:nblk].all())
        if not ok:
            for b in range(nblk):
                if crc[b]:
                    self.sb.data[b][:rlen] = tb[b * rlen:(b + 1) * rlen]
        else:
            par = crc24a(tb, tbs)
            ok = par != 0 and par == (int(tb[tbs // 8]) << 16 | int(tb[tbs // 8 + 1]) << 8 | int(tb[tbs // 8 + 2]))
        out.update(tb=tb[:tbs // 8 + 3], ok=ok, cb_ok=crc[:nblk].copy())
        return out

    def q(self, n):
        out = np.zeros(n, np.int16)
        assert H().srslte_hip_pusch_debug_q(self.h, p(out), n) == 0
        return out


def hip_cfg(c, ul, t, tti):
    ack, ri, cqi, I = c.get("ack", ()), c.get("ri", ()), c.get("cqi", ()), c.get("I", (0, 0, 0))
    lens = c.get("rank_len", (len(cqi), 0))
    return pusch_cfg(c["P"], 1, c["mod"], c["tbs"], c["L"], c["n_prb"], cp_ext=c.get("ext", False), shortened=c.get("short", False), rnti=ul.rnti, sf_idx=tti % 10,
                     rv=t["rv"], max_iterations=MAX_ITER, ack_len=len(ack), ri_len=len(ri), cqi_len=lens[0], I=I, cqi_len_rank2=lens[1])


@pytest.mark.parametrize("name", list(CASES))
def test_one_pusch_matches_the_oracle(name):
    c = CASES[name]
    ul, txs, data = expect(name)
    seg = ul.seg
    dev = Dev(max(c["tbs"], 40), ul.nbits, seg.C)
    n_len = H().srslte_hip_tdec_input_len(seg.K1, 1 if H().srslte_hip_tdec_autoimp_get_subblocks(seg.K1) else 0) if seg.C else 0
    stride = oracle().orc_harq_softbuffer_stride()
    # In the decoder's window layout a block is three rows of K + 32: the 32 slots behind each row's K LLRs hold nothing the rate de-matcher
    # wrote. Upstream's decoder, which reads the caller's buffer in place, parks the tail LLRs there on its first pass and the library does the
    # same to the caller's buffer (tests/test_gpu_ulsch_decode.py holds that to the reference); the oracle decodes from a copy. Compared: every
    # slot the de-matcher owns, which is all the next transmission combines into.
    owned = np.ones(n_len, bool)
    if seg.C and H().srslte_hip_tdec_autoimp_get_subblocks(seg.K1):
        for r in range(3):
            owned[r * (seg.K1 + 32) + seg.K1:(r + 1) * (seg.K1 + 32)] = False
    for k, t in enumerate(txs):
        fails = k in c.get("fails", ())
        if c["tbs"] and not fails and t["ok"]:  # the oracle alone, at the chosen SNR: at most half of max_iterations for every block
            assert t["iters"].max() <= MAX_ITER // 2, (name, t["iters"])
        assert not (fails and t["ok"]), "this transmission must fail alone"
        m = dev.decode(hip_cfg(c, ul, t, c["tti"]), t["grid"], t["ce"], t["noise"], seg)
        assert m["rc"] == 0, (name, m["rc"])
        llr_close(dev.q(ul.nbits), t["q"], (name, t["rv"]))
        res = m["res"]
        assert (res.Q_prime_ack, res.Q_prime_ri, res.Q_prime_cqi) == t["Qp"], (name, "Q'")
        n_ack, n_ri, n_cqi = len(c.get("ack", ())), len(c.get("ri", ())), len(c.get("cqi", ()))
        assert list(res.ack)[:n_ack] == t["ack"][:n_ack].tolist() == list(c.get("ack", ())), (name, "ACK")
        assert [res.ri][:n_ri] == t["ri"][:n_ri].tolist() == list(c.get("ri", ())), (name, "RI")
        assert res.cqi_len == n_cqi and bool(res.cqi_crc) == t["cqi_ok"] and list(res.cqi_bits)[:n_cqi] == t["cqi"].tolist(), (name, "report")
        if n_cqi:
            assert t["cqi_ok"] and tuple(t["cqi"].tolist()) == tuple(c["cqi"])
        rank_wait = 1 if "rank_len" in c else 0
        if c["tbs"] == 0:
            assert res.stream_waits == 1 + rank_wait
            continue
        assert m["ok"] == t["ok"] and np.array_equal(m["cb_ok"], t["cb_ok"]), (name, "CRC", m["cb_ok"], t["cb_ok"])
        assert np.array_equal(m["tb"], t["tb"]), (name, "bytes")
        if t["ok"]:
            assert np.array_equal(m["tb"][:c["tbs"] // 8], data)
            assert m["passes"] == int(t["iters"].sum())
        for b in range(seg.C):  # the soft buffers of the blocks that failed, as the next transmission combines into them
            if not t["cb_ok"][b]:
                d = np.nonzero((dev.sb.f[b][:n_len] != t["w"][b * stride:b * stride + n_len]) & owned)[0]
                assert d.size == 0, (name, t["rv"], "soft buffer", b, d.size, d[:8].tolist())
        assert res.stream_waits == (1 if t["cb_ok"].all() else 2) + rank_wait, (name, res.stream_waits)
    dev.free()


def test_device_call_refusals_queue_and_write_nothing():
    name = "6prb_L1_qpsk_ack1_cqi4"
    c = CASES[name]
    ul, txs, _ = expect(name)
    t = txs[0]
    dev = Dev(6208, ul.nbits, 2)
    good = lambda: hip_cfg(c, ul, t, c["tti"])  # noqa: E731
    assert dev.decode(good(), t["grid"], t["ce"], t["noise"], ul.seg)["ok"]
    q0, f0 = dev.q(ul.nbits), dev.sb.f.copy()
    dev.sb.crc[:] = 0
    bad = {"transport block beyond the object": lambda x: setattr(x.sch, "tbs", 75376), "filler bits": lambda x: setattr(x.sch, "tbs", 6208),
           "rv": lambda x: setattr(x.sch, "rv", 4), "no passes": lambda x: setattr(x.sch, "max_iterations", 0), "ri_len": lambda x: setattr(x.sch, "ri_len", 3),
           "report of 65 bits": lambda x: setattr(x.sch, "cqi_len", 65), "offset": lambda x: setattr(x.sch, "I_offset_ack", 16),
           "L_prb": lambda x: setattr(x.sch, "L_prb", 7), "slot 1 beyond the cell": lambda x: x.n_prb_tilde.__setitem__(1, 6), "nof_re": lambda x: setattr(x, "nof_re", 132),
           "shortened": lambda x: setattr(x, "shortened", 1), "256QAM": lambda x: setattr(x.sch, "mod", 4)}
    for what, change in bad.items():
        x = good()
        change(x)
        res = UlschRes()
        C.memset(C.byref(res), FILL, C.sizeof(res))
        crc, byt = np.zeros(2, np.uint8), np.full((2, 768), FILL, np.uint8)
        rc = H().srslte_hip_pusch_decode(dev.h, p(t["grid"]), p(t["ce"]), t["noise"], C.byref(x), dev.sb.ptrs, p(crc), p(byt), None, C.byref(res))
        assert rc == -2, (what, rc)
        assert bytes(res) == bytes([FILL]) * C.sizeof(res) and crc[0] == 0 and np.all(byt == FILL) and np.array_equal(dev.sb.f, f0), what
        assert np.array_equal(dev.q(ul.nbits), q0), (what, "the LLRs of the last served call are still there")
    l8 = Dev(40, ul.nbits, 1, l8=1)  # an object made for 8-bit LLRs
    assert l8.decode(good(), t["grid"], t["ce"], t["noise"], ul.seg)["rc"] == -2
    l8.free()
    assert dev.decode(good(), t["grid"], t["ce"], t["noise"], ul.seg)["ok"]  # and the object still serves
    dev.free()


# ---------------------------------------------------------------------------------------------------- the exported srslte_pusch_decode
class SoftbufferRx(C.Structure):
    _fields_ = [("max_cb", C.c_uint32), ("buffer_f", C.c_void_p), ("data", C.c_void_p), ("cb_crc", C.c_void_p), ("tb_crc", C.c_bool)]


class UlSf(C.Structure):
    _fields_ = [("sf_config", C.c_uint32), ("ss_config", C.c_uint32), ("configured", C.c_bool), ("tti", C.c_uint32), ("shortened", C.c_bool)]


class ChestUlRes(C.Structure):
    _fields_ = [("ce", C.c_void_p), ("nof_re", C.c_uint32)] + [(n, C.c_float) for n in ("noise_estimate", "noise_estimate_dbm", "snr", "snr_db", "cfo")]


class PuschRes(C.Structure):
    _fields_ = [("data", C.c_void_p), ("uci", UciValue), ("crc", C.c_bool), ("avg_iterations_block", C.c_float)]


def layout():
    if not _ly:
        _ly.update(struct_layout(FIELDS, ["srslte_hip/srslte_compat_pusch.h"], [os.path.join(ROOT, "include")]))
        assert C.sizeof(UlSf) == _ly["srslte_ul_sf_cfg_t"] and UlSf.tti.offset == _ly["srslte_ul_sf_cfg_t.tti"] and UlSf.shortened.offset == _ly["srslte_ul_sf_cfg_t.shortened"]
        assert C.sizeof(ChestUlRes) == _ly["srslte_chest_ul_res_t"] and ChestUlRes.snr_db.offset == _ly["srslte_chest_ul_res_t.snr_db"]
        assert C.sizeof(PuschRes) == _ly["srslte_pusch_res_t"] and PuschRes.crc.offset == _ly["srslte_pusch_res_t.crc"]
    return _ly


class Enb:
    """a srslte_pusch_t as srslte_pusch_init_enb + srslte_pusch_set_cell leave the fields the library reads: the cell, llr_is_8bit, and in ul_sch the
    decoder (the library's srslte_tdec_init), both CRC tables and max_iterations. The scratch pointers stay NULL: the call must not touch them."""

    def __init__(self, P, ext, nblk):
        L = self.L = layout()
        self.q = (C.c_uint8 * (L["srslte_pusch_t"] + 64))()
        self.b = np.frombuffer(self.q, np.uint8)
        cell = L["srslte_pusch_t.cell"]
        for f, v in (("nof_prb", P), ("nof_ports", 1), ("id", 1), ("cp", 1 if ext else 0)):
            self.b[cell + L["srslte_cell_t." + f]:][:4].view(np.uint32)[0] = v
        self.sch = L["srslte_pusch_t.ul_sch"]
        assert H().srslte_tdec_init(C.c_void_p(C.addressof(self.q) + self.sch + L["srslte_sch_t.decoder"]), 6144) == 0
        for f, poly in (("crc_tb", 0x1864CFB), ("crc_cb", 0x1800063)):
            crc = make_crc(poly, 24)
            C.memmove(C.addressof(self.q) + self.sch + L["srslte_sch_t." + f], C.byref(crc), C.sizeof(crc))
        self.b[self.sch + L["srslte_sch_t.max_iterations"]:][:4].view(np.uint32)[0] = MAX_ITER
        self.sb = Soft(nblk)
        n = max(nblk, 1)
        self.dptr = (C.c_void_p * n)(*[self.sb.data[c].ctypes.data for c in range(n)])
        self.crcb = np.zeros(n, np.bool_)
        self.sbrx = SoftbufferRx(n, C.addressof(self.sb.ptrs), C.addressof(self.dptr), self.crcb.ctypes.data, False)

    def free(self):
        H().srslte_tdec_free(C.c_void_p(C.addressof(self.q) + self.sch + self.L["srslte_sch_t.decoder"]))

    def handle(self):
        return H().srslte_hip_compat_sch_of(C.c_void_p(C.addressof(self.q) + self.sch))

    def cfg(self, c, ul, rv=0, mod=None):
        x = PuschCfg()
        x.rnti = ul.rnti
        g = x.grant
        g.L_prb, g.nof_re, g.nof_symb = ul.L_prb, ul.nof_re, ul.nsymb
        g.n_prb[0], g.n_prb[1] = g.n_prb_tilde[0], g.n_prb_tilde[1] = c["n_prb"]
        g.tb.mod, g.tb.tbs, g.tb.rv, g.tb.enabled = mod or c["mod"], c["tbs"], rv, True
        g.tb.nof_bits = ul.nof_re * 2 * (mod or c["mod"])
        x.uci_offset.I_offset_ack, x.uci_offset.I_offset_ri, x.uci_offset.I_offset_cqi = c.get("I", (0, 0, 0))
        x.uci_cfg.ack[0].nof_acks = len(c.get("ack", ()))
        x.uci_cfg.cqi.ri_len = len(c.get("ri", ()))
        if len(c.get("cqi", ())) == 4:
            x.uci_cfg.cqi.data_enable, x.uci_cfg.cqi.type = True, 0  # wideband
        x.enable_64qam = True
        x.softbuffers = C.addressof(self.sbrx)
        return x

    def decode(self, x, c, t, tti, snr_db=10.0, sf=None, ch=None, grid=None):
        sf = sf if sf is not None else UlSf(0, 0, False, tti, c.get("short", False))
        ce = np.ascontiguousarray(t["ce"], np.complex64)
        ch = ch if ch is not None else ChestUlRes(ce.ctypes.data, ce.size, t["noise"], 0.0, 0.0, snr_db, 0.0)
        out = PuschRes()
        C.memset(C.byref(out), FILL, C.sizeof(out))
        self.data = np.full(c["tbs"] // 8 + 3 + 768, FILL, np.uint8)
        out.data = self.data.ctypes.data
        g = np.ascontiguousarray(t["grid"] if grid is None else grid, np.complex64)
        rc = H().srslte_pusch_decode(self.q, C.byref(sf), C.byref(x), C.byref(ch), p(g), C.byref(out))
        return rc, out


def stats_pusch():
    out = (C.c_ulonglong * 2)()
    hip().srslte_hip_compat_stats_pusch(out)
    return out[0], out[1]


def test_the_exported_call_leaves_what_upstream_leaves():
    name = "6prb_L1_qpsk_ack1_cqi4"
    c = CASES[name]
    ul, txs, data = expect(name)
    t, enb = txs[0], Enb(c["P"], False, 1)
    x = enb.cfg(c, ul)
    x.meas_time_en = True
    scratch = bytes(enb.b[enb.L["srslte_pusch_t.ce"]:enb.L["srslte_pusch_t.mod"]])
    s0 = stats_pusch()
    rc, out = enb.decode(x, c, t, c["tti"], snr_db=-0.5)
    s1 = stats_pusch()
    assert rc == 0 and out.crc and (s1[0] - s0[0], s1[1] - s0[1]) == (1, 1)
    assert np.array_equal(enb.data[:c["tbs"] // 8 + 3], t["tb"]) and np.array_equal(enb.data[:c["tbs"] // 8], data)
    assert out.uci.ack.ack_value[0] == 1 and out.uci.ack.valid and out.uci.cqi.wideband.wideband_cqi == 0b1011 and out.uci.cqi.data_crc
    assert bytes(out.uci)[0] == FILL, "scheduling_request is not the call's to write"
    assert out.avg_iterations_block == float(t["iters"].sum()) and x.last_O_cqi == 4 and x.K_segm == ul.seg.K1 and x.meas_time_value < 1000000
    assert enb.sbrx.tb_crc and enb.crcb[0]
    assert bytes(enb.b[enb.L["srslte_pusch_t.ce"]:enb.L["srslte_pusch_t.mod"]]) == scratch, "q->ce / z / d / q / g are pusch.c's scratch"
    llr_close(np.frombuffer(_debug_q(enb, ul.nbits), np.int16), t["q"], name)
    enb.crcb[:] = False
    rc, out = enb.decode(x, c, t, c["tti"], snr_db=-1.5)  # ACK_SNR_TH
    assert rc == 0 and out.crc and not out.uci.ack.valid
    enb.free()


def _debug_q(enb, n):
    out = np.zeros(n, np.int16)
    assert H().srslte_hip_pusch_debug_q(enb.handle(), p(out), n) == 0
    return out.tobytes()


def test_a_64qam_grant_is_limited_to_16qam_when_64qam_is_disabled():
    c = dict(P=6, mod=2, tbs=1544, L=6, n_prb=(0, 0), snr=25.0, tti=9)
    ul = ul_config(c)
    CASES["_limited"] = c
    try:
        _, txs, data = expect("_limited")
    finally:
        del CASES["_limited"]
    assert txs[0]["ok"] and txs[0]["iters"].max() <= MAX_ITER // 2
    enb = Enb(6, False, 1)
    x = enb.cfg(c, ul, mod=3)
    x.enable_64qam = False
    assert x.grant.tb.nof_bits == ul.nof_re * 6
    rc, out = enb.decode(x, c, txs[0], c["tti"])
    assert rc == 0 and out.crc and np.array_equal(enb.data[:c["tbs"] // 8], data)
    assert x.grant.tb.mod == 2 and x.grant.tb.nof_bits == ul.nof_re * 4  # pusch.c:445-450
    llr_close(np.frombuffer(_debug_q(enb, ul.nbits), np.int16), txs[0]["q"], "limited")
    enb.free()


def test_refusals_of_the_exported_call_touch_nothing():
    name = "15prb_ext_L9"
    c = CASES[name]
    ul, txs, _ = expect(name)
    t, enb = txs[0], Enb(c["P"], True, 1)
    L = enb.L
    assert enb.decode(enb.cfg(c, ul), c, t, c["tti"])[1].crc
    enb.crcb[:] = False
    enb.sbrx.tb_crc = False
    enb.sb.f[:] = 7
    s0 = stats_pusch()

    def g(f, v):
        return lambda x: setattr(x.grant, f, v)
    bad = {"L_prb without a transform": (g("L_prb", 7), {}), "slot 0 beyond the cell": (lambda x: x.grant.n_prb_tilde.__setitem__(0, 7), {}),
           "slot 1 beyond the cell": (lambda x: x.grant.n_prb_tilde.__setitem__(1, 7), {}), "nof_re": (g("nof_re", ul.nof_re - 12), {}),
           "nof_symb": (g("nof_symb", 9), {}), "shortened subframe, 10 symbols": (lambda x: None, {"sf": UlSf(0, 0, False, c["tti"], True)}),
           "nof_bits": (lambda x: setattr(x.grant.tb, "nof_bits", ul.nbits - 4), {}), "BPSK": (lambda x: setattr(x.grant.tb, "mod", 0), {}),
           "256QAM": (lambda x: setattr(x.grant.tb, "mod", 4), {}), "filler bits": (lambda x: setattr(x.grant.tb, "tbs", 6208), {}),
           "ri_len": (lambda x: setattr(x.uci_cfg.cqi, "ri_len", 3), {}), "offset": (lambda x: setattr(x.uci_offset, "I_offset_ri", 16), {}),
           "no soft buffer": (lambda x: setattr(x, "softbuffers", None), {}), "no estimates": (lambda x: None, {"ch": ChestUlRes(None, 0, 0.0, 0.0, 0.0, 10.0, 0.0)}),
           "8-bit LLRs": (lambda x: None, {"l8": True}), "neither data nor a report": (lambda x: setattr(x.grant.tb, "tbs", 0), {})}
    for what, (change, kw) in bad.items():
        x = enb.cfg(c, ul)
        change(x)
        l8 = kw.pop("l8", False)
        enb.b[L["srslte_pusch_t.llr_is_8bit"]] = 1 if l8 else 0
        before = bytes(x)
        rc, out = enb.decode(x, c, t, c["tti"], **kw)
        enb.b[L["srslte_pusch_t.llr_is_8bit"]] = 0
        assert rc == -2, (what, rc)
        o = bytes(out)
        assert o[8:] == bytes([FILL]) * (len(o) - 8) and np.all(enb.data == FILL), (what, "out")
        assert bytes(x) == before, (what, "cfg")
        assert np.all(enb.sb.f == 7) and not enb.crcb.any() and not enb.sbrx.tb_crc, (what, "soft buffer")
    assert stats_pusch() == s0
    enb.sb.f[:] = 0
    assert enb.decode(enb.cfg(c, ul), c, t, c["tti"])[1].crc  # and the object still serves
    assert stats_pusch()[0] == s0[0] + 1
    enb.free()


def test_a_silent_grid_returns_cleanly():
    """tests/silent_cases.py: exact zeros, estimates and noise 0 - the equaliser computes 0 / 0; nothing is asserted about the LLRs"""
    name = "last_prbs"
    c = CASES[name]
    ul, txs, _ = expect(name)
    enb = Enb(c["P"], False, 1)
    silent = dict(txs[0], grid=np.zeros_like(txs[0]["grid"]), ce=np.zeros_like(txs[0]["ce"]), noise=0.0)
    s0 = stats_pusch()
    rc, out = enb.decode(enb.cfg(c, ul), c, silent, c["tti"])
    assert rc == 0 and not out.crc  # an all-zero block has CRC 0: its block check passes, the transport block's `par_rx != 0` does not (sch.c:482)
    assert stats_pusch()[0] == s0[0] + 1
    enb.free()
