"""Inputs the silent-capture and zero-parity tests share (test_silent_oracle.py, test_gpu_silent.py, test_gpu_zero_parity.py): nothing here is
part of the product.

* A silent capture is a subframe of exact zeros, what an emulator hands over when nobody transmits. The estimators return noise_estimate 0,
  the equaliser computes 0 / 0, every float-to-integer conversion behind it gets a NaN. The reference's answer is that of its x86 build:
  _mm_cvtps_epi32 / _mm_cvttps_epi32 return 0x80000000 for a NaN and for every value out of range, the saturating packs make -32768 / -128
  of it, the scalar tails truncate it to 0 (oracle/orc_modem.c cvt_rne / cvt_trunc).
* A zero-parity transport block is one whose CRC24A is 0: sch.c:482 reports `par_rx == par_tx && par_rx`, so it fails although every
  code-block CRC passes and the bytes are those that were sent. Two constructions: an all-zero payload, and tbs/8 - 3 random bytes followed
  by their own CRC24A (a block followed by its CRC has CRC 0)."""
import ctypes as C
import os

import numpy as np

from _libs import OrcSchCfg, oracle, p
from lte_sim import DlConfig, UlConfig, make_pmch_subframe, make_subframe, make_ul_subframe, oracle_pmch_rx, oracle_rx, oracle_ul_rx

AMP = 0.1
# components the symbols of symbol_set() cycle through: | value x demapper gain | >= 2^31 for the first five (the gains are 20 .. 1000), 1e7 is
# in range of the conversion and out of range of the 16- and 8-bit packs behind it
NONFINITE = np.array([np.nan, np.inf, -np.inf, 3e9, -3e9, 1e7, -1e7, 0.0], np.float32)

# the shared-channel shapes (tests/test_gpu_sch_fixed.py): name -> (configuration, first TTI of a batch)
DL_SHAPES = {"K352": (lambda **kw: DlConfig(6, 1, 1, 328, cfi=3, **kw), 4),                 # C = 1, K = 352: the unwindowed decoder, tb_crc_kernel
             "K832": (lambda **kw: DlConfig(6, 7, 1, 808, cfi=3, cp_ext=True, **kw), 1),    # one windowed block, compact parity layout
             "C2": (lambda **kw: DlConfig(50, 150, 1, 9912, cfi=3, **kw), 4)}               # C = 2, K = 4992, compact parity layout
UL_SHAPES = {"K352": lambda: UlConfig(15, 11, 1, 328, 3, 12, n_dmrs=3, cyclic_shift=2, delta_ss=5),
             "K4032": lambda: UlConfig(25, 11, 2, 4008, 10, 5, n_dmrs=3, cyclic_shift=2, delta_ss=5)}
DL_CK = {"K352": (1, 352), "K832": (1, 832), "C2": (2, 4992)}
UL_CK = {"K352": (1, 352), "K4032": (1, 4032)}


def symbol_set(nsym, start=0):
    """nsym symbols whose components (re, im, re, ...) cycle through NONFINITE from position `start`"""
    return NONFINITE[(start + np.arange(2 * nsym)) % len(NONFINITE)].view(np.complex64).copy()


def nan_symbols(nsym):
    return np.full(2 * nsym, np.nan, np.float32).view(np.complex64)


def crc24a(data, nbits):
    d = np.ascontiguousarray(data, np.uint8)
    return int(oracle().orc_crc_bytes(0x1864CFB, 24, p(d), nbits))


def zero_parity_payload(tbs, how, rng):
    """how "zeros": the all-zero payload; "crc": tbs/8 - 3 random bytes and their CRC24A. Either way crc24a(payload, tbs) == 0."""
    n = tbs // 8
    d = np.zeros(n, np.uint8)
    if how == "crc":
        d[:n - 3] = rng.integers(0, 256, n - 3, dtype=np.uint8)
        c = crc24a(d[:n - 3], tbs - 24)
        d[n - 3:] = (c >> 16) & 255, (c >> 8) & 255, c & 255
    else:
        assert how == "zeros"
    assert crc24a(d, tbs) == 0
    return d


def random_payload(tbs, rng):
    """a payload whose CRC24A is not zero (one in 2^24 random ones is)"""
    while True:
        d = rng.integers(0, 256, tbs // 8, dtype=np.uint8)
        if crc24a(d, tbs):
            return d


def same_floats(a, b, rtol, what=""):
    """NaN matches NaN, an infinity matches the infinity of its sign, finite figures to rtol (relative to the larger of 1 and |b|)"""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    assert a.shape == b.shape, what
    assert np.array_equal(np.isnan(a), np.isnan(b)), (what, a, b)
    assert np.array_equal(np.isposinf(a), np.isposinf(b)) and np.array_equal(np.isneginf(a), np.isneginf(b)), (what, a, b)
    f = np.isfinite(b)
    assert (np.abs(a[f] - b[f]) <= rtol * np.maximum(1.0, np.abs(b[f]))).all(), (what, a, b)


# ---------------------------------------------------------------------------------------------------------- the fixed-grant pipelines
# The pipelines' back ends are judged by the oracle's back end on the DEVICE's own LLRs (and gains): what is compared exactly then does not
# depend on the last bit of the FFT in front of the demapper.
def w_len(K, llr8):
    """length of a block's soft buffer: the input layout of the decoder the reference selects for K (turbodecoder.c:394-436)"""
    orc = oracle()
    fn = orc.orc_tdec_autoimp_subblocks_8bit if llr8 else orc.orc_tdec_autoimp_subblocks
    fn.restype = C.c_uint32
    return 3 * (K + 32) + 12 if fn(K) else 3 * K + 12


class DlPipe:
    """One fixed-grant DL configuration: how to make its objects and subframes, read its views and ask the oracle."""

    def __init__(self, hp, cfg, tti0, pmch=False):
        self.hp, self.cfg, self.tti0, self.pmch = hp, cfg, tti0, pmch
        self.llr8 = getattr(cfg, "llr8", False)
        self.dt = np.int8 if self.llr8 else np.int16
        self.C, self.K = cfg.seg.C, cfg.seg.K1
        self.n = w_len(self.K, self.llr8)
        self.stride = (self.n + 31) & ~31
        self.csi = getattr(cfg, "csi", False)
        self.silent = np.zeros(cfg.nof_rx * cfg.sf_len, np.complex64)

    def rx(self, nsf, compact=True):
        cfg, hp = self.cfg, self.hp
        hc = hp.ChestDlCfg()
        hc.filter_coef[0], hc.filter_coef[1] = 4.0, 1.0
        old = os.environ.pop("SRSLTE_HIP_PARITY_COMPACT", None)
        try:
            if not compact:
                os.environ["SRSLTE_HIP_PARITY_COMPACT"] = "0"  # read when the object is created
            if self.pmch:
                return hp.DlRx(cfg.cell_id, cfg.nof_prb, cfg.cfi, 0, cfg.mod, cfg.tbs, 6, nsf, True, hc, cp_ext=cfg.cp_ext, mbsfn=(cfg.area_id, cfg.non_mbsfn_region))
            return hp.DlRx(cfg.cell_id, cfg.nof_prb, cfg.cfi, cfg.rnti, cfg.mod, cfg.tbs, 6, nsf, True, hc, llr_8bit=cfg.llr8, nof_rx=cfg.nof_rx,
                           nof_ports=cfg.nof_ports, csi=cfg.csi, cp_ext=cfg.cp_ext)
        finally:
            os.environ.pop("SRSLTE_HIP_PARITY_COMPACT", None)
            if old is not None:
                os.environ["SRSLTE_HIP_PARITY_COMPACT"] = old

    def live(self, tti, rng, rv=0, data=None):
        if data is None:
            data = random_payload(self.cfg.tbs, rng)
        if self.pmch:
            return make_pmch_subframe(self.cfg, tti, rng, amp=AMP, data=data)[0].ravel(), data
        return make_subframe(self.cfg, tti, rng, amp=AMP, rv=rv, data=data)[0].ravel(), data

    def nbits(self, tti):
        return self.cfg.nbits if self.pmch else len(self.cfg.indices(tti % 10)) * self.cfg.Qm

    def views(self, rx, nsf, tti0):
        """per row: [LLRs, gains (csi) or None, soft buffer with its padding, pass counts, block flags]"""
        e = rx.debug(4, self.dt, nsf * rx.e_stride).reshape(nsf, rx.e_stride)
        w = rx.debug(5, self.dt, nsf * self.C * self.stride).reshape(nsf, self.C, self.stride)
        it, ok = rx.debug(6, np.uint32, nsf * self.C).reshape(nsf, self.C), rx.debug(7, np.uint8, nsf * self.C).reshape(nsf, self.C)
        max_re = max(rx.nof_re(s) for s in (0, 1, 5))
        g = rx.debug(9, np.float32, nsf * max_re).reshape(nsf, max_re) if self.csi else None
        out = []
        for b in range(nsf):
            nb = self.nbits(tti0 + b)
            out.append([e[b, :nb].copy(), None if g is None else g[b, :nb // self.cfg.Qm].copy(), w[b].copy(), it[b].copy(), ok[b].copy()])
        return out

    def oracle_front(self, iq, tti):
        """the oracle chain's LLRs before the CSI weighting (and its gains)"""
        if self.pmch:
            r = oracle_pmch_rx(self.cfg, iq, tti, keep=True)
            return r["e"], None
        r = oracle_rx(self.cfg, iq, tti, keep=True)
        return r["e_raw"], r["csi"] if self.csi else None

    def oracle_back(self, llr, gains, tti, harq, rv=0, new_data=True):
        """the oracle's CSI weighting, rate de-matcher, turbo decoder and CRCs on given LLRs, into harq"""
        cfg, orc = self.cfg, oracle()
        e = np.ascontiguousarray(llr).copy()
        nsym = len(e) // cfg.Qm
        if self.csi:
            (orc.orc_csi_correction_b if self.llr8 else orc.orc_csi_correction_s)(p(e), p(np.ascontiguousarray(gains, np.float32)), nsym, cfg.mod)
        sch = OrcSchCfg(cfg.tbs, len(e), getattr(cfg, "Qm_sch", cfg.Qm), rv, 6)
        tb, it, ok = np.zeros(cfg.tbs // 8 + 16, np.uint8), np.zeros(self.C, np.uint32), np.zeros(self.C, np.uint8)
        rc = orc.orc_dlsch_decode_harq(C.byref(sch), p(e), 1 if self.llr8 else 0, 1 if new_data else 0, p(harq.w), p(harq.crc), p(harq.data), p(tb), p(it), p(ok))
        return tb[:cfg.tbs // 8 + 3], rc == 0, it, ok

    def new_harq(self):
        class H:
            pass
        h = H()
        h.w = np.zeros(self.C * oracle().orc_harq_softbuffer_stride(), np.int16)
        h.crc, h.data = np.zeros(self.C, np.uint8), np.zeros(self.C * 768, np.uint8)
        return h

    def harq_w(self, h):
        st = oracle().orc_harq_softbuffer_stride()
        rows = h.w.reshape(self.C, st)
        return np.stack([rows[c].view(np.int8)[:self.n] if self.llr8 else rows[c, :self.n] for c in range(self.C)])

    def decode(self, rx, iq, tti0):
        return rx.decode(iq, tti0)

    def decode_harq(self, rx, iq, tti0, rv, new):
        return rx.decode_harq(iq, tti0, rv, new)


class UlPipe(DlPipe):
    def __init__(self, hp, cfg, tti0):
        self.hp, self.cfg, self.tti0, self.pmch = hp, cfg, tti0, False
        self.llr8, self.dt, self.csi = False, np.int16, False
        self.C, self.K = cfg.seg.C, cfg.seg.K1
        self.n = w_len(self.K, False)
        self.stride = (self.n + 31) & ~31
        self.silent = np.zeros(cfg.sf_len, np.complex64)

    def rx(self, nsf, compact=True):
        cfg = self.cfg
        return self.hp.UlRx(cfg.cell_id, cfg.nof_prb, cfg.rnti, cfg.mod, cfg.tbs, cfg.L_prb, cfg.n_prb, cfg.n_dmrs, 6, nsf, cfg.dmrs_cfg.cyclic_shift,
                            cfg.dmrs_cfg.delta_ss)

    def live(self, tti, rng, rv=0, data=None):
        if data is None:
            data = random_payload(self.cfg.tbs, rng)
        return make_ul_subframe(self.cfg, tti, rng, amp=AMP, rv=rv, data=data)[0], data

    def views(self, rx, nsf, tti0):
        nb = self.cfg.nbits
        g = rx.debug(4, np.int16, nsf * nb).reshape(nsf, nb)
        w = rx.debug(5, np.int16, nsf * self.C * self.stride).reshape(nsf, self.C, self.stride)
        it, ok = rx.debug(6, np.uint32, nsf * self.C).reshape(nsf, self.C), rx.debug(7, np.uint8, nsf * self.C).reshape(nsf, self.C)
        return [[g[b].copy(), None, w[b].copy(), it[b].copy(), ok[b].copy()] for b in range(nsf)]

    def oracle_front(self, iq, tti):
        return oracle_ul_rx(self.cfg, iq, tti, keep=True)["g"], None


def same_row(a, b, what):
    assert len(a) == len(b)
    for n, (x, y) in enumerate(zip(a, b)):
        assert (x is None and y is None) or np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), (what, n)


def row_of(P, rx, res, b, nsf, tti0):
    """everything the object holds of row b after a call: bytes, verdict and the views"""
    tb, ok = res
    return [tb[b].copy(), ok[b:b + 1].copy()] + P.views(rx, nsf, tti0)[b]


def check_against_oracle(P, row, tti, harq, rv=0, new_data=True, what=""):
    """row (from row_of) against the oracle's back end on the row's own LLRs: verdict, pass counts, block flags, soft buffer and bytes.
    The bytes are left out where this call decoded no block at all: upstream then copies every block from its soft buffer's data array,
    which it only writes after a call in which some block FAILED (sch.c:404-412) - after a call whose blocks all passed it holds whatever it
    held before (zeros in the oracle's), and the verdict is 0 whatever the bytes are."""
    tb, ok, it, cbok = P.oracle_back(row[2], row[3], tti, harq, rv, new_data)
    assert bool(row[1][0]) == ok and np.array_equal(row[5], it) and np.array_equal(row[6], cbok), (what, row[1], ok, row[5], it, row[6], cbok)
    if it.any():
        assert np.array_equal(row[0], tb), (what, "bytes")
    else:
        assert not ok, what
    assert np.array_equal(row[4][:, :P.n], P.harq_w(harq)), (what, "soft buffer")
    return ok, it, cbok


# ---------------------------------------------------------------------------------------------------------------- the ragged batches
# One grant per subframe, every decoder kind of the mixed launch (tdec_run_groups: K <= 400 generic, 400 < K <= 800 the 8-window body,
# above that the pair body) and a two-block grant: (first PRB, PRBs, TBS) on a 50-PRB cell with CFI 3, QPSK.
DL_RAGGED = ((0, 3, 328), (10, 7, 808), (0, 50, 9912), (30, 6, 776))
DL_RAGGED_CK = [(1, 352), (1, 832), (2, 4992), (1, 800)]
# (L_prb, n_prb, mod, TBS, n_dmrs) on a 25-PRB cell
UL_RAGGED = ((3, 20, 1, 328, 5), (10, 0, 2, 4008, 0), (12, 8, 3, 7992, 7), (4, 14, 1, 776, 2))
UL_RAGGED_CK = [(1, 352), (1, 4032), (2, 4032), (1, 800)]
UL_RAGGED_DMRS = dict(cyclic_shift=2, delta_ss=5, group_hopping=True, sequence_hopping=False)


def dl_ragged_cfgs(llr8=False):
    cfgs = []
    for b, (first, n, tbs) in enumerate(DL_RAGGED):
        m = np.zeros((2, 50), np.uint8)
        m[:, first:first + n] = 1
        cfgs.append(DlConfig(50, 150, 1, tbs, cfi=3, rnti=0x100 + b, llr8=llr8, prb_mask=m))
    assert [(c.seg.C, c.seg.K1) for c in cfgs] == DL_RAGGED_CK
    return cfgs


def ul_ragged_cfgs():
    cfgs = [UlConfig(25, 11, mod, tbs, L, n0, n_dmrs=nd, rnti=0x100 + b, **UL_RAGGED_DMRS) for b, (L, n0, mod, tbs, nd) in enumerate(UL_RAGGED)]
    assert [(c.seg.C, c.seg.K1) for c in cfgs] == UL_RAGGED_CK
    return cfgs


GRANTS_W_STRIDE = (3 * (6144 + 32) + 12 + 31) & ~31  # a block slot of the grants modes' soft buffer: the longest block's layout


def dl_grants_views(rx, cfgs, tti0, llr8=False):
    """the grants mode's views after a call of len(cfgs) grants (one per subframe), per row: [LLRs, None, soft buffer [C][stride], pass counts,
    block flags] - the middle of a row_of() row; block slot c of row b is slot b * Cmax + c"""
    n, dt = len(cfgs), np.int8 if llr8 else np.int16
    cmax = max(c.seg.C for c in cfgs)
    stride = 16 * ((14 * 12 * cfgs[0].nof_prb * 8 + 15) // 16)
    e = rx.debug(11, dt, n * stride).reshape(n, stride)
    w = rx.debug(12, dt, n * cmax * GRANTS_W_STRIDE).reshape(n, cmax, GRANTS_W_STRIDE)
    it, cb = rx.debug(13, np.uint32, n * cmax).reshape(n, cmax), rx.debug(14, np.uint8, n * cmax).reshape(n, cmax)
    out = []
    for b, c in enumerate(cfgs):
        nb = len(c.indices((tti0 + b) % 10)) * c.Qm
        out.append([e[b, :nb].copy(), None, w[b, :c.seg.C].copy(), it[b, :c.seg.C].copy(), cb[b, :c.seg.C].copy()])
    return out


def blur_symbols(cfg, iq, other, symbols):
    """iq with the OFDM symbols `symbols` (0 .. 13, normal CP) replaced by the mean of iq and other: two noise-free subframes of one cell and
    TTI share their CRS, so the estimates stay, and where the two payloads' QPSK symbols differ a component cancels - half the LLRs of those
    symbols are erased, the others keep their sign"""
    N = cfg.N
    cp0, cp = 160 * N // 2048, 144 * N // 2048
    out = np.array(iq, np.complex64)
    for l in symbols:
        s, ls = divmod(l, 7)
        a = s * (7 * N + cp0 + 6 * cp) + (0 if ls == 0 else cp0 + N + (ls - 1) * (cp + N))
        n = N + (cp0 if ls == 0 else cp)
        out[a:a + n] = 0.5 * (out[a:a + n] + other[a:a + n])
    return out
