"""UE CSI feedback, restated (test infrastructure): the measurement of srslte_hip_csi_batch in NumPy float32 with the sampling rule of the
reference's AVX build, wrappers that run the reference's own functions (oracle/_ref/libsrslte_ref.so) on the same estimates, a line-by-line
restatement of srslte_ue_dl_gen_cqi_periodic / _aperiodic (ue_dl.c:802-928), and the channels the tests draw.

h[i][j] of the reference is ce[port i][antenna j]; its locals are h00 = h[0][0], h01 = h[1][0], h10 = h[0][1], h11 = h[1][1]. Estimates are
ce [2][2][N] complex64 with N = nsym * 12 * nof_prb."""
import ctypes as C
import math

import numpy as np

from _libs import RefCell, RefChestRes, acopy, p

PMI_SEL_PRECISION = 24
F = np.float32
SQRT1_2 = F(math.sqrt(0.5))
CQI_TO_SNR = [F(v) for v in (1.95, 4, 6, 8, 10, 11.95, 14.05, 16, 17.9, 20.9, 22.5, 24.75, 25.5, 27.30, 29)]


def nof_samples(N):
    """(samples of the PMI selection, samples of the condition number): the AVX loops take groups of four and drop the tail
    (precoding.c:2352, :2721); srslte_precoding_2x2_cn_gen takes every 24th RE."""
    return 4 * (N // (4 * PMI_SEL_PRECISION)), -(-N // PMI_SEL_PRECISION)


def _seq_sum(x):
    """sum in the order of a C loop, float32"""
    return np.add.accumulate(x.astype(F), dtype=F)[-1] if len(x) else F(0)


def _h(ce, n):
    j = np.arange(n) * PMI_SEL_PRECISION
    c = np.asarray(ce, np.complex64)
    return c[0, 0, j], c[1, 0, j], c[0, 1, j], c[1, 1, j]


def _J(x):
    return (1j * x).astype(np.complex64)


def pmi_select_1l(ce, n, noise):
    """srslte_precoding_pmi_select_1l_gen over samples 24 k, k < n -> (pmi, sinr[4])"""
    h00, h01, h10, h11 = _h(ce, n)
    cj = np.conj
    sinr, pmi, mx = [], 0, F(0)
    for i in range(4):
        if i == 0:
            a0, a1 = cj(h00) + cj(h01), cj(h10) + cj(h11)
        elif i == 1:
            a0, a1 = cj(h00) - cj(h01), cj(h10) - cj(h11)
        elif i == 2:
            a0, a1 = cj(h00) - _J(cj(h01)), cj(h10) - _J(cj(h11))
        else:
            a0, a1 = cj(h00) + _J(cj(h01)), cj(h10) + _J(cj(h11))
        a0, a1 = (a0 * SQRT1_2).astype(np.complex64), (a1 * SQRT1_2).astype(np.complex64)
        b0 = a0 * h00 + a1 * h10
        b1 = a0 * h01 + a1 * h11
        c = (b0 + b1, b0 - b1, b0 + _J(b1), b0 - _J(b1))[i]
        s = _seq_sum((c * SQRT1_2).real) / (F(noise) * F(n))
        sinr.append(F(s))
        if s > mx:
            mx, pmi = s, i
    return pmi, np.array(sinr, F)


def pmi_select_2l(ce, n, noise):
    """srslte_precoding_pmi_select_2l_gen over samples 24 k, k < n -> (pmi, sinr[2])"""
    h00, h01, h10, h11 = _h(ce, n)
    cj = np.conj
    ne = F(noise)
    sinr, pmi, mx = [], 0, F(0)
    for i in range(2):
        if i == 0:
            a00, a01, a10, a11 = cj(h00) + cj(h01), cj(h10) + cj(h11), cj(h00) - cj(h01), cj(h10) - cj(h11)
        else:
            a00, a01 = cj(h00) - _J(cj(h01)), cj(h10) - _J(cj(h11))
            a10, a11 = cj(h00) + _J(cj(h01)), cj(h10) + _J(cj(h11))
        b00, b01 = a00 * h00 + a01 * h10, a00 * h01 + a01 * h11
        b10, b11 = a10 * h00 + a11 * h10, a10 * h01 + a11 * h11
        if i == 0:
            c00, c01, c10, c11 = b00 + b01, b00 - b01, b10 + b11, b10 - b11
        else:
            c00, c01, c10, c11 = b00 + _J(b01), b00 - _J(b01), b10 + _J(b11), b10 - _J(b11)
        c00, c01, c10, c11 = [(x * F(0.25)).astype(np.complex64) for x in (c00, c01, c10, c11)]
        c00, c11 = (c00 + ne).astype(np.complex64), (c11 + ne).astype(np.complex64)
        det = c00 * c11 - c01 * c10
        dd = det.real * det.real + det.imag * det.imag
        inv = (det.real / dd + 1j * (-det.imag / dd)).astype(np.complex64)
        den0, den1 = (c00 * ne).astype(np.complex64) * inv, (c11 * ne).astype(np.complex64) * inv
        g0 = den0.real / (den0.real * den0.real + den0.imag * den0.imag) - F(1)
        g1 = den1.real / (den1.real * den1.real + den1.imag * den1.imag) - F(1)
        s = _seq_sum(g0 + g1)
        if n:
            s = F(s / F(n))
        sinr.append(F(s))
        if s > mx:
            mx, pmi = s, i
    return pmi, np.array(sinr, F)


def cn_db(ce, n):
    """srslte_precoding_2x2_cn_gen over samples 24 k, k < n (srslte_mat_2x2_cn, mat.c:101-121)"""
    h00, h01, h10, h11 = _h(ce, n)
    a00 = h00.real * h00.real + h01.real * h01.real + h00.imag * h00.imag + h01.imag * h01.imag
    a01 = h00 * np.conj(h10) + h01 * np.conj(h11)
    a11 = h10.real * h10.real + h11.real * h11.real + h10.imag * h10.imag + h11.imag * h11.imag
    b = a00 + a11
    c = a00 * a11 - (a01.real * a01.real + a01.imag * a01.imag)
    sqr = np.sqrt(b * b - F(4) * c)
    v = F(10) * np.log10((b + sqr) / (b - sqr))
    s = _seq_sum(v)
    return F(s / F(n)) if n else F(s)


def cqi_from_snr(snr):
    """srslte_cqi_from_snr (cqi.c:561-569)"""
    for cqi in range(14, -1, -1):
        if F(snr) >= CQI_TO_SNR[cqi]:
            return cqi + 1
    return 0


def select_ri_pmi(sel, max_ri):
    """select_ri_pmi (ue_dl.c:735-779) over sel(ri) -> (pmi, sinr_list): (ri, pmi, sinr_db)"""
    best, best_pmi, best_ri = F(-np.inf), 0, 0
    for ri in range(max_ri):
        pmi, sinr = sel(ri)
        with np.errstate(divide="ignore", invalid="ignore"):
            this = F(F(10) * np.log10(F(sinr[pmi % 4])))
        if float(this) > float(best) + 0.1 or float(this) > 20.0:
            best, best_pmi, best_ri = this, pmi, ri
    return best_ri, best_pmi, best


def measure(ce, noise, snr_db, offset=0.0, nof_rx=2):
    """What srslte_hip_csi_batch writes for one subframe of a 2-port cell, as a dict of the record's fields."""
    N = np.asarray(ce).shape[-1]
    n_pmi, n_cn = nof_samples(N)
    if nof_rx == 1:
        ce = np.array(ce, np.complex64)
        ce[:, 1, :] = 0
    p1, s1 = pmi_select_1l(ce, n_pmi, noise)
    p2, s2 = pmi_select_2l(ce, n_pmi, noise) if nof_rx > 1 else (0, np.zeros(2, F))
    cn = cn_db(ce, n_cn) if nof_rx > 1 else F(0)
    ri, pmi, sinr_db = select_ri_pmi(lambda r: (p2, s2) if r else (p1, s1), min(nof_rx, 2))
    return dict(sinr_1l=s1, sinr_2l=s2, pmi_1l=p1, pmi_2l=p2, cn_db=cn, ri_cn=1 if nof_rx > 1 and cn < F(17.0) else 0, ri=ri, pmi=pmi, sinr_db=sinr_db,
                cqi_sinr=cqi_from_snr(F(sinr_db) + F(offset)), cqi_wideband=cqi_from_snr(F(snr_db) + F(offset)))


# ---------------------------------------------------------------- the reference's own functions
class Ref:
    """The reference library on ce [2][2][N] (copies kept aligned for its SIMD loads)."""

    def __init__(self, lib, ce, noise, nof_prb, cp_norm=True, nof_rx=2):
        self.lib = lib
        self.ce = [[acopy(np.ascontiguousarray(ce[i][j], np.complex64)) for j in range(2)] for i in range(2)]
        self.N = self.ce[0][0].size
        self.noise = float(noise)
        self.h = ((C.c_void_p * 4) * 4)()
        for i in range(2):
            for j in range(2):
                self.h[i][j] = self.ce[i][j].ctypes.data
        # srslte_pdsch_t starts with its cell and nof_rx_antennas (pdsch.h:53-56): all srslte_pdsch_select_pmi / _compute_cn read of it
        self.q = C.create_string_buffer(4096)
        cell = RefCell(nof_prb, 2, 1, 0 if cp_norm else 1, 0, 0, 0)
        C.memmove(self.q, C.byref(cell), C.sizeof(cell))
        C.memmove(C.byref(self.q, C.sizeof(cell)), C.byref(C.c_uint32(nof_rx)), 4)
        self.res = RefChestRes()
        for i in range(2):
            for j in range(2):
                self.res.ce[i][j] = self.ce[i][j].ctypes.data
        self.res.noise_estimate = self.noise
        assert self.N == (14 if cp_norm else 12) * 12 * nof_prb

    def _sel(self, fn, nof_symbols, *extra):
        pmi, sinr = C.c_uint32(0), (C.c_float * 4)()
        fn.restype = C.c_int
        r = fn(self.h, C.c_uint32(nof_symbols), C.c_float(self.noise), *extra, C.byref(pmi), sinr)
        assert r >= 0
        return pmi.value, np.array(sinr[:], F)

    def gen(self, layers, nof_symbols):
        """srslte_precoding_pmi_select_{1l,2l}_gen"""
        pmi, s = self._sel(getattr(self.lib, "srslte_precoding_pmi_select_%dl_gen" % layers), nof_symbols)
        return pmi, s[:4 if layers == 1 else 2]

    def dispatch(self, layers, nof_symbols):
        """srslte_precoding_pmi_select: the build's dispatch (AVX)"""
        pmi, s = self._sel(self.lib.srslte_precoding_pmi_select, nof_symbols, C.c_int(layers))
        return pmi, s[:4 if layers == 1 else 2]

    def pdsch_select_pmi(self, layers):
        """srslte_pdsch_select_pmi (pdsch.c:1186-1205): the dispatch over SRSLTE_NOF_RE(cell)"""
        pmi, sinr = C.c_uint32(0), (C.c_float * 4)()
        assert self.lib.srslte_pdsch_select_pmi(self.q, C.byref(self.res), C.c_uint32(layers), C.byref(pmi), sinr) == 0
        return pmi.value, np.array(sinr[:], F)

    def cn(self):
        """srslte_pdsch_compute_cn -> srslte_precoding_cn; None where it refuses"""
        v = C.c_float(0)
        return F(v.value) if self.lib.srslte_pdsch_compute_cn(self.q, C.byref(self.res), C.byref(v)) == 0 else None

    def select_ri_pmi(self, nof_rx=2):
        """select_ri_pmi (static in ue_dl.c) restated over srslte_pdsch_select_pmi -> (ri, pmi, sinr_db)"""
        return select_ri_pmi(lambda r: self.pdsch_select_pmi(r + 1), min(nof_rx, 2))


def ref_cqi_from_snr(lib, snr):
    lib.srslte_cqi_from_snr.restype = C.c_uint8
    return lib.srslte_cqi_from_snr(C.c_float(snr))


class RefCqiCfg(C.Structure):
    """srslte_cqi_cfg_t (cqi.h:121-132)"""
    _fields_ = [("data_enable", C.c_bool), ("ri_present", C.c_bool), ("pmi_present", C.c_bool), ("four_antenna_ports", C.c_bool),
                ("rank_is_not_one", C.c_bool), ("subband_label_2_bits", C.c_bool), ("L", C.c_uint32), ("N", C.c_uint32), ("type", C.c_int),
                ("ri_len", C.c_uint32)]


class RefHl(C.Structure):
    _fields_ = [("wideband_cqi_cw0", C.c_uint8), ("subband_diff_cqi_cw0", C.c_uint32), ("wideband_cqi_cw1", C.c_uint8), ("subband_diff_cqi_cw1", C.c_uint32),
                ("pmi", C.c_uint32)]


class RefUe(C.Structure):
    _fields_ = [("wideband_cqi", C.c_uint8), ("subband_diff_cqi", C.c_uint8), ("position_subband", C.c_uint32)]


class RefWb(C.Structure):
    _fields_ = [("wideband_cqi", C.c_uint8), ("spatial_diff_cqi", C.c_uint8), ("pmi", C.c_uint8)]


class RefSb(C.Structure):
    _fields_ = [("subband_cqi", C.c_uint8), ("subband_label", C.c_uint8)]


class _RefCqiUnion(C.Union):
    _fields_ = [("wideband", RefWb), ("subband", RefSb), ("subband_ue", RefUe), ("subband_hl", RefHl)]


class RefCqiValue(C.Structure):
    """srslte_cqi_value_t (cqi.h:134-142)"""
    _anonymous_ = ("u",)
    _fields_ = [("u", _RefCqiUnion), ("data_crc", C.c_bool)]


class RefCqiReportCfg(C.Structure):
    """srslte_cqi_report_cfg_t (cqi.h:55-65)"""
    _fields_ = [("periodic_configured", C.c_bool), ("aperiodic_configured", C.c_bool), ("pmi_idx", C.c_uint32), ("ri_idx", C.c_uint32),
                ("ri_idx_present", C.c_bool), ("format_is_subband", C.c_bool), ("subband_size", C.c_uint32), ("periodic_mode", C.c_int),
                ("aperiodic_mode", C.c_int)]


def to_ref(cfg, value):
    """(CqiCfg, CqiValue) of the package -> (RefCqiCfg, RefCqiValue)"""
    rc = RefCqiCfg(bool(cfg.data_enable), False, bool(cfg.pmi_present), bool(cfg.four_antenna_ports), bool(cfg.rank_is_not_one),
                   bool(cfg.subband_label_2_bits), cfg.L, cfg.N, cfg.type, 0)
    rv = RefCqiValue()
    if cfg.type == 0:
        rv.wideband = RefWb(value.wideband_cqi, value.spatial_diff_cqi, value.pmi)
    elif cfg.type == 1:
        rv.subband = RefSb(value.subband_cqi, value.subband_label)
    elif cfg.type == 2:
        rv.subband_ue = RefUe(value.wideband_cqi, value.subband_diff_cqi, 0)
    else:
        rv.subband_hl = RefHl(value.wideband_cqi, value.subband_diff_cqi, value.wideband_cqi_cw1, value.subband_diff_cqi_cw1, value.pmi)
    return rc, rv


# ---------------------------------------------------------------- ue_dl.c:802-928, line by line
class Uci:
    """the members of srslte_uci_data_t the two generators touch, zeroed as the caller zeroes them"""

    def __init__(self):
        self.type, self.data_enable, self.pmi_present, self.four_antenna_ports, self.rank_is_not_one, self.N = 0, False, False, False, False, 0
        self.ri_len, self.ri = 0, 0
        self.wideband_cqi = self.pmi = self.subband_cqi = self.subband_label = self.subband_diff_cqi = 0
        self.wideband_cqi_cw1 = self.subband_diff_cqi_cw1 = 0


class Ue:
    """srslte_ue_dl_t + srslte_ue_dl_cfg_t as far as the generators read them; csi: the measurement (dict of measure(), or a record)"""

    def __init__(self, csi, tm, nof_prb, nof_ports, nof_rx, last_ri=0, tdd=False, periodic_configured=True, ri_idx_present=True, I_cqi_pmi=0, I_ri=0,
                 format_is_subband=False, aperiodic_mode=31, snr_to_cqi_offset=0.0, send=None):
        self.__dict__.update(locals())
        self.send = send  # (periodic_send, periodic_ri_send) of the schedule under test

    def _get(self, k):
        return self.csi[k] if isinstance(self.csi, dict) else getattr(self.csi, k)

    def select_pmi(self, ri):
        """select_pmi(q, ri, &pmi, NULL)"""
        if self.nof_ports < 2:
            return 0
        return int(self._get("pmi_1l")) if ri == 0 else int(self._get("pmi_2l")) if ri == 1 else 0

    def select_ri_pmi(self):
        """select_ri_pmi(q, &cfg->last_ri, &pmi, &sinr_db)"""
        if self.nof_ports < 2:
            self.last_ri = 0
            return 0, F(-np.inf)
        self.last_ri = int(self._get("ri"))
        return int(self._get("pmi")), F(self._get("sinr_db"))

    def select_ri(self):
        """srslte_ue_dl_select_ri(q, &cfg->last_ri, NULL): srslte_precoding_cn succeeds for 2x2 only"""
        if self.nof_ports == 2 and self.nof_rx == 2:
            self.last_ri = int(self._get("ri_cn"))


def no_subbands(nof_prb):
    sz = 0 if nof_prb < 7 else 4 if nof_prb <= 26 else 6 if nof_prb <= 63 else 8 if nof_prb <= 110 else -1
    return int(math.ceil(F(nof_prb) / F(sz))) if sz > 0 else 0


def gen_cqi_periodic(q, wideband_value, tti):
    u = Uci()
    ps, prs = q.send
    if q.periodic_configured and q.ri_idx_present and prs(q.I_cqi_pmi, q.I_ri, tti, q.tdd):
        if q.nof_rx > 1:
            if q.tm == 3:
                q.select_ri()
            elif q.tm == 4:
                q.select_ri_pmi()
        else:
            q.last_ri = 0
        u.ri_len = 1
        u.ri = q.last_ri
    elif q.periodic_configured and ps(q.I_cqi_pmi, tti, q.tdd):
        if q.format_is_subband:
            u.type = 1
            u.subband_cqi = wideband_value
            u.subband_label = 0
        else:
            u.type = 0
            u.wideband_cqi = wideband_value
            if q.tm == 4:
                pmi = q.select_pmi(q.last_ri)
                u.pmi_present = True
                u.rank_is_not_one = q.last_ri != 0
                u.pmi = pmi & 0xff
        u.data_enable = True
        u.ri_len = 0
        u.ri = q.last_ri
    return u


def gen_cqi_aperiodic(q, wideband_value):
    u = Uci()
    if q.aperiodic_mode == 30:
        u.type = 3
        u.wideband_cqi = wideband_value
        u.subband_diff_cqi = 0
        u.N = no_subbands(q.nof_prb) if q.nof_prb > 7 else 0
        u.data_enable = True
        if q.tm in (3, 4):
            if q.nof_rx > 1:
                q.select_ri()
                u.ri = q.last_ri & 0xff
                u.ri_len = 1
            else:
                u.ri = 0
        else:
            u.ri_len = 0
    elif q.aperiodic_mode == 31:
        pmi, sinr_db = q.select_ri_pmi()
        u.type = 3
        u.wideband_cqi = cqi_from_snr(F(sinr_db) + F(q.snr_to_cqi_offset))
        u.subband_diff_cqi = 0
        if q.last_ri > 0:
            u.rank_is_not_one = True
            u.wideband_cqi_cw1 = cqi_from_snr(F(sinr_db) + F(q.snr_to_cqi_offset))
            u.subband_diff_cqi_cw1 = 0
        u.pmi = pmi
        u.pmi_present = True
        u.four_antenna_ports = q.nof_ports == 4
        u.N = no_subbands(q.nof_prb) if q.nof_prb > 7 else 0
        u.data_enable = True
        u.ri_len = 1
        u.ri = q.last_ri
    return u


# ---------------------------------------------------------------- drawn channels
def draw_ce(rng, nof_prb, cp_norm=True, cond="well", ripple=0.2):
    """ce [2][2][N]: a flat 2x2 matrix with a smooth frequency ripple on every entry. cond: "well" (i.i.d. complex Gaussian entries),
    "ill" (a rank-one matrix plus a fifth of an i.i.d. one: condition numbers of 15-25 dB, on either side of the 17 dB of the rank rule),
    "ortho" (a scaled unitary matrix). Why "ill" stops there: srslte_mat_2x2_cn takes the small eigenvalue as b - sqrt(b^2 - 4 c) in float32,
    whose relative error is a few 6e-8 times lambda_max / lambda_min; at 30 dB that alone is 1e-3 dB, the whole bound of the comparison, and
    the reference's own build (fused multiply-adds) and any restatement of its text then differ by as much."""
    N = (14 if cp_norm else 12) * 12 * nof_prb
    g = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)) * math.sqrt(0.5)
    if cond == "well":
        H = g(2, 2)
    elif cond == "ill":
        H = np.outer(g(2), g(2)) + 0.2 * g(2, 2)
    else:
        q, _ = np.linalg.qr(g(2, 2))
        H = q * (0.5 + rng.random())
    k = np.arange(N) / N
    rip = 1 + ripple * np.exp(2j * np.pi * (rng.random((2, 2, 1)) + k * rng.integers(1, 4, (2, 2, 1))))
    return (H[:, :, None] * rip).astype(np.complex64)
