"""Reference side of the PUCCH tests (tests/test_ul_ctrl_host.py, tests/test_gpu_ul_ctrl.py, tests/test_pucch_golden.py,
tests/test_gpu_pucch_sweep.py) and of scripts/bench_ul_ctrl.py.

srslte_pucch_* / srslte_ue_ul_* / srslte_enb_ul_* and srslte_refsignal_dmrs_pucch_* are not exported from oracle/_ref/libsrslte_ref.so, so the
chain of srslte_enb_ul_get_pucch (enb_ul.c:175-228) is assembled from what is: srslte_refsignal_ul_set_cell (n_cs_cell and f_gh read through a
mirror of srslte_refsignal_ul_t), srslte_refsignal_r_uv_arg_1prb, srslte_chest_ul_estimate_pucch (which runs the reference's own
srslte_refsignal_dmrs_pucch_gen / _get, srslte_pucch_alpha_format1 / 2, srslte_pucch_n_prb and the 2a / 2b hypotheses), srslte_predecoding_single,
srslte_vec_corr_ccc, srslte_demod_soft_demodulate_s, srslte_sequence_pucch, srslte_scrambling_s_offset, srslte_uci_encode_cqi_pucch and
srslte_uci_decode_cqi_pucch. Restated in numpy, each with its lines: encode_signal_format12 (pucch.c:429-492), pucch_cp (:380-417), the DMRS of
srslte_refsignal_dmrs_pucch_gen / _put (refsignal_ul.c:558-680), get_format (ue_ul.c:482-531) and get_npucch (:823-900). encode_z and the
format-2 means of _attempt follow the float operations of the reference's release build, and tests/test_pucch_golden.py holds all of it to
tests/golden/pucch.npz, recorded from the reference's own srslte_pucch_encode / srslte_pucch_decode. Test infrastructure only."""
import ctypes as C

import numpy as np

from _libs import RefCell, RefChestUlRes, aligned, opaque, ref

F1, F1A, F1B, F2, F2A, F2B = range(6)
QPSK = 1  # srslte_mod_t

# srslte_pucch_cfg_t (pucch_cfg.h:45-90) and srslte_refsignal_ul_t (refsignal_ul.h:73-83): offsets pinned by tests/test_ul_ctrl_host.py
PUCCH_CFG = {"size": 516, "rnti": 0, "ack.nof_acks": 4 + 4, "ack.ncce": 4 + 8, "cqi.data_enable": 4 + 340, "cqi.ri_len": 4 + 360,
             "is_scheduling_request_tti": 4 + 364, "delta_pucch_shift": 372, "n_rb_2": 376, "N_cs": 380, "N_pucch_1": 384, "group_hopping_en": 388,
             "n_pucch_2": 416, "n_pucch_sr": 420, "simul_cqi_ack": 424, "threshold_format1": 480, "threshold_data_valid_format1a": 484,
             "threshold_data_valid_format2": 488, "format": 492, "n_pucch": 496, "pucch2_drs_bits": 500}
REFSIGNAL_UL = {"size": 5560, "n_cs_cell": 40, "f_gh": 3000}
UL_SF_CFG = {"size": 20, "tti": 12, "shortened": 16}

W_N_OC = np.array([[[0, 0, 0, 0], [0, np.pi, 0, np.pi], [0, np.pi, np.pi, 0]],
                   [[0, 0, 0, 0], [0, 2 * np.pi / 3, 4 * np.pi / 3, 0], [0, 4 * np.pi / 3, 2 * np.pi / 3, 0]]], np.float32)  # pucch.c:297-303
ALPHA = np.array([2 * np.pi * n / 12 for n in range(12)], np.float32)  # srslte_pucch_alpha_format1 / 2's return value
S_NS = np.float32(np.pi / 2)
W_DMRS1 = np.array([[0, 0, 0], [0, 2 * np.pi / 3, 4 * np.pi / 3], [0, 4 * np.pi / 3, 2 * np.pi / 3]], np.float32)  # refsignal_ul.c:46-48
W_DMRS1E = np.array([[0, 0], [0, np.pi], [0, 0]], np.float32)  # :50-52
Z2AB = {(0, 0): 1, (0, 1): -1j, (1, 0): 1j, (1, 1): -1}  # srslte_pucch_format2ab_mod_bits (pucch.c:1061-1088) for 2b; 2a: bit 0 -> +-1


def _fma32(a, b, c):
    """float fma(a, b, c) element-wise: the product of two floats is exact in float64; its sum with c is rounded there once before the
    rounding to float, which moves the result only where that sum lies within 2^-29 ulp of a tie."""
    return (np.asarray(a, np.float32).astype(np.float64) * np.float64(np.float32(b)) + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


_libm = C.CDLL("libm.so.6")
_libm.sincosf.restype, _libm.sincosf.argtypes = None, [C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]


def _sincosf(x):
    """(cos, sin) float32 of glibc's sincosf, which the reference's cexpf(I x) is compiled to."""
    out, s, c = np.empty((2, x.size), np.float32), C.c_float(), C.c_float()
    for i, v in enumerate(np.asarray(x, np.float32).tolist()):
        _libm.sincosf(v, C.byref(s), C.byref(c))
        out[0, i], out[1, i] = c.value, s.value
    return out[0], out[1]


def n_rs(fmt, ext):  # srslte_refsignal_dmrs_N_rs (refsignal_ul.c:489-514)
    return (2 if ext else 3) if fmt < F2 else ((1 if ext else 2) if fmt == F2 else 2)


def dmrs_sym(fmt, m, ext):  # srslte_refsignal_dmrs_pucch_symbol (:517-555)
    return 2 + m if fmt < F2 else (3 if fmt == F2 and ext else (1, 5)[m])


def _R():
    R = ref()
    vp = C.c_void_p
    R.srslte_refsignal_ul_init.argtypes = [vp, C.c_uint32]
    R.srslte_refsignal_ul_set_cell.argtypes = [vp, RefCell]
    R.srslte_refsignal_r_uv_arg_1prb.argtypes = [vp, C.c_uint32]
    R.srslte_chest_ul_init.argtypes = [vp, C.c_uint32]
    R.srslte_chest_ul_set_cell.argtypes = [vp, RefCell]
    R.srslte_chest_ul_pregen.argtypes = [vp, vp]
    R.srslte_chest_ul_estimate_pucch.argtypes = [vp, vp, vp, vp, vp]
    R.srslte_vec_corr_ccc.restype = C.c_float
    R.srslte_vec_corr_ccc.argtypes = [vp, vp, C.c_uint32]
    R.srslte_vec_prod_conj_ccc.argtypes = [vp, vp, vp, C.c_int]
    R.srslte_demod_soft_demodulate_s.argtypes = [C.c_int, vp, vp, C.c_int]
    R.srslte_sequence_pucch.argtypes = [vp, C.c_uint16, C.c_uint32, C.c_uint32]
    R.srslte_scrambling_s_offset.argtypes = [vp, vp, C.c_int, C.c_int]
    R.srslte_uci_cqi_pucch_init.argtypes = [vp]
    R.srslte_uci_decode_cqi_pucch.restype = C.c_int16
    R.srslte_uci_decode_cqi_pucch.argtypes = [vp, vp, vp, C.c_uint32]
    R.srslte_uci_encode_cqi_pucch.argtypes = [vp, C.c_uint32, vp]
    return R


# ---------------------------------------------------------------- restated selection (ue_ul.c) and geometry (pucch.c)
def select(cp_ext, N_pucch_1, req, sr_tti, uci_sr=0):
    """srslte_ue_ul_pucch_resource_selection (ue_ul.c:482-531 get_format, :823-900 get_npucch) -> (format, n_pucch) or None."""
    data_enable = req.cqi_len > 0 and not (not req.simul_cqi_ack and req.ack_len > 0)  # the CQI drop, ue_ul.c:891-893
    f = None
    if not data_enable and req.ri_len == 0:
        if req.ack_len == 1:
            f = F1A
        elif req.ack_len == 2:
            f = F1B
        elif sr_tti or uci_sr:
            f = F1
    else:
        if req.ack_len == 0:
            f = F2
        elif req.ack_len == 1 and not cp_ext:
            f = F2A
        elif req.ack_len == 2:
            f = F2B
        elif req.ack_len == 1 and cp_ext:
            f = F2B
    if f is None:
        return None
    if sr_tti or uci_sr:
        return f, req.n_pucch_sr
    return f, (req.ncce + N_pucch_1 if f < F2 else req.n_pucch_2)


def n_sf(fmt, slot, shortened):
    return 5 if fmt >= F2 else (3 if slot and shortened else 4)  # get_N_sf, pucch.c:314-339


def data_sym(fmt, m, ext):  # get_pucch_symbol, pucch.c:341-377
    return ((0, 1, 2, 4, 5) if ext else (0, 2, 3, 4, 6))[m] if fmt >= F2 else ((0, 1, 4, 5) if ext else (0, 1, 5, 6))[m]


def pucch_n_prb(fmt, n_pucch, slot, nof_prb, D, N_cs, n_rb_2, ext):
    """srslte_pucch_m + srslte_pucch_n_prb (pucch.c:911-952)."""
    if fmt < F2:
        c = 2 if ext else 3
        m = n_rb_2
        if n_pucch >= c * N_cs // D:
            m = (n_pucch - c * N_cs // D) // (c * 12 // D) + n_rb_2 + int(np.ceil(np.float32(N_cs) / 8))
    else:
        m = n_pucch // 12
    return (nof_prb - 1 - m // 2) if (m + slot) % 2 else m // 2


def _u32(x):
    return x & 0xFFFFFFFF


def alpha1(n_cs_cell, ext, D, N_cs, n_pucch, ns, l):
    """srslte_pucch_alpha_format1 with is_dmrs = true (pucch.c:974-1031) -> (n_cs, n_oc, n')."""
    c = 2 if ext else 3
    thr = c * N_cs // D
    Np = N_cs if n_pucch < thr else 12
    npr = n_pucch if n_pucch < thr else (n_pucch - thr) % (c * 12 // D)
    if ns % 2:
        if n_pucch >= thr:
            npr = _u32((c * (npr + 1)) % (c * 12 // D + 1) - 1)
        else:
            h = (npr + (0 if ext else 2)) % (c * Np // D)
            npr = h // c + (h % c) * Np // D
    n_oc = npr * D // Np
    if ext:
        n_cs = (int(n_cs_cell[ns][l]) + (npr * D + n_oc) % Np) % 12
    else:
        n_cs = (int(n_cs_cell[ns][l]) + (npr * D + n_oc % D) % Np) % 12
    return n_cs, n_oc, npr


def alpha2(n_cs_cell, N_cs, n_rb_2, n_pucch, ns, l):
    """srslte_pucch_alpha_format2 (pucch.c:1034-1058) -> n_cs."""
    hi = n_pucch >= 12 * n_rb_2
    npr = (n_pucch + N_cs + 1) % 12 if hi else n_pucch % 12
    if ns % 2:
        npr = (12 * (npr + 1)) % 13 - 1
        if hi:
            x = int(np.fmod(12 - 2 - n_pucch, 12))  # C's remainder keeps the dividend's sign
            npr = x if x >= 0 else 12 + x
    return (int(n_cs_cell[ns][l]) + npr) % 12


class RefUlCtrl:
    """The reference's PUCCH chain for one cell and common PUCCH configuration (a srslte_hip_ul_ctrl_cfg_t or anything with its fields)."""

    def __init__(self, cfg):
        self.R = R = _R()
        self.cfg = cfg
        self.P, self.cell_id, self.ext = cfg.nof_prb, cfg.cell_id, bool(cfg.cp_ext)
        self.nsl = 6 if self.ext else 7
        self.glen = 2 * self.nsl * 12 * self.P
        self.cell = RefCell(self.P, 1, self.cell_id, 1 if self.ext else 0, 0, 0, 0)
        self.rs = opaque(1 << 14)
        assert R.srslte_refsignal_ul_init(self.rs, self.P) == 0 and R.srslte_refsignal_ul_set_cell(self.rs, self.cell) == 0
        raw = np.frombuffer(self.rs, np.uint32, count=REFSIGNAL_UL["size"] // 4)
        self.n_cs_cell = raw[REFSIGNAL_UL["n_cs_cell"] // 4:][:140].reshape(20, 7).copy()
        self.f_gh = raw[REFSIGNAL_UL["f_gh"] // 4:][:20].copy()
        self.arg = np.zeros((20, 12), np.float32)
        for ns in range(20):
            u = ((int(self.f_gh[ns]) if cfg.group_hopping_en else 0) + self.cell_id % 30) % 30
            a = aligned(12, np.float32)
            R.srslte_refsignal_r_uv_arg_1prb(a.ctypes.data, u)
            self.arg[ns] = a
        self.chest = opaque(1 << 16)
        assert R.srslte_chest_ul_init(self.chest, self.P) == 0 and R.srslte_chest_ul_set_cell(self.chest, self.cell) == 0
        R.srslte_chest_ul_pregen(self.chest, C.byref((C.c_uint32 * 4)()))  # any PUSCH DMRS configuration: it marks the estimator configured
        self.cqi = opaque(64)
        R.srslte_uci_cqi_pucch_init(self.cqi)
        self.seq = opaque(256)

    # ---- configuration structs of the reference
    def pucch_cfg(self, fmt, n_pucch, rnti=0):
        b = (C.c_uint8 * PUCCH_CFG["size"])()
        u = np.frombuffer(b, np.uint32)
        f = np.frombuffer(b, np.float32)
        c = self.cfg
        u[0] = rnti
        for k in ("delta_pucch_shift", "n_rb_2", "N_cs", "N_pucch_1", "format", "n_pucch"):
            u[PUCCH_CFG[k] // 4] = {"format": fmt, "n_pucch": n_pucch}.get(k, getattr(c, k, 0))
        b[PUCCH_CFG["group_hopping_en"]] = 1 if c.group_hopping_en else 0
        for k in ("threshold_format1", "threshold_data_valid_format1a", "threshold_data_valid_format2"):
            f[PUCCH_CFG[k] // 4] = getattr(c, k)
        return b

    @staticmethod
    def sf_cfg(tti, shortened):
        b = (C.c_uint8 * UL_SF_CFG["size"])()
        np.frombuffer(b, np.uint32)[UL_SF_CFG["tti"] // 4] = tti
        b[UL_SF_CFG["shortened"]] = 1 if shortened else 0
        return b

    # ---- restated transmit side
    def re_list(self, fmt, n_pucch, shortened):
        """pucch_cp (pucch.c:380-417): the grid index of z[i]."""
        c = self.cfg
        out = []
        for s in range(2):
            prb = pucch_n_prb(fmt, n_pucch, s, self.P, c.delta_pucch_shift, c.N_cs, c.n_rb_2, self.ext)
            for m in range(n_sf(fmt, s, shortened)):
                out += [(data_sym(fmt, m, self.ext) + s * self.nsl) * 12 * self.P + prb * 12 + k for k in range(12)]
        return np.array(out, np.int64)

    def encode_z(self, fmt, n_pucch, tti, shortened, d):
        """encode_signal_format12 (pucch.c:429-492): d = d(0) for 1/1a/1b, the 10 QPSK symbols (or ones) for 2/2a/2b -> z complex64. In the
        order of the reference's release build (-Ofast -mfma), read from its object code: the phase is fma(n, alpha, tmp_arg[n]) for formats
        2-2b and (w + tmp_arg[n]) + fma(n, alpha, S_ns) for 1-1b, cexpf is glibc's sincosf, and d (c + j s) is
        (fma(-s, Im d, Re d c), fma(c, Im d, Re d s)), which is exact for the unit values of d(0)."""
        c, sf_idx, n = self.cfg, tti % 10, np.arange(12, dtype=np.float32)
        d = np.atleast_1d(np.asarray(d, np.complex64))
        z = []
        for s in range(2):
            ns = 2 * sf_idx + s
            Nsf = n_sf(fmt, s, shortened)
            for m in range(Nsf):
                l = data_sym(fmt, m, self.ext)
                if fmt >= F2:
                    co, si = _sincosf(_fma32(n, ALPHA[alpha2(self.n_cs_cell, c.N_cs, c.n_rb_2, n_pucch, ns, l)], self.arg[ns]))
                    a, b = d[s * 5 + m].real, d[s * 5 + m].imag
                    z.append((_fma32(-si, b, a * co) + 1j * _fma32(co, b, a * si)).astype(np.complex64))
                else:
                    n_cs, n_oc, npr = alpha1(self.n_cs_cell, self.ext, c.delta_pucch_shift, c.N_cs, n_pucch, ns, l)
                    ph = (W_N_OC[1 if Nsf == 3 else 0][n_oc % 3][m] + self.arg[ns]) + _fma32(n, ALPHA[n_cs], S_NS if npr % 2 else np.float32(0))
                    co, si = _sincosf(ph)
                    z.append(d[0] * (co + 1j * si).astype(np.complex64))
        return np.concatenate(z).astype(np.complex64)

    def coded_bits(self, bits, length):
        """srslte_uci_encode_cqi_pucch -> 20 bits."""
        data, out = aligned(13, np.uint8), aligned(20, np.uint8)
        data[:len(bits)] = bits
        assert self.R.srslte_uci_encode_cqi_pucch(data.ctypes.data, length, out.ctypes.data) == 0
        return out.copy()

    def scrambling(self, rnti, sf_idx):
        """srslte_sequence_pucch's 20 bits, through the reference's srslte_scrambling_s_offset of +1s."""
        x = aligned(20, np.int16)
        x[:] = 1
        assert self.R.srslte_sequence_pucch(self.seq, rnti, 2 * sf_idx, self.cell_id) == 0
        self.R.srslte_scrambling_s_offset(self.seq, x.ctypes.data, 0, 20)
        return (x < 0).astype(np.uint8)

    def dmrs(self, fmt, n_pucch, tti, drs_bits=(0, 0)):
        """srslte_refsignal_dmrs_pucch_gen (refsignal_ul.c:558-639) -> r [2 N_rs 12] complex64."""
        c, n = self.cfg, np.arange(12, dtype=np.float32)
        z1 = (-1 if drs_bits[0] else 1) if fmt == F2A else (Z2AB[tuple(drs_bits)] if fmt == F2B else 1)
        r = []
        for s in range(2):
            ns = 2 * (tti % 10) + s
            for m in range(n_rs(fmt, self.ext)):
                l = dmrs_sym(fmt, m, self.ext)
                if fmt < F2:
                    n_cs, n_oc, _ = alpha1(self.n_cs_cell, self.ext, c.delta_pucch_shift, c.N_cs, n_pucch, ns, l)
                    w = (W_DMRS1E if self.ext else W_DMRS1)[n_oc][m]
                else:
                    n_cs, w = alpha2(self.n_cs_cell, c.N_cs, c.n_rb_2, n_pucch, ns, l), np.float32(0)
                ph = (w + self.arg[ns]) + ALPHA[n_cs] * n
                r.append(((z1 if m == 1 else 1) * np.exp(1j * ph.astype(np.float64))).astype(np.complex64))
        return np.concatenate(r)

    def dmrs_re(self, fmt, n_pucch):
        """srslte_refsignal_dmrs_pucch_put (refsignal_ul.c:641-678): the grid index of r[i]."""
        c, out = self.cfg, []
        for s in range(2):
            prb = pucch_n_prb(fmt, n_pucch, s, self.P, c.delta_pucch_shift, c.N_cs, c.n_rb_2, self.ext)
            for m in range(n_rs(fmt, self.ext)):
                out += [(dmrs_sym(fmt, m, self.ext) + s * self.nsl) * 12 * self.P + prb * 12 + k for k in range(12)]
        return np.array(out, np.int64)

    def dmrs_put(self, grid, fmt, n_pucch, tti, shortened, drs_bits=(0, 0)):
        r = self.dmrs(fmt, n_pucch, tti, drs_bits)
        grid[self.dmrs_re(fmt, n_pucch)] = r
        return r

    def encode(self, grid, tti, tx):
        """srslte_ue_ul's pucch_encode of one PucchTx into grid: the PUCCH (restated) and its DMRS (the reference's). Returns the format."""
        q = tx.req
        sel = select(self.ext, self.cfg.N_pucch_1, q, q.sr_tti, tx.sr)
        fmt, n_pucch = sel
        a0, a1 = tx.ack[0], tx.ack[1]
        if fmt < F2:
            d = [1, -1][a0] if fmt == F1A else ({(0, 0): 1, (0, 1): -1j, (1, 0): 1j, (1, 1): -1}[(a0, a1)] if fmt == F1B else 1)
        else:
            length = q.ri_len or q.cqi_len
            bits = [tx.ri] if q.ri_len else list(tx.cqi[:length])
            b = self.coded_bits(bits, length) ^ self.scrambling(q.rnti, tti % 10)
            s = np.float32(1 / np.sqrt(2))
            d = (np.where(b[0::2], -s, s) + 1j * np.where(b[1::2], -s, s)).astype(np.complex64)
        grid[self.re_list(fmt, n_pucch, q.shortened)] = self.encode_z(fmt, n_pucch, tti, q.shortened, d)
        self.dmrs_put(grid, fmt, n_pucch, tti, q.shortened, (a0, a1) if fmt in (F2A, F2B) else (0, 0))
        return fmt

    # ---- the receiver: srslte_enb_ul_get_pucch
    def _attempt(self, grid, tti, q, fmt, n_pucch):
        R, c = self.R, self.cfg
        cfgb = self.pucch_cfg(fmt, n_pucch, q.rnti)
        ce = aligned(self.glen, np.complex64)
        res = RefChestUlRes()
        res.ce = ce.ctypes.data
        assert R.srslte_chest_ul_estimate_pucch(self.chest, self.sf_cfg(tti, q.shortened), cfgb, grid.ctypes.data, C.byref(res)) == 0
        drs = (cfgb[PUCCH_CFG["pucch2_drs_bits"]], cfgb[PUCCH_CFG["pucch2_drs_bits"] + 1])
        idx = self.re_list(fmt, n_pucch, q.shortened)
        nre = idx.size
        zt, h, z = aligned(nre, np.complex64), aligned(nre, np.complex64), aligned(nre, np.complex64)
        zt[:], h[:] = grid[idx], ce[idx]
        R.srslte_predecoding_single(zt.ctypes.data, h.ctypes.data, z.ctypes.data, None, nre, 1.0, q.noise_estimate)
        out = {"format": fmt, "n_pucch": n_pucch, "drs": drs, "z": z.copy(), "bits": (0, 0), "word": 0, "llr": None, "hyp": None}
        if fmt < F2:
            hyps = [((0, 0), 1)] if fmt == F1 else ([((b, 0), [1, -1][b]) for b in range(2)] if fmt == F1A else
                                                   [((b, b2), {(0, 0): 1, (0, 1): -1j, (1, 0): 1j, (1, 1): -1}[(b, b2)]) for b in range(2) for b2 in range(2)])
            corrs, base = [], self.encode_z(fmt, n_pucch, tti, q.shortened, 1)
            for bits, d in hyps:
                e = aligned(nre, np.complex64)
                e[:] = np.complex64(d) * base  # exact for the unit values of d(0)
                corrs.append(R.srslte_vec_corr_ccc(z.ctypes.data, e.ctypes.data, nre))
            k = int(np.argmax(corrs))  # the first maximum (decode_signal's >)
            out["corr"], out["bits"], out["hyp"] = np.float32(corrs[k]), hyps[k][0], corrs
            out["detected"] = corrs[0] >= c.threshold_format1 if fmt == F1 else corrs[k] > c.threshold_format1
            return out
        # decode_signal (pucch.c:683-690) as the reference's release build runs it: srslte_vec_prod_conj_ccc over the 128 symbols, then each
        # 12-RE mean as z[0] r, fma(z[j], r, acc) for j = 1..11 with r = float(1 / 12) (-Ofast turns the division by SRSLTE_NRE into a
        # product with the reciprocal and contracts it with the sum). A noise-free QPSK symbol sits on a step of the int16 LLR (100), so
        # the order decides 99 or 100. The fma is taken in float64, where the product is exact.
        ref, zin, zz = aligned(128, np.complex64), aligned(128, np.complex64), aligned(128, np.complex64)
        ref[:nre], zin[:nre] = self.encode_z(fmt, n_pucch, tti, q.shortened, np.ones(10, np.complex64)), z
        R.srslte_vec_prod_conj_ccc(zin.ctypes.data, ref.ctypes.data, zz.ctypes.data, 128)
        r12 = np.float64(np.float32(1) / np.float32(12))
        zf = zz.view(np.float32).reshape(128, 2)
        z2 = aligned(10, np.complex64)
        z2f = z2.view(np.float32).reshape(10, 2)
        for i in range(10):
            acc = zf[12 * i] * np.float32(r12)
            for j in range(1, 12):
                acc = (zf[12 * i + j].astype(np.float64) * r12 + acc.astype(np.float64)).astype(np.float32)
            z2f[i] = acc
        llr = aligned(20, np.int16)
        R.srslte_demod_soft_demodulate_s(QPSK, z2.ctypes.data, llr.ctypes.data, 10)
        assert R.srslte_sequence_pucch(self.seq, q.rnti, 2 * (tti % 10), self.cell_id) == 0
        R.srslte_scrambling_s_offset(self.seq, llr.ctypes.data, 0, 20)
        bits = aligned(16, np.uint8)
        length = q.ri_len or q.cqi_len
        corr = R.srslte_uci_decode_cqi_pucch(self.cqi, llr.ctypes.data, bits.ctypes.data, length)
        out["corr"] = np.float32(corr) / np.float32(2000)
        out["bits"] = (int(bits[0]), int(bits[1]))
        out["word"] = int(sum(int(bits[i]) << (12 - i) for i in range(13)))
        out["llr"], out["z2"] = llr.copy(), z2.copy()
        out["detected"] = True
        return out

    def decode(self, grid, tti, q):
        """srslte_enb_ul_get_pucch for request q (a PucchReq) on one subframe's grid -> dict of the srslte_hip_pucch_res_t fields, plus the
        attempt's intermediate values."""
        c = self.cfg
        fmt, n_pucch = select(self.ext, c.N_pucch_1, q, q.sr_tti)
        a = self._attempt(grid, tti, q, fmt, n_pucch)
        sr = int(a["detected"]) if q.sr_tti else 0
        if q.sr_tti and q.ack_len and not a["detected"]:  # enb_ul.c:217-224
            f1, n1 = select(self.ext, c.N_pucch_1, q, False)
            a = self._attempt(grid, tti, q, f1, n1)
        fmt = a["format"]
        drs = bool(q.cqi_len > 0 and not (not q.simul_cqi_ack and q.ack_len > 0)) or q.ri_len > 0
        ack = [(a["drs"][k] if drs else a["bits"][k]) if k < q.ack_len else 0 for k in range(2)]
        valid = (a["corr"] > c.threshold_data_valid_format1a) if fmt in (F1A, F1B) else (a["corr"] > c.threshold_data_valid_format2) if fmt >= F2 else False
        return dict(a, detected=int(a["detected"]), sr=sr, ack=ack, ack_valid=int(valid), cqi_crc=int(fmt >= F2 and a["corr"] > c.threshold_data_valid_format2),
                    cqi=[(a["word"] >> (12 - k)) & 1 for k in range(13)] if fmt >= F2 else [0] * 13, ri=a["bits"][0] if q.ri_len else 0)
