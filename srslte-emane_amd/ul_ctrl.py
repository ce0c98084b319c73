"""UL control: PUCCH receive and transmit, PRACH generation and detection, the sounding reference signal."""
import ctypes as C

import numpy as np

from ._native import (SRSLTE_SUCCESS, DevBuf, Handle, P, _check, cint, host_copy, lib, read_structs, result_structs, struct_array, sync, sz, u32, void,
                      vp)

# ---------------------------------------------------------------- UL control: PUCCH (phy_hip.h "UL control")
PUCCH_FORMAT_1, PUCCH_FORMAT_1A, PUCCH_FORMAT_1B, PUCCH_FORMAT_2, PUCCH_FORMAT_2A, PUCCH_FORMAT_2B = range(6)


class UlCtrlCfg(C.Structure):
    """srslte_hip_ul_ctrl_cfg_t: the cell, the common PUCCH configuration of srslte_pucch_cfg_t and the requests per call."""
    C_TYPE = "srslte_hip_ul_ctrl_cfg_t"
    _fields_ = [("nof_prb", C.c_uint32), ("cell_id", C.c_uint32), ("cp_ext", C.c_int), ("delta_pucch_shift", C.c_uint32), ("n_rb_2", C.c_uint32),
                ("N_cs", C.c_uint32), ("N_pucch_1", C.c_uint32), ("group_hopping_en", C.c_int), ("threshold_format1", C.c_float),
                ("threshold_data_valid_format1a", C.c_float), ("threshold_data_valid_format2", C.c_float), ("max_pucch", C.c_uint32), ("tdd", C.c_int)]


class PucchReq(C.Structure):
    """srslte_hip_pucch_req_t: one (subframe, UE) as srslte_enb_ul_get_pucch is given it."""
    C_TYPE = "srslte_hip_pucch_req_t"
    _fields_ = [("sf", C.c_uint32), ("rnti", C.c_uint16), ("ack_len", C.c_uint32), ("ncce", C.c_uint32), ("sr_tti", C.c_int), ("n_pucch_sr", C.c_uint32),
                ("cqi_len", C.c_uint32), ("ri_len", C.c_uint32), ("n_pucch_2", C.c_uint32), ("simul_cqi_ack", C.c_int), ("shortened", C.c_int),
                ("noise_estimate", C.c_float)]

    @classmethod
    def make(cls, sf, rnti, ack_len=0, ncce=0, sr_tti=False, n_pucch_sr=0, cqi_len=0, ri_len=0, n_pucch_2=0, simul_cqi_ack=False, shortened=False,
             noise_estimate=0.0):
        return cls(sf, rnti, ack_len, ncce, 1 if sr_tti else 0, n_pucch_sr, cqi_len, ri_len, n_pucch_2, 1 if simul_cqi_ack else 0, 1 if shortened else 0,
                   noise_estimate)


class PucchRes(C.Structure):
    """srslte_hip_pucch_res_t."""
    C_TYPE = "srslte_hip_pucch_res_t"
    _fields_ = [("detected", C.c_uint32), ("correlation", C.c_float), ("format", C.c_uint32), ("n_pucch", C.c_uint32), ("sr", C.c_uint8),
                ("ack", C.c_uint8 * 2), ("ack_valid", C.c_uint8), ("cqi", C.c_uint8 * 13), ("cqi_crc", C.c_uint8), ("ri", C.c_uint8), ("reserved", C.c_uint8)]


class PucchTx(C.Structure):
    """srslte_hip_pucch_tx_t: a request and its UCI values."""
    C_TYPE = "srslte_hip_pucch_tx_t"
    _fields_ = [("req", PucchReq), ("ack", C.c_uint8 * 2), ("sr", C.c_uint8), ("ri", C.c_uint8), ("cqi", C.c_uint8 * 12)]

    @classmethod
    def make(cls, req, ack=(0, 0), sr=0, ri=0, cqi=()):
        t = cls()
        t.req = req
        t.ack[0], t.ack[1], t.sr, t.ri = ack[0], ack[1], sr, ri
        for i, b in enumerate(cqi):
            t.cqi[i] = b
        return t


# ---------------------------------------------------------------- UL control: PRACH (phy_hip.h "UL control: PRACH")
class PrachCfg(C.Structure):
    """srslte_hip_prach_cfg_t: the cell's PRACH configuration (SIB2), the detection factor and the entries per call."""
    C_TYPE = "srslte_hip_prach_cfg_t"
    _fields_ = [("nof_prb", C.c_uint32), ("config_idx", C.c_uint32), ("root_seq_idx", C.c_uint32), ("zero_corr_zone", C.c_uint32), ("hs_flag", C.c_int),
                ("tdd", C.c_int), ("detect_factor", C.c_float), ("max_occasions", C.c_uint32), ("max_preambles", C.c_uint32)]


class PrachInfo(C.Structure):
    """srslte_hip_prach_info_t."""
    C_TYPE = "srslte_hip_prach_info_t"
    _fields_ = [("N_zc", C.c_uint32), ("N_cs", C.c_uint32), ("N_cp", C.c_uint32), ("N_seq", C.c_uint32), ("N_ifft_prach", C.c_uint32),
                ("N_ifft_ul", C.c_uint32), ("format", C.c_uint32), ("nof_roots", C.c_uint32), ("n_wins", C.c_uint32), ("max_det", C.c_uint32),
                ("nof_sf", C.c_uint32), ("root_seqs_idx", C.c_uint32 * 64)]


class PrachTx(C.Structure):
    """srslte_hip_prach_tx_t: one preamble to generate."""
    C_TYPE = "srslte_hip_prach_tx_t"
    _fields_ = [("seq_index", C.c_uint32), ("freq_offset", C.c_uint32)]


class PrachOccasion(C.Structure):
    """srslte_hip_prach_occasion_t: the first sample after the CP in the signal, and the PRACH's PRB offset."""
    C_TYPE = "srslte_hip_prach_occasion_t"
    _fields_ = [("sample", C.c_uint64), ("freq_offset", C.c_uint32), ("reserved", C.c_uint32)]


# ---------------------------------------------------------------- UL sounding reference signal (phy_hip.h "UL sounding reference signal")
SRS_MAX_CE = 72


class SrsCfg(C.Structure):
    """srslte_hip_srs_cfg_t: the cell, its SRS subframe and bandwidth configuration, the sequence hopping switches and the entries per call."""
    C_TYPE = "srslte_hip_srs_cfg_t"
    _fields_ = [("nof_prb", C.c_uint32), ("cell_id", C.c_uint32), ("cp_ext", C.c_int), ("subframe_config", C.c_uint32), ("bw_cfg", C.c_uint32),
                ("group_hopping_en", C.c_int), ("sequence_hopping_en", C.c_int), ("delta_ss", C.c_uint32), ("max_srs", C.c_uint32), ("tdd", C.c_int)]


class SrsUe(C.Structure):
    """srslte_hip_srs_ue_t: one (subframe, UE)."""
    C_TYPE = "srslte_hip_srs_ue_t"
    _fields_ = [("sf", C.c_uint32), ("B", C.c_uint32), ("b_hop", C.c_uint32), ("n_srs", C.c_uint32), ("I_srs", C.c_uint32), ("k_tc", C.c_uint32),
                ("n_rrc", C.c_uint32), ("cs_used", C.c_uint32)]

    @classmethod
    def make(cls, sf, B=0, b_hop=3, n_srs=0, I_srs=0, k_tc=0, n_rrc=0, cs_used=0):
        return cls(sf, B, b_hop, n_srs, I_srs, k_tc, n_rrc, cs_used)


class SrsRes(C.Structure):
    """srslte_hip_srs_res_t."""
    C_TYPE = "srslte_hip_srs_res_t"
    _fields_ = [("rsrp", C.c_float), ("noise_estimate", C.c_float), ("noise_estimate_dbm", C.c_float), ("snr", C.c_float), ("snr_db", C.c_float),
                ("ta_us", C.c_float), ("nof_ce", C.c_uint32)]


SIGNATURES = {
    # UL control: PUCCH
    "srslte_hip_ul_ctrl_create": (vp, [P(UlCtrlCfg)]),
    "srslte_hip_ul_ctrl_destroy": (void, [vp]),
    "srslte_hip_ul_ctrl_pucch_batch": (None, [vp, vp, u32, u32, vp, u32, vp, vp]),
    "srslte_hip_ul_ctrl_debug_buffer": (vp, [vp, cint]),
    "srslte_hip_ul_rx_batch_grants_pucch": (None, [vp, vp, u32, u32, vp, u32, vp, u32, vp, vp, vp, u32, vp, vp]),
    "srslte_hip_ul_ctrl_tx_create": (vp, [P(UlCtrlCfg)]),
    "srslte_hip_ul_ctrl_tx_destroy": (void, [vp]),
    "srslte_hip_ul_ctrl_tx_put_pucch": (None, [vp, u32, u32, vp, u32, vp, vp]),
    "srslte_hip_pucch_n_cs_cell": (None, [P(UlCtrlCfg), vp]),
    "srslte_hip_pucch_resource": (None, [P(UlCtrlCfg), vp, P(PucchReq), vp]),
    "srslte_hip_pucch_dmrs": (None, [P(UlCtrlCfg), u32, u32, u32, vp, vp]),
    # UL control: PRACH
    "srslte_hip_prach_create": (vp, [P(PrachCfg)]),
    "srslte_hip_prach_destroy": (void, [vp]),
    "srslte_hip_prach_info": (None, [vp, P(PrachInfo)]),
    "srslte_hip_prach_gen_batch": (None, [vp, vp, u32, vp, vp]),
    "srslte_hip_prach_detect_batch": (None, [vp, vp, sz, vp, u32, vp, vp, vp, vp, vp]),
    "srslte_hip_prach_cfg_info": (None, [P(PrachCfg), P(PrachInfo)]),
    "srslte_hip_prach_gen_check": (None, [P(PrachCfg), vp, u32]),
    "srslte_hip_prach_detect_check": (None, [P(PrachCfg), sz, vp, u32]),
    "srslte_hip_prach_tti_opportunity_fdd": (None, [u32, u32, cint]),
    "srslte_hip_prach_preamble_format": (None, [u32]),
    # UL sounding reference signal
    "srslte_hip_srs_create": (vp, [P(SrsCfg)]),
    "srslte_hip_srs_destroy": (void, [vp]),
    "srslte_hip_srs_tx_put": (None, [vp, u32, u32, vp, u32, vp, vp]),
    "srslte_hip_srs_rx_batch": (None, [vp, vp, u32, u32, vp, u32, vp, vp, vp]),
    "srslte_hip_ul_rx_batch_grants_pucch_srs": (None, [vp, vp, u32, u32, vp, u32, vp, u32, vp, vp, vp, u32, vp, vp, vp, u32, vp, vp, vp]),
    "srslte_hip_srs_send_cs": (None, [u32, u32]),
    "srslte_hip_srs_send_ue": (None, [u32, u32]),
    "srslte_hip_srs_rb_start_cs": (u32, [u32, u32]),
    "srslte_hip_srs_rb_L_cs": (u32, [u32, u32]),
    "srslte_hip_srs_M_sc": (u32, [P(SrsCfg), P(SrsUe)]),
    "srslte_hip_srs_k0": (u32, [P(SrsCfg), P(SrsUe), u32]),
    "srslte_hip_srs_pusch_shortened": (None, [P(SrsCfg), P(SrsUe), u32, P(u32 * 2), u32]),
    "srslte_hip_srs_pucch_shortened": (None, [P(SrsCfg), cint, cint, u32, u32]),
    "srslte_hip_srs_gen": (None, [P(SrsCfg), P(SrsUe), u32, vp]),
    "srslte_hip_srs_check": (None, [P(SrsCfg), u32, u32, vp, u32]),
}


def ul_ctrl_cfg(nof_prb, cell_id, cp_ext=False, delta_pucch_shift=1, n_rb_2=2, N_cs=0, N_pucch_1=0, group_hopping_en=False, threshold_format1=0.5,
                threshold_data_valid_format1a=0.5, threshold_data_valid_format2=0.5, max_pucch=1, tdd=False):
    return UlCtrlCfg(nof_prb, cell_id, 1 if cp_ext else 0, delta_pucch_shift, n_rb_2, N_cs, N_pucch_1, 1 if group_hopping_en else 0, threshold_format1,
                     threshold_data_valid_format1a, threshold_data_valid_format2, max_pucch, 1 if tdd else 0)


def pucch_n_cs_cell(cfg):
    """srslte_pucch_n_cs_cell -> [20][7] uint32 (host; no GPU)."""
    out = np.zeros((20, 7), np.uint32)
    _check(lib().srslte_hip_pucch_n_cs_cell(C.byref(cfg), out.ctypes.data), "pucch_n_cs_cell")
    return out


def pucch_resource(cfg, req, uci=None):
    """srslte_ue_ul_pucch_resource_selection -> (format, n_pucch, n_prb slot 0, n_prb slot 1), or None where no format fits or the
    resource lies outside the band (host).
    uci: None for the receiver's zero value, else a PucchTx whose UCI values count."""
    out = np.zeros(4, np.uint32)
    rc = lib().srslte_hip_pucch_resource(C.byref(cfg), C.byref(uci) if uci is not None else None, C.byref(req), out.ctypes.data)
    return None if rc != SRSLTE_SUCCESS else tuple(int(x) for x in out)


def pucch_dmrs(cfg, fmt, n_pucch, tti, drs_bits=(0, 0)):
    """srslte_refsignal_dmrs_pucch_gen of one configuration -> [2][N_rs][12] complex64 (host)."""
    r = np.zeros(2 * 3 * 12, np.complex64)
    b = np.array(drs_bits, np.uint8)
    n = lib().srslte_hip_pucch_dmrs(C.byref(cfg), fmt, n_pucch, tti, b.ctypes.data, r.ctypes.data)
    if n < 0:
        raise ValueError("srslte_hip_pucch_dmrs: %d" % n)
    return r[:2 * n].reshape(2, n // 12, 12)


class UlCtrl(Handle):
    """Batched PUCCH receive: srslte_enb_ul_get_pucch for a list of (subframe, UE) requests."""
    DESTROY = "srslte_hip_ul_ctrl_destroy"

    def __init__(self, nof_prb, cell_id, max_pucch=1, **kw):
        self.cfg = ul_ctrl_cfg(nof_prb, cell_id, max_pucch=max_pucch, **kw)
        self._create("srslte_hip_ul_ctrl_create", C.byref(self.cfg))
        self.grid_len = (12 if self.cfg.cp_ext else 14) * 12 * nof_prb
        self.max_pucch = max_pucch

    def run_device(self, d_grid, tti0, nof_sf, reqs, d_res, stream=None):
        return lib().srslte_hip_ul_ctrl_pucch_batch(self.h, d_grid, tti0, nof_sf, struct_array(PucchReq, reqs), len(reqs), d_res, stream)

    def batch(self, grid, tti0, reqs):
        """grid [nof_sf][grid_len] complex64 -> (rc, [PucchRes] or None)."""
        g = np.ascontiguousarray(grid, np.complex64).reshape(-1, self.grid_len)
        dg, dr = DevBuf.from_host(g), DevBuf(C.sizeof(PucchRes) * max(1, len(reqs)))
        return result_structs(self.run_device(dg.ptr, tti0, g.shape[0], reqs, dr.ptr), dr.ptr, PucchRes, len(reqs))

    def debug(self, which, nof):
        """0: equalised symbols [nof][120] complex64; 1: descrambled LLRs [nof][20] int16 (last call)."""
        dt, n = (np.complex64, 120) if which == 0 else (np.int16, 20)
        return host_copy(lib().srslte_hip_ul_ctrl_debug_buffer(self.h, which), dt, nof * n).reshape(nof, n)


class UlCtrlTx(Handle):
    """Batched PUCCH transmit: srslte_pucch_encode + the PUCCH DMRS into UE grids."""
    DESTROY = "srslte_hip_ul_ctrl_tx_destroy"

    def __init__(self, nof_prb, cell_id, max_pucch=1, **kw):
        self.cfg = ul_ctrl_cfg(nof_prb, cell_id, max_pucch=max_pucch, **kw)
        self._create("srslte_hip_ul_ctrl_tx_create", C.byref(self.cfg))
        self.grid_len = (12 if self.cfg.cp_ext else 14) * 12 * nof_prb

    def put_device(self, d_grid, tti0, nof_sf, txs, stream=None):
        return lib().srslte_hip_ul_ctrl_tx_put_pucch(self.h, tti0, nof_sf, struct_array(PucchTx, txs), len(txs), d_grid, stream)

    def put(self, grid, tti0, txs):
        """grid [nof_sf][grid_len] complex64 (host) -> (rc, the grids after the call)."""
        g = np.ascontiguousarray(grid, np.complex64).reshape(-1, self.grid_len)
        d = DevBuf.from_host(g)
        rc = self.put_device(d.ptr, tti0, g.shape[0], txs)
        sync()
        return rc, d.to_host(np.complex64).reshape(g.shape)


def prach_cfg(nof_prb, config_idx, root_seq_idx=0, zero_corr_zone=1, hs_flag=False, tdd=False, detect_factor=0.0, max_occasions=1, max_preambles=1):
    return PrachCfg(nof_prb, config_idx, root_seq_idx, zero_corr_zone, 1 if hs_flag else 0, 1 if tdd else 0, detect_factor, max_occasions, max_preambles)


def prach_cfg_info(cfg):
    """srslte_hip_prach_cfg_info -> PrachInfo, or None where create would refuse the configuration (host; no GPU)."""
    info = PrachInfo()
    return info if lib().srslte_hip_prach_cfg_info(C.byref(cfg), C.byref(info)) == SRSLTE_SUCCESS else None


def prach_tti_opportunity_fdd(config_idx, tti, allowed_subframe=-1):
    """srslte_prach_tti_opportunity_config_fdd (host)."""
    return bool(lib().srslte_hip_prach_tti_opportunity_fdd(config_idx, tti, allowed_subframe))


def prach_preamble_format(config_idx):
    return lib().srslte_hip_prach_preamble_format(config_idx)


class Prach(Handle):
    """Batched PRACH: srslte_prach_gen for a list of preambles, srslte_prach_detect_offset for a list of occasions in one signal."""
    DESTROY = "srslte_hip_prach_destroy"

    def __init__(self, nof_prb, config_idx, max_occasions=1, max_preambles=1, **kw):
        self.cfg = prach_cfg(nof_prb, config_idx, max_occasions=max_occasions, max_preambles=max_preambles, **kw)
        self._create("srslte_hip_prach_create", C.byref(self.cfg))
        self.info = PrachInfo()
        _check(lib().srslte_hip_prach_info(self.h, C.byref(self.info)), "prach_info")
        self.len = self.info.N_cp + self.info.N_seq

    def gen_device(self, txs, d_out, stream=None):
        return lib().srslte_hip_prach_gen_batch(self.h, struct_array(PrachTx, txs), len(txs), d_out, stream)

    def gen(self, txs):
        """[(seq_index, freq_offset)] -> (rc, [n][N_cp + N_seq] complex64 or None)."""
        txs = [PrachTx(*t) for t in txs]
        d = DevBuf(8 * self.len * max(1, len(txs)))
        rc = self.gen_device(txs, d.ptr)
        if rc != SRSLTE_SUCCESS:
            return rc, None
        sync()
        return rc, d.to_host(np.complex64).reshape(-1, self.len)[:len(txs)]

    def detect_device(self, d_signal, sig_len, occs, d_nof, d_idx, d_toff, d_p2a, stream=None):
        return lib().srslte_hip_prach_detect_batch(self.h, d_signal, sig_len, struct_array(PrachOccasion, occs), len(occs), d_nof, d_idx, d_toff, d_p2a,
                                                   stream)

    def detect(self, signal, occs, d_signal=None, sig_len=None):
        """signal complex64 (host; or None with its device copy d_signal of sig_len samples), occs [(sample, freq_offset)] ->
        (rc, [(indices uint32, t_offsets float32, peak_to_avg float32)] per occasion, or None)."""
        occs = [PrachOccasion(s, f, 0) for s, f in occs]
        n, md = len(occs), self.info.max_det
        keep = None
        if d_signal is None:
            keep = DevBuf.from_host(np.ascontiguousarray(signal, np.complex64))
            d_signal = keep.ptr
        if sig_len is None:
            sig_len = int(np.asarray(signal).size)
        dn, di, dt, dp = DevBuf(4 * max(1, n)), DevBuf(4 * md * max(1, n)), DevBuf(4 * md * max(1, n)), DevBuf(4 * md * max(1, n))
        rc = self.detect_device(d_signal, sig_len, occs, dn.ptr, di.ptr, dt.ptr, dp.ptr)
        if rc != SRSLTE_SUCCESS:
            return rc, None
        sync()
        nof = dn.to_host(np.uint32)[:n]
        idx = di.to_host(np.uint32).reshape(-1, md)
        tof = dt.to_host(np.float32).reshape(-1, md)
        p2a = dp.to_host(np.float32).reshape(-1, md)
        return rc, [(idx[o, :nof[o]].copy(), tof[o, :nof[o]].copy(), p2a[o, :nof[o]].copy()) for o in range(n)]


def srs_cfg(nof_prb, cell_id, bw_cfg, subframe_config=0, cp_ext=False, group_hopping_en=False, sequence_hopping_en=False, delta_ss=0, max_srs=1,
            tdd=False):
    return SrsCfg(nof_prb, cell_id, 1 if cp_ext else 0, subframe_config, bw_cfg, 1 if group_hopping_en else 0, 1 if sequence_hopping_en else 0, delta_ss,
                  max_srs, 1 if tdd else 0)


def srs_send_cs(subframe_config, sf_idx):
    return lib().srslte_hip_srs_send_cs(subframe_config, sf_idx)


def srs_send_ue(I_srs, tti):
    return lib().srslte_hip_srs_send_ue(I_srs, tti)


def srs_rb_start_cs(bw_cfg, nof_prb):
    return lib().srslte_hip_srs_rb_start_cs(bw_cfg, nof_prb)


def srs_rb_L_cs(bw_cfg, nof_prb):
    return lib().srslte_hip_srs_rb_L_cs(bw_cfg, nof_prb)


def srs_M_sc(cfg, ue):
    return lib().srslte_hip_srs_M_sc(C.byref(cfg), C.byref(ue))


def srs_k0(cfg, ue, tti):
    return lib().srslte_hip_srs_k0(C.byref(cfg), C.byref(ue), tti)


def srs_pusch_shortened(cfg, ue, tti, n_prb_tilde, L_prb):
    """srslte_refsignal_srs_pusch_shortened (host); ue None: no UE-specific SRS configured."""
    n = (C.c_uint32 * 2)(*n_prb_tilde)
    return lib().srslte_hip_srs_pusch_shortened(C.byref(cfg), C.byref(ue) if ue is not None else None, tti, C.byref(n), L_prb)


def srs_pucch_shortened(cfg, ue_configured, simul_ack, fmt, tti):
    return lib().srslte_hip_srs_pucch_shortened(C.byref(cfg), 1 if ue_configured else 0, 1 if simul_ack else 0, fmt, tti)


def srs_gen(cfg, ue, sf_idx):
    """srslte_refsignal_srs_gen -> [2][M_sc] complex64 (host; no GPU)."""
    M = srs_M_sc(cfg, ue)
    r = np.zeros(2 * max(M, 1), np.complex64)
    _check(lib().srslte_hip_srs_gen(C.byref(cfg), C.byref(ue), sf_idx, r.ctypes.data), "srs_gen")
    return r.reshape(2, -1)


def srs_check(cfg, tti0, nof_sf, ues):
    """What srslte_hip_srs_create and a call with this list would answer, without a device."""
    return lib().srslte_hip_srs_check(C.byref(cfg), tti0, nof_sf, struct_array(SrsUe, ues), len(ues))


class Srs(Handle):
    """Batched SRS: srslte_refsignal_srs_put on UE grids and the eNB's sounding receiver."""
    DESTROY = "srslte_hip_srs_destroy"

    def __init__(self, nof_prb, cell_id, bw_cfg, max_srs=1, **kw):
        self.cfg = srs_cfg(nof_prb, cell_id, bw_cfg, max_srs=max_srs, **kw)
        self._create("srslte_hip_srs_create", C.byref(self.cfg))
        self.grid_len = (12 if self.cfg.cp_ext else 14) * 12 * nof_prb

    def put_device(self, d_grid, tti0, nof_sf, ues, stream=None):
        return lib().srslte_hip_srs_tx_put(self.h, tti0, nof_sf, struct_array(SrsUe, ues), len(ues), d_grid, stream)

    def put(self, grid, tti0, ues):
        """grid [nof_sf][grid_len] complex64 (host) -> (rc, the grids after the call)."""
        g = np.ascontiguousarray(grid, np.complex64).reshape(-1, self.grid_len)
        d = DevBuf.from_host(g)
        rc = self.put_device(d.ptr, tti0, g.shape[0], ues)
        sync()
        return rc, d.to_host(np.complex64).reshape(g.shape)

    def rx_device(self, d_grid, tti0, nof_sf, ues, d_res, d_ce, stream=None):
        return lib().srslte_hip_srs_rx_batch(self.h, d_grid, tti0, nof_sf, struct_array(SrsUe, ues), len(ues), d_res, d_ce, stream)

    @staticmethod
    def read(d_res, d_ce, nof):
        """-> ([SrsRes], ce [nof][SRS_MAX_CE] complex64; entries from nof_ce on are whatever the buffer held)."""
        return read_structs(d_res.ptr, SrsRes, nof), d_ce.to_host(np.complex64).reshape(-1, SRS_MAX_CE)[:nof]

    def rx(self, grid, tti0, ues):
        """grid [nof_sf][grid_len] complex64 -> (rc, [SrsRes] or None, ce or None)."""
        g = np.ascontiguousarray(grid, np.complex64).reshape(-1, self.grid_len)
        n = max(1, len(ues))
        dg, dr, dc = DevBuf.from_host(g), DevBuf(C.sizeof(SrsRes) * n), DevBuf(8 * SRS_MAX_CE * n)
        rc = self.rx_device(dg.ptr, tti0, g.shape[0], ues, dr.ptr, dc.ptr)
        if rc != SRSLTE_SUCCESS:
            return rc, None, None
        sync()
        return (rc,) + self.read(dr, dc, len(ues))
