"""UE CSI feedback (phy_hip.h "UE CSI feedback"): PMI, RI and CQI from the DL estimates, and the CQI report coding."""
import ctypes as C

import numpy as np

from ._native import DevBuf, Handle, P, _check, cint, f32, lib, result_structs, u32, void, vp

CQI_TYPE_WIDEBAND, CQI_TYPE_SUBBAND, CQI_TYPE_SUBBAND_UE, CQI_TYPE_SUBBAND_HL = range(4)
CQI_MAX_BITS = 64


class CsiRes(C.Structure):
    """srslte_hip_csi_res_t: the measurement of one subframe."""
    C_TYPE = "srslte_hip_csi_res_t"
    _fields_ = [("sinr_1l", C.c_float * 4), ("sinr_2l", C.c_float * 2), ("pmi_1l", C.c_uint32), ("pmi_2l", C.c_uint32), ("cn_db", C.c_float),
                ("ri_cn", C.c_uint32), ("ri", C.c_uint32), ("pmi", C.c_uint32), ("sinr_db", C.c_float), ("cqi_sinr", C.c_uint32),
                ("cqi_wideband", C.c_uint32), ("reserved", C.c_uint32)]


class CqiCfg(C.Structure):
    """srslte_hip_cqi_cfg_t (srslte_cqi_cfg_t)."""
    C_TYPE = "srslte_hip_cqi_cfg_t"
    _fields_ = [("type", C.c_int), ("data_enable", C.c_int), ("pmi_present", C.c_int), ("four_antenna_ports", C.c_int), ("rank_is_not_one", C.c_int),
                ("subband_label_2_bits", C.c_int), ("L", C.c_uint32), ("N", C.c_uint32)]


class CqiValue(C.Structure):
    """srslte_hip_cqi_value_t: the members of the four report structs of srslte_cqi_value_t side by side."""
    C_TYPE = "srslte_hip_cqi_value_t"
    _fields_ = [(n, C.c_uint32) for n in ("wideband_cqi", "spatial_diff_cqi", "pmi", "subband_cqi", "subband_label", "subband_diff_cqi",
                                          "wideband_cqi_cw1", "subband_diff_cqi_cw1")]


class CsiReportCfg(C.Structure):
    """srslte_hip_csi_report_cfg_t: the UE's reporting configuration; last_ri is carried in and out."""
    C_TYPE = "srslte_hip_csi_report_cfg_t"
    _fields_ = [("tm", C.c_int), ("nof_prb", C.c_uint32), ("nof_ports", C.c_uint32), ("nof_rx_antennas", C.c_uint32), ("tdd", C.c_int),
                ("periodic_configured", C.c_int), ("ri_idx_present", C.c_int), ("I_cqi_pmi", C.c_uint32), ("I_ri", C.c_uint32),
                ("format_is_subband", C.c_int), ("aperiodic_mode", C.c_int), ("snr_to_cqi_offset", C.c_float), ("last_ri", C.c_uint32)]


class CsiReport(C.Structure):
    """srslte_hip_csi_report_t."""
    C_TYPE = "srslte_hip_csi_report_t"
    _fields_ = [("cqi", CqiCfg), ("value", CqiValue), ("ri_len", C.c_uint32), ("ri", C.c_uint32), ("cqi_len", C.c_uint32),
                ("cqi_bits", C.c_uint8 * CQI_MAX_BITS)]


SIGNATURES = {
    "srslte_hip_csi_create": (vp, [u32, u32, u32, cint]),
    "srslte_hip_csi_destroy": (void, [vp]),
    "srslte_hip_csi_set_snr_to_cqi_offset": (None, [vp, f32]),
    "srslte_hip_csi_nof_samples": (None, [vp, P(u32), P(u32)]),
    "srslte_hip_csi_batch": (None, [vp, vp, vp, u32, vp, vp]),
    "srslte_hip_dl_rx_csi_batch": (None, [vp, u32, vp, vp]),
    "srslte_hip_dl_rx_set_snr_to_cqi_offset": (None, [vp, f32]),
    "srslte_hip_csi_decide": (None, [P(f32), u32, u32, f32, f32, f32, u32, P(CsiRes)]),
    "srslte_hip_cqi_from_snr": (u32, [f32]),
    "srslte_hip_cqi_size": (None, [P(CqiCfg)]),
    "srslte_hip_cqi_value_pack": (None, [P(CqiCfg), P(CqiValue), vp]),
    "srslte_hip_cqi_periodic_send": (None, [u32, u32, cint]),
    "srslte_hip_cqi_periodic_ri_send": (None, [u32, u32, u32, cint]),
    "srslte_hip_cqi_hl_get_no_subbands": (None, [cint]),
    "srslte_hip_csi_gen_cqi_periodic": (None, [P(CsiRes), P(CsiReportCfg), u32, u32, P(CsiReport)]),
    "srslte_hip_csi_gen_cqi_aperiodic": (None, [P(CsiRes), P(CsiReportCfg), u32, P(CsiReport)]),
}


class Csi(Handle):
    """Batched CSI measurement (select_ri_pmi / srslte_ue_dl_select_ri per subframe) on DL estimates."""
    DESTROY = "srslte_hip_csi_destroy"

    def __init__(self, nof_prb, nof_ports=2, nof_rx=2, cp_norm=True):
        self._create("srslte_hip_csi_create", nof_prb, nof_ports, nof_rx, 1 if cp_norm else 0)
        self.n = (14 if cp_norm else 12) * 12 * nof_prb
        self.nof_ports, self.nof_rx = nof_ports, nof_rx

    def set_snr_to_cqi_offset(self, offset):
        return lib().srslte_hip_csi_set_snr_to_cqi_offset(self.h, offset)

    def nof_samples(self):
        a, b = C.c_uint32(), C.c_uint32()
        _check(lib().srslte_hip_csi_nof_samples(self.h, C.byref(a), C.byref(b)), "csi_nof_samples")
        return a.value, b.value

    def run_device(self, d_ce, d_res, nof_sf, d_out, stream=None):
        return lib().srslte_hip_csi_batch(self.h, d_ce, d_res, nof_sf, d_out, stream)

    def batch(self, ce, noise_estimate, snr_db):
        """ce [nof_sf][nof_ports][nof_rx][nsym * 12 * nof_prb] complex64, noise_estimate / snr_db [nof_sf] -> (rc, [CsiRes] or None)."""
        ce = np.ascontiguousarray(ce, np.complex64).reshape(-1, self.nof_ports, self.nof_rx, self.n)
        n = ce.shape[0]
        res = np.zeros((n, 10), np.float32)
        res[:, 0], res[:, 2] = noise_estimate, snr_db
        dce, dres, dout = DevBuf.from_host(ce), DevBuf.from_host(res), DevBuf(n * C.sizeof(CsiRes))
        return result_structs(self.run_device(dce.ptr, dres.ptr, n, dout.ptr), dout.ptr, CsiRes, n)


def csi_decide(sums, n_pmi, n_cn, noise_estimate, snr_db, snr_to_cqi_offset=0.0, nof_rx=2):
    """srslte_hip_csi_decide (host): the record of one subframe from its seven sums."""
    out = CsiRes()
    _check(lib().srslte_hip_csi_decide((C.c_float * 7)(*sums), n_pmi, n_cn, noise_estimate, snr_db, snr_to_cqi_offset, nof_rx, C.byref(out)), "csi_decide")
    return out


def cqi_from_snr(snr):
    return lib().srslte_hip_cqi_from_snr(snr)


def cqi_size(cfg):
    return lib().srslte_hip_cqi_size(C.byref(cfg))


def cqi_value_pack(cfg, value):
    """-> (srslte_cqi_value_pack's return value, the 64-byte bit row)."""
    buf = np.zeros(CQI_MAX_BITS, np.uint8)
    return lib().srslte_hip_cqi_value_pack(C.byref(cfg), C.byref(value), buf.ctypes.data), buf


def cqi_periodic_send(I_cqi_pmi, tti, tdd=False):
    return bool(lib().srslte_hip_cqi_periodic_send(I_cqi_pmi, tti, 1 if tdd else 0))


def cqi_periodic_ri_send(I_cqi_pmi, I_ri, tti, tdd=False):
    return bool(lib().srslte_hip_cqi_periodic_ri_send(I_cqi_pmi, I_ri, tti, 1 if tdd else 0))


def cqi_hl_get_no_subbands(nof_prb):
    return lib().srslte_hip_cqi_hl_get_no_subbands(nof_prb)


def csi_gen_cqi_periodic(csi, cfg, wideband_value, tti):
    """srslte_ue_dl_gen_cqi_periodic on a CsiRes; cfg (CsiReportCfg) keeps last_ri. -> (rc, CsiReport)."""
    out = CsiReport()
    return lib().srslte_hip_csi_gen_cqi_periodic(C.byref(csi), C.byref(cfg), wideband_value, tti, C.byref(out)), out


def csi_gen_cqi_aperiodic(csi, cfg, wideband_value):
    """srslte_ue_dl_gen_cqi_aperiodic on a CsiRes; cfg (CsiReportCfg) keeps last_ri. -> (rc, CsiReport)."""
    out = CsiReport()
    return lib().srslte_hip_csi_gen_cqi_aperiodic(C.byref(csi), C.byref(cfg), wideband_value, C.byref(out)), out
