"""The DL control region: PCFICH / PDCCH / PHICH receive (UE side) and transmit (eNB side), and the broadcast signals PSS, SSS and PBCH."""
import ctypes as C

import numpy as np

from ._native import (SRSLTE_SUCCESS, DevBuf, Handle, P, _check, cint, host_copy, lib, read_structs, result_structs, struct_array, sync, u16, u32,
                      void, vp)

# ---------------------------------------------------------------- DL control region receive (phy_hip.h "DL control region receive")
DCI_FORMAT0, DCI_FORMAT1, DCI_FORMAT1A, DCI_FORMAT1C, DCI_FORMAT1B, DCI_FORMAT1D, DCI_FORMAT2, DCI_FORMAT2A, DCI_FORMAT2B = range(9)  # srslte_dci_format_t
DL_CTRL_MAX_CAND = 38
DL_CTRL_MAX_UL_DCI = 5


class DlCtrlCfg(C.Structure):
    """srslte_hip_dl_ctrl_cfg_t: the cell (srslte_cell_t) and the object's batch size."""
    C_TYPE = "srslte_hip_dl_ctrl_cfg_t"
    _fields_ = [("nof_prb", C.c_uint32), ("nof_ports", C.c_uint32), ("cell_id", C.c_uint32), ("cp_ext", C.c_int), ("phich_resources", C.c_int),
                ("phich_ext", C.c_int), ("tdd", C.c_int), ("nof_rx_antennas", C.c_uint32), ("max_batch", C.c_uint32)]


class DlCtrlReq(C.Structure):
    """srslte_hip_dl_ctrl_req_t: RNTI, srslte_tm_t (0-3), CFI (0 = from the PCFICH) and the MBSFN flag of one subframe."""
    C_TYPE = "srslte_hip_dl_ctrl_req_t"
    _fields_ = [("rnti", C.c_uint16), ("tm", C.c_uint32), ("cfi", C.c_uint32), ("mbsfn", C.c_int)]


class DlCtrlRes(C.Structure):
    """srslte_hip_dl_ctrl_res_t."""
    C_TYPE = "srslte_hip_dl_ctrl_res_t"
    _fields_ = [("cfi", C.c_uint32), ("cfi_corr", C.c_float), ("nof_dci", C.c_uint32)]


class DciMsg(C.Structure):
    """srslte_hip_dci_msg_t = srslte_dci_msg_t (dci.h:65-71)."""
    C_TYPE = "srslte_hip_dci_msg_t"
    _fields_ = [("payload", C.c_uint8 * 128), ("nof_bits", C.c_uint32), ("L", C.c_uint32), ("ncce", C.c_uint32), ("format", C.c_int), ("rnti", C.c_uint16)]


class DlCtrlCand(C.Structure):
    """srslte_hip_dl_ctrl_cand_t: one searched candidate."""
    C_TYPE = "srslte_hip_dl_ctrl_cand_t"
    _fields_ = [("L", C.c_uint32), ("ncce", C.c_uint32), ("format", C.c_uint32), ("nof_bits", C.c_uint32), ("skipped", C.c_uint32), ("crc_rem", C.c_uint32),
                ("format_decoded", C.c_uint32), ("payload", C.c_uint8 * 128)]


class DlCtrlUlRes(C.Structure):
    """srslte_hip_dl_ctrl_ul_res_t: the UL DCIs of one subframe; pending = 1 if they are the DL search's pending list."""
    C_TYPE = "srslte_hip_dl_ctrl_ul_res_t"
    _fields_ = [("nof_ul_dci", C.c_uint32), ("pending", C.c_uint32)]


class PhichReq(C.Structure):
    """srslte_hip_phich_req_t: the srslte_phich_grant_t of the PUSCH a PHICH acknowledges, with its subframe within the batch."""
    C_TYPE = "srslte_hip_phich_req_t"
    _fields_ = [("sf", C.c_uint32), ("n_prb_lowest", C.c_uint32), ("n_dmrs", C.c_uint32), ("I_phich", C.c_uint32)]


class PhichRes(C.Structure):
    """srslte_hip_phich_res_t: srslte_phich_res_t and the srslte_phich_resource_t it was read from."""
    C_TYPE = "srslte_hip_phich_res_t"
    _fields_ = [("ack_value", C.c_uint32), ("distance", C.c_float), ("ngroup", C.c_uint32), ("nseq", C.c_uint32)]


class PhichSoft(C.Structure):
    """srslte_hip_phich_soft_t: z after de-spreading (re, im) and the three BPSK soft bits of one PHICH."""
    C_TYPE = "srslte_hip_phich_soft_t"
    _fields_ = [("z", (C.c_float * 2) * 3), ("bits", C.c_float * 3)]


class MibRes(C.Structure):
    """srslte_hip_mib_res_t: the MIB of one subframe."""
    C_TYPE = "srslte_hip_mib_res_t"
    _fields_ = [("found", C.c_uint32), ("nof_tx_ports", C.c_uint32), ("sfn_offset", C.c_int32), ("nof_prb", C.c_uint32), ("phich_ext", C.c_uint32),
                ("phich_resources", C.c_uint32), ("sfn", C.c_uint32), ("payload", C.c_uint8 * 24)]


class MibCand(C.Structure):
    """srslte_hip_mib_cand_t: one decode_frame of the MIB decoder."""
    C_TYPE = "srslte_hip_mib_cand_t"
    _fields_ = [("nant", C.c_uint32), ("dst", C.c_uint32), ("hit", C.c_uint32), ("data", C.c_uint8 * 40)]


# ---------------------------------------------------------------- DL control region transmit (phy_hip.h "DL control region transmit")
class DlCtrlTxCfg(C.Structure):
    """srslte_hip_dl_ctrl_tx_cfg_t: the cell and the per-call limits."""
    C_TYPE = "srslte_hip_dl_ctrl_tx_cfg_t"
    _fields_ = [("nof_prb", C.c_uint32), ("nof_ports", C.c_uint32), ("cell_id", C.c_uint32), ("cp_ext", C.c_int), ("phich_resources", C.c_int),
                ("phich_ext", C.c_int), ("tdd", C.c_int), ("max_batch", C.c_uint32), ("max_dci", C.c_uint32), ("max_phich", C.c_uint32)]


class DlCtrlTxDci(C.Structure):
    """srslte_hip_dl_ctrl_tx_dci_t: a DCI message and its subframe within the batch."""
    C_TYPE = "srslte_hip_dl_ctrl_tx_dci_t"
    _fields_ = [("sf", C.c_uint32), ("msg", DciMsg)]


class PhichTx(C.Structure):
    """srslte_hip_phich_tx_t: srslte_phich_grant_t and the ack of one PHICH, with its subframe within the batch."""
    C_TYPE = "srslte_hip_phich_tx_t"
    _fields_ = [("sf", C.c_uint32), ("n_prb_lowest", C.c_uint32), ("n_dmrs", C.c_uint32), ("I_phich", C.c_uint32), ("ack", C.c_uint8)]


class DlCtrlTxIn(C.Structure):
    """srslte_hip_dl_ctrl_tx_in_t."""
    C_TYPE = "srslte_hip_dl_ctrl_tx_in_t"
    _fields_ = [("cfi", C.c_void_p), ("dci", C.POINTER(DlCtrlTxDci)), ("nof_dci", C.c_uint32), ("phich", C.POINTER(PhichTx)), ("nof_phich", C.c_uint32)]


_TX_GRANTS_CTRL = [vp, vp, u32, u32, u32, vp, u32, vp, P(DlCtrlTxIn), vp, vp]

SIGNATURES = {
    # DL control region receive
    "srslte_hip_dl_ctrl_create": (vp, [P(DlCtrlCfg)]),
    "srslte_hip_dl_ctrl_create_tdd": (vp, [P(DlCtrlCfg), u32]),
    "srslte_hip_dl_ctrl_destroy": (void, [vp]),
    "srslte_hip_dl_ctrl_batch": (None, [vp, vp, vp, vp, u32, u32, vp, vp, vp, vp]),
    "srslte_hip_dl_ctrl_debug_buffer": (vp, [vp, cint]),
    "srslte_hip_dl_ctrl_llr_stride": (u32, [vp]),
    "srslte_hip_dl_ctrl_pcfich_re": (None, [P(DlCtrlCfg), vp, u32]),
    "srslte_hip_dl_ctrl_pdcch_re": (None, [P(DlCtrlCfg), u32, vp, u32]),
    "srslte_hip_pdcch_ue_locations_ncce": (u32, [u32, vp, u32, u32, u16]),
    "srslte_hip_pdcch_common_locations_ncce": (u32, [u32, vp, u32]),
    "srslte_hip_dci_format_sizeof": (u32, [u32, u32, cint]),
    "srslte_hip_dl_ctrl_tdd_mi": (cint, [u32, u32]),
    "srslte_hip_dl_ctrl_pdcch_re_tdd": (None, [P(DlCtrlCfg), u32, u32, u32, vp, u32]),
    "srslte_hip_dci_format_sizeof_tdd": (u32, [u32, u32, cint]),
    # DL control region receive: UL DCIs and PHICH
    "srslte_hip_dl_ctrl_set_max_phich": (None, [vp, u32]),
    "srslte_hip_dl_ctrl_batch_ul": (None, [vp, vp, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp, u32, vp, vp]),
    "srslte_hip_dl_ctrl_phich_batch": (None, [vp, vp, vp, vp, u32, u32, vp, u32, vp, vp]),
    "srslte_hip_dl_ctrl_phich_debug_buffer": (vp, [vp]),
    # DL control region transmit
    "srslte_hip_dl_ctrl_tx_create": (vp, [P(DlCtrlTxCfg)]),
    "srslte_hip_dl_ctrl_tx_create_tdd": (vp, [P(DlCtrlTxCfg), u32]),
    "srslte_hip_dl_ctrl_tx_destroy": (void, [vp]),
    "srslte_hip_dl_ctrl_tx_put": (None, [vp, u32, u32, P(DlCtrlTxIn), vp, vp]),
    "srslte_hip_dl_tx_batch_grants_ctrl": (None, _TX_GRANTS_CTRL),
    "srslte_hip_dl_ctrl_phich_ngroups": (None, [P(DlCtrlTxCfg)]),
    "srslte_hip_phich_calc": (None, [P(DlCtrlTxCfg), u32, u32, u32, P(u32), P(u32)]),
    "srslte_hip_dl_ctrl_phich_re": (None, [P(DlCtrlTxCfg), u32, vp, u32]),
    "srslte_hip_dl_ctrl_phich_ngroups_tdd": (None, [P(DlCtrlTxCfg), u32, u32]),
    "srslte_hip_dl_ctrl_phich_re_tdd": (None, [P(DlCtrlTxCfg), u32, u32, u32, vp, u32]),
    # DL broadcast
    "srslte_hip_dl_ctrl_tx_put_bcast": (None, [vp, u32, u32, vp, vp]),
    "srslte_hip_dl_tx_batch_grants_full": (None, _TX_GRANTS_CTRL),
    "srslte_hip_dl_tx_batch_grants2_ctrl": (None, _TX_GRANTS_CTRL),
    "srslte_hip_dl_tx_batch_grants2_full": (None, _TX_GRANTS_CTRL),
    "srslte_hip_dl_ctrl_mib_batch": (None, [vp, vp, vp, vp, u32, u32, cint, vp, vp]),
    "srslte_hip_dl_ctrl_mib_debug_buffer": (vp, [vp, cint]),
    "srslte_hip_pbch_re": (None, [P(DlCtrlCfg), vp, u32]),
    "srslte_hip_sync_re": (None, [P(DlCtrlCfg), u32, vp, vp, u32]),
    "srslte_hip_pbch_mib_pack": (None, [u32, cint, cint, u32, vp]),
}


def _ctrl_cfg(nof_prb, nof_ports, cell_id, cp_ext=False, phich_resources=0, phich_ext=False, nof_rx=1, max_batch=1, tdd=False):
    return DlCtrlCfg(nof_prb, nof_ports, cell_id, 1 if cp_ext else 0, phich_resources, 1 if phich_ext else 0, 1 if tdd else 0, nof_rx, max_batch)


def _re_list(name, n, out):
    """The count n that a host-only *_re / *_pack function answered -> the first n entries of out."""
    if n < 0:
        raise ValueError("%s: %d" % (name, n))
    return out[:n]


def pcfich_re(nof_prb, nof_ports, cell_id, cp_ext=False, phich_resources=0, phich_ext=False):
    """The 16 PCFICH REs as indices into one antenna's [nsym][12 nof_prb] grid, in srslte_regs_pcfich_get's order (host; no GPU)."""
    out = np.zeros(16, np.uint32)
    cfg = _ctrl_cfg(nof_prb, nof_ports, cell_id, cp_ext, phich_resources, phich_ext)
    return _re_list("srslte_hip_dl_ctrl_pcfich_re", lib().srslte_hip_dl_ctrl_pcfich_re(C.byref(cfg), out.ctypes.data, 16), out)


def pdcch_re(nof_prb, nof_ports, cell_id, cfi, cp_ext=False, phich_resources=0, phich_ext=False):
    """The 36 NOF_CCE(cfi) PDCCH REs in srslte_regs_pdcch_get's order (host; no GPU)."""
    out = np.zeros(14 * 12 * 110, np.uint32)
    cfg = _ctrl_cfg(nof_prb, nof_ports, cell_id, cp_ext, phich_resources, phich_ext)
    return _re_list("srslte_hip_dl_ctrl_pdcch_re", lib().srslte_hip_dl_ctrl_pdcch_re(C.byref(cfg), cfi, out.ctypes.data, out.size), out)


def pdcch_ue_locations(nof_cce, sf_idx, rnti, max_candidates=16):
    """srslte_pdcch_ue_locations_ncce -> [(L, ncce), ...] (host)."""
    loc = np.zeros(2 * max_candidates, np.uint32)
    k = lib().srslte_hip_pdcch_ue_locations_ncce(nof_cce, loc.ctypes.data, max_candidates, sf_idx, rnti)
    return [(int(loc[2 * i]), int(loc[2 * i + 1])) for i in range(k)]


def pdcch_common_locations(nof_cce, max_candidates=6):
    """srslte_pdcch_common_locations_ncce -> [(L, ncce), ...] (host)."""
    loc = np.zeros(2 * max_candidates, np.uint32)
    k = lib().srslte_hip_pdcch_common_locations_ncce(nof_cce, loc.ctypes.data, max_candidates)
    return [(int(loc[2 * i]), int(loc[2 * i + 1])) for i in range(k)]


def dci_format_sizeof(nof_prb, nof_ports, fmt):
    """srslte_dci_format_sizeof for an FDD cell with a zero srslte_dci_cfg_t (host)."""
    return lib().srslte_hip_dci_format_sizeof(nof_prb, nof_ports, fmt)


def tdd_mi(tdd_sf_config, sf_idx):
    """mi of 36.213 Table 6.9-1 for subframe sf_idx of uplink-downlink configuration tdd_sf_config; < 0: uplink subframe or invalid (host)."""
    return lib().srslte_hip_dl_ctrl_tdd_mi(tdd_sf_config, sf_idx)


def pdcch_re_tdd(nof_prb, nof_ports, cell_id, tdd_sf_config, sf_idx, cfi, cp_ext=False, phich_resources=0, phich_ext=False):
    """pdcch_re for subframe sf_idx of a TDD cell: the list of srslte_regs_init_opts(cell, mi, sf1_6) (host; no GPU)."""
    out = np.zeros(14 * 12 * 110, np.uint32)
    cfg = _ctrl_cfg(nof_prb, nof_ports, cell_id, cp_ext, phich_resources, phich_ext, tdd=True)
    n = lib().srslte_hip_dl_ctrl_pdcch_re_tdd(C.byref(cfg), tdd_sf_config, sf_idx, cfi, out.ctypes.data, out.size)
    return _re_list("srslte_hip_dl_ctrl_pdcch_re_tdd", n, out)


def dci_format_sizeof_tdd(nof_prb, nof_ports, fmt):
    """srslte_dci_format_sizeof for a TDD cell with a zero srslte_dci_cfg_t (host)."""
    return lib().srslte_hip_dci_format_sizeof_tdd(nof_prb, nof_ports, fmt)


def pbch_re(nof_prb, nof_ports, cell_id, cp_ext=False):
    """The PBCH REs of one port's subframe grid in srslte_pbch_put's order (host; no GPU)."""
    out = np.zeros(240, np.uint32)
    return _re_list("srslte_hip_pbch_re", lib().srslte_hip_pbch_re(C.byref(_ctrl_cfg(nof_prb, nof_ports, cell_id, cp_ext)), out.ctypes.data, out.size), out)


def sync_re(nof_prb, cell_id, sf_idx, cp_ext=False):
    """The 72 PSS then 72 SSS REs of subframe sf_idx (0 / 5) with the zero guards -> (re [144] uint32, values [144] complex64) (host)."""
    re, val = np.zeros(144, np.uint32), np.zeros(144, np.complex64)
    n = lib().srslte_hip_sync_re(C.byref(_ctrl_cfg(nof_prb, 1, cell_id, cp_ext)), sf_idx, re.ctypes.data, val.ctypes.data, 144)
    if n < 0:
        raise ValueError("srslte_hip_sync_re: %d" % n)
    return re, val


def mib_pack(nof_prb, phich_ext, phich_resources, sfn):
    """srslte_pbch_mib_pack -> 24 bits (uint8) (host)."""
    out = np.zeros(24, np.uint8)
    n = lib().srslte_hip_pbch_mib_pack(nof_prb, 1 if phich_ext else 0, phich_resources, sfn, out.ctypes.data)
    if n < 0:
        raise ValueError("srslte_hip_pbch_mib_pack: %d" % n)
    return out


def _phich_reqs(phichs):
    """PhichReq or (sf, n_prb_lowest, n_dmrs, I_phich) -> a ctypes array, or None when empty."""
    return struct_array(PhichReq, [x if isinstance(x, PhichReq) else PhichReq(*x) for x in phichs]) if len(phichs) else None


class DlCtrl(Handle):
    """Batched control-region receive: srslte_pcfich_decode + srslte_pdcch_extract_llr + the DL DCI blind search of srslte_ue_dl_find_dl_dci;
    with batch_ul / phich also srslte_ue_dl_find_ul_dci and srslte_ue_dl_decode_phich (max_phich: PHICH requests per call)."""
    DESTROY = "srslte_hip_dl_ctrl_destroy"

    def __init__(self, nof_prb, nof_ports, cell_id, cp_ext=False, phich_resources=0, phich_ext=False, nof_rx=1, max_batch=1, tdd=False, max_phich=0,
                 tdd_sf_config=None):
        """tdd_sf_config 0-6: a TDD cell of that uplink-downlink configuration (srslte_hip_dl_ctrl_create_tdd); tdd alone is refused."""
        self.cfg = _ctrl_cfg(nof_prb, nof_ports, cell_id, cp_ext, phich_resources, phich_ext, nof_rx, max_batch, tdd or tdd_sf_config is not None)
        if tdd_sf_config is None:
            self._create("srslte_hip_dl_ctrl_create", C.byref(self.cfg))
        else:
            self._create("srslte_hip_dl_ctrl_create_tdd", C.byref(self.cfg), tdd_sf_config)
        self.grid_len = (12 if cp_ext else 14) * 12 * nof_prb
        self.nof_ports, self.nof_rx, self.max_batch = nof_ports, nof_rx, max_batch
        self.llr_stride = lib().srslte_hip_dl_ctrl_llr_stride(self.h)
        if max_phich:
            self.set_max_phich(max_phich)

    def set_max_phich(self, max_phich):
        """srslte_hip_dl_ctrl_set_max_phich: room for max_phich PHICH requests per call (waits for the device)."""
        _check(lib().srslte_hip_dl_ctrl_set_max_phich(self.h, max_phich), "srslte_hip_dl_ctrl_set_max_phich")

    def batch_ul_device(self, d_grid, d_ce, d_res, tti0, reqs, d_out, d_msg, d_ul_out, d_ul_msg, phichs=(), d_phich_res=None, stream=None):
        """srslte_hip_dl_ctrl_batch_ul on device pointers; reqs: list of DlCtrlReq, phichs: PhichReq or tuples. Returns the status code."""
        return lib().srslte_hip_dl_ctrl_batch_ul(self.h, d_grid, d_ce, d_res, tti0, len(reqs), struct_array(DlCtrlReq, reqs), d_out, d_msg, d_ul_out,
                                                 d_ul_msg, _phich_reqs(phichs), len(phichs), d_phich_res, stream)

    def phich_device(self, d_grid, d_ce, d_res, tti0, nof_sf, phichs, d_phich_res, stream=None):
        """srslte_hip_dl_ctrl_phich_batch on device pointers -> the status code."""
        return lib().srslte_hip_dl_ctrl_phich_batch(self.h, d_grid, d_ce, d_res, tti0, nof_sf, _phich_reqs(phichs), len(phichs), d_phich_res, stream)

    def _upload(self, n, grid, ce, res):
        g = np.ascontiguousarray(grid, np.complex64).reshape(n, self.nof_rx, self.grid_len)
        h = np.ascontiguousarray(ce, np.complex64).reshape(n, self.nof_ports, self.nof_rx, self.grid_len)
        r = np.ascontiguousarray(res, np.float32).reshape(n, 10)
        return DevBuf.from_host(g), DevBuf.from_host(h), DevBuf.from_host(r)

    def batch_ul(self, grid, ce, res, tti0, reqs, phichs=()):
        """grid, ce, res as batch takes them -> (rc, [DlCtrlRes], [DciMsg], [DlCtrlUlRes], [[DciMsg] per subframe, nof_ul_dci long], [PhichRes])."""
        n, m = len(reqs), len(phichs)
        dg, dh, dr = self._upload(n, grid, ce, res)
        dout, dmsg = DevBuf(C.sizeof(DlCtrlRes) * n), DevBuf(C.sizeof(DciMsg) * n)
        dul, dulm = DevBuf(C.sizeof(DlCtrlUlRes) * n), DevBuf(C.sizeof(DciMsg) * n * DL_CTRL_MAX_UL_DCI)
        dph = DevBuf(C.sizeof(PhichRes) * max(1, m))
        rc = self.batch_ul_device(dg.ptr, dh.ptr, dr.ptr, tti0, reqs, dout.ptr, dmsg.ptr, dul.ptr, dulm.ptr, phichs, dph.ptr)
        if rc != SRSLTE_SUCCESS:
            return rc, None, None, None, None, None
        sync()
        ul, ulm = read_structs(dul.ptr, DlCtrlUlRes, n), read_structs(dulm.ptr, DciMsg, n * DL_CTRL_MAX_UL_DCI)
        ul_msgs = [ulm[b * DL_CTRL_MAX_UL_DCI:b * DL_CTRL_MAX_UL_DCI + ul[b].nof_ul_dci] for b in range(n)]
        return rc, read_structs(dout.ptr, DlCtrlRes, n), read_structs(dmsg.ptr, DciMsg, n), ul, ul_msgs, read_structs(dph.ptr, PhichRes, m)

    def phich(self, grid, ce, res, tti0, phichs):
        """srslte_hip_dl_ctrl_phich_batch: grid, ce, res as batch takes them -> (rc, [PhichRes] or None)."""
        n, m = len(res), len(phichs)
        dg, dh, dr = self._upload(n, grid, ce, res)
        dph = DevBuf(C.sizeof(PhichRes) * max(1, m))
        return result_structs(self.phich_device(dg.ptr, dh.ptr, dr.ptr, tti0, n, phichs, dph.ptr), dph.ptr, PhichRes, m)

    def phich_soft(self, nof_phich):
        """The PHICH debug buffer of the last call: [PhichSoft] (z after de-spreading and the soft bits of each request)."""
        return read_structs(lib().srslte_hip_dl_ctrl_phich_debug_buffer(self.h), PhichSoft, nof_phich)

    def run_device(self, d_grid, d_ce, d_res, tti0, reqs, d_out, d_msg, stream=None):
        """Device pointers in and out; reqs: list of DlCtrlReq. Returns the status code."""
        return lib().srslte_hip_dl_ctrl_batch(self.h, d_grid, d_ce, d_res, tti0, len(reqs), struct_array(DlCtrlReq, reqs), d_out, d_msg, stream)

    def batch(self, grid, ce, res, tti0, reqs):
        """grid [nof_sf][nof_rx][grid_len], ce [nof_sf][nof_ports][nof_rx][grid_len] (complex64), res [nof_sf][10] float32 (srslte_hip_chest_dl_res_t)
        -> (rc, [DlCtrlRes], [DciMsg])."""
        n = len(reqs)
        dg, dh, dr = self._upload(n, grid, ce, res)
        dout, dmsg = DevBuf(C.sizeof(DlCtrlRes) * n), DevBuf(C.sizeof(DciMsg) * n)
        rc = self.run_device(dg.ptr, dh.ptr, dr.ptr, tti0, reqs, dout.ptr, dmsg.ptr)
        if rc != SRSLTE_SUCCESS:
            return rc, None, None
        sync()
        return rc, read_structs(dout.ptr, DlCtrlRes, n), read_structs(dmsg.ptr, DciMsg, n)

    def llr(self, nof_sf):
        """Debug buffer 0: the LLR rows of the last call, [nof_sf][llr_stride] float32."""
        return host_copy(lib().srslte_hip_dl_ctrl_debug_buffer(self.h, 0), np.float32, nof_sf * self.llr_stride).reshape(nof_sf, self.llr_stride)

    def candidates(self, nof_sf):
        """Debug buffers 1 and 2: for each subframe of the last call the list of DlCtrlCand in search order."""
        cand = read_structs(lib().srslte_hip_dl_ctrl_debug_buffer(self.h, 1), DlCtrlCand, nof_sf * DL_CTRL_MAX_CAND)
        cnt = host_copy(lib().srslte_hip_dl_ctrl_debug_buffer(self.h, 2), np.uint32, nof_sf)
        return [cand[b * DL_CTRL_MAX_CAND:b * DL_CTRL_MAX_CAND + int(cnt[b])] for b in range(nof_sf)]

    def decode_mib_device(self, d_grid, d_ce, d_res, tti0, nof_sf, search_all_ports, d_mib, stream=None):
        """srslte_hip_dl_ctrl_mib_batch on device pointers -> the status code."""
        return lib().srslte_hip_dl_ctrl_mib_batch(self.h, d_grid, d_ce, d_res, tti0, nof_sf, 1 if search_all_ports else 0, d_mib, stream)

    def decode_mib(self, grid, ce, res, tti0, search_all_ports=True):
        """srslte_hip_dl_ctrl_mib_batch: grid, ce, res as batch takes them -> (rc, [MibRes] or None)."""
        n = len(res)
        dg, dh, dr = self._upload(n, grid, ce, res)
        dm = DevBuf(C.sizeof(MibRes) * n)
        return result_structs(self.decode_mib_device(dg.ptr, dh.ptr, dr.ptr, tti0, n, search_all_ports, dm.ptr), dm.ptr, MibRes, n)

    def mib_llr(self, nof_sf):
        """MIB debug buffer 0: [nof_sf][3][480] float32, rows of nant 1, 2, 4."""
        return host_copy(lib().srslte_hip_dl_ctrl_mib_debug_buffer(self.h, 0), np.float32, nof_sf * 3 * 480).reshape(nof_sf, 3, 480)

    def mib_candidates(self, nof_sf):
        """MIB debug buffer 1: [nof_sf][3][4] MibCand (nant 1, 2, 4; dst 0-3)."""
        cand = read_structs(lib().srslte_hip_dl_ctrl_mib_debug_buffer(self.h, 1), MibCand, nof_sf * 12)
        return [[cand[(b * 3 + s) * 4:(b * 3 + s) * 4 + 4] for s in range(3)] for b in range(nof_sf)]


def _ctrl_tx_cfg(nof_prb, nof_ports, cell_id, cp_ext=False, phich_resources=0, phich_ext=False, max_batch=1, max_dci=0, max_phich=0, tdd=False):
    return DlCtrlTxCfg(nof_prb, nof_ports, cell_id, 1 if cp_ext else 0, phich_resources, 1 if phich_ext else 0, 1 if tdd else 0, max_batch, max_dci,
                       max_phich)


def _ctrl_tx_in(cfi, dcis, phichs):
    """(DlCtrlTxIn, the ctypes arrays it points at). dcis: (sf, msg) with msg anything of the srslte_dci_msg_t layout; phichs: PhichTx or
    (sf, n_prb_lowest, n_dmrs, I_phich, ack)."""
    c = np.ascontiguousarray(cfi, np.uint32)
    d = struct_array(DlCtrlTxDci, [DlCtrlTxDci(sf, DciMsg.from_buffer_copy(bytes(m)[:C.sizeof(DciMsg)])) for sf, m in dcis])
    p = struct_array(PhichTx, [x if isinstance(x, PhichTx) else PhichTx(*x) for x in phichs])
    return DlCtrlTxIn(c.ctypes.data if c.size else None, d, len(dcis), p, len(phichs)), (c, d, p)


def phich_ngroups(nof_prb, nof_ports, cell_id, cp_ext=False, phich_resources=0, phich_ext=False):
    """srslte_regs_phich_ngroups (PHICH groups; x 2 on an extended-CP cell) (host; no GPU)."""
    n = lib().srslte_hip_dl_ctrl_phich_ngroups(C.byref(_ctrl_tx_cfg(nof_prb, nof_ports, cell_id, cp_ext, phich_resources, phich_ext)))
    if n < 0:
        raise ValueError("srslte_hip_dl_ctrl_phich_ngroups: %d" % n)
    return n


def phich_calc(nof_prb, nof_ports, cell_id, n_prb_lowest, n_dmrs, I_phich, cp_ext=False, phich_resources=0, phich_ext=False):
    """srslte_phich_calc -> (ngroup, nseq) (host)."""
    g, q = C.c_uint32(0), C.c_uint32(0)
    rc = lib().srslte_hip_phich_calc(C.byref(_ctrl_tx_cfg(nof_prb, nof_ports, cell_id, cp_ext, phich_resources, phich_ext)), n_prb_lowest, n_dmrs, I_phich,
                                     C.byref(g), C.byref(q))
    if rc != SRSLTE_SUCCESS:
        raise ValueError("srslte_hip_phich_calc: %d" % rc)
    return g.value, q.value


def phich_re(nof_prb, nof_ports, cell_id, ngroup, cp_ext=False, phich_resources=0, phich_ext=False):
    """The 12 REs of PHICH group ngroup in srslte_regs_phich_add's order (host)."""
    out = np.zeros(12, np.uint32)
    cfg = _ctrl_tx_cfg(nof_prb, nof_ports, cell_id, cp_ext, phich_resources, phich_ext)
    return _re_list("srslte_hip_dl_ctrl_phich_re", lib().srslte_hip_dl_ctrl_phich_re(C.byref(cfg), ngroup, out.ctypes.data, 12), out)


def phich_ngroups_tdd(nof_prb, nof_ports, cell_id, tdd_sf_config, sf_idx, cp_ext=False, phich_resources=0, phich_ext=False):
    """PHICH groups of subframe sf_idx of a TDD cell: mi srslte_regs_phich_ngroups_m1 (x 2 on an extended-CP cell). ValueError for an uplink
    subframe, and for a cell and configuration the device refuses because two mapping units share a REG (host; no GPU)."""
    cfg = _ctrl_tx_cfg(nof_prb, nof_ports, cell_id, cp_ext, phich_resources, phich_ext, tdd=True)
    n = lib().srslte_hip_dl_ctrl_phich_ngroups_tdd(C.byref(cfg), tdd_sf_config, sf_idx)
    if n < 0:
        raise ValueError("srslte_hip_dl_ctrl_phich_ngroups_tdd: %d" % n)
    return n


def phich_re_tdd(nof_prb, nof_ports, cell_id, tdd_sf_config, sf_idx, ngroup, cp_ext=False, phich_resources=0, phich_ext=False):
    """phich_re for subframe sf_idx of a TDD cell (host)."""
    out = np.zeros(12, np.uint32)
    cfg = _ctrl_tx_cfg(nof_prb, nof_ports, cell_id, cp_ext, phich_resources, phich_ext, tdd=True)
    n = lib().srslte_hip_dl_ctrl_phich_re_tdd(C.byref(cfg), tdd_sf_config, sf_idx, ngroup, out.ctypes.data, 12)
    return _re_list("srslte_hip_dl_ctrl_phich_re_tdd", n, out)


class DlCtrlTx(Handle):
    """Batched control-region transmit: the PCFICH of srslte_enb_dl_put_base, srslte_enb_dl_put_phich and srslte_enb_dl_put_pdcch_dl / _ul."""
    DESTROY = "srslte_hip_dl_ctrl_tx_destroy"

    def __init__(self, nof_prb, nof_ports, cell_id, cp_ext=False, phich_resources=0, phich_ext=False, max_batch=1, max_dci=16, max_phich=16, tdd=False,
                 tdd_sf_config=None):
        """tdd_sf_config 0-6: a TDD cell of that uplink-downlink configuration (srslte_hip_dl_ctrl_tx_create_tdd); tdd alone is refused."""
        self.cfg = _ctrl_tx_cfg(nof_prb, nof_ports, cell_id, cp_ext, phich_resources, phich_ext, max_batch, max_dci, max_phich,
                                tdd or tdd_sf_config is not None)
        if tdd_sf_config is None:
            self._create("srslte_hip_dl_ctrl_tx_create", C.byref(self.cfg))
        else:
            self._create("srslte_hip_dl_ctrl_tx_create_tdd", C.byref(self.cfg), tdd_sf_config)
        self.grid_len = (12 if cp_ext else 14) * 12 * nof_prb
        self.nof_ports, self.max_batch = nof_ports, max_batch

    def put_device(self, d_grid, tti0, nof_sf, cfi, dcis=(), phichs=(), stream=None):
        """srslte_hip_dl_ctrl_tx_put on a device grid [nof_sf][nof_ports][grid_len] -> the status code."""
        inp, keep = _ctrl_tx_in(cfi, dcis, phichs)
        return lib().srslte_hip_dl_ctrl_tx_put(self.h, tti0, nof_sf, C.byref(inp), d_grid, stream)

    def put(self, grid, tti0, cfi, dcis=(), phichs=()):
        """grid [nof_sf][nof_ports][grid_len] complex64 (host), cfi [nof_sf] -> (rc, the grids after the call)."""
        g = np.ascontiguousarray(grid, np.complex64).reshape(len(cfi), self.nof_ports, self.grid_len)
        d = DevBuf.from_host(g)
        rc = self.put_device(d.ptr, tti0, len(cfi), cfi, dcis, phichs)
        sync()
        return rc, d.to_host(np.complex64).reshape(g.shape)

    def put_bcast_device(self, d_grid, tti0, nof_sf, stream=None):
        """srslte_hip_dl_ctrl_tx_put_bcast on a device grid [nof_sf][nof_ports][grid_len] -> the status code."""
        return lib().srslte_hip_dl_ctrl_tx_put_bcast(self.h, tti0, nof_sf, d_grid, stream)

    def put_bcast(self, grid, tti0):
        """PSS / SSS / PBCH of TTIs tti0 .. tti0 + nof_sf - 1 on grid [nof_sf][nof_ports][grid_len] complex64 (host) -> (rc, the grids after)."""
        g = np.ascontiguousarray(grid, np.complex64).reshape(-1, self.nof_ports, self.grid_len)
        d = DevBuf.from_host(g)
        rc = self.put_bcast_device(d.ptr, tti0, g.shape[0])
        sync()
        return rc, d.to_host(np.complex64).reshape(g.shape)
