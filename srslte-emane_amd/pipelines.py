"""The four batched pipelines: PDSCH and PUSCH receive, PUSCH and PDSCH transmit, with the calls that take other modules' objects along
(control region, PUCCH, SRS, CSI)."""
import ctypes as C

import numpy as np

from ._native import (IQ_CF32, IQ_SC16, SRSLTE_SUCCESS, DevBuf, DevView, Handle, P, _check, cint, f32, host_copy, i64, lib, read_structs,
                      result_structs, struct_array, symbol_sz, sync, u32, void, vp)
from .core import ChestDlCfg, DmrsPuschCfg
from .csi import CsiRes
from .dl_ctrl import _ctrl_tx_in
from .ul_ctrl import SRS_MAX_CE, PucchReq, PucchRes, Srs, SrsRes, SrsUe


class DlRxCfg(C.Structure):
    C_TYPE = "srslte_hip_dl_rx_cfg_t"
    _fields_ = [("cell_id", C.c_uint32), ("nof_prb", C.c_uint32), ("cfi", C.c_uint32), ("rnti", C.c_uint16), ("mod", C.c_int),
                ("tbs", C.c_uint32), ("max_iterations", C.c_uint32), ("max_batch", C.c_uint32), ("mmse", C.c_int), ("chest_cfg", ChestDlCfg),
                ("llr_8bit", C.c_int), ("nof_rx_antennas", C.c_uint32), ("nof_ports", C.c_uint32), ("csi_enable", C.c_int), ("power_scale", C.c_int), ("p_a", C.c_float),
                ("tx_scheme", C.c_int), ("pmi", C.c_uint32), ("mod2", C.c_int), ("tbs2", C.c_uint32), ("cp_ext", C.c_int),
                ("tdd", C.c_int), ("tdd_sf_config", C.c_uint32), ("tdd_ss_config", C.c_uint32),
                ("mbsfn", C.c_int), ("mbsfn_area_id", C.c_uint32), ("non_mbsfn_region", C.c_uint32)]


class DlGrant(C.Structure):
    """srslte_hip_dl_grant_t (phy_hip.h): the per-subframe part of srslte_pdsch_cfg_t / srslte_pdsch_grant_t."""
    C_TYPE = "srslte_hip_dl_grant_t"
    _fields_ = [("prb_mask", (C.c_uint32 * 4) * 2), ("mod", C.c_int), ("tbs", C.c_uint32), ("rv", C.c_uint32), ("cfi", C.c_uint32), ("rnti", C.c_uint16),
                ("new_data", C.c_int)]

    @classmethod
    def make(cls, nof_prb, mod, tbs, rnti, cfi=1, rv=0, new_data=True, prb_mask=None):
        """prb_mask: None = every PRB in both slots, else [2][nof_prb] of 0/1 (srslte_pdsch_grant_t.prb_idx)."""
        g = cls()
        g.mod, g.tbs, g.rv, g.cfi, g.rnti, g.new_data = mod, tbs, rv, cfi, rnti, 1 if new_data else 0
        for s in range(2):
            for n in range(nof_prb):
                if prb_mask is None or prb_mask[s][n]:
                    g.prb_mask[s][n >> 5] |= 1 << (n & 31)
        return g


class DlGrant2(C.Structure):
    """srslte_hip_dl_grant2_t: a grant with its transmission scheme, pmi and second transport block."""
    C_TYPE = "srslte_hip_dl_grant2_t"
    _fields_ = [("tb0", DlGrant), ("tx_scheme", C.c_int), ("pmi", C.c_uint32), ("mod2", C.c_int), ("tbs2", C.c_uint32), ("rv2", C.c_uint32), ("new_data2", C.c_int)]


class UlRxCfg(C.Structure):
    C_TYPE = "srslte_hip_ul_rx_cfg_t"
    _fields_ = [("cell_id", C.c_uint32), ("nof_prb", C.c_uint32), ("rnti", C.c_uint16), ("mod", C.c_int), ("tbs", C.c_uint32), ("L_prb", C.c_uint32),
                ("n_prb", C.c_uint32), ("n_dmrs", C.c_uint32), ("max_iterations", C.c_uint32), ("max_batch", C.c_uint32), ("mmse", C.c_int),
                ("dmrs_cfg", DmrsPuschCfg), ("shortened", C.c_int), ("ack_len", C.c_uint32), ("I_offset_ack", C.c_uint32),
                ("ri_len", C.c_uint32), ("I_offset_ri", C.c_uint32), ("cqi_len", C.c_uint32), ("I_offset_cqi", C.c_uint32),
                ("hopping", C.c_uint32), ("n_prb_slot1", C.c_uint32), ("max_grants", C.c_uint32), ("cp_ext", C.c_int)]


class UlGrant(C.Structure):
    """srslte_hip_ul_grant_t: one PUSCH of a srslte_hip_ul_rx_batch_grants call."""
    C_TYPE = "srslte_hip_ul_grant_t"
    _fields_ = [("sf", C.c_uint32), ("rnti", C.c_uint16), ("L_prb", C.c_uint32), ("n_prb", C.c_uint32), ("n_prb_slot1", C.c_uint32), ("n_dmrs", C.c_uint32),
                ("mod", C.c_int), ("tbs", C.c_uint32), ("rv", C.c_uint32), ("new_data", C.c_int), ("ack_len", C.c_uint32), ("I_offset_ack", C.c_uint32),
                ("ri_len", C.c_uint32), ("I_offset_ri", C.c_uint32), ("cqi_len", C.c_uint32), ("I_offset_cqi", C.c_uint32)]

    @classmethod
    def make(cls, sf, rnti, L_prb, n_prb, mod, tbs, n_dmrs=0, n_prb_slot1=None, rv=0, new_data=True, ack_len=0, I_offset_ack=0, ri_len=0, I_offset_ri=0,
             cqi_len=0, I_offset_cqi=0):
        return cls(sf, rnti, L_prb, n_prb, n_prb if n_prb_slot1 is None else n_prb_slot1, n_dmrs, mod, tbs, rv, 1 if new_data else 0, ack_len, I_offset_ack,
                   ri_len, I_offset_ri, cqi_len, I_offset_cqi)


class UlTxCfg(C.Structure):
    C_TYPE = "srslte_hip_ul_tx_cfg_t"
    _fields_ = [("cell_id", C.c_uint32), ("nof_prb", C.c_uint32), ("rnti", C.c_uint16), ("mod", C.c_int), ("tbs", C.c_uint32), ("L_prb", C.c_uint32),
                ("n_prb", C.c_uint32), ("n_dmrs", C.c_uint32), ("max_batch", C.c_uint32), ("dmrs_cfg", DmrsPuschCfg), ("shortened", C.c_int),
                ("ack_len", C.c_uint32), ("I_offset_ack", C.c_uint32), ("ri_len", C.c_uint32), ("I_offset_ri", C.c_uint32),
                ("cqi_len", C.c_uint32), ("I_offset_cqi", C.c_uint32), ("hopping", C.c_uint32), ("n_prb_slot1", C.c_uint32), ("max_grants", C.c_uint32),
                ("cp_ext", C.c_int)]


class DlTxCfg(C.Structure):
    C_TYPE = "srslte_hip_dl_tx_cfg_t"
    _fields_ = [("cell_id", C.c_uint32), ("nof_prb", C.c_uint32), ("cfi", C.c_uint32), ("rnti", C.c_uint16), ("mod", C.c_int), ("tbs", C.c_uint32),
                ("max_batch", C.c_uint32), ("nof_ports", C.c_uint32), ("p_a", C.c_float), ("max_grants", C.c_uint32), ("cp_ext", C.c_int),
                ("tdd", C.c_int), ("tdd_sf_config", C.c_uint32), ("tdd_ss_config", C.c_uint32),
                ("mbsfn", C.c_int), ("mbsfn_area_id", C.c_uint32), ("non_mbsfn_region", C.c_uint32)]


class DlTxGrant(C.Structure):
    """srslte_hip_dl_tx_grant_t: the subframe of the batch and the grant as the receive side takes it (DlGrant)."""
    C_TYPE = "srslte_hip_dl_tx_grant_t"
    _fields_ = [("sf", C.c_uint32), ("grant", DlGrant)]


class DlTxGrant2(C.Structure):
    """srslte_hip_dl_tx_grant2_t: the subframe of the batch and the grant as the receive side takes it (DlGrant2)."""
    C_TYPE = "srslte_hip_dl_tx_grant2_t"
    _fields_ = [("sf", C.c_uint32), ("grant", DlGrant2)]


_RX_BATCH = [vp, vp, u32, u32, vp, u32, vp, vp]
_RX_HARQ = [vp, vp, u32, u32, u32, cint, vp, u32, vp, vp]
_DL_RX_GRANTS = [vp, vp, u32, u32, vp, vp, u32, vp, vp]
_DL_TX_GRANTS = [vp, vp, u32, u32, u32, vp, u32, vp, vp]

SIGNATURES = {
    # PDSCH receive pipeline
    "srslte_hip_dl_rx_create": (vp, [P(DlRxCfg)]),
    "srslte_hip_dl_rx_destroy": (void, [vp]),
    "srslte_hip_dl_rx_set_iq_format": (None, [vp, cint, f32]),
    "srslte_hip_dl_rx_nof_re": (u32, [vp, u32]),
    "srslte_hip_dl_rx_batch": (None, _RX_BATCH),
    "srslte_hip_dl_rx_batch_harq": (None, _RX_HARQ),
    "srslte_hip_dl_rx_batch_harq2": (None, [vp, vp, u32, u32, vp, vp, vp, u32, vp, vp]),
    "srslte_hip_dl_rx_grid_batch": (None, _RX_BATCH),
    "srslte_hip_dl_rx_batch_grants": (None, _DL_RX_GRANTS),
    "srslte_hip_dl_rx_batch_grants2": (None, _DL_RX_GRANTS),
    "srslte_hip_dl_rx_grid_batch_grants2": (None, _DL_RX_GRANTS),
    "srslte_hip_dl_rx_pool_create": (vp, [vp, u32]),
    "srslte_hip_dl_rx_pool_destroy": (void, [vp]),
    "srslte_hip_dl_rx_pool_submit": (i64, [vp, vp, u32, u32, vp, vp, u32, vp, vp]),
    "srslte_hip_dl_rx_pool_wait": (None, [vp, i64]),
    "srslte_hip_dl_rx_pool_set_iq_format": (None, [vp, cint, f32]),
    "srslte_hip_dl_rx_pool_submit_host": (i64, [vp, vp, u32, u32, vp, vp, u32, vp, vp]),
    "srslte_hip_dl_rx_stage": (None, [vp, cint, vp, u32, u32, vp, u32, vp, vp]),
    "srslte_hip_dl_rx_debug_buffer": (vp, [vp, cint]),
    "srslte_hip_dl_rx_keep_symbols": (None, [vp, cint]),
    "srslte_hip_dl_rx_parity_compact": (None, [vp]),
    "srslte_hip_rm_parity_compact_limit": (u32, [u32]),
    # PUSCH receive pipeline
    "srslte_hip_ul_rx_create": (vp, [P(UlRxCfg)]),
    "srslte_hip_ul_rx_destroy": (void, [vp]),
    "srslte_hip_ul_rx_set_iq_format": (None, [vp, cint, f32]),
    "srslte_hip_ul_rx_batch": (None, _RX_BATCH),
    "srslte_hip_ul_rx_batch_harq": (None, _RX_HARQ),
    "srslte_hip_ul_rx_batch_grants": (None, [vp, vp, u32, u32, vp, u32, vp, u32, vp, vp]),
    "srslte_hip_ul_rx_grants_ack": (vp, [vp]),
    "srslte_hip_ul_rx_grants_ri": (vp, [vp]),
    "srslte_hip_ul_rx_grants_cqi": (vp, [vp]),
    "srslte_hip_ul_rx_ack": (vp, [vp]),
    "srslte_hip_ul_rx_ri": (vp, [vp]),
    "srslte_hip_ul_rx_cqi": (vp, [vp]),
    "srslte_hip_ul_rx_debug_buffer": (vp, [vp, cint]),
    # PUSCH transmit pipeline
    "srslte_hip_ul_tx_create": (vp, [P(UlTxCfg)]),
    "srslte_hip_ul_tx_destroy": (void, [vp]),
    "srslte_hip_ul_tx_set_iq_format": (None, [vp, cint, f32]),
    "srslte_hip_ul_tx_batch": (None, [vp, vp, u32, u32, u32, vp, vp]),
    "srslte_hip_ul_tx_batch_ack": (None, [vp, vp, u32, vp, u32, u32, vp, vp]),
    "srslte_hip_ul_tx_batch_uci": (None, [vp, vp, u32, vp, vp, u32, u32, vp, vp]),
    "srslte_hip_ul_tx_batch_uci_cqi": (None, [vp, vp, u32, vp, vp, vp, u32, u32, vp, vp]),
    "srslte_hip_ul_tx_batch_rv": (None, [vp, vp, u32, vp, vp, vp, u32, u32, u32, vp, vp]),
    "srslte_hip_ul_tx_batch_grants": (None, [vp, vp, u32, vp, vp, vp, u32, u32, vp, u32, vp, vp]),
    "srslte_hip_ul_tx_debug_buffer": (vp, [vp, cint]),
    # PDSCH transmit pipeline
    "srslte_hip_dl_tx_create": (vp, [P(DlTxCfg)]),
    "srslte_hip_dl_tx_destroy": (void, [vp]),
    "srslte_hip_dl_tx_set_iq_format": (None, [vp, cint, f32]),
    "srslte_hip_dl_tx_batch": (None, [vp, vp, u32, u32, u32, u32, vp, vp]),
    "srslte_hip_dl_tx_batch_grants": (None, _DL_TX_GRANTS),
    "srslte_hip_dl_tx_batch_grants2": (None, _DL_TX_GRANTS),
    "srslte_hip_dl_tx_debug_buffer": (vp, [vp, cint]),
}


class Pipeline(Handle):
    """A pipeline object: a handle with debug buffers, read through the C function DEBUG names, and the sample format of its time-domain side
    (phy_hip.h, "Sample formats"), set through the C function IQ_FORMAT names."""

    DEBUG = IQ_FORMAT = None
    iq_format = IQ_CF32

    def debug(self, which, dtype, count):
        return host_copy(getattr(lib(), self.DEBUG)(self.h, which), dtype, count)

    def set_iq_format(self, fmt, scale=1.0):
        """IQ_SC16: the object's time samples are int16 pairs, arrays [...][sf_len][2] (I, Q) where they were complex [...][sf_len]; scale as
        srslte_vec_convert_if / _fi take it. Returns the status code; a refused call leaves the object as it was."""
        rc = getattr(lib(), self.IQ_FORMAT)(self.h, fmt, scale)
        if rc == SRSLTE_SUCCESS:
            self.iq_format = fmt
        return rc

    def _iq_in(self, iq, width):
        """The caller's time samples as [nof_sf][width] rows of the object's format (int16: 2 * width values per row)."""
        if self.iq_format == IQ_SC16:
            return np.ascontiguousarray(iq, np.int16).reshape(-1, 2 * width)
        return np.ascontiguousarray(iq, np.complex64).reshape(-1, width)

    def _iq_out(self, *shape):
        """self.d_iq as an array of that shape in the object's format (int16: a last axis of 2)."""
        if self.iq_format == IQ_SC16:
            return self.d_iq.to_host(np.int16, 2 * int(np.prod(shape))).reshape(shape + (2,))
        return self.d_iq.to_host(np.complex64).reshape(shape)


def _tb_rows(d_tb, d_ok, stride, n, nbytes=None):
    """The first n rows of a transport-block buffer of row length stride, cut to nbytes, and of its CRC flags: (tb [n][nbytes], ok [n])."""
    return d_tb.to_host(np.uint8).reshape(-1, stride)[:n, :nbytes], d_ok.to_host(np.uint8)[:n]


def _tb_rows2(d_tb, d_ok, stride, n, nbytes=(None, None)):
    """Two transport blocks per subframe, rows b and n + b: ([tb0 [n][nbytes[0]], tb1 [n][nbytes[1]]], [ok0 [n], ok1 [n]])."""
    tb, ok = _tb_rows(d_tb, d_ok, stride, 2 * n)
    return [tb[:n, :nbytes[0]], tb[n:, :nbytes[1]]], [ok[:n], ok[n:]]


class DlRx(Pipeline):
    """Batched PDSCH receive chain (ue_dl.c:369-384 + pdsch.c:833-997 + sch.c:507-532 for one codeword)."""
    DESTROY, DEBUG, IQ_FORMAT = "srslte_hip_dl_rx_destroy", "srslte_hip_dl_rx_debug_buffer", "srslte_hip_dl_rx_set_iq_format"

    def __init__(self, cell_id, nof_prb, cfi, rnti, mod, tbs, max_iterations, max_batch, mmse=True, chest_cfg=None, llr_8bit=False, nof_rx=1,
                 nof_ports=1, csi=False, power_scale=False, p_a=0.0, out_ptrs=None, tx_scheme=0, pmi=0, mod2=0, tbs2=0, cp_ext=False, tdd=None,
                 mbsfn=None):
        """mbsfn = (area id, non-MBSFN region length): a PMCH pipeline (MBSFN subframes; rnti unused).
        tx_scheme 3 (large-delay CDD) / 2 (closed-loop multiplexing) with pmi, and mod2 / tbs2 for a second transport block: the two-layer
        modes; decode() then returns lists [transport block 0, transport block 1] of tb and ok arrays."""
        self.cfg = DlRxCfg(cell_id, nof_prb, cfi, rnti, mod, tbs, max_iterations, max_batch, 1 if mmse else 0, chest_cfg or ChestDlCfg(),
                           1 if llr_8bit else 0, nof_rx, nof_ports, 1 if csi else 0, 1 if power_scale else 0, p_a, tx_scheme, pmi, mod2, tbs2, 1 if cp_ext else 0,
                           1 if tdd else 0, tdd[0] if tdd else 0, tdd[1] if tdd else 0, 1 if mbsfn else 0, mbsfn[0] if mbsfn else 0, mbsfn[1] if mbsfn else 0)
        self.nof_rx = nof_rx
        self._create("srslte_hip_dl_rx_create", C.byref(self.cfg))
        self.tbs, self.max_batch, self.tbs2 = tbs, max_batch, tbs2
        self.tb_stride = (max(tbs, tbs2) // 8 + 6 + 15) & ~15
        self.sf_len = 15 * symbol_sz(nof_prb)
        if out_ptrs is None:
            self.d_tb, self.d_ok = DevBuf(self.tb_stride * max_batch * (2 if tbs2 else 1)), DevBuf(max_batch * (2 if tbs2 else 1))
        else:  # caller-owned device memory (e.g. a torch tensor that a collective reads): (tb pointer, ok pointer)
            self.d_tb, self.d_ok = DevView(out_ptrs[0], self.tb_stride * max_batch), DevView(out_ptrs[1], max_batch)
        # per-subframe stride of the LLR buffer e (debug buffer 4)
        self.e_stride = (max(self.nof_re(s) for s in (0, 1, 5)) * {1: 2, 2: 4, 3: 6, 4: 8}[mod] + 15) & ~15

    def nof_re(self, sf_idx):
        return lib().srslte_hip_dl_rx_nof_re(self.h, sf_idx)

    def keep_symbols(self, enable=True):
        """Also write the equalised symbols d (debug buffer 3); off by default: the fused kernel never stores them."""
        _check(lib().srslte_hip_dl_rx_keep_symbols(self.h, 1 if enable else 0), "dl_rx_keep_symbols")

    def parity_compact(self):
        """Whether the last rate de-matcher run wrote the soft buffer with its parity streams at a quarter of their rows."""
        return bool(lib().srslte_hip_dl_rx_parity_compact(self.h))

    def run_device(self, d_iq_ptr, tti0, nof_sf, stream=None):
        return lib().srslte_hip_dl_rx_batch(self.h, d_iq_ptr, tti0, nof_sf, self.d_tb.ptr, self.tb_stride, self.d_ok.ptr, stream)

    def stage(self, stage, d_iq_ptr, tti0, nof_sf, stream=None):
        return lib().srslte_hip_dl_rx_stage(self.h, stage, d_iq_ptr, tti0, nof_sf, self.d_tb.ptr, self.tb_stride, self.d_ok.ptr, stream)

    def _rows(self, n):
        return _tb_rows(self.d_tb, self.d_ok, self.tb_stride, n, self.tbs // 8 + 3)

    def _rows2(self, n):
        return _tb_rows2(self.d_tb, self.d_ok, self.tb_stride, n, (self.tbs // 8 + 3, self.tbs2 // 8 + 3))

    def decode(self, iq, tti0=0):
        x = self._iq_in(iq, self.nof_rx * self.sf_len)  # [nsf][nof_rx][sf_len]
        din = DevBuf.from_host(x)
        _check(self.run_device(din.ptr, tti0, x.shape[0]), "dl_rx_batch")
        sync()
        return self._rows2(x.shape[0]) if self.tbs2 else self._rows(x.shape[0])

    def decode_harq2(self, iq, tti0, rv, new_data):
        """srslte_hip_dl_rx_batch_harq2: rv / new_data per transport block (two-layer modes)."""
        x = self._iq_in(iq, self.nof_rx * self.sf_len)
        din = DevBuf.from_host(x)
        n = x.shape[0]
        _check(lib().srslte_hip_dl_rx_batch_harq2(self.h, din.ptr, tti0, n, (C.c_uint32 * 2)(*rv), (C.c_int * 2)(*[1 if v else 0 for v in new_data]),
                                                  self.d_tb.ptr, self.tb_stride, self.d_ok.ptr, None), "dl_rx_batch_harq2")
        sync()
        return self._rows2(n)

    def decode_grants(self, iq, tti0, grants):
        """srslte_hip_dl_rx_batch_grants: subframe b with grants[b] (DlGrant). Returns (rc, tb [nsf][tbs_max/8+3], ok [nsf])."""
        x = self._iq_in(iq, self.nof_rx * self.sf_len)
        assert len(grants) == x.shape[0]
        arr = (DlGrant * len(grants))(*grants)
        din = DevBuf.from_host(x)
        rc = lib().srslte_hip_dl_rx_batch_grants(self.h, din.ptr, tti0, x.shape[0], arr, self.d_tb.ptr, self.tb_stride, self.d_ok.ptr, None)
        if rc != SRSLTE_SUCCESS:
            return rc, None, None
        sync()
        return (rc,) + self._rows(x.shape[0])

    def decode_grants2(self, iq, tti0, grants, from_grid=False):
        """srslte_hip_dl_rx_batch_grants2: subframe b with grants[b] (DlGrant2: scheme, pmi and a second transport block per subframe).
        Returns (rc, [tb0 rows, tb1 rows], [ok0, ok1]); on a cell without two-layer grants the second entries are None.
        from_grid: iq holds frequency-domain grids [nsf][nof_rx][14 * 12 * nof_prb] (srslte_hip_dl_rx_grid_batch_grants2)."""
        if from_grid:
            x = np.ascontiguousarray(iq, np.complex64).reshape(-1, self.nof_rx * 14 * 12 * self.cfg.nof_prb)
        else:
            x = self._iq_in(iq, self.nof_rx * self.sf_len)
        n = x.shape[0]
        assert len(grants) == n
        arr = (DlGrant2 * n)(*grants)
        din, dtb, dok = DevBuf.from_host(x), DevBuf(self.tb_stride * n * 2), DevBuf(2 * n)
        fn = lib().srslte_hip_dl_rx_grid_batch_grants2 if from_grid else lib().srslte_hip_dl_rx_batch_grants2
        rc = fn(self.h, din.ptr, tti0, n, arr, dtb.ptr, self.tb_stride, dok.ptr, None)
        if rc != SRSLTE_SUCCESS:
            return rc, None, None
        sync()
        tb, ok = _tb_rows2(dtb, dok, self.tb_stride, n)
        if not (self.cfg.nof_ports == 2 and self.cfg.nof_rx_antennas == 2):
            tb[1] = ok[1] = None
        return rc, tb, ok

    def decode_harq(self, iq, tti0, rv, new_data):
        """srslte_hip_dl_rx_batch_harq: slot b keeps its soft buffers / CRC flags / bytes between calls."""
        x = self._iq_in(iq, self.nof_rx * self.sf_len)
        din = DevBuf.from_host(x)
        _check(lib().srslte_hip_dl_rx_batch_harq(self.h, din.ptr, tti0, x.shape[0], rv, 1 if new_data else 0, self.d_tb.ptr, self.tb_stride,
                                                 self.d_ok.ptr, None), "dl_rx_batch_harq")
        sync()
        return self._rows(x.shape[0])

    def decode_grid(self, grid, tti0=0):
        """Frequency-domain input [nsf][14*12*nof_prb] (srslte_hip_dl_rx_grid_batch)."""
        x = np.ascontiguousarray(grid, np.complex64)
        x = x.reshape(-1, x.shape[-1])
        din = DevBuf.from_host(x)
        _check(lib().srslte_hip_dl_rx_grid_batch(self.h, din.ptr, tti0, x.shape[0], self.d_tb.ptr, self.tb_stride, self.d_ok.ptr, None), "dl_rx_grid_batch")
        sync()
        return self._rows(x.shape[0])

    def csi(self, nof_sf, snr_to_cqi_offset=None):
        """srslte_hip_dl_rx_csi_batch on the estimates of the object's last batch -> (rc, [CsiRes] or None)."""
        if snr_to_cqi_offset is not None:
            _check(lib().srslte_hip_dl_rx_set_snr_to_cqi_offset(self.h, snr_to_cqi_offset), "dl_rx_set_snr_to_cqi_offset")
        dout = DevBuf(max(1, nof_sf) * C.sizeof(CsiRes))
        return result_structs(lib().srslte_hip_dl_rx_csi_batch(self.h, nof_sf, dout.ptr, None), dout.ptr, CsiRes, nof_sf)


class DlRxPool(Handle):
    """srslte_hip_dl_rx_pool_*: `depth` receive pipelines behind one submission call; cfg: a DlRxCfg (e.g. DlRx(...).cfg). Pointers are the
    caller's: device d_iq / d_tb / d_tb_ok, pinned host h_iq / h_record. submit calls return the ticket, or the negative status code."""
    DESTROY = "srslte_hip_dl_rx_pool_destroy"

    def __init__(self, cfg, depth):
        self._create("srslte_hip_dl_rx_pool_create", C.byref(cfg), depth)

    def set_iq_format(self, fmt, scale=1.0):
        return lib().srslte_hip_dl_rx_pool_set_iq_format(self.h, fmt, scale)

    def submit(self, d_iq, tti0, nof_sf, d_tb, tb_stride, d_tb_ok, grants=None, h_record=None):
        arr = (DlGrant * len(grants))(*grants) if grants else None
        return lib().srslte_hip_dl_rx_pool_submit(self.h, d_iq, tti0, nof_sf, arr, d_tb, tb_stride, d_tb_ok, h_record)

    def submit_host(self, h_iq, tti0, nof_sf, d_tb, tb_stride, d_tb_ok, grants=None, h_record=None):
        arr = (DlGrant * len(grants))(*grants) if grants else None
        return lib().srslte_hip_dl_rx_pool_submit_host(self.h, h_iq, tti0, nof_sf, arr, d_tb, tb_stride, d_tb_ok, h_record)

    def wait(self, ticket):
        return lib().srslte_hip_dl_rx_pool_wait(self.h, ticket)


class UlRx(Pipeline):
    """Batched PUSCH receive chain (enb_ul.c + pusch.c:423-520 + the UL-SCH part of sch.c:991-1066)."""
    DESTROY, DEBUG, IQ_FORMAT = "srslte_hip_ul_rx_destroy", "srslte_hip_ul_rx_debug_buffer", "srslte_hip_ul_rx_set_iq_format"

    def __init__(self, cell_id, nof_prb, rnti, mod, tbs, L_prb, n_prb, n_dmrs, max_iterations, max_batch, cyclic_shift=0, delta_ss=0,
                 group_hopping=False, sequence_hopping=False, mmse=True, shortened=False, ack_len=0, I_offset_ack=0, ri_len=0, I_offset_ri=0,
                 cqi_len=0, I_offset_cqi=0, n_prb_slot1=None, max_grants=0, cp_ext=False):
        self.cfg = UlRxCfg(cell_id, nof_prb, rnti, mod, tbs, L_prb, n_prb, n_dmrs, max_iterations, max_batch, 1 if mmse else 0,
                           DmrsPuschCfg(cyclic_shift, delta_ss, 1 if group_hopping else 0, 1 if sequence_hopping else 0), 1 if shortened else 0,
                           ack_len, I_offset_ack, ri_len, I_offset_ri, cqi_len, I_offset_cqi, 0 if n_prb_slot1 is None else 1, n_prb_slot1 or 0,
                           max_grants, 1 if cp_ext else 0)
        self._create("srslte_hip_ul_rx_create", C.byref(self.cfg))
        self.tbs, self.max_batch = tbs, max_batch
        self.tb_stride = (tbs // 8 + 6 + 15) & ~15
        self.sf_len = 15 * symbol_sz(nof_prb)
        self.rows = max(max_batch, max_grants)
        self.rows_grants = max_grants or max_batch
        self.d_tb, self.d_ok = DevBuf(self.tb_stride * self.rows), DevBuf(self.rows)

    def _rows(self, n, nbytes=None):
        return _tb_rows(self.d_tb, self.d_ok, self.tb_stride, n, nbytes)

    def decode_grants(self, iq, tti0, grants):
        """srslte_hip_ul_rx_batch_grants: grants = list of UlGrant; row p of the result belongs to grants[p]."""
        x = self._iq_in(iq, self.sf_len)
        din = DevBuf.from_host(x)
        arr = (UlGrant * len(grants))(*grants)
        _check(lib().srslte_hip_ul_rx_batch_grants(self.h, din.ptr, tti0, x.shape[0], arr, len(grants), self.d_tb.ptr, self.tb_stride, self.d_ok.ptr, None),
               "ul_rx_batch_grants")
        sync()
        self.last_nof_grants = len(grants)
        return self._rows(len(grants))

    def decode_grants_pucch(self, iq, tti0, grants, ctrl, reqs):
        """srslte_hip_ul_rx_batch_grants_pucch: (rc, tb, tb_ok, [PucchRes]); grants may be empty."""
        x = self._iq_in(iq, self.sf_len)
        din = DevBuf.from_host(x)
        dres = DevBuf(C.sizeof(PucchRes) * max(1, len(reqs)))
        rc = lib().srslte_hip_ul_rx_batch_grants_pucch(self.h, din.ptr, tti0, x.shape[0], struct_array(UlGrant, grants), len(grants), self.d_tb.ptr,
                                                       self.tb_stride, self.d_ok.ptr, ctrl.h, struct_array(PucchReq, reqs), len(reqs), dres.ptr, None)
        if rc != SRSLTE_SUCCESS:
            return rc, None, None, None
        sync()
        self.last_nof_grants = len(grants)
        return (rc,) + self._rows(len(grants)) + (read_structs(dres.ptr, PucchRes, len(reqs)),)

    def decode_grants_pucch_srs(self, iq, tti0, grants, ctrl, reqs, srs, ues):
        """srslte_hip_ul_rx_batch_grants_pucch_srs: (rc, tb, tb_ok, [PucchRes], [SrsRes], ce); ctrl and srs may each be None."""
        x = self._iq_in(iq, self.sf_len)
        din = DevBuf.from_host(x)
        dres = DevBuf(C.sizeof(PucchRes) * max(1, len(reqs)))
        dsr, dsc = DevBuf(C.sizeof(SrsRes) * max(1, len(ues))), DevBuf(8 * SRS_MAX_CE * max(1, len(ues)))
        rc = lib().srslte_hip_ul_rx_batch_grants_pucch_srs(self.h, din.ptr, tti0, x.shape[0], struct_array(UlGrant, grants), len(grants), self.d_tb.ptr,
                                                           self.tb_stride, self.d_ok.ptr, ctrl.h if ctrl is not None else None,
                                                           struct_array(PucchReq, reqs), len(reqs), dres.ptr, srs.h if srs is not None else None,
                                                           struct_array(SrsUe, ues), len(ues), dsr.ptr, dsc.ptr, None)
        if rc != SRSLTE_SUCCESS:
            return rc, None, None, None, None, None
        sync()
        self.last_nof_grants = len(grants)
        return (rc,) + self._rows(len(grants)) + (read_structs(dres.ptr, PucchRes, len(reqs)),) + Srs.read(dsr, dsc, len(ues))

    def grants_uci(self):
        """(HARQ-ACK decisions [nof_grants][2], rank indications [nof_grants][2]) of the last decode_grants()."""
        return [host_copy(fn(self.h), np.uint8, 2 * self.last_nof_grants).reshape(-1, 2)
                for fn in (lib().srslte_hip_ul_rx_grants_ack, lib().srslte_hip_ul_rx_grants_ri)]

    def grants_cqi(self):
        """(report bits [nof_grants][64], CRC flags [nof_grants]) of the last decode_grants()."""
        out = host_copy(lib().srslte_hip_ul_rx_grants_cqi(self.h), np.uint8, 65 * self.rows_grants)
        n = self.last_nof_grants
        return out[:64 * self.rows_grants].reshape(-1, 64)[:n], out[64 * self.rows_grants:][:n]

    def decode(self, iq, tti0=0):
        x = self._iq_in(iq, self.sf_len)
        din = DevBuf.from_host(x)
        _check(lib().srslte_hip_ul_rx_batch(self.h, din.ptr, tti0, x.shape[0], self.d_tb.ptr, self.tb_stride, self.d_ok.ptr, None), "ul_rx_batch")
        sync()
        self.last_nof_sf = x.shape[0]
        return self._rows(x.shape[0], self.tbs // 8 + 3)

    def decode_harq(self, iq, tti0, rv, new_data):
        """srslte_hip_ul_rx_batch_harq: slot b keeps its soft buffers between calls; new_data starts new transport blocks."""
        x = self._iq_in(iq, self.sf_len)
        din = DevBuf.from_host(x)
        _check(lib().srslte_hip_ul_rx_batch_harq(self.h, din.ptr, tti0, x.shape[0], rv, 1 if new_data else 0, self.d_tb.ptr, self.tb_stride,
                                                 self.d_ok.ptr, None), "ul_rx_batch_harq")
        sync()
        self.last_nof_sf = x.shape[0]
        return self._rows(x.shape[0], self.tbs // 8 + 3)

    def ack(self):
        """HARQ-ACK decisions [nof_sf][2] of the last decode() (srslte_uci_value_t.ack.ack_value of srslte_pusch_decode)."""
        out = host_copy(lib().srslte_hip_ul_rx_ack(self.h), np.uint8, 2 * self.max_batch)
        return out.reshape(-1, 2)[:self.last_nof_sf, :max(self.cfg.ack_len, 1)]

    def ri(self):
        """Rank-indication decisions [nof_sf][ri_len] of the last decode() (srslte_uci_value_t.ri)."""
        out = host_copy(lib().srslte_hip_ul_rx_ri(self.h), np.uint8, 2 * self.max_batch)
        return out.reshape(-1, 2)[:self.last_nof_sf, :max(self.cfg.ri_len, 1)]

    def cqi(self):
        """CQI reports of the last decode(): bits [nof_sf][cqi_len] and the CRC flags [nof_sf] (srslte_uci_value_t.cqi, .cqi.data_crc)."""
        out = host_copy(lib().srslte_hip_ul_rx_cqi(self.h), np.uint8, 65 * self.max_batch)
        n = self.last_nof_sf
        return out[:64 * self.max_batch].reshape(-1, 64)[:n, :self.cfg.cqi_len], out[64 * self.max_batch:][:n]


def _uci_rows(v, n, w, length=None):
    """UCI values v (one row per block: [n][length] values, or ragged rows when length is None) -> a device [n][w] uint8 array; None for None."""
    if v is None:
        return None
    a = np.zeros((n, w), np.uint8)
    if length is None:
        for p_, row in enumerate(v):
            a[p_, :len(row)] = row
    else:
        a[:, :length] = np.asarray(v, np.uint8).reshape(n, -1)[:, :length]
    return DevBuf.from_host(a)


def _ptr(buf):
    return buf.ptr if buf else None


def _tb_upload(tbs_bytes, n, stride):
    """Payloads tbs_bytes[p] -> a device [max(n, 1)][stride] uint8 array, row p zero-padded."""
    x = np.zeros((max(n, 1), stride), np.uint8)
    for p_, b in enumerate(tbs_bytes):
        x[p_, :len(b)] = b
    return DevBuf.from_host(x)


class UlTx(Pipeline):
    """Batched PUSCH transmit chain (srslte_ue_ul_encode ue_ul.c:300-340: srslte_pusch_encode pusch.c:314-421 with the UL-SCH part of
    srslte_ulsch_encode sch.c:1068-1160, DMRS, srslte_ofdm_tx_sf with ue_ul.c:59-64 settings)."""
    DESTROY, DEBUG, IQ_FORMAT = "srslte_hip_ul_tx_destroy", "srslte_hip_ul_tx_debug_buffer", "srslte_hip_ul_tx_set_iq_format"

    def __init__(self, cell_id, nof_prb, rnti, mod, tbs, L_prb, n_prb, n_dmrs, max_batch, cyclic_shift=0, delta_ss=0, group_hopping=False,
                 sequence_hopping=False, shortened=False, ack_len=0, I_offset_ack=0, ri_len=0, I_offset_ri=0, cqi_len=0, I_offset_cqi=0,
                 n_prb_slot1=None, max_grants=0, cp_ext=False):
        self.cfg = UlTxCfg(cell_id, nof_prb, rnti, mod, tbs, L_prb, n_prb, n_dmrs, max_batch,
                           DmrsPuschCfg(cyclic_shift, delta_ss, 1 if group_hopping else 0, 1 if sequence_hopping else 0), 1 if shortened else 0,
                           ack_len, I_offset_ack, ri_len, I_offset_ri, cqi_len, I_offset_cqi, 0 if n_prb_slot1 is None else 1, n_prb_slot1 or 0,
                           max_grants, 1 if cp_ext else 0)
        self._create("srslte_hip_ul_tx_create", C.byref(self.cfg))
        self.tbs, self.max_batch = tbs, max_batch
        self.sf_len = 15 * symbol_sz(nof_prb)
        self.d_iq = DevBuf(8 * self.sf_len * max_batch)

    def encode_grants(self, tbs_bytes, tti0, nof_sf, grants, ack=None, ri=None, cqi=None):
        """srslte_hip_ul_tx_batch_grants: grants = list of UlGrant, tbs_bytes[p] the payload of grants[p]; ack / ri: [nof_grants][<= 2] values,
        cqi: [nof_grants][<= 64] report bits (rows of grants without that UCI are ignored) -> iq [nof_sf][sf_len]."""
        n = len(grants)
        stride = (self.tbs // 8 + 15) & ~15
        din = _tb_upload(tbs_bytes, n, stride)
        bufs = [_uci_rows(v, max(n, 1), w) for v, w in ((ack, 2), (ri, 2), (cqi, 64))]
        _check(lib().srslte_hip_ul_tx_batch_grants(self.h, din.ptr, stride, *[_ptr(b) for b in bufs], tti0, nof_sf, struct_array(UlGrant, grants), n,
                                                   self.d_iq.ptr, None), "ul_tx_batch_grants")
        sync()
        return self._iq_out(self.max_batch, self.sf_len)[:nof_sf]

    def encode(self, tb, tti0=0, ack=None, ri=None, cqi=None, rv=None):
        """tb: [nof_sf][tbs/8] payload bytes (ack: [nof_sf][ack_len] HARQ-ACK values, ri: [nof_sf][ri_len] rank-indication bits,
        cqi: [nof_sf][cqi_len] report bits; rv: redundancy version through srslte_hip_ul_tx_batch_rv) -> iq [nof_sf][sf_len] (left on the
        device in self.d_iq). tbs = 0 (a PUSCH without UL-SCH data): tb is ignored, one subframe per row of cqi."""
        if self.tbs == 0:
            x = np.zeros((len(cqi), 1), np.uint8)
        else:
            x = np.ascontiguousarray(tb, np.uint8).reshape(-1, self.tbs // 8)
        din, n, L = DevBuf.from_host(x), x.shape[0], lib()
        dack, dri, dcqi = (_uci_rows(v, n, w, length) for v, w, length in ((ack, 2, self.cfg.ack_len), (ri, 2, self.cfg.ri_len), (cqi, 64, self.cfg.cqi_len)))
        head, tail = (self.h, din.ptr, self.tbs // 8), (tti0, n, self.d_iq.ptr, None)
        if rv is not None:
            _check(L.srslte_hip_ul_tx_batch_rv(*head, _ptr(dack), _ptr(dri), _ptr(dcqi), rv, *tail), "ul_tx_batch_rv")
        elif cqi is not None:
            _check(L.srslte_hip_ul_tx_batch_uci_cqi(*head, _ptr(dack), _ptr(dri), dcqi.ptr, *tail), "ul_tx_batch_uci_cqi")
        elif ri is not None:
            _check(L.srslte_hip_ul_tx_batch_uci(*head, _ptr(dack), dri.ptr, *tail), "ul_tx_batch_uci")
        elif ack is not None:
            _check(L.srslte_hip_ul_tx_batch_ack(*head, dack.ptr, *tail), "ul_tx_batch_ack")
        else:
            _check(L.srslte_hip_ul_tx_batch(*head, *tail), "ul_tx_batch")
        sync()
        return self._iq_out(self.max_batch, self.sf_len)[:n]


class DlTx(Pipeline):
    """Batched PDSCH transmit chain (srslte_pdsch_encode pdsch.c:1059-1185 + CRS + srslte_ofdm_tx_sf, enb_dl.c)."""
    DESTROY, DEBUG, IQ_FORMAT = "srslte_hip_dl_tx_destroy", "srslte_hip_dl_tx_debug_buffer", "srslte_hip_dl_tx_set_iq_format"

    def __init__(self, cell_id, nof_prb, cfi, rnti, mod, tbs, max_batch, nof_ports=1, p_a=0.0, max_grants=0, cp_ext=False, tdd=None, mbsfn=None):
        self.cfg = DlTxCfg(cell_id, nof_prb, cfi, rnti, mod, tbs, max_batch, nof_ports, p_a, max_grants, 1 if cp_ext else 0,
                           1 if tdd else 0, tdd[0] if tdd else 0, tdd[1] if tdd else 0, 1 if mbsfn else 0, mbsfn[0] if mbsfn else 0, mbsfn[1] if mbsfn else 0)
        self._create("srslte_hip_dl_tx_create", C.byref(self.cfg))
        self.tbs, self.max_batch, self.nof_ports = tbs, max_batch, max(1, nof_ports)
        self.sf_len = 15 * symbol_sz(nof_prb)
        self.d_iq = DevBuf(8 * self.sf_len * max_batch * self.nof_ports)

    def _iq(self, nof_sf):
        return self._iq_out(self.max_batch, self.nof_ports, self.sf_len)[:nof_sf]

    def _result(self, rc, nof_sf):
        if rc != SRSLTE_SUCCESS:
            return rc, None
        sync()
        return rc, self._iq(nof_sf)

    def encode_grants(self, tbs_bytes, tti0, nof_sf, grants):
        """srslte_hip_dl_tx_batch_grants: grants = list of (sf, DlGrant); tbs_bytes[p] = the payload of grants[p] -> iq [nof_sf][nof_ports][sf_len]."""
        stride = (self.tbs // 8 + 15) & ~15
        din = _tb_upload(tbs_bytes, len(grants), stride)
        arr = struct_array(DlTxGrant, [DlTxGrant(sf, g) for sf, g in grants])
        _check(lib().srslte_hip_dl_tx_batch_grants(self.h, din.ptr, stride, tti0, nof_sf, arr, len(grants), self.d_iq.ptr, None), "dl_tx_batch_grants")
        sync()
        return self._iq(nof_sf)

    def encode(self, tb, tti0=0, rv=0):
        """tb: [nof_sf][tbs/8] payload bytes -> iq [nof_sf][nof_ports][sf_len]."""
        x = np.ascontiguousarray(tb, np.uint8).reshape(-1, self.tbs // 8)
        din = DevBuf.from_host(x)
        _check(lib().srslte_hip_dl_tx_batch(self.h, din.ptr, self.tbs // 8, tti0, x.shape[0], rv, self.d_iq.ptr, None), "dl_tx_batch")
        sync()
        return self._iq(x.shape[0])

    def encode_grants_ctrl(self, tbs_bytes, tti0, nof_sf, grants, ctrl, cfi, dcis=(), phichs=()):
        """srslte_hip_dl_tx_batch_grants_ctrl: encode_grants with the control region of ctrl (a DlCtrlTx of the same cell) - cfi [nof_sf], dcis and
        phichs as DlCtrlTx.put takes them - on the grids before the OFDM modulation -> (rc, iq [nof_sf][nof_ports][sf_len] or None)."""
        return self._encode_grants_with(lib().srslte_hip_dl_tx_batch_grants_ctrl, tbs_bytes, tti0, nof_sf, grants, ctrl, cfi, dcis, phichs)

    def encode_grants_full(self, tbs_bytes, tti0, nof_sf, grants, ctrl, cfi, dcis=(), phichs=()):
        """srslte_hip_dl_tx_batch_grants_full: encode_grants_ctrl with ctrl's PSS / SSS / PBCH put before the PDSCHs, a complete FDD subframe per
        TTI -> (rc, iq [nof_sf][nof_ports][sf_len] or None)."""
        return self._encode_grants_with(lib().srslte_hip_dl_tx_batch_grants_full, tbs_bytes, tti0, nof_sf, grants, ctrl, cfi, dcis, phichs)

    def _encode_grants_with(self, fn, tbs_bytes, tti0, nof_sf, grants, ctrl, cfi, dcis, phichs):
        stride = (self.tbs // 8 + 15) & ~15
        din = _tb_upload(tbs_bytes, len(grants), stride)
        arr = struct_array(DlTxGrant, [DlTxGrant(sf, g) for sf, g in grants])
        inp, keep = _ctrl_tx_in(cfi, dcis, phichs)
        return self._result(fn(self.h, din.ptr, stride, tti0, nof_sf, arr, len(grants), ctrl.h, C.byref(inp), self.d_iq.ptr, None), nof_sf)

    def _tb_rows2(self, tbs_bytes, n):
        """[2 n][stride] device rows: row p = the first payload of entry p, row n + p its second (entries: lists of one or two payloads)."""
        stride = (self.tbs // 8 + 15) & ~15
        x = np.zeros((max(1, 2 * n), stride), np.uint8)
        for p_, tbs_ in enumerate(tbs_bytes):
            for cw, b in enumerate(tbs_):
                x[cw * n + p_, :len(b)] = b
        return DevBuf.from_host(x), stride

    def encode_grants2(self, tbs_bytes, tti0, nof_sf, grants):
        """srslte_hip_dl_tx_batch_grants2: grants = list of (sf, DlGrant2); tbs_bytes[p] = [payload of block 0] or [block 0, block 1] of grants[p]
        -> (rc, iq [nof_sf][nof_ports][sf_len] or None)."""
        n = len(grants)
        din, stride = self._tb_rows2(tbs_bytes, n)
        arr = struct_array(DlTxGrant2, [DlTxGrant2(sf, g) for sf, g in grants])
        return self._result(lib().srslte_hip_dl_tx_batch_grants2(self.h, din.ptr, stride, tti0, nof_sf, arr, n, self.d_iq.ptr, None), nof_sf)

    def encode_grants2_ctrl(self, tbs_bytes, tti0, nof_sf, grants, ctrl, cfi, dcis=(), phichs=()):
        """srslte_hip_dl_tx_batch_grants2_ctrl: encode_grants2 with the control region of ctrl, as encode_grants_ctrl."""
        return self._encode_grants2_with(lib().srslte_hip_dl_tx_batch_grants2_ctrl, tbs_bytes, tti0, nof_sf, grants, ctrl, cfi, dcis, phichs)

    def encode_grants2_full(self, tbs_bytes, tti0, nof_sf, grants, ctrl, cfi, dcis=(), phichs=()):
        """srslte_hip_dl_tx_batch_grants2_full: encode_grants2_ctrl with ctrl's PSS / SSS / PBCH, as encode_grants_full."""
        return self._encode_grants2_with(lib().srslte_hip_dl_tx_batch_grants2_full, tbs_bytes, tti0, nof_sf, grants, ctrl, cfi, dcis, phichs)

    def _encode_grants2_with(self, fn, tbs_bytes, tti0, nof_sf, grants, ctrl, cfi, dcis, phichs):
        n = len(grants)
        din, stride = self._tb_rows2(tbs_bytes, n)
        arr = struct_array(DlTxGrant2, [DlTxGrant2(sf, g) for sf, g in grants])
        inp, keep = _ctrl_tx_in(cfi, dcis, phichs)
        return self._result(fn(self.h, din.ptr, stride, tti0, nof_sf, arr, n, ctrl.h, C.byref(inp), self.d_iq.ptr, None), nof_sf)
