"""The core objects: OFDM, DFT, DL / UL channel estimators, soft demapper, turbo decoder and coder, segmentation, one-block SCH coder."""
import ctypes as C

import numpy as np

from ._native import (IQ_CF32, IQ_SC16, MOD_BPSK, SRSLTE_SUCCESS, DevBuf, Handle, P, _check, cint, f32, host_copy, lib, sync, u16, u32, void, vp)


class ChestDlCfg(C.Structure):
    """srslte_chest_dl_cfg_t (chest_dl.h:116-130)."""
    C_TYPE = "srslte_hip_chest_dl_cfg_t"
    _fields_ = [("noise_alg", C.c_int), ("filter_type", C.c_int), ("filter_coef", C.c_float * 2), ("mbsfn_area_id", C.c_uint16),
                ("interpolate_subframe", C.c_uint8), ("rsrp_neighbour", C.c_uint8), ("cfo_estimate_enable", C.c_uint8),
                ("cfo_estimate_sf_mask", C.c_uint32), ("sync_error_enable", C.c_uint8)]


CHEST_RES_FIELDS = ("noise_estimate", "noise_estimate_dbm", "snr_db", "rsrp", "rsrp_dbm", "rsrq", "rsrq_db", "rssi_dbm", "cfo", "sync_error")


class DmrsPuschCfg(C.Structure):
    C_TYPE = "srslte_hip_dmrs_pusch_cfg_t"
    _fields_ = [("cyclic_shift", C.c_uint32), ("delta_ss", C.c_uint32), ("group_hopping_en", C.c_int), ("sequence_hopping_en", C.c_int)]


class ChestUlRes(C.Structure):
    C_TYPE = "srslte_hip_chest_ul_res_t"
    _fields_ = [(n, C.c_float) for n in ("noise_estimate", "noise_estimate_dbm", "snr", "snr_db", "cfo")]


class Cbsegm(C.Structure):
    """srslte_cbsegm_t (cbsegm.h:33-44)."""
    C_TYPE = "srslte_hip_cbsegm_t"
    _fields_ = [(n, C.c_uint32) for n in ("F", "C", "K1", "K2", "K1_idx", "K2_idx", "C1", "C2", "tbs")]


_TDEC_RUN = [vp, vp, u32, cint, u32, u32, u32, u32, u32, vp, u32, vp, vp, vp]
_DEMOD = [cint, vp, vp, cint, cint, vp]

SIGNATURES = {
    # OFDM
    "srslte_hip_ofdm_create": (vp, [cint, cint, cint]),
    "srslte_hip_ofdm_create_sz": (vp, [cint, cint, cint, cint]),
    "srslte_hip_ofdm_destroy": (void, [vp]),
    "srslte_hip_ofdm_set_normalize": (None, [vp, cint]),
    "srslte_hip_ofdm_set_freq_shift": (None, [vp, f32]),
    "srslte_hip_ofdm_symbol_sz": (None, [vp]),
    "srslte_hip_ofdm_sf_len": (None, [vp]),
    "srslte_hip_ofdm_rx_sf_batch": (None, [vp, vp, vp, cint, vp]),
    "srslte_hip_ofdm_tx_sf_batch": (None, [vp, vp, vp, cint, vp]),
    "srslte_hip_ofdm_set_mbsfn": (None, [vp, cint, cint]),
    "srslte_hip_ofdm_slot_batch": (None, [vp, vp, vp, cint, cint, cint, vp]),
    "srslte_hip_ofdm_set_sample_format": (None, [vp, cint, f32]),
    "srslte_hip_dft_batch": (None, [vp, vp, cint, cint, cint, cint, cint, f32, vp]),
    "srslte_hip_dft_precoding_valid_prb": (None, [u32]),
    "srslte_hip_dft_precoding_batch": (None, [vp, vp, u32, u32, cint, vp]),
    # DL channel estimator
    "srslte_hip_chest_dl_create": (vp, [u32, u32, u32, cint]),
    "srslte_hip_chest_dl_set_tdd": (None, [vp, cint, cint]),
    "srslte_hip_chest_dl_destroy": (void, [vp]),
    "srslte_hip_chest_dl_set_symbol_sz": (None, [vp, cint]),
    "srslte_hip_chest_dl_pilots": (vp, [vp]),
    "srslte_hip_chest_dl_estimate_batch": (None, [vp, P(ChestDlCfg), u32, vp, vp, vp, cint, vp]),
    "srslte_hip_chest_dl_estimate_batch_multi": (None, [vp, P(ChestDlCfg), u32, vp, vp, vp, cint, cint, vp]),
    "srslte_hip_chest_dl_last_raw": (vp, [vp]),
    "srslte_hip_chest_dl_set_mbsfn_area_id": (None, [vp, u16]),
    "srslte_hip_chest_dl_mbsfn_pilots": (vp, [vp, u16]),
    "srslte_hip_chest_dl_estimate_mbsfn_batch": (None, [vp, P(ChestDlCfg), u32, vp, vp, vp, cint, cint, vp]),
    # UL channel estimator
    "srslte_hip_chest_ul_create": (vp, [u32, u32, cint, P(DmrsPuschCfg)]),
    "srslte_hip_chest_ul_destroy": (void, [vp]),
    "srslte_hip_refsignal_dmrs_pusch_gen": (None, [vp, u32, u32, u32, vp]),
    "srslte_hip_chest_ul_estimate_pusch_batch": (None, [vp, u32, u32, u32, u32, vp, vp, vp, cint, vp]),
    "srslte_hip_chest_ul_estimate_pusch_batch_hop": (None, [vp, u32, u32, u32, u32, u32, vp, vp, vp, cint, vp]),
    # soft demapper
    "srslte_hip_demod_soft_demodulate_batch": (None, _DEMOD),
    "srslte_hip_demod_soft_demodulate_s_batch": (None, _DEMOD),
    "srslte_hip_demod_soft_demodulate_b_batch": (None, _DEMOD),
    # turbo decoder
    "srslte_hip_tdec_create": (vp, [u32, u32]),
    "srslte_hip_tdec_destroy": (void, [vp]),
    "srslte_hip_tdec_autoimp_get_subblocks": (u32, [u32]),
    "srslte_hip_tdec_input_len": (u32, [u32, cint]),
    "srslte_hip_tdec_run_batch": (None, _TDEC_RUN),
    "srslte_hip_tdec_run_batch_manual": (None, [vp, vp, u32, cint, u32, u32, u32, u32, u32, u32, vp, u32, vp, vp, vp]),
    "srslte_hip_tdec_autoimp_get_subblocks_8bit": (u32, [u32]),
    "srslte_hip_tdec_run_batch_8bit": (None, _TDEC_RUN),
    # turbo encoder
    "srslte_hip_tcod_encode_batch": (None, [vp, vp, u32, u32, vp]),
    "srslte_hip_tcod_encode_bytes_batch": (None, [vp, u32, vp, u32, vp, u32, u32, vp]),
    # segmentation / interleaver
    "srslte_hip_cbsegm": (None, [P(Cbsegm), u32]),
    "srslte_hip_cbsegm_cbindex": (None, [u32]),
    "srslte_hip_cbsegm_cbsize": (None, [u32]),
    "srslte_hip_tc_interl_LTE_gen_interl": (None, [vp, vp, u32, u32]),
    # one transport block with host buffers in one device call, receive and transmit
    "srslte_hip_sch_create": (vp, [u32, u32, cint]),
    "srslte_hip_sch_destroy": (void, [vp]),
    "srslte_hip_sch_decode": (None, [vp, vp, u32, u32, cint, u32, u32, u32, vp, vp, vp, vp]),
    "srslte_hip_ulsch_decode": (None, [vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "srslte_hip_ulsch_debug_g": (None, [vp, vp, u32]),
    "srslte_hip_pusch_decode": (None, [vp, vp, vp, f32, vp, vp, vp, vp, vp, vp]),
    "srslte_hip_pusch_rows": (None, [vp, vp]),
    "srslte_hip_pusch_debug_q": (None, [vp, vp, u32]),
    "srslte_hip_sch_enc_create": (vp, [u32, u32]),
    "srslte_hip_sch_enc_destroy": (void, [vp]),
    "srslte_hip_sch_encode": (None, [vp, vp, u32, cint, u32, u32, u32, vp, vp]),
    "srslte_hip_ulsch_encode": (None, [vp, vp, vp, vp, vp, vp, vp]),
    "srslte_hip_ulsch_enc_debug": (None, [vp, vp, u32]),
}


class Ofdm(Handle):
    """srslte_ofdm_t: srslte_ofdm_rx_init/tx_init + set_normalize/set_freq_shift + rx_sf/tx_sf (ofdm.h), batched."""
    DESTROY = "srslte_hip_ofdm_destroy"

    def __init__(self, nof_prb, cp_norm=True, rx=True, symbol_sz=None):
        """symbol_sz: None = srslte_symbol_sz(nof_prb) of the default rate family; else as srslte_ofdm_init_ takes it (e.g. 2048 for 100 PRB
        after srslte_use_standard_symbol_size(true))."""
        if symbol_sz is None:
            self._create("srslte_hip_ofdm_create", nof_prb, 1 if cp_norm else 0, 1 if rx else 0)
        else:
            self._create("srslte_hip_ofdm_create_sz", nof_prb, symbol_sz, 1 if cp_norm else 0, 1 if rx else 0)
        self.nof_prb, self.rx = nof_prb, rx
        self.nsym = 14 if cp_norm else 12
        self.sf_len = lib().srslte_hip_ofdm_sf_len(self.h)
        self.grid_len = self.nsym * 12 * nof_prb
        self.iq_format = IQ_CF32

    def set_sample_format(self, fmt, scale=1.0):
        """IQ_SC16: time samples are int16 pairs [nof_sf][sf_len][2] (phy_hip.h, "Sample formats"). Returns the status code; a refused call
        leaves the object as it was."""
        rc = lib().srslte_hip_ofdm_set_sample_format(self.h, fmt, scale)
        if rc == SRSLTE_SUCCESS:
            self.iq_format = fmt
        return rc

    def set_normalize(self, en):
        _check(lib().srslte_hip_ofdm_set_normalize(self.h, 1 if en else 0), "set_normalize")

    def set_freq_shift(self, f):
        _check(lib().srslte_hip_ofdm_set_freq_shift(self.h, f), "set_freq_shift")

    def rx_sf(self, time_samples):
        if self.iq_format == IQ_SC16:
            x = np.ascontiguousarray(time_samples, np.int16).reshape(-1, 2 * self.sf_len)
        else:
            x = np.ascontiguousarray(time_samples, np.complex64).reshape(-1, self.sf_len)
        din, dout = DevBuf.from_host(x), DevBuf(x.shape[0] * self.grid_len * 8)
        _check(lib().srslte_hip_ofdm_rx_sf_batch(self.h, din.ptr, dout.ptr, x.shape[0], None), "ofdm_rx_sf_batch")
        sync()
        return dout.to_host(np.complex64).reshape(x.shape[0], self.grid_len)

    def tx_sf(self, grid):
        x = np.ascontiguousarray(grid, np.complex64).reshape(-1, self.grid_len)
        din, dout = DevBuf.from_host(x), DevBuf(x.shape[0] * self.sf_len * 8)
        _check(lib().srslte_hip_ofdm_tx_sf_batch(self.h, din.ptr, dout.ptr, x.shape[0], None), "ofdm_tx_sf_batch")
        sync()
        if self.iq_format == IQ_SC16:
            return dout.to_host(np.int16, 2 * x.shape[0] * self.sf_len).reshape(x.shape[0], self.sf_len, 2)
        return dout.to_host(np.complex64).reshape(x.shape[0], self.sf_len)


def dft(x, forward=True, scale=1.0):
    """srslte_dft_run_c on each row of x (unnormalised unless scale given)."""
    x = np.ascontiguousarray(x, np.complex64)
    x2 = x.reshape(-1, x.shape[-1])
    din, dout = DevBuf.from_host(x2), DevBuf(x2.nbytes)
    n = x2.shape[1]
    rc = lib().srslte_hip_dft_batch(din.ptr, dout.ptr, n, x2.shape[0], n, n, 1 if forward else 0, scale, None)
    _check(rc, "dft_batch")
    sync()
    return dout.to_host(np.complex64).reshape(x.shape)


def dft_precoding(x, nof_prb, nof_symbols, forward=True):
    """srslte_dft_precoding (dft_precoding.c:100-113)."""
    x = np.ascontiguousarray(x, np.complex64)
    din, dout = DevBuf.from_host(x), DevBuf(x.nbytes)
    rc = lib().srslte_hip_dft_precoding_batch(din.ptr, dout.ptr, nof_prb, nof_symbols, 1 if forward else 0, None)
    if rc != SRSLTE_SUCCESS:
        return rc, None
    sync()
    return rc, dout.to_host(np.complex64).reshape(x.shape)


class ChestDl(Handle):
    """srslte_chest_dl_t: init + set_cell + estimate_cfg (chest_dl.h:132-156), batched over subframes tti0, tti0+1, ..."""
    DESTROY = "srslte_hip_chest_dl_destroy"

    def __init__(self, cell_id, nof_prb, nof_ports=1, cp_norm=True):
        self._create("srslte_hip_chest_dl_create", cell_id, nof_prb, nof_ports, 1 if cp_norm else 0)
        self.grid_len = (14 if cp_norm else 12) * 12 * nof_prb
        self.nof_ports = nof_ports

    def set_tdd(self, sf_config, ss_config):
        """TDD cell: srslte_tdd_config_t of the subframes (sf_config < 0: FDD again)."""
        return lib().srslte_hip_chest_dl_set_tdd(self.h, sf_config, ss_config)

    def set_mbsfn_area_id(self, area_id):
        """srslte_chest_dl_set_mbsfn_area_id (chest_dl.c:244-262)."""
        return lib().srslte_hip_chest_dl_set_mbsfn_area_id(self.h, area_id)

    def estimate_mbsfn(self, grid, tti0, cfg, nof_rx=1, want_ce=True):
        """MBSFN subframes (cfg.mbsfn_area_id): grid [nof_sf][nof_rx][14*12*prb] -> (rc, ce [nof_sf][nof_ports][nof_rx][...], noise
        [nof_sf][nof_ports][nof_rx]); symbols 12, 13 of ce are not written (returned as zeros)."""
        g = np.ascontiguousarray(grid, np.complex64).reshape(-1, nof_rx, self.grid_len)
        n = g.shape[0]
        dg, dce, dn = DevBuf.from_host(g), DevBuf(g.nbytes * self.nof_ports), DevBuf(4 * n * nof_rx * self.nof_ports)
        _check(lib().srslte_hip_memset(dce.ptr, 0, g.nbytes * self.nof_ports), "memset")
        rc = lib().srslte_hip_chest_dl_estimate_mbsfn_batch(self.h, C.byref(cfg), tti0, dg.ptr, dce.ptr if want_ce else None, dn.ptr, n, nof_rx, None)
        if rc != SRSLTE_SUCCESS:
            return rc, None, None
        sync()
        return rc, dce.to_host(np.complex64).reshape(n, self.nof_ports, nof_rx, self.grid_len), dn.to_host(np.float32).reshape(n, self.nof_ports, nof_rx)

    def estimate_multi(self, grid, tti0, cfg, nof_rx=1, ce_in=None):
        """grid [nof_sf][nof_rx][14*12*prb] -> (rc, ce [nof_sf][nof_ports][nof_rx][...], res dict, raw [nof_sf][nof_ports][nof_rx][6]).
        ce_in: what the estimate buffer holds before the call (4-port cells with interpolate_subframe keep symbol 0 of ports 2/3)."""
        g = np.ascontiguousarray(grid, np.complex64).reshape(-1, nof_rx, self.grid_len)
        n = g.shape[0]
        dg, dres = DevBuf.from_host(g), DevBuf(n * 40)
        dce = DevBuf(g.nbytes * self.nof_ports) if ce_in is None else DevBuf.from_host(np.ascontiguousarray(ce_in, np.complex64))
        rc = lib().srslte_hip_chest_dl_estimate_batch_multi(self.h, C.byref(cfg), tti0, dg.ptr, dce.ptr, dres.ptr, n, nof_rx, None)
        if rc != SRSLTE_SUCCESS:
            return rc, None, None, None
        sync()
        res = dres.to_host(np.float32).reshape(n, 10)
        raw = host_copy(lib().srslte_hip_chest_dl_last_raw(self.h), np.float32, n * self.nof_ports * nof_rx * 6)
        return (rc, dce.to_host(np.complex64).reshape(n, self.nof_ports, nof_rx, self.grid_len), {k: res[:, i] for i, k in enumerate(CHEST_RES_FIELDS)},
                raw.reshape(n, self.nof_ports, nof_rx, 6))

    def estimate(self, grid, tti0=0, cfg=None, want_ce=True):
        cfg = cfg or ChestDlCfg()
        g = np.ascontiguousarray(grid, np.complex64).reshape(-1, self.grid_len)
        n = g.shape[0]
        dg, dce, dres = DevBuf.from_host(g), DevBuf(g.nbytes), DevBuf(n * 40)
        rc = lib().srslte_hip_chest_dl_estimate_batch(self.h, C.byref(cfg), tti0, dg.ptr, dce.ptr if want_ce else None, dres.ptr, n, None)
        _check(rc, "chest_dl_estimate_batch")
        sync()
        res = dres.to_host(np.float32).reshape(n, 10)
        return (dce.to_host(np.complex64).reshape(n, self.grid_len) if want_ce else None), {k: res[:, i] for i, k in enumerate(CHEST_RES_FIELDS)}


_LLR_DT = {"f": np.float32, "s": np.int16, "b": np.int8}


def demod_soft_demodulate(mod, symbols, kind="s", ncalls=1):
    """srslte_demod_soft_demodulate / _s / _b (demod_soft.h:39-53); kind in 'f','s','b'. Returns (rc, llr)."""
    s = np.ascontiguousarray(symbols, np.complex64).reshape(ncalls, -1)
    nsym = s.shape[1]
    qm = 1 if mod == MOD_BPSK else 2 * mod
    dt = np.dtype(_LLR_DT[kind])
    ds, dl = DevBuf.from_host(s), DevBuf(max(1, s.size * qm * dt.itemsize))
    fn = getattr(lib(), "srslte_hip_demod_soft_demodulate%s_batch" % ("" if kind == "f" else "_" + kind))
    rc = fn(mod, ds.ptr, dl.ptr, nsym, ncalls, None)
    if rc != SRSLTE_SUCCESS:
        return rc, None
    sync()
    return rc, dl.to_host(dt, s.size * qm).reshape(ncalls, nsym * qm)


class Tdec(Handle):
    """srslte_tdec_t: srslte_tdec_init + srslte_tdec_run_all / iteration-with-CRC (turbodecoder.h:63-135), batched."""
    DESTROY = "srslte_hip_tdec_destroy"

    def __init__(self, max_long_cb=6144, max_nof_cb=64):
        self._create("srslte_hip_tdec_create", max_long_cb, max_nof_cb)

    def run_all(self, llr, long_cb, nof_iterations, sb_layout=False, crc_poly=0, crc_nbits=0, force_subblocks=None, llr8=False):
        """llr8: int8 LLRs through srslte_hip_tdec_run_batch_8bit (srslte_tdec_run_all_8bit, turbodecoder.c:573-588)."""
        x = np.ascontiguousarray(llr, np.int8 if llr8 else np.int16)
        x = x.reshape(-1, x.shape[-1])
        ncb = x.shape[0]
        din, dout = DevBuf.from_host(x), DevBuf(ncb * (long_cb // 8))
        dit, dok = DevBuf(4 * ncb), DevBuf(ncb)
        if llr8:
            rc = lib().srslte_hip_tdec_run_batch_8bit(self.h, din.ptr, x.shape[1], 1 if sb_layout else 0, long_cb, ncb, nof_iterations, crc_poly,
                                                      crc_nbits, dout.ptr, long_cb // 8, dit.ptr, dok.ptr, None)
        elif force_subblocks is None:
            rc = lib().srslte_hip_tdec_run_batch(self.h, din.ptr, x.shape[1], 1 if sb_layout else 0, long_cb, ncb, nof_iterations, crc_poly,
                                                 crc_nbits, dout.ptr, long_cb // 8, dit.ptr, dok.ptr, None)
        else:
            rc = lib().srslte_hip_tdec_run_batch_manual(self.h, din.ptr, x.shape[1], 1 if sb_layout else 0, long_cb, force_subblocks, ncb,
                                                        nof_iterations, crc_poly, crc_nbits, dout.ptr, long_cb // 8, dit.ptr, dok.ptr, None)
        if rc != SRSLTE_SUCCESS:
            return rc, None, None, None
        sync()
        return rc, dout.to_host(np.uint8).reshape(ncb, long_cb // 8), dit.to_host(np.uint32), dok.to_host(np.uint8)


def tcod_encode(bits, long_cb):
    """srslte_tcod_encode (turbocoder.c:76-186): [ncb][K] bits -> [ncb][3K+12]. Returns (rc, out)."""
    x = np.ascontiguousarray(bits, np.uint8).reshape(-1, long_cb)
    din, dout = DevBuf.from_host(x), DevBuf(x.shape[0] * (3 * long_cb + 12))
    rc = lib().srslte_hip_tcod_encode_batch(din.ptr, dout.ptr, long_cb, x.shape[0], None)
    if rc != SRSLTE_SUCCESS:
        return rc, None
    sync()
    return rc, dout.to_host(np.uint8).reshape(x.shape[0], 3 * long_cb + 12)


def cbsegm(tbs):
    s = Cbsegm()
    rc = lib().srslte_hip_cbsegm(C.byref(s), tbs)
    return rc, s


def tc_interl(long_cb, win=1):
    f, r = np.zeros(long_cb, np.uint16), np.zeros(long_cb, np.uint16)
    rc = lib().srslte_hip_tc_interl_LTE_gen_interl(f.ctypes.data, r.ctypes.data, long_cb, win)
    return rc, f, r


class SchEnc(Handle):
    """srslte_hip_sch_enc_t: one transport block with host buffers in one device call, what encode_tb_off does behind srslte_dlsch_encode2
    (sch.c:183-289,:549-575)."""
    DESTROY = "srslte_hip_sch_enc_destroy"

    def __init__(self, max_tbs, max_e_bits):
        self._create("srslte_hip_sch_enc_create", max_tbs, max_e_bits)

    def encode(self, data, tbs, mod, Nl, rv, nof_e_bits, buffer_b):
        """data: tbs / 8 bytes or None (a retransmission); buffer_b: the code blocks' circular buffers, a list of C writable uint8 arrays of at
        least ceil((3K + 12) / 8) bytes (written for rv 0, read for rv 1-3) -> (rc, the e bits, one per element; None where nothing was written)."""
        d = None if data is None else np.ascontiguousarray(data, np.uint8)
        ptrs = (C.c_void_p * max(1, len(buffer_b)))(*[b.ctypes.data for b in buffer_b])
        e = np.zeros((nof_e_bits + 7) // 8 + 8, np.uint8)
        rc = lib().srslte_hip_sch_encode(self.h, None if d is None else d.ctypes.data, tbs, mod, Nl, rv, nof_e_bits, ptrs, e.ctypes.data)
        if rc != SRSLTE_SUCCESS or tbs == 0:
            return rc, None
        return rc, np.unpackbits(e)[:nof_e_bits // (2 * mod * Nl) * (2 * mod * Nl)]


class ChestUl(Handle):
    """srslte_chest_ul_t: init + set_cell + pregen + estimate_pusch (chest_ul.h:78-104), batched over subframes tti0, tti0+1, ..."""
    DESTROY = "srslte_hip_chest_ul_destroy"

    def __init__(self, cell_id, nof_prb, cyclic_shift=0, delta_ss=0, group_hopping=False, sequence_hopping=False, cp_ext=False):
        self.cfg = DmrsPuschCfg(cyclic_shift, delta_ss, 1 if group_hopping else 0, 1 if sequence_hopping else 0)
        self._create("srslte_hip_chest_ul_create", cell_id, nof_prb, 0 if cp_ext else 1, C.byref(self.cfg))
        self.nof_prb, self.nof_symb = nof_prb, 12 if cp_ext else 14

    def dmrs(self, L_prb, sf_idx, n_dmrs):
        r = np.zeros(2 * 12 * L_prb, np.complex64)
        rc = lib().srslte_hip_refsignal_dmrs_pusch_gen(self.h, L_prb, sf_idx, n_dmrs, r.ctypes.data)
        return rc, r

    def estimate_pusch(self, grid, tti0, L_prb, n_prb, n_dmrs, ce_init=None):
        x = np.ascontiguousarray(grid, np.complex64).reshape(-1, self.nof_symb * 12 * self.nof_prb)
        n = x.shape[0]
        dg = DevBuf.from_host(x)
        dce = DevBuf.from_host(np.zeros_like(x) if ce_init is None else np.ascontiguousarray(ce_init, np.complex64))
        dres = DevBuf(n * C.sizeof(ChestUlRes))
        rc = lib().srslte_hip_chest_ul_estimate_pusch_batch(self.h, tti0, L_prb, n_prb, n_dmrs, dg.ptr, dce.ptr, dres.ptr, n, None)
        if rc != SRSLTE_SUCCESS:
            return rc, None, None
        sync()
        return rc, dce.to_host(np.complex64).reshape(x.shape), dres.to_host(np.float32).reshape(n, 5)
