"""srslte-emane_amd — MI355X-native drop-in for the sample-level hot path of srsLTE's lib/src/phy.

The product is ``csrc/libsrslte_phy_hip.so`` (hand-written HIP for gfx950 behind a C ABI, see
``include/srslte_hip/phy_hip.h``). This module is only the host-side mirror of the reference's operator
interface used by the tests, ``bench.py`` and ``__graft_entry__``: same names, argument meaning and error
behaviour as the ``srslte_*`` calls, numpy arrays in and out, device buffers managed through the C ABI.

There is NO CPU fallback: importing the native handle without a built library raises, and every call needs a GPU.
(The directory name carries a hyphen; import it with ``importlib.import_module("srslte-emane_amd")``.)
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libsrslte_phy_hip.so")

SRSLTE_SUCCESS, SRSLTE_ERROR, SRSLTE_ERROR_INVALID_INPUTS = 0, -1, -2
MOD_BPSK, MOD_QPSK, MOD_16QAM, MOD_64QAM, MOD_256QAM = range(5)
CRC24A, CRC24B = 0x1864CFB, 0x1800063

_lib = None


class ChestDlCfg(C.Structure):
    """srslte_chest_dl_cfg_t (chest_dl.h:116-130)."""
    _fields_ = [("noise_alg", C.c_int), ("filter_type", C.c_int), ("filter_coef", C.c_float * 2), ("mbsfn_area_id", C.c_uint16),
                ("interpolate_subframe", C.c_uint8), ("rsrp_neighbour", C.c_uint8), ("cfo_estimate_enable", C.c_uint8),
                ("cfo_estimate_sf_mask", C.c_uint32), ("sync_error_enable", C.c_uint8)]


CHEST_RES_FIELDS = ("noise_estimate", "noise_estimate_dbm", "snr_db", "rsrp", "rsrp_dbm", "rsrq", "rsrq_db", "rssi_dbm", "cfo", "sync_error")


class Cbsegm(C.Structure):
    """srslte_cbsegm_t (cbsegm.h:33-44)."""
    _fields_ = [(n, C.c_uint32) for n in ("F", "C", "K1", "K2", "K1_idx", "K2_idx", "C1", "C2", "tbs")]


class DlRxCfg(C.Structure):
    _fields_ = [("cell_id", C.c_uint32), ("nof_prb", C.c_uint32), ("cfi", C.c_uint32), ("rnti", C.c_uint16), ("mod", C.c_int),
                ("tbs", C.c_uint32), ("max_iterations", C.c_uint32), ("max_batch", C.c_uint32), ("mmse", C.c_int), ("chest_cfg", ChestDlCfg),
                ("llr_8bit", C.c_int), ("nof_rx_antennas", C.c_uint32), ("nof_ports", C.c_uint32), ("csi_enable", C.c_int), ("power_scale", C.c_int), ("p_a", C.c_float),
                ("tx_scheme", C.c_int), ("pmi", C.c_uint32), ("mod2", C.c_int), ("tbs2", C.c_uint32), ("cp_ext", C.c_int),
                ("tdd", C.c_int), ("tdd_sf_config", C.c_uint32), ("tdd_ss_config", C.c_uint32),
                ("mbsfn", C.c_int), ("mbsfn_area_id", C.c_uint32), ("non_mbsfn_region", C.c_uint32)]


class DlGrant(C.Structure):
    """srslte_hip_dl_grant_t (phy_hip.h): the per-subframe part of srslte_pdsch_cfg_t / srslte_pdsch_grant_t."""
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


def lib():
    """The native library; raises if it was not built (no fallback path exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        vp = C.c_void_p
        L.srslte_hip_malloc.restype = vp
        L.srslte_hip_malloc.argtypes = [C.c_size_t]
        L.srslte_hip_free.argtypes = [vp]
        L.srslte_hip_memcpy_h2d.argtypes = [vp, vp, C.c_size_t]
        L.srslte_hip_memcpy_d2h.argtypes = [vp, vp, C.c_size_t]
        L.srslte_hip_memset.argtypes = [vp, C.c_int, C.c_size_t]
        L.srslte_hip_stream_create.restype = vp
        L.srslte_hip_stream_destroy.argtypes = [vp]
        L.srslte_hip_stream_sync.argtypes = [vp]
        L.srslte_hip_event_create.restype = vp
        L.srslte_hip_event_record.argtypes = [vp, vp]
        L.srslte_hip_event_elapsed_ms.restype = C.c_float
        L.srslte_hip_event_elapsed_ms.argtypes = [vp, vp]
        L.srslte_hip_event_destroy.argtypes = [vp]
        L.srslte_hip_ofdm_create.restype = vp
        L.srslte_hip_ofdm_create.argtypes = [C.c_int, C.c_int, C.c_int]
        L.srslte_hip_ofdm_create_sz.restype = vp
        L.srslte_hip_ofdm_create_sz.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
        L.srslte_hip_ofdm_destroy.argtypes = [vp]
        L.srslte_hip_ofdm_set_normalize.argtypes = [vp, C.c_int]
        L.srslte_hip_ofdm_set_freq_shift.argtypes = [vp, C.c_float]
        L.srslte_hip_ofdm_symbol_sz.argtypes = [vp]
        L.srslte_hip_ofdm_sf_len.argtypes = [vp]
        L.srslte_hip_ofdm_rx_sf_batch.argtypes = [vp, vp, vp, C.c_int, vp]
        L.srslte_hip_ofdm_tx_sf_batch.argtypes = [vp, vp, vp, C.c_int, vp]
        L.srslte_hip_dft_batch.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, vp]
        L.srslte_hip_dft_precoding_batch.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_int, vp]
        L.srslte_hip_chest_dl_create.restype = vp
        L.srslte_hip_chest_dl_create.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
        L.srslte_hip_chest_dl_destroy.argtypes = [vp]
        L.srslte_hip_chest_dl_estimate_batch.argtypes = [vp, C.POINTER(ChestDlCfg), C.c_uint32, vp, vp, vp, C.c_int, vp]
        L.srslte_hip_chest_dl_set_mbsfn_area_id.argtypes = [vp, C.c_uint16]
        L.srslte_hip_chest_dl_mbsfn_pilots.restype = vp
        L.srslte_hip_chest_dl_mbsfn_pilots.argtypes = [vp, C.c_uint16]
        L.srslte_hip_chest_dl_estimate_mbsfn_batch.argtypes = [vp, C.POINTER(ChestDlCfg), C.c_uint32, vp, vp, vp, C.c_int, C.c_int, vp]
        for n in ("", "_s", "_b"):
            getattr(L, "srslte_hip_demod_soft_demodulate%s_batch" % n).argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, vp]
        L.srslte_hip_tdec_create.restype = vp
        L.srslte_hip_tdec_create.argtypes = [C.c_uint32, C.c_uint32]
        L.srslte_hip_tdec_destroy.argtypes = [vp]
        L.srslte_hip_tdec_autoimp_get_subblocks.restype = C.c_uint32
        L.srslte_hip_tdec_input_len.restype = C.c_uint32
        L.srslte_hip_tdec_run_batch.argtypes = [vp, vp, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                vp, C.c_uint32, vp, vp, vp]
        L.srslte_hip_tdec_run_batch_manual.argtypes = [vp, vp, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                       C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, vp, vp]
        L.srslte_hip_tdec_run_batch_8bit.argtypes = L.srslte_hip_tdec_run_batch.argtypes
        L.srslte_hip_tdec_autoimp_get_subblocks_8bit.restype = C.c_uint32
        L.srslte_hip_tcod_encode_batch.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp]
        L.srslte_hip_tcod_encode_bytes_batch.argtypes = [vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, vp]
        L.srslte_hip_cbsegm.argtypes = [C.POINTER(Cbsegm), C.c_uint32]
        L.srslte_hip_sch_enc_create.restype = vp
        L.srslte_hip_sch_enc_create.argtypes = [C.c_uint32, C.c_uint32]
        L.srslte_hip_sch_enc_destroy.argtypes = [vp]
        L.srslte_hip_sch_encode.argtypes = [vp, vp, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp]
        L.srslte_hip_tc_interl_LTE_gen_interl.argtypes = [vp, vp, C.c_uint32, C.c_uint32]
        L.srslte_hip_dl_rx_create.restype = vp
        L.srslte_hip_dl_rx_create.argtypes = [C.POINTER(DlRxCfg)]
        L.srslte_hip_dl_rx_destroy.argtypes = [vp]
        L.srslte_hip_dl_rx_nof_re.restype = C.c_uint32
        L.srslte_hip_dl_rx_nof_re.argtypes = [vp, C.c_uint32]
        L.srslte_hip_dl_rx_batch.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, vp]
        L.srslte_hip_dl_rx_grid_batch.argtypes = L.srslte_hip_dl_rx_batch.argtypes
        L.srslte_hip_dl_rx_stage.argtypes = [vp, C.c_int, vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, vp]
        L.srslte_hip_dl_rx_batch_grants.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.POINTER(DlGrant), vp, C.c_uint32, vp, vp]
        L.srslte_hip_dl_rx_debug_buffer.restype = vp
        L.srslte_hip_dl_rx_debug_buffer.argtypes = [vp, C.c_int]
        L.srslte_hip_dl_rx_keep_symbols.argtypes = [vp, C.c_int]
        L.srslte_hip_dl_rx_parity_compact.argtypes = [vp]
        L.srslte_hip_rm_parity_compact_limit.restype = C.c_uint32
        L.srslte_hip_rm_parity_compact_limit.argtypes = [C.c_uint32]
        _bind_dl_ctrl(L)
        _bind_ul_ctrl(L)
        _bind_prach(L)
        _bind_csi(L)
        _bind_channel(L)
        _bind_srs(L)
        _bind_sync(L)
        _bind_meas(L)
        _bind_nbiot(L)
        _lib = L
    return _lib


def _check(rc, what):
    if rc != SRSLTE_SUCCESS:
        raise RuntimeError("%s failed with %d" % (what, rc))


class DevBuf:
    """A device allocation owned through the C ABI."""

    _poison = 0

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.ptr = lib().srslte_hip_malloc(self.nbytes)
        if not self.ptr:
            raise MemoryError("srslte_hip_malloc(%d)" % nbytes)
        if os.environ.get("SRSLTE_HIP_TEST_POISON"):  # tests: every allocation starts with its own byte pattern, so that comparing or
            DevBuf._poison = (DevBuf._poison * 37 + 11) & 0xFF  # reading bytes nobody wrote fails every time, not once in a while
            fill = np.full(self.nbytes, DevBuf._poison, np.uint8)
            _check(lib().srslte_hip_memcpy_h2d(self.ptr, fill.ctypes.data, fill.nbytes), "memcpy_h2d")

    @classmethod
    def from_host(cls, arr):
        arr = np.ascontiguousarray(arr)
        b = cls(max(arr.nbytes, 1))
        _check(lib().srslte_hip_memcpy_h2d(b.ptr, arr.ctypes.data, arr.nbytes), "memcpy_h2d")
        return b

    def to_host(self, dtype, count=None):
        dtype = np.dtype(dtype)
        n = self.nbytes // dtype.itemsize if count is None else int(count)
        out = np.empty(n, dtype)
        _check(lib().srslte_hip_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes), "memcpy_d2h")
        return out

    def free(self):
        if self.ptr:
            lib().srslte_hip_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DevView(DevBuf):
    """Device memory owned by somebody else (e.g. a torch tensor), seen through the same interface."""

    def __init__(self, ptr, nbytes):
        self.nbytes, self.ptr = int(nbytes), int(ptr)

    def free(self):
        self.ptr = None


def sync():
    _check(lib().srslte_hip_sync(), "sync")


def symbol_sz(nof_prb):
    """srslte_symbol_sz (phy_common.c:322-345)."""
    for lim, n in ((6, 128), (15, 256), (25, 384), (50, 768), (75, 1024), (110, 1536)):
        if 0 < nof_prb <= lim:
            return n
    return -1


class Ofdm:
    """srslte_ofdm_t: srslte_ofdm_rx_init/tx_init + set_normalize/set_freq_shift + rx_sf/tx_sf (ofdm.h), batched."""

    def __init__(self, nof_prb, cp_norm=True, rx=True, symbol_sz=None):
        """symbol_sz: None = srslte_symbol_sz(nof_prb) of the default rate family; else as srslte_ofdm_init_ takes it (e.g. 2048 for 100 PRB
        after srslte_use_standard_symbol_size(true))."""
        if symbol_sz is None:
            self.h = lib().srslte_hip_ofdm_create(nof_prb, 1 if cp_norm else 0, 1 if rx else 0)
        else:
            self.h = lib().srslte_hip_ofdm_create_sz(nof_prb, symbol_sz, 1 if cp_norm else 0, 1 if rx else 0)
        if not self.h:
            raise RuntimeError("srslte_hip_ofdm_create failed")
        self.nof_prb, self.rx = nof_prb, rx
        self.nsym = 14 if cp_norm else 12
        self.sf_len = lib().srslte_hip_ofdm_sf_len(self.h)
        self.grid_len = self.nsym * 12 * nof_prb

    def set_normalize(self, en):
        _check(lib().srslte_hip_ofdm_set_normalize(self.h, 1 if en else 0), "set_normalize")

    def set_freq_shift(self, f):
        _check(lib().srslte_hip_ofdm_set_freq_shift(self.h, f), "set_freq_shift")

    def rx_sf(self, time_samples):
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
        return dout.to_host(np.complex64).reshape(x.shape[0], self.sf_len)

    def free(self):
        if self.h:
            lib().srslte_hip_ofdm_destroy(self.h)
            self.h = None


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


class ChestDl:
    """srslte_chest_dl_t: init + set_cell + estimate_cfg (chest_dl.h:132-156), batched over subframes tti0, tti0+1, ..."""

    def __init__(self, cell_id, nof_prb, nof_ports=1, cp_norm=True):
        self.h = lib().srslte_hip_chest_dl_create(cell_id, nof_prb, nof_ports, 1 if cp_norm else 0)
        if not self.h:
            raise RuntimeError("srslte_hip_chest_dl_create failed")
        self.grid_len = (14 if cp_norm else 12) * 12 * nof_prb
        self.nof_ports = nof_ports

    def set_tdd(self, sf_config, ss_config):
        """TDD cell: srslte_tdd_config_t of the subframes (sf_config < 0: FDD again)."""
        L = lib()
        L.srslte_hip_chest_dl_set_tdd.argtypes = [C.c_void_p, C.c_int, C.c_int]
        return L.srslte_hip_chest_dl_set_tdd(self.h, sf_config, ss_config)

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
        L = lib()
        L.srslte_hip_chest_dl_estimate_batch_multi.argtypes = [C.c_void_p, C.POINTER(ChestDlCfg), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                               C.c_int, C.c_int, C.c_void_p]
        L.srslte_hip_chest_dl_last_raw.restype = C.c_void_p
        L.srslte_hip_chest_dl_last_raw.argtypes = [C.c_void_p]
        g = np.ascontiguousarray(grid, np.complex64).reshape(-1, nof_rx, self.grid_len)
        n = g.shape[0]
        dg, dres = DevBuf.from_host(g), DevBuf(n * 40)
        dce = DevBuf(g.nbytes * self.nof_ports) if ce_in is None else DevBuf.from_host(np.ascontiguousarray(ce_in, np.complex64))
        rc = L.srslte_hip_chest_dl_estimate_batch_multi(self.h, C.byref(cfg), tti0, dg.ptr, dce.ptr, dres.ptr, n, nof_rx, None)
        if rc != SRSLTE_SUCCESS:
            return rc, None, None, None
        sync()
        res = dres.to_host(np.float32).reshape(n, 10)
        raw = np.empty(n * self.nof_ports * nof_rx * 6, np.float32)
        _check(L.srslte_hip_memcpy_d2h(raw.ctypes.data, L.srslte_hip_chest_dl_last_raw(self.h), raw.nbytes), "memcpy_d2h")
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

    def free(self):
        if self.h:
            lib().srslte_hip_chest_dl_destroy(self.h)
            self.h = None


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


class Tdec:
    """srslte_tdec_t: srslte_tdec_init + srslte_tdec_run_all / iteration-with-CRC (turbodecoder.h:63-135), batched."""

    def __init__(self, max_long_cb=6144, max_nof_cb=64):
        self.h = lib().srslte_hip_tdec_create(max_long_cb, max_nof_cb)
        if not self.h:
            raise RuntimeError("srslte_hip_tdec_create failed")

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

    def free(self):
        if self.h:
            lib().srslte_hip_tdec_destroy(self.h)
            self.h = None


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


class SchEnc:
    """srslte_hip_sch_enc_t: one transport block with host buffers in one device call, what encode_tb_off does behind srslte_dlsch_encode2
    (sch.c:183-289,:549-575)."""

    def __init__(self, max_tbs, max_e_bits):
        self.h = lib().srslte_hip_sch_enc_create(max_tbs, max_e_bits)
        if not self.h:
            raise RuntimeError("srslte_hip_sch_enc_create failed")

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

    def free(self):
        if self.h:
            lib().srslte_hip_sch_enc_destroy(self.h)
            self.h = None


class DmrsPuschCfg(C.Structure):
    _fields_ = [("cyclic_shift", C.c_uint32), ("delta_ss", C.c_uint32), ("group_hopping_en", C.c_int), ("sequence_hopping_en", C.c_int)]


class ChestUlRes(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("noise_estimate", "noise_estimate_dbm", "snr", "snr_db", "cfo")]


class ChestUl:
    """srslte_chest_ul_t: init + set_cell + pregen + estimate_pusch (chest_ul.h:78-104), batched over subframes tti0, tti0+1, ..."""

    def __init__(self, cell_id, nof_prb, cyclic_shift=0, delta_ss=0, group_hopping=False, sequence_hopping=False, cp_ext=False):
        self.cfg = DmrsPuschCfg(cyclic_shift, delta_ss, 1 if group_hopping else 0, 1 if sequence_hopping else 0)
        lib().srslte_hip_chest_ul_create.restype = C.c_void_p
        lib().srslte_hip_chest_ul_create.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.POINTER(DmrsPuschCfg)]
        self.h = lib().srslte_hip_chest_ul_create(cell_id, nof_prb, 0 if cp_ext else 1, C.byref(self.cfg))
        if not self.h:
            raise RuntimeError("srslte_hip_chest_ul_create failed")
        self.nof_prb, self.nof_symb = nof_prb, 12 if cp_ext else 14

    def dmrs(self, L_prb, sf_idx, n_dmrs):
        r = np.zeros(2 * 12 * L_prb, np.complex64)
        lib().srslte_hip_refsignal_dmrs_pusch_gen.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        rc = lib().srslte_hip_refsignal_dmrs_pusch_gen(self.h, L_prb, sf_idx, n_dmrs, r.ctypes.data)
        return rc, r

    def estimate_pusch(self, grid, tti0, L_prb, n_prb, n_dmrs, ce_init=None):
        x = np.ascontiguousarray(grid, np.complex64).reshape(-1, self.nof_symb * 12 * self.nof_prb)
        n = x.shape[0]
        dg = DevBuf.from_host(x)
        dce = DevBuf.from_host(np.zeros_like(x) if ce_init is None else np.ascontiguousarray(ce_init, np.complex64))
        dres = DevBuf(n * C.sizeof(ChestUlRes))
        f = lib().srslte_hip_chest_ul_estimate_pusch_batch
        f.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        rc = f(self.h, tti0, L_prb, n_prb, n_dmrs, dg.ptr, dce.ptr, dres.ptr, n, None)
        if rc != SRSLTE_SUCCESS:
            return rc, None, None
        sync()
        res = np.frombuffer(dres.to_host(np.uint8).tobytes(), dtype=np.float32).reshape(n, 5)
        return rc, dce.to_host(np.complex64).reshape(x.shape), res

    def free(self):
        if self.h:
            lib().srslte_hip_chest_ul_destroy.argtypes = [C.c_void_p]
            lib().srslte_hip_chest_ul_destroy(self.h)
            self.h = None


class DlGrant2(C.Structure):
    """srslte_hip_dl_grant2_t: a grant with its transmission scheme, pmi and second transport block."""
    _fields_ = [("tb0", DlGrant), ("tx_scheme", C.c_int), ("pmi", C.c_uint32), ("mod2", C.c_int), ("tbs2", C.c_uint32), ("rv2", C.c_uint32), ("new_data2", C.c_int)]


class DlRx:
    """Batched PDSCH receive chain (ue_dl.c:369-384 + pdsch.c:833-997 + sch.c:507-532 for one codeword)."""

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
        self.h = lib().srslte_hip_dl_rx_create(C.byref(self.cfg))
        if not self.h:
            raise RuntimeError("srslte_hip_dl_rx_create failed")
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

    def decode(self, iq, tti0=0):
        x = np.ascontiguousarray(iq, np.complex64).reshape(-1, self.nof_rx * self.sf_len)  # [nsf][nof_rx][sf_len]
        din = DevBuf.from_host(x)
        _check(self.run_device(din.ptr, tti0, x.shape[0]), "dl_rx_batch")
        sync()
        if self.tbs2:  # rows b and nof_sf + b: the two transport blocks of subframe b
            n = x.shape[0]
            tb, ok = self.d_tb.to_host(np.uint8).reshape(-1, self.tb_stride), self.d_ok.to_host(np.uint8)
            return [tb[:n, :self.tbs // 8 + 3], tb[n:2 * n, :self.tbs2 // 8 + 3]], [ok[:n], ok[n:2 * n]]
        tb = self.d_tb.to_host(np.uint8).reshape(self.max_batch, self.tb_stride)[:x.shape[0], :self.tbs // 8 + 3]
        return tb, self.d_ok.to_host(np.uint8)[:x.shape[0]]

    def decode_harq2(self, iq, tti0, rv, new_data):
        """srslte_hip_dl_rx_batch_harq2: rv / new_data per transport block (two-layer modes)."""
        x = np.ascontiguousarray(iq, np.complex64).reshape(-1, self.nof_rx * self.sf_len)
        din = DevBuf.from_host(x)
        n = x.shape[0]
        lib().srslte_hip_dl_rx_batch_harq2.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                                       C.c_void_p, C.c_void_p]
        _check(lib().srslte_hip_dl_rx_batch_harq2(self.h, din.ptr, tti0, n, (C.c_uint32 * 2)(*rv), (C.c_int * 2)(*[1 if v else 0 for v in new_data]),
                                                  self.d_tb.ptr, self.tb_stride, self.d_ok.ptr, None), "dl_rx_batch_harq2")
        sync()
        tb, ok = self.d_tb.to_host(np.uint8).reshape(-1, self.tb_stride), self.d_ok.to_host(np.uint8)
        return [tb[:n, :self.tbs // 8 + 3], tb[n:2 * n, :self.tbs2 // 8 + 3]], [ok[:n], ok[n:2 * n]]

    def decode_grants(self, iq, tti0, grants):
        """srslte_hip_dl_rx_batch_grants: subframe b with grants[b] (DlGrant). Returns (rc, tb [nsf][tbs_max/8+3], ok [nsf])."""
        x = np.ascontiguousarray(iq, np.complex64).reshape(-1, self.nof_rx * self.sf_len)
        assert len(grants) == x.shape[0]
        arr = (DlGrant * len(grants))(*grants)
        din = DevBuf.from_host(x)
        rc = lib().srslte_hip_dl_rx_batch_grants(self.h, din.ptr, tti0, x.shape[0], arr, self.d_tb.ptr, self.tb_stride, self.d_ok.ptr, None)
        if rc != SRSLTE_SUCCESS:
            return rc, None, None
        sync()
        tb = self.d_tb.to_host(np.uint8).reshape(self.max_batch, self.tb_stride)[:x.shape[0], :self.tbs // 8 + 3]
        return rc, tb, self.d_ok.to_host(np.uint8)[:x.shape[0]]

    def decode_grants2(self, iq, tti0, grants, from_grid=False):
        """srslte_hip_dl_rx_batch_grants2: subframe b with grants[b] (DlGrant2: scheme, pmi and a second transport block per subframe).
        Returns (rc, [tb0 rows, tb1 rows], [ok0, ok1]); on a cell without two-layer grants the second entries are None.
        from_grid: iq holds frequency-domain grids [nsf][nof_rx][14 * 12 * nof_prb] (srslte_hip_dl_rx_grid_batch_grants2)."""
        x = np.ascontiguousarray(iq, np.complex64).reshape(-1, self.nof_rx * (14 * 12 * self.cfg.nof_prb if from_grid else self.sf_len))
        n = x.shape[0]
        assert len(grants) == n
        two = self.cfg.nof_ports == 2 and self.cfg.nof_rx_antennas == 2
        arr = (DlGrant2 * n)(*grants)
        din, dtb, dok = DevBuf.from_host(x), DevBuf(self.tb_stride * n * 2), DevBuf(2 * n)
        L = lib()
        fn = L.srslte_hip_dl_rx_grid_batch_grants2 if from_grid else L.srslte_hip_dl_rx_batch_grants2
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        rc = fn(self.h, din.ptr, tti0, n, arr, dtb.ptr, self.tb_stride, dok.ptr, None)
        if rc != SRSLTE_SUCCESS:
            return rc, None, None
        sync()
        tb, ok = dtb.to_host(np.uint8).reshape(2 * n, self.tb_stride), dok.to_host(np.uint8)
        return rc, [tb[:n], tb[n:] if two else None], [ok[:n], ok[n:2 * n] if two else None]

    def decode_harq(self, iq, tti0, rv, new_data):
        """srslte_hip_dl_rx_batch_harq: slot b keeps its soft buffers / CRC flags / bytes between calls."""
        x = np.ascontiguousarray(iq, np.complex64).reshape(-1, self.nof_rx * self.sf_len)
        din = DevBuf.from_host(x)
        lib().srslte_hip_dl_rx_batch_harq.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_uint32,
                                                      C.c_void_p, C.c_void_p]
        _check(lib().srslte_hip_dl_rx_batch_harq(self.h, din.ptr, tti0, x.shape[0], rv, 1 if new_data else 0, self.d_tb.ptr, self.tb_stride,
                                                 self.d_ok.ptr, None), "dl_rx_batch_harq")
        sync()
        tb = self.d_tb.to_host(np.uint8).reshape(self.max_batch, self.tb_stride)[:x.shape[0], :self.tbs // 8 + 3]
        return tb, self.d_ok.to_host(np.uint8)[:x.shape[0]]

    def decode_grid(self, grid, tti0=0):
        """Frequency-domain input [nsf][14*12*nof_prb] (srslte_hip_dl_rx_grid_batch)."""
        x = np.ascontiguousarray(grid, np.complex64)
        x = x.reshape(-1, x.shape[-1])
        din = DevBuf.from_host(x)
        _check(lib().srslte_hip_dl_rx_grid_batch(self.h, din.ptr, tti0, x.shape[0], self.d_tb.ptr, self.tb_stride, self.d_ok.ptr, None), "dl_rx_grid_batch")
        sync()
        tb = self.d_tb.to_host(np.uint8).reshape(self.max_batch, self.tb_stride)[:x.shape[0], :self.tbs // 8 + 3]
        return tb, self.d_ok.to_host(np.uint8)[:x.shape[0]]

    def debug(self, which, dtype, count):
        ptr = lib().srslte_hip_dl_rx_debug_buffer(self.h, which)
        out = np.empty(count, dtype)
        _check(lib().srslte_hip_memcpy_d2h(out.ctypes.data, ptr, out.nbytes), "memcpy_d2h")
        return out

    def free(self):
        if self.h:
            lib().srslte_hip_dl_rx_destroy(self.h)
            self.h = None


class UlRxCfg(C.Structure):
    _fields_ = [("cell_id", C.c_uint32), ("nof_prb", C.c_uint32), ("rnti", C.c_uint16), ("mod", C.c_int), ("tbs", C.c_uint32), ("L_prb", C.c_uint32),
                ("n_prb", C.c_uint32), ("n_dmrs", C.c_uint32), ("max_iterations", C.c_uint32), ("max_batch", C.c_uint32), ("mmse", C.c_int),
                ("dmrs_cfg", DmrsPuschCfg), ("shortened", C.c_int), ("ack_len", C.c_uint32), ("I_offset_ack", C.c_uint32),
                ("ri_len", C.c_uint32), ("I_offset_ri", C.c_uint32), ("cqi_len", C.c_uint32), ("I_offset_cqi", C.c_uint32),
                ("hopping", C.c_uint32), ("n_prb_slot1", C.c_uint32), ("max_grants", C.c_uint32), ("cp_ext", C.c_int)]


class UlGrant(C.Structure):
    """srslte_hip_ul_grant_t: one PUSCH of a srslte_hip_ul_rx_batch_grants call."""
    _fields_ = [("sf", C.c_uint32), ("rnti", C.c_uint16), ("L_prb", C.c_uint32), ("n_prb", C.c_uint32), ("n_prb_slot1", C.c_uint32), ("n_dmrs", C.c_uint32),
                ("mod", C.c_int), ("tbs", C.c_uint32), ("rv", C.c_uint32), ("new_data", C.c_int), ("ack_len", C.c_uint32), ("I_offset_ack", C.c_uint32),
                ("ri_len", C.c_uint32), ("I_offset_ri", C.c_uint32), ("cqi_len", C.c_uint32), ("I_offset_cqi", C.c_uint32)]

    @classmethod
    def make(cls, sf, rnti, L_prb, n_prb, mod, tbs, n_dmrs=0, n_prb_slot1=None, rv=0, new_data=True, ack_len=0, I_offset_ack=0, ri_len=0, I_offset_ri=0,
             cqi_len=0, I_offset_cqi=0):
        return cls(sf, rnti, L_prb, n_prb, n_prb if n_prb_slot1 is None else n_prb_slot1, n_dmrs, mod, tbs, rv, 1 if new_data else 0, ack_len, I_offset_ack,
                   ri_len, I_offset_ri, cqi_len, I_offset_cqi)


class UlRx:
    """Batched PUSCH receive chain (enb_ul.c + pusch.c:423-520 + the UL-SCH part of sch.c:991-1066)."""

    def __init__(self, cell_id, nof_prb, rnti, mod, tbs, L_prb, n_prb, n_dmrs, max_iterations, max_batch, cyclic_shift=0, delta_ss=0,
                 group_hopping=False, sequence_hopping=False, mmse=True, shortened=False, ack_len=0, I_offset_ack=0, ri_len=0, I_offset_ri=0,
                 cqi_len=0, I_offset_cqi=0, n_prb_slot1=None, max_grants=0, cp_ext=False):
        self.cfg = UlRxCfg(cell_id, nof_prb, rnti, mod, tbs, L_prb, n_prb, n_dmrs, max_iterations, max_batch, 1 if mmse else 0,
                           DmrsPuschCfg(cyclic_shift, delta_ss, 1 if group_hopping else 0, 1 if sequence_hopping else 0), 1 if shortened else 0,
                           ack_len, I_offset_ack, ri_len, I_offset_ri, cqi_len, I_offset_cqi, 0 if n_prb_slot1 is None else 1, n_prb_slot1 or 0,
                           max_grants, 1 if cp_ext else 0)
        L = lib()
        L.srslte_hip_ul_rx_ri.restype = C.c_void_p
        L.srslte_hip_ul_rx_ri.argtypes = [C.c_void_p]
        L.srslte_hip_ul_rx_cqi.restype = C.c_void_p
        L.srslte_hip_ul_rx_cqi.argtypes = [C.c_void_p]
        L.srslte_hip_ul_rx_create.restype = C.c_void_p
        L.srslte_hip_ul_rx_create.argtypes = [C.POINTER(UlRxCfg)]
        L.srslte_hip_ul_rx_destroy.argtypes = [C.c_void_p]
        L.srslte_hip_ul_rx_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.srslte_hip_ul_rx_batch_harq.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p,
                                                  C.c_void_p]
        L.srslte_hip_ul_rx_debug_buffer.restype = C.c_void_p
        L.srslte_hip_ul_rx_debug_buffer.argtypes = [C.c_void_p, C.c_int]
        L.srslte_hip_ul_rx_ack.restype = C.c_void_p
        L.srslte_hip_ul_rx_ack.argtypes = [C.c_void_p]
        self.h = L.srslte_hip_ul_rx_create(C.byref(self.cfg))
        if not self.h:
            raise RuntimeError("srslte_hip_ul_rx_create failed")
        self.tbs, self.max_batch = tbs, max_batch
        self.tb_stride = (tbs // 8 + 6 + 15) & ~15
        self.sf_len = 15 * symbol_sz(nof_prb)
        self.rows = max(max_batch, max_grants)
        self.rows_grants = max_grants or max_batch
        self.d_tb, self.d_ok = DevBuf(self.tb_stride * self.rows), DevBuf(self.rows)

    def decode_grants(self, iq, tti0, grants):
        """srslte_hip_ul_rx_batch_grants: grants = list of UlGrant; row p of the result belongs to grants[p]."""
        x = np.ascontiguousarray(iq, np.complex64).reshape(-1, self.sf_len)
        din = DevBuf.from_host(x)
        arr = (UlGrant * len(grants))(*grants)
        L = lib()
        L.srslte_hip_ul_rx_batch_grants.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                                    C.c_void_p]
        _check(L.srslte_hip_ul_rx_batch_grants(self.h, din.ptr, tti0, x.shape[0], arr, len(grants), self.d_tb.ptr, self.tb_stride, self.d_ok.ptr, None),
               "ul_rx_batch_grants")
        sync()
        tb = self.d_tb.to_host(np.uint8).reshape(self.rows, self.tb_stride)[:len(grants)]
        self.last_nof_grants = len(grants)
        return tb, self.d_ok.to_host(np.uint8)[:len(grants)]

    def grants_uci(self):
        """(HARQ-ACK decisions [nof_grants][2], rank indications [nof_grants][2]) of the last decode_grants()."""
        L = lib()
        out = []
        for fn in (L.srslte_hip_ul_rx_grants_ack, L.srslte_hip_ul_rx_grants_ri):
            fn.restype, fn.argtypes = C.c_void_p, [C.c_void_p]
            a = np.empty(2 * self.last_nof_grants, np.uint8)
            _check(L.srslte_hip_memcpy_d2h(a.ctypes.data, fn(self.h), a.nbytes), "memcpy_d2h")
            out.append(a.reshape(-1, 2))
        return out

    def grants_cqi(self):
        """(report bits [nof_grants][64], CRC flags [nof_grants]) of the last decode_grants()."""
        L = lib()
        L.srslte_hip_ul_rx_grants_cqi.restype, L.srslte_hip_ul_rx_grants_cqi.argtypes = C.c_void_p, [C.c_void_p]
        out = np.empty(65 * self.rows_grants, np.uint8)
        _check(L.srslte_hip_memcpy_d2h(out.ctypes.data, L.srslte_hip_ul_rx_grants_cqi(self.h), out.nbytes), "memcpy_d2h")
        n = self.last_nof_grants
        return out[:64 * self.rows_grants].reshape(-1, 64)[:n], out[64 * self.rows_grants:][:n]

    def decode(self, iq, tti0=0):
        x = np.ascontiguousarray(iq, np.complex64).reshape(-1, self.sf_len)
        din = DevBuf.from_host(x)
        _check(lib().srslte_hip_ul_rx_batch(self.h, din.ptr, tti0, x.shape[0], self.d_tb.ptr, self.tb_stride, self.d_ok.ptr, None), "ul_rx_batch")
        sync()
        tb = self.d_tb.to_host(np.uint8).reshape(self.rows, self.tb_stride)[:x.shape[0], :self.tbs // 8 + 3]
        self.last_nof_sf = x.shape[0]
        return tb, self.d_ok.to_host(np.uint8)[:x.shape[0]]

    def decode_harq(self, iq, tti0, rv, new_data):
        """srslte_hip_ul_rx_batch_harq: slot b keeps its soft buffers between calls; new_data starts new transport blocks."""
        x = np.ascontiguousarray(iq, np.complex64).reshape(-1, self.sf_len)
        din = DevBuf.from_host(x)
        _check(lib().srslte_hip_ul_rx_batch_harq(self.h, din.ptr, tti0, x.shape[0], rv, 1 if new_data else 0, self.d_tb.ptr, self.tb_stride,
                                                 self.d_ok.ptr, None), "ul_rx_batch_harq")
        sync()
        tb = self.d_tb.to_host(np.uint8).reshape(self.rows, self.tb_stride)[:x.shape[0], :self.tbs // 8 + 3]
        self.last_nof_sf = x.shape[0]
        return tb, self.d_ok.to_host(np.uint8)[:x.shape[0]]

    def ack(self):
        """HARQ-ACK decisions [nof_sf][2] of the last decode() (srslte_uci_value_t.ack.ack_value of srslte_pusch_decode)."""
        out = np.empty(2 * self.max_batch, np.uint8)
        _check(lib().srslte_hip_memcpy_d2h(out.ctypes.data, lib().srslte_hip_ul_rx_ack(self.h), out.nbytes), "memcpy_d2h")
        return out.reshape(-1, 2)[:self.last_nof_sf, :max(self.cfg.ack_len, 1)]

    def ri(self):
        """Rank-indication decisions [nof_sf][ri_len] of the last decode() (srslte_uci_value_t.ri)."""
        out = np.empty(2 * self.max_batch, np.uint8)
        _check(lib().srslte_hip_memcpy_d2h(out.ctypes.data, lib().srslte_hip_ul_rx_ri(self.h), out.nbytes), "memcpy_d2h")
        return out.reshape(-1, 2)[:self.last_nof_sf, :max(self.cfg.ri_len, 1)]

    def cqi(self):
        """CQI reports of the last decode(): bits [nof_sf][cqi_len] and the CRC flags [nof_sf] (srslte_uci_value_t.cqi, .cqi.data_crc)."""
        out = np.empty(65 * self.max_batch, np.uint8)
        _check(lib().srslte_hip_memcpy_d2h(out.ctypes.data, lib().srslte_hip_ul_rx_cqi(self.h), out.nbytes), "memcpy_d2h")
        n = self.last_nof_sf
        return out[:64 * self.max_batch].reshape(-1, 64)[:n, :self.cfg.cqi_len], out[64 * self.max_batch:][:n]

    def debug(self, which, dtype, count):
        ptr = lib().srslte_hip_ul_rx_debug_buffer(self.h, which)
        out = np.empty(count, dtype)
        _check(lib().srslte_hip_memcpy_d2h(out.ctypes.data, ptr, out.nbytes), "memcpy_d2h")
        return out

    def free(self):
        if self.h:
            lib().srslte_hip_ul_rx_destroy(self.h)
            self.h = None


class UlTxCfg(C.Structure):
    _fields_ = [("cell_id", C.c_uint32), ("nof_prb", C.c_uint32), ("rnti", C.c_uint16), ("mod", C.c_int), ("tbs", C.c_uint32), ("L_prb", C.c_uint32),
                ("n_prb", C.c_uint32), ("n_dmrs", C.c_uint32), ("max_batch", C.c_uint32), ("dmrs_cfg", DmrsPuschCfg), ("shortened", C.c_int),
                ("ack_len", C.c_uint32), ("I_offset_ack", C.c_uint32), ("ri_len", C.c_uint32), ("I_offset_ri", C.c_uint32),
                ("cqi_len", C.c_uint32), ("I_offset_cqi", C.c_uint32), ("hopping", C.c_uint32), ("n_prb_slot1", C.c_uint32), ("max_grants", C.c_uint32),
                ("cp_ext", C.c_int)]


class UlTx:
    """Batched PUSCH transmit chain (srslte_ue_ul_encode ue_ul.c:300-340: srslte_pusch_encode pusch.c:314-421 with the UL-SCH part of
    srslte_ulsch_encode sch.c:1068-1160, DMRS, srslte_ofdm_tx_sf with ue_ul.c:59-64 settings)."""

    def __init__(self, cell_id, nof_prb, rnti, mod, tbs, L_prb, n_prb, n_dmrs, max_batch, cyclic_shift=0, delta_ss=0, group_hopping=False,
                 sequence_hopping=False, shortened=False, ack_len=0, I_offset_ack=0, ri_len=0, I_offset_ri=0, cqi_len=0, I_offset_cqi=0,
                 n_prb_slot1=None, max_grants=0, cp_ext=False):
        self.cfg = UlTxCfg(cell_id, nof_prb, rnti, mod, tbs, L_prb, n_prb, n_dmrs, max_batch,
                           DmrsPuschCfg(cyclic_shift, delta_ss, 1 if group_hopping else 0, 1 if sequence_hopping else 0), 1 if shortened else 0,
                           ack_len, I_offset_ack, ri_len, I_offset_ri, cqi_len, I_offset_cqi, 0 if n_prb_slot1 is None else 1, n_prb_slot1 or 0,
                           max_grants, 1 if cp_ext else 0)
        L = lib()
        L.srslte_hip_ul_tx_batch_uci_cqi.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                                     C.c_void_p, C.c_void_p]
        L.srslte_hip_ul_tx_batch_uci.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.srslte_hip_ul_tx_create.restype = C.c_void_p
        L.srslte_hip_ul_tx_create.argtypes = [C.POINTER(UlTxCfg)]
        L.srslte_hip_ul_tx_destroy.argtypes = [C.c_void_p]
        L.srslte_hip_ul_tx_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.srslte_hip_ul_tx_batch_ack.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.srslte_hip_ul_tx_debug_buffer.restype = C.c_void_p
        L.srslte_hip_ul_tx_debug_buffer.argtypes = [C.c_void_p, C.c_int]
        self.h = L.srslte_hip_ul_tx_create(C.byref(self.cfg))
        if not self.h:
            raise RuntimeError("srslte_hip_ul_tx_create failed")
        self.tbs, self.max_batch = tbs, max_batch
        self.sf_len = 15 * symbol_sz(nof_prb)
        self.d_iq = DevBuf(8 * self.sf_len * max_batch)

    def encode_grants(self, tbs_bytes, tti0, nof_sf, grants, ack=None, ri=None, cqi=None):
        """srslte_hip_ul_tx_batch_grants: grants = list of UlGrant, tbs_bytes[p] the payload of grants[p]; ack / ri: [nof_grants][<= 2] values,
        cqi: [nof_grants][<= 64] report bits (rows of grants without that UCI are ignored) -> iq [nof_sf][sf_len]."""
        n = len(grants)
        stride = (self.tbs // 8 + 15) & ~15
        x = np.zeros((max(n, 1), stride), np.uint8)
        for p_, b in enumerate(tbs_bytes):
            x[p_, :len(b)] = b
        din = DevBuf.from_host(x)
        bufs = []
        for v, w in ((ack, 2), (ri, 2), (cqi, 64)):
            if v is None:
                bufs.append(None)
                continue
            a = np.zeros((max(n, 1), w), np.uint8)
            for p_, row in enumerate(v):
                a[p_, :len(row)] = row
            bufs.append(DevBuf.from_host(a))
        arr = (UlGrant * max(n, 1))(*grants)
        L = lib()
        L.srslte_hip_ul_tx_batch_grants.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                                    C.c_uint32, C.c_void_p, C.c_void_p]
        _check(L.srslte_hip_ul_tx_batch_grants(self.h, din.ptr, stride, *[b.ptr if b else None for b in bufs], tti0, nof_sf, arr, n, self.d_iq.ptr, None),
               "ul_tx_batch_grants")
        sync()
        return self.d_iq.to_host(np.complex64).reshape(self.max_batch, self.sf_len)[:nof_sf]

    def encode(self, tb, tti0=0, ack=None, ri=None, cqi=None, rv=None):
        """tb: [nof_sf][tbs/8] payload bytes (ack: [nof_sf][ack_len] HARQ-ACK values, ri: [nof_sf][ri_len] rank-indication bits,
        cqi: [nof_sf][cqi_len] report bits; rv: redundancy version through srslte_hip_ul_tx_batch_rv) -> iq [nof_sf][sf_len] (left on the
        device in self.d_iq). tbs = 0 (a PUSCH without UL-SCH data): tb is ignored, one subframe per row of cqi."""
        if self.tbs == 0:
            x = np.zeros((len(cqi), 1), np.uint8)
        else:
            x = np.ascontiguousarray(tb, np.uint8).reshape(-1, self.tbs // 8)
        din = DevBuf.from_host(x)
        if rv is not None:
            bufs = []
            for v, n, w in ((ack, self.cfg.ack_len, 2), (ri, self.cfg.ri_len, 2), (cqi, self.cfg.cqi_len, 64)):
                a = np.zeros((x.shape[0], w), np.uint8)
                if v is not None:
                    a[:, :n] = np.asarray(v, np.uint8).reshape(x.shape[0], -1)[:, :n]
                bufs.append(DevBuf.from_host(a) if v is not None else None)
            L = lib()
            L.srslte_hip_ul_tx_batch_rv.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                                    C.c_uint32, C.c_void_p, C.c_void_p]
            _check(L.srslte_hip_ul_tx_batch_rv(self.h, din.ptr, self.tbs // 8, *[b.ptr if b else None for b in bufs], rv, tti0, x.shape[0],
                                               self.d_iq.ptr, None), "ul_tx_batch_rv")
        elif cqi is not None:
            bufs = []
            for v, n, w in ((ack, self.cfg.ack_len, 2), (ri, self.cfg.ri_len, 2), (cqi, self.cfg.cqi_len, 64)):
                a = np.zeros((x.shape[0], w), np.uint8)
                if v is not None:
                    a[:, :n] = np.asarray(v, np.uint8).reshape(x.shape[0], -1)[:, :n]
                bufs.append(DevBuf.from_host(a) if v is not None else None)
            _check(lib().srslte_hip_ul_tx_batch_uci_cqi(self.h, din.ptr, self.tbs // 8, bufs[0].ptr if bufs[0] else None,
                                                        bufs[1].ptr if bufs[1] else None, bufs[2].ptr, tti0, x.shape[0], self.d_iq.ptr, None),
                   "ul_tx_batch_uci_cqi")
        elif ri is not None:
            bufs = []
            for v, n in ((ack, self.cfg.ack_len), (ri, self.cfg.ri_len)):
                a = np.zeros((x.shape[0], 2), np.uint8)
                if v is not None:
                    a[:, :n] = np.asarray(v, np.uint8).reshape(x.shape[0], -1)[:, :n]
                bufs.append(DevBuf.from_host(a) if v is not None else None)
            _check(lib().srslte_hip_ul_tx_batch_uci(self.h, din.ptr, self.tbs // 8, bufs[0].ptr if bufs[0] else None, bufs[1].ptr, tti0, x.shape[0],
                                                    self.d_iq.ptr, None), "ul_tx_batch_uci")
        elif ack is not None:
            a = np.zeros((x.shape[0], 2), np.uint8)
            a[:, :self.cfg.ack_len] = np.asarray(ack, np.uint8).reshape(x.shape[0], -1)[:, :self.cfg.ack_len]
            dack = DevBuf.from_host(a)
            _check(lib().srslte_hip_ul_tx_batch_ack(self.h, din.ptr, self.tbs // 8, dack.ptr, tti0, x.shape[0], self.d_iq.ptr, None), "ul_tx_batch_ack")
        else:
            _check(lib().srslte_hip_ul_tx_batch(self.h, din.ptr, self.tbs // 8, tti0, x.shape[0], self.d_iq.ptr, None), "ul_tx_batch")
        sync()
        return self.d_iq.to_host(np.complex64).reshape(self.max_batch, self.sf_len)[:x.shape[0]]

    def debug(self, which, dtype, count):
        ptr = lib().srslte_hip_ul_tx_debug_buffer(self.h, which)
        out = np.empty(count, dtype)
        _check(lib().srslte_hip_memcpy_d2h(out.ctypes.data, ptr, out.nbytes), "memcpy_d2h")
        return out

    def free(self):
        if self.h:
            lib().srslte_hip_ul_tx_destroy(self.h)
            self.h = None


class DlTxCfg(C.Structure):
    _fields_ = [("cell_id", C.c_uint32), ("nof_prb", C.c_uint32), ("cfi", C.c_uint32), ("rnti", C.c_uint16), ("mod", C.c_int), ("tbs", C.c_uint32),
                ("max_batch", C.c_uint32), ("nof_ports", C.c_uint32), ("p_a", C.c_float), ("max_grants", C.c_uint32), ("cp_ext", C.c_int),
                ("tdd", C.c_int), ("tdd_sf_config", C.c_uint32), ("tdd_ss_config", C.c_uint32),
                ("mbsfn", C.c_int), ("mbsfn_area_id", C.c_uint32), ("non_mbsfn_region", C.c_uint32)]


class DlTxGrant2(C.Structure):
    """srslte_hip_dl_tx_grant2_t: the subframe of the batch and the grant as the receive side takes it (DlGrant2)."""
    _fields_ = [("sf", C.c_uint32), ("grant", DlGrant2)]


class DlTx:
    """Batched PDSCH transmit chain (srslte_pdsch_encode pdsch.c:1059-1185 + CRS + srslte_ofdm_tx_sf, enb_dl.c)."""

    def __init__(self, cell_id, nof_prb, cfi, rnti, mod, tbs, max_batch, nof_ports=1, p_a=0.0, max_grants=0, cp_ext=False, tdd=None, mbsfn=None):
        self.cfg = DlTxCfg(cell_id, nof_prb, cfi, rnti, mod, tbs, max_batch, nof_ports, p_a, max_grants, 1 if cp_ext else 0,
                           1 if tdd else 0, tdd[0] if tdd else 0, tdd[1] if tdd else 0, 1 if mbsfn else 0, mbsfn[0] if mbsfn else 0, mbsfn[1] if mbsfn else 0)
        L = lib()
        L.srslte_hip_dl_tx_create.restype = C.c_void_p
        L.srslte_hip_dl_tx_create.argtypes = [C.POINTER(DlTxCfg)]
        L.srslte_hip_dl_tx_destroy.argtypes = [C.c_void_p]
        L.srslte_hip_dl_tx_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.srslte_hip_dl_tx_debug_buffer.restype = C.c_void_p
        L.srslte_hip_dl_tx_debug_buffer.argtypes = [C.c_void_p, C.c_int]
        self.h = L.srslte_hip_dl_tx_create(C.byref(self.cfg))
        if not self.h:
            raise RuntimeError("srslte_hip_dl_tx_create failed")
        self.tbs, self.max_batch, self.nof_ports = tbs, max_batch, max(1, nof_ports)
        self.sf_len = 15 * symbol_sz(nof_prb)
        self.d_iq = DevBuf(8 * self.sf_len * max_batch * self.nof_ports)

    def encode_grants(self, tbs_bytes, tti0, nof_sf, grants):
        """srslte_hip_dl_tx_batch_grants: grants = list of (sf, DlGrant); tbs_bytes[p] = the payload of grants[p] -> iq [nof_sf][nof_ports][sf_len]."""
        class TxGrant(C.Structure):
            _fields_ = [("sf", C.c_uint32), ("grant", DlGrant)]
        stride = (self.tbs // 8 + 15) & ~15
        x = np.zeros((len(grants), stride), np.uint8)
        for p_, b in enumerate(tbs_bytes):
            x[p_, :len(b)] = b
        din = DevBuf.from_host(x)
        arr = (TxGrant * max(1, len(grants)))(*[TxGrant(sf, g) for sf, g in grants])
        L = lib()
        L.srslte_hip_dl_tx_batch_grants.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        _check(L.srslte_hip_dl_tx_batch_grants(self.h, din.ptr, stride, tti0, nof_sf, arr, len(grants), self.d_iq.ptr, None), "dl_tx_batch_grants")
        sync()
        return self.d_iq.to_host(np.complex64).reshape(self.max_batch, self.nof_ports, self.sf_len)[:nof_sf]

    def encode(self, tb, tti0=0, rv=0):
        """tb: [nof_sf][tbs/8] payload bytes -> iq [nof_sf][nof_ports][sf_len]."""
        x = np.ascontiguousarray(tb, np.uint8).reshape(-1, self.tbs // 8)
        din = DevBuf.from_host(x)
        _check(lib().srslte_hip_dl_tx_batch(self.h, din.ptr, self.tbs // 8, tti0, x.shape[0], rv, self.d_iq.ptr, None), "dl_tx_batch")
        sync()
        return self.d_iq.to_host(np.complex64).reshape(self.max_batch, self.nof_ports, self.sf_len)[:x.shape[0]]

    def encode_grants_ctrl(self, tbs_bytes, tti0, nof_sf, grants, ctrl, cfi, dcis=(), phichs=()):
        """srslte_hip_dl_tx_batch_grants_ctrl: encode_grants with the control region of ctrl (a DlCtrlTx of the same cell) - cfi [nof_sf], dcis and
        phichs as DlCtrlTx.put takes them - on the grids before the OFDM modulation -> (rc, iq [nof_sf][nof_ports][sf_len] or None)."""
        return self._encode_grants_with(lib().srslte_hip_dl_tx_batch_grants_ctrl, tbs_bytes, tti0, nof_sf, grants, ctrl, cfi, dcis, phichs)

    def encode_grants_full(self, tbs_bytes, tti0, nof_sf, grants, ctrl, cfi, dcis=(), phichs=()):
        """srslte_hip_dl_tx_batch_grants_full: encode_grants_ctrl with ctrl's PSS / SSS / PBCH put before the PDSCHs, a complete FDD subframe per
        TTI -> (rc, iq [nof_sf][nof_ports][sf_len] or None)."""
        return self._encode_grants_with(lib().srslte_hip_dl_tx_batch_grants_full, tbs_bytes, tti0, nof_sf, grants, ctrl, cfi, dcis, phichs)

    def _encode_grants_with(self, fn, tbs_bytes, tti0, nof_sf, grants, ctrl, cfi, dcis, phichs):
        class TxGrant(C.Structure):
            _fields_ = [("sf", C.c_uint32), ("grant", DlGrant)]
        stride = (self.tbs // 8 + 15) & ~15
        x = np.zeros((max(1, len(grants)), stride), np.uint8)
        for p_, b in enumerate(tbs_bytes):
            x[p_, :len(b)] = b
        din = DevBuf.from_host(x)
        arr = (TxGrant * max(1, len(grants)))(*[TxGrant(sf, g) for sf, g in grants])
        inp, keep = _ctrl_tx_in(cfi, dcis, phichs)
        _bind_dl_ctrl_tx(lib())
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(DlCtrlTxIn), C.c_void_p,
                       C.c_void_p]
        rc = fn(self.h, din.ptr, stride, tti0, nof_sf, arr, len(grants), ctrl.h, C.byref(inp), self.d_iq.ptr, None)
        if rc != SRSLTE_SUCCESS:
            return rc, None
        sync()
        return rc, self.d_iq.to_host(np.complex64).reshape(self.max_batch, self.nof_ports, self.sf_len)[:nof_sf]

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
        arr = (DlTxGrant2 * max(1, n))(*[DlTxGrant2(sf, g) for sf, g in grants])
        fn = lib().srslte_hip_dl_tx_batch_grants2
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        rc = fn(self.h, din.ptr, stride, tti0, nof_sf, arr, n, self.d_iq.ptr, None)
        if rc != SRSLTE_SUCCESS:
            return rc, None
        sync()
        return rc, self.d_iq.to_host(np.complex64).reshape(self.max_batch, self.nof_ports, self.sf_len)[:nof_sf]

    def encode_grants2_ctrl(self, tbs_bytes, tti0, nof_sf, grants, ctrl, cfi, dcis=(), phichs=()):
        """srslte_hip_dl_tx_batch_grants2_ctrl: encode_grants2 with the control region of ctrl, as encode_grants_ctrl."""
        return self._encode_grants2_with(lib().srslte_hip_dl_tx_batch_grants2_ctrl, tbs_bytes, tti0, nof_sf, grants, ctrl, cfi, dcis, phichs)

    def encode_grants2_full(self, tbs_bytes, tti0, nof_sf, grants, ctrl, cfi, dcis=(), phichs=()):
        """srslte_hip_dl_tx_batch_grants2_full: encode_grants2_ctrl with ctrl's PSS / SSS / PBCH, as encode_grants_full."""
        return self._encode_grants2_with(lib().srslte_hip_dl_tx_batch_grants2_full, tbs_bytes, tti0, nof_sf, grants, ctrl, cfi, dcis, phichs)

    def _encode_grants2_with(self, fn, tbs_bytes, tti0, nof_sf, grants, ctrl, cfi, dcis, phichs):
        n = len(grants)
        din, stride = self._tb_rows2(tbs_bytes, n)
        arr = (DlTxGrant2 * max(1, n))(*[DlTxGrant2(sf, g) for sf, g in grants])
        inp, keep = _ctrl_tx_in(cfi, dcis, phichs)
        _bind_dl_ctrl_tx(lib())
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(DlCtrlTxIn), C.c_void_p,
                       C.c_void_p]
        rc = fn(self.h, din.ptr, stride, tti0, nof_sf, arr, n, ctrl.h, C.byref(inp), self.d_iq.ptr, None)
        if rc != SRSLTE_SUCCESS:
            return rc, None
        sync()
        return rc, self.d_iq.to_host(np.complex64).reshape(self.max_batch, self.nof_ports, self.sf_len)[:nof_sf]

    def debug(self, which, dtype, count):
        ptr = lib().srslte_hip_dl_tx_debug_buffer(self.h, which)
        out = np.empty(count, dtype)
        _check(lib().srslte_hip_memcpy_d2h(out.ctypes.data, ptr, out.nbytes), "memcpy_d2h")
        return out

    def free(self):
        if self.h:
            lib().srslte_hip_dl_tx_destroy(self.h)
            self.h = None


# ---------------------------------------------------------------- DL control region receive (phy_hip.h "DL control region receive")
DCI_FORMAT0, DCI_FORMAT1, DCI_FORMAT1A, DCI_FORMAT1C, DCI_FORMAT1B, DCI_FORMAT1D, DCI_FORMAT2, DCI_FORMAT2A, DCI_FORMAT2B = range(9)  # srslte_dci_format_t
DL_CTRL_MAX_CAND = 38


class DlCtrlCfg(C.Structure):
    """srslte_hip_dl_ctrl_cfg_t: the cell (srslte_cell_t) and the object's batch size."""
    _fields_ = [("nof_prb", C.c_uint32), ("nof_ports", C.c_uint32), ("cell_id", C.c_uint32), ("cp_ext", C.c_int), ("phich_resources", C.c_int),
                ("phich_ext", C.c_int), ("tdd", C.c_int), ("nof_rx_antennas", C.c_uint32), ("max_batch", C.c_uint32)]


class DlCtrlReq(C.Structure):
    """srslte_hip_dl_ctrl_req_t: RNTI, srslte_tm_t (0-3), CFI (0 = from the PCFICH) and the MBSFN flag of one subframe."""
    _fields_ = [("rnti", C.c_uint16), ("tm", C.c_uint32), ("cfi", C.c_uint32), ("mbsfn", C.c_int)]


class DlCtrlRes(C.Structure):
    """srslte_hip_dl_ctrl_res_t."""
    _fields_ = [("cfi", C.c_uint32), ("cfi_corr", C.c_float), ("nof_dci", C.c_uint32)]


class DciMsg(C.Structure):
    """srslte_hip_dci_msg_t = srslte_dci_msg_t (dci.h:65-71)."""
    _fields_ = [("payload", C.c_uint8 * 128), ("nof_bits", C.c_uint32), ("L", C.c_uint32), ("ncce", C.c_uint32), ("format", C.c_int), ("rnti", C.c_uint16)]


class DlCtrlCand(C.Structure):
    """srslte_hip_dl_ctrl_cand_t: one searched candidate."""
    _fields_ = [("L", C.c_uint32), ("ncce", C.c_uint32), ("format", C.c_uint32), ("nof_bits", C.c_uint32), ("skipped", C.c_uint32), ("crc_rem", C.c_uint32),
                ("format_decoded", C.c_uint32), ("payload", C.c_uint8 * 128)]


DL_CTRL_MAX_UL_DCI = 5


class DlCtrlUlRes(C.Structure):
    """srslte_hip_dl_ctrl_ul_res_t: the UL DCIs of one subframe; pending = 1 if they are the DL search's pending list."""
    _fields_ = [("nof_ul_dci", C.c_uint32), ("pending", C.c_uint32)]


class PhichReq(C.Structure):
    """srslte_hip_phich_req_t: the srslte_phich_grant_t of the PUSCH a PHICH acknowledges, with its subframe within the batch."""
    _fields_ = [("sf", C.c_uint32), ("n_prb_lowest", C.c_uint32), ("n_dmrs", C.c_uint32), ("I_phich", C.c_uint32)]


class PhichRes(C.Structure):
    """srslte_hip_phich_res_t: srslte_phich_res_t and the srslte_phich_resource_t it was read from."""
    _fields_ = [("ack_value", C.c_uint32), ("distance", C.c_float), ("ngroup", C.c_uint32), ("nseq", C.c_uint32)]


class PhichSoft(C.Structure):
    """srslte_hip_phich_soft_t: z after de-spreading (re, im) and the three BPSK soft bits of one PHICH."""
    _fields_ = [("z", (C.c_float * 2) * 3), ("bits", C.c_float * 3)]


def _bind_dl_ctrl(L):
    vp = C.c_void_p
    L.srslte_hip_dl_ctrl_set_max_phich.argtypes = [vp, C.c_uint32]
    L.srslte_hip_dl_ctrl_batch_ul.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, C.c_uint32, vp, vp]
    L.srslte_hip_dl_ctrl_phich_batch.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, vp]
    L.srslte_hip_dl_ctrl_phich_debug_buffer.restype = vp
    L.srslte_hip_dl_ctrl_phich_debug_buffer.argtypes = [vp]
    L.srslte_hip_dl_ctrl_create.restype = vp
    L.srslte_hip_dl_ctrl_create.argtypes = [C.POINTER(DlCtrlCfg)]
    L.srslte_hip_dl_ctrl_destroy.argtypes = [vp]
    L.srslte_hip_dl_ctrl_batch.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp]
    L.srslte_hip_dl_ctrl_debug_buffer.restype = vp
    L.srslte_hip_dl_ctrl_debug_buffer.argtypes = [vp, C.c_int]
    L.srslte_hip_dl_ctrl_llr_stride.restype = C.c_uint32
    L.srslte_hip_dl_ctrl_llr_stride.argtypes = [vp]
    L.srslte_hip_dl_ctrl_pcfich_re.argtypes = [C.POINTER(DlCtrlCfg), vp, C.c_uint32]
    L.srslte_hip_dl_ctrl_pdcch_re.argtypes = [C.POINTER(DlCtrlCfg), C.c_uint32, vp, C.c_uint32]
    L.srslte_hip_pdcch_ue_locations_ncce.restype = C.c_uint32
    L.srslte_hip_pdcch_ue_locations_ncce.argtypes = [C.c_uint32, vp, C.c_uint32, C.c_uint32, C.c_uint16]
    L.srslte_hip_pdcch_common_locations_ncce.restype = C.c_uint32
    L.srslte_hip_pdcch_common_locations_ncce.argtypes = [C.c_uint32, vp, C.c_uint32]
    L.srslte_hip_dci_format_sizeof.restype = C.c_uint32
    L.srslte_hip_dci_format_sizeof.argtypes = [C.c_uint32, C.c_uint32, C.c_int]
    L.srslte_hip_dl_ctrl_mib_batch.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_int, vp, vp]
    L.srslte_hip_dl_ctrl_mib_debug_buffer.restype = vp
    L.srslte_hip_dl_ctrl_mib_debug_buffer.argtypes = [vp, C.c_int]
    L.srslte_hip_pbch_re.argtypes = [C.POINTER(DlCtrlCfg), vp, C.c_uint32]
    L.srslte_hip_sync_re.argtypes = [C.POINTER(DlCtrlCfg), C.c_uint32, vp, vp, C.c_uint32]
    L.srslte_hip_pbch_mib_pack.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_uint32, vp]
    return L


def _ctrl_cfg(nof_prb, nof_ports, cell_id, cp_ext=False, phich_resources=0, phich_ext=False, nof_rx=1, max_batch=1, tdd=False):
    return DlCtrlCfg(nof_prb, nof_ports, cell_id, 1 if cp_ext else 0, phich_resources, 1 if phich_ext else 0, 1 if tdd else 0, nof_rx, max_batch)


def pcfich_re(nof_prb, nof_ports, cell_id, cp_ext=False, phich_resources=0, phich_ext=False):
    """The 16 PCFICH REs as indices into one antenna's [nsym][12 nof_prb] grid, in srslte_regs_pcfich_get's order (host; no GPU)."""
    L = _bind_dl_ctrl(lib())
    out = np.zeros(16, np.uint32)
    n = L.srslte_hip_dl_ctrl_pcfich_re(C.byref(_ctrl_cfg(nof_prb, nof_ports, cell_id, cp_ext, phich_resources, phich_ext)), out.ctypes.data, 16)
    if n < 0:
        raise ValueError("srslte_hip_dl_ctrl_pcfich_re: %d" % n)
    return out[:n]


def pdcch_re(nof_prb, nof_ports, cell_id, cfi, cp_ext=False, phich_resources=0, phich_ext=False):
    """The 36 NOF_CCE(cfi) PDCCH REs in srslte_regs_pdcch_get's order (host; no GPU)."""
    L = _bind_dl_ctrl(lib())
    out = np.zeros(14 * 12 * 110, np.uint32)
    n = L.srslte_hip_dl_ctrl_pdcch_re(C.byref(_ctrl_cfg(nof_prb, nof_ports, cell_id, cp_ext, phich_resources, phich_ext)), cfi, out.ctypes.data, out.size)
    if n < 0:
        raise ValueError("srslte_hip_dl_ctrl_pdcch_re: %d" % n)
    return out[:n]


def pdcch_ue_locations(nof_cce, sf_idx, rnti, max_candidates=16):
    """srslte_pdcch_ue_locations_ncce -> [(L, ncce), ...] (host)."""
    loc = np.zeros(2 * max_candidates, np.uint32)
    k = _bind_dl_ctrl(lib()).srslte_hip_pdcch_ue_locations_ncce(nof_cce, loc.ctypes.data, max_candidates, sf_idx, rnti)
    return [(int(loc[2 * i]), int(loc[2 * i + 1])) for i in range(k)]


def pdcch_common_locations(nof_cce, max_candidates=6):
    """srslte_pdcch_common_locations_ncce -> [(L, ncce), ...] (host)."""
    loc = np.zeros(2 * max_candidates, np.uint32)
    k = _bind_dl_ctrl(lib()).srslte_hip_pdcch_common_locations_ncce(nof_cce, loc.ctypes.data, max_candidates)
    return [(int(loc[2 * i]), int(loc[2 * i + 1])) for i in range(k)]


def dci_format_sizeof(nof_prb, nof_ports, fmt):
    """srslte_dci_format_sizeof for an FDD cell with a zero srslte_dci_cfg_t (host)."""
    return _bind_dl_ctrl(lib()).srslte_hip_dci_format_sizeof(nof_prb, nof_ports, fmt)


class MibRes(C.Structure):
    """srslte_hip_mib_res_t: the MIB of one subframe."""
    _fields_ = [("found", C.c_uint32), ("nof_tx_ports", C.c_uint32), ("sfn_offset", C.c_int32), ("nof_prb", C.c_uint32), ("phich_ext", C.c_uint32),
                ("phich_resources", C.c_uint32), ("sfn", C.c_uint32), ("payload", C.c_uint8 * 24)]


class MibCand(C.Structure):
    """srslte_hip_mib_cand_t: one decode_frame of the MIB decoder."""
    _fields_ = [("nant", C.c_uint32), ("dst", C.c_uint32), ("hit", C.c_uint32), ("data", C.c_uint8 * 40)]


def pbch_re(nof_prb, nof_ports, cell_id, cp_ext=False):
    """The PBCH REs of one port's subframe grid in srslte_pbch_put's order (host; no GPU)."""
    out = np.zeros(240, np.uint32)
    n = _bind_dl_ctrl(lib()).srslte_hip_pbch_re(C.byref(_ctrl_cfg(nof_prb, nof_ports, cell_id, cp_ext)), out.ctypes.data, out.size)
    if n < 0:
        raise ValueError("srslte_hip_pbch_re: %d" % n)
    return out[:n]


def sync_re(nof_prb, cell_id, sf_idx, cp_ext=False):
    """The 72 PSS then 72 SSS REs of subframe sf_idx (0 / 5) with the zero guards -> (re [144] uint32, values [144] complex64) (host)."""
    re, val = np.zeros(144, np.uint32), np.zeros(144, np.complex64)
    n = _bind_dl_ctrl(lib()).srslte_hip_sync_re(C.byref(_ctrl_cfg(nof_prb, 1, cell_id, cp_ext)), sf_idx, re.ctypes.data, val.ctypes.data, 144)
    if n < 0:
        raise ValueError("srslte_hip_sync_re: %d" % n)
    return re, val


def mib_pack(nof_prb, phich_ext, phich_resources, sfn):
    """srslte_pbch_mib_pack -> 24 bits (uint8) (host)."""
    out = np.zeros(24, np.uint8)
    n = _bind_dl_ctrl(lib()).srslte_hip_pbch_mib_pack(nof_prb, 1 if phich_ext else 0, phich_resources, sfn, out.ctypes.data)
    if n < 0:
        raise ValueError("srslte_hip_pbch_mib_pack: %d" % n)
    return out


def _phich_reqs(phichs):
    """PhichReq or (sf, n_prb_lowest, n_dmrs, I_phich) -> a ctypes array (one dummy entry when empty)."""
    return (PhichReq * max(1, len(phichs)))(*[x if isinstance(x, PhichReq) else PhichReq(*x) for x in phichs])


class DlCtrl:
    """Batched control-region receive: srslte_pcfich_decode + srslte_pdcch_extract_llr + the DL DCI blind search of srslte_ue_dl_find_dl_dci;
    with batch_ul / phich also srslte_ue_dl_find_ul_dci and srslte_ue_dl_decode_phich (max_phich: PHICH requests per call)."""

    def __init__(self, nof_prb, nof_ports, cell_id, cp_ext=False, phich_resources=0, phich_ext=False, nof_rx=1, max_batch=1, tdd=False, max_phich=0):
        L = _bind_dl_ctrl(lib())
        self.cfg = _ctrl_cfg(nof_prb, nof_ports, cell_id, cp_ext, phich_resources, phich_ext, nof_rx, max_batch, tdd)
        self.h = L.srslte_hip_dl_ctrl_create(C.byref(self.cfg))
        if not self.h:
            raise RuntimeError("srslte_hip_dl_ctrl_create failed")
        self.grid_len = (12 if cp_ext else 14) * 12 * nof_prb
        self.nof_ports, self.nof_rx, self.max_batch = nof_ports, nof_rx, max_batch
        self.llr_stride = L.srslte_hip_dl_ctrl_llr_stride(self.h)
        if max_phich:
            self.set_max_phich(max_phich)

    def set_max_phich(self, max_phich):
        """srslte_hip_dl_ctrl_set_max_phich: room for max_phich PHICH requests per call (waits for the device)."""
        _check(lib().srslte_hip_dl_ctrl_set_max_phich(self.h, max_phich), "srslte_hip_dl_ctrl_set_max_phich")

    def batch_ul_device(self, d_grid, d_ce, d_res, tti0, reqs, d_out, d_msg, d_ul_out, d_ul_msg, phichs=(), d_phich_res=None, stream=None):
        """srslte_hip_dl_ctrl_batch_ul on device pointers; reqs: list of DlCtrlReq, phichs: PhichReq or tuples. Returns the status code."""
        arr = (DlCtrlReq * max(1, len(reqs)))(*reqs)
        return lib().srslte_hip_dl_ctrl_batch_ul(self.h, d_grid, d_ce, d_res, tti0, len(reqs), arr, d_out, d_msg, d_ul_out, d_ul_msg,
                                                 _phich_reqs(phichs) if len(phichs) else None, len(phichs), d_phich_res, stream)

    def phich_device(self, d_grid, d_ce, d_res, tti0, nof_sf, phichs, d_phich_res, stream=None):
        """srslte_hip_dl_ctrl_phich_batch on device pointers -> the status code."""
        return lib().srslte_hip_dl_ctrl_phich_batch(self.h, d_grid, d_ce, d_res, tti0, nof_sf, _phich_reqs(phichs) if len(phichs) else None,
                                                    len(phichs), d_phich_res, stream)

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
        out, msg, ul, ulm, ph = (DlCtrlRes * n)(), (DciMsg * n)(), (DlCtrlUlRes * n)(), (DciMsg * (n * DL_CTRL_MAX_UL_DCI))(), (PhichRes * max(1, m))()
        for dst, src in ((out, dout), (msg, dmsg), (ul, dul), (ulm, dulm), (ph, dph)):
            _check(lib().srslte_hip_memcpy_d2h(C.addressof(dst), src.ptr, C.sizeof(dst)), "memcpy_d2h")
        ul_msgs = [list(ulm[b * DL_CTRL_MAX_UL_DCI:b * DL_CTRL_MAX_UL_DCI + ul[b].nof_ul_dci]) for b in range(n)]
        return rc, list(out), list(msg), list(ul), ul_msgs, list(ph)[:m]

    def phich(self, grid, ce, res, tti0, phichs):
        """srslte_hip_dl_ctrl_phich_batch: grid, ce, res as batch takes them -> (rc, [PhichRes] or None)."""
        n, m = len(res), len(phichs)
        dg, dh, dr = self._upload(n, grid, ce, res)
        dph = DevBuf(C.sizeof(PhichRes) * max(1, m))
        rc = self.phich_device(dg.ptr, dh.ptr, dr.ptr, tti0, n, phichs, dph.ptr)
        if rc != SRSLTE_SUCCESS:
            return rc, None
        sync()
        ph = (PhichRes * max(1, m))()
        _check(lib().srslte_hip_memcpy_d2h(C.addressof(ph), dph.ptr, C.sizeof(ph)), "memcpy_d2h")
        return rc, list(ph)[:m]

    def phich_soft(self, nof_phich):
        """The PHICH debug buffer of the last call: [PhichSoft] (z after de-spreading and the soft bits of each request)."""
        out = (PhichSoft * max(1, nof_phich))()
        ptr = lib().srslte_hip_dl_ctrl_phich_debug_buffer(self.h)
        if nof_phich:
            _check(lib().srslte_hip_memcpy_d2h(C.addressof(out), ptr, C.sizeof(PhichSoft) * nof_phich), "memcpy_d2h")
        return list(out)[:nof_phich]

    def run_device(self, d_grid, d_ce, d_res, tti0, reqs, d_out, d_msg, stream=None):
        """Device pointers in and out; reqs: list of DlCtrlReq. Returns the status code."""
        arr = (DlCtrlReq * max(1, len(reqs)))(*reqs)
        return lib().srslte_hip_dl_ctrl_batch(self.h, d_grid, d_ce, d_res, tti0, len(reqs), arr, d_out, d_msg, stream)

    def batch(self, grid, ce, res, tti0, reqs):
        """grid [nof_sf][nof_rx][grid_len], ce [nof_sf][nof_ports][nof_rx][grid_len] (complex64), res [nof_sf][10] float32 (srslte_hip_chest_dl_res_t)
        -> (rc, [DlCtrlRes], [DciMsg])."""
        n = len(reqs)
        g = np.ascontiguousarray(grid, np.complex64).reshape(n, self.nof_rx, self.grid_len)
        h = np.ascontiguousarray(ce, np.complex64).reshape(n, self.nof_ports, self.nof_rx, self.grid_len)
        r = np.ascontiguousarray(res, np.float32).reshape(n, 10)
        dg, dh, dr = DevBuf.from_host(g), DevBuf.from_host(h), DevBuf.from_host(r)
        dout, dmsg = DevBuf(C.sizeof(DlCtrlRes) * n), DevBuf(C.sizeof(DciMsg) * n)
        rc = self.run_device(dg.ptr, dh.ptr, dr.ptr, tti0, reqs, dout.ptr, dmsg.ptr)
        if rc != SRSLTE_SUCCESS:
            return rc, None, None
        sync()
        out, msg = (DlCtrlRes * n)(), (DciMsg * n)()
        _check(lib().srslte_hip_memcpy_d2h(C.addressof(out), dout.ptr, C.sizeof(out)), "memcpy_d2h")
        _check(lib().srslte_hip_memcpy_d2h(C.addressof(msg), dmsg.ptr, C.sizeof(msg)), "memcpy_d2h")
        return rc, list(out), list(msg)

    def llr(self, nof_sf):
        """Debug buffer 0: the LLR rows of the last call, [nof_sf][llr_stride] float32."""
        ptr = lib().srslte_hip_dl_ctrl_debug_buffer(self.h, 0)
        out = np.empty(nof_sf * self.llr_stride, np.float32)
        _check(lib().srslte_hip_memcpy_d2h(out.ctypes.data, ptr, out.nbytes), "memcpy_d2h")
        return out.reshape(nof_sf, self.llr_stride)

    def candidates(self, nof_sf):
        """Debug buffers 1 and 2: for each subframe of the last call the list of DlCtrlCand in search order."""
        L = lib()
        cand = (DlCtrlCand * (nof_sf * DL_CTRL_MAX_CAND))()
        cnt = np.empty(nof_sf, np.uint32)
        _check(L.srslte_hip_memcpy_d2h(C.addressof(cand), L.srslte_hip_dl_ctrl_debug_buffer(self.h, 1), C.sizeof(cand)), "memcpy_d2h")
        _check(L.srslte_hip_memcpy_d2h(cnt.ctypes.data, L.srslte_hip_dl_ctrl_debug_buffer(self.h, 2), cnt.nbytes), "memcpy_d2h")
        return [list(cand[b * DL_CTRL_MAX_CAND:b * DL_CTRL_MAX_CAND + int(cnt[b])]) for b in range(nof_sf)]

    def decode_mib_device(self, d_grid, d_ce, d_res, tti0, nof_sf, search_all_ports, d_mib, stream=None):
        """srslte_hip_dl_ctrl_mib_batch on device pointers -> the status code."""
        return lib().srslte_hip_dl_ctrl_mib_batch(self.h, d_grid, d_ce, d_res, tti0, nof_sf, 1 if search_all_ports else 0, d_mib, stream)

    def decode_mib(self, grid, ce, res, tti0, search_all_ports=True):
        """srslte_hip_dl_ctrl_mib_batch: grid, ce, res as batch takes them -> (rc, [MibRes] or None)."""
        n = len(res)
        g = np.ascontiguousarray(grid, np.complex64).reshape(n, self.nof_rx, self.grid_len)
        h = np.ascontiguousarray(ce, np.complex64).reshape(n, self.nof_ports, self.nof_rx, self.grid_len)
        r = np.ascontiguousarray(res, np.float32).reshape(n, 10)
        dg, dh, dr, dm = DevBuf.from_host(g), DevBuf.from_host(h), DevBuf.from_host(r), DevBuf(C.sizeof(MibRes) * n)
        rc = self.decode_mib_device(dg.ptr, dh.ptr, dr.ptr, tti0, n, search_all_ports, dm.ptr)
        if rc != SRSLTE_SUCCESS:
            return rc, None
        sync()
        out = (MibRes * n)()
        _check(lib().srslte_hip_memcpy_d2h(C.addressof(out), dm.ptr, C.sizeof(out)), "memcpy_d2h")
        return rc, list(out)

    def mib_llr(self, nof_sf):
        """MIB debug buffer 0: [nof_sf][3][480] float32, rows of nant 1, 2, 4."""
        out = np.empty(nof_sf * 3 * 480, np.float32)
        _check(lib().srslte_hip_memcpy_d2h(out.ctypes.data, lib().srslte_hip_dl_ctrl_mib_debug_buffer(self.h, 0), out.nbytes), "memcpy_d2h")
        return out.reshape(nof_sf, 3, 480)

    def mib_candidates(self, nof_sf):
        """MIB debug buffer 1: [nof_sf][3][4] MibCand (nant 1, 2, 4; dst 0-3)."""
        cand = (MibCand * (nof_sf * 12))()
        _check(lib().srslte_hip_memcpy_d2h(C.addressof(cand), lib().srslte_hip_dl_ctrl_mib_debug_buffer(self.h, 1), C.sizeof(cand)), "memcpy_d2h")
        return [[list(cand[(b * 3 + s) * 4:(b * 3 + s) * 4 + 4]) for s in range(3)] for b in range(nof_sf)]

    def free(self):
        if self.h:
            lib().srslte_hip_dl_ctrl_destroy(self.h)
            self.h = None


# ---------------------------------------------------------------- DL control region transmit (phy_hip.h "DL control region transmit")
class DlCtrlTxCfg(C.Structure):
    """srslte_hip_dl_ctrl_tx_cfg_t: the cell and the per-call limits."""
    _fields_ = [("nof_prb", C.c_uint32), ("nof_ports", C.c_uint32), ("cell_id", C.c_uint32), ("cp_ext", C.c_int), ("phich_resources", C.c_int),
                ("phich_ext", C.c_int), ("tdd", C.c_int), ("max_batch", C.c_uint32), ("max_dci", C.c_uint32), ("max_phich", C.c_uint32)]


class DlCtrlTxDci(C.Structure):
    """srslte_hip_dl_ctrl_tx_dci_t: a DCI message and its subframe within the batch."""
    _fields_ = [("sf", C.c_uint32), ("msg", DciMsg)]


class PhichTx(C.Structure):
    """srslte_hip_phich_tx_t: srslte_phich_grant_t and the ack of one PHICH, with its subframe within the batch."""
    _fields_ = [("sf", C.c_uint32), ("n_prb_lowest", C.c_uint32), ("n_dmrs", C.c_uint32), ("I_phich", C.c_uint32), ("ack", C.c_uint8)]


class DlCtrlTxIn(C.Structure):
    """srslte_hip_dl_ctrl_tx_in_t."""
    _fields_ = [("cfi", C.c_void_p), ("dci", C.POINTER(DlCtrlTxDci)), ("nof_dci", C.c_uint32), ("phich", C.POINTER(PhichTx)), ("nof_phich", C.c_uint32)]


def _bind_dl_ctrl_tx(L):
    vp = C.c_void_p
    L.srslte_hip_dl_ctrl_tx_create.restype = vp
    L.srslte_hip_dl_ctrl_tx_create.argtypes = [C.POINTER(DlCtrlTxCfg)]
    L.srslte_hip_dl_ctrl_tx_destroy.argtypes = [vp]
    L.srslte_hip_dl_ctrl_tx_put.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(DlCtrlTxIn), vp, vp]
    L.srslte_hip_dl_ctrl_tx_put_bcast.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp]
    L.srslte_hip_dl_ctrl_phich_ngroups.argtypes = [C.POINTER(DlCtrlTxCfg)]
    L.srslte_hip_phich_calc.argtypes = [C.POINTER(DlCtrlTxCfg), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.srslte_hip_dl_ctrl_phich_re.argtypes = [C.POINTER(DlCtrlTxCfg), C.c_uint32, vp, C.c_uint32]
    return L


def _ctrl_tx_cfg(nof_prb, nof_ports, cell_id, cp_ext=False, phich_resources=0, phich_ext=False, max_batch=1, max_dci=0, max_phich=0, tdd=False):
    return DlCtrlTxCfg(nof_prb, nof_ports, cell_id, 1 if cp_ext else 0, phich_resources, 1 if phich_ext else 0, 1 if tdd else 0, max_batch, max_dci,
                       max_phich)


def _ctrl_tx_in(cfi, dcis, phichs):
    """(DlCtrlTxIn, the ctypes arrays it points at). dcis: (sf, msg) with msg anything of the srslte_dci_msg_t layout; phichs: PhichTx or
    (sf, n_prb_lowest, n_dmrs, I_phich, ack)."""
    c = np.ascontiguousarray(cfi, np.uint32)
    d = (DlCtrlTxDci * max(1, len(dcis)))(*[DlCtrlTxDci(sf, DciMsg.from_buffer_copy(bytes(m)[:C.sizeof(DciMsg)])) for sf, m in dcis])
    p = (PhichTx * max(1, len(phichs)))(*[x if isinstance(x, PhichTx) else PhichTx(*x) for x in phichs])
    return DlCtrlTxIn(c.ctypes.data if c.size else None, d, len(dcis), p, len(phichs)), (c, d, p)


def phich_ngroups(nof_prb, nof_ports, cell_id, cp_ext=False, phich_resources=0, phich_ext=False):
    """srslte_regs_phich_ngroups (PHICH groups; x 2 on an extended-CP cell) (host; no GPU)."""
    n = _bind_dl_ctrl_tx(lib()).srslte_hip_dl_ctrl_phich_ngroups(C.byref(_ctrl_tx_cfg(nof_prb, nof_ports, cell_id, cp_ext, phich_resources, phich_ext)))
    if n < 0:
        raise ValueError("srslte_hip_dl_ctrl_phich_ngroups: %d" % n)
    return n


def phich_calc(nof_prb, nof_ports, cell_id, n_prb_lowest, n_dmrs, I_phich, cp_ext=False, phich_resources=0, phich_ext=False):
    """srslte_phich_calc -> (ngroup, nseq) (host)."""
    g, q = C.c_uint32(0), C.c_uint32(0)
    rc = _bind_dl_ctrl_tx(lib()).srslte_hip_phich_calc(C.byref(_ctrl_tx_cfg(nof_prb, nof_ports, cell_id, cp_ext, phich_resources, phich_ext)),
                                                        n_prb_lowest, n_dmrs, I_phich, C.byref(g), C.byref(q))
    if rc != SRSLTE_SUCCESS:
        raise ValueError("srslte_hip_phich_calc: %d" % rc)
    return g.value, q.value


def phich_re(nof_prb, nof_ports, cell_id, ngroup, cp_ext=False, phich_resources=0, phich_ext=False):
    """The 12 REs of PHICH group ngroup in srslte_regs_phich_add's order (host)."""
    out = np.zeros(12, np.uint32)
    n = _bind_dl_ctrl_tx(lib()).srslte_hip_dl_ctrl_phich_re(C.byref(_ctrl_tx_cfg(nof_prb, nof_ports, cell_id, cp_ext, phich_resources, phich_ext)),
                                                            ngroup, out.ctypes.data, 12)
    if n < 0:
        raise ValueError("srslte_hip_dl_ctrl_phich_re: %d" % n)
    return out[:n]


class DlCtrlTx:
    """Batched control-region transmit: the PCFICH of srslte_enb_dl_put_base, srslte_enb_dl_put_phich and srslte_enb_dl_put_pdcch_dl / _ul."""

    def __init__(self, nof_prb, nof_ports, cell_id, cp_ext=False, phich_resources=0, phich_ext=False, max_batch=1, max_dci=16, max_phich=16, tdd=False):
        L = _bind_dl_ctrl_tx(lib())
        self.cfg = _ctrl_tx_cfg(nof_prb, nof_ports, cell_id, cp_ext, phich_resources, phich_ext, max_batch, max_dci, max_phich, tdd)
        self.h = L.srslte_hip_dl_ctrl_tx_create(C.byref(self.cfg))
        if not self.h:
            raise RuntimeError("srslte_hip_dl_ctrl_tx_create failed")
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

    def free(self):
        if self.h:
            lib().srslte_hip_dl_ctrl_tx_destroy(self.h)
            self.h = None


# ---------------------------------------------------------------- UL control: PUCCH (phy_hip.h "UL control")
PUCCH_FORMAT_1, PUCCH_FORMAT_1A, PUCCH_FORMAT_1B, PUCCH_FORMAT_2, PUCCH_FORMAT_2A, PUCCH_FORMAT_2B = range(6)


class UlCtrlCfg(C.Structure):
    """srslte_hip_ul_ctrl_cfg_t: the cell, the common PUCCH configuration of srslte_pucch_cfg_t and the requests per call."""
    _fields_ = [("nof_prb", C.c_uint32), ("cell_id", C.c_uint32), ("cp_ext", C.c_int), ("delta_pucch_shift", C.c_uint32), ("n_rb_2", C.c_uint32),
                ("N_cs", C.c_uint32), ("N_pucch_1", C.c_uint32), ("group_hopping_en", C.c_int), ("threshold_format1", C.c_float),
                ("threshold_data_valid_format1a", C.c_float), ("threshold_data_valid_format2", C.c_float), ("max_pucch", C.c_uint32), ("tdd", C.c_int)]


class PucchReq(C.Structure):
    """srslte_hip_pucch_req_t: one (subframe, UE) as srslte_enb_ul_get_pucch is given it."""
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
    _fields_ = [("detected", C.c_uint32), ("correlation", C.c_float), ("format", C.c_uint32), ("n_pucch", C.c_uint32), ("sr", C.c_uint8),
                ("ack", C.c_uint8 * 2), ("ack_valid", C.c_uint8), ("cqi", C.c_uint8 * 13), ("cqi_crc", C.c_uint8), ("ri", C.c_uint8), ("reserved", C.c_uint8)]


class PucchTx(C.Structure):
    """srslte_hip_pucch_tx_t: a request and its UCI values."""
    _fields_ = [("req", PucchReq), ("ack", C.c_uint8 * 2), ("sr", C.c_uint8), ("ri", C.c_uint8), ("cqi", C.c_uint8 * 12)]

    @classmethod
    def make(cls, req, ack=(0, 0), sr=0, ri=0, cqi=()):
        t = cls()
        t.req = req
        t.ack[0], t.ack[1], t.sr, t.ri = ack[0], ack[1], sr, ri
        for i, b in enumerate(cqi):
            t.cqi[i] = b
        return t


def _bind_ul_ctrl(L):
    vp = C.c_void_p
    L.srslte_hip_ul_ctrl_create.restype = vp
    L.srslte_hip_ul_ctrl_create.argtypes = [C.POINTER(UlCtrlCfg)]
    L.srslte_hip_ul_ctrl_destroy.argtypes = [vp]
    L.srslte_hip_ul_ctrl_pucch_batch.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, vp]
    L.srslte_hip_ul_ctrl_debug_buffer.restype = vp
    L.srslte_hip_ul_ctrl_debug_buffer.argtypes = [vp, C.c_int]
    L.srslte_hip_ul_ctrl_tx_create.restype = vp
    L.srslte_hip_ul_ctrl_tx_create.argtypes = [C.POINTER(UlCtrlCfg)]
    L.srslte_hip_ul_ctrl_tx_destroy.argtypes = [vp]
    L.srslte_hip_ul_ctrl_tx_put_pucch.argtypes = [vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, vp]
    L.srslte_hip_ul_rx_batch_grants_pucch.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, vp, vp, vp, C.c_uint32, vp, vp]
    L.srslte_hip_pucch_n_cs_cell.argtypes = [C.POINTER(UlCtrlCfg), vp]
    L.srslte_hip_pucch_resource.argtypes = [C.POINTER(UlCtrlCfg), vp, C.POINTER(PucchReq), vp]
    L.srslte_hip_pucch_dmrs.argtypes = [C.POINTER(UlCtrlCfg), C.c_uint32, C.c_uint32, C.c_uint32, vp, vp]
    return L


def ul_ctrl_cfg(nof_prb, cell_id, cp_ext=False, delta_pucch_shift=1, n_rb_2=2, N_cs=0, N_pucch_1=0, group_hopping_en=False, threshold_format1=0.5,
                threshold_data_valid_format1a=0.5, threshold_data_valid_format2=0.5, max_pucch=1, tdd=False):
    return UlCtrlCfg(nof_prb, cell_id, 1 if cp_ext else 0, delta_pucch_shift, n_rb_2, N_cs, N_pucch_1, 1 if group_hopping_en else 0, threshold_format1,
                     threshold_data_valid_format1a, threshold_data_valid_format2, max_pucch, 1 if tdd else 0)


def pucch_n_cs_cell(cfg):
    """srslte_pucch_n_cs_cell -> [20][7] uint32 (host; no GPU)."""
    out = np.zeros((20, 7), np.uint32)
    _check(_bind_ul_ctrl(lib()).srslte_hip_pucch_n_cs_cell(C.byref(cfg), out.ctypes.data), "pucch_n_cs_cell")
    return out


def pucch_resource(cfg, req, uci=None):
    """srslte_ue_ul_pucch_resource_selection -> (format, n_pucch, n_prb slot 0, n_prb slot 1), or None where no format fits (host).
    uci: None for the receiver's zero value, else a PucchTx whose UCI values count."""
    out = np.zeros(4, np.uint32)
    rc = _bind_ul_ctrl(lib()).srslte_hip_pucch_resource(C.byref(cfg), C.byref(uci) if uci is not None else None, C.byref(req), out.ctypes.data)
    return None if rc != SRSLTE_SUCCESS else tuple(int(x) for x in out)


def pucch_dmrs(cfg, fmt, n_pucch, tti, drs_bits=(0, 0)):
    """srslte_refsignal_dmrs_pucch_gen of one configuration -> [2][N_rs][12] complex64 (host)."""
    r = np.zeros(2 * 3 * 12, np.complex64)
    b = np.array(drs_bits, np.uint8)
    n = _bind_ul_ctrl(lib()).srslte_hip_pucch_dmrs(C.byref(cfg), fmt, n_pucch, tti, b.ctypes.data, r.ctypes.data)
    if n < 0:
        raise ValueError("srslte_hip_pucch_dmrs: %d" % n)
    return r[:2 * n].reshape(2, n // 12, 12)


class UlCtrl:
    """Batched PUCCH receive: srslte_enb_ul_get_pucch for a list of (subframe, UE) requests."""

    def __init__(self, nof_prb, cell_id, max_pucch=1, **kw):
        L = _bind_ul_ctrl(lib())
        self.cfg = ul_ctrl_cfg(nof_prb, cell_id, max_pucch=max_pucch, **kw)
        self.h = L.srslte_hip_ul_ctrl_create(C.byref(self.cfg))
        if not self.h:
            raise RuntimeError("srslte_hip_ul_ctrl_create failed")
        self.grid_len = (12 if self.cfg.cp_ext else 14) * 12 * nof_prb
        self.max_pucch = max_pucch

    def run_device(self, d_grid, tti0, nof_sf, reqs, d_res, stream=None):
        arr = (PucchReq * max(1, len(reqs)))(*reqs)
        return lib().srslte_hip_ul_ctrl_pucch_batch(self.h, d_grid, tti0, nof_sf, arr, len(reqs), d_res, stream)

    def batch(self, grid, tti0, reqs):
        """grid [nof_sf][grid_len] complex64 -> (rc, [PucchRes] or None)."""
        g = np.ascontiguousarray(grid, np.complex64).reshape(-1, self.grid_len)
        dg, dr = DevBuf.from_host(g), DevBuf(C.sizeof(PucchRes) * max(1, len(reqs)))
        rc = self.run_device(dg.ptr, tti0, g.shape[0], reqs, dr.ptr)
        if rc != SRSLTE_SUCCESS:
            return rc, None
        sync()
        out = (PucchRes * max(1, len(reqs)))()
        _check(lib().srslte_hip_memcpy_d2h(C.addressof(out), dr.ptr, C.sizeof(out)), "memcpy_d2h")
        return rc, list(out)[:len(reqs)]

    def debug(self, which, nof):
        """0: equalised symbols [nof][120] complex64; 1: descrambled LLRs [nof][20] int16 (last call)."""
        dt, n = (np.complex64, 120) if which == 0 else (np.int16, 20)
        out = np.empty(nof * n, dt)
        _check(lib().srslte_hip_memcpy_d2h(out.ctypes.data, lib().srslte_hip_ul_ctrl_debug_buffer(self.h, which), out.nbytes), "memcpy_d2h")
        return out.reshape(nof, n)

    def free(self):
        if self.h:
            lib().srslte_hip_ul_ctrl_destroy(self.h)
            self.h = None


class UlCtrlTx:
    """Batched PUCCH transmit: srslte_pucch_encode + the PUCCH DMRS into UE grids."""

    def __init__(self, nof_prb, cell_id, max_pucch=1, **kw):
        L = _bind_ul_ctrl(lib())
        self.cfg = ul_ctrl_cfg(nof_prb, cell_id, max_pucch=max_pucch, **kw)
        self.h = L.srslte_hip_ul_ctrl_tx_create(C.byref(self.cfg))
        if not self.h:
            raise RuntimeError("srslte_hip_ul_ctrl_tx_create failed")
        self.grid_len = (12 if self.cfg.cp_ext else 14) * 12 * nof_prb

    def put_device(self, d_grid, tti0, nof_sf, txs, stream=None):
        arr = (PucchTx * max(1, len(txs)))(*txs)
        return lib().srslte_hip_ul_ctrl_tx_put_pucch(self.h, tti0, nof_sf, arr, len(txs), d_grid, stream)

    def put(self, grid, tti0, txs):
        """grid [nof_sf][grid_len] complex64 (host) -> (rc, the grids after the call)."""
        g = np.ascontiguousarray(grid, np.complex64).reshape(-1, self.grid_len)
        d = DevBuf.from_host(g)
        rc = self.put_device(d.ptr, tti0, g.shape[0], txs)
        sync()
        return rc, d.to_host(np.complex64).reshape(g.shape)

    def free(self):
        if self.h:
            lib().srslte_hip_ul_ctrl_tx_destroy(self.h)
            self.h = None


def _ul_rx_decode_grants_pucch(self, iq, tti0, grants, ctrl, reqs):
    """srslte_hip_ul_rx_batch_grants_pucch: (rc, tb, tb_ok, [PucchRes]); grants may be empty."""
    x = np.ascontiguousarray(iq, np.complex64).reshape(-1, self.sf_len)
    din = DevBuf.from_host(x)
    garr = (UlGrant * max(1, len(grants)))(*grants)
    rarr = (PucchReq * max(1, len(reqs)))(*reqs)
    dres = DevBuf(C.sizeof(PucchRes) * max(1, len(reqs)))
    L = _bind_ul_ctrl(lib())
    rc = L.srslte_hip_ul_rx_batch_grants_pucch(self.h, din.ptr, tti0, x.shape[0], garr, len(grants), self.d_tb.ptr, self.tb_stride, self.d_ok.ptr, ctrl.h,
                                               rarr, len(reqs), dres.ptr, None)
    if rc != SRSLTE_SUCCESS:
        return rc, None, None, None
    sync()
    self.last_nof_grants = len(grants)
    out = (PucchRes * max(1, len(reqs)))()
    _check(lib().srslte_hip_memcpy_d2h(C.addressof(out), dres.ptr, C.sizeof(out)), "memcpy_d2h")
    tb = self.d_tb.to_host(np.uint8).reshape(self.rows, self.tb_stride)[:len(grants)]
    return rc, tb, self.d_ok.to_host(np.uint8)[:len(grants)], list(out)[:len(reqs)]


UlRx.decode_grants_pucch = _ul_rx_decode_grants_pucch


# ---------------------------------------------------------------- UL control: PRACH (phy_hip.h "UL control: PRACH")
class PrachCfg(C.Structure):
    """srslte_hip_prach_cfg_t: the cell's PRACH configuration (SIB2), the detection factor and the entries per call."""
    _fields_ = [("nof_prb", C.c_uint32), ("config_idx", C.c_uint32), ("root_seq_idx", C.c_uint32), ("zero_corr_zone", C.c_uint32), ("hs_flag", C.c_int),
                ("tdd", C.c_int), ("detect_factor", C.c_float), ("max_occasions", C.c_uint32), ("max_preambles", C.c_uint32)]


class PrachInfo(C.Structure):
    """srslte_hip_prach_info_t."""
    _fields_ = [("N_zc", C.c_uint32), ("N_cs", C.c_uint32), ("N_cp", C.c_uint32), ("N_seq", C.c_uint32), ("N_ifft_prach", C.c_uint32),
                ("N_ifft_ul", C.c_uint32), ("format", C.c_uint32), ("nof_roots", C.c_uint32), ("n_wins", C.c_uint32), ("max_det", C.c_uint32),
                ("nof_sf", C.c_uint32), ("root_seqs_idx", C.c_uint32 * 64)]


class PrachTx(C.Structure):
    """srslte_hip_prach_tx_t: one preamble to generate."""
    _fields_ = [("seq_index", C.c_uint32), ("freq_offset", C.c_uint32)]


class PrachOccasion(C.Structure):
    """srslte_hip_prach_occasion_t: the first sample after the CP in the signal, and the PRACH's PRB offset."""
    _fields_ = [("sample", C.c_uint64), ("freq_offset", C.c_uint32), ("reserved", C.c_uint32)]


def _bind_prach(L):
    vp = C.c_void_p
    L.srslte_hip_prach_create.restype = vp
    L.srslte_hip_prach_create.argtypes = [C.POINTER(PrachCfg)]
    L.srslte_hip_prach_destroy.argtypes = [vp]
    L.srslte_hip_prach_info.argtypes = [vp, C.POINTER(PrachInfo)]
    L.srslte_hip_prach_gen_batch.argtypes = [vp, vp, C.c_uint32, vp, vp]
    L.srslte_hip_prach_detect_batch.argtypes = [vp, vp, C.c_size_t, vp, C.c_uint32, vp, vp, vp, vp, vp]
    L.srslte_hip_prach_cfg_info.argtypes = [C.POINTER(PrachCfg), C.POINTER(PrachInfo)]
    L.srslte_hip_prach_gen_check.argtypes = [C.POINTER(PrachCfg), vp, C.c_uint32]
    L.srslte_hip_prach_detect_check.argtypes = [C.POINTER(PrachCfg), C.c_size_t, vp, C.c_uint32]
    L.srslte_hip_prach_tti_opportunity_fdd.argtypes = [C.c_uint32, C.c_uint32, C.c_int]
    L.srslte_hip_prach_preamble_format.argtypes = [C.c_uint32]
    return L


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


class Prach:
    """Batched PRACH: srslte_prach_gen for a list of preambles, srslte_prach_detect_offset for a list of occasions in one signal."""

    def __init__(self, nof_prb, config_idx, max_occasions=1, max_preambles=1, **kw):
        self.cfg = prach_cfg(nof_prb, config_idx, max_occasions=max_occasions, max_preambles=max_preambles, **kw)
        self.h = lib().srslte_hip_prach_create(C.byref(self.cfg))
        if not self.h:
            raise RuntimeError("srslte_hip_prach_create failed")
        self.info = PrachInfo()
        _check(lib().srslte_hip_prach_info(self.h, C.byref(self.info)), "prach_info")
        self.len = self.info.N_cp + self.info.N_seq

    def gen_device(self, txs, d_out, stream=None):
        arr = (PrachTx * max(1, len(txs)))(*txs)
        return lib().srslte_hip_prach_gen_batch(self.h, arr, len(txs), d_out, stream)

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
        arr = (PrachOccasion * max(1, len(occs)))(*occs)
        return lib().srslte_hip_prach_detect_batch(self.h, d_signal, sig_len, arr, len(occs), d_nof, d_idx, d_toff, d_p2a, stream)

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

    def free(self):
        if self.h:
            lib().srslte_hip_prach_destroy(self.h)
            self.h = None


# ---------------------------------------------------------------- UE CSI feedback (phy_hip.h "UE CSI feedback")
class CsiRes(C.Structure):
    """srslte_hip_csi_res_t: the measurement of one subframe."""
    _fields_ = [("sinr_1l", C.c_float * 4), ("sinr_2l", C.c_float * 2), ("pmi_1l", C.c_uint32), ("pmi_2l", C.c_uint32), ("cn_db", C.c_float),
                ("ri_cn", C.c_uint32), ("ri", C.c_uint32), ("pmi", C.c_uint32), ("sinr_db", C.c_float), ("cqi_sinr", C.c_uint32),
                ("cqi_wideband", C.c_uint32), ("reserved", C.c_uint32)]


CQI_TYPE_WIDEBAND, CQI_TYPE_SUBBAND, CQI_TYPE_SUBBAND_UE, CQI_TYPE_SUBBAND_HL = range(4)
CQI_MAX_BITS = 64


class CqiCfg(C.Structure):
    """srslte_hip_cqi_cfg_t (srslte_cqi_cfg_t)."""
    _fields_ = [("type", C.c_int), ("data_enable", C.c_int), ("pmi_present", C.c_int), ("four_antenna_ports", C.c_int), ("rank_is_not_one", C.c_int),
                ("subband_label_2_bits", C.c_int), ("L", C.c_uint32), ("N", C.c_uint32)]


class CqiValue(C.Structure):
    """srslte_hip_cqi_value_t: the members of the four report structs of srslte_cqi_value_t side by side."""
    _fields_ = [(n, C.c_uint32) for n in ("wideband_cqi", "spatial_diff_cqi", "pmi", "subband_cqi", "subband_label", "subband_diff_cqi",
                                          "wideband_cqi_cw1", "subband_diff_cqi_cw1")]


class CsiReportCfg(C.Structure):
    """srslte_hip_csi_report_cfg_t: the UE's reporting configuration; last_ri is carried in and out."""
    _fields_ = [("tm", C.c_int), ("nof_prb", C.c_uint32), ("nof_ports", C.c_uint32), ("nof_rx_antennas", C.c_uint32), ("tdd", C.c_int),
                ("periodic_configured", C.c_int), ("ri_idx_present", C.c_int), ("I_cqi_pmi", C.c_uint32), ("I_ri", C.c_uint32),
                ("format_is_subband", C.c_int), ("aperiodic_mode", C.c_int), ("snr_to_cqi_offset", C.c_float), ("last_ri", C.c_uint32)]


class CsiReport(C.Structure):
    """srslte_hip_csi_report_t."""
    _fields_ = [("cqi", CqiCfg), ("value", CqiValue), ("ri_len", C.c_uint32), ("ri", C.c_uint32), ("cqi_len", C.c_uint32),
                ("cqi_bits", C.c_uint8 * CQI_MAX_BITS)]


def _bind_csi(L):
    vp = C.c_void_p
    L.srslte_hip_csi_create.restype = vp
    L.srslte_hip_csi_create.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
    L.srslte_hip_csi_destroy.argtypes = [vp]
    L.srslte_hip_csi_set_snr_to_cqi_offset.argtypes = [vp, C.c_float]
    L.srslte_hip_csi_nof_samples.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.srslte_hip_csi_batch.argtypes = [vp, vp, vp, C.c_uint32, vp, vp]
    L.srslte_hip_dl_rx_csi_batch.argtypes = [vp, C.c_uint32, vp, vp]
    L.srslte_hip_dl_rx_set_snr_to_cqi_offset.argtypes = [vp, C.c_float]
    L.srslte_hip_csi_decide.argtypes = [C.POINTER(C.c_float), C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_uint32, C.POINTER(CsiRes)]
    L.srslte_hip_cqi_from_snr.restype = C.c_uint32
    L.srslte_hip_cqi_from_snr.argtypes = [C.c_float]
    L.srslte_hip_cqi_size.argtypes = [C.POINTER(CqiCfg)]
    L.srslte_hip_cqi_value_pack.argtypes = [C.POINTER(CqiCfg), C.POINTER(CqiValue), vp]
    L.srslte_hip_cqi_periodic_send.argtypes = [C.c_uint32, C.c_uint32, C.c_int]
    L.srslte_hip_cqi_periodic_ri_send.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
    L.srslte_hip_cqi_hl_get_no_subbands.argtypes = [C.c_int]
    L.srslte_hip_csi_gen_cqi_periodic.argtypes = [C.POINTER(CsiRes), C.POINTER(CsiReportCfg), C.c_uint32, C.c_uint32, C.POINTER(CsiReport)]
    L.srslte_hip_csi_gen_cqi_aperiodic.argtypes = [C.POINTER(CsiRes), C.POINTER(CsiReportCfg), C.c_uint32, C.POINTER(CsiReport)]
    return L


def _csi_rows(buf, n):
    """DevBuf of n srslte_hip_csi_res_t -> list of CsiRes (host copies)."""
    raw = buf.to_host(np.uint8, n * C.sizeof(CsiRes))
    return [CsiRes.from_buffer_copy(raw[i * C.sizeof(CsiRes):(i + 1) * C.sizeof(CsiRes)].tobytes()) for i in range(n)]


class Csi:
    """Batched CSI measurement (select_ri_pmi / srslte_ue_dl_select_ri per subframe) on DL estimates."""

    def __init__(self, nof_prb, nof_ports=2, nof_rx=2, cp_norm=True):
        self.h = lib().srslte_hip_csi_create(nof_prb, nof_ports, nof_rx, 1 if cp_norm else 0)
        if not self.h:
            raise RuntimeError("srslte_hip_csi_create failed")
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
        rc = self.run_device(dce.ptr, dres.ptr, n, dout.ptr)
        if rc != SRSLTE_SUCCESS:
            return rc, None
        sync()
        return rc, _csi_rows(dout, n)

    def free(self):
        if self.h:
            lib().srslte_hip_csi_destroy(self.h)
            self.h = None


def _dl_rx_csi(self, nof_sf, snr_to_cqi_offset=None):
    """srslte_hip_dl_rx_csi_batch on the estimates of the object's last batch -> (rc, [CsiRes] or None)."""
    if snr_to_cqi_offset is not None:
        _check(lib().srslte_hip_dl_rx_set_snr_to_cqi_offset(self.h, snr_to_cqi_offset), "dl_rx_set_snr_to_cqi_offset")
    dout = DevBuf(max(1, nof_sf) * C.sizeof(CsiRes))
    rc = lib().srslte_hip_dl_rx_csi_batch(self.h, nof_sf, dout.ptr, None)
    if rc != SRSLTE_SUCCESS:
        return rc, None
    sync()
    return rc, _csi_rows(dout, nof_sf)


DlRx.csi = _dl_rx_csi


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


# ---------------------------------------------------------------- channel emulator
CHANNEL_FADING_NONE, CHANNEL_FADING_EPA, CHANNEL_FADING_EVA, CHANNEL_FADING_ETU = range(4)
CHANNEL_MAXTAPS = 9
_CHANNEL_MODELS = {"none": CHANNEL_FADING_NONE, "epa": CHANNEL_FADING_EPA, "eva": CHANNEL_FADING_EVA, "etu": CHANNEL_FADING_ETU}


class ChannelCfg(C.Structure):
    """srslte_hip_channel_cfg_t (phy_hip.h)."""
    _fields_ = [("srate_hz", C.c_double), ("nof_channels", C.c_uint32), ("max_calls", C.c_uint32), ("max_len", C.c_uint32),
                ("fading_enable", C.c_int), ("fading_model", C.c_int), ("doppler_hz", C.c_float), ("seed0", C.c_uint32), ("seed_stride", C.c_uint32),
                ("delay_enable", C.c_int), ("delay_min_us", C.c_float), ("delay_max_us", C.c_float), ("delay_period_s", C.c_float),
                ("delay_init_time_s", C.c_float),
                ("hst_enable", C.c_int), ("hst_fd_hz", C.c_float), ("hst_period_s", C.c_float), ("hst_init_time_s", C.c_float),
                ("rlf_enable", C.c_int), ("rlf_t_on_ms", C.c_uint32), ("rlf_t_off_ms", C.c_uint32),
                ("awgn_enable", C.c_int), ("awgn_n0", C.c_float), ("awgn_seed", C.c_uint32)]


class ChannelBlock(C.Structure):
    """srslte_hip_channel_block_t."""
    _fields_ = [("t", C.c_double), ("delay_samples", C.c_uint32), ("hst_fs_hz", C.c_float), ("rlf_on", C.c_int)]


def _bind_channel(L):
    vp, u32, u64, dp = C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(C.c_double)
    L.srslte_hip_channel_create.argtypes = [C.POINTER(vp), C.POINTER(ChannelCfg)]
    L.srslte_hip_channel_destroy.argtypes = [vp]
    L.srslte_hip_channel_reset.argtypes = [vp]
    L.srslte_hip_channel_run_batch.argtypes = [vp, vp, u64, u64, vp, u64, u64, u32, u32, C.c_int64, C.c_double, vp]
    L.srslte_hip_channel_fft_size.argtypes = [vp]
    L.srslte_hip_channel_path_delay.argtypes = [vp]
    L.srslte_hip_channel_coeffs.argtypes = [vp, u32, dp, dp, dp]
    L.srslte_hip_channel_draw_coeffs.argtypes = [C.c_int, C.c_float, u32, dp, dp, dp]
    L.srslte_hip_channel_fft_size_for.argtypes = [C.c_int, C.c_double]
    L.srslte_hip_channel_block_params.argtypes = [C.POINTER(ChannelCfg), u32, u32, C.c_int64, C.c_double, C.POINTER(ChannelBlock)]


def channel_cfg(srate_hz, nof_channels=1, max_calls=1, max_len=1, fading=None, seed0=0, seed_stride=0x1234, delay=None, hst=None, rlf=None, awgn=None):
    """fading: a model string as the reference takes it ("epa5", "etu300"), or (model number, doppler_hz); delay: (min_us, max_us, period_s,
    init_time_s); hst: (fd_hz, period_s, init_time_s); rlf: (t_on_ms, t_off_ms); awgn: (n0, seed). None: the stage is off."""
    c = ChannelCfg()
    c.srate_hz, c.nof_channels, c.max_calls, c.max_len, c.seed0, c.seed_stride = srate_hz, nof_channels, max_calls, max_len, seed0, seed_stride
    if fading is not None:
        c.fading_enable = 1
        if isinstance(fading, str):
            name = fading[:4] if fading.startswith("none") else fading[:3]
            c.fading_model = _CHANNEL_MODELS.get(name, -1)
            c.doppler_hz = float(fading[len(name):] or 0)
        else:
            c.fading_model, c.doppler_hz = fading
    if delay is not None:
        c.delay_enable, (c.delay_min_us, c.delay_max_us, c.delay_period_s, c.delay_init_time_s) = 1, delay
    if hst is not None:
        c.hst_enable, (c.hst_fd_hz, c.hst_period_s, c.hst_init_time_s) = 1, hst
    if rlf is not None:
        c.rlf_enable, (c.rlf_t_on_ms, c.rlf_t_off_ms) = 1, rlf
    if awgn is not None:
        c.awgn_enable, (c.awgn_n0, c.awgn_seed) = 1, awgn
    return c


def channel_n0_from_snr(snr_db, signal_power=1.0):
    """The n0 that puts a signal of the stated power (mean |x|^2) at snr_db."""
    return signal_power / 10.0 ** (snr_db / 10.0)


def channel_draw_coeffs(model, doppler_hz, seed):
    """srslte_hip_channel_draw_coeffs (host) -> a, w, p of fading.c:168-175."""
    a, w, p = (np.zeros(CHANNEL_MAXTAPS) for _ in range(3))
    dp = C.POINTER(C.c_double)
    n = lib().srslte_hip_channel_draw_coeffs(model, doppler_hz, seed, a.ctypes.data_as(dp), w.ctypes.data_as(dp), p.ctypes.data_as(dp))
    if n < 0:
        raise RuntimeError("srslte_hip_channel_draw_coeffs failed with %d" % n)
    return a[:n], w[:n], p[:n]


def channel_fft_size_for(model, srate_hz):
    return lib().srslte_hip_channel_fft_size_for(model, srate_hz)


def channel_block_params(cfg, length, i, t_full_secs, t_frac_secs):
    """srslte_hip_channel_block_params (host) -> (rc, ChannelBlock)."""
    out = ChannelBlock()
    return lib().srslte_hip_channel_block_params(C.byref(cfg), length, i, t_full_secs, t_frac_secs, C.byref(out)), out


class Channel:
    """srslte::channel for nof_channels channels and nof_calls blocks per call (srslte_hip_channel_*). cfg: channel_cfg(...)."""

    def __init__(self, cfg):
        h = C.c_void_p()
        rc = lib().srslte_hip_channel_create(C.byref(h), C.byref(cfg))
        if rc != SRSLTE_SUCCESS:
            raise RuntimeError("srslte_hip_channel_create failed with %d" % rc)
        self.h, self.cfg = h, cfg
        self.fft_size = lib().srslte_hip_channel_fft_size(h)
        self.path_delay = lib().srslte_hip_channel_path_delay(h)

    def coeffs(self, channel):
        a, w, p = (np.zeros(CHANNEL_MAXTAPS) for _ in range(3))
        dp = C.POINTER(C.c_double)
        n = lib().srslte_hip_channel_coeffs(self.h, channel, a.ctypes.data_as(dp), w.ctypes.data_as(dp), p.ctypes.data_as(dp))
        if n < 0:
            raise RuntimeError("srslte_hip_channel_coeffs failed with %d" % n)
        return a[:n], w[:n], p[:n]

    def reset(self):
        _check(lib().srslte_hip_channel_reset(self.h), "channel_reset")

    def run_dev(self, d_in, d_out, nof_calls, length, t_full_secs=0, t_frac_secs=0.0, in_strides=None, out_strides=None, stream=None):
        """Device buffers (DevBuf / DevView), [channel][call][len] with (channel, call) strides in samples; dense when None. -> rc."""
        ics, ibs = in_strides or (nof_calls * length, length)
        ocs, obs = out_strides or (nof_calls * length, length)
        return lib().srslte_hip_channel_run_batch(self.h, d_in.ptr, ics, ibs, d_out.ptr, ocs, obs, nof_calls, length, t_full_secs, t_frac_secs, stream)

    def run(self, x, t_full_secs=0, t_frac_secs=0.0):
        """x: [nof_channels][nof_calls][len] complex -> the same shape, complex64."""
        x = np.ascontiguousarray(x, np.complex64)
        nch, nof_calls, length = x.shape
        if nch != self.cfg.nof_channels:
            raise ValueError("x has %d channels, the object %d" % (nch, self.cfg.nof_channels))
        din, dout = DevBuf.from_host(x), DevBuf(max(x.nbytes, 1))
        _check(self.run_dev(din, dout, nof_calls, length, t_full_secs, t_frac_secs), "channel_run_batch")
        sync()
        return dout.to_host(np.complex64, x.size).reshape(x.shape)

    def free(self):
        if self.h:
            lib().srslte_hip_channel_destroy(self.h)
            self.h = None


# ---------------------------------------------------------------- UL sounding reference signal (phy_hip.h "UL sounding reference signal")
SRS_MAX_CE = 72


class SrsCfg(C.Structure):
    """srslte_hip_srs_cfg_t: the cell, its SRS subframe and bandwidth configuration, the sequence hopping switches and the entries per call."""
    _fields_ = [("nof_prb", C.c_uint32), ("cell_id", C.c_uint32), ("cp_ext", C.c_int), ("subframe_config", C.c_uint32), ("bw_cfg", C.c_uint32),
                ("group_hopping_en", C.c_int), ("sequence_hopping_en", C.c_int), ("delta_ss", C.c_uint32), ("max_srs", C.c_uint32), ("tdd", C.c_int)]


class SrsUe(C.Structure):
    """srslte_hip_srs_ue_t: one (subframe, UE)."""
    _fields_ = [("sf", C.c_uint32), ("B", C.c_uint32), ("b_hop", C.c_uint32), ("n_srs", C.c_uint32), ("I_srs", C.c_uint32), ("k_tc", C.c_uint32),
                ("n_rrc", C.c_uint32), ("cs_used", C.c_uint32)]

    @classmethod
    def make(cls, sf, B=0, b_hop=3, n_srs=0, I_srs=0, k_tc=0, n_rrc=0, cs_used=0):
        return cls(sf, B, b_hop, n_srs, I_srs, k_tc, n_rrc, cs_used)


class SrsRes(C.Structure):
    """srslte_hip_srs_res_t."""
    _fields_ = [("rsrp", C.c_float), ("noise_estimate", C.c_float), ("noise_estimate_dbm", C.c_float), ("snr", C.c_float), ("snr_db", C.c_float),
                ("ta_us", C.c_float), ("nof_ce", C.c_uint32)]


def _bind_srs(L):
    vp, u32, cp, up = C.c_void_p, C.c_uint32, C.POINTER(SrsCfg), C.POINTER(SrsUe)
    L.srslte_hip_srs_create.restype = vp
    L.srslte_hip_srs_create.argtypes = [cp]
    L.srslte_hip_srs_destroy.argtypes = [vp]
    L.srslte_hip_srs_tx_put.argtypes = [vp, u32, u32, vp, u32, vp, vp]
    L.srslte_hip_srs_rx_batch.argtypes = [vp, vp, u32, u32, vp, u32, vp, vp, vp]
    L.srslte_hip_ul_rx_batch_grants_pucch_srs.argtypes = [vp, vp, u32, u32, vp, u32, vp, u32, vp, vp, vp, u32, vp, vp, vp, u32, vp, vp, vp]
    L.srslte_hip_srs_send_cs.argtypes = [u32, u32]
    L.srslte_hip_srs_send_ue.argtypes = [u32, u32]
    for fn in (L.srslte_hip_srs_rb_start_cs, L.srslte_hip_srs_rb_L_cs):
        fn.restype, fn.argtypes = u32, [u32, u32]
    L.srslte_hip_srs_M_sc.restype, L.srslte_hip_srs_M_sc.argtypes = u32, [cp, up]
    L.srslte_hip_srs_k0.restype, L.srslte_hip_srs_k0.argtypes = u32, [cp, up, u32]
    L.srslte_hip_srs_pusch_shortened.argtypes = [cp, up, u32, C.POINTER(u32 * 2), u32]
    L.srslte_hip_srs_pucch_shortened.argtypes = [cp, C.c_int, C.c_int, u32, u32]
    L.srslte_hip_srs_gen.argtypes = [cp, up, u32, vp]
    L.srslte_hip_srs_check.argtypes = [cp, u32, u32, vp, u32]
    return L


def srs_cfg(nof_prb, cell_id, bw_cfg, subframe_config=0, cp_ext=False, group_hopping_en=False, sequence_hopping_en=False, delta_ss=0, max_srs=1,
            tdd=False):
    return SrsCfg(nof_prb, cell_id, 1 if cp_ext else 0, subframe_config, bw_cfg, 1 if group_hopping_en else 0, 1 if sequence_hopping_en else 0, delta_ss,
                  max_srs, 1 if tdd else 0)


def srs_send_cs(subframe_config, sf_idx):
    return _bind_srs(lib()).srslte_hip_srs_send_cs(subframe_config, sf_idx)


def srs_send_ue(I_srs, tti):
    return _bind_srs(lib()).srslte_hip_srs_send_ue(I_srs, tti)


def srs_rb_start_cs(bw_cfg, nof_prb):
    return _bind_srs(lib()).srslte_hip_srs_rb_start_cs(bw_cfg, nof_prb)


def srs_rb_L_cs(bw_cfg, nof_prb):
    return _bind_srs(lib()).srslte_hip_srs_rb_L_cs(bw_cfg, nof_prb)


def srs_M_sc(cfg, ue):
    return _bind_srs(lib()).srslte_hip_srs_M_sc(C.byref(cfg), C.byref(ue))


def srs_k0(cfg, ue, tti):
    return _bind_srs(lib()).srslte_hip_srs_k0(C.byref(cfg), C.byref(ue), tti)


def srs_pusch_shortened(cfg, ue, tti, n_prb_tilde, L_prb):
    """srslte_refsignal_srs_pusch_shortened (host); ue None: no UE-specific SRS configured."""
    n = (C.c_uint32 * 2)(*n_prb_tilde)
    return _bind_srs(lib()).srslte_hip_srs_pusch_shortened(C.byref(cfg), C.byref(ue) if ue is not None else None, tti, C.byref(n), L_prb)


def srs_pucch_shortened(cfg, ue_configured, simul_ack, fmt, tti):
    return _bind_srs(lib()).srslte_hip_srs_pucch_shortened(C.byref(cfg), 1 if ue_configured else 0, 1 if simul_ack else 0, fmt, tti)


def srs_gen(cfg, ue, sf_idx):
    """srslte_refsignal_srs_gen -> [2][M_sc] complex64 (host; no GPU)."""
    M = srs_M_sc(cfg, ue)
    r = np.zeros(2 * max(M, 1), np.complex64)
    _check(lib().srslte_hip_srs_gen(C.byref(cfg), C.byref(ue), sf_idx, r.ctypes.data), "srs_gen")
    return r.reshape(2, -1)


def srs_check(cfg, tti0, nof_sf, ues):
    """What srslte_hip_srs_create and a call with this list would answer, without a device."""
    arr = (SrsUe * max(1, len(ues)))(*ues)
    return _bind_srs(lib()).srslte_hip_srs_check(C.byref(cfg), tti0, nof_sf, arr, len(ues))


class Srs:
    """Batched SRS: srslte_refsignal_srs_put on UE grids and the eNB's sounding receiver."""

    def __init__(self, nof_prb, cell_id, bw_cfg, max_srs=1, **kw):
        L = _bind_srs(lib())
        self.cfg = srs_cfg(nof_prb, cell_id, bw_cfg, max_srs=max_srs, **kw)
        self.h = L.srslte_hip_srs_create(C.byref(self.cfg))
        if not self.h:
            raise RuntimeError("srslte_hip_srs_create failed")
        self.grid_len = (12 if self.cfg.cp_ext else 14) * 12 * nof_prb

    def put_device(self, d_grid, tti0, nof_sf, ues, stream=None):
        arr = (SrsUe * max(1, len(ues)))(*ues)
        return lib().srslte_hip_srs_tx_put(self.h, tti0, nof_sf, arr, len(ues), d_grid, stream)

    def put(self, grid, tti0, ues):
        """grid [nof_sf][grid_len] complex64 (host) -> (rc, the grids after the call)."""
        g = np.ascontiguousarray(grid, np.complex64).reshape(-1, self.grid_len)
        d = DevBuf.from_host(g)
        rc = self.put_device(d.ptr, tti0, g.shape[0], ues)
        sync()
        return rc, d.to_host(np.complex64).reshape(g.shape)

    def rx_device(self, d_grid, tti0, nof_sf, ues, d_res, d_ce, stream=None):
        arr = (SrsUe * max(1, len(ues)))(*ues)
        return lib().srslte_hip_srs_rx_batch(self.h, d_grid, tti0, nof_sf, arr, len(ues), d_res, d_ce, stream)

    @staticmethod
    def read(d_res, d_ce, nof):
        """-> ([SrsRes], ce [nof][SRS_MAX_CE] complex64; entries from nof_ce on are whatever the buffer held)."""
        out = (SrsRes * max(1, nof))()
        _check(lib().srslte_hip_memcpy_d2h(C.addressof(out), d_res.ptr, C.sizeof(out)), "memcpy_d2h")
        return list(out)[:nof], d_ce.to_host(np.complex64).reshape(-1, SRS_MAX_CE)[:nof]

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

    def free(self):
        if self.h:
            lib().srslte_hip_srs_destroy(self.h)
            self.h = None


def _ul_rx_decode_grants_pucch_srs(self, iq, tti0, grants, ctrl, reqs, srs, ues):
    """srslte_hip_ul_rx_batch_grants_pucch_srs: (rc, tb, tb_ok, [PucchRes], [SrsRes], ce); ctrl and srs may each be None."""
    x = np.ascontiguousarray(iq, np.complex64).reshape(-1, self.sf_len)
    din = DevBuf.from_host(x)
    garr = (UlGrant * max(1, len(grants)))(*grants)
    rarr = (PucchReq * max(1, len(reqs)))(*reqs)
    uarr = (SrsUe * max(1, len(ues)))(*ues)
    dres = DevBuf(C.sizeof(PucchRes) * max(1, len(reqs)))
    dsr, dsc = DevBuf(C.sizeof(SrsRes) * max(1, len(ues))), DevBuf(8 * SRS_MAX_CE * max(1, len(ues)))
    rc = _bind_srs(lib()).srslte_hip_ul_rx_batch_grants_pucch_srs(self.h, din.ptr, tti0, x.shape[0], garr, len(grants), self.d_tb.ptr, self.tb_stride,
                                                                   self.d_ok.ptr, ctrl.h if ctrl is not None else None, rarr, len(reqs), dres.ptr,
                                                                   srs.h if srs is not None else None, uarr, len(ues), dsr.ptr, dsc.ptr, None)
    if rc != SRSLTE_SUCCESS:
        return rc, None, None, None, None, None
    sync()
    self.last_nof_grants = len(grants)
    out = (PucchRes * max(1, len(reqs)))()
    _check(lib().srslte_hip_memcpy_d2h(C.addressof(out), dres.ptr, C.sizeof(out)), "memcpy_d2h")
    tb = self.d_tb.to_host(np.uint8).reshape(self.rows, self.tb_stride)[:len(grants)]
    sres, sce = Srs.read(dsr, dsc, len(ues))
    return rc, tb, self.d_ok.to_host(np.uint8)[:len(grants)], list(out)[:len(reqs)], sres, sce


UlRx.decode_grants_pucch_srs = _ul_rx_decode_grants_pucch_srs


# ---------------------------------------------------------------- UE synchronisation (phy_hip.h "UE synchronisation")
SYNC_FOUND, SYNC_FOUND_NOSPACE, SYNC_NOFOUND = 1, 2, 0
SSS_DIFF, SSS_PARTIAL_3, SSS_FULL = 0, 1, 2


class SyncCfg(C.Structure):
    """srslte_hip_sync_cfg_t."""
    _fields_ = [("fft_size", C.c_uint32), ("frame_size", C.c_uint32), ("max_offset", C.c_uint32), ("max_items", C.c_uint32), ("cp", C.c_int),
                ("detect_cp", C.c_uint8), ("sss_en", C.c_uint8), ("cfo_cp_enable", C.c_uint8), ("cfo_pss_enable", C.c_uint8),
                ("pss_filt_enable", C.c_uint8), ("sss_alg", C.c_uint8), ("tdd", C.c_uint8), ("reserved", C.c_uint8), ("cfo_cp_nsymbols", C.c_uint32),
                ("threshold", C.c_float), ("sss_threshold", C.c_float), ("ema_alpha", C.c_float), ("decimate", C.c_uint32)]


class SyncItem(C.Structure):
    """srslte_hip_sync_item_t."""
    _fields_ = [("N_id_2", C.c_uint32), ("find_offset", C.c_uint32), ("N_id_1", C.c_int32)]

    @classmethod
    def make(cls, N_id_2, find_offset=0, N_id_1=-1):
        return cls(N_id_2, find_offset, N_id_1)


class SyncRes(C.Structure):
    """srslte_hip_sync_res_t."""
    _fields_ = [("ret", C.c_int32), ("peak_pos", C.c_uint32), ("peak_value", C.c_float), ("corr_peak", C.c_float), ("cfo_cp", C.c_float),
                ("cfo_pss", C.c_float), ("cfo", C.c_float), ("sss_available", C.c_uint32), ("sss_detected", C.c_uint32), ("m0", C.c_uint32),
                ("m1", C.c_uint32), ("sf_idx", C.c_uint32), ("N_id_1", C.c_int32), ("cell_id", C.c_int32), ("sss_corr", C.c_float), ("cp", C.c_int32)]


class CellSearchResult(C.Structure):
    """srslte_hip_cell_search_result_t."""
    _fields_ = [("cell_id", C.c_uint32), ("cp", C.c_int), ("peak", C.c_float), ("mode", C.c_float), ("psr", C.c_float), ("cfo", C.c_float),
                ("nof_frames", C.c_uint32)]


def _bind_sync(L):
    vp, u32 = C.c_void_p, C.c_uint32
    L.srslte_hip_sync_create.restype = vp
    L.srslte_hip_sync_create.argtypes = [C.POINTER(SyncCfg)]
    L.srslte_hip_sync_destroy.argtypes = [vp]
    L.srslte_hip_sync_find_batch.argtypes = [vp, vp, C.c_size_t, vp, u32, vp, vp]
    L.srslte_hip_cfo_correct_batch.argtypes = [vp, vp, C.c_size_t, u32, u32, vp, vp]
    L.srslte_hip_sync_check.argtypes = [C.POINTER(SyncCfg), C.c_size_t, vp, u32]
    L.srslte_hip_cell_search_decide.argtypes = [vp, u32, C.POINTER(CellSearchResult)]
    L.srslte_hip_sync_cp_corr.argtypes = [vp, u32, vp]
    return L


def sync_cfg(fft_size, frame_size, max_offset, max_items=1, cp_ext=False, detect_cp=True, sss_en=True, cfo_cp_enable=False, cfo_pss_enable=False,
             pss_filt_enable=False, sss_alg=SSS_FULL, cfo_cp_nsymbols=3, threshold=0.0, sss_threshold=0.0, ema_alpha=0.0, tdd=False, decimate=0):
    """The defaults are those of srslte_sync_init (sync.c:64-82) but for the frame type, which is FDD."""
    return SyncCfg(fft_size, frame_size, max_offset, max_items, 1 if cp_ext else 0, int(bool(detect_cp)), int(bool(sss_en)), int(bool(cfo_cp_enable)),
                   int(bool(cfo_pss_enable)), int(bool(pss_filt_enable)), sss_alg, int(bool(tdd)), 0, cfo_cp_nsymbols, threshold, sss_threshold,
                   ema_alpha, decimate)


def sync_rows(items):
    """Result rows of a call: three for an item with N_id_2 = 3, one otherwise."""
    return sum(3 if it.N_id_2 == 3 else 1 for it in items)


def sync_check(cfg, in_stride, items):
    """What srslte_hip_sync_create and a call with these items would answer, without a device."""
    arr = (SyncItem * max(1, len(items)))(*items)
    return _bind_sync(lib()).srslte_hip_sync_check(C.byref(cfg), in_stride, arr, len(items))


def cell_search_decide(rows):
    """srslte_hip_cell_search_decide (host): (number of frames that counted, CellSearchResult)."""
    arr = (SyncRes * max(1, len(rows)))(*rows)
    out = CellSearchResult()
    return _bind_sync(lib()).srslte_hip_cell_search_decide(arr, len(rows), C.byref(out)), out


def cfo_correct_device(d_in, d_out, stride, length, n, freq, stream=None):
    f = np.ascontiguousarray(freq, np.float32)
    return _bind_sync(lib()).srslte_hip_cfo_correct_batch(d_in, d_out, stride, length, n, f.ctypes.data, stream)


def cfo_correct(x, freq, in_place=False):
    """x [n][len] complex64, freq [n] cycles per sample -> x exp(j 2 pi freq i) from the device."""
    a = np.ascontiguousarray(x, np.complex64)
    a = a.reshape(1, -1) if a.ndim == 1 else a
    din = DevBuf.from_host(a)
    dout = din if in_place else DevBuf(a.nbytes)
    _check(cfo_correct_device(din.ptr, dout.ptr, a.shape[1], a.shape[1], a.shape[0], freq), "cfo_correct_batch")
    sync()
    return dout.to_host(np.complex64).reshape(a.shape)


class Sync:
    """Batched PSS / SSS synchronisation: the first srslte_sync_find of a reset object per item."""

    def __init__(self, fft_size, frame_size, max_offset, max_items=1, **kw):
        L = _bind_sync(lib())
        self.cfg = sync_cfg(fft_size, frame_size, max_offset, max_items=max_items, **kw)
        self.h = L.srslte_hip_sync_create(C.byref(self.cfg))
        if not self.h:
            raise RuntimeError("srslte_hip_sync_create failed")

    def find_device(self, d_in, in_stride, items, d_res, stream=None):
        arr = (SyncItem * max(1, len(items)))(*items)
        return lib().srslte_hip_sync_find_batch(self.h, d_in, in_stride, arr, len(items), d_res, stream)

    @staticmethod
    def read(d_res, rows):
        out = (SyncRes * max(1, rows))()
        _check(lib().srslte_hip_memcpy_d2h(C.addressof(out), d_res.ptr, C.sizeof(SyncRes) * max(1, rows)), "memcpy_d2h")
        return list(out)[:rows]

    def find(self, x, items):
        """x [n][in_stride] complex64 -> (rc, [SyncRes] in row order or None)."""
        a = np.ascontiguousarray(x, np.complex64)
        a = a.reshape(1, -1) if a.ndim == 1 else a
        rows = sync_rows(items)
        din, dres = DevBuf.from_host(a), DevBuf(C.sizeof(SyncRes) * max(1, rows))
        rc = self.find_device(din.ptr, a.shape[1], items, dres.ptr)
        if rc != SRSLTE_SUCCESS:
            return rc, None
        sync()
        return rc, self.read(dres, rows)

    def cp_corr(self, item):
        """The CP stage's correlations of an item of the last call (diagnostic)."""
        M = min(self.cfg.max_offset, self.cfg.fft_size)
        out = np.zeros(M, np.complex64)
        _check(lib().srslte_hip_sync_cp_corr(self.h, item, out.ctypes.data), "sync_cp_corr")
        return out

    def free(self):
        if self.h:
            lib().srslte_hip_sync_destroy(self.h)
            self.h = None


# ---------------------------------------------------------------- UE synchronisation: tracks (phy_hip.h "UE synchronisation: tracks")
FRAME_FDD, FRAME_TDD, FRAME_DETECT = 0, 1, 2
SYNC_RESET_AVG, SYNC_RESET_CFO, SYNC_RESET_REST, SYNC_RESET_ALL = 1, 2, 4, 7


class SyncTracksCfg(C.Structure):
    """srslte_hip_sync_tracks_cfg_t."""
    _fields_ = [("n_tracks", C.c_uint32), ("cfo_ema_alpha", C.c_float), ("frame_mode", C.c_uint32)]


class SyncTrackItem(C.Structure):
    """srslte_hip_sync_track_item_t."""
    _fields_ = [("track", C.c_uint32), ("N_id_2", C.c_uint32), ("find_offset", C.c_uint32), ("N_id_1", C.c_int32)]

    @classmethod
    def make(cls, track, N_id_2, find_offset=0, N_id_1=-1):
        return cls(track, N_id_2, find_offset, N_id_1)


class SyncTrackRes(C.Structure):
    """srslte_hip_sync_track_res_t: r is the SyncRes; its fields also read as attributes of the row."""
    _fields_ = [("r", SyncRes), ("frame_type", C.c_int32), ("sss_corr_trial", C.c_float * 2), ("nof_calls", C.c_uint32), ("cfo_cp_inst", C.c_float),
                ("cfo_pss_inst", C.c_float), ("M_norm_avg", C.c_float), ("M_ext_avg", C.c_float)]

    def __getattr__(self, k):
        if k in _SYNC_RES_FIELDS:
            return getattr(self.r, k)
        raise AttributeError(k)


_SYNC_RES_FIELDS = frozenset(k for k, _ in SyncRes._fields_)


class SyncTrackState(C.Structure):
    """srslte_hip_sync_track_state_t."""
    _fields_ = [("cfo_cp_mean", C.c_float), ("cfo_pss_mean", C.c_float), ("cfo_cp_is_set", C.c_uint32), ("cfo_pss_is_set", C.c_uint32),
                ("M_norm_avg", C.c_float), ("M_ext_avg", C.c_float), ("peak_value", C.c_float), ("sss_corr", C.c_float), ("cp", C.c_int32),
                ("N_id_1", C.c_int32), ("frame_type", C.c_int32), ("sf_idx", C.c_uint32), ("sss_available", C.c_uint32), ("nof_calls", C.c_uint32),
                ("cfo_cp_inst", C.c_float), ("reserved", C.c_uint32)]


def _bind_sync_tracks(L):
    vp, u32 = C.c_void_p, C.c_uint32
    _bind_sync(L)
    L.srslte_hip_sync_tracks_create.restype = vp
    L.srslte_hip_sync_tracks_create.argtypes = [vp, C.POINTER(SyncTracksCfg)]
    L.srslte_hip_sync_tracks_destroy.argtypes = [vp]
    L.srslte_hip_sync_track_batch.argtypes = [vp, vp, C.c_size_t, vp, u32, vp, vp]
    L.srslte_hip_sync_tracks_reset.argtypes = [vp, vp, u32, u32, vp]
    L.srslte_hip_sync_tracks_copy_cfo.argtypes = [vp, vp, vp, vp, u32, vp]
    L.srslte_hip_sync_tracks_read.argtypes = [vp, u32, C.POINTER(SyncTrackState)]
    L.srslte_hip_sync_tracks_check.argtypes = [C.POINTER(SyncCfg), C.POINTER(SyncTracksCfg), C.c_size_t, vp, u32]
    L.srslte_hip_cell_search_decide_ft.argtypes = [vp, u32, C.POINTER(CellSearchResult), C.POINTER(C.c_int32)]
    return L


def sync_tracks_check(cfg, tracks_cfg, in_stride, items):
    """What srslte_hip_sync_tracks_create and a tracked call with these items would answer, without a device."""
    arr = (SyncTrackItem * max(1, len(items)))(*items)
    return _bind_sync_tracks(lib()).srslte_hip_sync_tracks_check(C.byref(cfg), C.byref(tracks_cfg), in_stride, arr, len(items))


def cell_search_decide_ft(rows):
    """srslte_hip_cell_search_decide_ft (host): (number of frames that counted, CellSearchResult, frame type)."""
    arr = (SyncTrackRes * max(1, len(rows)))(*rows)
    out, ft = CellSearchResult(), C.c_int32(0)
    return _bind_sync_tracks(lib()).srslte_hip_cell_search_decide_ft(arr, len(rows), C.byref(out), C.byref(ft)), out, ft.value


def _u32_list(idx):
    return None if idx is None else (C.c_uint32 * max(1, len(idx)))(*idx)


class SyncTracks:
    """The state of n_tracks srslte_sync_t on the device, over one Sync object's configuration: one srslte_sync_find per item and call."""

    def __init__(self, sync_obj, n_tracks, cfo_ema_alpha=0.0, frame_mode=FRAME_FDD):
        L = _bind_sync_tracks(lib())
        self.sync, self.cfg = sync_obj, SyncTracksCfg(n_tracks, cfo_ema_alpha, frame_mode)
        self.h = L.srslte_hip_sync_tracks_create(sync_obj.h, C.byref(self.cfg))
        if not self.h:
            raise RuntimeError("srslte_hip_sync_tracks_create failed")

    def track_device(self, d_in, in_stride, items, d_res, stream=None):
        arr = (SyncTrackItem * max(1, len(items)))(*items)
        return lib().srslte_hip_sync_track_batch(self.h, d_in, in_stride, arr, len(items), d_res, stream)

    @staticmethod
    def read_rows(d_res, rows):
        out = (SyncTrackRes * max(1, rows))()
        _check(lib().srslte_hip_memcpy_d2h(C.addressof(out), d_res.ptr, C.sizeof(SyncTrackRes) * max(1, rows)), "memcpy_d2h")
        return list(out)[:rows]

    def track(self, x, items):
        """x [n][in_stride] complex64, item i on row i -> (rc, [SyncTrackRes] or None)."""
        a = np.ascontiguousarray(x, np.complex64)
        a = a.reshape(1, -1) if a.ndim == 1 else a
        din, dres = DevBuf.from_host(a), DevBuf(C.sizeof(SyncTrackRes) * max(1, len(items)))
        rc = self.track_device(din.ptr, a.shape[1], items, dres.ptr)
        if rc != SRSLTE_SUCCESS:
            return rc, None
        sync()
        return rc, self.read_rows(dres, len(items))

    def reset(self, idx=None, flags=SYNC_RESET_ALL, stream=None):
        return lib().srslte_hip_sync_tracks_reset(self.h, _u32_list(idx), 0 if idx is None else len(idx), flags, stream)

    def copy_cfo(self, dst_idx, src, src_idx, stream=None):
        return lib().srslte_hip_sync_tracks_copy_cfo(self.h, _u32_list(dst_idx), src.h, _u32_list(src_idx), len(dst_idx), stream)

    def state(self, track):
        out = SyncTrackState()
        _check(lib().srslte_hip_sync_tracks_read(self.h, track, C.byref(out)), "sync_tracks_read")
        return out

    def free(self):
        if self.h:
            lib().srslte_hip_sync_tracks_destroy(self.h)
            self.h = None


# ---------------------------------------------------------------- neighbour-cell measurement (phy_hip.h "Neighbour-cell measurement")
class MeasCfg(C.Structure):
    """srslte_hip_meas_cfg_t."""
    _fields_ = [("nof_prb", C.c_uint32), ("symbol_sz", C.c_uint32), ("max_captures", C.c_uint32), ("max_cells", C.c_uint32), ("max_sf", C.c_uint32),
                ("threshold", C.c_float), ("cp_ext", C.c_uint32)]


class MeasRes(C.Structure):
    """srslte_hip_meas_res_t."""
    _fields_ = [("found", C.c_int32), ("peak_index", C.c_uint32), ("sf_idx", C.c_uint32), ("nof_sf", C.c_uint32), ("peak_value", C.c_float),
                ("rms_avg", C.c_float), ("rsrp_lin", C.c_float), ("rssi_lin", C.c_float), ("rsrp_dBfs", C.c_float), ("rssi_dBfs", C.c_float),
                ("rsrq_dB", C.c_float), ("cfo_Hz", C.c_float), ("cell_id", C.c_uint32), ("capture", C.c_uint32), ("reserved", C.c_uint32 * 2)]


def _bind_meas(L):
    vp, u32 = C.c_void_p, C.c_uint32
    L.srslte_hip_meas_create.restype = vp
    L.srslte_hip_meas_create.argtypes = [C.POINTER(MeasCfg)]
    L.srslte_hip_meas_destroy.argtypes = [vp]
    L.srslte_hip_meas_set_cells.argtypes = [vp, vp, u32, vp]
    L.srslte_hip_meas_run_batch.argtypes = [vp, vp, C.c_size_t, u32, u32, vp, vp]
    L.srslte_hip_meas_check.argtypes = [C.POINTER(MeasCfg), C.c_size_t, u32, u32, u32]
    L.srslte_hip_meas_replicas.argtypes = [vp, u32, vp]
    return L


def meas_cfg(nof_prb, max_captures=1, max_cells=1, max_sf=5, symbol_sz=0, threshold=0.0, cp_ext=False):
    return MeasCfg(nof_prb, symbol_sz, max_captures, max_cells, max_sf, threshold, 1 if cp_ext else 0)


def meas_check(cfg, in_stride, nof_sf, n_captures, n_cells):
    """What srslte_hip_meas_create and a call of this shape would answer, without a device."""
    return _bind_meas(lib()).srslte_hip_meas_check(C.byref(cfg), in_stride, nof_sf, n_captures, n_cells)


class Meas:
    """Batched neighbour-cell measurement: srslte_refsignal_dl_sync_run per (capture, candidate cell)."""

    def __init__(self, nof_prb, max_captures=1, max_cells=1, max_sf=5, **kw):
        L = _bind_meas(lib())
        self.cfg = meas_cfg(nof_prb, max_captures, max_cells, max_sf, **kw)
        self.h = L.srslte_hip_meas_create(C.byref(self.cfg))
        if not self.h:
            raise RuntimeError("srslte_hip_meas_create failed")
        self.symbol_sz = self.cfg.symbol_sz or symbol_sz(nof_prb)
        self.sf_len = 15 * self.symbol_sz
        self.n_cells = 0

    def set_cells(self, cell_ids, stream=None):
        ids = np.ascontiguousarray(cell_ids, np.uint16)
        rc = lib().srslte_hip_meas_set_cells(self.h, ids.ctypes.data, ids.size, stream)
        if rc == SRSLTE_SUCCESS:
            self.n_cells = ids.size
        return rc

    def run_device(self, d_in, in_stride, nof_sf, n_captures, d_res, stream=None):
        return lib().srslte_hip_meas_run_batch(self.h, d_in, in_stride, nof_sf, n_captures, d_res, stream)

    @staticmethod
    def read(d_res, rows):
        out = (MeasRes * max(1, rows))()
        _check(lib().srslte_hip_memcpy_d2h(C.addressof(out), d_res.ptr, C.sizeof(MeasRes) * max(1, rows)), "memcpy_d2h")
        return list(out)[:rows]

    def run(self, x, nof_sf):
        """x [n_captures][in_stride] complex64 -> (rc, [MeasRes] capture-major or None)."""
        a = np.ascontiguousarray(x, np.complex64)
        a = a.reshape(1, -1) if a.ndim == 1 else a
        rows = a.shape[0] * self.n_cells
        din, dres = DevBuf.from_host(a), DevBuf(C.sizeof(MeasRes) * max(1, rows))
        rc = self.run_device(din.ptr, a.shape[1], nof_sf, a.shape[0], dres.ptr)
        if rc != SRSLTE_SUCCESS:
            return rc, None
        sync()
        return rc, self.read(dres, rows)

    def replicas(self, cell):
        """The time-domain replicas [10][sf_len] of cell `cell` of the last set_cells (diagnostic)."""
        out = np.zeros(10 * self.sf_len, np.complex64)
        _check(lib().srslte_hip_meas_replicas(self.h, cell, out.ctypes.data), "meas_replicas")
        return out.reshape(10, self.sf_len)

    def free(self):
        if self.h:
            lib().srslte_hip_meas_destroy(self.h)
            self.h = None


# ---------------------------------------------------------------- NB-IoT synchronisation (phy_hip.h "NB-IoT synchronisation")
NBIOT_REPLICA_LEN, NBIOT_NSSS_IN_LEN, NBIOT_NSSS_NOUT, NBIOT_NUM_PCI = 1508, 3840, 5346, 504


class NbiotSyncCfg(C.Structure):
    """srslte_hip_nbiot_sync_cfg_t."""
    _fields_ = [("fft_size", C.c_uint32), ("frame_size", C.c_uint32), ("max_offset", C.c_uint32), ("max_items", C.c_uint32), ("n_tracks", C.c_uint32),
                ("threshold", C.c_float), ("nsss_threshold", C.c_float), ("npss_ema_alpha", C.c_float), ("cfo_ema_alpha", C.c_float),
                ("cfo_enable", C.c_uint32)]


class NbiotNpssItem(C.Structure):
    """srslte_hip_nbiot_npss_item_t."""
    _fields_ = [("track", C.c_uint32), ("find_offset", C.c_uint32)]


class NbiotNpssRes(C.Structure):
    """srslte_hip_nbiot_npss_res_t."""
    _fields_ = [("ret", C.c_int32), ("peak_pos", C.c_uint32), ("peak_value", C.c_float), ("corr_peak", C.c_float), ("cfo", C.c_float),
                ("mean_cfo", C.c_float), ("reserved", C.c_uint32 * 2)]


class NbiotNsssRes(C.Structure):
    """srslte_hip_nbiot_nsss_res_t."""
    _fields_ = [("found", C.c_int32), ("cell_id", C.c_int32), ("peak_value", C.c_float), ("peak_pos", C.c_uint32), ("sfn_partial", C.c_uint32),
                ("reserved", C.c_uint32 * 3)]


def _bind_nbiot(L):
    vp, u32 = C.c_void_p, C.c_uint32
    L.srslte_hip_nbiot_sync_create.restype = vp
    L.srslte_hip_nbiot_sync_create.argtypes = [C.POINTER(NbiotSyncCfg)]
    L.srslte_hip_nbiot_sync_destroy.argtypes = [vp]
    L.srslte_hip_nbiot_sync_tracks_reset.argtypes = [vp, u32, u32, vp]
    L.srslte_hip_nbiot_sync_tracks_set_cfo.argtypes = [vp, u32, u32, vp, vp]
    L.srslte_hip_nbiot_sync_tracks_read.argtypes = [vp, u32, vp, vp]
    L.srslte_hip_nbiot_npss_find_batch.argtypes = [vp, vp, C.c_size_t, vp, u32, vp, vp]
    L.srslte_hip_nbiot_nsss_find_batch.argtypes = [vp, vp, C.c_size_t, vp, u32, vp, vp]
    L.srslte_hip_nbiot_nsss_debug.argtypes = [vp, u32, vp, vp]
    L.srslte_hip_nbiot_sync_check.argtypes = [C.POINTER(NbiotSyncCfg), C.c_size_t, vp, u32]
    L.srslte_hip_nbiot_nsss_check.argtypes = [C.POINTER(NbiotSyncCfg), C.c_size_t, vp, u32]
    L.srslte_hip_nbiot_npss_nout.restype = u32
    L.srslte_hip_nbiot_npss_nout.argtypes = [u32]
    L.srslte_hip_nbiot_npss_generate.argtypes = [vp]
    L.srslte_hip_nbiot_nsss_generate.argtypes = [vp, u32]
    L.srslte_hip_nbiot_npss_replica.argtypes = [vp]
    L.srslte_hip_nbiot_nsss_replica.argtypes = [vp, u32]
    L.srslte_hip_nbiot_npss_re.argtypes = [u32, u32, vp]
    L.srslte_hip_nbiot_nsss_re.argtypes = [u32, u32, C.c_int, vp, C.POINTER(u32)]
    return L


def nbiot_sync_cfg(frame_size, max_offset=128, max_items=1, n_tracks=1, threshold=0.0, nsss_threshold=0.0, npss_ema_alpha=0.0, cfo_ema_alpha=0.0,
                   cfo_enable=True, fft_size=128):
    """The zeros select the defaults of srslte_sync_nbiot_init / srslte_npss_synch_init / srslte_nsss_synch_init."""
    return NbiotSyncCfg(fft_size, frame_size, max_offset, max_items, n_tracks, threshold, nsss_threshold, npss_ema_alpha, cfo_ema_alpha,
                        int(bool(cfo_enable)))


def nbiot_sync_check(cfg, in_stride, items):
    """What srslte_hip_nbiot_sync_create and an NPSS call with these items would answer, without a device."""
    arr = (NbiotNpssItem * max(1, len(items)))(*items)
    return _bind_nbiot(lib()).srslte_hip_nbiot_sync_check(C.byref(cfg), in_stride, arr, len(items))


def nbiot_nsss_check(cfg, in_stride, cell_ids):
    ids = np.ascontiguousarray(cell_ids, np.int32)
    return _bind_nbiot(lib()).srslte_hip_nbiot_nsss_check(C.byref(cfg), in_stride, ids.ctypes.data, ids.size)


def nbiot_npss_nout(frame_size):
    return _bind_nbiot(lib()).srslte_hip_nbiot_npss_nout(frame_size)


def nbiot_npss_generate():
    out = np.zeros(121, np.complex64)
    _check(_bind_nbiot(lib()).srslte_hip_nbiot_npss_generate(out.ctypes.data), "nbiot_npss_generate")
    return out


def nbiot_nsss_generate(cell_id):
    out = np.zeros(528, np.complex64)
    _check(_bind_nbiot(lib()).srslte_hip_nbiot_nsss_generate(out.ctypes.data, cell_id), "nbiot_nsss_generate")
    return out


def nbiot_npss_replica():
    out = np.zeros(NBIOT_REPLICA_LEN, np.complex64)
    _check(_bind_nbiot(lib()).srslte_hip_nbiot_npss_replica(out.ctypes.data), "nbiot_npss_replica")
    return out


def nbiot_nsss_replica(cell_id):
    out = np.zeros(NBIOT_REPLICA_LEN, np.complex64)
    _check(_bind_nbiot(lib()).srslte_hip_nbiot_nsss_replica(out.ctypes.data, cell_id), "nbiot_nsss_replica")
    return out


def nbiot_npss_re(nof_prb, prb_offset=0):
    """RE indices of srslte_npss_put_subframe in a subframe grid [14][12 nof_prb]: entry i receives NPSS value i."""
    re = np.zeros(121, np.uint32)
    _check(_bind_nbiot(lib()).srslte_hip_nbiot_npss_re(nof_prb, prb_offset, re.ctypes.data), "nbiot_npss_re")
    return re


def nbiot_nsss_re(nof_prb, prb_offset=0, nf=0):
    """(RE indices of srslte_nsss_put_subframe, index of the first of the 528 NSSS values frame nf carries)."""
    re, first = np.zeros(132, np.uint32), C.c_uint32(0)
    _check(_bind_nbiot(lib()).srslte_hip_nbiot_nsss_re(nof_prb, prb_offset, nf, re.ctypes.data, C.byref(first)), "nbiot_nsss_re")
    return re, first.value


class NbiotSync:
    """Batched NB-IoT synchronisation: srslte_sync_nbiot_find per item on device-resident tracks, and srslte_nsss_sync_find per capture."""

    def __init__(self, frame_size, **kw):
        L = _bind_nbiot(lib())
        self.cfg = nbiot_sync_cfg(frame_size, **kw)
        self.h = L.srslte_hip_nbiot_sync_create(C.byref(self.cfg))
        if not self.h:
            raise RuntimeError("srslte_hip_nbiot_sync_create failed")
        self.nout = L.srslte_hip_nbiot_npss_nout(frame_size)

    def npss_device(self, d_in, in_stride, items, d_res, stream=None):
        arr = (NbiotNpssItem * max(1, len(items)))(*items)
        return lib().srslte_hip_nbiot_npss_find_batch(self.h, d_in, in_stride, arr, len(items), d_res, stream)

    def nsss_device(self, d_in, in_stride, cell_ids, d_res, stream=None):
        ids = np.ascontiguousarray(cell_ids, np.int32)
        return lib().srslte_hip_nbiot_nsss_find_batch(self.h, d_in, in_stride, ids.ctypes.data, ids.size, d_res, stream)

    @staticmethod
    def read(d_res, rows, cls):
        out = (cls * max(1, rows))()
        _check(lib().srslte_hip_memcpy_d2h(C.addressof(out), d_res.ptr, C.sizeof(cls) * max(1, rows)), "memcpy_d2h")
        return list(out)[:rows]

    def npss_find(self, x, items):
        """x [n][in_stride] complex64, items [(track, find_offset)] -> (rc, [NbiotNpssRes] or None)."""
        a = np.ascontiguousarray(x, np.complex64)
        a = a.reshape(1, -1) if a.ndim == 1 else a
        its = [NbiotNpssItem(*it) for it in items]
        din, dres = DevBuf.from_host(a), DevBuf(C.sizeof(NbiotNpssRes) * max(1, len(its)))
        rc = self.npss_device(din.ptr, a.shape[1], its, dres.ptr)
        if rc != SRSLTE_SUCCESS:
            return rc, None
        sync()
        return rc, self.read(dres, len(its), NbiotNpssRes)

    def nsss_find(self, x, cell_ids):
        """x [n][in_stride] complex64, cell_ids [n] (-1: all 504) -> (rc, [NbiotNsssRes] or None)."""
        a = np.ascontiguousarray(x, np.complex64)
        a = a.reshape(1, -1) if a.ndim == 1 else a
        din, dres = DevBuf.from_host(a), DevBuf(C.sizeof(NbiotNsssRes) * max(1, len(cell_ids)))
        rc = self.nsss_device(din.ptr, a.shape[1], cell_ids, dres.ptr)
        if rc != SRSLTE_SUCCESS:
            return rc, None
        sync()
        return rc, self.read(dres, len(cell_ids), NbiotNsssRes)

    def nsss_debug(self, item):
        """(peak_values [504], the |c| row [5346] of the row's cell id) of an item of the last NSSS call."""
        pv, row = np.zeros(NBIOT_NUM_PCI, np.float32), np.zeros(NBIOT_NSSS_NOUT, np.float32)
        _check(lib().srslte_hip_nbiot_nsss_debug(self.h, item, pv.ctypes.data, row.ctypes.data), "nbiot_nsss_debug")
        return pv, row

    def tracks_reset(self, first=0, n=None, stream=None):
        return lib().srslte_hip_nbiot_sync_tracks_reset(self.h, first, self.cfg.n_tracks - first if n is None else n, stream)

    def tracks_set_cfo(self, first, cfo, stream=None):
        v = np.ascontiguousarray(cfo, np.float32).reshape(-1)
        return lib().srslte_hip_nbiot_sync_tracks_set_cfo(self.h, first, v.size, v.ctypes.data, stream)

    def track(self, k):
        """(mean_cfo, the averaged |c|^2 [nout]) of track k."""
        m, avg = np.zeros(1, np.float32), np.zeros(max(1, self.nout), np.float32)
        _check(lib().srslte_hip_nbiot_sync_tracks_read(self.h, k, m.ctypes.data, avg.ctypes.data), "nbiot_sync_tracks_read")
        return float(m[0]), avg[:self.nout]

    def free(self):
        if self.h:
            lib().srslte_hip_nbiot_sync_destroy(self.h)
            self.h = None


# ---------------------------------------------------------------- PUSCH UCI plan (phy_hip.h "PUSCH UCI plan")
PUSCH_UCI_OK, PUSCH_UCI_EMPTY, PUSCH_UCI_BETA, PUSCH_UCI_ROWS, PUSCH_UCI_NO_ROOM = range(5)


class PuschUciCfg(C.Structure):
    """srslte_hip_pusch_uci_cfg_t."""
    _fields_ = [(n, C.c_uint32) for n in ("L_prb", "nof_symb", "Qm", "rows", "K_segm", "C", "ack_len", "ri_len", "cqi_len", "I_offset_ack",
                                          "I_offset_ri", "I_offset_cqi", "sym")]


class PuschUciRes(C.Structure):
    """srslte_hip_pusch_uci_res_t."""
    _fields_ = [(n, C.c_uint32) for n in ("Qp_ack", "Qp_ri", "Qp_cqi", "Q_cqi", "G_prime", "syms_lo", "C_lo")] + [("ack_pos", C.c_uint32 * 2),
                                                                                                                ("ri_pos", C.c_uint32 * 2)]


def pusch_uci_plan(**cfg):
    """(reason, PuschUciRes) of srslte_hip_pusch_uci_plan for the fields of srslte_hip_pusch_uci_cfg_t given by name, without a device."""
    L = lib()
    L.srslte_hip_pusch_uci_plan.argtypes = [C.POINTER(PuschUciCfg), C.POINTER(PuschUciRes)]
    res = PuschUciRes()
    return L.srslte_hip_pusch_uci_plan(C.byref(PuschUciCfg(**cfg)), C.byref(res)), res
