"""UE synchronisation: PSS / SSS search with CFO, its tracks across calls, neighbour-cell measurement and NB-IoT NPSS / NSSS search."""
import ctypes as C

import numpy as np

from ._native import (SRSLTE_SUCCESS, DevBuf, Handle, P, _check, cint, i32, lib, read_structs, result_structs, struct_array, symbol_sz, sync, sz, u32, upload_rows, void,
                      vp)

# ---------------------------------------------------------------- UE synchronisation (phy_hip.h "UE synchronisation")
SYNC_FOUND, SYNC_FOUND_NOSPACE, SYNC_NOFOUND = 1, 2, 0
SSS_DIFF, SSS_PARTIAL_3, SSS_FULL = 0, 1, 2


class SyncCfg(C.Structure):
    """srslte_hip_sync_cfg_t."""
    C_TYPE = "srslte_hip_sync_cfg_t"
    _fields_ = [("fft_size", C.c_uint32), ("frame_size", C.c_uint32), ("max_offset", C.c_uint32), ("max_items", C.c_uint32), ("cp", C.c_int),
                ("detect_cp", C.c_uint8), ("sss_en", C.c_uint8), ("cfo_cp_enable", C.c_uint8), ("cfo_pss_enable", C.c_uint8),
                ("pss_filt_enable", C.c_uint8), ("sss_alg", C.c_uint8), ("tdd", C.c_uint8), ("reserved", C.c_uint8), ("cfo_cp_nsymbols", C.c_uint32),
                ("threshold", C.c_float), ("sss_threshold", C.c_float), ("ema_alpha", C.c_float), ("decimate", C.c_uint32)]


class SyncItem(C.Structure):
    """srslte_hip_sync_item_t."""
    C_TYPE = "srslte_hip_sync_item_t"
    _fields_ = [("N_id_2", C.c_uint32), ("find_offset", C.c_uint32), ("N_id_1", C.c_int32)]

    @classmethod
    def make(cls, N_id_2, find_offset=0, N_id_1=-1):
        return cls(N_id_2, find_offset, N_id_1)


class SyncRes(C.Structure):
    """srslte_hip_sync_res_t."""
    C_TYPE = "srslte_hip_sync_res_t"
    _fields_ = [("ret", C.c_int32), ("peak_pos", C.c_uint32), ("peak_value", C.c_float), ("corr_peak", C.c_float), ("cfo_cp", C.c_float),
                ("cfo_pss", C.c_float), ("cfo", C.c_float), ("sss_available", C.c_uint32), ("sss_detected", C.c_uint32), ("m0", C.c_uint32),
                ("m1", C.c_uint32), ("sf_idx", C.c_uint32), ("N_id_1", C.c_int32), ("cell_id", C.c_int32), ("sss_corr", C.c_float), ("cp", C.c_int32)]


class CellSearchResult(C.Structure):
    """srslte_hip_cell_search_result_t."""
    C_TYPE = "srslte_hip_cell_search_result_t"
    _fields_ = [("cell_id", C.c_uint32), ("cp", C.c_int), ("peak", C.c_float), ("mode", C.c_float), ("psr", C.c_float), ("cfo", C.c_float),
                ("nof_frames", C.c_uint32)]


# ---------------------------------------------------------------- UE synchronisation: tracks (phy_hip.h "UE synchronisation: tracks")
FRAME_FDD, FRAME_TDD, FRAME_DETECT = 0, 1, 2
SYNC_RESET_AVG, SYNC_RESET_CFO, SYNC_RESET_REST, SYNC_RESET_ALL = 1, 2, 4, 7


class SyncTracksCfg(C.Structure):
    """srslte_hip_sync_tracks_cfg_t."""
    C_TYPE = "srslte_hip_sync_tracks_cfg_t"
    _fields_ = [("n_tracks", C.c_uint32), ("cfo_ema_alpha", C.c_float), ("frame_mode", C.c_uint32)]


class SyncTrackItem(C.Structure):
    """srslte_hip_sync_track_item_t."""
    C_TYPE = "srslte_hip_sync_track_item_t"
    _fields_ = [("track", C.c_uint32), ("N_id_2", C.c_uint32), ("find_offset", C.c_uint32), ("N_id_1", C.c_int32)]

    @classmethod
    def make(cls, track, N_id_2, find_offset=0, N_id_1=-1):
        return cls(track, N_id_2, find_offset, N_id_1)


class SyncTrackRes(C.Structure):
    """srslte_hip_sync_track_res_t: r is the SyncRes; its fields also read as attributes of the row."""
    C_TYPE = "srslte_hip_sync_track_res_t"
    _fields_ = [("r", SyncRes), ("frame_type", C.c_int32), ("sss_corr_trial", C.c_float * 2), ("nof_calls", C.c_uint32), ("cfo_cp_inst", C.c_float),
                ("cfo_pss_inst", C.c_float), ("M_norm_avg", C.c_float), ("M_ext_avg", C.c_float)]

    def __getattr__(self, k):
        if k in _SYNC_RES_FIELDS:
            return getattr(self.r, k)
        raise AttributeError(k)


_SYNC_RES_FIELDS = frozenset(k for k, _ in SyncRes._fields_)


class SyncTrackState(C.Structure):
    """srslte_hip_sync_track_state_t."""
    C_TYPE = "srslte_hip_sync_track_state_t"
    _fields_ = [("cfo_cp_mean", C.c_float), ("cfo_pss_mean", C.c_float), ("cfo_cp_is_set", C.c_uint32), ("cfo_pss_is_set", C.c_uint32),
                ("M_norm_avg", C.c_float), ("M_ext_avg", C.c_float), ("peak_value", C.c_float), ("sss_corr", C.c_float), ("cp", C.c_int32),
                ("N_id_1", C.c_int32), ("frame_type", C.c_int32), ("sf_idx", C.c_uint32), ("sss_available", C.c_uint32), ("nof_calls", C.c_uint32),
                ("cfo_cp_inst", C.c_float), ("reserved", C.c_uint32)]


# ---------------------------------------------------------------- neighbour-cell measurement (phy_hip.h "Neighbour-cell measurement")
class MeasCfg(C.Structure):
    """srslte_hip_meas_cfg_t."""
    C_TYPE = "srslte_hip_meas_cfg_t"
    _fields_ = [("nof_prb", C.c_uint32), ("symbol_sz", C.c_uint32), ("max_captures", C.c_uint32), ("max_cells", C.c_uint32), ("max_sf", C.c_uint32),
                ("threshold", C.c_float), ("cp_ext", C.c_uint32)]


class MeasRes(C.Structure):
    """srslte_hip_meas_res_t."""
    C_TYPE = "srslte_hip_meas_res_t"
    _fields_ = [("found", C.c_int32), ("peak_index", C.c_uint32), ("sf_idx", C.c_uint32), ("nof_sf", C.c_uint32), ("peak_value", C.c_float),
                ("rms_avg", C.c_float), ("rsrp_lin", C.c_float), ("rssi_lin", C.c_float), ("rsrp_dBfs", C.c_float), ("rssi_dBfs", C.c_float),
                ("rsrq_dB", C.c_float), ("cfo_Hz", C.c_float), ("cell_id", C.c_uint32), ("capture", C.c_uint32), ("reserved", C.c_uint32 * 2)]


# ---------------------------------------------------------------- NB-IoT synchronisation (phy_hip.h "NB-IoT synchronisation")
NBIOT_REPLICA_LEN, NBIOT_NSSS_IN_LEN, NBIOT_NSSS_NOUT, NBIOT_NUM_PCI = 1508, 3840, 5346, 504


class NbiotSyncCfg(C.Structure):
    """srslte_hip_nbiot_sync_cfg_t."""
    C_TYPE = "srslte_hip_nbiot_sync_cfg_t"
    _fields_ = [("fft_size", C.c_uint32), ("frame_size", C.c_uint32), ("max_offset", C.c_uint32), ("max_items", C.c_uint32), ("n_tracks", C.c_uint32),
                ("threshold", C.c_float), ("nsss_threshold", C.c_float), ("npss_ema_alpha", C.c_float), ("cfo_ema_alpha", C.c_float),
                ("cfo_enable", C.c_uint32)]


class NbiotNpssItem(C.Structure):
    """srslte_hip_nbiot_npss_item_t."""
    C_TYPE = "srslte_hip_nbiot_npss_item_t"
    _fields_ = [("track", C.c_uint32), ("find_offset", C.c_uint32)]


class NbiotNpssRes(C.Structure):
    """srslte_hip_nbiot_npss_res_t."""
    C_TYPE = "srslte_hip_nbiot_npss_res_t"
    _fields_ = [("ret", C.c_int32), ("peak_pos", C.c_uint32), ("peak_value", C.c_float), ("corr_peak", C.c_float), ("cfo", C.c_float),
                ("mean_cfo", C.c_float), ("reserved", C.c_uint32 * 2)]


class NbiotNsssRes(C.Structure):
    """srslte_hip_nbiot_nsss_res_t."""
    C_TYPE = "srslte_hip_nbiot_nsss_res_t"
    _fields_ = [("found", C.c_int32), ("cell_id", C.c_int32), ("peak_value", C.c_float), ("peak_pos", C.c_uint32), ("sfn_partial", C.c_uint32),
                ("reserved", C.c_uint32 * 3)]


_FIND = [vp, vp, sz, vp, u32, vp, vp]

SIGNATURES = {
    # UE synchronisation
    "srslte_hip_sync_create": (vp, [P(SyncCfg)]),
    "srslte_hip_sync_destroy": (void, [vp]),
    "srslte_hip_sync_find_batch": (None, _FIND),
    "srslte_hip_cfo_correct_batch": (None, [vp, vp, sz, u32, u32, vp, vp]),
    "srslte_hip_sync_check": (None, [P(SyncCfg), sz, vp, u32]),
    "srslte_hip_cell_search_decide": (None, [vp, u32, P(CellSearchResult)]),
    "srslte_hip_sync_cp_corr": (None, [vp, u32, vp]),
    # UE synchronisation: tracks
    "srslte_hip_sync_tracks_create": (vp, [vp, P(SyncTracksCfg)]),
    "srslte_hip_sync_tracks_destroy": (void, [vp]),
    "srslte_hip_sync_track_batch": (None, _FIND),
    "srslte_hip_sync_tracks_reset": (None, [vp, vp, u32, u32, vp]),
    "srslte_hip_sync_tracks_copy_cfo": (None, [vp, vp, vp, vp, u32, vp]),
    "srslte_hip_sync_tracks_read": (None, [vp, u32, P(SyncTrackState)]),
    "srslte_hip_sync_tracks_check": (None, [P(SyncCfg), P(SyncTracksCfg), sz, vp, u32]),
    "srslte_hip_cell_search_decide_ft": (None, [vp, u32, P(CellSearchResult), P(i32)]),
    # neighbour-cell measurement
    "srslte_hip_meas_create": (vp, [P(MeasCfg)]),
    "srslte_hip_meas_destroy": (void, [vp]),
    "srslte_hip_meas_set_cells": (None, [vp, vp, u32, vp]),
    "srslte_hip_meas_run_batch": (None, [vp, vp, sz, u32, u32, vp, vp]),
    "srslte_hip_meas_check": (None, [P(MeasCfg), sz, u32, u32, u32]),
    "srslte_hip_meas_replicas": (None, [vp, u32, vp]),
    # NB-IoT synchronisation
    "srslte_hip_nbiot_sync_create": (vp, [P(NbiotSyncCfg)]),
    "srslte_hip_nbiot_sync_destroy": (void, [vp]),
    "srslte_hip_nbiot_sync_tracks_reset": (None, [vp, u32, u32, vp]),
    "srslte_hip_nbiot_sync_tracks_set_cfo": (None, [vp, u32, u32, vp, vp]),
    "srslte_hip_nbiot_sync_tracks_read": (None, [vp, u32, vp, vp]),
    "srslte_hip_nbiot_npss_find_batch": (None, _FIND),
    "srslte_hip_nbiot_nsss_find_batch": (None, _FIND),
    "srslte_hip_nbiot_nsss_debug": (None, [vp, u32, vp, vp]),
    "srslte_hip_nbiot_sync_check": (None, [P(NbiotSyncCfg), sz, vp, u32]),
    "srslte_hip_nbiot_nsss_check": (None, [P(NbiotSyncCfg), sz, vp, u32]),
    "srslte_hip_nbiot_npss_nout": (u32, [u32]),
    "srslte_hip_nbiot_npss_generate": (None, [vp]),
    "srslte_hip_nbiot_nsss_generate": (None, [vp, u32]),
    "srslte_hip_nbiot_npss_replica": (None, [vp]),
    "srslte_hip_nbiot_nsss_replica": (None, [vp, u32]),
    "srslte_hip_nbiot_npss_re": (None, [u32, u32, vp]),
    "srslte_hip_nbiot_nsss_re": (None, [u32, u32, cint, vp, P(u32)]),
}


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
    return lib().srslte_hip_sync_check(C.byref(cfg), in_stride, struct_array(SyncItem, items), len(items))


def cell_search_decide(rows):
    """srslte_hip_cell_search_decide (host): (number of frames that counted, CellSearchResult)."""
    out = CellSearchResult()
    return lib().srslte_hip_cell_search_decide(struct_array(SyncRes, rows), len(rows), C.byref(out)), out


def cfo_correct_device(d_in, d_out, stride, length, n, freq, stream=None):
    f = np.ascontiguousarray(freq, np.float32)
    return lib().srslte_hip_cfo_correct_batch(d_in, d_out, stride, length, n, f.ctypes.data, stream)


def cfo_correct(x, freq, in_place=False):
    """x [n][len] complex64, freq [n] cycles per sample -> x exp(j 2 pi freq i) from the device."""
    a, din = upload_rows(x)
    dout = din if in_place else DevBuf(a.nbytes)
    _check(cfo_correct_device(din.ptr, dout.ptr, a.shape[1], a.shape[1], a.shape[0], freq), "cfo_correct_batch")
    sync()
    return dout.to_host(np.complex64).reshape(a.shape)


class Sync(Handle):
    """Batched PSS / SSS synchronisation: the first srslte_sync_find of a reset object per item."""
    DESTROY = "srslte_hip_sync_destroy"

    def __init__(self, fft_size, frame_size, max_offset, max_items=1, **kw):
        self.cfg = sync_cfg(fft_size, frame_size, max_offset, max_items=max_items, **kw)
        self._create("srslte_hip_sync_create", C.byref(self.cfg))

    def find_device(self, d_in, in_stride, items, d_res, stream=None):
        return lib().srslte_hip_sync_find_batch(self.h, d_in, in_stride, struct_array(SyncItem, items), len(items), d_res, stream)

    @staticmethod
    def read(d_res, rows):
        return read_structs(d_res.ptr, SyncRes, rows)

    def find(self, x, items):
        """x [n][in_stride] complex64 -> (rc, [SyncRes] in row order or None)."""
        a, din = upload_rows(x)
        rows = sync_rows(items)
        dres = DevBuf(C.sizeof(SyncRes) * max(1, rows))
        return result_structs(self.find_device(din.ptr, a.shape[1], items, dres.ptr), dres.ptr, SyncRes, rows)

    def cp_corr(self, item):
        """The CP stage's correlations of an item of the last call (diagnostic)."""
        M = min(self.cfg.max_offset, self.cfg.fft_size)
        out = np.zeros(M, np.complex64)
        _check(lib().srslte_hip_sync_cp_corr(self.h, item, out.ctypes.data), "sync_cp_corr")
        return out


def sync_tracks_check(cfg, tracks_cfg, in_stride, items):
    """What srslte_hip_sync_tracks_create and a tracked call with these items would answer, without a device."""
    return lib().srslte_hip_sync_tracks_check(C.byref(cfg), C.byref(tracks_cfg), in_stride, struct_array(SyncTrackItem, items), len(items))


def cell_search_decide_ft(rows):
    """srslte_hip_cell_search_decide_ft (host): (number of frames that counted, CellSearchResult, frame type)."""
    out, ft = CellSearchResult(), C.c_int32(0)
    return lib().srslte_hip_cell_search_decide_ft(struct_array(SyncTrackRes, rows), len(rows), C.byref(out), C.byref(ft)), out, ft.value


def _u32_list(idx):
    return None if idx is None else (C.c_uint32 * max(1, len(idx)))(*idx)


class SyncTracks(Handle):
    """The state of n_tracks srslte_sync_t on the device, over one Sync object's configuration: one srslte_sync_find per item and call."""
    DESTROY = "srslte_hip_sync_tracks_destroy"

    def __init__(self, sync_obj, n_tracks, cfo_ema_alpha=0.0, frame_mode=FRAME_FDD):
        self.sync, self.cfg = sync_obj, SyncTracksCfg(n_tracks, cfo_ema_alpha, frame_mode)
        self._create("srslte_hip_sync_tracks_create", sync_obj.h, C.byref(self.cfg))

    def track_device(self, d_in, in_stride, items, d_res, stream=None):
        return lib().srslte_hip_sync_track_batch(self.h, d_in, in_stride, struct_array(SyncTrackItem, items), len(items), d_res, stream)

    @staticmethod
    def read_rows(d_res, rows):
        return read_structs(d_res.ptr, SyncTrackRes, rows)

    def track(self, x, items):
        """x [n][in_stride] complex64, item i on row i -> (rc, [SyncTrackRes] or None)."""
        a, din = upload_rows(x)
        dres = DevBuf(C.sizeof(SyncTrackRes) * max(1, len(items)))
        return result_structs(self.track_device(din.ptr, a.shape[1], items, dres.ptr), dres.ptr, SyncTrackRes, len(items))

    def reset(self, idx=None, flags=SYNC_RESET_ALL, stream=None):
        return lib().srslte_hip_sync_tracks_reset(self.h, _u32_list(idx), 0 if idx is None else len(idx), flags, stream)

    def copy_cfo(self, dst_idx, src, src_idx, stream=None):
        return lib().srslte_hip_sync_tracks_copy_cfo(self.h, _u32_list(dst_idx), src.h, _u32_list(src_idx), len(dst_idx), stream)

    def state(self, track):
        out = SyncTrackState()
        _check(lib().srslte_hip_sync_tracks_read(self.h, track, C.byref(out)), "sync_tracks_read")
        return out


def meas_cfg(nof_prb, max_captures=1, max_cells=1, max_sf=5, symbol_sz=0, threshold=0.0, cp_ext=False):
    return MeasCfg(nof_prb, symbol_sz, max_captures, max_cells, max_sf, threshold, 1 if cp_ext else 0)


def meas_check(cfg, in_stride, nof_sf, n_captures, n_cells):
    """What srslte_hip_meas_create and a call of this shape would answer, without a device."""
    return lib().srslte_hip_meas_check(C.byref(cfg), in_stride, nof_sf, n_captures, n_cells)


class Meas(Handle):
    """Batched neighbour-cell measurement: srslte_refsignal_dl_sync_run per (capture, candidate cell)."""
    DESTROY = "srslte_hip_meas_destroy"

    def __init__(self, nof_prb, max_captures=1, max_cells=1, max_sf=5, **kw):
        self.cfg = meas_cfg(nof_prb, max_captures, max_cells, max_sf, **kw)
        self._create("srslte_hip_meas_create", C.byref(self.cfg))
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
        return read_structs(d_res.ptr, MeasRes, rows)

    def run(self, x, nof_sf):
        """x [n_captures][in_stride] complex64 -> (rc, [MeasRes] capture-major or None)."""
        a, din = upload_rows(x)
        rows = a.shape[0] * self.n_cells
        dres = DevBuf(C.sizeof(MeasRes) * max(1, rows))
        return result_structs(self.run_device(din.ptr, a.shape[1], nof_sf, a.shape[0], dres.ptr), dres.ptr, MeasRes, rows)

    def replicas(self, cell):
        """The time-domain replicas [10][sf_len] of cell `cell` of the last set_cells (diagnostic)."""
        out = np.zeros(10 * self.sf_len, np.complex64)
        _check(lib().srslte_hip_meas_replicas(self.h, cell, out.ctypes.data), "meas_replicas")
        return out.reshape(10, self.sf_len)


def nbiot_sync_cfg(frame_size, max_offset=128, max_items=1, n_tracks=1, threshold=0.0, nsss_threshold=0.0, npss_ema_alpha=0.0, cfo_ema_alpha=0.0,
                   cfo_enable=True, fft_size=128):
    """The zeros select the defaults of srslte_sync_nbiot_init / srslte_npss_synch_init / srslte_nsss_synch_init."""
    return NbiotSyncCfg(fft_size, frame_size, max_offset, max_items, n_tracks, threshold, nsss_threshold, npss_ema_alpha, cfo_ema_alpha,
                        int(bool(cfo_enable)))


def nbiot_sync_check(cfg, in_stride, items):
    """What srslte_hip_nbiot_sync_create and an NPSS call with these items would answer, without a device."""
    return lib().srslte_hip_nbiot_sync_check(C.byref(cfg), in_stride, struct_array(NbiotNpssItem, items), len(items))


def nbiot_nsss_check(cfg, in_stride, cell_ids):
    ids = np.ascontiguousarray(cell_ids, np.int32)
    return lib().srslte_hip_nbiot_nsss_check(C.byref(cfg), in_stride, ids.ctypes.data, ids.size)


def nbiot_npss_nout(frame_size):
    return lib().srslte_hip_nbiot_npss_nout(frame_size)


def nbiot_npss_generate():
    out = np.zeros(121, np.complex64)
    _check(lib().srslte_hip_nbiot_npss_generate(out.ctypes.data), "nbiot_npss_generate")
    return out


def nbiot_nsss_generate(cell_id):
    out = np.zeros(528, np.complex64)
    _check(lib().srslte_hip_nbiot_nsss_generate(out.ctypes.data, cell_id), "nbiot_nsss_generate")
    return out


def nbiot_npss_replica():
    out = np.zeros(NBIOT_REPLICA_LEN, np.complex64)
    _check(lib().srslte_hip_nbiot_npss_replica(out.ctypes.data), "nbiot_npss_replica")
    return out


def nbiot_nsss_replica(cell_id):
    out = np.zeros(NBIOT_REPLICA_LEN, np.complex64)
    _check(lib().srslte_hip_nbiot_nsss_replica(out.ctypes.data, cell_id), "nbiot_nsss_replica")
    return out


def nbiot_npss_re(nof_prb, prb_offset=0):
    """RE indices of srslte_npss_put_subframe in a subframe grid [14][12 nof_prb]: entry i receives NPSS value i."""
    re = np.zeros(121, np.uint32)
    _check(lib().srslte_hip_nbiot_npss_re(nof_prb, prb_offset, re.ctypes.data), "nbiot_npss_re")
    return re


def nbiot_nsss_re(nof_prb, prb_offset=0, nf=0):
    """(RE indices of srslte_nsss_put_subframe, index of the first of the 528 NSSS values frame nf carries)."""
    re, first = np.zeros(132, np.uint32), C.c_uint32(0)
    _check(lib().srslte_hip_nbiot_nsss_re(nof_prb, prb_offset, nf, re.ctypes.data, C.byref(first)), "nbiot_nsss_re")
    return re, first.value


class NbiotSync(Handle):
    """Batched NB-IoT synchronisation: srslte_sync_nbiot_find per item on device-resident tracks, and srslte_nsss_sync_find per capture."""
    DESTROY = "srslte_hip_nbiot_sync_destroy"

    def __init__(self, frame_size, **kw):
        self.cfg = nbiot_sync_cfg(frame_size, **kw)
        self._create("srslte_hip_nbiot_sync_create", C.byref(self.cfg))
        self.nout = lib().srslte_hip_nbiot_npss_nout(frame_size)

    def npss_device(self, d_in, in_stride, items, d_res, stream=None):
        return lib().srslte_hip_nbiot_npss_find_batch(self.h, d_in, in_stride, struct_array(NbiotNpssItem, items), len(items), d_res, stream)

    def nsss_device(self, d_in, in_stride, cell_ids, d_res, stream=None):
        ids = np.ascontiguousarray(cell_ids, np.int32)
        return lib().srslte_hip_nbiot_nsss_find_batch(self.h, d_in, in_stride, ids.ctypes.data, ids.size, d_res, stream)

    @staticmethod
    def read(d_res, rows, cls):
        return read_structs(d_res.ptr, cls, rows)

    def npss_find(self, x, items):
        """x [n][in_stride] complex64, items [(track, find_offset)] -> (rc, [NbiotNpssRes] or None)."""
        a, din = upload_rows(x)
        its = [NbiotNpssItem(*it) for it in items]
        dres = DevBuf(C.sizeof(NbiotNpssRes) * max(1, len(its)))
        return result_structs(self.npss_device(din.ptr, a.shape[1], its, dres.ptr), dres.ptr, NbiotNpssRes, len(its))

    def nsss_find(self, x, cell_ids):
        """x [n][in_stride] complex64, cell_ids [n] (-1: all 504) -> (rc, [NbiotNsssRes] or None)."""
        a, din = upload_rows(x)
        dres = DevBuf(C.sizeof(NbiotNsssRes) * max(1, len(cell_ids)))
        return result_structs(self.nsss_device(din.ptr, a.shape[1], cell_ids, dres.ptr), dres.ptr, NbiotNsssRes, len(cell_ids))

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
