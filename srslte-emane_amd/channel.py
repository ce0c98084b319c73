"""The channel emulator (phy_hip.h "channel emulator"): fading, delay, HST, RLF and AWGN on batches of blocks."""
import ctypes as C

import numpy as np

from ._native import SRSLTE_SUCCESS, DevBuf, Handle, P, _check, cint, f32, f64, i64, lib, sync, u32, u64, void, vp

CHANNEL_FADING_NONE, CHANNEL_FADING_EPA, CHANNEL_FADING_EVA, CHANNEL_FADING_ETU = range(4)
CHANNEL_MAXTAPS = 9
_CHANNEL_MODELS = {"none": CHANNEL_FADING_NONE, "epa": CHANNEL_FADING_EPA, "eva": CHANNEL_FADING_EVA, "etu": CHANNEL_FADING_ETU}


class ChannelCfg(C.Structure):
    """srslte_hip_channel_cfg_t (phy_hip.h)."""
    C_TYPE = "srslte_hip_channel_cfg_t"
    _fields_ = [("srate_hz", C.c_double), ("nof_channels", C.c_uint32), ("max_calls", C.c_uint32), ("max_len", C.c_uint32),
                ("fading_enable", C.c_int), ("fading_model", C.c_int), ("doppler_hz", C.c_float), ("seed0", C.c_uint32), ("seed_stride", C.c_uint32),
                ("delay_enable", C.c_int), ("delay_min_us", C.c_float), ("delay_max_us", C.c_float), ("delay_period_s", C.c_float),
                ("delay_init_time_s", C.c_float),
                ("hst_enable", C.c_int), ("hst_fd_hz", C.c_float), ("hst_period_s", C.c_float), ("hst_init_time_s", C.c_float),
                ("rlf_enable", C.c_int), ("rlf_t_on_ms", C.c_uint32), ("rlf_t_off_ms", C.c_uint32),
                ("awgn_enable", C.c_int), ("awgn_n0", C.c_float), ("awgn_seed", C.c_uint32)]


class ChannelBlock(C.Structure):
    """srslte_hip_channel_block_t."""
    C_TYPE = "srslte_hip_channel_block_t"
    _fields_ = [("t", C.c_double), ("delay_samples", C.c_uint32), ("hst_fs_hz", C.c_float), ("rlf_on", C.c_int)]


SIGNATURES = {
    "srslte_hip_channel_create": (None, [P(vp), P(ChannelCfg)]),
    "srslte_hip_channel_destroy": (void, [vp]),
    "srslte_hip_channel_reset": (None, [vp]),
    "srslte_hip_channel_run_batch": (None, [vp, vp, u64, u64, vp, u64, u64, u32, u32, i64, f64, vp]),
    "srslte_hip_channel_fft_size": (None, [vp]),
    "srslte_hip_channel_path_delay": (None, [vp]),
    "srslte_hip_channel_coeffs": (None, [vp, u32, P(f64), P(f64), P(f64)]),
    "srslte_hip_channel_draw_coeffs": (None, [cint, f32, u32, P(f64), P(f64), P(f64)]),
    "srslte_hip_channel_fft_size_for": (None, [cint, f64]),
    "srslte_hip_channel_block_params": (None, [P(ChannelCfg), u32, u32, i64, f64, P(ChannelBlock)]),
}


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


class Channel(Handle):
    """srslte::channel for nof_channels channels and nof_calls blocks per call (srslte_hip_channel_*). cfg: channel_cfg(...)."""
    DESTROY = "srslte_hip_channel_destroy"

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
