"""numpy model of the two sample conversions an sc16 OFDM object does in its kernels (phy_hip.h, "Sample formats"): what the reference's
srslte_vec_convert_if / srslte_vec_convert_fi compute in their vector bodies (lib/src/phy/utils/vector_simd.c:362-427 in the AVX2 build).
tests/test_iq_format_host.py pins it to the compiled reference; tests/test_gpu_iq_format.py uses it as the expectation."""
import numpy as np


def gain_of(scale):
    """1.0f / scale, as srslte_vec_convert_if_simd computes it once (vector_simd.c:364)."""
    return np.float32(1.0) / np.float32(scale)


def sc16_to_f32(x, scale):
    """srslte_vec_convert_if: (float) x * gain, one fp32 rounding. x: int16 array of any shape -> float32 of the same shape."""
    return np.asarray(x, np.int16).astype(np.float32) * gain_of(scale)


def sc16_to_cf32(x, scale):
    """int16 [...][2] (I, Q) -> complex64 [...]."""
    return np.ascontiguousarray(sc16_to_f32(x, scale)).view(np.complex64)[..., 0]


def f32_to_sc16(v, scale):
    """srslte_vec_convert_fi's vector body (mul_ps, cvttps_epi32, packs_epi32): the product rounded to fp32, truncated towards zero, saturated
    to [-32768, 32767]; a product that is no int32 (NaN, +-inf, magnitude >= 2^31) converts to INT32_MIN and packs to -32768."""
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.asarray(v, np.float32) * np.float32(scale)
        r = np.trunc(s)
        ok = r < np.float32(2147483648.0)  # False for NaN and +inf; every negative value below -32768 saturates to -32768 anyway
        return np.where(ok, np.clip(np.where(ok, r, 0), -32768, 32767), -32768).astype(np.int16)


def cf32_to_sc16(v, scale):
    """complex64 [...] -> int16 [...][2] (I, Q)."""
    v = np.ascontiguousarray(v, np.complex64)
    return f32_to_sc16(v.view(np.float32).reshape(v.shape + (2,)), scale)
