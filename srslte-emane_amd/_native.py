"""The native library and what every module of the mirror shares: the binding table's loader, device buffers and the small helpers.

Each module of the package declares the C functions of its sections of ``include/srslte_hip/phy_hip.h`` in a dict ``SIGNATURES``:
``name: (restype, [argtypes])`` with ``None`` for the ``int`` status code and ``void`` for no return value. ``lib()`` binds all of them once;
nothing else in the package assigns a function's types. Every ``ctypes.Structure`` names its C typedef in ``C_TYPE``.
``tests/test_host_mirror_abi.py`` compares both with the header.
"""
import ctypes as C
import importlib
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libsrslte_phy_hip.so")

SRSLTE_SUCCESS, SRSLTE_ERROR, SRSLTE_ERROR_INVALID_INPUTS = 0, -1, -2
MOD_BPSK, MOD_QPSK, MOD_16QAM, MOD_64QAM, MOD_256QAM = range(5)
CRC24A, CRC24B = 0x1864CFB, 0x1800063
IQ_CF32, IQ_SC16 = 0, 1  # SRSLTE_HIP_IQ_*: the sample format of an object's time-domain side (phy_hip.h, "Sample formats")

# the spellings the SIGNATURES rows use
vp, cint, sz, P = C.c_void_p, C.c_int, C.c_size_t, C.POINTER
u8, u16, u32, u64, i32, i64, f32, f64 = C.c_uint8, C.c_uint16, C.c_uint32, C.c_uint64, C.c_int32, C.c_int64, C.c_float, C.c_double


class void:
    """restype of a C function that returns nothing."""


MODULES = ("_native", "core", "dl_ctrl", "ul_ctrl", "csi", "pipelines", "uci_plan", "channel", "ue_sync")

# device plumbing
SIGNATURES = {
    "srslte_hip_device_count": (None, []),
    "srslte_hip_set_device": (None, [cint]),
    "srslte_hip_malloc": (vp, [sz]),
    "srslte_hip_free": (void, [vp]),
    "srslte_hip_memcpy_h2d": (None, [vp, vp, sz]),
    "srslte_hip_memcpy_d2h": (None, [vp, vp, sz]),
    "srslte_hip_memset": (None, [vp, cint, sz]),
    "srslte_hip_sync": (None, []),
    "srslte_hip_stream_create": (vp, []),
    "srslte_hip_stream_destroy": (void, [vp]),
    "srslte_hip_stream_sync": (None, [vp]),
    "srslte_hip_event_create": (vp, []),
    "srslte_hip_event_record": (None, [vp, vp]),
    "srslte_hip_event_elapsed_ms": (f32, [vp, vp]),
    "srslte_hip_event_destroy": (void, [vp]),
    "srslte_hip_compat_thread_stream": (vp, [vp]),
    "srslte_hip_compat_stats": (void, [vp]),
}

_lib = None


def signatures():
    """Every module's rows in one dict."""
    out = {}
    for m in MODULES:
        out.update(importlib.import_module("." + m, __package__).SIGNATURES)
    return out


def lib():
    """The native library with every row of the binding table applied; raises if it was not built (no fallback path exists) or if it
    does not export a declared function."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in signatures().items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = {None: C.c_int, void: None}.get(res, res), args
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
        return host_copy(self.ptr, dtype, self.nbytes // np.dtype(dtype).itemsize if count is None else int(count))

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


# ---------------------------------------------------------------- shared by the modules
class Handle:
    """A native object: its handle self.h, made by _create and given back by free() through the C function DESTROY names."""

    DESTROY = None

    def _create(self, name, *args):
        self.h = getattr(lib(), name)(*args)
        if not self.h:
            raise RuntimeError(name + " failed")

    def free(self):
        if self.h:
            getattr(lib(), self.DESTROY)(self.h)
            self.h = None


def host_copy(ptr, dtype, count):
    """count elements of dtype from the device pointer ptr."""
    out = np.empty(count, dtype)
    _check(lib().srslte_hip_memcpy_d2h(out.ctypes.data, ptr, out.nbytes), "memcpy_d2h")
    return out


def read_structs(ptr, cls, n):
    """n structs cls from the device pointer ptr -> list (host copies)."""
    out = (cls * max(1, n))()
    if n:
        _check(lib().srslte_hip_memcpy_d2h(C.addressof(out), ptr, C.sizeof(cls) * n), "memcpy_d2h")
    return list(out)[:n]


def result_structs(rc, ptr, cls, n):
    """What a batch call returns: (rc, None) where it refused, else (rc, [cls] * n) once the device is done."""
    if rc != SRSLTE_SUCCESS:
        return rc, None
    sync()
    return rc, read_structs(ptr, cls, n)


def upload_rows(x):
    """x [n][stride] (or one row) complex -> (the contiguous complex64 [n][stride], its device copy)."""
    a = np.ascontiguousarray(x, np.complex64)
    a = a.reshape(1, -1) if a.ndim == 1 else a
    return a, DevBuf.from_host(a)


def struct_array(cls, items):
    """A ctypes array of the items (one dummy entry when empty: the C side is never handed a zero-length array)."""
    return (cls * max(1, len(items)))(*items)
