"""Records tests/golden/channel.npz from the reference's own channel sources (fading.c, delay.c, hst.c, rlf.c), compiled where they lie into a
temporary directory outside the tree, linked against oracle/_ref/libsrslte_ref.so (srslte_vec_*, srslte_random_*) and against a throwaway
double-precision DFT standing in for the srslte_dft_* calls fading.c makes (FFTW is not available; SURVEY 8(c) used the same device).
ringbuffer.c, timestamp.c and debug.c, whose symbols libsrslte_ref.so does not export, and random.cpp (with the reference's C++ flags, see build_recorder) are
compiled beside them. Nothing of the reference or compiled from it
enters the tree: the fixture holds the recorded outputs, the drawn coefficients, the per-block delays and the Doppler shifts; inputs are
regenerated from a seed (case_input).

    python tests/gen_golden_channel.py [REFERENCE_ROOT]

CASES is also what tests/test_channel_host.py and tests/test_gpu_channel.py run: the same configurations through the restatement and the device."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "channel.npz")

# name -> srate, channels, stages, and the calls [(full_secs, frac_secs, nof_blocks)] of len samples each (state carried from call to call)
CASES = {
    # N = 64; 400 is no multiple of 16: a short last segment in every block, two channels with the seeds of channel.cc's ports 0 and 1
    "fading_epa5_n64": dict(srate=1.92e6, channels=2, len=400, fading="epa5", calls=[(0, 0.0, 2), (0, 2 * 400 / 1.92e6, 1)]),
    # N = 1024, t reaching a thousand seconds, len no multiple of 256
    "fading_etu300_n1024": dict(srate=23.04e6, channels=1, len=1000, fading="etu300", calls=[(1000, 0.5, 3)]),
    # N = 512, blocks shorter than a segment: the overlap accumulates over more than four blocks
    "fading_eva70_n512": dict(srate=23.04e6, channels=1, len=100, fading="eva70", calls=[(2, 0.25, 12)]),
    # 10-100 us with a period of 1 s: 106 samples at t = 0, growing, the maximum of 192, shrinking, the minimum of 19, growing again
    "delay": dict(srate=1.92e6, channels=1, len=240, delay=(10.0, 100.0, 1.0, 0.0),
                  calls=[(0, 0.0, 2), (0, 0.1, 2), (0, 0.25, 2), (0, 0.6, 2), (0, 0.75, 2), (1, 0.05, 2)]),
    # the reference's CTest case `-f 750 -t 7.2`: the shift changes sign at a quarter period, t = 1.8 s
    "hst": dict(srate=1.92e6, channels=1, len=960, hst=(750.0, 7.2, 0.0), calls=[(1, 0.799, 4)]),
    "rlf": dict(srate=1.92e6, channels=1, len=64, rlf=(50, 30), calls=[(0, 0.04995, 3), (0, 0.0799, 2)]),
    "chain": dict(srate=1.92e6, channels=1, len=480, fading="epa5", delay=(10.0, 100.0, 1.0, 0.0), hst=(750.0, 7.2, 0.0), rlf=(50, 30),
                  calls=[(0, 0.0495, 3), (1, 0.7995, 2)]),
    # N = 128 (three radix-4 passes and a closing radix-2 pass), the 50-PRB rate; 700 is no multiple of 32: a short last segment in every block,
    # and the second call starts where the first ends, so the overlap crosses a call boundary
    "fading_eva5_n128": dict(srate=7.68e6, channels=2, len=700, fading="eva5", calls=[(3, 0.5, 3), (3, 0.5 + 3 * 700 / 7.68e6, 2)]),
    # N = 256 (four radix-4 passes) with the nine taps of ETU; blocks shorter than a segment of 64: the overlap accumulates over more than five blocks
    "fading_etu70_n256": dict(srate=7.68e6, channels=2, len=50, fading="etu70", calls=[(1, 0.75, 14)]),
}
# A case's input seed is 1000 + its position here: the first seven in the sorted order they were recorded with, later cases appended (never
# inserted), so that adding a case leaves the recorded inputs and outputs of the others as they are
SEED_ORDER = ("chain", "delay", "fading_epa5_n64", "fading_etu300_n1024", "fading_eva70_n512", "hst", "rlf", "fading_eva5_n128", "fading_etu70_n256")


def case_input(name):
    """[call] -> [channels][blocks][len] complex64, unit power, from the case's own seed."""
    c = CASES[name]
    rng = np.random.default_rng(SEED_ORDER.index(name) + 1000)
    return [((rng.standard_normal((c["channels"], nb, c["len"])) + 1j * rng.standard_normal((c["channels"], nb, c["len"]))) / np.sqrt(2)).astype(np.complex64)
            for (_, _, nb) in c["calls"]]


SHIM = r"""
/* Stand-in for the three srslte_dft_* calls of fading.c: the DFT sum in double precision. Plus accessors for the recorded figures. */
#include <complex.h>
#include <math.h>
#include <stdlib.h>
#include "srslte/phy/dft/dft.h"
#include "srslte/phy/channel/fading.h"
#include "srslte/phy/channel/delay.h"
#include "srslte/phy/channel/hst.h"
int srslte_dft_plan_c(srslte_dft_plan_t* plan, int dft_points, srslte_dft_dir_t dir) { plan->size = dft_points; plan->dir = dir; return 0; }
void srslte_dft_plan_free(srslte_dft_plan_t* plan) { (void)plan; }
void srslte_dft_run_c_zerocopy(srslte_dft_plan_t* plan, const cf_t* in, cf_t* out)
{
  const int    N = plan->size;
  const double s = plan->dir == SRSLTE_DFT_FORWARD ? -1.0 : 1.0;
  double complex* w = malloc(sizeof(double complex) * N);
  double complex* y = malloc(sizeof(double complex) * N);
  for (int k = 0; k < N; k++) w[k] = cexp(s * 2.0 * M_PI * I * k / N);
  for (int k = 0; k < N; k++) {
    double complex acc = 0;
    for (int n = 0; n < N; n++) acc += (double complex)in[n] * w[(int)(((long)k * n) % N)];
    y[k] = acc;
  }
  for (int k = 0; k < N; k++) out[k] = (cf_t)y[k];
  free(w);
  free(y);
}
size_t rec_sizeof(int what) { return what == 0 ? sizeof(srslte_channel_fading_t) : what == 1 ? sizeof(srslte_channel_delay_t) : sizeof(srslte_channel_hst_t); }
unsigned rec_fading_n(srslte_channel_fading_t* q) { return q->N; }
void rec_fading_coeffs(srslte_channel_fading_t* q, double* a, double* w, double* p)
{
  for (int i = 0; i < SRSLTE_CHANNEL_FADING_MAXTAPS; i++) a[i] = q->coeff_a[i], w[i] = q->coeff_w[i], p[i] = q->coeff_p[i];
}
float rec_delay_nsamples(srslte_channel_delay_t* q) { return q->delay_nsamples; }
float rec_hst_fs(srslte_channel_hst_t* q) { return q->fs_hz; }
"""


def build_recorder(ref_root, tmp):
    import subprocess
    root = os.path.dirname(HERE)
    ref_so_dir = os.path.join(root, "oracle", "_ref")
    lib = os.path.join(ref_root, "lib")
    shim = os.path.join(tmp, "shim.c")
    with open(shim, "w") as f:
        f.write(SHIM)
    srcs = [os.path.join(lib, "src/phy/channel", n) for n in ("fading.c", "delay.c", "hst.c", "rlf.c")]
    srcs += [os.path.join(lib, "src/phy/utils/ringbuffer.c"), os.path.join(lib, "src/phy/common/timestamp.c"),
             os.path.join(lib, "src/phy/utils/debug.c"), shim]
    inc = ["complex.h", "math.h", "string.h", "strings.h", "srslte/config.h", "srslte/phy/utils/vector.h", "srslte/phy/utils/ringbuffer.h",
           "srslte/phy/common/timestamp.h", "srslte/phy/common/phy_common.h", "srslte/phy/dft/dft.h"]
    out = os.path.join(tmp, "librec.so")
    cmd = ["gcc", "-std=gnu99", "-D_GNU_SOURCE", "-O3", "-Ofast", "-funroll-loops", "-mfpmath=sse", "-mavx2", "-mfma", "-DLV_HAVE_SSE", "-DLV_HAVE_AVX",
           "-DLV_HAVE_AVX2", "-DLV_HAVE_FMA", "-fPIC", "-w", "-DSRSLTE_SRSLTE_H", "-I" + os.path.join(lib, "include")]
    for h in inc:
        cmd += ["-include", h]
    # random.cpp with the reference's C++ release flags (its CMakeLists gives -Ofast to C only): under the C flags oracle/ref.mk builds it with,
    # -ffinite-math-only removes the isnan loop of srslte_random_uniform_real_dist and the function returns NaN
    rnd = os.path.join(tmp, "random.o")
    subprocess.check_call(["g++", "-std=c++11", "-O3", "-fno-trapping-math", "-fno-math-errno", "-mfpmath=sse", "-mavx2", "-fPIC", "-w",
                           "-I" + os.path.join(lib, "include"), "-c", os.path.join(lib, "src/phy/utils/random.cpp"), "-o", rnd])
    cmd += ["-shared", "-o", out] + srcs + [rnd, "-lstdc++", "-L" + ref_so_dir, "-lsrslte_ref", "-Wl,-rpath," + ref_so_dir, "-lm", "-lpthread"]
    subprocess.check_call(cmd)
    return out


def record(ref_root):
    import ctypes as C
    import tempfile

    class Ts(C.Structure):
        _fields_ = [("full_secs", C.c_long), ("frac_secs", C.c_double)]

    from channel_ref import block_time
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        L = C.CDLL(build_recorder(ref_root, tmp))
        vp, dp = C.c_void_p, C.POINTER(C.c_double)
        L.rec_sizeof.restype = C.c_size_t
        L.srslte_channel_fading_init.argtypes = [vp, C.c_double, C.c_char_p, C.c_uint32]
        L.srslte_channel_fading_execute.restype = C.c_double
        L.srslte_channel_fading_execute.argtypes = [vp, vp, vp, C.c_uint32, C.c_double]
        L.srslte_channel_delay_init.argtypes = [vp, C.c_float, C.c_float, C.c_float, C.c_float, C.c_uint32]
        L.srslte_channel_delay_update_srate.argtypes = [vp, C.c_uint32]
        L.srslte_channel_delay_execute.argtypes = [vp, vp, vp, C.c_uint32, C.POINTER(Ts)]
        L.srslte_channel_hst_init.argtypes = [vp, C.c_float, C.c_float, C.c_float]
        L.srslte_channel_hst_update_srate.argtypes = [vp, C.c_uint32]
        L.srslte_channel_hst_execute.argtypes = [vp, vp, vp, C.c_uint32, C.POINTER(Ts)]
        L.srslte_channel_rlf_init.argtypes = [vp, C.c_uint32, C.c_uint32]
        L.srslte_channel_rlf_execute.argtypes = [vp, vp, vp, C.c_uint32, C.POINTER(Ts)]
        L.rec_fading_coeffs.argtypes = [vp, dp, dp, dp]
        L.rec_fading_n.argtypes = [vp]
        L.rec_delay_nsamples.restype = C.c_float
        L.rec_delay_nsamples.argtypes = [vp]
        L.rec_hst_fs.restype = C.c_float
        L.rec_hst_fs.argtypes = [vp]
        for name, c in sorted(CASES.items()):
            srate, nch, ln = c["srate"], c["channels"], c["len"]
            fading, delay, hst, rlf = [], [], None, None
            coeffs = np.zeros((nch, 3, 9))
            for ch in range(nch):  # channel.cc:45-67 and set_srate, :188-208
                if "fading" in c:
                    q = C.create_string_buffer(L.rec_sizeof(0))
                    assert L.srslte_channel_fading_init(q, srate, c["fading"].encode(), 0x1234 * ch) == 0
                    L.rec_fading_coeffs(q, *(coeffs[ch, i].ctypes.data_as(dp) for i in range(3)))
                    res[name + ".N"] = np.array(L.rec_fading_n(q))
                    fading.append(q)
                if "delay" in c:
                    q = C.create_string_buffer(L.rec_sizeof(1))
                    assert L.srslte_channel_delay_init(q, *c["delay"], int(srate)) == 0
                    L.srslte_channel_delay_update_srate(q, int(srate))
                    delay.append(q)
            if "hst" in c:
                hst = C.create_string_buffer(L.rec_sizeof(2))
                L.srslte_channel_hst_init(hst, *c["hst"])
                L.srslte_channel_hst_update_srate(hst, int(srate))
            if "rlf" in c:
                rlf = C.create_string_buffer(64)
                L.srslte_channel_rlf_init(rlf, *c["rlf"])
            outs, delays, shifts = [], [], []
            for (full, frac, nb), x in zip(c["calls"], case_input(name)):
                y = np.empty_like(x)
                for i in range(nb):
                    fu, fr = block_time(full, frac, i, ln, srate)
                    ts = Ts(fu, fr)
                    for ch in range(nch):  # channel.cc:133-156
                        a, b = x[ch, i].copy(), np.empty(ln, np.complex64)
                        if fading:
                            L.srslte_channel_fading_execute(fading[ch], a.ctypes.data, b.ctypes.data, ln, fu + fr)
                            a[:] = b
                        if delay:
                            L.srslte_channel_delay_execute(delay[ch], a.ctypes.data, b.ctypes.data, ln, C.byref(ts))
                            a[:] = b
                        if hst:
                            L.srslte_channel_hst_execute(hst, a.ctypes.data, b.ctypes.data, ln, C.byref(ts))
                            a[:] = b
                        if rlf:
                            L.srslte_channel_rlf_execute(rlf, a.ctypes.data, b.ctypes.data, ln, C.byref(ts))
                            a[:] = b
                        y[ch, i] = a
                    delays.append(int(L.rec_delay_nsamples(delay[0])) if delay else 0)
                    shifts.append(float(L.rec_hst_fs(hst)) if hst else 0.0)
                outs.append(y.reshape(nch, -1))
            res[name + ".out"] = np.concatenate(outs, axis=1)  # [channels][all blocks of all calls]
            res[name + ".coeffs"] = coeffs
            res[name + ".delays"] = np.array(delays, np.int32)
            res[name + ".shifts"] = np.array(shifts, np.float32)
    return res


if __name__ == "__main__":
    sys.path.insert(0, HERE)
    res = record(sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
    np.savez_compressed(GOLDEN, **res)
    print("wrote %s: %d arrays, %d bytes" % (GOLDEN, len(res), os.path.getsize(GOLDEN)))
