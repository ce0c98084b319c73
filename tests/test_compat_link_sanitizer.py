"""The single-call API's host link (csrc/compat_link.hpp: the per-thread stream and pinned arena, the per-call scope, zero-copy
reservations, the grow-only device stage) under AddressSanitizer + UndefinedBehaviorSanitizer, in a stand-alone program on the CPU
(tests/link_asan_driver.cpp). The driver links no HIP library: it defines the runtime calls the header reaches over malloc / free, so a write
into an arena that hipHostFree released, or into a caller buffer that a failed call left queued, is a heap- or stack-use-after-free to ASan.
The paths that need a device are held to the oracle in tests/test_gpu_compat_lifecycle.py."""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "srslte-emane_amd", "csrc")


def test_compat_link_under_asan_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "drv")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
                               "-I/opt/rocm/include", "-I" + CSRC, os.path.join(HERE, "link_asan_driver.cpp"), "-pthread", "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
        assert out.returncode == 0, out.stdout + out.stderr
        assert "compat link sanitizer run ok: 32 checks, balanced at exit" in out.stdout
        assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
