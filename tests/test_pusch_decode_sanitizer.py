"""The host function behind srslte_pusch_decode (compat.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer, in a stand-alone program on the
CPU (tests/pusch_decode_asan_driver.cpp): every path of it that ends before a device is needed - NULL arguments and each refusal, those of the
allocation's geometry included (srslte_hip_pusch_rows) - with patterns in cfg, out, the transport block, the soft buffer and both grids that must
survive, and the served-call counter unchanged. compat.cpp and fec_tables.cpp are compiled with the sanitizers; the rest comes from the library as
built. The served path needs a device and takes no sanitizer: tests/test_gpu_pusch_decode.py holds it to the oracle instead."""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "srslte-emane_amd", "csrc")


def test_pusch_decode_host_paths_under_asan_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "drv")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
                               "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(HERE, "pusch_decode_asan_driver.cpp"),
                               os.path.join(CSRC, "compat.cpp"), os.path.join(CSRC, "fec_tables.cpp"), "-L" + CSRC, "-lsrslte_phy_hip", "-L/opt/rocm/lib",
                               "-lamdhip64", "-Wl,-rpath," + CSRC, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
        assert out.returncode == 0, out.stdout + out.stderr
        assert "pusch decode host sanitizer run ok: 62 checks" in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
