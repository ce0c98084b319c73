#!/usr/bin/env python3
"""What the synchronisation costs: one 64-item cell-search call (fft_size 128, 9600 positions, three hypotheses per item, the ue_sync find
setting) and one 64-item tracking call at fft_size 2048 (32 positions, one hypothesis) of srslte_hip_sync_find_batch on resident samples, and
srslte_hip_cfo_correct_batch of 64 x 9600 samples; ms per call, best of 5 rounds of `steps` calls timed with events on one stream. With a
second argument "big" also the unmeasured shape of the issue: 8 items at fft_size 2048 over a 5-subframe max_offset (153 600 positions).
Beside them, where oracle/_ref/hip was built, the seconds one srslte_sync_find of the reference's sync.c takes when linked against this library
(tests/sync_dropin_driver.c, `time` mode), else "not measured". One JSON line."""
import importlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _driver_seconds(fft_size, frame_size, max_offset, reps):
    lib_a = os.path.join(ROOT, "oracle", "_ref", "hip", "libsrslte_upper.a")
    if not os.path.exists(lib_a):
        return "not measured"
    csrc = os.path.join(ROOT, "srslte-emane_amd", "csrc")
    exe = os.path.join(tempfile.mkdtemp(), "sync_dropin_driver")
    subprocess.check_call(["gcc", "-std=c99", "-O2", os.path.join(ROOT, "tests", "sync_dropin_driver.c"), "-o", exe, lib_a, "-L" + csrc,
                           "-lsrslte_phy_hip", "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib", "-lstdc++", "-lm", "-lpthread"])
    out = subprocess.check_output([exe, "time", str(fft_size), str(frame_size), str(max_offset), str(reps)], timeout=300)
    return float(out.decode().split()[-1])


def main():
    hp = importlib.import_module("srslte-emane_amd")
    L = hp.lib()
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    big = len(sys.argv) > 2 and sys.argv[2] == "big"
    st = L.srslte_hip_stream_create()
    ev0, ev1 = L.srslte_hip_event_create(), L.srslte_hip_event_create()
    rng = np.random.default_rng(1)
    find = dict(detect_cp=True, cfo_cp_enable=True, cfo_pss_enable=True, pss_filt_enable=True, sss_alg=hp.SSS_PARTIAL_3, threshold=2.0, cfo_cp_nsymbols=14,
                ema_alpha=1.0)
    res = {"metric": "sync_ms_per_call", "steps": steps}

    def timed(fn):
        best = 1e30
        for _ in range(5):
            assert fn() == 0
            L.srslte_hip_stream_sync(st)
            L.srslte_hip_event_record(ev0, st)
            for _ in range(steps):
                assert fn() == 0
            L.srslte_hip_event_record(ev1, st)
            L.srslte_hip_stream_sync(st)
            best = min(best, L.srslte_hip_event_elapsed_ms(ev0, ev1) / steps)
        return best

    shapes = [("search_128_9600_x3", 128, 9728, 9600, 64, 3, 0), ("track_2048_32", 2048, 32768, 32, 64, 0, 15000)]
    if big:
        shapes.append(("search_2048_153600", 2048, 153600 + 2048, 153600, 8, 0, 0))
    for name, N, frame, mo, n, v, fo in shapes:
        x = ((rng.normal(size=(n, frame)) + 1j * rng.normal(size=(n, frame))) / np.sqrt(2)).astype(np.complex64)
        q = hp.Sync(N, frame, mo, max_items=n, **find)
        d_in = hp.DevBuf.from_host(x)
        items = [hp.SyncItem.make(v, fo)] * n
        d_res = hp.DevBuf(64 * hp.sync_rows(items))
        res[name + "_ms"] = timed(lambda: q.find_device(d_in.ptr, frame, items, d_res.ptr, st))
        res[name + "_items"] = n
        q.free()
    x = ((rng.normal(size=(64, 9600)) + 1j * rng.normal(size=(64, 9600))) / np.sqrt(2)).astype(np.complex64)
    d = hp.DevBuf.from_host(x)
    f = rng.uniform(-3e-3, 3e-3, 64).astype(np.float32)
    res["cfo_correct_64x9600_ms"] = timed(lambda: hp.cfo_correct_device(d.ptr, d.ptr, 9600, 9600, 64, f, st))
    res["reference_sync_find_128_9600_s"] = _driver_seconds(128, 9728, 9600, 20)
    res["reference_sync_find_2048_32_s"] = _driver_seconds(2048, 32768, 32, 20)
    L.srslte_hip_event_destroy(ev0)
    L.srslte_hip_event_destroy(ev1)
    L.srslte_hip_stream_destroy(st)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
