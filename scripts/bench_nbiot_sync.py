#!/usr/bin/env python3
"""What the batched NB-IoT synchronisation costs: srslte_hip_nbiot_npss_find_batch at frame_size 19200 with 64 resident items (one track
each, npss_ema_alpha 0.2, the CFO stage on), and srslte_hip_nbiot_nsss_find_batch with 64 resident items, all with an unknown cell id (504
hypotheses each) and all with a known one. The three calls alternate round by round, so drift of the clocks falls on all; ms per call is the
median over `rounds` rounds of a window of calls timed with events on one stream - 50 x `steps` NPSS calls, 20 x `steps` known-id and 10 x
`steps` exhaustive NSSS calls, a tenth to a quarter of a second each at the default - with the spread (min, max) beside it. The input is noise.
`nsss_unknown_call_tflops` is the product kernel's arithmetic over the WHOLE call's time (three kernels), not a kernel's share of peak.
With --driver (and oracle/_ref/hip/libsrslte_upper.a built) the line also carries the seconds ONE call of the reference's own
srslte_sync_nbiot_find / srslte_nsss_sync_find takes through tests/nbiot_sync_dropin_driver.c: the reference's code over this library's
single-call srslte_dft_* (one device round trip per transform), not a CPU baseline. One JSON line.
    python scripts/bench_nbiot_sync.py [steps] [rounds] [--driver]"""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    hp = importlib.import_module("srslte-emane_amd")
    L = hp.lib()
    steps = int(args[0]) if len(args) > 0 else 10
    rounds = int(args[1]) if len(args) > 1 else 9
    st = L.srslte_hip_stream_create()
    ev0, ev1 = L.srslte_hip_event_create(), L.srslte_hip_event_create()
    rng = np.random.default_rng(1)
    n, fs = 64, 19200
    res = {"metric": "nbiot_sync_ms_per_call", "steps": steps, "rounds": rounds, "items": n, "npss_frame_size": fs}

    def once(fn, k):
        assert fn() == 0  # warm-up
        L.srslte_hip_stream_sync(st)
        L.srslte_hip_event_record(ev0, st)
        for _ in range(k):
            assert fn() == 0
        L.srslte_hip_event_record(ev1, st)
        L.srslte_hip_stream_sync(st)
        return L.srslte_hip_event_elapsed_ms(ev0, ev1) / k

    x = ((rng.normal(size=(n, fs)) + 1j * rng.normal(size=(n, fs))) / np.sqrt(2)).astype(np.complex64)
    d_in = hp.DevBuf.from_host(x)
    d_res = hp.DevBuf(32 * n)
    q = hp.NbiotSync(fs, max_items=n, n_tracks=n)
    items = [hp.NbiotNpssItem(b, 0) for b in range(n)]
    calls = {"npss": lambda: q.npss_device(d_in.ptr, fs, items, d_res.ptr, st),
             "nsss_unknown": lambda: q.nsss_device(d_in.ptr, fs, [-1] * n, d_res.ptr, st),
             "nsss_known": lambda: q.nsss_device(d_in.ptr, fs, [(7 * b) % 504 for b in range(n)], d_res.ptr, st)}
    mult = {"npss": 50, "nsss_unknown": 10, "nsss_known": 20}
    res["calls_per_window"] = {k: m * steps for k, m in mult.items()}
    times = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            times[k].append(once(fn, mult[k] * steps))
    for k, v in times.items():
        res["%s_ms" % k] = [float(np.median(v)), float(min(v)), float(max(v))]
    # the product kernel's arithmetic: 504 ids x 132 rows x 5376 lags (84 tiles of 64) complex FMAs of 8 flops
    res["nsss_unknown_call_tflops"] = n * 504 * 132 * 84 * 64 * 8 / (np.median(times["nsss_unknown"]) * 1e-3) / 1e12
    q.free()
    if "--driver" in sys.argv:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from test_gpu_nbiot_sync import build_driver
        drv = build_driver()
        if drv is not None:
            res["reference_over_dft_s_per_item"] = {"npss_19200": float(drv.run("time_npss", fs, 5)), "nsss_unknown": float(drv.run("time_nsss", -1, 1)),
                                                    "nsss_known": float(drv.run("time_nsss", 7, 20))}
    L.srslte_hip_event_destroy(ev0)
    L.srslte_hip_event_destroy(ev1)
    L.srslte_hip_stream_destroy(st)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
