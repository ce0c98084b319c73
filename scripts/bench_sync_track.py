#!/usr/bin/env python3
"""What a tracked synchronisation call costs beside the stateless one: srslte_hip_sync_track_batch against srslte_hip_sync_find_batch on the
same 64 resident items, one hypothesis each, in the same run - fft_size 128 with max_offset 9600 and fft_size 2048 with max_offset 30720,
the ue_sync find setting, with ema_alpha 1 (no average kept) and 0.3 (the track's average row read and written, 2 nout 4 bytes per row) and
frame modes 0 (FDD) and 2 (detect: one more SSS stage per row). The two calls alternate round by round, so drift of the clocks falls on both;
ms per call is the median over `rounds` rounds of `steps` calls timed with events on one stream, with the spread (min, max) beside it, and the
ratio is that of the medians. The input is noise with the threshold at 0, so every row runs every stage. One JSON line.
    python scripts/bench_sync_track.py [steps] [rounds]"""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    hp = importlib.import_module("srslte-emane_amd")
    L = hp.lib()
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    st = L.srslte_hip_stream_create()
    ev0, ev1 = L.srslte_hip_event_create(), L.srslte_hip_event_create()
    rng = np.random.default_rng(1)
    res = {"metric": "sync_track_ms_per_call", "steps": steps, "rounds": rounds, "items": 64}

    def once(fn):
        assert fn() == 0  # warm-up
        L.srslte_hip_stream_sync(st)
        L.srslte_hip_event_record(ev0, st)
        for _ in range(steps):
            assert fn() == 0
        L.srslte_hip_event_record(ev1, st)
        L.srslte_hip_stream_sync(st)
        return L.srslte_hip_event_elapsed_ms(ev0, ev1) / steps

    n = 64
    for N, mo in ((128, 9600), (2048, 30720)):
        frame = mo + N
        x = ((rng.normal(size=(n, frame)) + 1j * rng.normal(size=(n, frame))) / np.sqrt(2)).astype(np.complex64)
        d_in = hp.DevBuf.from_host(x)
        d_res = hp.DevBuf(96 * n)
        for alpha in (1.0, 0.3):
            q = hp.Sync(N, frame, mo, max_items=n, detect_cp=True, cfo_cp_enable=True, cfo_pss_enable=True, pss_filt_enable=True,
                        sss_alg=hp.SSS_PARTIAL_3, threshold=0.0, cfo_cp_nsymbols=14, ema_alpha=alpha)
            items = [hp.SyncItem.make(b % 3) for b in range(n)]
            calls = {"stateless": lambda: q.find_device(d_in.ptr, frame, items, d_res.ptr, st)}
            tracks = {}
            for mode in (0, 2):
                tracks[mode] = hp.SyncTracks(q, n, 0.0, mode)
                titems = [hp.SyncTrackItem.make(b, b % 3) for b in range(n)]
                calls["mode%d" % mode] = (lambda k, ti: lambda: k.track_device(d_in.ptr, frame, ti, d_res.ptr, st))(tracks[mode], titems)
            times = {k: [] for k in calls}
            for _ in range(rounds):
                for k, fn in calls.items():
                    times[k].append(once(fn))
            key = "N%d_mo%d_alpha%.1f" % (N, mo, alpha)
            for k, v in times.items():
                res["%s_%s_ms" % (key, k)] = [float(np.median(v)), float(min(v)), float(max(v))]
            for mode in (0, 2):
                res["%s_mode%d_over_stateless" % (key, mode)] = float(np.median(times["mode%d" % mode]) / np.median(times["stateless"]))
            for k in tracks.values():
                k.free()
            q.free()
    L.srslte_hip_event_destroy(ev0)
    L.srslte_hip_event_destroy(ev1)
    L.srslte_hip_stream_destroy(st)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
