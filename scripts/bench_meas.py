#!/usr/bin/env python3
"""What the neighbour-cell measurement costs: srslte_hip_meas_run_batch of 8 captures x 8 candidate cells x 5 subframes on resident samples at
6, 25 and 100 PRB, and srslte_hip_meas_set_cells of the 8 cells; ms per call and us per row, the median of 7 rounds of `steps` calls timed
with events on one stream after 3 warm-up rounds (the spread of the rounds beside it). Beside them, where oracle/_ref/hip was built, the
seconds one set_cell and one run of the reference's refsignal_dl_sync.c take for ONE row of the same shape when linked against this library
(tests/meas_dropin_driver.c, `time` mode; 6 and 25 PRB only: its 2 sf_len-point transforms are O(N^2)), else "not measured". Writes
profiles/meas/bench_meas.json and prints the same JSON line."""
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


def _driver_seconds(nof_prb, nof_sf, reps):
    lib_a = os.path.join(ROOT, "oracle", "_ref", "hip", "libsrslte_upper.a")
    if not os.path.exists(lib_a):
        return "not measured", "not measured"
    csrc = os.path.join(ROOT, "srslte-emane_amd", "csrc")
    exe = os.path.join(tempfile.mkdtemp(), "meas_dropin_driver")
    subprocess.check_call(["gcc", "-std=c99", "-O2", os.path.join(ROOT, "tests", "meas_dropin_driver.c"), "-o", exe, lib_a, "-L" + csrc,
                           "-lsrslte_phy_hip", "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib", "-lstdc++", "-lm", "-lpthread"])
    out = subprocess.check_output([exe, "time", str(nof_prb), str(nof_sf), str(reps)], timeout=300).decode().split()
    return float(out[-2]), float(out[-1])


def main():
    import meas_ref as mr
    hp = importlib.import_module("srslte-emane_amd")
    L = hp.lib()
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    st = L.srslte_hip_stream_create()
    ev0, ev1 = L.srslte_hip_event_create(), L.srslte_hip_event_create()
    rng = np.random.default_rng(1)
    caps, cells, nof_sf = 8, 8, 5
    res = {"metric": "meas_ms_per_call", "steps": steps, "captures": caps, "cells": cells, "nof_sf": nof_sf, "rows": caps * cells}

    def timed(fn):
        t = []
        for r in range(10):
            assert fn() == 0
            L.srslte_hip_stream_sync(st)
            L.srslte_hip_event_record(ev0, st)
            for _ in range(steps):
                assert fn() == 0
            L.srslte_hip_event_record(ev1, st)
            L.srslte_hip_stream_sync(st)
            if r >= 3:
                t.append(L.srslte_hip_event_elapsed_ms(ev0, ev1) / steps)
        return float(np.median(t)), float(min(t)), float(max(t))

    ids = [150, 29, 153, 151, 350, 129, 77, 301]
    for nof_prb in (6, 25, 100):
        N = mr.symbol_sz(nof_prb)
        plan = [dict(id=150, start_sf=8, delay=1234, amp=1.0, cfo_hz=200.0), dict(id=29, start_sf=9, delay=99, amp=0.7, cfo_hz=-300.0)]
        one = mr.capture(plan, nof_prb, N, nof_sf, rng).astype(np.complex64)
        x = np.stack([np.roll(one, 17 * c) for c in range(caps)])  # eight different captures of the same two cells
        q = hp.Meas(nof_prb, caps, cells, nof_sf)
        assert q.set_cells(ids, st) == 0
        d_in, d_res = hp.DevBuf.from_host(x), hp.DevBuf(64 * caps * cells)
        name = "%dprb" % nof_prb
        med, lo, hi = timed(lambda: q.run_device(d_in.ptr, x.shape[1], nof_sf, caps, d_res.ptr, st))
        res[name + "_run_ms"], res[name + "_run_ms_min_max"], res[name + "_run_us_per_row"] = med, [lo, hi], 1e3 * med / (caps * cells)
        rows = q.read(d_res, caps * cells)
        res[name + "_found"] = int(sum(r.found for r in rows))  # 2 per capture: the timed call did the whole job
        med, lo, hi = timed(lambda: q.set_cells(ids, st))
        res[name + "_set_cells_ms"], res[name + "_set_cells_ms_min_max"] = med, [lo, hi]
        q.free()
    for nof_prb in (6, 25):
        s, r = _driver_seconds(nof_prb, nof_sf, 5)
        res["reference_%dprb_set_cell_s_per_row" % nof_prb], res["reference_%dprb_run_s_per_row" % nof_prb] = s, r
    L.srslte_hip_event_destroy(ev0)
    L.srslte_hip_event_destroy(ev1)
    L.srslte_hip_stream_destroy(st)
    os.makedirs(os.path.join(ROOT, "profiles", "meas"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "meas", "bench_meas.json"), "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
