#!/usr/bin/env python3
"""DL control region receive (srslte_hip_dl_ctrl_batch) timed on a batch of 128 subframes of a 100-PRB, 2-port cell with CFI 3: each subframe
carries a C-RNTI DCI for a drawn UE (formats of a drawn TM 1-4) among DCIs for other RNTIs, written by the reference's srslte_pcfich_encode /
srslte_pdcch_encode (oracle/_ref/libsrslte_ref.so) and received with a drawn channel at 20 dB. For context the reference's CPU control search
of the same subframes is timed per subframe: srslte_pcfich_decode + srslte_pdcch_extract_llr + the DL DCI blind search over
srslte_pdcch_decode_msg, driven from Python through ctypes: the figure includes the interpreter's share (the *_incl_python fields) and is an
upper bound of the reference's own cost. Prints one JSON line.

  python scripts/bench_ctrl.py [--steps K] [--warmup W] [--nof-sf N]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "tests")):
    if d not in sys.path:
        sys.path.insert(0, d)

import dl_ctrl_ref as T  # noqa: E402  the reference-side encoder and search of the tests (tests/dl_ctrl_ref.py)

pkg = importlib.import_module("srslte-emane_amd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--nof-sf", type=int, default=128)
    ap.add_argument("--ref-sf", type=int, default=128, help="subframes the reference's CPU search is timed on")
    a = ap.parse_args()
    nof_prb, ports, cell_id, cfi, n = 100, 2, 1, 3, a.nof_sf
    cell = T.Cell(nof_prb, ports, cell_id, False, 1, False, 1)
    rng = np.random.default_rng(0)
    reqs, ys, ces, subs = [], [], [], []
    for b in range(n):
        rnti, tm = int(rng.integers(0x0B, 0xFFF3)), int(rng.integers(0, 4))
        dcis, _ = T.draw_subframe(cell, b, cfi, rnti, tm, rng, "ue")
        y, ce, noise = T.channel(cell, cell.encode(b, cfi, dcis), 20.0, rng)
        reqs.append(pkg.DlCtrlReq(rnti, tm, 0, 0))
        ys.append(np.stack(y))
        ces.append(ce)
        subs.append((b, rnti, tm, y, ce, noise))
    res = np.zeros((n, 10), np.float32)
    res[:, 0] = [s[5] for s in subs]
    ctrl = pkg.DlCtrl(nof_prb, ports, cell_id, phich_resources=1, max_batch=n)
    dg, dce, dres = pkg.DevBuf.from_host(np.stack(ys)), pkg.DevBuf.from_host(np.stack(ces)), pkg.DevBuf.from_host(res)
    dout, dmsg = pkg.DevBuf(C.sizeof(pkg.DlCtrlRes) * n), pkg.DevBuf(C.sizeof(pkg.DciMsg) * n)
    L = pkg.lib()
    st = L.srslte_hip_stream_create()
    for _ in range(a.warmup):
        assert ctrl.run_device(dg.ptr, dce.ptr, dres.ptr, 0, reqs, dout.ptr, dmsg.ptr, st) == 0
    L.srslte_hip_stream_sync(st)
    e0, e1 = L.srslte_hip_event_create(), L.srslte_hip_event_create()
    t0 = time.perf_counter()
    L.srslte_hip_event_record(e0, st)
    for _ in range(a.steps):
        ctrl.run_device(dg.ptr, dce.ptr, dres.ptr, 0, reqs, dout.ptr, dmsg.ptr, st)
    L.srslte_hip_event_record(e1, st)
    L.srslte_hip_stream_sync(st)
    wall = time.perf_counter() - t0
    dev_ms = L.srslte_hip_event_elapsed_ms(e0, e1) / a.steps
    out = (pkg.DlCtrlRes * n)()
    L.srslte_hip_memcpy_d2h(C.addressof(out), dout.ptr, C.sizeof(out))
    found = sum(r.nof_dci for r in out)
    # the reference on the CPU, one subframe after the other
    m = min(a.ref_sf, n)
    t0 = time.perf_counter()
    ref_found = 0
    for b, rnti, tm, y, ce, noise in subs[:m]:
        c, _ = cell.pcfich(b, y, ce, noise)
        cell.extract(b, c, y, ce, noise)
        ref_found += T.blind_search(cell, b, c, rnti, tm) is not None
    ref_s = time.perf_counter() - t0
    print(json.dumps({"metric": "dl_ctrl_subframes_per_s", "nof_prb": nof_prb, "nof_ports": ports, "cfi": cfi, "batch": n, "steps": a.steps,
                      "device_ms_per_batch": round(dev_ms, 4), "device_subframes_per_s": round(n / (dev_ms / 1e3), 1),
                      "host_wall_ms_per_batch": round(1e3 * wall / a.steps, 4), "dci_found": int(found), "dci_expected": n,
                      "ref_cpu_us_per_subframe_incl_python": round(1e6 * ref_s / m, 2), "ref_cpu_subframes_per_s_incl_python": round(m / ref_s, 1),
                      "ref_found": int(ref_found), "ref_subframes": m}))
    L.srslte_hip_event_destroy(e0)
    L.srslte_hip_event_destroy(e1)
    L.srslte_hip_stream_destroy(st)
    ctrl.free()


if __name__ == "__main__":
    main()
