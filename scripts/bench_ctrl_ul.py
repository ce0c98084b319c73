#!/usr/bin/env python3
"""UL DCIs and the PHICH in the batched DL control receive, timed on scripts/bench_ctrl.py's cell: 128 subframes of a 100-PRB, 2-port cell
with CFI 3 at 20 dB, each with one DL DCI and one format-0 DCI for the subframe's UE among DCIs for other RNTIs and 16 PHICHs (written by the
reference's encoders, oracle/_ref/libsrslte_ref.so). With events on one stream after a warm-up it times (a) srslte_hip_dl_ctrl_batch,
(b) srslte_hip_dl_ctrl_batch_ul on the same buffers with the 16 x 128 PHICH requests, (c) srslte_hip_dl_ctrl_phich_batch alone, each
--repeats times in rotation, and prints one JSON line (medians, and the spread of the repeats).

  python scripts/bench_ctrl_ul.py [--steps K] [--warmup W] [--nof-sf N] [--repeats R]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "tests")):
    if d not in sys.path:
        sys.path.insert(0, d)

import dl_ctrl_ref as T  # noqa: E402
import dl_ctrl_ul_ref as U  # noqa: E402

pkg = importlib.import_module("srslte-emane_amd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--nof-sf", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--phich-per-sf", type=int, default=16)
    a = ap.parse_args()
    nof_prb, ports, cell_id, cfi, n = 100, 2, 1, 3, a.nof_sf
    cell = U.UlCell(nof_prb, ports, cell_id, False, 1, False, 1)
    rng = np.random.default_rng(0)
    reqs, ys, ces, noises, ph, sent = [], [], [], [], [], []
    n0, ncce = pkg.dci_format_sizeof(nof_prb, ports, T.F0), cell.ncce[cfi - 1]
    for b in range(n):
        rnti, tm = int(rng.integers(0x0B, 0xFFF3)), int(rng.integers(0, 4))
        dcis, _ = T.draw_subframe(cell, b, cfi, rnti, tm, rng, "ue")
        used = np.zeros(ncce, bool)
        for m in dcis:
            used[m.ncce:m.ncce + (1 << m.L)] = True
        for L, c0 in pkg.pdcch_ue_locations(ncce, b % 10, rnti):
            if not used[c0:c0 + (1 << L)].any():
                dcis.append(T.make_msg(rnti, L, c0, T.F0, n0, rng))
                break
        phichs = []
        while len(phichs) < a.phich_per_sf:
            p = (int(rng.integers(0, nof_prb)), int(rng.integers(0, 8)), 0, int(rng.integers(0, 2)))
            if cell.calc(*p[:3]) not in [cell.calc(*q[:3]) for q in phichs]:
                phichs.append(p)
        y, ce, noise = T.channel(cell, cell.encode_full(b, cfi, dcis, phichs), 20.0, rng)
        reqs.append(pkg.DlCtrlReq(rnti, tm, 0, 0))
        ys.append(np.stack(y))
        ces.append(ce)
        noises.append(noise)
        ph += [(b,) + p[:3] for p in phichs]
        sent += [p[3] for p in phichs]
    res = np.zeros((n, 10), np.float32)
    res[:, 0] = noises
    m = len(ph)
    ctrl = pkg.DlCtrl(nof_prb, ports, cell_id, phich_resources=1, max_batch=n, max_phich=m)
    dg, dce, dres = pkg.DevBuf.from_host(np.stack(ys)), pkg.DevBuf.from_host(np.stack(ces)), pkg.DevBuf.from_host(res)
    dout, dmsg = pkg.DevBuf(C.sizeof(pkg.DlCtrlRes) * n), pkg.DevBuf(C.sizeof(pkg.DciMsg) * n)
    dul, dulm = pkg.DevBuf(C.sizeof(pkg.DlCtrlUlRes) * n), pkg.DevBuf(C.sizeof(pkg.DciMsg) * n * pkg.DL_CTRL_MAX_UL_DCI)
    dph = pkg.DevBuf(C.sizeof(pkg.PhichRes) * m)
    L = pkg.lib()
    st = L.srslte_hip_stream_create()
    # the request arrays are built once: the timed loops hold the C calls alone, not the conversion of 2048 Python tuples per call
    rq, pq = (pkg.DlCtrlReq * n)(*reqs), (pkg.PhichReq * m)(*[pkg.PhichReq(*p) for p in ph])
    calls = {
        "dl_ctrl_batch": lambda: L.srslte_hip_dl_ctrl_batch(ctrl.h, dg.ptr, dce.ptr, dres.ptr, 0, n, rq, dout.ptr, dmsg.ptr, st),
        "dl_ctrl_batch_ul": lambda: L.srslte_hip_dl_ctrl_batch_ul(ctrl.h, dg.ptr, dce.ptr, dres.ptr, 0, n, rq, dout.ptr, dmsg.ptr, dul.ptr, dulm.ptr, pq, m,
                                                                  dph.ptr, st),
        "phich_batch": lambda: L.srslte_hip_dl_ctrl_phich_batch(ctrl.h, dg.ptr, dce.ptr, dres.ptr, 0, n, pq, m, dph.ptr, st),
    }
    e0, e1 = L.srslte_hip_event_create(), L.srslte_hip_event_create()
    ms = {k: [] for k in calls}
    for _ in range(a.repeats):
        for k, f in calls.items():
            for _ in range(a.warmup):
                assert f() == 0
            L.srslte_hip_stream_sync(st)
            L.srslte_hip_event_record(e0, st)
            for _ in range(a.steps):
                f()
            L.srslte_hip_event_record(e1, st)
            L.srslte_hip_stream_sync(st)
            ms[k].append(L.srslte_hip_event_elapsed_ms(e0, e1) / a.steps)
    assert calls["dl_ctrl_batch_ul"]() == 0
    L.srslte_hip_stream_sync(st)
    out, ul, phr = (pkg.DlCtrlRes * n)(), (pkg.DlCtrlUlRes * n)(), (pkg.PhichRes * m)()
    for dst, src in ((out, dout), (ul, dul), (phr, dph)):
        L.srslte_hip_memcpy_d2h(C.addressof(dst), src.ptr, C.sizeof(dst))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    print(json.dumps({"metric": "dl_ctrl_ul_ms_per_batch", "nof_prb": nof_prb, "nof_ports": ports, "cfi": cfi, "batch": n, "nof_phich": m,
                      "steps": a.steps, "repeats": a.repeats,
                      "a_dl_ctrl_batch_ms": round(med["dl_ctrl_batch"], 4), "b_dl_ctrl_batch_ul_ms": round(med["dl_ctrl_batch_ul"], 4),
                      "c_phich_batch_ms": round(med["phich_batch"], 4), "b_minus_a_ms": round(med["dl_ctrl_batch_ul"] - med["dl_ctrl_batch"], 4),
                      "runs_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                      "dl_dci_found": int(sum(r.nof_dci for r in out)), "ul_dci_found": int(sum(r.nof_ul_dci for r in ul)), "subframes": n,
                      "phich_acks_as_sent": int(sum(int(r.ack_value) == s for r, s in zip(phr, sent))), "phich_requests": m}))
    L.srslte_hip_event_destroy(e0)
    L.srslte_hip_event_destroy(e1)
    L.srslte_hip_stream_destroy(st)
    ctrl.free()


if __name__ == "__main__":
    main()
