"""Times of the UE CSI feedback measurement for 128 subframes at 100 PRB (2 ports, 2 antennas): srslte_hip_csi_batch alone, the time
srslte_hip_dl_rx_csi_batch adds behind a grants call, and the reference's select_ri_pmi + compute_cn per subframe on the CPU (where
oracle/_ref/libsrslte_ref.so exists; called through ctypes, so an upper bound on its time). Prints one JSON line; these are records, not thresholds.

    python scripts/bench_csi.py [--nsf 128] [--prb 100] [--reps 50]"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _timed(L, fn, reps, stream=None):
    e0, e1 = L.srslte_hip_event_create(), L.srslte_hip_event_create()
    for _ in range(5):
        fn()
    L.srslte_hip_sync()
    ms = []
    for _ in range(reps):
        L.srslte_hip_event_record(e0, stream)
        fn()
        L.srslte_hip_event_record(e1, stream)
        ms.append(L.srslte_hip_event_elapsed_ms(e0, e1))
    L.srslte_hip_event_destroy(e0)
    L.srslte_hip_event_destroy(e1)
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nsf", type=int, default=128)
    ap.add_argument("--prb", type=int, default=100)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    hp = importlib.import_module("srslte-emane_amd")
    L = hp.lib()
    import csi_ref as R
    from _libs import ref
    rng = np.random.default_rng(0)
    nsf, prb, N = a.nsf, a.prb, 14 * 12 * a.prb
    one = R.draw_ce(rng, prb)
    ce = np.ascontiguousarray(np.broadcast_to(one, (nsf, 2, 2, N)) * (1 + 0.01 * rng.standard_normal((nsf, 1, 1, 1))), np.complex64)
    res = np.zeros((nsf, 10), np.float32)
    res[:, 0], res[:, 2] = 0.05, 15.0
    q = hp.Csi(prb)
    dce, dres, dout = hp.DevBuf.from_host(ce), hp.DevBuf.from_host(res), hp.DevBuf(64 * nsf)
    out = dict(nof_sf=nsf, nof_prb=prb)
    out["csi_batch_ms"] = _timed(L, lambda: q.run_device(dce.ptr, dres.ptr, nsf, dout.ptr), a.reps)
    # behind a grants call: the same call with and without the measurement queued after it
    from lte_sim import DlConfig, make_subframe
    tbs = 4008
    cfg = DlConfig(prb, 1, 2, tbs, nof_rx=2, nof_ports=2)
    iq = np.stack([make_subframe(cfg, b % 10, rng, snr_db=12.0, amp=0.2)[0] for b in range(10)])
    iq = np.ascontiguousarray(np.tile(iq, ((nsf + 9) // 10, 1, 1))[:nsf], np.complex64)
    hc = hp.ChestDlCfg()
    hc.filter_coef[0], hc.filter_coef[1] = 4.0, 1.0
    rx = hp.DlRx(1, prb, 1, 0x1234, 2, tbs, 6, nsf, True, hc, nof_rx=2, nof_ports=2)
    grants = (hp.DlGrant * nsf)(*[hp.DlGrant.make(prb, 2, tbs, 0x1234) for _ in range(nsf)])
    din = hp.DevBuf.from_host(iq)

    def grants_call(with_csi):
        assert L.srslte_hip_dl_rx_batch_grants(rx.h, din.ptr, 0, nsf, grants, rx.d_tb.ptr, rx.tb_stride, rx.d_ok.ptr, None) == 0
        if with_csi:
            assert L.srslte_hip_dl_rx_csi_batch(rx.h, nsf, dout.ptr, None) == 0

    t0 = _timed(L, lambda: grants_call(False), max(5, a.reps // 5))
    t1 = _timed(L, lambda: grants_call(True), max(5, a.reps // 5))
    out["grants_ms"], out["grants_with_csi_ms"], out["dl_rx_csi_added_ms"] = t0, t1, t1 - t0
    if ref() is not None:
        r = R.Ref(ref(), ce[0], 0.05, prb)
        for _ in range(50):  # warm-up
            r.pdsch_select_pmi(1), r.pdsch_select_pmi(2), r.cn()
        t = time.perf_counter()
        for _ in range(1000):
            r.pdsch_select_pmi(1), r.pdsch_select_pmi(2), r.cn()
        # three calls through ctypes per iteration: their overhead is in the figure, which is therefore an upper bound on the reference's time
        out["reference_cpu_ms_per_sf_upper_bound"] = (time.perf_counter() - t) / 1000 * 1e3
    print(json.dumps(out))


if __name__ == "__main__":
    main()
