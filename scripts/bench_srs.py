#!/usr/bin/env python3
"""What the SRS costs: a 100-PRB cell, bw_cfg 0 (96 PRB sounded, M_sc 576, J 72), 128 subframes with 8 UEs each - the eight cyclic shifts of one
comb - per call. srslte_hip_srs_tx_put of the 1024 entries on a resident grid and srslte_hip_srs_rx_batch of the same list on the grid the
put left (ms per call, entries/s); best of 5 rounds of `steps` calls timed with events on one stream. There is no reference receiver and no
earlier implementation to compare with: the figures are recorded, not gated. One JSON line."""
import ctypes as C
import importlib
import json
import os
import sys


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    hp = importlib.import_module("srslte-emane_amd")
    L = hp.lib()
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    P, nsf, nue = 100, 128, 8
    st = L.srslte_hip_stream_create()
    ev0, ev1 = L.srslte_hip_event_create(), L.srslte_hip_event_create()
    q = hp.Srs(P, 5, 0, max_srs=nsf * nue)
    ues = [hp.SrsUe.make(sf, n_srs=u, cs_used=1 << u) for sf in range(nsf) for u in range(nue)]  # each UE alone in its bin: 7 free bins
    d_grid = hp.DevBuf(8 * q.grid_len * nsf)
    L.srslte_hip_memset(d_grid.ptr, 0, d_grid.nbytes)
    d_res, d_ce = hp.DevBuf(C.sizeof(hp.SrsRes) * len(ues)), hp.DevBuf(8 * hp.SRS_MAX_CE * len(ues))

    def put():
        return q.put_device(d_grid.ptr, 0, nsf, ues, st)

    def rx():
        return q.rx_device(d_grid.ptr, 0, nsf, ues, d_res.ptr, d_ce.ptr, st)

    best = {}
    for _ in range(5):
        for name, fn in (("tx_put", put), ("rx_batch", rx)):
            assert fn() == 0
            L.srslte_hip_stream_sync(st)
            L.srslte_hip_event_record(ev0, st)
            for _ in range(steps):
                assert fn() == 0
            L.srslte_hip_event_record(ev1, st)
            L.srslte_hip_stream_sync(st)
            best[name] = min(best.get(name, 1e30), L.srslte_hip_event_elapsed_ms(ev0, ev1) / steps)
    # the put of the last UE of a subframe is what the grid holds (a put writes, it does not add): that UE reads |h| = 1, nothing in its free bins
    res_, _ = hp.Srs.read(d_res, d_ce, len(ues))
    last = [r for r, u in zip(res_, ues) if u.n_srs == nue - 1]
    out = {"metric": "srs_ms_per_call", "nof_prb": P, "subframes": nsf, "ues_per_subframe": nue, "M_sc": hp.srs_M_sc(q.cfg, ues[0]), "steps": steps,
           "tx_put_ms": round(best["tx_put"], 4), "tx_put_entries_per_s": round(len(ues) / best["tx_put"] * 1e3),
           "rx_batch_ms": round(best["rx_batch"], 4), "rx_batch_requests_per_s": round(len(ues) / best["rx_batch"] * 1e3),
           "last_ue_rsrp_exact": int(sum(abs(r.rsrp - 1) < 1e-4 and r.nof_ce == 72 for r in last)), "last_ue_count": len(last)}
    L.srslte_hip_event_destroy(ev0)
    L.srslte_hip_event_destroy(ev1)
    L.srslte_hip_stream_destroy(st)
    q.free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
