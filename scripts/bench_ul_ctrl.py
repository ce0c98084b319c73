#!/usr/bin/env python3
"""What the PUCCH costs on the eNB side: 128 subframes of a 100-PRB cell with 16 PUCCHs per subframe mixing the six formats (SR, 1 / 2 HARQ-ACK
bits, CQI reports of 4-11 bits, reports with HARQ-ACK; one PRB pair each), received through srslte_hip_ul_ctrl_pucch_batch alone on a resident grid, and the
grants pipeline with the same PUSCH load (two PUSCHs per subframe) through srslte_hip_ul_rx_batch_grants and _grants_pucch. ms per call, best
of 5 rounds, interleaved within each round. Beside it, as an upper bound of what the reference's CPU chain costs per PUCCH, the chain of
tests/ul_ctrl_ref.py driven from Python (one core; needs oracle/_ref, else "not measured"). Prints one JSON line."""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    hp = importlib.import_module("srslte-emane_amd")
    P, B, cell_id, steps, tti0 = 100, 128, 1, 20, 0
    kw = dict(delta_pucch_shift=2, N_cs=0, n_rb_2=8, N_pucch_1=0, group_hopping_en=True, threshold_format1=0.8, threshold_data_valid_format1a=0.9,
              threshold_data_valid_format2=0.5)
    rng = np.random.default_rng(1)
    reqs, txs = [], []
    for b in range(B):
        j1 = j2 = 0
        for k in range(16):
            kind = k % 6
            # one PRB pair per UE (the reference's estimator does not separate PUCCHs that share a PRB): formats 2-2b at m = 0-7, formats
            # 1-1b at m = 8 + j (18 resources per PRB with delta_pucch_shift 2); PRBs 0-8 and 91-99, the PUSCHs at 10-39 and 50-79
            mk = dict(ncce=18 * j1, n_pucch_sr=18 * j1, n_pucch_2=12 * j2)
            if kind < 3:
                j1 += 1
            else:
                j2 += 1
            if kind == 0:
                q = hp.PucchReq.make(b, 0x46 + k, sr_tti=True, **mk)
            elif kind in (1, 2):
                q = hp.PucchReq.make(b, 0x46 + k, ack_len=kind, **mk)
            elif kind == 3:
                q = hp.PucchReq.make(b, 0x46 + k, cqi_len=4 + k % 8, **mk)
            else:
                q = hp.PucchReq.make(b, 0x46 + k, cqi_len=4 + k % 8, ack_len=kind - 3, simul_cqi_ack=True, **mk)
            q.noise_estimate = 0.01
            reqs.append(q)
            txs.append(hp.PucchTx.make(q, ack=(k & 1, (k >> 1) & 1), sr=1 if kind == 0 else 0, cqi=[int(x) for x in rng.integers(0, 2, q.cqi_len)]))
    glen = 14 * 12 * P
    ctx = hp.UlCtrlTx(P, cell_id, max_pucch=len(txs), **kw)
    grid = np.zeros((B, glen), np.complex64)
    for k in range(16):  # each UE its own grid; the receiver sees their sum
        rc, g = ctx.put(np.zeros((B, glen), np.complex64), tti0, txs[k::16])
        assert rc == 0
        grid += g
    ctx.free()
    ctrl = hp.UlCtrl(P, cell_id, max_pucch=len(reqs), **kw)
    d_grid = hp.DevBuf.from_host(grid)
    d_res, d_res2 = hp.DevBuf(64 * len(reqs)), hp.DevBuf(64 * len(reqs))
    import ctypes as C
    arr = (hp.PucchReq * len(reqs))(*reqs)
    L = hp.lib()

    def pucch():
        assert L.srslte_hip_ul_ctrl_pucch_batch(ctrl.h, d_grid.ptr, tti0, B, arr, len(reqs), d_res.ptr, None) == 0
    # the same PUSCH load through both grants calls: two PUSCHs per subframe in the middle of the band
    grants = []
    for b in range(B):
        grants += [hp.UlGrant.make(b, 0x400, 30, 10, 2, 15264), hp.UlGrant.make(b, 0x401, 30, 50, 2, 15264)]
    utx = hp.UlTx(cell_id, P, 0x1234, 2, 15264, 30, 10, 0, B, max_grants=len(grants))
    datas = [rng.integers(0, 256, 15264 // 8, dtype=np.uint8) for _ in grants]
    iq = utx.encode_grants(datas, tti0, B, grants).reshape(B, -1)
    utx.free()
    ofdm = hp.Ofdm(P, True, rx=False)  # the PUCCHs in the air beside the PUSCHs: SC-FDMA with the UL half-carrier shift
    ofdm.set_freq_shift(0.5)
    iq = (iq + ofdm.tx_sf(grid)).astype(np.complex64)
    ofdm.free()
    rx = hp.UlRx(cell_id, P, 0x1234, 2, 15264, 30, 10, 0, 6, B, max_grants=len(grants))
    d_iq = hp.DevBuf.from_host(iq)
    garr = (hp.UlGrant * len(grants))(*grants)
    L.srslte_hip_ul_rx_batch_grants.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                                C.c_void_p]

    def grants_only():
        assert L.srslte_hip_ul_rx_batch_grants(rx.h, d_iq.ptr, tti0, B, garr, len(grants), rx.d_tb.ptr, rx.tb_stride, rx.d_ok.ptr, None) == 0

    def grants_pucch():
        assert L.srslte_hip_ul_rx_batch_grants_pucch(rx.h, d_iq.ptr, tti0, B, garr, len(grants), rx.d_tb.ptr, rx.tb_stride, rx.d_ok.ptr, ctrl.h, arr,
                                                     len(reqs), d_res2.ptr, None) == 0
    fns = {"pucch": pucch, "grants": grants_only, "grants_pucch": grants_pucch}
    for f in fns.values():
        for _ in range(3):
            f()
    hp.sync()
    best = {k: 1e9 for k in fns}
    for _ in range(5):
        for k, f in fns.items():
            t0 = time.perf_counter()
            for _ in range(steps):
                f()
            hp.sync()
            best[k] = min(best[k], (time.perf_counter() - t0) / steps)
    res, res2 = (hp.PucchRes * len(reqs))(), (hp.PucchRes * len(reqs))()
    _ = L.srslte_hip_memcpy_d2h(C.addressof(res), d_res.ptr, C.sizeof(res))
    _ = L.srslte_hip_memcpy_d2h(C.addressof(res2), d_res2.ptr, C.sizeof(res2))
    detected, detected2 = sum(r.detected for r in res), sum(r.detected for r in res2)
    ok = int(rx.d_ok.to_host(np.uint8)[:len(grants)].sum())
    cpu = "not measured"
    from _libs import ref
    if ref() is not None:
        from ul_ctrl_ref import RefUlCtrl
        from _libs import aligned
        R = RefUlCtrl(ctrl.cfg)
        n = 0
        t0 = time.perf_counter()
        for q in reqs[:160]:
            g = aligned(glen, np.complex64)
            g[:] = grid[q.sf]
            R.decode(g, tti0 + q.sf, q)
            n += 1
        cpu = round((time.perf_counter() - t0) / n * 1e3, 4)
    print(json.dumps({"metric": "ul_ctrl_ms_per_call", "nof_prb": P, "batch": B, "pucch_per_sf": 16, "pucch_per_call": len(reqs), "puschs_per_call": len(grants),
                      "steps": steps, "pucch_batch_ms": round(best["pucch"] * 1e3, 4), "ul_rx_grants_ms": round(best["grants"] * 1e3, 4),
                      "ul_rx_grants_pucch_ms": round(best["grants_pucch"] * 1e3, 4),
                      "pucch_in_pipeline_ms": round((best["grants_pucch"] - best["grants"]) * 1e3, 4), "pucch_detected": int(detected),
                      "pucch_detected_in_pipeline": int(detected2), "pusch_crc_ok": ok,
                      "cpu_reference_chain_ms_per_pucch_python_driven": cpu}))
    ctrl.free()
    rx.free()


if __name__ == "__main__":
    main()
