#!/usr/bin/env python3
"""What PSS / SSS / PBCH cost on the transmit side: the workload of scripts/bench_dl_tx_ctrl.py (128 subframes of a 100-PRB cell, one
full-band 64QAM PDSCH each, payloads resident on the device, one stream, a CFI-3 control region with six DCIs and eight PHICHs per subframe)
through srslte_hip_dl_tx_batch_grants_ctrl and through srslte_hip_dl_tx_batch_grants_full, and srslte_hip_dl_ctrl_tx_put_bcast alone on the
pipeline's grids. ms per call, best of 5 rounds, the three interleaved within each round. Prints one JSON line."""
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    hp = importlib.import_module("srslte-emane_amd")
    L = hp.lib()
    P, B, tbs, steps, cfi, cell_id = 100, 128, 75376, 40, 3, 1
    tx = hp.DlTx(cell_id, P, 1, 0x1234, 3, tbs, B)
    ctrl = hp.DlCtrlTx(P, 1, cell_id, phich_resources=1, max_batch=B, max_dci=6 * B, max_phich=8 * B)

    class TxGrant(C.Structure):
        _fields_ = [("sf", C.c_uint32), ("grant", hp.DlGrant)]
    arr = (TxGrant * B)(*[TxGrant(b, hp.DlGrant.make(P, 3, tbs, 0x100 + b, cfi=cfi)) for b in range(B)])
    stride = (tbs // 8 + 15) & ~15
    rng = np.random.default_rng(1)
    din = hp.DevBuf.from_host(rng.integers(0, 256, (B, stride), dtype=np.uint8))
    ng = hp.phich_ngroups(P, 1, cell_id, phich_resources=1)  # PHICH e of a subframe: group e % 3, sequence e // 3
    dcis, phichs = [], []
    for b in range(B):
        for k, (L_, ncce, fmt) in enumerate([(2, 0, hp.DCI_FORMAT1A), (2, 4, hp.DCI_FORMAT0)] + [(0, 8 + i, hp.DCI_FORMAT1) for i in range(4)]):
            m = hp.DciMsg()
            n = hp.dci_format_sizeof(P, 1, fmt)
            m.payload[:n] = rng.integers(0, 2, n).tolist()
            m.nof_bits, m.L, m.ncce, m.format, m.rnti = n, L_, ncce, fmt, 0x100 + 6 * b + k
            dcis.append((b, m))
        phichs += [hp.PhichTx(b, ng * (e // 3) + e % 3, 0, 0, e & 1) for e in range(8)]
    inp, keep = hp._ctrl_tx_in([cfi] * B, dcis, phichs)
    for fn in (L.srslte_hip_dl_tx_batch_grants_ctrl, L.srslte_hip_dl_tx_batch_grants_full):
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(hp.DlCtrlTxIn), C.c_void_p,
                       C.c_void_p]
    d_grid = L.srslte_hip_dl_tx_debug_buffer(tx.h, 3)

    def with_ctrl():
        assert L.srslte_hip_dl_tx_batch_grants_ctrl(tx.h, din.ptr, stride, 0, B, arr, B, ctrl.h, C.byref(inp), tx.d_iq.ptr, None) == 0

    def full():
        assert L.srslte_hip_dl_tx_batch_grants_full(tx.h, din.ptr, stride, 0, B, arr, B, ctrl.h, C.byref(inp), tx.d_iq.ptr, None) == 0

    def put():
        assert L.srslte_hip_dl_ctrl_tx_put_bcast(ctrl.h, 0, B, d_grid, None) == 0
    fns = {"ctrl": with_ctrl, "full": full, "put": put}
    for f in fns.values():
        for _ in range(5):
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
    print(json.dumps({"metric": "dl_tx_bcast_ms_per_call", "nof_prb": P, "batch": B, "cfi": cfi, "dci_per_sf": 6, "phich_per_sf": 8, "steps": steps,
                      "dl_tx_grants_ctrl_ms": round(best["ctrl"] * 1e3, 4), "dl_tx_grants_full_ms": round(best["full"] * 1e3, 4),
                      "bcast_put_alone_ms": round(best["put"] * 1e3, 4), "bcast_cost_ms": round((best["full"] - best["ctrl"]) * 1e3, 4)}))
    ctrl.free()
    tx.free()


if __name__ == "__main__":
    main()
