#!/usr/bin/env python3
"""What the PRACH costs: a 100-PRB cell, config_idx 3 (format 0, N_ifft_prach 18432), zero_corr_zone 1 (one root) and 0 (64 roots, the most
correlations), 128 and 1024 occasions per call with 4 preambles in each. srslte_hip_prach_detect_batch on a resident signal (ms per call and
occasions/s) and srslte_hip_prach_gen_batch of the 4 preambles of every occasion (preambles/s); best of 5 rounds of `steps` calls timed with
events on one stream. Beside them, where oracle/_ref/hip was built, the time of one srslte_prach_detect_offset of the reference's prach.c linked
against this library (its DFTs of 18432 and 839 points through srslte_dft_*; tests/prach_dropin_driver.c), else "not measured". One JSON line."""
import ctypes as C
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


def _driver_seconds(zczc, reps):
    lib_a = os.path.join(ROOT, "oracle", "_ref", "hip", "libsrslte_upper.a")
    if not os.path.exists(lib_a):
        return "not measured"
    csrc = os.path.join(ROOT, "srslte-emane_amd", "csrc")
    exe = os.path.join(tempfile.mkdtemp(), "prach_dropin_driver")
    subprocess.check_call(["gcc", "-std=c99", "-O2", os.path.join(ROOT, "tests", "prach_dropin_driver.c"), "-o", exe, lib_a, "-L" + csrc,
                           "-lsrslte_phy_hip", "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib", "-lstdc++", "-lm", "-lpthread"])
    out = subprocess.check_output([exe, "time", "100", "3", "0", str(zczc), str(reps)], timeout=300)
    return float(out.decode().split()[-1])


def main():
    hp = importlib.import_module("srslte-emane_amd")
    L = hp.lib()
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    P, cfg_idx = 100, 3
    st = L.srslte_hip_stream_create()
    ev0, ev1 = L.srslte_hip_event_create(), L.srslte_hip_event_create()
    res = {"metric": "prach_ms_per_call", "nof_prb": P, "config_idx": cfg_idx, "preambles_per_occasion": 4, "steps": steps}
    rng = np.random.default_rng(1)
    for zczc in (1, 0):
        for n in (128, 1024):
            q = hp.Prach(P, cfg_idx, max_occasions=n, max_preambles=4 * n, zero_corr_zone=zczc)
            info, Lp = q.info, q.len
            # 64 distinct occasions of 4 preambles each (sums of device-generated preambles), laid out once; occasion o reads signal o % 64
            sets = [[int(x) for x in rng.choice(64, 4, replace=False)] for _ in range(64)]
            rc, pre = q.gen([(s, 0) for ss in sets for s in ss])
            assert rc == 0
            sig = pre.reshape(64, 4, Lp).sum(axis=1).astype(np.complex64)
            d_sig = hp.DevBuf.from_host(sig)
            occ = [hp.PrachOccasion((o % 64) * Lp + info.N_cp, 0, 0) for o in range(n)]
            md = info.max_det
            dn, di, dt, dp = hp.DevBuf(4 * n), hp.DevBuf(4 * md * n), hp.DevBuf(4 * md * n), hp.DevBuf(4 * md * n)
            txs = [hp.PrachTx(sets[o % 64][k], 0) for o in range(n) for k in range(4)]
            d_gen = hp.DevBuf(8 * Lp * 4 * n)

            def det():
                return q.detect_device(d_sig.ptr, sig.size, occ, dn.ptr, di.ptr, dt.ptr, dp.ptr, st)

            def gen():
                return q.gen_device(txs, d_gen.ptr, st)

            best = {}
            for _ in range(5):
                for name, fn in (("detect", det), ("gen", gen)):
                    assert fn() == 0
                    L.srslte_hip_stream_sync(st)
                    L.srslte_hip_event_record(ev0, st)
                    for _ in range(steps):
                        assert fn() == 0
                    L.srslte_hip_event_record(ev1, st)
                    L.srslte_hip_stream_sync(st)
                    ms = L.srslte_hip_event_elapsed_ms(ev0, ev1) / steps
                    best[name] = min(best.get(name, 1e30), ms)
            nof = dn.to_host(np.uint32)
            idx = di.to_host(np.uint32).reshape(n, md)
            found = sum(sorted(idx[o, :nof[o]].tolist()) == sorted(sets[o % 64]) for o in range(n))
            key = "zczc%d_n%d" % (zczc, n)
            res[key + "_detect_ms"] = round(best["detect"], 4)
            res[key + "_occasions_per_s"] = round(n / best["detect"] * 1e3)
            res[key + "_gen_ms"] = round(best["gen"], 4)
            res[key + "_preambles_per_s"] = round(4 * n / best["gen"] * 1e3)
            res[key + "_occasions_exact"] = int(found)
            q.free()
        t = _driver_seconds(zczc, 3)
        res["zczc%d_reference_prach_c_ms_per_occasion" % zczc] = round(t * 1e3, 3) if isinstance(t, float) else t
    L.srslte_hip_event_destroy(ev0)
    L.srslte_hip_event_destroy(ev1)
    L.srslte_hip_stream_destroy(st)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
