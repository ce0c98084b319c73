"""Writes tests/golden/nbiot_sync.npz: what the reference's own NB-IoT synchronisation (tests/nbiot_sync_dropin_driver.c over
oracle/_ref/hip/libsrslte_upper.a and this library's srslte_dft_*) answers on the drawn inputs of tests/nbiot_sync_ref.py - the parity items
and the state script - plus its sequences: the 121 NPSS values, the 528 NSSS values of cell ids 0, 125, 126, 377 and 503, and the first 64
samples of the NPSS replica (srslte_npss_corr_init). The NSSS replica lives only inside srslte_nsss_synch_t and has no accessor, so it is
pinned through the recorded NSSS rows instead. No samples are stored: tests/test_nbiot_sync_golden.py redraws them from the seeds.
Run once on a machine with a GPU and the reference build:  python tests/gen_golden_nbiot_sync.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import nbiot_sync_ref as nr  # noqa: E402
from test_gpu_nbiot_sync import build_driver  # noqa: E402

NSSS_IDS = (0, 125, 126, 377, 503)


def npss_rows(rows):
    return np.array([[r.ret, r.peak_pos, r.peak_value, r.mean_cfo] for r in rows], np.float64)


def nsss_rows(rows):
    return np.array([[r.found, r.cell_id, r.peak_value] for r in rows], np.float64)


def main():
    drv = build_driver()
    if drv is None:
        raise SystemExit("oracle/_ref/hip/libsrslte_upper.a is missing: build it first")
    pin = nr.parity_inputs()
    out = dict(seeds=np.array([nr.SEEDS[k] for k in sorted(nr.SEEDS)], np.int64), seed_names=np.array(sorted(nr.SEEDS)))
    for key, fs in (("npss_3840", 3840), ("npss_19200", 19200)):
        ops = []
        for x in pin[key]:
            ops += [("reset", 0), ("find", 0, 0, x)]
        out[key] = npss_rows(drv.npss(dict(nr.PARITY_CFG, frame_size=fs), fs, 1, ops))
    x, given, made = pin["nsss"]
    out["nsss"] = nsss_rows(drv.nsss(x, given))
    out["nsss_given"], out["nsss_made"] = np.array(given, np.int32), np.array(made, np.int32)
    ops = []
    for pre, items in nr.state_script():
        ops += [(op[0],) + tuple(op[1:]) for op in pre]
        ops += [("find", t, 0, xi) for t, xi in items]
    cfg = dict(nr.PARITY_CFG, frame_size=nr.STATE_FRAME, npss_ema_alpha=0.2)
    out["state"] = npss_rows(drv.npss(cfg, nr.STATE_FRAME, 3, ops))
    seq = os.path.join(os.path.dirname(drv.exe), "seq.out")
    drv.run("seq", seq, "-")
    v = np.fromfile(seq, np.complex64)
    assert v.size == 121 + 528 * len(NSSS_IDS) + 64
    out["npss_seq"], out["nsss_ids"] = v[:121], np.array(NSSS_IDS, np.int32)
    out["nsss_seq"] = v[121:121 + 528 * len(NSSS_IDS)].reshape(len(NSSS_IDS), 528)
    out["npss_replica_head"] = v[-64:]
    path = os.path.join(HERE, "golden", "nbiot_sync.npz")
    np.savez_compressed(path, **out)
    print("wrote %s, %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
