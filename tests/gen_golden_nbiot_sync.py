"""Writes tests/golden/nbiot_sync.npz: what the reference's own NB-IoT synchronisation (tests/nbiot_sync_dropin_driver.c over
oracle/_ref/hip/libsrslte_upper.a and this library's srslte_dft_*) answers on the drawn inputs of tests/nbiot_sync_ref.py - the parity items
and the state script - plus its sequences: the 121 NPSS values, the 528 NSSS values of cell ids 0, 125, 126, 377 and 503, and the first 64
samples of the NPSS replica (srslte_npss_corr_init). The NSSS replica lives only inside srslte_nsss_synch_t and has no accessor, so it is
pinned through the recorded NSSS rows instead. No samples are stored: tests/test_nbiot_sync_golden.py redraws them from the seeds.

A second file, tests/golden/nbiot_sync_edges.npz, holds the reference's rows on nbiot_sync_ref.edge_golden_inputs(): the edges
tests/test_gpu_nbiot_sync_edges.py runs on the device, each item with find_offset 0 and mean_cfo 0 on a reset srslte_sync_nbiot_t - noise at
frame_size 2, 3, 127 (short branch) and 128, 129, 286, the planted lags at 1508, the all-zero frame at 3840 - and the 18 planted NSSS items.
Again seeds, case lists and rows only; tests/test_nbiot_sync_edges_golden.py redraws the inputs. Left out: frame_size 1 (the reference's loop
leaves conv_output_len - 1 = 0 values, and its float outputs there are whatever its buffers held), 307200, whose L = frame_size + 1508
exceeds the library's DFT limit of 131072 points, and 66000, which is beyond the 19200 samples of the reference's corrected copy.
In the short branch the reference reads 127 samples past frame_size from a copy it corrected up to frame_size only; in a fresh object that
tail is zeros, and the golden's short items are the frame followed by zeros for the restatement as well.
Run once on a machine with a GPU and the reference build:  python tests/gen_golden_nbiot_sync.py [parity] [edges]   (default: both)"""
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


def edges(drv):
    out = dict(seeds=np.array([nr.EDGE_SEEDS[k] for k in sorted(nr.EDGE_SEEDS)], np.int64), seed_names=np.array(sorted(nr.EDGE_SEEDS)))
    names = []
    for name, (fs, x) in nr.edge_golden_inputs().items():
        ops = []
        for xi in x:
            ops += [("reset", 0), ("find", 0, 0, xi)]
        out[name] = npss_rows(drv.npss(dict(nr.EDGE_CFG, frame_size=fs), x.shape[1], 1, ops))
        names.append(name)
    out["npss_cases"], out["planted_lags"] = np.array(names), np.array(nr.EDGE_LAGS, np.int32)
    x, ids, lags = nr.edge_nsss()
    given = [v for c in ids for v in (c, -1)]
    out["nsss"] = nsss_rows(drv.nsss(np.repeat(x, 2, axis=0), given))
    out["nsss_given"], out["nsss_lags"] = np.array(given, np.int32), np.array(lags, np.int32)
    path = os.path.join(HERE, "golden", "nbiot_sync_edges.npz")
    np.savez_compressed(path, **out)
    print("wrote %s, %d bytes" % (path, os.path.getsize(path)))


def main():
    which = sys.argv[1:] or ["parity", "edges"]
    drv = build_driver()
    if drv is None:
        raise SystemExit("oracle/_ref/hip/libsrslte_upper.a is missing: build it first")
    if "edges" in which:
        edges(drv)
    if "parity" in which:
        parity(drv)


def parity(drv):
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
