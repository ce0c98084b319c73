"""The float64 restatement of tests/nbiot_sync_ref.py and the library's host sequences against what the reference's own code answered
(tests/golden/nbiot_sync.npz, recorded once by tests/gen_golden_nbiot_sync.py through tests/nbiot_sync_dropin_driver.c on a GPU machine; the
inputs are redrawn here from the recorded seeds). This leg needs no GPU and pins the restatement - which the GPU tests compare the device
with - to the reference.
The reference works in float32 through transforms of L = frame_size + 1508 points, so its floats may differ from the restatement's by
sync_ref.tol(L) = 4 L 2^-24, relative to the figure's scale; discrete outputs are compared where the restatement's smallest margin exceeds
10 x that bound, and a peak beside a near-equal neighbour may sit on either."""
import importlib
import os

import numpy as np
import pytest

import nbiot_sync_ref as nr
import sync_ref as sr

pkg = importlib.import_module("srslte-emane_amd")
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nbiot_sync.npz"))


def test_seeds_are_the_recorded_ones():
    assert {str(k): int(v) for k, v in zip(G["seed_names"], G["seeds"])} == nr.SEEDS


def test_sequences_against_the_reference():
    assert np.abs(pkg.nbiot_npss_generate() - G["npss_seq"]).max() <= 2e-7
    assert np.abs(nr.npss_seq().reshape(-1) - G["npss_seq"]).max() <= 2e-7
    for i, cid in enumerate(G["nsss_ids"]):
        assert np.abs(pkg.nbiot_nsss_generate(int(cid)) - G["nsss_seq"][i]).max() <= 4e-7, cid
        assert np.abs(nr.nsss_seq(int(cid)) - G["nsss_seq"][i]).max() <= 4e-7, cid
    h = G["npss_replica_head"]
    assert np.abs(pkg.nbiot_npss_replica()[:64] - h).max() <= sr.tol(128) * np.abs(h).max()
    assert np.abs(nr.npss_replica()[:64] - h).max() <= sr.tol(128) * np.abs(h).max()


def _npss_row(tag, w_fn, ref, Tr):
    """ref: (ret, peak_pos, peak_value, mean_cfo) of the reference. -> False when left out."""
    w = w_fn(None)
    near = False
    if "peak" in w["margins"] and w["margins"]["peak"] <= 10 * Tr:
        a, p = w["avg"], int(ref[1])
        b = np.array(a)
        b[w["peak_pos"]] = -1.0
        if abs(int(np.argmax(b)) - w["peak_pos"]) > 2:
            return False
        assert a[p] >= (1 - 10 * Tr) * a.max(), (tag, p, w["peak_pos"])
        w, near = w_fn(p), True
    if not nr.min_margin(w) > 10 * Tr:
        return False
    assert int(ref[0]) == w["ret"] and int(ref[1]) == w["peak_pos"], (tag, ref, w["ret"], w["peak_pos"], w["margins"])
    assert abs(ref[2] - w["peak_value"]) <= Tr * abs(w["peak_value"]), (tag, ref[2], w["peak_value"])
    assert abs(ref[3] - w["mean_cfo"]) <= Tr, (tag, ref[3], w["mean_cfo"])
    return True


@pytest.mark.parametrize("key,fs", [("npss_3840", 3840), ("npss_19200", 19200)])
def test_npss_parity_rows_against_the_reference(key, fs):
    x, cfg, Tr = nr.parity_inputs()[key], dict(nr.PARITY_CFG, frame_size=fs), sr.tol(fs + nr.LEN)
    left = 0
    for b in range(x.shape[0]):
        if not _npss_row((key, b), lambda p, b=b: nr.npss_find(x[b], cfg, nr.new_track(fs), 0, force_peak=p), G[key][b], Tr):
            left += 1
    print("%s: %d of %d rows left out" % (key, left, x.shape[0]))
    assert left <= 0.15 * x.shape[0]  # the margin asked is 10 tol(L), up to 13 times the GPU test's 10 T


def test_state_rows_against_the_reference():
    fs, Tr = nr.STATE_FRAME, sr.tol(nr.STATE_FRAME + nr.LEN)
    cfg = dict(nr.PARITY_CFG, frame_size=fs, npss_ema_alpha=0.2)
    tracks = [nr.new_track(fs) for _ in range(3)]
    i = left = 0
    for pre, items in nr.state_script():
        for op in pre:
            if op[0] == "reset":
                tracks[op[1]] = nr.new_track(fs)
            else:
                tracks[op[1]]["mean_cfo"] = float(np.float32(op[2]))
        for t, xi in items:
            before = {"avg": tracks[t]["avg"].copy(), "mean_cfo": tracks[t]["mean_cfo"]}

            def run(p, t=t, xi=xi, before=before):
                tracks[t] = {"avg": before["avg"].copy(), "mean_cfo": before["mean_cfo"]}
                return nr.npss_find(xi, cfg, tracks[t], 0, force_peak=p)

            left += 0 if _npss_row(("state", i), run, G["state"][i], Tr) else 1
            i += 1
    assert i == G["state"].shape[0] == 14
    assert left <= 2, left


def test_nsss_rows_against_the_reference():
    (x, given, made), exp = nr.parity_inputs()["nsss"], nr.parity_expected()["nsss"]
    assert np.array_equal(G["nsss_given"], given) and np.array_equal(G["nsss_made"], made)
    Tr, left = sr.tol(nr.NSSS_IN + nr.LEN), 0
    for b, w in enumerate(exp):
        found, cid, val = G["nsss"][b]
        m = min(v for k, v in w["margins"].items() if k != "peak")  # the reference's peak position has no getter
        if not m > 10 * Tr:
            left += 1
            continue
        assert int(found) == w["found"] and int(cid) == (w["cell_id"] if w["found"] or given[b] >= 0 else -1), (b, found, cid, w["cell_id"])
        assert abs(val - w["peak_value"]) <= Tr * w["peak_value"], (b, val, w["peak_value"])
    print("nsss: %d of %d rows left out" % (left, len(exp)))
    assert left <= 0.15 * len(exp)
