"""The float64 restatement of tests/nbiot_sync_ref.py at the edges tests/test_gpu_nbiot_sync_edges.py runs on the device, against what the
reference's own code answered there (tests/golden/nbiot_sync_edges.npz, recorded by tests/gen_golden_nbiot_sync.py edges through
tests/nbiot_sync_dropin_driver.c; the inputs are redrawn here from the recorded seeds): psr() with the peak on lags 0 .. 3 and on the last
lag, the short branch at frame_size 2, 3 and 127, the long branch at 128, 129 and 286, the all-zero frame, and the NSSS with its peak in the
wrap lags and the tail tile. No GPU is needed.
The bound is tests/test_nbiot_sync_golden.py's: floats within sync_ref.tol(L) = 4 L 2^-24 of the restatement, relative to the figure's
scale, discrete outputs where the restatement's smallest margin exceeds 10 x that bound. Below frame_size 1507 the tie set of
nbiot_sync_ref.tie_step applies: the reference's position is accepted where the restatement's row is within 10 tol(L) of its maximum and the
rest is compared from there. On the planted frames, the zero frame and the NSSS items no row is left out.
In the short branch the reference reads past frame_size from a copy it corrected up to frame_size only - zeros in a fresh object - so the
restatement is given the frame followed by zeros."""
import os

import numpy as np
import pytest

import nbiot_sync_ref as nr
import sync_ref as sr

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nbiot_sync_edges.npz"))
CASES = nr.edge_golden_inputs()


def test_seeds_and_case_lists_are_the_recorded_ones():
    assert {str(k): int(v) for k, v in zip(G["seed_names"], G["seeds"])} == nr.EDGE_SEEDS
    assert [str(k) for k in G["npss_cases"]] == list(CASES)
    assert tuple(int(v) for v in G["planted_lags"]) == nr.EDGE_LAGS
    assert tuple(int(v) for v in G["nsss_lags"]) == nr.EDGE_NSSS_LAGS
    for name, (fs, x) in CASES.items():
        assert G[name].shape == (x.shape[0], 4), name


@pytest.mark.parametrize("name", list(CASES))
def test_npss_edge_rows_against_the_reference(name):
    fs, x = CASES[name]
    Tr, L = sr.tol(fs + nr.LEN), fs + nr.LEN
    cfg = dict(nr.EDGE_CFG, frame_size=fs)
    left = ties = 0
    for b in range(x.shape[0]):
        ret, pos, val, mean = G[name][b]
        xi = np.r_[x[b], np.zeros(nr.N - 1, np.complex64)] if fs < nr.N else x[b]
        if name == "zero_3840":
            w = nr.npss_find(xi, cfg, nr.new_track(fs))
            assert (w["ret"], w["peak_pos"], w["corr_peak"], w["mean_cfo"]) == (0, 0, 0.0, 0.0) and np.isnan(w["peak_value"])
            assert (ret, pos, mean) == (0, 0, 0) and np.isnan(val), G[name][b]
            continue
        if fs >= 1507:
            w = nr.npss_find(xi, cfg, nr.new_track(fs))
            assert nr.min_margin(w) > 10 * Tr and w["peak_pos"] == nr.EDGE_LAGS[b] % L, (name, b, w["margins"])
        else:
            w, tie = nr.tie_step(xi, cfg, nr.new_track(fs), 0, int(pos), Tr)
            ties += int(tie)
            if not nr.min_margin(w) > 10 * Tr:
                left += 1
                continue
        assert int(ret) == w["ret"] and int(pos) == w["peak_pos"], (name, b, G[name][b], w["ret"], w["peak_pos"], w["margins"])
        assert abs(val - w["peak_value"]) <= Tr * abs(w["peak_value"]), (name, b, val, w["peak_value"])
        assert abs(mean - w["mean_cfo"]) <= Tr, (name, b, mean, w["mean_cfo"])
    print("%s: %d rows, %d compared from the reference's position, %d left out" % (name, x.shape[0], ties, left))
    assert left <= 1, (name, left)


def test_psr_edges_are_among_the_recorded_rows():
    """What the planted rows at 1508 pin in psr(): peak <= 2 (empty left range), the first peak > 2, and peak = nout - 1 (the right walk ends
    at conv_len and the right range is empty)."""
    pos = [int(v) for v in G["planted_1508"][:, 1]]
    assert pos[:4] == [0, 1, 2, 3] and nr.nout(1508) - 1 in pos
    # by hand. Peak on the last of 4 lags: the right walk ends at conv_len 5, its range is empty and answers the zero there; the left walk
    # goes from 2 to 1, so the left range is avg[:1]
    assert nr.psr(np.array([5.0, 1.0, 2.0, 9.0]), 3, 5) == 9.0 / 5.0
    # peak 0: the left range is empty and answers avg[0], the peak itself
    assert nr.psr(np.array([3.0, 2.0, 1.0]), 0, 4) == 1.0


def test_nsss_edge_rows_against_the_reference():
    x, ids, lags = nr.edge_nsss()
    given = [v for c in ids for v in (c, -1)]
    assert np.array_equal(G["nsss_given"], given)
    Tr, L = sr.tol(nr.NSSS_IN + nr.LEN), nr.NSSS_IN + nr.LEN
    for i, cid in enumerate(given):
        w = nr.nsss_find(x[i // 2], {}, cid)
        assert min(w["margins"].values()) > 10 * Tr and w["peak_pos"] == lags[i // 2] % L, (i, w["margins"])
        found, got_id, val = G["nsss"][i]
        assert int(found) == w["found"] == 1 and int(got_id) == w["cell_id"] == ids[i // 2], (i, found, got_id, w["cell_id"])
        assert abs(val - w["peak_value"]) <= Tr * w["peak_value"], (i, val, w["peak_value"])
