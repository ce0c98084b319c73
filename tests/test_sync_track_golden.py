"""The float64 restatement of tests/sync_track_ref.py against tests/golden/sync_track.npz: the rows the reference's own sync.c (over this
library's DFTs, one object per track kept alive over the sequence) gave for the sequences of the FDD and the TDD / detection parity tests,
recorded by tests/gen_golden_sync_track.py on a machine with a GPU. The sequences are drawn again from the recorded seeds. The rules are
those of the GPU test: a track is compared up to the first call whose smallest deciding margin is not above 10 T, at most 5 % of the rows
are left out, and a track is not compared from the call on in which the reference reads an uninitialised stack value."""
import importlib
import os

import numpy as np
import pytest

import sync_ref as sr
import sync_track_ref as st
from _libs import ROOT

pkg = importlib.import_module("srslte-emane_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden", "sync_track.npz")
NAMES = ["fdd_a0.3_c0.1", "fdd_a0.3_c0.8", "fdd_a1.0_c0.1", "fdd_a1.0_c0.8", "detect_full_a0.3", "detect_known_ext", "tdd_ext_diff", "tdd_find"]


@pytest.mark.skipif(not os.path.exists(GOLDEN), reason="tests/golden/sync_track.npz has not been recorded")
@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_the_recorded_reference_sequences(name):
    import gen_golden_sync_track as gen
    import test_gpu_sync as tg
    g = np.load(GOLDEN)
    assert sorted(g["names"]) == sorted(NAMES)
    kw, cfo_alpha, mode, known, x, kinds, seed = gen.sequences()[name]
    assert seed == int(g[name + ".seed"]) and float(np.abs(x).sum()) == pytest.approx(float(g[name + ".checksum"]), rel=1e-6)
    n_calls, n_tracks = x.shape[:2]
    N, T = int(g["fft_size"]), sr.tol(int(g["fft_size"]))
    rec = np.ascontiguousarray(g[name + ".rows"])
    cd = tg._dict(pkg.sync_cfg(N, int(g["in_stride"]), int(g["max_offset"]), n_tracks, **kw))
    left_out = compared = 0
    for t, kd in enumerate(kinds):
        trk, alive, defined = st.Track(cd, cfo_alpha, mode), True, True
        for k in range(n_calls):
            if not alive:
                left_out += 1
                continue
            w = trk.find(x[k, t], kd["cid"] % 3, 0, kd["cid"] // 3 if known else -1)
            if not min(w["margins"].values()) > 10 * T:
                alive = False
                left_out += 1
                continue
            defined = defined and not w["undefined_in_reference"]
            if not defined:
                continue
            r = pkg.SyncTrackRes.from_buffer_copy(rec[k, t].tobytes())
            compared += 1
            for f in st.DISCRETE:
                if f not in ("m0", "m1", "frame_type"):  # no getters in the reference
                    assert getattr(r, f) == w[f], (name, k, t, f, getattr(r, f), w[f])
            for f in ("peak_value", "cfo", "sss_corr"):
                s = max(abs(w[f]), 1e-30) if sr.FLOATS[f] == "self" else sr.FLOATS[f]
                # known-cell branch: sss_corr is the RATIO of two 62-term correlations; the smaller is what cancellation leaves, its float32
                # error is T of the larger one's scale, so the reference's own ratio carries a relative error of T x ratio
                cond = max(1.0, abs(w[f])) if known and f == "sss_corr" else 1.0
                assert abs(getattr(r, f) - w[f]) / s <= T * cond, (name, k, t, f, getattr(r, f), w[f])
    assert left_out <= 0.05 * n_calls * n_tracks, (name, left_out)
    assert compared >= 0.5 * n_calls * n_tracks, (name, compared)
