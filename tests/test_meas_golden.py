"""The float64 restatement of tests/meas_ref.py against tests/golden/meas.npz: the rows the reference's own refsignal_dl_sync.c (over this
library's DFTs) gave for three drawn captures x six candidate cells at 6 and 25 PRB, recorded by tests/gen_golden_meas.py on a machine with
a GPU. The captures are drawn again from the recorded seed. Same rules as the GPU test: found and peak_index equal wherever the
restatement's smallest deciding margin exceeds 10 T(sf_len), at most 5 % of the rows left out; the figures the reference's object keeps
within T(symbol_sz) of the restatement's, in units of their scales."""
import importlib
import os

import numpy as np
import pytest

import meas_ref as mr
from _libs import ROOT

pkg = importlib.import_module("srslte-emane_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden", "meas.npz")
SHAPES = [(6, 5), (25, 5), (6, 12)]


@pytest.mark.skipif(not os.path.exists(GOLDEN), reason="tests/golden/meas.npz has not been recorded")
@pytest.mark.parametrize("nof_prb,nof_sf", SHAPES)
def test_restatement_matches_the_recorded_reference_rows(nof_prb, nof_sf):
    import gen_golden_meas as gg
    g = np.load(GOLDEN)
    name, ids = "%d_%d" % (nof_prb, nof_sf), [int(i) for i in g["ids"]]
    N = mr.symbol_sz(nof_prb)
    x = gg.draw(nof_prb, nof_sf, int(g[name + ".seed"]))
    assert float(np.abs(x).sum()) == pytest.approx(float(g[name + ".checksum"]), rel=1e-6)
    rows = (pkg.MeasRes * 18).from_buffer_copy(np.ascontiguousarray(g[name + ".rows"]).tobytes())
    Ts, Tm, left_out, found = mr.tol(15 * N), mr.tol(N), 0, 0
    for i, r in enumerate(rows):
        w = mr.run_one(x[i // 6].astype(complex), nof_sf, ids[i % 6], nof_prb, N)
        assert r.cell_id == ids[i % 6]
        if not min(w["margins"].values()) > 10 * Ts:
            left_out += 1
            continue
        assert r.found == w["found"] and r.peak_index == w["peak_index"], (name, i, r.found, r.peak_index, w)
        found += w["found"]
        for k, kind in mr.MEAS_FLOATS.items():
            if k in ("rsrp_lin", "rssi_lin"):  # the object keeps only the dB figures
                continue
            if not w["found"]:
                assert np.isnan(getattr(r, k)), (name, i, k)
                continue
            scale = 10 / np.log(10) if kind == "dB" else mr.HZ_PER_RAD
            assert abs(getattr(r, k) - w[k]) / scale <= Tm, (name, i, k, getattr(r, k), w[k])
    assert left_out <= 0.05 * 18 and found == 6, (name, left_out, found)
