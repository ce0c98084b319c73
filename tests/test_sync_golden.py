"""The float64 restatement of tests/sync_ref.py against tests/golden/sync.npz: the rows the reference's own sync.c (over this library's DFTs)
gave for the 48 drawn items of every configuration of the parity test, recorded by tests/gen_golden_sync.py on a machine with a GPU. The items
are drawn again from the recorded seed. Same rules as the GPU test: discrete outputs equal wherever the restatement's smallest deciding margin
exceeds 10 T, at most 5 % of the items left out; float outputs within T of the reference's."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import sync_ref as sr
from _libs import ROOT

pkg = importlib.import_module("srslte-emane_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden", "sync.npz")
NAMES = ["diff", "find", "find_ext", "full_cp", "known", "off"]


@pytest.mark.skipif(not os.path.exists(GOLDEN), reason="tests/golden/sync.npz has not been recorded")
@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_the_recorded_reference_rows(name):
    import test_gpu_sync as t
    g = np.load(GOLDEN)
    N, mo, stride = int(g["fft_size"]), int(g["max_offset"]), int(g["in_stride"])
    x, items, _ = t._drawn_items(np.random.default_rng(int(g[name + ".seed"])), N, stride, 48, known=name == "known")
    assert float(np.abs(x).sum()) == pytest.approx(float(g[name + ".checksum"]), rel=1e-6)
    rows = (pkg.SyncRes * 48).from_buffer_copy(np.ascontiguousarray(g[name + ".rows"]).tobytes())
    cd, T, left_out = t._dict(pkg.sync_cfg(N, stride, mo, 48, **t.PARITY[name])), sr.tol(N), 0
    for b in range(48):
        w, r = sr.find_one(x[b], cd, items[b].N_id_2, 0, items[b].N_id_1), rows[b]
        if not min(w["margins"].values()) > 10 * T:
            left_out += 1
            continue
        for k in sr.DISCRETE:
            if k not in ("m0", "m1"):  # the driver has no getter for them
                assert getattr(r, k) == w[k], (name, b, k, getattr(r, k), w[k])
        for k in ("peak_value", "cfo", "sss_corr"):
            s = max(abs(w[k]), 1e-30) if sr.FLOATS[k] == "self" else sr.FLOATS[k]
            assert abs(getattr(r, k) - w[k]) / s <= T, (name, b, k, getattr(r, k), w[k])
    assert left_out <= 0.05 * 48, (name, left_out)
