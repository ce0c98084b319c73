"""The float64 restatement of tests/sync_ref.py against tests/golden/sync.npz: the rows the reference's own sync.c (over this library's DFTs)
gave for the 48 drawn items of every configuration of the parity test, recorded by tests/gen_golden_sync.py on a machine with a GPU, and
against tests/golden/sync_64.npz and sync_384.npz: the same for the 24 drawn items of test_parity_sizes at those sizes. The items
are drawn again from the recorded seed. The frame is corrected by the CP-based CFO as the reference's build corrects it, with a float32
phasor per SIMD lane (sync_ref.reference_cfo): its drift grows with the frame's length, not with fft_size, and with the exact phase the
recorded peak_value of 4 of the 24 rows at 384 points lies 1.7e-4 from the restatement's (6.2e-5 at 128 points), with the phasor 1.2e-5
(1.6e-6). The device computes the exact phase and is held to the exact restatement (tests/test_gpu_sync.py). Same rules as the GPU test: discrete outputs equal wherever the restatement's smallest deciding margin
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


def _check(path, name):
    import test_gpu_sync as t
    g = np.load(path)
    N, mo, stride = int(g["fft_size"]), int(g["max_offset"]), int(g["in_stride"])
    n, frame = int(g["n_items"]) if "n_items" in g else 48, int(g["frame_size"]) if "frame_size" in g else stride
    x, items, _ = t._drawn_items(np.random.default_rng(int(g[name + ".seed"])), N, stride, n, known=name == "known")
    assert float(np.abs(x).sum()) == pytest.approx(float(g[name + ".checksum"]), rel=1e-6)
    rows = (pkg.SyncRes * n).from_buffer_copy(np.ascontiguousarray(g[name + ".rows"]).tobytes())
    cd, T, left_out = t._dict(pkg.sync_cfg(N, frame, mo, n, **t.PARITY[name])), sr.tol(N), 0
    for b in range(n):
        w, r = sr.find_one(x[b], cd, items[b].N_id_2, 0, items[b].N_id_1, frame_cfo=sr.reference_cfo), rows[b]
        if not min(w["margins"].values()) > 10 * T:
            left_out += 1
            continue
        for k in sr.DISCRETE:
            if k not in ("m0", "m1"):  # the driver has no getter for them
                assert getattr(r, k) == w[k], (name, b, k, getattr(r, k), w[k])
        for k in ("peak_value", "cfo", "sss_corr"):
            s = max(abs(w[k]), 1e-30) if sr.FLOATS[k] == "self" else sr.FLOATS[k]
            assert abs(getattr(r, k) - w[k]) / s <= T, (name, b, k, getattr(r, k), w[k])
    assert left_out <= 0.05 * n, (name, left_out)


@pytest.mark.skipif(not os.path.exists(GOLDEN), reason="tests/golden/sync.npz has not been recorded")
@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_the_recorded_reference_rows(name):
    _check(GOLDEN, name)


def _size_cases():
    """The files tests/gen_golden_sync.py records at the other sizes: 24 drawn items over 5 ms, find and known configurations."""
    out = []
    for N in (64, 384):
        path = os.path.join(ROOT, "tests", "golden", "sync_%d.npz" % N)
        for name in ("find", "known"):
            out.append(pytest.param(path, name, id="%d-%s" % (N, name),
                                    marks=pytest.mark.skipif(not os.path.exists(path), reason="tests/golden/sync_%d.npz has not been recorded" % N)))
    return out


@pytest.mark.parametrize("path,name", _size_cases())
def test_restatement_matches_the_recorded_reference_rows_at_other_sizes(path, name):
    _check(path, name)
