"""Writes tests/golden/meas.npz: for the 6-PRB and 25-PRB shapes of the parity test of tests/test_gpu_meas.py, the seed of its three drawn
captures and the result rows of the reference's own refsignal_dl_sync.c on them (tests/meas_dropin_driver.c over this library's DFTs, so it
runs on a machine with a GPU and the reference build). No samples are stored: tests/test_meas_golden.py draws them again from the seed.
    python tests/gen_golden_meas.py [out.npz]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import test_gpu_meas as t  # noqa: E402

SHAPES = [(6, 5), (25, 5), (6, 12)]  # nof_prb, nof_sf
A, B = 150, 29


def draw(nof_prb, nof_sf, seed):
    return t.two_cell_captures(nof_prb, t.mr.symbol_sz(nof_prb), nof_sf, 3, seed, a=A, b=B)[0]


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(t.ROOT, "tests", "golden", "meas.npz")
    drv = t.build_driver()
    assert drv is not None, "oracle/_ref/hip/libsrslte_upper.a is absent"
    ids = t.candidates(A, B)
    data = {"shapes": np.array(SHAPES), "ids": np.array(ids)}
    for nof_prb, nof_sf in SHAPES:
        name, seed = "%d_%d" % (nof_prb, nof_sf), 2000 + nof_prb + nof_sf
        x = draw(nof_prb, nof_sf, seed)
        rows = drv(nof_prb, nof_sf, x, [(cid, c) for c in range(3) for cid in ids])
        data[name + ".seed"] = seed
        data[name + ".rows"] = np.frombuffer(b"".join(bytes(r) for r in rows), np.uint32).reshape(len(rows), 16).copy()
        data[name + ".checksum"] = float(np.abs(x).sum())  # the drawn samples are the ones the rows belong to
    np.savez_compressed(out, **data)
    print("wrote", out)


if __name__ == "__main__":
    main()
