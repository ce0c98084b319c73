"""Writes tests/golden/sync.npz: for every configuration of the parity test of tests/test_gpu_sync.py, the seed and parameters of its 48 drawn
items and the result rows of the reference's own sync.c on them (tests/sync_dropin_driver.c over this library's DFTs, so it runs on a machine
with a GPU and the reference build). No samples are stored: tests/test_sync_golden.py draws them again from the seed.
    python tests/gen_golden_sync.py [out.npz]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import test_gpu_sync as t  # noqa: E402

N, MO = 128, 9600


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(t.ROOT, "tests", "golden", "sync.npz")
    drv = t.build_driver()
    assert drv is not None, "oracle/_ref/hip/libsrslte_upper.a is absent"
    data = {"fft_size": N, "max_offset": MO, "in_stride": MO + N, "names": np.array(sorted(t.PARITY))}
    for name in sorted(t.PARITY):
        seed = sorted(t.PARITY).index(name) + 100
        x, items, _ = t._drawn_items(np.random.default_rng(seed), N, MO + N, 48, known=name == "known")
        c = t.pkg.sync_cfg(N, MO + N, MO, 48, **t.PARITY[name])
        rows = drv(c, x, t._expand(items))
        data[name + ".seed"] = seed
        data[name + ".rows"] = np.frombuffer(b"".join(bytes(r) for r in rows), np.uint32).reshape(len(rows), 16).copy()
        data[name + ".checksum"] = float(np.abs(x).sum())  # the drawn samples are the ones the rows belong to
    np.savez_compressed(out, **data)
    print("wrote", out)


if __name__ == "__main__":
    main()
