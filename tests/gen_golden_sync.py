"""Writes the recorded rows of the reference's own sync.c (tests/sync_dropin_driver.c over this library's DFTs, so it runs on a machine with a GPU
and the reference build) that tests/test_sync_golden.py holds the float64 restatement against. No samples are stored: the test draws them again
from the seed, and the checksum says they are the ones the rows belong to.
    python tests/gen_golden_sync.py [fft_size [out.npz]]
fft_size 128 (the default): tests/golden/sync.npz, every configuration of the parity test of tests/test_gpu_sync.py on its 48 drawn items.
Another fft_size: tests/golden/sync_<fft_size>.npz, the find and known configurations of test_parity_sizes on its 24 drawn items over 5 ms (a
configuration that test does not run at this size takes the seed of its find configuration)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import test_gpu_sync as t  # noqa: E402

SIZE_NAMES = ("find", "known")


def cases(N):
    """-> (names, n items, frame_size, max_offset, in_stride, name -> (seed, x, items))."""
    if N == 128:
        names, n, mo = sorted(t.PARITY), 48, 9600

        def draw(name):
            seed = sorted(t.PARITY).index(name) + 100
            x, items, _ = t._drawn_items(np.random.default_rng(seed), N, mo + N, n, known=name == "known")
            return seed, x, items
        return names, n, mo + N, mo, mo + N, draw

    def draw(name):
        seed = t.SIZES_SEED.get((N, name), t.SIZES_SEED[N, "find"])
        x, items, _, _, _ = t.sizes_items(N, name, seed)
        return seed, x, items
    return list(SIZE_NAMES), 24, 75 * N, 75 * N, 76 * N, draw


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(t.ROOT, "tests", "golden", "sync.npz" if N == 128 else "sync_%d.npz" % N)
    drv = t.build_driver()
    assert drv is not None, "oracle/_ref/hip/libsrslte_upper.a is absent"
    names, n, frame, mo, stride, draw = cases(N)
    data = {"fft_size": N, "max_offset": mo, "in_stride": stride, "frame_size": frame, "n_items": n, "names": np.array(names)}
    for name in names:
        seed, x, items = draw(name)
        c = t.pkg.sync_cfg(N, frame, mo, n, **t.PARITY[name])
        rows = drv(c, x, t._expand(items))
        data[name + ".seed"] = seed
        data[name + ".rows"] = np.frombuffer(b"".join(bytes(r) for r in rows), np.uint32).reshape(len(rows), 16).copy()
        data[name + ".checksum"] = float(np.abs(x).sum())  # the drawn samples are the ones the rows belong to
    np.savez_compressed(out, **data)
    print("wrote", out)


if __name__ == "__main__":
    main()
