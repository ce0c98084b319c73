"""Writes tests/golden/sync_track.npz: for every sequence of the FDD and the TDD / detection parity tests of tests/test_gpu_sync_track.py, the
seed and parameters it is drawn from and the rows the reference's own sync.c gave over the sequence (tests/sync_track_dropin_driver.c over
this library's DFTs, so it runs on a machine with a GPU and the reference build). No samples are stored: tests/test_sync_track_golden.py
draws them again from the seed.
    python tests/gen_golden_sync_track.py [out.npz]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import test_gpu_sync_track as t  # noqa: E402


def sequences():
    """name -> (sync keywords, cfo_ema_alpha, frame mode, known-cell branch, x, kinds, seed)"""
    out = {}
    for name in sorted(t.FDD_SEQ):
        kw, cfo_alpha, x, kinds = t.fdd_sequence(name)
        out["fdd_" + name] = (kw, cfo_alpha, 0, False, x, kinds, t.FDD_SEED[name])
    for name in sorted(t.TDD_SEQ):
        mode, known, kw, x, kinds = t.tdd_sequence(name)
        out[name] = (kw, 0.0, mode, known, x, kinds, t.TDD_SEED[name])
    return out


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(t.ROOT, "tests", "golden", "sync_track.npz")
    drv = t.build_track_driver()
    assert drv is not None, "oracle/_ref/hip/libsrslte_upper.a is absent"
    seqs = sequences()
    data = {"fft_size": t.N, "max_offset": t.MO, "in_stride": t.STRIDE, "names": np.array(sorted(seqs))}
    for name, (kw, cfo_alpha, mode, known, x, kinds, seed) in seqs.items():
        n_calls, n_tracks = x.shape[:2]
        c = t.pkg.sync_cfg(t.N, t.STRIDE, t.MO, n_tracks, **kw)
        tc = t.pkg.SyncTracksCfg(n_tracks, cfo_alpha, mode)
        rows = drv(c, tc, x, [t._items(kinds, known)] * n_calls, [[(0, 0)] * n_tracks] * n_calls)
        data[name + ".seed"] = seed
        data[name + ".rows"] = np.frombuffer(b"".join(bytes(r) for call in rows for r in call), np.uint32).reshape(n_calls, n_tracks, 24).copy()
        data[name + ".checksum"] = float(np.abs(x).sum())  # the drawn samples are the ones the rows belong to
    np.savez_compressed(out, **data)
    print("wrote", out)


if __name__ == "__main__":
    main()
