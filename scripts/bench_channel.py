"""Throughput of the batched channel emulator (srslte_hip_channel_run_batch): 20 MHz (23.04 MHz sampling), 8 channels x 128 subframes per call,
etu300 (N = 1024) alone and with delay, HST, RLF and AWGN behind it, and the other stages without fading. Reports samples/s, subframes/s and the
algorithmic bytes (input read once, output written once) per second beside a device-to-device copy of the same bytes timed in the same run.
Prints one JSON line; these are records, not thresholds.

    python scripts/bench_channel.py [--channels 8] [--nsf 128] [--reps 20]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch  # before the library: torch only finds the GPU through its own HIP runtime (tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--nsf", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    hp = importlib.import_module("srslte-emane_amd")
    srate, sf_len = 23.04e6, 23040
    n = a.channels * a.nsf * sf_len
    x = torch.view_as_real(torch.randn(n, dtype=torch.complex64, device="cuda"))
    y = torch.empty_like(x)
    d_in, d_out = hp.DevView(x.data_ptr(), 8 * n), hp.DevView(y.data_ptr(), 8 * n)
    stream = torch.cuda.current_stream().cuda_stream
    nbytes = 2 * 8 * n
    out = dict(srate_hz=srate, channels=a.channels, subframes_per_channel=a.nsf, samples_per_call=n, algorithmic_bytes_per_call=nbytes)
    copy_ms = _timed(lambda: y.copy_(x), a.reps)
    out["d2d_copy"] = dict(ms=copy_ms, GBps=nbytes / copy_ms / 1e6)
    others = dict(delay=(10.0, 100.0, 1.0, 0.0), hst=(750.0, 7.2, 0.0), rlf=(500, 30), awgn=(0.01, 1))
    for name, stages in (("etu300", dict(fading="etu300")), ("etu300_delay_hst_rlf_awgn", dict(fading="etu300", **others)),
                         ("delay_hst_rlf_awgn", others)):
        ch = hp.Channel(hp.channel_cfg(srate, a.channels, a.nsf, sf_len, **stages))
        t = [0]

        def call():
            assert ch.run_dev(d_in, d_out, a.nsf, sf_len, t[0], 0.25, stream=stream) == 0
            t[0] += 1

        ms = _timed(call, a.reps)
        out[name] = dict(ms=ms, samples_per_s=n / ms * 1e3, subframes_per_s=a.channels * a.nsf / ms * 1e3, GBps=nbytes / ms / 1e6,
                         of_d2d_copy=copy_ms / ms, fft_size=ch.fft_size)
        ch.free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
