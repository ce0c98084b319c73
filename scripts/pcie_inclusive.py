#!/usr/bin/env python3
"""The PCIe-inclusive rate of the headline workload (cfg2: 128 subframes of 100 PRB, 64QAM, TBS 75376 per batch, four HIP streams): every
step first copies its batch's time samples (128 x 184 320 B) from pinned host memory to the device on the step's own stream, then runs the
fused receive pipeline, then copies the transport blocks back - against the same loop with the samples already resident in HBM (what
bench.py's `value` is). The batched API takes device pointers; this is what a host-fed caller would see. One JSON object on stdout.

--iq sc16: the samples are int16 pairs as a radio delivers them (scale 2048, peak at 0.95 of full scale / 16: 12 bits), 128 x 92 160 B per
batch, converted inside the OFDM kernel (phy_hip.h, "Sample formats"). --pool-host: the same two loops from ONE host thread through
srslte_hip_dl_rx_pool_submit (resident) and srslte_hip_dl_rx_pool_submit_host (copy included), a pool of --streams objects.

  python scripts/pcie_inclusive.py [--steps 40] [--snr 18] [--iq {cf32,sc16}] [--pool-host]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--snr", type=float, default=18.0)
    ap.add_argument("--streams", type=int, default=4)
    ap.add_argument("--iq", choices=("cf32", "sc16"), default="cf32")
    ap.add_argument("--pool-host", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: the product has no CPU path")
    pkg = importlib.import_module("srslte-emane_amd")
    prb, mod, tbs, B = 100, 3, 75376, 128
    rng = np.random.default_rng(3)
    tx = pkg.DlTx(1, prb, 1, 0x1234, mod, tbs, B)
    data = rng.integers(0, 256, (B, tbs // 8), dtype=np.uint8)
    iq = tx.encode(data, 0)[:, 0, :]
    tx.free()
    sigma = np.sqrt(np.mean(np.abs(iq) ** 2) / 2) * 10 ** (-args.snr / 20)
    iq = (iq + sigma * (rng.standard_normal(iq.shape) + 1j * rng.standard_normal(iq.shape))).astype(np.complex64)
    sc16, scale = args.iq == "sc16", 2048.0
    if sc16:  # what srslte_vec_convert_fi makes of the samples at 12 bits: product in fp32, truncated
        iq = (iq * (0.95 / np.abs(iq.view(np.float32)).max())).astype(np.complex64)
        h_iq = torch.from_numpy(np.trunc(iq.view(np.float32) * np.float32(scale)).astype(np.int16)).pin_memory()
    else:
        h_iq = torch.from_numpy(iq.view(np.float32).copy()).pin_memory()
    hc = pkg.ChestDlCfg()
    hc.filter_coef[0], hc.filter_coef[1] = 4.0, 1.0
    n = args.streams
    tstreams = [torch.cuda.current_stream()] + [torch.cuda.Stream() for _ in range(n - 1)]
    d_iq = [torch.empty_like(h_iq, device="cuda") for _ in range(n)]
    for d in d_iq:
        d.copy_(h_iq)
    rxs = [pkg.DlRx(1, prb, 1, 0x1234, mod, tbs, 6, B, True, hc) for _ in range(1 if args.pool_host else n)]
    pool = pkg.DlRxPool(rxs[0].cfg, n) if args.pool_host else None
    if sc16:
        for r in rxs + ([pool] if pool else []):
            assert r.set_iq_format(pkg.IQ_SC16, scale) == 0
    d_res = [torch.zeros(rxs[0].tb_stride * B + B, dtype=torch.uint8, device="cuda") for _ in range(n)]
    h_res = [torch.zeros(rxs[0].tb_stride * B + B, dtype=torch.uint8).pin_memory() for _ in range(n)]
    L = pkg.lib()
    import ctypes as C
    L.srslte_hip_dl_rx_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]

    def run(copy_in):
        def pool_step(k):
            s = k % n  # submit waits for the batch that used object s before: d_res[s] and h_res[s] are free again
            tb, ok = d_res[s].data_ptr(), d_res[s].data_ptr() + rxs[0].tb_stride * B
            if copy_in:
                t = pool.submit_host(h_iq.data_ptr(), 0, B, tb, rxs[0].tb_stride, ok, h_record=h_res[s].data_ptr())
            else:
                t = pool.submit(d_iq[s].data_ptr(), 0, B, tb, rxs[0].tb_stride, ok, h_record=h_res[s].data_ptr())
            assert t >= 0
            tickets[s] = t

        def step(k):
            if pool:
                return pool_step(k)
            s = k % n
            with torch.cuda.stream(tstreams[s]):
                if copy_in:
                    d_iq[s].copy_(h_iq, non_blocking=True)
                rc = L.srslte_hip_dl_rx_batch(rxs[s].h, d_iq[s].data_ptr(), 0, B, d_res[s].data_ptr(), rxs[s].tb_stride,
                                              d_res[s].data_ptr() + rxs[s].tb_stride * B, tstreams[s].cuda_stream)
                assert rc == 0
                h_res[s].copy_(d_res[s], non_blocking=True)
        def drain():
            for t in tickets:
                assert t < 0 or pool.wait(t) == 0
            torch.cuda.synchronize()
        tickets = [-1] * n
        for k in range(2 * n):
            step(k)
        drain()
        best = None
        for _ in range(5):
            t0 = time.perf_counter()
            for k in range(args.steps):
                step(k)
            drain()
            dt = (time.perf_counter() - t0) / args.steps
            best = dt if best is None else min(best, dt)
        return best
    t_res, t_pcie = run(False), run(True)
    ok = h_res[0][rxs[0].tb_stride * B:].numpy()
    out = {"workload": "cfg2: 128 x (100 PRB, 64QAM, TBS 75376), AWGN %.1f dB, %d streams" % (args.snr, n),
           "hbm_resident_subframes_per_s": round(B / t_res), "pcie_inclusive_subframes_per_s": round(B / t_pcie),
           "h2d_bytes_per_batch": int(h_iq.numel() * h_iq.element_size()),
           "h2d_GBps_at_that_rate": round(h_iq.numel() * h_iq.element_size() / t_pcie / 1e9, 1),
           "blocks_ok": int(ok.sum()), "_about": "scripts/pcie_inclusive.py: best of 5 runs of %d steps each" % args.steps}
    if sc16 or pool:  # the default invocation prints what it always did
        out["iq"], out["loop"] = args.iq, "pool_submit_host, one host thread" if pool else "one stream per step"
    print(json.dumps(out))
    if pool:
        pool.free()
    for r in rxs:
        r.free()


if __name__ == "__main__":
    main()
