"""Batched PRACH on the device (srslte_hip_prach_gen_batch / _detect_batch) against the NumPy restatement (tests/prach_ref.py) and against
the reference's own prach.c as it runs when linked against this library (tests/prach_dropin_driver.c, compiled here with gcc against
oracle/_ref/hip/libsrslte_upper.a as oracle/ref_hip.mk links the reference's test programs)."""
import ctypes as C
import importlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

import prach_ref as R

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("srslte-emane_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_REF = os.path.join(ROOT, "oracle", "_ref", "hip")
CSRC = os.path.join(ROOT, "srslte-emane_amd", "csrc")
need_ref = pytest.mark.skipif(not os.path.exists(os.path.join(HIP_REF, "libsrslte_upper.a")),
                              reason="oracle/_ref/hip not built (needs /root/reference at build time)")


@pytest.fixture(scope="module")
def driver():
    d = tempfile.mkdtemp()
    exe = os.path.join(d, "prach_dropin_driver")
    subprocess.check_call(["gcc", "-std=c99", "-O2", os.path.join(ROOT, "tests", "prach_dropin_driver.c"), "-o", exe,
                           os.path.join(HIP_REF, "libsrslte_upper.a"), "-L" + CSRC, "-lsrslte_phy_hip", "-Wl,-rpath," + CSRC,
                           "-Wl,-rpath,/opt/rocm/lib", "-lstdc++", "-lm", "-lpthread"])

    class Drv:
        def gen(self, nof_prb, config_idx, rsi, zczc, txs, length):
            i, o = os.path.join(d, "g.in"), os.path.join(d, "g.out")
            with open(i, "wb") as f:
                f.write(np.array([len(txs)] + [v for t in txs for v in t], np.uint32).tobytes())
            subprocess.check_call([exe, "gen", str(nof_prb), str(config_idx), str(rsi), str(zczc), i, o], timeout=300)
            return np.fromfile(o, np.complex64).reshape(len(txs), length)

        def detect(self, nof_prb, config_idx, rsi, zczc, factor, occs):
            """occs [(freq_offset, signal)] -> [(indices, t_offsets, peak_to_avg)]"""
            i, o = os.path.join(d, "d.in"), os.path.join(d, "d.out")
            with open(i, "wb") as f:
                f.write(np.uint32(len(occs)).tobytes())
                for fo, s in occs:
                    f.write(np.array([fo, len(s)], np.uint32).tobytes() + np.asarray(s, np.complex64).tobytes())
            subprocess.check_call([exe, "detect", str(nof_prb), str(config_idx), str(rsi), str(zczc), repr(float(factor)), i, o], timeout=300)
            raw, out, p = open(o, "rb").read(), [], 0
            for _ in occs:
                n = int(np.frombuffer(raw, np.uint32, 1, p)[0])
                rec = np.frombuffer(raw, np.uint32, 3 * n, p + 4).reshape(n, 3)
                out.append((rec[:, 0].copy(), rec[:, 1].copy().view(np.float32), rec[:, 2].copy().view(np.float32)))
                p += 4 + 12 * n
            return out

        def opportunities(self):
            o = os.path.join(d, "o.out")
            subprocess.check_call([exe, "opp", "6", "0", "0", "0", o], timeout=60)
            return np.fromfile(o, np.uint8).reshape(64, 20, 11)

    return Drv()


def _fo(s, nof_prb):
    return (7 * s) % (nof_prb - 5)


GEN_CASES = [(n, 3) for n in (6, 15, 25, 50, 75, 100)] + [(n, c) for n in (25, 100) for c in (19, 35, 51)] + [(15, 63)]


@pytest.mark.parametrize("nof_prb,config_idx", GEN_CASES)
def test_generator_matches_the_restatement(nof_prb, config_idx):
    rsi, zczc = (config_idx * 5) % 838, (nof_prb + config_idx) % 16
    dev = pkg.Prach(nof_prb, config_idx, max_preambles=64, root_seq_idx=rsi, zero_corr_zone=zczc)
    ref = R.Prach(nof_prb, config_idx, rsi, zczc)
    rc, out = dev.gen([(s, _fo(s, nof_prb)) for s in range(64)])
    assert rc == 0 and out.shape == (64, ref.N_cp + ref.N_seq)
    for s in range(64):
        want = ref.gen(s, _fo(s, nof_prb))
        assert np.max(np.abs(out[s] - want)) <= 1e-4 * np.max(np.abs(want)), s
    dev.free()


@need_ref
@pytest.mark.parametrize("nof_prb,config_idx", [(6, 3), (25, 19), (50, 35), (100, 51), (100, 3)])
def test_generator_matches_the_reference(driver, nof_prb, config_idx):
    rsi, zczc = 11 * config_idx % 838, 1 + config_idx % 15
    dev = pkg.Prach(nof_prb, config_idx, max_preambles=64, root_seq_idx=rsi, zero_corr_zone=zczc)
    txs = [(s, _fo(s, nof_prb)) for s in range(64)]
    rc, out = dev.gen(txs)
    want = driver.gen(nof_prb, config_idx, rsi, zczc, txs, dev.len)
    assert rc == 0
    for s in range(64):
        assert np.max(np.abs(out[s] - want[s])) <= 1e-4 * np.max(np.abs(want[s])), s
    dev.free()


@need_ref
def test_opportunities_match_the_reference(driver):
    o = driver.opportunities()
    for c in range(64):
        for t in range(20):
            for a in range(-1, 10):
                assert pkg.prach_tti_opportunity_fdd(c, t, a) == bool(o[c, t, a + 1]), (c, t, a)


def _one_buffer(signals, gap=37):
    """signals laid out one after the other with gaps -> (buffer, start of each)"""
    starts, p = [], 11
    for s in signals:
        starts.append(p)
        p += len(s) + gap
    buf = np.zeros(p, np.complex64)
    for st, s in zip(starts, signals):
        buf[st:st + len(s)] = s
    return buf, starts


PRACH_TEST = [dict()] + [dict(nof_prb=n) for n in (6, 15, 25, 50, 75, 100)] + [dict(config_idx=c) for c in (0, 1, 2, 3, 19, 35, 51)] + \
             [dict(root_seq_idx=r) for r in (0, 1, 2, 3)] + [dict(zero_corr_zone=z) for z in (0, 2, 3, 15)]


@pytest.mark.parametrize("kw", PRACH_TEST, ids=[",".join("%s=%d" % i for i in k.items()) or "default" for k in PRACH_TEST])
def test_prach_test_matrix_on_the_device(kw):
    """prach_test: each of the 64 preambles, generated on the device, detected alone (its N_seq samples after the CP) with its own index."""
    c = dict(nof_prb=50, config_idx=3, root_seq_idx=0, zero_corr_zone=15)
    c.update(kw)
    dev = pkg.Prach(c["nof_prb"], c["config_idx"], max_occasions=64, max_preambles=64, root_seq_idx=c["root_seq_idx"],
                    zero_corr_zone=c["zero_corr_zone"])
    rc, pre = dev.gen([(s, 0) for s in range(64)])
    assert rc == 0
    i = dev.info
    buf, starts = _one_buffer([p[i.N_cp:i.N_cp + i.N_seq] for p in pre])
    rc, res = dev.detect(buf, [(st, 0) for st in starts])
    assert rc == 0
    assert [list(r[0]) for r in res] == [[s] for s in range(64)]
    dev.free()


@pytest.mark.parametrize("n", [4, 8, 16, 32, 64])
def test_prach_test_multi_on_the_device(n):
    """prach_test_multi: the sum of preambles 0 .. n-1 at factor 10 (6 PRB, config 0, zczc 1) gives exactly 0 .. n-1."""
    dev = pkg.Prach(6, 0, max_occasions=1, max_preambles=64, zero_corr_zone=1, detect_factor=10.0)
    rc, pre = dev.gen([(s, 0) for s in range(n)])
    x = pre.sum(axis=0)
    rc, res = dev.detect(x[dev.info.N_cp:], [(0, 0)])
    assert rc == 0 and list(res[0][0]) == list(range(n))
    dev.free()


def _stimulus(ref, rng, seqs, fo, snr_db, extra=0, advance=0):
    """preambles seqs (generated by the restatement) at integer delays whose correlation lag is close to an integer, in seeded AWGN ->
    (the samples from the first one after the CP on - or `advance` samples later: preambles that arrived early -, the delays)"""
    N, L = ref.N_ifft_prach, ref.N_cp + ref.N_seq
    win = ref.N_cs if ref.N_cs else R.NZC
    max_d = max(1, (min(win, 60) - 3) * N // R.NZC)
    sig = np.zeros(L + max_d + extra + advance, complex)
    delays = []
    for s in seqs:
        while True:
            d = int(rng.integers(0, max_d))
            frac = (d * R.NZC / N) % 1.0
            if frac < 0.25 or frac > 0.75:
                break
        delays.append(d)
        sig[d:d + L] += ref.gen(s, fo) * rng.uniform(0.7, 1.3)
    p = R.NZC / N
    sig += np.sqrt(p / 10 ** (snr_db / 10) / 2) * (rng.standard_normal(len(sig)) + 1j * rng.standard_normal(len(sig)))
    return sig[ref.N_cp + advance:].astype(np.complex64), delays


def _advance(ref, lag):
    """a whole number of samples that moves the correlation peaks by close to `lag` bins"""
    return int(round(lag * ref.N_ifft_prach / R.NZC))


DETECT_CASES = [(100, 3, 1, 18.0, 17), (25, 19, 0, 18.0, 3), (50, 35, 2, 18.0, 200), (6, 51, 15, 18.0, 5), (100, 3, 2, 60.0, 837),
                (75, 20, 7, 18.0, 64)]


@need_ref
@pytest.mark.parametrize("nof_prb,config_idx,zczc,factor,rsi", DETECT_CASES)
def test_detection_matches_the_reference(driver, nof_prb, config_idx, zczc, factor, rsi):
    rng = np.random.default_rng(nof_prb * 1000 + config_idx * 10 + zczc)
    ref = R.Prach(nof_prb, config_idx, rsi, zczc, factor)
    occs, sigs = [], []
    for o in range(4):
        fo = int(rng.integers(0, nof_prb - 5))
        seqs = [int(x) for x in rng.choice(64, size=1 + o, replace=False)]
        adv = 0
        if zczc == 2 and o == 3:
            # preambles 63 and 53 arriving about 20 bins early (N_cs 15): one window on, indices >= 64 and 54
            seqs, adv = [63, 53], _advance(ref, 20)
        s, _ = _stimulus(ref, rng, seqs, fo, snr_db=[10.0, 0.0, -5.0, 5.0][o], extra=64 * o, advance=adv)
        occs.append(fo)
        sigs.append(s)
    dev = pkg.Prach(nof_prb, config_idx, max_occasions=4, root_seq_idx=rsi, zero_corr_zone=zczc, detect_factor=factor)
    buf, starts = _one_buffer(sigs)
    rc, got = dev.detect(buf, [(st, fo) for st, fo in zip(starts, occs)])
    assert rc == 0
    want = driver.detect(nof_prb, config_idx, rsi, zczc, factor, list(zip(occs, sigs)))
    seen = 0
    for o in range(4):
        gi, gt, gp = got[o]
        wi, wt, wp = want[o]
        assert list(gi) == list(wi), (o, gi, wi)
        assert np.array_equal(gt, wt), (o, gt, wt)
        assert np.allclose(gp, wp, rtol=1e-3, atol=0), (o, gp, wp)
        ri, rt, rp = ref.detect_offset(occs[o], sigs[o])
        assert list(ri) == list(gi) and np.array_equal(rt, gt) and np.allclose(rp, gp, rtol=1e-3)
        seen += len(gi)
    assert seen >= 4
    if zczc == 2:
        assert dev.info.max_det == 110 and any(i >= 64 for i in got[3][0])
    dev.free()


def test_indices_of_64_and_above_are_reported():
    """zero_corr_zone 2: 55 windows x 2 roots; preamble 63 (root 1, v = 8) arriving 20 bins (> N_cs = 15) early lands in window 10 of root 1,
    index 65, beyond the 64 preambles a UE sends: reported as the reference reports it."""
    ref = R.Prach(100, 3, 0, 2)
    a = _advance(ref, 20)
    x = np.concatenate([ref.gen(63, 0), np.zeros(a)])
    sig = x[ref.N_cp + a:].astype(np.complex64)
    want = ref.detect_offset(0, sig)
    assert any(i >= 64 for i in want[0])
    dev = pkg.Prach(100, 3, zero_corr_zone=2)
    rc, got = dev.detect(sig, [(0, 0)])
    assert rc == 0 and list(got[0][0]) == list(want[0])
    assert np.array_equal(got[0][1], want[1]) and np.allclose(got[0][2], want[2], rtol=1e-3)
    dev.free()


def test_a_batch_equals_one_call_per_occasion():
    rng = np.random.default_rng(7)
    ref = R.Prach(50, 19, 123, 4)
    sigs, fos = [], []
    for o in range(9):
        fo = int(rng.integers(0, 45))
        s, _ = _stimulus(ref, rng, [int(x) for x in rng.choice(64, 3, replace=False)], fo, 3.0)
        sigs.append(s)
        fos.append(fo)
    buf, starts = _one_buffer(sigs, gap=int(rng.integers(1, 500)))
    dev = pkg.Prach(50, 19, max_occasions=9, root_seq_idx=123, zero_corr_zone=4)
    rc, batch = dev.detect(buf, [(st, fo) for st, fo in zip(starts, fos)])
    assert rc == 0
    d_buf = pkg.DevBuf.from_host(buf)
    for o in range(9):
        rc, one = dev.detect(None, [(starts[o], fos[o])], d_signal=d_buf.ptr, sig_len=len(buf))
        assert rc == 0
        for a, b in zip(batch[o], one[0]):
            assert np.array_equal(a, b), o
        assert len(batch[o][0]) == 3
    # an occasion whose window runs past the signal is refused, nothing queued
    rc, _ = dev.detect(buf, [(len(buf) - dev.info.N_ifft_prach + 1, 0)])
    assert rc == -2
    rc, _ = dev.gen([(0, 0)] * 2)
    assert rc == -2  # max_preambles 1
    dev.free()


def test_two_objects_on_two_streams():
    L = pkg.lib()
    rng = np.random.default_rng(3)
    cfgs = [(100, 3, 1), (25, 35, 0)]
    objs, bufs, occs, solo = [], [], [], []
    for nof_prb, ci, z in cfgs:
        ref = R.Prach(nof_prb, ci, 0, z)
        sigs = [_stimulus(ref, rng, [int(x) for x in rng.choice(64, 2, replace=False)], 0, 5.0)[0] for _ in range(16)]
        buf, starts = _one_buffer(sigs)
        dev = pkg.Prach(nof_prb, ci, max_occasions=16, max_preambles=64, zero_corr_zone=z)
        objs.append(dev)
        bufs.append(buf)
        occs.append([(st, 0) for st in starts])
        solo.append(dev.detect(buf, occs[-1])[1])
    streams = [L.srslte_hip_stream_create() for _ in objs]
    outs = []
    for dev, buf, oc, st in zip(objs, bufs, occs, streams):
        md, n = dev.info.max_det, len(oc)
        b = dict(sig=pkg.DevBuf.from_host(buf), n=pkg.DevBuf(4 * n), i=pkg.DevBuf(4 * md * n), t=pkg.DevBuf(4 * md * n), p=pkg.DevBuf(4 * md * n),
                 g=pkg.DevBuf(8 * dev.len * 64))
        outs.append(b)
    for _ in range(3):
        for dev, buf, oc, st, b in zip(objs, bufs, occs, streams, outs):
            assert dev.gen_device([pkg.PrachTx(s, 0) for s in range(64)], b["g"].ptr, st) == 0
            occ = [pkg.PrachOccasion(s, f, 0) for s, f in oc]
            assert dev.detect_device(b["sig"].ptr, len(buf), occ, b["n"].ptr, b["i"].ptr, b["t"].ptr, b["p"].ptr, st) == 0
    for st in streams:
        assert L.srslte_hip_stream_sync(st) == 0
    for dev, b, want in zip(objs, outs, solo):
        md = dev.info.max_det
        nof = b["n"].to_host(np.uint32)
        idx, tof = b["i"].to_host(np.uint32).reshape(-1, md), b["t"].to_host(np.float32).reshape(-1, md)
        for o, (wi, wt, _) in enumerate(want):
            assert nof[o] == len(wi) and np.array_equal(idx[o, :nof[o]], wi) and np.array_equal(tof[o, :nof[o]], wt)
        rc, g1 = dev.gen([(s, 0) for s in range(64)]) if dev.cfg.max_preambles >= 64 else (0, None)
        assert np.array_equal(b["g"].to_host(np.complex64).reshape(64, -1), g1)
    for st in streams:
        L.srslte_hip_stream_destroy(st)
    for dev in objs:
        dev.free()


def test_preambles_in_the_uplink_buffer_the_grants_receiver_decodes():
    """A run of 10 consecutive UL subframes from srslte_hip_ul_tx_batch_grants (one PUSCH per subframe on PRBs 10-19 of a 25-PRB cell) with
    preambles added at the FDD opportunities of config_idx 6 (subframes 1 and 6) on PRBs 2-7: every transport block decodes through
    srslte_hip_ul_rx_batch_grants, and srslte_hip_prach_detect_batch on the same device buffer at factor 60 finds exactly the preambles sent."""
    prb, nsf, tti0, cfg_idx, fo = 25, 10, 20, 6, 2
    rng = np.random.default_rng(11)
    grants, datas = [], []
    for b in range(nsf):
        grants.append(pkg.UlGrant.make(b, 0x400, 10, 10, 1, 1544, n_dmrs=b % 8))
        datas.append(rng.integers(0, 256, 1544 // 8, dtype=np.uint8))
    tx = pkg.UlTx(4, prb, 0x1234, 1, 1544, 10, 10, 0, nsf, max_grants=nsf)
    iq = np.ascontiguousarray(tx.encode_grants(datas, tti0, nsf, grants), np.complex64).reshape(nsf, -1)
    tx.free()
    sf_len = iq.shape[1]
    dev = pkg.Prach(prb, cfg_idx, max_occasions=nsf, max_preambles=8, zero_corr_zone=5, detect_factor=60.0)
    opp = [b for b in range(nsf) if pkg.prach_tti_opportunity_fdd(cfg_idx, tti0 + b)]
    assert opp == [1, 6]
    sent = {1: [5, 40], 6: [17]}
    rc, pre = dev.gen([(s, fo) for b in opp for s in sent[b]])
    assert rc == 0
    flat = iq.reshape(-1).copy()
    rms = np.sqrt(np.mean(np.abs(flat) ** 2))
    k = 0
    for b in opp:
        for _ in sent[b]:
            p = pre[k] * (rms / np.sqrt(np.mean(np.abs(pre[k]) ** 2)))
            flat[b * sf_len:b * sf_len + len(p)] += p
            k += 1
    rx = pkg.UlRx(4, prb, 0x1234, 1, 1544, 10, 10, 0, 6, nsf, max_grants=nsf)
    d_iq = pkg.DevBuf.from_host(flat)
    tb, ok = rx.decode_grants(flat.reshape(nsf, sf_len), tti0, grants)
    assert ok.all()
    for p in range(nsf):
        assert np.array_equal(tb[p][:1544 // 8], datas[p]), p
    rx.free()
    rc, res = dev.detect(None, [(b * sf_len + dev.info.N_cp, fo) for b in opp], d_signal=d_iq.ptr, sig_len=flat.size)
    assert rc == 0
    for b, r in zip(opp, res):
        assert sorted(r[0].tolist()) == sorted(sent[b]), (b, r)
    dev.free()
