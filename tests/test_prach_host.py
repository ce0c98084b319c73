"""PRACH on the host (no GPU): the numerology and the FDD opportunity helper against the NumPy restatement (tests/prach_ref.py), the
restatement against the reference's own prach_test / prach_test_multi assertions, every refusal of create / gen / detect, and the kernels'
resources."""
import ctypes as C
import importlib
import os
import shutil

import numpy as np
import pytest

import prach_ref as R

pkg = importlib.import_module("srslte-emane_amd")


@pytest.mark.parametrize("nof_prb", [6, 25, 100])
def test_info_matches_the_restatement_for_every_configuration(nof_prb):
    for config_idx in range(64):
        for zczc in range(16):
            info = pkg.prach_cfg_info(pkg.prach_cfg(nof_prb, config_idx, root_seq_idx=(config_idx * 13) % 838, zero_corr_zone=zczc))
            assert info is not None
            p = R.Prach(nof_prb, config_idx, (config_idx * 13) % 838, zczc)
            got = (info.N_zc, info.N_cs, info.N_cp, info.N_seq, info.N_ifft_prach, info.N_ifft_ul, info.format, info.nof_roots, info.n_wins,
                   info.max_det, info.nof_sf)
            want = (p.N_zc, p.N_cs, p.N_cp, p.N_seq, p.N_ifft_prach, p.N_ifft_ul, p.f, p.N_roots, p.n_wins, p.max_det, p.nof_sf)
            assert got == want, (config_idx, zczc)
            assert list(info.root_seqs_idx[:info.nof_roots]) == p.root_seqs_idx
            assert pkg.prach_preamble_format(config_idx) == config_idx // 16


def test_max_det_exceeds_64_with_zero_corr_zone_2():
    info = pkg.prach_cfg_info(pkg.prach_cfg(100, 3, zero_corr_zone=2))
    assert (info.N_cs, info.n_wins, info.nof_roots, info.max_det) == (15, 55, 2, 110)


def test_nof_sf_per_format():
    assert [pkg.prach_cfg_info(pkg.prach_cfg(25, 16 * f)).nof_sf for f in range(4)] == [1, 2, 2, 3]


def test_tti_opportunity_matches_the_restatement():
    for config_idx in range(64):
        for tti in range(0, 10240, 7):
            for allowed in (-1, tti % 10, (tti + 1) % 10):
                assert pkg.prach_tti_opportunity_fdd(config_idx, tti, allowed) == R.tti_opportunity_fdd(config_idx, tti, allowed), \
                    (config_idx, tti, allowed)
    assert all(pkg.prach_tti_opportunity_fdd(14, t) for t in range(40))
    assert not any(pkg.prach_tti_opportunity_fdd(c, t) for c in (30, 46, 62) for t in range(40))
    assert pkg.prach_preamble_format(64) < 0


# the CTest matrix of prach_test (lib/src/phy/phch/test/CMakeLists.txt): one argument changed at a time from 50 PRB, config 3, root 0, zczc 15;
# "-f" sets config_idx, so formats 1-3 are added as 16 f + 3
PRACH_TEST = [dict()] + [dict(nof_prb=n) for n in (6, 15, 25, 50, 75, 100)] + [dict(config_idx=c) for c in (0, 1, 2, 3, 19, 35, 51)] + \
             [dict(root_seq_idx=r) for r in (0, 1, 2, 3)] + [dict(zero_corr_zone=z) for z in (0, 2, 3, 15)]


def _prach_test_cfg(kw):
    c = dict(nof_prb=50, config_idx=3, root_seq_idx=0, zero_corr_zone=15)
    c.update(kw)
    return c


@pytest.mark.parametrize("kw", PRACH_TEST, ids=[",".join("%s=%d" % i for i in k.items()) or "default" for k in PRACH_TEST])
def test_restatement_passes_prach_test(kw):
    c = _prach_test_cfg(kw)
    p = R.Prach(c["nof_prb"], c["config_idx"], c["root_seq_idx"], c["zero_corr_zone"])
    for s in range(64):
        x = p.gen(s, 0)
        idx, _, _ = p.detect_offset(0, x[p.N_cp:p.N_cp + p.N_seq])
        assert list(idx) == [s], (c, s, idx)


@pytest.mark.parametrize("n", [4, 8, 16, 32, 64])
def test_restatement_passes_prach_test_multi(n):
    p = R.Prach(6, 0, 0, 1, detect_factor=10.0)
    x = sum(p.gen(s, 0) for s in range(n))
    idx, _, _ = p.detect_offset(0, x[p.N_cp:])
    assert list(idx) == list(range(n))


def test_create_gen_and_detect_refuse_without_gpu():
    L = pkg.lib()
    for kw in (dict(hs_flag=True), dict(tdd=True), dict(detect_factor=-1.0), dict(detect_factor=float("nan")), dict(root_seq_idx=838),
               dict(zero_corr_zone=16)):
        cfg = pkg.prach_cfg(25, 3, **kw)
        assert L.srslte_hip_prach_create(C.byref(cfg)) is None, kw
        assert pkg.prach_cfg_info(cfg) is None, kw
    for nof_prb, config_idx in ((5, 3), (111, 3), (25, 64)):
        cfg = pkg.prach_cfg(nof_prb, config_idx)
        assert L.srslte_hip_prach_create(C.byref(cfg)) is None
        assert pkg.prach_cfg_info(cfg) is None
    assert L.srslte_hip_prach_create(None) is None
    assert L.srslte_hip_prach_cfg_info(None, None) == -2
    # the calls on a missing object
    assert L.srslte_hip_prach_gen_batch(None, None, 0, None, None) == -2
    assert L.srslte_hip_prach_detect_batch(None, None, 0, None, 0, None, None, None, None, None) == -2
    assert L.srslte_hip_prach_info(None, None) == -2
    L.srslte_hip_prach_destroy(None)
    # gen: seq_index >= 64, 6 + freq_offset > nof_prb, n > max_preambles
    cfg = pkg.prach_cfg(25, 3, max_preambles=2, max_occasions=2)

    def gen(*txs):
        arr = (pkg.PrachTx * max(1, len(txs)))(*[pkg.PrachTx(*t) for t in txs])
        return L.srslte_hip_prach_gen_check(C.byref(cfg), arr, len(txs))

    assert gen((63, 19), (0, 0)) == 0
    assert gen((64, 0)) == -2
    assert gen((0, 20)) == -2
    assert gen((0, 0), (1, 0), (2, 0)) == -2
    assert L.srslte_hip_prach_gen_check(C.byref(cfg), None, 1) == -2
    # detect: the window of N_ifft_prach samples past sig_len, freq_offset, n > max_occasions
    N = pkg.prach_cfg_info(cfg).N_ifft_prach

    def det(sig_len, *occ):
        arr = (pkg.PrachOccasion * max(1, len(occ)))(*[pkg.PrachOccasion(s, f, 0) for s, f in occ])
        return L.srslte_hip_prach_detect_check(C.byref(cfg), sig_len, arr, len(occ))

    assert det(N, (0, 0)) == 0
    assert det(2 * N, (N, 19), (3, 0)) == 0
    assert det(N - 1, (0, 0)) == -2
    assert det(2 * N, (N + 1, 0)) == -2
    assert det(N, (N + 5, 0)) == -2
    assert det(2 * N, (0, 20)) == -2
    assert det(4 * N, (0, 0), (0, 0), (0, 0)) == -2
    assert L.srslte_hip_prach_detect_check(C.byref(cfg), N, None, 1) == -2
    # also through the high-level checks of a refused configuration
    assert L.srslte_hip_prach_gen_check(C.byref(pkg.prach_cfg(25, 3, hs_flag=True)), None, 0) == -2


@pytest.mark.skipif(not os.path.exists(shutil.which("hipcc") or "/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_prach_kernels_use_no_scratch():
    from test_kernel_resources import _remarks
    kernels = _remarks("prach.hip")
    assert len(kernels) == 4, kernels
    for k, r in kernels.items():
        assert r.get("ScratchSize [bytes/lane]", 0) == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
