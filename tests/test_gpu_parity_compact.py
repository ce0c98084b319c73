"""Punctured parity at a quarter of its rows (srslte_hip_dl_rx_parity_compact, phy_hip.h): the fixed-grant DL receive pipeline with the compact
soft-buffer layout against an object created with SRSLTE_HIP_PARITY_COMPACT=0 on the same IQ - transport blocks, CRC flags, per-block pass
counts and the soft buffer (debug view 5: always the whole layout) must be identical. The shapes are the smallest that take every path: the two
shortest block lengths of the 16-window decoder with K % 64 == 0 (Lw = K / 16 = 52: Lw % 8 == 4, and 56: Lw % 8 == 0) as single blocks, seven
blocks with gamma = 3 of the code-block split (sch.c:331-334) and a shadow slot, and the benchmark's own 100 PRB / MCS 28 - each over
subframes 0, 1 and 5 (three RE counts; a batch is consecutive TTIs). SNRs come from the CPU oracle's pass counts for these seeds; what they are chosen for is asserted."""
import importlib
import os

import numpy as np
import pytest

from lte_sim import DlConfig, make_subframe, oracle_rx

AMP = 0.1


@pytest.fixture(scope="module")
def hp():
    return importlib.import_module("srslte-emane_amd")


def _rx(hp, cfg, nsf, compact=True, llr8=False):
    """An object for cfg; compact=False: created with the switch off."""
    hc = hp.ChestDlCfg()
    hc.filter_coef[0], hc.filter_coef[1] = 4.0, 1.0
    old = os.environ.pop("SRSLTE_HIP_PARITY_COMPACT", None)
    try:
        if not compact:
            os.environ["SRSLTE_HIP_PARITY_COMPACT"] = "0"  # read when the object is created
        return hp.DlRx(cfg.cell_id, cfg.nof_prb, cfg.cfi, cfg.rnti, cfg.mod, cfg.tbs, 6, nsf, True, hc, llr_8bit=llr8, cp_ext=cfg.cp_ext)
    finally:
        os.environ.pop("SRSLTE_HIP_PARITY_COMPACT", None)
        if old is not None:
            os.environ["SRSLTE_HIP_PARITY_COMPACT"] = old


def _state(rx, cfg, nsf, llr8=False):
    """pass counts, block CRC flags and the soft buffer of the slots the last call used"""
    C_, K = cfg.seg.C, cfg.seg.K1
    stride = (3 * (K + 32) + 12 + 31) & ~31
    return (rx.debug(6, np.uint32, nsf * C_).reshape(nsf, C_), rx.debug(7, np.uint8, nsf * C_),
            rx.debug(5, np.int8 if llr8 else np.int16, nsf * C_ * stride))


def _same(a, b, what):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x, y), what


def _iq(cfg, snr, seed, ttis, rv=0, data=None):
    rng = np.random.default_rng(seed)
    out, dat = [], []
    for n, t in enumerate(ttis):
        x, d = make_subframe(cfg, t, rng, snr_db=snr, amp=AMP, rv=rv, data=None if data is None else data[n])
        out.append(x)
        dat.append(d)
    return np.stack(out), dat


# 6 PRB, extended CP, CFI 3, QPSK: 1104 bits in a normal subframe - below E_lim(832) = 1202 and E_lim(896) = 1294; subframes 5 and 0 carry 816
# and 288 bits, fewer than K: those blocks run all six passes and fail. 50 PRB, 64QAM, TBS 36992: C = 7 blocks of K = 5312 on 7080 / 7500 /
# 7356 RE, gamma = 3 / 3 / 6 (blocks 5, 6 get 6 LLRs more), at most 6432 LLRs per block, E_lim(5312) = 7641
SMALL = {"K832": (lambda: DlConfig(6, 7, 1, 808, cfi=3, cp_ext=True), 4.0, 1, 832),
         "K896": (lambda: DlConfig(6, 7, 1, 872, cfi=3, cp_ext=True), 6.0, 1, 896),
         "C7": (lambda: DlConfig(50, 7, 3, 36992, cfi=1), 18.0, 7, 5312),
         "bench": (lambda: DlConfig(100, 7, 3, 75376, cfi=1), 18.0, 13, 5824)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["K832", "K896", "C7"])
def test_compact_equals_whole_layout(hp, name):
    """One batch of TTIs 0 .. 5: subframes 0, 1 and 5 with their three RE counts; with C = 7 the pairs of blocks straddle subframes."""
    mk, snr, C_, K = SMALL[name]
    cfg = mk()
    assert (cfg.seg.C, cfg.seg.K1) == (C_, K) and K % 64 == 0
    nsf = 6
    iq, data = _iq(cfg, snr, 1, tuple(range(nsf)))
    on, off = _rx(hp, cfg, nsf), _rx(hp, cfg, nsf, compact=False)
    a, b = on.decode(iq, 0), off.decode(iq, 0)
    assert on.parity_compact() and not off.parity_compact()
    sa, sb = _state(on, cfg, nsf), _state(off, cfg, nsf)
    _same(a + sa, b + sb, name)
    its = sa[0].ravel()
    assert its.max() == 6, its  # a block that runs every pass
    if C_ > 1:  # the two blocks of a wavefront (launched blocks 2 i and 2 i + 1 of the batch) stop at different passes
        assert any(its[2 * i] != its[2 * i + 1] for i in range(len(its) // 2)), its
    else:  # an opinion from outside the library on the small shapes
        for t in range(nsf):
            r = oracle_rx(cfg, iq[t], t)
            assert bool(a[1][t]) == r["ok"] and np.array_equal(sa[0][t], r["iters"]), t
            if r["ok"]:
                assert np.array_equal(a[0][t], r["tb"]) and np.array_equal(a[0][t][:cfg.tbs // 8], data[t])
        assert a[1].any()
    on.free()
    off.free()


@pytest.mark.gpu
def test_compact_benchmark_geometry(hp):
    """100 PRB, MCS 28 (13 blocks of K = 5824) at batch 3: a batch is consecutive TTIs, so TTIs 4, 5, 6 and 9, 10, 11 in one call each cover
    subframes 0, 1 and 5."""
    mk, snr, C_, K = SMALL["bench"]
    cfg = mk()
    assert (cfg.seg.C, cfg.seg.K1) == (C_, K)
    on, off = _rx(hp, cfg, 3), _rx(hp, cfg, 3, compact=False)
    n_ok = 0
    for tti0 in (4, 9):
        ttis = (tti0, tti0 + 1, tti0 + 2)
        iq, _ = _iq(cfg, snr, 2 + tti0, ttis)
        a, b = on.decode(iq, tti0), off.decode(iq, tti0)
        assert on.parity_compact() and not off.parity_compact()
        _same(a + _state(on, cfg, 3), b + _state(off, cfg, 3), tti0)
        n_ok += int(a[1].sum())
    assert n_ok > 0
    on.free()
    off.free()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["n_e", "K", "llr8", "switch"])
def test_compact_is_off_where_it_does_not_apply(hp, case):
    """A grant whose blocks get more LLRs than the layout holds (6 PRB, normal CP, CFI 1: 1656 bits against E_lim(832) = 1202), a block length
    that is no multiple of 64 (K = 848), 8-bit LLRs, the switch: the whole layout, and the same results as an object with the switch off."""
    cfg = {"n_e": lambda: DlConfig(6, 7, 1, 808, cfi=1), "K": lambda: DlConfig(6, 7, 1, 824, cfi=3, cp_ext=True),
           "llr8": lambda: DlConfig(6, 7, 1, 808, cfi=3, cp_ext=True, llr8=True), "switch": lambda: DlConfig(6, 7, 1, 808, cfi=3, cp_ext=True)}[case]()
    llr8 = case == "llr8"
    assert cfg.seg.K1 == (848 if case == "K" else 832)
    iq, _ = _iq(cfg, 5.0, 3, (1,))
    a, b = _rx(hp, cfg, 1, compact=case != "switch", llr8=llr8), _rx(hp, cfg, 1, compact=False, llr8=llr8)
    ra, rb = a.decode(iq, 1), b.decode(iq, 1)
    assert not a.parity_compact() and not b.parity_compact()
    _same(ra + _state(a, cfg, 1, llr8), rb + _state(b, cfg, 1, llr8), case)
    if case == "switch":  # and the layout is on for this very configuration without it
        c = _rx(hp, cfg, 1)
        rc = c.decode(iq, 1)
        assert c.parity_compact()
        _same(rc + _state(c, cfg, 1), rb + _state(b, cfg, 1), case)
        c.free()
    a.free()
    b.free()


@pytest.mark.gpu
@pytest.mark.parametrize("name,snr", [("K832", 1.5), ("C7", 15.5)])
def test_compact_harq(hp, name, snr):
    """A compact first transmission that fails, rv 2 with new_data = 0 (the buffer is expanded in place, then combined), a new transport block
    on the same object (compact again), then rv 0, 2, 3, 1 of one more block: after every call everything equals the object without the
    layout. Calls 2 and 4 cover two of the three subframe slots: the expansion takes in a slot its call does not touch, and a compact call
    leaves the third slot as it was."""
    cfg = SMALL[name][0]()
    on, off = _rx(hp, cfg, 3), _rx(hp, cfg, 3, compact=False)
    first_fails = False
    n_after = 0
    seq = [(0, True, 3), (2, False, 2), (0, True, 3), (0, True, 2), (2, False, 3), (3, False, 3), (1, False, 3)]
    data = None
    for step, (rv, new, nsf) in enumerate(seq):
        ttis = tuple(4 + 10 * step + i for i in range(nsf))  # subframes 4, 5, 6
        iq, d = _iq(cfg, snr, 40 + step, ttis, rv=rv, data=None if new else data[:nsf])
        if new:
            data = d if nsf == 3 else d + data[nsf:]
        a, b = on.decode_harq(iq, ttis[0], rv, new), off.decode_harq(iq, ttis[0], rv, new)
        assert on.parity_compact() == (rv == 0 and new) and not off.parity_compact(), step
        if step == 0:
            first_fails = not a[1].any()
        n_after += int(a[1].sum()) if step else 0
        _same(a + _state(on, cfg, 3), b + _state(off, cfg, 3), (name, step))
    assert first_fails and n_after > 0  # the retransmissions did combine with what the compact call left
    on.free()
    off.free()


def _e_lim_36212(K):
    """36.212 5.1.4.1.1-2 for rv 0, written out: the first position of the circular buffer (NULLs skipped, from k0) whose parity bit sits in a row
    r = i % (K / 16) of the 16-window layout with r % 4 different from the row residue of that stream's first transmitted bit."""
    P = np.array([0, 16, 8, 24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30, 1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31])
    D = K + 4
    R = -(-D // 32)
    Kp, ND = 32 * R, 32 * R - D
    k = np.arange(Kp)
    y01 = 32 * (k % R) + P[k // R] - ND            # bit index of position k of the interleaved streams 0 and 1 (< 0: NULL)
    y2 = (P[k // R] + 32 * (k % R) + 1) % Kp - ND  # ... of stream 2
    stream = np.concatenate([np.zeros(Kp, int), np.tile([1, 2], Kp)])
    bit = np.concatenate([y01, np.stack([y01, y2], 1).ravel()])
    k0 = 2 * R  # R (2 ceil(Ncb / 8R) rv + 2), rv = 0
    order = (k0 + np.arange(3 * Kp)) % (3 * Kp)
    stream, bit = stream[order], bit[order]
    keep = bit >= 0
    stream, bit = stream[keep], bit[keep]
    row = bit % (K // 16)
    lim = len(bit)
    for s in (1, 2):
        m = (stream == s) & (bit < K)  # the four tail bits of a stream have their own slots
        phase = row[m][0] % 4
        bad = np.nonzero(m & (row % 4 != phase))[0]
        if len(bad):
            lim = min(lim, int(bad[0]))
    return lim


def test_e_lim_matches_36212():
    """every code-block length with K % 64 == 0 (36.212 Table 5.1.3-3), and none for the others"""
    hp = importlib.import_module("srslte-emane_amd")
    L = hp.lib()
    Ks = list(range(40, 512, 8)) + list(range(512, 1024, 16)) + list(range(1024, 2048, 32)) + list(range(2048, 6144 + 1, 64))
    assert len(Ks) == 188
    n = 0
    for K in Ks:
        got = L.srslte_hip_rm_parity_compact_limit(K)
        if K % 64:
            assert got == 0, K
        else:
            assert got == _e_lim_36212(K), K
            n += 1
    assert n > 60 and L.srslte_hip_rm_parity_compact_limit(5824) > 6930 and L.srslte_hip_rm_parity_compact_limit(44) == 0
