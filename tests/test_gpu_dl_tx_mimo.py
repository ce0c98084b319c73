"""TM3 / TM4 on the transmit side (srslte_hip_dl_tx_batch_grants2): two codewords, large-delay CDD and codebook precoding on a 2-port cell.

The grids against the oracle's stimulus generator run once per PDSCH (make_subframe_mimo: orc_precoding_cdd2 / orc_precoding_mux2) and
against the reference's own srslte_pdsch_encode; single-codeword batches against srslte_hip_dl_tx_batch_grants byte for byte; a round trip
through srslte_hip_dl_rx_batch_grants2, noise free and with noise; the CSI closed loop with the downlink made on the device; shapes and
refusals.

Bounds: those of tests/test_gpu_dl_tx_grants.py::test_dl_tx_grants_vs_oracle - grids 3e-7 x max(1, rho_a), time samples 1e-4 of the oracle's
peak. The kernel's arithmetic is the reference's operation by operation (levels from the same table, one IEEE-754 single-precision add and
one multiply per component, no contraction), so test_grids_equal_the_oracle_bit_for_bit also asks for equal values."""
import ctypes as C
import importlib

import numpy as np
import pytest

from _libs import OrcOfdm, oracle, p, ref
from test_gpu_dl_tx_grants import _mask, _ue_sets

pytestmark = pytest.mark.gpu
SCHEME = {"div": 1, "cdd": 3, "mux": 2}


@pytest.fixture(scope="module")
def hp():
    return importlib.import_module("srslte-emane_amd")


def _chest(hp):
    hc = hp.ChestDlCfg()
    hc.filter_coef[0], hc.filter_coef[1] = 4.0, 1.0
    return hc


def _grant2(hp, prb, kind, mask, rnti, mod, tbs, rv=0, mod2=0, tbs2=0, rv2=0, pmi=0, cfi=1):
    return hp.DlGrant2(hp.DlGrant.make(prb, mod, tbs, rnti, cfi=cfi, rv=rv, prb_mask=mask), SCHEME[kind], pmi, mod2, tbs2, rv2, 1)


# (kind, mask, mod, tbs, rv, mod2, tbs2, rv2, pmi) per UE, a list per subframe
def _sets(prb):
    if prb == 25:
        return [
            [("cdd", _mask(25, [(0, 25)]), 2, 4008, 0, 4, 7992, 0, 0)],
            [("div", _mask(25, [(0, 8)]), 2, 2216, 0, 0, 0, 0, 0), ("cdd", _mask(25, [(8, 17)]), 1, 1000, 1, 2, 2216, 2, 0),
             ("mux", _mask(25, [(17, 25)]), 3, 4008, 3, 1, 776, 0, 1)],
            [("mux", _mask(25, [(0, 6)]), 2, 1544, 0, 0, 0, 0, 0), ("mux", _mask(25, [(6, 12)]), 2, 1544, 1, 0, 0, 0, 1),       # sf_idx 0: centre PRBs lose REs
             ("mux", _mask(25, [(12, 19)]), 2, 1544, 2, 0, 0, 0, 2), ("mux", _mask(25, [(19, 25)]), 2, 1544, 3, 0, 0, 0, 3)],
            [("mux", _mask(25, [(0, 25)]), 4, 7992, 2, 2, 4008, 3, 0)],
            [],                                                                                                            # an empty subframe: CRS only
            [("cdd", _mask(25, [(2, 10)], [(14, 20)]), 2, 2216, 0, 1, 776, 1, 0), ("mux", _mask(25, [(14, 20)], [(2, 10)]), 1, 1000, 2, 2, 1544, 0, 1),
             ("div", _mask(25, [(0, 2), (10, 14), (20, 23)]), 1, 776, 1, 0, 0, 0, 0)],
        ]
    return [
        [("cdd", _mask(100, [(0, 50)]), 3, 30576, 0, 4, 30576, 2, 0), ("mux", _mask(100, [(50, 100)]), 2, 15264, 1, 3, 22152, 0, 0)],
        [("mux", _mask(100, [(0, 100)]), 3, 75376, 0, 0, 0, 0, 2)],
        [("div", _mask(100, [(0, 4), (40, 60), (90, 100)]), 2, 9144, 2, 0, 0, 0, 0), ("cdd", _mask(100, [(4, 40)]), 4, 30576, 0, 1, 4584, 3, 0),
         ("mux", _mask(100, [(60, 90)]), 1, 4584, 1, 0, 0, 0, 3)],
    ]


def _expected(hp, prb, cid, tti0, p_a, sets, rng):
    """The oracle's grids [nsf][2][14 * 12 * prb] (CRS once, every PDSCH's y on its idx), the grants and the payloads."""
    from lte_sim import DlConfig, make_subframe, make_subframe_mimo
    nsf = len(sets)
    grants, datas, exp = [], [], np.zeros((nsf, 2, 14 * 12 * prb), np.complex64)
    for b, lst in enumerate(sets):
        for port in range(2):
            oracle().orc_crs_put_sf(C.byref(DlConfig(prb, cid, 1, 1000, nof_ports=2).cell), (tti0 + b) % 10, port, p(exp[b, port]))
        for u, (kind, mask, mod, tbs, rv, mod2, tbs2, rv2, pmi) in enumerate(lst):
            rnti, k = 0x200 + 8 * b + u, {}
            if kind == "div":
                cfg = DlConfig(prb, cid, mod, tbs, nof_ports=2, p_a=p_a, rnti=rnti, prb_mask=mask)
                assert len(cfg.indices((tti0 + b) % 10)) % 2 == 0
                _, data = make_subframe(cfg, tti0 + b, rng, rv=rv, keep=k)
                data = [data]
            else:
                cfg = DlConfig(prb, cid, mod, tbs, nof_rx=2, nof_ports=2, p_a=p_a, rnti=rnti, prb_mask=mask, tx_scheme=kind, pmi=pmi, mod2=mod2 or None, tbs2=tbs2)
                _, data = make_subframe_mimo(cfg, tti0 + b, rng, rv=(rv, rv2), keep=k)
            for port in range(2):
                exp[b, port][k["idx"]] = k["y"][port]
            grants.append((b, _grant2(hp, prb, kind, mask, rnti, mod, tbs, rv, mod2, tbs2, rv2, pmi)))
            datas.append(data)
    return grants, datas, exp


@pytest.mark.parametrize("prb,tti0,p_a", [(25, 8, 0.0), (25, 8, -3.0), (100, 4, 0.0), (100, 4, -3.0)])
def test_dl_tx_grants2_vs_oracle(hp, prb, tti0, p_a):
    """Every port's grid and time samples for CDD, multiplexing with two blocks (pmi 0, 1) and one block (pmi 0-3), transmit diversity beside
    them in the same subframes, different modulations on the two codewords (256QAM on one), every redundancy version on either block."""
    rng = np.random.default_rng(7100 + prb)
    sets = _sets(prb)
    nsf = len(sets)
    grants, datas, exp = _expected(hp, prb, 7, tti0, p_a, sets, rng)
    tbs_max = max(max(g.tb0.tbs, g.tbs2) for _, g in grants)
    tx = hp.DlTx(7, prb, 1, 0x1234, 1, tbs_max, nsf, 2, p_a, max_grants=len(grants))
    rc, iq = tx.encode_grants2(datas, tti0, nsf, grants)
    assert rc == 0
    grid = tx.debug(3, np.complex64, nsf * 2 * 14 * 12 * prb).reshape(nsf, 2, -1)
    q = OrcOfdm()
    oracle().orc_ofdm_init(C.byref(q), prb, True)
    q.normalize = True
    scale = max(1.0, 10 ** (p_a / 20) * 2 ** 0.5)
    worst = 0.0
    for b in range(nsf):
        for port in range(2):
            worst = max(worst, float(np.abs(grid[b, port] - exp[b, port]).max()))
            assert np.abs(grid[b, port] - exp[b, port]).max() <= 3e-7 * scale, (b, port)
            iq_o = np.zeros(15 * q.symbol_sz, np.complex64)
            oracle().orc_ofdm_tx_sf(C.byref(q), p(np.ascontiguousarray(exp[b, port])), p(iq_o))
            assert np.abs(iq[b, port] - iq_o).max() <= 1e-4 * max(np.abs(iq_o).max(), 1e-9), (b, port)
    print("grants2 vs oracle: prb %d p_a %g: largest grid difference %.3g" % (prb, p_a, worst))
    tx.free()


def test_grids_equal_the_oracle_bit_for_bit(hp):
    """The same operations on the same table values in the same order: the grids are the oracle's, value for value (a gain folded into the
    levels before the add, a fused multiply-add or another order would move last bits)."""
    prb, tti0, p_a = 25, 8, -3.0
    sets = _sets(prb)
    grants, datas, exp = _expected(hp, prb, 7, tti0, p_a, sets, np.random.default_rng(7200))
    tx = hp.DlTx(7, prb, 1, 0x1234, 1, 7992, len(sets), 2, p_a, max_grants=len(grants))
    rc, _ = tx.encode_grants2(datas, tti0, len(sets), grants)
    assert rc == 0
    grid = tx.debug(3, np.complex64, len(sets) * 2 * 14 * 12 * prb).reshape(len(sets), 2, -1)
    for b, lst in enumerate(sets):
        if any(kind != "div" for kind, *_ in lst):
            assert np.array_equal(grid[b], exp[b]), (b, float(np.abs(grid[b] - exp[b]).max()))
    tx.free()


@pytest.mark.skipif(ref() is None, reason="oracle/_ref/libsrslte_ref.so is not built")
@pytest.mark.parametrize("prb,kind,pmi,two", [(25, "cdd", 0, True), (25, "mux", 0, True), (25, "mux", 1, True), (25, "mux", 0, False), (25, "mux", 1, False),
                                              (25, "mux", 2, False), (25, "mux", 3, False), (100, "cdd", 0, True), (100, "mux", 1, True), (100, "mux", 2, False)])
def test_dl_tx_grants2_vs_reference_pdsch_encode(hp, prb, kind, pmi, two):
    """Full band, rv 0: the PDSCH REs of both ports against the reference's own srslte_pdsch_encode (p_a = 0: rho_a = sqrt(2))."""
    from lte_sim import DlConfig, RefPdschTx
    rng = np.random.default_rng(7300 + prb + pmi)
    mod, tbs, mod2, tbs2 = (2, 4008, 3, 6200) if prb == 25 else (3, 30576, 2, 15264)
    cfg = DlConfig(prb, 11, mod, tbs, nof_rx=2, nof_ports=2, p_a=0.0, tx_scheme=kind, pmi=pmi, mod2=mod2 if two else None, tbs2=tbs2 if two else 0)
    r = RefPdschTx(cfg)
    tx = hp.DlTx(11, prb, 1, 0x1234, 1, max(tbs, tbs2), 3, 2, 0.0, max_grants=3)
    ttis = (0, 3, 5)
    datas = [[rng.integers(0, 256, t // 8, dtype=np.uint8) for t in cfg.tbss] for _ in ttis]
    for j, tti in enumerate(ttis):  # one call per subframe index: sync subframes among them
        g = _grant2(hp, prb, kind, None, cfg.rnti, mod, tbs, 0, mod2 if two else 0, tbs2 if two else 0, 0, pmi)
        rc, _ = tx.encode_grants2([datas[j]], tti, 1, [(0, g)])
        assert rc == 0
        grid = tx.debug(3, np.complex64, 2 * 14 * 12 * prb).reshape(2, -1)
        want = r.run_mimo(datas[j], tti)
        idx = cfg.indices(tti % 10)
        for port in range(2):
            assert np.abs(grid[port][idx] - want[port][idx]).max() <= 3e-7 * 2 ** 0.5, (tti, port)
    tx.free()


@pytest.mark.parametrize("npt", [1, 2])
def test_grants2_without_second_codeword_is_grants(hp, npt):
    """Entries of scheme 0 / 1 with tbs2 = 0: the time samples of srslte_hip_dl_tx_batch_grants with the same grants, byte for byte."""
    prb, tti0 = 25, 8
    rng = np.random.default_rng(7400 + npt)
    grants, datas = [], []
    for b, lst in enumerate(_ue_sets(prb)):
        for u, (mask, mod, tbs, rv) in enumerate(lst):
            grants.append((b, hp.DlGrant.make(prb, mod, tbs, 0x200 + 8 * b + u, cfi=1, rv=rv, prb_mask=mask)))
            datas.append(rng.integers(0, 256, tbs // 8, dtype=np.uint8))
    nsf = len(_ue_sets(prb))
    a, b_ = (hp.DlTx(7, prb, 1, 0x1234, 1, 7992, nsf, npt, -3.0 if npt == 2 else 0.0, max_grants=len(grants)) for _ in range(2))
    iq1 = a.encode_grants(datas, tti0, nsf, grants).copy()
    rc, iq2 = b_.encode_grants2([[d] for d in datas], tti0, nsf, [(sf, hp.DlGrant2(g, 1 if npt == 2 else 0, 0, 0, 0, 0, 0)) for sf, g in grants])
    assert rc == 0 and iq1.tobytes() == iq2.tobytes()
    a.free()
    b_.free()


def _mix(iq, H):
    """[nsf][2 ports][n] -> [nsf][2 antennas][n] through the flat 2x2 channel H[antenna][port]."""
    return np.stack([H[a][0] * iq[:, 0, :] + H[a][1] * iq[:, 1, :] for a in range(2)], axis=1).astype(np.complex64)


def test_grants2_round_trip_through_rx_grants2(hp):
    """100 PRB, 32 subframes, three UEs a subframe whose schemes rotate (CDD, two-block and one-block multiplexing, transmit diversity): one
    transmit call; a fixed well-conditioned 2x2 mixing of the two port signals into two antennas; each UE's srslte_hip_dl_rx_batch_grants2
    returns every transport block of both codewords, noise free. Then white noise from a kept seed at an SNR at which the oracle's chain
    decodes every block of the same samples (checked in the test): the device delivers every block too."""
    from lte_sim import DlConfig, oracle_rx, oracle_rx_mimo
    prb, nsf, tti0, cid, cfi = 100, 32, 6, 9, 2
    rng = np.random.default_rng(7500)
    # (PRBs, kind, mod, tbs, mod2, tbs2)
    shapes = [((0, 30), "cdd", 2, 9144, 2, 9144), ((30, 70), "mux", 3, 15264, 2, 9144), ((70, 100), "mux1", 1, 4584, 0, 0), ((70, 100), "div", 1, 4584, 0, 0)]
    grants, datas, per_ue = [], [], [[], [], []]
    for b in range(nsf):
        for u in range(3):
            (a, z), kind, mod, tbs, mod2, tbs2 = shapes[(u + b) % 3 if (u + b) % 3 < 2 else 2 + (b // 3) % 2]
            mask = _mask(prb, [(a, z)])
            pmi = (b % 2) if kind == "mux" else ((b % 4) if kind == "mux1" else 0)
            g = _grant2(hp, prb, "mux" if kind == "mux1" else kind, mask, 0x300 + u, mod, tbs, 0, mod2, tbs2, 0, pmi, cfi=cfi)
            d = [rng.integers(0, 256, t // 8, dtype=np.uint8) for t in ([tbs, tbs2] if tbs2 else [tbs])]
            grants.append((b, g))
            datas.append(d)
            per_ue[u].append((g, d, kind, mask, pmi))
    tx = hp.DlTx(cid, prb, cfi, 0x1234, 1, 15264, nsf, 2, 0.0, max_grants=len(grants))
    rc, iq = tx.encode_grants2(datas, tti0, nsf, grants)
    assert rc == 0
    tx.free()
    H = [[1.0, 0.35j], [0.3, 0.9 * np.exp(0.8j)]]
    clean = _mix(iq, H)
    snr_db, seed = 30.0, 7501
    sigma = np.sqrt(np.mean(np.abs(clean) ** 2) / 2) * 10 ** (-snr_db / 20)
    nrng = np.random.default_rng(seed)
    noisy = (clean + sigma * (nrng.standard_normal(clean.shape) + 1j * nrng.standard_normal(clean.shape))).astype(np.complex64)
    for name, rx_iq in (("noise free", clean), ("awgn", noisy)):
        for u in range(3):
            # the cell transmits at rho_a = sqrt(2) 10^(p_a/20) (pdsch.c:525): the receiver is told (srslte_pdsch_cfg_t.power_scale / p_a)
            rx = hp.DlRx(cid, prb, cfi, 0x300 + u, 1, 15264, 6, nsf, True, _chest(hp), nof_rx=2, nof_ports=2, power_scale=True, p_a=0.0)
            rc, tb, ok = rx.decode_grants2(rx_iq, tti0, [it[0] for it in per_ue[u]])
            assert rc == 0
            for b, (g, d, kind, mask, pmi) in enumerate(per_ue[u]):
                if name == "awgn":  # the oracle's chain on the same samples decodes this PDSCH: the SNR is a fair one
                    kw = dict(cfi=cfi, rnti=0x300 + u, nof_rx=2, nof_ports=2, p_a=0.0, prb_mask=mask)
                    if kind == "div":
                        assert oracle_rx(DlConfig(prb, cid, g.tb0.mod, g.tb0.tbs, **kw), rx_iq[b], tti0 + b)["ok"], (u, b, kind)
                    else:
                        c = DlConfig(prb, cid, g.tb0.mod, g.tb0.tbs, tx_scheme="cdd" if kind == "cdd" else "mux", pmi=pmi, mod2=g.mod2 or None, tbs2=g.tbs2, **kw)
                        assert all(oracle_rx_mimo(c, rx_iq[b], tti0 + b)["ok"]), (u, b, kind)
                for cw, dd in enumerate(d):
                    assert ok[cw][b] and np.array_equal(tb[cw][b][:len(dd)], dd), (name, u, b, kind, cw)
                if len(d) == 1:
                    assert not ok[1][b], (name, u, b)
            rx.free()


def _call2(hp, tx, datas, tti0, nof_sf, grants, stream=None, d_iq=None):
    """srslte_hip_dl_tx_batch_grants2 without the mirror's synchronisation: (rc, the device buffer of the payload rows - keep it until the stream is done)."""
    n = len(grants)
    din, stride = tx._tb_rows2(datas, n)
    arr = (hp.DlTxGrant2 * max(1, n))(*[hp.DlTxGrant2(sf, g) for sf, g in grants])
    fn = hp.lib().srslte_hip_dl_tx_batch_grants2
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    return fn(tx.h, din.ptr, stride, tti0, nof_sf, arr, n, (d_iq or tx.d_iq).ptr, stream), din


def test_grants2_batch_shapes_and_object_reuse(hp):
    """nof_sf 1 and 128, nof_grants 0; the first two-codeword call on an object that has served single-codeword calls and the other way round
    (the state is made anew for twice the codewords: results do not change); two objects on two streams."""
    prb, cid = 25, 7
    rng = np.random.default_rng(7600)
    full = _mask(prb, [(0, 25)])
    g1 = [(0, hp.DlGrant.make(prb, 2, 4008, 0x77, cfi=1, prb_mask=full))]
    d1 = [rng.integers(0, 256, 501, dtype=np.uint8)]
    gm = lambda sf, kind, pmi=0, two=True: (sf, _grant2(hp, prb, kind, full, 0x77, 2, 4008, 0, 3 if two else 0, 6200 if two else 0, 1, pmi))  # noqa: E731
    dm = lambda two=True: [rng.integers(0, 256, t // 8, dtype=np.uint8) for t in ((4008, 6200) if two else (4008,))]  # noqa: E731
    a, b_ = hp.DlTx(cid, prb, 1, 0x1234, 1, 6200, 128, 2, 0.0, max_grants=128), hp.DlTx(cid, prb, 1, 0x1234, 1, 6200, 128, 2, 0.0, max_grants=128)
    first = a.encode_grants(d1, 3, 1, g1).copy()                     # nof_sf 1, the single-codeword state
    d_cdd = dm()
    rc, iq_a = a.encode_grants2([d_cdd], 3, 1, [gm(0, "cdd")])        # ... replaced by the two-codeword one
    assert rc == 0
    iq_a = iq_a.copy()
    assert np.array_equal(a.encode_grants(d1, 3, 1, g1), first)     # ... which serves the single-codeword call as before
    rc, iq_b = b_.encode_grants2([d_cdd], 3, 1, [gm(0, "cdd")])       # the other way round
    assert rc == 0 and np.array_equal(iq_b, iq_a)
    assert np.array_equal(b_.encode_grants(d1, 3, 1, g1), first)
    rc, crs = a.encode_grants2([], 0, 128, [])                       # no PDSCH at all: CRS-only subframes
    assert rc == 0 and np.abs(crs).max(axis=2).min() > 0
    # 128 subframes, a PDSCH in each, schemes rotating; the same on two objects and two streams at once
    kinds = [("cdd", 0, True), ("mux", 1, True), ("mux", 3, False), ("div", 0, False), ("mux", 0, True)]
    grants = [gm(sf, *kinds[sf % 5]) for sf in range(128)]
    datas = [dm(kinds[sf % 5][2]) for sf in range(128)]
    rc, want = a.encode_grants2(datas, 5, 128, grants)
    assert rc == 0
    want = want.copy()
    L = hp.lib()
    s1, s2 = L.srslte_hip_stream_create(), L.srslte_hip_stream_create()
    rc1, keep1 = _call2(hp, a, datas, 5, 128, grants, s1)
    rc2, keep2 = _call2(hp, b_, datas, 5, 128, grants, s2)
    L.srslte_hip_stream_sync(s1), L.srslte_hip_stream_sync(s2)
    assert rc1 == 0 and rc2 == 0
    for t in (a, b_):
        assert np.array_equal(t.d_iq.to_host(np.complex64).reshape(128, 2, -1), want)
    L.srslte_hip_stream_destroy(s1), L.srslte_hip_stream_destroy(s2)
    a.free()
    b_.free()


def test_grants2_refusals_leave_d_iq_untouched(hp):
    """Every refusal returns SRSLTE_ERROR_INVALID_INPUTS before anything is queued: a poisoned d_iq keeps its bytes."""
    prb = 25
    full, none = _mask(prb, [(0, 25)]), _mask(prb, [])
    d = [[np.zeros(501, np.uint8), np.zeros(501, np.uint8)]]
    G = lambda kind, **kw: (kw.pop("sf", 0), _grant2(hp, prb, kind, kw.pop("mask", full), 1, kw.pop("mod", 2), kw.pop("tbs", 4008), **kw))  # noqa: E731
    two = dict(mod2=2, tbs2=4008)
    cases = {
        1: [G("cdd", **two), G("mux", **two), G("mux")],                                           # schemes 2 / 3 on a cell that is not 2-port
        4: [G("cdd", **two), G("mux")],
        2: [G("cdd"),                                                                              # CDD without a second block
            G("mux", pmi=2, **two), G("mux", pmi=4),                                               # pmi out of range for its block count
            G("div", **two),                                                                       # a diversity entry with tbs2 != 0
            G("cdd", mod2=5, tbs2=4008), G("cdd", mod2=0, tbs2=4008), G("mux", mod2=2, tbs2=4008, rv2=4),
            G("cdd", mod2=2, tbs2=6200), G("cdd", mod2=2, tbs2=4004),                              # above cfg.tbs; not a multiple of 8
            G("cdd", mod2=2, tbs2=4016), G("cdd", tbs=4016, **two),                                # filler bits
            G("cdd", mask=none, **two), G("mux", mask=none),                                       # fewer REs than code blocks
            G("cdd", sf=2, **two), G("mux", mod=5), G("mux", rv=4), G("mux", cfi=0)],             # as srslte_hip_dl_tx_batch_grants
    }
    L = hp.lib()
    for npt, bad in cases.items():
        tx = hp.DlTx(1, prb, 1, 0x1234, 2, 4008, 2, npt, max_grants=2)
        for how in ("fresh", "after a good call"):
            for i, g in enumerate(bad):
                L.srslte_hip_memset(tx.d_iq.ptr, 0xA5, tx.d_iq.nbytes)
                rc, _ = _call2(hp, tx, d, 0, 2, [g])
                hp.sync()
                assert rc == -2, (npt, how, i)
                assert (tx.d_iq.to_host(np.uint8) == 0xA5).all(), (npt, how, i)
            rc, _ = tx.encode_grants2([[d[0][0]]], 0, 2, [G("div")])
            assert rc == 0
        rc, _ = _call2(hp, tx, d * 3, 0, 2, [G("div")] * 3)  # more PDSCHs than cfg.max_grants
        assert rc == -2
        tx.free()
    # a block of two code-block lengths (6264 bits: C1 = C2 = 1, no filler bits) under cfg.tbs, as either block
    tx = hp.DlTx(1, prb, 1, 0x1234, 2, 7992, 2, 2, max_grants=2)
    d2 = [[np.zeros(999, np.uint8), np.zeros(999, np.uint8)]]
    for g in (G("cdd", mod2=2, tbs2=6264), G("cdd", tbs=6264, **two), G("mux", tbs=6264)):
        L.srslte_hip_memset(tx.d_iq.ptr, 0xA5, tx.d_iq.nbytes)
        rc, _ = _call2(hp, tx, d2, 0, 2, [g])
        hp.sync()
        assert rc == -2 and (tx.d_iq.to_host(np.uint8) == 0xA5).all()
    rc, _ = tx.encode_grants2(d2, 0, 2, [G("cdd", tbs=7992, mod2=2, tbs2=6200)])
    assert rc == 0
    tx.free()
    # extended-CP, TDD and MBSFN objects: out of scope of these calls, refused whatever the entry
    for kw in (dict(cp_ext=True), dict(tdd=(1, 4)), dict(mbsfn=(5, 2))):
        npt = 1 if "mbsfn" in kw else 2
        tx = hp.DlTx(1, prb, 1 if "mbsfn" not in kw else 2, 0x1234, 2, 4008, 2, npt, max_grants=2, **kw)
        L.srslte_hip_memset(tx.d_iq.ptr, 0xA5, tx.d_iq.nbytes)
        rc, _ = _call2(hp, tx, d, 0, 2, [G("div")])
        hp.sync()
        assert rc == -2 and (tx.d_iq.to_host(np.uint8) == 0xA5).all(), kw
        tx.free()


def _tm4_from_device(hp, tx, cfg, tti0, nsf, pmi, rng, H, snr_db, amp=0.2):
    """nsf TM4 subframes (one block, full band, precoder entry pmi) made by encode_grants2, then - on the host - the flat 2x2 channel
    H[antenna][port] with one delay per antenna and white noise, as tests/test_gpu_csi.py::_tm4_iq applies them to the oracle's grids.
    Returns (iq [nsf][2][sf_len], payloads)."""
    datas = [[rng.integers(0, 256, cfg.tbs // 8, dtype=np.uint8)] for _ in range(nsf)]
    grants = [(b, _grant2(hp, cfg.nof_prb, "mux", None, cfg.rnti, cfg.mod, cfg.tbs, pmi=pmi, cfi=cfg.cfi)) for b in range(nsf)]
    rc, _ = tx.encode_grants2(datas, tti0, nsf, grants)
    assert rc == 0
    grids = tx.debug(3, np.complex64, nsf * 2 * cfg.grid_len).reshape(nsf, 2, -1)
    q = OrcOfdm()
    oracle().orc_ofdm_init(C.byref(q), cfg.nof_prb, True)
    q.normalize = True
    kk = (np.arange(cfg.grid_len) % cfg.nre) - cfg.nre / 2
    sigma = np.sqrt(amp * amp * cfg.nre / cfg.N / 2) * 10 ** (-snr_db / 20)
    out = np.zeros((nsf, 2, cfg.sf_len), np.complex64)
    for b in range(nsf):
        for a in range(2):
            rxg = (grids[b, 0] * H[a][0] + grids[b, 1] * H[a][1]) * np.exp(-2j * np.pi * kk * (0.6 + 0.5 * a) / cfg.N)
            iq = np.zeros(cfg.sf_len, np.complex64)
            oracle().orc_ofdm_tx_sf(C.byref(q), p(np.ascontiguousarray(rxg.astype(np.complex64))), p(iq))
            out[b, a] = iq * np.float32(amp) + (sigma * (rng.standard_normal(cfg.sf_len) + 1j * rng.standard_normal(cfg.sf_len))).astype(np.complex64)
    return out, [d[0] for d in datas]


@pytest.mark.skipif(ref() is None, reason="oracle/_ref/libsrslte_ref.so is not built")
@pytest.mark.parametrize("prb,mod,tbs", [(25, 2, 4008), (100, 3, 30576)])
def test_closed_loop_pmi_and_ri_with_the_downlink_from_the_device(hp, prb, mod, tbs):
    """The scenario of tests/test_gpu_csi.py::test_closed_loop_pmi_and_ri_through_pusch_and_pucch with no host-made downlink: the TM4 batches
    come from encode_grants2. The cancelling precoder fails every block; the UE measures; the report travels through the PUSCH (aperiodic
    mode 31) and PUCCH format 2 (periodic wideband + PMI) and is unpacked by the reference's srslte_cqi_value_unpack; the eNB re-encodes with
    the reported pmi / ri through encode_grants2, and every block passes."""
    from lte_sim import DlConfig
    from test_gpu_csi import _ref_unpack
    cid, rnti, nsf, tti0, snr = 7, 0x1234, 2, 4, 12.0
    N = 14 * 12 * prb
    tx = hp.DlTx(cid, prb, 1, rnti, mod, tbs, nsf, 2, 0.0, max_grants=nsf)
    for theta, expect in ((0.0, 0), (np.pi / 2, 2)):
        rng = np.random.default_rng(7700 + prb + expect)
        H = np.outer([1.0, 0.8 * np.exp(0.9j)], [1.0, np.exp(-1j * theta)]) + 0.1 * np.array([[0.6 * np.exp(2.0j), -0.7], [0.5j, 0.8 * np.exp(-1.1j)]])
        wrong = {0: 1, 2: 3}[expect]
        cfg = DlConfig(prb, cid, mod, tbs, cfi=1, rnti=rnti, nof_rx=2, nof_ports=2, p_a=0.0, tx_scheme="mux", pmi=wrong, tbs2=0)
        iq0, _ = _tm4_from_device(hp, tx, cfg, tti0, nsf, wrong, rng, H, snr)
        rxkw = dict(nof_rx=2, nof_ports=2, tx_scheme=2, power_scale=True, p_a=0.0)
        rx0 = hp.DlRx(cid, prb, 1, rnti, mod, tbs, 6, nsf, True, _chest(hp), pmi=wrong, **rxkw)
        _, ok0 = rx0.decode(iq0, tti0)
        assert not ok0.any(), "the cancelling precoder should not decode"
        rc, recs = rx0.csi(nsf)
        assert rc == 0
        rx0.free()
        assert [(r.ri, r.pmi) for r in recs] == [(0, expect)] * nsf, (theta, [(r.ri, r.pmi) for r in recs])
        # aperiodic mode 31 on the PUSCH
        rep = hp.CsiReportCfg(4, prb, 2, 2, 0, 1, 0, 0, 0, 0, 31, 0.0, 1)
        outs = []
        for b in range(nsf):
            rc, out = hp.csi_gen_cqi_aperiodic(recs[b], rep, recs[b].cqi_wideband)
            assert rc == 0 and out.ri_len == 1 and out.ri == 0
            outs.append(out)
        clen = outs[0].cqi_len
        L_prb, n_prb, ul_tbs = 12, 2, 1000
        kw = dict(ri_len=1, I_offset_ri=6, cqi_len=clen, I_offset_cqi=6)
        utx = hp.UlTx(cid, prb, rnti, 1, ul_tbs, L_prb, n_prb, 3, nsf, **kw)
        urx = hp.UlRx(cid, prb, rnti, 1, ul_tbs, L_prb, n_prb, 3, 6, nsf, **kw)
        ul_data = rng.integers(0, 256, (nsf, ul_tbs // 8), dtype=np.uint8)
        bits = np.array([list(o.cqi_bits[:clen]) for o in outs], np.uint8)
        ul_iq = utx.encode(ul_data, tti0 + 4, ri=np.array([[o.ri] for o in outs], np.uint8), cqi=bits)
        _, ul_ok = urx.decode(ul_iq, tti0 + 4)
        got_bits, got_crc = urx.cqi()
        assert ul_ok.all() and got_crc.all() and np.array_equal(got_bits, bits)
        ri_rx = [int(v) for v in urx.ri()[:, 0]]
        utx.free()
        urx.free()
        reported = []
        for b in range(nsf):
            n, v = _ref_unpack(outs[b].cqi, got_bits[b])
            assert n == clen
            reported.append(int(v.subband_hl.pmi))
        # periodic wideband + PMI on PUCCH format 2: I_cqi_pmi 0 reports in even TTIs
        per = hp.CsiReportCfg(4, prb, 2, 2, 0, 1, 0, 0, 0, 0, 31, 0.0, rep.last_ri)
        txs, reqs, pouts = [], [], []
        for b in range(nsf):
            rc, out = hp.csi_gen_cqi_periodic(recs[b], per, recs[b].cqi_wideband, tti0 + b)
            assert rc == 0
            if out.cqi_len:
                req = hp.PucchReq.make(b, rnti, cqi_len=out.cqi_len, n_pucch_2=3, noise_estimate=0.1)
                reqs.append(req), txs.append(hp.PucchTx.make(req, cqi=list(out.cqi_bits[:out.cqi_len]))), pouts.append((b, out))
        assert len(reqs) == 1
        ptx, prx = hp.UlCtrlTx(prb, cid, max_pucch=nsf), hp.UlCtrl(prb, cid, max_pucch=nsf)
        rc, grid = ptx.put(np.zeros((nsf, N), np.complex64), tti0, txs)
        assert rc == 0
        rc, pres = prx.batch(grid, tti0, reqs)
        assert rc == 0
        for (b, out), pr in zip(pouts, pres):
            n, v = _ref_unpack(out.cqi, list(pr.cqi[:6]))
            assert pr.detected and n == 4 and v.wideband.pmi == expect
        ptx.free()
        prx.free()
        # the next downlink batch with what the eNB read: RI 0 -> one layer, the reported entry
        assert reported == [expect] * nsf and ri_rx == [0] * nsf
        iq1, sent = _tm4_from_device(hp, tx, cfg, tti0 + 8, nsf, reported[0], rng, H, snr)
        rx1 = hp.DlRx(cid, prb, 1, rnti, mod, tbs, 6, nsf, True, _chest(hp), pmi=reported[0], **rxkw)
        tb1, ok1 = rx1.decode(iq1, tti0 + 8)
        assert ok1.all(), (theta, ok1)
        for b in range(nsf):
            assert np.array_equal(tb1[b][:tbs // 8], sent[b])
        rx1.free()
    tx.free()


class _RefDciTb(C.Structure):
    """srslte_dci_tb_t (dci.h)."""
    _fields_ = [("mcs_idx", C.c_uint32), ("rv", C.c_int), ("ndi", C.c_bool), ("cw_idx", C.c_uint32)]


class _RefDciDl(C.Structure):
    """srslte_dci_dl_t (dci.h) as srslte_dci_msg_pack_pdsch reads it; the allocation union as its largest member (type 2), whose first word is
    the type-0 RBG bitmask."""
    _fields_ = [("rnti", C.c_uint16), ("format", C.c_int), ("L", C.c_uint32), ("ncce", C.c_uint32), ("alloc_type", C.c_int), ("rbg_bitmask", C.c_uint32),
                ("alloc_rest", C.c_uint32 * 3), ("tb", _RefDciTb * 2), ("tb_cw_swap", C.c_bool), ("pinfo", C.c_uint32), ("pconf", C.c_bool),
                ("power_offset", C.c_bool), ("tpc_pucch", C.c_uint8), ("is_ra_order", C.c_bool), ("ra_preamble", C.c_uint32), ("ra_mask_idx", C.c_uint32),
                ("cif", C.c_uint32), ("cif_present", C.c_bool), ("srs_request", C.c_bool), ("srs_request_present", C.c_bool), ("pid", C.c_uint32),
                ("dai", C.c_uint32), ("is_tdd", C.c_bool), ("is_dwpts", C.c_bool), ("sram_id", C.c_bool)]


def _pack_dci2(cell, tti, cfi, fmt, rnti, L, ncce, rbg_bitmask, mcs, pinfo):
    """srslte_dci_msg_pack_pdsch of a type-0 format 2 / 2A DCI; mcs: one or two MCS indices (a disabled block is mcs 0, rv 1) -> RefDciMsg."""
    from _libs import RefDlSfCfg
    from dl_ctrl_ref import RefDciMsg
    d = _RefDciDl()
    d.rnti, d.format, d.L, d.ncce, d.alloc_type, d.rbg_bitmask, d.pinfo = rnti, fmt, L, ncce, 0, rbg_bitmask, pinfo
    for i in range(2):
        d.tb[i].cw_idx = i
        d.tb[i].mcs_idx, d.tb[i].rv = (mcs[i], 0) if i < len(mcs) else (0, 1)
    sf, msg = RefDlSfCfg(), RefDciMsg()
    sf.tti, sf.cfi = tti, cfi
    R = cell.R
    R.srslte_dci_msg_pack_pdsch.argtypes = [C.c_void_p] * 5
    assert R.srslte_dci_msg_pack_pdsch(C.byref(cell.cell), C.byref(sf), None, C.byref(d), C.byref(msg)) == 0
    return msg


def _grant2_of(hp, prb, g, rnti, cfi):
    """dl_ctrl_ref.unpack_grant's dict -> DlGrant2, for either direction."""
    t0, t1 = g["tb"]
    assert t0["enabled"]
    g2 = hp.DlGrant2(hp.DlGrant.make(prb, t0["mod"], t0["tbs"], rnti, cfi=cfi, rv=max(0, t0["rv"]), prb_mask=g["prb_idx"]), g["tx_scheme"], g["pmi"], 0, 0, 0, 1)
    if t1["enabled"]:
        g2.mod2, g2.tbs2, g2.rv2 = t1["mod"], t1["tbs"], max(0, t1["rv"])
    return g2


def _device_tbs_ok(hp, tbs):
    rc, s = hp.cbsegm(tbs)
    return rc == 0 and tbs % 8 == 0 and s.F == 0 and s.C2 == 0


@pytest.mark.skipif(ref() is None, reason="oracle/_ref/libsrslte_ref.so is not built")
def test_whole_subframes_with_dci_format_2_and_2a(hp):
    """encode_grants2_full for 12 subframes (a subframe 0 and a subframe 5 among them) of a 50-PRB 2-port cell: per subframe a TM4 UE announced
    by a DCI format 2 and a TM3 UE by a format 2A, packed by the reference's srslte_dci_msg_pack_pdsch, with PCFICH, PSS / SSS / PBCH. Over a
    flat 2x2 channel at 30 dB srslte_hip_dl_ctrl_batch with tm 3 / 2 finds each UE's DCI bit for bit, dl_ctrl_ref.unpack_grant turns it into
    the DlGrant2 the transmitter was given, and decode_grants2 returns every block of both codewords."""
    from dl_ctrl_ref import F2, F2A, unpack_grant
    from dl_ctrl_tx_ref import TxCell
    from test_gpu_dl_ctrl import _ctrl_on_device, _front
    prb, cid, tti0, nsf = 50, 151, 10 * 321 + 7, 12
    cell = TxCell(prb, 2, cid, False, 2, False)
    rng = np.random.default_rng(7800)
    ues = [dict(rnti=0x4A1, tm=3, fmt=F2, rbg=0x001FF), dict(rnti=0x5B2, tm=2, fmt=F2A, rbg=0x1FE00)]
    cfis, grants, datas, dcis, per_ue = [], [], [], [], [[], []]
    for b in range(nsf):
        tti, cfi = tti0 + b, 2 + b % 2
        cfis.append(cfi)
        taken = set()
        for u, ue in enumerate(ues):
            L, n0 = next((l, n) for l, n in hp.pdcch_ue_locations(cell.ncce[cfi - 1], tti % 10, ue["rnti"]) if l == 1 and not taken & set(range(n, n + 2)))
            taken |= set(range(n0, n0 + 2))
            two = (b % 3 != 0) if u == 0 else (b % 4 != 3)
            pinfo = 0 if u == 1 else ((b % 2) if two else 1 + b % 4)  # 36.212 Table 5.3.3.1.5-4; format 2A has no field on 2 ports
            while True:
                mcs = [int(v) for v in rng.integers(2, 13, 2 if two else 1)]
                msg = _pack_dci2(cell, tti, cfi, ue["fmt"], ue["rnti"], L, n0, ue["rbg"], mcs, pinfo)
                g = unpack_grant(cell, tti, cfi, msg, ue["tm"])
                assert g is not None
                if all(_device_tbs_ok(hp, t["tbs"]) for t in g["tb"] if t["enabled"]):
                    break
            assert g["tx_scheme"] == ((2 if (two or pinfo) else 1) if u == 0 else (3 if two else 1)) and g["tb"][1]["enabled"] == two
            g2 = _grant2_of(hp, prb, g, ue["rnti"], cfi)
            d = [rng.integers(0, 256, t["tbs"] // 8, dtype=np.uint8) for t in g["tb"] if t["enabled"]]
            dcis.append((b, msg)), grants.append((b, g2)), datas.append(d)
            per_ue[u].append((g2, d, bytes(msg.payload[:msg.nof_bits])))
        assert not (per_ue[0][-1][0].tb0.prb_mask[0][0] & per_ue[1][-1][0].tb0.prb_mask[0][0]) and not (per_ue[0][-1][0].tb0.prb_mask[0][1] & per_ue[1][-1][0].tb0.prb_mask[0][1])
    tbs_max = max(max(g.tb0.tbs, g.tbs2) for _, g in grants)
    rc_s, seg = hp.cbsegm(tbs_max)
    while not _device_tbs_ok(hp, tbs_max):  # the object's own bound has to be a size the device segments
        tbs_max += 8
    tx = hp.DlTx(cid, prb, 1, 0x1234, 1, tbs_max, nsf, 2, 0.0, max_grants=len(grants))
    ctrl = hp.DlCtrlTx(prb, 2, cid, phich_resources=2, max_batch=nsf, max_dci=len(dcis))
    rc, time = tx.encode_grants2_full(datas, tti0, nsf, grants, ctrl, cfis, dcis)
    assert rc == 0
    ctrl.free()
    tx.free()
    iq = _mix(time, [[1.0, 0.35j], [0.3, 0.9 * np.exp(0.8j)]])
    sigma = 10 ** (-30 / 20) * np.sqrt(np.mean(np.abs(iq) ** 2))
    iq = (iq + sigma / np.sqrt(2) * (rng.normal(size=iq.shape) + 1j * rng.normal(size=iq.shape))).astype(np.complex64)
    bufs = _front(prb, 2, cid, iq, tti0, nof_rx=2)
    rx_ctrl = hp.DlCtrl(prb, 2, cid, phich_resources=2, nof_rx=2, max_batch=nsf)
    for u, ue in enumerate(ues):
        res, msgs = _ctrl_on_device(rx_ctrl, bufs, tti0, [hp.DlCtrlReq(ue["rnti"], ue["tm"], 0, 0)] * nsf)
        rx_grants = []
        for b, (g2, d, bits) in enumerate(per_ue[u]):
            assert res[b].cfi == cfis[b] and res[b].nof_dci == 1 and msgs[b].format == ue["fmt"] and bytes(msgs[b].payload[:msgs[b].nof_bits]) == bits, (u, b)
            g = unpack_grant(cell, tti0 + b, cfis[b], msgs[b], ue["tm"])
            r2 = _grant2_of(hp, prb, g, ue["rnti"], cfis[b])
            assert bytes(r2) == bytes(g2), (u, b)  # the grant unpacked once serves both directions
            rx_grants.append(r2)
        rx = hp.DlRx(cid, prb, 1, ue["rnti"], 1, tbs_max, 6, nsf, True, _chest(hp), nof_rx=2, nof_ports=2, power_scale=True, p_a=0.0)
        rc, tb, ok = rx.decode_grants2(bufs[3], tti0, rx_grants, from_grid=True)
        rx.free()
        assert rc == 0
        for b, (g2, d, bits) in enumerate(per_ue[u]):
            for cw, dd in enumerate(d):
                assert ok[cw][b] and np.array_equal(tb[cw][b][:len(dd)], dd), (u, b, cw, g2.tx_scheme, g2.pmi)
    rx_ctrl.free()


def test_grants2_ctrl_puts_the_control_region_beside_two_layer_pdschs(hp):
    """encode_grants2_ctrl with TM3 / TM4 PDSCHs, DCIs and PHICHs: the control symbols are those encode_grants_ctrl writes for the same inputs,
    everything behind them is what encode_grants2 writes for the same grants; _full adds PSS / SSS / PBCH and nothing else moves; a grant whose
    cfi is not its subframe's is refused with d_iq untouched."""
    from types import SimpleNamespace
    from dl_ctrl_ref import format1a_msg
    prb, cid, tti0, nsf = 25, 12, 9, 3  # subframes 9, 0, 1
    rng = np.random.default_rng(7900)
    cfis = [1, 2, 3]
    lo, hi = _mask(prb, [(0, 12)]), _mask(prb, [(12, 25)])
    g2, g1, datas = [], [], []
    for b in range(nsf):
        g2 += [(b, _grant2(hp, prb, "cdd", lo, 0x61, 2, 2216, 0, 1, 1000, 2, 0, cfi=cfis[b])), (b, _grant2(hp, prb, "mux", hi, 0x62, 2, 1544, 1, 0, 0, 0, b, cfi=cfis[b]))]
        g1 += [(b, hp.DlGrant.make(prb, 2, 2216, 0x61, cfi=cfis[b], prb_mask=lo)), (b, hp.DlGrant.make(prb, 2, 1544, 0x62, cfi=cfis[b], prb_mask=hi))]
        datas += [[rng.integers(0, 256, 277, dtype=np.uint8), rng.integers(0, 256, 125, dtype=np.uint8)], [rng.integers(0, 256, 193, dtype=np.uint8)]]
    c = SimpleNamespace(nof_prb=prb, ports=2)
    dcis = [(b, format1a_msg(c, 0x61 + u, 0, u, 6, 3 * u, 5)) for b in range(nsf) for u in range(2)]
    phichs = [(b, 3 * k, k, 0, k & 1) for b in range(nsf) for k in range(3)]
    tx = hp.DlTx(cid, prb, 1, 0x1234, 1, 2216, nsf, 2, 0.0, max_grants=len(g2))
    ctrl = hp.DlCtrlTx(prb, 2, cid, phich_resources=1, max_batch=nsf, max_dci=len(dcis), max_phich=len(phichs))
    n = nsf * 2 * 14 * 12 * prb
    grid = lambda: tx.debug(3, np.complex64, n).reshape(nsf, 2, 14, 12 * prb).copy()  # noqa: E731
    rc, _ = tx.encode_grants_ctrl([d[0] for d in datas], tti0, nsf, g1, ctrl, cfis, dcis, phichs)
    assert rc == 0
    one = grid()
    rc, _ = tx.encode_grants2(datas, tti0, nsf, g2)
    assert rc == 0
    plain = grid()
    rc, iq_c = tx.encode_grants2_ctrl(datas, tti0, nsf, g2, ctrl, cfis, dcis, phichs)
    assert rc == 0
    both, iq_c = grid(), iq_c.copy()
    rc, iq_f = tx.encode_grants2_full(datas, tti0, nsf, g2, ctrl, cfis, dcis, phichs)
    assert rc == 0
    full = grid()
    for b, cfi in enumerate(cfis):
        assert np.array_equal(both[b, :, :cfi], one[b, :, :cfi]) and np.abs(both[b, :, :cfi] - plain[b, :, :cfi]).max() > 0.1, b
        assert np.array_equal(both[b, :, cfi:], plain[b, :, cfi:]), b
    # PSS / SSS / PBCH: in subframe 0 only (b = 1), on the centre 6 PRBs, where no PDSCH RE lies; the rest of the grids does not move
    assert np.array_equal(full[0], both[0]) and np.array_equal(full[2], both[2])
    moved = np.argwhere(full[1] != both[1])
    assert len(moved) > 200 and moved[:, 1].min() >= 5 and moved[:, 1].max() <= 10 and moved[:, 2].min() >= 12 * prb // 2 - 36 and moved[:, 2].max() < 12 * prb // 2 + 36
    assert (both[1][full[1] != both[1]] == 0).all()  # nothing of a PDSCH or the control region was overwritten
    assert not np.array_equal(iq_f[1], iq_c[1]) and np.array_equal(iq_f[0], iq_c[0])
    # a grant whose cfi differs from its subframe's: refused before anything is queued
    L = hp.lib()
    bad = list(g2)
    bad[2] = (1, _grant2(hp, prb, "cdd", lo, 0x61, 2, 2216, 0, 1, 1000, 2, 0, cfi=3))
    for fn in (tx.encode_grants2_ctrl, tx.encode_grants2_full):
        L.srslte_hip_memset(tx.d_iq.ptr, 0xA5, tx.d_iq.nbytes)
        rc, _ = fn(datas, tti0, nsf, bad, ctrl, cfis, dcis, phichs)
        hp.sync()
        assert rc == -2 and (tx.d_iq.to_host(np.uint8) == 0xA5).all()
    ctrl.free()
    tx.free()
