"""The oracle on silent captures, non-finite symbols and zero-parity transport blocks (silent_cases.py says what they are): its answers are
recorded here as assertions, so that a changed oracle shows up before the GPU tests that take it as their judge (test_gpu_silent.py,
test_gpu_zero_parity.py), and - where oracle/_ref is built - it is compared with the reference's own compiled code on these very inputs:
the demappers srslte_demod_soft_demodulate / _s / _b element for element, the chains through srslte_pdsch_decode and srslte_ulsch_decode
(the drivers of test_oracle_vs_ref.py). No GPU."""
import numpy as np
import pytest

from _libs import acopy, aligned, oracle, p, ref
from lte_sim import OrcHarq, make_subframe, make_ul_subframe, oracle_rx, oracle_ul_rx
from silent_cases import (AMP, DL_CK, DL_SHAPES, NONFINITE, UL_CK, UL_SHAPES, nan_symbols, random_payload, same_floats, symbol_set,
                          zero_parity_payload)

needs_ref = pytest.mark.skipif(ref() is None, reason="oracle/_ref/libsrslte_ref.so not built")
KINDS = (("f", "", np.float32), ("s", "_s", np.int16), ("b", "_b", np.int8))


def _qm(mod):
    return 1 if mod == 0 else 2 * mod


def _orc_demod(mod, x, kind):
    dt = dict((k, d) for k, _, d in KINDS)[kind]
    out = np.zeros(len(x) * _qm(mod), dt)
    assert getattr(oracle(), "orc_demod_soft_" + kind)(mod, p(np.ascontiguousarray(x)), p(out), len(x)) == 0
    return out


# ---------------------------------------------------------------------------------------------------------------- recorded answers
def test_symbol_set_is_out_of_range_of_every_demapper():
    """| value x gain | >= 2^31 for NaN, +-Inf and +-3e9 at every gain of demod_soft.c (20 .. 1000, the smallest for 8-bit QPSK / BPSK:
    20 sqrt 2 and 20 / sqrt 2 - BPSK adds two components first); 1e7 x gain stays below 2^31 up to the gain 100 sqrt 2."""
    assert 3e9 * 20 / np.sqrt(2) >= 2.0 ** 31 and 1e7 * 100 * np.sqrt(2) < 2.0 ** 31 and 1e7 * 20 > 32767
    s = symbol_set(33)
    comp = s.view(np.float32)
    assert np.isnan(comp).sum() >= 8 and np.isposinf(comp).sum() >= 8 and np.isneginf(comp).sum() >= 8 and (comp == 0).sum() >= 8
    for start in range(len(NONFINITE)):  # every value reaches every position of a group of eight components
        assert np.array_equal(symbol_set(4, start).view(np.float32), np.roll(NONFINITE, -start), equal_nan=True)


@pytest.mark.parametrize("mod", [1, 2, 3])
def test_oracle_conversion_rule(mod):
    """The x86 rule the oracle models (orc_modem.c cvt_rne / cvt_trunc): in the vector bodies a NaN and every out-of-range value become
    0x80000000 and the packs saturate that to -32768 / -128 - whatever the sign of the value; in the scalar tails the same 0x80000000 is
    truncated to 0. A NaN symbol in the body therefore gives -32768 in its first two LLRs, in the tail 0."""
    for kind, lo, step in (("s", -32768, 8 if mod == 1 else 4), ("b", -128, 8)):
        qm = _qm(mod)
        body = _orc_demod(mod, nan_symbols(step), kind).reshape(step, qm)
        tail = _orc_demod(mod, nan_symbols(step - 1), kind).reshape(step - 1, qm)
        assert (body[:, :2] == lo).all() and (tail[:, :2] == 0).all(), (kind, body, tail)
        pos = np.full(step, 3e9 + 3e9j, np.complex64)  # times a negative gain: a negative overflow, and its mirror image
        assert (_orc_demod(mod, pos, kind).reshape(step, qm)[:, :2] == lo).all() and (_orc_demod(mod, -pos, kind).reshape(step, qm)[:, :2] == lo).all()


@pytest.mark.parametrize("name", list(DL_SHAPES))
def test_oracle_answers_dl(name):
    """Zero-parity blocks: ok False, one pass per block, every block CRC 1, the bytes those that were sent, parity bytes 00 00 00; a random
    payload of the same shape: ok True. Silent capture: noise 0, snr_db NaN, every equalised symbol NaN, LLRs -32768 (vector body) and 0
    (scalar tail: the shapes with nof_re % 8 != 0) only, one pass per block, block CRCs 1, the block all zero, ok False. With 8-bit LLRs
    -128 / 0, with two ports all 0. With the CSI weighting the subframe's maximum is 0 and the scale 32767 / 0: 0 x Inf is a NaN, which
    _mm_cvtps_pi16 turns into the weight -32768, and (-32768 x -32768) >> 16 = 16384 in the vector body, (int16) NaN = 0 in the tail -
    the reference's answer (test_dl_chain_vs_reference_pdsch_decode); the oracle said 0 everywhere until its weight got the x86 rule."""
    mk, tti = DL_SHAPES[name]
    cfg = mk()
    assert (cfg.seg.C, cfg.seg.K1) == DL_CK[name]
    rng = np.random.default_rng(5)
    for how in ("zeros", "crc", "random"):
        d = random_payload(cfg.tbs, rng) if how == "random" else zero_parity_payload(cfg.tbs, how, rng)
        iq, _ = make_subframe(cfg, tti, rng, amp=AMP, data=d)
        r = oracle_rx(cfg, iq, tti)
        assert r["ok"] == (how == "random") and (r["iters"] == 1).all() and r["cb_ok"].all(), how
        assert np.array_equal(r["tb"][:cfg.tbs // 8], d) and (r["tb"][-3:].any() == (how == "random")), how
    for kw, vals, raw in (({}, {-32768, 0}, {-32768, 0}), ({"llr8": True}, {-128, 0}, {-128, 0}), ({"csi": True}, {16384, 0}, {-32768, 0}),
                          ({"nof_ports": 2}, {0}, {0}), ({"nof_rx": 2}, {-32768, 0}, {-32768, 0})):
        c2 = mk(**kw)
        r = oracle_rx(c2, np.zeros((c2.nof_rx, c2.sf_len), np.complex64), tti, keep=True)
        assert r["noise"] == 0.0 and np.isnan(r["res"].snr_db), kw
        assert np.isnan(r["d"].view(np.float32)).all() == (c2.nof_ports == 1), kw
        got, got_raw = set(np.unique(r["e"]).tolist()), set(np.unique(r["e_raw"]).tolist())
        assert got <= vals and max(vals, key=abs) in got and got_raw <= raw and min(raw) in got_raw, (kw, got, got_raw)
        if c2.nof_ports == 1 and len(c2.indices(tti % 10)) % 8 == 0:
            assert got_raw == {min(raw)}, kw  # no scalar tail: every LLR non-zero
        if c2.csi:  # +16384 throughout is no code word: every pass runs, the block CRCs fail, some delivered bytes are non-zero
            assert not r["ok"] and (r["iters"] == 6).all() and not r["cb_ok"].any() and r["tb"].any(), kw
        else:
            assert not r["ok"] and (r["iters"] == 1).all() and r["cb_ok"].all() and not r["tb"].any(), kw


@pytest.mark.parametrize("name", list(UL_SHAPES))
def test_oracle_answers_ul(name):
    """As test_oracle_answers_dl. The silent capture on the 25-PRB shape is the case that is not "all zero": six passes, the block CRC
    fails, 403 of the delivered bytes are non-zero."""
    cfg = UL_SHAPES[name]()
    assert (cfg.seg.C, cfg.seg.K1) == UL_CK[name]
    rng = np.random.default_rng(6)
    for how in ("zeros", "crc", "random"):
        d = random_payload(cfg.tbs, rng) if how == "random" else zero_parity_payload(cfg.tbs, how, rng)
        iq, _ = make_ul_subframe(cfg, 4, rng, amp=AMP, data=d)
        r = oracle_ul_rx(cfg, iq, 4)
        assert r["ok"] == (how == "random") and (r["iters"] == 1).all() and r["cb_ok"].all(), how
        assert np.array_equal(r["tb"][:cfg.tbs // 8], d) and (r["tb"][-3:].any() == (how == "random")), how
    r = oracle_ul_rx(cfg, np.zeros(cfg.sf_len, np.complex64), 4, keep=True)
    assert r["noise"] == 0.0 and np.isnan(r["d"].view(np.float32)).all() and not r["ok"]
    if name == "K352":
        assert (r["g"] == -32768).all() and r["iters"][0] == 1 and r["cb_ok"][0] == 1 and not r["tb"].any()
    else:
        assert set(np.unique(r["g"]).tolist()) == {-32768, -32516, 32516}  # 16QAM: | -32768 | - 252 wraps
        assert r["iters"][0] == 6 and r["cb_ok"][0] == 0 and np.count_nonzero(r["tb"]) == 403


def test_oracle_harq_after_silence():
    """The soft buffer after a silent first transmission is full of -32768; the retransmission is wrap-added onto it: -32768 + x keeps x's
    low 15 bits and flips its sign, so a clean rv 2 on top of silence does not decode the way it does alone."""
    mk, tti = DL_SHAPES["K832"]
    cfg = mk()
    rng = np.random.default_rng(7)
    h = OrcHarq(cfg)
    r0 = oracle_rx(cfg, np.zeros(cfg.sf_len, np.complex64), tti, harq=h, rv=0, new_data=True)
    assert not r0["ok"] and (h.w[h.w != 0] == -32768).all() and np.count_nonzero(h.w) > cfg.seg.K1
    # every block CRC of the silent call passed (the block is all zero), so the retransmission finds its blocks already decoded
    assert h.crc.all()
    d = random_payload(cfg.tbs, rng)
    iq, _ = make_subframe(cfg, tti + 10, rng, amp=AMP, rv=2, data=d)
    r1 = oracle_rx(cfg, iq, tti + 10, harq=h, rv=2, new_data=False)
    assert not r1["ok"] and (r1["iters"] == 0).all() and not r1["tb"].any()


# ------------------------------------------------------------------------------------------------------- against the compiled reference
@needs_ref
@pytest.mark.parametrize("mod", [0, 1, 2, 3, 4])
def test_demappers_nonfinite_vs_ref(mod):
    """orc_demod_soft_f / _s / _b against srslte_demod_soft_demodulate / _s / _b on symbol_set(): nsym 3 is all scalar tail for every
    variant, 7 is all tail for the 8-symbol steps (QPSK, the 8-bit bodies) and body + tail for the 4-symbol ones, 16 all body, 33 body +
    tail; every start offset, so that each value meets each lane; and calls of NaN only. Integers exactly; floats: NaN and infinities in
    the same places (infinities with their sign), finite values to 1e-6."""
    R = ref()
    qm = _qm(mod)
    for nsym in (3, 7, 16, 33):
        for x in [symbol_set(nsym, start) for start in range(len(NONFINITE))] + [nan_symbols(nsym)]:
            xa = acopy(x.view(np.float32))
            for kind, name, dt in KINDS:
                l1 = aligned(nsym * qm + 64, dt)
                getattr(R, "srslte_demod_soft_demodulate" + name)(mod, p(xa), p(l1), nsym)
                l2 = _orc_demod(mod, x, kind)
                if kind == "f":
                    same_floats(l2, l1[:nsym * qm], 1e-6, (mod, nsym))
                else:
                    assert np.array_equal(l1[:nsym * qm], l2), (mod, nsym, kind, l1[:nsym * qm], l2)


def _dl_inputs(cfg, tti, rng):
    out = []
    for how in ("zeros", "crc"):
        d = zero_parity_payload(cfg.tbs, how, rng)
        out.append((how, make_subframe(cfg, tti, rng, amp=AMP, data=d)[0], d))
    out.append(("silent", np.zeros((cfg.nof_rx, cfg.sf_len), np.complex64), None))
    return out


@needs_ref
@pytest.mark.parametrize("name,kw", [("K352", {}), ("K832", {}), ("K352", {"llr8": True}), ("K832", {"csi": True}), ("K352", {"nof_rx": 2}),
                                     ("K352", {"csi": True}), ("K352", {"csi": True, "llr8": True}), ("K832", {"csi": True, "llr8": True})])
def test_dl_chain_vs_reference_pdsch_decode(name, kw):
    """srslte_chest_dl_estimate_cfg + srslte_pdsch_decode on the zero-parity subframes and the silent capture against the oracle chain:
    verdict, bytes and LLRs. On the silent capture the LLRs are equal element for element. On the noise-free subframes they may differ by
    one LSB: the reference's single-port equaliser multiplies by the AVX reciprocal approximation (relative error 1.5 * 2^-12, 0.04 LSB
    at | LLR | = 100), the oracle divides, and a noise-free QPSK LLR is +-100.0, right on the integer the truncation steps at - so
    how many differ is not bounded, by how much is."""
    from lte_sim import RefPdsch
    mk, tti = DL_SHAPES[name]
    cfg = mk(**kw)
    chain = RefPdsch(cfg, csi_enable=cfg.csi)
    for how, iq, d in _dl_inputs(cfg, tti, np.random.default_rng(8)):
        r, o = chain.run(iq, tti), oracle_rx(cfg, iq, tti, keep=True)
        assert r["ok"] == o["ok"] and not r["ok"], how
        assert np.array_equal(r["tb"], o["tb"]), how
        if how == "silent":
            assert r["noise"] == 0.0 and np.array_equal(r["e"], o["e"]), (how, np.unique(r["e"]), np.unique(o["e"]))
            assert np.array_equal(np.isnan(r["d"].view(np.float32)), np.isnan(o["d"].view(np.float32)))
        else:
            diff = np.abs(r["e"].astype(np.int32) - o["e"].astype(np.int32))
            assert diff.max() <= 1, (how, diff.max())
            assert np.array_equal(r["tb"][:cfg.tbs // 8], d) and not r["tb"][-3:].any(), how


@needs_ref
@pytest.mark.parametrize("name", list(UL_SHAPES))
def test_ul_chain_vs_reference_ulsch_decode(name):
    """srslte_ulsch_decode on the oracle chain's descrambled LLRs of the zero-parity subframes and of the silent capture (the -32768
    pattern; on the 25-PRB shape six passes and a failed block CRC): de-interleaved LLRs, verdict and bytes."""
    from lte_sim import RefUlsch
    cfg = UL_SHAPES[name]()
    chain = RefUlsch(cfg)
    rng = np.random.default_rng(9)
    inputs = [(how, zero_parity_payload(cfg.tbs, how, rng)) for how in ("zeros", "crc")]
    inputs = [(how, make_ul_subframe(cfg, 4, rng, amp=AMP, data=d)[0], d) for how, d in inputs] + [("silent", np.zeros(cfg.sf_len, np.complex64), None)]
    for how, iq, d in inputs:
        o = oracle_ul_rx(cfg, iq, 4, keep=True)
        r = chain.decode(o["q"], cfg.scramble(4))
        assert np.array_equal(r["g"], o["g"]) and r["ok"] == o["ok"] and not r["ok"], how
        assert np.array_equal(r["tb"], o["tb"]), how
        if d is not None:
            assert np.array_equal(r["tb"][:cfg.tbs // 8], d) and not r["tb"][-3:].any(), how
