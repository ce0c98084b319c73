"""The batched channel emulator on the device (srslte_hip_channel_*) against the NumPy restatement (tests/channel_ref.py) and the outputs
recorded from the reference's own sources (tests/golden/channel.npz, tests/gen_golden_channel.py).

Bounds. Against the restatement: the project's standing rule, |a - b| <= 1e-4 max(|b|, rms(b)). Against the fixture: 2e-4, the sum of that
bound and the same bound on the restatement's distance from the fixture, which tests/test_channel_host.py asserts on the CPU (measured there:
at most 7.4e-5, the N = 1024 filter, whose response upstream builds with a recursive oscillator). Delay and RLF alone are copies: bit-exact."""
import importlib

import numpy as np
import pytest

import channel_ref as R
from gen_golden_channel import CASES, GOLDEN, case_input

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(scope="module")
def hp():
    return importlib.import_module("srslte-emane_amd")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _err(a, b):
    b = np.asarray(b, np.complex128)
    rms = np.sqrt(np.mean(np.abs(b) ** 2))
    return float(np.max(np.abs(np.asarray(a, np.complex128) - b) / np.maximum(np.abs(b), rms)))


def _mk(hp, srate, channels, max_calls, max_len, seed0=0, **stages):
    return hp.Channel(hp.channel_cfg(srate, channels, max_calls, max_len, seed0=seed0, **stages))


def _noise(rng, shape):
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)).astype(np.complex64)


def _run_case(hp, name):
    """A fixture case through the device and the restatement -> ([channels][all samples] each, the restatement object)."""
    c = CASES[name]
    stages = {k: c[k] for k in ("fading", "delay", "hst", "rlf") if k in c}
    ch = _mk(hp, c["srate"], c["channels"], max(nb for _, _, nb in c["calls"]), c["len"], **stages)
    ref = R.ChannelRef(c["srate"], c["channels"], **stages)
    dev, res = [], []
    for (full, frac, nb), x in zip(c["calls"], case_input(name)):
        dev.append(ch.run(x, full, frac).reshape(c["channels"], -1))
        res.append(ref.run(x, full, frac).reshape(c["channels"], -1))
    if "fading" in c:
        assert ch.fft_size == ref.N and ch.path_delay == ref.N // 4
        for k in range(c["channels"]):
            for mine, theirs in zip(ch.coeffs(k), (ref.fading[k].a, ref.fading[k].w, ref.fading[k].p)):
                assert np.array_equal(mine, theirs)
    ch.free()
    return np.concatenate(dev, 1), np.concatenate(res, 1), ref


def _check_case(hp, golden, name, exact=False):
    dev, res, _ = _run_case(hp, name)
    e_res, e_fix = _err(dev, res), _err(dev, golden[name + ".out"])
    print("%s: device vs restatement %.3g, device vs recorded reference %.3g" % (name, e_res, e_fix))
    if exact:
        assert np.array_equal(dev, res.astype(np.complex64)) and np.array_equal(dev, golden[name + ".out"])
    else:
        assert e_res <= TOL and e_fix <= 2 * TOL


def test_fading_n64_state_across_blocks_and_calls(hp, golden):
    """1.92 MHz etu70 (N = 64; upstream's size is undefined there, so the restatement alone), 2 channels, len 1920: two blocks in one call,
    then a second call; and the recorded epa5 case of the same N with a short last segment."""
    ch = _mk(hp, 1.92e6, 2, 2, 1920, fading="etu70")
    ref = R.ChannelRef(1.92e6, 2, fading="etu70")
    assert ch.fft_size == 64 and ch.path_delay == 16
    rng = np.random.default_rng(1)
    for nb, (full, frac) in ((2, (5, 0.125)), (1, (5, 0.127))):
        x = _noise(rng, (2, nb, 1920))
        e = _err(ch.run(x, full, frac), ref.run(x, full, frac))
        print("etu70 N=64, %d block(s): %.3g" % (nb, e))
        assert e <= TOL
    ch.free()
    _check_case(hp, golden, "fading_epa5_n64")


def test_fading_n1024_short_last_segment_long_time(hp, golden):
    _check_case(hp, golden, "fading_etu300_n1024")


def test_fading_n512_blocks_shorter_than_a_segment(hp, golden):
    _check_case(hp, golden, "fading_eva70_n512")


def test_one_call_equals_split_calls_and_reset_repeats_bytes(hp):
    rng = np.random.default_rng(4)
    x = _noise(rng, (2, 4, 700))
    stages = dict(fading="eva5", delay=(10.0, 20.0, 1.0, 0.0), awgn=(0.01, 7))
    ch = _mk(hp, 7.68e6, 2, 4, 700, **stages)
    one = ch.run(x, 3, 0.5)
    ch.reset()
    again = ch.run(x, 3, 0.5)
    assert one.tobytes() == again.tobytes()
    ch.reset()
    parts = []
    for i in range(4):
        full, frac = R.block_time(3, 0.5, i, 700, 7680000)
        parts.append(ch.run(x[:, i:i + 1], full, frac))
    ch.free()
    e = _err(np.concatenate(parts, 1), one)
    print("four calls of one block vs one call of four: %.3g" % e)
    assert e <= TOL


def test_delay_alone_is_bit_exact(hp, golden):
    dev, res, ref = _run_case(hp, "delay")
    d = [t[0] for t in ref.trace]
    assert any(b > a for a, b in zip(d, d[1:])) and any(b < a for a, b in zip(d, d[1:]))  # grows and shrinks
    assert np.array_equal(dev, res.astype(np.complex64)) and np.array_equal(dev, golden["delay.out"])


def test_hst_alone_either_side_of_the_sign_change(hp, golden):
    _, _, ref = _run_case(hp, "hst")
    fs = [t[1] for t in ref.trace]
    assert fs[0] > 0 and fs[1] > 0 and fs[-1] < 0
    _check_case(hp, golden, "hst")


def test_rlf_alone_is_bit_exact(hp, golden):
    _, _, ref = _run_case(hp, "rlf")
    on = [t[2] for t in ref.trace]
    assert True in on and False in on
    _check_case(hp, golden, "rlf", exact=True)


def test_full_chain(hp, golden):
    """Fading, delay, HST and RLF as recorded from the reference; then the same chain with the noise stage on against the restatement."""
    _check_case(hp, golden, "chain")
    c = CASES["chain"]
    stages = {k: c[k] for k in ("fading", "delay", "hst", "rlf")}
    stages["awgn"] = (0.05, 11)
    ch = _mk(hp, c["srate"], 1, 3, c["len"], **stages)
    ref = R.ChannelRef(c["srate"], 1, **stages)
    for (full, frac, nb), x in zip(c["calls"], case_input("chain")):
        e = _err(ch.run(x, full, frac), ref.run(x, full, frac))
        print("chain with noise: %.3g" % e)
        assert e <= TOL
    ch.free()


def test_awgn_statistics_and_reproducibility(hp):
    C_, NB, L, n0 = 8, 4, 1920, 0.5
    ch = _mk(hp, 1.92e6, C_, NB, L, awgn=(n0, 1234))
    zero = np.zeros((C_, NB, L), np.complex64)
    y = ch.run(zero)
    n = NB * L
    for c in range(C_):
        v = y[c].reshape(-1).astype(np.complex128)
        for comp in (v.real, v.imag):
            sigma = np.sqrt(n0 / 2)
            assert abs(comp.mean()) <= 5 * sigma / np.sqrt(n)
            assert abs(comp.var() / (n0 / 2) - 1) <= 5 * np.sqrt(2 / n)
        assert abs(np.mean(v.real * v.imag)) / (n0 / 2) <= 5 / np.sqrt(n)
        for d in range(c):
            w = y[d].reshape(-1).astype(np.complex128)
            assert abs(np.mean(v * np.conj(w))) / n0 <= 5 / np.sqrt(n)
    # against the restatement's generator, the same seed again, and a run split into calls
    assert _err(y[3].reshape(-1), R.awgn(n0, 1234, 3, 0, n)) <= TOL
    ch.reset()
    assert ch.run(zero).tobytes() == y.tobytes()
    ch.reset()
    split = np.concatenate([ch.run(zero[:, :1]), ch.run(zero[:, 1:])], 1)
    assert split.tobytes() == y.tobytes()
    ch.free()
    other = _mk(hp, 1.92e6, C_, NB, L, awgn=(n0, 1235))
    assert other.run(zero).tobytes() != y.tobytes()
    other.free()


LOOPBACK_NSF, LOOPBACK_TTI0, LOOPBACK_TBS = 4, 1, 936


def test_loopback_dl_tx_channel_dl_rx(hp):
    """DlTx -> Channel (EPA5, no noise) -> DlRx on the device, the receiver's window shifted by path_delay. tests/test_channel_host.py checks the
    precondition on the CPU: the restatement's output for these subframes decodes in the oracle receiver."""
    nsf, sf_len = LOOPBACK_NSF, 1920
    rng = np.random.default_rng(10)
    payload = rng.integers(0, 256, (nsf, LOOPBACK_TBS // 8), dtype=np.uint8)
    tx = hp.DlTx(1, 6, 1, 0x1234, hp.MOD_QPSK, LOOPBACK_TBS, nsf)
    x = np.zeros((nsf + 1, sf_len), np.complex64)  # one zero subframe behind the signal: the filter's delay pushes the tail into it
    x[:nsf] = tx.encode(payload, LOOPBACK_TTI0)[:, 0]
    d_in = hp.DevBuf.from_host(x)
    ch = _mk(hp, 1.92e6, 1, nsf + 1, sf_len, fading="epa5")
    d_out = hp.DevBuf(d_in.nbytes)
    hp._check(ch.run_dev(d_in, d_out, nsf + 1, sf_len), "channel_run_batch")
    hc = hp.ChestDlCfg()
    hc.filter_coef[0], hc.filter_coef[1] = 4.0, 1.0
    rx = hp.DlRx(1, 6, 1, 0x1234, hp.MOD_QPSK, LOOPBACK_TBS, 6, nsf, True, hc)
    hp._check(rx.run_device(d_out.ptr + 8 * ch.path_delay, LOOPBACK_TTI0, nsf), "dl_rx_batch")
    hp.sync()
    tb = rx.d_tb.to_host(np.uint8).reshape(rx.max_batch, rx.tb_stride)[:nsf, :LOOPBACK_TBS // 8]
    ok = rx.d_ok.to_host(np.uint8)[:nsf]
    assert ok.all() and np.array_equal(tb, payload)
    for o in (tx, rx, ch):
        o.free()


def test_error_returns(hp):
    INV = hp.SRSLTE_ERROR_INVALID_INPUTS
    h = hp.C.c_void_p()

    def create(**kw):
        return hp.lib().srslte_hip_channel_create(hp.C.byref(h), hp.C.byref(hp.channel_cfg(1.92e6, 1, 2, 1920, **kw)))

    assert create(fading=(7, 5.0)) == INV and not h.value       # unknown model
    assert create(fading="none5") == INV                         # fading enabled with model none
    assert create(delay=(10.0, 100.0, 0.0, 0.0)) == INV          # a period of zero samples
    assert create(rlf=(0, 0)) == INV
    assert create(awgn=(-1.0, 0)) == INV
    assert hp.lib().srslte_hip_channel_create(hp.C.byref(h), hp.C.byref(hp.channel_cfg(1.92e6, 0, 1, 1))) == INV
    ch = _mk(hp, 1.92e6, 1, 2, 1920, delay=(10.0, 100.0, 1.0, 0.0))
    buf_in, buf_out = hp.DevBuf(3 * 1921 * 8), hp.DevBuf(3 * 1921 * 8)
    assert ch.run_dev(buf_in, buf_out, 2, 1921) == INV           # len > max_len
    assert ch.run_dev(buf_in, buf_out, 3, 1920) == INV           # nof_calls > max_calls
    assert ch.run_dev(buf_in, buf_in, 1, 1920) == INV            # in place
    assert ch.run_dev(buf_in, buf_out, 1, 64, 0, 0.25) == INV    # a block shorter than its delay (192 samples at the maximum)
    assert ch.run_dev(buf_in, buf_out, 1, 1920, in_strides=(1920, 100)) == INV
    assert ch.run_dev(buf_in, buf_out, 2, 1920) == hp.SRSLTE_SUCCESS
    hp.sync()
    ch.free()
