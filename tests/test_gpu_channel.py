"""The batched channel emulator on the device (srslte_hip_channel_*) against the NumPy restatement (tests/channel_ref.py) and the outputs
recorded from the reference's own sources (tests/golden/channel.npz, tests/gen_golden_channel.py).

Bounds. Against the restatement: the project's standing rule, |a - b| <= 1e-4 max(|b|, rms(b)). Against the fixture: 2e-4, the sum of that
bound and the same bound on the restatement's distance from the fixture, which tests/test_channel_host.py asserts on the CPU (measured there:
at most 7.4e-5, the N = 1024 filter, whose response upstream builds with a recursive oscillator; the N = 128 and N = 256 cases 9.0e-6 and
2.5e-5). Delay and RLF alone are copies: bit-exact. So is every layout variant (strides, a broadcast input, calls queued on a stream, two
objects on two streams) against the dense, synchronised run of the same calls: the arithmetic is the same, only addresses or timing differ."""
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


UL_LOOPBACK = dict(prb=25, cell_id=4, mod=1, tbs=1544, L_prb=10, n_prb=10, nsf=2, tti0=3, srate=5.76e6, fading="eva5")


def ul_loopback_payload():
    u = UL_LOOPBACK
    return np.random.default_rng(12).integers(0, 256, (u["nsf"], u["tbs"] // 8), dtype=np.uint8)


def test_loopback_ul_tx_channel_ul_rx_n128(hp):
    """UlTx -> Channel (EVA5 at the 25-PRB cell's 5.76 MHz: N = 128, no noise) -> UlRx on the device, the receiver's window shifted by
    path_delay. tests/test_channel_host.py::test_ul_loopback_precondition checks on the CPU that the restatement's output for these subframes
    decodes in the oracle's uplink receiver."""
    u = UL_LOOPBACK
    nsf, tbs = u["nsf"], u["tbs"]
    payload = ul_loopback_payload()
    tx = hp.UlTx(u["cell_id"], u["prb"], 0x1234, u["mod"], tbs, u["L_prb"], u["n_prb"], 0, nsf)
    sf_len = tx.sf_len
    assert u["mod"] == hp.MOD_QPSK and sf_len * 1000 == u["srate"]
    x = np.zeros((nsf + 1, sf_len), np.complex64)  # one zero subframe behind the signal for the filter's delay
    x[:nsf] = tx.encode(payload, u["tti0"])
    d_in = hp.DevBuf.from_host(x)
    ch = _mk(hp, u["srate"], 1, nsf + 1, sf_len, fading=u["fading"])
    assert ch.fft_size == 128 and ch.path_delay == 32
    d_out = hp.DevBuf(d_in.nbytes)
    hp._check(ch.run_dev(d_in, d_out, nsf + 1, sf_len), "channel_run_batch")
    rx = hp.UlRx(u["cell_id"], u["prb"], 0x1234, u["mod"], tbs, u["L_prb"], u["n_prb"], 0, 6, nsf)
    hp._check(hp.lib().srslte_hip_ul_rx_batch(rx.h, d_out.ptr + 8 * ch.path_delay, u["tti0"], nsf, rx.d_tb.ptr, rx.tb_stride, rx.d_ok.ptr, None),
              "ul_rx_batch")
    hp.sync()
    tb = rx.d_tb.to_host(np.uint8).reshape(rx.rows, rx.tb_stride)[:nsf, :tbs // 8]
    ok = rx.d_ok.to_host(np.uint8)[:nsf]
    assert ok.all() and np.array_equal(tb, payload)
    for o in (tx, rx, ch):
        o.free()


# ---------------------------------------------------------------- the 128- and 256-point filters
def test_fading_n128_short_last_segment_overlap_across_calls(hp, golden):
    """7.68 MHz eva5: three radix-4 passes and the closing radix-2 pass, 64 threads for 32 butterflies."""
    assert hp.channel_fft_size_for(hp.CHANNEL_FADING_EVA, 7.68e6) == 128 == int(golden["fading_eva5_n128.N"])
    _check_case(hp, golden, "fading_eva5_n128")


def test_fading_n256_nine_taps_blocks_shorter_than_a_segment(hp, golden):
    assert hp.channel_fft_size_for(hp.CHANNEL_FADING_ETU, 7.68e6) == 256 == int(golden["fading_etu70_n256.N"])
    _check_case(hp, golden, "fading_etu70_n256")


# ---------------------------------------------------------------- layouts
PAT, PAD, TAIL = 0xA5, 1e30, 16


def _layout(nch, nb, length, cs, bs):
    """The sample index of [channel][call][n] in a buffer with (channel, call) strides cs, bs."""
    return np.arange(nch)[:, None, None] * cs + np.arange(nb)[None, :, None] * bs + np.arange(length)[None, None, :]


def _run_layout(hp, ch, x, full, frac, in_strides=None, out_strides=None, stream=None):
    """One call. x [channels or 1][nb][len] is laid out by in_strides (channel, call) in a buffer whose padding holds PAD, a large finite value: a
    kernel that reads padding gives a visibly wrong sample. The output buffer is prefilled with PAT bytes and laid out by out_strides. -> the
    payload [channels][nb][len], after asserting that every byte outside it still holds the pattern."""
    nch = ch.cfg.nof_channels
    _, nb, length = x.shape
    ins, outs = in_strides or (nb * length, length), out_strides or (nb * length, length)
    i_idx, o_idx = _layout(x.shape[0], nb, length, *ins), _layout(nch, nb, length, *outs)
    src = np.full(int(i_idx.max()) + 1 + TAIL, PAD + 1j * PAD, np.complex64)
    src[i_idx] = x
    d_in, d_out = hp.DevBuf.from_host(src), hp.DevBuf(8 * (int(o_idx.max()) + 1 + TAIL))
    hp._check(hp.lib().srslte_hip_memset(d_out.ptr, PAT, d_out.nbytes), "memset")
    hp.sync()
    hp._check(ch.run_dev(d_in, d_out, nb, length, full, frac, in_strides=ins, out_strides=outs, stream=stream), "channel_run_batch")
    if stream is None:
        hp.sync()
    else:
        hp._check(hp.lib().srslte_hip_stream_sync(stream), "stream_sync")
    got = d_out.to_host(np.complex64)
    untouched = np.ones(got.size, bool)
    untouched[o_idx] = False
    assert (got.view(np.uint8).reshape(-1, 8)[untouched] == PAT).all(), "bytes outside the payload were written"
    return got[o_idx]


_CHAIN = {k: CASES["chain"][k] for k in ("fading", "delay", "hst", "rlf")}
LAYOUT_CONFIGS = {
    # name -> srate, len, the first call's time, stages, N, whether the device equals the restatement bit for bit (a copy)
    "fading_n128": (7.68e6, 700, (3, 0.5), dict(fading="eva5"), 128, False),
    "delay": (1.92e6, 240, (0, 0.1), dict(delay=(10.0, 100.0, 1.0, 0.0)), 0, True),
    "chain_awgn": (1.92e6, 480, (0, 0.0495), dict(awgn=(0.05, 11), **_CHAIN), 64, False),
}


def _two_calls(srate, length, t0, nb=3):
    return [t0, R.block_time(*t0, nb, length, int(srate))]


@pytest.mark.parametrize("name", sorted(LAYOUT_CONFIGS))
def test_padded_strides_are_bit_identical_to_the_dense_layout(hp, name):
    """Two channels, two successive calls of three blocks (the second reads the overlap and the delay history that ch_carry_kernel stored from
    the strided input): dense against the restatement; then input and output with different, padded strides on both axes against the dense run."""
    srate, length, t0, stages, n, exact = LAYOUT_CONFIGS[name]
    nch, nb = 2, 3
    rng = np.random.default_rng(21)
    xs = [_noise(rng, (nch, nb, length)) for _ in range(2)]
    ch = _mk(hp, srate, nch, nb, length, **stages)
    ref = R.ChannelRef(srate, nch, **stages)
    assert ch.fft_size == n
    dense = []
    for x, (full, frac) in zip(xs, _two_calls(srate, length, t0)):
        dense.append(ch.run(x, full, frac))
        want = ref.run(x, full, frac)
        e = _err(dense[-1], want)
        print("%s dense vs restatement: %.3g" % (name, e))
        assert np.array_equal(dense[-1], want.astype(np.complex64)) if exact else e <= TOL
    ch.reset()
    ins, outs = (nb * (length + 13) + 5, length + 13), (nb * (length + 7) + 3, length + 7)
    for x, (full, frac), want in zip(xs, _two_calls(srate, length, t0), dense):
        got = _run_layout(hp, ch, x, full, frac, ins, outs)
        print("%s padded vs dense: %d samples differ" % (name, int((got != want).sum())))
        assert got.tobytes() == want.tobytes()
    ch.free()


def test_broadcast_input_one_signal_over_three_channels(hp):
    """in_ch_stride = 0: one transmitted signal faded over three channels (N = 128) equals the dense run on the signal replicated."""
    nch, nb, length = 3, 3, 700
    rng = np.random.default_rng(22)
    xs = [_noise(rng, (1, nb, length)) for _ in range(2)]
    ch = _mk(hp, 7.68e6, nch, nb, length, fading="eva5")
    ref = R.ChannelRef(7.68e6, nch, fading="eva5")
    assert ch.fft_size == 128
    dense = []
    for x, (full, frac) in zip(xs, _two_calls(7.68e6, length, (3, 0.5))):
        rep = np.repeat(x, nch, axis=0)
        dense.append(ch.run(rep, full, frac))
        e = _err(dense[-1], ref.run(rep, full, frac))
        print("replicated input vs restatement: %.3g" % e)
        assert e <= TOL
    assert not np.array_equal(dense[0][0], dense[0][1])  # the channels differ: each has its own coefficients
    ch.reset()
    for x, (full, frac), want in zip(xs, _two_calls(7.68e6, length, (3, 0.5)), dense):
        got = _run_layout(hp, ch, x, full, frac, in_strides=(0, length))
        print("broadcast vs replicated: %d samples differ" % int((got != want).sum()))
        assert got.tobytes() == want.tobytes()
    ch.free()


# ---------------------------------------------------------------- calls in flight
def test_nine_calls_queued_on_one_stream_without_a_host_sync(hp):
    """More calls in flight than the descriptor ring has slots: nine one-block calls back to back on a created stream, one synchronisation at the
    end, against the restatement and, bit for bit, against the same calls synchronised one by one. The delay changes between the calls."""
    L = hp.lib()
    nch, ncalls, length, srate = 2, 9, 700, 7.68e6
    stages = dict(fading="eva5", delay=(10.0, 100.0, 1.0, 0.0), awgn=(0.01, 7))
    x = _noise(np.random.default_rng(23), (nch, ncalls, length))
    times = [R.block_time(0, 0.0, i, length, int(srate)) for i in range(ncalls)]
    ref = R.ChannelRef(srate, nch, **stages)
    want = np.concatenate([ref.run(x[:, i:i + 1], *t) for i, t in enumerate(times)], 1)
    assert len({t[0] for t in ref.trace}) >= 3 and max(t[0] for t in ref.trace) <= length
    d_in = hp.DevBuf.from_host(x)
    strides = (ncalls * length, length)
    st = L.srslte_hip_stream_create()
    assert st
    res = []
    for sync_each in (False, True):
        ch = _mk(hp, srate, nch, 1, length, **stages)
        d_out = hp.DevBuf(x.nbytes)
        hp._check(L.srslte_hip_memset(d_out.ptr, PAT, d_out.nbytes), "memset")
        hp.sync()
        for i, (full, frac) in enumerate(times):
            vin, vout = hp.DevView(d_in.ptr + 8 * i * length, 8 * length), hp.DevView(d_out.ptr + 8 * i * length, 8 * length)
            assert ch.run_dev(vin, vout, 1, length, full, frac, in_strides=strides, out_strides=strides, stream=st) == hp.SRSLTE_SUCCESS
            if sync_each:
                assert L.srslte_hip_stream_sync(st) == 0
        assert L.srslte_hip_stream_sync(st) == 0
        res.append(d_out.to_host(np.complex64).reshape(x.shape))
        ch.free()
    L.srslte_hip_stream_destroy(st)
    e = _err(res[0], want)
    print("nine queued calls vs restatement: %.3g; vs the synchronised run: %d samples differ" % (e, int((res[0] != res[1]).sum())))
    assert e <= TOL
    assert res[0].tobytes() == res[1].tobytes()


def test_two_objects_on_two_streams(hp):
    """Two objects with different configurations, their calls interleaved three times round on a stream each: each output equals its solo run."""
    L = hp.lib()
    rng = np.random.default_rng(24)
    specs = [(7.68e6, 2, 700, (3, 0.5), dict(fading="eva5", delay=(10.0, 20.0, 1.0, 0.0))),
             (1.92e6, 1, 480, (1, 0.7995), dict(fading="etu70", hst=(750.0, 7.2, 0.0), awgn=(0.05, 11)))]
    nb, rounds = 2, 3
    objs, xs, times, solo = [], [], [], []
    for srate, nch, length, t0, stages in specs:
        ch = _mk(hp, srate, nch, nb, length, **stages)
        x = [_noise(rng, (nch, nb, length)) for _ in range(rounds)]
        t = [R.block_time(*t0, r * nb, length, int(srate)) for r in range(rounds)]
        solo.append([ch.run(x[r], *t[r]) for r in range(rounds)])
        ch.reset()
        objs.append(ch), xs.append(x), times.append(t)
    assert objs[0].fft_size == 128 and objs[1].fft_size == 64
    streams = [L.srslte_hip_stream_create() for _ in objs]
    bufs = [[(hp.DevBuf.from_host(x[r]), hp.DevBuf(x[r].nbytes)) for r in range(rounds)] for x in xs]
    for r in range(rounds):
        for ch, x, t, st, b in zip(objs, xs, times, streams, bufs):
            assert ch.run_dev(b[r][0], b[r][1], nb, x[r].shape[2], *t[r], stream=st) == hp.SRSLTE_SUCCESS
    for st in streams:
        assert L.srslte_hip_stream_sync(st) == 0
    for k, (b, x, want) in enumerate(zip(bufs, xs, solo)):
        for r in range(rounds):
            got = b[r][1].to_host(np.complex64).reshape(x[r].shape)
            print("object %d round %d vs its solo run: %d samples differ" % (k, r, int((got != want[r]).sum())))
            assert got.tobytes() == want[r].tobytes()
    for st in streams:
        L.srslte_hip_stream_destroy(st)
    for ch in objs:
        ch.free()


# ---------------------------------------------------------------- channel and block counts, block-length edges
def test_five_channels_four_blocks_nine_taps_n256(hp):
    """etu70 at 7.68 MHz (N = 256, nine taps), every channel against the restatement built with that channel's own seed."""
    nch, nb, length, seed0, stride = 5, 4, 300, 7, 0x1234
    x = _noise(np.random.default_rng(25), (nch, nb, length))
    ch = hp.Channel(hp.channel_cfg(7.68e6, nch, nb, length, fading="etu70", seed0=seed0, seed_stride=stride))
    assert ch.fft_size == 256
    y = ch.run(x, 2, 0.25)
    for c in range(nch):
        one = R.ChannelRef(7.68e6, 1, fading="etu70", seed0=seed0 + c * stride)
        for mine, theirs in zip(ch.coeffs(c), (one.fading[0].a, one.fading[0].w, one.fading[0].p)):
            assert len(mine) == 9 and np.array_equal(mine, theirs)
        e = _err(y[c], one.run(x[c:c + 1], 2, 0.25)[0])
        print("channel %d of %d (seed %#x): %.3g" % (c, nch, seed0 + c * stride, e))
        assert e <= TOL
    ch.free()


@pytest.mark.parametrize("length", [1, 15, 16, 17, 63, 64, 65])
def test_block_lengths_around_a_segment_and_the_filter(hp, length):
    """epa5 at 1.92 MHz (N = 64, segments of 16): blocks of one sample (the gather walks more than N blocks back), just below, at and above N / 4
    and N; streams of at least 3 N samples per call, then a second call of the same shape."""
    nb = -(-200 // length)
    assert nb * length >= 3 * 64
    rng = np.random.default_rng(26)
    ch = _mk(hp, 1.92e6, 1, nb, length, fading="epa5")
    ref = R.ChannelRef(1.92e6, 1, fading="epa5")
    assert ch.fft_size == 64
    for full, frac in _two_calls(1.92e6, length, (0, 0.3), nb):
        x = _noise(rng, (1, nb, length))
        e = _err(ch.run(x, full, frac), ref.run(x, full, frac))
        print("len %d, %d blocks: %.3g" % (length, nb, e))
        assert e <= TOL
    ch.free()


def test_block_exactly_as_long_as_its_delay_and_a_refusal_moves_no_state(hp):
    """The recorded delay case's configuration at its maximum of 192 samples: two blocks of exactly 192 samples behind an ordinary call are bit-exact;
    the same call one sample shorter is refused, and the valid call after the refusal equals the one of a run that never made it."""
    stages = dict(delay=CASES["delay"]["delay"])
    srate, t_max = CASES["delay"]["srate"], (0, 0.25)
    rng = np.random.default_rng(27)
    x0, x1 = _noise(rng, (1, 1, 240)), _noise(rng, (1, 2, 192))
    ref = R.ChannelRef(srate, 1, **stages)
    want = [ref.run(x0, 0, 0.1), ref.run(x1, *t_max)]
    assert [t[0] for t in ref.trace[1:]] == [192, 192] and 0 < ref.trace[0][0] < 192
    ch = _mk(hp, srate, 1, 2, 240, **stages)
    plain = [ch.run(x0, 0, 0.1), ch.run(x1, *t_max)]
    for got, w in zip(plain, want):
        assert np.array_equal(got, w.astype(np.complex64))
    ch.reset()
    first = ch.run(x0, 0, 0.1)
    short = hp.DevBuf.from_host(x1[:, :, :191])
    assert ch.run_dev(short, hp.DevBuf(short.nbytes), 2, 191, *t_max) == hp.SRSLTE_ERROR_INVALID_INPUTS
    after = ch.run(x1, *t_max)
    hp.sync()
    ch.free()
    assert first.tobytes() == plain[0].tobytes() and after.tobytes() == plain[1].tobytes()


def test_a_rate_beyond_the_largest_filter_is_refused_at_create(hp):
    found = [(m, r) for m in (hp.CHANNEL_FADING_EPA, hp.CHANNEL_FADING_EVA, hp.CHANNEL_FADING_ETU) for r in (30.72e6, 61.44e6, 92.16e6)
             if hp.channel_fft_size_for(m, r) > 1024]
    assert found
    for model, srate in found:
        h = hp.C.c_void_p()
        cfg = hp.channel_cfg(srate, 1, 1, 1920, fading=(model, 70.0))
        assert hp.lib().srslte_hip_channel_create(hp.C.byref(h), hp.C.byref(cfg)) == hp.SRSLTE_ERROR_INVALID_INPUTS and not h.value
        print("model %d at %.2f MHz: N = %d, refused at create" % (model, srate / 1e6, hp.channel_fft_size_for(model, srate)))


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
