"""NB-IoT synchronisation, host side (no device): what srslte_hip_nbiot_sync_check / srslte_hip_nbiot_nsss_check refuse, the RE index helpers
against a direct restatement of srslte_npss_put_subframe / srslte_nsss_put_subframe, the host sequences and replicas against the float64
restatement, and the cap on the share of parity items the GPU test may leave out for a small margin."""
import importlib

import numpy as np
import pytest

import nbiot_sync_ref as nr

pkg = importlib.import_module("srslte-emane_amd")
INVALID = -2
It = pkg.NbiotNpssItem


def test_check_accepts_the_plain_cases():
    c = pkg.nbiot_sync_cfg(3840, max_items=4, n_tracks=4)
    assert pkg.nbiot_sync_check(c, 3840, []) == 0
    assert pkg.nbiot_sync_check(c, 3840, [It(0, 0), It(3, 0)]) == 0
    assert pkg.nbiot_sync_check(c, 4000, [It(1, 160)]) == 0
    assert pkg.nbiot_nsss_check(c, 3840, [-1, 0, 503]) == 0
    s = pkg.nbiot_sync_cfg(64, max_items=1)
    assert pkg.nbiot_sync_check(s, 64 + 127, [It(0, 0)]) == 0


@pytest.mark.parametrize("kw", [dict(fft_size=64), dict(fft_size=256), dict(frame_size=0), dict(frame_size=307201), dict(max_items=0),
                                dict(max_items=8192), dict(n_tracks=0), dict(n_tracks=65536), dict(threshold=-1.0), dict(nsss_threshold=-1.0),
                                dict(npss_ema_alpha=-0.1), dict(cfo_ema_alpha=float("nan")), dict(max_offset=0)])
def test_check_refuses_the_configuration(kw):
    a = dict(frame_size=3840, max_items=2, n_tracks=2)
    a.update(kw)
    c = pkg.nbiot_sync_cfg(a.pop("frame_size"), **a)
    assert pkg.nbiot_sync_check(c, 1 << 20, []) == INVALID
    assert pkg.nbiot_nsss_check(c, 1 << 20, []) == INVALID


def test_check_refuses_the_items():
    c = pkg.nbiot_sync_cfg(3840, max_items=3, n_tracks=3)
    assert pkg.nbiot_sync_check(c, 3840, [It(0, 0), It(0, 0)]) == INVALID          # a track named twice
    assert pkg.nbiot_sync_check(c, 3840, [It(3, 0)]) == INVALID                    # track >= n_tracks
    assert pkg.nbiot_sync_check(c, 3840, [It(0, 0)] * 4) == INVALID                # more than max_items
    assert pkg.nbiot_sync_check(c, 3840, [It(0, 1)]) == INVALID                    # find_offset + frame_size > in_stride
    assert pkg.nbiot_sync_check(c, 3839, [It(0, 0)]) == INVALID                    # the CFO stage reads the item up to frame_size
    assert pkg.nbiot_sync_check(c, 1 << 33, [It(0, 0xFFFFFFFF)]) == INVALID        # no wrap-around in the sum
    s = pkg.nbiot_sync_cfg(64, max_items=1)
    assert pkg.nbiot_sync_check(s, 64 + 126, [It(0, 0)]) == INVALID                # the short branch reads 127 samples past the frame
    assert pkg.nbiot_nsss_check(c, 3840, [504]) == INVALID
    assert pkg.nbiot_nsss_check(c, 3840, [-2]) == INVALID
    assert pkg.nbiot_nsss_check(c, 3839, [0]) == INVALID
    assert pkg.nbiot_nsss_check(c, 3840, [0, 1, 2, 3]) == INVALID


def test_nout_follows_the_reference_lengths():
    assert pkg.nbiot_npss_nout(3840) == 3840 + 1508 - 2 == nr.nout(3840)
    assert pkg.nbiot_npss_nout(128) == 128 + 1508 - 2
    assert pkg.nbiot_npss_nout(127) == 126 == nr.nout(127)
    assert pkg.nbiot_npss_nout(64) == 63


def test_nout_at_the_edges_of_both_branches():
    """frame_size - 1 below 128 (0 at frame_size 1, and 0 for the refused frame_size 0, not a wrap to 2^32 - 1), frame_size + 1506 from 128 up
    to the bound."""
    for fs, want in ((1, 0), (2, 1), (127, 126), (128, 1634), (307200, 308706), (0, 0)):
        assert pkg.nbiot_npss_nout(fs) == want, fs
        if fs:
            assert nr.nout(fs) == want and nr.conv_len(fs) == want + 1


def test_check_stride_rule_on_either_side_of_the_branch_switch():
    """The short branch's last dot product reads 127 samples past the frame: find_offset + frame_size + 127 <= in_stride at 127; at 128, the
    long branch, find_offset + frame_size is enough."""
    s = pkg.nbiot_sync_cfg(127, max_items=1)
    assert pkg.nbiot_sync_check(s, 127 + 127, [It(0, 0)]) == 0
    assert pkg.nbiot_sync_check(s, 127 + 126, [It(0, 0)]) == INVALID
    assert pkg.nbiot_sync_check(s, 9 + 127 + 127, [It(0, 9)]) == 0
    assert pkg.nbiot_sync_check(s, 9 + 127 + 126, [It(0, 9)]) == INVALID
    c = pkg.nbiot_sync_cfg(128, max_items=1)
    assert pkg.nbiot_sync_check(c, 128, [It(0, 0)]) == 0
    assert pkg.nbiot_sync_check(c, 127, [It(0, 0)]) == INVALID
    assert pkg.nbiot_sync_check(c, 9 + 128, [It(0, 9)]) == 0
    assert pkg.nbiot_sync_check(c, 9 + 127, [It(0, 9)]) == INVALID
    assert pkg.nbiot_sync_check(pkg.nbiot_sync_cfg(307200), 307200, [It(0, 0)]) == 0
    assert pkg.nbiot_sync_check(pkg.nbiot_sync_cfg(307201), 307201, [It(0, 0)]) == INVALID


def test_self_consistency_rule_has_teeth():
    """nbiot_sync_ref.self_consistent, the rule the GPU edge tests hold every device row to, on a row of the restatement itself: it accepts the
    row's own answers and names a later one of two equal maxima, a value one ulp off, a ratio 2^-22 off and a wrong decision."""
    fs = 255
    w = nr.npss_find(nr.edge_noise(fs, 1)[0], dict(nr.EDGE_CFG, frame_size=fs), nr.new_track(fs))
    row = w["avg"].astype(np.float32)
    row[40] = row[900] = 2 * row.max()  # two equal maxima: the first counts
    val = np.float32(nr.psr(row.astype(np.float64), 40, nr.conv_len(fs)))
    assert nr.self_consistent(row, (0, 40, val, row[40]), fs, 5.0) is None
    assert "first maximum" in nr.self_consistent(row, (0, 900, val, row[900]), fs, 5.0)
    assert "corr_peak" in nr.self_consistent(row, (0, 40, val, np.nextafter(row[40], np.float32(0))), fs, 5.0)
    assert "peak_value" in nr.self_consistent(row, (0, 40, val * np.float32(1 + 2.0 ** -21), row[40]), fs, 5.0)
    assert "ret" in nr.self_consistent(row, (1, 40, val, row[40]), fs, 5.0)
    assert nr.self_consistent(np.zeros(0, np.float32), (0, 0, float("nan"), 0.0), 1, 5.0) is None
    assert "peak_value" in nr.self_consistent(np.zeros(0, np.float32), (0, 0, 1.0, 0.0), 1, 5.0)


@pytest.mark.parametrize("nof_prb", [1, 6, 25])
def test_re_helpers_against_the_put_subframe_loops(nof_prb):
    for off in sorted({0, nof_prb // 2, nof_prb - 1}):
        k, want = 3 * nof_prb * 12 + off * 12, []
        for l in range(11):  # npss.c:425-436
            want += [k + 11 * l + n for n in range(11)]
            k += (nof_prb - 1) * 12 + 1
        got = pkg.nbiot_npss_re(nof_prb, off)
        assert got.tolist() == want
        assert got.max() < 14 * 12 * nof_prb and len(set(got.tolist())) == 121
        # every value lands in symbol 3 + l, subcarriers 12 off .. 12 off + 10
        assert np.array_equal(got // (12 * nof_prb), np.repeat(np.arange(3, 14), 11))
        assert np.array_equal(got % (12 * nof_prb), np.tile(12 * off + np.arange(11), 11))
        for nf in (0, 1, 2, 4, 6, 9, 1023):
            k, want = 3 * nof_prb * 12 + off * 12, []
            for l in range(11):  # nsss.c:379-398
                want += [k + 12 * l + n for n in range(12)]
                k += (nof_prb - 1) * 12
            got, first = pkg.nbiot_nsss_re(nof_prb, off, nf)
            assert got.tolist() == want
            assert first == 132 * (int(np.floor(33 / 132.0 * (nf / 2.0))) % 4)
            assert np.array_equal(got // (12 * nof_prb), np.repeat(np.arange(3, 14), 12))
    with pytest.raises(RuntimeError):
        pkg.nbiot_npss_re(nof_prb, nof_prb)
    with pytest.raises(RuntimeError):
        pkg.nbiot_nsss_re(0, 0, 0)


def test_host_sequences_and_replicas_against_the_restatement():
    """The library's float sequences are the restatement's within float rounding, and its replicas (formed through the closed form the device
    tables use) are the restatement's symbol-by-symbol construction."""
    assert np.abs(pkg.nbiot_npss_generate().reshape(11, 11) - nr.npss_seq()).max() < 2e-7
    assert np.abs(pkg.nbiot_npss_replica() - nr.npss_replica()).max() < 2e-7 * np.abs(nr.npss_replica()).max() * 8
    for cid in (0, 1, 125, 126, 251, 252, 377, 378, 503):
        assert np.abs(pkg.nbiot_nsss_generate(cid) - nr.nsss_seq(cid)).max() < 4e-7
        h = nr.nsss_replica(cid)
        assert np.abs(pkg.nbiot_nsss_replica(cid) - h).max() < 4e-7 * np.abs(h).max() * 8
    with pytest.raises(RuntimeError):
        pkg.nbiot_nsss_generate(504)
    # the four theta_f blocks differ only by the rounding of exp(-j 2 pi theta_f n) formed from an integer theta_f in float
    s = nr.nsss_seq(77).reshape(4, 132)
    assert np.abs(s[1:] - s[0]).max() < 1e-3


def test_left_out_cap_of_the_parity_draw():
    """The GPU parity test compares discrete outputs only where the restatement's smallest margin exceeds 10 T and may leave out at most 5 % of
    its rows on that ground. The cap is pinned here, on the same drawn inputs, where no device is needed. One decision is not counted, as in
    the PSS test at large fft_size: a peak whose runner-up within 10 T is its neighbour (the NPSS and NSSS are 11 times oversampled); the GPU
    test then asks the device's position to be within 10 T of the maximum and continues the restatement from there."""
    e = nr.parity_expected()
    T = nr.T
    rows = e["npss_3840"] + e["npss_19200"]
    left = sum(1 for o in rows if not nr.min_margin(o, o["avg"]) > 10 * T)
    near = sum(1 for o in rows if nr.near_tie(o, o["avg"]))
    print("NPSS: %d of %d rows under 10 T, %d more beside a neighbour" % (left, len(rows), near))
    assert left <= 0.05 * len(rows)
    left = sum(1 for o in e["nsss"] if not nr.min_margin(o, o["abs"]) > 10 * T)
    near = sum(1 for o in e["nsss"] if nr.near_tie(o, o["abs"]))
    print("NSSS: %d of %d rows under 10 T, %d more beside a neighbour" % (left, len(e["nsss"]), near))
    assert left <= 0.05 * len(e["nsss"])
