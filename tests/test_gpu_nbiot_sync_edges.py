"""NB-IoT synchronisation on the device at the edges of its kernels (csrc/nbiot_sync.hip): every frame-size branch of the NPSS search and the
sizes beside its switches, peaks in the partial-overlap lags, on the last lag, on lags 0 .. 3 and beside a 256-lag tile seam, the lobe walks over
an all-zero frame, the max_offset and npss_ema_alpha settings, and NSSS peaks in every part of the 84 product tiles.

Three rules, on top of tests/test_gpu_nbiot_sync.py's (whose _step, _cmp_npss and _cmp_nsss are used here; its build_driver by the generator):
  Device self-consistency (nbiot_sync_ref.self_consistent). Every object here runs with npss_ema_alpha >= 1, so after a call the track's row
    is that call's |c|^2. peak_pos is the row's first maximum, corr_peak the row's value there bit for bit, peak_value the walk of
    nbiot_sync_ref.psr on that row within 2^-23 (one float division against float64; NaN where the walk gives NaN), ret the comparison with the
    threshold. No margin is involved, so this holds on EVERY row, the tie-prone sizes included, and pins the tile maxima, the seams and both
    walks exactly.
  Row parity. The device's row agrees with the restatement's over all nout lags within T max(row), T = sync_ref.tol(1508) as in the other file.
  Tie set (nbiot_sync_ref.tie_step). Below some 400 samples the NPSS peak is structurally ambiguous: the replica is eleven copies of one
    symbol up to sign, so |c[n]| repeats every 137 lags. Where the restatement's peak margin is under 10 T the device's position is accepted
    if the restatement's row there is within 10 T of its maximum, at any distance, and the rest is compared from that position; the count of
    such rows is printed. It is used for frame_size < 1507 only. From 1507 on the inputs carry a planted replica
    (nbiot_sync_ref.plant_npss: the replica or the part of it inside the frame at a chosen lag, 0.03 subcarriers off, 10 .. 20 dB), every test
    first asserts on the CPU that the restatement's smallest margin exceeds 10 T, and no row is left out.
The reference's own rows at these edges are in tests/golden/nbiot_sync_edges.npz (tests/test_nbiot_sync_edges_golden.py pins the restatement to
them without a device). The reference driver is not run here: at these transform lengths (1636 .. 3017 points) some of its processes answered
rows that the restatement, the recorded rows and its own other processes contradict (profiles/nbiot_sync/README.md).

Not reached: the LEFT walk's second and later blocks of 256. They need 256 lags left of the peak over which the row never rises towards
lower lags; the NPSS correlation has side lobes every few lags, an all-zero row peaks at lag 0, and no input was found that the restatement
follows."""
import importlib

import numpy as np
import pytest

import nbiot_sync_ref as nr
from test_gpu_nbiot_sync import INVALID, T, _cfgd, _cmp_npss, _cmp_nsss, _step

pkg = importlib.import_module("srslte-emane_amd")
pytestmark = pytest.mark.gpu

NAN = np.complex64(complex(float("nan"), float("nan")))


def _res(g):
    return g.ret, g.peak_pos, g.peak_value, g.corr_peak


def _bits(g):
    return bytes(g)


def _run(tag, q, x, items, tracks, tie, stats):
    """One NPSS call of q on x [n][stride] against the three rules. tracks: the restatement's track per item (updated). tie: the tie set is
    allowed. stats: counters and largest distances, updated. -> (device rows, restatement rows)."""
    rc, got = q.npss_find(x, items)
    assert rc == 0
    cfg = _cfgd(q.cfg)
    fs, thr = cfg["frame_size"], cfg["threshold"] or 5.0
    out = []
    for b, (t, fo) in enumerate(items):
        g = got[b]
        mean, row = q.track(t)
        assert row.size == q.nout == nr.nout(fs)
        err = nr.self_consistent(row, _res(g), fs, thr)
        assert err is None, (tag, b, err)
        if tie:
            w, near = nr.tie_step(x[b], cfg, tracks[b], fo, g.peak_pos)
        else:
            w, near = _step(x[b], cfg, tracks[b], fo, g)
            assert not near, (tag, b)
        stats["rows"] = stats.get("rows", 0) + 1
        stats["from_device"] = stats.get("from_device", 0) + int(near)
        a = w["avg"]
        if a.size and a.max() > 0:
            d = float(np.abs(row - a).max() / a.max())
            stats["row_T"] = max(stats.get("row_T", 0.0), d / T)
            assert d <= T, (tag, b, "row", d)
        else:
            assert not row.any(), (tag, b)
        assert mean == g.mean_cfo
        if not _cmp_npss((tag, b), g, w, near):
            assert tie, (tag, b, "a row of a planted input was left out", w["margins"])
            stats["left"] = stats.get("left", 0) + 1
        out.append(w)
    return got, out


def _report(name, stats):
    print("%s: %d rows, %d compared from the device's position, %d left out for a margin under 10 T, largest row distance %.3f T"
          % (name, stats.get("rows", 0), stats.get("from_device", 0), stats.get("left", 0), stats.get("row_T", 0.0)))


# ---------------------------------------------------------------- 1. NPSS frame sizes
@pytest.mark.parametrize("fs", nr.EDGE_SHORT)
def test_short_branch_sizes(fs):
    """frame_size 1, 2, 3, 127: nout 0, 1, 2, 126; at 1 no value enters the maximum and ntiles is forced to 1. Three noise items with
    find_offset 0, 5, 3, mean_cfo 0.21 on track 1, stride = the largest find_offset + frame_size + 127, NaN behind what an item may read."""
    fos = [0, 5, 3]
    stride = max(fos) + fs + 127
    x = nr.edge_noise(fs, 3, stride)
    for b, fo in enumerate(fos):
        x[b, fo + fs + 127:] = NAN
    stats = {}
    for cfo_enable in (False, True):
        q = pkg.NbiotSync(fs, max_items=3, n_tracks=3, npss_ema_alpha=1.0, cfo_enable=cfo_enable)
        assert q.nout == fs - 1
        assert q.tracks_set_cfo(1, [0.21]) == 0
        tracks = [nr.new_track(fs) for _ in range(3)]
        tracks[1]["mean_cfo"] = float(np.float32(0.21))
        got, want = _run(("short", fs, cfo_enable), q, x, [(b, fos[b]) for b in range(3)], tracks, True, stats)
        for b, g in enumerate(got):
            assert np.isnan(g.cfo) and g.mean_cfo == (np.float32(0.21) if b == 1 else 0.0)
            if fs == 1:  # the documented row of a search over no lag
                assert (g.ret, g.peak_pos, g.corr_peak) == (0, 0, 0.0) and np.isnan(g.peak_value)
            if fs == 2:  # one lag: both side-lobe ranges are empty, the left one answers avg[0], the peak itself
                assert g.peak_pos == 0 and g.peak_value == 1.0 and g.corr_peak > 0 and g.ret == 0
        q.free()
    _report("short %d" % fs, stats)


@pytest.mark.parametrize("fs", nr.EDGE_LONG)
def test_long_branch_small_sizes(fs):
    """The long branch from its smallest size: at 128 the slide kernel's last tile loads up to index 3208 of a circle of L = 1636, most of a
    second turn (at 3840 it is a fifth of one); 285 .. 287 put nout on 1791, 1792, 1793, either side of a tile multiple. Noise items, so the
    tie set applies. Item 3 has find_offset 7."""
    x = nr.edge_noise(fs, 4, fs + 7)
    items = [(0, 0), (1, 0), (2, 0), (3, 7)]
    stats = {}
    for cfo_enable in (False, True):
        q = pkg.NbiotSync(fs, max_items=4, n_tracks=4, npss_ema_alpha=1.0, cfo_enable=cfo_enable)
        assert q.nout == fs + 1506
        assert -(-q.nout // 256) == {128: 7, 129: 7, 255: 7, 256: 7, 257: 7, 285: 7, 286: 7, 287: 8}[fs]
        got, _ = _run(("long", fs, cfo_enable), q, x, items, [nr.new_track(fs) for _ in range(4)], True, stats)
        assert all(np.isnan(g.cfo) for g in got)  # peak_pos + 1499 < frame_size never holds
        q.free()
    _report("long %d" % fs, stats)


@pytest.mark.parametrize("fs", nr.EDGE_PLANTED)
def test_planted_lags_around_the_replica_length(fs):
    """frame_size 1507, 1508, 1509 - shorter than, equal to and longer than the replica - with the peak planted on lags 0, 1, 2 (pl_lb = 0: the
    left range is empty), 3 (the first peak_pos > 2), 7, nout - 1 (the right walk ends at conv_len, the right range is empty), nout - 2 and
    L - 700 (partial overlap before the frame: zero padding and the circular wrap)."""
    x, L = nr.edge_planted(fs), fs + nr.LEN
    n = len(nr.EDGE_LAGS)
    stats = {}
    for cfo_enable in (False, True):
        cfg = dict(nr.PARITY_CFG, frame_size=fs, npss_ema_alpha=1.0, cfo_enable=cfo_enable)
        for b, lag in enumerate(nr.EDGE_LAGS):  # clear inputs, asserted before the device is asked
            w = nr.npss_find(x[b], cfg, nr.new_track(fs))
            assert nr.min_margin(w) > 10 * T and w["peak_pos"] == lag % L, (fs, lag, w["peak_pos"], w["margins"])
        q = pkg.NbiotSync(fs, max_items=n, n_tracks=n, npss_ema_alpha=1.0, cfo_enable=cfo_enable)
        got, want = _run(("planted", fs, cfo_enable), q, x, [(b, 0) for b in range(n)], [nr.new_track(fs) for _ in range(n)], False, stats)
        for b, lag in enumerate(nr.EDGE_LAGS):
            assert got[b].peak_pos == lag % L, (fs, lag, got[b].peak_pos)
            assert np.isnan(got[b].cfo) == (not cfo_enable or lag % L + 1499 >= fs), (fs, lag, got[b].cfo)
        assert got[nr.EDGE_LAGS.index(-3)].peak_pos == q.nout - 1
        q.free()
    assert stats.get("left", 0) == 0 and stats["from_device"] == 0
    _report("planted %d" % fs, stats)


BIG_LAGS = (65537, 64492, -3, 255, 256)


def test_frame_size_66000_takes_the_tile_loop_a_second_time():
    """nout = 67506 is 264 tiles: the decide kernel's loop over the tile maxima runs a second time for tiles 256 .. 263. Peaks planted in tile
    256 (lag 65537), in the last tile (nout - 1), on either side of the first seam (255, 256) and at 64492, the last but a few of the lags that
    enter the CFO stage."""
    fs, n = 66000, len(BIG_LAGS)
    x, L = nr.edge_planted(fs, BIG_LAGS, "big"), fs + nr.LEN
    cfg = dict(nr.PARITY_CFG, frame_size=fs, npss_ema_alpha=1.0)
    for b, lag in enumerate(BIG_LAGS):
        w = nr.npss_find(x[b], cfg, nr.new_track(fs))
        assert nr.min_margin(w) > 10 * T and w["peak_pos"] == lag % L, (lag, w["peak_pos"], w["margins"])
    stats = {}
    q = pkg.NbiotSync(fs, max_items=n, n_tracks=n, npss_ema_alpha=1.0)
    assert q.nout == 67506 and -(-q.nout // 256) == 264
    got, _ = _run("66000", q, x, [(b, 0) for b in range(n)], [nr.new_track(fs) for _ in range(n)], False, stats)
    for b, lag in enumerate(BIG_LAGS):
        assert got[b].peak_pos == lag % L
    assert sum(1 for g in got if g.peak_pos // 256 >= 256) >= 2
    assert got[2].peak_pos == q.nout - 1 and got[2].peak_pos // 256 == 263
    for b in (1, 3, 4):  # inside the CFO stage's entry condition
        assert abs(got[b].cfo - 0.03) < 0.01, (BIG_LAGS[b], got[b].cfo)
    assert np.isnan(got[0].cfo) and np.isnan(got[2].cfo)  # 65537 + 1499 >= frame_size
    assert stats.get("left", 0) == 0
    _report("66000", stats)
    q.free()


def test_frame_size_307200_the_documented_bound():
    """The largest frame create accepts: a peak at 304200, near the CFO stage's limit peak_pos < frame_size - 1499, then a second call on the
    same track planted at L - 5. 307201 is refused by create and by the host check."""
    fs = 307200
    x, L = nr.edge_planted(fs, (304200, -5), "big"), fs + nr.LEN
    stats = {}
    q = pkg.NbiotSync(fs, max_items=1, n_tracks=1, npss_ema_alpha=1.0)
    assert q.nout == fs + 1506
    cfg = _cfgd(q.cfg)
    tr_check, tr = nr.new_track(fs), nr.new_track(fs)
    for b, lag in enumerate((304200, -5)):
        w = nr.npss_find(x[b], cfg, tr_check)
        assert nr.min_margin(w) > 10 * T and w["peak_pos"] == lag % L, (lag, w["peak_pos"], w["margins"])
        got, _ = _run(("307200", lag), q, x[b:b + 1], [(0, 0)], [tr], False, stats)
        assert got[0].peak_pos == lag % L
        if b == 0:
            assert abs(got[0].cfo - 0.03) < 0.01 and got[0].mean_cfo != 0.0
        else:
            assert np.isnan(got[0].cfo)
    assert stats.get("left", 0) == 0
    _report("307200", stats)
    q.free()
    with pytest.raises(RuntimeError):
        pkg.NbiotSync(fs + 1)
    assert pkg.nbiot_sync_check(pkg.nbiot_sync_cfg(fs + 1), fs + 1, []) == INVALID


# ---------------------------------------------------------------- 2. the walks
@pytest.mark.parametrize("fs", [3840, 64])
def test_all_zero_frame(fs):
    """Every lag ties at 0: the first maximum is lag 0, the right walk crosses the whole row (5347 positions at 3840: 21 blocks of 256 on the
    device) and ends at conv_len, both ranges are empty, 0 / 0 is NaN and ret 0. At 3840 the CFO stage is entered and answers the argument of
    0 + 0 j; at 64 it is not. Item 1 has find_offset 50 with noise before its window and NaN behind it."""
    reach = fs + (127 if fs < 128 else 0)
    x = np.zeros((2, reach + 50), np.complex64)
    x[0, reach:] = NAN
    x[1, :50] = nr.edge_noise(64, 1)[0, :50]  # nothing reads these: the window starts at 50, the CFO stage at index 548 of the item
    q = pkg.NbiotSync(fs, max_items=2, n_tracks=2, npss_ema_alpha=1.0)
    # a row of some other frame first, so that the zeros below are this call's
    rc, _ = q.npss_find(nr.edge_noise(64, 2, reach + 50), [(0, 0), (1, 0)])
    assert rc == 0 and q.track(0)[1].any() and q.track(1)[1].any()
    assert q.tracks_set_cfo(0, [0.0, 0.0]) == 0
    rc, got = q.npss_find(x, [(0, 0), (1, 50)])
    assert rc == 0
    cfg = _cfgd(q.cfg)
    for b, fo in enumerate((0, 50)):
        g, w = got[b], nr.npss_find(x[b], cfg, nr.new_track(fs), fo)
        mean, row = q.track(b)
        assert not row.any() and row.size == q.nout
        assert nr.self_consistent(row, _res(g), fs, 5.0) is None
        for o in (g.peak_pos, w["peak_pos"], g.ret, w["ret"], g.corr_peak, w["corr_peak"], g.mean_cfo, w["mean_cfo"], mean):
            assert o == 0
        assert np.isnan(g.peak_value) and np.isnan(w["peak_value"])
        if fs >= 128:
            assert g.cfo == 0 and w["cfo"] == 0
        else:
            assert np.isnan(g.cfo) and np.isnan(w["cfo"])
    q.free()


def test_left_walk_switch_at_peak_three():
    """Rows of 5 lags (frame_size 6) whose shape decides what the left walk answers: a peak on 3 with a bump on 1 (the first peak_pos > 2: the
    left range is avg[:2], where peak_pos <= 2 would answer avg[0]), a peak on 3 that walks down to 1, a peak on 2 (pl_lb = 0: avg[0] although
    avg[1] is larger) and a peak on the last lag. nbiot_sync_ref.EDGE_WALK_SEEDS says how they were picked."""
    fs = nr.EDGE_WALK_FRAME
    x = nr.edge_walk_items()
    cfg = dict(nr.PARITY_CFG, frame_size=fs, npss_ema_alpha=1.0)
    want = [nr.npss_find(xi, cfg, nr.new_track(fs)) for xi in x]
    assert [w["peak_pos"] for w in want] == [3, 3, 2, 4] and all(nr.min_margin(w) > 10 * T for w in want)
    a = want[0]["avg"]
    assert a[1] > max(a[0], a[2], a[4]) and abs(want[0]["peak_value"] - a[3] / a[1]) < 1e-12  # the side lobe is avg[1]
    a = want[2]["avg"]
    assert a[1] > a[0] > max(a[3], a[4]) and abs(want[2]["peak_value"] - a[2] / a[0]) < 1e-12  # the side lobe is avg[0]
    stats = {}
    q = pkg.NbiotSync(fs, max_items=4, n_tracks=4, npss_ema_alpha=1.0)
    got, _ = _run("walk switch", q, x, [(b, 0) for b in range(4)], [nr.new_track(fs) for _ in range(4)], False, stats)
    assert [g.peak_pos for g in got] == [3, 3, 2, 4] and stats.get("left", 0) == 0
    q.free()


def test_one_planted_peak_between_exact_zeros():
    """Noise-free at 3840: the replica at lag 2000 and, in item 1, its last 808 samples at the frame's start (lag L - 700). Outside the
    replica's reach the device's row is exact zeros - the FFT restatement's is not -, so the walks and the side-lobe maxima are compared
    through self-consistency and the rest by parity."""
    fs, lags = 3840, (2000, -700)
    L = fs + nr.LEN
    x = np.stack([nr.plant(nr.npss_replica(), fs, lag, 0.0, None, None) for lag in lags]).astype(np.complex64)
    cfg = dict(nr.PARITY_CFG, frame_size=fs, npss_ema_alpha=1.0)
    for b, lag in enumerate(lags):
        w = nr.npss_find(x[b], cfg, nr.new_track(fs))
        assert nr.min_margin(w) > 10 * T and w["peak_pos"] == lag % L
    stats = {}
    q = pkg.NbiotSync(fs, max_items=2, n_tracks=2, npss_ema_alpha=1.0)
    got, _ = _run("zeros around", q, x, [(0, 0), (1, 0)], [nr.new_track(fs), nr.new_track(fs)], False, stats)
    assert [g.peak_pos for g in got] == [lag % L for lag in lags] and got[0].ret == 1
    row = q.track(0)[1]
    assert not row[:2000 - 1507].any() and not row[2000 + 1508:].any() and row[2000 - 1507] > 0
    assert stats.get("left", 0) == 0
    _report("zeros around", stats)
    q.free()


# ---------------------------------------------------------------- 3. configuration
def test_max_offset_values():
    """max_offset 1, 2, 64, 127, 128, 129 and 500 on one planted frame: the CFO estimate is one of the restatement's candidates, and values
    above 128 count as 128 - the rows of 128, 129 and 500 are equal bit for bit."""
    fs = 3840
    rng = np.random.default_rng(nr.EDGE_SEEDS["walks"])
    x = nr.plant_npss(fs, 1000, rng, snr_db=20.0)[None, :]
    rows, stats = {}, {}
    for mo in (1, 2, 64, 127, 128, 129, 500):
        q = pkg.NbiotSync(fs, max_offset=mo, max_items=1, n_tracks=1, npss_ema_alpha=1.0)
        cfg = _cfgd(q.cfg)
        w = nr.npss_find(x[0], cfg, nr.new_track(fs))
        assert nr.min_margin(w) > 10 * T and w["peak_pos"] == 1000 and len(w["cfo_candidates"]) == 1
        got, _ = _run(("max_offset", mo), q, x, [(0, 0)], [nr.new_track(fs)], False, stats)
        assert abs(got[0].cfo - w["cfo"]) <= T and abs(got[0].cfo - 0.03) < 0.01
        rows[mo] = _bits(got[0])
        q.free()
    assert rows[128] == rows[129] == rows[500]
    assert stats.get("left", 0) == 0
    with pytest.raises(RuntimeError):  # srslte_cp_synch over no offset
        pkg.NbiotSync(fs, max_offset=0)
    q = pkg.NbiotSync(fs, max_offset=0, cfo_enable=False)
    q.free()


def test_ema_alpha_above_one_keeps_no_average():
    """npss_ema_alpha 1.5 is outside 0 < alpha < 1 (npss.c:278): a second call on other input leaves exactly that input's row."""
    fs = 3840
    xa, xb = nr.edge_planted(fs, (500,), "walks"), nr.edge_planted(fs, (-700,), "big")
    stats = {}
    q = pkg.NbiotSync(fs, max_items=1, n_tracks=1, npss_ema_alpha=1.5, cfo_enable=False)
    tr = nr.new_track(fs)
    _run("alpha 1.5, first", q, xa, [(0, 0)], [tr], False, stats)
    first = q.track(0)[1].copy()
    got, want = _run("alpha 1.5, second", q, xb, [(0, 0)], [tr], False, stats)
    fresh = nr.npss_find(xb[0], _cfgd(q.cfg), nr.new_track(fs))
    row = q.track(0)[1]
    assert np.abs(row - fresh["avg"]).max() <= T * fresh["avg"].max() and got[0].peak_pos == fresh["peak_pos"] == fs + nr.LEN - 700
    assert np.abs(row - first).max() > 0.5 * first.max()  # nothing of the first call is left
    assert stats.get("left", 0) == 0
    q.free()


# ---------------------------------------------------------------- 4. NSSS lags
def test_nsss_planted_lags_in_every_part_of_the_product_tiles():
    """Nine ids at the edges of the 64-id product rows (0, 63, 64, 127, 448, 503), around the b_q groups (250, 252) and a drawn one, planted
    at lags 0, 63, 64 (a 64-lag seam), 2332, 3000, 4648 (partial overlap before the capture), 5312 (the first lag of the tail tile, which
    holds 34 lags), 5344 and 5345 (the last), each once with its id given and once exhaustive, in one call of 18 items with in_stride 3840 +
    77 and NaN behind. Position and id are asked exactly."""
    x9, ids, lags = nr.edge_nsss()
    L = nr.NSSS_IN + nr.LEN
    x = np.full((18, nr.NSSS_IN + 77), NAN, np.complex64)
    given = []
    for b in range(9):
        x[2 * b, :nr.NSSS_IN] = x[2 * b + 1, :nr.NSSS_IN] = x9[b]
        given += [ids[b], -1]
    want = [nr.nsss_find(x[i, :nr.NSSS_IN], {}, given[i]) for i in range(18)]
    for i, w in enumerate(want):  # clear inputs
        assert min(w["margins"].values()) > 10 * T and w["peak_pos"] == lags[i // 2] % L and w["cell_id"] == ids[i // 2] and w["found"] == 1, (i, w["margins"])
    q = pkg.NbiotSync(3840, max_items=18)
    rc, got = q.nsss_find(x, given)
    assert rc == 0
    worst = 0.0  # the reference's 18 rows are in tests/golden/nbiot_sync_edges.npz
    for i, (g, w) in enumerate(zip(got, want)):
        pv, row = q.nsss_debug(i)
        assert g.peak_pos == w["peak_pos"] and g.cell_id == w["cell_id"] and g.found == 1, (i, g.peak_pos, g.cell_id, w["peak_pos"], w["cell_id"])
        assert _cmp_nsss(("planted nsss", i), g, w, pv if given[i] < 0 else None, known=given[i] >= 0)
        d = float(np.abs(row - w["abs"]).max() / w["abs"].max())
        worst = max(worst, d)
        assert d <= T, (i, d)
        assert int(np.argmax(row)) == g.peak_pos and abs(row[g.peak_pos] - g.peak_value) <= T * g.peak_value
        if given[i] < 0:
            assert int(np.argmax(pv)) == g.cell_id and pv[g.cell_id] == g.peak_value
        else:
            assert np.count_nonzero(pv) == 1 and pv[given[i]] == g.peak_value
    assert sorted({g.peak_pos // 64 for g in got}) == [0, 1, 36, 46, 72, 83]
    print("planted nsss: 18 rows, 0 left out, largest row distance %.3f T" % (worst / T))
    q.free()
