"""The host side of the tracked synchronisation (no device): srslte_hip_sync_tracks_check, srslte_hip_cell_search_decide_ft against
get_cell of ue_cell_search.c restated in tests/sync_track_ref.py, and the layouts of the structs."""
import ctypes as C
import importlib

import numpy as np

import sync_track_ref as st

pkg = importlib.import_module("srslte-emane_amd")
INVALID = -2
N, MO, STRIDE = 128, 9600, 9728


def test_struct_sizes():
    assert C.sizeof(pkg.SyncRes) == 64 and C.sizeof(pkg.SyncTrackRes) == 96 and pkg.SyncTrackRes.r.offset == 0
    assert pkg.SyncTrackRes.frame_type.offset == 64 and pkg.SyncTrackRes.M_ext_avg.offset == 92
    assert C.sizeof(pkg.SyncTrackState) == 64 and C.sizeof(pkg.SyncTrackItem) == 16 and C.sizeof(pkg.SyncTracksCfg) == 12


def test_tracks_check():
    cfg = pkg.sync_cfg(N, MO, MO, max_items=4)
    tc = pkg.SyncTracksCfg(4, 0.0, pkg.FRAME_DETECT)
    mk = pkg.SyncTrackItem.make
    assert pkg.sync_tracks_check(cfg, tc, STRIDE, [mk(t, t % 3) for t in range(4)]) == 0
    assert pkg.sync_tracks_check(cfg, tc, STRIDE, []) == 0
    assert pkg.sync_tracks_check(cfg, tc, STRIDE, [mk(3, 2, 0, 167)]) == 0
    for items in ([mk(1, 0), mk(1, 1)], [mk(4, 0)], [mk(0, 3)], [mk(0, 0, 0, 168)], [mk(0, 0, 1)], [mk(t, 0) for t in range(4)] + [mk(0, 0)]):
        assert pkg.sync_tracks_check(cfg, tc, STRIDE, items) == INVALID, [(i.track, i.N_id_2, i.find_offset, i.N_id_1) for i in items]
    ok = [mk(0, 0)]
    assert pkg.sync_tracks_check(cfg, tc, STRIDE - 3, ok) == INVALID  # the last possible peak's stages would read past the item
    assert pkg.sync_tracks_check(cfg, tc, STRIDE - 2, ok) == 0
    assert pkg.sync_tracks_check(cfg, tc, MO - 1, ok) == INVALID
    for bad in (pkg.SyncTracksCfg(0, 0.0, 0), pkg.SyncTracksCfg(65536, 0.0, 0), pkg.SyncTracksCfg(4, 0.0, 3), pkg.SyncTracksCfg(4, -0.5, 0),
                pkg.SyncTracksCfg(4, float("nan"), 0)):
        assert pkg.sync_tracks_check(cfg, bad, STRIDE, ok) == INVALID
    assert pkg.sync_tracks_check(cfg, pkg.SyncTracksCfg(65535, 1.0, 1), STRIDE, ok) == 0
    assert pkg.sync_tracks_check(pkg.sync_cfg(N, MO, MO, tdd=True), tc, STRIDE, ok) == INVALID  # cfg.tdd stays refused
    assert pkg.sync_tracks_check(cfg, pkg.SyncTracksCfg(2, 0.0, 0), STRIDE, [mk(0, 0), mk(1, 0), mk(1, 2)]) == INVALID
    # the tracking branch: find_offset + max_offset + fft_size samples have to lie in the item
    trk = pkg.sync_cfg(N, 1920, 32, max_items=2)
    assert pkg.sync_tracks_check(trk, tc, 1920, [mk(0, 0, 1920 - 32 - N)]) == 0
    assert pkg.sync_tracks_check(trk, tc, 1920, [mk(0, 0, 1920 - 32 - N + 1)]) == INVALID


def _row(ret, cell_id, cp, ft, corr_peak=1.0, peak_value=3.0, cfo=0.1):
    r = pkg.SyncTrackRes()
    r.r.ret, r.r.cell_id, r.r.cp, r.r.corr_peak, r.r.peak_value, r.r.cfo = ret, cell_id, cp, corr_peak, peak_value, cfo
    r.frame_type = ft
    return r


def test_cell_search_decide_ft_against_get_cell():
    rng = np.random.default_rng(11)
    for trial in range(200):
        n = int(rng.integers(0, 12))
        rows = [_row(int(rng.choice([0, 1, 1, 1, 2])), int(rng.choice([-1, 7, 7, 7, 301, 12])), int(rng.integers(0, 2)), int(rng.integers(0, 2)),
                     float(rng.uniform(0.1, 5)), float(rng.uniform(1, 9)), float(rng.uniform(-0.5, 0.5))) for _ in range(n)]
        cnt, out, ft = pkg.cell_search_decide_ft(rows)
        n_ref, want = st.get_cell_ft(rows)
        assert cnt == n_ref, trial
        if n_ref == 0:
            assert (out.cell_id, out.nof_frames, ft) == (0, 0, 0)
            continue
        assert (out.cell_id, out.cp, ft, out.nof_frames) == (want["cell_id"], want["cp"], want["frame_type"], want["nof_frames"]), trial
        assert abs(out.peak - want["peak"]) <= 1e-6 * want["peak"] and out.mode == np.float32(want["mode"])
        assert out.psr == np.float32(want["psr"]) and abs(out.cfo - want["cfo"]) <= 1e-3
        cnt0, out0 = pkg.cell_search_decide([r.r for r in rows])  # the old helper over the first 16 words says the same
        assert cnt0 == cnt and (out0.cell_id, out0.cp) == (out.cell_id, out.cp)
    # the majority rule: FDD needs more than the integer half of the winning id's rows
    assert pkg.cell_search_decide_ft([_row(1, 7, 0, 0), _row(1, 7, 0, 1)])[2] == 1
    assert pkg.cell_search_decide_ft([_row(1, 7, 0, 0), _row(1, 7, 0, 1), _row(1, 7, 0, 0)])[2] == 0
    assert pkg.cell_search_decide_ft([_row(1, 7, 0, 1), _row(1, 9, 0, 0), _row(1, 9, 0, 0), _row(1, 7, 0, 1), _row(1, 7, 0, 0)])[2] == 1


def test_restatement_first_call_is_find_one():
    """A fresh FDD Track is sync_ref.find_one: the bridge between the stateless restatement and the tracked one."""
    import sync_ref as sr
    rng = np.random.default_rng(3)
    cfg = {k: getattr(pkg.sync_cfg(N, STRIDE, MO, cfo_cp_enable=True, cfo_pss_enable=True, pss_filt_enable=True, sss_alg=1, threshold=2.0,
                                   cfo_cp_nsymbols=14, ema_alpha=0.3), k) for k, _ in pkg.SyncCfg._fields_}
    x = sr.awgn(sr.ofdm_frame(77, False, N, 7, rng)[500:500 + STRIDE], 10.0, rng)
    a, b = sr.find_one(x, cfg, 77 % 3), st.Track(cfg).find(x, 77 % 3)
    for k in sr.DISCRETE:
        assert a[k] == b[k], k
    for k in sr.FLOATS:
        assert a[k] == b[k], k
    assert b["nof_calls"] == 1 and b["frame_type"] == 0 and a["ret"] == 1 and a["cell_id"] == 77
