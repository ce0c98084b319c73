"""float64 restatement of the NB-IoT synchronisation (phy_hip.h "NB-IoT synchronisation") from the reference's own steps: the sequences of
srslte_npss_generate / srslte_nsss_generate, the replicas symbol by symbol through a mirrored inverse transform, CP and the half-subcarrier
table (npss.c:170-239, nsss.c:144-229), the circular correlation through transforms of frame_size + 1508 points, the peak-to-sidelobe walk and
the CFO stage of sync_nbiot.c:189-265. Every decision comes with its relative margin, as in sync_ref.find_one."""
import numpy as np

import sync_ref as sr
from sync_ref import psr  # npss.c:301-343 walks as compute_peak_sidelobe (pss.c:412-441) does

N, LEN, SF = 128, 1508, 1920
CORR_OFFSET = SF - LEN                      # 412
CFO_OFFSET = SF // 2 - CORR_OFFSET          # 548
CFO_NSAMP = 6 * N + 5 * 9 + 10              # 823
NSSS_IN, NUM_PCI = 2 * SF, 504
NPSS_SIGN = np.array([1, 1, 1, 1, -1, -1, 1, 1, 1, -1, 1], float)
T = sr.tol(LEN)


def npss_seq():
    """srslte_npss_generate (npss.c:399-421): [11][11]."""
    n = np.arange(11, dtype=np.float64)
    arg = (-np.pi * 5.0 * (n * (n + 1.0)) / 11.0).astype(np.float32)
    z = np.cos(arg).astype(np.float64) + 1j * np.sin(arg).astype(np.float64)
    return NPSS_SIGN[:, None] * z[None, :]


def b_q(q):
    """36.211 Table 10.2.7.2.1-1: column 0, 31, 63, 127 of the 128-point Hadamard matrix."""
    col = (0, 31, 63, 127)[q]
    return np.array([-1.0 if bin(m & col).count("1") & 1 else 1.0 for m in range(128)])


def nsss_seq(cell_id):
    """srslte_nsss_generate (nsss.c:348-377): the 4 x 132 values; the theta_f factor is exp(-j 2 pi theta_f n) with the integer theta_f."""
    u, q = cell_id % 126 + 3, cell_id // 126
    n = np.arange(132)
    npr = (n % 131).astype(np.float64)
    a2 = (-np.pi * u * npr * (npr + 1.0) / 131.0).astype(np.float32)
    t2 = np.cos(a2).astype(np.float64) + 1j * np.sin(a2).astype(np.float64)
    b = b_q(q)[n % 128]
    out = []
    for th in range(4):
        a1 = (-2.0 * np.pi * th * n.astype(np.float64)).astype(np.float32)
        t1 = np.cos(a1).astype(np.float64) + 1j * np.sin(a1).astype(np.float64)
        out.append(b * t1 * t2)
    return np.concatenate(out)


def shift_sf(freq=0.5):
    """srslte_cexptab_gen_sf (cexptab.c:80-92) for a subframe of 128-point symbols."""
    out = []
    for _ in range(2):
        for i in range(7):
            cpl = 10 if i == 0 else 9
            a = (2 * np.pi * (np.arange(N + cpl, dtype=np.float64) - cpl) * freq / N).astype(np.float32).astype(np.float64)
            out.append(np.exp(1j * a))
    return np.concatenate(out)


def replica(S, k0, scale=1.0):
    """S [11][nsc] at buffer index k0 of each symbol's 128 bins -> the 1508 samples of srslte_npss_corr_init / srslte_nsss_corr_init."""
    out = []
    for i in range(11):
        buf = np.zeros(N, complex)
        buf[k0:k0 + S.shape[1]] = S[i]
        sym = np.fft.ifft(np.fft.ifftshift(buf)) * N / np.sqrt(N)  # mirror, no DC handling, 1 / sqrt(N)
        cpl = 10 if i == 4 else 9
        out.append(np.r_[sym[N - cpl:], sym])
    h = np.concatenate(out)
    assert h.size == LEN
    return h * shift_sf()[CORR_OFFSET:CORR_OFFSET + LEN] * scale


_CACHE = {}


def npss_replica():
    if "npss" not in _CACHE:
        _CACHE["npss"] = replica(npss_seq(), (N - 12) // 2, 1.0 / 3)
    return _CACHE["npss"]


def nsss_replica(cell_id):
    if ("nsss", cell_id) not in _CACHE:
        _CACHE["nsss", cell_id] = replica(nsss_seq(cell_id)[:132].reshape(11, 12), 57)
    return _CACHE["nsss", cell_id]


def _nsss_spectra():
    if "nsss_fft" not in _CACHE:
        L = NSSS_IN + LEN
        _CACHE["nsss_fft"] = np.conj(np.fft.fft(np.array([np.r_[nsss_replica(c), np.zeros(L - LEN)] for c in range(NUM_PCI)]), axis=1))
    return _CACHE["nsss_fft"]


def nout(frame_size):
    """conv_output_len - 1 (npss.c:273-288): srslte_corr_fft_cc_run_opt returns output_len - 1."""
    return frame_size + LEN - 2 if frame_size >= N else frame_size - 1


def circ_corr(x, h, L):
    """c[n] = sum_k x[(n + k) mod L] conj(h[k]) (convolution.c:130-136 with its normalisations)."""
    return np.fft.ifft(np.fft.fft(np.r_[x, np.zeros(L - x.size)]) * np.conj(np.fft.fft(np.r_[h, np.zeros(L - h.size)])))


def cp_symbols():
    """The symbols srslte_cp_synch (cp.c:61-77) walks: 6 of CP 9, the first one sample longer -> [(start, cplen)]."""
    off, out = 0, []
    for n in range(6):
        cpl = 9 + (0 if n % 7 else 1)
        out.append((off, cpl))
        off += N + cpl
    return out


def new_track(frame_size):
    return {"avg": np.zeros(nout(frame_size)), "mean_cfo": 0.0}


def npss_find(x, cfg, track, find_offset=0, force_peak=None):
    """One srslte_sync_nbiot_find on `track` (updated in place). force_peak: take this index as the maximum of the average (for a caller that
    has checked it to be one within its tolerance: the NPSS is 11 times oversampled, so the peak's neighbours are close to it) and go on. x: the item's samples; cfg: dict with frame_size, max_offset, threshold,
    npss_ema_alpha, cfo_ema_alpha, cfo_enable (zeros select the defaults). -> dict with the fields of srslte_hip_nbiot_npss_res_t, "margins",
    "cfo_candidates" (the estimates of every offset whose |corr|^2 is within 10 T of the largest) and "avg"."""
    fs, fo = cfg["frame_size"], find_offset
    thr = np.float32(cfg.get("threshold", 0.0) or 5.0)
    alpha = np.float32(cfg.get("npss_ema_alpha", 0.0) or 0.2)
    ca = np.float32(cfg.get("cfo_ema_alpha", 0.0) or 0.1)
    x = np.asarray(x, complex)
    f = np.float64(np.float32(-np.float32(track["mean_cfo"])) / np.float32(N))
    xr = x * np.exp(2j * np.pi * f * np.arange(x.size))
    h = npss_replica()
    no = nout(fs)
    if fs >= N:
        c = circ_corr(xr[fo:fo + fs], h, fs + LEN)[:no]
        conv_len = fs + LEN - 1
    else:
        c = np.array([np.sum(h[:N] * xr[fo + i:fo + i + N]) for i in range(no)])
        conv_len = fs
    v = np.abs(c) ** 2
    if 0.0 < alpha < 1.0:
        track["avg"] = v * np.float64(alpha) + track["avg"] * np.float64(np.float32(1) - alpha)
    else:
        track["avg"] = v
    avg = track["avg"]
    mg = {}
    pk, mg["peak"] = sr._top2(avg) if avg.size else (0, 1.0)
    if force_peak is not None:
        pk = int(force_peak)
        del mg["peak"]
    o = dict(peak_pos=pk, corr_peak=float(avg[pk]) if avg.size else 0.0, cfo=float("nan"), margins=mg, avg=avg, cfo_candidates=[])
    o["peak_value"] = psr(avg, pk, conv_len)
    if np.isfinite(o["peak_value"]):
        mg["threshold"] = abs(o["peak_value"] - thr) / max(o["peak_value"], thr)
    o["ret"] = 1 if o["peak_value"] >= thr else 0
    if cfg.get("cfo_enable", True) and pk + CFO_OFFSET + CFO_NSAMP + N < fs:
        y = x[pk + CFO_OFFSET:].copy()  # the uncorrected item, not offset by find_offset
        y[:CFO_NSAMP] *= shift_sf()[SF // 2:SF // 2 + CFO_NSAMP]
        M = min(cfg["max_offset"], N)
        corr = np.zeros(M, complex)
        for off, cpl in cp_symbols():
            for i in range(M):
                corr[i] += np.sum(y[off + i:off + i + cpl] * np.conj(y[off + i + N:off + i + N + cpl])) / 6
        p = np.abs(corr) ** 2
        i = int(np.argmax(p))
        o["cfo"] = float(-np.angle(corr[i]) / np.pi / 2)
        o["cfo_candidates"] = [float(-np.angle(corr[k]) / np.pi / 2) for k in np.nonzero(p >= (1 - 10 * T) * p[i])[0]]
        track["mean_cfo"] = float(np.float64(ca) * o["cfo"] + np.float64(np.float32(1) - ca) * track["mean_cfo"])
    o["mean_cfo"] = track["mean_cfo"]
    return o


def nsss_find(x, cfg, cell_id=-1):
    """srslte_nsss_sync_find on the first 3840 samples of x. cell_id -1: all 504. -> dict with the fields of srslte_hip_nbiot_nsss_res_t,
    "margins", "peak_values" (504; 0 for ids that did not run) and "abs" (the |c| row of the row's id)."""
    thr = np.float32(cfg.get("nsss_threshold", 0.0) or 2.0)
    L = NSSS_IN + LEN
    X = np.fft.fft(np.r_[np.asarray(x[:NSSS_IN], complex), np.zeros(LEN)])
    mg = {}
    pv = np.zeros(NUM_PCI)
    if cell_id < 0:
        a = np.abs(np.fft.ifft(X[None, :] * _nsss_spectra(), axis=1))[:, :L - 2]
        pv = a.max(axis=1)
        cid, mg["cell_id"] = sr._top2(pv)
        row = a[cid]
    else:
        cid = cell_id
        row = np.abs(np.fft.ifft(X * np.conj(np.fft.fft(np.r_[nsss_replica(cid), np.zeros(L - LEN)]))))[:L - 2]
        pv[cid] = row.max()
    pos, mg["peak"] = sr._top2(row)
    val = float(row[pos])
    mg["threshold"] = abs(val - thr) / max(val, thr)
    return dict(found=1 if val > thr else 0, cell_id=cid, peak_value=val, peak_pos=pos, sfn_partial=0, margins=mg, peak_values=pv, abs=row)


# ---------------------------------------------------------------- signals
def subframe_time(values, shift):
    """One 1-PRB subframe of 1920 samples carrying `values` [11][nsc] in symbols 3..13 from subcarrier 0 of the PRB, as srslte_ofdm_tx_sf
    modulates it at 128 points (un-normalised transform scaled here by 1 / sqrt(128)). shift: srslte_ofdm_set_freq_shift(+0.5), which also turns
    the DC handling off (ofdm.c:360-377) - subcarrier k at frequency k - 6 + 1/2; otherwise the DC bin is skipped - frequencies -6..-1, 1..6."""
    out = []
    for l in range(14):
        X = np.zeros(N, complex)
        if l >= 3:
            for k in range(values.shape[1]):
                X[(k - 6 if shift or k < 6 else k - 5) % N] = values[l - 3][k]
        sym = np.fft.ifft(X) * N / np.sqrt(N)
        cpl = 10 if l % 7 == 0 else 9
        out.append(np.r_[sym[N - cpl:], sym])
    t = np.concatenate(out)
    return t * shift_sf() if shift else t


def npss_subframe():
    """npss_test.c:108-126: the transmitter with the half-subcarrier shift."""
    return subframe_time(npss_seq(), True)


def nsss_subframe(cell_id, theta_f=0):
    """nsss_test.c:121-178: the transmitter WITHOUT the shift. (With it the signal lies one subcarrier above the replica, which
    srslte_nsss_corr_init places at index 57: in this restatement 24 of 60 drawn ids then come out of a noise-free exhaustive search, against
    60 of 60 as nsss_test transmits.)"""
    return subframe_time(nsss_seq(cell_id)[132 * theta_f:132 * theta_f + 132].reshape(11, 12), False)


def impair(x, cfo_sc, snr_db, rng, ref_power=None):
    """x rotated by cfo_sc subcarriers (of 15 kHz at 128 samples per symbol) plus noise snr_db below ref_power (None: x's mean power)."""
    y = x * np.exp(2j * np.pi * cfo_sc / N * np.arange(x.size))
    if snr_db is None:
        return y
    pw = np.mean(np.abs(x) ** 2) if ref_power is None else ref_power
    s = np.sqrt(pw * 10 ** (-snr_db / 10) / 2)
    return y + s * (rng.normal(size=x.size) + 1j * rng.normal(size=x.size))


SNR_CLASSES = (None, 5.0, -5.0, "noise")


def draw_npss(frame_size, count, seed, stride=None):
    """The parity test's NPSS items: delay anywhere in the frame, CFO within +-0.4 subcarriers, a quarter each noise-free, +5 dB, -5 dB and
    noise only. -> x [count][stride] complex64."""
    rng = np.random.default_rng(seed)
    stride = stride or frame_size
    sf = npss_subframe()
    pw = np.mean(np.abs(sf[CORR_OFFSET:]) ** 2)
    x = np.zeros((count, stride), np.complex64)
    for b in range(count):
        cls = SNR_CLASSES[b % 4]
        sig = np.zeros(frame_size, complex)
        if cls != "noise":
            d = int(rng.integers(0, frame_size - SF + 1))
            sig[d:d + SF] = sf
        cfo = float(rng.uniform(-0.4, 0.4))
        if cls == "noise":
            sig = impair(sig, 0.0, 0.0, rng, ref_power=pw)
        else:
            sig = impair(sig, cfo, cls, rng, ref_power=pw)
        x[b, :frame_size] = sig
    return x


def draw_nsss(count, seed):
    """The parity test's NSSS items: 3840 samples, the NSSS subframe at a drawn delay, the same four classes; even items known, odd unknown.
    -> (x [count][3840] complex64, cell ids given to the call, constructed ids)."""
    rng = np.random.default_rng(seed)
    x = np.zeros((count, NSSS_IN), np.complex64)
    given, made = [], []
    for b in range(count):
        cls = SNR_CLASSES[(b // 2) % 4]
        cid = int(rng.integers(0, NUM_PCI))
        sf = nsss_subframe(cid)
        pw = np.mean(np.abs(sf[CORR_OFFSET:]) ** 2)
        sig = np.zeros(NSSS_IN, complex)
        if cls != "noise":
            d = int(rng.integers(0, NSSS_IN - SF + 1))
            sig[d:d + SF] = sf
            sig = impair(sig, float(rng.uniform(-0.05, 0.05)), cls, rng, ref_power=pw)
        else:
            sig = impair(sig, 0.0, 0.0, rng, ref_power=pw)
        x[b] = sig
        made.append(cid)
        given.append(cid if b % 2 == 0 else -1)
    return x, given, made


NPSS_DISCRETE = ("ret", "peak_pos")
NPSS_FLOATS = {"peak_value": "self", "corr_peak": "self", "mean_cfo": 1.0}


# ---------------------------------------------------------------- the drawn inputs the GPU parity test, the host test and the golden share
SEEDS = dict(npss_3840=20261, npss_19200=20262, nsss=20263, state=20264)
PARITY_CFG = dict(max_offset=128, threshold=0.0, npss_ema_alpha=0.0, cfo_ema_alpha=0.0, cfo_enable=True)
_PARITY = {}


def parity_inputs():
    """-> dict: "npss_3840" x [32][3840], "npss_19200" x [8][19200], "nsss" (x [32][3840], ids given, ids made). Redrawn from SEEDS."""
    if "in" not in _PARITY:
        _PARITY["in"] = dict(npss_3840=draw_npss(3840, 32, SEEDS["npss_3840"]), npss_19200=draw_npss(19200, 8, SEEDS["npss_19200"]),
                             nsss=draw_nsss(32, SEEDS["nsss"]))
    return _PARITY["in"]


def parity_expected():
    """The restatement of every parity item, computed once: "npss_3840" / "npss_19200" -> [npss_find of a fresh track], "nsss" -> [nsss_find]."""
    if "exp" not in _PARITY:
        pin, e = parity_inputs(), {}
        for k, fs in (("npss_3840", 3840), ("npss_19200", 19200)):
            cfg = dict(PARITY_CFG, frame_size=fs)
            e[k] = [npss_find(x, cfg, new_track(fs)) for x in pin[k]]
        x, given, _ = pin["nsss"]
        e["nsss"] = [nsss_find(x[b], {}, given[b]) for b in range(len(given))]
        _PARITY["exp"] = e
    return _PARITY["exp"]


def near_tie(o, row):
    """The decision "peak" of o is within 10 T of a tie and the runner-up of `row` is a neighbour of the peak (within two samples): the
    signals occupy 11 or 12 of 128 bins, so that is the rule beside a peak that falls between two samples, not an accident."""
    if "peak" not in o["margins"] or o["margins"]["peak"] > 10 * T:
        return False
    pk = o["peak_pos"]
    a = np.array(row, float)
    a[pk] = -1.0
    return abs(int(np.argmax(a)) - pk) <= 2


def min_margin(o, row=None):
    """The smallest deciding margin; with `row` (the values "peak" was taken over) a near tie between neighbours does not count."""
    m = dict(o["margins"])
    if row is not None and near_tie(o, row):
        del m["peak"]
    return min(m.values()) if m else 1.0


STATE_FRAME = 3840


def state_script():
    """Three tracks over five calls: track 1 skips call 2, track 2 is reset before call 3, track 0 gets a CFO set before call 4. -> list of
    calls; a call is (ops before it [("reset", track) | ("set_cfo", track, value)], [(track, x [3840] complex64)])."""
    rng = np.random.default_rng(SEEDS["state"])
    sf = npss_subframe()
    pw = np.mean(np.abs(sf[CORR_OFFSET:]) ** 2)
    delay = [int(rng.integers(0, STATE_FRAME - SF + 1)) for _ in range(3)]
    cfo = [float(rng.uniform(-0.3, 0.3)) for _ in range(3)]
    calls = []
    for c in range(5):
        items = []
        for t in range(3):
            if t == 1 and c == 2:
                continue
            sig = np.zeros(STATE_FRAME, complex)
            sig[delay[t]:delay[t] + SF] = sf
            items.append((t, impair(sig, cfo[t], 0.0, rng, ref_power=pw).astype(np.complex64)))
        ops = []
        if c == 3:
            ops.append(("reset", 2))
        if c == 4:
            ops.append(("set_cfo", 0, cfo[0]))
        calls.append((ops, items))
    return calls


def run_state_script(cfg):
    """The restatement run in the script's order -> (rows per call [[npss_find dict]], tracks)."""
    tracks = [new_track(STATE_FRAME) for _ in range(3)]
    rows = []
    for ops, items in state_script():
        for op in ops:
            if op[0] == "reset":
                tracks[op[1]] = new_track(STATE_FRAME)
            else:
                tracks[op[1]]["mean_cfo"] = float(np.float32(op[2]))
        rows.append([npss_find(x, cfg, tracks[t]) for t, x in items])
    return rows, tracks


# ---------------------------------------------------------------- the edge cases the GPU edge test, the generator and the edge golden share
EDGE_SEEDS = dict(short=20271, long=20272, planted=20273, big=20274, nsss=20275, walks=20276)
EDGE_SHORT = (1, 2, 3, 127)
EDGE_LONG = (128, 129, 255, 256, 257, 285, 286, 287)
EDGE_PLANTED = (1507, 1508, 1509)
EDGE_LAGS = (0, 1, 2, 3, 7, -3, -4, -700)
EDGE_NSSS_IDS = (0, 63, 64, 127, 250, 252, 448, 503)
EDGE_NSSS_LAGS = (0, 63, 64, 2332, 3000, -700, -36, -4, -3)


def plant(h, n, lag, cfo_sc, snr_db, rng):
    """n samples that hold the replica h - or the part of it that falls inside - with h[0] at index lag (negative: only the tail is inside, and
    the circular correlation peaks at lag + n + 1508), rotated by cfo_sc subcarriers, plus noise snr_db below the replica's mean power
    (None: noise-free, the samples outside the replica exact zeros)."""
    sig = np.zeros(n, complex)
    a, b = max(lag, 0), min(lag + LEN, n)
    sig[a:b] = h[a - lag:b - lag]
    return impair(sig, cfo_sc, snr_db, rng, ref_power=np.mean(np.abs(h) ** 2))


def plant_npss(frame_size, lag, rng, cfo_sc=0.03, snr_db=15.0):
    return plant(npss_replica(), frame_size, lag, cfo_sc, snr_db, rng).astype(np.complex64)


def edge_noise(frame_size, count, stride=None):
    """Seeded Gaussian items of the short and the tie-prone long frame sizes -> x [count][stride] complex64, all of the stride drawn."""
    rng = np.random.default_rng([EDGE_SEEDS["short" if frame_size < N else "long"], frame_size])
    stride = stride or frame_size
    return (rng.normal(size=(count, stride)) + 1j * rng.normal(size=(count, stride))).astype(np.complex64)


def edge_planted(frame_size, lags=EDGE_LAGS, key="planted"):
    """One item per planted lag -> x [len(lags)][frame_size] complex64; SNR drawn in 10 .. 20 dB."""
    rng = np.random.default_rng([EDGE_SEEDS[key], frame_size])
    return np.stack([plant_npss(frame_size, lag, rng, snr_db=float(rng.uniform(10.0, 20.0))) for lag in lags])


def edge_nsss():
    """The nine planted NSSS captures at 20 dB -> (x [9][3840] complex64, ids, lags)."""
    rng = np.random.default_rng(EDGE_SEEDS["nsss"])
    ids = list(EDGE_NSSS_IDS) + [int(rng.integers(0, NUM_PCI))]
    x = np.stack([plant(nsss_replica(c), NSSS_IN, lag, 0.0, 20.0, rng) for c, lag in zip(ids, EDGE_NSSS_LAGS)]).astype(np.complex64)
    return x, ids, list(EDGE_NSSS_LAGS)


EDGE_CFG = dict(PARITY_CFG, npss_ema_alpha=1.0)
EDGE_GOLDEN_NOISE = (2, 3, 127, 128, 129, 286)


def edge_golden_inputs():
    """The NPSS cases of tests/golden/nbiot_sync_edges.npz, each item for find_offset 0 and a fresh track: name -> (frame_size, x [n][frame_size])."""
    out = {}
    for fs in EDGE_GOLDEN_NOISE:
        out["noise_%d" % fs] = (fs, edge_noise(fs, 3 if fs < N else 4))
    out["planted_1508"] = (1508, edge_planted(1508))
    out["zero_3840"] = (3840, np.zeros((1, 3840), np.complex64))
    return out


EDGE_WALK_FRAME = 6
# noise items at frame_size 6 (5 lags), picked by a search over seeds for the shape of their row a[0..4], every pair of values 20 T apart:
#   53:  peak 3, a[1] above a[0], a[2] and a[4]: the left walk stops at 2 and the left range a[:2] holds the side lobe (peak > 2 taken as <= 2: a[0])
#   412: peak 3, a[2] > a[1] > a[0] > a[4]: the left walk runs down to 1 and the left range is a[:1]
#   144: peak 2, a[1] > a[0] > a[3], a[4]: pl_lb is 0, the empty left range answers a[0], not a[1]
#   1:   peak 4, the last lag, a[3] < a[2]: the left walk stops at once and the right range is empty
EDGE_WALK_SEEDS = (53, 412, 144, 1)


def edge_walk_items():
    """-> x [4][6 + 127] complex64 of EDGE_WALK_SEEDS."""
    out = []
    for seed in EDGE_WALK_SEEDS:
        rng = np.random.default_rng([EDGE_SEEDS["walks"], seed])
        n = EDGE_WALK_FRAME + N - 1
        out.append((rng.normal(size=n) + 1j * rng.normal(size=n)).astype(np.complex64))
    return np.stack(out)


def conv_len(frame_size):
    """conv_output_len of npss.c: nout + 1 in both branches."""
    return frame_size + LEN - 1 if frame_size >= N else frame_size


def tie_step(x, cfg, track, find_offset, dev_pos, Tm=None):
    """The tie set: where the restatement's peak is within 10 Tm of a tie - at ANY distance, as below some 400 samples, where |c| repeats every
    137 lags - a position p with avg[p] >= (1 - 10 Tm) max(avg) is accepted and the restatement is continued from it. dev_pos: the position to
    test. -> (restatement row on `track` (updated), True when the row was continued from dev_pos). Raises AssertionError outside the set."""
    Tm = T if Tm is None else Tm
    before = {"avg": track["avg"].copy(), "mean_cfo": track["mean_cfo"]}
    w = npss_find(x, cfg, track, find_offset)
    if "peak" in w["margins"] and w["margins"]["peak"] <= 10 * Tm:
        a, p = w["avg"], int(dev_pos)
        assert 0 <= p < a.size and a[p] >= (1 - 10 * Tm) * a.max(), (p, w["peak_pos"])
        track.clear()
        track.update(before)
        return npss_find(x, cfg, track, find_offset, force_peak=p), True
    return w, False


def self_consistent(row, res, frame_size, threshold):
    """A device row against the device's own track row (npss_ema_alpha 1: the row is this call's |c|^2): the first maximum, the value there bit
    for bit, the walk of psr() on that row within one float division, and the decision. res: (ret, peak_pos, peak_value, corr_peak).
    Needs no margin, so it holds on every row. -> None or a description of what differs."""
    ret, pos, val, peak = res
    row = np.asarray(row, np.float32)
    p = int(np.argmax(row)) if row.size else 0
    if pos != p:
        return "peak_pos %d, the row's first maximum is at %d" % (pos, p)
    want = row[p] if row.size else np.float32(0)
    if np.float32(peak).tobytes() != np.float32(want).tobytes():
        return "corr_peak %r, the row holds %r" % (peak, want)
    v = psr(row.astype(np.float64), p, conv_len(frame_size))
    if np.isnan(v) != np.isnan(val) or (np.isinf(v) and val != v) or (np.isfinite(v) and not abs(val - v) <= 2.0 ** -23 * abs(v)):
        return "peak_value %r, the walk on the row gives %r" % (val, v)
    if ret != (1 if val >= threshold else 0):
        return "ret %d with peak_value %r and threshold %r" % (ret, val, threshold)
    return None
