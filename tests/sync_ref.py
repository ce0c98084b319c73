"""Float64 NumPy restatement of one item of srslte_hip_sync_find_batch: the first srslte_sync_find (lib/src/phy/sync/sync.c:618-839) of a reset
object with cfo_i_enable false, decimate 1 and frame type FDD, stage by stage, with the top-two margin of every maximum and the distance of
every thresholded figure from its threshold (relative to the figure's scale). It is the arbiter for the tolerances of tests/test_gpu_sync.py.
Also: the PSS / SSS sequences and a NumPy OFDM modulator for test signals, and get_cell of ue_cell_search.c:189-250."""
import numpy as np

FREQ = np.r_[-31:0, 1:32]  # frequency of bin j of the 62 around DC: the mirrored transforms skip DC (dft_fftw.c:249-272)
FOUND, FOUND_NOSPACE, NOFOUND = 1, 2, 0


def tol(N):
    """float32 bound for sums of N terms; 1e-4 is the convention of the other modules."""
    return max(1e-4, 4 * N * 2.0 ** -24)


def cp_len(N, c):
    return -(-c * N // 2048)


def pss_seq(v):
    """srslte_pss_generate (pss.c:348-376): the phase rounded to float as the reference's expression leaves it."""
    root = (25.0, 29.0, 34.0)[v]
    i = np.arange(62, dtype=np.float64)
    arg = np.where(i < 31, i * (i + 1.0), (i + 2.0) * (i + 1.0)) * (-np.pi * root) / 63.0
    arg = arg.astype(np.float32)
    return np.cos(arg).astype(np.float64) + 1j * np.sin(arg).astype(np.float64)


def _mseq(taps):
    x = np.zeros(31, int)
    x[4] = 1
    for i in range(26):
        x[i + 5] = sum(x[i + t] for t in taps) % 2
    return 1 - 2 * x


S_T, C_T, Z_T = _mseq((2, 0)), _mseq((3, 0)), _mseq((4, 2, 1, 0))
S_TAB = np.array([[S_T[(i + m) % 31] for i in range(31)] for m in range(31)], float)
Z1_TAB = np.array([[Z_T[(i + m % 8) % 31] for i in range(31)] for m in range(31)], float)


def c_tab(v):
    return np.array([[C_T[(i + v + s) % 31] for i in range(31)] for s in (0, 3)], float)


def m0m1(id1):
    qp = id1 // 30
    q = (id1 + qp * (qp + 1) // 2) // 30
    mp = id1 + q * (q + 1) // 2
    m0 = mp % 31
    return m0, (m0 + mp // 31 + 1) % 31


N_ID_1_TABLE = np.zeros((30, 30), int)  # the zeroed table of srslte_sss_init: a pair no cell uses reads 0
for _id in range(168):
    _a, _b = m0m1(_id)
    N_ID_1_TABLE[_a, _b - 1] = _id


def sss_seq(cell_id):
    """srslte_sss_generate (gen_sss.c:121-155): the 62 values of subframe 0 and of subframe 5."""
    m0, m1 = m0m1(cell_id // 3)
    c = c_tab(cell_id % 3)
    s0, s5 = np.zeros(62), np.zeros(62)
    s0[0::2], s0[1::2] = S_TAB[m0] * c[0], S_TAB[m1] * c[1] * Z1_TAB[m0]
    s5[0::2], s5[1::2] = S_TAB[m1] * c[0], S_TAB[m0] * c[1] * Z1_TAB[m1]
    return s0, s5


def idft62(X, N):
    """sum_j X[j] exp(j 2 pi f_j n / N), n < N: the mirrored, unnormalised inverse transform of 62 bins around DC."""
    return np.exp(2j * np.pi * np.outer(np.arange(N), FREQ) / N) @ np.asarray(X, complex)


def dft62(x, N):
    return np.exp(-2j * np.pi * np.outer(FREQ, np.arange(N)) / N) @ np.asarray(x[:N], complex)


def replica(N, v):
    """srslte_pss_init_N_id_2 (pss.c:32-66)."""
    return np.conj(idft62(pss_seq(v), N) / np.sqrt(N)) / 62.0


def sync_slot(cell_id, cp_ext, N, sf_idx=0):
    """Slot 0 of subframe 0 / 5 holding only the SSS and the PSS (its last two symbols), OFDM-modulated with unit-power bins."""
    nsym = 6 if cp_ext else 7
    cps = [cp_len(N, 512)] * 6 if cp_ext else [cp_len(N, 160)] + [cp_len(N, 144)] * 6
    out = []
    for l in range(nsym):
        body = np.zeros(N, complex)
        if l == nsym - 2:
            body = idft62(sss_seq(cell_id)[1 if sf_idx else 0], N) / np.sqrt(62.0)
        if l == nsym - 1:
            body = idft62(pss_seq(cell_id % 3), N) / np.sqrt(62.0)
        out.append(np.r_[body[N - cps[l]:], body])
    return np.concatenate(out)


def _top2(a):
    """(first argmax, (top - second) / top) of a non-negative array."""
    a = np.asarray(a, float)
    i = int(np.argmax(a))
    if a.size < 2 or not a[i] > 0:
        return i, 0.0
    b = np.delete(a, i).max()
    return i, float((a[i] - b) / a[i])


def cp_corr(x, N, max_offset, nsym):
    """srslte_cp_synch (cp.c:61-77)."""
    M = min(max_offset, N)
    corr = np.zeros(M, complex)
    off = 0
    for n in range(nsym):
        cpl = cp_len(N, 144) + (0 if n % 7 else 1)
        for i in range(M):
            a = x[off + i:off + i + cpl]
            b = x[off + i + N:off + i + N + cpl]
            corr[i] += np.sum(a * np.conj(b)) / nsym
        off += N + cpl
    return corr


def lobe_ends(avg, peak, conv_len):
    """The walks of compute_peak_sidelobe (pss.c:412-441) and npss.c:301-343 from the peak to the ends of its lobe -> (pl_lb, pl_ub); avg
    (conv_len - 1 values) is followed by zeros, as conv_output_avg is."""
    A = np.r_[avg, np.zeros(4)]
    ub = peak + 1
    while A[ub + 1] <= A[ub] and ub < conv_len:
        ub += 1
    lb = 0
    if peak > 2:
        lb = peak - 1
        while A[lb - 1] <= A[lb] and lb > 1:
            lb -= 1
    return lb, ub


def psr(avg, peak, conv_len):
    """The peak over the larger of the maxima right of pl_ub and left of pl_lb; an empty range answers its first index."""
    A = np.r_[avg, np.zeros(4)]
    lb, ub = lobe_ends(avg, peak, conv_len)
    dr = max(conv_len - 1 - ub, 0)
    right = A[ub:ub + dr].max() if dr > 0 else A[ub]
    left = A[:lb].max() if lb > 0 else A[0]
    side = right if right > left else left
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(A[peak]) / side)


def _sss_half(y, alg):
    if alg == 0:
        z = y[1:] * np.conj(y[:-1])
        sd = S_TAB[:, 1:] * S_TAB[:, :-1]
        return np.abs(sd @ z) ** 2
    M = 3 if alg == 1 else 1
    Nm = 31 // M
    return sum(np.abs(S_TAB[:, j * Nm:(j + 1) * Nm] @ y[j * Nm:(j + 1) * Nm]) ** 2 for j in range(M))


def detect_cp(x, N, tot):
    """srslte_sync_detect_cp (sync.c:440-495) from M_norm_avg = M_ext_avg = 0, tot = peak_pos + find_offset -> (cp, relative gap of the two
    metrics; None when no symbol fits)."""
    cpn, cpe = cp_len(N, 144), cp_len(N, 512)
    ns = min(tot // (N + cpe), 3)
    if ns == 0:
        return 0, None
    R, M = [], []
    for cpl in (cpn, cpe):
        b = tot - ns * (N + cpl)
        rr = cc = 0.0
        for s in range(ns):
            a = x[b + s * (N + cpl):b + s * (N + cpl) + cpl]
            d = x[b + s * (N + cpl) + N:b + s * (N + cpl) + N + cpl]
            rr += float(np.sum(d * np.conj(a)).real)
            cc += float(np.sum(np.abs(a) ** 2))
        R.append(rr)
        M.append(0.1 * ((rr / cc if cc > 0 else 0.0) / ns))
    cp = 0 if M[0] > M[1] else 1 if M[0] < M[1] else 0 if R[0] > R[1] else 1
    return cp, abs(M[0] - M[1]) / max(abs(M[0]), abs(M[1]), 1e-30)


def exact_cfo(f, length):
    """exp(j 2 pi f n), n < length."""
    return np.exp(2j * np.pi * f * np.arange(length))


def reference_cfo(f, length, lanes=8):
    """What srslte_vec_apply_cfo (vector_simd.c:1556-1604) multiplies by in the reference build of oracle/ref.mk (AVX2: 8 complex lanes): a
    float32 phasor per lane, started at cexpf(j 2 pi f k) and multiplied once per vector by cexpf(j 2 pi f lanes). The step is rounded to
    float32 once, so its modulus and its angle are off by a few 1e-8 and the factors drift from the exact ones in proportion to the
    sample index: 6e-5 of peak_value over the 9600 samples of a 128-point window of 5 ms, 1.7e-4 over the 28 800 of a 384-point one. The
    rounding of the single products, which has no preferred direction, is left out."""
    f32 = np.float32
    w = f32(2.0) * f32(np.pi) * f32(f)
    cexpf = lambda a: np.cos(f32(a)).astype(f32).astype(float) + 1j * np.sin(f32(a)).astype(f32).astype(float)
    n = np.arange(length)
    return cexpf(w * np.arange(lanes, dtype=f32))[n % lanes] * complex(cexpf(w * f32(lanes))) ** (n // lanes)


def find_one(x, cfg, N_id_2, find_offset=0, N_id_1=-1, force_peak=None, force_cp=None, frame_cfo=None):
    """x: the item's samples. cfg: a dict with the fields of srslte_hip_sync_cfg_t. -> dict with the fields of srslte_hip_sync_res_t, "margins"
    {stage: relative margin} of every decision taken, "cp_corr" and "avg" (the averaged |c|^2). force_peak: take this index as the maximum
    of the correlation (for a caller that has checked it to be one within its tolerance: at large fft_size the peak's neighbours are within
    0.3 % of it) and go on from there. force_cp: the same for the maximum of the CP correlation, whose neighbours are as close at those sizes. frame_cfo(f, length): the factors that correct the frame by the CP-based CFO (sync.c:674), exact_cfo
    unless given; reference_cfo is what the reference's own build multiplies by."""
    N, mo, fo = cfg["fft_size"], cfg["max_offset"], find_offset
    x = np.asarray(x, complex)
    mg = {}
    o = dict(ret=NOFOUND, peak_pos=0, peak_value=0.0, corr_peak=0.0, cfo_cp=0.0, cfo_pss=0.0, cfo=0.0, sss_available=0, sss_detected=0, m0=0, m1=0,
             sf_idx=0, N_id_1=N_id_1 if N_id_1 >= 0 else -1, cell_id=-1, sss_corr=0.0, cp=cfg["cp"], margins=mg, cp_corr=None)
    if cfg["cfo_cp_enable"]:
        corr = cp_corr(x, N, mo, cfg["cfo_cp_nsymbols"])
        i, mg["cp_argmax"] = _top2(np.abs(corr) ** 2)
        if force_cp is not None:
            i = int(force_cp)
            del mg["cp_argmax"]
        o["cp_corr"] = corr
        o["cfo_cp"] = float(-np.angle(corr[i]) / np.pi / 2)
        x = x * (frame_cfo or exact_cfo)(-o["cfo_cp"] / N, x.size)
    h = replica(N, N_id_2)
    if mo >= N:
        conv = np.convolve(x[fo:fo + mo], h)[:mo + N - 2]
    else:
        conv = np.array([np.sum(h * x[fo + i:fo + i + N]) for i in range(mo - 1)])
    alpha = cfg.get("ema_alpha", 0.0) or 0.2
    avg = np.abs(conv) ** 2 * (alpha if 0.0 < alpha < 1.0 else 1.0)
    peak, mg["peak"] = _top2(avg)
    o["avg"] = avg
    if force_peak is not None:
        peak = int(force_peak)
        del mg["peak"]
    o["corr_peak"] = float(avg[peak])
    thr = cfg["threshold"]
    if thr > 0:
        o["peak_value"] = psr(avg, peak, avg.size + 1)
        mg["threshold"] = abs(o["peak_value"] - thr) / max(o["peak_value"], thr)
    peak_pos = peak + (N if mo < N else 0)
    o["peak_pos"] = peak_pos
    if not (o["peak_value"] >= thr or thr == 0):
        return _finish(o, N_id_2)
    tot = peak_pos + fo
    if cfg["cfo_pss_enable"] and peak_pos >= N:
        p = x[tot - N:tot]
        if cfg["pss_filt_enable"]:
            p = idft62(dft62(p, N), N)
        y0, y1 = np.sum(h[:N // 2] * p[:N // 2]), np.sum(h[N // 2:] * p[N // 2:])
        o["cfo_pss"] = float(np.angle(np.conj(y0) * y1) / np.pi)
    cpn, cpe = cp_len(N, 144), cp_len(N, 512)
    if tot < 2 * (N + cpe):
        o["ret"] = FOUND_NOSPACE
        return _finish(o, N_id_2)
    if cfg["sss_en"]:
        o["sss_available"] = 1
        cp_sz = cpe if cfg["cp"] else cpn
        sss_idx = tot - 2 * (N + cp_sz) + cp_sz
        if sss_idx >= 0:
            s = x[sss_idx:sss_idx + N]
            if cfg["cfo_pss_enable"]:
                s = s * np.exp(-2j * np.pi * o["cfo_pss"] / N * np.arange(N))
            Y = dft62(s, N)
            if N_id_1 >= 0:
                s0, s5 = sss_seq(3 * N_id_1 + N_id_2)
                r0, r5 = abs(np.sum(s0 * np.conj(Y))), abs(np.sum(s5 * np.conj(Y)))
                ratio = r0 / r5 if r0 > r5 else r5 / r0
                mg["known_sf"] = abs(r0 - r5) / max(r0, r5)
                mg["known_ratio"] = abs(ratio - 1.2) / 1.2
                if ratio > 1.2:
                    o.update(sss_detected=1, sf_idx=0 if r0 > r5 else 5, sss_corr=float(ratio))
            else:
                c = c_tab(N_id_2)
                y = [Y[0::2], Y[1::2]]
                for w in range(2):
                    pw = np.mean(np.abs(y[w]) ** 2)
                    y[w] = y[w] / (np.sqrt(pw) if pw != 0 else 1.0) * c[w]
                c0 = _sss_half(y[0], cfg["sss_alg"])
                m0, mg["m0"] = _top2(c0)
                c1 = _sss_half(y[1] * Z1_TAB[m0], cfg["sss_alg"])
                m1, mg["m1"] = _top2(c1)
                corr = float(c0[m0] + c1[m1])
                o.update(m0=m0, m1=m1)
                mg["sss_threshold"] = abs(corr - cfg["sss_threshold"]) / max(corr, abs(cfg["sss_threshold"]), 1e-30)
                nid = -1
                if corr > cfg["sss_threshold"]:
                    if m1 > m0:
                        if m0 < 30 and m1 - 1 < 30:
                            nid = int(N_ID_1_TABLE[m0, m1 - 1])
                    elif m1 < 30 and 0 <= m0 - 1 < 30:
                        nid = int(N_ID_1_TABLE[m1, m0 - 1])
                if nid >= 0:
                    o.update(sss_detected=1, sf_idx=0 if m1 > m0 else 5, N_id_1=nid, sss_corr=corr)
        else:
            o["sss_available"] = 0
    if cfg["detect_cp"]:
        o["cp"], m = detect_cp(x, N, tot)
        if m is not None:
            mg["cp_detect"] = m
    o["ret"] = FOUND
    return _finish(o, N_id_2)


def _finish(o, N_id_2):
    o["cfo"] = o["cfo_cp"] + o["cfo_pss"]
    o["cell_id"] = 3 * o["N_id_1"] + N_id_2 if 0 <= o["N_id_1"] < 168 else -1
    return o


DISCRETE = ("ret", "peak_pos", "m0", "m1", "sf_idx", "N_id_1", "cell_id", "cp", "sss_available", "sss_detected")
FLOATS = {"peak_value": "self", "corr_peak": "self", "cfo_cp": 1.0, "cfo_pss": 1.0, "cfo": 1.0, "sss_corr": "self"}


def get_cell(rows):
    """get_cell (ue_cell_search.c:189-250) over rows (dicts or structs with ret, cell_id, cp, corr_peak, peak_value, cfo): those with ret == 1
    and cell_id >= 0 count (:311-332). -> (n, dict) with n = 0 and None when none counts."""
    g = (lambda r, k: r[k]) if rows and isinstance(rows[0], dict) else getattr
    cand = [r for r in rows if g(r, "ret") == 1 and g(r, "cell_id") >= 0]
    n = len(cand)
    if n == 0:
        return 0, None
    counted, ntimes = [0] * n, [0] * n
    for i in range(n):
        cnt = 1
        for j in range(i + 1, n):
            if g(cand[j], "cell_id") == g(cand[i], "cell_id") and not counted[j]:
                counted[j] = 1
                cnt += 1
        ntimes[i] = cnt
    max_times, mode_pos = 0, 0
    for i in range(n):
        if ntimes[i] > max_times:
            max_times, mode_pos = ntimes[i], i
    cid = g(cand[mode_pos], "cell_id")
    nof_normal = sum(1 for r in cand if g(r, "cell_id") == cid and g(r, "cp") == 0)
    peak = np.float32(0)
    for r in cand:
        peak = np.float32(peak + np.float32(g(r, "corr_peak")))
    return n, dict(cell_id=cid, cp=0 if nof_normal > ntimes[mode_pos] // 2 else 1, peak=float(np.float32(peak / np.float32(n))),
                   mode=float(np.float32(ntimes[mode_pos]) / np.float32(n)), psr=float(g(cand[-1], "peak_value")),
                   cfo=float(np.float32(15000) * np.float32(g(cand[-1], "cfo"))), nof_frames=n)


def ofdm_frame(cell_id, cp_ext, N, nsf, rng, first_sf=0):
    """nsf subframes from subframe first_sf of a 6-PRB-wide FDD cell: unit-power random QPSK on the 72 central carriers of every symbol, the
    SSS and PSS (62 carriers, the 10 around them empty) in the last two symbols of slot 0 of subframes 0 and 5."""
    nsym = 6 if cp_ext else 7
    cps = [cp_len(N, 512)] * 6 if cp_ext else [cp_len(N, 160)] + [cp_len(N, 144)] * 6
    f72 = np.r_[-36:0, 1:37]
    E = np.exp(2j * np.pi * np.outer(np.arange(N), f72) / N) / np.sqrt(72.0)
    out = []
    for b in range(nsf):
        sf = (first_sf + b) % 10
        for slot in range(2):
            for l in range(nsym):
                X = (rng.choice([-1.0, 1.0], 72) + 1j * rng.choice([-1.0, 1.0], 72)) / np.sqrt(2)
                if slot == 0 and sf in (0, 5) and l >= nsym - 2:
                    X[:] = 0
                    X[5:67] = sss_seq(cell_id)[1 if sf else 0] if l == nsym - 2 else pss_seq(cell_id % 3)
                body = E @ X
                out.append(np.r_[body[N - cps[l]:], body])
    return np.concatenate(out)


def awgn(x, snr_db, rng):
    """x plus complex noise snr_db below x's mean power (None: none)."""
    if snr_db is None:
        return x
    s = np.sqrt(np.mean(np.abs(x) ** 2) * 10 ** (-snr_db / 10) / 2)
    return x + s * (rng.normal(size=x.size) + 1j * rng.normal(size=x.size))
