"""Float64 NumPy restatement of one row of srslte_hip_meas_run_batch: srslte_refsignal_dl_sync_set_cell + srslte_refsignal_dl_sync_run
(lib/src/phy/sync/refsignal_dl_sync.c:84-154, :185-355) for one capture and one candidate cell, normal CP, FDD - the replicas, the search
through numpy.fft and the measurement - with the deciding margins of every row: how far peak / (thr mean(rms)) is from 1, and the
correlation's runner-up over its peak. It is the arbiter for the tolerances of tests/test_gpu_meas.py. Also: the cell-specific reference
signal, a NumPy OFDM modulator and a builder of captures that hold several cells."""
import functools

import numpy as np

from sync_ref import awgn, cp_len, pss_seq, sss_seq, tol  # noqa: F401  (awgn and tol are re-exported for the tests)

THR = 5.5
UINT32_MAX = 0xFFFFFFFF
CRS_SYMBOLS = (0, 4, 7, 11)  # srslte_refsignal_cs_nsymbol(l, SRSLTE_CP_NORM, 0 / 1)
DISCRETE = ("found", "peak_index", "sf_idx", "nof_sf")
SEARCH_FLOATS = ("peak_value", "rms_avg")
MEAS_FLOATS = {"rsrp_lin": "self", "rssi_lin": "self", "rsrp_dBfs": "dB", "rssi_dBfs": "dB", "rsrq_dB": "dB", "cfo_Hz": "rad"}
HZ_PER_RAD = 15000.0 / (2 * np.pi * 7.5)  # measure_sf's factor on the angle between CRS symbols half a slot apart (:350-351)


def symbol_sz(nof_prb):
    """srslte_symbol_sz (phy_common.c:322-345), the default family."""
    for lim, n in ((6, 128), (15, 256), (25, 384), (50, 768), (75, 1024), (110, 1536)):
        if nof_prb <= lim:
            return n
    raise ValueError(nof_prb)


@functools.lru_cache(maxsize=None)
def _x1(n):
    x = [0] * (n + 31)
    x[0] = 1
    for i in range(n):
        x[i + 31] = x[i + 3] ^ x[i]
    return x


def gold(c_init, length):
    """c(n) of 36.211 7.2: x1(0) = 1, x2 from c_init, N_c = 1600."""
    n = length + 1600
    x1 = _x1(n)
    x2 = [(c_init >> i) & 1 for i in range(31)] + [0] * n
    for i in range(n):
        x2[i + 31] = x2[i + 3] ^ x2[i + 2] ^ x2[i + 1] ^ x2[i]
    return np.array([x1[i + 1600] ^ x2[i + 1600] for i in range(length)], np.int8)


@functools.lru_cache(maxsize=None)
def crs_pilots(cell_id, nof_prb):
    """r_l,ns(m) of 36.211 6.10.1.1 for ports 0 and 1, normal CP (refsignal_dl.c:66-112): [10][4][2 nof_prb], symbol l of the subframe's four."""
    out = np.zeros((10, 4, 2 * nof_prb), complex)
    for ns in range(20):
        for l, lp in enumerate((0, 4)):
            c = gold(1024 * (7 * (ns + 1) + lp + 1) * (2 * cell_id + 1) + 2 * cell_id + 1, 440)
            m = np.arange(2 * nof_prb) + 110 - nof_prb
            out[ns // 2, (ns % 2) * 2 + l] = ((1 - 2.0 * c[2 * m]) + 1j * (1 - 2.0 * c[2 * m + 1])) / np.sqrt(2)
    return out


def crs_positions(cell_id, nof_prb, l, port):
    """(symbol, carriers) of CRS symbol l < 4 of port 0 / 1 (srslte_refsignal_cs_nsymbol, _fidx)."""
    v = 3 if (l + port) % 2 else 0
    return CRS_SYMBOLS[l], (v + cell_id % 6) % 6 + 6 * np.arange(2 * nof_prb)


def replica_grids(cell_id, nof_prb):
    """The 10 frequency-domain grids of set_cell (:110-139), [10][14][12 nof_prb]: PSS + SSS in subframes 0 and 5, the CRS of ports 0 and 1."""
    nre = 12 * nof_prb
    g = np.zeros((10, 14, nre), complex)
    pil = crs_pilots(cell_id, nof_prb)
    s0, s5 = sss_seq(cell_id)
    k = nre // 2 - 31
    for sf in range(10):
        if sf in (0, 5):
            g[sf, 6, k:k + 62] = pss_seq(cell_id % 3)
            g[sf, 5, k:k + 62] = s5 if sf else s0
        for port in range(2):
            for l in range(4):
                sym, car = crs_positions(cell_id, nof_prb, l, port)
                g[sf, sym, car] = pil[sf, l]
    return g


def ofdm_mod(grid, N):
    """[nsf][14][nre] -> [nsf][15 N]: the un-normalised modulator of srslte_ofdm_tx_sf (ofdm.c:488-530), DC skipped, normal CP."""
    grid = np.asarray(grid, complex)
    nsf, _, nre = grid.shape
    half = nre // 2
    bins = np.zeros((nsf, 14, N), complex)
    bins[:, :, N - half:] = grid[:, :, :half]
    bins[:, :, 1:1 + half] = grid[:, :, half:]
    body = np.fft.ifft(bins, axis=2) * N
    out = []
    for s in range(14):
        c = cp_len(N, 160 if s % 7 == 0 else 144)
        out += [body[:, s, N - c:], body[:, s]]
    return np.concatenate(out, axis=1)


@functools.lru_cache(maxsize=64)
def replicas(cell_id, nof_prb, N):
    """q->sequences of set_cell: [10][15 N], the modulated grids times 1 / (8 nof_prb) (:145-148)."""
    return ofdm_mod(replica_grids(cell_id, nof_prb), N) / (8.0 * nof_prb)


def correlate_fft(x2, seq0):
    """c[k] = sum_m x2[k + m] conj(seq0[m]), k < L, from a block of 2 L samples as find_peak forms it (:195-209)."""
    L = seq0.size
    H = np.fft.fft(np.r_[seq0, np.zeros(L)])
    return np.fft.ifft(np.fft.fft(x2[:2 * L]) * np.conj(H))[:L]


def correlate_direct(x2, seq0):
    L = seq0.size
    return np.array([np.sum(x2[k:k + L] * np.conj(seq0)) for k in range(L)])


def measure_sf(buf, seq, nof_prb, N):
    """srslte_refsignal_dl_sync_measure_sf (:303-355) -> rsrp, rssi, cfo."""
    cp0, cp1 = cp_len(N, 160), cp_len(N, 144)
    corr, rssi = [], 0.0
    for l, symbidx in enumerate(CRS_SYMBOLS):
        off = cp0 + (N + cp1) * symbidx + (cp0 - cp1 if l >= 2 else 0)
        a = buf[off:off + N]
        corr.append(np.sum(a * np.conj(seq[off:off + N])))
        rssi += float(np.sum(np.abs(a) ** 2))
    rsrp = sum(abs(c) ** 2 for c in corr) * 4
    cfo = (np.angle(corr[2] * np.conj(corr[0])) + np.angle(corr[3] * np.conj(corr[1]))) * HZ_PER_RAD / 2
    return float(rsrp), nof_prb * rssi / 4 * 7.41, float(cfo)


def run_one(x, nof_sf, cell_id, nof_prb, N=None, thr=THR):
    """x: the capture's nof_sf 15 N samples (more are ignored). -> dict with the fields of srslte_hip_meas_res_t and "margins": "threshold" =
    |peak / (thr mean(rms)) - 1| and, on found rows, "peak" = 1 - runner-up / peak over all searched blocks."""
    N = N or symbol_sz(nof_prb)
    L = 15 * N
    x = np.asarray(x, complex)[:nof_sf * L]
    seq = replicas(cell_id, nof_prb, N)
    nb = min(nof_sf - 1, 10)
    mags = np.empty((nb, L))
    for b in range(nb):
        mags[b] = np.abs(correlate_fft(x[b * L:(b + 2) * L], seq[0]))
    peak_value, peak_idx = 0.0, 0
    for b in range(nb):
        i = int(np.argmax(mags[b]))
        if mags[b, i] > peak_value:
            peak_value, peak_idx = float(mags[b, i]), i + b * L
    rms_avg = float(np.mean(np.sqrt(np.mean(mags ** 2, axis=1))))
    found = peak_value > rms_avg * thr
    o = dict(found=int(found), peak_index=UINT32_MAX, sf_idx=0, nof_sf=0, peak_value=peak_value, rms_avg=rms_avg, rsrp_lin=np.nan, rssi_lin=np.nan,
             rsrp_dBfs=np.nan, rssi_dBfs=np.nan, rsrq_dB=np.nan, cfo_Hz=np.nan, cell_id=cell_id,
             margins=dict(threshold=abs(peak_value / (thr * rms_avg) - 1)))
    if not found:
        return o
    flat = mags.ravel().copy()
    flat[peak_idx] = -1.0
    o["margins"]["peak"] = 1 - float(flat.max()) / peak_value
    sf0, n = (20 - peak_idx // L) % 10, peak_idx % L
    acc, cnt = np.zeros(3), 0
    while n < nof_sf * L - L + 1:
        acc += measure_sf(x[n:n + L], seq[(sf0 + cnt) % 10], nof_prb, N)
        cnt += 1
        n += L
    rsrp, rssi, cfo = acc / cnt
    o.update(peak_index=peak_idx, sf_idx=sf0, nof_sf=cnt, rsrp_lin=rsrp, rssi_lin=rssi, cfo_Hz=cfo, rsrp_dBfs=10 * np.log10(rsrp) + 30,
             rssi_dBfs=10 * np.log10(rssi) + 30)
    o["rsrq_dB"] = 10 * np.log10(nof_prb) + o["rsrp_dBfs"] - o["rssi_dBfs"]
    return o


# ---------------------------------------------------------------- test signals
def cell_subframes(cell_id, nof_prb, N, first_sf, nsf, rng):
    """nsf subframes from subframe first_sf of a two-port cell: the grids of replica_grids (CRS on both ports, PSS / SSS) with unit-power random
    QPSK on every other RE, modulated with unit mean power per occupied carrier -> nsf 15 N samples."""
    nre = 12 * nof_prb
    ref = replica_grids(cell_id, nof_prb)
    g = np.empty((nsf, 14, nre), complex)
    for b in range(nsf):
        sf = (first_sf + b) % 10
        data = (rng.choice([-1.0, 1.0], (14, nre)) + 1j * rng.choice([-1.0, 1.0], (14, nre))) / np.sqrt(2)
        used = ref[sf] != 0
        if sf in (0, 5):
            used[5:7, nre // 2 - 36:nre // 2 + 36] = True  # the 72 carriers of the synchronisation symbols, their empty edges included
        g[b] = np.where(used, ref[sf], data)
    return ofdm_mod(g, N).ravel() / np.sqrt(nre)


def capture(cells, nof_prb, N, nof_sf, rng, snr_db=10.0):
    """cells: dicts(id, start_sf, delay, amp, cfo_hz): the cell's subframe start_sf begins at sample delay < 15 N of the capture. -> nof_sf 15 N
    samples, the cells summed, noise snr_db below the sum's power."""
    L = 15 * N
    x = np.zeros(nof_sf * L, complex)
    n = np.arange(nof_sf * L)
    for c in cells:
        d = c.get("delay", 0)
        assert 0 <= d < L
        f = cell_subframes(c["id"], nof_prb, N, (c.get("start_sf", 0) - 1) % 10, nof_sf + 1, rng)
        x += c.get("amp", 1.0) * f[L - d:L - d + nof_sf * L] * np.exp(2j * np.pi * c.get("cfo_hz", 0.0) * n / (15000.0 * N))
    return awgn(x, snr_db, rng)


def planted_index(c, N, nof_sf):
    """Where find_peak should see a planted cell: the start of its subframe 0, or None when none starts inside the searched blocks."""
    L = 15 * N
    idx = c.get("delay", 0) + ((10 - c.get("start_sf", 0)) % 10) * L
    return idx if idx < min(nof_sf - 1, 10) * L else None
