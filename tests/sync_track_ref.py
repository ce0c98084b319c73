"""Float64 NumPy restatement of a SEQUENCE of srslte_sync_find calls on one srslte_sync_t (lib/src/phy/sync/sync.c:618-839), as
srslte_hip_sync_track_batch runs them on a track: the state the reference keeps between calls - the PSS correlation average (pss.c:495-503),
the two CFO means and their is_set flags, M_norm_avg / M_ext_avg, cp, N_id_1, sf_idx, sss_corr, peak_value, frame_type, sss_available - the
TDD SSS position and frame-type detection (sync.c:732-809), srslte_sync_reset, srslte_sync_cfo_reset and srslte_sync_copy_cfo. Built on
tests/sync_ref.py, whose find_one is the first call of a Track in frame mode FDD. Every call returns the margins of its maxima and decisions
as find_one does; the arbiter for the tolerances of tests/test_gpu_sync_track.py.
Two cases the reference leaves to uninitialised stack values are defined as phy_hip.h defines them: a trial whose symbol would start before
the item does not run, cannot win and has sss_corr_trial NaN; a winning m0 / m1 trial that detected nothing leaves the previous N_id_1.
Also: the TDD variant of sync_ref.ofdm_frame and get_cell with the frame type."""
import numpy as np

import sync_ref as sr

FDD, TDD, DETECT = 0, 1, 2
RESET_AVG, RESET_CFO, RESET_REST = 1, 2, 4
DISCRETE = sr.DISCRETE + ("frame_type", "nof_calls")
FLOATS = dict(sr.FLOATS, cfo_cp_inst=1.0, cfo_pss_inst=1.0, M_norm_avg=1.0, M_ext_avg=1.0)


def _ema(data, avg, alpha):
    return alpha * data + (1 - alpha) * avg  # SRSLTE_VEC_EMA


class Track:
    """One srslte_sync_t. cfg: a dict with the fields of srslte_hip_sync_cfg_t."""

    def __init__(self, cfg, cfo_ema_alpha=0.0, frame_mode=FDD):
        self.cfg, self.frame_mode = dict(cfg), frame_mode
        self.cfo_alpha = float(np.float32(cfo_ema_alpha or 0.1))
        N, mo = cfg["fft_size"], cfg["max_offset"]
        self.nout = mo + N - 2 if mo >= N else mo - 1
        a = cfg.get("ema_alpha", 0.0) or 0.2
        self.alpha = float(np.float32(a)) if 0.0 < a < 1.0 else None
        self.reset(7)

    def reset(self, flags):
        if flags & RESET_AVG:  # srslte_sync_reset (sync.c:841-845)
            self.M_norm_avg = self.M_ext_avg = 0.0
            self.avg = np.zeros(self.nout)
        if flags & RESET_CFO:  # srslte_sync_cfo_reset (sync.c:346-352)
            self.cfo_cp_mean = self.cfo_pss_mean = 0.0
            self.cfo_cp_is_set = self.cfo_pss_is_set = False
        if flags & RESET_REST:
            self.cp, self.N_id_1, self.sf_idx, self.sss_corr, self.peak_value = self.cfg["cp"], -1, 0, 0.0, 0.0
            self.sss_available, self.nof_calls = 0, 0
            self.frame_type = TDD if self.frame_mode == TDD else FDD

    def copy_cfo(self, src):
        """srslte_sync_copy_cfo (sync.c:354-360)."""
        self.cfo_cp_mean, self.cfo_pss_mean = src.cfo_cp_mean, src.cfo_pss_mean
        self.cfo_cp_is_set = self.cfo_pss_is_set = False

    def _sss(self, s, N_id_2, known, mg, tag):
        """sync_sss_symbol (sync.c:500-564) on the N samples s -> (detected, sf_idx, N_id_1 or None where none is written, corr, m0, m1)."""
        N, cfg = self.cfg["fft_size"], self.cfg
        Y = sr.dft62(s, N)
        if known >= 0:
            s0, s5 = sr.sss_seq(3 * known + N_id_2)
            r0, r5 = abs(np.sum(s0 * np.conj(Y))), abs(np.sum(s5 * np.conj(Y)))
            ratio = r0 / r5 if r0 > r5 else r5 / r0
            mg["known_sf" + tag] = abs(r0 - r5) / max(r0, r5)
            mg["known_ratio" + tag] = abs(ratio - 1.2) / 1.2
            return ratio > 1.2, 0 if r0 > r5 else 5, known, float(ratio), 0, 0
        c = sr.c_tab(N_id_2)
        y = [Y[0::2], Y[1::2]]
        for w in range(2):
            pw = np.mean(np.abs(y[w]) ** 2)
            y[w] = y[w] / (np.sqrt(pw) if pw != 0 else 1.0) * c[w]
        c0 = sr._sss_half(y[0], cfg["sss_alg"])
        m0, mg["m0" + tag] = sr._top2(c0)
        c1 = sr._sss_half(y[1] * sr.Z1_TAB[m0], cfg["sss_alg"])
        m1, mg["m1" + tag] = sr._top2(c1)
        corr = float(c0[m0] + c1[m1])
        mg["sss_threshold" + tag] = abs(corr - cfg["sss_threshold"]) / max(corr, abs(cfg["sss_threshold"]), 1e-30)
        nid = -1
        if corr > cfg["sss_threshold"]:
            if m1 > m0:
                if m0 < 30 and m1 - 1 < 30:
                    nid = int(sr.N_ID_1_TABLE[m0, m1 - 1])
            elif m1 < 30 and 0 <= m0 - 1 < 30:
                nid = int(sr.N_ID_1_TABLE[m1, m0 - 1])
        return nid >= 0, 0 if m1 > m0 else 5, nid if nid >= 0 else None, corr, m0, m1

    def find(self, x, N_id_2, find_offset=0, N_id_1=-1, force_peak=None, force_cp=None):
        """One srslte_sync_find on the item's samples x -> dict with the fields of srslte_hip_sync_track_res_t (those of srslte_hip_sync_res_t
        flat), "margins", "avg" and "cp_corr". force_peak and force_cp as in sync_ref.find_one."""
        cfg = self.cfg
        N, mo, fo = cfg["fft_size"], cfg["max_offset"], find_offset
        x = np.asarray(x, complex)
        mg = {}
        self.nof_calls += 1
        if N_id_1 >= 0:
            self.N_id_1 = N_id_1  # srslte_sync_set_N_id_1
        o = dict(ret=sr.NOFOUND, sss_detected=0, m0=0, m1=0, cfo_cp_inst=0.0, cfo_pss_inst=0.0, sss_corr_trial=[np.nan, np.nan], margins=mg,
                 cp_corr=None, undefined_in_reference=False)
        if cfg["cfo_cp_enable"]:
            corr = sr.cp_corr(x, N, mo, cfg["cfo_cp_nsymbols"])
            i, mg["cp_argmax"] = sr._top2(np.abs(corr) ** 2)
            if force_cp is not None:
                i = int(force_cp)
                del mg["cp_argmax"]
            o["cp_corr"] = corr
            est = float(-np.angle(corr[i]) / np.pi / 2)
            self.cfo_cp_mean = _ema(est, self.cfo_cp_mean, self.cfo_alpha) if self.cfo_cp_is_set else est
            self.cfo_cp_is_set = True
            o["cfo_cp_inst"] = est
            x = x * np.exp(-2j * np.pi * self.cfo_cp_mean / N * np.arange(x.size))
        h = sr.replica(N, N_id_2)
        if mo >= N:
            conv = np.convolve(x[fo:fo + mo], h)[:mo + N - 2]
        else:
            conv = np.array([np.sum(h * x[fo + i:fo + i + N]) for i in range(mo - 1)])
        if self.alpha is not None:
            self.avg = self.alpha * np.abs(conv) ** 2 + (1 - self.alpha) * self.avg
        else:
            self.avg = np.abs(conv) ** 2
        avg = self.avg
        peak, mg["peak"] = sr._top2(avg)
        o["avg"] = avg.copy()
        if force_peak is not None:
            peak = int(force_peak)
            del mg["peak"]
        o["corr_peak"] = float(avg[peak])
        thr = cfg["threshold"]
        if thr > 0:
            self.peak_value = sr.psr(avg, peak, avg.size + 1)
            mg["threshold"] = abs(self.peak_value - thr) / max(self.peak_value, thr)
        peak_pos = peak + (N if mo < N else 0)
        o["peak_pos"] = peak_pos
        if not (self.peak_value >= thr or thr == 0):
            return self._finish(o, N_id_2)
        tot = peak_pos + fo
        if cfg["cfo_pss_enable"] and peak_pos >= N:
            p = x[tot - N:tot]
            if cfg["pss_filt_enable"]:
                p = sr.idft62(sr.dft62(p, N), N)
            y0, y1 = np.sum(h[:N // 2] * p[:N // 2]), np.sum(h[N // 2:] * p[N // 2:])
            est = float(np.angle(np.conj(y0) * y1) / np.pi)
            o["cfo_pss_inst"] = est
            if not self.cfo_pss_is_set:
                self.cfo_pss_mean, self.cfo_pss_is_set = est, True
            else:
                mg["cfo_pss_gate"] = abs(15000 * abs(est) - 7000) / 7000
                if 15000 * abs(est) < 7000:
                    self.cfo_pss_mean = _ema(est, self.cfo_pss_mean, self.cfo_alpha)
        cpn, cpe = sr.cp_len(N, 144), sr.cp_len(N, 512)
        if tot < 2 * (N + cpe):
            o["ret"] = sr.FOUND_NOSPACE
            return self._finish(o, N_id_2)
        if cfg["sss_en"]:
            self.sss_available = 1
            cp_sz = cpe if self.cp else cpn
            trials = (FDD, TDD) if self.frame_mode == DETECT else (self.frame_mode,)
            res = {}
            for f in trials:
                sss_idx = tot - (4 if f == TDD else 2) * (N + cp_sz) + cp_sz
                if sss_idx < 0:
                    self.sss_available = 0
                    continue
                s = x[sss_idx:sss_idx + N]
                if cfg["cfo_pss_enable"]:
                    s = s * np.exp(-2j * np.pi * self.cfo_pss_mean / N * np.arange(N))
                res[f] = self._sss(s, N_id_2, self.N_id_1 if N_id_1 >= 0 else -1, mg, "_tdd" if f == TDD and self.frame_mode == DETECT else "")
                o["sss_corr_trial"][f] = res[f][3]
                o["sss_detected"] |= int(res[f][0])
            if self.frame_mode == DETECT:
                if FDD in res:
                    w = FDD
                    if TDD in res:
                        a, b = res[FDD][3], res[TDD][3]
                        mg["frame_type"] = abs(a - b) / max(abs(a), abs(b), 1e-30)
                        w = FDD if a > b else TDD
                    det, sf, nid, corr, m0, m1 = res[w]
                    self.frame_type, self.sf_idx, self.sss_corr = w, sf + w, corr
                    if nid is not None:
                        self.N_id_1 = nid
                    o.update(m0=m0, m1=m1)
                    # what the reference reads from uninitialised stack values here: the correlation of a trial that did not run, the
                    # N_id_1 of a winning m0 / m1 trial that detected nothing. Its own rows are not comparable from this call on.
                    o["undefined_in_reference"] = TDD not in res or nid is None
            elif trials[0] in res:
                det, sf, nid, corr, m0, m1 = res[trials[0]]
                o.update(m0=m0, m1=m1)
                if det:
                    self.sf_idx, self.N_id_1, self.sss_corr = sf + trials[0], nid, corr
        if cfg["detect_cp"]:
            ns = min(tot // (N + cpe), 3)
            if ns > 0:
                R, M = [], []
                for cpl, prev in ((cpn, self.M_norm_avg), (cpe, self.M_ext_avg)):
                    b = tot - ns * (N + cpl)
                    rr = cc = 0.0
                    for k in range(ns):
                        a = x[b + k * (N + cpl):b + k * (N + cpl) + cpl]
                        d = x[b + k * (N + cpl) + N:b + k * (N + cpl) + N + cpl]
                        rr += float(np.sum(d * np.conj(a)).real)
                        cc += float(np.sum(np.abs(a) ** 2))
                    R.append(rr)
                    M.append(_ema((rr / cc if cc > 0 else 0.0) / ns, prev, 0.1))
                self.M_norm_avg, self.M_ext_avg = M
                self.cp = 0 if M[0] > M[1] else 1 if M[0] < M[1] else 0 if R[0] > R[1] else 1
                mg["cp_detect"] = abs(M[0] - M[1]) / max(abs(M[0]), abs(M[1]), 1e-30)
            else:
                self.cp = 0
        o["ret"] = sr.FOUND
        return self._finish(o, N_id_2)

    def _finish(self, o, N_id_2):
        o.update(peak_value=self.peak_value, cfo_cp=self.cfo_cp_mean, cfo_pss=self.cfo_pss_mean, cfo=self.cfo_cp_mean + self.cfo_pss_mean,
                 sss_available=self.sss_available, sf_idx=self.sf_idx, N_id_1=self.N_id_1, sss_corr=self.sss_corr, cp=self.cp,
                 cell_id=3 * self.N_id_1 + N_id_2 if 0 <= self.N_id_1 < 168 else -1, frame_type=self.frame_type, nof_calls=self.nof_calls,
                 M_norm_avg=self.M_norm_avg, M_ext_avg=self.M_ext_avg)
        return o


def ofdm_frame_tdd(cell_id, cp_ext, N, nsf, rng, first_sf=0):
    """sync_ref.ofdm_frame for a TDD cell: the PSS in the third symbol of subframes 1 and 6, the SSS in the last symbol of subframes 0 and 5;
    every subframe carries downlink-like QPSK (the synchroniser does not look at the uplink / guard structure)."""
    nsym = 6 if cp_ext else 7
    cps = [sr.cp_len(N, 512)] * 6 if cp_ext else [sr.cp_len(N, 160)] + [sr.cp_len(N, 144)] * 6
    f72 = np.r_[-36:0, 1:37]
    E = np.exp(2j * np.pi * np.outer(np.arange(N), f72) / N) / np.sqrt(72.0)
    out = []
    for b in range(nsf):
        sf = (first_sf + b) % 10
        for slot in range(2):
            for l in range(nsym):
                X = (rng.choice([-1.0, 1.0], 72) + 1j * rng.choice([-1.0, 1.0], 72)) / np.sqrt(2)
                if slot == 1 and sf in (0, 5) and l == nsym - 1:
                    X[:] = 0
                    X[5:67] = sr.sss_seq(cell_id)[1 if sf else 0]
                if slot == 0 and sf in (1, 6) and l == 2:
                    X[:] = 0
                    X[5:67] = sr.pss_seq(cell_id % 3)
                body = E @ X
                out.append(np.r_[body[N - cps[l]:], body])
    return np.concatenate(out)


def get_cell_ft(rows):
    """sync_ref.get_cell plus the frame type (ue_cell_search.c:216-242): FDD when more than the integer half of the winning id's rows say FDD."""
    n, out = sr.get_cell(rows)
    if n == 0:
        return 0, None
    g = (lambda r, k: r[k]) if isinstance(rows[0], dict) else getattr
    mine = [r for r in rows if g(r, "ret") == 1 and g(r, "cell_id") == out["cell_id"]]
    nof_fdd = sum(1 for r in mine if g(r, "frame_type") == FDD)
    out["frame_type"] = FDD if nof_fdd > len(mine) // 2 else TDD
    return n, out
