"""NumPy restatement of the reference's channel emulator: fading.c, delay.c, hst.c, rlf.c in channel.cc's order, plus this project's
counter-based noise stage. float64 where the value is defined by a formula (the frequency response, the filter, the Doppler rotation); the
reference's float casts where they decide an integer or a branch (delay in samples, the HST branch, the segment times, the tap frequency).
What it deliberately does not imitate: the recursive oscillators of srslte_vec_gen_sine / srslte_vec_apply_cfo, whose rounding drifts
(tests/test_channel_host.py measures the distance to outputs recorded from the reference's own sources, tests/golden/channel.npz)."""
import numpy as np

MODELS = {"none": 0, "epa": 1, "eva": 2, "etu": 3}
NOF_TAPS = (1, 7, 9, 9)
TAP_DELAY_NS = ((0,), (0, 30, 70, 90, 110, 190, 410), (0, 30, 150, 310, 370, 710, 1090, 1730, 2510), (0, 50, 120, 200, 230, 500, 1600, 2300, 5000))
TAP_POWER_DB = ((0.0,), (0.0, -1.0, -2.0, -3.0, -8.0, -17.2, -20.8), (0.0, -1.5, -1.4, -3.6, -0.6, -9.1, -7.0, -12.0, -16.9),
                (-1.0, -1.0, -1.0, 0.0, 0.0, 0.0, -3.0, -5.0, -7.0))
f32 = np.float32


def parse_model(s):
    """fading.c:53-83: "etu300" -> (3, 300.0)."""
    for name, m in MODELS.items():
        if s.startswith(name) and len(s) > len(name):
            return m, float(s[len(name):])
    raise ValueError("invalid channel model %r" % s)


def fft_size(model, srate):
    """fading.c:162-164; a negative exponent (undefined upstream: it is converted to unsigned) gives the floor of 64."""
    e = int(np.round(np.log2(float(f32(TAP_DELAY_NS[model][-1])) * 1e-9 * srate))) + 3
    return 64 if e < 6 else 1 << e


def mt19937_raw(seed, n):
    """n outputs of std::mt19937(seed) (init_genrand seeding, which numpy's legacy RandomState(seed) also uses)."""
    bg = np.random.MT19937()
    bg.state = np.random.RandomState(seed).get_state(legacy=False)
    return bg.random_raw(n).astype(np.uint32)


def uniform_real(raw, lo, hi):
    """std::uniform_real_distribution<float>(lo, hi) of libstdc++ on one 32-bit draw (random.cpp:36-40)."""
    u = f32(raw) / f32(4294967296.0)
    if u >= f32(1):
        u = np.nextafter(f32(1), f32(0))
    return f32(u * (f32(hi) - f32(lo)) + f32(lo))


def draw_coeffs(model, doppler, seed):
    """fading.c:168-175 -> a, w, p as doubles."""
    n = NOF_TAPS[model]
    raw = mt19937_raw(seed, 2 * n)
    a = np.array([float(uniform_real(raw[2 * i], 100, 2000)) for i in range(n)])
    p = np.array([float(uniform_real(raw[2 * i + 1], 0, f32(np.pi) / f32(2))) for i in range(n)])
    w = 2.0 * np.pi * float(f32(doppler)) / a
    return a, w, p


def timestamp_add(full, frac, add):
    """srslte_timestamp_add(t, 0, add), timestamp.c:73-84."""
    frac = frac + add
    r = np.floor(frac)
    return int(full + r), float(frac - r)


def block_time(full, frac, i, length, srate):
    return timestamp_add(full, frac, float(i * length) / srate)


def _mod_nsamples(period_s, init_time_s, srate, full, frac):
    period_n = int(np.round(f32(period_s) * f32(srate)))
    ts_n = full * int(srate) + int(np.round(frac * float(srate))) + int(f32(init_time_s)) * int(srate)
    return ts_n % period_n


def delay_nsamples(dmin_us, dmax_us, period_s, init_time_s, srate, full, frac):
    """delay.c:26-47."""
    t = _mod_nsamples(period_s, init_time_s, srate, full, frac) / float(srate)
    arg = 2.0 * np.pi * t / float(f32(period_s))
    delay_us = f32(float(f32(dmin_us)) + float(f32(dmax_us) - f32(dmin_us)) * (1.0 + np.sin(arg)) / 2.0)
    return int(np.round(float(delay_us) * float(srate) / 1e6))


def hst_fs(fd_hz, period_s, init_time_s, srate, full, frac):
    """hst.c:52-75 in float, ds_m = 300, dmin_m = 2."""
    t = f32(_mod_nsamples(period_s, init_time_s, srate, full, frac)) / f32(srate)
    T, costheta = f32(period_s), f32(0)
    k = (f32(2) * T / (f32(300) * f32(2))) ** 2
    if 0 <= t <= T / f32(2):
        num = T / f32(4) - t
        costheta = num / np.sqrt(f32(k + num * num))
    elif T / f32(2) < t < T:
        num = f32(-1.5) / f32(2) * T + t
        costheta = num / np.sqrt(f32(k + num * num))
    return f32(f32(fd_hz) * f32(costheta))


def rlf_on(t_on_ms, t_off_ms, full, frac):
    """rlf.c:34-39."""
    return float((full * 1000) % (t_on_ms + t_off_ms)) + frac * 1000 < t_on_ms


def philox4x32_10(c0, c1, k0, k1):
    """Philox-4x32-10 on counters (c0, c1, 0, 0) with key (k0, k1); the first two output words. uint64 arithmetic on arrays."""
    c0, c1 = np.asarray(c0, np.uint64), np.asarray(c1, np.uint64)
    c2, c3 = np.zeros_like(c0), np.zeros_like(c0)
    k0, k1, m32 = np.uint64(k0), np.uint64(k1), np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return c0.astype(np.uint32), c1.astype(np.uint32)


def awgn(n0, seed, channel, first, count):
    """The noise of samples first .. first + count - 1 of a channel: Box-Muller on the two words, variance n0 / 2 per component."""
    idx = np.arange(first, first + count, dtype=np.uint64)
    x0, x1 = philox4x32_10(idx & np.uint64(0xFFFFFFFF), idx >> np.uint64(32), seed, channel)
    u1 = ((x0 >> 9).astype(np.float64) + 0.5) / 8388608.0
    u2 = (x1 >> 8).astype(np.float64) / 16777216.0
    rad = np.sqrt(float(f32(n0)) / 2.0) * np.sqrt(-2.0 * np.log(u1))
    return rad * np.exp(2j * np.pi * u2)


class Fading:
    """srslte_channel_fading_t: init (fading.c:147-223) and execute (fading.c:249-275) with the frequency response computed per bin."""

    def __init__(self, srate, model, seed):
        self.model, self.doppler = parse_model(model)
        self.srate = f32(srate)
        self.N = fft_size(self.model, srate)
        self.path_delay = self.N // 4
        self.a, self.w, self.p = draw_coeffs(self.model, self.doppler, seed)
        nt = NOF_TAPS[self.model]
        self.amp = np.array([float(f32(10.0) ** (f32(TAP_POWER_DB[self.model][i]) / f32(20.0))) for i in range(nt)])
        # fading.c:94 in float: the tap's frequency in cycles per bin
        self.O = np.array([float((f32(TAP_DELAY_NS[self.model][i]) * f32(1e-9) * self.srate + f32(self.path_delay)) / f32(self.N)) for i in range(nt)])
        k = np.arange(self.N)
        self.E = np.exp(-2j * np.pi * np.outer(self.O, k))
        self.state = np.zeros(self.N, np.complex128)

    def h_freq(self, t):
        phase = (self.a * np.sin(self.w * t + self.p)).astype(f32).astype(np.float64)  # fading.c:85-88
        return ((self.amp / self.N * np.exp(-1j * phase))[:, None] * self.E).sum(0)

    def execute(self, x, t):
        N, out, cnt = self.N, np.empty(len(x), np.complex128), 0
        while cnt < len(x):
            n = min(N // 4, len(x) - cnt)
            temp = np.zeros(N, np.complex128)
            temp[:n] = x[cnt:cnt + n]
            temp = np.fft.ifft(np.fft.fft(temp) * self.h_freq(t)) * N + self.state
            out[cnt:cnt + n] = temp[:n]
            self.state = np.concatenate([temp[n:], np.zeros(n)])
            t += float(f32(n) / self.srate)  # fading.c:266: a float quotient added to the double
            cnt += n
        return out


class Delay:
    """srslte_channel_delay_execute (delay.c:99-126) on a plain FIFO."""

    def __init__(self):
        self.rb = np.zeros(0, np.complex128)

    def execute(self, x, d):
        n_read = min(d, len(x))
        n_copy = len(x) - n_read
        if len(self.rb) < d:
            self.rb = np.concatenate([self.rb, np.zeros(d - len(self.rb))])
        elif len(self.rb) > d:
            self.rb = self.rb[len(self.rb) - d:]
        out = np.concatenate([self.rb[:n_read], x[:n_copy]])
        self.rb = np.concatenate([self.rb[n_read:], x[n_copy:]])
        return out


class ChannelRef:
    """srslte::channel with one fading and one delay object per channel (channel.cc:45-67; seed0 + c * seed_stride for 0x1234 * port), run over
    [channel][block][len] arrays: block i at srslte_timestamp_add(t0, 0, i * len / srate)."""

    def __init__(self, srate, nof_channels, fading=None, seed0=0, seed_stride=0x1234, delay=None, hst=None, rlf=None, awgn=None):
        self.srate, self.C = int(srate), nof_channels
        self.fading = [Fading(srate, fading, seed0 + c * seed_stride) for c in range(nof_channels)] if fading else None
        self.delay_cfg, self.hst_cfg, self.rlf_cfg, self.awgn_cfg = delay, hst, rlf, awgn
        self.delay = [Delay() for _ in range(nof_channels)] if delay else None
        self.samples = 0
        self.N = self.fading[0].N if fading else 0
        self.path_delay = self.N // 4
        self.trace = []  # (delay in samples, Doppler shift in Hz, gate) per block

    def run(self, x, full, frac):
        x = np.asarray(x)
        C, nb, L = x.shape
        assert C == self.C
        out = np.empty((C, nb, L), np.complex128)
        for i in range(nb):
            fu, fr = block_time(full, frac, i, L, self.srate)
            d = delay_nsamples(*self.delay_cfg, self.srate, fu, fr) if self.delay_cfg else 0
            fs = hst_fs(*self.hst_cfg, self.srate, fu, fr) if self.hst_cfg else f32(0)
            on = rlf_on(*self.rlf_cfg, fu, fr) if self.rlf_cfg else True
            self.trace.append((d, float(fs), on))
            for c in range(C):
                v = x[c, i].astype(np.complex128)
                if self.fading:
                    v = self.fading[c].execute(v, fu + fr)
                if self.delay:
                    v = self.delay[c].execute(v, d)
                if self.hst_cfg:  # hst.c:78: cfo = -fs / srate in float, the phase from 0 in every block
                    v = v * np.exp(2j * np.pi * float(-fs / f32(self.srate)) * np.arange(L))
                if self.rlf_cfg:
                    v = v * (1.0 if on else 0.0)
                if self.awgn_cfg:
                    v = v + awgn(self.awgn_cfg[0], self.awgn_cfg[1], c, self.samples + i * L, L)
                out[c, i] = v
        self.samples += nb * L
        return out
