"""NumPy restatement of the reference's PRACH (lib/src/phy/phch/prach.c) for FDD preamble formats 0-3, in double precision: the numerology and
sequences of srslte_prach_set_cell_ / srslte_prach_gen_seqs (:224-322, :394-508), srslte_prach_gen (:510-549), srslte_prach_detect_offset
(:564-666) and srslte_prach_tti_opportunity_config_fdd (:82-104). srslte_dft semantics: `norm` scales by 1/sqrt(N); `mirror` swaps the two
halves (the input of a backward transform, the output of a forward one). Tables restated from 36.211."""
import math

import numpy as np

NZC = 839
# 36.211 Table 5.7.2-4: logical roots 2i and 2i+1 are the physical roots u and 839 - u; u of each pair
_ROOT_FIRST = [int(x) for x in """
    129 140 120 210 168 84 105 93 70 60 2 1 56 112 148 80 42 40 35 73 146 31 28 30
    27 29 24 48 68 74 178 136 86 78 43 39 20 21 95 202 190 181 137 125 151 217 128 142
    122 203 118 110 89 103 61 55 15 14 12 23 34 37 46 207 179 145 130 223 228 227 132 133
    143 135 161 201 173 106 83 91 66 53 10 9 7 8 16 47 64 57 104 101 108 208 184 197
    191 121 141 149 216 218 152 144 134 138 199 162 176 119 158 164 174 171 170 87 169 88 107 81
    82 100 98 71 59 65 50 49 26 17 13 6 5 33 51 75 99 96 97 166 172 175 187 163
    185 200 114 189 115 194 195 192 182 157 156 211 154 123 139 212 153 213 215 150 225 224 221 220
    127 147 124 193 205 206 116 160 186 167 79 85 77 92 58 62 69 54 36 32 25 18 11 4
    3 19 22 41 38 44 52 45 63 67 72 76 94 102 90 109 165 111 209 204 117 188 159 198
    113 183 180 177 196 155 214 126 131 219 222 226 230 232 262 252 418 416 413 411 376 395 283 285
    379 390 363 384 388 386 361 387 360 310 354 328 315 337 349 335 324 323 320 334 359 295 385 292
    291 381 399 380 397 369 377 410 407 281 414 247 277 271 272 264 259 237 239 244 243 275 278 250
    246 417 248 394 393 370 365 300 299 364 362 298 312 313 314 353 352 343 327 350 326 319 332 333
    348 347 322 330 338 341 340 342 301 366 401 371 408 375 249 269 238 234 257 273 255 254 245 251
    412 372 282 403 396 392 391 382 389 294 297 311 344 345 318 331 325 321 346 339 351 306 289 400
    378 374 415 270 241 231 260 268 276 409 398 290 304 308 358 316 293 288 284 368 253 256 263 242
    274 402 383 357 329 317 307 286 287 266 261 236 303 356 355 405 404 406 235 267 302 309 265 233
    367 296 336 305 373 280 279 419 240 258 229
""".split()]
NCS_UNRESTRICTED = [0, 13, 15, 18, 22, 26, 32, 38, 46, 59, 76, 93, 119, 167, 279, 419]  # Table 5.7.2-2
T_CP = [3168, 21024, 6240, 21024]                                                        # Table 5.7.1-1, units of T_s
T_SEQ = [24576, 24576, 2 * 24576, 2 * 24576]
# Table 5.7.1-2 (FDD) by config_idx % 16: subframe numbers (14: every subframe; srslte's table has none for 30 / 46 / 62)
FDD_SF = [(1,), (4,), (7,), (1,), (4,), (7,), (1, 6), (2, 7), (3, 8), (1, 4, 7), (2, 5, 8), (3, 6, 9), (0, 2, 4, 6, 8), (1, 3, 5, 7, 9), (), (9,)]
SYMBOL_SZ = [(6, 128), (15, 256), (25, 384), (50, 768), (75, 1024), (110, 1536)]
NOF_PRB_OF_SZ = {128: 6, 256: 15, 384: 25, 768: 50, 1024: 75, 1536: 100}


def zc_root(logical):
    i = logical % 838
    u = _ROOT_FIRST[i // 2]
    return NZC - u if i & 1 else u


def symbol_sz(nof_prb):
    for p, n in SYMBOL_SZ:
        if nof_prb <= p:
            return n
    raise ValueError(nof_prb)


def tti_opportunity_fdd(config_idx, tti, allowed_subframe=-1):
    if config_idx == 14:
        return True
    even_only = config_idx % 16 < 3 or config_idx % 16 == 15
    if even_only and (tti // 10) % 2 != 0:
        return False
    sf = tti % 10
    return sf in FDD_SF[config_idx % 16] and (allowed_subframe == -1 or sf == allowed_subframe)


class Prach:
    """srslte_prach_t after srslte_prach_init(symbol_sz(nof_prb)) + srslte_prach_set_cell_ (unrestricted set, FDD)."""

    def __init__(self, nof_prb, config_idx, root_seq_idx=0, zero_corr_zone=1, detect_factor=18.0):
        assert config_idx < 64 and root_seq_idx < 838 and zero_corr_zone < 16
        self.nof_prb, self.config_idx, self.rsi, self.zczc = nof_prb, config_idx, root_seq_idx, zero_corr_zone
        self.f = config_idx // 16
        self.detect_factor = detect_factor
        self.N_ifft_ul = symbol_sz(nof_prb)
        self.N_rb_ul = NOF_PRB_OF_SZ[self.N_ifft_ul]
        self.N_zc, self.N_cs = NZC, NCS_UNRESTRICTED[zero_corr_zone]
        self.N_ifft_prach = self.N_ifft_ul * 15000 // 1250
        self.N_seq = T_SEQ[self.f] * self.N_ifft_ul // 2048
        self.N_cp = T_CP[self.f] * self.N_ifft_ul // 2048
        self.nof_sf = math.ceil((T_SEQ[self.f] + T_CP[self.f]) / 30720.0)
        # srslte_prach_gen_seqs, normal cell
        v_max = 0 if self.N_cs == 0 else NZC // self.N_cs - 1
        self.root_seqs_idx, self.seqs = [], np.zeros((64, NZC), complex)
        v, j = v_max + 1, np.arange(NZC)
        for i in range(64):
            if v > v_max:
                u = zc_root(self.rsi + len(self.root_seqs_idx))
                root = np.exp(-1j * np.pi * u * j * (j + 1) / NZC)
                self.root_seqs_idx.append(i)
                v = 0
            self.seqs[i] = root[(j + v * self.N_cs) % NZC]
            v += 1
        self.N_roots = len(self.root_seqs_idx)
        self.n_wins = NZC // (self.N_cs if self.N_cs else NZC)
        self.max_det = self.N_roots * self.n_wins
        self.dft_seqs = np.fft.fft(self.seqs, axis=1) / np.sqrt(NZC)  # zc_fft: forward, norm, no mirror

    def begin(self, freq_offset):
        k_0 = freq_offset * 12 - self.N_rb_ul * 12 // 2 + self.N_ifft_ul // 2
        return 7 + 12 * k_0 + 12 // 2

    def gen(self, seq_index, freq_offset):
        """srslte_prach_gen -> N_cp + N_seq complex samples."""
        N, b = self.N_ifft_prach, self.begin(freq_offset)
        x = np.zeros(N, complex)
        x[b:b + NZC] = self.dft_seqs[seq_index]
        out = np.fft.ifft(np.fft.fftshift(x)) * np.sqrt(N)  # backward, mirror, norm: N ifft / sqrt(N)
        return np.concatenate([out[N - self.N_cp:], out[np.arange(self.N_seq) % N]])

    def correlations(self, freq_offset, signal):
        """|IDFT(bins conj(dft root))|^2 per root -> [N_roots][839]."""
        N, b = self.N_ifft_prach, self.begin(freq_offset)
        spec = np.fft.fftshift(np.fft.fft(np.asarray(signal, complex)[:N]))  # forward, mirror, no norm
        bins = spec[b:b + NZC]
        prod = bins[None, :] * np.conj(self.dft_seqs[self.root_seqs_idx])
        return np.abs(np.fft.ifft(prod, axis=1) * NZC) ** 2  # zc_ifft: backward, no norm

    def detect_offset(self, freq_offset, signal):
        """srslte_prach_detect_offset -> (indices, t_offsets float32, peak_to_avg)."""
        assert len(signal) >= self.N_ifft_prach
        corr = self.correlations(freq_offset, signal)
        win = self.N_cs if self.N_cs else NZC
        idx, toff, p2a = [], [], []
        for i in range(self.N_roots):
            ave = corr[i].sum() / NZC
            for j in range(self.n_wins):
                start = (NZC - j * self.N_cs) % NZC
                w = corr[i, start:start + win]
                k = int(np.argmax(w))  # the first maximum
                peak = w[k]
                if peak > self.detect_factor * ave:
                    c = np.float32(1.8) if k <= 30 else (np.float32(1.9) if k <= 250 else np.float32(1.91))
                    idx.append(i * self.n_wins + j)
                    toff.append(np.float32(c * np.float32(k)) / np.float32(1250 * NZC))
                    p2a.append(peak / ave)
        return np.array(idx, np.uint32), np.array(toff, np.float32), np.array(p2a)
