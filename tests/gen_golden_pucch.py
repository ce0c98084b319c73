"""Records tests/golden/pucch.npz from the reference's own pucch.c and refsignal_ul.c, compiled where they lie into a temporary directory outside
the tree and linked against oracle/_ref/libsrslte_ref.so (whose export map keeps srslte_pucch_* and srslte_refsignal_dmrs_pucch_* local).
phy_common.c (srslte_group_hopping_f_gh) and debug.c are compiled beside them. Nothing of the reference or compiled from it enters the tree: the
fixture holds recorded outputs only.

    python tests/gen_golden_pucch.py [REFERENCE_ROOT]

SWEEP_CELLS is also what tests/test_pucch_golden.py and tests/test_gpu_pucch_sweep.py run. Recorded per cell NAME:
  NAME.f1_prb [n][2], NAME.f2_prb [n][2]   srslte_pucch_n_prb of both slots for n_pucch 0 .. the first index out of band in either slot (the last
                                           row), formats 1-1b and 2-2b; a PRB outside the band (nof_prb, or the unsigned wrap) is stored as 0xFFFF
  NAME.f1_state [n][2][2][nsym][3]         n_cs, n_oc, n' of srslte_pucch_alpha_format1(is_dmrs = true) for subframes 0 and 9, both slots, every symbol
  NAME.f2_ncs [n][2][2][nsym]              n_cs of srslte_pucch_alpha_format2, likewise
  NAME.all_idx [4], NAME.all_f1 [4][20][nsym][3], NAME.all_f2 [4][20][nsym]   the same at all 20 slots for four indices
  NAME.rec_meta [r][8], NAME.rec_uci [r][15]   the full-signal records: format, n_pucch, tti, shortened, rnti, ack_len, cqi_len, ri_len and
                                           ack[2], ri, cqi[12] (records())
  NAME.enc_idx / enc_val [r][96 | 84 | 120 padded to 120], NAME.enc_n [r]   srslte_pucch_encode on a zeroed grid: the non-zero indices and values
  NAME.dmrs_r / dmrs_idx / dmrs_val [r][72 padded], NAME.dmrs_n [r]         srslte_refsignal_dmrs_pucch_gen, and _put on a zeroed grid
  NAME.dec_corr [r], NAME.dec [r][21]      srslte_chest_ul_estimate_pucch + srslte_pucch_decode on the sum of the two grids: correlation and
                                           detected, ack[2], ack.valid, cqi.data_crc, ri, pucch2_drs_bits[2], the decoded report's 13 bits
and r_uv_arg [30][12], srslte_refsignal_r_uv_arg_1prb of every u. A report of cqi_len bits is a higher-layer subband report (cqi.h: 4 + 2 N bits, or
9 with two codewords and a PMI), whose pack and unpack mirror each other, so the bits given are the bits coded."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "pucch.npz")

F1, F1A, F1B, F2, F2A, F2B = range(6)
# name -> (nof_prb, cell_id, cp_ext, group_hopping, delta_pucch_shift, N_cs, n_rb_2, N_pucch_1)
SWEEP_CELLS = {
    "S1": (6, 503, False, False, 1, 0, 0, 0),   # no mixed RB; 36 resources per RB; format 1 in band for n_pucch 0..431
    "S2": (6, 17, False, True, 2, 6, 1, 0),     # mixed RB, threshold 9
    "S3": (15, 150, True, False, 3, 6, 2, 0),   # extended CP, threshold 4
    "S4": (6, 301, True, True, 1, 7, 0, 0),     # extended CP, threshold 14, ceil(N_cs / 8) = 1
    "S5": (25, 200, False, True, 3, 3, 3, 0),   # wider band, for the PRB mapping
}
# the thresholds the recorded srslte_pucch_decode ran with: those of tests/test_gpu_ul_ctrl.py
TH = dict(threshold_format1=0.8, threshold_data_valid_format1a=0.9, threshold_data_valid_format2=1.5)
STATE_SF = (0, 9)
CQI_LENS = (4, 6, 8, 9, 10, 12)
OOB = 0xFFFF


def threshold(spec):
    """c N_cs / delta_pucch_shift: the first n_pucch outside the mixed RB."""
    return (2 if spec[2] else 3) * spec[5] // spec[4]


def last_in_band(spec, family):
    """The last n_pucch whose PRBs lie in the band: m < 2 nof_prb (36.211 5.4.3), from the definition of m alone."""
    P, _, ext, _, D, Ncs, nrb2, _ = spec
    if family == 2:
        return 24 * P - 1
    c = 2 if ext else 3
    return threshold(spec) + (2 * P - nrb2 - (Ncs + 7) // 8) * (c * 12 // D) - 1


def _n_oc_pairs(spec):
    """(n_oc of slot 0, n_oc of slot 1) -> the first n_pucch past the mixed RB with it, from 36.211 5.4.1 alone (not from the code under test)."""
    c, D, thr = (2 if spec[2] else 3), spec[4], threshold(spec)
    per, out = c * 12 // D, {}
    for n in range(thr, thr + per):
        n0 = n - thr
        n1 = (c * (n0 + 1)) % (per + 1) - 1
        out.setdefault((n0 * D // 12, n1 * D // 12), n)
    return out


def records(name):
    """The full-signal records of a cell: (format, n_pucch, tti, shortened, rnti, ack (2), ri, cqi bits). At most 16 a cell."""
    spec = SWEEP_CELLS[name]
    ext, thr, nrb2 = spec[2], threshold(spec), spec[6]
    L1, L2 = last_in_band(spec, 1), last_in_band(spec, 2)
    rng = np.random.default_rng(sum(name.encode()))
    out = []

    def f1(n, tti, sh, k):
        fmt, ack = [(F1, (0, 0)), (F1A, (1, 0)), (F1B, (0, 1)), (F1B, (1, 0)), (F1A, (0, 0)), (F1B, (1, 1)), (F1B, (0, 0))][k % 7]
        out.append((fmt, n, tti, sh, 0x46 + len(out), ack, 0, ()))

    def f2(n, tti, sh, k, rnti=None):
        fmt, ack, ln = [(F2, (0, 0), 12), (F2B if ext else F2A, (1, 0), 4), (F2B, (0, 1), 9), (F2, (0, 0), 0), (F2B, (1, 1), 6), (F2B, (1, 0), 0),
                        (F2, (0, 0), 10), (F2B if ext else F2A, (0, 0), 8)][k % 8]
        out.append((fmt, n, tti, sh, rnti if rnti is not None else 0x146 + len(out), ack, int(rng.integers(0, 2)) if ln == 0 else 0,
                    tuple(int(b) for b in rng.integers(0, 2, ln))))

    pairs = _n_oc_pairs(spec)
    if name == "S1":  # every n_oc of both slots, shortened and not, at the first and at a late RB pair; the two RNTI edges of format 2
        want, k = set(), 0
        for (a, b), n in sorted(pairs.items(), key=lambda x: x[1]):
            if not {(0, a), (1, b)} <= want:
                want |= {(0, a), (1, b)}
                f1(n, 19 + 10 * k, False, k)
                f1(n + 36 * 7, 20 + 10 * k, True, k + 3)
                k += 1
        f2(5, 9, False, 0, rnti=0xFFF2)
        f2(77, 123, True, 2, rnti=0x000B)
    else:  # n_oc 2 (1 on the extended CP) in each slot, one shortened
        top = 1 if ext else 2
        f1(min(n for (a, b), n in pairs.items() if a == top), 4, True, 2)
        f1(min(n for (a, b), n in pairs.items() if b == top), 9, False, 5)
    if thr:  # both sides of c N_cs / delta, in both slots' remapping
        f1(thr - 1, 10, False, 1)
        f1(thr, 1009, True, 3)
        f1(0, 5, True, 6)
    if nrb2:  # both sides of 12 n_rb_2
        f2(12 * nrb2 - 1, 39, False, 1)
        f2(12 * nrb2, 40, True, 2)
        f2(12 * nrb2 + 7, 8, False, 4)
    f1(L1, 7, name in ("S2", "S4"), 0 if name == "S3" else 1)  # the last in-band index of each family
    f2(L2, 6, False, 3 if name == "S4" else 5 if name == "S2" else 6)
    f2(L2 // 2, 13, True, 7)
    assert len(out) <= 16, (name, len(out))
    return out


SHIM = r"""
/* Plain-argument entries to the PUCCH functions of pucch.c and refsignal_ul.c. */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "srslte/phy/ch_estimation/chest_ul.h"
#include "srslte/phy/ch_estimation/refsignal_ul.h"
#include "srslte/phy/phch/cqi.h"
#include "srslte/phy/phch/pucch.h"
typedef struct {
  srslte_cell_t         cell;
  srslte_pucch_t        ue, enb;
  srslte_refsignal_ul_t rs;
  srslte_chest_ul_t     chest;
  cf_t*                 ce;
} rec_t;
void* rec_new(uint32_t nof_prb, uint32_t cell_id, int cp_ext)
{
  rec_t* q = calloc(1, sizeof(*q));
  memset(&q->cell, 0, sizeof(q->cell));
  q->cell.nof_prb = nof_prb, q->cell.nof_ports = 1, q->cell.id = cell_id, q->cell.cp = cp_ext ? SRSLTE_CP_EXT : SRSLTE_CP_NORM;
  srslte_refsignal_dmrs_pusch_cfg_t d;
  memset(&d, 0, sizeof(d));
  if (srslte_pucch_init_ue(&q->ue) || srslte_pucch_set_cell(&q->ue, q->cell) || srslte_pucch_init_enb(&q->enb) || srslte_pucch_set_cell(&q->enb, q->cell) ||
      srslte_refsignal_ul_init(&q->rs, nof_prb) || srslte_refsignal_ul_set_cell(&q->rs, q->cell) || srslte_chest_ul_init(&q->chest, nof_prb) ||
      srslte_chest_ul_set_cell(&q->chest, q->cell))
    return NULL;
  srslte_chest_ul_pregen(&q->chest, &d);
  q->ce = calloc(2 * 7 * 12 * nof_prb, sizeof(cf_t));
  return q;
}
void rec_free(void* p)
{
  rec_t* q = p;
  srslte_pucch_free(&q->ue), srslte_pucch_free(&q->enb), srslte_refsignal_ul_free(&q->rs), srslte_chest_ul_free(&q->chest);
  free(q->ce), free(q);
}
static void mk(const uint32_t* c, const float* th, srslte_pucch_cfg_t* p)
{ /* delta_pucch_shift, N_cs, n_rb_2, N_pucch_1, group hopping, format, n_pucch, rnti, ack_len, cqi_len, ri_len */
  memset(p, 0, sizeof(*p));
  p->delta_pucch_shift = c[0], p->N_cs = c[1], p->n_rb_2 = c[2], p->N_pucch_1 = c[3], p->group_hopping_en = c[4] != 0;
  p->format = (srslte_pucch_format_t)c[5], p->n_pucch = c[6], p->rnti = (uint16_t)c[7];
  p->uci_cfg.ack[0].nof_acks = c[8];
  if (c[9]) {
    p->uci_cfg.cqi.data_enable = true, p->uci_cfg.cqi.type = SRSLTE_CQI_TYPE_SUBBAND_HL;
    if (c[9] == 9)
      p->uci_cfg.cqi.N = 0, p->uci_cfg.cqi.rank_is_not_one = p->uci_cfg.cqi.pmi_present = true;
    else
      p->uci_cfg.cqi.N = (c[9] - 4) / 2;
  }
  p->uci_cfg.cqi.ri_len = c[10];
  if (th) p->threshold_format1 = th[0], p->threshold_data_valid_format1a = th[1], p->threshold_data_valid_format2 = th[2];
}
uint32_t rec_n_prb(void* p, const uint32_t* c, uint32_t ns)
{
  rec_t*             q = p;
  srslte_pucch_cfg_t cfg;
  mk(c, NULL, &cfg);
  return srslte_pucch_n_prb(&q->cell, &cfg, ns);
}
static uint32_t n_cs_of(float alpha) { return (uint32_t)lroundf(alpha * 12 / (2 * (float)M_PI)); }
/* out [nsym][3]: n_cs, n_oc, n' */
void rec_alpha1(void* p, const uint32_t* c, uint32_t ns, uint32_t nsym, uint8_t* out)
{
  rec_t*             q = p;
  srslte_pucch_cfg_t cfg;
  mk(c, NULL, &cfg);
  for (uint32_t l = 0; l < nsym; l++) {
    uint32_t n_oc = 0, n_prime = 0;
    out[3 * l] = (uint8_t)n_cs_of(srslte_pucch_alpha_format1(q->rs.n_cs_cell, &cfg, q->cell.cp, true, ns, l, &n_oc, &n_prime));
    out[3 * l + 1] = (uint8_t)n_oc, out[3 * l + 2] = (uint8_t)n_prime;
    if (n_oc > 255 || n_prime > 255) abort();
  }
}
void rec_alpha2(void* p, const uint32_t* c, uint32_t ns, uint32_t nsym, uint8_t* out)
{
  rec_t*             q = p;
  srslte_pucch_cfg_t cfg;
  mk(c, NULL, &cfg);
  for (uint32_t l = 0; l < nsym; l++) out[l] = (uint8_t)n_cs_of(srslte_pucch_alpha_format2(q->rs.n_cs_cell, &cfg, ns, l));
}
/* uci: ack[2], ri, cqi bits[12] */
int rec_encode(void* p, const uint32_t* c, uint32_t tti, int shortened, const uint8_t* uci, cf_t* grid)
{
  rec_t*             q = p;
  srslte_pucch_cfg_t cfg;
  srslte_ul_sf_cfg_t sf;
  srslte_uci_value_t v;
  mk(c, NULL, &cfg);
  memset(&sf, 0, sizeof(sf)), memset(&v, 0, sizeof(v));
  sf.tti = tti, sf.shortened = shortened != 0;
  v.ack.ack_value[0] = uci[0], v.ack.ack_value[1] = uci[1], v.ri = uci[2];
  if (c[9]) {
    uint8_t bits[SRSLTE_CQI_MAX_BITS] = {0};
    memcpy(bits, uci + 3, c[9]);
    srslte_cqi_value_unpack(&cfg.uci_cfg.cqi, bits, &v.cqi);
  }
  return srslte_pucch_encode(&q->ue, &sf, &cfg, &v, grid);
}
int rec_dmrs(void* p, const uint32_t* c, uint32_t tti, int shortened, const uint8_t* drs, cf_t* r, cf_t* grid)
{
  rec_t*             q = p;
  srslte_pucch_cfg_t cfg;
  srslte_ul_sf_cfg_t sf;
  mk(c, NULL, &cfg);
  memset(&sf, 0, sizeof(sf));
  sf.tti = tti, sf.shortened = shortened != 0;
  cfg.pucch2_drs_bits[0] = drs[0], cfg.pucch2_drs_bits[1] = drs[1];
  if (srslte_refsignal_dmrs_pucch_gen(&q->rs, &sf, &cfg, r)) return -1;
  return srslte_refsignal_dmrs_pucch_put(&q->rs, &cfg, r, grid);
}
/* out: detected, ack[2], ack.valid, cqi.data_crc, ri, pucch2_drs_bits[2], the report's bits[13] */
int rec_decode(void* p, const uint32_t* c, const float* th, uint32_t tti, int shortened, cf_t* grid, float* corr, uint8_t* out)
{
  rec_t*                q = p;
  srslte_pucch_cfg_t    cfg;
  srslte_ul_sf_cfg_t    sf;
  srslte_chest_ul_res_t res;
  srslte_pucch_res_t    data;
  mk(c, th, &cfg);
  memset(&sf, 0, sizeof(sf)), memset(&res, 0, sizeof(res)), memset(&data, 0, sizeof(data));
  sf.tti = tti, sf.shortened = shortened != 0;
  res.ce = q->ce;
  if (srslte_chest_ul_estimate_pucch(&q->chest, &sf, &cfg, grid, &res)) return -1;
  if (srslte_pucch_decode(&q->enb, &sf, &cfg, &res, grid, &data)) return -2;
  *corr  = data.correlation;
  out[0] = data.detected, out[1] = data.uci_data.ack.ack_value[0], out[2] = data.uci_data.ack.ack_value[1], out[3] = data.uci_data.ack.valid;
  out[4] = data.uci_data.cqi.data_crc, out[5] = data.uci_data.ri, out[6] = cfg.pucch2_drs_bits[0], out[7] = cfg.pucch2_drs_bits[1];
  memset(out + 8, 0, 13);
  if (c[9]) {
    uint8_t bits[SRSLTE_CQI_MAX_BITS] = {0};
    srslte_cqi_value_pack(&cfg.uci_cfg.cqi, &data.uci_data.cqi, bits);
    memcpy(out + 8, bits, c[9]);
  }
  return 0;
}
"""


def build_recorder(ref_root, tmp):
    import subprocess
    root = os.path.dirname(HERE)
    ref_so_dir = os.path.join(root, "oracle", "_ref")
    lib = os.path.join(ref_root, "lib")
    shim = os.path.join(tmp, "shim.c")
    with open(shim, "w") as f:
        f.write(SHIM)
    srcs = [os.path.join(lib, "src/phy/phch/pucch.c"), os.path.join(lib, "src/phy/ch_estimation/refsignal_ul.c"),
            os.path.join(lib, "src/phy/common/phy_common.c"), os.path.join(lib, "src/phy/utils/debug.c"), shim]
    out = os.path.join(tmp, "librec.so")
    # the reference's release flags (oracle/ref.mk): -Ofast -mfma decides how w + tmp_arg[n] + alpha * n + S_ns rounds. pucch.c includes the umbrella
    # header, which wants the generated version.h: its guard is pre-defined and what it would have brought is force-included, as oracle/ref.mk does
    cmd = ["gcc", "-std=gnu99", "-D_GNU_SOURCE", "-O3", "-fno-trapping-math", "-fno-math-errno", "-Ofast", "-funroll-loops", "-mfpmath=sse", "-mavx2", "-mfma",
           "-DLV_HAVE_SSE", "-DLV_HAVE_AVX", "-DLV_HAVE_AVX2", "-DLV_HAVE_FMA", "-fPIC", "-w", "-DSRSLTE_SRSLTE_H", "-include", "complex.h", "-include", "math.h",
           "-include", "srslte/config.h", "-include", "srslte/phy/utils/debug.h", "-include", "srslte/phy/phch/uci.h", "-include", "srslte/phy/modem/mod.h",
           "-I" + os.path.join(lib, "include"), "-shared", "-Wl,-z,defs", "-o", out] + srcs
    cmd += ["-L" + ref_so_dir, "-lsrslte_ref", "-Wl,-rpath," + ref_so_dir, "-lm", "-lpthread"]
    subprocess.check_call(cmd)
    return out


def cfg_words(spec, fmt=0, n_pucch=0, rnti=0, ack_len=0, cqi_len=0, ri_len=0):
    return np.array([spec[4], spec[5], spec[6], spec[7], int(spec[3]), fmt, n_pucch, rnti, ack_len, cqi_len, ri_len], np.uint32)


def rec_lengths(fmt, ack, cqi):
    """ack_len, cqi_len, ri_len of a record."""
    if fmt < F2:
        return (0, 1, 2)[fmt], 0, 0
    return (0, 1, 2)[fmt - F2], len(cqi), 0 if cqi else 1


def record(ref_root):
    import ctypes as C
    import tempfile
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        L = C.CDLL(build_recorder(ref_root, tmp))
        vp, u32 = C.c_void_p, C.c_uint32
        L.rec_new.restype = vp
        L.rec_new.argtypes = [u32, u32, C.c_int]
        L.rec_free.argtypes = [vp]
        L.rec_n_prb.restype = u32
        L.rec_n_prb.argtypes = [vp, vp, u32]
        L.rec_alpha1.argtypes = L.rec_alpha2.argtypes = [vp, vp, u32, u32, vp]
        L.rec_encode.argtypes = [vp, vp, u32, C.c_int, vp, vp]
        L.rec_dmrs.argtypes = [vp, vp, u32, C.c_int, vp, vp, vp]
        L.rec_decode.argtypes = [vp, vp, vp, u32, C.c_int, vp, vp, vp]
        L.srslte_refsignal_r_uv_arg_1prb.argtypes = [vp, u32]
        th = np.array([TH["threshold_format1"], TH["threshold_data_valid_format1a"], TH["threshold_data_valid_format2"]], np.float32)
        arg = np.zeros((30, 12), np.float32)
        for u in range(30):
            L.srslte_refsignal_r_uv_arg_1prb(arg[u].ctypes.data, u)
        res["r_uv_arg"] = arg
        for name, spec in sorted(SWEEP_CELLS.items()):
            P, cell_id, ext = spec[0], spec[1], spec[2]
            nsym = 6 if ext else 7
            q = L.rec_new(P, cell_id, 1 if ext else 0)
            assert q, name

            def prbs(fmt, n):
                w = cfg_words(spec, fmt, n)
                v = [L.rec_n_prb(q, w.ctypes.data, s) for s in range(2)]
                return [x if x < P else OOB for x in v]

            def state(fmt, n, ns):
                w = cfg_words(spec, fmt, n)
                o = np.zeros((nsym, 3) if fmt < F2 else nsym, np.uint8)
                (L.rec_alpha1 if fmt < F2 else L.rec_alpha2)(q, w.ctypes.data, ns, nsym, o.ctypes.data)
                return o

            for fam, fmt in ((1, F1A), (2, F2)):
                rows, n = [], 0
                while True:
                    rows.append(prbs(fmt, n))
                    if OOB in rows[-1]:
                        break
                    n += 1
                assert n == last_in_band(spec, fam) + 1, (name, fam, n)  # the reference's band edge is the definition's
                res["%s.f%d_prb" % (name, fam)] = np.array(rows, np.uint16)
                res["%s.f%d_%s" % (name, fam, "state" if fam == 1 else "ncs")] = np.array(
                    [[[state(fmt, k, 2 * sf + s) for s in range(2)] for sf in STATE_SF] for k in range(n + 1)], np.uint8)
            thr = threshold(spec)
            allidx = sorted({max(thr - 1, 0), thr + 1, 12 * spec[6] + 3, last_in_band(spec, 1) - 5})
            allidx += [k for k in (50, 51, 52, 53) if k not in allidx][:4 - len(allidx)]
            res[name + ".all_idx"] = np.array(allidx, np.uint16)
            res[name + ".all_f1"] = np.array([[state(F1A, k, ns) for ns in range(20)] for k in allidx], np.uint8)
            res[name + ".all_f2"] = np.array([[state(F2, k, ns) for ns in range(20)] for k in allidx], np.uint8)
            recs = records(name)
            R, glen = len(recs), 2 * nsym * 12 * P
            meta, uci = np.zeros((R, 8), np.uint32), np.zeros((R, 15), np.uint8)
            enc_idx, enc_val, enc_n = np.zeros((R, 120), np.uint32), np.zeros((R, 120), np.complex64), np.zeros(R, np.uint16)
            d_r, d_idx, d_val, d_n = np.zeros((R, 72), np.complex64), np.zeros((R, 72), np.uint32), np.zeros((R, 72), np.complex64), np.zeros(R, np.uint16)
            dec_corr, dec = np.zeros(R, np.float32), np.zeros((R, 21), np.uint8)
            for i, (fmt, n, tti, sh, rnti, ack, ri, cqi) in enumerate(recs):
                ack_len, cqi_len, ri_len = rec_lengths(fmt, ack, cqi)
                assert cqi_len == 0 or cqi_len in CQI_LENS
                w = cfg_words(spec, fmt, n, rnti, ack_len, cqi_len, ri_len)
                meta[i] = (fmt, n, tti, int(sh), rnti, ack_len, cqi_len, ri_len)
                uci[i, :3], uci[i, 3:3 + cqi_len] = (ack[0], ack[1], ri), cqi
                g = np.zeros(glen, np.complex64)
                assert L.rec_encode(q, w.ctypes.data, tti, int(sh), uci[i].ctypes.data, g.ctypes.data) == 0, (name, i)
                nz = np.flatnonzero(g)  # unit-modulus values: none is zero
                assert nz.size == ((4 + (3 if sh else 4)) * 12 if fmt < F2 else 120), (name, i, nz.size)
                enc_n[i], enc_idx[i, :nz.size], enc_val[i, :nz.size] = nz.size, nz, g[nz]
                drs = np.array(ack if fmt > F2 else (0, 0), np.uint8)
                r, gd = np.zeros(72, np.complex64), np.zeros(glen, np.complex64)
                assert L.rec_dmrs(q, w.ctypes.data, tti, int(sh), drs.ctypes.data, r.ctypes.data, gd.ctypes.data) == 0, (name, i)
                nzd = np.flatnonzero(gd)
                # 2b on the extended CP: the DMRS symbols {1, 5} of refsignal_ul.c:544-548 are data symbols too, and the DMRS, put second, stays
                assert not np.intersect1d(nz, nzd).size or (ext and fmt > F2)
                d_n[i], d_r[i, :nzd.size], d_idx[i, :nzd.size], d_val[i, :nzd.size] = nzd.size, r[:nzd.size], nzd, gd[nzd]
                rx, corr = g.copy(), np.zeros(1, np.float32)
                rx[nzd] = gd[nzd]
                assert L.rec_decode(q, w.ctypes.data, th.ctypes.data, tti, int(sh), rx.ctypes.data, corr.ctypes.data, dec[i].ctypes.data) == 0, (name, i)
                dec_corr[i] = corr[0]
            for k, v in (("rec_meta", meta), ("rec_uci", uci), ("enc_idx", enc_idx), ("enc_val", enc_val), ("enc_n", enc_n), ("dmrs_r", d_r), ("dmrs_idx", d_idx),
                         ("dmrs_val", d_val), ("dmrs_n", d_n), ("dec_corr", dec_corr), ("dec", dec)):
                res["%s.%s" % (name, k)] = v
            L.rec_free(q)
    check_coverage(res)
    return res


def check_coverage(res):
    """What the records must reach over the five cells, read from the recorded state itself."""
    fmts, noc, rntis = set(), set(), set()
    for name, spec in SWEEP_CELLS.items():
        thr, meta = threshold(spec), res[name + ".rec_meta"]
        ns = {(int(m[0]) >= F2, int(m[1])) for m in meta}
        for m in meta:
            fmt, n, tti, sh, rnti = (int(x) for x in m[:5])
            fmts.add(fmt)
            if fmt < F2:
                for s in range(2):
                    noc.add((int(res[name + ".f1_state"][n, 0, s, 0, 1]), s, sh))
            elif spec[1] == 503 and tti % 10 == 9 or rnti == 0x000B:
                rntis.add(rnti)
        assert (False, last_in_band(spec, 1)) in ns and (True, last_in_band(spec, 2)) in ns, name
        if thr:
            assert {(False, thr - 1), (False, thr)} <= ns, name
        if spec[6]:
            assert {(True, 12 * spec[6] - 1), (True, 12 * spec[6])} <= ns, name
    assert fmts == set(range(6)), fmts
    assert noc >= {(k, s, sh) for k in range(3) for s in range(2) for sh in range(2)}, sorted(noc)
    assert rntis >= {0xFFF2, 0x000B}, rntis


def save(res, path=GOLDEN):
    """A byte-identical archive for identical arrays: fixed names order and time stamps (numpy's savez stamps each member with the clock)."""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(res):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(res[k]), version=(1, 0))
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type, info.external_attr = zipfile.ZIP_DEFLATED, 0o644 << 16
            z.writestr(info, b.getvalue(), compresslevel=9)


if __name__ == "__main__":
    sys.path.insert(0, HERE)
    res = record(sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
    save(res)
    print("wrote %s: %d arrays, %d bytes" % (GOLDEN, len(res), os.path.getsize(GOLDEN)))
