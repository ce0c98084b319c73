"""Records tests/golden/srs.npz from the reference's own refsignal_ul.c, compiled where it lies into a temporary directory outside the tree and
linked against oracle/_ref/libsrslte_ref.so (whose export map keeps srslte_refsignal_srs_* local). phy_common.c (srslte_group_hopping_f_gh) and debug.c are
compiled beside it; the PUCCH functions refsignal_ul.c names but the SRS never reaches are stubbed in the shim. Nothing of the
reference or compiled from it enters the tree: the fixture holds recorded outputs only.

    python tests/gen_golden_srs.py [REFERENCE_ROOT]

CASES is also what tests/test_srs_host.py and tests/test_gpu_srs.py run. Recorded: srslte_refsignal_srs_gen and srslte_refsignal_srs_put (on a zeroed
grid: the non-zero indices and their values) for every TTI of every case, M_sc, srslte_refsignal_srs_send_cs over the 15 x 10 pairs,
srslte_refsignal_srs_send_ue over I_srs 0-636 x SEND_UE_TTIS, srslte_refsignal_srs_rb_start_cs / _rb_L_cs over BW_PRBS x 8, and the two
shortened decisions over the drawn inputs of shortened_inputs(). The 32 row_* cases - one per (band, bw_cfg) row of 36.211 Tables 5.5.3.2-1..4 - are
recorded at two TTIs; the HOP_CASES at every occasion of one hopping period and one more, the first index of srslte_refsignal_srs_put alone
(.put_idx0); and sweep_M_sc / sweep_k0 hold srslte_refsignal_srs_M_sc and the first put index for every B and n_rrc of every row without hopping."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "srs.npz")


def _occ(I_srs, n, first=0):
    """n consecutive occasions of I_srs from the first-th on (36.213 Table 8.2-1)."""
    for lo, T in ((0, 2), (2, 5), (7, 10), (17, 20), (37, 40), (77, 80), (157, 160), (317, 320)):
        if I_srs < lo + T:
            return [I_srs - lo + T * (first + k) for k in range(n)]
    raise ValueError(I_srs)


# name -> the cell, the common and the UE-specific configuration, and the TTIs the SRS is generated and put at
CASES = {
    # M_sc 24: the 24-entry phi table, J = 3; T_srs 160
    "p6_bw7": dict(nof_prb=6, cell_id=1, cp_ext=False, bw_cfg=7, subframe_config=0, gh=False, sh=False, delta_ss=0, B=0, b_hop=3, n_srs=0, I_srs=160,
                   k_tc=0, n_rrc=0, ttis=_occ(160, 2)),
    # M_sc 144: a Zadoff-Chu sequence of 12 PRB with sequence hopping on (v from delta_ss 7); T_srs 5
    "p25_bw2_B0": dict(nof_prb=25, cell_id=200, cp_ext=False, bw_cfg=2, subframe_config=3, gh=False, sh=True, delta_ss=7, B=0, b_hop=3, n_srs=7, I_srs=3,
                       k_tc=1, n_rrc=0, ttis=_occ(3, 10, 5)),
    # B 1 under b_hop 0 with N_1 = 6: six hop positions over consecutive occasions (seven, to see the wrap); T_srs 10
    "p25_bw2_B1_hop": dict(nof_prb=25, cell_id=77, cp_ext=False, bw_cfg=2, subframe_config=9, gh=False, sh=False, delta_ss=0, B=1, b_hop=0, n_srs=2, I_srs=8,
                           k_tc=0, n_rrc=3, ttis=_occ(8, 7, 11)),
    # the full hopping tree, N_1 N_2 N_3 = 2 2 3 (even and odd N_b), 13 occasions; group hopping on; T_srs 2
    "p50_bw0_B3_hop": dict(nof_prb=50, cell_id=150, cp_ext=False, bw_cfg=0, subframe_config=0, gh=True, sh=False, delta_ss=0, B=3, b_hop=0, n_srs=5, I_srs=0,
                           k_tc=1, n_rrc=5, ttis=_occ(0, 13, 100)),
    # extended CP, M_sc 72 (6 PRB: the smallest with sequence hopping), group and sequence hopping on, partial hopping (b_hop 1 < B 2); T_srs 20
    "p75_bw3_ext": dict(nof_prb=75, cell_id=301, cp_ext=True, bw_cfg=3, subframe_config=7, gh=True, sh=True, delta_ss=3, B=2, b_hop=1, n_srs=3, I_srs=20,
                        k_tc=0, n_rrc=17, ttis=_occ(20, 4, 9)),
    # M_sc 576, J = 72: two wavefronts; T_srs 320
    "p100_bw0_B0": dict(nof_prb=100, cell_id=5, cp_ext=False, bw_cfg=0, subframe_config=14, gh=False, sh=False, delta_ss=0, B=0, b_hop=3, n_srs=0, I_srs=320,
                        k_tc=0, n_rrc=0, ttis=_occ(320, 2, 3)),
    # 15 PRB: T_srs 40 and 80, M_sc 24 at B 1 without hopping (n_rrc picks the position)
    "p15_bw5_T40": dict(nof_prb=15, cell_id=33, cp_ext=False, bw_cfg=5, subframe_config=1, gh=True, sh=False, delta_ss=29, B=1, b_hop=1, n_srs=7, I_srs=50,
                        k_tc=1, n_rrc=2, ttis=_occ(50, 3, 1)),
    "p15_bw5_T80": dict(nof_prb=15, cell_id=33, cp_ext=True, bw_cfg=5, subframe_config=1, gh=False, sh=False, delta_ss=0, B=1, b_hop=0, n_srs=4, I_srs=100,
                        k_tc=0, n_rrc=23, ttis=_occ(100, 4, 2)),
}


def _row_n_rrc(band, bw_cfg, B):
    """The n_rrc of a row case: the one whose position indices n_b = floor(4 n_rrc / m_SRS,b) mod N_b (36.211 5.5.3.2, no hopping) add up highest
    over b <= B, so that every level with N_b > 1 moves k0; the largest of equals."""
    from srs_ref import M_SRS_B
    m = [M_SRS_B[band][b][bw_cfg] for b in range(4)]
    return max(range(24), key=lambda n: (sum((4 * n // m[b]) % (m[b - 1] // m[b]) for b in range(1, B + 1)), n))


# One case per row of the four bandwidth tables (the first eight cases reach six of the 32): the smallest cell of the band that holds m_SRS,0,
# every B (the wide B 0 and 1 on one bw_cfg each, to keep the fixture small), both combs, every cyclic shift, both CPs, T_srs 2 and 5, two
# occasions each.
ROW_B = (3, 2, 3, 3, 1, 2, 3, 0)
ROW_PRB = ((40, 40, 25, 25, 25, 15, 15, 6), (50,) * 8, (75,) * 8, (100,) * 8)
for _band in range(4):
    for _bw in range(8):
        _i, _B = 8 * _band + _bw, ROW_B[_bw]
        CASES["row_b%d_c%d" % (_band, _bw)] = dict(
            nof_prb=ROW_PRB[_band][_bw], cell_id=17 * _i % 504, cp_ext=(_band + _bw) % 3 == 0, bw_cfg=_bw, subframe_config=_i % 15, gh=_bw % 4 == 1,
            sh=_bw % 4 == 2, delta_ss=(7 * _bw + _band) % 30, B=_B, b_hop=3, n_srs=(3 * _bw + _band) % 8, I_srs=_bw % 7, k_tc=_bw % 2,
            n_rrc=_row_n_rrc(_band, _bw, _B), ttis=_occ(_bw % 7, 2, 3 + _band))

# Hopping over a whole period (the product of the N_b above b_hop, in occasions) and one occasion more, positions only. Not in CASES: they carry
# no values, so only the host walks them.
HOP_CASES = {
    # N_1 N_2 N_3 = 2 2 5 (an odd N_b last): 20 positions; T_srs 2
    "hop_p100_bw2": dict(nof_prb=100, cell_id=421, cp_ext=False, bw_cfg=2, subframe_config=0, gh=False, sh=False, delta_ss=0, B=3, b_hop=0, n_srs=1, I_srs=1,
                         k_tc=1, n_rrc=7, period=20, ttis=_occ(1, 21, 37)),
    # b_hop 1 < B 3: level 1 stays where n_rrc puts it, N_2 N_3 = 2 4 (even N_b only): 8 positions; T_srs 5, extended CP
    "hop_p75_bw1": dict(nof_prb=75, cell_id=88, cp_ext=True, bw_cfg=1, subframe_config=3, gh=False, sh=False, delta_ss=0, B=3, b_hop=1, n_srs=6, I_srs=4,
                        k_tc=0, n_rrc=13, period=8, ttis=_occ(4, 9, 5)),
}
# every B and n_rrc of every row, without hopping, on the smallest usual cell of each band that holds every m_SRS,0 of it
SWEEP_PRBS = [40, 50, 75, 100]
# every offset of the longest period's first subframes (tti < T_offset for most I_srs), a stretch further on, and the end of the TTI range
SEND_UE_TTIS = list(range(0, 24)) + [39, 40, 79, 80, 159, 160, 161, 319, 320, 321, 477, 636, 637, 5000, 5003, 10239]
BW_PRBS = [6, 15, 25, 40, 41, 50, 60, 61, 75, 80, 81, 100, 110]


def shortened_inputs():
    """(pusch [n][8]: nof_prb, subframe_config, bw_cfg, configured, I_srs, tti, n_prb_tilde 0 / 1 ... L_prb in column 8; pucch [m][6]:
    subframe_config, configured, simul_ack, format, tti, 0) - drawn once from a fixed seed, edges of the sounding band included."""
    rng = np.random.default_rng(20260)
    pusch = []
    for nof_prb, bw_cfg in ((6, 7), (25, 2), (25, 7), (50, 0), (50, 5), (75, 3), (100, 0), (100, 7)):
        for _ in range(40):
            sc, I = int(rng.integers(0, 15)), int(rng.choice([0, 1, 3, 8, 20]))
            tti = int(rng.integers(0, 10240))
            L = int(rng.integers(1, nof_prb + 1))
            n0 = int(rng.integers(0, nof_prb - L + 1))
            n1 = n0 if rng.random() < 0.6 else int(rng.integers(0, nof_prb - L + 1))
            pusch.append((nof_prb, sc, bw_cfg, int(rng.random() < 0.8), I, tti, n0, n1, L))
        from srs_ref import M_SRS_B, bw_table_idx  # the band's edges, on an occasion of the cell and of the UE (I_srs 0, subframe_config 0)
        m0 = M_SRS_B[bw_table_idx(nof_prb)][0][bw_cfg]
        s = nof_prb // 2 - m0 // 2
        for n0, L in ((s + m0, 1), (max(s - 1, 0), 1), (0, s), (0, max(s - 1, 1)), (s, m0), (0, nof_prb), (s + m0 - 1, 1), (0, s + 1)):
            if L >= 1 and n0 + L <= nof_prb:
                for tti in (100, 101):
                    pusch.append((nof_prb, 0, bw_cfg, 1, 0, tti, n0, n0, L))
                    pusch.append((nof_prb, 0, bw_cfg, 1, 1, tti, n0, n0, L))
    pucch = [(sc, conf, sim, fmt, tti, 0) for sc in (0, 3, 7, 13) for conf in (0, 1) for sim in (0, 1) for fmt in range(6) for tti in (7, 10, 123)]
    return np.array(pusch, np.uint32), np.array(pucch, np.uint32)


SHIM = r"""
/* Plain-argument entries to the SRS functions of refsignal_ul.c, and stubs for the PUCCH functions it names but the SRS never reaches. */
#include <stdlib.h>
#include <string.h>
#include "srslte/phy/ch_estimation/refsignal_ul.h"
int srslte_pucch_n_cs_cell(srslte_cell_t cell, uint32_t n_cs_cell[SRSLTE_NSLOTS_X_FRAME][SRSLTE_CP_NORM_NSYMB]) { (void)cell; (void)n_cs_cell; return 0; }
float srslte_pucch_alpha_format1(uint32_t a[SRSLTE_NSLOTS_X_FRAME][SRSLTE_CP_NORM_NSYMB], srslte_pucch_cfg_t* c, srslte_cp_t cp, bool s, uint32_t ns, uint32_t l, uint32_t* o, uint32_t* n) { abort(); }
float srslte_pucch_alpha_format2(uint32_t a[SRSLTE_NSLOTS_X_FRAME][SRSLTE_CP_NORM_NSYMB], srslte_pucch_cfg_t* c, uint32_t ns, uint32_t l) { abort(); }
uint32_t srslte_pucch_n_prb(srslte_cell_t* cell, srslte_pucch_cfg_t* cfg, uint32_t ns) { abort(); }
int srslte_pucch_format2ab_mod_bits(srslte_pucch_format_t format, uint8_t bits[2], cf_t* d_10) { abort(); }
void* rec_new(uint32_t nof_prb, uint32_t cell_id, int cp_ext)
{
  srslte_refsignal_ul_t* q = calloc(1, sizeof(*q));
  srslte_cell_t cell;
  memset(&cell, 0, sizeof(cell));
  cell.nof_prb = nof_prb, cell.nof_ports = 1, cell.id = cell_id, cell.cp = cp_ext ? SRSLTE_CP_EXT : SRSLTE_CP_NORM;
  if (srslte_refsignal_ul_init(q, 110) || srslte_refsignal_ul_set_cell(q, cell)) return NULL;
  return q;
}
void rec_free(void* q) { srslte_refsignal_ul_free(q); free(q); }
static srslte_refsignal_srs_cfg_t mk(const uint32_t* c)
{ /* subframe_config, bw_cfg, B, b_hop, n_srs, I_srs, k_tc, n_rrc, configured, simul_ack */
  srslte_refsignal_srs_cfg_t s;
  memset(&s, 0, sizeof(s));
  s.subframe_config = c[0], s.bw_cfg = c[1], s.B = c[2], s.b_hop = c[3], s.n_srs = c[4], s.I_srs = c[5], s.k_tc = c[6], s.n_rrc = c[7];
  s.configured = c[8] != 0, s.simul_ack = c[9] != 0, s.dedicated_enabled = s.common_enabled = true;
  return s;
}
uint32_t rec_M_sc(void* q, const uint32_t* c) { srslte_refsignal_srs_cfg_t s = mk(c); return srslte_refsignal_srs_M_sc(q, &s); }
int rec_gen(void* q, const uint32_t* c, uint32_t delta_ss, int gh, int sh, uint32_t sf_idx, cf_t* r)
{
  srslte_refsignal_srs_cfg_t s = mk(c);
  srslte_refsignal_dmrs_pusch_cfg_t d;
  memset(&d, 0, sizeof(d));
  d.delta_ss = delta_ss, d.group_hopping_en = gh != 0, d.sequence_hopping_en = sh != 0;
  return srslte_refsignal_srs_gen(q, &s, &d, sf_idx, r);
}
int rec_put(void* q, const uint32_t* c, uint32_t tti, cf_t* r, cf_t* grid) { srslte_refsignal_srs_cfg_t s = mk(c); return srslte_refsignal_srs_put(q, &s, tti, r, grid); }
int rec_pusch_shortened(void* q, const uint32_t* c, uint32_t tti, uint32_t n0, uint32_t n1, uint32_t L)
{
  srslte_refsignal_srs_cfg_t s = mk(c);
  srslte_ul_sf_cfg_t sf;
  srslte_pusch_cfg_t p;
  memset(&sf, 0, sizeof(sf));
  memset(&p, 0, sizeof(p));
  sf.tti = tti, p.grant.n_prb_tilde[0] = n0, p.grant.n_prb_tilde[1] = n1, p.grant.L_prb = L;
  srslte_refsignal_srs_pusch_shortened(q, &sf, &s, &p);
  return sf.shortened ? 1 : 0;
}
int rec_pucch_shortened(void* q, const uint32_t* c, uint32_t format, uint32_t tti)
{
  srslte_refsignal_srs_cfg_t s = mk(c);
  srslte_ul_sf_cfg_t sf;
  srslte_pucch_cfg_t p;
  memset(&sf, 0, sizeof(sf));
  memset(&p, 0, sizeof(p));
  sf.tti = tti, p.format = (srslte_pucch_format_t)format;
  srslte_refsignal_srs_pucch_shortened(q, &sf, &s, &p);
  return sf.shortened ? 1 : 0;
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
    srcs = [os.path.join(lib, "src/phy/ch_estimation/refsignal_ul.c"), os.path.join(lib, "src/phy/common/phy_common.c"),
            os.path.join(lib, "src/phy/utils/debug.c"), shim]
    out = os.path.join(tmp, "librec.so")
    # the reference's release flags (oracle/ref.mk): -Ofast -mfma decides how tmp_arg[i] + alpha * i rounds
    cmd = ["gcc", "-std=gnu99", "-D_GNU_SOURCE", "-O3", "-Ofast", "-funroll-loops", "-mfpmath=sse", "-mavx2", "-mfma", "-DLV_HAVE_SSE", "-DLV_HAVE_AVX",
           "-DLV_HAVE_AVX2", "-DLV_HAVE_FMA", "-fPIC", "-w", "-I" + os.path.join(lib, "include"), "-shared", "-Wl,-z,defs", "-o", out] + srcs
    cmd += ["-L" + ref_so_dir, "-lsrslte_ref", "-Wl,-rpath," + ref_so_dir, "-lm", "-lpthread"]
    subprocess.check_call(cmd)
    return out


def cfg_words(c, configured=1, simul_ack=0):
    return np.array([c["subframe_config"], c["bw_cfg"], c["B"], c["b_hop"], c["n_srs"], c["I_srs"], c["k_tc"], c["n_rrc"], configured, simul_ack], np.uint32)


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
        L.rec_M_sc.restype = u32
        L.rec_M_sc.argtypes = [vp, vp]
        L.rec_gen.argtypes = [vp, vp, u32, C.c_int, C.c_int, u32, vp]
        L.rec_put.argtypes = [vp, vp, u32, vp, vp]
        L.rec_pusch_shortened.argtypes = [vp, vp, u32, u32, u32, u32]
        L.rec_pucch_shortened.argtypes = [vp, vp, u32, u32]
        for fn in (L.srslte_refsignal_srs_rb_start_cs, L.srslte_refsignal_srs_rb_L_cs):
            fn.restype, fn.argtypes = u32, [u32, u32]
        for name, c in sorted(CASES.items()):
            q = L.rec_new(c["nof_prb"], c["cell_id"], 1 if c["cp_ext"] else 0)
            assert q, name
            w = cfg_words(c)
            M = L.rec_M_sc(q, w.ctypes.data)
            nsym = 12 if c["cp_ext"] else 14
            gens, idxs, vals = [], [], []
            for tti in c["ttis"]:
                r = np.zeros(2 * M, np.complex64)
                assert L.rec_gen(q, w.ctypes.data, c["delta_ss"], int(c["gh"]), int(c["sh"]), tti % 10, r.ctypes.data) == 0
                grid = np.zeros(nsym * 12 * c["nof_prb"], np.complex64)
                assert L.rec_put(q, w.ctypes.data, tti, r.ctypes.data, grid.ctypes.data) == 0
                nz = np.flatnonzero(grid)
                assert nz.size == M  # unit-modulus values: none is zero
                gens.append(r.reshape(2, M))
                idxs.append(nz.astype(np.uint32))
                vals.append(grid[nz])
            res[name + ".M_sc"] = np.array(M, np.uint32)
            res[name + ".gen"] = np.stack(gens)
            res[name + ".put_idx"] = np.stack(idxs)
            res[name + ".put_val"] = np.stack(vals)
            L.rec_free(q)
        for name, c in sorted(HOP_CASES.items()):
            q = L.rec_new(c["nof_prb"], c["cell_id"], 1 if c["cp_ext"] else 0)
            assert q, name
            w = cfg_words(c)
            M = L.rec_M_sc(q, w.ctypes.data)
            r, first = np.ones(2 * M, np.complex64), []
            for tti in c["ttis"]:
                grid = np.zeros((12 if c["cp_ext"] else 14) * 12 * c["nof_prb"], np.complex64)
                assert L.rec_put(q, w.ctypes.data, tti, r.ctypes.data, grid.ctypes.data) == 0
                first.append(np.flatnonzero(grid)[0])
            res[name + ".put_idx0"] = np.array(first, np.uint32)
            L.rec_free(q)
        sw_M, sw_k0 = np.zeros((len(SWEEP_PRBS), 8, 4), np.uint32), np.zeros((len(SWEEP_PRBS), 8, 4, 24), np.uint32)
        for pi, P in enumerate(SWEEP_PRBS):
            q = L.rec_new(P, 1, 0)
            assert q, P
            r = np.ones(2 * 12 * P, np.complex64)
            for bw in range(8):
                for B in range(4):
                    for n_rrc in range(24):
                        w = np.array([0, bw, B, 3, 0, 0, 0, n_rrc, 1, 0], np.uint32)
                        sw_M[pi, bw, B] = L.rec_M_sc(q, w.ctypes.data)
                        grid = np.zeros(14 * 12 * P, np.complex64)
                        assert L.rec_put(q, w.ctypes.data, 0, r.ctypes.data, grid.ctypes.data) == 0
                        sw_k0[pi, bw, B, n_rrc] = np.flatnonzero(grid)[0] - 13 * 12 * P
            L.rec_free(q)
        res["sweep_M_sc"], res["sweep_k0"] = sw_M, sw_k0
        res["send_cs"] = np.array([[L.srslte_refsignal_srs_send_cs(sc, sf) for sf in range(10)] for sc in range(15)], np.int8)
        res["send_ue"] = np.array([[L.srslte_refsignal_srs_send_ue(I, t) for t in SEND_UE_TTIS] for I in range(637)], np.int8)
        res["rb_start_cs"] = np.array([[L.srslte_refsignal_srs_rb_start_cs(b, p) for b in range(8)] for p in BW_PRBS], np.uint32)
        res["rb_L_cs"] = np.array([[L.srslte_refsignal_srs_rb_L_cs(b, p) for b in range(8)] for p in BW_PRBS], np.uint32)
        pusch, pucch = shortened_inputs()
        out, qs = [], {}
        for (P, sc, bw, conf, I, tti, n0, n1, Lp) in pusch.tolist():
            if P not in qs:
                qs[P] = L.rec_new(P, 1, 0)
            w = np.array([sc, bw, 0, 0, 0, I, 0, 0, conf, 0], np.uint32)
            out.append(L.rec_pusch_shortened(qs[P], w.ctypes.data, tti, n0, n1, Lp))
        res["pusch_shortened"] = np.array(out, np.int8)
        out = []
        for (sc, conf, sim, fmt, tti, _) in pucch.tolist():
            w = np.array([sc, 0, 0, 0, 0, 0, 0, 0, conf, sim], np.uint32)
            out.append(L.rec_pucch_shortened(qs[6], w.ctypes.data, fmt, tti))
        res["pucch_shortened"] = np.array(out, np.int8)
        for q in qs.values():
            L.rec_free(q)
    return res


if __name__ == "__main__":
    sys.path.insert(0, HERE)
    res = record(sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
    np.savez_compressed(GOLDEN, **res)
    print("wrote %s: %d arrays, %d bytes" % (GOLDEN, len(res), os.path.getsize(GOLDEN)))
