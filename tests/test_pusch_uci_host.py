"""The PUSCH UCI plan (srslte_hip_pusch_uci_plan, pusch_uci_host.cpp; no device): Q'_ack, Q'_ri, Q'_cqi and the UL-SCH symbols G' of a sweep of
configurations against the oracle's Q' functions (tied to the reference by test_oracle_vs_ref.py), every reason the plan gives, and the ACK / RI
symbol positions against the column sets of 36.212 Table 5.2.2.8-1 / -2."""
import ctypes as C
import importlib
import itertools
import math
import random
from types import SimpleNamespace

import numpy as np

from _libs import oracle
from lte_sim import OrcCbsegm, ul_ack_ri_qprime

pkg = importlib.import_module("srslte-emane_amd")
OK, EMPTY, BETA, ROWS, NO_ROOM = pkg.PUSCH_UCI_OK, pkg.PUSCH_UCI_EMPTY, pkg.PUSCH_UCI_BETA, pkg.PUSCH_UCI_ROWS, pkg.PUSCH_UCI_NO_ROOM

# 36.213 Tables 8.6.3-1..3, None = reserved
BETA_ACK = [2.0, 2.5, 3.125, 4.0, 5.0, 6.25, 8.0, 10.0, 12.625, 15.875, 20.0, 31.0, 50.0, 80.0, 126.0, None]
BETA_RI = [1.25, 1.625, 2.0, 2.5, 3.125, 4.0, 5.0, 6.25, 8.0, 10.0, 12.625, 15.875, 20.0, None, None, None]
BETA_CQI = [None, None, 1.125, 1.25, 1.375, 1.625, 1.75, 2.0, 2.25, 2.5, 2.875, 3.125, 3.5, 4.0, 5.0, 6.25]

GRID = dict(L_prb=(1, 6, 25, 100, 110), nof_symb=(9, 10, 11, 12), mod=(1, 2, 3), tbs=(0, 1000, 75376), ack_len=(0, 1, 2, 3, 10), ri_len=(0, 1, 2),
            cqi_len=(0, 4, 11, 12, 64), I_offset_ack=(0, 2, 7, 14, 15), I_offset_ri=(0, 2, 7, 12, 13), I_offset_cqi=(0, 2, 7, 15, 1))
# the rows of the matrix are an input of their own (the decode call does not tie nof_bits to 12 L_prb): half and twice the allocation, too
ROWS_PER_PRB = (12, 12, 12, 6, 24)
# test_gpu_ulsch_encode.py's "25prb_16qam_c3": three code blocks behind a report whose Q'_cqi Qm bits end inside a byte
C3 = dict(L_prb=25, nof_symb=12, mod=2, tbs=15264, ack_len=0, ri_len=0, cqi_len=4 + 2 * 7, I_offset_ack=9, I_offset_ri=6, I_offset_cqi=2, rows=300)


def segm(tbs, _cache={}):
    if tbs not in _cache:
        _cache[tbs] = OrcCbsegm()
        if tbs:
            assert oracle().orc_cbsegm(C.byref(_cache[tbs]), tbs) == 0
    return _cache[tbs]


def cases():
    """every (L_prb, nof_symb, tbs, ack_len, ri_len, cqi_len) of the grid, each with 24 seeded draws of the modulation, the three offset
    indices and the rows; the whole product is five million plans"""
    rng = random.Random(36212)
    outer = ("L_prb", "nof_symb", "tbs", "ack_len", "ri_len", "cqi_len")
    inner = ("mod", "I_offset_ack", "I_offset_ri", "I_offset_cqi")
    for vals in itertools.product(*(GRID[k] for k in outer)):
        for _ in range(24):
            c = dict(zip(outer, vals), **{k: rng.choice(GRID[k]) for k in inner})
            c["rows"] = rng.choice(ROWS_PER_PRB) * c["L_prb"]
            yield c
    yield dict(C3)


def closed_qprime(O, beta, beta_cqi, L_prb, nsymb, K):
    """Q_prime_ri_ack (uci.c:547-571) written out in float32, operand by operand; beta_cqi divides the offset on a PUSCH without data"""
    f = np.float32
    b = f(beta) if beta_cqi is None else f(beta) / f(beta_cqi)
    x = f(O) * f(L_prb) * f(12) * f(nsymb) * b / f(K)
    return min(int(math.ceil(float(x))), 4 * 12 * L_prb)


def expected(c):
    """(reason, Q'_ack, Q'_ri, Q'_cqi, G') from the oracle; None where the plan stops before it gets there"""
    seg = segm(c["tbs"])
    sim = SimpleNamespace(tbs=c["tbs"], L_prb=c["L_prb"], nsymb=c["nof_symb"], seg=seg)
    data = c["tbs"] > 0
    if not data and c["cqi_len"] == 0:
        return EMPTY, None, None, None, None
    in_use = [(c["ack_len"] > 0, BETA_ACK, c["I_offset_ack"]), (c["ri_len"] > 0, BETA_RI, c["I_offset_ri"]),
              (c["cqi_len"] > 0 or not data, BETA_CQI, c["I_offset_cqi"])]
    Qp = [ul_ack_ri_qprime(sim, c[k + "_len"], c["I_offset_" + k], k == "ri", c["cqi_len"], c["I_offset_cqi"]) for k in ("ack", "ri")]
    reserved = [used and tab[i] is None for used, tab, i in in_use]
    if any(reserved):
        assert all(Qp[n] < 0 for n in (0, 1) if reserved[n])  # the oracle refuses a reserved ACK / RI offset itself
        return BETA, None, None, None, None
    if c["ack_len"] > 2:  # beyond what the batched pipelines take: the closed formula beside the oracle
        K = seg.C * seg.K1 if data else (c["cqi_len"] if c["cqi_len"] <= 11 else c["cqi_len"] + 8)
        assert Qp[0] == closed_qprime(c["ack_len"], BETA_ACK[c["I_offset_ack"]], None if data else BETA_CQI[c["I_offset_cqi"]], c["L_prb"], c["nof_symb"], K)
    if max(Qp) > 4 * c["rows"]:
        return ROWS, Qp[0], Qp[1], None, None
    Qc = oracle().orc_uci_cqi_qprime(c["cqi_len"], c["I_offset_cqi"], c["L_prb"], c["nof_symb"], seg.C * seg.K1, Qp[1]) if c["cqi_len"] else 0
    assert Qc >= 0
    H = c["rows"] * c["nof_symb"]
    if Qp[1] + Qc > H or (data and Qp[1] + Qc == H):
        return NO_ROOM, Qp[0], Qp[1], Qc, None
    return OK, Qp[0], Qp[1], Qc, H - Qp[1] - Qc


def plan(c, **kw):
    seg = segm(c["tbs"])
    f = {k: v for k, v in c.items() if k not in ("mod", "tbs")}
    return pkg.pusch_uci_plan(Qm=2 * c["mod"], K_segm=seg.C * seg.K1, C=seg.C, **f, **kw)


def test_plan_matches_the_oracle_over_the_grid():
    assert segm(1000).C == 1 and segm(75376).C >= 13 and segm(15264).C == 3
    reasons, kinds, seen = set(), set(), {k: set() for k in GRID}
    for c in cases():
        why, res = plan(c)
        want = expected(c)
        assert why == want[0], (c, why, want)
        got = (res.Qp_ack, res.Qp_ri, res.Qp_cqi, res.G_prime)
        assert all(w is None or w == g for w, g in zip(want[1:], got)), (c, got, want)
        reasons.add(why)
        for k in GRID:
            seen[k].add(c[k])
        if why != OK:
            continue
        seg = segm(c["tbs"])
        assert res.Q_cqi == res.Qp_cqi * 2 * c["mod"]
        if c["tbs"]:  # sch.c:205-207: the first C - gamma blocks carry floor(G' / C) symbols, gamma = G' mod C
            assert (res.syms_lo, res.C_lo) == (res.G_prime // seg.C, seg.C - res.G_prime % seg.C) and res.G_prime > 0
            kinds.add("data with all three" if c["ack_len"] and c["ri_len"] and c["cqi_len"] else "data")
        else:
            assert (res.syms_lo, res.C_lo) == (0, 0)
            kinds.add("report, ACK and RI alone" if c["ack_len"] and c["ri_len"] else ("report alone" if not c["ack_len"] and not c["ri_len"] else "report"))
            if c["rows"] == 12 * c["L_prb"]:
                assert res.G_prime == 0  # the report of a PUSCH without data fills what the RI leaves
    assert reasons == {OK, EMPTY, BETA, ROWS, NO_ROOM}, reasons
    assert {"data with all three", "report alone", "report, ACK and RI alone"} <= kinds, kinds
    assert all(seen[k] >= set(GRID[k]) for k in GRID), seen
    why, res = plan(C3)
    assert why == OK and res.Qp_cqi == 7 and res.Q_cqi % 8 != 0 and res.G_prime % 3 != 0 and res.syms_lo * res.C_lo + (res.syms_lo + 1) * (3 - res.C_lo) == res.G_prime


def test_plan_refuses_what_is_no_configuration():
    L = pkg.lib()
    assert L.srslte_hip_pusch_uci_plan(None, None) == -2
    for bad in (dict(L_prb=0), dict(nof_symb=0), dict(rows=0)):
        assert plan(dict(C3, **bad))[0] == -2
    f = {k: v for k, v in C3.items() if k not in ("mod", "tbs")}
    assert pkg.pusch_uci_plan(Qm=4, K_segm=0, C=3, **f)[0] == -2 and pkg.pusch_uci_plan(Qm=4, K_segm=6144, C=0, **f)[0] == -2
    # an offset index above 15 of a field in use is no index of the table; of a field not in use it is not looked at
    assert plan(dict(C3, I_offset_cqi=16))[0] == BETA and plan(dict(C3, I_offset_ack=16, I_offset_ri=99))[0] == OK
    assert plan(dict(C3, ack_len=1, I_offset_ack=16))[0] == BETA and plan(dict(C3, ri_len=1, I_offset_ri=16))[0] == BETA


def test_symbol_positions_follow_the_column_sets_of_36212():
    """36.212 5.2.2.8: symbol i sits in row R'_mux - 1 - floor(i / 4) of ColumnSet(j), j starting at 0 and advancing by 3 mod 4; the sets of Tables
    5.2.2.8-1 and -2 for the normal and the extended CP, chosen by the number of columns as upstream does (uci.c:497-545)"""
    ACK = {True: (2, 3, 8, 9), False: (1, 2, 6, 7)}
    RI = {True: (1, 4, 7, 10), False: (0, 3, 5, 8)}
    for nof_symb, rows in itertools.product((9, 10, 11, 12), (12, 30, 72)):
        j = 0
        for i in range(4 * rows):
            _, res = plan(dict(C3, nof_symb=nof_symb, rows=rows), sym=i)
            row = rows - 1 - i // 4
            assert tuple(res.ack_pos) == (row, ACK[nof_symb > 10][j]) and tuple(res.ri_pos) == (row, RI[nof_symb > 10][j]), (nof_symb, rows, i)
            j = (j + 3) % 4
