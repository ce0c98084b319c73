"""The PUSCH receiver's hook of the link-time drop-in without a GPU: the library exports the device call with its geometry helper and debug accessor
(phy_hip.h), the reference's srslte_pusch_decode on top of it and its counter (srslte_compat_pusch.h); every struct that function takes lies
in the header as in the reference's headers - against the stored numbers of tests/golden/ref_abi_pusch.json (tests/gen_golden_pusch_abi.py) and,
where they are present, against the headers themselves; and the rows the call stages are those pusch_cp walks (pusch.c:53-91), for hopping,
shortened and extended-CP grants. pusch_cp is static in the reference, so the expectation is the oracle's: the symbols and offsets
lte_sim.oracle_ul_rx extracts, which tests/test_oracle_vs_ref.py pins to the reference."""
import ctypes as C
import json
import os

import pytest

from _libs import HIP_SO, REF_INC, ROOT, struct_layout
from lte_sim import UlConfig
from pusch_decode_abi import FIELDS, INCLUDES, PuschCfgHip, UlschCfg, UlschRes, pusch_cfg

INC = [os.path.join(ROOT, "include")]


def lib():
    return C.CDLL(HIP_SO)


def test_the_entry_points_are_exported():
    missing = [n for n in ("srslte_hip_pusch_decode", "srslte_hip_pusch_rows", "srslte_hip_pusch_debug_q", "srslte_pusch_decode", "srslte_hip_compat_stats_pusch")
               if not hasattr(lib(), n)]
    assert not missing, missing


def test_pusch_struct_layouts_match_the_reference():
    ours = struct_layout(FIELDS, ["srslte_hip/srslte_compat_pusch.h"], INC)
    with open(os.path.join(ROOT, "tests", "golden", "ref_abi_pusch.json")) as f:
        stored = json.load(f)["layouts"]
    assert set(stored) == set(ours) and len(ours) == len(FIELDS) + sum(len(v) for v in FIELDS.values())
    assert ours == stored
    if os.path.isdir(REF_INC):
        assert struct_layout(FIELDS, INCLUDES, [REF_INC]) == ours


def test_the_mirrors_of_the_device_call_match_the_header():
    names = {"srslte_hip_ulsch_cfg_t": UlschCfg, "srslte_hip_pusch_cfg_t": PuschCfgHip, "srslte_hip_ulsch_res_t": UlschRes}
    ly = struct_layout({n: [f[0] for f in t._fields_] for n, t in names.items()}, ["srslte_hip/phy_hip.h"], INC)
    for n, t in names.items():
        assert C.sizeof(t) == ly[n], n
        for f, *_ in t._fields_:
            assert getattr(t, f).offset == ly["%s.%s" % (n, f)], (n, f)


def rows_of(c):
    rows = (C.c_uint32 * 24)(*([0xdeadbeef] * 24))
    n = lib().srslte_hip_pusch_rows(C.byref(c), rows)
    return n, [(rows[2 * i], rows[2 * i + 1]) for i in range(max(n, 0))], list(rows)[2 * max(n, 0):]


# cell PRBs, L_prb, (n_prb_tilde slot 0, slot 1), extended CP, shortened
GEOMETRIES = {"plain": (6, 1, (2, 2), False, False), "hopping": (25, 15, (0, 10), False, False), "hopping_shortened": (25, 15, (10, 0), False, True),
              "ext_cp": (15, 9, (3, 3), True, False), "ext_cp_shortened_hopping": (15, 9, (6, 0), True, True), "last_prbs": (6, 2, (4, 4), False, False),
              "whole_cell": (100, 100, (0, 0), False, True)}


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_the_staged_rows_are_those_of_pusch_cp(name):
    P, L, n_prb, ext, short = GEOMETRIES[name]
    ul = UlConfig(P, 1, 1, 0, L, n_prb=n_prb[0], n_prb_slot1=n_prb[1], shortened=short, cp_ext=ext)
    n, rows, rest = rows_of(pusch_cfg(P, 1, 1, 0, L, n_prb, cp_ext=ext, shortened=short))
    assert n == ul.nsymb == len(ul.data_syms) == 2 * ul.nsl - 2 - int(short)
    assert rows == [(l, 12 * ul.n_prbs[l // ul.nsl]) for l in ul.data_syms]  # the rows oracle_ul_rx selects, in pusch_cp's order
    assert all(r == 0xdeadbeef for r in rest), "written behind the last row"
    assert all(sc + 12 * L <= 12 * P and l < 2 * ul.nsl for l, sc in rows)
    assert lib().srslte_hip_pusch_rows(C.byref(pusch_cfg(P, 1, 1, 0, L, n_prb, cp_ext=ext, shortened=short)), None) == n  # the check alone


def test_allocations_that_do_not_fit_are_refused():
    good = lambda: pusch_cfg(25, 1, 2, 0, 15, (0, 10))  # noqa: E731
    assert rows_of(good())[0] == 12
    bad = {}
    for what, change in {"L_prb 7 has no transform": lambda c: setattr(c.sch, "L_prb", 7), "L_prb 0": lambda c: setattr(c.sch, "L_prb", 0),
                         "slot 0 beyond the cell": lambda c: c.n_prb_tilde.__setitem__(0, 11), "slot 1 beyond the cell": lambda c: c.n_prb_tilde.__setitem__(1, 11),
                         "nof_re": lambda c: setattr(c, "nof_re", c.nof_re - 12), "nof_symb of a shortened subframe": lambda c: setattr(c.sch, "nof_symb", 11),
                         "shortened with 12 symbols": lambda c: setattr(c, "shortened", 1), "extended CP with 12 symbols": lambda c: setattr(c, "cp_ext", 1),
                         "nof_bits": lambda c: setattr(c.sch, "nof_bits", c.sch.nof_bits - 4), "BPSK": lambda c: setattr(c.sch, "mod", 0),
                         "256QAM": lambda c: setattr(c.sch, "mod", 4), "sf_idx": lambda c: setattr(c, "sf_idx", 10), "no cell": lambda c: setattr(c, "nof_prb", 0)}.items():
        c = good()
        change(c)
        n, _, rest = rows_of(c)
        bad[what] = n
        assert all(r == 0xdeadbeef for r in rest), what
    assert all(n == -2 for n in bad.values()), bad
    assert lib().srslte_hip_pusch_rows(None, None) == -2


def test_null_arguments_are_refused_without_a_device():
    L = lib()
    c, res = pusch_cfg(6, 1, 1, 40, 1, (0, 0)), UlschRes()
    L.srslte_hip_pusch_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float] + [C.c_void_p] * 6
    assert L.srslte_hip_pusch_decode(None, None, None, 0.0, C.byref(c), None, None, None, None, C.byref(res)) == -2
    assert L.srslte_hip_pusch_debug_q(None, None, 0) == -2
    L.srslte_pusch_decode.argtypes = [C.c_void_p] * 6
    assert L.srslte_pusch_decode(None, None, None, None, None, None) == -2
    out = (C.c_ulonglong * 2)(7, 7)
    L.srslte_hip_compat_stats_pusch(out)
    assert list(out) == [0, 0]
