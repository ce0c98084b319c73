"""Host helpers of the PUCCH path (srslte_hip_pucch_n_cs_cell, srslte_hip_pucch_resource, srslte_hip_pucch_dmrs) against the reference over
drawn cells: n_cs_cell as srslte_refsignal_ul_set_cell leaves it, the DMRS of every format / CP / n_pucch / slot (also through the reference's
own srslte_chest_ul_estimate_pucch, which must see a unit channel on it), the resource selection with its SR and collision rules, and the
layouts of the ctypes mirrors tests/ul_ctrl_ref.py drives the reference with. No GPU."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

from _libs import REF_INC, RefChestUlRes, aligned, ref, struct_layout
from ul_ctrl_ref import PUCCH_CFG, REFSIGNAL_UL, UL_SF_CFG, RefUlCtrl, select

pkg = importlib.import_module("srslte-emane_amd")
needs_ref = pytest.mark.skipif(ref() is None, reason="oracle/_ref/libsrslte_ref.so is not built")

# (nof_prb, cell_id, cp_ext, group hopping, delta_pucch_shift, N_cs, n_rb_2, N_pucch_1)
CELLS = [(6, 1, False, False, 1, 0, 1, 0), (15, 77, False, True, 2, 6, 2, 4), (25, 200, True, True, 2, 4, 2, 10), (50, 150, False, False, 3, 6, 3, 0),
         (75, 301, True, False, 1, 7, 0, 20), (100, 5, False, True, 3, 3, 4, 36), (100, 411, True, True, 1, 0, 6, 12), (6, 503, False, False, 2, 2, 1, 3)]  # srslte_cell_isvalid stops at 100 PRB


def _cfg(spec):
    P, cid, ext, gh, D, Ncs, nrb2, N1 = spec
    return pkg.ul_ctrl_cfg(P, cid, cp_ext=ext, group_hopping_en=gh, delta_pucch_shift=D, N_cs=Ncs, n_rb_2=nrb2, N_pucch_1=N1)


@pytest.mark.skipif(not os.path.isdir(REF_INC), reason="the reference headers are not on this machine")
def test_mirror_layouts():
    lay = struct_layout({"srslte_pucch_cfg_t": ["rnti", "uci_cfg", "delta_pucch_shift", "n_rb_2", "N_cs", "N_pucch_1", "group_hopping_en", "n_pucch_2",
                                                "n_pucch_sr", "simul_cqi_ack", "threshold_format1", "threshold_data_valid_format1a",
                                                "threshold_data_valid_format2", "format", "n_pucch", "pucch2_drs_bits"],
                         "srslte_uci_cfg_t": ["ack", "cqi", "is_scheduling_request_tti"], "srslte_uci_cfg_ack_t": ["nof_acks", "ncce"],
                         "srslte_cqi_cfg_t": ["data_enable", "ri_len"], "srslte_refsignal_ul_t": ["n_cs_cell", "f_gh"],
                         "srslte_ul_sf_cfg_t": ["tti", "shortened"]},
                        ["srslte/config.h", "srslte/phy/common/phy_common.h", "srslte/phy/phch/pucch_cfg.h", "srslte/phy/ch_estimation/refsignal_ul.h"], [REF_INC])
    p = "srslte_pucch_cfg_t"
    assert lay[p] == PUCCH_CFG["size"]
    for k in ("rnti", "delta_pucch_shift", "n_rb_2", "N_cs", "N_pucch_1", "group_hopping_en", "n_pucch_2", "n_pucch_sr", "simul_cqi_ack", "threshold_format1",
              "threshold_data_valid_format1a", "threshold_data_valid_format2", "format", "n_pucch", "pucch2_drs_bits"):
        assert lay[p + "." + k] == PUCCH_CFG[k], k
    u = lay[p + ".uci_cfg"]
    assert u + lay["srslte_uci_cfg_t.ack"] + lay["srslte_uci_cfg_ack_t.nof_acks"] == PUCCH_CFG["ack.nof_acks"]
    assert u + lay["srslte_uci_cfg_t.ack"] + lay["srslte_uci_cfg_ack_t.ncce"] == PUCCH_CFG["ack.ncce"]
    assert u + lay["srslte_uci_cfg_t.cqi"] + lay["srslte_cqi_cfg_t.data_enable"] == PUCCH_CFG["cqi.data_enable"]
    assert u + lay["srslte_uci_cfg_t.cqi"] + lay["srslte_cqi_cfg_t.ri_len"] == PUCCH_CFG["cqi.ri_len"]
    assert u + lay["srslte_uci_cfg_t.is_scheduling_request_tti"] == PUCCH_CFG["is_scheduling_request_tti"]
    assert lay["srslte_refsignal_ul_t"] == REFSIGNAL_UL["size"]
    assert lay["srslte_refsignal_ul_t.n_cs_cell"] == REFSIGNAL_UL["n_cs_cell"] and lay["srslte_refsignal_ul_t.f_gh"] == REFSIGNAL_UL["f_gh"]
    assert lay["srslte_ul_sf_cfg_t"] == UL_SF_CFG["size"] and lay["srslte_ul_sf_cfg_t.tti"] == UL_SF_CFG["tti"]
    assert lay["srslte_ul_sf_cfg_t.shortened"] == UL_SF_CFG["shortened"]


@needs_ref
@pytest.mark.parametrize("idx", range(len(CELLS)))
def test_n_cs_cell_and_dmrs(idx):
    cfg = _cfg(CELLS[idx])
    R = RefUlCtrl(cfg)
    assert np.array_equal(pkg.pucch_n_cs_cell(cfg)[:, :R.nsl], R.n_cs_cell[:, :R.nsl])
    rng = np.random.default_rng(idx)
    c = 2 if cfg.cp_ext else 3
    lim1 = c * cfg.N_cs // cfg.delta_pucch_shift
    for fmt in range(6):
        ns = sorted({0, 1, max(lim1 - 1, 0), lim1, lim1 + 1, 12 * cfg.n_rb_2, 12 * cfg.n_rb_2 + 5} | set(rng.integers(0, 60, 6).tolist()))
        for n in ns:
            if pkg.pucch_resource(cfg, pkg.PucchReq.make(0, 0x46, sr_tti=True, n_pucch_sr=n)) is None:
                continue
            for tti in rng.integers(0, 10240, 3):
                for drs in ((0, 0), (1, 0), (0, 1), (1, 1)):
                    got = pkg.pucch_dmrs(cfg, fmt, n, int(tti), drs).reshape(-1)
                    assert np.abs(got - R.dmrs(fmt, n, int(tti), drs)).max() < 1e-5, (fmt, n, tti, drs)
                # the reference's estimator on the restated DMRS (its own srslte_refsignal_dmrs_pucch_gen inside) sees a unit channel, and a
                # 2a / 2b grid made with bits (1, 0) gives those bits back
                if any(pucch_prb >= cfg.nof_prb for pucch_prb in _prbs(cfg, fmt, n)):
                    continue
                g = aligned(R.glen, np.complex64)
                R.dmrs_put(g, fmt, n, int(tti), False, (1, 0))
                cfgb, ce = R.pucch_cfg(fmt, n), aligned(R.glen, np.complex64)
                res = RefChestUlRes()
                res.ce = ce.ctypes.data
                assert R.R.srslte_chest_ul_estimate_pucch(R.chest, R.sf_cfg(int(tti), False), cfgb, g.ctypes.data, C.byref(res)) == 0
                assert np.abs(ce[R.dmrs_re(fmt, n)] - 1).max() < 1e-4, (fmt, n, tti)
                if fmt in (4, 5):
                    assert (cfgb[PUCCH_CFG["pucch2_drs_bits"]], cfgb[PUCCH_CFG["pucch2_drs_bits"] + 1]) == (1, 0)


def _prbs(cfg, fmt, n):
    from ul_ctrl_ref import pucch_n_prb
    return [pucch_n_prb(fmt, n, s, cfg.nof_prb, cfg.delta_pucch_shift, cfg.N_cs, cfg.n_rb_2, bool(cfg.cp_ext)) for s in range(2)]


@pytest.mark.parametrize("idx", range(len(CELLS)))
def test_resource_selection(idx):
    """srslte_ue_ul_pucch_resource_selection restated (ue_ul.c) against the library, receiver (zero UCI value) and transmitter (SR value)."""
    cfg = _cfg(CELLS[idx])
    rng = np.random.default_rng(100 + idx)
    seen = set()
    for _ in range(400):
        ack, cqi = int(rng.integers(0, 3)), int(rng.choice([0, 0, 1, 4, 11, 12]))
        ri = int(rng.integers(0, 2)) if cqi == 0 and rng.random() < 0.3 else 0
        q = pkg.PucchReq.make(0, 0x46, ack_len=ack, ncce=int(rng.integers(0, 40)), sr_tti=bool(rng.random() < 0.4), n_pucch_sr=int(rng.integers(0, 40)),
                              cqi_len=cqi, ri_len=ri, n_pucch_2=int(rng.integers(0, 40)), simul_cqi_ack=bool(rng.random() < 0.5))
        for sr_val in (None, 0, 1):
            uci = None if sr_val is None else pkg.PucchTx.make(q, sr=sr_val)
            got = pkg.pucch_resource(cfg, q, uci)
            want = select(bool(cfg.cp_ext), cfg.N_pucch_1, q, q.sr_tti, 0 if sr_val is None else sr_val)
            assert (got is None) == (want is None), (got, want)
            if want is not None:
                assert got[:2] == want and list(got[2:]) == _prbs(cfg, *want)
                seen.add(want[0])
    assert seen == ({0, 1, 2, 3, 5} if cfg.cp_ext else set(range(6)))
