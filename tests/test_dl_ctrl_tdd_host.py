"""Host side of the TDD control region: the helpers that need no device (mi, the REG lists of a subframe, the PHICH groups, the DCI sizes)
against the reference's own srslte_regs_init_opts / srslte_dci_format_sizeof in oracle/_ref/libsrslte_ref.so, the shared-REG refusal, the
creators' refusals that touch no device, and the share of near-tie PHICH requests among the draws the GPU test uses. No GPU needed."""
import ctypes as C
import importlib

import numpy as np
import pytest

from _libs import RefCell, ref

pkg = importlib.import_module("srslte-emane_amd")

needs_ref = pytest.mark.skipif(ref() is None, reason="oracle/_ref/libsrslte_ref.so is not built")


def _shared(cell, sf_idx):
    """From the reference alone: does a REG of the subframe's srslte_regs_t lie in two PHICH mapping units?"""
    step = 2 if cell.cp_ext else 1
    res = [cell.phich_re_sf(sf_idx, g) for g in range(0, cell.ngroups_sf(sf_idx), step)]
    return len(res) > 0 and np.unique(np.concatenate(res)).size != 12 * len(res)


@needs_ref
@pytest.mark.parametrize("idx", range(5))
def test_helpers_agree_with_the_reference(idx):
    from dl_ctrl_tdd_ref import MI_TDD, TDD_CELLS, TddCell, is_ul
    spec = TDD_CELLS[idx]
    nof_prb, ports, cell_id = spec[:3]
    kw = dict(cp_ext=spec[3], phich_resources=spec[4], phich_ext=spec[5])
    checked = 0
    for sf_config in range(7):
        cell = TddCell(*spec[:7], sf_config)
        dl = [sf for sf in range(10) if not is_ul(sf_config, sf)]
        # what the creators refuse, from the reference alone: a REG in two mapping units, or no CCE at CFI 1 (srslte_regs_pdcch_ncce: -1)
        shared = any(_shared(cell, sf) for sf in dl) or any(cell.ncce6[cell.mi_idx(sf)][0] <= 0 for sf in dl)
        for sf_idx in range(10):
            if is_ul(sf_config, sf_idx):
                assert pkg.tdd_mi(sf_config, sf_idx) < 0
                with pytest.raises(ValueError):
                    pkg.pdcch_re_tdd(nof_prb, ports, cell_id, sf_config, sf_idx, 1, **kw)
                with pytest.raises(ValueError):
                    pkg.phich_ngroups_tdd(nof_prb, ports, cell_id, sf_config, sf_idx, **kw)
                continue
            assert pkg.tdd_mi(sf_config, sf_idx) == MI_TDD[sf_config][sf_idx] == cell.mi(sf_idx)
            for cfi in (1, 2, 3):
                want = cell.pdcch_re_sf(sf_idx, cfi)
                got = pkg.pdcch_re_tdd(nof_prb, ports, cell_id, sf_config, sf_idx, cfi, **kw)
                assert np.array_equal(got, want), (spec, sf_config, sf_idx, cfi)
            ng = cell.ngroups_sf(sf_idx)
            if shared:  # the configuration is one the creators refuse: the helper says so
                with pytest.raises(ValueError):
                    pkg.phich_ngroups_tdd(nof_prb, ports, cell_id, sf_config, sf_idx, **kw)
            else:
                assert pkg.phich_ngroups_tdd(nof_prb, ports, cell_id, sf_config, sf_idx, **kw) == ng
            for g in range(ng):
                assert np.array_equal(pkg.phich_re_tdd(nof_prb, ports, cell_id, sf_config, sf_idx, g, **kw), cell.phich_re_sf(sf_idx, g)), (spec, sf_config,
                                                                                                                                          sf_idx, g)
            with pytest.raises(ValueError):
                pkg.phich_re_tdd(nof_prb, ports, cell_id, sf_config, sf_idx, ng, **kw)
            checked += 1
    assert checked == sum(10 - "".join(u).count("U") for u in __import__("dl_ctrl_tdd_ref").UL_SF)
    assert pkg.tdd_mi(7, 0) < 0 and pkg.tdd_mi(0, 10) < 0


@needs_ref
def test_the_issue_cells_share_no_reg_and_reach_their_branches():
    """The five cells are served with their own configuration - the group helper's error return is the creators' check - and they hold what
    the issue chose them for."""
    from dl_ctrl_tdd_ref import TDD_CELLS, TddCell, is_ul
    variants = []
    for spec in TDD_CELLS:
        cell = TddCell(*spec)
        dl = [sf for sf in range(10) if not is_ul(spec[7], sf)]
        assert not any(_shared(cell, sf) for sf in dl), spec
        kw = dict(cp_ext=spec[3], phich_resources=spec[4], phich_ext=spec[5])
        for sf in dl:
            assert pkg.phich_ngroups_tdd(*spec[:3], spec[7], sf, **kw) == cell.ngroups_sf(sf), (spec, sf)
            assert pkg.pdcch_re_tdd(*spec[:3], spec[7], sf, 3, **kw).size == 36 * cell.ncce6[cell.mi_idx(sf)][2], (spec, sf)
        variants.append({cell.mi_idx(sf) for sf in dl})
    assert variants[0] == {2, 0}                     # configuration 0: mi = 2 and mi = 1
    assert variants[1] == {1, 0, 3}                  # mi = 0, mi = 1, and mi = 1 under the rule of subframes 1 and 6
    assert variants[3] == {0, 1, 4}                  # regs[4] (mi = 0, sf1_6) holds the lists of regs[1]: the device folds the two
    cell = TddCell(*TDD_CELLS[4])
    assert cell.ncce6[1][2] == 88 and cell.max_bits == 72 * 88
    c0 = TddCell(*TDD_CELLS[0])
    c0.select(0)
    assert c0.ngroups_sf(0) == 2 * c0.ngroups_sf(1) and any(c0.calc(lo, dm, 1)[0] < c0.ngroups_sf(0) for lo in range(6) for dm in range(8))


@needs_ref
def test_dci_sizes_of_a_tdd_cell():
    R = ref()
    R.srslte_dci_format_sizeof.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    R.srslte_dci_format_sizeof.restype = C.c_uint32
    differ = 0
    for nof_prb in range(6, 111):
        for ports in (1, 2, 4):
            cell = RefCell(nof_prb, ports, 1, 0, 0, 0, 1)
            for fmt in range(9):
                want = R.srslte_dci_format_sizeof(C.byref(cell), None, None, fmt)
                assert pkg.dci_format_sizeof_tdd(nof_prb, ports, fmt) == want, (nof_prb, ports, fmt)
                differ += want != pkg.dci_format_sizeof(nof_prb, ports, fmt)
            assert pkg.dci_format_sizeof_tdd(nof_prb, ports, 0) == pkg.dci_format_sizeof_tdd(nof_prb, ports, 2)  # formats 0 and 1A: one size
    assert differ > 2000  # every format but 1C grows
    assert pkg.dci_format_sizeof_tdd(5, 1, 0) == 0 and pkg.dci_format_sizeof_tdd(111, 1, 0) == 0


@needs_ref
def test_shared_reg_refusal():
    """6 PRB, Ng = 2, configuration 0: with mi = 2 the reference puts mapping units 0 and 2 on one REG of symbol 0; the helper's error return
    says the creators refuse that cell. Ng = 1 is served."""
    from dl_ctrl_tdd_ref import TddCell
    cell = TddCell(6, 1, 1, False, 3, False, 1, 0)
    assert _shared(cell, 0) and np.intersect1d(cell.phich_re_sf(0, 0), cell.phich_re_sf(0, 2)).size == 4
    for sf_idx in (0, 1, 5, 6):
        with pytest.raises(ValueError):
            pkg.phich_ngroups_tdd(6, 1, 1, 0, sf_idx, phich_resources=3)
    assert pkg.phich_ngroups_tdd(6, 1, 1, 0, 0, phich_resources=2) == 2 and pkg.phich_ngroups_tdd(6, 1, 1, 0, 1, phich_resources=2) == 1
    # the lists themselves are still the reference's
    assert np.array_equal(pkg.phich_re_tdd(6, 1, 1, 0, 0, 2, phich_resources=3), cell.phich_re_sf(0, 2))
    L = pkg.lib()
    cfg = pkg.DlCtrlCfg(6, 1, 1, 0, 3, 0, 1, 1, 1)
    txc = pkg.DlCtrlTxCfg(6, 1, 1, 0, 3, 0, 1, 1, 1, 1)
    assert L.srslte_hip_dl_ctrl_create_tdd(C.byref(cfg), 0) is None and L.srslte_hip_dl_ctrl_tx_create_tdd(C.byref(txc), 0) is None


@needs_ref
def test_no_cce_refusal():
    """25 PRB, Ng = 2, configuration 0: mi = 2 takes 42 of the 46 free REGs of symbol 0, so a CFI-1 region has no CCE (the reference's
    srslte_regs_pdcch_ncce answers -1). Both creators refuse the cell, the helper's error return says so; configuration 6 (mi = 1) is served."""
    from dl_ctrl_tdd_ref import TddCell
    cell = TddCell(25, 1, 9, False, 3, False, 1, 0)
    assert cell.ncce6[2][0] <= 0 < cell.ncce6[0][0] and not _shared(cell, 0)
    for sf_idx in (0, 1, 5, 6):
        with pytest.raises(ValueError):
            pkg.phich_ngroups_tdd(25, 1, 9, 0, sf_idx, phich_resources=3)
    assert pkg.pdcch_re_tdd(25, 1, 9, 0, 0, 1, phich_resources=3).size == 0  # the list itself is the reference's: empty
    assert pkg.phich_ngroups_tdd(25, 1, 9, 6, 0, phich_resources=3) == cell.ngroups_sf(1) == 7
    L = pkg.lib()
    cfg = pkg.DlCtrlCfg(25, 1, 9, 0, 3, 0, 1, 1, 1)
    txc = pkg.DlCtrlTxCfg(25, 1, 9, 0, 3, 0, 1, 1, 1, 1)
    assert L.srslte_hip_dl_ctrl_create_tdd(C.byref(cfg), 0) is None and L.srslte_hip_dl_ctrl_tx_create_tdd(C.byref(txc), 0) is None


def test_creators_refuse_before_touching_a_device():
    L = pkg.lib()
    for tdd, sf_config in ((0, 0), (1, 7), (2, 0)):
        cfg = pkg.DlCtrlCfg(25, 1, 1, 0, 1, 0, tdd, 1, 1)
        txc = pkg.DlCtrlTxCfg(25, 1, 1, 0, 1, 0, tdd, 1, 1, 1)
        assert L.srslte_hip_dl_ctrl_create_tdd(C.byref(cfg), sf_config) is None, (tdd, sf_config)
        assert L.srslte_hip_dl_ctrl_tx_create_tdd(C.byref(txc), sf_config) is None, (tdd, sf_config)
    assert L.srslte_hip_dl_ctrl_create_tdd(None, 0) is None and L.srslte_hip_dl_ctrl_tx_create_tdd(None, 0) is None
    # cfg.tdd alone stays refused by the FDD creators
    assert L.srslte_hip_dl_ctrl_create(C.byref(pkg.DlCtrlCfg(25, 1, 1, 0, 1, 0, 1, 1, 1))) is None
    assert L.srslte_hip_dl_ctrl_tx_create(C.byref(pkg.DlCtrlTxCfg(25, 1, 1, 0, 1, 0, 1, 1, 1, 1))) is None


@needs_ref
def test_near_ties_among_the_phich_draws_of_the_gpu_test():
    """The share of the GPU test's drawn requests that the reference alone puts within the float bound of a tie (the GPU test may set those
    aside, 1 % at most)."""
    from dl_ctrl_tdd_ref import TDD_CELLS, tdd_phich_subframes
    from dl_ctrl_ul_ref import near_tie
    total = ties = ip1 = 0
    for idx, spec in enumerate(TDD_CELLS):
        cell, tti0, subs = tdd_phich_subframes(spec, 7000 + idx)
        for s in subs:
            for p in s["phichs"]:
                r = cell.phich_decode_full(s["tti"], s["y"], s["ce"], s["noise"], *p[:3])
                z, bits, ack, dist = cell.phich_chain(s["tti"], s["y"], s["ce"], s["noise"], r["ngroup"], r["nseq"])
                assert abs(dist - r["distance"]) <= 1e-5 * max(1.0, abs(dist)) and (ack == r["ack"] or near_tie(r)), (spec, p)
                total += 1
                ties += near_tie(r)
                ip1 += p[2] == 1 and idx == 0
    print("TDD PHICH requests drawn: %d, within the bound of a tie for the reference: %d, I_phich = 1 in configuration 0: %d" % (total, ties, ip1))
    assert total > 100 and ties <= 0.01 * total and ip1 >= 3
