"""Host side of the DL control region transmit (srslte_hip_dl_ctrl_tx_*): the PHICH REG lists, group counts and srslte_phich_calc against the
reference's own functions in oracle/_ref/libsrslte_ref.so, the compile-time resource check of the new translation unit. No GPU needed."""
import importlib

import numpy as np
import pytest

import test_kernel_resources as tkr
from _libs import ref

pkg = importlib.import_module("srslte-emane_amd")

needs_ref = pytest.mark.skipif(ref() is None, reason="oracle/_ref/libsrslte_ref.so is not built")


def _cells(nof_prb):
    for cp_ext in (False, True):
        for ports in (1, 2, 4):
            for phich_res in range(4):
                for phich_ext in (False, True):
                    yield ports, (nof_prb * 11 + ports * 37 + phich_res * 7 + phich_ext * 3 + cp_ext) % 504, cp_ext, phich_res, phich_ext


@needs_ref
@pytest.mark.parametrize("nof_prb", [6, 15, 25, 50, 75, 100])
def test_phich_re_match_reference(nof_prb):
    from dl_ctrl_tx_ref import TxCell
    n = 0
    for ports, cell_id, cp_ext, phich_res, phich_ext in _cells(nof_prb):
        cell = TxCell(nof_prb, ports, cell_id, cp_ext, phich_res, phich_ext)
        kw = dict(cp_ext=cp_ext, phich_resources=phich_res, phich_ext=phich_ext)
        ng = pkg.phich_ngroups(nof_prb, ports, cell_id, **kw)
        assert ng == cell.ngroups() > 0, (nof_prb, ports, cell_id, kw)
        seen = []
        for g in range(ng):
            mine = pkg.phich_re(nof_prb, ports, cell_id, g, **kw)
            assert np.array_equal(mine, cell.phich_re(g)), (nof_prb, ports, cell_id, kw, g)
            seen.append(mine)
        # no PHICH RE is a PCFICH or PDCCH RE of any CFI
        allre = np.concatenate(seen)
        others = np.concatenate([pkg.pcfich_re(nof_prb, ports, cell_id, **kw)] + [pkg.pdcch_re(nof_prb, ports, cell_id, c, **kw) for c in (1, 2, 3)])
        assert not np.isin(allre, others).any()
        with pytest.raises(ValueError):
            pkg.phich_re(nof_prb, ports, cell_id, ng + (1 if cp_ext else 0) + 1, **kw)
        n += 1
    assert n == 2 * 3 * 4 * 2


@needs_ref
@pytest.mark.parametrize("nof_prb", [6, 15, 25, 50, 75, 100])
def test_phich_calc_match_reference(nof_prb):
    from dl_ctrl_tx_ref import TxCell
    for ports, cell_id, cp_ext, phich_res, phich_ext in list(_cells(nof_prb))[::5]:
        cell = TxCell(nof_prb, ports, cell_id, cp_ext, phich_res, phich_ext)
        kw = dict(cp_ext=cp_ext, phich_resources=phich_res, phich_ext=phich_ext)
        for n_prb_lowest in range(nof_prb):
            for n_dmrs in range(8):
                for I_phich in range(2):
                    assert pkg.phich_calc(nof_prb, ports, cell_id, n_prb_lowest, n_dmrs, I_phich, **kw) == cell.calc(n_prb_lowest, n_dmrs, I_phich), \
                        (nof_prb, ports, cell_id, kw, n_prb_lowest, n_dmrs, I_phich)


def test_phich_helpers_refuse_bad_cells():
    with pytest.raises(ValueError):
        pkg.phich_ngroups(5, 1, 0)
    with pytest.raises(ValueError):
        pkg.phich_calc(50, 3, 0, 0, 0, 0)
    with pytest.raises(ValueError):
        pkg.phich_re(50, 1, 0, 0, phich_resources=4)


@pytest.mark.skipif(not tkr.os.path.exists(tkr.HIPCC), reason="hipcc not available")
def test_dl_ctrl_tx_kernels_use_no_scratch():
    kernels = tkr._remarks("pdcch_tx.hip")
    assert {k for k in kernels if "dl_ctrl_tx" in k} and len(kernels) == 2, kernels
    for k, r in kernels.items():
        assert r.get("ScratchSize [bytes/lane]", 0) == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
