"""Host side of the DL broadcast channels (srslte_hip_dl_ctrl_tx_put_bcast, srslte_hip_dl_ctrl_mib_batch): the PBCH RE list, the PSS / SSS
positions and values and srslte_pbch_mib_pack against the reference's own functions in oracle/_ref/libsrslte_ref.so, and the compile-time
resource check of the new translation unit. No GPU needed."""
import importlib

import numpy as np
import pytest

import test_kernel_resources as tkr
from _libs import ref

pkg = importlib.import_module("srslte-emane_amd")

needs_ref = pytest.mark.skipif(ref() is None, reason="oracle/_ref/libsrslte_ref.so is not built")


@needs_ref
@pytest.mark.parametrize("nof_prb", [6, 15, 25, 50, 75, 100, 110])
@pytest.mark.parametrize("cp_ext", [False, True])
def test_pbch_re_match_reference(nof_prb, cp_ext):
    from dl_bcast_ref import BcastCell
    for v in range(3):
        cell_id = 3 * ((nof_prb * 7 + 11 * cp_ext) % 168) + v
        for ports in (1, 2, 4):
            cell = BcastCell(nof_prb, ports, cell_id, cp_ext)
            mine = pkg.pbch_re(nof_prb, ports, cell_id, cp_ext=cp_ext)
            assert mine.size == (216 if cp_ext else 240)
            assert np.array_equal(mine, cell.pbch_put_re()), (nof_prb, ports, cell_id, cp_ext)
            assert np.array_equal(mine, cell.pbch_get_re()), (nof_prb, ports, cell_id, cp_ext)


@needs_ref
@pytest.mark.parametrize("cp_ext", [False, True])
def test_sync_re_match_reference(cp_ext):
    """All 504 cell IDs, subframes 0 and 5, on an even and an odd bandwidth: positions, values and zero guards bit for bit."""
    from dl_bcast_ref import BcastCell
    for nof_prb in (6, 25, 15):
        for cell_id in range(504):
            cell = BcastCell(nof_prb, 1, cell_id, cp_ext)
            for sf_idx in (0, 5):
                want = np.zeros(cell.glen, np.complex64)
                marker = np.complex64(7 + 7j)
                want[:] = marker
                cell.put_sync(want, sf_idx)
                re, val = pkg.sync_re(nof_prb, cell_id, sf_idx, cp_ext=cp_ext)
                touched = np.flatnonzero(want != marker)
                assert set(touched) <= set(re.tolist()), (nof_prb, cell_id, sf_idx)
                assert np.array_equal(want[re].view(np.uint32), val.view(np.uint32)), (nof_prb, cell_id, sf_idx, cp_ext)
                assert np.count_nonzero(val) == 124 and not val[:5].any() and not val[67:77].any() and not val[139:].any()


@needs_ref
def test_mib_pack_match_reference():
    from dl_bcast_ref import BcastCell
    for nof_prb in (6, 15, 25, 50, 75, 100, 110):
        for phich_res in range(4):
            for phich_ext in (False, True):
                cell = BcastCell(nof_prb, 1, 1, False, phich_res, phich_ext)
                for sfn in range(1024):
                    assert np.array_equal(pkg.mib_pack(nof_prb, phich_ext, phich_res, sfn), cell.mib_pack(sfn)), (nof_prb, phich_res, phich_ext, sfn)


def test_bcast_helpers_refuse_bad_input():
    with pytest.raises(ValueError):
        pkg.pbch_re(5, 1, 0)
    with pytest.raises(ValueError):
        pkg.pbch_re(50, 3, 0)
    with pytest.raises(ValueError):
        pkg.sync_re(50, 0, 1)
    with pytest.raises(ValueError):
        pkg.sync_re(50, 504, 0)
    with pytest.raises(ValueError):
        pkg.mib_pack(50, False, 4, 0)


@pytest.mark.skipif(not tkr.os.path.exists(tkr.HIPCC), reason="hipcc not available")
def test_bcast_kernels_use_no_scratch():
    kernels = tkr._remarks("pbch.hip")
    assert {k for k in kernels if "dl_bcast_tx" in k} and {k for k in kernels if "dl_mib" in k} and len(kernels) == 2, kernels
    for k, r in kernels.items():
        assert r.get("ScratchSize [bytes/lane]", 0) == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
