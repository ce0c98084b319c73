"""Host side of the DL control region receive (srslte_hip_dl_ctrl_*): the REG lists of the PCFICH and the PDCCH, the PDCCH candidate locations
and the DCI sizes, each against the reference's own function in oracle/_ref/libsrslte_ref.so; and the compile-time resource check of the
new translation unit. No GPU needed."""
import ctypes as C
import importlib

import numpy as np
import pytest

import test_kernel_resources as tkr
from _libs import RefCell, opaque, ref

pkg = importlib.import_module("srslte-emane_amd")

needs_ref = pytest.mark.skipif(ref() is None, reason="oracle/_ref/libsrslte_ref.so is not built")


class RefLoc(C.Structure):
    """srslte_dci_location_t (dci.h:60-63)."""
    _fields_ = [("L", C.c_uint32), ("ncce", C.c_uint32)]


def _cell(nof_prb, nof_ports, cell_id, cp_ext, phich_res, phich_ext):
    return RefCell(nof_prb, nof_ports, cell_id, 1 if cp_ext else 0, 1 if phich_ext else 0, phich_res, 0)


def _ref_regs(nof_prb, nof_ports, cell_id, cp_ext, phich_res, phich_ext):
    """srslte_regs_init on a grid whose REs hold their own index: the order srslte_regs_pcfich_get / _pdcch_get read gives the RE lists."""
    R = ref()
    h = opaque(1 << 16)
    R.srslte_regs_init.argtypes = [C.c_void_p, RefCell]
    assert R.srslte_regs_init(h, _cell(nof_prb, nof_ports, cell_id, cp_ext, phich_res, phich_ext)) == 0
    nsym = 12 if cp_ext else 14
    grid = (np.arange(nsym * 12 * nof_prb, dtype=np.float32) + 0j).astype(np.complex64)
    out = np.zeros(nsym * 12 * nof_prb, np.complex64)
    R.srslte_regs_pcfich_get.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    assert R.srslte_regs_pcfich_get(h, grid.ctypes.data, out.ctypes.data) == 16
    pcfich = out[:16].real.astype(np.uint32)
    pdcch = []
    R.srslte_regs_pdcch_get.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    for cfi in (1, 2, 3):
        n = R.srslte_regs_pdcch_get(h, cfi, grid.ctypes.data, out.ctypes.data)
        assert n >= 0
        pdcch.append(out[:n].real.astype(np.uint32))
    R.srslte_regs_free.argtypes = [C.c_void_p]
    R.srslte_regs_free(h)
    return pcfich, pdcch


@needs_ref
@pytest.mark.parametrize("nof_prb", [6, 15, 25, 50, 75, 100])
def test_reg_lists_match_reference(nof_prb):
    n = 0
    for cp_ext in (False, True):
        for ports in (1, 2, 4):
            for phich_res in range(4):
                for phich_ext in (False, True):
                    for cell_id in ((nof_prb * 7 + ports * 31 + phich_res * 5 + phich_ext) % 504, (nof_prb * 13 + ports + 3 * phich_res + 1) % 504):
                        pc, pd = _ref_regs(nof_prb, ports, cell_id, cp_ext, phich_res, phich_ext)
                        assert np.array_equal(pkg.pcfich_re(nof_prb, ports, cell_id, cp_ext, phich_res, phich_ext), pc), (nof_prb, ports, cell_id)
                        for cfi in (1, 2, 3):
                            mine = pkg.pdcch_re(nof_prb, ports, cell_id, cfi, cp_ext, phich_res, phich_ext)
                            assert mine.size == pd[cfi - 1].size and mine.size % 36 == 0, (nof_prb, ports, cell_id, cp_ext, phich_res, phich_ext, cfi)
                            assert np.array_equal(mine, pd[cfi - 1]), (nof_prb, ports, cell_id, cp_ext, phich_res, phich_ext, cfi)
                            n += 1
    assert n == 2 * 3 * 4 * 2 * 2 * 3


def test_reg_lists_refuse_bad_cells():
    with pytest.raises(ValueError):
        pkg.pdcch_re(5, 1, 0, 1)
    with pytest.raises(ValueError):
        pkg.pdcch_re(50, 3, 0, 1)
    with pytest.raises(ValueError):
        pkg.pdcch_re(50, 1, 0, 4)


@needs_ref
def test_candidate_locations_match_reference():
    R = ref()
    R.srslte_pdcch_ue_locations_ncce.restype = C.c_uint32
    R.srslte_pdcch_ue_locations_ncce.argtypes = [C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint16]
    R.srslte_pdcch_common_locations_ncce.restype = C.c_uint32
    R.srslte_pdcch_common_locations_ncce.argtypes = [C.c_uint32, C.c_void_p, C.c_uint32]
    rng = np.random.default_rng(7)
    loc = (RefLoc * 16)()
    rntis = [1, 0x0A, 0x0B, 0xFFF3, 0xFFFD] + [int(r) for r in rng.integers(0x0B, 0xFFF4, 60)]
    for nof_cce in list(range(0, 90)):
        n = R.srslte_pdcch_common_locations_ncce(nof_cce, loc, 6)
        assert pkg.pdcch_common_locations(nof_cce) == [(loc[i].L, loc[i].ncce) for i in range(n)], nof_cce
        for rnti in rntis[:: 1 if nof_cce % 7 == 0 else 9]:
            for sf_idx in range(10):
                n = R.srslte_pdcch_ue_locations_ncce(nof_cce, loc, 16, sf_idx, rnti)
                assert pkg.pdcch_ue_locations(nof_cce, sf_idx, rnti) == [(loc[i].L, loc[i].ncce) for i in range(n)], (nof_cce, rnti, sf_idx)


@needs_ref
def test_dci_sizes_match_reference():
    R = ref()
    R.srslte_dci_format_sizeof.restype = C.c_uint32
    R.srslte_dci_format_sizeof.argtypes = [C.POINTER(RefCell), C.c_void_p, C.c_void_p, C.c_int]
    for nof_prb in range(6, 111):
        for ports in (1, 2, 4):
            cell = _cell(nof_prb, ports, 1, False, 0, False)
            for fmt in range(9):
                assert pkg.dci_format_sizeof(nof_prb, ports, fmt) == R.srslte_dci_format_sizeof(C.byref(cell), None, None, fmt), (nof_prb, ports, fmt)


@pytest.mark.skipif(not tkr.os.path.exists(tkr.HIPCC), reason="hipcc not available")
def test_dl_ctrl_kernels_use_no_scratch():
    kernels = tkr._remarks("pdcch.hip")
    assert {k for k in kernels if "dl_ctrl" in k} and len(kernels) == 3, kernels
    for k, r in kernels.items():
        assert r.get("ScratchSize [bytes/lane]", 0) == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
