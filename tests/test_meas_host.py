"""The host side of the neighbour-cell measurement (no device): every refusal of srslte_hip_meas_check."""
import importlib

import pytest

pkg = importlib.import_module("srslte-emane_amd")
INVALID = -2


def test_check_accepts_the_measurement_shapes():
    assert pkg.meas_check(pkg.meas_cfg(6, 3, 6, 5), 5 * 1920, 5, 3, 6) == 0
    assert pkg.meas_check(pkg.meas_cfg(6, 3, 6, 12), 12 * 1920 + 77, 12, 1, 1) == 0
    assert pkg.meas_check(pkg.meas_cfg(100, 1, 3, 3), 3 * 23040, 3, 1, 3) == 0
    assert pkg.meas_check(pkg.meas_cfg(100, 1, 3, 3, symbol_sz=2048), 3 * 30720, 3, 1, 3) == 0
    assert pkg.meas_check(pkg.meas_cfg(110, 8, 8, 5, threshold=7.0), 5 * 23040, 2, 8, 8) == 0
    assert pkg.meas_check(pkg.meas_cfg(25, 1, 1, 2), 2 * 5760, 2, 0, 0) == 0


@pytest.mark.parametrize("kw", [dict(cp_ext=True), dict(nof_prb=5), dict(nof_prb=111), dict(nof_prb=0), dict(symbol_sz=640), dict(symbol_sz=4096),
                                dict(nof_prb=25, symbol_sz=256), dict(nof_prb=100, symbol_sz=1024), dict(max_captures=0), dict(max_cells=0),
                                dict(max_cells=505), dict(max_captures=200, max_cells=400), dict(max_sf=1), dict(max_sf=0), dict(max_sf=3000000),
                                dict(threshold=-1.0), dict(threshold=float("nan"))])
def test_check_refuses_configurations(kw):
    base = dict(nof_prb=6, max_captures=2, max_cells=3, max_sf=5)
    base.update(kw)
    c = pkg.meas_cfg(**base)
    assert pkg.meas_check(c, 1 << 24, 2, 1, 1) == INVALID
    assert pkg.meas_check(c, 1 << 24, 2, 0, 0) == INVALID


def test_check_refuses_calls():
    c = pkg.meas_cfg(6, 2, 3, 5)
    L = 1920
    assert pkg.meas_check(c, 5 * L, 5, 2, 3) == 0
    assert pkg.meas_check(c, 5 * L, 1, 2, 3) == INVALID       # nof_sf < 2: no block to search
    assert pkg.meas_check(c, 5 * L, 0, 2, 3) == INVALID
    assert pkg.meas_check(c, 6 * L, 6, 2, 3) == INVALID       # nof_sf > max_sf
    assert pkg.meas_check(c, 5 * L - 1, 5, 2, 3) == INVALID   # in_stride < nof_sf sf_len
    assert pkg.meas_check(c, 4 * L, 4, 2, 3) == 0
    assert pkg.meas_check(c, 5 * L, 5, 3, 3) == INVALID       # more captures than the object was made for
    assert pkg.meas_check(c, 5 * L, 5, 2, 4) == INVALID       # more cells
    assert pkg.lib().srslte_hip_meas_check(None, 5 * L, 5, 2, 3) == INVALID
    c2 = pkg.meas_cfg(100, 1, 1, 3, symbol_sz=2048)
    assert pkg.meas_check(c2, 3 * 30720 - 1, 3, 1, 1) == INVALID and pkg.meas_check(c2, 3 * 30720, 3, 1, 1) == 0


def test_device_entry_points_refuse_null_objects_without_a_device():
    L = pkg.lib()
    assert L.srslte_hip_meas_create(None) is None
    assert L.srslte_hip_meas_set_cells(None, None, 1, None) == INVALID
    assert L.srslte_hip_meas_run_batch(None, None, 0, 2, 1, None, None) == INVALID
    assert L.srslte_hip_meas_replicas(None, 0, None) == INVALID
    bad = pkg.meas_cfg(6, 1, 1, 5, cp_ext=True)
    import ctypes as C
    assert L.srslte_hip_meas_create(C.byref(bad)) is None
