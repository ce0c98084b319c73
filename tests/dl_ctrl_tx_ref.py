"""Reference side of the DL control region transmit tests and of scripts/bench_dl_tx_ctrl.py: the reference's PHICH (srslte_phich_calc /
_encode / _decode, srslte_regs_phich_add) beside the PCFICH / PDCCH encoders of dl_ctrl_ref.Cell, the complete control region of a subframe as
srslte_enb_dl_put_base + _put_phich + _put_pdcch_dl / _ul write it, and the drawing of a subframe's DCIs and PHICHs. Test infrastructure only."""
import ctypes as C
import importlib

import numpy as np

from _libs import RefChestRes, aligned, opaque
from dl_ctrl_ref import F0, F1, F1A, F1C, F2, F2A, SIRNTI, Cell, make_msg

pkg = importlib.import_module("srslte-emane_amd")

TX_FORMATS = [F0, F1, F1A, F1C, F2, F2A]


class RefPhichRes(C.Structure):
    """srslte_phich_resource_t (phich.h:82-85)."""
    _fields_ = [("ngroup", C.c_uint32), ("nseq", C.c_uint32)]


class RefPhichGrant(C.Structure):
    """srslte_phich_grant_t (phich.h:87-91)."""
    _fields_ = [("n_prb_lowest", C.c_uint32), ("n_dmrs", C.c_uint32), ("I_phich", C.c_uint32)]


class RefPhichDec(C.Structure):
    """srslte_phich_res_t (phich.h:93-96)."""
    _fields_ = [("ack_value", C.c_bool), ("distance", C.c_float)]


class TxCell(Cell):
    """dl_ctrl_ref.Cell plus the reference's PHICH of the same srslte_regs_t."""

    def __init__(self, nof_prb, ports, cell_id, cp_ext, phich_res, phich_ext, nof_rx=1):
        super().__init__(nof_prb, ports, cell_id, cp_ext, phich_res, phich_ext, nof_rx)
        R, vp = self.R, C.c_void_p
        R.srslte_phich_init.argtypes = [vp, C.c_uint32]
        R.srslte_phich_set_cell.argtypes = [vp, vp, type(self.cell)]
        R.srslte_phich_calc.argtypes = [vp, C.POINTER(RefPhichGrant), C.POINTER(RefPhichRes)]
        R.srslte_phich_encode.argtypes = [vp, vp, RefPhichRes, C.c_uint8, vp]
        R.srslte_phich_decode.argtypes = [vp, vp, vp, RefPhichRes, vp, C.POINTER(RefPhichDec)]
        R.srslte_phich_ngroups.restype = C.c_uint32
        R.srslte_phich_ngroups.argtypes = [vp]
        R.srslte_regs_phich_add.argtypes = [vp, vp, C.c_uint32, vp]
        self.phich = opaque(1 << 16)
        assert R.srslte_phich_init(self.phich, 1) == 0 and R.srslte_phich_set_cell(self.phich, self.regs, self.cell) == 0
        self.cp_ext = cp_ext

    def ngroups(self):
        return self.R.srslte_phich_ngroups(self.phich)

    def calc(self, n_prb_lowest, n_dmrs, I_phich):
        r = RefPhichRes()
        self.R.srslte_phich_calc(self.phich, C.byref(RefPhichGrant(n_prb_lowest, n_dmrs, I_phich)), C.byref(r))
        return r.ngroup, r.nseq

    def phich_re(self, ngroup):
        """Where srslte_regs_phich_add puts the 12 symbols of a group: 12 distinct values added into a zero grid, read back."""
        grid = aligned(self.glen, np.complex64)
        sym = aligned(12, np.complex64)
        sym[:] = np.arange(1, 13)
        assert self.R.srslte_regs_phich_add(self.regs, sym.ctypes.data, ngroup, grid.ctypes.data) == 12
        nz = np.flatnonzero(grid)
        assert nz.size == 12
        return nz[np.argsort(grid[nz].real)].astype(np.uint32)

    def encode_full(self, tti, cfi, msgs, phichs):
        """Zero grids, srslte_pcfich_encode, srslte_phich_calc + srslte_phich_encode of each (n_prb_lowest, n_dmrs, I_phich, ack) in order,
        srslte_pdcch_encode of each message in order -> [ports][glen]. The messages' payloads get the CRC written behind nof_bits."""
        R = self.R
        grids = [aligned(self.glen, np.complex64) for _ in range(4)]
        ptrs = (C.c_void_p * 4)(*[g.ctypes.data for g in grids])
        sf = self.sf(tti, cfi)
        assert R.srslte_pcfich_encode(self.pcf, C.byref(sf), ptrs) == 0
        for n_prb_lowest, n_dmrs, I_phich, ack in phichs:
            r = RefPhichRes()
            R.srslte_phich_calc(self.phich, C.byref(RefPhichGrant(n_prb_lowest, n_dmrs, I_phich)), C.byref(r))
            assert R.srslte_phich_encode(self.phich, C.byref(sf), r, ack, ptrs) == 0
        for m in msgs:
            assert R.srslte_pdcch_encode(self.enc, C.byref(sf), C.byref(m), ptrs) == 0
        return np.stack(grids[:self.ports])

    def phich_decode(self, tti, y, n_prb_lowest, n_dmrs, I_phich):
        """srslte_phich_decode of one PHICH on the single-antenna grid y with unit channel estimates of every port and no noise -> ack."""
        ones = aligned(self.glen, np.complex64)
        ones[:] = 1
        res = RefChestRes()
        for p in range(self.ports):
            res.ce[p][0] = ones.ctypes.data
        res.noise_estimate = 0.0
        ya = aligned(self.glen, np.complex64)
        ya[:] = y
        ptrs = (C.c_void_p * 4)(ya.ctypes.data, None, None, None)
        r = RefPhichRes()
        self.R.srslte_phich_calc(self.phich, C.byref(RefPhichGrant(n_prb_lowest, n_dmrs, I_phich)), C.byref(r))
        out = RefPhichDec()
        assert self.R.srslte_phich_decode(self.phich, C.byref(self.sf(tti, 0)), C.byref(res), r, ptrs, C.byref(out)) == 0
        return int(out.ack_value)


def draw_dcis(cell, cfi, rng, tries=12, used=None, formats=TX_FORMATS):
    """DCIs at random non-overlapping locations of every aggregation level, formats 0 / 1 / 1A / 1C / 2 / 2A with this cell's sizes, random
    RNTIs (SI-RNTI among them)."""
    ncce = cell.ncce[cfi - 1]
    used = np.zeros(ncce, bool) if used is None else used
    msgs = []
    for _ in range(tries):
        L = int(rng.integers(0, 4))
        if (1 << L) > ncce:
            continue
        n0 = (1 << L) * int(rng.integers(0, ncce >> L))
        if used[n0:n0 + (1 << L)].any():
            continue
        used[n0:n0 + (1 << L)] = True
        fmt = formats[int(rng.integers(0, len(formats)))]
        rnti = SIRNTI if rng.random() < 0.15 else int(rng.integers(1, 0xFFF4))
        msgs.append(make_msg(rnti, L, n0, fmt, pkg.dci_format_sizeof(cell.nof_prb, cell.ports, fmt), rng))
    return msgs


def draw_phichs(cell, rng, nmax=10):
    """(n_prb_lowest, n_dmrs, I_phich, ack) of up to nmax PHICHs, several in one group (a few shared n_prb_lowest), both acks; I_phich 1 only
    where it names a group (extended CP)."""
    n = int(rng.integers(0, nmax + 1))
    lows = rng.integers(0, cell.nof_prb, 3)
    out = []
    for _ in range(n):
        out.append((int(lows[int(rng.integers(0, 3))]) if rng.random() < 0.6 else int(rng.integers(0, cell.nof_prb)), int(rng.integers(0, 8)),
                    int(rng.integers(0, 2)) if cell.cp_ext else 0, int(rng.integers(0, 2))))
    return out


def control_res(cell, cfi, msgs):
    """The REs a control region with these DCIs writes: PCFICH, every PHICH REG, the DCIs' CCEs."""
    kw = cell.kw
    re = [pkg.pcfich_re(cell.nof_prb, cell.ports, cell.cell_id, **kw)]
    for g in range(pkg.phich_ngroups(cell.nof_prb, cell.ports, cell.cell_id, **kw)):
        re.append(pkg.phich_re(cell.nof_prb, cell.ports, cell.cell_id, g, **kw))
    pd = pkg.pdcch_re(cell.nof_prb, cell.ports, cell.cell_id, cfi, **kw)
    for m in msgs:
        re.append(pd[36 * m.ncce:36 * (m.ncce + (1 << m.L))])
    return np.unique(np.concatenate(re))
