"""Reference side of the TDD control region and broadcast tests: dl_ctrl_ul_ref.UlCell (dl_ctrl_ref.Cell + dl_ctrl_tx_ref.TxCell + the PHICH
receiver) on a cell with frame_type TDD, holding the six srslte_regs_t of srslte_ue_dl_set_cell (ue_dl.c:184-189) and switching the PDCCH and
PHICH objects to the subframe's own with srslte_pdcch_set_regs / srslte_phich_set_regs as set_mi_value does (ue_dl.c:315-332); and the drawing
of TDD subframes. Test infrastructure only."""
import ctypes as C
import importlib

import numpy as np

from _libs import RefCell, RefDlSfCfg, opaque
from dl_ctrl_ref import F0, F1, F1A, F1C, F2A, SIRNTI, UE_FORMATS, _R, make_msg
from dl_ctrl_tx_ref import RefPhichDec, RefPhichGrant, RefPhichRes  # noqa: F401
from dl_ctrl_ul_ref import UlCell

pkg = importlib.import_module("srslte-emane_amd")

# the cells of the issue: (nof_prb, ports, cell_id, cp_ext, phich_res, phich_ext, nof_rx, tdd_sf_config). phich_res is srslte_phich_r_t:
# 0-3 = Ng 1/6, 1/2, 1, 2
TDD_CELLS = [(6, 1, 1, False, 2, False, 1, 0),      # mi 2 and 1 in one frame, I_phich = 1
             (15, 2, 77, False, 1, True, 2, 1),     # extended PHICH: the subframe-1/6 variant with mi = 1, beside mi = 0 and plain mi = 1
             (25, 4, 200, True, 3, False, 3, 6),    # extended CP, Ng = 2
             (50, 2, 150, True, 1, True, 4, 3),     # extended CP and PHICH; subframe 6 is a normal DL subframe that still gets the CFI clamp
             (100, 1, 5, False, 0, False, 2, 5)]    # mi = 0 almost everywhere, 88 CCEs at CFI 3, the stride

MI_TDD = [[2, 1, 0, 0, 0, 2, 1, 0, 0, 0], [0, 1, 0, 0, 1, 0, 1, 0, 0, 1], [0, 0, 0, 1, 0, 0, 0, 0, 1, 0], [1, 0, 0, 0, 0, 0, 0, 0, 1, 1],
          [0, 0, 0, 0, 0, 0, 0, 0, 1, 1], [0, 0, 0, 0, 0, 0, 0, 0, 1, 0], [1, 1, 0, 0, 0, 1, 1, 0, 0, 1]]  # 36.213 Table 6.9-1 (ue_dl.c:49-55)
UL_SF = ["DSUUUDSUUU", "DSUUDDSUUD", "DSUDDDSUDD", "DSUUUDDDDD", "DSUUDDDDDD", "DSUDDDDDDD", "DSUUUDSUUD"]  # 36.211 Table 4.2-2
MI_REG_IDX = (1, 0, 2)  # mi_reg_idx = mi_reg_idx_inv (ue_dl.c:45-46)


def is_ul(sf_config, sf_idx):
    return UL_SF[sf_config][sf_idx] == "U"


class TddCell(UlCell):
    """The reference's control-region objects of a TDD cell. select(tti) points them at regs[MI_IDX(tti % 10)]; every method that takes a tti
    does that first, so the inherited encoders, receivers and restated chains run over the subframe's own srslte_regs_t."""

    def __init__(self, nof_prb, ports, cell_id, cp_ext, phich_res, phich_ext, nof_rx, sf_config, frame_type=1):
        self.R = R = _R()
        vp = C.c_void_p
        self.nof_prb, self.ports, self.cell_id, self.nof_rx, self.sf_config = nof_prb, ports, cell_id, nof_rx, sf_config
        self.cell = RefCell(nof_prb, ports, cell_id, 1 if cp_ext else 0, 1 if phich_ext else 0, phich_res, frame_type)
        self.kw = dict(cp_ext=cp_ext, phich_resources=phich_res, phich_ext=phich_ext)
        self.cp_ext, self.phich_ext = cp_ext, phich_ext
        self.glen = (12 if cp_ext else 14) * 12 * nof_prb
        R.srslte_regs_init_opts.argtypes = [vp, RefCell, C.c_uint32, C.c_bool]
        R.srslte_regs_phich_ngroups.argtypes = [vp]
        R.srslte_regs_pdcch_nregs.argtypes = [vp, C.c_uint32]
        R.srslte_pdcch_set_regs.argtypes = [vp, vp]
        R.srslte_phich_set_regs.argtypes = [vp, vp]
        R.srslte_phich_init.argtypes = [vp, C.c_uint32]
        R.srslte_phich_set_cell.argtypes = [vp, vp, RefCell]
        R.srslte_phich_calc.argtypes = [vp, C.POINTER(RefPhichGrant), C.POINTER(RefPhichRes)]
        R.srslte_phich_encode.argtypes = [vp, vp, RefPhichRes, C.c_uint8, vp]
        R.srslte_phich_decode.argtypes = [vp, vp, vp, RefPhichRes, vp, C.POINTER(RefPhichDec)]
        R.srslte_phich_ngroups.restype = C.c_uint32
        R.srslte_phich_ngroups.argtypes = [vp]
        R.srslte_regs_phich_add.argtypes = [vp, vp, C.c_uint32, vp]
        R.srslte_regs_phich_get.argtypes = [vp, vp, vp, C.c_uint32]
        R.srslte_sequence_phich.argtypes = [vp, C.c_uint32, C.c_uint32]
        R.srslte_scrambling_c.argtypes = [vp, vp]
        R.srslte_dci_format_sizeof.argtypes = [vp, vp, vp, C.c_int]
        R.srslte_dci_format_sizeof.restype = C.c_uint32
        # the six srslte_regs_t of ue_dl.c:184-189
        self.regs6 = [opaque(1 << 16) for _ in range(6)]
        for i, r in enumerate(self.regs6):
            assert R.srslte_regs_init_opts(r, self.cell, MI_REG_IDX[i % 3], i > 2) == 0
        self.ncce6 = [[R.srslte_regs_pdcch_ncce(r, c) for c in (1, 2, 3)] for r in self.regs6]
        # the objects as srslte_ue_dl_set_cell sets them up: PCFICH on regs[0], PHICH on regs[2] (mi = 2), PDCCH on regs[1] (mi = 0)
        self.pcf, self.pcf_rx, self.enc, self.dec = opaque(1 << 16), opaque(1 << 16), opaque(1 << 16), opaque(1 << 16)
        self.phich, self.phich_rx = opaque(1 << 16), opaque(1 << 16)
        assert R.srslte_pcfich_init(self.pcf, 1) == 0 and R.srslte_pcfich_set_cell(self.pcf, self.regs6[0], self.cell) == 0
        assert R.srslte_pcfich_init(self.pcf_rx, nof_rx) == 0 and R.srslte_pcfich_set_cell(self.pcf_rx, self.regs6[0], self.cell) == 0
        assert R.srslte_pdcch_init_enb(self.enc, nof_prb) == 0 and R.srslte_pdcch_set_cell(self.enc, self.regs6[1], self.cell) == 0
        assert R.srslte_pdcch_init_ue(self.dec, nof_prb, nof_rx) == 0 and R.srslte_pdcch_set_cell(self.dec, self.regs6[1], self.cell) == 0
        assert R.srslte_phich_init(self.phich, 1) == 0 and R.srslte_phich_set_cell(self.phich, self.regs6[2], self.cell) == 0
        assert R.srslte_phich_init(self.phich_rx, nof_rx) == 0 and R.srslte_phich_set_cell(self.phich_rx, self.regs6[2], self.cell) == 0
        self.max_bits = 72 * self.ncce6[1][2]  # q->max_bits of the PDCCH: CFI 3 with mi = 0
        self.select(0)

    def mi(self, sf_idx):
        return MI_TDD[self.sf_config][sf_idx] if self.cell.frame_type else 1

    def mi_idx(self, sf_idx):
        """MI_IDX of ue_dl.c:57-62."""
        return MI_REG_IDX[self.mi(sf_idx)] + (3 if self.cell.frame_type and self.phich_ext and sf_idx in (1, 6) else 0)

    def select(self, tti):
        """set_mi_value (ue_dl.c:315-332) for every object of this cell."""
        i = self.mi_idx(tti % 10)
        self.regs, self.ncce = self.regs6[i], self.ncce6[i]
        for q in (self.enc, self.dec):
            self.R.srslte_pdcch_set_regs(q, self.regs)
        for q in (self.phich, self.phich_rx):
            self.R.srslte_phich_set_regs(q, self.regs)
        return i

    def sf(self, tti, cfi):
        s = RefDlSfCfg()
        s.tti, s.cfi = tti, cfi
        s.tdd_config.sf_config, s.tdd_config.ss_config, s.tdd_config.configured = self.sf_config, 0, True
        return s

    def ngroups_sf(self, sf_idx):
        """srslte_regs_phich_ngroups of the subframe's srslte_regs_t (0 with mi = 0: regs_phich_init is not run)."""
        return self.R.srslte_regs_phich_ngroups(self.regs6[self.mi_idx(sf_idx)]) if self.mi(sf_idx) else 0

    def dci_sizeof(self, fmt):
        return self.R.srslte_dci_format_sizeof(C.byref(self.cell), None, None, fmt)

    # every inherited method with a tti runs on the subframe's own REGs
    def encode(self, tti, cfi, msgs):
        self.select(tti)
        return super().encode(tti, cfi, msgs)

    def encode_full(self, tti, cfi, msgs, phichs):
        self.select(tti)
        return super().encode_full(tti, cfi, msgs, phichs)

    def extract(self, tti, cfi, y, ce, noise):
        self.select(tti)
        return super().extract(tti, cfi, y, ce, noise)

    def decode_msg(self, tti, cfi, L, ncce, fmt):
        self.select(tti)
        return super().decode_msg(tti, cfi, L, ncce, fmt)

    def llr_chain(self, tti, cfi, y, ce, noise):
        self.select(tti)
        return super().llr_chain(tti, cfi, y, ce, noise)

    def phich_decode_full(self, tti, y, ce, noise, n_prb_lowest, n_dmrs, I_phich):
        self.select(tti)
        return super().phich_decode_full(tti, y, ce, noise, n_prb_lowest, n_dmrs, I_phich)

    def phich_re_sf(self, sf_idx, ngroup):
        self.select(sf_idx)
        return self.phich_re(ngroup)

    def pdcch_re_sf(self, sf_idx, cfi):
        """What srslte_regs_pdcch_get reads of a grid holding its own indices."""
        from _libs import aligned
        self.select(sf_idx)
        n = 36 * self.ncce[cfi - 1]
        if n <= 0:  # fewer than nine REGs are left (25 PRB, Ng = 2, mi = 2 at CFI 1): no CCE (srslte_regs_pdcch_ncce answers -1)
            return np.zeros(0, np.uint32)
        grid, out = aligned(self.glen, np.complex64), aligned(max(n, 1), np.complex64)
        grid[:] = np.arange(self.glen)
        assert self.R.srslte_regs_pdcch_get(self.regs, cfi, grid.ctypes.data, out.ctypes.data) == n
        return out[:n].real.astype(np.uint32)


def sizeof(cell, fmt):
    return pkg.dci_format_sizeof_tdd(cell.nof_prb, cell.ports, fmt)


def draw_tdd_phichs(cell, sf_idx, rng, nmax=8):
    """(n_prb_lowest, n_dmrs, I_phich, ack) of distinct PHICH resources the subframe has: I_phich = 1 where mi = 2 (and where an extended-CP
    cell's doubled groups make it name one), several in one mapping unit."""
    ng = cell.ngroups_sf(sf_idx)
    if ng == 0:
        return []
    cell.select(sf_idx)
    seen, out = set(), []
    lows = rng.integers(0, cell.nof_prb, 3)
    for _ in range(int(rng.integers(1, nmax + 1))):
        lo = int(lows[int(rng.integers(0, 3))]) if rng.random() < 0.6 else int(rng.integers(0, cell.nof_prb))
        p = (lo, int(rng.integers(0, 8)), int(rng.integers(0, 2)))
        key = cell.calc(*p)
        if key[0] < ng and key not in seen:
            seen.add(key)
            out.append(p + (int(rng.integers(0, 2)),))
    return out


def max_cfi(sf_idx):
    return 2 if sf_idx in (1, 6) else 3


def draw_tdd_dcis(cell, tti, cfi, rng, tries=10):
    """DCIs at random non-overlapping locations with this TDD cell's sizes (dl_ctrl_tx_ref.draw_dcis with the TDD sizes)."""
    cell.select(tti)
    ncce = cell.ncce[cfi - 1]
    used, msgs = np.zeros(ncce, bool), []
    for _ in range(tries):
        L = int(rng.integers(0, 4))
        if (1 << L) > ncce:
            continue
        n0 = (1 << L) * int(rng.integers(0, ncce >> L))
        if used[n0:n0 + (1 << L)].any():
            continue
        used[n0:n0 + (1 << L)] = True
        fmt = [F0, F1, F1A, F1C, 6, F2A][int(rng.integers(0, 6))]
        rnti = SIRNTI if rng.random() < 0.15 else int(rng.integers(1, 0xFFF4))
        msgs.append(make_msg(rnti, L, n0, fmt, sizeof(cell, fmt), rng))
    return msgs


def draw_tdd_subframe(cell, tti, cfi, rnti, tm, rng, kind):
    """dl_ctrl_ref.draw_subframe with the TDD sizes and the subframe's own CCE count."""
    cell.select(tti)
    ncce = cell.ncce[cfi - 1]
    used, msgs = np.zeros(ncce, bool), []

    def place(L, n0):
        if n0 + (1 << L) > ncce or used[n0:n0 + (1 << L)].any():
            return False
        used[n0:n0 + (1 << L)] = True
        return True

    if kind in ("ue", "ul"):
        fmt = F0 if kind == "ul" else UE_FORMATS[tm][int(rng.integers(0, 2))]
        locs = pkg.pdcch_ue_locations(ncce, tti % 10, rnti)
        if fmt in (F0, F1A) and rng.random() < 0.3 and pkg.pdcch_common_locations(ncce):
            locs = pkg.pdcch_common_locations(ncce)
        rng.shuffle(locs)
        for L, n0 in locs:
            if place(L, n0):
                msgs.append(make_msg(rnti, L, n0, fmt, sizeof(cell, fmt), rng))
                break
    elif kind in ("si1a", "si1c"):
        fmt = F1A if kind == "si1a" else F1C
        for L, n0 in pkg.pdcch_common_locations(ncce):
            if place(L, n0):
                msgs.append(make_msg(SIRNTI, L, n0, fmt, sizeof(cell, fmt), rng))
                break
    placed = len(msgs) > 0
    for _ in range(3):
        L = int(rng.integers(0, 4))
        n0 = (1 << L) * int(rng.integers(0, max(1, ncce >> L)))
        if place(L, n0):
            fmt = [F0, F1, F1A, F2A][int(rng.integers(0, 4))]
            msgs.append(make_msg(int(rng.integers(0x100, 0xFF00)), L, n0, fmt, sizeof(cell, fmt), rng))
    return msgs, placed


def draw_tdd_ul_subframe(cell, tti, cfi, rnti, tm, rng):
    """dl_ctrl_ul_ref.draw_ul_subframe with the TDD sizes."""
    cell.select(tti)
    ncce = cell.ncce[cfi - 1]
    used, msgs = np.zeros(ncce, bool), []

    def place(L, n0):
        if n0 + (1 << L) > ncce or used[n0:n0 + (1 << L)].any():
            return False
        used[n0:n0 + (1 << L)] = True
        return True

    ue, com = pkg.pdcch_ue_locations(ncce, tti % 10, rnti), pkg.pdcch_common_locations(ncce)
    for _ in range(1 + int(rng.random() < 0.3)):
        locs = list(com) if com and rng.random() < 0.3 else list(ue)
        rng.shuffle(locs)
        for L, n0 in locs:
            if place(L, n0):
                msgs.append(make_msg(rnti, L, n0, F0, sizeof(cell, F0), rng))
                break
    if rng.random() < 0.6:
        fmt = UE_FORMATS[tm][int(rng.integers(0, 2))]
        locs = list(ue)
        rng.shuffle(locs)
        for L, n0 in locs:
            if place(L, n0):
                msgs.append(make_msg(rnti, L, n0, fmt, sizeof(cell, fmt), rng))
                break
    for _ in range(3):
        L = int(rng.integers(0, 4))
        n0 = (1 << L) * int(rng.integers(0, max(1, ncce >> L)))
        if place(L, n0):
            fmt = [F0, F1, F1A, F2A][int(rng.integers(0, 4))]
            msgs.append(make_msg(int(rng.integers(0x100, 0xFF00)), L, n0, fmt, sizeof(cell, fmt), rng))
    return msgs


PHICH_SNRS = (30.0, 10.0)


def tdd_phich_subframes(spec, seed, nof_frames=2):
    """nof_frames frames of consecutive subframes from a drawn tti0; the downlink subframes with PHICH groups carry drawn distinct PHICHs
    encoded by the reference, through dl_ctrl_ref.channel -> (cell, tti0, [dict(tti, ul, y, ce, noise, phichs)])."""
    from dl_ctrl_ref import channel
    cell = TddCell(*spec)
    rng = np.random.default_rng(seed)
    tti0 = int(rng.integers(0, 10240))
    subs = []
    for b in range(10 * nof_frames):
        tti = tti0 + b
        sf_idx = tti % 10
        if is_ul(spec[7], sf_idx):
            y = [np.zeros(cell.glen, np.complex64) for _ in range(cell.nof_rx)]
            subs.append(dict(tti=tti, ul=True, y=y, ce=np.ones((cell.ports, cell.nof_rx, cell.glen), np.complex64), noise=1.0, phichs=[]))
            continue
        phichs = draw_tdd_phichs(cell, sf_idx, rng)
        tx = cell.encode_full(tti, 1 + b % max_cfi(sf_idx), [], phichs)
        y, ce, noise = channel(cell, tx, PHICH_SNRS[b % 2], rng)
        subs.append(dict(tti=tti, ul=False, y=y, ce=ce, noise=noise, phichs=phichs))
    return cell, tti0, subs
