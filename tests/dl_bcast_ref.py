"""Reference side of the DL broadcast tests (PSS / SSS / PBCH) and of scripts/bench_dl_tx_bcast.py: the reference's own srslte_pss_*,
srslte_sss_*, srslte_pbch_* and the decode_frame steps (srslte_rm_conv_rx, srslte_viterbi_decode_f, CRC-16) from oracle/_ref/libsrslte_ref.so
for one cell. Test infrastructure only."""
import ctypes as C

import numpy as np

from _libs import RefCell, RefChestRes, aligned, opaque, ref

RX_NULL = np.float32(10000.0)
VITERBI_37 = 2  # srslte_viterbi_type_t (viterbi.h:39-44)
CRC_MASK = {1: 0x0000, 2: 0xFFFF, 4: 0x5555}  # srslte_crc_mask (pbch.c:42-46) as the 16-bit parity word


def _R():
    R = ref()
    vp = C.c_void_p
    R.srslte_pbch_init.argtypes = [vp]
    R.srslte_pbch_set_cell.argtypes = [vp, RefCell]
    R.srslte_pbch_put.argtypes = [vp, vp, RefCell]
    R.srslte_pbch_get.argtypes = [vp, vp, RefCell]
    R.srslte_pbch_encode.argtypes = [vp, vp, vp, C.c_uint32]
    R.srslte_pbch_decode.argtypes = [vp, vp, vp, vp, vp, vp]
    R.srslte_pbch_decode_reset.argtypes = [vp]
    R.srslte_pbch_mib_pack.argtypes = [vp, C.c_uint32, vp]
    R.srslte_pss_generate.argtypes = [vp, C.c_uint32]
    R.srslte_pss_put_slot.argtypes = [vp, vp, C.c_uint32, C.c_int]
    R.srslte_sss_generate.argtypes = [vp, vp, C.c_uint32]
    R.srslte_sss_put_slot.argtypes = [vp, vp, C.c_uint32, C.c_int]
    R.srslte_sequence_pbch.argtypes = [vp, C.c_int, C.c_uint32]
    R.srslte_scrambling_f_offset.argtypes = [vp, vp, C.c_int, C.c_int]
    R.srslte_rm_conv_rx.argtypes = [vp, C.c_uint32, vp, C.c_uint32]
    R.srslte_viterbi_init.argtypes = [vp, C.c_int, vp, C.c_uint32, C.c_bool]
    R.srslte_viterbi_decode_f.argtypes = [vp, vp, vp, C.c_uint32]
    R.srslte_predecoding_diversity.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_float]
    R.srslte_layerdemap_diversity.argtypes = [vp, vp, C.c_int, C.c_int]
    R.srslte_demod_soft_demodulate.argtypes = [C.c_int, vp, vp, C.c_int]
    return R


class BcastCell:
    """The reference's PSS / SSS / PBCH of one cell. ports 0: srslte_pbch_set_cell's search over every port count (as srslte_ue_mib)."""

    def __init__(self, nof_prb, ports, cell_id, cp_ext=False, phich_res=0, phich_ext=False):
        self.R = R = _R()
        self.nof_prb, self.ports, self.cell_id, self.cp_ext = nof_prb, ports, cell_id, cp_ext
        self.cell = RefCell(nof_prb, ports, cell_id, 1 if cp_ext else 0, 1 if phich_ext else 0, phich_res, 0)
        self.glen = (12 if cp_ext else 14) * 12 * nof_prb
        self.slot = self.glen // 2
        self.nof_bits = 432 if cp_ext else 480
        self._pbch = None  # srslte_pbch_t, made on first use (srslte_cell_isvalid stops at 100 PRB; the RE and packing functions do not)
        self.seq = opaque(1 << 12)
        assert R.srslte_sequence_pbch(self.seq, 1 if cp_ext else 0, cell_id) == 0
        self.vit = opaque(1 << 16)
        poly = (C.c_int * 3)(0x6D, 0x4F, 0x57)
        assert R.srslte_viterbi_init(self.vit, VITERBI_37, poly, 40, True) == 0

    @property
    def pbch(self):
        if self._pbch is None:
            self._pbch = opaque(1 << 16)
            assert self.R.srslte_pbch_init(self._pbch) == 0 and self.R.srslte_pbch_set_cell(self._pbch, self.cell) == 0
        return self._pbch

    def mib_pack(self, sfn):
        out = np.zeros(24, np.uint8)
        self.R.srslte_pbch_mib_pack(C.byref(self.cell), sfn, out.ctypes.data)
        return out

    def pss(self):
        s = aligned(62, np.complex64)
        assert self.R.srslte_pss_generate(s.ctypes.data, self.cell_id % 3) == 0
        return s

    def sss(self):
        s0, s5 = aligned(62, np.float32), aligned(62, np.float32)
        self.R.srslte_sss_generate(s0.ctypes.data, s5.ctypes.data, self.cell_id)
        return s0, s5

    def put_sync(self, grid, sf_idx):
        """srslte_pss_put_slot + srslte_sss_put_slot on one port's subframe grid (put_sync of enb_dl.c:297-307)."""
        pss, (s0, s5) = self.pss(), self.sss()
        cp = 1 if self.cp_ext else 0
        self.R.srslte_pss_put_slot(pss.ctypes.data, grid.ctypes.data, self.nof_prb, cp)
        self.R.srslte_sss_put_slot((s5 if sf_idx else s0).ctypes.data, grid.ctypes.data, self.nof_prb, cp)

    def pbch_put_re(self):
        """Where srslte_pbch_put puts symbol i: distinct values into a zero slot, read back."""
        n = self.nof_bits // 2
        sym = aligned(n, np.complex64)
        sym[:] = np.arange(1, n + 1)
        grid = aligned(self.glen, np.complex64)
        assert self.R.srslte_pbch_put(sym.ctypes.data, grid[self.slot:].ctypes.data, self.cell) == n
        nz = np.flatnonzero(grid)
        assert nz.size == n
        return nz[np.argsort(grid[nz].real)].astype(np.uint32)

    def pbch_get_re(self):
        """What srslte_pbch_get reads: a grid holding its own indices."""
        n = self.nof_bits // 2
        grid = aligned(self.glen, np.complex64)
        grid[:] = np.arange(self.glen)
        out = aligned(n, np.complex64)
        assert self.R.srslte_pbch_get(grid[self.slot:].ctypes.data, out.ctypes.data, self.cell) == n
        return out.real.astype(np.uint32)

    def put_base(self, tti, grids):
        """put_sync + put_mib of srslte_enb_dl_put_base (enb_dl.c:297-335) on grids [ports][glen] (in place)."""
        sf_idx, sfn = tti % 10, (tti // 10) % 1024
        if sf_idx in (0, 5):
            for p in range(self.ports):
                self.put_sync(grids[p], sf_idx)
        if sf_idx == 0:
            g = [aligned(self.glen, np.complex64) for _ in range(4)]
            for p in range(self.ports):
                g[p][:] = grids[p]
            ptrs = (C.c_void_p * 4)(*[x.ctypes.data for x in g])
            pay = self.mib_pack(sfn)
            assert self.R.srslte_pbch_encode(self.pbch, pay.ctypes.data, ptrs, sfn % 4) == 0
            for p in range(self.ports):
                grids[p][:] = g[p]
        return grids

    def encode(self, tti):
        """put_base's sync and MIB on zero grids -> [ports][glen]."""
        return self.put_base(tti, np.zeros((self.ports, self.glen), np.complex64))

    def decode(self, y, ce, noise):
        """srslte_pbch_decode_reset + srslte_pbch_decode on the antenna-0 grid y [glen] with estimates ce [nof ce ports][glen] ->
        (ret, nof_tx_ports, sfn_offset, payload [24])."""
        ya = aligned(self.glen, np.complex64)
        ya[:] = y
        res = RefChestRes()
        keep = []
        for p in range(ce.shape[0]):
            a = aligned(self.glen, np.complex64)
            a[:] = ce[p]
            keep.append(a)
            res.ce[p][0] = a.ctypes.data
        res.noise_estimate = float(noise)
        ptrs = (C.c_void_p * 4)(ya.ctypes.data, None, None, None)
        pay = np.zeros(24, np.uint8)
        nports, off = C.c_uint32(0), C.c_int(0)
        self.R.srslte_pbch_decode_reset(self.pbch)
        ret = self.R.srslte_pbch_decode(self.pbch, C.byref(res), ptrs, pay.ctypes.data, C.byref(nports), C.byref(off))
        return ret, nports.value, off.value, pay

    def llr(self, y, ce, noise, nant):
        """The LLR row srslte_pbch_decode demodulates for nant ports (pbch.c:477-516) from the antenna-0 grid y and estimates ce."""
        R, n = self.R, self.nof_bits // 2
        ya = aligned(self.glen, np.complex64)
        ya[:] = y
        sym = aligned(n, np.complex64)
        assert R.srslte_pbch_get(ya[self.slot:].ctypes.data, sym.ctypes.data, self.cell) == n
        hs = []
        for p in range(4):
            a, h = aligned(self.glen, np.complex64), aligned(n, np.complex64)
            a[:] = ce[min(p, ce.shape[0] - 1)]
            assert R.srslte_pbch_get(a[self.slot:].ctypes.data, h.ctypes.data, self.cell) == n
            hs.append(h)
        d = aligned(n, np.complex64)
        if nant == 1:
            R.srslte_predecoding_single(sym.ctypes.data, hs[0].ctypes.data, d.ctypes.data, None, n, 1.0, float(noise))
        else:
            x = [aligned(n, np.complex64) for _ in range(4)]
            xp = (C.c_void_p * 4)(*[v.ctypes.data for v in x])
            R.srslte_predecoding_diversity(sym.ctypes.data, (C.c_void_p * 4)(*[h.ctypes.data for h in hs]), xp, nant, n, 1.0)
            R.srslte_layerdemap_diversity(xp, d.ctypes.data, nant, n // nant)
        llr = aligned(2 * n, np.float32)
        R.srslte_demod_soft_demodulate(1, d.ctypes.data, llr.ctypes.data, n)
        return llr

    def decode_frame(self, llr, dst, nant):
        """decode_frame(src 0, dst, n 1) (pbch.c:393-431) on an LLR row of nof_bits -> (crc check passed, the 40 decoded bits)."""
        nb = self.nof_bits
        temp = aligned(4 * nb, np.float32)
        temp[:] = RX_NULL
        temp[dst * nb:(dst + 1) * nb] = llr[:nb]
        self.R.srslte_scrambling_f_offset(self.seq, temp[dst * nb:].ctypes.data, dst * nb, nb)
        rm = aligned(120, np.float32)
        assert self.R.srslte_rm_conv_rx(temp.ctypes.data, 4 * nb, rm.ctypes.data, 120) == 0
        rm *= np.float32(0.5)
        data = np.zeros(40, np.uint8)
        self.R.srslte_viterbi_decode_f(self.vit, rm.ctypes.data, data.ctypes.data, 40)
        return crc_check(data, nant), data


def crc16(bits):
    r = 0
    for i in range(len(bits) + 16):
        r = (r << 1) | (int(bits[i]) if i < len(bits) else 0)
        if r & 0x10000:
            r ^= 0x11021
    return r & 0xFFFF


def crc_check(data, nant):
    """srslte_pbch_crc_check: the CRC with the nant mask, and a payload that is not all zeros."""
    parity = int("".join(str(int(b)) for b in data[24:40]), 2) ^ CRC_MASK[nant]
    return parity == crc16(data[:24]) and bool(np.any(data[:24]))
