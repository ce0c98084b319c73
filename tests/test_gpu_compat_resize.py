"""The single-call API's resize paths (include/srslte_hip/srslte_compat.h): objects built once for the widest cell and resized to the one
the UE learns, as srsue's cc_worker.cc:74,79 and ue_dl.c:191-210 / ue_ul.c:146 / enb_dl.c:160-166 / enb_ul.c:120 use them. Every object is
checked ON ITS OWN after the resize against an independent reference at the target size - the oracle for OFDM and DFT, the reference's compiled
code (oracle/_ref/libsrslte_ref.so) for the estimator and the small helpers - because a round trip through two resized objects can hide a stale
setting: a stale +0.5 shift on the UE's transmitter cancels the matching stale -0.5 on the eNB's receiver."""
import ctypes as C

import numpy as np
import pytest

from _libs import OrcCell, OrcOfdm, RefCell, RefChestCfg, RefChestRes, RefDlSfCfg, acopy, aligned, hip, opaque, oracle, p, ref
from test_gpu_compat import DftPlan, close

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(ref() is None, reason="oracle/_ref/libsrslte_ref.so not built")]
NORM, EXT = 0, 1
FWD, BWD = 0, 1


class Ofdm(C.Structure):
    """srslte_ofdm_t (ofdm.h:42-82), as include/srslte_hip/srslte_compat.h declares it"""
    _fields_ = [("fft_plan", DftPlan), ("fft_plan_sf", DftPlan * 2), ("max_prb", C.c_uint32), ("nof_symbols", C.c_uint32), ("symbol_sz", C.c_uint32),
                ("nof_guards", C.c_uint32), ("nof_re", C.c_uint32), ("slot_sz", C.c_uint32), ("sf_sz", C.c_uint32), ("cp", C.c_int), ("tmp", C.c_void_p),
                ("in_buffer", C.c_void_p), ("out_buffer", C.c_void_p), ("mbsfn_subframe", C.c_bool), ("mbsfn_guard_len", C.c_uint32),
                ("nof_symbols_mbsfn", C.c_uint32), ("non_mbsfn_region", C.c_uint8), ("freq_shift", C.c_bool), ("freq_shift_f", C.c_float),
                ("shift_buffer", C.c_void_p)]


class RefSignal(C.Structure):
    """srslte_refsignal_t (refsignal_dl.h:49-54)"""
    _fields_ = [("cell", RefCell), ("pilots", (C.c_void_p * 10) * 2), ("type", C.c_int), ("mbsfn_area_id", C.c_uint16)]


def libs():
    H, R = hip(), ref()
    for L in (H, R):
        L.srslte_use_standard_symbol_size.argtypes = [C.c_bool]
        for fn in ("srslte_cbsegm_cbsize_isvalid", "srslte_dft_precoding_valid_prb"):
            getattr(L, fn).restype = C.c_bool
    H.srslte_ofdm_set_freq_shift.argtypes = [C.c_void_p, C.c_float]
    H.srslte_ofdm_set_normalize.argtypes = [C.c_void_p, C.c_bool]
    H.srslte_ofdm_set_non_mbsfn_region.argtypes = [C.c_void_p, C.c_uint8]
    return H, R


def cplx(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def arr(ptr, n):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_float)), (2 * n,)).view(np.complex64)


# ---------------------------------------------------------------------------------------------------------------- OFDM
SENT = np.complex64(3 + 4j)
MAXN = 2048  # the largest symbol size of either family (110 PRB at the standard rates)


class OfdmUnderTest:
    """one srslte_ofdm_t built at 110 PRB on caller buffers sized for the largest cell, plus what the caller set on it"""

    def __init__(self, H, rx, mbsfn=False, cp=NORM, symbol_sz=None, prb=110):
        """symbol_sz: built by srslte_ofdm_init_mbsfn_ with the caller's symbol size instead of the rx / tx init functions"""
        self.H, self.rx, self.mbsfn = H, rx, mbsfn
        self.time, self.grid = aligned(2 * 15 * MAXN, np.float32).view(np.complex64), aligned(2 * 14 * 12 * 110, np.float32).view(np.complex64)
        self.inb, self.outb = (self.time, self.grid) if rx else (self.grid, self.time)
        self.q = Ofdm()
        if symbol_sz:
            H.srslte_ofdm_init_mbsfn_.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
            assert H.srslte_ofdm_init_mbsfn_(C.byref(self.q), cp, p(self.inb), p(self.outb), symbol_sz, prb, FWD if rx else BWD, 1 if mbsfn else 0) == 0
        else:
            init = {(True, False): H.srslte_ofdm_rx_init, (False, False): H.srslte_ofdm_tx_init,
                    (True, True): H.srslte_ofdm_rx_init_mbsfn, (False, True): H.srslte_ofdm_tx_init_mbsfn}[(rx, mbsfn)]
            assert init(C.byref(self.q), cp, p(self.inb), p(self.outb), prb) == 0
        self.shift, self.norm, self.region = None, False, 2 if mbsfn else 0

    def set_prb(self, cp, prb):
        return (self.H.srslte_ofdm_rx_set_prb if self.rx else self.H.srslte_ofdm_tx_set_prb)(C.byref(self.q), cp, prb)

    def set_shift(self, f):
        assert self.H.srslte_ofdm_set_freq_shift(C.byref(self.q), f) == 0
        self.shift = f

    def set_norm(self, v):
        self.H.srslte_ofdm_set_normalize(C.byref(self.q), v)
        self.norm = v

    def set_region(self, r):
        self.H.srslte_ofdm_set_non_mbsfn_region(C.byref(self.q), r)
        self.region = r

    def oracle_at(self, prb, N, cp):
        o = OrcOfdm()
        assert oracle().orc_ofdm_init_sz(C.byref(o), prb, N, cp == NORM) == 0
        o.normalize = self.norm
        o.freq_shift = self.shift is not None
        o.freq_shift_f = self.shift or 0.0
        o.non_mbsfn_region = self.region if self.mbsfn else 0
        return o

    def check_fields(self, R, prb, cp):
        """what srslte_ofdm_replan_ (ofdm.c:138-212) leaves in the struct, and what the caller set before"""
        q, N = self.q, R.srslte_symbol_sz(prb)
        nsymb = 7 if cp == NORM else 6
        assert (q.symbol_sz, q.nof_re, q.nof_guards, q.slot_sz, q.sf_sz, q.cp, q.nof_symbols) == (N, 12 * prb, (N - 12 * prb) // 2, N * 15 // 2, 15 * N, cp, nsymb)
        assert q.max_prb == 110 and q.fft_plan.norm == self.norm and q.mbsfn_subframe == self.mbsfn
        assert q.freq_shift == (self.shift is not None) and q.fft_plan.dc == (self.shift is None)
        if self.shift is not None:
            assert q.freq_shift_f == np.float32(self.shift)
        if self.mbsfn:
            assert q.non_mbsfn_region == self.region
        return N

    def check_run(self, rng, prb, N, cp):
        """srslte_ofdm_rx_sf / _rx_sf_ng / _tx_sf on this object against the oracle object at that size"""
        o = self.oracle_at(prb, N, cp)
        nre = 2 * (7 if cp == NORM else 6) * 12 * prb
        sf = 15 * N
        if self.rx:
            t = cplx(rng, sf)
            self.time[:sf] = t
            self.H.srslte_ofdm_rx_sf(C.byref(self.q))
            ref_g = np.zeros(nre, np.complex64)
            oracle().orc_ofdm_rx_sf(C.byref(o), p(t), p(ref_g))
            assert close(self.grid[:nre], ref_g), (prb, N, cp)
            if not self.mbsfn:  # the MBSFN branch of _rx_sf_ng works on the bound buffers (ofdm.c:469-483)
                t2, g2, ref2 = cplx(rng, sf), np.zeros(nre, np.complex64), np.zeros(nre, np.complex64)
                self.H.srslte_ofdm_rx_sf_ng(C.byref(self.q), p(t2), p(g2))
                oracle().orc_ofdm_rx_sf(C.byref(o), p(t2), p(ref2))
                assert close(g2, ref2), (prb, N, cp, "ng")
        else:
            g = cplx(rng, nre)
            self.grid[:nre] = g
            self.time[:] = SENT
            self.H.srslte_ofdm_tx_sf(C.byref(self.q))
            ref_t = np.full(sf, SENT, np.complex64)
            oracle().orc_ofdm_tx_sf(C.byref(o), p(g), p(ref_t))
            if self.mbsfn:  # the guard between the regions stays as the caller left it (ofdm.c:570-572)
                gap = ref_t == SENT
                assert gap.sum() > 0 and np.all(self.time[:sf][gap] == SENT)
            assert close(self.time[:sf], ref_t), (prb, N, cp)
            assert np.all(self.time[sf:] == SENT)

    def resize_and_check(self, R, rng, prb, cp):
        self.inb[:] = SENT
        assert self.set_prb(cp, prb) == 0
        N = self.check_fields(R, prb, cp)
        zeroed = 15 * N if self.rx else 2 * (7 if cp == NORM else 6) * 12 * prb  # ofdm.c:174-178
        assert np.all(self.inb[:zeroed] == 0) and np.all(self.inb[zeroed:] == SENT), (prb, cp)
        self.check_run(rng, prb, N, cp)
        return N

    def free(self):
        (self.H.srslte_ofdm_rx_free if self.rx else self.H.srslte_ofdm_tx_free)(C.byref(self.q))


WALK = [(6, NORM), (15, EXT), (25, NORM), (50, EXT), (75, NORM), (100, EXT), (110, NORM), (25, EXT)]


@pytest.mark.parametrize("std", [False, True])
@pytest.mark.parametrize("rx,shift", [(True, None), (True, -0.5), (False, None), (False, 0.5)])
def test_ofdm_set_prb_walk(rx, shift, std):
    """srslte_ofdm_rx_set_prb / _tx_set_prb from 110 PRB down to 6, up to 110 and back to 25, switching CP, in both rate families. The
    frequency shift (enb_ul.c:62-63 sets -0.5 on its receiver, ue_ul.c:63-64 +0.5 on its transmitter) and the normalisation are set before
    the first resize, as those callers do, and the shift changes once between two resizes. After each resize the struct holds the new
    geometry, the caller's input buffer is zeroed over the span upstream zeroes, and the object computes what a fresh oracle object at that
    size computes. A resize above max_prb is refused and leaves the object working at its last size."""
    H, R = libs()
    rng = np.random.default_rng(7 + 2 * rx + std + (0 if shift is None else 4))
    try:
        for L in (H, R):
            L.srslte_use_standard_symbol_size(std)
        u = OfdmUnderTest(H, rx)
        if shift is not None:
            u.set_shift(shift)
        u.set_norm(True)
        for step, (prb, cp) in enumerate(WALK):
            if step == 4 and shift is not None:
                u.set_shift(shift / 2)
            N = u.resize_and_check(R, rng, prb, cp)
        assert u.set_prb(NORM, 111) == -1
        u.check_fields(R, WALK[-1][0], WALK[-1][1])
        u.check_run(rng, WALK[-1][0], N, WALK[-1][1])
        u.free()
    finally:
        for L in (H, R):
            L.srslte_use_standard_symbol_size(False)


@pytest.mark.parametrize("rx", [True, False])
def test_ofdm_mbsfn_set_prb_keeps_region(rx):
    """MBSFN objects built at 110 PRB (srslte_ofdm_rx_init_mbsfn / _tx_init_mbsfn) and resized with SRSLTE_CP_EXT as ue_dl.c:205 and
    enb_dl.c:166 do: a non_mbsfn_region of 1 set before the resize survives it (upstream's replan never touches it), and the object's
    subframes follow the oracle's MBSFN layout for that region; then region 2 for one more resize."""
    H, R = libs()
    rng = np.random.default_rng(30 + rx)
    u = OfdmUnderTest(H, rx, mbsfn=True, cp=EXT)
    u.set_norm(True)
    u.set_region(1)
    for step, prb in enumerate((6, 25, 100, 50, 15)):
        if step == 3:
            u.set_region(2)
        u.resize_and_check(R, rng, prb, EXT)
    u.free()


@pytest.mark.parametrize("prb,N", [(6, 128), (25, 384), (25, 512), (100, 1536), (100, 2048)])
def test_ofdm_init_mbsfn_explicit_symbol_size(prb, N):
    """srslte_ofdm_init_mbsfn_ with the caller's symbol size, from either rate family, in both directions: the default region 2
    (ofdm.c:123-130) and the oracle's MBSFN layout at that size."""
    H, R = libs()
    rng = np.random.default_rng(prb + N)
    for rx in (True, False):
        u = OfdmUnderTest(H, rx, mbsfn=True, cp=EXT, symbol_sz=N, prb=prb)
        assert u.q.mbsfn_subframe and u.q.non_mbsfn_region == 2 and u.q.symbol_sz == N and u.q.nof_re == 12 * prb and u.q.cp == EXT
        u.set_norm(True)
        u.check_run(rng, prb, N, EXT)
        u.free()


# ---------------------------------------------------------------------------------------------------------------- DFT
def model_run_c(x, N, forward, mirror, dc, norm, out_before):
    """srslte_dft_run_c (dft_fftw.c:249-305): copy_pre, the transform, 1/sqrt(N), copy_post; the exact DFT in double precision"""
    off = 1 if dc else 0
    pin = x.copy()
    if mirror and not forward:
        hlen = N // 2
        pin[:off] = 0
        pin[off:N - hlen] = x[hlen:hlen + N - hlen - off]
        pin[N - hlen:] = x[:hlen]
    y = np.zeros(N, np.complex64)
    oracle().orc_dft_exact(p(np.ascontiguousarray(pin, np.complex64)), p(y), N, 1 if forward else 0)
    if norm:
        y = y / np.sqrt(N)
    out = out_before.copy()
    if mirror and forward:
        hlen = (N + 1) // 2
        out[:N - hlen] = y[hlen:]
        out[N - hlen:N - off] = y[off:hlen]
    else:
        out[:] = y
    return out


# (init size, direction, mirror, dc, norm, sizes walked): prach.c:349-384 plans 839-point Zadoff-Chu transforms and the long PRACH (I)FFTs
# at their largest and replans them to 139 and N_ifft_prach (:453-488; 4608 = 384 * 12 and 9216 = 768 * 12); ofdm.c plans mirrored,
# DC-skipping transforms
DFT_CASES = [(839, FWD, False, False, True, [139, 839]), (839, BWD, False, False, False, [139, 839]),
             (24576, BWD, True, False, True, [4608, 9216]), (24576, FWD, True, False, False, [9216, 4608]),
             (1536, FWD, True, True, True, [384, 128, 1536]), (1536, BWD, True, True, False, [768, 1536])]


@pytest.mark.parametrize("init,dir_,mirror,dc,norm,sizes", DFT_CASES)
def test_dft_replan_c(init, dir_, mirror, dc, norm, sizes):
    """srslte_dft_replan_c / srslte_dft_replan on a complex plan whose mirror / dc / norm flags are set: the plan keeps its flags and its
    init_size, transforms at the new size as the reference's run_c does there, and srslte_dft_run_c_zerocopy (dft_fftw.c:277-279) gives the
    bare transform. srslte_dft_replan past init_size is refused (dft_fftw.c:66-78)."""
    H, _ = libs()
    rng = np.random.default_rng(init + len(sizes) + dir_)
    pl = DftPlan()
    assert H.srslte_dft_plan_c(C.byref(pl), init, dir_) == 0
    H.srslte_dft_plan_set_mirror(C.byref(pl), mirror)
    H.srslte_dft_plan_set_dc(C.byref(pl), dc)
    H.srslte_dft_plan_set_norm(C.byref(pl), norm)
    for i, n in enumerate(sizes):
        assert (H.srslte_dft_replan if i % 2 else H.srslte_dft_replan_c)(C.byref(pl), n) == 0
        assert (pl.size, pl.init_size, pl.mirror, pl.dc, pl.norm, pl.forward, pl.mode) == (n, init, mirror, dc, norm, dir_ == FWD, 0)
        x, y = cplx(rng, n), np.full(n, -7.0, np.complex64)
        H.srslte_dft_run_c(C.byref(pl), p(x), p(y))
        assert close(y, model_run_c(x, n, dir_ == FWD, mirror, dc, norm, np.full(n, -7.0, np.complex64))), n
        z, ref_z = np.zeros(n, np.complex64), np.zeros(n, np.complex64)
        H.srslte_dft_run_c_zerocopy(C.byref(pl), p(x), p(z))
        oracle().orc_dft_exact(p(x), p(ref_z), n, 1 if dir_ == FWD else 0)
        assert close(z, ref_z), n
    assert H.srslte_dft_replan(C.byref(pl), init + 1) == -1 and pl.size == sizes[-1]
    H.srslte_dft_plan_free(C.byref(pl))


@pytest.mark.parametrize("init,dir_,sizes", [(1536, FWD, [300, 128, 1536]), (1536, BWD, [1000, 1536]), (839, FWD, [139])])
def test_dft_replan_r(init, dir_, sizes):
    """srslte_dft_replan_r / srslte_dft_replan on a real (FFTW half-complex) plan with norm set: the new size's R2HC / HC2R with 1/N."""
    H, _ = libs()
    rng = np.random.default_rng(init + dir_)
    pl = DftPlan()
    assert H.srslte_dft_plan_r(C.byref(pl), init, dir_) == 0
    H.srslte_dft_plan_set_norm(C.byref(pl), True)
    for i, n in enumerate(sizes):
        assert (H.srslte_dft_replan if i % 2 else H.srslte_dft_replan_r)(C.byref(pl), n) == 0
        assert (pl.size, pl.init_size, pl.norm, pl.mode) == (n, init, True, 1)
        x, y, r = rng.standard_normal(n).astype(np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
        H.srslte_dft_run_r(C.byref(pl), p(x), p(y))
        oracle().orc_dft_r2hc(p(x), p(r), n, 1 if dir_ == FWD else 0)
        assert close(y, r / n), n
    assert H.srslte_dft_replan(C.byref(pl), init + 1) == -1 and pl.size == sizes[-1]
    H.srslte_dft_plan_free(C.byref(pl))


@pytest.mark.parametrize("dir_", [FWD, BWD])
def test_dft_replan_guru_keeps_flags(dir_):
    """srslte_dft_replan_guru_c (dft_fftw.c:93-118) from a contiguous batch to a strided one: the plan keeps its direction and the norm /
    dc / mirror flags its owner set, takes the new size as init_size, and runs the new layout (a guru plan executes the bare transform)."""
    H, _ = libs()
    rng = np.random.default_rng(50 + dir_)
    N, M, N2, M2, ist, ost, idist, odist = 128, 7, 64, 5, 5, 1, 1, 64
    x0, y0 = aligned(N * M, np.complex64), aligned(N * M, np.complex64)
    pl = DftPlan()
    assert H.srslte_dft_plan_guru_c(C.byref(pl), N, dir_, p(x0), p(y0), 1, 1, M, N, N) == 0
    H.srslte_dft_plan_set_norm(C.byref(pl), True)
    H.srslte_dft_plan_set_dc(C.byref(pl), True)
    H.srslte_dft_plan_set_mirror(C.byref(pl), True)
    nin, nout = (M2 - 1) * idist + (N2 - 1) * ist + 1, (M2 - 1) * odist + (N2 - 1) * ost + 1
    x, y = aligned(nin, np.complex64), aligned(nout, np.complex64)
    x[:], y[:] = cplx(rng, nin), -7.0
    assert H.srslte_dft_replan_guru_c(C.byref(pl), N2, p(x), p(y), ist, ost, M2, idist, odist) == 0
    assert (pl.size, pl.init_size, pl.is_guru, pl.forward, pl.dir, pl.norm, pl.dc, pl.mirror) == (N2, N2, True, dir_ == FWD, dir_, True, True, True)
    H.srslte_dft_run_guru_c(C.byref(pl))
    for i in range(M2):
        xi, r = np.ascontiguousarray(x[i * idist:i * idist + (N2 - 1) * ist + 1:ist]), np.zeros(N2, np.complex64)
        oracle().orc_dft_exact(p(xi), p(r), N2, 1 if dir_ == FWD else 0)
        assert close(y[i * odist:i * odist + (N2 - 1) * ost + 1:ost], r), i
    H.srslte_dft_plan_free(C.byref(pl))


# ---------------------------------------------------------------------------------------------------------------- estimator
# (id, nof_prb, ports, cp): every step changes the id (upstream re-plans on an id change only, chest_dl.c:262-300), the width, and
# ports / CP along the way
CHEST_WALK = [(17, 25, 1, NORM), (302, 100, 2, NORM), (5, 6, 4, NORM), (211, 50, 2, EXT), (88, 15, 1, EXT), (499, 75, 4, NORM), (3, 100, 1, NORM)]


def chest_grids(rng, cid, prb, npt, cp, nrx, sf_idx):
    """a subframe of the cell: the CRS of every port through a smooth per-(port, antenna) channel, data on the other REs, noise"""
    nsymb = 14 if cp == NORM else 12
    n, nre = nsymb * 12 * prb, 12 * prb
    cell = OrcCell(cid, prb, npt, cp == NORM)
    tx = []
    for port in range(npt):
        g = np.zeros(n, np.complex64)
        oracle().orc_crs_put_sf(C.byref(cell), sf_idx, port, p(g))
        tx.append(g)
    hole = np.zeros(n, bool)
    for g in tx:
        hole |= g != 0
    data = (cplx(rng, n) * 0.7).astype(np.complex64)
    k, l = np.arange(n) % nre, np.arange(n) // nre
    grids = []
    for a in range(nrx):
        g = np.where(hole, 0, data).astype(np.complex64) * (1.3 - 0.3 * a)
        for port in range(npt):
            g = g + tx[port] * ((2.0 - 0.3 * port + 0.2 * a) * (1 + 0.25 * np.sin(k / 33.0 + port + a)) * np.exp(1j * (0.5 * port - 0.7 * a + k / 90.0 + 0.04 * l)))
        g = g + (0.04 + 0.05 * a) * cplx(rng, n)
        grids.append(acopy(g.astype(np.complex64).view(np.float32)))
    return grids, n


def ref_estimate(R, cell, nrx, sf_idx, grids, n):
    """a fresh reference srslte_chest_dl_t created at the cell"""
    q = opaque(1 << 20)
    assert R.srslte_chest_dl_init(q, cell.nof_prb, nrx) == 0 and R.srslte_chest_dl_set_cell(q, cell) == 0
    res, sf, rc = RefChestRes(), RefDlSfCfg(), chest_cfg()
    ces = [aligned(2 * n, np.float32) for _ in range(cell.nof_ports * nrx)]
    for i, c_ in enumerate(ces):
        res.ce[i // nrx][i % nrx] = c_.ctypes.data
    sf.tti = sf_idx
    inp = (C.c_void_p * 4)(*([g.ctypes.data for g in grids] + [0] * (4 - nrx)))
    assert R.srslte_chest_dl_estimate_cfg(q, C.byref(sf), C.byref(rc), inp, C.byref(res)) == 0
    R.srslte_chest_dl_free(q)
    return res, [c_.view(np.complex64) for c_ in ces]


def chest_cfg():
    rc = RefChestCfg()
    rc.filter_coef[0], rc.filter_coef[1] = 4.0, 1.0
    return rc


def check_against_ref(H, R, est, res, cell, nrx, rng, tag):
    for sf_idx in (1, 5):
        grids, n = chest_grids(rng, cell.id, cell.nof_prb, cell.nof_ports, cell.cp, nrx, sf_idx)
        sf = RefDlSfCfg()
        sf.tti = 10 + sf_idx
        inp = (C.c_void_p * 4)(*([g.ctypes.data for g in grids] + [0] * (4 - nrx)))
        assert H.srslte_chest_dl_estimate_cfg(est, C.byref(sf), C.byref(chest_cfg()), inp, C.byref(res)) == 0
        rres, rce = ref_estimate(R, cell, nrx, sf_idx, grids, n)
        for i in range(cell.nof_ports * nrx):
            assert close(arr(res.ce[i // nrx][i % nrx], n), rce[i]), (tag, sf_idx, i)
        for nm in ("noise_estimate", "noise_estimate_dbm", "snr_db", "rsrp", "rsrp_dbm", "rsrq", "rsrq_db", "rssi_dbm"):
            x, y = getattr(res, nm), getattr(rres, nm)
            assert abs(x - y) <= 1e-4 * abs(y) + 1e-5, (tag, sf_idx, nm, x, y)


@pytest.mark.parametrize("nrx", [1, 2])
def test_chest_dl_set_cell_walk(nrx):
    """srslte_chest_dl_init(q, 110, nrx) and srslte_chest_dl_res_init(res, 110) once, then srslte_chest_dl_set_cell through cells that change
    id, width, ports and CP: at each, the estimates, noise, RSRP and RSRQ of subframes made at that cell equal those of a fresh reference
    estimator created at that cell."""
    H, R = libs()
    rng = np.random.default_rng(70 + nrx)
    est, res = opaque(1 << 16), RefChestRes()
    assert H.srslte_chest_dl_init(est, 110, nrx) == 0 and H.srslte_chest_dl_res_init(C.byref(res), 110) == 0
    for cid, prb, npt, cp in CHEST_WALK:
        cell = RefCell(prb, npt, cid, cp, 0, 0, 0)
        assert H.srslte_chest_dl_set_cell(est, cell) == 0
        assert np.frombuffer(est, np.uint32, 4)[:3].tolist() == [prb, npt, cid]
        check_against_ref(H, R, est, res, cell, nrx, rng, (cid, prb, npt, cp))
    # srslte_cell_isvalid (phy_common.c:38-60) stops at 100 PRB: a 110-PRB cell is refused as the reference refuses it, and the object
    # still estimates at its last cell
    big, rq = RefCell(110, 1, 9, NORM, 0, 0, 0), opaque(1 << 20)
    assert R.srslte_chest_dl_init(rq, 110, nrx) == 0
    assert H.srslte_chest_dl_set_cell(est, big) == R.srslte_chest_dl_set_cell(rq, big) == -2
    R.srslte_chest_dl_free(rq)
    check_against_ref(H, R, est, res, cell, nrx, rng, "after the refused cell")
    H.srslte_chest_dl_res_free(C.byref(res))
    H.srslte_chest_dl_free(est)


def test_chest_dl_set_cell_same_id_new_width_replans():
    """A deliberate divergence from upstream. srslte_chest_dl_set_cell upstream (chest_dl.c:262-300) re-plans on a change of cell id only:
    given the same id with another bandwidth it keeps the old cell, and its interpolators and CRS stay at the old width. Every upstream caller
    changes the id with the bandwidth, so that rule never bites there, but an estimator left at the wrong width would read the wrong grid.
    This library re-plans when the id OR the bandwidth changes, and then estimates correctly at the new size - pinned here against a
    fresh reference estimator at the new cell, next to the reference object walked the same way, which keeps the old width."""
    H, R = libs()
    rng = np.random.default_rng(77)
    est, res, rq = opaque(1 << 16), RefChestRes(), opaque(1 << 20)
    assert H.srslte_chest_dl_init(est, 110, 1) == 0 and H.srslte_chest_dl_res_init(C.byref(res), 110) == 0
    assert R.srslte_chest_dl_init(rq, 110, 1) == 0
    for prb in (50, 25):
        cell = RefCell(prb, 2, 123, NORM, 0, 0, 0)
        assert H.srslte_chest_dl_set_cell(est, cell) == 0 and R.srslte_chest_dl_set_cell(rq, cell) == 0
        assert np.frombuffer(est, np.uint32, 1)[0] == prb
        check_against_ref(H, R, est, res, cell, 1, rng, prb)
    assert np.frombuffer(rq, np.uint32, 1)[0] == 50  # upstream kept the first width
    R.srslte_chest_dl_free(rq)
    H.srslte_chest_dl_res_free(C.byref(res))
    H.srslte_chest_dl_free(est)


def test_chest_dl_res_set_identity_and_ones():
    """srslte_chest_dl_res_set_identity / _set_ones (chest_dl.c:212-231) on a result sized for 110 PRB: every [i][j] buffer over nof_re,
    equal to the reference's functions on the reference's result of the same size."""
    H, R = libs()
    rng = np.random.default_rng(80)
    mine, theirs = RefChestRes(), RefChestRes()
    assert H.srslte_chest_dl_res_init(C.byref(mine), 110) == 0 and R.srslte_chest_dl_res_init(C.byref(theirs), 110) == 0
    assert mine.nof_re == theirs.nof_re == 14 * 12 * 110
    n = mine.nof_re
    for fn in ("srslte_chest_dl_res_set_identity", "srslte_chest_dl_res_set_ones"):
        for r_ in (mine, theirs):
            for i in range(4):
                for j in range(4):
                    arr(r_.ce[i][j], n)[:] = cplx(rng, n)
        getattr(H, fn)(C.byref(mine))
        getattr(R, fn)(C.byref(theirs))
        for i in range(4):
            for j in range(4):
                assert np.array_equal(arr(mine.ce[i][j], n), arr(theirs.ce[i][j], n)), (fn, i, j)
        assert np.all(arr(mine.ce[0][0], n) == 1) and (fn.endswith("ones") or np.all(arr(mine.ce[0][1], n) == 0))
    H.srslte_chest_dl_res_free(C.byref(mine))
    R.srslte_chest_dl_res_free(C.byref(theirs))


# ---------------------------------------------------------------------------------------------------------------- small entry points
def test_host_helpers_match_reference():
    """srslte_cbsegm_cbsize_isvalid over 0..6200, srslte_dft_precoding_valid_prb over 0..110 (upstream's table: 0 is accepted, nothing above
    100 is, dft_precoding.c:87-98 - srsenb's scheduler_metric.cc:222 counts down until it is true) and srslte_tdec_autoimp_get_subblocks /
    _8bit for all 188 block sizes, against the reference's functions."""
    H, R = libs()
    for n in range(6201):
        assert H.srslte_cbsegm_cbsize_isvalid(n) == R.srslte_cbsegm_cbsize_isvalid(n), n
    for n in range(111):
        assert H.srslte_dft_precoding_valid_prb(n) == R.srslte_dft_precoding_valid_prb(n), n
    R.srslte_cbsegm_cbsize.restype = C.c_int
    for i in range(188):
        K = R.srslte_cbsegm_cbsize(i)
        assert H.srslte_cbsegm_cbsize(i) == K
        assert H.srslte_tdec_autoimp_get_subblocks(K) == R.srslte_tdec_autoimp_get_subblocks(K), K
        assert H.srslte_tdec_autoimp_get_subblocks_8bit(K) == R.srslte_tdec_autoimp_get_subblocks_8bit(K), K


@pytest.mark.parametrize("qprb,prb,cid,area", [(110, 110, 1, 0), (110, 25, 77, 3), (50, 50, 400, 255), (6, 6, 0, 17), (100, 15, 250, 128)])
def test_refsignal_mbsfn_gen_seq(qprb, prb, cid, area):
    """srslte_refsignal_mbsfn_gen_seq (refsignal_dl.c:361-400) on a table from srslte_refsignal_mbsfn_init(q, 110) whose cell is set to
    qprb PRB: the table is indexed with q's own width and the sequence offset with the argument's, as upstream; every pilot of both groups
    and all ten subframes against the reference's."""
    H, R = libs()
    mine, theirs = RefSignal(), RefSignal()
    for L, q in ((H, mine), (R, theirs)):
        assert L.srslte_refsignal_mbsfn_init(C.byref(q), 110) == 0
        assert L.srslte_refsignal_mbsfn_set_cell(C.byref(q), RefCell(qprb, 1, cid, EXT, 0, 0, 0), C.c_uint16(area)) == 0
        assert L.srslte_refsignal_mbsfn_gen_seq(C.byref(q), RefCell(prb, 1, cid, EXT, 0, 0, 0), (area * 7 + 1) % 256) == 0
    for g in range(2):
        for sf in range(10):
            assert np.array_equal(arr(mine.pilots[g][sf], 18 * qprb), arr(theirs.pilots[g][sf], 18 * qprb)), (g, sf)
    H.srslte_refsignal_free(C.byref(mine))
    R.srslte_refsignal_free(C.byref(theirs))


@pytest.mark.parametrize("prb,tbs,mod,nre,snr", [(25, 4008, 2, 3000, 2.0), (6, 328, 1, 600, -5.5)])
def test_dlsch_decode_is_decode2_of_codeword_0(prb, tbs, mod, nre, snr):
    """srslte_dlsch_decode (sch.c:507-510) is srslte_dlsch_decode2(..., 0, 1): return code, bytes and soft buffer, byte for byte."""
    from lte_sim import OrcSchCfg
    from test_gpu_sch_host import Side, hip_seg
    H = hip()
    rng = np.random.default_rng(tbs)
    nbits = nre * 2 * mod
    data = rng.integers(0, 256, tbs // 8, dtype=np.uint8)
    K, C_ = hip_seg(tbs)
    bits = np.zeros(nbits, np.uint8)
    assert oracle().orc_dlsch_encode(C.byref(OrcSchCfg(tbs, nbits, 2 * mod, 0, 4)), p(data), p(bits)) == 0
    e = np.clip(np.round(100.0 * ((2.0 * bits - 1) + 10 ** (-snr / 20) * rng.standard_normal(nbits))), -32000, 32000).astype(np.int16)
    a, b = Side(True, prb, tbs, mod, nbits, False, 4), Side(True, prb, tbs, mod, nbits, False, 4)
    for s in (a, b):
        s.set(0, 1)
    out_a, out_b = np.zeros(tbs // 8 + 64, np.uint8), np.zeros(tbs // 8 + 64, np.uint8)
    H.srslte_dlsch_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    rc_a = H.srslte_dlsch_decode(a.q, a.cfg, p(e.copy()), p(out_a))
    rc_b = b.decode(e.copy(), out_b, 1)
    assert rc_a == rc_b and np.array_equal(out_a, out_b)
    n_soft = 3 * (K + 32) + 12
    sa, sb = a.soft(C_, n_soft), b.soft(C_, n_soft)
    assert np.array_equal(sa[0], sb[0]) and sa[3] == sb[3] and all(np.array_equal(x, y) for x, y in zip(sa[1], sb[1]))
    if rc_a == 0:
        assert np.array_equal(out_a[:tbs // 8], data)


@pytest.mark.parametrize("is_tx", [True, False])
def test_dft_precoding_init_at_max_prb(is_tx):
    """srslte_dft_precoding_init / _init_rx at max_prb 110, then runs at smaller valid widths against the oracle; widths upstream's
    srslte_dft_precoding_valid_prb refuses (7, 108) are refused."""
    H, _ = libs()
    rng = np.random.default_rng(90 + is_tx)
    q = opaque(1 << 16)
    assert (H.srslte_dft_precoding_init(q, 110, True) if is_tx else H.srslte_dft_precoding_init_rx(q, 110)) == 0
    for nprb in (3, 25, 48, 100):
        x = cplx(rng, 12 * 12 * nprb)
        y, r = np.zeros_like(x), np.zeros_like(x)
        assert H.srslte_dft_precoding(q, p(x), p(y), nprb, 12) == 0
        oracle().orc_dft_precoding(p(x), p(r), nprb, 12, 1 if is_tx else 0, True)
        assert close(y, r), nprb
    x = cplx(rng, 12 * 12 * 108)
    y = np.zeros_like(x)
    assert H.srslte_dft_precoding(q, p(x), p(y), 7, 12) == -1 and H.srslte_dft_precoding(q, p(x), p(y), 108, 12) == -1
    H.srslte_dft_precoding_free(q)
