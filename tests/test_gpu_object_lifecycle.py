"""The control and auxiliary objects' memory and descriptor staging (csrc/dev_buf.hpp), at the smallest shapes: 6 PRB, normal CP, one
subframe, one or two entries per call.

Staging ring wrap. Six calls with different descriptors and their own output buffers, queued on one stream with no host synchronisation in
between, then the same six with a synchronisation after each: the outputs are byte-identical. Six is more than the four pinned buffers of a
ring, so descriptors overwritten while a copy still reads them show as a difference. The control-region encoder and the channel emulator
have this test already (test_gpu_dl_ctrl_tx.py::test_calls_in_flight, test_gpu_channel.py::test_nine_calls_queued_on_one_stream_...).

Create / use / destroy, three times in a row per object kind, each use compared with the module's reference at the bound of the module's
own GPU test; then the configurations every create refuses."""
import ctypes as C
import importlib

import numpy as np
import pytest

import channel_ref
import prach_ref
from _libs import aligned, ref
from gen_golden_srs import CASES as SRS_CASES
from srs_ref import case_cfg, case_ue, golden as srs_golden, rx_model

pkg = importlib.import_module("srslte-emane_amd")
pytestmark = pytest.mark.gpu
need_ref = pytest.mark.skipif(ref() is None, reason="oracle/_ref/libsrslte_ref.so is not built")

NCALLS = 6
# (nof_prb, ports, cell_id, cp_ext, phich_res, phich_ext, nof_rx): Ng = 2 gives a 6 PRB cell two PHICH groups
DL = (6, 1, 1, False, 3, False, 1)
# (nof_prb, cell_id) and the PUCCH configuration of tests/test_gpu_ul_ctrl.py's first cell
UL = dict(cp_ext=False, group_hopping_en=False, delta_pucch_shift=1, N_cs=0, n_rb_2=1, N_pucch_1=0, threshold_format1=0.8,
          threshold_data_valid_format1a=0.9, threshold_data_valid_format2=1.5)
SRS = SRS_CASES["p6_bw7"]


def _queued_equals_synchronised(calls, distinct=True):
    """calls: NCALLS pairs (run(stream) -> rc, read() -> bytes), their buffers allocated and filled already."""
    L = pkg.lib()
    st = L.srslte_hip_stream_create()
    got = []
    for sync_each in (False, True):
        for run, _ in calls:
            assert run(st) == 0
            if sync_each:
                assert L.srslte_hip_stream_sync(st) == 0
        assert L.srslte_hip_stream_sync(st) == 0
        got.append([read() for _, read in calls])
    L.srslte_hip_stream_destroy(st)
    assert len(calls) == NCALLS and got[0] == got[1]
    assert not distinct or len(set(got[0])) == NCALLS  # the descriptors differ and so do the outputs
    return got[0]


# ---------------------------------------------------------------- PUCCH
def _pucch_tx(k):
    n = 1 + k % 2
    return pkg.PucchTx.make(pkg.PucchReq.make(0, 0x46 + k, ack_len=n, ncce=3 * k + 1), ack=(k & 1, (k >> 1) & 1))


def test_ring_wrap_pucch_tx():
    tx = pkg.UlCtrlTx(6, 1, max_pucch=1, **UL)
    grids = [pkg.DevBuf.from_host(np.zeros(tx.grid_len, np.complex64)) for _ in range(NCALLS)]
    calls = [(lambda st, k=k: tx.put_device(grids[k].ptr, 10 + k, 1, [_pucch_tx(k)], st), lambda k=k: grids[k].to_host(np.uint8).tobytes())
             for k in range(NCALLS)]
    _queued_equals_synchronised(calls)
    tx.free()


def test_ring_wrap_pucch_rx():
    """Each call's grid carries the PUCCH of its own request alone: a call that read another call's descriptor finds nothing."""
    tx, rx = pkg.UlCtrlTx(6, 1, max_pucch=1, **UL), pkg.UlCtrl(6, 1, max_pucch=1, **UL)
    grids = [pkg.DevBuf.from_host(tx.put(np.zeros((1, tx.grid_len), np.complex64), 10 + k, [_pucch_tx(k)])[1]) for k in range(NCALLS)]
    outs = [pkg.DevBuf(C.sizeof(pkg.PucchRes)) for _ in range(NCALLS)]
    calls = [(lambda st, k=k: rx.run_device(grids[k].ptr, 10 + k, 1, [_pucch_tx(k).req], outs[k].ptr, st),
              lambda k=k: outs[k].to_host(np.uint8).tobytes()) for k in range(NCALLS)]
    for k, raw in enumerate(_queued_equals_synchronised(calls)):
        r, t = pkg.PucchRes.from_buffer_copy(raw), _pucch_tx(k)
        assert r.detected == 1 and r.n_pucch == 3 * k + 1 and list(r.ack)[:t.req.ack_len] == list(t.ack)[:t.req.ack_len], k
    tx.free()
    rx.free()


# ---------------------------------------------------------------- PRACH
def test_ring_wrap_prach_gen():
    dev = pkg.Prach(6, 3, max_preambles=2)
    outs = [pkg.DevBuf(8 * dev.len * 2) for _ in range(NCALLS)]
    calls = [(lambda st, k=k: dev.gen_device([pkg.PrachTx(5 + 9 * k, 0), pkg.PrachTx(60 - k, 0)], outs[k].ptr, st),
              lambda k=k: outs[k].to_host(np.uint8).tobytes()) for k in range(NCALLS)]
    _queued_equals_synchronised(calls)
    dev.free()


def test_ring_wrap_prach_detect():
    """Call k: preamble 7 k + 2 behind 7 k samples of silence, the occasion at sample 7 k."""
    dev = pkg.Prach(6, 3, max_preambles=1)
    md = dev.info.max_det
    sigs, outs = [], []
    for k in range(NCALLS):
        rc, pre = dev.gen([(7 * k + 2, 0)])
        assert rc == 0
        sigs.append(pkg.DevBuf.from_host(np.concatenate([np.zeros(7 * k, np.complex64), pre[0][dev.info.N_cp:]])))
        outs.append([pkg.DevBuf(4), pkg.DevBuf(4 * md), pkg.DevBuf(4 * md), pkg.DevBuf(4 * md)])
        for o in outs[-1]:
            pkg.lib().srslte_hip_memset(o.ptr, 0, o.nbytes)  # rows are written up to nof_det only
    pkg.sync()
    n = dev.info.N_ifft_prach
    calls = [(lambda st, k=k: dev.detect_device(sigs[k].ptr, 7 * k + n, [pkg.PrachOccasion(7 * k, 0, 0)], *[o.ptr for o in outs[k]], st),
              lambda k=k: b"".join(o.to_host(np.uint8).tobytes() for o in outs[k])) for k in range(NCALLS)]
    for k, raw in enumerate(_queued_equals_synchronised(calls)):
        w = np.frombuffer(raw, np.uint32)
        assert (w[0], w[1]) == (1, 7 * k + 2), (k, w[:3])
    dev.free()


# ---------------------------------------------------------------- SRS
def _srs(max_srs):
    return pkg.Srs(6, SRS["cell_id"], SRS["bw_cfg"], max_srs=max_srs, subframe_config=SRS["subframe_config"])


def _srs_ue(k):
    return pkg.SrsUe.make(0, B=SRS["B"], b_hop=SRS["b_hop"], n_srs=k, I_srs=SRS["I_srs"], k_tc=k % 2, n_rrc=k, cs_used=1 << k)


def test_ring_wrap_srs_tx_and_rx():
    """The sequence tables are loaded first (a first use allocates and copies, which synchronises); then six puts, and six receive calls on
    the grids the puts wrote: |h| = 1 where the receiver used the descriptor of its own call."""
    q = _srs(1)
    rng = np.random.default_rng(5)
    tti = SRS["ttis"][0]
    bg = (rng.normal(size=(NCALLS, q.grid_len)) + 1j * rng.normal(size=(NCALLS, q.grid_len))).astype(np.complex64)
    for k in range(NCALLS):
        assert q.put(bg[k], tti + k, [_srs_ue(k)])[0] == 0
    grids = [pkg.DevBuf.from_host(bg[k]) for k in range(NCALLS)]
    calls = [(lambda st, k=k: q.put_device(grids[k].ptr, tti + k, 1, [_srs_ue(k)], st), lambda k=k: grids[k].to_host(np.uint8).tobytes())
             for k in range(NCALLS)]
    _queued_equals_synchronised(calls)
    outs = [(pkg.DevBuf(C.sizeof(pkg.SrsRes)), pkg.DevBuf(8 * pkg.SRS_MAX_CE)) for _ in range(NCALLS)]
    for _, d in outs:
        pkg.lib().srslte_hip_memset(d.ptr, 0, d.nbytes)  # a row is written up to nof_ce only
    pkg.sync()
    calls = [(lambda st, k=k: q.rx_device(grids[k].ptr, tti + k, 1, [_srs_ue(k)], outs[k][0].ptr, outs[k][1].ptr, st),
              lambda k=k: outs[k][0].to_host(np.uint8).tobytes() + outs[k][1].to_host(np.uint8).tobytes()) for k in range(NCALLS)]
    for k, raw in enumerate(_queued_equals_synchronised(calls, distinct=False)):  # every call reads |h| = 1: told apart by that, below
        r = pkg.SrsRes.from_buffer_copy(raw)
        assert r.nof_ce == 3 and abs(r.rsrp - 1) < 1e-4, (k, r.rsrp)
    q.free()


# ---------------------------------------------------------------- PHICH
def _stack(y, ce, noise):
    res = np.zeros((1, 10), np.float32)
    res[0, 0] = noise
    return np.stack(y)[None], np.asarray(ce)[None], res


def _ul_cell():
    from dl_ctrl_ul_ref import UlCell
    return UlCell(*DL)


def _dl_ctrl(max_phich=0):
    return pkg.DlCtrl(DL[0], DL[1], DL[2], cp_ext=DL[3], phich_resources=DL[4], phich_ext=DL[5], nof_rx=DL[6], max_batch=1, max_phich=max_phich)


@need_ref
def test_ring_wrap_phich():
    """Call k asks for two PHICHs of one subframe that carries them with opposite acks; the (group, sequence) pairs differ from call to call."""
    from dl_ctrl_ref import channel
    cell, rng = _ul_cell(), np.random.default_rng(17)
    assert cell.ngroups() == 2
    ctrl = _dl_ctrl(max_phich=2)
    pairs, bufs, outs = [], [], []
    for k in range(NCALLS):
        a, b = (k % 6, k, 0), ((k + 3) % 6, (k + 2) % 8, 0)
        assert cell.calc(*a) != cell.calc(*b)
        tx = cell.encode_full(20 + k, 1, [], [a + (k & 1,), b + (1 - (k & 1),)])
        y, ce, noise = channel(cell, tx, 30.0, rng)
        pairs.append((a, b))
        bufs.append([pkg.DevBuf.from_host(x) for x in _stack(y, ce, noise)])
        outs.append(pkg.DevBuf(C.sizeof(pkg.PhichRes) * 2))
    assert len({cell.calc(*p[0]) for p in pairs}) == NCALLS
    calls = [(lambda st, k=k: ctrl.phich_device(*[b.ptr for b in bufs[k]], 20 + k, 1, [(0,) + pairs[k][0], (0,) + pairs[k][1]], outs[k].ptr, st),
              lambda k=k: outs[k].to_host(np.uint8).tobytes()) for k in range(NCALLS)]
    for k, raw in enumerate(_queued_equals_synchronised(calls)):
        got = (pkg.PhichRes * 2).from_buffer_copy(raw)
        for g, p, ack in zip(got, pairs[k], (k & 1, 1 - (k & 1))):
            assert (g.ngroup, g.nseq) == cell.calc(*p) and g.ack_value == ack, (k, p)
    ctrl.free()


# ---------------------------------------------------------------- create / use / destroy
def _use_prach():
    dev, R = pkg.Prach(6, 3), prach_ref.Prach(6, 3, 0, 1)
    rc, out = dev.gen([(11, 0)])
    want = R.gen(11, 0)
    assert rc == 0 and np.max(np.abs(out[0] - want)) <= 1e-4 * np.max(np.abs(want))
    sig = want[R.N_cp:].astype(np.complex64)
    rc, got = dev.detect(sig, [(0, 0)])
    wi, wt, wp = R.detect_offset(0, sig)
    assert rc == 0 and list(got[0][0]) == list(wi) == [11] and np.array_equal(got[0][1], wt) and np.allclose(got[0][2], wp, rtol=1e-3)
    dev.free()


def _al(x):
    a = aligned(x.size, np.complex64)
    a[:] = x
    return a


def _use_ul_ctrl_tx():
    from ul_ctrl_ref import RefUlCtrl
    tx = pkg.UlCtrlTx(6, 1, max_pucch=1, **UL)
    R, t = RefUlCtrl(tx.cfg), _pucch_tx(3)
    want = _al(np.zeros(tx.grid_len, np.complex64))
    R.encode(want, 13, t)
    rc, got = tx.put(np.zeros((1, tx.grid_len), np.complex64), 13, [t])
    assert rc == 0 and np.abs(got[0] - want).max() < 1e-5
    tx.free()


def _use_ul_ctrl_rx():
    from ul_ctrl_ref import RefUlCtrl
    rx = pkg.UlCtrl(6, 1, max_pucch=1, **UL)
    R, t = RefUlCtrl(rx.cfg), _pucch_tx(2)
    grid = _al(np.zeros(rx.grid_len, np.complex64))
    R.encode(grid, 12, t)
    grid += (np.random.default_rng(2).normal(0, 0.1, (grid.size, 2)) @ [1, 1j]).astype(np.complex64)
    t.req.noise_estimate = 0.02
    rc, got = rx.batch(grid, 12, [t.req])
    want, g = R.decode(grid, 12, t.req), got[0]
    assert rc == 0 and (g.format, g.n_pucch) == (want["format"], want["n_pucch"]) and abs(g.correlation - float(want["corr"])) < 1e-4
    z = rx.debug(0, 1)[0][:want["z"].size]
    assert np.abs(z - want["z"]).max() <= 1e-3 * max(1.0, np.abs(want["z"]).max())
    assert (g.detected, g.sr, list(g.ack), g.ack_valid) == (want["detected"], want["sr"], want["ack"], want["ack_valid"]) and g.detected == 1
    rx.free()


def _use_srs():
    q, g = _srs(1), srs_golden()
    tti, ue = SRS["ttis"][0], case_ue(SRS, cs_used=0x5A)
    rc, got = q.put(np.zeros((1, q.grid_len), np.complex64), tti, [ue])
    idx = g["p6_bw7.put_idx"][0]
    assert rc == 0 and np.array_equal(got[0][idx].view(np.uint32), g["p6_bw7.put_val"][0].view(np.uint32))  # the recorded reference, bit for bit
    rng = np.random.default_rng(21)
    grid = ((rng.normal(size=(1, q.grid_len)) + 1j * rng.normal(size=(1, q.grid_len))) / np.sqrt(2)).astype(np.complex64)
    rc, res, ce = q.rx(grid, tti, [ue])
    cfg = case_cfg(SRS)
    k0, M = pkg.srs_k0(cfg, ue, tti), pkg.srs_M_sc(cfg, ue)
    m = rx_model(grid[0].reshape(-1, 72)[-1][k0 + 2 * np.arange(M)], g["p6_bw7.gen"][0][0], ue.n_srs, ue.cs_used)
    assert rc == 0 and res[0].nof_ce == 3 and np.abs(ce[0][:3] - m["ce"]).max() <= 1e-5
    assert abs(res[0].rsrp - m["rsrp"]) <= 1e-4 * m["rsrp"] and abs(res[0].noise_estimate - m["noise_estimate"]) <= 1e-4 * m["noise_estimate"]
    q.free()


def _use_dl_ctrl():
    """srslte_hip_dl_ctrl_batch: the PCFICH and the DCI search against the reference's (tests/test_gpu_dl_ctrl.py's bounds)."""
    from dl_ctrl_ref import blind_search, channel, draw_subframe
    cell, rng = _ul_cell(), np.random.default_rng(31)
    tti, cfi, rnti, tm = 77, 3, 0x4601, 0
    dcis, placed = draw_subframe(cell, tti, cfi, rnti, tm, rng, "ue")
    y, ce, noise = channel(cell, cell.encode(tti, cfi, dcis), 30.0, rng)
    ctrl = _dl_ctrl()
    rc, out, msgs = ctrl.batch(*_stack(y, ce, noise), tti, [pkg.DlCtrlReq(rnti, tm, 0, 0)])
    ctrl.free()
    cfi_ref, corr_ref = cell.pcfich(tti, y, ce, noise)
    assert rc == 0 and out[0].cfi == cfi_ref == cfi and abs(out[0].cfi_corr - corr_ref) <= 1e-3 * max(1.0, abs(corr_ref))
    cell.extract(tti, cfi, y, ce, noise)
    m = blind_search(cell, tti, cfi, rnti, tm)
    assert out[0].nof_dci == (1 if m is not None else 0) and (m is not None or not placed)
    if m is not None:
        d = msgs[0]
        assert (d.nof_bits, d.L, d.ncce, d.format, d.rnti) == (m.nof_bits, m.L, m.ncce, m.format, m.rnti)
        assert bytes(d.payload[:d.nof_bits]) == bytes(m.payload[:m.nof_bits])


def _use_phich_rx():
    """The PhichRx of a control object, made, replaced and made again by srslte_hip_dl_ctrl_set_max_phich (test_gpu_dl_ctrl_ul.py's bounds)."""
    from dl_ctrl_ref import channel
    cell, rng = _ul_cell(), np.random.default_rng(41)
    p = (2, 5, 0)
    y, ce, noise = channel(cell, cell.encode_full(31, 1, [], [p + (1,)]), 30.0, rng)
    ctrl = _dl_ctrl(max_phich=4)
    for max_phich in (0, 1):
        ctrl.set_max_phich(max_phich)
    rc, got = ctrl.phich(*_stack(y, ce, noise), 31, [(0,) + p])
    r = cell.phich_decode_full(31, y, ce, noise, *p)
    assert rc == 0 and (got[0].ngroup, got[0].nseq, got[0].ack_value) == (r["ngroup"], r["nseq"], r["ack"]) and r["ack"] == 1
    assert abs(got[0].distance - r["distance"]) <= 1e-3 * max(1.0, abs(r["distance"]))
    ctrl.free()


def _use_dl_ctrl_tx():
    from dl_ctrl_ref import F1A, make_msg
    from dl_ctrl_tx_ref import TxCell
    cell, rng = TxCell(*DL[:6]), np.random.default_rng(51)
    msg = make_msg(0x4601, 1, 0, F1A, pkg.dci_format_sizeof(6, 1, F1A), rng)
    ph = (1, 3, 0, 1)
    want = cell.encode_full(42, 2, [msg], [ph])
    tx = pkg.DlCtrlTx(DL[0], DL[1], DL[2], cp_ext=DL[3], phich_resources=DL[4], phich_ext=DL[5], max_batch=1, max_dci=1, max_phich=1)
    rc, got = tx.put(np.zeros((1,) + np.shape(want), np.complex64), 42, [2], [(0, msg)], [(0,) + ph])
    assert rc == 0 and np.array_equal(np.ascontiguousarray(got[0]).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
    tx.free()


def _use_bcast_tables():
    """The BcastTables of an encoder (PSS, SSS, PBCH: bit-exact) and of a receiver (the MIB found as the reference finds it)."""
    from dl_bcast_ref import BcastCell
    cell, rng = BcastCell(*DL[:6]), np.random.default_rng(61)
    want = cell.encode(40)
    tx = pkg.DlCtrlTx(DL[0], DL[1], DL[2], cp_ext=DL[3], phich_resources=DL[4], phich_ext=DL[5], max_batch=1)
    rc, got = tx.put_bcast(np.zeros((1,) + np.shape(want), np.complex64), 40)
    assert rc == 0 and np.array_equal(np.ascontiguousarray(got[0]).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
    tx.free()
    # one port at 20 dB: a smooth gain over the grid, which is also the estimate handed in, and sigma^2 as the noise estimate
    k, a, s2 = np.arange(cell.glen), (rng.normal(size=2) + 1j * rng.normal(size=2)) / np.sqrt(2), np.float32(0.01)
    h = (a[0] + 0.3 * a[1] * np.exp(2j * np.pi * k / cell.glen * rng.uniform(0.5, 2)))[None].astype(np.complex64)
    noise = np.sqrt(s2 / 2) * (rng.normal(size=cell.glen) + 1j * rng.normal(size=cell.glen))
    y = (h[0] * want[0] + noise).astype(np.complex64)
    res = np.zeros((1, 10), np.float32)
    res[0, 0] = s2
    ctrl = _dl_ctrl()
    rc, out = ctrl.decode_mib(y[None, None], h[None, :, None], res, 40, False)
    ctrl.free()
    ret, ports, off, pay = BcastCell(*DL[:6]).decode(y, h, s2)
    assert rc == 0 and ret == 1 and out[0].found == 1 and (out[0].nof_tx_ports, out[0].sfn_offset, bytes(out[0].payload)) == (ports, off, bytes(pay))
    assert out[0].nof_prb == 6 and out[0].sfn == 4


def _use_channel():
    """A 1.92 MHz subframe through delay and RLF: copies, bit-exact against the restatement as in test_gpu_channel.py."""
    stages = dict(delay=(10.0, 20.0, 1.0, 0.0), rlf=(500, 500))
    ch = pkg.Channel(pkg.channel_cfg(1.92e6, 1, 1, 1920, **stages))
    R = channel_ref.ChannelRef(1.92e6, 1, **stages)
    rng = np.random.default_rng(71)
    x = ((rng.standard_normal((1, 1, 1920)) + 1j * rng.standard_normal((1, 1, 1920))) / np.sqrt(2)).astype(np.complex64)
    assert np.array_equal(ch.run(x, 3, 0.25), R.run(x, 3, 0.25).astype(np.complex64))
    ch.free()


def _use_channel_fading():
    """The members only a fading channel allocates: 1.92 MHz EPA (N = 64) within the module's 1e-4 of the restatement."""
    ch = pkg.Channel(pkg.channel_cfg(1.92e6, 1, 1, 1920, fading="epa5"))
    R = channel_ref.ChannelRef(1.92e6, 1, fading="epa5")
    rng = np.random.default_rng(72)
    x = ((rng.standard_normal((1, 1, 1920)) + 1j * rng.standard_normal((1, 1, 1920))) / np.sqrt(2)).astype(np.complex64)
    a, b = np.asarray(ch.run(x, 3, 0.25), np.complex128), np.asarray(R.run(x, 3, 0.25), np.complex128)
    assert np.max(np.abs(a - b) / np.maximum(np.abs(b), np.sqrt(np.mean(np.abs(b) ** 2)))) <= 1e-4
    ch.free()


USES = {"prach": _use_prach, "srs": _use_srs, "channel": _use_channel, "channel_fading": _use_channel_fading}
REF_USES = {"ul_ctrl_tx": _use_ul_ctrl_tx, "ul_ctrl_rx": _use_ul_ctrl_rx, "dl_ctrl": _use_dl_ctrl, "phich_rx": _use_phich_rx,
            "dl_ctrl_tx": _use_dl_ctrl_tx, "bcast_tables": _use_bcast_tables}


@pytest.mark.parametrize("kind", sorted(USES) + [pytest.param(k, marks=need_ref) for k in sorted(REF_USES)])
def test_create_use_destroy_three_times(kind):
    for _ in range(3):
        dict(USES, **REF_USES)[kind]()


def test_invalid_configurations_are_refused():
    L, INV = pkg.lib(), pkg.SRSLTE_ERROR_INVALID_INPUTS
    assert L.srslte_hip_prach_create(C.byref(pkg.prach_cfg(6, 3, tdd=True))) is None
    assert L.srslte_hip_prach_create(C.byref(pkg.prach_cfg(5, 3))) is None
    for create in (L.srslte_hip_ul_ctrl_create, L.srslte_hip_ul_ctrl_tx_create):
        assert create(C.byref(pkg.ul_ctrl_cfg(6, 1, tdd=True, max_pucch=1))) is None
        assert create(C.byref(pkg.ul_ctrl_cfg(6, 1, max_pucch=0))) is None
    assert L.srslte_hip_srs_create(C.byref(pkg.srs_cfg(6, 1, 0, max_srs=1))) is None  # a 36 PRB sounding band in a 6 PRB cell
    for bad in (dict(tdd=True), dict(nof_rx=5), dict(max_batch=0)):  # the last two refuse the BcastTables' owner before they are made
        with pytest.raises(RuntimeError):
            pkg.DlCtrl(6, 1, 1, **bad)
    with pytest.raises(RuntimeError):
        pkg.DlCtrl(5, 1, 1)  # a cell bcast_tables_create refuses as well
    for bad in (dict(tdd=True), dict(max_batch=0)):
        with pytest.raises(RuntimeError):
            pkg.DlCtrlTx(6, 1, 1, **bad)
    # the PHICH receiver: no object, and a request before srslte_hip_dl_ctrl_set_max_phich has made one
    ctrl = _dl_ctrl()
    assert L.srslte_hip_dl_ctrl_set_max_phich(None, 1) == INV
    bufs = [pkg.DevBuf(8 * ctrl.grid_len), pkg.DevBuf(8 * ctrl.grid_len), pkg.DevBuf(40), pkg.DevBuf(C.sizeof(pkg.PhichRes))]
    assert ctrl.phich_device(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, 0, 1, [(0, 0, 0, 0)], bufs[3].ptr) == INV
    ctrl.free()
    h = C.c_void_p()
    for bad in (dict(rlf=(0, 0)), dict(fading="none5"), dict(awgn=(-1.0, 0))):
        assert L.srslte_hip_channel_create(C.byref(h), C.byref(pkg.channel_cfg(1.92e6, 1, 1, 1920, **bad))) == INV and not h.value
