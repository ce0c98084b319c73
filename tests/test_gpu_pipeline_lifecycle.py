"""The PDSCH / PUSCH pipelines' memory and descriptor staging (csrc/dev_buf.hpp in pdsch.hip), as test_gpu_object_lifecycle.py does it for the
control and auxiliary modules: 6 PRB, normal CP, one subframe, one grant per call, QPSK, and the smallest transport block that segments
without filler bits (16 bits: one code block of K = 40).

Staging ring wrap. Six grants calls with different RNTIs and payloads and their own output buffers, queued on one stream with no host
synchronisation in between, then the same six with a synchronisation after each: byte-identical outputs, pairwise distinct. In the two
receive modes a kernel of the call reads the pinned descriptor buffer itself.

Create / use / destroy, three times in a row per kind; the kinds are chosen so that every part an object makes on first use is there at
destroy in one kind and absent in another. Each use is compared as the module's own GPU test compares it: receivers against the oracle
chain on identical IQ (transport block bytes, CRC flags; noise free, so every block decodes and equals the payload sent), transmitters
against the oracle's stimulus generator at 1e-4 of the signal's largest sample. Then the configurations every create refuses."""
import ctypes as C
import importlib

import numpy as np
import pytest

from lte_sim import DlConfig, UlConfig, make_subframe, make_subframe_mimo, make_ul_subframe, oracle_rx, oracle_ul_rx
from test_gpu_object_lifecycle import NCALLS, _queued_equals_synchronised

pkg = importlib.import_module("srslte-emane_amd")
pytestmark = pytest.mark.gpu

P, CELL, MOD, TBS, CFI = 6, 1, 1, 16, 1
NB = TBS // 8
TTIS = (1, 2, 3, 4, 6, 7)  # one per call: no subframe whose centre six PRBs - the whole cell - carry PSS / SSS / PBCH
UL = dict(L_prb=2, n_prb=1, n_dmrs=0)
TOL = 1e-4
vp, u32 = C.c_void_p, C.c_uint32


class DlTxGrant(C.Structure):
    _fields_ = [("sf", u32), ("grant", pkg.DlGrant)]


def _close(a, b, what):
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    assert np.abs(a - b).max() <= TOL * np.abs(b).max(), what


def _chest():
    hc = pkg.ChestDlCfg()
    hc.filter_coef[0], hc.filter_coef[1] = 4.0, 1.0
    return hc


def _dl_cfg(rnti=0x1234, **kw):
    return DlConfig(P, CELL, MOD, TBS, cfi=CFI, rnti=rnti, **kw)


def _dl_rx(rnti=0x1234, **kw):
    return pkg.DlRx(CELL, P, CFI, rnti, MOD, TBS, 6, 1, True, _chest(), **kw)


def _dl_grant(rnti, rv=0):
    return pkg.DlGrant.make(P, MOD, TBS, rnti, cfi=CFI, rv=rv)


def _ul_cfg(rnti=0x1234):
    return UlConfig(P, CELL, MOD, TBS, UL["L_prb"], UL["n_prb"], UL["n_dmrs"], rnti=rnti)


def _ul_rx(**kw):
    return pkg.UlRx(CELL, P, 0x1234, MOD, TBS, UL["L_prb"], UL["n_prb"], UL["n_dmrs"], 6, 1, **kw)


def _ul_tx(**kw):
    return pkg.UlTx(CELL, P, 0x1234, MOD, TBS, UL["L_prb"], UL["n_prb"], UL["n_dmrs"], 1, **kw)


def _ul_grant(rnti, **kw):
    return pkg.UlGrant.make(0, rnti, UL["L_prb"], UL["n_prb"], MOD, TBS, n_dmrs=UL["n_dmrs"], **kw)


def _bind(L):
    L.srslte_hip_ul_rx_batch_grants.argtypes = [vp, vp, u32, u32, vp, u32, vp, u32, vp, vp]
    L.srslte_hip_dl_tx_batch_grants.argtypes = [vp, vp, u32, u32, u32, vp, u32, vp, vp]
    L.srslte_hip_ul_tx_batch_grants.argtypes = [vp, vp, u32, vp, vp, vp, u32, u32, vp, u32, vp, vp]
    for fn in (L.srslte_hip_ul_rx_grants_ack, L.srslte_hip_ul_rx_grants_ri, L.srslte_hip_ul_rx_grants_cqi):
        fn.restype, fn.argtypes = vp, [vp]
    return L


# ---------------------------------------------------------------- ring wrap
def _rx_calls(fn_of_k, stride):
    """Six receive calls with their own transport-block and flag buffers; read(): the block's bytes (payload + CRC) and the flag."""
    outs = [(pkg.DevBuf(stride), pkg.DevBuf(1)) for _ in range(NCALLS)]
    calls = [(lambda st, k=k: fn_of_k(k, outs[k][0].ptr, outs[k][1].ptr, st),
              lambda k=k: outs[k][0].to_host(np.uint8)[:NB + 3].tobytes() + outs[k][1].to_host(np.uint8).tobytes()) for k in range(NCALLS)]
    assert calls[0][0](None) == 0  # the state and tables of the mode are made by the first call, which synchronises: not among the six
    pkg.sync()
    return calls


def test_ring_wrap_dl_rx_grants():
    L, rng, rx = pkg.lib(), np.random.default_rng(101), _dl_rx()
    sent = [make_subframe(_dl_cfg(0x100 + k), TTIS[k], rng) for k in range(NCALLS)]
    ins = [pkg.DevBuf.from_host(iq) for iq, _ in sent]
    grants = [(pkg.DlGrant * 1)(_dl_grant(0x100 + k)) for k in range(NCALLS)]
    calls = _rx_calls(lambda k, tb, ok, st: L.srslte_hip_dl_rx_batch_grants(rx.h, ins[k].ptr, TTIS[k], 1, grants[k], tb, rx.tb_stride, ok, st), rx.tb_stride)
    for k, raw in enumerate(_queued_equals_synchronised(calls)):
        r = oracle_rx(_dl_cfg(0x100 + k), sent[k][0], TTIS[k])
        assert r["ok"] and raw == r["tb"].tobytes() + b"\x01" and raw[:NB] == sent[k][1].tobytes(), k
    rx.free()


def test_ring_wrap_ul_rx_grants():
    L, rng, rx = _bind(pkg.lib()), np.random.default_rng(102), _ul_rx(max_grants=1)
    sent = [make_ul_subframe(_ul_cfg(0x200 + k), TTIS[k], rng) for k in range(NCALLS)]
    ins = [pkg.DevBuf.from_host(iq) for iq, _ in sent]
    grants = [(pkg.UlGrant * 1)(_ul_grant(0x200 + k)) for k in range(NCALLS)]
    calls = _rx_calls(lambda k, tb, ok, st: L.srslte_hip_ul_rx_batch_grants(rx.h, ins[k].ptr, TTIS[k], 1, grants[k], 1, tb, rx.tb_stride, ok, st), rx.tb_stride)
    for k, raw in enumerate(_queued_equals_synchronised(calls)):
        r = oracle_ul_rx(_ul_cfg(0x200 + k), sent[k][0], TTIS[k])
        assert r["ok"] and raw == r["tb"].tobytes() + b"\x01" and raw[:NB] == sent[k][1].tobytes(), k
    rx.free()


def _tx_calls(fn_of_k, sf_len, rng):
    datas = [rng.integers(0, 256, NB, dtype=np.uint8) for _ in range(NCALLS)]
    tbs = [pkg.DevBuf.from_host(np.concatenate([d, np.zeros(16 - NB, np.uint8)])) for d in datas]
    outs = [pkg.DevBuf(8 * sf_len) for _ in range(NCALLS)]
    calls = [(lambda st, k=k: fn_of_k(k, tbs[k].ptr, outs[k].ptr, st), lambda k=k: outs[k].to_host(np.uint8).tobytes()) for k in range(NCALLS)]
    assert calls[0][0](None) == 0  # as in _rx_calls
    pkg.sync()
    return calls, datas


def test_ring_wrap_dl_tx_grants():
    L, rng = _bind(pkg.lib()), np.random.default_rng(103)
    tx = pkg.DlTx(CELL, P, CFI, 0x1234, MOD, TBS, 1, max_grants=1)
    grants = [(DlTxGrant * 1)(DlTxGrant(0, _dl_grant(0x300 + k))) for k in range(NCALLS)]
    calls, datas = _tx_calls(lambda k, tb, iq, st: L.srslte_hip_dl_tx_batch_grants(tx.h, tb, 16, TTIS[k], 1, grants[k], 1, iq, st), tx.sf_len, rng)
    for k, raw in enumerate(_queued_equals_synchronised(calls)):
        iq_o, _ = make_subframe(_dl_cfg(0x300 + k), TTIS[k], rng, data=datas[k])
        _close(np.frombuffer(raw, np.complex64), iq_o, k)
    tx.free()


def test_ring_wrap_ul_tx_grants():
    L, rng, tx = _bind(pkg.lib()), np.random.default_rng(104), _ul_tx(max_grants=1)
    grants = [(pkg.UlGrant * 1)(_ul_grant(0x400 + k)) for k in range(NCALLS)]
    calls, datas = _tx_calls(lambda k, tb, iq, st: L.srslte_hip_ul_tx_batch_grants(tx.h, tb, 16, None, None, None, TTIS[k], 1, grants[k], 1, iq, st),
                             tx.sf_len, rng)
    for k, raw in enumerate(_queued_equals_synchronised(calls)):
        iq_o, _ = make_ul_subframe(_ul_cfg(0x400 + k), TTIS[k], rng, data=datas[k])
        _close(np.frombuffer(raw, np.complex64), iq_o, k)
    tx.free()


# ---------------------------------------------------------------- create / use / destroy
def _same_as_oracle(tb, ok, r, data, what=None):
    assert r["ok"] and ok == 1 and np.array_equal(tb, r["tb"]) and np.array_equal(tb[:NB], data), what


def _use_dl_rx(grants):
    rng, cfg, rx = np.random.default_rng(111), _dl_cfg(), _dl_rx()
    iq, data = make_subframe(cfg, 3, rng)
    r = oracle_rx(cfg, iq, 3)
    tb, ok = rx.decode(iq[None], 3)
    _same_as_oracle(tb[0], ok[0], r, data)
    if grants:
        rc, tb, ok = rx.decode_grants(iq[None], 3, [_dl_grant(cfg.rnti)])
        assert rc == 0
        _same_as_oracle(tb[0], ok[0], r, data, "grants")
    rx.free()


def _use_dl_rx_two_codewords():
    """test_gpu_mimo.py's noise-free check: both transport blocks of a large-delay CDD subframe come back."""
    rng = np.random.default_rng(112)
    cfg = _dl_cfg(nof_rx=2, nof_ports=2, tx_scheme="cdd", mod2=MOD, tbs2=TBS)
    iq, data = make_subframe_mimo(cfg, 3, rng)
    rx = _dl_rx(nof_rx=2, nof_ports=2, tx_scheme=3, mod2=MOD, tbs2=TBS)
    tb, ok = rx.decode(iq[None], 3)
    for cw in range(2):
        assert ok[cw].all() and np.array_equal(tb[cw][0][:NB], data[cw]), cw
    rx.free()


def _use_dl_rx_keep_symbols():
    rng, cfg, rx = np.random.default_rng(113), _dl_cfg(), _dl_rx()
    iq, data = make_subframe(cfg, 3, rng)
    r = oracle_rx(cfg, iq, 3, keep=True)
    for enable in (True, False, True):
        rx.keep_symbols(enable)
        assert bool(pkg.lib().srslte_hip_dl_rx_debug_buffer(rx.h, 3)) == enable
        tb, ok = rx.decode(iq[None], 3)
        _same_as_oracle(tb[0], ok[0], r, data, enable)
        if enable:
            _close(rx.debug(3, np.complex64, len(r["d"])), r["d"], "d")
    rx.free()


def _use_dl_rx_harq():
    """rv 1 and 2 make their rate de-matching tables on first use; noise free, every transmission decodes on its own."""
    rng, cfg, rx = np.random.default_rng(114), _dl_cfg(), _dl_rx()
    for rv in (1, 2):
        iq, data = make_subframe(cfg, 3 + rv, rng, rv=rv)
        r = oracle_rx(cfg, iq, 3 + rv, rv=rv)
        tb, ok = rx.decode_harq(iq[None], 3 + rv, rv, True)
        _same_as_oracle(tb[0], ok[0], r, data, rv)
    rx.free()


def _use_dl_rx_ce_full():
    """A single-port pipeline keeps one row of estimates per subframe; debug buffer 1 expands it to whole grids in a buffer made on request."""
    rng, cfg, rx = np.random.default_rng(115), _dl_cfg(), _dl_rx()
    iq, data = make_subframe(cfg, 3, rng)
    r = oracle_rx(cfg, iq, 3, keep=True)
    tb, ok = rx.decode(iq[None], 3)
    _same_as_oracle(tb[0], ok[0], r, data)
    _close(rx.debug(1, np.complex64, cfg.grid_len), r["ce"], "ce")
    rx.free()


def _use_dl_rx_csi():
    """srslte_hip_dl_rx_csi_batch on the batch's own estimates: the record of a stand-alone Csi object on the same estimates and noise figure."""
    rng = np.random.default_rng(116)
    cfg = _dl_cfg(nof_rx=2, nof_ports=2)
    iq, data = make_subframe(cfg, 3, rng)
    rx = _dl_rx(nof_rx=2, nof_ports=2)
    tb, ok = rx.decode(iq[None], 3)
    assert ok[0] == 1 and np.array_equal(tb[0][:NB], data)
    rc, recs = rx.csi(1)
    assert rc == 0
    d_ce, d_res = pkg.lib().srslte_hip_dl_rx_debug_buffer(rx.h, 1), pkg.lib().srslte_hip_dl_rx_debug_buffer(rx.h, 2)
    csi, out = pkg.Csi(P, 2, 2), pkg.DevBuf(C.sizeof(pkg.CsiRes))
    assert csi.run_device(d_ce, d_res, 1, out.ptr) == 0
    pkg.sync()
    assert bytes(out.to_host(np.uint8)) == bytes(recs[0])
    csi.free()
    rx.free()


def _use_ul_rx_harq():
    rng, cfg, rx = np.random.default_rng(121), _ul_cfg(), _ul_rx()
    for rv, tti in ((0, 3), (1, 4)):
        iq, data = make_ul_subframe(cfg, tti, rng, rv=rv)
        r = oracle_ul_rx(cfg, iq, tti, rv=rv)
        tb, ok = rx.decode_harq(iq[None], tti, rv, True) if rv else rx.decode(iq[None], tti)
        _same_as_oracle(tb[0], ok[0], r, data, rv)
    rx.free()


def _use_ul_rx_grants():
    """HARQ-ACK, rank indication and an 8-bit CQI report on the PUSCH: the three accessors are null until the first grants call has made the state."""
    L, rng, cfg, rx = _bind(pkg.lib()), np.random.default_rng(122), _ul_cfg(), _ul_rx(max_grants=1)
    for fn in (L.srslte_hip_ul_rx_grants_ack, L.srslte_hip_ul_rx_grants_ri, L.srslte_hip_ul_rx_grants_cqi):
        assert fn(rx.h) is None
    uci = dict(ack_len=2, I_offset_ack=9, ri_len=1, I_offset_ri=8, cqi_len=8, I_offset_cqi=7)
    ack, ri, cqi = (1, 0), (1,), tuple(int(v) for v in rng.integers(0, 2, 8))
    iq, data = make_ul_subframe(cfg, 3, rng, ack=ack, I_offset_ack=9, ri=ri, I_offset_ri=8, cqi=cqi, I_offset_cqi=7)
    r = oracle_ul_rx(cfg, iq, 3, O_ack=2, I_offset_ack=9, O_ri=1, I_offset_ri=8, O_cqi=8, I_offset_cqi=7)
    tb, ok = rx.decode_grants(iq[None], 3, [_ul_grant(cfg.rnti, **uci)])
    _same_as_oracle(tb[0][:NB + 3], ok[0], r, data)
    (a, i), (q, q_ok) = rx.grants_uci(), rx.grants_cqi()
    assert tuple(a[0]) == ack and tuple(i[0][:1]) == ri and q_ok[0] == 1 and tuple(q[0][:8]) == cqi == tuple(r["cqi"])
    rx.free()


def _use_dl_tx(rvs):
    rng, cfg = np.random.default_rng(131), _dl_cfg()
    tx = pkg.DlTx(CELL, P, CFI, cfg.rnti, MOD, TBS, 1)
    data = rng.integers(0, 256, NB, dtype=np.uint8)
    for rv in rvs:
        iq_o, _ = make_subframe(cfg, 3, rng, rv=rv, data=data)
        _close(tx.encode(data[None], 3, rv)[0, 0], iq_o, rv)
    tx.free()


def _dl_tx_grants_two(tx, rng, rnti):
    """A two-codeword grants call on a 2-port cell -> the samples of both ports."""
    g2 = pkg.DlGrant2(_dl_grant(rnti), 3, 0, MOD, TBS, 0, 1)
    rc, iq = tx.encode_grants2([[rng.integers(0, 256, NB, dtype=np.uint8) for _ in range(2)]], 3, 1, [(0, g2)])
    assert rc == 0
    return iq.copy()


def _use_dl_tx_grants():
    rng, cfg = np.random.default_rng(132), _dl_cfg(0x77)
    tx = pkg.DlTx(CELL, P, CFI, 0x1234, MOD, TBS, 1, max_grants=1)
    data = rng.integers(0, 256, NB, dtype=np.uint8)
    iq_o, _ = make_subframe(cfg, 3, rng, data=data)
    _close(tx.encode_grants([data], 3, 1, [(0, _dl_grant(0x77))])[0, 0], iq_o, "grants")
    tx.free()


def _use_dl_tx_grants_regrow():
    """A single-codeword grants call, then a two-codeword one, which makes the state anew for twice the codewords: the samples of an object
    whose first call is the two-codeword one."""
    tx, fresh = [pkg.DlTx(CELL, P, CFI, 0x1234, MOD, TBS, 1, 2, max_grants=1) for _ in range(2)]
    rng = np.random.default_rng(133)
    data = rng.integers(0, 256, NB, dtype=np.uint8)
    one = tx.encode_grants([data], 3, 1, [(0, _dl_grant(0x78))])
    assert np.abs(one).max() > 0
    got, want = _dl_tx_grants_two(tx, np.random.default_rng(5), 0x79), _dl_tx_grants_two(fresh, np.random.default_rng(5), 0x79)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.abs(got).max() > 0
    tx.free()
    fresh.free()


def _use_ul_tx():
    rng, cfg, tx = np.random.default_rng(141), _ul_cfg(), _ul_tx()
    data = rng.integers(0, 256, NB, dtype=np.uint8)
    iq_o, _ = make_ul_subframe(cfg, 3, rng, data=data)
    _close(tx.encode(data[None], 3)[0], iq_o, "ul_tx")
    tx.free()


def _use_ul_tx_grants_long_cqi():
    """A CQI report of 20 bits (above 11: the convolutional code, whose rate-matching order table the grants state makes on first use)."""
    rng, cfg, tx = np.random.default_rng(142), _ul_cfg(0x55), _ul_tx(max_grants=1)
    data, cqi = rng.integers(0, 256, NB, dtype=np.uint8), tuple(int(v) for v in rng.integers(0, 2, 20))
    iq_o, _ = make_ul_subframe(cfg, 3, rng, data=data, cqi=cqi, I_offset_cqi=2)  # beta 1.125: 227 of the 288 symbols, 61 left for the UL-SCH
    iq = tx.encode_grants([data], 3, 1, [_ul_grant(0x55, cqi_len=20, I_offset_cqi=2)], cqi=[cqi])
    _close(iq[0], iq_o, "ul_tx grants")
    tx.free()


def _use_sch():
    """srslte_hip_sch_decode: one transport block from host LLRs into host soft buffers, as the drop-in's srslte_dlsch_decode2 calls it."""
    from _libs import oracle, p
    from lte_sim import OrcSchCfg
    L, rng = pkg.lib(), np.random.default_rng(151)
    L.srslte_hip_sch_create.restype, L.srslte_hip_sch_create.argtypes = vp, [u32, u32, C.c_int]
    L.srslte_hip_sch_destroy.argtypes = [vp]
    L.srslte_hip_sch_decode.argtypes = [vp, vp, u32, u32, C.c_int, u32, u32, u32, vp, vp, vp, vp]
    nbits, K = 288, TBS + 24
    data, bits = rng.integers(0, 256, NB, dtype=np.uint8), np.zeros(nbits, np.uint8)
    assert oracle().orc_dlsch_encode(C.byref(OrcSchCfg(TBS, nbits, 2, 0, 4)), p(data), p(bits)) == 0
    e = (100 * (2 * bits.astype(np.int16) - 1)).astype(np.int16)
    soft, crc, out, passes = np.zeros(3 * (6144 + 32) + 64, np.int16), np.zeros(1, np.uint8), np.zeros(768, np.uint8), u32(0)
    rows = (vp * 1)(soft.ctypes.data)
    q = L.srslte_hip_sch_create(TBS, nbits, 0)
    assert q
    assert L.srslte_hip_sch_decode(q, e.ctypes.data, nbits, TBS, MOD, 1, 0, 4, rows, crc.ctypes.data, out.ctypes.data, C.byref(passes)) == 0
    assert crc[0] == 1 and passes.value >= 1 and np.array_equal(out[:NB], data) and K == 40
    L.srslte_hip_sch_destroy(q)


def _use_pool():
    """srslte_hip_dl_rx_pool_* at depth 2: one submission, then the wait; the pool's destroy synchronises its streams before the objects go."""
    L, rng, cfg, rx = pkg.lib(), np.random.default_rng(161), _dl_cfg(), _dl_rx()
    L.srslte_hip_dl_rx_pool_create.restype, L.srslte_hip_dl_rx_pool_create.argtypes = vp, [vp, u32]
    L.srslte_hip_dl_rx_pool_submit.restype = C.c_int64
    L.srslte_hip_dl_rx_pool_submit.argtypes = [vp, vp, u32, u32, vp, vp, u32, vp, vp]
    L.srslte_hip_dl_rx_pool_wait.argtypes = [vp, C.c_int64]
    L.srslte_hip_dl_rx_pool_destroy.argtypes = [vp]
    iq, data = make_subframe(cfg, 3, rng)
    r = oracle_rx(cfg, iq, 3)
    pool = L.srslte_hip_dl_rx_pool_create(C.byref(rx.cfg), 2)
    assert pool
    din = pkg.DevBuf.from_host(iq)
    t = L.srslte_hip_dl_rx_pool_submit(pool, din.ptr, 3, 1, None, rx.d_tb.ptr, rx.tb_stride, rx.d_ok.ptr, None)
    assert t == 0 and L.srslte_hip_dl_rx_pool_wait(pool, t) == 0
    _same_as_oracle(rx.d_tb.to_host(np.uint8)[:NB + 3], rx.d_ok.to_host(np.uint8)[0], r, data)
    L.srslte_hip_dl_rx_pool_destroy(pool)
    rx.free()


USES = {"dl_rx_fixed": lambda: _use_dl_rx(False), "dl_rx_fixed_then_grants": lambda: _use_dl_rx(True), "dl_rx_two_codewords": _use_dl_rx_two_codewords,
        "dl_rx_keep_symbols": _use_dl_rx_keep_symbols, "dl_rx_harq_rv_1_2": _use_dl_rx_harq, "dl_rx_ce_full": _use_dl_rx_ce_full, "dl_rx_csi": _use_dl_rx_csi,
        "ul_rx_fixed_then_harq": _use_ul_rx_harq, "ul_rx_grants": _use_ul_rx_grants, "dl_tx_fixed_rv_0_2": lambda: _use_dl_tx((0, 2)),
        "dl_tx_grants": _use_dl_tx_grants, "dl_tx_grants_one_then_two_codewords": _use_dl_tx_grants_regrow, "ul_tx_fixed": _use_ul_tx,
        "ul_tx_grants_long_cqi": _use_ul_tx_grants_long_cqi, "sch": _use_sch, "pool": _use_pool}


@pytest.mark.parametrize("kind", sorted(USES))
def test_create_use_destroy_three_times(kind):
    for _ in range(3):
        USES[kind]()


def test_invalid_configurations_are_refused():
    """A modulation out of range, a TBS that needs filler bits (496 + 24 = 520 lies between the interleaver sizes 512 and 528), three ports,
    MBSFN with two ports."""
    L = _bind(pkg.lib())
    dl_rx = dict(cell_id=CELL, nof_prb=P, cfi=CFI, rnti=1, mod=MOD, tbs=TBS, max_iterations=6, max_batch=1)
    for bad in (dict(mod=5), dict(tbs=496), dict(nof_ports=3), dict(nof_ports=2, mbsfn=(1, 1))):
        with pytest.raises(RuntimeError):
            pkg.DlRx(**dict(dl_rx, **bad))
    dl_tx = dict(cell_id=CELL, nof_prb=P, cfi=CFI, rnti=1, mod=MOD, tbs=TBS, max_batch=1)
    for bad in (dict(mod=5), dict(tbs=496), dict(nof_ports=3), dict(nof_ports=2, mbsfn=(1, 1))):
        with pytest.raises(RuntimeError):
            pkg.DlTx(**dict(dl_tx, **bad))
    ul = dict(cell_id=CELL, nof_prb=P, rnti=1, mod=MOD, tbs=TBS, **UL)
    for bad in (dict(mod=4), dict(tbs=496)):
        with pytest.raises(RuntimeError):
            pkg.UlRx(max_iterations=6, max_batch=1, **dict(ul, **bad))
        with pytest.raises(RuntimeError):
            pkg.UlTx(max_batch=1, **dict(ul, **bad))
    L.srslte_hip_sch_create.restype, L.srslte_hip_sch_create.argtypes = vp, [u32, u32, C.c_int]
    assert L.srslte_hip_sch_create(0, 288, 0) is None and L.srslte_hip_sch_create(TBS, 0, 0) is None
    L.srslte_hip_dl_rx_pool_create.restype, L.srslte_hip_dl_rx_pool_create.argtypes = vp, [vp, u32]
    rx = _dl_rx()
    assert L.srslte_hip_dl_rx_pool_create(C.byref(rx.cfg), 0) is None and L.srslte_hip_dl_rx_pool_create(C.byref(rx.cfg), 17) is None
    rx.free()
