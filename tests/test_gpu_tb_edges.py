"""The top of the per-grant transport-block range: srslte_hip_dl_rx_batch_grants / _grants2 take any transport block up to 105 528 bits, which
is up to 18 code blocks of K = 5888 (110 PRB, 256QAM). With 16-bit LLRs the decoders assemble and judge the transport blocks themselves
(TdecOpts::tb_Cof), multiplying block r's CRC24A share by a factor x^((C-1-r)(K-24)) of a table that holds 16 of them; a call with a larger
transport block has the assembly kernel (tb_crc_bytes_kernel) do it. Transport blocks of 16, 17 and 18 blocks - the last factor of the table,
and both sides of the limit - against the oracle chain on the same samples (bytes, verdicts, passes of every block), against the assembly
kernel (SRSLTE_HIP_GRANTS_TB_DIRECT=0) and against the fixed-grant pipeline; HARQ with blocks kept from the first transmission; two codewords;
8-bit LLRs; the argument checks at the top; and the fixed pipeline's stage 5 with other outputs than stage 4's."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

from _libs import OrcCbsegm, OrcOfdm, oracle, p
from lte_sim import DlConfig, OrcHarq, make_subframe, make_subframe_mimo, oracle_rx, oracle_rx_mimo

pytestmark = pytest.mark.gpu

P, CELL, AMP, SNR = 110, 5, 0.1, 34.0
# tbs -> (C, K): every one segments without filler bits and into blocks of one size
TOP = {97896: (16, 6144), 98576: (17, 5824), 104016: (17, 6144), 104376: (18, 5824), 105528: (18, 5888)}
TBS_MAX = 105528


@pytest.fixture(scope="module")
def hp():
    return importlib.import_module("srslte-emane_amd")


def chest(hp):
    hc = hp.ChestDlCfg()
    hc.filter_coef[0], hc.filter_coef[1] = 4.0, 1.0
    return hc


def erased_subframe(cfg, tti, rng, erase=None, snr_db=SNR, rv=0, data=None, width=0.6):
    """make_subframe, and with erase = r the middle `width` of the resource elements that carry code block r sent as nothing (the OFDM
    transmitter is linear: the symbols' negative is added on those REs only), so that block r fails and every other block decodes."""
    keep = {}
    iq, data = make_subframe(cfg, tti, rng, snr_db=snr_db, amp=AMP, rv=rv, data=data, keep=keep)
    if erase is not None:
        idx, y, nc = keep["idx"], keep["y"][0], int(cfg.seg.C)
        lo, hi = int((erase + 0.5 - width / 2) * len(idx) / nc), int((erase + 0.5 + width / 2) * len(idx) / nc)
        grid = np.zeros(cfg.grid_len, np.complex64)
        grid[idx[lo:hi]] = -y[lo:hi]
        q = OrcOfdm()
        oracle().orc_ofdm_init(C.byref(q), cfg.nof_prb, cfg.cp_norm)
        q.normalize = True
        out = np.zeros(cfg.sf_len, np.complex64)
        oracle().orc_ofdm_tx_sf(C.byref(q), p(grid), p(out))
        iq = (iq + np.float32(AMP) * out).astype(np.complex64)
    return iq, data


def short_mask(first, n):
    m = np.zeros((2, P), np.uint8)
    m[:, first:first + n] = 1
    return m


def run_objects(hp, llr8, calls, nsf, cmax):
    """Every call of `calls` ([(iq [nsf][...], tti0, grants)]) on a fresh object, with the decoders' own assembly (16-bit default) and then with
    SRSLTE_HIP_GRANTS_TB_DIRECT=0 (the assembly kernel); with 8-bit LLRs the assembly kernel is the only way. Per way and call: (tb, ok, passes)."""
    results = []
    for assembly_kernel in ((False, True) if not llr8 else (False,)):
        if assembly_kernel:
            os.environ["SRSLTE_HIP_GRANTS_TB_DIRECT"] = "0"  # read when the object's grants state is made (its first grants call)
        try:
            rx = hp.DlRx(CELL, P, 1, 0, 4, TBS_MAX, 6, nsf, True, chest(hp), llr_8bit=llr8)
            out = []
            for iq, tti0, grants in calls:
                hp.lib().srslte_hip_memset(rx.d_tb.ptr, 0xA5, rx.d_tb.nbytes)  # a dirty result buffer: every row and verdict must be written
                hp.lib().srslte_hip_memset(rx.d_ok.ptr, 0xA5, rx.d_ok.nbytes)
                rc, tb, ok = rx.decode_grants(np.stack(iq), tti0, grants)
                assert rc == 0
                out.append((tb.copy(), ok.copy(), rx.debug(13, np.uint32, len(iq) * cmax).reshape(len(iq), cmax)))
            results.append(out)
            rx.free()
        finally:
            os.environ.pop("SRSLTE_HIP_GRANTS_TB_DIRECT", None)
    if len(results) == 2:  # verdicts, passes and every row's bytes (of failed transport blocks too) identical both ways
        for c, ((tb_d, ok_d, it_d), (tb_k, ok_k, it_k)) in enumerate(zip(*results)):
            assert np.array_equal(ok_d, ok_k), (c, ok_d, ok_k)
            for b, g in enumerate(calls[c][2]):
                seg, nb = OrcCbsegm(), g.tbs // 8 + 3
                assert oracle().orc_cbsegm(C.byref(seg), g.tbs) == 0
                assert np.array_equal(it_d[b, :seg.C], it_k[b, :seg.C]), (c, b, g.tbs, it_d[b, :seg.C], it_k[b, :seg.C])  # the slot's own blocks
                assert np.array_equal(tb_d[b, :nb], tb_k[b, :nb]), (c, b, g.tbs, np.flatnonzero(tb_d[b, :nb] != tb_k[b, :nb])[:8])
    return results[0]


def check_vs_oracle(cfg, iq, tti, tb, ok, it, data, **kw):
    r = oracle_rx(cfg, iq, tti, **kw)
    what = (cfg.tbs, int(cfg.seg.C), tti)
    assert bool(ok) == bool(r["ok"]), what + (int(ok), r["ok"])
    assert np.array_equal(it[:cfg.seg.C], r["iters"]), what + (it[:cfg.seg.C], r["iters"])
    if r["ok"]:
        assert np.array_equal(tb[:cfg.tbs // 8 + 3], r["tb"]) and np.array_equal(tb[:cfg.tbs // 8], data), what
    return r


@pytest.mark.parametrize("llr8", [False, True])
def test_top_of_range_vs_oracle_and_assembly_kernel(hp, llr8):
    """Call 1: the five sizes of TOP on full-band 256QAM grants, each decoded, plus a 16- and an 18-block transport block with one block erased
    (those fail on block 15 / 17 resp. 0 while the others pass). Call 2: a 16- and an 18-block transport block beside short blocks
    (K = 320, 640: the unwindowed and 8-window decoders) - the mixed launch, with the assembly kernel because of the 18-block one. Call 3: the
    same without the 18-block transport block - the decoders' own assembly. Every row against the oracle chain; 16-bit: identical with
    the assembly kernel."""
    rng = np.random.default_rng(105 + llr8)
    full = {tbs: DlConfig(P, CELL, 4, tbs, cfi=1, rnti=0x4000 + i, llr8=llr8) for i, tbs in enumerate(TOP)}
    for tbs, (c, k) in TOP.items():
        s = full[tbs].seg
        assert (s.C, s.K1, s.F, s.C2) == (c, k, 0, 0), tbs
    short = [DlConfig(P, CELL, 1, 296, cfi=1, rnti=0x4100, prb_mask=short_mask(0, 3), llr8=llr8),
             DlConfig(P, CELL, 1, 616, cfi=1, rnti=0x4101, prb_mask=short_mask(5, 5), llr8=llr8)]
    assert [int(c.seg.K1) for c in short] == [320, 640]
    plan = [[(full[t], None) for t in TOP] + [(full[97896], 15), (full[105528], 0)],
            [(full[105528], None), short[0], (full[97896], 3), short[1]],
            [short[1], (full[97896], None), short[0]]]
    calls, streams = [], []
    for ci, pl in enumerate(plan):
        tti0 = 3 * ci
        st = []
        for b, x in enumerate(pl):
            cfg, erase = x if isinstance(x, tuple) else (x, None)
            iq, data = erased_subframe(cfg, tti0 + b, rng, erase, snr_db=SNR if cfg.mod == 4 else 12.0)
            st.append((cfg, iq, data, erase))
        streams.append(st)
        calls.append(([s[1] for s in st], tti0, [hp.DlGrant.make(P, c.mod, c.tbs, c.rnti, cfi=c.cfi, prb_mask=c.prb_mask) for c, _, _, _ in st]))
    out = run_objects(hp, llr8, calls, max(len(pl) for pl in plan), 18)
    n_ok = n_fail = 0
    for ci, st in enumerate(streams):
        tb, ok, it = out[ci]
        for b, (cfg, iq, data, erase) in enumerate(st):
            r = check_vs_oracle(cfg, iq, calls[ci][1] + b, tb[b], ok[b], it[b], data)
            if erase is None:
                assert r["ok"], (ci, b, cfg.tbs)  # the SNR decodes every block
            else:
                assert not r["ok"] and not r["cb_ok"][erase] and r["cb_ok"].sum() == cfg.seg.C - 1, (ci, b, r["cb_ok"])
            n_ok += bool(ok[b])
            n_fail += not ok[b]
    assert n_ok == 11 and n_fail == 3, (n_ok, n_fail)


@pytest.mark.parametrize("llr8", [False, True])
def test_top_of_range_harq_with_kept_blocks(hp, llr8):
    """A 16-block transport block, and an 18- and a 17-block one, whose LAST block is partly erased in the first transmission: blocks
    0 .. C-2 pass and are kept, the transport block fails. The retransmission (rv 2) decodes the last block only; the kept blocks' stored bytes
    complete the transport block. The 16-block one has calls of its own, so that with 16-bit LLRs the decoders assemble it (tdec_tb_stored_block:
    block 0's share times the table's last factor); the calls of the other two take the assembly kernel. Verdicts, bytes and passes (0 = kept)
    against the oracle's HARQ chain on the same samples; 16-bit: identical with the assembly kernel. (8-bit LLRs lose a little at 256QAM:
    3 dB more, so that the early blocks pass.)"""
    rng = np.random.default_rng(212 + llr8)
    for group in ((97896,), (105528, 98576)):
        cfgs = [DlConfig(P, CELL, 4, tbs, cfi=1, rnti=0x4200 + i, llr8=llr8) for i, tbs in enumerate(group)]
        datas = [rng.integers(0, 256, c.tbs // 8, dtype=np.uint8) for c in cfgs]
        tx = []
        for t, rv in enumerate((0, 2)):
            st = [erased_subframe(c, 10 * t + b, rng, int(c.seg.C) - 1 if t == 0 else None, SNR + 3.0 * llr8, rv, datas[b], 0.1)[0] for b, c in enumerate(cfgs)]
            tx.append((st, 10 * t, [hp.DlGrant.make(P, 4, c.tbs, c.rnti, cfi=1, rv=rv, new_data=t == 0) for c in cfgs]))
        out = run_objects(hp, llr8, tx, len(cfgs), 18)
        harq = [OrcHarq(c) for c in cfgs]
        for t, rv in enumerate((0, 2)):
            tb, ok, it = out[t]
            for b, c in enumerate(cfgs):
                r = check_vs_oracle(c, tx[t][0][b], 10 * t + b, tb[b], ok[b], it[b], datas[b], harq=harq[b], rv=rv, new_data=t == 0)
                nc = int(c.seg.C)
                if t == 0:  # the case this test is for: the early blocks passed, the transport block did not
                    assert not ok[b] and r["cb_ok"][:nc - 1].all() and not r["cb_ok"][nc - 1], (c.tbs, r["cb_ok"])
                else:  # delivered by the retransmission, with every block but the last one kept (not decoded again)
                    assert ok[b] and not it[b, :nc - 1].any() and it[b, nc - 1] > 0, (c.tbs, it[b, :nc])


def test_two_codewords_at_the_top(hp):
    """srslte_hip_dl_rx_batch_grants2 with closed-loop spatial multiplexing (2 ports x 2 antennas), two 105 528-bit transport blocks per
    subframe (36 code blocks), and in a second subframe a 16-block first one beside an 18-block second: both codewords' rows against the
    oracle's two-layer chain."""
    rng = np.random.default_rng(3)
    plan = [(105528, 105528, 0), (97896, 105528, 1), (105528, 104016, 0)]
    items = []
    for b, (t0, t1, pmi) in enumerate(plan):
        cfg = DlConfig(P, CELL, 4, t0, cfi=1, rnti=0x4300 + b, nof_rx=2, nof_ports=2, tx_scheme="mux", pmi=pmi, mod2=4, tbs2=t1)
        iq, data = make_subframe_mimo(cfg, 1 + b, rng, snr_db=40.0, amp=0.2)
        g = hp.DlGrant2(hp.DlGrant.make(P, 4, t0, cfg.rnti, cfi=1), 2, pmi, 4, t1, 0, 1)
        items.append((cfg, iq, data, g))
    rx = hp.DlRx(CELL, P, 1, 0, 4, TBS_MAX, 6, len(items), True, chest(hp), nof_rx=2, nof_ports=2)
    rc, tb, ok = rx.decode_grants2(np.stack([it[1] for it in items]), 1, [it[3] for it in items])
    assert rc == 0
    n_ok = 0
    for b, (cfg, iq, data, g) in enumerate(items):
        r = oracle_rx_mimo(cfg, iq, 1 + b)
        for cw in range(2):
            tbs = cfg.tbss[cw]
            assert bool(ok[cw][b]) == bool(r["ok"][cw]), (b, cw)
            if r["ok"][cw]:
                assert np.array_equal(tb[cw][b, :tbs // 8 + 3], r["tb"][cw]) and np.array_equal(tb[cw][b, :tbs // 8], data[cw]), (b, cw)
                n_ok += 1
    assert n_ok == 2 * len(items)
    rx.free()


@pytest.mark.parametrize("llr8", [False, True])
def test_top_of_range_grants_equal_fixed_pipeline(hp, llr8):
    """The fixed-grant pipeline made for 105 528 bits (18 blocks) and the per-grant entry point on the same object and subframes - decoded ones
    and one with an erased block - give the same bytes and verdicts."""
    rng = np.random.default_rng(6 + llr8)
    cfg = DlConfig(P, CELL, 4, TBS_MAX, cfi=1, rnti=0x1234, llr8=llr8)
    iq = np.stack([erased_subframe(cfg, t, rng, 7 if t == 2 else None)[0] for t in range(4)])
    rx = hp.DlRx(CELL, P, 1, 0x1234, 4, TBS_MAX, 6, 4, True, chest(hp), llr_8bit=llr8)
    tb0, ok0 = rx.decode(iq, 0)
    tb0, ok0 = tb0.copy(), ok0.copy()
    rc, tb1, ok1 = rx.decode_grants(iq, 0, [hp.DlGrant.make(P, 4, TBS_MAX, 0x1234) for _ in range(4)])
    assert rc == 0
    assert np.array_equal(ok0, ok1) and ok0.tolist() == [1, 1, 0, 1], (ok0, ok1)
    for b in range(4):
        assert not ok0[b] or np.array_equal(tb0[b], tb1[b]), b
    rx.free()


def test_top_of_range_argument_checks(hp):
    """Grants above 105 528 bits, with filler bits, with a second block size or not a whole number of bytes are refused."""
    seg = [OrcCbsegm() for _ in range(3)]
    for s, tbs in zip(seg, (105536, 105520, 105464)):
        assert oracle().orc_cbsegm(C.byref(s), tbs) == 0
    assert seg[1].F > 0 and seg[2].F == 0 and seg[2].C2 > 0
    rng = np.random.default_rng(0)
    cfg = DlConfig(P, CELL, 4, TBS_MAX, cfi=1, rnti=0x1234)
    iq = erased_subframe(cfg, 0, rng)[0][None]
    rx = hp.DlRx(CELL, P, 1, 0, 4, TBS_MAX, 6, 1, True, chest(hp))
    for tbs in (105536, 105520, 105464, 105524):
        rc, _, _ = rx.decode_grants(iq, 0, [hp.DlGrant.make(P, 4, tbs, 0x1234)])
        assert rc == hp.SRSLTE_ERROR_INVALID_INPUTS, tbs
    rc, tb, ok = rx.decode_grants(iq, 0, [hp.DlGrant.make(P, 4, TBS_MAX, 0x1234)])  # the object is still usable
    assert rc == 0 and ok[0] == 1
    rx.free()


def test_stage5_with_other_outputs_than_stage4(hp):
    """srslte_hip_dl_rx_stage one by one on a pipeline whose decoders assemble the transport blocks in stage 4 (16 bit, 16 windows): stage 5
    called with another verdict buffer, and then with another row stride, than stage 4 still writes rows and verdicts there - equal to
    decode()'s."""
    rng = np.random.default_rng(5)
    cfg = DlConfig(100, 1, 3, 75376, cfi=1, rnti=0x1234)
    nsf = 4
    x = np.stack([make_subframe(cfg, t, rng, snr_db=18.5 if t != 1 else 14.0, amp=0.1)[0] for t in range(nsf)])
    rx = hp.DlRx(1, 100, 1, 0x1234, 3, 75376, 6, nsf, True, chest(hp))
    tb_ref, ok_ref = rx.decode(x, 0)
    tb_ref, ok_ref = tb_ref.copy(), ok_ref.copy()
    assert ok_ref.any()
    L = hp.lib()
    s1, s2 = rx.tb_stride, rx.tb_stride + 48
    din, dtb, dok, dok2 = hp.DevBuf.from_host(x), hp.DevBuf(s2 * nsf), hp.DevBuf(nsf), hp.DevBuf(nsf)
    nb = 75376 // 8 + 3

    def fill():
        for d in (dtb, dok, dok2):
            L.srslte_hip_memset(d.ptr, 0xA5, d.nbytes)

    def rows(stride):
        return dtb.to_host(np.uint8)[:stride * nsf].reshape(nsf, stride)[:, :nb]

    fill()
    for s in range(5):
        assert L.srslte_hip_dl_rx_stage(rx.h, s, din.ptr, 0, nsf, dtb.ptr, s1, dok.ptr, None) == 0
    assert L.srslte_hip_dl_rx_stage(rx.h, 5, din.ptr, 0, nsf, dtb.ptr, s1, dok2.ptr, None) == 0  # another verdict buffer
    hp.sync()
    assert np.array_equal(dok2.to_host(np.uint8), ok_ref), (dok2.to_host(np.uint8), ok_ref)
    tb = rows(s1)
    for b in range(nsf):
        assert not ok_ref[b] or np.array_equal(tb[b], tb_ref[b]), b
    fill()
    assert L.srslte_hip_dl_rx_stage(rx.h, 5, din.ptr, 0, nsf, dtb.ptr, s2, dok.ptr, None) == 0  # another row stride
    hp.sync()
    assert np.array_equal(dok.to_host(np.uint8), ok_ref)
    tb = rows(s2)
    for b in range(nsf):
        assert not ok_ref[b] or np.array_equal(tb[b], tb_ref[b]), b
    for d in (din, dtb, dok, dok2):
        d.free()
    rx.free()
