"""UL DCIs and the PHICH on the device (srslte_hip_dl_ctrl_batch_ul, srslte_hip_dl_ctrl_phich_batch) against the reference's own functions in
oracle/_ref/libsrslte_ref.so: srslte_phich_calc + srslte_phich_decode with the estimates and the noise figure the device is given, and the
restatement of dci_blind_search's pending rule + srslte_ue_dl_find_ul_dci over srslte_pdcch_decode_msg (tests/dl_ctrl_ul_ref.py)."""
import ctypes as C
import importlib

import numpy as np
import pytest

from _libs import ref
from dl_ctrl_ref import F0, SIRNTI, blind_search, channel
from dl_ctrl_ul_ref import UlCell, draw_ul_subframe, hand_cases, is_crnti, near_tie, phich_subframes, ul_search
from test_gpu_dl_ctrl import CELLS

pkg = importlib.import_module("srslte-emane_amd")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(ref() is None, reason="oracle/_ref/libsrslte_ref.so is not built")]

BAD = pkg.SRSLTE_ERROR_INVALID_INPUTS


def _ctrl(spec, max_batch, max_phich=0):
    return pkg.DlCtrl(spec[0], spec[1], spec[2], cp_ext=spec[3], phich_resources=spec[4], phich_ext=spec[5], nof_rx=spec[6], max_batch=max_batch,
                      max_phich=max_phich)


def _stack(subs):
    res = np.zeros((len(subs), 10), np.float32)
    res[:, 0] = [s["noise"] for s in subs]
    return np.stack([np.stack(s["y"]) for s in subs]), np.stack([s["ce"] for s in subs]), res


def _close(a, b):
    return abs(a - b) <= 1e-3 * max(1.0, abs(b))


@pytest.mark.parametrize("idx", range(len(CELLS)))
def test_phich_against_the_reference(idx):
    """ngroup / nseq equal; distance, z and the soft bits within the bound of the PCFICH correlation (1e-3 max(1, |ref|)); ack_value equal
    unless the reference's own |corr1 - corr0| is within that bound (none of the 448 requests drawn here is: tests/test_dl_ctrl_ul_host.py)."""
    spec = CELLS[idx]
    cell, tti0, subs = phich_subframes(spec, 3000 + idx)
    reqs = [(b,) + p[:3] for b, s in enumerate(subs) for p in s["phichs"]]
    ctrl = _ctrl(spec, len(subs), max(1, len(reqs)))
    rc, got = ctrl.phich(*_stack(subs), tti0, reqs)
    assert rc == 0 and len(got) == len(reqs) > 10
    soft = ctrl.phich_soft(len(reqs))
    ctrl.free()
    aside, worst = 0, 0.0
    for (b, *p), g, sv in zip(reqs, got, soft):
        s = subs[b]
        r = cell.phich_decode_full(s["tti"], s["y"], s["ce"], s["noise"], *p)
        assert (g.ngroup, g.nseq) == (r["ngroup"], r["nseq"]), (spec, b, p)
        worst = max(worst, abs(g.distance - r["distance"]) / max(1.0, abs(r["distance"])))
        assert _close(g.distance, r["distance"]), (spec, b, p, g.distance, r["distance"])
        for i in range(3):
            assert _close(sv.z[i][0], r["z"][i].real) and _close(sv.z[i][1], r["z"][i].imag) and _close(sv.bits[i], r["bits"][i]), (spec, b, p, i)
        if near_tie(r):
            aside += 1
        else:
            assert g.ack_value == r["ack"], (spec, b, p, g.distance, r["distance"])
    print("cell %s: %d PHICHs, largest distance deviation %.3g of the bound's scale, %d set aside" % (spec, len(reqs), worst, aside))
    assert aside <= 0.01 * len(reqs)
    # clean subframes (30 dB): the ack that was sent
    for (b, *p), g in zip(reqs, got):
        if b % 2 == 0:
            sent = next(q[3] for q in subs[b]["phichs"] if q[:3] == tuple(p))
            assert g.ack_value == sent, (spec, b, p)


@pytest.mark.parametrize("spec", [(25, 2, 31, False, 1, False, 2), (25, 1, 40, True, 3, False, 1), (50, 4, 9, True, 2, True, 2)])
def test_two_phichs_of_one_group_and_of_one_unit(spec):
    """Opposite acks on two sequences of one group, and (extended CP) on the two groups 2m, 2m + 1 of one mapping unit: both are read."""
    cell = UlCell(*spec)
    rng = np.random.default_rng(spec[2])
    ng = cell.ngroups()
    want = {"group": None, "unit": None}
    cand = [(lo, dm, ip) for lo in range(spec[0]) for dm in range(8) for ip in range(2 if spec[3] else 1)]
    calc = {c: cell.calc(*c) for c in cand}
    calc = {c: v for c, v in calc.items() if v[0] < ng}
    for a in calc:
        for b in calc:
            if want["group"] is None and calc[a][0] == calc[b][0] and calc[a][1] != calc[b][1]:
                want["group"] = (a, b)
            if spec[3] and want["unit"] is None and calc[a][0] // 2 == calc[b][0] // 2 and calc[a][0] % 2 == 0 and calc[b][0] % 2 == 1:
                want["unit"] = (a, b)
    ctrl = _ctrl(spec, 1, 4)
    for kind, pair in want.items():
        if pair is None:
            assert kind == "unit" and not spec[3]
            continue
        for acks in ((0, 1), (1, 0)):
            tti = int(rng.integers(0, 10240))
            tx = cell.encode_full(tti, 2, [], [pair[0] + (acks[0],), pair[1] + (acks[1],)])
            y, ce, noise = channel(cell, tx, 30.0, rng)
            sub = [dict(y=y, ce=ce, noise=noise)]
            rc, got = ctrl.phich(*_stack(sub), tti, [(0,) + pair[0], (0,) + pair[1]])
            assert rc == 0
            for g, p, a in zip(got, pair, acks):
                r = cell.phich_decode_full(tti, y, ce, noise, *p)
                assert (g.ngroup, g.nseq, g.ack_value) == (r["ngroup"], r["nseq"], a) and r["ack"] == a and _close(g.distance, r["distance"]), (kind, p, a)
    ctrl.free()


def _check_ul(cell, s, out, msg, ul, ulm, tag):
    cell.extract(s["tti"], out.cfi, s["y"], s["ce"], s["noise"])
    dl, want, pend = ul_search(cell, s["tti"], out.cfi, s["rnti"], s["tm"])
    assert (ul.nof_ul_dci, ul.pending) == (len(want), pend), (tag, ul.nof_ul_dci, ul.pending, len(want), pend)
    for d, m in zip(ulm, want):
        assert (d.nof_bits, d.L, d.ncce, d.format, d.rnti) == (m.nof_bits, m.L, m.ncce, F0, m.rnti), tag
        assert bytes(d.payload[:d.nof_bits + 16]) == bytes(m.payload[:m.nof_bits + 16]), tag
    m = blind_search(cell, s["tti"], out.cfi, s["rnti"], s["tm"])
    assert out.nof_dci == (1 if m is not None else 0), tag
    if is_crnti(s["rnti"]):
        assert (m is None) == (dl is None), tag
    return len(want), pend


@pytest.mark.parametrize("idx", range(len(CELLS)))
def test_ul_dcis_against_the_restated_search(idx):
    spec = CELLS[idx]
    cell = UlCell(*spec)
    rng = np.random.default_rng(5000 + idx)
    nof_sf, tti0 = 20, int(rng.integers(0, 10240))
    subs, reqs = [], []
    for b in range(nof_sf):
        tti, cfi, tm = tti0 + b, 1 + int(rng.integers(0, 3)), int(rng.integers(0, 4))
        rnti = SIRNTI if b == 7 else 0 if b == 13 else int(rng.integers(0x0B, 0xFFF3))
        msgs = draw_ul_subframe(cell, tti, cfi, rnti if rnti not in (0, SIRNTI) else 0x1234, tm, rng)
        y, ce, noise = channel(cell, cell.encode(tti, cfi, msgs), (30.0, 30.0, 4.0)[b % 3], rng)
        subs.append(dict(tti=tti, rnti=rnti, tm=tm, y=y, ce=ce, noise=noise))
        reqs.append(pkg.DlCtrlReq(rnti, tm, cfi if b % 4 == 3 else 0, 0))
    ctrl = _ctrl(spec, nof_sf)
    rc, out, msg, ul, ulm, ph = ctrl.batch_ul(*_stack(subs), tti0, reqs)
    ctrl.free()
    assert rc == 0 and ph == []
    found = pending = 0
    for b, s in enumerate(subs):
        n, p = _check_ul(cell, s, out[b], msg[b], ul[b], ulm[b], (spec, b))
        found += n
        pending += p
    assert ul[7].nof_ul_dci == 0 and ul[13].nof_ul_dci == 0
    assert found >= 8 and pending >= 3, (found, pending)


@pytest.mark.parametrize("spec", [(25, 1, 89, False, 2, False, 1), (100, 2, 5, False, 2, False, 2)])
def test_hand_built_ul_cases_on_the_device(spec):
    cell = UlCell(*spec)
    rng = np.random.default_rng(11)
    tti, cfi, tm = 4017, 3, 1
    cases = hand_cases(cell, tti, cfi, tm, rng)
    ctrl = _ctrl(spec, 1)
    for name, rnti, msgs, (nof_ul, pending, dl_found) in cases:
        y, ce, noise = channel(cell, cell.encode(tti, cfi, msgs), 30.0, rng)
        s = dict(tti=tti, rnti=rnti, tm=tm, y=y, ce=ce, noise=noise)
        rc, out, msg, ul, ulm, _ = ctrl.batch_ul(*_stack([s]), tti, [pkg.DlCtrlReq(rnti, tm, 0, 0)])
        assert rc == 0 and (ul[0].nof_ul_dci, ul[0].pending, out[0].nof_dci) == (nof_ul, pending, int(dl_found)), (name, ul[0].nof_ul_dci, ul[0].pending)
        _check_ul(cell, s, out[0], msg[0], ul[0], ulm[0], name)
        for d in ulm[0]:
            want = next(t for t in msgs if t.format == F0)
            assert bytes(d.payload[:d.nof_bits]) == bytes(want.payload[:want.nof_bits]), name
    ctrl.free()


def _drawn_batch(spec, nof_sf, seed, nof_phich):
    """nof_sf subframes (drawn once for ten TTIs and repeated) with UL and DL DCIs and PHICHs; nof_phich requests spread over them."""
    cell = UlCell(*spec)
    rng = np.random.default_rng(seed)
    tti0, base = 10 * int(rng.integers(0, 1024)), []
    for b in range(10):
        cfi, tm, rnti = 1 + b % 3, b % 4, int(rng.integers(0x0B, 0xFFF3))
        msgs = draw_ul_subframe(cell, tti0 + b, cfi, rnti, tm, rng)
        phichs = [(int(rng.integers(0, spec[0])), int(rng.integers(0, 8)), 0, int(rng.integers(0, 2))) for _ in range(4)]
        y, ce, noise = channel(cell, cell.encode_full(tti0 + b, cfi, msgs, phichs), 25.0, rng)
        base.append(dict(rnti=rnti, tm=tm, y=y, ce=ce, noise=noise, phichs=phichs))
    subs = [dict(base[b % 10], tti=tti0 + b) for b in range(nof_sf)]
    reqs = [pkg.DlCtrlReq(s["rnti"], s["tm"], 0, 0) for s in subs]
    ph = []
    for i in range(nof_phich):
        b = int(rng.integers(0, nof_sf))
        ph.append((b,) + subs[b]["phichs"][i % 4][:3])
    return cell, tti0, subs, reqs, ph


def _raw(ctrl, bufs, tti0, reqs, ph, ul=True, stream=None, pinned=False):
    """One call on device buffers -> bytes of (out, msg, ul_out, ul_msg, phich_res); a poison pattern where nothing was written."""
    import torch
    n, m = len(reqs), max(1, len(ph))
    sizes = [C.sizeof(pkg.DlCtrlRes) * n, C.sizeof(pkg.DciMsg) * n, C.sizeof(pkg.DlCtrlUlRes) * n, C.sizeof(pkg.DciMsg) * n * pkg.DL_CTRL_MAX_UL_DCI,
             C.sizeof(pkg.PhichRes) * m]
    if pinned:
        outs = [torch.full((sz,), 0xA5, dtype=torch.uint8).pin_memory() for sz in sizes]
        ptrs = [t.data_ptr() for t in outs]
    else:
        outs = [pkg.DevBuf.from_host(np.full(sz, 0xA5, np.uint8)) for sz in sizes]
        ptrs = [t.ptr for t in outs]
    if ul:
        rc = ctrl.batch_ul_device(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, tti0, reqs, ptrs[0], ptrs[1], ptrs[2], ptrs[3], ph, ptrs[4], stream)
    else:
        rc = ctrl.run_device(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, tti0, reqs, ptrs[0], ptrs[1], stream)
    pkg.sync()
    return rc, [t.numpy().tobytes() if pinned else t.to_host(np.uint8).tobytes() for t in outs]


def _bufs(subs):
    g, h, r = _stack(subs)
    return pkg.DevBuf.from_host(np.ascontiguousarray(g, np.complex64)), pkg.DevBuf.from_host(np.ascontiguousarray(h, np.complex64)), pkg.DevBuf.from_host(r)


def test_dl_outputs_untouched_chunk_edges_streams_and_pinned_results():
    """d_out / d_msg of batch_ul equal srslte_hip_dl_ctrl_batch's byte for byte, with and without PHICH requests; a batch equals single calls
    at nof_sf 1, 128, 129 and 0, 1, 2049 PHICH requests; two objects on two streams; results in pinned host memory."""
    spec = (25, 2, 31, False, 1, False, 2)
    L = pkg.lib()
    singles = {}
    for nof_sf, nof_phich in ((1, 0), (1, 1), (128, 2049), (129, 1), (129, 2049)):
        cell, tti0, subs, reqs, ph = _drawn_batch(spec, nof_sf, 77, nof_phich)
        bufs = _bufs(subs)
        ctrl = _ctrl(spec, nof_sf, nof_phich)
        rc0, dl = _raw(ctrl, bufs, tti0, reqs, [], ul=False)
        rc1, a = _raw(ctrl, bufs, tti0, reqs, ph)
        rc2, b = _raw(ctrl, bufs, tti0, reqs, [])
        assert (rc0, rc1, rc2) == (0, 0, 0)
        assert a[0] == dl[0] and a[1] == dl[1] and b[0] == dl[0] and b[1] == dl[1], (nof_sf, nof_phich)
        assert a[2] == b[2] and a[3] == b[3] and b[4] == b"\xa5" * len(b[4])
        # the PHICH part alone gives the same results
        if nof_phich:
            dph = pkg.DevBuf(C.sizeof(pkg.PhichRes) * nof_phich)
            assert ctrl.phich_device(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, tti0, nof_sf, ph, dph.ptr) == 0
            pkg.sync()
            assert dph.to_host(np.uint8).tobytes() == a[4]
        # single calls: subframe b alone (its TTI, its request, its PHICHs) on a one-subframe object
        one = _ctrl(spec, 1, 64)
        ul_res = np.frombuffer(a[2], np.uint32).reshape(nof_sf, 2)
        ul_msg = np.frombuffer(a[3], np.uint8).reshape(nof_sf, -1)
        ph_res = np.frombuffer(a[4], np.uint8).reshape(max(1, nof_phich), -1)
        for sb in sorted({0, nof_sf // 2, min(127, nof_sf - 1), nof_sf - 1}):  # 127: the last subframe of the first chunk
            key = (sb % 10)
            mine = [i for i, p in enumerate(ph) if p[0] == sb][:64]
            sbuf = _bufs([subs[sb]])
            rc, s = _raw(one, sbuf, tti0 + sb, [reqs[sb]], [(0,) + ph[i][1:] for i in mine])
            assert rc == 0
            assert s[2] == ul_res[sb].tobytes() and s[3] == ul_msg[sb].tobytes(), (nof_sf, sb)
            for k, i in enumerate(mine):
                assert s[4][16 * k:16 * k + 16] == ph_res[i].tobytes(), (nof_sf, sb, i)
            singles[key] = s[2]
        one.free()
        ctrl.free()
    assert len(set(singles.values())) > 1  # the drawn subframes do differ in their UL results: the comparisons above are not of one constant
    # two objects on two streams, results in pinned host memory
    cell, tti0, subs, reqs, ph = _drawn_batch(spec, 40, 78, 100)
    bufs = _bufs(subs)
    c1, c2 = _ctrl(spec, 40, 100), _ctrl(spec, 40, 100)
    s1, s2 = L.srslte_hip_stream_create(), L.srslte_hip_stream_create()
    rc, want = _raw(c1, bufs, tti0, reqs, ph)
    assert rc == 0
    import torch
    sizes = [len(w) for w in want]
    pins = [[torch.full((sz,), 0xA5, dtype=torch.uint8).pin_memory() for sz in sizes] for _ in range(2)]
    for _ in range(3):
        for c, st, pin in ((c1, s1, pins[0]), (c2, s2, pins[1])):
            p = [t.data_ptr() for t in pin]
            assert c.batch_ul_device(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, tti0, reqs, p[0], p[1], p[2], p[3], ph, p[4], st) == 0
    L.srslte_hip_stream_sync(s1)
    L.srslte_hip_stream_sync(s2)
    for pin in pins:
        assert [t.numpy().tobytes() for t in pin] == want
    L.srslte_hip_stream_destroy(s1)
    L.srslte_hip_stream_destroy(s2)
    c1.free()
    c2.free()


def test_refusals_leave_the_results_unwritten():
    spec = (25, 1, 40, True, 3, False, 1)  # extended CP: I_phich 1 names a group
    cell, tti0, subs, reqs, ph = _drawn_batch(spec, 2, 79, 2)
    bufs = _bufs(subs)
    ctrl = _ctrl(spec, 2, 4)
    ng = cell.ngroups()
    ok_ip1 = next((lo, dm, 1) for lo in range(25) for dm in range(8) if cell.calc(lo, dm, 1)[0] < ng)
    rc, good = _raw(ctrl, bufs, tti0, reqs, ph + [(1,) + ok_ip1])
    assert rc == 0 and all(g != b"\xa5" * len(g) for g in good)
    poison = lambda r: all(x == b"\xa5" * len(x) for x in r)  # noqa: E731
    bad_req = [pkg.DlCtrlReq(0x4601, 1, 0, 1), pkg.DlCtrlReq(0x4601, 4, 0, 0), pkg.DlCtrlReq(0x4601, 1, 4, 0)]
    for br in bad_req:
        rc, r = _raw(ctrl, bufs, tti0, [reqs[0], br], ph)
        assert rc == BAD and poison(r)
    for bad_ph in ([(2, 0, 0, 0)], [(0, 0, 0, 2)], [(0, 0, 0, 0)] * 5):  # sf >= nof_sf, I_phich beyond any group, more than the capacity
        rc, r = _raw(ctrl, bufs, tti0, reqs, bad_ph)
        assert rc == BAD and poison(r), bad_ph
        dph = pkg.DevBuf.from_host(np.full(16 * len(bad_ph), 0xA5, np.uint8))
        assert ctrl.phich_device(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, tti0, 2, bad_ph, dph.ptr) == BAD
        pkg.sync()
        assert dph.to_host(np.uint8).tobytes() == b"\xa5" * (16 * len(bad_ph))
    rc, r = _raw(ctrl, bufs, tti0, reqs * 2, ph)  # nof_sf beyond max_batch
    assert rc == BAD and poison(r)
    assert ctrl.batch_ul_device(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, tti0, reqs, None, None, None, None, ph, None) == BAD
    assert ctrl.phich_device(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, tti0, 2, ph, None) == BAD
    assert ctrl.phich_device(None, bufs[1].ptr, bufs[2].ptr, tti0, 2, ph, None) == BAD
    ctrl.free()
    # normal CP: I_phich 1 names no group; an object without capacity takes no PHICH request
    spec2 = (25, 2, 31, False, 1, False, 2)
    cell, tti0, subs, reqs, ph = _drawn_batch(spec2, 1, 80, 1)
    bufs = _bufs(subs)
    ctrl = _ctrl(spec2, 1, 4)
    rc, r = _raw(ctrl, bufs, tti0, reqs, [(0, 3, 1, 1)])
    assert rc == BAD and poison(r)
    ctrl.free()
    ctrl = _ctrl(spec2, 1, 0)
    rc, r = _raw(ctrl, bufs, tti0, reqs, ph)
    assert rc == BAD and poison(r)
    rc, r = _raw(ctrl, bufs, tti0, reqs, [])
    assert rc == 0
    ctrl.free()


@pytest.mark.parametrize("spec", [(25, 2, 31, False, 1, False, 2), (25, 1, 40, True, 3, False, 1)])
def test_an_exact_tie_reads_as_nack(spec):
    """An empty grid gives z = 0 and two equal correlations: srslte_phich_ack_decode takes the second only if it is strictly greater, so the
    reference reads ack 0, and so does the device."""
    cell = UlCell(*spec)
    y = [np.zeros(cell.glen, np.complex64) for _ in range(spec[6])]
    ce = np.ones((spec[1], spec[6], cell.glen), np.complex64)
    ctrl = _ctrl(spec, 1, 4)
    rc, got = ctrl.phich(*_stack([dict(y=y, ce=ce, noise=0.1)]), 7, [(0, 3, 1, 0), (0, 0, 0, 0)])
    ctrl.free()
    assert rc == 0
    for g, p in zip(got, ((3, 1, 0), (0, 0, 0))):
        r = cell.phich_decode_full(7, y, ce, 0.1, *p)
        assert r["ack"] == 0 and r["distance"] == 0.0 and (g.ack_value, g.distance) == (0, 0.0), (p, g.ack_value, g.distance, r)


# ---------------------------------------------------------------- the closed uplink HARQ loop
RV_SEQ = (0, 2, 3, 1)  # the redundancy versions of non-adaptive retransmissions (36.321 5.4.2.2)


def _ul_tbs(cell, mcs, L_prb):
    """Modulation and transport block size of a format-0 MCS 0-10 (36.213 Table 8.6.1-1: QPSK, I_TBS = I_MCS) by srslte_ra_tbs_from_idx; this
    part of srslte_ra_ul_dci_to_grant (ra_ul.c is not in the reference library of the tests) is restated, the DCI unpacking is the reference's."""
    assert mcs <= 10
    cell.R.srslte_ra_tbs_from_idx.argtypes = [C.c_uint32, C.c_uint32]
    return 1, cell.R.srslte_ra_tbs_from_idx(mcs, L_prb)


def _one_block(tbs):
    rc, s = pkg.cbsegm(tbs)
    return rc == 0 and tbs > 0 and tbs % 8 == 0 and s.F == 0 and s.C2 == 0


@pytest.mark.parametrize("nof_prb,cfi", [(25, 3), (100, 2)])
def test_closed_uplink_harq_loop(nof_prb, cfi):
    """Three UEs, six DL batches of three subframes eight TTIs apart (UE u is served in subframe u of each), the eNB and the UE side both on
    the device: srslte_hip_dl_tx_batch_grants_full sends format-0 DCIs packed by the reference's srslte_dci_msg_pack_pusch and, from the
    second batch on, the PHICHs of the PUSCHs received four TTIs earlier -> OFDM receive + chest_dl -> srslte_hip_dl_ctrl_batch_ul finds the
    DCIs and reads the PHICHs in one call -> the reference's srslte_dci_msg_unpack_pusch gives back what was packed -> srslte_hip_ul_tx_batch_grants
    sends the PUSCHs four TTIs later -> noise (15 dB per RE for UE 0, 1 dB for UEs 1 and 2, whose rate-0.6 QPSK blocks cannot pass at that in
    one transmission) -> srslte_hip_ul_rx_batch_grants -> its CRC verdicts are the next batch's PHICHs. A NACKed UE retransmits the block
    with the next redundancy version without a DCI, an ACKed one gets a DCI with the NDI toggled and sends new data (while the schedule
    leaves room for three transmissions). Every block arrives, every ack the UE read equals the verdict the eNB formed, and NACKs occurred.
    The samples pass through the host between the two sides, where the noise is added; no control decision is taken there."""
    from test_gpu_dl_ctrl import _front
    cell_id, K, t0 = 2 * nof_prb + 1, 6, 16
    cell = UlCell(nof_prb, 1, cell_id, False, 1, False, 1)
    rng = np.random.default_rng(nof_prb)
    ncce = cell.ncce[cfi - 1]
    ues = []
    for u, (L_prb, n_prb, n_dmrs, snr_re) in enumerate(((6, 1, 0, 15.0), (8, 8, 3, 1.0), (5, 18, 6, 1.0))):
        mcs = next(m for m in (10, 9, 8, 7) if _one_block(_ul_tbs(cell, m, L_prb)[1]))
        ues.append(dict(rnti=0x4600 + 17 * u, L_prb=L_prb, n_prb=n_prb, n_dmrs=n_dmrs, mcs=mcs, snr_re=snr_re, ndi=0, data=None, ntx=0, grant=None,
                        pending_ack=None, sent=[], arrived=0))
    tbs_max = max(_ul_tbs(cell, ue["mcs"], ue["L_prb"])[1] for ue in ues)
    dm = dict(cyclic_shift=1, delta_ss=3, group_hopping=False, sequence_hopping=False)
    # slot p of a receiver is the soft buffer of row p of its grant list: one receiver per UE keeps each UE's HARQ process in slot 0 whoever else
    # is scheduled
    enb_rx = [pkg.UlRx(cell_id, nof_prb, 0x1234, 1, tbs_max, 6, 0, 0, 6, 3, max_grants=1, **dm) for _ in ues]
    ue_tx = pkg.UlTx(cell_id, nof_prb, 0x1234, 1, tbs_max, 6, 0, 0, 3, max_grants=3, **dm)
    # a small PDSCH for another RNTI in subframe 0 of every batch, so that the DL subframes are complete ones
    dl_tbs = next(t for t in (_ul_tbs(cell, m, 4)[1] for m in range(10, 0, -1)) if _one_block(t))
    mask = np.zeros((2, nof_prb), bool)
    mask[:, :4] = True
    enb_tx = pkg.DlTx(cell_id, nof_prb, cfi, 0x1234, 1, dl_tbs, 3, 1, max_grants=1)
    enb_ctrl = pkg.DlCtrlTx(nof_prb, 1, cell_id, phich_resources=1, max_batch=3, max_dci=3, max_phich=3)
    ue_ctrl = pkg.DlCtrl(nof_prb, 1, cell_id, phich_resources=1, max_batch=3, max_phich=3)
    symsz = pkg.symbol_sz(nof_prb)
    nacks = acks = round_trips = 0
    for k in range(K):
        tti0 = t0 + 8 * k
        # eNB: PHICHs for the PUSCHs of the last batch, DCIs for the UEs that start a new block
        dcis, phichs, packed = [], [], {}
        for u, ue in enumerate(ues):
            if ue["pending_ack"] is not None:
                phichs.append((u, ue["n_prb"], ue["n_dmrs"], 0, ue["pending_ack"]))
            idle = ue["pending_ack"] is None or ue["pending_ack"] == 1
            if idle and k <= K - 4:
                L, n0 = next((l, n) for l, n in pkg.pdcch_ue_locations(ncce, (tti0 + u) % 10, ue["rnti"]) if l >= 2)
                ndi = ue["ndi"] ^ 1
                packed[u] = dict(rnti=ue["rnti"], L_prb=ue["L_prb"], n_prb=ue["n_prb"], mcs=ue["mcs"], ndi=ndi, n_dmrs=ue["n_dmrs"])
                dcis.append((u, cell.pack_pusch(ue["rnti"], L, n0, ue["L_prb"], ue["n_prb"], ue["mcs"], ndi, ue["n_dmrs"])))
        pdsch = [(0, pkg.DlGrant.make(nof_prb, 1, dl_tbs, 0x0777, cfi=cfi, prb_mask=mask))]
        rc, time = enb_tx.encode_grants_full([rng.integers(0, 256, dl_tbs // 8, dtype=np.uint8)], tti0, 3, pdsch, enb_ctrl, [cfi] * 3, dcis, phichs)
        assert rc == 0
        iq = time[:, :1, :] * (0.8 * np.exp(0.4j))
        sigma = 10 ** (-30 / 20) * np.sqrt(np.mean(np.abs(iq) ** 2))
        iq = (iq + sigma / np.sqrt(2) * (rng.normal(size=iq.shape) + 1j * rng.normal(size=iq.shape))).astype(np.complex64)
        # UE: one call for the DL search, the UL DCIs and the PHICHs of the three subframes
        d_grid, d_ce, d_res, _ = _front(nof_prb, 1, cell_id, iq, tti0)
        reqs = [pkg.DlCtrlReq(ue["rnti"], 0, 0, 0) for ue in ues]
        ph_req = [p[:4] for p in phichs]
        n = 3
        bufs = [pkg.DevBuf(C.sizeof(pkg.DlCtrlRes) * n), pkg.DevBuf(C.sizeof(pkg.DciMsg) * n), pkg.DevBuf(C.sizeof(pkg.DlCtrlUlRes) * n),
                pkg.DevBuf(C.sizeof(pkg.DciMsg) * n * pkg.DL_CTRL_MAX_UL_DCI), pkg.DevBuf(C.sizeof(pkg.PhichRes) * 3)]
        assert ue_ctrl.batch_ul_device(d_grid.ptr, d_ce.ptr, d_res.ptr, tti0, reqs, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, ph_req, bufs[4].ptr) == 0
        pkg.sync()
        out, ul, ulm, phr = (pkg.DlCtrlRes * n)(), (pkg.DlCtrlUlRes * n)(), (pkg.DciMsg * (n * pkg.DL_CTRL_MAX_UL_DCI))(), (pkg.PhichRes * 3)()
        for dst, src in ((out, bufs[0]), (ul, bufs[2]), (ulm, bufs[3]), (phr, bufs[4])):
            pkg.lib().srslte_hip_memcpy_d2h(C.addressof(dst), src.ptr, C.sizeof(dst))
        read = {p[0]: int(phr[i].ack_value) for i, p in enumerate(phichs)}
        for u, ue in enumerate(ues):
            assert out[u].cfi == cfi and out[u].nof_dci == 0, (k, u)
            # the ack the UE read is the verdict the eNB formed
            if ue["pending_ack"] is not None:
                assert read[u] == ue["pending_ack"], (k, u, read[u], ue["pending_ack"], phr[[p[0] for p in phichs].index(u)].distance)
                round_trips += 1
                if read[u]:
                    acks += 1
                    ue["arrived"] += 1
                    ue["grant"] = None
                else:
                    nacks += 1
                ue["pending_ack"] = None
            # the UL DCI, unpacked by the reference, is what the reference packed
            assert ul[u].nof_ul_dci == (1 if u in packed else 0), (k, u, ul[u].nof_ul_dci)
            if u in packed:
                got = cell.unpack_pusch(ulm[u * pkg.DL_CTRL_MAX_UL_DCI])
                assert got is not None and {f: got[f] for f in packed[u]} == packed[u] and got["hop"] == -1, (k, u, got, packed[u])
                assert got["ndi"] != ue["ndi"]  # toggled: new data
                mod, tbs = _ul_tbs(cell, got["mcs"], got["L_prb"])
                ue.update(ndi=got["ndi"], ntx=0, data=rng.integers(0, 256, tbs // 8, dtype=np.uint8),
                          grant=dict(L_prb=got["L_prb"], n_prb=got["n_prb"], n_dmrs=got["n_dmrs"], mod=mod, tbs=tbs))
                ue["sent"].append(ue["data"])
        if k == K - 1:
            break
        # UE: the PUSCHs four TTIs later (new data, or the next redundancy version of a NACKed block); eNB: receive, verdicts
        active = [u for u, ue in enumerate(ues) if ue["grant"] is not None]
        if not active:
            continue
        grants = []
        for u in active:
            ue, g = ues[u], ues[u]["grant"]
            grants.append(pkg.UlGrant.make(u, ue["rnti"], g["L_prb"], g["n_prb"], g["mod"], g["tbs"], n_dmrs=g["n_dmrs"], rv=RV_SEQ[ue["ntx"] % 4],
                                           new_data=ue["ntx"] == 0))
        x = ue_tx.encode_grants([ues[u]["data"] for u in active], tti0 + 4, 3, grants).astype(np.complex64).copy()
        for u in active:
            p_re = np.mean(np.abs(x[u]) ** 2) * symsz / (12 * ues[u]["grant"]["L_prb"])  # per occupied RE
            s = np.sqrt(p_re / 10 ** (ues[u]["snr_re"] / 10) / 2)
            x[u] += (s * (rng.standard_normal(x.shape[1]) + 1j * rng.standard_normal(x.shape[1]))).astype(np.complex64)
        for p_, u in enumerate(active):
            ue = ues[u]
            tb, ok = enb_rx[u].decode_grants(x, tti0 + 4, [grants[p_]])
            ue["pending_ack"] = int(ok[0])
            ue["ntx"] += 1
            if ok[0]:
                assert np.array_equal(tb[0][:len(ue["data"])], ue["data"]), (k, u)
    for m in enb_rx + [ue_tx, enb_tx, enb_ctrl, ue_ctrl]:
        m.free()
    print("closed loop %d PRB: %d round trips, %d ACKs, %d NACKs, blocks per UE %s" % (nof_prb, round_trips, acks, nacks, [len(ue["sent"]) for ue in ues]))
    for u, ue in enumerate(ues):
        assert ue["grant"] is None and ue["pending_ack"] is None and ue["arrived"] == len(ue["sent"]) >= 1, (u, ue["arrived"], len(ue["sent"]))
    assert nacks >= 1 and acks >= 3 and round_trips >= 2 * 3 and len(ues[0]["sent"]) >= 2
