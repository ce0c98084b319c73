"""The DL control region and broadcast of TDD cells on the device (srslte_hip_dl_ctrl_create_tdd, srslte_hip_dl_ctrl_tx_create_tdd) against
the reference's own functions in oracle/_ref/libsrslte_ref.so over the subframe's own srslte_regs_t (tests/dl_ctrl_tdd_ref.py): transmit
grids bit for bit, the receive chain (PCFICH, LLR rows, candidates, search), UL DCIs and PHICH, PSS / SSS at the TDD positions and the MIB, the
combined transmit calls, refusals, and calls in flight. Every batch covers every sf_idx."""
import ctypes as C
import importlib

import numpy as np
import pytest

from _libs import aligned, ref
from dl_ctrl_ref import F0, F1A, SIRNTI, blind_search, channel, make_msg
from dl_ctrl_tdd_ref import (TDD_CELLS, TddCell, draw_tdd_dcis, draw_tdd_phichs, draw_tdd_subframe, draw_tdd_ul_subframe, is_ul, max_cfi, sizeof,
                             tdd_phich_subframes)
from dl_ctrl_ul_ref import is_crnti, near_tie, ul_search

pkg = importlib.import_module("srslte-emane_amd")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(ref() is None, reason="oracle/_ref/libsrslte_ref.so is not built")]

BAD = pkg.SRSLTE_ERROR_INVALID_INPUTS


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _tx(spec, max_batch=10, max_dci=160, max_phich=128):
    return pkg.DlCtrlTx(spec[0], spec[1], spec[2], cp_ext=spec[3], phich_resources=spec[4], phich_ext=spec[5], max_batch=max_batch, max_dci=max_dci,
                        max_phich=max_phich, tdd_sf_config=spec[7])


def _rx(spec, max_batch, max_phich=0):
    return pkg.DlCtrl(spec[0], spec[1], spec[2], cp_ext=spec[3], phich_resources=spec[4], phich_ext=spec[5], nof_rx=spec[6], max_batch=max_batch,
                      max_phich=max_phich, tdd_sf_config=spec[7])


def _kw(spec):
    return dict(cp_ext=spec[3], phich_resources=spec[4], phich_ext=spec[5])


# ---------------------------------------------------------------- transmit
def _draw_tx(spec, seed, nof_sf=10):
    """A batch from a drawn tti0: per downlink subframe a CFI (at most 2 in subframes 1 and 6), DCIs and PHICHs and the reference's grids;
    uplink subframes get a CFI of 0 (not looked at) and nothing else."""
    cell = TddCell(*spec)
    rng = np.random.default_rng(seed)
    tti0 = int(rng.integers(0, 10240))
    cfi, dcis, phichs, want = [], [], [], []
    for b in range(nof_sf):
        tti = tti0 + b
        if is_ul(spec[7], tti % 10):
            cfi.append(0)
            want.append(None)
            continue
        c = 1 + int(rng.integers(0, max_cfi(tti % 10)))
        msgs = draw_tdd_dcis(cell, tti, c, rng, tries=int(rng.integers(2, 14)))
        ph = draw_tdd_phichs(cell, tti % 10, rng)
        want.append(cell.encode_full(tti, c, msgs, ph))
        cfi.append(c)
        dcis += [(b, m) for m in msgs]
        phichs += [(b,) + p for p in ph]
    return cell, tti0, cfi, dcis, phichs, want


def _control_res(spec, sf_idx, cfi, msgs):
    """The REs a control region with these DCIs writes in subframe sf_idx: PCFICH, every PHICH REG of the subframe's variant, the DCIs' CCEs."""
    a = spec[:3]
    re = [pkg.pcfich_re(*a, **_kw(spec))]
    for g in range(pkg.phich_ngroups_tdd(*a, spec[7], sf_idx, **_kw(spec))):
        re.append(pkg.phich_re_tdd(*a, spec[7], sf_idx, g, **_kw(spec)))
    pd = pkg.pdcch_re_tdd(*a, spec[7], sf_idx, cfi, **_kw(spec))
    for m in msgs:
        re.append(pd[36 * m.ncce:36 * (m.ncce + (1 << m.L))])
    return np.unique(np.concatenate(re))


@pytest.mark.parametrize("idx", range(len(TDD_CELLS)))
def test_transmit_is_bit_exact_and_touches_nothing_else(idx):
    spec = TDD_CELLS[idx]
    cell, tti0, cfi, dcis, phichs, want = _draw_tx(spec, 2100 + idx)
    assert {(tti0 + b) % 10 for b in range(10)} == set(range(10)) and len(dcis) > 0 and len(phichs) > 0
    shape = (10, spec[1], cell.glen)
    rng = np.random.default_rng(idx)
    pre = (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(np.complex64)
    tx = _tx(spec)
    rc0, zero = tx.put(np.zeros(shape, np.complex64), tti0, cfi, dcis, phichs)
    rc1, rand = tx.put(pre, tti0, cfi, dcis, phichs)
    tx.free()
    assert (rc0, rc1) == (0, 0)
    nul = 0
    for b in range(10):
        if want[b] is None:  # uplink: untouched entirely
            assert not zero[b].any() and np.array_equal(_bits(rand[b]), _bits(pre[b])), (spec, b)
            nul += 1
            continue
        assert np.array_equal(_bits(zero[b]), _bits(want[b])), (spec, b, np.flatnonzero(_bits(zero[b]) != _bits(want[b]))[:8])
        re = _control_res(spec, (tti0 + b) % 10, cfi[b], [m for s, m in dcis if s == b])
        exp = pre[b].copy()
        exp[:, re] = want[b][:, re]
        assert np.array_equal(_bits(rand[b]), _bits(exp)), (spec, b)
    assert nul == sum(is_ul(spec[7], s) for s in range(10))


# ---------------------------------------------------------------- receive
def _stack(subs):
    res = np.zeros((len(subs), 10), np.float32)
    res[:, 0] = [s["noise"] for s in subs]
    return np.stack([np.stack(s["y"]) for s in subs]), np.stack([s["ce"] for s in subs]), res


def _ul_sub(cell, tti, rng):
    """An uplink subframe as the receiver sees it: whatever is on the grid (here noise) must not be read."""
    y = [(rng.normal(size=cell.glen) + 1j * rng.normal(size=cell.glen)).astype(np.complex64) for _ in range(cell.nof_rx)]
    return dict(tti=tti, ul=True, y=y, ce=np.ones((cell.ports, cell.nof_rx, cell.glen), np.complex64), noise=1.0)


@pytest.mark.parametrize("idx", range(len(TDD_CELLS)))
def test_pcfich_llr_candidates_and_search(idx):
    """The TDD twin of tests/test_gpu_dl_ctrl.py::test_pcfich_llr_candidates_and_search."""
    spec = TDD_CELLS[idx]
    cell = TddCell(*spec)
    rng = np.random.default_rng(1100 + idx)
    nof_sf, tti0 = 10, int(rng.integers(0, 10240))
    kinds = ["ue", "ue", "ul", "none", "si1a", "si1c", "ue", "ue", "ue", "none"]
    subs, reqs = [], []
    for b in range(nof_sf):
        tti = tti0 + b
        sf_idx = tti % 10
        if is_ul(spec[7], sf_idx):
            subs.append(_ul_sub(cell, tti, rng))
            reqs.append(pkg.DlCtrlReq(int(rng.integers(0x0B, 0xFFF3)), 0, 0, 0))
            continue
        # subframes 1 and 6, special or (subframe 6 of configurations 3-5) normal downlink: the PCFICH says 3, which the receiver must read as 2
        cfi = 3 if sf_idx in (1, 6) else 1 + int(rng.integers(0, max_cfi(sf_idx)))
        use = min(cfi, max_cfi(sf_idx))  # the region the DCIs are placed in
        tm, kind = int(rng.integers(0, 4)), kinds[sf_idx]
        rnti = SIRNTI if kind.startswith("si") else int(rng.integers(0x0B, 0xFFF3))
        dcis, placed = draw_tdd_subframe(cell, tti, use, rnti, tm, rng, kind)
        tx = cell.encode(tti, use, dcis)
        if cfi != use:  # the PCFICH of CFI 3 over a two-symbol region
            pc = pkg.pcfich_re(*spec[:3], **_kw(spec))
            tx[:, pc] = cell.encode(tti, cfi, [])[:, pc]
        snr = (30.0, 2.0)[b % 2] if cfi == use else 30.0
        y, ce, noise = channel(cell, tx, snr, rng)
        given = use if b % 4 == 3 and cfi == use else 0
        subs.append(dict(tti=tti, ul=False, cfi=cfi, use=use, tm=tm, rnti=rnti, kind=kind, placed=placed, snr=snr, y=y, ce=ce, noise=noise))
        reqs.append(pkg.DlCtrlReq(rnti, tm, given, 0))
    ctrl = _rx(spec, nof_sf)
    assert ctrl.llr_stride == (cell.max_bits + 3) & ~3  # the largest list: mi = 0 at CFI 3
    rc, out, msgs = ctrl.batch(*_stack(subs), tti0, reqs)
    assert rc == 0
    llr, cands = ctrl.llr(nof_sf), ctrl.candidates(nof_sf)
    ctrl.free()
    found = clamped = 0
    for b, s in enumerate(subs):
        if s["ul"]:
            assert (out[b].cfi, out[b].cfi_corr, out[b].nof_dci, msgs[b].nof_bits) == (0, 0.0, 0, 0) and len(cands[b]) == 0 and not llr[b].any(), (spec, b)
            continue
        cfi_ref, corr_ref = cell.pcfich(s["tti"], s["y"], s["ce"], s["noise"])
        assert abs(out[b].cfi_corr - corr_ref) <= 1e-3 * max(1.0, abs(corr_ref)), (spec, b, out[b].cfi_corr, corr_ref)
        cfi = reqs[b].cfi or cfi_ref
        if s["tti"] % 10 in (1, 6):  # ue_dl.c:351-354
            assert cfi_ref == 3 and out[b].cfi == 2, (spec, b, cfi_ref, out[b].cfi)
            cfi = 2
            clamped += 1
        assert out[b].cfi == cfi, (spec, b, out[b].cfi, cfi_ref)
        if s["snr"] > 20:
            assert cfi_ref == s["cfi"] and cfi == s["use"], (spec, b)
        n = 72 * cell.ncce6[cell.mi_idx(s["tti"] % 10)][cfi - 1]
        want = cell.llr_chain(s["tti"], cfi, s["y"], s["ce"], s["noise"])
        assert want.size == n
        np.testing.assert_allclose(llr[b, :n], want, rtol=1e-4, atol=1e-4 * max(1.0, float(np.abs(want).max())), err_msg=str((spec, b)))
        assert not llr[b, n:].any()
        row = aligned(llr.shape[1], np.float32)
        row[:] = llr[b]
        for c in cands[b]:
            E = 72 << c.L
            assert c.nof_bits == cell.dci_sizeof(c.format) and c.ncce * 72 + E <= n, (spec, b, c.format)
            seg = row[c.ncce * 72:c.ncce * 72 + E].astype(np.float64)
            assert bool(c.skipped) == (not (np.abs(seg).sum() / E > 0.3)), (spec, b)
            if c.skipped:
                continue
            data, crc = np.zeros(256, np.uint8), C.c_uint16(0)
            assert cell.R.srslte_pdcch_dci_decode(cell.dec, row.ctypes.data + 4 * 72 * c.ncce, data.ctypes.data, E, c.nof_bits, C.byref(crc)) == 0
            assert c.crc_rem == crc.value, (spec, b, c.L, c.ncce, c.format)
            assert bytes(c.payload[:c.nof_bits + 16]) == data[:c.nof_bits + 16].tobytes(), (spec, b, c.L, c.ncce)
            if c.format in (F0, F1A):
                assert c.format_decoded == (F0 if data[0] == 0 else F1A)
        cell.extract(s["tti"], cfi, s["y"], s["ce"], s["noise"])
        m = blind_search(cell, s["tti"], cfi, s["rnti"], s["tm"])
        assert out[b].nof_dci == (1 if m is not None else 0), (spec, b, s["kind"], s["snr"])
        if m is not None:
            found += 1
            d = msgs[b]
            assert (d.nof_bits, d.L, d.ncce, d.format, d.rnti) == (m.nof_bits, m.L, m.ncce, m.format, m.rnti), (spec, b)
            assert bytes(d.payload[:d.nof_bits]) == bytes(m.payload[:m.nof_bits])
        else:
            assert msgs[b].nof_bits == 0
        if s["snr"] > 20 and s["kind"] in ("ue", "si1a", "si1c") and s["placed"]:
            assert m is not None, (spec, b, s["kind"])
        if s["kind"] in ("none", "ul"):
            assert m is None
    assert found >= 1 and clamped == 2, (found, clamped)  # configuration 0 has four downlink subframes; subframes 1 and 6 are clean and carry a DCI


# ---------------------------------------------------------------- UL DCIs and PHICH
def _close(a, b):
    return abs(a - b) <= 1e-3 * max(1.0, abs(b))


@pytest.mark.parametrize("idx", range(len(TDD_CELLS)))
def test_phich_against_the_reference(idx):
    """The TDD twin of tests/test_gpu_dl_ctrl_ul.py::test_phich_against_the_reference over two frames: every request on the subframe's own
    mapping units; in configuration 0 that includes I_phich = 1 (tests/test_dl_ctrl_tdd_host.py counts them and the near ties: 0 of 104)."""
    spec = TDD_CELLS[idx]
    cell, tti0, subs = tdd_phich_subframes(spec, 7000 + idx)
    reqs = [(b,) + p[:3] for b, s in enumerate(subs) for p in s["phichs"]]
    ctrl = _rx(spec, len(subs), max(1, len(reqs)))
    rc, got = ctrl.phich(*_stack(subs), tti0, reqs)
    assert rc == 0 and len(got) == len(reqs) >= 4  # configuration 5 has PHICH groups in subframe 8 alone
    soft = ctrl.phich_soft(len(reqs))
    ctrl.free()
    aside = 0
    for (b, *p), g, sv in zip(reqs, got, soft):
        s = subs[b]
        r = cell.phich_decode_full(s["tti"], s["y"], s["ce"], s["noise"], *p)
        assert (g.ngroup, g.nseq) == (r["ngroup"], r["nseq"]), (spec, b, p)
        assert _close(g.distance, r["distance"]), (spec, b, p, g.distance, r["distance"])
        for i in range(3):
            assert _close(sv.z[i][0], r["z"][i].real) and _close(sv.z[i][1], r["z"][i].imag) and _close(sv.bits[i], r["bits"][i]), (spec, b, p, i)
        if near_tie(r):
            aside += 1
        else:
            assert g.ack_value == r["ack"], (spec, b, p, g.distance, r["distance"])
    assert aside <= 0.01 * len(reqs)
    for (b, *p), g in zip(reqs, got):  # clean subframes (30 dB): the ack that was sent
        if b % 2 == 0:
            sent = next(q[3] for q in subs[b]["phichs"] if q[:3] == tuple(p))
            assert g.ack_value == sent, (spec, b, p)
    if idx == 0:
        assert sum(p[2] == 1 for _, *p in reqs) >= 3  # I_phich = 1 in the mi = 2 subframes of configuration 0


def test_two_phichs_in_one_unit_of_an_mi2_subframe():
    """Configuration 0, subframe 0 (mi = 2): opposite acks on two sequences of the second mapping unit, which only I_phich = 1 reaches."""
    spec = TDD_CELLS[0]
    cell = TddCell(*spec)
    rng = np.random.default_rng(3)
    cell.select(0)
    pair = [(lo, dm, 1) for lo, dm in ((0, 0), (0, 3))]
    assert cell.calc(*pair[0])[0] == cell.calc(*pair[1])[0] == 1 and cell.calc(*pair[0])[1] != cell.calc(*pair[1])[1]
    ctrl = _rx(spec, 1, 4)
    for tti in (4000, 4005):
        for acks in ((0, 1), (1, 0)):
            tx = cell.encode_full(tti, 2, [], [pair[0] + (acks[0],), pair[1] + (acks[1],)])
            y, ce, noise = channel(cell, tx, 30.0, rng)
            rc, got = ctrl.phich(*_stack([dict(y=y, ce=ce, noise=noise)]), tti, [(0,) + pair[0], (0,) + pair[1]])
            assert rc == 0
            for g, p, a in zip(got, pair, acks):
                r = cell.phich_decode_full(tti, y, ce, noise, *p)
                assert (g.ngroup, g.nseq, g.ack_value) == (r["ngroup"], r["nseq"], a) and r["ack"] == a and _close(g.distance, r["distance"]), (tti, p, a)
    # the same requests in subframe 1 (mi = 1) name no group
    rc, got = ctrl.phich(*_stack([dict(y=y, ce=ce, noise=noise)]), 4001, [(0,) + pair[0]])
    assert rc == BAD
    ctrl.free()


@pytest.mark.parametrize("idx", range(len(TDD_CELLS)))
def test_ul_dcis_against_the_restated_search(idx):
    """The TDD twin of tests/test_gpu_dl_ctrl_ul.py::test_ul_dcis_against_the_restated_search: formats 0 and 1A share the TDD size, so the UL
    search still reads the candidates the 1A search decoded."""
    spec = TDD_CELLS[idx]
    cell = TddCell(*spec)
    rng = np.random.default_rng(5100 + idx)
    nof_sf, tti0 = 20, int(rng.integers(0, 10240))
    subs, reqs = [], []
    for b in range(nof_sf):
        tti = tti0 + b
        if is_ul(spec[7], tti % 10):
            subs.append(_ul_sub(cell, tti, rng))
            reqs.append(pkg.DlCtrlReq(0x4601, 1, 0, 0))
            continue
        cfi, tm = 1 + int(rng.integers(0, max_cfi(tti % 10))), int(rng.integers(0, 4))
        rnti = SIRNTI if b == 0 else int(rng.integers(0x0B, 0xFFF3))
        msgs = draw_tdd_ul_subframe(cell, tti, cfi, rnti if rnti != SIRNTI else 0x1234, tm, rng)
        y, ce, noise = channel(cell, cell.encode(tti, cfi, msgs), (30.0, 30.0, 4.0)[b % 3], rng)
        subs.append(dict(tti=tti, ul=False, rnti=rnti, tm=tm, y=y, ce=ce, noise=noise))
        reqs.append(pkg.DlCtrlReq(rnti, tm, cfi if b % 4 == 3 else 0, 0))
    ctrl = _rx(spec, nof_sf)
    rc, out, msg, ul, ulm, ph = ctrl.batch_ul(*_stack(subs), tti0, reqs)
    ctrl.free()
    assert rc == 0 and ph == []
    found = 0
    for b, s in enumerate(subs):
        if s["ul"]:
            assert (out[b].cfi, out[b].nof_dci, ul[b].nof_ul_dci, ul[b].pending, msg[b].nof_bits) == (0, 0, 0, 0, 0) and ulm[b] == [], (spec, b)
            continue
        cell.extract(s["tti"], out[b].cfi, s["y"], s["ce"], s["noise"])
        dl, want, pend = ul_search(cell, s["tti"], out[b].cfi, s["rnti"], s["tm"])
        assert (ul[b].nof_ul_dci, ul[b].pending) == (len(want), pend), (spec, b, ul[b].nof_ul_dci, ul[b].pending, len(want), pend)
        for d, m in zip(ulm[b], want):
            assert (d.nof_bits, d.L, d.ncce, d.format, d.rnti) == (m.nof_bits, m.L, m.ncce, F0, m.rnti), (spec, b)
            assert d.nof_bits == sizeof(cell, F0) == cell.dci_sizeof(F0)
            assert bytes(d.payload[:d.nof_bits + 16]) == bytes(m.payload[:m.nof_bits + 16]), (spec, b)
        m = blind_search(cell, s["tti"], out[b].cfi, s["rnti"], s["tm"])
        assert out[b].nof_dci == (1 if m is not None else 0), (spec, b)
        if is_crnti(s["rnti"]):
            assert (m is None) == (dl is None), (spec, b)
        found += len(want)
    assert found >= 4, found


# ---------------------------------------------------------------- broadcast
@pytest.mark.parametrize("spec", [TDD_CELLS[0], TDD_CELLS[3], TDD_CELLS[2]])
def test_pss_sss_at_the_tdd_positions_and_the_mib(spec):
    """PSS on symbol 2 of subframes 1 and 6, SSS (signal0 / signal5) on the last symbol of subframes 0 and 5, each with its five zero guards,
    the reference's values; the PBCH where it is in FDD; nothing else written. The MIB of the batch is decoded by srslte_hip_dl_ctrl_mib_batch."""
    from dl_bcast_ref import BcastCell
    nof_prb, ports, cell_id, cp_ext = spec[:4]
    bc = BcastCell(nof_prb, ports, cell_id, cp_ext, spec[4], spec[5])
    glen, w, nsym = bc.glen, 12 * nof_prb, 6 if cp_ext else 7
    tti0 = 10 * 37 + 8  # subframes 8, 9, 0 .. 7
    rng = np.random.default_rng(cell_id)
    pre = (rng.normal(size=(10, ports, glen)) + 1j * rng.normal(size=(10, ports, glen))).astype(np.complex64)
    tx = _tx(spec)
    rc, got = tx.put_bcast(pre, tti0)
    rc0, clean = tx.put_bcast(np.zeros_like(pre), tti0)
    tx.free()
    assert rc == 0 and rc0 == 0
    pss, (s0, s5) = bc.pss(), bc.sss()
    k_pss, k_sss = 2 * w + w // 2 - 36, (2 * nsym - 1) * w + w // 2 - 36
    for b in range(10):
        sf_idx = (tti0 + b) % 10
        exp = pre[b].copy()
        if sf_idx in (1, 6):
            exp[:, k_pss:k_pss + 72] = 0
            exp[:, k_pss + 5:k_pss + 67] = pss
        if sf_idx in (0, 5):
            exp[:, k_sss:k_sss + 72] = 0
            exp[:, k_sss + 5:k_sss + 67] = s5 if sf_idx else s0
        if sf_idx == 0:  # the PBCH of the FDD position: srslte_pbch_encode over the reference's RE list
            fdd = bc.encode(tti0 + b)
            re = bc.pbch_put_re()
            exp[:, re] = fdd[:, re]
        assert np.array_equal(_bits(got[b]), _bits(exp)), (spec, b, sf_idx)
    # the MIB: the clean batch through a unit channel
    y = clean.sum(axis=1)[:, None, :].repeat(spec[6], axis=1).astype(np.complex64)
    ce = np.ones((10, ports, spec[6], glen), np.complex64)
    res = np.zeros((10, 10), np.float32)
    res[:, 0] = 1e-3
    ctrl = _rx(spec, 10)
    rc, mib = ctrl.decode_mib(y, ce, res, tti0)
    ctrl.free()
    assert rc == 0
    for b in range(10):
        if (tti0 + b) % 10 == 0:
            sfn = (tti0 + b) // 10
            assert mib[b].found == 1 and mib[b].nof_tx_ports == ports and mib[b].nof_prb == nof_prb, (spec, b, mib[b].found)
            assert mib[b].sfn == sfn and bytes(mib[b].payload) == bc.mib_pack(sfn - mib[b].sfn_offset).tobytes(), (spec, b)
        else:
            assert mib[b].found == 0


# ---------------------------------------------------------------- refusals and calls in flight
def _raw(ctrl, bufs, tti0, reqs, ph):
    """One batch_ul call on device buffers -> (rc, bytes of the five result buffers, a poison pattern where nothing was written)."""
    n, m = len(reqs), max(1, len(ph))
    sizes = [C.sizeof(pkg.DlCtrlRes) * n, C.sizeof(pkg.DciMsg) * n, C.sizeof(pkg.DlCtrlUlRes) * n, C.sizeof(pkg.DciMsg) * n * pkg.DL_CTRL_MAX_UL_DCI,
             C.sizeof(pkg.PhichRes) * m]
    outs = [pkg.DevBuf.from_host(np.full(sz, 0xA5, np.uint8)) for sz in sizes]
    rc = ctrl.batch_ul_device(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, tti0, reqs, outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr, ph, outs[4].ptr)
    pkg.sync()
    return rc, [t.to_host(np.uint8).tobytes() for t in outs]


def _bufs(subs):
    g, h, r = _stack(subs)
    return pkg.DevBuf.from_host(np.ascontiguousarray(g, np.complex64)), pkg.DevBuf.from_host(np.ascontiguousarray(h, np.complex64)), pkg.DevBuf.from_host(r)


def test_refusals_leave_the_results_unwritten():
    for kw in (dict(tdd=True), dict(tdd_sf_config=7)):
        with pytest.raises(RuntimeError):
            pkg.DlCtrl(25, 1, 1, **kw)
        with pytest.raises(RuntimeError):
            pkg.DlCtrlTx(25, 1, 1, **kw)
    with pytest.raises(RuntimeError):  # a REG in two mapping units
        pkg.DlCtrlTx(6, 1, 1, phich_resources=3, tdd_sf_config=0)
    with pytest.raises(RuntimeError):
        pkg.DlCtrl(6, 1, 1, phich_resources=3, tdd_sf_config=0)
    L = pkg.lib()
    for make, cfg in ((L.srslte_hip_dl_ctrl_create_tdd, pkg.DlCtrlCfg(25, 1, 1, 0, 1, 0, 0, 1, 1)),
                      (L.srslte_hip_dl_ctrl_tx_create_tdd, pkg.DlCtrlTxCfg(25, 1, 1, 0, 1, 0, 0, 1, 1, 1))):
        assert make(C.byref(cfg), 0) is None  # cfg.tdd = 0
    # receive: configuration 1 (D S U U D D S U U D, mi 0 1 - - 1 0 1 - - 1) from tti0 = 0
    spec = (25, 1, 40, False, 1, False, 1, 1)
    cell = TddCell(*spec)
    rng = np.random.default_rng(79)
    subs, reqs = [], []
    for tti in range(10):
        if is_ul(1, tti):
            subs.append(_ul_sub(cell, tti, rng))
        else:
            y, ce, noise = channel(cell, cell.encode_full(tti, 2, draw_tdd_ul_subframe(cell, tti, 2, 0x4601, 1, rng), []), 30.0, rng)
            subs.append(dict(tti=tti, y=y, ce=ce, noise=noise))
        reqs.append(pkg.DlCtrlReq(0x4601, 1, 0, 0))
    bufs = _bufs(subs)
    ctrl = _rx(spec, 10, 4)
    rc, good = _raw(ctrl, bufs, 0, reqs, [(1, 3, 1, 0), (4, 0, 0, 0)])
    assert rc == 0 and all(g != b"\xa5" * len(g) for g in good)
    poison = lambda r: all(x == b"\xa5" * len(x) for x in r)  # noqa: E731
    for bad_ph in ([(2, 3, 1, 0)], [(0, 3, 1, 0)], [(5, 0, 0, 0)], [(1, 3, 1, 1)]):  # uplink; mi = 0 (twice); I_phich = 1 with mi = 1
        rc, r = _raw(ctrl, bufs, 0, reqs, bad_ph)
        assert rc == BAD and poison(r), bad_ph
        dph = pkg.DevBuf.from_host(np.full(16, 0xA5, np.uint8))
        assert ctrl.phich_device(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, 0, 10, bad_ph, dph.ptr) == BAD
        pkg.sync()
        assert dph.to_host(np.uint8).tobytes() == b"\xa5" * 16
    for sf in (1, 6):  # a given CFI of 3 in subframes 1 and 6
        bad = list(reqs)
        bad[sf] = pkg.DlCtrlReq(0x4601, 1, 3, 0)
        rc, r = _raw(ctrl, bufs, 0, bad, [])
        assert rc == BAD and poison(r), sf
    ok3 = list(reqs)
    ok3[4] = pkg.DlCtrlReq(0x4601, 1, 3, 0)
    assert _raw(ctrl, bufs, 0, ok3, [])[0] == 0
    ctrl.free()
    # transmit: the grids keep their sentinel
    tx = _tx(spec, max_batch=10, max_dci=4, max_phich=4)
    sentinel = (rng.normal(size=(10, 1, cell.glen)) + 1j * rng.normal(size=(10, 1, cell.glen))).astype(np.complex64)
    d_grid = pkg.DevBuf.from_host(sentinel)
    ok_cfi = [2, 2, 0, 9, 2, 2, 2, 0, 0, 2]  # uplink entries are not looked at
    nbits = pkg.dci_format_sizeof_tdd(25, 1, F1A)
    dci = lambda sf: (sf, make_msg(0x4601, 0, 0, F1A, nbits, rng))  # noqa: E731
    cfi3 = lambda sf: [3 if b == sf else c for b, c in enumerate(ok_cfi)]  # noqa: E731
    bad = [dict(cfi=ok_cfi, dcis=[dci(2)]), dict(cfi=ok_cfi, dcis=[dci(8)]),                     # a DCI in an uplink subframe
           dict(cfi=ok_cfi, phichs=[(3, 0, 0, 0, 1)]),                                           # a PHICH in an uplink subframe
           dict(cfi=ok_cfi, phichs=[(0, 0, 0, 0, 1)]), dict(cfi=ok_cfi, phichs=[(5, 3, 1, 0, 0)]),  # mi = 0
           dict(cfi=ok_cfi, phichs=[(4, 3, 1, 1, 0)]),                                           # I_phich = 1 with mi = 1
           dict(cfi=cfi3(1)), dict(cfi=cfi3(6)),                                                 # CFI 3 in subframes 1 and 6
           dict(cfi=[0 if b == 4 else c for b, c in enumerate(ok_cfi)])]                         # a downlink subframe still needs its CFI
    for case in bad:
        assert tx.put_device(d_grid.ptr, 0, 10, case["cfi"], case.get("dcis", ()), case.get("phichs", ())) == BAD, case
    pkg.sync()
    assert np.array_equal(_bits(d_grid.to_host(np.complex64).reshape(sentinel.shape)), _bits(sentinel))
    assert tx.put_device(d_grid.ptr, 0, 10, cfi3(4), [dci(0), dci(9)], [(1, 3, 1, 0, 1), (9, 0, 0, 0, 0)]) == 0
    pkg.sync()
    tx.free()


def test_combined_calls_need_matching_frame_type_and_configuration():
    """srslte_hip_dl_tx_batch_grants_ctrl / _full: a TDD pipeline with a TDD control object of its configuration is served; FDD with TDD, TDD
    with FDD and two configurations are refused and the IQ buffer keeps its sentinel."""
    nof_prb, cell_id, tbs = 25, 40, 4584
    rng = np.random.default_rng(4)
    mk_dl = lambda tdd: pkg.DlTx(cell_id, nof_prb, 1, 0x1234, 1, tbs, 2, 1, max_grants=2, tdd=tdd)  # noqa: E731
    mk_ctrl = lambda cfgi: pkg.DlCtrlTx(nof_prb, 1, cell_id, phich_resources=1, max_batch=2, tdd_sf_config=cfgi)  # noqa: E731
    grants = [(b, pkg.DlGrant.make(nof_prb, 1, tbs, 0x100 + b, cfi=2)) for b in range(2)]
    datas = [rng.integers(0, 256, tbs // 8, dtype=np.uint8) for _ in range(2)]
    dls = {"fdd": mk_dl(None), "tdd1": mk_dl((1, 7)), "tdd2": mk_dl((2, 7))}
    ctrls = {"fdd": mk_ctrl(None), "tdd1": mk_ctrl(1), "tdd2": mk_ctrl(2)}
    for d in dls:
        for c in ctrls:
            for full in (False, True):
                dl = dls[d]
                fill = np.full(dl.d_iq.nbytes // 4, 0x7F7F7F7F, np.uint32)
                pkg.lib().srslte_hip_memcpy_h2d(dl.d_iq.ptr, fill.ctypes.data, fill.nbytes)
                call = dl.encode_grants_full if full else dl.encode_grants_ctrl
                rc, iq = call(datas, 4, 2, grants, ctrls[c], [2, 2])  # subframes 4 and 5: downlink in both configurations
                pkg.sync()
                if d == c:
                    assert rc == 0 and np.abs(iq).max() > 0, (d, c, full)
                else:
                    assert rc == BAD and np.array_equal(dl.d_iq.to_host(np.uint32), fill), (d, c, full)
    # in->cfi of an uplink subframe is not looked at: a grant there (the pipeline does not know the direction) is not compared with it.
    # Configuration 1 from TTI 3: subframe 3 is uplink, subframe 4 downlink
    rc, iq = dls["tdd1"].encode_grants_ctrl(datas, 3, 2, grants, ctrls["tdd1"], [0, 2])
    assert rc == 0
    rc, iq = dls["tdd1"].encode_grants_ctrl(datas, 3, 2, grants, ctrls["tdd1"], [2, 3])
    assert rc == BAD
    for o in list(dls.values()) + list(ctrls.values()):
        o.free()


def test_creators_accept_the_issue_cells_and_agree_on_a_region_without_a_cce():
    """Both creators make every cell of the issue with its configuration; 25 PRB, Ng = 2, configuration 0 - mi = 2 leaves 4 REGs, no CCE, to a
    CFI-1 region - is refused by both, while configuration 6 of that cell (mi = 1) is served by both."""
    for spec in TDD_CELLS:
        _rx(spec, 1).free()
        _tx(spec, 1, 1, 1).free()
    for make in (pkg.DlCtrl, pkg.DlCtrlTx):
        with pytest.raises(RuntimeError):
            make(25, 1, 9, phich_resources=3, tdd_sf_config=0)
        make(25, 1, 9, phich_resources=3, tdd_sf_config=6).free()


def test_two_calls_in_flight_on_two_objects_and_streams():
    spec = TDD_CELLS[1]
    cell, tti0, subs = tdd_phich_subframes(spec, 91, nof_frames=1)
    rng = np.random.default_rng(92)
    for s in subs:  # add DCIs to the downlink subframes
        if not s["ul"]:
            msgs = draw_tdd_ul_subframe(cell, s["tti"], 2, 0x4601, 1, rng)
            y, ce, noise = channel(cell, cell.encode_full(s["tti"], 2, msgs, s["phichs"]), 25.0, rng)
            s.update(y=y, ce=ce, noise=noise)
    reqs = [pkg.DlCtrlReq(0x4601, 1, 0, 0) for _ in subs]
    ph = [(b,) + p[:3] for b, s in enumerate(subs) for p in s["phichs"]]
    bufs = _bufs(subs)
    c1, c2 = _rx(spec, 10, len(ph)), _rx(spec, 10, len(ph))
    rc, want = _raw(c1, bufs, tti0, reqs, ph)
    assert rc == 0 and len(ph) > 3
    L = pkg.lib()
    s1, s2 = L.srslte_hip_stream_create(), L.srslte_hip_stream_create()
    outs = [[pkg.DevBuf.from_host(np.full(len(w), 0xA5, np.uint8)) for w in want] for _ in range(2)]
    for _ in range(3):
        for c, st, o in ((c1, s1, outs[0]), (c2, s2, outs[1])):
            assert c.batch_ul_device(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, tti0, reqs, o[0].ptr, o[1].ptr, o[2].ptr, o[3].ptr, ph, o[4].ptr, st) == 0
    L.srslte_hip_stream_sync(s1)
    L.srslte_hip_stream_sync(s2)
    for o in outs:
        assert [t.to_host(np.uint8).tobytes() for t in o] == want
    L.srslte_hip_stream_destroy(s1)
    L.srslte_hip_stream_destroy(s2)
    c1.free()
    c2.free()


# ---------------------------------------------------------------- the closed loop: a complete TDD frame on the device, both directions
def _format1a_tdd(cell, rnti, L, ncce, L_crb, RB_start, mcs, pid=0, ndi=0, rv=0, dai=1):
    """A format-1A C-RNTI DCI of a TDD cell (36.212 5.3.3.1.3, localized): flag, VRB type, RIV, MCS, HARQ process (4 bits), NDI, RV, TPC, DAI,
    padding - dl_ctrl_ref.format1a_msg with the TDD fields."""
    from dl_ctrl_ref import RefDciMsg, riv
    n = sizeof(cell, F1A)
    nb = int(np.ceil(np.log2(cell.nof_prb * (cell.nof_prb + 1) / 2)))
    bits = [1, 0]
    for v, w in ((riv(cell.nof_prb, L_crb, RB_start), nb), (mcs, 5), (pid, 4), (ndi, 1), (rv, 2), (0, 2), (dai, 2)):
        bits += [(v >> (w - 1 - i)) & 1 for i in range(w)]
    bits += [0] * (n - len(bits))
    m = RefDciMsg()
    m.payload[:n] = bits
    m.nof_bits, m.L, m.ncce, m.format, m.rnti = n, L, ncce, F1A, rnti
    return m


@pytest.mark.parametrize("spec,ss_config", [((6, 1, 13, False, 2, False, 1, 1), 7), ((25, 1, 76, False, 1, True, 1, 1), 7)])
def test_closed_loop_of_one_tdd_frame(spec, ss_config):
    """srslte_hip_dl_tx_batch_grants_full on a TDD pipeline writes ten subframes of IQ: PSS / SSS / PBCH, PCFICH, a format-1A DCI with its
    PDSCH in the normal downlink subframes behind subframe 0, a format-0 DCI packed by the reference in every downlink and special subframe,
    PHICHs where the subframe has groups. A flat channel at 30 dB. The tracked synchronisation in detect mode reports TDD, the cell id and
    subframe 1; the device's OFDM, the estimator with set_tdd and the TDD control receiver find every DCI (the reference unpacks the grants
    and the format-0 fields it packed) and read every PHICH; srslte_hip_dl_rx_batch_grants returns the transport blocks."""
    from dl_ctrl_ref import unpack_grant
    from test_gpu_dl_ctrl import _front
    from test_gpu_sync import FIND
    nof_prb, ports, cell_id, sf_config = spec[0], spec[1], spec[2], spec[7]
    cell = TddCell(*spec)
    rng = np.random.default_rng(nof_prb)
    tti0, nsf, tm = 40, 10, 0
    cfis, dcis, phichs, grants, datas, subs = [], [], [], [], [], []
    for b in range(nsf):
        tti = tti0 + b
        sf_idx = tti % 10
        if is_ul(sf_config, sf_idx):
            cfis.append(0)
            subs.append(None)
            continue
        # subframes 1 and 6 carry the PSS on symbol 2: two control symbols, which is CFI 1 on a cell of at most 10 PRB (36.211 Table 6.7-1)
        cfi = (1 if nof_prb <= 10 else 2) if sf_idx in (1, 6) else 3
        cell.select(tti)
        ncce, rnti = cell.ncce[cfi - 1], 0x4600 + 37 * b
        locs = pkg.pdcch_ue_locations(ncce, sf_idx, rnti)
        s = dict(tti=tti, cfi=cfi, rnti=rnti, dl=None, ul=None, phichs=[])
        used = set()
        if sf_idx not in (0, 1, 6):  # a PDSCH: not beside the PBCH, not in a DwPTS
            L, n0 = next((l, n) for l, n in locs if l >= 1)
            used |= set(range(n0, n0 + (1 << L)))
            while True:  # a grant the per-subframe receive takes: one code-block size, no filler bits
                L_crb = int(rng.integers(4, nof_prb + 1))
                msg = _format1a_tdd(cell, rnti, L, n0, L_crb, int(rng.integers(0, nof_prb - L_crb + 1)), int(rng.integers(0, 10 if nof_prb == 6 else 16)))
                g = unpack_grant(cell, tti, cfi, msg, tm)
                rc_s, seg = pkg.cbsegm(g["tb"][0]["tbs"])
                if rc_s == 0 and g["tb"][0]["tbs"] % 8 == 0 and seg.F == 0 and seg.C2 == 0:
                    break
            tbs = g["tb"][0]["tbs"]
            s["dl"] = dict(msg=bytes(msg.payload[:msg.nof_bits]), grant=g, data=rng.integers(0, 256, tbs // 8, dtype=np.uint8))
            dcis.append((b, msg))
            grants.append((b, pkg.DlGrant.make(nof_prb, g["tb"][0]["mod"], tbs, rnti, cfi=cfi, prb_mask=g["prb_idx"])))
            datas.append(s["dl"]["data"])
        free = [(l, n) for l, n in locs if not (set(range(n, n + (1 << l))) & used)]
        if free:  # a format-0 DCI for the same UE, packed by the reference with the TDD fields
            L, n0 = free[0]
            s["ul"] = dict(L_prb=int(rng.integers(1, nof_prb)), n_prb=0, mcs=int(rng.integers(0, 20)), ndi=int(rng.integers(0, 2)), n_dmrs=int(rng.integers(0, 8)))
            dcis.append((b, cell.pack_pusch(rnti, L, n0, s["ul"]["L_prb"], 0, s["ul"]["mcs"], s["ul"]["ndi"], s["ul"]["n_dmrs"])))
        s["phichs"] = draw_tdd_phichs(cell, sf_idx, rng, nmax=3)
        phichs += [(b,) + p for p in s["phichs"]]
        cfis.append(cfi)
        subs.append(s)
    assert len(grants) >= 3 and len(phichs) >= 3 and sum(1 for s in subs if s and s["ul"]) >= 4
    tbs_max = max(gr.tbs for _, gr in grants)
    tdd = (sf_config, ss_config)
    dl = pkg.DlTx(cell_id, nof_prb, 1, 0x1234, 1, tbs_max, nsf, ports, max_grants=len(grants), tdd=tdd)
    enb = _tx(spec, max_batch=nsf, max_dci=len(dcis), max_phich=len(phichs))
    rc, time = dl.encode_grants_full(datas, tti0, nsf, grants, enb, cfis, dcis, phichs)
    assert rc == 0
    dl.free()
    enb.free()
    iq = time[:, 0, :] * (0.8 * np.exp(0.4j))
    sigma = 10 ** (-30 / 20) * np.sqrt(np.mean(np.abs(iq) ** 2))
    iq = (iq + sigma / np.sqrt(2) * (rng.normal(size=iq.shape) + 1j * rng.normal(size=iq.shape))).astype(np.complex64)
    sf_len = iq.shape[1]
    # synchronisation: one tracked call in detect mode over the frame; the PSS of subframe 1 is the first in the window
    fft = pkg.symbol_sz(nof_prb)
    q = pkg.Sync(fft, 5 * sf_len, 5 * sf_len, max_items=1, **FIND)
    tr = pkg.SyncTracks(q, 1, 0.0, pkg.FRAME_DETECT)
    rc, rows = tr.track(iq.reshape(1, -1), [pkg.SyncTrackItem.make(0, cell_id % 3)])
    tr.free()
    q.free()
    assert rc == 0
    cp0, cp = 160 * fft // 2048, 144 * fft // 2048
    assert (rows[0].ret, rows[0].frame_type, rows[0].cell_id, rows[0].sf_idx) == (1, 1, cell_id, 1), (rows[0].ret, rows[0].frame_type, rows[0].cell_id,
                                                                                                    rows[0].sf_idx)
    assert abs(int(rows[0].peak_pos) - (sf_len + cp0 + fft + 2 * (cp + fft))) <= 1, rows[0].peak_pos  # the end of symbol 2 of subframe 1
    # OFDM, the estimator of a TDD cell, the control receiver
    est = pkg.ChestDl(cell_id, nof_prb, nof_ports=ports)
    assert est.set_tdd(sf_config, ss_config) == 0
    d_grid, d_ce, d_res, _ = _front(nof_prb, ports, cell_id, iq[:, None, :], tti0, 1, est=est)
    est.free()
    ue = _rx(spec, nsf, max(1, len(phichs)))
    reqs = [pkg.DlCtrlReq(s["rnti"] if s else 0x4601, tm, 0, 0) for s in subs]
    ph_req = [p[:4] for p in phichs]
    n = nsf
    bufs = [pkg.DevBuf(C.sizeof(pkg.DlCtrlRes) * n), pkg.DevBuf(C.sizeof(pkg.DciMsg) * n), pkg.DevBuf(C.sizeof(pkg.DlCtrlUlRes) * n),
            pkg.DevBuf(C.sizeof(pkg.DciMsg) * n * pkg.DL_CTRL_MAX_UL_DCI), pkg.DevBuf(C.sizeof(pkg.PhichRes) * len(phichs))]
    assert ue.batch_ul_device(d_grid.ptr, d_ce.ptr, d_res.ptr, tti0, reqs, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, ph_req, bufs[4].ptr) == 0
    pkg.sync()
    ue.free()
    out, msg, ul = (pkg.DlCtrlRes * n)(), (pkg.DciMsg * n)(), (pkg.DlCtrlUlRes * n)()
    ulm, phr = (pkg.DciMsg * (n * pkg.DL_CTRL_MAX_UL_DCI))(), (pkg.PhichRes * len(phichs))()
    for dst, src in ((out, bufs[0]), (msg, bufs[1]), (ul, bufs[2]), (ulm, bufs[3]), (phr, bufs[4])):
        pkg.lib().srslte_hip_memcpy_d2h(C.addressof(dst), src.ptr, C.sizeof(dst))
    rx_grants = []
    for b, s in enumerate(subs):
        if s is None:
            assert (out[b].cfi, out[b].nof_dci, ul[b].nof_ul_dci) == (0, 0, 0), b
            rx_grants.append(pkg.DlGrant.make(nof_prb, 1, 0, 0))
            continue
        assert out[b].cfi == s["cfi"], (b, out[b].cfi)
        assert out[b].nof_dci == (1 if s["dl"] else 0) and ul[b].nof_ul_dci == (1 if s["ul"] else 0), (b, out[b].nof_dci, ul[b].nof_ul_dci)
        if s["ul"]:
            got = cell.unpack_pusch(ulm[b * pkg.DL_CTRL_MAX_UL_DCI])
            assert got is not None and got["rnti"] == s["rnti"] and {f: got[f] for f in s["ul"]} == s["ul"], (b, got, s["ul"])
        if s["dl"]:
            assert msg[b].rnti == s["rnti"] and bytes(msg[b].payload[:msg[b].nof_bits]) == s["dl"]["msg"], b
            g = unpack_grant(cell, s["tti"], out[b].cfi, msg[b], tm)
            assert g is not None and np.array_equal(g["prb_idx"], s["dl"]["grant"]["prb_idx"]) and g["tb"][0] == s["dl"]["grant"]["tb"][0], b
            rx_grants.append(pkg.DlGrant.make(nof_prb, g["tb"][0]["mod"], g["tb"][0]["tbs"], msg[b].rnti, cfi=out[b].cfi, prb_mask=g["prb_idx"]))
        else:
            rx_grants.append(pkg.DlGrant.make(nof_prb, 1, 0, 0))
    for (b, lo, dm, ip, ack), r in zip(phichs, phr):
        assert r.ack_value == ack, (b, lo, dm, ip, ack, r.distance)
    hc = pkg.ChestDlCfg()
    hc.filter_coef[0], hc.filter_coef[1] = 4.0, 1.0
    rx = pkg.DlRx(cell_id, nof_prb, 1, 0x1234, 1, tbs_max, 6, nsf, True, hc, tdd=tdd)
    rc, tb, ok = rx.decode_grants(iq, tti0, rx_grants)
    rx.free()
    assert rc == 0
    for b, s in enumerate(subs):
        if s and s["dl"]:
            assert ok[b] == 1 and np.array_equal(tb[b][:len(s["dl"]["data"])], s["dl"]["data"]), b
