"""DL control region receive on the device (srslte_hip_dl_ctrl_batch) against the reference's own PCFICH / PDCCH functions in
oracle/_ref/libsrslte_ref.so. Control regions are written by srslte_pcfich_encode / srslte_pdcch_encode (the target UE's DCI among DCIs for
other RNTIs), passed through a drawn per-RE channel of every port to every receive antenna plus noise; the device and the reference receive
them with the same channel estimates and noise estimate."""
import ctypes as C
import importlib

import numpy as np
import pytest

import refdrv
from _libs import aligned, ref
from dl_ctrl_ref import F0, F1A, SIRNTI, Cell, blind_search, channel, draw_subframe, unpack_grant

pkg = importlib.import_module("srslte-emane_amd")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(ref() is None, reason="oracle/_ref/libsrslte_ref.so is not built")]

# (nof_prb, ports, cell_id, cp_ext, phich_res, phich_ext, nof_rx)
CELLS = [(6, 1, 1, False, 0, False, 1), (15, 2, 77, False, 1, True, 2), (25, 4, 200, True, 2, False, 1), (50, 2, 150, False, 3, False, 1),
         (75, 1, 301, True, 1, True, 3), (100, 2, 5, False, 2, False, 2), (100, 4, 411, False, 0, True, 4), (50, 1, 17, False, 0, False, 2),
         (6, 2, 503, True, 3, True, 4), (25, 1, 89, False, 2, True, 4)]


def _run_cell(spec, seed, nof_sf=10, snrs=(30.0, 2.0)):
    cell = Cell(*spec)
    rng = np.random.default_rng(seed)
    tti0 = int(rng.integers(0, 10240))
    ctrl = pkg.DlCtrl(spec[0], spec[1], spec[2], cp_ext=spec[3], phich_resources=spec[4], phich_ext=spec[5], nof_rx=spec[6], max_batch=nof_sf)
    kinds = ["ue", "ue", "ul", "none", "si1a", "si1c", "ue", "ue", "ue", "none"]
    subs, reqs, ys, ces, res = [], [], [], [], []
    for b in range(nof_sf):
        tti = tti0 + b
        cfi = 1 + int(rng.integers(0, 3))
        tm = int(rng.integers(0, 4))
        kind = kinds[b % len(kinds)]
        rnti = SIRNTI if kind.startswith("si") else int(rng.integers(0x0B, 0xFFF3))
        dcis, placed = draw_subframe(cell, tti, cfi, rnti, tm, rng, kind)
        tx = cell.encode(tti, cfi, dcis)
        snr = snrs[b % len(snrs)]
        y, ce, noise = channel(cell, tx, snr, rng)
        r10 = np.zeros(10, np.float32)
        r10[0] = noise
        subs.append(dict(tti=tti, cfi=cfi, tm=tm, rnti=rnti, kind=kind, placed=placed, snr=snr, y=y, ce=ce, noise=noise))
        given = cfi if b % 4 == 3 else 0  # every fourth subframe: the CFI is given, not decoded
        reqs.append(pkg.DlCtrlReq(rnti, tm, given, 0))
        ys.append(np.stack(y))
        ces.append(ce)
        res.append(r10)
    rc, out, msgs = ctrl.batch(np.stack(ys), np.stack(ces), np.stack(res), tti0, reqs)
    assert rc == 0
    llr, cands = ctrl.llr(nof_sf), ctrl.candidates(nof_sf)
    ctrl.free()
    return cell, subs, reqs, out, msgs, llr, cands


@pytest.mark.parametrize("idx", range(len(CELLS)))
def test_pcfich_llr_candidates_and_search(idx):
    spec = CELLS[idx]
    cell, subs, reqs, out, msgs, llr, cands = _run_cell(spec, 1000 + idx)
    found = 0
    for b, s in enumerate(subs):
        # PCFICH: srslte_pcfich_decode on the same inputs
        cfi_ref, corr_ref = cell.pcfich(s["tti"], s["y"], s["ce"], s["noise"])
        assert abs(out[b].cfi_corr - corr_ref) <= 1e-3 * max(1.0, abs(corr_ref)), (spec, b, out[b].cfi_corr, corr_ref)
        cfi = reqs[b].cfi or cfi_ref
        assert out[b].cfi == cfi, (spec, b, out[b].cfi, cfi_ref)
        if s["snr"] > 20:
            assert cfi_ref == s["cfi"], (spec, b)
        # LLR rows: the reference chain from exported pieces, the project's float tolerance
        n = 72 * cell.ncce[cfi - 1]
        want = cell.llr_chain(s["tti"], cfi, s["y"], s["ce"], s["noise"])
        np.testing.assert_allclose(llr[b, :n], want, rtol=1e-4, atol=1e-4 * max(1.0, float(np.abs(want).max())), err_msg=str((spec, b)))
        assert not llr[b, n:].any()
        # every searched candidate, bit-exact: srslte_pdcch_dci_decode on the device's own LLRs
        row = aligned(llr.shape[1], np.float32)
        row[:] = llr[b]
        for c in cands[b]:
            E = 72 << c.L
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
        # the search: a restatement of dci_blind_search over the reference's srslte_pdcch_decode_msg on its own LLRs
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
            assert m is not None, (spec, b, s["kind"])  # clean subframes: the DCI is found
        if s["kind"] in ("none", "ul"):
            assert m is None
    assert found >= 3


def test_refusals_and_pinned_outputs():
    import torch

    with pytest.raises(RuntimeError):
        pkg.DlCtrl(25, 1, 1, tdd=True)
    spec = (25, 2, 31, False, 1, False, 2)
    cell = Cell(*spec)
    rng = np.random.default_rng(5)
    ctrl = pkg.DlCtrl(25, 2, 31, phich_resources=1, nof_rx=2, max_batch=2)
    rnti = 0x4601
    tx = cell.encode(3, 2, draw_subframe(cell, 3, 2, rnti, 1, rng, "ue")[0])
    y, ce, noise = channel(cell, tx, 30.0, rng)
    r10 = np.zeros((1, 10), np.float32)
    r10[0, 0] = noise
    dg, dce, dres = pkg.DevBuf.from_host(np.stack(y)), pkg.DevBuf.from_host(ce), pkg.DevBuf.from_host(r10)
    dout, dmsg = pkg.DevBuf(64), pkg.DevBuf(2 * C.sizeof(pkg.DciMsg))
    ok = pkg.DlCtrlReq(rnti, 1, 0, 0)
    for bad in (pkg.DlCtrlReq(rnti, 1, 0, 1), pkg.DlCtrlReq(rnti, 4, 0, 0), pkg.DlCtrlReq(rnti, 1, 4, 0)):
        assert ctrl.run_device(dg.ptr, dce.ptr, dres.ptr, 3, [bad], dout.ptr, dmsg.ptr) == pkg.SRSLTE_ERROR_INVALID_INPUTS
    assert ctrl.run_device(dg.ptr, dce.ptr, dres.ptr, 3, [ok] * 3, dout.ptr, dmsg.ptr) == pkg.SRSLTE_ERROR_INVALID_INPUTS  # > max_batch
    assert ctrl.run_device(dg.ptr, dce.ptr, dres.ptr, 3, [ok], None, dmsg.ptr) == pkg.SRSLTE_ERROR_INVALID_INPUTS
    # results straight into pinned host memory
    h_out = torch.zeros(C.sizeof(pkg.DlCtrlRes), dtype=torch.uint8).pin_memory()
    h_msg = torch.zeros(C.sizeof(pkg.DciMsg), dtype=torch.uint8).pin_memory()
    assert ctrl.run_device(dg.ptr, dce.ptr, dres.ptr, 3, [ok], h_out.data_ptr(), h_msg.data_ptr()) == 0
    pkg.sync()
    res = pkg.DlCtrlRes.from_buffer_copy(h_out.numpy().tobytes())
    msg = pkg.DciMsg.from_buffer_copy(h_msg.numpy().tobytes())
    cell.extract(3, res.cfi, y, ce, noise)
    m = blind_search(cell, 3, res.cfi, rnti, 1)
    assert res.cfi == 2 and res.nof_dci == 1 and m is not None
    assert (msg.nof_bits, msg.L, msg.ncce, msg.format, msg.rnti) == (m.nof_bits, m.L, m.ncce, m.format, rnti)
    ctrl.free()


# ---------------------------------------------------------------- the device's own front end: OFDM -> chest_dl -> control region
def _front(nof_prb, ports, cell_id, iq, tti0, nof_rx=1, est=None):
    """iq [nof_sf][nof_rx][sf_len] -> device buffers (grid, ce, res) from srslte_hip_ofdm_rx_sf_batch + srslte_hip_chest_dl_estimate_batch_multi
    (default srslte_chest_dl_cfg_t, as ue_dl's ZERO_OBJECT), plus the grid read back."""
    L = pkg.lib()
    x = np.ascontiguousarray(iq, np.complex64)
    nsf = x.shape[0]
    o = pkg.Ofdm(nof_prb, True, rx=True)
    glen = 14 * 12 * nof_prb
    d_iq, d_grid = pkg.DevBuf.from_host(x), pkg.DevBuf(8 * nsf * nof_rx * glen)
    assert L.srslte_hip_ofdm_rx_sf_batch(o.h, d_iq.ptr, d_grid.ptr, nsf * nof_rx, None) == 0
    own = est is None
    est = est or pkg.ChestDl(cell_id, nof_prb, nof_ports=ports)
    d_ce, d_res = pkg.DevBuf(8 * nsf * ports * nof_rx * glen), pkg.DevBuf(40 * nsf)
    L.srslte_hip_chest_dl_estimate_batch_multi.argtypes = [C.c_void_p, C.POINTER(pkg.ChestDlCfg), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                           C.c_int, C.c_int, C.c_void_p]
    cfg = pkg.ChestDlCfg()
    assert L.srslte_hip_chest_dl_estimate_batch_multi(est.h, C.byref(cfg), tti0, d_grid.ptr, d_ce.ptr, d_res.ptr, nsf, nof_rx, None) == 0
    pkg.sync()
    grid = d_grid.to_host(np.complex64).reshape(nsf, nof_rx, glen)
    o.free()
    if own:
        est.free()
    return d_grid, d_ce, d_res, grid


def _ctrl_on_device(ctrl, bufs, tti0, reqs):
    d_grid, d_ce, d_res = bufs[:3]
    n = len(reqs)
    dout, dmsg = pkg.DevBuf(C.sizeof(pkg.DlCtrlRes) * n), pkg.DevBuf(C.sizeof(pkg.DciMsg) * n)
    assert ctrl.run_device(d_grid.ptr, d_ce.ptr, d_res.ptr, tti0, reqs, dout.ptr, dmsg.ptr) == 0
    pkg.sync()
    out, msg = (pkg.DlCtrlRes * n)(), (pkg.DciMsg * n)()
    pkg.lib().srslte_hip_memcpy_d2h(C.addressof(out), dout.ptr, C.sizeof(out))
    pkg.lib().srslte_hip_memcpy_d2h(C.addressof(msg), dmsg.ptr, C.sizeof(msg))
    return list(out), list(msg)


@pytest.mark.skipif(refdrv.lib() is None, reason="oracle/_ref/librefdrv.so is not built")
def test_recorded_iq():
    """signal.1.92M.amar.dat (pdsch_pdcch_file_test: 6 PRB, cell 1, SI-RNTI) through the device's OFDM, estimator and control receive, one
    subframe per call as srsue runs them (the estimator's automatic filter follows the previous subframe's noise estimate): the CFI and the
    SI-RNTI DCIs with the grants refdrv_dl_find_dci finds on the same grids; signal.10M.dat (pcfich_file_test: 50 PRB, 2 ports, cell 150):
    CFI 2 with a correlation above 2.8."""
    import recorded_iq
    cell = Cell(6, 1, 1, False, 2, False, 1)
    ctrl = pkg.DlCtrl(6, 1, 1, phich_resources=2, max_batch=1)
    est = pkg.ChestDl(1, 6)
    grids, found = [], []
    for sf in range(10):
        bufs = _front(6, 1, 1, refdrv.read_iq("signal.1.92M.amar.dat", 1920, sf * 1920).reshape(1, 1, -1), sf, est=est)
        out, msg = _ctrl_on_device(ctrl, bufs, sf, [pkg.DlCtrlReq(SIRNTI, 0, 0, 0)])
        grids.append(bufs[3][0, 0])
        found.append((out[0], msg[0]))
    it = iter(grids)
    want = recorded_iq.pdsch_pdcch_file(lambda *a: next(it))  # the reference's estimator, PCFICH, PDCCH and search on the device's grids
    assert [w["sf"] for w in want if w["dci"]] == [2, 5]
    for sf, ((out, msg), w) in enumerate(zip(found, want)):
        assert out.cfi == w["cfi"] == 3 and abs(out.cfi_corr - w["cfi_corr"]) < 1e-2, (sf, out.cfi, out.cfi_corr, w["cfi_corr"])
        assert out.nof_dci == int(w["dci"]), sf
        if w["dci"]:
            g = unpack_grant(cell, sf, out.cfi, msg, 0)
            assert msg.rnti == SIRNTI and g is not None
            assert (g["tb"][0]["mcs"], g["tb"][0]["tbs"], g["nof_prb"]) == (w["grant"]["mcs"], w["grant"]["tbs"], w["grant"]["nof_prb"]), sf
    ctrl.free()
    est.free()
    ctrl2 = pkg.DlCtrl(50, 2, 150, phich_resources=2, max_batch=1)
    bufs = _front(50, 2, 150, refdrv.read_iq("signal.10M.dat", 15 * 768).reshape(1, 1, -1), 0)
    out, _ = _ctrl_on_device(ctrl2, bufs, 0, [pkg.DlCtrlReq(0x1234, 1, 0, 0)])
    assert out[0].cfi == 2 and out[0].cfi_corr > 2.8, (out[0].cfi, out[0].cfi_corr)
    ctrl2.free()


@pytest.mark.skipif(refdrv.lib() is None, reason="oracle/_ref/librefdrv.so is not built")
@pytest.mark.parametrize("nof_prb,ports,nof_rx", [(25, 1, 1), (50, 2, 2)])
def test_end_to_end(nof_prb, ports, nof_rx):
    """Subframes 1-4 of a cell, each with a format-1A DCI for its own C-RNTI (reference encoders) and the PDSCH it announces
    (srslte_hip_dl_tx_batch_grants), through OFDM modulation, a flat channel and noise; received by the device's OFDM, estimator and control
    receive; the DCIs unpacked by the reference (srslte_dci_msg_unpack_pdsch + srslte_ra_dl_dci_to_grant) feed
    srslte_hip_dl_rx_grid_batch_grants2, which returns the transmitted transport blocks. The grants equal refdrv_dl_find_dci's on the
    device's grids."""
    from dl_ctrl_ref import format1a_msg, unpack_grant as unpack
    cell_id, tti0, nsf, tm = 3 * nof_prb + ports, 1, 4, 0 if ports == 1 else 1
    cell = Cell(nof_prb, ports, cell_id, False, 1, False, nof_rx)
    rng = np.random.default_rng(nof_prb + ports)
    glen = 14 * 12 * nof_prb
    ctrl_grid = np.zeros((nsf, ports, glen), np.complex64)
    tx_grants, datas, subs = [], [], []
    for b in range(nsf):
        tti, cfi, rnti = tti0 + b, 1 + b % 3, int(rng.integers(0x0B, 0xFFF3))
        ncce = cell.ncce[cfi - 1]
        L, n0 = next((l, n) for l, n in pkg.pdcch_ue_locations(ncce, tti % 10, rnti) if l >= 2)
        while True:  # a grant the per-subframe receive takes: one code-block size, no filler bits
            L_crb = int(rng.integers(4, nof_prb + 1))
            msg = format1a_msg(cell, rnti, L, n0, L_crb, int(rng.integers(0, nof_prb - L_crb + 1)), int(rng.integers(0, 28)))
            g = unpack(cell, tti, cfi, msg, tm)
            rc_s, s = pkg.cbsegm(g["tb"][0]["tbs"])
            if rc_s == 0 and g["tb"][0]["tbs"] % 8 == 0 and s.F == 0 and s.C2 == 0:
                break
        ctrl_grid[b] = cell.encode(tti, cfi, [msg])
        tbs = g["tb"][0]["tbs"]
        datas.append(rng.integers(0, 256, tbs // 8, dtype=np.uint8))
        tx_grants.append((b, pkg.DlGrant.make(nof_prb, g["tb"][0]["mod"], tbs, rnti, cfi=cfi, prb_mask=g["prb_idx"])))
        subs.append(dict(tti=tti, cfi=cfi, rnti=rnti, grant=g))
    tbs_max = max(gr.tbs for _, gr in tx_grants)
    tx = pkg.DlTx(cell_id, nof_prb, 1, 0x1234, 1, tbs_max, nsf, ports, max_grants=nsf)
    tx.encode_grants(datas, tti0, nsf, tx_grants)
    grid = tx.debug(3, np.complex64, nsf * ports * glen).reshape(nsf, ports, glen) + ctrl_grid
    tx.free()
    otx = pkg.Ofdm(nof_prb, True, rx=False)
    time = otx.tx_sf(grid.reshape(nsf * ports, glen)).reshape(nsf, ports, -1)
    otx.free()
    gains = (rng.normal(size=(ports, nof_rx)) + 1j * rng.normal(size=(ports, nof_rx))) / np.sqrt(2 * ports)
    iq = np.einsum("pa,bpt->bat", gains, time)
    sigma = 10 ** (-30 / 20) * np.sqrt(np.mean(np.abs(iq) ** 2))
    iq = (iq + sigma / np.sqrt(2) * (rng.normal(size=iq.shape) + 1j * rng.normal(size=iq.shape))).astype(np.complex64)
    bufs = _front(nof_prb, ports, cell_id, iq, tti0, nof_rx)
    ctrl = pkg.DlCtrl(nof_prb, ports, cell_id, phich_resources=1, nof_rx=nof_rx, max_batch=nsf)
    out, msgs = _ctrl_on_device(ctrl, bufs, tti0, [pkg.DlCtrlReq(s["rnti"], tm, 0, 0) for s in subs])
    ctrl.free()
    ref_rx = refdrv.RefDl(nof_prb, ports, cell_id, nof_rx=nof_rx, phich_resources=1)
    ref_rx.set_chest_cfg()
    rx_grants = []
    for b, s in enumerate(subs):
        assert out[b].cfi == s["cfi"] and out[b].nof_dci == 1 and msgs[b].rnti == s["rnti"], (b, out[b].cfi, out[b].nof_dci)
        g = unpack(cell, s["tti"], out[b].cfi, msgs[b], tm)
        assert g is not None and np.array_equal(g["prb_idx"], s["grant"]["prb_idx"]) and g["tb"][0] == s["grant"]["tb"][0], b
        for a in range(nof_rx):
            ref_rx.put_grid(bufs[3][b, a], a)
        rc, cfi_ref, _ = ref_rx.estimate(s["tti"])
        found, rg = ref_rx.find_dci(s["rnti"], tm)
        assert rc == 0 and cfi_ref == out[b].cfi and found == 1
        assert (rg["mcs"], rg["tbs"], rg["nof_prb"]) == (g["tb"][0]["mcs"], g["tb"][0]["tbs"], g["nof_prb"]), b
        g2 = pkg.DlGrant2()
        g2.tb0 = pkg.DlGrant.make(nof_prb, g["tb"][0]["mod"], g["tb"][0]["tbs"], msgs[b].rnti, cfi=out[b].cfi, rv=max(0, g["tb"][0]["rv"]),
                                  prb_mask=g["prb_idx"])
        g2.tx_scheme, g2.pmi = g["tx_scheme"], g["pmi"]
        rx_grants.append(g2)
    ref_rx.free()
    rx = pkg.DlRx(cell_id, nof_prb, 1, 0x1234, 1, tbs_max, 6, nsf, nof_rx=nof_rx, nof_ports=ports)
    rc, tb, ok = rx.decode_grants2(bufs[3], tti0, rx_grants, from_grid=True)
    rx.free()
    assert rc == 0
    for b in range(nsf):
        assert ok[0][b] == 1 and np.array_equal(tb[0][b][:len(datas[b])], datas[b]), b
