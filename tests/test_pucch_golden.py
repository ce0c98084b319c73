"""The PUCCH restatement (tests/ul_ctrl_ref.py) and the host helpers against tests/golden/pucch.npz, recorded from the reference's own pucch.c
and refsignal_ul.c by tests/gen_golden_pucch.py: srslte_pucch_n_prb and the cyclic-shift state of srslte_pucch_alpha_format1 / 2 at every
n_pucch up to the band edge of five cells, and srslte_pucch_encode, the DMRS and srslte_chest_ul_estimate_pucch + srslte_pucch_decode at the
full-signal records. Then the share of the receive sweep's requests (tests/test_gpu_pucch_sweep.py) that the reference chain alone puts within
1e-4 of a threshold or a tie. No GPU."""
import collections

import numpy as np
import pytest

from _libs import ref
from pucch_sweep import (NAMES, OOB, STATE_SF, SWEEP_CELLS, SWEEP_SNRS, al, cfg_of, golden, last_in_band, pkg, rec_grid, rec_tx, ref_of, sweep_scene,
                         threshold)
from ul_ctrl_ref import ALPHA, F1A, F2, alpha1, alpha2, pucch_n_prb

needs_ref = pytest.mark.skipif(ref() is None, reason="oracle/_ref/libsrslte_ref.so is not built")


def _n_cs_cell(spec):
    return pkg.pucch_n_cs_cell(cfg_of(spec))  # pinned to the reference's by tests/test_ul_ctrl_host.py


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_recorded_integer_state(name):
    """pucch_n_prb, alpha1 and alpha2 of ul_ctrl_ref.py against the reference's srslte_pucch_n_prb / srslte_pucch_alpha_format1 / 2 at every
    recorded (n_pucch, slot, symbol): every index to the first one out of band at subframes 0 and 9, four indices at all 20 slots."""
    g, spec = golden(), SWEEP_CELLS[name]
    P, _, ext, _, D, Ncs, nrb2, _ = spec
    ncc, nsym = _n_cs_cell(spec), 6 if ext else 7
    prb1, prb2, st1, st2 = (g["%s.%s" % (name, k)] for k in ("f1_prb", "f2_prb", "f1_state", "f2_ncs"))
    assert prb1.shape[0] == last_in_band(spec, 1) + 2 and prb2.shape[0] == last_in_band(spec, 2) + 2
    assert st1.shape == (prb1.shape[0], 2, 2, nsym, 3) and st2.shape == (prb2.shape[0], 2, 2, nsym)
    for fmt, prb in ((F1A, prb1), (F2, prb2)):
        for n in range(prb.shape[0]):
            got = [pucch_n_prb(fmt, n, s, P, D, Ncs, nrb2, ext) for s in range(2)]
            assert [x if 0 <= x < P else OOB for x in got] == prb[n].tolist(), (fmt, n)
        assert OOB in prb[-1] and not (prb[:-1] == OOB).any()
    for n in range(st1.shape[0]):
        for i, sf in enumerate(STATE_SF):
            for s in range(2):
                for l in range(nsym):
                    assert alpha1(ncc, ext, D, Ncs, n, 2 * sf + s, l) == tuple(st1[n, i, s, l]), (n, sf, s, l)
    for n in range(st2.shape[0]):
        for i, sf in enumerate(STATE_SF):
            for s in range(2):
                for l in range(nsym):
                    assert alpha2(ncc, Ncs, nrb2, n, 2 * sf + s, l) == st2[n, i, s, l], (n, sf, s, l)
    for k, n in enumerate(g[name + ".all_idx"].tolist()):
        for ns in range(20):
            for l in range(nsym):
                assert alpha1(ncc, ext, D, Ncs, n, ns, l) == tuple(g[name + ".all_f1"][k, ns, l]), (n, ns, l)
                assert alpha2(ncc, Ncs, nrb2, n, ns, l) == g[name + ".all_f2"][k, ns, l], (n, ns, l)
    # the sweep reaches what it is there for: n_oc 2 (1 on the extended CP) in both slots, both sides of c N_cs / delta, the innermost PRB
    assert {int(x) for x in st1[:, 0, :, 0, 1].ravel()} == ({0, 1} if ext else {0, 1, 2})
    assert P // 2 in prb1[:-1] and (P - 1) // 2 in prb2[:-1] and threshold(spec) < prb1.shape[0]


@pytest.mark.parametrize("name", NAMES)
def test_pucch_resource_over_the_band(name):
    """srslte_hip_pucch_resource gives the recorded PRBs at every index, and refuses exactly the first index out of band."""
    g, spec = golden(), SWEEP_CELLS[name]
    cfg, mk = cfg_of(spec), pkg.PucchReq.make
    for fam, key in ((1, "f1_prb"), (2, "f2_prb")):
        prb = g["%s.%s" % (name, key)]
        for n in range(prb.shape[0]):
            q = mk(0, 0x46, ack_len=1, ncce=n - spec[7]) if fam == 1 else mk(0, 0x46, cqi_len=4, n_pucch_2=n)
            got = pkg.pucch_resource(cfg, q)
            if OOB in prb[n]:
                assert got is None and n == prb.shape[0] - 1, (fam, n, got)
            else:
                assert got == ((F1A if fam == 1 else F2), n, int(prb[n, 0]), int(prb[n, 1])), (fam, n, got)
        # the same resource through the SR selection
        q = mk(0, 0x46, sr_tti=True, n_pucch_sr=prb.shape[0] - 1, **(dict(cqi_len=4) if fam == 2 else {}))
        assert pkg.pucch_resource(cfg, q) is None
        q.n_pucch_sr -= 1
        assert pkg.pucch_resource(cfg, q)[1:] == (prb.shape[0] - 2, int(prb[-2, 0]), int(prb[-2, 1]))


@pytest.mark.parametrize("name", NAMES)
def test_pucch_dmrs_matches_recorded(name):
    """srslte_hip_pucch_dmrs against the reference's srslte_refsignal_dmrs_pucch_gen at every full-signal record, within the 1e-5 of the
    transmit tests (float phase sums in another order, libm against the reference's cexpf)."""
    g, spec = golden(), SWEEP_CELLS[name]
    cfg = cfg_of(spec)
    for i, m in enumerate(g[name + ".rec_meta"]):
        fmt, n, tti = int(m[0]), int(m[1]), int(m[2])
        drs = tuple(int(b) for b in g[name + ".rec_uci"][i, :2]) if fmt > F2 else (0, 0)
        got = pkg.pucch_dmrs(cfg, fmt, n, tti, drs).reshape(-1)
        assert got.size == g[name + ".dmrs_n"][i]
        assert np.abs(got - g[name + ".dmrs_r"][i, :got.size]).max() < 1e-5, (i, fmt, n)


def test_base_sequence_phases_recorded():
    """The 30 x 12 table of srslte_refsignal_r_uv_arg_1prb is 36.211 Table 5.5.1.2-1's phi pi / 4: odd multiples of pi / 4, and the row of
    every u the five cells use is what the host DMRS of a format 2 (w = 0) carries at n_cs_cell + n' = 0."""
    arg = golden()["r_uv_arg"]
    assert arg.shape == (30, 12) and np.array_equal(np.abs(np.round(arg / (np.pi / 4))) % 2, np.ones((30, 12)))
    assert np.abs(arg / np.float32(np.pi / 4) - np.round(arg / (np.pi / 4))).max() < 1e-6
    for name in ("S1", "S3"):  # no group hopping: u = cell_id % 30 in every slot
        spec = SWEEP_CELLS[name]
        cfg, ncc = cfg_of(spec), _n_cs_cell(spec)
        r = pkg.pucch_dmrs(cfg, F2, 0, 0)[0, 0]
        n_cs = alpha2(ncc, spec[5], spec[6], 0, 0, 3 if spec[2] else 1)
        want = np.exp(1j * (arg[spec[1] % 30].astype(np.float64) + float(ALPHA[n_cs]) * np.arange(12)))
        assert np.abs(r - want).max() < 1e-5, name


@needs_ref
@pytest.mark.parametrize("name", NAMES)
def test_restated_encoder_matches_recorded_grids(name):
    """RefUlCtrl.encode on a zeroed grid against srslte_pucch_encode + srslte_refsignal_dmrs_pucch_gen / _put: the same REs, values within 1e-5."""
    g, spec = golden(), SWEEP_CELLS[name]
    R = ref_of(spec)
    assert np.array_equal(R.arg, golden()["r_uv_arg"][[((int(R.f_gh[ns]) if spec[3] else 0) + spec[1] % 30) % 30 for ns in range(20)]])
    seen = set()
    for i, m in enumerate(g[name + ".rec_meta"]):
        want, idx = rec_grid(g, name, i, R.glen)
        got = al(np.zeros(R.glen, np.complex64))
        fmt = R.encode(got, int(m[2]), rec_tx(spec, m, g[name + ".rec_uci"][i]))
        assert fmt == int(m[0]), (i, fmt)
        assert np.array_equal(np.flatnonzero(got), idx), i
        assert np.abs(got - want).max() < 1e-5, (i, fmt, int(m[1]), np.abs(got - want).max())
        seen.add(fmt)
    assert len(seen) >= 4


@needs_ref
@pytest.mark.parametrize("name", NAMES)
def test_restated_decoder_matches_recorded_decisions(name):
    """RefUlCtrl.decode (the chain assembled from exported pieces) on the recorded grids against the reference's own
    srslte_chest_ul_estimate_pucch + srslte_pucch_decode: every decision and bit, the correlation within 1e-4 (formats 1-1b) or equal (2-2b)."""
    g, spec = golden(), SWEEP_CELLS[name]
    R = ref_of(spec)
    for i, m in enumerate(g[name + ".rec_meta"]):
        fmt, n, tti = int(m[0]), int(m[1]), int(m[2])
        grid, _ = rec_grid(g, name, i, R.glen)
        t = rec_tx(spec, m, g[name + ".rec_uci"][i])
        q = t.req
        q.noise_estimate = 0.0
        got = R.decode(al(grid), tti, q)
        det, a0, a1, valid, crc, ri, d0, d1 = (int(x) for x in g[name + ".dec"][i, :8])
        corr = float(g[name + ".dec_corr"][i])
        assert (got["format"], got["n_pucch"]) == (fmt, n), i
        if fmt >= F2:
            assert float(got["corr"]) == pytest.approx(corr, abs=1e-6), (i, fmt, n)
        else:
            assert abs(float(got["corr"]) - corr) < 1e-4, (i, fmt, n, got["corr"], corr)
        assert got["detected"] == det == 1 and got["ack"] == [a0, a1][:2] and got["ack_valid"] == valid, (i, fmt, got["ack"], a0, a1)
        assert got["ack"][:q.ack_len] == [int(b) for b in g[name + ".rec_uci"][i, :q.ack_len]], i  # noise-free: the bits sent
        if fmt >= F2:
            assert got["cqi_crc"] == crc and tuple(got["drs"]) == (d0, d1), i
            if q.ri_len:
                assert got["ri"] == ri == int(g[name + ".rec_uci"][i, 2]), i
            else:
                assert got["cqi"] == g[name + ".dec"][i, 8:].tolist(), i
                assert got["cqi"][:q.cqi_len] == g[name + ".rec_uci"][i, 3:3 + q.cqi_len].tolist(), i


@needs_ref
@pytest.mark.parametrize("name", NAMES)
def test_reference_alone_rarely_sits_on_a_threshold(name):
    """The receive sweep's scenes through RefUlCtrl.decode alone, with the threshold and tie rules of test_gpu_ul_ctrl._excluded: at most 1 % of a
    cell's requests lie within 1e-4 of a threshold or a tie, so the GPU test's 2 % has room for the device's LLR steps and none for hiding."""
    from test_gpu_ul_ctrl import _excluded
    total, excl, R = 0, collections.Counter(), None
    for family in (1, 2):
        for snr in SWEEP_SNRS:
            R, reqs, grid, tti0 = sweep_scene(name, family, snr, R)
            for q in reqs:
                want = R.decode(al(grid[q.sf]), tti0 + q.sf, q)
                why = _excluded(R, grid[q.sf], tti0 + q.sf, q, want, want["llr"])
                assert why != "llr"
                if why:
                    excl[why] += 1
            total += len(reqs)
    spec = SWEEP_CELLS[name]
    assert total == 2 * (last_in_band(spec, 1) + last_in_band(spec, 2) + 2)
    print("%s: %d requests, the reference alone sets aside %s" % (name, total, dict(excl)))
    assert sum(excl.values()) <= total // 100, (total, dict(excl))
