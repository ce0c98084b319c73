"""What tests/test_pucch_golden.py (CPU) and tests/test_gpu_pucch_sweep.py (GPU) share: the sweep cells and the fixture of
tests/gen_golden_pucch.py, the requests its full-signal records stand for, and the receive-sweep scenes (one UE per subframe, every in-band
n_pucch of a cell, the request kinds of tests/test_gpu_ul_ctrl.py cycled). Test infrastructure only."""
import importlib

import numpy as np

from _libs import aligned
from gen_golden_pucch import GOLDEN, OOB, STATE_SF, SWEEP_CELLS, TH, last_in_band, threshold  # noqa: F401
from ul_ctrl_ref import F1, F2, RefUlCtrl

pkg = importlib.import_module("srslte-emane_amd")
NAMES = sorted(SWEEP_CELLS)
F1_KINDS = ["sr", "ack", "dtx", "cqi_drop"]       # formats 1, 1a, 1b: "cqi_drop" is KINDS' cqi_ack without simul_cqi_ack
F2_KINDS = ["cqi", "ri", "cqi_ack", "ri_ack"]     # formats 2, 2a, 2b
SWEEP_SNRS = (30.0, 0.0)
_cache = {}


def golden():
    if "g" not in _cache:
        with np.load(GOLDEN) as z:
            _cache["g"] = {k: z[k] for k in z.files}
    return _cache["g"]


def kw(spec, **extra):
    return dict(cp_ext=spec[2], group_hopping_en=spec[3], delta_pucch_shift=spec[4], N_cs=spec[5], n_rb_2=spec[6], N_pucch_1=spec[7], **dict(TH, **extra))


def cfg_of(spec, **extra):
    return pkg.ul_ctrl_cfg(spec[0], spec[1], **kw(spec, **extra))


def ref_of(spec):
    return RefUlCtrl(cfg_of(spec))


def al(x):
    a = aligned(x.size, np.complex64)
    a[:] = x
    return a


def rec_tx(spec, meta, uci, sf=0):
    """The UE side of a full-signal record: the PucchTx whose selected (format, n_pucch) are the record's."""
    fmt, n, tti, sh, rnti, ack_len, cqi_len, ri_len = (int(x) for x in meta)
    ack, mk = (int(uci[0]), int(uci[1])), pkg.PucchReq.make
    if fmt == F1:
        return pkg.PucchTx.make(mk(sf, rnti, sr_tti=True, n_pucch_sr=n, shortened=bool(sh)), sr=1)
    if fmt < F2:
        return pkg.PucchTx.make(mk(sf, rnti, ack_len=ack_len, ncce=n - spec[7], shortened=bool(sh)), ack=ack)
    q = mk(sf, rnti, ack_len=ack_len, cqi_len=cqi_len, ri_len=ri_len, n_pucch_2=n, simul_cqi_ack=True, shortened=bool(sh))
    return pkg.PucchTx.make(q, ack=ack, ri=int(uci[2]), cqi=[int(b) for b in uci[3:3 + cqi_len]])


def rec_grid(g, name, i, glen):
    """The recorded subframe of record i: srslte_pucch_encode's REs, then the DMRS put over them (ue_ul.c's order; on the extended CP 2b's DMRS
    symbols are data symbols too). -> (grid, the indices written)."""
    out = np.zeros(glen, np.complex64)
    ne, nd = int(g[name + ".enc_n"][i]), int(g[name + ".dmrs_n"][i])
    out[g[name + ".enc_idx"][i, :ne]] = g[name + ".enc_val"][i, :ne]
    out[g[name + ".dmrs_idx"][i, :nd]] = g[name + ".dmrs_val"][i, :nd]
    return out, np.union1d(g[name + ".enc_idx"][i, :ne], g[name + ".dmrs_idx"][i, :nd])


def sweep_ue(rng, sf, n, other, kind, spec, shortened, rnti):
    """(the eNB's PucchReq, the UE's PucchTx or None) of subframe sf whose decoded resource is n_pucch = n; `other` is an in-band index that
    stays empty (the SR resource of an SR TTI in which the UE answers on the HARQ-ACK resource: the retry of enb_ul.c:217-224 then lands on n)."""
    N1 = spec[7]
    ack = (int(rng.integers(0, 2)), int(rng.integers(0, 2)))
    cqi_len = int(rng.integers(1, 13))
    cqi = [int(b) for b in rng.integers(0, 2, cqi_len)]
    mk = lambda **a: pkg.PucchReq.make(sf, rnti, shortened=shortened, **a)  # noqa: E731
    if kind == "sr":
        q = mk(sr_tti=True, n_pucch_sr=n)
        return q, (pkg.PucchTx.make(q, sr=1) if rng.random() < 0.7 else None)
    if kind == "ack":
        nack, how = int(rng.integers(1, 3)), int(rng.integers(0, 3))
        if how == 0:    # no SR TTI
            q = mk(ack_len=nack, ncce=n - N1)
            return q, pkg.PucchTx.make(q, ack=ack)
        if how == 1:    # SR TTI, positive SR: the ACK goes out on the SR resource
            q = mk(ack_len=nack, ncce=other - N1, sr_tti=True, n_pucch_sr=n)
            return q, pkg.PucchTx.make(q, ack=ack, sr=1)
        q = mk(ack_len=nack, ncce=n - N1, sr_tti=True, n_pucch_sr=other)  # SR TTI, no SR: found by the retry on the HARQ-ACK resource
        return q, pkg.PucchTx.make(mk(ack_len=nack, ncce=n - N1), ack=ack)
    if kind == "dtx":
        return mk(ack_len=int(rng.integers(1, 3)), ncce=n - N1), None
    if kind == "cqi_drop":
        q = mk(ack_len=int(rng.integers(1, 3)), cqi_len=cqi_len, ncce=n - N1)
        return q, pkg.PucchTx.make(q, ack=ack, cqi=cqi)
    if kind == "cqi":
        q = mk(cqi_len=cqi_len, n_pucch_2=n)
        return q, pkg.PucchTx.make(q, cqi=cqi)
    if kind == "ri":
        q = mk(ri_len=1, n_pucch_2=n)
        return q, pkg.PucchTx.make(q, ri=ack[0])
    if kind == "cqi_ack":
        q = mk(ack_len=int(rng.integers(1, 3)), cqi_len=cqi_len, simul_cqi_ack=True, n_pucch_2=n)
        return q, pkg.PucchTx.make(q, ack=ack, cqi=cqi)
    assert kind == "ri_ack"
    q = mk(ack_len=int(rng.integers(1, 3)), ri_len=1, n_pucch_2=n)
    return q, pkg.PucchTx.make(q, ack=ack, ri=int(rng.integers(0, 2)))


def sweep_seed(name, family, snr):
    return 7000 + 100 * NAMES.index(name) + 10 * family + SWEEP_SNRS.index(snr)


def sweep_scene(name, family, snr, R=None):
    """Every in-band n_pucch of a cell's format family, one UE per subframe, kinds cycled, AWGN at snr dB -> (R, reqs, grid [n][glen], tti0).
    The seed is sweep_seed's: both test files see the same scenes."""
    spec = SWEEP_CELLS[name]
    rng = np.random.default_rng(sweep_seed(name, family, snr))
    R = R or ref_of(spec)
    last = last_in_band(spec, family)
    kinds, tti0 = (F1_KINDS if family == 1 else F2_KINDS), int(rng.integers(0, 10240))
    reqs, grid = [], np.zeros((last + 1, R.glen), np.complex64)
    for n in range(last + 1):
        other = (n + last // 2 + 1) % (last + 1)
        q, t = sweep_ue(rng, n, n, other, kinds[(n + n // len(kinds)) % len(kinds)], spec, bool(rng.random() < 0.3), 0x46 + n)
        reqs.append(q)
        if t is not None:
            g = aligned(R.glen, np.complex64)
            R.encode(g, tti0 + n, t)
            grid[n] = g
    noise = np.float32(10 ** (-snr / 10))
    grid += (rng.normal(0, np.sqrt(noise / 2), grid.shape) + 1j * rng.normal(0, np.sqrt(noise / 2), grid.shape)).astype(np.complex64)
    for q in reqs:
        q.noise_estimate = float(noise) * float(rng.choice([0.0, 0.5, 1.0]))
    return R, reqs, grid, tti0
