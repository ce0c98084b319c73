"""The PUSCHs tests/test_gpu_pusch_decode.py sends through srslte_hip_pusch_decode / srslte_pusch_decode, and what the oracle makes of them: stimulus
from lte_sim.make_ul_subframe, grid and estimates from the oracle's OFDM receiver and UL estimator, expectation from lte_sim.oracle_ul_rx (pinned
to the reference by tests/test_oracle_vs_ref.py). Nothing here needs a GPU: `python tests/pusch_decode_cases.py` prints, per case and
transmission, the oracle's verdict and its passes per block - the SNR of every passing case is chosen so that the oracle alone decodes each block
in at most half of max_iterations, which the GPU test asserts again before it compares.

The shapes are the smallest at which each thing can go wrong: the 12-point transform with one code block, a 1-bit ACK (c_seq from the device's
sequence) and a 4-bit report; L_prb 15 (radices 3 and 5) with intra-subframe hopping and 11 symbols, rv 0 - which cannot decode alone: 7920 LLRs for
15360 coded bits - then rv 2 into the same soft buffers; the extended CP with 10 and 9 symbols; 100 PRB 64QAM with 13 code blocks, bare and with a
2-bit ACK, an RI and a report whose size the decoded rank decides (6 bits at rank 1, 9 above: a higher-layer subband report with PMI and N = 0);
a PUSCH without data; an allocation at the cell's last PRBs.

Every report here has at most 11 bits. Above that upstream's decoder hands int16 soft bits to srslte_viterbi_decode_s, whose quantiser loses every
positive one (tests/test_oracle_vs_ref.py::test_reference_viterbi_decode_s_loses_positive_soft_bits); the call follows upstream there, as
srslte_hip_ulsch_decode does - tests/test_gpu_ulsch_decode.py holds that chain to the reference itself -, while the oracle decodes such a report
through the float entry point (oracle/orc_cqi.c), so the two differ by design."""
import numpy as np

from lte_sim import OrcHarq, UlConfig, make_ul_subframe, oracle_ul_rx, ul_ack_ri_qprime, ul_cqi_qprime

MAX_ITER = 6


def bits(n, seed):
    return tuple(int(b) for b in np.random.default_rng(seed).integers(0, 2, n))


# I: (I_offset_ack, I_offset_ri, I_offset_cqi); cqi: the report's bits; rank_len: (size at rank 1, size above) where the rank decides
CASES = {
    "6prb_L1_qpsk_ack1_cqi4": dict(P=6, mod=1, tbs=40, L=1, n_prb=(2, 2), ack=(1,), cqi=(1, 0, 1, 1), I=(5, 0, 6), snr=25.0, tti=1),
    "25prb_L15_16qam_hop_short": dict(P=25, mod=2, tbs=15264, L=15, n_prb=(0, 10), short=True, snr=30.0, tti=12, rvs=(0, 2), fails=(0,)),
    "15prb_ext_L9": dict(P=15, mod=2, tbs=1544, L=9, n_prb=(3, 3), ext=True, ack=(0, 1), ri=(1,), I=(9, 8, 0), snr=25.0, tti=3),
    "15prb_ext_L9_short": dict(P=15, mod=1, tbs=1544, L=9, n_prb=(6, 0), ext=True, short=True, ri=(0,), I=(0, 8, 0), snr=25.0, tti=24),
    "100prb_64qam": dict(P=100, mod=3, tbs=75376, L=100, n_prb=(0, 0), snr=40.0, tti=5),
    "100prb_64qam_ack2_ri_report": dict(P=100, mod=3, tbs=75376, L=100, n_prb=(0, 0), ack=(1, 0), ri=(1,), cqi=bits(9, 41), rank_len=(6, 9), I=(9, 12, 15),
                                        snr=40.0, tti=6),
    "no_data_report_only": dict(P=6, mod=1, tbs=0, L=2, n_prb=(1, 1), cqi=bits(8, 20), I=(0, 0, 6), snr=25.0, tti=7),
    "last_prbs": dict(P=6, mod=1, tbs=136, L=2, n_prb=(4, 4), snr=25.0, tti=8),
}
_cache = {}


def ul_config(c, mod=None):
    return UlConfig(c["P"], 1, mod or c["mod"], c["tbs"], c["L"], n_prb=c["n_prb"][0], n_prb_slot1=c["n_prb"][1], max_iter=MAX_ITER, shortened=c.get("short", False),
                    cp_ext=c.get("ext", False))


def expect(name):
    """-> (UlConfig, [per transmission: dict(rv, grid, ce, noise, q, tb, ok, cb_ok, iters, ack, ri, cqi, cqi_ok, Qp, w)], payload); computed once"""
    if name in _cache:
        return _cache[name]
    c = CASES[name]
    ul = ul_config(c)
    rng = np.random.default_rng(sum(name.encode()))
    ack, ri, cqi, I = c.get("ack", ()), c.get("ri", ()), c.get("cqi", ()), c.get("I", (0, 0, 0))
    harq = OrcHarq(ul) if c["tbs"] else None
    data, txs = None, []
    for k, rv in enumerate(c.get("rvs", (0,))):
        iq, data = make_ul_subframe(ul, c["tti"], rng, snr_db=c["snr"], data=data, ack=ack, I_offset_ack=I[0], ri=ri, I_offset_ri=I[1], cqi=cqi, I_offset_cqi=I[2],
                                    rv=rv)
        r = oracle_ul_rx(ul, iq, c["tti"], keep=True, O_ack=len(ack), I_offset_ack=I[0], O_ri=len(ri), I_offset_ri=I[1], O_cqi=len(cqi), I_offset_cqi=I[2],
                         harq=harq, rv=rv, new_data=k == 0)
        Qp_ri = ul_ack_ri_qprime(ul, len(ri), I[1], True, len(cqi), I[2])
        Qp = (ul_ack_ri_qprime(ul, len(ack), I[0], False, len(cqi), I[2]), Qp_ri, ul_cqi_qprime(ul, len(cqi), I[2], Qp_ri))
        txs.append(dict(rv=rv, grid=r["grid"].copy(), ce=r["ce"].copy(), noise=float(r["noise"]), q=r["q_before_ack"].copy(), tb=r["tb"].copy(), ok=r["ok"],
                        cb_ok=r["cb_ok"].copy(), iters=r["iters"].copy(), ack=r["ack"].copy(), ri=r["ri"].copy(), cqi=r["cqi"].copy(), cqi_ok=r["cqi_ok"], Qp=Qp,
                        w=None if harq is None else harq.w.copy()))
    _cache[name] = (ul, txs, data)
    return _cache[name]


if __name__ == "__main__":
    for n in CASES:
        ul, txs, _ = expect(n)
        for t in txs:
            print("%-32s rv %d ok %d blocks %s passes %s ack %s ri %s cqi_ok %d Q' %s" % (n, t["rv"], t["ok"], t["cb_ok"].tolist(), t["iters"].tolist(),
                                                                                        t["ack"].tolist(), t["ri"].tolist(), t["cqi_ok"], t["Qp"]))
