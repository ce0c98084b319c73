"""PUSCH UCI plan (phy_hip.h "PUSCH UCI plan"): how a PUSCH's symbols are divided between HARQ-ACK, rank indication, CQI report and UL-SCH."""
import ctypes as C

from ._native import P, lib

PUSCH_UCI_OK, PUSCH_UCI_EMPTY, PUSCH_UCI_BETA, PUSCH_UCI_ROWS, PUSCH_UCI_NO_ROOM = range(5)


class PuschUciCfg(C.Structure):
    """srslte_hip_pusch_uci_cfg_t."""
    C_TYPE = "srslte_hip_pusch_uci_cfg_t"
    _fields_ = [(n, C.c_uint32) for n in ("L_prb", "nof_symb", "Qm", "rows", "K_segm", "C", "ack_len", "ri_len", "cqi_len", "I_offset_ack",
                                          "I_offset_ri", "I_offset_cqi", "sym")]


class PuschUciRes(C.Structure):
    """srslte_hip_pusch_uci_res_t."""
    C_TYPE = "srslte_hip_pusch_uci_res_t"
    _fields_ = [(n, C.c_uint32) for n in ("Qp_ack", "Qp_ri", "Qp_cqi", "Q_cqi", "G_prime", "syms_lo", "C_lo")] + [("ack_pos", C.c_uint32 * 2),
                                                                                                                ("ri_pos", C.c_uint32 * 2)]


SIGNATURES = {
    "srslte_hip_pusch_uci_plan": (None, [P(PuschUciCfg), P(PuschUciRes)]),
}


def pusch_uci_plan(**cfg):
    """(reason, PuschUciRes) of srslte_hip_pusch_uci_plan for the fields of srslte_hip_pusch_uci_cfg_t given by name, without a device."""
    res = PuschUciRes()
    return lib().srslte_hip_pusch_uci_plan(C.byref(PuschUciCfg(**cfg)), C.byref(res)), res
