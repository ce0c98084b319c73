"""The structs srslte_pusch_decode takes beyond those of srslte_ulsch_decode (tests/ulsch_abi.py), field by field, the reference headers they come
from, and ctypes mirrors of the device call's own structs (phy_hip.h): shared by tests/test_pusch_decode_host.py, tests/gen_golden_pusch_abi.py
and the GPU tests."""
import ctypes as C

INCLUDES = ["srslte/phy/ch_estimation/chest_ul.h", "srslte/phy/phch/pusch.h"]  # in this order: pusch.h names the estimator's result
FIELDS = {
    "srslte_ul_sf_cfg_t": ["tdd_config", "tti", "shortened"],
    "srslte_chest_ul_res_t": ["ce", "nof_re", "noise_estimate", "noise_estimate_dbm", "snr", "snr_db", "cfo"],
    "srslte_sequence_t": ["c", "c_bytes", "c_float", "c_short", "c_char", "cur_len", "max_len"],
    "srslte_modem_table_t": ["symbol_table", "nsymbols", "nbits_x_symbol", "byte_tables_init", "symbol_table_bpsk", "symbol_table_qpsk", "symbol_table_16qam",
                             "symbol_table_256qam"],
    "srslte_pusch_user_t": ["seq", "cell_id", "sequence_generated"],
    "srslte_pusch_t": ["cell", "is_ue", "ue_rnti", "max_re", "llr_is_8bit", "dft_precoding", "ce", "z", "d", "q", "g", "mod", "ul_sch", "users", "tmp_seq"],
    "srslte_pusch_res_t": ["data", "uci", "crc", "avg_iterations_block"],
    "srslte_sch_t": ["max_iterations", "avg_iterations", "llr_is_8bit", "decoder", "crc_tb", "crc_cb"],
    "srslte_cell_t": ["nof_prb", "nof_ports", "id", "cp"],
}


class UlschCfg(C.Structure):
    """srslte_hip_ulsch_cfg_t"""
    _fields_ = [("mod", C.c_int)] + [(n, C.c_uint32) for n in ("tbs", "rv", "nof_bits", "L_prb", "nof_symb", "max_iterations", "ack_len", "ri_len", "cqi_len",
                                                               "I_offset_ack", "I_offset_ri", "I_offset_cqi", "cqi_len_rank2", "cqi_rank2")]


class PuschCfgHip(C.Structure):
    """srslte_hip_pusch_cfg_t"""
    _fields_ = [("sch", UlschCfg), ("nof_prb", C.c_uint32), ("cell_id", C.c_uint32), ("cp_ext", C.c_uint32), ("rnti", C.c_uint32), ("sf_idx", C.c_uint32),
                ("n_prb_tilde", C.c_uint32 * 2), ("shortened", C.c_uint32), ("nof_re", C.c_uint32)]


class UlschRes(C.Structure):
    """srslte_hip_ulsch_res_t"""
    _fields_ = [("ack", C.c_uint8 * 2), ("ri", C.c_uint8), ("cqi_bits", C.c_uint8 * 64), ("cqi_crc", C.c_uint8), ("cqi_len", C.c_uint32),
                ("Q_prime_ack", C.c_uint32), ("Q_prime_ri", C.c_uint32), ("Q_prime_cqi", C.c_uint32), ("stream_waits", C.c_uint32)]


def pusch_cfg(nof_prb, cell_id, mod, tbs, L_prb, n_prb_tilde, cp_ext=False, shortened=False, rnti=0x1234, sf_idx=0, rv=0, max_iterations=6, ack_len=0, ri_len=0,
              cqi_len=0, I=(0, 0, 0), cqi_len_rank2=0):
    """A srslte_hip_pusch_cfg_t whose derived fields (nof_symb, nof_re, nof_bits) are those of the allocation"""
    c = PuschCfgHip()
    nsymb = 2 * (6 if cp_ext else 7) - 2 - (1 if shortened else 0)
    s = c.sch
    s.mod, s.tbs, s.rv, s.L_prb, s.nof_symb, s.max_iterations = mod, tbs, rv, L_prb, nsymb, max_iterations
    s.nof_bits = 12 * L_prb * nsymb * 2 * mod
    s.ack_len, s.ri_len, s.cqi_len, s.cqi_len_rank2 = ack_len, ri_len, cqi_len, cqi_len_rank2
    s.I_offset_ack, s.I_offset_ri, s.I_offset_cqi = I
    c.nof_prb, c.cell_id, c.cp_ext, c.rnti, c.sf_idx, c.shortened, c.nof_re = nof_prb, cell_id, int(cp_ext), rnti, sf_idx, int(shortened), 12 * L_prb * nsymb
    c.n_prb_tilde[0], c.n_prb_tilde[1] = n_prb_tilde
    return c
