"""The structs srslte_ulsch_decode reads and writes, field by field, and the reference headers they come from: shared by
tests/test_ulsch_host.py and tests/gen_golden_ulsch_abi.py."""
INCLUDES = ["srslte/phy/phch/cqi.h", "srslte/phy/phch/uci_cfg.h", "srslte/phy/phch/pusch_cfg.h"]
FIELDS = {
    "srslte_cqi_hl_subband_t": ["wideband_cqi_cw0", "subband_diff_cqi_cw0", "wideband_cqi_cw1", "subband_diff_cqi_cw1", "pmi"],
    "srslte_cqi_ue_subband_t": ["wideband_cqi", "subband_diff_cqi", "position_subband"],
    "srslte_cqi_format2_wideband_t": ["wideband_cqi", "spatial_diff_cqi", "pmi"],
    "srslte_cqi_format2_subband_t": ["subband_cqi", "subband_label"],
    "srslte_cqi_cfg_t": ["data_enable", "ri_present", "pmi_present", "four_antenna_ports", "rank_is_not_one", "subband_label_2_bits", "L", "N", "type", "ri_len"],
    "srslte_cqi_value_t": ["wideband", "subband", "subband_ue", "subband_hl", "data_crc"],
    "srslte_uci_value_ack_t": ["ack_value", "valid"],
    "srslte_uci_cfg_ack_t": ["pending_tb", "nof_acks", "ncce", "N_bundle", "tdd_ack_M", "tdd_ack_m", "tdd_is_multiplex", "tpc_for_pucch", "grant_cc_idx"],
    "srslte_uci_cfg_t": ["ack", "cqi", "is_scheduling_request_tti"],
    "srslte_uci_value_t": ["scheduling_request", "cqi", "ack", "ri"],
    "srslte_uci_offset_cfg_t": ["I_offset_cqi", "I_offset_ri", "I_offset_ack"],
    "srslte_pusch_grant_t": ["is_from_rar", "L_prb", "n_prb", "n_prb_tilde", "freq_hopping", "nof_re", "nof_symb", "tb", "last_tb", "n_dmrs"],
    "srslte_pusch_cfg_t": ["rnti", "uci_cfg", "uci_offset", "grant", "max_nof_iterations", "last_O_cqi", "K_segm", "current_tx_nb", "csi_enable", "enable_64qam",
                           "softbuffers", "meas_time_en", "meas_time_value"],
}
