"""What srslte_ulsch_encode reads and writes beyond the structs of tests/ulsch_abi.py, field by field, and the reference headers they come from:
shared by tests/test_ulsch_encode_host.py and tests/gen_golden_ulsch_enc_abi.py."""
INCLUDES = ["srslte/phy/phch/sch.h", "srslte/phy/phch/uci_cfg.h", "srslte/phy/fec/softbuffer.h"]
FIELDS = {
    "srslte_uci_bit_t": ["position", "type"],
    "srslte_sch_t": ["ack_ri_bits", "temp_g_bits", "cb_in", "parity_bits", "encoder"],
    "srslte_softbuffer_tx_t": ["max_cb", "buffer_b"],
    "srslte_uci_value_ack_t": ["ack_value"],
    "srslte_uci_value_t": ["cqi", "ack", "ri"],
    "srslte_cqi_value_t": ["wideband", "subband", "subband_ue", "subband_hl"],
}
