"""sizeof/offsetof of every public struct in include/srslte_hip/srslte_compat.h against the reference headers.
Callers embed these structs by value and poke their fields, so the layouts must be identical.
The reference's side is stored in tests/golden/ref_abi.json (tests/gen_golden.py --abi-only); where the reference headers are present the
stored data is checked against them too."""
import json
import os

from _libs import REF_ABI, REF_INC, ROOT, struct_layout

STRUCTS = {
    "srslte_cell_t": ["nof_prb", "nof_ports", "id", "cp", "phich_length", "phich_resources", "frame_type"],
    "srslte_dl_sf_cfg_t": ["tdd_config", "tti", "cfi", "sf_type", "non_mbsfn_region"],
    "srslte_dft_plan_t": ["init_size", "size", "in", "out", "p", "is_guru", "forward", "mirror", "db", "norm", "dc", "dir", "mode"],
    "srslte_ofdm_t": ["fft_plan", "fft_plan_sf", "max_prb", "nof_symbols", "symbol_sz", "nof_guards", "nof_re", "slot_sz", "sf_sz", "cp", "tmp",
                      "in_buffer", "out_buffer", "mbsfn_subframe", "mbsfn_guard_len", "nof_symbols_mbsfn", "non_mbsfn_region", "freq_shift",
                      "freq_shift_f", "shift_buffer"],
    "srslte_dft_precoding_t": ["max_prb", "dft_plan"],
    "srslte_cbsegm_t": ["F", "C", "K1", "K2", "K1_idx", "K2_idx", "C1", "C2", "tbs"],
    "srslte_tc_interl_t": ["forward", "reverse", "max_long_cb"],
    "srslte_tcod_t": ["max_long_cb", "temp"],
    "srslte_crc_t": ["table", "polynom", "order", "crcinit", "crcmask", "crchighbit", "srslte_crc_out"],
    "srslte_tdec_t": ["max_long_cb", "dec8_hdlr", "dec16_hdlr", "dec8", "dec16", "nof_blocks8", "nof_blocks16", "app1", "app2", "ext1", "ext2", "syst0",
                      "parity0", "parity1", "input_conv", "force_not_sb", "dec_type", "current_llr_type", "current_dec", "current_long_cb",
                      "current_inter_idx", "current_cbidx", "interleaver", "n_iter"],
    "srslte_refsignal_t": ["cell", "pilots", "type", "mbsfn_area_id"],
    "srslte_chest_dl_res_t": ["ce", "nof_re", "noise_estimate", "noise_estimate_dbm", "snr_db", "snr_ant_port_db", "rsrp", "rsrp_dbm", "rsrp_neigh",
                              "rsrp_port_dbm", "rsrp_ant_port_dbm", "rsrq", "rsrq_db", "rsrq_ant_port_db", "rssi_dbm", "cfo", "sync_error"],
    "srslte_chest_dl_t": ["cell", "nof_rx_antennas", "csr_refs", "mbsfn_refs", "pilot_estimates", "pilot_estimates_average", "pilot_recv_signal",
                          "tmp_noise", "tmp_cfo_estimate", "srslte_interp_linvec", "srslte_interp_lin", "srslte_interp_lin_3",
                          "srslte_interp_lin_mbsfn", "rssi", "rsrp", "rsrp_corr", "noise_estimate", "sync_err", "cfo", "pss_signal", "tmp_pss",
                          "tmp_pss_noisy"],
    "srslte_ra_tb_t": ["mod", "tbs", "rv", "nof_bits", "cw_idx", "enabled", "mcs_idx"],
    "srslte_pdsch_grant_t": ["tx_scheme", "pmi", "prb_idx", "nof_prb", "nof_re", "nof_symb_slot", "tb", "last_tbs", "nof_tb", "nof_layers"],
    "srslte_softbuffer_rx_t": ["max_cb", "buffer_f", "data", "cb_crc", "tb_crc"],
    "srslte_pdsch_cfg_t": ["grant", "rnti", "max_nof_iterations", "decoder_type", "p_a", "p_b", "rs_power", "power_scale", "csi_enable",
                           "use_tbs_index_alt", "softbuffers", "meas_time_en", "meas_time_value"],
    "srslte_uci_bit_t": ["position", "type"],
    "srslte_viterbi_t": ["ptr", "R", "K", "framebits", "tail_biting", "gain_quant", "gain_quant_s", "decode", "decode_s", "decode_f", "free", "tmp",
                         "tmp_s", "symbols_uc", "symbols_us"],
    "srslte_uci_cqi_pusch_t": ["crc", "viterbi", "tmp_cqi", "encoded_cqi", "encoded_cqi_s", "cqi_table", "cqi_table_s"],
    "srslte_sch_t": ["max_iterations", "avg_iterations", "llr_is_8bit", "cb_in", "parity_bits", "e", "temp_g_bits", "ul_interleaver", "ack_ri_bits",
                     "encoder", "decoder", "crc_tb", "crc_cb", "uci_cqi"],
    "srslte_chest_dl_cfg_t": ["noise_alg", "filter_type", "filter_coef", "mbsfn_area_id", "interpolate_subframe", "rsrp_neighbour",
                              "cfo_estimate_enable", "cfo_estimate_sf_mask", "sync_error_enable"],
}


REF_HEADERS = ["srslte/phy/dft/ofdm.h", "srslte/phy/dft/dft_precoding.h", "srslte/phy/fec/cbsegm.h", "srslte/phy/fec/tc_interl.h",
               "srslte/phy/fec/turbocoder.h", "srslte/phy/fec/turbodecoder.h", "srslte/phy/ch_estimation/chest_dl.h", "srslte/phy/phch/sch.h"]
# the eleven headers the boundary names
BOUNDARY_HEADERS = ["dft/dft", "dft/ofdm", "dft/dft_precoding", "fec/turbocoder", "fec/turbodecoder", "fec/tc_interl", "fec/cbsegm",
                    "ch_estimation/chest_dl", "ch_estimation/chest_common", "ch_estimation/refsignal_dl", "modem/demod_soft"]


def boundary_prototypes_from_headers():
    import re
    names = set()
    for h in BOUNDARY_HEADERS:
        src = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(os.path.join(REF_INC, "srslte/phy", h + ".h")).read(), flags=re.S)
        names.update(re.findall(r"SRSLTE_API\s+[^;{(]*?\b(srslte_[A-Za-z0-9_]+)\s*\(", src))
    return sorted(names)


def stored_abi():
    with open(REF_ABI) as f:
        return json.load(f)


def test_struct_layouts_match_reference():
    stored = stored_abi()["layouts"]
    names = list(STRUCTS) + ["%s.%s" % (st, f) for st, fs in STRUCTS.items() for f in fs]
    ref = {k: stored[k] for k in names}
    if os.path.isdir(REF_INC):
        assert struct_layout(STRUCTS, REF_HEADERS, [REF_INC]) == ref, "tests/golden/ref_abi.json is stale: tests/gen_golden.py --abi-only"
    ours = struct_layout(STRUCTS, ["srslte_hip/srslte_compat.h"], [os.path.join(ROOT, "include")])
    diff = {k: (ref[k], ours.get(k)) for k in ref if ref[k] != ours.get(k)}
    assert not diff, "layout differences (reference, ours): %s" % diff


def test_every_prototype_of_the_boundary_headers_is_exported():
    """'every SRSLTE_API prototype' of the eleven headers the boundary names - all of them, by name, in the product library
    (plus srslte_tc_interl_UMTS_gen, which row a6 cites and no header declares)."""
    import ctypes
    from _libs import HIP_SO
    names = set(stored_abi()["boundary_prototypes"])
    if os.path.isdir(REF_INC):
        assert sorted(names) == boundary_prototypes_from_headers(), "tests/golden/ref_abi.json is stale: tests/gen_golden.py --abi-only"
    assert len(names) >= 100, len(names)
    lib = ctypes.CDLL(HIP_SO)
    missing = sorted(n for n in names | {"srslte_tc_interl_UMTS_gen"} if not hasattr(lib, n))
    assert not missing, missing
