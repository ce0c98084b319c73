/*
 * include/srslte_hip/srslte_compat_pusch.h — the PUSCH receiver's hook of the link-time drop-in: srslte_pusch_decode with upstream's prototype
 * (phch/pusch.h:120-125, pusch.c:427-522), served by libsrslte_phy_hip.so as ONE device call per PUSCH (srslte_hip_pusch_decode, phy_hip.h).
 * A header of its own on top of srslte_compat.h: callers of that header have declared the small structs of the PUSCH interface themselves
 * (tests/ulsch_dropin_driver.c does), and C has no way to declare them twice.
 *
 * Upstream's srslte_pusch_decode, linked against the library, extracts the allocation twice and equalises on the CPU, enters the library for
 * the inverse transform precoding (copy in, launch, copy out, wait), again for the soft demapper, descrambles on the CPU, and a third time
 * through srslte_ulsch_decode, which copies the LLRs it has just received straight back up. Here only the allocation's rows of sf_symbols
 * and channel->ce go up (2 x nof_re x 8 bytes), and the call waits for its stream once when every code block passes (srslte_ulsch_decode's
 * second and third waits stay: the soft buffers of failed blocks, a report whose size depends on the rank decoded in the same call).
 *
 * Left as upstream leaves it, everything a caller can observe:
 *  - cfg->grant.tb.mod / nof_bits rewritten to 16QAM when enable_64qam is false and the grant is 64QAM (pusch.c:445-450);
 *  - out->crc, out->data (with its three CRC bytes), out->uci (ACK, RI, the report and its CRC flag), out->uci.ack.valid = snr_db > -1.0
 *    (ACK_SNR_TH), out->avg_iterations_block;
 *  - cfg->last_O_cqi, cfg->K_segm, cfg->uci_cfg.cqi.rank_is_not_one, and cfg->meas_time_value when meas_time_en is set;
 *  - the srslte_softbuffer_rx_t (buffer_f, cb_crc, data, tb_crc) exactly as srslte_ulsch_decode through the library writes it.
 * The return value is upstream's: SRSLTE_SUCCESS whatever the CRC says.
 * NOT written: q->d, q->z, q->ce, q->q and q->g - pusch.c's scratch, which nothing reads after the call - and q->ul_sch.ack_ri_bits. The
 * sequences of q->users are not read: the PUSCH's sequence is made on the device from cfg->rnti, sf->tti % 10 and q->cell.id, whether
 * srslte_pusch_set_rnti has generated the user's or not (upstream generates it into q->tmp_seq then).
 * The decoder object is the one behind q->ul_sch.decoder.dec16_hdlr[0], as srslte_ulsch_decode finds it; it grows on demand.
 *
 * Refusals: SRSLTE_ERROR_INVALID_INPUTS and one log line naming the reason, before anything is queued or written - cfg, out and the soft
 * buffer are untouched, so a forwarder can hand the same arguments to upstream's own function ("The PUSCH receiver's hook").
 * Upstream returns that code for NULL q / cfg / sf_symbols / out only, which the forwarder may hand on. Refused: everything
 * srslte_ulsch_decode refuses (srslte_compat.h); NULL sf, channel or channel->ce; objects with llr_is_8bit; a transport block size without a
 * segmentation; an L_prb that srslte_dft_precoding_valid_prb rejects; n_prb_tilde[s] + L_prb beyond the cell; nof_re other than
 * 12 L_prb nof_symb; nof_symb other than 2 N_symb - 2 - shortened; nof_bits other than nof_re Qm. One receive antenna, as upstream.
 */
#ifndef SRSLTE_HIP_SRSLTE_COMPAT_PUSCH_H
#define SRSLTE_HIP_SRSLTE_COMPAT_PUSCH_H

#include "srslte_hip/srslte_compat.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { srslte_tdd_config_t tdd_config; uint32_t tti; bool shortened; } srslte_ul_sf_cfg_t;                              /* phy_common.h:214-218 */
typedef struct { cf_t* ce; uint32_t nof_re; float noise_estimate; float noise_estimate_dbm; float snr; float snr_db; float cfo; } srslte_chest_ul_res_t; /* chest_ul.h:48-56 */
typedef struct { uint8_t* c; uint8_t* c_bytes; float* c_float; short* c_short; int8_t* c_char; uint32_t cur_len; uint32_t max_len; } srslte_sequence_t; /* sequence.h:37-45 */
typedef struct { /* modem_table.h:56-66 */
  cf_t* symbol_table; uint32_t nsymbols; uint32_t nbits_x_symbol; bool byte_tables_init;
  void* symbol_table_bpsk; void* symbol_table_qpsk; void* symbol_table_16qam; void* symbol_table_256qam;
} srslte_modem_table_t;
typedef struct { srslte_sequence_t seq[SRSLTE_NOF_SF_X_FRAME]; uint32_t cell_id; bool sequence_generated; } srslte_pusch_user_t; /* pusch.h:47-51 */
typedef struct { /* pusch.h:54-82 */
  srslte_cell_t cell; bool is_ue; uint16_t ue_rnti; uint32_t max_re; bool llr_is_8bit; srslte_dft_precoding_t dft_precoding;
  cf_t* ce; cf_t* z; cf_t* d; void* q; void* g;
  srslte_modem_table_t mod[4]; srslte_sch_t ul_sch; srslte_pusch_user_t** users; srslte_sequence_t tmp_seq;
} srslte_pusch_t;
typedef struct { uint8_t* data; srslte_uci_value_t uci; bool crc; float avg_iterations_block; } srslte_pusch_res_t;               /* pusch.h:89-94 */

int srslte_pusch_decode(srslte_pusch_t* q, srslte_ul_sf_cfg_t* sf, srslte_pusch_cfg_t* cfg, srslte_chest_ul_res_t* channel, cf_t* sf_symbols,
                        srslte_pusch_res_t* out);
/* {srslte_pusch_decode calls served, stream waits inside them} (the three other stats calls keep their shapes) */
void srslte_hip_compat_stats_pusch(unsigned long long out[2]);

#ifdef __cplusplus
}
#endif
#endif
