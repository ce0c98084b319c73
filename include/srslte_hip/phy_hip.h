/*
 * include/srslte_hip/phy_hip.h — batched C ABI of libsrslte_phy_hip.so (MI355X / gfx950).
 *
 * This is the throughput path of the drop-in (last row): device-resident buffers, one launch per
 * stage per batch of subframes. Every entry point is extern "C", takes plain pointers/sizes (device pointers are
 * marked d_), returns SRSLTE_SUCCESS 0 / SRSLTE_ERROR -1 / SRSLTE_ERROR_INVALID_INPUTS -2 (config.h:58-66) and
 * names the reference interface it replaces (paths relative to the reference tree).
 * The single-subframe srslte_* look-alikes that a caller such as lib/src/phy/ue/ue_dl.c binds are declared in
 * include/srslte_hip/srslte_compat.h and are thin host wrappers over these.
 *
 * Layouts (all cf_t = interleaved float re,im):
 *   time samples  [nof_sf][15*N]            N = srslte_symbol_sz(nof_prb)
 *   resource grid [nof_sf][nsym][12*prb]    nsym = 14 (normal CP) / 12, sub-carrier ascending, DC removed
 *   LLRs          [nof_sf][nof_re*Qm]       bit order b0(I) b1(Q) b2 ... as demod_soft.c
 */
#ifndef SRSLTE_HIP_PHY_HIP_H
#define SRSLTE_HIP_PHY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ device plumbing (no HIP headers needed by callers) */
int   srslte_hip_device_count(void);
int   srslte_hip_set_device(int device);
void* srslte_hip_malloc(size_t nbytes);
void  srslte_hip_free(void* d_ptr);
int   srslte_hip_memcpy_h2d(void* d_dst, const void* h_src, size_t nbytes);
int   srslte_hip_memcpy_d2h(void* h_dst, const void* d_src, size_t nbytes);
int   srslte_hip_memset(void* d_dst, int value, size_t nbytes);
int   srslte_hip_sync(void);
void* srslte_hip_stream_create(void);
void  srslte_hip_stream_destroy(void* stream);
int   srslte_hip_stream_sync(void* stream);
void* srslte_hip_event_create(void);                      /* HIP events on the caller's stream, for kernel timing */
int   srslte_hip_event_record(void* event, void* stream);
float srslte_hip_event_elapsed_ms(void* start, void* stop);
void  srslte_hip_event_destroy(void* event);
/* The single-call (compat) layer gives every host thread its own stream (SURVEY 8b "Threading": one object per worker thread, calls from
 * several threads at once). Returns the CALLING thread's stream, created on first use, and its hipStreamGetFlags value in *flags. */
void* srslte_hip_compat_thread_stream(unsigned* flags);
/* Counters of the compat layer since process start: [0] stream waits (one per synchronous call), [1] srslte_dlsch_decode2 calls served by the
 * device pipeline, [2] single-code-block decoder calls (srslte_tdec_run_all / _iteration), [3] srslte_dlsch_encode2 calls served by the device pipeline. With SRSLTE_HIP_STATS set in the
 * environment the library prints them to stderr at exit ("[srslte_hip] stats: ..."): how a caller's processes used the boundary. */
void  srslte_hip_compat_stats(unsigned long long out[4]);

/* ------------------------------------------------------------------ OFDM (replaces srslte_ofdm_rx_sf / srslte_ofdm_tx_sf,
 * lib/include/srslte/phy/dft/ofdm.h:82-153, lib/src/phy/dft/ofdm.c:384-594, and FFTW behind dft_fftw.c) */
typedef struct srslte_hip_ofdm srslte_hip_ofdm_t;
srslte_hip_ofdm_t* srslte_hip_ofdm_create(int nof_prb, int cp_is_norm, int is_rx);     /* ofdm.c:235-273 */
/* the same with the symbol size given, as srslte_ofdm_init_ takes it (ofdm.c:38-57): srslte_symbol_sz(nof_prb) of either rate family - 128 / 256 /
 * 384 / 768 / 1024 / 1536, or 128 / 256 / 512 / 1024 / 1536 / 2048 with srslte_use_standard_symbol_size(true) (phy_common.c:304-345) */
srslte_hip_ofdm_t* srslte_hip_ofdm_create_sz(int nof_prb, int symbol_sz, int cp_is_norm, int is_rx);
void               srslte_hip_ofdm_destroy(srslte_hip_ofdm_t* q);                      /* ofdm.c:214-233 */
int                srslte_hip_ofdm_set_normalize(srslte_hip_ofdm_t* q, int enable);    /* ofdm.c:576-578 */
int                srslte_hip_ofdm_set_freq_shift(srslte_hip_ofdm_t* q, float shift);  /* ofdm.c:360-378 */
int                srslte_hip_ofdm_symbol_sz(const srslte_hip_ofdm_t* q);
int                srslte_hip_ofdm_sf_len(const srslte_hip_ofdm_t* q);
int srslte_hip_ofdm_rx_sf_batch(srslte_hip_ofdm_t* q, const void* d_in_time, void* d_out_grid, int nof_sf, void* stream); /* ofdm.c:453-467 */
int srslte_hip_ofdm_tx_sf_batch(srslte_hip_ofdm_t* q, const void* d_in_grid, void* d_out_time, int nof_sf, void* stream); /* ofdm.c:580-594 */
/* MBSFN subframe layout on an extended-CP object (srslte_ofdm_{rx,tx}_init_mbsfn + srslte_ofdm_set_non_mbsfn_region,
 * ofdm.c:120-137,:248-258,:286-305; slot layout of srslte_ofdm_rx_slot_mbsfn :424-437 / srslte_ofdm_tx_slot_mbsfn :558-574).
 * The samples of the guard between the two regions are neither read (rx) nor written (tx). */
int srslte_hip_ofdm_set_mbsfn(srslte_hip_ofdm_t* q, int enable, int non_mbsfn_region);
/* one slot of each subframe (srslte_ofdm_rx_slot/_tx_slot ofdm.c:398-422,:488-530; mbsfn_layout=1: the MBSFN slot-0 layout);
 * rx or tx according to the object; d_in/d_out are subframe bases as in the _sf_batch calls */
int srslte_hip_ofdm_slot_batch(srslte_hip_ofdm_t* q, const void* d_in, void* d_out, int nof_sf, int slot_in_sf, int mbsfn_layout, void* stream);

/* ------------------------------------------------------------------ Sample formats
 * The radios the reference drives deliver and accept int16 pairs; its bladeRF path runs srslte_vec_convert_if(rx_buffer, 2048, data, 2 * nsamples)
 * after every receive and srslte_vec_convert_fi(data, 2048, tx_buffer, 2 * nsamples) before every send (lib/src/phy/rf/rf_blade_imp.c:443,:485;
 * bodies in lib/src/phy/utils/vector_simd.c:362-427). An OFDM object does either conversion inside its kernel, so that a caller moves 4 bytes per
 * sample over the link instead of 8 and touches no sample on the CPU. The format belongs to the object and concerns its TIME-DOMAIN side only:
 * d_in_time of srslte_hip_ofdm_rx_sf_batch / d_in of srslte_hip_ofdm_slot_batch on a receive object, d_out_time / d_out on a transmit object.
 *   SRSLTE_HIP_IQ_CF32  interleaved float re, im: 8 bytes per sample (the default; scale is not used)
 *   SRSLTE_HIP_IQ_SC16  interleaved int16 I, Q: 4 bytes per sample, same layouts counted in samples ([nof_sf][15 N])
 * Receive, sc16: each component is (float)x * gain with gain = 1.0f / scale computed once on the host, the product rounded to fp32 before the
 * half-carrier shift or the transform sees it: srslte_vec_convert_if (vector_simd.c:362-390) in the load. The grid is bit for bit that of the
 * cf32 call on the converted samples.
 * Transmit, sc16: each component of the cf32 value the object would store (after 1/sqrt(N) and the half-carrier shift), cyclic prefix
 * included, goes through the vector body of srslte_vec_convert_fi (vector_simd.c:395-422, srslte_simd_convert_2f_s simd.h:1681-1686 in the
 * reference's AVX2 build: mul, cvttps_epi32, packs_epi32): multiplied by scale and rounded to fp32, truncated towards zero, saturated to
 * [-32768, 32767]; a product that is not finite or whose magnitude is 2^31 or more gives -32768 (the conversion's "integer indefinite", packed).
 * The reference's scalar tail, (int16_t)(x * scale) at vector_simd.c:424-426, does not saturate; it only touches the last
 * len % SRSLTE_SIMD_S_SIZE values, and a subframe (2 * 15 N floats, N >= 128) has none. Guard samples of an MBSFN layout stay unwritten.
 * format outside the two, or a scale that is not finite and > 0: SRSLTE_ERROR_INVALID_INPUTS, object unchanged. The format may be switched
 * between calls (a call uses the format set when it is made). The pipelines forward it: srslte_hip_{dl,ul}_{rx,tx}_set_iq_format and
 * srslte_hip_dl_rx_pool_set_iq_format below. cf32 only: the single-call API of srslte_compat.h (srslte_ofdm_rx_sf and friends), synchronisation
 * (srslte_hip_sync_*, srslte_hip_nbiot_sync_*), neighbour-cell measurement, PRACH and the channel emulator. */
#define SRSLTE_HIP_IQ_CF32 0
#define SRSLTE_HIP_IQ_SC16 1 /* int16 I, int16 Q interleaved, 4 bytes per sample */
int srslte_hip_ofdm_set_sample_format(srslte_hip_ofdm_t* q, int format, float scale);

/* generic batched c2c DFT (replaces srslte_dft_run_guru_c, dft.h:137-152, dft_fftw.c:137-165,307-313) */
int srslte_hip_dft_batch(const void* d_in, void* d_out, int N, int howmany, int idist, int odist, int forward, float scale, void* stream);
/* SC-FDMA transform precoding (replaces srslte_dft_precoding, dft_precoding.h:39-64, dft_precoding.c:88-113) */
int srslte_hip_dft_precoding_valid_prb(uint32_t nof_prb);
int srslte_hip_dft_precoding_batch(const void* d_in, void* d_out, uint32_t nof_prb, uint32_t nof_symbols, int forward, void* stream);

/* ------------------------------------------------------------------ DL channel estimator (replaces srslte_chest_dl_estimate_cfg,
 * ch_estimation/chest_dl.h:49-156, chest_dl.c:598-908) */
typedef struct srslte_hip_chest_dl srslte_hip_chest_dl_t;
typedef struct {             /* same members, order and meaning as srslte_chest_dl_cfg_t (chest_dl.h:116-130) */
  int      noise_alg;        /* 0 REFS, 1 PSS, 2 EMPTY (chest_dl.h:85-89); PSS / EMPTY renew the estimate in subframes 0 and 5 and report the
                              * kept one otherwise, carried through the batch in subframe order and between calls on the object */
  int      filter_type;      /* 0 GAUSS, 1 TRIANGLE, 2 NONE (chest_common.h:30-34) */
  float    filter_coef[2];
  uint16_t mbsfn_area_id;
  uint8_t  interpolate_subframe;
  uint8_t  rsrp_neighbour;
  uint8_t  cfo_estimate_enable;
  uint32_t cfo_estimate_sf_mask;
  uint8_t  sync_error_enable;
} srslte_hip_chest_dl_cfg_t;
typedef struct {             /* scalar members of srslte_chest_dl_res_t (chest_dl.h:49-67), one per subframe */
  float noise_estimate, noise_estimate_dbm, snr_db, rsrp, rsrp_dbm, rsrq, rsrq_db, rssi_dbm, cfo, sync_error;
} srslte_hip_chest_dl_res_t;
/* cp_is_norm = 0: extended-CP cell, 12 symbols per subframe: every "[14]" below reads "[12]" then (CRS on symbols 0, 3, 6, 9; chest_dl.c:497-502) */
srslte_hip_chest_dl_t* srslte_hip_chest_dl_create(uint32_t cell_id, uint32_t nof_prb, uint32_t nof_ports, int cp_is_norm); /* chest_dl.c:69-160,193-300 */
/* TDD cell (srslte_cell_t.frame_type = SRSLTE_TDD; sf_config / ss_config = srslte_tdd_config_t of srslte_dl_sf_cfg_t, phy_common.h:381-388): special
 * subframes are estimated from the CRS symbols their DwPTS holds (refsignal_dl.c:162-225). sf_config < 0: FDD again. */
int srslte_hip_chest_dl_set_tdd(srslte_hip_chest_dl_t* q, int sf_config, int ss_config);
void                   srslte_hip_chest_dl_destroy(srslte_hip_chest_dl_t* q);
/* the symbol size the CFO and timing-error estimates scale with (chest_dl.c:575,:695: srslte_symbol_sz(cell.nof_prb), read at every call);
 * default: the default rate family's; e.g. 2048 for 100 PRB after srslte_use_standard_symbol_size(true) */
int                    srslte_hip_chest_dl_set_symbol_sz(srslte_hip_chest_dl_t* q, int symbol_sz);
const void*            srslte_hip_chest_dl_pilots(const srslte_hip_chest_dl_t* q); /* device CRS table [10][4][2*prb] (refsignal_dl.c:66-116) */
int srslte_hip_chest_dl_estimate_batch(srslte_hip_chest_dl_t* q, const srslte_hip_chest_dl_cfg_t* cfg, uint32_t tti0, const void* d_grid,
                                       void* d_ce, void* d_res, int nof_sf, void* stream);
/* nof_rx receive antennas x the object's 1 or 2 tx ports (chest_dl.c:884-908 loops over antennas and ports; fill_res :747-871
 * combines them): d_grid is [nof_sf][nof_rx][14][12*nof_prb], d_ce [nof_sf][nof_ports][nof_rx][14][12*nof_prb], d_res stays one
 * entry per subframe. 4-port cells: not with cfg->interpolate_subframe (upstream's result is undefined there, chest_dl.c:467-471). */
int srslte_hip_chest_dl_estimate_batch_multi(srslte_hip_chest_dl_t* q, const srslte_hip_chest_dl_cfg_t* cfg, uint32_t tti0, const void* d_grid,
                                             void* d_ce, void* d_res, int nof_sf, int nof_rx, void* stream);
/* device pointer to [nof_sf][nof_ports][nof_rx] x {noise_estimate, rsrp, rssi, cfo, sync_err, rsrp_corr} (6 floats) of the last call
 * with d_res: the per-antenna / per-port terms of fill_res (chest_dl.c:860-870) and of get_rsrp_neighbour (:821-843) */
const float* srslte_hip_chest_dl_last_raw(const srslte_hip_chest_dl_t* q);
/* MBSFN subframes (srslte_chest_dl_set_mbsfn_area_id chest_dl.c:244-262 with the reference signal of refsignal_dl.c:361-400,
 * estimate_port_mbsfn :718-745 and the MBSFN branches of :304-556). 1- and 2-port cells, cfg->interpolate_subframe set (the reference's
 * result without it is undefined), area id from cfg->mbsfn_area_id. d_grid [nof_sf][nof_rx][14][12*nof_prb] holds the 12 symbols of
 * the extended-CP subframe; d_ce [nof_sf][nof_ports][nof_rx][14][12*nof_prb] gets symbols 0-11. d_noise (or NULL):
 * [nof_sf][nof_ports][nof_rx] REFS noise estimates, written only with cfg->noise_alg == REFS. As in the reference an MBSFN subframe
 * measures nothing else: rsrp, rssi, cfo and the sync error keep the values of the last normal subframe (the compat layer keeps them). */
int         srslte_hip_chest_dl_set_mbsfn_area_id(srslte_hip_chest_dl_t* q, uint16_t mbsfn_area_id);
const void* srslte_hip_chest_dl_mbsfn_pilots(const srslte_hip_chest_dl_t* q, uint16_t mbsfn_area_id); /* device [10][3][6*nof_prb] or NULL */
int srslte_hip_chest_dl_estimate_mbsfn_batch(srslte_hip_chest_dl_t* q, const srslte_hip_chest_dl_cfg_t* cfg, uint32_t tti0, const void* d_grid,
                                             void* d_ce, float* d_noise, int nof_sf, int nof_rx, void* stream);

/* ------------------------------------------------------------------ UL channel estimator (replaces
 * srslte_chest_ul_init/_set_cell/_pregen/_estimate_pusch, ch_estimation/chest_ul.h:47-104, chest_ul.c:51-327, and the PUSCH DMRS of
 * refsignal_ul.c:118-487). Normal CP, grants of >= 1 PRB (the 1- and 2-PRB base sequences from the tables of 36.211 5.5.1.2), same
 * allocation in both slots (the reference's estimator does not support intra-subframe hopping either, chest_ul.c:297-299). */
typedef struct srslte_hip_chest_ul srslte_hip_chest_ul_t;
typedef struct { /* srslte_refsignal_dmrs_pusch_cfg_t, refsignal_ul.h:46-51 */
  uint32_t cyclic_shift, delta_ss;
  int      group_hopping_en, sequence_hopping_en;
} srslte_hip_dmrs_pusch_cfg_t;
typedef struct { /* scalar part of srslte_chest_ul_res_t */
  float noise_estimate, noise_estimate_dbm, snr, snr_db, cfo;
} srslte_hip_chest_ul_res_t;
srslte_hip_chest_ul_t* srslte_hip_chest_ul_create(uint32_t cell_id, uint32_t nof_prb, int cp_is_norm, const srslte_hip_dmrs_pusch_cfg_t* cfg);
void                   srslte_hip_chest_ul_destroy(srslte_hip_chest_ul_t* q);
/* srslte_refsignal_dmrs_pusch_gen (refsignal_ul.c:459-487): r_host [2][12*L_prb] cf32 in HOST memory */
int srslte_hip_refsignal_dmrs_pusch_gen(const srslte_hip_chest_ul_t* q, uint32_t L_prb, uint32_t sf_idx, uint32_t n_dmrs, void* r_host);
/* d_grid [nof_sf][14][12*nof_prb]; d_ce same shape or NULL - only the granted PRBs are written, as upstream; d_res [nof_sf] or NULL;
 * subframe b is TTI tti0 + b; one grant (L_prb, n_prb, n_dmrs) for the batch */
int srslte_hip_chest_ul_estimate_pusch_batch(srslte_hip_chest_ul_t* q, uint32_t tti0, uint32_t L_prb, uint32_t n_prb, uint32_t n_dmrs,
                                             const void* d_grid, void* d_ce, void* d_res, int nof_sf, void* stream);
/* the same with a PRB offset per slot (srslte_pusch_grant_t.n_prb[0 / 1], intra-subframe hopping: chest_ul.c:244-266,:293-295) */
int srslte_hip_chest_ul_estimate_pusch_batch_hop(srslte_hip_chest_ul_t* q, uint32_t tti0, uint32_t L_prb, uint32_t n_prb, uint32_t n_prb_slot1,
                                                 uint32_t n_dmrs, const void* d_grid, void* d_ce, void* d_res, int nof_sf, void* stream);

/* ------------------------------------------------------------------ soft demapper (replaces srslte_demod_soft_demodulate{,_s,_b},
 * modem/demod_soft.h:39-53, demod_soft.c:479-549). mod: 0 BPSK, 1 QPSK, 2 16QAM, 3 64QAM, 4 256QAM (srslte_mod_t).
 * ncalls independent calls of nsymbols each (the scalar-tail rounding of the reference depends on nsymbols). */
int srslte_hip_demod_soft_demodulate_batch(int mod, const void* d_symbols, float* d_llr, int nsymbols, int ncalls, void* stream);
int srslte_hip_demod_soft_demodulate_s_batch(int mod, const void* d_symbols, short* d_llr, int nsymbols, int ncalls, void* stream);
int srslte_hip_demod_soft_demodulate_b_batch(int mod, const void* d_symbols, int8_t* d_llr, int nsymbols, int ncalls, void* stream);

/* ------------------------------------------------------------------ turbo decoder (replaces srslte_tdec_run_all / srslte_tdec_iteration,
 * fec/turbodecoder.h:63-135, turbodecoder.c:146-593, turbodecoder_iter.h:71-139, turbodecoder_win.h, turbodecoder_gen.c) */
typedef struct srslte_hip_tdec srslte_hip_tdec_t;
srslte_hip_tdec_t* srslte_hip_tdec_create(uint32_t max_long_cb, uint32_t max_nof_cb);
void               srslte_hip_tdec_destroy(srslte_hip_tdec_t* q);
uint32_t           srslte_hip_tdec_autoimp_get_subblocks(uint32_t long_cb);           /* turbodecoder.c:394-406 */
uint32_t           srslte_hip_tdec_input_len(uint32_t long_cb, int sb_layout);        /* int16 per code block */
/* Decodes nof_cb code blocks of equal length long_cb.
 *   d_input: [nof_cb][in_stride] int16; layout = [s p0 p1]*K + 12 tail (sb_layout = 0, srslte_tdec_force_not_sb)
 *            or the rm_turbo "SB" layout 3*(K+32)+12 (sb_layout = 1; turbodecoder_iter.h:84-91)
 *   nof_iterations: SISO passes (one srslte_tdec_iteration each)
 *   crc_poly: 0 = run all passes (srslte_tdec_run_all); else stop a block at the first pass whose hard decision has
 *             a zero CRC-24 remainder over crc_nbits bits (sch.c:353-383)
 *   d_output: [nof_cb][out_stride] bytes, K/8 per block, MSB first; d_iters/d_crc_ok: [nof_cb] or NULL */
int srslte_hip_tdec_run_batch(srslte_hip_tdec_t* q, const int16_t* d_input, uint32_t in_stride, int sb_layout, uint32_t long_cb,
                              uint32_t nof_cb, uint32_t nof_iterations, uint32_t crc_poly, uint32_t crc_nbits, uint8_t* d_output,
                              uint32_t out_stride, uint32_t* d_iters, uint8_t* d_crc_ok, void* stream);

/* srslte_tdec_init_manual equivalent (turbodecoder.c:168-215): nof_subblocks 0 = generic, 8 = sse16, 16 = avx16 numerics on any K */
int srslte_hip_tdec_run_batch_manual(srslte_hip_tdec_t* q, const int16_t* d_input, uint32_t in_stride, int sb_layout, uint32_t long_cb,
                                     uint32_t nof_subblocks, uint32_t nof_cb, uint32_t nof_iterations, uint32_t crc_poly, uint32_t crc_nbits,
                                     uint8_t* d_output, uint32_t out_stride, uint32_t* d_iters, uint8_t* d_crc_ok, void* stream);

/* 8-bit LLRs (replaces srslte_tdec_run_all_8bit / srslte_tdec_iteration_8bit, turbodecoder.h:117-135, turbodecoder.c:438-469,
 * :565-593). Back-end per K as AUTO selects on an AVX2 host: K > 2048 avx8 (32 windows), K > 800 sse8 (16 windows)
 * - saturating int8, max-normalisation every step, output >> 1 (turbodecoder_win.h:92-173) - and below that the LLRs are widened
 * and the 16-bit back-ends run. sb_layout as above with 8-bit elements (srslte_rm_turbo_rx_lut_8bit output). */
uint32_t srslte_hip_tdec_autoimp_get_subblocks_8bit(uint32_t long_cb); /* turbodecoder.c:421-436 */
int srslte_hip_tdec_run_batch_8bit(srslte_hip_tdec_t* q, const int8_t* d_input, uint32_t in_stride, int sb_layout, uint32_t long_cb,
                                   uint32_t nof_cb, uint32_t nof_iterations, uint32_t crc_poly, uint32_t crc_nbits, uint8_t* d_output,
                                   uint32_t out_stride, uint32_t* d_iters, uint8_t* d_crc_ok, void* stream);

/* ------------------------------------------------------------------ turbo encoder (replaces srslte_tcod_encode, fec/turbocoder.h:44-76,
 * turbocoder.c:76-186): bits in (one per byte) -> 3K+12 bits out ([s p0 p1] triplets + 12 tail), nof_cb blocks */
int srslte_hip_tcod_encode_batch(const uint8_t* d_input, uint8_t* d_output, uint32_t long_cb, uint32_t nof_cb, void* stream);
/* byte-packed form (replaces the encoder proper of srslte_tcod_encode_lut, turbocoder.c:189-367; the CRC attachment of that
 * call stays with the caller): d_input [nof_cb][in_stride] K/8 bytes MSB first; d_parity [nof_cb][par_stride] K/4+1 bytes =
 * p1[K] t1[4] p2[K] t2[4] as one bit stream; d_sys_tail [nof_cb] = the byte the reference stores in input[K/8] */
int srslte_hip_tcod_encode_bytes_batch(const uint8_t* d_input, uint32_t in_stride, uint8_t* d_parity, uint32_t par_stride, uint8_t* d_sys_tail,
                                       uint32_t long_cb, uint32_t nof_cb, void* stream);

/* ------------------------------------------------------------------ segmentation / interleaver (host, replaces cbsegm.c, tc_interl_lte.c) */
typedef struct { /* same members and order as srslte_cbsegm_t (cbsegm.h:33-44) */
  uint32_t F, C, K1, K2, K1_idx, K2_idx, C1, C2, tbs;
} srslte_hip_cbsegm_t;
int srslte_hip_cbsegm(srslte_hip_cbsegm_t* s, uint32_t tbs);
int srslte_hip_cbsegm_cbindex(uint32_t long_cb);
int srslte_hip_cbsegm_cbsize(uint32_t index);
int srslte_hip_tc_interl_LTE_gen_interl(uint16_t* forward, uint16_t* reverse, uint32_t long_cb, uint32_t interl_win);

/* ------------------------------------------------------------------ PDSCH receive pipeline (SURVEY §8f N1 glue fused on device):
 * OFDM RX -> chest_dl -> RE extraction + one-tap MMSE -> soft demap + descramble -> turbo rate de-matching ->
 * turbo decode with CRC early stop -> TB CRC. One codeword, TM1 (single port) or TM2 (2-port transmit diversity), 1..4 rx antennas,
 * full-band grant, rv 0, FDD, normal CP. */
typedef struct srslte_hip_dl_rx srslte_hip_dl_rx_t;
typedef struct {
  uint32_t cell_id, nof_prb, cfi;
  uint16_t rnti;
  int      mod;            /* srslte_mod_t */
  uint32_t tbs;            /* transport block size, bits */
  uint32_t max_iterations; /* SISO passes, sch.c:114 */
  uint32_t max_batch;      /* subframes per call */
  int      mmse;           /* 1: noise_estimate from chest (pdsch.c:862), 0: ZF */
  srslte_hip_chest_dl_cfg_t chest_cfg;
  int      llr_8bit;       /* 1: the 8-bit LLR path the applications select (q->llr_is_8bit: pdsch.c:760-779 demod_b + int8
                              descrambling, sch.c:336-356 srslte_rm_turbo_rx_lut_8bit + srslte_tdec_iteration_8bit) */
  uint32_t nof_rx_antennas; /* 0 or 1: one antenna; 2..4: per-antenna estimation + srslte_predecoding_single_multi (precoding.c:325-348,
                               pdsch.c:890-935); d_iq / d_grid are then [nof_sf][nof_rx][...] */
  uint32_t nof_ports;       /* 0 or 1: single antenna port (TM1); 2 or 4: cell with that many ports and transmit diversity (TM2): multi-port
                               chest_dl and RE mapping, srslte_predecoding_diversity_multi + srslte_layerdemap_diversity (precoding.c:564-650,
                               layermap.c:140-148), for nof_rx_antennas 1..4; 4 ports: not with
                               chest_cfg.interpolate_subframe */
  int      csi_enable;      /* srslte_pdsch_cfg_t.csi_enable (pdsch_cfg.h:63; the srsUE default): LLRs weighted by each symbol's channel
                               gain relative to the subframe's largest (csi_correction, pdsch.c:574-690, applied inside the rate
                               de-matching kernels as they read the LLRs) */
  int      power_scale;     /* srslte_pdsch_cfg_t.power_scale / p_a (pdsch_cfg.h:58-62, pdsch.c:518-554,:852-858): the equaliser divides by
                               rho_a = 10^(p_a/20) (x sqrt(2) for a 2-port cell). Only p_b values with rho_b = 1 (no rescaling of the
                               CRS-bearing symbols) are covered */
  float    p_a;             /* dB */
  int      tx_scheme;       /* 0: by nof_ports as above. srslte_tx_scheme_t of the grant for the two-layer modes of a 2-port cell received with 2
                               antennas: SRSLTE_TXSCHEME_CDD (3): large-delay CDD, TM3, two transport blocks
                               (srslte_predecoding_ccd_2x2_mmse_csi, precoding.c:918-1014); SRSLTE_TXSCHEME_SPATIALMUX (2): closed-loop
                               multiplexing, TM4, two transport blocks with pmi 0-1 (srslte_predecoding_multiplex_2x2_mmse_csi :1326-1438) or
                               one with pmi 0-3 (srslte_predecoding_multiplex_2x1_mrc_csi :1624-1707). mmse = 0 zeroes the noise term
                               (pdsch.c:866). 16-bit LLRs */
  uint32_t pmi;             /* srslte_pdsch_grant_t.pmi */
  int      mod2;            /* grant.tb[1].mod */
  uint32_t tbs2;            /* grant.tb[1].tbs; 0: one transport block. With two, d_tb / d_tb_ok of the batch calls have 2 * nof_sf rows:
                               row b = transport block 0 of subframe b, row nof_sf + b = transport block 1; tb_stride covers the larger */
  int      cp_ext;          /* 1: extended-CP cell (srslte_cell_t.cp = SRSLTE_CP_EXT): 12 symbols per subframe - grids, estimates and RE lists
                               are [12][12 * nof_prb] -, CRS on symbols 0 and 3 of each slot, PSS / SSS on symbols 5 and 4 of slot 0
                               (ofdm.c:424-437, chest_dl.c:497-502, pdsch.c:81-206 with nof_symb_slot = 6) */
  int      tdd;             /* 1: TDD cell (srslte_cell_t.frame_type = SRSLTE_TDD) with tdd_sf_config (uplink-downlink configuration 0-6) and
                               tdd_ss_config (special-subframe configuration 0-9) = the srslte_tdd_config_t of its subframes. Served by the
                               per-subframe-grant entry points (srslte_hip_dl_rx_batch_grants*): SSS on the last symbol of slot 1 in subframes
                               0 / 5, PSS on symbol 2 of subframes 1 / 6, and in the special subframes PDSCH and CRS on the DwPTS symbols only
                               (pdsch.c:124-140, ra_dl.c:446-460, refsignal_dl.c:162-225); uplink subframes of the batch carry tbs = 0. The
                               fixed-grant calls refuse a TDD cell (their three subframe classes are FDD's) */
  uint32_t tdd_sf_config, tdd_ss_config;
  int      mbsfn;           /* 1: the batch is MBSFN subframes carrying the PMCH of MBSFN area mbsfn_area_id (0-255) - srslte_ofdm_rx_sf on an MBSFN
                               object with non_mbsfn_region (1 or 2) symbols in front (ofdm.c:424-437), srslte_chest_dl_estimate_cfg with sf_type
                               MBSFN (chest_dl.c:718-745; chest_cfg.interpolate_subframe is implied, the estimate is undefined without it) and
                               srslte_pmch_decode (pmch.c:291-394): every PRB from symbol SRSLTE_NOF_CTRL_SYMBOLS(cfi) on, every second RE in the
                               symbols of the MBSFN reference signal, the area's scrambling sequence (sequences.c:76-80), rv 0. Grids, estimates
                               and RE lists are [12][12 * nof_prb] whatever the cell's CP (cp_ext: the CRS sequence of symbol 0); single-port
                               cell, 16-bit LLRs, 1-4 receive antennas; mod / tbs = the PMCH's (srslte_configure_pmch). Fixed-grant calls only */
  uint32_t mbsfn_area_id, non_mbsfn_region;
} srslte_hip_dl_rx_cfg_t;
srslte_hip_dl_rx_t* srslte_hip_dl_rx_create(const srslte_hip_dl_rx_cfg_t* cfg);
void                srslte_hip_dl_rx_destroy(srslte_hip_dl_rx_t* q);
/* "Sample formats" above: forwards to the object's OFDM object. After the call d_iq of EVERY entry point of the object that takes time samples is
 * in that format, layout [nof_sf][nof_rx][15 N] samples as before: the fixed grant, _harq / _harq2, _grants / _grants2 and stage 0 of
 * srslte_hip_dl_rx_stage. The *_grid_batch calls take grids and are not concerned. */
int                 srslte_hip_dl_rx_set_iq_format(srslte_hip_dl_rx_t* q, int format, float scale);
uint32_t            srslte_hip_dl_rx_nof_re(const srslte_hip_dl_rx_t* q, uint32_t sf_idx);
/* d_iq: [nof_sf][15*N]; outputs: d_tb [nof_sf][tb_stride] bytes (tbs/8 + 3 CRC bytes used), d_tb_ok [nof_sf]. The two output pointers may be
 * device-visible HOST memory (hipHostMalloc / a pinned allocation): the pipeline's last phase then stores the results where the MAC reads them and no
 * copy follows the batch (bench.py's N = 1 line; tests/test_gpu_fullsize.py::test_results_straight_into_pinned_host_memory) */
int srslte_hip_dl_rx_batch(srslte_hip_dl_rx_t* q, const void* d_iq, uint32_t tti0, uint32_t nof_sf, uint8_t* d_tb, uint32_t tb_stride,
                           uint8_t* d_tb_ok, void* stream);
/* HARQ (decode_tb_cb sch.c:299-414 on a srslte_softbuffer_rx_t per transport block, softbuffer.c:46-150): slot b of the object keeps
 * its blocks' soft buffers, CRC flags and decoded bytes between calls. new_data != 0: new transport blocks (the MAC's
 * srslte_softbuffer_rx_reset_tbs on a toggled NDI). new_data == 0: retransmission with redundancy version rv, de-matched LLRs are
 * added to the kept soft buffers (rm_turbo.c:407-409), blocks whose CRC already passed are left alone (sch.c:317-318). A retransmission
 * into a slot whose transport block has already passed (the MAC does not schedule one) is answered as upstream answers it: d_tb_ok 0
 * (decode_tb_cb saves passed blocks' bytes only while the block as a whole has failed, sch.c:399-410, and the reassembled block fails its
 * CRC-24A); the same holds for every HARQ entry point of this header (uplink, per-subframe grants) */
int srslte_hip_dl_rx_batch_harq(srslte_hip_dl_rx_t* q, const void* d_iq, uint32_t tti0, uint32_t nof_sf, uint32_t rv, int new_data,
                                uint8_t* d_tb, uint32_t tb_stride, uint8_t* d_tb_ok, void* stream);
/* the same with a redundancy version and a new-data flag per transport block (two-layer modes: grant.tb[0 / 1].rv and the state of
 * softbuffers.rx[0 / 1]); srslte_hip_dl_rx_batch_harq applies one pair to both */
int srslte_hip_dl_rx_batch_harq2(srslte_hip_dl_rx_t* q, const void* d_iq, uint32_t tti0, uint32_t nof_sf, const uint32_t rv[2], const int new_data[2],
                                 uint8_t* d_tb, uint32_t tb_stride, uint8_t* d_tb_ok, void* stream);
/* same from frequency-domain grids d_grid [nof_sf][14][12*nof_prb] (the part of srslte_ue_dl_decode after srslte_ofdm_rx_sf,
 * ue_dl.c:375-397; SURVEY §8d cfg5 feeds grids) */
int srslte_hip_dl_rx_grid_batch(srslte_hip_dl_rx_t* q, const void* d_grid, uint32_t tti0, uint32_t nof_sf, uint8_t* d_tb, uint32_t tb_stride,
                                uint8_t* d_tb_ok, void* stream);
/* A new grant every subframe, as srslte_pdsch_decode takes it (pdsch.c:833-997 with a srslte_pdsch_grant_t per call, pdsch_cfg.h:38-50):
 * subframe b of the batch is received with grants[b] (host array). prb_mask[s]: bit n = srslte_pdsch_grant_t.prb_idx[s][n], the PRBs of
 * slot s (any subset; the two slots may differ, as with distributed virtual resource blocks), walked as srslte_pdsch_cp does
 * (pdsch.c:81-206). tbs = 0: no transport block in that subframe (tb_ok = 0). rv / new_data as srslte_hip_dl_rx_batch_harq, per subframe.
 * cfg.tbs of the object bounds every grant's tbs; cfg.mod / cfg.rnti / cfg.cfi are not used. Single antenna port or transmit diversity (cfg.nof_ports); cfg.llr_8bit, cfg.csi_enable
 * (csi_correction with every subframe's own allocation and modulation) and cfg.nof_rx_antennas apply.
 * Every grant's tbs is at most 105528 bits (36.213 Table 7.1.7.2.1-1 at 110 PRB), a multiple of 8, and segments without filler bits and
 * into code blocks of one size (srslte_cbsegm: F = 0, C2 = 0); other grants are refused with SRSLTE_ERROR_INVALID_INPUTS.
 * With 16-bit LLRs the transport blocks are assembled and judged by the decoder launch itself (no assembly kernel behind it; blocks kept from an
 * earlier transmission contribute their stored bytes) when every transport block of the call has at most 16 code blocks; a call with a larger
 * one has the separate assembly kernel do it for all of its transport blocks. Environment SRSLTE_HIP_GRANTS_TB_DIRECT=0, read when an object serves its first grants
 * call, keeps the separate assembly kernel (A/B, tests). Results are the same either way. */
typedef struct {
  uint32_t prb_mask[2][4];
  int      mod;      /* srslte_mod_t: 1 QPSK, 2 16QAM, 3 64QAM, 4 256QAM */
  uint32_t tbs;      /* bits */
  uint32_t rv;
  uint32_t cfi;
  uint16_t rnti;
  int      new_data; /* != 0: new transport block in HARQ slot b (soft buffer overwritten); 0: retransmission (combined) */
} srslte_hip_dl_grant_t;
int srslte_hip_dl_rx_batch_grants(srslte_hip_dl_rx_t* q, const void* d_iq, uint32_t tti0, uint32_t nof_sf, const srslte_hip_dl_grant_t* grants,
                                  uint8_t* d_tb, uint32_t tb_stride, uint8_t* d_tb_ok, void* stream);
/* The same with the transmission scheme of each subframe's grant and a second transport block (srslte_pdsch_grant_t.tx_scheme / pmi / tb[1],
 * as srslte_ra_dl_dci_to_grant fills them from DCI formats 1 / 1A / 2 / 2A, ra_dl.c:530-600): on a 2-port cell received with 2 antennas
 * (cfg.nof_ports = cfg.nof_rx_antennas = 2, cfg.tx_scheme = 0) a batch may mix transmit diversity (tx_scheme 0 or 1), large-delay CDD
 * (SRSLTE_TXSCHEME_CDD 3: two transport blocks) and closed-loop multiplexing (SRSLTE_TXSCHEME_SPATIALMUX 2: two blocks with pmi 0-1, or one
 * with pmi 0-3). Then d_tb / d_tb_ok have 2 * nof_sf rows: row b = transport block 0 of subframe b, row nof_sf + b = transport block 1
 * (tb_ok 0 where there is none); HARQ slot of block 1: its own. On other cells tx_scheme must be 0 / 1 and the rows are nof_sf. */
typedef struct {
  srslte_hip_dl_grant_t tb0; /* allocation, CFI, RNTI and transport block 0 */
  int      tx_scheme;         /* srslte_tx_scheme_t */
  uint32_t pmi;               /* srslte_pdsch_grant_t.pmi */
  int      mod2;              /* transport block 1: modulation, size (0: none), redundancy version, new-data flag */
  uint32_t tbs2, rv2;
  int      new_data2;
} srslte_hip_dl_grant2_t;
int srslte_hip_dl_rx_batch_grants2(srslte_hip_dl_rx_t* q, const void* d_iq, uint32_t tti0, uint32_t nof_sf, const srslte_hip_dl_grant2_t* grants,
                                   uint8_t* d_tb, uint32_t tb_stride, uint8_t* d_tb_ok, void* stream);
/* ... from frequency-domain grids d_grid, as srslte_hip_dl_rx_grid_batch takes them (the caller ran the OFDM demodulation) */
int srslte_hip_dl_rx_grid_batch_grants2(srslte_hip_dl_rx_t* q, const void* d_grid, uint32_t tti0, uint32_t nof_sf, const srslte_hip_dl_grant2_t* grants,
                                        uint8_t* d_tb, uint32_t tb_stride, uint8_t* d_tb_ok, void* stream);
/* A pool of `depth` receive pipelines behind ONE submission call. A batch of 128 subframes is 832 decoder wavefronts for 1024 SIMDs and a chain of
 * dependent launches: one object on one stream reaches 0.4 of what the chip does with four batches in flight ("One call, one stream").
 * The pool owns the objects, a non-blocking stream and a completion event each, and takes the batches round-robin: the caller - one host thread, one
 * call per batch, as a worker of srsue / srsenb would make it - gets the overlapped rate without managing streams. submit() queues batch n on object
 * n % depth (waiting first, on the host, for the batch that used that object `depth` submissions ago) and returns a ticket; wait(ticket) blocks
 * until that batch's d_tb / d_tb_ok are final (their device buffers are the caller's; copy them on any stream after wait, or pass a pinned host
 * record to have the pool copy [nof_sf][tb_stride] bytes + [nof_sf] flags there on the batch's stream before the event). grants may be NULL (the
 * object's fixed grant). All calls from one host thread.
 * Precondition of submit(), as it has always been: the pool's streams are non-blocking and order against NOTHING of the caller's, so d_iq must be
 * complete (whatever filled it has finished, not merely been queued) and d_tb / d_tb_ok must not be in use by earlier work when submit() is called.
 * submit_host() is the call without such a precondition on device work: it first copies nof_sf * nof_rx * 15 N samples of the pool's format from
 * h_iq (host memory; pinned, or the copy is not asynchronous) into a device staging buffer of the chosen object, ON THAT OBJECT'S STREAM, and runs
 * the batch from there - after waiting, as submit() does, for the batch that used the object before. h_iq must stay valid and unchanged until
 * wait(ticket). The staging buffers (one per object, max_batch subframes) are allocated by the first submit_host(); a pool that never calls it
 * allocates nothing for it. The same refusals as submit(), made before anything is queued: NULL pointers, nof_sf > max_batch. The d_tb / d_tb_ok
 * part of the precondition remains. set_iq_format() sets the format of all the pool's objects ("Sample formats" above) and is refused once a
 * batch has been submitted. */
typedef struct srslte_hip_dl_rx_pool srslte_hip_dl_rx_pool_t;
srslte_hip_dl_rx_pool_t* srslte_hip_dl_rx_pool_create(const srslte_hip_dl_rx_cfg_t* cfg, uint32_t depth);
void                     srslte_hip_dl_rx_pool_destroy(srslte_hip_dl_rx_pool_t* p);
int64_t srslte_hip_dl_rx_pool_submit(srslte_hip_dl_rx_pool_t* p, const void* d_iq, uint32_t tti0, uint32_t nof_sf, const srslte_hip_dl_grant_t* grants,
                                     uint8_t* d_tb, uint32_t tb_stride, uint8_t* d_tb_ok, void* h_record /* pinned, or NULL */);
int     srslte_hip_dl_rx_pool_wait(srslte_hip_dl_rx_pool_t* p, int64_t ticket);
int     srslte_hip_dl_rx_pool_set_iq_format(srslte_hip_dl_rx_pool_t* p, int format, float scale);
int64_t srslte_hip_dl_rx_pool_submit_host(srslte_hip_dl_rx_pool_t* p, const void* h_iq, uint32_t tti0, uint32_t nof_sf, const srslte_hip_dl_grant_t* grants,
                                          uint8_t* d_tb, uint32_t tb_stride, uint8_t* d_tb_ok, void* h_record /* pinned, or NULL */);

/* one stage of the chain (0 OFDM RX, 1 chest_dl, 2 extract+equalise+demap+descramble, 3 rate de-matching, 4 turbo decode, 5 TB CRC):
 * what srslte_hip_dl_rx_batch runs in order; exposed so that each kernel can be timed on its own */
int srslte_hip_dl_rx_stage(srslte_hip_dl_rx_t* q, int stage, const void* d_iq, uint32_t tti0, uint32_t nof_sf, uint8_t* d_tb,
                           uint32_t tb_stride, uint8_t* d_tb_ok, void* stream);
/* intermediate device buffers of the last call, for parity tests: 0 grid, 1 ce, 2 chest res, 3 d (NULL unless
 * srslte_hip_dl_rx_keep_symbols(q, 1): the equalised symbols are otherwise never written to memory), 4 e (LLRs, per-subframe stride
 * = max nof_re * Qm rounded up to 16; before the CSI weighting), 5 w, 6 cb iters, 7 cb ok, 8 cb bytes, 9 csi [nof_sf][max nof_re] (csi_enable),
 * 10 the subframes' largest csi [nof_sf] */
const void* srslte_hip_dl_rx_debug_buffer(const srslte_hip_dl_rx_t* q, int which);
int         srslte_hip_dl_rx_keep_symbols(srslte_hip_dl_rx_t* q, int enable);
/* At a high code rate the parity streams of a code block are mostly puncturing zeros: in the decoder's 16-window layout the transmitted
 * values of rv 0 sit in every fourth 32-byte row. A fixed-grant call with rv 0 and new data (srslte_hip_dl_rx_batch, _stage, _batch_harq*)
 * then keeps those rows alone in the soft buffer when the object has 16-bit LLRs, the 16-window decoder (K > 800), K a multiple of 64 and no
 * code block of any subframe gets more than srslte_hip_rm_parity_compact_limit(K) LLRs; the rate de-matcher stores half the bytes and the
 * decoder fetches a quarter of the parity rows. A retransmission into such a buffer expands it first; buffer 5 of the debug view is always the
 * whole layout. Results are the same either way. Environment SRSLTE_HIP_PARITY_COMPACT=0, read when an object is created, keeps the whole
 * layout (A/B, tests). srslte_hip_dl_rx_parity_compact: 1 if the object's last rate de-matcher run wrote the compact layout, else 0.
 * srslte_hip_rm_parity_compact_limit: the first position of rv 0's circular buffer (36.212 5.1.4.1.2) that falls into a row the compact layout
 * of block length K does not keep; 0 where K has no such layout (K not a multiple of 64, or no code-block length) */
int      srslte_hip_dl_rx_parity_compact(const srslte_hip_dl_rx_t* q);
uint32_t srslte_hip_rm_parity_compact_limit(uint32_t K);

/* ------------------------------------------------------------------ PUSCH receive pipeline (eNB side): OFDM RX with the
 * -1/2 carrier shift (enb_ul.c:58-63) -> chest_ul -> RE extraction + one-tap MMSE -> inverse transform precoding -> soft demap +
 * descramble + UL channel de-interleaver (pusch.c:423-520, sch.c:891-913,:991-1066) -> rate de-matching -> turbo decode -> TB CRC.
 * UL-SCH with optional HARQ-ACK / RI / CQI multiplexing (cfg fields below), one grant per object (optionally hopping between the slots), normal or extended CP (cfg.cp_ext),
 * 16-bit LLRs (pusch.llr_is_8bit has no counterpart here: with it the reference hands int8 LLRs to an int16 channel deinterleaver,
 * pusch.c:481-503 / sch.c:890-918, and fails its own noise-free round trip - tests/test_oracle_vs_ref.py); redundancy versions and soft
 * combining through srslte_hip_ul_rx_batch_harq. */
typedef struct srslte_hip_ul_rx srslte_hip_ul_rx_t;
typedef struct {
  uint32_t cell_id, nof_prb;
  uint16_t rnti;
  int      mod;            /* srslte_mod_t: QPSK, 16QAM, 64QAM */
  uint32_t tbs;            /* grant.tb.tbs. 0 with cqi_len > 0: a PUSCH WITHOUT UL-SCH data (36.212 5.2.4.1; srslte_ulsch_decode with cb_segm.tbs == 0,
                            * sch.c:943-975,:1031-1065): the CQI report fills what the rank indication leaves (uci.c:266-281), HARQ-ACK and RI are sized by
                            * the report (uci.c:557-564); the batch calls decode the UCI and set d_tb_ok to 0. In grants mode: per grant (tbs = 0 with cqi_len > 0),
                            * on an object made with the largest transport-block size */
  uint32_t L_prb, n_prb, n_dmrs; /* grant: srslte_pusch_grant_t.L_prb / n_prb_tilde / n_dmrs (pusch_cfg.h:47-60) */
  uint32_t max_iterations, max_batch;
  int      mmse;           /* 1: noise_estimate from chest_ul (pusch.c:475) */
  srslte_hip_dmrs_pusch_cfg_t dmrs_cfg;
  int      shortened;      /* 1: the subframe's last symbol is left to the SRS (srslte_ul_sf_cfg_t.shortened, N_srs = 1): 11 data symbols */
  uint32_t ack_len;        /* 0..2 HARQ-ACK bits multiplexed on the PUSCH (srslte_uci_cfg_t.ack[0].nof_acks, sch.c:1074-1090, uci.c:755-790) */
  uint32_t I_offset_ack;   /* beta_offset index of 36.213 Table 8.6.3-1 (srslte_uci_offset_cfg_t.I_offset_ack) */
  uint32_t ri_len;         /* 0..2 rank-indication bits on the PUSCH (srslte_cqi_cfg_t.ri_len, sch.c:968-979,:1110-1129): their symbols are
                            * left out by the channel interleaver and the UL-SCH is rate-matched to the rest */
  uint32_t I_offset_ri;    /* index into 36.213 Table 8.6.3-2 (srslte_uci_offset_cfg_t.I_offset_ri) */
  uint32_t cqi_len, I_offset_cqi; /* CQI / PMI report of cqi_len bits (srslte_cqi_size of uci_cfg.cqi, up to 64) multiplexed in front of the UL-SCH
                                     with srslte_uci_offset_cfg_t.I_offset_cqi (sch.c:1031-1060,:1133-1160, uci.c:264-494); 0 = none */
  uint32_t hopping, n_prb_slot1;  /* hopping != 0: intra-subframe hopping, slot 1 at PRB offset n_prb_slot1 (srslte_pusch_grant_t.n_prb[1] /
                                     n_prb_tilde[1]; pusch.c:52-91, chest_ul.c:244-266, refsignal_ul.c:316-346); 0: both slots at n_prb */
  uint32_t max_grants;            /* srslte_hip_ul_rx_batch_grants: PUSCHs (= HARQ slots) per call; 0 = max_batch */
  int      cp_ext;                /* 1: extended cyclic prefix (srslte_cell_t.cp): 6 symbols per slot, DMRS in symbol 2 of each slot (refsignal_ul.h:43,
                                     pusch.c:57-60), 10 data symbols (9 shortened; ra_ul.c:234), the UCI column sets of uci.c:502,:527, the DMRS
                                     cyclic-shift hopping read at a stride of 8 x 6 bits (refsignal_ul.c:127-133); d_iq is [nof_sf][15*N] as before */
} srslte_hip_ul_rx_cfg_t;
srslte_hip_ul_rx_t* srslte_hip_ul_rx_create(const srslte_hip_ul_rx_cfg_t* cfg);
void                srslte_hip_ul_rx_destroy(srslte_hip_ul_rx_t* q);
/* "Sample formats": d_iq of every receive call of the object (fixed grant, _harq, _grants, _grants_pucch, _grants_pucch_srs) */
int                 srslte_hip_ul_rx_set_iq_format(srslte_hip_ul_rx_t* q, int format, float scale);
/* d_iq: [nof_sf][15*N]; d_tb [nof_sf][tb_stride] (tbs/8 + 3 CRC bytes used), d_tb_ok [nof_sf]; subframe b is TTI tti0 + b */
int srslte_hip_ul_rx_batch(srslte_hip_ul_rx_t* q, const void* d_iq, uint32_t tti0, uint32_t nof_sf, uint8_t* d_tb, uint32_t tb_stride,
                           uint8_t* d_tb_ok, void* stream);
/* HARQ (srslte_ulsch_decode -> decode_tb with grant.tb.rv and cfg->softbuffers.rx, sch.c:1063, :299-414): slot b of the object keeps its code
 * blocks' soft buffers, CRC flags and bytes between calls. new_data != 0: new transport blocks (srslte_hip_ul_rx_batch is rv 0 / new data);
 * new_data == 0: a retransmission with redundancy version rv (0..3) is added to the kept buffers, blocks whose CRC already passed are neither
 * combined nor decoded again. UCI is decoded afresh on every call. */
int srslte_hip_ul_rx_batch_harq(srslte_hip_ul_rx_t* q, const void* d_iq, uint32_t tti0, uint32_t nof_sf, uint32_t rv, int new_data, uint8_t* d_tb,
                                uint32_t tb_stride, uint8_t* d_tb_ok, void* stream);
/* Per-PUSCH grants (srslte_enb_ul_get_pusch once per scheduled UE after one srslte_enb_ul_fft per TTI, enb_ul.c:170-235): grants[p] names the
 * subframe of the batch it was received in (several PUSCHs may share one, on disjoint PRBs), its allocation (srslte_pusch_grant_t.L_prb,
 * n_prb_tilde[0 / 1]), n_dmrs, RNTI, modulation (1..3), transport block (<= cfg.tbs, no filler bits, one block size), redundancy version and
 * new-data flag. Slot p of the object is that PUSCH's srslte_softbuffer_rx_t between calls (HARQ as srslte_hip_ul_rx_batch_harq). Rows p of
 * d_tb / d_tb_ok. The object's cell, DMRS configuration, shortened flag, equaliser and pass limit apply (its own grant and UCI fields are those of
 * the fixed pipeline and play no part here); cfg.tbs = the largest transport block, cfg.max_grants >= nof_grants. HARQ-ACK and rank indication
 * per PUSCH (decisions: srslte_hip_ul_rx_grants_ack / _ri, [max_grants][2] device bytes each, row p; a call in which no grant carries either leaves
 * the rows as they were) and CQI reports (srslte_hip_ul_rx_grants_cqi:
 * [max_grants][64] bits, then [max_grants] CRC flags, as srslte_hip_ul_rx_cqi; rows whose grant carries no report keep their content). */
typedef struct {
  uint32_t sf;                       /* 0 .. nof_sf-1 */
  uint16_t rnti;
  uint32_t L_prb, n_prb, n_prb_slot1, n_dmrs;
  int      mod;
  uint32_t tbs, rv;
  int      new_data;
  uint32_t ack_len, I_offset_ack; /* 0..2 HARQ-ACK bits on this PUSCH and their offset index (as the cfg fields of the fixed pipeline) */
  uint32_t ri_len, I_offset_ri;   /* 0..2 rank-indication bits */
  uint32_t cqi_len, I_offset_cqi; /* 0..64 bits of CQI / PMI report (srslte_cqi_size) */
} srslte_hip_ul_grant_t;
int srslte_hip_ul_rx_batch_grants(srslte_hip_ul_rx_t* q, const void* d_iq, uint32_t tti0, uint32_t nof_sf, const srslte_hip_ul_grant_t* grants,
                                  uint32_t nof_grants, uint8_t* d_tb, uint32_t tb_stride, uint8_t* d_tb_ok, void* stream);
const uint8_t* srslte_hip_ul_rx_grants_ack(const srslte_hip_ul_rx_t* q);
const uint8_t* srslte_hip_ul_rx_grants_ri(const srslte_hip_ul_rx_t* q);
const uint8_t* srslte_hip_ul_rx_grants_cqi(const srslte_hip_ul_rx_t* q);
/* Device pointer to the HARQ-ACK decisions of the last batch on this object, [max_batch][2] bytes (srslte_uci_value_t.ack.ack_value of
 * srslte_pusch_decode); valid once the batch's stream work is done, all zero when cfg.ack_len == 0 */
const uint8_t* srslte_hip_ul_rx_ack(const srslte_hip_ul_rx_t* q);
const uint8_t* srslte_hip_ul_rx_ri(const srslte_hip_ul_rx_t* q); /* the same for the rank indication (srslte_uci_value_t.ri in [b][0]) */
/* the CQI reports of the last batch: [max_batch][64] bits (one per byte, srslte_cqi_value_pack order), then [max_batch] flags
 * (srslte_uci_value_t.cqi.data_crc: always 1 up to 11 bits, the CRC-8 result above; bits are only written when the flag is 1) */
const uint8_t* srslte_hip_ul_rx_cqi(const srslte_hip_ul_rx_t* q);
/* intermediate device buffers of the last call, for parity tests: 0 grid, 1 ce, 2 chest_ul res, 3 d (after de-precoding), 4 g (LLRs after
 * the de-interleaver), 5 w, 6 cb iters, 7 cb ok, 8 cb bytes, 9 z (equalised) */
const void* srslte_hip_ul_rx_debug_buffer(const srslte_hip_ul_rx_t* q, int which);

/* ------------------------------------------------------------------ PUSCH transmit pipeline (UE side): TB CRC24A +
 * segmentation + CB CRC24B -> turbo encoder -> rate matching + UL channel interleaver + scrambling + modulation -> transform precoding
 * -> RE mapping with the DMRS -> OFDM TX with 1/sqrt(N) and the +1/2 carrier shift (srslte_ue_ul_encode ue_ul.c:300-340 with
 * srslte_pusch_encode pusch.c:314-421, the UL-SCH part of srslte_ulsch_encode sch.c:1068-1160, srslte_refsignal_dmrs_pusch_put and
 * srslte_ofdm_tx_sf). Same restrictions as the receive pipeline. */
typedef struct srslte_hip_ul_tx srslte_hip_ul_tx_t;
typedef struct {
  uint32_t cell_id, nof_prb;
  uint16_t rnti;
  int      mod;            /* srslte_mod_t: QPSK, 16QAM, 64QAM */
  uint32_t tbs;            /* 0 with cqi_len > 0: a PUSCH without UL-SCH data (srslte_ulsch_encode with cb_segm.tbs == 0, sch.c:1111-1114,:1157-1174):
                            * d_tb of the batch calls is not read (may be NULL). In grants mode: per grant, on an object made with tbs > 0 */
  uint32_t L_prb, n_prb, n_dmrs;
  uint32_t max_batch;
  srslte_hip_dmrs_pusch_cfg_t dmrs_cfg;
  int      shortened;      /* as in srslte_hip_ul_rx_cfg_t */
  uint32_t ack_len, I_offset_ack; /* as in srslte_hip_ul_rx_cfg_t (srslte_ulsch_encode's uci_cfg, sch.c:1168-1215) */
  uint32_t ri_len, I_offset_ri;   /* as in srslte_hip_ul_rx_cfg_t (sch.c:1110-1129) */
  uint32_t cqi_len, I_offset_cqi; /* as in srslte_hip_ul_rx_cfg_t (srslte_uci_encode_cqi_pusch, sch.c:1133-1150) */
  uint32_t hopping, n_prb_slot1;  /* as in srslte_hip_ul_rx_cfg_t */
  uint32_t max_grants;            /* srslte_hip_ul_tx_batch_grants: PUSCHs per call; 0 = max_batch */
  int      cp_ext;                /* as in srslte_hip_ul_rx_cfg_t */
} srslte_hip_ul_tx_cfg_t;
srslte_hip_ul_tx_t* srslte_hip_ul_tx_create(const srslte_hip_ul_tx_cfg_t* cfg);
void                srslte_hip_ul_tx_destroy(srslte_hip_ul_tx_t* q);
/* "Sample formats": d_iq of every transmit call of the object, after 1/sqrt(N) and the half-carrier shift */
int                 srslte_hip_ul_tx_set_iq_format(srslte_hip_ul_tx_t* q, int format, float scale);
/* d_tb: [nof_sf][tb_stride] payload bytes (tbs/8 used); d_iq: [nof_sf][15*N] cf32 time samples; subframe b is TTI tti0 + b */
int srslte_hip_ul_tx_batch(srslte_hip_ul_tx_t* q, const uint8_t* d_tb, uint32_t tb_stride, uint32_t tti0, uint32_t nof_sf, void* d_iq,
                           void* stream);
/* The same with the HARQ-ACK values d_ack [nof_sf][2] (0/1 bytes, device) multiplexed in; requires cfg.ack_len > 0 */
int srslte_hip_ul_tx_batch_ack(srslte_hip_ul_tx_t* q, const uint8_t* d_tb, uint32_t tb_stride, const uint8_t* d_ack, uint32_t tti0,
                               uint32_t nof_sf, void* d_iq, void* stream);
/* HARQ-ACK values d_ack and rank-indication bits d_ri, each [nof_sf][2] device bytes, each required exactly when configured */
int srslte_hip_ul_tx_batch_uci(srslte_hip_ul_tx_t* q, const uint8_t* d_tb, uint32_t tb_stride, const uint8_t* d_ack, const uint8_t* d_ri,
                               uint32_t tti0, uint32_t nof_sf, void* d_iq, void* stream);
/* ... and the CQI / PMI report d_cqi [nof_sf][64] device bytes (one bit each, the first cfg.cqi_len used: srslte_cqi_value_pack's output),
 * required exactly when cfg.cqi_len > 0 (srslte_uci_encode_cqi_pusch, sch.c:1133-1150) */
int srslte_hip_ul_tx_batch_uci_cqi(srslte_hip_ul_tx_t* q, const uint8_t* d_tb, uint32_t tb_stride, const uint8_t* d_ack, const uint8_t* d_ri,
                                   const uint8_t* d_cqi, uint32_t tti0, uint32_t nof_sf, void* d_iq, void* stream);
/* ... with a redundancy version rv (0..3; srslte_pusch_grant_t.tb.rv -> srslte_ulsch_encode -> srslte_rm_turbo_tx_lut, sch.c:1157-1160): what a
 * HARQ retransmission sends. d_ack / d_ri / d_cqi as above (NULL when not configured). */
int srslte_hip_ul_tx_batch_rv(srslte_hip_ul_tx_t* q, const uint8_t* d_tb, uint32_t tb_stride, const uint8_t* d_ack, const uint8_t* d_ri,
                              const uint8_t* d_cqi, uint32_t rv, uint32_t tti0, uint32_t nof_sf, void* d_iq, void* stream);
/* Per-PUSCH grants on the transmit side: grants[p] as srslte_hip_ul_rx_batch_grants takes them (new_data unused) - what srslte_ue_ul_encode sends
 * TTI after TTI as the grants come in (ue_ul.c:300-340); several PUSCHs on disjoint PRBs of one subframe give the composite signal of several
 * UEs. Row p of d_tb is its transport block; d_ack / d_ri [nof_grants][2] and d_cqi [nof_grants][64] device bytes, rows p (NULL when no grant of
 * the call carries that UCI). cfg.tbs bounds every grant's tbs, cfg.max_grants the PUSCHs per call. */
int srslte_hip_ul_tx_batch_grants(srslte_hip_ul_tx_t* q, const uint8_t* d_tb, uint32_t tb_stride, const uint8_t* d_ack, const uint8_t* d_ri,
                                  const uint8_t* d_cqi, uint32_t tti0, uint32_t nof_sf, const srslte_hip_ul_grant_t* grants, uint32_t nof_grants,
                                  void* d_iq, void* stream);
/* intermediate device buffers of the last call, for parity tests: 0 code blocks (stride (K/8+15)&~15), 1 parity streams (stride
 * (K/4+1+15)&~15), 2 d (modulated), 3 z (after transform precoding), 4 grid, 5 TB CRCs (one word per subframe) */
const void* srslte_hip_ul_tx_debug_buffer(const srslte_hip_ul_tx_t* q, int which);

/* ------------------------------------------------------------------ PDSCH transmit pipeline (eNB side): srslte_pdsch_encode
 * (pdsch.c:1059-1185: DL-SCH coding, scrambling, modulation, layer mapping + SFBC precoding, RE mapping) + CRS
 * (srslte_refsignal_cs_put_sf refsignal_dl.c:253-272) + srslte_ofdm_tx_sf with 1/sqrt(N) (enb_dl.c:56-62). One codeword, TM1 or 2-port
 * TM2, full-band grant; no control region, PSS/SSS or PBCH content (their REs stay zero). Two codewords, TM3 (large-delay CDD) and TM4
 * (codebook precoding) on a 2-port cell: srslte_hip_dl_tx_batch_grants2 below. */
typedef struct srslte_hip_dl_tx srslte_hip_dl_tx_t;
typedef struct {
  uint32_t cell_id, nof_prb, cfi;
  uint16_t rnti;
  int      mod;            /* srslte_mod_t: QPSK .. 256QAM */
  uint32_t tbs;
  uint32_t max_batch;
  uint32_t nof_ports;      /* 0 or 1: TM1; 2 or 4: transmit diversity */
  float    p_a;            /* dB; rho_a = 10^(p_a/20) (x sqrt(2) for 2 ports), pdsch.c:518-554 with p_b giving rho_b = 1 */
  uint32_t max_grants;     /* srslte_hip_dl_tx_batch_grants: PDSCHs per call; 0 = max_batch */
  int      cp_ext;         /* 1: extended-CP cell (as srslte_hip_dl_rx_cfg_t.cp_ext): grids [12][12 * nof_prb], CRS on symbols 0 and 3 of each slot
                              with the extended-CP sequences (N_CP = 0 in c_init, refsignal_dl.c:79-99), srslte_ofdm_tx_sf with the long prefix */
  int      tdd;            /* as srslte_hip_dl_rx_cfg_t.tdd: TDD cell, per-PDSCH grants only (srslte_hip_dl_tx_batch_grants); special subframes get the
                              CRS symbols of their DwPTS (srslte_refsignal_cs_put_sf, refsignal_dl.c:253-272) and PDSCH there */
  uint32_t tdd_sf_config, tdd_ss_config;
  int      mbsfn;          /* as srslte_hip_dl_rx_cfg_t.mbsfn: srslte_pmch_encode (pmch.c:423-483) + srslte_refsignal_mbsfn_put_sf (refsignal_dl.c:297-326:
                              the CRS of symbol 0 and the MBSFN reference signal in symbols 2, 6, 10) + srslte_ofdm_tx_sf on an MBSFN object
                              (ofdm.c:558-574); single port, rv 0, fixed-grant calls only; rnti is not used */
  uint32_t mbsfn_area_id, non_mbsfn_region;
} srslte_hip_dl_tx_cfg_t;
srslte_hip_dl_tx_t* srslte_hip_dl_tx_create(const srslte_hip_dl_tx_cfg_t* cfg);
void                srslte_hip_dl_tx_destroy(srslte_hip_dl_tx_t* q);
/* "Sample formats": d_iq [nof_sf][nof_ports][15 N] of every transmit call of the object (fixed grant, _grants / _grants2, their _ctrl and _full
 * forms); the guard samples of an MBSFN subframe are zero in either format */
int                 srslte_hip_dl_tx_set_iq_format(srslte_hip_dl_tx_t* q, int format, float scale);
/* d_tb: [nof_sf][tb_stride] payload bytes; d_iq: [nof_sf][nof_ports][15*N] cf32, one time-domain signal per antenna port; rv: the
 * redundancy version of the whole batch (the circular buffer is re-encoded, not kept) */
int srslte_hip_dl_tx_batch(srslte_hip_dl_tx_t* q, const uint8_t* d_tb, uint32_t tb_stride, uint32_t tti0, uint32_t nof_sf, uint32_t rv, void* d_iq,
                           void* stream);
/* Per-PDSCH grants (srslte_enb_dl_put_base once per TTI, srslte_enb_dl_put_pdsch once per scheduled UE, srslte_enb_dl_gen_signal; enb_dl.c:330-419):
 * grants[p] = the subframe of the batch and a grant as the receive side takes it (PRB masks of both slots, modulation, transport block <= cfg.tbs,
 * redundancy version, RNTI, CFI; new_data unused); row p of d_tb is its transport block. Several PDSCHs may share a subframe; its grids carry the
 * CRS of every port and nothing else besides the PDSCHs (no control region, PSS / SSS / PBCH). d_iq as srslte_hip_dl_tx_batch.
 * srslte_hip_dl_tx_batch_grants_ctrl ("DL control region transmit" below) is the same call with the PCFICH, PHICH and PDCCH added. */
typedef struct {
  uint32_t              sf; /* 0 .. nof_sf-1 */
  srslte_hip_dl_grant_t grant;
} srslte_hip_dl_tx_grant_t;
int srslte_hip_dl_tx_batch_grants(srslte_hip_dl_tx_t* q, const uint8_t* d_tb, uint32_t tb_stride, uint32_t tti0, uint32_t nof_sf,
                                  const srslte_hip_dl_tx_grant_t* grants, uint32_t nof_grants, void* d_iq, void* stream);
/* The same with the transmission scheme of each PDSCH and a second transport block: grants[p].grant is the srslte_hip_dl_grant2_t the receive
 * side takes (srslte_hip_dl_rx_batch_grants2; new_data / new_data2 unused), so a grant unpacked once from DCI 2 / 2A serves both directions.
 * srslte_pdsch_encode with nof_layers == nof_tb (pdsch.c:1100-1173): every enabled block is CRC-attached, segmented, turbo-coded and
 * rate-matched on its own with the split unit Qm * N_L, N_L = 1 (sch.c:552-556), scrambled with its own codeword's sequence and modulated;
 * srslte_precoding_type then applies rho_a: large-delay CDD (precoding.c:1897-1956) or the codebook of 36.211 Table 6.3.4.2.3-1 with
 * codebook_idx = pmi for one block, pmi + 1 for two (pdsch.c:1152). On a 2-port object a call may mix, per entry, transmit diversity (tx_scheme
 * 0 / 1, tbs2 = 0), CDD (SRSLTE_TXSCHEME_CDD 3: two blocks) and multiplexing (SRSLTE_TXSCHEME_SPATIALMUX 2: two blocks with pmi 0-1, or one
 * with pmi 0-3) - what srslte_hip_dl_rx_batch_grants2 accepts; on other objects every entry is tx_scheme 0 / 1 with one block.
 * d_tb has 2 * nof_grants rows: row p = transport block 0 of entry p, row nof_grants + p = its block 1 (not read where tbs2 = 0).
 * cfg.tbs bounds both blocks, cfg.max_grants the PDSCHs of a call (so up to twice that many codewords). The buffers of the second
 * codewords are made by the first of these calls on an object (it replaces the per-codeword buffers of srslte_hip_dl_tx_batch_grants by ones
 * of twice the size, which both calls then use); an object that never makes one allocates nothing for them.
 * Refused with SRSLTE_ERROR_INVALID_INPUTS and a log line, before anything is queued: tx_scheme 2 / 3 on an object whose cell is not 2-port;
 * CDD without a second block; pmi out of range for its block count; a diversity entry with tbs2 != 0; mod2 / tbs2 / rv2 out of range; a block
 * that needs filler bits or two block lengths; fewer REs than code blocks; and everything srslte_hip_dl_tx_batch_grants refuses.
 * Out of scope, and refused the same way: objects created with cp_ext, tdd or mbsfn (they take srslte_hip_dl_tx_batch_grants only).
 * Not here: 4-port cells and more than two layers (the reference's precoders are 2x2), the TB-swap flag, a disabled block 0 with block 1
 * enabled, the fixed-grant srslte_hip_dl_tx_batch. srslte_hip_dl_tx_batch_grants2_ctrl / _full ("DL control region transmit" below): with
 * the control region / the whole subframe, as srslte_hip_dl_tx_batch_grants_ctrl / _full. */
typedef struct {
  uint32_t               sf; /* 0 .. nof_sf-1 */
  srslte_hip_dl_grant2_t grant;
} srslte_hip_dl_tx_grant2_t;
int srslte_hip_dl_tx_batch_grants2(srslte_hip_dl_tx_t* q, const uint8_t* d_tb, uint32_t tb_stride, uint32_t tti0, uint32_t nof_sf,
                                   const srslte_hip_dl_tx_grant2_t* grants, uint32_t nof_grants, void* d_iq, void* stream);
/* intermediate device buffers of the last call: 0 code blocks, 1 parity streams, 2 per-port symbol streams [nof_sf][nof_ports][max nof_re],
 * 3 grids [nof_sf][nof_ports][14][12*nof_prb] */
const void* srslte_hip_dl_tx_debug_buffer(const srslte_hip_dl_tx_t* q, int which);

/* ---- one transport block with HOST buffers in one device call: decode_tb_cb behind srslte_dlsch_decode2 / srslte_ulsch_decode
 * (lib/src/phy/phch/sch.c:299-414,:507-531): rate de-matching of every code block into its soft buffer, turbo decoding with CRC early stop,
 * decoded bytes. The single-call srslte_tdec_* API costs a host round trip per code block and per SISO pass; this entry costs one per
 * transport block. include/srslte_hip/srslte_compat.h exports srslte_dlsch_decode2 on top of it. ---- */
typedef struct srslte_hip_sch srslte_hip_sch_t;
srslte_hip_sch_t* srslte_hip_sch_create(uint32_t max_tbs, uint32_t max_e_bits, int llr_8bit);
void              srslte_hip_sch_destroy(srslte_hip_sch_t* q);
/* e_bits (host): nof_e_bits LLRs, int16 (int8 for an 8-bit object); mod 1 QPSK .. 4 256QAM; Nl 1 or 2 (sch.c:510-514); buffer_f[c] / cb_crc[c]:
 * the C soft buffers and CRC flags of the srslte_softbuffer_rx_t (in / out, host); cb_bytes [C][768]: K / 8 decoded bytes of every block this
 * call decoded; sum_passes: SISO passes over those blocks */
int srslte_hip_sch_decode(srslte_hip_sch_t* q, const void* e_bits, uint32_t nof_e_bits, uint32_t tbs, int mod, uint32_t Nl, uint32_t rv,
                          uint32_t max_iterations, int16_t** buffer_f, uint8_t* cb_crc, uint8_t* cb_bytes, uint32_t* sum_passes);
/* The same for one PUSCH: what srslte_ulsch_decode does (sch.c:991-1066) from the caller's descrambled LLRs q_bits (host, int16, nof_bits of
 * them; 16-bit objects only) - HARQ-ACK and RI decisions with upstream's int32 sums, the UL channel de-interleaver with its ACK positions
 * cleared, the CQI report in front of the UL-SCH, then the transport block as srslte_hip_sch_decode. One stream wait when every block passes
 * (a second for the soft buffers of failed blocks; one more where the report's size depends on the rank decoded in the same call). tbs 0: a
 * PUSCH without UL-SCH data, which carries a report (cqi_len > 0); buffer_f / cb_crc / cb_bytes are then not looked at. c_seq: the scrambling
 * sequence, one bit per byte (read at the positions of a 1-bit ACK / RI). Refused with SRSLTE_ERROR_INVALID_INPUTS before anything is queued:
 * mod outside 1..3, nof_symb outside 9..12, nof_bits no multiple of nof_symb Qm, ri_len > 2, a report longer than 64 bits, offsets above 15, a
 * transport block with filler bits or two block sizes, Q' beyond the matrix; SRSLTE_ERROR for a reserved beta offset, as upstream. */
typedef struct {
  int      mod;                                   /* 1 QPSK, 2 16QAM, 3 64QAM */
  uint32_t tbs, rv, nof_bits, L_prb, nof_symb, max_iterations;
  uint32_t ack_len, ri_len, cqi_len;              /* total ACK bits (3 and more: positions cleared, nothing decided, as upstream); RI bits 0-2;
                                                     srslte_cqi_size of the report with rank_is_not_one = false */
  uint32_t I_offset_ack, I_offset_ri, I_offset_cqi;
  uint32_t cqi_len_rank2, cqi_rank2;              /* a report whose size depends on the rank (sch.c:932-936,:982-986): its size for rank > 1, or 0;
                                                     the rank decoded by this call decides, or cqi_rank2 when ri_len = 0 */
} srslte_hip_ulsch_cfg_t;
typedef struct {
  uint8_t  ack[2], ri;                            /* decisions (sum > 0); ack[1] meaningful with ack_len = 2 */
  uint8_t  cqi_bits[64], cqi_crc;                 /* the report, one bit per byte (zeros where its CRC8 failed); cqi_crc: srslte_cqi_value_t.data_crc */
  uint32_t cqi_len;                               /* the size that was decoded */
  uint32_t Q_prime_ack, Q_prime_ri, Q_prime_cqi;
  uint32_t stream_waits;
} srslte_hip_ulsch_res_t;
int srslte_hip_ulsch_decode(srslte_hip_sch_t* q, const int16_t* q_bits, const uint8_t* c_seq, const srslte_hip_ulsch_cfg_t* cfg, int16_t** buffer_f,
                            uint8_t* cb_crc, uint8_t* cb_bytes, uint32_t* sum_passes, srslte_hip_ulsch_res_t* res);
/* debugging accessor: the first n LLRs of the last srslte_hip_ulsch_decode's de-interleaved stream g (n <= its nof_bits) to host memory */
int srslte_hip_ulsch_debug_g(srslte_hip_sch_t* q, int16_t* out, uint32_t n);
/* One level up: what srslte_pusch_decode does (pusch.c:427-522) from the subframe's grid and channel estimates in HOST memory, in one visit of
 * the device - the allocation's rows as pusch_cp takes them (pusch.c:53-91), the one-tap MMSE equaliser with noise_estimate as given
 * (srslte_predecoding_single), the inverse transform precoding over nof_symb symbols of 12 L_prb points, the int16 soft demapper and the
 * descrambling with the sequence of c_init = (rnti << 14) + (sf_idx << 9) + cell_id made on the device (sequences.c:65-67), then everything
 * srslte_hip_ulsch_decode does, from the LLRs where the chain left them. sf_symbols / ce: [2 nsl][12 nof_prb] cf32 (nsl 7, or 6 with cp_ext).
 * Only the allocation's rows cross the link, 2 x nof_re x 8 bytes; bytes, decisions, report and flags come back; nothing else goes up or
 * down between the steps. Stream waits as srslte_hip_ulsch_decode: one when every block passes. The bits of the sequence that a 1-bit ACK /
 * RI reads come from the device's own sequence. Refused with SRSLTE_ERROR_INVALID_INPUTS before anything is queued or written: everything
 * srslte_hip_ulsch_decode refuses for cfg->sch; an L_prb that srslte_hip_dft_precoding_valid_prb rejects; n_prb_tilde[s] + L_prb > nof_prb;
 * nof_re != 12 L_prb nof_symb; nof_symb != 2 nsl - 2 - shortened; sch.nof_bits != nof_re Qm; 8-bit objects. One receive antenna. */
typedef struct {
  srslte_hip_ulsch_cfg_t sch;                     /* everything srslte_hip_ulsch_decode takes (nof_bits = nof_re Qm) */
  uint32_t nof_prb, cell_id, cp_ext;              /* the cell */
  uint32_t rnti, sf_idx;                          /* srslte_pusch_cfg_t.rnti, srslte_ul_sf_cfg_t.tti % 10 */
  uint32_t n_prb_tilde[2];                        /* the PRB offset of each slot (intra-subframe hopping where they differ) */
  uint32_t shortened;                             /* srslte_ul_sf_cfg_t.shortened: the last symbol is left to the SRS */
  uint32_t nof_re;                                /* srslte_pusch_grant_t.nof_re */
} srslte_hip_pusch_cfg_t;
int srslte_hip_pusch_decode(srslte_hip_sch_t* q, const void* sf_symbols, const void* ce, float noise_estimate, const srslte_hip_pusch_cfg_t* cfg,
                            int16_t** buffer_f, uint8_t* cb_crc, uint8_t* cb_bytes, uint32_t* sum_passes, srslte_hip_ulsch_res_t* res);
/* The geometry of that call alone, without a device: the refusals that concern the allocation, and the rows the call stages, in pusch_cp's order.
 * rows: NULL, or [nof_symb][2] = (symbol of the subframe, first sub-carrier) of each row of 12 L_prb REs. Returns nof_symb, or
 * SRSLTE_ERROR_INVALID_INPUTS. */
int srslte_hip_pusch_rows(const srslte_hip_pusch_cfg_t* cfg, uint32_t* rows);
/* debugging accessor: the first n descrambled LLRs of the last srslte_hip_pusch_decode, in received order (pusch.c:499's q; n <= its nof_bits) */
int srslte_hip_pusch_debug_q(srslte_hip_sch_t* q, int16_t* out, uint32_t n);

/* ---- the transmit counterpart: encode_tb_off with w_offset = 0 behind srslte_dlsch_encode2 (sch.c:183-289,:549-575) in one device call with
 * one stream wait per transport block: TB CRC24A, segmentation, CB CRC24B, turbo encoding, the circular buffer of every code block as
 * srslte_rm_turbo_tx_lut leaves it (rm_turbo.c:328-372: packed bits without the NULLs, the interleaved systematic bits from bit 0, the
 * interlaced parity bits from bit K + 4; 3K + 12 bits, the rest of the last byte undefined) and the bit selection of the rv. Upstream enters the
 * library once per code block (srslte_tcod_encode_lut). include/srslte_hip/srslte_compat.h exports srslte_dlsch_encode2 on top of it. ---- */
typedef struct srslte_hip_sch_enc srslte_hip_sch_enc_t;
srslte_hip_sch_enc_t* srslte_hip_sch_enc_create(uint32_t max_tbs, uint32_t max_e_bits);
void                  srslte_hip_sch_enc_destroy(srslte_hip_sch_enc_t* q);
/* data (host): tbs / 8 bytes, or NULL for a retransmission (rv != 0); mod 1 QPSK .. 4 256QAM; Nl 1 or 2 (sch.c:552-556).
 * buffer_b[c]: the C circular buffers of a srslte_softbuffer_tx_t (host): written for rv == 0; for rv 1-3 they are read and the result depends
 * on them alone, whether data is given or not - buffers written by the reference's own encoder serve, and the other way round.
 * e_bits (host): packed, MSB first, Qm Nl floor(nof_e_bits / (Qm Nl)) bits from bit 0: block i carries Qm Nl floor(G' / C) bits for
 * i <= C - gamma - 1, else Qm Nl ceil(G' / C) (G' = nof_e_bits / (Qm Nl), gamma = G' mod C), and follows block i - 1 at bit granularity.
 * Refused before anything is queued, e_bits and buffer_b untouched: a transport block with filler bits (SRSLTE_ERROR and upstream's message,
 * sch.c:194-197); one with two code-block sizes (SRSLTE_ERROR_INVALID_INPUTS: no entry of this library takes them, as the grants modes and the
 * fixed-grant pipelines); rv > 3, mod outside 1..4, Nl outside 1..2, tbs % 8, tbs > max_tbs, nof_e_bits of 0 or above max_e_bits, and data ==
 * NULL with rv == 0, where upstream would rate-match what its scratch buffers held (all SRSLTE_ERROR_INVALID_INPUTS).
 * tbs == 0: SRSLTE_SUCCESS and nothing written, as upstream's loop over C = 0 blocks. */
int srslte_hip_sch_encode(srslte_hip_sch_enc_t* q, const uint8_t* data, uint32_t tbs, int mod, uint32_t Nl, uint32_t rv, uint32_t nof_e_bits,
                          uint8_t** buffer_b, uint8_t* e_bits);
/* The same for one PUSCH: what srslte_ulsch_encode does (sch.c:1068-1210) into the caller's packed q_bits (host, nof_bits / 8 bytes, MSB first,
 * every byte written) - the coded CQI report in bits [0, Q'_cqi Qm) of the stream g (srslte_uci_encode_cqi_pusch, uci.c:467-494), the UL-SCH's
 * G Qm bits behind it at bit granularity (G = H' - Q'_ri - Q'_cqi; data / buffer_b / rv as srslte_hip_sch_encode), the channel interleaver
 * that leaves the rank indication's symbols out of its read order (36.212 5.2.2.8) and the HARQ-ACK symbols over what it wrote: a coded bit of
 * type 1 sets its position, every other type (0, repetition, placeholder) clears it, as upstream - pusch.c fills the placeholder and
 * repetition bits after scrambling. One stream wait per call. g_bits: NULL, or (H' - Q'_ri) Qm bits of g from bit 0; the rest of the last
 * byte keeps the caller's value. tbs 0: a PUSCH without UL-SCH data, which carries a report (cqi_len > 0); data / buffer_b are not looked at.
 * Q' in upstream's float arithmetic (uci.c:266-281,:547-571). Refused before anything is queued or written, with
 * SRSLTE_ERROR_INVALID_INPUTS: what srslte_hip_sch_encode refuses, with its codes (filler bits: SRSLTE_ERROR); mod outside 1..3, nof_symb
 * outside 9..12, nof_bits != 12 L_prb nof_symb Qm, ri_len > 2, ack_len > 10, cqi_len > 64, offsets above 15, tbs 0 without a report,
 * Q'_ri + Q'_cqi >= H' with tbs > 0; a reserved beta offset of a field in use: -1, as upstream. */
typedef struct {
  int      mod;                                   /* 1 QPSK, 2 16QAM, 3 64QAM */
  uint32_t tbs, rv, nof_bits, L_prb, nof_symb;
  uint32_t ack_len, ri_len, cqi_len;              /* HARQ-ACK bits 0-10 (3 and more: the (32, O) block code), RI bits 0-2, report bits 0-64 */
  uint32_t I_offset_ack, I_offset_ri, I_offset_cqi;
  uint8_t  ack[10], ri;                           /* srslte_uci_value_t.ack.ack_value / .ri (a 2-bit RI sends ri and a zero, sch.c:1115) */
  uint8_t  cqi_bits[64];                          /* the packed report, one bit per byte (srslte_hip_cqi_value_pack's row) */
} srslte_hip_ulsch_enc_cfg_t;
typedef struct {
  uint32_t Q_prime_ack, Q_prime_ri, Q_prime_cqi;
  uint32_t stream_waits;
} srslte_hip_ulsch_enc_res_t;
int srslte_hip_ulsch_encode(srslte_hip_sch_enc_t* q, const uint8_t* data, const srslte_hip_ulsch_enc_cfg_t* cfg, uint8_t** buffer_b, uint8_t* g_bits,
                            uint8_t* q_bits, srslte_hip_ulsch_enc_res_t* res);
/* debugging accessor: the first n_words 32-bit words of the last srslte_hip_ulsch_encode's stream g from the device (n_words <= ceil of its
 * (H' - Q'_ri) Qm bits / 32; byte order as g_bits) */
int srslte_hip_ulsch_enc_debug(srslte_hip_sch_enc_t* q, uint32_t* out, uint32_t n_words);

/* ---- PUSCH UCI plan: how the rows x nof_symb symbols of a PUSCH are divided between HARQ-ACK, rank indication, CQI report and UL-SCH
 * (36.212 5.2.2.6, 5.2.4.1; Q_prime_ri_ack and Q_prime_cqi in upstream's float arithmetic, uci.c:264-281,:547-571) - what the PUSCH pipelines
 * and the two UL-SCH calls above size themselves with, here for a check without a device. Returns one of the reasons below (the outputs
 * computed up to that point stand, the rest are 0), or SRSLTE_ERROR_INVALID_INPUTS for a null pointer, a size of 0, or K_segm and C of which
 * only one is 0. Limits beyond these - on the number of ACK / RI bits, on the report's length, on how many symbols the UL-SCH needs - are
 * each caller's own. ---- */
#define SRSLTE_HIP_PUSCH_UCI_OK 0
#define SRSLTE_HIP_PUSCH_UCI_EMPTY 1   /* neither UL-SCH data nor a CQI report */
#define SRSLTE_HIP_PUSCH_UCI_BETA 2    /* the offset index of a field in use is reserved or above 15 (the report's is in use without data, too) */
#define SRSLTE_HIP_PUSCH_UCI_ROWS 3    /* Q'_ack or Q'_ri beyond the 4 rows symbols its columns hold */
#define SRSLTE_HIP_PUSCH_UCI_NO_ROOM 4 /* Q'_ri + Q'_cqi beyond the matrix, or no symbol left for the UL-SCH data */
typedef struct {
  uint32_t L_prb, nof_symb, Qm;
  uint32_t rows;                                  /* of the channel interleaver's matrix: 12 L_prb where nof_bits = 12 L_prb nof_symb Qm */
  uint32_t K_segm, C;                             /* sum K_r and the number of code blocks; both 0 without UL-SCH data */
  uint32_t ack_len, ri_len, cqi_len;
  uint32_t I_offset_ack, I_offset_ri, I_offset_cqi;
  uint32_t sym;                                   /* the ACK / RI symbol whose position is asked for */
} srslte_hip_pusch_uci_cfg_t;
typedef struct {
  uint32_t Qp_ack, Qp_ri, Qp_cqi;
  uint32_t Q_cqi;                                 /* Q'_cqi Qm: the coded report's bits in front of the UL-SCH's */
  uint32_t G_prime;                               /* rows nof_symb - Q'_ri - Q'_cqi symbols for the UL-SCH */
  uint32_t syms_lo, C_lo;                         /* the first C_lo code blocks carry syms_lo = floor(G' / C) symbols, the others one more */
  uint32_t ack_pos[2], ri_pos[2];                 /* (row, column) of ACK / RI symbol cfg->sym (uci.c:497-545) */
} srslte_hip_pusch_uci_res_t;
int srslte_hip_pusch_uci_plan(const srslte_hip_pusch_uci_cfg_t* cfg, srslte_hip_pusch_uci_res_t* res);

/* ------------------------------------------------------------------ DL control region receive (UE side): the part of srslte_ue_dl_find_dl_dci
 * that precedes the DCI unpacking, for a batch of subframes (ue/ue_dl.c:334-367 estimate_pdcch_pcfich, :422-478 dci_blind_search, :534-646
 * find_dl_dci_type_siprarnti / _crnti): PCFICH -> CFI -> PDCCH LLRs -> blind search -> one DL DCI message per subframe, all on the device and
 * in one sequence of launches on the caller's stream (no host synchronisation; the CFI decided on the device selects the REG list and the
 * candidates there). Inputs are what srslte_hip_ofdm_rx_sf_batch and srslte_hip_chest_dl_estimate_batch[_multi] produce.
 *   PCFICH (pcfich.c:160-227): srslte_predecoding_single_multi with the noise estimate as it is, or srslte_predecoding_diversity_multi +
 *     srslte_layerdemap_diversity (2 / 4 ports), QPSK soft demapping, the subframe's sequence (sequences.c:36-38), then
 *     srslte_pcfich_cfi_decode (pcfich.c:124-142): max_corr starts at 0 with index 0, so all-negative correlations give CFI 1, correlation 0.
 *   PDCCH LLRs (srslte_pdcch_extract_llr, pdcch.c:424-488): 36 NOF_CCE(cfi) REs of the REG list of the CFI (regs.c, built on the host once per
 *     object), srslte_predecoding_single_multi with noise / 2, QPSK demapping, srslte_scrambling_f_offset with srslte_sequence_pdcch of slot
 *     2 sf_idx sized 8 srslte_regs_pdcch_nregs(3) (pdcch.c:199-201, sequences.c:51-53). As on an AVX host the equaliser of a single-port cell
 *     combines at most antennas 0 and 1 over the first 16 (n / 16) symbols (antenna 0 alone with 3 or 4; precoding.c:149-236), the 2-port
 *     diversity equaliser antennas 0 and 1 (antenna 0 alone with 3 or 4; srslte_predecoding_diversity2_sse precoding.c:433-540); 4 ports: all.
 *   Candidates: srslte_pdcch_ue_locations_ncce (the Y_k hash, pdcch.c:228-275) and srslte_pdcch_common_locations_ncce (:291-314) with
 *     NOF_CCE of the CFI in use. A candidate whose mean |LLR| (summed in double) is not above 0.3 is skipped (pdcch.c:382-389). Otherwise
 *     srslte_pdcch_dci_decode (pdcch.c:327-363): srslte_rm_conv_rx to 3 (nof_bits + 16) with the repetitions added in the reference's order
 *     (rm_conv.c), srslte_viterbi_decode_f's quantisation and tail-biting decoder, CRC-16 and the XOR with the received parity; formats 0 / 1A
 *     told apart by the flag bit (pdcch.c:393-396). DCI sizes: srslte_dci_format_sizeof with a zero srslte_dci_cfg_t (dci.c:114-360).
 *   Search (cif disabled): SI / P / RA-RNTI: common space, 1A then 1C; C-RNTI: UE-specific space with ue_dci_formats[tm] (1A + 1 / 1 / 2A / 2
 *     for TM1-4, ue_dl.c:31-39), then 1A in the common space. The first candidate whose CRC remainder equals the RNTI and whose format is the
 *     one searched ends the search; a format-0 hit while searching 1A is not a DL DCI (ue_dl.c:452-470).
 * FDD and TDD cells, normal / extended CP, 6-110 PRB, 1 / 2 / 4 ports, 1-4 receive antennas, every PHICH configuration (phich_resources
 * srslte_phich_r_t 0-3 = 1/6, 1/2, 1, 2; phich_ext = SRSLTE_PHICH_EXT; the PHICH REGs of regs.c:245-367, with mi = 1 on an FDD cell). Refused: cfg.tdd in
 * srslte_hip_dl_ctrl_create (NULL; a TDD object comes from srslte_hip_dl_ctrl_create_tdd) and MBSFN subframes (SRSLTE_ERROR_INVALID_INPUTS).
 * TDD cells (srslte_hip_dl_ctrl_create_tdd, uplink-downlink configuration 0-6; the special-subframe configuration is not needed: the control
 * region lies inside every DwPTS). Per subframe, sf_idx = (tti0 + b) % 10:
 *   REG lists: those of srslte_regs_init_opts(cell, mi, sf1_6) with mi of 36.213 Table 6.9-1 (mi_tdd_table, ue_dl.c:49-55) and sf1_6 set in
 *     subframes 1 and 6 of an extended-PHICH cell - the regs[MI_IDX(sf_idx)] srslte_ue_dl's set_mi_value picks (ue_dl.c:57-62, :315-332).
 *     With mi = 0 the PDCCH has every REG but the PCFICH's; the PCFICH REGs are the same everywhere. One list set per variant in use is
 *     built when the object is made; the kernels pick the subframe's from a ten-entry table.
 *   Sizes: the LLR row stride and the PDCCH scrambling length are those of the largest list, mi = 0 at CFI 3 (ue_dl.c:197-226).
 *   Uplink subframes (36.211 Table 4.2-2): nothing of the grid is read; cfi 0, cfi_corr 0, nof_dci 0, nof_ul_dci 0, messages with nof_bits 0.
 *   Subframes 1 and 6: a decoded CFI of 3 becomes 2 before the PDCCH is read (ue_dl.c:351-354), in every configuration; cfi_corr stays the
 *     decoder's. A given cfi of 3 there is refused (36.211 Table 6.7-1; a deliberate narrowing). On a cell of at most 10 PRB a cfi of 2 is
 *     three symbols and its REGs reach the PSS on symbol 2: it is served as the reference serves it, and the caller picks 1 there.
 *   DCI sizes: srslte_dci_format_sizeof of a TDD cell (the DAI / UL index and the fourth HARQ process bit, dci.c:38-40, :142-143, :176-189);
 *     formats 0 and 1A still share one size; search order and ue_dci_formats as in FDD.
 *   PHICH: ngroup, nseq from srslte_phich_calc unchanged; a request whose ngroup is not below mi ngroups_m1 (x 2, extended CP) of its
 *     subframe is refused - every request in an mi = 0 or uplink subframe, and I_phich = 1 outside the mi = 2 subframes of configuration 0.
 *   A deliberate difference: where the cell is too small the reference lets two mapping units share a REG (6 PRB, Ng = 2, mi = 2: units 0
 *     and 2). The device adds PHICHs in parallel, so srslte_hip_dl_ctrl_create_tdd / _tx_create_tdd return NULL for a cell and configuration
 *     where any variant in use has such a REG; srslte_hip_dl_ctrl_phich_ngroups_tdd returns SRSLTE_ERROR for it.
 *   A second refusal of both creators, with the same error return of that helper: a variant in use whose PHICH leaves fewer than nine REGs to a
 *     CFI-1 region, so that it has no CCE (25 PRB, Ng = 2, configuration 0: mi = 2 takes 42 of the 46 REGs of symbol 0). The reference's
 *     srslte_regs_pdcch_ncce answers -1 there.
 * The MIB: srslte_hip_dl_ctrl_mib_batch ("DL broadcast" below).
 * UL DCIs and the PHICH: srslte_hip_dl_ctrl_batch_ul / srslte_hip_dl_ctrl_phich_batch below.
 * Not here: carrier indicator / carrier
 * aggregation, the DCI -> grant unpacking (srslte_dci_msg_unpack_pdsch + srslte_ra_dl_dci_to_grant stay with the caller), and
 * the single-subframe drop-in's pcfich.c / pdcch.c, which remain the reference's. */
typedef struct srslte_hip_dl_ctrl srslte_hip_dl_ctrl_t;
typedef struct {
  uint32_t nof_prb, nof_ports, cell_id;
  int      cp_ext;          /* srslte_cell_t.cp == SRSLTE_CP_EXT */
  int      phich_resources; /* srslte_phich_r_t */
  int      phich_ext;       /* srslte_cell_t.phich_length == SRSLTE_PHICH_EXT */
  int      tdd;             /* srslte_cell_t.frame_type == SRSLTE_TDD: 0 for srslte_hip_dl_ctrl_create, 1 for srslte_hip_dl_ctrl_create_tdd */
  uint32_t nof_rx_antennas; /* 1-4 */
  uint32_t max_batch;       /* subframes per call */
} srslte_hip_dl_ctrl_cfg_t;
typedef struct {            /* per subframe (host array) */
  uint16_t rnti;            /* SI / P / RA-RNTI: common space; anything else: C-RNTI. 0: nothing is searched (ue_dl.c:474-476) */
  uint32_t tm;              /* srslte_tm_t: 0-3 = TM1-TM4 */
  uint32_t cfi;             /* 0: from the PCFICH; 1-3: given (the sf->cfi a caller sets, refdrv_dl_estimate's cfi_in) */
  int      mbsfn;           /* MBSFN subframe: refused */
} srslte_hip_dl_ctrl_req_t;
typedef struct {            /* per subframe */
  uint32_t cfi;             /* the CFI used */
  float    cfi_corr;        /* srslte_pcfich_decode's correlation (computed also when the CFI is given) */
  uint32_t nof_dci;         /* DL DCIs found: 0 or 1 */
} srslte_hip_dl_ctrl_res_t;
typedef struct {            /* same members, order and sizes as srslte_dci_msg_t (dci.h:65-71) */
  uint8_t  payload[128];    /* nof_bits + 16 decoded bits (message, then the received CRC), zero behind */
  uint32_t nof_bits;
  uint32_t L, ncce;         /* srslte_dci_location_t */
  int      format;          /* srslte_dci_format_t */
  uint16_t rnti;
} srslte_hip_dci_msg_t;
typedef struct {            /* one searched candidate (srslte_hip_dl_ctrl_debug_buffer 1) */
  uint32_t L, ncce, format, nof_bits; /* location, format searched, srslte_dci_format_sizeof */
  uint32_t skipped;         /* mean |LLR| <= 0.3: not decoded */
  uint32_t crc_rem;         /* CRC-16 XOR received parity (msg->rnti of srslte_pdcch_decode_msg) */
  uint32_t format_decoded;  /* after the 0 / 1A differentiation */
  uint8_t  payload[128];    /* as srslte_hip_dci_msg_t.payload */
} srslte_hip_dl_ctrl_cand_t;
#define SRSLTE_HIP_DL_CTRL_MAX_CAND 38 /* 16 UE-specific x 2 formats + 6 common */
srslte_hip_dl_ctrl_t* srslte_hip_dl_ctrl_create(const srslte_hip_dl_ctrl_cfg_t* cfg);
/* a TDD cell: cfg->tdd must be 1, tdd_sf_config 0-6 (srslte_tdd_config_t.sf_config); every call below works on the object unchanged */
srslte_hip_dl_ctrl_t* srslte_hip_dl_ctrl_create_tdd(const srslte_hip_dl_ctrl_cfg_t* cfg, uint32_t tdd_sf_config);
void                  srslte_hip_dl_ctrl_destroy(srslte_hip_dl_ctrl_t* q);
/* d_grid [nof_sf][nof_rx][nsym][12 nof_prb] (nsym 14 / 12), d_ce [nof_sf][nof_ports][nof_rx][nsym][12 nof_prb], d_res [nof_sf]
 * srslte_hip_chest_dl_res_t; subframe b is TTI tti0 + b and is searched with reqs[b]. d_out [nof_sf] and d_msg [nof_sf] (subframes without
 * a DCI: nof_bits 0) may be device-visible pinned host memory. */
int srslte_hip_dl_ctrl_batch(srslte_hip_dl_ctrl_t* q, const void* d_grid, const void* d_ce, const void* d_res, uint32_t tti0, uint32_t nof_sf,
                             const srslte_hip_dl_ctrl_req_t* reqs, srslte_hip_dl_ctrl_res_t* d_out, srslte_hip_dci_msg_t* d_msg, void* stream);
/* device buffers of the last call: 0 LLR rows [max_batch][srslte_hip_dl_ctrl_llr_stride] float (72 NOF_CCE(cfi) LLRs, zeros behind, as
 * q->llr of pdcch.c), 1 candidates [max_batch][SRSLTE_HIP_DL_CTRL_MAX_CAND] srslte_hip_dl_ctrl_cand_t in search order, 2 their numbers
 * [max_batch] uint32 */
const void* srslte_hip_dl_ctrl_debug_buffer(const srslte_hip_dl_ctrl_t* q, int which);
uint32_t    srslte_hip_dl_ctrl_llr_stride(const srslte_hip_dl_ctrl_t* q);
/* host helpers (no device needed): RE indices into one antenna's [nsym][12 nof_prb] grid, in the order srslte_regs_pcfich_get (16) and
 * srslte_regs_pdcch_get (36 NOF_CCE(cfi)) read them; return the count, or < 0 for an invalid cell / cfi / too small max */
int      srslte_hip_dl_ctrl_pcfich_re(const srslte_hip_dl_ctrl_cfg_t* cfg, uint32_t* re, uint32_t max);
int      srslte_hip_dl_ctrl_pdcch_re(const srslte_hip_dl_ctrl_cfg_t* cfg, uint32_t cfi, uint32_t* re, uint32_t max);
/* srslte_pdcch_ue_locations_ncce / srslte_pdcch_common_locations_ncce: loc[2 k] = L (0-3), loc[2 k + 1] = ncce; returns k */
uint32_t srslte_hip_pdcch_ue_locations_ncce(uint32_t nof_cce, uint32_t* loc, uint32_t max_candidates, uint32_t sf_idx, uint16_t rnti);
uint32_t srslte_hip_pdcch_common_locations_ncce(uint32_t nof_cce, uint32_t* loc, uint32_t max_candidates);
/* srslte_dci_format_sizeof of an FDD cell with a zero srslte_dci_cfg_t, format srslte_dci_format_t 0-8 (0 1 1A 1C 1B 1D 2 2A 2B); 0 otherwise */
uint32_t srslte_hip_dci_format_sizeof(uint32_t nof_prb, uint32_t nof_ports, int format);
/* TDD twins. srslte_hip_dl_ctrl_tdd_mi: mi of 36.213 Table 6.9-1 for subframe sf_idx of configuration tdd_sf_config, < 0 for an uplink
 * subframe or an invalid configuration / subframe. srslte_hip_dl_ctrl_pdcch_re_tdd: the PDCCH RE list of that subframe (cfg->tdd is not
 * looked at); < 0 also for an uplink subframe. srslte_hip_dci_format_sizeof_tdd: the sizes of a TDD cell (only the frame type enters them) */
int      srslte_hip_dl_ctrl_tdd_mi(uint32_t tdd_sf_config, uint32_t sf_idx);
int      srslte_hip_dl_ctrl_pdcch_re_tdd(const srslte_hip_dl_ctrl_cfg_t* cfg, uint32_t tdd_sf_config, uint32_t sf_idx, uint32_t cfi, uint32_t* re,
                                         uint32_t max);
uint32_t srslte_hip_dci_format_sizeof_tdd(uint32_t nof_prb, uint32_t nof_ports, int format);

/* ------------------------------------------------------------------ DL control region receive: UL DCIs and PHICH (UE side). What
 * srslte_ue_dl_find_ul_dci (ue_dl.c:480-531, with the pending-UL-DCI rule of dci_blind_search :448-470) and srslte_ue_dl_decode_phich
 * (:673-703 -> srslte_phich_calc + srslte_phich_decode, phich.c:132-143, :181-313) do per TTI, for a batch of subframes on a
 * srslte_hip_dl_ctrl_t: a UE's find_dl_dci -> find_ul_dci -> decode_phich becomes one call, queued on the caller's stream with no host
 * synchronisation, one launch behind the three of srslte_hip_dl_ctrl_batch.
 *   UL DCIs (stateless per subframe, cif disabled), for a C-RNTI request:
 *     1. The DL search is walked as srslte_hip_dl_ctrl_batch walks it. While the format searched is 1A (UE-specific space, and the common
 *        space last), every candidate decoded before the DL hit whose CRC remainder equals the RNTI and whose flag bit says format 0 joins
 *        the subframe's pending list, unless SRSLTE_HIP_DL_CTRL_MAX_UL_DCI are held or one with the same nof_bits and payload is (find_dci,
 *        ue_dl.c:406-420). The walk ends at the first DL hit; candidates behind it are not looked at in this step.
 *     2. A pending list that is not empty is the UL result, in the order of discovery (pending = 1). Otherwise the UE-specific locations are
 *        walked again for format 0 and the first candidate with a matching CRC and the format-0 flag is the one UL result (pending = 0).
 *     3. Formats 0 and 1A have one size and srslte_pdcch_decode_msg is a pure function of the LLR row, so step 2 runs no decoder: it reads
 *        the candidates the 1A search decoded.
 *     A deliberate narrowing: for an SI-, P- or RA-RNTI request and for RNTI 0 the UL result is empty (srsue searches no UL DCI with those).
 *   PHICH: ngroup, nseq by srslte_phich_calc; the 12 REs of the group's mapping unit (the REG lists of the transmit side; mi = 1; on an
 *     extended-CP cell groups 2m and 2m + 1 share a unit and the odd one takes symbols 2, 3 of each REG, phich.c:263-277) on every receive
 *     antenna; srslte_predecoding_single_multi with the noise estimate as it is, or srslte_predecoding_diversity_multi +
 *     srslte_layerdemap_diversity (2 / 4 ports) - 12 symbols are below every SIMD threshold of precoding.c, so the generic bodies with all
 *     antennas; srslte_scrambling_c with srslte_sequence_phich; de-spreading by the conjugate orthogonal sequence with the 1 / N_SF factor
 *     inside the sum (N_SF 4 / 2); BPSK soft demapping; srslte_phich_ack_decode: ack_value 1 only if the +1 correlation is strictly greater,
 *     distance the winning correlation.
 * Capacity for PHICH requests is not part of srslte_hip_dl_ctrl_cfg_t (its layout is kept): srslte_hip_dl_ctrl_set_max_phich allocates it
 * (0 after create; calling it again replaces the buffers and waits for the device, so not with work of this object in flight). The requests
 * and soft values of a call lie in one device buffer per object, as the candidates of srslte_hip_dl_ctrl_batch do: calls on one object belong
 * on one stream at a time; use one object per stream.
 * Refused with SRSLTE_ERROR_INVALID_INPUTS before anything is queued: what srslte_hip_dl_ctrl_batch refuses (null pointers, nof_sf 0 or
 * beyond max_batch, MBSFN, tm > 3, cfi > 3), nof_phich beyond the capacity, a request's sf >= nof_sf, I_phich > 1, a resulting ngroup >=
 * srslte_regs_phich_ngroups (I_phich 1 names a group only on an extended-CP cell; phich.c:215-218. nseq is within the CP's sequence count by
 * srslte_phich_calc's own modulo, so the check of phich.c:204-214 has nothing to refuse).
 * TDD objects (srslte_hip_dl_ctrl_create_tdd): see "TDD cells" above - the group check is the subframe's own, and requests naming an
 * uplink subframe are refused; a cfi of 3 given for subframe 1 or 6 is refused.
 * Not here: a manual mi (mi_manual of srslte_ue_dl), MBSFN subframes, carrier indicator / cross-carrier UL DCIs, TPC formats
 * 3 / 3A, the DCI -> grant unpacking (srslte_dci_msg_unpack_pusch + srslte_ra_ul_dci_to_grant stay with the caller), several UEs searching
 * one subframe's LLR row in one call, PHICH / UL DCIs in the fixed-grant srslte_hip_dl_rx_batch, and the single-subframe drop-in's phich.c,
 * which remains the reference's. */
#define SRSLTE_HIP_DL_CTRL_MAX_UL_DCI 5 /* SRSLTE_MAX_DCI_MSG */
typedef struct {            /* per subframe */
  uint32_t nof_ul_dci;      /* format-0 messages found: 0 .. SRSLTE_HIP_DL_CTRL_MAX_UL_DCI */
  uint32_t pending;         /* 1: they are the pending list of the DL search; 0: found by the format-0 search (or none) */
} srslte_hip_dl_ctrl_ul_res_t;
typedef struct {            /* one PHICH to read (host array): the srslte_phich_grant_t of the PUSCH it acknowledges */
  uint32_t sf;              /* subframe within the batch; several requests per subframe are allowed */
  uint32_t n_prb_lowest, n_dmrs, I_phich;
} srslte_hip_phich_req_t;
typedef struct {            /* per request */
  uint32_t ack_value;       /* srslte_phich_res_t.ack_value */
  float    distance;        /* srslte_phich_res_t.distance */
  uint32_t ngroup, nseq;    /* srslte_phich_resource_t */
} srslte_hip_phich_res_t;
typedef struct {            /* per request (srslte_hip_dl_ctrl_phich_debug_buffer) */
  float z[3][2];            /* q->z of phich.c after de-spreading (re, im) */
  float bits[3];            /* q->data_rx: the BPSK soft bits */
} srslte_hip_phich_soft_t;
int srslte_hip_dl_ctrl_set_max_phich(srslte_hip_dl_ctrl_t* q, uint32_t max_phich);
/* Everything srslte_hip_dl_ctrl_batch takes and returns (d_out and d_msg get what that call writes), plus d_ul_out [nof_sf], d_ul_msg
 * [nof_sf][SRSLTE_HIP_DL_CTRL_MAX_UL_DCI] (format 0; unused entries: nof_bits 0), and phich [nof_phich] (host; may be NULL with
 * nof_phich 0) -> d_phich_res [nof_phich] in request order. Result buffers may be device-visible pinned host memory. */
int srslte_hip_dl_ctrl_batch_ul(srslte_hip_dl_ctrl_t* q, const void* d_grid, const void* d_ce, const void* d_res, uint32_t tti0, uint32_t nof_sf,
                                const srslte_hip_dl_ctrl_req_t* reqs, srslte_hip_dl_ctrl_res_t* d_out, srslte_hip_dci_msg_t* d_msg,
                                srslte_hip_dl_ctrl_ul_res_t* d_ul_out, srslte_hip_dci_msg_t* d_ul_msg, const srslte_hip_phich_req_t* phich,
                                uint32_t nof_phich, srslte_hip_phich_res_t* d_phich_res, void* stream);
/* the PHICH part alone, for callers that know the grants already; nof_phich 0 queues nothing */
int srslte_hip_dl_ctrl_phich_batch(srslte_hip_dl_ctrl_t* q, const void* d_grid, const void* d_ce, const void* d_res, uint32_t tti0, uint32_t nof_sf,
                                   const srslte_hip_phich_req_t* phich, uint32_t nof_phich, srslte_hip_phich_res_t* d_phich_res, void* stream);
/* device buffer of the last call with PHICH requests: [nof_phich] srslte_hip_phich_soft_t; NULL before srslte_hip_dl_ctrl_set_max_phich */
const void* srslte_hip_dl_ctrl_phich_debug_buffer(const srslte_hip_dl_ctrl_t* q);

/* ------------------------------------------------------------------ DL control region transmit (eNB side): what srslte_enb_dl_put_base does
 * for the PCFICH (enb_dl.c:342-351), srslte_enb_dl_put_phich (:353-358) and srslte_enb_dl_put_pdcch_dl / _ul (:360-390) for a batch of
 * subframes, in one call on the caller's stream with no host synchronisation (the descriptors travel through pinned buffers, as the grants
 * paths' do). Per subframe b (TTI tti0 + b) of d_grid [nof_sf][nof_ports][nsym][12 nof_prb] cf32 it writes, and touches nothing else:
 *   PCFICH (srslte_pcfich_encode, pcfich.c:231-275): the 32-bit code word of in->cfi[b] (pcfich.c:39-47), srslte_sequence_pcfich of sf_idx,
 *     QPSK, srslte_layermap_diversity + srslte_precoding_diversity(..., 1.0f) for 2 / 4 ports, put on the 16 REs of every port.
 *   PHICH (srslte_regs_phich_reset + srslte_phich_encode + srslte_regs_phich_add; phich.c:318-430, regs.c:413-449): every PHICH REG of the
 *     cell is set to zero, then each of the subframe's PHICHs is added in entry order: three BPSK symbols of the ack, spread by the orthogonal
 *     sequence nseq of 36.211 Table 6.9.1-2 (phich.c:36-41), srslte_sequence_phich (the first 12 bits of the PCFICH's), on an extended-CP cell
 *     groups 2m and 2m + 1 share the REGs of mapping unit m and the odd group sits in the second half of each REG (phich.c:392-407), the
 *     precoding above on 12 symbols. Four ports follow the reference's precoding, not the rule of 36.211 6.9.2 (its FIXME, phich.c:421).
 *   PDCCH (srslte_pdcch_encode, pdcch.c:503-629): per DCI the CRC-16 with the RNTI mask, the tail-biting rate-1/3 convolutional code (K = 7,
 *     0x6D / 0x4F / 0x57), srslte_rm_conv_tx to E = 72 2^L bits, srslte_sequence_pdcch from bit 72 ncce, QPSK, the precoding above, put on
 *     entries [36 ncce, 36 (ncce + 2^L)) of the CFI's PDCCH RE list of every port. REGs of unused CCEs keep what they hold.
 * The result is bit-identical to the reference's grids. The REG lists and sequences are built on the host when the object is made.
 * Refused with SRSLTE_ERROR_INVALID_INPUTS before anything is queued: a cfi outside 1-3, an entry's sf >= nof_sf, nof_sf > max_batch, L > 3,
 * ncce + 2^L > NOF_CCE(cfi), nof_bits 0 or >= SRSLTE_DCI_MAX_BITS - 16 (pdcch.c:572-573), two DCIs of one subframe on a common CCE (the
 * reference would silently overwrite: a deliberate difference), a PHICH group >= srslte_regs_phich_ngroups, ack > 1, more than max_dci DCIs or
 * max_phich PHICHs. cfg.tdd is refused by srslte_hip_dl_ctrl_tx_create (NULL).
 * TDD cells (srslte_hip_dl_ctrl_tx_create_tdd; "TDD cells" of the receive side above has the REG variants, the group check and the shared-REG
 * refusal): each subframe is written over its own variant's lists, and every PHICH REG of that variant is set to zero first. An uplink
 * subframe is not written at all and in->cfi[b] is not looked at there. Refused besides the above: a DCI or PHICH naming an uplink subframe,
 * a PHICH group not below mi ngroups_m1 (x 2, extended CP) of its subframe, and cfi 3 in subframes 1 and 6 (36.211 Table 6.7-1; the
 * reference's eNB has no TDD, so this is this library's narrowing). The grids are bit-identical to srslte_pcfich_encode +
 * srslte_phich_encode + srslte_pdcch_encode over the subframe's own srslte_regs_t.
 * Not here: control in the fixed-grant srslte_hip_dl_tx_batch, MBSFN subframes, DCI packing (srslte_dci_msg_pack_pdsch / _pusch stay with the caller), carrier indicator, and the
 * single-subframe drop-in's pcfich.c / pdcch.c / phich.c, which remain the reference's. */
typedef struct srslte_hip_dl_ctrl_tx srslte_hip_dl_ctrl_tx_t;
typedef struct {
  uint32_t nof_prb, nof_ports, cell_id;
  int      cp_ext, phich_resources, phich_ext, tdd; /* as srslte_hip_dl_ctrl_cfg_t; tdd: 0 for _tx_create, 1 for _tx_create_tdd */
  uint32_t max_batch;       /* subframes per call */
  uint32_t max_dci;         /* DCIs per call */
  uint32_t max_phich;       /* PHICHs per call */
} srslte_hip_dl_ctrl_tx_cfg_t;
typedef struct {            /* one DCI (host array) */
  uint32_t             sf;  /* its subframe within the batch */
  srslte_hip_dci_msg_t msg; /* payload (one bit per byte, the first nof_bits read), nof_bits, L, ncce, rnti; format is not used */
} srslte_hip_dl_ctrl_tx_dci_t;
typedef struct {            /* one PHICH (host array): the srslte_phich_grant_t of srslte_enb_dl_put_phich, resource by srslte_phich_calc */
  uint32_t sf, n_prb_lowest, n_dmrs, I_phich;
  uint8_t  ack;             /* 0 / 1 */
} srslte_hip_phich_tx_t;
typedef struct {
  const uint32_t*                    cfi; /* [nof_sf], 1-3 */
  const srslte_hip_dl_ctrl_tx_dci_t* dci;
  uint32_t                           nof_dci;
  const srslte_hip_phich_tx_t*       phich; /* added in this order, per subframe */
  uint32_t                           nof_phich;
} srslte_hip_dl_ctrl_tx_in_t;
srslte_hip_dl_ctrl_tx_t* srslte_hip_dl_ctrl_tx_create(const srslte_hip_dl_ctrl_tx_cfg_t* cfg);
/* a TDD cell: cfg->tdd must be 1, tdd_sf_config 0-6; every call below works on the object unchanged */
srslte_hip_dl_ctrl_tx_t* srslte_hip_dl_ctrl_tx_create_tdd(const srslte_hip_dl_ctrl_tx_cfg_t* cfg, uint32_t tdd_sf_config);
void                     srslte_hip_dl_ctrl_tx_destroy(srslte_hip_dl_ctrl_tx_t* q);
int srslte_hip_dl_ctrl_tx_put(srslte_hip_dl_ctrl_tx_t* q, uint32_t tti0, uint32_t nof_sf, const srslte_hip_dl_ctrl_tx_in_t* in, void* d_grid, void* stream);
/* srslte_hip_dl_tx_batch_grants with srslte_hip_dl_ctrl_tx_put on its grids between the PDSCH mapping and the OFDM modulation: one complete
 * subframe per TTI apart from PSS / SSS / PBCH (srslte_hip_dl_tx_batch_grants_full below adds them). Refused (SRSLTE_ERROR_INVALID_INPUTS) besides what either call refuses: a ctrl object of
 * another cell (nof_prb, ports - a pipeline's nof_ports 0 is 1 -, cell_id, cp_ext), an MBSFN pipeline, a grant whose cfi differs from
 * in->cfi[grant.sf] (not compared for a grant in an uplink subframe of a TDD object, where in->cfi is not looked at), and a pipeline and control object of different frame types or uplink-downlink configurations (a TDD pipeline takes a
 * control object of srslte_hip_dl_ctrl_tx_create_tdd with its tdd_sf_config). */
int srslte_hip_dl_tx_batch_grants_ctrl(srslte_hip_dl_tx_t* q, const uint8_t* d_tb, uint32_t tb_stride, uint32_t tti0, uint32_t nof_sf,
                                       const srslte_hip_dl_tx_grant_t* grants, uint32_t nof_grants, srslte_hip_dl_ctrl_tx_t* ctrl,
                                       const srslte_hip_dl_ctrl_tx_in_t* in, void* d_iq, void* stream);
/* host helpers (no device needed), for a cell given as srslte_hip_dl_ctrl_tx_cfg_t (limits not looked at): srslte_regs_phich_ngroups (x 2 on
 * an extended-CP cell); srslte_phich_calc (36.213 9.1.2, phich.c:132-143): ngroup, nseq; the 12 REs of a group in srslte_regs_phich_add
 * order. Return < 0 for an invalid cell / group / too small max. */
int srslte_hip_dl_ctrl_phich_ngroups(const srslte_hip_dl_ctrl_tx_cfg_t* cfg);
int srslte_hip_phich_calc(const srslte_hip_dl_ctrl_tx_cfg_t* cfg, uint32_t n_prb_lowest, uint32_t n_dmrs, uint32_t I_phich, uint32_t* ngroup,
                          uint32_t* nseq);
int srslte_hip_dl_ctrl_phich_re(const srslte_hip_dl_ctrl_tx_cfg_t* cfg, uint32_t ngroup, uint32_t* re, uint32_t max);
/* TDD twins for subframe sf_idx of configuration tdd_sf_config (cfg->tdd is not looked at): the groups are mi srslte_regs_phich_ngroups_m1
 * (x 2, extended CP), 0 with mi = 0. < 0 for an uplink subframe; srslte_hip_dl_ctrl_phich_ngroups_tdd also returns SRSLTE_ERROR for a cell
 * and configuration the creators refuse: two mapping units of a variant share a REG, or a variant has no CCE at CFI 1 */
int srslte_hip_dl_ctrl_phich_ngroups_tdd(const srslte_hip_dl_ctrl_tx_cfg_t* cfg, uint32_t tdd_sf_config, uint32_t sf_idx);
int srslte_hip_dl_ctrl_phich_re_tdd(const srslte_hip_dl_ctrl_tx_cfg_t* cfg, uint32_t tdd_sf_config, uint32_t sf_idx, uint32_t ngroup, uint32_t* re,
                                    uint32_t max);

/* ------------------------------------------------------------------ DL broadcast: PSS, SSS and PBCH of a batch of subframes (eNB side) and
 * the MIB of every subframe 0 of a batch (UE side), on the control objects above, one launch each on the caller's stream, no host
 * synchronisation and no per-call descriptors (the MIB depends only on the cell and the TTI). On a TDD object (the _create_tdd calls) the
 * PBCH and the MIB are where they are in FDD; the SSS goes on the last symbol of slot 1 of subframes 0 and 5 (signal0 / signal5) and the PSS
 * on symbol 2 of subframes 1 and 6, each with its five zero guards - the positions the PDSCH pipelines skip (srslte_hip_dl_rx_cfg_t.tdd) and
 * sync.c:732-809 searches.
 * srslte_hip_dl_ctrl_tx_put_bcast writes what put_sync and put_mib of srslte_enb_dl_put_base write (enb_dl.c:297-307, :324-335), on every port
 * of d_grid [nof_sf][nof_ports][nsym][12 nof_prb] cf32, subframe b being TTI t = tti0 + b, and touches nothing else:
 *   t % 10 in {0, 5}: the PSS (srslte_pss_generate of cell_id % 3, built on the host with the reference's expression) in the last symbol of
 *     slot 0 and the SSS (srslte_sss_generate's signal0 / signal5, imaginary part 0) in the one before, each with five zeros on either side
 *     (pss.c:380-386, sss.c:106-119);
 *   t % 10 == 0: srslte_pbch_encode (pbch.c:554-607) of srslte_pbch_mib_pack(nof_prb, phich_ext, phich_resources, sfn = t / 10): CRC-16 and
 *     the port mask of srslte_crc_set_mask, the K = 7 tail-biting code, srslte_rm_conv_tx to 4 nof_bits (480 normal CP, 432 extended), and
 *     the quarter sfn % 4 alone scrambled with srslte_sequence_pbch at offset (sfn % 4) nof_bits, QPSK, layer mapping + precoding (1.0f),
 *     put in slot 1 on the REs of srslte_pbch_cp (pbch.c:54-101: the CRS positions of four ports are always skipped).
 * The result is bit-identical to the reference's. Refused with SRSLTE_ERROR_INVALID_INPUTS: a null object or grid, nof_sf > max_batch.
 * srslte_hip_dl_ctrl_mib_batch is srslte_pbch_decode called right after srslte_pbch_decode_reset (pbch.c:441-550, as srslte_ue_mib_decode's
 * first frame) on every subframe whose TTI % 10 == 0; the others get found = 0. d_grid, d_ce, d_res as srslte_hip_dl_ctrl_batch; only
 * receive antenna 0 is read (sf_symbols[0], ce[p][0]). For nant = 1, 2, 4 up to the object's nof_ports (search_all_ports), or nof_ports
 * alone: srslte_predecoding_single with noise_estimate (the AVX body, the generic tail) or srslte_predecoding_diversity (the SSE path for 2
 * ports) + srslte_layerdemap_diversity, QPSK demapping, then for dst = 0-3 decode_frame(0, dst, 1): descrambling at dst nof_bits, the other
 * quarters SRSLTE_RX_NULL, srslte_rm_conv_rx to 120 in its combining order, times 1 / 2, srslte_viterbi_decode_f, and the CRC check with the
 * nant mask, which rejects an all-zero payload (pbch.c:373-391). The first hit in (nant, dst) order wins. Stateless: each subframe 0 of a
 * batch is decoded on its own. d_mib [nof_sf] may be device-visible pinned host memory. Buffers are allocated by srslte_hip_dl_ctrl_create.
 * Refused with SRSLTE_ERROR_INVALID_INPUTS: null pointers, nof_sf > max_batch.
 * Not here: soft combining across calls (the reference's frame_idx window and memmove), cell search (PSS / SSS detection: srslte_hip_sync_find_batch below), broadcast in the fixed-grant srslte_hip_dl_tx_batch, and the single-subframe drop-in's pbch.c / pss.c / sss.c, which remain
 * the reference's. */
int srslte_hip_dl_ctrl_tx_put_bcast(srslte_hip_dl_ctrl_tx_t* q, uint32_t tti0, uint32_t nof_sf, void* d_grid, void* stream);
/* srslte_hip_dl_tx_batch_grants_ctrl with srslte_hip_dl_ctrl_tx_put_bcast on its grids after the CRS and before the PDSCHs, as the reference
 * writes sync and MIB before srslte_enb_dl_put_pdsch (a PDSCH RE wins where the two meet): srslte_enb_dl_put_base + _put_phich +
 * _put_pdcch_dl / _ul + _put_pdsch + srslte_enb_dl_gen_signal, a complete subframe per TTI, FDD or TDD. Refused as srslte_hip_dl_tx_batch_grants_ctrl. */
int srslte_hip_dl_tx_batch_grants_full(srslte_hip_dl_tx_t* q, const uint8_t* d_tb, uint32_t tb_stride, uint32_t tti0, uint32_t nof_sf,
                                       const srslte_hip_dl_tx_grant_t* grants, uint32_t nof_grants, srslte_hip_dl_ctrl_tx_t* ctrl,
                                       const srslte_hip_dl_ctrl_tx_in_t* in, void* d_iq, void* stream);
/* srslte_hip_dl_tx_batch_grants_ctrl / _full with two-codeword grants (srslte_hip_dl_tx_batch_grants2: TM3 / TM4 PDSCHs beside the DCI
 * formats 2A / 2 that announce them). Refused as those calls and as srslte_hip_dl_tx_batch_grants2. */
int srslte_hip_dl_tx_batch_grants2_ctrl(srslte_hip_dl_tx_t* q, const uint8_t* d_tb, uint32_t tb_stride, uint32_t tti0, uint32_t nof_sf,
                                        const srslte_hip_dl_tx_grant2_t* grants, uint32_t nof_grants, srslte_hip_dl_ctrl_tx_t* ctrl,
                                        const srslte_hip_dl_ctrl_tx_in_t* in, void* d_iq, void* stream);
int srslte_hip_dl_tx_batch_grants2_full(srslte_hip_dl_tx_t* q, const uint8_t* d_tb, uint32_t tb_stride, uint32_t tti0, uint32_t nof_sf,
                                        const srslte_hip_dl_tx_grant2_t* grants, uint32_t nof_grants, srslte_hip_dl_ctrl_tx_t* ctrl,
                                        const srslte_hip_dl_ctrl_tx_in_t* in, void* d_iq, void* stream);
typedef struct {            /* per subframe */
  uint32_t found;           /* 1: a MIB was decoded; 0 otherwise and in every subframe whose TTI % 10 != 0 */
  uint32_t nof_tx_ports;    /* nant that decoded */
  int32_t  sfn_offset;      /* as srslte_pbch_decode returns it (dst) */
  uint32_t nof_prb, phich_ext, phich_resources, sfn; /* srslte_pbch_mib_unpack; sfn = (unpacked + sfn_offset) % 1024 as srsue's sync does */
  uint8_t  payload[24];     /* the MIB bits */
} srslte_hip_mib_res_t;
typedef struct {            /* one decode_frame of the last call (srslte_hip_dl_ctrl_mib_debug_buffer 1) */
  uint32_t nant, dst;       /* nant 0: not tried */
  uint32_t hit;             /* srslte_pbch_crc_check passed */
  uint8_t  data[40];        /* srslte_viterbi_decode_f's output: payload, received CRC (before the mask) */
} srslte_hip_mib_cand_t;
int srslte_hip_dl_ctrl_mib_batch(srslte_hip_dl_ctrl_t* q, const void* d_grid, const void* d_ce, const void* d_res, uint32_t tti0, uint32_t nof_sf,
                                 int search_all_ports, srslte_hip_mib_res_t* d_mib, void* stream);
/* device buffers of the last srslte_hip_dl_ctrl_mib_batch: 0 LLR rows [max_batch][3][480] float (nant 1, 2, 4; nof_bits LLRs before
 * descrambling, as q->llr; zeros behind and in rows not tried), 1 candidates [max_batch][3][4] srslte_hip_mib_cand_t (nant, dst) */
const void* srslte_hip_dl_ctrl_mib_debug_buffer(const srslte_hip_dl_ctrl_t* q, int which);
/* host helpers (no device needed), for a cell given as srslte_hip_dl_ctrl_cfg_t (limits and receive antennas not looked at): the PBCH REs of
 * one port's subframe grid in srslte_pbch_put order (240 / 216); the 72 PSS REs then the 72 SSS REs of subframe sf_idx (0 or 5) with their
 * values val [144][2] (re, im), guards included; srslte_pbch_mib_pack into payload [24]. Return the count, or < 0 for invalid input. */
int srslte_hip_pbch_re(const srslte_hip_dl_ctrl_cfg_t* cfg, uint32_t* re, uint32_t max);
int srslte_hip_sync_re(const srslte_hip_dl_ctrl_cfg_t* cfg, uint32_t sf_idx, uint32_t* re, float* val, uint32_t max);
int srslte_hip_pbch_mib_pack(uint32_t nof_prb, int phich_ext, int phich_resources, uint32_t sfn, uint8_t* payload);

/* ------------------------------------------------------------------ UL control: PUCCH formats 1, 1a, 1b, 2, 2a, 2b (eNB receive, UE transmit)
 * srslte_hip_ul_ctrl_pucch_batch does what srslte_enb_ul_get_pucch does (enb_ul.c:175-228) for a list of (subframe, UE) requests, in one
 * launch on the caller's stream with no host synchronisation (descriptors through pinned buffers, as the DL control calls):
 *   resource selection  srslte_ue_ul_pucch_resource_selection with a zero srslte_uci_value_t (ue_ul.c:482-531 get_format, :823-900 get_npucch):
 *                       the CQI is dropped when HARQ-ACK collides and simul_cqi_ack is off; an SR TTI uses n_pucch_sr; formats 1/1a/1b
 *                       use ncce + N_pucch_1, formats 2/2a/2b n_pucch_2. Done on the host when the call is made.
 *   estimate            srslte_chest_ul_estimate_pucch (chest_ul.c:329-412): LS estimates at the DMRS of srslte_refsignal_dmrs_pucch_gen
 *                       (refsignal_ul.c:558-639), each slot's mean over its DMRS symbols, the 3-tap filter {0.3333, 1 - 2 0.3333, 0.3333}
 *                       with srslte_conv_same_cf's end extrapolation. 2a / 2b: every DMRS hypothesis, the last maximum of |sum| (>=) wins
 *                       and gives the HARQ-ACK bits.
 *   decode              srslte_pucch_decode (pucch.c:767-828, decode_signal :612-708): srslte_predecoding_single with req.noise_estimate
 *                       (the AVX body over 16 (n / 16) symbols, the generic tail). 1/1a/1b: srslte_vec_corr_ccc against every hypothesis,
 *                       the first maximum (>) wins; format 1 is detected with corr >= threshold_format1, 1a / 1b with >. 2/2a/2b: the
 *                       product with the conjugate reference, the 12-RE means, int16 QPSK LLRs, srslte_sequence_pucch (sequences.c:72-74,
 *                       made on the device), srslte_uci_decode_cqi_pucch (uci.c:169-200): the int32 correlation with every RM(20, A)
 *                       word in steps of 1 << (13 - len), the first maximum wins, returned as int16 and divided by 2000.
 *   SR retry            an SR TTI with HARQ-ACK that is not detected is decoded again on the HARQ-ACK resource (enb_ul.c:217-224).
 *   validity            ack_valid: corr > threshold_data_valid_format1a (1a / 1b) or > threshold_data_valid_format2 (2 / 2a / 2b), which
 *                       also gives cqi_crc; 0 otherwise.
 * srslte_hip_ul_ctrl_tx_put_pucch writes what srslte_ue_ul's pucch_encode writes: srslte_pucch_encode (pucch.c:741-765, encode_signal_format12
 * :429-492, pucch_cp :380-417) plus srslte_refsignal_dmrs_pucch_gen / _put (refsignal_ul.c:558-680), the selection made with the UCI values
 * (a positive SR selects n_pucch_sr). Only the PUCCH's REs are written. The per-(slot, symbol) tables (n_cs_cell pucch.c:954-972, the group's
 * srslte_refsignal_r_uv_arg_1prb, the orthogonal sequences) are made on the host once per object; the cyclic shifts (pucch.c:974-1059) on the
 * device. The time-domain signal comes from srslte_hip_ofdm_tx_sf_batch with the UL half-carrier shift. Requests of one call that write the same
 * RE (two UEs on one PRB of one grid) leave either value there: a subframe's grid is one UE's, as srslte_ue_ul's.
 * Grids are [nof_sf][nsym][12 nof_prb] (nsym 14 / 12), one antenna, as srslte_hip_ofdm_rx_sf_batch makes them; subframe b is TTI tti0 + b.
 * FDD, normal / extended CP, 6-110 PRB, one receive antenna (srslte_enb_ul_t), shortened subframes (SRS).
 * Refused with SRSLTE_ERROR_INVALID_INPUTS before anything is queued: ack_len > 2 (format 3, channel selection), cqi_len > 12 (a 13-bit
 * report: srslte_uci_decode_cqi_pucch tests cqi_len < 13 and fails it), cqi_len and ri_len together, ri_len > 1, a request that selects no
 * format (no HARQ-ACK, no SR TTI, no report), an n_pucch whose PRB lies outside the band in either slot, sf >= nof_sf, nof > max_pucch,
 * and a format 2 / 2a / 2b for an RNTI outside [SRSLTE_CRNTI_START, SRSLTE_CRNTI_END) (0x000B-0xFFF2), for which get_user_sequence
 * (pucch.c:214-236) has no scrambling sequence and the reference decodes nothing.
 * srslte_hip_ul_ctrl_create returns NULL for a configuration srslte_pucch_cfg_isvalid rejects (pucch.c:901-909), an invalid cell or TDD.
 * Not here: format 3, CA channel selection, TDD (n_pucch_i_tdd), several receive antennas, PUCCH inside srslte_hip_ul_tx_*, and the
 * single-subframe drop-in's pucch.c, which remains the reference's. */
typedef struct srslte_hip_ul_ctrl    srslte_hip_ul_ctrl_t;
typedef struct srslte_hip_ul_ctrl_tx srslte_hip_ul_ctrl_tx_t;
typedef struct {
  uint32_t nof_prb, cell_id;
  int      cp_ext;                  /* srslte_cell_t.cp == SRSLTE_CP_EXT */
  uint32_t delta_pucch_shift, n_rb_2, N_cs, N_pucch_1; /* srslte_pucch_cfg_t common configuration (pucch_cfg.h:45-90) */
  int      group_hopping_en;
  float    threshold_format1, threshold_data_valid_format1a, threshold_data_valid_format2;
  uint32_t max_pucch;               /* requests per call */
  int      tdd;                     /* refused */
} srslte_hip_ul_ctrl_cfg_t;
typedef struct {                    /* one (subframe, UE): what srslte_enb_ul_get_pucch is given */
  uint32_t sf;                      /* 0 .. nof_sf-1 */
  uint16_t rnti;
  uint32_t ack_len;                 /* 0-2 HARQ-ACK bits (srslte_uci_cfg_total_ack) */
  uint32_t ncce;                    /* n_pucch = ncce + N_pucch_1 for formats 1a / 1b */
  int      sr_tti;                  /* srslte_uci_cfg_t.is_scheduling_request_tti */
  uint32_t n_pucch_sr;
  uint32_t cqi_len;                 /* 0, 1-12: periodic CQI report (srslte_cqi_size) */
  uint32_t ri_len;                  /* 0, 1: rank indication instead of a report */
  uint32_t n_pucch_2;
  int      simul_cqi_ack;
  int      shortened;               /* srslte_ul_sf_cfg_t.shortened */
  float    noise_estimate;          /* the equaliser's noise (receive; srslte_chest_ul_estimate_pucch leaves chest_res.noise_estimate alone) */
} srslte_hip_pucch_req_t;
typedef struct {                    /* per request */
  uint32_t detected;
  float    correlation;
  uint32_t format;                  /* srslte_pucch_format_t used last (0-5) */
  uint32_t n_pucch;                 /* the resource used last */
  uint8_t  sr;                      /* SR TTI: detected on n_pucch_sr; 0 otherwise */
  uint8_t  ack[2];                  /* 1a / 1b: the hypothesis; 2a / 2b (and a report with ACK): the DMRS hypothesis */
  uint8_t  ack_valid;
  uint8_t  cqi[13];                 /* formats 2 / 2a / 2b: the 13 bits of the decoded word, the report in the first cqi_len */
  uint8_t  cqi_crc;
  uint8_t  ri;
  uint8_t  reserved;
} srslte_hip_pucch_res_t;
typedef struct {                    /* transmit: the request and the UCI values (srslte_uci_value_t) */
  srslte_hip_pucch_req_t req;       /* noise_estimate unused */
  uint8_t                ack[2], sr, ri;
  uint8_t                cqi[12];   /* the report's bits, cqi_len of them */
} srslte_hip_pucch_tx_t;
srslte_hip_ul_ctrl_t* srslte_hip_ul_ctrl_create(const srslte_hip_ul_ctrl_cfg_t* cfg);
void                  srslte_hip_ul_ctrl_destroy(srslte_hip_ul_ctrl_t* q);
/* d_grid [nof_sf][nsym][12 nof_prb]; d_res [nof] may be device-visible pinned host memory */
int srslte_hip_ul_ctrl_pucch_batch(srslte_hip_ul_ctrl_t* q, const void* d_grid, uint32_t tti0, uint32_t nof_sf, const srslte_hip_pucch_req_t* reqs,
                                   uint32_t nof, srslte_hip_pucch_res_t* d_res, void* stream);
/* device buffers of the last call: 0 equalised symbols [max_pucch][120] cf32 of the attempt used last (q->z of pucch.c, nof_re of them),
 * 1 descrambled LLRs [max_pucch][20] int16 (formats 2 / 2a / 2b) */
const void* srslte_hip_ul_ctrl_debug_buffer(const srslte_hip_ul_ctrl_t* q, int which);
/* srslte_hip_ul_rx_batch_grants plus the PUCCHs of reqs, decoded from the pipeline's own grid (one SC-FDMA demodulation for both, as
 * srslte_enb_ul_fft + get_pusch + get_pucch). ctrl must be made for the receiver's cell; nof_grants may be 0. PUSCH outputs are those of
 * srslte_hip_ul_rx_batch_grants. */
int srslte_hip_ul_rx_batch_grants_pucch(srslte_hip_ul_rx_t* q, const void* d_iq, uint32_t tti0, uint32_t nof_sf, const srslte_hip_ul_grant_t* grants,
                                        uint32_t nof_grants, uint8_t* d_tb, uint32_t tb_stride, uint8_t* d_tb_ok, srslte_hip_ul_ctrl_t* ctrl,
                                        const srslte_hip_pucch_req_t* reqs, uint32_t nof_pucch, srslte_hip_pucch_res_t* d_res, void* stream);
srslte_hip_ul_ctrl_tx_t* srslte_hip_ul_ctrl_tx_create(const srslte_hip_ul_ctrl_cfg_t* cfg);
void                     srslte_hip_ul_ctrl_tx_destroy(srslte_hip_ul_ctrl_tx_t* q);
/* writes the PUCCHs and their DMRS of tx[0 .. nof) into d_grid [nof_sf][nsym][12 nof_prb] */
int srslte_hip_ul_ctrl_tx_put_pucch(srslte_hip_ul_ctrl_tx_t* q, uint32_t tti0, uint32_t nof_sf, const srslte_hip_pucch_tx_t* tx, uint32_t nof, void* d_grid,
                                    void* stream);
/* host helpers (no device needed), for a configuration given as srslte_hip_ul_ctrl_cfg_t (max_pucch not looked at):
 * srslte_pucch_n_cs_cell into n_cs_cell [20][7]; the resource selection of a request (uci: NULL = the receiver's zero value, else the
 * transmitter's values) into res = {format, n_pucch, n_prb slot 0, n_prb slot 1}; the DMRS of srslte_refsignal_dmrs_pucch_gen for (format,
 * n_pucch, TTI, 2a / 2b bits) into r [2][N_rs][12] cf32, returning 12 N_rs per slot. < 0: invalid input; for the resource selection also a
 * request no format fits, or whose n_pucch puts a slot outside the band (what put_pucch and pucch_batch refuse). */
int srslte_hip_pucch_n_cs_cell(const srslte_hip_ul_ctrl_cfg_t* cfg, uint32_t* n_cs_cell);
int srslte_hip_pucch_resource(const srslte_hip_ul_ctrl_cfg_t* cfg, const srslte_hip_pucch_tx_t* uci, const srslte_hip_pucch_req_t* req, uint32_t* res);
int srslte_hip_pucch_dmrs(const srslte_hip_ul_ctrl_cfg_t* cfg, uint32_t format, uint32_t n_pucch, uint32_t tti, const uint8_t* drs_bits, void* r);

/* ------------------------------------------------------------------ UL control: PRACH preamble formats 0-3, FDD (UE generate, eNB detect)
 * The object holds what srslte_prach_set_cell_ / srslte_prach_gen_seqs build (lib/src/phy/phch/prach.c:224-322, :394-508), made on the host
 * once: the 64 sequences of the unrestricted set, shifted by v N_cs from roots u taken in the order of 36.211 Table 5.7.2-4 starting at
 * root_seq_idx, N_zc = 839, N_cs (Table 5.7.2-2), N_cp / N_seq (Table 5.7.1-1 scaled by N_ifft_ul / 2048), N_ifft_prach = 12 N_ifft_ul
 * (N_ifft_ul = srslte_symbol_sz(nof_prb)) and the DFT of every sequence as srslte_dft makes it (forward, 1/sqrt(839), not mirrored).
 * srslte_hip_prach_gen_batch writes what srslte_prach_gen writes (prach.c:510-549) for each entry: the sequence's DFT in the bins
 * [begin, begin + 839) of an N_ifft_prach-point inverse DFT, begin = 7 + 12 k_0 + 6, k_0 = 12 freq_offset - 6 N_rb_ul + N_ifft_ul / 2 with
 * N_rb_ul = srslte_nof_prb(N_ifft_ul); the transform mirrored (bin m is frequency m - N_ifft_prach / 2) and scaled by 1/sqrt(N_ifft_prach);
 * then the last N_cp samples and N_seq samples taken modulo N_ifft_prach (formats 2 and 3 repeat the sequence).
 * srslte_hip_prach_detect_batch is srslte_prach_detect_offset (prach.c:564-666) for each occasion: the bins [begin, begin + 839) of the
 * mirrored, unnormalised forward DFT of N_ifft_prach samples from occ.sample on; for each root the product with conj(DFT of the root
 * sequence), the unnormalised inverse DFT of 839 points, |.|^2 and its mean; window j of n_wins = 839 / N_cs (1 for N_cs = 0) starts at
 * (839 - j N_cs) % 839 and spans N_cs samples (839 for N_cs = 0), its first maximum (>) is the peak; a peak > detect_factor mean is reported
 * with index root n_wins + j, t_offset = c peak_offset / (1250 839) (c = 1.8, 1.9 above 30, 1.91 above 250; float) and peak / mean, in the
 * order (root, window). Rows of max_det = nof_roots n_wins per occasion; d_nof_det[o] tells how many of row o are written, the rest of the
 * row is left as it was. max_det may exceed 64 and indices >= 64 are reported as the reference reports them (zero_corr_zone 2: 2 roots x 55).
 * The long transforms are split as N_ifft_prach = 12 N_ifft_ul and only the 839 bins of the PRACH band are computed; the 839-point
 * correlations are direct sums with the twiddles in LDS. Both calls queue their work on the caller's stream with no host synchronisation
 * (descriptors through pinned buffers): gen_batch one launch, detect_batch three. Calls on one object run one after another on one stream.
 * Refused with SRSLTE_ERROR_INVALID_INPUTS before anything is queued: n greater than max_preambles / max_occasions, seq_index >= 64,
 * 6 + freq_offset > nof_prb, an occasion whose N_ifft_prach samples run past sig_len.
 * srslte_hip_prach_create returns NULL for a high-speed (restricted) set - the reference generates restricted-set sequences but numbers its
 * detections as windows of an unrestricted set, so there is nothing consistent to match -, TDD, and what srslte_prach_set_cell_ refuses
 * (config_idx >= 64, root_seq_idx >= 838, zero_corr_zone >= 16) or a cell outside 6-110 PRB.
 * Not here: high-speed sets, TDD and preamble format 4 (config_idx / 16 is 0-3 for FDD), several receive antennas (srsenb detects on antenna
 * 0), the deadzone (0 in the reference), and the single-call drop-in's prach.c, which remains the reference's over srslte_dft_*. */
typedef struct srslte_hip_prach srslte_hip_prach_t;
typedef struct {
  uint32_t nof_prb, config_idx, root_seq_idx, zero_corr_zone;
  int      hs_flag;                 /* refused */
  int      tdd;                     /* refused */
  float    detect_factor;           /* 0: the reference's PRACH_DETECT_FACTOR 18 (srsenb sets 60, srslte_prach_set_detect_factor) */
  uint32_t max_occasions;           /* srslte_hip_prach_detect_batch: occasions per call */
  uint32_t max_preambles;           /* srslte_hip_prach_gen_batch: preambles per call */
} srslte_hip_prach_cfg_t;
typedef struct {
  uint32_t N_zc, N_cs, N_cp, N_seq, N_ifft_prach, N_ifft_ul;
  uint32_t format;                  /* config_idx / 16 */
  uint32_t nof_roots, n_wins, max_det;
  uint32_t nof_sf;                  /* ceil(T_tot 1000): subframes a preamble spans (what srsenb buffers) */
  uint32_t root_seqs_idx[64];       /* first sequence of each root */
} srslte_hip_prach_info_t;
typedef struct {
  uint32_t seq_index, freq_offset;
} srslte_hip_prach_tx_t;
typedef struct {
  uint64_t sample;                  /* index into d_signal of the first sample after the CP (prach_worker.cc passes &samples[N_cp]) */
  uint32_t freq_offset;
  uint32_t reserved;
} srslte_hip_prach_occasion_t;
srslte_hip_prach_t* srslte_hip_prach_create(const srslte_hip_prach_cfg_t* cfg);
void                srslte_hip_prach_destroy(srslte_hip_prach_t* q);
int                 srslte_hip_prach_info(const srslte_hip_prach_t* q, srslte_hip_prach_info_t* info);
/* d_out [n][N_cp + N_seq] cf32 */
int srslte_hip_prach_gen_batch(srslte_hip_prach_t* q, const srslte_hip_prach_tx_t* list, uint32_t n, void* d_out, void* stream);
/* d_signal cf32 [sig_len] (e.g. the [nof_sf][15 N] buffer given to srslte_hip_ul_rx_batch_grants); d_nof_det [n]; d_indices, d_t_offsets,
 * d_peak_to_avg [n][max_det] (the last two may be NULL) */
int srslte_hip_prach_detect_batch(srslte_hip_prach_t* q, const void* d_signal, size_t sig_len, const srslte_hip_prach_occasion_t* occ, uint32_t n,
                                  uint32_t* d_nof_det, uint32_t* d_indices, float* d_t_offsets, float* d_peak_to_avg, void* stream);
/* host helpers (no device needed): the info of a configuration (< 0: create would refuse it); the checks of gen_batch / detect_batch for an
 * object of that configuration alone (nothing is queued); srslte_prach_tti_opportunity_config_fdd (prach.c:82-104); the preamble format
 * of config_idx (srslte_prach_get_preamble_format, < 0 for config_idx >= 64) */
int srslte_hip_prach_cfg_info(const srslte_hip_prach_cfg_t* cfg, srslte_hip_prach_info_t* info);
int srslte_hip_prach_gen_check(const srslte_hip_prach_cfg_t* cfg, const srslte_hip_prach_tx_t* list, uint32_t n);
int srslte_hip_prach_detect_check(const srslte_hip_prach_cfg_t* cfg, size_t sig_len, const srslte_hip_prach_occasion_t* occ, uint32_t n);
int srslte_hip_prach_tti_opportunity_fdd(uint32_t config_idx, uint32_t tti, int allowed_subframe);
int srslte_hip_prach_preamble_format(uint32_t config_idx);

/* ------------------------------------------------------------------ UE CSI feedback: PMI, RI and CQI from the DL estimates. What
 * select_pmi / select_ri_pmi / srslte_ue_dl_select_ri (ue_dl.c:705-800) measure per TTI - srslte_precoding_pmi_select for one and two
 * layers, srslte_precoding_cn (precoding.c:2151-2929) and srslte_cqi_from_snr - for a batch of subframes in ONE launch, one workgroup per
 * subframe, on the estimates where srslte_hip_chest_dl_estimate_batch_multi left them: d_ce [nof_sf][nof_ports][nof_rx][nsym][12 nof_prb]
 * (the reference's h[i][j] is port i, antenna j), d_res [nof_sf] srslte_hip_chest_dl_res_t, whose noise_estimate and snr_db are read on the
 * device; d_out [nof_sf] may be device-visible pinned host memory.
 * Sampling is that of the reference's AVX build: with N = nsym 12 nof_prb the PMI selection reads RE 24 k for k < 4 floor(N / 96) (the vector
 * loops drop the tail group), the condition number k < ceil(N / 24) (srslte_precoding_2x2_cn_gen). Per sample the arithmetic is the _gen
 * text with exact divisions; the sums are reduced in a fixed order. The AVX two-layer variant's _mm256_rcp_ps is not imitated.
 * 2-port cells with 2 receive antennas are what the reference computes. nof_ports = 1: every field 0 (select_pmi does nothing).
 * nof_rx = 1 on a 2-port cell: one-layer selection with the missing antenna's row zero, ri = 0, and no condition number (srslte_precoding_cn
 * refuses all but 2x2): sinr_2l, pmi_2l, cn_db and ri_cn are 0. srslte_hip_csi_create returns NULL for 4 ports, more than 2 antennas or a cell
 * outside 6-110 PRB; srslte_hip_csi_batch refuses null pointers with SRSLTE_ERROR_INVALID_INPUTS before anything is queued.
 * A noise_estimate of 0 (the estimator on a noise-free signal) is not clamped, as the reference does not clamp it: the one-layer SINRs are
 * +inf (none exceeds another: pmi_1l 0, sinr_db +inf, cqi_sinr 15), the two-layer ones 0 / 0 = NaN (pmi_2l 0, never chosen), cn_db is
 * unaffected. A caller that wants a floor applies it to d_res before the call. */
typedef struct srslte_hip_csi srslte_hip_csi_t;
typedef struct {
  float    sinr_1l[4], sinr_2l[2]; /* linear, sinr_list of srslte_precoding_pmi_select for 1 / 2 layers */
  uint32_t pmi_1l, pmi_2l;         /* the selected codebook entries */
  float    cn_db;                  /* srslte_precoding_cn */
  uint32_t ri_cn;                  /* cn_db < 17.0f ? 1 : 0 (srslte_ue_dl_select_ri) */
  uint32_t ri, pmi;                /* select_ri_pmi: this_sinr_db > best + 0.1 || this_sinr_db > 20.0 over ri < min(nof_rx, nof_ports) */
  float    sinr_db;
  uint32_t cqi_sinr;               /* srslte_cqi_from_snr(sinr_db + snr_to_cqi_offset) */
  uint32_t cqi_wideband;           /* srslte_cqi_from_snr(snr_db + snr_to_cqi_offset) */
  uint32_t reserved;               /* 0; the record is 64 bytes */
} srslte_hip_csi_res_t;
srslte_hip_csi_t* srslte_hip_csi_create(uint32_t nof_prb, uint32_t nof_ports, uint32_t nof_rx, int cp_is_norm);
void              srslte_hip_csi_destroy(srslte_hip_csi_t* q);
int               srslte_hip_csi_set_snr_to_cqi_offset(srslte_hip_csi_t* q, float offset); /* srslte_ue_dl_cfg_t.snr_to_cqi_offset; default 0 */
int               srslte_hip_csi_nof_samples(const srslte_hip_csi_t* q, uint32_t* n_pmi, uint32_t* n_cn); /* the two sample counts above */
int srslte_hip_csi_batch(srslte_hip_csi_t* q, const void* d_ce, const void* d_res, uint32_t nof_sf, srslte_hip_csi_res_t* d_out, void* stream);
/* The same measurement on the estimates and noise figures the last batch call of a receive pipeline left in its buffers (the ones stage 2 of
 * srslte_hip_dl_rx_stage reads): one launch behind the existing ones. Refused with SRSLTE_ERROR_INVALID_INPUTS before anything is queued: no batch
 * has run on the object, nof_sf greater than that batch, null pointers, a 4-port cell or more than 2 receive antennas. A single-port pipeline
 * writes zeros. srslte_hip_dl_rx_set_snr_to_cqi_offset: the offset of these calls (default 0). */
int srslte_hip_dl_rx_csi_batch(srslte_hip_dl_rx_t* q, uint32_t nof_sf, srslte_hip_csi_res_t* d_out, void* stream);
int srslte_hip_dl_rx_set_snr_to_cqi_offset(srslte_hip_dl_rx_t* q, float offset);
/* TEST AND DIAGNOSTIC ENTRIES, not needed to use the feature (srslte_hip_csi_nof_samples above is one too): they let the sampling rule and the
 * decision rules be checked exactly without a device.
 * host (no device needed): the decisions of one subframe from its seven sums - sums[0..3] the one-layer entries, [4..5] the two-layer ones,
 * [6] the condition numbers, over n_pmi / n_cn samples - by the function the kernel's deciding lane runs; and srslte_cqi_from_snr */
int      srslte_hip_csi_decide(const float sums[7], uint32_t n_pmi, uint32_t n_cn, float noise_estimate, float snr_db, float snr_to_cqi_offset,
                               uint32_t nof_rx, srslte_hip_csi_res_t* out);
uint32_t srslte_hip_cqi_from_snr(float snr);
/* Host report generation (cqi.c, ue_dl.c:802-928; no device needed). srslte_hip_cqi_cfg_t / _value_t: srslte_cqi_cfg_t and the members of the four
 * report structs of srslte_cqi_value_t side by side - WIDEBAND (PUCCH format 2): wideband_cqi, spatial_diff_cqi, pmi; SUBBAND: subband_cqi,
 * subband_label; SUBBAND_UE: wideband_cqi, subband_diff_cqi; SUBBAND_HL: wideband_cqi / subband_diff_cqi (codeword 0), wideband_cqi_cw1 /
 * subband_diff_cqi_cw1, pmi. srslte_hip_cqi_size and srslte_hip_cqi_value_pack return what srslte_cqi_size / srslte_cqi_value_pack return, the
 * reference's quirks included (a SUBBAND report counts 2 bits; a SUBBAND_UE report repeats the differential in the position field); the packed
 * row holds one bit per byte, the form srslte_hip_ul_tx_batch_uci_cqi (d_cqi rows) and srslte_hip_pucch_tx_t.cqi take. A report of
 * more than 64 bits (SUBBAND_HL above 104 PRB with two codewords, SUBBAND_UE with L > 58) does not fit the row and is refused.
 * srslte_hip_cqi_periodic_send / _ri_send: cqi_send / ri_send of cqi.c:457-528 (36.213 Tables 7.2.2-1A / -1B, FDD and TDD). */
#define SRSLTE_HIP_CQI_MAX_BITS 64
typedef struct {
  int      type;                 /* srslte_cqi_type_t: 0 WIDEBAND, 1 SUBBAND, 2 SUBBAND_UE, 3 SUBBAND_HL */
  int      data_enable, pmi_present, four_antenna_ports, rank_is_not_one, subband_label_2_bits;
  uint32_t L, N;
} srslte_hip_cqi_cfg_t;
typedef struct {
  uint32_t wideband_cqi, spatial_diff_cqi, pmi, subband_cqi, subband_label, subband_diff_cqi, wideband_cqi_cw1, subband_diff_cqi_cw1;
} srslte_hip_cqi_value_t;
int srslte_hip_cqi_size(const srslte_hip_cqi_cfg_t* cfg);
int srslte_hip_cqi_value_pack(const srslte_hip_cqi_cfg_t* cfg, const srslte_hip_cqi_value_t* value, uint8_t buff[SRSLTE_HIP_CQI_MAX_BITS]);
int srslte_hip_cqi_periodic_send(uint32_t I_cqi_pmi, uint32_t tti, int tdd);
int srslte_hip_cqi_periodic_ri_send(uint32_t I_cqi_pmi, uint32_t I_ri, uint32_t tti, int tdd);
int srslte_hip_cqi_hl_get_no_subbands(int nof_prb);
/* srslte_ue_dl_gen_cqi_periodic / _aperiodic on a host copy of a measurement record, branch for branch. cfg: the UE's reporting configuration
 * and last_ri, which is carried in and out as srslte_ue_dl_cfg_t.last_ri is (rank_is_not_one of a periodic report comes from it, not from
 * the record). wideband_value: the caller's wideband CQI (srsue passes srslte_cqi_from_snr(snr_db + offset): the record's cqi_wideband).
 * Subband differentials are zero and N = srslte_cqi_hl_get_no_subbands (0 up to 7 PRB), as in the reference. out: the report's configuration
 * and value, ri_len / ri, cqi_len = srslte_cqi_size and the packed row. A TTI without a periodic report leaves everything 0. */
typedef struct {
  int      tm;                   /* 1-4 (srslte_tm_t + 1) */
  uint32_t nof_prb, nof_ports, nof_rx_antennas;
  int      tdd;                  /* frame type of the report schedule */
  int      periodic_configured, ri_idx_present;
  uint32_t I_cqi_pmi, I_ri;      /* cqi-pmi-ConfigIndex, ri-ConfigIndex */
  int      format_is_subband;
  int      aperiodic_mode;       /* 30 or 31 */
  float    snr_to_cqi_offset;
  uint32_t last_ri;              /* in / out */
} srslte_hip_csi_report_cfg_t;
typedef struct {
  srslte_hip_cqi_cfg_t   cqi;
  srslte_hip_cqi_value_t value;
  uint32_t               ri_len, ri, cqi_len;
  uint8_t                cqi_bits[SRSLTE_HIP_CQI_MAX_BITS];
} srslte_hip_csi_report_t;
int srslte_hip_csi_gen_cqi_periodic(const srslte_hip_csi_res_t* csi, srslte_hip_csi_report_cfg_t* cfg, uint32_t wideband_value, uint32_t tti,
                                    srslte_hip_csi_report_t* out);
int srslte_hip_csi_gen_cqi_aperiodic(const srslte_hip_csi_res_t* csi, srslte_hip_csi_report_cfg_t* cfg, uint32_t wideband_value,
                                     srslte_hip_csi_report_t* out);

/* ------------------------------------------------------------------ channel emulator (replaces srslte::channel::run, lib/src/phy/channel/channel.cc:124-186,
 * over fading.c, delay.c, hst.c and rlf.c; the noise stage is this library's own). One object emulates nof_channels independent channels (a channel
 * is a UE x port: channel.cc keeps one fading and one delay object per port) at one sample rate. One call processes nof_calls consecutive blocks of
 * len samples per channel and equals nof_calls successive channel::run(in, out, len, t_i) calls, t_i = srslte_timestamp_add(t0, 0, i * len / srate);
 * the fading filter's overlap, the delay line and the noise counter are carried on the device from block to block and from call to call.
 *   fading: 36.104 B.2 EPA / EVA / ETU as fading.c:85-145,:249-275 computes them (N-point overlap-add filter, N = srslte_hip_channel_fft_size, a new
 *           frequency response every N/4 samples, segments restarting at every block); channel c draws its coefficients from seed0 + c * seed_stride
 *           (channel.cc: 0x1234 * port). The filter delays the signal by N/4 samples (srslte_hip_channel_path_delay): a receiver shifts its window by it.
 *   delay:  delay.c:26-126, one delay per block, computed on the host as upstream does; a pure copy. A block must be at least as long as its delay.
 *   hst:    hst.c:48-80, one Doppler shift per block, out[i] = in[i] exp(j 2 pi (-fs / srate) i), the phase restarting at 0 in every block as upstream.
 *   rlf:    rlf.c:31-44, the block times 1.0f or 0.0f.
 *   awgn:   complex noise of variance n0 per sample (n0 / 2 per component) from Philox-4x32-10 keyed by (awgn_seed, channel) with the sample's index
 *           since creation or reset as counter, and Box-Muller: the noise does not depend on how a run is split into calls.
 * Disabled stages cost nothing. Samples: d_in[c * in_ch_stride + i * in_call_stride + n], d_out likewise (strides in samples; d_out must not overlap
 * d_in; a call stride is at least len; in_ch_stride may be 0: one transmitted signal through every channel). Results are bit-reproducible from run to run (the overlap-add is a gather in a fixed order, no atomics). */
typedef struct srslte_hip_channel srslte_hip_channel_t;
enum { SRSLTE_HIP_CHANNEL_FADING_NONE = 0, SRSLTE_HIP_CHANNEL_FADING_EPA, SRSLTE_HIP_CHANNEL_FADING_EVA, SRSLTE_HIP_CHANNEL_FADING_ETU };
#define SRSLTE_HIP_CHANNEL_MAXTAPS 9
typedef struct {
  double   srate_hz;
  uint32_t nof_channels, max_calls, max_len; /* the largest nof_calls and len of a call */
  int      fading_enable, fading_model;      /* SRSLTE_HIP_CHANNEL_FADING_*; the model string "etu300" is model ETU with doppler_hz 300 */
  float    doppler_hz;
  uint32_t seed0, seed_stride;
  int      delay_enable;
  float    delay_min_us, delay_max_us, delay_period_s, delay_init_time_s;
  int      hst_enable;
  float    hst_fd_hz, hst_period_s, hst_init_time_s;
  int      rlf_enable;
  uint32_t rlf_t_on_ms, rlf_t_off_ms;
  int      awgn_enable;
  float    awgn_n0;
  uint32_t awgn_seed;
} srslte_hip_channel_cfg_t;
/* Refused with SRSLTE_ERROR_INVALID_INPUTS and a message: null pointers, no channels, a rate or a model out of range (a rate at which the model's filter would
 * be longer than 1024 points included: ETU at 61.44 MHz), fading enabled with model NONE (upstream leaves its N undefined), a delay or RLF period of zero, a negative n0; at run time nof_calls > max_calls, len > max_len or a block
 * shorter than its delay. */
int  srslte_hip_channel_create(srslte_hip_channel_t** q, const srslte_hip_channel_cfg_t* cfg);
void srslte_hip_channel_destroy(srslte_hip_channel_t* q);
int  srslte_hip_channel_reset(srslte_hip_channel_t* q); /* the state of a new object: no overlap, an empty delay line, noise counter 0 */
int  srslte_hip_channel_run_batch(srslte_hip_channel_t* q, const void* d_in, uint64_t in_ch_stride, uint64_t in_call_stride, void* d_out,
                                  uint64_t out_ch_stride, uint64_t out_call_stride, uint32_t nof_calls, uint32_t len, int64_t t_full_secs,
                                  double t_frac_secs, void* stream);
int  srslte_hip_channel_fft_size(const srslte_hip_channel_t* q);   /* N; 0 without fading */
int  srslte_hip_channel_path_delay(const srslte_hip_channel_t* q); /* N / 4; 0 without fading */
/* TEST AND DIAGNOSTIC ENTRIES (no device needed but for _coeffs' object): the drawn coefficients of a channel (returns the number of taps), the draw
 * itself, N for a model and rate, and the per-block figures the host computes for block i of a call starting at (t_full_secs, t_frac_secs) */
int srslte_hip_channel_coeffs(const srslte_hip_channel_t* q, uint32_t channel, double a[SRSLTE_HIP_CHANNEL_MAXTAPS], double w[SRSLTE_HIP_CHANNEL_MAXTAPS],
                              double p[SRSLTE_HIP_CHANNEL_MAXTAPS]);
int srslte_hip_channel_draw_coeffs(int fading_model, float doppler_hz, uint32_t seed, double a[SRSLTE_HIP_CHANNEL_MAXTAPS],
                                   double w[SRSLTE_HIP_CHANNEL_MAXTAPS], double p[SRSLTE_HIP_CHANNEL_MAXTAPS]);
int srslte_hip_channel_fft_size_for(int fading_model, double srate_hz);
typedef struct {
  double   t;             /* full + frac seconds of the block's timestamp: the fading filter's time */
  uint32_t delay_samples; /* delay.c:26-47 */
  float    hst_fs_hz;     /* hst.c:52-75 */
  int      rlf_on;        /* rlf.c:34-39 */
} srslte_hip_channel_block_t;
int srslte_hip_channel_block_params(const srslte_hip_channel_cfg_t* cfg, uint32_t len, uint32_t i, int64_t t_full_secs, double t_frac_secs,
                                    srslte_hip_channel_block_t* out);

/* ------------------------------------------------------------------ UL sounding reference signal, FDD (UE transmit, eNB sounding and timing)
 * srslte_hip_srs_tx_put writes what srslte_refsignal_srs_gen + srslte_refsignal_srs_put write (refsignal_ul.c:987-1026) for a list of
 * (subframe, UE) entries in one launch: r[i] into grid[sf][nsym-1][k0 + 2 i], i < M_sc, with M_sc = 6 m_srs_b[B][bw_cfg] (Tables
 * 5.5.3.2-1..4 of 36.211), k0 of srs_k0_ue (:919-941, frequency hopping for b > b_hop with n_srs = tti / T_srs, srs_Fb :896-916) and
 * r = exp(j (arg r_uv(i) + alpha i)), alpha = 2 pi n_srs / 8, u taken with delta_ss = 0, v = v_pusch[ns][delta_ss] when M_sc / 12 >= 6 and
 * sequence hopping is on. Only the SRS REs are written. The call always writes: whether TTI tti0 + sf is an SRS occasion is the caller's
 * decision, made with srslte_hip_srs_send_cs / _send_ue (the division of srs_tx_enabled and the put in ue_ul.c:283-291).
 * Three things are the reference's and are kept: (1) the symbol, which lies in the subframe's second slot, carries the sequence of the
 * FIRST slot (r_srs[i], not r_srs[M_sc + i]); with group hopping on that is not 36.211's sequence; (2) srslte_hip_srs_send_ue computes
 * (tti - T_offset) % T_srs in uint32_t, so for tti < T_offset the answer is that of 2^32 + tti - T_offset; (3) the comparisons of
 * srslte_hip_srs_pusch_shortened are those of :769-814 as written (an allocation whose last PRB lies just below the cell's sounding
 * band counts as overlapping it: n_prb + L_prb >= start is tested, not >).
 * srslte_hip_srs_rx_batch is this library's own (the reference has no SRS receiver): one launch, one workgroup per request, no scratch memory.
 * With y[i] = grid[sf][nsym-1][k0 + 2 i], z[i] = y[i] conj(r[i]) and J = M_sc / 8 blocks (M_sc is a multiple of 24; J <= 72):
 *   Z_j[k] = 1/8 sum_{i<8} z[8 j + i] exp(-j 2 pi k i / 8), k = 0..7: bin k holds the UE whose cyclic shift is (n_srs + k) % 8
 *   h_j = Z_j[0] -> d_ce[req][j] (rows of SRSLTE_HIP_SRS_MAX_CE, entries from J on are left alone); nof_ce = J
 *   free bins F = {k != 0 : bit (n_srs + k) % 8 of cs_used clear}; noise_estimate = 8 mean_{j, k in F} |Z_j[k]|^2, 0 when F is empty
 *   rsrp = mean_j |h_j|^2; snr = rsrp / noise_estimate, NaN when noise_estimate is 0; snr_db = 10 log10(snr); noise_estimate_dbm =
 *   10 log10(noise_estimate) + 30 (the conventions of chest_ul.c:317-321)
 *   ta_us = -arg(sum_{j<J-1} h_{j+1} conj(h_j)) / (2 pi 16 15e3) 1e6: blocks are 16 subcarriers apart, unambiguous within +-2.08 us
 * Both calls queue their work on the caller's stream with no host synchronisation (descriptors through pinned buffers); the sequence tables
 * of each (M_sc, n_srs) are made on the host on first use and kept on the device. Grids are [nof_sf][nsym][12 nof_prb] (nsym 14 / 12), one
 * antenna; subframe b is TTI tti0 + b. d_res and d_ce may be device-visible pinned host memory.
 * srslte_hip_srs_create returns NULL for a cell outside 6-110 PRB, TDD, subframe_config >= 15, bw_cfg >= 8 and a bw_cfg whose
 * m_srs_b[0][bw_cfg] exceeds nof_prb (6 PRB with bw_cfg < 7: the reference then computes a negative k0 in unsigned arithmetic and writes
 * outside the grid). A call returns SRSLTE_ERROR_INVALID_INPUTS before anything is queued for B > 3, b_hop > 3, n_srs > 7, k_tc > 1,
 * I_srs >= 637, n_rrc > 23, sf >= nof_sf, nof > max_srs.
 * Not here: TDD and UpPTS, aperiodic (DCI-triggered) SRS, antenna selection, several receive antennas, and the single-call drop-in, whose
 * refsignal_ul.c remains the reference's. */
#define SRSLTE_HIP_SRS_MAX_CE 72    /* M_sc / 8 at 96 PRB */
typedef struct srslte_hip_srs srslte_hip_srs_t;
typedef struct {
  uint32_t nof_prb, cell_id;
  int      cp_ext;                  /* srslte_cell_t.cp == SRSLTE_CP_EXT */
  uint32_t subframe_config;         /* 0-14: srs-SubframeConfig (Table 5.5.3.3-1) */
  uint32_t bw_cfg;                  /* 0-7: srs-BandwidthConfig C_SRS */
  int      group_hopping_en, sequence_hopping_en; /* srslte_refsignal_dmrs_pusch_cfg_t, which the SRS sequence shares */
  uint32_t delta_ss;                /* 0-29; selects v only (u is taken with delta_ss = 0) */
  uint32_t max_srs;                 /* entries per call */
  int      tdd;                     /* refused */
} srslte_hip_srs_cfg_t;
typedef struct {                    /* one (subframe, UE): srslte_refsignal_srs_cfg_t's UE-specific part */
  uint32_t sf;                      /* 0 .. nof_sf-1 */
  uint32_t B, b_hop;                /* 0-3: srs-Bandwidth, srs-HoppingBandwidth */
  uint32_t n_srs;                   /* 0-7: cyclic shift */
  uint32_t I_srs;                   /* 0-636: srs-ConfigIndex (36.213 Table 8.2-1) */
  uint32_t k_tc;                    /* 0, 1: transmission comb */
  uint32_t n_rrc;                   /* 0-23: freqDomainPosition */
  uint32_t cs_used;                 /* receive only: bit c set = some UE uses cyclic shift c on these REs in that subframe (own bit implied) */
} srslte_hip_srs_ue_t;
typedef struct {                    /* per request */
  float    rsrp, noise_estimate, noise_estimate_dbm, snr, snr_db, ta_us;
  uint32_t nof_ce;                  /* J: entries of the request's d_ce row that were written */
} srslte_hip_srs_res_t;
srslte_hip_srs_t* srslte_hip_srs_create(const srslte_hip_srs_cfg_t* cfg);
void              srslte_hip_srs_destroy(srslte_hip_srs_t* q);
/* d_grid [nof_sf][nsym][12 nof_prb] */
int srslte_hip_srs_tx_put(srslte_hip_srs_t* q, uint32_t tti0, uint32_t nof_sf, const srslte_hip_srs_ue_t* list, uint32_t nof, void* d_grid, void* stream);
/* d_res [nof]; d_ce [nof][SRSLTE_HIP_SRS_MAX_CE] cf32 */
int srslte_hip_srs_rx_batch(srslte_hip_srs_t* q, const void* d_grid, uint32_t tti0, uint32_t nof_sf, const srslte_hip_srs_ue_t* list, uint32_t nof,
                            srslte_hip_srs_res_t* d_res, void* d_ce, void* stream);
/* srslte_hip_ul_rx_batch_grants_pucch plus the SRS requests of srs_list, read from the pipeline's own grid right after its SC-FDMA
 * demodulation. ctrl and srs may each be NULL (then their lists are not looked at); objects given must be made for the receiver's cell. */
int srslte_hip_ul_rx_batch_grants_pucch_srs(srslte_hip_ul_rx_t* q, const void* d_iq, uint32_t tti0, uint32_t nof_sf, const srslte_hip_ul_grant_t* grants,
                                            uint32_t nof_grants, uint8_t* d_tb, uint32_t tb_stride, uint8_t* d_tb_ok, srslte_hip_ul_ctrl_t* ctrl,
                                            const srslte_hip_pucch_req_t* reqs, uint32_t nof_pucch, srslte_hip_pucch_res_t* d_res, srslte_hip_srs_t* srs,
                                            const srslte_hip_srs_ue_t* srs_list, uint32_t nof_srs, srslte_hip_srs_res_t* d_srs_res, void* d_srs_ce,
                                            void* stream);
/* host helpers (no device needed). srslte_refsignal_srs_send_cs / _send_ue (1, 0, or < 0 for invalid input); _rb_start_cs / _rb_L_cs
 * (:881-894); M_sc and k0 of a UE at a TTI (0 where srs_k0_ue gives 0); the two shortened decisions (:750-814; ue NULL / ue_configured 0:
 * srs_cfg->configured false; format: srslte_pucch_format_t, 0-2 are formats 1 / 1a / 1b); srslte_refsignal_srs_gen into r [2][M_sc] cf32;
 * srslte_hip_srs_check: what create (list NULL, nof 0) and a call with this list would refuse, SRSLTE_SUCCESS otherwise. */
int      srslte_hip_srs_send_cs(uint32_t subframe_config, uint32_t sf_idx);
int      srslte_hip_srs_send_ue(uint32_t I_srs, uint32_t tti);
uint32_t srslte_hip_srs_rb_start_cs(uint32_t bw_cfg, uint32_t nof_prb);
uint32_t srslte_hip_srs_rb_L_cs(uint32_t bw_cfg, uint32_t nof_prb);
uint32_t srslte_hip_srs_M_sc(const srslte_hip_srs_cfg_t* cfg, const srslte_hip_srs_ue_t* ue);
uint32_t srslte_hip_srs_k0(const srslte_hip_srs_cfg_t* cfg, const srslte_hip_srs_ue_t* ue, uint32_t tti);
int      srslte_hip_srs_pusch_shortened(const srslte_hip_srs_cfg_t* cfg, const srslte_hip_srs_ue_t* ue, uint32_t tti, const uint32_t n_prb_tilde[2],
                                        uint32_t L_prb);
int      srslte_hip_srs_pucch_shortened(const srslte_hip_srs_cfg_t* cfg, int ue_configured, int simul_ack, uint32_t format, uint32_t tti);
int      srslte_hip_srs_gen(const srslte_hip_srs_cfg_t* cfg, const srslte_hip_srs_ue_t* ue, uint32_t sf_idx, void* r);
int      srslte_hip_srs_check(const srslte_hip_srs_cfg_t* cfg, uint32_t tti0, uint32_t nof_sf, const srslte_hip_srs_ue_t* list, uint32_t nof);

/* ------------------------------------------------------------------ UE synchronisation: PSS / SSS search, CFO estimate and correction, FDD
 * srslte_hip_sync_find_batch runs, for every item of a batch, what the FIRST srslte_sync_find (lib/src/phy/sync/sync.c:618-839) on a freshly
 * initialised and reset srslte_sync_t returns, with cfo_i_enable false, decimate 1, detect_frame_type false, frame_type FDD and
 * sss_channel_equalize false: the moving averages are in their reset state, so the first CFO estimates are the means, M_norm_avg / M_ext_avg
 * start from 0 and the correlation average starts from zeros. Averaging across calls is the caller's business (the call keeps no state).
 * Item b is the cf32 samples d_in[b in_stride .. b in_stride + in_stride); the first frame_size of them are the reference's frame.
 *   CP-based CFO (cfo_cp_enable): srslte_cp_synch (cp.c:61-77) over min(max_offset, fft_size) offsets and cfo_cp_nsymbols symbols of normal
 *     CP, every seventh one sample longer; cfo_cp = -arg(corr[argmax |corr|]) / 2 pi. The frame is then read rotated by -cfo_cp / fft_size
 *     cycles per sample (index 0 = the item's first sample) by every later stage; no corrected copy is written. The phase is exact at every
 *     index (the reference multiplies by a table or a running phasor).
 *   PSS search: the replica of srslte_pss_init_N_id_2 (offset 0, conjugated, 1 / sqrt(fft_size) / 62). max_offset >= fft_size: the linear
 *     convolution of the max_offset samples from find_offset on with it, of which max_offset + fft_size - 2 values enter the maximum
 *     (pss.c:493-506); max_offset < fft_size (tracking): the dot products of pss.c:485-490, max_offset - 1 values, peak_pos = index + fft_size.
 *     |c|^2, times ema_alpha when 0 < ema_alpha < 1 (the first update of an average that starts from 0). ema_alpha: 0 selects the 0.2 of
 *     srslte_pss_init, 1 is what ue_sync.c:369,397 set for the find object. First maximum; peak_value is compute_peak_sidelobe (pss.c:412-441)
 *     and - as the reference passes no output when threshold is 0 - stays 0 then; corr_peak is the averaged |c|^2 at the peak.
 *   Found: peak_value >= threshold or threshold == 0; else ret = SRSLTE_SYNC_NOFOUND (0) and nothing below runs.
 *   PSS-based CFO (cfo_pss_enable and peak_pos >= fft_size): on the fft_size samples before find_offset + peak_pos; with pss_filt_enable
 *     through srslte_pss_filter (the 62 bins around DC of the mirrored, unnormalised transform, transformed back - computed as the product of
 *     those bins with the transform of the replica's halves, which is the same sum); srslte_pss_cfo_compute on the two halves.
 *   peak_pos + find_offset >= 2 (fft_size + CP_EXT) (else ret = SRSLTE_SYNC_FOUND_NOSPACE, 2):
 *     SSS (sss_en): the symbol at sss_idx = find_offset + peak_pos - 2 symbol_sz(cp) + cp_sz(cp) with cp the configured one; sss_idx < 0:
 *     sss_available = 0. Rotated by -cfo_pss / fft_size when cfo_pss_enable; extract_pair_sss (find_sss.c:65-95), the m0 / m1 search of
 *     sss_alg, srslte_sss_N_id_1 with sss_threshold, srslte_sss_subframe. item.N_id_1 >= 0: the known-cell branch (sync.c:507-536), the
 *     ratio of the correlations with the cell's subframe-0 and subframe-5 sequences against 1.2 (taken on the 62 bins; the reference takes
 *     it in the time domain after srslte_pss_filter, the same sums times fft_size); m0 = m1 = 0 then.
 *     CP detection (detect_cp): srslte_sync_detect_cp (sync.c:440-495); cp is the configured one otherwise. ret = SRSLTE_SYNC_FOUND (1).
 *   N_id_1 is -1 (the reference's field holds 1000) and cell_id -1 while no SSS was detected and none was given; sf_idx, sss_corr are 0 then.
 *   cfo_cp, cfo_pss (the means after this first call; 0 for a stage that did not run) and cfo = cfo_cp + cfo_pss are in subcarriers.
 * item.N_id_2 = 3 tries the three hypotheses: such an item has three result rows (N_id_2 = 0, 1, 2), every other item one. Rows are in item
 * order: d_res must hold sum over items of (1 or 3) rows; the CP stage runs once per item. d_res may be device-visible pinned host memory.
 * A call makes three launches (two without cfo_cp_enable) on the caller's stream and no host synchronisation; calls on one object queued
 * back to back on one stream are each correct. Kernels use no scratch memory and at most 40 KB of LDS.
 * srslte_hip_sync_create returns NULL, and srslte_hip_sync_find_batch / srslte_hip_sync_check return SRSLTE_ERROR_INVALID_INPUTS before anything
 * is queued, for: an fft_size outside 64..2048 or no multiple of 64; tdd or decimate > 1; max_offset < 2; max_items 0 or above 21845 (three rows per item, 65535 rows per launch); frame_size <
 * max_offset; cp not 0 / 1; sss_alg > 2; a negative threshold or ema_alpha; cfo_cp_enable with cfo_cp_nsymbols 0 or with the CP stage's reach
 * (min(max_offset, fft_size) - 1 + the symbols' lengths) beyond frame_size; and per call: null pointers, n > max_items, frame_size >
 * in_stride, N_id_2 > 3, N_id_1 >= 168, find_offset + max_offset > frame_size, and a window whose last possible peak would make the CFO, SSS
 * or CP stage read past the item: find_offset + max_offset + fft_size - 2 > in_stride, or in the tracking branch find_offset + max_offset +
 * fft_size > in_stride (the reference reads these samples from a buffer of frame_size; give items fft_size samples of room after the frame
 * when max_offset = frame_size; the furthest sample actually read is find_offset + max_offset + fft_size - 4, so both bounds
 * are on the safe side by one and by three samples, the second because the reference's loop forms all max_offset products although max_offset - 1 enter the maximum). Every read stays
 * inside [0, in_stride) of its own item.
 * srslte_hip_cfo_correct_batch: out[b stride + i] = in[b stride + i] exp(j 2 pi freq[b] i), i < len (srslte_cfo_correct / srslte_vec_apply_cfo
 * with freq in cycles per sample); the phase is the fractional part of freq[b] i taken in double, so it is as exact at sample 150 000 as at
 * sample 0 (the reference's running phasor drifts). d_out == d_in is allowed; freq is a host array read before the call returns.
 * Not here: decimation, the integer-CFO stage, SSS equalisation from the PSS channel estimate, srslte_pss_sic, ue_sync's find / track state
 * machine, and the single-call drop-in (NB-IoT: see "NB-IoT synchronisation" below), whose sync directory remains the reference's over srslte_dft_*. TDD positions, frame-type
 * detection and the averages across calls are the tracked call's ("UE synchronisation: tracks" below); this call stays FDD and stateless. */
typedef struct srslte_hip_sync_s srslte_hip_sync_t;
typedef struct {
  uint32_t fft_size;          /* 64..2048, multiple of 64 */
  uint32_t frame_size;        /* samples of an item that make the reference's frame (srslte_sync_init's frame_size) */
  uint32_t max_offset;        /* positions the PSS is searched over (srslte_sync_init's max_offset) */
  uint32_t max_items;         /* items per call */
  int      cp;                /* srslte_cp_t (0 normal, 1 extended): the CP assumed by the SSS stage, and the result's when detect_cp is 0 */
  uint8_t  detect_cp, sss_en, cfo_cp_enable, cfo_pss_enable, pss_filt_enable;
  uint8_t  sss_alg;           /* 0 DIFF, 1 PARTIAL_3, 2 FULL (sync.c:538-548) */
  uint8_t  tdd, reserved;     /* tdd: refused */
  uint32_t cfo_cp_nsymbols;   /* srslte_sync_set_cfo_cp_enable's second argument */
  float    threshold;         /* on the peak-to-sidelobe ratio; 0: always found */
  float    sss_threshold;     /* srslte_sss_set_threshold */
  float    ema_alpha;         /* srslte_sync_set_em_alpha; 0: the default 0.2 */
  uint32_t decimate;          /* 0 or 1; more is refused */
} srslte_hip_sync_cfg_t;
typedef struct {
  uint32_t N_id_2;            /* 0..2, or 3: all three, one result row per hypothesis */
  uint32_t find_offset;
  int32_t  N_id_1;            /* >= 0: known cell (srslte_sync_set_N_id_1); < 0: the m0 / m1 search */
} srslte_hip_sync_item_t;
typedef struct {              /* one per (item, hypothesis), 16 x 4 bytes */
  int32_t  ret;               /* srslte_sync_find_ret_t: 1 FOUND, 2 FOUND_NOSPACE, 0 NOFOUND */
  uint32_t peak_pos;
  float    peak_value;        /* the peak-to-sidelobe ratio */
  float    corr_peak;         /* pss.peak_value */
  float    cfo_cp, cfo_pss, cfo;
  uint32_t sss_available, sss_detected, m0, m1, sf_idx;
  int32_t  N_id_1, cell_id;
  float    sss_corr;
  int32_t  cp;
} srslte_hip_sync_res_t;
typedef struct {              /* srslte_ue_cellsearch_result_t without the frame type */
  uint32_t cell_id;
  int      cp;
  float    peak;              /* mean corr_peak of the frames */
  float    mode;              /* share of the frames that gave cell_id */
  float    psr;               /* the last frame's peak_value */
  float    cfo;               /* the last frame's cfo in Hz (15000 cfo) */
  uint32_t nof_frames;        /* rows that counted */
} srslte_hip_cell_search_result_t;
srslte_hip_sync_t* srslte_hip_sync_create(const srslte_hip_sync_cfg_t* cfg);
void               srslte_hip_sync_destroy(srslte_hip_sync_t* q);
/* in_stride in cf32 samples per item; d_res [rows] */
int srslte_hip_sync_find_batch(srslte_hip_sync_t* q, const void* d_in, size_t in_stride, const srslte_hip_sync_item_t* items, uint32_t n,
                               srslte_hip_sync_res_t* d_res, void* stream);
int srslte_hip_cfo_correct_batch(const void* d_in, void* d_out, size_t stride, uint32_t len, uint32_t n, const float* freq, void* stream);
/* host (no device needed): what create and a call with these items would refuse; and get_cell of ue_cell_search.c:189-250 over the rows of
 * one N_id_2, one per scanned 5 ms frame in scan order: rows with ret != 1 or cell_id < 0 do not count (:311-332); the mode of the cell ids
 * (the first on a tie), normal CP if more than half of that id's rows (integer half) say so, the mean corr_peak, the last row's peak_value
 * and cfo. Returns the number of rows that counted; 0: no cell, *out zeroed. Choosing the N_id_2 with the largest peak is
 * srslte_ue_cellsearch_scan (:257-280). */
int srslte_hip_sync_check(const srslte_hip_sync_cfg_t* cfg, size_t in_stride, const srslte_hip_sync_item_t* items, uint32_t n);
int srslte_hip_cell_search_decide(const srslte_hip_sync_res_t* found, uint32_t nof_found, srslte_hip_cell_search_result_t* out);
/* TEST AND DIAGNOSTIC ENTRY: the CP stage's correlations of item b of the last call, min(max_offset, fft_size) cf32 values to the host
 * (synchronises the device) */
int srslte_hip_sync_cp_corr(srslte_hip_sync_t* q, uint32_t item, void* h_corr);

/* ------------------------------------------------------------------ UE synchronisation: tracks - a srslte_sync_t's state across calls, TDD
 * A tracks object belongs to a srslte_hip_sync_t (destroy it first) and holds, on the device, the state of n_tracks independent srslte_sync_t
 * that share the sync object's configuration: one track per UE or per scan. srslte_hip_sync_track_batch runs ONE srslte_sync_find per item on
 * the item's track - whatever number of calls the track has seen - and leaves the row the reference's getters would show afterwards. A track
 * that was just created or reset with flags 7, in frame mode 0, gives in the first 16 words the very row of srslte_hip_sync_find_batch.
 * State a call reads and leaves (lines of lib/src/phy/sync/):
 *   pss.conv_output_avg (pss.c:495-503): with 0 < ema_alpha < 1 the track's own row, avg = alpha |c|^2 + (1 - alpha) avg, kept; otherwise
 *     |c|^2 overwrites it and nothing is kept. The maximum, the lobe search (peak_value) and corr_peak work on the averaged values.
 *   cfo_cp_mean / cfo_cp_is_set (sync.c:660-676): the first estimate is the mean, later ones enter by SRSLTE_VEC_EMA with cfo_ema_alpha; the
 *     frame is read rotated by the mean AFTER the update. cfo_cp is the mean, cfo_cp_inst this call's estimate.
 *   cfo_pss_mean / cfo_pss_is_set (sync.c:704-726): the first estimate is the mean; later ones are averaged in only while
 *     15000 |cfo_pss| < 7000. The SSS symbol is rotated by the mean (also in a call whose PSS stage did not run). cfo_pss is the mean.
 *   M_norm_avg / M_ext_avg: srslte_sync_detect_cp's averages with the constant 0.1 (sync.c:468,479).
 *   cp: detect_cp writes it (sync.c:813); the NEXT call's SSS position uses it. It starts as cfg.cp.
 *   N_id_1, sf_idx, sss_corr, peak_value, frame_type: a call that does not write them leaves the previous values, and the row shows those -
 *     an undetected SSS outside detect mode, a peak with no room for the SSS stage (ret 2), no peak (ret 0), and for peak_value threshold 0
 *     (the found test then reads the kept value, as sync.c:702 does). They start as -1 (cell_id -1), 0, 0, 0 and FDD (TDD in frame mode 1).
 *     item.N_id_1 >= 0 is srslte_sync_set_N_id_1 before the call: the known-cell branch, and the track's N_id_1 from then on.
 *   sss_detected is cleared by every call; sss_available is written where the SSS stage runs and kept otherwise; m0 / m1 are this call's
 *     (0 where no m0 / m1 search ran); nof_calls counts the calls since the track was made or reset with flag 4.
 * Frame modes (sync.c:732-809). 0: FDD, as the stateless call. 1 (TDD): the SSS symbol at find_offset + peak_pos - 4 symbol_sz(cp) +
 * cp_sz(cp) - the reference's expression, which neglects the slot's longer first CP - and sf_idx = srslte_sss_subframe + 1. 2 (detect, what
 * srslte_sync_init leaves): both trials, FDD then TDD, each through sss_alg or the known-cell branch; sss_detected is the OR; FDD wins when
 * sss_corr[0] > sss_corr[1], otherwise TDD; frame_type, sf_idx (+ 1 for TDD), sss_corr, m0 / m1 and N_id_1 are the winning trial's, whether
 * or not it detected. The CP and PSS stages do not depend on the frame type. Two cases the reference leaves to uninitialised stack values
 * are defined here: a trial whose symbol would start before the item's first sample (sss_idx < 0) does not run, sss_available = 0, its
 * correlation counts as lower than any other so it cannot win, and its sss_corr_trial is NaN (only the TDD trial can lack room once ret is
 * 1: in mode 1 nothing is written then, in mode 2 the FDD trial wins); and a winning m0 / m1 trial that detected nothing leaves the track's
 * previous N_id_1 and cell_id.
 * Reads: the TDD trial reads two symbols further back than the FDD one, never further on, and a trial with sss_idx < 0 reads nothing; so the
 * window checks are those of srslte_hip_sync_find_batch and every read stays inside [0, in_stride) of its own item.
 * One call holds at most one item per track. Calls on one tracks object queued back to back on one stream see each other's state in order;
 * there is no host synchronisation and no allocation in a call, three launches (two without cfo_cp_enable). The calls' temporaries are the
 * sync object's: tracked and stateless calls on one sync object belong on one stream. reset and copy_cfo are one launch each.
 * Refused with SRSLTE_ERROR_INVALID_INPUTS before anything is queued, d_res and the state untouched: what srslte_hip_sync_find_batch refuses,
 * n_tracks 0 or above 65535, frame_mode > 2, a negative cfo_ema_alpha, track >= n_tracks, a track named twice in one call, N_id_2 > 2 (one
 * srslte_sync_t has one PSS object), reset flags > 7, and in copy_cfo an index out of range or a destination named twice.
 * Not here: see the list above; cfg.tdd of srslte_hip_sync_cfg_t stays refused - the frame mode is a property of the tracks object. */
typedef struct srslte_hip_sync_tracks_s srslte_hip_sync_tracks_t;
typedef struct {
  uint32_t n_tracks;
  float    cfo_ema_alpha;     /* srslte_sync_set_cfo_ema_alpha; 0: the 0.1 of sync.c:34 */
  uint32_t frame_mode;        /* 0 FDD (srslte_sync_set_frame_type FDD), 1 TDD, 2 detect */
} srslte_hip_sync_tracks_cfg_t;
typedef struct {
  uint32_t track, N_id_2 /* 0..2 */, find_offset;
  int32_t  N_id_1;            /* >= 0: known cell; < 0: the m0 / m1 search */
} srslte_hip_sync_track_item_t;
typedef struct {              /* 24 x 4 bytes; the first 16 words are srslte_hip_sync_res_t */
  srslte_hip_sync_res_t r;
  int32_t  frame_type;        /* 0 FDD, 1 TDD: q->frame_type after the call */
  float    sss_corr_trial[2]; /* FDD, TDD trial of this call; NaN for a trial that did not run */
  uint32_t nof_calls;         /* this one included */
  float    cfo_cp_inst, cfo_pss_inst; /* this call's estimates before averaging; 0 for a stage that did not run */
  float    M_norm_avg, M_ext_avg;
} srslte_hip_sync_track_res_t;
typedef struct {              /* the scalars of one track, 16 x 4 bytes */
  float    cfo_cp_mean, cfo_pss_mean;
  uint32_t cfo_cp_is_set, cfo_pss_is_set;
  float    M_norm_avg, M_ext_avg, peak_value, sss_corr;
  int32_t  cp, N_id_1, frame_type;
  uint32_t sf_idx, sss_available, nof_calls;
  float    cfo_cp_inst;       /* the CP stage's last estimate */
  uint32_t reserved;
} srslte_hip_sync_track_state_t;
#define SRSLTE_HIP_SYNC_RESET_AVG 1u   /* srslte_sync_reset (sync.c:841-845): M_norm_avg, M_ext_avg and the PSS average to zero */
#define SRSLTE_HIP_SYNC_RESET_CFO 2u   /* srslte_sync_cfo_reset (sync.c:346-352) */
#define SRSLTE_HIP_SYNC_RESET_REST 4u  /* cp = cfg.cp, N_id_1, sf_idx, sss_corr, peak_value, sss_available, frame type, nof_calls as created */
srslte_hip_sync_tracks_t* srslte_hip_sync_tracks_create(srslte_hip_sync_t* q, const srslte_hip_sync_tracks_cfg_t* cfg);
void                      srslte_hip_sync_tracks_destroy(srslte_hip_sync_tracks_t* k);
int srslte_hip_sync_track_batch(srslte_hip_sync_tracks_t* k, const void* d_in, size_t in_stride, const srslte_hip_sync_track_item_t* items, uint32_t n,
                                srslte_hip_sync_track_res_t* d_res, void* stream);
/* idx NULL: all tracks (n is ignored) */
int srslte_hip_sync_tracks_reset(srslte_hip_sync_tracks_t* k, const uint32_t* idx, uint32_t n, uint32_t flags, void* stream);
/* srslte_sync_copy_cfo (sync.c:354-360) from src's track src_idx[i] to dst's track dst_idx[i]: the two means, and both is_set flags cleared, so
 * the destination's next estimate REPLACES the mean. dst and src may belong to different sync objects (queue both on one stream). */
int srslte_hip_sync_tracks_copy_cfo(srslte_hip_sync_tracks_t* dst, const uint32_t* dst_idx, srslte_hip_sync_tracks_t* src, const uint32_t* src_idx,
                                    uint32_t n, void* stream);
/* TEST AND DIAGNOSTIC ENTRY: the scalars of one track to the host (synchronises the device) */
int srslte_hip_sync_tracks_read(srslte_hip_sync_tracks_t* k, uint32_t track, srslte_hip_sync_track_state_t* h_state);
/* host (no device needed): what create and a call with these items would refuse; and srslte_hip_cell_search_decide over tracked rows, with
 * the frame type by get_cell's majority rule (ue_cell_search.c:216-242): FDD (0) when more than the integer half of the winning id's rows
 * say FDD, else TDD (1) */
int srslte_hip_sync_tracks_check(const srslte_hip_sync_cfg_t* cfg, const srslte_hip_sync_tracks_cfg_t* tracks_cfg, size_t in_stride,
                                 const srslte_hip_sync_track_item_t* items, uint32_t n);
int srslte_hip_cell_search_decide_ft(const srslte_hip_sync_track_res_t* found, uint32_t nof_found, srslte_hip_cell_search_result_t* out,
                                     int32_t* frame_type);

/* ------------------------------------------------------------------ Neighbour-cell measurement: CRS search, RSRP, RSRQ and CFO, FDD, normal CP
 * srslte_hip_meas_run_batch leaves, per (capture, candidate cell), what srslte_refsignal_dl_sync_run (lib/src/phy/sync/refsignal_dl_sync.c:
 * 242-301) leaves in a srslte_refsignal_dl_sync_t after srslte_refsignal_dl_sync_set_cell - the job srsue/src/phy/scell/intra_measure.cc:
 * 160-235 runs once per candidate cell on a capture of intra_freq_meas_len_ms subframes. Capture c is the cf32 samples d_in[c in_stride ..
 * c in_stride + nof_sf sf_len), sf_len = 15 symbol_sz; L below is sf_len.
 *   Replicas (set_cell, :84-154; srslte_hip_meas_set_cells): for subframe i = 0..9 of a cell a grid with PSS + SSS in subframes 0 and 5
 *     (srslte_pss_put_slot / srslte_sss_put_slot) and the CRS of ports 0 AND 1 whatever the cell's port count (:128-139; both ports carry the
 *     same r_l,ns(m) at their own positions), through the un-normalised OFDM modulator, times 1 / (8 nof_prb) (:145, nof_re of port 0).
 *   Search (find_peak, :185-240): min(nof_sf - 1, 10) blocks; block b gives c[k] = sum_{m<L} x[b L + k + m] conj(seq0[m]), k < L - what the
 *     reference's normalised forward and un-normalised backward transforms of 2 L points leave in the first L outputs, a linear correlation
 *     with no wrap-around. Per block the first maximum of |c|^2, peak = |c[imax]|, rms = sqrt(mean |c|^2); the overall peak is the first block
 *     whose peak is strictly larger; found when peak > threshold mean(rms).
 *   Measurement (run :255-291, measure_sf :303-355): from n = peak_index % L and sf_idx = (20 - peak_index / L) % 10, stepping by L while
 *     n < nof_sf L - L + 1: on the four CRS symbols of port 0 (symbols 0, 4, 7, 11 at the window offsets of :317-327) corr[l] over symbol_sz
 *     samples against the replica of that subframe index and the symbol's power; rsrp = 4 sum |corr[l]|^2, rssi = nof_prb sum power / 4 x 7.41,
 *     cfo = the mean of arg(corr[2] conj corr[0]) and arg(corr[3] conj corr[1]) over 2 pi 7.5 x 15000. Averages over the subframes (nof_sf of
 *     the row: how many were measured; sf_idx: the first one's index); dB figures carry + 30; rsrq = 10 log10(nof_prb) + rsrp - rssi.
 *   Not found: found = 0, rsrp_lin, rssi_lin, the three dB figures and cfo_Hz are NaN, peak_index = UINT32_MAX, sf_idx = nof_sf = 0;
 *     peak_value and rms_avg are what the search saw.
 * Device side (csrc/meas.hip, the row transforms in csrc/fft.hip). 2 L = 30 symbol_sz for every symbol size, so the 2 L-point transforms are
 * four-step: 30-point column DFTs (a lane per n2 reads 30 rows at stride symbol_sz), the inter-stage twiddle from a 2 L-entry table built in
 * double on the host, and symbol_sz-point row FFTs through the fixed LDS plans of the OFDM kernels. Spectra stay in [k1][k2] order (k = k1 +
 * 30 k2): the product is pointwise, so nothing is transposed. The forward transform of a block is computed once and shared by all candidate
 * cells; per (capture, cell, block) the product with the conjugated filter spectrum rides on the loads of the inverse's row pass; the closing
 * 30-point pass forms only the L outputs that count and reduces them on the spot to (max |c|^2, first index, sum |c|^2) per workgroup: the
 * correlation itself is never written to memory.
 *   srslte_hip_meas_set_cells: copy + memset + 5 launches (fill, OFDM transmit, scale, column pass, row pass); reads the id list before it
 *     returns and is otherwise asynchronous on the stream. A later run_batch on another stream needs the caller's ordering.
 *   srslte_hip_meas_run_batch: 7 launches (column pass, row pass, product + inverse row pass, closing column pass + reduction, decide, measure -
 *     one workgroup per (row, subframe) -, finish) and no host synchronisation; calls queued back to back on one stream are each correct.
 *   No kernel uses scratch memory or spills. LDS per workgroup: meas_col_inv_kernel at most 2 KB (the reduction), meas_sf_kernel at most 1 KB,
 *   the row passes and the OFDM transmit kernel (N + N / 16 + 2) x 8 bytes of dynamic LDS, 17 424 at N = 2048; the other kernels none.
 * Result rows are capture-major: d_res[c n_cells + k]; d_res may be device-visible pinned host memory. Every read stays inside
 * [0, nof_sf sf_len) of its own capture.
 * srslte_hip_meas_create returns NULL, and the calls return SRSLTE_ERROR_INVALID_INPUTS before anything is queued (result rows untouched),
 * for: extended CP (cp_ext != 0; measure_sf uses normal-CP offsets whatever the cell's CP, so there is nothing to be faithful to); nof_prb
 * outside 6..110 or a symbol_sz srslte_hip_ofdm_create_sz would refuse; max_captures or max_cells 0, max_cells above 504, max_captures
 * max_cells above 65535, max_sf < 2 or max_sf sf_len beyond 32 bits; a negative threshold; nof_sf < 2 or > max_sf; in_stride < nof_sf sf_len; more captures or cells than the object was made for; a
 * cell id above 503; null pointers; run_batch before any set_cells. The capture length is given in whole subframes, as intra_measure.cc does;
 * for other lengths the reference reads past its buffer.
 * Not here: extended CP, TDD positions, MBSFN; the neighbour-list bookkeeping of intra_measure.cc:195-230; averaging across calls; and the
 * single-call drop-in, whose refsignal_dl_sync.c stays the reference's over srslte_dft_*. */
typedef struct srslte_hip_meas_s srslte_hip_meas_t;
typedef struct {
  uint32_t nof_prb;
  uint32_t symbol_sz;         /* 0: srslte_symbol_sz(nof_prb) of the default family */
  uint32_t max_captures, max_cells;
  uint32_t max_sf;            /* subframes per capture */
  float    threshold;         /* on peak / mean(rms); 0: the reference's 5.5 */
  uint32_t cp_ext;            /* refused when not 0 */
} srslte_hip_meas_cfg_t;
typedef struct {              /* one per (capture, cell), 16 x 4 bytes */
  int32_t  found;
  uint32_t peak_index;        /* UINT32_MAX when not found */
  uint32_t sf_idx;            /* subframe index of the first measured subframe */
  uint32_t nof_sf;            /* subframes measured */
  float    peak_value, rms_avg;
  float    rsrp_lin, rssi_lin;
  float    rsrp_dBfs, rssi_dBfs, rsrq_dB, cfo_Hz;
  uint32_t cell_id, capture, reserved[2];
} srslte_hip_meas_res_t;
srslte_hip_meas_t* srslte_hip_meas_create(const srslte_hip_meas_cfg_t* cfg);
void               srslte_hip_meas_destroy(srslte_hip_meas_t* q);
int srslte_hip_meas_set_cells(srslte_hip_meas_t* q, const uint16_t* cell_ids, uint32_t n_cells, void* stream);
/* in_stride in cf32 samples per capture; d_res [n_captures][n_cells of the last set_cells] */
int srslte_hip_meas_run_batch(srslte_hip_meas_t* q, const void* d_in, size_t in_stride, uint32_t nof_sf, uint32_t n_captures,
                              srslte_hip_meas_res_t* d_res, void* stream);
/* host (no device needed): what create and a call of this shape would refuse */
int srslte_hip_meas_check(const srslte_hip_meas_cfg_t* cfg, size_t in_stride, uint32_t nof_sf, uint32_t n_captures, uint32_t n_cells);
/* TEST AND DIAGNOSTIC ENTRY: the time-domain replicas of cell k of the last set_cells, [10][sf_len] cf32, to the host (synchronises the
 * device) */
int srslte_hip_meas_replicas(srslte_hip_meas_t* q, uint32_t cell, void* h_seq);

/* ------------------------------------------------------------------ NB-IoT synchronisation: NPSS / NSSS search and CFO, fft_size 128
 * One object serves both signals of lib/src/phy/sync/{npss.c, nsss.c, sync_nbiot.c}. Item b of a call is the cf32 samples d_in[b in_stride ..
 * b in_stride + in_stride). Both replicas have 1508 samples: 11 OFDM symbols of 128 samples with CP 9, and CP 10 for the fifth one.
 * A replica symbol i with frequency values S[i][sc] is, for t < 128 + cp_i (npss.c:170-239, nsss.c:144-229),
 *   h[s_i + t] = 1 / sqrt(128) sum_sc S[i][sc] exp(j 2 pi (f_sc + 1/2) (t - cp_i) / 128),   s_i = 137 i + (i > 4)
 * - the mirrored inverse transform with set_dc(false), which maps buffer index k to frequency k - 64 (dft_fftw.c:249-260: no bin is skipped),
 * so f_sc = sc - 6 for the 11 NPSS values at index (128 - 12) / 2 and f_sc = sc - 7 for the 12 NSSS values at index 57; the CP is the
 * periodic continuation, and the half-subcarrier table (offset 412 = SRSLTE_NPSS_CORR_OFFSET into a subframe) restarts in every symbol.
 * The NPSS replica carries the further factor 1 / 3, the NSSS one does not (nsss.c:213).
 *
 * srslte_hip_nbiot_npss_find_batch: one srslte_sync_nbiot_find (sync_nbiot.c:189-254) per item on the item's track. A track is a
 * srslte_sync_nbiot_t's state on the device: conv_output_avg and mean_cfo.
 *   CFO pre-correction: every sample the search reads is rotated by -mean_cfo / 128 cycles per sample, index 0 = the item's first sample, the
 *     phase exact at every index (as srslte_hip_cfo_correct_batch); no corrected copy is written. (The reference's srslte_vec_apply_cfo runs a
 *     float phasor that drifts along the frame, and corrects frame_size samples from the item's start, so with find_offset > 0 the tail of
 *     its window is whatever its buffer held before; here every sample of the window is the item's own, rotated.)
 *   Correlation, frame_size >= 128 (npss.c:257-264, convolution.c:31-63,130-136): c[n] = sum_k x[(n + k) mod L] conj(h[k]), L = frame_size +
 *     1508, x the frame_size samples from find_offset on and zero from frame_size on - the two 1 / sqrt(L) and the unnormalised inverse
 *     cancel. srslte_corr_fft_cc_run_opt returns L - 1 as conv_output_len, and npss.c:273-288 works on conv_output_len - 1 values: nout = L - 2
 *     lags enter the average and the maximum; lags frame_size .. L - 3 are the partial overlaps before the frame.
 *     frame_size < 128 (npss.c:266-269): c[i] = sum_{t<128} h[t] x[i + t], NOT conjugated, conv_output_len = frame_size, nout = frame_size - 1.
 *     The reference reads these samples from a buffer it corrected only up to frame_size; here they are the item's samples, rotated.
 *   |c|^2; with 0 < npss_ema_alpha < 1 avg = alpha |c|^2 + (1 - alpha) avg over the nout values (npss.c:278-285), otherwise avg = |c|^2.
 *   peak_pos = the first maximum of avg; corr_peak = avg[peak_pos]; peak_value = the peak-to-sidelobe ratio of npss.c:301-343 as it walks:
 *     the right walk tests avg[pl_ub + 1] before pl_ub < conv_output_len, so it reads up to index conv_output_len + 1 of a buffer whose
 *     entries from nout on are zero and may end at conv_output_len; the left walk stops at 1; an empty side-lobe range gives index pl_ub
 *     on the right and index 0 on the left (srslte_vec_max_fi of length 0). ret = 1 when peak_value >= threshold, else 0.
 *   CFO stage (cfo_enable; sync_nbiot.c:224-242, :257-265): entered only when peak_pos + 548 + 823 + 128 < frame_size (SRSLTE_NPSS_CFO_OFFSET,
 *     SRSLTE_NPSS_CFO_NUM_SAMPS). It reads the UNCORRECTED item from index peak_pos + 548 - not offset by find_offset, as the reference
 *     indexes it -, the first 823 samples multiplied by the second half of the half-subcarrier table on the fly (the reference overwrites
 *     its input, the device leaves it alone; samples from 823 on are read as they are); srslte_cp_synch (cp.c:61-77) over min(max_offset,
 *     128) offsets, 6 symbols of CP 9, the first one sample longer; cfo = -arg(corr[first argmax |corr|^2]) / 2 pi, then mean_cfo = alpha
 *     cfo + (1 - alpha) mean_cfo with cfo_ema_alpha. The stage's furthest read is peak_pos + 548 + 127 + 822 < frame_size.
 *   Row: ret, peak_pos, peak_value, corr_peak, cfo (this call's estimate; NaN when the stage did not run), mean_cfo after the call.
 *   A track may be named once per call. Calls queued on one stream apply in order. The candidate test of sync_nbiot.c:200-203 is a caller's
 *   loop over srslte_hip_nbiot_sync_tracks_set_cfo.
 * srslte_hip_nbiot_nsss_find_batch: srslte_nsss_sync_find (nsss.c:231-281, :284-344) on the first 3840 samples of every item.
 *   Per cell id the circular correlation over L = 5348 with that id's replica, |c| = sqrt(re^2 + im^2) (srslte_vec_abs_cf: not squared), the
 *   first maximum over L - 2 = 5346 lags (conv_output_len - 1, as above). cell_ids[b] in 0..503 runs that id; -1 runs all 504 and the first
 *   maximum of the 504 peaks wins. found = peak_value > nsss_threshold (strictly). cell_id in the row is the id that was run / that won, also
 *   when found is 0 (the reference leaves its argument alone then); sfn_partial is 0: only theta_f = 0 is searched (nsss.c:192-196,:274).
 *   Sequences: srslte_nsss_generate (nsss.c:348-377) in its float expression order, including its theta_f factor exp(-j 2 pi theta_f n) formed
 *   from an integer theta_f in float. b_q(m) = (-1)^popcount(m & c_q), c_q = 0, 31, 63, 127: columns of the 128-point Hadamard matrix.
 *   srslte_hip_nbiot_nsss_debug copies, for an item of the last call, peak_values [504] (entries of ids that did not run are 0) and the
 *   |c| row [5346] of the row's cell_id.
 * Device side (csrc/nbiot_sync.hip), the structure route: with Y_cls,sc[m] = 1 / sqrt(128) sum_t x[(m + t) mod L] exp(-j 2 pi (f_sc + 1/2) (t -
 * cp_cls) / 128), t < 128 + cp_cls, c_id[n] = sum_{i,sc} conj(S_id[i][sc]) Y_cls(i),sc[n + s_i]: 24 sliding correlations of 137 / 138 taps per
 * item, then a [504 x 132] x [132 x lags] complex product in fp32 FMAs on the VALU, 64 ids x 64 lags per workgroup, the table [132][504] and
 * Y streamed through LDS a symbol (12 rows) at a time; only each tile's (maximum, first index) is written. The NPSS has one shared 11-value
 * symbol and 11 signs: one sliding correlation per CP class, then c[n] = sum_i sign_i W_cls(i)[n + s_i].
 *   npss_find_batch: descriptor copy + 3 launches (slide, combine + average + tile maxima, decide + CFO); 2 for frame_size < 128.
 *   nsss_find_batch: descriptor copy + 3 launches (slide, product + tile maxima, decide + debug row). Independent of n and of 504.
 *   tracks_reset, tracks_set_cfo: one launch each. No host synchronisation in any of them; d_res may be device-visible pinned host memory.
 *   No kernel uses scratch memory or spills. Static LDS per workgroup: at most 12 288 bytes (the product kernel: 2 x 12 x 64 cf32; the slide
 *   kernels 4 256; the others at most 4 KB). Temporaries per item: 24 x 6912 cf32 (NSSS), 2 x (L + 1369) cf32 (NPSS).
 * srslte_hip_nbiot_sync_create returns NULL, and the calls and checks return SRSLTE_ERROR_INVALID_INPUTS before anything is queued (result
 * rows and tracks untouched), for: fft_size != 128 (the reference hard-codes SRSLTE_NBIOT_FFT_SIZE in the CP lengths, k = 57 and the offsets);
 * frame_size 0 or above 307 200 (srslte_sync_nbiot_resize's bound; 32-bit indices); max_items 0 or above 8191 (eight product rows per item,
 * 65535 per launch); n_tracks 0 or above 65535; negative thresholds or alphas; and per call: null pointers, n > max_items, track >= n_tracks,
 * a track named twice, find_offset + frame_size (+ 127 for frame_size < 128) > in_stride or beyond 32 bits - which also keeps the CFO stage inside the item -, a
 * cell id outside -1..503, in_stride < 3840 for the NSSS. Every read stays inside [0, in_stride) of its own item.
 * Not here: srslte_ue_sync_nbiot's state machine, the theta_f != 0 hypotheses (the reference searches none), fft_size != 128, decimation,
 * the NSSS peak-to-sidelobe variant (compiled out in the reference), and the single-call drop-in, whose npss.c / nsss.c / sync_nbiot.c remain
 * the reference's over srslte_dft_*. */
#define SRSLTE_HIP_NBIOT_REPLICA_LEN 1508
#define SRSLTE_HIP_NBIOT_NSSS_IN_LEN 3840  /* SRSLTE_NSSS_NUM_SF_DETECT x 1920 */
#define SRSLTE_HIP_NBIOT_NSSS_NOUT 5346    /* 3840 + 1508 - 2 */
#define SRSLTE_HIP_NBIOT_NUM_PCI 504
typedef struct srslte_hip_nbiot_sync_s srslte_hip_nbiot_sync_t;
typedef struct {
  uint32_t fft_size;          /* 128 */
  uint32_t frame_size;        /* what srslte_sync_nbiot_init passes to srslte_npss_synch_init */
  uint32_t max_offset;        /* the CFO stage's srslte_cp_synch offsets (at most 128 count) */
  uint32_t max_items;         /* items per call */
  uint32_t n_tracks;
  float    threshold;         /* on the NPSS peak-to-sidelobe ratio; 0: 5.0 */
  float    nsss_threshold;    /* 0: 2.0 */
  float    npss_ema_alpha;    /* 0: 0.2; 1: no averaging */
  float    cfo_ema_alpha;     /* 0: 0.1 */
  uint32_t cfo_enable;        /* srslte_sync_nbiot_set_cfo_enable */
} srslte_hip_nbiot_sync_cfg_t;
typedef struct {
  uint32_t track, find_offset;
} srslte_hip_nbiot_npss_item_t;
typedef struct {              /* 8 x 4 bytes */
  int32_t  ret;               /* 1 FOUND, 0 NOFOUND */
  uint32_t peak_pos;
  float    peak_value;        /* the peak-to-sidelobe ratio */
  float    corr_peak;         /* the average at the peak */
  float    cfo;               /* this call's estimate in subcarriers; NaN when the CFO stage did not run */
  float    mean_cfo;          /* after the call */
  uint32_t reserved[2];
} srslte_hip_nbiot_npss_res_t;
typedef struct {              /* 8 x 4 bytes */
  int32_t  found;
  int32_t  cell_id;
  float    peak_value;
  uint32_t peak_pos;
  uint32_t sfn_partial;       /* 0 */
  uint32_t reserved[3];
} srslte_hip_nbiot_nsss_res_t;
srslte_hip_nbiot_sync_t* srslte_hip_nbiot_sync_create(const srslte_hip_nbiot_sync_cfg_t* cfg);
void                     srslte_hip_nbiot_sync_destroy(srslte_hip_nbiot_sync_t* q);
/* srslte_npss_synch_reset plus mean_cfo = 0 for tracks first .. first + n - 1 */
int srslte_hip_nbiot_sync_tracks_reset(srslte_hip_nbiot_sync_t* q, uint32_t first, uint32_t n, void* stream);
/* mean_cfo of tracks first .. first + n - 1 = cfo[0 .. n) (srslte_sync_nbiot_set_cfo); cfo is a host array read before the call returns */
int srslte_hip_nbiot_sync_tracks_set_cfo(srslte_hip_nbiot_sync_t* q, uint32_t first, uint32_t n, const float* cfo, void* stream);
/* TEST AND DIAGNOSTIC ENTRY: mean_cfo and, when h_avg is not NULL, the nout averaged values of one track to the host (synchronises the device) */
int srslte_hip_nbiot_sync_tracks_read(srslte_hip_nbiot_sync_t* q, uint32_t track, float* h_mean_cfo, float* h_avg);
/* in_stride in cf32 samples per item; d_res [n] */
int srslte_hip_nbiot_npss_find_batch(srslte_hip_nbiot_sync_t* q, const void* d_in, size_t in_stride, const srslte_hip_nbiot_npss_item_t* items, uint32_t n,
                                     srslte_hip_nbiot_npss_res_t* d_res, void* stream);
int srslte_hip_nbiot_nsss_find_batch(srslte_hip_nbiot_sync_t* q, const void* d_in, size_t in_stride, const int32_t* cell_ids, uint32_t n,
                                     srslte_hip_nbiot_nsss_res_t* d_res, void* stream);
/* TEST AND DIAGNOSTIC ENTRY: of item b of the last NSSS call (synchronises the device); either pointer may be NULL */
int srslte_hip_nbiot_nsss_debug(srslte_hip_nbiot_sync_t* q, uint32_t item, float* h_peak_values, float* h_abs_row);
/* host (no device needed). The checks: what create (items NULL, n 0) and a call with these items / ids would refuse. nout of a frame_size.
 * The sequences: srslte_npss_generate into out [121] cf32, srslte_nsss_generate into out [528] cf32 (nothing written, error, for an id above
 * 503); the two time-domain replicas, [1508] cf32 each. The RE indices srslte_npss_put_subframe (npss.c:425-436) and srslte_nsss_put_subframe
 * (nsss.c:379-398) write in a subframe grid [14][12 nof_prb]: re [121] resp. re [132], entry i receives value i of the NPSS resp. value
 * *first + i of the 528 NSSS values (first = 132 theta_f, theta_f = floor(33 / 132 (nf / 2)) % 4). */
int      srslte_hip_nbiot_sync_check(const srslte_hip_nbiot_sync_cfg_t* cfg, size_t in_stride, const srslte_hip_nbiot_npss_item_t* items, uint32_t n);
int      srslte_hip_nbiot_nsss_check(const srslte_hip_nbiot_sync_cfg_t* cfg, size_t in_stride, const int32_t* cell_ids, uint32_t n);
uint32_t srslte_hip_nbiot_npss_nout(uint32_t frame_size);
int      srslte_hip_nbiot_npss_generate(void* out);
int      srslte_hip_nbiot_nsss_generate(void* out, uint32_t cell_id);
int      srslte_hip_nbiot_npss_replica(void* out);
int      srslte_hip_nbiot_nsss_replica(void* out, uint32_t cell_id);
int      srslte_hip_nbiot_npss_re(uint32_t nof_prb, uint32_t prb_offset, uint32_t* re);
int      srslte_hip_nbiot_nsss_re(uint32_t nof_prb, uint32_t prb_offset, int nf, uint32_t* re, uint32_t* first);

#ifdef __cplusplus
}
#endif
#endif
