// Internal (non-ABI) declarations shared between the translation units of libsrslte_phy_hip.so.
#pragma once
#include "common.hpp"
#include "srslte_hip/phy_hip.h"
#include <functional>
#include <vector>

struct FftFactors {
  int N, nf;
  int radix[8];
  int inplace; // LDS->LDS passes fit one butterfly per thread: single LDS buffer
};

// Returns (creating on first use, per device) the factorisation and the device twiddle table exp(-j2*pi*k/N).
int fft_get_plan(int N, FftFactors* f, const cf32** d_tw);
size_t ofdm_sample_bytes(const srslte_hip_ofdm_t* q); // of one time-domain sample in the object's format (phy_hip.h, "Sample formats")


// Gold sequence c(n) of 36.211 7.2 (sequence.c:48-79), host side, for init-time tables.
void lte_gold_sequence(uint32_t c_init, uint32_t len, std::vector<uint8_t>& c);

// demod.hip: type 0 float / 1 int16 / 2 int8; optional packed scrambling bits [10][scr_words] selected by (tti0+call)%10
int demod_launch(int type, int mod, const void* d_sym, void* d_llr, int nsym, int ncalls, const uint32_t* d_scr, int scr_words, int tti0,
                 hipStream_t st);

// fec_tables.cpp: 36.212 tables shared by encoder, decoder and rate matching (host)
struct QppRow { uint16_t K, f1, f2; };
extern const QppRow lte_qpp_table[188];
int  lte_cb_index(uint32_t K);
void lte_qpp_tables(uint32_t K, uint32_t W, std::vector<uint16_t>& fwd, std::vector<uint16_t>& rev);
void lte_rm_rx_table(uint32_t K, uint32_t rv, std::vector<uint32_t>& d_index); // circular-buffer order -> 3*i+s
uint32_t lte_rm_tx_start(uint32_t K, uint32_t rv); // bit of the NULL-free circular buffer that lte_rm_rx_table(K, rv) begins with
// fec_tables.cpp: tables of the fixed-grant pipelines - the packed scrambling rows [10][words] of c_init(sf), nbits bits each; the TB CRC24A
// remainders x^(tbs+23-j) mod g [tbs + 24]; the same per code block in the W-window decoder's array order [C][K]
void lte_scr_table(const std::function<uint32_t(uint32_t)>& c_init, uint32_t nbits, uint32_t words, std::vector<uint32_t>& scr);
void lte_tbcrc_rem_table(uint32_t tbs, std::vector<uint32_t>& rem);
void lte_tbcrc_win_table(const std::vector<uint32_t>& rem, uint32_t C, uint32_t K, uint32_t W, std::vector<uint32_t>& t);
// fec_tables.cpp: one period of the coded bit types of a HARQ-ACK / rank indication of O bits on the PUSCH (encode_ri_ack / encode_ack_long,
// uci.c:573-623): 0 / 1 a value, 2 a repetition, 3 a placeholder; returns the period (Qm, 3 Qm or 32; 0 for O = 0 or above 10)
uint32_t lte_uci_ack_ri_types(const uint8_t* d, uint32_t O, uint32_t Qm, uint8_t types[32]);
// pdsch.hip: the checks of srslte_hip_ulsch_encode on the configuration and the caller's buffers alone, with its codes (no object, nothing queued)
int ulsch_enc_check(const srslte_hip_ulsch_enc_cfg_t* c, const uint8_t* data, uint8_t** buffer_b);
// pusch_uci_host.cpp (beside srslte_hip_pusch_uci_plan): Q'_cqi of a report of O bits behind Q'_ri symbols, the offset index being the caller's to
// check; (row, column) of ACK / RI symbol i in the channel interleaver's matrix of rows x nof_symb (uci.c:497-545)
uint32_t pusch_uci_cqi_qprime(const srslte_hip_pusch_uci_cfg_t* c, uint32_t O, uint32_t Qp_ri);
void     pusch_uci_symbol_pos(bool is_ri, uint32_t i, uint32_t rows, uint32_t nof_symb, uint32_t* row, uint32_t* col);

// chest.hip: srslte_chest_ul_estimate_pusch for a list of PUSCHs of one (L_prb, n_dmrs): item i = {subframe of the batch, PRB offset of slot 0 / 1,
// row of d_res}; d_items on the device
struct ChestUlItem { int sf, n_prb, n_prb1, row; };
int chest_ul_estimate_items(srslte_hip_chest_ul_t* q, uint32_t tti0, uint32_t L_prb, uint32_t n_dmrs, const ChestUlItem* d_items, int n_items,
                            const void* d_grid, void* d_ce, void* d_res, hipStream_t st);
int chest_ul_dmrs_table_cached(srslte_hip_chest_ul_t* q, uint32_t L_prb, uint32_t n_dmrs, const void** d_r); // one table per (L_prb, n_dmrs), all kept
// chest.hip: device DMRS table of a PUSCH grant, [10][2][12 * L_prb] cf32 (owned by q)
int chest_ul_dmrs_table(srslte_hip_chest_ul_t* q, uint32_t L_prb, uint32_t n_dmrs, const void** d_r);
// chest.hip: chest_common.c's stand-alone array helpers on device buffers (filter_len <= nof_ref, nof_ref >= 2 as the extrapolation reads in[0..1])
int chest_average_pilots_launch(const void* d_in, void* d_out, const float* d_filt, int nof_ref, int nof_symbols, int filter_len, hipStream_t st);
int chest_noise_pilots_launch(const void* d_noisy, const void* d_noiseless, void* d_noise_vec, int n, float* d_power, hipStream_t st);
// chest.hip: the noise estimates [port][antenna] the PSS / EMPTY algorithms keep between calls (q->noise_estimate of the reference)
int chest_dl_set_noise_state(srslte_hip_chest_dl_t* q, const float* noise);
// chest.hip: srslte_hip_chest_dl_estimate_batch_multi with the estimates kept as ONE row per (subframe, port, antenna) (ce_compact; only
// without interpolate_subframe, where every symbol of the subframe gets the same row)
int chest_dl_estimate_batch_rows(srslte_hip_chest_dl_t* q, const srslte_hip_chest_dl_cfg_t* cfg, uint32_t tti0, const void* d_grid, void* d_ce,
                                 void* d_res, int nof_sf, int nof_rx, int ce_compact, void* stream);
// chest.hip: the MBSFN estimate on grids of 2 nsl symbols per subframe with a result record (noise figure) per subframe, for the PMCH pipeline
int chest_dl_estimate_mbsfn_rows(srslte_hip_chest_dl_t* q, const srslte_hip_chest_dl_cfg_t* cfg, uint32_t tti0, const void* d_grid, void* d_ce,
                                 int nof_sf, int nof_rx, int nsl, void* d_res, void* stream);
// tdec.hip: what one run of the decoder does beyond its arguments. A run depends on its own options only: the object keeps none of them.
struct TdecOpts {
  // The windowed decoders also emit each block's share of the transport-block CRC syndrome into tb_syn[cb] (tdec_run_batch_w only).
  // tb_rem: [tb_C][K] words, x^(tbs+24-1-position in the TB) mod g for the block's payload bits in the decoder's array order, 0 elsewhere;
  // ignored by the unwindowed decoder. tb_C = 0 counts as 1
  const uint32_t* tb_rem = nullptr;
  uint32_t        tb_C   = 1;
  uint32_t*       tb_syn = nullptr;
  // Blocks with skip[cb] != 0 are left alone: bytes, CRC flag, TB-CRC share stay
  const uint8_t* skip = nullptr;
  // The run works on the block slots cb_map[0 .. nof_cb) instead of 0 .. nof_cb-1 (input, output, iteration count, CRC flag, skip flag). For
  // ragged batches, where the code blocks of one length are scattered over the batch's slots
  const uint32_t* cb_map = nullptr;
  // The run continues blocks whose passes 0..start_iter-1 the previous run on this object did (same inputs, same block slots):
  // srslte_tdec_iteration's one-more-pass without redoing the earlier ones (turbodecoder.c:539-545). tdec_run_batch_w only; a value of
  // nof_iterations or more counts as 0
  uint32_t start_iter = 0;
  // The decoder writes every block's payload bytes (tb_rb per block) straight into its transport block tb_out[cb / tb_C][...] and the last
  // block of a transport block to finish writes tb_ok_out[cb / tb_C] (all block CRCs, the XOR of the TB-CRC shares, a non-zero parity:
  // sch.c:470-488): no assembly kernel behind the decoder. tdec_run_batch_w: the 16-window 16-bit decoder or an 8-bit one, with tb_rem,
  // without skip, cb_map or start_iter, nof_cb a multiple of tb_C - anything else is refused
  uint8_t* tb_out        = nullptr;
  uint32_t tb_out_stride = 0, tb_rb = 0;
  uint8_t* tb_ok_out     = nullptr;
  // ... tdec_run_groups (a ragged batch of 16-bit blocks; tb_Cof is required there): transport-block slot v = block slot / tb_width has
  // tb_Cof[v] blocks and row v (v < tb_B) or tb_rows0 + v - tb_B of tb_out / tb_ok_out; tb_rb is not read
  const uint8_t* tb_Cof   = nullptr;
  uint32_t       tb_width = 0, tb_B = 0, tb_rows0 = 0;
  // Punctured parity at a quarter of its rows (pdsch_kernels.inc, rm_parity_compact): the input keeps row r of parity stream i only where
  // r % 4 == pc_phase[i], as row r / 4 of K / 4 elements at K + 32 + i K / 4 of the block; the rows it does not keep count as zeros, the
  // tails sit at K + 32 + K / 2. tdec_run_batch_w with the 16-window 16-bit decoder on an SB-layout input it reads in place (16-byte aligned
  // base and stride) and K % 64 == 0 - anything else is refused
  uint32_t pc = 0, pc_phase[2] = {0, 0};
};
// The largest block count of a transport block that TdecOpts::tb_Cof may hold: block r of C multiplies its CRC24A share by factor C-1-r of
// tdec_tbA_table (tdec.hip), which holds 16 factors. A grants call with a larger transport block has tb_crc_bytes_kernel assemble and judge them.
constexpr uint32_t TDEC_TB_MAX_C_DIRECT = 16;
// tdec.hip: a ragged batch in one call - groups of equal block length, in the order of the block map opts.cb_map - with ONE launch
// per decoder kernel the lengths need instead of one per length (back-ends chosen per length as on an AVX2 host; CRC per group for the early stop)
struct srslte_hip_tdec_group_t {
  uint32_t K, nof_cb, crc_poly, crc_nbits;
};
int tdec_run_groups(srslte_hip_tdec_t* q, const void* d_input, int llr8, uint32_t in_stride, const srslte_hip_tdec_group_t* groups, uint32_t nof_groups,
                    uint32_t nof_iterations, uint8_t* d_output, uint32_t out_stride, uint32_t* d_iters, uint8_t* d_crc_ok, hipStream_t st,
                    const TdecOpts& opts);
// tdec.hip: srslte_hip_tdec_run_batch with an optional forced back-end (force_w = -1 auto, 0 generic, 8, 16, 32 with llr8);
// llr8: d_input is int8 and the 8-bit numerics / fall-backs of turbodecoder.c:438-487 apply
int tdec_run_batch_w(srslte_hip_tdec_t* q, const void* d_input, int llr8, uint32_t in_stride, int sb_layout, uint32_t K, int force_w,
                     uint32_t nof_cb, uint32_t nof_iterations, uint32_t crc_poly, uint32_t crc_nbits, uint8_t* d_output,
                     uint32_t out_stride, uint32_t* d_iters, uint8_t* d_crc_ok, hipStream_t st, const TdecOpts& opts);
// pdcch_tx.hip: the checks of srslte_hip_dl_ctrl_tx_put alone (nothing is queued), and the cell an object was made for
int                                dl_ctrl_tx_check(srslte_hip_dl_ctrl_tx_t* q, uint32_t tti0, uint32_t nof_sf, const srslte_hip_dl_ctrl_tx_in_t* in);
const srslte_hip_dl_ctrl_tx_cfg_t* dl_ctrl_tx_cfg(const srslte_hip_dl_ctrl_tx_t* q);
int                                dl_ctrl_tx_tdd_sf_config(const srslte_hip_dl_ctrl_tx_t* q); // -1: an FDD object
bool                               dl_ctrl_tx_is_uplink(const srslte_hip_dl_ctrl_tx_t* q, uint32_t tti); // an uplink subframe of a TDD object
// pbch.hip: the broadcast tables of a cell on the device (PBCH REs, PSS / SSS, srslte_sequence_pbch; rx: the MIB decoder's buffers for
// c->max_batch subframes), owned by a srslte_hip_dl_ctrl_tx_t / srslte_hip_dl_ctrl_t; the broadcast put of a batch on the stream
struct BcastTables;
BcastTables* bcast_tables_create(const srslte_hip_dl_ctrl_cfg_t* c, int phich_ext, int phich_resources, bool rx);
void         bcast_tables_destroy(BcastTables* t);
int          bcast_tx_launch(const BcastTables* t, uint32_t tti0, uint32_t nof_sf, void* d_grid, hipStream_t st);
// pdcch_tx.hip / pdcch.hip: an object's broadcast tables
const BcastTables* dl_ctrl_tx_bcast(const srslte_hip_dl_ctrl_tx_t* q);
const BcastTables* dl_ctrl_bcast(const srslte_hip_dl_ctrl_t* q);
// pdcch.hip: the checks of srslte_hip_dl_ctrl_batch on the object, the batch size and the requests alone (nothing is queued), and what
// phich.hip reads of a srslte_hip_dl_ctrl_t: its cell, the PCFICH / PHICH sequences and the searched candidates on the device; and the PHICH
// receiver the object owns (phich.hip makes it in srslte_hip_dl_ctrl_set_max_phich and hands it over with dl_ctrl_set_phich, which does not free
// the one held before; srslte_hip_dl_ctrl_destroy frees it with phich_rx_destroy)
struct PhichRx;
struct DlCtrlView {
  const srslte_hip_dl_ctrl_cfg_t*  cfg;
  int                              tdd_sf_config; // -1: FDD
  const uint32_t*                  d_scr_pcfich;  // [10] words
  const srslte_hip_dl_ctrl_cand_t* d_cand;       // [max_batch][SRSLTE_HIP_DL_CTRL_MAX_CAND]
  const uint32_t*                  d_ncand;      // [max_batch]
};
int        dl_ctrl_check(const srslte_hip_dl_ctrl_t* q, uint32_t tti0, uint32_t nof_sf, const srslte_hip_dl_ctrl_req_t* reqs);
DlCtrlView dl_ctrl_view(srslte_hip_dl_ctrl_t* q);
PhichRx*   dl_ctrl_phich(const srslte_hip_dl_ctrl_t* q);
void       dl_ctrl_set_phich(srslte_hip_dl_ctrl_t* q, PhichRx* t);
void       phich_rx_destroy(PhichRx* t);
// pucch.hip: the checks of srslte_hip_ul_ctrl_pucch_batch alone (nothing is queued), and whether an object was made for a receiver's cell
int  ul_ctrl_check(const srslte_hip_ul_ctrl_t* q, uint32_t nof_sf, const srslte_hip_pucch_req_t* reqs, uint32_t nof);
bool ul_ctrl_same_cell(const srslte_hip_ul_ctrl_t* q, uint32_t nof_prb, uint32_t cell_id, int cp_ext);
// chest.hip: compute_r_uv_arg (refsignal_ul.c:285-293): the argument of the uplink base sequence r_uv of nof_prb PRB into arg [12 nof_prb] (host)
void ul_r_uv_arg(uint32_t nof_prb, uint32_t u, uint32_t v, float* arg);
// srs_host.cpp: the checks of srslte_hip_srs_tx_put / _rx_batch on the configuration and the list alone (nothing is queued); the first slot's
// sequence of every subframe of a frame, [10][M_sc], as srslte_refsignal_srs_put reads it from srslte_refsignal_srs_gen's output
bool srs_cfg_valid(const srslte_hip_srs_cfg_t* c);
int  srs_list_check(const srslte_hip_srs_cfg_t* c, uint32_t tti0, uint32_t nof_sf, const srslte_hip_srs_ue_t* list, uint32_t nof);
void srs_first_slot_table(const srslte_hip_srs_cfg_t* c, uint32_t M_sc, uint32_t n_srs, std::vector<cf32>& r);
// srs.hip: whether an object was made for a receiver's cell, and the configuration it was made with
bool                        srs_same_cell(const srslte_hip_srs_t* q, uint32_t nof_prb, uint32_t cell_id, int cp_ext);
const srslte_hip_srs_cfg_t* srs_cfg(const srslte_hip_srs_t* q);
// sync_host.cpp: the tables of an fft_size - the conjugated, scaled time-domain PSS replicas [3][N], their half-symbol transforms [3][2][62],
// the DFT twiddles exp(-j 2 pi k / N), the SSS tables s, z1 [31][31], c [3][2][31] and the N_id_1 table [30][30] -, the frequency of bin j of
// the 62 around DC, generate_m0m1, and the checks of a configuration alone
struct SyncTables {
  std::vector<cf32>    replica, half, tw;
  std::vector<float>   s, z1, c;
  std::vector<int32_t> nid1;
};
void sync_tables(uint32_t N, SyncTables& t);
int  sync_bin_freq(int j);
void sync_m0m1(uint32_t N_id_1, uint32_t* m0, uint32_t* m1);
bool sync_fft_size_valid(uint32_t N);
bool sync_cfg_valid(const srslte_hip_sync_cfg_t* c);
bool sync_tracks_cfg_valid(const srslte_hip_sync_tracks_cfg_t* c);
// sync_host.cpp: the 62 PSS values of srslte_pss_generate (pss.c:348-376) for N_id_2 = v
void sync_pss_seq(int v, cf32* pss);
// chest.hip: the CRS values r_l,ns(m) of a cell (refsignal_dl.c:66-116; 36.211 6.10.1.1): [10][4][2 nof_prb] for ports 0 and 1 (symbols 0 and
// N_symb - 3 of each slot), then [10][2][2 nof_prb] for ports 2 and 3 (symbol 1 of each slot) (host)
void lte_crs_values(uint32_t cell_id, uint32_t nof_prb, bool cp_is_norm, std::vector<cf32>& pil);
// fft.hip: the N-point row passes of the four-step transforms of 30 N points (meas.hip) on the plans of the OFDM sizes.
// Inverse rows with the spectral product on their loads and the inter-stage twiddle on their stores: for x in [n_x][nblk][30][N], h in
// [n_h][30][N] (both in [k1][k2] order), out[((ix n_h + ih) nblk + b)][k1][n2] = scale conj(tw2[n2 k1]) sum_k2 x[ix][b][k1][k2]
// conj(h[ih][k1][k2]) exp(+j 2 pi n2 k2 / N); tw2[i] = exp(-j 2 pi i / (30 N)). n_x n_h <= 65535, nblk <= 65535
int fft_rows30_mulconj_inverse(const cf32* d_x, const cf32* d_h, const cf32* d_tw2, cf32* d_out, int N, uint32_t nblk, uint32_t n_x, uint32_t n_h,
                               float scale, hipStream_t st);
// meas_host.cpp: the checks of a measurement configuration alone, its symbol size, the inter-stage twiddles exp(-j 2 pi i / (30 N)), i < 30 N,
// formed in double, and the SSS values of subframes 0 and 5 of a cell (srslte_sss_generate, gen_sss.c:121-155)
bool     meas_cfg_valid(const srslte_hip_meas_cfg_t* c);
uint32_t meas_symbol_sz(const srslte_hip_meas_cfg_t* c);
void     meas_twiddles(uint32_t N, std::vector<cf32>& tw2);
void     meas_sss_seq(uint32_t cell_id, float* s0, float* s5);
// nbiot_sync_host.cpp: the tables nbiot_sync.hip uploads, formed in double on the host - the NPSS taps of the two CP classes [2][138]
// (conjugated, 1 / 3 / sqrt(128)), the first 128 replica samples (the frame_size < 128 branch), the second half of the half-subcarrier table
// [823], the NSSS slide twiddles [2][12][138] and the conjugated NSSS values of theta_f = 0 [132][504] - and the check of a configuration
struct NbiotTables {
  std::vector<cf32> npss_taps, npss_head, shift2, nsss_tw, nsss_seq;
};
void nbiot_tables(NbiotTables& t);
bool nbiot_cfg_valid(const srslte_hip_nbiot_sync_cfg_t* c);
