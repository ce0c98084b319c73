/* oracle/dropin_resize_test.c - TEST INFRASTRUCTURE ONLY. A caller of the reference's PHY library that does what srsue does with its
 * objects: srslte_enb_dl / srslte_ue_dl / srslte_ue_ul / srslte_enb_ul are built ONCE at SRSLTE_MAX_PRB and then moved from cell to cell
 * with their *_set_cell calls, which resize every OFDM object (srslte_ofdm_rx_set_prb / _tx_set_prb), the estimator
 * (srslte_chest_dl_set_cell) and the rest - served by libsrslte_phy_hip.so where INTEGRATION.md §1 says so. Each cell has a new id, since
 * the set_cell calls only re-plan on a change of id. On each cell a few noise-free subframes go eNB -> UE (PCFICH + PDCCH + PDSCH: the DCI
 * must be found and the transport block's bytes must arrive) and UE -> eNB (one PUSCH per subframe, from the UE's transmitter with its +0.5
 * shift and normalisation to the eNB's receiver with its -0.5 shift). One line per cell; exit 0 only if everything passed.
 * This checks that the reference's callers work end to end over the resized objects; tests/test_gpu_compat_resize.py checks each object
 * numerically on its own. Built by ref_hip.mk, run by tests/test_gpu_dropin.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "srslte/srslte.h"

#define RNTI 0x4601
#define NOF_SF 3

typedef struct {
  uint32_t id, nof_prb, nof_ports;
  srslte_cp_t cp;
} cell_step_t;

static const cell_step_t STEPS[] = {{11, 6, 1, SRSLTE_CP_NORM},   {222, 15, 2, SRSLTE_CP_NORM}, {33, 25, 1, SRSLTE_CP_NORM},
                                    {444, 50, 2, SRSLTE_CP_NORM}, {55, 75, 1, SRSLTE_CP_NORM},  {366, 100, 2, SRSLTE_CP_NORM},
                                    {77, 25, 2, SRSLTE_CP_EXT},   {488, 50, 1, SRSLTE_CP_EXT}};

static uint32_t fill_random(uint8_t* p, uint32_t nbytes, uint32_t seed)
{
  for (uint32_t i = 0; i < nbytes; i++) {
    seed = seed * 1103515245u + 12345u;
    p[i] = (uint8_t)(seed >> 16);
  }
  return seed;
}

/* the largest PUSCH width that DFT precoding takes on about 80 % of the cell */
static uint32_t pusch_width(uint32_t nof_prb)
{
  uint32_t L = nof_prb * 4 / 5;
  while (L > 1 && !srslte_dft_precoding_valid_prb(L)) {
    L--;
  }
  return L;
}

static int dl_subframe(srslte_enb_dl_t* enb, srslte_ue_dl_t* ue, cf_t** enb_out, cf_t* ue_in, const srslte_cell_t* cell, uint32_t tti,
                       uint8_t* tx_data, uint8_t* rx_data, srslte_softbuffer_tx_t* sb_tx, srslte_softbuffer_rx_t* sb_rx, uint32_t* seed)
{
  const srslte_tm_t tm = cell->nof_ports == 1 ? SRSLTE_TM1 : SRSLTE_TM2;

  srslte_dl_sf_cfg_t sf;
  bzero(&sf, sizeof(sf));
  sf.tti = tti;
  sf.cfi = 2;

  /* eNB: a format-1 grant of every RBG for the UE at the first of its candidates */
  srslte_dci_dl_t dci;
  bzero(&dci, sizeof(dci));
  dci.rnti                    = RNTI;
  dci.format                  = SRSLTE_DCI_FORMAT1;
  dci.alloc_type              = SRSLTE_RA_ALLOC_TYPE0;
  const uint32_t P            = srslte_ra_type0_P(cell->nof_prb);
  const uint32_t nof_rbg      = (cell->nof_prb + P - 1) / P;
  dci.type0_alloc.rbg_bitmask = (1u << nof_rbg) - 1;
  dci.tb[0].mcs_idx           = 9 + tti % 4;
  dci.tb[0].rv                = 0;
  dci.tb[0].ndi               = tti % 2;
  dci.tb[0].cw_idx            = 0;
  dci.tb[1].mcs_idx           = 0;
  dci.tb[1].rv                = 1;
  srslte_dci_location_t loc[MAX_CANDIDATES_UE];
  if (srslte_pdcch_ue_locations(&enb->pdcch, &sf, loc, MAX_CANDIDATES_UE, RNTI) < 1) {
    printf("no PDCCH candidate\n");
    return -1;
  }
  dci.location = loc[0];

  srslte_pdsch_cfg_t tx_cfg;
  bzero(&tx_cfg, sizeof(tx_cfg));
  if (srslte_ra_dl_dci_to_grant((srslte_cell_t*)cell, &sf, tm, false, &dci, &tx_cfg.grant)) {
    printf("srslte_ra_dl_dci_to_grant failed\n");
    return -1;
  }
  tx_cfg.rnti              = RNTI;
  tx_cfg.softbuffers.tx[0] = sb_tx;
  const uint32_t tbs       = (uint32_t)tx_cfg.grant.tb[0].tbs;
  *seed                    = fill_random(tx_data, tbs / 8, *seed);
  srslte_softbuffer_tx_reset(sb_tx);

  srslte_dci_cfg_t dci_cfg;
  bzero(&dci_cfg, sizeof(dci_cfg));
  srslte_enb_dl_put_base(enb, &sf);
  uint8_t* data_tx[SRSLTE_MAX_CODEWORDS] = {tx_data, NULL};
  if (srslte_enb_dl_put_pdcch_dl(enb, &dci_cfg, &dci) || srslte_enb_dl_put_pdsch(enb, &tx_cfg, data_tx)) {
    printf("eNB put failed\n");
    return -1;
  }
  srslte_enb_dl_gen_signal(enb);

  /* one receive antenna, a flat channel of gain 1 from every port */
  const uint32_t sf_len = SRSLTE_SF_LEN_PRB(cell->nof_prb);
  memcpy(ue_in, enb_out[0], sizeof(cf_t) * sf_len);
  for (uint32_t p = 1; p < cell->nof_ports; p++) {
    srslte_vec_sum_ccc(ue_in, enb_out[p], ue_in, sf_len);
  }

  /* UE */
  srslte_ue_dl_cfg_t cfg;
  bzero(&cfg, sizeof(cfg));
  cfg.cfg.tm                = tm;
  cfg.chest_cfg.filter_type = SRSLTE_CHEST_FILTER_NONE;
  cfg.chest_cfg.noise_alg   = SRSLTE_NOISE_ALG_REFS;
  srslte_dl_sf_cfg_t rx_sf;
  bzero(&rx_sf, sizeof(rx_sf));
  rx_sf.tti = tti;
  if (srslte_ue_dl_decode_fft_estimate(ue, &rx_sf, &cfg) < 0) {
    printf("srslte_ue_dl_decode_fft_estimate failed\n");
    return -1;
  }
  if (rx_sf.cfi != sf.cfi) {
    printf("CFI %u decoded, %u sent\n", rx_sf.cfi, sf.cfi);
    return -1;
  }
  srslte_dci_dl_t found[SRSLTE_MAX_DCI_MSG];
  bzero(found, sizeof(found));
  int n = srslte_ue_dl_find_dl_dci(ue, &rx_sf, &cfg, RNTI, found);
  if (n != 1 || found[0].location.ncce != dci.location.ncce || found[0].tb[0].mcs_idx != dci.tb[0].mcs_idx) {
    printf("DCI not found (%d found)\n", n);
    return -1;
  }
  if (srslte_ue_dl_dci_to_pdsch_grant(ue, &rx_sf, &cfg, &found[0], &cfg.cfg.pdsch.grant)) {
    printf("srslte_ue_dl_dci_to_pdsch_grant failed\n");
    return -1;
  }
  if (cfg.cfg.pdsch.grant.tb[0].tbs != (int)tbs) {
    printf("TBS %d decoded, %u sent\n", cfg.cfg.pdsch.grant.tb[0].tbs, tbs);
    return -1;
  }
  srslte_pdsch_cfg_t rx_cfg = cfg.cfg.pdsch;
  rx_cfg.rnti               = RNTI;
  rx_cfg.max_nof_iterations = 8;
  rx_cfg.softbuffers.rx[0]  = sb_rx;
  srslte_softbuffer_rx_reset(sb_rx);
  srslte_pdsch_res_t res[SRSLTE_MAX_CODEWORDS];
  bzero(res, sizeof(res));
  res[0].payload = rx_data;
  bzero(rx_data, tbs / 8);
  if (srslte_ue_dl_decode_pdsch(ue, &rx_sf, &rx_cfg, res) || !res[0].crc || memcmp(rx_data, tx_data, tbs / 8)) {
    printf("PDSCH of %u bits not received (crc %d)\n", tbs, res[0].crc);
    return -1;
  }
  return (int)tbs;
}

static int ul_subframe(srslte_ue_ul_t* ue, srslte_enb_ul_t* enb, cf_t* ue_out, cf_t* enb_in, const srslte_cell_t* cell, uint32_t tti,
                       uint8_t* tx_data, uint8_t* rx_data, srslte_softbuffer_tx_t* sb_tx, srslte_softbuffer_rx_t* sb_rx, uint32_t* seed)
{
  srslte_ul_sf_cfg_t sf;
  bzero(&sf, sizeof(sf));
  sf.tti = tti;

  const uint32_t L = pusch_width(cell->nof_prb);
  srslte_dci_ul_t dci;
  bzero(&dci, sizeof(dci));
  dci.rnti             = RNTI;
  dci.format           = SRSLTE_DCI_FORMAT0;
  dci.type2_alloc.riv  = srslte_ra_type2_to_riv(L, (cell->nof_prb - L) / 2, cell->nof_prb);
  dci.freq_hop_fl      = SRSLTE_RA_PUSCH_HOP_DISABLED;
  dci.tb.mcs_idx       = 6 + tti % 5;
  dci.tb.rv            = 0;
  dci.tb.ndi           = tti % 2;

  srslte_ue_ul_cfg_t cfg;
  bzero(&cfg, sizeof(cfg));
  cfg.grant_available = true;
  if (srslte_ue_ul_dci_to_pusch_grant(ue, &sf, &cfg, &dci, &cfg.ul_cfg.pusch.grant)) {
    printf("srslte_ue_ul_dci_to_pusch_grant failed\n");
    return -1;
  }
  cfg.ul_cfg.pusch.rnti           = RNTI;
  cfg.ul_cfg.pusch.softbuffers.tx = sb_tx;
  const uint32_t tbs              = (uint32_t)cfg.ul_cfg.pusch.grant.tb.tbs;
  *seed                           = fill_random(tx_data, tbs / 8, *seed);
  srslte_softbuffer_tx_reset(sb_tx);
  srslte_pusch_data_t data;
  bzero(&data, sizeof(data));
  data.ptr = tx_data;
  if (srslte_ue_ul_encode(ue, &sf, &cfg, &data) != 1) {
    printf("srslte_ue_ul_encode failed\n");
    return -1;
  }

  memcpy(enb_in, ue_out, sizeof(cf_t) * SRSLTE_SF_LEN_PRB(cell->nof_prb));
  srslte_enb_ul_fft(enb);
  srslte_pusch_cfg_t rx_cfg = cfg.ul_cfg.pusch;
  rx_cfg.softbuffers.rx     = sb_rx;
  rx_cfg.max_nof_iterations = 8;
  srslte_softbuffer_rx_reset(sb_rx);
  srslte_pusch_res_t res;
  bzero(&res, sizeof(res));
  res.data = rx_data;
  bzero(rx_data, tbs / 8);
  if (srslte_enb_ul_get_pusch(enb, &sf, &rx_cfg, &res) || !res.crc || memcmp(rx_data, tx_data, tbs / 8)) {
    printf("PUSCH of %u bits on %u PRB not received (crc %d)\n", tbs, L, res.crc);
    return -1;
  }
  return (int)tbs;
}

int main(void)
{
  const uint32_t max_sf = SRSLTE_SF_LEN_PRB(SRSLTE_MAX_PRB);
  cf_t *         enb_dl_out[SRSLTE_MAX_PORTS] = {NULL}, *ue_dl_in[SRSLTE_MAX_PORTS] = {NULL};
  for (int p = 0; p < SRSLTE_MAX_PORTS; p++) {
    enb_dl_out[p] = srslte_vec_malloc(sizeof(cf_t) * max_sf);
  }
  ue_dl_in[0]       = srslte_vec_malloc(sizeof(cf_t) * max_sf);
  cf_t*    ul_sig   = srslte_vec_malloc(sizeof(cf_t) * max_sf);
  cf_t*    enb_in   = srslte_vec_malloc(sizeof(cf_t) * max_sf);
  uint8_t* tx_data  = srslte_vec_malloc(150000);
  uint8_t* rx_data  = srslte_vec_malloc(150000);

  srslte_enb_dl_t enb_dl;
  srslte_ue_dl_t  ue_dl;
  srslte_ue_ul_t  ue_ul;
  srslte_enb_ul_t enb_ul;
  if (srslte_enb_dl_init(&enb_dl, enb_dl_out, SRSLTE_MAX_PRB) || srslte_ue_dl_init(&ue_dl, ue_dl_in, SRSLTE_MAX_PRB, 1) ||
      srslte_ue_ul_init(&ue_ul, ul_sig, SRSLTE_MAX_PRB) || srslte_enb_ul_init(&enb_ul, enb_in, SRSLTE_MAX_PRB)) {
    printf("init at %d PRB failed\n", SRSLTE_MAX_PRB);
    return 1;
  }
  srslte_softbuffer_tx_t dl_sb_tx, ul_sb_tx;
  srslte_softbuffer_rx_t dl_sb_rx, ul_sb_rx;
  if (srslte_softbuffer_tx_init(&dl_sb_tx, SRSLTE_MAX_PRB) || srslte_softbuffer_rx_init(&dl_sb_rx, SRSLTE_MAX_PRB) ||
      srslte_softbuffer_tx_init(&ul_sb_tx, SRSLTE_MAX_PRB) || srslte_softbuffer_rx_init(&ul_sb_rx, SRSLTE_MAX_PRB)) {
    printf("softbuffer init failed\n");
    return 1;
  }

  uint32_t seed = 1;
  int      failed = 0;
  for (uint32_t s = 0; s < sizeof(STEPS) / sizeof(STEPS[0]); s++) {
    srslte_cell_t cell;
    bzero(&cell, sizeof(cell));
    cell.id              = STEPS[s].id;
    cell.nof_prb         = STEPS[s].nof_prb;
    cell.nof_ports       = STEPS[s].nof_ports;
    cell.cp              = STEPS[s].cp;
    cell.phich_length    = SRSLTE_PHICH_NORM;
    cell.phich_resources = SRSLTE_PHICH_R_1;
    cell.frame_type      = SRSLTE_FDD;
    srslte_refsignal_dmrs_pusch_cfg_t dmrs;
    bzero(&dmrs, sizeof(dmrs));
    if (srslte_enb_dl_set_cell(&enb_dl, cell) || srslte_ue_dl_set_cell(&ue_dl, cell) || srslte_ue_ul_set_cell(&ue_ul, cell) ||
        srslte_enb_ul_set_cell(&enb_ul, cell, &dmrs)) {
      printf("cell %u: set_cell failed\n", cell.id);
      failed++;
      break;
    }
    srslte_enb_dl_add_rnti(&enb_dl, RNTI);
    srslte_ue_dl_set_rnti(&ue_dl, RNTI);
    srslte_ue_ul_set_rnti(&ue_ul, RNTI);
    srslte_enb_ul_add_rnti(&enb_ul, RNTI);
    int dl_bits = 0, ul_bits = 0, ok = 1;
    for (uint32_t i = 0; i < NOF_SF && ok; i++) {
      const uint32_t tti = 10 * s + 1 + i;
      int            d   = dl_subframe(&enb_dl, &ue_dl, enb_dl_out, ue_dl_in[0], &cell, tti, tx_data, rx_data, &dl_sb_tx, &dl_sb_rx, &seed);
      int            u   = d < 0 ? -1 : ul_subframe(&ue_ul, &enb_ul, ul_sig, enb_in, &cell, tti, tx_data, rx_data, &ul_sb_tx, &ul_sb_rx, &seed);
      ok                 = d > 0 && u > 0;
      dl_bits += d > 0 ? d : 0;
      ul_bits += u > 0 ? u : 0;
    }
    printf("cell id=%u prb=%u ports=%u cp=%s: %s (%d DL, %d UL transport-block bits)\n", cell.id, cell.nof_prb, cell.nof_ports,
           cell.cp == SRSLTE_CP_NORM ? "norm" : "ext", ok ? "ok" : "FAILED", dl_bits, ul_bits);
    failed += !ok;
    srslte_enb_dl_rem_rnti(&enb_dl, RNTI);
    srslte_enb_ul_rem_rnti(&enb_ul, RNTI);
  }

  srslte_softbuffer_tx_free(&dl_sb_tx);
  srslte_softbuffer_tx_free(&ul_sb_tx);
  srslte_softbuffer_rx_free(&dl_sb_rx);
  srslte_softbuffer_rx_free(&ul_sb_rx);
  srslte_enb_dl_free(&enb_dl);
  srslte_ue_dl_free(&ue_dl);
  srslte_ue_ul_free(&ue_ul);
  srslte_enb_ul_free(&enb_ul);
  for (int p = 0; p < SRSLTE_MAX_PORTS; p++) {
    free(enb_dl_out[p]);
  }
  free(ue_dl_in[0]);
  free(ul_sig);
  free(enb_in);
  free(tx_data);
  free(rx_data);
  printf("%s\n", failed ? "FAILED" : "all cells passed");
  return failed ? 1 : 0;
}
