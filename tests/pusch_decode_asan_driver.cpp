// TEST INFRASTRUCTURE: the host function behind srslte_pusch_decode (compat.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU,
// in a program of its own: every path of it that ends before a device is needed - NULL arguments, each refusal of srslte_compat_pusch.h that is
// arithmetic on the configuration, and the allocation's refusals of srslte_hip_pusch_rows (phy_hip.h), which the host function asks for before it
// makes an object. The structs are heap blocks of exactly their size, so a read or write past one shows as a heap overflow; cfg, out, the
// transport block's bytes, the soft buffer and the grids carry patterns that must survive every refused call, and the counter of served calls
// must not move. The served path needs a device and is not run here: GPU runs take no sanitizer.
// Built and run by tests/test_pusch_decode_sanitizer.py from compat.cpp and fec_tables.cpp (both instrumented) and the library.
#include "srslte_hip/phy_hip.h"
#include "srslte_hip/srslte_compat_pusch.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

template <typename T> static T* exact(int fill = 0)
{
  T* p = (T*)malloc(sizeof(T));
  if (!p) exit(3);
  memset(p, fill, sizeof(T));
  return p;
}

int main()
{
  srslte_pusch_t*         q   = exact<srslte_pusch_t>();
  srslte_pusch_cfg_t*     cfg = exact<srslte_pusch_cfg_t>();
  srslte_ul_sf_cfg_t*     sf  = exact<srslte_ul_sf_cfg_t>();
  srslte_chest_ul_res_t*  ch  = exact<srslte_chest_ul_res_t>();
  srslte_pusch_res_t*     out = exact<srslte_pusch_res_t>(0x5A);
  srslte_softbuffer_rx_t* sb  = exact<srslte_softbuffer_rx_t>();
  // a 15-PRB cell, L_prb 9 at PRB 3, 16QAM, tbs 1544: one block of K = 1568
  const uint32_t P = 15, L = 9, nsymb = 12, nof_re = 12 * L * nsymb, tbs = 1544, grid_len = 14 * 12 * P, W = 3 * (1568 + 32) + 12;
  cf_t *         grid = (cf_t*)malloc(sizeof(cf_t) * grid_len), *ce = (cf_t*)malloc(sizeof(cf_t) * grid_len);
  uint8_t*       data = (uint8_t*)malloc(tbs / 8 + 3);
  int16_t**      buffer_f = (int16_t**)malloc(sizeof(int16_t*));
  uint8_t**      sb_data  = (uint8_t**)malloc(sizeof(uint8_t*));
  bool*          cb_crc   = (bool*)malloc(sizeof(bool));
  if (!grid || !ce || !data || !buffer_f || !sb_data || !cb_crc) return 3;
  buffer_f[0] = (int16_t*)malloc(2 * W);
  sb_data[0]  = (uint8_t*)malloc(1568 / 8);
  if (!buffer_f[0] || !sb_data[0]) return 3;
  memset(grid, 0x21, sizeof(cf_t) * grid_len);
  memset(ce, 0x22, sizeof(cf_t) * grid_len);
  memset(data, 0xC3, tbs / 8 + 3);
  memset(buffer_f[0], 0x11, 2 * W);
  memset(sb_data[0], 0x12, 1568 / 8);
  cb_crc[0]  = false;
  sb->max_cb = 1; sb->buffer_f = buffer_f; sb->data = sb_data; sb->cb_crc = cb_crc;
  q->cell.nof_prb = P; q->cell.nof_ports = 1; q->cell.id = 1; q->cell.cp = SRSLTE_CP_NORM;
  q->ul_sch.max_iterations = 6;
  int fake_decoder;                              // never dereferenced: every call below ends before the object behind it is looked at
  q->ul_sch.decoder.dec16_hdlr[0] = &fake_decoder;
  sf->tti = 13;
  ch->ce = ce; ch->nof_re = grid_len; ch->noise_estimate = 0.01f; ch->snr_db = 20.f;
  out->data = data;
  srslte_pusch_grant_t* g = &cfg->grant;
  g->L_prb = L; g->nof_symb = nsymb; g->nof_re = nof_re; g->n_prb_tilde[0] = g->n_prb_tilde[1] = 3;
  srslte_ra_tb_t* tb = &g->tb;
  tb->mod = SRSLTE_MOD_16QAM; tb->tbs = (int)tbs; tb->rv = 0; tb->nof_bits = nof_re * 4; tb->enabled = true;
  cfg->rnti = 0x1234; cfg->enable_64qam = true; cfg->softbuffers.rx = sb;
  cfg->uci_cfg.ack[0].nof_acks = 1;
  cfg->uci_offset.I_offset_ack = 9; cfg->uci_offset.I_offset_ri = 6; cfg->uci_offset.I_offset_cqi = 6;
  srslte_pusch_cfg_t*  cfg0 = exact<srslte_pusch_cfg_t>();
  srslte_pusch_res_t*  out0 = exact<srslte_pusch_res_t>();
  unsigned long long   before[2], after[2];
  srslte_hip_compat_stats_pusch(before);
  int  bad = 0, n = 0;
  auto want = [&](int got, int expected) {
    n++;
    if (got != expected) {
      fprintf(stderr, "check %d: %d, expected %d\n", n, got, expected);
      bad++;
    }
  };
  // one refused call: SRSLTE_ERROR_INVALID_INPUTS, and cfg and out as they went in
  auto refused = [&]() {
    memcpy(cfg0, cfg, sizeof(*cfg));
    memcpy(out0, out, sizeof(*out));
    want(srslte_pusch_decode(q, sf, cfg, ch, grid, out), SRSLTE_ERROR_INVALID_INPUTS);
    want(memcmp(cfg0, cfg, sizeof(*cfg)) || memcmp(out0, out, sizeof(*out)), 0);
  };
  // NULL arguments: upstream's four, then the two it would dereference
  want(srslte_pusch_decode(nullptr, sf, cfg, ch, grid, out), SRSLTE_ERROR_INVALID_INPUTS);
  want(srslte_pusch_decode(q, sf, nullptr, ch, grid, out), SRSLTE_ERROR_INVALID_INPUTS);
  want(srslte_pusch_decode(q, sf, cfg, ch, nullptr, out), SRSLTE_ERROR_INVALID_INPUTS);
  want(srslte_pusch_decode(q, sf, cfg, ch, grid, nullptr), SRSLTE_ERROR_INVALID_INPUTS);
  want(srslte_pusch_decode(q, nullptr, cfg, ch, grid, out), SRSLTE_ERROR_INVALID_INPUTS);
  want(srslte_pusch_decode(q, sf, cfg, nullptr, grid, out), SRSLTE_ERROR_INVALID_INPUTS);
  ch->ce = nullptr; refused(); ch->ce = ce;
  // the object and the transport block
  q->llr_is_8bit = true; refused(); q->llr_is_8bit = false;
  q->ul_sch.llr_is_8bit = true; refused(); q->ul_sch.llr_is_8bit = false;
  tb->mod = SRSLTE_MOD_BPSK; refused();
  tb->mod = SRSLTE_MOD_256QAM; refused();
  tb->mod = SRSLTE_MOD_64QAM; tb->nof_bits = nof_re * 6; cfg->enable_64qam = false; // limited to 16QAM locally (pusch.c:445-450) ...
  g->nof_re -= 12; refused(); g->nof_re = nof_re;                                   // ... and refused for its allocation: the grant stays 64QAM
  want((int)tb->mod, (int)SRSLTE_MOD_64QAM);
  cfg->enable_64qam = true; tb->mod = SRSLTE_MOD_16QAM; tb->nof_bits = nof_re * 4;
  tb->tbs = 6208; refused();   // filler bits / two block sizes
  tb->tbs = 1000000; refused(); // no segmentation
  tb->tbs = (int)tbs;
  tb->nof_bits -= 4; refused(); tb->nof_bits = nof_re * 4;
  g->nof_symb = 8; refused(); g->nof_symb = nsymb;
  out->data = nullptr; refused(); out->data = data;
  cfg->softbuffers.rx = nullptr; refused(); cfg->softbuffers.rx = sb;
  sb->max_cb = 0; refused(); sb->max_cb = 1;
  // the control information
  cfg->uci_cfg.cqi.ri_len = 3; refused(); cfg->uci_cfg.cqi.ri_len = 0;
  cfg->uci_offset.I_offset_ack = 16; refused(); cfg->uci_offset.I_offset_ack = 9;
  cfg->uci_cfg.cqi.data_enable = true; cfg->uci_cfg.cqi.type = SRSLTE_CQI_TYPE_SUBBAND_HL; cfg->uci_cfg.cqi.N = 31; // a report of 66 bits
  refused();
  cfg->uci_cfg.cqi.data_enable = false; cfg->uci_cfg.cqi.type = SRSLTE_CQI_TYPE_WIDEBAND; cfg->uci_cfg.cqi.N = 0;
  tb->tbs = 0; refused(); tb->tbs = (int)tbs; // neither data nor a report
  q->ul_sch.decoder.dec16_hdlr[0] = nullptr; refused(); q->ul_sch.decoder.dec16_hdlr[0] = &fake_decoder;
  // the allocation (srslte_hip_pusch_rows)
  g->L_prb = 7; refused(); g->L_prb = L;
  g->n_prb_tilde[0] = 7; refused(); g->n_prb_tilde[0] = 3;
  g->n_prb_tilde[1] = 7; refused(); g->n_prb_tilde[1] = 3;
  g->nof_re = nof_re + 12; refused(); g->nof_re = nof_re;
  sf->shortened = true; refused(); sf->shortened = false;        // 11 symbols are a shortened subframe's
  q->cell.cp = SRSLTE_CP_EXT; refused(); q->cell.cp = SRSLTE_CP_NORM; // and 10 an extended CP's
  q->cell.nof_prb = 11; refused(); q->cell.nof_prb = P;
  // the rows of a good allocation, and of its refusals, without a device
  srslte_hip_pusch_cfg_t* pc = exact<srslte_hip_pusch_cfg_t>();
  uint32_t*               rows = (uint32_t*)malloc(sizeof(uint32_t) * 2 * 12);
  if (!rows) return 3;
  pc->sch.mod = 2; pc->sch.L_prb = L; pc->sch.nof_symb = 11; pc->sch.nof_bits = 12 * L * 11 * 4; pc->nof_re = 12 * L * 11;
  pc->nof_prb = P; pc->n_prb_tilde[0] = 0; pc->n_prb_tilde[1] = 6; pc->shortened = 1;
  want(srslte_hip_pusch_rows(pc, rows), 11);
  want((int)rows[0] == 0 && rows[1] == 0 && rows[2 * 10] == 12 && rows[2 * 10 + 1] == 72, 1);
  pc->cp_ext = 1;
  want(srslte_hip_pusch_rows(pc, rows), SRSLTE_ERROR_INVALID_INPUTS);
  pc->sch.nof_symb = 9; pc->sch.nof_bits = 12 * L * 9 * 4; pc->nof_re = 12 * L * 9;
  want(srslte_hip_pusch_rows(pc, rows), 9);
  want(srslte_hip_pusch_decode(nullptr, grid, ce, 0.f, pc, nullptr, nullptr, nullptr, nullptr, nullptr), SRSLTE_ERROR_INVALID_INPUTS);
  // nothing was written, nothing was served
  for (uint32_t i = 0; i < sizeof(cf_t) * grid_len; i++) bad += ((uint8_t*)grid)[i] != 0x21 || ((uint8_t*)ce)[i] != 0x22;
  for (uint32_t i = 0; i < tbs / 8 + 3; i++) bad += data[i] != 0xC3;
  for (uint32_t i = 0; i < 2 * W; i++) bad += ((uint8_t*)buffer_f[0])[i] != 0x11;
  for (uint32_t i = 0; i < 1568 / 8; i++) bad += sb_data[0][i] != 0x12;
  bad += cb_crc[0] || sb->tb_crc;
  srslte_hip_compat_stats_pusch(after);
  bad += before[0] != after[0] || before[1] != after[1];
  free(rows); free(pc); free(cfg0); free(out0); free(buffer_f[0]); free(sb_data[0]); free(buffer_f); free(sb_data); free(cb_crc); free(data); free(grid);
  free(ce); free(q); free(cfg); free(sf); free(ch); free(out); free(sb);
  if (bad) {
    fprintf(stderr, "%d failures\n", bad);
    return 1;
  }
  printf("pusch decode host sanitizer run ok: %d checks\n", n);
  return 0;
}
