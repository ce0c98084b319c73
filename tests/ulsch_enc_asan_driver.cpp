// TEST INFRASTRUCTURE: the host function behind srslte_ulsch_encode (compat.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer on the
// CPU, in a program of its own: every path of it and of the device call srslte_hip_ulsch_encode that ends before a device is needed - NULL
// arguments, a report that does not pack, each refusal of srslte_compat.h and each refusal of phy_hip.h, which the host function asks for
// before it makes an object. The structs are heap blocks of exactly their size, so a read or write past one shows as a heap overflow; q_bits,
// g_bits, data, the circular buffers and the (position, type) list carry a pattern that must survive every refused call, cfg->K_segm must be
// written, and the counter of served calls must not move. The served path needs a device and is not run here: GPU runs take no sanitizer.
// Built and run by tests/test_ulsch_encode_sanitizer.py from compat.cpp and fec_tables.cpp (both instrumented) and the library.
#include "srslte_hip/phy_hip.h"
#include "srslte_hip/srslte_compat.h"
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
  srslte_sch_t*           q   = exact<srslte_sch_t>(0x77);
  srslte_pusch_cfg_t*     cfg = exact<srslte_pusch_cfg_t>();
  srslte_softbuffer_tx_t* sb  = exact<srslte_softbuffer_tx_t>();
  srslte_uci_value_t*     uci = exact<srslte_uci_value_t>();
  const uint32_t          nof_bits = 6 * 12 * 12 * 2, tbs = 6200, WB = (3 * 3136 + 12 + 7) / 8; // 6 PRB, QPSK; tbs 6200: C = 2, K = 3136
  uint8_t *               q_bits = (uint8_t*)malloc(nof_bits / 8), *g_bits = (uint8_t*)malloc(nof_bits / 8), *data = (uint8_t*)malloc(tbs / 8);
  uint8_t**               buffer_b = (uint8_t**)malloc(2 * sizeof(uint8_t*));
  if (!q_bits || !g_bits || !data || !buffer_b) return 3;
  memset(q_bits, 0xA5, nof_bits / 8);
  memset(g_bits, 0x3C, nof_bits / 8);
  memset(data, 0xC3, tbs / 8);
  for (int c = 0; c < 2; c++) {
    buffer_b[c] = (uint8_t*)malloc(WB);
    if (!buffer_b[c]) return 3;
    memset(buffer_b[c], 0x11, WB);
  }
  sb->max_cb = 2; sb->buffer_b = buffer_b;
  cfg->grant.L_prb = 6; cfg->grant.nof_symb = 12;
  srslte_ra_tb_t* tb = &cfg->grant.tb;
  tb->mod = SRSLTE_MOD_QPSK; tb->tbs = (int)tbs; tb->rv = 0; tb->nof_bits = nof_bits; tb->enabled = true;
  cfg->softbuffers.tx = sb;
  cfg->uci_cfg.ack[0].nof_acks = 1;
  uci->ack.ack_value[0] = 1;
  cfg->uci_offset.I_offset_ack = 9; cfg->uci_offset.I_offset_ri = 6; cfg->uci_offset.I_offset_cqi = 6;
  unsigned long long before[2], after[2];
  srslte_hip_compat_stats_ul_tx(before);
  int  bad = 0, n = 0;
  auto want = [&](int got, int expected) {
    n++;
    if (got != expected) {
      fprintf(stderr, "check %d: %d, expected %d\n", n, got, expected);
      bad++;
    }
  };
  auto call = [&]() { return srslte_ulsch_encode(q, cfg, data, uci, g_bits, q_bits); };
  // NULL arguments
  want(srslte_ulsch_encode(nullptr, cfg, data, uci, g_bits, q_bits), SRSLTE_ERROR_INVALID_INPUTS);
  want(srslte_ulsch_encode(q, nullptr, data, uci, g_bits, q_bits), SRSLTE_ERROR_INVALID_INPUTS);
  want(srslte_ulsch_encode(q, cfg, data, nullptr, g_bits, q_bits), SRSLTE_ERROR_INVALID_INPUTS);
  want(srslte_ulsch_encode(q, cfg, data, uci, g_bits, nullptr), SRSLTE_ERROR_INVALID_INPUTS);
  tb->mod = (srslte_mod_t)7; // a modulation of no bits (sch.c:1085-1087)
  want(call(), SRSLTE_ERROR_INVALID_INPUTS);
  tb->mod = SRSLTE_MOD_QPSK;
  want((int)cfg->K_segm, 0); // nothing has got as far as the segmentation
  want(srslte_ulsch_encode(q, cfg, nullptr, uci, g_bits, q_bits), SRSLTE_ERROR_INVALID_INPUTS); // rv 0 without a payload
  want((int)cfg->K_segm, 2 * 3136);                                                             // sch.c:1096, written before the refusal
  // upstream's own codes
  cfg->uci_cfg.cqi.data_enable = true; // a report that does not pack: 16 subbands
  cfg->uci_cfg.cqi.type = SRSLTE_CQI_TYPE_SUBBAND_HL; cfg->uci_cfg.cqi.N = 16;
  want(call(), SRSLTE_ERROR);
  cfg->uci_cfg.cqi.data_enable = false; cfg->uci_cfg.cqi.type = SRSLTE_CQI_TYPE_WIDEBAND; cfg->uci_cfg.cqi.N = 0;
  cfg->softbuffers.tx = nullptr;
  want(call(), SRSLTE_ERROR_INVALID_INPUTS);
  cfg->softbuffers.tx = sb;
  tb->tbs = 4016; // filler bits
  cfg->K_segm = 0;
  want(call(), SRSLTE_ERROR);
  want((int)cfg->K_segm >= 4016 + 24 ? 1 : 0, 1);
  tb->tbs = (int)tbs;
  sb->max_cb = 1; // two blocks out of a soft buffer of one
  want(call(), -1);
  sb->max_cb = 2;
  cfg->uci_offset.I_offset_ack = 15; // the reserved entry of Table 8.6.3-1
  want(call(), -1);
  cfg->uci_offset.I_offset_ack = 9;
  cfg->uci_cfg.cqi.data_enable = true; // a 4-bit report at the reserved entry of Table 8.6.3-3
  cfg->uci_offset.I_offset_cqi = 1;
  want(call(), -1);
  cfg->uci_cfg.cqi.data_enable = false;
  cfg->uci_offset.I_offset_cqi = 6;
  // the refusals of srslte_compat.h
  cfg->uci_cfg.ack[0].N_bundle = 3;
  want(call(), SRSLTE_ERROR_INVALID_INPUTS);
  cfg->uci_cfg.ack[0].N_bundle = 0;
  tb->mod = SRSLTE_MOD_BPSK;
  want(call(), SRSLTE_ERROR_INVALID_INPUTS);
  tb->mod = SRSLTE_MOD_256QAM;
  want(call(), SRSLTE_ERROR_INVALID_INPUTS);
  tb->mod = SRSLTE_MOD_QPSK;
  cfg->uci_cfg.ack[1].nof_acks = 10; // 11 ACK bits over the carriers
  want(call(), SRSLTE_ERROR_INVALID_INPUTS);
  cfg->uci_cfg.ack[1].nof_acks = 0;
  sb->buffer_b = nullptr;
  want(call(), SRSLTE_ERROR_INVALID_INPUTS);
  sb->buffer_b = buffer_b;
  // the refusals of the device call, asked before an object is made
  uint8_t* second = buffer_b[1];
  buffer_b[1] = nullptr;
  want(call(), SRSLTE_ERROR_INVALID_INPUTS);
  buffer_b[1] = second;
  tb->tbs = 6264; // C = 2 with two block sizes and no filler bits: K_segm is their sum
  want(call(), SRSLTE_ERROR_INVALID_INPUTS);
  want((int)cfg->K_segm, 3200 + 3136);
  tb->tbs = (int)tbs;
  tb->rv = 4;
  want(call(), SRSLTE_ERROR_INVALID_INPUTS);
  tb->rv = 0;
  tb->nof_bits = nof_bits - 8; // not 12 L_prb nof_symb Qm
  want(call(), SRSLTE_ERROR_INVALID_INPUTS);
  tb->nof_bits = 0;
  want(call(), SRSLTE_ERROR_INVALID_INPUTS);
  tb->nof_bits = nof_bits;
  cfg->grant.nof_symb = 8;
  want(call(), SRSLTE_ERROR_INVALID_INPUTS);
  cfg->grant.nof_symb = 12;
  cfg->grant.L_prb = 0;
  want(call(), SRSLTE_ERROR_INVALID_INPUTS);
  cfg->grant.L_prb = 6;
  cfg->uci_cfg.cqi.ri_len = 3;
  want(call(), SRSLTE_ERROR_INVALID_INPUTS);
  cfg->uci_cfg.cqi.ri_len = 0;
  cfg->uci_offset.I_offset_ack = 16;
  want(call(), SRSLTE_ERROR_INVALID_INPUTS);
  cfg->uci_offset.I_offset_ack = 9;
  cfg->uci_offset.I_offset_ri = 16;
  want(call(), SRSLTE_ERROR_INVALID_INPUTS);
  cfg->uci_offset.I_offset_ri = 6;
  cfg->uci_offset.I_offset_cqi = 16;
  want(call(), SRSLTE_ERROR_INVALID_INPUTS);
  cfg->uci_offset.I_offset_cqi = 6;
  tb->tbs = 0; // a PUSCH without data and without a report
  want(call(), SRSLTE_ERROR_INVALID_INPUTS);
  want((int)cfg->K_segm, 0);
  // 1 PRB, tbs 16 (K = 40) with a 20-bit report at beta 6.25: Q'_cqi = min(ceil(28 x 144 x 6.25 / 40), 144) leaves the block no symbol
  cfg->grant.L_prb = 1; tb->tbs = 16; tb->nof_bits = 12 * 12 * 2;
  cfg->uci_cfg.cqi.data_enable = true; cfg->uci_cfg.cqi.type = SRSLTE_CQI_TYPE_SUBBAND_HL; cfg->uci_cfg.cqi.N = 8;
  cfg->uci_offset.I_offset_cqi = 15;
  want(call(), SRSLTE_ERROR_INVALID_INPUTS);
  want((int)cfg->K_segm, 40);
  // the device call itself, which has no object here
  srslte_hip_ulsch_enc_cfg_t dc;
  srslte_hip_ulsch_enc_res_t res;
  memset(&dc, 0, sizeof(dc));
  memset(&res, 0x5A, sizeof(res));
  want(srslte_hip_ulsch_encode(nullptr, data, &dc, buffer_b, g_bits, q_bits, &res), SRSLTE_ERROR_INVALID_INPUTS);
  uint32_t words[2] = {0x5A5A5A5Au, 0x5A5A5A5Au};
  want(srslte_hip_ulsch_enc_debug(nullptr, words, 2), SRSLTE_ERROR_INVALID_INPUTS);
  bad += words[0] != 0x5A5A5A5Au || words[1] != 0x5A5A5A5Au;
  for (size_t i = 0; i < sizeof(res); i++) bad += ((uint8_t*)&res)[i] != 0x5A;
  srslte_hip_compat_stats_ul_tx(after);
  bad += after[0] != before[0] || after[1] != before[1];
  for (uint32_t i = 0; i < nof_bits / 8; i++) bad += q_bits[i] != 0xA5 || g_bits[i] != 0x3C;
  for (uint32_t i = 0; i < tbs / 8; i++) bad += data[i] != 0xC3;
  for (size_t i = 0; i < sizeof(*q); i++) bad += ((uint8_t*)q)[i] != 0x77; // the position list and upstream's scratch pointers
  for (int c = 0; c < 2; c++) {
    for (uint32_t i = 0; i < WB; i++) bad += buffer_b[c][i] != 0x11;
    free(buffer_b[c]);
  }
  free(buffer_b); free(data); free(g_bits); free(q_bits); free(uci); free(sb); free(cfg); free(q);
  if (bad) return 1;
  printf("ulsch encode host sanitizer run ok: %d checks\n", n);
  return 0;
}
