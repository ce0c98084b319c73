// TEST INFRASTRUCTURE: the host function behind srslte_ulsch_decode (compat.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer on the
// CPU, in a program of its own: every path of it that ends before a device is needed - NULL arguments, a transport block that does not
// segment, and each refusal of srslte_compat.h. The structs are heap blocks of exactly their size, so a read or write past one shows as a heap
// overflow; data, uci_data and the soft buffer carry a pattern that must survive every refused call, cfg->K_segm must be written, and the
// counter of served calls must not move. The served path needs a device and is not run here: GPU runs take no sanitizer. Built and run by
// tests/test_ulsch_sanitizer.py from compat.cpp and fec_tables.cpp (both instrumented) and the library.
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
  srslte_sch_t*           q   = exact<srslte_sch_t>();
  srslte_pusch_cfg_t*     cfg = exact<srslte_pusch_cfg_t>();
  srslte_softbuffer_rx_t* sb  = exact<srslte_softbuffer_rx_t>();
  srslte_uci_value_t*     uci = exact<srslte_uci_value_t>(0x5A);
  const uint32_t          nof_bits = 6 * 12 * 12 * 2, tbs = 6200, LEN = 3 * (3136 + 32) + 12; // 6 PRB, QPSK; tbs 6200: C = 2, K = 3136
  int16_t*                q_bits = (int16_t*)malloc(sizeof(int16_t) * nof_bits);
  uint8_t *               c_seq = (uint8_t*)malloc(nof_bits), *data = (uint8_t*)malloc(tbs / 8 + 3);
  int16_t**               buffer_f = (int16_t**)malloc(2 * sizeof(int16_t*));
  uint8_t**               sdata    = (uint8_t**)malloc(2 * sizeof(uint8_t*));
  bool*                   cb_crc   = (bool*)malloc(2 * sizeof(bool));
  if (!q_bits || !c_seq || !data || !buffer_f || !sdata || !cb_crc) return 3;
  for (uint32_t i = 0; i < nof_bits; i++) q_bits[i] = (int16_t)(i * 37 % 201 - 100), c_seq[i] = (uint8_t)(i * 7 % 2);
  memset(data, 0xC3, tbs / 8 + 3);
  for (int c = 0; c < 2; c++) {
    buffer_f[c] = (int16_t*)malloc(sizeof(int16_t) * LEN);
    sdata[c]    = (uint8_t*)malloc(3136 / 8);
    if (!buffer_f[c] || !sdata[c]) return 3;
    memset(buffer_f[c], 0x11, sizeof(int16_t) * LEN);
    memset(sdata[c], 0x22, 3136 / 8);
    cb_crc[c] = false;
  }
  sb->max_cb = 2; sb->buffer_f = buffer_f; sb->data = sdata; sb->cb_crc = cb_crc; sb->tb_crc = false;
  q->max_iterations = 4;
  cfg->grant.L_prb = 6; cfg->grant.nof_symb = 12;
  srslte_ra_tb_t* tb = &cfg->grant.tb;
  tb->mod = SRSLTE_MOD_QPSK; tb->tbs = (int)tbs; tb->rv = 0; tb->nof_bits = nof_bits; tb->enabled = true;
  cfg->softbuffers.rx = sb;
  cfg->uci_cfg.ack[0].nof_acks = 1;
  cfg->uci_offset.I_offset_ack = 9; cfg->uci_offset.I_offset_ri = 6; cfg->uci_offset.I_offset_cqi = 6;
  unsigned long long before[2], after[2];
  srslte_hip_compat_stats_ul(before);
  int  bad = 0, n = 0;
  auto want = [&](int got, int expected) {
    n++;
    if (got != expected) {
      fprintf(stderr, "check %d: %d, expected %d\n", n, got, expected);
      bad++;
    }
  };
  auto call = [&]() { return srslte_ulsch_decode(q, cfg, q_bits, nullptr, c_seq, data, uci); };
  // NULL arguments
  want(srslte_ulsch_decode(nullptr, cfg, q_bits, nullptr, c_seq, data, uci), SRSLTE_ERROR_INVALID_INPUTS);
  want(srslte_ulsch_decode(q, nullptr, q_bits, nullptr, c_seq, data, uci), SRSLTE_ERROR_INVALID_INPUTS);
  want(srslte_ulsch_decode(q, cfg, nullptr, nullptr, c_seq, data, uci), SRSLTE_ERROR_INVALID_INPUTS);
  want(srslte_ulsch_decode(q, cfg, q_bits, nullptr, nullptr, data, uci), SRSLTE_ERROR_INVALID_INPUTS);
  want(srslte_ulsch_decode(q, cfg, q_bits, nullptr, c_seq, data, nullptr), SRSLTE_ERROR_INVALID_INPUTS);
  want((int)cfg->K_segm, 0); // nothing has got as far as the segmentation
  want(srslte_ulsch_decode(q, cfg, q_bits, nullptr, c_seq, nullptr, uci), SRSLTE_ERROR_INVALID_INPUTS); // tbs > 0 without data
  want((int)cfg->K_segm, 2 * 3136);                                                                  // sch.c:1011, written before the refusal
  cfg->softbuffers.rx = nullptr;
  want(call(), SRSLTE_ERROR_INVALID_INPUTS);
  cfg->softbuffers.rx = sb;
  sb->max_cb = 1; // two blocks into a soft buffer of one
  want(call(), SRSLTE_ERROR_INVALID_INPUTS);
  sb->max_cb = 2;
  // the refusals of srslte_compat.h
  q->llr_is_8bit = true;
  want(call(), SRSLTE_ERROR_INVALID_INPUTS);
  q->llr_is_8bit = false;
  tb->mod = SRSLTE_MOD_BPSK;
  want(call(), SRSLTE_ERROR_INVALID_INPUTS);
  tb->mod = SRSLTE_MOD_256QAM;
  want(call(), SRSLTE_ERROR_INVALID_INPUTS);
  tb->mod = SRSLTE_MOD_QPSK;
  tb->tbs = 4016; // filler bits
  cfg->K_segm = 0;
  want(call(), SRSLTE_ERROR_INVALID_INPUTS);
  want((int)cfg->K_segm >= 4016 + 24 ? 1 : 0, 1);
  tb->tbs = 6208; // C = 2 with two block sizes: K_segm is their sum
  want(call(), SRSLTE_ERROR_INVALID_INPUTS);
  want((int)cfg->K_segm > 6208 ? 1 : 0, 1);
  tb->tbs = (int)tbs;
  tb->nof_bits = nof_bits - 2; // no multiple of nof_symb Qm
  want(call(), SRSLTE_ERROR_INVALID_INPUTS);
  tb->nof_bits = nof_bits;
  cfg->grant.nof_symb = 8;
  want(call(), SRSLTE_ERROR_INVALID_INPUTS);
  cfg->grant.nof_symb = 12;
  cfg->uci_cfg.cqi.ri_len = 3;
  want(call(), SRSLTE_ERROR_INVALID_INPUTS);
  cfg->uci_cfg.cqi.ri_len = 0;
  cfg->uci_offset.I_offset_ack = 16;
  want(call(), SRSLTE_ERROR_INVALID_INPUTS);
  cfg->uci_offset.I_offset_ack = 9;
  tb->tbs = 0; // a PUSCH without data and without a report
  want(call(), SRSLTE_ERROR_INVALID_INPUTS);
  want((int)cfg->K_segm, 0);
  tb->tbs = (int)tbs;
  want(call(), SRSLTE_ERROR_INVALID_INPUTS); // everything in order, but the decoder of this srslte_sch_t was never initialised
  srslte_hip_compat_stats_ul(after);
  bad += after[0] != before[0] || after[1] != before[1];
  for (uint32_t i = 0; i < tbs / 8 + 3; i++) bad += data[i] != 0xC3;
  for (size_t i = 0; i < sizeof(*uci); i++) bad += ((uint8_t*)uci)[i] != 0x5A;
  for (int c = 0; c < 2; c++) {
    for (uint32_t i = 0; i < LEN; i++) bad += buffer_f[c][i] != 0x1111;
    for (uint32_t i = 0; i < 3136 / 8; i++) bad += sdata[c][i] != 0x22;
    bad += cb_crc[c];
    free(buffer_f[c]);
    free(sdata[c]);
  }
  bad += sb->tb_crc || cfg->uci_cfg.cqi.rank_is_not_one;
  for (uint32_t i = 0; i < nof_bits; i++) bad += q_bits[i] != (int16_t)(i * 37 % 201 - 100);
  free(cb_crc); free(sdata); free(buffer_f); free(data); free(c_seq); free(q_bits); free(uci); free(sb); free(cfg); free(q);
  if (bad) return 1;
  printf("ulsch host sanitizer run ok: %d checks\n", n);
  return 0;
}
