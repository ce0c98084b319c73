// TEST INFRASTRUCTURE: the host function behind srslte_dlsch_encode2 / srslte_dlsch_encode (compat.cpp) under AddressSanitizer +
// UndefinedBehaviorSanitizer on the CPU, in a program of its own: every path of it that ends before the device is needed - the argument
// checks, the segmentation, upstream's refusals (filler bits, a soft buffer of too few blocks), the empty transport block and what the
// library refuses beyond upstream. The structs are heap blocks of exactly their size, so a read or write past one shows as a heap overflow.
// The served path (the calling thread's encoder object, srslte_hip_sch_encode) needs a device and is not run here: GPU runs take no
// sanitizer. Built and run by tests/test_sch_encode_sanitizer.py from compat.cpp and fec_tables.cpp (both instrumented) and the library.
#include "srslte_hip/phy_hip.h"
#include "srslte_hip/srslte_compat.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

template <typename T> static T* exact()
{
  T* p = (T*)malloc(sizeof(T));
  if (!p) exit(3);
  memset(p, 0, sizeof(T));
  return p;
}

int main()
{
  srslte_sch_t*           q   = exact<srslte_sch_t>();
  srslte_pdsch_cfg_t*     cfg = exact<srslte_pdsch_cfg_t>();
  srslte_softbuffer_tx_t* sb  = exact<srslte_softbuffer_tx_t>();
  uint8_t *               data = (uint8_t*)malloc(6200 / 8), *e = (uint8_t*)malloc(376);
  uint8_t**               bufs = (uint8_t**)malloc(sizeof(uint8_t*));
  if (!data || !e || !bufs) return 3;
  memset(data, 0x3c, 6200 / 8);
  memset(e, 0xA5, 376);
  bufs[0]      = nullptr;
  sb->max_cb   = 1;
  sb->buffer_b = bufs;
  cfg->grant.nof_tb = 1;
  srslte_ra_tb_t* tb = &cfg->grant.tb[0];
  tb->mod = SRSLTE_MOD_QPSK; tb->tbs = 6200; tb->rv = 0; tb->nof_bits = 3002; tb->enabled = true;
  cfg->softbuffers.tx[0] = sb;
  unsigned long long before[4], after[4];
  srslte_hip_compat_stats(before);
  int bad = 0, n = 0;
  auto want = [&](int got, int expected) {
    n++;
    if (got != expected) {
      fprintf(stderr, "check %d: %d, expected %d\n", n, got, expected);
      bad++;
    }
  };
  want(srslte_dlsch_encode2(q, nullptr, data, e, 0, 1), SRSLTE_ERROR_INVALID_INPUTS);
  want(srslte_dlsch_encode2(q, cfg, data, e, -1, 1), SRSLTE_ERROR_INVALID_INPUTS);
  want(srslte_dlsch_encode2(q, cfg, data, e, SRSLTE_MAX_CODEWORDS, 1), SRSLTE_ERROR_INVALID_INPUTS);
  want(srslte_dlsch_encode2(nullptr, cfg, data, e, 0, 1), SRSLTE_ERROR_INVALID_INPUTS);
  want(srslte_dlsch_encode2(q, cfg, data, nullptr, 0, 1), SRSLTE_ERROR_INVALID_INPUTS);
  want(srslte_dlsch_encode2(q, cfg, data, e, 1, 1), SRSLTE_ERROR_INVALID_INPUTS); // codeword 1 has no soft buffer
  want(srslte_dlsch_encode2(q, cfg, data, e, 0, 1), -1);                          // C = 2 blocks, a soft buffer of one
  want(srslte_dlsch_encode(q, cfg, data, e), -1);
  tb->tbs = 4016;
  want(srslte_dlsch_encode2(q, cfg, data, e, 0, 1), SRSLTE_ERROR); // filler bits
  tb->tbs = 0;
  want(srslte_dlsch_encode2(q, cfg, data, e, 0, 2), SRSLTE_SUCCESS); // no transport block
  want(srslte_dlsch_encode2(q, cfg, nullptr, e, 0, 1), SRSLTE_SUCCESS);
  tb->tbs = 328;
  tb->mod = SRSLTE_MOD_BPSK;
  want(srslte_dlsch_encode2(q, cfg, data, e, 0, 1), SRSLTE_ERROR_INVALID_INPUTS);
  tb->mod = SRSLTE_MOD_QPSK;
  tb->nof_bits = 0;
  want(srslte_dlsch_encode2(q, cfg, data, e, 0, 1), SRSLTE_ERROR_INVALID_INPUTS);
  tb->nof_bits = 1200;
  sb->buffer_b = nullptr;
  want(srslte_dlsch_encode2(q, cfg, data, e, 0, 1), SRSLTE_ERROR_INVALID_INPUTS);
  srslte_hip_compat_stats(after);
  for (int i = 0; i < 376; i++) bad += e[i] != 0xA5;
  bad += after[3] != before[3];
  free(bufs); free(e); free(data); free(sb); free(cfg); free(q);
  if (bad) return 1;
  printf("sch encode host sanitizer run ok: %d checks\n", n);
  return 0;
}
