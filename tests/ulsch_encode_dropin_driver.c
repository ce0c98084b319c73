/* The reference's own PUSCH transmitter (lib/src/phy/phch/pusch.c, built into oracle/_ref/hip/libsrslte_upper.a) as it runs when linked against
 * libsrslte_phy_hip.so: srslte_pusch_encode calls srslte_ulsch_encode once per PUSCH (pusch.c:367).
 * tests/test_gpu_ulsch_encode_dropin.py compiles this file twice at run time:
 *   plain    the archive's own sch.o serves that call - upstream's path: the report and the channel interleaver on the host, and one
 *            srslte_tcod_encode_lut round trip into the library per code block;
 *   wrapped  -DWRAPPED -Wl,--wrap=srslte_ulsch_encode: the call lands in the __wrap_ forwarder below, which hands it to the library's
 *            srslte_ulsch_encode (found with dlsym in the library itself) - one device call per transport block.
 * Both builds are linked with -Wl,--wrap=srslte_tcod_encode_lut: the forwarder below counts the entries sch.o makes and passes them on.
 * Struct layouts come from this repository's compat header; the two small structs of the PUSCH interface that it does not hold are declared
 * below as the reference's headers have them; srslte_pusch_t is opaque storage.
 *
 *   ulsch_encode_dropin_driver run OUT      6 PRB 64QAM tbs 4008 with a 1-bit ACK and a wideband CQI report; 25 PRB 16QAM tbs 15264, rv 0 then rv 2 on
 *                                           one soft buffer; 100 PRB 64QAM tbs 75376 without UCI and with a 2-bit ACK and a 1-bit RI. OUT: the five resource grids.
 *   ulsch_encode_dropin_driver time N UCI   100 PRB / 64QAM / tbs 75376, UCI 0: no UCI, 1: a 2-bit ACK and a wideband report. 20 warm-up encodes,
 *                                           then N timed ones. Prints "us_per_encode median p10 p90 min".
 * Both print "encodes=<n>", "lut_entries=<n>", the library's counters "stats: <[0]> <[1]> <[2]> <[3]>" and "stats_ul_tx: <calls> <waits>".
 * Exit code 0 on success. */
#define _GNU_SOURCE
#include "srslte_hip/srslte_compat.h"
#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

typedef struct { srslte_tdd_config_t tdd_config; uint32_t tti; bool shortened; } srslte_ul_sf_cfg_t; /* phy_common.h:214-218 */
typedef struct { uint8_t* ptr; srslte_uci_value_t uci; } srslte_pusch_data_t;                        /* pusch.h:84-87 */

int  srslte_pusch_init_ue(void* q, uint32_t max_prb);
int  srslte_pusch_set_cell(void* q, srslte_cell_t cell);
int  srslte_pusch_set_rnti(void* q, uint16_t rnti);
void srslte_pusch_free(void* q);
int  srslte_pusch_encode(void* q, srslte_ul_sf_cfg_t* sf, srslte_pusch_cfg_t* cfg, srslte_pusch_data_t* data, cf_t* sf_symbols);
int  srslte_softbuffer_tx_init(srslte_softbuffer_tx_t* q, uint32_t nof_prb);
void srslte_softbuffer_tx_reset(srslte_softbuffer_tx_t* q);
void srslte_softbuffer_tx_free(srslte_softbuffer_tx_t* q);
void srslte_hip_compat_stats(unsigned long long out[4]);

static unsigned n_enc, n_lut;

int __real_srslte_tcod_encode_lut(srslte_tcod_t* h, srslte_crc_t* crc_tb, srslte_crc_t* crc_cb, uint8_t* input, uint8_t* parity, uint32_t cblen_idx, bool last_cb);
int __wrap_srslte_tcod_encode_lut(srslte_tcod_t* h, srslte_crc_t* crc_tb, srslte_crc_t* crc_cb, uint8_t* input, uint8_t* parity, uint32_t cblen_idx, bool last_cb)
{
  n_lut++;
  return __real_srslte_tcod_encode_lut(h, crc_tb, crc_cb, input, parity, cblen_idx, last_cb);
}

#ifdef WRAPPED
int __wrap_srslte_ulsch_encode(srslte_sch_t* q, srslte_pusch_cfg_t* cfg, uint8_t* data, srslte_uci_value_t* uci, uint8_t* g_bits, uint8_t* q_bits)
{
  static int (*f)(srslte_sch_t*, srslte_pusch_cfg_t*, uint8_t*, srslte_uci_value_t*, uint8_t*, uint8_t*);
  if (!f) {
    Dl_info info;
    void*   lib = dladdr((void*)srslte_hip_compat_stats, &info) ? dlopen(info.dli_fname, RTLD_NOW | RTLD_NOLOAD) : NULL;
    *(void**)&f = lib ? dlsym(lib, "srslte_ulsch_encode") : NULL;
    if (!f) {
      fprintf(stderr, "srslte_ulsch_encode: not in the library\n");
      exit(20);
    }
  }
  return f(q, cfg, data, uci, g_bits, q_bits);
}
#endif

#define PUSCH_STORAGE (8u << 20) /* sizeof(srslte_pusch_t): the srslte_sch_t with its 57600-entry position list, 111 DFT plans, a table of 65536 users */

static double now_us(void)
{
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return 1e6 * (double)t.tv_sec + 1e-3 * (double)t.tv_nsec;
}

typedef struct {
  void*                  ue;
  srslte_cell_t          cell;
  srslte_softbuffer_tx_t sb_tx;
  srslte_pusch_cfg_t     cfg;
  uint8_t*               data;
  cf_t*                  grid;
  size_t                 grid_len;
} link_t;

static int link_init(link_t* t, uint32_t nof_prb, srslte_mod_t mod, int tbs)
{
  memset(t, 0, sizeof(*t));
  t->cell.nof_prb = nof_prb; t->cell.nof_ports = 1; t->cell.id = 1; t->cell.cp = SRSLTE_CP_NORM;
  t->ue       = calloc(PUSCH_STORAGE, 1);
  t->data     = malloc((size_t)tbs / 8 + 64);
  t->grid_len = (size_t)14 * 12 * nof_prb;
  t->grid     = calloc(t->grid_len, sizeof(cf_t));
  if (!t->ue || !t->data || !t->grid) return -1;
  for (int i = 0; i < tbs / 8; i++) t->data[i] = (uint8_t)((i * 2654435761u) >> 13);
  if (srslte_pusch_init_ue(t->ue, nof_prb) || srslte_pusch_set_cell(t->ue, t->cell) || srslte_pusch_set_rnti(t->ue, 0x1234)) return -2;
  if (srslte_softbuffer_tx_init(&t->sb_tx, nof_prb)) return -4;
  srslte_softbuffer_tx_reset(&t->sb_tx);
  srslte_pusch_grant_t* g = &t->cfg.grant;
  g->L_prb = nof_prb; g->nof_symb = 12; g->nof_re = 12 * 12 * nof_prb;
  g->tb.mod = mod; g->tb.tbs = tbs; g->tb.enabled = true;
  g->tb.nof_bits = g->nof_re * (mod == SRSLTE_MOD_QPSK ? 2 : mod == SRSLTE_MOD_16QAM ? 4 : 6);
  t->cfg.rnti = 0x1234;
  t->cfg.enable_64qam = true;
  t->cfg.uci_offset.I_offset_ack = 9; t->cfg.uci_offset.I_offset_ri = 6; t->cfg.uci_offset.I_offset_cqi = 6;
  return 0;
}

/* one subframe through srslte_pusch_encode -> its duration in us; negative on failure */
static double link_encode(link_t* t, uint32_t tti, int rv, const srslte_uci_value_t* uci)
{
  srslte_ul_sf_cfg_t sf;
  memset(&sf, 0, sizeof(sf));
  sf.tti = tti;
  srslte_pusch_cfg_t cfg = t->cfg;
  cfg.grant.tb.rv    = rv;
  cfg.softbuffers.tx = &t->sb_tx;
  srslte_pusch_data_t d;
  memset(&d, 0, sizeof(d));
  d.ptr = t->data;
  if (uci) d.uci = *uci;
  memset(t->grid, 0, t->grid_len * sizeof(cf_t));
  const double t0 = now_us();
  if (srslte_pusch_encode(t->ue, &sf, &cfg, &d, t->grid) < 0) return -1.0;
  n_enc++;
  return now_us() - t0;
}

static void link_free(link_t* t)
{
  srslte_pusch_free(t->ue);
  srslte_softbuffer_tx_free(&t->sb_tx);
  free(t->ue); free(t->data); free(t->grid);
}

static int record(FILE* out, const char* what, const link_t* t, double us)
{
  printf("%s: %.0f us\n", what, us);
  return fwrite(t->grid, sizeof(cf_t), t->grid_len, out) == t->grid_len ? 0 : -1;
}

static int cmp(const void* a, const void* b) { return *(const double*)a < *(const double*)b ? -1 : *(const double*)a > *(const double*)b; }

int main(int argc, char** argv)
{
  if (argc < 3) return 2;
  link_t             t;
  srslte_uci_value_t uci;
  memset(&uci, 0, sizeof(uci));
  if (!strcmp(argv[1], "run") && argc == 3) {
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 3;
    /* 6 PRB 64QAM with a 1-bit ACK and a wideband report */
    if (link_init(&t, 6, SRSLTE_MOD_64QAM, 4008)) return 4;
    t.cfg.uci_cfg.ack[0].nof_acks = 1;
    t.cfg.uci_cfg.cqi.data_enable = true;
    t.cfg.uci_cfg.cqi.type        = SRSLTE_CQI_TYPE_WIDEBAND;
    uci.ack.ack_value[0]          = 1;
    uci.cqi.wideband.wideband_cqi = 11;
    double us = link_encode(&t, 1, 0, &uci);
    if (us < 0 || record(out, "6 PRB 64QAM tbs 4008 ACK + CQI", &t, us)) return 5;
    link_free(&t);
    /* 25 PRB 16QAM, rv 0 then rv 2 on one soft buffer (C = 3, K = 5120) */
    if (link_init(&t, 25, SRSLTE_MOD_16QAM, 15264)) return 8;
    for (int rv = 0; rv <= 2; rv += 2) {
      us = link_encode(&t, 2, rv, NULL);
      if (us < 0 || record(out, rv ? "25 PRB 16QAM tbs 15264 rv 2" : "25 PRB 16QAM tbs 15264 rv 0", &t, us)) return 9;
    }
    link_free(&t);
    /* 100 PRB 64QAM (C = 13), then the same with a 2-bit ACK and a 1-bit RI */
    if (link_init(&t, 100, SRSLTE_MOD_64QAM, 75376)) return 12;
    us = link_encode(&t, 3, 0, NULL);
    if (us < 0 || record(out, "100 PRB 64QAM tbs 75376", &t, us)) return 13;
    memset(&uci, 0, sizeof(uci));
    t.cfg.uci_cfg.ack[0].nof_acks = 2;
    t.cfg.uci_cfg.cqi.ri_len      = 1;
    uci.ack.ack_value[0] = 1; uci.ack.ack_value[1] = 0; uci.ri = 1;
    us = link_encode(&t, 4, 0, &uci);
    if (us < 0 || record(out, "100 PRB 64QAM tbs 75376 ACK + RI", &t, us)) return 14;
    link_free(&t);
    if (fclose(out)) return 16;
  } else if (!strcmp(argv[1], "time") && argc == 4) {
    const int n = atoi(argv[2]), with_uci = atoi(argv[3]);
    if (n < 10 || n > 100000) return 2;
    double* us = malloc(sizeof(double) * (size_t)n);
    if (!us || link_init(&t, 100, SRSLTE_MOD_64QAM, 75376)) return 12;
    if (with_uci) {
      t.cfg.uci_cfg.ack[0].nof_acks = 2;
      t.cfg.uci_cfg.cqi.data_enable = true;
      t.cfg.uci_cfg.cqi.type        = SRSLTE_CQI_TYPE_WIDEBAND;
      uci.ack.ack_value[0] = 1; uci.ack.ack_value[1] = 1;
      uci.cqi.wideband.wideband_cqi = 9;
    }
    for (int i = -20; i < n; i++) { /* 20 warm-up encodes: tables, streams and the device object are made in the first */
      const double d = link_encode(&t, 3, 0, with_uci ? &uci : NULL);
      if (d < 0) return 14;
      if (i >= 0) us[i] = d;
    }
    qsort(us, (size_t)n, sizeof(double), cmp);
    printf("us_per_encode %.1f %.1f %.1f %.1f\n", us[n / 2], us[n / 10], us[n - 1 - n / 10], us[0]);
    link_free(&t);
    free(us);
  } else {
    return 2;
  }
  unsigned long long st[4], tx[2];
  srslte_hip_compat_stats(st);
  srslte_hip_compat_stats_ul_tx(tx);
  printf("encodes=%u\nlut_entries=%u\nstats: %llu %llu %llu %llu\nstats_ul_tx: %llu %llu\n", n_enc, n_lut, st[0], st[1], st[2], st[3], tx[0], tx[1]);
  return 0;
}
