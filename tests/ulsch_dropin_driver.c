/* The reference's own PUSCH transmitter and receiver (lib/src/phy/phch/pusch.c, built into oracle/_ref/hip/libsrslte_upper.a) as they run when
 * linked against libsrslte_phy_hip.so, on an identity channel: srslte_pusch_decode calls srslte_ulsch_decode once per PUSCH (pusch.c:503).
 * tests/test_gpu_ulsch_dropin.py compiles this file twice at run time:
 *   plain    the archive's own sch.o serves that call - upstream's path: UCI and the de-interleaver on the host, then one srslte_tdec_iteration
 *            round trip into the library per code block and pass;
 *   wrapped  -DWRAPPED -Wl,--wrap=srslte_ulsch_decode: the call lands in the __wrap_ forwarder below, which hands it to the library's
 *            srslte_ulsch_decode (found with dlsym in the library itself) - one device call per transport block.
 * Struct layouts come from this repository's compat header; the four small structs of the PUSCH interface that it does not hold are declared
 * below as the reference's headers have them; srslte_pusch_t is opaque storage.
 *
 *   ulsch_dropin_driver run OUT    6 PRB QPSK tbs 600 with a 1-bit ACK and a wideband CQI report; 25 PRB 16QAM tbs 15264, rv 0 (fails: more bits than one
 *                                  transmission carries) then rv 2 on one soft buffer; 100 PRB 64QAM tbs 75376. OUT: per decode the return code, crc, ACK, report, and the decoded bytes.
 *   ulsch_dropin_driver time N     100 PRB / 64QAM / tbs 75376, no UCI: 20 warm-up decodes, then N timed ones. Prints "us_per_decode mean median min".
 * Both print "decodes=<n>", the library's counters "stats: <[0]> <[1]> <[2]> <[3]>" and "stats_ul: <calls> <waits>". Exit code 0 on success. */
#define _GNU_SOURCE
#include "srslte_hip/srslte_compat.h"
#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

typedef struct { srslte_tdd_config_t tdd_config; uint32_t tti; bool shortened; } srslte_ul_sf_cfg_t;                         /* phy_common.h:214-218 */
typedef struct { uint8_t* ptr; srslte_uci_value_t uci; } srslte_pusch_data_t;                                                /* pusch.h:84-87 */
typedef struct { uint8_t* data; srslte_uci_value_t uci; bool crc; float avg_iterations_block; } srslte_pusch_res_t;          /* pusch.h:89-94 */
typedef struct { cf_t* ce; uint32_t nof_re; float noise_estimate, noise_estimate_dbm, snr, snr_db, cfo; } srslte_chest_ul_res_t; /* chest_ul.h:47-55 */

int  srslte_pusch_init_ue(void* q, uint32_t max_prb);
int  srslte_pusch_init_enb(void* q, uint32_t max_prb);
int  srslte_pusch_set_cell(void* q, srslte_cell_t cell);
int  srslte_pusch_set_rnti(void* q, uint16_t rnti);
void srslte_pusch_free(void* q);
int  srslte_pusch_encode(void* q, srslte_ul_sf_cfg_t* sf, srslte_pusch_cfg_t* cfg, srslte_pusch_data_t* data, cf_t* sf_symbols);
int  srslte_pusch_decode(void* q, srslte_ul_sf_cfg_t* sf, srslte_pusch_cfg_t* cfg, srslte_chest_ul_res_t* channel, cf_t* sf_symbols, srslte_pusch_res_t* out);
int  srslte_softbuffer_tx_init(srslte_softbuffer_tx_t* q, uint32_t nof_prb);
void srslte_softbuffer_tx_reset(srslte_softbuffer_tx_t* q);
void srslte_softbuffer_tx_free(srslte_softbuffer_tx_t* q);
int  srslte_softbuffer_rx_init(srslte_softbuffer_rx_t* q, uint32_t nof_prb);
void srslte_softbuffer_rx_reset(srslte_softbuffer_rx_t* q);
void srslte_softbuffer_rx_free(srslte_softbuffer_rx_t* q);
void srslte_hip_compat_stats(unsigned long long out[4]);

#ifdef WRAPPED
int __wrap_srslte_ulsch_decode(srslte_sch_t* q, srslte_pusch_cfg_t* cfg, int16_t* q_bits, int16_t* g_bits, uint8_t* c_seq, uint8_t* data, srslte_uci_value_t* uci)
{
  static int (*f)(srslte_sch_t*, srslte_pusch_cfg_t*, int16_t*, int16_t*, uint8_t*, uint8_t*, srslte_uci_value_t*);
  if (!f) {
    Dl_info info;
    void*   lib = dladdr((void*)srslte_hip_compat_stats, &info) ? dlopen(info.dli_fname, RTLD_NOW | RTLD_NOLOAD) : NULL;
    *(void**)&f = lib ? dlsym(lib, "srslte_ulsch_decode") : NULL;
    if (!f) {
      fprintf(stderr, "srslte_ulsch_decode: not in the library\n");
      exit(20);
    }
  }
  return f(q, cfg, q_bits, g_bits, c_seq, data, uci);
}
#endif

#define PUSCH_STORAGE (8u << 20) /* sizeof(srslte_pusch_t): the srslte_sch_t with its 57600-entry position list, 111 DFT plans, a table of 65536 users */

static unsigned n_dec;

static double now_us(void)
{
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return 1e6 * (double)t.tv_sec + 1e-3 * (double)t.tv_nsec;
}

typedef struct {
  void *                 ue, *enb;
  srslte_cell_t          cell;
  srslte_softbuffer_tx_t sb_tx;
  srslte_softbuffer_rx_t sb_rx;
  srslte_pusch_cfg_t     cfg;
  uint8_t *              data, *out;
  cf_t *                 grid, *ce;
  size_t                 grid_len;
  int                    tbs;
} link_t;

static int link_init(link_t* t, uint32_t nof_prb, srslte_mod_t mod, int tbs)
{
  memset(t, 0, sizeof(*t));
  t->cell.nof_prb = nof_prb; t->cell.nof_ports = 1; t->cell.id = 1; t->cell.cp = SRSLTE_CP_NORM;
  t->tbs      = tbs;
  t->ue       = calloc(PUSCH_STORAGE, 1);
  t->enb      = calloc(PUSCH_STORAGE, 1);
  t->data     = malloc((size_t)tbs / 8 + 64);
  t->out      = malloc((size_t)tbs / 8 + 64);
  t->grid_len = (size_t)14 * 12 * nof_prb;
  t->grid     = calloc(t->grid_len, sizeof(cf_t));
  t->ce       = calloc(t->grid_len, sizeof(cf_t));
  if (!t->ue || !t->enb || !t->data || !t->out || !t->grid || !t->ce) return -1;
  for (size_t i = 0; i < t->grid_len; i++) ((float*)t->ce)[2 * i] = 1.0f; /* the identity channel */
  for (int i = 0; i < tbs / 8; i++) t->data[i] = (uint8_t)((i * 2654435761u) >> 13);
  if (srslte_pusch_init_ue(t->ue, nof_prb) || srslte_pusch_set_cell(t->ue, t->cell) || srslte_pusch_set_rnti(t->ue, 0x1234)) return -2;
  if (srslte_pusch_init_enb(t->enb, nof_prb) || srslte_pusch_set_cell(t->enb, t->cell) || srslte_pusch_set_rnti(t->enb, 0x1234)) return -3;
  if (srslte_softbuffer_tx_init(&t->sb_tx, nof_prb) || srslte_softbuffer_rx_init(&t->sb_rx, nof_prb)) return -4;
  srslte_softbuffer_tx_reset(&t->sb_tx);
  srslte_softbuffer_rx_reset(&t->sb_rx);
  srslte_pusch_grant_t* g = &t->cfg.grant;
  g->L_prb = nof_prb; g->nof_symb = 12; g->nof_re = 12 * 12 * nof_prb;
  g->tb.mod = mod; g->tb.tbs = tbs; g->tb.enabled = true;
  g->tb.nof_bits = g->nof_re * (mod == SRSLTE_MOD_QPSK ? 2 : mod == SRSLTE_MOD_16QAM ? 4 : 6);
  t->cfg.rnti = 0x1234;
  t->cfg.enable_64qam = true;
  t->cfg.uci_offset.I_offset_ack = 9; t->cfg.uci_offset.I_offset_ri = 6; t->cfg.uci_offset.I_offset_cqi = 6;
  return 0;
}

/* one subframe through srslte_pusch_encode; < 0 on failure */
static int link_encode(link_t* t, uint32_t tti, int rv, const srslte_uci_value_t* uci)
{
  srslte_ul_sf_cfg_t sf;
  memset(&sf, 0, sizeof(sf));
  sf.tti = tti;
  srslte_pusch_cfg_t cfg = t->cfg;
  cfg.grant.tb.rv   = rv;
  cfg.softbuffers.tx = &t->sb_tx;
  srslte_pusch_data_t d;
  memset(&d, 0, sizeof(d));
  d.ptr = t->data;
  if (uci) d.uci = *uci;
  memset(t->grid, 0, t->grid_len * sizeof(cf_t));
  return srslte_pusch_encode(t->ue, &sf, &cfg, &d, t->grid);
}

/* one srslte_pusch_decode of what link_encode left -> its duration in us (negative: the call failed); res: what it returned */
static double link_decode(link_t* t, uint32_t tti, int rv, srslte_pusch_res_t* res)
{
  srslte_ul_sf_cfg_t sf;
  memset(&sf, 0, sizeof(sf));
  sf.tti = tti;
  srslte_pusch_cfg_t cfg = t->cfg;
  cfg.grant.tb.rv    = rv;
  cfg.softbuffers.rx = &t->sb_rx;
  srslte_chest_ul_res_t ch;
  memset(&ch, 0, sizeof(ch));
  ch.ce = t->ce; ch.nof_re = (uint32_t)t->grid_len; ch.snr_db = 30.0f;
  memset(res, 0, sizeof(*res));
  memset(t->out, 0, (size_t)t->tbs / 8 + 64);
  res->data = t->out;
  const double t0 = now_us();
  if (srslte_pusch_decode(t->enb, &sf, &cfg, &ch, t->grid, res)) return -1.0;
  n_dec++;
  return now_us() - t0;
}

static void link_free(link_t* t)
{
  srslte_pusch_free(t->ue);
  srslte_pusch_free(t->enb);
  srslte_softbuffer_tx_free(&t->sb_tx);
  srslte_softbuffer_rx_free(&t->sb_rx);
  free(t->ue); free(t->enb); free(t->data); free(t->out); free(t->grid); free(t->ce);
}

static int record(FILE* out, const char* what, link_t* t, const srslte_pusch_res_t* r, double us)
{
  const uint8_t head[8] = {(uint8_t)r->crc, r->uci.ack.ack_value[0], r->uci.cqi.wideband.wideband_cqi, (uint8_t)r->uci.cqi.data_crc, r->uci.ri, 0, 0, 0};
  printf("%s: crc %d, %.0f us\n", what, (int)r->crc, us);
  return fwrite(head, 1, 8, out) == 8 && fwrite(t->out, 1, (size_t)t->tbs / 8, out) == (size_t)t->tbs / 8 ? 0 : -1;
}

static int cmp(const void* a, const void* b) { return *(const double*)a < *(const double*)b ? -1 : *(const double*)a > *(const double*)b; }

int main(int argc, char** argv)
{
  if (argc != 3) return 2;
  link_t             t;
  srslte_pusch_res_t r;
  if (!strcmp(argv[1], "run")) {
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 3;
    /* 6 PRB QPSK with a 1-bit ACK and a wideband report */
    if (link_init(&t, 6, SRSLTE_MOD_QPSK, 600)) return 4;
    t.cfg.uci_cfg.ack[0].nof_acks = 1;
    t.cfg.uci_cfg.cqi.data_enable = true;
    t.cfg.uci_cfg.cqi.type        = SRSLTE_CQI_TYPE_WIDEBAND;
    srslte_uci_value_t uci;
    memset(&uci, 0, sizeof(uci));
    uci.ack.ack_value[0]         = 1;
    uci.cqi.wideband.wideband_cqi = 11;
    if (link_encode(&t, 1, 0, &uci) < 0) return 5;
    double us = link_decode(&t, 1, 0, &r);
    if (us < 0 || !r.crc || r.uci.ack.ack_value[0] != 1 || r.uci.cqi.wideband.wideband_cqi != 11 || memcmp(t.out, t.data, 600 / 8)) return 6;
    if (record(out, "6 PRB QPSK tbs 600 ACK + CQI", &t, &r, us)) return 7;
    link_free(&t);
    /* 25 PRB 16QAM, rv 0 then rv 2 on one soft buffer: 15264 bits (C = 3, K = 5120) do not fit the 14400 of one transmission, so rv 0 fails
     * and leaves its soft values, and rv 2 combines into them and decodes */
    if (link_init(&t, 25, SRSLTE_MOD_16QAM, 15264)) return 8;
    for (int rv = 0; rv <= 2; rv += 2) {
      if (link_encode(&t, 2, rv, NULL) < 0) return 9;
      us = link_decode(&t, 2, rv, &r);
      if (us < 0 || r.crc != (rv == 2) || (rv == 2 && memcmp(t.out, t.data, 15264 / 8))) return 10;
      if (record(out, rv ? "25 PRB 16QAM tbs 15264 rv 2" : "25 PRB 16QAM tbs 15264 rv 0", &t, &r, us)) return 11;
    }
    link_free(&t);
    /* 100 PRB 64QAM */
    if (link_init(&t, 100, SRSLTE_MOD_64QAM, 75376)) return 12;
    if (link_encode(&t, 3, 0, NULL) < 0) return 13;
    us = link_decode(&t, 3, 0, &r);
    if (us < 0 || !r.crc || memcmp(t.out, t.data, 75376 / 8)) return 14;
    if (record(out, "100 PRB 64QAM tbs 75376", &t, &r, us)) return 15;
    link_free(&t);
    if (fclose(out)) return 16;
  } else if (!strcmp(argv[1], "time")) {
    const int n = atoi(argv[2]);
    if (n < 1 || n > 100000) return 2;
    double* us = malloc(sizeof(double) * (size_t)n);
    if (!us || link_init(&t, 100, SRSLTE_MOD_64QAM, 75376)) return 12;
    if (link_encode(&t, 3, 0, NULL) < 0) return 13;
    double sum = 0;
    for (int i = -20; i < n; i++) { /* 20 warm-up decodes: tables, streams and the device object are made in the first */
      srslte_softbuffer_rx_reset(&t.sb_rx);
      const double d = link_decode(&t, 3, 0, &r);
      if (d < 0 || !r.crc) return 14;
      if (i >= 0) us[i] = d, sum += d;
    }
    qsort(us, (size_t)n, sizeof(double), cmp);
    printf("us_per_decode %.1f %.1f %.1f\n", sum / n, us[n / 2], us[0]);
    link_free(&t);
    free(us);
  } else {
    return 2;
  }
  unsigned long long st[4], ul[2];
  srslte_hip_compat_stats(st);
  srslte_hip_compat_stats_ul(ul);
  printf("decodes=%u\nstats: %llu %llu %llu %llu\nstats_ul: %llu %llu\n", n_dec, st[0], st[1], st[2], st[3], ul[0], ul[1]);
  return 0;
}
