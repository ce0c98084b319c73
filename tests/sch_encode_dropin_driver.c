/* The reference's own PDSCH transmitter (lib/src/phy/phch/pdsch.c, built into oracle/_ref/hip/libsrslte_upper.a) as it runs when linked against
 * libsrslte_phy_hip.so: srslte_pdsch_encode calls srslte_dlsch_encode2 once per codeword (pdsch.c:1032). tests/test_gpu_sch_encode_dropin.py
 * compiles this file twice at run time:
 *   plain    the archive's own sch.o serves that call - upstream's loop, one srslte_tcod_encode_lut round trip into the library per code block;
 *   wrapped  -DWRAPPED -Wl,--wrap=srslte_dlsch_encode2 -Wl,--wrap=srslte_dlsch_encode: the call lands in the __wrap_ forwarders below, which hand
 *            it to the library's srslte_dlsch_encode2 (found with dlsym in the library itself) - one device call per transport block.
 * Struct layouts come from this repository's compat header; srslte_pdsch_t is opaque storage, so no reference header is needed.
 *
 *   sch_encode_dropin_driver grid OUT   25 PRB: tbs 4008 16QAM, rv 0 then rv 2, for two subframes; 100 PRB: tbs 75376 64QAM for two subframes.
 *                                       OUT: the resource grids of all six calls. Prints the time of each call.
 *   sch_encode_dropin_driver time N     100 PRB / tbs 75376: one warm-up subframe, then N timed ones. Prints "us_per_encode mean median min".
 * Both print "transport_blocks=<n>" and the library's counters, "stats: <[0]> <[1]> <[2]> <[3]>". Exit code 0 on success. */
#define _GNU_SOURCE
#include "srslte_hip/srslte_compat.h"
#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

int  srslte_pdsch_init_enb(void* q, uint32_t max_prb);
int  srslte_pdsch_set_cell(void* q, srslte_cell_t cell);
int  srslte_pdsch_set_rnti(void* q, uint16_t rnti);
void srslte_pdsch_free(void* q);
int  srslte_pdsch_encode(void* q, srslte_dl_sf_cfg_t* sf, srslte_pdsch_cfg_t* cfg, uint8_t* data[SRSLTE_MAX_CODEWORDS], cf_t* sf_symbols[SRSLTE_MAX_PORTS]);
void srslte_ra_dl_compute_nof_re(srslte_cell_t* cell, srslte_dl_sf_cfg_t* sf, srslte_pdsch_grant_t* grant);
int  srslte_softbuffer_tx_init(srslte_softbuffer_tx_t* q, uint32_t nof_prb);
void srslte_softbuffer_tx_reset(srslte_softbuffer_tx_t* q);
void srslte_softbuffer_tx_free(srslte_softbuffer_tx_t* q);
void srslte_hip_compat_stats(unsigned long long out[4]);

#ifdef WRAPPED
static void* library_symbol(const char* name)
{
  static void* lib;
  Dl_info      info;
  if (!lib && dladdr((void*)srslte_hip_compat_stats, &info)) lib = dlopen(info.dli_fname, RTLD_NOW | RTLD_NOLOAD);
  void* f = lib ? dlsym(lib, name) : NULL;
  if (!f) {
    fprintf(stderr, "%s: not in the library\n", name);
    exit(20);
  }
  return f;
}
int __wrap_srslte_dlsch_encode2(srslte_sch_t* q, srslte_pdsch_cfg_t* cfg, uint8_t* data, uint8_t* e_bits, int tb_idx, uint32_t nof_layers)
{
  static int (*f)(srslte_sch_t*, srslte_pdsch_cfg_t*, uint8_t*, uint8_t*, int, uint32_t);
  if (!f) *(void**)&f = library_symbol("srslte_dlsch_encode2");
  return f(q, cfg, data, e_bits, tb_idx, nof_layers);
}
int __wrap_srslte_dlsch_encode(srslte_sch_t* q, srslte_pdsch_cfg_t* cfg, uint8_t* data, uint8_t* e_bits)
{
  static int (*f)(srslte_sch_t*, srslte_pdsch_cfg_t*, uint8_t*, uint8_t*);
  if (!f) *(void**)&f = library_symbol("srslte_dlsch_encode");
  return f(q, cfg, data, e_bits);
}
#endif

#define PDSCH_STORAGE (8u << 20) /* sizeof(srslte_pdsch_t): a table of 65536 user pointers and a few dozen members */

static unsigned n_tb;

static double now_us(void)
{
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return 1e6 * (double)t.tv_sec + 1e-3 * (double)t.tv_nsec;
}

typedef struct {
  void*                  pdsch;
  srslte_cell_t          cell;
  srslte_softbuffer_tx_t sb;
  srslte_pdsch_cfg_t     cfg;
  uint8_t*               data;
  cf_t*                  grid;
  size_t                 grid_len;
} tx_t;

static int tx_init(tx_t* t, uint32_t nof_prb, srslte_mod_t mod, int tbs)
{
  memset(t, 0, sizeof(*t));
  t->cell.nof_prb = nof_prb; t->cell.nof_ports = 1; t->cell.id = 1; t->cell.cp = SRSLTE_CP_NORM;
  t->pdsch    = calloc(PDSCH_STORAGE, 1);
  t->data     = malloc((size_t)tbs / 8 + 64);
  t->grid_len = (size_t)14 * 12 * nof_prb;
  t->grid     = calloc(t->grid_len, sizeof(cf_t));
  if (!t->pdsch || !t->data || !t->grid) return -1;
  for (int i = 0; i < tbs / 8; i++) t->data[i] = (uint8_t)((i * 2654435761u) >> 13);
  if (srslte_pdsch_init_enb(t->pdsch, nof_prb) || srslte_pdsch_set_cell(t->pdsch, t->cell) || srslte_pdsch_set_rnti(t->pdsch, 0x1234)) return -2;
  if (srslte_softbuffer_tx_init(&t->sb, nof_prb)) return -3;
  srslte_softbuffer_tx_reset(&t->sb);
  srslte_pdsch_grant_t* g = &t->cfg.grant;
  g->tx_scheme = SRSLTE_TXSCHEME_PORT0;
  g->nof_prb = nof_prb; g->nof_tb = 1; g->nof_layers = 1;
  for (uint32_t n = 0; n < nof_prb; n++) g->prb_idx[0][n] = g->prb_idx[1][n] = true;
  g->tb[0].mod = mod; g->tb[0].tbs = tbs; g->tb[0].enabled = true;
  t->cfg.rnti = 0x1234;
  t->cfg.softbuffers.tx[0] = &t->sb;
  return 0;
}

/* one srslte_pdsch_encode of subframe tti with rv -> its duration in us, or a negative number */
static double tx_encode(tx_t* t, uint32_t tti, int rv)
{
  srslte_dl_sf_cfg_t sf;
  memset(&sf, 0, sizeof(sf));
  sf.tti = tti; sf.cfi = 1;
  t->cfg.grant.tb[0].rv = rv;
  srslte_ra_dl_compute_nof_re(&t->cell, &sf, &t->cfg.grant); /* nof_re, nof_symb_slot and tb[0].nof_bits of this subframe */
  memset(t->grid, 0, t->grid_len * sizeof(cf_t));
  uint8_t*     data[SRSLTE_MAX_CODEWORDS] = {t->data, NULL};
  cf_t*        sym[SRSLTE_MAX_PORTS]      = {t->grid, NULL, NULL, NULL};
  const double t0 = now_us();
  if (srslte_pdsch_encode(t->pdsch, &sf, &t->cfg, data, sym)) return -1.0;
  n_tb++;
  return now_us() - t0;
}

static void tx_free(tx_t* t)
{
  srslte_pdsch_free(t->pdsch);
  srslte_softbuffer_tx_free(&t->sb);
  free(t->pdsch);
  free(t->data);
  free(t->grid);
}

static int cmp(const void* a, const void* b) { return *(const double*)a < *(const double*)b ? -1 : *(const double*)a > *(const double*)b; }

int main(int argc, char** argv)
{
  if (argc != 3) return 2;
  tx_t t;
  if (!strcmp(argv[1], "grid")) {
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 3;
    if (tx_init(&t, 25, SRSLTE_MOD_16QAM, 4008)) return 4;
    for (uint32_t tti = 1; tti <= 2; tti++) {
      for (int rv = 0; rv <= 2; rv += 2) {
        const double us = tx_encode(&t, tti, rv);
        if (us < 0 || fwrite(t.grid, sizeof(cf_t), t.grid_len, out) != t.grid_len) return 5;
        printf("25 PRB tbs 4008 tti %u rv %d: %.0f us\n", tti, rv, us);
      }
    }
    tx_free(&t);
    if (tx_init(&t, 100, SRSLTE_MOD_64QAM, 75376)) return 6;
    for (uint32_t tti = 1; tti <= 2; tti++) {
      const double us = tx_encode(&t, tti, 0);
      if (us < 0 || fwrite(t.grid, sizeof(cf_t), t.grid_len, out) != t.grid_len) return 7;
      printf("100 PRB tbs 75376 tti %u rv 0: %.0f us\n", tti, us);
    }
    tx_free(&t);
    if (fclose(out)) return 8;
  } else if (!strcmp(argv[1], "time")) {
    const int n = atoi(argv[2]);
    if (n < 1 || n > 100000) return 2;
    double* us = malloc(sizeof(double) * (size_t)n);
    if (!us || tx_init(&t, 100, SRSLTE_MOD_64QAM, 75376)) return 6;
    if (tx_encode(&t, 1, 0) < 0) return 7; /* warm-up: tables, streams and the encoder object are made here */
    double sum = 0;
    for (int i = 0; i < n; i++) {
      us[i] = tx_encode(&t, 1, 0);
      if (us[i] < 0) return 7;
      sum += us[i];
    }
    qsort(us, (size_t)n, sizeof(double), cmp);
    printf("us_per_encode %.1f %.1f %.1f\n", sum / n, us[n / 2], us[0]);
    tx_free(&t);
    free(us);
  } else {
    return 2;
  }
  unsigned long long st[4];
  srslte_hip_compat_stats(st);
  printf("transport_blocks=%u\nstats: %llu %llu %llu %llu\n", n_tb, st[0], st[1], st[2], st[3]);
  return 0;
}
