/* The reference's own PUSCH transmitter and receiver (lib/src/phy/phch/pusch.c in oracle/_ref/hip/libsrslte_upper.a) linked against
 * libsrslte_phy_hip.so, on an identity channel. tests/test_gpu_pusch_decode_dropin.py compiles this file three times at run time; every build
 * counts the entries into srslte_dft_precoding, srslte_demod_soft_demodulate_s and srslte_ulsch_decode with -Wl,--wrap forwarders:
 *   plain        the archive's pusch.o and sch.o serve srslte_pusch_decode: extraction and equaliser on the CPU, one visit of the library for the
 *                transform, one for the demapper, then upstream's UL-SCH with one srslte_tdec_iteration round trip per code block and pass;
 *   -DHOOK_ULSCH the counting forwarder of srslte_ulsch_decode hands the call to the library's (found with dlsym in the library itself) and
 *                falls back to the archive's where that refuses: the parent's best path, three visits per PUSCH;
 *   -DHOOK_PUSCH -Wl,--wrap=srslte_pusch_decode: the call lands in the forwarder below, which hands it to the library's srslte_pusch_decode -
 *                one device call per PUSCH - and falls back to the archive's (__real_) where that answers SRSLTE_ERROR_INVALID_INPUTS.
 * Struct layouts come from this repository's headers (tests/test_pusch_decode_host.py holds them to the reference's).
 *
 *   pusch_decode_dropin_driver run OUT          6 PRB QPSK tbs 600 with a 1-bit ACK and a wideband report; 25 PRB 16QAM tbs 15264, rv 0 (fails: more
 *                                               bits than one transmission carries) then rv 2 on one soft buffer; 100 PRB 64QAM tbs 75376; and the
 *                                               6-PRB case once more on an 8-bit srslte_pusch_t, which no hook serves. OUT: per decode crc, ACK, its
 *                                               valid flag, report, its CRC flag, RI, and the decoded bytes.
 *   pusch_decode_dropin_driver time PRB N       PRB 100 (64QAM tbs 75376), 25 (16QAM tbs 15264: rv 0 then rv 2 per soft buffer) or 6 (QPSK tbs 600,
 *                                               ACK + report): every shape is warmed up, then one host clock around N decodes, each of which ends
 *                                               in its own stream wait. Prints "us_per_decode <mean over the window> window_s <seconds>".
 * `run` prints per decode "dec <i> crc <c> waits <w> dft <n> demod <n> ulsch <n> served <n>": the stream waits inside the call (the library's three
 * wait counters together), the entries counted during it, and whether the library's srslte_pusch_decode served it. Exit code 0 on success. */
#define _GNU_SOURCE
#include "srslte_hip/srslte_compat_pusch.h"
#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

typedef struct { uint8_t* ptr; srslte_uci_value_t uci; } srslte_pusch_data_t; /* pusch.h:84-87 */

int  srslte_pusch_init_ue(srslte_pusch_t* q, uint32_t max_prb);
int  srslte_pusch_init_enb(srslte_pusch_t* q, uint32_t max_prb);
int  srslte_pusch_set_cell(srslte_pusch_t* q, srslte_cell_t cell);
int  srslte_pusch_set_rnti(srslte_pusch_t* q, uint16_t rnti);
void srslte_pusch_free(srslte_pusch_t* q);
int  srslte_pusch_encode(srslte_pusch_t* q, srslte_ul_sf_cfg_t* sf, srslte_pusch_cfg_t* cfg, srslte_pusch_data_t* data, cf_t* sf_symbols);
int  srslte_softbuffer_tx_init(srslte_softbuffer_tx_t* q, uint32_t nof_prb);
void srslte_softbuffer_tx_reset(srslte_softbuffer_tx_t* q);
void srslte_softbuffer_tx_free(srslte_softbuffer_tx_t* q);
int  srslte_softbuffer_rx_init(srslte_softbuffer_rx_t* q, uint32_t nof_prb);
void srslte_softbuffer_rx_reset(srslte_softbuffer_rx_t* q);
void srslte_softbuffer_rx_free(srslte_softbuffer_rx_t* q);
void srslte_hip_compat_stats(unsigned long long out[4]);

static unsigned n_dft, n_demod, n_ulsch;

#if defined(HOOK_ULSCH) || defined(HOOK_PUSCH)
static void* in_library(const char* name)
{
  Dl_info info;
  void*   lib = dladdr((void*)srslte_hip_compat_stats, &info) ? dlopen(info.dli_fname, RTLD_NOW | RTLD_NOLOAD) : NULL;
  void*   f   = lib ? dlsym(lib, name) : NULL;
  if (!f) {
    fprintf(stderr, "%s: not in the library\n", name);
    exit(20);
  }
  return f;
}
#endif

int __real_srslte_dft_precoding(srslte_dft_precoding_t* q, cf_t* input, cf_t* output, uint32_t nof_prb, uint32_t nof_symbols);
int __wrap_srslte_dft_precoding(srslte_dft_precoding_t* q, cf_t* input, cf_t* output, uint32_t nof_prb, uint32_t nof_symbols)
{
  n_dft++;
  return __real_srslte_dft_precoding(q, input, output, nof_prb, nof_symbols);
}
int __real_srslte_demod_soft_demodulate_s(srslte_mod_t modulation, const cf_t* symbols, short* llr, int nsymbols);
int __wrap_srslte_demod_soft_demodulate_s(srslte_mod_t modulation, const cf_t* symbols, short* llr, int nsymbols)
{
  n_demod++;
  return __real_srslte_demod_soft_demodulate_s(modulation, symbols, llr, nsymbols);
}
int __real_srslte_ulsch_decode(srslte_sch_t* q, srslte_pusch_cfg_t* cfg, int16_t* q_bits, int16_t* g_bits, uint8_t* c_seq, uint8_t* data, srslte_uci_value_t* uci);
int __wrap_srslte_ulsch_decode(srslte_sch_t* q, srslte_pusch_cfg_t* cfg, int16_t* q_bits, int16_t* g_bits, uint8_t* c_seq, uint8_t* data, srslte_uci_value_t* uci)
{
  n_ulsch++;
#ifdef HOOK_ULSCH
  static int (*f)(srslte_sch_t*, srslte_pusch_cfg_t*, int16_t*, int16_t*, uint8_t*, uint8_t*, srslte_uci_value_t*);
  if (!f) *(void**)&f = in_library("srslte_ulsch_decode");
  const int r = f(q, cfg, q_bits, g_bits, c_seq, data, uci);
  if (r != SRSLTE_ERROR_INVALID_INPUTS) return r;
#endif
  return __real_srslte_ulsch_decode(q, cfg, q_bits, g_bits, c_seq, data, uci);
}
#ifdef HOOK_PUSCH
int __real_srslte_pusch_decode(srslte_pusch_t* q, srslte_ul_sf_cfg_t* sf, srslte_pusch_cfg_t* cfg, srslte_chest_ul_res_t* channel, cf_t* sf_symbols, srslte_pusch_res_t* out);
int __wrap_srslte_pusch_decode(srslte_pusch_t* q, srslte_ul_sf_cfg_t* sf, srslte_pusch_cfg_t* cfg, srslte_chest_ul_res_t* channel, cf_t* sf_symbols, srslte_pusch_res_t* out)
{
  static int (*f)(srslte_pusch_t*, srslte_ul_sf_cfg_t*, srslte_pusch_cfg_t*, srslte_chest_ul_res_t*, cf_t*, srslte_pusch_res_t*);
  if (!f) *(void**)&f = in_library("srslte_pusch_decode");
  const int r = f(q, sf, cfg, channel, sf_symbols, out);
  if (r != SRSLTE_ERROR_INVALID_INPUTS || !q || !cfg || !sf_symbols || !out) return r; /* upstream's own use of the code: handed on */
  return __real_srslte_pusch_decode(q, sf, cfg, channel, sf_symbols, out);
}
#endif

static unsigned n_dec;

static double now_us(void)
{
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return 1e6 * (double)t.tv_sec + 1e-3 * (double)t.tv_nsec;
}

static unsigned long long waits_now(unsigned long long* served)
{
  unsigned long long st[4], ul[2], pu[2];
  srslte_hip_compat_stats(st);
  srslte_hip_compat_stats_ul(ul);
  srslte_hip_compat_stats_pusch(pu);
  if (served) *served = pu[0];
  return st[0] + ul[1] + pu[1];
}

typedef struct {
  srslte_pusch_t *       ue, *enb;
  srslte_cell_t          cell;
  srslte_softbuffer_tx_t sb_tx;
  srslte_softbuffer_rx_t sb_rx;
  srslte_pusch_cfg_t     cfg;
  uint8_t *              data, *out;
  cf_t *                 grid, *grid2, *ce;
  size_t                 grid_len;
  int                    tbs;
} link_t;

static int link_init(link_t* t, uint32_t nof_prb, srslte_mod_t mod, int tbs)
{
  memset(t, 0, sizeof(*t));
  t->cell.nof_prb = nof_prb; t->cell.nof_ports = 1; t->cell.id = 1; t->cell.cp = SRSLTE_CP_NORM;
  t->tbs      = tbs;
  t->ue       = calloc(1, sizeof(srslte_pusch_t));
  t->enb      = calloc(1, sizeof(srslte_pusch_t));
  t->data     = malloc((size_t)tbs / 8 + 64);
  t->out      = malloc((size_t)tbs / 8 + 1024);
  t->grid_len = (size_t)14 * 12 * nof_prb;
  t->grid     = calloc(t->grid_len, sizeof(cf_t));
  t->grid2    = calloc(t->grid_len, sizeof(cf_t));
  t->ce       = calloc(t->grid_len, sizeof(cf_t));
  if (!t->ue || !t->enb || !t->data || !t->out || !t->grid || !t->grid2 || !t->ce) return -1;
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

/* one subframe through srslte_pusch_encode into grid; < 0 on failure */
static int link_encode(link_t* t, cf_t* grid, uint32_t tti, int rv, const srslte_uci_value_t* uci)
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
  memset(grid, 0, t->grid_len * sizeof(cf_t));
  return srslte_pusch_encode(t->ue, &sf, &cfg, &d, grid);
}

/* one srslte_pusch_decode of grid; nonzero: the call failed */
static int link_decode(link_t* t, cf_t* grid, uint32_t tti, int rv, srslte_pusch_res_t* res)
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
  if (srslte_pusch_decode(t->enb, &sf, &cfg, &ch, grid, res)) return -1;
  n_dec++;
  return 0;
}

static void link_free(link_t* t)
{
  srslte_pusch_free(t->ue);
  srslte_pusch_free(t->enb);
  srslte_softbuffer_tx_free(&t->sb_tx);
  srslte_softbuffer_rx_free(&t->sb_rx);
  free(t->ue); free(t->enb); free(t->data); free(t->out); free(t->grid); free(t->grid2); free(t->ce);
}

/* decode with the counters around it, print them, append the record */
static int decode_recorded(FILE* out, const char* what, link_t* t, uint32_t tti, int rv, srslte_pusch_res_t* r)
{
  unsigned long long s0, s1;
  const unsigned long long w0 = waits_now(&s0);
  const unsigned           d0 = n_dft, m0 = n_demod, u0 = n_ulsch;
  if (link_decode(t, t->grid, tti, rv, r)) return -1;
  const unsigned long long w1 = waits_now(&s1);
  printf("dec %u crc %d waits %llu dft %u demod %u ulsch %u served %llu  (%s)\n", n_dec, (int)r->crc, w1 - w0, n_dft - d0, n_demod - m0, n_ulsch - u0, s1 - s0, what);
  const uint8_t head[8] = {(uint8_t)r->crc, r->uci.ack.ack_value[0], r->uci.cqi.wideband.wideband_cqi, (uint8_t)r->uci.cqi.data_crc, r->uci.ri, (uint8_t)r->uci.ack.valid, 0, 0};
  return fwrite(head, 1, 8, out) == 8 && fwrite(t->out, 1, (size_t)t->tbs / 8, out) == (size_t)t->tbs / 8 ? 0 : -1;
}

static void with_ack_and_report(link_t* t, srslte_uci_value_t* uci)
{
  t->cfg.uci_cfg.ack[0].nof_acks = 1;
  t->cfg.uci_cfg.cqi.data_enable = true;
  t->cfg.uci_cfg.cqi.type        = SRSLTE_CQI_TYPE_WIDEBAND;
  memset(uci, 0, sizeof(*uci));
  uci->ack.ack_value[0]          = 1;
  uci->cqi.wideband.wideband_cqi = 11;
}

int main(int argc, char** argv)
{
  link_t             t;
  srslte_pusch_res_t r;
  srslte_uci_value_t uci;
  if (argc == 3 && !strcmp(argv[1], "run")) {
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 3;
    for (int l8 = 0; l8 < 2; l8++) { /* 6 PRB QPSK with a 1-bit ACK and a wideband report: first, and last on an 8-bit object */
      if (l8) {
        /* 25 PRB 16QAM, rv 0 then rv 2 on one soft buffer: 15264 bits (C = 3, K = 5120) do not fit the 14400 of one transmission */
        if (link_init(&t, 25, SRSLTE_MOD_16QAM, 15264)) return 8;
        for (int rv = 0; rv <= 2; rv += 2) {
          if (link_encode(&t, t.grid, 2, rv, NULL) < 0) return 9;
          if (decode_recorded(out, rv ? "25 PRB 16QAM tbs 15264 rv 2" : "25 PRB 16QAM tbs 15264 rv 0", &t, 2, rv, &r)) return 10;
          if (r.crc != (rv == 2) || (rv == 2 && memcmp(t.out, t.data, 15264 / 8))) return 11;
        }
        link_free(&t);
        if (link_init(&t, 100, SRSLTE_MOD_64QAM, 75376)) return 12;
        if (link_encode(&t, t.grid, 3, 0, NULL) < 0) return 13;
        if (decode_recorded(out, "100 PRB 64QAM tbs 75376", &t, 3, 0, &r)) return 14;
        if (!r.crc || memcmp(t.out, t.data, 75376 / 8)) return 15;
        link_free(&t);
      }
      if (link_init(&t, 6, SRSLTE_MOD_QPSK, 600)) return 4;
      with_ack_and_report(&t, &uci);
      if (l8) {
        t.enb->llr_is_8bit = t.enb->ul_sch.llr_is_8bit = true;
        /* upstream fills q->q with nof_bits int8 LLRs and reads nof_bits int16 from it (pusch.c:483,:503): the second half is whatever malloc
         * left there. Zeroed, so that what the 8-bit object decodes is a function of the input in every build */
        memset(t.enb->q, 0, sizeof(int16_t) * t.enb->max_re * 6);
        memset(t.enb->g, 0, sizeof(int16_t) * t.enb->max_re * 6);
      }
      if (link_encode(&t, t.grid, 1, 0, &uci) < 0) return 5;
      if (decode_recorded(out, l8 ? "6 PRB QPSK tbs 600 ACK + CQI, 8-bit object" : "6 PRB QPSK tbs 600 ACK + CQI", &t, 1, 0, &r)) return 6;
      /* the 8-bit object is held to nothing here: upstream reads its int8 LLRs through an int16_t* (sch.c:1018-1030); the builds must agree on it */
      if (!l8 && (!r.crc || r.uci.ack.ack_value[0] != 1 || !r.uci.ack.valid || r.uci.cqi.wideband.wideband_cqi != 11 || memcmp(t.out, t.data, 600 / 8))) return 7;
      link_free(&t);
    }
    if (fclose(out)) return 16;
  } else if (argc == 4 && !strcmp(argv[1], "time")) {
    const int prb = atoi(argv[2]), n = atoi(argv[3]);
    if (n < 2 || n > 1000000 || (prb != 100 && prb != 25 && prb != 6)) return 2;
    if (link_init(&t, (uint32_t)prb, prb == 100 ? SRSLTE_MOD_64QAM : prb == 25 ? SRSLTE_MOD_16QAM : SRSLTE_MOD_QPSK, prb == 100 ? 75376 : prb == 25 ? 15264 : 600)) return 12;
    if (prb == 6) with_ack_and_report(&t, &uci);
    if (link_encode(&t, t.grid, 3, 0, prb == 6 ? &uci : NULL) < 0) return 13;
    if (prb == 25 && link_encode(&t, t.grid2, 3, 2, NULL) < 0) return 13;
    double t0 = 0;
    for (int i = -20; i < n; i++) { /* 20 warm-up decodes: tables, streams and the device object are made in the first */
      if (i == 0) t0 = now_us();
      const int second = prb == 25 && (i & 1); /* rv 0 fails and leaves its soft values, rv 2 combines into them and decodes */
      if (!second) srslte_softbuffer_rx_reset(&t.sb_rx);
      if (link_decode(&t, second ? t.grid2 : t.grid, 3, second ? 2 : 0, &r) || r.crc != (prb != 25 || second)) return 14;
    }
    const double w = now_us() - t0;
    printf("us_per_decode %.2f window_s %.3f\n", w / n, w * 1e-6);
    link_free(&t);
  } else {
    return 2;
  }
  unsigned long long st[4], ul[2], pu[2];
  srslte_hip_compat_stats(st);
  srslte_hip_compat_stats_ul(ul);
  srslte_hip_compat_stats_pusch(pu);
  printf("decodes=%u\nstats: %llu %llu %llu %llu\nstats_ul: %llu %llu\nstats_pusch: %llu %llu\n", n_dec, st[0], st[1], st[2], st[3], ul[0], ul[1], pu[0], pu[1]);
  return 0;
}
