/* The reference's own synchronisation (lib/src/phy/sync/sync.c, pss.c, sss.c, find_sss.c, cfo.c, cp.c, built into
 * oracle/_ref/hip/libsrslte_upper.a) as it runs when linked against libsrslte_phy_hip.so, whose srslte_dft_* it uses:
 * tests/test_gpu_sync.py compiles this file at run time and compares the batched device path with it.
 * It declares the few functions it calls and treats srslte_sync_t as opaque storage of generous size, so it needs no reference header; what
 * has no getter (pss.peak_value, the two CFO means apart, m0, m1) is written as NaN / 0xffffffff, and the SSS threshold, which is set on a
 * member of the struct, stays at the 0 of srslte_sss_init.
 *
 *   sync_dropin_driver find in out
 *       in:  uint32 fft_size, frame_size, max_offset, cp, detect_cp, sss_en, cfo_cp_enable, cfo_pss_enable, pss_filt_enable, sss_alg,
 *            cfo_cp_nsymbols; float threshold, ema_alpha; uint32 n, in_stride; then n x (uint32 N_id_2, uint32 find_offset, int32 N_id_1,
 *            in_stride cf32)
 *       out: n rows of 16 x 4 bytes in the layout of srslte_hip_sync_res_t
 *       for every item: srslte_sync_init, the setters, srslte_sync_reset, one srslte_sync_find, srslte_sync_free
 *   sync_dropin_driver time fft_size frame_size max_offset reps
 *       prints the seconds one srslte_sync_find takes (the ue_sync find setting, noise input), averaged over reps calls
 * Exit code 0 on success. */
#define _POSIX_C_SOURCE 199309L
#include <complex.h>
#include <math.h>
#include <stdbool.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

typedef float complex cf_t;

int      srslte_sync_init(void* q, uint32_t frame_size, uint32_t max_offset, uint32_t fft_size);
void     srslte_sync_free(void* q);
void     srslte_sync_reset(void* q);
void     srslte_sync_set_frame_type(void* q, int frame_type); /* 0: FDD */
void     srslte_sync_set_threshold(void* q, float threshold);
void     srslte_sync_sss_en(void* q, bool enabled);
void     srslte_sync_cp_en(void* q, bool enabled);
void     srslte_sync_set_cp(void* q, int cp);
void     srslte_sync_set_cfo_cp_enable(void* q, bool enable, uint32_t nof_symbols);
void     srslte_sync_set_cfo_pss_enable(void* q, bool enable);
void     srslte_sync_set_pss_filt_enable(void* q, bool enable);
void     srslte_sync_set_sss_algorithm(void* q, int alg);
void     srslte_sync_set_em_alpha(void* q, float alpha);
int      srslte_sync_set_N_id_2(void* q, uint32_t N_id_2);
int      srslte_sync_set_N_id_1(void* q, uint32_t N_id_1);
int      srslte_sync_find(void* q, const cf_t* input, uint32_t find_offset, uint32_t* peak_position);
float    srslte_sync_get_cfo(void* q);
float    srslte_sync_get_peak_value(void* q);
int      srslte_sync_get_cell_id(void* q);
uint32_t srslte_sync_get_sf_idx(void* q);
int      srslte_sync_get_cp(void* q);
bool     srslte_sync_sss_detected(void* q);
bool     srslte_sync_sss_available(void* q);
float    srslte_sync_sss_correlation_peak(void* q);

#define SYNC_STORAGE (8u << 20) /* sizeof(srslte_sync_t) is a few hundred KB (the pss objects' symbol buffers) */

typedef struct {
  int32_t  ret;
  uint32_t peak_pos;
  float    peak_value, corr_peak, cfo_cp, cfo_pss, cfo;
  uint32_t sss_available, sss_detected, m0, m1, sf_idx;
  int32_t  N_id_1, cell_id;
  float    sss_corr;
  int32_t  cp;
} row_t;

typedef struct {
  uint32_t fft_size, frame_size, max_offset, cp, detect_cp, sss_en, cfo_cp_enable, cfo_pss_enable, pss_filt_enable, sss_alg, cfo_cp_nsymbols;
  float    threshold, ema_alpha;
  uint32_t n, in_stride;
} hdr_t;

static int rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n ? 0 : -1; }

static int setup(void* q, const hdr_t* h)
{
  memset(q, 0, SYNC_STORAGE);
  if (srslte_sync_init(q, h->frame_size, h->max_offset, h->fft_size)) return -1;
  srslte_sync_set_frame_type(q, 0);
  srslte_sync_set_cp(q, (int)h->cp);
  srslte_sync_cp_en(q, h->detect_cp != 0);
  srslte_sync_sss_en(q, h->sss_en != 0);
  srslte_sync_set_cfo_cp_enable(q, h->cfo_cp_enable != 0, h->cfo_cp_nsymbols);
  srslte_sync_set_cfo_pss_enable(q, h->cfo_pss_enable != 0);
  srslte_sync_set_pss_filt_enable(q, h->pss_filt_enable != 0);
  static const int alg[3] = {0, 2, 1}; /* sss_alg_t: SSS_DIFF 0, SSS_PARTIAL_3 2, SSS_FULL 1 */
  srslte_sync_set_sss_algorithm(q, alg[h->sss_alg % 3]);
  srslte_sync_set_threshold(q, h->threshold);
  if (h->ema_alpha != 0.f) srslte_sync_set_em_alpha(q, h->ema_alpha);
  return 0;
}

int main(int argc, char** argv)
{
  if (argc < 4) return 2;
  void* q = malloc(SYNC_STORAGE);
  if (!q) return 3;
  if (argv[1][0] == 'f' && argc == 4) {
    FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    hdr_t h;
    if (!in || !out || rd(in, &h, sizeof(h))) return 4;
    cf_t* buf = calloc((size_t)h.in_stride + 16, sizeof(cf_t));
    if (!buf) return 3;
    for (uint32_t i = 0; i < h.n; i++) {
      uint32_t e[3];
      if (rd(in, e, 12) || rd(in, buf, (size_t)h.in_stride * sizeof(cf_t))) return 5;
      const int32_t known = (int32_t)e[2];
      if (setup(q, &h) || srslte_sync_set_N_id_2(q, e[0])) return 6;
      if (known >= 0 && srslte_sync_set_N_id_1(q, (uint32_t)known)) return 6;
      srslte_sync_reset(q);
      row_t    r;
      uint32_t pos = 0;
      r.ret        = srslte_sync_find(q, buf, e[1], &pos);
      r.peak_pos   = pos;
      r.peak_value = srslte_sync_get_peak_value(q);
      r.corr_peak = r.cfo_cp = r.cfo_pss = NAN;
      r.cfo                              = srslte_sync_get_cfo(q);
      r.sss_available                    = srslte_sync_sss_available(q) ? 1 : 0;
      r.sss_detected                     = srslte_sync_sss_detected(q) ? 1 : 0;
      r.m0 = r.m1 = 0xffffffffu;
      r.sf_idx    = srslte_sync_get_sf_idx(q);
      r.cell_id   = srslte_sync_get_cell_id(q);
      r.N_id_1    = r.cell_id >= 0 ? r.cell_id / 3 : -1;
      r.sss_corr  = srslte_sync_sss_correlation_peak(q);
      r.cp        = srslte_sync_get_cp(q);
      if (fwrite(&r, sizeof(r), 1, out) != 1) return 7;
      srslte_sync_free(q);
    }
    fclose(in);
    return fclose(out) ? 7 : 0;
  }
  if (argv[1][0] == 't' && argc == 6) {
    hdr_t h;
    memset(&h, 0, sizeof(h));
    h.fft_size = (uint32_t)atoi(argv[2]), h.frame_size = (uint32_t)atoi(argv[3]), h.max_offset = (uint32_t)atoi(argv[4]);
    h.detect_cp = 0, h.sss_en = 1, h.cfo_cp_enable = 1, h.cfo_pss_enable = 1, h.pss_filt_enable = 1, h.sss_alg = 1, h.cfo_cp_nsymbols = 14;
    h.threshold = 2.0f, h.ema_alpha = 1.0f;
    const int    reps = atoi(argv[5]);
    const size_t len  = (size_t)h.frame_size + h.fft_size + 16;
    cf_t*        buf  = calloc(len, sizeof(cf_t));
    if (!buf || reps < 1 || setup(q, &h) || srslte_sync_set_N_id_2(q, 0)) return 3;
    uint32_t s = 1;
    for (size_t i = 0; i < len; i++) {
      s = s * 1664525u + 1013904223u;
      const float a = (float)(s >> 8) / 16777216.f - 0.5f;
      s = s * 1664525u + 1013904223u;
      buf[i] = a + I * ((float)(s >> 8) / 16777216.f - 0.5f);
    }
    uint32_t        pos = 0;
    const uint32_t  fo  = h.max_offset < h.fft_size ? h.frame_size / 2 : 0;
    struct timespec t0, t1;
    srslte_sync_find(q, buf, fo, &pos);
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (int r = 0; r < reps; r++) srslte_sync_find(q, buf, fo, &pos);
    clock_gettime(CLOCK_MONOTONIC, &t1);
    printf("%.9f\n", ((t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec)) / reps);
    srslte_sync_free(q);
    return 0;
  }
  return 2;
}
