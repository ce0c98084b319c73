/* The reference's own NB-IoT synchronisation (lib/src/phy/sync/sync_nbiot.c, npss.c, nsss.c, cp.c and utils/convolution.c, built into
 * oracle/_ref/hip/libsrslte_upper.a) as it runs when linked against libsrslte_phy_hip.so, whose srslte_dft_* it uses (the 5348-point and
 * frame_size + 1508-point transforms take that library's direct path): tests/test_gpu_nbiot_sync.py and tests/gen_golden_nbiot_sync.py compile
 * this file at run time and compare the batched device path with it.
 * It declares the few functions it calls and treats the reference's structs as opaque, zeroed storage of generous size (srslte_sync_nbiot_init
 * leaves several members unset), so it needs no reference header. What has no getter (the average at the peak, the call's own CFO estimate,
 * the NSSS peak position) is written as NaN / 0xffffffff; the NSSS threshold is a struct member and stays at srslte_nsss_synch_init's 2.0.
 *
 *   nbiot_sync_dropin_driver npss in out
 *       in:  uint32 frame_size, max_offset, cfo_enable, n_tracks, n_ops, in_stride; float threshold, npss_ema_alpha, cfo_ema_alpha (0: the
 *            reference's default is left alone); then n_ops x (uint32 op, uint32 track, ...):
 *              op 1 find:    uint32 find_offset, in_stride cf32   -> one row out
 *              op 2 reset:   srslte_sync_nbiot_reset and srslte_sync_nbiot_set_cfo(0)
 *              op 3 set_cfo: float cfo
 *       out: one row of 8 x 4 bytes in the layout of srslte_hip_nbiot_npss_res_t per find, in order
 *       one srslte_sync_nbiot_t per track, made at the start
 *   nbiot_sync_dropin_driver nsss in out
 *       in:  uint32 n, in_stride; then n x (int32 cell_id (-1: unknown), in_stride cf32)
 *       out: n rows of 8 x 4 bytes in the layout of srslte_hip_nbiot_nsss_res_t (cell_id: what the reference leaves in its argument, -1
 *            when that is still "unknown")
 *   nbiot_sync_dropin_driver seq out -
 *       out: cf32: srslte_npss_generate [121], srslte_nsss_generate [528] of cell ids 0, 125, 126, 377, 503, and the first 64 samples of
 *            srslte_npss_corr_init's replica
 *   nbiot_sync_dropin_driver time_npss frame_size reps | time_nsss cell_id reps
 *       prints the seconds one srslte_sync_nbiot_find / srslte_nsss_sync_find takes on noise, averaged over reps calls
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

int   srslte_sync_nbiot_init(void* q, uint32_t frame_size, uint32_t max_offset, uint32_t fft_size);
void  srslte_sync_nbiot_free(void* q);
int   srslte_sync_nbiot_find(void* q, cf_t* input, uint32_t find_offset, uint32_t* peak_position);
void  srslte_sync_nbiot_set_threshold(void* q, float threshold);
void  srslte_sync_nbiot_set_cfo_enable(void* q, bool enable);
void  srslte_sync_nbiot_set_cfo_ema_alpha(void* q, float alpha);
void  srslte_sync_nbiot_set_npss_ema_alpha(void* q, float alpha);
void  srslte_sync_nbiot_set_cfo(void* q, float cfo);
float srslte_sync_nbiot_get_cfo(void* q);
float srslte_sync_nbiot_get_peak_value(void* q);
void  srslte_sync_nbiot_reset(void* q);
int   srslte_nsss_synch_init(void* q, uint32_t input_size, uint32_t fft_size);
void  srslte_nsss_synch_free(void* q);
int   srslte_nsss_sync_find(void* q, cf_t* input, float* corr_peak_value, uint32_t* cell_id, uint32_t* sfn_partial);
int   srslte_npss_generate(cf_t* signal);
void  srslte_nsss_generate(cf_t* signal, uint32_t cell_id);
int   srslte_npss_corr_init(cf_t* npss_signal_time, uint32_t fft_size, uint32_t frame_size);

#define STORAGE (1u << 20) /* sizeof(srslte_sync_nbiot_t) is some 20 KB: two srslte_nsss_synch_t-sized tables of 504 pointers and floats */
#define CELL_ID_UNKNOWN 1000u

typedef struct {
  int32_t  ret;
  uint32_t peak_pos;
  float    peak_value, corr_peak, cfo, mean_cfo;
  uint32_t reserved[2];
} npss_row_t;

typedef struct {
  int32_t  found, cell_id;
  float    peak_value;
  uint32_t peak_pos, sfn_partial, reserved[3];
} nsss_row_t;

typedef struct {
  uint32_t frame_size, max_offset, cfo_enable, n_tracks, n_ops, in_stride;
  float    threshold, npss_ema_alpha, cfo_ema_alpha;
} npss_hdr_t;

static int rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n ? 0 : -1; }

static void* make_sync(const npss_hdr_t* h)
{
  void* q = calloc(1, STORAGE);
  if (!q || srslte_sync_nbiot_init(q, h->frame_size, h->max_offset, 128)) return NULL;
  srslte_sync_nbiot_set_cfo_enable(q, h->cfo_enable != 0);
  if (h->threshold != 0.f) srslte_sync_nbiot_set_threshold(q, h->threshold);
  if (h->npss_ema_alpha != 0.f) srslte_sync_nbiot_set_npss_ema_alpha(q, h->npss_ema_alpha);
  if (h->cfo_ema_alpha != 0.f) srslte_sync_nbiot_set_cfo_ema_alpha(q, h->cfo_ema_alpha);
  return q;
}

static void noise(cf_t* buf, size_t len)
{
  uint32_t s = 1;
  for (size_t i = 0; i < len; i++) {
    s = s * 1664525u + 1013904223u;
    const float a = (float)(s >> 8) / 16777216.f - 0.5f;
    s = s * 1664525u + 1013904223u;
    buf[i] = a + I * ((float)(s >> 8) / 16777216.f - 0.5f);
  }
}

static double now(void)
{
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return t.tv_sec + 1e-9 * t.tv_nsec;
}

int main(int argc, char** argv)
{
  if (argc < 4) return 2;
  if (!strcmp(argv[1], "npss")) {
    FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    npss_hdr_t h;
    if (!in || !out || rd(in, &h, sizeof(h)) || h.n_tracks == 0 || h.n_tracks > 64) return 4;
    void* q[64];
    for (uint32_t t = 0; t < h.n_tracks; t++)
      if (!(q[t] = make_sync(&h))) return 6;
    /* the reference reads its corrected copy up to find_offset + frame_size (+ 128 in the short branch) */
    cf_t* buf = calloc((size_t)h.in_stride + 256, sizeof(cf_t));
    if (!buf) return 3;
    for (uint32_t i = 0; i < h.n_ops; i++) {
      uint32_t e[2];
      if (rd(in, e, 8) || e[1] >= h.n_tracks) return 5;
      if (e[0] == 1) {
        uint32_t fo;
        if (rd(in, &fo, 4) || rd(in, buf, (size_t)h.in_stride * sizeof(cf_t))) return 5;
        npss_row_t r;
        uint32_t   pos = 0;
        memset(&r, 0, sizeof(r));
        r.ret        = srslte_sync_nbiot_find(q[e[1]], buf, fo, &pos);
        r.peak_pos   = pos;
        r.peak_value = srslte_sync_nbiot_get_peak_value(q[e[1]]);
        r.corr_peak = r.cfo = NAN;
        r.mean_cfo          = srslte_sync_nbiot_get_cfo(q[e[1]]);
        if (fwrite(&r, sizeof(r), 1, out) != 1) return 7;
      } else if (e[0] == 2) {
        srslte_sync_nbiot_reset(q[e[1]]);
        srslte_sync_nbiot_set_cfo(q[e[1]], 0.f);
      } else if (e[0] == 3) {
        float cfo;
        if (rd(in, &cfo, 4)) return 5;
        srslte_sync_nbiot_set_cfo(q[e[1]], cfo);
      } else {
        return 5;
      }
    }
    for (uint32_t t = 0; t < h.n_tracks; t++) srslte_sync_nbiot_free(q[t]);
    fclose(in);
    return fclose(out) ? 7 : 0;
  }
  if (!strcmp(argv[1], "nsss")) {
    FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    uint32_t hd[2];
    if (!in || !out || rd(in, hd, 8) || hd[1] < 3840) return 4;
    void* q   = calloc(1, STORAGE);
    cf_t* buf = calloc((size_t)hd[1], sizeof(cf_t));
    if (!q || !buf || srslte_nsss_synch_init(q, 3840, 128)) return 6;
    for (uint32_t i = 0; i < hd[0]; i++) {
      int32_t want;
      if (rd(in, &want, 4) || rd(in, buf, (size_t)hd[1] * sizeof(cf_t))) return 5;
      nsss_row_t r;
      uint32_t   id = want < 0 ? CELL_ID_UNKNOWN : (uint32_t)want, sfn = 77;
      float      pk = NAN;
      memset(&r, 0, sizeof(r));
      r.found       = srslte_nsss_sync_find(q, buf, &pk, &id, &sfn) == 0 ? 1 : 0;
      r.cell_id     = id == CELL_ID_UNKNOWN ? -1 : (int32_t)id;
      r.peak_value  = pk;
      r.peak_pos    = 0xffffffffu;
      r.sfn_partial = sfn;
      if (fwrite(&r, sizeof(r), 1, out) != 1) return 7;
    }
    srslte_nsss_synch_free(q);
    fclose(in);
    return fclose(out) ? 7 : 0;
  }
  if (!strcmp(argv[1], "seq")) {
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 4;
    static const uint32_t ids[5] = {0, 125, 126, 377, 503};
    cf_t                  v[528];
    memset(v, 0, sizeof(v));
    srslte_npss_generate(v);
    if (fwrite(v, sizeof(cf_t), 121, out) != 121) return 7;
    for (int i = 0; i < 5; i++) {
      memset(v, 0, sizeof(v));
      srslte_nsss_generate(v, ids[i]);
      if (fwrite(v, sizeof(cf_t), 528, out) != 528) return 7;
    }
    cf_t* h = calloc(128 + 1920 + 16, sizeof(cf_t)); /* srslte_npss_corr_init clears fft_size + frame_size samples */
    if (!h || srslte_npss_corr_init(h, 128, 1920)) return 6;
    if (fwrite(h, sizeof(cf_t), 64, out) != 64) return 7;
    return fclose(out) ? 7 : 0;
  }
  if (!strcmp(argv[1], "time_npss")) {
    npss_hdr_t h;
    memset(&h, 0, sizeof(h));
    h.frame_size = (uint32_t)atoi(argv[2]), h.max_offset = 128, h.cfo_enable = 1;
    const int reps = atoi(argv[3]);
    void*     q    = make_sync(&h);
    cf_t*     buf  = calloc((size_t)h.frame_size + 256, sizeof(cf_t));
    if (!q || !buf || reps < 1) return 3;
    noise(buf, h.frame_size);
    uint32_t pos = 0;
    srslte_sync_nbiot_find(q, buf, 0, &pos);
    const double t0 = now();
    for (int r = 0; r < reps; r++) srslte_sync_nbiot_find(q, buf, 0, &pos);
    printf("%.9f\n", (now() - t0) / reps);
    return 0;
  }
  if (!strcmp(argv[1], "time_nsss")) {
    const int want = atoi(argv[2]), reps = atoi(argv[3]);
    void*     q    = calloc(1, STORAGE);
    cf_t*     buf  = calloc(3840, sizeof(cf_t));
    if (!q || !buf || reps < 1 || srslte_nsss_synch_init(q, 3840, 128)) return 3;
    noise(buf, 3840);
    float    pk;
    uint32_t id = want < 0 ? CELL_ID_UNKNOWN : (uint32_t)want, sfn;
    srslte_nsss_sync_find(q, buf, &pk, &id, &sfn);
    const double t0 = now();
    for (int r = 0; r < reps; r++) {
      id = want < 0 ? CELL_ID_UNKNOWN : (uint32_t)want;
      srslte_nsss_sync_find(q, buf, &pk, &id, &sfn);
    }
    printf("%.9f\n", (now() - t0) / reps);
    return 0;
  }
  return 2;
}
