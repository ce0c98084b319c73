/* The reference's own synchronisation over a SEQUENCE of calls (lib/src/phy/sync/sync.c and what it uses, built into
 * oracle/_ref/hip/libsrslte_upper.a and linked against libsrslte_phy_hip.so, whose srslte_dft_* it runs on): one srslte_sync_t per track,
 * kept alive over the whole sequence. tests/test_gpu_sync_track.py and tests/gen_golden_sync_track.py compile this file at run time, as
 * tests/test_gpu_sync.py compiles tests/sync_dropin_driver.c. srslte_sync_t is opaque storage here and only declared functions are called.
 *
 *   sync_track_dropin_driver in out
 *     in:  the header below, then n_calls x n_tracks records { uint32 ops, src, N_id_2, find_offset; int32 N_id_1 }, each followed by
 *          in_stride cf32 when ops has OP_FIND. Records are handled in file order. ops, in this order:
 *            OP_NEW      free the track's object and make it again (the created state)
 *            OP_RESET    srslte_sync_reset
 *            OP_CFO_RST  srslte_sync_cfo_reset
 *            OP_COPY_CFO srslte_sync_copy_cfo from track src
 *            OP_FIND     srslte_sync_set_N_id_2 (and srslte_sync_set_N_id_1 for N_id_1 >= 0), srslte_sync_find
 *     out: for every record with OP_FIND a row of 24 x 4 bytes in the layout of srslte_hip_sync_track_res_t. What has no getter is NaN /
 *          0xffffffff (corr_peak, the two CFO means apart, m0, m1, the trial correlations, the instantaneous estimates, M_norm_avg,
 *          M_ext_avg); frame_type is read off sf_idx (1 or 6: TDD), the only trace the reference leaves of it.
 *   frame_mode 0 / 1: srslte_sync_set_frame_type; 2: detection stays on, as srslte_sync_init leaves it.
 * Exit code 0 on success. */
#include <complex.h>
#include <math.h>
#include <stdbool.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef float complex cf_t;

int      srslte_sync_init(void* q, uint32_t frame_size, uint32_t max_offset, uint32_t fft_size);
void     srslte_sync_free(void* q);
void     srslte_sync_reset(void* q);
void     srslte_sync_cfo_reset(void* q);
void     srslte_sync_copy_cfo(void* q, void* src);
void     srslte_sync_set_frame_type(void* q, int frame_type); /* 0: FDD, 1: TDD */
void     srslte_sync_set_threshold(void* q, float threshold);
void     srslte_sync_sss_en(void* q, bool enabled);
void     srslte_sync_cp_en(void* q, bool enabled);
void     srslte_sync_set_cp(void* q, int cp);
void     srslte_sync_set_cfo_cp_enable(void* q, bool enable, uint32_t nof_symbols);
void     srslte_sync_set_cfo_pss_enable(void* q, bool enable);
void     srslte_sync_set_pss_filt_enable(void* q, bool enable);
void     srslte_sync_set_sss_algorithm(void* q, int alg);
void     srslte_sync_set_em_alpha(void* q, float alpha);
void     srslte_sync_set_cfo_ema_alpha(void* q, float alpha);
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
enum { OP_NEW = 1, OP_RESET = 2, OP_CFO_RST = 4, OP_COPY_CFO = 8, OP_FIND = 16 };

typedef struct {
  int32_t  ret;
  uint32_t peak_pos;
  float    peak_value, corr_peak, cfo_cp, cfo_pss, cfo;
  uint32_t sss_available, sss_detected, m0, m1, sf_idx;
  int32_t  N_id_1, cell_id;
  float    sss_corr;
  int32_t  cp;
  int32_t  frame_type;
  float    sss_corr_trial[2];
  uint32_t nof_calls;
  float    cfo_cp_inst, cfo_pss_inst, M_norm_avg, M_ext_avg;
} row_t;

typedef struct {
  uint32_t fft_size, frame_size, max_offset, cp, detect_cp, sss_en, cfo_cp_enable, cfo_pss_enable, pss_filt_enable, sss_alg, cfo_cp_nsymbols;
  float    threshold, ema_alpha, cfo_ema_alpha;
  uint32_t frame_mode, n_tracks, n_calls, in_stride;
} hdr_t;

static int rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n ? 0 : -1; }

static int setup(void* q, const hdr_t* h)
{
  memset(q, 0, SYNC_STORAGE);
  if (srslte_sync_init(q, h->frame_size, h->max_offset, h->fft_size)) return -1;
  if (h->frame_mode < 2) srslte_sync_set_frame_type(q, (int)h->frame_mode);
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
  if (h->cfo_ema_alpha != 0.f) srslte_sync_set_cfo_ema_alpha(q, h->cfo_ema_alpha);
  srslte_sync_reset(q);
  return 0;
}

int main(int argc, char** argv)
{
  if (argc != 3) return 2;
  FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
  hdr_t h;
  if (!in || !out || rd(in, &h, sizeof(h)) || h.n_tracks == 0 || h.n_tracks > 64) return 4;
  void**    q     = calloc(h.n_tracks, sizeof(void*));
  uint32_t* calls = calloc(h.n_tracks, sizeof(uint32_t));
  cf_t*     buf   = calloc((size_t)h.in_stride + 16, sizeof(cf_t));
  if (!q || !calls || !buf) return 3;
  for (uint32_t t = 0; t < h.n_tracks; t++) {
    q[t] = malloc(SYNC_STORAGE);
    if (!q[t] || setup(q[t], &h)) return 6;
  }
  for (uint32_t c = 0; c < h.n_calls; c++) {
    for (uint32_t t = 0; t < h.n_tracks; t++) {
      uint32_t e[5];
      if (rd(in, e, sizeof(e))) return 5;
      const uint32_t ops = e[0], src = e[1];
      const int32_t  known = (int32_t)e[4];
      if (ops & OP_NEW) {
        srslte_sync_free(q[t]);
        if (setup(q[t], &h)) return 6;
        calls[t] = 0;
      }
      if (ops & OP_RESET) srslte_sync_reset(q[t]);
      if (ops & OP_CFO_RST) srslte_sync_cfo_reset(q[t]);
      if (ops & OP_COPY_CFO) {
        if (src >= h.n_tracks) return 5;
        srslte_sync_copy_cfo(q[t], q[src]);
      }
      if (!(ops & OP_FIND)) continue;
      if (rd(in, buf, (size_t)h.in_stride * sizeof(cf_t))) return 5;
      if (srslte_sync_set_N_id_2(q[t], e[2])) return 6;
      if (known >= 0 && srslte_sync_set_N_id_1(q[t], (uint32_t)known)) return 6;
      row_t    r;
      uint32_t pos = 0;
      r.ret        = srslte_sync_find(q[t], buf, e[3], &pos);
      r.peak_pos   = pos;
      r.peak_value = srslte_sync_get_peak_value(q[t]);
      r.corr_peak = r.cfo_cp = r.cfo_pss = NAN;
      r.cfo                              = srslte_sync_get_cfo(q[t]);
      r.sss_available                    = srslte_sync_sss_available(q[t]) ? 1 : 0;
      r.sss_detected                     = srslte_sync_sss_detected(q[t]) ? 1 : 0;
      r.m0 = r.m1 = 0xffffffffu;
      r.sf_idx    = srslte_sync_get_sf_idx(q[t]);
      r.cell_id   = srslte_sync_get_cell_id(q[t]);
      r.N_id_1    = r.cell_id >= 0 ? r.cell_id / 3 : -1;
      r.sss_corr  = srslte_sync_sss_correlation_peak(q[t]);
      r.cp        = srslte_sync_get_cp(q[t]);
      r.frame_type        = (r.sf_idx == 1 || r.sf_idx == 6) ? 1 : 0;
      r.sss_corr_trial[0] = r.sss_corr_trial[1] = NAN;
      r.nof_calls                               = ++calls[t];
      r.cfo_cp_inst = r.cfo_pss_inst = r.M_norm_avg = r.M_ext_avg = NAN;
      if (fwrite(&r, sizeof(r), 1, out) != 1) return 7;
    }
  }
  for (uint32_t t = 0; t < h.n_tracks; t++) srslte_sync_free(q[t]);
  fclose(in);
  return fclose(out) ? 7 : 0;
}
