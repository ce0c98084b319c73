/* The reference's own PRACH (lib/src/phy/phch/prach.c, built into oracle/_ref/hip/libsrslte_upper.a) as it runs when linked against
 * libsrslte_phy_hip.so: tests/test_gpu_prach.py compiles this file at run time and compares the batched device path with it.
 * It declares the few functions it calls and treats srslte_prach_t as opaque storage of generous size, so it needs no reference header.
 *
 *   prach_dropin_driver gen    nof_prb config_idx root_seq_idx zero_corr_zone in out
 *       in:  uint32 n, then n x (uint32 seq_index, uint32 freq_offset)
 *       out: n x (N_cp + N_seq) cf32, srslte_prach_gen's output
 *   prach_dropin_driver detect nof_prb config_idx root_seq_idx zero_corr_zone detect_factor in out
 *       in:  uint32 n, then n x (uint32 freq_offset, uint32 sig_len, sig_len cf32)
 *       out: per occasion uint32 n_indices, then n_indices x (uint32 index, float t_offset, float peak_to_avg)
 *   prach_dropin_driver opp    6 0 0 0 out
 *       out: srslte_prach_tti_opportunity_config_fdd as bytes [config_idx 64][tti 20][allowed_subframe -1, 0 .. 9]
 *   prach_dropin_driver time   nof_prb config_idx root_seq_idx zero_corr_zone reps
 *       prints the seconds one srslte_prach_detect_offset takes, averaged over reps calls on one generated preamble
 * Exit code 0 on success. */
#define _POSIX_C_SOURCE 199309L
#include <complex.h>
#include <stdbool.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

typedef float complex cf_t;

int  srslte_prach_init(void* p, uint32_t max_N_ifft_ul);
int  srslte_prach_set_cell_(void* p, uint32_t N_ifft_ul, uint32_t config_idx, uint32_t root_seq_index, bool high_speed_flag,
                            uint32_t zero_corr_zone_config, void* tdd_config); /* tdd_config NULL: FDD */
void srslte_prach_set_detect_factor(void* p, float ratio);
int  srslte_prach_gen(void* p, uint32_t seq_index, uint32_t freq_offset, cf_t* signal);
int  srslte_prach_detect_offset(void* p, uint32_t freq_offset, cf_t* signal, uint32_t sig_len, uint32_t* indices, float* t_offsets,
                                float* peak_to_avg, uint32_t* n_indices);
int  srslte_prach_free(void* p);
bool srslte_prach_tti_opportunity_config_fdd(uint32_t config_idx, uint32_t current_tti, int allowed_subframe);
int  srslte_symbol_sz(uint32_t nof_prb);

#define PRACH_STORAGE (4u << 20) /* sizeof(srslte_prach_t) is about 0.9 MB (two [64][839] cf_t tables) */
#define MAX_SIG (2 * 24576 * 12 + 21024 * 12) /* the longest preamble: N_cp + N_seq of format 3 at 1536 */
#define MAX_DET 1024

static int rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n ? 0 : -1; }

int main(int argc, char** argv)
{
  if (argc < 6) return 2;
  const uint32_t nof_prb = (uint32_t)atoi(argv[2]), config_idx = (uint32_t)atoi(argv[3]), rsi = (uint32_t)atoi(argv[4]),
                 zczc    = (uint32_t)atoi(argv[5]);
  void*          p       = calloc(1, PRACH_STORAGE);
  cf_t*          buf     = calloc(MAX_SIG, sizeof(cf_t));
  const int      N_ul    = srslte_symbol_sz(nof_prb);
  if (!p || !buf || N_ul <= 0 || srslte_prach_init(p, (uint32_t)N_ul) || srslte_prach_set_cell_(p, (uint32_t)N_ul, config_idx, rsi, false, zczc, NULL))
    return 3;
  uint32_t n = 0;
  if (argv[1][0] == 'g' && argc == 8) {
    FILE *in = fopen(argv[6], "rb"), *out = fopen(argv[7], "wb");
    if (!in || !out || rd(in, &n, 4)) return 4;
    /* N_cp and N_seq of this configuration: 36.211 Table 5.7.1-1 scaled by N_ifft_ul / 2048 and rounded down, as prach.c does */
    static const uint32_t tcp[4] = {3168, 21024, 6240, 21024}, tseq[4] = {24576, 24576, 49152, 49152};
    const uint32_t        f = config_idx / 16, ncp = tcp[f] * (uint32_t)N_ul / 2048, nseq = tseq[f] * (uint32_t)N_ul / 2048;
    for (uint32_t i = 0; i < n; i++) {
      uint32_t e[2];
      if (rd(in, e, 8) || srslte_prach_gen(p, e[0], e[1], buf)) return 5;
      if (fwrite(buf, sizeof(cf_t), ncp + nseq, out) != ncp + nseq) return 6;
    }
    fclose(in);
    return fclose(out) ? 7 : 0;
  }
  if (argv[1][0] == 'd' && argc == 9) {
    srslte_prach_set_detect_factor(p, (float)atof(argv[6]));
    FILE *in = fopen(argv[7], "rb"), *out = fopen(argv[8], "wb");
    if (!in || !out || rd(in, &n, 4)) return 4;
    static uint32_t idx[MAX_DET];
    static float    toff[MAX_DET], p2a[MAX_DET];
    for (uint32_t i = 0; i < n; i++) {
      uint32_t e[2], nd = 0;
      if (rd(in, e, 8) || e[1] > MAX_SIG || rd(in, buf, (size_t)e[1] * sizeof(cf_t))) return 5;
      if (srslte_prach_detect_offset(p, e[0], buf, e[1], idx, toff, p2a, &nd)) return 6;
      fwrite(&nd, 4, 1, out);
      for (uint32_t k = 0; k < nd; k++) {
        fwrite(&idx[k], 4, 1, out);
        fwrite(&toff[k], 4, 1, out);
        fwrite(&p2a[k], 4, 1, out);
      }
    }
    fclose(in);
    return fclose(out) ? 7 : 0;
  }
  if (argv[1][0] == 'o' && argc == 7) {
    FILE* out = fopen(argv[6], "wb");
    if (!out) return 4;
    for (uint32_t c = 0; c < 64; c++)
      for (uint32_t t = 0; t < 20; t++)
        for (int a = -1; a < 10; a++) fputc(srslte_prach_tti_opportunity_config_fdd(c, t, a) ? 1 : 0, out);
    return fclose(out) ? 7 : 0;
  }
  if (argv[1][0] == 't' && argc == 7) {
    const int reps = atoi(argv[6]);
    static uint32_t idx[MAX_DET];
    uint32_t        nd = 0;
    srslte_prach_gen(p, 0, 0, buf);
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (int r = 0; r < reps; r++) srslte_prach_detect_offset(p, 0, buf + 1, MAX_SIG - 1, idx, NULL, NULL, &nd);
    clock_gettime(CLOCK_MONOTONIC, &t1);
    printf("%.9f\n", ((t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec)) / reps);
    return 0;
  }
  srslte_prach_free(p);
  free(p);
  free(buf);
  return 2;
}
