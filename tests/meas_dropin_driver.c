/* The reference's own neighbour-cell measurement (lib/src/phy/sync/refsignal_dl_sync.c, built into oracle/_ref/hip/libsrslte_upper.a) as it
 * runs when linked against libsrslte_phy_hip.so, whose srslte_dft_* and OFDM modulator it uses: tests/test_gpu_meas.py compiles this file at
 * run time and compares the batched device path with it.
 * It declares the few functions it calls and treats srslte_refsignal_dl_sync_t as opaque storage, so it needs no reference header. The
 * object has no getters; its results are its last six members (bool found; float rsrp_dBfs, rssi_dBfs, rsrq_dB, cfo_Hz; uint32_t peak_index:
 * 24 bytes behind pointer-aligned members, so nothing pads them). srslte_refsignal_dl_sync_init begins with bzero(q, sizeof(*q)): the
 * storage is filled with 0xA5 before, and the last byte that init changed marks the end of the struct. What the object does not keep
 * (peak_value, rms_avg, the linear figures, sf_idx, nof_sf) is written as NaN / 0xffffffff.
 *
 *   meas_dropin_driver run in out
 *       in:  uint32 nof_prb, nof_sf, n, in_stride; then n x (uint32 cell_id, in_stride cf32)
 *       out: n rows of 16 x 4 bytes in the layout of srslte_hip_meas_res_t
 *       for every row: srslte_refsignal_dl_sync_init, _set_cell, one _run over nof_sf sf_len samples, _free
 *   meas_dropin_driver time nof_prb nof_sf reps
 *       prints the seconds one set_cell and one run take (noise input), averaged over reps calls
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
typedef struct { /* srslte_cell_t (phy_common.h:195-212) */
  uint32_t nof_prb, nof_ports, id;
  int      cp, phich_length, phich_resources, frame_type;
} cell_t;

int  srslte_refsignal_dl_sync_init(void* q);
int  srslte_refsignal_dl_sync_set_cell(void* q, cell_t cell);
void srslte_refsignal_dl_sync_free(void* q);
void srslte_refsignal_dl_sync_run(void* q, cf_t* buffer, uint32_t nsamples);
int  srslte_symbol_sz(uint32_t nof_prb);

#define STORAGE (1u << 20) /* sizeof(srslte_refsignal_dl_sync_t) is a few hundred bytes */

typedef struct {
  int32_t  found;
  uint32_t peak_index, sf_idx, nof_sf;
  float    peak_value, rms_avg, rsrp_lin, rssi_lin, rsrp_dBfs, rssi_dBfs, rsrq_dB, cfo_Hz;
  uint32_t cell_id, capture, reserved[2];
} row_t;

typedef struct {
  uint32_t nof_prb, nof_sf, n, in_stride;
} hdr_t;

static int rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n ? 0 : -1; }

/* init on marked storage -> sizeof(srslte_refsignal_dl_sync_t), or 0 */
static size_t setup(uint8_t* q)
{
  memset(q, 0xA5, STORAGE);
  if (srslte_refsignal_dl_sync_init(q)) return 0;
  size_t end = STORAGE;
  while (end > 0 && q[end - 1] == 0xA5) end--;
  return (end % 8 == 0 && end >= 64 && end < STORAGE) ? end : 0;
}

int main(int argc, char** argv)
{
  if (argc < 4) return 2;
  uint8_t* q = malloc(STORAGE);
  if (!q) return 3;
  if (argv[1][0] == 'r' && argc == 4) {
    FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    hdr_t h;
    if (!in || !out || rd(in, &h, sizeof(h))) return 4;
    cf_t* buf = calloc((size_t)h.in_stride + 16, sizeof(cf_t));
    if (!buf) return 3;
    const uint32_t sf_len = 15 * (uint32_t)srslte_symbol_sz(h.nof_prb);
    if ((uint64_t)h.nof_sf * sf_len > h.in_stride) return 4;
    for (uint32_t i = 0; i < h.n; i++) {
      uint32_t id;
      if (rd(in, &id, 4) || rd(in, buf, (size_t)h.in_stride * sizeof(cf_t))) return 5;
      const size_t sz = setup(q);
      cell_t       cell = {h.nof_prb, 1, id, 0, 0, 0, 0};
      if (!sz || srslte_refsignal_dl_sync_set_cell(q, cell)) return 6;
      srslte_refsignal_dl_sync_run(q, buf, h.nof_sf * sf_len);
      row_t r;
      memset(&r, 0, sizeof(r));
      bool found;
      memcpy(&found, q + sz - 24, sizeof(found));
      r.found = found ? 1 : 0;
      memcpy(&r.rsrp_dBfs, q + sz - 20, 4);
      memcpy(&r.rssi_dBfs, q + sz - 16, 4);
      memcpy(&r.rsrq_dB, q + sz - 12, 4);
      memcpy(&r.cfo_Hz, q + sz - 8, 4);
      memcpy(&r.peak_index, q + sz - 4, 4);
      r.sf_idx = r.nof_sf = 0xffffffffu;
      r.peak_value = r.rms_avg = r.rsrp_lin = r.rssi_lin = NAN;
      r.cell_id = id, r.capture = i;
      if (fwrite(&r, sizeof(r), 1, out) != 1) return 7;
      srslte_refsignal_dl_sync_free(q);
    }
    fclose(in);
    return fclose(out) ? 7 : 0;
  }
  if (argv[1][0] == 't' && argc == 5) {
    const uint32_t nof_prb = (uint32_t)atoi(argv[2]), nof_sf = (uint32_t)atoi(argv[3]);
    const int      reps    = atoi(argv[4]);
    const uint32_t sf_len  = 15 * (uint32_t)srslte_symbol_sz(nof_prb);
    const size_t   len     = (size_t)nof_sf * sf_len;
    cf_t*          buf     = calloc(len + 16, sizeof(cf_t));
    if (!buf || reps < 1 || !setup(q)) return 3;
    uint32_t s = 1;
    for (size_t i = 0; i < len; i++) {
      s = s * 1664525u + 1013904223u;
      const float a = (float)(s >> 8) / 16777216.f - 0.5f;
      s = s * 1664525u + 1013904223u;
      buf[i] = a + I * ((float)(s >> 8) / 16777216.f - 0.5f);
    }
    cell_t cell = {nof_prb, 1, 1, 0, 0, 0, 0};
    if (srslte_refsignal_dl_sync_set_cell(q, cell)) return 6;
    srslte_refsignal_dl_sync_run(q, buf, (uint32_t)len);
    struct timespec t0, t1, t2;
    double          ts = 0, tr = 0;
    for (int r = 0; r < reps; r++) {
      cell.id = 2 + (uint32_t)r; /* set_cell rebuilds only for a new id */
      clock_gettime(CLOCK_MONOTONIC, &t0);
      if (srslte_refsignal_dl_sync_set_cell(q, cell)) return 6;
      clock_gettime(CLOCK_MONOTONIC, &t1);
      srslte_refsignal_dl_sync_run(q, buf, (uint32_t)len);
      clock_gettime(CLOCK_MONOTONIC, &t2);
      ts += (t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec);
      tr += (t2.tv_sec - t1.tv_sec) + 1e-9 * (t2.tv_nsec - t1.tv_nsec);
    }
    printf("%.9f %.9f\n", ts / reps, tr / reps);
    srslte_refsignal_dl_sync_free(q);
    return 0;
  }
  return 2;
}
