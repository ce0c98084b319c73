// The host side of the PSS / SSS synchronisation (include/srslte_hip/phy_hip.h, "UE synchronisation"): the tables sync.hip uploads - the
// time-domain PSS replicas of srslte_pss_init_N_id_2, their half-symbol transforms for the filtered CFO estimate, the DFT twiddles, the SSS
// tables of gen_sss.c / convert_tables - the checks of a call, and get_cell of ue_cell_search.c. No device is needed for anything here.
#include "common.hpp"
#include "phy_hip_internal.hpp"
#include <math.h>
#include <string.h>
#include <vector>

namespace {

// CP lengths in samples of an N-point symbol (phy_common.h:93-113)
uint32_t cp_norm(uint32_t N) { return (uint32_t)lte_cp_len((int)N, 144); }

} // namespace

bool sync_fft_size_valid(uint32_t N) { return N >= 64 && N <= 2048 && N % 64 == 0; } // sync.c:41-47

int sync_bin_freq(int j) { return j < 31 ? j - 31 : j - 30; } // bin j of the 62 around DC in a mirrored transform that skips DC (dft_fftw.c:249-272)

void sync_pss_seq(int v, cf32* pss)
{ // srslte_pss_generate (pss.c:348-376): the phase formed in double, rounded to float, then cosf / sinf
  const float root = v == 0 ? 25.0f : v == 1 ? 29.0f : 34.0f;
  for (int i = 0; i < 62; i++) {
    const float fi  = (float)i;
    float       arg = (float)((float)-1 * M_PI * root * (i < 31 ? fi * (fi + 1.0) : (fi + 2.0) * (fi + 1.0)) / 63.0);
    pss[i]          = make_float2(cosf(arg), sinf(arg));
  }
}

void sync_tables(uint32_t N, SyncTables& t)
{
  t.replica.assign(3 * (size_t)N, make_float2(0.f, 0.f));
  t.half.assign(3 * 2 * 62, make_float2(0.f, 0.f));
  t.tw.resize(N);
  for (uint32_t k = 0; k < N; k++) {
    const double a = -2.0 * M_PI * (double)k / (double)N;
    t.tw[k]        = make_float2((float)cos(a), (float)sin(a));
  }
  for (int v = 0; v < 3; v++) {
    cf32   pss[62];
    double pr[62], pi[62];
    sync_pss_seq(v, pss);
    for (int i = 0; i < 62; i++) pr[i] = pss[i].x, pi[i] = pss[i].y;
    // srslte_pss_init_N_id_2 (pss.c:32-66): the 62 values around DC, inverse transform scaled by 1 / sqrt(N), conjugated, times 1 / 62
    cf32* h = &t.replica[(size_t)v * N];
    for (uint32_t n = 0; n < N; n++) {
      double re = 0, im = 0;
      for (int j = 0; j < 62; j++) {
        const int64_t k = (((int64_t)sync_bin_freq(j) * (int64_t)n) % (int64_t)N + N) % N;
        const double  a = 2.0 * M_PI * (double)k / (double)N, c = cos(a), s = sin(a);
        re += pr[j] * c - pi[j] * s, im += pr[j] * s + pi[j] * c;
      }
      const double g = 1.0 / sqrt((double)N) / 62.0;
      h[n]           = make_float2((float)(re * g), (float)(-im * g));
    }
    // H_p[j] = sum over half p of h[n] exp(j 2 pi f_j n / N): with X the 62 bins of the received symbol, sum_j X[j] H_p[j] is the product of
    // the replica's half with srslte_pss_filter's output (pss.c:587-600,:617-618)
    for (int p = 0; p < 2; p++)
      for (int j = 0; j < 62; j++) {
        double re = 0, im = 0;
        for (uint32_t n = p * N / 2; n < (p + 1) * N / 2; n++) {
          const int64_t k = (((int64_t)sync_bin_freq(j) * (int64_t)n) % (int64_t)N + N) % N;
          const double  a = 2.0 * M_PI * (double)k / (double)N, c = cos(a), s = sin(a);
          re += (double)h[n].x * c - (double)h[n].y * s, im += (double)h[n].x * s + (double)h[n].y * c;
        }
        t.half[(v * 2 + p) * 62 + j] = make_float2((float)re, (float)im);
      }
  }
  // gen_sss.c:31-119: s~, c~, z~; s[m][i] = s~[(i + m) % 31], z1[m][i] = z~[(i + m % 8) % 31], c[v][0 / 1][i] = c~[(i + v (+ 3)) % 31]
  int       st[31], ct[31], zt[31], x[31];
  const int taps[3][4] = {{2, 0, -1, -1}, {3, 0, -1, -1}, {4, 2, 1, 0}};
  int*      dst[3]     = {st, ct, zt};
  for (int s = 0; s < 3; s++) {
    memset(x, 0, sizeof(x));
    x[4] = 1;
    for (int i = 0; i < 26; i++) {
      int b = 0;
      for (int j = 0; j < 4; j++)
        if (taps[s][j] >= 0) b += x[i + taps[s][j]];
      x[i + 5] = b % 2;
    }
    for (int i = 0; i < 31; i++) dst[s][i] = 1 - 2 * x[i];
  }
  t.s.resize(31 * 31), t.z1.resize(31 * 31), t.c.resize(3 * 2 * 31);
  for (int m = 0; m < 31; m++)
    for (int i = 0; i < 31; i++) t.s[m * 31 + i] = (float)st[(i + m) % 31], t.z1[m * 31 + i] = (float)zt[(i + m % 8) % 31];
  for (int v = 0; v < 3; v++)
    for (int i = 0; i < 31; i++) t.c[(v * 2) * 31 + i] = (float)ct[(i + v) % 31], t.c[(v * 2 + 1) * 31 + i] = (float)ct[(i + v + 3) % 31];
  // generate_N_id_1_table (gen_sss.c:63-71) over the zeroed table of srslte_sss_init: a pair no cell uses reads 0
  t.nid1.assign(30 * 30, 0);
  for (uint32_t id = 0; id < 168; id++) {
    uint32_t m0, m1;
    sync_m0m1(id, &m0, &m1);
    t.nid1[m0 * 30 + m1 - 1] = (int32_t)id;
  }
}

void sync_m0m1(uint32_t N_id_1, uint32_t* m0, uint32_t* m1) // generate_m0m1 (gen_sss.c:54-60)
{
  const uint32_t qp = N_id_1 / 30, q = (N_id_1 + qp * (qp + 1) / 2) / 30, mp = N_id_1 + q * (q + 1) / 2;
  *m0 = mp % 31;
  *m1 = (*m0 + mp / 31 + 1) % 31;
}

// samples srslte_cp_synch reads from the start of an item (cp.c:61-77): offsets < min(max_offset, N), nsym symbols, every seventh one sample longer
static uint64_t cp_stage_extent(const srslte_hip_sync_cfg_t* c)
{
  const uint32_t N = c->fft_size, M = c->max_offset < N ? c->max_offset : N;
  uint64_t       e = M - 1;
  for (uint32_t n = 0; n < c->cfo_cp_nsymbols; n++) e += N + cp_norm(N) + (n % 7 ? 0 : 1);
  return e;
}

bool sync_cfg_valid(const srslte_hip_sync_cfg_t* c)
{
  if (!c || !sync_fft_size_valid(c->fft_size) || c->tdd || c->decimate > 1) return false;
  if (c->max_offset < 2 || c->max_items == 0 || c->max_items > 21845 || c->frame_size < c->max_offset) return false; // 3 max_items rows: grid.y <= 65535
  if ((c->cp != 0 && c->cp != 1) || c->sss_alg > 2) return false;
  if (c->cfo_cp_enable && (c->cfo_cp_nsymbols == 0 || cp_stage_extent(c) > c->frame_size)) return false;
  if (!(c->ema_alpha >= 0.f) || !(c->threshold >= 0.f)) return false;
  return true;
}

bool sync_tracks_cfg_valid(const srslte_hip_sync_tracks_cfg_t* c)
{
  return c && c->n_tracks > 0 && c->n_tracks <= 65535 && c->frame_mode <= 2 && c->cfo_ema_alpha >= 0.f; // a launch's grid holds 65535 tracks
}

extern "C" {

int srslte_hip_sync_check(const srslte_hip_sync_cfg_t* c, size_t in_stride, const srslte_hip_sync_item_t* items, uint32_t n)
{
  if (!sync_cfg_valid(c) || (n && !items) || n > c->max_items) return SRSLTE_ERROR_INVALID_INPUTS;
  if (c->frame_size > in_stride) return SRSLTE_ERROR_INVALID_INPUTS;
  const uint64_t N = c->fft_size;
  for (uint32_t i = 0; i < n; i++) {
    const srslte_hip_sync_item_t& it = items[i];
    if (it.N_id_2 > 3 || it.N_id_1 >= 168) return SRSLTE_ERROR_INVALID_INPUTS;
    // the searched window lies in the frame; a peak at the window's last position makes the CFO, SSS and CP stages read up to that position:
    // find_offset + max_offset + N - 2 samples in the convolution branch, find_offset + max_offset + N in the tracking branch (pss.c:485-490)
    if ((uint64_t)it.find_offset + c->max_offset > c->frame_size) return SRSLTE_ERROR_INVALID_INPUTS;
    const uint64_t reach = (uint64_t)it.find_offset + c->max_offset + N - (c->max_offset < N ? 0 : 2);
    if (reach > in_stride) return SRSLTE_ERROR_INVALID_INPUTS;
  }
  return SRSLTE_SUCCESS;
}

// The TDD trial reads the symbol two symbols before the FDD one's: further back, never further on, and a trial whose symbol would start before
// the item's first sample does not run. So the window checks are those of the stateless call.
int srslte_hip_sync_tracks_check(const srslte_hip_sync_cfg_t* c, const srslte_hip_sync_tracks_cfg_t* tc, size_t in_stride,
                                 const srslte_hip_sync_track_item_t* items, uint32_t n)
{
  if (!sync_cfg_valid(c) || !sync_tracks_cfg_valid(tc) || (n && !items) || n > c->max_items || n > tc->n_tracks) return SRSLTE_ERROR_INVALID_INPUTS;
  if (c->frame_size > in_stride) return SRSLTE_ERROR_INVALID_INPUTS;
  std::vector<uint8_t> seen(tc->n_tracks, 0);
  for (uint32_t i = 0; i < n; i++) {
    const srslte_hip_sync_track_item_t& it = items[i];
    if (it.track >= tc->n_tracks || seen[it.track] || it.N_id_2 > 2 || it.N_id_1 >= 168) return SRSLTE_ERROR_INVALID_INPUTS;
    seen[it.track] = 1;
    const srslte_hip_sync_item_t one = {it.N_id_2, it.find_offset, it.N_id_1};
    if (int r = srslte_hip_sync_check(c, in_stride, &one, 1)) return r;
  }
  return SRSLTE_SUCCESS;
}

// get_cell (ue_cell_search.c:189-250) over the rows srslte_ue_cellsearch_scan_N_id_2 keeps (:311-332): a found peak with a valid cell id
int srslte_hip_cell_search_decide(const srslte_hip_sync_res_t* found, uint32_t nof_found, srslte_hip_cell_search_result_t* out)
{
  if (!out || (nof_found && !found)) return SRSLTE_ERROR_INVALID_INPUTS;
  std::vector<const srslte_hip_sync_res_t*> cand;
  for (uint32_t i = 0; i < nof_found; i++)
    if (found[i].ret == 1 && found[i].cell_id >= 0) cand.push_back(&found[i]);
  memset(out, 0, sizeof(*out));
  const uint32_t n = (uint32_t)cand.size();
  if (n == 0) return 0;
  std::vector<uint8_t>  counted(n, 0);
  std::vector<uint32_t> ntimes(n, 0);
  for (uint32_t i = 0; i < n; i++) {
    uint32_t cnt = 1;
    for (uint32_t j = i + 1; j < n; j++)
      if (cand[j]->cell_id == cand[i]->cell_id && !counted[j]) counted[j] = 1, cnt++;
    ntimes[i] = cnt;
  }
  uint32_t max_times = 0, mode_pos = 0;
  for (uint32_t i = 0; i < n; i++)
    if (ntimes[i] > max_times) max_times = ntimes[i], mode_pos = i;
  out->cell_id        = (uint32_t)cand[mode_pos]->cell_id;
  uint32_t nof_normal = 0;
  float    peak       = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (cand[i]->cell_id == (int32_t)out->cell_id && cand[i]->cp == 0) nof_normal++;
    peak += cand[i]->corr_peak;
  }
  out->peak       = peak / n;
  out->cp         = nof_normal > ntimes[mode_pos] / 2 ? 0 : 1;
  out->mode       = (float)ntimes[mode_pos] / n;
  out->psr        = cand[n - 1]->peak_value;
  out->cfo        = 15000 * cand[n - 1]->cfo;
  out->nof_frames = n;
  return (int)n;
}

// the same over tracked rows, with the frame type by the rule of the CP (ue_cell_search.c:216-242)
int srslte_hip_cell_search_decide_ft(const srslte_hip_sync_track_res_t* found, uint32_t nof_found, srslte_hip_cell_search_result_t* out, int32_t* frame_type)
{
  if (!out || !frame_type || (nof_found && !found)) return SRSLTE_ERROR_INVALID_INPUTS;
  std::vector<srslte_hip_sync_res_t> rows(nof_found);
  for (uint32_t i = 0; i < nof_found; i++) rows[i] = found[i].r;
  *frame_type = 0;
  const int n = srslte_hip_cell_search_decide(rows.data(), nof_found, out);
  if (n <= 0) return n;
  uint32_t times = 0, nof_fdd = 0;
  for (uint32_t i = 0; i < nof_found; i++)
    if (found[i].r.ret == 1 && found[i].r.cell_id == (int32_t)out->cell_id) times++, nof_fdd += found[i].frame_type == 0 ? 1 : 0;
  *frame_type = nof_fdd > times / 2 ? 0 : 1;
  return n;
}

} // extern "C"
