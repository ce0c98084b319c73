// The host side of the NB-IoT synchronisation (include/srslte_hip/phy_hip.h, "NB-IoT synchronisation"): the NPSS / NSSS sequences of
// srslte_npss_generate / srslte_nsss_generate, the time-domain replicas of srslte_npss_corr_init / srslte_nsss_corr_init, the tables
// nbiot_sync.hip uploads, the RE positions of the two put_subframe functions and the checks of a call. No device is needed for anything here.
#include "common.hpp"
#include "phy_hip_internal.hpp"
#include <math.h>
#include <string.h>
#include <vector>

namespace {

constexpr uint32_t NB_N = 128, NB_NSYM = 11, NB_LEN = SRSLTE_HIP_NBIOT_REPLICA_LEN, NB_TAPS = 138;

uint32_t sym_cp(uint32_t i) { return i == 4 ? 10u : 9u; }          // the fifth symbol of the replica is symbol 0 of the second slot
uint32_t sym_start(uint32_t i) { return 137 * i + (i > 4 ? 1u : 0u); }

// srslte_npss_generate (npss.c:399-421): the phase formed in double, rounded to float, then cosf / sinf, times the symbol's sign
const float npss_sign[NB_NSYM] = {1, 1, 1, 1, -1, -1, 1, 1, 1, -1, 1};
void        npss_seq(cf32* out)
{
  for (uint32_t l = 0; l < NB_NSYM; l++)
    for (uint32_t n = 0; n < 11; n++) {
      const float fn  = (float)n;
      const float arg = (float)((float)-1 * M_PI * 5.0f * (fn * (fn + 1.0)) / 11.0);
      out[l * 11 + n] = make_float2(cosf(arg) * npss_sign[l], sinf(arg) * npss_sign[l]);
    }
}

// b_q(m) of 36.211 Table 10.2.7.2.1-1: column 0, 31, 63 or 127 of the 128-point Hadamard matrix
int nsss_b(uint32_t q, uint32_t m)
{
  const uint32_t col[4] = {0, 31, 63, 127};
  return (__builtin_popcount(m & col[q]) & 1) ? -1 : 1;
}

// srslte_nsss_generate (nsss.c:348-377), all four theta_f, in the reference's float expression order
void nsss_seq(uint32_t cell_id, cf32* out)
{
  const int      u = (int)(cell_id % 126) + 3;
  const uint32_t q = cell_id / 126;
  for (int theta_f = 0; theta_f < 4; theta_f++)
    for (int n = 0; n < 132; n++) {
      const int   n_prime = n % 131, m = n % 128;
      float       arg = (float)((float)-1 * 2.0 * M_PI * ((float)theta_f) * ((float)n));
      const float c1 = cosf(arg), s1 = sinf(arg);
      arg            = (float)(((float)-1 * M_PI * ((float)u) * (float)n_prime * ((float)n_prime + 1.0)) / 131.0);
      const float c2 = cosf(arg), s2 = sinf(arg);
      const float b  = (float)nsss_b(q, (uint32_t)m);
      const float x = b * c1, y = b * s1;
      out[theta_f * 132 + n] = make_float2(x * c2 - y * s2, x * s2 + y * c2);
    }
}

// exp(j 2 pi (f + 1/2) d / 128) for an integer frequency f and a sample distance d from the end of the CP, the argument reduced exactly
void half_sc_phasor(int f, int d, double* c, double* s)
{
  const int64_t k = (((int64_t)(2 * f + 1) * d) % 256 + 256) % 256; // (f + 1/2) d / 128 = (2 f + 1) d / 256 cycles
  const double  a = 2.0 * M_PI * (double)k / 256.0;
  *c = cos(a), *s = sin(a);
}

// h[s_i + t] = scale sum_sc S[i][sc] exp(j 2 pi (f0 + sc + 1/2) (t - cp_i) / 128): the mirrored inverse transform (buffer index k is frequency
// k - 64), the CP as the periodic continuation, and the half-subcarrier table, which restarts in every symbol
void replica(const cf32* S, uint32_t nsc, int f0, double scale, cf32* h)
{
  for (uint32_t i = 0; i < NB_NSYM; i++) {
    const uint32_t cp = sym_cp(i);
    for (uint32_t t = 0; t < NB_N + cp; t++) {
      double re = 0, im = 0;
      for (uint32_t sc = 0; sc < nsc; sc++) {
        double c, s;
        half_sc_phasor(f0 + (int)sc, (int)t - (int)cp, &c, &s);
        const double xr = S[i * nsc + sc].x, xi = S[i * nsc + sc].y;
        re += xr * c - xi * s, im += xr * s + xi * c;
      }
      h[sym_start(i) + t] = make_float2((float)(re * scale), (float)(im * scale));
    }
  }
}

} // namespace

void nbiot_tables(NbiotTables& t)
{
  const double g = 1.0 / sqrt(128.0);
  cf32         npss[121], h[NB_LEN];
  npss_seq(npss);
  replica(npss, 11, -6, g / 3.0, h);
  t.npss_head.assign(h, h + NB_N);
  // the taps of a CP class: the conjugated first symbol of that length (sign +1); the symbols differ by their sign only
  t.npss_taps.assign(2 * NB_TAPS, make_float2(0.f, 0.f));
  for (uint32_t cls = 0; cls < 2; cls++)
    for (uint32_t tt = 0; tt < NB_N + 9 + cls; tt++) {
      double re = 0, im = 0;
      for (uint32_t sc = 0; sc < 11; sc++) {
        double c, s;
        half_sc_phasor(-6 + (int)sc, (int)tt - (int)(9 + cls), &c, &s);
        re += (double)npss[sc].x * c - (double)npss[sc].y * s, im += (double)npss[sc].x * s + (double)npss[sc].y * c;
      }
      t.npss_taps[cls * NB_TAPS + tt] = make_float2((float)(re * g / 3.0), (float)(-im * g / 3.0));
    }
  // srslte_cexptab_gen_sf(-SRSLTE_NBIOT_FREQ_SHIFT_FACTOR) from sample 960 on: the second slot's symbols, CP 10 then CP 9
  t.shift2.resize(823);
  for (uint32_t i = 0, o = 0; i < 6; i++) {
    const uint32_t cp = i == 0 ? 10 : 9;
    for (uint32_t tt = 0; tt < NB_N + cp; tt++) {
      const float a    = (float)(2 * M_PI * ((float)tt - (float)cp) * 0.5f / 128);
      t.shift2[o + tt] = make_float2(cosf(a), sinf(a));
    }
    o += NB_N + cp;
  }
  t.nsss_tw.assign(2 * 12 * NB_TAPS, make_float2(0.f, 0.f));
  for (uint32_t cls = 0; cls < 2; cls++)
    for (uint32_t sc = 0; sc < 12; sc++)
      for (uint32_t tt = 0; tt < NB_N + 9 + cls; tt++) {
        double c, s;
        half_sc_phasor(-7 + (int)sc, (int)tt - (int)(9 + cls), &c, &s);
        t.nsss_tw[(cls * 12 + sc) * NB_TAPS + tt] = make_float2((float)(c * g), (float)(-s * g));
      }
  t.nsss_seq.resize(132 * (size_t)SRSLTE_HIP_NBIOT_NUM_PCI);
  for (uint32_t id = 0; id < SRSLTE_HIP_NBIOT_NUM_PCI; id++) {
    cf32 s[528];
    nsss_seq(id, s);
    for (uint32_t r = 0; r < 132; r++) t.nsss_seq[(size_t)r * SRSLTE_HIP_NBIOT_NUM_PCI + id] = make_float2(s[r].x, -s[r].y);
  }
}

bool nbiot_cfg_valid(const srslte_hip_nbiot_sync_cfg_t* c)
{
  if (!c || c->fft_size != NB_N) return false;
  if (c->frame_size == 0 || c->frame_size > 307200) return false; // srslte_sync_nbiot_resize's bound
  if (c->max_items == 0 || c->max_items > 8191 || c->n_tracks == 0 || c->n_tracks > 65535) return false;
  if (c->cfo_enable && c->max_offset == 0) return false; // srslte_cp_synch over no offset leaves nothing to take the argument of
  if (!(c->threshold >= 0.f) || !(c->nsss_threshold >= 0.f) || !(c->npss_ema_alpha >= 0.f) || !(c->cfo_ema_alpha >= 0.f)) return false;
  return true;
}

extern "C" {

uint32_t srslte_hip_nbiot_npss_nout(uint32_t frame_size)
{ // conv_output_len - 1: srslte_corr_fft_cc_run_opt returns output_len - 1 (convolution.c:135), the short branch frame_size (npss.c:269)
  return frame_size >= NB_N ? frame_size + NB_LEN - 2 : (frame_size ? frame_size - 1 : 0);
}

int srslte_hip_nbiot_sync_check(const srslte_hip_nbiot_sync_cfg_t* c, size_t in_stride, const srslte_hip_nbiot_npss_item_t* items, uint32_t n)
{
  if (!nbiot_cfg_valid(c) || (n && !items) || n > c->max_items) return SRSLTE_ERROR_INVALID_INPUTS;
  if (n == 0) return SRSLTE_SUCCESS;
  // the CFO stage reads the item, not the window: up to peak_pos + 548 + 127 + 822 < frame_size by its entry condition
  if (c->frame_size > in_stride) return SRSLTE_ERROR_INVALID_INPUTS;
  const uint64_t       reach = (uint64_t)c->frame_size + (c->frame_size < NB_N ? NB_N - 1 : 0);
  std::vector<uint8_t> seen(c->n_tracks, 0);
  for (uint32_t i = 0; i < n; i++) {
    if (items[i].track >= c->n_tracks || seen[items[i].track]) return SRSLTE_ERROR_INVALID_INPUTS;
    seen[items[i].track] = 1;
    // the kernels index an item's samples in 32 bits
    if ((uint64_t)items[i].find_offset + reach > in_stride || (uint64_t)items[i].find_offset + reach > 0xffffffffull) return SRSLTE_ERROR_INVALID_INPUTS;
  }
  return SRSLTE_SUCCESS;
}

int srslte_hip_nbiot_nsss_check(const srslte_hip_nbiot_sync_cfg_t* c, size_t in_stride, const int32_t* cell_ids, uint32_t n)
{
  if (!nbiot_cfg_valid(c) || (n && !cell_ids) || n > c->max_items) return SRSLTE_ERROR_INVALID_INPUTS;
  if (n && in_stride < SRSLTE_HIP_NBIOT_NSSS_IN_LEN) return SRSLTE_ERROR_INVALID_INPUTS;
  for (uint32_t i = 0; i < n; i++)
    if (cell_ids[i] < -1 || cell_ids[i] >= SRSLTE_HIP_NBIOT_NUM_PCI) return SRSLTE_ERROR_INVALID_INPUTS;
  return SRSLTE_SUCCESS;
}

int srslte_hip_nbiot_npss_generate(void* out)
{
  if (!out) return SRSLTE_ERROR_INVALID_INPUTS;
  npss_seq((cf32*)out);
  return SRSLTE_SUCCESS;
}

int srslte_hip_nbiot_nsss_generate(void* out, uint32_t cell_id)
{
  if (!out || cell_id >= SRSLTE_HIP_NBIOT_NUM_PCI) return SRSLTE_ERROR_INVALID_INPUTS;
  nsss_seq(cell_id, (cf32*)out);
  return SRSLTE_SUCCESS;
}

int srslte_hip_nbiot_npss_replica(void* out)
{
  if (!out) return SRSLTE_ERROR_INVALID_INPUTS;
  cf32 s[121];
  npss_seq(s);
  replica(s, 11, -6, 1.0 / sqrt(128.0) / 3.0, (cf32*)out);
  return SRSLTE_SUCCESS;
}

int srslte_hip_nbiot_nsss_replica(void* out, uint32_t cell_id)
{
  if (!out || cell_id >= SRSLTE_HIP_NBIOT_NUM_PCI) return SRSLTE_ERROR_INVALID_INPUTS;
  cf32 s[528];
  nsss_seq(cell_id, s);
  replica(s, 12, -7, 1.0 / sqrt(128.0), (cf32*)out); // theta_f = 0: the first 132 values
  return SRSLTE_SUCCESS;
}

int srslte_hip_nbiot_npss_re(uint32_t nof_prb, uint32_t prb_offset, uint32_t* re)
{
  if (!re || nof_prb == 0 || prb_offset >= nof_prb) return SRSLTE_ERROR_INVALID_INPUTS;
  uint32_t k = 3 * nof_prb * 12 + prb_offset * 12; // the first three symbols carry nothing
  for (uint32_t l = 0; l < NB_NSYM; l++) {
    for (uint32_t n = 0; n < 11; n++) re[11 * l + n] = k + 11 * l + n;
    k += (nof_prb - 1) * 12 + 1; // the PRB's last subcarrier stays empty
  }
  return SRSLTE_SUCCESS;
}

int srslte_hip_nbiot_nsss_re(uint32_t nof_prb, uint32_t prb_offset, int nf, uint32_t* re, uint32_t* first)
{
  if (!re || !first || nof_prb == 0 || prb_offset >= nof_prb || nf < 0) return SRSLTE_ERROR_INVALID_INPUTS;
  const int theta_f = (int)floor(33 / 132.0 * (nf / 2.0)) % 4;
  *first            = (uint32_t)theta_f * 132;
  uint32_t k        = 3 * nof_prb * 12 + prb_offset * 12;
  for (uint32_t l = 0; l < NB_NSYM; l++) {
    for (uint32_t n = 0; n < 12; n++) re[12 * l + n] = k + 12 * l + n;
    k += (nof_prb - 1) * 12;
  }
  return SRSLTE_SUCCESS;
}

} // extern "C"
