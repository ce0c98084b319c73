// PSS / SSS synchronisation for gfx950, FDD (include/srslte_hip/phy_hip.h, "UE synchronisation"): the first srslte_sync_find of a reset
// srslte_sync_t for a batch of items, and the batched CFO correction.
//   sync_cp_kernel      one workgroup per item: srslte_cp_synch's correlations, their first maximum, cfo_cp
//   sync_corr_kernel    grid (tile of 256 outputs, item x hypothesis): the replica and the tile's input samples - rotated by -cfo_cp / N as
//                       they are loaded - in LDS, a lane per output with consecutive-address LDS reads; writes the averaged |c|^2 and the
//                       tile's (maximum, first index)
//   sync_decide_kernel  one workgroup per (item, hypothesis): the peak over the tiles, the side lobe, the 62-bin direct DFTs of the PSS and SSS
//                       symbols, the CFO from the replica's halves, the m0 / m1 correlations, the CP metrics, and the result row
//   cfo_correct_kernel  a lane per sample, the phase reduced in double before sincospif
// The tracked call (srslte_hip_sync_track_batch: a srslte_sync_t's state per track, kept on the device) runs the same three bodies, instantiated a
// second time under kernel names of their own (track_cp_kernel, track_corr_kernel, track_decide_kernel): the stateless kernels take no state
// pointer and compile to what they were.
//   track_cp_kernel      also folds the estimate into the track's CP-CFO mean; the later stages read the frame rotated by that mean
//   track_corr_kernel    with 0 < ema_alpha < 1 reads and writes the track's own average row where the stateless kernel writes the call's row
//   track_decide_kernel  the carried cp, the FDD / TDD SSS trials one after the other in the same LDS, the frame-type decision, the state
//                        update and the 24-word row
//   track_reset_kernel, track_copy_cfo_kernel   one workgroup per listed track
// The rotated load, the workgroup reductions, the side lobe and the CP correlation are search_dev.hpp's, shared with nbiot_sync.hip.
// The tables come from sync_host.cpp.
#include "common.hpp"
#include "dev_buf.hpp"
#include "phy_hip_internal.hpp"
#include "search_dev.hpp"
#include <math.h>
#include <string.h>
#include <vector>

namespace {

constexpr int      SYNC_THREADS = 256;
constexpr uint32_t SYNC_TILE    = 256;

struct SyncRow {
  uint32_t item, N_id_2, find_offset;
  int32_t  N_id_1;
  uint32_t m0, m1, track, pad; // generate_m0m1 of a known N_id_1; track: the tracked call's state index
};

typedef srslte_hip_sync_track_state_t TrackState;
struct TrackParams {
  TrackState* st;        // [n_tracks]
  float*      avg;       // [n_tracks][nout] with 0 < ema_alpha < 1, else null
  float       cfo_alpha; // cfo_ema_alpha
  uint32_t    frame_mode;
};

struct SyncParams {
  uint32_t N, max_offset, nout, ntiles, track; // nout: values that enter the maximum
  uint32_t cpn, cpe;                           // CP_LEN_NORM(1, N) = CP_LEN_NORM(7, N), CP_LEN_EXT(N)
  uint32_t cp_nsym;
  int      cp;
  uint32_t detect_cp, sss_en, cfo_cp_enable, cfo_pss_enable, pss_filt_enable, sss_alg;
  float    threshold, sss_threshold, alpha; // alpha: 0 = no scaling
  size_t   in_stride;
  const cf32 *   replica, *half, *tw;
  const float *  s, *z1, *c;
  const int32_t* nid1;
  float*         avg;      // [row][nout]
  float2*        tile_max; // [row][ntiles]: value, index as bits
  float*         cfo_cp;   // [item]
  cf32*          cp_corr;  // [item][min(max_offset, N)]
};

__device__ float block_sum(float v, float* s_red)
{
  v = wave_sum(v);
  if (threadIdx.x % 64 == 0) s_red[threadIdx.x / 64] = v;
  __syncthreads();
  v = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
  __syncthreads();
  return v;
}

template <bool TR>
__device__ __forceinline__ void cp_body(const SyncParams& p, const cf32* __restrict__ in, const SyncRow* __restrict__ rows, const TrackParams& t)
{
  __shared__ float    s_v[SYNC_THREADS];
  __shared__ uint32_t s_i[SYNC_THREADS];
  const uint32_t item = blockIdx.x, M = p.max_offset < p.N ? p.max_offset : p.N;
  const cf32*    x    = in + (size_t)item * p.in_stride;
  cf32*          corr = p.cp_corr + (size_t)item * M;
  float          best = -INFINITY;
  uint32_t       bi   = NO_INDEX;
  for (uint32_t i = threadIdx.x; i < M; i += SYNC_THREADS) {
    const cf32 acc = cp_synch_at([&](uint32_t j) { return x[j]; }, p.N, p.cpn, p.cp_nsym, i);
    corr[i]        = acc;
    const float v  = acc.x * acc.x + acc.y * acc.y;
    if (v > best) best = v, bi = i;
  }
  block_argmax<SYNC_THREADS>(best, bi, s_v, s_i);
  if (threadIdx.x == 0) {
    const cf32  c   = corr[bi == NO_INDEX ? 0u : bi];
    const float est = (float)(-atan2((double)c.y, (double)c.x) / M_PI / 2); // cfo_cp_estimate (sync.c:572-579)
    if constexpr (!TR) {
      p.cfo_cp[item] = est;
    } else { // sync.c:660-676: the first estimate is the mean, later ones are averaged into it; the frame is read rotated by the mean
      TrackState& s    = t.st[rows[item].track];
      const float mean = s.cfo_cp_is_set ? t.cfo_alpha * est + (1 - t.cfo_alpha) * s.cfo_cp_mean : est;
      s.cfo_cp_mean = mean, s.cfo_cp_is_set = 1, s.cfo_cp_inst = est;
      p.cfo_cp[item] = mean;
    }
  }
}
__global__ __launch_bounds__(SYNC_THREADS) void sync_cp_kernel(SyncParams p, const cf32* __restrict__ in) { cp_body<false>(p, in, nullptr, TrackParams{}); }
__global__ __launch_bounds__(SYNC_THREADS) void track_cp_kernel(SyncParams p, TrackParams t, const SyncRow* __restrict__ rows, const cf32* __restrict__ in)
{
  cp_body<true>(p, in, rows, t);
}

template <bool TR>
__device__ __forceinline__ void corr_body(const SyncParams& p, const SyncRow* __restrict__ rows, const cf32* __restrict__ in, const TrackParams& t)
{
  extern __shared__ cf32 s_mem[];
  __shared__ float       s_v[SYNC_THREADS];
  __shared__ uint32_t    s_i[SYNC_THREADS];
  cf32*                  s_h = s_mem;       // [N]
  cf32*                  s_x = s_mem + p.N; // [SYNC_TILE + N - 1]
  const SyncRow          r   = rows[blockIdx.y];
  const cf32*            x   = in + (size_t)r.item * p.in_stride;
  const float            f   = p.cfo_cp_enable ? -p.cfo_cp[r.item] / (float)p.N : 0.f;
  const uint32_t         N = p.N, m0 = blockIdx.x * SYNC_TILE, tid = threadIdx.x;
  for (uint32_t k = tid; k < N; k += SYNC_THREADS) s_h[k] = p.replica[(size_t)r.N_id_2 * N + k];
  if (!p.track) {
    // s_x[u] = w[m0 - (N - 1) + u], w the window's max_offset samples with zeros on both sides
    for (uint32_t u = tid; u < SYNC_TILE + N - 1; u += SYNC_THREADS) {
      const int64_t j = (int64_t)m0 - (int64_t)(N - 1) + u;
      s_x[u]          = (j >= 0 && j < (int64_t)p.max_offset) ? ld_rot(x, r.find_offset + (uint32_t)j, f) : make_float2(0.f, 0.f);
    }
  } else {
    for (uint32_t u = tid; u < SYNC_TILE + N - 1; u += SYNC_THREADS)
      s_x[u] = (m0 + u < p.nout + N - 1) ? ld_rot(x, r.find_offset + m0 + u, f) : make_float2(0.f, 0.f);
  }
  __syncthreads();
  const uint32_t m    = m0 + tid;
  float          best = -INFINITY;
  uint32_t       bi   = NO_INDEX;
  if (m < p.nout) {
    cf32 acc = make_float2(0.f, 0.f);
    if (!p.track) {
      const cf32* xe = s_x + tid + N - 1; // conv[m] = sum_k h[k] w[m - k]
#pragma unroll 4
      for (uint32_t k = 0; k < N; k++) acc = cadd(acc, cmul(s_h[k], xe[-(int)k]));
    } else {
      const cf32* xb = s_x + tid; // sum_k h[k] x[m + k]
#pragma unroll 4
      for (uint32_t k = 0; k < N; k++) acc = cadd(acc, cmul(s_h[k], xb[k]));
    }
    float v = acc.x * acc.x + acc.y * acc.y;
    if (TR && t.avg) { // pss.c:496-500: the track's own conv_output_avg, one read and one write per value
      float* a = t.avg + (size_t)r.track * p.nout + m;
      v        = p.alpha * v + (1 - p.alpha) * *a;
      *a       = v;
    } else {
      if (p.alpha != 0.f) v *= p.alpha;
      p.avg[(size_t)blockIdx.y * p.nout + m] = v;
    }
    best = v, bi = m;
  }
  block_argmax<SYNC_THREADS>(best, bi, s_v, s_i);
  if (tid == 0) p.tile_max[(size_t)blockIdx.y * p.ntiles + blockIdx.x] = make_float2(best, __uint_as_float(bi));
}
__global__ __launch_bounds__(SYNC_THREADS) void sync_corr_kernel(SyncParams p, const SyncRow* __restrict__ rows, const cf32* __restrict__ in)
{
  corr_body<false>(p, rows, in, TrackParams{});
}
__global__ __launch_bounds__(SYNC_THREADS) void track_corr_kernel(SyncParams p, TrackParams t, const SyncRow* __restrict__ rows, const cf32* __restrict__ in)
{
  corr_body<true>(p, rows, in, t);
}

// the 62 bins around DC of the mirrored, unnormalised forward transform of s_sym[0 .. N) (dft_fftw.c:249-272 with mirror and dc)
__device__ void dft62(const SyncParams& p, const cf32* s_sym, cf32 (*s_part)[64], cf32* s_bins)
{
  const uint32_t tid = threadIdx.x, j = tid & 63u, part = tid >> 6, N = p.N;
  if (j < 62) {
    const int      fj   = j < 31 ? (int)j - 31 : (int)j - 30;
    const uint32_t step = (uint32_t)(fj + (int)N) % N, n0 = part * (N / 4);
    uint32_t       idx  = (uint32_t)(((uint64_t)step * n0) % N);
    cf32           acc  = make_float2(0.f, 0.f);
    for (uint32_t n = n0; n < n0 + N / 4; n++) {
      acc = cadd(acc, cmul(s_sym[n], p.tw[idx]));
      idx += step;
      if (idx >= N) idx -= N;
    }
    s_part[part][j] = acc;
  }
  __syncthreads();
  if (tid < 62) s_bins[tid] = cadd(cadd(s_part[0][tid], s_part[1][tid]), cadd(s_part[2][tid], s_part[3][tid]));
  __syncthreads();
}

// corr[m], m < 31, of one SSS half against the table (find_sss.c:32-63), and its first maximum
__device__ uint32_t sss_half(const SyncParams& p, const cf32* y, float* s_corr)
{
  const uint32_t m = threadIdx.x;
  if (m < 31) {
    const float* s = p.s + m * 31;
    float        o = 0.f;
    if (p.sss_alg == 0) { // corr_all_zs over y[i + 1] conj(y[i]) and sd[m][i] = s[m][i + 1] s[m][i]
      cf32 a = make_float2(0.f, 0.f);
      for (int i = 0; i < 30; i++) a = cadd(a, cscale(cmulconj(y[i + 1], y[i]), s[i + 1] * s[i]));
      o = a.x * a.x + a.y * a.y;
    } else { // corr_all_sz_partial with M = 3 / 1
      const int M = p.sss_alg == 1 ? 3 : 1, Nm = 31 / M;
      for (int j = 0; j < M; j++) {
        cf32 a = make_float2(0.f, 0.f);
        for (int i = 0; i < Nm; i++) a = cadd(a, cscale(y[j * Nm + i], s[j * Nm + i]));
        o += a.x * a.x + a.y * a.y;
      }
    }
    s_corr[m] = o;
  }
  __syncthreads();
  float    best = -INFINITY;
  uint32_t bi   = 0;
  for (uint32_t i = 0; i < 31; i++)
    if (s_corr[i] > best) best = s_corr[i], bi = i;
  return bi;
}

struct DecideLds {
  cf32     sym[2048];
  cf32     part[4][64];
  cf32     bins[62];
  cf32     y[2][31];
  float    corr[31];
  float    v[SYNC_THREADS];
  uint32_t i[SYNC_THREADS];
  float    red[4];
  float    scale[2];
};

// sync_sss_symbol (sync.c:500-564) on the symbol at x[sss_idx .. sss_idx + N), read rotated by f_cp and f_pss: what the reference's call
// writes - det its return value, sf / corr always, id the N_id_1 (the known one, or srslte_sss_N_id_1's; -1: nothing written)
struct SssOut {
  uint32_t det, sf, m0, m1;
  int32_t  id;
  float    corr;
};
__device__ __forceinline__ SssOut sss_trial(const SyncParams& p, const SyncRow& r, const cf32* x, uint32_t sss_idx, float f_cp, float f_pss, DecideLds& L)
{
  const uint32_t tid = threadIdx.x, N = p.N;
  SssOut         o;
  o.det = 0, o.sf = 0, o.m0 = 0, o.m1 = 0, o.id = r.N_id_1 >= 0 ? r.N_id_1 : -1, o.corr = 0.f;
  __syncthreads();
  for (uint32_t n = tid; n < N; n += SYNC_THREADS) {
    cf32 v = ld_rot(x, sss_idx + n, f_cp);
    if (f_pss != 0.f) v = rot(v, f_pss, n);
    L.sym[n] = v;
  }
  __syncthreads();
  dft62(p, L.sym, L.part, L.bins);
  if (r.N_id_1 >= 0) {
    // the known cell's subframe-0 and subframe-5 sequences (srslte_sss_generate) against the bins (sync.c:507-536)
    const uint32_t m0 = r.m0, m1 = r.m1;
    cf32 a0 = make_float2(0.f, 0.f), a5 = a0;
    if (tid < 62) {
      const uint32_t i  = tid / 2;
      const float    c0 = p.c[(r.N_id_2 * 2) * 31 + i], c1 = p.c[(r.N_id_2 * 2 + 1) * 31 + i];
      const float    s0 = p.s[m0 * 31 + i], s1 = p.s[m1 * 31 + i];
      const float    v0 = tid & 1 ? s1 * c1 * p.z1[m0 * 31 + i] : s0 * c0, v5 = tid & 1 ? s0 * c1 * p.z1[m1 * 31 + i] : s1 * c0;
      a0 = cscale(cconj(L.bins[tid]), v0), a5 = cscale(cconj(L.bins[tid]), v5);
    }
    a0.x = block_sum(a0.x, L.red), a0.y = block_sum(a0.y, L.red), a5.x = block_sum(a5.x, L.red), a5.y = block_sum(a5.y, L.red);
    const float r0 = sqrtf(a0.x * a0.x + a0.y * a0.y), r5 = sqrtf(a5.x * a5.x + a5.y * a5.y);
    const float ratio = r0 > r5 ? r0 / r5 : r5 / r0;
    o.sf = r0 > r5 ? 0 : 5, o.corr = ratio;
    if (ratio > 1.2f) o.det = 1;
  } else {
    // extract_pair_sss (find_sss.c:65-95): even and odd bins, each scaled to unit power and unmasked with c0 / c1
    if (tid < 2) {
      float pw = 0.f;
      for (int i = 0; i < 31; i++) pw += L.bins[2 * i + tid].x * L.bins[2 * i + tid].x + L.bins[2 * i + tid].y * L.bins[2 * i + tid].y;
      pw /= 31.f;
      L.scale[tid] = (float)(1.0 / (double)(pw != 0.f ? sqrtf(pw) : 1.f));
    }
    __syncthreads();
    if (tid < 62) {
      const uint32_t w = tid / 31, i = tid % 31;
      L.y[w][i]        = cscale(cscale(L.bins[2 * i + w], L.scale[w]), p.c[(r.N_id_2 * 2 + w) * 31 + i]);
    }
    __syncthreads();
    const uint32_t m0  = sss_half(p, L.y[0], L.corr);
    const float    m0v = L.corr[m0];
    __syncthreads();
    if (tid < 31) L.y[1][tid] = cscale(L.y[1][tid], p.z1[m0 * 31 + tid]);
    __syncthreads();
    const uint32_t m1  = sss_half(p, L.y[1], L.corr);
    const float    m1v = L.corr[m1];
    __syncthreads();
    const float corr = m0v + m1v;
    o.m0 = m0, o.m1 = m1, o.sf = m1 > m0 ? 0 : 5, o.corr = corr;
    int id = -1; // srslte_sss_N_id_1 (sss.c:136-154)
    if (corr > p.sss_threshold) {
      if (m1 > m0) {
        if (m0 < 30 && m1 - 1 < 30) id = p.nid1[m0 * 30 + m1 - 1];
      } else if (m1 < 30 && m0 - 1 < 30) {
        id = p.nid1[m1 * 30 + m0 - 1];
      }
    }
    if (id >= 0) o.det = 1, o.id = id;
  }
  return o;
}

// TR: the row is the track's srslte_sync_t after this call (R = srslte_hip_sync_track_res_t); else the first call of a reset object
template <bool TR, typename R>
__device__ __forceinline__ void decide_body(const SyncParams& p, const SyncRow* __restrict__ rows, const cf32* __restrict__ in, R* __restrict__ res,
                                            const TrackParams& t, DecideLds& L)
{
  const SyncRow  r   = rows[blockIdx.x];
  const cf32*    x   = in + (size_t)r.item * p.in_stride;
  const float*   A   = (TR && t.avg) ? t.avg + (size_t)r.track * p.nout : p.avg + (size_t)blockIdx.x * p.nout;
  const uint32_t tid = threadIdx.x, N = p.N, fo = r.find_offset;
  const int      nout = (int)p.nout;
  // The track's state: the stages read only what steers them - the CP-CFO mean (track_cp_kernel left it in p.cfo_cp), the PSS-CFO mean and
  // the carried cp. They note in wr what the call writes (WR_*), and thread 0 merges that into the state at the end: the row shows the
  // previous value of whatever the call left alone.
  enum : uint32_t { WR_PEAK = 1, WR_AVAIL = 2, WR_SSS = 4, WR_ID = 8, WR_FT = 16, WR_CP = 32, WR_PSS = 64 };
  const TrackState* const s0 = TR ? t.st + r.track : nullptr;
  uint32_t                wr = 0;
  const float cfo_cp   = p.cfo_cp_enable ? p.cfo_cp[r.item] : 0.f;
  const float f_cp   = p.cfo_cp_enable ? -cfo_cp / (float)N : 0.f;
  auto        Aat    = [&](int i) -> float { return (i >= 0 && i < nout) ? A[i] : 0.f; }; // conv_output_avg is zero where nothing was written

  // the peak: first maximum over the tiles
  float    pv = -INFINITY;
  uint32_t pi = NO_INDEX;
  for (uint32_t tl = tid; tl < p.ntiles; tl += SYNC_THREADS) {
    const float2   tm = p.tile_max[(size_t)blockIdx.x * p.ntiles + tl];
    const uint32_t ti = __float_as_uint(tm.y);
    if (tm.x > pv || (tm.x == pv && ti < pi)) pv = tm.x, pi = ti;
  }
  block_argmax<SYNC_THREADS>(pv, pi, L.v, L.i);
  const int   peak = pi == NO_INDEX ? 0 : (int)pi;
  const float cpk  = Aat(peak);

  // compute_peak_sidelobe (pss.c:412-441); the reference is handed no output for it when threshold is 0: a track keeps its previous value
  float peak_value = 0.f;
  if (p.threshold > 0.f) {
    wr |= WR_PEAK;
    peak_value = cpk / side_lobe<SYNC_THREADS>(Aat, (uint32_t)peak, p.nout + 1, L.v, L.i); // conv_output_len of pss.c is nout + 1
  }
  const bool     found    = peak_value >= p.threshold || p.threshold == 0.f;
  const uint32_t peak_pos = (uint32_t)peak + (p.track ? N : 0u);
  const uint32_t tot      = peak_pos + fo;

  srslte_hip_sync_res_t o;
  o.ret = 0, o.peak_pos = peak_pos, o.peak_value = peak_value, o.corr_peak = cpk;
  o.cfo_cp = cfo_cp, o.cfo_pss = TR ? s0->cfo_pss_mean : 0.f;
  o.sss_available = 0, o.sss_detected = 0, o.m0 = 0, o.m1 = 0, o.sf_idx = 0;
  o.N_id_1 = r.N_id_1 >= 0 ? r.N_id_1 : -1;
  o.sss_corr = 0.f, o.cp = TR ? s0->cp : p.cp;
  if (r.N_id_1 >= 0) wr |= WR_ID; // srslte_sync_set_N_id_1 before the call
  float cfo_pss_inst = 0.f, trial_corr0 = NAN, trial_corr1 = NAN, m_norm = 0.f, m_ext = 0.f, r_norm = 0.f, r_ext = 0.f;
  int   frame_type = 0;

  if (found) {
    // PSS-based CFO on the symbol that ends at the peak (sync.c:704-726)
    if (p.cfo_pss_enable && peak_pos >= N) {
      const uint32_t b       = tot - N;
      const bool     pss_set = TR && s0->cfo_pss_is_set;
      for (uint32_t n = tid; n < N; n += SYNC_THREADS) L.sym[n] = ld_rot(x, b + n, f_cp);
      __syncthreads();
      const cf32* h = p.replica + (size_t)r.N_id_2 * N;
      cf32        y0 = make_float2(0.f, 0.f), y1 = y0;
      if (p.pss_filt_enable) {
        dft62(p, L.sym, L.part, L.bins);
        const cf32* H = p.half + (size_t)r.N_id_2 * 2 * 62;
        if (tid < 62) y0 = cmul(L.bins[tid], H[tid]), y1 = cmul(L.bins[tid], H[62 + tid]);
      } else {
        for (uint32_t n = tid; n < N / 2; n += SYNC_THREADS) y0 = cadd(y0, cmul(h[n], L.sym[n])), y1 = cadd(y1, cmul(h[N / 2 + n], L.sym[N / 2 + n]));
      }
      y0.x = block_sum(y0.x, L.red), y0.y = block_sum(y0.y, L.red), y1.x = block_sum(y1.x, L.red), y1.y = block_sum(y1.y, L.red);
      const cf32 z = cmulconj(y1, y0); // conjf(y0) * y1 (pss.c:619)
      cfo_pss_inst = (float)(atan2((double)z.y, (double)z.x) / M_PI);
      if constexpr (TR) { // the first estimate is the mean; later ones are averaged into it while under 7 kHz (sync.c:715-720)
        if (!pss_set)
          o.cfo_pss = cfo_pss_inst;
        else if (15000 * fabsf(cfo_pss_inst) < 7000)
          o.cfo_pss = t.cfo_alpha * cfo_pss_inst + (1 - t.cfo_alpha) * o.cfo_pss;
        wr |= WR_PSS;
      } else {
        o.cfo_pss = cfo_pss_inst;
      }
    }
    if (tot >= 2 * (N + p.cpe)) {
      if (p.sss_en) {
        o.sss_available = 1, wr |= WR_AVAIL;
        const float f_pss = p.cfo_pss_enable ? -o.cfo_pss / (float)N : 0.f;
        const int   cp_sz = o.cp == 0 ? (int)p.cpn : (int)p.cpe; // the configured CP, or the one the track's last detect_cp left
        if constexpr (!TR) {
          const int64_t sss_idx = (int64_t)tot - 2 * ((int64_t)N + cp_sz) + cp_sz;
          if (sss_idx >= 0) {
            const SssOut q = sss_trial(p, r, x, (uint32_t)sss_idx, f_cp, f_pss, L);
            o.m0 = q.m0, o.m1 = q.m1;
            if (q.det) o.sss_detected = 1, o.sf_idx = q.sf, o.N_id_1 = q.id, o.sss_corr = q.corr;
          } else {
            o.sss_available = 0;
          }
        } else {
          // sync.c:751-808: the trials of the frame mode, FDD then TDD; a trial whose symbol would start before the item does not run
          SssOut w   = {};
          int    wf  = -1; // the trial that wins so far
#pragma unroll
          for (int f = 0; f < 2; f++) {
            if (t.frame_mode != 2 && (uint32_t)f != t.frame_mode) continue;
            const int64_t sss_idx = (int64_t)tot - (f ? 4 : 2) * ((int64_t)N + cp_sz) + cp_sz;
            if (sss_idx >= 0) {
              const SssOut q = sss_trial(p, r, x, (uint32_t)sss_idx, f_cp, f_pss, L);
              if (f) trial_corr1 = q.corr;
              else trial_corr0 = q.corr;
              o.sss_detected |= q.det;
              if (wf < 0 || !(w.corr > q.corr)) w = q, wf = f; // FDD wins when sss_corr[0] > sss_corr[1], otherwise TDD (sync.c:785-795)
            } else {
              o.sss_available = 0;
            }
          }
          if (wf >= 0) { // the FDD trial always has room here, so a TDD trial that did not run cannot win
            o.m0 = w.m0, o.m1 = w.m1;
            if (t.frame_mode == 2) {
              frame_type = wf, o.sf_idx = w.sf + (uint32_t)wf, o.sss_corr = w.corr, wr |= WR_SSS | WR_FT;
              if (w.id >= 0) o.N_id_1 = w.id, wr |= WR_ID; // a winning m0 / m1 trial that detected nothing leaves the previous N_id_1
            } else if (w.det) {
              o.sf_idx = w.sf + (uint32_t)wf, o.N_id_1 = w.id, o.sss_corr = w.corr, wr |= WR_SSS | WR_ID;
            }
          }
        }
      }
      if (p.detect_cp) { // srslte_sync_detect_cp (sync.c:440-495); M_norm_avg = M_ext_avg = 0 before the first call
        uint32_t ns = tot / (N + p.cpe);
        if (ns > 3) ns = 3;
        o.cp = 0, wr |= WR_CP;
        if (ns > 0) {
          float Rr[2], M[2];
#pragma unroll
          for (int e = 0; e < 2; e++) {
            const uint32_t cpl = e ? p.cpe : p.cpn, b = tot - ns * (N + cpl);
            float          rr = 0.f, cc = 0.f;
            for (uint32_t u = tid; u < ns * cpl; u += SYNC_THREADS) {
              const uint32_t i0 = b + (u / cpl) * (N + cpl) + u % cpl;
              const cf32     a = ld_rot(x, i0, f_cp), c = ld_rot(x, i0 + N, f_cp);
              rr += c.x * a.x + c.y * a.y; // Re(x[N + i] conj(x[i]))
              cc += a.x * a.x + a.y * a.y;
            }
            rr = block_sum(rr, L.red), cc = block_sum(cc, L.red);
            const float m = cc > 0.f ? rr / cc : 0.f;
            Rr[e]         = rr;
            M[e]          = TR ? m / (float)ns : (float)(0.1 * (double)(m / (float)ns) + (1 - 0.1) * 0.0);
          }
          if constexpr (TR)
            m_norm = M[0], m_ext = M[1], r_norm = Rr[0], r_ext = Rr[1]; // thread 0 averages and decides below
          else
            o.cp = M[0] > M[1] ? 0 : M[0] < M[1] ? 1 : Rr[0] > Rr[1] ? 0 : 1;
        } else {
          wr &= ~(uint32_t)WR_CP;
        }
      }
      o.ret = 1;
    } else {
      o.ret = 2;
    }
  }
  if constexpr (!TR) {
    o.cfo     = o.cfo_cp + o.cfo_pss;
    o.cell_id = (o.N_id_1 >= 0 && o.N_id_1 < 168) ? 3 * o.N_id_1 + (int32_t)r.N_id_2 : -1;
    if (tid == 0) res[blockIdx.x] = o;
  } else if (tid == 0) {
    TrackState* const sp = t.st + rows[blockIdx.x].track;
    TrackState        st = *sp;
    if (wr & WR_PEAK) st.peak_value = o.peak_value;
    if (wr & WR_PSS) st.cfo_pss_mean = o.cfo_pss, st.cfo_pss_is_set = 1;
    if (wr & WR_AVAIL) st.sss_available = o.sss_available;
    if (wr & WR_SSS) st.sf_idx = o.sf_idx, st.sss_corr = o.sss_corr;
    if (wr & WR_ID) st.N_id_1 = o.N_id_1;
    if (wr & WR_FT) st.frame_type = frame_type;
    if (p.detect_cp && o.ret == 1) {
      st.cp = 0; // fewer than one symbol before the peak (not reachable once ret is 1): normal, the averages untouched
      if (wr & WR_CP) {
        st.M_norm_avg = (float)(0.1 * (double)m_norm + (1 - 0.1) * (double)st.M_norm_avg);
        st.M_ext_avg  = (float)(0.1 * (double)m_ext + (1 - 0.1) * (double)st.M_ext_avg);
        st.cp         = st.M_norm_avg > st.M_ext_avg ? 0 : st.M_norm_avg < st.M_ext_avg ? 1 : r_norm > r_ext ? 0 : 1;
      }
    }
    st.nof_calls++;
    *sp = st;
    R w;
    w.r            = o;
    w.r.peak_value = st.peak_value, w.r.cfo_cp = st.cfo_cp_mean, w.r.cfo_pss = st.cfo_pss_mean, w.r.cfo = st.cfo_cp_mean + st.cfo_pss_mean;
    w.r.sss_available = st.sss_available, w.r.sf_idx = st.sf_idx, w.r.N_id_1 = st.N_id_1, w.r.sss_corr = st.sss_corr, w.r.cp = st.cp;
    w.r.cell_id = (st.N_id_1 >= 0 && st.N_id_1 < 168) ? 3 * st.N_id_1 + (int32_t)r.N_id_2 : -1;
    w.frame_type = st.frame_type, w.sss_corr_trial[0] = trial_corr0, w.sss_corr_trial[1] = trial_corr1, w.nof_calls = st.nof_calls;
    w.cfo_cp_inst = p.cfo_cp_enable ? st.cfo_cp_inst : 0.f, w.cfo_pss_inst = cfo_pss_inst, w.M_norm_avg = st.M_norm_avg, w.M_ext_avg = st.M_ext_avg;
    res[blockIdx.x] = w;
  }
}
// 21.6 KB of LDS admit seven workgroups per CU: the register budget of seven waves per SIMD, which the kernel has always met
__global__ __launch_bounds__(SYNC_THREADS, 7) void sync_decide_kernel(SyncParams p, const SyncRow* __restrict__ rows, const cf32* __restrict__ in,
                                                                  srslte_hip_sync_res_t* __restrict__ res)
{
  __shared__ DecideLds L;
  decide_body<false>(p, rows, in, res, TrackParams{}, L);
}
__global__ __launch_bounds__(SYNC_THREADS) void track_decide_kernel(SyncParams p, TrackParams t, const SyncRow* __restrict__ rows,
                                                                   const cf32* __restrict__ in, srslte_hip_sync_track_res_t* __restrict__ res)
{
  __shared__ DecideLds L;
  decide_body<true>(p, rows, in, res, t, L);
}

// srslte_sync_reset (1), srslte_sync_cfo_reset (2), everything else back to the created state (4); one workgroup per track
__global__ __launch_bounds__(SYNC_THREADS) void track_reset_kernel(TrackParams t, const uint32_t* __restrict__ idx, uint32_t nout, uint32_t flags, int cp)
{
  const uint32_t k = idx ? idx[blockIdx.x] : blockIdx.x;
  if ((flags & 1u) && t.avg)
    for (uint32_t i = threadIdx.x; i < nout; i += SYNC_THREADS) t.avg[(size_t)k * nout + i] = 0.f;
  if (threadIdx.x == 0) {
    TrackState s = t.st[k];
    if (flags & 1u) s.M_norm_avg = 0.f, s.M_ext_avg = 0.f;
    if (flags & 2u) s.cfo_cp_mean = 0.f, s.cfo_pss_mean = 0.f, s.cfo_cp_is_set = 0, s.cfo_pss_is_set = 0;
    if (flags & 4u) {
      s.cp = cp, s.N_id_1 = -1, s.sf_idx = 0, s.sss_corr = 0.f, s.peak_value = 0.f, s.sss_available = 0, s.nof_calls = 0, s.cfo_cp_inst = 0.f;
      s.frame_type = t.frame_mode == 1 ? 1 : 0;
    }
    t.st[k] = s;
  }
}

// srslte_sync_copy_cfo (sync.c:354-360): the two means, and both is_set flags cleared; idx [2][n]: destination tracks, source tracks
__global__ __launch_bounds__(64) void track_copy_cfo_kernel(TrackState* dst, const TrackState* src, const uint32_t* __restrict__ idx, uint32_t n)
{
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  TrackState&      d = dst[idx[i]];
  const TrackState s = src[idx[n + i]];
  d.cfo_cp_mean = s.cfo_cp_mean, d.cfo_pss_mean = s.cfo_pss_mean, d.cfo_cp_is_set = 0, d.cfo_pss_is_set = 0;
}

constexpr uint32_t CFO_ITEMS = 64; // frequencies a launch carries in its arguments
struct CfoFreqs {
  float f[CFO_ITEMS];
};

__global__ __launch_bounds__(256) void cfo_correct_kernel(const cf32* in, cf32* out, size_t stride, uint32_t len, CfoFreqs fr)
{
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= len) return;
  const size_t a = (size_t)blockIdx.y * stride + i;
  out[a]         = rot(in[a], fr.f[blockIdx.y], i);
}

} // namespace

struct srslte_hip_sync_s {
  srslte_hip_sync_cfg_t cfg;
  SyncParams            p;
  DescStage             desc;
  DevBuf<cf32>          replica, half, tw, cp_corr;
  DevBuf<float>         s, z1, c, avg, cfo_cp;
  DevBuf<int32_t>       nid1;
  DevBuf<float2>        tile_max;
};

// n_tracks srslte_sync_t states of one sync object's configuration; the calls' temporaries (descriptors, correlations, tile maxima) are q's
struct srslte_hip_sync_tracks_s {
  srslte_hip_sync_t*           q;
  srslte_hip_sync_tracks_cfg_t cfg;
  TrackParams                  t;
  DescStage                    idx; // track lists of reset and copy_cfo
  DevBuf<TrackState>           st;
  DevBuf<float>                avg;
};

extern "C" {

srslte_hip_sync_t* srslte_hip_sync_create(const srslte_hip_sync_cfg_t* cfg)
{
  if (!sync_cfg_valid(cfg)) {
    hip_log("[srslte_hip] sync: invalid configuration (TDD and decimation are not supported; see phy_hip.h for the sizes)\n");
    return nullptr;
  }
  auto* q = new srslte_hip_sync_s();
  q->cfg  = *cfg;
  SyncTables t;
  sync_tables(cfg->fft_size, t);
  SyncParams&    p    = q->p;
  const uint32_t N    = cfg->fft_size, rows = 3 * cfg->max_items;
  p.N = N, p.max_offset = cfg->max_offset, p.track = cfg->max_offset < N ? 1u : 0u;
  p.nout    = p.track ? cfg->max_offset - 1 : cfg->max_offset + N - 2;
  p.ntiles  = (p.nout + SYNC_TILE - 1) / SYNC_TILE;
  p.cpn = (uint32_t)lte_cp_len((int)N, 144), p.cpe = (uint32_t)lte_cp_len((int)N, 512);
  p.cp_nsym = cfg->cfo_cp_nsymbols, p.cp = cfg->cp;
  p.detect_cp = cfg->detect_cp, p.sss_en = cfg->sss_en, p.cfo_cp_enable = cfg->cfo_cp_enable, p.cfo_pss_enable = cfg->cfo_pss_enable;
  p.pss_filt_enable = cfg->pss_filt_enable, p.sss_alg = cfg->sss_alg;
  p.threshold = cfg->threshold, p.sss_threshold = cfg->sss_threshold;
  const float alpha = cfg->ema_alpha == 0.f ? 0.2f : cfg->ema_alpha;
  p.alpha           = (alpha < 1.0f && alpha > 0.0f) ? alpha : 0.f; // pss.c:496-503
  const size_t M    = cfg->max_offset < N ? cfg->max_offset : N;
  if (q->replica.upload(t.replica) || q->half.upload(t.half) || q->tw.upload(t.tw) || q->s.upload(t.s) || q->z1.upload(t.z1) || q->c.upload(t.c) ||
      q->nid1.upload(t.nid1) || q->avg.alloc((size_t)rows * p.nout) || q->tile_max.alloc((size_t)rows * p.ntiles) || q->cfo_cp.alloc(cfg->max_items) ||
      q->cp_corr.alloc(cfg->max_items * M) || q->desc.init(sizeof(SyncRow) * rows) ||
      hipMemset(q->cfo_cp.get(), 0, sizeof(float) * cfg->max_items) != hipSuccess ||
      hipMemset(q->cp_corr.get(), 0, sizeof(cf32) * cfg->max_items * M) != hipSuccess) {
    hip_log("[srslte_hip] sync: device allocation failed\n");
    delete q;
    return nullptr;
  }
  p.replica = q->replica, p.half = q->half, p.tw = q->tw, p.s = q->s, p.z1 = q->z1, p.c = q->c, p.nid1 = q->nid1;
  p.avg = q->avg, p.tile_max = q->tile_max, p.cfo_cp = q->cfo_cp, p.cp_corr = q->cp_corr;
  return q;
}

void srslte_hip_sync_destroy(srslte_hip_sync_t* q) { delete q; }

int srslte_hip_sync_find_batch(srslte_hip_sync_t* q, const void* d_in, size_t in_stride, const srslte_hip_sync_item_t* items, uint32_t n,
                               srslte_hip_sync_res_t* d_res, void* stream)
{
  if (!q || (n && (!d_in || !d_res || !items))) return SRSLTE_ERROR_INVALID_INPUTS;
  if (int r = srslte_hip_sync_check(&q->cfg, in_stride, items, n)) return r;
  if (n == 0) return SRSLTE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  SyncRow*    h  = nullptr;
  if (int r = q->desc.begin(&h)) return r;
  uint32_t rows = 0;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t v0 = items[i].N_id_2 == 3 ? 0 : items[i].N_id_2, v1 = items[i].N_id_2 == 3 ? 2 : items[i].N_id_2;
    uint32_t       m0 = 0, m1 = 0;
    if (items[i].N_id_1 >= 0) sync_m0m1((uint32_t)items[i].N_id_1, &m0, &m1);
    for (uint32_t v = v0; v <= v1; v++) h[rows++] = {i, v, items[i].find_offset, items[i].N_id_1 >= 0 ? items[i].N_id_1 : -1, m0, m1, 0u, 0u};
  }
  if (int r = q->desc.commit(sizeof(SyncRow) * rows, st)) return r;
  SyncParams p = q->p;
  p.in_stride  = in_stride;
  if (p.cfo_cp_enable) {
    hipLaunchKernelGGL(sync_cp_kernel, dim3(n), dim3(SYNC_THREADS), 0, st, p, (const cf32*)d_in);
    LAUNCH_CHECK();
  }
  const size_t lds = sizeof(cf32) * (2 * (size_t)p.N + SYNC_TILE - 1);
  hipLaunchKernelGGL(sync_corr_kernel, dim3(p.ntiles, rows), dim3(SYNC_THREADS), lds, st, p, q->desc.dev<SyncRow>(), (const cf32*)d_in);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(sync_decide_kernel, dim3(rows), dim3(SYNC_THREADS), 0, st, p, q->desc.dev<SyncRow>(), (const cf32*)d_in, d_res);
  LAUNCH_CHECK();
  return SRSLTE_SUCCESS;
}

srslte_hip_sync_tracks_t* srslte_hip_sync_tracks_create(srslte_hip_sync_t* q, const srslte_hip_sync_tracks_cfg_t* cfg)
{
  if (!q || !sync_tracks_cfg_valid(cfg)) {
    hip_log("[srslte_hip] sync tracks: invalid configuration (n_tracks 1..65535, frame_mode 0..2, cfo_ema_alpha >= 0)\n");
    return nullptr;
  }
  auto* k = new srslte_hip_sync_tracks_s();
  k->q = q, k->cfg = *cfg;
  const bool ema = q->p.alpha != 0.f; // pss.c:496: an average is kept only with 0 < ema_alpha < 1
  if (k->st.alloc(cfg->n_tracks) || (ema && k->avg.alloc((size_t)cfg->n_tracks * q->p.nout)) || k->idx.init(sizeof(uint32_t) * 2 * cfg->n_tracks)) {
    hip_log("[srslte_hip] sync tracks: device allocation failed\n");
    delete k;
    return nullptr;
  }
  k->t.st = k->st, k->t.avg = ema ? k->avg.get() : nullptr, k->t.frame_mode = cfg->frame_mode;
  k->t.cfo_alpha = cfg->cfo_ema_alpha == 0.f ? 0.1f : cfg->cfo_ema_alpha; // CFO_EMA_ALPHA (sync.c:34)
  if (srslte_hip_sync_tracks_reset(k, nullptr, cfg->n_tracks, 7, nullptr) || hipStreamSynchronize(nullptr) != hipSuccess) {
    delete k;
    return nullptr;
  }
  return k;
}

void srslte_hip_sync_tracks_destroy(srslte_hip_sync_tracks_t* k) { delete k; }

int srslte_hip_sync_track_batch(srslte_hip_sync_tracks_t* k, const void* d_in, size_t in_stride, const srslte_hip_sync_track_item_t* items, uint32_t n,
                                srslte_hip_sync_track_res_t* d_res, void* stream)
{
  if (!k || (n && (!d_in || !d_res || !items))) return SRSLTE_ERROR_INVALID_INPUTS;
  srslte_hip_sync_t* q = k->q;
  if (int r = srslte_hip_sync_tracks_check(&q->cfg, &k->cfg, in_stride, items, n)) return r;
  if (n == 0) return SRSLTE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  SyncRow*    h  = nullptr;
  if (int r = q->desc.begin(&h)) return r;
  for (uint32_t i = 0; i < n; i++) {
    uint32_t m0 = 0, m1 = 0;
    if (items[i].N_id_1 >= 0) sync_m0m1((uint32_t)items[i].N_id_1, &m0, &m1);
    h[i] = {i, items[i].N_id_2, items[i].find_offset, items[i].N_id_1 >= 0 ? items[i].N_id_1 : -1, m0, m1, items[i].track, 0u};
  }
  if (int r = q->desc.commit(sizeof(SyncRow) * n, st)) return r;
  SyncParams p = q->p;
  p.in_stride  = in_stride;
  if (p.cfo_cp_enable) {
    hipLaunchKernelGGL(track_cp_kernel, dim3(n), dim3(SYNC_THREADS), 0, st, p, k->t, q->desc.dev<SyncRow>(), (const cf32*)d_in);
    LAUNCH_CHECK();
  }
  const size_t lds = sizeof(cf32) * (2 * (size_t)p.N + SYNC_TILE - 1);
  hipLaunchKernelGGL(track_corr_kernel, dim3(p.ntiles, n), dim3(SYNC_THREADS), lds, st, p, k->t, q->desc.dev<SyncRow>(), (const cf32*)d_in);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(track_decide_kernel, dim3(n), dim3(SYNC_THREADS), 0, st, p, k->t, q->desc.dev<SyncRow>(), (const cf32*)d_in, d_res);
  LAUNCH_CHECK();
  return SRSLTE_SUCCESS;
}

int srslte_hip_sync_tracks_reset(srslte_hip_sync_tracks_t* k, const uint32_t* idx, uint32_t n, uint32_t flags, void* stream)
{
  if (!k || flags > 7 || n > k->cfg.n_tracks) return SRSLTE_ERROR_INVALID_INPUTS;
  if (idx)
    for (uint32_t i = 0; i < n; i++)
      if (idx[i] >= k->cfg.n_tracks) return SRSLTE_ERROR_INVALID_INPUTS;
  if (!idx) n = k->cfg.n_tracks; // all of them
  if (n == 0 || flags == 0) return SRSLTE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  if (idx) {
    uint32_t* h = nullptr;
    if (int r = k->idx.begin(&h)) return r;
    memcpy(h, idx, sizeof(uint32_t) * n);
    if (int r = k->idx.commit(sizeof(uint32_t) * n, st)) return r;
  }
  hipLaunchKernelGGL(track_reset_kernel, dim3(n), dim3(SYNC_THREADS), 0, st, k->t, idx ? k->idx.dev<uint32_t>() : nullptr, k->q->p.nout, flags, k->q->p.cp);
  LAUNCH_CHECK();
  return SRSLTE_SUCCESS;
}

int srslte_hip_sync_tracks_copy_cfo(srslte_hip_sync_tracks_t* dst, const uint32_t* dst_idx, srslte_hip_sync_tracks_t* src, const uint32_t* src_idx,
                                    uint32_t n, void* stream)
{
  if (!dst || !src || (n && (!dst_idx || !src_idx)) || n > dst->cfg.n_tracks) return SRSLTE_ERROR_INVALID_INPUTS;
  for (uint32_t i = 0; i < n; i++) {
    if (dst_idx[i] >= dst->cfg.n_tracks || src_idx[i] >= src->cfg.n_tracks) return SRSLTE_ERROR_INVALID_INPUTS;
    for (uint32_t j = 0; j < i; j++)
      if (dst_idx[j] == dst_idx[i]) return SRSLTE_ERROR_INVALID_INPUTS;
  }
  if (n == 0) return SRSLTE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  uint32_t*   h  = nullptr;
  if (int r = dst->idx.begin(&h)) return r;
  memcpy(h, dst_idx, sizeof(uint32_t) * n), memcpy(h + n, src_idx, sizeof(uint32_t) * n);
  if (int r = dst->idx.commit(sizeof(uint32_t) * 2 * n, st)) return r;
  hipLaunchKernelGGL(track_copy_cfo_kernel, dim3((n + 63) / 64), dim3(64), 0, st, dst->st.get(), (const TrackState*)src->st.get(),
                     dst->idx.dev<uint32_t>(), n);
  LAUNCH_CHECK();
  return SRSLTE_SUCCESS;
}

int srslte_hip_sync_tracks_read(srslte_hip_sync_tracks_t* k, uint32_t track, srslte_hip_sync_track_state_t* h_state)
{
  if (!k || !h_state || track >= k->cfg.n_tracks) return SRSLTE_ERROR_INVALID_INPUTS;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(h_state, k->st.get() + track, sizeof(*h_state), hipMemcpyDeviceToHost));
  return SRSLTE_SUCCESS;
}

int srslte_hip_cfo_correct_batch(const void* d_in, void* d_out, size_t stride, uint32_t len, uint32_t n, const float* freq, void* stream)
{
  if ((n && len && (!d_in || !d_out || !freq)) || (n > 1 && stride < len)) return SRSLTE_ERROR_INVALID_INPUTS;
  if (n == 0 || len == 0) return SRSLTE_SUCCESS;
  for (uint32_t b = 0; b < n; b += CFO_ITEMS) {
    const uint32_t nb = n - b < CFO_ITEMS ? n - b : CFO_ITEMS;
    CfoFreqs       fr;
    for (uint32_t i = 0; i < CFO_ITEMS; i++) fr.f[i] = i < nb ? freq[b + i] : 0.f;
    hipLaunchKernelGGL(cfo_correct_kernel, dim3((len + 255) / 256, nb), dim3(256), 0, (hipStream_t)stream, (const cf32*)d_in + (size_t)b * stride,
                       (cf32*)d_out + (size_t)b * stride, stride, len, fr);
    LAUNCH_CHECK();
  }
  return SRSLTE_SUCCESS;
}

int srslte_hip_sync_cp_corr(srslte_hip_sync_t* q, uint32_t item, void* h_corr)
{
  if (!q || !h_corr || item >= q->cfg.max_items) return SRSLTE_ERROR_INVALID_INPUTS;
  const size_t M = q->cfg.max_offset < q->cfg.fft_size ? q->cfg.max_offset : q->cfg.fft_size;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(h_corr, q->cp_corr.get() + item * M, sizeof(cf32) * M, hipMemcpyDeviceToHost));
  return SRSLTE_SUCCESS;
}

} // extern "C"
