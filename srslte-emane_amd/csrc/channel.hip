// Batched channel emulator for gfx950: fading -> delay -> HST -> RLF (channel.cc:124-158) -> AWGN, nof_channels x nof_calls blocks per call.
//
// Replaces srslte_channel_fading_execute (fading.c:249-275), srslte_channel_delay_execute (delay.c:99-126), srslte_channel_hst_execute
// (hst.c:48-80) and srslte_channel_rlf_execute (rlf.c:31-44) behind srslte::channel::run; the noise stage is ours (ch_awgn.c draws from rand()).
//
// Two launches per call (three with state to carry):
//   ch_fading_kernel  one workgroup per (segment, block, channel): the segment's <= N/4 samples zero-padded to N, FFT, times the frequency response
//                     H of the segment's time, inverse FFT, the N results to a scratch row. H[k] = sum_taps a0_tap E_tap[k] per bin (fading.c:90-118
//                     without the recursive oscillator): E_tap[k] = exp(-j 2 pi k O_tap) is a table made once, a0_tap = amp / N exp(-j phi) with
//                     phi = (float)(a sin(w t + p)) evaluated in FP64 by one lane per tap.
//   ch_output_kernel  one thread per output sample: the delay line picks the source position, the overlap-add is a GATHER over the scratch rows whose
//                     segment covers it (oldest first, after the carried state: the order in which fading.c:137 accumulates), then Doppler, gating
//                     and noise. No atomics: the same bytes every run.
//   ch_carry_kernel   the N samples of overlap past the end of the call and the last delay_cap samples of the fading output, for the next call
//                     (ping-pong buffers: the kernels above read the previous call's).
#include "cf32_dev.hpp"
#include "common.hpp"
#include "dev_buf.hpp"
#include "phy_hip_internal.hpp"
#include <math.h>
#include <random>
#include <string.h>
#include <vector>

namespace {

constexpr int MAXTAPS = SRSLTE_HIP_CHANNEL_MAXTAPS;

// 36.104 B.2 (fading.c:38-51)
const int   ch_nof_taps[4]              = {1, 7, 9, 9};
const float ch_tap_delay_ns[4][MAXTAPS] = {{0, 0, 0, 0, 0, 0, 0, 0, 0},
                                           {0, 30, 70, 90, 110, 190, 410, 0, 0},
                                           {0, 30, 150, 310, 370, 710, 1090, 1730, 2510},
                                           {0, 50, 120, 200, 230, 500, 1600, 2300, 5000}};
const float ch_tap_power_db[4][MAXTAPS] = {{0, 0, 0, 0, 0, 0, 0, 0, 0},
                                           {0.0f, -1.0f, -2.0f, -3.0f, -8.0f, -17.2f, -20.8f, 0, 0},
                                           {0.0f, -1.5f, -1.4f, -3.6f, -0.6f, -9.1f, -7.0f, -12.0f, -16.9f},
                                           {-1.0f, -1.0f, -1.0f, 0.0f, 0.0f, 0.0f, -3.0f, -5.0f, -7.0f}};

// What the host works out per block (delay.c:26-47, hst.c:52-78, rlf.c:34-39) and the device reads
struct ChBlock {
  double t;     // fading time of the block's first segment
  int    delay; // samples
  int    avail; // samples the delay line holds when the block starts (the previous block's delay)
  float  cfo;   // -fs / srate
  float  gate;  // 1.0f or 0.0f
};

struct ChGeom {
  int      N, Nq, ntaps, nseg; // Nq = N / 4 samples per segment, nseg segments per block
  int      nb, len;            // blocks of the call and their length
  int      fading, delay, hst, rlf, awgn;
  int      dcap;               // delay-line history kept per channel
  float    dt;                 // (float)Nq / (float)srate: what fading.c:266 adds per segment
  float    sigma;              // sqrt(n0 / 2)
  uint32_t seed;
  uint64_t sample0;            // samples per channel before this call
  uint64_t in_cs, in_bs, out_cs, out_bs;
};

// exp(-j 2 pi k / N) from the table, conjugated for the inverse transform
__device__ __forceinline__ cf32 twid(const cf32* __restrict__ tw, int i, float sgn)
{
  cf32 w = tw[i];
  w.y    = -sgn * w.y;
  return w;
}

constexpr int ilog2(int n) { return n <= 1 ? 0 : 1 + ilog2(n / 2); }

// One radix-4 Stockham pass over N points (fft.hip's indexing: butterfly j reads x[j + r N/4], twiddles by w^(r k), k = j mod Ns, writes
// y[(j / Ns) 4 Ns + k + r Ns]); the three twiddles are read from the table, not multiplied up.
template <int N, int T, typename Ld, typename St>
__device__ __forceinline__ void ch_r4_pass(int Ns, float sgn, const cf32* __restrict__ tw, Ld ld, St st)
{
  constexpr int nb = N / 4;
  const int     tstep = nb / Ns;
  for (int j = threadIdx.x; j < nb; j += T) {
    const int k = j & (Ns - 1);
    cf32      v0 = ld(j), v1 = ld(j + nb), v2 = ld(j + 2 * nb), v3 = ld(j + 3 * nb);
    if (k != 0) {
      v1 = cmul(v1, twid(tw, k * tstep, sgn));
      v2 = cmul(v2, twid(tw, 2 * k * tstep, sgn));
      v3 = cmul(v3, twid(tw, 3 * k * tstep, sgn));
    }
    const cf32 a = cadd(v0, v2), b = csub(v0, v2), c = cadd(v1, v3), e = csub(v1, v3);
    const cf32 d  = make_float2(-sgn * e.y, sgn * e.x); // e * (j sgn)
    const int  j0 = (j - k) * 4 + k;
    st(j0, cadd(a, c));
    st(j0 + Ns, cadd(b, d));
    st(j0 + 2 * Ns, csub(a, c));
    st(j0 + 3 * Ns, csub(b, d));
  }
}

// The closing radix-2 pass of an odd power of two (Ns = N / 2)
template <int N, int T, typename Ld, typename St>
__device__ __forceinline__ void ch_r2_pass(float sgn, const cf32* __restrict__ tw, Ld ld, St st)
{
  constexpr int nb = N / 2;
  for (int j = threadIdx.x; j < nb; j += T) {
    const cf32 a = ld(j), b = cmul(ld(j + nb), twid(tw, j, sgn));
    st(j, cadd(a, b));
    st(j + nb, csub(a, b));
  }
}

// Unnormalised N-point transform, N = 2^L: L / 2 radix-4 passes and one radix-2 pass when L is odd, ping-pong between two LDS buffers; the first
// pass reads through gld, the last writes through gst (neither may be A or B).
template <int N, int T, typename GLd, typename GSt>
__device__ __forceinline__ void ch_fft(float sgn, const cf32* __restrict__ tw, cf32* A, cf32* B, GLd gld, GSt gst)
{
  constexpr int L = ilog2(N), P4 = L / 2, P = P4 + (L & 1);
  int           Ns = 1;
#pragma unroll
  for (int p = 0; p < P; p++) {
    const bool  first = p == 0, last = p == P - 1;
    const cf32* src = (p & 1) ? A : B;
    cf32*       dst = (p & 1) ? B : A;
    auto        ld  = [&](int i) { return first ? gld(i) : src[i]; };
    auto        st  = [&](int i, cf32 v) {
      if (last) {
        gst(i, v);
      } else {
        dst[i] = v;
      }
    };
    if (p < P4) {
      ch_r4_pass<N, T>(Ns, sgn, tw, ld, st);
      Ns *= 4;
    } else {
      ch_r2_pass<N, T>(sgn, tw, ld, st);
    }
    __syncthreads();
  }
}

template <int N>
constexpr int ch_threads() { return N / 4 < 64 ? 64 : N / 4; }

// grid = (nseg, nb, nof_channels). y: [channel][block][segment][N].
template <int N>
__global__ __launch_bounds__(ch_threads<N>()) void ch_fading_kernel(const cf32* __restrict__ in, cf32* __restrict__ y, ChGeom g,
                                                                    const ChBlock* __restrict__ blk, const double* __restrict__ coef,
                                                                    const float* __restrict__ amp, const cf32* __restrict__ E,
                                                                    const cf32* __restrict__ tw)
{
  constexpr int   T = ch_threads<N>();
  __shared__ cf32 A[N], B[N], F[N];
  __shared__ cf32 a0[MAXTAPS];
  const int       k = blockIdx.x, b = blockIdx.y, c = blockIdx.z, tid = threadIdx.x;
  const int       n = min(g.Nq, g.len - k * g.Nq);
  if (tid < g.ntaps) { // fading.c:85-88,:93-95 with the time of fading.c:266: k additions of the float quotient to the double
    double       t  = blk[b].t;
    const double dt = (double)g.dt;
    for (int i = 0; i < k; i++) t += dt;
    const double* cc    = coef + (size_t)c * 3 * MAXTAPS;
    const float   phase = (float)(cc[tid] * sin(cc[MAXTAPS + tid] * t + cc[2 * MAXTAPS + tid]));
    double        s, co;
    sincos((double)phase, &s, &co);
    a0[tid] = make_float2((float)(amp[tid] * co), (float)(-amp[tid] * s));
  }
  const cf32* src = in + (size_t)c * g.in_cs + (size_t)b * g.in_bs + (size_t)k * g.Nq;
  ch_fft<N, T>(
      -1.0f, tw, A, B, [&](int i) { return i < n ? src[i] : make_float2(0.f, 0.f); }, [&](int i, cf32 v) { F[i] = v; });
  // a0 and F are complete: ch_fft ends on a barrier
  const int ntaps = g.ntaps;
  cf32*     dst   = y + (((size_t)c * g.nb + b) * g.nseg + k) * N;
  ch_fft<N, T>(
      1.0f, tw, A, B,
      [&](int i) { // fading.c:103-116,:131: the response of bin i, taps summed in their order, times the spectrum
        cf32 h = make_float2(0.f, 0.f);
        for (int tp = 0; tp < ntaps; tp++) h = cadd(h, cmul(a0[tp], E[tp * N + i]));
        return cmul(F[i], h);
      },
      [&](int i, cf32 v) { dst[i] = v; });
}

// The fading filter's output at position p >= 0 of the call's sample stream (block b, sample i: p = b len + i; p may run past the call's end, into
// the overlap): the carried state, then every segment that covers p, oldest first.
__device__ __forceinline__ cf32 ch_fading_at(const ChGeom& g, const cf32* __restrict__ yc, const cf32* __restrict__ state_c, long p)
{
  cf32       acc = p < g.N ? state_c[p] : make_float2(0.f, 0.f);
  const long lo  = p - g.N + 1; // a segment covers p when it starts in [lo, p]
  const int  b0  = lo <= 0 ? 0 : (int)(lo / g.len);
  const int  b1  = min((long)g.nb - 1, p / g.len);
  for (int b = b0; b <= b1; b++) {
    const long base = (long)b * g.len;
    const int  k0   = lo <= base ? 0 : (int)((lo - base + g.Nq - 1) / g.Nq);
    const int  k1   = min((long)g.nseg - 1, (p - base) / g.Nq);
    for (int k = k0; k <= k1; k++) acc = cadd(acc, yc[((size_t)b * g.nseg + k) * g.N + (p - base - (long)k * g.Nq)]);
  }
  return acc;
}

// The signal after the fading stage at position p of the stream; p < 0 is the previous call's (hist holds its last dcap samples)
__device__ __forceinline__ cf32 ch_stage1_at(const ChGeom& g, const cf32* __restrict__ in_c, const cf32* __restrict__ yc,
                                             const cf32* __restrict__ state_c, const cf32* __restrict__ hist_c, long p)
{
  if (p < 0) return hist_c[g.dcap + p];
  if (g.fading) return ch_fading_at(g, yc, state_c, p);
  return in_c[(size_t)(p / g.len) * g.in_bs + (size_t)(p % g.len)];
}

// Philox-4x32-10 (Salmon et al., SC'11): counter (c0, c1, 0, 0), key (k0, k1); the first two output words
__device__ __forceinline__ uint2 philox2(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1)
{
  uint32_t c2 = 0, c3 = 0;
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return make_uint2(c0, c1);
}

constexpr int CH_OUT_THREADS = 256;

// grid = (ceil(len / 256), nb, nof_channels)
__global__ __launch_bounds__(CH_OUT_THREADS) void ch_output_kernel(const cf32* __restrict__ in, cf32* __restrict__ out, const cf32* __restrict__ y,
                                                                   ChGeom g, const ChBlock* __restrict__ blk, const cf32* __restrict__ state_in,
                                                                   const cf32* __restrict__ hist_in)
{
  const int i = blockIdx.x * CH_OUT_THREADS + threadIdx.x, b = blockIdx.y, c = blockIdx.z;
  if (i >= g.len) return;
  const ChBlock bk   = blk[b];
  const long    base = (long)b * g.len;
  long          p    = base + i;
  bool          zero = false;
  if (g.delay && i < bk.delay) { // delay.c:108-117: the line is first brought to `delay` samples - zeros appended behind the history when it
    if (bk.delay >= bk.avail) {  // grows, the oldest dropped when it shrinks - and read out ahead of the block's own samples
      zero = i >= bk.avail;
      p    = base - bk.avail + i;
    } else {
      p = base - bk.delay + i;
    }
  } else if (g.delay) {
    p = base + i - bk.delay;
  }
  cf32 v = make_float2(0.f, 0.f);
  if (!zero) {
    v = ch_stage1_at(g, in + (size_t)c * g.in_cs, y + (size_t)c * g.nb * g.nseg * g.N, state_in + (size_t)c * g.N,
                     hist_in + (size_t)c * g.dcap, p);
  }
  if (g.hst) { // hst.c:78: the phase cfo * i, exact in double, reduced to a turn before the sine
    double ph = (double)bk.cfo * (double)i;
    ph -= rint(ph);
    float s, co;
    sincospif((float)(2.0 * ph), &s, &co);
    v = cmul(v, make_float2(co, s));
  }
  if (g.rlf) v = make_float2(v.x * bk.gate, v.y * bk.gate); // rlf.c:39-43
  if (g.awgn) {
    const uint64_t idx = g.sample0 + (uint64_t)base + (uint64_t)i;
    const uint2    r   = philox2((uint32_t)idx, (uint32_t)(idx >> 32), g.seed, (uint32_t)c);
    const float    u1  = ((float)(r.x >> 9) + 0.5f) * (1.0f / 8388608.0f); // (0, 1), exact
    const float    u2  = (float)(r.y >> 8) * (1.0f / 16777216.0f);         // [0, 1), exact
    const float    rad = g.sigma * sqrtf(-2.0f * logf(u1));
    float          s, co;
    sincospif(2.0f * u2, &s, &co);
    v = make_float2(v.x + rad * co, v.y + rad * s);
  }
  out[(size_t)c * g.out_cs + (size_t)b * g.out_bs + i] = v;
}

// grid = (ceil((N + dcap) / 256), nof_channels): thread j < N the overlap at position P + j, P = nb len; thread N + j the fading output at
// P - dcap + j (the previous call's where that lies before this one)
__global__ __launch_bounds__(CH_OUT_THREADS) void ch_carry_kernel(const cf32* __restrict__ in, const cf32* __restrict__ y, ChGeom g,
                                                                  const cf32* __restrict__ state_in, cf32* __restrict__ state_out,
                                                                  const cf32* __restrict__ hist_in, cf32* __restrict__ hist_out)
{
  const int   j = blockIdx.x * CH_OUT_THREADS + threadIdx.x, c = blockIdx.y;
  const long  P = (long)g.nb * g.len;
  const cf32* yc = y + (size_t)c * g.nb * g.nseg * g.N;
  const cf32* sc = state_in + (size_t)c * g.N;
  const int   nstate = g.fading ? g.N : 0;
  if (j < nstate) {
    state_out[(size_t)c * g.N + j] = ch_fading_at(g, yc, sc, P + j);
  } else if (j < nstate + g.dcap) {
    const int  h = j - nstate;
    const long p = P - g.dcap + h;
    hist_out[(size_t)c * g.dcap + h] = ch_stage1_at(g, in + (size_t)c * g.in_cs, yc, sc, hist_in + (size_t)c * g.dcap, p);
  }
}

// ---------------------------------------------------------------- host side
bool model_ok(int m) { return m >= SRSLTE_HIP_CHANNEL_FADING_NONE && m <= SRSLTE_HIP_CHANNEL_FADING_ETU; }

// fading.c:162-164 for the rates whose exponent is positive; upstream converts a negative exponent to unsigned (ETU at 1.92 MHz: -4), which is
// undefined, and the floor of 64 is what it is after there
int fading_fft_size(int model, double srate)
{
  const double e = round(log2(ch_tap_delay_ns[model][ch_nof_taps[model] - 1] * 1e-9 * srate)) + 3;
  return e < 6 ? 64 : 1 << (int)e;
}

// srslte_random_uniform_real_dist (random.cpp:36-40) as libstdc++ evaluates std::uniform_real_distribution<float> on std::mt19937: one 32-bit
// draw, to float, over 2^32 (below 1 by nextafter when it rounds to 1), times the range plus the minimum
float uniform_real(std::mt19937& gen, float lo, float hi)
{
  float u = (float)gen() / 4294967296.0f;
  if (u >= 1.0f) u = nextafterf(1.0f, 0.0f);
  return u * (hi - lo) + lo;
}

void draw_coeffs(int model, float doppler, uint32_t seed, double* a, double* w, double* p)
{ // fading.c:168-175
  std::mt19937 gen(seed);
  for (int i = 0; i < ch_nof_taps[model]; i++) {
    a[i] = uniform_real(gen, 100, 2000);
    w[i] = 2.0 * M_PI * doppler / a[i];
    p[i] = uniform_real(gen, 0, (float)M_PI / 2.0f);
  }
}

// delay.c:28-35 / hst.c:52-59: the block's time within the period, in samples
uint64_t mod_nsamples(float period_s, float init_time_s, uint32_t srate, int64_t full, double frac)
{
  const uint64_t period_nsamples = (uint64_t)roundf(period_s * srate);
  const uint64_t ts_nsamples     = (uint64_t)(full * (uint64_t)(double)srate) + (uint64_t)round(frac * (double)srate) + (uint64_t)init_time_s * srate;
  return ts_nsamples - period_nsamples * (ts_nsamples / period_nsamples);
}

const char* cfg_error(const srslte_hip_channel_cfg_t* c)
{
  if (!(c->srate_hz >= 1e5 && c->srate_hz <= 1e8)) return "sample rate outside 0.1-100 MHz";
  if (c->fading_enable && !model_ok(c->fading_model)) return "unknown fading model";
  if (c->fading_enable && c->fading_model == SRSLTE_HIP_CHANNEL_FADING_NONE) return "fading enabled with model none (no filter size is defined for it)";
  if (c->fading_enable && !(c->doppler_hz >= 0.0f)) return "negative Doppler";
  if (c->delay_enable && !(c->delay_min_us >= 0.0f && c->delay_max_us >= c->delay_min_us && c->delay_max_us <= 1e5f)) return "delay range";
  if (c->delay_enable && !(roundf(c->delay_period_s * (uint32_t)c->srate_hz) >= 1.0f && c->delay_init_time_s >= 0.0f)) return "delay period / init time";
  if (c->hst_enable && !(roundf(c->hst_period_s * (uint32_t)c->srate_hz) >= 1.0f && c->hst_init_time_s >= 0.0f)) return "HST period / init time";
  if (c->rlf_enable && c->rlf_t_on_ms + c->rlf_t_off_ms == 0) return "RLF period of zero";
  if (c->awgn_enable && !(c->awgn_n0 >= 0.0f)) return "negative n0";
  return nullptr;
}

void block_params(const srslte_hip_channel_cfg_t* c, uint32_t len, uint32_t i, int64_t t_full, double t_frac, srslte_hip_channel_block_t* o)
{
  const uint32_t srate = (uint32_t)c->srate_hz;
  // srslte_timestamp_add(t0, 0, i len / srate), timestamp.c:73-84
  double       frac = t_frac + (double)((uint64_t)i * len) / c->srate_hz;
  const double r    = floor(frac);
  int64_t      full = t_full + (int64_t)r;
  frac -= r;
  o->t             = (double)full + frac; // channel.cc:136
  o->delay_samples = 0;
  o->hst_fs_hz     = 0.0f;
  o->rlf_on        = 1;
  if (c->delay_enable) { // delay.c:26-47
    const double t        = (double)mod_nsamples(c->delay_period_s, c->delay_init_time_s, srate, full, frac) / (double)srate;
    const double arg      = 2.0 * M_PI * t / (double)c->delay_period_s;
    const float  delay_us = (float)(c->delay_min_us + (c->delay_max_us - c->delay_min_us) * (1.0 + sin(arg)) / 2.0);
    o->delay_samples      = (uint32_t)round(delay_us * (double)srate / 1e6);
  }
  if (c->hst_enable) { // hst.c:52-75, ds_m = 300, dmin_m = 2
    const float t = (float)mod_nsamples(c->hst_period_s, c->hst_init_time_s, srate, full, frac) / (float)srate;
    const float T = c->hst_period_s, ds_m = 300.0f, dmin_m = 2.0f;
    float       costheta = 0;
    if (0 <= t && t <= T / 2.0f) {
      const float num = T / 4.0f - t;
      costheta        = num / sqrtf(powf(dmin_m * T / (ds_m * 2), 2.0f) + powf(num, 2.0f));
    } else if (T / 2.0f < t && t < T) {
      const float num = -1.5f / 2.0f * T + t;
      costheta        = num / sqrtf(powf(dmin_m * T / (ds_m * 2), 2.0f) + powf(num, 2.0f));
    }
    o->hst_fs_hz = c->hst_fd_hz * costheta;
  }
  if (c->rlf_enable) { // rlf.c:34-39
    const uint32_t period_ms = c->rlf_t_on_ms + c->rlf_t_off_ms;
    const double   time_ms   = (double)((full * 1000) % (int64_t)period_ms) + frac * 1000;
    o->rlf_on                = time_ms < c->rlf_t_on_ms;
  }
}

} // namespace

struct srslte_hip_channel {
  srslte_hip_channel_cfg_t cfg;
  int                      model, N, ntaps, dcap;
  std::vector<double>      coef; // [channel][a, w, p][MAXTAPS]
  const cf32*              d_tw    = nullptr;
  DevBuf<double>           d_coef;
  DevBuf<float>            d_amp;
  DevBuf<cf32>             d_E, d_y, d_state[2], d_hist[2];
  DevBuf<ChBlock>          d_blk; // [4][max_calls], one row per pinned buffer
  PinnedRing               ring;  // destroy() leaves a ring that was never initialised alone
  int                      cur     = 0; // which of d_state / d_hist the next call reads
  uint32_t                 avail   = 0; // samples in the delay line
  uint64_t                 samples = 0; // per channel, since creation or reset
  ~srslte_hip_channel() { ring.destroy(); }
};

extern "C" {

int srslte_hip_channel_fft_size_for(int fading_model, double srate_hz)
{
  if (!model_ok(fading_model) || fading_model == SRSLTE_HIP_CHANNEL_FADING_NONE || !(srate_hz >= 1e5 && srate_hz <= 1e8)) return SRSLTE_ERROR_INVALID_INPUTS;
  return fading_fft_size(fading_model, srate_hz);
}

int srslte_hip_channel_draw_coeffs(int fading_model, float doppler_hz, uint32_t seed, double a[MAXTAPS], double w[MAXTAPS], double p[MAXTAPS])
{
  if (!model_ok(fading_model) || !a || !w || !p) return SRSLTE_ERROR_INVALID_INPUTS;
  draw_coeffs(fading_model, doppler_hz, seed, a, w, p);
  return ch_nof_taps[fading_model];
}

int srslte_hip_channel_block_params(const srslte_hip_channel_cfg_t* cfg, uint32_t len, uint32_t i, int64_t t_full_secs, double t_frac_secs,
                                    srslte_hip_channel_block_t* out)
{
  if (!cfg || !out || !(t_frac_secs >= 0.0) || t_full_secs < 0) return SRSLTE_ERROR_INVALID_INPUTS;
  if (const char* e = cfg_error(cfg)) {
    hip_log("[srslte_hip] channel: %s\n", e);
    return SRSLTE_ERROR_INVALID_INPUTS;
  }
  block_params(cfg, len, i, t_full_secs, t_frac_secs, out);
  return SRSLTE_SUCCESS;
}

void srslte_hip_channel_destroy(srslte_hip_channel_t* q) { delete q; }

int srslte_hip_channel_reset(srslte_hip_channel_t* q)
{
  if (!q) return SRSLTE_ERROR_INVALID_INPUTS;
  HIP_TRY(hipDeviceSynchronize()); // calls in flight still read the state
  const size_t C = q->cfg.nof_channels;
  for (int i = 0; i < 2; i++) {
    if (q->d_state[i].get()) HIP_TRY(hipMemset(q->d_state[i].get(), 0, sizeof(cf32) * C * q->N));
    if (q->d_hist[i].get()) HIP_TRY(hipMemset(q->d_hist[i].get(), 0, sizeof(cf32) * C * q->dcap));
  }
  q->cur     = 0;
  q->avail   = 0;
  q->samples = 0;
  return SRSLTE_SUCCESS;
}

static int channel_alloc_failed()
{
  hip_log("[srslte_hip] channel: device allocation failed\n");
  return SRSLTE_ERROR;
}

// returns at the first step that fails
static int channel_init(srslte_hip_channel_t* q)
{
  const srslte_hip_channel_cfg_t& c = q->cfg;
  const size_t                    C = c.nof_channels;
  if (q->d_blk.alloc((size_t)4 * c.max_calls)) return channel_alloc_failed();
  if (q->ring.init(sizeof(ChBlock) * c.max_calls)) return SRSLTE_ERROR;
  if (c.fading_enable) {
    FftFactors f;
    if (fft_get_plan(q->N, &f, &q->d_tw)) return SRSLTE_ERROR;
    const int          N = q->N, path_delay = N / 4;
    std::vector<float> amp(MAXTAPS, 0.0f);
    std::vector<cf32>  E((size_t)q->ntaps * N);
    for (int i = 0; i < q->ntaps; i++) { // fading.c:93-97: the amplitude over N and the tap's frequency, both in float as upstream has them
      amp[i]        = powf(10.0f, ch_tap_power_db[q->model][i] / 20.0f) / N;
      const float O = (ch_tap_delay_ns[q->model][i] * 1e-9f * (float)c.srate_hz + path_delay) / (float)N;
      for (int k = 0; k < N; k++) {
        double ph = (double)O * k;
        ph -= rint(ph);
        E[(size_t)i * N + k] = make_float2((float)cos(2.0 * M_PI * ph), (float)-sin(2.0 * M_PI * ph));
      }
    }
    for (size_t ch = 0; ch < C; ch++) {
      double* cc = &q->coef[ch * 3 * MAXTAPS];
      draw_coeffs(q->model, c.doppler_hz, c.seed0 + (uint32_t)ch * c.seed_stride, cc, cc + MAXTAPS, cc + 2 * MAXTAPS);
    }
    const size_t nseg_max = (c.max_len + path_delay - 1) / path_delay;
    if (q->d_amp.upload(amp) || q->d_E.upload(E) || q->d_coef.upload(q->coef) || q->d_y.alloc(C * c.max_calls * nseg_max * N) ||
        q->d_state[0].alloc(C * N) || q->d_state[1].alloc(C * N))
      return channel_alloc_failed();
  }
  if (c.delay_enable && (q->d_hist[0].alloc(C * q->dcap) || q->d_hist[1].alloc(C * q->dcap))) return channel_alloc_failed();
  return srslte_hip_channel_reset(q);
}

int srslte_hip_channel_create(srslte_hip_channel_t** out, const srslte_hip_channel_cfg_t* cfg)
{
  if (!out || !cfg) return SRSLTE_ERROR_INVALID_INPUTS;
  *out          = nullptr;
  const char* e = cfg_error(cfg);
  if (!e && (cfg->nof_channels < 1 || cfg->nof_channels > 65535 || cfg->max_calls < 1 || cfg->max_calls > 65535 || cfg->max_len < 1 ||
             cfg->max_len > (1u << 24) || (uint64_t)cfg->max_calls * cfg->max_len > (1ull << 30))) {
    e = "nof_channels / max_calls 1-65535, max_len 1-2^24, max_calls max_len <= 2^30";
  }
  if (e) {
    hip_log("[srslte_hip] channel: %s\n", e);
    return SRSLTE_ERROR_INVALID_INPUTS;
  }
  auto* q  = new srslte_hip_channel();
  q->cfg   = *cfg;
  q->model = cfg->fading_enable ? cfg->fading_model : SRSLTE_HIP_CHANNEL_FADING_NONE;
  q->N     = cfg->fading_enable ? fading_fft_size(q->model, cfg->srate_hz) : 0;
  q->ntaps = cfg->fading_enable ? ch_nof_taps[q->model] : 0;
  q->dcap  = cfg->delay_enable ? (int)ceil((double)cfg->delay_max_us * cfg->srate_hz / 1e6) + 1 : 0;
  q->coef.assign((size_t)cfg->nof_channels * 3 * MAXTAPS, 0.0);
  if (q->N > 1024) {
    hip_log("[srslte_hip] channel: filter size %d for this model and rate (64-1024 are covered)\n", q->N);
    delete q;
    return SRSLTE_ERROR_INVALID_INPUTS;
  }
  if (channel_init(q)) {
    delete q;
    return SRSLTE_ERROR;
  }
  *out = q;
  return SRSLTE_SUCCESS;
}

int srslte_hip_channel_fft_size(const srslte_hip_channel_t* q) { return q ? q->N : SRSLTE_ERROR_INVALID_INPUTS; }
int srslte_hip_channel_path_delay(const srslte_hip_channel_t* q) { return q ? q->N / 4 : SRSLTE_ERROR_INVALID_INPUTS; }

int srslte_hip_channel_coeffs(const srslte_hip_channel_t* q, uint32_t channel, double a[MAXTAPS], double w[MAXTAPS], double p[MAXTAPS])
{
  if (!q || channel >= q->cfg.nof_channels || !a || !w || !p) return SRSLTE_ERROR_INVALID_INPUTS;
  const double* cc = &q->coef[(size_t)channel * 3 * MAXTAPS];
  for (int i = 0; i < MAXTAPS; i++) a[i] = cc[i], w[i] = cc[MAXTAPS + i], p[i] = cc[2 * MAXTAPS + i];
  return q->ntaps;
}

int srslte_hip_channel_run_batch(srslte_hip_channel_t* q, const void* d_in, uint64_t in_ch_stride, uint64_t in_call_stride, void* d_out,
                                 uint64_t out_ch_stride, uint64_t out_call_stride, uint32_t nof_calls, uint32_t len, int64_t t_full_secs,
                                 double t_frac_secs, void* stream)
{
  if (!q || !d_in || !d_out || d_in == d_out || !(t_frac_secs >= 0.0) || t_full_secs < 0) return SRSLTE_ERROR_INVALID_INPUTS;
  const srslte_hip_channel_cfg_t& c = q->cfg;
  if (nof_calls > c.max_calls || len > c.max_len) {
    hip_log("[srslte_hip] channel: nof_calls %u / len %u beyond the object's max_calls %u / max_len %u\n", nof_calls, len, c.max_calls, c.max_len);
    return SRSLTE_ERROR_INVALID_INPUTS;
  }
  if (nof_calls == 0 || len == 0) return SRSLTE_SUCCESS;
  if (in_call_stride < len || out_call_stride < len) {
    hip_log("[srslte_hip] channel: a call stride shorter than len\n");
    return SRSLTE_ERROR_INVALID_INPUTS;
  }
  hipStream_t st = (hipStream_t)stream;
  // the per-block figures, all checked before anything is queued or any state moves
  std::vector<ChBlock> blocks(nof_calls);
  uint32_t             avail = q->avail;
  for (uint32_t i = 0; i < nof_calls; i++) {
    srslte_hip_channel_block_t b;
    block_params(&c, len, i, t_full_secs, t_frac_secs, &b);
    if (b.delay_samples > len || (int)b.delay_samples > q->dcap) {
      hip_log("[srslte_hip] channel: block %u of %u samples is shorter than its delay of %u samples\n", i, len, b.delay_samples);
      return SRSLTE_ERROR_INVALID_INPUTS;
    }
    blocks[i].t     = b.t;
    blocks[i].delay = (int)b.delay_samples;
    blocks[i].avail = (int)avail;
    blocks[i].cfo   = -b.hst_fs_hz / (uint32_t)c.srate_hz; // hst.c:78
    blocks[i].gate  = b.rlf_on ? 1.0f : 0.0f;
    avail           = b.delay_samples;
  }
  uint8_t* h;
  if (q->ring.acquire(&h)) return SRSLTE_ERROR;
  memcpy(h, blocks.data(), sizeof(ChBlock) * nof_calls);
  ChBlock* d_blk = q->d_blk.get() + (size_t)q->ring.cur * c.max_calls;
  HIP_TRY(hipMemcpyAsync(d_blk, h, sizeof(ChBlock) * nof_calls, hipMemcpyHostToDevice, st));
  if (q->ring.release(st)) return SRSLTE_ERROR;

  ChGeom g;
  g.N = q->N, g.Nq = q->N / 4, g.ntaps = q->ntaps, g.nseg = q->N ? (int)((len + g.Nq - 1) / g.Nq) : 0;
  g.nb = (int)nof_calls, g.len = (int)len;
  g.fading = c.fading_enable != 0, g.delay = c.delay_enable != 0, g.hst = c.hst_enable != 0, g.rlf = c.rlf_enable != 0, g.awgn = c.awgn_enable != 0;
  g.dcap    = q->dcap;
  g.dt      = q->N ? (float)(uint32_t)g.Nq / (float)c.srate_hz : 0.0f;
  g.sigma   = c.awgn_enable ? sqrtf(c.awgn_n0 / 2.0f) : 0.0f;
  g.seed    = c.awgn_seed;
  g.sample0 = q->samples;
  g.in_cs = in_ch_stride, g.in_bs = in_call_stride, g.out_cs = out_ch_stride, g.out_bs = out_call_stride;
  const cf32* in = (const cf32*)d_in;
  if (g.fading) {
    const dim3 grid(g.nseg, nof_calls, c.nof_channels);
#define CH_FADING(NN)                                                                                                                         \
  case NN:                                                                                                                                    \
    hipLaunchKernelGGL(ch_fading_kernel<NN>, grid, dim3(ch_threads<NN>()), 0, st, in, q->d_y.get(), g, (const ChBlock*)d_blk,                    \
                       (const double*)q->d_coef.get(), (const float*)q->d_amp.get(), (const cf32*)q->d_E.get(), q->d_tw);                      \
    break;
    switch (q->N) {
      CH_FADING(64)
      CH_FADING(128)
      CH_FADING(256)
      CH_FADING(512)
      CH_FADING(1024)
      default: return SRSLTE_ERROR;
    }
#undef CH_FADING
    LAUNCH_CHECK();
  }
  const int cur = q->cur;
  hipLaunchKernelGGL(ch_output_kernel, dim3((len + CH_OUT_THREADS - 1) / CH_OUT_THREADS, nof_calls, c.nof_channels), dim3(CH_OUT_THREADS), 0, st, in,
                     (cf32*)d_out, (const cf32*)q->d_y.get(), g, (const ChBlock*)d_blk, (const cf32*)q->d_state[cur].get(), (const cf32*)q->d_hist[cur].get());
  LAUNCH_CHECK();
  const int ncarry = (g.fading ? g.N : 0) + g.dcap;
  if (ncarry) {
    hipLaunchKernelGGL(ch_carry_kernel, dim3((ncarry + CH_OUT_THREADS - 1) / CH_OUT_THREADS, c.nof_channels), dim3(CH_OUT_THREADS), 0, st, in,
                       (const cf32*)q->d_y.get(), g, (const cf32*)q->d_state[cur].get(), q->d_state[cur ^ 1].get(), (const cf32*)q->d_hist[cur].get(),
                       q->d_hist[cur ^ 1].get());
    LAUNCH_CHECK();
    q->cur = cur ^ 1;
  }
  q->avail = avail;
  q->samples += (uint64_t)nof_calls * len;
  return SRSLTE_SUCCESS;
}

} // extern "C"
