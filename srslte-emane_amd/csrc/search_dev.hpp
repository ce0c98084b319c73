// The search helpers shared by the synchronisation modules (sync.hip, nbiot_sync.hip): the rotated load, the workgroup reductions of a peak
// search, the peak's side lobe and the CP correlation. Both modules follow one algorithm of the reference under two names
// (compute_peak_sidelobe, pss.c:412-441, and npss.c:301-343; srslte_cp_synch, cp.c:61-77), so it is written once here.
// T is the workgroup's thread count, a power of two; every thread of the workgroup calls a reduction, with T words of LDS of the caller's, and
// every thread gets the result. The reductions end on a barrier, so the same LDS may go into the next call at once.
// Internal linkage, as in cf32_dev.hpp: meas.hip keeps a NO_INDEX and a reduction of its own.
#pragma once
#include "cf32_dev.hpp"
#include <math.h>

namespace {

constexpr uint32_t NO_INDEX = 0xffffffffu;

// x exp(j 2 pi f idx): the fractional part of f idx in double, so the phase is as exact at the end of a frame as at its start
__device__ __forceinline__ cf32 rot(cf32 x, float f, uint32_t idx)
{
  double p = (double)f * (double)idx;
  p -= rint(p);
  float s, c;
  sincospif(2.f * (float)p, &s, &c);
  return cmul(x, make_float2(c, s));
}
__device__ __forceinline__ cf32 ld_rot(const cf32* x, uint32_t idx, float f) { return f != 0.f ? rot(x[idx], f, idx) : x[idx]; }

// the first maximum over the workgroup (srslte_vec_max_fi: strict >, so the lowest index among equals)
template <int T>
__device__ void block_argmax(float& v, uint32_t& i, float* s_v, uint32_t* s_i)
{
  const int tid = threadIdx.x;
  s_v[tid] = v, s_i[tid] = i;
  __syncthreads();
  for (int o = T / 2; o > 0; o >>= 1) {
    if (tid < o) {
      const float    v2 = s_v[tid + o];
      const uint32_t i2 = s_i[tid + o];
      if (v2 > s_v[tid] || (v2 == s_v[tid] && i2 < s_i[tid])) s_v[tid] = v2, s_i[tid] = i2;
    }
    __syncthreads();
  }
  v = s_v[0], i = s_i[0];
  __syncthreads();
}
template <int T>
__device__ uint32_t block_min_u32(uint32_t v, uint32_t* s_i)
{
  const int tid = threadIdx.x;
  s_i[tid]      = v;
  __syncthreads();
  for (int o = T / 2; o > 0; o >>= 1) {
    if (tid < o && s_i[tid + o] < s_i[tid]) s_i[tid] = s_i[tid + o];
    __syncthreads();
  }
  v = s_i[0];
  __syncthreads();
  return v;
}
// fmaxf, not a > b ? a : b: the two can differ only on a NaN (fmaxf drops it, > keeps the left operand) and on +0 against -0. Every value that
// enters here is a lane's fmaxf, from a start of -INFINITY, over averaged |c|^2 values: that drops a NaN, and sums of squares, their averages
// and the 0 behind the row are never -0. So -INFINITY, +0 and positive numbers are all there is, and on those both forms answer the same bits.
template <int T>
__device__ float block_max_float(float v, float* s_v)
{
  const int tid = threadIdx.x;
  s_v[tid]      = v;
  __syncthreads();
  for (int o = T / 2; o > 0; o >>= 1) {
    if (tid < o) s_v[tid] = fmaxf(s_v[tid], s_v[tid + o]);
    __syncthreads();
  }
  v = s_v[0];
  __syncthreads();
  return v;
}

// The larger of the maxima on the two sides of the peak's lobe. av(j): the averaged value at lag j, 0 behind the row (the reference's buffer
// is zeros there, and conv_len = the row's length + 1 lets the walk and the right maximum read them). The lobe's ends are each a parallel
// find-first over blocks of T lags.
template <int T, typename A>
__device__ __forceinline__ float side_lobe(A av, uint32_t peak, uint32_t conv_len, float* s_v, uint32_t* s_i)
{
  const uint32_t tid = threadIdx.x;
  // pl_ub runs on from peak + 1 while av[pl_ub + 1] <= av[pl_ub] and pl_ub < conv_len
  uint32_t ub = peak + 1;
  for (;;) {
    const uint32_t j     = ub + tid;
    const bool     go    = j < conv_len && av(j + 1) <= av(j);
    const uint32_t first = block_min_u32<T>(go ? NO_INDEX : j, s_i);
    if (first != NO_INDEX) {
      ub = first;
      break;
    }
    ub += T;
  }
  // pl_lb runs down from peak - 1 while av[pl_lb - 1] <= av[pl_lb] and pl_lb > 1; a peak on lags 0 .. 2 has pl_lb = 0
  uint32_t lb = 0;
  if (peak > 2) {
    lb = peak - 1;
    for (;;) {
      const bool     in_range = lb >= tid + 1; // j = lb - tid >= 1
      const uint32_t j        = in_range ? lb - tid : 0u;
      const bool     stop     = in_range && !(j > 1 && av(j - 1) <= av(j));
      // the first stop going down is the largest such j: the minimum of lb - j
      const uint32_t d = block_min_u32<T>(stop ? lb - j : NO_INDEX, s_i);
      if (d != NO_INDEX) {
        lb -= d;
        break;
      }
      lb -= T; // no stop among T lags that all lie above 1
    }
  }
  // the maxima of [pl_ub, conv_len - 1) and of [0, pl_lb); an empty range answers its first index and costs no reduction (dr and lb are the
  // workgroup's: a lobe that fills a short tracking window leaves nothing to its right in every row)
  const uint32_t dr    = conv_len - 1 > ub ? conv_len - 1 - ub : 0u;
  float          right = -INFINITY, left = -INFINITY;
  for (uint32_t j = tid; j < dr; j += T) right = fmaxf(right, av(ub + j));
  for (uint32_t j = tid; j < lb; j += T) left = fmaxf(left, av(j));
  right = dr > 0 ? block_max_float<T>(right, s_v) : av(ub);
  left  = lb > 0 ? block_max_float<T>(left, s_v) : av(0);
  return right > left ? right : left;
}

// srslte_cp_synch's correlation at offset i (cp.c:61-77): nsym symbols of N samples behind a CP of cpn, one more in the first of every seven,
// each symbol's sum divided by nsym as it is added. ld(j): sample j.
template <typename Ld>
__device__ __forceinline__ cf32 cp_synch_at(Ld ld, uint32_t N, uint32_t cpn, uint32_t nsym, uint32_t i)
{
  const float ns  = (float)nsym;
  cf32        acc = make_float2(0.f, 0.f);
  uint32_t    off = i;
  for (uint32_t n = 0; n < nsym; n++) {
    const uint32_t cpl = cpn + (n % 7 ? 0u : 1u);
    cf32           d   = make_float2(0.f, 0.f);
    for (uint32_t k = 0; k < cpl; k++) d = cadd(d, cmulconj(ld(off + k), ld(off + N + k)));
    acc.x += d.x / ns, acc.y += d.y / ns;
    off += N + cpl;
  }
  return acc;
}

} // namespace
