// Complex helpers and the wavefront sum shared by the control and auxiliary modules (prach.hip, pucch.hip, srs.hip, channel.hip, csi.hip).
// The library is built with -ffp-contract=off -fno-fast-math: these expressions give the same bits wherever they are inlined.
// Internal linkage, as the copies they replace had: fft.hip and the pipelines keep helpers of their own under some of these names.
#pragma once
#include "common.hpp"

namespace {

__host__ __device__ __forceinline__ cf32 cadd(cf32 a, cf32 b) { return make_float2(a.x + b.x, a.y + b.y); }
__host__ __device__ __forceinline__ cf32 csub(cf32 a, cf32 b) { return make_float2(a.x - b.x, a.y - b.y); }
__host__ __device__ __forceinline__ cf32 cmul(cf32 a, cf32 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__host__ __device__ __forceinline__ cf32 cmulconj(cf32 a, cf32 b) { return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); } // a conj(b)
__host__ __device__ __forceinline__ cf32 cconj(cf32 a) { return make_float2(a.x, -a.y); }
__host__ __device__ __forceinline__ cf32 cmulj(cf32 a) { return make_float2(-a.y, a.x); } // _Complex_I * a
__host__ __device__ __forceinline__ cf32 cscale(cf32 a, float s) { return make_float2(a.x * s, a.y * s); }

__device__ __forceinline__ float wave_sum(float v)
{
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_sum(int v) // exact: the int32 sums of the UCI decisions (uci.c:627-654)
{
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

} // namespace
