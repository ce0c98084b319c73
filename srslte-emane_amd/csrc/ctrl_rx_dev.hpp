// Device helpers of the DL control and broadcast receive kernels (pdcch.hip, pbch.hip): the equalisers of precoding.c in the variants the
// reference's AVX / SSE build runs, srslte_rm_conv_rx's permutations and null value, the CRC-16 and a packed scrambling bit.
#pragma once
#include "common.hpp"

namespace {

constexpr float RX_NULL = 10000.0f; // SRSLTE_RX_NULL (rm_conv.c)

__constant__ uint8_t RM_PERM[32]     = {1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31, 0, 16, 8, 24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30};
__constant__ uint8_t RM_PERM_INV[32] = {16, 0, 24, 8, 20, 4, 28, 12, 18, 2, 26, 10, 22, 6, 30, 14, 17, 1, 25, 9, 21, 5, 29, 13, 19, 3, 27, 11, 23, 7, 31, 15};

// srslte_predecoding_single_gen (precoding.c:238-249): all antennas, x = r / ((hh + noise) scaling), scaling 1
__device__ __forceinline__ cf32 eq_single_gen(const cf32* y, const cf32* h, int nof_rx, int glen, uint32_t k, float noise)
{
  float re = 0.f, im = 0.f, hh = 0.f;
  for (int a = 0; a < nof_rx; a++) {
    const cf32 yy = y[(size_t)a * glen + k], hv = h[(size_t)a * glen + k];
    re += yy.x * hv.x + yy.y * hv.y;
    im += yy.y * hv.x - yy.x * hv.y;
    hh += hv.x * hv.x + hv.y * hv.y;
  }
  const float den = hh + noise;
  return make_float2(re / den, im / den);
}

// srslte_predecoding_single_avx's body (precoding.c:149-226): antenna 0, plus antenna 1 when there are exactly two; noise added when > 0
__device__ __forceinline__ cf32 eq_single_avx(const cf32* y, const cf32* h, int nof_rx, int glen, uint32_t k, float noise)
{
  const int na = nof_rx == 2 ? 2 : 1;
  float     re = 0.f, im = 0.f, hh = 0.f;
  for (int a = 0; a < na; a++) {
    const cf32 yy = y[(size_t)a * glen + k], hv = h[(size_t)a * glen + k];
    re += yy.x * hv.x + yy.y * hv.y;
    im += yy.y * hv.x - yy.x * hv.y;
    hh += hv.x * hv.x + hv.y * hv.y;
  }
  if (noise > 0.f) hh += noise;
  return make_float2(re / hh * 1.0f, im / hh * 1.0f);
}

// one SFBC pair of srslte_predecoding_diversity_gen_ (gen = 1: precoding.c:351-384, every antenna, the 1e-4 guard, sqrt(2) in double) or of
// srslte_predecoding_diversity2_sse (gen = 0: :433-540, antennas 0 and 1 only when there are exactly two, sqrtf(2) in float)
__device__ __forceinline__ void eq_div2(const cf32* y, const cf32* h0, const cf32* h1, int nof_rx, int glen, uint32_t k0, uint32_t k1, bool gen, cf32* x)
{
  const int na = gen ? nof_rx : (nof_rx == 2 ? 2 : 1);
  float     hh = 0.f, x0r = 0.f, x0i = 0.f, x1r = 0.f, x1i = 0.f;
  for (int a = 0; a < na; a++) {
    const size_t o   = (size_t)a * glen;
    const cf32   h00 = h0[o + k0], h01 = h0[o + k1], h10 = h1[o + k0], h11 = h1[o + k1], r0 = y[o + k0], r1 = y[o + k1];
    hh += h00.x * h00.x + h00.y * h00.y + h11.x * h11.x + h11.y * h11.y;
    if (gen && hh == 0.f) hh = 1e-4f;
    x0r += h00.x * r0.x + h00.y * r0.y + h11.x * r1.x + h11.y * r1.y;
    x0i += h00.x * r0.y - h00.y * r0.x + h11.y * r1.x - h11.x * r1.y;
    x1r += h01.x * r1.x + h01.y * r1.y - (h10.x * r0.x + h10.y * r0.y);
    x1i += h01.x * r1.y - h01.y * r1.x - (h10.y * r0.x - h10.x * r0.y);
  }
  if (gen) {
    x[0] = make_float2((float)((double)(x0r / hh) * 1.4142135623730951), (float)((double)(x0i / hh) * 1.4142135623730951));
    x[1] = make_float2((float)((double)(x1r / hh) * 1.4142135623730951), (float)((double)(x1i / hh) * 1.4142135623730951));
  } else {
    const float s2 = sqrtf(2.0f);
    x[0] = make_float2(x0r / hh * s2, x0i / hh * s2);
    x[1] = make_float2(x1r / hh * s2, x1i / hh * s2);
  }
}

// one group of four of srslte_predecoding_diversity_gen_ for 4 ports (precoding.c:385-420) + srslte_layerdemap_diversity: d[4i + l] = x[l]
__device__ __forceinline__ void eq_div4(const cf32* y, const cf32* const* h, int nof_rx, int glen, const uint32_t* k, cf32* x)
{
  float hh02 = 0.f, hh13 = 0.f, xr[4] = {0.f, 0.f, 0.f, 0.f}, xi[4] = {0.f, 0.f, 0.f, 0.f};
  for (int a = 0; a < nof_rx; a++) {
    const size_t o  = (size_t)a * glen;
    const cf32   g0 = h[0][o + k[0]], g1 = h[1][o + k[2]], g2 = h[2][o + k[0]], g3 = h[3][o + k[2]];
    const cf32   r0 = y[o + k[0]], r1 = y[o + k[1]], r2 = y[o + k[2]], r3 = y[o + k[3]];
    hh02 += g0.x * g0.x + g0.y * g0.y + g2.x * g2.x + g2.y * g2.y;
    hh13 += g1.x * g1.x + g1.y * g1.y + g3.x * g3.x + g3.y * g3.y;
    // x0 = conj(g0) r0 + g2 conj(r1); x1 = -g2 conj(r0) + conj(g0) r1; x2, x3 the same with g1, g3 on r2, r3
    xr[0] += g0.x * r0.x + g0.y * r0.y + g2.x * r1.x + g2.y * r1.y;
    xi[0] += g0.x * r0.y - g0.y * r0.x + g2.y * r1.x - g2.x * r1.y;
    xr[1] += -(g2.x * r0.x + g2.y * r0.y) + g0.x * r1.x + g0.y * r1.y;
    xi[1] += -(g2.y * r0.x - g2.x * r0.y) + g0.x * r1.y - g0.y * r1.x;
    xr[2] += g1.x * r2.x + g1.y * r2.y + g3.x * r3.x + g3.y * r3.y;
    xi[2] += g1.x * r2.y - g1.y * r2.x + g3.y * r3.x - g3.x * r3.y;
    xr[3] += -(g3.x * r2.x + g3.y * r2.y) + g1.x * r3.x + g1.y * r3.y;
    xi[3] += -(g3.y * r2.x - g3.x * r2.y) + g1.x * r3.y - g1.y * r3.x;
  }
#pragma unroll
  for (int l = 0; l < 4; l++) {
    const float hh = l < 2 ? hh02 : hh13;
    x[l]           = make_float2((float)((double)(xr[l] / hh) * 1.4142135623730951), (float)((double)(xi[l] / hh) * 1.4142135623730951));
  }
}

__device__ __forceinline__ int scr_bit(const uint32_t* s, int i) { return (s[i >> 5] >> (i & 31)) & 1; }

// CRC-16 of 36.212 5.1.1 (srslte_crc_checksum with SRSLTE_LTE_CRC16 0x11021 on unpacked bits, crc.c)
__device__ __forceinline__ uint32_t crc16(const uint8_t* bits, int n)
{
  uint32_t r = 0;
  for (int i = 0; i < n + 16; i++) {
    r = (r << 1) | (i < n ? (bits[i] & 1u) : 0u);
    if (r & 0x10000u) r ^= 0x11021u;
  }
  return r & 0xffffu;
}

} // namespace
