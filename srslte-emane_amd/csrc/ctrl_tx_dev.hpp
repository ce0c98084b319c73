// Device helpers of the DL control and broadcast transmit kernels (pdcch_tx.hip, pbch.hip): srslte_rm_conv_tx's column permutation, the
// QPSK level, and srslte_layermap_diversity + srslte_precoding_diversity of one group of symbols.
#pragma once
#include "common.hpp"

namespace {

__constant__ uint8_t RM_PERM_TX[32] = {1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31, 0, 16, 8, 24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30};

// srslte_mod_modulate's QPSK (lte_tables.c:46-58) / BPSK (:32-41) level, QPSK_LEVEL = BPSK_LEVEL = 1/sqrt(2) as float
constexpr float LVL = 0.70710677f;

__device__ __forceinline__ cf32 qpsk(uint32_t b0, uint32_t b1) { return make_float2(b0 ? -LVL : LVL, b1 ? -LVL : LVL); }

// one Alamouti pair of srslte_precoding_diversity: position 0 gives xa, -conj(xb), position 1 xb, conj(xa), on the pair's two ports, times s
__device__ __forceinline__ void sfbc(cf32 xa, cf32 xb, int odd, float s, cf32& first, cf32& second)
{
  if (!odd) {
    first  = make_float2(xa.x * s, xa.y * s);
    second = make_float2(-xb.x * s, xb.y * s);
  } else {
    first  = make_float2(xb.x * s, xb.y * s);
    second = make_float2(xa.x * s, -xa.y * s);
  }
}

// srslte_layermap_diversity + srslte_precoding_diversity (layermap.c:36-44, precoding.c:1848-1893) at position k of a group of P symbols whose
// layer symbols are x[0 .. P): y[p] for every port. 2 ports: one pair; 4 ports: layers 0, 1 on ports 0 / 2 at positions 0, 1, layers 2, 3 on
// ports 1 / 3 at positions 2, 3, zero on the other two ports. 1 port: the symbol itself, no scaling.
__device__ __forceinline__ void precode(int P, int k, const cf32* x, float s, cf32* y)
{
  y[0] = y[1] = y[2] = y[3] = make_float2(0.f, 0.f);
  if (P == 1) {
    y[0] = x[0];
  } else if (P == 2) {
    sfbc(x[0], x[1], k & 1, s, y[0], y[1]);
  } else if (k < 2) {
    sfbc(x[0], x[1], k & 1, s, y[0], y[2]);
  } else {
    sfbc(x[2], x[3], k & 1, s, y[1], y[3]);
  }
}

} // namespace
