// Device-side tail-biting K = 7 rate-1/3 Viterbi decoder shared by the PUSCH CQI decoder (pusch_rx.inc) and the PDCCH blind search
// (pdcch.hip): srslte_viterbi_decode_f of an SRSLTE_VITERBI_37 tail-biting decoder on an AVX2 host (viterbi.c:130-152,:532-560 with
// viterbi37_avx2_16bit.c). One wavefront, one lane per state; all buffers in LDS.
#pragma once
#include "common.hpp"

namespace viterbi_dev {

// srslte_viterbi_decode_f's quantisation (viterbi.c:532-540, srslte_vec_quant_fus vector.c:401-413): gain 1000 / max |.|, offset 32767.5,
// clip to 16 bits. Lanes 0..63 of one wavefront; `in` holds len = 3 F soft bits.
template <typename T>
__device__ __forceinline__ void quant_fus(const T* in, uint16_t* us, int len, int lane)
{
  float mx = -9e9f;
  for (int i = lane; i < len; i += 64) mx = fmaxf(mx, fabsf((float)in[i]));
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  const float gain = 1000.0f / mx;
  for (int i = lane; i < len; i += 64) {
    const long t = (long)fmaf(gain, (float)in[i], 32767.5f);
    us[i]        = (uint16_t)(t < 0 ? 0 : (t > 65535 ? 65535 : t));
  }
}

// srslte_viterbi_decode_s's quantisation on an AVX2 host (viterbi.c:570-572, srslte_vec_quant_sus vector.c:443-453 with gain 1 and offset
// 32767): the sum goes through an int16, so every positive soft bit wraps below zero and is clipped to 0; 0 gives 32767 and a negative one
// 32767 + in. This, not the float form above, is what srslte_uci_decode_cqi_pusch's long report goes through (uci.c:403).
__device__ __forceinline__ void quant_sus(const int16_t* in, uint16_t* us, int len, int lane)
{
  for (int i = lane; i < len; i += 64) {
    const int v = in[i];
    us[i]       = (uint16_t)(v > 0 || v == -32768 ? 0 : 32767 + v);
  }
}

// The decoder on three repetitions of the F-bit frame (viterbi.c:144-150, TB_ITER = 3): predecessors by shuffle, decisions by ballot into
// dec[0 .. 3F), traceback on lane 0 from the LAST state of smallest metric. dec[3F .. 3F + 6) must be zero on entry (the traceback reads
// six words past the decisions, as the reference's does). Lane 0 leaves the decoded bits in bits[F .. 3F); the frame is bits[F .. 2F) (the
// middle repetition, viterbi.c:150). Lanes 0..63 of one wavefront.
__device__ __forceinline__ void decode37_tb(const uint16_t* us, unsigned long long* dec, uint8_t* bits, int F, int lane)
{
  __builtin_amdgcn_s_waitcnt(0xc07f); // lgkmcnt(0): one wavefront from here on, LDS in order
  const int      n = lane, b = n >> 1;
  const uint32_t bt0 = (__builtin_popcount((2 * b) & 0x6D) & 1) ? 65535u : 0u, bt1 = (__builtin_popcount((2 * b) & 0x4F) & 1) ? 65535u : 0u,
                 bt2 = (__builtin_popcount((2 * b) & 0x57) & 1) ? 65535u : 0u;
  uint32_t old = 63;
  for (int t = 0; t < 3 * F; t++) {
    const int      f  = t % F;
    const uint32_t a = bt0 ^ us[3 * f], bb = bt1 ^ us[3 * f + 1], c = bt2 ^ us[3 * f + 2];
    const uint32_t m01 = (a + bb + 1) >> 1, met = ((c + m01 + 1) >> 1) >> 3, mm = 8191u - met;
    const uint32_t oi = (uint32_t)__shfl((int)old, b, 64), oj = (uint32_t)__shfl((int)old, b + 32, 64);
    const uint16_t x  = (uint16_t)(oi + ((n & 1) ? mm : met)), y = (uint16_t)(oj + ((n & 1) ? met : mm)); // (m0, m1) or (m2, m3)
    const bool     d  = (int16_t)(uint16_t)(x - y) > 0;
    old               = d ? y : x;
    const unsigned long long bal = __ballot(d);
    if (lane == 0) dec[t] = bal;
  }
  uint32_t mn = old;
  for (int o = 32; o > 0; o >>= 1) mn = min(mn, (uint32_t)__shfl_xor((int)mn, o, 64));
  const unsigned long long at_min = __ballot(old == mn);
  if (lane == 0) {
    uint32_t endstate = (uint32_t)(63 - __builtin_clzll(at_min)) << 2; // the LAST state with the smallest metric
    for (int i = 3 * F - 1; i >= F; i--) {
      const uint32_t k = (uint32_t)(dec[6 + i] >> (endstate >> 2)) & 1u;
      endstate         = (endstate >> 1) | (k << 7);
      bits[i]          = (uint8_t)k;
    }
  }
}

} // namespace viterbi_dev
