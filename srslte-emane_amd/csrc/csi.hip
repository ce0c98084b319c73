// UE CSI feedback measurement for gfx950 (include/srslte_hip/phy_hip.h, "UE CSI feedback"): what select_ri_pmi / srslte_ue_dl_select_ri
// (ue_dl.c:705-800) compute per TTI from the DL channel estimates - srslte_precoding_pmi_select for one and two layers, srslte_precoding_cn
// (precoding.c:2151-2929, srslte_mat_2x2_cn mat.c:101-121) and srslte_cqi_from_snr (cqi.c:556-569) - for a batch of subframes in ONE
// launch on the caller's stream, on the estimates where the estimator left them.
//
// Sampling follows the reference's AVX build: N = nsym 12 nof_prb estimates per (port, antenna); the PMI selection reads RE 24 k for
// k < 4 floor(N / 96) (the vector loops of precoding.c:2352 / :2721 take groups of four and drop the tail), the condition number reads
// k < ceil(N / 24) (srslte_precoding_2x2_cn_gen has no vector form). Per sample the arithmetic is the _gen text with exact divisions;
// the AVX two-layer variant's _mm256_rcp_ps is not imitated (DESIGN.md section 7 has the measured distance between the two).
//
// One workgroup of 256 lanes per subframe; lane t takes samples t, t + 256, ... (at most 700 at 100 PRB: three rounds), loads the 2x2
// matrix once and uses it for all seven sums (four one-layer SINRs, two two-layer SINRs, the condition number). The loads are 8 bytes
// at a stride of 192 bytes: about 22 KB of the 538 KB of a 100 PRB subframe are touched, the kernel waits on latency, not bandwidth.
// The sums are reduced in a fixed order (in-wave shuffles, then the four waves' partials in wave order), so a result does not change
// from run to run. Lane 0 takes the decisions (csi_decide, shared with the host entry srslte_hip_csi_decide) and writes the 64-byte record.
#include "cf32_dev.hpp"
#include "common.hpp"
#include "phy_hip_internal.hpp"
#include <math.h>
#include <string.h>

namespace {

constexpr int   CSI_BLOCK = 256;
constexpr int   PMI_SEL_PRECISION = 24; // precoding.c:2151

struct CsiGeom {
  int   nof_ports, nof_rx, N; // N = nsym * 12 * nof_prb
  int   n_pmi, n_cn;          // samples of the PMI selection / of the condition number
  float offset;               // snr_to_cqi_offset
};

// crealf(c) of srslte_precoding_pmi_select_1l_gen for codebook entry i (precoding.c:2166-2221)
__device__ __forceinline__ float pmi_1l_term(int i, cf32 h00, cf32 h01, cf32 h10, cf32 h11)
{
  const float SQRT1_2 = 0.70710678118654752440f;
  cf32        a0, a1;
  switch (i) {
    case 0: a0 = cadd(cconj(h00), cconj(h01)), a1 = cadd(cconj(h10), cconj(h11)); break;
    case 1: a0 = csub(cconj(h00), cconj(h01)), a1 = csub(cconj(h10), cconj(h11)); break;
    case 2: a0 = csub(cconj(h00), cmulj(cconj(h01))), a1 = csub(cconj(h10), cmulj(cconj(h11))); break;
    default: a0 = cadd(cconj(h00), cmulj(cconj(h01))), a1 = cadd(cconj(h10), cmulj(cconj(h11))); break;
  }
  a0 = cscale(a0, SQRT1_2), a1 = cscale(a1, SQRT1_2);
  const cf32 b0 = cadd(cmul(a0, h00), cmul(a1, h10));
  const cf32 b1 = cadd(cmul(a0, h01), cmul(a1, h11));
  cf32       c;
  switch (i) {
    case 0: c = cadd(b0, b1); break;
    case 1: c = csub(b0, b1); break;
    case 2: c = cadd(b0, cmulj(b1)); break;
    default: c = csub(b0, cmulj(b1)); break;
  }
  return c.x * SQRT1_2;
}

// gamma0 + gamma1 of srslte_precoding_pmi_select_2l_gen for codebook entry i (precoding.c:2489-2559)
__device__ __forceinline__ float pmi_2l_term(int i, cf32 h00, cf32 h01, cf32 h10, cf32 h11, float noise)
{
  cf32 a00, a01, a10, a11;
  if (i == 0) {
    a00 = cadd(cconj(h00), cconj(h01)), a01 = cadd(cconj(h10), cconj(h11));
    a10 = csub(cconj(h00), cconj(h01)), a11 = csub(cconj(h10), cconj(h11));
  } else {
    a00 = csub(cconj(h00), cmulj(cconj(h01))), a01 = csub(cconj(h10), cmulj(cconj(h11)));
    a10 = cadd(cconj(h00), cmulj(cconj(h01))), a11 = cadd(cconj(h10), cmulj(cconj(h11)));
  }
  const cf32 b00 = cadd(cmul(a00, h00), cmul(a01, h10)), b01 = cadd(cmul(a00, h01), cmul(a01, h11));
  const cf32 b10 = cadd(cmul(a10, h00), cmul(a11, h10)), b11 = cadd(cmul(a10, h01), cmul(a11, h11));
  cf32       c00, c01, c10, c11;
  if (i == 0) {
    c00 = cadd(b00, b01), c01 = csub(b00, b01), c10 = cadd(b10, b11), c11 = csub(b10, b11);
  } else {
    c00 = cadd(b00, cmulj(b01)), c01 = csub(b00, cmulj(b01)), c10 = cadd(b10, cmulj(b11)), c11 = csub(b10, cmulj(b11));
  }
  c00 = cscale(c00, 0.25f), c01 = cscale(c01, 0.25f), c10 = cscale(c10, 0.25f), c11 = cscale(c11, 0.25f);
  c00.x += noise, c11.x += noise;
  const cf32  detC = csub(cmul(c00, c11), cmul(c01, c10));
  const float dd   = detC.x * detC.x + detC.y * detC.y;
  const cf32  inv  = make_float2(detC.x / dd, -detC.y / dd);
  const cf32  den0 = cmul(cscale(c00, noise), inv), den1 = cmul(cscale(c11, noise), inv);
  const float g0   = den0.x / (den0.x * den0.x + den0.y * den0.y) - 1.0f;
  const float g1   = den1.x / (den1.x * den1.x + den1.y * den1.y) - 1.0f;
  return g0 + g1;
}

// srslte_mat_2x2_cn (mat.c:101-121), dB
__device__ __forceinline__ float cn_term(cf32 h00, cf32 h01, cf32 h10, cf32 h11)
{
  const float a00 = h00.x * h00.x + h01.x * h01.x + h00.y * h00.y + h01.y * h01.y;
  const cf32  a01 = cadd(cmul(h00, cconj(h10)), cmul(h01, cconj(h11)));
  const float a11 = h10.x * h10.x + h11.x * h11.x + h10.y * h10.y + h11.y * h11.y;
  const float b = a00 + a11, c = a00 * a11 - (a01.x * a01.x + a01.y * a01.y);
  const float sqr = sqrtf(b * b - 4.0f * c);
  return 10 * log10f((b + sqr) / (b - sqr));
}

// srslte_cqi_from_snr (cqi.c:556-569)
__host__ __device__ __forceinline__ uint32_t cqi_from_snr(float snr)
{
  const float t[15] = {1.95f, 4.f, 6.f, 8.f, 10.f, 11.95f, 14.05f, 16.f, 17.9f, 20.9f, 22.5f, 24.75f, 25.5f, 27.30f, 29.f};
  uint32_t    cqi = 0;
#pragma unroll
  for (int i = 0; i < 15; i++) cqi = snr >= t[i] ? (uint32_t)i + 1 : cqi; // the thresholds ascend: the last one met is the first the reference meets
  return cqi;
}

// From the seven sums to the record: the tails of srslte_precoding_pmi_select_1l / _2l (division, strict maximum from 0 with pmi 0 kept when
// nothing exceeds it: srslte_pdsch_select_pmi starts from pmi = 0), srslte_precoding_2x2_cn_gen's mean, srslte_ue_dl_select_ri and
// select_ri_pmi (ue_dl.c:735-800). nof_rx == 1: one layer only, no condition number (srslte_precoding_cn refuses all but 2x2).
__host__ __device__ __forceinline__ void csi_decide(const float s[7], uint32_t n_pmi, uint32_t n_cn, float noise, float snr_db, float offset, int nof_rx,
                                                    srslte_hip_csi_res_t* o)
{
  // sel1 / sel2: sinr_list[pmi] of the selected entry, kept in a scalar (an index into the record would move it out of registers)
  float    max_sinr = 0.0f, sel1 = 0.0f, sel2 = 0.0f;
  uint32_t pmi1 = 0, pmi2 = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const float v = s[i] / (noise * (float)n_pmi);
    o->sinr_1l[i] = v;
    if (i == 0) sel1 = v;
    if (v > max_sinr) max_sinr = v, sel1 = v, pmi1 = (uint32_t)i;
  }
  max_sinr = 0.0f;
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const float v = nof_rx > 1 ? (n_pmi ? s[4 + i] / (float)n_pmi : s[4 + i]) : 0.0f;
    o->sinr_2l[i] = v;
    if (i == 0) sel2 = v;
    if (v > max_sinr) max_sinr = v, sel2 = v, pmi2 = (uint32_t)i;
  }
  o->pmi_1l = pmi1, o->pmi_2l = pmi2;
  const float cn = nof_rx > 1 ? (n_cn ? s[6] / (float)n_cn : s[6]) : 0.0f;
  o->cn_db  = cn;
  o->ri_cn  = nof_rx > 1 && cn < 17.0f ? 1u : 0u;
  float    best = -INFINITY;
  uint32_t best_pmi = 0, best_ri = 0;
  const int max_ri = nof_rx < 2 ? nof_rx : 2;
  for (int ri = 0; ri < max_ri; ri++) {
    const uint32_t this_pmi = ri ? pmi2 : pmi1;
    const float    this_db  = 10.0f * log10f(ri ? sel2 : sel1);
    if ((double)this_db > (double)best + 0.1 || (double)this_db > 20.0) best = this_db, best_pmi = this_pmi, best_ri = (uint32_t)ri;
  }
  o->ri = best_ri, o->pmi = best_pmi, o->sinr_db = best;
  o->cqi_sinr     = cqi_from_snr(best + offset);
  o->cqi_wideband = cqi_from_snr(snr_db + offset);
  o->reserved     = 0;
}

// grid = nof_sf, 256 lanes. ce [nof_sf][nof_ports][nof_rx][N], res [nof_sf][10] floats (srslte_hip_chest_dl_res_t)
__global__ __launch_bounds__(CSI_BLOCK) void csi_kernel(const cf32* __restrict__ ce, const float* __restrict__ res, CsiGeom g,
                                                        srslte_hip_csi_res_t* __restrict__ out)
{
  __shared__ float part[CSI_BLOCK / 64][8];
  const int        b = blockIdx.x, tid = threadIdx.x;
  const float      noise = res[(size_t)b * 10], snr_db = res[(size_t)b * 10 + 2];
  if (g.nof_ports < 2) { // select_pmi / select_ri_pmi "do nothing" on a single-port cell (ue_dl.c:712-714)
    if (tid < 16) reinterpret_cast<uint32_t*>(out + b)[tid] = 0u;
    return;
  }
  // h[i][j] of the reference is ce[port i][antenna j]; its locals: h00 = h[0][0], h01 = h[1][0], h10 = h[0][1], h11 = h[1][1]
  const int   R   = g.nof_rx;
  const cf32* p00 = ce + ((size_t)b * 2 + 0) * R * g.N;
  const cf32* p01 = ce + ((size_t)b * 2 + 1) * R * g.N;
  const cf32* p10 = p00 + (R > 1 ? g.N : 0);
  const cf32* p11 = p01 + (R > 1 ? g.N : 0);
  float       s[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int k = tid; k < g.n_cn; k += CSI_BLOCK) {
    const int  j   = k * PMI_SEL_PRECISION; // < N: k < ceil(N / 24)
    const cf32 h00 = p00[j], h01 = p01[j];
    const cf32 zero = make_float2(0.f, 0.f);
    const cf32 h10 = R > 1 ? p10[j] : zero, h11 = R > 1 ? p11[j] : zero;
    if (k < g.n_pmi) {
#pragma unroll
      for (int i = 0; i < 4; i++) s[i] += pmi_1l_term(i, h00, h01, h10, h11);
      if (R > 1) {
        s[4] += pmi_2l_term(0, h00, h01, h10, h11, noise);
        s[5] += pmi_2l_term(1, h00, h01, h10, h11, noise);
      }
    }
    if (R > 1) s[6] += cn_term(h00, h01, h10, h11);
  }
  // fixed-order reduction: the wave's 64 lanes by halving, then the four waves in order
#pragma unroll
  for (int q = 0; q < 7; q++) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s[q] += __shfl_down(s[q], d, 64);
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int q = 0; q < 7; q++) part[tid >> 6][q] = s[q];
  }
  __syncthreads();
  if (tid == 0) {
    float t[7];
#pragma unroll
    for (int q = 0; q < 7; q++) {
      t[q] = part[0][q];
#pragma unroll
      for (int w = 1; w < CSI_BLOCK / 64; w++) t[q] += part[w][q];
    }
    srslte_hip_csi_res_t o;
    csi_decide(t, (uint32_t)g.n_pmi, (uint32_t)g.n_cn, noise, snr_db, g.offset, R, &o);
    out[b] = o;
  }
}

} // namespace

struct srslte_hip_csi {
  uint32_t nof_prb, nof_ports, nof_rx, nsym;
  float    offset;
};

extern "C" {

srslte_hip_csi_t* srslte_hip_csi_create(uint32_t nof_prb, uint32_t nof_ports, uint32_t nof_rx, int cp_is_norm)
{
  if (nof_prb < 6 || nof_prb > 110 || nof_ports < 1 || nof_ports > 2 || nof_rx < 1 || nof_rx > 2) {
    hip_log("[srslte_hip] csi: 6-110 PRB, 1 or 2 ports (the 4-port codebooks are not covered), 1 or 2 receive antennas\n");
    return nullptr;
  }
  auto* q      = new srslte_hip_csi();
  q->nof_prb   = nof_prb;
  q->nof_ports = nof_ports;
  q->nof_rx    = nof_rx;
  q->nsym      = cp_is_norm ? 14 : 12;
  q->offset    = 0.0f;
  return q;
}

void srslte_hip_csi_destroy(srslte_hip_csi_t* q) { delete q; }

int srslte_hip_csi_set_snr_to_cqi_offset(srslte_hip_csi_t* q, float offset)
{
  if (!q || !(offset == offset)) return SRSLTE_ERROR_INVALID_INPUTS;
  q->offset = offset;
  return SRSLTE_SUCCESS;
}

int srslte_hip_csi_nof_samples(const srslte_hip_csi_t* q, uint32_t* n_pmi, uint32_t* n_cn)
{
  if (!q) return SRSLTE_ERROR_INVALID_INPUTS;
  const uint32_t N = q->nsym * 12 * q->nof_prb;
  if (n_pmi) *n_pmi = 4 * (N / (4 * PMI_SEL_PRECISION));
  if (n_cn) *n_cn = (N + PMI_SEL_PRECISION - 1) / PMI_SEL_PRECISION;
  return SRSLTE_SUCCESS;
}

int srslte_hip_csi_batch(srslte_hip_csi_t* q, const void* d_ce, const void* d_res, uint32_t nof_sf, srslte_hip_csi_res_t* d_out, void* stream)
{
  if (!q || !d_ce || !d_res || !d_out) return SRSLTE_ERROR_INVALID_INPUTS;
  if (nof_sf == 0) return SRSLTE_SUCCESS;
  CsiGeom  g;
  uint32_t n_pmi, n_cn;
  srslte_hip_csi_nof_samples(q, &n_pmi, &n_cn);
  g.nof_ports = (int)q->nof_ports, g.nof_rx = (int)q->nof_rx, g.N = (int)(q->nsym * 12 * q->nof_prb);
  g.n_pmi = (int)n_pmi, g.n_cn = (int)n_cn, g.offset = q->offset;
  hipLaunchKernelGGL(csi_kernel, dim3(nof_sf), dim3(CSI_BLOCK), 0, (hipStream_t)stream, (const cf32*)d_ce, (const float*)d_res, g, d_out);
  LAUNCH_CHECK();
  return SRSLTE_SUCCESS;
}

// The decisions of one subframe from its seven sums (sums[0..3] one layer, [4..5] two layers, [6] condition number) on the host: the
// very function lane 0 of the kernel runs
int srslte_hip_csi_decide(const float sums[7], uint32_t n_pmi, uint32_t n_cn, float noise_estimate, float snr_db, float snr_to_cqi_offset,
                          uint32_t nof_rx, srslte_hip_csi_res_t* out)
{
  if (!sums || !out || nof_rx < 1 || nof_rx > 2) return SRSLTE_ERROR_INVALID_INPUTS;
  csi_decide(sums, n_pmi, n_cn, noise_estimate, snr_db, snr_to_cqi_offset, (int)nof_rx, out);
  return SRSLTE_SUCCESS;
}

uint32_t srslte_hip_cqi_from_snr(float snr) { return cqi_from_snr(snr); }

} // extern "C"
