// Fragment of pdsch.hip (same translation unit): the PDSCH receive kernels - fused demappers (single port, transmit diversity, two-layer
// modes), rate de-matching, transport-block assembly, RE lists and Gold sequences of the grants modes - and the descriptor structs they share.
#include <vector>

namespace {

struct ChestResDev {
  float noise_estimate, noise_estimate_dbm, snr_db, rsrp, rsrp_dbm, rsrq, rsrq_db, rssi_dbm, cfo, sync_error;
};

struct SfClass { // RE list per subframe class: 0 = sf 0 (PSS/SSS+PBCH), 1 = sf 5 (PSS/SSS), 2 = the rest
  const uint32_t* idx;
  int             nof_re;
};

// Per-subframe / per-code-block descriptors of srslte_hip_dl_rx_batch_grants: every subframe of a batch carries its own grant
// (srslte_pdsch_grant_t: PRB masks of both slots, modulation, transport block size, redundancy version; RNTI, CFI). Null descriptor
// pointers in the geometry structs = the one fixed full-band configuration of srslte_hip_dl_rx_batch.
struct SfDesc {
  const uint32_t* idx; // RE list of the subframe (pdsch_relist_kernel)
  const uint32_t* scr; // packed scrambling bits of the subframe (scr_gen_kernel)
  int             nof_re, mod, Qm;
  int             C, K, tbs, rlen; // segmentation of its transport block (36.212 5.1.2): C blocks of K bits, rlen payload bits per block
  const uint32_t* crc_fac;         // [256] x^(8 cB (255 - t)) mod g_CRC24A, cB = ceil((tbs / 8 + 3) / 256): tb_crc_bytes_kernel's chunk weights
  int             scheme, codebook, nof_tb; // srslte_tx_scheme_t of the subframe's grant (0 / 1: the cell's single-port or diversity mode; 2, 3: two-layer
                                            // modes), pre-decoder codebook index, transport blocks; codeword 1 has its own entry max_batch further on
};
struct CbDesc {
  int             sf, cb;  // subframe of the batch, code block of its transport block
  int             C, K, Qm, nof_re;
  int             combine; // 0: new data, the soft buffer is overwritten; 1: retransmission, added (and skipped if the block's CRC passed)
  int             w_len;   // soft-buffer slots of this block length (multiple of 32) = stride of its slot table
  const uint32_t* tbl;     // slot table of (K, rv)
  int             Nl;      // the block split counts in units of Qm * Nl bits: 2 for transmit diversity, else 1 (sch.c:507-531)
  int             e_off;   // LLRs in front of the shared channel's in this block's row (PUSCH: the CQI report's)
};
struct GrantDev { // what the list / sequence kernels need of a grant
  uint32_t mask[2][4]; // prb_idx[s][n] as bits
  int      sf_idx, lstart, q_off, rnti;
  int      cw;         // codeword of the scrambling sequence (36.211 6.3.1: q << 13 in c_init)
  int      tdd;        // TDD cell: the sync-signal positions of pdsch.c:124-140
  int      nss[2];     // grant.nof_symb_slot: symbols of slot 0 / 1 that carry downlink (ra_dl.c:446-460); 0, 0 = the cyclic prefix's count
};

struct PdschGeom {
  const SfDesc* desc; // grants mode, else null
  SfClass cls[3];
  int     grid_len;   // 14 * 12 * nof_prb
  // channel estimates of one (subframe, antenna): ce_len values; ce_nre = 0: a grid like the received one, indexed alike; ce_nre = 12 nof_prb:
  // ONE row (single-port cells without interpolate_subframe: the estimator gives every symbol the same row), indexed by the sub-carrier
  int      ce_len, ce_nre;
  uint32_t ce_magic;  // ceil(2^32 / ce_nre): k / ce_nre = umulhi(k, ce_magic) for k < 2^16
  int     max_re, max_bits, mod, Qm, mmse, scr_words, tti0, nof_rx, nof_ports;
  float     inv_scaling; // 1 / pdsch_scaling (pdsch.c:852-858): 1, or 1 / rho_a with cfg.power_scale
  float*    csi;     // [nof_sf][max_re] channel gain per RE, or null (cfg.csi_enable)
  uint32_t* csi_max; // [nof_sf] bit pattern of the largest gain of each subframe (non-negative floats order like their bits), zeroed per call
  // two-layer modes (pdsch_demod_mimo_kernel): srslte_tx_scheme_t, codebook index, and the second codeword's modulation and buffers
  int             tx_scheme, codebook_idx, nof_tb, mod1, Qm1, max_bits1, scr_words1;
  const uint32_t* scr1;
  float*          csi1;
  uint32_t*       csi_max1;
  int             cw1_off; // grants mode: codeword 1 of subframe sf is described by desc[cw1_off + sf]
};

// the subframe's largest csi: wavefront maximum, one atomic per wavefront
__device__ __forceinline__ void csi_note_max(uint32_t* dst, float v)
{
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) atomicMax(dst, __float_as_uint(v));
}

__device__ __forceinline__ int sf_class(int sf_idx) { return sf_idx == 0 ? 0 : (sf_idx == 5 ? 1 : 2); }

// grid = (ceil(max_re/256), nof_sf). LLR = int16_t (srslte_demod_soft_demodulate_s + srslte_scrambling_s_offset) or int8_t
// (srslte_demod_soft_demodulate_b + srslte_scrambling_sb_offset, the q->llr_is_8bit branch of pdsch.c:760-779)
template <typename LLR>
__global__ __launch_bounds__(256) void pdsch_demod_kernel(const cf32* __restrict__ grid, const cf32* __restrict__ ce,
                                                          const ChestResDev* __restrict__ res, const uint32_t* __restrict__ scr,
                                                          cf32* __restrict__ d_out, LLR* __restrict__ e_out, PdschGeom g)
{
  __shared__ __attribute__((aligned(16))) LLR stage[256 * 8]; // the workgroup's LLRs, written out with 16-byte stores
  const int       sf = blockIdx.y, sf_idx = (g.tti0 + sf) % 10;
  SfClass         c  = g.cls[sf_class(sf_idx)];
  int             mod = g.mod, Qm = g.Qm;
  const uint32_t* cs = scr + (size_t)sf_idx * g.scr_words; // one spare word behind every sequence
  if (g.desc) {
    const SfDesc d = g.desc[sf];
    if (d.scheme >= 2) return; // a two-layer grant: pdsch_demod_mimo_kernel's
    c.idx = d.idx; c.nof_re = d.nof_re; mod = d.mod; Qm = d.Qm; cs = d.scr;
  }
  const int     base = blockIdx.x * blockDim.x, i = base + threadIdx.x;
  if (base >= c.nof_re) return;
  const bool     live = i < c.nof_re;
  const uint32_t k  = c.idx[live ? i : c.nof_re - 1];
  const float    n0 = g.mmse ? res[sf].noise_estimate : 0.f;
  cf32           x;
  float          gain; // srslte_predecoding_single_csi's side output (precoding.c:251-291)
  const uint32_t kh = g.ce_nre ? k - __umulhi(k, g.ce_magic) * (uint32_t)g.ce_nre : k; // position of this RE's estimate
  if (g.nof_rx == 1) {
    const cf32 y = grid[(size_t)sf * g.grid_len + k], h = ce[(size_t)sf * g.ce_len + kh];
    // precoding.c:277-288 with scaling = 1 (pdsch.c:852-858, power_scale off)
    const float re = y.x * h.x + y.y * h.y, im = y.y * h.x - y.x * h.y, csi = h.x * h.x + h.y * h.y + n0;
    x = make_float2(re * g.inv_scaling / csi, im * g.inv_scaling / csi);
    gain = csi;
  } else { // srslte_predecoding_single_multi (precoding.c:138-262): maximum-ratio combining over the receive antennas
    float re = 0.f, im = 0.f, hh = 0.f;
    for (int a = 0; a < g.nof_rx; a++) {
      const size_t o = ((size_t)sf * g.nof_rx + a) * g.grid_len + k;
      const cf32   y = grid[o], h = ce[((size_t)sf * g.nof_rx + a) * g.ce_len + kh];
      const float  pr = y.x * h.x + y.y * h.y, pi = y.y * h.x - y.x * h.y, ph = h.x * h.x + h.y * h.y;
      re = a ? re + pr : pr;
      im = a ? im + pi : pi;
      hh = a ? hh + ph : ph;
    }
    if (n0 > 0.f) hh += n0;
    x = make_float2(re / hh * g.inv_scaling, im / hh * g.inv_scaling);
    gain = hh;
  }
  if (g.csi) {
    if (live) g.csi[(size_t)sf * g.max_re + i] = gain;
    csi_note_max(g.csi_max + sf, live ? gain : 0.f);
  }
  if (d_out && live) d_out[(size_t)sf * g.max_re + i] = x;
  LLR o[8];
  if constexpr (sizeof(LLR) == 1) {
    demod_dev::demod_b(mod, x, i, c.nof_re, o);
  } else {
    demod_dev::demod_s(mod, x, i, c.nof_re, o);
  }
  const int       bit0 = (live ? i : 0) * Qm;
  const uint32_t  c2   = (uint32_t)((((uint64_t)cs[(bit0 >> 5) + 1] << 32) | cs[bit0 >> 5]) >> (bit0 & 31));
  for (int j = 0; j < Qm; j++) {
    LLR v = o[j];
    if ((c2 >> j) & 1) v = (LLR)-v; // scrambling.c:45-51: sign instruction, -(-min) stays min
    stage[threadIdx.x * Qm + j] = v;
  }
  __syncthreads();
  // max_bits is a multiple of 16 and so is 256 * Qm: the workgroup's output starts on a 16-byte boundary
  const int   nbytes = min(256, c.nof_re - base) * Qm * (int)sizeof(LLR);
  char*       dst    = reinterpret_cast<char*>(e_out + (size_t)sf * g.max_bits + (size_t)base * Qm);
  const char* src    = reinterpret_cast<const char*>(stage);
  for (int o16 = threadIdx.x * 16; o16 + 16 <= nbytes; o16 += 256 * 16) *reinterpret_cast<uint4*>(dst + o16) = *reinterpret_cast<const uint4*>(src + o16);
  const int rem = nbytes & 15;
  if ((int)threadIdx.x < rem) dst[nbytes - rem + threadIdx.x] = src[nbytes - rem + threadIdx.x];
}

// 2-port transmit diversity (TM2): srslte_predecoding_diversity_csi for 2 ports + srslte_layerdemap_diversity (precoding.c:564-598,
// layermap.c:140-148; pdsch.c:890-935 with tx_scheme DIVERSITY) fused with the demapper and descrambler. One thread per PAIR of
// consecutive PDSCH REs (2i, 2i+1) = one SFBC block: x0 = sum_a h00* r0 + h11 r1*, x1 = sum_a -h10 r0* + h01* r1, both divided by
// sum_a |h00|^2 + |h11|^2 and scaled by sqrt(2); d[2i] = x0, d[2i+1] = x1. ce is [sf][port][antenna][grid]. grid = (ceil(max_re/512), nof_sf).
template <typename LLR>
__global__ __launch_bounds__(256) void pdsch_demod_div_kernel(const cf32* __restrict__ grid, const cf32* __restrict__ ce,
                                                              const uint32_t* __restrict__ scr, cf32* __restrict__ d_out, LLR* __restrict__ e_out,
                                                              PdschGeom g)
{
  __shared__ __attribute__((aligned(16))) LLR stage[512 * 8];
  const int       sf = blockIdx.y, sf_idx = (g.tti0 + sf) % 10;
  SfClass         c  = g.cls[sf_class(sf_idx)];
  const uint32_t* cs = scr + (size_t)sf_idx * g.scr_words; // one spare word behind every sequence
  int             mod = g.mod, Qm = g.Qm; // locals: writing to the by-value argument would move it to scratch
  if (g.desc) { // per-subframe grants
    const SfDesc d = g.desc[sf];
    if (d.scheme >= 2) return; // a two-layer grant: pdsch_demod_mimo_kernel's
    c.idx = d.idx; c.nof_re = d.nof_re; mod = d.mod; Qm = d.Qm; cs = d.scr;
  }
  const int     base = blockIdx.x * 512, i0 = base + 2 * threadIdx.x; // nof_re is even for a 2-port cell
  if (base >= c.nof_re) return;
  const bool     live = i0 < c.nof_re;
  const uint32_t k0 = c.idx[live ? i0 : c.nof_re - 2], k1 = c.idx[live ? i0 + 1 : c.nof_re - 1];
  float          hh = 0.f, x0r = 0.f, x0i = 0.f, x1r = 0.f, x1i = 0.f;
  for (int a = 0; a < g.nof_rx; a++) {
    const cf32* y  = grid + ((size_t)sf * g.nof_rx + a) * g.grid_len;
    const cf32* h0 = ce + (((size_t)sf * 2 + 0) * g.nof_rx + a) * g.grid_len;
    const cf32* h1 = ce + (((size_t)sf * 2 + 1) * g.nof_rx + a) * g.grid_len;
    const cf32  r0 = y[k0], r1 = y[k1], h00 = h0[k0], h01 = h0[k1], h10 = h1[k0], h11 = h1[k1];
    hh += h00.x * h00.x + h00.y * h00.y + h11.x * h11.x + h11.y * h11.y;
    if (hh == 0.f) hh = 1e-4f;
    x0r += h00.x * r0.x + h00.y * r0.y + h11.x * r1.x + h11.y * r1.y;
    x0i += h00.x * r0.y - h00.y * r0.x + h11.y * r1.x - h11.x * r1.y;
    x1r += -(h10.x * r0.x + h10.y * r0.y) + h01.x * r1.x + h01.y * r1.y;
    x1i += -(h10.y * r0.x - h10.x * r0.y) + h01.x * r1.y - h01.y * r1.x;
  }
  if (g.csi) { // csi[2i] = csi[2i + 1] = hh (precoding.c:590-591)
    if (live) *reinterpret_cast<float2*>(g.csi + (size_t)sf * g.max_re + i0) = make_float2(hh, hh);
    csi_note_max(g.csi_max + sf, live ? hh : 0.f);
  }
  hh *= 1.0f / g.inv_scaling; // hh *= scaling (precoding.c:593)
  const cf32 x[2] = {make_float2((float)((double)(x0r / hh) * 1.4142135623730951), (float)((double)(x0i / hh) * 1.4142135623730951)),
                     make_float2((float)((double)(x1r / hh) * 1.4142135623730951), (float)((double)(x1i / hh) * 1.4142135623730951))};
#pragma unroll
  for (int t = 0; t < 2; t++) {
    const int i = (live ? i0 : 0) + t;
    if (d_out && live) d_out[(size_t)sf * g.max_re + i] = x[t];
    LLR o[8];
    if constexpr (sizeof(LLR) == 1) {
      demod_dev::demod_b(mod, x[t], i, c.nof_re, o);
    } else {
      demod_dev::demod_s(mod, x[t], i, c.nof_re, o);
    }
    const int      bit0 = i * Qm;
    const uint32_t c2   = (uint32_t)((((uint64_t)cs[(bit0 >> 5) + 1] << 32) | cs[bit0 >> 5]) >> (bit0 & 31));
    for (int j = 0; j < Qm; j++) stage[(2 * threadIdx.x + t) * Qm + j] = ((c2 >> j) & 1) ? (LLR)-o[j] : o[j];
  }
  __syncthreads();
  const int   nbytes = min(512, c.nof_re - base) * Qm * (int)sizeof(LLR);
  char*       dst    = reinterpret_cast<char*>(e_out + (size_t)sf * g.max_bits + (size_t)base * Qm);
  const char* src    = reinterpret_cast<const char*>(stage);
  for (int o16 = threadIdx.x * 16; o16 + 16 <= nbytes; o16 += 256 * 16) *reinterpret_cast<uint4*>(dst + o16) = *reinterpret_cast<const uint4*>(src + o16);
  const int rem = nbytes & 15;
  if ((int)threadIdx.x < rem) dst[nbytes - rem + threadIdx.x] = src[nbytes - rem + threadIdx.x];
}

// 4-port transmit diversity (SFBC + FSTD): srslte_predecoding_diversity_csi for 4 ports + srslte_layerdemap_diversity (precoding.c:599-650,
// layermap.c:140-148). One thread per group of four consecutive PDSCH REs: sub-carriers 4i, 4i+1 carry the Alamouti pair of ports 0/2,
// 4i+2, 4i+3 that of ports 1/3; every symbol has its own divisor. grid = (ceil(max_re/1024), nof_sf).
template <typename LLR>
__global__ __launch_bounds__(256) void pdsch_demod_div4_kernel(const cf32* __restrict__ grid, const cf32* __restrict__ ce,
                                                               const uint32_t* __restrict__ scr, cf32* __restrict__ d_out, LLR* __restrict__ e_out,
                                                               PdschGeom g)
{
  __shared__ __attribute__((aligned(16))) LLR stage[1024 * 8];
  const int       sf = blockIdx.y, sf_idx = (g.tti0 + sf) % 10;
  SfClass         c  = g.cls[sf_class(sf_idx)];
  const uint32_t* cs = scr + (size_t)sf_idx * g.scr_words;
  int             mod = g.mod, Qm = g.Qm; // locals: writing to the by-value argument would move it to scratch
  if (g.desc) { // per-subframe grants
    const SfDesc d = g.desc[sf];
    if (d.scheme >= 2) return;
    c.idx = d.idx; c.nof_re = d.nof_re; mod = d.mod; Qm = d.Qm; cs = d.scr;
  }
  const int     base = blockIdx.x * 1024, i0 = base + 4 * threadIdx.x; // nof_re is a multiple of 4 for a 4-port cell
  if (base >= c.nof_re) return;
  const bool live = i0 < c.nof_re;
  uint32_t   k[4];
#pragma unroll
  for (int t = 0; t < 4; t++) k[t] = c.idx[live ? i0 + t : c.nof_re - 4 + t];
  float a[4] = {0.f, 0.f, 0.f, 0.f}, xr[4] = {0.f, 0.f, 0.f, 0.f}, xi[4] = {0.f, 0.f, 0.f, 0.f};
  for (int an = 0; an < g.nof_rx; an++) {
    const cf32* y = grid + ((size_t)sf * g.nof_rx + an) * g.grid_len;
#pragma unroll
    for (int half = 0; half < 2; half++) {
      const cf32* hA = ce + (((size_t)sf * 4 + half) * g.nof_rx + an) * g.grid_len;     // port 0 / 1
      const cf32* hB = ce + (((size_t)sf * 4 + 2 + half) * g.nof_rx + an) * g.grid_len; // port 2 / 3
      const uint32_t k0 = k[2 * half], k1 = k[2 * half + 1];
      const cf32     h00 = hA[k0], h01 = hB[k0], h10 = hA[k1], h11 = hB[k1], r0 = y[k0], r1 = y[k1];
      a[2 * half] += h00.x * h00.x + h00.y * h00.y + h11.x * h11.x + h11.y * h11.y;
      a[2 * half + 1] += h10.x * h10.x + h10.y * h10.y + h01.x * h01.x + h01.y * h01.y;
      xr[2 * half] += h00.x * r0.x + h00.y * r0.y + h11.x * r1.x + h11.y * r1.y;
      xi[2 * half] += h00.x * r0.y - h00.y * r0.x + h11.y * r1.x - h11.x * r1.y;
      xr[2 * half + 1] += -(h01.x * r0.x + h01.y * r0.y) + h10.x * r1.x + h10.y * r1.y;
      xi[2 * half + 1] += -(h01.y * r0.x - h01.x * r0.y) + h10.x * r1.y - h10.y * r1.x;
    }
  }
  float           gmax = 0.f;
#pragma unroll
  for (int t = 0; t < 4; t++) {
    const int   i  = (live ? i0 : 0) + t;
    const float at = a[t] * (1.0f / g.inv_scaling); // a *= scaling (precoding.c:634-637)
    const cf32  x  = make_float2(xr[t] / at * 1.41421356f, xi[t] / at * 1.41421356f);
    if (g.csi && live) g.csi[(size_t)sf * g.max_re + i] = at / g.nof_rx; // precoding.c:639-642
    gmax = fmaxf(gmax, live ? at / g.nof_rx : 0.f);
    if (d_out && live) d_out[(size_t)sf * g.max_re + i] = x;
    LLR o[8];
    if constexpr (sizeof(LLR) == 1) {
      demod_dev::demod_b(mod, x, i, c.nof_re, o);
    } else {
      demod_dev::demod_s(mod, x, i, c.nof_re, o);
    }
    const int      bit0 = i * Qm;
    const uint32_t c2   = (uint32_t)((((uint64_t)cs[(bit0 >> 5) + 1] << 32) | cs[bit0 >> 5]) >> (bit0 & 31));
    for (int j = 0; j < Qm; j++) stage[(4 * threadIdx.x + t) * Qm + j] = ((c2 >> j) & 1) ? (LLR)-o[j] : o[j];
  }
  if (g.csi) csi_note_max(g.csi_max + sf, gmax);
  __syncthreads();
  const int   nbytes = min(1024, c.nof_re - base) * Qm * (int)sizeof(LLR);
  char*       dst    = reinterpret_cast<char*>(e_out + (size_t)sf * g.max_bits + (size_t)base * Qm);
  const char* src    = reinterpret_cast<const char*>(stage);
  for (int o16 = threadIdx.x * 16; o16 + 16 <= nbytes; o16 += 256 * 16) *reinterpret_cast<uint4*>(dst + o16) = *reinterpret_cast<const uint4*>(src + o16);
  const int rem = nbytes & 15;
  if ((int)threadIdx.x < rem) dst[nbytes - rem + threadIdx.x] = src[nbytes - rem + threadIdx.x];
}

// Two-layer modes on a 2-port cell with 2 receive antennas (SURVEY §8f N4): large-delay CDD (TM3; srslte_predecoding_ccd_2x2_mmse_csi,
// precoding.c:918-1014) and closed-loop multiplexing (TM4; srslte_predecoding_multiplex_2x2_mmse_csi :1326-1438, one layer:
// srslte_predecoding_multiplex_2x1_mrc_csi :1624-1707), each with srslte_mat_2x2_mmse_csi_gen's algebra (mat.c) in exact divisions, fused with
// the demapper and descrambler of BOTH codewords (nof_layers == nof_tb in every case ra_dl.c:556-600 lets through: layer l is codeword l,
// no layer de-mapping; srslte_pdsch_codeword_decode pdsch.c:729-790 with the codeword's own modulation and scrambling sequence).
// One thread per PDSCH RE; ce is [sf][port][antenna][grid], grid [sf][antenna][grid]. grid = (ceil(max_re/256), nof_sf).
// cmul, cadd, csub, cmulj: cf32_dev.hpp
__device__ __forceinline__ cf32 cmulc(cf32 a, cf32 b) { return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); } // a conj(b)

template <typename LLR>
__global__ __launch_bounds__(256) void pdsch_demod_mimo_kernel(const cf32* __restrict__ grid, const cf32* __restrict__ ce,
                                                               const ChestResDev* __restrict__ res, const uint32_t* __restrict__ scr,
                                                               cf32* __restrict__ d_out0, cf32* __restrict__ d_out1, LLR* __restrict__ e_out0,
                                                               LLR* __restrict__ e_out1, PdschGeom g)
{
  __shared__ __attribute__((aligned(16))) LLR stage[2][256 * 8];
  const int       sf = blockIdx.y, sf_idx = (g.tti0 + sf) % 10;
  SfClass         c  = g.cls[sf_class(sf_idx)];
  int             tx_scheme = g.tx_scheme, codebook_idx = g.codebook_idx, nof_tb = g.nof_tb, mods[2] = {g.mod, g.mod1}, Qms[2] = {g.Qm, g.Qm1};
  const uint32_t* css[2] = {scr + (size_t)sf_idx * g.scr_words, g.scr1 ? g.scr1 + (size_t)sf_idx * g.scr_words1 : nullptr};
  if (g.desc) { // per-subframe grants: this subframe's own scheme, allocation, modulations and sequences
    const SfDesc d0 = g.desc[sf];
    if (d0.scheme < 2) return; // single antenna port or transmit diversity: the other kernels'
    const SfDesc d1 = g.desc[g.cw1_off + sf];
    c.idx = d0.idx; c.nof_re = d0.nof_re; tx_scheme = d0.scheme; codebook_idx = d0.codebook; nof_tb = d0.nof_tb;
    mods[0] = d0.mod; Qms[0] = d0.Qm; css[0] = d0.scr;
    mods[1] = d1.mod; Qms[1] = d1.Qm; css[1] = d1.scr;
  }
  const int     base = blockIdx.x * blockDim.x, i = base + threadIdx.x;
  if (base >= c.nof_re) return;
  const bool     live = i < c.nof_re;
  const int      ii = live ? i : c.nof_re - 1;
  const uint32_t k  = c.idx[ii];
  const float    n0 = g.mmse ? res[sf].noise_estimate : 0.f;
  const cf32*    yb = grid + (size_t)sf * 2 * g.grid_len;
  const cf32*    hb = ce + (size_t)sf * 4 * g.grid_len;
  const cf32     y0 = yb[k], y1 = yb[g.grid_len + k];
  const cf32     p0a0 = hb[k], p0a1 = hb[(size_t)g.grid_len + k], p1a0 = hb[(size_t)2 * g.grid_len + k], p1a1 = hb[(size_t)3 * g.grid_len + k];
  const float    scaling = 1.0f / g.inv_scaling;
  cf32           x[2];
  float          csi[2];
  if (nof_tb == 1) { // one layer: the codebook column applied to the ports, maximum-ratio combining over the antennas
    cf32 h0, h1;
    switch (codebook_idx) {
      case 0: h0 = cadd(p0a0, p1a0); h1 = cadd(p0a1, p1a1); break;
      case 1: h0 = csub(p0a0, p1a0); h1 = csub(p0a1, p1a1); break;
      case 2: h0 = cadd(p0a0, cmulj(p1a0)); h1 = cadd(p0a1, cmulj(p1a1)); break;
      default: h0 = csub(p0a0, cmulj(p1a0)); h1 = csub(p0a1, cmulj(p1a1)); break;
    }
    const float norm = 1.41421356f / scaling;
    const float cs = h0.x * h0.x + h0.y * h0.y + h1.x * h1.x + h1.y * h1.y, hh = norm / cs;
    const cf32  t  = cadd(cmulc(y0, h0), cmulc(y1, h1)); // conj(h0) y0 + conj(h1) y1
    x[0]   = make_float2(t.x * hh, t.y * hh);
    x[1]   = x[0];
    csi[0] = cs / norm * 0.70710678f;
    csi[1] = 0.f;
  } else {
    cf32  h00, h01, h10, h11; // effective channel: h[antenna][layer]
    float norm = 2.0f / scaling;
    if (tx_scheme == 3) { // H W U D(i): the sign of the second port alternates with the symbol index
      if (!(ii & 1)) {
        h00 = cadd(p0a0, p1a0); h10 = cadd(p0a1, p1a1); h01 = csub(p0a0, p1a0); h11 = csub(p0a1, p1a1);
      } else {
        h00 = csub(p0a0, p1a0); h10 = csub(p0a1, p1a1); h01 = cadd(p0a0, p1a0); h11 = cadd(p0a1, p1a1);
      }
    } else if (codebook_idx == 0) {
      h00 = p0a0; h01 = p1a0; h10 = p0a1; h11 = p1a1;
      norm = 1.41421356f / scaling;
    } else if (codebook_idx == 1) {
      h00 = cadd(p0a0, p1a0); h01 = csub(p0a0, p1a0); h10 = cadd(p0a1, p1a1); h11 = csub(p0a1, p1a1);
    } else {
      h00 = cadd(p0a0, cmulj(p1a0)); h01 = csub(p0a0, cmulj(p1a0)); h10 = cadd(p0a1, cmulj(p1a1)); h11 = csub(p0a1, cmulj(p1a1));
    }
    // A = H'H + N0 I; B = norm A^-1; W = B H'; x = W y; csi_l = 1 / Re(B_ll)
    cf32 a00 = cadd(cmulc(h00, h00), cmulc(h10, h10)), a11 = cadd(cmulc(h01, h01), cmulc(h11, h11));
    a00.x += n0;
    a11.x += n0;
    const cf32  a01 = cadd(cmulc(h01, h00), cmulc(h11, h10)), a10 = cadd(cmulc(h00, h01), cmulc(h10, h11));
    const cf32  det = csub(cmul(a00, a11), cmul(a01, a10));
    const float dm  = det.x * det.x + det.y * det.y;
    const cf32  nr  = make_float2(norm * (det.x / dm), norm * (-det.y / dm));
    const cf32  b00 = cmul(a11, nr), b01 = cmul(make_float2(-a01.x, -a01.y), nr), b10 = cmul(make_float2(-a10.x, -a10.y), nr), b11 = cmul(a00, nr);
    const cf32  w00 = cadd(cmulc(b00, h00), cmulc(b01, h01)), w01 = cadd(cmulc(b00, h10), cmulc(b01, h11));
    const cf32  w10 = cadd(cmulc(b10, h00), cmulc(b11, h01)), w11 = cadd(cmulc(b10, h10), cmulc(b11, h11));
    x[0]   = cadd(cmul(y0, w00), cmul(y1, w01));
    x[1]   = cadd(cmul(y0, w10), cmul(y1, w11));
    csi[0] = 1.0f / b00.x;
    csi[1] = 1.0f / b11.x;
  }
#pragma unroll
  for (int cw = 0; cw < 2; cw++) {
    if (cw >= nof_tb) break;
    const int       mod = mods[cw], Qm = Qms[cw];
    float*          csi_o = cw ? g.csi1 : g.csi;
    cf32*           d_out = cw ? d_out1 : d_out0;
    if (csi_o) {
      if (live) csi_o[(size_t)sf * g.max_re + i] = csi[cw];
      csi_note_max((cw ? g.csi_max1 : g.csi_max) + sf, live ? csi[cw] : 0.f);
    }
    if (d_out && live) d_out[(size_t)sf * g.max_re + i] = x[cw];
    LLR o[8];
    if constexpr (sizeof(LLR) == 1) {
      demod_dev::demod_b(mod, x[cw], i, c.nof_re, o);
    } else {
      demod_dev::demod_s(mod, x[cw], i, c.nof_re, o);
    }
    const uint32_t* cs   = css[cw];
    const int       bit0 = (live ? i : 0) * Qm;
    const uint32_t  c2   = (uint32_t)((((uint64_t)cs[(bit0 >> 5) + 1] << 32) | cs[bit0 >> 5]) >> (bit0 & 31));
    for (int j = 0; j < Qm; j++) stage[cw][threadIdx.x * Qm + j] = ((c2 >> j) & 1) ? (LLR)-o[j] : o[j];
  }
  __syncthreads();
#pragma unroll
  for (int cw = 0; cw < 2; cw++) {
    if (cw >= nof_tb) break;
    const int   Qm = Qms[cw], nbytes = min(256, c.nof_re - base) * Qm * (int)sizeof(LLR);
    char*       dst = reinterpret_cast<char*>((cw ? e_out1 : e_out0) + (size_t)sf * (cw ? g.max_bits1 : g.max_bits) + (size_t)base * Qm);
    const char* src = reinterpret_cast<const char*>(stage[cw]);
    for (int o16 = threadIdx.x * 16; o16 + 16 <= nbytes; o16 += 256 * 16) *reinterpret_cast<uint4*>(dst + o16) = *reinterpret_cast<const uint4*>(src + o16);
    const int rem = nbytes & 15;
    if ((int)threadIdx.x < rem) dst[nbytes - rem + threadIdx.x] = src[nbytes - rem + threadIdx.x];
  }
}

struct RmGeom {
  const CbDesc* cbd;       // grants mode: one entry per launched block (then C = code-block slots per subframe), else null
  uint8_t*      cb_ok_rst; // grants mode: CRC flags, cleared here for blocks that start new data
  int C, K, Qm, tti0, max_bits, w_stride, out_len; // out_len = 3K+12
  int nof_re[3];
  int             max_re, mod;
  int             Nl;      // the code-block split counts in units of Qm * N_L bits, N_L = 2 for transmit diversity (sch.c:507-531)
  const float*    csi;     // as PdschGeom; null = no CSI weighting
  const uint32_t* csi_max;
  int             combine; // HARQ: add to the soft buffer kept from earlier transmissions (rm_turbo.c:407-409 accumulates) instead of writing it
  const uint8_t*  skip;    // HARQ: [B*C] blocks whose CRC already passed are not touched (sch.c:317-318)
  int             e_off;   // LLRs in front of the shared channel's in every subframe (PUSCH: the CQI report's, sch.c:1058-1064)
  int             w_len;   // slots of the table, where it covers less than the w_stride slots between two blocks (rm_parity_compact); 0: w_stride
};

// wrapping lane-wise add of packed int16 / int8 (the soft buffer accumulates with plain C '+=' on int16_t / int8_t)
template <typename LLR>
__device__ __forceinline__ uint32_t add_wrap(uint32_t a, uint32_t b)
{
  if constexpr (sizeof(LLR) == 2) {
    return (((a & 0xffffu) + (b & 0xffffu)) & 0xffffu) | (((a >> 16) + (b >> 16)) << 16);
  } else {
    const uint32_t lo = ((a & 0x00ff00ffu) + (b & 0x00ff00ffu)) & 0x00ff00ffu, hi = ((a & 0xff00ff00u) >> 8) + ((b & 0xff00ff00u) >> 8);
    return lo | ((hi & 0x00ff00ffu) << 8);
  }
}

// csi_correction (pdsch.c:574-690) applied to LLR number b of a subframe as it is read: 16-bit LLRs: (e * w) >> 16 with w = the gain of
// "its" symbol scaled to 32767 at the subframe's maximum, rounded to nearest even and saturated, for the whole groups of 4 / 4 / 12 / 8
// LLRs the SSE loops cover, (int16)(e * gain / max) for the symbols behind them; in the two-symbol groups (QPSK, 64QAM) the reference's
// _mm_blend_ps takes the low lanes from the SECOND symbol: reproduced. 8-bit LLRs: (int8)(e * (gain / max)). The conversions are
// demod_dev's, with the x86 rule for a NaN: a subframe of zeros has gain = max = 0, its weights are -32768 and its casts 0.
struct CsiW {
  const float* csi; // the subframe's gains
  float        scale, inv;
  int          Qm, mod, body_bits, nsym;
};
__device__ __forceinline__ CsiW csi_setup(const RmGeom& g, int sf, int nsym, int Qm)
{ // Qm: of this block's transport block (grants mode: from its descriptor); srslte_mod_t = Qm / 2
  CsiW c;
  c.csi = g.csi + (size_t)sf * g.max_re;
  const float mx = nsym > 0 ? __uint_as_float(g.csi_max[sf]) : 1.0f;
  c.scale = 32767.0f / mx;
  c.inv   = 1.0f / mx;
  c.Qm = Qm; c.mod = Qm / 2; c.nsym = nsym;
  const int G = c.mod == 3 ? 12 : (c.mod == 4 ? 8 : 4);
  c.body_bits = (nsym * Qm / G) * G;
  return c;
}
template <typename LLR>
__device__ __forceinline__ LLR csi_apply(const CsiW& c, LLR v, int b)
{
  if constexpr (sizeof(LLR) == 1) {
    const int s = min(b / c.Qm, c.nsym - 1);
    return (LLR)demod_dev::trunc_i((float)v * (c.csi[s] * c.inv));
  } else {
    if (b >= c.body_bits) {
      const int s = min(b / c.Qm, c.nsym - 1);
      return (LLR)demod_dev::trunc_i((float)v * (c.csi[s] * c.inv));
    }
    int s;
    if (c.mod == 1) { // QPSK: LLRs 0,1 of a group of 4 take the second symbol's gain
      s = 2 * (b >> 2) + (((b & 3) < 2) ? 1 : 0);
    } else if (c.mod == 3) { // 64QAM: 0-3 first, 4,5 second, 6,7 first, 8-11 second
      const int r = b % 12;
      s = 2 * (b / 12) + ((r < 4 || r == 6 || r == 7) ? 0 : 1);
    } else {
      s = b / c.Qm;
    }
    const int w = demod_dev::sat16(demod_dev::rne(c.csi[s] * c.scale)); // _mm_cvtps_pi16: cvtps2pi + packssdw
    return (LLR)(((int)v * w) >> 16);
  }
}


// grid = (ceil(w_stride/512), nof_sf*C): gather form of w[deint[i]] += e[i] (wrapping int16, rm_turbo.c:407-409).
// inv[j] = circular-buffer position n that lands on soft-buffer slot j (0xffffffff for padding); a thread owns two
// adjacent slots, sums their <= ceil(n_e/out_len) wraps from e and writes one dword: stores are coalesced and every
// slot, padding included, is written exactly once (no memset, no atomics).
// LLR = int8_t (srslte_rm_turbo_rx_lut_8bit, rm_turbo.c:428-465: wrapping int8 sums): a thread owns four adjacent slots.
template <typename LLR>
__global__ __launch_bounds__(256) void rm_rx_kernel(const LLR* __restrict__ e, LLR* __restrict__ w, const uint32_t* __restrict__ inv, RmGeom g)
{
  constexpr int PER = 4 / (int)sizeof(LLR); // slots per dword
  // the block: memory slot cbg = sf * g.C + cb; in grants mode its own (C, K, Qm, nof_re, table) come from the descriptor
  int             cbg = blockIdx.y, sf = cbg / g.C, cb = cbg - sf * g.C, C = g.C, Qm = g.Qm, out_len = g.out_len, w_len = g.w_len ? g.w_len : g.w_stride, combine = g.combine;
  int             nre = g.nof_re[sf_class((g.tti0 + sf) % 10)], Nl = g.Nl, e_off = g.e_off;
  const uint32_t* tbl = inv;
  if (g.cbd) {
    const CbDesc d = g.cbd[blockIdx.y];
    sf = d.sf; cb = d.cb; cbg = sf * g.C + cb; C = d.C; Qm = d.Qm; out_len = 3 * d.K + 12; w_len = d.w_len; combine = d.combine; nre = d.nof_re; tbl = d.tbl;
    Nl = d.Nl; e_off = d.e_off;
  }
  const int j = PER * (blockIdx.x * blockDim.x + threadIdx.x);
  if (j >= w_len || (g.skip && combine && g.skip[cbg])) return;
  if (g.cb_ok_rst && !combine && j == 0) g.cb_ok_rst[cbg] = 0;
  const int QmL = Qm * Nl, Gp = nre / Nl; // Gp = nof_bits / (Qm N_L)
  const int gamma = Gp % C, n_e = QmL * (Gp / C);
  int       rp = cb * n_e, n_e2 = n_e;
  if (cb > C - gamma) { // sch.c:331-334 (the '>' quirk is upstream's)
    n_e2 = n_e + QmL;
    rp   = (C - gamma) * n_e + (cb - (C - gamma)) * n_e2;
  }
  const LLR* src = e + (size_t)sf * g.max_bits + e_off + rp;
  CsiW       cw;
  if (g.csi) cw = csi_setup(g, sf, nre, Qm);
  uint32_t   n[PER], word = 0;
  if constexpr (PER == 2) {
    const uint2 t = *reinterpret_cast<const uint2*>(tbl + j);
    n[0] = t.x; n[1] = t.y;
  } else {
    const uint4 t = *reinterpret_cast<const uint4*>(tbl + j);
    n[0] = t.x; n[1] = t.y; n[2] = t.z; n[3] = t.w;
  }
#pragma unroll
  for (int s = 0; s < PER; s++) {
    int acc = 0;
    if (n[s] != 0xffffffffu) {
      for (int i = (int)n[s]; i < n_e2; i += out_len) acc += g.csi ? csi_apply<LLR>(cw, src[i], rp + i) : src[i];
    }
    word |= ((uint32_t)acc & ((1u << (8 * sizeof(LLR))) - 1u)) << (8 * sizeof(LLR) * s);
  }
  uint32_t* dst = reinterpret_cast<uint32_t*>(w + (size_t)cbg * g.w_stride + j);
  *dst          = combine ? add_wrap<LLR>(*dst, word) : word;
}

// Same result with the code block's LLR segment staged in LDS: one workgroup per code block copies its n_e LLRs with 16-byte
// loads, then every thread produces 16 bytes of adjacent soft-buffer slots per step from LDS gathers. A 2-byte global gather
// costs the L1 one cache line per lane; the LDS gather a few bank-conflict cycles. The slot table is the 16-bit copy behind the
// 32-bit one (inv + w_stride), four steps' worth of it loaded ahead; LDS is sized to the segment (rm_lds_bytes) so that eight
// workgroups share a CU. Used when the segment fits 64 KB.
template <typename LLR>
__global__ __launch_bounds__(256) void rm_rx_lds_kernel(const LLR* __restrict__ e, LLR* __restrict__ w, const uint32_t* __restrict__ inv, RmGeom g)
{
  extern __shared__ __attribute__((aligned(16))) char seg_raw[];
  constexpr int PER = 16 / (int)sizeof(LLR), NV = PER / 8; // slots per 16 bytes; uint4 loads of 16-bit table entries per step
  LLR*          seg = reinterpret_cast<LLR*>(seg_raw);
  int             cbg = blockIdx.x, sf = cbg / g.C, cb = cbg - sf * g.C, C = g.C, Qm = g.Qm, out_len = g.out_len, w_len = g.w_len ? g.w_len : g.w_stride, combine = g.combine;
  int             nre = g.nof_re[sf_class((g.tti0 + sf) % 10)], Nl = g.Nl, e_off = g.e_off;
  const uint32_t* tbl = inv;
  if (g.cbd) {
    const CbDesc d = g.cbd[blockIdx.x];
    sf = d.sf; cb = d.cb; cbg = sf * g.C + cb; C = d.C; Qm = d.Qm; out_len = 3 * d.K + 12; w_len = d.w_len; combine = d.combine; nre = d.nof_re; tbl = d.tbl;
    Nl = d.Nl; e_off = d.e_off;
  }
  if (g.skip && combine && g.skip[cbg]) return;
  if (g.cb_ok_rst && !combine && threadIdx.x == 0) g.cb_ok_rst[cbg] = 0;
  const int QmL = Qm * Nl, Gp = nre / Nl;
  const int gamma = Gp % C, n_e = QmL * (Gp / C);
  int       rp = cb * n_e, n_e2 = n_e;
  if (cb > C - gamma) { // sch.c:331-334
    n_e2 = n_e + QmL;
    rp   = (C - gamma) * n_e + (cb - (C - gamma)) * n_e2;
  }
  const LLR* src = e + (size_t)sf * g.max_bits + e_off + rp;
  // the segment starts at an arbitrary LLR index: copy from the 16-byte boundary below it
  const int mis = (int)((reinterpret_cast<uintptr_t>(src) & 15) / sizeof(LLR));
  const int4* s4 = reinterpret_cast<const int4*>(src - mis);
  const int   n16 = (n_e2 + mis + PER - 1) / PER;
  if (g.csi) { // weigh while staging: element j of 16-byte word i is LLR rp - mis + PER * i + j of the subframe
    const CsiW cw = csi_setup(g, sf, nre, Qm);
    for (int i = threadIdx.x; i < n16; i += 256) {
      union {
        int4 v;
        LLR  h[PER];
      } u;
      u.v = s4[i];
#pragma unroll
      for (int j = 0; j < PER; j++) u.h[j] = csi_apply<LLR>(cw, u.h[j], rp - mis + PER * i + j);
      reinterpret_cast<int4*>(seg)[i] = u.v;
    }
  } else {
#pragma unroll 4
    for (int i = threadIdx.x; i < n16; i += 256) reinterpret_cast<int4*>(seg)[i] = s4[i];
  }
  __syncthreads();
  const LLR*   ls    = seg + mis;
  const uint4* inv16 = reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(tbl + w_len));
  uint4*       dst   = reinterpret_cast<uint4*>(w + (size_t)cbg * g.w_stride);
  const int    ngroups = w_len / PER;
  for (int j0 = threadIdx.x; j0 < ngroups; j0 += 4 * 256) {
    uint4 tt[4][NV];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int j = j0 + 256 * u;
#pragma unroll
      for (int v = 0; v < NV; v++) tt[u][v] = j < ngroups ? inv16[j * NV + v] : make_uint4(~0u, ~0u, ~0u, ~0u);
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int j = j0 + 256 * u;
      if (j >= ngroups) break;
      uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
      for (int s = 0; s < PER; s++) {
        const uint32_t pair = (&tt[u][s / 8].x)[(s / 2) & 3], n = (s & 1) ? pair >> 16 : pair & 0xffffu;
        int            acc  = 0;
        if (n != 0xffffu) {
          for (int i = (int)n; i < n_e2; i += out_len) acc += ls[i];
        }
        constexpr int BITS = 8 * (int)sizeof(LLR);
        o[s * BITS / 32] |= ((uint32_t)acc & ((1u << BITS) - 1u)) << ((s * BITS) & 31);
      }
      if (combine) {
        const uint4 old = dst[j];
        dst[j] = make_uint4(add_wrap<LLR>(old.x, o[0]), add_wrap<LLR>(old.y, o[1]), add_wrap<LLR>(old.z, o[2]), add_wrap<LLR>(old.w, o[3]));
      } else {
        dst[j] = make_uint4(o[0], o[1], o[2], o[3]);
      }
    }
  }
}

__device__ __forceinline__ uint32_t gf24_mul(uint32_t a, uint32_t b, uint32_t poly)
{ // a(x) b(x) mod g(x), deg g = 24 (poly carries the x^24 term)
  uint32_t r = 0;
  for (int i = 23; i >= 0; i--) {
    r <<= 1;
    if (r & 0x1000000u) r ^= poly;
    if ((b >> i) & 1) r ^= a;
  }
  return r;
}

// CRC24 (init 0, MSB first) of nbytes bytes by a 256-thread block: the message is zero-extended at the FRONT to 256 equal chunks
// (leading zeros do not change the remainder), every thread runs the byte-table recursion over its chunk, and the chunk
// remainders are folded pairwise with x^(8*chunk*2^level) mod g. tab/red: 256 words of LDS each. Result valid in every thread.
template <typename Byte>
__device__ uint32_t block_crc24(Byte byte_at, int nbytes, uint32_t poly, uint32_t* tab, uint32_t* red)
{
  const int t = threadIdx.x;
  {
    uint32_t v = (uint32_t)t << 16;
    for (int i = 0; i < 8; i++) {
      v <<= 1;
      if (v & 0x1000000u) v ^= poly;
    }
    tab[t] = v;
  }
  __syncthreads();
  const int cB = (nbytes + 255) / 256, pad = 256 * cB - nbytes;
  uint32_t  crc = 0;
  for (int i = 0; i < cB; i++) {
    const int v = t * cB + i - pad;
    if (v >= 0) crc = ((crc << 8) & 0xffffffu) ^ tab[((crc >> 16) & 0xff) ^ byte_at(v)];
  }
  uint32_t m = 1; // x^(8 cB) mod g
  for (int i = 0; i < 8 * cB; i++) {
    m <<= 1;
    if (m & 0x1000000u) m ^= poly;
  }
  red[t] = crc;
  __syncthreads();
  for (int s = 1; s < 256; s <<= 1) {
    uint32_t v = 0;
    if ((t & (2 * s - 1)) == 0) v = gf24_mul(red[t], m, poly) ^ red[t + s];
    __syncthreads();
    if ((t & (2 * s - 1)) == 0) red[t] = v;
    m = gf24_mul(m, m, poly);
    __syncthreads();
  }
  return red[0];
}

struct TbGeom {
  const SfDesc* desc; // grants mode (tb_crc_bytes_kernel): per-subframe (C, K, tbs, rlen), C = code-block slots per subframe; else null
  int C, K, tbs, rlen, cb_stride, tb_stride;
  int nof_sf, cw1_off; // grants mode: subframes of the call, descriptor offset of their second transport blocks
  // pass counts of the call's code blocks, laid out like cb_ok (0 = skipped: its CRC had passed in an earlier transmission). A transport block
  // of which NO block was decoded in this call is reported as failed, as upstream does: decode_tb_cb keeps the bytes of passed blocks for the
  // next transmission only while the block as a whole has failed (sch.c:399-410), so a retransmission after a success reassembles stale bytes
  // and fails its CRC-24A (sch.c:470-488). The MAC does not schedule one (it discards duplicates), the PHY answers as upstream's would.
  const uint32_t* iters;
};
__device__ __forceinline__ bool tb_any_block_decoded(const uint32_t* iters, int first, int C)
{
  if (!iters) return true;
  bool any = false;
  for (int c = 0; c < C; c++) any = any || iters[first + c] != 0;
  return any;
}

// one workgroup per subframe: assemble the payload (sch.c:360,:401-410) and check CRC24A (sch.c:470-488).
// The CRC is the XOR over set bits of precomputed x^(n-1-j) mod g: branch-free, every lookup independent.
__global__ __launch_bounds__(512) void tb_crc_kernel(const uint8_t* __restrict__ cb_bytes, const uint8_t* __restrict__ cb_ok,
                                                     const uint32_t* __restrict__ crc_rem, uint8_t* __restrict__ tb, uint8_t* __restrict__ tb_ok,
                                                     TbGeom g)
{
  __shared__ uint32_t red[8];
  const int C = g.C, K = g.K, tbs = g.tbs, rlen = g.rlen;
  const int sf = blockIdx.x, nbytes = tbs / 8 + 3, rb = rlen / 8;
  uint8_t*  dst = tb + (size_t)sf * g.tb_stride;
  uint32_t  syn = 0;
  for (int b0 = threadIdx.x * 4; b0 < nbytes + 3; b0 += blockDim.x * 4) {
    uint32_t word = 0;
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const int b = b0 + t;
      int       cb = b / rb;
      if (cb > C - 1) cb = C - 1;
      const int     off = b - cb * rb;
      const uint8_t v   = (b < nbytes + 3 && off < K / 8) ? cb_bytes[((size_t)sf * g.C + cb) * g.cb_stride + off] : 0;
      if (b < nbytes + 3) dst[b] = v;
      word |= (uint32_t)(b < nbytes ? v : 0) << (8 * t);
    }
#pragma unroll
    for (int j = 0; j < 32; j++) { // bit j of byte t = message bit 8*(b0+t) + (7 - j%8)
      const int      t = j >> 3, bit = 8 * (b0 + t) + 7 - (j & 7);
      const uint32_t m = 0u - ((word >> j) & 1u);
      syn ^= (bit < 8 * nbytes ? crc_rem[bit] : 0u) & m;
    }
  }
  for (int o = 32; o > 0; o >>= 1) syn ^= __shfl_xor(syn, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = syn;
  __syncthreads();
  if (threadIdx.x == 0) {
    syn = 0;
    for (int i = 0; i < (int)blockDim.x / 64; i++) syn ^= red[i];
    bool ok = syn == 0;
    for (int c = 0; c < C; c++) ok = ok && cb_ok[sf * g.C + c];
    // par_rx == par_tx && par_rx != 0 (sch.c:481): a zero parity with zero syndrome is rejected upstream
    const uint8_t* p = dst + tbs / 8;
    ok               = ok && (p[0] | p[1] | p[2]) && tb_any_block_decoded(g.iters, sf * g.C, C);
    tb_ok[sf]        = ok ? 1 : 0;
  }
}

// The same for transport blocks of any size (grants mode): the bytes go through LDS, 256 threads take the CRC24A of contiguous chunks with a
// byte table, and the chunk CRCs are combined with 256 weights x^(8 n) mod g that the host makes once per transport block size.
constexpr int TB_MAX_BITS = 105528;
__global__ __launch_bounds__(256) void tb_crc_bytes_kernel(const uint8_t* __restrict__ cb_bytes, const uint8_t* __restrict__ cb_ok, uint8_t* __restrict__ tb,
                                                           uint8_t* __restrict__ tb_ok, TbGeom g)
{
  __shared__ uint32_t tab[256], red[4];
  __shared__ uint8_t  bytes[TB_MAX_BITS / 8 + 8]; // the largest one-layer transport block (36.213 Table 7.1.7.2.1-1: 105528 bits at 110 PRB) + CRC
  // row r < nof_sf: transport block 0 of subframe r (descriptor / HARQ slot r); row nof_sf + b: transport block 1 of subframe b (slot cw1_off + b)
  const int    row = blockIdx.x, sf = row < g.nof_sf ? row : g.cw1_off + row - g.nof_sf;
  const SfDesc d   = g.desc[sf];
  const int    C = d.C, K = d.K, nbytes = d.tbs / 8 + 3, rb = d.rlen / 8, t = threadIdx.x;
  uint8_t*     dst = tb + (size_t)row * g.tb_stride;
  if (C == 0) { // no transport block here
    if (t == 0) tb_ok[row] = 0;
    return;
  }
  {
    uint32_t v = (uint32_t)t << 16; // byte table of CRC24A
    for (int i = 0; i < 8; i++) {
      v <<= 1;
      if (v & 0x1000000u) v ^= 0x1864CFBu;
    }
    tab[t] = v;
  }
  for (int cb = 0; cb < C; cb++) { // block cb carries bytes [cb rb, (cb + 1) rb) of the transport block (the last one also the 3 bytes behind)
    const uint8_t* src = cb_bytes + ((size_t)sf * g.C + cb) * g.cb_stride;
    const int      n   = cb == C - 1 ? nbytes + 3 - cb * rb : rb;
    for (int i = t; i < n; i += 256) {
      const uint8_t v = i < K / 8 ? src[i] : 0;
      dst[cb * rb + i] = v;
      if (cb * rb + i < nbytes) bytes[cb * rb + i] = v;
    }
  }
  __syncthreads();
  // CRC of 256 contiguous chunks of cB bytes (zeros in front do not change a CRC), each weighted by x^(8 cB (chunks behind it)) mod g
  const int cB = (nbytes + 255) / 256, pad = 256 * cB - nbytes;
  uint32_t  crc = 0;
  for (int i = 0; i < cB; i++) {
    const int v = t * cB + i - pad;
    if (v >= 0) crc = ((crc << 8) & 0xffffffu) ^ tab[((crc >> 16) & 0xff) ^ bytes[v]];
  }
  uint32_t syn = gf24_mul(crc, d.crc_fac[t], 0x1864CFBu);
  for (int o = 32; o > 0; o >>= 1) syn ^= __shfl_xor(syn, o, 64);
  if ((t & 63) == 0) red[t >> 6] = syn;
  __syncthreads();
  if (t == 0) {
    bool ok = (red[0] ^ red[1] ^ red[2] ^ red[3]) == 0;
    for (int c = 0; c < C; c++) ok = ok && cb_ok[sf * g.C + c];
    ok        = ok && (bytes[nbytes - 3] | bytes[nbytes - 2] | bytes[nbytes - 1]); // par_rx != 0 (sch.c:481)
    ok        = ok && tb_any_block_decoded(g.iters, sf * g.C, C);
    tb_ok[row] = ok ? 1 : 0;
  }
}

// ---- grants mode: RE lists and scrambling sequences made on the device from the grants of the batch
// pdsch.c:81-206 as a per-RE rule for a single-port cell (see pdsch_re_indices below and oracle/orc_pdsch.c): symbol sym = 7 s + l,
// sub-carrier k. q_off: what upstream's `offset` variable holds when it reaches the half PRBs of an odd-bandwidth cell (pdsch.c:172-190)
// nsl: symbols per slot, 7 or 6 (extended CP): CRS symbols 0 and nsl - 3, PSS / SSS on the last two symbols of slot 0
// tdd / nss0 / nss1: TDD cell and the grant's nof_symb_slot (SSS on the last downlink symbol of slot 1 in subframes 0 / 5, PSS on symbol 2 of
// subframes 1 / 6, pdsch.c:124-140); the caller keeps l below the slot's downlink symbols
__host__ __device__ __forceinline__ bool pdsch_re_used(int P, int cell_id, int sf_idx, int q_off, int s, int l, int k, int nof_ports = 1, int nsl = 7, int tdd = 0,
                                                       int nss1 = 0)
{
  const int  nre  = 12 * P;
  const bool ss   = tdd ? ((s == 1 && (sf_idx == 0 || sf_idx == 5) && l >= (nss1 ? nss1 : nsl) - 1) || (s == 0 && (sf_idx == 1 || sf_idx == 6) && l == 2))
                        : (s == 0 && (sf_idx == 0 || sf_idx == 5) && l >= nsl - 2);
  const bool sync = ss || (s == 1 && sf_idx == 0 && l < 4);
  if (sync && k + 36 >= nre / 2 && k < nre / 2 + 36) return false;
  if (l == 0 || l == nsl - 3 || (l == 1 && nof_ports == 4)) { // phy_common.h:139-141
    const int  p      = k / 12;
    const bool centre = p >= P / 2 - 3 && p < P / 2 + 3 + (P % 2);
    // q_off: upstream's stale `offset` at the half PRBs of a sync symbol that also carries CRS - bits 0-7 for symbol 0 of slot 1, bits 8-15 for
    // symbol 1 (4 ports), bits 16-23 for symbol 3 of an extended-CP cell (its PBCH region spans two CRS symbols)
    const int qv = l == 0 ? (q_off & 255) : (l == 1 ? ((q_off >> 8) & 255) : ((q_off >> 16) & 255));
    if (nof_ports == 1) {
      const int off = (centre && sync) ? qv : (l == 0 ? cell_id % 6 : (cell_id + 3) % 6);
      if (k % 6 == off % 6) return false;
    } else { // every port's CRS positions stay empty: one RE in three, the same offset in every CRS symbol (pdsch.c:103-107)
      const int off = (centre && sync) ? qv : cell_id % 3;
      if (k % 3 == off % 3) return false;
    }
  }
  return true;
}

// One workgroup per subframe: idx_out[sf][...] = the grid positions of the subframe's PDSCH REs in the reference's order (symbol-major,
// sub-carrier ascending). Two sweeps over the 14 x 12 P grid positions in chunks of 64: per-chunk counts by ballot, a prefix sum, then
// every wavefront writes its chunks' positions compacted (coalesced).
constexpr int RELIST_THREADS = 512;
__device__ __forceinline__ void pdsch_relist_body(const GrantDev* __restrict__ gr, uint32_t* __restrict__ idx_out, int P, int cell_id, int max_re,
                                                  int nof_ports, int nsl, int sf);
__global__ __launch_bounds__(RELIST_THREADS) void pdsch_relist_kernel(const GrantDev* __restrict__ gr, uint32_t* __restrict__ idx_out, int P, int cell_id,
                                                                      int max_re, int nof_ports, int nsl)
{
  pdsch_relist_body(gr, idx_out, P, cell_id, max_re, nof_ports, nsl, (int)blockIdx.x);
}
__device__ __forceinline__ void pdsch_relist_body(const GrantDev* __restrict__ gr, uint32_t* __restrict__ idx_out, int P, int cell_id, int max_re,
                                                  int nof_ports, int nsl, int sf)
{
  __shared__ int cnt[14 * 21 + 1]; // chunks: 14 symbols x ceil(12 * 110 / 64)
  const int      nre = 12 * P, cps = (nre + 63) / 64, nsym = 2 * nsl, nchunks = nsym * cps;
  const int      wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nwaves = RELIST_THREADS / 64;
  const GrantDev g  = gr[sf];
  auto           used = [&](int sym, int kc) { // position (sym, kc * 64 + lane)
    const int k = kc * 64 + lane, s = sym >= nsl ? 1 : 0, l = sym - nsl * s, p = k / 12;
    if (k >= nre || !((g.mask[s][p >> 5] >> (p & 31)) & 1u)) return false;
    if (g.nss[0] && l >= g.nss[s]) return false; // behind the DwPTS of a TDD special subframe (slot 1 only exists when slot 0 is whole: sym = l + s nss[0])
    return pdsch_re_used(P, cell_id, g.sf_idx, g.q_off, s, l, k, nof_ports, nsl, g.tdd, g.nss[1]);
  };
  __shared__ unsigned long long msk[14 * 21]; // the chunks' masks: the second sweep does not evaluate the rule again
  for (int sym = 0; sym < nsym; sym++) {
    const bool on = sym >= nsl || sym >= g.lstart; // control region
    for (int kc = wave; kc < cps; kc += nwaves) {
      const unsigned long long b = on ? __ballot(used(sym, kc)) : 0ull;
      if (lane == 0) {
        cnt[sym * cps + kc] = __popcll(b);
        msk[sym * cps + kc] = b;
      }
    }
  }
  __syncthreads();
  if (wave == 0) { // exclusive prefix over <= 294 entries: five consecutive entries per lane, then a wavefront scan
    constexpr int PL = (14 * 21 + 63) / 64;
    int           v[PL], sum = 0;
#pragma unroll
    for (int j = 0; j < PL; j++) {
      const int c = lane * PL + j;
      v[j]        = c < nchunks ? cnt[c] : 0;
      sum += v[j];
    }
    int incl = sum;
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    int acc = incl - sum;
#pragma unroll
    for (int j = 0; j < PL; j++) {
      const int c = lane * PL + j;
      if (c < nchunks) cnt[c] = acc;
      acc += v[j];
    }
  }
  __syncthreads();
  uint32_t* o = idx_out + (size_t)sf * max_re;
  for (int sym = (g.lstart < nsl ? g.lstart : nsl); sym < nsym; sym++) {
    for (int kc = wave; kc < cps; kc += nwaves) {
      const unsigned long long b = msk[sym * cps + kc];
      if ((b >> lane) & 1ull) o[cnt[sym * cps + kc] + __popcll(b & ((1ull << lane) - 1ull))] = (uint32_t)(sym * nre + kc * 64 + lane);
    }
  }
}
__device__ __forceinline__ void scr_gen_body(const GrantDev* __restrict__ gr, const uint32_t* __restrict__ basis, uint32_t* __restrict__ out, int words,
                                             int cell_id, int sf, int w)
{
  if (w >= words) return;
  const GrantDev g = gr[sf];
  uint32_t       c_init = ((uint32_t)g.rnti << 14) + ((uint32_t)g.cw << 13) + ((uint32_t)g.sf_idx << 9) + (uint32_t)cell_id, v = basis[w];
  for (int j = 0; j < 31; j++) {
    if ((c_init >> j) & 1u) v ^= basis[(size_t)(1 + j) * words + w];
  }
  out[(size_t)sf * words + w] = v;
}
__global__ __launch_bounds__(256) void scr_gen_kernel(const GrantDev* __restrict__ gr, const uint32_t* __restrict__ basis, uint32_t* __restrict__ out,
                                                      int words, int cell_id)
{
  scr_gen_body(gr, basis, out, words, cell_id, (int)blockIdx.y, (int)(blockIdx.x * 256 + threadIdx.x));
}
// A call's descriptors from the pinned host buffer to the device by a kernel of the call's stream (the uplink's grants mode; the downlink's does it in
// grants_prep_kernel): hipMemcpyAsync of 100-200 KB was a 17-56 us blit kernel or an engine hand-over there (profiles/r04/ab_mix_kernel.txt, 10)
__global__ __launch_bounds__(256) void desc_copy_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, int n16)
{
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (i < n16) dst[i] = src[i];
}

// The two per-call preparations of the DL grants mode in ONE launch: workgroups 0 .. nof_sf - 1 list the subframes' REs, the ones behind them
// make the scrambling sequences (RELIST_THREADS words each; codeword 0 of every subframe, then - gr1 != null - codeword 1). Neither depends on
// the other; as two launches in a row on the call's stream the second waited for the first (profiles/r04/ab_mix_kernel.txt, 5)
__global__ __launch_bounds__(RELIST_THREADS) void grants_prep_kernel(const GrantDev* __restrict__ gr, uint32_t* __restrict__ idx_out, int P, int cell_id,
                                                                     int max_re, int nof_ports, int nsl, int nof_sf, const uint32_t* __restrict__ basis,
                                                                     uint32_t* __restrict__ scr0, const GrantDev* __restrict__ gr1,
                                                                     uint32_t* __restrict__ scr1, int words, uint8_t* __restrict__ tb_ok, int nrows,
                                                                     const uint4* __restrict__ desc_src, uint4* __restrict__ desc_dst, int desc_n16,
                                                                     int copy_first)
{
  // Third role (workgroups from copy_first on): the call's descriptors from the pinned host buffer to the device - what a hipMemcpyAsync in front of
  // this launch did (an engine hand-over or a 17-56 us blit kernel on the call's stream). gr / gr1 then point into the HOST buffer: the two roles
  // above read their 64-byte grant from there (wave-uniform loads), every later kernel reads the device copy.
  if ((int)blockIdx.x >= copy_first) {
    const int i = ((int)blockIdx.x - copy_first) * RELIST_THREADS + (int)threadIdx.x;
    if (i < desc_n16) desc_dst[i] = desc_src[i];
    return;
  }
  if ((int)blockIdx.x < nof_sf) {
    // the call's verdict rows start at "no transport block" (rows behind the first nof_sf: second codewords): the decoders' own assembly only
    // writes the rows that have one
    if (threadIdx.x == 0) {
      tb_ok[blockIdx.x] = 0;
      if ((int)blockIdx.x + nof_sf < nrows) tb_ok[blockIdx.x + nof_sf] = 0;
    }
    pdsch_relist_body(gr, idx_out, P, cell_id, max_re, nof_ports, nsl, (int)blockIdx.x);
    return;
  }
  const int per = (words + RELIST_THREADS - 1) / RELIST_THREADS;
  int       b = (int)blockIdx.x - nof_sf;
  const int cw = b / (nof_sf * per);
  b -= cw * nof_sf * per;
  const int sf = b / per, w = (b - sf * per) * RELIST_THREADS + (int)threadIdx.x;
  scr_gen_body(cw ? gr1 : gr, basis, cw ? scr1 : scr0, words, cell_id, sf, w);
}

// Same result from the per-block syndrome shares the windowed turbo decoders emit (TdecOpts::tb_rem): the CRC is linear,
// so the TB syndrome is the XOR of the C shares; what is left is the payload copy.
__global__ __launch_bounds__(256) void tb_asm_kernel(const uint8_t* __restrict__ cb_bytes, const uint8_t* __restrict__ cb_ok,
                                                     const uint32_t* __restrict__ cb_syn, uint8_t* __restrict__ tb, uint8_t* __restrict__ tb_ok,
                                                     TbGeom g)
{
  // the subframe's code-block bytes (C x cb_stride, contiguous) come in with 8-byte loads, the transport block leaves with 4-byte stores:
  // byte-wide global accesses made this 2.4 MB copy cost 16 us
  __shared__ __attribute__((aligned(8))) uint8_t cbb[32 * 768];
  const int      sf = blockIdx.x, nbytes = g.tbs / 8 + 3, rb = g.rlen / 8, tot = g.C * g.cb_stride;
  const uint8_t* src0 = cb_bytes + (size_t)sf * tot;
  uint8_t*       dst = tb + (size_t)sf * g.tb_stride;
  if ((reinterpret_cast<uintptr_t>(src0) & 7) == 0) {
    for (int i = threadIdx.x; i < tot / 8; i += blockDim.x) reinterpret_cast<uint64_t*>(cbb)[i] = reinterpret_cast<const uint64_t*>(src0)[i];
    for (int i = tot / 8 * 8 + threadIdx.x; i < tot; i += blockDim.x) cbb[i] = src0[i];
  } else {
    for (int i = threadIdx.x; i < tot; i += blockDim.x) cbb[i] = src0[i];
  }
  __syncthreads();
  auto src = [&](int b) -> uint32_t {
    int cb = b / rb;
    if (cb > g.C - 1) cb = g.C - 1;
    const int off = b - cb * rb;
    return off < g.K / 8 ? cbb[cb * g.cb_stride + off] : 0u;
  };
  const bool a4 = ((reinterpret_cast<uintptr_t>(dst) | (uintptr_t)g.tb_stride) & 3) == 0;
  const int  n  = nbytes + 3, n4 = a4 ? n / 4 : 0;
  for (int w = threadIdx.x; w < n4; w += blockDim.x)
    reinterpret_cast<uint32_t*>(dst)[w] = src(4 * w) | (src(4 * w + 1) << 8) | (src(4 * w + 2) << 16) | (src(4 * w + 3) << 24);
  for (int b = 4 * n4 + threadIdx.x; b < n; b += blockDim.x) dst[b] = (uint8_t)src(b);
  if (threadIdx.x == 0) {
    uint32_t syn = 0;
    bool     ok  = true;
    for (int c = 0; c < g.C; c++) {
      syn ^= cb_syn[sf * g.C + c];
      ok = ok && cb_ok[sf * g.C + c];
    }
    // par_rx == par_tx && par_rx != 0 (sch.c:481): a zero parity with zero syndrome is rejected upstream
    ok        = ok && syn == 0 && (src(g.tbs / 8) | src(g.tbs / 8 + 1) | src(g.tbs / 8 + 2)) && tb_any_block_decoded(g.iters, sf * g.C, g.C);
    tb_ok[sf] = ok ? 1 : 0;
  }
}

// largest segment of any subframe class + the Qm extra LLRs of the last blocks must fit the LDS kernel; w_stride is a multiple of 32
int rm_lds_bytes(const RmGeom& g, int llr_bytes)
{
  int mx = g.nof_re[0] > g.nof_re[1] ? g.nof_re[0] : g.nof_re[1];
  mx     = mx > g.nof_re[2] ? mx : g.nof_re[2];
  return ((g.Qm * (mx / g.C) + 2 * g.Qm) * llr_bytes + 32 + 15) & ~15; // + the bytes below the 16-byte boundary and the rounded-up last load
}

// rate de-matching of nblk code blocks: rm_rx_lds_kernel with `lds` bytes of LDS when they fit 64 KB, else rm_rx_kernel (1024 / sizeof(T)
// slots of w_stride per workgroup)
template <typename T>
int rm_rx_launch(int lds, uint32_t nblk, const void* e, void* w, const uint32_t* tbl, const RmGeom& g, hipStream_t st)
{
  if (lds <= 64 * 1024) {
    hipLaunchKernelGGL(rm_rx_lds_kernel<T>, dim3(nblk), dim3(256), lds, st, (const T*)e, (T*)w, tbl, g);
  } else {
    hipLaunchKernelGGL(rm_rx_kernel<T>, dim3(ceil_div(g.w_stride, 1024 / (int)sizeof(T)), nblk), dim3(256), 0, st, (const T*)e, (T*)w, tbl, g);
  }
  LAUNCH_CHECK();
  return SRSLTE_SUCCESS;
}

// slot -> circular-buffer position: 32-bit entries [w_stride] for the generic kernels, then the same as 16-bit entries for the LDS kernel
std::vector<uint32_t> rm_slot_table(const std::vector<uint32_t>& t, uint32_t w_stride)
{
  std::vector<uint32_t> inv(w_stride + w_stride / 2, 0xffffffffu);
  uint16_t*             inv16 = reinterpret_cast<uint16_t*>(inv.data() + w_stride);
  for (uint32_t n = 0; n < t.size(); n++) {
    if (t[n] == 0xffffffffu) continue; // a position without a slot (rm_parity_compact)
    inv[t[n]]   = n;
    inv16[t[n]] = (uint16_t)n; // n < 3 * 6144 + 12
  }
  return inv;
}

// pdsch.c:81-206 as a per-RE rule (see oracle/orc_pdsch.c for the derivation): symbol-major, sub-carrier ascending,
// skipping CRS, and the central 72 sub-carriers of the PSS/SSS symbols (slot 0, l >= 5, sf 0/5) and PBCH symbols (slot 1, l < 4, sf 0)
// pmch_cp (pmch.c:44-99): the PMCH's RE in the 12-symbol MBSFN subframe in mapping order - every PRB from symbol lstart on; the symbols of the
// MBSFN reference signal (SRSLTE_SYMBOL_HAS_REF_MBSFN: l = 2 of slot 0, l = 0 and 4 of slot 1) keep every second sub-carrier for data: prb_cp_ref
// with six references per PRB (prb_dl.c:45-76) leaves the odd ones, the even ones where the references sit at offset 1 (symbol 0 of slot 1)
void pmch_re_indices(uint32_t nof_prb, uint32_t lstart, std::vector<uint32_t>& idx)
{
  idx.clear();
  for (uint32_t s = 0; s < 2; s++) {
    for (uint32_t l = (s == 0 ? lstart : 0); l < 6; l++) {
      const bool     has_ref = (l == 2 && s == 0) || (l == 0 && s == 1) || (l == 4 && s == 1);
      const uint32_t keep    = (l == 0 && s == 1) ? 0 : 1;
      for (uint32_t k = 0; k < 12 * nof_prb; k++) {
        if (!has_ref || (k & 1) == keep) idx.push_back((6 * s + l) * 12 * nof_prb + k);
      }
    }
  }
}

void pdsch_re_indices(uint32_t cell_id, uint32_t nof_prb, uint32_t nof_ports, uint32_t sf_idx, uint32_t lstart, std::vector<uint32_t>& idx,
                      uint32_t nsl = 7)
{
  const uint32_t nre = 12 * nof_prb, step = nof_ports == 1 ? 6 : 3; // 2/4 ports: the other ports' CRS positions are left empty too (pdsch.c:103-107)
  idx.clear();
  for (uint32_t s = 0; s < 2; s++) {
    for (uint32_t l = (s == 0 ? lstart : 0); l < nsl; l++) {
      const bool     has_ref = l == 0 || l == nsl - 3 || (l == 1 && nof_ports == 4); // phy_common.h:139-141
      const uint32_t offset  = l == 0 ? cell_id % 6 : (cell_id + 3) % 6;
      const bool     sync    = (s == 0 && (sf_idx == 0 || sf_idx == 5) && l >= nsl - 2) || (s == 1 && sf_idx == 0 && l < 4);
      for (uint32_t k = 0; k < nre; k++) {
        if (sync && k + 36 >= nre / 2 && k < nre / 2 + 36) continue;
        if (has_ref && (k % step) == offset % step) continue;
        idx.push_back((s * nsl + l) * nre + k);
      }
    }
  }
}

// an empty vector still gets one element: the objects test these buffers for "present"
template <typename T>
int upload(DevBuf<T>& d, const std::vector<T>& h)
{
  if (h.empty() ? d.alloc(1) : d.upload(h)) {
    hip_log("[srslte_hip] upload of a %zu-byte table to the device failed\n", sizeof(T) * h.size());
    return SRSLTE_ERROR;
  }
  return SRSLTE_SUCCESS;
}

// rate de-matching table of (K, rv) (rm_turbo.c:160-260) in the turbo decoder's input layout, as rm_slot_table's slot table of w_stride; W != 0:
// the windowed decoders' layout (stream s at s (K + 32), bit i at (i % (K / W)) W + i / (K / W), the tails behind the three streams)
int rm_rx_table_upload(uint32_t K, uint32_t rv, uint32_t W, uint32_t w_stride, DevBuf<uint32_t>& d_tbl)
{
  std::vector<uint32_t> t;
  lte_rm_rx_table(K, rv, t);
  if (W) {
    for (auto& v : t) v = v < 3 * K ? (v % 3) * (K + 32) + ((v / 3) % (K / W)) * W + (v / 3) / (K / W) : (v - 3 * K) + 3 * (K + 32);
  }
  return upload(d_tbl, rm_slot_table(t, w_stride));
}

// Punctured parity at a quarter of its rows. At a high code rate the receiver gets the first few columns of the parity sub-block interleavers
// only (36.212 5.1.4.1.1: columns 0, 16, 8, 24, 4, 20, 12, 28 come first, all = 0 mod 4), which in the 16-window layout of a block with
// Lw = K / 16 = 0 mod 4 are the rows r = phase mod 4 of each parity stream - one 32-byte row of every 128-byte line. The compact layout of
// rv 0 keeps those rows alone: the systematic stream as it is, row r of parity stream 1 + i (r % 4 == phase[i]) as row r / 4 of K / 4 slots at
// K + 32 + i K / 4, the tails at K + 32 + K / 2; `len` slots (a multiple of 32) instead of 3 (K + 32) + 12. Nothing is hard-coded about the
// interleaver: the phases are those of each stream's first position in the circular buffer, and e_lim is the first position whose slot the
// layout does not hold - a block of at most e_lim LLRs loses nothing. The 16-window 16-bit decoder reads it (TdecOpts::pc).
struct RmParityCompact {
  uint32_t phase[2], len, e_lim;
};
// false: no such layout for this K (K % 64 != 0). t: lte_rm_rx_table's positions replaced by their slots, 0xffffffff where there is none
bool rm_parity_compact(uint32_t K, RmParityCompact& c, std::vector<uint32_t>* t_out = nullptr)
{
  if (K % 64 || K / 16 < 4) return false;
  std::vector<uint32_t> t;
  lte_rm_rx_table(K, 0, t);
  const uint32_t Lw = K / 16;
  bool           seen[2] = {false, false};
  c.phase[0] = c.phase[1] = 0;
  c.len   = (K + 32 + K / 2 + 12 + 31) & ~31u;
  c.e_lim = (uint32_t)t.size();
  for (uint32_t n = 0; n < t.size(); n++) {
    const uint32_t v = t[n], s = v % 3, i = v / 3;
    if (v >= 3 * K) {
      t[n] = (v - 3 * K) + K + 32 + K / 2;
    } else if (s == 0) {
      t[n] = (i % Lw) * 16 + i / Lw;
    } else {
      const uint32_t r = i % Lw;
      if (!seen[s - 1]) {
        seen[s - 1]    = true;
        c.phase[s - 1] = r % 4;
      }
      if (r % 4 == c.phase[s - 1]) {
        t[n] = K + 32 + (s - 1) * (K / 4) + (r / 4) * 16 + i / Lw;
      } else {
        if (c.e_lim == t.size()) c.e_lim = n;
        t[n] = 0xffffffffu;
      }
    }
  }
  if (t_out) t_out->swap(t);
  return true;
}
int rm_rx_table_upload_compact(uint32_t K, RmParityCompact& c, DevBuf<uint32_t>& d_tbl)
{
  std::vector<uint32_t> t;
  if (!rm_parity_compact(K, c, &t)) return SRSLTE_ERROR_INVALID_INPUTS;
  return upload(d_tbl, rm_slot_table(t, c.len));
}

// A block's soft buffer from the compact layout above to the whole one, in place: one workgroup per block takes the compact parity rows and
// the tails through LDS, then writes both parity streams (zeros and the rows held), the tails and the padding up to the block's stride - slot for
// slot what the rate de-matcher leaves with the whole table
__global__ __launch_bounds__(256) void rm_parity_expand_kernel(int16_t* __restrict__ w, int w_stride, int K, int phase0, int phase1)
{
  __shared__ __attribute__((aligned(16))) int16_t cp[6144 / 2 + 16]; // the longest code block's two quarter streams and tails
  int16_t*  p  = w + (size_t)blockIdx.x * w_stride;
  const int nc = K / 2 + 12, base = K + 32;
  for (int i = threadIdx.x; i < (nc + 7) / 8; i += 256) reinterpret_cast<uint4*>(cp)[i] = reinterpret_cast<const uint4*>(p + base)[i];
  __syncthreads();
  const int per = (K + 32) / 8; // 16-byte half rows of a whole stream, padding included
  for (int j = threadIdx.x; j < 2 * per; j += 256) {
    const int s = j >= per, h = j - s * per, r = h >> 1;
    uint4     v = make_uint4(0, 0, 0, 0);
    if (r < K / 16 && (r & 3) == (s ? phase1 : phase0)) v = *reinterpret_cast<const uint4*>(cp + s * (K / 4) + (r >> 2) * 16 + (h & 1) * 8);
    *reinterpret_cast<uint4*>(p + (1 + s) * (K + 32) + h * 8) = v;
  }
  for (int i = 3 * (K + 32) + threadIdx.x; i < w_stride; i += 256) p[i] = i < 3 * (K + 32) + 12 ? cp[K / 2 + i - 3 * (K + 32)] : (int16_t)0;
}

// rate matching table of (K, rv) (rm_turbo.c:100-158): the coded bit of each circular-buffer position from k0(rv) on, addressed in the encoder's
// byte streams (systematic byte p, tail bit (1 << 30) | p - K, parity bytes (2 << 30) | p of stream 1, K + 4 + p of stream 2)
int rm_tx_table_upload(uint32_t K, uint32_t rv, DevBuf<uint32_t>& d_tbl)
{
  std::vector<uint32_t> t;
  lte_rm_rx_table(K, rv, t);
  for (auto& v : t) {
    const uint32_t p = v / 3, s = v % 3;
    v = s == 0 ? (p < K ? p : (1u << 30) | (p - K)) : (2u << 30) | (s == 1 ? p : K + 4 + p);
  }
  return upload(d_tbl, t);
}

// the levels of one axis of modulation mod (1 QPSK .. 4 256QAM) for each of its 2^mod bit patterns (36.211 7.1.2-7.1.5, lte_tables.c:57-262)
void constellation_levels(int mod, float* lvl)
{
  for (uint32_t idx = 0; idx < (1u << mod); idx++) {
    double v = 1.0;
    for (int i = mod - 1; i >= 1; i--) v = (double)(1 << (mod - i)) - (1 - 2 * (int)((idx >> (mod - 1 - i)) & 1)) * v;
    const double norm = mod == 1 ? sqrt(2.0) : (mod == 2 ? sqrt(10.0) : (mod == 3 ? sqrt(42.0) : sqrt(170.0)));
    lvl[idx]          = (float)((1 - 2 * (int)((idx >> (mod - 1)) & 1)) * v / norm);
  }
}

// srslte_rm_conv_tx (rm_conv.c:44-89) for a CQI report of cqi_len bits (+ 8 CRC bits): the coded bits 3 i + stream in the order the sub-block
// interleaved streams are read, dummies skipped - one turn of the circular buffer
std::vector<uint16_t> cqi_rm_conv_order(uint32_t cqi_len)
{
  static const uint8_t perm[32] = {1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31, 0, 16, 8, 24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30};
  const int             F = (int)cqi_len + 8, nrows = (F - 1) / 32 + 1, ndummy = nrows * 32 - F;
  std::vector<uint16_t> w;
  for (int s = 0; s < 3; s++) {
    for (int j = 0; j < 32; j++) {
      for (int i = 0; i < nrows; i++) {
        const int pos = i * 32 + perm[j];
        if (pos >= ndummy) w.push_back((uint16_t)((pos - ndummy) * 3 + s));
      }
    }
  }
  return w;
}

// srslte_refsignal_cs_put_sf (refsignal_dl.c:253-272) as a grid initialiser: the CRS of `port` in its first nsym CRS symbols (ports 0 / 1:
// 0, nsl - 3, nsl, 2 nsl - 3; ports 2 / 3: 1, nsl + 1) -> -(pilot index + 2) in src, a subframe of 12 P sub-carriers per symbol
void crs_src_put(int32_t* src, uint32_t port, int nsym, uint32_t nsl, uint32_t P, uint32_t cell_id)
{
  for (int l = 0; l < nsym; l++) {
    const uint32_t sym = port >= 2 ? 1 + nsl * l : ((l & 1) ? (l / 2 + 1) * nsl - 3 : (l / 2) * nsl), fidx = ((((l + port) & 1) ? 3 : 0) + cell_id % 6) % 6;
    for (uint32_t i = 0; i < 2 * P; i++) src[sym * 12 * P + fidx + 6 * i] = -(int32_t)(l * 2 * P + i) - 2;
  }
}

} // namespace
