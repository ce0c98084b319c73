// PUCCH formats 1, 1a, 1b, 2, 2a and 2b for gfx950 (include/srslte_hip/phy_hip.h, "UL control"): one launch per call on the caller's stream.
//   ul_pucch_rx_kernel  one wavefront per request: srslte_chest_ul_estimate_pucch + srslte_pucch_decode (+ the SR retry of
//                       srslte_enb_ul_get_pucch), the RM(20, A) search of srslte_uci_decode_cqi_pucch over the 64 lanes
//   ul_pucch_tx_kernel  one wavefront per request: encode_signal_format12 + pucch_put and srslte_refsignal_dmrs_pucch_gen / _put
// The format and resource of a request are chosen on the host when the call is made (srslte_ue_ul_pucch_resource_selection); the device
// derives the cyclic shifts from integer state and the per-(slot, symbol) tables the object keeps.
#include "cf32_dev.hpp"
#include "common.hpp"
#include "ctrl_rx_dev.hpp"
#include "demod_dev.hpp"
#include "dev_buf.hpp"
#include "phy_hip_internal.hpp"
#include <math.h>
#include <string.h>
#include <vector>

void ul_r_uv_arg_1prb(uint32_t u, float* arg); // chest.hip

namespace {

enum { F1 = 0, F1A, F1B, F2, F2A, F2B, F_ERR = 7 };
constexpr int MAX_RE = 120; // 2 slots x 5 symbols x 12 (SRSLTE_PUCCH_MAX_SYMBOLS holds them)

// the object's tables (device): per slot of the frame the group's base-sequence phases and n_cs_cell per symbol, the orthogonal sequences
// as the reference's float tables, the RM(20, 13) basis rows and the Gold sequence's bases
struct UlCtrlTab {
  float    arg[20][12];       // srslte_refsignal_r_uv_arg_1prb(u(ns)) with u = (f_gh(ns) [group hopping] + cell_id % 30) % 30
  uint32_t n_cs_cell[20][7];  // srslte_pucch_n_cs_cell (pucch.c:954-972)
  float    w_dmrs1[3][3];     // w_arg_pucch_format1_cpnorm (refsignal_ul.c:46-48), [n_oc][m]
  float    w_dmrs1e[3][2];    // w_arg_pucch_format1_cpext (:50-52)
  float    w_n_oc[2][3][4];   // w_n_oc of pucch.c:297-303, [N_sf == 3][n_oc][m]
  float    alpha[12];         // 2 pi n_cs / 12 as srslte_pucch_alpha_format1 / 2 return it
  float    s_ns;              // S(ns) = pi / 2 (pucch.c:472-475)
  uint32_t rm_row[20];        // M_basis_seq_pucch (uci.c:79-100) row i as a 13-bit mask, basis bit n -> bit 12 - n (srslte_bit_unpack order)
  uint32_t gold0, gold_basis[31]; // c(0..19) of c_init 0, and c(0..19) of c_init 1 << i XOR it: c of any c_init is their XOR
};

struct UlCtrlGeom {
  int   nof_prb, nsl, cp_ext;
  int   delta, N_cs, n_rb_2;
  float th1, th1a, th2;
  int   cell_id;
};

// a request as the device sees it: the resources decided on the host (attempt 0, and the SR retry's attempt 1: format < 0 = none)
struct PucchDesc {
  int      sf, shortened, sr_tti, ack_len, data_enable, ri_len, uci_len;
  int      format[2], n_pucch[2];
  uint32_t rnti;
  float    noise;
};
// a transmit request: format, resource, the modulated values decided on the host (1/1a/1b: d(0); 2a/2b: the DMRS's z(1)) and the RM-coded
// 20 bits of a format 2 (scrambled on the device)
struct PucchTxDesc {
  int      sf, shortened, format, n_pucch;
  uint32_t rnti, coded;
  float    d0[2], z1[2];
};

__device__ __forceinline__ cf32 cexpi(float x)
{
  float s, c;
  sincosf(x, &s, &c);
  return make_float2(c, s);
}

// get_N_sf (pucch.c:314-339) for formats 1-2b
__host__ __device__ __forceinline__ int n_sf(int fmt, int slot, int shortened) { return fmt >= F2 ? 5 : (slot && shortened ? 3 : 4); }
// get_pucch_symbol (pucch.c:341-377)
__host__ __device__ __forceinline__ int data_sym(int fmt, int m, int ext)
{
  if (fmt >= F2) return ext ? (m < 3 ? m : m + 1) : (m == 0 ? 0 : (m < 4 ? m + 1 : 6)); // {0,1,2,4,5} / {0,2,3,4,6}
  return ext ? (m < 2 ? m : m + 2) : (m < 2 ? m : m + 3);                               // {0,1,4,5} / {0,1,5,6}
}
// srslte_refsignal_dmrs_N_rs / _pucch_symbol (refsignal_ul.c:489-555)
__host__ __device__ __forceinline__ int n_rs(int fmt, int ext) { return fmt < F2 ? (ext ? 2 : 3) : (fmt == F2 ? (ext ? 1 : 2) : 2); }
__host__ __device__ __forceinline__ int dmrs_sym(int fmt, int m, int ext)
{
  if (fmt < F2) return 2 + m;     // {2,3,4} / {2,3}
  if (fmt == F2 && ext) return 3; // {3}
  return m ? 5 : 1;               // {1,5}: format 2 normal CP, and 2a / 2b on either CP
}

// srslte_pucch_m + srslte_pucch_n_prb (pucch.c:911-952) for slot ns % 2
__host__ __device__ __forceinline__ uint32_t pucch_n_prb(int fmt, uint32_t n_pucch, uint32_t slot, uint32_t nof_prb, uint32_t delta, uint32_t N_cs,
                                                         uint32_t n_rb_2, int ext)
{
  uint32_t m;
  if (fmt < F2) {
    const uint32_t c = ext ? 2 : 3;
    m                = n_rb_2;
    if (n_pucch >= c * N_cs / delta) m = (n_pucch - c * N_cs / delta) / (c * 12 / delta) + n_rb_2 + (uint32_t)ceilf((float)N_cs / 8);
  } else {
    m = n_pucch / 12;
  }
  return ((m + slot) % 2) ? nof_prb - 1 - m / 2 : m / 2;
}

// srslte_pucch_alpha_format1 with is_dmrs = true, as encode_signal_format12 and the DMRS call it (pucch.c:974-1031): n_cs; n_oc and n'(ns)
__host__ __device__ __forceinline__ uint32_t alpha1(const uint32_t (*n_cs_cell)[7], int ext, uint32_t D, uint32_t Ncs, uint32_t n_pucch, uint32_t ns,
                                                    uint32_t l, uint32_t* n_oc_out, uint32_t* n_prime_out)
{
  const uint32_t c = ext ? 2 : 3, thr = c * Ncs / D;
  const uint32_t Np = n_pucch < thr ? Ncs : 12;
  uint32_t       np = n_pucch;
  if (n_pucch >= thr) np = (n_pucch - thr) % (c * 12 / D);
  if (ns % 2) {
    if (n_pucch >= thr) {
      np = (c * (np + 1)) % (c * 12 / D + 1) - 1;
    } else {
      const uint32_t d = ext ? 0 : 2, h = (np + d) % (c * Np / D);
      np = (h / c) + (h % c) * Np / D;
    }
  }
  const uint32_t n_oc = np * D / Np;
  *n_oc_out = n_oc, *n_prime_out = np;
  return ext ? (n_cs_cell[ns][l] + (np * D + n_oc) % Np) % 12 : (n_cs_cell[ns][l] + (np * D + (n_oc % D)) % Np) % 12;
}

// srslte_pucch_alpha_format2 (pucch.c:1034-1058): n_cs
__host__ __device__ __forceinline__ uint32_t alpha2(const uint32_t (*n_cs_cell)[7], uint32_t Ncs, uint32_t n_rb_2, uint32_t n_pucch, uint32_t ns,
                                                    uint32_t l)
{
  const bool hi = n_pucch >= 12u * n_rb_2;
  uint32_t   np = hi ? (n_pucch + Ncs + 1) % 12 : n_pucch % 12;
  if (ns % 2) {
    np = (12 * (np + 1)) % 13 - 1;
    if (hi) {
      const int x = (12 - 2 - (int)n_pucch) % 12;
      np          = x >= 0 ? (uint32_t)x : (uint32_t)(12 + x);
    }
  }
  return (n_cs_cell[ns][l] + np) % 12;
}

// element i of encode_signal_format12's z with d = 1 (the signal_only reference of decode_signal, and the base the hypotheses scale):
// slot i / (N_sf(0) 12), symbol m, subcarrier n
__device__ __forceinline__ cf32 base_signal(const UlCtrlTab* t, const UlCtrlGeom& g, int fmt, uint32_t n_pucch, int shortened, uint32_t sf_idx, int i)
{
  const int      n0 = n_sf(fmt, 0, shortened), s = i >= n0 * 12 ? 1 : 0, j = i - s * n0 * 12, m = j / 12, n = j % 12;
  const uint32_t ns = 2 * sf_idx + s, l = (uint32_t)data_sym(fmt, m, g.cp_ext);
  if (fmt >= F2) {
    const float alpha = t->alpha[alpha2(t->n_cs_cell, (uint32_t)g.N_cs, (uint32_t)g.n_rb_2, n_pucch, ns, l)];
    return cexpi(t->arg[ns][n] + alpha * (float)n);
  }
  uint32_t    n_oc, np;
  const float alpha = t->alpha[alpha1(t->n_cs_cell, g.cp_ext, (uint32_t)g.delta, (uint32_t)g.N_cs, n_pucch, ns, l, &n_oc, &np)];
  const float S     = (np % 2) ? t->s_ns : 0.f;
  const int   widx  = n_sf(fmt, s, shortened) == 3 ? 1 : 0;
  return cexpi(t->w_n_oc[widx][n_oc % 3][m] + t->arg[ns][n] + alpha * (float)n + S);
}

// element i of srslte_refsignal_dmrs_pucch_gen with z(1) = 1: slot i / (N_rs 12), DMRS symbol m, subcarrier n
__device__ __forceinline__ cf32 dmrs_signal(const UlCtrlTab* t, const UlCtrlGeom& g, int fmt, uint32_t n_pucch, uint32_t sf_idx, int i)
{
  const int      nrs = n_rs(fmt, g.cp_ext), s = i / (nrs * 12), m = (i / 12) % nrs, n = i % 12;
  const uint32_t ns = 2 * sf_idx + s, l = (uint32_t)dmrs_sym(fmt, m, g.cp_ext);
  float          w = 0.f, alpha;
  if (fmt < F2) {
    uint32_t n_oc, np;
    alpha = t->alpha[alpha1(t->n_cs_cell, g.cp_ext, (uint32_t)g.delta, (uint32_t)g.N_cs, n_pucch, ns, l, &n_oc, &np)];
    w     = g.cp_ext ? t->w_dmrs1e[n_oc][m] : t->w_dmrs1[n_oc][m];
  } else {
    alpha = t->alpha[alpha2(t->n_cs_cell, (uint32_t)g.N_cs, (uint32_t)g.n_rb_2, n_pucch, ns, l)];
  }
  return cexpi(w + t->arg[ns][n] + alpha * (float)n);
}

// c(0..19) of srslte_sequence_pucch (sequences.c:72-74) for (rnti, subframe): bit k of the word is c(k)
__device__ __forceinline__ uint32_t pucch_seq(const UlCtrlTab* t, uint32_t rnti, uint32_t sf_idx, uint32_t cell_id)
{
  const uint32_t c_init = (((sf_idx + 1) * (2 * cell_id + 1)) << 16) + rnti;
  uint32_t       w      = t->gold0;
  for (int i = 0; i < 31; i++)
    if ((c_init >> i) & 1u) w ^= t->gold_basis[i];
  return w;
}

struct RxLds {
  cf32  dm[72];    // DMRS LS estimates [2][N_rs][12]
  cf32  ce[2][12]; // per-slot estimates after the filter
  cf32  z[MAX_RE]; // format 2: z conj(ref)
  short llr[20];
  int   bcorr[64], bw[64];
};

struct Attempt {
  int      detected;
  float    corr;
  uint8_t  bits[2]; // pucch_bits[0..1] (1a / 1b) or the decoded word's first bits
  uint8_t  drs[2];  // pucch2_drs_bits
  uint32_t word;    // format 2: the decoded 13-bit word
};

// srslte_chest_ul_estimate_pucch + srslte_pucch_decode's equalisation and decode_signal for one (format, n_pucch); every lane returns the same
__device__ Attempt decode_attempt(const UlCtrlTab* t, const UlCtrlGeom& g, const cf32* grid, const PucchDesc& d, int fmt, uint32_t n_pucch,
                                  uint32_t sf_idx, RxLds& L, cf32* dbg_z, short* dbg_llr)
{
  const int lane = threadIdx.x, W = 12 * g.nof_prb, nrs = n_rs(fmt, g.cp_ext);
  Attempt   a;
  a.bits[0] = a.bits[1] = a.drs[0] = a.drs[1] = 0, a.word = 0, a.detected = 0, a.corr = 0.f;
  const uint32_t prb0 = pucch_n_prb(fmt, n_pucch, 0, (uint32_t)g.nof_prb, (uint32_t)g.delta, (uint32_t)g.N_cs, (uint32_t)g.n_rb_2, g.cp_ext);
  const uint32_t prb1 = pucch_n_prb(fmt, n_pucch, 1, (uint32_t)g.nof_prb, (uint32_t)g.delta, (uint32_t)g.N_cs, (uint32_t)g.n_rb_2, g.cp_ext);
  // LS estimates against the DMRS with z(1) = 1; for 2a / 2b the sums of the m = 0 and m = 1 symbols decide the hypothesis
  float ar = 0.f, ai = 0.f, br = 0.f, bi = 0.f;
  for (int i = lane; i < 2 * nrs * 12; i += 64) {
    const int  s = i / (nrs * 12), m = (i / 12) % nrs, n = i % 12;
    const cf32 y = grid[(size_t)(s * g.nsl + dmrs_sym(fmt, m, g.cp_ext)) * W + (s ? prb1 : prb0) * 12 + n];
    const cf32 e = cmulconj(y, dmrs_signal(t, g, fmt, n_pucch, sf_idx, i));
    L.dm[i]      = e;
    if (m == 0) {
      ar += e.x, ai += e.y;
    } else if (m == 1) {
      br += e.x, bi += e.y;
    }
  }
  cf32 zsel = make_float2(1.f, 0.f);
  if (fmt == F2A || fmt == F2B) {
    ar = wave_sum(ar), ai = wave_sum(ai), br = wave_sum(br), bi = wave_sum(bi);
    // hypothesis h: pucch2_drs_bits = {h % 2, h / 2} and z(1) of srslte_pucch_format2ab_mod_bits; |sum y conj(z r)| with >= (chest_ul.c:354-372)
    float     mx = -1e9f;
    int       im = 0;
    const int nh = fmt == F2A ? 2 : 4;
    for (int h = 0; h < nh; h++) {
      const int   b0 = h % 2, b1 = h / 2;
      const cf32  z  = fmt == F2A ? make_float2(b0 ? -1.f : 1.f, 0.f)
                                  : (b0 == 0 ? (b1 == 0 ? make_float2(1.f, 0.f) : make_float2(0.f, -1.f))
                                             : (b1 == 0 ? make_float2(0.f, 1.f) : make_float2(-1.f, 0.f)));
      const cf32  bz = cmulconj(make_float2(br, bi), z);
      const float x  = hypotf(ar + bz.x, ai + bz.y);
      if (x >= mx) mx = x, im = h, zsel = z;
    }
    a.drs[0] = (uint8_t)(im % 2), a.drs[1] = (uint8_t)(im / 2);
  }
  __syncthreads();
  // each slot's mean over its DMRS symbols, then the 3-tap filter (chest_ul.c:382-396)
  if (lane < 24) {
    const int s = lane / 12, n = lane % 12;
    cf32      acc = L.dm[s * nrs * 12 + n];
    for (int m = 1; m < nrs; m++) {
      cf32 e = L.dm[(s * nrs + m) * 12 + n];
      if (m == 1) e = cmulconj(e, zsel);
      acc = cadd(acc, e);
    }
    L.ce[s][n] = cscale(acc, 1.0f / (float)nrs);
  }
  __syncthreads();
  cf32 o = make_float2(0.f, 0.f);
  if (lane < 24) {
    const int   s = lane / 12, k = lane % 12;
    const cf32* e = L.ce[s];
    const float f0 = 0.3333f, f1 = 1 - 2 * 0.3333f;
    if (k == 0) {
      const cf32 first = make_float2(e[1].x * 3.0f - e[0].x * 2.0f, e[1].y * 3.0f - e[0].y * 2.0f);
      o = cadd(cadd(cscale(first, f0), cscale(e[0], f1)), cscale(e[1], f0));
    } else if (k == 11) {
      const cf32 last = make_float2(e[11].x * 3.0f - e[10].x * 2.0f, e[11].y * 3.0f - e[10].y * 2.0f);
      o = cadd(cadd(cscale(e[10], f0), cscale(e[11], f1)), cscale(last, f0));
    } else {
      o = cadd(cadd(cscale(e[k - 1], f0), cscale(e[k], f1)), cscale(e[k + 1], f0));
    }
  }
  __syncthreads();
  if (lane < 24) L.ce[lane / 12][lane % 12] = o;
  __syncthreads();
  // pucch_get + srslte_predecoding_single (AVX body over 16 (n / 16) symbols, generic tail) + the base signal's sums
  const int n0 = n_sf(fmt, 0, d.shortened), nre = (n0 + n_sf(fmt, 1, d.shortened)) * 12, n16 = 16 * (nre / 16);
  float     sx = 0.f, sy = 0.f, cr = 0.f, ci = 0.f;
  for (int i = lane; i < nre; i += 64) {
    const int  s = i >= n0 * 12 ? 1 : 0, j = i - s * n0 * 12, m = j / 12, n = j % 12;
    const cf32 y = grid[(size_t)(s * g.nsl + data_sym(fmt, m, g.cp_ext)) * W + (s ? prb1 : prb0) * 12 + n];
    const cf32 h = L.ce[s][n];
    const cf32 x = i < n16 ? eq_single_avx(&y, &h, 1, 1, 0, d.noise) : eq_single_gen(&y, &h, 1, 1, 0, d.noise);
    const cf32 b = base_signal(t, g, fmt, n_pucch, d.shortened, sf_idx, i);
    dbg_z[i]     = x;
    if (fmt < F2) {
      sx += x.x * x.x + x.y * x.y;
      sy += b.x * b.x + b.y * b.y;
      const cf32 c = cmulconj(x, b);
      cr += c.x, ci += c.y;
    } else {
      L.z[i] = cmulconj(x, b);
    }
  }
  if (fmt < F2) {
    // srslte_vec_corr_ccc (vector.c:370-376) against d(0) b for every hypothesis: cov = Re(conj(d) sum x conj(b)) / len
    sx = wave_sum(sx), sy = wave_sum(sy), cr = wave_sum(cr), ci = wave_sum(ci);
    const float len = (float)nre, s_x = sx / len, s_y = sy / len, den = sqrtf(s_x * s_y);
    if (fmt == F1) {
      a.corr     = (cr / len) / den;
      a.detected = a.corr >= g.th1;
    } else {
      // 1a: b = 0, 1 -> d = 1, -1; 1b: (0,0) 1, (0,1) -j, (1,0) j, (1,1) -1 (pucch.c:190-212); the first maximum wins
      float     mx = -1e9f;
      const int nh = fmt == F1A ? 2 : 4;
      for (int h = 0; h < nh; h++) {
        const int b0 = fmt == F1A ? h : h / 2, b1 = fmt == F1A ? 0 : h % 2;
        // Re(conj(d) C): d = 1: cr; -1: -cr; -j: -ci; j: ci
        const float cov = fmt == F1A ? (b0 ? -cr : cr) : (b0 == 0 ? (b1 == 0 ? cr : -ci) : (b1 == 0 ? ci : -cr));
        const float c   = (cov / len) / den;
        if (c > mx) mx = c, a.bits[0] = (uint8_t)b0, a.bits[1] = (uint8_t)b1;
      }
      a.corr     = mx;
      a.detected = mx > g.th1;
    }
    return a;
  }
  __syncthreads();
  // format 2: the 12-RE means, int16 QPSK LLRs, descrambling, then the RM search
  if (lane < 10) {
    cf32 acc = make_float2(0.f, 0.f);
    for (int j = 0; j < 12; j++) acc = cadd(acc, make_float2(L.z[lane * 12 + j].x / 12.0f, L.z[lane * 12 + j].y / 12.0f));
    short v[2];
    demod_dev::demod_s(demod_dev::MOD_QPSK, acc, lane, 10, v);
    const uint32_t c = pucch_seq(t, d.rnti, sf_idx, (uint32_t)g.cell_id);
    for (int k = 0; k < 2; k++) {
      const short q         = ((c >> (2 * lane + k)) & 1u) ? (short)-v[k] : v[k];
      L.llr[2 * lane + k]   = q;
      dbg_llr[2 * lane + k] = q;
    }
  }
  __syncthreads();
  const int len = d.uci_len, step = 1 << (13 - len), nw = 1 << len;
  int       best = INT32_MIN, bw = 0;
  for (int k = lane; k < nw; k += 64) {
    const uint32_t w  = (uint32_t)(k * step);
    int            cc = 0;
    for (int j = 0; j < 20; j++) cc += (__popc(w & t->rm_row[j]) & 1) ? (int)L.llr[j] : -(int)L.llr[j];
    if (cc > best) best = cc, bw = (int)w; // ascending words per lane: the first maximum stays
  }
  L.bcorr[lane] = best, L.bw[lane] = bw;
  __syncthreads();
  if (lane == 0) {
    // the lowest word among the lanes' maxima: srslte_uci_decode_cqi_pucch's first maximum
    int mb = INT32_MIN, mw = 0;
    for (int l = 0; l < 64; l++)
      if (L.bcorr[l] > mb || (L.bcorr[l] == mb && L.bw[l] < mw)) mb = L.bcorr[l], mw = L.bw[l];
    L.bcorr[0] = mb, L.bw[0] = mw;
  }
  __syncthreads();
  a.word     = (uint32_t)L.bw[0];
  a.corr     = (float)(int16_t)L.bcorr[0] / 2000;
  a.detected = 1;
  a.bits[0] = (uint8_t)((a.word >> 12) & 1u), a.bits[1] = (uint8_t)((a.word >> 11) & 1u);
  __syncthreads();
  return a;
}

// grid = (nof), 64 threads
__global__ __launch_bounds__(64) void ul_pucch_rx_kernel(const UlCtrlTab* __restrict__ t, UlCtrlGeom g, const PucchDesc* __restrict__ desc,
                                                         const cf32* __restrict__ grid, uint32_t tti0, srslte_hip_pucch_res_t* __restrict__ out,
                                                         cf32* __restrict__ dbg_z, short* __restrict__ dbg_llr)
{
  __shared__ RxLds L;
  const int       r = blockIdx.x, lane = threadIdx.x;
  const PucchDesc d      = desc[r];
  const uint32_t  sf_idx = (tti0 + (uint32_t)d.sf) % 10;
  const cf32*     gs     = grid + (size_t)d.sf * 2 * g.nsl * 12 * g.nof_prb;
  cf32*           z      = dbg_z + (size_t)r * MAX_RE;
  short*          llr    = dbg_llr + (size_t)r * 20;
  for (int i = lane; i < MAX_RE; i += 64) z[i] = make_float2(0.f, 0.f);
  if (lane < 20) llr[lane] = 0;
  Attempt a  = decode_attempt(t, g, gs, d, d.format[0], (uint32_t)d.n_pucch[0], sf_idx, L, z, llr);
  int     at = 0;
  // decode_bits (pucch.c:710-739): an SR TTI reports the detection of the first attempt
  const int sr = d.sr_tti ? a.detected : 0;
  if (d.sr_tti && d.ack_len && !a.detected && d.format[1] >= 0) {
    a  = decode_attempt(t, g, gs, d, d.format[1], (uint32_t)d.n_pucch[1], sf_idx, L, z, llr);
    at = 1;
  }
  if (lane == 0) {
    const int               fmt = at ? d.format[1] : d.format[0];
    srslte_hip_pucch_res_t& o   = out[r];
    o.detected    = (uint32_t)a.detected;
    o.correlation = a.corr;
    o.format      = (uint32_t)fmt;
    o.n_pucch     = (uint32_t)(at ? d.n_pucch[1] : d.n_pucch[0]);
    o.sr          = (uint8_t)sr;
    const bool drs = d.data_enable || d.ri_len;
    for (int k = 0; k < 2; k++) o.ack[k] = k < d.ack_len ? (drs ? a.drs[k] : a.bits[k]) : 0;
    o.ack_valid = fmt == F1A || fmt == F1B ? (a.corr > g.th1a) : fmt >= F2 ? (a.corr > g.th2) : 0;
    o.cqi_crc   = fmt >= F2 ? (a.corr > g.th2) : 0;
    for (int k = 0; k < 13; k++) o.cqi[k] = fmt >= F2 ? (uint8_t)((a.word >> (12 - k)) & 1u) : 0;
    o.ri       = d.ri_len ? a.bits[0] : 0;
    o.reserved = 0;
  }
}

// grid = (nof), 64 threads: the PUCCH's data REs, then its DMRS
__global__ __launch_bounds__(64) void ul_pucch_tx_kernel(const UlCtrlTab* __restrict__ t, UlCtrlGeom g, const PucchTxDesc* __restrict__ desc,
                                                         uint32_t tti0, cf32* __restrict__ grid)
{
  const int         r = blockIdx.x, lane = threadIdx.x, W = 12 * g.nof_prb;
  const PucchTxDesc d      = desc[r];
  const int         fmt    = d.format;
  const uint32_t    sf_idx = (tti0 + (uint32_t)d.sf) % 10, n_pucch = (uint32_t)d.n_pucch;
  cf32*             gs     = grid + (size_t)d.sf * 2 * g.nsl * W;
  uint32_t          prb[2];
  for (int s = 0; s < 2; s++)
    prb[s] = pucch_n_prb(fmt, n_pucch, (uint32_t)s, (uint32_t)g.nof_prb, (uint32_t)g.delta, (uint32_t)g.N_cs, (uint32_t)g.n_rb_2, g.cp_ext);
  // uci_mod_bits (pucch.c:240-286): format 2 scrambles the 20 coded bits with srslte_sequence_pucch and maps them to QPSK
  const uint32_t cb = fmt >= F2 ? d.coded ^ pucch_seq(t, d.rnti, sf_idx, (uint32_t)g.cell_id) : 0u;
  const int      n0 = n_sf(fmt, 0, d.shortened), nre = (n0 + n_sf(fmt, 1, d.shortened)) * 12;
  const float    q  = 1.0f / sqrtf(2.0f);
  for (int i = lane; i < nre; i += 64) {
    const int s = i >= n0 * 12 ? 1 : 0, j = i - s * n0 * 12, m = j / 12, n = j % 12;
    cf32      dv;
    if (fmt >= F2) {
      const int k = s * 5 + m; // d((ns % 2) N_sf + m)
      dv          = make_float2(((cb >> (2 * k)) & 1u) ? -q : q, ((cb >> (2 * k + 1)) & 1u) ? -q : q);
    } else {
      dv = make_float2(d.d0[0], d.d0[1]);
    }
    gs[(size_t)(s * g.nsl + data_sym(fmt, m, g.cp_ext)) * W + prb[s] * 12 + n] = cmul(dv, base_signal(t, g, fmt, n_pucch, d.shortened, sf_idx, i));
  }
  const int nrs = n_rs(fmt, g.cp_ext);
  for (int i = lane; i < 2 * nrs * 12; i += 64) {
    const int s = i / (nrs * 12), m = (i / 12) % nrs, n = i % 12;
    cf32      v = dmrs_signal(t, g, fmt, n_pucch, sf_idx, i);
    if (m == 1) v = cmul(make_float2(d.z1[0], d.z1[1]), v);
    gs[(size_t)(s * g.nsl + dmrs_sym(fmt, m, g.cp_ext)) * W + prb[s] * 12 + n] = v;
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------

// M_basis_seq_pucch (uci.c:79-100, 36.212 Table 5.2.3.3-1)
const uint8_t RM_BASIS[20][13] = {
    {1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0}, {1, 1, 1, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0}, {1, 0, 0, 1, 0, 0, 1, 0, 1, 1, 1, 1, 1},
    {1, 0, 1, 1, 0, 0, 0, 0, 1, 0, 1, 1, 1}, {1, 1, 1, 1, 0, 0, 0, 1, 0, 0, 1, 1, 1}, {1, 1, 0, 0, 1, 0, 1, 1, 1, 0, 1, 1, 1},
    {1, 0, 1, 0, 1, 0, 1, 0, 1, 1, 1, 1, 1}, {1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 1, 1, 1}, {1, 1, 0, 1, 1, 0, 0, 1, 0, 1, 1, 1, 1},
    {1, 0, 1, 1, 1, 0, 1, 0, 0, 1, 1, 1, 1}, {1, 0, 1, 0, 0, 1, 1, 1, 0, 1, 1, 1, 1}, {1, 1, 1, 0, 0, 1, 1, 0, 1, 0, 1, 1, 1},
    {1, 0, 0, 1, 0, 1, 0, 1, 1, 1, 1, 1, 1}, {1, 1, 0, 1, 0, 1, 0, 1, 0, 1, 1, 1, 1}, {1, 0, 0, 0, 1, 1, 0, 1, 0, 0, 1, 0, 1},
    {1, 1, 0, 0, 1, 1, 1, 1, 0, 1, 1, 0, 1}, {1, 1, 1, 0, 1, 1, 1, 0, 0, 1, 0, 1, 1}, {1, 0, 0, 1, 1, 1, 0, 0, 1, 0, 0, 1, 1},
    {1, 1, 0, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {1, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0}};

bool cfg_ok(const srslte_hip_ul_ctrl_cfg_t* c)
{ // srslte_cell_isvalid's limits + srslte_pucch_cfg_isvalid (pucch.c:901-909); TDD refused
  return c && !c->tdd && c->nof_prb >= 6 && c->nof_prb <= 110 && c->cell_id < 504 && c->delta_pucch_shift > 0 && c->delta_pucch_shift < 4 &&
         c->N_cs < 8 && c->N_cs % c->delta_pucch_shift == 0 && c->n_rb_2 <= c->nof_prb;
}

void n_cs_cell(const srslte_hip_ul_ctrl_cfg_t* c, uint32_t out[20][7])
{ // srslte_pucch_n_cs_cell: srslte_sequence_LTE_pr(8 nsym 20, cell_id), 8 bits per (slot, symbol), LSB first
  const uint32_t       nsl = c->cp_ext ? 6 : 7;
  std::vector<uint8_t> s;
  lte_gold_sequence(c->cell_id, 8 * nsl * 20, s);
  for (uint32_t ns = 0; ns < 20; ns++)
    for (uint32_t l = 0; l < 7; l++) {
      out[ns][l] = 0;
      if (l < nsl)
        for (uint32_t i = 0; i < 8; i++) out[ns][l] += (uint32_t)s[8 * nsl * ns + 8 * l + i] << i;
    }
}

void build_tab(const srslte_hip_ul_ctrl_cfg_t* c, UlCtrlTab& t)
{
  memset(&t, 0, sizeof(t));
  std::vector<uint8_t> s;
  lte_gold_sequence(c->cell_id / 30, 160, s); // srslte_group_hopping_f_gh (phy_common.c:419-436)
  for (uint32_t ns = 0; ns < 20; ns++) {
    uint32_t f_gh = 0;
    for (int i = 0; i < 8; i++) f_gh += (uint32_t)s[8 * ns + i] << i;
    ul_r_uv_arg_1prb(((c->group_hopping_en ? f_gh : 0) + c->cell_id % 30) % 30, t.arg[ns]);
  }
  n_cs_cell(c, t.n_cs_cell);
  const float w1[3][3]    = {{0, 0, 0}, {0, 2 * M_PI / 3, 4 * M_PI / 3}, {0, 4 * M_PI / 3, 2 * M_PI / 3}};
  const float w1e[3][2]   = {{0, 0}, {0, M_PI}, {0, 0}};
  const float wn[2][3][4] = {{{0, 0, 0, 0}, {0, M_PI, 0, M_PI}, {0, M_PI, M_PI, 0}},
                             {{0, 0, 0, 0}, {0, 2 * M_PI / 3, 4 * M_PI / 3, 0}, {0, 4 * M_PI / 3, 2 * M_PI / 3, 0}}};
  memcpy(t.w_dmrs1, w1, sizeof(w1));
  memcpy(t.w_dmrs1e, w1e, sizeof(w1e));
  memcpy(t.w_n_oc, wn, sizeof(wn));
  for (int n = 0; n < 12; n++) t.alpha[n] = (float)(2 * M_PI * (n) / 12);
  t.s_ns = (float)(M_PI / 2);
  for (int i = 0; i < 20; i++)
    for (int n = 0; n < 13; n++) t.rm_row[i] |= (uint32_t)RM_BASIS[i][n] << (12 - n);
  auto word = [&](uint32_t c_init) {
    lte_gold_sequence(c_init, 20, s);
    uint32_t w = 0;
    for (int k = 0; k < 20; k++) w |= (uint32_t)s[k] << k;
    return w;
  };
  t.gold0 = word(0);
  for (int i = 0; i < 31; i++) t.gold_basis[i] = word(1u << i) ^ t.gold0;
}

// srslte_ue_ul_pucch_resource_selection (ue_ul.c:482-531, :823-900) for the formats here: uci = nullptr is the receiver's zero value.
// Returns false for a request no format fits
bool select_res(const srslte_hip_ul_ctrl_cfg_t* c, const srslte_hip_pucch_req_t& q, const srslte_hip_pucch_tx_t* uci, int sr_tti, int* fmt,
                uint32_t* n_pucch)
{
  const bool data_enable = q.cqi_len > 0 && !(!q.simul_cqi_ack && q.ack_len > 0); // the CQI drop on an ACK collision
  const bool sr_val      = uci && uci->sr;
  int        f           = F_ERR;
  if (!data_enable && q.ri_len == 0) {
    if (q.ack_len == 1) {
      f = F1A;
    } else if (q.ack_len == 2) {
      f = F1B;
    } else if (sr_tti || sr_val) {
      f = F1;
    }
  } else {
    if (q.ack_len == 0) {
      f = F2;
    } else if (q.ack_len == 1 && !c->cp_ext) {
      f = F2A;
    } else if (q.ack_len == 2) {
      f = F2B;
    } else if (q.ack_len == 1 && c->cp_ext) {
      f = F2B;
    }
  }
  if (f == F_ERR) return false;
  *fmt     = f;
  *n_pucch = (sr_tti || sr_val) ? q.n_pucch_sr : f < F2 ? q.ncce + c->N_pucch_1 : q.n_pucch_2;
  return true;
}

bool in_band(const srslte_hip_ul_ctrl_cfg_t* c, int fmt, uint32_t n_pucch)
{
  for (uint32_t s = 0; s < 2; s++)
    if (pucch_n_prb(fmt, n_pucch, s, c->nof_prb, c->delta_pucch_shift, c->N_cs, c->n_rb_2, c->cp_ext) >= c->nof_prb) return false;
  return true;
}

// get_user_sequence (pucch.c:214-236) has no format 2 scrambling sequence outside the C-RNTI range [SRSLTE_CRNTI_START, SRSLTE_CRNTI_END)
bool rnti_ok(int fmt, uint32_t rnti) { return fmt < F2 || (rnti >= 0x000Bu && rnti < 0xFFF3u); }

bool req_ok(const srslte_hip_pucch_req_t& q, uint32_t nof_sf)
{
  return q.sf < nof_sf && q.ack_len <= 2 && q.cqi_len <= 12 && q.ri_len <= 1 && !(q.cqi_len && q.ri_len);
}

} // namespace

struct srslte_hip_ul_ctrl {
  srslte_hip_ul_ctrl_cfg_t cfg;
  UlCtrlGeom               g;
  DevBuf<UlCtrlTab>        tab;
  DescStage                desc;
  DevBuf<cf32>             z;   // the receiver's alone, as llr
  DevBuf<short>            llr;
};

namespace {

srslte_hip_ul_ctrl* ul_ctrl_make(const srslte_hip_ul_ctrl_cfg_t* cfg, bool rx)
{
  if (!cfg_ok(cfg) || cfg->max_pucch == 0) {
    hip_log("[srslte_hip] ul_ctrl: invalid PUCCH configuration\n");
    return nullptr;
  }
  auto* q = new srslte_hip_ul_ctrl();
  q->cfg  = *cfg;
  UlCtrlTab t;
  build_tab(cfg, t);
  const size_t desc_bytes = (size_t)cfg->max_pucch * (rx ? sizeof(PucchDesc) : sizeof(PucchTxDesc));
  if (q->tab.upload(&t, 1) || q->desc.init(desc_bytes) || (rx && (q->z.alloc((size_t)MAX_RE * cfg->max_pucch) || q->llr.alloc((size_t)20 * cfg->max_pucch)))) {
    hip_log("[srslte_hip] ul_ctrl: device allocation failed\n");
    delete q;
    return nullptr;
  }
  UlCtrlGeom& g = q->g;
  g.nof_prb = (int)cfg->nof_prb, g.nsl = cfg->cp_ext ? 6 : 7, g.cp_ext = cfg->cp_ext ? 1 : 0;
  g.delta = (int)cfg->delta_pucch_shift, g.N_cs = (int)cfg->N_cs, g.n_rb_2 = (int)cfg->n_rb_2;
  g.th1 = cfg->threshold_format1, g.th1a = cfg->threshold_data_valid_format1a, g.th2 = cfg->threshold_data_valid_format2;
  g.cell_id = (int)cfg->cell_id;
  return q;
}

// the receiver's descriptors of a call (h_desc null: the checks alone)
int ul_ctrl_build(const srslte_hip_ul_ctrl* q, uint32_t nof_sf, const srslte_hip_pucch_req_t* reqs, uint32_t nof, PucchDesc* h_desc)
{
  if (!q || (nof && !reqs) || nof > q->cfg.max_pucch) return SRSLTE_ERROR_INVALID_INPUTS;
  for (uint32_t r = 0; r < nof; r++) {
    const srslte_hip_pucch_req_t& rq = reqs[r];
    int                           f0, f1 = -1;
    uint32_t                      n0, n1 = 0;
    if (!req_ok(rq, nof_sf) || !select_res(&q->cfg, rq, nullptr, rq.sr_tti, &f0, &n0) || !in_band(&q->cfg, f0, n0) || !rnti_ok(f0, rq.rnti)) {
      hip_log("[srslte_hip] ul_ctrl: request %u refused (sf %u of %u, ack %u, cqi %u, ri %u, sr %d)\n", r, rq.sf, nof_sf, rq.ack_len, rq.cqi_len,
              rq.ri_len, rq.sr_tti);
      return SRSLTE_ERROR_INVALID_INPUTS;
    }
    if (rq.sr_tti && rq.ack_len && f0 < F2) { // the retry on the HARQ-ACK resource (enb_ul.c:217-224)
      if (!select_res(&q->cfg, rq, nullptr, 0, &f1, &n1) || !in_band(&q->cfg, f1, n1)) {
        hip_log("[srslte_hip] ul_ctrl: request %u refused (HARQ-ACK resource %u outside the band)\n", r, n1);
        return SRSLTE_ERROR_INVALID_INPUTS;
      }
    }
    if (!h_desc) continue;
    PucchDesc& d = h_desc[r];
    d.sf = (int)rq.sf, d.shortened = rq.shortened ? 1 : 0, d.sr_tti = rq.sr_tti ? 1 : 0, d.ack_len = (int)rq.ack_len;
    d.data_enable = rq.cqi_len > 0 && !(!rq.simul_cqi_ack && rq.ack_len > 0);
    d.ri_len      = (int)rq.ri_len;
    d.uci_len     = rq.ri_len ? (int)rq.ri_len : (int)rq.cqi_len;
    d.format[0] = f0, d.n_pucch[0] = (int)n0, d.format[1] = f1, d.n_pucch[1] = (int)n1;
    d.rnti  = rq.rnti;
    d.noise = rq.noise_estimate;
  }
  return SRSLTE_SUCCESS;
}

// the transmitter's descriptors of a call (h_desc null: the checks alone)
int ul_ctrl_tx_build(const srslte_hip_ul_ctrl* q, uint32_t nof_sf, const srslte_hip_pucch_tx_t* tx, uint32_t nof, PucchTxDesc* h_desc)
{
  for (uint32_t r = 0; r < nof; r++) {
    const srslte_hip_pucch_tx_t&  u  = tx[r];
    const srslte_hip_pucch_req_t& rq = u.req;
    int                           f;
    uint32_t                      n;
    if (!req_ok(rq, nof_sf) || !select_res(&q->cfg, rq, &u, rq.sr_tti, &f, &n) || !in_band(&q->cfg, f, n) || !rnti_ok(f, rq.rnti)) {
      hip_log("[srslte_hip] ul_ctrl_tx: request %u refused (sf %u of %u, ack %u, cqi %u, ri %u)\n", r, rq.sf, nof_sf, rq.ack_len, rq.cqi_len, rq.ri_len);
      return SRSLTE_ERROR_INVALID_INPUTS;
    }
    if (!h_desc) continue;
    PucchTxDesc& d = h_desc[r];
    memset(&d, 0, sizeof(d));
    d.sf = (int)rq.sf, d.shortened = rq.shortened ? 1 : 0, d.format = f, d.n_pucch = (int)n, d.rnti = rq.rnti;
    d.d0[0] = 1.f, d.z1[0] = 1.f;
    const uint8_t a0 = u.ack[0], a1 = u.ack[1];
    if (f == F1A) { // uci_encode_format1a / 1b (pucch.c:190-212) of encode_bits' ack bits
      d.d0[0] = a0 ? -1.f : 1.f;
    } else if (f == F1B) {
      d.d0[0] = a0 == 0 ? (a1 == 0 ? 1.f : 0.f) : (a1 == 0 ? 0.f : -1.f);
      d.d0[1] = a0 == 0 ? (a1 == 0 ? 0.f : -1.f) : (a1 == 0 ? 1.f : 0.f);
    } else if (f >= F2) {
      // encode_bits (pucch.c:567-610): the RI alone, or the report; srslte_uci_encode_cqi_pucch (uci.c:136-151)
      uint8_t        bits[13] = {0};
      const uint32_t len      = rq.ri_len ? rq.ri_len : rq.cqi_len;
      if (rq.ri_len) {
        bits[0] = u.ri;
      } else {
        for (uint32_t i = 0; i < len; i++) bits[i] = u.cqi[i];
      }
      for (int i = 0; i < 20; i++) {
        uint32_t x = 0;
        for (uint32_t k = 0; k < len; k++) x += (uint32_t)bits[k] * RM_BASIS[i][k];
        d.coded |= (x % 2) << i;
      }
      if (f == F2A) { // srslte_pucch_format2ab_mod_bits (pucch.c:1061-1088) of pucch2_drs_bits = the ACK values
        d.z1[0] = a0 ? -1.f : 1.f;
      } else if (f == F2B) {
        d.z1[0] = a0 == 0 ? (a1 == 0 ? 1.f : 0.f) : (a1 == 0 ? 0.f : -1.f);
        d.z1[1] = a0 == 0 ? (a1 == 0 ? 0.f : -1.f) : (a1 == 0 ? 1.f : 0.f);
      }
    }
  }
  return SRSLTE_SUCCESS;
}

} // namespace

int ul_ctrl_check(const srslte_hip_ul_ctrl_t* q, uint32_t nof_sf, const srslte_hip_pucch_req_t* reqs, uint32_t nof)
{
  return ul_ctrl_build(q, nof_sf, reqs, nof, nullptr);
}

bool ul_ctrl_same_cell(const srslte_hip_ul_ctrl_t* q, uint32_t nof_prb, uint32_t cell_id, int cp_ext)
{
  return q && q->z.get() && q->cfg.nof_prb == nof_prb && q->cfg.cell_id == cell_id && (q->cfg.cp_ext ? 1 : 0) == (cp_ext ? 1 : 0);
}

extern "C" {

srslte_hip_ul_ctrl_t* srslte_hip_ul_ctrl_create(const srslte_hip_ul_ctrl_cfg_t* cfg) { return ul_ctrl_make(cfg, true); }
void                  srslte_hip_ul_ctrl_destroy(srslte_hip_ul_ctrl_t* q) { delete q; }

int srslte_hip_ul_ctrl_pucch_batch(srslte_hip_ul_ctrl_t* q, const void* d_grid, uint32_t tti0, uint32_t nof_sf, const srslte_hip_pucch_req_t* reqs,
                                   uint32_t nof, srslte_hip_pucch_res_t* d_res, void* stream)
{
  if (!q || !q->z.get() || !d_grid || (nof && !d_res)) return SRSLTE_ERROR_INVALID_INPUTS;
  if (int r = ul_ctrl_build(q, nof_sf, reqs, nof, nullptr)) return r;
  if (nof == 0) return SRSLTE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  PucchDesc*  h  = nullptr;
  if (int r = q->desc.begin(&h)) return r;
  ul_ctrl_build(q, nof_sf, reqs, nof, h);
  if (int r = q->desc.commit(sizeof(PucchDesc) * nof, st)) return r;
  hipLaunchKernelGGL(ul_pucch_rx_kernel, dim3(nof), dim3(64), 0, st, (const UlCtrlTab*)q->tab.get(), q->g, q->desc.dev<PucchDesc>(), (const cf32*)d_grid,
                     tti0, d_res, q->z.get(), q->llr.get());
  LAUNCH_CHECK();
  return SRSLTE_SUCCESS;
}

const void* srslte_hip_ul_ctrl_debug_buffer(const srslte_hip_ul_ctrl_t* q, int which)
{
  if (!q) return nullptr;
  return which == 0 ? (const void*)q->z.get() : which == 1 ? (const void*)q->llr.get() : nullptr;
}

srslte_hip_ul_ctrl_tx_t* srslte_hip_ul_ctrl_tx_create(const srslte_hip_ul_ctrl_cfg_t* cfg)
{
  return reinterpret_cast<srslte_hip_ul_ctrl_tx_t*>(ul_ctrl_make(cfg, false));
}
void srslte_hip_ul_ctrl_tx_destroy(srslte_hip_ul_ctrl_tx_t* q) { delete reinterpret_cast<srslte_hip_ul_ctrl*>(q); }

int srslte_hip_ul_ctrl_tx_put_pucch(srslte_hip_ul_ctrl_tx_t* qt, uint32_t tti0, uint32_t nof_sf, const srslte_hip_pucch_tx_t* tx, uint32_t nof,
                                    void* d_grid, void* stream)
{
  auto* q = reinterpret_cast<srslte_hip_ul_ctrl*>(qt);
  if (!q || !d_grid || (nof && !tx) || nof > q->cfg.max_pucch) return SRSLTE_ERROR_INVALID_INPUTS;
  if (int r = ul_ctrl_tx_build(q, nof_sf, tx, nof, nullptr)) return r;
  if (nof == 0) return SRSLTE_SUCCESS;
  hipStream_t  st = (hipStream_t)stream;
  PucchTxDesc* h  = nullptr;
  if (int r = q->desc.begin(&h)) return r;
  ul_ctrl_tx_build(q, nof_sf, tx, nof, h);
  if (int r = q->desc.commit(sizeof(PucchTxDesc) * nof, st)) return r;
  hipLaunchKernelGGL(ul_pucch_tx_kernel, dim3(nof), dim3(64), 0, st, (const UlCtrlTab*)q->tab.get(), q->g, q->desc.dev<PucchTxDesc>(), tti0, (cf32*)d_grid);
  LAUNCH_CHECK();
  return SRSLTE_SUCCESS;
}

int srslte_hip_pucch_n_cs_cell(const srslte_hip_ul_ctrl_cfg_t* cfg, uint32_t* out)
{
  if (!cfg || !out || cfg->nof_prb < 6 || cfg->nof_prb > 110 || cfg->cell_id >= 504) return SRSLTE_ERROR_INVALID_INPUTS;
  n_cs_cell(cfg, reinterpret_cast<uint32_t(*)[7]>(out));
  return SRSLTE_SUCCESS;
}

int srslte_hip_pucch_resource(const srslte_hip_ul_ctrl_cfg_t* cfg, const srslte_hip_pucch_tx_t* uci, const srslte_hip_pucch_req_t* req, uint32_t* res)
{
  if (!cfg_ok(cfg) || !req || !res || !req_ok(*req, 0xffffffffu)) return SRSLTE_ERROR_INVALID_INPUTS;
  int      f;
  uint32_t n;
  // a resource outside the band is refused as put_pucch and pucch_batch refuse it, not answered with a wrapped nof_prb - 1 - m / 2
  if (!select_res(cfg, *req, uci, req->sr_tti, &f, &n) || !in_band(cfg, f, n)) return SRSLTE_ERROR_INVALID_INPUTS;
  res[0] = (uint32_t)f, res[1] = n;
  for (uint32_t s = 0; s < 2; s++) res[2 + s] = pucch_n_prb(f, n, s, cfg->nof_prb, cfg->delta_pucch_shift, cfg->N_cs, cfg->n_rb_2, cfg->cp_ext);
  return SRSLTE_SUCCESS;
}

// srslte_refsignal_dmrs_pucch_gen on the host, with the device's integer state and float phase sum (libm cosf / sinf)
int srslte_hip_pucch_dmrs(const srslte_hip_ul_ctrl_cfg_t* cfg, uint32_t format, uint32_t n_pucch, uint32_t tti, const uint8_t* drs_bits, void* r_out)
{
  if (!cfg_ok(cfg) || !r_out || format > F2B) return SRSLTE_ERROR_INVALID_INPUTS;
  UlCtrlTab t;
  build_tab(cfg, t);
  const int      ext = cfg->cp_ext ? 1 : 0, fmt = (int)format, nrs = n_rs(fmt, ext);
  const uint32_t sf_idx = tti % 10;
  float          z1r = 1.f, z1i = 0.f;
  const uint8_t  b0 = drs_bits ? drs_bits[0] : 0, b1 = drs_bits ? drs_bits[1] : 0;
  if (fmt == F2A) z1r = b0 ? -1.f : 1.f;
  if (fmt == F2B) {
    z1r = b0 == 0 ? (b1 == 0 ? 1.f : 0.f) : (b1 == 0 ? 0.f : -1.f);
    z1i = b0 == 0 ? (b1 == 0 ? 0.f : -1.f) : (b1 == 0 ? 1.f : 0.f);
  }
  float* r = (float*)r_out;
  for (uint32_t s = 0; s < 2; s++) {
    const uint32_t ns = 2 * sf_idx + s;
    for (int m = 0; m < nrs; m++) {
      const uint32_t l = (uint32_t)dmrs_sym(fmt, m, ext);
      uint32_t       n_cs;
      float          w = 0.f;
      if (fmt < F2) {
        uint32_t n_oc, np;
        n_cs = alpha1(t.n_cs_cell, ext, cfg->delta_pucch_shift, cfg->N_cs, n_pucch, ns, l, &n_oc, &np);
        w    = ext ? t.w_dmrs1e[n_oc][m] : t.w_dmrs1[n_oc][m];
      } else {
        n_cs = alpha2(t.n_cs_cell, cfg->N_cs, cfg->n_rb_2, n_pucch, ns, l);
      }
      const float alpha = t.alpha[n_cs];
      for (int n = 0; n < 12; n++) {
        const float  x  = w + t.arg[ns][n] + alpha * (float)n;
        const float  cr = cosf(x), ci = sinf(x);
        const size_t o  = 2 * (((size_t)s * nrs + m) * 12 + n);
        r[o]            = m == 1 ? z1r * cr - z1i * ci : cr;
        r[o + 1]        = m == 1 ? z1r * ci + z1i * cr : ci;
      }
    }
  }
  return 12 * nrs;
}

} // extern "C"
