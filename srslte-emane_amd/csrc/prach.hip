// PRACH preamble formats 0-3 for gfx950, FDD (include/srslte_hip/phy_hip.h, "UL control: PRACH"): srslte_prach_gen and
// srslte_prach_detect_offset (lib/src/phy/phch/prach.c) for batches of preambles and occasions on the caller's stream.
//   prach_gen_kernel   one thread per n2 of a preamble: the N_ifft_prach = 12 M point inverse DFT (M = N_ifft_ul) of the 839 occupied bins
//                      split as n = n2 + M n1, k = k1 + 12 k2: for each k1 the M-point sum over the ~70 occupied k2, the twiddle W_N^-(k1 n2),
//                      then the 12-point sums give the 12 samples n2 + M n1, written to their CP and sequence positions
//   prach_fwd_kernel   one workgroup per (occasion, k1): Y[n2] = W_N^(k1 n2) sum_n1 x[n2 + M n1] W_12^(k1 n1) in LDS, then one wavefront per
//                      occupied bin k1 + 12 k2: sum_n2 Y[n2] W_M^(k2 n2) - only the 839 bins of the PRACH band of the forward transform
//   prach_corr_kernel  one workgroup per (occasion, root): product with conj(DFT of the root sequence), direct 839-point inverse DFT with the
//                      twiddles in LDS, |.|^2, the mean and the first maximum of each window
//   prach_pick_kernel  one workgroup per occasion: the peaks above detect_factor mean, placed in (root, window) order by a ballot prefix
// Tables (sequence DFTs, twiddles) are made on the host once per object, in double, and kept as float.
#include "cf32_dev.hpp"
#include "common.hpp"
#include "dev_buf.hpp"
#include "phy_hip_internal.hpp"
#include <math.h>
#include <string.h>
#include <vector>

namespace {

constexpr int NZC  = 839;  // N_zc of formats 0-3
constexpr int MMAX = 1536; // largest N_ifft_ul

// 36.211 Table 5.7.2-4: logical root sequence numbers 0-837 give the physical roots in pairs (u, 839 - u); the first of each pair, in order
const uint16_t ZC_ROOT_FIRST[419] = {
  129, 140, 120, 210, 168,  84, 105,  93,  70,  60,   2,   1,  56, 112, 148,  80,  42,  40,  35,  73,
  146,  31,  28,  30,  27,  29,  24,  48,  68,  74, 178, 136,  86,  78,  43,  39,  20,  21,  95, 202,
  190, 181, 137, 125, 151, 217, 128, 142, 122, 203, 118, 110,  89, 103,  61,  55,  15,  14,  12,  23,
   34,  37,  46, 207, 179, 145, 130, 223, 228, 227, 132, 133, 143, 135, 161, 201, 173, 106,  83,  91,
   66,  53,  10,   9,   7,   8,  16,  47,  64,  57, 104, 101, 108, 208, 184, 197, 191, 121, 141, 149,
  216, 218, 152, 144, 134, 138, 199, 162, 176, 119, 158, 164, 174, 171, 170,  87, 169,  88, 107,  81,
   82, 100,  98,  71,  59,  65,  50,  49,  26,  17,  13,   6,   5,  33,  51,  75,  99,  96,  97, 166,
  172, 175, 187, 163, 185, 200, 114, 189, 115, 194, 195, 192, 182, 157, 156, 211, 154, 123, 139, 212,
  153, 213, 215, 150, 225, 224, 221, 220, 127, 147, 124, 193, 205, 206, 116, 160, 186, 167,  79,  85,
   77,  92,  58,  62,  69,  54,  36,  32,  25,  18,  11,   4,   3,  19,  22,  41,  38,  44,  52,  45,
   63,  67,  72,  76,  94, 102,  90, 109, 165, 111, 209, 204, 117, 188, 159, 198, 113, 183, 180, 177,
  196, 155, 214, 126, 131, 219, 222, 226, 230, 232, 262, 252, 418, 416, 413, 411, 376, 395, 283, 285,
  379, 390, 363, 384, 388, 386, 361, 387, 360, 310, 354, 328, 315, 337, 349, 335, 324, 323, 320, 334,
  359, 295, 385, 292, 291, 381, 399, 380, 397, 369, 377, 410, 407, 281, 414, 247, 277, 271, 272, 264,
  259, 237, 239, 244, 243, 275, 278, 250, 246, 417, 248, 394, 393, 370, 365, 300, 299, 364, 362, 298,
  312, 313, 314, 353, 352, 343, 327, 350, 326, 319, 332, 333, 348, 347, 322, 330, 338, 341, 340, 342,
  301, 366, 401, 371, 408, 375, 249, 269, 238, 234, 257, 273, 255, 254, 245, 251, 412, 372, 282, 403,
  396, 392, 391, 382, 389, 294, 297, 311, 344, 345, 318, 331, 325, 321, 346, 339, 351, 306, 289, 400,
  378, 374, 415, 270, 241, 231, 260, 268, 276, 409, 398, 290, 304, 308, 358, 316, 293, 288, 284, 368,
  253, 256, 263, 242, 274, 402, 383, 357, 329, 317, 307, 286, 287, 266, 261, 236, 303, 356, 355, 405,
  404, 406, 235, 267, 302, 309, 265, 233, 367, 296, 336, 305, 373, 280, 279, 419, 240, 258, 229};
uint32_t zc_root(uint32_t logical)
{
  const uint32_t i = logical % 838, u = ZC_ROOT_FIRST[i / 2];
  return (i & 1) ? NZC - u : u;
}
// 36.211 Table 5.7.2-2, unrestricted set: N_cs of zeroCorrelationZoneConfig 0-15
const uint32_t NCS_UNRESTRICTED[16] = {0, 13, 15, 18, 22, 26, 32, 38, 46, 59, 76, 93, 119, 167, 279, 419};
// 36.211 Table 5.7.1-1: T_CP and T_SEQ of preamble formats 0-3 in units of T_s = 1 / (15000 2048) s
const uint32_t T_CP[4]  = {3168, 21024, 6240, 21024};
const uint32_t T_SEQ[4] = {24576, 24576, 2 * 24576, 2 * 24576};
// 36.211 Table 5.7.1-2 (FDD), by config_idx % 16: the subframes (bit s) and whether only even system frames carry them. 14 is every
// subframe of every frame; 30, 46 and 62 are not available in the table and srslte's table gives them no subframe (never an opportunity)
const uint16_t FDD_SF_MASK[16] = {1 << 1, 1 << 4, 1 << 7, 1 << 1, 1 << 4, 1 << 7, (1 << 1) | (1 << 6), (1 << 2) | (1 << 7), (1 << 3) | (1 << 8),
                                  (1 << 1) | (1 << 4) | (1 << 7), (1 << 2) | (1 << 5) | (1 << 8), (1 << 3) | (1 << 6) | (1 << 9), 0x155, 0x2aa, 0, 1 << 9};
bool fdd_even_sfn_only(uint32_t config_idx) { return config_idx % 16 < 3 || config_idx % 16 == 15; }

// srslte_nof_prb of srslte_symbol_sz (phy_common.c, the non-standard sizes lte_symbol_sz gives)
int nof_prb_of_symbol_sz(int N)
{
  switch (N) {
    case 128: return 6;
    case 256: return 15;
    case 384: return 25;
    case 768: return 50;
    case 1024: return 75;
    case 1536: return 100;
  }
  return -1;
}

struct PrachGeom {
  int   N, M, N_cp, L;        // L = N_cp + N_seq
  float norm;                 // 1 / sqrt(N) of the generator's transform
  int   N_cs, n_wins, winsize, nof_roots, max_det;
  float factor;
};
struct PrachGenDesc {
  uint32_t seq, kb; // kb: the transform index of bin begin, (begin + N / 2) % N
};
struct PrachOccDesc {
  uint64_t sample;
  uint32_t kb, reserved;
};
struct PrachPeak {
  float    peak;
  uint32_t off;
};

// the first occupied bin t of residue k1 (mod 12) and its k2: bins t = t0 + 12 j have transform index kb + t (mod N), = k1 + 12 (k2_0 + j) mod N
__device__ __forceinline__ int first_bin(int k1, uint32_t kb) { return (k1 - (int)(kb % 12u) + 12) % 12; }

// tw[k] = exp(-2 pi i k / N); W_M^x = tw[12 x], W_12^x = tw[M x]
__global__ __launch_bounds__(256) void prach_gen_kernel(PrachGeom g, const cf32* __restrict__ dft, const cf32* __restrict__ tw,
                                                        const PrachGenDesc* __restrict__ desc, cf32* __restrict__ out)
{
  __shared__ cf32 s_x[NZC];
  __shared__ cf32 s_tw[MMAX];
  const PrachGenDesc d = desc[blockIdx.y];
  const int          M = g.M, N = g.N;
  for (int i = threadIdx.x; i < NZC; i += blockDim.x) s_x[i] = dft[(size_t)d.seq * NZC + i];
  for (int i = threadIdx.x; i < M; i += blockDim.x) s_tw[i] = tw[12 * i];
  __syncthreads();
  const int n2 = blockIdx.x * blockDim.x + threadIdx.x;
  if (n2 >= M) return;
  cf32 z[12];
#pragma unroll
  for (int k1 = 0; k1 < 12; k1++) {
    int t = first_bin(k1, d.kb);
    int k = (int)d.kb + t;
    if (k >= N) k -= N;
    int  p   = (int)((k / 12) * n2 % M); // (k2 n2) mod M; k2 grows by one per bin, also across the wrap of k at N
    cf32 acc = make_float2(0.f, 0.f);
    for (; t < NZC; t += 12) {
      const cf32 v = cmulconj(s_x[t], s_tw[p]);
      acc.x += v.x, acc.y += v.y;
      p += n2;
      if (p >= M) p -= M;
    }
    z[k1] = cmulconj(acc, tw[k1 * n2]); // W_N^-(k1 n2); k1 n2 < 12 M = N
  }
  cf32* o = out + (size_t)blockIdx.y * g.L;
#pragma unroll
  for (int n1 = 0; n1 < 12; n1++) {
    cf32 s = make_float2(0.f, 0.f);
#pragma unroll
    for (int k1 = 0; k1 < 12; k1++) {
      const cf32 v = cmulconj(z[k1], tw[((k1 * n1) % 12) * M]);
      s.x += v.x, s.y += v.y;
    }
    s.x *= g.norm, s.y *= g.norm;
    const int n = n2 + M * n1;
    for (int pos = g.N_cp + n; pos < g.L; pos += N) o[pos] = s; // the sequence, repeated modulo N (formats 2, 3)
    if (n >= N - g.N_cp) o[n - (N - g.N_cp)] = s;               // the CP: the last N_cp samples
  }
}

__global__ __launch_bounds__(256) void prach_fwd_kernel(PrachGeom g, const cf32* __restrict__ sig, const cf32* __restrict__ tw,
                                                        const PrachOccDesc* __restrict__ desc, cf32* __restrict__ bins)
{
  __shared__ cf32 s_y[MMAX];
  __shared__ cf32 s_tw[MMAX];
  const int          k1 = blockIdx.x, M = g.M, N = g.N;
  const PrachOccDesc d  = desc[blockIdx.y];
  const cf32*        x  = sig + d.sample;
  for (int n2 = threadIdx.x; n2 < M; n2 += blockDim.x) {
    cf32 s = make_float2(0.f, 0.f);
    for (int n1 = 0; n1 < 12; n1++) {
      const cf32 v = cmul(x[n2 + M * n1], tw[((k1 * n1) % 12) * M]);
      s.x += v.x, s.y += v.y;
    }
    s_y[n2]  = cmul(s, tw[k1 * n2]);
    s_tw[n2] = tw[12 * n2];
  }
  __syncthreads();
  const int t0 = first_bin(k1, d.kb), nb = (NZC - t0 + 11) / 12;
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64, nwave = blockDim.x / 64;
  for (int j = wave; j < nb; j += nwave) {
    const int t = t0 + 12 * j;
    int       k = (int)d.kb + t;
    if (k >= N) k -= N;
    const int k2   = k / 12;
    int       p    = k2 * lane % M;
    const int step = k2 * 64 % M;
    cf32      acc  = make_float2(0.f, 0.f);
    for (int n2 = lane; n2 < M; n2 += 64) {
      const cf32 v = cmul(s_y[n2], s_tw[p]);
      acc.x += v.x, acc.y += v.y;
      p += step;
      if (p >= M) p -= M;
    }
    acc.x = wave_sum(acc.x), acc.y = wave_sum(acc.y);
    if (lane == 0) bins[(size_t)blockIdx.y * NZC + t] = acc;
  }
}

__global__ __launch_bounds__(256) void prach_corr_kernel(PrachGeom g, const cf32* __restrict__ bins, const cf32* __restrict__ dft,
                                                         const cf32* __restrict__ tw839, const uint32_t* __restrict__ root_seq,
                                                         PrachPeak* __restrict__ peaks, float* __restrict__ means)
{
  __shared__ cf32  s_p[NZC];
  __shared__ cf32  s_w[NZC];
  __shared__ float s_c[NZC];
  __shared__ float s_red[4];
  const int   r = blockIdx.x, o = blockIdx.y;
  const cf32* b = bins + (size_t)o * NZC;
  const cf32* q = dft + (size_t)root_seq[r] * NZC;
  for (int i = threadIdx.x; i < NZC; i += blockDim.x) {
    s_p[i] = cmulconj(b[i], q[i]);
    s_w[i] = tw839[i];
  }
  __syncthreads();
  float part = 0.f;
  for (int n = threadIdx.x; n < NZC; n += blockDim.x) {
    cf32 acc = make_float2(0.f, 0.f);
    int  p   = 0;
    for (int k = 0; k < NZC; k++) {
      const cf32 v = cmulconj(s_p[k], s_w[p]); // backward: exp(+2 pi i n k / 839)
      acc.x += v.x, acc.y += v.y;
      p += n;
      if (p >= NZC) p -= NZC;
    }
    const float c = acc.x * acc.x + acc.y * acc.y;
    s_c[n] = c;
    part += c;
  }
  part = wave_sum(part);
  if (threadIdx.x % 64 == 0) s_red[threadIdx.x / 64] = part;
  __syncthreads();
  const float mean = (s_red[0] + s_red[1] + s_red[2] + s_red[3]) / (float)NZC;
  PrachPeak*  pk   = peaks + ((size_t)o * g.nof_roots + r) * g.n_wins;
  for (int j = threadIdx.x; j < g.n_wins; j += blockDim.x) {
    const int start = (NZC - j * g.N_cs) % NZC;
    PrachPeak m     = {0.f, 0u};
    for (int k = 0; k < g.winsize; k++)
      if (s_c[start + k] > m.peak) m.peak = s_c[start + k], m.off = (uint32_t)k;
    pk[j] = m;
  }
  if (threadIdx.x == 0) means[(size_t)o * g.nof_roots + r] = mean;
}

__global__ __launch_bounds__(128) void prach_pick_kernel(PrachGeom g, const PrachPeak* __restrict__ peaks, const float* __restrict__ means,
                                                         uint32_t* __restrict__ nof_det, uint32_t* __restrict__ indices,
                                                         float* __restrict__ t_offsets, float* __restrict__ peak_to_avg)
{
  __shared__ uint32_t s_cnt[2];
  const int o = blockIdx.y, lane = threadIdx.x % 64, wave = threadIdx.x / 64;
  uint32_t  placed = 0;
  for (int base = 0; base < g.max_det; base += 128) {
    const int i    = base + (int)threadIdx.x;
    bool      hit  = false;
    PrachPeak pk   = {0.f, 0u};
    float     mean = 0.f;
    if (i < g.max_det) {
      const int r = i / g.n_wins;
      pk          = peaks[(size_t)o * g.nof_roots * g.n_wins + i];
      mean        = means[(size_t)o * g.nof_roots + r];
      hit         = pk.peak > g.factor * mean;
    }
    const uint64_t ball = __ballot(hit);
    if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(ball);
    __syncthreads();
    const uint32_t pos = placed + (wave ? s_cnt[0] : 0u) + (uint32_t)__popcll(ball & ((1ull << lane) - 1ull));
    if (hit) {
      const size_t w = (size_t)o * g.max_det + pos;
      indices[w]     = (uint32_t)i;
      if (peak_to_avg) peak_to_avg[w] = pk.peak / mean;
      if (t_offsets) {
        float c = 1.8f;
        if (pk.off > 30) c = 1.9f;
        if (pk.off > 250) c = 1.91f;
        t_offsets[w] = c * (float)pk.off / (float)(1250u * NZC);
      }
    }
    placed += s_cnt[0] + s_cnt[1];
    __syncthreads();
  }
  if (threadIdx.x == 0) nof_det[o] = placed;
}

// the numerology of a configuration (srslte_prach_set_cell_ for FDD formats 0-3 and srslte_prach_gen_seqs' root count); false: refused
bool prach_numerology(const srslte_hip_prach_cfg_t* c, srslte_hip_prach_info_t* in)
{
  if (!c || c->hs_flag || c->tdd || c->config_idx >= 64 || c->root_seq_idx >= 838 || c->zero_corr_zone >= 16 || c->nof_prb < 6 ||
      c->nof_prb > 110 || !(c->detect_factor >= 0.f) || !isfinite(c->detect_factor))
    return false;
  memset(in, 0, sizeof(*in));
  const uint32_t f = c->config_idx / 16, Nul = (uint32_t)lte_symbol_sz((int)c->nof_prb);
  in->format       = f;
  in->N_zc         = NZC;
  in->N_cs         = NCS_UNRESTRICTED[c->zero_corr_zone];
  in->N_ifft_ul    = Nul;
  in->N_ifft_prach = Nul * 12; // 15000 / 1250
  in->N_seq        = T_SEQ[f] * Nul / 2048;
  in->N_cp         = T_CP[f] * Nul / 2048;
  in->n_wins       = in->N_cs ? NZC / in->N_cs : 1;
  const uint32_t per_root = in->n_wins; // v_max + 1 of srslte_prach_gen_seqs
  in->nof_roots           = (64 + per_root - 1) / per_root;
  for (uint32_t r = 0; r < in->nof_roots; r++) in->root_seqs_idx[r] = r * per_root;
  in->max_det = in->nof_roots * in->n_wins;
  in->nof_sf  = (uint32_t)ceil((double)(T_SEQ[f] + T_CP[f]) / 30720.0); // T_tot 1000, T_s = 1 / 30720 ms
  return true;
}

// begin of srslte_prach_gen / _detect_offset as the transform index of the mirrored bin: (begin + N / 2) % N
uint32_t prach_kb(const srslte_hip_prach_info_t& in, uint32_t freq_offset)
{
  const uint32_t N_rb_ul = (uint32_t)nof_prb_of_symbol_sz((int)in.N_ifft_ul);
  const uint32_t k_0     = freq_offset * 12 - N_rb_ul * 12 / 2 + in.N_ifft_ul / 2;
  const uint32_t begin   = 7 + 12 * k_0 + 12 / 2; // PHI + K k_0 + K / 2
  return (begin + in.N_ifft_prach / 2) % in.N_ifft_prach;
}

int gen_check(const srslte_hip_prach_cfg_t* c, const srslte_hip_prach_info_t& in, const srslte_hip_prach_tx_t* list, uint32_t n)
{
  if ((n && !list) || n > c->max_preambles) return SRSLTE_ERROR_INVALID_INPUTS;
  for (uint32_t i = 0; i < n; i++) {
    if (list[i].seq_index >= 64 || 6 + list[i].freq_offset > c->nof_prb) {
      hip_log("[srslte_hip] prach: preamble %u refused (seq_index %u, freq_offset %u, %u PRB)\n", i, list[i].seq_index, list[i].freq_offset,
              c->nof_prb);
      return SRSLTE_ERROR_INVALID_INPUTS;
    }
  }
  (void)in;
  return SRSLTE_SUCCESS;
}

int detect_check(const srslte_hip_prach_cfg_t* c, const srslte_hip_prach_info_t& in, size_t sig_len, const srslte_hip_prach_occasion_t* occ,
                 uint32_t n)
{
  if ((n && !occ) || n > c->max_occasions) return SRSLTE_ERROR_INVALID_INPUTS;
  for (uint32_t i = 0; i < n; i++) {
    if (6 + occ[i].freq_offset > c->nof_prb || occ[i].sample > sig_len || sig_len - occ[i].sample < in.N_ifft_prach) {
      hip_log("[srslte_hip] prach: occasion %u refused (sample %llu, freq_offset %u, signal of %zu samples)\n", i,
              (unsigned long long)occ[i].sample, occ[i].freq_offset, sig_len);
      return SRSLTE_ERROR_INVALID_INPUTS;
    }
  }
  return SRSLTE_SUCCESS;
}

// the 64 sequences' DFTs (srslte_prach_gen_seqs + srslte_dft_run of the forward 839-point plan with norm: 1 / sqrt(839)), in double
void prach_dft_seqs(const srslte_hip_prach_cfg_t* c, const srslte_hip_prach_info_t& in, std::vector<cf32>& out)
{
  std::vector<double> cs(NZC), sn(NZC);
  for (int k = 0; k < NZC; k++) cs[k] = cos(2 * M_PI * k / NZC), sn[k] = -sin(2 * M_PI * k / NZC);
  out.assign((size_t)64 * NZC, make_float2(0.f, 0.f));
  std::vector<double> xr(NZC), xi(NZC);
  for (uint32_t i = 0; i < 64; i++) {
    const uint32_t r = i / in.n_wins, v = i % in.n_wins, C_v = v * in.N_cs, u = zc_root(c->root_seq_idx + r);
    for (int j = 0; j < NZC; j++) { // x_u((j + C_v) mod N_zc), rounded to float as the reference's cf_t table holds it
      const uint32_t m     = (j + C_v) % NZC;
      const double   phase = -M_PI * u * m * (m + 1) / NZC;
      xr[j] = (float)cos(phase), xi[j] = (float)sin(phase);
    }
    for (int k = 0; k < NZC; k++) {
      double   ar = 0, ai = 0;
      uint32_t p  = 0;
      for (int j = 0; j < NZC; j++) {
        ar += xr[j] * cs[p] - xi[j] * sn[p];
        ai += xr[j] * sn[p] + xi[j] * cs[p];
        p += k;
        if (p >= (uint32_t)NZC) p -= NZC;
      }
      out[(size_t)i * NZC + k] = make_float2((float)(ar / sqrt((double)NZC)), (float)(ai / sqrt((double)NZC)));
    }
  }
}

} // namespace

struct srslte_hip_prach {
  srslte_hip_prach_cfg_t  cfg;
  srslte_hip_prach_info_t info;
  PrachGeom               g;
  DevBuf<cf32>            dft, tw, tw839, bins;
  DevBuf<uint32_t>        roots;
  DevBuf<PrachPeak>       peaks;
  DevBuf<float>           means;
  DescStage               gen, occ; // the generator's and the detector's descriptors
};

extern "C" {

int srslte_hip_prach_cfg_info(const srslte_hip_prach_cfg_t* cfg, srslte_hip_prach_info_t* info)
{
  srslte_hip_prach_info_t in;
  if (!info || !prach_numerology(cfg, &in)) return SRSLTE_ERROR_INVALID_INPUTS;
  *info = in;
  return SRSLTE_SUCCESS;
}

srslte_hip_prach_t* srslte_hip_prach_create(const srslte_hip_prach_cfg_t* cfg)
{
  srslte_hip_prach_info_t in;
  if (!prach_numerology(cfg, &in)) {
    hip_log("[srslte_hip] prach: invalid PRACH configuration (high-speed sets, TDD and format 4 are not supported)\n");
    return nullptr;
  }
  auto* q = new srslte_hip_prach();
  q->cfg  = *cfg;
  q->info = in;
  if (q->cfg.detect_factor == 0.f) q->cfg.detect_factor = 18.f; // PRACH_DETECT_FACTOR
  PrachGeom& g = q->g;
  g.N = (int)in.N_ifft_prach, g.M = (int)in.N_ifft_ul, g.N_cp = (int)in.N_cp, g.L = (int)(in.N_cp + in.N_seq);
  g.norm      = 1.f / sqrtf((float)in.N_ifft_prach); // srslte_dft_run_c: 1.0 / sqrtf(size)
  g.N_cs      = (int)in.N_cs, g.n_wins = (int)in.n_wins, g.winsize = in.N_cs ? (int)in.N_cs : NZC;
  g.nof_roots = (int)in.nof_roots, g.max_det = (int)in.max_det;
  g.factor    = q->cfg.detect_factor;

  std::vector<cf32> dft, tw(in.N_ifft_prach), tw839(NZC);
  prach_dft_seqs(cfg, in, dft);
  for (uint32_t k = 0; k < in.N_ifft_prach; k++)
    tw[k] = make_float2((float)cos(2 * M_PI * k / in.N_ifft_prach), (float)-sin(2 * M_PI * k / in.N_ifft_prach));
  for (int k = 0; k < NZC; k++) tw839[k] = make_float2((float)cos(2 * M_PI * k / NZC), (float)-sin(2 * M_PI * k / NZC));
  std::vector<uint32_t> roots(in.root_seqs_idx, in.root_seqs_idx + in.nof_roots);
  const size_t          n_occ = cfg->max_occasions ? cfg->max_occasions : 1, n_pre = cfg->max_preambles ? cfg->max_preambles : 1;
  if (q->dft.upload(dft) || q->tw.upload(tw) || q->tw839.upload(tw839) || q->roots.upload(roots) || q->bins.alloc(NZC * n_occ) ||
      q->peaks.alloc(in.max_det * n_occ) || q->means.alloc(in.nof_roots * n_occ) || q->gen.init(sizeof(PrachGenDesc) * n_pre) ||
      q->occ.init(sizeof(PrachOccDesc) * n_occ)) {
    hip_log("[srslte_hip] prach: device allocation failed\n");
    delete q;
    return nullptr;
  }
  return q;
}

void srslte_hip_prach_destroy(srslte_hip_prach_t* q) { delete q; }

int srslte_hip_prach_info(const srslte_hip_prach_t* q, srslte_hip_prach_info_t* info)
{
  if (!q || !info) return SRSLTE_ERROR_INVALID_INPUTS;
  *info = q->info;
  return SRSLTE_SUCCESS;
}

int srslte_hip_prach_gen_batch(srslte_hip_prach_t* q, const srslte_hip_prach_tx_t* list, uint32_t n, void* d_out, void* stream)
{
  if (!q || (n && !d_out)) return SRSLTE_ERROR_INVALID_INPUTS;
  if (int r = gen_check(&q->cfg, q->info, list, n)) return r;
  if (n == 0) return SRSLTE_SUCCESS;
  hipStream_t   st = (hipStream_t)stream;
  PrachGenDesc* h  = nullptr;
  if (int r = q->gen.begin(&h)) return r;
  for (uint32_t i = 0; i < n; i++) h[i] = {list[i].seq_index, prach_kb(q->info, list[i].freq_offset)};
  if (int r = q->gen.commit(sizeof(PrachGenDesc) * n, st)) return r;
  hipLaunchKernelGGL(prach_gen_kernel, dim3(ceil_div(q->g.M, 256), n), dim3(256), 0, st, q->g, (const cf32*)q->dft.get(), (const cf32*)q->tw.get(),
                     q->gen.dev<PrachGenDesc>(), (cf32*)d_out);
  LAUNCH_CHECK();
  return SRSLTE_SUCCESS;
}

int srslte_hip_prach_detect_batch(srslte_hip_prach_t* q, const void* d_signal, size_t sig_len, const srslte_hip_prach_occasion_t* occ, uint32_t n,
                                  uint32_t* d_nof_det, uint32_t* d_indices, float* d_t_offsets, float* d_peak_to_avg, void* stream)
{
  if (!q || (n && (!d_signal || !d_nof_det || !d_indices))) return SRSLTE_ERROR_INVALID_INPUTS;
  if (int r = detect_check(&q->cfg, q->info, sig_len, occ, n)) return r;
  if (n == 0) return SRSLTE_SUCCESS;
  hipStream_t   st = (hipStream_t)stream;
  PrachOccDesc* h  = nullptr;
  if (int r = q->occ.begin(&h)) return r;
  for (uint32_t i = 0; i < n; i++) h[i] = {occ[i].sample, prach_kb(q->info, occ[i].freq_offset), 0u};
  if (int r = q->occ.commit(sizeof(PrachOccDesc) * n, st)) return r;
  hipLaunchKernelGGL(prach_fwd_kernel, dim3(12, n), dim3(256), 0, st, q->g, (const cf32*)d_signal, (const cf32*)q->tw.get(), q->occ.dev<PrachOccDesc>(),
                     q->bins.get());
  LAUNCH_CHECK();
  hipLaunchKernelGGL(prach_corr_kernel, dim3(q->info.nof_roots, n), dim3(256), 0, st, q->g, (const cf32*)q->bins.get(), (const cf32*)q->dft.get(),
                     (const cf32*)q->tw839.get(), (const uint32_t*)q->roots.get(), q->peaks.get(), q->means.get());
  LAUNCH_CHECK();
  hipLaunchKernelGGL(prach_pick_kernel, dim3(1, n), dim3(128), 0, st, q->g, (const PrachPeak*)q->peaks.get(), (const float*)q->means.get(), d_nof_det,
                     d_indices, d_t_offsets, d_peak_to_avg);
  LAUNCH_CHECK();
  return SRSLTE_SUCCESS;
}

int srslte_hip_prach_gen_check(const srslte_hip_prach_cfg_t* cfg, const srslte_hip_prach_tx_t* list, uint32_t n)
{
  srslte_hip_prach_info_t in;
  if (!prach_numerology(cfg, &in)) return SRSLTE_ERROR_INVALID_INPUTS;
  return gen_check(cfg, in, list, n);
}

int srslte_hip_prach_detect_check(const srslte_hip_prach_cfg_t* cfg, size_t sig_len, const srslte_hip_prach_occasion_t* occ, uint32_t n)
{
  srslte_hip_prach_info_t in;
  if (!prach_numerology(cfg, &in)) return SRSLTE_ERROR_INVALID_INPUTS;
  return detect_check(cfg, in, sig_len, occ, n);
}

int srslte_hip_prach_tti_opportunity_fdd(uint32_t config_idx, uint32_t tti, int allowed_subframe)
{
  if (config_idx >= 64) return 0;
  if (config_idx == 14) return 1; // the one configuration with an opportunity in every subframe
  if (fdd_even_sfn_only(config_idx) && (tti / 10) % 2 != 0) return 0;
  const uint32_t sf = tti % 10;
  return (FDD_SF_MASK[config_idx % 16] >> sf & 1u) && (allowed_subframe == -1 || (int)sf == allowed_subframe) ? 1 : 0;
}

int srslte_hip_prach_preamble_format(uint32_t config_idx) { return config_idx < 64 ? (int)(config_idx / 16) : SRSLTE_ERROR_INVALID_INPUTS; }

} // extern "C"
