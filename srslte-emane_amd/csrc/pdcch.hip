// DL control region receive for gfx950 (include/srslte_hip/phy_hip.h, "DL control region receive"): PCFICH -> CFI -> PDCCH LLRs ->
// blind search -> DL DCI messages for a batch of subframes, three launches on the caller's stream:
//   dl_ctrl_llr_kernel     one workgroup per subframe: srslte_pcfich_decode (pcfich.c:160-227), srslte_pdcch_extract_llr for the CFI it
//                          decided or was given (pdcch.c:424-488) into an LLR row, and the subframe's candidate list in search order
//                          (ue_dl.c:534-618 with srslte_pdcch_ue_locations_ncce / srslte_pdcch_common_locations_ncce, pdcch.c:228-314)
//   dl_ctrl_dci_kernel     one wavefront per (subframe, candidate): the skip rule and srslte_pdcch_dci_decode (pdcch.c:327-396) - rate
//                          de-matching with the reference's combining order, the Viterbi decoder of viterbi_dev.hpp, CRC-16
//   dl_ctrl_select_kernel  one lane per subframe: dci_blind_search's first hit (ue_dl.c:422-478)
// The REG lists (regs.c), the DCI sizes (dci.c:93-360) and the scrambling sequences are built on the host when the object is made.
#include "common.hpp"
#include "ctrl_host.hpp"
#include "ctrl_rx_dev.hpp"
#include "demod_dev.hpp"
#include "dev_buf.hpp"
#include "phy_hip_internal.hpp"
#include "viterbi_dev.hpp"
#include <math.h>
#include <string.h>
#include <vector>

namespace {

constexpr int      MAX_CAND = SRSLTE_HIP_DL_CTRL_MAX_CAND;
constexpr int      REQ_CHUNK = 128;        // subframes per launch of dl_ctrl_llr_kernel (their requests travel as a kernel argument)
constexpr int      DCI_CHUNK = 32768;      // subframes per launch of dl_ctrl_dci_kernel (gridDim.y)
constexpr int      MAX_F     = 128;        // nof_bits + 16 of the largest DCI decoded (rm_conv.c's limit is 32 rows; DCIs here stay below 80)
constexpr uint16_t SIRNTI = 0xFFFF, PRNTI = 0xFFFE, RARNTI_START = 0x0001, RARNTI_END = 0x000A; // phy_common.h:71-80
enum { F0 = 0, F1, F1A, F1C, F1B, F1D, F2, F2A, F2B, NOF_FORMATS };      // srslte_dci_format_t (phy_common.h:249-265)

__constant__ uint8_t UE_FORMATS[4][2] = {{F1A, F1}, {F1A, F1}, {F1A, F2A}, {F1A, F2}}; // ue_dci_formats, ue_dl.c:31-39

// srslte_pdcch_ue_locations_ncce (pdcch.c:228-275): Y_k of the subframe, aggregation levels 8 .. 1, candidates of 36.213 Table 9.1.1-1
__host__ __device__ inline uint32_t ue_locations(uint32_t nof_cce, uint32_t* loc, uint32_t max_candidates, uint32_t sf_idx, uint16_t rnti)
{
  const uint32_t nof_candidates[4] = {6, 6, 2, 2};
  uint32_t       Yk = rnti, k = 0;
  for (uint32_t m = 0; m < sf_idx + 1; m++) Yk = (39827 * Yk) % 65537;
  for (int l = 3; l >= 0; l--) {
    const uint32_t L = 1u << l;
    for (uint32_t i = 0; i < nof_candidates[l]; i++) {
      if (nof_cce >= L) {
        const uint32_t ncce = L * ((Yk + i) % (nof_cce / L));
        if (k < max_candidates && ncce + L <= nof_cce) {
          loc[2 * k] = l, loc[2 * k + 1] = ncce;
          k++;
        }
      }
    }
  }
  return k;
}

// srslte_pdcch_common_locations_ncce (pdcch.c:291-314)
__host__ __device__ inline uint32_t common_locations(uint32_t nof_cce, uint32_t* loc, uint32_t max_candidates)
{
  uint32_t k = 0;
  for (uint32_t l = 3; l > 1; l--) {
    const uint32_t L = 1u << l;
    for (uint32_t i = 0; i < (nof_cce < 16 ? nof_cce : 16) / L; i++) {
      const uint32_t ncce = L * i;
      if (k < max_candidates && ncce + L <= nof_cce) {
        loc[2 * k] = l, loc[2 * k + 1] = ncce;
        k++;
      }
    }
  }
  return k;
}

struct CtrlGeom {
  const uint32_t* re;        // [16 PCFICH][n[0]][n[1]][n[2]] RE indices into one [nsym][12 prb] grid
  const uint32_t* scr_pcfich; // [10] words: the 32 bits of srslte_sequence_pcfich of each subframe, bit i = bit i
  const uint32_t* scr_pdcch;  // [10][scr_words]
  int             scr_words;
  int             off[CTRL_MAX_VAR][3], n[CTRL_MAX_VAR][3]; // PDCCH REs of CFI 1-3 (36 NOF_CCE) of each REG variant (ctrl_host.hpp)
  uint8_t         var[10];      // the variant of subframe sf_idx; CTRL_SF_UL: an uplink subframe of a TDD cell. FDD: all 0
  int             tdd;
  int             nof_ports, nof_rx, grid_len;
  int             llr_stride;
  uint32_t        dci_bits[NOF_FORMATS];
};
struct CtrlReqs { uint32_t w[REQ_CHUNK]; }; // rnti | tm << 16 | cfi << 20

// grid = (chunk, 1), 256 threads
__global__ __launch_bounds__(256) void dl_ctrl_llr_kernel(const cf32* __restrict__ grid, const cf32* __restrict__ ce, const float* __restrict__ res,
                                                          uint32_t tti0, int sf0, CtrlReqs reqs, CtrlGeom g, float* __restrict__ llr,
                                                          srslte_hip_dl_ctrl_cand_t* __restrict__ cand, uint32_t* __restrict__ ncand,
                                                          srslte_hip_dl_ctrl_res_t* __restrict__ out)
{
  __shared__ int      cfi_s;
  __shared__ float    d[32];      // the PCFICH's 32 LLRs
  __shared__ uint32_t loc[2 * 16]; // candidate locations
  const int      b = sf0 + blockIdx.x, tid = threadIdx.x, sf_idx = (tti0 + b) % 10;
  const uint32_t rq = reqs.w[blockIdx.x];
  const int      P = g.nof_ports, R = g.nof_rx, glen = g.grid_len;
  const cf32*    y = grid + (size_t)b * R * glen;
  const cf32*    h[4];
  for (int p = 0; p < 4; p++) h[p] = ce + ((size_t)b * P + (p < P ? p : 0)) * R * glen;
  const int   v = g.var[sf_idx];
  float*      row = llr + (size_t)b * g.llr_stride;
  if (v == CTRL_SF_UL) { // nothing of the grid is read: no CFI, no candidates, an empty row
    for (int i = tid; i < g.llr_stride; i += 256) row[i] = 0.f;
    if (tid == 0) out[b].cfi = 0, out[b].cfi_corr = 0.f, ncand[b] = 0;
    return;
  }
  const float noise = res[(size_t)b * 10]; // srslte_hip_chest_dl_res_t.noise_estimate
  if (tid == 0) {
    // PCFICH: 16 REs, srslte_predecoding_single_multi / diversity_multi take their generic paths at 16 symbols (precoding.c:325-348,:665-683)
    for (int i = 0; i < 16; i += P) {
      cf32 x[4];
      if (P == 1) {
        x[0] = eq_single_gen(y, h[0], R, glen, g.re[i], noise);
      } else if (P == 2) {
        eq_div2(y, h[0], h[1], R, glen, g.re[i], g.re[i + 1], true, x);
      } else {
        eq_div4(y, h, R, glen, g.re + i, x);
      }
#pragma unroll
      for (int l = 0; l < 4; l++) {
        if (l < P) {
          float o[8];
          demod_dev::demod_f(demod_dev::MOD_QPSK, x[l], o);
          d[2 * (i + l)]     = scr_bit(g.scr_pcfich + sf_idx, 2 * (i + l)) ? -o[0] : o[0];
          d[2 * (i + l) + 1] = scr_bit(g.scr_pcfich + sf_idx, 2 * (i + l) + 1) ? -o[1] : o[1];
        }
      }
    }
    // srslte_pcfich_cfi_decode (pcfich.c:124-142): CFI c's code word is the pattern "011" / "101" / "110" repeated (36.212 Table 5.3.4-1)
    int   index = 0;
    float max_corr = 0.f;
    for (int c = 0; c < 3; c++) {
      float corr = 0.f;
      for (int j = 0; j < 32; j++) corr += (j % 3) == c ? -d[j] : d[j];
      if (corr > max_corr) max_corr = corr, index = c;
    }
    const int cfi_req = (rq >> 20) & 3;
    cfi_s = cfi_req ? cfi_req : index + 1;
    if (g.tdd && (sf_idx == 1 || sf_idx == 6) && cfi_s == 3) cfi_s = 2; // ue_dl.c:351-354
    out[b].cfi = cfi_s;
    out[b].cfi_corr = max_corr;
  }
  __syncthreads();
  const int       cfi = cfi_s, n = g.n[v][cfi - 1], e_bits = 2 * n, ncce = n / 36;
  const uint32_t* re  = g.re + g.off[v][cfi - 1];
  const uint32_t* cs  = g.scr_pdcch + (size_t)sf_idx * g.scr_words;
  const int       G = P, n16 = 16 * (n / 16);
  for (int q = tid; q < n / G; q += 256) {
    cf32 x[4];
    if (P == 1) {
      const int i = q;
      x[0] = i < n16 ? eq_single_avx(y, h[0], R, glen, re[i], noise / 2) : eq_single_gen(y, h[0], R, glen, re[i], noise / 2);
    } else if (P == 2) {
      eq_div2(y, h[0], h[1], R, glen, re[2 * q], re[2 * q + 1], false, x); // 36 NOF_CCE > 32 symbols: the SSE path, no tail
    } else {
      eq_div4(y, h, R, glen, re + 4 * q, x);
    }
#pragma unroll
    for (int l = 0; l < 4; l++) {
      if (l < G) {
        const int i = G * q + l;
        float     o[8];
        demod_dev::demod_f(demod_dev::MOD_QPSK, x[l], o);
        row[2 * i]     = scr_bit(cs, 2 * i) ? -o[0] : o[0];
        row[2 * i + 1] = scr_bit(cs, 2 * i + 1) ? -o[1] : o[1];
      }
    }
  }
  for (int i = e_bits + tid; i < g.llr_stride; i += 256) row[i] = 0.f; // bzero(q->llr) (pdcch.c:441)
  if (tid == 0) {
    // the candidates in the order the searches of ue_dl.c:534-618 try them
    const uint16_t rnti = (uint16_t)(rq & 0xffff);
    const int      tm = (rq >> 16) & 3;
    srslte_hip_dl_ctrl_cand_t* c = cand + (size_t)b * MAX_CAND;
    uint32_t k = 0;
    if (rnti == SIRNTI || rnti == PRNTI || (rnti >= RARNTI_START && rnti <= RARNTI_END)) {
      const uint32_t nc = common_locations(ncce, loc, 6);
      for (int f = 0; f < 2; f++)
        for (uint32_t i = 0; i < nc; i++, k++) c[k].L = loc[2 * i], c[k].ncce = loc[2 * i + 1], c[k].format = f ? F1C : F1A;
    } else if (rnti) {
      const uint32_t nu = ue_locations(ncce, loc, 16, sf_idx, rnti);
      for (int f = 0; f < 2; f++)
        for (uint32_t i = 0; i < nu; i++, k++) c[k].L = loc[2 * i], c[k].ncce = loc[2 * i + 1], c[k].format = UE_FORMATS[tm][f];
      const uint32_t nc = common_locations(ncce, loc, 6);
      for (uint32_t i = 0; i < nc; i++, k++) c[k].L = loc[2 * i], c[k].ncce = loc[2 * i + 1], c[k].format = F1A;
    }
    for (uint32_t i = 0; i < k; i++) c[i].nof_bits = g.dci_bits[c[i].format];
    ncand[b] = k;
  }
}

// grid = (MAX_CAND, nof_sf), one wavefront per candidate
__global__ __launch_bounds__(64) void dl_ctrl_dci_kernel(const float* __restrict__ llr, int llr_stride, srslte_hip_dl_ctrl_cand_t* __restrict__ cand,
                                                         const uint32_t* __restrict__ ncand, int sf0)
{
  __shared__ float              tmp[3 * MAX_F], rmf[3 * MAX_F];
  __shared__ uint16_t           us[3 * MAX_F];
  __shared__ unsigned long long dec[3 * MAX_F + 6];
  __shared__ uint8_t            bits[3 * MAX_F];
  const int b = sf0 + blockIdx.y, lane = threadIdx.x;
  if ((uint32_t)blockIdx.x >= ncand[b]) return;
  srslte_hip_dl_ctrl_cand_t* cd = cand + (size_t)b * MAX_CAND + blockIdx.x;
  const int    L = cd->L, nb = cd->nof_bits, E = 72 << L;
  const float* e = llr + (size_t)b * llr_stride + cd->ncce * 72;
  // skip rule (pdcch.c:382-389): mean |LLR| accumulated in double
  double s = 0.0;
  for (int i = lane; i < E; i += 64) s += (double)fabsf(e[i]);
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (!(s / E > 0.3)) {
    if (lane == 0) cd->skipped = 1, cd->crc_rem = 0, cd->format_decoded = cd->format;
    for (int i = lane; i < 128; i += 64) cd->payload[i] = 0;
    return;
  }
  // srslte_rm_conv_rx (rm_conv.c): the walk over the 3 K_p positions of the circular buffer skips the dummy ones and wraps; valid position j
  // of rank r receives input r, r + 3F, r + 6F, ... in that order (the first replaces the RX_NULL fill, later ones are added unless RX_NULL)
  const int F = nb + 16, nrows = (F - 1) / 32 + 1, Kp = nrows * 32, nd = Kp - F, W = 3 * Kp;
  int       base = 0;
  for (int j0 = 0; j0 < W; j0 += 64) {
    const int  j = j0 + lane, r = j % Kp, di = r / nrows, dj = r % nrows;
    const bool valid = j < W && dj * 32 + RM_PERM[di] >= nd;
    const unsigned long long m = __ballot(valid);
    const int  rank = base + __popcll(m & ((1ull << lane) - 1ull));
    if (j < W) {
      float acc = RX_NULL;
      if (valid) {
        for (int k = rank; k < E; k += 3 * F) {
          const float v = e[k];
          if (acc == RX_NULL) {
            acc = v;
          } else if (v != RX_NULL) {
            acc += v;
          }
        }
      }
      tmp[j] = acc;
    }
    base += __popcll(m);
  }
  __syncthreads();
  for (int i = lane; i < 3 * F; i += 64) {
    const int   ii = i / 3, sidx = i - 3 * ii, di = (ii + nd) / 32, dj = (ii + nd) % 32;
    const float o = tmp[Kp * sidx + RM_PERM_INV[dj] * nrows + di];
    rmf[i]        = o != RX_NULL ? o : 0.f;
  }
  for (int i = 3 * F + lane; i < 3 * F + 6; i += 64) dec[i] = 0ull;
  __syncthreads();
  viterbi_dev::quant_fus(rmf, us, 3 * F, lane);
  viterbi_dev::decode37_tb(us, dec, bits, F, lane);
  __syncthreads();
  const uint8_t* msg = bits + F; // the middle repetition
  for (int i = lane; i < 128; i += 64) cd->payload[i] = i < F ? msg[i] : 0;
  if (lane == 0) {
    uint32_t p = 0;
    for (int i = 0; i < 16; i++) p = (p << 1) | msg[nb + i];
    cd->skipped        = 0;
    cd->crc_rem        = p ^ crc16(msg, nb);
    cd->format_decoded = (cd->format == F0 || cd->format == F1A) ? (msg[0] == 0 ? F0 : F1A) : cd->format;
  }
}

// grid = ceil(nof_sf / 64), one lane per subframe
__global__ __launch_bounds__(64) void dl_ctrl_select_kernel(const srslte_hip_dl_ctrl_cand_t* __restrict__ cand, const uint32_t* __restrict__ ncand,
                                                            int sf0, CtrlReqs reqs, int nof_sf, srslte_hip_dl_ctrl_res_t* __restrict__ out,
                                                            srslte_hip_dci_msg_t* __restrict__ msg)
{
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= nof_sf) return;
  const int                        b    = sf0 + i;
  const uint32_t                   rnti = reqs.w[i] & 0xffff;
  const srslte_hip_dl_ctrl_cand_t* c    = cand + (size_t)b * MAX_CAND;
  int                              hit  = -1;
  for (uint32_t k = 0; k < ncand[b] && hit < 0; k++) {
    if (!c[k].skipped && c[k].crc_rem == rnti && c[k].format_decoded == c[k].format) hit = (int)k;
  }
  srslte_hip_dci_msg_t* m = msg + b;
  out[b].nof_dci          = hit >= 0 ? 1 : 0;
  for (int j = 0; j < 128; j += 4) *reinterpret_cast<uint32_t*>(m->payload + j) = hit >= 0 ? *reinterpret_cast<const uint32_t*>(c[hit].payload + j) : 0u;
  m->nof_bits = hit >= 0 ? c[hit].nof_bits : 0;
  m->L        = hit >= 0 ? c[hit].L : 0;
  m->ncce     = hit >= 0 ? c[hit].ncce : 0;
  m->format   = hit >= 0 ? (int)c[hit].format : 0;
  m->rnti     = hit >= 0 ? (uint16_t)rnti : 0;
}

// ---------------------------------------------------------------- host: DCI sizes (dci.c); the REG lists and sequences are in ctrl_host.cpp
static uint32_t riv_nbits(uint32_t n) { return (uint32_t)ceilf(log2f((float)n * ((float)n + 1) / 2)); }
static bool     ambiguous(uint32_t n)
{
  static const uint32_t a[10] = {12, 14, 16, 20, 24, 26, 32, 40, 44, 56};
  for (uint32_t v : a)
    if (n == v) return true;
  return false;
}
static uint32_t type0_P(uint32_t prb) { return prb <= 10 ? 1 : prb <= 26 ? 2 : prb <= 63 ? 3 : 4; } // ra.c:62-72

// srslte_dci_format_sizeof (dci.c:114-360), cif / multiple CSI request / SRS request / resource allocation type bit off. A TDD cell adds the
// DAI / UL index (2 bits) and a fourth HARQ process bit (dci.c:38-40, :142-143, :176-189); the uplink-downlink configuration does not enter
static uint32_t dci_sizeof(uint32_t prb, uint32_t ports, int f, bool tdd = false)
{
  const uint32_t dai = tdd ? 2 : 0, pid = tdd ? 4 : 3;
  const uint32_t f0_ = 1 + 1 + riv_nbits(prb) + 5 + 1 + 2 + 3 + dai + 1;
  uint32_t       f1a = 1 + 1 + riv_nbits(prb) + 5 + pid + 1 + 2 + 2 + dai;
  while (f1a < f0_) f1a++;
  if (ambiguous(f1a)) f1a++;
  uint32_t f0 = f0_;
  while (f0 < f1a) f0++;
  const uint32_t rbg = (uint32_t)ceilf((float)prb / type0_P(prb)) + (prb > 10 ? 1 : 0);
  switch (f) {
    case F0: return f0;
    case F1A: return f1a;
    case F1: {
      uint32_t n = rbg + 5 + pid + 1 + 2 + 2 + dai;
      while (n == f0 || n == f1a || ambiguous(n)) n++;
      return n;
    }
    case F1C: { // ra.c:81-120: N_gap,1, n_vrb_dl = 2 min(N_gap, N_rb - N_gap), step 2 / 4
      const uint32_t ngap = prb <= 10 ? prb / 2 : prb == 11 ? 4 : prb <= 19 ? 8 : prb <= 26 ? 12 : prb <= 44 ? 18 : prb <= 49 ? 27 : prb <= 63 ? 27
                          : prb <= 79 ? 32 : 48;
      const uint32_t nvrb = 2 * (ngap < prb - ngap ? ngap : prb - ngap), step = prb < 50 ? 2 : 4;
      return riv_nbits(nvrb / step) + 5 + (prb >= 50 ? 1 : 0);
    }
    case F1B:
    case F1D: {
      uint32_t n = f1a - 1 + (ports <= 2 ? 2 : 4) + 1 + dai;
      while (ambiguous(n)) n++;
      return n;
    }
    case F2:
    case F2A:
    case F2B: {
      const uint32_t pre = f == F2 ? (ports <= 2 ? 3 : 6) : f == F2A ? (ports <= 2 ? 0 : 2) : 0;
      uint32_t       n   = rbg + 2 + pid + 1 + 2 * (5 + 1 + 2) + pre + dai;
      while (ambiguous(n)) n++;
      return n;
    }
    default: return 0;
  }
}

} // namespace

struct srslte_hip_dl_ctrl {
  srslte_hip_dl_ctrl_cfg_t cfg;
  CtrlGeom                 g;
  DevBuf<uint32_t>         re, scr, ncand;
  DevBuf<float>            llr;
  DevBuf<srslte_hip_dl_ctrl_cand_t> cand;
  int                      tdd_sf_config = -1; // uplink-downlink configuration of a TDD object; -1: FDD
  BcastTables*             bc = nullptr; // the MIB decoder (pbch.hip)
  PhichRx*                 ph = nullptr; // the PHICH receiver (phich.hip), once srslte_hip_dl_ctrl_set_max_phich has made it
};

const BcastTables* dl_ctrl_bcast(const srslte_hip_dl_ctrl_t* q) { return q ? q->bc : nullptr; }

DlCtrlView dl_ctrl_view(srslte_hip_dl_ctrl_t* q) { return DlCtrlView{&q->cfg, q->tdd_sf_config, q->g.scr_pcfich, q->cand.get(), q->ncand.get()}; }
PhichRx*   dl_ctrl_phich(const srslte_hip_dl_ctrl_t* q) { return q->ph; }
void       dl_ctrl_set_phich(srslte_hip_dl_ctrl_t* q, PhichRx* t) { q->ph = t; }

int dl_ctrl_check(const srslte_hip_dl_ctrl_t* q, uint32_t tti0, uint32_t nof_sf, const srslte_hip_dl_ctrl_req_t* reqs)
{
  if (!q || !reqs || nof_sf < 1 || nof_sf > q->cfg.max_batch) return SRSLTE_ERROR_INVALID_INPUTS;
  for (uint32_t b = 0; b < nof_sf; b++) {
    if (reqs[b].mbsfn || reqs[b].tm > 3 || reqs[b].cfi > 3) return SRSLTE_ERROR_INVALID_INPUTS;
    // TDD: subframes 1 and 6 hold at most two control symbols (36.211 Table 6.7-1)
    const uint32_t sf_idx = (tti0 + b) % 10;
    if (q->cfg.tdd && reqs[b].cfi == 3 && (sf_idx == 1 || sf_idx == 6)) return SRSLTE_ERROR_INVALID_INPUTS;
  }
  return SRSLTE_SUCCESS;
}

extern "C" {

int srslte_hip_dl_ctrl_pcfich_re(const srslte_hip_dl_ctrl_cfg_t* cfg, uint32_t* re, uint32_t max)
{
  CtrlRegs  r;
  const int rc = ctrl_build_regs(cfg, r);
  if (rc != SRSLTE_SUCCESS) return rc;
  if (!re || max < r.pcfich.size()) return SRSLTE_ERROR_INVALID_INPUTS;
  memcpy(re, r.pcfich.data(), r.pcfich.size() * 4);
  return (int)r.pcfich.size();
}

int srslte_hip_dl_ctrl_pdcch_re(const srslte_hip_dl_ctrl_cfg_t* cfg, uint32_t cfi, uint32_t* re, uint32_t max)
{
  if (cfi < 1 || cfi > 3) return SRSLTE_ERROR_INVALID_INPUTS;
  CtrlRegs  r;
  const int rc = ctrl_build_regs(cfg, r);
  if (rc != SRSLTE_SUCCESS) return rc;
  const std::vector<uint32_t>& v = r.pdcch[cfi - 1];
  if (!re || max < v.size()) return SRSLTE_ERROR_INVALID_INPUTS;
  memcpy(re, v.data(), v.size() * 4);
  return (int)v.size();
}

uint32_t srslte_hip_pdcch_ue_locations_ncce(uint32_t nof_cce, uint32_t* loc, uint32_t max_candidates, uint32_t sf_idx, uint16_t rnti)
{
  return loc ? ue_locations(nof_cce, loc, max_candidates, sf_idx, rnti) : 0;
}

uint32_t srslte_hip_pdcch_common_locations_ncce(uint32_t nof_cce, uint32_t* loc, uint32_t max_candidates)
{
  return loc ? common_locations(nof_cce, loc, max_candidates) : 0;
}

uint32_t srslte_hip_dci_format_sizeof(uint32_t nof_prb, uint32_t nof_ports, int format)
{
  if (nof_prb < 6 || nof_prb > 110) return 0;
  return dci_sizeof(nof_prb, nof_ports, format);
}

uint32_t srslte_hip_dci_format_sizeof_tdd(uint32_t nof_prb, uint32_t nof_ports, int format)
{
  if (nof_prb < 6 || nof_prb > 110) return 0;
  return dci_sizeof(nof_prb, nof_ports, format, true);
}

int srslte_hip_dl_ctrl_tdd_mi(uint32_t tdd_sf_config, uint32_t sf_idx) { return ctrl_tdd_mi(tdd_sf_config, sf_idx); }

int srslte_hip_dl_ctrl_pdcch_re_tdd(const srslte_hip_dl_ctrl_cfg_t* cfg, uint32_t tdd_sf_config, uint32_t sf_idx, uint32_t cfi, uint32_t* re, uint32_t max)
{
  const int mi = ctrl_tdd_mi(tdd_sf_config, sf_idx);
  if (cfi < 1 || cfi > 3 || mi < 0 || !cfg) return SRSLTE_ERROR_INVALID_INPUTS;
  CtrlRegs  r;
  const int rc = ctrl_build_regs_opts(cfg, (uint32_t)mi, sf_idx == 1 || sf_idx == 6, r);
  if (rc != SRSLTE_SUCCESS) return rc;
  const std::vector<uint32_t>& v = r.pdcch[cfi - 1];
  if (!re || max < v.size()) return SRSLTE_ERROR_INVALID_INPUTS;
  memcpy(re, v.data(), v.size() * 4);
  return (int)v.size();
}

void srslte_hip_dl_ctrl_destroy(srslte_hip_dl_ctrl_t* q)
{
  if (!q) return;
  bcast_tables_destroy(q->bc);
  phich_rx_destroy(q->ph);
  delete q;
}

// tdd_sf_config < 0: FDD
static srslte_hip_dl_ctrl_t* dl_ctrl_make(const srslte_hip_dl_ctrl_cfg_t* cfg, int tdd_sf_config)
{
  if (!ctrl_cell_ok(cfg) || cfg->nof_rx_antennas < 1 || cfg->nof_rx_antennas > 4 || cfg->max_batch < 1) return nullptr;
  CtrlRegsSet set;
  if (ctrl_build_regs_set(cfg, tdd_sf_config, set) != SRSLTE_SUCCESS) return nullptr;
  srslte_hip_dl_ctrl_t* q = new srslte_hip_dl_ctrl_t();
  q->cfg                  = *cfg;
  q->tdd_sf_config        = tdd_sf_config;
  CtrlGeom& g             = q->g;
  memset(&g, 0, sizeof(g));
  std::vector<uint32_t> re(set.v[0].pcfich); // the PCFICH REGs are the same in every variant
  bool                  cce = true;
  for (size_t v = 0; v < set.v.size(); v++) {
    for (int c = 0; c < 3; c++) {
      const std::vector<uint32_t>& pd = set.v[v].pdcch[c];
      g.off[v][c] = (int)re.size(), g.n[v][c] = (int)pd.size();
      re.insert(re.end(), pd.begin(), pd.end());
    }
    cce = cce && g.n[v][0] >= 36;
  }
  memcpy(g.var, set.var, sizeof(g.var));
  g.tdd        = tdd_sf_config >= 0 ? 1 : 0;
  g.nof_ports  = (int)cfg->nof_ports;
  g.nof_rx     = (int)cfg->nof_rx_antennas;
  g.grid_len   = (cfg->cp_ext ? 12 : 14) * 12 * (int)cfg->nof_prb;
  g.llr_stride = (2 * (int)set.max_pdcch_re + 3) & ~3; // 72 NOF_CCE(3) of the largest list
  for (int f = 0; f < NOF_FORMATS; f++) g.dci_bits[f] = dci_sizeof(cfg->nof_prb, cfg->nof_ports, f, g.tdd != 0);
  if (g.dci_bits[F2] + 16 > MAX_F || !cce) { // every cell of the range fits; an FDD CFI-1 region without a CCE does not happen, and
                                               // ctrl_build_regs_set has refused the TDD cells where one does
    delete q;
    return nullptr;
  }
  // scrambling: srslte_sequence_pcfich (32 bits) and srslte_sequence_pdcch sized 8 srslte_regs_pdcch_nregs(3) bits of the largest list, slot 2 sf_idx
  std::vector<uint32_t> scr;
  ctrl_scrambling(cfg->cell_id, 2 * set.max_pdcch_re, scr, &g.scr_words);
  const size_t B = cfg->max_batch;
  if (q->re.upload(re) || q->scr.upload(scr) || q->llr.alloc(B * g.llr_stride) || q->cand.alloc(B * MAX_CAND) || q->ncand.alloc(B) ||
      !(q->bc = bcast_tables_create(cfg, cfg->phich_ext, cfg->phich_resources, true))) {
    hip_log("[srslte_hip] srslte_hip_dl_ctrl_create: device allocation failed\n");
    srslte_hip_dl_ctrl_destroy(q);
    return nullptr;
  }
  g.re = q->re.get(), g.scr_pcfich = q->scr.get(), g.scr_pdcch = q->scr.get() + 10;
  return q;
}

srslte_hip_dl_ctrl_t* srslte_hip_dl_ctrl_create(const srslte_hip_dl_ctrl_cfg_t* cfg) { return cfg && !cfg->tdd ? dl_ctrl_make(cfg, -1) : nullptr; }

srslte_hip_dl_ctrl_t* srslte_hip_dl_ctrl_create_tdd(const srslte_hip_dl_ctrl_cfg_t* cfg, uint32_t tdd_sf_config)
{
  return cfg && cfg->tdd == 1 && tdd_sf_config <= 6 ? dl_ctrl_make(cfg, (int)tdd_sf_config) : nullptr;
}

int srslte_hip_dl_ctrl_batch(srslte_hip_dl_ctrl_t* q, const void* d_grid, const void* d_ce, const void* d_res, uint32_t tti0, uint32_t nof_sf,
                             const srslte_hip_dl_ctrl_req_t* reqs, srslte_hip_dl_ctrl_res_t* d_out, srslte_hip_dci_msg_t* d_msg, void* stream)
{
  if (!d_grid || !d_ce || !d_res || !d_out || !d_msg) return SRSLTE_ERROR_INVALID_INPUTS;
  if (int r = dl_ctrl_check(q, tti0, nof_sf, reqs)) return r;
  hipStream_t st = (hipStream_t)stream;
  for (uint32_t s0 = 0; s0 < nof_sf; s0 += REQ_CHUNK) {
    const uint32_t n = nof_sf - s0 < (uint32_t)REQ_CHUNK ? nof_sf - s0 : (uint32_t)REQ_CHUNK;
    CtrlReqs       r;
    memset(&r, 0, sizeof(r));
    for (uint32_t i = 0; i < n; i++) r.w[i] = reqs[s0 + i].rnti | reqs[s0 + i].tm << 16 | reqs[s0 + i].cfi << 20;
    hipLaunchKernelGGL(dl_ctrl_llr_kernel, dim3(n), dim3(256), 0, st, (const cf32*)d_grid, (const cf32*)d_ce, (const float*)d_res, tti0, (int)s0, r, q->g,
                       q->llr.get(), q->cand.get(), q->ncand.get(), d_out);
    LAUNCH_CHECK();
  }
  for (uint32_t s0 = 0; s0 < nof_sf; s0 += DCI_CHUNK) { // gridDim.y stays below 65536 whatever max_batch is
    const uint32_t n = nof_sf - s0 < (uint32_t)DCI_CHUNK ? nof_sf - s0 : (uint32_t)DCI_CHUNK;
    hipLaunchKernelGGL(dl_ctrl_dci_kernel, dim3(MAX_CAND, n), dim3(64), 0, st, q->llr.get(), q->g.llr_stride, q->cand.get(), q->ncand.get(), (int)s0);
    LAUNCH_CHECK();
  }
  for (uint32_t s0 = 0; s0 < nof_sf; s0 += REQ_CHUNK) {
    const uint32_t n = nof_sf - s0 < (uint32_t)REQ_CHUNK ? nof_sf - s0 : (uint32_t)REQ_CHUNK;
    CtrlReqs       r;
    memset(&r, 0, sizeof(r));
    for (uint32_t i = 0; i < n; i++) r.w[i] = reqs[s0 + i].rnti;
    hipLaunchKernelGGL(dl_ctrl_select_kernel, dim3(ceil_div((int)n, 64)), dim3(64), 0, st, q->cand.get(), q->ncand.get(), (int)s0, r, (int)n, d_out, d_msg);
    LAUNCH_CHECK();
  }
  return SRSLTE_SUCCESS;
}

const void* srslte_hip_dl_ctrl_debug_buffer(const srslte_hip_dl_ctrl_t* q, int which)
{
  if (!q) return nullptr;
  switch (which) {
    case 0: return q->llr.get();
    case 1: return q->cand.get();
    case 2: return q->ncand.get();
    default: return nullptr;
  }
}

uint32_t srslte_hip_dl_ctrl_llr_stride(const srslte_hip_dl_ctrl_t* q) { return q ? (uint32_t)q->g.llr_stride : 0; }

} // extern "C"
