// UL half of the DL control region receive for gfx950 (include/srslte_hip/phy_hip.h, "DL control region receive: UL DCIs and PHICH"): what
// srslte_ue_dl_find_ul_dci (ue_dl.c:480-531, with the pending rule of dci_blind_search :448-470) and srslte_ue_dl_decode_phich (:673-703 ->
// srslte_phich_calc + srslte_phich_decode, phich.c:132-143, :181-313) do per TTI, for a batch of subframes. One launch on the caller's stream
// behind the three of srslte_hip_dl_ctrl_batch (pdcch.hip), one kernel with two kinds of workgroup:
//   UL selection   one lane per subframe. Formats 0 and 1A have one size and srslte_pdcch_decode_msg is a pure function of the LLR row, so
//                  the format-0 search decodes nothing: every candidate it would decode has been decoded by the 1A search already and lies
//                  in the 38-entry candidate buffer of dl_ctrl_dci_kernel. No Viterbi run is added; this part reads
//                  srslte_hip_dl_ctrl_cand_t only. It is not free, though: a lane walks up to 38 candidates of 156 bytes with dependent
//                  loads and writes five 148-byte messages, which is latency - measured 57-64 us for 128 subframes, twice
//                  dl_ctrl_select_kernel and several times the PHICH part (a wavefront per subframe is the next step,
//                  and with it a kernel of its own for this half).
//   PHICH          four lanes per request, lane i < 3 owns REG i of the group's mapping unit: its 4 REs on every receive antenna and port,
//                  the equaliser's generic body (12 symbols are below every SIMD threshold of precoding.c), descrambling, de-spreading into
//                  z[i] with j = 0 .. N_SF - 1 in the reference's order, the BPSK soft bit; lane 0 gathers the three bits with shuffles for
//                  srslte_phich_ack_decode. 64 requests per workgroup: 2048 requests are 32 workgroups.
#include "common.hpp"
#include "ctrl_host.hpp"
#include "ctrl_rx_dev.hpp"
#include "dev_buf.hpp"
#include "phy_hip_internal.hpp"
#include <string.h>
#include <vector>

namespace {

constexpr int      MAX_CAND  = SRSLTE_HIP_DL_CTRL_MAX_CAND;
constexpr int      MAX_UL    = SRSLTE_HIP_DL_CTRL_MAX_UL_DCI;
constexpr int      REQ_CHUNK = 128; // subframes per launch (their RNTIs travel as a kernel argument), as in pdcch.hip
constexpr int      PH_BLOCK  = 64;  // PHICH requests per workgroup
constexpr uint16_t SIRNTI = 0xFFFF, PRNTI = 0xFFFE, RARNTI_START = 0x0001, RARNTI_END = 0x000A; // phy_common.h:71-80
enum { F0 = 0, F1A = 2 };                                                                        // srslte_dci_format_t

struct UlReqs { uint32_t rnti[REQ_CHUNK]; };
struct PhichGeom {
  const uint32_t* re;  // per REG variant [units][12]: the REs of each PHICH mapping unit in srslte_regs_phich_get order
  const uint32_t* scr; // [10] words: srslte_sequence_pcfich of each subframe; its first 12 bits are srslte_sequence_phich
  int             off[CTRL_MAX_VAR]; // where each variant's list starts in re
  uint8_t         var[10];           // the variant of subframe sf_idx (ctrl_host.hpp); FDD: all 0
  int             nof_ports, nof_rx, grid_len, cp_ext;
};

// srslte_ue_dl_find_ul_dci of one subframe from the candidates the DL search decoded
__device__ __forceinline__ void ul_select(const srslte_hip_dl_ctrl_cand_t* __restrict__ c, uint32_t n, uint32_t rnti,
                                          srslte_hip_dl_ctrl_ul_res_t* __restrict__ out, srslte_hip_dci_msg_t* __restrict__ msg)
{
  uint32_t pend = 0, npend = 0; // candidate numbers of the pending list, 6 bits each
  const bool crnti = rnti && rnti != SIRNTI && rnti != PRNTI && !(rnti >= RARNTI_START && rnti <= RARNTI_END);
  if (!crnti) n = 0;
  // the walk of srslte_ue_dl_find_dl_dci up to its first DL hit: a format-0 message met while 1A is searched is kept, unless 5 are held
  // or one with the same size and payload is (find_dci, ue_dl.c:406-420)
  for (uint32_t k = 0; k < n; k++) {
    if (c[k].skipped || c[k].crc_rem != rnti) continue;
    if (c[k].format_decoded == c[k].format) break;
    if (c[k].format == F1A && c[k].format_decoded == F0 && npend < (uint32_t)MAX_UL) {
      bool dup = false;
      for (uint32_t p = 0; p < npend && !dup; p++) {
        const srslte_hip_dl_ctrl_cand_t* o = c + ((pend >> (6 * p)) & 63u);
        if (o->nof_bits == c[k].nof_bits) {
          dup = true;
          for (uint32_t i = 0; i < c[k].nof_bits; i++) dup = dup && o->payload[i] == c[k].payload[i];
        }
      }
      if (!dup) pend |= k << (6 * npend), npend++;
    }
  }
  const uint32_t from_pending = npend ? 1u : 0u;
  if (!npend) {
    // nothing pending: the UE-specific locations are searched for format 0 (ue_dl.c:497-515). They are the leading 1A candidates, and a
    // format-0 decode of one of them is the 1A decode that is there already
    for (uint32_t k = 0; k < n && c[k].format == F1A && !npend; k++) {
      if (!c[k].skipped && c[k].crc_rem == rnti && c[k].format_decoded == F0) pend = k, npend = 1;
    }
  }
  out->nof_ul_dci = npend;
  out->pending    = from_pending;
  for (uint32_t j = 0; j < (uint32_t)MAX_UL; j++) {
    const bool                       on = j < npend;
    const srslte_hip_dl_ctrl_cand_t* s  = c + (on ? (pend >> (6 * j)) & 63u : 0u);
    srslte_hip_dci_msg_t*            m  = msg + j;
    for (int i = 0; i < 128; i += 4) *reinterpret_cast<uint32_t*>(m->payload + i) = on ? *reinterpret_cast<const uint32_t*>(s->payload + i) : 0u;
    m->nof_bits = on ? s->nof_bits : 0;
    m->L        = on ? s->L : 0;
    m->ncce     = on ? s->ncce : 0;
    m->format   = on ? (int)F0 : 0;
    m->rnti     = on ? (uint16_t)rnti : 0;
  }
}

// conj(w[j]) d / N_SF of phich.c:286-300 with w = w_normal / w_ext[nseq] (36.211 Table 6.9.1-2): the sequences are +-1 or +-j, so the
// product is a sign change or a swap and the division by 4 / 2 is exact
__device__ __forceinline__ cf32 despread_term(cf32 d, uint32_t nseq, int j, int ext)
{
  bool neg, imag;
  if (ext) {
    imag = nseq >= 2;
    neg  = (nseq & 1) && (j & 1);
  } else {
    imag = nseq >= 4;
    const uint32_t q = nseq & 3;
    neg = q == 1 ? (j & 1) : q == 2 ? (j >= 2) : q == 3 ? (j == 1 || j == 2) : false;
  }
  cf32 t = imag ? make_float2(d.y, -d.x) : d; // conj(j) d = -j d
  if (neg) t = make_float2(-t.x, -t.y);
  const float s = ext ? 0.5f : 0.25f;
  return make_float2(t.x * s, t.y * s);
}

// grid = (ul_blocks + ceil(nof_phich / 64)), 256 threads. Workgroups below ul_blocks: subframes sf0 .. sf0 + nof_sf - 1, one lane each.
// The others: PHICH requests req[2 q] = subframe, req[2 q + 1] = ngroup | nseq << 16, four lanes each
__global__ __launch_bounds__(256) void dl_ctrl_ul_phich_kernel(const srslte_hip_dl_ctrl_cand_t* __restrict__ cand, const uint32_t* __restrict__ ncand,
                                                               int sf0, UlReqs reqs, int nof_sf, int ul_blocks,
                                                               srslte_hip_dl_ctrl_ul_res_t* __restrict__ ul_out, srslte_hip_dci_msg_t* __restrict__ ul_msg,
                                                               const cf32* __restrict__ grid, const cf32* __restrict__ ce, const float* __restrict__ res,
                                                               uint32_t tti0, PhichGeom g, const uint32_t* __restrict__ req, int nof_phich,
                                                               srslte_hip_phich_res_t* __restrict__ ph_out, srslte_hip_phich_soft_t* __restrict__ soft)
{
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < ul_blocks) {
    const int i = blockIdx.x * 256 + tid;
    if (i < nof_sf) {
      const int b = sf0 + i;
      ul_select(cand + (size_t)b * MAX_CAND, ncand[b], reqs.rnti[i] & 0xffffu, ul_out + b, ul_msg + (size_t)b * MAX_UL);
    }
    return;
  }
  const int  q = ((int)blockIdx.x - ul_blocks) * PH_BLOCK + (tid >> 2), i = tid & 3;
  const bool on = q < nof_phich && i < 3;
  float      bit = 0.f;
  uint32_t   ngroup = 0, nseq = 0;
  if (on) {
    const uint32_t b = req[2 * q], w = req[2 * q + 1];
    ngroup = w & 0xffffu, nseq = w >> 16;
    const int       P = g.nof_ports, R = g.nof_rx, glen = g.grid_len, ext = g.cp_ext;
    const uint32_t  unit = ext ? ngroup >> 1 : ngroup, odd = ext ? ngroup & 1u : 0u;
    const uint32_t  sf_idx = (tti0 + b) % 10, scr = g.scr[sf_idx];
    const uint32_t* re = g.re + g.off[g.var[sf_idx]] + 12 * unit + 4 * i; // the host refused uplink subframes: var < CTRL_MAX_VAR
    const cf32*     y = grid + (size_t)b * R * glen;
    const cf32*     h[4];
    for (int p = 0; p < 4; p++) h[p] = ce + ((size_t)b * P + (p < P ? p : 0)) * R * glen;
    const float noise = res[(size_t)b * 10]; // srslte_hip_chest_dl_res_t.noise_estimate, not halved (phich.c:252-253)
    cf32        lo[2], hi[2]; // d0[4 i], d0[4 i + 1] and d0[4 i + 2], d0[4 i + 3] of phich.c
    if (P == 1) {
#pragma unroll
      for (int l = 0; l < 2; l++) lo[l] = eq_single_gen(y, h[0], R, glen, re[l], noise), hi[l] = eq_single_gen(y, h[0], R, glen, re[2 + l], noise);
    } else if (P == 2) {
      eq_div2(y, h[0], h[1], R, glen, re[0], re[1], true, lo);
      eq_div2(y, h[0], h[1], R, glen, re[2], re[3], true, hi);
    } else {
      cf32 x[4];
      eq_div4(y, h, R, glen, re, x);
      lo[0] = x[0], lo[1] = x[1], hi[0] = x[2], hi[1] = x[3];
    }
    // normal CP: d = d0, z[i] over d[4 i + j]; extended CP: group 2m takes symbols 0, 1 and group 2m + 1 symbols 2, 3 of each REG
    // (phich.c:263-277), z[i] over d[2 i + j]. srslte_scrambling_c with bit (index in d) of the sequence, then the sum in j order
    cf32 z = make_float2(0.f, 0.f);
    if (ext) {
#pragma unroll
      for (int j = 0; j < 2; j++) {
        cf32 d = odd ? hi[j] : lo[j];
        if ((scr >> (2 * i + j)) & 1u) d = make_float2(-d.x, -d.y);
        const cf32 t = despread_term(d, nseq, j, 1);
        z.x += t.x, z.y += t.y;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        cf32 d = j < 2 ? lo[j] : hi[j - 2];
        if ((scr >> (4 * i + j)) & 1u) d = make_float2(-d.x, -d.y);
        const cf32 t = despread_term(d, nseq, j, 0);
        z.x += t.x, z.y += t.y;
      }
    }
    bit             = (float)(-(double)(z.x + z.y) / 1.4142135623730951); // demod_bpsk_lte (demod_soft.c:58-62), as demod_dev::demod_f
    soft[q].z[i][0] = z.x, soft[q].z[i][1] = z.y;
    soft[q].bits[i] = bit;
  }
  // srslte_phich_ack_decode (phich.c:149-172): the correlations with -1 -1 -1 and 1 1 1 over 3, the second wins only if strictly greater
  const int   base = (tid & 63) & ~3;
  const float b0 = __shfl(bit, base, 64), b1 = __shfl(bit, base + 1, 64), b2 = __shfl(bit, base + 2, 64);
  if (on && i == 0) {
    float    max_corr = -9999.f, dist = 0.f;
    uint32_t ack = 0;
    float    r0  = 0.f;
    r0 += -1.0f * b0, r0 += -1.0f * b1, r0 += -1.0f * b2;
    const float c0 = r0 / 3;
    if (c0 > max_corr) max_corr = c0, dist = c0, ack = 0;
    float r1 = 0.f;
    r1 += b0, r1 += b1, r1 += b2;
    const float c1 = r1 / 3;
    if (c1 > max_corr) max_corr = c1, dist = c1, ack = 1;
    ph_out[q].ack_value = ack;
    ph_out[q].distance  = dist;
    ph_out[q].ngroup    = ngroup;
    ph_out[q].nseq      = nseq;
  }
}

} // namespace

// The PHICH receiver's tables and buffers of a srslte_hip_dl_ctrl_t, made by srslte_hip_dl_ctrl_set_max_phich
struct PhichRx {
  uint32_t                 ngroups_m1 = 0, max_phich = 0;
  uint32_t                 units[CTRL_MAX_VAR] = {}; // mapping units of each REG variant
  int                      off[CTRL_MAX_VAR]   = {}; // its list in re
  uint8_t                  var[10];
  DevBuf<uint32_t>         re;
  DescStage                req;
  DevBuf<srslte_hip_phich_soft_t> soft;
  std::vector<uint32_t>    words; // the requests of a call, as they are built
};

void phich_rx_destroy(PhichRx* t) { delete t; }

namespace {

// phich_calc of ctrl_host.hpp and the group check of srslte_phich_decode (phich.c:215-218) for every request; fills t->words. The sequence
// check of phich.c:204-214 has nothing to refuse: srslte_phich_calc reduces nseq modulo the CP's sequence count
int phich_prepare(const srslte_hip_dl_ctrl_cfg_t& c, PhichRx* t, uint32_t tti0, uint32_t nof_sf, const srslte_hip_phich_req_t* ph, uint32_t nof_phich)
{
  if (nof_phich == 0) return SRSLTE_SUCCESS;
  if (!t || !ph || nof_phich > t->max_phich) return SRSLTE_ERROR_INVALID_INPUTS;
  t->words.resize(2 * (size_t)nof_phich);
  for (uint32_t i = 0; i < nof_phich; i++) {
    const srslte_hip_phich_req_t& p = ph[i];
    uint32_t                      ngroup, nseq;
    if (p.sf >= nof_sf || p.I_phich > 1) return SRSLTE_ERROR_INVALID_INPUTS;
    // TDD: the subframe's own group count, mi ngroups_m1 - none in an uplink subframe or with mi = 0, and I_phich = 1 only where mi = 2
    const uint8_t v = t->var[(tti0 + p.sf) % 10];
    if (v == CTRL_SF_UL) return SRSLTE_ERROR_INVALID_INPUTS;
    phich_calc(t->ngroups_m1, c.cp_ext, p.n_prb_lowest, p.n_dmrs, p.I_phich, &ngroup, &nseq);
    if (ngroup >= t->units[v] * (c.cp_ext ? 2u : 1u)) return SRSLTE_ERROR_INVALID_INPUTS;
    t->words[2 * i] = p.sf, t->words[2 * i + 1] = ngroup | nseq << 16;
  }
  return SRSLTE_SUCCESS;
}

// the requests of t->words to the device through the pinned ring
int phich_upload(PhichRx* t, uint32_t nof_phich, hipStream_t st)
{
  uint32_t* h = nullptr;
  if (int r = t->req.begin(&h)) return r;
  const size_t bytes = 8 * (size_t)nof_phich;
  memcpy(h, t->words.data(), bytes);
  return t->req.commit(bytes, st);
}

PhichGeom phich_geom(const DlCtrlView& v, const PhichRx* t)
{
  PhichGeom g;
  g.re = t ? t->re.get() : nullptr, g.scr = v.d_scr_pcfich;
  g.nof_ports = (int)v.cfg->nof_ports, g.nof_rx = (int)v.cfg->nof_rx_antennas;
  g.grid_len = (v.cfg->cp_ext ? 12 : 14) * 12 * (int)v.cfg->nof_prb, g.cp_ext = v.cfg->cp_ext ? 1 : 0;
  memset(g.off, 0, sizeof(g.off)), memset(g.var, 0, sizeof(g.var));
  if (t) memcpy(g.off, t->off, sizeof(g.off)), memcpy(g.var, t->var, sizeof(g.var));
  return g;
}

} // namespace

extern "C" {

int srslte_hip_dl_ctrl_set_max_phich(srslte_hip_dl_ctrl_t* q, uint32_t max_phich)
{
  if (!q) return SRSLTE_ERROR_INVALID_INPUTS;
  const DlCtrlView v = dl_ctrl_view(q);
  phich_rx_destroy(dl_ctrl_phich(q));
  dl_ctrl_set_phich(q, nullptr);
  if (max_phich == 0) return SRSLTE_SUCCESS;
  CtrlRegsSet set;
  if (ctrl_build_regs_set(v.cfg, v.tdd_sf_config, set) != SRSLTE_SUCCESS || set.v[0].ngroups_m1 == 0) return SRSLTE_ERROR;
  PhichRx* t    = new PhichRx();
  t->ngroups_m1 = set.v[0].ngroups_m1;
  t->max_phich  = max_phich;
  memcpy(t->var, set.var, sizeof(t->var));
  std::vector<uint32_t> re;
  for (size_t i = 0; i < set.v.size(); i++) {
    t->units[i] = set.v[i].units, t->off[i] = (int)re.size();
    re.insert(re.end(), set.v[i].phich.begin(), set.v[i].phich.end());
  }
  if (re.empty()) re.push_back(0u); // a TDD configuration whose downlink subframes all have mi = 0: every request is refused
  if (t->re.upload(re) || t->req.init(8 * (size_t)max_phich) || t->soft.alloc(max_phich)) {
    hip_log("[srslte_hip] srslte_hip_dl_ctrl_set_max_phich: device allocation failed\n");
    phich_rx_destroy(t);
    return SRSLTE_ERROR;
  }
  dl_ctrl_set_phich(q, t); // the control object owns it from here: srslte_hip_dl_ctrl_destroy frees it
  return SRSLTE_SUCCESS;
}

int srslte_hip_dl_ctrl_phich_batch(srslte_hip_dl_ctrl_t* q, const void* d_grid, const void* d_ce, const void* d_res, uint32_t tti0, uint32_t nof_sf,
                                   const srslte_hip_phich_req_t* phich, uint32_t nof_phich, srslte_hip_phich_res_t* d_phich_res, void* stream)
{
  if (!q || !d_grid || !d_ce || !d_res) return SRSLTE_ERROR_INVALID_INPUTS;
  const DlCtrlView v = dl_ctrl_view(q);
  if (nof_sf < 1 || nof_sf > v.cfg->max_batch || (nof_phich && !d_phich_res)) return SRSLTE_ERROR_INVALID_INPUTS;
  PhichRx* t = dl_ctrl_phich(q);
  if (int r = phich_prepare(*v.cfg, t, tti0, nof_sf, phich, nof_phich)) return r;
  if (nof_phich == 0) return SRSLTE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  if (int r = phich_upload(t, nof_phich, st)) return r;
  hipLaunchKernelGGL(dl_ctrl_ul_phich_kernel, dim3(ceil_div((int)nof_phich, PH_BLOCK)), dim3(256), 0, st, v.d_cand, v.d_ncand, 0, UlReqs(), 0, 0,
                     (srslte_hip_dl_ctrl_ul_res_t*)nullptr, (srslte_hip_dci_msg_t*)nullptr, (const cf32*)d_grid, (const cf32*)d_ce, (const float*)d_res,
                     tti0, phich_geom(v, t), t->req.dev<uint32_t>(), (int)nof_phich, d_phich_res, t->soft.get());
  LAUNCH_CHECK();
  return SRSLTE_SUCCESS;
}

int srslte_hip_dl_ctrl_batch_ul(srslte_hip_dl_ctrl_t* q, const void* d_grid, const void* d_ce, const void* d_res, uint32_t tti0, uint32_t nof_sf,
                                const srslte_hip_dl_ctrl_req_t* reqs, srslte_hip_dl_ctrl_res_t* d_out, srslte_hip_dci_msg_t* d_msg,
                                srslte_hip_dl_ctrl_ul_res_t* d_ul_out, srslte_hip_dci_msg_t* d_ul_msg, const srslte_hip_phich_req_t* phich,
                                uint32_t nof_phich, srslte_hip_phich_res_t* d_phich_res, void* stream)
{
  if (!d_grid || !d_ce || !d_res || !d_out || !d_msg || !d_ul_out || !d_ul_msg || (nof_phich && !d_phich_res)) return SRSLTE_ERROR_INVALID_INPUTS;
  if (int r = dl_ctrl_check(q, tti0, nof_sf, reqs)) return r;
  const DlCtrlView v = dl_ctrl_view(q);
  PhichRx*         t = dl_ctrl_phich(q);
  if (int r = phich_prepare(*v.cfg, t, tti0, nof_sf, phich, nof_phich)) return r;
  hipStream_t st = (hipStream_t)stream;
  if (nof_phich)
    if (int r = phich_upload(t, nof_phich, st)) return r;
  if (int r = srslte_hip_dl_ctrl_batch(q, d_grid, d_ce, d_res, tti0, nof_sf, reqs, d_out, d_msg, stream)) return r;
  const PhichGeom g = phich_geom(v, t);
  for (uint32_t s0 = 0; s0 < nof_sf; s0 += REQ_CHUNK) {
    const uint32_t n = nof_sf - s0 < (uint32_t)REQ_CHUNK ? nof_sf - s0 : (uint32_t)REQ_CHUNK;
    UlReqs         r;
    memset(&r, 0, sizeof(r));
    for (uint32_t i = 0; i < n; i++) r.rnti[i] = reqs[s0 + i].rnti;
    // the PHICHs depend on no subframe chunk: all of them ride in the first chunk's launch
    const int np = s0 == 0 ? (int)nof_phich : 0, ul_blocks = ceil_div((int)n, 256);
    hipLaunchKernelGGL(dl_ctrl_ul_phich_kernel, dim3(ul_blocks + ceil_div(np, PH_BLOCK)), dim3(256), 0, st, v.d_cand, v.d_ncand, (int)s0, r, (int)n,
                       ul_blocks, d_ul_out, d_ul_msg, (const cf32*)d_grid, (const cf32*)d_ce, (const float*)d_res, tti0, g,
                       t ? t->req.dev<uint32_t>() : nullptr, np, d_phich_res, t ? t->soft.get() : nullptr);
    LAUNCH_CHECK();
  }
  return SRSLTE_SUCCESS;
}

const void* srslte_hip_dl_ctrl_phich_debug_buffer(const srslte_hip_dl_ctrl_t* q)
{
  if (!q) return nullptr;
  const PhichRx* t = dl_ctrl_phich(q);
  return t ? t->soft.get() : nullptr;
}

} // extern "C"
