// DL control region transmit for gfx950 (include/srslte_hip/phy_hip.h, "DL control region transmit"): PCFICH, PHICH and PDCCH of a batch of
// subframes written into the caller's grids, two launches on the caller's stream:
//   dl_ctrl_tx_pcfich_phich_kernel  one workgroup per subframe: srslte_pcfich_encode (pcfich.c:231-275) and, one lane per (PHICH mapping unit,
//                                   symbol), srslte_regs_phich_reset + srslte_phich_encode + srslte_regs_phich_add of every PHICH of the
//                                   subframe in entry order (phich.c:318-430, regs.c:413-449)
//   dl_ctrl_tx_pdcch_kernel         one wavefront per DCI: srslte_pdcch_encode (pdcch.c:503-629) - CRC-16 with the RNTI mask, tail-biting
//                                   convolutional code, srslte_rm_conv_tx, scrambling, QPSK, layer mapping + precoding, the put on its CCEs
// Every value is the reference's exactly: the modulator levels, products with +-1 / +-j and the precoding's 1/sqrt(2), and the PHICH sums in
// entry order. The REG lists and sequences are built on the host when the object is made (ctrl_host.cpp); the per-call descriptors travel
// through a DescStage (dev_buf.hpp).
#include "common.hpp"
#include "ctrl_host.hpp"
#include "ctrl_tx_dev.hpp"
#include "dev_buf.hpp"
#include "phy_hip_internal.hpp"
#include <math.h>
#include <string.h>
#include <vector>

namespace {

constexpr int MAX_F = 128; // nof_bits + 16 < SRSLTE_DCI_MAX_BITS (pdcch.c:572-573)

struct CtrlTxGeom {
  const uint32_t* re;         // [16 PCFICH], then per REG variant [n[0]][n[1]][n[2]][units x 12 PHICH] RE indices into one port's [nsym][12 prb] grid
  const uint32_t* scr_pcfich; // [10] words: srslte_sequence_pcfich of each subframe (its first 12 bits are srslte_sequence_phich's)
  const uint32_t* scr_pdcch;  // [10][scr_words]
  int             scr_words;
  int             off[CTRL_MAX_VAR][3];                          // PDCCH REs of CFI 1-3 of each REG variant (ctrl_host.hpp)
  int             phich_off[CTRL_MAX_VAR], units[CTRL_MAX_VAR]; // its PHICH mapping units
  int             max_units;                                     // the descriptors' stride
  uint8_t         var[10];    // the variant of subframe sf_idx; CTRL_SF_UL: an uplink subframe of a TDD cell. FDD: all 0
  int             nof_ports, grid_len, cp_ext;
  float           s;          // srslte_precoding_diversity's scaling / sqrtf(2) with scaling 1.0f (precoding.c:1859, :1863)
};

struct DciTxDesc {
  uint32_t sf, cfi, L, ncce, nof_bits, rnti;
  uint32_t pay[4]; // payload bit i -> word i / 32, bit i % 32
};

// symbol m (0-11) of a PHICH entry before precoding, d0 of srslte_phich_encode: BPSK of the ack, times the orthogonal sequence nseq (36.211
// Table 6.9.1-2, w_normal / w_ext of phich.c:36-41), times c(m) of srslte_sequence_phich; on an extended-CP cell the six symbols of group
// 2m (odd = 0) fill the first, of 2m + 1 the second half of each REG, zero elsewhere (phich.c:392-407)
__device__ __forceinline__ cf32 phich_d0(uint32_t ent, int m, uint32_t scr, int ext)
{
  const uint32_t nseq = ent & 7, ack = (ent >> 3) & 1, odd = (ent >> 4) & 1;
  int            j = m;
  if (ext) {
    const int r = m & 3;
    if ((r < 2) == (odd != 0)) return make_float2(0.f, 0.f);
    j = 2 * (m >> 2) + (r & 1);
  }
  const float z  = ack ? -LVL : LVL; // both components of the BPSK symbol
  bool        neg, imag;             // w = (neg ? -1 : 1) (imag ? j : 1)
  if (ext) {
    imag = nseq >= 2;
    neg  = (nseq & 1) && (j & 1);
  } else {
    imag = nseq >= 4;
    const int q = nseq & 3, i = j & 3;
    neg = q == 1 ? (i & 1) : q == 2 ? (i >= 2) : q == 3 ? (i == 1 || i == 2) : false;
  }
  cf32 d = imag ? make_float2(-z, z) : make_float2(z, z); // j z = (-z.y, z.x)
  if (neg) d = make_float2(-d.x, -d.y);
  if ((scr >> j) & 1) d = make_float2(-d.x, -d.y);         // c_float = 1 - 2 c
  return d;
}

// grid = (nof_sf), 64 threads. desc: cfi [nof_sf] | ... | phich offsets [nof_sf units + 1] at ph_off | entries at ph_ent
__global__ __launch_bounds__(64) void dl_ctrl_tx_pcfich_phich_kernel(const uint32_t* __restrict__ desc, int ph_off, int ph_ent, uint32_t tti0,
                                                                     CtrlTxGeom g, cf32* __restrict__ grid)
{
  const int      b = blockIdx.x, tid = threadIdx.x, P = g.nof_ports, sf_idx = (tti0 + b) % 10, v = g.var[sf_idx];
  if (v == CTRL_SF_UL) return; // nothing is written
  const uint32_t cfi = desc[b], scr = g.scr_pcfich[sf_idx];
  cf32*          gb  = grid + (size_t)b * P * g.grid_len;
  if (tid < 16) {
    // PCFICH: bit j of the code word of CFI c is 0 where j % 3 == c - 1 (pcfich.c:39-47), scrambled, QPSK
    const int k = tid % P;
    cf32      x[4], y[4];
#pragma unroll
    for (int l = 0; l < 4; l++) {
      const int m = tid - k + l;
      x[l] = l < P ? qpsk(((2 * m) % 3 != (int)cfi - 1) ^ ((scr >> (2 * m)) & 1), ((2 * m + 1) % 3 != (int)cfi - 1) ^ ((scr >> (2 * m + 1)) & 1))
                   : make_float2(0.f, 0.f);
    }
    precode(P, k, x, g.s, y);
    const uint32_t re = g.re[tid];
#pragma unroll
    for (int p = 0; p < 4; p++)
      if (p < P) gb[(size_t)p * g.grid_len + re] = y[p];
  }
  const uint32_t* off = desc + ph_off + (size_t)b * g.max_units;
  for (int pos = tid; pos < 12 * g.units[v]; pos += 64) {
    const int u = pos / 12, i = pos - 12 * u, k = i % P;
    float     ar[4] = {0.f, 0.f, 0.f, 0.f}, ai[4] = {0.f, 0.f, 0.f, 0.f}; // srslte_regs_phich_reset
    for (uint32_t e = off[u]; e < off[u + 1]; e++) {
      const uint32_t ent = desc[ph_ent + e];
      cf32           x[4], y[4];
#pragma unroll
      for (int l = 0; l < 4; l++) x[l] = l < P ? phich_d0(ent, i - k + l, scr, g.cp_ext) : make_float2(0.f, 0.f);
      precode(P, k, x, g.s, y);
#pragma unroll
      for (int p = 0; p < 4; p++) ar[p] += y[p].x, ai[p] += y[p].y; // srslte_regs_phich_add, entry by entry
    }
    const uint32_t re = g.re[g.phich_off[v] + pos];
#pragma unroll
    for (int p = 0; p < 4; p++)
      if (p < P) gb[(size_t)p * g.grid_len + re] = make_float2(ar[p], ai[p]);
  }
}

// grid = (nof_dci), one wavefront per DCI
__global__ __launch_bounds__(64) void dl_ctrl_tx_pdcch_kernel(const DciTxDesc* __restrict__ dci, uint32_t tti0, CtrlTxGeom g, cf32* __restrict__ grid)
{
  __shared__ uint8_t bits[MAX_F], coded[3 * MAX_F], w[3 * MAX_F];
  const int        lane = threadIdx.x, P = g.nof_ports;
  const DciTxDesc* dc   = dci + blockIdx.x;
  const int        nb = (int)dc->nof_bits, F = nb + 16, E = 72 << dc->L, b = (int)dc->sf, sf_idx = (tti0 + b) % 10;
  const uint32_t   cfi = dc->cfi, ncce = dc->ncce, rnti = dc->rnti;
  for (int i = lane; i < nb; i += 64) bits[i] = (dc->pay[i >> 5] >> (i & 31)) & 1u;
  __syncthreads();
  // srslte_crc_attach (CRC-16 0x11021 over the message bits, written MSB first) and crc_set_mask_rnti (pdcch.c:490-506): every lane divides
  uint32_t r = 0;
  for (int i = 0; i < F; i++) {
    r = (r << 1) | (i < nb ? (uint32_t)bits[i] : 0u);
    if (r & 0x10000u) r ^= 0x11021u;
  }
  const uint32_t parity = (r ^ rnti) & 0xffffu;
  for (int i = nb + lane; i < F; i += 64) bits[i] = (parity >> (15 - (i - nb))) & 1u;
  __syncthreads();
  // srslte_convcoder_encode, tail biting (convcoder.c): output 3 i + j = parity(poly_j & the window input[i], input[i - 1], ... input[i - 6])
  for (int i = lane; i < F; i += 64) {
    uint32_t sr = 0;
    for (int k = 0; k < 7; k++) sr |= (uint32_t)bits[(i - k + F) % F] << k;
    coded[3 * i]     = __popc(sr & 0x6Du) & 1;
    coded[3 * i + 1] = __popc(sr & 0x4Fu) & 1;
    coded[3 * i + 2] = __popc(sr & 0x57u) & 1;
  }
  __syncthreads();
  // srslte_rm_conv_tx (rm_conv.c:44-89): the three sub-block interleaved streams read column by column with the dummy positions dropped (ballot
  // compaction); the circular read of E bits is then w[k mod 3F]
  const int nrows = (F - 1) / 32 + 1, Kp = nrows * 32, nd = Kp - F, W = 3 * Kp;
  int       base = 0;
  for (int j0 = 0; j0 < W; j0 += 64) {
    const int j = j0 + lane, s = j / Kp, rr = j - s * Kp, col = rr / nrows, row = rr - col * nrows, pos = row * 32 + RM_PERM_TX[col];
    const bool               valid = j < W && pos >= nd;
    const unsigned long long m     = __ballot(valid);
    if (valid) w[base + __popcll(m & ((1ull << lane) - 1ull))] = coded[(pos - nd) * 3 + s];
    base += __popcll(m);
  }
  __syncthreads();
  // scrambling from bit 72 ncce (pdcch.c:589), QPSK, precoding, srslte_regs_pdcch_put_offset on REs [36 ncce, 36 (ncce + 2^L)) of the CFI's list
  const uint32_t* cs  = g.scr_pdcch + (size_t)sf_idx * g.scr_words;
  const uint32_t* re  = g.re + g.off[g.var[sf_idx]][cfi - 1] + 36 * ncce; // the host refused DCIs in uplink subframes
  const int       e0  = 72 * (int)ncce, n3 = 3 * F;
  cf32*           gb  = grid + (size_t)b * P * g.grid_len;
  for (int q = lane; q < (E / 2) / P; q += 64) {
    cf32 x[4], y[4];
#pragma unroll
    for (int l = 0; l < 4; l++) {
      const int k0 = 2 * (q * P + l), k1 = k0 + 1, c0 = e0 + k0, c1 = e0 + k1;
      x[l] = l < P ? qpsk(w[k0 % n3] ^ ((cs[c0 >> 5] >> (c0 & 31)) & 1u), w[k1 % n3] ^ ((cs[c1 >> 5] >> (c1 & 31)) & 1u)) : make_float2(0.f, 0.f);
    }
#pragma unroll
    for (int l = 0; l < 4; l++) {
      if (l < P) {
        precode(P, l, x, g.s, y);
        const uint32_t k = re[q * P + l];
#pragma unroll
        for (int p = 0; p < 4; p++)
          if (p < P) gb[(size_t)p * g.grid_len + k] = y[p];
      }
    }
  }
}

srslte_hip_dl_ctrl_cfg_t rx_cfg(const srslte_hip_dl_ctrl_tx_cfg_t* c)
{
  srslte_hip_dl_ctrl_cfg_t r;
  memset(&r, 0, sizeof(r));
  r.nof_prb = c->nof_prb, r.nof_ports = c->nof_ports, r.cell_id = c->cell_id, r.cp_ext = c->cp_ext, r.phich_resources = c->phich_resources;
  r.phich_ext = c->phich_ext, r.tdd = c->tdd, r.nof_rx_antennas = 1, r.max_batch = 1;
  return r;
}

} // namespace

struct srslte_hip_dl_ctrl_tx {
  srslte_hip_dl_ctrl_tx_cfg_t cfg;
  CtrlTxGeom                  g;
  int                         tdd_sf_config = -1; // uplink-downlink configuration of a TDD object; -1: FDD
  int                         nof_cce[CTRL_MAX_VAR][3], max_cce = 0;
  uint32_t                    ngroups_m1 = 0;
  DevBuf<uint32_t>            re, scr;
  DescStage                   desc;
  std::vector<uint32_t>       words;   // the descriptor block of a call, as it is built
  std::vector<uint8_t>        used;    // CCEs taken, per subframe
  std::vector<uint32_t>       ph_unit; // per PHICH of the call: its mapping unit
  BcastTables*                bc = nullptr; // PSS / SSS / PBCH (pbch.hip)
};

namespace {

// The checks of srslte_hip_dl_ctrl_tx_put, and the descriptor block in q->words: cfi [nof_sf] | DciTxDesc [nof_dci] | PHICH offsets
// [nof_sf units + 1] (entries of subframe b, unit u: [off[b units + u], off[b units + u + 1])) | PHICH entries, nseq | ack << 3 | odd << 4,
// stable-sorted by (subframe, unit)
int ctrl_tx_prepare(srslte_hip_dl_ctrl_tx_t* q, uint32_t tti0, uint32_t nof_sf, const srslte_hip_dl_ctrl_tx_in_t* in, int* ph_off, int* ph_ent)
{
  const srslte_hip_dl_ctrl_tx_cfg_t& c = q->cfg;
  if (!in || nof_sf > c.max_batch || (nof_sf && !in->cfi) || in->nof_dci > c.max_dci || in->nof_phich > c.max_phich || (in->nof_dci && !in->dci) ||
      (in->nof_phich && !in->phich))
    return SRSLTE_ERROR_INVALID_INPUTS;
  const uint32_t U = (uint32_t)q->g.max_units, maxcce = (uint32_t)q->max_cce;
  const bool     tdd = q->tdd_sf_config >= 0;
  auto           var_of = [&](uint32_t sf) { return q->g.var[(tti0 + sf) % 10]; };
  std::vector<uint32_t>& w = q->words;
  w.assign(nof_sf + (size_t)in->nof_dci * (sizeof(DciTxDesc) / 4) + (size_t)nof_sf * U + 1 + in->nof_phich, 0u);
  for (uint32_t b = 0; b < nof_sf; b++) {
    if (var_of(b) == CTRL_SF_UL) continue; // in->cfi[b] is not looked at
    const uint32_t sf_idx = (tti0 + b) % 10;
    if (in->cfi[b] < 1 || in->cfi[b] > 3 || (tdd && in->cfi[b] == 3 && (sf_idx == 1 || sf_idx == 6))) return SRSLTE_ERROR_INVALID_INPUTS;
    w[b] = in->cfi[b];
  }
  q->used.assign((size_t)nof_sf * maxcce, 0);
  auto* dd = reinterpret_cast<DciTxDesc*>(w.data() + nof_sf);
  for (uint32_t i = 0; i < in->nof_dci; i++) {
    const srslte_hip_dl_ctrl_tx_dci_t& d = in->dci[i];
    const srslte_hip_dci_msg_t&        m = d.msg;
    if (d.sf >= nof_sf || m.L > 3 || m.nof_bits == 0 || m.nof_bits >= 128 - 16 || var_of(d.sf) == CTRL_SF_UL) return SRSLTE_ERROR_INVALID_INPUTS;
    const uint32_t cfi = in->cfi[d.sf], n = 1u << m.L, cces = (uint32_t)q->nof_cce[var_of(d.sf)][cfi - 1];
    if (m.ncce > cces || m.ncce + n > cces) return SRSLTE_ERROR_INVALID_INPUTS;
    uint8_t* u = q->used.data() + (size_t)d.sf * maxcce + m.ncce;
    for (uint32_t k = 0; k < n; k++) {
      if (u[k]) return SRSLTE_ERROR_INVALID_INPUTS; // two DCIs on one CCE: the reference would overwrite the first, here it is refused
      u[k] = 1;
    }
    DciTxDesc& t = dd[i];
    t.sf = d.sf, t.cfi = cfi, t.L = m.L, t.ncce = m.ncce, t.nof_bits = m.nof_bits, t.rnti = m.rnti;
    for (uint32_t k = 0; k < m.nof_bits; k++) t.pay[k >> 5] |= (uint32_t)(m.payload[k] & 1) << (k & 31);
  }
  const size_t o_off = nof_sf + (size_t)in->nof_dci * (sizeof(DciTxDesc) / 4), o_ent = o_off + (size_t)nof_sf * U + 1;
  q->ph_unit.resize(in->nof_phich);
  for (uint32_t i = 0; i < in->nof_phich; i++) {
    const srslte_hip_phich_tx_t& p = in->phich[i];
    uint32_t                     ngroup, nseq;
    if (p.sf >= nof_sf || p.ack > 1 || p.I_phich > 1) return SRSLTE_ERROR_INVALID_INPUTS;
    // TDD: the subframe's own group count, mi ngroups_m1 - none in an uplink subframe or with mi = 0, and I_phich = 1 only where mi = 2
    if (var_of(p.sf) == CTRL_SF_UL) return SRSLTE_ERROR_INVALID_INPUTS;
    phich_calc(q->ngroups_m1, c.cp_ext, p.n_prb_lowest, p.n_dmrs, p.I_phich, &ngroup, &nseq);
    if (ngroup >= (uint32_t)q->g.units[var_of(p.sf)] * (c.cp_ext ? 2u : 1u)) return SRSLTE_ERROR_INVALID_INPUTS;
    const uint32_t unit = c.cp_ext ? ngroup / 2 : ngroup, key = p.sf * U + unit;
    q->ph_unit[i] = nseq | (uint32_t)p.ack << 3 | (c.cp_ext ? (ngroup & 1) << 4 : 0u) | key << 8;
    w[o_off + key + 1]++;
  }
  for (size_t k = 0; k < (size_t)nof_sf * U; k++) w[o_off + k + 1] += w[o_off + k]; // counts -> offsets
  std::vector<uint32_t> fill(w.begin() + o_off, w.begin() + o_ent - 1);
  for (uint32_t i = 0; i < in->nof_phich; i++) w[o_ent + fill[q->ph_unit[i] >> 8]++] = q->ph_unit[i] & 0xffu; // stable: entry order kept
  *ph_off = (int)o_off, *ph_ent = (int)o_ent;
  return SRSLTE_SUCCESS;
}

} // namespace

int dl_ctrl_tx_check(srslte_hip_dl_ctrl_tx_t* q, uint32_t tti0, uint32_t nof_sf, const srslte_hip_dl_ctrl_tx_in_t* in)
{
  int a, b;
  return q ? ctrl_tx_prepare(q, tti0, nof_sf, in, &a, &b) : SRSLTE_ERROR_INVALID_INPUTS;
}

int dl_ctrl_tx_tdd_sf_config(const srslte_hip_dl_ctrl_tx_t* q) { return q ? q->tdd_sf_config : -1; }

bool dl_ctrl_tx_is_uplink(const srslte_hip_dl_ctrl_tx_t* q, uint32_t tti) { return q && q->g.var[tti % 10] == CTRL_SF_UL; }

const srslte_hip_dl_ctrl_tx_cfg_t* dl_ctrl_tx_cfg(const srslte_hip_dl_ctrl_tx_t* q) { return q ? &q->cfg : nullptr; }

const BcastTables* dl_ctrl_tx_bcast(const srslte_hip_dl_ctrl_tx_t* q) { return q ? q->bc : nullptr; }

extern "C" {

void srslte_hip_dl_ctrl_tx_destroy(srslte_hip_dl_ctrl_tx_t* q)
{
  if (!q) return;
  bcast_tables_destroy(q->bc);
  delete q;
}

// tdd_sf_config < 0: FDD
static srslte_hip_dl_ctrl_tx_t* dl_ctrl_tx_make(const srslte_hip_dl_ctrl_tx_cfg_t* cfg, int tdd_sf_config)
{
  if (!cfg || cfg->max_batch < 1) return nullptr;
  const srslte_hip_dl_ctrl_cfg_t rc = rx_cfg(cfg);
  CtrlRegsSet                    set;
  if (!ctrl_cell_ok(&rc) || ctrl_build_regs_set(&rc, tdd_sf_config, set) != SRSLTE_SUCCESS) return nullptr;
  auto* q = new srslte_hip_dl_ctrl_tx_t();
  q->cfg           = *cfg;
  q->tdd_sf_config = tdd_sf_config;
  q->ngroups_m1    = set.v[0].ngroups_m1;
  CtrlTxGeom& g    = q->g;
  memset(&g, 0, sizeof(g));
  memset(q->nof_cce, 0, sizeof(q->nof_cce));
  std::vector<uint32_t> re(set.v[0].pcfich); // the PCFICH REGs are the same in every variant
  for (size_t v = 0; v < set.v.size(); v++) {
    const CtrlRegs& regs = set.v[v];
    for (int c = 0; c < 3; c++) {
      g.off[v][c] = (int)re.size(), q->nof_cce[v][c] = (int)regs.pdcch[c].size() / 36;
      re.insert(re.end(), regs.pdcch[c].begin(), regs.pdcch[c].end());
    }
    g.phich_off[v] = (int)re.size(), g.units[v] = (int)regs.units;
    re.insert(re.end(), regs.phich.begin(), regs.phich.end());
  }
  memcpy(g.var, set.var, sizeof(g.var));
  g.max_units = (int)set.max_units();
  q->max_cce  = (int)set.max_pdcch_re / 36;
  g.nof_ports = (int)cfg->nof_ports;
  g.grid_len  = (cfg->cp_ext ? 12 : 14) * 12 * (int)cfg->nof_prb;
  g.cp_ext    = cfg->cp_ext ? 1 : 0;
  g.s         = 1.0f / sqrtf(2.0f);
  std::vector<uint32_t> scr;
  ctrl_scrambling(cfg->cell_id, 72 * (uint32_t)q->max_cce, scr, &g.scr_words);
  const size_t desc_bytes = 4 * ((size_t)cfg->max_batch + (size_t)cfg->max_dci * (sizeof(DciTxDesc) / 4) + (size_t)cfg->max_batch * g.max_units + 1 + cfg->max_phich);
  if (q->re.upload(re) || q->scr.upload(scr) || q->desc.init(desc_bytes) ||
      !(q->bc = bcast_tables_create(&rc, cfg->phich_ext, cfg->phich_resources, false))) {
    hip_log("[srslte_hip] srslte_hip_dl_ctrl_tx_create: device allocation failed\n");
    srslte_hip_dl_ctrl_tx_destroy(q);
    return nullptr;
  }
  g.re = q->re.get(), g.scr_pcfich = q->scr.get(), g.scr_pdcch = q->scr.get() + 10;
  return q;
}

srslte_hip_dl_ctrl_tx_t* srslte_hip_dl_ctrl_tx_create(const srslte_hip_dl_ctrl_tx_cfg_t* cfg) { return cfg && !cfg->tdd ? dl_ctrl_tx_make(cfg, -1) : nullptr; }

srslte_hip_dl_ctrl_tx_t* srslte_hip_dl_ctrl_tx_create_tdd(const srslte_hip_dl_ctrl_tx_cfg_t* cfg, uint32_t tdd_sf_config)
{
  return cfg && cfg->tdd == 1 && tdd_sf_config <= 6 ? dl_ctrl_tx_make(cfg, (int)tdd_sf_config) : nullptr;
}

int srslte_hip_dl_ctrl_tx_put(srslte_hip_dl_ctrl_tx_t* q, uint32_t tti0, uint32_t nof_sf, const srslte_hip_dl_ctrl_tx_in_t* in, void* d_grid, void* stream)
{
  int ph_off = 0, ph_ent = 0;
  if (!q || !d_grid) return SRSLTE_ERROR_INVALID_INPUTS;
  if (int r = ctrl_tx_prepare(q, tti0, nof_sf, in, &ph_off, &ph_ent)) return r;
  if (nof_sf == 0) return SRSLTE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  uint32_t*   h  = nullptr;
  if (int r = q->desc.begin(&h)) return r;
  const size_t bytes = q->words.size() * 4;
  memcpy(h, q->words.data(), bytes);
  if (int r = q->desc.commit(bytes, st)) return r;
  hipLaunchKernelGGL(dl_ctrl_tx_pcfich_phich_kernel, dim3(nof_sf), dim3(64), 0, st, q->desc.dev<uint32_t>(), ph_off, ph_ent, tti0, q->g, (cf32*)d_grid);
  LAUNCH_CHECK();
  if (in->nof_dci) {
    hipLaunchKernelGGL(dl_ctrl_tx_pdcch_kernel, dim3(in->nof_dci), dim3(64), 0, st, (const DciTxDesc*)(q->desc.dev<uint32_t>() + nof_sf), tti0, q->g, (cf32*)d_grid);
    LAUNCH_CHECK();
  }
  return SRSLTE_SUCCESS;
}

int srslte_hip_dl_ctrl_phich_ngroups(const srslte_hip_dl_ctrl_tx_cfg_t* cfg)
{
  if (!cfg) return SRSLTE_ERROR_INVALID_INPUTS;
  const srslte_hip_dl_ctrl_cfg_t rc = rx_cfg(cfg);
  CtrlRegs                       regs;
  if (int r = ctrl_build_regs(&rc, regs)) return r;
  return (int)regs.ngroups_m1 * (cfg->cp_ext ? 2 : 1);
}

// the REG lists of subframe sf_idx of a TDD cell; < 0 for an uplink subframe, an invalid configuration or cell
static int tdd_regs(const srslte_hip_dl_ctrl_tx_cfg_t* cfg, uint32_t tdd_sf_config, uint32_t sf_idx, CtrlRegs& regs)
{
  const int mi = ctrl_tdd_mi(tdd_sf_config, sf_idx);
  if (!cfg || mi < 0) return SRSLTE_ERROR_INVALID_INPUTS;
  const srslte_hip_dl_ctrl_cfg_t rc = rx_cfg(cfg);
  return ctrl_build_regs_opts(&rc, (uint32_t)mi, sf_idx == 1 || sf_idx == 6, regs);
}

int srslte_hip_dl_ctrl_phich_ngroups_tdd(const srslte_hip_dl_ctrl_tx_cfg_t* cfg, uint32_t tdd_sf_config, uint32_t sf_idx)
{
  if (!cfg) return SRSLTE_ERROR_INVALID_INPUTS;
  const srslte_hip_dl_ctrl_cfg_t rc = rx_cfg(cfg);
  CtrlRegsSet                    set;
  CtrlRegs                       regs;
  if (int r = tdd_regs(cfg, tdd_sf_config, sf_idx, regs)) return r;
  if (int r = ctrl_build_regs_set(&rc, (int)tdd_sf_config, set)) return r; // SRSLTE_ERROR: the creators refuse the cell and configuration (ctrl_host.hpp)
  return (int)regs.units * (cfg->cp_ext ? 2 : 1);
}

int srslte_hip_dl_ctrl_phich_re_tdd(const srslte_hip_dl_ctrl_tx_cfg_t* cfg, uint32_t tdd_sf_config, uint32_t sf_idx, uint32_t ngroup, uint32_t* re, uint32_t max)
{
  CtrlRegs regs;
  if (int r = tdd_regs(cfg, tdd_sf_config, sf_idx, regs)) return r;
  const uint32_t unit = cfg->cp_ext ? ngroup / 2 : ngroup;
  if (unit >= regs.units || !re || max < 12) return SRSLTE_ERROR_INVALID_INPUTS;
  memcpy(re, regs.phich.data() + 12 * unit, 12 * 4);
  return 12;
}

int srslte_hip_phich_calc(const srslte_hip_dl_ctrl_tx_cfg_t* cfg, uint32_t n_prb_lowest, uint32_t n_dmrs, uint32_t I_phich, uint32_t* ngroup, uint32_t* nseq)
{
  if (!cfg || !ngroup || !nseq) return SRSLTE_ERROR_INVALID_INPUTS;
  const srslte_hip_dl_ctrl_cfg_t rc = rx_cfg(cfg);
  CtrlRegs                       regs;
  if (int r = ctrl_build_regs(&rc, regs)) return r;
  phich_calc(regs.ngroups_m1, cfg->cp_ext, n_prb_lowest, n_dmrs, I_phich, ngroup, nseq);
  return SRSLTE_SUCCESS;
}

int srslte_hip_dl_ctrl_phich_re(const srslte_hip_dl_ctrl_tx_cfg_t* cfg, uint32_t ngroup, uint32_t* re, uint32_t max)
{
  if (!cfg) return SRSLTE_ERROR_INVALID_INPUTS;
  const srslte_hip_dl_ctrl_cfg_t rc = rx_cfg(cfg);
  CtrlRegs                       regs;
  if (int r = ctrl_build_regs(&rc, regs)) return r;
  const uint32_t unit = cfg->cp_ext ? ngroup / 2 : ngroup;
  if (unit >= regs.ngroups_m1 || !re || max < 12) return SRSLTE_ERROR_INVALID_INPUTS;
  memcpy(re, regs.phich.data() + 12 * unit, 12 * 4);
  return 12;
}

} // extern "C"
