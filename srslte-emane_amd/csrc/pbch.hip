// Broadcast channels for gfx950 (include/srslte_hip/phy_hip.h, "DL broadcast"): PSS, SSS and PBCH of a batch of subframes on the eNB side,
// the MIB of every subframe 0 of a batch on the UE side, one launch each on the caller's stream:
//   dl_bcast_tx_kernel  one wavefront per subframe, at once done outside subframes 0 and 5: put_sync of srslte_enb_dl_put_base
//                       (enb_dl.c:297-307) on every port, and in subframe 0 put_mib (:324-335) - srslte_pbch_mib_pack, CRC-16 with the
//                       port mask, tail-biting convolutional code, srslte_rm_conv_tx, then the quarter sfn % 4 scrambled, QPSK, layer
//                       mapping + precoding and srslte_pbch_put (srslte_pbch_encode, pbch.c:554-607)
//   dl_mib_kernel       one workgroup per subframe, at once done outside subframe 0: srslte_pbch_decode right after
//                       srslte_pbch_decode_reset (pbch.c:441-550) - the LLR rows of every port count tried in LDS, then one wavefront per
//                       quarter dst runs decode_frame(0, dst, 1) (:393-431) for each of them; the first hit in the reference's order wins
// The RE list, the PSS / SSS values and the scrambling sequence are built on the host when an object is made (ctrl_host.cpp).
#include "common.hpp"
#include "ctrl_host.hpp"
#include "ctrl_rx_dev.hpp"
#include "ctrl_tx_dev.hpp"
#include "demod_dev.hpp"
#include "dev_buf.hpp"
#include "phy_hip_internal.hpp"
#include "viterbi_dev.hpp"
#include <math.h>
#include <string.h>
#include <vector>

namespace {

constexpr int MIB_F    = 40;  // SRSLTE_BCH_PAYLOADCRC_LEN
constexpr int MIB_E    = 120; // SRSLTE_BCH_ENCODED_LEN
constexpr int MAX_BITS = 480; // nof_bits of a normal-CP cell (432 extended)

struct BcastGeom {
  const uint32_t* re;   // [nof_bits / 2] the PBCH REs of one port's subframe grid, srslte_pbch_put order
  const uint32_t* scr;  // srslte_sequence_pbch, 4 nof_bits bits
  const float*    sync; // [72][2] PSS with its guards, then [2][72] SSS of subframe 0 / 5 (real parts)
  // first RE of the PSS / SSS with their guards. FDD: both in slot 0 of subframes 0 and 5. TDD: the PSS in symbol 2 of subframes 1 and 6, the
  // SSS in the last symbol of subframes 0 and 5
  uint32_t        pss_k0, sss_k0;
  int             tdd;
  int             nof_ports, grid_len, nof_bits;
  uint32_t        mib_head; // bandwidth, PHICH length and resources: the first 6 bits of the MIB
  float           s;        // srslte_precoding_diversity's 1/sqrtf(2) (scaling 1.0f)
};

// srslte_crc_mask of srslte_crc_set_mask (pbch.c:42-46) for 1 / 2 / 4 ports, as the 16-bit parity word (first CRC bit = MSB)
__host__ __device__ inline uint32_t crc_port_mask(int nant) { return nant == 2 ? 0xFFFFu : nant == 4 ? 0x5555u : 0u; }

// grid = (nof_sf), 64 threads
__global__ __launch_bounds__(64) void dl_bcast_tx_kernel(uint32_t tti0, BcastGeom g, cf32* __restrict__ grid)
{
  __shared__ uint8_t bits[MIB_F], coded[MIB_E], w[MIB_E];
  const int      b = blockIdx.x, lane = threadIdx.x, P = g.nof_ports;
  const uint32_t t = tti0 + (uint32_t)b, sf_idx = t % 10;
  const bool     sss_sf = sf_idx == 0 || sf_idx == 5, pss_sf = g.tdd ? (sf_idx == 1 || sf_idx == 6) : sss_sf;
  if (!sss_sf && !pss_sf) return;
  cf32* gb = grid + (size_t)b * P * g.grid_len;
  // srslte_pss_put_slot / srslte_sss_put_slot on every port (pss.c:380-386, sss.c:106-119)
  for (int i = lane; i < 72; i += 64) {
    const cf32 pss = make_float2(g.sync[2 * i], g.sync[2 * i + 1]), sss = make_float2(g.sync[144 + (sf_idx ? 72 : 0) + i], 0.f);
    for (int p = 0; p < P; p++) {
      if (pss_sf) gb[(size_t)p * g.grid_len + g.pss_k0 + i] = pss;
      if (sss_sf) gb[(size_t)p * g.grid_len + g.sss_k0 + i] = sss;
    }
  }
  if (sf_idx != 0) return;
  // srslte_pbch_mib_pack (pbch.c:318-354): 6 bits of the cell, the 8 high bits of the SFN, 10 zeros
  const uint32_t sfn = t / 10, mib = g.mib_head << 18 | ((sfn >> 2) & 0xffu) << 10;
  if (lane < 24) bits[lane] = (mib >> (23 - lane)) & 1u;
  __syncthreads();
  // srslte_crc_attach + srslte_crc_set_mask with the cell's port count: every lane divides
  uint32_t r = 0;
  for (int i = 0; i < MIB_F; i++) {
    r = (r << 1) | (i < 24 ? (uint32_t)bits[i] : 0u);
    if (r & 0x10000u) r ^= 0x11021u;
  }
  const uint32_t parity = (r ^ crc_port_mask(P)) & 0xffffu;
  if (lane >= 24 && lane < MIB_F) bits[lane] = (parity >> (15 - (lane - 24))) & 1u;
  __syncthreads();
  // srslte_convcoder_encode, tail biting, as dl_ctrl_tx_pdcch_kernel
  if (lane < MIB_F) {
    uint32_t sr = 0;
    for (int k = 0; k < 7; k++) sr |= (uint32_t)bits[(lane - k + MIB_F) % MIB_F] << k;
    coded[3 * lane]     = __popc(sr & 0x6Du) & 1;
    coded[3 * lane + 1] = __popc(sr & 0x4Fu) & 1;
    coded[3 * lane + 2] = __popc(sr & 0x57u) & 1;
  }
  __syncthreads();
  // srslte_rm_conv_tx to 4 nof_bits: the compacted interleaved streams w read circularly
  constexpr int nrows = (MIB_F - 1) / 32 + 1, Kp = nrows * 32, nd = Kp - MIB_F, W = 3 * Kp;
  int           base = 0;
  for (int j0 = 0; j0 < W; j0 += 64) {
    const int j = j0 + lane, s = j / Kp, rr = j - s * Kp, col = rr / nrows, row = rr - col * nrows, pos = row * 32 + RM_PERM_TX[col];
    const bool               valid = j < W && pos >= nd;
    const unsigned long long m     = __ballot(valid);
    if (valid) w[base + __popcll(m & ((1ull << lane) - 1ull))] = coded[(pos - nd) * 3 + s];
    base += __popcll(m);
  }
  __syncthreads();
  // the quarter frame_idx = sfn % 4: srslte_scrambling_b_offset from bit frame_idx nof_bits, QPSK, precoding, srslte_pbch_put on every port
  const int nb = g.nof_bits, e0 = (int)(sfn % 4) * nb;
  for (int q = lane; q < (nb / 2) / P; q += 64) {
    cf32 x[4], y[4];
#pragma unroll
    for (int l = 0; l < 4; l++) {
      const int k0 = 2 * (q * P + l), k1 = k0 + 1, c0 = e0 + k0, c1 = e0 + k1;
      x[l] = l < P ? qpsk(w[c0 % MIB_E] ^ ((g.scr[c0 >> 5] >> (c0 & 31)) & 1u), w[c1 % MIB_E] ^ ((g.scr[c1 >> 5] >> (c1 & 31)) & 1u))
                   : make_float2(0.f, 0.f);
    }
#pragma unroll
    for (int l = 0; l < 4; l++) {
      if (l < P) {
        precode(P, l, x, g.s, y);
        const uint32_t k = g.re[q * P + l];
#pragma unroll
        for (int p = 0; p < 4; p++)
          if (p < P) gb[(size_t)p * g.grid_len + k] = y[p];
      }
    }
  }
}

// grid = (nof_sf), 256 threads: wavefront dst decodes quarter dst
__global__ __launch_bounds__(256) void dl_mib_kernel(const cf32* __restrict__ grid, const cf32* __restrict__ ce, const float* __restrict__ res,
                                                     uint32_t tti0, int all_ports, int nof_rx, BcastGeom g, float* __restrict__ llr,
                                                     srslte_hip_mib_cand_t* __restrict__ cand, srslte_hip_mib_res_t* __restrict__ out)
{
  __shared__ float              row[3][MAX_BITS];
  __shared__ float              tmp[4][3 * 64], rmf[4][MIB_E];
  __shared__ uint16_t           us[4][MIB_E];
  __shared__ unsigned long long dec[4][MIB_E + 6];
  __shared__ uint8_t            bits[4][MIB_E];
  __shared__ uint8_t            hit[3][4], pay[3][4][24];
  const int             b = blockIdx.x, tid = threadIdx.x, P = g.nof_ports, glen = g.grid_len, nb = g.nof_bits, ns = nb / 2;
  const uint32_t        t = tti0 + (uint32_t)b;
  srslte_hip_mib_res_t* o = out + b;
  if (t % 10 != 0) {
    if (tid == 0) {
      o->found = 0, o->nof_tx_ports = 0, o->sfn_offset = 0, o->nof_prb = 0, o->phich_ext = 0, o->phich_resources = 0, o->sfn = 0;
      for (int i = 0; i < 24; i++) o->payload[i] = 0;
    }
    return;
  }
  // srslte_pbch_get of slot 1 on receive antenna 0 and the estimates ce[p][0]
  const cf32* y = grid + (size_t)b * nof_rx * glen;
  const cf32* h[4];
  for (int p = 0; p < 4; p++) h[p] = ce + ((size_t)b * P + (p < P ? p : 0)) * nof_rx * glen;
  const float noise = res[(size_t)b * 10]; // srslte_hip_chest_dl_res_t.noise_estimate
  // the port counts tried (pbch.c:499-546): 1, 2, 4 up to the cell's, or the cell's alone; slot s holds nant 1 << s
  int tm = 0;
  for (int s = 0; s < 3; s++) tm |= ((1 << s) <= P && (all_ports || (1 << s) == P)) << s;
  auto tried = [tm](int s) { return (tm >> s) & 1; };
  const int n16 = 16 * (ns / 16);
  for (int s = 0; s < 3; s++) {
    float* grow = llr + ((size_t)b * 3 + s) * MAX_BITS;
    if (!tried(s)) {
      for (int i = tid; i < MAX_BITS; i += 256) grow[i] = 0.f;
      continue;
    }
    const int nant = 1 << s;
    for (int q = tid; q < ns / nant; q += 256) {
      cf32 x[4];
      if (nant == 1) {
        // srslte_predecoding_single with noise_estimate itself: the AVX body over 16 (n / 16) symbols, the generic tail behind
        x[0] = q < n16 ? eq_single_avx(y, h[0], 1, glen, g.re[q], noise) : eq_single_gen(y, h[0], 1, glen, g.re[q], noise);
      } else if (nant == 2) {
        eq_div2(y, h[0], h[1], 1, glen, g.re[2 * q], g.re[2 * q + 1], false, x); // > 32 symbols, a multiple of 4: the SSE path alone
      } else {
        eq_div4(y, h, 1, glen, g.re + 4 * q, x);
      }
#pragma unroll
      for (int l = 0; l < 4; l++) {
        if (l < nant) {
          const int i = nant * q + l; // srslte_layerdemap_diversity
          float     v[8];
          demod_dev::demod_f(demod_dev::MOD_QPSK, x[l], v);
          row[s][2 * i] = v[0], row[s][2 * i + 1] = v[1];
          grow[2 * i] = v[0], grow[2 * i + 1] = v[1];
        }
      }
    }
    for (int i = nb + tid; i < MAX_BITS; i += 256) grow[i] = 0.f;
  }
  __syncthreads();
  const int wv = tid >> 6, lane = tid & 63, dst = wv;
  for (int s = 0; s < 3; s++) {
    if (!tried(s)) continue; // the same for every wavefront: the barriers below stay matched
    // decode_frame(src 0, dst, n 1): the row descrambled at offset dst nof_bits into quarter dst, SRSLTE_RX_NULL elsewhere, srslte_rm_conv_rx
    // to 120 with the reference's combining order (as dl_ctrl_dci_kernel), times 1 / 2
    constexpr int nrows = (MIB_F - 1) / 32 + 1, Kp = nrows * 32, nd = Kp - MIB_F, W = 3 * Kp;
    const int     lo = dst * nb, hi = lo + nb, E = 4 * nb;
    int           base = 0;
    for (int j0 = 0; j0 < W; j0 += 64) {
      const int                j = j0 + lane, rr = j % Kp, di = rr / nrows, dj = rr % nrows;
      const bool               valid = j < W && dj * 32 + RM_PERM[di] >= nd;
      const unsigned long long m     = __ballot(valid);
      const int                rank  = base + __popcll(m & ((1ull << lane) - 1ull));
      if (j < W) {
        float acc = RX_NULL;
        if (valid) {
          for (int k = rank; k < E; k += MIB_E) {
            const float v = (k >= lo && k < hi) ? (scr_bit(g.scr, k) ? -row[s][k - lo] : row[s][k - lo]) : RX_NULL;
            if (acc == RX_NULL) {
              acc = v;
            } else if (v != RX_NULL) {
              acc += v;
            }
          }
        }
        tmp[wv][j] = acc;
      }
      base += __popcll(m);
    }
    __syncthreads();
    for (int i = lane; i < MIB_E; i += 64) {
      const int   ii = i / 3, sidx = i - 3 * ii, di = (ii + nd) / 32, dj = (ii + nd) % 32;
      const float v = tmp[wv][Kp * sidx + RM_PERM_INV[dj] * nrows + di];
      rmf[wv][i]    = (v != RX_NULL ? v : 0.f) * 0.5f;
    }
    for (int i = MIB_E + lane; i < MIB_E + 6; i += 64) dec[wv][i] = 0ull;
    __syncthreads();
    viterbi_dev::quant_fus(rmf[wv], us[wv], MIB_E, lane);
    viterbi_dev::decode37_tb(us[wv], dec[wv], bits[wv], MIB_F, lane);
    __syncthreads();
    // srslte_pbch_crc_check (pbch.c:373-391): CRC with the port mask, and a payload that is not all zeros
    const uint8_t*         msg = bits[wv] + MIB_F;
    srslte_hip_mib_cand_t* c   = cand + ((size_t)b * 3 + s) * 4 + dst;
    if (lane < MIB_F) c->data[lane] = msg[lane];
    if (lane < 24) pay[s][dst][lane] = msg[lane];
    if (lane == 0) {
      uint32_t p = 0, nz = 0;
      for (int i = 0; i < 16; i++) p = (p << 1) | msg[24 + i];
      for (int i = 0; i < 24; i++) nz |= msg[i];
      const int ok = (p ^ crc_port_mask(1 << s)) == crc16(msg, 24) && nz;
      hit[s][dst] = (uint8_t)ok;
      c->nant = 1u << s, c->dst = (uint32_t)dst, c->hit = (uint32_t)ok;
    }
  }
  if (tid < 12 && !tried(tid / 4)) {
    srslte_hip_mib_cand_t* c = cand + ((size_t)b * 3 + tid / 4) * 4 + tid % 4;
    c->nant = 0, c->dst = 0, c->hit = 0;
    for (int i = 0; i < MIB_F; i++) c->data[i] = 0;
  }
  __syncthreads();
  if (tid == 0) {
    int ws = -1, wd = 0;
    for (int s = 0; s < 3 && ws < 0; s++)
      for (int d = 0; d < 4 && ws < 0; d++)
        if (tried(s) && hit[s][d]) ws = s, wd = d;
    const uint8_t* v = pay[ws >= 0 ? ws : 0][wd];
    for (int i = 0; i < 24; i++) o->payload[i] = ws >= 0 ? v[i] : 0;
    o->found        = ws >= 0 ? 1 : 0;
    o->nof_tx_ports = ws >= 0 ? 1u << ws : 0;
    o->sfn_offset   = ws >= 0 ? wd : 0;
    // srslte_pbch_mib_unpack (pbch.c:269-308) and srsue's (sfn + sfn_offset) % 1024
    const uint32_t bw = ws >= 0 ? (uint32_t)(v[0] << 2 | v[1] << 1 | v[2]) : 0;
    uint32_t       sfn = 0;
    for (int i = 6; i < 14; i++) sfn = sfn << 1 | (ws >= 0 ? v[i] : 0u);
    o->nof_prb         = ws < 0 ? 0 : bw == 0 ? 6 : bw == 1 ? 15 : (bw - 1) * 25;
    o->phich_ext       = ws >= 0 ? v[3] : 0;
    o->phich_resources = ws >= 0 ? (uint32_t)(v[4] << 1 | v[5]) : 0;
    o->sfn             = ws >= 0 ? ((sfn << 2) + (uint32_t)wd) % 1024 : 0;
  }
}

} // namespace

struct BcastTables {
  BcastGeom g;
  DevBuf<uint32_t> tab; // RE list, then the scrambling words
  DevBuf<float>    sync;
  DevBuf<float>    llr;  // receive: [max_batch][3][MAX_BITS]
  DevBuf<srslte_hip_mib_cand_t> cand; // receive: [max_batch][3][4]
  uint32_t  max_batch = 0;
  int       nof_rx = 1;
};

void bcast_tables_destroy(BcastTables* t) { delete t; }

BcastTables* bcast_tables_create(const srslte_hip_dl_ctrl_cfg_t* c, int phich_ext, int phich_resources, bool rx)
{
  if (!ctrl_cell_ok(c)) return nullptr;
  BcastHost h;
  bcast_build(c->nof_prb, c->cell_id, c->cp_ext, h);
  auto* t = new BcastTables();
  std::vector<uint32_t> tab(h.pbch_re);
  tab.insert(tab.end(), h.scr.begin(), h.scr.end());
  float sync[288];
  memcpy(sync, h.pss, sizeof(h.pss));
  memcpy(sync + 144, h.sss, sizeof(h.sss));
  t->max_batch = rx ? c->max_batch : 0;
  t->nof_rx    = (int)c->nof_rx_antennas;
  if (t->tab.upload(tab) || t->sync.upload(sync, sizeof(sync) / sizeof(sync[0])) ||
      (rx && (t->llr.alloc((size_t)c->max_batch * 3 * MAX_BITS) || t->cand.alloc((size_t)c->max_batch * 12)))) {
    hip_log("[srslte_hip] broadcast tables: device allocation failed\n");
    delete t;
    return nullptr;
  }
  BcastGeom& g = t->g;
  g.re = t->tab.get(), g.scr = t->tab.get() + h.pbch_re.size(), g.sync = t->sync.get();
  g.pss_k0 = h.pss_k0, g.sss_k0 = h.sss_k0;
  g.tdd = c->tdd ? 1 : 0;
  if (g.tdd) { // the positions sync.c:732-809 searches: PSS on symbol 2 of subframes 1 and 6, SSS on the last symbol of subframes 0 and 5
    const uint32_t w = 12 * c->nof_prb, nsym = c->cp_ext ? 6 : 7;
    g.pss_k0 = 2 * w + w / 2 - 36, g.sss_k0 = (2 * nsym - 1) * w + w / 2 - 36;
  }
  g.nof_ports = (int)c->nof_ports, g.grid_len = (c->cp_ext ? 12 : 14) * 12 * (int)c->nof_prb, g.nof_bits = (int)h.nof_bits;
  g.mib_head = mib_head(c->nof_prb, phich_ext, phich_resources);
  g.s        = 1.0f / sqrtf(2.0f);
  return t;
}

int bcast_tx_launch(const BcastTables* t, uint32_t tti0, uint32_t nof_sf, void* d_grid, hipStream_t st)
{
  if (nof_sf == 0) return SRSLTE_SUCCESS;
  hipLaunchKernelGGL(dl_bcast_tx_kernel, dim3(nof_sf), dim3(64), 0, st, tti0, t->g, (cf32*)d_grid);
  LAUNCH_CHECK();
  return SRSLTE_SUCCESS;
}

extern "C" {

int srslte_hip_dl_ctrl_tx_put_bcast(srslte_hip_dl_ctrl_tx_t* q, uint32_t tti0, uint32_t nof_sf, void* d_grid, void* stream)
{
  const srslte_hip_dl_ctrl_tx_cfg_t* c = dl_ctrl_tx_cfg(q);
  if (!c || !d_grid || nof_sf > c->max_batch) return SRSLTE_ERROR_INVALID_INPUTS;
  return bcast_tx_launch(dl_ctrl_tx_bcast(q), tti0, nof_sf, d_grid, (hipStream_t)stream);
}

int srslte_hip_dl_ctrl_mib_batch(srslte_hip_dl_ctrl_t* q, const void* d_grid, const void* d_ce, const void* d_res, uint32_t tti0, uint32_t nof_sf,
                                 int search_all_ports, srslte_hip_mib_res_t* d_mib, void* stream)
{
  const BcastTables* t = dl_ctrl_bcast(q);
  if (!t || !d_grid || !d_ce || !d_res || !d_mib || nof_sf > t->max_batch) return SRSLTE_ERROR_INVALID_INPUTS;
  if (nof_sf == 0) return SRSLTE_SUCCESS;
  hipLaunchKernelGGL(dl_mib_kernel, dim3(nof_sf), dim3(256), 0, (hipStream_t)stream, (const cf32*)d_grid, (const cf32*)d_ce, (const float*)d_res, tti0,
                     search_all_ports ? 1 : 0, t->nof_rx, t->g, t->llr.get(), t->cand.get(), d_mib);
  LAUNCH_CHECK();
  return SRSLTE_SUCCESS;
}

const void* srslte_hip_dl_ctrl_mib_debug_buffer(const srslte_hip_dl_ctrl_t* q, int which)
{
  const BcastTables* t = dl_ctrl_bcast(q);
  if (!t) return nullptr;
  return which == 0 ? (const void*)t->llr.get() : which == 1 ? (const void*)t->cand.get() : nullptr;
}

int srslte_hip_pbch_re(const srslte_hip_dl_ctrl_cfg_t* cfg, uint32_t* re, uint32_t max)
{
  if (!ctrl_cell_ok(cfg)) return SRSLTE_ERROR_INVALID_INPUTS;
  BcastHost h;
  bcast_build(cfg->nof_prb, cfg->cell_id, cfg->cp_ext, h);
  if (!re || max < h.pbch_re.size()) return SRSLTE_ERROR_INVALID_INPUTS;
  memcpy(re, h.pbch_re.data(), h.pbch_re.size() * 4);
  return (int)h.pbch_re.size();
}

int srslte_hip_sync_re(const srslte_hip_dl_ctrl_cfg_t* cfg, uint32_t sf_idx, uint32_t* re, float* val, uint32_t max)
{
  if (!ctrl_cell_ok(cfg) || (sf_idx != 0 && sf_idx != 5) || !re || !val || max < 144) return SRSLTE_ERROR_INVALID_INPUTS;
  BcastHost h;
  bcast_build(cfg->nof_prb, cfg->cell_id, cfg->cp_ext, h);
  for (uint32_t i = 0; i < 72; i++) {
    re[i] = h.pss_k0 + i, val[2 * i] = h.pss[i][0], val[2 * i + 1] = h.pss[i][1];
    re[72 + i] = h.sss_k0 + i, val[2 * (72 + i)] = h.sss[sf_idx ? 1 : 0][i], val[2 * (72 + i) + 1] = 0.f;
  }
  return 144;
}

int srslte_hip_pbch_mib_pack(uint32_t nof_prb, int phich_ext, int phich_resources, uint32_t sfn, uint8_t* payload)
{
  if (!payload || nof_prb < 6 || nof_prb > 110 || phich_resources < 0 || phich_resources > 3) return SRSLTE_ERROR_INVALID_INPUTS;
  const uint32_t m = mib_head(nof_prb, phich_ext, phich_resources) << 18 | ((sfn >> 2) & 0xffu) << 10;
  for (int i = 0; i < 24; i++) payload[i] = (uint8_t)((m >> (23 - i)) & 1u);
  return 24;
}

} // extern "C"
