// Fragment of pdsch.hip (same translation unit): the PUSCH transmit pipeline (UE side), fixed grant.
// ====================================================================================================================
// PUSCH transmit pipeline (UE side, SURVEY §8d cfg3): TB CRC24A + segmentation + CB CRC24B (sch.c:183-297 as used by
// srslte_ulsch_encode :1068-1160) -> turbo encoder -> rate matching + UL channel interleaver + scrambling + modulation
// (rm_turbo.c:100-158, sch.c:580-598, pusch.c:380-400) -> transform precoding (:406) -> RE mapping with the DMRS
// (pusch_put :52-91, ue_ul.c:320-326) -> OFDM TX with 1/sqrt(N) and the +1/2 carrier shift (ue_ul.c:59-64).
// Same restrictions as the receive side: UL-SCH data only, same allocation in both slots, normal CP, rv 0.
// ====================================================================================================================
namespace {


struct PuschTxGeom {
  int   cell_nre, M_sc, n_prb, n_prb1, Qm, tti0, scr_words, C, K, tbs, rlenB, cb_stride, par_stride, tb_stride, rm_len, syms_lo, C_lo;
  int   nsymb; // 12 data symbols, 11 in a shortened subframe (extended CP: 10, 9)
  int   nsl;   // symbols per slot: 7, or 6 with the extended CP
  AckGeom        ack, ri;
  const uint8_t* ack_bits; // [nof_sf][2] HARQ-ACK values of this call, or null
  const uint8_t* ri_bits;  // [nof_sf][2] rank indication bits of this call, or null
  const uint8_t* q_cqi;    // [nof_sf][cqi_stride] coded CQI report bits of this call, or null
  int            Qp_cqi, cqi_stride;
  float lvl[16];
};

// grid = nof_sf, 256 threads: the coded CQI / PMI report, Q = Q' Qm bits per subframe (srslte_uci_encode_cqi_pusch, uci.c:470-494). Up to 11
// bits: the (32, O) block code repeated (encode_cqi_short :283-302). Above: CRC-8, the tail-biting rate-1/3 convolutional code (a circular
// convolution with 0x6D, 0x4F, 0x57; convcoder.c:43-72) and srslte_rm_conv_tx (rm_conv.c:44-89) as the table rm: output bit -> coded bit.
__global__ __launch_bounds__(256) void pusch_cqi_encode_kernel(const uint8_t* __restrict__ cqi, uint8_t* __restrict__ qb, int q_stride, int Q, int O,
                                                               const uint16_t* __restrict__ rm)
{
  __shared__ uint8_t msg[72], enc[3 * 72];
  const int          sf = blockIdx.x, tid = threadIdx.x;
  const uint8_t*     in = cqi + (size_t)sf * 64;
  uint8_t*           out = qb + (size_t)sf * q_stride;
  if (O <= 11) {
    if (tid < 32) {
      int b = 0;
      for (int n = 0; n < O; n++) b ^= in[n] & (CQI_M32[tid] >> n) & 1;
      enc[tid] = (uint8_t)b;
    }
    __syncthreads();
    for (int i = tid; i < Q; i += 256) out[i] = enc[i & 31];
    return;
  }
  const int F = O + 8;
  if (tid < O) msg[tid] = in[tid] & 1;
  __syncthreads();
  if (tid == 0) {
    const uint32_t c = cqi_crc8(msg, O);
    for (int i = 0; i < 8; i++) msg[O + i] = (c >> (7 - i)) & 1;
  }
  __syncthreads();
  for (int e = tid; e < 3 * F; e += 256) {
    const int      i = e / 3, p = e - 3 * i;
    const uint32_t poly = p == 0 ? 0x6Du : (p == 1 ? 0x4Fu : 0x57u);
    int            b = 0;
    for (int j = 0; j < 7; j++) b ^= ((poly >> j) & 1u) & msg[(i - j + F) % F];
    enc[e] = (uint8_t)b;
  }
  __syncthreads();
  for (int i = tid; i < Q; i += 256) out[i] = enc[rm[i]];
}

// grid = nof_sf, 256 threads: CRC24A of each transport block (sch.c:470-488 on the transmit side :1104-1110)
__global__ __launch_bounds__(256) void pusch_tx_tbcrc_kernel(const uint8_t* __restrict__ tb, uint32_t* __restrict__ crc_out, PuschTxGeom g)
{
  __shared__ uint32_t tab[256], red[256];
  const uint8_t*      x = tb + (size_t)blockIdx.x * g.tb_stride;
  const uint32_t      c = block_crc24([&](int i) { return (uint32_t)x[i]; }, g.tbs / 8, 0x1864CFBu, tab, red);
  if (threadIdx.x == 0) crc_out[blockIdx.x] = c;
}

// grid = (C, nof_sf), 256 threads: code block r = bytes [r*rlenB, (r+1)*rlenB) of TB | CRC24A, then its CRC24B when C > 1 (sch.c:222-262)
__global__ __launch_bounds__(256) void pusch_tx_seg_kernel(const uint8_t* __restrict__ tb, const uint32_t* __restrict__ tbcrc, uint8_t* __restrict__ cb,
                                                           PuschTxGeom g)
{
  __shared__ uint32_t tab[256], red[256];
  __shared__ uint8_t  xs[768];
  const int           r = blockIdx.x, sf = blockIdx.y, t = threadIdx.x, tbB = g.tbs / 8;
  const uint8_t*      x   = tb + (size_t)sf * g.tb_stride;
  const uint32_t      crc = tbcrc[sf];
  uint8_t*            out = cb + ((size_t)sf * g.C + r) * g.cb_stride;
  for (int i = t; i < g.rlenB; i += 256) {
    const int j = r * g.rlenB + i;
    xs[i]       = j < tbB ? x[j] : (uint8_t)(crc >> (8 * (2 - (j - tbB))));
  }
  __syncthreads();
  for (int i = t; i < g.rlenB; i += 256) out[i] = xs[i];
  if (g.C > 1) {
    const uint32_t c = block_crc24([&](int i) { return (uint32_t)xs[i]; }, g.rlenB, 0x1800063u, tab, red);
    if (t < 3) out[g.rlenB + t] = (uint8_t)(c >> (8 * (2 - t)));
  }
}

// grid = (ceil(M_sc/256), 12, nof_sf): modulation symbol (n, k) of the interleaved, scrambled stream: its Qm bits are
// g[(k*12 + n)*Qm + b] (36.212 5.2.2.8 without UCI), all from one code block; bit e of a block = coded bit rm[e mod (3K+12)]
// (rm: circular-buffer order with the NULLs removed; source 0 = systematic byte stream, 1 = its tail nibble, 2 = parity stream)
// One PUSCH: cs its scrambling bits, cb0 its first code-block slot, ack / ri / qc its UCI inputs (or null), d its [nsymb][M_sc] symbols, lvl the
// levels of its modulation (the geometry's own lvl member is not read here)
__device__ __forceinline__ void pusch_tx_mod_body(const uint8_t* __restrict__ cb, const uint8_t* __restrict__ parity, const uint8_t* __restrict__ sys_tail,
                                                  const uint32_t* __restrict__ rm, const uint32_t* __restrict__ cs, cf32* __restrict__ d, const PuschTxGeom& g,
                                                  int k, int n, int cb0, const uint8_t* __restrict__ ack, const uint8_t* __restrict__ rib,
                                                  const uint8_t* __restrict__ qc, const float* __restrict__ lvl)
{
  if (k >= g.M_sc) return;
  const int ri = rib ? ri_symbol_index(g.ri, n, k, g.M_sc, g.nsymb) : -1; // RI symbol: outside the UL-SCH stream (sch.c:580-598)
  // symbol index in g order; blocks 0..C_lo-1 carry syms_lo symbols, the rest syms_lo + 1 (sch.c:238-243)
  const int s0 = ri >= 0 ? 0 : k * g.nsymb + n - (rib ? ri_before(g.ri, n, k, g.M_sc, g.nsymb) : 0);
  // the first Q'_cqi symbols of the stream carry the CQI report, the UL-SCH follows (sch.c:1133-1160)
  const bool is_cqi = ri < 0 && s0 < g.Qp_cqi;
  const int  s      = is_cqi || ri >= 0 ? 0 : s0 - g.Qp_cqi;
  const bool data   = g.C > 0 && !is_cqi && ri < 0; // a PUSCH without UL-SCH data (C = 0) is CQI and RI symbols only (sch.c:1157)
  int        r = 0, e0 = 0;
  if (data) {
    if (s < g.C_lo * g.syms_lo) {
      r  = s / g.syms_lo;
      e0 = (s - r * g.syms_lo) * g.Qm;
    } else {
      const int u = s - g.C_lo * g.syms_lo;
      r           = g.C_lo + u / (g.syms_lo + 1);
      e0          = (u % (g.syms_lo + 1)) * g.Qm;
    }
  }
  const size_t    cbi = (size_t)cb0 + r;
  const uint8_t * xb = cb + cbi * g.cb_stride, *pb = parity + cbi * g.par_stride;
  const int       q0  = (n * g.M_sc + k) * g.Qm;
  const int       ai  = ack ? ack_symbol_index(g.ack, n, k, g.M_sc, g.nsymb) : -1;
  int             re = 0, im = 0, prev = 0;
  for (int b = 0; b < g.Qm; b++) {
    int bit = 0;
    if (data) {
      const uint32_t src = rm[(e0 + b) % g.rm_len], pos = src & 0x3fffffffu;
      const uint8_t  byte = (src >> 30) == 0 ? xb[pos >> 3] : ((src >> 30) == 1 ? sys_tail[cbi] : pb[pos >> 3]);
      bit                 = (byte >> (7 - (pos & 7))) & 1;
    }
    const int cbit = (cs[(q0 + b) >> 5] >> ((q0 + b) & 31)) & 1;
    if (is_cqi) bit = qc[s0 * g.Qm + b];
    bit ^= cbit;
    if (ai >= 0) { // HARQ-ACK symbol: value bits are scrambled, placeholders are 1, a repetition bit copies the transmitted bit before it
      const int t = ack_bit_type(ack, g.ack.O, g.Qm, ai * g.Qm + b); // (sch.c:1203-1215, pusch.c:386-400)
      bit         = t == 3 ? 1 : (t == 2 ? prev : (t ^ cbit));
    }
    if (ri >= 0) { // rank indication: the same encoder (sch.c:1110-1129)
      const int t = ack_bit_type(rib, g.ri.O, g.Qm, ri * g.Qm + b);
      bit         = t == 3 ? 1 : (t == 2 ? prev : (t ^ cbit));
    }
    prev = bit;
    if (b & 1) im = (im << 1) | bit;
    else re = (re << 1) | bit;
  }
  d[(size_t)n * g.M_sc + k] = make_float2(lvl[re], lvl[im]);
}


__global__ __launch_bounds__(256) void pusch_tx_mod_kernel(const uint8_t* __restrict__ cb, const uint8_t* __restrict__ parity,
                                                           const uint8_t* __restrict__ sys_tail, const uint32_t* __restrict__ rm,
                                                           const uint32_t* __restrict__ scr, cf32* __restrict__ d, PuschTxGeom g)
{
  const int sf = blockIdx.z, sf_idx = (g.tti0 + sf) % 10;
  pusch_tx_mod_body(cb, parity, sys_tail, rm, scr + (size_t)sf_idx * g.scr_words, d + (size_t)sf * g.nsymb * g.M_sc, g, blockIdx.x * blockDim.x + threadIdx.x,
                    blockIdx.y, sf * g.C, g.ack_bits ? g.ack_bits + 2 * sf : nullptr, g.ri_bits ? g.ri_bits + 2 * sf : nullptr,
                    g.q_cqi ? g.q_cqi + (size_t)sf * g.cqi_stride : nullptr, g.lvl);
}

// grid = (ceil(cell_nre/256), 2 nsl, nof_sf): resource grid of the subframe: z on the granted PRBs of the data symbols, DMRS on
// l = nsl - 4 of each slot (3, 10; extended CP: 2, 8), zero elsewhere (the caller's memset + pusch_put + srslte_refsignal_dmrs_pusch_put)
__global__ __launch_bounds__(256) void pusch_tx_map_kernel(const cf32* __restrict__ z, const cf32* __restrict__ dmrs, cf32* __restrict__ grid,
                                                           PuschTxGeom g)
{
  const int k = blockIdx.x * blockDim.x + threadIdx.x, l = blockIdx.y, sf = blockIdx.z, sf_idx = (g.tti0 + sf) % 10;
  if (k >= g.cell_nre) return;
  const int L0 = g.nsl - 4, L1 = 2 * g.nsl - 4;
  const int kk = k - 12 * (l < g.nsl ? g.n_prb : g.n_prb1); // each slot at its own offset (pusch_cp, pusch.c:52-91; refsignal_ul.c:316-330)
  cf32      v  = make_float2(0.f, 0.f);
  if (kk >= 0 && kk < g.M_sc) {
    if (l == L0 || l == L1) {
      v = dmrs[((size_t)sf_idx * 2 + (l == L1)) * g.M_sc + kk];
    } else {
      const int n = l < L0 ? l : (l < L1 ? l - 1 : l - 2);
      if (n < g.nsymb) v = z[((size_t)sf * g.nsymb + n) * g.M_sc + kk]; // the last symbol of a shortened subframe stays empty
    }
  }
  grid[((size_t)sf * 2 * g.nsl + l) * g.cell_nre + k] = v;
}

struct TxLevels { float v[5][16]; };   // constellation levels of one axis per srslte_mod_t (the grants modes of both transmit pipelines)

} // namespace

// The encoder half of a fixed-grant transmitter, downlink or uplink: TB CRC24A, segmentation + CB CRC24B and the turbo encoder of a batch into
// code-block slots of one block length, and the rate-matching tables the modulation kernels read them through
struct SchTxFixed {
  srslte_hip_cbsegm_t seg = {};
  PuschTxGeom         cg  = {}; // CRC attachment / segmentation geometry: C, K, tbs, rlenB, cb_stride, par_stride
  DevBuf<uint32_t>    d_tbcrc;
  DevBuf<uint32_t>    d_rm_rv[4]; // rate-matching tables: [0] made by init, 1-3 on first use
  DevBuf<uint8_t>     d_cb, d_parity, d_sys_tail;
  // seg has passed fixed_grant_segmentation; seg.C = 0 (a PUSCH without UL-SCH data): no code-block slots, no table
  int init(uint32_t B)
  {
    const uint32_t C = seg.C, K = seg.K1;
    cg.C = (int)C; cg.K = (int)K; cg.tbs = (int)seg.tbs; cg.rlenB = (int)((C <= 1 ? K : K - 24) / 8); cg.cb_stride = (int)((K / 8 + 15) & ~15u);
    cg.par_stride = (int)((K / 4 + 1 + 15) & ~15u);
    if (d_tbcrc.alloc(B)) return SRSLTE_ERROR;
    if (C == 0) return SRSLTE_SUCCESS;
    const bool bad = rm_tx_table_upload(K, 0, d_rm_rv[0]) || d_cb.alloc((size_t)cg.cb_stride * B * C) || d_parity.alloc((size_t)cg.par_stride * B * C) ||
                     d_sys_tail.alloc((size_t)B * C);
    return bad ? SRSLTE_ERROR : SRSLTE_SUCCESS;
  }
  // rows of d_tb -> d_cb / d_parity / d_sys_tail of slots 0 .. nof_sf C - 1; *d_rm: the rate-matching table of rv (null and no launch for C = 0)
  int encode(const uint8_t* d_tb, uint32_t tb_stride, uint32_t nof_sf, uint32_t rv, void* stream, const uint32_t** d_rm)
  {
    *d_rm = nullptr;
    if (cg.C == 0) return SRSLTE_SUCCESS; // no UL-SCH data (tbs = 0): no CRC, no segmentation, no encoder (sch.c:1157)
    if (!d_rm_rv[rv]) {
      if (int r = rm_tx_table_upload(seg.K1, rv, d_rm_rv[rv])) return r;
    }
    *d_rm          = d_rm_rv[rv];
    hipStream_t st = (hipStream_t)stream;
    PuschTxGeom g  = cg;
    g.tb_stride    = (int)tb_stride;
    hipLaunchKernelGGL(pusch_tx_tbcrc_kernel, dim3(nof_sf), dim3(256), 0, st, d_tb, d_tbcrc, g);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(pusch_tx_seg_kernel, dim3(g.C, nof_sf), dim3(256), 0, st, d_tb, (const uint32_t*)d_tbcrc, d_cb, g);
    LAUNCH_CHECK();
    return srslte_hip_tcod_encode_bytes_batch(d_cb, (uint32_t)g.cb_stride, d_parity, (uint32_t)g.par_stride, d_sys_tail, (uint32_t)g.K, nof_sf * (uint32_t)g.C,
                                              stream);
  }
};

// The encoder half of a transmit grants mode, downlink or uplink: ncw codewords of up to Cmax code blocks in slots spaced for the largest block
// length, their scrambling rows and CRC words, the call's descriptor block and the rate-matching tables made on first use
struct TxGrantsEnc {
  uint32_t         Cmax = 0, words = 0, cb_stride = (6144 / 8 + 15) & ~15u, par_stride = (6144 / 4 + 1 + 15) & ~15u;
  DevBuf<uint32_t> d_scr, d_basis, d_tbcrc;
  DevBuf<uint8_t>  d_cb, d_parity, d_sys_tail;
  size_t           desc_bytes = 0;
  DescStage        desc; // the descriptor block: pinned host copies and the device block
  TxLevels         lv = {};
  std::map<std::pair<uint32_t, uint32_t>, DevBuf<uint32_t>> rm_tbl; // (K, rv) -> rate-matching table over the encoder's byte streams
  int enc_init(uint32_t ncw, uint32_t Cmax_, uint32_t words_, size_t desc_bytes_)
  {
    Cmax = Cmax_; words = words_; desc_bytes = desc_bytes_;
    const size_t nblk = (size_t)ncw * Cmax;
    if (desc.init(desc_bytes) || gold_basis_upload(words, d_basis) || d_scr.alloc((size_t)words * ncw) || d_tbcrc.alloc(ncw) ||
        d_cb.alloc((size_t)cb_stride * nblk) || d_parity.alloc((size_t)par_stride * nblk) || d_sys_tail.alloc(nblk))
      return SRSLTE_ERROR;
    for (int mod = 1; mod <= 4; mod++) constellation_levels(mod, lv.v[mod]);
    return SRSLTE_SUCCESS;
  }
  const uint32_t* rm_table(uint32_t K, uint32_t rv) // null: the upload failed
  {
    auto it = rm_tbl.find({K, rv});
    if (it == rm_tbl.end()) {
      DevBuf<uint32_t> d;
      if (rm_tx_table_upload(K, rv, d)) return nullptr;
      it = rm_tbl.emplace(std::make_pair(K, rv), std::move(d)).first;
    }
    return it->second;
  }
};

// Device / host resources of the per-PUSCH grants mode of the transmit pipeline (pusch_tx_grants.inc)
struct UlTxGrantsState : TxGrantsEnc {
  uint32_t        V = 0, max_sym = 0, cqi_stride = 0;
  DevBuf<uint8_t> d_qcqi;
  DevBuf<cf32>    d_d, d_z;
  std::map<uint32_t, DevBuf<uint16_t>> cqi_w; // report size O > 11 -> srslte_rm_conv_tx order of its coded bits
};

struct srslte_hip_ul_tx {
  srslte_hip_ul_tx_cfg_t cfg  = {};
  srslte_hip_ofdm_t*     ofdm = nullptr;
  srslte_hip_chest_ul_t* dmrs = nullptr;
  SchTxFixed             enc;
  PuschTxGeom            g    = {};
  DevBuf<uint32_t>       d_scr;
  DevBuf<uint8_t>        d_qcqi;
  DevBuf<uint16_t>       d_cqi_rm;
  DevBuf<cf32>           d_d, d_z, d_grid;
  std::unique_ptr<UlTxGrantsState> gs; // srslte_hip_ul_tx_batch_grants: created on first use
  ~srslte_hip_ul_tx()
  {
    srslte_hip_ofdm_destroy(ofdm);
    srslte_hip_chest_ul_destroy(dmrs);
  }
};

extern "C" void srslte_hip_ul_tx_destroy(srslte_hip_ul_tx_t* q) { delete q; }

// phy_hip.h, "Sample formats": d_iq of every entry point of the object is in the OFDM object's format from here on
extern "C" int srslte_hip_ul_tx_set_iq_format(srslte_hip_ul_tx_t* q, int format, float scale)
{
  return q ? srslte_hip_ofdm_set_sample_format(q->ofdm, format, scale) : SRSLTE_ERROR_INVALID_INPUTS;
}

extern "C" srslte_hip_ul_tx_t* srslte_hip_ul_tx_create(const srslte_hip_ul_tx_cfg_t* cfg)
{
  if (!cfg || cfg->max_batch == 0 || cfg->mod < 1 || cfg->mod > 3 || cfg->L_prb < 1 || cfg->n_prb + cfg->L_prb > cfg->nof_prb ||
      (cfg->hopping && cfg->n_prb_slot1 + cfg->L_prb > cfg->nof_prb) ||
      !srslte_hip_dft_precoding_valid_prb(cfg->L_prb)) {
    hip_log("[srslte_hip] ul_tx: invalid configuration\n");
    return nullptr;
  }
  std::unique_ptr<srslte_hip_ul_tx> q(new srslte_hip_ul_tx());
  q->cfg = *cfg;
  if (fixed_grant_segmentation("ul_tx", cfg->tbs, &q->enc.seg)) return nullptr;
  const uint32_t P = cfg->nof_prb, B = cfg->max_batch, C = q->enc.seg.C, K = q->enc.seg.K1, Qm = 2 * (uint32_t)cfg->mod, M_sc = 12 * cfg->L_prb;
  const uint32_t nsl = cfg->cp_ext ? 6 : 7, nsymb = 2 * (nsl - 1) - (cfg->shortened ? 1 : 0); // ra_ul.c:234 nof_symb
  const uint32_t nof_re = nsymb * M_sc, nbits = nof_re * Qm, scr_words = (nbits + 31) / 32;
  PuschTxGeom&   g = q->g;
  g.cell_nre = 12 * (int)P; g.M_sc = (int)M_sc; g.n_prb = (int)cfg->n_prb; g.n_prb1 = (int)(cfg->hopping ? cfg->n_prb_slot1 : cfg->n_prb); g.Qm = (int)Qm; g.scr_words = (int)scr_words; g.C = (int)C; g.K = (int)K;
  g.nsymb = (int)nsymb;
  g.nsl   = (int)nsl;
  srslte_hip_pusch_uci_res_t uci;
  if (const int why = pusch_pipeline_uci(*cfg, nsymb, q->enc.seg, &uci)) {
    // a PUSCH without UL-SCH data carries a CQI report (srslte_ulsch_encode, sch.c:1133-1165)
    hip_log(why == SRSLTE_HIP_PUSCH_UCI_EMPTY ? "[srslte_hip] ul_tx: neither a transport block nor a CQI report\n"
                                              : "[srslte_hip] ul_tx: invalid HARQ-ACK, rank-indication or CQI configuration\n");
    return nullptr;
  }
  g.tbs = (int)cfg->tbs; g.rm_len = (int)(3 * K + 12);
  g.ack.O = (int)cfg->ack_len; g.ack.Qprime = (int)uci.Qp_ack;
  g.ri.O = (int)cfg->ri_len; g.ri.Qprime = (int)uci.Qp_ri;
  g.Qp_cqi = (int)uci.Qp_cqi; g.cqi_stride = ((int)uci.Q_cqi + 15) & ~15;
  g.syms_lo = (int)uci.syms_lo; g.C_lo = (int)uci.C_lo; // of G', the symbols the RI and the report leave to the UL-SCH
  constellation_levels(cfg->mod, g.lvl); // one axis: bits b0 b2 b4 of the symbol
  q->ofdm = srslte_hip_ofdm_create((int)P, cfg->cp_ext ? 0 : 1, 0);
  q->dmrs = srslte_hip_chest_ul_create(cfg->cell_id, P, cfg->cp_ext ? 0 : 1, &cfg->dmrs_cfg);
  bool ok = q->ofdm && q->dmrs && srslte_hip_ofdm_set_normalize(q->ofdm, 1) == SRSLTE_SUCCESS &&
            srslte_hip_ofdm_set_freq_shift(q->ofdm, 0.5f) == SRSLTE_SUCCESS; // ue_ul.c:63-64
  if (ok) { // srslte_sequence_pusch (sequences.c:65-67)
    std::vector<uint32_t> scr;
    lte_scr_table([&](uint32_t sf) { return ((uint32_t)cfg->rnti << 14) + (sf << 9) + cfg->cell_id; }, nbits, scr_words, scr);
    ok = upload(q->d_scr, scr) == SRSLTE_SUCCESS && q->enc.init(B) == SRSLTE_SUCCESS;
  }
  g.rlenB = q->enc.cg.rlenB; g.cb_stride = q->enc.cg.cb_stride; g.par_stride = q->enc.cg.par_stride;
  if (ok && cfg->cqi_len > 11) { // the CQI report's rate matching: cqi_rm_conv_order read circularly up to Q
    const std::vector<uint16_t> w = cqi_rm_conv_order(cfg->cqi_len);
    const int                   Q = g.Qp_cqi * (int)Qm;
    std::vector<uint16_t>       t((size_t)(Q > 0 ? Q : 1));
    for (int i = 0; i < Q; i++) t[i] = w[(size_t)i % w.size()];
    ok = upload(q->d_cqi_rm, t) == SRSLTE_SUCCESS;
  }
  if (ok && cfg->cqi_len) ok = !q->d_qcqi.alloc((size_t)g.cqi_stride * B + 16);
  const size_t glen = (size_t)2 * nsl * 12 * P;
  ok = ok && !q->d_d.alloc((size_t)nof_re * B) && !q->d_z.alloc((size_t)nof_re * B) && !q->d_grid.alloc(glen * B);
  if (!ok) {
    hip_log("[srslte_hip] ul_tx: initialisation failed\n");
    return nullptr;
  }
  return q.release();
}

extern "C" const void* srslte_hip_ul_tx_debug_buffer(const srslte_hip_ul_tx_t* q, int which)
{
  if (!q) return nullptr;
  switch (which) {
    case 0: return q->enc.d_cb;
    case 1: return q->enc.d_parity;
    case 2: return q->d_d;
    case 3: return q->d_z;
    case 4: return q->d_grid;
    case 5: return q->enc.d_tbcrc;
  }
  return nullptr;
}

extern "C" int srslte_hip_ul_tx_batch(srslte_hip_ul_tx_t* q, const uint8_t* d_tb, uint32_t tb_stride, uint32_t tti0, uint32_t nof_sf, void* d_iq,
                                      void* stream)
{
  if (q && (q->cfg.ack_len || q->cfg.ri_len || q->cfg.cqi_len)) return SRSLTE_ERROR_INVALID_INPUTS; // UCI configured: the values come through _batch_ack / _batch_uci / _batch_uci_cqi
  return srslte_hip_ul_tx_batch_ack(q, d_tb, tb_stride, nullptr, tti0, nof_sf, d_iq, stream);
}

extern "C" int srslte_hip_ul_tx_batch_ack(srslte_hip_ul_tx_t* q, const uint8_t* d_tb, uint32_t tb_stride, const uint8_t* d_ack, uint32_t tti0,
                                          uint32_t nof_sf, void* d_iq, void* stream)
{
  return srslte_hip_ul_tx_batch_uci(q, d_tb, tb_stride, d_ack, nullptr, tti0, nof_sf, d_iq, stream);
}

extern "C" int srslte_hip_ul_tx_batch_uci(srslte_hip_ul_tx_t* q, const uint8_t* d_tb, uint32_t tb_stride, const uint8_t* d_ack, const uint8_t* d_ri,
                                          uint32_t tti0, uint32_t nof_sf, void* d_iq, void* stream)
{
  return srslte_hip_ul_tx_batch_uci_cqi(q, d_tb, tb_stride, d_ack, d_ri, nullptr, tti0, nof_sf, d_iq, stream);
}

extern "C" int srslte_hip_ul_tx_batch_uci_cqi(srslte_hip_ul_tx_t* q, const uint8_t* d_tb, uint32_t tb_stride, const uint8_t* d_ack, const uint8_t* d_ri,
                                              const uint8_t* d_cqi, uint32_t tti0, uint32_t nof_sf, void* d_iq, void* stream)
{
  return srslte_hip_ul_tx_batch_rv(q, d_tb, tb_stride, d_ack, d_ri, d_cqi, 0, tti0, nof_sf, d_iq, stream);
}

// The same with a redundancy version (srslte_pusch_grant_t.tb.rv -> srslte_ulsch_encode -> srslte_rm_turbo_tx_lut's k0, rm_turbo.c:100-158):
// what a retransmission sends. Everything else - UCI multiplexing, interleaver, scrambling - does not depend on it.
extern "C" int srslte_hip_ul_tx_batch_rv(srslte_hip_ul_tx_t* q, const uint8_t* d_tb, uint32_t tb_stride, const uint8_t* d_ack, const uint8_t* d_ri,
                                         const uint8_t* d_cqi, uint32_t rv, uint32_t tti0, uint32_t nof_sf, void* d_iq, void* stream)
{
  if (!q || (!d_tb && q->cfg.tbs) || !d_iq || rv > 3 || nof_sf > q->cfg.max_batch || tb_stride < q->cfg.tbs / 8) return SRSLTE_ERROR_INVALID_INPUTS;
  if ((q->cfg.ack_len != 0) != (d_ack != nullptr) || (q->cfg.ri_len != 0) != (d_ri != nullptr) || (q->cfg.cqi_len != 0) != (d_cqi != nullptr))
    return SRSLTE_ERROR_INVALID_INPUTS;
  if (nof_sf == 0) return SRSLTE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  const void* d_r = nullptr;
  if (int r = chest_ul_dmrs_table(q->dmrs, q->cfg.L_prb, q->cfg.n_dmrs, &d_r)) return r;
  PuschTxGeom g = q->g;
  g.tti0        = (int)tti0;
  g.tb_stride   = (int)tb_stride;
  g.ack_bits    = d_ack;
  g.ri_bits     = d_ri;
  g.q_cqi       = d_cqi ? q->d_qcqi : nullptr;
  if (d_cqi) {
    hipLaunchKernelGGL(pusch_cqi_encode_kernel, dim3(nof_sf), dim3(256), 0, st, d_cqi, q->d_qcqi, g.cqi_stride, g.Qp_cqi * g.Qm, (int)q->cfg.cqi_len,
                       (const uint16_t*)q->d_cqi_rm);
    LAUNCH_CHECK();
  }
  const uint32_t* d_rm = nullptr;
  int             r    = q->enc.encode(d_tb, tb_stride, nof_sf, rv, stream, &d_rm);
  if (r) return r;
  hipLaunchKernelGGL(pusch_tx_mod_kernel, dim3(ceil_div(g.M_sc, 256), g.nsymb, nof_sf), dim3(256), 0, st, (const uint8_t*)q->enc.d_cb,
                     (const uint8_t*)q->enc.d_parity, (const uint8_t*)q->enc.d_sys_tail, d_rm, (const uint32_t*)q->d_scr, q->d_d, g);
  LAUNCH_CHECK();
  r = srslte_hip_dft_precoding_batch(q->d_d, q->d_z, q->cfg.L_prb, g.nsymb * nof_sf, 1, stream); // srslte_dft_precoding_init_tx: forward, 1/sqrt(N)
  if (r) return r;
  hipLaunchKernelGGL(pusch_tx_map_kernel, dim3(ceil_div(g.cell_nre, 256), 2 * g.nsl, nof_sf), dim3(256), 0, st, (const cf32*)q->d_z, (const cf32*)d_r,
                     q->d_grid, g);
  LAUNCH_CHECK();
  return srslte_hip_ofdm_tx_sf_batch(q->ofdm, q->d_grid, d_iq, (int)nof_sf, stream);
}
