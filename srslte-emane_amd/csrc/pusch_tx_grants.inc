// Fragment of pdsch.hip (same translation unit): per-PUSCH grants on the transmit side (uses the descriptors of pdsch_tx.inc).
// ====================================================================================================================
// Per-PUSCH grants on the transmit side (srslte_hip_ul_tx_batch_grants): every PUSCH of a call has its own allocation, DMRS cyclic shift, RNTI,
// modulation, transport block, redundancy version and UCI - what srslte_ue_ul_encode sends TTI after TTI as the grants come in (ue_ul.c:300-340),
// and, with several PUSCHs on disjoint PRBs of one subframe, the composite signal of several UEs as an eNB receives it.
// ====================================================================================================================
namespace {

struct PuschTxDesc {
  int             M_sc, n_prb, n_prb1, zoff, syms_lo, C_lo, Qp_cqi, cqi_O, cqi_wlen, sf_idx;
  AckGeom         ack, ri;
  const uint16_t* cqi_w; // srslte_rm_conv_tx order of the report's coded bits (reports above 11 bits), read circularly
  const cf32*     dmrs;  // table of (L_prb, n_dmrs): [10][2][M_sc]
};

// grid = nof_pusch: the coded CQI report of each PUSCH that carries one (pusch_cqi_encode_kernel with the sizes of the row's descriptor)
__global__ __launch_bounds__(256) void pusch_cqi_encode_grants_kernel(const uint8_t* __restrict__ cqi, uint8_t* __restrict__ qb, int q_stride,
                                                                      const PuschTxDesc* __restrict__ desc, const TxDesc* __restrict__ td)
{
  __shared__ uint8_t msg[72], enc[3 * 72];
  const int          p = blockIdx.x, tid = threadIdx.x, O = desc[p].cqi_O, Q = desc[p].Qp_cqi * td[p].Qm;
  if (O == 0) return;
  const uint8_t* in  = cqi + (size_t)p * 64;
  uint8_t*       out = qb + (size_t)p * q_stride;
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
    const int      i = e / 3, pp = e - 3 * i;
    const uint32_t poly = pp == 0 ? 0x6Du : (pp == 1 ? 0x4Fu : 0x57u);
    int            b = 0;
    for (int j = 0; j < 7; j++) b ^= ((poly >> j) & 1u) & msg[(i - j + F) % F];
    enc[e] = (uint8_t)b;
  }
  __syncthreads();
  const uint16_t* w = desc[p].cqi_w;
  const int       wlen = desc[p].cqi_wlen;
  for (int i = tid; i < Q; i += 256) out[i] = enc[w[i % wlen]];
}

// grid = (ceil(max M_sc / 256), nsymb, nof_pusch)
__global__ __launch_bounds__(256) void pusch_tx_mod_grants_kernel(const uint8_t* __restrict__ cb, const uint8_t* __restrict__ parity,
                                                                  const uint8_t* __restrict__ sys_tail, const uint32_t* __restrict__ scr, int scr_words,
                                                                  cf32* __restrict__ d, const PuschTxDesc* __restrict__ desc, const TxDesc* __restrict__ td,
                                                                  TxLevels lv, int nsymb, int cb_stride, int par_stride, const uint8_t* __restrict__ ack,
                                                                  const uint8_t* __restrict__ rib, const uint8_t* __restrict__ qcqi, int cqi_stride)
{
  const int          p = blockIdx.z;
  const PuschTxDesc& pd = desc[p];
  PuschTxGeom        g; // a local built from the descriptors (its lvl member stays untouched: the levels come through lv)
  g.M_sc = pd.M_sc; g.Qm = td[p].Qm; g.C = td[p].C; g.rm_len = 3 * td[p].K + 12; g.syms_lo = pd.syms_lo; g.C_lo = pd.C_lo; g.nsymb = nsymb;
  g.cb_stride = cb_stride; g.par_stride = par_stride; g.ack = pd.ack; g.ri = pd.ri; g.Qp_cqi = pd.Qp_cqi;
  pusch_tx_mod_body(cb, parity, sys_tail, td[p].rm, scr + (size_t)p * scr_words, d + pd.zoff, g, blockIdx.x * blockDim.x + threadIdx.x, blockIdx.y, td[p].cb0,
                    pd.ack.O ? ack + 2 * p : nullptr, pd.ri.O ? rib + 2 * p : nullptr, pd.cqi_O ? qcqi + (size_t)p * cqi_stride : nullptr, lv.v[td[p].mod]);
}

// grid = (ceil(max M_sc / 256), 2 nsl, nof_pusch): pusch_put + srslte_refsignal_dmrs_pusch_put of PUSCH p into the (zeroed) grid of its subframe
__global__ __launch_bounds__(256) void pusch_tx_scatter_kernel(const cf32* __restrict__ z, cf32* __restrict__ grid, const PuschTxDesc* __restrict__ desc,
                                                               const TxDesc* __restrict__ td, int cell_nre, int nsymb, int nsl)
{
  const int          L0 = nsl - 4, L1 = 2 * nsl - 4; // the DMRS symbols (3, 10; extended CP: 2, 8)
  const int          kk = blockIdx.x * blockDim.x + threadIdx.x, l = blockIdx.y, p = blockIdx.z;
  const PuschTxDesc& pd = desc[p];
  if (kk >= pd.M_sc) return;
  cf32 v;
  if (l == L0 || l == L1) {
    v = pd.dmrs[((size_t)pd.sf_idx * 2 + (l == L1)) * pd.M_sc + kk];
  } else {
    const int n = l < L0 ? l : (l < L1 ? l - 1 : l - 2);
    if (n >= nsymb) return; // the last symbol of a shortened subframe stays empty
    v = z[(size_t)pd.zoff + (size_t)n * pd.M_sc + kk];
  }
  grid[((size_t)td[p].sf * 2 * nsl + l) * cell_nre + 12 * (l < nsl ? pd.n_prb : pd.n_prb1) + kk] = v;
}

} // namespace

static int ul_tx_grants_init(srslte_hip_ul_tx_t* q, uint32_t V)
{
  const uint32_t P = q->cfg.nof_prb, nsymb = (uint32_t)q->g.nsymb;
  q->gs.reset(new UlTxGrantsState());
  UlTxGrantsState* g = q->gs.get();
  g->V          = V;
  g->max_sym    = nsymb * 12 * P;
  g->cqi_stride = (g->max_sym * 6 + 15) & ~15u; // a report may take the whole allocation (min(.., M_sc N_symb - Q'_ri), uci.c:264-281)
  if (g->enc_init(V, q->enc.seg.C, (g->max_sym * 6 + 31) / 32 + 2, (sizeof(GrantDev) + sizeof(TxDesc) + sizeof(PuschTxDesc)) * V) ||
      g->d_qcqi.alloc((size_t)g->cqi_stride * V) || g->d_d.alloc((size_t)g->max_sym * V) || g->d_z.alloc((size_t)g->max_sym * V))
    return SRSLTE_ERROR;
  return SRSLTE_SUCCESS;
}

// grants[p]: as srslte_hip_ul_rx_batch_grants takes them (new_data is not used). Row p of d_tb is its transport block; d_ack / d_ri: [nof_grants][2],
// d_cqi: [nof_grants][64] device bytes, rows p (each may be NULL when no grant of the call carries that kind of UCI). The object's cell, DMRS
// configuration and shortened flag apply; cfg.tbs bounds every grant's tbs, cfg.max_grants the number of PUSCHs per call.
extern "C" int srslte_hip_ul_tx_batch_grants(srslte_hip_ul_tx_t* q, const uint8_t* d_tb, uint32_t tb_stride, const uint8_t* d_ack, const uint8_t* d_ri,
                                             const uint8_t* d_cqi, uint32_t tti0, uint32_t nof_sf, const srslte_hip_ul_grant_t* grants, uint32_t nof_grants,
                                             void* d_iq, void* stream)
{
  if (!q || !d_tb || !d_iq || !grants || nof_sf > q->cfg.max_batch) return SRSLTE_ERROR_INVALID_INPUTS;
  const uint32_t V = q->cfg.max_grants ? q->cfg.max_grants : q->cfg.max_batch, P = q->cfg.nof_prb, nsymb = (uint32_t)q->g.nsymb;
  if (nof_grants > V || q->enc.seg.C == 0) return SRSLTE_ERROR_INVALID_INPUTS; // an object made without a transport-block size has no encoder buffers
  if (nof_sf == 0) return SRSLTE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  if (!q->gs && ul_tx_grants_init(q, V)) { // a failed start leaves no half-made state behind
    hip_log("[srslte_hip] ul_tx grants: initialisation failed\n");
    q->gs.reset();
    return SRSLTE_ERROR;
  }
  UlTxGrantsState* g    = q->gs.get();
  GrantDev*        h_gr = nullptr;
  if (int r = g->desc.begin(&h_gr)) return r;
  auto* h_td = reinterpret_cast<TxDesc*>(h_gr + V);
  auto* h_pd = reinterpret_cast<PuschTxDesc*>(h_td + V);
  auto* d_gr = g->desc.dev<GrantDev>();
  auto* d_td = reinterpret_cast<const TxDesc*>(d_gr + V);
  auto* d_pd = reinterpret_cast<const PuschTxDesc*>(d_td + V);
  std::vector<srslte_hip_cbsegm_t> segs(nof_grants);
  std::vector<uint32_t>            by_k(nof_grants), by_l(nof_grants);
  uint32_t                         max_M = 0;
  bool                             any_cqi = false;
  for (uint32_t p = 0; p < nof_grants; p++) {
    const srslte_hip_ul_grant_t& gr = grants[p];
    by_k[p] = by_l[p] = p;
    if (gr.sf >= nof_sf || gr.L_prb == 0 || !srslte_hip_dft_precoding_valid_prb(gr.L_prb) || gr.n_prb + gr.L_prb > P || gr.n_prb_slot1 + gr.L_prb > P ||
        gr.n_dmrs >= 8 || gr.mod < 1 || gr.mod > 3 || gr.rv > 3 || (gr.tbs == 0 && gr.cqi_len == 0) || gr.tbs > q->cfg.tbs || (gr.tbs % 8) || tb_stride < gr.tbs / 8 ||
        srslte_hip_cbsegm(&segs[p], gr.tbs) || segs[p].F || segs[p].C2 || segs[p].C > g->Cmax || (gr.ack_len && !d_ack) || (gr.ri_len && !d_ri) ||
        (gr.cqi_len && !d_cqi)) {
      hip_log("[srslte_hip] ul_tx grants: entry %u: unsupported grant (subframe %u of %u, L_prb %u at %u / %u, mod %d, tbs %u, rv %u)\n", p, gr.sf, nof_sf, gr.L_prb,
              gr.n_prb, gr.n_prb_slot1, gr.mod, gr.tbs, gr.rv);
      return SRSLTE_ERROR_INVALID_INPUTS;
    }
    max_M = 12 * gr.L_prb > max_M ? 12 * gr.L_prb : max_M;
    any_cqi = any_cqi || gr.cqi_len;
  }
  // code-block slots in block-length order (one encoder launch per length), symbol buffers in L_prb order (one transform-precoding launch per size)
  std::stable_sort(by_k.begin(), by_k.end(), [&](uint32_t a, uint32_t b) { return segs[a].K1 < segs[b].K1; });
  std::stable_sort(by_l.begin(), by_l.end(), [&](uint32_t a, uint32_t b) { return grants[a].L_prb < grants[b].L_prb; });
  uint32_t cb0 = 0, zoff = 0;
  for (uint32_t i = 0; i < nof_grants; i++) {
    h_td[by_k[i]].cb0 = (int)cb0;
    cb0 += segs[by_k[i]].C;
    h_pd[by_l[i]].zoff = (int)zoff;
    zoff += nsymb * 12 * grants[by_l[i]].L_prb;
  }
  for (uint32_t p = 0; p < nof_grants; p++) {
    const srslte_hip_ul_grant_t& gr = grants[p];
    const uint32_t               K = segs[p].K1, C = segs[p].C, nof_re = nsymb * 12 * gr.L_prb;
    GrantDev&                    gd = h_gr[p];
    memset(&gd, 0, sizeof(gd));
    gd.sf_idx = (int)((tti0 + gr.sf) % 10); gd.rnti = gr.rnti;
    // tbs = 0: a PUSCH without UL-SCH data (C = 0) - the Q' rules of 36.212 5.2.4.1 (pusch_uci_host.cpp), no code blocks
    srslte_hip_pusch_uci_res_t uci;
    if (pusch_pipeline_uci(gr, nsymb, segs[p], &uci)) {
      hip_log("[srslte_hip] ul_tx grants: entry %u: invalid UCI configuration\n", p);
      return SRSLTE_ERROR_INVALID_INPUTS;
    }
    TxDesc& td = h_td[p];
    td.rm      = C ? g->rm_table(K, gr.rv) : nullptr;
    if (C && !td.rm) return SRSLTE_ERROR;
    td.row = (int)p; td.sf = (int)gr.sf; td.tbs = (int)gr.tbs; td.C = (int)C; td.K = (int)K; td.rlenB = (int)((C <= 1 ? K : K - 24) / 8);
    td.nre = (int)nof_re; td.mod = gr.mod; td.Qm = 2 * gr.mod;
    PuschTxDesc& pd = h_pd[p];
    pd.M_sc = 12 * (int)gr.L_prb; pd.n_prb = (int)gr.n_prb; pd.n_prb1 = (int)gr.n_prb_slot1; pd.syms_lo = (int)uci.syms_lo; pd.C_lo = (int)uci.C_lo;
    pd.Qp_cqi = (int)uci.Qp_cqi; pd.cqi_O = (int)gr.cqi_len; pd.cqi_w = nullptr; pd.cqi_wlen = 1; pd.sf_idx = gd.sf_idx;
    pd.ack.O = (int)gr.ack_len; pd.ack.Qprime = (int)uci.Qp_ack; pd.ri.O = (int)gr.ri_len; pd.ri.Qprime = (int)uci.Qp_ri;
    if (gr.cqi_len > 11) { // the CQI report's rate matching (cqi_rm_conv_order), read circularly by the kernel
      auto cw = g->cqi_w.find(gr.cqi_len);
      if (cw == g->cqi_w.end()) {
        DevBuf<uint16_t> d;
        if (upload(d, cqi_rm_conv_order(gr.cqi_len))) return SRSLTE_ERROR;
        cw = g->cqi_w.emplace(gr.cqi_len, std::move(d)).first;
      }
      pd.cqi_w = cw->second; pd.cqi_wlen = (int)cw->second.size();
    }
    const void* d_r = nullptr;
    if (int r = chest_ul_dmrs_table_cached(q->dmrs, gr.L_prb, gr.n_dmrs, &d_r)) return r;
    pd.dmrs = (const cf32*)d_r;
  }
  if (int r = g->desc.commit(g->desc_bytes, st)) return r;
  HIP_TRY(hipMemsetAsync(q->d_grid, 0, sizeof(cf32) * (size_t)2 * q->g.nsl * 12 * P * nof_sf, st)); // ue_ul.c:320: the grid is cleared, then pusch_put
  if (nof_grants) {
    hipLaunchKernelGGL(scr_gen_kernel, dim3(ceil_div((int)g->words, 256), nof_grants), dim3(256), 0, st, (const GrantDev*)d_gr, (const uint32_t*)g->d_basis,
                       g->d_scr, (int)g->words, (int)q->cfg.cell_id);
    if (any_cqi) {
      hipLaunchKernelGGL(pusch_cqi_encode_grants_kernel, dim3(nof_grants), dim3(256), 0, st, d_cqi, g->d_qcqi, (int)g->cqi_stride, (const PuschTxDesc*)d_pd,
                         (const TxDesc*)d_td);
    }
    hipLaunchKernelGGL(tx_tbcrc_grants_kernel, dim3(nof_grants), dim3(256), 0, st, d_tb, (int)tb_stride, (const TxDesc*)d_td, g->d_tbcrc);
    hipLaunchKernelGGL(tx_seg_grants_kernel, dim3(g->Cmax, nof_grants), dim3(256), 0, st, d_tb, (int)tb_stride, (const uint32_t*)g->d_tbcrc, (const TxDesc*)d_td,
                       g->d_cb, (int)g->cb_stride);
    LAUNCH_CHECK();
    for (uint32_t i = 0; i < nof_grants;) { // the encoder: runs of equal block length
      uint32_t j = i, n = 0;
      while (j < nof_grants && segs[by_k[j]].K1 == segs[by_k[i]].K1) n += segs[by_k[j++]].C;
      const size_t s0 = (size_t)h_td[by_k[i]].cb0;
      if (n == 0) { // PUSCHs without UL-SCH data
        i = j;
        continue;
      }
      if (int r = srslte_hip_tcod_encode_bytes_batch(g->d_cb + s0 * g->cb_stride, g->cb_stride, g->d_parity + s0 * g->par_stride, g->par_stride,
                                                     g->d_sys_tail + s0, segs[by_k[i]].K1, n, stream))
        return r;
      i = j;
    }
    hipLaunchKernelGGL(pusch_tx_mod_grants_kernel, dim3(ceil_div((int)max_M, 256), nsymb, nof_grants), dim3(256), 0, st, (const uint8_t*)g->d_cb,
                       (const uint8_t*)g->d_parity, (const uint8_t*)g->d_sys_tail, (const uint32_t*)g->d_scr, (int)g->words, g->d_d, (const PuschTxDesc*)d_pd,
                       (const TxDesc*)d_td, g->lv, (int)nsymb, (int)g->cb_stride, (int)g->par_stride, d_ack, d_ri, (const uint8_t*)g->d_qcqi, (int)g->cqi_stride);
    LAUNCH_CHECK();
    for (uint32_t i = 0; i < nof_grants;) { // transform precoding: runs of equal L_prb (srslte_dft_precoding_init_tx: forward, 1/sqrt(N))
      uint32_t j = i + 1;
      while (j < nof_grants && grants[by_l[j]].L_prb == grants[by_l[i]].L_prb) j++;
      const size_t off = (size_t)h_pd[by_l[i]].zoff;
      if (int r = srslte_hip_dft_precoding_batch(g->d_d + off, g->d_z + off, grants[by_l[i]].L_prb, nsymb * (j - i), 1, stream)) return r;
      i = j;
    }
    hipLaunchKernelGGL(pusch_tx_scatter_kernel, dim3(ceil_div((int)max_M, 256), 2 * q->g.nsl, nof_grants), dim3(256), 0, st, (const cf32*)g->d_z, q->d_grid,
                       (const PuschTxDesc*)d_pd, (const TxDesc*)d_td, 12 * (int)P, (int)nsymb, q->g.nsl);
    LAUNCH_CHECK();
  }
  return srslte_hip_ofdm_tx_sf_batch(q->ofdm, q->d_grid, d_iq, (int)nof_sf, stream);
}
