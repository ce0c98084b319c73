// Fragment of pdsch.hip (same translation unit): the PDSCH receive pipeline object with its fixed-grant entry points (stages, HARQ, two codewords,
// grids) and the state of the grants modes.
// Device / host resources of the per-subframe-grant mode (srslte_hip_dl_rx_batch_grants)
struct GrantsState {
  srslte_hip_tdec_t* tdec = nullptr; // any block length up to 6144
  uint32_t           Cmax = 0, stride = 0, max_re = 0, max_bits = 0, words = 0;
  uint32_t           V = 0; // per-subframe slots: max_batch, twice that on a cell where two-layer grants can occur (codeword 1 of subframe b: slot max_batch + b)
  DevBuf<uint32_t>   d_relist, d_scr, d_basis, d_cb_iters;
  DevBuf<int16_t>    d_e, d_w;
  DevBuf<uint8_t>    d_cb_bytes, d_cb_ok;
  DevBuf<float>      d_csi;     // [B][max_re], cfg.csi_enable
  DevBuf<uint32_t>   d_csi_max; // [B]
  size_t             desc_bytes = 0;
  DescStage          desc; // the descriptor block: pinned host copies and the device block, desc_bytes + 16 each; a kernel of the call copies
  bool               tb_direct = false; // 16-bit calls: the decoders assemble the transport blocks (environment SRSLTE_HIP_GRANTS_TB_DIRECT=0: the assembly kernel, for A/B and tests)
  std::map<std::pair<uint32_t, uint32_t>, DevBuf<uint32_t>> rm_tbl;  // (K, rv) -> slot table in the layout of that K's decoder
  std::map<uint32_t, DevBuf<uint32_t>>                      crc_fac; // tbs -> tb_crc_bytes_kernel's 256 chunk weights
  ~GrantsState() { srslte_hip_tdec_destroy(tdec); }
};

struct srslte_hip_dl_rx {
  srslte_hip_dl_rx_cfg_t cfg   = {};
  srslte_hip_ofdm_t*     ofdm  = nullptr;
  srslte_hip_chest_dl_t* chest = nullptr;
  PdschGeom              pg    = {};
  DevBuf<uint32_t>       d_idx[3];
  // What the demapper (stage 2) leaves per codeword, and the codeword's back end (stages 3-5). Two-layer modes with two transport blocks: ncw = 2
  struct Codeword {
    DevBuf<uint32_t> d_scr;     // scrambling sequence q = the codeword (36.211 6.3.1)
    DevBuf<int16_t>  d_e;       // [B][max_bits] + 16
    DevBuf<cf32>     d_d;       // [B][max_re] equalised symbols, srslte_hip_dl_rx_keep_symbols
    DevBuf<float>    d_csi;     // [B][max_re], cfg.csi_enable
    DevBuf<uint32_t> d_csi_max; // [B]
    SchRxFixed       sch;
  } cw[2];
  int                    ncw = 1;
  DevBuf<cf32>           d_grid, d_ce;
  DevBuf<cf32>           d_ce_full; // debug view of a compact d_ce (pg.ce_nre != 0) expanded to whole grids, made on request
  DevBuf<ChestResDev>    d_res;
  std::unique_ptr<GrantsState> gs; // srslte_hip_dl_rx_batch_grants: created on first use
  srslte_hip_csi_t*      csi = nullptr; // srslte_hip_dl_rx_csi_batch: made on first use
  uint32_t               est_nof_sf = 0; // subframes the last estimator run (stage 1) left in d_ce / d_res; 0: none yet
  float                  csi_offset = 0.f; // snr_to_cqi_offset of srslte_hip_dl_rx_csi_batch
  ~srslte_hip_dl_rx()
  {
    srslte_hip_ofdm_destroy(ofdm);
    srslte_hip_chest_dl_destroy(chest);
    srslte_hip_csi_destroy(csi);
  }
};

// What one call of the fixed-grant stages does beyond their arguments: where the resource grids come from and the HARQ of each codeword
struct DlRxCall {
  const cf32* grid = nullptr; // resource grids supplied by the caller (srslte_hip_dl_rx_grid_batch), or null: the object's d_grid
  SchHarq     harq[2];
};

extern "C" void srslte_hip_dl_rx_destroy(srslte_hip_dl_rx_t* q) { delete q; }

// phy_hip.h, "Sample formats": d_iq of every entry point of the object is in the OFDM object's format from here on
extern "C" int srslte_hip_dl_rx_set_iq_format(srslte_hip_dl_rx_t* q, int format, float scale)
{
  return q ? srslte_hip_ofdm_set_sample_format(q->ofdm, format, scale) : SRSLTE_ERROR_INVALID_INPUTS;
}

extern "C" srslte_hip_dl_rx_t* srslte_hip_dl_rx_create(const srslte_hip_dl_rx_cfg_t* cfg)
{
  if (!cfg || cfg->max_batch == 0 || cfg->mod < 1 || cfg->mod > 4 || cfg->max_iterations == 0 || cfg->nof_rx_antennas > 4 || cfg->nof_ports > 4 ||
      cfg->nof_ports == 3) {
    hip_log("[srslte_hip] dl_rx: invalid configuration\n");
    return nullptr;
  }
  const bool mimo = cfg->tx_scheme != 0, two = mimo && cfg->tbs2 != 0;
  if (mimo) { // what ra_dl.c:556-600 and precoding.c:1710-1759,:1087-1114 let through
    const bool ok = (cfg->tx_scheme == 2 || cfg->tx_scheme == 3) && cfg->nof_ports == 2 && cfg->nof_rx_antennas == 2 &&
                    (cfg->tx_scheme == 2 || two) && (two ? cfg->pmi < 2 : cfg->pmi < 4) && (!two || (cfg->mod2 >= 1 && cfg->mod2 <= 4));
    if (!ok) {
      hip_log("[srslte_hip] dl_rx: two-layer modes need a 2-port cell and 2 receive antennas; CDD with two transport blocks, "
              "multiplexing with two (pmi 0-1) or one (pmi 0-3)\n");
      return nullptr;
    }
  }
  std::unique_ptr<srslte_hip_dl_rx> q(new srslte_hip_dl_rx());
  q->cfg = *cfg;
  q->ncw = two ? 2 : 1;
  srslte_hip_cbsegm_t seg;
  if (fixed_grant_segmentation("dl_rx", cfg->tbs, &seg) || (two && fixed_grant_segmentation("dl_rx", cfg->tbs2, &seg))) return nullptr;
  const uint32_t P = cfg->nof_prb, nre = 12 * P, B = cfg->max_batch;
  const uint32_t lstart = cfg->cfi + (P < 10 ? 1 : 0); // SRSLTE_NOF_CTRL_SYMBOLS, phy_common.h:143
  const uint32_t nrx    = cfg->nof_rx_antennas ? cfg->nof_rx_antennas : 1;
  const uint32_t npt    = cfg->nof_ports ? cfg->nof_ports : 1;
  const uint32_t nsl    = (cfg->cp_ext || cfg->mbsfn) ? 6 : 7; // symbols per slot (an MBSFN subframe has the extended CP's 12 on any cell)
  if (cfg->mbsfn && (npt != 1 || mimo || cfg->tdd || cfg->llr_8bit || cfg->csi_enable || cfg->power_scale || cfg->mbsfn_area_id > 255 ||
                     cfg->non_mbsfn_region < 1 || cfg->non_mbsfn_region > 2)) {
    // srslte_pmch_decode: one port (pmch.c:159), int16 LLRs (:377), no CSI weighting, no power allocation
    hip_log("[srslte_hip] dl_rx: an MBSFN pipeline is single-port FDD with 16-bit LLRs, area id 0-255, a non-MBSFN region of 1 or 2 symbols\n");
    return nullptr;
  }
  if (cfg->mbsfn) q->cfg.chest_cfg.interpolate_subframe = 1;
  if (cfg->tdd && (cfg->tdd_sf_config > 6 || cfg->tdd_ss_config > 9)) {
    hip_log("[srslte_hip] dl_rx: TDD uplink-downlink configuration %u / special-subframe configuration %u\n", cfg->tdd_sf_config, cfg->tdd_ss_config);
    return nullptr;
  }
  q->ofdm  = srslte_hip_ofdm_create((int)P, nsl == 6 ? 0 : 1, 1);
  q->chest = srslte_hip_chest_dl_create(cfg->cell_id, P, npt, cfg->cp_ext ? 0 : 1);
  if (q->chest && cfg->tdd) srslte_hip_chest_dl_set_tdd(q->chest, (int)cfg->tdd_sf_config, (int)cfg->tdd_ss_config);
  if (cfg->mbsfn && q->ofdm && q->chest &&
      (srslte_hip_ofdm_set_mbsfn(q->ofdm, 1, (int)cfg->non_mbsfn_region) || srslte_hip_chest_dl_set_mbsfn_area_id(q->chest, (uint16_t)cfg->mbsfn_area_id))) {
    srslte_hip_chest_dl_destroy(q->chest);
    q->chest = nullptr;
  }
  bool ok = q->ofdm && q->chest;
  // RE lists
  SchRxFixed::Cfg sc = {};
  const uint32_t  rep_sf[3] = {0, 5, 1};
  for (int c = 0; c < 3 && ok; c++) {
    std::vector<uint32_t> idx;
    if (cfg->mbsfn) pmch_re_indices(P, lstart, idx); // the same list for every subframe index: no PSS / SSS / PBCH in an MBSFN subframe
    else pdsch_re_indices(cfg->cell_id, P, npt, rep_sf[c], lstart, idx, nsl);
    q->pg.cls[c].nof_re = (int)idx.size();
    sc.nof_re[c]        = (uint32_t)idx.size();
    sc.max_re           = idx.size() > sc.max_re ? (uint32_t)idx.size() : sc.max_re;
    ok                  = upload(q->d_idx[c], idx) == SRSLTE_SUCCESS;
    q->pg.cls[c].idx    = q->d_idx[c];
  }
  const uint32_t max_re = sc.max_re;
  const size_t   glen   = (size_t)2 * nsl * nre;
  ok = ok && !q->d_grid.alloc(glen * B * nrx) && !q->d_ce.alloc(glen * B * nrx * npt) &&
       hipMemset(q->d_ce, 0, sizeof(cf32) * glen * B * nrx * npt) == hipSuccess && /* 4 ports + interpolate_subframe: ports 2/3 keep what is there */
       !q->d_res.alloc(B);
  // per codeword: scrambling sequences, LLR rows, CSI weights and the back end, which waits for the device's memsets - the one above among them
  sc.max_batch = B; sc.max_iterations = cfg->max_iterations; sc.llr_8bit = cfg->llr_8bit != 0;
  // code-block split in units of Qm N_L bits: N_L = 2 for transmit diversity, 1 where nof_layers == nof_tb (srslte_dlsch_decode2, sch.c:507-531)
  sc.Nl = (npt > 1 && !mimo) ? 2 : 1;
  uint32_t scr_words[2] = {0, 0};
  for (int c = 0; c < q->ncw && ok; c++) {
    srslte_hip_dl_rx::Codeword& w = q->cw[c];
    sc.mod = c ? cfg->mod2 : cfg->mod; sc.tbs = c ? cfg->tbs2 : cfg->tbs; sc.Qm = 2 * (uint32_t)sc.mod;
    sc.max_bits  = (max_re * sc.Qm + 15) & ~15u;
    scr_words[c] = (max_re * sc.Qm + 31) / 32 + 1; // spare word: the demapper reads two per RE
    // scrambling sequences, one per subframe index (sequences.c:58-60, pdsch.c:469); srslte_sequence_pmch (sequences.c:76-80) with nslot = 2 sf
    // (pmch.c:263-275) for an MBSFN pipeline
    std::vector<uint32_t> scr;
    const uint32_t        c_init0 = cfg->mbsfn ? cfg->mbsfn_area_id : ((uint32_t)cfg->rnti << 14) + ((uint32_t)c << 13) + cfg->cell_id;
    lte_scr_table([&](uint32_t sf) { return c_init0 + (sf << 9); }, max_re * sc.Qm, scr_words[c], scr);
    ok = upload(w.d_scr, scr) == SRSLTE_SUCCESS && !w.d_e.alloc((size_t)sc.max_bits * B + 16); /* +16: rm_rx_lds_kernel reads whole 16-byte words */
    if (ok && cfg->csi_enable) ok = !w.d_csi.alloc((size_t)max_re * B) && !w.d_csi_max.alloc(B);
    sc.csi = w.d_csi; sc.csi_max = w.d_csi_max;
    // the first codeword of a single-codeword, single-layer pipeline: compact parity, transport blocks assembled by the decoders
    sc.may_compact = c == 0; sc.may_direct = !two && !mimo;
    ok = ok && w.sch.init(sc) == SRSLTE_SUCCESS;
  }
  if (!ok) {
    hip_log("[srslte_hip] dl_rx: initialisation failed\n");
    return nullptr;
  }
  const SchRxFixed& s0 = q->cw[0].sch;
  q->pg.grid_len = (int)glen; q->pg.max_re = (int)max_re; q->pg.max_bits = s0.rg.max_bits; q->pg.mod = cfg->mod; q->pg.Qm = s0.rg.Qm;
  q->pg.mmse = cfg->mmse; q->pg.scr_words = (int)scr_words[0]; q->pg.nof_rx = (int)nrx; q->pg.nof_ports = (int)npt;
  q->pg.csi = q->cw[0].d_csi; q->pg.csi_max = q->cw[0].d_csi_max;
  // Without interpolate_subframe the estimator gives every symbol of a subframe the same row of estimates (chest_dl.c:467-471): a single-port
  // pipeline keeps that row only - the estimator writes 12 nof_prb values per subframe and antenna instead of 14 times as many, the demapper
  // reads the row for every symbol
  const bool compact = npt == 1 && !q->cfg.chest_cfg.interpolate_subframe;
  q->pg.ce_len = compact ? (int)(12 * P) : (int)glen; q->pg.ce_nre = compact ? (int)(12 * P) : 0;
  q->pg.ce_magic = compact ? (uint32_t)((0x100000000ull + 12 * P - 1) / (12 * P)) : 0;
  // apply_power_allocation (pdsch.c:518-554) with rho_b = 1: pdsch_scaling = rho_a = 10^(p_a/20), times sqrt(2) for a 2-port cell
  q->pg.inv_scaling = cfg->power_scale ? 1.0f / (powf(10.0f, cfg->p_a / 20.0f) * (npt == 1 ? 1.0f : sqrtf(2.0f))) : 1.0f;
  if (mimo) {
    q->pg.tx_scheme = cfg->tx_scheme; q->pg.nof_tb = two ? 2 : 1;
    q->pg.codebook_idx = (int)(two ? cfg->pmi + 1 : cfg->pmi); // pdsch.c:914
    if (two) {
      const SchRxFixed& s1 = q->cw[1].sch;
      q->pg.mod1 = cfg->mod2; q->pg.Qm1 = s1.rg.Qm; q->pg.max_bits1 = s1.rg.max_bits; q->pg.scr_words1 = (int)scr_words[1];
      q->pg.scr1 = q->cw[1].d_scr; q->pg.csi1 = q->cw[1].d_csi; q->pg.csi_max1 = q->cw[1].d_csi_max;
    }
  }
  return q.release();
}

extern "C" int srslte_hip_dl_rx_keep_symbols(srslte_hip_dl_rx_t* q, int enable)
{
  if (!q) return SRSLTE_ERROR_INVALID_INPUTS;
  for (int c = q->ncw - 1; c >= 0; c--) {
    DevBuf<cf32>& d_d = q->cw[c].d_d;
    if (enable && !d_d && d_d.alloc((size_t)q->pg.max_re * q->cfg.max_batch)) {
      hip_log("[srslte_hip] dl_rx: no device memory for the equalised symbols\n");
      return SRSLTE_ERROR;
    }
    if (!enable) d_d = DevBuf<cf32>();
  }
  return SRSLTE_SUCCESS;
}

extern "C" uint32_t srslte_hip_dl_rx_nof_re(const srslte_hip_dl_rx_t* q, uint32_t sf_idx)
{
  return q ? (uint32_t)q->pg.cls[sf_idx % 10 == 0 ? 0 : (sf_idx % 10 == 5 ? 1 : 2)].nof_re : 0;
}

// debug view: a compact estimate buffer ([B][nrx][nre]) as the whole grids the tests compare ([B][nrx][symbols][nre]), every symbol the row
__global__ void ce_expand_kernel(const cf32* __restrict__ row, cf32* __restrict__ full, int nre, int nsym)
{
  const int plane = blockIdx.y;
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < nre; k += gridDim.x * blockDim.x) {
    const cf32 v = row[(size_t)plane * nre + k];
    for (int l = 0; l < nsym; l++) full[((size_t)plane * nsym + l) * nre + k] = v;
  }
}
static const void* dl_rx_ce_full(srslte_hip_dl_rx_t* q)
{
  const size_t planes = (size_t)q->cfg.max_batch * q->pg.nof_rx;
  if (hipDeviceSynchronize() != hipSuccess) return nullptr;
  if (!q->d_ce_full && q->d_ce_full.alloc(planes * q->pg.grid_len)) return nullptr;
  hipLaunchKernelGGL(ce_expand_kernel, dim3(ceil_div(q->pg.ce_nre, 256), (unsigned)planes), dim3(256), 0, 0, (const cf32*)q->d_ce, q->d_ce_full, q->pg.ce_nre,
                     q->pg.grid_len / q->pg.ce_nre);
  return hipDeviceSynchronize() == hipSuccess ? q->d_ce_full : nullptr;
}

extern "C" int srslte_hip_dl_rx_parity_compact(const srslte_hip_dl_rx_t* q) { return q ? q->cw[0].sch.last_compact : 0; }

extern "C" uint32_t srslte_hip_rm_parity_compact_limit(uint32_t K)
{
  RmParityCompact c;
  return lte_cb_index(K) >= 0 && lte_qpp_table[lte_cb_index(K)].K == K && rm_parity_compact(K, c) ? c.e_lim : 0;
}

extern "C" const void* srslte_hip_dl_rx_debug_buffer(const srslte_hip_dl_rx_t* q, int which)
{
  if (!q) return nullptr;
  const int c = which >= 100 ? 1 : 0; // 100 + n: the second codeword's buffers 3 .. 10 (it has no grids, estimates or grants mode of its own)
  which -= 100 * c;
  if (c && (q->ncw < 2 || which < 3 || which > 10)) return nullptr;
  srslte_hip_dl_rx_t*         m = const_cast<srslte_hip_dl_rx_t*>(q);
  srslte_hip_dl_rx::Codeword& w = m->cw[c];
  switch (which) {
    case 0: return q->d_grid;
    case 1: return q->pg.ce_nre ? dl_rx_ce_full(m) : q->d_ce;
    case 2: return q->d_res;
    case 3: return w.d_d;
    case 4: return w.d_e;
    case 5: // the whole layout, whatever the last call left
      if (hipDeviceSynchronize() != hipSuccess || w.sch.w_whole(0) || hipDeviceSynchronize() != hipSuccess) return nullptr;
      return w.sch.d_w;
    case 6: return w.sch.d_cb_iters;
    case 7: return w.sch.d_cb_ok;
    case 8: return w.sch.d_cb_bytes;
    case 9: return w.d_csi;
    case 10: return w.d_csi_max;
    // grants mode (srslte_hip_dl_rx_batch_grants): 11 e [nof_sf][max_bits], 12 w [nof_sf * Cmax][stride], 13 cb iters, 14 cb ok,
    // 15 RE lists [nof_sf][max_re], 16 scrambling words [nof_sf][words]
    case 11: return q->gs ? q->gs->d_e : nullptr;
    case 12: return q->gs ? q->gs->d_w : nullptr;
    case 13: return q->gs ? q->gs->d_cb_iters : nullptr;
    case 14: return q->gs ? q->gs->d_cb_ok : nullptr;
    case 15: return q->gs ? q->gs->d_relist : nullptr;
    case 16: return q->gs ? q->gs->d_scr : nullptr;
    case 17: return q->gs ? q->gs->d_csi : nullptr;
  }
  return nullptr;
}

// Stage 2: the demapper of the object's transmission scheme and port count for its LLR type
template <typename LLR>
static void dl_rx_demod_launch(srslte_hip_dl_rx_t* q, const PdschGeom& g, const cf32* grid, uint32_t nof_sf, hipStream_t st)
{
  const cf32*        ce  = q->d_ce;
  const ChestResDev* res = q->d_res;
  const uint32_t*    scr = q->cw[0].d_scr;
  cf32*              d   = q->cw[0].d_d;
  LLR*               e   = reinterpret_cast<LLR*>(q->cw[0].d_e.get());
  if (g.tx_scheme) { // pdsch.c:760-779: q->llr_is_8bit with any transmission scheme
    hipLaunchKernelGGL(pdsch_demod_mimo_kernel<LLR>, dim3(ceil_div(g.max_re, 256), nof_sf), dim3(256), 0, st, grid, ce, res, scr, d, q->cw[1].d_d.get(), e,
                       reinterpret_cast<LLR*>(q->cw[1].d_e.get()), g);
  } else if (g.nof_ports == 4) {
    hipLaunchKernelGGL(pdsch_demod_div4_kernel<LLR>, dim3(ceil_div(g.max_re, 1024), nof_sf), dim3(256), 0, st, grid, ce, scr, d, e, g);
  } else if (g.nof_ports == 2) {
    hipLaunchKernelGGL(pdsch_demod_div_kernel<LLR>, dim3(ceil_div(g.max_re, 512), nof_sf), dim3(256), 0, st, grid, ce, scr, d, e, g);
  } else {
    hipLaunchKernelGGL(pdsch_demod_kernel<LLR>, dim3(ceil_div(g.max_re, 256), nof_sf), dim3(256), 0, st, grid, ce, res, scr, d, e, g);
  }
}

// The stages of one call. Stages 3-5 run the second codeword's launch in front of the first's
static int dl_rx_stage(srslte_hip_dl_rx_t* q, int stage, const void* d_iq, uint32_t tti0, uint32_t nof_sf, uint8_t* d_tb, uint32_t tb_stride, uint8_t* d_tb_ok,
                       void* stream, const DlRxCall& call)
{
  if (!q || nof_sf > q->cfg.max_batch) return SRSLTE_ERROR_INVALID_INPUTS;
  if (nof_sf == 0) return SRSLTE_SUCCESS;
  hipStream_t st   = (hipStream_t)stream;
  const cf32* grid = call.grid ? call.grid : q->d_grid;
  if (q->cfg.tdd && stage >= 2) { // OFDM and estimator serve the grants mode; the fixed grant's RE lists, sequences and tables are per FDD subframe class
    hip_log("[srslte_hip] dl_rx: a TDD cell is received through the per-subframe-grant entry points (srslte_hip_dl_rx_batch_grants*)\n");
    return SRSLTE_ERROR;
  }
  // rows nof_sf .. 2 nof_sf - 1 of d_tb / d_tb_ok: the second transport block of every subframe
  uint8_t* const tb[2] = {d_tb, d_tb ? d_tb + (size_t)nof_sf * tb_stride : nullptr};
  uint8_t* const tb_ok[2] = {d_tb_ok, d_tb_ok ? d_tb_ok + nof_sf : nullptr};
  switch (stage) {
    case 0: return srslte_hip_ofdm_rx_sf_batch(q->ofdm, d_iq, q->d_grid, (int)nof_sf * q->pg.nof_rx, stream); // [sf][rx] = nof_sf * nof_rx subframes
    case 1: {
      q->est_nof_sf = 0; // srslte_hip_dl_rx_csi_batch measures what a successful estimator run left, nothing after a failed one
      int r;
      if (q->cfg.mbsfn) { // estimate_port_mbsfn; the result's noise figure is the mean of the antennas' REFS estimates (get_noise, chest_dl.c:747-758)
        srslte_hip_chest_dl_cfg_t mc = q->cfg.chest_cfg;
        mc.mbsfn_area_id             = (uint16_t)q->cfg.mbsfn_area_id;
        r = chest_dl_estimate_mbsfn_rows(q->chest, &mc, tti0, grid, q->d_ce, (int)nof_sf, q->pg.nof_rx, 6, q->d_res, stream);
      } else {
        r = chest_dl_estimate_batch_rows(q->chest, &q->cfg.chest_cfg, tti0, grid, q->d_ce, q->d_res, (int)nof_sf, q->pg.nof_rx, q->pg.ce_nre != 0, stream);
      }
      if (r == SRSLTE_SUCCESS) q->est_nof_sf = nof_sf;
      return r;
    }
    case 2: {
      PdschGeom g = q->pg;
      g.tti0      = (int)tti0;
      if (g.csi_max) HIP_TRY(hipMemsetAsync(g.csi_max, 0, sizeof(uint32_t) * nof_sf, st));
      if (g.tx_scheme && g.csi_max1) HIP_TRY(hipMemsetAsync(g.csi_max1, 0, sizeof(uint32_t) * nof_sf, st));
      if (q->cfg.llr_8bit) dl_rx_demod_launch<int8_t>(q, g, grid, nof_sf, st);
      else dl_rx_demod_launch<int16_t>(q, g, grid, nof_sf, st);
      LAUNCH_CHECK();
      return SRSLTE_SUCCESS;
    }
    case 3:
    case 4:
    case 5:
      for (int c = 0; c < q->ncw && stage == 5; c++) { // every refusal before the first launch
        if (!d_tb || !d_tb_ok || tb_stride < q->cw[c].sch.cfg.tbs / 8 + 6) return SRSLTE_ERROR_INVALID_INPUTS;
      }
      for (int c = q->ncw - 1; c >= 0; c--) {
        SchRxFixed& s = q->cw[c].sch;
        const int   r = stage == 3 ? s.dematch(q->cw[c].d_e, tti0, nof_sf, call.harq[c], st)
                                   : (stage == 4 ? s.decode(nof_sf, call.harq[c], tb[c], tb_stride, tb_ok[c], st) : s.assemble(nof_sf, tb[c], tb_stride, tb_ok[c], st));
        if (r) return r;
      }
      return SRSLTE_SUCCESS;
  }
  return SRSLTE_ERROR_INVALID_INPUTS;
}

// Stage launchers, also used one by one by bench.py to time each kernel in isolation: rv 0, new data, the object's own grids
extern "C" int srslte_hip_dl_rx_stage(srslte_hip_dl_rx_t* q, int stage, const void* d_iq, uint32_t tti0, uint32_t nof_sf, uint8_t* d_tb,
                                      uint32_t tb_stride, uint8_t* d_tb_ok, void* stream)
{
  return dl_rx_stage(q, stage, d_iq, tti0, nof_sf, d_tb, tb_stride, d_tb_ok, stream, DlRxCall());
}

extern "C" int srslte_hip_dl_rx_batch(srslte_hip_dl_rx_t* q, const void* d_iq, uint32_t tti0, uint32_t nof_sf, uint8_t* d_tb,
                                      uint32_t tb_stride, uint8_t* d_tb_ok, void* stream)
{
  return srslte_hip_dl_rx_batch_harq(q, d_iq, tti0, nof_sf, 0, 1, d_tb, tb_stride, d_tb_ok, stream);
}

// HARQ (decode_tb_cb, sch.c:299-414, on a srslte_softbuffer_rx_t per transport block, softbuffer.c:46-150): slot b of the object keeps
// its code blocks' soft buffers, CRC flags and decoded bytes between calls. new_data != 0 starts new transport blocks (what the MAC's
// srslte_softbuffer_rx_reset_tbs does on a toggled NDI): buffers are overwritten, every block is decoded. new_data == 0 is a
// retransmission with redundancy version rv: the de-matched LLRs are ADDED to the kept soft buffers (rm_turbo.c:407-409), blocks whose
// CRC already passed are neither combined nor decoded again. srslte_hip_dl_rx_batch is rv 0 / new data.
extern "C" int srslte_hip_dl_rx_batch_harq(srslte_hip_dl_rx_t* q, const void* d_iq, uint32_t tti0, uint32_t nof_sf, uint32_t rv, int new_data,
                                           uint8_t* d_tb, uint32_t tb_stride, uint8_t* d_tb_ok, void* stream)
{
  if (!q || !d_iq || !d_tb || !d_tb_ok || rv > 3) return SRSLTE_ERROR_INVALID_INPUTS;
  const uint32_t rv2[2] = {rv, rv};
  const int      nd2[2] = {new_data, new_data};
  return srslte_hip_dl_rx_batch_harq2(q, d_iq, tti0, nof_sf, rv2, nd2, d_tb, tb_stride, d_tb_ok, stream);
}

// the same with a redundancy version and a new-data flag per transport block (two-layer modes: each block has its own HARQ process state,
// srslte_pdsch_cfg_t.softbuffers.rx[0 / 1] and grant.tb[0 / 1].rv)
extern "C" int srslte_hip_dl_rx_batch_harq2(srslte_hip_dl_rx_t* q, const void* d_iq, uint32_t tti0, uint32_t nof_sf, const uint32_t rv[2],
                                            const int new_data[2], uint8_t* d_tb, uint32_t tb_stride, uint8_t* d_tb_ok, void* stream)
{
  if (!q || !d_iq || !d_tb || !d_tb_ok || !rv || !new_data || rv[0] > 3 || rv[1] > 3) return SRSLTE_ERROR_INVALID_INPUTS;
  DlRxCall call;
  for (int c = 0; c < q->ncw; c++) { // a table made on first use, or the refusal, before anything is queued
    call.harq[c] = {rv[c], new_data[c] ? 0 : 1};
    if (int r = q->cw[c].sch.ensure_rv(rv[c])) return r;
  }
  int r = SRSLTE_SUCCESS;
  for (int s = 0; s < 6 && !r; s++) r = dl_rx_stage(q, s, d_iq, tti0, nof_sf, d_tb, tb_stride, d_tb_ok, stream, call);
  return r;
}

// UE CSI feedback (csi.hip) on the estimates and noise figures of the last batch: one launch behind that batch's on the caller's stream
extern "C" int srslte_hip_dl_rx_csi_batch(srslte_hip_dl_rx_t* q, uint32_t nof_sf, srslte_hip_csi_res_t* d_out, void* stream)
{
  if (!q || !d_out || nof_sf == 0 || q->est_nof_sf == 0 || nof_sf > q->est_nof_sf) return SRSLTE_ERROR_INVALID_INPUTS;
  if (!q->csi) {
    q->csi = srslte_hip_csi_create(q->cfg.nof_prb, (uint32_t)q->pg.nof_ports, (uint32_t)q->pg.nof_rx, (q->cfg.cp_ext || q->cfg.mbsfn) ? 0 : 1);
    if (!q->csi) return SRSLTE_ERROR_INVALID_INPUTS;
  }
  if (int r = srslte_hip_csi_set_snr_to_cqi_offset(q->csi, q->csi_offset)) return r;
  return srslte_hip_csi_batch(q->csi, q->d_ce, q->d_res, nof_sf, d_out, stream);
}

extern "C" int srslte_hip_dl_rx_set_snr_to_cqi_offset(srslte_hip_dl_rx_t* q, float offset)
{
  if (!q || !(offset == offset)) return SRSLTE_ERROR_INVALID_INPUTS;
  q->csi_offset = offset;
  return SRSLTE_SUCCESS;
}

// Same chain from resource grids already in the frequency domain (what follows srslte_ofdm_rx_sf in ue_dl.c:375-397): stages 1..5
extern "C" int srslte_hip_dl_rx_grid_batch(srslte_hip_dl_rx_t* q, const void* d_grid, uint32_t tti0, uint32_t nof_sf, uint8_t* d_tb,
                                           uint32_t tb_stride, uint8_t* d_tb_ok, void* stream)
{
  if (!q || !d_grid || !d_tb || !d_tb_ok) return SRSLTE_ERROR_INVALID_INPUTS;
  DlRxCall call;
  call.grid = (const cf32*)d_grid;
  int r     = SRSLTE_SUCCESS;
  for (int s = 1; s < 6 && r == SRSLTE_SUCCESS; s++) r = dl_rx_stage(q, s, nullptr, tti0, nof_sf, d_tb, tb_stride, d_tb_ok, stream, call);
  return r;
}
