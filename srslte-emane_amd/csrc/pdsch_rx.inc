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
  srslte_hip_tdec_t*     tdec  = nullptr;
  srslte_hip_cbsegm_t    seg   = {};
  PdschGeom              pg    = {};
  RmGeom                 rg    = {};
  TbGeom                 tg    = {};
  uint32_t               W = 0, in_stride = 0;
  DevBuf<uint32_t>       d_idx[3];
  DevBuf<uint32_t>       d_scr;
  DevBuf<uint32_t>       d_rm_tbl_rv[4]; // [0] made with the object; 1..3 built on first use (srslte_hip_dl_rx_batch_harq)
  uint32_t               harq_rv      = 0;
  int                    harq_combine = 0;
  // Punctured parity at a quarter of its rows (rm_parity_compact, pdsch_kernels.inc): whether this object's calls with rv 0 and new data take that
  // layout, its table, the subframe slots [0, w_compact_n) of d_w that are in it now (every other slot holds the whole layout) and what
  // the last rate de-matcher run (stage 3) chose
  bool                   pc_ok = false;
  RmParityCompact        pc    = {};
  DevBuf<uint32_t>       d_rm_tbl_pc;
  uint32_t               w_compact_n  = 0;
  int                    last_compact = 0;
  DevBuf<uint32_t>       d_tbcrc;
  DevBuf<cf32>           d_grid, d_ce, d_d;
  const uint8_t*         direct_tb = nullptr; // where the last decoder run (stage 4) assembled the transport blocks itself, or null: stage 5 has nothing to do then,
  const uint8_t*         direct_ok = nullptr; // if it is called with the same rows, verdicts, stride and subframe count as that run
  uint32_t               direct_stride = 0, direct_nof_sf = 0;
  DevBuf<cf32>           d_ce_full; // debug view of a compact d_ce (pg.ce_nre != 0) expanded to whole grids, made on request
  DevBuf<ChestResDev>    d_res;
  DevBuf<int16_t>        d_e, d_w;
  DevBuf<uint8_t>        d_cb_bytes, d_cb_ok;
  DevBuf<uint32_t>       d_cb_iters;
  DevBuf<uint32_t>       d_tb_rem, d_cb_syn; // TB CRC shares from the windowed decoders ([C][K] table, [B*C] out); null for W = 0
  DevBuf<float>          d_csi;     // [B][max_re], cfg.csi_enable
  DevBuf<uint32_t>       d_csi_max; // [B]
  const cf32*            grid_in = nullptr; // resource grids supplied by the caller (srslte_hip_dl_rx_grid_batch) instead of d_grid
  std::unique_ptr<GrantsState> gs; // srslte_hip_dl_rx_batch_grants: created on first use
  struct srslte_hip_dl_rx* cw1 = nullptr; // two-layer modes: the second codeword's back end (rate de-matching, decoder, TB assembly and their buffers)
  srslte_hip_csi_t*      csi = nullptr; // srslte_hip_dl_rx_csi_batch: made on first use
  uint32_t               est_nof_sf = 0; // subframes the last estimator run (stage 1) left in d_ce / d_res; 0: none yet
  float                  csi_offset = 0.f; // snr_to_cqi_offset of srslte_hip_dl_rx_csi_batch
  ~srslte_hip_dl_rx()
  {
    srslte_hip_dl_rx_destroy(cw1);
    srslte_hip_ofdm_destroy(ofdm);
    srslte_hip_chest_dl_destroy(chest);
    srslte_hip_tdec_destroy(tdec);
    srslte_hip_csi_destroy(csi);
  }
};

extern "C" void srslte_hip_dl_rx_destroy(srslte_hip_dl_rx_t* q) { delete q; }

// cw: 0 = a whole pipeline; 1 = the back end of the second codeword of a two-layer mode (cfg->mod / tbs already those of that codeword):
// no OFDM / estimator objects, no grids, scrambling sequence q = 1 (36.211 6.3.1)
static srslte_hip_dl_rx_t* dl_rx_create_impl(const srslte_hip_dl_rx_cfg_t* cfg, int cw)
{
  if (!cfg || cfg->max_batch == 0 || cfg->mod < 1 || cfg->mod > 4 || cfg->max_iterations == 0 || cfg->nof_rx_antennas > 4 || cfg->nof_ports > 4 ||
      cfg->nof_ports == 3) {
    hip_log("[srslte_hip] dl_rx: invalid configuration\n");
    return nullptr;
  }
  const bool mimo = cfg->tx_scheme != 0;
  if (mimo && cw == 0) { // what ra_dl.c:556-600 and precoding.c:1710-1759,:1087-1114 let through
    const bool two = cfg->tbs2 != 0;
    const bool ok  = (cfg->tx_scheme == 2 || cfg->tx_scheme == 3) && cfg->nof_ports == 2 && cfg->nof_rx_antennas == 2 &&
                    (cfg->tx_scheme == 2 || two) && (two ? cfg->pmi < 2 : cfg->pmi < 4) && (!two || (cfg->mod2 >= 1 && cfg->mod2 <= 4));
    if (!ok) {
      hip_log("[srslte_hip] dl_rx: two-layer modes need a 2-port cell and 2 receive antennas; CDD with two transport blocks, "
              "multiplexing with two (pmi 0-1) or one (pmi 0-3)\n");
      return nullptr;
    }
  }
  std::unique_ptr<srslte_hip_dl_rx> q(new srslte_hip_dl_rx());
  q->cfg = *cfg;
  if (srslte_hip_cbsegm(&q->seg, cfg->tbs) || q->seg.F || q->seg.C2 || (cfg->tbs % 8)) {
    hip_log("[srslte_hip] dl_rx: TBS %u needs filler bits or two code-block sizes; not supported on device yet\n", cfg->tbs);
    return nullptr;
  }
  const uint32_t P = cfg->nof_prb, nre = 12 * P, B = cfg->max_batch, C = q->seg.C, K = q->seg.K1, Qm = 2 * (uint32_t)cfg->mod;
  const uint32_t lstart = cfg->cfi + (P < 10 ? 1 : 0); // SRSLTE_NOF_CTRL_SYMBOLS, phy_common.h:143
  const uint32_t nrx    = cfg->nof_rx_antennas ? cfg->nof_rx_antennas : 1;
  const uint32_t npt    = cfg->nof_ports ? cfg->nof_ports : 1;
  const uint32_t nsl    = (cfg->cp_ext || cfg->mbsfn) ? 6 : 7; // symbols per slot (an MBSFN subframe has the extended CP's 12 on any cell)
  if (cfg->mbsfn && (npt != 1 || mimo || cfg->tdd || cfg->llr_8bit || cfg->csi_enable || cfg->power_scale || cfg->mbsfn_area_id > 255 ||
                     cfg->non_mbsfn_region < 1 || cfg->non_mbsfn_region > 2 || cw)) {
    // srslte_pmch_decode: one port (pmch.c:159), int16 LLRs (:377), no CSI weighting, no power allocation
    hip_log("[srslte_hip] dl_rx: an MBSFN pipeline is single-port FDD with 16-bit LLRs, area id 0-255, a non-MBSFN region of 1 or 2 symbols\n");
    return nullptr;
  }
  if (cfg->mbsfn) q->cfg.chest_cfg.interpolate_subframe = 1;
  if (cfg->tdd && (cfg->tdd_sf_config > 6 || cfg->tdd_ss_config > 9)) {
    hip_log("[srslte_hip] dl_rx: TDD uplink-downlink configuration %u / special-subframe configuration %u\n", cfg->tdd_sf_config, cfg->tdd_ss_config);
    return nullptr;
  }
  if (cw == 0) {
    q->ofdm  = srslte_hip_ofdm_create((int)P, nsl == 6 ? 0 : 1, 1);
    q->chest = srslte_hip_chest_dl_create(cfg->cell_id, P, npt, cfg->cp_ext ? 0 : 1);
    if (q->chest && cfg->tdd) srslte_hip_chest_dl_set_tdd(q->chest, (int)cfg->tdd_sf_config, (int)cfg->tdd_ss_config);
    if (cfg->mbsfn && q->ofdm && q->chest &&
        (srslte_hip_ofdm_set_mbsfn(q->ofdm, 1, (int)cfg->non_mbsfn_region) || srslte_hip_chest_dl_set_mbsfn_area_id(q->chest, (uint16_t)cfg->mbsfn_area_id))) {
      srslte_hip_chest_dl_destroy(q->chest);
      q->chest = nullptr;
    }
  }
  q->tdec  = srslte_hip_tdec_create(K, B * C);
  bool ok  = (cw || (q->ofdm && q->chest)) && q->tdec;
  // RE lists
  uint32_t max_re = 0;
  const uint32_t rep_sf[3] = {0, 5, 1};
  for (int c = 0; c < 3 && ok; c++) {
    std::vector<uint32_t> idx;
    if (cfg->mbsfn) pmch_re_indices(P, lstart, idx); // the same list for every subframe index: no PSS / SSS / PBCH in an MBSFN subframe
    else pdsch_re_indices(cfg->cell_id, P, npt, rep_sf[c], lstart, idx, nsl);
    q->pg.cls[c].nof_re = (int)idx.size();
    q->rg.nof_re[c]     = (int)idx.size();
    max_re              = idx.size() > max_re ? (uint32_t)idx.size() : max_re;
    if (cw) continue; // the lists are the first codeword's object's
    ok                  = upload(q->d_idx[c], idx) == SRSLTE_SUCCESS;
    q->pg.cls[c].idx    = q->d_idx[c];
  }
  const uint32_t max_bits = (max_re * Qm + 15) & ~15u, scr_words = (max_re * Qm + 31) / 32 + 1; // spare word: the demapper reads two per RE
  // scrambling sequences, one per subframe index (sequences.c:58-60, pdsch.c:469)
  if (ok) {
    std::vector<uint32_t> scr((size_t)10 * scr_words, 0);
    std::vector<uint8_t>  c;
    for (uint32_t sf = 0; sf < 10; sf++) {
      // srslte_sequence_pmch (sequences.c:76-80) with nslot = 2 sf (pmch.c:263-275) for an MBSFN pipeline
      const uint32_t c_init = cfg->mbsfn ? (sf << 9) + cfg->mbsfn_area_id : ((uint32_t)cfg->rnti << 14) + ((uint32_t)cw << 13) + (sf << 9) + cfg->cell_id;
      lte_gold_sequence(c_init, max_re * Qm, c);
      for (uint32_t i = 0; i < max_re * Qm; i++) scr[(size_t)sf * scr_words + (i >> 5)] |= (uint32_t)c[i] << (i & 31);
    }
    ok = upload(q->d_scr, scr) == SRSLTE_SUCCESS;
  }
  // rate-dematching table in the decoder's input layout (rm_turbo.c:160-260)
  q->W         = cfg->llr_8bit ? srslte_hip_tdec_autoimp_get_subblocks_8bit(K) : srslte_hip_tdec_autoimp_get_subblocks(K);
  q->in_stride = (srslte_hip_tdec_input_len(K, q->W != 0) + 31) & ~31u;
  ok = ok && rm_rx_table_upload(K, 0, q->W, q->in_stride, q->d_rm_tbl_rv[0]) == SRSLTE_SUCCESS;
  // TB CRC24A remainders x^(tbs+24-1-j) mod g
  if (ok) {
    std::vector<uint32_t> rem(cfg->tbs + 24);
    uint32_t              v = 1;
    for (int j = (int)cfg->tbs + 23; j >= 0; j--) {
      rem[j] = v;
      v <<= 1;
      if (v & 0x1000000) v ^= 0x1864CFB;
    }
    ok = upload(q->d_tbcrc, rem) == SRSLTE_SUCCESS;
    if (ok && q->W) { // per code block, in the decoder's array order (window-interleaved); 0 on the CB CRC bits
      const uint32_t        rlen = C == 1 ? K : K - 24, Lw = K / q->W;
      std::vector<uint32_t> t((size_t)C * K, 0);
      for (uint32_t c = 0; c < C; c++) {
        for (uint32_t n = 0; n < rlen; n++) {
          const uint32_t pos = c * rlen + n;
          if (pos < cfg->tbs + 24) t[(size_t)c * K + (n % Lw) * q->W + n / Lw] = rem[pos];
        }
      }
      ok = upload(q->d_tb_rem, t) == SRSLTE_SUCCESS && q->d_cb_syn.alloc((size_t)B * C) == SRSLTE_SUCCESS;
    }
  }
  const size_t glen = (size_t)2 * nsl * nre;
  if (cw == 0) {
    ok = ok && !q->d_grid.alloc(glen * B * nrx) && !q->d_ce.alloc(glen * B * nrx * npt) &&
         hipMemset(q->d_ce, 0, sizeof(cf32) * glen * B * nrx * npt) == hipSuccess && /* 4 ports + interpolate_subframe: ports 2/3 keep what is there */
         !q->d_res.alloc(B);
  }
  ok = ok && !q->d_e.alloc((size_t)max_bits * B + 16) /* +16: rm_rx_lds_kernel reads whole 16-byte words */ &&
       !q->d_w.alloc((size_t)q->in_stride * B * C) && !q->d_cb_bytes.alloc((size_t)(K / 8) * B * C) && !q->d_cb_ok.alloc((size_t)B * C) &&
       !q->d_cb_iters.alloc((size_t)B * C);
  if (ok && cfg->csi_enable) ok = !q->d_csi.alloc((size_t)max_re * B) && !q->d_csi_max.alloc(B);
  // HARQ state of slots that have not seen new data yet (a retransmission into such a slot combines with an empty soft buffer and
  // decodes every block); the memsets run on the null stream, which the callers' non-blocking streams do not order against: wait here
  ok = ok && hipMemset(q->d_cb_ok, 0, (size_t)B * C) == hipSuccess && hipMemset(q->d_w, 0, sizeof(int16_t) * (size_t)q->in_stride * B * C) == hipSuccess &&
       hipMemset(q->d_cb_bytes, 0, (size_t)(K / 8) * B * C) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
  // The compact parity layout serves the 16-window 16-bit decoder on a buffer it reads in place, when no block of any subframe class gets
  // more LLRs than the layout holds (the code-block split of sch.c:331-334). Environment SRSLTE_HIP_PARITY_COMPACT=0, read here: never (A/B, tests)
  if (ok && !cw && !cfg->llr_8bit && q->W == 16 && K % 64 == 0 && ((reinterpret_cast<uintptr_t>(q->d_w.get()) | (q->in_stride * sizeof(int16_t))) & 15) == 0) {
    const char*     e = getenv("SRSLTE_HIP_PARITY_COMPACT");
    RmParityCompact c;
    if (!(e && atoi(e) == 0) && rm_parity_compact(K, c)) {
      const uint32_t Nl = (npt > 1 && !mimo) ? 2 : 1;
      uint32_t       mx = 0;
      for (int i = 0; i < 3; i++) {
        const uint32_t Gp = (uint32_t)q->rg.nof_re[i] / Nl, n_e = Qm * Nl * (Gp / C) + (Gp % C > 1 ? Qm * Nl : 0); // some cb > C - gamma
        mx = n_e > mx ? n_e : mx;
      }
      if (mx <= c.e_lim) {
        ok        = rm_rx_table_upload_compact(K, q->pc, q->d_rm_tbl_pc) == SRSLTE_SUCCESS;
        q->pc_ok = ok;
      }
    }
  }
  if (!ok) {
    hip_log("[srslte_hip] dl_rx: initialisation failed\n");
    return nullptr;
  }
  q->pg.grid_len = (int)glen; q->pg.max_re = (int)max_re; q->pg.max_bits = (int)max_bits; q->pg.mod = cfg->mod; q->pg.Qm = (int)Qm;
  q->pg.mmse = cfg->mmse; q->pg.scr_words = (int)scr_words; q->pg.nof_rx = (int)nrx; q->pg.nof_ports = (int)npt;
  q->pg.csi = q->d_csi; q->pg.csi_max = q->d_csi_max;
  // Without interpolate_subframe the estimator gives every symbol of a subframe the same row of estimates (chest_dl.c:467-471): a single-port
  // pipeline keeps that row only - the estimator writes 12 nof_prb values per subframe and antenna instead of 14 times as many, the demapper
  // reads the row for every symbol
  const bool compact = npt == 1 && !q->cfg.chest_cfg.interpolate_subframe && !cw;
  q->pg.ce_len = compact ? (int)(12 * P) : (int)glen; q->pg.ce_nre = compact ? (int)(12 * P) : 0;
  q->pg.ce_magic = compact ? (uint32_t)((0x100000000ull + 12 * P - 1) / (12 * P)) : 0;
  // apply_power_allocation (pdsch.c:518-554) with rho_b = 1: pdsch_scaling = rho_a = 10^(p_a/20), times sqrt(2) for a 2-port cell
  q->pg.inv_scaling = cfg->power_scale ? 1.0f / (powf(10.0f, cfg->p_a / 20.0f) * (npt == 1 ? 1.0f : sqrtf(2.0f))) : 1.0f;
  // code-block split in units of Qm N_L bits: N_L = 2 for transmit diversity, 1 where nof_layers == nof_tb (srslte_dlsch_decode2, sch.c:507-531)
  q->rg.csi = q->d_csi; q->rg.csi_max = q->d_csi_max; q->rg.max_re = (int)max_re; q->rg.mod = cfg->mod; q->rg.Nl = (npt > 1 && !mimo) ? 2 : 1;
  q->rg.C = (int)C; q->rg.K = (int)K; q->rg.Qm = (int)Qm; q->rg.max_bits = (int)max_bits; q->rg.w_stride = (int)q->in_stride;
  q->rg.out_len = (int)(3 * K + 12);
  q->tg.C = (int)C; q->tg.K = (int)K; q->tg.tbs = (int)cfg->tbs; q->tg.rlen = (int)(C == 1 ? K : K - 24); q->tg.cb_stride = (int)(K / 8);
  if (mimo && cw == 0) {
    q->pg.tx_scheme = cfg->tx_scheme; q->pg.nof_tb = cfg->tbs2 ? 2 : 1;
    q->pg.codebook_idx = (int)(cfg->tbs2 ? cfg->pmi + 1 : cfg->pmi); // pdsch.c:914
    if (cfg->tbs2) {
      srslte_hip_dl_rx_cfg_t c1 = *cfg;
      c1.mod = cfg->mod2; c1.tbs = cfg->tbs2; c1.mod2 = 0; c1.tbs2 = 0;
      q->cw1 = dl_rx_create_impl(&c1, 1);
      if (!q->cw1) return nullptr;
      q->pg.mod1 = c1.mod; q->pg.Qm1 = q->cw1->pg.Qm; q->pg.max_bits1 = q->cw1->pg.max_bits; q->pg.scr_words1 = q->cw1->pg.scr_words;
      q->pg.scr1 = q->cw1->d_scr; q->pg.csi1 = q->cw1->d_csi; q->pg.csi_max1 = q->cw1->d_csi_max;
    }
  }
  return q.release();
}

extern "C" srslte_hip_dl_rx_t* srslte_hip_dl_rx_create(const srslte_hip_dl_rx_cfg_t* cfg) { return dl_rx_create_impl(cfg, 0); }

extern "C" int srslte_hip_dl_rx_keep_symbols(srslte_hip_dl_rx_t* q, int enable)
{
  if (!q) return SRSLTE_ERROR_INVALID_INPUTS;
  if (q->cw1) {
    if (int r = srslte_hip_dl_rx_keep_symbols(q->cw1, enable)) return r;
  }
  if (enable && !q->d_d && q->d_d.alloc((size_t)q->pg.max_re * q->cfg.max_batch)) {
    hip_log("[srslte_hip] dl_rx: no device memory for the equalised symbols\n");
    return SRSLTE_ERROR;
  }
  if (!enable) q->d_d = DevBuf<cf32>();
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

// d_w's slots in the compact parity layout back to the whole one (HARQ combining, a call the compact layout does not serve, the debug view)
static int dl_rx_w_whole(srslte_hip_dl_rx_t* q, hipStream_t st)
{
  if (!q->w_compact_n) return SRSLTE_SUCCESS;
  hipLaunchKernelGGL(rm_parity_expand_kernel, dim3(q->w_compact_n * q->seg.C), dim3(256), 0, st, q->d_w.get(), (int)q->in_stride, (int)q->seg.K1,
                     (int)q->pc.phase[0], (int)q->pc.phase[1]);
  LAUNCH_CHECK();
  q->w_compact_n = 0;
  return SRSLTE_SUCCESS;
}

extern "C" int srslte_hip_dl_rx_parity_compact(const srslte_hip_dl_rx_t* q) { return q ? q->last_compact : 0; }

extern "C" uint32_t srslte_hip_rm_parity_compact_limit(uint32_t K)
{
  RmParityCompact c;
  return lte_cb_index(K) >= 0 && lte_qpp_table[lte_cb_index(K)].K == K && rm_parity_compact(K, c) ? c.e_lim : 0;
}

extern "C" const void* srslte_hip_dl_rx_debug_buffer(const srslte_hip_dl_rx_t* q, int which)
{
  if (!q) return nullptr;
  if (which >= 100) return srslte_hip_dl_rx_debug_buffer(q->cw1, which - 100); // the second codeword's buffers
  switch (which) {
    case 0: return q->d_grid;
    case 1: return q->pg.ce_nre ? dl_rx_ce_full(const_cast<srslte_hip_dl_rx_t*>(q)) : q->d_ce;
    case 2: return q->d_res;
    case 3: return q->d_d;
    case 4: return q->d_e;
    case 5: { // the whole layout, whatever the last call left
      srslte_hip_dl_rx_t* m = const_cast<srslte_hip_dl_rx_t*>(q);
      if (hipDeviceSynchronize() != hipSuccess || dl_rx_w_whole(m, 0) || hipDeviceSynchronize() != hipSuccess) return nullptr;
      return q->d_w;
    }
    case 6: return q->d_cb_iters;
    case 7: return q->d_cb_ok;
    case 8: return q->d_cb_bytes;
    case 9: return q->d_csi;
    case 10: return q->d_csi_max;
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

// The 16-window 16-bit decoder (K > 800) and the two 8-bit back-ends (avx8, sse8) assemble the transport blocks themselves when nothing of an earlier
// transmission has to be merged in: stage 5 is then empty. (HARQ combining keeps blocks of earlier calls, the short-block decoders have no such mode:
// tb_asm / tb_crc.)
static bool dl_rx_tb_direct(const srslte_hip_dl_rx_t* q, const uint8_t* d_tb, uint32_t tb_stride, const uint8_t* d_tb_ok)
{
  return q->d_tb_rem && (q->cfg.llr_8bit ? q->W >= 16 : q->W == 16) && !q->harq_combine && !q->cw1 && !q->pg.tx_scheme && d_tb && d_tb_ok &&
         tb_stride >= q->cfg.tbs / 8 + 6;
}

// Stage launchers, also used one by one by bench.py to time each kernel in isolation.
extern "C" int srslte_hip_dl_rx_stage(srslte_hip_dl_rx_t* q, int stage, const void* d_iq, uint32_t tti0, uint32_t nof_sf, uint8_t* d_tb,
                                      uint32_t tb_stride, uint8_t* d_tb_ok, void* stream)
{
  if (!q || nof_sf > q->cfg.max_batch) return SRSLTE_ERROR_INVALID_INPUTS;
  if (nof_sf == 0) return SRSLTE_SUCCESS;
  hipStream_t    st = (hipStream_t)stream;
  const uint32_t C = q->seg.C, K = q->seg.K1;
  const cf32*    grid = q->grid_in ? q->grid_in : q->d_grid;
  if (q->cfg.tdd && stage >= 2) { // OFDM and estimator serve the grants mode; the fixed grant's RE lists, sequences and tables are per FDD subframe class
    hip_log("[srslte_hip] dl_rx: a TDD cell is received through the per-subframe-grant entry points (srslte_hip_dl_rx_batch_grants*)\n");
    return SRSLTE_ERROR;
  }
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
      if (g.tx_scheme) {
        if (g.csi_max1) HIP_TRY(hipMemsetAsync(g.csi_max1, 0, sizeof(uint32_t) * nof_sf, st));
        if (q->cfg.llr_8bit) { // pdsch.c:760-779: q->llr_is_8bit with any transmission scheme
          hipLaunchKernelGGL(pdsch_demod_mimo_kernel<int8_t>, dim3(ceil_div(g.max_re, 256), nof_sf), dim3(256), 0, st, grid, (const cf32*)q->d_ce,
                             (const ChestResDev*)q->d_res, (const uint32_t*)q->d_scr, q->d_d, q->cw1 ? q->cw1->d_d : (cf32*)nullptr, (int8_t*)q->d_e.get(),
                             q->cw1 ? (int8_t*)q->cw1->d_e.get() : (int8_t*)nullptr, g);
        } else {
          hipLaunchKernelGGL(pdsch_demod_mimo_kernel<int16_t>, dim3(ceil_div(g.max_re, 256), nof_sf), dim3(256), 0, st, grid, (const cf32*)q->d_ce,
                             (const ChestResDev*)q->d_res, (const uint32_t*)q->d_scr, q->d_d, q->cw1 ? q->cw1->d_d : (cf32*)nullptr, q->d_e,
                             q->cw1 ? q->cw1->d_e : (int16_t*)nullptr, g);
        }
      } else if (g.nof_ports == 4) {
        if (q->cfg.llr_8bit) {
          hipLaunchKernelGGL(pdsch_demod_div4_kernel<int8_t>, dim3(ceil_div(g.max_re, 1024), nof_sf), dim3(256), 0, st, grid, (const cf32*)q->d_ce,
                             (const uint32_t*)q->d_scr, q->d_d, (int8_t*)q->d_e.get(), g);
        } else {
          hipLaunchKernelGGL(pdsch_demod_div4_kernel<int16_t>, dim3(ceil_div(g.max_re, 1024), nof_sf), dim3(256), 0, st, grid, (const cf32*)q->d_ce,
                             (const uint32_t*)q->d_scr, q->d_d, q->d_e, g);
        }
      } else if (g.nof_ports == 2) {
        if (q->cfg.llr_8bit) {
          hipLaunchKernelGGL(pdsch_demod_div_kernel<int8_t>, dim3(ceil_div(g.max_re, 512), nof_sf), dim3(256), 0, st, grid, (const cf32*)q->d_ce,
                             (const uint32_t*)q->d_scr, q->d_d, (int8_t*)q->d_e.get(), g);
        } else {
          hipLaunchKernelGGL(pdsch_demod_div_kernel<int16_t>, dim3(ceil_div(g.max_re, 512), nof_sf), dim3(256), 0, st, grid, (const cf32*)q->d_ce,
                             (const uint32_t*)q->d_scr, q->d_d, q->d_e, g);
        }
      } else if (q->cfg.llr_8bit) {
        hipLaunchKernelGGL(pdsch_demod_kernel<int8_t>, dim3(ceil_div(g.max_re, 256), nof_sf), dim3(256), 0, st, grid,
                           (const cf32*)q->d_ce, (const ChestResDev*)q->d_res, (const uint32_t*)q->d_scr, q->d_d, (int8_t*)q->d_e.get(), g);
      } else {
        hipLaunchKernelGGL(pdsch_demod_kernel<int16_t>, dim3(ceil_div(g.max_re, 256), nof_sf), dim3(256), 0, st, grid,
                           (const cf32*)q->d_ce, (const ChestResDev*)q->d_res, (const uint32_t*)q->d_scr, q->d_d, q->d_e, g);
      }
      LAUNCH_CHECK();
      return SRSLTE_SUCCESS;
    }
    case 3: {
      if (q->cw1) {
        if (int r = srslte_hip_dl_rx_stage(q->cw1, 3, nullptr, tti0, nof_sf, nullptr, 0, nullptr, stream)) return r;
      }
      RmGeom g = q->rg;
      g.tti0   = (int)tti0;
      g.combine = q->harq_combine;
      g.skip    = q->harq_combine ? q->d_cb_ok : nullptr;
      const uint32_t* tbl = q->d_rm_tbl_rv[q->harq_rv];
      // New data at rv 0 goes to the compact parity layout where the object has it. Anything else works on the whole layout: slots a compact
      // call left are expanded first if this call combines with them or does not overwrite all of them
      q->last_compact = q->pc_ok && q->harq_rv == 0 && !q->harq_combine;
      if (q->last_compact) {
        tbl     = q->d_rm_tbl_pc;
        g.w_len = (int)q->pc.len;
        q->w_compact_n = nof_sf > q->w_compact_n ? nof_sf : q->w_compact_n;
      } else if (q->harq_combine || nof_sf < q->w_compact_n) {
        if (int r = dl_rx_w_whole(q, st)) return r;
      } else {
        q->w_compact_n = 0;
      }
      if (q->cfg.llr_8bit) return rm_rx_launch<int8_t>(rm_lds_bytes(g, 1), nof_sf * C, q->d_e, q->d_w, tbl, g, st);
      return rm_rx_launch<int16_t>(rm_lds_bytes(g, 2), nof_sf * C, q->d_e, q->d_w, tbl, g, st);
    }
    case 4: {
      if (q->cw1) {
        if (int r = srslte_hip_dl_rx_stage(q->cw1, 4, nullptr, tti0, nof_sf, nullptr, 0, nullptr, stream)) return r;
      }
      TdecOpts o;
      o.tb_rem = q->d_tb_rem; o.tb_C = C; o.tb_syn = q->d_cb_syn;
      o.skip   = q->harq_combine ? q->d_cb_ok.get() : nullptr;
      if (q->w_compact_n && q->w_compact_n < nof_sf) { // a decoder run over more slots than the last compact call filled
        if (int r = dl_rx_w_whole(q, st)) return r;
      }
      if (q->w_compact_n) {
        o.pc = 1; o.pc_phase[0] = q->pc.phase[0]; o.pc_phase[1] = q->pc.phase[1];
      }
      q->direct_tb = nullptr;
      if (dl_rx_tb_direct(q, d_tb, tb_stride, d_tb_ok)) {
        o.tb_out = d_tb; o.tb_out_stride = tb_stride; o.tb_rb = q->tg.rlen / 8; o.tb_ok_out = d_tb_ok;
        q->direct_tb = d_tb; q->direct_ok = d_tb_ok; q->direct_stride = tb_stride; q->direct_nof_sf = nof_sf;
      }
      return tdec_run_batch_w(q->tdec, q->d_w, q->cfg.llr_8bit ? 1 : 0, q->in_stride, q->W != 0, K, -1, nof_sf * C, q->cfg.max_iterations,
                              C > 1 ? 0x1800063u : 0x1864CFBu, C > 1 ? K : q->cfg.tbs + 24, q->d_cb_bytes, K / 8, q->d_cb_iters, q->d_cb_ok, st, o);
    }
    case 5: {
      if (!d_tb || !d_tb_ok || tb_stride < q->cfg.tbs / 8 + 6) return SRSLTE_ERROR_INVALID_INPUTS;
      if (q->cw1) { // rows nof_sf .. 2 nof_sf - 1 of d_tb / d_tb_ok: the second transport block of every subframe
        if (int r = srslte_hip_dl_rx_stage(q->cw1, 5, nullptr, tti0, nof_sf, d_tb + (size_t)nof_sf * tb_stride, tb_stride, d_tb_ok + nof_sf, stream)) return r;
      }
      // stage 4 assembled these transport blocks and gave these verdicts; other outputs: the assembly kernel, from the blocks' bytes and CRC
      // syndromes, which the decoders store in that mode as well
      if (q->direct_tb && q->direct_tb == d_tb && q->direct_ok == d_tb_ok && q->direct_stride == tb_stride && q->direct_nof_sf == nof_sf) return SRSLTE_SUCCESS;
      TbGeom g    = q->tg;
      g.tb_stride = (int)tb_stride;
      g.iters     = q->d_cb_iters;
      if (q->d_tb_rem) {
        hipLaunchKernelGGL(tb_asm_kernel, dim3(nof_sf), dim3(256), 0, st, (const uint8_t*)q->d_cb_bytes, (const uint8_t*)q->d_cb_ok,
                           (const uint32_t*)q->d_cb_syn, d_tb, d_tb_ok, g);
      } else {
        hipLaunchKernelGGL(tb_crc_kernel, dim3(nof_sf), dim3(512), 0, st, (const uint8_t*)q->d_cb_bytes, (const uint8_t*)q->d_cb_ok,
                           (const uint32_t*)q->d_tbcrc, d_tb, d_tb_ok, g);
      }
      LAUNCH_CHECK();
      return SRSLTE_SUCCESS;
    }
  }
  return SRSLTE_ERROR_INVALID_INPUTS;
}

extern "C" int srslte_hip_dl_rx_batch(srslte_hip_dl_rx_t* q, const void* d_iq, uint32_t tti0, uint32_t nof_sf, uint8_t* d_tb,
                                      uint32_t tb_stride, uint8_t* d_tb_ok, void* stream)
{
  if (!q || !d_iq || !d_tb || !d_tb_ok) return SRSLTE_ERROR_INVALID_INPUTS;
  for (int s = 0; s < 6; s++) {
    int r = srslte_hip_dl_rx_stage(q, s, d_iq, tti0, nof_sf, d_tb, tb_stride, d_tb_ok, stream);
    if (r) return r;
  }
  return SRSLTE_SUCCESS;
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
  srslte_hip_dl_rx_t* objs[2] = {q, q->cw1};
  for (int c = 0; c < 2; c++) {
    srslte_hip_dl_rx_t* o = objs[c];
    if (!o) continue;
    if (!o->d_rm_tbl_rv[rv[c]]) {
      if (int r = rm_rx_table_upload(o->seg.K1, rv[c], o->W, o->in_stride, o->d_rm_tbl_rv[rv[c]])) return r;
    }
    o->harq_rv      = rv[c];
    o->harq_combine = new_data[c] ? 0 : 1;
  }
  int r = SRSLTE_SUCCESS;
  for (int s = 0; s < 6 && !r; s++) r = srslte_hip_dl_rx_stage(q, s, d_iq, tti0, nof_sf, d_tb, tb_stride, d_tb_ok, stream);
  for (srslte_hip_dl_rx_t* o : objs) {
    if (o) {
      o->harq_rv      = 0;
      o->harq_combine = 0;
    }
  }
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
  q->grid_in = (const cf32*)d_grid;
  int r      = SRSLTE_SUCCESS;
  for (int s = 1; s < 6 && r == SRSLTE_SUCCESS; s++) r = srslte_hip_dl_rx_stage(q, s, nullptr, tti0, nof_sf, d_tb, tb_stride, d_tb_ok, stream);
  q->grid_in = nullptr;
  return r;
}
