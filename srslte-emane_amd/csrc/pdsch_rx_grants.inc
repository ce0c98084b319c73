// Fragment of pdsch.hip (same translation unit): per-subframe grants on the PDSCH receive side and the grants machinery the other pipelines share
// (allocation, transport-block builder, back end).
// --------------------------------------------------------------------------------------------------------------------
// Per-subframe grants (what a TTI stream looks like: srslte_pdsch_decode takes a new srslte_pdsch_grant_t every subframe, pdsch.c:833-997):
// subframe b of the batch is received with grants[b] - PRB masks of both slots (srslte_pdsch_grant_t.prb_idx, walked by srslte_pdsch_cp
// pdsch.c:81-206), modulation, transport block size, redundancy version, RNTI, CFI, new-data flag. RE lists and scrambling sequences are made
// on the device from the grants, rate de-matching runs over the ragged set of code blocks of the batch, the turbo decoder once per block
// length present in it. cfg.tbs bounds the transport block size (buffer sizes), cfg.mod / cfg.rnti / cfg.cfi are not used here.
// Single-port cells (TM1) and 2- / 4-port cells with transmit diversity (TM2), 1..4 receive antennas, 16- or 8-bit LLRs (cfg.llr_8bit), with or
// without the CSI weighting of cfg.csi_enable.
// --------------------------------------------------------------------------------------------------------------------
// Gold-sequence basis (sequence.c:48-79) for scr_gen_kernel: row 0 = the x1 sequence, row 1 + j = the x2 sequence of c_init = 1 << j, `words`
// packed words each; all 31 x2 basis sequences advance together, bit j of the state word = basis j
static int gold_basis_upload(uint32_t words, DevBuf<uint32_t>& d_basis)
{
  const uint32_t         nbits = words * 32, Nc = 1600, tot = nbits + Nc + 31;
  std::vector<uint8_t>   x1(tot);
  std::vector<uint32_t>  x2(tot);
  for (uint32_t n = 0; n < 31; n++) {
    x1[n] = n == 0;
    x2[n] = 1u << n;
  }
  for (uint32_t n = 0; n + 31 < tot; n++) {
    x1[n + 31] = x1[n + 3] ^ x1[n];
    x2[n + 31] = x2[n + 3] ^ x2[n + 2] ^ x2[n + 1] ^ x2[n];
  }
  std::vector<uint32_t> basis((size_t)32 * words, 0);
  for (uint32_t n = 0; n < nbits; n++) {
    const uint32_t w = n >> 5, b = n & 31, v2 = x2[n + Nc];
    basis[w] |= (uint32_t)x1[n + Nc] << b;
    for (uint32_t j = 0; j < 31; j++) basis[(size_t)(1 + j) * words + w] |= ((v2 >> j) & 1u) << b;
  }
  return upload(d_basis, basis);
}

// Buffers of a grants mode: V per-transport-block slots of up to Cmax code blocks and max_re resource elements each; relist_rows > 0 adds the
// PDSCH RE lists, csi the CSI rows. Shared by the downlink (slot = subframe, or max_batch + subframe for codeword 1) and the uplink (slot = PUSCH).
static int grants_alloc(GrantsState* g, uint32_t max_re, uint32_t V, uint32_t Cmax, uint32_t relist_rows, bool csi, size_t extra_desc_bytes)
{
  g->Cmax     = Cmax;
  g->stride   = (srslte_hip_tdec_input_len(6144, 1) + 31) & ~31u;
  g->max_re   = max_re;                            // upper bound of any allocation
  g->max_bits = (g->max_re * 8 + 15) & ~15u;       // 256QAM
  g->words    = (g->max_re * 8 + 31) / 32 + 2;     // + the spare word the demapper reads
  g->V        = V;
  {
    const char* e = getenv("SRSLTE_HIP_GRANTS_TB_DIRECT");
    g->tb_direct  = !(e && e[0] == '0');
  }
  g->tdec     = srslte_hip_tdec_create(6144, g->V * g->Cmax);
  if (!g->tdec) return SRSLTE_ERROR;
  if (gold_basis_upload(g->words, g->d_basis)) return SRSLTE_ERROR;
  const size_t nblk = (size_t)g->V * g->Cmax;
  g->desc_bytes     = sizeof(GrantDev) * g->V + sizeof(SfDesc) * g->V + sizeof(CbDesc) * nblk + sizeof(uint32_t) * nblk + extra_desc_bytes + ((g->V + 15) & ~15u);
  if (g->desc.init(g->desc_bytes + 16)) return SRSLTE_ERROR; // + 16: copied in 16-byte words (grants_prep_kernel, desc_copy_kernel)
  if (relist_rows && g->d_relist.alloc((size_t)g->max_re * relist_rows)) return SRSLTE_ERROR;
  if (g->d_scr.alloc((size_t)g->words * g->V) || g->d_e.alloc((size_t)g->max_bits * g->V + 16) || g->d_w.alloc((size_t)g->stride * nblk) ||
      g->d_cb_bytes.alloc((size_t)768 * nblk) || g->d_cb_ok.alloc(nblk) || g->d_cb_iters.alloc(nblk))
    return SRSLTE_ERROR;
  if (csi && (g->d_csi.alloc((size_t)g->max_re * g->V) || g->d_csi_max.alloc(g->V))) return SRSLTE_ERROR;
  // HARQ state of slots that have not seen new data yet: nothing decoded, empty soft buffers
  HIP_TRY(hipMemset(g->d_cb_ok, 0, nblk));
  HIP_TRY(hipMemset(g->d_w, 0, sizeof(int16_t) * (size_t)g->stride * nblk));
  HIP_TRY(hipMemset(g->d_cb_bytes, 0, (size_t)768 * nblk));
  HIP_TRY(hipDeviceSynchronize());
  return SRSLTE_SUCCESS;
}

// The sections of a descriptor block of a grants mode, host or device copy: GrantDev[V] | SfDesc[V] | CbDesc[V Cmax] | block map[V Cmax] |
// the caller's extra_desc_bytes | cof[(V + 15) & ~15], one byte per slot: its transport block's code-block count (the decoders' own
// transport-block assembly, TdecOpts::tb_Cof)
struct GrantsDesc {
  GrantDev* gr;
  SfDesc*   sf;
  CbDesc*   cb;
  uint32_t* map;
  uint8_t * extra, *cof;
  GrantsDesc(const GrantsState* g, uint8_t* base)
  {
    const size_t nblk = (size_t)g->V * g->Cmax;
    gr    = reinterpret_cast<GrantDev*>(base);
    sf    = reinterpret_cast<SfDesc*>(gr + g->V);
    cb    = reinterpret_cast<CbDesc*>(sf + g->V);
    map   = reinterpret_cast<uint32_t*>(cb + nblk);
    extra = reinterpret_cast<uint8_t*>(map + nblk);
    cof   = base + g->desc_bytes - ((g->V + 15) & ~15u);
  }
};

// Direct assembly: the decoders assemble the transport blocks themselves (16-bit LLRs, unless SRSLTE_HIP_GRANTS_TB_DIRECT=0), when none of the
// call's has more blocks than their CRC factor table covers (TDEC_TB_MAX_C_DIRECT). Writes the block counts of slots 0 .. n-1 to h.cof;
// counts(v): slot v holds a transport block of this call. Returns d.cof, or null: tb_crc_bytes_kernel assembles
template <typename Counts>
static const uint8_t* grants_direct_cof(const GrantsState* g, const GrantsDesc& h, const GrantsDesc& d, uint32_t n, bool l8, Counts counts)
{
  uint32_t max_C = 0;
  for (uint32_t v = 0; v < n; v++) {
    h.cof[v] = (uint8_t)h.sf[v].C;
    if (counts(v)) max_C = std::max(max_C, (uint32_t)h.sf[v].C);
  }
  return !l8 && g->tb_direct && max_C <= TDEC_TB_MAX_C_DIRECT ? d.cof : nullptr;
}

static int grants_init(srslte_hip_dl_rx_t* q)
{
  const uint32_t P = q->cfg.nof_prb, B = q->cfg.max_batch;
  q->gs.reset(new GrantsState());
  return grants_alloc(q->gs.get(), 14 * 12 * P, (q->pg.nof_ports == 2 && q->pg.nof_rx == 2) ? 2 * B : B, q->cw[0].sch.seg.C, B, q->cfg.csi_enable != 0, 0);
}

// slot table of (K, rv) in the input layout of the decoder AUTO selects for K, stride = that layout's length rounded up to 32
static int grants_rm_table(GrantsState* g, uint32_t K, uint32_t rv, uint32_t W, uint32_t w_len, const uint32_t** d_tbl)
{
  auto it = g->rm_tbl.find({K, rv});
  if (it == g->rm_tbl.end()) {
    DevBuf<uint32_t> d;
    if (rm_rx_table_upload(K, rv, W, w_len, d)) return SRSLTE_ERROR;
    it = g->rm_tbl.emplace(std::make_pair(K, rv), std::move(d)).first;
  }
  *d_tbl = it->second;
  return SRSLTE_SUCCESS;
}

// weights of tb_crc_bytes_kernel for a transport block of tbs bits: w[t] = x^(8 cB (255 - t)) mod g_CRC24A
static int grants_crc_factors(GrantsState* g, uint32_t tbs, const uint32_t** d_fac)
{
  auto it = g->crc_fac.find(tbs);
  if (it == g->crc_fac.end()) {
    const uint32_t poly = 0x1864CFBu, nbytes = tbs / 8 + 3, cB = (nbytes + 255) / 256;
    auto           mul  = [&](uint32_t a, uint32_t b) {
      uint32_t r = 0;
      for (int i = 23; i >= 0; i--) {
        r <<= 1;
        if (r & 0x1000000u) r ^= poly;
        if ((b >> i) & 1) r ^= a;
      }
      return r;
    };
    uint32_t m = 1; // x^(8 cB) mod g
    for (uint32_t i = 0; i < 8 * cB; i++) {
      m <<= 1;
      if (m & 0x1000000u) m ^= poly;
    }
    std::vector<uint32_t> w(256);
    w[255] = 1;
    for (int t = 254; t >= 0; t--) w[t] = mul(w[t + 1], m);
    DevBuf<uint32_t> d;
    if (upload(d, w)) return SRSLTE_ERROR;
    it = g->crc_fac.emplace(tbs, std::move(d)).first;
  }
  *d_fac = it->second;
  return SRSLTE_SUCCESS;
}

// The PRB masks of a grant as the RE-list kernel wants them, upstream's stale `offset` values, and the number of PDSCH REs of the allocation
// (what pdsch_relist_kernel will list). gd.sf_idx / gd.lstart must be set; shared by the receive and the transmit grants modes.
// srslte_ra_dl_compute_nof_re's nof_symb_slot (ra_dl.c:446-460) for subframe sf_idx of a TDD cell: the DwPTS symbols of a special subframe
// (phy_common.c:101-135), the cyclic prefix's count elsewhere. FDD: gd.tdd = 0, gd.nss = {0, 0}
static void tdd_grant_symbols(int tdd, uint32_t sf_config, uint32_t ss_config, int nsl, uint32_t sf_idx, GrantDev& gd)
{
  static const int dw[10] = {3, 9, 10, 11, 12, 3, 9, 10, 11, 6};
  gd.tdd = tdd ? 1 : 0;
  gd.nss[0] = gd.nss[1] = 0;
  if (!tdd) return;
  const bool special = sf_idx == 1 || (sf_idx == 6 && (sf_config <= 2 || sf_config == 6));
  const int  n = special ? dw[ss_config % 10] : 2 * nsl;
  gd.nss[0] = n < nsl ? n : nsl;
  gd.nss[1] = n < nsl ? 0 : n - nsl;
}

static uint32_t pdsch_grant_dev(const srslte_hip_dl_grant_t& gr, uint32_t P, uint32_t cell_id, int npt, GrantDev& gd, int nsl = 7)
{
  const uint32_t sf_idx = (uint32_t)gd.sf_idx, lstart = (uint32_t)gd.lstart;
  bool any0 = false, below1 = false;
  for (uint32_t n = 0; n < P; n++) {
    for (int s_ = 0; s_ < 2; s_++) {
      if ((gr.prb_mask[s_][n >> 5] >> (n & 31)) & 1u) {
        gd.mask[s_][n >> 5] |= 1u << (n & 31);
        if (s_ == 0 && nsl - 3 >= (int)lstart) any0 = true; // slot 0's CRS symbol nsl - 3 lies behind the control region (always, bar 4 control symbols on an extended-CP cell)
        if (s_ == 1 && n + 3 < P / 2) below1 = true;
      }
    }
  }
  // upstream's `offset` when it reaches the half PRBs of slot 1, symbol 0 (pdsch.c:147-157,:172-190): set by the whole PRBs before them;
  // with 2 / 4 ports every CRS symbol sets the same value
  bool any1_whole = false; // any whole (non-centre) PRB of slot 1: by symbol 1 its symbol-0 row has set `offset` too
  for (uint32_t n = 0; n < P; n++) {
    if (((gr.prb_mask[1][n >> 5] >> (n & 31)) & 1u) && !(n >= P / 2 - 3 && n < P / 2 + 3 + (P % 2))) any1_whole = true;
  }
  // bits 0-7: at symbol 0 of slot 1; bits 8-15: at symbol 1 (4 ports); bits 16-23: at symbol 3 of slot 1 on an extended-CP cell, whose PBCH
  // symbols 0-3 hold a second CRS symbol - by then the whole PRBs of symbol 0 of the slot have set `offset` too
  const int q0 = npt == 1 ? (below1 ? (int)(cell_id % 6) : (any0 ? (int)((cell_id + 3) % 6) : 0)) : ((below1 || any0) ? (int)(cell_id % 3) : 0);
  const int q1 = npt == 1 ? 0 : ((below1 || any0 || any1_whole) ? (int)(cell_id % 3) : 0);
  const int q3 = npt == 1 ? (below1 ? (int)((cell_id + 3) % 6) : (any1_whole ? (int)(cell_id % 6) : (any0 ? (int)((cell_id + 3) % 6) : 0)))
                          : ((below1 || any0 || any1_whole) ? (int)(cell_id % 3) : 0);
  gd.q_off = q0 | (q1 << 8) | (q3 << 16);
  // number of PDSCH REs (what pdsch_relist_kernel will list; srslte_ra_dl_grant_nof_re): per symbol, whole PRBs carry 12 REs (10 with
  // CRS, 8 on a multi-port cell), PRBs inside the PSS / SSS / PBCH region of a sync symbol none, the two PRBs an odd bandwidth cuts in half
  // there half of that
  auto pop = [](const uint32_t* m, const uint32_t* f) {
    return __builtin_popcount(m[0] & f[0]) + __builtin_popcount(m[1] & f[1]) + __builtin_popcount(m[2] & f[2]) + __builtin_popcount(m[3] & f[3]);
  };
  uint32_t centre[4] = {0, 0, 0, 0}, half[4] = {0, 0, 0, 0}, all[4] = {~0u, ~0u, ~0u, ~0u};
  for (uint32_t n = P / 2 - 3; n < P / 2 + 3 + (P % 2); n++) centre[n >> 5] |= 1u << (n & 31);
  if (P % 2) {
    half[(P / 2 - 3) >> 5] |= 1u << ((P / 2 - 3) & 31);
    half[(P / 2 + 3) >> 5] |= 1u << ((P / 2 + 3) & 31);
  }
  uint32_t nre = 0;
  const int nss[2] = {gd.nss[0] ? gd.nss[0] : nsl, gd.nss[0] ? gd.nss[1] : nsl};
  for (int sym = 0; sym < 2 * nsl; sym++) {
    const int s_ = sym / nsl, l = sym % nsl;
    if ((s_ == 0 && l < (int)lstart) || l >= nss[s_]) continue;
    const bool ref = l == 0 || l == nsl - 3 || (l == 1 && npt == 4);
    const bool ss  = gd.tdd ? ((s_ == 1 && (sf_idx == 0 || sf_idx == 5) && l >= nss[1] - 1) || (s_ == 0 && (sf_idx == 1 || sf_idx == 6) && l == 2))
                            : (s_ == 0 && (sf_idx == 0 || sf_idx == 5) && l >= nsl - 2);
    const bool sync = ss || (s_ == 1 && sf_idx == 0 && l < 4);
    const int  per = ref ? (npt == 1 ? 10 : 8) : 12;
    nre += per * pop(gd.mask[s_], all);
    if (sync) nre += (per / 2) * pop(gd.mask[s_], half) - per * pop(gd.mask[s_], centre);
  }
  return nre;
}

// Host side of one grants-mode call: transport blocks are added one by one (descriptor of their slot, one descriptor per code block, decoder
// group by block length), then grants_back_end runs rate de-matching, the decoders and the transport-block check over what was added.
struct GrantsBuild {
  struct Group { uint32_t K, single; std::vector<uint32_t> slots; };
  GrantsState*       g;
  SfDesc*            h_sf;
  CbDesc*            h_cb;
  bool               l8;      // 8-bit LLRs (pdsch.c:760-779, sch.c:336-356): same buffers, as bytes
  uint32_t           max_tbs; // the object's largest transport block (its buffers are sized for it)
  int                npt, max_mod;
  const char*        who;
  std::vector<Group> groups;
  uint32_t           ncb = 0, max_seg = 0;
  // one transport block into slot v: descriptor, code-block descriptors, decoder group. b: the caller's index, for the message
  int add_tb(uint32_t b, uint32_t v, int mod, uint32_t tbs, uint32_t rv, int new_data, uint32_t nre, uint32_t Nl, uint32_t e_off = 0)
  {
    SfDesc& sd = h_sf[v];
    srslte_hip_cbsegm_t seg;
    if (mod < 1 || mod > max_mod || rv > 3 || tbs > max_tbs || tbs > (uint32_t)TB_MAX_BITS || (tbs % 8) || srslte_hip_cbsegm(&seg, tbs) || seg.F || seg.C2 ||
        seg.C == 0 /* tbs = 0 segments into no block at all: nothing to decode, and nre / C below must not see it */ || seg.C > g->Cmax) {
      hip_log("[srslte_hip] %s grants: entry %u: unsupported transport block (mod %d, tbs %u, rv %u)\n", who, b, mod, tbs, rv);
      return SRSLTE_ERROR_INVALID_INPUTS;
    }
    const uint32_t Qm = 2 * (uint32_t)mod, K = seg.K1, C = seg.C;
    if (nre == 0 || nre < C * Nl) {
      hip_log("[srslte_hip] %s grants: entry %u: empty allocation\n", who, b);
      return SRSLTE_ERROR_INVALID_INPUTS;
    }
    sd.nof_re = (int)nre; sd.mod = mod; sd.Qm = (int)Qm; sd.C = (int)C; sd.K = (int)K; sd.tbs = (int)tbs; sd.rlen = (int)(C == 1 ? K : K - 24);
    if (grants_crc_factors(g, tbs, &sd.crc_fac)) return SRSLTE_ERROR;
    const uint32_t W = l8 ? srslte_hip_tdec_autoimp_get_subblocks_8bit(K) : srslte_hip_tdec_autoimp_get_subblocks(K);
    const uint32_t w_len = (srslte_hip_tdec_input_len(K, W != 0) + 31) & ~31u;
    const uint32_t* tbl = nullptr;
    if (grants_rm_table(g, K, rv, W, w_len, &tbl)) return SRSLTE_ERROR;
    Group* grp = nullptr;
    for (auto& x : groups) {
      if (x.K == K && x.single == (C == 1 ? tbs : 0)) grp = &x;
    }
    if (!grp) {
      groups.push_back(Group{K, C == 1 ? tbs : 0, {}});
      grp = &groups.back();
    }
    for (uint32_t c = 0; c < C; c++) {
      CbDesc& cd = h_cb[ncb++];
      cd.sf = (int)v; cd.cb = (int)c; cd.C = (int)C; cd.K = (int)K; cd.Qm = (int)Qm; cd.nof_re = (int)nre; cd.combine = new_data ? 0 : 1;
      cd.w_len = (int)w_len; cd.tbl = tbl; cd.Nl = (int)Nl; cd.e_off = (int)e_off;
      grp->slots.push_back(v * g->Cmax + c);
    }
    const uint32_t seg_bytes = (Qm * (nre / C) + 2 * Qm * (uint32_t)npt) * (l8 ? 1 : 2) + 32;
    max_seg = seg_bytes > max_seg ? seg_bytes : max_seg;
    return SRSLTE_SUCCESS;
  }
  uint32_t fill_map(uint32_t* h_map) const
  {
    uint32_t n = 0;
    for (auto& x : groups) {
      for (uint32_t v : x.slots) h_map[n++] = v;
    }
    return n;
  }
};

// rate de-matching of every added block, the decoders group by group, and the transport-block check of rows 0 .. nrows-1 (row -> slot: the row
// itself, or cw1_off + row - nof_rows0 for rows behind the first nof_rows0: the second codewords)
// d_cof != null (16-bit LLRs): the decoders assemble the transport blocks and give the verdicts themselves - a block kept from an earlier
// transmission contributes its stored bytes (tdec_tb_stored_block), rows without a transport block were zeroed by the caller -, no
// tb_crc_bytes_kernel behind them
static int grants_back_end(GrantsState* g, const GrantsBuild& bd, const SfDesc* d_sf, const CbDesc* d_cb, const uint32_t* d_map, uint32_t tti0,
                           uint32_t max_iterations, uint32_t nrows, uint32_t nof_rows0, uint32_t cw1_off, uint8_t* d_tb, uint32_t tb_stride,
                           uint8_t* d_tb_ok, hipStream_t st, const uint8_t* d_cof = nullptr)
{
  const bool l8 = bd.l8;
  const bool direct = d_cof != nullptr && !l8;
  if (bd.ncb) {
    RmGeom rg;
    memset(&rg, 0, sizeof(rg));
    rg.cbd = d_cb; rg.cb_ok_rst = g->d_cb_ok; rg.C = (int)g->Cmax; rg.tti0 = (int)tti0; rg.max_bits = (int)g->max_bits; rg.w_stride = (int)g->stride;
    rg.Nl = 1; rg.skip = g->d_cb_ok; rg.max_re = (int)g->max_re; rg.csi = g->d_csi; rg.csi_max = g->d_csi_max;
    const int lds = (int)((bd.max_seg + 15) & ~15u);
    if (int r = l8 ? rm_rx_launch<int8_t>(lds, bd.ncb, g->d_e, g->d_w, nullptr, rg, st) : rm_rx_launch<int16_t>(lds, bd.ncb, g->d_e, g->d_w, nullptr, rg, st))
      return r;
    TdecOpts o;
    o.skip = g->d_cb_ok;
    if (direct) {
      o.tb_out = d_tb; o.tb_out_stride = tb_stride; o.tb_ok_out = d_tb_ok;
      o.tb_Cof = d_cof; o.tb_width = g->Cmax; o.tb_B = cw1_off; o.tb_rows0 = nof_rows0;
    }
    // every block length of the batch in one call: one launch per decoder kernel, not one per length (tdec_run_groups)
    std::vector<srslte_hip_tdec_group_t> gv;
    gv.reserve(bd.groups.size());
    for (auto& x : bd.groups) gv.push_back({x.K, (uint32_t)x.slots.size(), x.single ? 0x1864CFBu : 0x1800063u, x.single ? x.single + 24 : x.K});
    int rc = SRSLTE_SUCCESS;
    for (size_t first = 0, off = 0; first < gv.size() && rc == SRSLTE_SUCCESS;) { // more lengths than a launch's table holds: several calls
      const size_t cnt = gv.size() - first < 24 ? gv.size() - first : 24;
      o.cb_map = d_map + off;
      rc = tdec_run_groups(g->tdec, g->d_w, l8 ? 1 : 0, g->stride, gv.data() + first, (uint32_t)cnt, max_iterations, g->d_cb_bytes, 768, g->d_cb_iters, g->d_cb_ok, st, o);
      for (size_t i = first; i < first + cnt; i++) off += gv[i].nof_cb;
      first += cnt;
    }
    if (rc) return rc;
  }
  if (direct || !d_tb) return SRSLTE_SUCCESS; // d_tb = null: the caller takes the blocks' bytes and flags and assembles on the host (sch_host.inc)
  TbGeom tg;
  memset(&tg, 0, sizeof(tg));
  tg.desc = d_sf; tg.C = (int)g->Cmax; tg.cb_stride = 768; tg.tb_stride = (int)tb_stride; tg.nof_sf = (int)nof_rows0; tg.cw1_off = (int)cw1_off;
  tg.iters = g->d_cb_iters;
  hipLaunchKernelGGL(tb_crc_bytes_kernel, dim3(nrows), dim3(256), 0, st, (const uint8_t*)g->d_cb_bytes, (const uint8_t*)g->d_cb_ok, d_tb, d_tb_ok, tg);
  LAUNCH_CHECK();
  return SRSLTE_SUCCESS;
}

static int grants_run(srslte_hip_dl_rx_t* q, const void* d_iq, uint32_t tti0, uint32_t nof_sf, const srslte_hip_dl_grant2_t* grants, uint8_t* d_tb,
                      uint32_t tb_stride, uint8_t* d_tb_ok, void* stream, bool second_rows, const cf32* grid_in = nullptr);

extern "C" int srslte_hip_dl_rx_batch_grants(srslte_hip_dl_rx_t* q, const void* d_iq, uint32_t tti0, uint32_t nof_sf, const srslte_hip_dl_grant_t* grants,
                                             uint8_t* d_tb, uint32_t tb_stride, uint8_t* d_tb_ok, void* stream)
{
  if (!q || !grants || nof_sf > q->cfg.max_batch) return SRSLTE_ERROR_INVALID_INPUTS;
  std::vector<srslte_hip_dl_grant2_t> g2(nof_sf);
  for (uint32_t b = 0; b < nof_sf; b++) {
    memset(&g2[b], 0, sizeof(g2[b]));
    g2[b].tb0 = grants[b];
  }
  return grants_run(q, d_iq, tti0, nof_sf, g2.data(), d_tb, tb_stride, d_tb_ok, stream, false);
}

// The same with the transmission scheme per subframe and a second transport block: on a 2-port cell received with 2 antennas a grant can be
// transmit diversity (tx_scheme 0 / 1: DCI 1 / 1A), large-delay CDD (3, two transport blocks) or closed-loop multiplexing (2, two blocks
// with pmi 0-1 or one with pmi 0-3), as srslte_ra_dl_dci_to_grant makes them (ra_dl.c:530-600). Codeword 1 of subframe b is a second
// per-subframe slot (descriptor, LLR row, CSI row, HARQ soft buffers) max_batch further on; its transport block is row nof_sf + b of d_tb.
extern "C" int srslte_hip_dl_rx_batch_grants2(srslte_hip_dl_rx_t* q, const void* d_iq, uint32_t tti0, uint32_t nof_sf, const srslte_hip_dl_grant2_t* grants,
                                              uint8_t* d_tb, uint32_t tb_stride, uint8_t* d_tb_ok, void* stream)
{
  return grants_run(q, d_iq, tti0, nof_sf, grants, d_tb, tb_stride, d_tb_ok, stream, true);
}

// The same from frequency-domain grids (what follows srslte_ofdm_rx_sf in ue_dl.c:375-397; d_grid as srslte_hip_dl_rx_grid_batch takes it)
extern "C" int srslte_hip_dl_rx_grid_batch_grants2(srslte_hip_dl_rx_t* q, const void* d_grid, uint32_t tti0, uint32_t nof_sf, const srslte_hip_dl_grant2_t* grants,
                                                   uint8_t* d_tb, uint32_t tb_stride, uint8_t* d_tb_ok, void* stream)
{
  if (!q || !d_grid) return SRSLTE_ERROR_INVALID_INPUTS;
  return grants_run(q, d_grid, tti0, nof_sf, grants, d_tb, tb_stride, d_tb_ok, stream, true, (const cf32*)d_grid);
}

// second_rows: rows nof_sf .. 2 nof_sf - 1 of d_tb / d_tb_ok exist (srslte_hip_dl_rx_batch_grants2 on a cell where two-layer grants can occur);
// grid_in: resource grids supplied by the caller instead of d_iq's
static int grants_run(srslte_hip_dl_rx_t* q, const void* d_iq, uint32_t tti0, uint32_t nof_sf, const srslte_hip_dl_grant2_t* grants, uint8_t* d_tb,
                      uint32_t tb_stride, uint8_t* d_tb_ok, void* stream, bool second_rows, const cf32* grid_in)
{
  if (!q || !d_iq || !grants || !d_tb || !d_tb_ok || nof_sf > q->cfg.max_batch || tb_stride < q->cfg.tbs / 8 + 6) return SRSLTE_ERROR_INVALID_INPUTS;
  if (q->cfg.tx_scheme) {
    hip_log("[srslte_hip] dl_rx grants mode: create the object without a fixed two-layer scheme; the grants carry it\n");
    return SRSLTE_ERROR;
  }
  if (q->cfg.mbsfn) {
    hip_log("[srslte_hip] dl_rx grants mode: an MBSFN pipeline has one PMCH configuration, no per-subframe grants\n");
    return SRSLTE_ERROR;
  }
  if (nof_sf == 0) return SRSLTE_SUCCESS;
  if (!q->gs && grants_init(q)) { // a failed start leaves no half-made state behind
    hip_log("[srslte_hip] dl_rx grants: initialisation failed\n");
    q->gs.reset();
    return SRSLTE_ERROR;
  }
  GrantsState*   g  = q->gs.get();
  hipStream_t    st = (hipStream_t)stream;
  const uint32_t P = q->cfg.nof_prb, cell_id = q->cfg.cell_id, B = q->cfg.max_batch, V = g->V;
  const int      npt = q->pg.nof_ports;
  uint8_t*       h_pin = nullptr;
  if (int r = g->desc.begin(&h_pin)) return r;
  const GrantsDesc h(g, h_pin), d(g, g->desc.dev_bytes());
  GrantDev*        h_gr = h.gr;
  SfDesc*          h_sf = h.sf;
  const bool         l8 = q->cfg.llr_8bit != 0; // the 8-bit LLR path the applications select (pdsch.c:760-779, sch.c:336-356): same buffers, as bytes
  bool               any_mimo = false;
  GrantsBuild        bd;
  bd.g = g; bd.h_sf = h_sf; bd.h_cb = h.cb; bd.l8 = l8; bd.max_tbs = q->cfg.tbs; bd.npt = npt; bd.max_mod = 4; bd.who = "dl_rx";
  auto add_tb = [&](uint32_t b, uint32_t v, int mod, uint32_t tbs, uint32_t rv, int new_data, uint32_t nre, uint32_t Nl) -> int {
    return bd.add_tb(b, v, mod, tbs, rv, new_data, nre, Nl);
  };
  for (uint32_t b = 0; b < nof_sf; b++) {
    const srslte_hip_dl_grant2_t& g2 = grants[b];
    const srslte_hip_dl_grant_t&  gr = g2.tb0;
    GrantDev&                     gd = h_gr[b];
    SfDesc&                       sd = h_sf[b];
    memset(&gd, 0, sizeof(gd));
    memset(&sd, 0, sizeof(sd));
    if (V > B) {
      memset(&h_gr[B + b], 0, sizeof(gd));
      memset(&h_sf[B + b], 0, sizeof(sd));
    }
    const uint32_t sf_idx = (tti0 + b) % 10, lstart = gr.cfi + (P < 10 ? 1 : 0);
    gd.sf_idx = (int)sf_idx; gd.lstart = (int)lstart; gd.rnti = gr.rnti;
    tdd_grant_symbols(q->cfg.tdd, q->cfg.tdd_sf_config, q->cfg.tdd_ss_config, q->cfg.cp_ext ? 6 : 7, sf_idx, gd);
    sd.idx = g->d_relist + (size_t)b * g->max_re;
    sd.scr = g->d_scr + (size_t)b * g->words;
    if (gr.tbs == 0) continue; // no transport block in this subframe: C = 0, tb_ok = 0
    const bool two_layer = g2.tx_scheme >= 2;
    if (gr.cfi < 1 || gr.cfi > 3 || g2.tx_scheme < 0 || g2.tx_scheme > 3 ||
        (two_layer && (V == B || (g2.tx_scheme == 3 && g2.tbs2 == 0) || (g2.tbs2 ? g2.pmi > 1 : g2.pmi > 3))) || (!two_layer && g2.tbs2)) {
      hip_log("[srslte_hip] dl_rx grants: subframe %u: unsupported grant (cfi %u, tx_scheme %d, pmi %u, second transport block %u bits)\n", b, gr.cfi, g2.tx_scheme,
              g2.pmi, g2.tbs2);
      return SRSLTE_ERROR_INVALID_INPUTS;
    }
    const uint32_t nre = pdsch_grant_dev(gr, P, cell_id, npt, gd, q->cfg.cp_ext ? 6 : 7);
    if (!two_layer && (nre % (uint32_t)npt)) { // the transmit-diversity pre-decoders take the REs in groups of nof_ports (precoding.c:564-650)
      hip_log("[srslte_hip] dl_rx grants: subframe %u: %u REs are not a multiple of the %d ports\n", b, nre, npt);
      return SRSLTE_ERROR_INVALID_INPUTS;
    }
    // nof_layers == nof_tb for the two-layer modes: N_L = 1; transmit diversity: 2 (srslte_dlsch_decode2, sch.c:507-531)
    if (int r = add_tb(b, b, gr.mod, gr.tbs, gr.rv, gr.new_data, nre, (!two_layer && npt > 1) ? 2 : 1)) return r;
    sd.scheme = g2.tx_scheme; sd.nof_tb = g2.tbs2 ? 2 : 1; sd.codebook = (int)(g2.tbs2 ? g2.pmi + 1 : g2.pmi); // pdsch.c:914
    if (two_layer) any_mimo = true;
    if (g2.tbs2) { // codeword 1: slot max_batch + b, the same REs, its own sequence (q = 1), modulation, transport block
      GrantDev& gd1 = h_gr[B + b];
      SfDesc&   sd1 = h_sf[B + b];
      gd1 = gd; gd1.cw = 1;
      sd1.idx = sd.idx;
      sd1.scr = g->d_scr + (size_t)(B + b) * g->words;
      if (int r = add_tb(b, B + b, g2.mod2, g2.tbs2, g2.rv2, g2.new_data2, nre, 1)) return r;
      sd1.scheme = g2.tx_scheme; sd1.nof_tb = 2; sd1.codebook = sd.codebook;
    }
  }
  bd.fill_map(h.map);
  // slots of subframes nof_sf .. B - 1 keep an earlier call's descriptors
  const uint8_t* d_cof = grants_direct_cof(g, h, d, V, l8, [&](uint32_t v) { return v % B < nof_sf; });
  // stages 0, 1: OFDM demodulation and channel estimation do not depend on the grants
  const DlRxCall call = {grid_in, {}};
  int r = grid_in ? SRSLTE_SUCCESS : dl_rx_stage(q, 0, d_iq, tti0, nof_sf, d_tb, tb_stride, d_tb_ok, stream, call); // grids from the caller: no OFDM stage
  if (!r) r = dl_rx_stage(q, 1, d_iq, tti0, nof_sf, d_tb, tb_stride, d_tb_ok, stream, call);
  if (r) return r;
  const uint32_t nrows = (second_rows && V > B) ? 2 * nof_sf : nof_sf; // transport-block rows of the call
  { // RE lists and scrambling sequences (with the second codewords' when a two-layer grant is among them) and the descriptors: one launch,
    // whose last workgroups copy the descriptors (the grants the first ones need are read from the pinned buffer)
    const int       per = ceil_div((int)g->words, RELIST_THREADS), work = (int)(nof_sf + (any_mimo ? 2 : 1) * nof_sf * per);
    const int       n16 = (int)((g->desc_bytes + 15) / 16);
    const GrantDev* src = h_gr;
    hipLaunchKernelGGL(grants_prep_kernel, dim3(work + ceil_div(n16, RELIST_THREADS)), dim3(RELIST_THREADS), 0, st, src, g->d_relist, (int)P,
                       (int)cell_id, (int)g->max_re, q->pg.nof_ports, q->cfg.cp_ext ? 6 : 7, (int)nof_sf, (const uint32_t*)g->d_basis, g->d_scr,
                       any_mimo ? src + B : nullptr, g->d_scr + (size_t)B * g->words, (int)g->words, d_tb_ok,
                       (int)nrows, (const uint4*)h_pin, (uint4*)g->desc.dev_bytes(), n16, work);
  }
  LAUNCH_CHECK();
  if (int r = g->desc.committed(st)) return r; // the pinned buffer is free again when this launch has run
  {
    PdschGeom pg = q->pg;
    pg.desc = d.sf; pg.tti0 = (int)tti0; pg.max_re = (int)g->max_re; pg.max_bits = (int)g->max_bits; pg.csi = g->d_csi; pg.csi_max = g->d_csi_max;
    if (g->d_csi_max) HIP_TRY(hipMemsetAsync(g->d_csi_max, 0, sizeof(uint32_t) * V, st));
    const cf32* grid = grid_in ? grid_in : q->d_grid;
    if (pg.nof_ports == 4) {
      if (l8) {
        hipLaunchKernelGGL(pdsch_demod_div4_kernel<int8_t>, dim3(ceil_div((int)g->max_re, 1024), nof_sf), dim3(256), 0, st, grid, (const cf32*)q->d_ce,
                           (const uint32_t*)g->d_scr, (cf32*)nullptr, (int8_t*)g->d_e.get(), pg);
      } else {
        hipLaunchKernelGGL(pdsch_demod_div4_kernel<int16_t>, dim3(ceil_div((int)g->max_re, 1024), nof_sf), dim3(256), 0, st, grid, (const cf32*)q->d_ce,
                           (const uint32_t*)g->d_scr, (cf32*)nullptr, g->d_e, pg);
      }
    } else if (pg.nof_ports == 2) {
      if (l8) {
        hipLaunchKernelGGL(pdsch_demod_div_kernel<int8_t>, dim3(ceil_div((int)g->max_re, 512), nof_sf), dim3(256), 0, st, grid, (const cf32*)q->d_ce,
                           (const uint32_t*)g->d_scr, (cf32*)nullptr, (int8_t*)g->d_e.get(), pg);
      } else {
        hipLaunchKernelGGL(pdsch_demod_div_kernel<int16_t>, dim3(ceil_div((int)g->max_re, 512), nof_sf), dim3(256), 0, st, grid, (const cf32*)q->d_ce,
                           (const uint32_t*)g->d_scr, (cf32*)nullptr, g->d_e, pg);
      }
      if (any_mimo) { // the two-layer subframes (the kernels above skipped them); codeword 1's rows sit max_batch further on in every buffer
        pg.cw1_off  = (int)B;
        pg.max_bits1 = pg.max_bits;
        pg.csi1     = g->d_csi ? g->d_csi + (size_t)B * g->max_re : nullptr;
        pg.csi_max1 = g->d_csi_max ? g->d_csi_max + B : nullptr;
        if (l8) {
          hipLaunchKernelGGL(pdsch_demod_mimo_kernel<int8_t>, dim3(ceil_div((int)g->max_re, 256), nof_sf), dim3(256), 0, st, grid, (const cf32*)q->d_ce,
                             (const ChestResDev*)q->d_res, (const uint32_t*)g->d_scr, (cf32*)nullptr, (cf32*)nullptr, (int8_t*)g->d_e.get(),
                             (int8_t*)g->d_e.get() + (size_t)B * g->max_bits, pg);
        } else {
          hipLaunchKernelGGL(pdsch_demod_mimo_kernel<int16_t>, dim3(ceil_div((int)g->max_re, 256), nof_sf), dim3(256), 0, st, grid, (const cf32*)q->d_ce,
                             (const ChestResDev*)q->d_res, (const uint32_t*)g->d_scr, (cf32*)nullptr, (cf32*)nullptr, g->d_e, g->d_e + (size_t)B * g->max_bits, pg);
        }
      }
    } else if (l8) {
      hipLaunchKernelGGL(pdsch_demod_kernel<int8_t>, dim3(ceil_div((int)g->max_re, 256), nof_sf), dim3(256), 0, st, grid, (const cf32*)q->d_ce,
                         (const ChestResDev*)q->d_res, (const uint32_t*)g->d_scr, (cf32*)nullptr, (int8_t*)g->d_e.get(), pg);
    } else {
      hipLaunchKernelGGL(pdsch_demod_kernel<int16_t>, dim3(ceil_div((int)g->max_re, 256), nof_sf), dim3(256), 0, st, grid, (const cf32*)q->d_ce,
                         (const ChestResDev*)q->d_res, (const uint32_t*)g->d_scr, (cf32*)nullptr, g->d_e, pg);
    }
    LAUNCH_CHECK();
  }
  return grants_back_end(g, bd, d.sf, d.cb, d.map, tti0, q->cfg.max_iterations, nrows, nof_sf, B, d_tb, tb_stride, d_tb_ok, st, d_cof);
}

// ---- srslte_hip_dl_rx_pool_*: `depth` pipelines behind one submission call (phy_hip.h)
struct srslte_hip_dl_rx_pool {
  std::vector<srslte_hip_dl_rx_t*> rx;
  std::vector<hipStream_t>         st;
  std::vector<hipEvent_t>          ev;
  std::vector<int64_t>             last; // ticket of the batch each object works on, -1: none
  std::vector<DevBuf<uint8_t>>     iq;   // submit_host: one batch of time samples per object, allocated by the first such call
  int64_t                          next = 0;
  ~srslte_hip_dl_rx_pool()
  {
    for (size_t i = 0; i < rx.size(); i++) {
      if (st[i]) (void)hipStreamSynchronize(st[i]); // before the object's buffers go
      srslte_hip_dl_rx_destroy(rx[i]);
      if (ev[i]) (void)hipEventDestroy(ev[i]);
      if (st[i]) (void)hipStreamDestroy(st[i]);
    }
  }
};

extern "C" void srslte_hip_dl_rx_pool_destroy(srslte_hip_dl_rx_pool_t* p) { delete p; }

extern "C" srslte_hip_dl_rx_pool_t* srslte_hip_dl_rx_pool_create(const srslte_hip_dl_rx_cfg_t* cfg, uint32_t depth)
{
  if (!cfg || depth == 0 || depth > 16) return nullptr;
  std::unique_ptr<srslte_hip_dl_rx_pool> p(new srslte_hip_dl_rx_pool());
  p->rx.assign(depth, nullptr);
  p->st.assign(depth, nullptr);
  p->ev.assign(depth, nullptr);
  p->last.assign(depth, -1);
  p->iq.resize(depth);
  for (uint32_t i = 0; i < depth; i++) {
    p->rx[i] = srslte_hip_dl_rx_create(cfg);
    if (!p->rx[i] || hipStreamCreateWithFlags(&p->st[i], hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&p->ev[i], hipEventDisableTiming) != hipSuccess)
      return nullptr;
  }
  return p.release();
}

extern "C" int64_t srslte_hip_dl_rx_pool_submit(srslte_hip_dl_rx_pool_t* p, const void* d_iq, uint32_t tti0, uint32_t nof_sf, const srslte_hip_dl_grant_t* grants,
                                                uint8_t* d_tb, uint32_t tb_stride, uint8_t* d_tb_ok, void* h_record)
{
  if (!p || !d_iq || !d_tb || !d_tb_ok) return SRSLTE_ERROR_INVALID_INPUTS;
  const size_t i = (size_t)(p->next % (int64_t)p->rx.size());
  if (p->last[i] >= 0 && hipEventSynchronize(p->ev[i]) != hipSuccess) return SRSLTE_ERROR; // the object's previous batch: its buffers are free again
  const int r = grants ? srslte_hip_dl_rx_batch_grants(p->rx[i], d_iq, tti0, nof_sf, grants, d_tb, tb_stride, d_tb_ok, p->st[i])
                       : srslte_hip_dl_rx_batch(p->rx[i], d_iq, tti0, nof_sf, d_tb, tb_stride, d_tb_ok, p->st[i]);
  if (r) return r < 0 ? r : SRSLTE_ERROR;
  if (h_record) { // [nof_sf][tb_stride] transport-block bytes, then [nof_sf] flags, on the batch's stream
    if (hipMemcpyAsync(h_record, d_tb, (size_t)nof_sf * tb_stride, hipMemcpyDeviceToHost, p->st[i]) != hipSuccess ||
        hipMemcpyAsync((uint8_t*)h_record + (size_t)nof_sf * tb_stride, d_tb_ok, nof_sf, hipMemcpyDeviceToHost, p->st[i]) != hipSuccess)
      return SRSLTE_ERROR;
  }
  if (hipEventRecord(p->ev[i], p->st[i]) != hipSuccess) return SRSLTE_ERROR;
  p->last[i] = p->next;
  return p->next++;
}

extern "C" int srslte_hip_dl_rx_pool_set_iq_format(srslte_hip_dl_rx_pool_t* p, int format, float scale)
{
  if (!p || p->next != 0) return SRSLTE_ERROR_INVALID_INPUTS; // before the first submit: no batch is in flight in the other format
  for (auto* rx : p->rx)
    if (int r = srslte_hip_dl_rx_set_iq_format(rx, format, scale)) return r; // the first object refuses what any would: none is changed
  return SRSLTE_SUCCESS;
}

extern "C" int64_t srslte_hip_dl_rx_pool_submit_host(srslte_hip_dl_rx_pool_t* p, const void* h_iq, uint32_t tti0, uint32_t nof_sf, const srslte_hip_dl_grant_t* grants,
                                                     uint8_t* d_tb, uint32_t tb_stride, uint8_t* d_tb_ok, void* h_record)
{
  if (!p || !h_iq || !d_tb || !d_tb_ok || nof_sf > p->rx[0]->cfg.max_batch) return SRSLTE_ERROR_INVALID_INPUTS;
  const size_t          i  = (size_t)(p->next % (int64_t)p->rx.size());
  srslte_hip_dl_rx_t*   rx = p->rx[i];
  const size_t          sf_bytes = ofdm_sample_bytes(rx->ofdm) * (size_t)rx->pg.nof_rx * (size_t)srslte_hip_ofdm_sf_len(rx->ofdm);
  if (!p->iq[0]) { // sized for either format, so that the buffers never move
    for (auto& b : p->iq)
      if (b.alloc(sizeof(cf32) * (size_t)rx->pg.nof_rx * (size_t)srslte_hip_ofdm_sf_len(rx->ofdm) * rx->cfg.max_batch)) {
        for (auto& c : p->iq) c = DevBuf<uint8_t>();
        hip_log("[srslte_hip] dl_rx_pool: device allocation failed\n");
        return SRSLTE_ERROR;
      }
  }
  // the staging buffer is the object's: its previous batch has to be through before the copy overwrites it. submit() waits for the same event.
  if (p->last[i] >= 0 && hipEventSynchronize(p->ev[i]) != hipSuccess) return SRSLTE_ERROR;
  if (nof_sf && hipMemcpyAsync(p->iq[i], h_iq, sf_bytes * nof_sf, hipMemcpyHostToDevice, p->st[i]) != hipSuccess) return SRSLTE_ERROR;
  return srslte_hip_dl_rx_pool_submit(p, p->iq[i], tti0, nof_sf, grants, d_tb, tb_stride, d_tb_ok, h_record);
}

extern "C" int srslte_hip_dl_rx_pool_wait(srslte_hip_dl_rx_pool_t* p, int64_t ticket)
{
  if (!p || ticket < 0 || ticket >= p->next) return SRSLTE_ERROR_INVALID_INPUTS;
  const size_t i = (size_t)(ticket % (int64_t)p->rx.size());
  if (p->last[i] > ticket) return SRSLTE_SUCCESS; // a later batch on the same object was submitted: submit() waited for this one then
  return hipEventSynchronize(p->ev[i]) == hipSuccess ? SRSLTE_SUCCESS : SRSLTE_ERROR;
}
