// Fragment of pdsch.hip (same translation unit): the transport-block back end of the fixed-grant receivers - what the per-subframe-grant modes
// have in GrantsState / grants_back_end. The PDSCH receiver holds one per codeword, the PUSCH receiver one.

// The fixed-grant pipelines take transport blocks without filler bits and with one code-block size. who: the pipeline, for the log line
static int fixed_grant_segmentation(const char* who, uint32_t tbs, srslte_hip_cbsegm_t* seg)
{
  if (srslte_hip_cbsegm(seg, tbs) == 0 && !seg->F && !seg->C2 && (tbs % 8) == 0) return SRSLTE_SUCCESS;
  hip_log("[srslte_hip] %s: TBS %u needs filler bits or two code-block sizes; not supported on device yet\n", who, tbs);
  return SRSLTE_ERROR;
}

// HARQ of one call on one transport block: its rv, and whether it combines with what the slots keep or starts new data. The back end keeps neither
struct SchHarq { uint32_t rv = 0; int combine = 0; };

// From the LLR rows of a batch ([B][max_bits], the subframe's shared-channel LLRs from e_off on) to its transport blocks: rate de-matching,
// turbo decoding, assembly + TB CRC, and the HARQ state of the B slots between calls (soft buffers, CRC flags, decoded bytes)
struct SchRxFixed {
  struct Cfg {
    uint32_t        tbs, max_batch, max_iterations;
    bool            llr_8bit;
    uint32_t        nof_re[3], Qm, Nl, e_off, max_bits, max_re; // nof_re: per subframe class (SfClass)
    int             mod;
    const float*    csi; // CSI weights and maxima of the rows, or null
    const uint32_t* csi_max;
    // permissions, each for where the rest allows it: rv 0 / new data takes the compact parity layout; the decoder assembles the transport blocks
    bool            may_compact, may_direct;
  };
  Cfg                 cfg = {};
  srslte_hip_tdec_t*  tdec = nullptr;
  srslte_hip_cbsegm_t seg  = {};
  RmGeom              rg   = {};
  TbGeom              tg   = {};
  uint32_t            W = 0, in_stride = 0;
  DevBuf<uint32_t>    d_rm_tbl_rv[4]; // [0] made by init; 1..3 built on first use
  // Punctured parity at a quarter of its rows (rm_parity_compact, pdsch_kernels.inc): whether calls with rv 0 and new data take that
  // layout, its table, the subframe slots [0, w_compact_n) of d_w that are in it now (every other slot holds the whole layout) and what
  // the last rate de-matcher run chose
  bool                pc_ok = false;
  RmParityCompact     pc    = {};
  DevBuf<uint32_t>    d_rm_tbl_pc;
  uint32_t            w_compact_n  = 0;
  int                 last_compact = 0;
  const uint8_t*      direct_tb = nullptr; // where the last decoder run assembled the transport blocks itself, or null: assemble() has nothing to do then,
  const uint8_t*      direct_ok = nullptr; // if it is called with the same rows, verdicts, stride and subframe count as that run
  uint32_t            direct_stride = 0, direct_nof_sf = 0;
  DevBuf<int16_t>     d_w;
  DevBuf<uint8_t>     d_cb_bytes, d_cb_ok;
  DevBuf<uint32_t>    d_cb_iters, d_tbcrc;
  DevBuf<uint32_t>    d_tb_rem, d_cb_syn; // TB CRC shares from the windowed decoders ([C][K] table, [B*C] out); null for W = 0
  ~SchRxFixed() { srslte_hip_tdec_destroy(tdec); }

  // c.tbs has passed fixed_grant_segmentation and is not 0. Returns when the device has zeroed the slots' state
  int init(const Cfg& c)
  {
    cfg = c;
    if (srslte_hip_cbsegm(&seg, c.tbs)) return SRSLTE_ERROR;
    const uint32_t B = c.max_batch, C = seg.C, K = seg.K1;
    if (!(tdec = srslte_hip_tdec_create(K, B * C))) return SRSLTE_ERROR;
    // rate-dematching table in the decoder's input layout (rm_turbo.c:160-260)
    W         = c.llr_8bit ? srslte_hip_tdec_autoimp_get_subblocks_8bit(K) : srslte_hip_tdec_autoimp_get_subblocks(K);
    in_stride = (srslte_hip_tdec_input_len(K, W != 0) + 31) & ~31u;
    if (rm_rx_table_upload(K, 0, W, in_stride, d_rm_tbl_rv[0])) return SRSLTE_ERROR;
    std::vector<uint32_t> rem, t;
    lte_tbcrc_rem_table(c.tbs, rem);
    if (upload(d_tbcrc, rem)) return SRSLTE_ERROR;
    if (W) {
      lte_tbcrc_win_table(rem, C, K, W, t);
      if (upload(d_tb_rem, t) || d_cb_syn.alloc((size_t)B * C)) return SRSLTE_ERROR;
    }
    if (d_w.alloc((size_t)in_stride * B * C) || d_cb_bytes.alloc((size_t)(K / 8) * B * C) || d_cb_ok.alloc((size_t)B * C) || d_cb_iters.alloc((size_t)B * C))
      return SRSLTE_ERROR;
    // HARQ state of slots that have not seen new data yet (a retransmission into such a slot combines with an empty soft buffer and
    // decodes every block); the memsets run on the null stream, which the callers' non-blocking streams do not order against: wait here
    HIP_TRY(hipMemset(d_cb_ok, 0, (size_t)B * C));
    HIP_TRY(hipMemset(d_w, 0, sizeof(int16_t) * (size_t)in_stride * B * C));
    HIP_TRY(hipMemset(d_cb_bytes, 0, (size_t)(K / 8) * B * C));
    HIP_TRY(hipDeviceSynchronize());
    rg.csi = c.csi; rg.csi_max = c.csi_max; rg.max_re = (int)c.max_re; rg.mod = c.mod; rg.Nl = (int)c.Nl; rg.e_off = (int)c.e_off;
    rg.C = (int)C; rg.K = (int)K; rg.Qm = (int)c.Qm; rg.max_bits = (int)c.max_bits; rg.w_stride = (int)in_stride; rg.out_len = (int)(3 * K + 12);
    for (int i = 0; i < 3; i++) rg.nof_re[i] = (int)c.nof_re[i];
    tg.C = (int)C; tg.K = (int)K; tg.tbs = (int)c.tbs; tg.rlen = (int)(C == 1 ? K : K - 24); tg.cb_stride = (int)(K / 8);
    // The compact parity layout serves the 16-window 16-bit decoder on a buffer it reads in place, when no block of any subframe class gets
    // more LLRs than the layout holds (the code-block split of sch.c:331-334). Environment SRSLTE_HIP_PARITY_COMPACT=0, read here: never (A/B, tests)
    if (c.may_compact && !c.llr_8bit && W == 16 && K % 64 == 0 && ((reinterpret_cast<uintptr_t>(d_w.get()) | (in_stride * sizeof(int16_t))) & 15) == 0) {
      const char*     e = getenv("SRSLTE_HIP_PARITY_COMPACT");
      RmParityCompact lim;
      if (!(e && atoi(e) == 0) && rm_parity_compact(K, lim)) {
        uint32_t mx = 0;
        for (int i = 0; i < 3; i++) {
          const uint32_t Gp = c.nof_re[i] / c.Nl, n_e = c.Qm * c.Nl * (Gp / C) + (Gp % C > 1 ? c.Qm * c.Nl : 0); // some cb > C - gamma
          mx = n_e > mx ? n_e : mx;
        }
        if (mx <= lim.e_lim) {
          if (rm_rx_table_upload_compact(K, pc, d_rm_tbl_pc)) return SRSLTE_ERROR;
          pc_ok = true;
        }
      }
    }
    return SRSLTE_SUCCESS;
  }

  // d_w's slots in the compact parity layout back to the whole one (HARQ combining, a call the compact layout does not serve, the debug view)
  int w_whole(hipStream_t st)
  {
    if (!w_compact_n) return SRSLTE_SUCCESS;
    hipLaunchKernelGGL(rm_parity_expand_kernel, dim3(w_compact_n * seg.C), dim3(256), 0, st, d_w.get(), (int)in_stride, (int)seg.K1, (int)pc.phase[0],
                       (int)pc.phase[1]);
    LAUNCH_CHECK();
    w_compact_n = 0;
    return SRSLTE_SUCCESS;
  }

  // the rate de-matching table of rv, made on first use: an entry point calls this for a call's rv before it queues anything
  int ensure_rv(uint32_t rv) { return d_rm_tbl_rv[rv] ? SRSLTE_SUCCESS : rm_rx_table_upload(seg.K1, rv, W, in_stride, d_rm_tbl_rv[rv]); }

  // LLR rows d_e of subframes tti0 .. tti0 + nof_sf - 1 into the soft buffers of slots 0 .. nof_sf - 1; h.rv has been through ensure_rv
  int dematch(const void* d_e, uint32_t tti0, uint32_t nof_sf, SchHarq h, hipStream_t st)
  {
    RmGeom g  = rg;
    g.tti0    = (int)tti0;
    g.combine = h.combine;
    g.skip    = h.combine ? d_cb_ok : nullptr;
    const uint32_t* tbl = d_rm_tbl_rv[h.rv];
    // New data at rv 0 goes to the compact parity layout where the object has it. Anything else works on the whole layout: slots a compact
    // call left are expanded first if this call combines with them or does not overwrite all of them
    last_compact = pc_ok && h.rv == 0 && !h.combine;
    if (last_compact) {
      tbl         = d_rm_tbl_pc;
      g.w_len     = (int)pc.len;
      w_compact_n = nof_sf > w_compact_n ? nof_sf : w_compact_n;
    } else if (h.combine || nof_sf < w_compact_n) {
      if (int r = w_whole(st)) return r;
    } else {
      w_compact_n = 0;
    }
    if (cfg.llr_8bit) return rm_rx_launch<int8_t>(rm_lds_bytes(g, 1), nof_sf * seg.C, d_e, d_w, tbl, g, st);
    return rm_rx_launch<int16_t>(rm_lds_bytes(g, 2), nof_sf * seg.C, d_e, d_w, tbl, g, st);
  }

  // d_tb / d_tb_ok: the rows assemble() will be given, or null
  int decode(uint32_t nof_sf, SchHarq h, uint8_t* d_tb, uint32_t tb_stride, uint8_t* d_tb_ok, hipStream_t st)
  {
    const uint32_t C = seg.C, K = seg.K1;
    TdecOpts       o;
    o.tb_rem = d_tb_rem; o.tb_C = C; o.tb_syn = d_cb_syn;
    o.skip   = h.combine ? d_cb_ok.get() : nullptr;
    if (w_compact_n && w_compact_n < nof_sf) { // a decoder run over more slots than the last compact call filled
      if (int r = w_whole(st)) return r;
    }
    if (w_compact_n) {
      o.pc = 1; o.pc_phase[0] = pc.phase[0]; o.pc_phase[1] = pc.phase[1];
    }
    // The 16-window 16-bit decoder (K > 800) and the two 8-bit back-ends (avx8, sse8) assemble the transport blocks themselves when nothing of an earlier
    // transmission has to be merged in: assemble() is then empty. (HARQ combining keeps blocks of earlier calls, the short-block decoders have no such mode:
    // tb_asm / tb_crc.)
    direct_tb = nullptr;
    if (cfg.may_direct && d_tb_rem && (cfg.llr_8bit ? W >= 16 : W == 16) && !h.combine && d_tb && d_tb_ok && tb_stride >= cfg.tbs / 8 + 6) {
      o.tb_out = d_tb; o.tb_out_stride = tb_stride; o.tb_rb = tg.rlen / 8; o.tb_ok_out = d_tb_ok;
      direct_tb = d_tb; direct_ok = d_tb_ok; direct_stride = tb_stride; direct_nof_sf = nof_sf;
    }
    return tdec_run_batch_w(tdec, d_w, cfg.llr_8bit ? 1 : 0, in_stride, W != 0, K, -1, nof_sf * C, cfg.max_iterations, C > 1 ? 0x1800063u : 0x1864CFBu,
                            C > 1 ? K : cfg.tbs + 24, d_cb_bytes, K / 8, d_cb_iters, d_cb_ok, st, o);
  }

  // rows 0 .. nof_sf - 1 of d_tb (tb_stride >= tbs / 8 + 6) / d_tb_ok
  int assemble(uint32_t nof_sf, uint8_t* d_tb, uint32_t tb_stride, uint8_t* d_tb_ok, hipStream_t st)
  {
    // decode() assembled these transport blocks and gave these verdicts; other outputs: the assembly kernel, from the blocks' bytes and CRC
    // syndromes, which the decoders store in that mode as well
    if (direct_tb && direct_tb == d_tb && direct_ok == d_tb_ok && direct_stride == tb_stride && direct_nof_sf == nof_sf) return SRSLTE_SUCCESS;
    TbGeom g    = tg;
    g.tb_stride = (int)tb_stride;
    g.iters     = d_cb_iters;
    if (d_tb_rem) {
      hipLaunchKernelGGL(tb_asm_kernel, dim3(nof_sf), dim3(256), 0, st, (const uint8_t*)d_cb_bytes, (const uint8_t*)d_cb_ok, (const uint32_t*)d_cb_syn, d_tb,
                         d_tb_ok, g);
    } else {
      hipLaunchKernelGGL(tb_crc_kernel, dim3(nof_sf), dim3(512), 0, st, (const uint8_t*)d_cb_bytes, (const uint8_t*)d_cb_ok, (const uint32_t*)d_tbcrc, d_tb,
                         d_tb_ok, g);
    }
    LAUNCH_CHECK();
    return SRSLTE_SUCCESS;
  }
};
