// Fragment of pdsch.hip: ONE transport block with HOST buffers in one device call - what decode_tb_cb does (sch.c:299-414) behind
// srslte_dlsch_decode2 (sch.c:507-531): rate de-matching of every code block into its soft buffer (added, rm_turbo.c:407-409), turbo
// decoding with CRC early stop, decoded bytes. The single-call turbo decoder API costs a host round trip per code block AND per pass
// (srslte_tdec_iteration): 13 x 1-6 of them for a 20 MHz transport block; this entry costs one.
// The caller's srslte_softbuffer_rx_t stays the HARQ state, in host memory as upstream: soft buffers of blocks still to decode go up
// (unless all zero: a fresh buffer, srslte_softbuffer_rx_reset_tbs) and those that failed come back; blocks whose CRC passed in an
// earlier transmission are neither combined nor decoded (sch.c:317-318). Built on the grants machinery (one slot).
struct srslte_hip_sch {
  GrantsState  gs;
  uint32_t     max_tbs = 0, max_e = 0, Cmax = 0;
  bool         l8 = false;
  hipStream_t  st = nullptr;
  PinBuf       h_pin; // pinned: e_bits | soft buffers [Cmax][stride] | bytes [Cmax][768] | flags [Cmax] | passes [Cmax]
  size_t       o_w = 0, o_bytes = 0, o_ok = 0, o_it = 0, pin_bytes = 0;
  // srslte_hip_ulsch_decode (ulsch_host.inc), made by its first call: the interleaved LLRs, the UCI sums, and pinned memory its kernels read
  // (c_seq at the ACK / RI positions) and write (decisions, report)
  DevBuf<int16_t> d_q;
  DevBuf<int>     d_uci_sum;
  PinBuf          h_ul;
  uint32_t        g_len = 0; // LLRs of the last srslte_hip_ulsch_decode in d_e (srslte_hip_ulsch_debug_g)
  // srslte_hip_pusch_decode (pusch_host.inc), made by its first call: the allocation's rows of grid and estimates (pinned, then device), the
  // equalised and the de-precoded symbols, and c_seq at the ACK / RI positions from the device's own sequence
  PinBuf          h_re;
  DevBuf<cf32>    d_re, d_z, d_d;
  DevBuf<uint8_t> d_cs;
  uint32_t        q_len = 0; // LLRs of the last srslte_hip_pusch_decode in d_q (srslte_hip_pusch_debug_q)
  ~srslte_hip_sch()
  {
    if (st) (void)hipStreamSynchronize(st); // a decode that returned early may have left copies queued: they end before the buffers go
    if (st) (void)hipStreamDestroy(st);
  }
};

extern "C" void srslte_hip_sch_destroy(srslte_hip_sch_t* q) { delete q; }

extern "C" srslte_hip_sch_t* srslte_hip_sch_create(uint32_t max_tbs, uint32_t max_e_bits, int llr_8bit)
{
  srslte_hip_cbsegm_t seg;
  if (max_tbs == 0 || max_tbs > (uint32_t)TB_MAX_BITS || max_e_bits == 0 || srslte_hip_cbsegm(&seg, max_tbs)) {
    hip_log("[srslte_hip] sch: invalid max_tbs=%u / max_e_bits=%u\n", max_tbs, max_e_bits);
    return nullptr;
  }
  std::unique_ptr<srslte_hip_sch> q(new srslte_hip_sch());
  q->max_tbs = max_tbs; q->max_e = max_e_bits; q->Cmax = seg.C; q->l8 = llr_8bit != 0;
  const size_t esz = q->l8 ? 1 : 2;
  bool ok = grants_alloc(&q->gs, (max_e_bits + 7) / 8, 1, q->Cmax, 0, false, 0) == SRSLTE_SUCCESS &&
            hipStreamCreateWithFlags(&q->st, hipStreamNonBlocking) == hipSuccess;
  q->o_w     = ((size_t)q->gs.max_bits * esz + 63) & ~(size_t)63;
  q->o_bytes = q->o_w + (((size_t)q->Cmax * q->gs.stride * esz + 63) & ~(size_t)63);
  q->o_ok    = q->o_bytes + (size_t)q->Cmax * 768;
  q->o_it    = (q->o_ok + q->Cmax + 63) & ~(size_t)63;
  q->pin_bytes = q->o_it + (size_t)q->Cmax * 4;
  if (!ok || q->h_pin.alloc(q->pin_bytes)) {
    hip_log("[srslte_hip] sch: initialisation failed\n");
    return nullptr;
  }
  return q.release();
}

// e_bits: nof_e_bits LLRs of the transport block (int16, or int8 if the object was made for 8-bit LLRs). mod: 1 QPSK .. 4 256QAM; Nl as
// srslte_dlsch_decode2 derives it (2 where nof_layers != nof_tb). buffer_f[c] / cb_crc[c]: the srslte_softbuffer_rx_t's arrays of the C
// code blocks (in / out). cb_bytes: [C][768] decoded bytes of the blocks decoded by THIS call (K / 8 each, block CRC included); blocks
// with cb_crc set on entry are left alone. sum_passes: SISO passes over all decoded blocks (avg_iterations x C).
// e_bits = null (srslte_hip_ulsch_decode): the LLRs are what the stream has already been told to write to d_e, the transport block's from e_off
// on, and the call waits for the stream even when no block is left to decode (the UCI results come down with it). waits: stream waits, added
static int sch_decode_run(srslte_hip_sch_t* q, const void* e_bits, uint32_t nof_e_bits, uint32_t e_off, uint32_t tbs, int mod, uint32_t Nl, uint32_t rv,
                          uint32_t max_iterations, int16_t** buffer_f, uint8_t* cb_crc, uint8_t* cb_bytes, uint32_t* sum_passes, uint32_t* waits)
{
  if (!q || !buffer_f || !cb_crc || !cb_bytes || nof_e_bits == 0 || nof_e_bits > q->max_e || max_iterations == 0 || Nl < 1 || Nl > 2 || mod < 1 || mod > 4)
    return SRSLTE_ERROR_INVALID_INPUTS;
  GrantsState*   g    = &q->gs;
  const size_t   esz  = q->l8 ? 1 : 2;
  uint8_t*       h_pin = nullptr;
  if (int r = g->desc.begin(&h_pin)) return r;
  const GrantsDesc h(g, h_pin), d(g, g->desc.dev_bytes());
  SfDesc*          h_sf = h.sf;
  CbDesc*          h_cb = h.cb;
  memset(h.gr, 0, sizeof(GrantDev));
  memset(h_sf, 0, sizeof(SfDesc));
  GrantsBuild bd;
  bd.g = g; bd.h_sf = h_sf; bd.h_cb = h_cb; bd.l8 = q->l8; bd.max_tbs = q->max_tbs; bd.npt = 1; bd.max_mod = 4; bd.who = "sch";
  const uint32_t Qm = 2 * (uint32_t)mod;
  if (int r = bd.add_tb(0, 0, mod, tbs, rv, 0, nof_e_bits / Qm, Nl, e_off)) return r;
  const uint32_t C = (uint32_t)h_sf[0].C, K = (uint32_t)h_sf[0].K;
  const uint32_t W = q->l8 ? srslte_hip_tdec_autoimp_get_subblocks_8bit(K) : srslte_hip_tdec_autoimp_get_subblocks(K);
  const uint32_t len = srslte_hip_tdec_input_len(K, W != 0); // meaningful soft-buffer elements of a block
  hipStream_t    st = q->st;
  // ---- soft buffers up: blocks still to decode whose buffer holds something; an all-zero one is overwritten on the device instead
  uint8_t* h_ok = q->h_pin + q->o_ok;
  uint32_t todo = 0;
  for (uint32_t c = 0; c < C; c++) {
    h_ok[c] = cb_crc[c] ? 1 : 0;
    h_cb[c].combine = 1;
    if (cb_crc[c]) continue;
    todo++;
    const uint8_t* src = reinterpret_cast<const uint8_t*>(buffer_f[c]);
    bool           any = false;
    const uint64_t* s8 = reinterpret_cast<const uint64_t*>(src);
    const size_t    n8 = (size_t)len * esz / 8;
    for (size_t i = 0; i + 8 <= n8 && !any; i += 8) any = (s8[i] | s8[i + 1] | s8[i + 2] | s8[i + 3] | s8[i + 4] | s8[i + 5] | s8[i + 6] | s8[i + 7]) != 0;
    for (size_t i = n8 / 8 * 64; i < (size_t)len * esz && !any; i++) any = src[i] != 0;
    if (!any) {
      h_cb[c].combine = 0;
      continue;
    }
    uint8_t* stage = q->h_pin + q->o_w + (size_t)c * g->stride * esz;
    memcpy(stage, src, (size_t)len * esz);
    HIP_TRY(hipMemcpyAsync((uint8_t*)g->d_w.get() + (size_t)c * g->stride * esz, stage, (size_t)len * esz, hipMemcpyHostToDevice, st));
  }
  if (sum_passes) *sum_passes = 0;
  if (todo == 0) {
    if (!e_bits) {
      HIP_TRY(hipStreamSynchronize(st));
      ++*waits;
    }
    return SRSLTE_SUCCESS;
  }
  bd.fill_map(h.map);
  if (e_bits) {
    memcpy(q->h_pin, e_bits, (size_t)nof_e_bits * esz);
    HIP_TRY(hipMemcpyAsync(g->d_e, q->h_pin, (size_t)nof_e_bits * esz, hipMemcpyHostToDevice, st));
  }
  HIP_TRY(hipMemcpyAsync(g->d_cb_ok, h_ok, C, hipMemcpyHostToDevice, st));
  if (int r = g->desc.commit(g->desc_bytes, st)) return r;
  // no transport-block assembly on the device: the caller (sch.c's decode_tb, compat) assembles from the blocks' bytes as upstream does
  if (int r = grants_back_end(g, bd, d.sf, d.cb, d.map, 0, max_iterations, 1, 1, 0, nullptr, 0, nullptr, st)) return r;
  // ---- results down: bytes, flags, pass counts; the soft buffers of blocks that failed (the next transmission combines into them)
  uint8_t*  h_bytes = q->h_pin + q->o_bytes;
  uint8_t*  h_ok2   = q->h_pin + q->o_ok;
  uint32_t* h_it    = reinterpret_cast<uint32_t*>(q->h_pin + q->o_it);
  HIP_TRY(hipMemcpyAsync(h_bytes, g->d_cb_bytes, (size_t)C * 768, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(h_it, g->d_cb_iters, (size_t)C * 4, hipMemcpyDeviceToHost, st));
  std::vector<uint8_t> was(cb_crc, cb_crc + C);
  HIP_TRY(hipMemcpyAsync(h_ok2, g->d_cb_ok, C, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  ++*waits;
  uint32_t failed = 0, passes = 0;
  for (uint32_t c = 0; c < C; c++) {
    if (was[c]) continue;
    passes += h_it[c];
    memcpy(cb_bytes + (size_t)c * 768, h_bytes + (size_t)c * 768, K / 8);
    cb_crc[c] = h_ok2[c];
    if (!h_ok2[c]) {
      failed++;
      HIP_TRY(hipMemcpyAsync(q->h_pin + q->o_w + (size_t)c * g->stride * esz, (uint8_t*)g->d_w.get() + (size_t)c * g->stride * esz, (size_t)len * esz,
                             hipMemcpyDeviceToHost, st));
    }
  }
  if (failed) {
    HIP_TRY(hipStreamSynchronize(st));
    ++*waits;
    for (uint32_t c = 0; c < C; c++) {
      if (was[c] || cb_crc[c]) continue;
      memcpy(buffer_f[c], q->h_pin + q->o_w + (size_t)c * g->stride * esz, (size_t)len * esz);
      if (W != 0) {
        // upstream's decoder reads an SB-layout buffer in place and, on its first pass, puts the tail LLRs behind the three K-long rows OF
        // THE CALLER'S BUFFER (extract_input_tail_sb, turbodecoder_iter.h:55-64): part of the soft buffer's state a caller can see
        const size_t T = 3 * ((size_t)K + 32);
        auto put = [&](size_t dst, size_t src) {
          if (q->l8) reinterpret_cast<int8_t*>(buffer_f[c])[dst] = reinterpret_cast<int8_t*>(buffer_f[c])[src];
          else buffer_f[c][dst] = buffer_f[c][src];
        };
        for (uint32_t i = 0; i < 3; i++) {
          put(K + i, T + 2 * i);
          put((K + 32) + K + i, T + 2 * i + 1);
          put(2 * ((size_t)K + 32) + K + i, T + 6 + 2 * i + 1);
        }
      }
    }
  }
  if (sum_passes) *sum_passes = passes;
  return SRSLTE_SUCCESS;
}

extern "C" int srslte_hip_sch_decode(srslte_hip_sch_t* q, const void* e_bits, uint32_t nof_e_bits, uint32_t tbs, int mod, uint32_t Nl, uint32_t rv,
                                     uint32_t max_iterations, int16_t** buffer_f, uint8_t* cb_crc, uint8_t* cb_bytes, uint32_t* sum_passes)
{
  uint32_t waits = 0;
  if (!e_bits) return SRSLTE_ERROR_INVALID_INPUTS;
  return sch_decode_run(q, e_bits, nof_e_bits, 0, tbs, mod, Nl, rv, max_iterations, buffer_f, cb_crc, cb_bytes, sum_passes, &waits);
}
