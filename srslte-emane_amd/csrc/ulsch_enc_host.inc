// Fragment of pdsch.hip: ONE PUSCH transport block with its UCI into the caller's HOST buffers in one device call, transmit side - what
// srslte_ulsch_encode does (sch.c:1068-1210): the coded CQI report in front of the stream g (srslte_uci_encode_cqi_pusch, uci.c:467-494), the
// UL-SCH behind it at bit granularity (encode_tb_off with w_offset = e_offset % 8, here any offset), the channel interleaver with the rank
// indication's symbols left out of its read order (ulsch_interleave :580-888) and the HARQ-ACK symbols over what it wrote (:1194-1205). On the
// object, stream and circular-buffer chain of sch_enc_host.inc; the counterpart of ulsch_host.inc. The batched PUSCH transmitter (pusch_tx.inc)
// fuses all of this into its modulation and never materialises g or q; new here are the two kernels that do, in PACKED bits.
namespace {

// sch_enc_select_kernel's selection for a word that need not begin on a word of e - its twin, kept apart so that the DL-SCH kernel stays the
// code it was. Bits [first, 32) of the 32-bit word whose bit 0 is bit g0 of the transport block's e (g0 + first >= 0; 36.212 5.1.4.1.2): each
// bit is fetched from the circular buffer of the block it belongs to, from the rv's start on and round at 3K + 12, so a word that straddles a
// block boundary is composed by one thread. w: as sch_enc_select_kernel takes it, read a byte at a time, each byte once per run of bits.
// Bits past `total`: 0.
__device__ __forceinline__ uint32_t ulsch_enc_select_word(const uint8_t* __restrict__ w, const SchEncGeom& g, int g0, int first)
{
  int c, n;
  const int lo = g.C_lo * g.n_lo, e0 = g0 + first;
  if (e0 < lo) {
    c = e0 / g.n_lo;
    n = e0 - c * g.n_lo;
  } else {
    c = g.C_lo + (e0 - lo) / g.n_hi;
    n = (e0 - lo) % g.n_hi;
  }
  int            pos = (g.r + n) % g.L, at = -1;
  uint32_t       v = 0, byte = 0;
  const uint8_t* wc = w + (size_t)c * g.w_words * 4;
  for (int b = first; b < 32 && g0 + b < g.total; b++) {
    while (n >= (c < g.C_lo ? g.n_lo : g.n_hi)) { // the next block (one that carries no bits is passed over)
      c++;
      n = 0; pos = g.r; at = -1;
      wc = w + (size_t)c * g.w_words * 4;
    }
    if ((pos >> 3) != at) {
      at   = pos >> 3;
      byte = wc[at];
    }
    if ((byte >> (7 - (pos & 7))) & 1) v |= packed_bit(b);
    n++;
    pos = pos + 1 == g.L ? 0 : pos + 1;
  }
  return v;
}

// grid = ceil(nwords / 256), 256 threads: the packed g. A thread owns one 32-bit word: its bits below `off` are the coded report's (qc, one bit
// per byte, pusch_cqi_encode_kernel's output), the rest the UL-SCH's selection from bit 0 of e on. The word that holds the last report bits and
// the first UL-SCH bits is composed by one thread; nothing is read back. Stored to the device copy the interleaver reads and to the pinned
// copy g_bits is filled from. Bits past off + total of the last word: 0.
__global__ __launch_bounds__(256) void ulsch_enc_g_kernel(const uint8_t* __restrict__ w, const uint8_t* __restrict__ qc, uint32_t* __restrict__ g_dev,
                                                          uint32_t* __restrict__ g_host, SchEncGeom g, int off, int nwords)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nwords) return;
  const int g0 = 32 * i - off, first = g0 < 0 ? (g0 < -32 ? 32 : -g0) : 0;
  uint32_t  v = 0;
  for (int b = 0; b < first; b++) {
    if (qc[32 * i + b] & 1) v |= packed_bit(b);
  }
  if (first < 32 && g0 + first < g.total) v |= ulsch_enc_select_word(w, g, g0, first);
  g_dev[i]  = v;
  g_host[i] = v;
}

struct UlschEncGeom {
  int      rows, cols, Qm, nof_bits; // the channel interleaver's matrix (36.212 5.2.2.8): cols = N_pusch_symb, rows = H' / cols, Qm bits per entry
  AckGeom  ack, ri;                  // O = number of bits, Qprime coded symbols
  uint32_t ack_ones, ri_ones;        // bit m: coded bit m of one period of the sequence is UCI_BIT_1 (the only type that sets a bit, sch.c:1197)
  int      ack_period, ri_period;    // coded bit e of the ACK / RI has the type of e % period
};

// grid = ceil(ceil(nof_bits / 32) / 256), 256 threads: the channel interleaver with RI and ACK insertion. A thread owns one 32-bit word of q and
// walks its bits p: entry p / Qm of the column-major matrix is (row, col) = (entry % rows, entry / rows). An ACK entry takes its coded type and
// overrides whatever the interleaver reads there; an RI entry takes its coded type; any other takes g's entry row cols + col - (RI entries before
// it in the row-major read order). Which of the three, and that count, are pusch_rx.inc's closed forms of (row, col, Q'): no table, no scratch.
// g is read from its device copy a byte at a time, each byte once per run of bits: a thread's 32 bits come from 32 / Qm entries of one column,
// cols Qm bits apart in g, so from a window of 32 cols bits - 48 bytes or fewer -, and the 10.8 KB of g at most stay in the vector L1.
// Bits past nof_bits of the last word: 0.
__global__ __launch_bounds__(256) void ulsch_enc_interleave_kernel(const uint8_t* __restrict__ g, uint32_t* __restrict__ q, UlschEncGeom u)
{
  const int i = blockIdx.x * 256 + threadIdx.x, p0 = 32 * i;
  if (p0 >= u.nof_bits) return;
  int      s = p0 / u.Qm, k = p0 - s * u.Qm, col = s / u.rows, row = s - col * u.rows;
  int      at = -1, src = 0, m = 0, kind = -1; // kind: -1 not looked at yet, 0 a g entry from bit src, 1 ACK / 2 RI from coded bit m
  uint32_t v = 0, byte = 0;
  for (int b = 0; b < 32 && p0 + b < u.nof_bits; b++) {
    if (kind < 0) {
      const int ai = ack_symbol_index(u.ack, col, row, u.rows, u.cols), ri = ri_symbol_index(u.ri, col, row, u.rows, u.cols);
      kind = ai >= 0 ? 1 : (ri >= 0 ? 2 : 0);
      m    = (ai >= 0 ? ai : ri) * u.Qm;
      src  = (row * u.cols + col - ri_before(u.ri, col, row, u.rows, u.cols)) * u.Qm;
    }
    uint32_t bit;
    if (kind == 0) {
      const int e = src + k;
      if ((e >> 3) != at) {
        at   = e >> 3;
        byte = g[at];
      }
      bit = (byte >> (7 - (e & 7))) & 1u;
    } else if (kind == 1) {
      bit = (u.ack_ones >> ((m + k) % u.ack_period)) & 1u;
    } else {
      bit = (u.ri_ones >> ((m + k) % u.ri_period)) & 1u;
    }
    if (bit) v |= packed_bit(b);
    if (++k == u.Qm) {
      k = 0; kind = -1;
      if (++row == u.rows) row = 0, col++;
    }
  }
  q[i] = v;
}

constexpr size_t UL_ENC_O_RM = 64; // the pinned block's report bits end here

int ulsch_enc_init(srslte_hip_sch_enc* q)
{
  if (q->d_g) return SRSLTE_SUCCESS;
  const size_t words = ((size_t)q->max_e + 31) / 32 + 1, wb = (words * 4 + 63) & ~(size_t)63;
  q->o_ul_g = (UL_ENC_O_RM + (size_t)q->max_e * 2 + 63) & ~(size_t)63;
  q->o_ul_q = q->o_ul_g + wb;
  if (q->h_ul.alloc(q->o_ul_q + wb) || q->d_qcqi.alloc((size_t)q->max_e + 32) || q->d_g.alloc(words)) {
    hip_log("[srslte_hip] sch_enc: allocation for the UL-SCH call failed\n");
    return SRSLTE_ERROR;
  }
  return SRSLTE_SUCCESS;
}

// the bits of one period of lte_uci_ack_ri_types that are UCI_BIT_1; *period stays 1 without bits
uint32_t ulsch_enc_ones(const uint8_t* d, uint32_t O, uint32_t Qm, int* period)
{
  uint8_t        t[32];
  const uint32_t n = lte_uci_ack_ri_types(d, O, Qm, t);
  uint32_t       ones = 0;
  for (uint32_t i = 0; i < n; i++) ones |= t[i] == 1 ? 1u << i : 0u;
  *period = n ? (int)n : 1;
  return ones;
}

// what a call is made of, from its configuration alone
struct UlschEncPlan {
  srslte_hip_cbsegm_t        seg;
  srslte_hip_pusch_uci_res_t uci;
};

} // namespace

// The checks of srslte_hip_ulsch_encode on the configuration and the caller's buffers alone, with its codes, and the sizes they lead to: no
// object, nothing queued
static int ulsch_enc_plan(const srslte_hip_ulsch_enc_cfg_t* c, const uint8_t* data, uint8_t** buffer_b, UlschEncPlan* pl)
{
  if (!c || c->mod < 1 || c->mod > 3 || c->rv > 3) return SRSLTE_ERROR_INVALID_INPUTS;
  const uint32_t Qm = 2 * (uint32_t)c->mod, nsymb = c->nof_symb;
  if (nsymb < 9 || nsymb > 12 || c->L_prb == 0 || c->L_prb > 110 || c->nof_bits != 12 * c->L_prb * nsymb * Qm || c->ri_len > 2 || c->ack_len > 10 ||
      c->cqi_len > 64 || c->I_offset_ack > 15 || c->I_offset_ri > 15 || c->I_offset_cqi > 15 || (c->tbs % 8))
    return SRSLTE_ERROR_INVALID_INPUTS;
  srslte_hip_cbsegm_t& seg = pl->seg;
  memset(&seg, 0, sizeof(seg));
  if (int r = c->tbs ? sch_enc_check(data, c->tbs, c->rv, buffer_b, &seg) : 0) return r;
  const srslte_hip_pusch_uci_cfg_t uc = {c->L_prb,   nsymb,     Qm,         12 * c->L_prb,   seg.C * seg.K1,   seg.C,
                                         c->ack_len, c->ri_len, c->cqi_len, c->I_offset_ack, c->I_offset_ri, c->I_offset_cqi};
  const int why = srslte_hip_pusch_uci_plan(&uc, &pl->uci);
  if (why == SRSLTE_HIP_PUSCH_UCI_BETA) {
    hip_log("Error beta is reserved\n"); // uci.c:475-478,:705-708
    return -1;
  }
  if (why == SRSLTE_HIP_PUSCH_UCI_EMPTY) // upstream would interleave stale scratch
    hip_log("[srslte_hip] ulsch_enc: a PUSCH without UL-SCH data carries a CQI report (36.212 5.2.4)\n");
  if (why == SRSLTE_HIP_PUSCH_UCI_NO_ROOM)
    hip_log("[srslte_hip] ulsch_enc: Q'_ri %u + Q'_cqi %u leave no symbol of %u to the UL-SCH\n", pl->uci.Qp_ri, pl->uci.Qp_cqi, uc.rows * nsymb);
  return why ? SRSLTE_ERROR_INVALID_INPUTS : SRSLTE_SUCCESS;
}
int ulsch_enc_check(const srslte_hip_ulsch_enc_cfg_t* c, const uint8_t* data, uint8_t** buffer_b)
{
  UlschEncPlan pl;
  return ulsch_enc_plan(c, data, buffer_b, &pl);
}

// data, buffer_b: as srslte_hip_sch_encode takes them (not looked at with tbs = 0). q_bits: cfg->nof_bits / 8 bytes, all written. g_bits: null,
// or (H' - Q'_ri) Qm bits from bit 0, the rest of the last byte keeping the caller's value. Everything is checked before anything is queued or
// written.
extern "C" int srslte_hip_ulsch_encode(srslte_hip_sch_enc_t* q, const uint8_t* data, const srslte_hip_ulsch_enc_cfg_t* c, uint8_t** buffer_b,
                                       uint8_t* g_bits, uint8_t* q_bits, srslte_hip_ulsch_enc_res_t* res)
{
  if (!q || !c || !q_bits || !res) return SRSLTE_ERROR_INVALID_INPUTS;
  UlschEncPlan pl;
  if (int r = ulsch_enc_plan(c, data, buffer_b, &pl)) return r;
  if (c->nof_bits > q->max_e || c->tbs > q->max_tbs) return SRSLTE_ERROR_INVALID_INPUTS;
  const srslte_hip_cbsegm_t& seg = pl.seg;
  const uint32_t Qm = 2 * (uint32_t)c->mod, nsymb = c->nof_symb, rows = 12 * c->L_prb, Qp_ack = pl.uci.Qp_ack, Qp_ri = pl.uci.Qp_ri, Qp_cqi = pl.uci.Qp_cqi;
  if (ulsch_enc_init(q)) return SRSLTE_ERROR;
  const srslte_hip_sch_enc::KTab* kt = c->tbs ? q->table(seg.K1) : nullptr;
  if (c->tbs && !kt) return SRSLTE_ERROR;

  hipStream_t st = q->st;
  uint8_t*    h_cqi = q->h_ul;
  uint16_t*   h_rm  = reinterpret_cast<uint16_t*>(q->h_ul + UL_ENC_O_RM);
  uint32_t *  h_g = reinterpret_cast<uint32_t*>(q->h_ul + q->o_ul_g), *h_q = reinterpret_cast<uint32_t*>(q->h_ul + q->o_ul_q);
  // ---- the coded report: bits [0, Q'_cqi Qm) of g
  const int off = (int)pl.uci.Q_cqi;
  if (off) {
    memcpy(h_cqi, c->cqi_bits, 64);
    if (c->cqi_len > 11) { // the rate matching of the convolutional code: cqi_rm_conv_order read circularly
      const std::vector<uint16_t> order = cqi_rm_conv_order(c->cqi_len);
      for (int i = 0; i < off; i++) h_rm[i] = order[(size_t)i % order.size()];
    }
    hipLaunchKernelGGL(pusch_cqi_encode_kernel, dim3(1), dim3(256), 0, st, (const uint8_t*)h_cqi, q->d_qcqi.get(), 0, off, (int)c->cqi_len, (const uint16_t*)h_rm);
    LAUNCH_CHECK();
  }
  // ---- the UL-SCH behind it: G = H' - Q'_ri - Q'_cqi symbols (sch.c:1159-1166)
  SchEncGeom sg;
  memset(&sg, 0, sizeof(sg));
  const uint8_t* w_src = nullptr;
  if (c->tbs) {
    sg = sch_enc_geom(q, kt, seg.C, seg.K1, Qm, pl.uci.G_prime, c->rv);
    if (int r = sch_enc_queue_w(q, kt, data, c->tbs, c->rv, buffer_b, sg, &w_src)) return r;
  }
  const int g_bits_n = off + sg.total, g_words = ceil_div(g_bits_n, 32);
  hipLaunchKernelGGL(ulsch_enc_g_kernel, dim3(ceil_div(g_words, 256)), dim3(256), 0, st, w_src, (const uint8_t*)q->d_qcqi, q->d_g.get(), h_g, sg, off, g_words);
  LAUNCH_CHECK();
  q->g_words = (uint32_t)g_words;
  // ---- the channel interleaver with the RI and ACK symbols
  uint8_t      ri_bits[2] = {c->ri, 0}; // sch.c:1115: a 2-bit rank indication sends the value and a zero
  UlschEncGeom u;
  u.rows = (int)rows; u.cols = (int)nsymb; u.Qm = (int)Qm; u.nof_bits = (int)c->nof_bits;
  u.ack = AckGeom{(int)c->ack_len, (int)Qp_ack};
  u.ri  = AckGeom{(int)c->ri_len, (int)Qp_ri};
  u.ack_ones = ulsch_enc_ones(c->ack, c->ack_len, Qm, &u.ack_period);
  u.ri_ones  = ulsch_enc_ones(ri_bits, c->ri_len, Qm, &u.ri_period);
  hipLaunchKernelGGL(ulsch_enc_interleave_kernel, dim3(ceil_div(ceil_div((int)c->nof_bits, 32), 256)), dim3(256), 0, st,
                     reinterpret_cast<const uint8_t*>(q->d_g.get()), h_q, u);
  LAUNCH_CHECK();
  HIP_TRY(hipStreamSynchronize(st));
  memcpy(q_bits, h_q, c->nof_bits / 8);
  if (g_bits) sch_enc_copy_bits(g_bits, reinterpret_cast<const uint8_t*>(h_g), (size_t)g_bits_n);
  if (c->tbs && c->rv == 0) sch_enc_copy_w(q, sg, buffer_b);
  res->Q_prime_ack = Qp_ack; res->Q_prime_ri = Qp_ri; res->Q_prime_cqi = Qp_cqi;
  res->stream_waits = 1;
  return SRSLTE_SUCCESS;
}

extern "C" int srslte_hip_ulsch_enc_debug(srslte_hip_sch_enc_t* q, uint32_t* out, uint32_t n_words)
{
  if (!q || !out || !q->d_g || n_words > q->g_words) return SRSLTE_ERROR_INVALID_INPUTS;
  HIP_TRY(hipMemcpy(out, q->d_g.get(), (size_t)n_words * 4, hipMemcpyDeviceToHost));
  return SRSLTE_SUCCESS;
}
