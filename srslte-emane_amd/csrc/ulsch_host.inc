// Fragment of pdsch.hip: ONE PUSCH transport block with its UCI from the caller's descrambled LLRs in HOST memory, in one device call - what
// srslte_ulsch_decode does (sch.c:991-1066): uci_decode_ri_ack (:920-989, uci.c:627-654,:748-788), ulsch_deinterleave (:891-918), the CQI report
// in front of the UL-SCH (uci.c:423-463) and decode_tb. On the object and stream of sch_host.inc: the LLRs go up once, ulsch_deint_kernel
// writes the de-interleaved stream g straight into the back end's d_e, pusch_rx.inc's CQI decoder reads its first Q'_cqi Qm LLRs and the back end
// the rest; decisions, report, bytes, flags and pass counts come down with one stream wait (two when a block failed, sch_host.inc).
namespace {

struct UlschGeom {
  int     rows, cols, Qm;  // the channel interleaver's matrix (36.212 5.2.2.8): cols = N_pusch_symb, rows = H' / cols, Qm LLRs per entry
  AckGeom ack, ri;         // O = number of bits (ACK: 3 and more clear their positions and decide nothing), Qprime symbols
  int     ri_imax;         // the RI symbol that holds the largest RI position
};

// sums of one ACK / RI symbol (uci.c:627-654). x0, x1: its first two LLRs; cs: c_seq at those two positions (1-bit only)
__device__ __forceinline__ void ulsch_uci_sums(int O, int Qprime, int i, int16_t x0, int16_t x1, const uint8_t* __restrict__ cs, int* s)
{
  if (O == 1) { // decode_ri_ack_1bit: p1 descrambled in place, then scrambled with p0's bit; int16 negations as upstream's assignments
    const int16_t t  = cs[2 * i + 1] ? (int16_t)(-(int)x1) : x1;
    const int16_t q1 = cs[2 * i] ? (int16_t)(-(int)t) : t;
    s[0] += (int)x0 + (int)q1;
  } else if (O == 2 && i < 3 * ((Qprime - 1) / 3)) { // decode_ri_ack_2bits at i = 3, 6, .. over symbols i - 3 .. i - 1 (uci.c:775-776)
    const int r = i % 3;
    s[r == 0 ? 0 : (r == 1 ? 2 : 1)] += x0;
    s[r == 0 ? 1 : (r == 1 ? 0 : 2)] += x1;
  }
}

// One thread per matrix entry (row, col), in the row-major order g is written in: thread s reads the Qm LLRs q[(col rows + row) Qm ..] and writes
// them to g[(s - RI entries before it) Qm ..]. The STORES are the coalesced side (consecutive lanes, consecutive dwords; the rate de-matcher
// reads g with 16-byte loads next); the loads of a wavefront fall into `cols` runs of about 64 / cols entries, and the whole input - 170 KB at
// 100 PRB 64QAM - is L2-resident behind its upload. Positions come from pusch_rx.inc's arithmetic; nothing is looked up.
// What upstream's scatter g[lut[i]] = q[i] (ascending i, lut = 0 at RI positions) leaves: ACK entries reach g as zeros IN their data positions;
// RI entries reach nothing but g[0], which ends up with the LLR of the largest RI position - a 1-bit RI has flipped the sign of its p1 LLR in
// place, and with Qm = 2 that is the one. The Q'_ri Qm LLRs behind the stream, which upstream leaves as they were, are zeroed.
// sums[0..2] ACK, sums[4..6] RI (zero on entry). cs: [Q'_ack][2] then [Q'_ri][2] bits of c_seq at p0 / p1 of each symbol (1-bit cases).
__global__ __launch_bounds__(256) void ulsch_deint_kernel(const int16_t* __restrict__ q, const uint8_t* __restrict__ cs, int16_t* __restrict__ g,
                                                          int* __restrict__ sums, UlschGeom u)
{
  const int s = blockIdx.x * 256 + threadIdx.x, H = u.rows * u.cols, nw = u.Qm / 2;
  int       sa[3] = {0, 0, 0}, sr[3] = {0, 0, 0};
  bool      uci = false;
  if (s < H) {
    const int       row = s / u.cols, col = s - row * u.cols;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(q + (size_t)(col * u.rows + row) * u.Qm);
    uint32_t        w[3] = {0, 0, 0};
    for (int d = 0; d < nw; d++) w[d] = src[d];
    const int16_t x0 = (int16_t)(w[0] & 0xffffu), x1 = (int16_t)(w[0] >> 16);
    const int     ai = ack_symbol_index(u.ack, col, row, u.rows, u.cols), ri = ri_symbol_index(u.ri, col, row, u.rows, u.cols);
    if (ai >= 0) {
      ulsch_uci_sums(u.ack.O, u.ack.Qprime, ai, x0, x1, cs, sa);
      w[0] = w[1] = w[2] = 0; // sch.c:961-964
      uci = true;
    }
    uint32_t* dst;
    if (ri >= 0) {
      ulsch_uci_sums(u.ri.O, u.ri.Qprime, ri, x0, x1, cs + 2 * u.ack.Qprime, sr);
      w[0] = w[1] = w[2] = 0;
      uci = true;
      dst = reinterpret_cast<uint32_t*>(g + (size_t)(H - u.ri.Qprime + ri) * u.Qm);
    } else {
      const int idx = s - ri_before(u.ri, col, row, u.rows, u.cols);
      if (idx == 0 && u.ri.Qprime > 0) { // g[0]: the largest RI position, Qm - 1 of symbol ri_imax in the last row
        const int ccol = u.ri_imax == 0 ? (u.cols > 10 ? 1 : 0) : (u.cols > 10 ? 10 : 8);
        int16_t   v    = q[(size_t)(ccol * u.rows + u.rows - 1) * u.Qm + u.Qm - 1];
        if (u.ri.O == 1 && u.Qm == 2 && cs[2 * u.ack.Qprime + 2 * u.ri_imax + 1]) v = (int16_t)(-(int)v);
        w[0] = (w[0] & 0xffff0000u) | (uint16_t)v;
      }
      dst = reinterpret_cast<uint32_t*>(g + (size_t)idx * u.Qm);
    }
    for (int d = 0; d < nw; d++) dst[d] = w[d];
  }
  if (__any(uci)) { // wave-uniform: most wavefronts hold no UCI entry
    for (int k = 0; k < 3; k++) {
      const int a = wave_sum(sa[k]), r = wave_sum(sr[k]);
      if ((threadIdx.x & 63) == 0) {
        if (a) atomicAdd(sums + k, a);
        if (r) atomicAdd(sums + 4 + k, r);
      }
    }
  }
}

// decode_cqi_short folds the repetitions of the 32-bit code word into the first 32 LLRs of g IN PLACE before it correlates (uci.c:315-322,
// wrapping int16 adds); the CQI decoder has read g by now, this leaves g as upstream does
__global__ void ulsch_cqi_fold_kernel(int16_t* __restrict__ g, int Q)
{
  const int tid = threadIdx.x;
  int       a   = 0;
  for (int i = tid; i < Q; i += 32) a += g[i];
  g[tid] = (int16_t)a;
}

// pinned block of the UL call: decisions [4] (ACK 0, 1, RI 0, 1) | report bits [64] at 64 | its CRC flag at 128 | c_seq bits from 256 on
constexpr size_t UL_O_CQI = 64, UL_O_CRC = 128, UL_O_CS = 256;

int ulsch_init(srslte_hip_sch* q)
{
  if (q->d_q) return SRSLTE_SUCCESS;
  // c_seq bits: 2 per symbol, Q'_ack + Q'_ri <= 8 rows symbols, rows <= max_e / (2 x 9) - fewer than max_e bytes
  if (q->d_q.alloc((size_t)q->max_e + 16) || q->d_uci_sum.alloc(8) || q->h_ul.alloc(UL_O_CS + q->max_e)) {
    hip_log("[srslte_hip] sch: allocation for the UL-SCH call failed\n");
    return SRSLTE_ERROR;
  }
  return SRSLTE_SUCCESS;
}

} // namespace

// What both UL entries - srslte_hip_ulsch_decode here, srslte_hip_pusch_decode in pusch_host.inc - share: the plan (every check, nothing queued) and
// everything behind the upload of the LLRs (ulsch_run).
struct UlschPlan {
  uint32_t            Qm, nsymb, rows, H; // the channel interleaver's matrix: rows x nsymb entries of Qm LLRs
  uint32_t            Qp_ack, Qp_ri, Qc[2], len2; // Q'_cqi and the report's size for rank 1 / above (equal where the size does not depend on it)
  srslte_hip_cbsegm_t seg;
};

// Everything is checked before anything is queued. SRSLTE_ERROR for a reserved beta offset (with upstream's message), else SRSLTE_ERROR_INVALID_INPUTS.
static int ulsch_plan(srslte_hip_sch_t* q, const srslte_hip_ulsch_cfg_t* c, int16_t** buffer_f, const uint8_t* cb_crc, const uint8_t* cb_bytes, UlschPlan* p)
{
  if (!q || !c || q->l8 || c->mod < 1 || c->mod > 3) return SRSLTE_ERROR_INVALID_INPUTS;
  const uint32_t Qm = 2 * (uint32_t)c->mod, nsymb = c->nof_symb;
  if (nsymb < 9 || nsymb > 12 || c->L_prb == 0 || c->nof_bits == 0 || c->nof_bits > q->max_e || c->nof_bits % (nsymb * Qm) || c->ri_len > 2 || c->cqi_len > 64 ||
      c->cqi_len_rank2 > 64 || c->I_offset_ack > 15 || c->I_offset_ri > 15 || c->I_offset_cqi > 15)
    return SRSLTE_ERROR_INVALID_INPUTS;
  srslte_hip_cbsegm_t& seg = p->seg;
  memset(&seg, 0, sizeof(seg));
  if (c->tbs) {
    if (!buffer_f || !cb_crc || !cb_bytes || c->max_iterations == 0 || c->rv > 3 || c->tbs > q->max_tbs || srslte_hip_cbsegm(&seg, c->tbs) || seg.F || seg.C2 ||
        seg.C > q->Cmax)
      return SRSLTE_ERROR_INVALID_INPUTS;
  }
  const uint32_t rows = c->nof_bits / Qm / nsymb, H = rows * nsymb; // nof_bits is the caller's: the rows are not tied to 12 L_prb here
  const bool     cqi = c->cqi_len > 0;
  const srslte_hip_pusch_uci_cfg_t uc = {c->L_prb,   nsymb,     Qm,         rows,            seg.C * seg.K1,   seg.C,
                                         c->ack_len, c->ri_len, c->cqi_len, c->I_offset_ack, c->I_offset_ri, c->I_offset_cqi};
  srslte_hip_pusch_uci_res_t       pl;
  const int                        why = srslte_hip_pusch_uci_plan(&uc, &pl); // any ack_len: 3 bits and more clear their positions and decide nothing
  if (why == SRSLTE_HIP_PUSCH_UCI_BETA) {
    hip_log("Error beta is reserved\n"); // uci.c:432,:761
    return SRSLTE_ERROR;
  }
  if (why == SRSLTE_HIP_PUSCH_UCI_EMPTY) hip_log("[srslte_hip] ulsch: a PUSCH without UL-SCH data carries a CQI report (36.212 5.2.4)\n");
  if (why) return SRSLTE_ERROR_INVALID_INPUTS;
  // the report's size may depend on the rank (cqi_len_rank2): both hypotheses are sized before anything runs, each leaving every code block a symbol
  p->len2  = cqi && c->cqi_len_rank2 ? c->cqi_len_rank2 : c->cqi_len;
  p->Qc[0] = pl.Qp_cqi;
  p->Qc[1] = pusch_uci_cqi_qprime(&uc, p->len2, pl.Qp_ri);
  for (int k = 0; k < 2; k++) {
    if (pl.Qp_ri + p->Qc[k] > H || (c->tbs && H - pl.Qp_ri - p->Qc[k] < seg.C)) return SRSLTE_ERROR_INVALID_INPUTS;
  }
  p->Qm = Qm; p->nsymb = nsymb; p->rows = rows; p->H = H; p->Qp_ack = pl.Qp_ack; p->Qp_ri = pl.Qp_ri;
  return SRSLTE_SUCCESS;
}

// From the LLRs the stream has been told to leave in q->d_q: decisions, de-interleaver, report, transport block, results down.
// cs: [Q'_ack][2] then [Q'_ri][2] bits of c_seq at p0 / p1 of each ACK / RI symbol, where the kernels can read them (1-bit cases only)
static int ulsch_run(srslte_hip_sch_t* q, const srslte_hip_ulsch_cfg_t* c, const UlschPlan& p, const uint8_t* cs, int16_t** buffer_f, uint8_t* cb_crc,
                     uint8_t* cb_bytes, uint32_t* sum_passes, srslte_hip_ulsch_res_t* res)
{
  const uint32_t Qm = p.Qm, H = p.H, Qp_ack = p.Qp_ack, Qp_ri = p.Qp_ri, len2 = p.len2;
  const bool     cqi = c->cqi_len > 0;
  hipStream_t    st = q->st;
  uint8_t *      h_dec = q->h_ul, *h_cqi = q->h_ul + UL_O_CQI, *h_crc = q->h_ul + UL_O_CRC;
  memset(h_dec, 0, 4);
  memset(h_cqi, 0, 64); // uci.c / sch.c:1042: the report starts as zeros and a failed CRC leaves it so
  *h_crc = 0;
  HIP_TRY(hipMemsetAsync(q->d_uci_sum.get(), 0, sizeof(int) * 8, st));
  UlschGeom u;
  u.rows = (int)p.rows; u.cols = (int)p.nsymb; u.Qm = (int)Qm;
  u.ack = AckGeom{(int)c->ack_len, (int)Qp_ack};
  u.ri  = AckGeom{(int)c->ri_len, (int)Qp_ri};
  u.ri_imax = Qp_ri >= 2 ? 1 : 0;
  int16_t* d_g = q->gs.d_e;
  hipLaunchKernelGGL(ulsch_deint_kernel, dim3(ceil_div((int)H, 256)), dim3(256), 0, st, (const int16_t*)q->d_q, cs, d_g, q->d_uci_sum.get(), u);
  LAUNCH_CHECK();
  q->g_len = c->nof_bits;
  uint32_t waits = 0;
  if (c->ack_len || c->ri_len) { // rows 0 / 1 of the decision kernel: ACK, RI
    hipLaunchKernelGGL(pusch_ack_decide_kernel, dim3(1), dim3(64), 0, st, (const int*)q->d_uci_sum, h_dec, 2);
    LAUNCH_CHECK();
  }
  // ---- the report in front of the UL-SCH (sch.c:1036-1056)
  uint32_t cqi_len = c->cqi_len;
  int      Qp_cqi  = p.Qc[0];
  if (len2 != c->cqi_len) {
    bool rank2 = c->cqi_rank2 != 0;
    if (c->ri_len) { // sch.c:982-986: the rank just decoded sizes the report; the one case in which the call waits for its own first half
      HIP_TRY(hipStreamSynchronize(st));
      waits++;
      rank2 = h_dec[2] > 0;
    }
    if (rank2) cqi_len = len2, Qp_cqi = p.Qc[1];
  }
  if (cqi) {
    hipLaunchKernelGGL(pusch_cqi_decode_kernel, dim3(1), dim3(256), 0, st, (const int16_t*)d_g, 0, Qp_cqi * (int)Qm, (int)cqi_len, h_cqi, h_crc,
                       (const PuschDesc*)nullptr, 1);
    LAUNCH_CHECK();
    if (cqi_len <= 11 && Qp_cqi * (int)Qm > 32) {
      hipLaunchKernelGGL(ulsch_cqi_fold_kernel, dim3(1), dim3(32), 0, st, d_g, Qp_cqi * (int)Qm);
      LAUNCH_CHECK();
    }
  }
  // ---- the transport block behind it
  if (sum_passes) *sum_passes = 0;
  if (c->tbs) {
    const uint32_t G = H - Qp_ri - (uint32_t)Qp_cqi;
    if (int r = sch_decode_run(q, nullptr, G * Qm, (uint32_t)Qp_cqi * Qm, c->tbs, c->mod, 1, c->rv, c->max_iterations, buffer_f, cb_crc, cb_bytes, sum_passes, &waits))
      return r;
  } else {
    HIP_TRY(hipStreamSynchronize(st));
    waits++;
  }
  memset(res, 0, sizeof(*res));
  res->ack[0] = h_dec[0]; res->ack[1] = h_dec[1]; res->ri = h_dec[2];
  memcpy(res->cqi_bits, h_cqi, 64);
  res->cqi_crc = *h_crc; res->cqi_len = cqi ? cqi_len : 0;
  res->Q_prime_ack = Qp_ack; res->Q_prime_ri = Qp_ri; res->Q_prime_cqi = cqi ? (uint32_t)Qp_cqi : 0;
  res->stream_waits = waits;
  return SRSLTE_SUCCESS;
}

// q_bits: cfg->nof_bits descrambled LLRs as pusch.c:499 leaves them; c_seq: the scrambling sequence, one bit per byte (read at the ACK / RI
// positions of a 1-bit ACK / RI only). buffer_f / cb_crc / cb_bytes / sum_passes as srslte_hip_sch_decode takes them (unused with tbs = 0).
extern "C" int srslte_hip_ulsch_decode(srslte_hip_sch_t* q, const int16_t* q_bits, const uint8_t* c_seq, const srslte_hip_ulsch_cfg_t* c, int16_t** buffer_f,
                                       uint8_t* cb_crc, uint8_t* cb_bytes, uint32_t* sum_passes, srslte_hip_ulsch_res_t* res)
{
  if (!q_bits || !c_seq || !res) return SRSLTE_ERROR_INVALID_INPUTS;
  UlschPlan p;
  if (int r = ulsch_plan(q, c, buffer_f, cb_crc, cb_bytes, &p)) return r;
  if (ulsch_init(q)) return SRSLTE_ERROR;
  uint8_t* h_cs = q->h_ul + UL_O_CS;
  // ---- up: the LLRs, and c_seq where a 1-bit ACK / RI reads it (p0 and p1 of every symbol, uci.c:627-640)
  for (int w = 0; w < 2; w++) {
    const uint32_t Qp = w ? p.Qp_ri : p.Qp_ack, O = w ? c->ri_len : c->ack_len;
    uint8_t*       cs = h_cs + (w ? 2 * p.Qp_ack : 0);
    for (uint32_t i = 0; i < Qp; i++) {
      uint32_t row, col;
      pusch_uci_symbol_pos(w != 0, i, p.rows, p.nsymb, &row, &col);
      const uint32_t p0 = (col * p.rows + row) * p.Qm;
      cs[2 * i]     = O == 1 ? c_seq[p0] : 0;
      cs[2 * i + 1] = O == 1 ? c_seq[p0 + 1] : 0;
    }
  }
  memcpy(q->h_pin, q_bits, (size_t)c->nof_bits * 2);
  HIP_TRY(hipMemcpyAsync(q->d_q.get(), q->h_pin, (size_t)c->nof_bits * 2, hipMemcpyHostToDevice, q->st));
  return ulsch_run(q, c, p, h_cs, buffer_f, cb_crc, cb_bytes, sum_passes, res);
}

extern "C" int srslte_hip_ulsch_debug_g(srslte_hip_sch_t* q, int16_t* out, uint32_t n)
{
  if (!q || !out || n > q->g_len) return SRSLTE_ERROR_INVALID_INPUTS;
  HIP_TRY(hipMemcpy(out, q->gs.d_e.get(), (size_t)n * 2, hipMemcpyDeviceToHost));
  return SRSLTE_SUCCESS;
}
