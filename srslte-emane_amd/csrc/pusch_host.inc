// Fragment of pdsch.hip: ONE PUSCH from the subframe's grid and channel estimates in HOST memory, in one device call - what srslte_pusch_decode does
// (pusch.c:427-522) in front of srslte_ulsch_decode: pusch_get of symbols and estimates (:53-91,:462-473), srslte_predecoding_single (:476),
// srslte_dft_precoding (:479), srslte_demod_soft_demodulate_s (:485), the user's sequence and srslte_scrambling_s_offset (:489-499). On the object
// and stream of sch_host.inc: the allocation's rows go up once (2 x nof_re x 8 bytes), the chain leaves the descrambled LLRs in d_q, where
// ulsch_deint_kernel reads them, and ulsch_host.inc's ulsch_run does the rest. Upstream through the drop-in made three visits for this: the
// equalised symbols went down for the transform, up, down for the demapper, up, and the LLRs down again.
namespace {

// One thread per RE of the staged rows: yh = the allocation's received symbols [nof_re], then its channel estimates [nof_re], both in pusch_cp's
// order - the gather was the host's copy into pinned memory, so y, h and z are read and written at consecutive addresses.
// z = y h* / (|h|^2 + n0) (srslte_predecoding_single, precoding.c:277-288, scaling 1), with pusch_eq_kernel's arithmetic.
__global__ __launch_bounds__(256) void pusch_eq_rows_kernel(const cf32* __restrict__ yh, cf32* __restrict__ z, int nof_re, float n0)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nof_re) return;
  const cf32  y = yh[i], h = yh[nof_re + i];
  const float re = y.x * h.x + y.y * h.y, im = y.y * h.x - y.x * h.y, csi = h.x * h.x + h.y * h.y + n0;
  z[i] = make_float2(re * 1.0f / csi, im * 1.0f / csi);
}

// The PUSCH's Gold sequence from the basis of the object's grants state (scr_gen_kernel with c_init by value): `used` packed words of it
__global__ __launch_bounds__(256) void pusch_scr_kernel(const uint32_t* __restrict__ basis, uint32_t* __restrict__ out, int used, int words, uint32_t c_init)
{
  const int w = blockIdx.x * 256 + threadIdx.x;
  if (w >= used) return;
  uint32_t v = basis[w];
  for (int j = 0; j < 31; j++) {
    if ((c_init >> j) & 1u) v ^= basis[(size_t)(1 + j) * words + w];
  }
  out[w] = v;
}

// One thread per RE: demap symbol i of the de-precoded stream, descramble, store its Qm LLRs at q[i Qm ..] - the received order, which the
// de-interleaver reads. Consecutive lanes store consecutive runs of Qm / 2 dwords. cs holds one word more than the sequence needs.
__global__ __launch_bounds__(256) void pusch_demod_rows_kernel(const cf32* __restrict__ d, const uint32_t* __restrict__ cs, int16_t* __restrict__ q, int nof_re,
                                                               int mod, int Qm)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nof_re) return;
  short o[8];
  demod_dev::demod_s(mod, d[i], i, nof_re, o);
  const int      bit0 = i * Qm;
  const uint32_t c2   = (uint32_t)((((uint64_t)cs[(bit0 >> 5) + 1] << 32) | cs[bit0 >> 5]) >> (bit0 & 31));
  uint32_t*      dst  = reinterpret_cast<uint32_t*>(q + (size_t)bit0); // bit0 is even: dword-aligned
  for (int b = 0; b < Qm; b += 2) {
    const short v0 = ((c2 >> b) & 1) ? (short)-o[b] : o[b], v1 = ((c2 >> (b + 1)) & 1) ? (short)-o[b + 1] : o[b + 1];
    dst[b >> 1] = (uint32_t)(uint16_t)v0 | ((uint32_t)(uint16_t)v1 << 16);
  }
}

// The bits of the sequence a 1-bit ACK / RI reads (uci.c:627-640), in ulsch_deint_kernel's layout: thread t < Q'_ack is ACK symbol t, the ones behind
// them the RI symbols; positions as pusch_uci_symbol_pos (uci.c:497-545)
__global__ __launch_bounds__(256) void pusch_cs_kernel(const uint32_t* __restrict__ scr, uint8_t* __restrict__ cs, UlschGeom u)
{
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= u.ack.Qprime + u.ri.Qprime) return;
  const bool is_ri = t >= u.ack.Qprime;
  const int  i = is_ri ? t - u.ack.Qprime : t, O = is_ri ? u.ri.O : u.ack.O, c4 = (3 * i) % 4, row = u.rows - 1 - i / 4;
  int        col;
  if (u.cols > 10) col = is_ri ? 1 + 3 * c4 : (c4 == 0 ? 2 : (c4 == 1 ? 3 : (c4 == 2 ? 8 : 9)));
  else col = is_ri ? (c4 == 0 ? 0 : (c4 == 1 ? 3 : (c4 == 2 ? 5 : 8))) : (c4 == 0 ? 1 : (c4 == 1 ? 2 : (c4 == 2 ? 6 : 7)));
  const int p0 = (col * u.rows + row) * u.Qm; // even: p0 and p0 + 1 share a word
  const uint32_t w = scr[p0 >> 5] >> (p0 & 31);
  cs[2 * t]     = O == 1 ? (w & 1u) : 0;
  cs[2 * t + 1] = O == 1 ? ((w >> 1) & 1u) : 0;
}

// made by the first srslte_hip_pusch_decode: an allocation of nof_re REs carries at least 2 nof_re bits, so max_e / 2 REs bound every call
int pusch_init(srslte_hip_sch* q)
{
  if (q->d_re) return SRSLTE_SUCCESS;
  const size_t max_re = q->max_e / 2 + 1;
  if (q->d_re.alloc(2 * max_re) || q->d_z.alloc(max_re) || q->d_d.alloc(max_re) || q->d_cs.alloc((size_t)q->max_e + 16) || q->h_re.alloc(2 * max_re * sizeof(cf32))) {
    hip_log("[srslte_hip] sch: allocation for the PUSCH call failed\n");
    return SRSLTE_ERROR;
  }
  return SRSLTE_SUCCESS;
}

} // namespace

extern "C" int srslte_hip_pusch_decode(srslte_hip_sch_t* q, const void* sf_symbols, const void* ce, float noise_estimate, const srslte_hip_pusch_cfg_t* pc,
                                       int16_t** buffer_f, uint8_t* cb_crc, uint8_t* cb_bytes, uint32_t* sum_passes, srslte_hip_ulsch_res_t* res)
{
  if (!q || !sf_symbols || !ce || !pc || !res) return SRSLTE_ERROR_INVALID_INPUTS;
  uint32_t  rows[2 * 12];
  const int nrows = srslte_hip_pusch_rows(pc, rows); // the allocation's own refusals; nof_symb <= 12 rows
  if (nrows < 0) return SRSLTE_ERROR_INVALID_INPUTS;
  const srslte_hip_ulsch_cfg_t* c = &pc->sch;
  UlschPlan                     p;
  if (int r = ulsch_plan(q, c, buffer_f, cb_crc, cb_bytes, &p)) return r;
  if (ulsch_init(q) || pusch_init(q)) return SRSLTE_ERROR;
  hipStream_t    st = q->st;
  const uint32_t M_sc = 12 * c->L_prb, nof_re = pc->nof_re, cell_nre = 12 * pc->nof_prb;
  // ---- up: the allocation's rows of both grids, as pusch_cp copies them (pusch.c:62-85)
  cf32* h_y = reinterpret_cast<cf32*>(q->h_re.get());
  for (int n = 0; n < nrows; n++) {
    const size_t o = (size_t)rows[2 * n] * cell_nre + rows[2 * n + 1];
    memcpy(h_y + (size_t)n * M_sc, static_cast<const cf32*>(sf_symbols) + o, sizeof(cf32) * M_sc);
    memcpy(h_y + nof_re + (size_t)n * M_sc, static_cast<const cf32*>(ce) + o, sizeof(cf32) * M_sc);
  }
  HIP_TRY(hipMemcpyAsync(q->d_re.get(), h_y, sizeof(cf32) * 2 * nof_re, hipMemcpyHostToDevice, st));
  // ---- the sequence (srslte_sequence_pusch, sequences.c:65-67), with the spare word the demapper reads behind it
  GrantsState*   g = &q->gs;
  const int      used = (int)((c->nof_bits + 31) / 32 + 1);
  const uint32_t c_init = (pc->rnti << 14) + (pc->sf_idx << 9) + pc->cell_id;
  hipLaunchKernelGGL(pusch_scr_kernel, dim3(ceil_div(used, 256)), dim3(256), 0, st, (const uint32_t*)g->d_basis, g->d_scr.get(), used, (int)g->words, c_init);
  hipLaunchKernelGGL(pusch_eq_rows_kernel, dim3(ceil_div((int)nof_re, 256)), dim3(256), 0, st, (const cf32*)q->d_re, q->d_z.get(), (int)nof_re, noise_estimate);
  LAUNCH_CHECK();
  if (int r = srslte_hip_dft_precoding_batch(q->d_z, q->d_d, c->L_prb, c->nof_symb, 0, st)) return r; // srslte_dft_precoding_init_rx: inverse, 1/sqrt(N)
  hipLaunchKernelGGL(pusch_demod_rows_kernel, dim3(ceil_div((int)nof_re, 256)), dim3(256), 0, st, (const cf32*)q->d_d, (const uint32_t*)g->d_scr, q->d_q.get(), (int)nof_re,
                     c->mod, (int)p.Qm);
  LAUNCH_CHECK();
  q->q_len = c->nof_bits;
  if ((c->ack_len == 1 && p.Qp_ack) || (c->ri_len == 1 && p.Qp_ri)) {
    UlschGeom u;
    u.rows = (int)p.rows; u.cols = (int)p.nsymb; u.Qm = (int)p.Qm;
    u.ack = AckGeom{(int)c->ack_len, (int)p.Qp_ack};
    u.ri  = AckGeom{(int)c->ri_len, (int)p.Qp_ri};
    u.ri_imax = 0;
    hipLaunchKernelGGL(pusch_cs_kernel, dim3(ceil_div((int)(p.Qp_ack + p.Qp_ri), 256)), dim3(256), 0, st, (const uint32_t*)g->d_scr, q->d_cs.get(), u);
    LAUNCH_CHECK();
  }
  return ulsch_run(q, c, p, q->d_cs.get(), buffer_f, cb_crc, cb_bytes, sum_passes, res);
}

extern "C" int srslte_hip_pusch_debug_q(srslte_hip_sch_t* q, int16_t* out, uint32_t n)
{
  if (!q || !out || n > q->q_len) return SRSLTE_ERROR_INVALID_INPUTS;
  HIP_TRY(hipMemcpy(out, q->d_q.get(), (size_t)n * 2, hipMemcpyDeviceToHost));
  return SRSLTE_SUCCESS;
}
