// Fragment of pdsch.hip: ONE transport block with HOST buffers in one device call, transmit side - what encode_tb_off does (sch.c:183-289, with
// w_offset = 0) behind srslte_dlsch_encode2 (sch.c:549-575): TB CRC24A, segmentation, CB CRC24B, turbo encoding, the circular buffer of every
// code block as srslte_rm_turbo_tx_lut leaves it (rm_turbo.c:328-372) and the bit selection of the rv into e_bits, the blocks following each
// other at bit granularity. Upstream enters the library once per code block (srslte_tcod_encode_lut: a copy in, a launch, a copy out and a
// wait each); this entry costs one wait per transport block. The counterpart of sch_host.inc.
// The caller's srslte_softbuffer_tx_t stays the HARQ state, in host memory as upstream: rv 0 writes its circular buffers, a retransmission
// reads them - and nothing else, so a buffer the reference's own encoder wrote serves as well, and the other way round.
// The front of the chain is the fixed-grant transmitters' (SchTxFixed, pusch_tx.inc); new is the rate matching into PACKED bits: those
// pipelines fuse it into the modulation and never materialise w or e.
namespace {

struct SchEncGeom {
  int C, K, L;       // code blocks, block length, 3K + 12 bits of a circular buffer
  int n0;            // entry of the rv 0 rate-matching table that is bit 0 of the circular buffer
  int r;             // bit of the circular buffer the rv's selection begins with
  int w_words;       // 32-bit words between the blocks' circular buffers
  int C_lo, n_lo, n_hi, total; // blocks 0 .. C_lo - 1 carry n_lo bits of e, the rest n_hi (sch.c:204-236); all of them: total
};

// e bit b of a 32-bit word as the host sees its bytes: bit 7 - b % 8 of byte b / 8 (MSB first)
__device__ __forceinline__ uint32_t packed_bit(int b) { return 1u << ((b & ~7) | (7 - (b & 7))); }

// grid = C, 256 threads: the circular buffer of block c without its NULLs, packed MSB first: the interleaved systematic bits from bit 0, the
// interlaced parity bits from bit K + 4 (rm_turbo.c:340-350). The block's three byte streams (under 2.4 KB) are staged in LDS; a thread
// composes whole 32-bit words, each bit through the rate-matching table of rv 0 turned back by its start (lte_rm_tx_start), and stores them
// to the device copy the selection reads and to the pinned host copy the soft buffer is filled from. Bits past 3K + 12 of the last word: 0.
__global__ __launch_bounds__(256) void sch_enc_w_kernel(const uint8_t* __restrict__ cb, int cb_stride, const uint8_t* __restrict__ parity, int par_stride,
                                                        const uint8_t* __restrict__ sys_tail, const uint32_t* __restrict__ rm, uint32_t* __restrict__ w_dev,
                                                        uint32_t* __restrict__ w_host, SchEncGeom g)
{
  __shared__ __attribute__((aligned(16))) uint8_t xs[6144 / 8], ps[(6144 / 4 + 1 + 15) & ~15];
  const int                                       c = blockIdx.x, t = threadIdx.x;
  // the slots are multiples of 16 bytes on 16-byte boundaries (hipMalloc, the strides): whole uint4, at most up to the slot's end
  const uint4 *xg = reinterpret_cast<const uint4*>(cb + (size_t)c * cb_stride), *pg = reinterpret_cast<const uint4*>(parity + (size_t)c * par_stride);
  for (int i = t; i < (g.K / 8 + 15) / 16; i += 256) reinterpret_cast<uint4*>(xs)[i] = xg[i];
  for (int i = t; i < (g.K / 4 + 1 + 15) / 16; i += 256) reinterpret_cast<uint4*>(ps)[i] = pg[i];
  const uint32_t tail = sys_tail[c];
  __syncthreads();
  for (int i = t; i < (g.L + 31) / 32; i += 256) {
    uint32_t v = 0;
    int      n = 32 * i + g.n0;
    n -= n >= g.L ? g.L : 0;
#pragma unroll 8
    for (int b = 0; b < 32; b++) {
      if (32 * i + b < g.L) {
        const uint32_t src = rm[n], pos = src & 0x3fffffffu, s = src >> 30;
        const uint32_t byte = s == 0 ? xs[pos >> 3] : (s == 1 ? tail : ps[pos >> 3]);
        if ((byte >> (7 - (pos & 7))) & 1) v |= packed_bit(b);
      }
      n = n + 1 == g.L ? 0 : n + 1;
    }
    w_dev[(size_t)c * g.w_words + i]  = v;
    w_host[(size_t)c * g.w_words + i] = v;
  }
}

// grid = ceil(ceil(total / 32) / 256), 256 threads: bit selection (36.212 5.1.4.1.2) of all blocks into the packed e. A thread owns one 32-bit
// word of e and fetches each of its bits from the circular buffer of the block the bit belongs to, from the rv's start on and round at 3K + 12:
// the word that straddles a block boundary is composed by one thread. w: the blocks' circular buffers, the device copy sch_enc_w_kernel wrote
// (rv 0) or the pinned host copy of the caller's soft buffer (a retransmission): read a byte at a time, each byte once per run of bits.
// Bits past `total` of the last word: 0.
__global__ __launch_bounds__(256) void sch_enc_select_kernel(const uint8_t* __restrict__ w, uint32_t* __restrict__ e, SchEncGeom g)
{
  const int i = blockIdx.x * 256 + threadIdx.x, g0 = 32 * i;
  if (g0 >= g.total) return;
  int c, n;
  const int lo = g.C_lo * g.n_lo;
  if (g0 < lo) {
    c = g0 / g.n_lo;
    n = g0 - c * g.n_lo;
  } else {
    c = g.C_lo + (g0 - lo) / g.n_hi;
    n = (g0 - lo) % g.n_hi;
  }
  int            pos = (g.r + n) % g.L, at = -1;
  uint32_t       v = 0, byte = 0;
  const uint8_t* wc = w + (size_t)c * g.w_words * 4;
  for (int b = 0; b < 32 && g0 + b < g.total; b++) {
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
  e[i] = v;
}

} // namespace

struct srslte_hip_sch_enc {
  static constexpr uint32_t CB_STRIDE = (6144 / 8 + 15) & ~15u, PAR_STRIDE = (6144 / 4 + 1 + 15) & ~15u, W_WORDS = ((3 * 6144 + 12 + 31) / 32 + 3) & ~3u;
  struct KTab { // per block length: the rate-matching table of rv 0 over the encoder's byte streams and where each rv begins in the circular buffer
    DevBuf<uint32_t> d_rm;
    uint32_t         start[4];
  };
  uint32_t         max_tbs = 0, max_e = 0, Cmax = 0;
  hipStream_t      st = nullptr;
  PinBuf           h_pin; // pinned, read and written by the kernels themselves: transport block | e words | circular buffers [Cmax][W_WORDS]
  size_t           o_e = 0, o_w = 0;
  DevBuf<uint32_t> d_tbcrc, d_w;
  DevBuf<uint8_t>  d_cb, d_parity, d_sys_tail;
  std::map<uint32_t, KTab> tab;
  // srslte_hip_ulsch_encode (ulsch_enc_host.inc), made by its first call. Pinned: the report's bits [64] | the rate-matching order of its coded
  // bits [max_e] uint16 | g words | q words. Device: the coded report, one bit per byte, and the copy of g the channel interleaver reads
  PinBuf           h_ul;
  size_t           o_ul_g = 0, o_ul_q = 0;
  DevBuf<uint8_t>  d_qcqi;
  DevBuf<uint32_t> d_g;
  uint32_t         g_words = 0; // of the last call
  ~srslte_hip_sch_enc()
  {
    if (st) (void)hipStreamSynchronize(st); // a call that returned early may have left launches queued: they end before the buffers go
    if (st) (void)hipStreamDestroy(st);
  }
  const KTab* table(uint32_t K) // null: the upload failed
  {
    auto it = tab.find(K);
    if (it == tab.end()) {
      KTab t;
      if (rm_tx_table_upload(K, 0, t.d_rm)) return nullptr;
      for (uint32_t rv = 0; rv < 4; rv++) t.start[rv] = lte_rm_tx_start(K, rv);
      it = tab.emplace(K, std::move(t)).first;
    }
    return &it->second;
  }
};

extern "C" void srslte_hip_sch_enc_destroy(srslte_hip_sch_enc_t* q) { delete q; }

extern "C" srslte_hip_sch_enc_t* srslte_hip_sch_enc_create(uint32_t max_tbs, uint32_t max_e_bits)
{
  srslte_hip_cbsegm_t seg;
  if (max_tbs == 0 || max_tbs > (uint32_t)TB_MAX_BITS || max_e_bits == 0 || max_e_bits > (1u << 30) || srslte_hip_cbsegm(&seg, max_tbs)) {
    hip_log("[srslte_hip] sch_enc: invalid max_tbs=%u / max_e_bits=%u\n", max_tbs, max_e_bits);
    return nullptr;
  }
  std::unique_ptr<srslte_hip_sch_enc> q(new srslte_hip_sch_enc());
  q->max_tbs = max_tbs; q->max_e = max_e_bits; q->Cmax = seg.C;
  q->o_e = ((size_t)max_tbs / 8 + 63) & ~(size_t)63;
  q->o_w = q->o_e + ((((size_t)max_e_bits + 31) / 32 * 4 + 63) & ~(size_t)63);
  const size_t C = q->Cmax;
  const bool   ok = hipStreamCreateWithFlags(&q->st, hipStreamNonBlocking) == hipSuccess && !q->h_pin.alloc(q->o_w + C * q->W_WORDS * 4) && !q->d_tbcrc.alloc(1) &&
                  !q->d_w.alloc(C * q->W_WORDS) && !q->d_cb.alloc(C * q->CB_STRIDE) && !q->d_parity.alloc(C * q->PAR_STRIDE) && !q->d_sys_tail.alloc(C);
  if (!ok) {
    hip_log("[srslte_hip] sch_enc: initialisation failed\n");
    return nullptr;
  }
  return q.release();
}

// The steps srslte_hip_sch_encode and srslte_hip_ulsch_encode (ulsch_enc_host.inc) share.
// 1. The checks on a transport block of tbs > 0 bits and its buffers, with upstream's codes; seg: its segmentation.
static int sch_enc_check(const uint8_t* data, uint32_t tbs, uint32_t rv, uint8_t** buffer_b, srslte_hip_cbsegm_t* seg)
{
  if (!buffer_b || (!data && rv == 0)) return SRSLTE_ERROR_INVALID_INPUTS; // upstream would rate-match what its scratch buffers held
  if (srslte_hip_cbsegm(seg, tbs)) return SRSLTE_ERROR;
  if (seg->F) {
    hip_log("Error filler bits are not supported. Use standard TBS\n"); // sch.c:194-197
    return SRSLTE_ERROR;
  }
  if (seg->C2) {
    hip_log("[srslte_hip] sch_enc: TBS %u needs two code-block sizes; not supported on device yet\n", tbs);
    return SRSLTE_ERROR_INVALID_INPUTS;
  }
  for (uint32_t c = 0; c < seg->C; c++) {
    if (!buffer_b[c]) return SRSLTE_ERROR_INVALID_INPUTS;
  }
  return SRSLTE_SUCCESS;
}

// 2. The geometry of C blocks of K bits whose selection of the rv fills QN Gp bits (QN = Qm Nl)
static SchEncGeom sch_enc_geom(const srslte_hip_sch_enc* q, const srslte_hip_sch_enc::KTab* kt, uint32_t C, uint32_t K, uint32_t QN, uint32_t Gp, uint32_t rv)
{
  const uint32_t gamma = Gp % C;
  SchEncGeom     g;
  g.C = (int)C; g.K = (int)K; g.L = (int)(3 * K + 12);
  g.n0 = (int)((g.L - kt->start[0]) % g.L);
  g.r = (int)kt->start[rv];
  g.w_words = (int)q->W_WORDS;
  g.C_lo = (int)(C - gamma); g.n_lo = (int)(QN * (Gp / C)); g.n_hi = g.n_lo + (int)QN; // sch.c:232-236
  g.total = (int)(QN * Gp);
  return g;
}

// 3. Queues what leaves the circular buffers where the selection reads them (*w_src): for rv 0 the chain from the transport block to
// sch_enc_w_kernel, which also fills the pinned copy; for a retransmission the caller's buffers are staged in that pinned copy
static int sch_enc_queue_w(srslte_hip_sch_enc* q, const srslte_hip_sch_enc::KTab* kt, const uint8_t* data, uint32_t tbs, uint32_t rv, uint8_t** buffer_b,
                           const SchEncGeom& g, const uint8_t** w_src)
{
  const size_t   w_bytes = ((size_t)g.L + 7) / 8, w_stride = (size_t)q->W_WORDS * 4;
  const uint32_t C = (uint32_t)g.C, K = (uint32_t)g.K;
  uint8_t *      h_tb = q->h_pin, *h_w = q->h_pin + q->o_w;
  hipStream_t    st   = q->st;
  *w_src = h_w;
  if (rv != 0) {
    for (uint32_t c = 0; c < C; c++) memcpy(h_w + c * w_stride, buffer_b[c], w_bytes);
    return SRSLTE_SUCCESS;
  }
  memcpy(h_tb, data, tbs / 8);
  PuschTxGeom cg = {};
  cg.C = (int)C; cg.K = (int)K; cg.tbs = (int)tbs; cg.rlenB = (int)((C <= 1 ? K : K - 24) / 8); cg.cb_stride = (int)q->CB_STRIDE;
  cg.par_stride = (int)q->PAR_STRIDE; cg.tb_stride = 0;
  hipLaunchKernelGGL(pusch_tx_tbcrc_kernel, dim3(1), dim3(256), 0, st, (const uint8_t*)h_tb, q->d_tbcrc.get(), cg);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(pusch_tx_seg_kernel, dim3(C, 1), dim3(256), 0, st, (const uint8_t*)h_tb, (const uint32_t*)q->d_tbcrc, q->d_cb.get(), cg);
  LAUNCH_CHECK();
  if (int r = srslte_hip_tcod_encode_bytes_batch(q->d_cb, q->CB_STRIDE, q->d_parity, q->PAR_STRIDE, q->d_sys_tail, K, C, st)) return r;
  hipLaunchKernelGGL(sch_enc_w_kernel, dim3(C), dim3(256), 0, st, (const uint8_t*)q->d_cb, (int)q->CB_STRIDE, (const uint8_t*)q->d_parity, (int)q->PAR_STRIDE,
                     (const uint8_t*)q->d_sys_tail, (const uint32_t*)kt->d_rm, q->d_w.get(), reinterpret_cast<uint32_t*>(h_w), g);
  LAUNCH_CHECK();
  *w_src = reinterpret_cast<const uint8_t*>(q->d_w.get());
  return SRSLTE_SUCCESS;
}

// 4. After the stream wait: nbits packed bits from src; the bits of the last byte past them keep the caller's values ...
static void sch_enc_copy_bits(uint8_t* dst, const uint8_t* src, size_t nbits)
{
  memcpy(dst, src, nbits / 8);
  if (nbits % 8) {
    const uint8_t m = (uint8_t)(0xff00u >> (nbits % 8));
    dst[nbits / 8] = (uint8_t)((src[nbits / 8] & m) | (dst[nbits / 8] & ~m));
  }
}
// ... and for rv 0 the circular buffers into the caller's soft buffer
static void sch_enc_copy_w(const srslte_hip_sch_enc* q, const SchEncGeom& g, uint8_t** buffer_b)
{
  const uint8_t* h_w = q->h_pin + q->o_w;
  for (int c = 0; c < g.C; c++) memcpy(buffer_b[c], h_w + (size_t)c * q->W_WORDS * 4, ((size_t)g.L + 7) / 8);
}

// data: tbs / 8 bytes of the transport block, or null for a retransmission. mod: 1 QPSK .. 4 256QAM; Nl as srslte_dlsch_encode2 derives it (2
// where nof_layers != nof_tb). buffer_b[c]: the srslte_softbuffer_tx_t's circular buffers of the C code blocks, ceil((3K + 12) / 8) bytes each:
// written for rv 0, read for rv 1-3 (whose result depends on them alone: data is not looked at, as upstream encodes it and then selects from
// the buffer all the same). e_bits: Qm Nl floor(nof_e_bits / (Qm Nl)) bits from bit 0, MSB first; the bits of the last byte past them keep the
// caller's values. Everything is checked before anything is queued or written.
extern "C" int srslte_hip_sch_encode(srslte_hip_sch_enc_t* q, const uint8_t* data, uint32_t tbs, int mod, uint32_t Nl, uint32_t rv, uint32_t nof_e_bits,
                                     uint8_t** buffer_b, uint8_t* e_bits)
{
  if (!q || !e_bits || rv > 3 || mod < 1 || mod > 4 || Nl < 1 || Nl > 2 || (tbs % 8) || tbs > q->max_tbs || nof_e_bits == 0 || nof_e_bits > q->max_e)
    return SRSLTE_ERROR_INVALID_INPUTS;
  if (tbs == 0) return SRSLTE_SUCCESS; // upstream's loop over C = 0 code blocks
  srslte_hip_cbsegm_t seg;
  if (int r = sch_enc_check(data, tbs, rv, buffer_b, &seg)) return r;
  const srslte_hip_sch_enc::KTab* kt = q->table(seg.K1);
  if (!kt) return SRSLTE_ERROR;
  const uint32_t   QN = 2 * (uint32_t)mod * Nl;
  const SchEncGeom g  = sch_enc_geom(q, kt, seg.C, seg.K1, QN, nof_e_bits / QN, rv);
  uint32_t*        h_e = reinterpret_cast<uint32_t*>(q->h_pin + q->o_e);
  const uint8_t*   w_src;
  if (int r = sch_enc_queue_w(q, kt, data, tbs, rv, buffer_b, g, &w_src)) return r;
  if (g.total) {
    hipLaunchKernelGGL(sch_enc_select_kernel, dim3(ceil_div(ceil_div(g.total, 32), 256)), dim3(256), 0, q->st, w_src, h_e, g);
    LAUNCH_CHECK();
  }
  HIP_TRY(hipStreamSynchronize(q->st));
  sch_enc_copy_bits(e_bits, reinterpret_cast<const uint8_t*>(h_e), (size_t)g.total);
  if (rv == 0) sch_enc_copy_w(q, g, buffer_b);
  return SRSLTE_SUCCESS;
}
