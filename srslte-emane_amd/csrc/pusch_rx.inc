// Fragment of pdsch.hip (same translation unit): the PUSCH receive pipeline (eNB side), fixed-grant and per-PUSCH grants.
// ====================================================================================================================
// PUSCH receive pipeline (eNB side, SURVEY §8f N3): OFDM RX with the -1/2 carrier shift (enb_ul.c:58-63) -> chest_ul ->
// RE extraction + one-tap MMSE (pusch.c:461-475) -> inverse transform precoding (:477-478) -> soft demap + descramble + UL
// channel de-interleaver (:480-503, sch.c:891-913) -> rate de-matching -> turbo decode -> TB CRC (decode_tb, sch.c:429-500).
// UL-SCH data only (no UCI multiplexing), same allocation in both slots, normal CP, not shortened, rv 0.
// ====================================================================================================================
namespace {

// HARQ-ACK on the PUSCH (36.212 5.2.2.6-5.2.2.8; srslte_uci_encode_ack_ri / _decode_ack_ri, uci.c:497-520,:547-602,:627-656,:695-788; 1 or 2 bits,
// no RI / CQI): ACK symbol i sits on data symbol {2,3,8,9}[(3i)%4] ({1,2,6,7} with at most 10 data symbols), sub-carrier M_sc-1-i/4.
struct AckGeom {
  int O, Qprime; // 0: no ACK
};
__device__ __forceinline__ int ack_symbol_index(const AckGeom& a, int n, int k, int M_sc, int nsymb)
{ // index i of the ACK symbol at data symbol n, sub-carrier k, or -1
  int colidx;
  if (nsymb > 10) {
    colidx = n == 2 ? 0 : (n == 3 ? 1 : (n == 8 ? 2 : (n == 9 ? 3 : -1)));
  } else {
    colidx = n == 1 ? 0 : (n == 2 ? 1 : (n == 6 ? 2 : (n == 7 ? 3 : -1)));
  }
  if (a.O == 0 || colidx < 0) return -1;
  const int i = 4 * (M_sc - 1 - k) + (3 * colidx) % 4; // (3 i) % 4 == colidx <=> i % 4 == (3 colidx) % 4
  return i < a.Qprime ? i : -1;
}
// rank indication: the same rule on the columns {1,4,7,10} ({0,3,5,8} with at most 10 symbols; uci.c:521-545)
__device__ __forceinline__ int ri_symbol_index(const AckGeom& a, int n, int k, int M_sc, int nsymb)
{
  int colidx;
  if (nsymb > 10) {
    colidx = n == 1 ? 0 : (n == 4 ? 1 : (n == 7 ? 2 : (n == 10 ? 3 : -1)));
  } else {
    colidx = n == 0 ? 0 : (n == 3 ? 1 : (n == 5 ? 2 : (n == 8 ? 3 : -1)));
  }
  if (a.O == 0 || colidx < 0) return -1;
  const int i = 4 * (M_sc - 1 - k) + (3 * colidx) % 4;
  return i < a.Qprime ? i : -1;
}
// number of RI symbols before (k, n) in the row-by-row order the channel interleaver fills (ulsch_interleave_gen, sch.c:580-598):
// the UL-SCH symbol at (k, n) is symbol k nsymb + n - ri_before of the rate-matched stream
__device__ __forceinline__ int ri_before(const AckGeom& a, int n, int k, int M_sc, int nsymb)
{
  if (a.O == 0) return 0;
  int cnt = max(0, a.Qprime - 4 * (M_sc - k)); // rows above k in the matrix are sub-carriers below it: RI symbols i >= 4 (M_sc - k)
  const int i0 = 4 * (M_sc - 1 - k);
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int c   = (3 * j) % 4;
    const int col = nsymb > 10 ? 1 + 3 * c : (c == 0 ? 0 : (c == 1 ? 3 : (c == 2 ? 5 : 8)));
    cnt += (i0 + j < a.Qprime && col < n) ? 1 : 0;
  }
  return cnt;
}
__device__ __forceinline__ int ack_bit_type(const uint8_t* ack, int O, int Qm, int e)
{ // encode_ri_ack (uci.c:573-602) repeated: 0 / 1 value, 2 repetition of the previous bit, 3 placeholder
  if (O == 1) {
    const int r = e % Qm;
    return r == 0 ? ack[0] : (r == 1 ? 2 : 3);
  }
  const int r = e % (3 * Qm), s3 = r / Qm, b = r % Qm;
  if (b >= 2) return 3;
  const int v = (2 * s3 + b) % 3; // o0 o1 | o2 o0 | o1 o2
  return v == 0 ? ack[0] : (v == 1 ? ack[1] : (ack[0] ^ ack[1]));
}

struct PuschGeom {
  int cell_nre, M_sc, n_prb, n_prb1, mod, Qm, tti0, scr_words, mmse; // n_prb / n_prb1: PRB offset of slot 0 / slot 1 (grant.n_prb_tilde[2])
  AckGeom ack, ri;
  int*    ack_sum; // [nof_sf][4] accumulators of the ACK decisions (zeroed per call), or null
  int*    ri_sum;  // the same for the rank indication
  int nsymb; // data symbols per subframe: 12, or 11 when the last symbol is left to the SRS (shortened subframe, pusch.c:52-91); 10 / 9 with the extended CP
  int nsl;   // symbols per slot: 7, or 6 with the extended CP (DMRS in symbol nsl - 4 of each slot, pusch.c:57-60)
};

// data symbol n -> symbol of the subframe: the DMRS symbols nsl - 4 and 2 nsl - 4 are skipped (l = 3, 10; extended CP: 2, 8)
__device__ __forceinline__ int pusch_data_symbol(int n, int nsl) { return n < nsl - 4 ? n : (n < 2 * nsl - 5 ? n + 1 : n + 2); }

// grid = (ceil(M_sc/256), 12, nof_sf): z[sf][n][k] = y h* / (|h|^2 + noise) on the granted PRBs of data symbol n
__global__ __launch_bounds__(256) void pusch_eq_kernel(const cf32* __restrict__ grid, const cf32* __restrict__ ce,
                                                       const float* __restrict__ noise /* stride 5 floats */, cf32* __restrict__ z, PuschGeom g)
{
  const int k = blockIdx.x * blockDim.x + threadIdx.x, n = blockIdx.y, sf = blockIdx.z;
  if (k >= g.M_sc) return;
  const int    l  = pusch_data_symbol(n, g.nsl);
  const size_t o  = ((size_t)sf * 2 * g.nsl + l) * g.cell_nre + (l < g.nsl ? g.n_prb : g.n_prb1) * 12 + k;
  const cf32   y = grid[o], h = ce[o];
  const float  n0 = g.mmse ? noise[sf * 5] : 0.f;
  const float  re = y.x * h.x + y.y * h.y, im = y.y * h.x - y.x * h.y, csi = h.x * h.x + h.y * h.y + n0; // precoding.c:277-288, scaling 1
  z[((size_t)sf * g.nsymb + n) * g.M_sc + k] = make_float2(re * 1.0f / csi, im * 1.0f / csi);
}

// grid = (ceil(M_sc/64), nof_sf), 256 threads: demap the 12 symbols of 64 sub-carriers, descramble in the received (symbol-major)
// bit order and store at the de-interleaved position g[(k * 12 + n) * Qm + b] = q[(n * M_sc + k) * Qm + b] (36.212 5.2.2.8 without
// UCI). The 64 x 12 x Qm LLRs of a workgroup are contiguous in g: they are collected in LDS and leave with 16-byte stores
// (a 2-byte store per lane at a 24 Qm byte stride costs the L1 one cache line per lane).
// d: the PUSCH's de-precoded symbols [nsymb][M_sc]; cs: its scrambling bits; gout: its LLR row; sf: its row of the UCI accumulators
__device__ __forceinline__ void pusch_demod_body(const cf32* __restrict__ d, const uint32_t* __restrict__ cs, int16_t* __restrict__ gout, const PuschGeom& g,
                                                 int sf, int k0, int16_t* stage)
{
  const int nsym = g.nsymb * g.M_sc;
  const int nk = min(64, g.M_sc - k0);
  const int rb0 = ri_before(g.ri, 0, k0, g.M_sc, g.nsymb); // RI symbols on the sub-carriers before this workgroup's
  for (int t = threadIdx.x; t < 64 * g.nsymb; t += 256) {
    const int n = t >> 6, kl = t & 63;
    if (kl >= nk) continue;
    const int i = n * g.M_sc + k0 + kl;
    short     o[8];
    demod_dev::demod_s(g.mod, d[i], i, nsym, o);
    const int      bit0 = i * g.Qm;
    const uint32_t c2   = (uint32_t)((((uint64_t)cs[(bit0 >> 5) + 1] << 32) | cs[bit0 >> 5]) >> (bit0 & 31));
    const int      ai   = ack_symbol_index(g.ack, n, k0 + kl, g.M_sc, g.nsymb);
    const int      ri   = ri_symbol_index(g.ri, n, k0 + kl, g.M_sc, g.nsymb);
    if (ri >= 0) { // the interleaver left this symbol out of the UL-SCH stream (sch.c:968-979): it only feeds the RI decision
      const int d0 = (c2 & 1) ? -o[0] : o[0], d1 = (c2 & 2) ? -o[1] : o[1];
      if (g.ri.O == 1) {
        atomicAdd(&g.ri_sum[sf * 4], d0 + ((c2 & 1) ? -o[1] : o[1]));
      } else if (3 * (ri / 3) + 3 < g.ri.Qprime) {
        const int s3 = ri % 3;
        atomicAdd(&g.ri_sum[sf * 4 + (s3 == 0 ? 0 : (s3 == 1 ? 2 : 1))], d0);
        atomicAdd(&g.ri_sum[sf * 4 + (s3 == 0 ? 1 : (s3 == 1 ? 0 : 2))], d1);
      }
      continue;
    }
    const int sl = kl * g.nsymb + n - (ri_before(g.ri, n, k0 + kl, g.M_sc, g.nsymb) - rb0); // symbol slot in this workgroup's stage
    if (ai >= 0) { // uci_decode_ri_ack (sch.c:929-966): this symbol feeds the ACK decision and reaches the decoder as zeros
      const int d0 = (c2 & 1) ? -o[0] : o[0], d1 = (c2 & 2) ? -o[1] : o[1]; // descrambled
      if (g.ack.O == 1) { // value bit + its repetition, which carries the value bit's scrambling (uci.c:627-640)
        atomicAdd(&g.ack_sum[sf * 4], d0 + ((c2 & 1) ? -o[1] : o[1]));
      } else if (3 * (ai / 3) + 3 < g.ack.Qprime) { // a triplet is only used if another symbol follows it (uci.c:776-777)
        const int s3 = ai % 3; // o0 o1 | o2 o0 | o1 o2
        atomicAdd(&g.ack_sum[sf * 4 + (s3 == 0 ? 0 : (s3 == 1 ? 2 : 1))], d0);
        atomicAdd(&g.ack_sum[sf * 4 + (s3 == 0 ? 1 : (s3 == 1 ? 0 : 2))], d1);
      }
      for (int b = 0; b < g.Qm; b++) stage[sl * g.Qm + b] = 0;
      continue;
    }
    for (int b = 0; b < g.Qm; b++) stage[sl * g.Qm + b] = ((c2 >> b) & 1) ? (short)-o[b] : o[b];
  }
  __syncthreads();
  if (g.ri.O && k0 == 0 && threadIdx.x == 0) {
    // ulsch_deinterleave scatters g[lut[i]] = q[i] in ascending i with lut = 0 at the RI positions (sch.c:589-591,:910): g[0] ends up
    // with the LLR of the LAST RI bit position: last bit of RI symbol 1 (symbol 0 if it is the only one), on the bottom sub-carrier; the
    // 1-bit decoder has re-scrambled its repetition bit by then (uci.c:632-633)
    const int n = g.ri.Qprime >= 2 ? (g.nsymb > 10 ? 10 : 8) : (g.nsymb > 10 ? 1 : 0), i = n * g.M_sc + g.M_sc - 1, bit = i * g.Qm + g.Qm - 1;
    short     o[8];
    demod_dev::demod_s(g.mod, d[i], i, nsym, o);
    const int cbit = (cs[bit >> 5] >> (bit & 31)) & 1;
    stage[0]       = (g.ri.O == 1 && g.Qm == 2) ? o[1] : (cbit ? (short)-o[g.Qm - 1] : o[g.Qm - 1]);
    __threadfence_block();
  }
  if (g.ri.O && k0 == 0) __syncthreads();
  const int    nsl    = nk * g.nsymb - (ri_before(g.ri, 0, k0 + nk, g.M_sc, g.nsymb) - rb0); // UL-SCH symbols of this workgroup
  const size_t first  = (size_t)(k0 * g.nsymb - rb0) * g.Qm;
  if (g.ri.O == 0 || (rb0 == 0 && nsl == nk * g.nsymb)) {
    const int    nbytes = nk * g.nsymb * g.Qm * 2; // nk is a multiple of 4, Qm even: a multiple of 16
    char*        dst    = reinterpret_cast<char*>(gout + first);
    const char*  src    = reinterpret_cast<const char*>(stage);
    for (int o16 = threadIdx.x * 16; o16 < nbytes; o16 += 256 * 16) *reinterpret_cast<uint4*>(dst + o16) = *reinterpret_cast<const uint4*>(src + o16);
  } else { // the few workgroups that hold RI symbols: neither the length nor the start is 16-byte granular any more
    for (int e = threadIdx.x; e < nsl * g.Qm; e += 256) gout[first + e] = stage[e];
  }
}


__global__ __launch_bounds__(256) void pusch_demod_kernel(const cf32* __restrict__ d, const uint32_t* __restrict__ scr, int16_t* __restrict__ gout,
                                                          PuschGeom g)
{
  __shared__ __attribute__((aligned(16))) int16_t stage[64 * 12 * 8];
  const int sf = blockIdx.y, sf_idx = (g.tti0 + sf) % 10, nsym = g.nsymb * g.M_sc;
  pusch_demod_body(d + (size_t)sf * nsym, scr + (size_t)sf_idx * g.scr_words /* one spare word behind every sequence */, gout + (size_t)sf * nsym * g.Qm, g, sf,
                   blockIdx.x * 64, stage);
}

// Per-PUSCH grants (srslte_hip_ul_rx_batch_grants): PUSCH p of a call has its own allocation, modulation and sequence; its symbols sit at zoff in
// the z / d buffers (PUSCHs of one L_prb next to each other, for the batched transform de-precoding), its LLRs in row p.
struct PuschDesc {
  int sf;                        // subframe of the batch whose grid it is in
  int M_sc, n_prb, n_prb1, mod, Qm;
  int zoff;                      // in cf32
  AckGeom ack, ri;
  int cqi_Q, cqi_O;              // LLRs and bits of its CQI report (0: none)
};

// grid = (ceil(max M_sc / 256), nsymb, nof_pusch)
__global__ __launch_bounds__(256) void pusch_eq_grants_kernel(const cf32* __restrict__ grid, const cf32* __restrict__ ce,
                                                              const float* __restrict__ noise /* stride 5 floats */, cf32* __restrict__ z,
                                                              const PuschDesc* __restrict__ desc, int cell_nre, int nsymb, int mmse, int nsl)
{
  const PuschDesc& pd = desc[blockIdx.z];
  const int        k = blockIdx.x * blockDim.x + threadIdx.x, n = blockIdx.y, M_sc = pd.M_sc;
  if (k >= M_sc) return;
  const int    l  = pusch_data_symbol(n, nsl);
  const size_t o  = ((size_t)pd.sf * 2 * nsl + l) * cell_nre + (l < nsl ? pd.n_prb : pd.n_prb1) * 12 + k;
  const cf32   y = grid[o], h = ce[o];
  const float  n0 = mmse ? noise[blockIdx.z * 5] : 0.f;
  const float  re = y.x * h.x + y.y * h.y, im = y.y * h.x - y.x * h.y, csi = h.x * h.x + h.y * h.y + n0; // precoding.c:277-288, scaling 1
  z[(size_t)pd.zoff + (size_t)n * M_sc + k] = make_float2(re * 1.0f / csi, im * 1.0f / csi);
}

// grid = (ceil(max M_sc / 64), nof_pusch)
__global__ __launch_bounds__(256) void pusch_demod_grants_kernel(const cf32* __restrict__ d, const uint32_t* __restrict__ scr, int scr_words,
                                                                 int16_t* __restrict__ gout, int max_bits, const PuschDesc* __restrict__ desc, int nsymb,
                                                                 int* __restrict__ ack_sum, int* __restrict__ ri_sum)
{
  __shared__ __attribute__((aligned(16))) int16_t stage[64 * 12 * 8];
  const int p = blockIdx.y, k0 = blockIdx.x * 64;
  if (k0 >= desc[p].M_sc) return;
  PuschGeom g; // a local, not the kernel argument: filled from the descriptor
  g.cell_nre = 0; g.M_sc = desc[p].M_sc; g.n_prb = desc[p].n_prb; g.n_prb1 = desc[p].n_prb1; g.mod = desc[p].mod; g.Qm = desc[p].Qm; g.tti0 = 0;
  g.scr_words = scr_words; g.mmse = 0; g.ack = desc[p].ack; g.ri = desc[p].ri; g.ack_sum = ack_sum; g.ri_sum = ri_sum; g.nsymb = nsymb;
  pusch_demod_body(d + desc[p].zoff, scr + (size_t)p * scr_words, gout + (size_t)p * max_bits, g, p, k0, stage);
}

} // namespace

namespace {
// ---- CQI / PMI report on the PUSCH (36.212 5.2.2.6, 5.2.2.6.4; srslte_uci_decode_cqi_pusch, uci.c:423-467): the first Q = Q' Qm LLRs of the
// de-interleaved stream. Up to 11 bits: (32, O) block code - the repetitions are added up with wrapping int16 (srslte_vec_sum_sss) and the
// sum is correlated with all 2^O code words, the first word of the highest correlation wins (decode_cqi_short :305-341). Above 11 bits:
// srslte_rm_conv_rx_s (rm_conv.c:160-219, sequential because of its 10000 = "no value yet" sentinel), then the tail-biting K = 7 rate-1/3
// Viterbi decoder of viterbi37_avx2_16bit.c on three repetitions of the frame - one lane per state, predecessors by shuffle, decisions by
// ballot - with the soft bits scaled as srslte_viterbi_decode_f scales them (the reference's int16 wrapper overflows, see oracle/orc_cqi.c),
// and the CRC-8. One workgroup per subframe; the Viterbi runs on its first wavefront.
__constant__ uint16_t CQI_M32[32] = {0x403, 0x607, 0x749, 0x50D, 0x48F, 0x5D3, 0x755, 0x599, 0x69B, 0x65D, 0x6E5, 0x567, 0x7A9, 0x6AB, 0x4B1, 0x6F3,
                                     0x277, 0x139, 0x0FB, 0x061, 0x445, 0x60B, 0x591, 0x717, 0x3DF, 0x4E3, 0x32D, 0x3AF, 0x175, 0x1FD, 0x7FF, 0x001}; // Table 5.2.2.6.4-1
__constant__ uint8_t  CQI_PERM[32]     = {1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31, 0, 16, 8, 24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30};
__constant__ uint8_t  CQI_PERM_INV[32] = {16, 0, 24, 8, 20, 4, 28, 12, 18, 2, 26, 10, 22, 6, 30, 14, 17, 1, 25, 9, 21, 5, 29, 13, 19, 3, 27, 11, 23, 7, 31, 15};
__device__ __forceinline__ uint32_t cqi_crc8(const uint8_t* bits, int n)
{
  uint32_t r = 0;
  for (int i = 0; i < n + 8; i++) {
    r = (r << 1) | (i < n ? (bits[i] & 1u) : 0u);
    if (r & 0x100u) r ^= 0x19Bu;
  }
  return r & 0xffu;
}

__global__ __launch_bounds__(256) void pusch_cqi_decode_kernel(const int16_t* __restrict__ gl, int g_stride, int Q_all, int O_all, uint8_t* __restrict__ cqi_out,
                                                               uint8_t* __restrict__ ok_out, const PuschDesc* __restrict__ desc, int as_host = 0)
{
  // as_host (srslte_hip_ulsch_decode): the two places where the reference's int16 arithmetic shows once a report is repeated until its sums
  // are large - the block code's correlation in 16 int16 lanes (srslte_vec_dot_prod_sss_simd, vector_simd.c:62-98) and the Viterbi decoder's
  // int16 quantiser (viterbi_dev::quant_sus). Without it: int32 correlation and the float quantiser, as before
  // per-PUSCH grants: the report's size comes from the row's descriptor (rows without a report are left alone)
  const int Q = desc ? desc[blockIdx.x].cqi_Q : Q_all, O = desc ? desc[blockIdx.x].cqi_O : O_all;
  if (O == 0) return;
  __shared__ int16_t            acc[32];
  __shared__ long long          best[4];
  __shared__ int16_t            tmp[3 * 96], dem[3 * 72];
  __shared__ uint16_t           us[3 * 72];
  __shared__ unsigned long long dec[3 * 72 + 6];
  __shared__ uint8_t            bits[3 * 72];
  const int      sf = blockIdx.x, tid = threadIdx.x;
  const int16_t* q  = gl + (size_t)sf * g_stride;
  uint8_t*       out = cqi_out + (size_t)sf * 64;
  if (O <= 11) {
    if (tid < 32) {
      int a = 0;
      for (int i = tid; i < Q; i += 32) a += q[i];
      acc[tid] = (int16_t)a; // wrapping, like the int16 adds of srslte_vec_sum_sss
    }
    __syncthreads();
    const int n = Q < 32 ? Q : 32;
    long long key = INT64_MIN;
    for (uint32_t w = tid; w < (1u << O); w += 256) {
      int  corr = 0;
      auto term = [&](int i) {
        uint32_t m = 0; // code bit i of word w: bit k of the report is bit O-1-k of w
        for (int k = 0; k < O; k++) m ^= ((w >> (O - 1 - k)) & 1u) & ((CQI_M32[i] >> k) & 1u);
        return m ? (int)acc[i] : -(int)acc[i];
      };
      const int nv = as_host ? (n & ~15) : 0; // whole 16-lane vectors: products and sums wrap per int16 lane
      for (int k = 0; k < 16 && nv; k++) {
        int lane = 0;
        for (int i = k; i < nv; i += 16) lane += term(i);
        corr += (int16_t)lane;
      }
      for (int i = nv; i < n; i++) corr += term(i);
      const long long kk = ((long long)corr << 32) | (long long)(0xffffffffu - w); // highest correlation, then lowest word
      key = kk > key ? kk : key;
    }
    for (int o = 32; o > 0; o >>= 1) {
      const long long other = __shfl_xor(key, o, 64);
      key = other > key ? other : key;
    }
    if ((tid & 63) == 0) best[tid >> 6] = key;
    __syncthreads();
    if (tid == 0) {
      for (int i = 1; i < 4; i++) key = best[i] > key ? best[i] : key;
      const uint32_t w = 0xffffffffu - (uint32_t)(key & 0xffffffffll);
      for (int k = 0; k < O; k++) out[k] = (w >> (O - 1 - k)) & 1u;
      ok_out[sf] = 1;
    }
    return;
  }
  const int F = O + 8, nrows = (F - 1) / 32 + 1, K_p = nrows * 32, ndummy = K_p - F;
  for (int i = tid; i < 3 * K_p; i += 256) tmp[i] = 10000; // SRSLTE_RX_NULL
  for (int i = tid; i < 3 * F + 6; i += 256) dec[i] = 0ull;
  __syncthreads();
  if (tid == 0) {
    int k = 0, j = 0;
    while (k < Q) {
      const int d_i = (j % K_p) / nrows, d_j = (j % K_p) % nrows;
      if (d_j * 32 + CQI_PERM[d_i] >= ndummy) {
        const int16_t v = q[k];
        if (tmp[j] == 10000) {
          tmp[j] = v;
        } else if (v != 10000) {
          tmp[j] = (int16_t)(tmp[j] + v);
        }
        k++;
      }
      if (++j == 3 * K_p) j = 0;
    }
  }
  __syncthreads();
  for (int e = tid; e < 3 * F; e += 256) {
    const int     i = e / 3, s = e - 3 * i, d_i = (i + ndummy) / 32, d_j = (i + ndummy) % 32;
    const int16_t o = tmp[K_p * s + CQI_PERM_INV[d_j] * nrows + d_i];
    dem[e]          = o != 10000 ? o : (int16_t)0;
  }
  __syncthreads();
  if (tid >= 64) return;
  if (as_host) viterbi_dev::quant_sus(dem, us, 3 * F, tid);
  else viterbi_dev::quant_fus(dem, us, 3 * F, tid);
  viterbi_dev::decode37_tb(us, dec, bits, F, tid);
  if (tid == 0) {
    const uint8_t* msg = bits + F; // the middle repetition
    uint32_t       rx  = 0;
    for (int i = 0; i < 8; i++) rx = (rx << 1) | msg[O + i];
    const bool good = cqi_crc8(msg, O) == rx;
    if (good) {
      for (int k = 0; k < O; k++) out[k] = msg[k];
    }
    ok_out[sf] = good ? 1 : 0;
  }
}
} // namespace

// The UCI plan (pusch_uci_host.cpp) of a PUSCH of the four batched pipelines: u is a fixed grant's configuration or one grant of a grants call,
// which name these fields alike, and the matrix has the allocation's 12 L_prb rows. On top of the plan, the limits these pipelines share: their
// kernels code HARQ-ACK and RI of 1 or 2 bits and reports of up to 64, the UL-SCH keeps more symbols than it has code blocks, and the report of
// a PUSCH without data leaves none. Returns the plan's reason, or -1 for one of these limits.
template <class U>
static int pusch_pipeline_uci(const U& u, uint32_t nsymb, const srslte_hip_cbsegm_t& seg, srslte_hip_pusch_uci_res_t* pl)
{
  const srslte_hip_pusch_uci_cfg_t c = {u.L_prb,   nsymb,    2 * (uint32_t)u.mod, 12 * u.L_prb,   seg.C * seg.K1, seg.C,
                                        u.ack_len, u.ri_len, u.cqi_len,           u.I_offset_ack, u.I_offset_ri,  u.I_offset_cqi};
  if (const int why = srslte_hip_pusch_uci_plan(&c, pl)) return why;
  return u.ack_len > 2 || u.ri_len > 2 || u.cqi_len > 64 || (seg.C ? pl->G_prime <= seg.C : pl->G_prime != 0) ? -1 : 0;
}

namespace {
__global__ void pusch_ack_decide_kernel(const int* __restrict__ sum, uint8_t* __restrict__ ack, int nof_sf)
{
  const int sf = blockIdx.x * blockDim.x + threadIdx.x;
  if (sf >= nof_sf) return;
  ack[2 * sf]     = sum[4 * sf] > 0;     // uci.c:782-785
  ack[2 * sf + 1] = sum[4 * sf + 1] > 0;
}
} // namespace

// srslte_hip_ul_rx_batch_grants: the shared grants machinery with one slot per PUSCH, plus the PUSCH front end's buffers; made on first use
struct UlRxGrants {
  GrantsState      gs;
  DevBuf<cf32>     g_z, g_d;  // [max_grants][nsymb * 12 * nof_prb]
  DevBuf<float>    g_res;     // [max_grants] x srslte_hip_chest_ul_res_t
  DevBuf<int>      g_uci_sum; // [max_grants][4] HARQ-ACK accumulators, then the same for the rank indication
  DevBuf<uint8_t>  g_uci;     // [max_grants][2] HARQ-ACK decisions of the last grants call, then [max_grants][2] rank indications
  DevBuf<uint8_t>  g_cqi;     // [max_grants][64] CQI report bits of the last grants call, then [max_grants] CRC flags
};

struct srslte_hip_ul_rx {
  srslte_hip_ul_rx_cfg_t cfg   = {};
  srslte_hip_ofdm_t*     ofdm  = nullptr;
  srslte_hip_chest_ul_t* chest = nullptr;
  srslte_hip_cbsegm_t    seg   = {};
  PuschGeom              pg    = {};
  std::unique_ptr<SchRxFixed> sch; // from the LLR rows d_g to transport blocks; none (seg.C = 0) for a PUSCH that carries only a CQI report
  DevBuf<uint32_t>       d_scr;
  DevBuf<cf32>           d_grid, d_ce, d_z, d_d;
  DevBuf<float>          d_res; // [B] x srslte_hip_chest_ul_res_t
  DevBuf<int16_t>        d_g;   // [B][nbits] + 16; the CQI report's Qp_cqi Qm LLRs in front of the UL-SCH's in every row
  DevBuf<int>            d_ack_sum; // [B][4] ACK, then [B][4] RI
  DevBuf<uint8_t>        d_ack;     // [B][2] HARQ-ACK decisions of the last call, then [B][2] rank indications
  DevBuf<uint8_t>        d_cqi;     // [B][64] CQI report bits of the last call, then [B] CRC flags
  int                    Qp_cqi = 0;
  std::unique_ptr<UlRxGrants> ug; // srslte_hip_ul_rx_batch_grants: created on first use
  ~srslte_hip_ul_rx()
  {
    srslte_hip_ofdm_destroy(ofdm);
    srslte_hip_chest_ul_destroy(chest);
  }
};

extern "C" const uint8_t* srslte_hip_ul_rx_ack(const srslte_hip_ul_rx_t* q) { return q ? q->d_ack : nullptr; }
extern "C" const uint8_t* srslte_hip_ul_rx_ri(const srslte_hip_ul_rx_t* q) { return q ? q->d_ack + 2 * q->cfg.max_batch : nullptr; }
extern "C" const uint8_t* srslte_hip_ul_rx_cqi(const srslte_hip_ul_rx_t* q) { return q ? q->d_cqi : nullptr; }
extern "C" const uint8_t* srslte_hip_ul_rx_grants_ack(const srslte_hip_ul_rx_t* q) { return q && q->ug ? q->ug->g_uci : nullptr; }
extern "C" const uint8_t* srslte_hip_ul_rx_grants_cqi(const srslte_hip_ul_rx_t* q) { return q && q->ug ? q->ug->g_cqi : nullptr; }
extern "C" const uint8_t* srslte_hip_ul_rx_grants_ri(const srslte_hip_ul_rx_t* q)
{
  return q && q->ug ? q->ug->g_uci + 2 * (q->cfg.max_grants ? q->cfg.max_grants : q->cfg.max_batch) : nullptr;
}

extern "C" void srslte_hip_ul_rx_destroy(srslte_hip_ul_rx_t* q) { delete q; }

// phy_hip.h, "Sample formats": d_iq of every entry point of the object is in the OFDM object's format from here on
extern "C" int srslte_hip_ul_rx_set_iq_format(srslte_hip_ul_rx_t* q, int format, float scale)
{
  return q ? srslte_hip_ofdm_set_sample_format(q->ofdm, format, scale) : SRSLTE_ERROR_INVALID_INPUTS;
}

extern "C" srslte_hip_ul_rx_t* srslte_hip_ul_rx_create(const srslte_hip_ul_rx_cfg_t* cfg)
{
  if (!cfg || cfg->max_batch == 0 || cfg->mod < 1 || cfg->mod > 3 || cfg->max_iterations == 0 || cfg->L_prb < 1 ||
      cfg->n_prb + cfg->L_prb > cfg->nof_prb || (cfg->hopping && cfg->n_prb_slot1 + cfg->L_prb > cfg->nof_prb) ||
      !srslte_hip_dft_precoding_valid_prb(cfg->L_prb)) {
    hip_log("[srslte_hip] ul_rx: invalid configuration\n");
    return nullptr;
  }
  std::unique_ptr<srslte_hip_ul_rx> q(new srslte_hip_ul_rx());
  q->cfg = *cfg;
  if (fixed_grant_segmentation("ul_rx", cfg->tbs, &q->seg)) return nullptr;
  const uint32_t P = cfg->nof_prb, B = cfg->max_batch, C = q->seg.C, Qm = 2 * (uint32_t)cfg->mod, M_sc = 12 * cfg->L_prb;
  const uint32_t nsl   = cfg->cp_ext ? 6 : 7;                       // SRSLTE_CP_NSYMB
  const uint32_t nsymb = 2 * (nsl - 1) - (cfg->shortened ? 1 : 0); // 2 (N_symb - 1) - N_srs data symbols (ra_ul.c nof_symb, pusch.c:52-91)
  const uint32_t nof_re = nsymb * M_sc, nbits = nof_re * Qm, scr_words = (nbits + 31) / 32 + 1; // spare word: the demapper reads two per symbol
  srslte_hip_pusch_uci_res_t uci;
  if (const int why = pusch_pipeline_uci(*cfg, nsymb, q->seg, &uci)) {
    // tbs = 0: a PUSCH without UL-SCH data carries a CQI report and nothing to decode (srslte_ulsch_decode, sch.c:1031-1065)
    hip_log(why == SRSLTE_HIP_PUSCH_UCI_EMPTY ? "[srslte_hip] ul_rx: neither a transport block nor a CQI report\n" : "[srslte_hip] ul_rx: initialisation failed\n");
    return nullptr;
  }
  q->ofdm  = srslte_hip_ofdm_create((int)P, cfg->cp_ext ? 0 : 1, 1);
  q->chest = srslte_hip_chest_ul_create(cfg->cell_id, P, cfg->cp_ext ? 0 : 1, &cfg->dmrs_cfg);
  bool ok  = q->ofdm && q->chest && srslte_hip_ofdm_set_freq_shift(q->ofdm, -0.5f) == SRSLTE_SUCCESS; // enb_ul.c:62-63 (no normalisation)
  if (ok) { // srslte_sequence_pusch (sequences.c:65-67), one sequence per subframe index
    std::vector<uint32_t> scr;
    lte_scr_table([&](uint32_t sf) { return ((uint32_t)cfg->rnti << 14) + (sf << 9) + cfg->cell_id; }, nbits, scr_words, scr);
    ok = upload(q->d_scr, scr) == SRSLTE_SUCCESS;
  }
  const size_t glen = (size_t)2 * nsl * 12 * P;
  ok = ok && !q->d_grid.alloc(glen * B) && !q->d_ce.alloc(glen * B) && hipMemset(q->d_ce, 0, sizeof(cf32) * glen * B) == hipSuccess &&
       !q->d_z.alloc((size_t)nof_re * B) && !q->d_d.alloc((size_t)nof_re * B) && !q->d_res.alloc((size_t)5 * B) && !q->d_g.alloc((size_t)nbits * B + 16) &&
       !q->d_ack_sum.alloc((size_t)8 * B) && !q->d_ack.alloc((size_t)4 * B) && hipMemset(q->d_ack, 0, (size_t)4 * B) == hipSuccess &&
       !q->d_cqi.alloc((size_t)65 * B) && hipMemset(q->d_cqi, 0, (size_t)65 * B) == hipSuccess;
  ok = ok && hipDeviceSynchronize() == hipSuccess; // the memsets above ran on the null stream
  if (ok && C) { // as for the PDSCH, with the whole parity layout and the assembly kernel
    // the UL-SCH is rate-matched to what the RI and the CQI report leave (sch.c:1157-1160) and follows the report in the stream
    SchRxFixed::Cfg sc = {}; // 16-bit LLRs, no CSI weighting, neither permission
    sc.tbs = cfg->tbs; sc.max_batch = B; sc.max_iterations = cfg->max_iterations; sc.Qm = Qm; sc.Nl = 1; sc.e_off = uci.Q_cqi; sc.max_bits = nbits;
    sc.nof_re[0] = sc.nof_re[1] = sc.nof_re[2] = uci.G_prime;
    q->sch.reset(new SchRxFixed());
    ok = q->sch->init(sc) == SRSLTE_SUCCESS;
  }
  if (!ok) {
    hip_log("[srslte_hip] ul_rx: initialisation failed\n");
    return nullptr;
  }
  q->pg.cell_nre = 12 * (int)P; q->pg.M_sc = (int)M_sc; q->pg.n_prb = (int)cfg->n_prb; q->pg.n_prb1 = (int)(cfg->hopping ? cfg->n_prb_slot1 : cfg->n_prb); q->pg.mod = cfg->mod; q->pg.Qm = (int)Qm;
  q->pg.scr_words = (int)scr_words; q->pg.mmse = cfg->mmse; q->pg.nsymb = (int)nsymb; q->pg.nsl = (int)nsl;
  q->pg.ack.O = (int)cfg->ack_len; q->pg.ack.Qprime = (int)uci.Qp_ack;
  q->pg.ack_sum = q->d_ack_sum;
  q->pg.ri.O = (int)cfg->ri_len; q->pg.ri.Qprime = (int)uci.Qp_ri; q->pg.ri_sum = q->d_ack_sum + 4 * B;
  q->Qp_cqi   = (int)uci.Qp_cqi;
  return q.release();
}

extern "C" const void* srslte_hip_ul_rx_debug_buffer(const srslte_hip_ul_rx_t* q, int which)
{
  if (!q) return nullptr;
  switch (which) {
    case 0: return q->d_grid;
    case 1: return q->d_ce;
    case 2: return q->d_res;
    case 3: return q->d_d;
    case 4: return q->d_g;
    case 5: return q->sch ? q->sch->d_w.get() : nullptr;
    case 6: return q->sch ? q->sch->d_cb_iters.get() : nullptr;
    case 7: return q->sch ? q->sch->d_cb_ok.get() : nullptr;
    case 8: return q->sch ? q->sch->d_cb_bytes.get() : nullptr;
    case 9: return q->d_z;
    case 10: return q->d_ack;
    // per-PUSCH grants mode: estimator results, de-precoded symbols (at each PUSCH's offset), LLR rows, pass counts per block slot
    case 20: return q->ug ? q->ug->g_res : nullptr;
    case 21: return q->ug ? q->ug->g_d : nullptr;
    case 22: return q->ug ? q->ug->gs.d_e : nullptr;
    case 23: return q->ug ? q->ug->gs.d_cb_iters : nullptr;
  }
  return nullptr;
}

// d_iq: [nof_sf][15*N]; outputs as srslte_hip_dl_rx_batch. Subframe b is TTI tti0 + b.
extern "C" int srslte_hip_ul_rx_batch(srslte_hip_ul_rx_t* q, const void* d_iq, uint32_t tti0, uint32_t nof_sf, uint8_t* d_tb, uint32_t tb_stride,
                                      uint8_t* d_tb_ok, void* stream)
{
  return srslte_hip_ul_rx_batch_harq(q, d_iq, tti0, nof_sf, 0, 1, d_tb, tb_stride, d_tb_ok, stream);
}

// HARQ on the uplink (srslte_ulsch_decode hands grant.tb.rv and cfg->softbuffers.rx to the same decode_tb as the downlink, sch.c:1063):
// slot b keeps its code blocks' soft buffers, CRC flags and bytes between calls, exactly as srslte_hip_dl_rx_batch_harq. new_data != 0
// starts new transport blocks; new_data == 0 adds the de-matched LLRs of redundancy version rv to the kept buffers and leaves blocks whose
// CRC already passed alone. UCI (ACK / RI / CQI) is per transmission and decoded afresh on every call.
extern "C" int srslte_hip_ul_rx_batch_harq(srslte_hip_ul_rx_t* q, const void* d_iq, uint32_t tti0, uint32_t nof_sf, uint32_t rv, int new_data,
                                           uint8_t* d_tb, uint32_t tb_stride, uint8_t* d_tb_ok, void* stream)
{
  if (!q || !d_iq || !d_tb || !d_tb_ok || rv > 3 || nof_sf > q->cfg.max_batch || tb_stride < q->cfg.tbs / 8 + 6) return SRSLTE_ERROR_INVALID_INPUTS;
  if (nof_sf == 0) return SRSLTE_SUCCESS;
  hipStream_t    st = (hipStream_t)stream;
  const SchHarq  harq = {rv, new_data ? 0 : 1};
  if (q->sch && q->sch->ensure_rv(rv)) return SRSLTE_ERROR; // made on first use, before anything is queued
  int            r = srslte_hip_ofdm_rx_sf_batch(q->ofdm, d_iq, q->d_grid, (int)nof_sf, stream);
  if (r) return r;
  r = srslte_hip_chest_ul_estimate_pusch_batch_hop(q->chest, tti0, q->cfg.L_prb, q->cfg.n_prb, (uint32_t)q->pg.n_prb1, q->cfg.n_dmrs, q->d_grid, q->d_ce, q->d_res, (int)nof_sf,
                                               stream);
  if (r) return r;
  PuschGeom g = q->pg;
  g.tti0      = (int)tti0;
  g.ack_sum   = q->d_ack_sum;
  g.ri_sum    = q->d_ack_sum + 4 * q->cfg.max_batch;
  const dim3 grid(ceil_div(g.M_sc, 256), g.nsymb, nof_sf);
  hipLaunchKernelGGL(pusch_eq_kernel, grid, dim3(256), 0, st, (const cf32*)q->d_grid, (const cf32*)q->d_ce, (const float*)q->d_res, q->d_z, g);
  LAUNCH_CHECK();
  r = srslte_hip_dft_precoding_batch(q->d_z, q->d_d, q->cfg.L_prb, g.nsymb * nof_sf, 0, stream); // srslte_dft_precoding_init_rx: inverse, 1/sqrt(N)
  if (r) return r;
  if (g.ack.O) HIP_TRY(hipMemsetAsync(q->d_ack_sum, 0, sizeof(int) * 4 * nof_sf, st));
  if (g.ri.O) HIP_TRY(hipMemsetAsync(q->d_ack_sum + 4 * q->cfg.max_batch, 0, sizeof(int) * 4 * nof_sf, st));
  hipLaunchKernelGGL(pusch_demod_kernel, dim3(ceil_div(g.M_sc, 64), nof_sf), dim3(256), 0, st, (const cf32*)q->d_d, (const uint32_t*)q->d_scr, q->d_g, g);
  LAUNCH_CHECK();
  if (g.ack.O) {
    hipLaunchKernelGGL(pusch_ack_decide_kernel, dim3(ceil_div((int)nof_sf, 64)), dim3(64), 0, st, (const int*)q->d_ack_sum, q->d_ack, (int)nof_sf);
    LAUNCH_CHECK();
  }
  if (g.ri.O) {
    hipLaunchKernelGGL(pusch_ack_decide_kernel, dim3(ceil_div((int)nof_sf, 64)), dim3(64), 0, st, (const int*)(q->d_ack_sum + 4 * q->cfg.max_batch),
                       q->d_ack + 2 * q->cfg.max_batch, (int)nof_sf);
    LAUNCH_CHECK();
  }
  if (q->cfg.cqi_len) { // the report in front of the UL-SCH (sch.c:1031-1056)
    hipLaunchKernelGGL(pusch_cqi_decode_kernel, dim3(nof_sf), dim3(256), 0, st, (const int16_t*)q->d_g, g.nsymb * g.M_sc * g.Qm, q->Qp_cqi * g.Qm,
                       (int)q->cfg.cqi_len, q->d_cqi, q->d_cqi + 64 * q->cfg.max_batch, (const PuschDesc*)nullptr);
    LAUNCH_CHECK();
  }
  if (!q->sch) { // no UL-SCH data: nothing to de-match or decode, no transport block (sch.c:1062-1065)
    HIP_TRY(hipMemsetAsync(d_tb_ok, 0, nof_sf, st));
    return SRSLTE_SUCCESS;
  }
  if (int rc = q->sch->dematch(q->d_g, tti0, nof_sf, harq, st)) return rc;
  if (int rc = q->sch->decode(nof_sf, harq, d_tb, tb_stride, d_tb_ok, st)) return rc;
  return q->sch->assemble(nof_sf, d_tb, tb_stride, d_tb_ok, st);
}

static int ul_rx_grants_init(srslte_hip_ul_rx_t* q, uint32_t V, uint32_t max_re)
{
  const uint32_t P = q->cfg.nof_prb;
  q->ug.reset(new UlRxGrants());
  UlRxGrants* u = q->ug.get();
  if (grants_alloc(&u->gs, 12 * 12 * P, V, q->seg.C, 0, false, (sizeof(PuschDesc) + sizeof(ChestUlItem)) * V)) return SRSLTE_ERROR;
  if (u->g_z.alloc((size_t)max_re * V) || u->g_d.alloc((size_t)max_re * V) || u->g_res.alloc((size_t)5 * V) || u->g_uci_sum.alloc((size_t)8 * V) ||
      u->g_uci.alloc((size_t)4 * V) || u->g_cqi.alloc((size_t)65 * V))
    return SRSLTE_ERROR;
  HIP_TRY(hipMemset(u->g_cqi, 0, (size_t)65 * V));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemset(u->g_uci, 0, (size_t)4 * V));
  HIP_TRY(hipDeviceSynchronize());
  return SRSLTE_SUCCESS;
}

// Per-PUSCH grants: what an eNB receives in a run of TTIs - any number of PUSCHs per subframe, each with its own allocation (L_prb, PRB offset per
// slot), DMRS cyclic shift, RNTI, modulation, transport block and redundancy version (srslte_enb_ul_get_pusch called once per scheduled UE,
// enb_ul.c:200-235, after one srslte_enb_ul_fft per TTI). The OFDM demodulation runs once per subframe; estimator, equaliser and demapper take
// their geometry from per-PUSCH descriptors, the transform de-precoding runs once per distinct L_prb (PUSCHs of one size sit next to each other
// in the symbol buffers), and from the LLRs on it is the downlink's grants machinery with one slot per PUSCH: slot p = grants[p] keeps soft
// buffers, CRC flags and bytes between calls (HARQ as srslte_hip_ul_rx_batch_harq). HARQ-ACK, rank indication and CQI report per PUSCH.
// pucch: the PUCCHs of srslte_hip_ul_rx_batch_grants_pucch, decoded from the grid right after the OFDM demodulation (nullptr: none)
struct UlPucchCall {
  srslte_hip_ul_ctrl_t*         ctrl;
  const srslte_hip_pucch_req_t* reqs;
  uint32_t                      nof;
  srslte_hip_pucch_res_t*       d_res;
};
// srs: the sounding requests of srslte_hip_ul_rx_batch_grants_pucch_srs, read from the same grid (nullptr: none)
struct UlSrsCall {
  srslte_hip_srs_t*          srs;
  const srslte_hip_srs_ue_t* list;
  uint32_t                   nof;
  srslte_hip_srs_res_t*      d_res;
  void*                      d_ce;
};

static int ul_rx_grants(srslte_hip_ul_rx_t* q, const void* d_iq, uint32_t tti0, uint32_t nof_sf, const srslte_hip_ul_grant_t* grants, uint32_t nof_grants,
                        uint8_t* d_tb, uint32_t tb_stride, uint8_t* d_tb_ok, const UlPucchCall* pucch, const UlSrsCall* srs, void* stream)
{
  if (!q || !d_iq || !grants || !d_tb || !d_tb_ok || nof_sf > q->cfg.max_batch || tb_stride < q->cfg.tbs / 8 + 6) return SRSLTE_ERROR_INVALID_INPUTS;
  const uint32_t V = q->cfg.max_grants ? q->cfg.max_grants : q->cfg.max_batch, P = q->cfg.nof_prb;
  if (nof_grants > V || q->seg.C == 0) return SRSLTE_ERROR_INVALID_INPUTS; // an object made without a transport-block size has no decoder
  if (nof_sf == 0 || nof_grants == 0) return SRSLTE_SUCCESS;
  hipStream_t    st    = (hipStream_t)stream;
  const uint32_t nsymb = (uint32_t)q->pg.nsymb, max_re = nsymb * 12 * P;
  if (!q->ug && ul_rx_grants_init(q, V, max_re)) { // a failed start leaves no half-made state behind: srslte_hip_ul_rx_grants_ack() stays null
    hip_log("[srslte_hip] ul_rx grants: initialisation failed\n");
    q->ug.reset();
    return SRSLTE_ERROR;
  }
  UlRxGrants*  u     = q->ug.get();
  GrantsState* g     = &u->gs;
  uint8_t*     h_pin = nullptr;
  if (int r = g->desc.begin(&h_pin)) return r;
  const GrantsDesc h(g, h_pin), d(g, g->desc.dev_bytes());
  GrantDev*        h_gr = h.gr;
  SfDesc*          h_sf = h.sf;
  auto*            h_pd = reinterpret_cast<PuschDesc*>(h.extra); // extra_desc_bytes: PuschDesc[V] | ChestUlItem[V]
  auto*            h_it = reinterpret_cast<ChestUlItem*>(h_pd + V);
  auto*            d_pd = reinterpret_cast<PuschDesc*>(d.extra);
  auto*            d_it = reinterpret_cast<ChestUlItem*>(d_pd + V);
  GrantsBuild bd;
  bd.g = g; bd.h_sf = h_sf; bd.h_cb = h.cb; bd.l8 = false; bd.max_tbs = q->cfg.tbs; bd.npt = 1; bd.max_mod = 3; bd.who = "ul_rx";
  // PUSCHs in the order (L_prb, n_dmrs): one estimator launch per (L_prb, n_dmrs), one de-precoding launch per L_prb
  std::vector<uint32_t> order(nof_grants);
  for (uint32_t p = 0; p < nof_grants; p++) order[p] = p;
  uint32_t max_M = 0;
  for (uint32_t p = 0; p < nof_grants; p++) {
    const srslte_hip_ul_grant_t& gr = grants[p];
    // tbs = 0 is a PUSCH without UL-SCH data: it has to carry a CQI report (srslte_ulsch_decode, sch.c:1031-1065); nothing of it reaches the decoder
    if ((gr.tbs == 0 && gr.cqi_len == 0) || gr.tbs > q->cfg.tbs) {
      hip_log("[srslte_hip] ul_rx grants: entry %u: transport block of %u bits (object made for up to %u; 0 needs a CQI report)\n", p, gr.tbs, q->cfg.tbs);
      return SRSLTE_ERROR_INVALID_INPUTS;
    }
    if (gr.sf >= nof_sf || gr.L_prb == 0 || !srslte_hip_dft_precoding_valid_prb(gr.L_prb) || gr.n_prb + gr.L_prb > P || gr.n_prb_slot1 + gr.L_prb > P ||
        gr.n_dmrs >= 8) {
      hip_log("[srslte_hip] ul_rx grants: entry %u: invalid allocation (subframe %u of %u, L_prb %u at %u / %u of %u PRB, n_dmrs %u)\n", p, gr.sf, nof_sf, gr.L_prb,
              gr.n_prb, gr.n_prb_slot1, P, gr.n_dmrs);
      return SRSLTE_ERROR_INVALID_INPUTS;
    }
    max_M = 12 * gr.L_prb > max_M ? 12 * gr.L_prb : max_M;
  }
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    return grants[a].L_prb != grants[b].L_prb ? grants[a].L_prb < grants[b].L_prb : grants[a].n_dmrs < grants[b].n_dmrs;
  });
  uint32_t zoff = 0;
  bool     any_uci = false, any_cqi = false;
  for (uint32_t i = 0; i < nof_grants; i++) {
    const uint32_t               p  = order[i];
    const srslte_hip_ul_grant_t& gr = grants[p];
    GrantDev&                    gd = h_gr[p];
    memset(&gd, 0, sizeof(gd));
    memset(&h_sf[p], 0, sizeof(SfDesc));
    gd.sf_idx = (int)((tti0 + gr.sf) % 10); gd.rnti = gr.rnti; // srslte_sequence_pusch (sequences.c:65-67): the PDSCH's c_init with q = 0
    h_sf[p].scr = g->d_scr + (size_t)p * g->words;
    PuschDesc& pd = h_pd[p];
    memset(&pd, 0, sizeof(pd));
    pd.sf = (int)gr.sf; pd.M_sc = 12 * (int)gr.L_prb; pd.n_prb = (int)gr.n_prb; pd.n_prb1 = (int)gr.n_prb_slot1; pd.mod = gr.mod; pd.Qm = 2 * gr.mod;
    pd.zoff = (int)zoff;
    zoff += nsymb * 12 * gr.L_prb;
    h_it[i].sf = (int)gr.sf; h_it[i].n_prb = (int)gr.n_prb; h_it[i].n_prb1 = (int)gr.n_prb_slot1; h_it[i].row = (int)p;
    // HARQ-ACK and rank indication of this PUSCH (srslte_uci_cfg_t of its srslte_pusch_cfg_t): Q' from the grant's own size and code blocks; the
    // UL-SCH is rate-matched to what the RI symbols leave (sch.c:1157-1160), the ACK symbols overwrite it
    srslte_hip_cbsegm_t seg;
    if (srslte_hip_cbsegm(&seg, gr.tbs)) return SRSLTE_ERROR_INVALID_INPUTS;
    srslte_hip_pusch_uci_res_t uci;
    if (pusch_pipeline_uci(gr, nsymb, seg, &uci) || gr.mod < 1 || gr.mod > 3) {
      hip_log("[srslte_hip] ul_rx grants: entry %u: invalid UCI configuration (ack %u / %u, ri %u / %u, cqi %u / %u)\n", p, gr.ack_len, gr.I_offset_ack, gr.ri_len,
              gr.I_offset_ri, gr.cqi_len, gr.I_offset_cqi);
      return SRSLTE_ERROR_INVALID_INPUTS;
    }
    pd.ack.O = (int)gr.ack_len; pd.ack.Qprime = (int)uci.Qp_ack; pd.ri.O = (int)gr.ri_len; pd.ri.Qprime = (int)uci.Qp_ri;
    pd.cqi_O = (int)gr.cqi_len; pd.cqi_Q = (int)uci.Q_cqi;
    any_uci = any_uci || gr.ack_len || gr.ri_len;
    any_cqi = any_cqi || gr.cqi_len;
    // the report's LLRs come first in the row; the UL-SCH is rate-matched to the rest (sch.c:1058-1064)
    if (gr.tbs == 0) continue; // no code blocks: row p of d_tb_ok becomes 0
    if (int r = bd.add_tb(p, p, gr.mod, gr.tbs, gr.rv, gr.new_data, uci.G_prime, 1, uci.Q_cqi)) return r;
  }
  bd.fill_map(h.map);
  const uint8_t* d_cof = grants_direct_cof(g, h, d, nof_grants, false, [](uint32_t) { return true; });
  bool           no_tb = false;
  for (uint32_t p = 0; p < nof_grants; p++) no_tb = no_tb || grants[p].tbs == 0;
  if (d_cof && no_tb) HIP_TRY(hipMemsetAsync(d_tb_ok, 0, nof_grants, st)); // rows without a transport block get no verdict from a decoder
  int r = srslte_hip_ofdm_rx_sf_batch(q->ofdm, d_iq, q->d_grid, (int)nof_sf, stream);
  if (r) return r;
  if (pucch && (r = srslte_hip_ul_ctrl_pucch_batch(pucch->ctrl, q->d_grid, tti0, nof_sf, pucch->reqs, pucch->nof, pucch->d_res, stream))) return r;
  if (srs && (r = srslte_hip_srs_rx_batch(srs->srs, q->d_grid, tti0, nof_sf, srs->list, srs->nof, srs->d_res, srs->d_ce, stream))) return r;
  const int n16 = (int)((g->desc_bytes + 15) / 16);
  hipLaunchKernelGGL(desc_copy_kernel, dim3(ceil_div(n16, 256)), dim3(256), 0, st, (const uint4*)h_pin, (uint4*)g->desc.dev_bytes(), n16);
  LAUNCH_CHECK();
  if (int rc = g->desc.committed(st)) return rc;
  for (uint32_t i = 0; i < nof_grants;) { // estimator: runs of equal (L_prb, n_dmrs)
    uint32_t j = i + 1;
    while (j < nof_grants && grants[order[j]].L_prb == grants[order[i]].L_prb && grants[order[j]].n_dmrs == grants[order[i]].n_dmrs) j++;
    r = chest_ul_estimate_items(q->chest, tti0, grants[order[i]].L_prb, grants[order[i]].n_dmrs, d_it + i, (int)(j - i), q->d_grid, q->d_ce, u->g_res, st);
    if (r) return r;
    i = j;
  }
  hipLaunchKernelGGL(scr_gen_kernel, dim3(ceil_div((int)g->words, 256), nof_grants), dim3(256), 0, st, (const GrantDev*)d.gr, (const uint32_t*)g->d_basis, g->d_scr,
                     (int)g->words, (int)q->cfg.cell_id);
  hipLaunchKernelGGL(pusch_eq_grants_kernel, dim3(ceil_div((int)max_M, 256), nsymb, nof_grants), dim3(256), 0, st, (const cf32*)q->d_grid, (const cf32*)q->d_ce,
                     (const float*)u->g_res, u->g_z, (const PuschDesc*)d_pd, 12 * (int)P, (int)nsymb, q->cfg.mmse, q->pg.nsl);
  LAUNCH_CHECK();
  for (uint32_t i = 0; i < nof_grants;) { // inverse transform precoding: runs of equal L_prb (srslte_dft_precoding_init_rx: inverse, 1/sqrt(N))
    uint32_t j = i + 1;
    while (j < nof_grants && grants[order[j]].L_prb == grants[order[i]].L_prb) j++;
    const size_t off = (size_t)h_pd[order[i]].zoff;
    r = srslte_hip_dft_precoding_batch(u->g_z + off, u->g_d + off, grants[order[i]].L_prb, nsymb * (j - i), 0, stream);
    if (r) return r;
    i = j;
  }
  if (any_uci) HIP_TRY(hipMemsetAsync(u->g_uci_sum, 0, sizeof(int) * 8 * V, st));
  hipLaunchKernelGGL(pusch_demod_grants_kernel, dim3(ceil_div((int)max_M, 64), nof_grants), dim3(256), 0, st, (const cf32*)u->g_d, (const uint32_t*)g->d_scr,
                     (int)g->words, g->d_e, (int)g->max_bits, (const PuschDesc*)d_pd, (int)nsymb, u->g_uci_sum, u->g_uci_sum + 4 * V);
  LAUNCH_CHECK();
  if (any_uci) { // decisions of every row of the call (zero sums -> 0 where a PUSCH carries none); a call without any leaves the rows alone
    hipLaunchKernelGGL(pusch_ack_decide_kernel, dim3(ceil_div((int)nof_grants, 64)), dim3(64), 0, st, (const int*)u->g_uci_sum, u->g_uci, (int)nof_grants);
    hipLaunchKernelGGL(pusch_ack_decide_kernel, dim3(ceil_div((int)nof_grants, 64)), dim3(64), 0, st, (const int*)(u->g_uci_sum + 4 * V), u->g_uci + 2 * V,
                       (int)nof_grants);
  }
  if (any_cqi) { // the reports in front of the UL-SCH (sch.c:1031-1056); rows without one keep what they held
    hipLaunchKernelGGL(pusch_cqi_decode_kernel, dim3(nof_grants), dim3(256), 0, st, (const int16_t*)g->d_e, (int)g->max_bits, 0, 0, u->g_cqi, u->g_cqi + 64 * V,
                       (const PuschDesc*)d_pd);
  }
  LAUNCH_CHECK();
  return grants_back_end(g, bd, d.sf, d.cb, d.map, tti0, q->cfg.max_iterations, nof_grants, nof_grants, V, d_tb, tb_stride, d_tb_ok, st, d_cof);
}

extern "C" int srslte_hip_ul_rx_batch_grants(srslte_hip_ul_rx_t* q, const void* d_iq, uint32_t tti0, uint32_t nof_sf, const srslte_hip_ul_grant_t* grants,
                                             uint32_t nof_grants, uint8_t* d_tb, uint32_t tb_stride, uint8_t* d_tb_ok, void* stream)
{
  return ul_rx_grants(q, d_iq, tti0, nof_sf, grants, nof_grants, d_tb, tb_stride, d_tb_ok, nullptr, nullptr, stream);
}

// srslte_enb_ul_fft + get_pusch per grant + get_pucch per request: the PUCCH requests are checked before anything is queued; without grants
// the call is the OFDM demodulation and the PUCCH batch alone
extern "C" int srslte_hip_ul_rx_batch_grants_pucch(srslte_hip_ul_rx_t* q, const void* d_iq, uint32_t tti0, uint32_t nof_sf, const srslte_hip_ul_grant_t* grants,
                                                   uint32_t nof_grants, uint8_t* d_tb, uint32_t tb_stride, uint8_t* d_tb_ok, srslte_hip_ul_ctrl_t* ctrl,
                                                   const srslte_hip_pucch_req_t* reqs, uint32_t nof_pucch, srslte_hip_pucch_res_t* d_res, void* stream)
{
  if (!q || !d_iq || nof_sf > q->cfg.max_batch || !ul_ctrl_same_cell(ctrl, q->cfg.nof_prb, q->cfg.cell_id, q->cfg.cp_ext) || (nof_pucch && !d_res))
    return SRSLTE_ERROR_INVALID_INPUTS;
  if (int r = ul_ctrl_check(ctrl, nof_sf, reqs, nof_pucch)) return r;
  if (nof_grants == 0) {
    if (nof_sf == 0 || nof_pucch == 0) return SRSLTE_SUCCESS;
    if (int r = srslte_hip_ofdm_rx_sf_batch(q->ofdm, d_iq, q->d_grid, (int)nof_sf, stream)) return r;
    return srslte_hip_ul_ctrl_pucch_batch(ctrl, q->d_grid, tti0, nof_sf, reqs, nof_pucch, d_res, stream);
  }
  const UlPucchCall pc = {ctrl, reqs, nof_pucch, d_res};
  return ul_rx_grants(q, d_iq, tti0, nof_sf, grants, nof_grants, d_tb, tb_stride, d_tb_ok, nof_pucch ? &pc : nullptr, nullptr, stream);
}

// ... + the sounding requests of srs_list on the same grid. ctrl and srs may each be NULL; both lists are checked before anything is queued;
// without grants the call is the OFDM demodulation and the two batches alone
extern "C" int srslte_hip_ul_rx_batch_grants_pucch_srs(srslte_hip_ul_rx_t* q, const void* d_iq, uint32_t tti0, uint32_t nof_sf, const srslte_hip_ul_grant_t* grants,
                                                       uint32_t nof_grants, uint8_t* d_tb, uint32_t tb_stride, uint8_t* d_tb_ok, srslte_hip_ul_ctrl_t* ctrl,
                                                       const srslte_hip_pucch_req_t* reqs, uint32_t nof_pucch, srslte_hip_pucch_res_t* d_res,
                                                       srslte_hip_srs_t* srs, const srslte_hip_srs_ue_t* srs_list, uint32_t nof_srs,
                                                       srslte_hip_srs_res_t* d_srs_res, void* d_srs_ce, void* stream)
{
  if (!q || !d_iq || nof_sf > q->cfg.max_batch) return SRSLTE_ERROR_INVALID_INPUTS;
  if (!ctrl) nof_pucch = 0;
  if (!srs) nof_srs = 0;
  if (ctrl && (!ul_ctrl_same_cell(ctrl, q->cfg.nof_prb, q->cfg.cell_id, q->cfg.cp_ext) || (nof_pucch && !d_res))) return SRSLTE_ERROR_INVALID_INPUTS;
  if (srs && (!srs_same_cell(srs, q->cfg.nof_prb, q->cfg.cell_id, q->cfg.cp_ext) || (nof_srs && (!d_srs_res || !d_srs_ce)))) return SRSLTE_ERROR_INVALID_INPUTS;
  if (ctrl)
    if (int r = ul_ctrl_check(ctrl, nof_sf, reqs, nof_pucch)) return r;
  if (srs)
    if (int r = srs_list_check(srs_cfg(srs), tti0, nof_sf, srs_list, nof_srs)) return r;
  if (nof_grants == 0) {
    if (nof_sf == 0 || (nof_pucch == 0 && nof_srs == 0)) return SRSLTE_SUCCESS;
    if (int r = srslte_hip_ofdm_rx_sf_batch(q->ofdm, d_iq, q->d_grid, (int)nof_sf, stream)) return r;
    if (nof_pucch)
      if (int r = srslte_hip_ul_ctrl_pucch_batch(ctrl, q->d_grid, tti0, nof_sf, reqs, nof_pucch, d_res, stream)) return r;
    return nof_srs ? srslte_hip_srs_rx_batch(srs, q->d_grid, tti0, nof_sf, srs_list, nof_srs, d_srs_res, d_srs_ce, stream) : SRSLTE_SUCCESS;
  }
  const UlPucchCall pc = {ctrl, reqs, nof_pucch, d_res};
  const UlSrsCall   sc = {srs, srs_list, nof_srs, d_srs_res, d_srs_ce};
  return ul_rx_grants(q, d_iq, tti0, nof_sf, grants, nof_grants, d_tb, tb_stride, d_tb_ok, nof_pucch ? &pc : nullptr, nof_srs ? &sc : nullptr, stream);
}
