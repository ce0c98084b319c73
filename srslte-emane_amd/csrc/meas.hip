// Neighbour-cell measurement for gfx950, FDD, normal CP (include/srslte_hip/phy_hip.h, "Neighbour-cell measurement"):
// srslte_refsignal_dl_sync_set_cell + srslte_refsignal_dl_sync_run (lib/src/phy/sync/refsignal_dl_sync.c:84-154, :185-355) for a batch of
// captures x candidate cells. L = sf_len = 15 N, N = symbol_sz; the 2 L-point transforms of find_peak are four-step, n = N n1 + n2 and
// k = k1 + 30 k2 (n1, k1 < 30; n2, k2 < N), spectra kept in [k1][k2] order.
//   meas_fill_kernel     one workgroup per (subframe, cell): PSS / SSS of subframes 0 and 5 and the CRS of ports 0 and 1 on a zeroed grid
//   (ofdm_tx_kernel of fft.hip over the 10 n_cells grids)
//   meas_scale_kernel    the replicas times 1 / (8 nof_prb)
//   meas_col_fwd_kernel  grid (N / 128, block, item): a lane per n2 reads 30 rows at stride N (coalesced across lanes; rows past the input's
//                        length read as zero: the replica's padding), the 30-point DFT over n1 in registers, times the inter-stage twiddle
//   (dft_batch_kernel of fft.hip: the N-point row FFTs, forward)
//   (dft_rows30_mulconj_kernel of fft.hip: product with the conjugated filter spectrum, N-point inverse row FFTs, conjugated twiddle, 1 / 2 L)
//   meas_col_inv_kernel  grid (N / 128, block, row): the closing 30-point pass for the 15 outputs n1 < 15 that make c[k], k < L, reduced to the
//                        workgroup's (max |c|^2, first index, sum |c|^2); 2 KB of LDS
//   meas_decide_kernel   a thread per row: the peak over blocks (the first one strictly larger), mean rms, threshold; peak_idx for the next stage
//   meas_sf_kernel       one workgroup per (subframe, row): the four dot products of N terms and the four powers (wave_sum); 1 KB of LDS
//   meas_finish_kernel   a thread per row: the subframes summed in order, averages, dB figures, the result row
#include "cf32_dev.hpp"
#include "common.hpp"
#include "dev_buf.hpp"
#include "phy_hip_internal.hpp"
#include <math.h>
#include <string.h>
#include <vector>

namespace {

constexpr int      COL_THREADS = 128; // every symbol size is a multiple
constexpr int      SF_THREADS  = 256;
constexpr uint32_t NO_INDEX    = 0xffffffffu;
constexpr uint32_t MAX_BLOCKS  = 10; // SRSLTE_NOF_SF_X_FRAME (refsignal_dl_sync.c:201)

// cos / sin of 2 pi k / 30
__device__ const float C30[30] = {1.f,           0.978147601f,  0.913545458f,  0.809016994f,  0.669130606f,  0.5f,           0.309016994f,  0.104528463f,
                                  -0.104528463f, -0.309016994f, -0.5f,         -0.669130606f, -0.809016994f, -0.913545458f, -0.978147601f, -1.f,
                                  -0.978147601f, -0.913545458f, -0.809016994f, -0.669130606f, -0.5f,         -0.309016994f, -0.104528463f, 0.104528463f,
                                  0.309016994f,  0.5f,          0.669130606f,  0.809016994f,  0.913545458f,  0.978147601f};
__device__ const float S30[30] = {0.f,           0.207911691f,  0.406736643f,  0.587785252f,  0.743144825f,  0.866025404f,  0.951056516f,  0.994521895f,
                                  0.994521895f,  0.951056516f,  0.866025404f,  0.743144825f,  0.587785252f,  0.406736643f,  0.207911691f,  0.f,
                                  -0.207911691f, -0.406736643f, -0.587785252f, -0.743144825f, -0.866025404f, -0.951056516f, -0.994521895f, -0.994521895f,
                                  -0.951056516f, -0.866025404f, -0.743144825f, -0.587785252f, -0.406736643f, -0.207911691f};

// a exp(SGN j 2 pi m / 30); m is a compile-time constant where the caller's loops are unrolled
template <int SGN> __device__ __forceinline__ cf32 mulw30(cf32 a, int m)
{
  const float c = C30[m % 30], s = SGN > 0 ? S30[m % 30] : -S30[m % 30];
  return make_float2(a.x * c - a.y * s, a.x * s + a.y * c);
}
template <int SGN> __device__ __forceinline__ void dft3(cf32& a, cf32& b, cf32& c)
{
  const float s3 = SGN * 0.86602540378443864676f;
  const cf32  t = cadd(b, c), d = csub(b, c), u = make_float2(-s3 * d.y, s3 * d.x), m = make_float2(a.x - 0.5f * t.x, a.y - 0.5f * t.y);
  a = cadd(a, t), b = cadd(m, u), c = csub(m, u);
}
// o[r] = sum_q v[q] exp(SGN j 2 pi q r / 30) in registers, 30 = 5 x 6 (q = 6 qa + qb, r = ra + 5 rb): 5-point sums over qa, the twiddle
// exp(SGN j 2 pi qb ra / 30), 6-point transforms (2 x 3) over qb. A caller that uses only r < 15 (rb < 3) pays for half of the last step.
template <int SGN> __device__ __forceinline__ void dft30(const cf32 (&v)[30], cf32 (&o)[30])
{
  cf32 t[5][6]; // [ra][qb]
#pragma unroll
  for (int qb = 0; qb < 6; qb++) {
#pragma unroll
    for (int ra = 0; ra < 5; ra++) {
      cf32 acc = v[qb];
#pragma unroll
      for (int qa = 1; qa < 5; qa++) acc = cadd(acc, mulw30<SGN>(v[6 * qa + qb], 6 * qa * ra));
      t[ra][qb] = (qb * ra) ? mulw30<SGN>(acc, qb * ra) : acc;
    }
  }
#pragma unroll
  for (int ra = 0; ra < 5; ra++) {
    cf32 e0 = t[ra][0], e1 = t[ra][2], e2 = t[ra][4], o0 = t[ra][1], o1 = t[ra][3], o2 = t[ra][5];
    dft3<SGN>(e0, e1, e2);
    dft3<SGN>(o0, o1, o2);
    o1 = mulw30<SGN>(o1, 5), o2 = mulw30<SGN>(o2, 10);
    o[ra] = cadd(e0, o0), o[ra + 5] = cadd(e1, o1), o[ra + 10] = cadd(e2, o2);
    o[ra + 15] = csub(e0, o0), o[ra + 20] = csub(e1, o1), o[ra + 25] = csub(e2, o2);
  }
}

struct MeasCellDesc { // offsets in floats into a cell's block of the descriptor: pilots [10][4][2 P] cf32, PSS [62] cf32, SSS [2][62], the id
  uint32_t pss, sss, id, stride;
};
__host__ __device__ inline MeasCellDesc cell_desc(uint32_t P)
{
  MeasCellDesc d;
  d.pss = 160 * P, d.sss = d.pss + 124, d.id = d.sss + 124, d.stride = d.id + 4;
  return d;
}

struct MeasDecision {
  int32_t  found;
  uint32_t peak_idx;
  float    peak, rms;
};

struct MeasParams {
  uint32_t N, L, P, cp0, cp1;
  uint32_t nb, nwg, n_cells, rows, nof_sf, max_sf;
  float    thr;
  size_t   in_stride;
  const cf32*   tw2;     // [30 N]
  const cf32*   seq;     // [cell][10][L]
  const float*  desc;    // the cells' descriptor blocks
  float4*       partial; // [row][nb][nwg]: max |c|^2, first index as bits, sum |c|^2
  MeasDecision* dec;     // [row]
  float4*       sfm;     // [row][max_sf]: rsrp, rssi, cfo of a measured subframe
};

__global__ __launch_bounds__(256) void meas_fill_kernel(const float* __restrict__ desc, cf32* __restrict__ grid, uint32_t P)
{
  const MeasCellDesc d   = cell_desc(P);
  const uint32_t     sf  = blockIdx.x, cell = blockIdx.y, nre = 12 * P, nref = 2 * P, tid = threadIdx.x;
  const float*       blk = desc + (size_t)cell * d.stride;
  const uint32_t     id  = __float_as_uint(blk[d.id]);
  const cf32*        pil = reinterpret_cast<const cf32*>(blk) + (size_t)sf * 4 * nref;
  cf32*              g   = grid + ((size_t)cell * 10 + sf) * 14 * nre;
  if ((sf == 0 || sf == 5) && tid < 62) { // srslte_pss_put_slot / srslte_sss_put_slot: the last two symbols of slot 0, 62 carriers around DC
    const uint32_t k = nre / 2 - 31 + tid;
    g[6 * nre + k]   = reinterpret_cast<const cf32*>(blk + d.pss)[tid];
    g[5 * nre + k]   = make_float2(blk[d.sss + (sf ? 62 : 0) + tid], 0.f);
  }
  for (uint32_t i = tid; i < 4 * 2 * nref; i += 256) { // srslte_refsignal_cs_put_sf of ports 0 and 1 (refsignal_dl.c:249-270)
    const uint32_t l = i / (2 * nref), port = (i / nref) & 1u, m = i % nref;
    const uint32_t sym = (l & 1u) ? (l / 2 + 1) * 7 - 3 : (l / 2) * 7, fidx = ((((l + port) & 1u) ? 3u : 0u) + id % 6) % 6;
    g[sym * nre + fidx + 6 * m] = pil[l * nref + m];
  }
}

__global__ __launch_bounds__(256) void meas_scale_kernel(cf32* __restrict__ x, size_t n, float scale)
{
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) x[i] = cscale(x[i], scale);
}

// out[((item nblk + b) 30 + k1) N + n2] = tw2[n2 k1] sum_{n1 < n1_in} in[item item_stride + b L + n1 N + n2] exp(-j 2 pi n1 k1 / 30)
__global__ __launch_bounds__(COL_THREADS) void meas_col_fwd_kernel(const cf32* __restrict__ in, size_t item_stride, uint32_t L, uint32_t N,
                                                                   uint32_t n1_in, const cf32* __restrict__ tw2, cf32* __restrict__ out)
{
  const uint32_t n2 = blockIdx.x * COL_THREADS + threadIdx.x, b = blockIdx.y, nblk = gridDim.y, item = blockIdx.z;
  if (n2 >= N) return;
  const cf32* x = in + (size_t)item * item_stride + (size_t)b * L + n2;
  cf32        v[30];
#pragma unroll
  for (int n1 = 0; n1 < 30; n1++) v[n1] = (uint32_t)n1 < n1_in ? x[(size_t)n1 * N] : make_float2(0.f, 0.f);
  cf32* o = out + ((size_t)item * nblk + b) * 30 * N + n2;
  cf32 y[30];
  dft30<-1>(v, y);
#pragma unroll
  for (int k1 = 0; k1 < 30; k1++) o[(size_t)k1 * N] = cmul(y[k1], tw2[n2 * (uint32_t)k1]);
}

// c[n1 N + n2] = sum_k1 B[k1][n2] exp(+j 2 pi n1 k1 / 30), n1 < 15: the L outputs of block b of a row that find_peak looks at
__global__ __launch_bounds__(COL_THREADS) void meas_col_inv_kernel(MeasParams p, const cf32* __restrict__ B)
{
  __shared__ float    s_v[COL_THREADS];
  __shared__ uint32_t s_i[COL_THREADS];
  __shared__ float    s_sum[COL_THREADS / 64];
  const uint32_t tid = threadIdx.x, n2 = blockIdx.x * COL_THREADS + tid, b = blockIdx.y, row = blockIdx.z, N = p.N;
  float          best = -INFINITY, sum = 0.f;
  uint32_t       bi   = NO_INDEX;
  if (n2 < N) {
    const cf32* src = B + ((size_t)row * p.nb + b) * 30 * N + n2;
    cf32        v[30];
#pragma unroll
    for (int k1 = 0; k1 < 30; k1++) v[k1] = src[(size_t)k1 * N];
    cf32 y[30];
    dft30<1>(v, y);
#pragma unroll
    for (int n1 = 0; n1 < 15; n1++) {
      const cf32  c = y[n1];
      const float m = c.x * c.x + c.y * c.y;
      sum += m;
      if (m > best) best = m, bi = (uint32_t)n1 * N + n2;
    }
  }
  // the first maximum (srslte_vec_max_abs_ci: the lowest index among equals) and the power, in a fixed order
  sum = wave_sum(sum);
  if (tid % 64 == 0) s_sum[tid / 64] = sum;
  s_v[tid] = best, s_i[tid] = bi;
  __syncthreads();
  for (int o = COL_THREADS / 2; o > 0; o >>= 1) {
    if (tid < (uint32_t)o) {
      const float    v2 = s_v[tid + o];
      const uint32_t i2 = s_i[tid + o];
      if (v2 > s_v[tid] || (v2 == s_v[tid] && i2 < s_i[tid])) s_v[tid] = v2, s_i[tid] = i2;
    }
    __syncthreads();
  }
  if (tid == 0) p.partial[((size_t)row * p.nb + b) * p.nwg + blockIdx.x] = make_float4(s_v[0], __uint_as_float(s_i[0]), s_sum[0] + s_sum[1], 0.f);
}

// find_peak's loop over the blocks and its threshold (refsignal_dl_sync.c:204-228)
__global__ __launch_bounds__(64) void meas_decide_kernel(MeasParams p)
{
  const uint32_t row = blockIdx.x * 64 + threadIdx.x;
  if (row >= p.rows) return;
  float    peak_value = 0.f, rms_avg = 0.f;
  uint32_t peak_idx = 0;
  for (uint32_t b = 0; b < p.nb; b++) {
    const float4* part = p.partial + ((size_t)row * p.nb + b) * p.nwg;
    float         mx = -INFINITY, sum = 0.f;
    uint32_t      imax = NO_INDEX;
    for (uint32_t w = 0; w < p.nwg; w++) {
      const float4   t  = part[w];
      const uint32_t ti = __float_as_uint(t.y);
      if (t.x > mx || (t.x == mx && ti < imax)) mx = t.x, imax = ti;
      sum += t.z;
    }
    const float peak = sqrtf(mx), rms = sqrtf(sum / (float)p.L);
    rms_avg += rms;
    if (peak > peak_value) peak_value = peak, peak_idx = imax + b * p.L;
  }
  rms_avg /= (float)p.nb;
  MeasDecision d;
  d.found = peak_value > rms_avg * p.thr ? 1 : 0, d.peak_idx = peak_idx, d.peak = peak_value, d.rms = rms_avg;
  p.dec[row] = d;
}

// srslte_refsignal_dl_sync_measure_sf (refsignal_dl_sync.c:303-355) of subframe j of a row's measurement loop (:260-271)
__global__ __launch_bounds__(SF_THREADS) void meas_sf_kernel(MeasParams p, const cf32* __restrict__ in)
{
  __shared__ float   s_red[12][SF_THREADS / 64];
  const uint32_t     j = blockIdx.x, row = blockIdx.y, tid = threadIdx.x, N = p.N, L = p.L;
  const MeasDecision d = p.dec[row];
  if (!d.found) return;
  const uint32_t n = d.peak_idx % L + j * L;
  if (n + L > p.nof_sf * L) return; // n < nsamples - sf_len + 1
  const uint32_t sf_idx = ((20 - d.peak_idx / L) % 10 + j) % 10, cap = row / p.n_cells, cell = row % p.n_cells;
  const cf32*    x      = in + (size_t)cap * p.in_stride + n;
  const cf32*    y      = p.seq + ((size_t)cell * 10 + sf_idx) * L;
  float          acc[12];
#pragma unroll
  for (int l = 0; l < 4; l++) {
    // the FFT window of CRS symbol l of port 0: symbols 0, 4, 7, 11 (:322-327)
    const uint32_t symbidx = (l & 1) ? (l / 2 + 1) * 7 - 3 : (l / 2) * 7;
    const uint32_t offset  = p.cp0 + (N + p.cp1) * symbidx + (l >= 2 ? p.cp0 - p.cp1 : 0u);
    cf32           c       = make_float2(0.f, 0.f);
    float          pw      = 0.f;
    for (uint32_t i = tid; i < N; i += SF_THREADS) {
      const cf32 a = x[offset + i];
      c            = cadd(c, cmulconj(a, y[offset + i]));
      pw += a.x * a.x + a.y * a.y;
    }
    acc[3 * l] = c.x, acc[3 * l + 1] = c.y, acc[3 * l + 2] = pw;
  }
#pragma unroll
  for (int k = 0; k < 12; k++) {
    const float v = wave_sum(acc[k]);
    if (tid % 64 == 0) s_red[k][tid / 64] = v;
  }
  __syncthreads();
  if (tid != 0) return;
  cf32  corr[4];
  float rsrp_lin = 0.f, rssi_lin = 0.f;
#pragma unroll
  for (int l = 0; l < 4; l++) {
    float t[3];
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = (s_red[3 * l + k][0] + s_red[3 * l + k][1]) + (s_red[3 * l + k][2] + s_red[3 * l + k][3]);
    corr[l] = make_float2(t[0], t[1]);
    rsrp_lin += t[0] * t[0] + t[1] * t[1];
    rssi_lin += t[2];
  }
  const cf32 z0 = cmulconj(corr[2], corr[0]), z1 = cmulconj(corr[3], corr[1]);
  float      cfo = 0.f;
  cfo += (float)((double)atan2f(z0.y, z0.x) / (2.0f * M_PI * 7.5f) * 15000.0f);
  cfo += (float)((double)atan2f(z1.y, z1.x) / (2.0f * M_PI * 7.5f) * 15000.0f);
  cfo /= 2;
  p.sfm[(size_t)row * p.max_sf + j] = make_float4(rsrp_lin * 4.f, (float)p.P * rssi_lin / 4.f * 7.41f, cfo, 0.f);
}

// the averages and dB figures of srslte_refsignal_dl_sync_run (refsignal_dl_sync.c:273-299)
__global__ __launch_bounds__(64) void meas_finish_kernel(MeasParams p, srslte_hip_meas_res_t* __restrict__ res)
{
  const uint32_t row = blockIdx.x * 64 + threadIdx.x;
  if (row >= p.rows) return;
  const MeasDecision    d = p.dec[row];
  const MeasCellDesc    cd = cell_desc(p.P);
  srslte_hip_meas_res_t o;
  o.found = d.found, o.peak_value = d.peak, o.rms_avg = d.rms;
  o.cell_id = __float_as_uint(p.desc[(size_t)(row % p.n_cells) * cd.stride + cd.id]), o.capture = row / p.n_cells;
  o.reserved[0] = o.reserved[1] = 0;
  if (d.found) {
    const uint32_t n0 = d.peak_idx % p.L;
    uint32_t       cnt = 0;
    float          rsrp = 0.f, rssi = 0.f, cfo = 0.f;
    for (uint32_t j = 0; n0 + j * p.L + p.L <= p.nof_sf * p.L; j++) {
      const float4 t = p.sfm[(size_t)row * p.max_sf + j];
      rsrp += t.x, rssi += t.y, cfo += t.z;
      cnt++;
    }
    if (cnt) rsrp /= cnt, rssi /= cnt, cfo /= cnt;
    o.peak_index = d.peak_idx, o.sf_idx = (20 - d.peak_idx / p.L) % 10, o.nof_sf = cnt;
    o.rsrp_lin = rsrp, o.rssi_lin = rssi, o.cfo_Hz = cfo;
    o.rsrp_dBfs = 10.0f * log10f(rsrp) + 30.0f;
    o.rssi_dBfs = 10.0f * log10f(rssi) + 30.0f;
    o.rsrq_dB   = 10.0f * log10f((float)p.P) + o.rsrp_dBfs - o.rssi_dBfs;
  } else {
    o.peak_index = NO_INDEX, o.sf_idx = 0, o.nof_sf = 0;
    o.rsrp_lin = o.rssi_lin = o.rsrp_dBfs = o.rssi_dBfs = o.rsrq_dB = o.cfo_Hz = NAN;
  }
  res[row] = o;
}

} // namespace

struct srslte_hip_meas_s {
  srslte_hip_meas_cfg_t cfg;
  MeasParams            p;
  uint32_t              n_cells = 0;
  srslte_hip_ofdm_t*    ofdm    = nullptr;
  DescStage             desc;
  DevBuf<cf32>          tw2, grid, seq, hspec, xspec, work;
  DevBuf<float4>        partial, sfm;
  DevBuf<MeasDecision>  dec;
  ~srslte_hip_meas_s() { srslte_hip_ofdm_destroy(ofdm); }
};

extern "C" {

srslte_hip_meas_t* srslte_hip_meas_create(const srslte_hip_meas_cfg_t* cfg)
{
  if (!meas_cfg_valid(cfg)) {
    hip_log("[srslte_hip] meas: invalid configuration (normal CP only; see phy_hip.h for the sizes)\n");
    return nullptr;
  }
  auto* q = new srslte_hip_meas_s();
  q->cfg  = *cfg;
  const uint32_t N = meas_symbol_sz(cfg), L = 15 * N, P = cfg->nof_prb;
  const uint32_t nbmax = cfg->max_sf - 1 < MAX_BLOCKS ? cfg->max_sf - 1 : MAX_BLOCKS, nwg = N / COL_THREADS;
  const size_t   rows = (size_t)cfg->max_captures * cfg->max_cells, M = 30 * (size_t)N;
  MeasParams&    p = q->p;
  p.N = N, p.L = L, p.P = P, p.cp0 = (uint32_t)lte_cp_len_norm(0, (int)N), p.cp1 = (uint32_t)lte_cp_len_norm(1, (int)N);
  p.nwg = nwg, p.max_sf = cfg->max_sf, p.thr = cfg->threshold == 0.f ? 5.5f : cfg->threshold;
  std::vector<cf32> tw2;
  meas_twiddles(N, tw2);
  q->ofdm = srslte_hip_ofdm_create_sz((int)P, (int)N, 1, 0);
  if (!q->ofdm || q->tw2.upload(tw2) || q->grid.alloc((size_t)cfg->max_cells * 10 * 14 * 12 * P) || q->seq.alloc((size_t)cfg->max_cells * 10 * L) ||
      q->hspec.alloc(cfg->max_cells * M) || q->xspec.alloc((size_t)cfg->max_captures * nbmax * M) || q->work.alloc(rows * nbmax * M) ||
      q->partial.alloc(rows * nbmax * nwg) || q->sfm.alloc(rows * cfg->max_sf) || q->dec.alloc(rows) ||
      q->desc.init(sizeof(float) * cell_desc(P).stride * cfg->max_cells)) {
    hip_log("[srslte_hip] meas: device allocation failed\n");
    delete q;
    return nullptr;
  }
  p.tw2 = q->tw2, p.seq = q->seq, p.desc = q->desc.dev<float>(), p.partial = q->partial, p.dec = q->dec, p.sfm = q->sfm;
  return q;
}

void srslte_hip_meas_destroy(srslte_hip_meas_t* q) { delete q; }

int srslte_hip_meas_set_cells(srslte_hip_meas_t* q, const uint16_t* cell_ids, uint32_t n_cells, void* stream)
{
  if (!q || !cell_ids || n_cells == 0 || n_cells > q->cfg.max_cells) return SRSLTE_ERROR_INVALID_INPUTS;
  for (uint32_t k = 0; k < n_cells; k++)
    if (cell_ids[k] > 503) return SRSLTE_ERROR_INVALID_INPUTS;
  hipStream_t        st = (hipStream_t)stream;
  const MeasParams&  p  = q->p;
  const MeasCellDesc d  = cell_desc(p.P);
  float*             h  = nullptr;
  if (int r = q->desc.begin(&h)) return r;
  std::vector<cf32> pil;
  for (uint32_t k = 0; k < n_cells; k++) {
    float* blk = h + (size_t)k * d.stride;
    lte_crs_values(cell_ids[k], p.P, true, pil); // ports 0 and 1 share the first [10][4][2 P] values
    memcpy(blk, pil.data(), sizeof(cf32) * 10 * 4 * 2 * p.P);
    sync_pss_seq(cell_ids[k] % 3, reinterpret_cast<cf32*>(blk + d.pss));
    meas_sss_seq(cell_ids[k], blk + d.sss, blk + d.sss + 62);
    const uint32_t id = cell_ids[k];
    memcpy(blk + d.id, &id, sizeof(id));
    blk[d.id + 1] = blk[d.id + 2] = blk[d.id + 3] = 0.f;
  }
  if (int r = q->desc.commit(sizeof(float) * d.stride * n_cells, st)) return r;
  q->n_cells = n_cells;
  HIP_TRY(hipMemsetAsync(q->grid.get(), 0, sizeof(cf32) * n_cells * 10 * 14 * 12 * p.P, st));
  hipLaunchKernelGGL(meas_fill_kernel, dim3(10, n_cells), dim3(256), 0, st, q->desc.dev<float>(), q->grid.get(), p.P);
  LAUNCH_CHECK();
  if (int r = srslte_hip_ofdm_tx_sf_batch(q->ofdm, q->grid.get(), q->seq.get(), (int)(10 * n_cells), st)) return r;
  const size_t nseq = (size_t)n_cells * 10 * p.L;
  hipLaunchKernelGGL(meas_scale_kernel, dim3((unsigned)((nseq + 255) / 256 < 4096 ? (nseq + 255) / 256 : 4096)), dim3(256), 0, st, q->seq.get(), nseq,
                     1.0f / (float)(8 * p.P));
  LAUNCH_CHECK();
  // the filter spectrum of find_peak (:195-198): replica 0 followed by L zeros, forward; its 1 / sqrt(2 L) is in the inverse's scale
  hipLaunchKernelGGL(meas_col_fwd_kernel, dim3(p.nwg, 1, n_cells), dim3(COL_THREADS), 0, st, (const cf32*)q->seq.get(), (size_t)10 * p.L, p.L, p.N, 15u,
                     p.tw2, q->work.get());
  LAUNCH_CHECK();
  return srslte_hip_dft_batch(q->work.get(), q->hspec.get(), (int)p.N, (int)(30 * n_cells), (int)p.N, (int)p.N, 1, 1.0f, st);
}

int srslte_hip_meas_run_batch(srslte_hip_meas_t* q, const void* d_in, size_t in_stride, uint32_t nof_sf, uint32_t n_captures,
                              srslte_hip_meas_res_t* d_res, void* stream)
{
  if (!q || !d_in || !d_res || q->n_cells == 0) return SRSLTE_ERROR_INVALID_INPUTS;
  if (int r = srslte_hip_meas_check(&q->cfg, in_stride, nof_sf, n_captures, q->n_cells)) return r;
  if (n_captures == 0) return SRSLTE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  MeasParams  p  = q->p;
  p.nb = nof_sf - 1 < MAX_BLOCKS ? nof_sf - 1 : MAX_BLOCKS, p.n_cells = q->n_cells, p.rows = n_captures * q->n_cells, p.nof_sf = nof_sf;
  p.in_stride = in_stride;
  // forward once per (capture, block) ...
  hipLaunchKernelGGL(meas_col_fwd_kernel, dim3(p.nwg, p.nb, n_captures), dim3(COL_THREADS), 0, st, (const cf32*)d_in, in_stride, p.L, p.N, 30u, p.tw2,
                     q->work.get());
  LAUNCH_CHECK();
  if (int r = srslte_hip_dft_batch(q->work.get(), q->xspec.get(), (int)p.N, (int)(30 * p.nb * n_captures), (int)p.N, (int)p.N, 1, 1.0f, st)) return r;
  // ... inverse per (capture, cell, block): normalised forward transforms of input and filter, unnormalised backward (convolution.c:58-60)
  if (int r = fft_rows30_mulconj_inverse(q->xspec.get(), q->hspec.get(), p.tw2, q->work.get(), (int)p.N, p.nb, n_captures, p.n_cells,
                                         1.0f / (float)(2 * p.L), st))
    return r;
  hipLaunchKernelGGL(meas_col_inv_kernel, dim3(p.nwg, p.nb, p.rows), dim3(COL_THREADS), 0, st, p, (const cf32*)q->work.get());
  LAUNCH_CHECK();
  hipLaunchKernelGGL(meas_decide_kernel, dim3((p.rows + 63) / 64), dim3(64), 0, st, p);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(meas_sf_kernel, dim3(nof_sf, p.rows), dim3(SF_THREADS), 0, st, p, (const cf32*)d_in);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(meas_finish_kernel, dim3((p.rows + 63) / 64), dim3(64), 0, st, p, d_res);
  LAUNCH_CHECK();
  return SRSLTE_SUCCESS;
}

int srslte_hip_meas_replicas(srslte_hip_meas_t* q, uint32_t cell, void* h_seq)
{
  if (!q || !h_seq || cell >= q->n_cells) return SRSLTE_ERROR_INVALID_INPUTS;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(h_seq, q->seq.get() + (size_t)cell * 10 * q->p.L, sizeof(cf32) * 10 * q->p.L, hipMemcpyDeviceToHost));
  return SRSLTE_SUCCESS;
}

} // extern "C"
