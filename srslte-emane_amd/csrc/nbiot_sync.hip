// NB-IoT synchronisation for gfx950 (include/srslte_hip/phy_hip.h, "NB-IoT synchronisation"): one srslte_sync_nbiot_find per item on a track kept
// on the device, and srslte_nsss_sync_find for a batch of captures, by the structure of the two replicas (11 symbols of 11 / 12 subcarriers,
// two CP classes) instead of the reference's generic FFT convolution.
//   nbiot_npss_slide_kernel   grid (tile of 256 positions, CP class, item): the sliding correlation of the circularly extended, CFO-rotated
//                             frame with the class's 137 / 138 conjugated taps; input tile and taps in LDS, a lane per position
//   nbiot_npss_comb_kernel    grid (tile of 256 lags, item): c[n] = sum_i sign_i W_cls(i)[n + s_i] (frame_size < 128: the 128-tap dot products),
//                             |c|^2, the average into the track's row, the tile's (maximum, first index)
//   nbiot_npss_decide_kernel  one workgroup per item: the peak over the tiles, the side lobe, the CFO stage on the uncorrected item, the track's
//                             mean_cfo and the row
//   nbiot_nsss_slide_kernel   grid (tile of 256 positions, CP class x subcarrier, item): Y_cls,sc[m]
//   nbiot_nsss_prod_kernel    grid (tile of 64 lags, row of up to 64 cell ids): the [ids x 132] x [132 x lags] complex product in fp32 FMAs, the
//                             table and Y through LDS a symbol (12 rows) at a time, 4 x 4 outputs per lane; writes each id's (maximum of |c|,
//                             first index) of the tile
//   nbiot_nsss_decide_kernel  one workgroup per item: every id's peak over the tiles, the first maximum over the ids, the row, and the |c| row
//                             of the row's id for the debug entry
//   nbiot_track_reset_kernel, nbiot_track_set_cfo_kernel
// The rotated load, the workgroup reductions, the side lobe and the CP correlation are search_dev.hpp's, shared with sync.hip.
// The tables come from nbiot_sync_host.cpp.
#include "common.hpp"
#include "dev_buf.hpp"
#include "phy_hip_internal.hpp"
#include "search_dev.hpp"
#include <math.h>
#include <string.h>

namespace {

constexpr int      NB_THREADS = 256;
constexpr uint32_t NB_TILE    = 256;
constexpr uint32_t NB_TAPS    = 138;                          // 128 + CP 10, the longer class
constexpr uint32_t NB_HALO    = NB_TILE + NB_TAPS - 1;        // input samples of a tile of positions
constexpr uint32_t NB_LAST    = 137 * 10 + 1;                 // s_10: start of the last symbol in the replica
constexpr uint32_t NB_LEN     = SRSLTE_HIP_NBIOT_REPLICA_LEN; // 1508
constexpr uint32_t NB_PCI     = SRSLTE_HIP_NBIOT_NUM_PCI;
constexpr uint32_t NS_IN      = SRSLTE_HIP_NBIOT_NSSS_IN_LEN; // 3840
constexpr uint32_t NS_L       = NS_IN + NB_LEN;               // 5348
constexpr uint32_t NS_NOUT    = SRSLTE_HIP_NBIOT_NSSS_NOUT;   // 5346
constexpr uint32_t NS_PT      = 64;                           // ids and lags of a product tile
constexpr uint32_t NS_NT      = (NS_NOUT + NS_PT - 1) / NS_PT; // 84 lag tiles
constexpr uint32_t NS_MY      = 27 * NB_TILE;                 // 6912 >= 84 x 64 + s_10: positions of Y a product tile may read
constexpr uint32_t NS_IDROWS  = (NB_PCI + NS_PT - 1) / NS_PT; // 8 product rows of an exhaustive item
constexpr uint32_t CFO_OFFSET = 548, CFO_NSAMP = 823;         // SRSLTE_NPSS_CFO_OFFSET, SRSLTE_NPSS_CFO_NUM_SAMPS

__device__ __forceinline__ uint32_t sym_start(uint32_t i) { return 137u * i + (i > 4u ? 1u : 0u); }

struct NpssRow {
  uint32_t track, find_offset;
};

struct NpssParams {
  uint32_t frame_size, L, nout, conv_len, mw, ntiles, short_branch, cfo_enable, cp_offsets;
  float    threshold, alpha, cfo_alpha; // alpha: 0 = no averaging
  size_t   in_stride;
  const cf32 *taps, *head, *shift2;
  cf32*    w;        // [item][2][mw]
  float*   avg;      // [track][nout]
  float*   mean_cfo; // [track]
  float2*  tile_max; // [item][ntiles]: value, index as bits
};

struct NsssRow {
  uint32_t item, id0, nid, pad;
};

struct NsssParams {
  size_t      in_stride;
  float       threshold;
  const cf32 *tw, *seq; // [2][12][138], [132][504]
  cf32*       y;        // [item][2][12][NS_MY]
  float2*     tile_max; // [item][504][NS_NT]
  float*      peak_values; // [item][504]
  float*      abs_row;  // [item][NS_NOUT]
};

// W_cls[m] = sum_t xe[m + t] taps[cls][t], xe the frame continued circularly over L with zeros from frame_size on, rotated by the track's mean
__global__ __launch_bounds__(NB_THREADS) void nbiot_npss_slide_kernel(NpssParams p, const NpssRow* __restrict__ rows, const cf32* __restrict__ in)
{
  __shared__ cf32 s_x[NB_HALO];
  __shared__ cf32 s_h[NB_TAPS];
  const uint32_t  item = blockIdx.z, cls = blockIdx.y, m0 = blockIdx.x * NB_TILE, tid = threadIdx.x, ntap = 137u + cls;
  const NpssRow   r    = rows[item];
  const cf32*     x    = in + (size_t)item * p.in_stride;
  const float     f    = -p.mean_cfo[r.track] / 128.f; // sync_nbiot.c:206
  for (uint32_t u = tid; u < NB_HALO; u += NB_THREADS) {
    const uint32_t j = (m0 + u) % p.L;
    s_x[u] = j < p.frame_size ? ld_rot(x, r.find_offset + j, f) : make_float2(0.f, 0.f);
  }
  if (tid < NB_TAPS) s_h[tid] = p.taps[cls * NB_TAPS + tid];
  __syncthreads();
  const uint32_t m = m0 + tid;
  if (m >= p.mw) return;
  cf32 acc = make_float2(0.f, 0.f);
  for (uint32_t t = 0; t < ntap; t++) acc = cadd(acc, cmul(s_x[tid + t], s_h[t]));
  p.w[((size_t)item * 2 + cls) * p.mw + m] = acc;
}

__global__ __launch_bounds__(NB_THREADS) void nbiot_npss_comb_kernel(NpssParams p, const NpssRow* __restrict__ rows, const cf32* __restrict__ in)
{
  __shared__ float    s_v[NB_THREADS];
  __shared__ uint32_t s_i[NB_THREADS];
  const uint32_t      item = blockIdx.y, tid = threadIdx.x, n = blockIdx.x * NB_TILE + tid;
  const NpssRow       r    = rows[item];
  float               best = -INFINITY;
  uint32_t            bi   = NO_INDEX;
  if (n < p.nout) {
    cf32 c = make_float2(0.f, 0.f);
    if (!p.short_branch) {
      const cf32* w = p.w + (size_t)item * 2 * p.mw;
      for (uint32_t i = 0; i < 11; i++) {
        const cf32 v = w[(i == 4 ? p.mw : 0u) + n + sym_start(i)];
        c = ((0x230u >> i) & 1u) ? csub(c, v) : cadd(c, v); // factor_lut (npss.c:42): symbols 4, 5 and 9 are negated
      }
    } else { // npss.c:266-269: the replica's first 128 samples, not conjugated
      const cf32* x = in + (size_t)item * p.in_stride;
      const float f = -p.mean_cfo[r.track] / 128.f;
      for (uint32_t t = 0; t < 128; t++) c = cadd(c, cmul(p.head[t], ld_rot(x, r.find_offset + n + t, f)));
    }
    float        v = c.x * c.x + c.y * c.y;
    float* const a = p.avg + (size_t)r.track * p.nout + n;
    if (p.alpha != 0.f) v = v * p.alpha + *a * (1 - p.alpha); // npss.c:278-282
    *a   = v;
    best = v, bi = n;
  }
  block_argmax<NB_THREADS>(best, bi, s_v, s_i);
  if (tid == 0) p.tile_max[(size_t)item * p.ntiles + blockIdx.x] = make_float2(best, __uint_as_float(bi));
}

__global__ __launch_bounds__(NB_THREADS) void nbiot_npss_decide_kernel(NpssParams p, const NpssRow* __restrict__ rows, const cf32* __restrict__ in,
                                                                      srslte_hip_nbiot_npss_res_t* __restrict__ res)
{
  __shared__ float    s_v[NB_THREADS];
  __shared__ uint32_t s_i[NB_THREADS];
  __shared__ cf32     s_corr[128];
  const uint32_t      item = blockIdx.x, tid = threadIdx.x;
  const NpssRow       r    = rows[item];
  const float*        avg  = p.avg + (size_t)r.track * p.nout;
  const uint32_t      nout = p.nout, CL = p.conv_len;
  // the buffer behind the nout averaged values is zeros (npss.c:62-82, :384-390)
  auto av = [&](uint32_t j) { return j < nout ? avg[j] : 0.f; };

  float    best = -INFINITY;
  uint32_t pk   = NO_INDEX;
  for (uint32_t t = tid; t < p.ntiles; t += NB_THREADS) {
    const float2   m = p.tile_max[(size_t)item * p.ntiles + t];
    const uint32_t i = __float_as_uint(m.y);
    if (i != NO_INDEX && (m.x > best || (m.x == best && i < pk))) best = m.x, pk = i;
  }
  block_argmax<NB_THREADS>(best, pk, s_v, s_i);
  if (pk == NO_INDEX) pk = 0; // nothing compared greater than -inf: srslte_vec_max_fi answers index 0
  const float peak = av(pk);

  const float psr = peak / side_lobe<NB_THREADS>(av, pk, CL, s_v, s_i); // npss.c:301-343

  // sync_nbiot.c:224-242
  const bool cfo_run = p.cfo_enable && (uint64_t)pk + CFO_OFFSET + CFO_NSAMP + 128 < p.frame_size;
  float      cfo     = NAN;
  if (cfo_run) { // uniform over the workgroup
    const cf32* x   = in + (size_t)item * p.in_stride + pk + CFO_OFFSET;
    auto        ld  = [&](uint32_t j) { return j < CFO_NSAMP ? cmul(p.shift2[j], x[j]) : x[j]; };
    float       bv  = -INFINITY;
    uint32_t    bi  = NO_INDEX;
    if (tid < p.cp_offsets) { // cp.c:61-77
      const cf32 acc = cp_synch_at(ld, 128, 9, 6, tid);
      s_corr[tid] = acc;
      bv = acc.x * acc.x + acc.y * acc.y, bi = tid;
    }
    block_argmax<NB_THREADS>(bv, bi, s_v, s_i);
    const cf32 c = s_corr[bi == NO_INDEX ? 0u : bi];
    cfo          = (float)(-atan2((double)c.y, (double)c.x) / M_PI / 2); // sync_nbiot.c:263
  }
  if (tid == 0) {
    float mean = p.mean_cfo[r.track];
    if (cfo_run) {
      mean                = p.cfo_alpha * cfo + (1 - p.cfo_alpha) * mean; // SRSLTE_VEC_EMA
      p.mean_cfo[r.track] = mean;
    }
    srslte_hip_nbiot_npss_res_t o;
    o.ret = psr >= p.threshold ? 1 : 0, o.peak_pos = pk, o.peak_value = psr, o.corr_peak = peak, o.cfo = cfo, o.mean_cfo = mean;
    o.reserved[0] = o.reserved[1] = 0;
    res[item] = o;
  }
}

__global__ __launch_bounds__(NB_THREADS) void nbiot_track_reset_kernel(float* avg, float* mean_cfo, uint32_t first, uint32_t nout)
{
  const uint32_t k = first + blockIdx.x;
  for (uint32_t i = threadIdx.x; i < nout; i += NB_THREADS) avg[(size_t)k * nout + i] = 0.f;
  if (threadIdx.x == 0) mean_cfo[k] = 0.f;
}

__global__ __launch_bounds__(64) void nbiot_track_set_cfo_kernel(float* mean_cfo, const float* __restrict__ v, uint32_t first, uint32_t n)
{
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) mean_cfo[first + i] = v[i];
}

// Y_cls,sc[m] = sum_t xe[m + t] tw[cls][sc][t], xe the 3840 samples continued circularly over 5348 with zeros from 3840 on
__global__ __launch_bounds__(NB_THREADS) void nbiot_nsss_slide_kernel(NsssParams p, const cf32* __restrict__ in)
{
  __shared__ cf32 s_x[NB_HALO];
  __shared__ cf32 s_h[NB_TAPS];
  const uint32_t  item = blockIdx.z, row = blockIdx.y, m0 = blockIdx.x * NB_TILE, tid = threadIdx.x, ntap = 137u + row / 12u;
  const cf32*     x    = in + (size_t)item * p.in_stride;
  for (uint32_t u = tid; u < NB_HALO; u += NB_THREADS) {
    uint32_t j = m0 + u; // < NS_MY + 393 < 2 NS_L
    if (j >= NS_L) j -= NS_L;
    s_x[u] = j < NS_IN ? x[j] : make_float2(0.f, 0.f);
  }
  if (tid < NB_TAPS) s_h[tid] = p.tw[row * NB_TAPS + tid];
  __syncthreads();
  cf32 acc = make_float2(0.f, 0.f);
  for (uint32_t t = 0; t < ntap; t++) acc = cadd(acc, cmul(s_x[tid + t], s_h[t]));
  p.y[((size_t)item * 24 + row) * NS_MY + m0 + tid] = acc; // grid.x NS_MY / 256 tiles: every position is in range
}

// c_id[n] = sum_{i, sc} seq[12 i + sc][id] Y_cls(i),sc[n + s_i] for the row's ids and the tile's 64 lags; lane (ty, tx) holds ids ty + 16 a and lags
// tx + 16 b, a, b < 4: LDS reads of consecutive lanes are consecutive (lags) or one address per 16 lanes (ids)
__global__ __launch_bounds__(NB_THREADS) void nbiot_nsss_prod_kernel(NsssParams p, const NsssRow* __restrict__ rows)
{
  __shared__ cf32 s_a[12][NS_PT];
  __shared__ cf32 s_b[12][NS_PT];
  const NsssRow   r   = rows[blockIdx.y];
  const uint32_t  tid = threadIdx.x, tx = tid % 16, ty = tid / 16, n0 = blockIdx.x * NS_PT;
  const cf32*     y   = p.y + (size_t)r.item * 24 * NS_MY;
  float           ax[4][4], ay[4][4];
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) ax[a][b] = 0.f, ay[a][b] = 0.f;
  for (uint32_t i = 0; i < 11; i++) {
    const uint32_t yrow = (i == 4 ? 12u : 0u), s = n0 + sym_start(i);
    __syncthreads();
    for (uint32_t e = tid; e < 12 * NS_PT; e += NB_THREADS) {
      const uint32_t sc = e / NS_PT, k = e % NS_PT;
      s_a[sc][k] = k < r.nid ? p.seq[(size_t)(12 * i + sc) * NB_PCI + r.id0 + k] : make_float2(0.f, 0.f);
      s_b[sc][k] = y[(size_t)(yrow + sc) * NS_MY + s + k]; // s + k <= 83 x 64 + 1371 + 63 < NS_MY
    }
    __syncthreads();
    if (ty < r.nid) { // a row of one id (a known cell) works in its first 16 lanes only
#pragma unroll
      for (uint32_t sc = 0; sc < 12; sc++) {
        cf32 va[4], vb[4];
#pragma unroll
        for (int a = 0; a < 4; a++) va[a] = s_a[sc][ty + 16 * a];
#pragma unroll
        for (int b = 0; b < 4; b++) vb[b] = s_b[sc][tx + 16 * b];
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
          for (int b = 0; b < 4; b++) {
            ax[a][b] = fmaf(va[a].x, vb[b].x, ax[a][b]);
            ax[a][b] = fmaf(-va[a].y, vb[b].y, ax[a][b]);
            ay[a][b] = fmaf(va[a].x, vb[b].y, ay[a][b]);
            ay[a][b] = fmaf(va[a].y, vb[b].x, ay[a][b]);
          }
      }
    }
  }
  // |c| (srslte_vec_abs_cf), per id the first maximum over the tile's lags: over the lane's four, then over the 16 lanes that share ty
#pragma unroll
  for (int a = 0; a < 4; a++) {
    float    best = -INFINITY;
    uint32_t bi   = NO_INDEX;
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const uint32_t n = n0 + tx + 16 * b;
      const float    v = sqrtf(ax[a][b] * ax[a][b] + ay[a][b] * ay[a][b]);
      if (n < NS_NOUT && v > best) best = v, bi = n; // lags ascend with b
    }
    for (int o = 8; o > 0; o >>= 1) {
      const float    v2 = __shfl_xor(best, o, 16);
      const uint32_t i2 = __shfl_xor(bi, o, 16);
      if (v2 > best || (v2 == best && i2 < bi)) best = v2, bi = i2;
    }
    const uint32_t k = ty + 16 * a;
    if (tx == 0 && k < r.nid) p.tile_max[((size_t)r.item * NB_PCI + r.id0 + k) * NS_NT + blockIdx.x] = make_float2(best, __uint_as_float(bi));
  }
}

__global__ __launch_bounds__(NB_THREADS) void nbiot_nsss_decide_kernel(NsssParams p, const int32_t* __restrict__ cell_ids,
                                                                      srslte_hip_nbiot_nsss_res_t* __restrict__ res)
{
  __shared__ float    s_v[NB_THREADS];
  __shared__ uint32_t s_i[NB_THREADS];
  __shared__ uint32_t s_pos[NB_PCI];
  const uint32_t      item = blockIdx.x, tid = threadIdx.x;
  const int32_t       want = cell_ids[item];
  float               best = -INFINITY;
  uint32_t            bid  = NO_INDEX;
  for (uint32_t id = tid; id < NB_PCI; id += NB_THREADS) {
    float    v   = 0.f;
    uint32_t pos = 0;
    if (want < 0 || (uint32_t)want == id) {
      const float2* t = p.tile_max + ((size_t)item * NB_PCI + id) * NS_NT;
      v               = -INFINITY;
      for (uint32_t k = 0; k < NS_NT; k++) { // tiles ascend: strict > keeps the first maximum
        const float2 m = t[k];
        if (m.x > v) v = m.x, pos = __float_as_uint(m.y);
      }
      if (v > best) best = v, bid = id; // ids ascend per lane
    }
    p.peak_values[(size_t)item * NB_PCI + id] = v;
    s_pos[id]                                 = pos;
  }
  block_argmax<NB_THREADS>(best, bid, s_v, s_i); // nsss.c:252: the first maximum of peak_values
  if (bid == NO_INDEX) bid = want < 0 ? 0u : (uint32_t)want;
  if (tid == 0) {
    const float v = p.peak_values[(size_t)item * NB_PCI + bid];
    srslte_hip_nbiot_nsss_res_t o;
    o.found = v > p.threshold ? 1 : 0, o.cell_id = (int32_t)bid, o.peak_value = v, o.peak_pos = s_pos[bid], o.sfn_partial = 0;
    o.reserved[0] = o.reserved[1] = o.reserved[2] = 0;
    res[item] = o;
  }
  // the |c| row of that id for srslte_hip_nbiot_nsss_debug
  const cf32* y = p.y + (size_t)item * 24 * NS_MY;
  for (uint32_t n = tid; n < NS_NOUT; n += NB_THREADS) {
    cf32 c = make_float2(0.f, 0.f);
    for (uint32_t i = 0; i < 11; i++) {
      const cf32* yr = y + (size_t)(i == 4 ? 12u : 0u) * NS_MY + n + sym_start(i);
      for (uint32_t sc = 0; sc < 12; sc++) c = cadd(c, cmul(p.seq[(size_t)(12 * i + sc) * NB_PCI + bid], yr[(size_t)sc * NS_MY]));
    }
    p.abs_row[(size_t)item * NS_NOUT + n] = sqrtf(c.x * c.x + c.y * c.y);
  }
}

} // namespace

struct srslte_hip_nbiot_sync_s {
  srslte_hip_nbiot_sync_cfg_t cfg;
  NpssParams                  np;
  NsssParams                  ns;
  DescStage                   desc; // a call's rows: NpssRow [n], NsssRow [8 n] followed by the ids [n], or mean_cfo values [n]
  DevBuf<cf32>                taps, head, shift2, tw, seq, w, y;
  DevBuf<float>               avg, mean_cfo, peak_values, abs_row;
  DevBuf<float2>              np_tile, ns_tile;
  uint32_t                    last_nsss = 0; // items of the last NSSS call
};

extern "C" {

srslte_hip_nbiot_sync_t* srslte_hip_nbiot_sync_create(const srslte_hip_nbiot_sync_cfg_t* cfg)
{
  if (!nbiot_cfg_valid(cfg)) {
    hip_log("[srslte_hip] nbiot sync: invalid configuration (fft_size must be 128; see phy_hip.h for the sizes)\n");
    return nullptr;
  }
  auto* q = new srslte_hip_nbiot_sync_s();
  q->cfg  = *cfg;
  NbiotTables t;
  nbiot_tables(t);
  NpssParams& p  = q->np;
  p.frame_size   = cfg->frame_size;
  p.short_branch = cfg->frame_size < 128 ? 1u : 0u;
  p.L            = cfg->frame_size + NB_LEN;
  p.nout         = srslte_hip_nbiot_npss_nout(cfg->frame_size);
  p.conv_len     = p.nout + 1;
  p.mw           = p.short_branch ? 1u : p.nout + NB_LAST; // n + s_i < nout + s_10
  p.ntiles       = (p.nout + NB_TILE - 1) / NB_TILE;
  if (p.ntiles == 0) p.ntiles = 1; // frame_size 1: no value enters the maximum
  p.cfo_enable = cfg->cfo_enable ? 1u : 0u, p.cp_offsets = cfg->max_offset < 128 ? cfg->max_offset : 128u;
  p.threshold       = cfg->threshold == 0.f ? 5.0f : cfg->threshold;
  const float alpha = cfg->npss_ema_alpha == 0.f ? 0.2f : cfg->npss_ema_alpha;
  p.alpha           = (alpha < 1.0f && alpha > 0.0f) ? alpha : 0.f; // npss.c:278
  p.cfo_alpha       = cfg->cfo_ema_alpha == 0.f ? 0.1f : cfg->cfo_ema_alpha;
  NsssParams& s     = q->ns;
  s.threshold       = cfg->nsss_threshold == 0.f ? 2.0f : cfg->nsss_threshold;
  const size_t M = cfg->max_items, rows_bytes = sizeof(NsssRow) * NS_IDROWS * M + sizeof(int32_t) * M;
  const size_t navg = (size_t)cfg->n_tracks * (p.nout ? p.nout : 1);
  if (q->taps.upload(t.npss_taps) || q->head.upload(t.npss_head) || q->shift2.upload(t.shift2) || q->tw.upload(t.nsss_tw) || q->seq.upload(t.nsss_seq) ||
      q->w.alloc(M * 2 * p.mw) || q->y.alloc(M * 24 * NS_MY) || q->avg.alloc(navg) || q->mean_cfo.alloc(cfg->n_tracks) ||
      q->peak_values.alloc(M * NB_PCI) || q->abs_row.alloc(M * NS_NOUT) || q->np_tile.alloc(M * p.ntiles) || q->ns_tile.alloc(M * NB_PCI * NS_NT) ||
      q->desc.init(rows_bytes > sizeof(float) * cfg->n_tracks ? rows_bytes : sizeof(float) * cfg->n_tracks) ||
      hipMemset(q->avg.get(), 0, sizeof(float) * navg) != hipSuccess ||
      hipMemset(q->mean_cfo.get(), 0, sizeof(float) * cfg->n_tracks) != hipSuccess ||
      hipMemset(q->peak_values.get(), 0, sizeof(float) * M * NB_PCI) != hipSuccess ||
      hipMemset(q->abs_row.get(), 0, sizeof(float) * M * NS_NOUT) != hipSuccess) {
    hip_log("[srslte_hip] nbiot sync: device allocation failed\n");
    delete q;
    return nullptr;
  }
  p.taps = q->taps, p.head = q->head, p.shift2 = q->shift2, p.w = q->w, p.avg = q->avg, p.mean_cfo = q->mean_cfo, p.tile_max = q->np_tile;
  s.tw = q->tw, s.seq = q->seq, s.y = q->y, s.tile_max = q->ns_tile, s.peak_values = q->peak_values, s.abs_row = q->abs_row;
  return q;
}

void srslte_hip_nbiot_sync_destroy(srslte_hip_nbiot_sync_t* q) { delete q; }

int srslte_hip_nbiot_sync_tracks_reset(srslte_hip_nbiot_sync_t* q, uint32_t first, uint32_t n, void* stream)
{
  if (!q || first > q->cfg.n_tracks || n > q->cfg.n_tracks - first) return SRSLTE_ERROR_INVALID_INPUTS;
  if (n == 0) return SRSLTE_SUCCESS;
  hipLaunchKernelGGL(nbiot_track_reset_kernel, dim3(n), dim3(NB_THREADS), 0, (hipStream_t)stream, q->avg.get(), q->mean_cfo.get(), first, q->np.nout);
  LAUNCH_CHECK();
  return SRSLTE_SUCCESS;
}

int srslte_hip_nbiot_sync_tracks_set_cfo(srslte_hip_nbiot_sync_t* q, uint32_t first, uint32_t n, const float* cfo, void* stream)
{
  if (!q || first > q->cfg.n_tracks || n > q->cfg.n_tracks - first || (n && !cfo)) return SRSLTE_ERROR_INVALID_INPUTS;
  if (n == 0) return SRSLTE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  float*      h  = nullptr;
  if (int r = q->desc.begin(&h)) return r;
  memcpy(h, cfo, sizeof(float) * n);
  if (int r = q->desc.commit(sizeof(float) * n, st)) return r;
  hipLaunchKernelGGL(nbiot_track_set_cfo_kernel, dim3((n + 63) / 64), dim3(64), 0, st, q->mean_cfo.get(), q->desc.dev<float>(), first, n);
  LAUNCH_CHECK();
  return SRSLTE_SUCCESS;
}

int srslte_hip_nbiot_sync_tracks_read(srslte_hip_nbiot_sync_t* q, uint32_t track, float* h_mean_cfo, float* h_avg)
{
  if (!q || !h_mean_cfo || track >= q->cfg.n_tracks) return SRSLTE_ERROR_INVALID_INPUTS;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(h_mean_cfo, q->mean_cfo.get() + track, sizeof(float), hipMemcpyDeviceToHost));
  if (h_avg && q->np.nout) HIP_TRY(hipMemcpy(h_avg, q->avg.get() + (size_t)track * q->np.nout, sizeof(float) * q->np.nout, hipMemcpyDeviceToHost));
  return SRSLTE_SUCCESS;
}

int srslte_hip_nbiot_npss_find_batch(srslte_hip_nbiot_sync_t* q, const void* d_in, size_t in_stride, const srslte_hip_nbiot_npss_item_t* items, uint32_t n,
                                     srslte_hip_nbiot_npss_res_t* d_res, void* stream)
{
  if (!q || (n && (!d_in || !d_res || !items))) return SRSLTE_ERROR_INVALID_INPUTS;
  if (int r = srslte_hip_nbiot_sync_check(&q->cfg, in_stride, items, n)) return r;
  if (n == 0) return SRSLTE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  NpssRow*    h  = nullptr;
  if (int r = q->desc.begin(&h)) return r;
  for (uint32_t i = 0; i < n; i++) h[i] = {items[i].track, items[i].find_offset};
  if (int r = q->desc.commit(sizeof(NpssRow) * n, st)) return r;
  NpssParams p = q->np;
  p.in_stride  = in_stride;
  if (!p.short_branch) {
    hipLaunchKernelGGL(nbiot_npss_slide_kernel, dim3((p.mw + NB_TILE - 1) / NB_TILE, 2, n), dim3(NB_THREADS), 0, st, p, q->desc.dev<NpssRow>(),
                       (const cf32*)d_in);
    LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(nbiot_npss_comb_kernel, dim3(p.ntiles, n), dim3(NB_THREADS), 0, st, p, q->desc.dev<NpssRow>(), (const cf32*)d_in);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(nbiot_npss_decide_kernel, dim3(n), dim3(NB_THREADS), 0, st, p, q->desc.dev<NpssRow>(), (const cf32*)d_in, d_res);
  LAUNCH_CHECK();
  return SRSLTE_SUCCESS;
}

int srslte_hip_nbiot_nsss_find_batch(srslte_hip_nbiot_sync_t* q, const void* d_in, size_t in_stride, const int32_t* cell_ids, uint32_t n,
                                     srslte_hip_nbiot_nsss_res_t* d_res, void* stream)
{
  if (!q || (n && (!d_in || !d_res || !cell_ids))) return SRSLTE_ERROR_INVALID_INPUTS;
  if (int r = srslte_hip_nbiot_nsss_check(&q->cfg, in_stride, cell_ids, n)) return r;
  if (n == 0) return SRSLTE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  NsssRow*    h  = nullptr;
  if (int r = q->desc.begin(&h)) return r;
  // the ids follow the rows' full capacity, so their place does not depend on the call
  int32_t* const hid  = reinterpret_cast<int32_t*>(h + (size_t)NS_IDROWS * q->cfg.max_items);
  uint32_t       rows = 0;
  for (uint32_t i = 0; i < n; i++) {
    hid[i] = cell_ids[i];
    if (cell_ids[i] >= 0) {
      h[rows++] = {i, (uint32_t)cell_ids[i], 1u, 0u};
    } else {
      for (uint32_t k = 0; k < NS_IDROWS; k++) h[rows++] = {i, k * NS_PT, NB_PCI - k * NS_PT < NS_PT ? NB_PCI - k * NS_PT : NS_PT, 0u};
    }
  }
  for (uint32_t k = rows; k < NS_IDROWS * q->cfg.max_items; k++) h[k] = {0u, 0u, 0u, 0u}; // the copy carries the whole block
  if (int r = q->desc.commit(sizeof(NsssRow) * NS_IDROWS * q->cfg.max_items + sizeof(int32_t) * n, st)) return r;
  NsssParams p = q->ns;
  p.in_stride  = in_stride;
  const auto* d_rows = q->desc.dev<NsssRow>();
  const auto* d_ids  = reinterpret_cast<const int32_t*>(d_rows + (size_t)NS_IDROWS * q->cfg.max_items);
  hipLaunchKernelGGL(nbiot_nsss_slide_kernel, dim3(NS_MY / NB_TILE, 24, n), dim3(NB_THREADS), 0, st, p, (const cf32*)d_in);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(nbiot_nsss_prod_kernel, dim3(NS_NT, rows), dim3(NB_THREADS), 0, st, p, d_rows);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(nbiot_nsss_decide_kernel, dim3(n), dim3(NB_THREADS), 0, st, p, d_ids, d_res);
  LAUNCH_CHECK();
  q->last_nsss = n;
  return SRSLTE_SUCCESS;
}

int srslte_hip_nbiot_nsss_debug(srslte_hip_nbiot_sync_t* q, uint32_t item, float* h_peak_values, float* h_abs_row)
{
  if (!q || item >= q->last_nsss) return SRSLTE_ERROR_INVALID_INPUTS;
  HIP_TRY(hipDeviceSynchronize());
  if (h_peak_values) HIP_TRY(hipMemcpy(h_peak_values, q->peak_values.get() + (size_t)item * NB_PCI, sizeof(float) * NB_PCI, hipMemcpyDeviceToHost));
  if (h_abs_row) HIP_TRY(hipMemcpy(h_abs_row, q->abs_row.get() + (size_t)item * NS_NOUT, sizeof(float) * NS_NOUT, hipMemcpyDeviceToHost));
  return SRSLTE_SUCCESS;
}

} // extern "C"
