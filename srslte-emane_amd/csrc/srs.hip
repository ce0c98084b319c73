// Sounding reference signal for gfx950, FDD (include/srslte_hip/phy_hip.h, "UL sounding reference signal"): srslte_refsignal_srs_put for a list
// of (subframe, UE) entries on UE grids, and the eNB's sounding receiver - this library's own, the reference has none - on received grids.
//   srs_tx_kernel  one workgroup per entry: r[i] into grid[sf][nsym-1][k0 + 2 i]
//   srs_rx_kernel  one workgroup of two wavefronts per request, a lane per block of 8 sounded REs: z = y conj(r), the 8-point DFT over the
//                  block in registers (bin k: the UE whose cyclic shift is n_srs + k), h_j = bin 0 to d_ce; |h|^2, the free bins' power and
//                  h_{j+1} conj(h_j) (the neighbour lane's h, through LDS across the wavefront boundary at J > 64) summed in the wavefront and
//                  then over the two wavefronts; lane 0 writes the record
// The sequences come from srs_host.cpp: the first slot's of each subframe of a frame per (M_sc, n_srs), made on first use and kept.
#include "cf32_dev.hpp"
#include "common.hpp"
#include "dev_buf.hpp"
#include "phy_hip_internal.hpp"
#include <map>
#include <math.h>
#include <vector>

namespace {

constexpr int SRS_RX_THREADS = 128; // J <= 72 blocks: two wavefronts

struct SrsDesc {
  const cf32* r;      // the sequence of this entry's subframe, M_sc values
  uint32_t    re0;    // index into the grid of the first sounded RE: (sf nsym + nsym - 1) 12 nof_prb + k0
  uint32_t    M_sc;
  uint32_t    free_bins; // bit k: bin k (1-7) of the block DFT belongs to no UE
  uint32_t    reserved;
};

__device__ __forceinline__ cf32 mulmj(cf32 a) { return make_float2(a.y, -a.x); } // -j a

// forward 4-point DFT: X[k] = sum_n x[n] exp(-j 2 pi k n / 4)
__device__ __forceinline__ void dft4(cf32 a, cf32 b, cf32 c, cf32 d, cf32 X[4])
{
  const cf32 s0 = cadd(a, c), s1 = csub(a, c), s2 = cadd(b, d), s3 = mulmj(csub(b, d));
  X[0] = cadd(s0, s2), X[1] = cadd(s1, s3), X[2] = csub(s0, s2), X[3] = csub(s1, s3);
}

__global__ __launch_bounds__(256) void srs_tx_kernel(const SrsDesc* __restrict__ desc, cf32* __restrict__ grid)
{
  const SrsDesc d = desc[blockIdx.x];
  cf32*         g = grid + d.re0;
  for (uint32_t i = threadIdx.x; i < d.M_sc; i += blockDim.x) g[2 * i] = d.r[i];
}

__global__ __launch_bounds__(SRS_RX_THREADS) void srs_rx_kernel(const SrsDesc* __restrict__ desc, const cf32* __restrict__ grid,
                                                                srslte_hip_srs_res_t* __restrict__ res, cf32* __restrict__ ce)
{
  __shared__ cf32  s_edge;    // h of the second wavefront's first block
  __shared__ float s_red[2][4];
  const SrsDesc d = desc[blockIdx.x];
  const int     j = threadIdx.x, lane = j % 64, wave = j / 64, J = (int)(d.M_sc / 8);
  cf32  h = make_float2(0.f, 0.f);
  float pw = 0.f, nz = 0.f;
  if (j < J) {
    const cf32* y = grid + d.re0 + 16 * j;
    const cf32* r = d.r + 8 * j;
    cf32        z[8], E[4], O[4];
#pragma unroll
    for (int i = 0; i < 8; i++) z[i] = cmulconj(y[2 * i], r[i]);
    dft4(z[0], z[2], z[4], z[6], E);
    dft4(z[1], z[3], z[5], z[7], O);
    const float c = 0.70710678118654752f;
    O[1] = make_float2((O[1].x + O[1].y) * c, (O[1].y - O[1].x) * c);  // exp(-j pi / 4) O[1]
    O[2] = mulmj(O[2]);
    O[3] = make_float2((O[3].y - O[3].x) * c, -(O[3].x + O[3].y) * c); // exp(-j 3 pi / 4) O[3]
    cf32 Z[8];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      Z[k]     = make_float2((E[k].x + O[k].x) * 0.125f, (E[k].y + O[k].y) * 0.125f);
      Z[k + 4] = make_float2((E[k].x - O[k].x) * 0.125f, (E[k].y - O[k].y) * 0.125f);
    }
    h  = Z[0];
    pw = h.x * h.x + h.y * h.y;
#pragma unroll
    for (int k = 1; k < 8; k++)
      if (d.free_bins >> k & 1u) nz += Z[k].x * Z[k].x + Z[k].y * Z[k].y;
    ce[(size_t)blockIdx.x * SRSLTE_HIP_SRS_MAX_CE + j] = h;
  }
  if (j == 64) s_edge = h;
  cf32 hn = make_float2(__shfl_down(h.x, 1, 64), __shfl_down(h.y, 1, 64)); // h_{j+1}; lane 63 keeps its own
  __syncthreads();
  if (j == 63) hn = s_edge;
  cf32 cr = make_float2(0.f, 0.f);
  if (j + 1 < J) cr = cmulconj(hn, h);
  pw = wave_sum(pw), nz = wave_sum(nz), cr.x = wave_sum(cr.x), cr.y = wave_sum(cr.y);
  if (lane == 0) s_red[wave][0] = pw, s_red[wave][1] = nz, s_red[wave][2] = cr.x, s_red[wave][3] = cr.y;
  __syncthreads();
  if (j == 0) {
    const int   nfree = __popc(d.free_bins);
    const float rsrp  = (s_red[0][0] + s_red[1][0]) / (float)J;
    const float noise = nfree ? 8.f * (s_red[0][1] + s_red[1][1]) / (float)(J * nfree) : 0.f;
    const float cx = s_red[0][2] + s_red[1][2], cy = s_red[0][3] + s_red[1][3];
    srslte_hip_srs_res_t o;
    o.rsrp               = rsrp;
    o.noise_estimate     = noise;
    o.noise_estimate_dbm = (float)(10 * log10((double)noise) + 30); // chest_ul.c:317-321
    o.snr                = noise ? rsrp / noise : NAN;
    o.snr_db             = (float)(10 * log10((double)o.snr));
    o.ta_us              = J > 1 ? (float)(-atan2((double)cy, (double)cx) / (2.0 * M_PI * 16.0 * 15e3) * 1e6) : 0.f;
    o.nof_ce             = (uint32_t)J;
    res[blockIdx.x]      = o;
  }
}

} // namespace

struct srslte_hip_srs {
  srslte_hip_srs_cfg_t cfg;
  uint32_t             nsym;
  DescStage            desc;
  std::map<std::pair<uint32_t, uint32_t>, DevBuf<cf32>> tables; // (M_sc, n_srs) -> [10][M_sc], every one seen so far
};

namespace {

int srs_table_cached(srslte_hip_srs* q, uint32_t M_sc, uint32_t n_srs, const cf32** d_r)
{
  auto it = q->tables.find({M_sc, n_srs});
  if (it == q->tables.end()) {
    std::vector<cf32> r;
    srs_first_slot_table(&q->cfg, M_sc, n_srs, r);
    DevBuf<cf32> d;
    if (d.upload(r)) {
      hip_log("[srslte_hip] srs: the upload of a sequence table failed\n");
      return SRSLTE_ERROR;
    }
    it = q->tables.emplace(std::make_pair(M_sc, n_srs), std::move(d)).first;
  }
  *d_r = it->second.get();
  return SRSLTE_SUCCESS;
}

// checks, tables and descriptors of a call; the descriptors are on their way to the device when it returns
int srs_stage(srslte_hip_srs* q, uint32_t tti0, uint32_t nof_sf, const srslte_hip_srs_ue_t* list, uint32_t nof, hipStream_t st)
{
  if (int r = srs_list_check(&q->cfg, tti0, nof_sf, list, nof)) return r;
  if (nof == 0) return SRSLTE_SUCCESS;
  std::vector<const cf32*> tab(nof);
  for (uint32_t i = 0; i < nof; i++)
    if (int r = srs_table_cached(q, srslte_hip_srs_M_sc(&q->cfg, &list[i]), list[i].n_srs, &tab[i])) return r;
  SrsDesc* h = nullptr;
  if (int r = q->desc.begin(&h)) return r;
  const uint32_t nre = 12 * q->cfg.nof_prb;
  for (uint32_t i = 0; i < nof; i++) {
    const srslte_hip_srs_ue_t& ue  = list[i];
    const uint32_t             tti = tti0 + ue.sf, M_sc = srslte_hip_srs_M_sc(&q->cfg, &ue);
    uint32_t                   fb  = 0;
    for (uint32_t k = 1; k < 8; k++)
      if (!(ue.cs_used >> ((ue.n_srs + k) % 8) & 1u)) fb |= 1u << k;
    h[i] = {tab[i] + (size_t)(tti % 10) * M_sc, (ue.sf * q->nsym + q->nsym - 1) * nre + srslte_hip_srs_k0(&q->cfg, &ue, tti), M_sc, fb, 0u};
  }
  return q->desc.commit(sizeof(SrsDesc) * nof, st);
}

} // namespace

bool srs_same_cell(const srslte_hip_srs_t* q, uint32_t nof_prb, uint32_t cell_id, int cp_ext)
{
  return q && q->cfg.nof_prb == nof_prb && q->cfg.cell_id == cell_id && !q->cfg.cp_ext == !cp_ext;
}

const srslte_hip_srs_cfg_t* srs_cfg(const srslte_hip_srs_t* q) { return &q->cfg; }

extern "C" {

srslte_hip_srs_t* srslte_hip_srs_create(const srslte_hip_srs_cfg_t* cfg)
{
  if (!srs_cfg_valid(cfg)) {
    hip_log("[srslte_hip] srs: invalid SRS configuration (TDD is not supported; the cell's sounding band has to fit the cell)\n");
    return nullptr;
  }
  auto* q  = new srslte_hip_srs();
  q->cfg   = *cfg;
  q->nsym  = cfg->cp_ext ? 12 : 14;
  const size_t n = cfg->max_srs ? cfg->max_srs : 1;
  if (q->desc.init(sizeof(SrsDesc) * n)) {
    hip_log("[srslte_hip] srs: device allocation failed\n");
    delete q;
    return nullptr;
  }
  return q;
}

void srslte_hip_srs_destroy(srslte_hip_srs_t* q) { delete q; }

int srslte_hip_srs_tx_put(srslte_hip_srs_t* q, uint32_t tti0, uint32_t nof_sf, const srslte_hip_srs_ue_t* list, uint32_t nof, void* d_grid, void* stream)
{
  if (!q || (nof && !d_grid)) return SRSLTE_ERROR_INVALID_INPUTS;
  hipStream_t st = (hipStream_t)stream;
  if (int r = srs_stage(q, tti0, nof_sf, list, nof, st)) return r;
  if (nof == 0) return SRSLTE_SUCCESS;
  hipLaunchKernelGGL(srs_tx_kernel, dim3(nof), dim3(256), 0, st, q->desc.dev<SrsDesc>(), (cf32*)d_grid);
  LAUNCH_CHECK();
  return SRSLTE_SUCCESS;
}

int srslte_hip_srs_rx_batch(srslte_hip_srs_t* q, const void* d_grid, uint32_t tti0, uint32_t nof_sf, const srslte_hip_srs_ue_t* list, uint32_t nof,
                            srslte_hip_srs_res_t* d_res, void* d_ce, void* stream)
{
  if (!q || (nof && (!d_grid || !d_res || !d_ce))) return SRSLTE_ERROR_INVALID_INPUTS;
  hipStream_t st = (hipStream_t)stream;
  if (int r = srs_stage(q, tti0, nof_sf, list, nof, st)) return r;
  if (nof == 0) return SRSLTE_SUCCESS;
  hipLaunchKernelGGL(srs_rx_kernel, dim3(nof), dim3(SRS_RX_THREADS), 0, st, q->desc.dev<SrsDesc>(), (const cf32*)d_grid, d_res, (cf32*)d_ce);
  LAUNCH_CHECK();
  return SRSLTE_SUCCESS;
}

} // extern "C"
