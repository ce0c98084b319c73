// The host side of the neighbour-cell measurement (include/srslte_hip/phy_hip.h, "Neighbour-cell measurement"): the checks of a configuration
// and of a call, the inter-stage twiddles of the four-step transforms and the SSS values meas.hip places on its replica grids. No device is
// needed for anything here.
#include "common.hpp"
#include "phy_hip_internal.hpp"
#include <math.h>
#include <vector>

uint32_t meas_symbol_sz(const srslte_hip_meas_cfg_t* c)
{
  if (c->symbol_sz) return c->symbol_sz;
  const int n = lte_symbol_sz((int)c->nof_prb);
  return n > 0 ? (uint32_t)n : 0u;
}

bool meas_cfg_valid(const srslte_hip_meas_cfg_t* c)
{
  if (!c || c->cp_ext || c->nof_prb < 6 || c->nof_prb > 110) return false;
  const uint32_t N = meas_symbol_sz(c);
  // the sizes srslte_hip_ofdm_create_sz takes: the two symbol-size families of phy_common.c:304-345, holding the carriers
  if (!(N == 128 || N == 256 || N == 384 || N == 512 || N == 768 || N == 1024 || N == 1536 || N == 2048) || 12 * c->nof_prb >= N) return false;
  if (c->max_captures == 0 || c->max_cells == 0 || c->max_cells > 504 || (uint64_t)c->max_captures * c->max_cells > 65535) return false; // rows: grid.z
  if (c->max_sf < 2 || (uint64_t)c->max_sf * 15 * N > 0xffffffffull) return false; // peak_index is 32 bits wide
  if (!(c->threshold >= 0.f)) return false;
  return true;
}

void meas_twiddles(uint32_t N, std::vector<cf32>& tw2)
{
  const uint32_t M = 30 * N;
  tw2.resize(M);
  for (uint32_t i = 0; i < M; i++) {
    const double a = -2.0 * M_PI * (double)i / (double)M;
    tw2[i]         = make_float2((float)cos(a), (float)sin(a));
  }
}

void meas_sss_seq(uint32_t cell_id, float* s0, float* s5)
{ // srslte_sss_generate (gen_sss.c:121-155) from the tables of sync_tables
  static const SyncTables t = [] {
    SyncTables x;
    sync_tables(64, x);
    return x;
  }();
  uint32_t       m0, m1;
  const uint32_t v = cell_id % 3;
  sync_m0m1(cell_id / 3, &m0, &m1);
  for (int i = 0; i < 31; i++) {
    const float c0 = t.c[(v * 2) * 31 + i], c1 = t.c[(v * 2 + 1) * 31 + i];
    s0[2 * i]     = t.s[m0 * 31 + i] * c0;
    s0[2 * i + 1] = t.s[m1 * 31 + i] * c1 * t.z1[m0 * 31 + i];
    s5[2 * i]     = t.s[m1 * 31 + i] * c0;
    s5[2 * i + 1] = t.s[m0 * 31 + i] * c1 * t.z1[m1 * 31 + i];
  }
}

extern "C" int srslte_hip_meas_check(const srslte_hip_meas_cfg_t* c, size_t in_stride, uint32_t nof_sf, uint32_t n_captures, uint32_t n_cells)
{
  if (!meas_cfg_valid(c)) return SRSLTE_ERROR_INVALID_INPUTS;
  if (nof_sf < 2 || nof_sf > c->max_sf || n_captures > c->max_captures || n_cells > c->max_cells) return SRSLTE_ERROR_INVALID_INPUTS;
  if ((uint64_t)in_stride < (uint64_t)nof_sf * 15 * meas_symbol_sz(c)) return SRSLTE_ERROR_INVALID_INPUTS;
  return SRSLTE_SUCCESS;
}
