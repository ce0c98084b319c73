// The host side of the sounding reference signal (include/srslte_hip/phy_hip.h, "UL sounding reference signal"): the tables and decisions of
// refsignal_ul.c:62-114 and :686-1026 restated operation by operation - who sends when, where in the band, which PUSCHs and PUCCHs give up
// their last symbol - and srslte_refsignal_srs_gen with the float / double mix of the reference. No device is needed for anything here;
// srs.hip uploads the sequences this file makes.
#include "common.hpp"
#include "phy_hip_internal.hpp"
#include <math.h>
#include <vector>

namespace {

// 36.211 Table 5.5.3.3-1, frame structure type 1: period and offsets of the cell's SRS subframes (refsignal_ul.c:62-65)
const uint32_t T_SFC[15]     = {1, 2, 2, 5, 5, 5, 5, 5, 5, 10, 10, 10, 10, 10, 10};
const uint32_t DELTA_SFC1[7] = {0, 0, 1, 0, 1, 2, 3};
const uint32_t DELTA_SFC2[4] = {0, 1, 2, 3};

// 36.211 Tables 5.5.3.2-1..4: m_SRS,b and N_b by [band of nof_prb][b][C_SRS] (refsignal_ul.c:68-114)
const uint32_t M_SRS_B[4][4][8] = {{{36, 32, 24, 20, 16, 12, 8, 4}, {12, 16, 4, 4, 4, 4, 4, 4}, {4, 8, 4, 4, 4, 4, 4, 4}, {4, 4, 4, 4, 4, 4, 4, 4}},
                                   {{48, 48, 40, 36, 32, 24, 20, 16}, {24, 16, 20, 12, 16, 4, 4, 4}, {12, 8, 4, 4, 8, 4, 4, 4}, {4, 4, 4, 4, 4, 4, 4, 4}},
                                   {{72, 64, 60, 48, 48, 40, 36, 32}, {24, 32, 20, 24, 16, 20, 12, 16}, {12, 16, 4, 12, 8, 4, 4, 8}, {4, 4, 4, 4, 4, 4, 4, 4}},
                                   {{96, 96, 80, 72, 64, 60, 48, 48}, {48, 32, 40, 24, 32, 20, 24, 16}, {24, 16, 20, 12, 16, 4, 12, 8}, {4, 4, 4, 4, 4, 4, 4, 4}}};
const uint32_t N_B[4][4][8]     = {{{1, 1, 1, 1, 1, 1, 1, 1}, {3, 2, 6, 5, 4, 3, 2, 1}, {3, 2, 1, 1, 1, 1, 1, 1}, {1, 2, 1, 1, 1, 1, 1, 1}},
                                   {{1, 1, 1, 1, 1, 1, 1, 1}, {2, 3, 2, 3, 2, 6, 5, 4}, {2, 2, 5, 3, 2, 1, 1, 1}, {3, 2, 1, 1, 2, 1, 1, 1}},
                                   {{1, 1, 1, 1, 1, 1, 1, 1}, {3, 2, 3, 2, 3, 2, 3, 2}, {2, 2, 5, 2, 2, 5, 3, 2}, {3, 4, 1, 3, 2, 1, 1, 2}},
                                   {{1, 1, 1, 1, 1, 1, 1, 1}, {2, 3, 2, 3, 2, 3, 2, 3}, {2, 2, 2, 2, 2, 5, 2, 2}, {6, 4, 5, 3, 4, 1, 3, 2}}};

uint32_t bw_table_idx(uint32_t nof_prb) { return nof_prb <= 40 ? 0 : nof_prb <= 60 ? 1 : nof_prb <= 80 ? 2 : 3; } // srsbwtable_idx :867-878

// 36.213 Table 8.2-1 (T_srs_table :686-710 and the offsets of srslte_refsignal_srs_send_ue :716-747): the first I_srs of each period
const uint32_t I_SRS_FIRST[9] = {0, 2, 7, 17, 37, 77, 157, 317, 637};
const uint32_t T_SRS[8]       = {2, 5, 10, 20, 40, 80, 160, 320};
int            t_srs_row(uint32_t I_srs)
{
  for (int i = 0; i < 8; i++)
    if (I_srs < I_SRS_FIRST[i + 1]) return i;
  return -1;
}
uint32_t t_srs(uint32_t I_srs)
{
  const int i = t_srs_row(I_srs);
  return i < 0 ? 0 : T_SRS[i];
}

// srs_Fb :896-916
uint32_t srs_Fb(const srslte_hip_srs_cfg_t* c, const srslte_hip_srs_ue_t* ue, uint32_t b, uint32_t tti)
{
  uint32_t       Fb = 0;
  const uint32_t T  = t_srs(ue->I_srs);
  if (T) {
    const uint32_t n_srs = tti / T, ti = bw_table_idx(c->nof_prb);
    const uint32_t N_b   = N_B[ti][b][c->bw_cfg];
    uint32_t       prod_1 = 1;
    for (uint32_t bp = ue->b_hop + 1; bp < b; bp++) prod_1 *= N_B[ti][bp][c->bw_cfg];
    const uint32_t prod_2 = prod_1 * N_B[ti][b][c->bw_cfg];
    if ((N_b % 2) == 0) {
      Fb = (N_b / 2) * ((n_srs % prod_2) / prod_1) + ((n_srs % prod_2) / prod_1 / 2);
    } else {
      Fb = (N_b / 2) * (n_srs / prod_1);
    }
  }
  return Fb;
}

// what srslte_refsignal_ul_set_cell keeps of the cell for the sequence: f_gh (srslte_group_hopping_f_gh, phy_common.c:419-436) and
// v_pusch[ns][delta_ss] (generate_srslte_sequence_hopping_v :149-163) of one delta_ss
void hopping_tables(const srslte_hip_srs_cfg_t* c, uint32_t f_gh[20], uint32_t v[20])
{
  std::vector<uint8_t> seq;
  lte_gold_sequence(c->cell_id / 30, 160, seq);
  for (uint32_t ns = 0; ns < 20; ns++) {
    f_gh[ns] = 0;
    for (int i = 0; i < 8; i++) f_gh[ns] += (uint32_t)seq[8 * ns + i] << i;
  }
  lte_gold_sequence(((c->cell_id / 30) << 5) + ((c->cell_id % 30) + c->delta_ss) % 30, 20, seq);
  for (uint32_t ns = 0; ns < 20; ns++) v[ns] = seq[ns];
}

// one slot of srslte_refsignal_srs_gen :998-1007: compute_r (:352-371) with delta_ss 0 for u, then exp(j (arg + alpha i))
void srs_gen_slot(const srslte_hip_srs_cfg_t* c, const uint32_t f_gh[20], const uint32_t v_tab[20], uint32_t M_sc, uint32_t n_srs, uint32_t ns, float* arg,
                  cf32* r)
{
  const uint32_t nof_prb = M_sc / 12;
  const uint32_t u       = ((c->group_hopping_en ? f_gh[ns] : 0) + (c->cell_id % 30) + 0) % 30;
  const uint32_t v       = (nof_prb >= 6 && c->sequence_hopping_en) ? v_tab[ns] : 0;
  ul_r_uv_arg(nof_prb, u, v, arg);
  const float alpha = (float)(2 * M_PI * n_srs / 8);
  for (uint32_t i = 0; i < M_sc; i++) {
    const float x = fmaf(alpha, (float)i, arg[i]); // the reference's -Ofast -mfma build fuses tmp_arg[i] + alpha * i
    r[i]          = make_float2(cosf(x), sinf(x));
  }
}

} // namespace

bool srs_cfg_valid(const srslte_hip_srs_cfg_t* c)
{
  return c && c->nof_prb >= 6 && c->nof_prb <= 110 && c->cell_id <= 503 && !c->tdd && c->subframe_config < 15 && c->bw_cfg < 8 && c->delta_ss < 30 &&
         M_SRS_B[bw_table_idx(c->nof_prb)][0][c->bw_cfg] <= c->nof_prb;
}

int srs_list_check(const srslte_hip_srs_cfg_t* c, uint32_t tti0, uint32_t nof_sf, const srslte_hip_srs_ue_t* list, uint32_t nof)
{
  if (!srs_cfg_valid(c) || (nof && !list) || nof > c->max_srs) return SRSLTE_ERROR_INVALID_INPUTS;
  for (uint32_t i = 0; i < nof; i++) {
    const srslte_hip_srs_ue_t& ue = list[i];
    bool ok = ue.B <= 3 && ue.b_hop <= 3 && ue.n_srs <= 7 && ue.k_tc <= 1 && ue.I_srs < 637 && ue.n_rrc <= 23 && ue.sf < nof_sf;
    // the tables keep every position of the hopping tree inside the cell's sounding band; the launch still relies on nothing but this test
    ok = ok && srslte_hip_srs_k0(c, &ue, tti0 + ue.sf) + 2 * (srslte_hip_srs_M_sc(c, &ue) - 1) < 12 * c->nof_prb;
    if (!ok) {
      hip_log("[srslte_hip] srs: entry %u refused (sf %u of %u, B %u, b_hop %u, n_srs %u, I_srs %u, k_tc %u, n_rrc %u)\n", i, ue.sf, nof_sf, ue.B, ue.b_hop,
              ue.n_srs, ue.I_srs, ue.k_tc, ue.n_rrc);
      return SRSLTE_ERROR_INVALID_INPUTS;
    }
  }
  return SRSLTE_SUCCESS;
}

void srs_first_slot_table(const srslte_hip_srs_cfg_t* c, uint32_t M_sc, uint32_t n_srs, std::vector<cf32>& r)
{
  uint32_t f_gh[20], v[20];
  hopping_tables(c, f_gh, v);
  std::vector<float> arg(M_sc);
  r.resize((size_t)10 * M_sc);
  for (uint32_t sf_idx = 0; sf_idx < 10; sf_idx++) srs_gen_slot(c, f_gh, v, M_sc, n_srs, 2 * sf_idx, arg.data(), r.data() + (size_t)sf_idx * M_sc);
}

extern "C" {

// srslte_refsignal_srs_send_cs :820-865
int srslte_hip_srs_send_cs(uint32_t subframe_config, uint32_t sf_idx)
{
  if (subframe_config >= 15 || sf_idx >= 10) return SRSLTE_ERROR_INVALID_INPUTS;
  const uint32_t m = sf_idx % T_SFC[subframe_config];
  if (subframe_config < 7) return m == DELTA_SFC1[subframe_config] ? 1 : 0;
  if (subframe_config == 7) return (m == 0 || m == 1) ? 1 : 0;
  if (subframe_config == 8) return (m == 2 || m == 3) ? 1 : 0;
  if (subframe_config < 13) return m == DELTA_SFC2[subframe_config - 9] ? 1 : 0;
  if (subframe_config == 13) return (m == 5 || m == 7 || m == 9) ? 0 : 1;
  return (m == 7 || m == 9) ? 0 : 1;
}

// srslte_refsignal_srs_send_ue :716-747. tti - Toffset is a uint32_t difference: for tti < Toffset it is 2^32 + tti - Toffset, as there
int srslte_hip_srs_send_ue(uint32_t I_srs, uint32_t tti)
{
  if (!(I_srs < 1024 && tti < 10240)) return SRSLTE_ERROR_INVALID_INPUTS;
  const int row = t_srs_row(I_srs);
  if (row < 0) return 0;
  const uint32_t Toffset = I_srs - I_SRS_FIRST[row];
  return ((tti - Toffset) % T_SRS[row]) == 0 ? 1 : 0;
}

uint32_t srslte_hip_srs_rb_start_cs(uint32_t bw_cfg, uint32_t nof_prb)
{
  return bw_cfg < 8 ? nof_prb / 2 - M_SRS_B[bw_table_idx(nof_prb)][0][bw_cfg] / 2 : 0;
}

uint32_t srslte_hip_srs_rb_L_cs(uint32_t bw_cfg, uint32_t nof_prb) { return bw_cfg < 8 ? M_SRS_B[bw_table_idx(nof_prb)][0][bw_cfg] : 0; }

// srslte_refsignal_srs_M_sc :943-946
uint32_t srslte_hip_srs_M_sc(const srslte_hip_srs_cfg_t* cfg, const srslte_hip_srs_ue_t* ue)
{
  if (!cfg || !ue || cfg->bw_cfg >= 8 || ue->B >= 4) return 0;
  return M_SRS_B[bw_table_idx(cfg->nof_prb)][ue->B][cfg->bw_cfg] * 12 / 2;
}

// srs_k0_ue :919-941
uint32_t srslte_hip_srs_k0(const srslte_hip_srs_cfg_t* cfg, const srslte_hip_srs_ue_t* ue, uint32_t tti)
{
  if (!cfg || !ue || !(cfg->bw_cfg < 8 && ue->B < 4 && ue->k_tc < 2)) return 0;
  const uint32_t ti = bw_table_idx(cfg->nof_prb);
  uint32_t       k0 = srslte_hip_srs_rb_start_cs(cfg->bw_cfg, cfg->nof_prb) * 12 + ue->k_tc;
  for (uint32_t b = 0; b <= ue->B; b++) {
    const uint32_t m_srs = M_SRS_B[ti][b][cfg->bw_cfg], m_sc = m_srs * 12 / 2;
    uint32_t       nb;
    if (b <= ue->b_hop) {
      nb = (4 * ue->n_rrc / m_srs) % N_B[ti][b][cfg->bw_cfg];
    } else {
      nb = ((4 * ue->n_rrc / m_srs) + srs_Fb(cfg, ue, b, tti)) % N_B[ti][b][cfg->bw_cfg];
    }
    k0 += 2 * m_sc * nb;
  }
  return k0;
}

// srslte_refsignal_srs_pusch_shortened :769-814, the comparisons as they are written there
int srslte_hip_srs_pusch_shortened(const srslte_hip_srs_cfg_t* cfg, const srslte_hip_srs_ue_t* ue, uint32_t tti, const uint32_t n_prb_tilde[2],
                                   uint32_t L_prb)
{
  if (!cfg || !n_prb_tilde) return SRSLTE_ERROR_INVALID_INPUTS;
  bool shortened = false;
  if (ue) {
    const uint32_t k0_srs = srslte_hip_srs_rb_start_cs(cfg->bw_cfg, cfg->nof_prb), nrb_srs = srslte_hip_srs_rb_L_cs(cfg->bw_cfg, cfg->nof_prb);
    if (srslte_hip_srs_send_cs(cfg->subframe_config, tti % 10) == 1 && srslte_hip_srs_send_ue(ue->I_srs, tti) == 1) {
      shortened = true;
      for (uint32_t ns = 0; ns < 2 && shortened; ns++) {
        if (n_prb_tilde[ns] == k0_srs + nrb_srs || n_prb_tilde[ns] + L_prb == k0_srs) shortened = false;
      }
    }
    if (!shortened) {
      if (srslte_hip_srs_send_cs(cfg->subframe_config, tti % 10) == 1) {
        for (uint32_t ns = 0; ns < 2 && !shortened; ns++) {
          if ((n_prb_tilde[ns] >= k0_srs && n_prb_tilde[ns] < k0_srs + nrb_srs) ||
              (n_prb_tilde[ns] + L_prb >= k0_srs && n_prb_tilde[ns] + L_prb < k0_srs + nrb_srs) ||
              (n_prb_tilde[ns] <= k0_srs && n_prb_tilde[ns] + L_prb >= k0_srs + nrb_srs)) {
            shortened = true;
          }
        }
      }
    }
  }
  return shortened ? 1 : 0;
}

// srslte_refsignal_srs_pucch_shortened :750-767
int srslte_hip_srs_pucch_shortened(const srslte_hip_srs_cfg_t* cfg, int ue_configured, int simul_ack, uint32_t format, uint32_t tti)
{
  if (!cfg) return SRSLTE_ERROR_INVALID_INPUTS;
  bool shortened = false;
  if (ue_configured && format < 3 /* SRSLTE_PUCCH_FORMAT_2 */) {
    if (simul_ack && srslte_hip_srs_send_cs(cfg->subframe_config, tti % 10) == 1) shortened = true;
  }
  return shortened ? 1 : 0;
}

// srslte_refsignal_srs_gen :987-1011: r [2][M_sc]
int srslte_hip_srs_gen(const srslte_hip_srs_cfg_t* cfg, const srslte_hip_srs_ue_t* ue, uint32_t sf_idx, void* r)
{
  if (!srs_cfg_valid(cfg) || !ue || !r || sf_idx >= 10 || ue->B > 3 || ue->n_srs > 7) return SRSLTE_ERROR_INVALID_INPUTS;
  uint32_t f_gh[20], v[20];
  hopping_tables(cfg, f_gh, v);
  const uint32_t     M_sc = srslte_hip_srs_M_sc(cfg, ue);
  std::vector<float> arg(M_sc);
  for (uint32_t ns = 2 * sf_idx; ns < 2 * (sf_idx + 1); ns++) srs_gen_slot(cfg, f_gh, v, M_sc, ue->n_srs, ns, arg.data(), (cf32*)r + (size_t)(ns % 2) * M_sc);
  return SRSLTE_SUCCESS;
}

int srslte_hip_srs_check(const srslte_hip_srs_cfg_t* cfg, uint32_t tti0, uint32_t nof_sf, const srslte_hip_srs_ue_t* list, uint32_t nof)
{
  return srs_list_check(cfg, tti0, nof_sf, list, nof);
}

} // extern "C"
