// The host side of the control information on a PUSCH (include/srslte_hip/phy_hip.h, "PUSCH UCI plan"): how a subframe's symbols are divided
// between HARQ-ACK, rank indication, CQI report and UL-SCH (36.212 5.2.2.6, 5.2.4.1; uci.c:264-281,:547-571 as sch.c:920-989,:1096-1176 call them)
// and where the ACK / RI symbols sit in the channel interleaver's matrix. The checks alone, nothing is queued, no device is needed. The four PUSCH
// pipelines and both UL-SCH drop-ins size their calls with it; each maps the reason to its own code and adds its own bounds.
#include "common.hpp"
#include "phy_hip_internal.hpp"
#include <math.h>
#include <string.h>

// 36.213 Tables 8.6.3-1..3 (sch.c:43-52); -1: reserved
static const float pusch_beta_harq[16] = {2.0f, 2.5f, 3.125f, 4.0f, 5.0f, 6.250f, 8.0f, 10.0f, 12.625f, 15.875f, 20.0f, 31.0f, 50.0f, 80.0f, 126.0f, -1.0f};
static const float pusch_beta_ri[16]   = {1.25f, 1.625f, 2.0f, 2.5f, 3.125f, 4.0f, 5.0f, 6.25f, 8.0f, 10.0f, 12.625f, 15.875f, 20.0f, -1.0f, -1.0f, -1.0f};
static const float pusch_beta_cqi[16]  = {-1.0f, -1.0f, 1.125f, 1.25f, 1.375f, 1.625f, 1.750f, 2.0f, 2.25f, 2.5f, 2.875f, 3.125f, 3.5f, 4.0f, 5.0f, 6.25f};

// the offset of a field in use: negative for a reserved index and for one outside the table
static float beta_of(const float* tab, uint32_t I_offset) { return I_offset > 15 ? -1.0f : tab[I_offset]; }

// Q_prime_ri_ack (uci.c:547-571): min(ceil(O M_sc N_symb beta / K), 4 M_sc) in float arithmetic, any number of bits O
static uint32_t qprime_ack_ri(uint32_t O, float beta, uint32_t L_prb, uint32_t nsymb, uint32_t K)
{
  const uint32_t x = (uint32_t)ceilf((float)O * L_prb * 12 * nsymb * beta / K), m = 4 * L_prb * 12;
  return x < m ? x : m;
}

uint32_t pusch_uci_cqi_qprime(const srslte_hip_pusch_uci_cfg_t* c, uint32_t O, uint32_t Qp_ri)
{ // Q_prime_cqi (uci.c:264-281), 0 without a report; upstream tests O < 11 here, so an 11-bit report is sized with the CRC it does not carry
  if (O == 0) return 0;
  const uint32_t L = O < 11 ? 0 : 8, m = c->L_prb * 12 * c->nof_symb - Qp_ri;
  const uint32_t x = c->K_segm ? (uint32_t)ceilf((float)(O + L) * c->L_prb * 12 * c->nof_symb * pusch_beta_cqi[c->I_offset_cqi] / c->K_segm) : 999999u;
  return x < m ? x : m;
}

void pusch_uci_symbol_pos(bool is_ri, uint32_t i, uint32_t rows, uint32_t nof_symb, uint32_t* row, uint32_t* col)
{ // uci.c:497-545: the column sets of 36.212 Table 5.2.2.8-1 / -2, walked three apart, four symbols to a row from the last row up
  static const uint32_t set_norm[2][4] = {{2, 3, 8, 9}, {1, 4, 7, 10}}, set_ext[2][4] = {{1, 2, 6, 7}, {0, 3, 5, 8}};
  *row = rows - 1 - i / 4;
  *col = nof_symb > 10 ? set_norm[is_ri][(3 * i) % 4] : set_ext[is_ri][(3 * i) % 4];
}

extern "C" int srslte_hip_pusch_uci_plan(const srslte_hip_pusch_uci_cfg_t* c, srslte_hip_pusch_uci_res_t* r)
{
  if (!c || !r || c->L_prb == 0 || c->nof_symb == 0 || c->rows == 0 || (c->K_segm == 0) != (c->C == 0)) return SRSLTE_ERROR_INVALID_INPUTS;
  memset(r, 0, sizeof(*r));
  pusch_uci_symbol_pos(false, c->sym, c->rows, c->nof_symb, &r->ack_pos[0], &r->ack_pos[1]);
  pusch_uci_symbol_pos(true, c->sym, c->rows, c->nof_symb, &r->ri_pos[0], &r->ri_pos[1]);
  const bool data = c->K_segm != 0;
  if (!data && c->cqi_len == 0) return SRSLTE_HIP_PUSCH_UCI_EMPTY; // a PUSCH without UL-SCH data carries a report (sch.c:1031-1065,:1133-1165)
  float       b_ack = c->ack_len ? beta_of(pusch_beta_harq, c->I_offset_ack) : 0.f, b_ri = c->ri_len ? beta_of(pusch_beta_ri, c->I_offset_ri) : 0.f;
  const float b_cqi = c->cqi_len || !data ? beta_of(pusch_beta_cqi, c->I_offset_cqi) : 0.f;
  if (b_ack < 0 || b_ri < 0 || b_cqi < 0) return SRSLTE_HIP_PUSCH_UCI_BETA; // uci.c:432,:475-478,:705-708,:761
  // without data the report's offset divides the two others and its size - plus its 8 CRC bits above 11 - stands for sum K_r (sch.c:943-946,
  // :970-973,:1111-1114,:1171-1174, uci.c:555-564)
  if (!data) b_ack /= b_cqi, b_ri /= b_cqi;
  const uint32_t Kq = data ? c->K_segm : (c->cqi_len <= 11 ? c->cqi_len : c->cqi_len + 8);
  r->Qp_ack = c->ack_len ? qprime_ack_ri(c->ack_len, b_ack, c->L_prb, c->nof_symb, Kq) : 0;
  r->Qp_ri  = c->ri_len ? qprime_ack_ri(c->ri_len, b_ri, c->L_prb, c->nof_symb, Kq) : 0;
  if (r->Qp_ack > 4 * c->rows || r->Qp_ri > 4 * c->rows) return SRSLTE_HIP_PUSCH_UCI_ROWS; // uci.c:504,:529: the rows must exist
  r->Qp_cqi = pusch_uci_cqi_qprime(c, c->cqi_len, r->Qp_ri);
  r->Q_cqi  = r->Qp_cqi * c->Qm;
  const uint32_t H = c->rows * c->nof_symb;
  if (r->Qp_ri + r->Qp_cqi > H || (data && r->Qp_ri + r->Qp_cqi == H)) return SRSLTE_HIP_PUSCH_UCI_NO_ROOM;
  r->G_prime = H - r->Qp_ri - r->Qp_cqi; // what the RI and the report leave (sch.c:1157-1160); the ACK symbols overwrite theirs
  if (data) r->syms_lo = r->G_prime / c->C, r->C_lo = c->C - r->G_prime % c->C; // gamma = G' mod C (sch.c:205-207)
  return SRSLTE_HIP_PUSCH_UCI_OK;
}

// The allocation of one PUSCH as pusch_cp walks it (pusch.c:53-91): slot by slot, every symbol but the DMRS (l = 3, or 2 with the extended CP) and,
// in a shortened subframe, the last one of slot 1; 12 L_prb REs from sub-carrier 12 n_prb_tilde[slot]. What srslte_hip_pusch_decode stages.
extern "C" int srslte_hip_pusch_rows(const srslte_hip_pusch_cfg_t* c, uint32_t* rows)
{
  if (!c || c->sch.mod < 1 || c->sch.mod > 3 || c->shortened > 1 || c->cp_ext > 1 || c->sf_idx > 9 || c->rnti > 0xffff || c->cell_id > 503)
    return SRSLTE_ERROR_INVALID_INPUTS;
  const uint32_t nsl = c->cp_ext ? 6 : 7, L = c->sch.L_prb, nsymb = 2 * nsl - 2 - c->shortened;
  if (!srslte_hip_dft_precoding_valid_prb(L) || c->nof_prb == 0 || c->nof_prb > 110 || c->n_prb_tilde[0] + L > c->nof_prb || c->n_prb_tilde[1] + L > c->nof_prb ||
      c->sch.nof_symb != nsymb || c->nof_re != 12 * L * nsymb || c->sch.nof_bits != c->nof_re * 2 * (uint32_t)c->sch.mod)
    return SRSLTE_ERROR_INVALID_INPUTS;
  uint32_t n = 0;
  for (uint32_t slot = 0; slot < 2; slot++) {
    for (uint32_t l = 0; l < nsl - (slot ? c->shortened : 0); l++) {
      if (l == nsl - 4) continue;
      if (rows) rows[2 * n] = l + slot * nsl, rows[2 * n + 1] = 12 * c->n_prb_tilde[slot];
      n++;
    }
  }
  return (int)n;
}
