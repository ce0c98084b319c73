// Host side of the UE CSI feedback (include/srslte_hip/phy_hip.h, "UE CSI feedback"): the report schedule, sizes and packing of cqi.c
// and the two report generators of ue_dl.c:802-928 on a measurement record of srslte_hip_csi_batch. Pure host code, no device call.
#include "phy_hip_internal.hpp"
#include <math.h>
#include <string.h>

namespace {

enum { TYPE_WIDEBAND = 0, TYPE_SUBBAND, TYPE_SUBBAND_UE, TYPE_SUBBAND_HL }; // srslte_cqi_type_t (cqi.h:114-119)

// srslte_bit_unpack (bit.c): nof_bits of value, most significant first, one per byte
void bit_unpack(uint32_t value, uint8_t** bits, uint32_t nof_bits)
{
  for (uint32_t i = 0; i < nof_bits; i++) (*bits)[i] = (uint8_t)((value >> (nof_bits - i - 1)) & 0x1);
  *bits += nof_bits;
}

// 36.213 Table 7.2.2-1A (cqi.c:386-455). As in the reference an index above the table's last row of a TDD cell leaves N_p = 0
bool get_N_fdd(uint32_t I, uint32_t* N_p, uint32_t* N_offset)
{
  if (I <= 1) *N_p = 2, *N_offset = I;
  else if (I <= 6) *N_p = 5, *N_offset = I - 2;
  else if (I <= 16) *N_p = 10, *N_offset = I - 7;
  else if (I <= 36) *N_p = 20, *N_offset = I - 17;
  else if (I <= 76) *N_p = 40, *N_offset = I - 37;
  else if (I <= 156) *N_p = 80, *N_offset = I - 77;
  else if (I <= 316) *N_p = 160, *N_offset = I - 157;
  else if (I == 317) return false;
  else if (I <= 349) *N_p = 32, *N_offset = I - 318;
  else if (I <= 413) *N_p = 64, *N_offset = I - 350;
  else if (I <= 541) *N_p = 128, *N_offset = I - 414;
  else if (I <= 1023) return false;
  return true;
}

bool get_N_tdd(uint32_t I, uint32_t* N_p, uint32_t* N_offset)
{
  if (I == 0) *N_p = 1, *N_offset = I;
  else if (I <= 5) *N_p = 5, *N_offset = I - 1;
  else if (I <= 15) *N_p = 10, *N_offset = I - 5;
  else if (I <= 35) *N_p = 20, *N_offset = I - 16;
  else if (I <= 75) *N_p = 40, *N_offset = I - 36;
  else if (I <= 155) *N_p = 80, *N_offset = I - 76;
  else if (I <= 315) *N_p = 160, *N_offset = I - 156;
  else if (I == 1023) return false;
  return true;
}

// srslte_cqi_hl_get_no_subbands (cqi.c:575-601)
int hl_no_subbands(int nof_prb)
{
  const int sz = nof_prb < 7 ? 0 : nof_prb <= 26 ? 4 : nof_prb <= 63 ? 6 : nof_prb <= 110 ? 8 : -1;
  return sz > 0 ? (int)ceil((float)nof_prb / sz) : 0;
}

// select_pmi(q, ri, &pmi, NULL) of ue_dl.c:707-733 on the record: nothing on a single-port cell, the selection for ri + 1 layers otherwise
// (more than two layers: srslte_precoding_pmi_select refuses and pmi keeps its 0)
uint32_t select_pmi(const srslte_hip_csi_res_t* csi, const srslte_hip_csi_report_cfg_t* cfg, uint32_t ri)
{
  if (cfg->nof_ports < 2) return 0;
  return ri == 0 ? csi->pmi_1l : ri == 1 ? csi->pmi_2l : 0;
}

// srslte_ue_dl_select_ri(q, &cfg->last_ri, NULL): srslte_precoding_cn computes 2x2 only and leaves last_ri alone otherwise
void select_ri_cn(const srslte_hip_csi_res_t* csi, srslte_hip_csi_report_cfg_t* cfg)
{
  if (cfg->nof_ports == 2 && cfg->nof_rx_antennas == 2) cfg->last_ri = csi->ri_cn;
}

// select_ri_pmi(q, &cfg->last_ri, pmi, sinr_db) of ue_dl.c:735-779: on a single-port cell it still writes ri 0, pmi 0 and -inf
void select_ri_pmi(const srslte_hip_csi_res_t* csi, srslte_hip_csi_report_cfg_t* cfg, uint32_t* pmi, float* sinr_db)
{
  const bool on = cfg->nof_ports >= 2;
  cfg->last_ri  = on ? csi->ri : 0;
  if (pmi) *pmi = on ? csi->pmi : 0;
  if (sinr_db) *sinr_db = on ? csi->sinr_db : -INFINITY;
}

// cqi_len = srslte_cqi_size and the packed row; a report past 64 bits (mode 31 with two codewords above 104 PRB) is refused
int finish(srslte_hip_csi_report_t* out)
{
  memset(out->cqi_bits, 0, sizeof(out->cqi_bits));
  const int len = srslte_hip_cqi_size(&out->cqi);
  if (len > SRSLTE_HIP_CQI_MAX_BITS) return SRSLTE_ERROR_INVALID_INPUTS;
  out->cqi_len = len > 0 ? (uint32_t)len : 0;
  if (out->cqi.data_enable && srslte_hip_cqi_value_pack(&out->cqi, &out->value, out->cqi_bits) < 0) return SRSLTE_ERROR_INVALID_INPUTS;
  return SRSLTE_SUCCESS;
}

} // namespace

extern "C" {

int srslte_hip_cqi_size(const srslte_hip_cqi_cfg_t* cfg)
{
  if (!cfg) return SRSLTE_ERROR_INVALID_INPUTS;
  int size = 0;
  if (!cfg->data_enable) return 0;
  switch (cfg->type) {
    case TYPE_WIDEBAND: // 36.212 Tables 5.2.3.3.1-1 and 5.2.3.3.1-2
      size = 4;
      if (cfg->pmi_present) {
        if (cfg->four_antenna_ports) size += (cfg->rank_is_not_one ? 3 : 0) + 4;
        else size += cfg->rank_is_not_one ? 3 + 1 : 2;
      }
      break;
    case TYPE_SUBBAND: size = 2; break; // cqi.c:353 reads "4 + (label_2_bits) ? 2 : 1", which is 2 for either label width
    case TYPE_SUBBAND_UE: size = 4 + 2 + (int)cfg->L; break;
    case TYPE_SUBBAND_HL:
      size += 4 + 2 * (int)cfg->N;
      if (cfg->rank_is_not_one && cfg->pmi_present) size += 4 + 2 * (int)cfg->N;
      if (cfg->pmi_present) size += cfg->four_antenna_ports ? 4 : cfg->rank_is_not_one ? 1 : 2;
      break;
    default: size = SRSLTE_ERROR;
  }
  return size;
}

int srslte_hip_cqi_value_pack(const srslte_hip_cqi_cfg_t* cfg, const srslte_hip_cqi_value_t* v, uint8_t buff[SRSLTE_HIP_CQI_MAX_BITS])
{
  if (!cfg || !v || !buff) return SRSLTE_ERROR_INVALID_INPUTS;
  uint8_t* ptr = buff;
  switch (cfg->type) {
    case TYPE_WIDEBAND: // cqi_format2_wideband_pack
      bit_unpack(v->wideband_cqi, &ptr, 4);
      if (cfg->pmi_present) {
        if (cfg->four_antenna_ports) {
          if (cfg->rank_is_not_one) bit_unpack(v->spatial_diff_cqi, &ptr, 3);
          bit_unpack(v->pmi, &ptr, 4);
        } else if (cfg->rank_is_not_one) {
          bit_unpack(v->spatial_diff_cqi, &ptr, 3);
          bit_unpack(v->pmi, &ptr, 1);
        } else {
          bit_unpack(v->pmi, &ptr, 2);
        }
      }
      return (int)(ptr - buff);
    case TYPE_SUBBAND: // cqi_format2_subband_pack: writes the label, returns the 2 of srslte_cqi_size
      bit_unpack(v->subband_cqi, &ptr, 4);
      bit_unpack(v->subband_label, &ptr, cfg->subband_label_2_bits ? 2 : 1);
      return 2;
    case TYPE_SUBBAND_UE: // cqi_ue_subband_pack: the differential fills the position field too, as in the reference
      if (cfg->L > SRSLTE_HIP_CQI_MAX_BITS - 6) return SRSLTE_ERROR_INVALID_INPUTS;
      bit_unpack(v->wideband_cqi, &ptr, 4);
      bit_unpack(v->subband_diff_cqi, &ptr, 2);
      bit_unpack(v->subband_diff_cqi, &ptr, cfg->L);
      return 4 + 2 + (int)cfg->L;
    case TYPE_SUBBAND_HL: { // cqi_hl_subband_pack
      // what does not fit the row: 14 subbands (above 104 PRB) with two codewords and the PMI are 65 bits
      const uint32_t pmi_bits = !cfg->pmi_present ? 0 : cfg->four_antenna_ports ? 4 : cfg->rank_is_not_one ? 1 : 2;
      if (cfg->N > 15 || (4 + 2 * cfg->N) * (cfg->rank_is_not_one ? 2 : 1) + pmi_bits > SRSLTE_HIP_CQI_MAX_BITS) return SRSLTE_ERROR_INVALID_INPUTS;
      int bit_count = 0;
      bit_unpack(v->wideband_cqi, &ptr, 4);
      bit_unpack(v->subband_diff_cqi, &ptr, 2 * cfg->N);
      bit_count += 4 + 2 * (int)cfg->N;
      if (cfg->rank_is_not_one) {
        bit_unpack(v->wideband_cqi_cw1, &ptr, 4);
        bit_unpack(v->subband_diff_cqi_cw1, &ptr, 2 * cfg->N);
        bit_count += 4 + 2 * (int)cfg->N;
      }
      bit_unpack(v->pmi, &ptr, pmi_bits);
      bit_count += (int)pmi_bits;
      return bit_count;
    }
  }
  return SRSLTE_ERROR;
}

int srslte_hip_cqi_periodic_send(uint32_t I_cqi_pmi, uint32_t tti, int tdd)
{
  uint32_t N_p = 0, N_offset = 0;
  if (!(tdd ? get_N_tdd(I_cqi_pmi, &N_p, &N_offset) : get_N_fdd(I_cqi_pmi, &N_p, &N_offset))) return 0;
  return N_p && (tti - N_offset) % N_p == 0 ? 1 : 0;
}

int srslte_hip_cqi_periodic_ri_send(uint32_t I_cqi_pmi, uint32_t I_ri, uint32_t tti, int tdd)
{
  uint32_t M_ri = 0, N_p = 0, N_offset_p = 0;
  int      N_offset_ri = 0;
  if (!(tdd ? get_N_tdd(I_cqi_pmi, &N_p, &N_offset_p) : get_N_fdd(I_cqi_pmi, &N_p, &N_offset_p))) return 0;
  // 36.213 Table 7.2.2-1B
  if (I_ri <= 160) M_ri = 1, N_offset_ri = -(int)I_ri;
  else if (I_ri <= 321) M_ri = 2, N_offset_ri = -(int)(I_ri - 161);
  else if (I_ri <= 482) M_ri = 4, N_offset_ri = -(int)(I_ri - 322);
  else if (I_ri <= 643) M_ri = 8, N_offset_ri = -(int)(I_ri - 483);
  else if (I_ri <= 804) M_ri = 16, N_offset_ri = -(int)(I_ri - 644);
  else if (I_ri <= 965) M_ri = 32, N_offset_ri = -(int)(I_ri - 805);
  else return 0;
  return M_ri && N_p && (tti - N_offset_p - (uint32_t)N_offset_ri) % (N_p * M_ri) == 0 ? 1 : 0;
}

int srslte_hip_cqi_hl_get_no_subbands(int nof_prb) { return hl_no_subbands(nof_prb); }

int srslte_hip_csi_gen_cqi_periodic(const srslte_hip_csi_res_t* csi, srslte_hip_csi_report_cfg_t* cfg, uint32_t wideband_value, uint32_t tti,
                                    srslte_hip_csi_report_t* out)
{
  if (!csi || !cfg || !out) return SRSLTE_ERROR_INVALID_INPUTS;
  memset(out, 0, sizeof(*out));
  if (cfg->periodic_configured && cfg->ri_idx_present && srslte_hip_cqi_periodic_ri_send(cfg->I_cqi_pmi, cfg->I_ri, tti, cfg->tdd)) {
    if (cfg->nof_rx_antennas > 1) {
      if (cfg->tm == 3) select_ri_cn(csi, cfg);
      else if (cfg->tm == 4) select_ri_pmi(csi, cfg, nullptr, nullptr);
    } else {
      cfg->last_ri = 0;
    }
    out->ri_len = 1;
    out->ri     = cfg->last_ri;
  } else if (cfg->periodic_configured && srslte_hip_cqi_periodic_send(cfg->I_cqi_pmi, tti, cfg->tdd)) {
    if (cfg->format_is_subband) {
      out->cqi.type            = TYPE_SUBBAND;
      out->value.subband_cqi   = wideband_value;
      out->value.subband_label = 0;
    } else {
      out->cqi.type           = TYPE_WIDEBAND;
      out->value.wideband_cqi = wideband_value;
      if (cfg->tm == 4) {
        out->cqi.pmi_present     = 1;
        out->cqi.rank_is_not_one = cfg->last_ri != 0;
        out->value.pmi           = select_pmi(csi, cfg, cfg->last_ri) & 0xffu;
      }
    }
    out->cqi.data_enable = 1;
    out->ri_len          = 0;
    out->ri              = cfg->last_ri;
  }
  return finish(out);
}

int srslte_hip_csi_gen_cqi_aperiodic(const srslte_hip_csi_res_t* csi, srslte_hip_csi_report_cfg_t* cfg, uint32_t wideband_value,
                                     srslte_hip_csi_report_t* out)
{
  if (!csi || !cfg || !out) return SRSLTE_ERROR_INVALID_INPUTS;
  memset(out, 0, sizeof(*out));
  const uint32_t N = cfg->nof_prb > 7 ? (uint32_t)hl_no_subbands((int)cfg->nof_prb) : 0;
  switch (cfg->aperiodic_mode) {
    case 30:
      out->cqi.type               = TYPE_SUBBAND_HL;
      out->value.wideband_cqi     = wideband_value;
      out->value.subband_diff_cqi = 0;
      out->cqi.N                  = N;
      out->cqi.data_enable        = 1;
      if (cfg->tm == 3 || cfg->tm == 4) {
        if (cfg->nof_rx_antennas > 1) {
          select_ri_cn(csi, cfg);
          out->ri     = cfg->last_ri & 0xffu;
          out->ri_len = 1;
        } else {
          out->ri = 0;
        }
      } else {
        out->ri_len = 0;
      }
      break;
    case 31: {
      uint32_t pmi     = 0;
      float    sinr_db = 0.0f;
      select_ri_pmi(csi, cfg, &pmi, &sinr_db);
      out->cqi.type               = TYPE_SUBBAND_HL;
      out->value.wideband_cqi     = srslte_hip_cqi_from_snr(sinr_db + cfg->snr_to_cqi_offset);
      out->value.subband_diff_cqi = 0;
      if (cfg->last_ri > 0) {
        out->cqi.rank_is_not_one        = 1;
        out->value.wideband_cqi_cw1     = srslte_hip_cqi_from_snr(sinr_db + cfg->snr_to_cqi_offset);
        out->value.subband_diff_cqi_cw1 = 0;
      }
      out->value.pmi              = pmi;
      out->cqi.pmi_present        = 1;
      out->cqi.four_antenna_ports = cfg->nof_ports == 4;
      out->cqi.N                  = N;
      out->cqi.data_enable        = 1;
      out->ri_len                 = 1;
      out->ri                     = cfg->last_ri;
      break;
    }
    default:
      hip_log("[srslte_hip] csi: aperiodic CQI mode %d not supported (30 or 31)\n", cfg->aperiodic_mode);
      return SRSLTE_ERROR_INVALID_INPUTS;
  }
  return finish(out);
}

} // extern "C"
