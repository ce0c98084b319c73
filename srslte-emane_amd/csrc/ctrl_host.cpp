// Host tables of the DL control region (ctrl_host.hpp): REG lists and scrambling sequences, shared by pdcch.hip and pdcch_tx.hip.
#include "ctrl_host.hpp"
#include "common.hpp"
#include "phy_hip_internal.hpp"
#include <math.h>

namespace {
struct Reg {
  uint32_t l, k0, k[4];
  bool     assigned;
};
} // namespace

bool ctrl_cell_ok(const srslte_hip_dl_ctrl_cfg_t* c)
{
  return c && c->nof_prb >= 6 && c->nof_prb <= 110 && (c->nof_ports == 1 || c->nof_ports == 2 || c->nof_ports == 4) && c->cell_id < 504 &&
         c->phich_resources >= 0 && c->phich_resources <= 3;
}

int ctrl_build_regs(const srslte_hip_dl_ctrl_cfg_t* c, CtrlRegs& out)
{
  if (!ctrl_cell_ok(c)) return SRSLTE_ERROR_INVALID_INPUTS;
  const uint32_t prb = c->nof_prb, id = c->cell_id, max_ctrl = prb <= 10 ? 4 : 3, vo = id % 3;
  uint32_t       n[4];
  for (uint32_t i = 0; i < max_ctrl; i++) n[i] = i == 0 ? 2 : i == 1 ? (c->nof_ports == 4 ? 2 : 3) : i == 2 ? 3 : (c->cp_ext ? 2 : 3);
  uint32_t nof_regs = 0;
  for (uint32_t i = 0; i < max_ctrl; i++) nof_regs += prb * n[i];
  std::vector<Reg> regs(nof_regs);
  uint32_t         j[4] = {0, 0, 0, 0}, k = 0, i = 0, p = 0, jmax = 0;
  while (k < nof_regs) { // lowest symbol first, then frequency, PRB by PRB
    if (n[i] == 3 || (n[i] == 2 && jmax != 1)) {
      Reg& r = regs[k];
      r.l = i, r.assigned = false;
      const uint32_t b0 = p * 12;
      if (n[i] == 2) { // two REGs around the reference signals at vo, vo + 3
        r.k0 = b0 + j[i] * 6;
        uint32_t t = 0;
        for (uint32_t z = 0; z < 6; z++)
          if (z != vo && z != vo + 3) r.k[t++] = r.k0 + z;
      } else {
        r.k0 = b0 + j[i] * 4;
        for (uint32_t z = 0; z < 4; z++) r.k[z] = r.k0 + z;
      }
      j[i]++, k++;
    }
    if (++i == max_ctrl) i = 0, jmax++;
    if (jmax == 3) p++, j[0] = j[1] = j[2] = j[3] = 0, jmax = 0;
  }
  auto re_of = [prb](const Reg& r, uint32_t t) { return r.k[t] + r.l * prb * 12; };
  // PCFICH
  out.pcfich.clear();
  const uint32_t k_hat = 6 * (id % (2 * prb));
  for (uint32_t q = 0; q < 4; q++) {
    const uint32_t kk = (k_hat + (q * prb / 2) * 6) % (prb * 12);
    Reg*           f  = nullptr;
    for (auto& r : regs)
      if (r.l == 0 && r.k0 == kk) {
        f = &r;
        break;
      }
    if (!f || f->assigned) return SRSLTE_ERROR;
    f->assigned = true;
    for (uint32_t t = 0; t < 4; t++) out.pcfich.push_back(re_of(*f, t));
  }
  // PHICH: mapping unit mi takes REG q = 0, 1, 2 in this order (regs.c:320-340)
  const float    ng[4]   = {(float)1 / 6, (float)1 / 2, 1.0f, 2.0f};
  const uint32_t ngroups = (uint32_t)(int)ceilf(ng[c->phich_resources] * ((float)prb / 8));
  std::vector<Reg*> ph[3];
  for (auto& r : regs)
    if (r.l < 3 && !r.assigned) ph[r.l].push_back(&r);
  out.ngroups_m1 = ngroups;
  out.phich.clear();
  for (uint32_t mi = 0; mi < ngroups; mi++) {
    for (uint32_t q = 0; q < 3; q++) {
      const uint32_t li = c->phich_ext ? q : 0, nl = (uint32_t)ph[li].size();
      const uint32_t ni = ((id * nl / (uint32_t)ph[0].size()) + mi + q * nl / 3) % nl;
      ph[li][ni]->assigned = true;
      for (uint32_t t = 0; t < 4; t++) out.phich.push_back(re_of(*ph[li][ni], t));
    }
  }
  // PDCCH: quadruplet sub-block interleaver (32 columns, PDCCH_PERM) and the cyclic shift by the cell id
  static const uint8_t PERM[32] = {1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31, 0, 16, 8, 24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30};
  for (uint32_t cfi = 0; cfi < 3; cfi++) {
    const uint32_t    nsym = prb <= 10 ? cfi + 2 : cfi + 1;
    std::vector<Reg*> tmp;
    for (auto& r : regs)
      if (r.l < nsym && !r.assigned) tmp.push_back(&r);
    const uint32_t    m = (uint32_t)tmp.size(), nrows = (m - 1) / 32 + 1;
    const int         ndummy = (int)(32 * nrows) - (int)m;
    std::vector<Reg*> perm(m);
    uint32_t          kk = 0;
    for (uint32_t jj = 0; jj < 32; jj++) {
      for (uint32_t ii = 0; ii < nrows; ii++) {
        if ((int)(ii * 32 + PERM[jj]) >= ndummy) {
          const uint32_t mm = ii * 32 + PERM[jj] - ndummy;
          const uint32_t kp = kk < id ? (m + kk - (id % m)) % m : (kk - id) % m;
          perm[mm]          = tmp[kp];
          kk++;
        }
      }
    }
    out.pdcch[cfi].clear();
    for (uint32_t r = 0; r < (m / 9) * 9; r++)
      for (uint32_t t = 0; t < 4; t++) out.pdcch[cfi].push_back(re_of(*perm[r], t));
  }
  return SRSLTE_SUCCESS;
}

void ctrl_scrambling(uint32_t cell_id, uint32_t pdcch_bits, std::vector<uint32_t>& scr, int* scr_words)
{
  const int w = (int)(pdcch_bits + 31) / 32;
  scr.assign(10 + 10 * (size_t)w, 0u);
  std::vector<uint8_t> c;
  for (uint32_t s = 0; s < 10; s++) {
    lte_gold_sequence((s + 1) * (2 * cell_id + 1) * 512 + cell_id, 32, c);
    for (int i = 0; i < 32; i++) scr[s] |= (uint32_t)(c[i] & 1) << i;
    lte_gold_sequence(s * 512 + cell_id, pdcch_bits, c);
    for (uint32_t i = 0; i < pdcch_bits; i++) scr[10 + s * w + (i >> 5)] |= (uint32_t)(c[i] & 1) << (i & 31);
  }
  *scr_words = w;
}
