// Host tables of the DL control region (ctrl_host.hpp): REG lists and scrambling sequences, shared by pdcch.hip and pdcch_tx.hip, and the
// PSS / SSS / PBCH tables of pbch.hip.
#include "ctrl_host.hpp"
#include "common.hpp"
#include "phy_hip_internal.hpp"
#include <math.h>
#include <string.h>

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

int ctrl_build_regs(const srslte_hip_dl_ctrl_cfg_t* c, CtrlRegs& out) { return ctrl_build_regs_opts(c, 1, false, out); }

int ctrl_build_regs_opts(const srslte_hip_dl_ctrl_cfg_t* c, uint32_t phich_mi, bool sf1_6, CtrlRegs& out)
{
  if (!ctrl_cell_ok(c) || phich_mi > 2) return SRSLTE_ERROR_INVALID_INPUTS;
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
  // PHICH: mapping unit mi takes REG q = 0, 1, 2 in this order (regs.c:320-340); with an extended PHICH in subframes 1 and 6 of a TDD cell
  // the REGs alternate between symbols 0 and 1 and the cell offset is scaled by symbol 1's count (regs.c:325-335)
  const float    ng[4]   = {(float)1 / 6, (float)1 / 2, 1.0f, 2.0f};
  const uint32_t ngroups = (uint32_t)(int)ceilf(ng[c->phich_resources] * ((float)prb / 8));
  std::vector<Reg*> ph[3];
  for (auto& r : regs)
    if (r.l < 3 && !r.assigned) ph[r.l].push_back(&r);
  const bool two_sym = c->phich_ext && sf1_6;
  out.ngroups_m1 = ngroups;
  out.units      = phich_mi * ngroups;
  out.shared     = false;
  out.phich.clear();
  for (uint32_t mi = 0; mi < out.units; mi++) {
    for (uint32_t q = 0; q < 3; q++) {
      const uint32_t li = !c->phich_ext ? 0 : two_sym ? (mi / 2 + q + 1) % 2 : q, nl = (uint32_t)ph[li].size();
      const uint32_t ni = ((id * nl / (uint32_t)ph[two_sym ? 1 : 0].size()) + mi + q * nl / 3) % nl;
      if (ph[li][ni]->assigned) out.shared = true;
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

int ctrl_tdd_mi(uint32_t tdd_sf_config, uint32_t sf_idx)
{
  // 36.213 Table 6.9-1 on the downlink and special subframes of 36.211 Table 4.2-2; -1: uplink
  static const int8_t MI[7][10] = {{2, 1, -1, -1, -1, 2, 1, -1, -1, -1}, {0, 1, -1, -1, 1, 0, 1, -1, -1, 1}, {0, 0, -1, 1, 0, 0, 0, -1, 1, 0},
                                   {1, 0, -1, -1, -1, 0, 0, 0, 1, 1},   {0, 0, -1, -1, 0, 0, 0, 0, 1, 1},   {0, 0, -1, 0, 0, 0, 0, 0, 1, 0},
                                   {1, 1, -1, -1, -1, 1, 1, -1, -1, 1}};
  return tdd_sf_config <= 6 && sf_idx < 10 ? MI[tdd_sf_config][sf_idx] : -1;
}

int ctrl_build_regs_set(const srslte_hip_dl_ctrl_cfg_t* c, int tdd_sf_config, CtrlRegsSet& s)
{
  if (!ctrl_cell_ok(c) || tdd_sf_config > 6) return SRSLTE_ERROR_INVALID_INPUTS;
  s.v.clear();
  if (tdd_sf_config < 0) {
    s.v.resize(1);
    memset(s.var, 0, sizeof(s.var));
    const int r    = ctrl_build_regs(c, s.v[0]);
    s.max_pdcch_re = (uint32_t)s.v[0].pdcch[2].size();
    return r;
  }
  CtrlRegs mi0;
  if (int r = ctrl_build_regs_opts(c, 0, false, mi0)) return r;
  s.max_pdcch_re = (uint32_t)mi0.pdcch[2].size();
  int key[CTRL_MAX_VAR];
  for (uint32_t sf = 0; sf < 10; sf++) {
    const int mi = ctrl_tdd_mi((uint32_t)tdd_sf_config, sf);
    s.var[sf]    = CTRL_SF_UL;
    if (mi < 0) continue;
    // without PHICH REGs (mi = 0) or with a normal PHICH the rule of subframes 1 and 6 changes nothing: one variant serves both
    const int k = mi | ((mi > 0 && c->phich_ext && (sf == 1 || sf == 6)) ? 4 : 0);
    size_t    i = 0;
    while (i < s.v.size() && key[i] != k) i++;
    if (i == s.v.size()) {
      if (i == (size_t)CTRL_MAX_VAR) return SRSLTE_ERROR;
      key[i] = k;
      s.v.emplace_back();
      if (int r = ctrl_build_regs_opts(c, (uint32_t)mi, (k & 4) != 0, s.v.back())) return r;
      if (s.v.back().shared || s.v.back().pdcch[0].size() < 36) return SRSLTE_ERROR;
    }
    s.var[sf] = (uint8_t)i;
  }
  return SRSLTE_SUCCESS;
}

uint32_t CtrlRegsSet::max_units() const
{
  uint32_t m = 0;
  for (const CtrlRegs& r : v) m = r.units > m ? r.units : m;
  return m;
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

void bcast_build(uint32_t nof_prb, uint32_t cell_id, int cp_ext, BcastHost& b)
{
  const uint32_t w = 12 * nof_prb, nsym = cp_ext ? 6 : 7, v = cell_id % 3;
  // srslte_pbch_cp with put = true: the output walks slot 1 from the first RE of the six central PRBs. A symbol with reference signals takes
  // v REs, then 23 times (skip one, take two), then (skip one, take 2 - v) when 2 - v > 0: the CRS positions of four ports are never used.
  // After each of the first two symbols the walk moves on by w - 72, plus one when v == 2 (the last skip did not happen). Symbols 2 and 3
  // are taken whole on a normal-CP cell; on an extended-CP cell symbol 2 is, and symbol 3 (which carries CRS) is walked like symbol 0
  b.pbch_re.clear();
  uint32_t out = nsym * w + w / 2 - 36;
  auto     ref_sym = [&](bool advance) {
    for (uint32_t i = 0; i < v; i++) b.pbch_re.push_back(out++);
    for (int i = 0; i < 23; i++) {
      out++;
      b.pbch_re.push_back(out++), b.pbch_re.push_back(out++);
    }
    if (2 > v) {
      out++;
      for (uint32_t i = 0; i < 2 - v; i++) b.pbch_re.push_back(out++);
    }
    if (advance) out += w - 72 + (v == 2 ? 1 : 0);
  };
  auto full_sym = [&]() {
    for (int i = 0; i < 72; i++) b.pbch_re.push_back(out++);
    out += w - 72;
  };
  ref_sym(true);
  ref_sym(true);
  full_sym();
  if (cp_ext) {
    ref_sym(false);
  } else {
    full_sym();
  }
  b.nof_bits = cp_ext ? 432 : 480;
  // PSS in the last, SSS in the second-to-last symbol of slot 0, 62 values around DC with five zeros on each side
  b.pss_k0 = (nsym - 1) * w + w / 2 - 31 - 5;
  b.sss_k0 = (nsym - 2) * w + w / 2 - 31 - 5;
  memset(b.pss, 0, sizeof(b.pss));
  memset(b.sss, 0, sizeof(b.sss));
  // srslte_pss_generate (36.211 6.11.1.1): Zadoff-Chu of root 25 / 29 / 34; the phase is formed in double as the reference's expression
  // promotes it, rounded to float, then cosf / sinf
  const float root = v == 0 ? 25.0f : v == 1 ? 29.0f : 34.0f;
  for (int i = 0; i < 62; i++) {
    const float fi  = (float)i;
    float       arg = (float)((float)-1 * M_PI * root * (i < 31 ? fi * (fi + 1.0) : (fi + 2.0) * (fi + 1.0)) / 63.0);
    if (arg == 0.f) arg = 0.f; // i = 0: the reference's build (-Ofast, no signed zeros) has sinf(+0), not sinf(-0)
    b.pss[5 + i][0] = cosf(arg);
    b.pss[5 + i][1] = sinf(arg);
  }
  // srslte_sss_generate (36.211 6.11.2.1): the m-sequences s~, c~, z~ of x^5 + x^2 + 1, x^5 + x^3 + 1, x^5 + x^4 + x^2 + x + 1; as in gen_sss.c,
  // c0 is c~ shifted by N_id_2 and c1 by N_id_2 + 3
  int st[31], ct[31], zt[31], x[31];
  const int taps[3][4] = {{2, 0, -1, -1}, {3, 0, -1, -1}, {4, 2, 1, 0}};
  int*      dst[3]     = {st, ct, zt};
  for (int s = 0; s < 3; s++) {
    memset(x, 0, sizeof(x));
    x[4] = 1;
    for (int i = 0; i < 26; i++) {
      int t = 0;
      for (int j = 0; j < 4; j++)
        if (taps[s][j] >= 0) t += x[i + taps[s][j]];
      x[i + 5] = t % 2;
    }
    for (int i = 0; i < 31; i++) dst[s][i] = 1 - 2 * x[i];
  }
  const uint32_t id1 = cell_id / 3, qp = id1 / 30, q = (id1 + qp * (qp + 1) / 2) / 30, mp = id1 + q * (q + 1) / 2;
  const uint32_t m0 = mp % 31, m1 = (m0 + mp / 31 + 1) % 31;
  for (int i = 0; i < 31; i++) {
    const int s0 = st[(i + m0) % 31], s1 = st[(i + m1) % 31], c0 = ct[(i + v) % 31], c1 = ct[(i + v + 3) % 31];
    const int z0 = zt[(i + m0 % 8) % 31], z1 = zt[(i + m1 % 8) % 31];
    b.sss[0][5 + 2 * i] = (float)(s0 * c0), b.sss[0][5 + 2 * i + 1] = (float)(s1 * c1 * z0);
    b.sss[1][5 + 2 * i] = (float)(s1 * c0), b.sss[1][5 + 2 * i + 1] = (float)(s0 * c1 * z1);
  }
  // srslte_sequence_pbch: c_init = cell_id, 1920 / 1728 bits
  std::vector<uint8_t> c;
  lte_gold_sequence(cell_id, 4 * b.nof_bits, c);
  b.scr.assign((4 * b.nof_bits + 31) / 32, 0u);
  for (uint32_t i = 0; i < 4 * b.nof_bits; i++) b.scr[i >> 5] |= (uint32_t)(c[i] & 1) << (i & 31);
}

uint32_t mib_head(uint32_t nof_prb, int phich_ext, int phich_resources)
{
  const uint32_t bw = nof_prb <= 6 ? 0 : nof_prb <= 15 ? 1 : 1 + nof_prb / 25;
  return (bw & 7) << 3 | (phich_ext ? 1u : 0u) << 2 | ((uint32_t)phich_resources & 3);
}
