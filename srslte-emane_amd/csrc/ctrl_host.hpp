// Host tables of the DL control region, shared by the receiver (pdcch.hip) and the encoder (pdcch_tx.hip): the REG lists of regs.c and the
// scrambling sequences of the PCFICH, PHICH and PDCCH (sequences.c), for one cell.
#pragma once
#include "srslte_hip/phy_hip.h"
#include <stdint.h>
#include <vector>

struct CtrlRegs {
  std::vector<uint32_t> pcfich;   // the 16 PCFICH REs in srslte_regs_pcfich_put order
  std::vector<uint32_t> pdcch[3]; // the 36 NOF_CCE(cfi) PDCCH REs of CFI 1-3 in srslte_regs_pdcch_put order
  std::vector<uint32_t> phich;    // [units][12]: the REs of each PHICH mapping unit in srslte_regs_phich_add order
  uint32_t              ngroups_m1 = 0; // srslte_regs_phich_ngroups_m1, what srslte_phich_calc takes
  uint32_t              units = 0;      // mapping units: mi ngroups_m1 (mi = 1 on an FDD cell); PHICH groups: that, x 2 on an extended-CP cell
  bool                  shared = false; // a REG lies in two mapping units (the reference maps both onto it when the cell is too small)
};

// the cell description of srslte_hip_dl_ctrl_cfg_t is one srslte_regs_init accepts (TDD and nof_rx_antennas are not looked at)
bool ctrl_cell_ok(const srslte_hip_dl_ctrl_cfg_t* c);

// srslte_regs_init_opts with mi = 1 outside MBSFN / TDD special subframes (regs.c:698-786, REGs :633-675, PCFICH :491-523, PHICH :245-367,
// PDCCH :77-154), as RE indices of one port's [nsym][12 prb] grid
int ctrl_build_regs(const srslte_hip_dl_ctrl_cfg_t* c, CtrlRegs& r);
// srslte_regs_init_opts(cell, mi, sf1_6) of a TDD cell: mi = 0 leaves every REG but the PCFICH's to the PDCCH, mi = 2 doubles the mapping
// units, sf1_6 is the two-symbol rule of an extended PHICH in subframes 1 and 6 (regs.c:325-335)
int ctrl_build_regs_opts(const srslte_hip_dl_ctrl_cfg_t* c, uint32_t mi, bool sf1_6, CtrlRegs& r);

// The REG lists of every subframe of a frame. FDD (tdd_sf_config < 0): one variant for all ten. TDD: one per (mi, sf1_6) the uplink-downlink
// configuration uses, MI_IDX of ue_dl.c:57-62 with the duplicates folded; var[sf_idx] is the subframe's variant, CTRL_SF_UL for an uplink
// subframe (36.211 Table 4.2-2). No configuration uses more than CTRL_MAX_VAR variants (mi = 0, mi = 1 and mi = 1 with sf1_6 in
// configuration 1; mi = 2 occurs in configuration 0 alone, beside mi = 1 or mi = 1 with sf1_6)
constexpr int     CTRL_MAX_VAR = 3;
constexpr uint8_t CTRL_SF_UL   = 0xff;
struct CtrlRegsSet {
  std::vector<CtrlRegs> v;
  uint8_t               var[10];
  uint32_t              max_pdcch_re; // the longest PDCCH RE list. TDD: CFI 3 with mi = 0, whether the configuration has such a subframe or not,
                                      // as the reference sets its PDCCH up on regs[1] (ue_dl.c:197-226)
  uint32_t max_units() const;
};
// mi of 36.213 Table 6.9-1 (mi_tdd_table, ue_dl.c:49-55); < 0 for an uplink subframe or an invalid configuration / subframe
int ctrl_tdd_mi(uint32_t tdd_sf_config, uint32_t sf_idx);
// SRSLTE_ERROR_INVALID_INPUTS for an invalid cell or configuration; SRSLTE_ERROR for a TDD cell and configuration the control objects do not
// serve: a variant has a REG in two PHICH mapping units, or its PHICH leaves fewer than nine REGs, no CCE, to a CFI-1 region
int ctrl_build_regs_set(const srslte_hip_dl_ctrl_cfg_t* c, int tdd_sf_config, CtrlRegsSet& s);

// srslte_sequence_pcfich (32 bits; its first 12 are srslte_sequence_phich, the same c_init: sequences.c:36-46) and srslte_sequence_pdcch of
// pdcch_bits bits (sequences.c:51-53) of subframes 0-9, packed bit i -> word i / 32, bit i % 32: scr = [10 PCFICH words][10][scr_words]
void ctrl_scrambling(uint32_t cell_id, uint32_t pdcch_bits, std::vector<uint32_t>& scr, int* scr_words);

// srslte_phich_calc (phich.c:132-143) for the transmit (pdcch_tx.hip) and the receive side (phich.hip): Ngroups is
// srslte_regs_phich_ngroups_m1, nsf 4 (normal CP) or 2 (extended)
inline void phich_calc(uint32_t ng_m1, int cp_ext, uint32_t n_prb_lowest, uint32_t n_dmrs, uint32_t I_phich, uint32_t* ngroup, uint32_t* nseq)
{
  *ngroup = (n_prb_lowest + n_dmrs) % ng_m1 + I_phich * ng_m1;
  *nseq   = ((n_prb_lowest / ng_m1) + n_dmrs) % (2 * (cp_ext ? 2u : 4u));
}

// Broadcast channels of one cell (pbch.hip): the RE list of srslte_pbch_cp (pbch.c:54-101) as indices into one port's [nsym][12 prb] grid
// of the subframe (slot 1), the 72 REs of the PSS and of the SSS with their zero guards (pss.c:380-386, sss.c:106-119) and their values,
// srslte_sequence_pbch (4 nof_bits bits) packed bit i -> word i / 32, bit i % 32
struct BcastHost {
  std::vector<uint32_t> pbch_re;      // 240 (normal CP) / 216 (extended) in srslte_pbch_put order
  uint32_t              pss_k0, sss_k0; // first RE of the 72 (5 guards, 62 values, 5 guards) of each signal in slot 0
  float                 pss[72][2];   // srslte_pss_generate(cell_id % 3) with the guards
  float                 sss[2][72];   // srslte_sss_generate's signal0 / signal5 with the guards (real parts; the imaginary parts are 0)
  std::vector<uint32_t> scr;          // srslte_sequence_pbch
  uint32_t              nof_bits;     // 480 / 432
};
void bcast_build(uint32_t nof_prb, uint32_t cell_id, int cp_ext, BcastHost& b);

// srslte_pbch_mib_pack (pbch.c:318-354) without the SFN: the first 6 bits (bandwidth, PHICH length, PHICH resources) as an integer, MSB first
uint32_t mib_head(uint32_t nof_prb, int phich_ext, int phich_resources);
