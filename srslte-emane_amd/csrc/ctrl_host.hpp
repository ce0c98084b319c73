// Host tables of the DL control region, shared by the receiver (pdcch.hip) and the encoder (pdcch_tx.hip): the REG lists of regs.c and the
// scrambling sequences of the PCFICH, PHICH and PDCCH (sequences.c), for one cell.
#pragma once
#include "srslte_hip/phy_hip.h"
#include <stdint.h>
#include <vector>

struct CtrlRegs {
  std::vector<uint32_t> pcfich;   // the 16 PCFICH REs in srslte_regs_pcfich_put order
  std::vector<uint32_t> pdcch[3]; // the 36 NOF_CCE(cfi) PDCCH REs of CFI 1-3 in srslte_regs_pdcch_put order
  std::vector<uint32_t> phich;    // [ngroups_m1][12]: the REs of each PHICH mapping unit in srslte_regs_phich_add order
  uint32_t              ngroups_m1 = 0; // mapping units (srslte_regs_phich_ngroups_m1); PHICH groups: that, x 2 on an extended-CP cell
};

// the cell description of srslte_hip_dl_ctrl_cfg_t is one srslte_regs_init accepts (TDD and nof_rx_antennas are not looked at)
bool ctrl_cell_ok(const srslte_hip_dl_ctrl_cfg_t* c);

// srslte_regs_init_opts with mi = 1 outside MBSFN / TDD special subframes (regs.c:698-786, REGs :633-675, PCFICH :491-523, PHICH :245-367,
// PDCCH :77-154), as RE indices of one port's [nsym][12 prb] grid
int ctrl_build_regs(const srslte_hip_dl_ctrl_cfg_t* c, CtrlRegs& r);

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
