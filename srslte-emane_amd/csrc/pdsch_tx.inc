// Fragment of pdsch.hip (same translation unit): the PDSCH transmit pipeline (eNB side), fixed-grant and per-PDSCH grants.
// ====================================================================================================================
// PDSCH transmit pipeline (eNB side; SURVEY §3.2): srslte_pdsch_encode (pdsch.c:1059-1185: DL-SCH coding sch.c:183-297 with the
// Qm * N_L block split :549-575, scrambling, modulation, layer mapping + SFBC precoding, RE mapping) + CRS (srslte_refsignal_cs_put_sf,
// refsignal_dl.c:253-272) + srslte_ofdm_tx_sf with 1/sqrt(N) (enb_dl.c:56-62). One codeword, TM1 or 2-port TM2, full-band grant;
// the per-PDSCH grants mode also with two codewords, large-delay CDD and codebook precoding on a 2-port cell (TM3 / TM4).
// Re-uses the PUSCH transmit kernels for CRC attachment / segmentation and the byte-stream turbo encoder.
// ====================================================================================================================
namespace {

struct PdschTxGeom {
  SfClass cls[3];
  const int32_t* src[3][4]; // per subframe class and port: grid RE -> >= 0 index into the port's symbol stream, -1 zero, <= -2 CRS pilot -(v + 2)
  int   grid_len, max_re, Qm, Nl, nof_ports, tti0, scr_words, C, K, cb_stride, par_stride, rm_len;
  float lvl[16], gain; // constellation levels of one axis; rho_a (TM1) or rho_a / sqrt(2) (TM2)
  // TDD cell (grants mode): special subframes - 1, and 6 when tdd_s6 - take the map with the CRS symbols of their DwPTS only; tdd_s6 < 0: FDD
  const int32_t* src_sp[4];
  int   tdd_s6;
  // MBSFN subframes (cfg.mbsfn): map values <= -2 - MBSFN_REF point into the area's reference signal [10][3][6 nof_prb] (chest.hip)
  const cf32* mbsfn_pilots;
  int   mbsfn_nref; // 18 nof_prb
};
constexpr int MBSFN_REF = 1 << 24;

// Symbol i of a transport block on nre REs -> the indices of its two levels: its Qm coded bits - bit e of a code block = coded bit
// rm[e mod (3K+12)] in the encoder's byte streams, as in pusch_tx_mod_kernel; the block split in units of Qm * Nl bits - scrambled with cs. Shared by every
// modulation kernel of the transmit side.
__device__ __forceinline__ void pdsch_tx_sym_bits(const uint8_t* __restrict__ cb, const uint8_t* __restrict__ parity, const uint8_t* __restrict__ sys_tail,
                                                  const uint32_t* __restrict__ rm, const uint32_t* __restrict__ cs, int cb_stride, int par_stride, int i, int Nl,
                                                  int nre, int cb0, int C, int Qm, int rm_len, int& re, int& im)
{
  const int Gp = nre / Nl; // Gp = G' of 36.212 5.1.4.1.2
  const int QmL = Qm * Nl, gamma = Gp % C, lo = Gp / C, C_lo = C - gamma; // blocks 0..C_lo-1 carry lo units, the rest lo + 1 (sch.c:232-236)
  const int u = i / Nl; // split unit
  int       r, e0;
  if (u < C_lo * lo) {
    r  = u / lo;
    e0 = (u - r * lo) * QmL;
  } else {
    const int v = u - C_lo * lo;
    r           = C_lo + v / (lo + 1);
    e0          = (v % (lo + 1)) * QmL;
  }
  e0 += (i % Nl) * Qm;
  const size_t   cbi = (size_t)cb0 + r;
  const uint8_t *xb = cb + cbi * cb_stride, *pb = parity + cbi * par_stride;
  const int      q0 = i * Qm;
  re = 0;
  im = 0;
  for (int b = 0; b < Qm; b++) {
    const uint32_t src = rm[(e0 + b) % rm_len], pos = src & 0x3fffffffu;
    const uint8_t  byte = (src >> 30) == 0 ? xb[pos >> 3] : ((src >> 30) == 1 ? sys_tail[cbi] : pb[pos >> 3]);
    int            bit  = (byte >> (7 - (pos & 7))) & 1;
    bit ^= (cs[(q0 + b) >> 5] >> ((q0 + b) & 31)) & 1;
    if (b & 1) im = (im << 1) | bit;
    else re = (re << 1) | bit;
  }
}

// grid = (ceil(max_re / (256 * G)), nof_sf), G = nof_ports: one thread per precoding group (one symbol for TM1, the SFBC pair 2i, 2i+1 for
// 2 ports, four symbols for 4 ports). The block split counts in units of Qm * N_L bits (N_L = 2 with transmit diversity). y: [nof_sf][nof_ports][max_re].
// One transport block: nre symbols in precoding groups of G = nof_ports; cs: its scrambling bits; cb0: its first code-block slot; C / Qm / rm_len /
// lvl: of ITS segmentation and modulation; y0: its [nof_ports][max_re] symbol streams.
__device__ __forceinline__ void pdsch_tx_mod_body(const uint8_t* __restrict__ cb, const uint8_t* __restrict__ parity, const uint8_t* __restrict__ sys_tail,
                                                  const uint32_t* __restrict__ rm, const uint32_t* __restrict__ cs, cf32* __restrict__ y0, const PdschTxGeom& g,
                                                  int grp, int nre, int cb0, int C, int Qm, int rm_len, const float* __restrict__ lvl)
{
  const int G = g.nof_ports;
  if (grp * G >= nre) return;
  cf32            d[4];
  for (int t = 0; t < G; t++) {
    int re, im;
    pdsch_tx_sym_bits(cb, parity, sys_tail, rm, cs, g.cb_stride, g.par_stride, grp * G + t, g.Nl, nre, cb0, C, Qm, rm_len, re, im);
    d[t] = make_float2(lvl[re] * g.gain, lvl[im] * g.gain);
  }
  const cf32 z  = make_float2(0.f, 0.f);
  if (G == 1) {
    y0[grp] = d[0];
  } else if (G == 2) { // srslte_precoding_diversity, 2 ports (precoding.c:1851-1861): y0 = x0, x1; y1 = -x1*, x0*
    cf32* y1        = y0 + g.max_re;
    y0[2 * grp]     = d[0];
    y0[2 * grp + 1] = d[1];
    y1[2 * grp]     = make_float2(-d[1].x, d[1].y);
    y1[2 * grp + 1] = make_float2(d[0].x, -d[0].y);
  } else { // 4 ports (precoding.c:1862-1890): ports 0/2 on sub-carriers 4i, 4i+1, ports 1/3 on 4i+2, 4i+3, the others silent
    cf32 *y1 = y0 + g.max_re, *y2 = y1 + g.max_re, *y3 = y2 + g.max_re;
    const int k = 4 * grp;
    y0[k] = d[0];     y1[k] = z;        y2[k] = make_float2(-d[1].x, d[1].y);     y3[k] = z;
    y0[k + 1] = d[1]; y1[k + 1] = z;    y2[k + 1] = make_float2(d[0].x, -d[0].y); y3[k + 1] = z;
    y0[k + 2] = z;    y1[k + 2] = d[2]; y2[k + 2] = z; y3[k + 2] = make_float2(-d[3].x, d[3].y);
    y0[k + 3] = z;    y1[k + 3] = d[3]; y2[k + 3] = z; y3[k + 3] = make_float2(d[2].x, -d[2].y);
  }
}


__global__ __launch_bounds__(256) void pdsch_tx_mod_kernel(const uint8_t* __restrict__ cb, const uint8_t* __restrict__ parity,
                                                           const uint8_t* __restrict__ sys_tail, const uint32_t* __restrict__ rm,
                                                           const uint32_t* __restrict__ scr, cf32* __restrict__ y, PdschTxGeom g)
{
  const int sf = blockIdx.y, sf_idx = (g.tti0 + sf) % 10, nre = g.cls[sf_class(sf_idx)].nof_re, grp = blockIdx.x * blockDim.x + threadIdx.x;
  if (grp * g.nof_ports >= nre) return;
  pdsch_tx_mod_body(cb, parity, sys_tail, rm, scr + (size_t)sf_idx * g.scr_words, y + ((size_t)sf * g.nof_ports) * g.max_re, g, grp, nre, sf * g.C, g.C, g.Qm,
                    g.rm_len, g.lvl);
}

// ---- per-PDSCH grants on the transmit side (srslte_hip_dl_tx_batch_grants): PDSCH p of a call has its own allocation, RNTI, modulation, transport
// block and redundancy version; several may share a subframe's grid
struct TxDesc {
  int             row, sf;             // row of the caller's d_tb; subframe of the batch
  int             tbs, C, K, rlenB;    // segmentation of its transport block
  int             cb0;                 // its first code-block slot (slots have the strides of the largest block size)
  int             nre, mod, Qm;
  const uint32_t* rm;                  // rate-matching table of (K, rv)
  // descriptor of a PDSCH's codeword 0 (srslte_hip_dl_tx_batch_grants2): srslte_tx_scheme_t, the precoder's codebook index (pdsch.c:1152), and
  // the descriptor of its codeword 1 (-1: one transport block)
  int             scheme, codebook, cw1;
};

// grid = nof_pdsch: CRC24A of each transport block
__global__ __launch_bounds__(256) void tx_tbcrc_grants_kernel(const uint8_t* __restrict__ tb, int tb_stride, const TxDesc* __restrict__ desc,
                                                              uint32_t* __restrict__ crc_out)
{
  __shared__ uint32_t tab[256], red[256];
  const uint8_t*      x = tb + (size_t)desc[blockIdx.x].row * tb_stride;
  const uint32_t      c = block_crc24([&](int i) { return (uint32_t)x[i]; }, desc[blockIdx.x].tbs / 8, 0x1864CFBu, tab, red);
  if (threadIdx.x == 0) crc_out[blockIdx.x] = c;
}

// grid = (Cmax, nof_pdsch): segmentation + CRC24B as pusch_tx_seg_kernel, per descriptor
__global__ __launch_bounds__(256) void tx_seg_grants_kernel(const uint8_t* __restrict__ tb, int tb_stride, const uint32_t* __restrict__ tbcrc,
                                                            const TxDesc* __restrict__ desc, uint8_t* __restrict__ cb, int cb_stride)
{
  __shared__ uint32_t tab[256], red[256];
  __shared__ uint8_t  xs[768];
  const TxDesc&       d = desc[blockIdx.y];
  const int           r = blockIdx.x, t = threadIdx.x, tbB = d.tbs / 8, rlenB = d.rlenB;
  if (r >= d.C) return;
  const uint8_t* x   = tb + (size_t)d.row * tb_stride;
  const uint32_t crc = tbcrc[blockIdx.y];
  uint8_t*       out = cb + ((size_t)d.cb0 + r) * cb_stride;
  for (int i = t; i < rlenB; i += 256) {
    const int j = r * rlenB + i;
    xs[i]       = j < tbB ? x[j] : (uint8_t)(crc >> (8 * (2 - (j - tbB))));
  }
  __syncthreads();
  for (int i = t; i < rlenB; i += 256) out[i] = xs[i];
  if (d.C > 1) {
    const uint32_t c = block_crc24([&](int i) { return (uint32_t)xs[i]; }, rlenB, 0x1800063u, tab, red);
    if (t < 3) out[rlenB + t] = (uint8_t)(c >> (8 * (2 - t)));
  }
}

// grid = (ceil(max_re / (256 * G)), nof_pdsch)
__global__ __launch_bounds__(256) void pdsch_tx_mod_grants_kernel(const uint8_t* __restrict__ cb, const uint8_t* __restrict__ parity,
                                                                  const uint8_t* __restrict__ sys_tail, const uint32_t* __restrict__ scr, int scr_words,
                                                                  cf32* __restrict__ y, const TxDesc* __restrict__ desc, TxLevels lv, PdschTxGeom g)
{
  const TxDesc& d   = desc[blockIdx.y];
  const int     grp = blockIdx.x * blockDim.x + threadIdx.x;
  if (grp * g.nof_ports >= d.nre) return;
  pdsch_tx_mod_body(cb, parity, sys_tail, d.rm, scr + (size_t)blockIdx.y * scr_words, y + ((size_t)blockIdx.y * g.nof_ports) * g.max_re, g, grp, d.nre, d.cb0,
                    d.C, d.Qm, 3 * d.K + 12, lv.v[d.mod]);
}

// The two-layer modes of a 2-port cell (srslte_pdsch_encode with nof_layers == nof_tb, pdsch.c:1100-1173): grid = (ceil(max_re / 256), nof_pdsch2),
// PDSCH v0 + blockIdx.y, one thread per symbol i of the PDSCH. Symbol i of codeword 0 and - where the PDSCH has one - of codeword 1 (descriptor
// cw1: its own code blocks, rate-matching table, modulation and scrambling row), each split in units of Qm (N_L = 1, sch.c:552-556) and modulated
// to the table's levels as srslte_mod_modulate leaves them; then the precoder, which applies the gain, operation by operation as the reference:
//   large-delay CDD (srslte_precoding_cdd_2x2, precoding.c:1897-1956), s2 = 0.5 scaling: y0 = (x0 + x1) s2; y1 = (x0 - x1) s2 for even i,
//     (-x0 + x1) s2 for odd i - i counts the symbols of the PDSCH
//   multiplexing, one layer (srslte_precoding_multiplex, :1988-2010), s1 = scaling / sqrt(2): y0 = x s1; y1 = x s1, -x s1, j x s1, -j x s1 for
//     codebook index 0-3
//   multiplexing, two layers (:2015-2090): index 1: y0 = (x0 + x1) s2, y1 = (x0 - x1) s2; index 2: y1 = j (x0 - x1) s2
// y: [nof_pdsch][2][max_re], as pdsch_tx_scatter_kernel reads it.
__global__ __launch_bounds__(256) void pdsch_tx_mod2_grants_kernel(const uint8_t* __restrict__ cb, const uint8_t* __restrict__ parity,
                                                                   const uint8_t* __restrict__ sys_tail, const uint32_t* __restrict__ scr, int scr_words,
                                                                   cf32* __restrict__ y, const TxDesc* __restrict__ desc, int v0, TxLevels lv, float s1,
                                                                   float s2, int max_re, int cb_stride, int par_stride)
{
  const int     v = v0 + (int)blockIdx.y, i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const TxDesc& d = desc[v];
  const int     nre = d.nre, scheme = d.scheme, codebook = d.codebook, cw1 = d.cw1;
  if (i >= nre) return;
  int re, im;
  pdsch_tx_sym_bits(cb, parity, sys_tail, d.rm, scr + (size_t)v * scr_words, cb_stride, par_stride, i, 1, nre, d.cb0, d.C, d.Qm, 3 * d.K + 12, re, im);
  const cf32 x0 = make_float2(lv.v[d.mod][re], lv.v[d.mod][im]);
  cf32*      y0 = y + (size_t)v * 2 * max_re;
  cf32*      y1 = y0 + max_re;
  if (cw1 < 0) { // one layer: srslte_vec_sc_prod_cfc / _ccc with the codebook's second entry
    const float a = x0.x * s1, b = x0.y * s1;
    y0[i] = make_float2(a, b);
    y1[i] = codebook == 0 ? make_float2(a, b) : (codebook == 1 ? make_float2(-a, -b) : (codebook == 2 ? make_float2(-b, a) : make_float2(b, -a)));
    return;
  }
  const TxDesc& e = desc[cw1];
  pdsch_tx_sym_bits(cb, parity, sys_tail, e.rm, scr + (size_t)cw1 * scr_words, cb_stride, par_stride, i, 1, nre, e.cb0, e.C, e.Qm, 3 * e.K + 12, re, im);
  const cf32 x1 = make_float2(lv.v[e.mod][re], lv.v[e.mod][im]);
  y0[i] = make_float2((x0.x + x1.x) * s2, (x0.y + x1.y) * s2);
  float dr = x0.x - x1.x, di = x0.y - x1.y;
  if (scheme == 3 && (i & 1)) { // -x0 + x1
    dr = -x0.x + x1.x;
    di = -x0.y + x1.y;
  }
  y1[i] = (scheme == 2 && codebook == 2) ? make_float2(-di * s2, dr * s2) : make_float2(dr * s2, di * s2);
}

// grid = (ceil(max_re / 256), nof_pdsch * nof_ports): the symbols of PDSCH p, port by port, onto the REs of its list in its subframe's grids
__global__ __launch_bounds__(256) void pdsch_tx_scatter_kernel(const cf32* __restrict__ y, const uint32_t* __restrict__ relist, cf32* __restrict__ grid,
                                                               const TxDesc* __restrict__ desc, int max_re, int grid_len, int nof_ports)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x, p = blockIdx.y / nof_ports, port = blockIdx.y - p * nof_ports;
  if (i >= desc[p].nre) return;
  grid[((size_t)desc[p].sf * nof_ports + port) * grid_len + relist[(size_t)p * max_re + i]] = y[((size_t)p * nof_ports + port) * max_re + i];
}

// grid = (ceil(grid_len/256), nof_sf * nof_ports): the resource grid of one port: PDSCH symbols, this port's CRS, zero elsewhere
__global__ __launch_bounds__(256) void pdsch_tx_map_kernel(const cf32* __restrict__ y, const cf32* __restrict__ pilots, cf32* __restrict__ grid,
                                                           int nref4 /* 4 * 2 * nof_prb */, PdschTxGeom g)
{
  const int k = blockIdx.x * blockDim.x + threadIdx.x, sp = blockIdx.y, sf = sp / g.nof_ports, port = sp - sf * g.nof_ports;
  if (k >= g.grid_len) return;
  const int  sf_idx  = (g.tti0 + sf) % 10;
  const bool special = g.tdd_s6 >= 0 && (sf_idx == 1 || (sf_idx == 6 && g.tdd_s6));
  const int  v       = special ? g.src_sp[port][k] : g.src[sf_class(sf_idx)][port][k];
  cf32      o = make_float2(0.f, 0.f);
  if (v >= 0) o = y[(size_t)sp * g.max_re + v];
  else if (v <= -2 - MBSFN_REF) o = g.mbsfn_pilots[(size_t)sf_idx * g.mbsfn_nref + (-(v + 2) - MBSFN_REF)];
  else if (v <= -2) { // ports 0/1: [10][4][nref]; ports 2/3: [10][2][nref] behind them (chest.hip)
    o = port < 2 ? pilots[(size_t)sf_idx * nref4 + (-(v + 2))] : pilots[(size_t)10 * nref4 + (size_t)sf_idx * (nref4 / 2) + (-(v + 2))];
  }
  grid[(size_t)sp * g.grid_len + k] = o;
}

} // namespace

// Device / host resources of the per-PDSCH grants mode of the transmit pipeline
struct TxGrantsState : TxGrantsEnc {
  uint32_t         V = 0, W = 0, max_re = 0; // V PDSCHs of W codewords: W = V, or 2 V from the first srslte_hip_dl_tx_batch_grants2 call on
  DevBuf<uint32_t> d_relist;
  DevBuf<cf32>     d_y;
  DevBuf<int32_t>  d_crs_src[4]; // per port: grid RE -> -1 (zero) or the CRS pilot -(v + 2), for pdsch_tx_map_kernel as the grid initialiser
  DevBuf<int32_t>  d_crs_src_sp[4]; // the same for a TDD special subframe: the CRS symbols its DwPTS holds (refsignal_dl.c:162-225), or null
};

struct srslte_hip_dl_tx {
  srslte_hip_dl_tx_cfg_t cfg  = {};
  srslte_hip_ofdm_t*     ofdm = nullptr;
  srslte_hip_chest_dl_t* crs  = nullptr; // for its CRS table
  SchTxFixed             enc;
  PdschTxGeom            g    = {};
  DevBuf<uint32_t>       d_scr, d_idx[3];
  DevBuf<int32_t>        d_src[3][4];
  DevBuf<cf32>           d_y, d_grid;
  std::unique_ptr<TxGrantsState> gs; // srslte_hip_dl_tx_batch_grants / _grants2: created on first use
  float                  rho_a = 0.f; // pdsch.c:525: the precoders' `scaling`
  ~srslte_hip_dl_tx()
  {
    srslte_hip_ofdm_destroy(ofdm);
    srslte_hip_chest_dl_destroy(crs);
  }
};

extern "C" void srslte_hip_dl_tx_destroy(srslte_hip_dl_tx_t* q) { delete q; }

// phy_hip.h, "Sample formats": d_iq of every entry point of the object is in the OFDM object's format from here on
extern "C" int srslte_hip_dl_tx_set_iq_format(srslte_hip_dl_tx_t* q, int format, float scale)
{
  return q ? srslte_hip_ofdm_set_sample_format(q->ofdm, format, scale) : SRSLTE_ERROR_INVALID_INPUTS;
}

extern "C" srslte_hip_dl_tx_t* srslte_hip_dl_tx_create(const srslte_hip_dl_tx_cfg_t* cfg)
{
  if (!cfg || cfg->max_batch == 0 || cfg->mod < 1 || cfg->mod > 4 || cfg->nof_ports > 4 || cfg->nof_ports == 3 || cfg->nof_prb < 6 || cfg->nof_prb > 110) {
    hip_log("[srslte_hip] dl_tx: invalid configuration\n");
    return nullptr;
  }
  std::unique_ptr<srslte_hip_dl_tx> q(new srslte_hip_dl_tx());
  q->cfg = *cfg;
  if (fixed_grant_segmentation("dl_tx", cfg->tbs, &q->enc.seg)) return nullptr;
  const uint32_t P = cfg->nof_prb, nre = 12 * P, B = cfg->max_batch, C = q->enc.seg.C, K = q->enc.seg.K1, Qm = 2 * (uint32_t)cfg->mod;
  const uint32_t nsl = (cfg->cp_ext || cfg->mbsfn) ? 6 : 7; // symbols per slot (an MBSFN subframe has 12 on any cell)
  const uint32_t lstart = cfg->cfi + (P < 10 ? 1 : 0), npt = cfg->nof_ports ? cfg->nof_ports : 1, glen = 2 * nsl * nre;
  if (cfg->mbsfn && (npt != 1 || cfg->tdd || cfg->mbsfn_area_id > 255 || cfg->non_mbsfn_region < 1 || cfg->non_mbsfn_region > 2 || cfg->p_a != 0.f)) {
    hip_log("[srslte_hip] dl_tx: an MBSFN pipeline is single-port FDD, area id 0-255, a non-MBSFN region of 1 or 2 symbols, no power offset\n");
    return nullptr;
  }
  q->ofdm = srslte_hip_ofdm_create((int)P, nsl == 6 ? 0 : 1, 0);
  q->crs  = srslte_hip_chest_dl_create(cfg->cell_id, P, npt, cfg->cp_ext ? 0 : 1);
  bool ok = q->ofdm && q->crs && srslte_hip_ofdm_set_normalize(q->ofdm, 1) == SRSLTE_SUCCESS; // enb_dl.c:61
  if (ok && cfg->mbsfn) {
    ok = srslte_hip_ofdm_set_mbsfn(q->ofdm, 1, (int)cfg->non_mbsfn_region) == SRSLTE_SUCCESS &&
         srslte_hip_chest_dl_set_mbsfn_area_id(q->crs, (uint16_t)cfg->mbsfn_area_id) == SRSLTE_SUCCESS;
  }
  uint32_t       max_re    = 0;
  const uint32_t rep_sf[3] = {0, 5, 1};
  PdschTxGeom&   g = q->g;
  for (int c = 0; c < 3 && ok; c++) {
    std::vector<uint32_t> idx;
    if (cfg->mbsfn) pmch_re_indices(P, lstart, idx);
    else pdsch_re_indices(cfg->cell_id, P, npt, rep_sf[c], lstart, idx, nsl);
    g.cls[c].nof_re = (int)idx.size();
    max_re          = idx.size() > max_re ? (uint32_t)idx.size() : max_re;
    ok              = upload(q->d_idx[c], idx) == SRSLTE_SUCCESS;
    g.cls[c].idx    = q->d_idx[c];
    for (uint32_t port = 0; port < npt && ok; port++) {
      std::vector<int32_t> src(glen, -1);
      for (size_t i = 0; i < idx.size(); i++) src[idx[i]] = (int32_t)i;
      if (cfg->mbsfn) { // srslte_refsignal_mbsfn_put_sf (refsignal_dl.c:297-326): the CRS of symbol 0, the MBSFN reference signal in 2, 6, 10
        const uint32_t fidx0 = cfg->cell_id % 6;
        for (uint32_t i = 0; i < 2 * P; i++) src[fidx0 + 6 * i] = -(int32_t)i - 2;
        for (uint32_t l = 0; l < 3; l++) {
          for (uint32_t i = 0; i < 6 * P; i++) src[(2 + 4 * l) * nre + (l == 1 ? 1 : 0) + 2 * i] = -(int32_t)(l * 6 * P + i) - 2 - MBSFN_REF;
        }
      } else {
        crs_src_put(src.data(), port, port < 2 ? 4 : 2, nsl, P, cfg->cell_id);
      }
      ok             = upload(q->d_src[c][port], src) == SRSLTE_SUCCESS;
      g.src[c][port] = q->d_src[c][port];
    }
  }
  const uint32_t max_bits = max_re * Qm, scr_words = (max_bits + 31) / 32;
  if (ok) { // srslte_sequence_pdsch (sequences.c:58-60), codeword 0; srslte_sequence_pmch (sequences.c:76-80) for an MBSFN pipeline
    std::vector<uint32_t> scr;
    lte_scr_table([&](uint32_t sf) { return cfg->mbsfn ? (sf << 9) + cfg->mbsfn_area_id : ((uint32_t)cfg->rnti << 14) + (sf << 9) + cfg->cell_id; }, max_bits,
                  scr_words, scr);
    ok = upload(q->d_scr, scr) == SRSLTE_SUCCESS;
  }
  ok = ok && q->enc.init(B) == SRSLTE_SUCCESS;
  const PuschTxGeom& cg = q->enc.cg;
  g.mbsfn_pilots = cfg->mbsfn && ok ? (const cf32*)srslte_hip_chest_dl_mbsfn_pilots(q->crs, (uint16_t)cfg->mbsfn_area_id) : nullptr;
  g.mbsfn_nref   = 18 * (int)P;
  g.tdd_s6 = -1; // the fixed-grant calls are FDD (srslte_hip_dl_tx_batch refuses a TDD cell); the grants mode sets its own
  g.grid_len = (int)glen; g.max_re = (int)max_re; g.Qm = (int)Qm; g.Nl = npt > 1 ? 2 : 1; g.nof_ports = (int)npt; g.scr_words = (int)scr_words;
  g.C = (int)C; g.K = (int)K; g.cb_stride = cg.cb_stride; g.par_stride = cg.par_stride; g.rm_len = (int)(3 * K + 12);
  constellation_levels(cfg->mod, g.lvl);
  const float rho_a = powf(10.0f, cfg->p_a / 20.0f) * (npt == 1 ? 1.0f : sqrtf(2.0f)); // pdsch.c:525
  g.gain            = npt == 1 ? rho_a : rho_a / sqrtf(2.0f);                          // precoding.c:1859-1860
  q->rho_a          = rho_a;
  ok = ok && !q->d_y.alloc((size_t)max_re * B * npt) && !q->d_grid.alloc((size_t)glen * B * npt);
  if (!ok) {
    hip_log("[srslte_hip] dl_tx: initialisation failed\n");
    return nullptr;
  }
  return q.release();
}

extern "C" const void* srslte_hip_dl_tx_debug_buffer(const srslte_hip_dl_tx_t* q, int which)
{
  if (!q) return nullptr;
  switch (which) {
    case 0: return q->enc.d_cb;
    case 1: return q->enc.d_parity;
    case 2: return q->d_y;
    case 3: return q->d_grid;
  }
  return nullptr;
}

extern "C" int srslte_hip_dl_tx_batch(srslte_hip_dl_tx_t* q, const uint8_t* d_tb, uint32_t tb_stride, uint32_t tti0, uint32_t nof_sf, uint32_t rv,
                                      void* d_iq, void* stream)
{
  if (!q || !d_tb || !d_iq || nof_sf > q->cfg.max_batch || tb_stride < q->cfg.tbs / 8 || rv > 3) return SRSLTE_ERROR_INVALID_INPUTS;
  if (nof_sf == 0) return SRSLTE_SUCCESS;
  if (q->cfg.tdd) {
    hip_log("[srslte_hip] dl_tx: a TDD cell is served by srslte_hip_dl_tx_batch_grants (per-PDSCH grants)\n");
    return SRSLTE_ERROR;
  }
  hipStream_t     st   = (hipStream_t)stream;
  const uint32_t* d_rm = nullptr;
  int             r    = q->enc.encode(d_tb, tb_stride, nof_sf, rv, stream, &d_rm);
  if (r || !d_rm) return r ? r : SRSLTE_ERROR; // tbs = 0: create makes an object, this call fails, as ever (it used to fail at a launch of 0 blocks)
  PdschTxGeom g = q->g;
  g.tti0        = (int)tti0;
  hipLaunchKernelGGL(pdsch_tx_mod_kernel, dim3(ceil_div(g.max_re / g.nof_ports, 256), nof_sf), dim3(256), 0, st, (const uint8_t*)q->enc.d_cb,
                     (const uint8_t*)q->enc.d_parity, (const uint8_t*)q->enc.d_sys_tail, d_rm, (const uint32_t*)q->d_scr, q->d_y, g);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(pdsch_tx_map_kernel, dim3(ceil_div(g.grid_len, 256), nof_sf * g.nof_ports), dim3(256), 0, st, (const cf32*)q->d_y,
                     (const cf32*)srslte_hip_chest_dl_pilots(q->crs), q->d_grid, 8 * (int)q->cfg.nof_prb, g);
  LAUNCH_CHECK();
  if (q->cfg.mbsfn) { // srslte_ofdm_tx_slot_mbsfn skips the guard between the two regions (ofdm.c:558-574): those samples are zero here, not left-overs
    HIP_TRY(hipMemsetAsync(d_iq, 0, ofdm_sample_bytes(q->ofdm) * (size_t)srslte_hip_ofdm_sf_len(q->ofdm) * nof_sf, st));
  }
  return srslte_hip_ofdm_tx_sf_batch(q->ofdm, q->d_grid, d_iq, (int)nof_sf * g.nof_ports, stream);
}

// W: the codewords the state holds (code-block slots, parity, scrambling rows, CRC words, descriptors): V, or 2 V for the two-layer modes
static int dl_tx_grants_init(srslte_hip_dl_tx_t* q, uint32_t V, uint32_t W)
{
  const uint32_t P = q->cfg.nof_prb, cell_id = q->cfg.cell_id;
  const int      npt = q->g.nof_ports;
  q->gs.reset(new TxGrantsState());
  TxGrantsState* g = q->gs.get();
  g->V      = V;
  g->W      = W;
  g->max_re = 14 * 12 * P;
  if (g->enc_init(W, q->enc.seg.C, (g->max_re * 8 + 31) / 32 + 2, (sizeof(GrantDev) + sizeof(TxDesc)) * W) || g->d_relist.alloc((size_t)g->max_re * V) ||
      g->d_y.alloc((size_t)g->max_re * V * npt))
    return SRSLTE_ERROR;
  for (int port = 0; port < npt; port++) { // the CRS as srslte_hip_dl_tx_create maps them
    const uint32_t       nsl = q->cfg.cp_ext ? 6 : 7;
    std::vector<int32_t> src((size_t)14 * 12 * P, -1);
    crs_src_put(src.data(), port, port < 2 ? 4 : 2, nsl, P, cell_id);
    if (upload(g->d_crs_src[port], src)) return SRSLTE_ERROR;
    if (q->cfg.tdd) { // srslte_refsignal_cs_nof_symbols for a special subframe: by the DwPTS length (phy_common.c:128-135)
      static const int dwt[10] = {3, 9, 10, 11, 12, 3, 9, 10, 11, 6};
      const int dw = dwt[q->cfg.tdd_ss_config % 10], t3 = nsl == 7 ? 12 : 10, t2 = nsl == 7 ? 9 : 8, t1 = nsl == 7 ? 5 : 4;
      const int nsym = dw >= t3 ? (port < 2 ? 4 : 2) : (dw >= t2 ? (port < 2 ? 3 : 2) : (dw >= t1 ? (port < 2 ? 2 : 1) : 1));
      std::vector<int32_t> sp((size_t)14 * 12 * P, -1);
      crs_src_put(sp.data(), port, nsym, nsl, P, cell_id);
      if (upload(g->d_crs_src_sp[port], sp)) return SRSLTE_ERROR;
    }
  }
  return SRSLTE_SUCCESS;
}

// Per-PDSCH grants on the transmit side: what an eNB sends in a run of TTIs - srslte_enb_dl_put_base once per TTI, then srslte_enb_dl_put_pdsch
// once per scheduled UE (enb_dl.c:330-398 -> srslte_pdsch_encode, pdsch.c:1059-1185), each with its own srslte_pdsch_grant_t, then
// srslte_enb_dl_gen_signal. grants[p]: the subframe of the batch, and a srslte_hip_dl_grant2_t as the receive side takes it (PRB masks of both
// slots, modulation, transport block, redundancy version, RNTI, CFI, and - two_cw - the transmission scheme, pmi and second transport block;
// new_data is not used). Row p of d_tb is its transport block 0, row nof_grants + p its block 1. The grids are
// initialised with the CRS of every port, each PDSCH's symbols go onto the REs pdsch_relist_kernel lists for its masks (srslte_pdsch_cp, put =
// true, including upstream's stale-offset rule); allocations that overlap within a subframe are the caller's error (which PDSCH wins an RE is
// not defined here; upstream the later put would). The object's
// cell, antenna ports, p_a apply; cfg.tbs bounds every transport block, cfg.max_grants the number of PDSCHs per call.
// Every codeword is one TxDesc / GrantDev: descriptors 0 .. n - 1 are the PDSCHs (codeword 0, the RE list, the symbol streams; the transmit-
// diversity ones first, so that each modulation kernel runs over a range), the ones behind them the second codewords.
// two_cw = false (srslte_hip_dl_tx_batch_grants): every entry is TM1 / transmit diversity with one block, and d_tb has nof_grants rows.
// ctrl / in: srslte_hip_dl_tx_batch_grants_ctrl's control region, put on the grids after the PDSCHs (nullptr: none); bcast: ctrl's PSS / SSS /
// PBCH put between the grid initialisation and the PDSCHs (srslte_hip_dl_tx_batch_grants_full)
static int dl_tx_batch_grants(srslte_hip_dl_tx_t* q, const uint8_t* d_tb, uint32_t tb_stride, uint32_t tti0, uint32_t nof_sf,
                              const srslte_hip_dl_tx_grant2_t* grants, uint32_t nof_grants, bool two_cw, srslte_hip_dl_ctrl_tx_t* ctrl,
                              const srslte_hip_dl_ctrl_tx_in_t* in, void* d_iq, void* stream, bool bcast = false)
{
  if (!q || !d_tb || !d_iq || !grants || nof_sf > q->cfg.max_batch) return SRSLTE_ERROR_INVALID_INPUTS;
  const uint32_t V = q->cfg.max_grants ? q->cfg.max_grants : q->cfg.max_batch, P = q->cfg.nof_prb, cell_id = q->cfg.cell_id, Cmax = q->enc.seg.C;
  const int      npt = q->g.nof_ports;
  if (nof_grants > V) return SRSLTE_ERROR_INVALID_INPUTS;
  if (q->cfg.mbsfn) {
    hip_log("[srslte_hip] dl_tx grants mode: an MBSFN pipeline has one PMCH configuration, no per-PDSCH grants\n");
    return SRSLTE_ERROR;
  }
  if (nof_sf == 0) return SRSLTE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  // every refusal before anything is allocated or queued
  struct Cw { uint32_t p, row, tbs, rv; int mod, cw; srslte_hip_cbsegm_t seg; };
  auto tb_ok = [&](int mod, uint32_t tbs, uint32_t rv, srslte_hip_cbsegm_t* seg) {
    return mod >= 1 && mod <= 4 && rv <= 3 && tbs != 0 && tbs <= q->cfg.tbs && (tbs % 8) == 0 && tb_stride >= tbs / 8 && srslte_hip_cbsegm(seg, tbs) == 0 &&
           seg->F == 0 && seg->C2 == 0 && seg->C <= Cmax;
  };
  std::vector<GrantDev>            gds(nof_grants);
  std::vector<uint32_t>            nres(nof_grants);
  std::vector<srslte_hip_cbsegm_t> seg0(nof_grants), seg1(nof_grants);
  uint32_t                         nd = 0, n2 = 0; // transmit-diversity PDSCHs, second codewords
  for (uint32_t p = 0; p < nof_grants; p++) {
    const srslte_hip_dl_grant2_t& g2 = grants[p].grant;
    const srslte_hip_dl_grant_t&  gr = g2.tb0;
    if (grants[p].sf >= nof_sf || gr.cfi < 1 || gr.cfi > 3 || !tb_ok(gr.mod, gr.tbs, gr.rv, &seg0[p])) {
      hip_log("[srslte_hip] dl_tx grants: entry %u: unsupported grant (subframe %u of %u, mod %d, tbs %u, rv %u, cfi %u)\n", p, grants[p].sf, nof_sf, gr.mod,
              gr.tbs, gr.rv, gr.cfi);
      return SRSLTE_ERROR_INVALID_INPUTS;
    }
    const bool two_layer = g2.tx_scheme >= 2;
    if (g2.tx_scheme < 0 || g2.tx_scheme > 3 || (two_layer && (npt != 2 || (g2.tx_scheme == 3 && g2.tbs2 == 0) || (g2.tbs2 ? g2.pmi > 1 : g2.pmi > 3))) ||
        (!two_layer && g2.tbs2)) {
      hip_log("[srslte_hip] dl_tx grants: entry %u: unsupported grant (%d ports, tx_scheme %d, pmi %u, second transport block %u bits)\n", p, npt, g2.tx_scheme,
              g2.pmi, g2.tbs2);
      return SRSLTE_ERROR_INVALID_INPUTS;
    }
    if (g2.tbs2 && !tb_ok(g2.mod2, g2.tbs2, g2.rv2, &seg1[p])) {
      hip_log("[srslte_hip] dl_tx grants: entry %u: unsupported second transport block (mod %d, tbs %u, rv %u)\n", p, g2.mod2, g2.tbs2, g2.rv2);
      return SRSLTE_ERROR_INVALID_INPUTS;
    }
    GrantDev& gd = gds[p];
    memset(&gd, 0, sizeof(gd));
    gd.sf_idx = (int)((tti0 + grants[p].sf) % 10); gd.lstart = (int)(gr.cfi + (P < 10 ? 1 : 0)); gd.rnti = gr.rnti;
    tdd_grant_symbols(q->cfg.tdd, q->cfg.tdd_sf_config, q->cfg.tdd_ss_config, q->cfg.cp_ext ? 6 : 7, (uint32_t)gd.sf_idx, gd);
    const uint32_t nre = nres[p] = pdsch_grant_dev(gr, P, cell_id, npt, gd, q->cfg.cp_ext ? 6 : 7);
    // the block split: Qm * N_L bits a unit, N_L = 2 with transmit diversity, 1 where nof_layers == nof_tb (sch.c:552-556)
    if (two_layer ? (nre == 0 || nre < seg0[p].C || (g2.tbs2 && nre < seg1[p].C)) : (nre == 0 || (nre % (uint32_t)npt) || nre < seg0[p].C * (uint32_t)q->g.Nl)) {
      hip_log("[srslte_hip] dl_tx grants: entry %u: %u REs do not carry %u code blocks on %d ports\n", p, nre, two_layer && g2.tbs2 ? seg1[p].C : seg0[p].C, npt);
      return SRSLTE_ERROR_INVALID_INPUTS;
    }
    nd += two_layer ? 0 : 1;
    n2 += g2.tbs2 ? 1 : 0;
  }
  const uint32_t W = two_cw ? 2 * V : V;
  // the first two-codeword call of an object that served single-codeword calls: the state is made anew for 2 V codewords, the old one freed first
  // (freeing waits for what the device still runs on the old buffers)
  if (q->gs && q->gs->W < W) q->gs.reset();
  if (!q->gs && dl_tx_grants_init(q, V, W)) { // a failed start leaves no half-made state behind
    hip_log("[srslte_hip] dl_tx grants: initialisation failed\n");
    q->gs.reset();
    return SRSLTE_ERROR;
  }
  TxGrantsState* g    = q->gs.get();
  GrantDev*      h_gr = nullptr;
  if (int r = g->desc.begin(&h_gr)) return r;
  auto* h_td = reinterpret_cast<TxDesc*>(h_gr + g->W);
  auto* d_gr = g->desc.dev<GrantDev>();
  auto* d_td = reinterpret_cast<const TxDesc*>(d_gr + g->W);
  // the codewords: descriptor v < nof_grants = codeword 0 of a PDSCH, transmit diversity in front; then the codewords 1
  const uint32_t  ncw = nof_grants + n2;
  std::vector<Cw> cws(ncw);
  uint32_t        max_nre = 0, max_nre2 = 0;
  {
    uint32_t vd = 0, v2 = nd, c1 = nof_grants;
    for (uint32_t p = 0; p < nof_grants; p++) {
      const srslte_hip_dl_grant2_t& g2 = grants[p].grant;
      const bool                    two_layer = g2.tx_scheme >= 2;
      const uint32_t                v = two_layer ? v2++ : vd++;
      cws[v] = {p, p, g2.tb0.tbs, g2.tb0.rv, g2.tb0.mod, -1, seg0[p]};
      if (two_layer) max_nre2 = std::max(max_nre2, nres[p]);
      else max_nre = std::max(max_nre, nres[p]);
      if (g2.tbs2) {
        cws[v].cw = (int)c1;
        cws[c1++] = {p, nof_grants + p, g2.tbs2, g2.rv2, g2.mod2, -1, seg1[p]};
      }
    }
  }
  // code-block slots in the order of the block length, so that the encoder runs once per length over neighbouring slots
  std::vector<uint32_t> order(ncw);
  for (uint32_t c = 0; c < ncw; c++) order[c] = c;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return cws[a].seg.K1 < cws[b].seg.K1; });
  uint32_t cb0 = 0;
  for (uint32_t i = 0; i < ncw; i++) {
    const uint32_t                c  = order[i];
    const Cw&                     w  = cws[c];
    const srslte_hip_dl_grant2_t& g2 = grants[w.p].grant;
    h_gr[c]    = gds[w.p];
    h_gr[c].cw = c < nof_grants ? 0 : 1; // the codeword's own scrambling sequence (36.211 6.3.1)
    const uint32_t K  = w.seg.K1;
    TxDesc&        td = h_td[c];
    if (!(td.rm = g->rm_table(K, w.rv))) return SRSLTE_ERROR;
    td.row = (int)w.row; td.sf = (int)grants[w.p].sf; td.tbs = (int)w.tbs; td.C = (int)w.seg.C; td.K = (int)K; td.rlenB = (int)((w.seg.C == 1 ? K : K - 24) / 8);
    td.cb0 = (int)cb0; td.nre = (int)nres[w.p]; td.mod = w.mod; td.Qm = 2 * w.mod;
    td.scheme = g2.tx_scheme; td.codebook = (int)(g2.tbs2 ? g2.pmi + 1 : g2.pmi); td.cw1 = w.cw; // pdsch.c:1152
    cb0 += w.seg.C;
  }
  if (int r = g->desc.commit(g->desc_bytes, st)) return r;
  PdschTxGeom tg = q->g; // ports, N_L, gain; the grid initialiser's maps
  tg.max_re = (int)g->max_re;
  tg.cb_stride = (int)g->cb_stride; tg.par_stride = (int)g->par_stride; // the slots of this mode are spaced for the largest block length
  for (auto& c : tg.src) {
    for (int port = 0; port < 4; port++) c[port] = g->d_crs_src[port];
  }
  for (int port = 0; port < 4; port++) tg.src_sp[port] = g->d_crs_src_sp[port];
  tg.tdd_s6 = q->cfg.tdd ? ((q->cfg.tdd_sf_config <= 2 || q->cfg.tdd_sf_config == 6) ? 1 : 0) : -1;
  tg.tti0 = (int)tti0;
  hipLaunchKernelGGL(pdsch_tx_map_kernel, dim3(ceil_div(tg.grid_len, 256), nof_sf * npt), dim3(256), 0, st, (const cf32*)g->d_y,
                     (const cf32*)srslte_hip_chest_dl_pilots(q->crs), q->d_grid, 8 * (int)P, tg);
  LAUNCH_CHECK();
  if (bcast) {
    if (int r = bcast_tx_launch(dl_ctrl_tx_bcast(ctrl), tti0, nof_sf, q->d_grid, st)) return r;
  }
  if (nof_grants) {
    hipLaunchKernelGGL(pdsch_relist_kernel, dim3(nof_grants), dim3(RELIST_THREADS), 0, st, (const GrantDev*)d_gr, g->d_relist, (int)P, (int)cell_id,
                       (int)g->max_re, npt, q->cfg.cp_ext ? 6 : 7);
    hipLaunchKernelGGL(scr_gen_kernel, dim3(ceil_div((int)g->words, 256), ncw), dim3(256), 0, st, (const GrantDev*)d_gr, (const uint32_t*)g->d_basis,
                       g->d_scr, (int)g->words, (int)cell_id);
    hipLaunchKernelGGL(tx_tbcrc_grants_kernel, dim3(ncw), dim3(256), 0, st, d_tb, (int)tb_stride, (const TxDesc*)d_td, g->d_tbcrc);
    hipLaunchKernelGGL(tx_seg_grants_kernel, dim3(g->Cmax, ncw), dim3(256), 0, st, d_tb, (int)tb_stride, (const uint32_t*)g->d_tbcrc, (const TxDesc*)d_td,
                       g->d_cb, (int)g->cb_stride);
    LAUNCH_CHECK();
    for (uint32_t i = 0; i < ncw;) { // the encoder: runs of equal block length
      uint32_t j = i, n = 0;
      while (j < ncw && cws[order[j]].seg.K1 == cws[order[i]].seg.K1) n += cws[order[j++]].seg.C;
      const size_t s0 = (size_t)h_td[order[i]].cb0;
      if (int r = srslte_hip_tcod_encode_bytes_batch(g->d_cb + s0 * g->cb_stride, g->cb_stride, g->d_parity + s0 * g->par_stride, g->par_stride,
                                                     g->d_sys_tail + s0, cws[order[i]].seg.K1, n, stream))
        return r;
      i = j;
    }
    if (nd) {
      hipLaunchKernelGGL(pdsch_tx_mod_grants_kernel, dim3(ceil_div((int)max_nre / npt, 256), nd), dim3(256), 0, st, (const uint8_t*)g->d_cb,
                         (const uint8_t*)g->d_parity, (const uint8_t*)g->d_sys_tail, (const uint32_t*)g->d_scr, (int)g->words, g->d_y, (const TxDesc*)d_td, g->lv, tg);
    }
    if (nof_grants > nd) { // scaling / sqrt(2) and scaling / 2 as the reference's precoders form them
      hipLaunchKernelGGL(pdsch_tx_mod2_grants_kernel, dim3(ceil_div((int)max_nre2, 256), nof_grants - nd), dim3(256), 0, st, (const uint8_t*)g->d_cb,
                         (const uint8_t*)g->d_parity, (const uint8_t*)g->d_sys_tail, (const uint32_t*)g->d_scr, (int)g->words, g->d_y, (const TxDesc*)d_td, (int)nd,
                         g->lv, q->rho_a / sqrtf(2.0f), q->rho_a / 2.0f, (int)g->max_re, (int)g->cb_stride, (int)g->par_stride);
    }
    hipLaunchKernelGGL(pdsch_tx_scatter_kernel, dim3(ceil_div((int)std::max(max_nre, max_nre2), 256), nof_grants * npt), dim3(256), 0, st, (const cf32*)g->d_y,
                       (const uint32_t*)g->d_relist, q->d_grid, (const TxDesc*)d_td, (int)g->max_re, tg.grid_len, npt);
    LAUNCH_CHECK();
  }
  if (ctrl) {
    if (int r = srslte_hip_dl_ctrl_tx_put(ctrl, tti0, nof_sf, in, q->d_grid, stream)) return r;
  }
  return srslte_hip_ofdm_tx_sf_batch(q->ofdm, q->d_grid, d_iq, (int)nof_sf * npt, stream);
}

// a single-codeword grant as the entry the pipeline takes: the object's scheme (TM1 / transmit diversity), no second transport block
static std::vector<srslte_hip_dl_tx_grant2_t> dl_tx_grants_as2(const srslte_hip_dl_tx_grant_t* grants, uint32_t nof_grants)
{
  std::vector<srslte_hip_dl_tx_grant2_t> g2(grants ? nof_grants : 0);
  for (size_t p = 0; p < g2.size(); p++) {
    memset(&g2[p], 0, sizeof(g2[p]));
    g2[p].sf        = grants[p].sf;
    g2[p].grant.tb0 = grants[p].grant;
  }
  return g2;
}

static int dl_tx_batch_grants(srslte_hip_dl_tx_t* q, const uint8_t* d_tb, uint32_t tb_stride, uint32_t tti0, uint32_t nof_sf,
                              const srslte_hip_dl_tx_grant_t* grants, uint32_t nof_grants, srslte_hip_dl_ctrl_tx_t* ctrl,
                              const srslte_hip_dl_ctrl_tx_in_t* in, void* d_iq, void* stream, bool bcast = false)
{
  if (!grants) return SRSLTE_ERROR_INVALID_INPUTS;
  const std::vector<srslte_hip_dl_tx_grant2_t> g2 = dl_tx_grants_as2(grants, nof_grants);
  srslte_hip_dl_tx_grant2_t                    none = {};
  return dl_tx_batch_grants(q, d_tb, tb_stride, tti0, nof_sf, g2.empty() ? &none : g2.data(), nof_grants, false, ctrl, in, d_iq, stream, bcast);
}

extern "C" int srslte_hip_dl_tx_batch_grants(srslte_hip_dl_tx_t* q, const uint8_t* d_tb, uint32_t tb_stride, uint32_t tti0, uint32_t nof_sf,
                                             const srslte_hip_dl_tx_grant_t* grants, uint32_t nof_grants, void* d_iq, void* stream)
{
  return dl_tx_batch_grants(q, d_tb, tb_stride, tti0, nof_sf, grants, nof_grants, nullptr, nullptr, d_iq, stream);
}

// the checks srslte_hip_dl_tx_batch_grants_ctrl / _full add: the control object's cell is the pipeline's, and everything the control region
// refuses is refused before anything is queued
static uint32_t dl_tx_grant_cfi(const srslte_hip_dl_tx_grant_t& g) { return g.grant.cfi; }
static uint32_t dl_tx_grant_cfi(const srslte_hip_dl_tx_grant2_t& g) { return g.grant.tb0.cfi; }
template <typename Grant>
static int dl_tx_ctrl_check(srslte_hip_dl_tx_t* q, uint32_t tti0, uint32_t nof_sf, const Grant* grants, uint32_t nof_grants, srslte_hip_dl_ctrl_tx_t* ctrl,
                            const srslte_hip_dl_ctrl_tx_in_t* in)
{
  const srslte_hip_dl_ctrl_tx_cfg_t* cc = dl_ctrl_tx_cfg(ctrl);
  // a TDD pipeline takes a TDD control object of its uplink-downlink configuration, an FDD pipeline an FDD one
  const int tdd_cfg = q && q->cfg.tdd ? (int)q->cfg.tdd_sf_config : -1;
  if (!q || !cc || !in || !grants || tdd_cfg != dl_ctrl_tx_tdd_sf_config(ctrl) || q->cfg.mbsfn || cc->nof_prb != q->cfg.nof_prb || cc->nof_ports != (uint32_t)q->g.nof_ports ||
      cc->cell_id != q->cfg.cell_id || (cc->cp_ext != 0) != (q->cfg.cp_ext != 0))
    return SRSLTE_ERROR_INVALID_INPUTS;
  if (int r = dl_ctrl_tx_check(ctrl, tti0, nof_sf, in)) return r;
  for (uint32_t p = 0; p < nof_grants; p++) {
    // in->cfi[b] of an uplink subframe is not looked at, here as in srslte_hip_dl_ctrl_tx_put
    if (grants[p].sf < nof_sf && !dl_ctrl_tx_is_uplink(ctrl, tti0 + grants[p].sf) && dl_tx_grant_cfi(grants[p]) != in->cfi[grants[p].sf])
      return SRSLTE_ERROR_INVALID_INPUTS;
  }
  return SRSLTE_SUCCESS;
}

// srslte_enb_dl_put_base's PCFICH, srslte_enb_dl_put_phich, srslte_enb_dl_put_pdcch_dl / _ul and srslte_enb_dl_put_pdsch of a run of TTIs
// (sf_worker.cc:428-753) in one call: the grants path above with srslte_hip_dl_ctrl_tx_put on its grids before the OFDM modulation. Everything
// the control region refuses is refused before anything is queued.
extern "C" int srslte_hip_dl_tx_batch_grants_ctrl(srslte_hip_dl_tx_t* q, const uint8_t* d_tb, uint32_t tb_stride, uint32_t tti0, uint32_t nof_sf,
                                                  const srslte_hip_dl_tx_grant_t* grants, uint32_t nof_grants, srslte_hip_dl_ctrl_tx_t* ctrl,
                                                  const srslte_hip_dl_ctrl_tx_in_t* in, void* d_iq, void* stream)
{
  if (int r = dl_tx_ctrl_check(q, tti0, nof_sf, grants, nof_grants, ctrl, in)) return r;
  return dl_tx_batch_grants(q, d_tb, tb_stride, tti0, nof_sf, grants, nof_grants, ctrl, in, d_iq, stream);
}

// the same with PSS / SSS / PBCH (srslte_hip_dl_ctrl_tx_put_bcast) put after the CRS and before the PDSCHs: the whole of
// srslte_enb_dl_put_base, a complete FDD subframe per TTI
extern "C" int srslte_hip_dl_tx_batch_grants_full(srslte_hip_dl_tx_t* q, const uint8_t* d_tb, uint32_t tb_stride, uint32_t tti0, uint32_t nof_sf,
                                                  const srslte_hip_dl_tx_grant_t* grants, uint32_t nof_grants, srslte_hip_dl_ctrl_tx_t* ctrl,
                                                  const srslte_hip_dl_ctrl_tx_in_t* in, void* d_iq, void* stream)
{
  if (int r = dl_tx_ctrl_check(q, tti0, nof_sf, grants, nof_grants, ctrl, in)) return r;
  return dl_tx_batch_grants(q, d_tb, tb_stride, tti0, nof_sf, grants, nof_grants, ctrl, in, d_iq, stream, true);
}

// The two-layer modes of a 2-port cell on the transmit side (srslte_pdsch_encode with tx_scheme CDD / SPATIALMUX, pdsch.c:1100-1173): the grants
// path above with the receive side's srslte_hip_dl_grant2_t per PDSCH; d_tb has 2 * nof_grants rows. Extended-CP, TDD and MBSFN objects are
// not served by these calls.
static int dl_tx_grants2_check(const srslte_hip_dl_tx_t* q, const uint8_t* d_tb, uint32_t nof_sf, const srslte_hip_dl_tx_grant2_t* grants, uint32_t nof_grants,
                               const void* d_iq)
{
  if (!q || !d_tb || !d_iq || !grants) {
    hip_log("[srslte_hip] dl_tx grants2: null argument\n");
    return SRSLTE_ERROR_INVALID_INPUTS;
  }
  if (q->cfg.cp_ext || q->cfg.tdd || q->cfg.mbsfn) {
    hip_log("[srslte_hip] dl_tx grants2: extended-CP, TDD and MBSFN objects take single-codeword grants only (srslte_hip_dl_tx_batch_grants)\n");
    return SRSLTE_ERROR_INVALID_INPUTS;
  }
  const uint32_t V = q->cfg.max_grants ? q->cfg.max_grants : q->cfg.max_batch;
  if (nof_sf > q->cfg.max_batch || nof_grants > V) {
    hip_log("[srslte_hip] dl_tx grants2: %u subframes / %u PDSCHs on an object made for %u / %u\n", nof_sf, nof_grants, q->cfg.max_batch, V);
    return SRSLTE_ERROR_INVALID_INPUTS;
  }
  return SRSLTE_SUCCESS;
}

// dl_tx_ctrl_check with the log line the two-codeword calls promise for every refusal
static int dl_tx_grants2_ctrl_check(srslte_hip_dl_tx_t* q, uint32_t tti0, uint32_t nof_sf, const srslte_hip_dl_tx_grant2_t* grants, uint32_t nof_grants,
                                    srslte_hip_dl_ctrl_tx_t* ctrl, const srslte_hip_dl_ctrl_tx_in_t* in)
{
  const int r = dl_tx_ctrl_check(q, tti0, nof_sf, grants, nof_grants, ctrl, in);
  if (r) hip_log("[srslte_hip] dl_tx grants2: the control region is refused (another cell, a grant's cfi that is not its subframe's, or its own inputs)\n");
  return r;
}

extern "C" int srslte_hip_dl_tx_batch_grants2(srslte_hip_dl_tx_t* q, const uint8_t* d_tb, uint32_t tb_stride, uint32_t tti0, uint32_t nof_sf,
                                              const srslte_hip_dl_tx_grant2_t* grants, uint32_t nof_grants, void* d_iq, void* stream)
{
  if (int r = dl_tx_grants2_check(q, d_tb, nof_sf, grants, nof_grants, d_iq)) return r;
  return dl_tx_batch_grants(q, d_tb, tb_stride, tti0, nof_sf, grants, nof_grants, true, nullptr, nullptr, d_iq, stream);
}

extern "C" int srslte_hip_dl_tx_batch_grants2_ctrl(srslte_hip_dl_tx_t* q, const uint8_t* d_tb, uint32_t tb_stride, uint32_t tti0, uint32_t nof_sf,
                                                   const srslte_hip_dl_tx_grant2_t* grants, uint32_t nof_grants, srslte_hip_dl_ctrl_tx_t* ctrl,
                                                   const srslte_hip_dl_ctrl_tx_in_t* in, void* d_iq, void* stream)
{
  if (int r = dl_tx_grants2_check(q, d_tb, nof_sf, grants, nof_grants, d_iq)) return r;
  if (int r = dl_tx_grants2_ctrl_check(q, tti0, nof_sf, grants, nof_grants, ctrl, in)) return r;
  return dl_tx_batch_grants(q, d_tb, tb_stride, tti0, nof_sf, grants, nof_grants, true, ctrl, in, d_iq, stream);
}

extern "C" int srslte_hip_dl_tx_batch_grants2_full(srslte_hip_dl_tx_t* q, const uint8_t* d_tb, uint32_t tb_stride, uint32_t tti0, uint32_t nof_sf,
                                                   const srslte_hip_dl_tx_grant2_t* grants, uint32_t nof_grants, srslte_hip_dl_ctrl_tx_t* ctrl,
                                                   const srslte_hip_dl_ctrl_tx_in_t* in, void* d_iq, void* stream)
{
  if (int r = dl_tx_grants2_check(q, d_tb, nof_sf, grants, nof_grants, d_iq)) return r;
  if (int r = dl_tx_grants2_ctrl_check(q, tti0, nof_sf, grants, nof_grants, ctrl, in)) return r;
  return dl_tx_batch_grants(q, d_tb, tb_stride, tti0, nof_sf, grants, nof_grants, true, ctrl, in, d_iq, stream, true);
}
