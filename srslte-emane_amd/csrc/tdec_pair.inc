// 16-window, 16-bit turbo decoder (avx16 numerics, turbodecoder_win.h:398-679 / turbodecoder_iter.h:71-139), second-generation mapping.
// Included by tdec.hip inside its anonymous namespace; bit-exact with tdec_win_kernel<16, 0> (the tests run both on the same inputs).
//
// What the issue probes of round 3 showed (scripts/ubench_single.hip, ubench_issue16.hip): ONE wavefront already issues packed-int16 and
// DPP instructions at the pipe's rate (4.2 cycles each); more wavefronts per SIMD do not raise it. So the decoder's time is its instruction
// count times 4.2 cycles plus what its dependent chains leave unused. The state-per-lane mapping spends most of its instructions moving
// data between lanes (2-3 DPP per add-compare-select, 5 per output) and has ONE dependent chain per wavefront.
// Here a lane owns a BUTTERFLY PAIR of state slots (registers vA, vB = slot bit 2 clear / set), each a packed pair of windows:
//   lane = (block slot h: bit 5) x (window pair g: bits 2-4) x (slot bits p1 p0: bits 0-1) - two code blocks per wavefront;
//   * the in-place radix-2 butterfly (slot p holds state rotr3^t(p), partner p ^ (1 << t%3)) is lane-local at phase 2 and a
//     quad_perm DPP at phases 0 and 1; a slot SENDS old + metric-of-the-partner's-transition, so the receiver needs one max:
//     (4 add + 2 DPP + 2 max) / (4 add + 2 max) for two states against 2 x (2 add + 2.3 DPP + 1 max);
//   * the four branch metrics {0, x, y, x + y} of a step are LDS arrays; each lane reads the 2-4 it needs at per-lane offsets with
//     compile-time row displacements (no selects, no address arithmetic);
//   * state 0 always sits in slot 0 = register vA of the quad's lane 0: normalisation is one quad broadcast + two subtractions;
//   * max-log output: 4 candidates per lane, two lane-local max, then the exchange runs across the lane bit that EQUALS the own
//     transition's information bit at that phase, so no lane has to choose what it keeps (12-15 instructions for two blocks);
//   * beta checkpoints every 12 steps go to a per-wave global row (512 B, written once, read once 10-20 us later: L2), the segment's
//     recomputed beta metrics to LDS (two dwords per lane and step): 13 KB of LDS per wavefront, 12 wavefronts = 24 blocks per CU.
#ifndef P_SG_LDS
#define P_SG_LDS 0
#endif
#ifndef P_AWU_FIRST
#define P_AWU_FIRST 0 // 1: the alpha warm-up before the beta pass (p_siso) - measured, not kept (profiles/r04/ab_tdec_bytes.txt, table 5)
#endif
#ifndef P_MHALF
#define P_MHALF 0
#endif
constexpr int PB      = 12;                         // steps per staged block = checkpoint spacing = alpha segment length (multiple of 6)
constexpr int P_ARR   = PB * 16 + 8;                // dwords of one metric array: 16 window pairs (two blocks) per step; + 8 spreads the arrays over the banks
constexpr int P_SEG   = (PB + 1) * 128;             // recomputed beta metrics: 2 dwords per lane and step
constexpr int P_PERM  = SRSLTE_HIP_MAX_K / 2;       // dwords of the interleaver permutation buffer (one block at a time)
constexpr int P_OVER  = (P_SEG + 3 * P_ARR > P_PERM ? P_SEG + 3 * P_ARR : P_PERM); // the permutation buffer overlays segment + staged rows
constexpr int P_ZERO  = P_OVER + 24;                // the constant zero metric, outside the overlay; + 24: its own bank group
constexpr int P_TAIL  = P_ZERO + P_ARR;             // end of the round-3 pool; checkpoint rows beyond the idle areas follow (P_CK_C)
// Checkpoint rows (128 dwords: 64 lanes x 2) 1 .. P_CK_LDS live in LDS instead of the per-wavefront global row: the recomputed-segment area
// [0, P_SEG) is idle during the sweeps (13 rows) and so is the slack of the permutation overlay behind the staged rows (6 rows). These are
// the LAST rows the beta pass writes and the FIRST the alpha pass reads; by the time the remainder segment uses `seg` they are consumed.
#ifndef P_CK_LDS
#define P_CK_LDS 19
#endif
constexpr int P_CK_A = P_SEG / 128;                          // rows 1 .. P_CK_A at dword 128 (r - 1)
constexpr int P_CK_B = (P_OVER - P_SEG - 3 * P_ARR) / 128;   // rows P_CK_A + 1 .. at dword P_SEG + 3 P_ARR + 128 (r - P_CK_A - 1)
constexpr int P_CK_C = P_CK_LDS > P_CK_A + P_CK_B ? P_CK_LDS - P_CK_A - P_CK_B : 0; // further rows in LDS of their own, behind the pool
constexpr int P_POOL = P_TAIL + 128 * P_CK_C;
static_assert(!P_SG_LDS || P_CK_LDS == 0, "checkpoint rows in LDS use the recomputed-segment area");
__device__ __forceinline__ int p_ck_off(int r)
{
  return r <= P_CK_A ? (r - 1) * 128 : (r <= P_CK_A + P_CK_B ? P_SEG + 3 * P_ARR + (r - P_CK_A - 1) * 128 : P_TAIL + (r - P_CK_A - P_CK_B - 1) * 128);
}
__device__ __forceinline__ void p_ck_put(pk_t* __restrict__ lds, int2* __restrict__ ck, int r, int lane, int2 v)
{
  if (r >= 1 && r <= P_CK_LDS) *reinterpret_cast<int2*>(lds + p_ck_off(r) + lane * 2) = v;
  else if (r > 0) ck[r * 64 + lane] = v; // row 0 (beta at step 0) is never read
}
__device__ __forceinline__ int2 p_ck_get(const pk_t* __restrict__ lds, const int2* __restrict__ ck, int r, int lane)
{
  if (r >= 1 && r <= P_CK_LDS) return *reinterpret_cast<const int2*>(lds + p_ck_off(r) + lane * 2);
  return ck[r * 64 + lane];
}
// The alpha pass requests its checkpoints two segments ahead, next to the row loads: a branch there makes the compiler wait for
// everything outstanding at the merge. So both sources are read, each at a clamped row, and the value is selected (wavefront-uniform).
__device__ __forceinline__ int2 p_ck_get_lds(const pk_t* __restrict__ lds, int r, int lane)
{
  const int rr = P_CK_LDS ? min(max(r, 1), P_CK_LDS) : 1;
  return *reinterpret_cast<const int2*>(lds + p_ck_off(rr) + lane * 2);
}

struct PLane {
  int lane, q, g, h, gp; // gp = 8 h + g: window pair among the wavefront's 16
  bool p0, p1;
  // LDS dword offsets (array base + gp) of the branch metrics this lane adds, per trellis phase:
  // phases 0 / 1: {vA own, vA sent, vB own, vB sent}, phase 2: {own, partner's} (the pair is lane-local, both slots in one class)
  int f0, f1, f2, f3, g0, g1, g2, g3, e0, e1;
  int keep_off[3];       // byte offsets (within a 12-step segment of the output array) of the three outputs this lane keeps
  int rowdw, col;        // output rows: dwords per step and this lane's column (two blocks: 8 and g; one block of 32 windows: 16 and gp)
};
__device__ __forceinline__ int p_arr_base(int i) { return i == 0 ? P_ZERO : P_SEG + (i - 1) * P_ARR; } // metric i of {0, x, y, x + y}
// ONE: the wavefront's 16 window pairs belong to ONE code block of 32 windows (the 8-bit avx8 back-end) instead of two blocks of 16
template <bool ONE = false>
__device__ __forceinline__ PLane p_lane()
{
  PLane L;
  L.lane = threadIdx.x & 63;
  L.q    = L.lane & 3;
  L.g    = (L.lane >> 2) & 7;
  L.h    = L.lane >> 5;
  L.gp   = L.lane >> 2;
  L.p0   = L.lane & 1;
  L.p1   = (L.lane >> 1) & 1;
  const int p0 = L.p0, p1 = L.p1;
  // class index i = 2 b1 + b0 of a slot's state at the phase ((b1, b0) = state bits 2, 1): phase 0 (p2, p1), phase 1 (p0, p2),
  // phase 2 (p1, p0) - LaneGeom::io. Own transition: metric i, the one sent to the partner: 3 - i.
  L.f0 = p_arr_base(p1) + L.gp;
  L.f1 = p_arr_base(3 - p1) + L.gp;
  L.f2 = p_arr_base(2 + p1) + L.gp;
  L.f3 = p_arr_base(1 - p1) + L.gp;
  L.g0 = p_arr_base(2 * p0) + L.gp;
  L.g1 = p_arr_base(3 - 2 * p0) + L.gp;
  L.g2 = p_arr_base(2 * p0 + 1) + L.gp;
  L.g3 = p_arr_base(2 - 2 * p0) + L.gp;
  L.e0 = p_arr_base(L.q) + L.gp;
  L.e1 = p_arr_base(3 - L.q) + L.gp;
  // outputs of a segment: step j is kept by a lane of the quad whose result is valid at the step's phase (p_llr): phase 0 lanes with p1,
  // phase 2 lanes with p0, phase 1 any. q = 0: steps 1, 7, 10; q = 1: 2, 8, 11; q = 2: 0, 4, 6; q = 3: 3, 5, 9
  const int ks[4][3] = {{1, 7, 10}, {2, 8, 11}, {0, 4, 6}, {3, 5, 9}};
  for (int n = 0; n < 3; n++) {
    int j = ks[0][n];
    j     = L.q == 1 ? ks[1][n] : j;
    j     = L.q == 2 ? ks[2][n] : j;
    j     = L.q == 3 ? ks[3][n] : j;
    L.keep_off[n] = ONE ? (j * 16 + L.gp) * 4 : (j * 8 + L.g) * 4;
  }
  L.rowdw = ONE ? 16 : 8;
  L.col   = ONE ? L.gp : L.g;
  return L;
}
// which lane of the quad keeps step j of a segment, and in which of its three registers
__host__ __device__ constexpr int p_keeper(int j) { return j % 3 == 1 ? (j == 4 ? 2 : 0) : (j % 3 == 2 ? (j == 5 ? 3 : 1) : (j % 6 == 0 ? 2 : 3)); }
__host__ __device__ constexpr int p_keep_slot(int j) { return j == 0 || j == 1 || j == 2 || j == 3 ? 0 : (j == 4 || j == 5 || j == 7 || j == 8 ? 1 : 2); }
static_assert(p_keeper(0) == 2 && p_keeper(4) == 2 && p_keeper(6) == 2 && p_keeper(3) == 3 && p_keeper(5) == 3 && p_keeper(9) == 3, "keepers");
static_assert(p_keeper(1) == 0 && p_keeper(7) == 0 && p_keeper(10) == 0 && p_keeper(2) == 1 && p_keeper(8) == 1 && p_keeper(11) == 1, "keepers");
static_assert(p_keep_slot(6) == 2 && p_keep_slot(9) == 2 && p_keep_slot(10) == 2 && p_keep_slot(11) == 2, "keep slots");

__device__ __forceinline__ pk_t p_x1(pk_t v) { return DPP_MOV(v, 0xB1); } // lane ^ 1
__device__ __forceinline__ pk_t p_x2(pk_t v) { return DPP_MOV(v, 0x4E); } // lane ^ 2
__device__ __forceinline__ pk_t p_b0(pk_t v) { return DPP_MOV(v, 0x00); } // lane 0 of the quad

struct PV { pk_t a, b; }; // metrics of the lane's two slots

template <int AR = 0>
__device__ __forceinline__ void p_normalize(PV& v)
{ // turbodecoder_win.h:332-349: subtract state 0's metric; 8-bit back-ends (AR): the maximum over the eight states (normalize_max), which sit
  // in the two registers of the quad's four lanes. v <= max: the difference never saturates upwards, no mask
  if constexpr (AR) {
    pk_t m = pk_max(v.a, v.b);
    m      = pk_max(m, p_x1(m));
    m      = pk_max(m, p_x2(m));
    v.a    = pk_sub<true>(v.a, m);
    v.b    = pk_sub<true>(v.b, m);
  } else {
    const pk_t s0 = p_b0(v.a);
    v.a = pk_sub<true>(v.a, s0);
    v.b = pk_sub<true>(v.b, s0);
  }
}

struct PT { pk_t tAo, rA, tBo, rB; }; // the two transitions into each slot's new state: own slot's and the one received from the partner

// branch metrics of one step, in the order p_acs adds them: phases 0 / 1 {vA own, vA sent, vB own, vB sent}, phase 2 {own, partner's}
struct PM { pk_t m0, m1, m2, m3; };
template <int PH>
__device__ __forceinline__ PM p_metrics(const pk_t* __restrict__ lds, const PLane& L, int row)
{
  PM        m;
  const int r = row * 16;
  if constexpr (PH == 2) {
    m.m0 = lds[L.e0 + r];
    m.m1 = lds[L.e1 + r];
    m.m2 = m.m3 = 0;
  } else {
    m.m0 = lds[(PH ? L.g0 : L.f0) + r];
    m.m1 = lds[(PH ? L.g1 : L.f1) + r];
    m.m2 = lds[(PH ? L.g2 : L.f2) + r];
    m.m3 = lds[(PH ? L.g3 : L.f3) + r];
  }
  return m;
}
// all PB rows of the staged block; PHR0 = phase of row 0. One batch of LDS reads per block: their latency is paid once, and the alpha pass
// uses every value twice (beta recomputation, then the alpha step)
struct PMB { PM r[PB]; };
// LDS returns in issue order, so the reads are issued in the order of first use: the first step
// then waits for one read instead of all of them
// ORDER 1: the consumer starts at row PB - 1; 2: two consumers, one from each end (the alpha pass: beta recomputation downwards, alpha
// steps upwards, interleaved by the scheduler)
template <int PHR0, int ORDER>
__device__ __forceinline__ void p_metrics_block(const pk_t* __restrict__ lds, const PLane& L, PMB& M)
{
#pragma unroll
  for (int n = 0; n < PB; n++) {
    const int row = ORDER == 1 ? PB - 1 - n : (ORDER == 2 ? ((n & 1) ? n / 2 : PB - 1 - n / 2) : n);
    switch ((PHR0 + row) % 3) {
      case 0: M.r[row] = p_metrics<0>(lds, L, row); break;
      case 1: M.r[row] = p_metrics<1>(lds, L, row); break;
      default: M.r[row] = p_metrics<2>(lds, L, row); break;
    }
  }
}

// add-compare-select of both slots at phase PH (= time % 3, of the old metrics forward, of the new ones backward)
// AR: int8 metrics in the high bytes of the int16 halves (tdec.hip, M8): the new state metrics are masked, the transitions are not
template <int PH, int AR = 0>
__device__ __forceinline__ PT p_acs(const PM& m, PV& v)
{
  PT t;
  if constexpr (PH == 2) {
    t.tAo = pk_add<true>(v.a, m.m0);
    t.rA  = pk_add<true>(v.b, m.m1);
    t.tBo = pk_add<true>(v.b, m.m0);
    t.rB  = pk_add<true>(v.a, m.m1);
  } else {
    t.tAo = pk_add<true>(v.a, m.m0);
    t.tBo = pk_add<true>(v.b, m.m2);
    const pk_t sA = pk_add<true>(v.a, m.m1), sB = pk_add<true>(v.b, m.m3);
    t.rA = PH ? p_x2(sA) : p_x1(sA);
    t.rB = PH ? p_x2(sB) : p_x1(sB);
  }
  v.a = pk_max(t.tAo, t.rA);
  v.b = pk_max(t.tBo, t.rB);
  if constexpr (AR) {
    v.a &= M8;
    v.b &= M8;
  }
  return t;
}

// Max-log output m1 - m0 (turbodecoder_win.h:643-659) from the transitions of a step and the beta metrics B of the slots' new states.
// The own transition of a slot carries information bit b0 = state bit 1: slot bit p1 at phase 0, p2 (the register) at phase 1, p0 at
// phase 2. Valid in: lanes with p1 set (phase 0), every lane (phase 1), lanes with p0 set (phase 2).
template <int PH, int AR = 0>
__device__ __forceinline__ pk_t p_llr(const PT& t, const PV& B)
{
  // AR: the two reduced candidates are masked (0x7fff of a positive saturation -> 0x7f00), the difference goes back to an int8 value in
  // an int16 container and takes divide_output in the same shift (turbodecoder_win.h:143-147; tdec.hip win_step)
  auto fin = [](pk_t m1, pk_t m0) -> pk_t {
    if constexpr (AR) return as_p(as_v(pk_sub<true>(m1 & M8, m0 & M8)) >> (short)9);
    return pk_sub<true>(m1, m0);
  };
  const pk_t cAo = pk_add<true>(B.a, t.tAo), cAp = pk_add<true>(B.a, t.rA), cBo = pk_add<true>(B.b, t.tBo), cBp = pk_add<true>(B.b, t.rB);
  if constexpr (PH == 1) {
    pk_t m0 = pk_max(cAo, cBp), m1 = pk_max(cAp, cBo);
    m0 = pk_max(m0, p_x1(m0));
    m1 = pk_max(m1, p_x1(m1));
    m0 = pk_max(m0, p_x2(m0));
    m1 = pk_max(m1, p_x2(m1));
    return fin(m1, m0);
  } else {
    const pk_t K = pk_max(cAo, cBo), S = pk_max(cAp, cBp); // information bit b0 / its complement
    if constexpr (PH == 0) {
      pk_t r = pk_max(K, p_x2(S)); // the lane across p1 sends the candidates that carry THIS lane's bit
      r      = pk_max(r, p_x1(r));
      return fin(r, p_x2(r));
    } else {
      pk_t r = pk_max(K, p_x1(S));
      r      = pk_max(r, p_x2(r));
      return fin(r, p_x1(r));
    }
  }
}

// ---- staging of the branch metrics: rows k_lo .. k_lo + n - 1 (n <= 12) of both blocks' x and y arrays to LDS, x + y formed on the way.
//      Lane t < 48 moves half a row: row t >> 2, block (t >> 1) & 1, window pairs 4 (t & 1) .. + 3.
struct PSrc { // x / y arrays of block slot 0 / 1 (packed window pairs, 8 per step)
  const pk_t *x0, *x1, *y0, *y1;
  int  dbg;
  // a slot whose block has stopped keeps computing in lockstep with its partner; nobody reads what it produces. It reads the first rows of
  // its arrays over and over (cache hits instead of HBM traffic) and stores nothing
  bool dead0, dead1;
  int  rs; // dwords between two steps' rows: 8 (a block of 16 windows per slot) or 16 (one block of 32 windows: x1 / y1 = x0 / y0 + 8)
  // Punctured parity at a quarter of its rows (TdecArgs::pc): ysel = 3 | yph << 2 - the y arrays hold row r, r % 4 == yph, at row r >> 2 and
  // every other row is zero. Every staged run of rows starts at a multiple of 4 (Lw % 4 == 0: the 12-step blocks, the 40-step warm-ups, their
  // 4-step remainders, the last short segment), so a lane's row has the same residue every time. ysel = 0: whole arrays. (One word, as
  // TdecArgs::pc: with two the kernel spills a fourth pointer around the sweeps, 36 bytes of scratch instead of 28.)
  int  ysel = 0;
};
struct PRows { int4 x, y; };
__device__ __forceinline__ PRows p_stage_load(const PSrc& S, const PLane& L, int k_lo, int n)
{
  const int   t = L.lane < 48 ? L.lane : L.lane - 16, row = min(t >> 2, n - 1);
  const bool  b1 = (t >> 1) & 1;
  const int   kr = (((S.dbg & 32) || (b1 ? S.dead1 : S.dead0)) ? row : k_lo + row); // a dead slot reads its first rows over and over
  const int   off = kr * S.rs + (t & 1) * 4, offy = (kr >> (S.ysel & 2)) * S.rs + (t & 1) * 4; // ysel = 3: k_lo % 4 == 0
  const pk_t *xs = b1 ? S.x1 : S.x0, *ys = b1 ? S.y1 : S.y0;
  PRows       r;
  r.x = *reinterpret_cast<const int4*>(xs + off);
  r.y = *reinterpret_cast<const int4*>(ys + offy);
  return r;
}
// AR: the y rows come straight from the parity array (int8 values in int16 containers) and move to the high bytes here (tdec.hip stage_store)
template <int AR = 0>
__device__ __forceinline__ void p_stage_store(pk_t* __restrict__ lds, const PLane& L, const PSrc& S, int n, const PRows& r)
{
  if (L.lane < 48 && (L.lane >> 2) < n) {
    pk_t*      d = lds + P_SEG + (L.lane >> 2) * 16 + ((L.lane >> 1) & 1) * 8 + (L.lane & 1) * 4;
    // a row the y arrays do not hold (PSrc::ysel) was loaded from its group's row all the same - no branch around a load - and is zero from
    // here on, where the rows are first used
    const bool held = ((L.lane >> 2) & (S.ysel & 3)) == (S.ysel >> 2); // 0: every row
    const int4 y = AR ? make_int4((r.y.x & 0x00FF00FF) << 8, (r.y.y & 0x00FF00FF) << 8, (r.y.z & 0x00FF00FF) << 8, (r.y.w & 0x00FF00FF) << 8)
                      : make_int4(held ? r.y.x : 0, held ? r.y.y : 0, held ? r.y.z : 0, held ? r.y.w : 0);
    *reinterpret_cast<int4*>(d)             = r.x;
    *reinterpret_cast<int4*>(d + P_ARR)     = y;
    *reinterpret_cast<int4*>(d + 2 * P_ARR) = // turbodecoder_win.h:472-491; 8-bit: a 0x7fff here is harmless (tdec.hip, M8)
        make_int4(pk_add<true>(r.x.x, y.x), pk_add<true>(r.x.y, y.y), pk_add<true>(r.x.z, y.z), pk_add<true>(r.x.w, y.w));
  }
  // one wavefront per workgroup, LDS operations complete in order: only the compiler has to be kept from moving reads above this
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// one step at a run-time phase (left-over steps); MODE 0: recursion only, 2: with output
template <int MODE, int AR = 0>
__device__ __forceinline__ pk_t p_step_rt(const pk_t* __restrict__ lds, const PLane& L, int ph, int row, PV& v, const PV& B)
{
  pk_t o = 0;
  switch (ph) {
    case 0: { const PT t = p_acs<0, AR>(p_metrics<0>(lds, L, row), v); if constexpr (MODE == 2) o = p_llr<0, AR>(t, B); } break;
    case 1: { const PT t = p_acs<1, AR>(p_metrics<1>(lds, L, row), v); if constexpr (MODE == 2) o = p_llr<1, AR>(t, B); } break;
    default: { const PT t = p_acs<2, AR>(p_metrics<2>(lds, L, row), v); if constexpr (MODE == 2) o = p_llr<2, AR>(t, B); } break;
  }
  return o;
}

// a run of nb staged blocks of PB steps without output. DIR < 0: first step k_first = PB - 1 (mod PB) going down, DIR > 0: first
// step k_first going up; PH0 = k_first % 3. n_first: normalisation counter of the first step (parity NPAR0); MODE 0: warm-up (no
// normalisation at counter 0), 1: beta main pass (checkpoint after every step k = 0 mod PB)
template <int DIR, int PH0, int NPAR0, int MODE, int AR = 0>
__device__ __forceinline__ void p_run(pk_t* __restrict__ lds, const PLane& L, const PSrc& S, PV& v, int k_first, int n_first, int nb, int2* __restrict__ ck)
{
  if (nb <= 0) return;
  auto lo = [&](int b) { // lowest step of block min(b, nb - 1): loads past the end repeat the last block instead of branching
    const int bb = min(b, nb - 1);
    return DIR > 0 ? k_first + PB * bb : k_first - PB * bb - (PB - 1);
  };
  // Two blocks of rows in flight, in two register sets used alternately (the loop is unrolled by two): rotating one set into the other
  // is a VALU move that has to wait for the load that was just issued
  auto body = [&](PRows& r, int b) {
    p_stage_store<AR>(lds, L, S, PB, r);
    r = p_stage_load(S, L, lo(b + 2), PB);
    const int k0 = k_first + DIR * PB * b, n0 = n_first + DIR * PB * b;
    constexpr int PHR0 = DIR > 0 ? PH0 : (PH0 + 1) % 3; // phase of the block's row 0 (its lowest step)
    PMB M;
    p_metrics_block<PHR0, (DIR < 0 ? 1 : 0)>(lds, L, M);
#pragma unroll
    for (int j = 0; j < PB; j++) {
      const int row = DIR > 0 ? j : PB - 1 - j;
      switch ((PHR0 + row) % 3) { // static after unrolling
        case 0: p_acs<0, AR>(M.r[row], v); break;
        case 1: p_acs<1, AR>(M.r[row], v); break;
        default: p_acs<2, AR>(M.r[row], v); break;
      }
      if constexpr (MODE == 1) {
        if (j == PB - 1) p_ck_put(lds, ck, (k0 + DIR * j) / PB, L.lane, make_int2(v.a, v.b)); // before its normalisation, as upstream stores it
      }
      if (AR || ((NPAR0 + j) & 1) == 0) { // 8-bit: every step; 16-bit: every second one
        if (MODE == 1 || n0 + DIR * j != 0) p_normalize<AR>(v);
      }
    }
  };
  PRows ra = p_stage_load(S, L, lo(0), PB), rb = p_stage_load(S, L, lo(1), PB);
  int   b  = 0;
  for (; b + 1 < nb; b += 2) {
    body(ra, b);
    body(rb, b + 1);
  }
  if (b < nb) body(ra, b);
}

// up to PB - 1 left-over steps at run-time phases, staged together
template <int DIR, int MODE, int AR = 0>
__device__ __forceinline__ void p_rem(pk_t* __restrict__ lds, const PLane& L, const PSrc& S, PV& v, int k_first, int n_first, int cnt, int2* __restrict__ ck)
{
  if (cnt <= 0) return;
  const int k_lo = DIR > 0 ? k_first : k_first - (cnt - 1);
  p_stage_store<AR>(lds, L, S, cnt, p_stage_load(S, L, k_lo, cnt));
  const PV none = {0, 0};
  for (int j = 0; j < cnt; j++) {
    const int k = k_first + DIR * j, n = n_first + DIR * j;
    p_step_rt<0, AR>(lds, L, k % 3, k - k_lo, v, none);
    if constexpr (MODE == 1) {
      if (k % PB == 0) p_ck_put(lds, ck, k / PB, L.lane, make_int2(v.a, v.b));
    }
    if ((AR || (n & 1) == 0) && n != 0) p_normalize<AR>(v);
  }
}

// metric of state s (slot s at time 0 / slot rotl3 at other times: the caller passes the SLOT) of window pair gs of the lane's block
__device__ __forceinline__ pk_t p_fetch(const PV& v, int slot, int gp16)
{
  const int  src = (gp16 << 2) | (slot & 3);
  const pk_t a = __shfl(v.a, src, 64), b = __shfl(v.b, src, 64);
  return (slot & 4) ? b : a;
}

// One SISO pass of both block slots. x / y arrays per slot in S, tails per slot in tl (systematic [0..2], parity [3..5] of THIS
// constituent decoder), outputs to out0 / out1 (packed pairs, 8 per step), ck: this wavefront's checkpoint rows.
// AR = 1, ONE: the avx8 back-end (32 windows of one block = the wavefront's 16 window pairs; int8 saturating arithmetic in the high bytes,
// INF = 0, normalisation by the maximum after every step, output >> 1: turbodecoder_win.h:92-173)
template <int AR = 0, bool ONE = false>
__device__ __forceinline__ void p_siso(const PLane& L, const PSrc& S, const int16_t* tl_x, const int16_t* tl_y, pk_t* __restrict__ out, pk_t* __restrict__ lds,
                                       int2* __restrict__ ck, int K PROF_ARGS)
{
  const int  Lw  = K / (ONE ? 32 : 16);
  const pk_t NEG = AR ? 0 : pk_make(-TD_INF, -TD_INF); // INF = 0 for the 8-bit back-ends (turbodecoder_win.h:120,:152)
  // the window pair after / before this lane's, and whether this is the block's last / first pair
  const int  gp_next = ONE ? ((L.gp + 1) & 15) : ((L.h << 3) | ((L.g + 1) & 7)), gp_prev = ONE ? ((L.gp + 15) & 15) : ((L.h << 3) | ((L.g + 7) & 7));
  const bool gp_last = ONE ? L.gp == 15 : L.g == 7, gp_first = ONE ? L.gp == 0 : L.g == 0;
  pk_t*      seg = lds; // [PB + 1][64] x 2 dwords
  PV         v;
#if P_AWU_FIRST
  // The alpha warm-up does not depend on the beta pass: run FIRST, its 40 rows (the windows' last steps) are the ones the beta main pass starts
  // with a few blocks later - cache hits instead of a second trip to memory after the whole beta pass. Two registers wait for the alpha pass.
  v.a = v.b = NEG;
  {
    const int k0 = Lw - WIN_OVERLAP;
    switch (k0 % 3) {
      case 0: p_run<1, 0, 0, 0, AR>(lds, L, S, v, k0, 0, 3, nullptr); break;
      case 1: p_run<1, 1, 0, 0, AR>(lds, L, S, v, k0, 0, 3, nullptr); break;
      default: p_run<1, 2, 0, 0, AR>(lds, L, S, v, k0, 0, 3, nullptr); break;
    }
    p_rem<1, 0, AR>(lds, L, S, v, k0 + 36, 36, 4, nullptr);
  }
  PROF(7)
  const PV v_awu = v;
#endif
  // ---- beta warm-up over the first 40 steps of every window (turbodecoder_win.h:456-464): steps 39 .. 0, counter = step index
  static_assert(WIN_OVERLAP == 40, "block plan below is written for the 40-step overlap");
  v.a = v.b = NEG;
  p_run<-1, 39 % 3, 1, 0, AR>(lds, L, S, v, 39, 39, 3, nullptr); // steps 39 .. 4
  p_rem<-1, 0, AR>(lds, L, S, v, 3, 3, 4, nullptr);               // steps 3 .. 0
  PROF(5)
  // ---- tail trellis of the last window (scalar; turbodecoder_win.h:351-395): wrapping int16; 8-bit: sadd() clamps at +127 and wraps below
  //      (:322-330), INF = 0
  int tail[8];
  {
    int  o[8] = {0, -TD_INF, -TD_INF, -TD_INF, -TD_INF, -TD_INF, -TD_INF, -TD_INF};
    if constexpr (AR) {
      for (int i = 1; i < 8; i++) o[i] = 0;
    }
    auto WA = [](int a, int b) -> int {
      if constexpr (AR) {
        const int z = (int)(short)(a + b);
        return z > 127 ? 127 : (int)(signed char)z;
      } else {
        return (int)(short)(a + b);
      }
    };
    for (int j = 2; j >= 0; j--) {
      const int x = tl_x[j], y = tl_y[j], xy_ = WA(x, y);
      int m[8] = {WA(o[4], xy_), o[4], WA(o[5], y), WA(o[5], x), WA(o[6], x), WA(o[6], y), o[7], WA(o[7], xy_)};
      int n[8] = {o[0], WA(o[0], xy_), WA(o[1], x), WA(o[1], y), WA(o[2], y), WA(o[2], x), WA(o[3], xy_), o[3]};
      for (int i = 0; i < 8; i++) o[i] = m[i] > n[i] ? m[i] : n[i];
    }
    for (int i = 0; i < 8; i++) tail[i] = AR ? o[i] * 256 : o[i];
  }
  // ---- window shift (:428-448): window w starts from the warm-up of window w + 1, the last one from the tail. The warm-up ended at
  //      time 0, where slot s holds state s; at time Lw slot p holds state rotr3^Lw(p)
  {
    PV nv;
#pragma unroll
    for (int r = 0; r < 2; r++) {
      const int  s = rotr3(4 * r + L.q, Lw % 3);
      const pk_t a = p_fetch(v, s, L.gp), b = p_fetch(v, s, gp_next);
      int        ts = tail[0];
      for (int i = 1; i < 8; i++) ts = s == i ? tail[i] : ts;
      const pk_t n_ = pk_make(pk_hi(a), gp_last ? ts : pk_lo(b));
      if (r == 0) nv.a = n_; else nv.b = n_;
    }
    v = nv;
  }
  // ---- beta main pass (:466-526): every PB-th metric set is kept (global row, L2), the alpha pass recomputes the rest
  const int nf = Lw / PB, t = Lw - nf * PB, top = nf + (t > 0);
  p_ck_put(lds, ck, top, L.lane, make_int2(v.a, v.b));
  p_rem<-1, 1, AR>(lds, L, S, v, Lw - 1, Lw - 1, t, ck);
  p_run<-1, (PB - 1) % 3, 1, 1, AR>(lds, L, S, v, nf * PB - 1, nf * PB - 1, nf, ck);
  PROF(6)
#if !P_AWU_FIRST
  // ---- alpha warm-up over the last 40 steps of every window (:586-603), counter 0 .. 39
  v.a = v.b = NEG;
  {
    const int k0 = Lw - WIN_OVERLAP;
    switch (k0 % 3) {
      case 0: p_run<1, 0, 0, 0, AR>(lds, L, S, v, k0, 0, 3, nullptr); break;
      case 1: p_run<1, 1, 0, 0, AR>(lds, L, S, v, k0, 0, 3, nullptr); break;
      default: p_run<1, 2, 0, 0, AR>(lds, L, S, v, k0, 0, 3, nullptr); break;
    }
    p_rem<1, 0, AR>(lds, L, S, v, k0 + 36, 36, 4, nullptr);
  }
  PROF(7)
#else
  v = v_awu;
#endif
  // ---- window shift (:560-583): window w starts from the end of window w - 1, window 0 from the known state. At time Lw state p sits
  //      in slot rotl3^Lw(p); the main pass starts at time 0, where slot p holds state p
  {
    PV nv;
#pragma unroll
    for (int r = 0; r < 2; r++) {
      const int  p = 4 * r + L.q, sp = rotl3(p, Lw % 3);
      const pk_t a = p_fetch(v, sp, L.gp), b = p_fetch(v, sp, gp_prev);
      const int  init = (AR || p == 0) ? 0 : -TD_INF;
      const pk_t n_ = pk_make(gp_first ? init : pk_hi(b), pk_lo(a));
      if (r == 0) nv.a = n_; else nv.b = n_;
    }
    v = nv;
  }
  // ---- alpha main pass with the extrinsic output (:605-679), a segment of PB steps at a time: its beta metrics are recomputed from the
  //      checkpoint above it into LDS with the operands the alpha steps need anyway, then consumed
  {
    const bool k1 = L.q == 1, k2 = L.q == 2, k3 = L.q == 3;
    const bool wr = !(L.h ? S.dead1 : S.dead0); // this lane's slot still has a reader for its output
    // rows and checkpoint of segment min(j, nf - 1): two segments in flight in two register sets used alternately (as p_run)
    auto rows_of = [&](int j) { return p_stage_load(S, L, PB * min(j, nf - 1), PB); };
    // rows 1 .. P_CK_LDS wait in LDS (read at the top of their segment); the global request is clamped to the rows behind them
    auto ck_of   = [&](int j) { return ck[min(max(min(j, nf - 1) + 1, P_CK_LDS + 1), nf + 1) * 64 + L.lane]; };
    auto body = [&](PRows& sr, int2& cb, int j) {
      const int k0 = PB * j;
      int2 cl = make_int2(0, 0);
      if constexpr (P_CK_LDS > 0) cl = p_ck_get_lds(lds, j + 1, L.lane);
      p_stage_store<AR>(lds, L, S, PB, sr);
      if (P_CK_LDS > 0 && j + 1 <= P_CK_LDS) cb = cl;
      const PV Btop = {cb.x, cb.y}; // beta[k0 + PB] as stored: before its normalisation
      sr = rows_of(j + 2);
      cb = ck_of(j + 2);
      PMB M;
      p_metrics_block<0, 2>(lds, L, M);
      PV vb = Btop;
      if (k0 + PB < Lw) p_normalize<AR>(vb); // the recursion went on from the normalised value; beta[Lw] is a start value
#if P_SG_LDS
      // sg[i] = beta[k0 + i], i = 1 .. PB - 1, waits in LDS (two dwords per lane and step)
#define SG_PUT(i, val) *reinterpret_cast<int2*>(seg + (i) * 128 + L.lane * 2) = make_int2((val).a, (val).b)
#else
      PV sg[PB]; // in registers, two per step
#define SG_PUT(i, val) sg[i] = (val)
#endif
#pragma unroll
      for (int i = PB - 1; i >= 1; i--) { // phase i % 3
        switch (i % 3) {
          case 0: p_acs<0, AR>(M.r[i], vb); break;
          case 1: p_acs<1, AR>(M.r[i], vb); break;
          default: p_acs<2, AR>(M.r[i], vb); break;
        }
        SG_PUT(i, vb);
        if (AR || (i & 1) == 0) p_normalize<AR>(vb);
      }
#undef SG_PUT
#if P_MHALF
      p_metrics_block<0, 0>(lds, L, M); // read again: between the two uses the 40 values are not live
#endif
      pk_t kp0 = 0, kp1 = 0, kp2 = 0;
#pragma unroll
      for (int i = 0; i < PB; i++) {
        PV B = Btop;
        if (i < PB - 1) {
#if P_SG_LDS
          const int2 bb = *reinterpret_cast<const int2*>(seg + (i + 1) * 128 + L.lane * 2);
          B.a = bb.x;
          B.b = bb.y;
#else
          B = sg[i + 1];
#endif
        }
        pk_t o;
        switch (i % 3) {
          case 0: { const PT tt = p_acs<0, AR>(M.r[i], v); o = p_llr<0, AR>(tt, B); } break;
          case 1: { const PT tt = p_acs<1, AR>(M.r[i], v); o = p_llr<1, AR>(tt, B); } break;
          default: { const PT tt = p_acs<2, AR>(M.r[i], v); o = p_llr<2, AR>(tt, B); } break;
        }
        const int  kq   = p_keeper(i);
        const bool mine = kq == 0 ? L.q == 0 : (kq == 1 ? k1 : (kq == 2 ? k2 : k3));
        if (p_keep_slot(i) == 0) kp0 = mine ? o : kp0;
        else if (p_keep_slot(i) == 1) kp1 = mine ? o : kp1;
        else kp2 = mine ? o : kp2;
        if ((AR || (i & 1) == 0) && (i != 0 || k0 != 0)) p_normalize<AR>(v);
      }
      if (wr) {
        char* ob = reinterpret_cast<char*>(out) + (size_t)k0 * 4 * L.rowdw;
        *reinterpret_cast<pk_t*>(ob + L.keep_off[0]) = kp0;
        *reinterpret_cast<pk_t*>(ob + L.keep_off[1]) = kp1;
        *reinterpret_cast<pk_t*>(ob + L.keep_off[2]) = kp2;
      }
    };
    if (nf > 0) {
      PRows sra = rows_of(0), srb = rows_of(1);
      int2  cba = ck_of(0), cbb = ck_of(1);
      int   j   = 0;
      for (; j + 1 < nf; j += 2) {
        body(sra, cba, j);
        body(srb, cbb, j + 1);
      }
      if (j < nf) body(sra, cba, j);
    }
    // the last, shorter segment [PB nf, Lw): run-time phases
    if (t > 0) {
      const int k0 = PB * nf;
      p_stage_store<AR>(lds, L, S, t, p_stage_load(S, L, k0, t));
      const int2 cbt  = p_ck_get(lds, ck, top, L.lane); // read before the segment area below is written (LDS runs in order)
      const PV   Btop = {cbt.x, cbt.y}, none = {0, 0};
      PV         vb   = Btop;
      for (int i = t - 1; i >= 1; i--) {
        p_step_rt<0, AR>(lds, L, (k0 + i) % 3, i, vb, none);
        *reinterpret_cast<int2*>(seg + i * 128 + L.lane * 2) = make_int2(vb.a, vb.b);
        if (AR || ((k0 + i) & 1) == 0) p_normalize<AR>(vb);
      }
      for (int i = 0; i < t; i++) {
        PV B = Btop;
        if (i < t - 1) {
          const int2 bb = *reinterpret_cast<const int2*>(seg + (i + 1) * 128 + L.lane * 2);
          B.a = bb.x;
          B.b = bb.y;
        }
        const int  ph = (k0 + i) % 3;
        const pk_t o  = p_step_rt<2, AR>(lds, L, ph, i, v, B);
        if (wr && L.q == (ph == 0 ? 2 : (ph == 1 ? 0 : 1))) out[(k0 + i) * L.rowdw + L.col] = o; // a lane whose result is valid at this phase
        if ((AR || ((k0 + i) & 1) == 0) && k0 + i != 0) p_normalize<AR>(v);
      }
    }
  }
}

// Element-wise phases of one wavefront: their time is memory round trips, not instructions. The block's own arrays (written a pass ago:
// HBM / MALL latency) are all requested before anything is used - UC 16-byte elements per lane cover the longest block in one trip -
// while the tables every block shares (interleaver, x^i mod g: L2 hits) follow in batches of UH. Loads run on clamped indices instead
// of under a branch (a guarded load is a branch, and the compiler waits for everything outstanding at the merge); `st` is predicated.
template <int UC, int UH, typename LdC, typename LdH, typename St>
__device__ __forceinline__ void p_batched2(int lane, int n, LdC ldc, LdH ldh, St st)
{
  static_assert(UC % UH == 0, "batch sizes");
  for (int base = lane; base < n; base += 64 * UC) {
    decltype(ldc(0)) c[UC];
#pragma unroll
    for (int u = 0; u < UC; u++) c[u] = ldc(min(base + 64 * u, n - 1));
#pragma unroll
    for (int u0 = 0; u0 < UC; u0 += UH) {
      if (base - lane + 64 * u0 >= n) break; // wavefront-uniform: whole batches past the end are skipped
      asm volatile("" ::: "memory"); // keeps the scheduler from requesting every batch's tables at once (registers)
      decltype(ldh(0)) h[UH];
#pragma unroll
      for (int u = 0; u < UH; u++) h[u] = ldh(min(base + 64 * (u0 + u), n - 1));
#pragma unroll
      for (int u = 0; u < UH; u++) {
        const int i = base + 64 * (u0 + u);
        if (i < n) st(i, c[u0 + u], h[u]);
      }
    }
  }
}

// Two code blocks per wavefront: block slot h = lanes 32 h .. 32 h + 31 in the sweeps; the element-wise phases between the sweeps
// (extrinsic exchange, interleaver permutations through LDS, CRC syndrome, decisions) run slot after slot with all 64 lanes.
// Block pointers are formed as kernel-argument base + offset wherever they are used (never kept in an indexed array): an array of
// pointers lives in scratch and the loads / stores through it become flat ones, which also count as LDS operations and force
// s_waitcnt 0 on everything behind them.
struct PBlk {
  size_t in_off, wk_off; // elements from a.in / a.work
  bool   ok;             // this slot has stopped (CRC passed, or no block)
  uint32_t its;
};
// P_XCHG_INT 1: the exchange after an odd pass works in the INTERLEAVED domain (see the kernel); 0: round 3's natural-domain form
#ifndef P_XCHG_INT
#define P_XCHG_INT 1
#endif
#ifndef TDEC_PAIR_WAVES
#define TDEC_PAIR_WAVES 3
#endif
#ifndef TDEC_PAIR_MINW
#define TDEC_PAIR_MINW 2
#endif
#ifndef TDEC_PAIR_EWU
#define TDEC_PAIR_EWU 3
#endif
#ifndef TDEC_PAIR_EWC
#define TDEC_PAIR_EWC 6
#endif
// Register budget: 184 VGPRs (round 4; round 3: 216). What two decoder wavefronts leave of a SIMD's 512 registers per lane is where the
// front-end kernels of the other streams run: 80 at 216 (one channel-estimator or OFDM wavefront), 112 at the 194 the kernel needs since the
// exchange phase shrank, 144 at 184 - TWO OFDM wavefronts (71 -> 72 each) or three rate-de-matcher / estimator ones (47 / 46 -> 48). Same-box
// A/B (profiles/r04/ab_tdec_bytes.txt, table 6): 194 -> 539 k subframes/s, 192 -> 543 k, 184 -> 550 k (20 bytes of scratch outside the loops),
// 176 / 168 -> 547 k; above 216 the pipeline loses 5 % (round 3, X82). amdgpu_num_vgpr counts in units of two on gfx90a and later (unified
// VGPR / AGPR file): 92 means 184; a plain 184 is dropped as incompatible with the occupancy range.
#ifndef TDEC_PAIR_NVGPR
#define TDEC_PAIR_NVGPR 92
#endif
#if TDEC_PAIR_NVGPR > 0
#define P_NVGPR_ATTR __attribute__((amdgpu_num_vgpr(TDEC_PAIR_NVGPR)))
#else
#define P_NVGPR_ATTR
#endif
// ENTRY SEAM (pair), to be left a preprocessor seam. tdec_mix.hip compiles this file's kernel as a BODY that tdec_mix_kernel calls for the
// wavefronts of its K > 800 groups: `a` describes the wavefront's group, bx is its index there, pool / tl are the mixed kernel's LDS. (A second
// translation unit, so that nothing about the kernel below - inlining order, register allocation - depends on the mixed kernel's existence:
// with both in one unit it lost 1.5 % of the headline.) A thin kernel around one shared body was tried: the headline kernel changed, 14016 ->
// 14149 assembly lines with `a` by reference, 13985 and other spills by value (profiles/tdec_seams/README.md, finding 2).
#ifdef TDEC_MIX_TU
__device__ __forceinline__ void tdec_pair_body(TdecArgs& a, const uint32_t bx, pk_t* pool, int16_t (*tl)[12])
{
  constexpr int W   = 16;
  const int     K   = (int)a.K, K8 = K / 8;
  const PLane   L   = p_lane();
#else
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(TDEC_PAIR_MINW, TDEC_PAIR_WAVES))) P_NVGPR_ATTR void tdec_pair_kernel(TdecArgs a0, TdecGroups gs)
{
  TdecArgs       a  = a0;
  const uint32_t bx = tdec_enter_group(a, gs); // wavefront index within its group of equal block length
  constexpr int W   = 16;
  const int     K   = (int)a.K, K8 = K / 8;
  const PLane   L   = p_lane();
  __shared__ __attribute__((aligned(16))) pk_t pool[P_POOL];
  __shared__ int16_t tl[2][12]; // per slot: systematic tail, parity-0 tail, interleaved systematic tail, parity-1 tail
#endif
  int16_t*           perm = reinterpret_cast<int16_t*>(pool);
  static_assert(2 * P_OVER >= SRSLTE_HIP_MAX_K, "permutation buffer must hold one code block");
  for (int i = L.lane; i < P_ARR; i += 64) pool[P_ZERO + i] = 0;

  // ---- the wavefront's two blocks; a missing or skipped one (sch.c:317-318) leaves its slot without work
  const int lcb_a = 2 * (int)bx, lcb_b = lcb_a + 1;
  const int cb_a  = a.cb_map ? (int)a.cb_map[lcb_a] : lcb_a;
  bool      live_a = true, live_b = lcb_b < (int)a.nof_cb;
  const int cb_b  = live_b ? (a.cb_map ? (int)a.cb_map[lcb_b] : lcb_b) : cb_a;
  if (a.skip && a.skip[cb_a]) {
    if (L.lane == 0 && a.iters) a.iters[cb_a] = 0;
    live_a = false;
    if (TDEC_RAGGED_TB && a.tb_out && a.tb_Cof) tdec_tb_stored_block(a, cb_a, K, L.lane);
  }
  if (live_b && a.skip && a.skip[cb_b]) {
    if (L.lane == 0 && a.iters) a.iters[cb_b] = 0;
    live_b = false;
    if (TDEC_RAGGED_TB && a.tb_out && a.tb_Cof) tdec_tb_stored_block(a, cb_b, K, L.lane);
  }
  if (!live_a && !live_b) return;
  // slot 0 always holds a live block; a slot 1 without one shadows slot 0: same loads, same stores of the same values
  const bool two = live_a && live_b;
  const int  cb0 = live_a ? cb_a : cb_b, lcb0 = live_a ? lcb_a : lcb_b, cb1 = two ? cb_b : cb0, lcb1 = two ? lcb_b : lcb0;
  PBlk       b0 = {(size_t)cb0 * a.in_stride, (size_t)lcb0 * 7 * a.Kp, false, a.start_iter};
  PBlk       b1 = {(size_t)cb1 * a.in_stride, (size_t)lcb1 * 7 * a.Kp, !two, a.start_iter};
  const int  tb = a.pc ? K + 32 + K / 2 : (a.sb_layout ? 3 * (K + 32) : 3 * K);
  const bool inplace = a.sb_layout && ((reinterpret_cast<uintptr_t>(a.in) | (a.in_stride * sizeof(int16_t))) & 15) == 0; // a.pc: the host has checked it
  const size_t Kp = a.Kp;
  // arrays of a block: work arrays 0 .. 6 = syst, par0, par1, app1, app2, ext1, ext2; systematic / parity LLRs in place when possible
  auto WK   = [&](const PBlk& b, int i) -> int16_t* { return a.work + b.wk_off + (size_t)i * Kp; };
  auto SYST = [&](const PBlk& b) -> const int16_t* { return inplace ? a.in + b.in_off : a.work + b.wk_off; };
  auto PAR  = [&](const PBlk& b, int i) -> const int16_t* { return a.work + b.wk_off + (size_t)(1 + i) * Kp; }; // extracted; in place: see the sweeps

  // ---- input extraction (turbodecoder_win.h:727-769 / turbodecoder_iter.h:58-68,84-91); a 16-byte aligned SB-layout buffer is read in place
  auto extract = [&](const PBlk& b, int h) {
    const int16_t* in = a.in + b.in_off;
    int16_t *      syst = WK(b, 0), *par0 = WK(b, 1), *par1 = WK(b, 2);
    if (!inplace && a.sb_layout) {
      batched<8>(
          L.lane, K, [&](int i) { return I3{in[i], in[K + 32 + i], in[2 * (K + 32) + i]}; },
          [&](int i, I3 t) {
            syst[i] = (int16_t)t.a;
            par0[i] = (int16_t)t.b;
            par1[i] = (int16_t)t.c;
          });
    } else if (!a.sb_layout) {
      batched<8>(
          L.lane, K, [&](int n) { return I3{in[3 * n], in[3 * n + 1], in[3 * n + 2]}; },
          [&](int n, I3 t) {
            const int x = win_pos<W>(n, K);
            syst[x]     = (int16_t)t.a;
            par0[x]     = (int16_t)t.b;
            par1[x]     = (int16_t)t.c;
          });
    }
    if (L.lane < 3) {
      tl[h][L.lane]     = in[tb + 2 * L.lane];
      tl[h][3 + L.lane] = in[tb + 2 * L.lane + 1];
      tl[h][6 + L.lane] = in[tb + 6 + 2 * L.lane];
      tl[h][9 + L.lane] = in[tb + 6 + 2 * L.lane + 1];
    }
  };
  PROF_DECL;
  extract(b0, 0);
  extract(b1, 1); // a shadow slot repeats slot 0's (idempotent) extraction: its tails have to be there
  __syncthreads();
  PROF(0)

  int2*    ck     = reinterpret_cast<int2*>(a.beta) + (size_t)bx * (a.beta_stride / 2);
  uint32_t n_iter = a.start_iter; // > 0: the work arrays hold the state this kernel leaves after that many passes (TdecOpts::start_iter)
  constexpr int EWU = TDEC_PAIR_EWU;             // table elements (16 bytes) in flight per lane in the element-wise phases
  constexpr int EWC = TDEC_PAIR_EWC;             // elements of the block's own arrays in flight per lane (12 = the longest block in one round trip)
  // The extrinsic exchange of turbodecoder_iter.h:71-139 happens AFTER each pass, in one element-wise phase that also takes the CRC of the
  // pass's hard decisions (sch.c:362-378) and leaves the next pass's input ready (A = a-priori array app1, E = extrinsic):
  //   after an even pass n (DEC1 -> ext1):  syndrome over sign(ext1);  E = ext1 - A (n >= 2; srslte_vec_sub, wrapping), NOT stored;
  //                                          app2[deinter[i]] = E[i]    (ext1 keeps the pass's decision metrics)
  //   after an odd pass n (DEC2 -> ext2), in the interleaved domain j (app2[j] = E[inter[j]], app1'[inter[j]] = ext2[j]):
  //                                          syndrome over sign(ext2[j]) with the table crc_rem[inter[j]];  D[j] = ext2[j] - app2[j];
  //                                          A[inter[j]] = D[j] -> app1;  x = sat(A + syst) -> ext2 array (turbodecoder_win.h:472-476)
  // Upstream subtracts at the START of the next pass and in the natural domain; here every array is read once, nothing is written that
  // the next phase can form itself, and the decision metrics of a block that stops are still there: ext1 after an odd number of passes,
  // app1' = A + E after an even number (wrapping int16 arithmetic: exact), E taken back out of app2 through the interleaver (finish).
  while (n_iter < a.nof_iter && !(b0.ok && b1.ok)) {
    const bool odd = n_iter & 1;
    // ---- the SISO pass of both slots (a stopped slot keeps computing on its arrays; its output goes to an array nobody reads any more)
    if (!(a.dbg & 1)) {
      auto P = [](const int16_t* p) { return reinterpret_cast<const pk_t*>(p); };
      PSrc S;
      S.dbg = a.dbg;
      S.dead0 = b0.ok;
      S.dead1 = b1.ok && two; // a shadow slot repeats slot 0's stores: same values to the same addresses
      S.rs    = 8;
      S.ysel  = a.pc ? 3 | (int)((a.pc >> (odd ? 4 : 2)) & 3) << 2 : 0;
      if (!odd) {
        S.x0 = P(n_iter ? WK(b0, 6) : SYST(b0)); S.x1 = P(n_iter ? WK(b1, 6) : SYST(b1));
      } else {
        S.x0 = P(WK(b0, 4)); S.x1 = P(WK(b1, 4));
      }
      if (inplace) { // the parity rows sit behind the systematic ones of the same buffer: one uniform offset from there
        uint32_t po = a.pc ? (uint32_t)(K + 32) + (odd ? K / 4 : 0) : (odd ? 2u : 1u) * (K + 32);
        // formed per pass: hoisted out of the pass loop, the pointers of both parities wait in scratch (36 bytes instead of 28; the
        // kernel-resources test allows 32)
        asm volatile("" : "+s"(po));
        S.y0 = P(a.in + b0.in_off + po); S.y1 = P(a.in + b1.in_off + po);
      } else {
        S.y0 = P(PAR(b0, odd)); S.y1 = P(PAR(b1, odd));
      }
#if P_XCHG_INT
      // outputs: even pass -> ext1, odd -> ext2. A stopped slot's decision metrics are in ext1 (odd number of passes) or in ext2 (even):
      // its sweeps write the other one of the two, which nobody reads any more (garbage in, garbage out, no effect on the live slot)
      auto        oi  = [&](const PBlk& b, bool stopped) { return stopped ? ((b.its & 1) ? 6 : 5) : (odd ? 6 : 5); };
      const int   oi0 = oi(b0, b0.ok), oi1 = two ? oi(b1, b1.ok) : oi0;
#else
      // outputs: even pass -> ext1, odd -> ext2. A stopped slot's decision metrics are in ext1 and app1: its sweeps write ext2 (odd
      // passes) / app2 (even passes: its x is the ext2 array) instead
      const int   oi0 = odd ? 6 : (b0.ok ? 4 : 5), oi1 = odd ? 6 : (b1.ok && two ? 4 : 5);
#endif
      const size_t oo = (L.h ? b1.wk_off : b0.wk_off) + (size_t)(L.h ? oi1 : oi0) * Kp;
      p_siso(L, S, tl[L.h] + (odd ? 6 : 0), tl[L.h] + (odd ? 9 : 3), reinterpret_cast<pk_t*>(a.work + oo), pool, ck, K PROF_PASS);
    }
    __syncthreads();
    PROF(2)
    n_iter++;
    // ---- exchange + CRC, slot after slot
    auto exchange = [&](PBlk& b) {
      if (b.ok) return;
      b.its = n_iter;
      if (a.dbg & 64) return;
      int16_t *app1 = WK(b, 3), *app2 = WK(b, 4), *ext1 = WK(b, 5), *ext2 = WK(b, 6);
      uint32_t syn = 0;
      const bool crc = a.t.crc_rem != nullptr;
      struct XC { v8s e, ap; };            // the block's own arrays
      struct XH { v8u lut; v4w t0, t1; };  // shared tables
      auto crc_rows = [&](int i8, XH& x) {
        if (crc) {
          const v4w* tp = reinterpret_cast<const v4w*>(a.t.crc_rem + 8 * i8);
          x.t0 = tp[0];
          x.t1 = tp[1];
        }
      };
      __syncthreads(); // perm is free: the previous slot's reads of it have been issued, LDS runs in order; this orders the compiler
      if (!odd) { // the pass just run was even
        const bool sub = n_iter > 1;
        p_batched2<EWC, EWU>(
            L.lane, K8, [&](int i8) { return XC{ld8(ext1, i8), sub ? ld8(app1, i8) : v8s{}}; },
            [&](int i8) {
              XH x;
              x.lut = ld8u(a.t.deinter, i8);
              crc_rows(i8, x);
              return x;
            },
            [&](int i8, const XC& c, const XH& x) {
              if (crc) {
#pragma unroll
                for (int j = 0; j < 4; j++) syn ^= (c.e[j] > 0 ? x.t0[j] : 0u) ^ (c.e[4 + j] > 0 ? x.t1[j] : 0u);
              }
              const v8s e = sub ? c.e - c.ap : c.e;
#if !P_XCHG_INT
              if (sub) st8(ext1, i8, e);
#endif
#pragma unroll
              for (int j = 0; j < 8; j++) perm[x.lut[j]] = e[j];
            });
        __syncthreads();
        for (int i8 = L.lane; i8 < K8; i8 += 64) st8(app2, i8, *reinterpret_cast<const v8s*>(perm + 8 * i8));
      } else {
        const int16_t* syst = SYST(b);
#if P_XCHG_INT
        p_batched2<EWC, EWU>(
            L.lane, K8, [&](int i8) { return XC{ld8(ext2, i8), ld8(app2, i8)}; },
            [&](int i8) {
              XH x;
              x.lut = ld8u(a.t.inter, i8);
              if (crc) {
                const v4w* tp = reinterpret_cast<const v4w*>(a.t.crc_rem_i + 8 * i8);
                x.t0 = tp[0];
                x.t1 = tp[1];
              }
              return x;
            },
            [&](int i8, const XC& c, const XH& x) {
              if (crc) { // sign(app1'[inter[j]]) = sign(ext2[j]): this pass's hard decisions
#pragma unroll
                for (int j = 0; j < 4; j++) syn ^= (c.e[j] > 0 ? x.t0[j] : 0u) ^ (c.e[4 + j] > 0 ? x.t1[j] : 0u);
              }
              const v8s d = c.e - c.ap;
#pragma unroll
              for (int j = 0; j < 8; j++) perm[x.lut[j]] = d[j];
            });
        __syncthreads();
        if (crc) { // a block that stops here needs no input for a next pass: its ext2 array keeps the pass's raw output (finish)
          for (int o = 32; o > 0; o >>= 1) syn ^= __shfl_xor(syn, o, 64);
          if (syn == 0 && !(a.dbg & (1 | 16))) {
            b.ok = true;
            return;
          }
        }
        p_batched2<EWC, EWC>(
            L.lane, K8, [&](int i8) { return ld8(syst, i8); }, [&](int) { return 0; },
            [&](int i8, const v8s& sy, int) {
              const v8s an = *reinterpret_cast<const v8s*>(perm + 8 * i8);
              st8(app1, i8, an);
              st8(ext2, i8, __builtin_elementwise_add_sat(an, sy));
            });
        return;
#else
        p_batched2<EWC, EWU>(
            L.lane, K8, [&](int i8) { return ld8(ext2, i8); }, [&](int i8) { return ld8u(a.t.inter, i8); },
            [&](int i8, const v8s& e2, const v8u& lut) {
#pragma unroll
              for (int j = 0; j < 8; j++) perm[lut[j]] = e2[j];
            });
        __syncthreads();
        p_batched2<EWC, EWU>(
            L.lane, K8, [&](int i8) { return XC{ld8(ext1, i8), ld8(syst, i8)}; },
            [&](int i8) {
              XH x;
              x.lut = v8u{};
              crc_rows(i8, x);
              return x;
            },
            [&](int i8, const XC& c, const XH& x) {
              const v8s ap = *reinterpret_cast<const v8s*>(perm + 8 * i8); // app1 of this pass: its sign is the hard decision
              if (crc) {
#pragma unroll
                for (int j = 0; j < 4; j++) syn ^= (ap[j] > 0 ? x.t0[j] : 0u) ^ (ap[4 + j] > 0 ? x.t1[j] : 0u);
              }
              const v8s an = ap - c.e;
              st8(app1, i8, an);
              st8(ext2, i8, __builtin_elementwise_add_sat(an, c.ap));
            });
#endif
      }
      if (crc) {
        for (int o = 32; o > 0; o >>= 1) syn ^= __shfl_xor(syn, o, 64);
        b.ok = syn == 0 && !(a.dbg & (1 | 16));
      }
    };
    exchange(b0);
    exchange(b1);
    __syncthreads();
    PROF(3)
  }
  // ---- hard decision bytes, MSB first, natural bit order (turbodecoder_win.h:771-838), and the block's share of the transport-block
  //      CRC24A syndrome (sch.c:470-488), slot after slot
  const int      Lw    = K / W;
  const uint32_t magic = (uint32_t)((0x100000000ull + (uint32_t)Lw - 1) / (uint32_t)Lw); // n / Lw = (n * magic) >> 32
  auto finish = [&](const PBlk& b, int cb) {
    const int16_t *app1 = WK(b, 3), *ext1 = WK(b, 5);
    uint8_t*        o    = a.out + (size_t)cb * a.out_stride;
    uint32_t        tsyn = 0;
    const uint32_t* tab  = a.tb_rem ? a.tb_rem + (size_t)(cb % a.tb_C) * K : nullptr;
    // transport-block assembly (sch.c:360,:401-410): block r of transport block cb / C owns bytes [r rb, r rb + rb) of it; the last block
    // also leaves its own CRC behind the TB's, as the assembly kernel does
    const int       tbr  = (int)(cb % a.tb_C), tbi = (int)(cb / a.tb_C);
    int             tbC  = (int)a.tb_C, rb = (int)a.tb_rb;
    size_t          row  = (size_t)tbi;
    uint32_t        fac  = 1;
    if (TDEC_RAGGED_TB && a.tb_Cof) { // a ragged batch: this transport block's own block count; the share tables do not depend on the block's position, its factor does
      tbC = (int)a.tb_Cof[tbi];
      rb  = (tbC == 1 ? K : K - 24) / 8;
      tab = a.tbA + (tbC == 1 ? 0 : K);
      fac = a.tbA[2 * K + (tbC - 1 - tbr)];
      row = (uint32_t)tbi < a.tb_B ? (size_t)tbi : (size_t)a.tb_rows0 + tbi - a.tb_B;
    }
    uint8_t*        tbo  = a.tb_out ? a.tb_out + row * a.tb_out_stride + (size_t)tbr * rb : nullptr;
    const int       tlim = tbr == tbC - 1 ? K8 : rb;
    bool            par_nz = false; // the TB's CRC24A bytes, the last rb - 3 .. rb - 1 of the last block: not all zero (sch.c:481)
    __syncthreads();
    struct XC { v8s e, ap; };
    struct XT { v4w t0, t1; };
#if P_XCHG_INT
    // Decision metrics (turbodecoder.c:383-390): ext1 after an odd number of passes. After an even number app1' = the interleaver's image
    // of the last DEC2 output: a block that stopped on its CRC still has that output in its ext2 array; one that ran out of passes has
    // A in app1 and E in app2 (interleaved), app1' = A + E in wrapping arithmetic
    const bool even = !(b.its & 1) && !(a.dbg & 64), raw2 = even && b.ok, sum = even && !raw2;
    if (even) {
      const int16_t* src = WK(b, raw2 ? 6 : 4);
      p_batched2<EWC, EWU>(
          L.lane, K8, [&](int i8) { return ld8(src, i8); }, [&](int i8) { return ld8u(a.t.inter, i8); },
          [&](int i8, const v8s& v, const v8u& lut) {
#pragma unroll
            for (int j = 0; j < 8; j++) perm[lut[j]] = v[j];
          });
      __syncthreads();
    }
#else
    const bool      sum  = b.its != 1 && !(a.dbg & 64);
    constexpr bool  even = false;
#endif
    p_batched2<EWC, EWU>(
        L.lane, K8, [&](int i8) { return XC{even ? v8s{} : ld8(ext1, i8), sum ? ld8(app1, i8) : v8s{}}; },
        [&](int i8) {
          XT x = {};
          if (tab) {
            const v4w* tp = reinterpret_cast<const v4w*>(tab + 8 * i8);
            x.t0 = tp[0];
            x.t1 = tp[1];
          }
          return x;
        },
        [&](int i8, const XC& c, const XT& x) {
          const v8s e = even ? *reinterpret_cast<const v8s*>(perm + 8 * i8) : c.e;
          const v8s d = sum ? e + c.ap : e;
          *reinterpret_cast<v8s*>(perm + 8 * i8) = d;
          if (tab) {
#pragma unroll
            for (int j = 0; j < 4; j++) tsyn ^= (d[j] > 0 ? x.t0[j] : 0u) ^ (d[4 + j] > 0 ? x.t1[j] : 0u);
          }
        });
    if (tab) {
      for (int o2 = 32; o2 > 0; o2 >>= 1) tsyn ^= __shfl_xor(tsyn, o2, 64);
    }
    __syncthreads();
    for (int bi = L.lane; bi < K8; bi += 64) {
      int      q = (int)__umulhi((uint32_t)(8 * bi), magic), r = 8 * bi - q * Lw; // natural index n -> array position (n % Lw) * W + n / Lw
      uint32_t byte = 0;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        byte |= (perm[r * W + q] > 0 ? 0x80u : 0u) >> j;
        if (++r == Lw) {
          r = 0;
          q++;
        }
      }
      o[bi] = (uint8_t)byte;
      if (tbo && bi < tlim) tbo[bi] = (uint8_t)byte;
      par_nz = par_nz || (bi >= rb - 3 && bi < rb && byte != 0);
    }
    if (tbo) par_nz = __ballot(par_nz) != 0;
    if (L.lane == 0) {
      if (a.iters) a.iters[cb] = b.its;
      if (a.crc_ok) a.crc_ok[cb] = b.ok ? 1 : 0;
      if (a.tb_rem) a.tb_syn[cb] = tsyn;
      if (fac != 1) tsyn = tdec_gf24_mul(tsyn, fac); // ragged batches: the payload's remainder times x^(bits behind this block in its transport block)
      if (tbo) { // the verdict of sch.c:470-488 by the last block to get here: every block's CRC, the XOR of the shares, a non-zero parity
        // Agent-scope atomics are performed at the memory side (the eight XCDs' L2s are not coherent with each other), so nothing else is
        // needed to make the contributions visible to the last block - a __threadfence() here writes back and invalidates the XCD's whole
        // L2, 1664 times per launch: the pipeline lost 20 %. Only the ORDER matters: the count goes last, after the two contributions
        // have come back (returning atomics, waited for)
        uint32_t* acc = a.tb_acc + 4 * (size_t)tbi;
        const uint32_t o1 = atomicXor(acc, tsyn);
        uint32_t want = 2u, flags = (b.ok ? 0u : 1u) | ((tbr == tbC - 1 && par_nz) ? 2u : 0u);
        if (TDEC_RAGGED_TB && a.tb_Cof) { // ragged batches: bit 2 = a block of this transport block was decoded in this call (skipped ones do not set it, tdec_tb_stored_block)
          flags |= 4u;
          want = 6u;
        }
        const uint32_t o2 = atomicOr(acc + 1, flags);
        uint32_t dep = o1 | o2;
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(dep)::"memory");
        if (atomicAdd(acc + 2, 1u) == (uint32_t)tbC - 1) {
          const uint32_t syn = atomicExch(acc, 0u), fl = atomicExch(acc + 1, 0u);
          atomicExch(acc + 2, 0u); // clean for the next launch
          a.tb_ok_out[row] = (syn == 0 && fl == want) ? 1 : 0;
        }
      }
    }
  };
  finish(b0, cb0);
  if (two) finish(b1, cb1);
  PROF(4)
#ifdef TDEC_PROF
  if (a.prof && L.lane == 0) {
    for (int i = 0; i < 10; i++) a.prof[(size_t)blockIdx.x * 10 + i] = prof_acc[i];
  }
#endif
}
