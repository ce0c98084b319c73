// The mixed-kind decoder launch of ragged batches: a translation unit of its own that compiles tdec.hip's decoder BODIES - the pair-mapped one
// of tdec_pair.inc, the 8-window one, the unwindowed one - into one kernel, tdec_mix_kernel below. Kept apart so that the kernels of tdec.hip
// come out exactly as they do without it: with the mixed kernel in the same unit the inliner takes another order through the shared device
// functions and tdec_pair_kernel lost 1.5 % of the headline line (profiles/r04/ab_mix_kernel.txt).
// What this reading of tdec.hip and tdec_pair.inc differs in is said there in two ways only: the constant TDEC_RAGGED_TB (true here: the
// transport-block assembly of ragged batches, the 8-window body's LDS for K <= 800) and three entry seams - pair, windowed, unwindowed - that
// make each decoder a body called with this kernel's LDS instead of a kernel (profiles/tdec_seams/README.md on why those stay seams).
#define TDEC_MIX_TU 1
#include "tdec.hip"

namespace {
// ------------------------------------------------------------------------------------------------------------------
// A ragged batch (tdec_run_groups) in ONE launch: its groups of equal block length may be of different KINDS - the two-blocks-per-wavefront
// decoder (K > 800), the 8-window one (400 < K <= 800), the unwindowed one (K <= 400). Launched one kind after the other on the batch's stream
// they were a chain: the short-block launches are a few wavefronts each and as long as their longest recursion (unwindowed 127 us, 8-window
// 59 us behind the 376 us of the long blocks in the mixed-grant workload). Here every wavefront looks up its group, reads its kind and runs
// that decoder's body; the LDS pool is laid out for the larger need (pair sweeps / the 8-window body with the checkpoint rows of K <= 800).
// Register budget and occupancy: the pair kernel's. Mixed-grant line 622 k -> 791 k subframes/s (profiles/r04/ab_mix_kernel.txt).
// ------------------------------------------------------------------------------------------------------------------
constexpr int MIX_WIN8_POOL = WIN_POOL<8>;
constexpr int MIX_POOL      = MIX_WIN8_POOL > P_POOL ? MIX_WIN8_POOL : P_POOL;
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(TDEC_PAIR_MINW, TDEC_PAIR_WAVES))) P_NVGPR_ATTR void tdec_mix_kernel(TdecArgs a0, TdecGroups gs)
{
  TdecArgs       a = a0;
  uint32_t       gi = 0;
  for (uint32_t i = 1; i < gs.n; i++) gi = blockIdx.x >= gs.g[i].first_wave ? i : gi;
  const uint32_t kind = gs.kind[gi];
  const uint32_t bx   = tdec_enter_group(a, gs);
  __shared__ __attribute__((aligned(16))) pk_t pool[MIX_POOL];
  __shared__ int16_t tl[2][12];
  a.sb_layout = kind != TDEC_KIND_GEN; // the unwindowed decoder reads the plain [s p0 p1] layout, the windowed ones the rate de-matcher's
  a.tbA       = gs.tbA[gi];
  if (kind == TDEC_KIND_PAIR) tdec_pair_body(a, bx, pool, tl);
  else if (kind == TDEC_KIND_WIN8) tdec_win_body<8, 0>(a, bx, pool, tl[0]);
  else tdec_gen_body(a, bx);
}
} // namespace
// called by tdec_run_groups (tdec.hip); args / groups: that unit's TdecArgs / TdecGroups (the same definitions)
int tdec_mix_launch(const void* args, const void* groups, unsigned waves, hipStream_t st)
{
  hipLaunchKernelGGL(tdec_mix_kernel, dim3(waves), dim3(64), 0, st, *static_cast<const TdecArgs*>(args), *static_cast<const TdecGroups*>(groups));
  LAUNCH_CHECK();
  return SRSLTE_SUCCESS;
}
