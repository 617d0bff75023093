// gpsig_amd -- launches of the higher-order Gram VJP kernel (sig_ho_bwd.h): orders 2 (levels 2..8) and 3
// (levels 3..5), the (order, levels) whose multiplier slab fits the LDS next to the cell buffer.  Orders
// at or above the level count are the exact signature kernel: order min(order, M).  Which kernel runs a shape
// is the plan's decision (ho_bwd_plan, sig_ho_bwd_split.h): the support check, the slab region, the launches
// and the route query below read the same plan.
#include "internal.h"
#include "sig_ho_bwd_split.h"

namespace gpsig {

constexpr size_t HO_BWD_STATIC_LDS = (size_t)4 * GPSIG_WIDE_BWD_R * 64 * 8 * sizeof(float);  // cbuf

template <int ORD, int M>
static int launch_ho_bwd(const BwdArgs &a, int seed, long long nblocks, hipStream_t s) {
  constexpr size_t lds = ho_bwd_lds_bytes<ORD, M>();
  static_assert(ho_bwd_reg_ok(ORD, M) && lds + HO_BWD_STATIC_LDS <= HO_BWD_LDS_BUDGET, "LDS");
  static_assert(ho_bwd_np(ORD, M) == HoBwdLayout<ORD, M>::np && ho_bwd_ncb(ORD, M) == HoBwdLayout<ORD, M>::ncb &&
                    ho_bwd_slots(ORD, M) == HoBwdLayout<ORD, M>::np + HoBwdLayout<ORD, M>::ncb,
                "slab slots");
  if (seed == SEED_RBF_DIFF)
    hipLaunchKernelGGL((sig_ho_bwd_kernel<ORD, M, SEED_RBF_DIFF>), dim3((unsigned)nblocks), dim3(256), lds, s, a);
  else if (seed == SEED_LIN_DIFF)
    hipLaunchKernelGGL((sig_ho_bwd_kernel<ORD, M, SEED_LIN_DIFF>), dim3((unsigned)nblocks), dim3(256), lds, s, a);
  else
    return GPSIG_EUNSUPPORTED;
  return hipGetLastError() == hipSuccess ? GPSIG_OK : GPSIG_ELAUNCH;
}

static int ho_eff_order(int order, int M) { return order < M ? order : M; }

// the plan of a call: GPSIG_HO_SPLIT is read here, once per query or launch
static HoBwdPlan ho_bwd_plan_of(int l2, int order, int M) {
  if (order < 2) return ho_bwd_plan(0, 0, 0, false);
  return ho_bwd_plan(l2, ho_eff_order(order, M), M, ho_split_on());
}

bool ho_bwd_supported(int l2, int order, int M, int seed) {
  if (seed != SEED_RBF_DIFF && seed != SEED_LIN_DIFF) return false;
  return ho_bwd_plan_of(l2, order, M).kernel != HO_BWD_NONE;
}

// global slabs of the 8-wave split VJP (510 .. 1017 points): one launch chunk of workgroups
size_t ho_bwd_slab_bytes(int l2, int order, int M) {
  return (size_t)HO_SPLIT8_BLOCKS * (size_t)ho_bwd_plan_of(l2, order, M).slab_floats * sizeof(float);
}

// Workgroups of the one-pair-per-workgroup kernels (LDS-state, split) over rows [r0, r1): not pair_tiles, the
// tiles are single (a, b) pairs; tile_base: the first pair's index in the upper triangle's enumeration
static long long ho_bwd_pair_blocks(int pair_mode, int r0, int r1, int n2, long long *tile_base) {
  *tile_base = 0;
  if (pair_mode == GPSIG_PAIRS_DIAG) return r1 - r0;
  if (pair_mode == GPSIG_PAIRS_UPPER) {
    auto P = [&](long long r) { return r * n2 - r * (r - 1) / 2; };
    *tile_base = P(r0);
    return P(r1) - P(r0);
  }
  return (long long)(r1 - r0) * n2;
}

// The LDS kernel runs one pair per workgroup: its own grid over the launch's rows [row_begin, row_end)
static int ho_bwd_lds_launch(BwdArgs a, const HoBwdPlan &pl, int o, int seed, hipStream_t s) {
  long long tile_base;
  const long long nblocks = ho_bwd_pair_blocks(a.pair_mode, a.row_begin, a.row_end, a.n2, &tile_base);
  if (a.pair_mode == GPSIG_PAIRS_UPPER) a.tile_base = tile_base;
  a.blk0 = 0;
  if (nblocks <= 0) return GPSIG_OK;
  if (nblocks > 0x7fffffffLL) return GPSIG_EUNSUPPORTED;
  switch (o) {
    case 2: return sig_ho_bwd_lds_launch_o<2>(a, pl, seed, nblocks, s);
    case 3: return sig_ho_bwd_lds_launch_o<3>(a, pl, seed, nblocks, s);
    case 4: return sig_ho_bwd_lds_launch_o<4>(a, pl, seed, nblocks, s);
    case 5: return sig_ho_bwd_lds_launch_o<5>(a, pl, seed, nblocks, s);
    case 6: return sig_ho_bwd_lds_launch_o<6>(a, pl, seed, nblocks, s);
    default: return GPSIG_EUNSUPPORTED;
  }
}

int sig_ho_bwd_launch(const BwdArgs &a, int order, int seed, long long nblocks, hipStream_t s) {
  const int o = ho_eff_order(order, a.M);
  const HoBwdPlan pl = ho_bwd_plan_of(a.l2, order, a.M);
  if (pl.kernel == HO_BWD_NONE) return GPSIG_EUNSUPPORTED;
  if (pl.kernel != HO_BWD_REG) return ho_bwd_lds_launch(a, pl, o, seed, s);
  switch (o * 16 + a.M) {
    case 2 * 16 + 2: return launch_ho_bwd<2, 2>(a, seed, nblocks, s);
    case 2 * 16 + 3: return launch_ho_bwd<2, 3>(a, seed, nblocks, s);
    case 2 * 16 + 4: return launch_ho_bwd<2, 4>(a, seed, nblocks, s);
    case 2 * 16 + 5: return launch_ho_bwd<2, 5>(a, seed, nblocks, s);
    case 2 * 16 + 6: return launch_ho_bwd<2, 6>(a, seed, nblocks, s);
    case 2 * 16 + 7: return launch_ho_bwd<2, 7>(a, seed, nblocks, s);
    case 2 * 16 + 8: return launch_ho_bwd<2, 8>(a, seed, nblocks, s);
    case 3 * 16 + 3: return launch_ho_bwd<3, 3>(a, seed, nblocks, s);
    case 3 * 16 + 4: return launch_ho_bwd<3, 4>(a, seed, nblocks, s);
    case 3 * 16 + 5: return launch_ho_bwd<3, 5>(a, seed, nblocks, s);
    default: return GPSIG_EUNSUPPORTED;
  }
}

// gpsig_sig_vjp_ho_route: the plan's fields (false: no kernel) ...
bool sig_ho_bwd_route_plan(int l2, int order, int M, HoVjpRoute *r) {
  const HoBwdPlan pl = ho_bwd_plan_of(l2, order, M);
  r->kernel = pl.kernel;
  r->W = pl.W;
  r->waves = pl.waves;
  r->slots = pl.slots;
  r->variant = pl.variant;
  r->lds_bytes = pl.lds_bytes;
  return pl.kernel != HO_BWD_NONE;
}
// ... and the kernel launches sig_ho_bwd_launch issues for one chunk: rows [row_begin, row_end), nblocks pair tiles
int sig_ho_bwd_route_launches(int l2, int order, int M, int pair_mode, int row_begin, int row_end, int n2,
                              long long nblocks, int *launches) {
  *launches = 0;
  const HoBwdPlan pl = ho_bwd_plan_of(l2, order, M);
  if (pl.kernel == HO_BWD_NONE) return GPSIG_EUNSUPPORTED;
  if (pl.kernel == HO_BWD_REG) {
    *launches = nblocks > 0 ? 1 : 0;
    return GPSIG_OK;
  }
  long long tile_base;
  const long long nb = ho_bwd_pair_blocks(pair_mode, row_begin, row_end, n2, &tile_base);
  if (nb <= 0) return GPSIG_OK;
  if (nb > 0x7fffffffLL) return GPSIG_EUNSUPPORTED;
  *launches = pl.kernel == HO_BWD_SPLIT8 ? (int)ho_split8_launches(nb) : 1;
  return GPSIG_OK;
}

}  // namespace gpsig
