// gpsig_amd -- instantiations of the matrix-core wide-channel Gram (sig_fo_mf.h) for one level count
// (GPSIG_M): columns per lane 4 / 8 / 10, RBF and linear difference seeds, with and without saved state.
#include "internal.h"
#include "sig_fo_mf.h"

#ifndef GPSIG_M
#error "GPSIG_M"
#endif

namespace gpsig {

template <int NW, int W, int M, int SEED, bool BLK, int NP>
static int mf_launch_np(const MfArgs &a, long long nblocks, hipStream_t s) {
  const size_t lds = mf_lds_bytes(a.d, a.p.l2, NW, NP);
  if (a.p.state)
    hipLaunchKernelGGL((sig_fo_mf_kernel<NW, W, M, SEED, true, BLK, false, NP>), dim3((unsigned)nblocks), dim3(64 * NW), lds,
                       s, a);
  else
    hipLaunchKernelGGL((sig_fo_mf_kernel<NW, W, M, SEED, false, BLK, false, NP>), dim3((unsigned)nblocks), dim3(64 * NW), lds,
                       s, a);
  return hipGetLastError() == hipSuccess ? GPSIG_OK : GPSIG_ELAUNCH;
}
template <int NW, int W, int M, int SEED, bool BLK>
static int mf_launch_blk(const MfArgs &a, long long nblocks, hipStream_t s) {
  return mf_geo(a.d, a.p.l2).np == 3 ? mf_launch_np<NW, W, M, SEED, BLK, 3>(a, nblocks, s)
                                     : mf_launch_np<NW, W, M, SEED, BLK, 2>(a, nblocks, s);
}
template <int NW, int W, int M, int SEED>
static int mf_launch_nw(const MfArgs &a, long long nblocks, hipStream_t s) {
  if constexpr (W == 8) {
    if (a.nblk > 1) {  // column blocks: chunks of MF_BLK_CHUNK workgroups share the carry scratch
      MfArgs c = a;
      const long long nl = mf_launches(a.nblk, nblocks);
      for (long long k = 0; k < nl; ++k) {
        const long long b0 = k * MF_BLK_CHUNK;
        c.blk0 = b0;
        const long long nb = nblocks - b0 < MF_BLK_CHUNK ? nblocks - b0 : MF_BLK_CHUNK;
        const int rc = mf_launch_blk<NW, W, M, SEED, true>(c, nb, s);
        if (rc) return rc;
      }
      return GPSIG_OK;
    }
  }
  return mf_launch_blk<NW, W, M, SEED, false>(a, nblocks, s);
}
template <int W, int M, int SEED>
static int mf_launch_w(const MfArgs &a, long long nblocks, hipStream_t s) {
  return dispatch<8, 4>(mf_waves(a.d, a.p.l2),
                        [&](auto nw) { return mf_launch_nw<decltype(nw)::value, W, M, SEED>(a, nblocks, s); });
}

template <int M, int SEED>
static int mf_launch_seed(const MfArgs &a, long long nblocks, hipStream_t s) {
  return dispatch<4, 8, 10>(mf_w(a.p.l2),
                            [&](auto w) { return mf_launch_w<decltype(w)::value, M, SEED>(a, nblocks, s); });
}

template <>
int sig_fo_mf_launch_m<GPSIG_M>(const MfArgs &a, int seed, long long nblocks, hipStream_t s) {
  if (seed == SEED_RBF_DIFF) return mf_launch_seed<GPSIG_M, SEED_RBF_DIFF>(a, nblocks, s);
  if (seed == SEED_LIN_DIFF) return mf_launch_seed<GPSIG_M, SEED_LIN_DIFF>(a, nblocks, s);
  return GPSIG_EUNSUPPORTED;
}

#if GPSIG_M == 1
// The RBF cells of a chunk of pairs into the higher-order recursion's tile (DMO instantiations).
template <int NW, int W, bool BLK, int NP>
static int mf_cells_np(const MfArgs &a, long long nblocks, hipStream_t s) {
  const size_t lds = mf_lds_bytes(a.d, a.p.l2, NW, NP);
  hipLaunchKernelGGL((sig_fo_mf_kernel<NW, W, 1, SEED_RBF_DIFF, false, BLK, true, NP>), dim3((unsigned)nblocks),
                     dim3(64 * NW), lds, s, a);
  return hipGetLastError() == hipSuccess ? GPSIG_OK : GPSIG_ELAUNCH;
}
template <int NW, int W, bool BLK>
static int mf_cells_launch(const MfArgs &a, long long nblocks, hipStream_t s) {
  return mf_geo(a.d, a.p.l2).np == 3 ? mf_cells_np<NW, W, BLK, 3>(a, nblocks, s) : mf_cells_np<NW, W, BLK, 2>(a, nblocks, s);
}
template <int NW>
static int mf_cells_nw(const MfArgs &a, long long nblocks, hipStream_t s) {
  return dispatch<4, 8, 10>(mf_w(a.p.l2), [&](auto w) {
    constexpr int W = decltype(w)::value;
    if constexpr (W == 8)
      if (a.nblk > 1) return mf_cells_launch<NW, 8, true>(a, nblocks, s);
    return mf_cells_launch<NW, W, false>(a, nblocks, s);
  });
}
int sig_fo_mf_cells_launch(const MfArgs &a, long long nblocks, hipStream_t s) {
  return dispatch<8, 4>(mf_waves(a.d, a.p.l2),
                        [&](auto nw) { return mf_cells_nw<decltype(nw)::value>(a, nblocks, s); });
}
#endif

}  // namespace gpsig
