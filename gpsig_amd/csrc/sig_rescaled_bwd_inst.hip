// gpsig_amd -- instantiations of the rescaled kernel's VJP (sig_rescaled_bwd.h) for one level (GPSIG_LVL):
// W = 1 / 2 columns per lane (l - 1 <= 64 / 128), W = 4 (l - 1 <= 256) up to level 4; both embeddings.
#include "internal.h"
#include "sig_rescaled_bwd.h"

#ifndef GPSIG_LVL
#error "GPSIG_LVL"
#endif

namespace gpsig {

template <int I, int W>
static int launch_rs_bwd(RsBwdArgs a, hipStream_t s) {
  // the accumulators of gZ and gX in LDS while they fit beside the multipliers
  a.direct = rs_bwd_lds_bytes(I, W, a.d, false) > RS_BWD_LDS_MAX ? 1 : 0;
  const size_t lds = rs_bwd_lds_bytes(I, W, a.d, a.direct != 0);
  const dim3 grid((unsigned)((long long)a.n * (a.t + 1)));
  if (a.emb == 1)
    hipLaunchKernelGGL((rescaled_bwd_kernel<I, W, true>), grid, dim3(64), lds, s, a);
  else
    hipLaunchKernelGGL((rescaled_bwd_kernel<I, W, false>), grid, dim3(64), lds, s, a);
  return hipGetLastError() == hipSuccess ? GPSIG_OK : GPSIG_ELAUNCH;
}

template <>
int rescaled_bwd_launch_level<GPSIG_LVL>(const RsBwdArgs &a, hipStream_t s) {
  constexpr int I = GPSIG_LVL;
  if (a.l - 1 <= 64) return launch_rs_bwd<I, 1>(a, s);
  if (a.l - 1 <= 128) return launch_rs_bwd<I, 2>(a, s);
  if constexpr (I <= 4) {
    if (a.l - 1 <= 256) return launch_rs_bwd<I, 4>(a, s);
  }
  return GPSIG_EUNSUPPORTED;
}

}  // namespace gpsig
