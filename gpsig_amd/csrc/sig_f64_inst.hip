// gpsig_amd -- explicit instantiation unit: the float64 first-order kernels of one level count.  Compiled
// once per GPSIG_M by gpsig_amd/csrc/Makefile.
#include "internal.h"
#include "sig_f64.h"
#if !defined(GPSIG_M)
#error "GPSIG_M must be defined"
#endif
namespace gpsig {
// the (W, LP) table of f64_geometry
template <int M>
int sig_f64_launch_m(const F64Args &a, int W, int LP, long long nblocks, hipStream_t s) {
  if (W == 4 && LP == 16) return launch_f64<4, 16, M>(a, nblocks, s);
  if (W == 4 && LP == 32) return launch_f64<4, 32, M>(a, nblocks, s);
  if (W == 4 && LP == 64) return launch_f64<4, 64, M>(a, nblocks, s);
  if (W == 8 && LP == 64) return launch_f64<8, 64, M>(a, nblocks, s);
  return GPSIG_EUNSUPPORTED;
}

template int sig_f64_launch_m<GPSIG_M>(const F64Args &, int, int, long long, hipStream_t);
}
