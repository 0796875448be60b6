// Single translation unit of libstil_hip.so (gfx950).  C ABI declared in include/stil_hip.h.
#include "common.h"
#include <stdarg.h>

static thread_local char g_err[512] = "";
void stil_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* stil_last_error(void) { return g_err; }
extern "C" int stil_version(void) { return 106; }   // 106: stil_alb_* (albumentations branch of the input pipeline)
// number of HIP devices visible (0 = none): lets the host fail loudly before any launch
extern "C" int stil_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

#include "gemm.hip"
#include "bn.hip"
#include "bn_prior.hip"
#include "bn_memory.hip"
#include "transformer.hip"
#include "loss.hip"
#include "saint.hip"
#include "optim.hip"
#include "augment.hip"
#include "augment_alb.hip"
#include "layout.hip"
#include "state.hip"
// the adaptation files share through tta_common.h, which each includes itself: their order is free, but for read.hip, which
// launches two kernels of infomax.hip and so comes after it
#include "tta.hip"
#include "eata.hip"
#include "infomax.hip"
#include "margent.hip"
#include "deyo.hip"
#include "sar.hip"
#include "read.hip"
#include "cgpl.hip"
#include "roid.hip"
#include "rotta.hip"
#include "lame.hip"
#include "shift.hip"
