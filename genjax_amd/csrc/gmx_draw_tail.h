// gmx_draw_tail.h — the host statement of gmx_std_normal_from_bits (include/genmi.h): the normal draw's tail of gmx_rng.h
// over an array of chosen bits, as a sequential loop.  Only a plain host compiler building the C-ABI from these headers
// sees it (gmx_vm.h); the device entry point and its kernel are in gmx_kernels.hip.
#pragma once
#if defined(__cplusplus) && !defined(__HIPCC__) && !defined(__HIPCC_RTC__)
#include "genmi.h"
#include "gmx_rng.h"
#include "gmx_sizes.h"
// (`used`: emitted, and so exported by a shared library, although nothing in the translation unit calls it)
extern "C" __attribute__((used)) inline int gmx_std_normal_from_bits(const uint32_t* bits_d, int64_t n, float* out_d, gmx_stream) {
  if (n <= 0) return 0;
  if (!bits_d || !out_d) return gmx_fail("gmx_std_normal_from_bits: null argument%s");
  for (int64_t i = 0; i < n; ++i) out_d[i] = gmx_std_normal_from_bits(bits_d[i]);
  return 0;
}
#endif
