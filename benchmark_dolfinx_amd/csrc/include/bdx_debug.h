// Debug checks of index paths, usable from code shared by the device kernels
// and the host runtime.
//
// Debug builds (BDX_DEBUG=1: `python -m benchmark_dolfinx_amd.ops.build
// --variant debug=-DBDX_DEBUG=1`, loaded with BDX_HIP_LIB) turn on
// device-side checks of the operator kernels' LDS and global index paths; a
// failing check prints the expression and aborts the process (HIP device
// assert) instead of reading or writing out of bounds.  Release builds compile
// them out, and so does every host compilation (the checks print the block and
// thread of the offender).
#pragma once

#ifndef BDX_DEBUG
#define BDX_DEBUG 0
#endif
#if BDX_DEBUG && defined(__HIP_DEVICE_COMPILE__)
// report (do not trap: a trapped wave would take the queue down with it)
#define BDX_DASSERT(c) \
  ((c) ? (void)0 : (void)printf("[bdx ASSERT] %s:%d %s\n", __FILE__, __LINE__, #c))
// out-of-range global offset: print the first few offenders, skip the access
#define BDX_OOB(off, n, tag)                                                        \
  (((off) < 0 || (off) >= (n))                                                      \
       ? (printf("[bdx OOB] %s off=%lld n=%lld block=%d thread=%d\n", tag,          \
                 static_cast<long long>(off), static_cast<long long>(n),            \
                 static_cast<int>(blockIdx.x), static_cast<int>(threadIdx.x)),      \
          true)                                                                     \
       : false)
#else
#define BDX_DASSERT(c) ((void)0)
#define BDX_OOB(off, n, tag) false
#endif
