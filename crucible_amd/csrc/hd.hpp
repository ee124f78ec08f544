// hd.hpp -- what CR_HD and CR_D mean, decided by the compiler and not by the order of includes.  Under
// hipcc: the HIP runtime's declarations, CR_HD a function of host and device, CR_D one of the device, both always inlined.
// Under a plain C++ compiler: CR_HD an inline function, nothing of HIP read, and no CR_D -- device code stays behind
// `#if defined(__HIPCC__)`.  Every header that uses one of the two includes this one.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CR_HD __host__ __device__ __forceinline__
#define CR_D __device__ __forceinline__
#else
#define CR_HD inline
#endif
