// fsk_mac_dev.h -- one step of a filter's sum, once for fsk_fir.hip and fsk_resample.hip: acc + c * x in the handle's precision.
#pragma once
#include <hip/hip_runtime.h>

namespace fsk {
template <typename Real>
__device__ __forceinline__ Real mac(Real acc, Real c, float x);
template <>
__device__ __forceinline__ double mac<double>(double acc, double c, float x) { return acc + c * (double)x; }  // two roundings (-ffp-contract=off)
template <>
__device__ __forceinline__ float mac<float>(float acc, float c, float x) { return __builtin_fmaf(c, x, acc); }
}  // namespace fsk
