// The priority of a candidate in the greedy NMS kernels (nms_fast.hip, nms_map.hip): the higher score first, then the lower
// raster index, packed into one 64-bit key.  One definition, so that the tie rule is fixed in one place.
#pragma once
#include <hip/hip_runtime.h>

namespace balf {
namespace {

constexpr unsigned KEY_BIAS = 0x00100000u;   // keeps a key's high word out of the double's denormal range

// a key is a positive normal double: (score bits + 2^20) << 32 | ~index orders exactly like the unsigned integer; +0 = no candidate
__device__ __forceinline__ double make_key(float v, int idx) {
    const unsigned long long k = ((unsigned long long)(__float_as_uint(v) + KEY_BIAS) << 32) | (unsigned long long)(0xffffffffu - (unsigned)idx);
    return __longlong_as_double((long long)k);
}
// maximum of two keys (positive normal doubles or +0) = the unsigned maximum of their bit patterns, in one instruction
__device__ __forceinline__ double kmax(double x, double y) {
    asm("v_max_f64 %0, %0, %1" : "+v"(x) : "v"(y));      // ("+v": the repo-wide rule for inline-asm VALU, test_build_invariants.py)
    return x;
}

}  // namespace
}  // namespace balf
