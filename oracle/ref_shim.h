/*
 * ref_shim.h -- force-included (-include) in front of every reference translation unit that oracle/ref_build.py
 * compiles as host C++.  TEST INFRASTRUCTURE: it lets the reference's CUDA sources build without nvcc and libcudart, so
 * that the oracle can be compared with the reference's own code (tests/test_reference_pin.py).
 *
 * What it provides: the CUDA headers' types (float3, dim3, cudaError_t, ...) from a header-only CUDA include directory,
 * threadIdx / blockIdx / blockDim / gridDim as ordinary mutable globals (defined in oracle/ref_driver.cpp), and the few
 * device intrinsics and symbol calls the sources name.  The runtime calls themselves (cudaMalloc, cudaMemcpy, ...) are
 * defined in oracle/ref_driver.cpp on top of malloc / memcpy.
 */
#pragma once
#include <cuda_runtime.h>
#define __STORAGE__ extern /* device_launch_parameters.h: the launch coordinates become host globals we can assign */
#include <device_launch_parameters.h>
#include <atomic>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <limits>
#include <math.h>
#include <memory>
#include <mutex>
#include <thread>
#include <tuple>
#include <vector>

/* The reference's helper header defines its own fminf / fmaxf for host compilers (plain comparisons: the SECOND operand
 * comes back when one is NaN).  g++ compiles calls to those definitions; clang++ binds the same calls to the C library's
 * fminf / fmaxf, which return the operand that is not NaN.  Every system header is included above, so renaming the two
 * names from here on makes the helper header define, and the reference's code call, functions of these new names under
 * either compiler: the bodies that run are the reference's own.  (Under nvcc that header defines neither and CUDA's
 * NaN-ignoring fminf / fmaxf run instead: see DESIGN.md section 2, what stays unpinned.) */
#define fminf vxref_helper_fminf
#define fmaxf vxref_helper_fmaxf
#include "helper_math.h" /* the reference's, from the include path: every unit gets the same two definitions */

/* float -> integer conversions whose value does not fit are undefined in C++ and defined on the reference's target (PTX
 * cvt.rzi: truncate, clamp to the destination's range, NaN gives 0).  oracle/ref_build.py routes the conversions that
 * ordinary inputs drive out of range through these two (CVT_I32 and CVT_U32 there); every other conversion stays a plain
 * cast, and the cast sanitizer run shows that the pin's inputs keep those in range. */
static inline int vxref_cvt_i32(float v)
{
    if (!(v == v))
        return 0;
    if (v >= 2147483648.0f)
        return 2147483647;
    if (v <= -2147483648.0f)
        return -2147483647 - 1;
    return (int)v;
}
static inline unsigned vxref_cvt_u32(float v)
{
    if (!(v == v) || v <= 0.0f)
        return 0u;
    if (v >= 4294967296.0f)
        return 4294967295u;
    return (unsigned)v;
}

static inline float __saturatef(float x) { return x < 0.f ? 0.f : (x > 1.f ? 1.f : x); }

/* a "device symbol" is the host object itself */
template <class T> static inline cudaError_t cudaGetSymbolAddress(void **p, const T &symbol)
{
    *p = (void *)&symbol;
    return cudaSuccess;
}
template <class T> static inline cudaError_t cudaMemcpyToSymbol(const T &symbol, const void *src, size_t n)
{
    memcpy((void *)&symbol, src, n);
    return cudaSuccess;
}
