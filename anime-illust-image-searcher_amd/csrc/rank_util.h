// rank_util.h -- the small pieces the ranking kernels of query.hip, crerank.hip and tags.hip share (radius.hip: the scan): the
// order-preserving u32 image of a float, the block-wide exclusive scan and the block-wide maximum.  Device code only.  Everything lives in an anonymous namespace, so
// each including object gets its own copy under the same symbol names.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace {

// Order-preserving u32 image of a float (a > b  <=>  key(a) > key(b) for non-NaN values; 0 is below every real value) and its inverse.
// -0.0 and +0.0 get DIFFERENT images (-0.0 below +0.0): the callers that must treat them as equal use float_order_key_canon.
__device__ __forceinline__ uint32_t float_order_key(float x) {
    const uint32_t u = __float_as_uint(x);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float float_from_key(uint32_t k) {
    return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k);
}
// the variant that maps -0.0 and +0.0 to one image (a sort by this key ties them, as Python's sorted() does)
__device__ __forceinline__ uint32_t float_order_key_canon(float x) {
    if (x == 0.0f) x = 0.0f;
    return float_order_key(x);
}

// Block-wide exclusive scan of one value per thread, for workgroups of 1024 threads (16 waves); returns the exclusive prefix, the
// total in *total.  `scratch` is [17] in LDS and free again on return.
template <typename T>
__device__ __forceinline__ T block_excl_scan(T x, T* scratch /*[17]*/, T* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T incl = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T y = __shfl_up(incl, o);
        if (lane >= o) incl += y;
    }
    if (lane == 63) scratch[wave] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        T run = 0;
        for (int w = 0; w < 16; ++w) {
            const T t = scratch[w];
            scratch[w] = run;
            run += t;
        }
        scratch[16] = run;
    }
    __syncthreads();
    const T res = scratch[wave] + incl - x;
    *total = scratch[16];
    __syncthreads();
    return res;
}

// Block-wide maximum of one value per thread (NaN-free inputs), for workgroups of NT threads: fmax across the wave, one partial per
// wave in LDS, every thread folds the NT / 64 partials in wave order.  max is exact, so the order of the folds does not show in the
// result.  All threads must call it; it holds one barrier.
template <int NT, typename T>
__device__ __forceinline__ T block_max(T v) {
    __shared__ T part[NT / 64];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    v = part[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) v = fmax(v, part[w]);
    return v;
}

}  // namespace
