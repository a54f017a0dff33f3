// gsvc_amd/csrc/reduce.h — device-side reductions over a 64-lane wave and over a 256-thread workgroup, gfx950.
//
// Every result is left in ALL lanes / threads.  The wave reductions are the xor butterfly in the order 32, 16, .., 1: a fixed
// order, so a float result is the same bits wherever and whenever it is formed.
#pragma once
#include <hip/hip_runtime.h>

namespace gsvc {

// float, double, int, uint32_t
template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

template <typename T>
__device__ __forceinline__ T wave_max(T v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m, 64));
    return v;
}

template <typename T>
__device__ __forceinline__ T wave_min(T v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m, 64));
    return v;
}

// How block_sum_256 adds the four wave sums s0 .. s3.  Floating-point addition is not associative and both orders feed bit patterns
// that tests pin, so the order is part of every call: keep the one a kernel has.
enum class SumOrder {
    Chain,   // ((s0 + s1) + s2) + s3
    Pairs,   // (s0 + s1) + (s2 + s3)
};

// Whether block_sum_256 may be called again on the same smem without a barrier of the caller's in between.
enum class Slot {
    Reused,   // a barrier in front of the store: two sums in a row, or a loop, on one smem are safe
    Once,     // no barrier in front: for a kernel that sums ONCE.  A second call on the same smem could store a wave's next sum while
              // another wave still reads this one.  (Not folded into Reused: with the barrier k_rate_fwd measured 95.2 -> 97.0 us.)
};

// Sum of v over the 256 threads of a workgroup (float or double); every thread must call it.  smem: four T of LDS.
template <SumOrder ORDER, Slot SLOT = Slot::Reused, typename T>
__device__ __forceinline__ T block_sum_256(T v, T *smem)
{
    v = wave_sum(v);
    if (SLOT == Slot::Reused) __syncthreads();
    if ((threadIdx.x & 63) == 0) smem[threadIdx.x >> 6] = v;
    __syncthreads();
    return ORDER == SumOrder::Chain ? smem[0] + smem[1] + smem[2] + smem[3] : (smem[0] + smem[1]) + (smem[2] + smem[3]);
}

}  // namespace gsvc
