// gsvc_amd/csrc/common.h — shared host-side helpers of libgsvc_hip.so (error slot, launch checks).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/gsvc_hip.h"

namespace gsvc {

void set_error(const char *fmt, ...);

inline int check_launch(const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return GSVC_E_LAUNCH;
    }
    return GSVC_OK;
}

// bench.py's per-kernel timer: brackets a launch with events on its stream when profiling is enabled
bool profile_enabled();
bool bwd_probe_enabled();      // gsvc_profile_enable bit 1: k_blend_bwd_tile counts its replays (diagnostic instantiation)
bool deterministic();           // gsvc_set_deterministic: launches whose float sums depend on workgroup order take their fixed-order form
void profile_begin(const char *name, hipStream_t s);
void profile_end(hipStream_t s);

struct ProfScope {
    hipStream_t s;
    bool on;
    ProfScope(const char *name, hipStream_t stream) : s(stream), on(profile_enabled())
    {
        if (on) profile_begin(name, s);
    }
    ~ProfScope()
    {
        if (on) profile_end(s);
    }
};

inline uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

// Zeroing of a buffer inside an entry point: a kernel, not hipMemsetAsync.  A hipMemsetAsync captured into a graph by torch.cuda.graph
// replayed correctly the first time and from the second replay on left other words than zero where only the memset writes (the
// low byte of each 32-bit word 0, the other three stray; 0x60606060 in a 4-byte buffer), with nothing but the replay between the
// right and the wrong result; the kernels of the same graphs were right every time (tests/test_abi_contract_gpu.py, the ssim_l1,
// ste_binary, yuv_planes and picture_hash cases before this).  A stand-alone HIP program that captures the same memsets replays
// them as zeros, so the fault needs more than the call itself and its cause inside the runtime is not known; a kernel's
// arguments are kept by the graph by value.  p: 4-byte aligned, bytes: a multiple of 4 (every caller zeroes 4- or 8-byte elements).
template <int = 0>
__global__ void __launch_bounds__(256) k_zero_words(uint32_t *__restrict__ p, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = 0u;
}

inline hipError_t zero_words_async(void *p, size_t bytes, hipStream_t s)
{
    const size_t n = bytes / 4;
    if (n == 0) return hipSuccess;
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_zero_words<0>, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, s, static_cast<uint32_t *>(p), n);
    return hipGetLastError();
}

}  // namespace gsvc

#define GSVC_REQUIRE(cond, ...)            \
    do {                                   \
        if (!(cond)) {                     \
            gsvc::set_error(__VA_ARGS__);  \
            return GSVC_E_INVALID;         \
        }                                  \
    } while (0)
