// gsvc_amd/csrc/picture_hash.hip — the picture hash of the bitstream file (section PHSH), gfx950: per frame and plane
// a 64-bit sum over the delivered sample codes that depends on where a sample sits.
//
// gsvc_picture_hash   one launch for the n frames of a buffer (frame = blockIdx.y), the shape of k_frames_sse (metrics.hip) reading one
//   buffer: a frame is ONE flat run of samples and a plane a range of sample indices, plane(f) = (f >= HW) + (f >= HW + chroma samples)
//   with s = f - the plane's first sample; rgb24's channel is f mod 3 and s = f / 3.  Per sample, all in uint32:
//     x = s * 0x9E3779B1 ^ (c + 1) * 0x85EBCA6B;  x ^= x >> 15;  x *= 0x2C1B3C6D;  x ^= x >> 12
//   and hash[p] = the sum of x over the plane modulo 2^64.  A lane's three accumulators are 64-bit; a wave reduces them with shuffles,
//   the workgroup through LDS, and one thread per plane issues one 64-bit integer atomic — integer addition is associative: the
//   result is the same bits in every run and for every launch shape.
//     wide path   (base and, for n > 1, stride 16-byte aligned): a lane takes 16 bytes per unit and four units 256 units apart
//                 (rgb24: 48 bytes = three vectors = 16 pixels per unit, so that byte j of a unit is channel j mod 3 of pixel j / 3).
//                 A vector may straddle a plane boundary (H W = 60: U starts at byte 60): its samples are then classified one by
//                 one.  The samples behind the last whole unit of the frame are taken one per lane by the units that follow.
//     edge path   one sample per lane and four samples 256 apart, at any alignment (deep formats: even).
//   Nothing past the last sample of a frame is read.
#include "common.h"

namespace gsvc {

constexpr int PH_PER_LANE = 4;           // units (wide) or samples (edge) per lane, 256 apart

struct HashArgs {
    const uint8_t *a;
    long long stride;
    unsigned long long *out;           // [n, 3]
    long long samples;                 // of one frame
    long long p0, p1;                  // first sample of the second / third plane (planar layouts)
};

__device__ __forceinline__ uint32_t ph_mix(uint32_t s, uint32_t c)
{
    uint32_t x = (s * 0x9E3779B1u) ^ ((c + 1u) * 0x85EBCA6Bu);
    x ^= x >> 15;
    x *= 0x2C1B3C6Du;
    x ^= x >> 12;
    return x;
}

template <int BPS>
__device__ __forceinline__ uint32_t ph_code_of(const uint32_t *w, int k)
{
    return BPS == 1 ? (w[k >> 2] >> (8 * (k & 3))) & 255u : (w[k >> 1] >> (16 * (k & 1))) & 65535u;
}

template <int BPS>
__device__ __forceinline__ uint32_t ph_code_at(const uint8_t *p, long long f)
{
    return BPS == 1 ? (uint32_t)p[f] : (uint32_t)reinterpret_cast<const uint16_t *>(p)[f];
}

__device__ __forceinline__ void ph_add(unsigned long long acc[3], int plane, unsigned long long v)
{
    acc[0] += plane == 0 ? v : 0ull;
    acc[1] += plane == 1 ? v : 0ull;
    acc[2] += plane == 2 ? v : 0ull;
}

// one sample at flat index f of the frame
template <int BPS, bool RGB>
__device__ __forceinline__ void ph_sample(unsigned long long acc[3], const HashArgs &g, long long f, uint32_t c)
{
    if (RGB) {
        const uint32_t px = (uint32_t)f / 3u;          // (a frame has at most 3 * 2^30 samples)
        ph_add(acc, (int)((uint32_t)f - 3u * px), ph_mix(px, c));
    } else {
        const int p = (f >= g.p0) + (f >= g.p1);
        const long long start = p == 0 ? 0ll : (p == 1 ? g.p0 : g.p1);
        ph_add(acc, p, ph_mix((uint32_t)(f - start), c));
    }
}

template <int BPS, bool RGB, bool WIDE>
__global__ void __launch_bounds__(256) k_picture_hash(HashArgs g)
{
    __shared__ unsigned long long red[4][3];
    const uint8_t *a = g.a + (size_t)blockIdx.y * (size_t)g.stride;
    unsigned long long acc[3] = {0ull, 0ull, 0ull};
    const long long first = (long long)blockIdx.x * (256 * PH_PER_LANE) + threadIdx.x;
    if (WIDE) {
        constexpr int SPV = 16 / BPS;                    // samples of a 16-byte vector
        constexpr int SPU = RGB ? 3 * SPV : SPV;         // samples of a unit
        const long long units = g.samples / SPU, tail0 = units * SPU;
#pragma unroll
        for (int j = 0; j < PH_PER_LANE; j++) {
            const long long unit = first + 256 * j;
            if (unit < units) {
                const long long f0 = unit * SPU;
                if (RGB) {
                    const uint4 *pa = reinterpret_cast<const uint4 *>(a + f0);
                    const uint4 a0 = pa[0], a1 = pa[1], a2 = pa[2];
                    const uint32_t wa[12] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w};
                    const uint32_t px0 = (uint32_t)unit * 16u;
                    unsigned long long t[3] = {0ull, 0ull, 0ull};
#pragma unroll
                    for (int k = 0; k < 48; k++) t[k % 3] += ph_mix(px0 + (uint32_t)(k / 3), ph_code_of<1>(wa, k));
                    acc[0] += t[0];
                    acc[1] += t[1];
                    acc[2] += t[2];
                } else {
                    const uint4 qa = *reinterpret_cast<const uint4 *>(a + f0 * BPS);
                    const uint32_t wa[4] = {qa.x, qa.y, qa.z, qa.w};
                    const long long fl = f0 + SPV - 1;
                    const int pf = (f0 >= g.p0) + (f0 >= g.p1), pl = (fl >= g.p0) + (fl >= g.p1);
                    if (pf == pl) {
                        const long long start = pf == 0 ? 0ll : (pf == 1 ? g.p0 : g.p1);
                        const uint32_t s0 = (uint32_t)(f0 - start);
                        unsigned long long t = 0ull;
#pragma unroll
                        for (int k = 0; k < SPV; k++) t += ph_mix(s0 + (uint32_t)k, ph_code_of<BPS>(wa, k));
                        ph_add(acc, pf, t);
                    } else {                              // a plane boundary inside the vector
#pragma unroll
                        for (int k = 0; k < SPV; k++) ph_sample<BPS, false>(acc, g, f0 + k, ph_code_of<BPS>(wa, k));
                    }
                }
            } else {
                const long long f = tail0 + (unit - units);
                if (f < g.samples) ph_sample<BPS, RGB>(acc, g, f, ph_code_at<BPS>(a, f));
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < PH_PER_LANE; j++) {
            const long long f = first + 256 * j;
            if (f < g.samples) ph_sample<BPS, RGB>(acc, g, f, ph_code_at<BPS>(a, f));
        }
    }
    // wave, then workgroup, then one atomic per plane
#pragma unroll
    for (int p = 0; p < 3; p++) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const uint32_t lo = __shfl_xor((uint32_t)acc[p], m, 64), hi = __shfl_xor((uint32_t)(acc[p] >> 32), m, 64);
            acc[p] += ((unsigned long long)hi << 32) | lo;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        red[wave][0] = acc[0];
        red[wave][1] = acc[1];
        red[wave][2] = acc[2];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const unsigned long long v = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
        if (v) atomicAdd(&g.out[3 * (size_t)blockIdx.y + threadIdx.x], v);
    }
}

}  // namespace gsvc

using namespace gsvc;

extern "C" int gsvc_picture_hash(const uint8_t *frames, int64_t stride, int32_t n, int32_t H, int32_t W, int32_t layout, int32_t depth,
                                 uint64_t *out, void *stream)
{
    GSVC_REQUIRE(frames && out, "picture_hash: NULL pointer");
    GSVC_REQUIRE(n >= 1 && n <= 65535, "picture_hash: n must be 1 .. 65535 (got %d)", (int)n);
    GSVC_REQUIRE(layout == GSVC_FRAMES_RGB24 || layout == GSVC_FRAMES_YUV444P || layout == GSVC_FRAMES_YUV420P,
                 "picture_hash: unknown layout %d", (int)layout);
    GSVC_REQUIRE(depth >= 8 && depth <= 16, "picture_hash: depth must be 8 .. 16 (got %d)", (int)depth);
    GSVC_REQUIRE(layout != GSVC_FRAMES_RGB24 || depth == 8, "picture_hash: rgb24 frames are 8-bit only");
    GSVC_REQUIRE(H >= 1 && W >= 1 && H <= 32768 && W <= 32768, "picture_hash: image size must be 1 .. 32768 (got %d x %d)", (int)H, (int)W);
    GSVC_REQUIRE(layout != GSVC_FRAMES_YUV420P || (H % 2 == 0 && W % 2 == 0), "picture_hash: yuv420p needs even H and W (got %d x %d)",
                 (int)H, (int)W);
    const int64_t bytes = gsvc_frames_bytes(H, W, layout, depth);
    GSVC_REQUIRE(stride >= bytes, "picture_hash: stride %lld is shorter than a frame (%lld bytes)", (long long)stride, (long long)bytes);
    const bool deep = depth > 8;
    if (deep) {
        GSVC_REQUIRE((reinterpret_cast<uintptr_t>(frames) & 1) == 0, "picture_hash: the frame base is not 2-byte aligned");
        GSVC_REQUIRE((stride & 1) == 0, "picture_hash: stride %lld is not a multiple of 2", (long long)stride);
    }
    GSVC_REQUIRE((reinterpret_cast<uintptr_t>(out) & 7) == 0, "picture_hash: out is not 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(out, 0, (size_t)n * 3 * sizeof(uint64_t), s) != hipSuccess) {
        set_error("picture_hash: hipMemsetAsync failed");
        return GSVC_E_LAUNCH;
    }
    HashArgs g;
    g.a = frames;
    g.stride = stride;
    g.out = reinterpret_cast<unsigned long long *>(out);
    const int64_t px = (int64_t)H * W, chroma = layout == GSVC_FRAMES_YUV420P ? px / 4 : px;
    g.samples = bytes / (deep ? 2 : 1);
    g.p0 = px;
    g.p1 = px + chroma;
    uintptr_t align = reinterpret_cast<uintptr_t>(frames);
    if (n > 1) align |= (uintptr_t)stride;
    const bool wide = (align & 15) == 0;
    const bool rgb = layout == GSVC_FRAMES_RGB24;
    int64_t units = g.samples;
    if (wide) {
        const int64_t spu = rgb ? 48 : (deep ? 8 : 16);
        units = g.samples / spu + g.samples % spu;          // whole units, then the samples behind them one by one
    }
    const int64_t per_block = 256 * PH_PER_LANE;
    const dim3 grid((unsigned)((units + per_block - 1) / per_block), (unsigned)n), block(256);
    ProfScope _p("k_picture_hash", s);
    if (rgb) {
        if (wide) hipLaunchKernelGGL((k_picture_hash<1, true, true>), grid, block, 0, s, g);
        else hipLaunchKernelGGL((k_picture_hash<1, true, false>), grid, block, 0, s, g);
    } else if (!deep) {
        if (wide) hipLaunchKernelGGL((k_picture_hash<1, false, true>), grid, block, 0, s, g);
        else hipLaunchKernelGGL((k_picture_hash<1, false, false>), grid, block, 0, s, g);
    } else {
        if (wide) hipLaunchKernelGGL((k_picture_hash<2, false, true>), grid, block, 0, s, g);
        else hipLaunchKernelGGL((k_picture_hash<2, false, false>), grid, block, 0, s, g);
    }
    return check_launch("picture_hash");
}
