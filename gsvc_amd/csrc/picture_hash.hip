// gsvc_amd/csrc/picture_hash.hip — the picture hash of the bitstream file (section PHSH), gfx950: per frame and plane
// a 64-bit sum over the delivered sample codes that depends on where a sample sits.
//
// gsvc_picture_hash   one launch for the n frames of a buffer (frame = blockIdx.y), the walk of k_frames_sse (metrics.hip) over one
//   buffer.  The two share the sample helpers, the 64-bit three-plane reduction (add_block_sums) and the host part (frames_sums_setup)
//   through frames_common.h; the walk itself is written in both (DESIGN section 8g says why).  A frame is ONE flat run of samples and
//   a plane a range of sample indices, plane(f) = (f >= HW) + (f >= HW + chroma samples) with s = f - the plane's first sample;
//   rgb24's channel is f mod 3 and s = f / 3.  Per sample, all in uint32:
//     x = s * 0x9E3779B1 ^ (c + 1) * 0x85EBCA6B;  x ^= x >> 15;  x *= 0x2C1B3C6D;  x ^= x >> 12
//   and hash[p] = the sum of x over the plane modulo 2^64 — integer addition is associative: the result is the same bits in every run
//   and for every launch shape.
//     wide path   (base and, for n > 1, stride 16-byte aligned): a lane takes 16 bytes per unit (rgb24: 48 bytes = 16 pixels)
//     edge path   one sample per lane, at any alignment (deep formats: even).
//   Nothing past the last sample of a frame is read.
#include "frames_common.h"

namespace gsvc {

struct HashArgs {
    const uint8_t *a;
    long long stride;
    unsigned long long *out;           // [n, 3]
    SampleRun run;
};

__device__ __forceinline__ uint32_t ph_mix(uint32_t s, uint32_t c)
{
    uint32_t x = (s * 0x9E3779B1u) ^ ((c + 1u) * 0x85EBCA6Bu);
    x ^= x >> 15;
    x *= 0x2C1B3C6Du;
    x ^= x >> 12;
    return x;
}

// one sample at flat index f of the frame
template <bool RGB>
__device__ __forceinline__ void ph_sample(unsigned long long acc[3], const SampleRun &g, long long f, uint32_t c)
{
    if (RGB) {
        const uint32_t px = (uint32_t)f / 3u;          // (a frame has at most 3 * 2^30 samples)
        add_to_plane(acc, (int)((uint32_t)f - 3u * px), ph_mix(px, c));
    } else {
        const int p = (f >= g.p0) + (f >= g.p1);
        const long long start = p == 0 ? 0ll : (p == 1 ? g.p0 : g.p1);
        add_to_plane(acc, p, ph_mix((uint32_t)(f - start), c));
    }
}

// the walk of frames_common.h (SampleRun); the per-sample work: the mix of a sample's index inside its plane and its code
template <int BPS, bool RGB, bool WIDE>
__global__ void __launch_bounds__(256) k_picture_hash(HashArgs args)
{
    const SampleRun &g = args.run;
    const uint8_t *a = args.a + (size_t)blockIdx.y * (size_t)args.stride;
    unsigned long long acc[3] = {0ull, 0ull, 0ull};
    const long long first = (long long)blockIdx.x * (256 * SUMS_PER_LANE) + threadIdx.x;
    if (WIDE) {
        constexpr int SPV = 16 / BPS;                    // samples of a 16-byte vector
        constexpr int SPU = RGB ? 3 * SPV : SPV;         // samples of a unit
        constexpr int NW = SPU * BPS / 4;                // its 32-bit words
        const long long units = g.samples / SPU, tail0 = units * SPU;
#pragma unroll
        for (int j = 0; j < SUMS_PER_LANE; j++) {
            const long long unit = first + 256 * j;
            if (unit < units) {
                const long long f0 = unit * SPU;
                uint32_t wa[NW];
                load_words<4 * NW>(a + f0 * BPS, wa);
                if (RGB) {
                    const uint32_t px0 = (uint32_t)unit * 16u;
                    unsigned long long t[3] = {0ull, 0ull, 0ull};
#pragma unroll
                    for (int k = 0; k < SPU; k++) t[k % 3] += ph_mix(px0 + (uint32_t)(k / 3), code_of<1>(wa, k));
                    acc[0] += t[0];
                    acc[1] += t[1];
                    acc[2] += t[2];
                } else {
                    const long long fl = f0 + SPV - 1;
                    const int pf = (f0 >= g.p0) + (f0 >= g.p1), pl = (fl >= g.p0) + (fl >= g.p1);
                    if (pf == pl) {
                        const long long start = pf == 0 ? 0ll : (pf == 1 ? g.p0 : g.p1);
                        const uint32_t s0 = (uint32_t)(f0 - start);
                        unsigned long long t = 0ull;
#pragma unroll
                        for (int k = 0; k < SPV; k++) t += ph_mix(s0 + (uint32_t)k, code_of<BPS>(wa, k));
                        add_to_plane(acc, pf, t);
                    } else {                              // a plane boundary inside the vector
#pragma unroll
                        for (int k = 0; k < SPV; k++) ph_sample<false>(acc, g, f0 + k, code_of<BPS>(wa, k));
                    }
                }
            } else {
                const long long f = tail0 + (unit - units);
                if (f < g.samples) ph_sample<RGB>(acc, g, f, code_at<BPS>(a, f));
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < SUMS_PER_LANE; j++) {
            const long long f = first + 256 * j;
            if (f < g.samples) ph_sample<RGB>(acc, g, f, code_at<BPS>(a, f));
        }
    }
    add_block_sums(acc, args.out + 3 * (size_t)blockIdx.y);
}

}  // namespace gsvc

using namespace gsvc;

extern "C" int gsvc_picture_hash(const uint8_t *frames, int64_t stride, int32_t n, int32_t H, int32_t W, int32_t layout, int32_t depth,
                                 uint64_t *out, void *stream)
{
    GSVC_REQUIRE(frames && out, "picture_hash: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    FrameSums fs;
    GSVC_FRAMES_TRY(frames_sums_setup("picture_hash", FrameBufs{"stride", frames, stride, nullptr, 0}, n, H, W, layout, depth, out, s, fs));
    const HashArgs g = {frames, stride, reinterpret_cast<unsigned long long *>(out), fs.run};
    static void (*const kernels[3][2])(HashArgs) = GSVC_FRAME_SUMS_KERNELS(k_picture_hash);
    ProfScope _p("k_picture_hash", s);
    hipLaunchKernelGGL(kernels[fs.variant][fs.wide], fs.grid, dim3(256), 0, s, g);
    return check_launch("picture_hash");
}
