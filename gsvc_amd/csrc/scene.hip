// gsvc_amd/csrc/scene.hip — per-plane code histograms of delivered frames, gfx950: what the scene-cut detector of
// gsvc_amd/scene.py reads.
//
// gsvc_frames_histogram   one launch for the n frames of a buffer (frame = blockIdx.y): out[f, p, b] = the number of samples of plane p
//   of frame f whose code falls in bin b = min(code >> (depth - 8), 255).  The min is a safety condition: a deep sample with stray upper
//   bits must not index outside the 256 counters of its plane.
//   A frame is walked as k_picture_hash walks it (frames_common.h, SampleRun: the wide path with 16-byte units and the samples behind the
//   last whole unit one per lane, the edge path one sample per lane, a vector that straddles a plane boundary classified sample by
//   sample); the walk is written here a third time for the reason DESIGN section 8g gives.  What differs from the two sums:
//     a workgroup walks a contiguous stretch of HIST_UNITS_PER_LANE x 256 units in a loop: 8 per lane, twice what the two sums take.  The
//       worry was the flush (1080p 4:2:0 with the sums' 1 024 units per workgroup: 190 workgroups per frame, each with up to 768 global
//       atomics); measured, the flush is not what decides: 4 and 8 per lane are the fastest, 16 and more lose to too few workgroups per
//       launch, 1 and 2 to the zeroing and the flush of the 12 KB of counters (DESIGN section 8h has the sweep);
//     counts are kept in LDS, one copy of the 3 x 256 counters per wave (12 KB), so that the four waves do not contend;
//     the samples of a lane's vector are neighbours and often equal: a run of equal bins is counted in a register and sent to LDS as
//       ONE atomic.  A constant picture costs one LDS atomic per vector (per channel for rgb24), noise one per sample.
//   The flush adds the four copies and issues one 32-bit atomicAdd per non-zero bin.  Integer sums: the same bits for every launch shape.
//   Nothing past the last sample of a frame is read.
#include "frames_common.h"

namespace gsvc {

// The two decisions above were taken by measurement (tools/bench_scene.py); the two macros build the alternatives
// it measured and are not set by the Makefile.
#ifndef GSVC_HIST_UNITS_PER_LANE
#define GSVC_HIST_UNITS_PER_LANE 8
#endif
constexpr int HIST_UNITS_PER_LANE = GSVC_HIST_UNITS_PER_LANE;        // units (wide) or samples (edge) per lane of a workgroup, 256 apart
constexpr int HIST_BINS = 256;

struct HistArgs {
    const uint8_t *a;
    long long stride;
    uint32_t *out;                     // [n, 3, 256]
    SampleRun run;
    int shift;                         // depth - 8
};

__device__ __forceinline__ uint32_t hist_bin(uint32_t code, int shift)
{
    const uint32_t b = code >> shift;
    return b < 255u ? b : 255u;
}

// a run of equal bins of one plane, kept in registers; `slot` = plane * 256 + bin
struct BinRun {
    uint32_t slot, count;
};

__device__ __forceinline__ void run_flush(uint32_t *h, const BinRun &r)
{
    atomicAdd(&h[r.slot], r.count);
}

__device__ __forceinline__ void run_add(uint32_t *h, BinRun &r, uint32_t slot)
{
#ifdef GSVC_HIST_NO_RUNS
    if (false) {
#else
    if (slot == r.slot) {
#endif
        r.count++;
    } else {
        run_flush(h, r);
        r.slot = slot;
        r.count = 1u;
    }
}

// one sample at flat index f of the frame
template <bool RGB>
__device__ __forceinline__ void hist_sample(uint32_t *h, const SampleRun &g, long long f, uint32_t bin)
{
    int p;
    if (RGB) {
        const uint32_t px = (uint32_t)f / 3u;          // (a frame has at most 3 * 2^30 samples)
        p = (int)((uint32_t)f - 3u * px);
    } else {
        p = (f >= g.p0) + (f >= g.p1);
    }
    atomicAdd(&h[p * HIST_BINS + (int)bin], 1u);
}

template <int BPS, bool RGB, bool WIDE>
__global__ void __launch_bounds__(256) k_frames_histogram(HistArgs args)
{
    __shared__ uint32_t counts[4][3 * HIST_BINS];
    for (int i = threadIdx.x; i < 4 * 3 * HIST_BINS; i += 256) (&counts[0][0])[i] = 0u;
    __syncthreads();
    uint32_t *h = counts[threadIdx.x >> 6];
    const SampleRun &g = args.run;
    const uint8_t *a = args.a + (size_t)blockIdx.y * (size_t)args.stride;
    const int shift = args.shift;
    const long long first = (long long)blockIdx.x * (256 * HIST_UNITS_PER_LANE) + threadIdx.x;
    if (WIDE) {
        constexpr int SPV = 16 / BPS;                    // samples of a 16-byte vector
        constexpr int SPU = RGB ? 3 * SPV : SPV;         // samples of a unit
        constexpr int NW = SPU * BPS / 4;                // its 32-bit words
        const long long units = g.samples / SPU, tail0 = units * SPU;
        for (int j = 0; j < HIST_UNITS_PER_LANE; j++) {
            const long long unit = first + 256 * j;
            if (unit < units) {
                const long long f0 = unit * SPU;
                uint32_t wa[NW];
                load_words<4 * NW>(a + f0 * BPS, wa);
                if (RGB) {
#pragma unroll
                    for (int c = 0; c < 3; c++) {          // sample k of a unit is channel k mod 3: 16 samples per channel
                        BinRun r = {(uint32_t)(c * HIST_BINS) + hist_bin(code_of<1>(wa, c), 0), 1u};
#pragma unroll
                        for (int k = c + 3; k < SPU; k += 3) run_add(h, r, (uint32_t)(c * HIST_BINS) + hist_bin(code_of<1>(wa, k), 0));
                        run_flush(h, r);
                    }
                } else {
                    const long long fl = f0 + SPV - 1;
                    const int pf = (f0 >= g.p0) + (f0 >= g.p1), pl = (fl >= g.p0) + (fl >= g.p1);
                    if (pf == pl) {
                        const uint32_t base = (uint32_t)(pf * HIST_BINS);
                        BinRun r = {base + hist_bin(code_of<BPS>(wa, 0), shift), 1u};
#pragma unroll
                        for (int k = 1; k < SPV; k++) run_add(h, r, base + hist_bin(code_of<BPS>(wa, k), shift));
                        run_flush(h, r);
                    } else {                              // a plane boundary inside the vector
#pragma unroll
                        for (int k = 0; k < SPV; k++) hist_sample<false>(h, g, f0 + k, hist_bin(code_of<BPS>(wa, k), shift));
                    }
                }
            } else {
                const long long f = tail0 + (unit - units);
                if (f < g.samples) hist_sample<RGB>(h, g, f, hist_bin(code_at<BPS>(a, f), shift));
            }
        }
    } else {
        for (int j = 0; j < HIST_UNITS_PER_LANE; j++) {
            const long long f = first + 256 * j;
            if (f < g.samples) hist_sample<RGB>(h, g, f, hist_bin(code_at<BPS>(a, f), shift));
        }
    }
    __syncthreads();
    uint32_t *out = args.out + (size_t)blockIdx.y * (3 * HIST_BINS);
    for (int i = threadIdx.x; i < 3 * HIST_BINS; i += 256) {
        const uint32_t v = counts[0][i] + counts[1][i] + counts[2][i] + counts[3][i];
        if (v) atomicAdd(&out[i], v);
    }
}

}  // namespace gsvc

using namespace gsvc;

extern "C" int gsvc_frames_histogram(const uint8_t *frames, int64_t stride, int32_t n, int32_t H, int32_t W, int32_t layout, int32_t depth,
                                     uint32_t *out, void *stream)
{
    GSVC_REQUIRE(frames && out, "frames_histogram: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    FrameSums fs;
    GSVC_FRAMES_TRY(frames_sums_setup("frames_histogram", FrameBufs{"stride", frames, stride, nullptr, 0}, n, H, W, layout, depth, out, s, fs,
                                      (int)sizeof(uint32_t), 3 * HIST_BINS));
    const HistArgs g = {frames, stride, out, fs.run, depth - 8};
    const int64_t per_block = 256 * HIST_UNITS_PER_LANE;
    const dim3 grid((unsigned)((fs.units + per_block - 1) / per_block), (unsigned)n);
    static void (*const kernels[3][2])(HistArgs) = GSVC_FRAME_SUMS_KERNELS(k_frames_histogram);
    ProfScope _p("k_frames_histogram", s);
    hipLaunchKernelGGL(kernels[fs.variant][fs.wide], grid, dim3(256), 0, s, g);
    return check_launch("frames_histogram");
}
