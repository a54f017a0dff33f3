// gsvc_amd/csrc/frames_common.h — what frames_out.hip, frames_in.hip, metrics.hip (plane SSE), picture_hash.hip and scene.hip share: the
// frame format stated once.
//   host     the argument checks of the six entries (their texts carry the entry's name), the colour matrix and the range constants as
//            functions of (matrix) and (range, depth), the gather of a batch's image pointers, and the host part of the per-plane
//            sums (gsvc_frames_sse, gsvc_picture_hash, gsvc_frames_histogram): checks, memset, launch shape, dispatch;
//   device   sample codes out of loaded words, vector loads and stores by byte count, and the 64-bit three-plane workgroup reduction of
//            the two per-plane sums.  (Their walks over a frame's samples stay two bodies of one shape, k_frames_sse and
//            k_picture_hash: as one template over the per-sample work the 8-bit wide instantiations took 74 - 108 registers
//            instead of 34 - 52 and lost occupancy)
#pragma once
#include "common.h"

namespace gsvc {

// ============================================================================================================================
// host: the checks, in the order the entries make them (a call with two bad arguments reports the first)
// ============================================================================================================================
// the one or two buffers of frames of an entry; stride_name is what the entry's error texts call the stride
struct FrameBufs {
    const char *stride_name;
    const void *a;
    int64_t stride_a;
    const void *b;                      // NULL: one buffer
    int64_t stride_b;

    void strides_text(char (&s)[48]) const
    {
        if (b) snprintf(s, sizeof(s), "%lld / %lld", (long long)stride_a, (long long)stride_b);
        else snprintf(s, sizeof(s), "%lld", (long long)stride_a);
    }
    // what the wide paths need 16-byte aligned: every base and, where a second frame is addressed, every stride
    uintptr_t alignment(int32_t n) const
    {
        uintptr_t v = reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b);
        if (n > 1) v |= (uintptr_t)stride_a | (uintptr_t)stride_b;
        return v;
    }
};

// n, layout and depth.  depth_lo .. depth_hi is what the entry takes (8 .. 8: the _u8 converters, 9 .. 16: the _u16 converters, which
// refuse rgb24 before they look at the layout any further; 8 .. 16: the sums)
inline int frames_check_format(const char *who, int32_t n, int32_t n_max, int32_t layout, int32_t depth, int32_t depth_lo, int32_t depth_hi)
{
    GSVC_REQUIRE(n >= 1 && n <= n_max, "%s: n must be 1 .. %d (got %d)", who, (int)n_max, (int)n);
    GSVC_REQUIRE(depth_lo <= 8 || layout != GSVC_FRAMES_RGB24, "%s: rgb24 frames are 8-bit only", who);
    GSVC_REQUIRE(layout == GSVC_FRAMES_RGB24 || layout == GSVC_FRAMES_YUV444P || layout == GSVC_FRAMES_YUV420P, "%s: unknown layout %d", who,
                 (int)layout);
    GSVC_REQUIRE(depth >= depth_lo && depth <= depth_hi, "%s: depth must be %d .. %d (got %d)", who, (int)depth_lo, (int)depth_hi, (int)depth);
    GSVC_REQUIRE(layout != GSVC_FRAMES_RGB24 || depth == 8, "%s: rgb24 frames are 8-bit only", who);
    return GSVC_OK;
}

inline int frames_check_colour(const char *who, int32_t matrix, int32_t range)
{
    GSVC_REQUIRE(matrix == GSVC_FRAMES_BT709 || matrix == GSVC_FRAMES_BT601, "%s: unknown matrix %d", who, (int)matrix);
    GSVC_REQUIRE(range == GSVC_FRAMES_LIMITED || range == GSVC_FRAMES_FULL, "%s: unknown range %d", who, (int)range);
    return GSVC_OK;
}

inline int frames_check_size(const char *who, int32_t H, int32_t W, int32_t layout)
{
    GSVC_REQUIRE(H >= 1 && W >= 1 && H <= 32768 && W <= 32768, "%s: image size must be 1 .. 32768 (got %d x %d)", who, (int)H, (int)W);
    GSVC_REQUIRE(layout != GSVC_FRAMES_YUV420P || (H % 2 == 0 && W % 2 == 0), "%s: yuv420p needs even H and W (got %d x %d)", who, (int)H,
                 (int)W);
    return GSVC_OK;
}

inline int frames_check_strides(const char *who, const FrameBufs &f, int64_t bytes)
{
    char s[48];
    f.strides_text(s);
    GSVC_REQUIRE(f.stride_a >= bytes && (!f.b || f.stride_b >= bytes), "%s: %s %s is shorter than a frame (%lld bytes)", who, f.stride_name, s,
                 (long long)bytes);
    return GSVC_OK;
}

// deep frames are 16-bit words: even bases and strides
inline int frames_check_even(const char *who, const FrameBufs &f)
{
    char s[48];
    f.strides_text(s);
    GSVC_REQUIRE(((reinterpret_cast<uintptr_t>(f.a) | reinterpret_cast<uintptr_t>(f.b)) & 1) == 0, "%s: %s frame base is not 2-byte aligned", who,
                 f.b ? "a" : "the");
    GSVC_REQUIRE(((f.stride_a | (f.b ? f.stride_b : 0)) & 1) == 0, "%s: %s %s is not a multiple of 2", who, f.stride_name, s);
    return GSVC_OK;
}

#define GSVC_FRAMES_TRY(call)           \
    do {                                \
        const int rc_ = (call);         \
        if (rc_ != GSVC_OK) return rc_; \
    } while (0)

// ---- colour: Kr, Kb in double; each direction derives its floats from them ---------------------------------------------------------
struct FrameMatrix {
    double Kr, Kb;
};
inline FrameMatrix frames_matrix(int32_t matrix)
{
    return matrix == GSVC_FRAMES_BT709 ? FrameMatrix{0.2126, 0.0722} : FrameMatrix{0.299, 0.114};
}

// code = off + scale * value at a depth of d bits.  Limited range: the 8-bit constants times 2^(d - 8), so that the value before
// rounding is exactly 2^(d - 8) times the 8-bit one; full range: 0 .. 2^d - 1 with the chroma zero at 2^(d - 1).  d = 8 gives 219, 16,
// 224, 128 and 255.
struct FrameRange {
    float y_scale, y_off, c_scale, c_off;
    float top;          // the largest code, 2^d - 1
};
inline FrameRange frames_range(int32_t range, int32_t depth)
{
    const float up = (float)(1 << (depth - 8)), top = (float)((1 << depth) - 1);
    const bool limited = range == GSVC_FRAMES_LIMITED;
    return FrameRange{limited ? 219.f * up : top, limited ? 16.f * up : 0.f, limited ? 224.f * up : top, 128.f * up, top};
}

// ---- the image pointers of a batch: img[k] = images_host[k] (k >= n: image 0 again, never addressed), each 4-byte aligned; their bits
//      are added to `align` for the wide-path decision.  P = const float * (output) or float * (input). ------------------------------
template <typename P>
inline int frames_gather_images(const char *who, P const *images_host, int32_t n, P (&img)[GSVC_FRAMES_MAX_BATCH], uintptr_t &align)
{
    for (int k = 0; k < GSVC_FRAMES_MAX_BATCH; k++) {
        img[k] = images_host[k < n ? k : 0];
        GSVC_REQUIRE(img[k], "%s: NULL image pointer", who);
        GSVC_REQUIRE((reinterpret_cast<uintptr_t>(img[k]) & 3) == 0, "%s: image %d is not 4-byte aligned", who, k);
        align |= reinterpret_cast<uintptr_t>(img[k]);
    }
    return GSVC_OK;
}

// ============================================================================================================================
// device: samples
// ============================================================================================================================
__device__ __forceinline__ float clamp01(float x)
{
    const float c = x > 0.f ? x : 0.f;      // NaN, -inf -> 0
    return c < 1.f ? c : 1.f;               // +inf -> 1
}

// sample k of an array of loaded 32-bit words; BPS = bytes per sample
template <int BPS>
__device__ __forceinline__ uint32_t code_of(const uint32_t *w, int k)
{
    return BPS == 1 ? (w[k >> 2] >> (8 * (k & 3))) & 255u : (w[k >> 1] >> (16 * (k & 1))) & 65535u;
}

// sample s of a frame in memory
template <int BPS>
__device__ __forceinline__ uint32_t code_at(const uint8_t *p, long long s)
{
    return BPS == 1 ? (uint32_t)p[s] : (uint32_t)reinterpret_cast<const uint16_t *>(p)[s];
}

// BYTES (4, 8 or a multiple of 16) from / to an address aligned to min(BYTES, 16), as one access per 16 bytes
template <int BYTES>
__device__ __forceinline__ void load_words(const void *src, uint32_t *w)
{
    if constexpr (BYTES == 4) {
        w[0] = *reinterpret_cast<const uint32_t *>(src);
    } else if constexpr (BYTES == 8) {
        const uint2 t = *reinterpret_cast<const uint2 *>(src);
        w[0] = t.x; w[1] = t.y;
    } else {
        static_assert(BYTES % 16 == 0, "load_words: 4, 8 or a multiple of 16 bytes");
        const uint4 t = *reinterpret_cast<const uint4 *>(src);
        w[0] = t.x; w[1] = t.y; w[2] = t.z; w[3] = t.w;
        if constexpr (BYTES > 16) load_words<BYTES - 16>(reinterpret_cast<const uint4 *>(src) + 1, w + 4);
    }
}

template <int BYTES>
__device__ __forceinline__ void store_words(void *dst, const uint32_t *w)
{
    if constexpr (BYTES == 4) {
        *reinterpret_cast<uint32_t *>(dst) = w[0];
    } else if constexpr (BYTES == 8) {
        *reinterpret_cast<uint2 *>(dst) = make_uint2(w[0], w[1]);
    } else {
        static_assert(BYTES % 16 == 0, "store_words: 4, 8 or a multiple of 16 bytes");
#pragma unroll
        for (int i = 0; i < BYTES / 16; i++) reinterpret_cast<uint4 *>(dst)[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
    }
}

// ============================================================================================================================
// device: the per-plane sums (k_frames_sse, k_picture_hash)
// ============================================================================================================================
constexpr int SUMS_PER_LANE = 4;         // units (wide) or samples (edge) per lane, 256 apart

// a frame as ONE flat run of samples: a plane is a range of sample indices, plane(f) = (f >= p0) + (f >= p1) (rgb24: the channel is
// the index mod 3).  Both kernels walk it alike:
//   wide path   a lane takes one unit of 16 bytes (rgb24: 48 bytes = three vectors = 16 pixels, so that sample j of a unit is channel
//               j mod 3 of pixel j / 3) and SUMS_PER_LANE units 256 apart.  A vector may straddle a plane boundary (H W = 60: U starts
//               at sample 60): its samples are then classified one by one.  The samples behind the last whole unit of the frame are
//               taken one per lane by the units that follow.
//   edge path   one sample per lane and SUMS_PER_LANE samples 256 apart, at any alignment (deep formats: even).
struct SampleRun {
    long long samples;                 // of one frame
    long long p0, p1;                  // first sample of the second / third plane (planar layouts)
};

__device__ __forceinline__ void add_to_plane(unsigned long long acc[3], int plane, unsigned long long v)
{
    acc[0] += plane == 0 ? v : 0ull;
    acc[1] += plane == 1 ? v : 0ull;
    acc[2] += plane == 2 ? v : 0ull;
}

// the three 64-bit sums of a 256-thread workgroup: a wave reduces them with shuffles, the workgroup through LDS, and one thread per
// plane issues one 64-bit integer atomic (none for a sum of zero).  Integer addition is associative: the same bits in every run and
// for every launch shape.
__device__ __forceinline__ void add_block_sums(unsigned long long acc[3], unsigned long long *out)
{
    __shared__ unsigned long long red[4][3];
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
        if (v) atomicAdd(&out[threadIdx.x], v);
    }
}

// ---- host part of the sums: checks, the zeroed out[n, out_per_frame] of out_elem-byte integers (uint64 [n, 3] for the two 64-bit
//      sums, uint32 [n, 768] for the histograms), the run of samples and the launch shape -------------------------------------------
struct FrameSums {
    SampleRun run;
    int variant;          // 0 rgb24, 1 8-bit planar, 2 deep planar: the row of GSVC_FRAME_SUMS_KERNELS
    bool wide;
    int64_t units;        // what the lanes share out: whole units, then the samples behind them (wide), or samples (edge)
    dim3 grid;            // SUMS_PER_LANE of them per lane (the histogram takes more per workgroup and sets its own)
};

inline int frames_sums_setup(const char *who, const FrameBufs &bufs, int32_t n, int32_t H, int32_t W, int32_t layout, int32_t depth,
                             void *out, hipStream_t s, FrameSums &fs, int out_elem = 8, int out_per_frame = 3)
{
    GSVC_FRAMES_TRY(frames_check_format(who, n, 65535, layout, depth, 8, 16));
    GSVC_FRAMES_TRY(frames_check_size(who, H, W, layout));
    const int64_t bytes = gsvc_frames_bytes(H, W, layout, depth);
    GSVC_FRAMES_TRY(frames_check_strides(who, bufs, bytes));
    const bool deep = depth > 8, rgb = layout == GSVC_FRAMES_RGB24;
    if (deep) GSVC_FRAMES_TRY(frames_check_even(who, bufs));
    GSVC_REQUIRE((reinterpret_cast<uintptr_t>(out) & (uintptr_t)(out_elem - 1)) == 0, "%s: out is not %d-byte aligned", who, out_elem);
    GSVC_REQUIRE(out_elem % 4 == 0, "%s: sums of %d bytes", who, out_elem);
    if (zero_words_async(out, (size_t)n * (size_t)out_per_frame * (size_t)out_elem, s) != hipSuccess) {
        set_error("%s: zeroing failed", who);
        return GSVC_E_LAUNCH;
    }
    const int64_t px = (int64_t)H * W, chroma = layout == GSVC_FRAMES_YUV420P ? px / 4 : px;
    fs.run.samples = bytes / (deep ? 2 : 1);
    fs.run.p0 = px;
    fs.run.p1 = px + chroma;
    fs.variant = rgb ? 0 : (deep ? 2 : 1);
    fs.wide = (bufs.alignment(n) & 15) == 0;
    int64_t units = fs.run.samples;
    if (fs.wide) {
        const int64_t spu = rgb ? 48 : (deep ? 8 : 16);
        units = fs.run.samples / spu + fs.run.samples % spu;          // whole units, then the samples behind them one by one
    }
    fs.units = units;
    const int64_t per_block = 256 * SUMS_PER_LANE;
    fs.grid = dim3((unsigned)((units + per_block - 1) / per_block), (unsigned)n);
    return GSVC_OK;
}

// the instantiations of a sum kernel K<BPS, RGB, WIDE>, indexed [FrameSums::variant][FrameSums::wide]
#define GSVC_FRAME_SUMS_KERNELS(K) \
    {{K<1, true, false>, K<1, true, true>}, {K<1, false, false>, K<1, false, true>}, {K<2, false, false>, K<2, false, true>}}

}  // namespace gsvc
