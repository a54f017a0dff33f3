// gsvc_amd/csrc/frames_out.hip — decoder output: float [3, H, W] images -> 8-bit RGB24 / YUV 4:4:4 / YUV 4:2:0 frames and 9 .. 16-bit
// planar YUV frames (little-endian 16-bit words), gfx950.
//
// The render loop leaves one float32 image per frame in device memory (24.9 MB at 1080p); what a player, a file or a quality
// tool takes is 8 bits per sample (6.2 MB as RGB24, 3.1 MB as 4:2:0).  The reference does it on the host (utils/report_utils.py:
// 439-445: clamp, ToPILImage); here one launch converts the up to 16 images of a render batch — a pure stream, 12 bytes read
// and 1.5 - 6 bytes written per pixel, no LDS, no reuse.
//
// One kernel body per layout; the sample type T (uint8_t, uint16_t) and the lane's pixels per row PX are template arguments:
//   wide path   (W a multiple of PX, every image base, the output base and its stride 16-byte aligned): a lane reads 16 bytes per
//               access and never stores less than 4:
//                   rgb24       16 pixels x 1 row  -> 48 B as 3 x 16 B                                (8-bit only, interleaved)
//                   yuv444p     <uint8_t, 16>  16 pixels x 1 row  -> 16 B to each of the three planes
//                               <uint16_t, 4>   4 pixels x 1 row  ->  8 B to each of the three planes
//                   yuv420p     <uint8_t, 8>    8 pixels x 2 rows -> 2 x 8 B of Y, 4 B of U, 4 B of V
//                               <uint16_t, 4>   4 pixels x 2 rows -> 2 x 8 B of Y, 4 B of U, 4 B of V
//               The deep lane owns FOUR pixels so that lane i of a wave loads its float4 at base + 16 i: one wave instruction reads
//               1 KiB of one row contiguously, the 12 of 14 - 18 bytes per pixel that are this stage's traffic.
//   edge path   (any W, any 4-byte-aligned image base, any output alignment a sample allows): one pixel (4:2:0: one 2x2 block) per
//               lane, one store per sample.
// Both paths and both sample types evaluate the same expressions in the same order, every fused multiply-add spelled out (no sum is
// left for the compiler to contract one way here and another way there), so which path a frame takes does not change its bytes.
// The batch index is blockIdx.y; the image pointers travel by value in the kernel arguments.
// The profile names of the deep instantiations keep their 16: k_frames_yuv444p16, k_frames_yuv420p16.
// The argument checks, Kr / Kb and the range constants are those of frames_common.h; one host body serves both entries.
#include "frames_common.h"

namespace gsvc {

struct FramesArgs {
    const float *img[GSVC_FRAMES_MAX_BATCH];
    uint8_t *out;
    long long out_stride;
    int H, W;
    float kr, kg, kb;           // luma weights
    float icb, icr;             // 1 / (2 (1 - Kb)), 1 / (2 (1 - Kr))
    float y_scale, y_off;       // Y code = y_off + y_scale Y      (rgb24: 255, 0)
    float c_scale, c_off;       // C code = c_off + c_scale C
    float rnd;                  // 0 (trunc) or 0.5 (nearest)
    float top;                  // the largest code, 2^d - 1
};

__device__ __forceinline__ uint32_t quant(float v, float rnd, float top)
{
    v = v > 0.f ? v : 0.f;
    v = v < top ? v : top;
    return (uint32_t)(v + rnd);
}

__device__ __forceinline__ void ycc(const FramesArgs &a, float r, float g, float b, float &y, float &cb, float &cr)
{
    y = fmaf(a.kr, r, fmaf(a.kg, g, a.kb * b));
    cb = (b - y) * a.icb;
    cr = (r - y) * a.icr;
}

// the largest code of a sample type: a.top = 2^d - 1, which at 8 bits is stated as the constant it is (the clamp to a constant range is
// one v_med3_f32; to a range in a register it is three instructions, 1 % of the 8-bit 4:4:4 kernel's time)
template <typename T>
__device__ __forceinline__ float top_of(const FramesArgs &a) { return sizeof(T) == 1 ? 255.f : a.top; }

template <typename T>
__device__ __forceinline__ uint32_t luma(const FramesArgs &a, float y) { return quant(fmaf(a.y_scale, y, a.y_off), a.rnd, top_of<T>(a)); }
template <typename T>
__device__ __forceinline__ uint32_t chroma(const FramesArgs &a, float c) { return quant(fmaf(a.c_scale, c, a.c_off), a.rnd, top_of<T>(a)); }
__device__ __forceinline__ float mean4(const float c[2][2]) { return ((c[0][0] + c[0][1]) + (c[1][0] + c[1][1])) * 0.25f; }

__device__ __forceinline__ void load4(const float *p, float *v)
{
    const float4 t = *reinterpret_cast<const float4 *>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}

// code p of a lane's run of samples of type T into its (zeroed) 32-bit words
template <typename T>
__device__ __forceinline__ void put_code(uint32_t *w, int p, uint32_t code)
{
    constexpr int PER = 4 / (int)sizeof(T);
    w[p / PER] |= code << (8 * (int)sizeof(T) * (p % PER));
}

// ---- rgb24 -------------------------------------------------------------------------------------------------------------
template <bool WIDE>
__global__ void __launch_bounds__(256) k_frames_rgb24(FramesArgs a)
{
    const float *img = a.img[blockIdx.y];
    uint8_t *out = a.out + (size_t)blockIdx.y * (size_t)a.out_stride;
    const size_t plane = (size_t)a.H * (size_t)a.W;
    const int unit = blockIdx.x * 256 + threadIdx.x;
    if (WIDE) {
        if ((size_t)unit >= plane / 16) return;
        const size_t at = (size_t)unit * 16;          // (W is a multiple of 16: units are consecutive over the rows)
        float c[3][16];
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
#pragma unroll
            for (int q = 0; q < 4; q++) load4(img + ch * plane + at + 4 * q, &c[ch][4 * q]);
        uint32_t w[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int p = 0; p < 16; p++)
#pragma unroll
            for (int ch = 0; ch < 3; ch++) put_code<uint8_t>(w, 3 * p + ch, quant(255.f * clamp01(c[ch][p]), a.rnd, 255.f));
        store_words<48>(out + 3 * at, w);
    } else {
        if ((size_t)unit >= plane) return;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) out[3 * (size_t)unit + ch] = (uint8_t)quant(255.f * clamp01(img[ch * plane + unit]), a.rnd, 255.f);
    }
}

// ---- yuv444p -----------------------------------------------------------------------------------------------------------
template <typename T, int PX, bool WIDE>
__global__ void __launch_bounds__(256) k_frames_yuv444p(FramesArgs a)
{
    const float *img = a.img[blockIdx.y];
    T *out = reinterpret_cast<T *>(a.out + (size_t)blockIdx.y * (size_t)a.out_stride);
    const size_t plane = (size_t)a.H * (size_t)a.W;
    const int unit = blockIdx.x * 256 + threadIdx.x;
    if (WIDE) {
        if ((size_t)unit >= plane / PX) return;
        const size_t at = (size_t)unit * PX;          // (W is a multiple of PX: units are consecutive over the rows)
        constexpr int NW = PX * (int)sizeof(T) / 4;
        float c[3][PX];
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
#pragma unroll
            for (int q = 0; q < PX / 4; q++) load4(img + ch * plane + at + 4 * q, &c[ch][4 * q]);
        uint32_t wy[NW] = {}, wu[NW] = {}, wv[NW] = {};
#pragma unroll
        for (int p = 0; p < PX; p++) {
            float Y, cb, cr;
            ycc(a, clamp01(c[0][p]), clamp01(c[1][p]), clamp01(c[2][p]), Y, cb, cr);
            put_code<T>(wy, p, luma<T>(a, Y));
            put_code<T>(wu, p, chroma<T>(a, cb));
            put_code<T>(wv, p, chroma<T>(a, cr));
        }
        store_words<4 * NW>(out + at, wy);
        store_words<4 * NW>(out + plane + at, wu);
        store_words<4 * NW>(out + 2 * plane + at, wv);
    } else {
        if ((size_t)unit >= plane) return;
        float Y, cb, cr;
        ycc(a, clamp01(img[unit]), clamp01(img[plane + unit]), clamp01(img[2 * plane + unit]), Y, cb, cr);
        out[unit] = (T)luma<T>(a, Y);
        out[plane + unit] = (T)chroma<T>(a, cb);
        out[2 * plane + unit] = (T)chroma<T>(a, cr);
    }
}

// ---- yuv420p: a lane owns PX pixels of two rows = PX / 2 chroma samples; chroma = mean of the 2x2 block's float Cb / Cr,
//      ((c00 + c01) + (c10 + c11)) * 0.25 on both paths ---------------------------------------------------------------------------
template <typename T, int PX, bool WIDE>
__global__ void __launch_bounds__(256) k_frames_yuv420p(FramesArgs a)
{
    const float *img = a.img[blockIdx.y];
    T *out = reinterpret_cast<T *>(a.out + (size_t)blockIdx.y * (size_t)a.out_stride);
    const size_t plane = (size_t)a.H * (size_t)a.W;
    const int W2 = a.W >> 1, H2 = a.H >> 1;
    T *out_u = out + plane, *out_v = out_u + (size_t)H2 * W2;
    const int unit = blockIdx.x * 256 + threadIdx.x;
    if (WIDE) {
        const int per_row = a.W / PX;
        if (unit >= per_row * H2) return;
        const int yb = unit / per_row, x = (unit - yb * per_row) * PX;
        const size_t at = (size_t)(2 * yb) * a.W + x;
        constexpr int NW = PX * (int)sizeof(T) / 4, NC = PX / 2 * (int)sizeof(T) / 4;
        float c[3][2][PX];
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
#pragma unroll
            for (int r = 0; r < 2; r++)
#pragma unroll
                for (int q = 0; q < PX / 4; q++) load4(img + ch * plane + at + (size_t)r * a.W + 4 * q, &c[ch][r][4 * q]);
        uint32_t wy[2][NW] = {}, wu[NC] = {}, wv[NC] = {};
#pragma unroll
        for (int p = 0; p < PX / 2; p++) {
            float cb[2][2], cr[2][2];
#pragma unroll
            for (int r = 0; r < 2; r++)
#pragma unroll
                for (int s = 0; s < 2; s++) {
                    const int px = 2 * p + s;
                    float Y;
                    ycc(a, clamp01(c[0][r][px]), clamp01(c[1][r][px]), clamp01(c[2][r][px]), Y, cb[r][s], cr[r][s]);
                    put_code<T>(wy[r], px, luma<T>(a, Y));
                }
            put_code<T>(wu, p, chroma<T>(a, mean4(cb)));
            put_code<T>(wv, p, chroma<T>(a, mean4(cr)));
        }
        store_words<4 * NW>(out + at, wy[0]);
        store_words<4 * NW>(out + at + a.W, wy[1]);
        const size_t cat = (size_t)yb * W2 + (x >> 1);
        store_words<4 * NC>(out_u + cat, wu);
        store_words<4 * NC>(out_v + cat, wv);
    } else {
        if (unit >= W2 * H2) return;
        const int yb = unit / W2, xb = unit - yb * W2;
        const size_t at = (size_t)(2 * yb) * a.W + 2 * xb;
        float cb[2][2], cr[2][2];
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int s = 0; s < 2; s++) {
                const size_t i = at + (size_t)r * a.W + s;
                float Y;
                ycc(a, clamp01(img[i]), clamp01(img[plane + i]), clamp01(img[2 * plane + i]), Y, cb[r][s], cr[r][s]);
                out[i] = (T)luma<T>(a, Y);
            }
        out_u[unit] = (T)chroma<T>(a, mean4(cb));
        out_v[unit] = (T)chroma<T>(a, mean4(cr));
    }
}

}  // namespace gsvc

using namespace gsvc;

extern "C" int64_t gsvc_frames_u8_bytes(int32_t H, int32_t W, int32_t layout)
{
    if (H < 1 || W < 1 || H > 32768 || W > 32768) return -1;
    const int64_t px = (int64_t)H * W;
    switch (layout) {
    case GSVC_FRAMES_RGB24:
    case GSVC_FRAMES_YUV444P: return 3 * px;
    case GSVC_FRAMES_YUV420P: return (H % 2 || W % 2) ? -1 : px * 3 / 2;
    default: return -1;
    }
}

extern "C" int64_t gsvc_frames_bytes(int32_t H, int32_t W, int32_t layout, int32_t depth)
{
    if (depth == 8) return gsvc_frames_u8_bytes(H, W, layout);
    if (depth < 9 || depth > 16 || layout == GSVC_FRAMES_RGB24) return -1;
    const int64_t bytes = gsvc_frames_u8_bytes(H, W, layout);
    return bytes < 0 ? bytes : 2 * bytes;
}

// both entries; who = the entry's name, deep = the _u16 one (depth 9 .. 16; the _u8 one passes depth 8)
static int frames_to(const char *who, bool deep, const float *const *images_host, int32_t n, int32_t H, int32_t W, int32_t layout,
                     int32_t matrix, int32_t range, int32_t rounding, int32_t depth, uint8_t *out, int64_t out_stride, void *stream)
{
    GSVC_REQUIRE(images_host && out, "%s: NULL pointer", who);
    GSVC_FRAMES_TRY(frames_check_format(who, n, GSVC_FRAMES_MAX_BATCH, layout, depth, deep ? 9 : 8, deep ? 16 : 8));
    GSVC_FRAMES_TRY(frames_check_colour(who, matrix, range));
    GSVC_REQUIRE(rounding == GSVC_FRAMES_TRUNC || rounding == GSVC_FRAMES_NEAREST, "%s: unknown rounding %d", who, (int)rounding);
    GSVC_FRAMES_TRY(frames_check_size(who, H, W, layout));
    const FrameBufs bufs = {"out_stride", out, out_stride, nullptr, 0};
    if (deep) GSVC_FRAMES_TRY(frames_check_even(who, bufs));
    GSVC_FRAMES_TRY(frames_check_strides(who, bufs, gsvc_frames_bytes(H, W, layout, depth)));
    FramesArgs a;
    uintptr_t align = bufs.alignment(n);
    GSVC_FRAMES_TRY(frames_gather_images(who, images_host, n, a.img, align));
    a.out = out;
    a.out_stride = out_stride;
    a.H = H;
    a.W = W;
    const FrameMatrix m = frames_matrix(matrix);
    a.kr = (float)m.Kr;
    a.kg = (float)(1.0 - m.Kr - m.Kb);
    a.kb = (float)m.Kb;
    a.icb = (float)(1.0 / (2.0 * (1.0 - m.Kb)));
    a.icr = (float)(1.0 / (2.0 * (1.0 - m.Kr)));
    const FrameRange r = frames_range(range, depth);
    a.y_scale = r.y_scale;
    a.y_off = r.y_off;
    a.c_scale = r.c_scale;
    a.c_off = r.c_off;
    a.top = r.top;
    a.rnd = rounding == GSVC_FRAMES_NEAREST ? 0.5f : 0.f;
    // the wide path: whole lanes of PX pixels per row and 16-byte-aligned bases.  W % 4 == 0 keeps every float row 16-byte aligned; the
    // code rows and planes of a lane's PX samples (4:2:0 chroma: PX / 2) keep the alignment of the lane's store
    const bool yuv420 = layout == GSVC_FRAMES_YUV420P;
    const int lane_px = deep ? 4 : (yuv420 ? 8 : 16);
    const bool wide = W % lane_px == 0 && (align & 15) == 0;
    int64_t units;
    if (yuv420) units = (int64_t)(W / (wide ? lane_px : 2)) * (H / 2);
    else units = (int64_t)W * H / (wide ? lane_px : 1);
    using Kernel = void (*)(FramesArgs);
    static const Kernel rgb24[2] = {k_frames_rgb24<false>, k_frames_rgb24<true>};          // [wide]
    static const Kernel yuv444p[2][2] = {{k_frames_yuv444p<uint8_t, 16, false>, k_frames_yuv444p<uint8_t, 16, true>},
                                         {k_frames_yuv444p<uint16_t, 4, false>, k_frames_yuv444p<uint16_t, 4, true>}};      // [deep][wide]
    static const Kernel yuv420p[2][2] = {{k_frames_yuv420p<uint8_t, 8, false>, k_frames_yuv420p<uint8_t, 8, true>},
                                         {k_frames_yuv420p<uint16_t, 4, false>, k_frames_yuv420p<uint16_t, 4, true>}};
    const Kernel kernel = layout == GSVC_FRAMES_RGB24 ? rgb24[wide] : (yuv420 ? yuv420p[deep][wide] : yuv444p[deep][wide]);
    const char *const name = layout == GSVC_FRAMES_RGB24 ? "k_frames_rgb24"
                             : (yuv420 ? (deep ? "k_frames_yuv420p16" : "k_frames_yuv420p") : (deep ? "k_frames_yuv444p16" : "k_frames_yuv444p"));
    hipStream_t s = (hipStream_t)stream;
    ProfScope _p(name, s);
    hipLaunchKernelGGL(kernel, dim3((unsigned)((units + 255) / 256), (unsigned)n), dim3(256), 0, s, a);
    return check_launch(who);
}

extern "C" int gsvc_frames_to_u8(const float *const *images_host, int32_t n, int32_t H, int32_t W, int32_t layout, int32_t matrix,
                                 int32_t range, int32_t rounding, uint8_t *out, int64_t out_stride, void *stream)
{
    return frames_to("frames_to_u8", false, images_host, n, H, W, layout, matrix, range, rounding, 8, out, out_stride, stream);
}

extern "C" int gsvc_frames_to_u16(const float *const *images_host, int32_t n, int32_t H, int32_t W, int32_t layout, int32_t matrix,
                                  int32_t range, int32_t rounding, int32_t depth, uint8_t *out, int64_t out_stride, void *stream)
{
    return frames_to("frames_to_u16", true, images_host, n, H, W, layout, matrix, range, rounding, depth, out, out_stride, stream);
}
