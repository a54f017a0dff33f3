// gsvc_amd/csrc/frames_out.hip — decoder output: float [3, H, W] images -> 8-bit RGB24 / YUV 4:4:4 / YUV 4:2:0 frames and 9 .. 16-bit
// planar YUV frames (little-endian 16-bit words), gfx950.
//
// The render loop leaves one float32 image per frame in device memory (24.9 MB at 1080p); what a player, a file or a quality
// tool takes is 8 bits per sample (6.2 MB as RGB24, 3.1 MB as 4:2:0).  The reference does it on the host (utils/report_utils.py:
// 439-445: clamp, ToPILImage); here one launch converts the up to 16 images of a render batch — a pure stream, 12 bytes read
// and 1.5 - 3 bytes written per pixel, no LDS, no reuse:
//   fast path   (W a multiple of the lane's pixel count, every base 16-byte aligned): a lane reads 16 bytes per access and
//               never stores less than 4 bytes:  rgb24    16 pixels x 1 row  -> 48 B as 3 x 16 B
//                                                yuv444p  16 pixels x 1 row  -> 16 B to each of the three planes
//                                                yuv420p   8 pixels x 2 rows -> 2 x 8 B of Y, 4 B of U, 4 B of V
//   edge path   (any W, any 4-byte-aligned image base, any output alignment): one pixel (4:2:0: one 2x2 block) per lane, byte stores.
// Both paths evaluate the same expressions in the same order, every fused multiply-add spelled out (no sum is left for the
// compiler to contract one way here and another way there), so which path a frame takes does not change its bytes.
// The batch index is blockIdx.y; the image pointers travel by value in the kernel arguments.
//
// Deep frames (gsvc_frames_to_u16, the k_frames_*16 kernels below) share the per-pixel functions and differ in the lane shape: a lane
// owns FOUR pixels of a row (4:2:0: of two rows), so that lane i of a wave loads its float4 at base + 16 i — one wave instruction reads
// 1 KiB of one row contiguously, the 12 of 14 - 18 bytes per pixel that are this stage's traffic — and stores 8 bytes of 16-bit codes
// at base + 8 i (4:2:0 chroma: 4 bytes at base + 4 i).
//   wide path   (W a multiple of 4, every image base, the output base and its stride 16-byte aligned)
//   edge path   (any W, any 4-byte-aligned image base, any 2-byte-aligned output): one pixel (4:2:0: one 2x2 block) per lane, 2-byte stores.
#include "common.h"

namespace gsvc {

struct FramesArgs {
    const float *img[GSVC_FRAMES_MAX_BATCH];
    uint8_t *out;
    long long out_stride;
    int H, W;
    float kr, kg, kb;           // luma weights
    float icb, icr;             // 1 / (2 (1 - Kb)), 1 / (2 (1 - Kr))
    float y_scale, y_off;       // Y8 = y_off + y_scale Y      (rgb24: 255, 0)
    float c_scale, c_off;       // C8 = c_off + c_scale C
    float rnd;                  // 0 (trunc) or 0.5 (nearest)
    float top;                  // the largest code, 2^d - 1 (read by the deep kernels only)
};

__device__ __forceinline__ float clamp01(float x)
{
    const float c = x > 0.f ? x : 0.f;      // NaN, -inf -> 0
    return c < 1.f ? c : 1.f;               // +inf -> 1
}

__device__ __forceinline__ uint32_t quant8(float v, float rnd)
{
    v = v > 0.f ? v : 0.f;
    v = v < 255.f ? v : 255.f;
    return (uint32_t)(v + rnd);
}

__device__ __forceinline__ void ycc(const FramesArgs &a, float r, float g, float b, float &y, float &cb, float &cr)
{
    y = fmaf(a.kr, r, fmaf(a.kg, g, a.kb * b));
    cb = (b - y) * a.icb;
    cr = (r - y) * a.icr;
}

__device__ __forceinline__ uint32_t luma8(const FramesArgs &a, float y) { return quant8(fmaf(a.y_scale, y, a.y_off), a.rnd); }
__device__ __forceinline__ uint32_t chroma8(const FramesArgs &a, float c) { return quant8(fmaf(a.c_scale, c, a.c_off), a.rnd); }

// the deep forms: the same expressions, clamped to [0, 2^d - 1]
__device__ __forceinline__ uint32_t quant16(float v, float rnd, float top)
{
    v = v > 0.f ? v : 0.f;
    v = v < top ? v : top;
    return (uint32_t)(v + rnd);
}
__device__ __forceinline__ uint32_t luma16(const FramesArgs &a, float y) { return quant16(fmaf(a.y_scale, y, a.y_off), a.rnd, a.top); }
__device__ __forceinline__ uint32_t chroma16(const FramesArgs &a, float c) { return quant16(fmaf(a.c_scale, c, a.c_off), a.rnd, a.top); }

__device__ __forceinline__ void load4(const float *p, float *v)
{
    const float4 t = *reinterpret_cast<const float4 *>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}

// ---- rgb24 -------------------------------------------------------------------------------------------------------------
template <bool FAST>
__global__ void __launch_bounds__(256) k_frames_rgb24(FramesArgs a)
{
    const float *img = a.img[blockIdx.y];
    uint8_t *out = a.out + (size_t)blockIdx.y * (size_t)a.out_stride;
    const size_t plane = (size_t)a.H * (size_t)a.W;
    const int unit = blockIdx.x * 256 + threadIdx.x;
    if (FAST) {
        const int per_row = a.W >> 4;
        if (unit >= per_row * a.H) return;
        const int y = unit / per_row, x = (unit - y * per_row) << 4;
        const size_t at = (size_t)y * a.W + x;
        float c[3][16];
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
#pragma unroll
            for (int q = 0; q < 4; q++) load4(img + ch * plane + at + 4 * q, &c[ch][4 * q]);
        uint32_t w[12];
#pragma unroll
        for (int k = 0; k < 12; k++) w[k] = 0;
#pragma unroll
        for (int p = 0; p < 16; p++)
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                const int j = 3 * p + ch;
                w[j >> 2] |= quant8(255.f * clamp01(c[ch][p]), a.rnd) << (8 * (j & 3));
            }
        uint4 *dst = reinterpret_cast<uint4 *>(out + 3 * at);
        dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
        dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
        dst[2] = make_uint4(w[8], w[9], w[10], w[11]);
    } else {
        if ((size_t)unit >= plane) return;
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
            out[3 * (size_t)unit + ch] = (uint8_t)quant8(255.f * clamp01(img[ch * plane + unit]), a.rnd);
    }
}

// ---- yuv444p -----------------------------------------------------------------------------------------------------------
template <bool FAST>
__global__ void __launch_bounds__(256) k_frames_yuv444p(FramesArgs a)
{
    const float *img = a.img[blockIdx.y];
    uint8_t *out = a.out + (size_t)blockIdx.y * (size_t)a.out_stride;
    const size_t plane = (size_t)a.H * (size_t)a.W;
    const int unit = blockIdx.x * 256 + threadIdx.x;
    if (FAST) {
        const int per_row = a.W >> 4;
        if (unit >= per_row * a.H) return;
        const int y = unit / per_row, x = (unit - y * per_row) << 4;
        const size_t at = (size_t)y * a.W + x;
        float c[3][16];
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
#pragma unroll
            for (int q = 0; q < 4; q++) load4(img + ch * plane + at + 4 * q, &c[ch][4 * q]);
        uint32_t wy[4] = {0, 0, 0, 0}, wu[4] = {0, 0, 0, 0}, wv[4] = {0, 0, 0, 0};
#pragma unroll
        for (int p = 0; p < 16; p++) {
            float Y, cb, cr;
            ycc(a, clamp01(c[0][p]), clamp01(c[1][p]), clamp01(c[2][p]), Y, cb, cr);
            const int sh = 8 * (p & 3);
            wy[p >> 2] |= luma8(a, Y) << sh;
            wu[p >> 2] |= chroma8(a, cb) << sh;
            wv[p >> 2] |= chroma8(a, cr) << sh;
        }
        *reinterpret_cast<uint4 *>(out + at) = make_uint4(wy[0], wy[1], wy[2], wy[3]);
        *reinterpret_cast<uint4 *>(out + plane + at) = make_uint4(wu[0], wu[1], wu[2], wu[3]);
        *reinterpret_cast<uint4 *>(out + 2 * plane + at) = make_uint4(wv[0], wv[1], wv[2], wv[3]);
    } else {
        if ((size_t)unit >= plane) return;
        float Y, cb, cr;
        ycc(a, clamp01(img[unit]), clamp01(img[plane + unit]), clamp01(img[2 * plane + unit]), Y, cb, cr);
        out[unit] = (uint8_t)luma8(a, Y);
        out[plane + unit] = (uint8_t)chroma8(a, cb);
        out[2 * plane + unit] = (uint8_t)chroma8(a, cr);
    }
}

// ---- yuv420p: chroma = mean of the 2x2 block's float Cb / Cr, ((c00 + c01) + (c10 + c11)) * 0.25 on both paths ------------
template <bool FAST>
__global__ void __launch_bounds__(256) k_frames_yuv420p(FramesArgs a)
{
    const float *img = a.img[blockIdx.y];
    uint8_t *out = a.out + (size_t)blockIdx.y * (size_t)a.out_stride;
    const size_t plane = (size_t)a.H * (size_t)a.W;
    const int W2 = a.W >> 1, H2 = a.H >> 1;
    uint8_t *out_u = out + plane, *out_v = out_u + (size_t)H2 * W2;
    const int unit = blockIdx.x * 256 + threadIdx.x;
    if (FAST) {
        const int per_row = a.W >> 3;
        if (unit >= per_row * H2) return;
        const int yb = unit / per_row, x = (unit - yb * per_row) << 3;
        const size_t at = (size_t)(2 * yb) * a.W + x;
        float c[3][2][8];
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
#pragma unroll
            for (int r = 0; r < 2; r++)
#pragma unroll
                for (int q = 0; q < 2; q++) load4(img + ch * plane + at + (size_t)r * a.W + 4 * q, &c[ch][r][4 * q]);
        uint32_t wy[2][2] = {{0, 0}, {0, 0}}, wu = 0, wv = 0;
#pragma unroll
        for (int p = 0; p < 4; p++) {
            float cb[2][2], cr[2][2];
#pragma unroll
            for (int r = 0; r < 2; r++)
#pragma unroll
                for (int s = 0; s < 2; s++) {
                    const int px = 2 * p + s;
                    float Y;
                    ycc(a, clamp01(c[0][r][px]), clamp01(c[1][r][px]), clamp01(c[2][r][px]), Y, cb[r][s], cr[r][s]);
                    wy[r][px >> 2] |= luma8(a, Y) << (8 * (px & 3));
                }
            wu |= chroma8(a, ((cb[0][0] + cb[0][1]) + (cb[1][0] + cb[1][1])) * 0.25f) << (8 * p);
            wv |= chroma8(a, ((cr[0][0] + cr[0][1]) + (cr[1][0] + cr[1][1])) * 0.25f) << (8 * p);
        }
        *reinterpret_cast<uint2 *>(out + at) = make_uint2(wy[0][0], wy[0][1]);
        *reinterpret_cast<uint2 *>(out + at + a.W) = make_uint2(wy[1][0], wy[1][1]);
        const size_t cat = (size_t)yb * W2 + (x >> 1);
        *reinterpret_cast<uint32_t *>(out_u + cat) = wu;
        *reinterpret_cast<uint32_t *>(out_v + cat) = wv;
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
                out[i] = (uint8_t)luma8(a, Y);
            }
        out_u[unit] = (uint8_t)chroma8(a, ((cb[0][0] + cb[0][1]) + (cb[1][0] + cb[1][1])) * 0.25f);
        out_v[unit] = (uint8_t)chroma8(a, ((cr[0][0] + cr[0][1]) + (cr[1][0] + cr[1][1])) * 0.25f);
    }
}

// ---- deep yuv444p: 16-bit words, a lane owns 4 pixels of a row ---------------------------------------------------------------
template <bool WIDE>
__global__ void __launch_bounds__(256) k_frames_yuv444p16(FramesArgs a)
{
    const float *img = a.img[blockIdx.y];
    uint16_t *out = reinterpret_cast<uint16_t *>(a.out + (size_t)blockIdx.y * (size_t)a.out_stride);
    const size_t plane = (size_t)a.H * (size_t)a.W;
    const int unit = blockIdx.x * 256 + threadIdx.x;
    if (WIDE) {
        if ((size_t)unit >= (plane >> 2)) return;
        const size_t at = (size_t)unit << 2;          // (W is a multiple of 4: units are consecutive over the rows)
        float c[3][4];
#pragma unroll
        for (int ch = 0; ch < 3; ch++) load4(img + ch * plane + at, c[ch]);
        uint32_t wy[2] = {0, 0}, wu[2] = {0, 0}, wv[2] = {0, 0};
#pragma unroll
        for (int p = 0; p < 4; p++) {
            float Y, cb, cr;
            ycc(a, clamp01(c[0][p]), clamp01(c[1][p]), clamp01(c[2][p]), Y, cb, cr);
            const int sh = 16 * (p & 1);
            wy[p >> 1] |= luma16(a, Y) << sh;
            wu[p >> 1] |= chroma16(a, cb) << sh;
            wv[p >> 1] |= chroma16(a, cr) << sh;
        }
        *reinterpret_cast<uint2 *>(out + at) = make_uint2(wy[0], wy[1]);
        *reinterpret_cast<uint2 *>(out + plane + at) = make_uint2(wu[0], wu[1]);
        *reinterpret_cast<uint2 *>(out + 2 * plane + at) = make_uint2(wv[0], wv[1]);
    } else {
        if ((size_t)unit >= plane) return;
        float Y, cb, cr;
        ycc(a, clamp01(img[unit]), clamp01(img[plane + unit]), clamp01(img[2 * plane + unit]), Y, cb, cr);
        out[unit] = (uint16_t)luma16(a, Y);
        out[plane + unit] = (uint16_t)chroma16(a, cb);
        out[2 * plane + unit] = (uint16_t)chroma16(a, cr);
    }
}

// ---- deep yuv420p: a lane owns 4 pixels of two rows = two chroma samples; the same chroma mean as the 8-bit kernel --------------
template <bool WIDE>
__global__ void __launch_bounds__(256) k_frames_yuv420p16(FramesArgs a)
{
    const float *img = a.img[blockIdx.y];
    uint16_t *out = reinterpret_cast<uint16_t *>(a.out + (size_t)blockIdx.y * (size_t)a.out_stride);
    const size_t plane = (size_t)a.H * (size_t)a.W;
    const int W2 = a.W >> 1, H2 = a.H >> 1;
    uint16_t *out_u = out + plane, *out_v = out_u + (size_t)H2 * W2;
    const int unit = blockIdx.x * 256 + threadIdx.x;
    if (WIDE) {
        const int per_row = a.W >> 2;
        if (unit >= per_row * H2) return;
        const int yb = unit / per_row, x = (unit - yb * per_row) << 2;
        const size_t at = (size_t)(2 * yb) * a.W + x;
        float c[3][2][4];
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
#pragma unroll
            for (int r = 0; r < 2; r++) load4(img + ch * plane + at + (size_t)r * a.W, c[ch][r]);
        uint32_t wy[2][2] = {{0, 0}, {0, 0}}, wu = 0, wv = 0;
#pragma unroll
        for (int p = 0; p < 2; p++) {
            float cb[2][2], cr[2][2];
#pragma unroll
            for (int r = 0; r < 2; r++)
#pragma unroll
                for (int s = 0; s < 2; s++) {
                    const int px = 2 * p + s;
                    float Y;
                    ycc(a, clamp01(c[0][r][px]), clamp01(c[1][r][px]), clamp01(c[2][r][px]), Y, cb[r][s], cr[r][s]);
                    wy[r][p] |= luma16(a, Y) << (16 * s);
                }
            wu |= chroma16(a, ((cb[0][0] + cb[0][1]) + (cb[1][0] + cb[1][1])) * 0.25f) << (16 * p);
            wv |= chroma16(a, ((cr[0][0] + cr[0][1]) + (cr[1][0] + cr[1][1])) * 0.25f) << (16 * p);
        }
        *reinterpret_cast<uint2 *>(out + at) = make_uint2(wy[0][0], wy[0][1]);
        *reinterpret_cast<uint2 *>(out + at + a.W) = make_uint2(wy[1][0], wy[1][1]);
        const size_t cat = (size_t)yb * W2 + (x >> 1);
        *reinterpret_cast<uint32_t *>(out_u + cat) = wu;
        *reinterpret_cast<uint32_t *>(out_v + cat) = wv;
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
                out[i] = (uint16_t)luma16(a, Y);
            }
        out_u[unit] = (uint16_t)chroma16(a, ((cb[0][0] + cb[0][1]) + (cb[1][0] + cb[1][1])) * 0.25f);
        out_v[unit] = (uint16_t)chroma16(a, ((cr[0][0] + cr[0][1]) + (cr[1][0] + cr[1][1])) * 0.25f);
    }
}

}  // namespace gsvc

using namespace gsvc;

static void set_matrix(FramesArgs &a, int32_t matrix)
{
    const double Kr = matrix == GSVC_FRAMES_BT709 ? 0.2126 : 0.299, Kb = matrix == GSVC_FRAMES_BT709 ? 0.0722 : 0.114;
    a.kr = (float)Kr;
    a.kg = (float)(1.0 - Kr - Kb);
    a.kb = (float)Kb;
    a.icb = (float)(1.0 / (2.0 * (1.0 - Kb)));
    a.icr = (float)(1.0 / (2.0 * (1.0 - Kr)));
}

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

extern "C" int gsvc_frames_to_u8(const float *const *images_host, int32_t n, int32_t H, int32_t W, int32_t layout, int32_t matrix,
                                 int32_t range, int32_t rounding, uint8_t *out, int64_t out_stride, void *stream)
{
    GSVC_REQUIRE(images_host && out, "frames_to_u8: NULL pointer");
    GSVC_REQUIRE(n >= 1 && n <= GSVC_FRAMES_MAX_BATCH, "frames_to_u8: n must be 1 .. %d (got %d)", GSVC_FRAMES_MAX_BATCH, (int)n);
    GSVC_REQUIRE(layout == GSVC_FRAMES_RGB24 || layout == GSVC_FRAMES_YUV444P || layout == GSVC_FRAMES_YUV420P,
                 "frames_to_u8: unknown layout %d", (int)layout);
    GSVC_REQUIRE(matrix == GSVC_FRAMES_BT709 || matrix == GSVC_FRAMES_BT601, "frames_to_u8: unknown matrix %d", (int)matrix);
    GSVC_REQUIRE(range == GSVC_FRAMES_LIMITED || range == GSVC_FRAMES_FULL, "frames_to_u8: unknown range %d", (int)range);
    GSVC_REQUIRE(rounding == GSVC_FRAMES_TRUNC || rounding == GSVC_FRAMES_NEAREST, "frames_to_u8: unknown rounding %d", (int)rounding);
    GSVC_REQUIRE(H >= 1 && W >= 1 && H <= 32768 && W <= 32768, "frames_to_u8: image size must be 1 .. 32768 (got %d x %d)", (int)H, (int)W);
    GSVC_REQUIRE(layout != GSVC_FRAMES_YUV420P || (H % 2 == 0 && W % 2 == 0), "frames_to_u8: yuv420p needs even H and W (got %d x %d)",
                 (int)H, (int)W);
    const int64_t bytes = gsvc_frames_u8_bytes(H, W, layout);
    GSVC_REQUIRE(out_stride >= bytes, "frames_to_u8: out_stride %lld is shorter than a frame (%lld bytes)", (long long)out_stride,
                 (long long)bytes);
    FramesArgs a;
    uintptr_t align = reinterpret_cast<uintptr_t>(out) | (n > 1 ? (uintptr_t)out_stride : 0);
    for (int k = 0; k < GSVC_FRAMES_MAX_BATCH; k++) {
        a.img[k] = images_host[k < n ? k : 0];
        GSVC_REQUIRE(a.img[k], "frames_to_u8: NULL image pointer");
        GSVC_REQUIRE((reinterpret_cast<uintptr_t>(a.img[k]) & 3) == 0, "frames_to_u8: image %d is not 4-byte aligned", k);
        align |= reinterpret_cast<uintptr_t>(a.img[k]);
    }
    a.out = out;
    a.out_stride = out_stride;
    a.H = H;
    a.W = W;
    set_matrix(a, matrix);
    a.y_scale = range == GSVC_FRAMES_LIMITED ? 219.f : 255.f;
    a.y_off = range == GSVC_FRAMES_LIMITED ? 16.f : 0.f;
    a.c_scale = range == GSVC_FRAMES_LIMITED ? 224.f : 255.f;
    a.c_off = 128.f;
    a.rnd = rounding == GSVC_FRAMES_NEAREST ? 0.5f : 0.f;
    a.top = 255.f;
    // the wide path: whole lanes of pixels per row and 16-byte-aligned bases (a row of W % 4 == 0 floats keeps the alignment)
    const int lane_px = layout == GSVC_FRAMES_YUV420P ? 8 : 16;
    const bool fast = W % lane_px == 0 && (align & 15) == 0;
    int64_t units;
    if (layout == GSVC_FRAMES_YUV420P) units = fast ? (int64_t)(W / 8) * (H / 2) : (int64_t)(W / 2) * (H / 2);
    else units = fast ? (int64_t)(W / 16) * H : (int64_t)W * H;
    const dim3 grid((unsigned)((units + 255) / 256), (unsigned)n), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (layout == GSVC_FRAMES_RGB24) {
        ProfScope _p("k_frames_rgb24", s);
        if (fast) hipLaunchKernelGGL(k_frames_rgb24<true>, grid, block, 0, s, a);
        else hipLaunchKernelGGL(k_frames_rgb24<false>, grid, block, 0, s, a);
    } else if (layout == GSVC_FRAMES_YUV444P) {
        ProfScope _p("k_frames_yuv444p", s);
        if (fast) hipLaunchKernelGGL(k_frames_yuv444p<true>, grid, block, 0, s, a);
        else hipLaunchKernelGGL(k_frames_yuv444p<false>, grid, block, 0, s, a);
    } else {
        ProfScope _p("k_frames_yuv420p", s);
        if (fast) hipLaunchKernelGGL(k_frames_yuv420p<true>, grid, block, 0, s, a);
        else hipLaunchKernelGGL(k_frames_yuv420p<false>, grid, block, 0, s, a);
    }
    return check_launch("frames_to_u8");
}

extern "C" int64_t gsvc_frames_bytes(int32_t H, int32_t W, int32_t layout, int32_t depth)
{
    if (depth == 8) return gsvc_frames_u8_bytes(H, W, layout);
    if (depth < 9 || depth > 16 || layout == GSVC_FRAMES_RGB24) return -1;
    const int64_t bytes = gsvc_frames_u8_bytes(H, W, layout);
    return bytes < 0 ? bytes : 2 * bytes;
}

extern "C" int gsvc_frames_to_u16(const float *const *images_host, int32_t n, int32_t H, int32_t W, int32_t layout, int32_t matrix,
                                  int32_t range, int32_t rounding, int32_t depth, uint8_t *out, int64_t out_stride, void *stream)
{
    GSVC_REQUIRE(images_host && out, "frames_to_u16: NULL pointer");
    GSVC_REQUIRE(n >= 1 && n <= GSVC_FRAMES_MAX_BATCH, "frames_to_u16: n must be 1 .. %d (got %d)", GSVC_FRAMES_MAX_BATCH, (int)n);
    GSVC_REQUIRE(layout != GSVC_FRAMES_RGB24, "frames_to_u16: rgb24 frames are 8-bit only");
    GSVC_REQUIRE(layout == GSVC_FRAMES_YUV444P || layout == GSVC_FRAMES_YUV420P, "frames_to_u16: unknown layout %d", (int)layout);
    GSVC_REQUIRE(depth >= 9 && depth <= 16, "frames_to_u16: depth must be 9 .. 16 (got %d)", (int)depth);
    GSVC_REQUIRE(matrix == GSVC_FRAMES_BT709 || matrix == GSVC_FRAMES_BT601, "frames_to_u16: unknown matrix %d", (int)matrix);
    GSVC_REQUIRE(range == GSVC_FRAMES_LIMITED || range == GSVC_FRAMES_FULL, "frames_to_u16: unknown range %d", (int)range);
    GSVC_REQUIRE(rounding == GSVC_FRAMES_TRUNC || rounding == GSVC_FRAMES_NEAREST, "frames_to_u16: unknown rounding %d", (int)rounding);
    GSVC_REQUIRE(H >= 1 && W >= 1 && H <= 32768 && W <= 32768, "frames_to_u16: image size must be 1 .. 32768 (got %d x %d)", (int)H, (int)W);
    GSVC_REQUIRE(layout != GSVC_FRAMES_YUV420P || (H % 2 == 0 && W % 2 == 0), "frames_to_u16: yuv420p needs even H and W (got %d x %d)",
                 (int)H, (int)W);
    GSVC_REQUIRE((reinterpret_cast<uintptr_t>(out) & 1) == 0, "frames_to_u16: the frame base is not 2-byte aligned");
    GSVC_REQUIRE((out_stride & 1) == 0, "frames_to_u16: out_stride %lld is not a multiple of 2", (long long)out_stride);
    const int64_t bytes = gsvc_frames_bytes(H, W, layout, depth);
    GSVC_REQUIRE(out_stride >= bytes, "frames_to_u16: out_stride %lld is shorter than a frame (%lld bytes)", (long long)out_stride,
                 (long long)bytes);
    FramesArgs a;
    uintptr_t align = reinterpret_cast<uintptr_t>(out) | (n > 1 ? (uintptr_t)out_stride : 0);
    for (int k = 0; k < GSVC_FRAMES_MAX_BATCH; k++) {
        a.img[k] = images_host[k < n ? k : 0];
        GSVC_REQUIRE(a.img[k], "frames_to_u16: NULL image pointer");
        GSVC_REQUIRE((reinterpret_cast<uintptr_t>(a.img[k]) & 3) == 0, "frames_to_u16: image %d is not 4-byte aligned", k);
        align |= reinterpret_cast<uintptr_t>(a.img[k]);
    }
    a.out = out;
    a.out_stride = out_stride;
    a.H = H;
    a.W = W;
    set_matrix(a, matrix);
    // limited range: the 8-bit constants times 2^(d - 8), so the value before rounding is exactly 2^(d - 8) times the 8-bit kernel's
    const float up = (float)(1 << (depth - 8)), top = (float)((1 << depth) - 1);
    a.y_scale = range == GSVC_FRAMES_LIMITED ? 219.f * up : top;
    a.y_off = range == GSVC_FRAMES_LIMITED ? 16.f * up : 0.f;
    a.c_scale = range == GSVC_FRAMES_LIMITED ? 224.f * up : top;
    a.c_off = 128.f * up;
    a.rnd = rounding == GSVC_FRAMES_NEAREST ? 0.5f : 0.f;
    a.top = top;
    // the wide path: whole lanes of 4 pixels per row and 16-byte-aligned bases.  W % 4 == 0 keeps every float row 16-byte aligned,
    // the code rows and planes (2 H W bytes apart) 8-byte aligned and the 4:2:0 chroma rows (W bytes; V at H W / 2 bytes behind U) 4-byte aligned.
    const bool wide = W % 4 == 0 && (align & 15) == 0;
    int64_t units;
    if (layout == GSVC_FRAMES_YUV420P) units = wide ? (int64_t)(W / 4) * (H / 2) : (int64_t)(W / 2) * (H / 2);
    else units = wide ? (int64_t)W * H / 4 : (int64_t)W * H;
    const dim3 grid((unsigned)((units + 255) / 256), (unsigned)n), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (layout == GSVC_FRAMES_YUV444P) {
        ProfScope _p("k_frames_yuv444p16", s);
        if (wide) hipLaunchKernelGGL(k_frames_yuv444p16<true>, grid, block, 0, s, a);
        else hipLaunchKernelGGL(k_frames_yuv444p16<false>, grid, block, 0, s, a);
    } else {
        ProfScope _p("k_frames_yuv420p16", s);
        if (wide) hipLaunchKernelGGL(k_frames_yuv420p16<true>, grid, block, 0, s, a);
        else hipLaunchKernelGGL(k_frames_yuv420p16<false>, grid, block, 0, s, a);
    }
    return check_launch("frames_to_u16");
}
