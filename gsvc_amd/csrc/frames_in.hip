// gsvc_amd/csrc/frames_in.hip — encoder input: 8-bit RGB24 / YUV 4:4:4 / YUV 4:2:0 frames and 9 .. 16-bit planar YUV frames
// (little-endian 16-bit words) -> float [3, H, W] RGB images, gfx950.
//
// The mirror image of frames_out.hip.  A video file holds 8 bits per sample (3.1 MB per 1080p 4:2:0 frame); the fitting step reads
// float32 images (24.9 MB).  One launch converts the up to 16 frames of an upload chunk — a pure stream, 1.5 - 6 bytes read and 12
// bytes written per pixel, no LDS, no reuse beyond the chroma neighbours that the caches serve.
//
// One kernel body per layout; the sample type T (uint8_t, uint16_t) and the lane's pixels per row PX are template arguments:
//   wide path   (W a multiple of PX, the input base, its stride and every image base 16-byte aligned): a lane stores 16 bytes at a time
//                   rgb24       16 pixels x 1 row   <- 48 B as 3 x 16 B                               (8-bit only, interleaved)
//                   yuv444p     <uint8_t, 16>  16 pixels x 1 row   <- 16 B of each plane
//                               <uint16_t, 4>   4 pixels x 1 row   <-  8 B of each plane
//                   yuv420p     <uint8_t, 16>  16 pixels x 2 rows  <- 2 x 16 B of Y, 8 B of U and of V per chroma row
//                               <uint16_t, 4>   4 pixels x 2 rows  <- 2 x  8 B of Y, 4 B of U and of V per chroma row
//                               (bilinear: three chroma rows, and one sample to either side of the lane's PX / 2 chroma columns)
//               The deep lane owns FOUR pixels so that lane i of a wave stores its float4 at base + 16 i: one wave instruction writes
//               1 KiB of one row contiguously, the 12 of 14 - 18 bytes per pixel that are this stage's traffic.
//   edge path   (any W, any input alignment a sample allows, any 4-byte-aligned image base): one pixel per lane, one load per sample,
//               4-byte stores.
// Both paths and both sample types evaluate the same expressions in the same order, every fused multiply-add spelled out, so which
// path a frame takes does not change a bit of its floats.  The 4:2:0 chroma is upsampled on the CODES (exact in float32: every
// interpolated code is a multiple of 1/16 below 2^16, 20 bits) and goes through the affine map afterwards.  A deep code above 2^d - 1
// is not masked; the result clamps.
// The batch index is blockIdx.y; the image pointers travel by value in the kernel arguments.
// The profile names of the deep instantiations keep their 16: k_frames_in_yuv444p16, k_frames_in_yuv420p16.
// The argument checks, Kr / Kb and the range constants are those of frames_common.h; one host body serves both entries.
#include "frames_common.h"

namespace gsvc {

struct FramesInArgs {
    float *img[GSVC_FRAMES_MAX_BATCH];
    const uint8_t *in;
    long long in_stride;
    int H, W;
    float y_off, y_div;         // Y = (y code - y_off) / y_div      (frames_range: limited 16, 219; full 0, 255; times 2^(d - 8) / 2^d - 1)
    float c_off, c_div;         // C = (c code - c_off) / c_div
    float r_cr, b_cb;           // 2 (1 - Kr), 2 (1 - Kb)
    float g_cr, g_cb;           // 2 Kr (1 - Kr) / Kg, 2 Kb (1 - Kb) / Kg
};

// one pixel: sample codes (the chroma codes may be interpolated, multiples of 1/16) -> clamped R, G, B
__device__ __forceinline__ void rgb_of(const FramesInArgs &a, float y8, float cb8, float cr8, float &r, float &g, float &b)
{
    const float Y = (y8 - a.y_off) / a.y_div;
    const float Cb = (cb8 - a.c_off) / a.c_div;
    const float Cr = (cr8 - a.c_off) / a.c_div;
    r = clamp01(fmaf(a.r_cr, Cr, Y));
    g = clamp01(fmaf(-a.g_cb, Cb, fmaf(-a.g_cr, Cr, Y)));
    b = clamp01(fmaf(a.b_cb, Cb, Y));
}

// one axis of the centre-sited 2x upsampling: 0.75 of the sample the luma position lies in, 0.25 of its neighbour on that side
__device__ __forceinline__ float up2(float near, float far) { return fmaf(0.25f, far, 0.75f * near); }

// rows first, then columns: nn = (near row, near column), fn = (far row, near column), nf = (near row, far column), ff
__device__ __forceinline__ float up2x2(float nn, float fn, float nf, float ff) { return up2(up2(nn, fn), up2(nf, ff)); }

__device__ __forceinline__ void store4(float *p, const float *v) { *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]); }

__device__ __forceinline__ void store_pixel(float *img, size_t plane, size_t at, float r, float g, float b)
{
    img[at] = r;
    img[plane + at] = g;
    img[2 * plane + at] = b;
}

// ---- rgb24: c = b / 255, an IEEE division (bit-equal to uint8 -> float32 -> div(255)) --------------------------------------
template <bool WIDE>
__global__ void __launch_bounds__(256) k_frames_in_rgb24(FramesInArgs a)
{
    float *img = a.img[blockIdx.y];
    const uint8_t *in = a.in + (size_t)blockIdx.y * (size_t)a.in_stride;
    const size_t plane = (size_t)a.H * (size_t)a.W;
    const int unit = blockIdx.x * 256 + threadIdx.x;
    if (WIDE) {
        if ((size_t)unit >= plane / 16) return;
        const size_t at = (size_t)unit * 16;          // (W is a multiple of 16: units are consecutive over the rows)
        uint32_t w[12];
        load_words<48>(in + 3 * at, w);
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                float v[4];
#pragma unroll
                for (int p = 0; p < 4; p++) v[p] = (float)code_of<1>(w, 3 * (4 * q + p) + ch) / 255.f;
                store4(img + ch * plane + at + 4 * q, v);
            }
    } else {
        if ((size_t)unit >= plane) return;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) img[ch * plane + unit] = (float)in[3 * (size_t)unit + ch] / 255.f;
    }
}

// ---- yuv444p -----------------------------------------------------------------------------------------------------------
template <typename T, int PX, bool WIDE>
__global__ void __launch_bounds__(256) k_frames_in_yuv444p(FramesInArgs a)
{
    constexpr int BPS = (int)sizeof(T);
    float *img = a.img[blockIdx.y];
    const T *in = reinterpret_cast<const T *>(a.in + (size_t)blockIdx.y * (size_t)a.in_stride);
    const size_t plane = (size_t)a.H * (size_t)a.W;
    const int unit = blockIdx.x * 256 + threadIdx.x;
    if (WIDE) {
        if ((size_t)unit >= plane / PX) return;
        const size_t at = (size_t)unit * PX;          // (W is a multiple of PX: units are consecutive over the rows)
        uint32_t wy[PX * BPS / 4], wu[PX * BPS / 4], wv[PX * BPS / 4];
        load_words<PX * BPS>(in + at, wy);
        load_words<PX * BPS>(in + plane + at, wu);
        load_words<PX * BPS>(in + 2 * plane + at, wv);
#pragma unroll
        for (int q = 0; q < PX / 4; q++) {
            float r[4], g[4], b[4];
#pragma unroll
            for (int p = 0; p < 4; p++) {
                const int px = 4 * q + p;
                rgb_of(a, (float)code_of<BPS>(wy, px), (float)code_of<BPS>(wu, px), (float)code_of<BPS>(wv, px), r[p], g[p], b[p]);
            }
            store4(img + at + 4 * q, r);
            store4(img + plane + at + 4 * q, g);
            store4(img + 2 * plane + at + 4 * q, b);
        }
    } else {
        if ((size_t)unit >= plane) return;
        float r, g, b;
        rgb_of(a, (float)in[unit], (float)in[plane + unit], (float)in[2 * plane + unit], r, g, b);
        store_pixel(img, plane, unit, r, g, b);
    }
}

// ---- yuv420p: centre-sited chroma, BIL ? bilinear 2x upsampling of the codes (indices clamped at the borders) : nearest.
//      A lane owns PX pixels of two rows = PX / 2 chroma samples of the near chroma row. ------------------------------------------
template <typename T, int PX, bool WIDE, bool BIL>
__global__ void __launch_bounds__(256) k_frames_in_yuv420p(FramesInArgs a)
{
    constexpr int BPS = (int)sizeof(T);
    float *img = a.img[blockIdx.y];
    const T *in = reinterpret_cast<const T *>(a.in + (size_t)blockIdx.y * (size_t)a.in_stride);
    const size_t plane = (size_t)a.H * (size_t)a.W;
    const int W2 = a.W >> 1, H2 = a.H >> 1;
    const T *in_u = in + plane, *in_v = in_u + (size_t)H2 * W2;
    const int unit = blockIdx.x * 256 + threadIdx.x;
    if (WIDE) {
        constexpr int CX = PX / 2;          // chroma columns of a lane
        const int per_row = a.W / PX;
        if (unit >= per_row * H2) return;
        const int i = unit / per_row, x0 = (unit - i * per_row) * PX, j0 = x0 >> 1;
        const size_t at = (size_t)(2 * i) * a.W + x0;
        // chroma codes of the rows (i - 1, i, i + 1) at the columns j0 - 1 .. j0 + CX, all indices clamped: cu[row][1 + k] = column j0 + k
        float cu[3][CX + 2], cv[3][CX + 2];
        const int jl = j0 > 0 ? j0 - 1 : 0, jr = j0 + CX < W2 ? j0 + CX : W2 - 1;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            if (!BIL && r != 1) continue;
            int ir = i + r - 1;
            ir = ir < 0 ? 0 : (ir > H2 - 1 ? H2 - 1 : ir);
            const size_t row = (size_t)ir * W2;
            uint32_t tu[CX * BPS / 4], tv[CX * BPS / 4];
            load_words<CX * BPS>(in_u + row + j0, tu);
            load_words<CX * BPS>(in_v + row + j0, tv);
#pragma unroll
            for (int k = 0; k < CX; k++) {
                cu[r][1 + k] = (float)code_of<BPS>(tu, k);
                cv[r][1 + k] = (float)code_of<BPS>(tv, k);
            }
            if (BIL) {
                cu[r][0] = (float)in_u[row + jl];
                cu[r][CX + 1] = (float)in_u[row + jr];
                cv[r][0] = (float)in_v[row + jl];
                cv[r][CX + 1] = (float)in_v[row + jr];
            }
        }
#pragma unroll
        for (int s = 0; s < 2; s++) {          // luma row 2 i + s: its far chroma row is i - 1 (s = 0) or i + 1 (s = 1)
            uint32_t wy[PX * BPS / 4];
            load_words<PX * BPS>(in + at + (size_t)s * a.W, wy);
            const int fr = 2 * s;
#pragma unroll
            for (int q = 0; q < PX / 4; q++) {
                float r[4], g[4], b[4];
#pragma unroll
                for (int p = 0; p < 4; p++) {
                    const int px = 4 * q + p, nc = 1 + (px >> 1), fc = (px & 1) ? nc + 1 : nc - 1;
                    const float cb = BIL ? up2x2(cu[1][nc], cu[fr][nc], cu[1][fc], cu[fr][fc]) : cu[1][nc];
                    const float cr = BIL ? up2x2(cv[1][nc], cv[fr][nc], cv[1][fc], cv[fr][fc]) : cv[1][nc];
                    rgb_of(a, (float)code_of<BPS>(wy, px), cb, cr, r[p], g[p], b[p]);
                }
                const size_t o = at + (size_t)s * a.W + 4 * q;
                store4(img + o, r);
                store4(img + plane + o, g);
                store4(img + 2 * plane + o, b);
            }
        }
    } else {
        if ((size_t)unit >= plane) return;
        const int y = unit / a.W, x = unit - y * a.W;
        const int i = y >> 1, j = x >> 1;
        float cb, cr;
        if (BIL) {
            int fi = (y & 1) ? i + 1 : i - 1, fj = (x & 1) ? j + 1 : j - 1;
            fi = fi < 0 ? 0 : (fi > H2 - 1 ? H2 - 1 : fi);
            fj = fj < 0 ? 0 : (fj > W2 - 1 ? W2 - 1 : fj);
            const size_t nrow = (size_t)i * W2, frow = (size_t)fi * W2;
            cb = up2x2((float)in_u[nrow + j], (float)in_u[frow + j], (float)in_u[nrow + fj], (float)in_u[frow + fj]);
            cr = up2x2((float)in_v[nrow + j], (float)in_v[frow + j], (float)in_v[nrow + fj], (float)in_v[frow + fj]);
        } else {
            cb = (float)in_u[(size_t)i * W2 + j];
            cr = (float)in_v[(size_t)i * W2 + j];
        }
        float r, g, b;
        rgb_of(a, (float)in[unit], cb, cr, r, g, b);
        store_pixel(img, plane, unit, r, g, b);
    }
}

}  // namespace gsvc

using namespace gsvc;

// both entries; who = the entry's name, deep = the _u16 one (depth 9 .. 16; the _u8 one passes depth 8)
static int frames_from(const char *who, bool deep, const uint8_t *in, int64_t in_stride, int32_t n, int32_t H, int32_t W, int32_t layout,
                       int32_t matrix, int32_t range, int32_t chroma, int32_t depth, float *const *images_host, void *stream)
{
    GSVC_REQUIRE(images_host && in, "%s: NULL pointer", who);
    GSVC_FRAMES_TRY(frames_check_format(who, n, GSVC_FRAMES_MAX_BATCH, layout, depth, deep ? 9 : 8, deep ? 16 : 8));
    GSVC_FRAMES_TRY(frames_check_colour(who, matrix, range));
    GSVC_REQUIRE(chroma == GSVC_FRAMES_CHROMA_NEAREST || chroma == GSVC_FRAMES_CHROMA_BILINEAR, "%s: unknown chroma mode %d", who, (int)chroma);
    GSVC_FRAMES_TRY(frames_check_size(who, H, W, layout));
    const FrameBufs bufs = {"in_stride", in, in_stride, nullptr, 0};
    if (deep) GSVC_FRAMES_TRY(frames_check_even(who, bufs));
    GSVC_FRAMES_TRY(frames_check_strides(who, bufs, gsvc_frames_bytes(H, W, layout, depth)));
    FramesInArgs a;
    uintptr_t align = bufs.alignment(n);
    GSVC_FRAMES_TRY(frames_gather_images(who, images_host, n, a.img, align));
    a.in = in;
    a.in_stride = in_stride;
    a.H = H;
    a.W = W;
    const FrameMatrix m = frames_matrix(matrix);
    const double Kg = 1.0 - m.Kr - m.Kb;
    a.r_cr = (float)(2.0 * (1.0 - m.Kr));
    a.b_cb = (float)(2.0 * (1.0 - m.Kb));
    a.g_cr = (float)(2.0 * m.Kr * (1.0 - m.Kr) / Kg);
    a.g_cb = (float)(2.0 * m.Kb * (1.0 - m.Kb) / Kg);
    const FrameRange r = frames_range(range, depth);
    a.y_off = r.y_off;
    a.y_div = r.y_scale;
    a.c_off = r.c_off;
    a.c_div = r.c_scale;
    // the wide path: whole lanes of PX pixels per row and 16-byte-aligned bases.  At 8 bits W % 16 == 0 keeps every row, the planes of a
    // 4:4:4 frame (H W) and the 8-byte chroma rows of a 4:2:0 frame (planes at H W and H W + H W / 4, rows of W / 2) aligned; at 16 bits
    // W % 4 == 0 keeps every float row 16-byte aligned, the code rows and planes (2 H W bytes apart) 8-byte aligned and the 4:2:0 chroma
    // rows (W bytes; V at H W / 2 bytes behind U) 4-byte aligned.
    const int lane_px = deep ? 4 : 16;
    const bool wide = W % lane_px == 0 && (align & 15) == 0;
    int64_t units;
    if (layout == GSVC_FRAMES_YUV420P && wide) units = (int64_t)(W / lane_px) * (H / 2);
    else units = (int64_t)W * H / (wide ? lane_px : 1);
    using Kernel = void (*)(FramesInArgs);
    static const Kernel rgb24[2] = {k_frames_in_rgb24<false>, k_frames_in_rgb24<true>};          // [wide]
    static const Kernel yuv444p[2][2] = {{k_frames_in_yuv444p<uint8_t, 16, false>, k_frames_in_yuv444p<uint8_t, 16, true>},
                                         {k_frames_in_yuv444p<uint16_t, 4, false>, k_frames_in_yuv444p<uint16_t, 4, true>}};      // [deep][wide]
    static const Kernel yuv420p[2][2][2] = {                                                                    // [deep][wide][bilinear]
        {{k_frames_in_yuv420p<uint8_t, 16, false, false>, k_frames_in_yuv420p<uint8_t, 16, false, true>},
         {k_frames_in_yuv420p<uint8_t, 16, true, false>, k_frames_in_yuv420p<uint8_t, 16, true, true>}},
        {{k_frames_in_yuv420p<uint16_t, 4, false, false>, k_frames_in_yuv420p<uint16_t, 4, false, true>},
         {k_frames_in_yuv420p<uint16_t, 4, true, false>, k_frames_in_yuv420p<uint16_t, 4, true, true>}}};
    const bool bil = chroma == GSVC_FRAMES_CHROMA_BILINEAR;
    const Kernel kernel = layout == GSVC_FRAMES_RGB24 ? rgb24[wide] : (layout == GSVC_FRAMES_YUV444P ? yuv444p[deep][wide] : yuv420p[deep][wide][bil]);
    const char *const name = layout == GSVC_FRAMES_RGB24 ? "k_frames_in_rgb24"
                             : (layout == GSVC_FRAMES_YUV444P ? (deep ? "k_frames_in_yuv444p16" : "k_frames_in_yuv444p")
                                                              : (deep ? "k_frames_in_yuv420p16" : "k_frames_in_yuv420p"));
    hipStream_t s = (hipStream_t)stream;
    ProfScope _p(name, s);
    hipLaunchKernelGGL(kernel, dim3((unsigned)((units + 255) / 256), (unsigned)n), dim3(256), 0, s, a);
    return check_launch(who);
}

extern "C" int gsvc_frames_from_u8(const uint8_t *in, int64_t in_stride, int32_t n, int32_t H, int32_t W, int32_t layout, int32_t matrix,
                                   int32_t range, int32_t chroma, float *const *images_host, void *stream)
{
    return frames_from("frames_from_u8", false, in, in_stride, n, H, W, layout, matrix, range, chroma, 8, images_host, stream);
}

extern "C" int gsvc_frames_from_u16(const uint8_t *in, int64_t in_stride, int32_t n, int32_t H, int32_t W, int32_t layout, int32_t matrix,
                                    int32_t range, int32_t chroma, int32_t depth, float *const *images_host, void *stream)
{
    return frames_from("frames_from_u16", true, in, in_stride, n, H, W, layout, matrix, range, chroma, depth, images_host, stream);
}
