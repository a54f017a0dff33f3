// gsvc_amd/csrc/frames_in.hip — encoder input: 8-bit RGB24 / YUV 4:4:4 / YUV 4:2:0 frames and 9 .. 16-bit planar YUV frames
// (little-endian 16-bit words) -> float [3, H, W] RGB images, gfx950.
//
// The mirror image of frames_out.hip.  A video file holds 8 bits per sample (3.1 MB per 1080p 4:2:0 frame); the fitting step reads
// float32 images (24.9 MB).  One launch converts the up to 16 frames of an upload chunk — a pure stream, 1.5 - 3 bytes read and 12
// bytes written per pixel, no LDS, no reuse beyond the chroma neighbours that the caches serve:
//   wide path   (W a multiple of 16, the input base, its stride and every output base 16-byte aligned): a lane never loads less
//               than 8 bytes and stores 16 at a time:  rgb24    16 pixels x 1 row   <- 48 B as 3 x 16 B
//                                                      yuv444p  16 pixels x 1 row   <- 16 B of each plane
//                                                      yuv420p  16 pixels x 2 rows  <- 2 x 16 B of Y, 8 B of U and of V per chroma
//                                                               row (bilinear: three chroma rows and one byte to either side)
//   edge path   (any W, any input alignment, any 4-byte-aligned image base): one pixel per lane, byte loads, 4-byte stores.
// Both paths evaluate the same expressions in the same order, every fused multiply-add spelled out, so which path a frame takes
// does not change a bit of its floats.  The 4:2:0 chroma is upsampled on the CODES (exact in float32: every interpolated code is
// a multiple of 1/16 below 256) and goes through the affine map afterwards.
// The batch index is blockIdx.y; the image pointers travel by value in the kernel arguments.
//
// Deep frames (gsvc_frames_from_u16, the k_frames_in_*16 kernels below) share the per-pixel functions and differ in the lane shape: a
// lane owns FOUR pixels of a row (4:2:0: of two rows), so that lane i of a wave stores its float4 at base + 16 i — one wave instruction
// writes 1 KiB of one row contiguously, the 12 of 14 - 18 bytes per pixel that are this stage's traffic — and loads 8 bytes of codes at
// base + 8 i (4:2:0 chroma: 4 bytes at base + 4 i per chroma row, and in bilinear mode one 2-byte sample to either side).
//   wide path   (W a multiple of 4, the input base, its stride and every image base 16-byte aligned)
//   edge path   (any W, any 2-byte-aligned input, any 4-byte-aligned image base): one pixel per lane, 2-byte loads, 4-byte stores.
// Interpolated deep codes are multiples of 1/16 below 2^16: 20 bits, still exact in float32.
#include "common.h"

namespace gsvc {

struct FramesInArgs {
    float *img[GSVC_FRAMES_MAX_BATCH];
    const uint8_t *in;
    long long in_stride;
    int H, W;
    float y_off, y_div;         // Y = (y8 - y_off) / y_div        (limited: 16, 219; full: 0, 255)
    float c_off, c_div;         // C = (c8 - c_off) / c_div        (c_off 128; limited: 224; full: 255)
                                // (deep frames of d bits: limited 2^(d - 8) times the 8-bit values; full: 0, 2^d - 1, 2^(d - 1), 2^d - 1)
    float r_cr, b_cb;           // 2 (1 - Kr), 2 (1 - Kb)
    float g_cr, g_cb;           // 2 Kr (1 - Kr) / Kg, 2 Kb (1 - Kb) / Kg
};

__device__ __forceinline__ float clamp01_in(float x)
{
    const float c = x > 0.f ? x : 0.f;
    return c < 1.f ? c : 1.f;
}

__device__ __forceinline__ float byte_of(uint32_t w, int k) { return (float)((w >> (8 * k)) & 255u); }
__device__ __forceinline__ float half_of(uint32_t w, int k) { return (float)((w >> (16 * k)) & 65535u); }

// one pixel: sample codes (the chroma codes may be interpolated, multiples of 1/16) -> clamped R, G, B
__device__ __forceinline__ void rgb_of(const FramesInArgs &a, float y8, float cb8, float cr8, float &r, float &g, float &b)
{
    const float Y = (y8 - a.y_off) / a.y_div;
    const float Cb = (cb8 - a.c_off) / a.c_div;
    const float Cr = (cr8 - a.c_off) / a.c_div;
    r = clamp01_in(fmaf(a.r_cr, Cr, Y));
    g = clamp01_in(fmaf(-a.g_cb, Cb, fmaf(-a.g_cr, Cr, Y)));
    b = clamp01_in(fmaf(a.b_cb, Cb, Y));
}

// one axis of the centre-sited 2x upsampling: 0.75 of the sample the luma position lies in, 0.25 of its neighbour on that side
__device__ __forceinline__ float up2(float near, float far) { return fmaf(0.25f, far, 0.75f * near); }

// rows first, then columns: nn = (near row, near column), fn = (far row, near column), nf = (near row, far column), ff
__device__ __forceinline__ float up2x2(float nn, float fn, float nf, float ff) { return up2(up2(nn, fn), up2(nf, ff)); }

__device__ __forceinline__ void store4(float *p, const float *v) { *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]); }

// ---- rgb24: c = b / 255, an IEEE division (bit-equal to uint8 -> float32 -> div(255)) --------------------------------------
template <bool WIDE>
__global__ void __launch_bounds__(256) k_frames_in_rgb24(FramesInArgs a)
{
    float *img = a.img[blockIdx.y];
    const uint8_t *in = a.in + (size_t)blockIdx.y * (size_t)a.in_stride;
    const size_t plane = (size_t)a.H * (size_t)a.W;
    const int unit = blockIdx.x * 256 + threadIdx.x;
    if (WIDE) {
        const int per_row = a.W >> 4;
        if (unit >= per_row * a.H) return;
        const size_t at = (size_t)unit << 4;          // (W is a multiple of 16: units are consecutive over the rows)
        const uint4 *src = reinterpret_cast<const uint4 *>(in + 3 * at);
        const uint4 q0 = src[0], q1 = src[1], q2 = src[2];
        const uint32_t w[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                float v[4];
#pragma unroll
                for (int p = 0; p < 4; p++) {
                    const int j = 3 * (4 * q + p) + ch;
                    v[p] = byte_of(w[j >> 2], j & 3) / 255.f;
                }
                store4(img + ch * plane + at + 4 * q, v);
            }
    } else {
        if ((size_t)unit >= plane) return;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) img[ch * plane + unit] = (float)in[3 * (size_t)unit + ch] / 255.f;
    }
}

// ---- yuv444p -----------------------------------------------------------------------------------------------------------
template <bool WIDE>
__global__ void __launch_bounds__(256) k_frames_in_yuv444p(FramesInArgs a)
{
    float *img = a.img[blockIdx.y];
    const uint8_t *in = a.in + (size_t)blockIdx.y * (size_t)a.in_stride;
    const size_t plane = (size_t)a.H * (size_t)a.W;
    const int unit = blockIdx.x * 256 + threadIdx.x;
    if (WIDE) {
        const int per_row = a.W >> 4;
        if (unit >= per_row * a.H) return;
        const size_t at = (size_t)unit << 4;
        const uint4 qy = *reinterpret_cast<const uint4 *>(in + at);
        const uint4 qu = *reinterpret_cast<const uint4 *>(in + plane + at);
        const uint4 qv = *reinterpret_cast<const uint4 *>(in + 2 * plane + at);
        const uint32_t wy[4] = {qy.x, qy.y, qy.z, qy.w}, wu[4] = {qu.x, qu.y, qu.z, qu.w}, wv[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
        for (int q = 0; q < 4; q++) {
            float r[4], g[4], b[4];
#pragma unroll
            for (int p = 0; p < 4; p++) rgb_of(a, byte_of(wy[q], p), byte_of(wu[q], p), byte_of(wv[q], p), r[p], g[p], b[p]);
            store4(img + at + 4 * q, r);
            store4(img + plane + at + 4 * q, g);
            store4(img + 2 * plane + at + 4 * q, b);
        }
    } else {
        if ((size_t)unit >= plane) return;
        float r, g, b;
        rgb_of(a, (float)in[unit], (float)in[plane + unit], (float)in[2 * plane + unit], r, g, b);
        img[unit] = r;
        img[plane + unit] = g;
        img[2 * plane + unit] = b;
    }
}

// ---- yuv420p: centre-sited chroma, BIL ? bilinear 2x upsampling of the codes (indices clamped at the borders) : nearest ----
template <bool WIDE, bool BIL>
__global__ void __launch_bounds__(256) k_frames_in_yuv420p(FramesInArgs a)
{
    float *img = a.img[blockIdx.y];
    const uint8_t *in = a.in + (size_t)blockIdx.y * (size_t)a.in_stride;
    const size_t plane = (size_t)a.H * (size_t)a.W;
    const int W2 = a.W >> 1, H2 = a.H >> 1;
    const uint8_t *in_u = in + plane, *in_v = in_u + (size_t)H2 * W2;
    const int unit = blockIdx.x * 256 + threadIdx.x;
    if (WIDE) {
        const int per_row = a.W >> 4;
        if (unit >= per_row * H2) return;
        const int i = unit / per_row, x0 = (unit - i * per_row) << 4, j0 = x0 >> 1;
        const size_t at = (size_t)(2 * i) * a.W + x0;
        // chroma codes of the rows (i - 1, i, i + 1) at the columns j0 - 1 .. j0 + 8, all indices clamped: cu[row][1 + k] = column j0 + k
        float cu[3][10], cv[3][10];
        const int jl = j0 > 0 ? j0 - 1 : 0, jr = j0 + 8 < W2 ? j0 + 8 : W2 - 1;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            if (!BIL && r != 1) continue;
            int ir = i + r - 1;
            ir = ir < 0 ? 0 : (ir > H2 - 1 ? H2 - 1 : ir);
            const size_t row = (size_t)ir * W2;
            const uint2 tu = *reinterpret_cast<const uint2 *>(in_u + row + j0), tv = *reinterpret_cast<const uint2 *>(in_v + row + j0);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                cu[r][1 + k] = byte_of(tu.x, k);
                cu[r][5 + k] = byte_of(tu.y, k);
                cv[r][1 + k] = byte_of(tv.x, k);
                cv[r][5 + k] = byte_of(tv.y, k);
            }
            if (BIL) {
                cu[r][0] = (float)in_u[row + jl];
                cu[r][9] = (float)in_u[row + jr];
                cv[r][0] = (float)in_v[row + jl];
                cv[r][9] = (float)in_v[row + jr];
            }
        }
#pragma unroll
        for (int s = 0; s < 2; s++) {          // luma row 2 i + s: its far chroma row is i - 1 (s = 0) or i + 1 (s = 1)
            const uint4 qy = *reinterpret_cast<const uint4 *>(in + at + (size_t)s * a.W);
            const uint32_t wy[4] = {qy.x, qy.y, qy.z, qy.w};
            const int fr = 2 * s;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                float r[4], g[4], b[4];
#pragma unroll
                for (int p = 0; p < 4; p++) {
                    const int px = 4 * q + p, nc = 1 + (px >> 1), fc = (px & 1) ? nc + 1 : nc - 1;
                    const float cb = BIL ? up2x2(cu[1][nc], cu[fr][nc], cu[1][fc], cu[fr][fc]) : cu[1][nc];
                    const float cr = BIL ? up2x2(cv[1][nc], cv[fr][nc], cv[1][fc], cv[fr][fc]) : cv[1][nc];
                    rgb_of(a, byte_of(wy[q], p), cb, cr, r[p], g[p], b[p]);
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
        img[unit] = r;
        img[plane + unit] = g;
        img[2 * plane + unit] = b;
    }
}

// ---- deep yuv444p: 16-bit words as they are (a code above 2^d - 1 is not masked; the result clamps), 4 pixels of a row per lane ----
template <bool WIDE>
__global__ void __launch_bounds__(256) k_frames_in_yuv444p16(FramesInArgs a)
{
    float *img = a.img[blockIdx.y];
    const uint16_t *in = reinterpret_cast<const uint16_t *>(a.in + (size_t)blockIdx.y * (size_t)a.in_stride);
    const size_t plane = (size_t)a.H * (size_t)a.W;
    const int unit = blockIdx.x * 256 + threadIdx.x;
    if (WIDE) {
        if ((size_t)unit >= (plane >> 2)) return;
        const size_t at = (size_t)unit << 2;          // (W is a multiple of 4: units are consecutive over the rows)
        const uint2 qy = *reinterpret_cast<const uint2 *>(in + at);
        const uint2 qu = *reinterpret_cast<const uint2 *>(in + plane + at);
        const uint2 qv = *reinterpret_cast<const uint2 *>(in + 2 * plane + at);
        const uint32_t wy[2] = {qy.x, qy.y}, wu[2] = {qu.x, qu.y}, wv[2] = {qv.x, qv.y};
        float r[4], g[4], b[4];
#pragma unroll
        for (int p = 0; p < 4; p++) rgb_of(a, half_of(wy[p >> 1], p & 1), half_of(wu[p >> 1], p & 1), half_of(wv[p >> 1], p & 1), r[p], g[p], b[p]);
        store4(img + at, r);
        store4(img + plane + at, g);
        store4(img + 2 * plane + at, b);
    } else {
        if ((size_t)unit >= plane) return;
        float r, g, b;
        rgb_of(a, (float)in[unit], (float)in[plane + unit], (float)in[2 * plane + unit], r, g, b);
        img[unit] = r;
        img[plane + unit] = g;
        img[2 * plane + unit] = b;
    }
}

// ---- deep yuv420p: 4 pixels of two rows per lane = two chroma samples of the near row; the upsampling of the 8-bit kernel ---------
template <bool WIDE, bool BIL>
__global__ void __launch_bounds__(256) k_frames_in_yuv420p16(FramesInArgs a)
{
    float *img = a.img[blockIdx.y];
    const uint16_t *in = reinterpret_cast<const uint16_t *>(a.in + (size_t)blockIdx.y * (size_t)a.in_stride);
    const size_t plane = (size_t)a.H * (size_t)a.W;
    const int W2 = a.W >> 1, H2 = a.H >> 1;
    const uint16_t *in_u = in + plane, *in_v = in_u + (size_t)H2 * W2;
    const int unit = blockIdx.x * 256 + threadIdx.x;
    if (WIDE) {
        const int per_row = a.W >> 2;
        if (unit >= per_row * H2) return;
        const int i = unit / per_row, x0 = (unit - i * per_row) << 2, j0 = x0 >> 1;
        const size_t at = (size_t)(2 * i) * a.W + x0;
        // chroma codes of the rows (i - 1, i, i + 1) at the columns j0 - 1 .. j0 + 2, all indices clamped: cu[row][1 + k] = column j0 + k
        float cu[3][4], cv[3][4];
        const int jl = j0 > 0 ? j0 - 1 : 0, jr = j0 + 2 < W2 ? j0 + 2 : W2 - 1;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            if (!BIL && r != 1) continue;
            int ir = i + r - 1;
            ir = ir < 0 ? 0 : (ir > H2 - 1 ? H2 - 1 : ir);
            const size_t row = (size_t)ir * W2;
            const uint32_t tu = *reinterpret_cast<const uint32_t *>(in_u + row + j0), tv = *reinterpret_cast<const uint32_t *>(in_v + row + j0);
            cu[r][1] = half_of(tu, 0);
            cu[r][2] = half_of(tu, 1);
            cv[r][1] = half_of(tv, 0);
            cv[r][2] = half_of(tv, 1);
            if (BIL) {
                cu[r][0] = (float)in_u[row + jl];
                cu[r][3] = (float)in_u[row + jr];
                cv[r][0] = (float)in_v[row + jl];
                cv[r][3] = (float)in_v[row + jr];
            }
        }
#pragma unroll
        for (int s = 0; s < 2; s++) {          // luma row 2 i + s: its far chroma row is i - 1 (s = 0) or i + 1 (s = 1)
            const uint2 qy = *reinterpret_cast<const uint2 *>(in + at + (size_t)s * a.W);
            const uint32_t wy[2] = {qy.x, qy.y};
            const int fr = 2 * s;
            float r[4], g[4], b[4];
#pragma unroll
            for (int px = 0; px < 4; px++) {
                const int nc = 1 + (px >> 1), fc = (px & 1) ? nc + 1 : nc - 1;
                const float cb = BIL ? up2x2(cu[1][nc], cu[fr][nc], cu[1][fc], cu[fr][fc]) : cu[1][nc];
                const float cr = BIL ? up2x2(cv[1][nc], cv[fr][nc], cv[1][fc], cv[fr][fc]) : cv[1][nc];
                rgb_of(a, half_of(wy[px >> 1], px & 1), cb, cr, r[px], g[px], b[px]);
            }
            const size_t o = at + (size_t)s * a.W;
            store4(img + o, r);
            store4(img + plane + o, g);
            store4(img + 2 * plane + o, b);
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
        img[unit] = r;
        img[plane + unit] = g;
        img[2 * plane + unit] = b;
    }
}

}  // namespace gsvc

using namespace gsvc;

static void set_matrix_in(FramesInArgs &a, int32_t matrix)
{
    const double Kr = matrix == GSVC_FRAMES_BT709 ? 0.2126 : 0.299, Kb = matrix == GSVC_FRAMES_BT709 ? 0.0722 : 0.114;
    const double Kg = 1.0 - Kr - Kb;
    a.r_cr = (float)(2.0 * (1.0 - Kr));
    a.b_cb = (float)(2.0 * (1.0 - Kb));
    a.g_cr = (float)(2.0 * Kr * (1.0 - Kr) / Kg);
    a.g_cb = (float)(2.0 * Kb * (1.0 - Kb) / Kg);
}

extern "C" int gsvc_frames_from_u8(const uint8_t *in, int64_t in_stride, int32_t n, int32_t H, int32_t W, int32_t layout, int32_t matrix,
                                   int32_t range, int32_t chroma, float *const *images_host, void *stream)
{
    GSVC_REQUIRE(images_host && in, "frames_from_u8: NULL pointer");
    GSVC_REQUIRE(n >= 1 && n <= GSVC_FRAMES_MAX_BATCH, "frames_from_u8: n must be 1 .. %d (got %d)", GSVC_FRAMES_MAX_BATCH, (int)n);
    GSVC_REQUIRE(layout == GSVC_FRAMES_RGB24 || layout == GSVC_FRAMES_YUV444P || layout == GSVC_FRAMES_YUV420P,
                 "frames_from_u8: unknown layout %d", (int)layout);
    GSVC_REQUIRE(matrix == GSVC_FRAMES_BT709 || matrix == GSVC_FRAMES_BT601, "frames_from_u8: unknown matrix %d", (int)matrix);
    GSVC_REQUIRE(range == GSVC_FRAMES_LIMITED || range == GSVC_FRAMES_FULL, "frames_from_u8: unknown range %d", (int)range);
    GSVC_REQUIRE(chroma == GSVC_FRAMES_CHROMA_NEAREST || chroma == GSVC_FRAMES_CHROMA_BILINEAR, "frames_from_u8: unknown chroma mode %d",
                 (int)chroma);
    GSVC_REQUIRE(H >= 1 && W >= 1 && H <= 32768 && W <= 32768, "frames_from_u8: image size must be 1 .. 32768 (got %d x %d)", (int)H, (int)W);
    GSVC_REQUIRE(layout != GSVC_FRAMES_YUV420P || (H % 2 == 0 && W % 2 == 0), "frames_from_u8: yuv420p needs even H and W (got %d x %d)",
                 (int)H, (int)W);
    const int64_t bytes = gsvc_frames_u8_bytes(H, W, layout);
    GSVC_REQUIRE(in_stride >= bytes, "frames_from_u8: in_stride %lld is shorter than a frame (%lld bytes)", (long long)in_stride,
                 (long long)bytes);
    FramesInArgs a;
    uintptr_t align = reinterpret_cast<uintptr_t>(in) | (n > 1 ? (uintptr_t)in_stride : 0);
    for (int k = 0; k < GSVC_FRAMES_MAX_BATCH; k++) {
        a.img[k] = images_host[k < n ? k : 0];
        GSVC_REQUIRE(a.img[k], "frames_from_u8: NULL image pointer");
        GSVC_REQUIRE((reinterpret_cast<uintptr_t>(a.img[k]) & 3) == 0, "frames_from_u8: image %d is not 4-byte aligned", k);
        align |= reinterpret_cast<uintptr_t>(a.img[k]);
    }
    a.in = in;
    a.in_stride = in_stride;
    a.H = H;
    a.W = W;
    set_matrix_in(a, matrix);
    a.y_off = range == GSVC_FRAMES_LIMITED ? 16.f : 0.f;
    a.y_div = range == GSVC_FRAMES_LIMITED ? 219.f : 255.f;
    a.c_off = 128.f;
    a.c_div = range == GSVC_FRAMES_LIMITED ? 224.f : 255.f;
    // the wide path: whole lanes of 16 pixels per row and 16-byte-aligned bases.  W % 16 == 0 keeps every row, the planes of a
    // 4:4:4 frame (H W) and the 8-byte chroma rows of a 4:2:0 frame (planes at H W and H W + H W / 4, rows of W / 2) aligned.
    const bool wide = W % 16 == 0 && (align & 15) == 0;
    int64_t units;
    if (layout == GSVC_FRAMES_YUV420P && wide) units = (int64_t)(W / 16) * (H / 2);
    else units = wide ? (int64_t)(W / 16) * H : (int64_t)W * H;
    const dim3 grid((unsigned)((units + 255) / 256), (unsigned)n), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (layout == GSVC_FRAMES_RGB24) {
        ProfScope _p("k_frames_in_rgb24", s);
        if (wide) hipLaunchKernelGGL(k_frames_in_rgb24<true>, grid, block, 0, s, a);
        else hipLaunchKernelGGL(k_frames_in_rgb24<false>, grid, block, 0, s, a);
    } else if (layout == GSVC_FRAMES_YUV444P) {
        ProfScope _p("k_frames_in_yuv444p", s);
        if (wide) hipLaunchKernelGGL(k_frames_in_yuv444p<true>, grid, block, 0, s, a);
        else hipLaunchKernelGGL(k_frames_in_yuv444p<false>, grid, block, 0, s, a);
    } else {
        ProfScope _p("k_frames_in_yuv420p", s);
        const bool bil = chroma == GSVC_FRAMES_CHROMA_BILINEAR;
        if (wide && bil) hipLaunchKernelGGL((k_frames_in_yuv420p<true, true>), grid, block, 0, s, a);
        else if (wide) hipLaunchKernelGGL((k_frames_in_yuv420p<true, false>), grid, block, 0, s, a);
        else if (bil) hipLaunchKernelGGL((k_frames_in_yuv420p<false, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((k_frames_in_yuv420p<false, false>), grid, block, 0, s, a);
    }
    return check_launch("frames_from_u8");
}

extern "C" int gsvc_frames_from_u16(const uint8_t *in, int64_t in_stride, int32_t n, int32_t H, int32_t W, int32_t layout, int32_t matrix,
                                    int32_t range, int32_t chroma, int32_t depth, float *const *images_host, void *stream)
{
    GSVC_REQUIRE(images_host && in, "frames_from_u16: NULL pointer");
    GSVC_REQUIRE(n >= 1 && n <= GSVC_FRAMES_MAX_BATCH, "frames_from_u16: n must be 1 .. %d (got %d)", GSVC_FRAMES_MAX_BATCH, (int)n);
    GSVC_REQUIRE(layout != GSVC_FRAMES_RGB24, "frames_from_u16: rgb24 frames are 8-bit only");
    GSVC_REQUIRE(layout == GSVC_FRAMES_YUV444P || layout == GSVC_FRAMES_YUV420P, "frames_from_u16: unknown layout %d", (int)layout);
    GSVC_REQUIRE(depth >= 9 && depth <= 16, "frames_from_u16: depth must be 9 .. 16 (got %d)", (int)depth);
    GSVC_REQUIRE(matrix == GSVC_FRAMES_BT709 || matrix == GSVC_FRAMES_BT601, "frames_from_u16: unknown matrix %d", (int)matrix);
    GSVC_REQUIRE(range == GSVC_FRAMES_LIMITED || range == GSVC_FRAMES_FULL, "frames_from_u16: unknown range %d", (int)range);
    GSVC_REQUIRE(chroma == GSVC_FRAMES_CHROMA_NEAREST || chroma == GSVC_FRAMES_CHROMA_BILINEAR, "frames_from_u16: unknown chroma mode %d",
                 (int)chroma);
    GSVC_REQUIRE(H >= 1 && W >= 1 && H <= 32768 && W <= 32768, "frames_from_u16: image size must be 1 .. 32768 (got %d x %d)", (int)H, (int)W);
    GSVC_REQUIRE(layout != GSVC_FRAMES_YUV420P || (H % 2 == 0 && W % 2 == 0), "frames_from_u16: yuv420p needs even H and W (got %d x %d)",
                 (int)H, (int)W);
    GSVC_REQUIRE((reinterpret_cast<uintptr_t>(in) & 1) == 0, "frames_from_u16: the frame base is not 2-byte aligned");
    GSVC_REQUIRE((in_stride & 1) == 0, "frames_from_u16: in_stride %lld is not a multiple of 2", (long long)in_stride);
    const int64_t bytes = gsvc_frames_bytes(H, W, layout, depth);
    GSVC_REQUIRE(in_stride >= bytes, "frames_from_u16: in_stride %lld is shorter than a frame (%lld bytes)", (long long)in_stride,
                 (long long)bytes);
    FramesInArgs a;
    uintptr_t align = reinterpret_cast<uintptr_t>(in) | (n > 1 ? (uintptr_t)in_stride : 0);
    for (int k = 0; k < GSVC_FRAMES_MAX_BATCH; k++) {
        a.img[k] = images_host[k < n ? k : 0];
        GSVC_REQUIRE(a.img[k], "frames_from_u16: NULL image pointer");
        GSVC_REQUIRE((reinterpret_cast<uintptr_t>(a.img[k]) & 3) == 0, "frames_from_u16: image %d is not 4-byte aligned", k);
        align |= reinterpret_cast<uintptr_t>(a.img[k]);
    }
    a.in = in;
    a.in_stride = in_stride;
    a.H = H;
    a.W = W;
    set_matrix_in(a, matrix);
    const float up = (float)(1 << (depth - 8)), top = (float)((1 << depth) - 1);
    a.y_off = range == GSVC_FRAMES_LIMITED ? 16.f * up : 0.f;
    a.y_div = range == GSVC_FRAMES_LIMITED ? 219.f * up : top;
    a.c_off = 128.f * up;
    a.c_div = range == GSVC_FRAMES_LIMITED ? 224.f * up : top;
    // the wide path: whole lanes of 4 pixels per row and 16-byte-aligned bases.  W % 4 == 0 keeps every float row 16-byte aligned, the
    // code rows and planes (2 H W bytes apart) 8-byte aligned and the 4:2:0 chroma rows (W bytes; V at H W / 2 bytes behind U) 4-byte aligned.
    const bool wide = W % 4 == 0 && (align & 15) == 0;
    int64_t units;
    if (layout == GSVC_FRAMES_YUV420P && wide) units = (int64_t)(W / 4) * (H / 2);
    else units = wide ? (int64_t)W * H / 4 : (int64_t)W * H;
    const dim3 grid((unsigned)((units + 255) / 256), (unsigned)n), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (layout == GSVC_FRAMES_YUV444P) {
        ProfScope _p("k_frames_in_yuv444p16", s);
        if (wide) hipLaunchKernelGGL(k_frames_in_yuv444p16<true>, grid, block, 0, s, a);
        else hipLaunchKernelGGL(k_frames_in_yuv444p16<false>, grid, block, 0, s, a);
    } else {
        ProfScope _p("k_frames_in_yuv420p16", s);
        const bool bil = chroma == GSVC_FRAMES_CHROMA_BILINEAR;
        if (wide && bil) hipLaunchKernelGGL((k_frames_in_yuv420p16<true, true>), grid, block, 0, s, a);
        else if (wide) hipLaunchKernelGGL((k_frames_in_yuv420p16<true, false>), grid, block, 0, s, a);
        else if (bil) hipLaunchKernelGGL((k_frames_in_yuv420p16<false, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((k_frames_in_yuv420p16<false, false>), grid, block, 0, s, a);
    }
    return check_launch("frames_from_u16");
}
