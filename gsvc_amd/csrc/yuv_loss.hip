// gsvc_amd/csrc/yuv_loss.hip — the fitting step's distortion in the delivered domain: float Y'CbCr planes of the render (forward and
// adjoint) and of the file's sample codes, gfx950.
//
// The codec reads Y'CbCr files and is measured on Y'CbCr sample codes; with OptimizationParams.loss_domain = "yuv420" / "yuv444" the
// step's L1 + SSIM is taken on planes instead of on float RGB.  A plane buffer of a picture of H x W is one contiguous float32 array
//     [ Y: H W | Cb: ch cw | Cr: ch cw ],   (ch, cw) = (H / 2, W / 2) for yuv420p (H, W even), (H, W) for yuv444p,
// every plane on a nominal [0, 1]: Y is the luma of frames_out.hip, the chroma planes are its C + 0.5.  Nothing is clamped.  The SSIM /
// L1 kernels of ssim.hip then run on Y (C = 1) and on the two chroma planes (C = 2) as they are.
//
//   k_frames_planes      sample codes -> planes, the ground truth: Y = (y - y_off) / y_scale, C = (c - c_off) / c_scale + 0.5 with the
//                        constants of frames_range (one IEEE division, one addition).  The plane buffer has the frame's own sample
//                        order, so the kernel is a flat walk: a lane takes 4 samples (4 or 8 bytes in, one float4 out).  H W is a
//                        multiple of 4 whenever the flat run is, so a lane's four samples are all luma or all chroma.
//   k_yuv_planes_fwd     a = 0.5 (f + flip_W(b)) (a = f without b), Y = fma(Kr, R, fma(Kg, G, Kb B)), Cb = fma(B - Y, 1 / (2 (1 - Kb)), 0.5),
//                        Cr = fma(R - Y, 1 / (2 (1 - Kr)), 0.5); 4:2:0 chroma = 0.25 ((c00 + c01) + (c10 + c11)) of the 2x2 block.
//   k_yuv_planes_bwd     the exact adjoint (see gsvc_yuv_planes_backward in include/gsvc_hip.h).
//
// The two transform kernels share one shape, the split of frames_out.hip:
//   wide path   (W a multiple of 4, H even, every base 16-byte aligned): a lane owns 2 rows x 4 columns: float4 loads of f, a reversed
//               float4 load of b at column W - 4 - x (aligned because W and x are multiples of 4), float4 stores of Y (and a), float2
//               (4:2:0) or float4 (4:4:4) stores of Cb / Cr.  The chroma mean never leaves registers.
//   edge path   (any W, any 4-byte-aligned base, the odd sizes of 4:4:4): one 2x2 block (4:2:0) or one pixel (4:4:4) per lane.
// Both paths evaluate the same expressions in the same order, every fused multiply-add spelled out, so the path a picture takes does
// not change a bit of its result.  Pure streams: no LDS, no atomics, no scratch.
#include "frames_common.h"

namespace gsvc {

// ---- sample codes -> planes --------------------------------------------------------------------------------------------------------
struct PlanesInArgs {
    float *out[GSVC_FRAMES_MAX_BATCH];
    const uint8_t *in;
    long long in_stride;
    long long samples, luma;            // of one frame; the first `luma` samples are Y
    float y_off, y_div, c_off, c_div;
};

__device__ __forceinline__ float plane_of(const PlanesInArgs &a, float code, bool is_luma)
{
    return is_luma ? (code - a.y_off) / a.y_div : (code - a.c_off) / a.c_div + 0.5f;
}

template <int BPS, bool WIDE>
__global__ void __launch_bounds__(256) k_frames_planes(PlanesInArgs a)
{
    float *out = a.out[blockIdx.y];
    const uint8_t *in = a.in + (size_t)blockIdx.y * (size_t)a.in_stride;
    const long long unit = (long long)blockIdx.x * 256 + threadIdx.x;
    if (WIDE) {
        const long long at = 4 * unit;          // (samples and luma are multiples of 4)
        if (at >= a.samples) return;
        uint32_t w[BPS];
        load_words<4 * BPS>(in + at * BPS, w);
        const bool is_luma = at < a.luma;
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = plane_of(a, (float)code_of<BPS>(w, k), is_luma);
        *reinterpret_cast<float4 *>(out + at) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        if (unit >= a.samples) return;
        out[unit] = plane_of(a, (float)code_at<BPS>(in, unit), unit < a.luma);
    }
}

// ---- the transform -----------------------------------------------------------------------------------------------------------------
struct YuvArgs {
    const float *f, *b;          // forward: the render(s) [3, H, W]; b may be NULL
    float *planes, *avg;         // forward: outputs; avg may be NULL
    const float *d_planes;       // backward: input
    float *d_f, *d_b;            // backward: outputs; d_b may be NULL
    int H, W;
    float kr, kg, kb;            // luma weights
    float icb, icr;              // s_b = 1 / (2 (1 - Kb)), s_r = 1 / (2 (1 - Kr))
};

__device__ __forceinline__ void ycc_planes(const YuvArgs &a, float r, float g, float b, float &y, float &cb, float &cr)
{
    y = fmaf(a.kr, r, fmaf(a.kg, g, a.kb * b));
    cb = fmaf(b - y, a.icb, 0.5f);
    cr = fmaf(r - y, a.icr, 0.5f);
}

// the adjoint of ycc_planes at one pixel, the chroma gradients already scaled by q (0.25: the pixel's share of its 2x2 mean; 1)
__device__ __forceinline__ void ycc_adjoint(const YuvArgs &a, float gy, float qgcb, float qgcr, float &dr, float &dg, float &db)
{
    const float gb = qgcb * a.icb, gr = qgcr * a.icr;
    const float y = fmaf(-qgcr, a.icr, fmaf(-qgcb, a.icb, gy));          // gY' = gY - gB' - gR'
    dr = fmaf(a.kr, y, gr);
    dg = a.kg * y;
    db = fmaf(a.kb, y, gb);
}

__device__ __forceinline__ float mean2x2(const float c[2][2]) { return ((c[0][0] + c[0][1]) + (c[1][0] + c[1][1])) * 0.25f; }

__device__ __forceinline__ void ld4(const float *p, float *v)
{
    const float4 t = *reinterpret_cast<const float4 *>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
__device__ __forceinline__ void ld4_reversed(const float *p, float *v)
{
    const float4 t = *reinterpret_cast<const float4 *>(p);
    v[0] = t.w; v[1] = t.z; v[2] = t.y; v[3] = t.x;
}
__device__ __forceinline__ void st4(float *p, const float *v) { *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ void st4_reversed(float *p, const float *v) { *reinterpret_cast<float4 *>(p) = make_float4(v[3], v[2], v[1], v[0]); }

// the two-view frame at one pixel (row offset `row` = y W, column x) of channel plane `ch`
__device__ __forceinline__ float view_at(const YuvArgs &a, size_t ch, size_t row, int x)
{
    const float f = a.f[ch + row + x];
    return a.b ? 0.5f * (f + a.b[ch + row + (a.W - 1 - x)]) : f;
}

template <bool YUV420, bool WIDE>
__global__ void __launch_bounds__(256) k_yuv_planes_fwd(YuvArgs a)
{
    const size_t plane = (size_t)a.H * (size_t)a.W;
    const int cw = YUV420 ? a.W >> 1 : a.W, chh = YUV420 ? a.H >> 1 : a.H;
    float *out_y = a.planes, *out_cb = a.planes + plane, *out_cr = out_cb + (size_t)chh * cw;
    const int unit = blockIdx.x * 256 + threadIdx.x;
    if (WIDE) {
        const int per_row = a.W >> 2, H2 = a.H >> 1;
        if (unit >= per_row * H2) return;
        const int yb = unit / per_row, x = (unit - yb * per_row) * 4;
        const size_t at = (size_t)(2 * yb) * a.W + x, bat = (size_t)(2 * yb) * a.W + (a.W - 4 - x);
        float v[3][2][4];
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
#pragma unroll
            for (int r = 0; r < 2; r++) {
                ld4(a.f + ch * plane + at + (size_t)r * a.W, v[ch][r]);
                if (a.b) {
                    float t[4];
                    ld4_reversed(a.b + ch * plane + bat + (size_t)r * a.W, t);
#pragma unroll
                    for (int k = 0; k < 4; k++) v[ch][r][k] = 0.5f * (v[ch][r][k] + t[k]);
                }
                if (a.avg) st4(a.avg + ch * plane + at + (size_t)r * a.W, v[ch][r]);
            }
        float Y[2][4], cb[2][4], cr[2][4];
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int k = 0; k < 4; k++) ycc_planes(a, v[0][r][k], v[1][r][k], v[2][r][k], Y[r][k], cb[r][k], cr[r][k]);
        st4(out_y + at, Y[0]);
        st4(out_y + at + a.W, Y[1]);
        if (YUV420) {
            float mb[2], mr[2];
#pragma unroll
            for (int p = 0; p < 2; p++) {
                const float qb[2][2] = {{cb[0][2 * p], cb[0][2 * p + 1]}, {cb[1][2 * p], cb[1][2 * p + 1]}};
                const float qr[2][2] = {{cr[0][2 * p], cr[0][2 * p + 1]}, {cr[1][2 * p], cr[1][2 * p + 1]}};
                mb[p] = mean2x2(qb);
                mr[p] = mean2x2(qr);
            }
            const size_t cat = (size_t)yb * cw + (x >> 1);
            *reinterpret_cast<float2 *>(out_cb + cat) = make_float2(mb[0], mb[1]);
            *reinterpret_cast<float2 *>(out_cr + cat) = make_float2(mr[0], mr[1]);
        } else {
            st4(out_cb + at, cb[0]);
            st4(out_cb + at + a.W, cb[1]);
            st4(out_cr + at, cr[0]);
            st4(out_cr + at + a.W, cr[1]);
        }
    } else if (YUV420) {
        if (unit >= cw * chh) return;
        const int yb = unit / cw, xb = unit - yb * cw;
        float cb[2][2], cr[2][2];
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int s = 0; s < 2; s++) {
                const size_t row = (size_t)(2 * yb + r) * a.W;
                const int x = 2 * xb + s;
                const float R = view_at(a, 0, row, x), G = view_at(a, plane, row, x), B = view_at(a, 2 * plane, row, x);
                if (a.avg) {
                    a.avg[row + x] = R;
                    a.avg[plane + row + x] = G;
                    a.avg[2 * plane + row + x] = B;
                }
                float Y;
                ycc_planes(a, R, G, B, Y, cb[r][s], cr[r][s]);
                out_y[row + x] = Y;
            }
        out_cb[unit] = mean2x2(cb);
        out_cr[unit] = mean2x2(cr);
    } else {
        if ((size_t)unit >= plane) return;
        const int y = unit / a.W, x = unit - y * a.W;
        const size_t row = (size_t)y * a.W;
        const float R = view_at(a, 0, row, x), G = view_at(a, plane, row, x), B = view_at(a, 2 * plane, row, x);
        if (a.avg) {
            a.avg[unit] = R;
            a.avg[plane + unit] = G;
            a.avg[2 * plane + unit] = B;
        }
        float Y, cb, cr;
        ycc_planes(a, R, G, B, Y, cb, cr);
        out_y[unit] = Y;
        out_cb[unit] = cb;
        out_cr[unit] = cr;
    }
}

// one pixel of the adjoint's outputs: d_f at (row, x), d_b at the flipped column
__device__ __forceinline__ void put_grad(const YuvArgs &a, size_t plane, size_t row, int x, float dr, float dg, float db)
{
    if (a.d_b) {
        dr *= 0.5f; dg *= 0.5f; db *= 0.5f;
        const size_t o = row + (a.W - 1 - x);
        a.d_b[o] = dr;
        a.d_b[plane + o] = dg;
        a.d_b[2 * plane + o] = db;
    }
    a.d_f[row + x] = dr;
    a.d_f[plane + row + x] = dg;
    a.d_f[2 * plane + row + x] = db;
}

template <bool YUV420, bool WIDE>
__global__ void __launch_bounds__(256) k_yuv_planes_bwd(YuvArgs a)
{
    const size_t plane = (size_t)a.H * (size_t)a.W;
    const int cw = YUV420 ? a.W >> 1 : a.W, chh = YUV420 ? a.H >> 1 : a.H;
    const float *g_y = a.d_planes, *g_cb = a.d_planes + plane, *g_cr = g_cb + (size_t)chh * cw;
    const float q = YUV420 ? 0.25f : 1.f;
    const int unit = blockIdx.x * 256 + threadIdx.x;
    if (WIDE) {
        const int per_row = a.W >> 2, H2 = a.H >> 1;
        if (unit >= per_row * H2) return;
        const int yb = unit / per_row, x = (unit - yb * per_row) * 4;
        const size_t at = (size_t)(2 * yb) * a.W + x, bat = (size_t)(2 * yb) * a.W + (a.W - 4 - x);
        float gy[2][4], gcb[2][4], gcr[2][4];
        ld4(g_y + at, gy[0]);
        ld4(g_y + at + a.W, gy[1]);
        if (YUV420) {
            const size_t cat = (size_t)yb * cw + (x >> 1);
            const float2 tb = *reinterpret_cast<const float2 *>(g_cb + cat), tr = *reinterpret_cast<const float2 *>(g_cr + cat);
#pragma unroll
            for (int r = 0; r < 2; r++) {
                gcb[r][0] = gcb[r][1] = tb.x; gcb[r][2] = gcb[r][3] = tb.y;
                gcr[r][0] = gcr[r][1] = tr.x; gcr[r][2] = gcr[r][3] = tr.y;
            }
        } else {
            ld4(g_cb + at, gcb[0]);
            ld4(g_cb + at + a.W, gcb[1]);
            ld4(g_cr + at, gcr[0]);
            ld4(g_cr + at + a.W, gcr[1]);
        }
        const float h = a.d_b ? 0.5f : 1.f;
#pragma unroll
        for (int r = 0; r < 2; r++) {
            float d[3][4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                ycc_adjoint(a, gy[r][k], q * gcb[r][k], q * gcr[r][k], d[0][k], d[1][k], d[2][k]);
                d[0][k] *= h; d[1][k] *= h; d[2][k] *= h;
            }
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                st4(a.d_f + ch * plane + at + (size_t)r * a.W, d[ch]);
                if (a.d_b) st4_reversed(a.d_b + ch * plane + bat + (size_t)r * a.W, d[ch]);
            }
        }
    } else if (YUV420) {
        if (unit >= cw * chh) return;
        const int yb = unit / cw, xb = unit - yb * cw;
        const float qb = q * g_cb[unit], qr = q * g_cr[unit];
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int s = 0; s < 2; s++) {
                const size_t row = (size_t)(2 * yb + r) * a.W;
                const int x = 2 * xb + s;
                float dr, dg, db;
                ycc_adjoint(a, g_y[row + x], qb, qr, dr, dg, db);
                put_grad(a, plane, row, x, dr, dg, db);
            }
    } else {
        if ((size_t)unit >= plane) return;
        const int y = unit / a.W, x = unit - y * a.W;
        float dr, dg, db;
        ycc_adjoint(a, g_y[unit], q * g_cb[unit], q * g_cr[unit], dr, dg, db);
        put_grad(a, plane, (size_t)y * a.W, x, dr, dg, db);
    }
}

// the checks and constants both transform entries share
static int yuv_setup(const char *who, int32_t H, int32_t W, int32_t layout, int32_t matrix, YuvArgs &a)
{
    GSVC_REQUIRE(layout == GSVC_FRAMES_YUV444P || layout == GSVC_FRAMES_YUV420P, "%s: the layout must be yuv444p or yuv420p (got %d)", who,
                 (int)layout);
    GSVC_FRAMES_TRY(frames_check_colour(who, matrix, GSVC_FRAMES_LIMITED));
    GSVC_FRAMES_TRY(frames_check_size(who, H, W, layout));
    a = YuvArgs{};
    a.H = H;
    a.W = W;
    const FrameMatrix m = frames_matrix(matrix);
    a.kr = (float)m.Kr;
    a.kg = (float)(1.0 - m.Kr - m.Kb);
    a.kb = (float)m.Kb;
    a.icb = (float)(1.0 / (2.0 * (1.0 - m.Kb)));
    a.icr = (float)(1.0 / (2.0 * (1.0 - m.Kr)));
    return GSVC_OK;
}

static int yuv_pointer(const char *who, const char *name, const void *p)
{
    GSVC_REQUIRE((reinterpret_cast<uintptr_t>(p) & 3) == 0, "%s: %s is not 4-byte aligned", who, name);
    return GSVC_OK;
}

// units of a launch: 2 x 4 tiles (wide), 2 x 2 blocks (4:2:0 edge) or pixels (4:4:4 edge)
static int64_t yuv_units(int32_t H, int32_t W, bool yuv420, bool wide)
{
    if (wide) return (int64_t)(W / 4) * (H / 2);
    return yuv420 ? (int64_t)(W / 2) * (H / 2) : (int64_t)W * H;
}

}  // namespace gsvc

using namespace gsvc;

extern "C" int64_t gsvc_yuv_planes_floats(int32_t H, int32_t W, int32_t layout)
{
    if (layout != GSVC_FRAMES_YUV444P && layout != GSVC_FRAMES_YUV420P) return -1;
    return gsvc_frames_u8_bytes(H, W, layout);          // one float per sample
}

extern "C" int gsvc_frames_planes(const uint8_t *in, int64_t in_stride, int32_t n, int32_t H, int32_t W, int32_t layout, int32_t range,
                                  int32_t depth, float *const *planes_host, void *stream)
{
    const char *const who = "frames_planes";
    GSVC_REQUIRE(planes_host && in, "%s: NULL pointer", who);
    GSVC_REQUIRE(layout != GSVC_FRAMES_RGB24, "%s: rgb24 frames hold no Y'CbCr planes", who);
    GSVC_FRAMES_TRY(frames_check_format(who, n, GSVC_FRAMES_MAX_BATCH, layout, depth, 8, 16));
    GSVC_FRAMES_TRY(frames_check_colour(who, GSVC_FRAMES_BT709, range));
    GSVC_FRAMES_TRY(frames_check_size(who, H, W, layout));
    const bool deep = depth > 8;
    const FrameBufs bufs = {"in_stride", in, in_stride, nullptr, 0};
    if (deep) GSVC_FRAMES_TRY(frames_check_even(who, bufs));
    GSVC_FRAMES_TRY(frames_check_strides(who, bufs, gsvc_frames_bytes(H, W, layout, depth)));
    PlanesInArgs a;
    uintptr_t align = bufs.alignment(n);
    GSVC_FRAMES_TRY(frames_gather_images(who, planes_host, n, a.out, align));
    a.in = in;
    a.in_stride = in_stride;
    a.samples = gsvc_yuv_planes_floats(H, W, layout);
    a.luma = (long long)H * W;
    const FrameRange r = frames_range(range, depth);
    a.y_off = r.y_off;
    a.y_div = r.y_scale;
    a.c_off = r.c_off;
    a.c_div = r.c_scale;
    // the wide path: whole lanes of 4 samples, every base and stride 16-byte aligned.  The flat run is a multiple of 4 only when H W is
    // (4:4:4: 3 H W; 4:2:0: 6 (H W / 4) with H W a multiple of 4 already), so no lane straddles the luma / chroma boundary.
    const bool wide = a.samples % 4 == 0 && a.luma % 4 == 0 && (align & 15) == 0;
    const int64_t units = wide ? a.samples / 4 : a.samples;
    using Kernel = void (*)(PlanesInArgs);
    static const Kernel kernels[2][2] = {{k_frames_planes<1, false>, k_frames_planes<1, true>},
                                         {k_frames_planes<2, false>, k_frames_planes<2, true>}};          // [deep][wide]
    hipStream_t s = (hipStream_t)stream;
    ProfScope _p(deep ? "k_frames_planes16" : "k_frames_planes", s);
    hipLaunchKernelGGL(kernels[deep][wide], dim3((unsigned)((units + 255) / 256), (unsigned)n), dim3(256), 0, s, a);
    return check_launch(who);
}

extern "C" int gsvc_yuv_planes_forward(const float *img_f, const float *img_b, int32_t H, int32_t W, int32_t layout, int32_t matrix,
                                       float *planes_out, float *avg_out, void *stream)
{
    const char *const who = "yuv_planes_forward";
    GSVC_REQUIRE(img_f && planes_out, "%s: NULL pointer", who);
    YuvArgs a;
    GSVC_FRAMES_TRY(yuv_setup(who, H, W, layout, matrix, a));
    GSVC_FRAMES_TRY(yuv_pointer(who, "img_f", img_f));
    GSVC_FRAMES_TRY(yuv_pointer(who, "img_b", img_b));
    GSVC_FRAMES_TRY(yuv_pointer(who, "planes_out", planes_out));
    GSVC_FRAMES_TRY(yuv_pointer(who, "avg_out", avg_out));
    a.f = img_f;
    a.b = img_b;
    a.planes = planes_out;
    a.avg = avg_out;
    const uintptr_t align = reinterpret_cast<uintptr_t>(img_f) | reinterpret_cast<uintptr_t>(img_b) | reinterpret_cast<uintptr_t>(planes_out) |
                            reinterpret_cast<uintptr_t>(avg_out);
    const bool yuv420 = layout == GSVC_FRAMES_YUV420P;
    // the wide path: W % 4 == 0 keeps every float row, the planes behind Y (H W floats) and a lane's reversed load 16-byte aligned; the
    // 4:2:0 chroma rows (W / 2 floats) and Cr (H W / 4 floats behind Cb, H even) keep the 8 bytes of a float2
    const bool wide = W % 4 == 0 && H % 2 == 0 && (align & 15) == 0;
    const int64_t units = yuv_units(H, W, yuv420, wide);
    using Kernel = void (*)(YuvArgs);
    static const Kernel kernels[2][2] = {{k_yuv_planes_fwd<false, false>, k_yuv_planes_fwd<false, true>},
                                         {k_yuv_planes_fwd<true, false>, k_yuv_planes_fwd<true, true>}};          // [4:2:0][wide]
    hipStream_t s = (hipStream_t)stream;
    ProfScope _p("k_yuv_planes_fwd", s);
    hipLaunchKernelGGL(kernels[yuv420][wide], dim3((unsigned)((units + 255) / 256)), dim3(256), 0, s, a);
    return check_launch(who);
}

extern "C" int gsvc_yuv_planes_backward(const float *d_planes, int32_t H, int32_t W, int32_t layout, int32_t matrix, float *dL_dimg_f,
                                        float *dL_dimg_b, void *stream)
{
    const char *const who = "yuv_planes_backward";
    GSVC_REQUIRE(d_planes && dL_dimg_f, "%s: NULL pointer", who);
    YuvArgs a;
    GSVC_FRAMES_TRY(yuv_setup(who, H, W, layout, matrix, a));
    GSVC_FRAMES_TRY(yuv_pointer(who, "d_planes", d_planes));
    GSVC_FRAMES_TRY(yuv_pointer(who, "dL_dimg_f", dL_dimg_f));
    GSVC_FRAMES_TRY(yuv_pointer(who, "dL_dimg_b", dL_dimg_b));
    a.d_planes = d_planes;
    a.d_f = dL_dimg_f;
    a.d_b = dL_dimg_b;
    const uintptr_t align = reinterpret_cast<uintptr_t>(d_planes) | reinterpret_cast<uintptr_t>(dL_dimg_f) | reinterpret_cast<uintptr_t>(dL_dimg_b);
    const bool yuv420 = layout == GSVC_FRAMES_YUV420P;
    const bool wide = W % 4 == 0 && H % 2 == 0 && (align & 15) == 0;          // (as in the forward)
    const int64_t units = yuv_units(H, W, yuv420, wide);
    using Kernel = void (*)(YuvArgs);
    static const Kernel kernels[2][2] = {{k_yuv_planes_bwd<false, false>, k_yuv_planes_bwd<false, true>},
                                         {k_yuv_planes_bwd<true, false>, k_yuv_planes_bwd<true, true>}};          // [4:2:0][wide]
    hipStream_t s = (hipStream_t)stream;
    ProfScope _p("k_yuv_planes_bwd", s);
    hipLaunchKernelGGL(kernels[yuv420][wide], dim3((unsigned)((units + 255) / 256)), dim3(256), 0, s, a);
    return check_launch(who);
}
