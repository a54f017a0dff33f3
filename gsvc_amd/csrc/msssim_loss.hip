// gsvc_amd/csrc/msssim_loss.hip — MS-SSIM + L1 as a fitting loss (forward and backward), gfx950: the value of
// gsvc_amd.metrics.ms_ssim(x, y, data_range=1) per plane, the mean |x - y|, and the gradient of both with respect to x.
//
// forward   k_msl_scale per scale (the structure of k_msssim_scale, metrics.hip: 32x32 outputs of the VALID blur per workgroup, the
//           samples centred on one pixel of the tile) and k_msl_pool between scales; k_msl_means adds the tile sums of a
//           (scale, plane) in a fixed order in double, k_msl_value forms v = prod relu(t_s)^w_s per plane, the two scalars and, for the
//           backward, coef[s, p] = w_s v / (t_s n_s P).  Eleven launches, no float atomics, nothing synchronises.
//           Scale 0 also sums |x - y|: a tile OWNS the first 32 rows / columns of its 42 staged ones, the last tile of a row / column of
//           tiles owns all of them (the valid outputs stop 10 short of the picture's edge, the staged inputs do not).
// partials  a scale keeps three maps over its valid outputs q for the way back, as k_ssim_fwd does:
//             B = dM/dE[x^2],  C = dM/dE[xy],  A' = dM/dmu1 + 2 cx B + cy C          (M: the cs map, at scale 4 the SSIM map)
//           (cx, cy) the centre of the tile that wrote q, kept per tile.  dM/dmu1 alone is -(2 mu1 B + mu2 C) (+ the luminance part at
//           scale 4): of order 1 / C2, while what the backward needs is sum_q w(q - p) [dM/dmu1 + 2 x_p B + y_p C], a difference
//           (x_p - mu1) away from zero.  A' = -(2 (mu1 - cx) B + (mu2 - cy) C) is that small number itself, formed from the centred
//           means the forward already has.
// backward  k_msl_bwd, one launch per scale from 4 down to 0, a GATHER with one owner per input pixel p of the scale:
//             D_s(p) = g coef[s] [ Gt(A'') + 2 (x_p - bx) Gt(B) + (y_p - by) Gt(C) ](p) + 0.25 D_{s+1}((r + H%2) / 2, (c + W%2) / 2)
//           Gt = the tile blur over the maps extended by 10 zeros on every side (the window is symmetric), (bx, by) one pixel of the
//           backward tile, A'' = A' + 2 (bx - cx) B + (by - cy) C re-centred on load (all three terms small).  Scale 0 adds
//           g_l1 / (P H W) sign(x - y).  A plane with any t_s <= 0 has coef = 0: its blur is skipped and its gradient is exactly 0.
// pair form x = (img_f + flip_W(img_b)) / 2 is formed on load in the scale-0 kernels (k_ssim_fwd's img1b); d_f = D_0 / 2,
//           d_b = flip_W(d_f).
#include "common.h"
#include "msssim_layout.h"
#include "reduce.h"
#include "ssim_tile.h"

#include <cmath>

namespace gsvc {

// x of a scale: the picture itself, or with b != NULL (scale 0 of the pair form) the two-view frame
__device__ __forceinline__ float msl_x(const float *__restrict__ f, const float *__restrict__ b, size_t row, int gx, int W)
{
    const float xa = f[row + gx];
    return b ? (xa + b[row + (W - 1 - gx)]) / 2.0f : xa;
}

struct MslMaps {
    float *a, *b, *c;                  // [P, H - 10, W - 10] each; a == NULL: not kept
};

// one scale.  partials[plane * tiles + tile] = the sum over the tile's valid outputs of the cs map (last = 0) or the SSIM map
// (last = 1), centres[..] = the tile's centre; l1_partials (scale 0) = the tile's owned sum of |x - y|
__global__ void __launch_bounds__(256) k_msl_scale(SsimWindow win_s, const float *__restrict__ xf, const float *__restrict__ xb,
                                                   const float *__restrict__ yy, int H, int W, int last, float *__restrict__ avg_out,
                                                   double *__restrict__ partials, double *__restrict__ l1_partials,
                                                   float2 *__restrict__ centres, MslMaps maps)
{
    __shared__ __attribute__((aligned(16))) float st[2][ST_HALO][ST_LD];   // the staged pictures: x, y
    __shared__ float hb[5][ST_HALO][ST_HLD];
    __shared__ double red[4];
    const SsimWindow win = window_in_vgprs(win_s);
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * ST_TILE, y0 = blockIdx.y * ST_TILE;
    const int Hv = H - (ST_TAPS - 1), Wv = W - (ST_TAPS - 1);       // the valid outputs
    const size_t plane = (size_t)blockIdx.z * H * W;
    const size_t tile = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    // the 42x42 inputs of the tile's valid outputs, zero past the picture
    float v[ST_LOADS][2];
#pragma unroll
    for (int it = 0; it < ST_LOADS; it++) {
        int r, c;
        const bool live = tile_slot(it, r, c);
        const int gy = y0 + r, gx = x0 + c;
        const bool in = live && gy < H && gx < W;
        v[it][0] = in ? msl_x(xf, xb, plane + (size_t)gy * W, gx, W) : 0.f;
        v[it][1] = in ? yy[plane + (size_t)gy * W + gx] : 0.f;
    }
    store_tile(st, v);
    if (l1_partials) {
        const bool last_row = blockIdx.y == gridDim.y - 1, last_col = blockIdx.x == gridDim.x - 1;
        float l1 = 0.f;
#pragma unroll
        for (int it = 0; it < ST_LOADS; it++) {
            int r, c;
            const bool live = tile_slot(it, r, c);
            const int gy = y0 + r, gx = x0 + c;
            if (live && gy < H && gx < W && (r < ST_TILE || last_row) && (c < ST_TILE || last_col)) {
                l1 += fabsf(v[it][0] - v[it][1]);
                if (avg_out) avg_out[plane + (size_t)gy * W + gx] = v[it][0];
            }
        }
        const double total = block_sum_256<SumOrder::Pairs>((double)l1, red);
        if (tid == 0) l1_partials[tile] = total;
    }
    __syncthreads();
    // the centre of the staged part of the picture: one pixel of each picture, the same for the whole workgroup
    const int rc = min(ST_HALO / 2, H - 1 - y0), cc = min(ST_HALO / 2, W - 1 - x0);
    const float cx = st[0][rc][cc], cy = st[1][rc][cc];
    // horizontal pass: group g = (row r, outputs 4 cg .. 4 cg + 3 <- columns 4 cg .. 4 cg + 13)
    for (int g = tid; g < ST_GROUPS; g += 256) {
        const int r = g >> 3, c0 = 4 * (g & 7);
        if (y0 + r >= H || x0 + c0 >= Wv) continue;      // a row below the picture, outputs right of the last valid one
        float xv[16], yv[16];
        staged_row16(st[0], r, c0, xv);
        staged_row16(st[1], r, c0, yv);
#pragma unroll
        for (int k = 0; k < 16; k++) { xv[k] -= cx; yv[k] -= cy; }
        blur4_moments(win, xv, yv, hb, r, c0);
    }
    __syncthreads();
    // vertical pass: thread = (column lx, outputs 4 gq .. 4 gq + 3 <- rows 4 gq .. 4 gq + 13)
    const int lx = tid & 31, gq = tid >> 5;
    const int gx = x0 + lx;
    float sum = 0.f;
    if (gx < Wv && y0 + 4 * gq < Hv) {
        float mom[5][4];
#pragma unroll
        for (int m = 0; m < 5; m++) blur4_column(win, hb[m], 4 * gq, lx, mom[m]);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int gy = y0 + 4 * gq + j;
            if (gy < Hv) {                       // (rows of hb below the picture were not written: their outputs are not taken)
                const float m1 = mom[0][j], m2 = mom[1][j];
                const float s1 = mom[2][j] - m1 * m1, s2 = mom[3][j] - m2 * m2, s12 = mom[4][j] - m1 * m2;
                const float den = s1 + s2 + SSIM_C2;
                const float cs = (2.f * s12 + SSIM_C2) / den;
                float val = cs;
                float pb = -cs / den, pc = 2.f / den;
                float pa = -(2.f * m1 * pb + m2 * pc);
                if (last) {
                    const float mu1 = m1 + cx, mu2 = m2 + cy;
                    const float la = mu1 * mu1 + mu2 * mu2 + SSIM_C1;
                    const float lum = (2.f * mu1 * mu2 + SSIM_C1) / la;
                    const float dlum = 2.f * (mu2 - lum * mu1) / la;
                    val = lum * cs;
                    pa = cs * dlum + lum * pa;
                    pb *= lum;
                    pc *= lum;
                }
                sum += val;
                if (maps.a) {
                    const size_t o = ((size_t)blockIdx.z * Hv + gy) * Wv + gx;
                    maps.a[o] = pa;
                    maps.b[o] = pb;
                    maps.c[o] = pc;
                }
            }
        }
    }
    const double total = block_sum_256<SumOrder::Pairs>((double)sum, red);
    if (tid == 0) {
        partials[tile] = total;
        centres[tile] = make_float2(cx, cy);
    }
}

// 2x2 mean of both pictures, as k_msssim_pool (metrics.hip): a leading zero row / column on an odd side, the divisor stays 4, the sum
// runs row by row
__global__ void __launch_bounds__(256) k_msl_pool(const float *__restrict__ xf, const float *__restrict__ xb, const float *__restrict__ yy,
                                                  int H, int W, int H2, int W2, float *__restrict__ out_x, float *__restrict__ out_y)
{
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= H2 * W2) return;
    const int i = o / W2, j = o - i * W2;
    const int r0 = 2 * i - (H & 1), c0 = 2 * j - (W & 1);
    const size_t plane = (size_t)blockIdx.y * H * W;
    float sx = 0.f, sy = 0.f;
#pragma unroll
    for (int dr = 0; dr < 2; dr++)
#pragma unroll
        for (int dc = 0; dc < 2; dc++) {
            const int r = r0 + dr, c = c0 + dc;
            const bool in = r >= 0 && c >= 0;            // (r <= H - 1 and c <= W - 1 by construction)
            sx += in ? msl_x(xf, xb, plane + (size_t)r * W, c, W) : 0.f;
            sy += in ? yy[plane + (size_t)r * W + c] : 0.f;
        }
    const size_t at = (size_t)blockIdx.y * ((size_t)H2 * W2) + o;
    out_x[at] = 0.25f * sx;
    out_y[at] = 0.25f * sy;
}

// the sum of n doubles in a fixed order, in all threads' view of red[0]: lane t takes t, t + 256, ... in rising order, then a tree
// over the 256 lanes whose shape does not depend on anything
__device__ __forceinline__ double msl_ordered_sum(const double *__restrict__ p, long long n, double *red)
{
    double a = 0.0;
    for (long long i = threadIdx.x; i < n; i += 256) a += p[i];
    __syncthreads();
    red[threadIdx.x] = a;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
        __syncthreads();
    }
    return red[0];
}

struct MslFinalize {
    long long offset[MS_SCALES];       // first partial of a scale
    int tiles[MS_SCALES];              // tiles of one plane
    double inv_count[MS_SCALES];       // 1 / valid outputs of one plane
    double weight[MS_SCALES];
};

// means[scale, plane] = the plane's tile sums / outputs
__global__ void __launch_bounds__(256) k_msl_means(MslFinalize f, const double *__restrict__ partials, int P, double *__restrict__ means)
{
    __shared__ double red[256];
    const int plane = blockIdx.x, scale = blockIdx.y, n = f.tiles[scale];
    const double t = msl_ordered_sum(partials + f.offset[scale] + (size_t)plane * n, n, red);
    if (threadIdx.x == 0) means[(size_t)scale * P + plane] = t * f.inv_count[scale];
}

// out[0] = mean over planes of prod_s relu(t_s)^w_s (the factors multiplied one after the other, in double), out[1] = the L1 tile
// sums / samples; coef[s, p] = d out[0] / d t_s / n_s, zero for every scale of a plane with a t_s <= 0
__global__ void __launch_bounds__(256) k_msl_value(MslFinalize f, const double *__restrict__ means, int P,
                                                   const double *__restrict__ l1_partials, long long l1_tiles, double inv_samples,
                                                   double *__restrict__ values, float *__restrict__ coef, float *__restrict__ out)
{
    __shared__ double red[256];
    for (int p = threadIdx.x; p < P; p += 256) {
        double t[MS_SCALES], v = 1.0;
        bool clipped = false;
#pragma unroll
        for (int s = 0; s < MS_SCALES; s++) {
            t[s] = means[(size_t)s * P + p];
            clipped = clipped || !(t[s] > 0.0);
            const double fac = pow(fmax(t[s], 0.0), f.weight[s]);
            v = s == 0 ? fac : v * fac;
        }
        if (clipped) v = 0.0;
        values[p] = v;
#pragma unroll
        for (int s = 0; s < MS_SCALES; s++)
            coef[(size_t)s * P + p] = clipped ? 0.f : (float)(f.weight[s] * v / t[s] * f.inv_count[s] / (double)P);
    }
    __syncthreads();
    const double vs = msl_ordered_sum(values, P, red);
    const double ls = msl_ordered_sum(l1_partials, l1_tiles, red);
    if (threadIdx.x == 0) {
        out[0] = (float)(vs / (double)P);
        out[1] = (float)(ls * inv_samples);
    }
}

// the gradient of one scale (the formula at the head of the file).  d_next: D of the scale below (H2 x W2), NULL at scale 4;
// l1_samples > 0 (scale 0): add grads[1] / l1_samples * sign(x - y); out_b != NULL: the pair form's two images
__global__ void __launch_bounds__(256) k_msl_bwd(SsimWindow win_s, const float *__restrict__ xf, const float *__restrict__ xb,
                                                 const float *__restrict__ yy, int H, int W, MslMaps maps,
                                                 const float2 *__restrict__ centres, int tiles_x, int tiles_y,
                                                 const float *__restrict__ coef, const float *__restrict__ grads,
                                                 const float *__restrict__ d_next, int H2, int W2, float l1_samples,
                                                 float *__restrict__ out, float *__restrict__ out_b)
{
    __shared__ __attribute__((aligned(16))) float sm[3][ST_HALO][ST_LD];
    __shared__ float hb[3][ST_HALO][ST_HLD];
    const SsimWindow win = window_in_vgprs(win_s);
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * ST_TILE, y0 = blockIdx.y * ST_TILE;
    const int Hv = H - (ST_TAPS - 1), Wv = W - (ST_TAPS - 1);
    const size_t plane = (size_t)blockIdx.z * H * W;
    const float cf = coef[blockIdx.z];
    const int lx = tid & 31, gq = tid >> 5;
    // the centre of this tile of input pixels
    const int rb = min(y0 + ST_TILE / 2, H - 1), cb = min(x0 + ST_TILE / 2, W - 1);
    const float bx = msl_x(xf, xb, plane + (size_t)rb * W, cb, W), by = yy[plane + (size_t)rb * W + cb];
    float bl[3][4] = {};
    if (cf != 0.f) {                                     // (the same for the whole workgroup)
        // the maps at the outputs q = p - 10 .. p, zero outside the valid outputs, re-centred on (bx, by)
        float ma[ST_LOADS][3];
#pragma unroll
        for (int it = 0; it < ST_LOADS; it++) {
            int r, c;
            const bool live = tile_slot(it, r, c);
            const int qy = y0 + r - (ST_TAPS - 1), qx = x0 + c - (ST_TAPS - 1);
            const bool in = live && qy >= 0 && qy < Hv && qx >= 0 && qx < Wv;
            const size_t o = ((size_t)blockIdx.z * Hv + qy) * Wv + qx;
            const float a = in ? maps.a[o] : 0.f, b = in ? maps.b[o] : 0.f, c2 = in ? maps.c[o] : 0.f;
            const float2 cen = in ? centres[((size_t)blockIdx.z * tiles_y + (qy >> 5)) * tiles_x + (qx >> 5)] : make_float2(bx, by);
            ma[it][0] = fmaf(2.f * (bx - cen.x), b, fmaf(by - cen.y, c2, a));
            ma[it][1] = b;
            ma[it][2] = c2;
        }
        store_tile(sm, ma);
        __syncthreads();
        for (int g = tid; g < ST_GROUPS; g += 256) {
            const int r = g >> 3, c0 = 4 * (g & 7);
#pragma unroll
            for (int m = 0; m < 3; m++) {
                float v[16], o4[4];
                staged_row16(sm[m], r, c0, v);
                blur4(win, v, o4);
#pragma unroll
                for (int j = 0; j < 4; j++) hb[m][r][c0 + j] = o4[j];
            }
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 3; m++) blur4_column(win, hb[m], 4 * gq, lx, bl[m]);
    }
    const int gx = x0 + lx;
    const float k = grads[0] * cf;
    const float gl = l1_samples > 0.f ? grads[1] / l1_samples : 0.f;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int gy = y0 + 4 * gq + j;
        if (gx < W && gy < H) {
            const size_t row = plane + (size_t)gy * W;
            const float x = msl_x(xf, xb, row, gx, W), y = yy[row + gx];
            float v = k * (bl[0][j] + 2.f * (x - bx) * bl[1][j] + (y - by) * bl[2][j]);
            if (d_next) v += 0.25f * d_next[((size_t)blockIdx.z * H2 + ((gy + (H & 1)) >> 1)) * W2 + ((gx + (W & 1)) >> 1)];
            if (l1_samples > 0.f) {
                const float d = x - y;
                const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
                v = fmaf(gl, sgn, v);
            }
            if (out_b) {
                out[row + gx] = 0.5f * v;
                out_b[row + (W - 1 - gx)] = 0.5f * v;
            } else {
                out[row + gx] = v;
            }
        }
    }
}

// the loss's workspace: the pooled pictures of ms_layout, then what the backward reads
struct MslLayout {
    MsLayout ms;
    int64_t valid[MS_SCALES];          // valid outputs of one plane
    int64_t maps[MS_SCALES];           // byte offset of a scale's three maps, [3, P, valid]
    int64_t grad[MS_SCALES];           // byte offset of D_s [P, h, w], s >= 1
    int64_t partials, l1, centres, means, values, coef;
    int64_t parts;                     // tiles of all scales and planes
    int64_t bytes;
};

static MslLayout msl_layout(int32_t P, int32_t H, int32_t W)
{
    MslLayout L;
    L.ms = ms_layout(P, H, W);
    int64_t at = L.ms.partials;        // the end of the pooled pictures
    auto take = [&at](uint64_t bytes) {
        const int64_t here = at;
        at += (int64_t)align_up(bytes, 256);
        return here;
    };
    L.parts = L.ms.part_off[MS_SCALES - 1] + (int64_t)P * L.ms.tx[MS_SCALES - 1] * L.ms.ty[MS_SCALES - 1];
    for (int s = 0; s < MS_SCALES; s++) {
        L.valid[s] = (int64_t)(L.ms.h[s] - (ST_TAPS - 1)) * (L.ms.w[s] - (ST_TAPS - 1));
        L.maps[s] = take((uint64_t)3 * P * L.valid[s] * sizeof(float));
        L.grad[s] = s > 0 ? take((uint64_t)P * L.ms.h[s] * L.ms.w[s] * sizeof(float)) : 0;
    }
    L.partials = take((uint64_t)L.parts * sizeof(double));
    L.l1 = take((uint64_t)P * L.ms.tx[0] * L.ms.ty[0] * sizeof(double));
    L.centres = take((uint64_t)L.parts * sizeof(float2));
    L.means = take((uint64_t)MS_SCALES * P * sizeof(double));
    L.values = take((uint64_t)P * sizeof(double));
    L.coef = take((uint64_t)MS_SCALES * P * sizeof(float));
    L.bytes = at;
    return L;
}

static MslMaps msl_maps(uint8_t *ws, const MslLayout &L, int32_t P, int s)
{
    float *m = reinterpret_cast<float *>(ws + L.maps[s]);
    const size_t n = (size_t)P * L.valid[s];
    return MslMaps{m, m + n, m + 2 * n};
}

// the checks both entries share, before any GPU call
static int msl_check(const char *who, const void *img, const void *gt, const void *img_b, const void *extra, int32_t P, int32_t H,
                     int32_t W, const void *workspace)
{
    GSVC_REQUIRE(img && gt && workspace, "%s: NULL pointer", who);
    GSVC_REQUIRE(P >= 1 && P <= 65535, "%s: P must be 1 .. 65535 (got %d)", who, (int)P);
    GSVC_REQUIRE(H >= 1 && W >= 1 && H <= 32768 && W <= 32768, "%s: image size must be 1 .. 32768 (got %d x %d)", who, (int)H, (int)W);
    GSVC_REQUIRE(H > 160 && W > 160, "%s: image sides must exceed 160 pixels for 5 scales (got %d x %d)", who, (int)H, (int)W);
    const uintptr_t bases = reinterpret_cast<uintptr_t>(img) | reinterpret_cast<uintptr_t>(gt) | reinterpret_cast<uintptr_t>(img_b) |
                            reinterpret_cast<uintptr_t>(extra);
    GSVC_REQUIRE((bases & 3) == 0, "%s: an image is not 4-byte aligned", who);
    GSVC_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "%s: the workspace must be 16-byte aligned", who);
    return GSVC_OK;
}

}  // namespace gsvc

using namespace gsvc;

extern "C" int64_t gsvc_msssim_loss_workspace_bytes(int32_t P, int32_t H, int32_t W)
{
    if (!ms_shape_ok(P, H, W)) return -1;
    return msl_layout(P, H, W).bytes;
}

extern "C" int gsvc_msssim_loss_forward(const float *img, const float *img_b, const float *gt, int32_t P, int32_t H, int32_t W,
                                        int32_t keep_maps, void *workspace, float *out, float *avg_out, void *stream)
{
    static const char *who = "msssim_loss_forward";
    const int rc = msl_check(who, img, gt, img_b, avg_out, P, H, W, workspace);
    if (rc != GSVC_OK) return rc;
    GSVC_REQUIRE(out, "%s: NULL pointer", who);
    GSVC_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3) == 0, "%s: out is not 4-byte aligned", who);
    GSVC_REQUIRE(img_b || !avg_out, "%s: avg_out without img_b", who);
    const MslLayout L = msl_layout(P, H, W);
    static const SsimWindow win = make_msssim_window();
    hipStream_t s = (hipStream_t)stream;
    uint8_t *ws = reinterpret_cast<uint8_t *>(workspace);
    double *partials = reinterpret_cast<double *>(ws + L.partials);
    float2 *centres = reinterpret_cast<float2 *>(ws + L.centres);
    const float *x = img, *xb = img_b, *y = gt;
    for (int k = 0; k < MS_SCALES; k++) {
        const int h = L.ms.h[k], w = L.ms.w[k];
        const MslMaps maps = keep_maps ? msl_maps(ws, L, P, k) : MslMaps{nullptr, nullptr, nullptr};
        {
            ProfScope _p("k_msl_scale", s);
            hipLaunchKernelGGL(k_msl_scale, dim3(L.ms.tx[k], L.ms.ty[k], P), dim3(256), 0, s, win, x, xb, y, h, w,
                               k == MS_SCALES - 1 ? 1 : 0, k == 0 ? avg_out : nullptr, partials + L.ms.part_off[k],
                               k == 0 ? reinterpret_cast<double *>(ws + L.l1) : nullptr, centres + L.ms.part_off[k], maps);
        }
        if (k + 1 < MS_SCALES) {
            ProfScope _p("k_msl_pool", s);
            const int outs = L.ms.h[k + 1] * L.ms.w[k + 1];
            float *nx = reinterpret_cast<float *>(ws + L.ms.pyr[k + 1]);
            hipLaunchKernelGGL(k_msl_pool, dim3((outs + 255) / 256, P), dim3(256), 0, s, x, xb, y, h, w, L.ms.h[k + 1], L.ms.w[k + 1], nx,
                               nx + (size_t)P * outs);
            x = nx;
            xb = nullptr;
            y = nx + (size_t)P * outs;
        }
    }
    MslFinalize f;
    static const double weights[MS_SCALES] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
    for (int k = 0; k < MS_SCALES; k++) {
        f.offset[k] = L.ms.part_off[k];
        f.tiles[k] = L.ms.tx[k] * L.ms.ty[k];
        f.inv_count[k] = 1.0 / (double)L.valid[k];
        f.weight[k] = weights[k];
    }
    double *means = reinterpret_cast<double *>(ws + L.means);
    {
        ProfScope _p("k_msl_means", s);
        hipLaunchKernelGGL(k_msl_means, dim3(P, MS_SCALES), dim3(256), 0, s, f, partials, P, means);
    }
    {
        ProfScope _p("k_msl_value", s);
        hipLaunchKernelGGL(k_msl_value, dim3(1), dim3(256), 0, s, f, means, P, reinterpret_cast<const double *>(ws + L.l1),
                           (long long)P * f.tiles[0], 1.0 / ((double)P * (double)H * (double)W), reinterpret_cast<double *>(ws + L.values),
                           reinterpret_cast<float *>(ws + L.coef), out);
    }
    return check_launch(who);
}

extern "C" int gsvc_msssim_loss_backward(const float *img, const float *img_b, const float *gt, int32_t P, int32_t H, int32_t W,
                                         void *workspace, const float *grads, float *d_img, float *d_img_b, void *stream)
{
    static const char *who = "msssim_loss_backward";
    const int rc = msl_check(who, img, gt, img_b, d_img_b, P, H, W, workspace);
    if (rc != GSVC_OK) return rc;
    GSVC_REQUIRE(grads && d_img, "%s: NULL pointer", who);
    GSVC_REQUIRE(((reinterpret_cast<uintptr_t>(grads) | reinterpret_cast<uintptr_t>(d_img)) & 3) == 0, "%s: an image is not 4-byte aligned",
                 who);
    GSVC_REQUIRE((img_b != nullptr) == (d_img_b != nullptr), "%s: img_b and d_img_b go together", who);
    const MslLayout L = msl_layout(P, H, W);
    static const SsimWindow win = make_msssim_window();
    hipStream_t s = (hipStream_t)stream;
    // (the forward's regions are only read; the gradients of scales 1 .. 4 are this call's scratch in the same workspace)
    uint8_t *ws = reinterpret_cast<uint8_t *>(workspace);
    const float2 *centres = reinterpret_cast<const float2 *>(ws + L.centres);
    const float *coef = reinterpret_cast<const float *>(ws + L.coef);
    for (int k = MS_SCALES - 1; k >= 0; k--) {
        const int h = L.ms.h[k], w = L.ms.w[k];
        const float *x = img, *xb = img_b, *y = gt;
        if (k > 0) {
            x = reinterpret_cast<const float *>(ws + L.ms.pyr[k]);
            xb = nullptr;
            y = x + (size_t)P * h * w;
        }
        const float *d_next = k + 1 < MS_SCALES ? reinterpret_cast<const float *>(ws + L.grad[k + 1]) : nullptr;
        const int h2 = k + 1 < MS_SCALES ? L.ms.h[k + 1] : 0, w2 = k + 1 < MS_SCALES ? L.ms.w[k + 1] : 0;
        ProfScope _p("k_msl_bwd", s);
        hipLaunchKernelGGL(k_msl_bwd, dim3((w + ST_TILE - 1) / ST_TILE, (h + ST_TILE - 1) / ST_TILE, P), dim3(256), 0, s, win, x, xb, y, h,
                           w, msl_maps(ws, L, P, k), centres + L.ms.part_off[k], L.ms.tx[k], L.ms.ty[k], coef + (size_t)k * P, grads,
                           d_next, h2, w2, k == 0 ? (float)P * (float)H * (float)W : 0.f,
                           k == 0 ? d_img : reinterpret_cast<float *>(ws + L.grad[k]), k == 0 ? d_img_b : nullptr);
    }
    return check_launch(who);
}
