// gsvc_amd/csrc/wdist.hip — spatially weighted distortion, gfx950: the fused SSIM + L1 loss of ssim.hip with a weight
// per cell of cell x cell pixels (a region of interest, activity-adaptive weighting: gsvc_amd/wdist.py), forward and backward, single image
// and two-view pair; and the per-cell luma SSE of two buffers of delivered frames, which a weighted PSNR is formed from.
//
//   forward   k_ssim_fwd's tile, window, zero padding, moments and SSIM map.  Pixel (y, x) of every channel has the weight
//             w[y / cell][x / cell]; sums[0] = sum w ssim, sums[1] = sum w |x - gt|, and the three partial maps leave the kernel already
//             multiplied by the pixel's weight.
//   backward  the blur of those maps combined with x, y: k_ssim_bwd's arithmetic unchanged (the weight is a constant factor of the map at
//             the pixel, so d(sum w map)/d(moments) = w d(map)/d(moments): it enters where the partials are stored and nowhere else);
//             the L1 part is ((grads[1] inv_count) w) sign(x - y).
//   sums      NO float atomics: workgroup b writes its two partial sums to row b of the workspace (2 floats per tile), and
//             k_wssim_finalize adds the rows in a fixed order, in double: the same bits in every run for any number of tiles.
//   weights   straight from the cache, one load per thread and pass: tiles start at multiples of 32 and cell divides 32, so a tile
//             touches at most 8 x 8 weights, and a thread's four vertical outputs (rows 4 gq .. 4 gq + 3) lie in one cell.  The load is
//             issued before the tile is staged; its latency is covered by both blur passes (DESIGN section 8o has the choice against LDS).
//
// ssim.hip is untouched: these kernels stand beside it and share ssim_tile.h / reduce.h with it.
#include "frames_common.h"
#include "reduce.h"
#include "ssim_tile.h"

namespace gsvc {

struct CellWeights {
    const float *w;      // [Hc][Wc]
    int shift;           // log2(cell)
    int Wc;
};

// the weight of the thread's outputs (column gx, rows gy0 .. gy0 + 3 of one cell); 0 for a thread that owns no pixel (never used)
__device__ __forceinline__ float weight_of(const CellWeights &cw, int gx, int gy0, int H, int W)
{
    return (gx < W && gy0 < H) ? cw.w[(size_t)(gy0 >> cw.shift) * cw.Wc + (gx >> cw.shift)] : 0.f;
}

__global__ void __launch_bounds__(256) k_wssim_fwd(SsimWindow win_s, const float *__restrict__ img1, const float *__restrict__ img1b,
                                                   float *__restrict__ avg_out, const float *__restrict__ img2, CellWeights cw, int H, int W,
                                                   float *__restrict__ partials /* [tiles][2]: w ssim, w l1 */,
                                                   float *__restrict__ dm_dmu1, float *__restrict__ dm_de11, float *__restrict__ dm_de12)
{
    __shared__ __attribute__((aligned(16))) float st[2][ST_HALO][ST_LD];   // the staged images: x, y
    __shared__ float hb[5][ST_HALO][ST_HLD];  // horizontally blurred moments
    __shared__ float red[4];
    const SsimWindow win = window_in_vgprs(win_s);
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * ST_TILE, y0 = blockIdx.y * ST_TILE;
    const size_t plane = (size_t)blockIdx.z * H * W;
    const int lx = tid & 31, gq = tid >> 5;
    const int gx = x0 + lx;
    const float wt = weight_of(cw, gx, y0 + 4 * gq, H, W);
    float v[ST_LOADS][2];
#pragma unroll
    for (int it = 0; it < ST_LOADS; it++) {
        int r, c;
        const bool live = tile_slot(it, r, c);
        const int gy = y0 + r - ST_R, gxx = x0 + c - ST_R;
        const bool in = live && gy >= 0 && gy < H && gxx >= 0 && gxx < W;
        const float xa = in ? img1[plane + (size_t)gy * W + gxx] : 0.f;
        const float xb = (img1b && in) ? img1b[plane + (size_t)gy * W + (W - 1 - gxx)] : 0.f;
        v[it][0] = img1b ? (xa + xb) / 2.0f : xa;
        v[it][1] = in ? img2[plane + (size_t)gy * W + gxx] : 0.f;
    }
    store_tile(st, v);
    __syncthreads();
    for (int g = tid; g < ST_GROUPS; g += 256) {
        const int r = g >> 3, c0 = 4 * (g & 7);
        float xv[16], yv[16];
        staged_row16(st[0], r, c0, xv);
        staged_row16(st[1], r, c0, yv);
        blur4_moments(win, xv, yv, hb, r, c0);
    }
    __syncthreads();
    float mom[5][4];
#pragma unroll
    for (int m = 0; m < 5; m++) blur4_column(win, hb[m], 4 * gq, lx, mom[m]);
    float ssim_sum = 0.f, l1_sum = 0.f;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int ly = 4 * gq + j, gy = y0 + ly;
        if (gx < W && gy < H) {
            const float mu1 = mom[0][j], mu2 = mom[1][j], e11 = mom[2][j], e22 = mom[3][j], e12 = mom[4][j];
            const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
            const float s1 = e11 - mu1_sq, s2 = e22 - mu2_sq, s12 = e12 - mu12;
            const float num1 = 2.f * mu12 + SSIM_C1, num2 = 2.f * s12 + SSIM_C2;
            const float A = mu1_sq + mu2_sq + SSIM_C1, B = s1 + s2 + SSIM_C2;
            const float inv = 1.0f / (A * B);
            const float ssim = num1 * num2 * inv;
            const float xc = st[0][ly + ST_R][lx + ST_R], yc = st[1][ly + ST_R][lx + ST_R];
            // said explicitly, so that the sums do not depend on what the compiler fuses around them
            ssim_sum = fmaf(wt, ssim, ssim_sum);
            l1_sum = fmaf(wt, fabsf(xc - yc), l1_sum);
            const size_t o = plane + (size_t)gy * W + gx;
            if (avg_out) avg_out[o] = xc;
            if (dm_dmu1) {
                dm_dmu1[o] = wt * (2.f * mu2 * (num2 - num1) * inv - 2.f * mu1 * ssim * (1.0f / A - 1.0f / B));
                dm_de11[o] = wt * (-ssim / B);
                dm_de12[o] = wt * (2.f * num1 * inv);
            }
        }
    }
    const float ssum = block_sum_256<SumOrder::Chain>(ssim_sum, red);
    const float lsum = block_sum_256<SumOrder::Chain>(l1_sum, red);
    if (tid == 0) {
        // this workgroup's own row: a plain store, every row of the workspace is written once per call
        const size_t row = blockIdx.x + (size_t)gridDim.x * (blockIdx.y + (size_t)gridDim.y * blockIdx.z);
        partials[2 * row + 0] = ssum;
        partials[2 * row + 1] = lsum;
    }
}

// the rows in a fixed order: thread t adds rows t, t + 256, .. in double, then the workgroup's fixed tree
__global__ void __launch_bounds__(256) k_wssim_finalize(const float *__restrict__ partials, long long rows, float *__restrict__ sums)
{
    __shared__ double red[4];
    double a = 0.0, b = 0.0;
    for (long long i = threadIdx.x; i < rows; i += 256) { a += (double)partials[2 * i]; b += (double)partials[2 * i + 1]; }
    a = block_sum_256<SumOrder::Chain>(a, red);
    b = block_sum_256<SumOrder::Chain>(b, red);
    if (threadIdx.x == 0) { sums[0] = (float)a; sums[1] = (float)b; }
}

// dL/dimg1 = conv(g wm_dmu1) + 2 x conv(g wm_de11) + y conv(g wm_de12) + (g_l1 w) sign(x - y): the maps carry the weights already
__global__ void __launch_bounds__(256) k_wssim_bwd(SsimWindow win_s, const float *__restrict__ img1, const float *__restrict__ img1b,
                                                   float *__restrict__ dL_dimg1b, const float *__restrict__ img2, CellWeights cw, int H, int W,
                                                   float inv_count, const float *__restrict__ grads, const float *__restrict__ dm_dmu1,
                                                   const float *__restrict__ dm_de11, const float *__restrict__ dm_de12,
                                                   float *__restrict__ dL_dimg1)
{
    __shared__ __attribute__((aligned(16))) float sm[3][ST_HALO][ST_LD];
    __shared__ float hb[3][ST_HALO][ST_HLD];
    const SsimWindow win = window_in_vgprs(win_s);
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * ST_TILE, y0 = blockIdx.y * ST_TILE;
    const size_t plane = (size_t)blockIdx.z * H * W;
    const int lx = tid & 31, gq = tid >> 5;
    const int gx = x0 + lx;
    const float wt = weight_of(cw, gx, y0 + 4 * gq, H, W);
    float ma[ST_LOADS][3];
#pragma unroll
    for (int it = 0; it < ST_LOADS; it++) {          // all loads first (ssim_tile.h)
        int r, c;
        const bool live = tile_slot(it, r, c);
        const int gy = y0 + r - ST_R, gxx = x0 + c - ST_R;
        const bool in = live && gy >= 0 && gy < H && gxx >= 0 && gxx < W;
        const size_t o = plane + (size_t)gy * W + gxx;
        ma[it][0] = in ? dm_dmu1[o] : 0.f;
        ma[it][1] = in ? dm_de11[o] : 0.f;
        ma[it][2] = in ? dm_de12[o] : 0.f;
    }
    store_tile(sm, ma);
    __syncthreads();
    for (int g = tid; g < ST_GROUPS; g += 256) {
        const int r = g >> 3, c0 = 4 * (g & 7);
#pragma unroll
        for (int m = 0; m < 3; m++) {
            float v[16], out[4];
            staged_row16(sm[m], r, c0, v);
            blur4(win, v, out);
#pragma unroll
            for (int j = 0; j < 4; j++) hb[m][r][c0 + j] = out[j];
        }
    }
    __syncthreads();
    float bl[3][4];
#pragma unroll
    for (int m = 0; m < 3; m++) blur4_column(win, hb[m], 4 * gq, lx, bl[m]);
    const float g = grads[0] * inv_count, gl = (grads[1] * inv_count) * wt;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int gy = y0 + 4 * gq + j;
        if (gx < W && gy < H) {
            const size_t o = plane + (size_t)gy * W + gx;
            const size_t ob = plane + (size_t)gy * W + (W - 1 - gx);
            float x = img1[o];
            if (img1b) x = (x + img1b[ob]) / 2.0f;
            const float y = img2[o];
            const float d = x - y;
            const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
            // the L1 term joins the ROUNDED SSIM term in one fma, as in k_ssim_bwd
            const float v = fmaf(gl, sgn, g * (bl[0][j] + 2.f * x * bl[1][j] + y * bl[2][j]));
            if (img1b) {
                dL_dimg1[o] = 0.5f * v;
                dL_dimg1b[ob] = 0.5f * v;
            } else {
                dL_dimg1[o] = v;
            }
        }
    }
}

// ---- per-cell luma SSE ----------------------------------------------------------------------------------------------------------------
// out[f, cy, cx] = sum over the pixels of cell (cy, cx) of (a - b)^2 on the luma codes.  A workgroup of 256 owns 128 x 32 pixels = whole
// cells for every cell size, a lane the 4 x 4 block (bx, by); a cell of 8 or 16 is the sum of 2 x 2 or 4 x 4 block sums through LDS.  Every
// output is written once by a plain store.  Width of the sums: a squared difference of 16-bit codes is at most 65535^2 < 2^32, a cell has at
// most 16 x 16 = 2^8 pixels: every sum is below 2^40.
constexpr int BS_W = 128, BS_H = 32, BS_BX = BS_W / 4, BS_BY = BS_H / 4;
static_assert(BS_BX * BS_BY == 256, "one 4 x 4 block per lane");

struct BlockSseArgs {
    const uint8_t *a, *b;
    long long stride;
    long long *out;          // [n, Hc, Wc]
    int H, W, cell, Hc, Wc;
};

// WIDE: the four samples of a block's row as one load of 4 BPS bytes (bases, stride and W BPS allow it, and W % 4 == 0: the row lies
// wholly inside the picture)
template <int BPS, bool WIDE>
__global__ void __launch_bounds__(256) k_frames_block_sse(BlockSseArgs args)
{
    __shared__ unsigned long long blk[BS_BY][BS_BX];
    const int H = args.H, W = args.W;
    const int f = blockIdx.z, x0 = blockIdx.x * BS_W, y0 = blockIdx.y * BS_H;
    const uint8_t *pa = args.a + (size_t)f * (size_t)args.stride, *pb = args.b + (size_t)f * (size_t)args.stride;
    const int bx = threadIdx.x % BS_BX, by = threadIdx.x / BS_BX;
    const int px = x0 + 4 * bx, py = y0 + 4 * by;
    unsigned long long sum = 0;
    if (px < W) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int y = py + j;
            if (y < H) {
                const long long s = (long long)y * W + px;
                if (WIDE) {
                    uint32_t wa[BPS], wb[BPS];
                    load_words<4 * BPS>(pa + s * BPS, wa);
                    load_words<4 * BPS>(pb + s * BPS, wb);
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const long long d = (long long)code_of<BPS>(wa, i) - (long long)code_of<BPS>(wb, i);
                        sum += (unsigned long long)(d * d);
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        if (px + i < W) {
                            const long long d = (long long)code_at<BPS>(pa, s + i) - (long long)code_at<BPS>(pb, s + i);
                            sum += (unsigned long long)(d * d);
                        }
                    }
                }
            }
        }
    }
    const int cell = args.cell;
    long long *out = args.out + (size_t)f * (size_t)args.Hc * (size_t)args.Wc;
    if (cell == 4) {
        const int cx = x0 / 4 + bx, cy = y0 / 4 + by;
        if (cx < args.Wc && cy < args.Hc) out[(size_t)cy * args.Wc + cx] = (long long)sum;
        return;
    }
    blk[by][bx] = sum;
    __syncthreads();
    const int k = cell / 4, cells_x = BS_W / cell, cells_y = BS_H / cell;
    if ((int)threadIdx.x < cells_x * cells_y) {
        const int lx = threadIdx.x % cells_x, ly = threadIdx.x / cells_x;
        const int cx = x0 / cell + lx, cy = y0 / cell + ly;
        if (cx < args.Wc && cy < args.Hc) {
            unsigned long long v = 0;
            for (int j = 0; j < k; j++)
                for (int i = 0; i < k; i++) v += blk[ly * k + j][lx * k + i];
            out[(size_t)cy * args.Wc + cx] = (long long)v;
        }
    }
}

}  // namespace gsvc

using namespace gsvc;

static inline int64_t wssim_tiles(int32_t C, int32_t H, int32_t W)
{
    return (int64_t)C * ((H + ST_TILE - 1) / ST_TILE) * ((W + ST_TILE - 1) / ST_TILE);
}

static inline bool wssim_shape_ok(int32_t C, int32_t H, int32_t W) { return C > 0 && C <= 65535 && H > 0 && W > 0 && H <= 32768 && W <= 32768; }

static inline CellWeights cell_weights(const float *weights, int32_t W, int32_t cell)
{
    return CellWeights{weights, cell == 4 ? 2 : (cell == 8 ? 3 : 4), (W + cell - 1) / cell};
}

extern "C" int64_t gsvc_wssim_workspace_floats(int32_t C, int32_t H, int32_t W)
{
    return wssim_shape_ok(C, H, W) ? 2 * wssim_tiles(C, H, W) : -1;
}

extern "C" int gsvc_wssim_l1_forward(const float *img1, const float *img1b, const float *img2, const float *weights, int32_t C, int32_t H,
                                     int32_t W, int32_t cell, float *sums, float *workspace, float *dm_dmu1, float *dm_de11, float *dm_de12,
                                     float *avg_out, void *stream)
{
    GSVC_REQUIRE(img1 && img2 && weights && sums && workspace, "wssim_l1_forward: NULL pointer");
    GSVC_REQUIRE(wssim_shape_ok(C, H, W), "wssim_l1_forward: bad shape");
    GSVC_REQUIRE(cell == 4 || cell == 8 || cell == 16, "wssim_l1_forward: cell must be 4, 8 or 16 (got %d)", (int)cell);
    GSVC_REQUIRE((dm_dmu1 && dm_de11 && dm_de12) || (!dm_dmu1 && !dm_de11 && !dm_de12),
                 "wssim_l1_forward: pass all three partial maps or none");
    GSVC_REQUIRE(!img1b || avg_out, "wssim_l1_forward: the pair form needs avg_out");
    hipStream_t s = (hipStream_t)stream;
    static const SsimWindow win = make_loss_window();
    const dim3 grid((W + ST_TILE - 1) / ST_TILE, (H + ST_TILE - 1) / ST_TILE, C);
    {
        ProfScope _prof("k_wssim_fwd", s);
        hipLaunchKernelGGL(k_wssim_fwd, grid, dim3(256), 0, s, win, img1, img1b, avg_out, img2, cell_weights(weights, W, cell), H, W,
                           workspace, dm_dmu1, dm_de11, dm_de12);
    }
    {
        ProfScope _prof("k_wssim_finalize", s);
        hipLaunchKernelGGL(k_wssim_finalize, dim3(1), dim3(256), 0, s, workspace, (long long)wssim_tiles(C, H, W), sums);
    }
    return check_launch("wssim_l1_forward");
}

extern "C" int gsvc_wssim_l1_backward(const float *img1, const float *img1b, const float *img2, const float *weights, int32_t C, int32_t H,
                                      int32_t W, int32_t cell, const float *grads, const float *dm_dmu1, const float *dm_de11,
                                      const float *dm_de12, float *dL_dimg1, float *dL_dimg1b, void *stream)
{
    GSVC_REQUIRE(img1 && img2 && weights && grads && dm_dmu1 && dm_de11 && dm_de12 && dL_dimg1, "wssim_l1_backward: NULL pointer");
    GSVC_REQUIRE(wssim_shape_ok(C, H, W), "wssim_l1_backward: bad shape");
    GSVC_REQUIRE(cell == 4 || cell == 8 || cell == 16, "wssim_l1_backward: cell must be 4, 8 or 16 (got %d)", (int)cell);
    GSVC_REQUIRE((img1b != nullptr) == (dL_dimg1b != nullptr), "wssim_l1_backward: the pair form needs img1b and dL_dimg1b together");
    hipStream_t s = (hipStream_t)stream;
    static const SsimWindow win = make_loss_window();
    {
        ProfScope _prof("k_wssim_bwd", s);
        hipLaunchKernelGGL(k_wssim_bwd, dim3((W + ST_TILE - 1) / ST_TILE, (H + ST_TILE - 1) / ST_TILE, C), dim3(256), 0, s, win, img1, img1b,
                           dL_dimg1b, img2, cell_weights(weights, W, cell), H, W, 1.0f / ((float)C * (float)H * (float)W), grads, dm_dmu1,
                           dm_de11, dm_de12, dL_dimg1);
    }
    return check_launch("wssim_l1_backward");
}

extern "C" int gsvc_frames_block_sse(const uint8_t *a, const uint8_t *b, int64_t stride, int32_t n, int32_t H, int32_t W, int32_t layout,
                                     int32_t depth, int32_t cell, int64_t *out, void *stream)
{
    const char *who = "frames_block_sse";
    GSVC_REQUIRE(a && b && out, "%s: NULL pointer", who);
    GSVC_REQUIRE(layout != GSVC_FRAMES_RGB24, "%s: rgb24 frames hold no luma plane", who);
    GSVC_FRAMES_TRY(frames_check_format(who, n, 65535, layout, depth, 8, 16));
    GSVC_REQUIRE(cell == 4 || cell == 8 || cell == 16, "%s: cell must be 4, 8 or 16 (got %d)", who, (int)cell);
    GSVC_FRAMES_TRY(frames_check_size(who, H, W, layout));
    const FrameBufs bufs{"stride", a, stride, b, stride};
    GSVC_FRAMES_TRY(frames_check_strides(who, bufs, gsvc_frames_bytes(H, W, layout, depth)));
    const bool deep = depth > 8;
    if (deep) GSVC_FRAMES_TRY(frames_check_even(who, bufs));
    GSVC_REQUIRE((reinterpret_cast<uintptr_t>(out) & 7) == 0, "%s: out is not 8-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    const int Hc = (H + cell - 1) / cell, Wc = (W + cell - 1) / cell;
    const BlockSseArgs g = {a, b, stride, reinterpret_cast<long long *>(out), H, W, cell, Hc, Wc};
    const uintptr_t row_bytes = deep ? 8 : 4;          // of a block's row of four samples
    const bool wide = (bufs.alignment(n) & (row_bytes - 1)) == 0 && W % 4 == 0;
    const dim3 grid((unsigned)((W + BS_W - 1) / BS_W), (unsigned)((H + BS_H - 1) / BS_H), (unsigned)n);
    static void (*const kernels[2][2])(BlockSseArgs) = {{k_frames_block_sse<1, false>, k_frames_block_sse<1, true>},
                                                        {k_frames_block_sse<2, false>, k_frames_block_sse<2, true>}};
    ProfScope _p("k_frames_block_sse", s);
    hipLaunchKernelGGL(kernels[deep][wide], grid, dim3(256), 0, s, g);
    return check_launch(who);
}
