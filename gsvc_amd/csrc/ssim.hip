// gsvc_amd/csrc/ssim.hip — fused SSIM + L1 image loss (forward and backward), gfx950.
//
// Replaces the distortion part of the fitting step: reference utils/loss_utils.py:20-72 (l1_loss_func and
// ssim_func/_ssim: five depthwise 11x11 Gaussian-window conv2d calls with zero padding plus ~15 elementwise
// kernels per image pair, and their autograd).  One kernel each way:
//   forward   per 32x32 tile: img1/img2 with a 5-pixel halo staged in LDS, separable 11-tap blur of the five
//             moments (x, y, x^2, y^2, xy) through LDS, the SSIM map, its sum, |x-y| summed, and the three
//             per-pixel partials d(map)/d(mu1), d(map)/d(E[x^2]), d(map)/d(E[xy]) for the backward
//   backward  per 32x32 tile: the three partial maps (times dL/dmap) blurred again (the window is symmetric,
//             so the transposed convolution is the same convolution) and combined with x, y; + the L1 sign
// The tile blur itself (staging, the register-blocked horizontal and vertical passes, the window) is ssim_tile.h, shared with
// the MS-SSIM kernel of metrics.hip; what is written here is what the two loss kernels do with the blurred planes.
#include "common.h"
#include "reduce.h"
#include "ssim_tile.h"

namespace gsvc {

constexpr int SS_SLOTS = 1024;             // rows of the partial-sum workspace

// img1b != NULL: the first image is the two-view frame 0.5 * (img1 + flip_W(img1b)) (reference pipeline/train.py:368-375), formed
// on load (and stored to avg_out where the caller wants it) instead of by three elementwise launches each way.
__global__ void __launch_bounds__(256) k_ssim_fwd(SsimWindow win_s, const float *__restrict__ img1, const float *__restrict__ img1b,
                                                  float *__restrict__ avg_out,
                                                  const float *__restrict__ img2, int H, int W,
                                                  float *__restrict__ partials /* [SS_SLOTS][2]: ssim, l1 */,
                                                  float *__restrict__ dm_dmu1, float *__restrict__ dm_de11,
                                                  float *__restrict__ dm_de12)
{
    __shared__ __attribute__((aligned(16))) float st[2][ST_HALO][ST_LD];   // the staged images: x, y
    __shared__ float hb[5][ST_HALO][ST_HLD];  // horizontally blurred moments
    __shared__ float red[4];
    const SsimWindow win = window_in_vgprs(win_s);
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * ST_TILE, y0 = blockIdx.y * ST_TILE;
    const size_t plane = (size_t)blockIdx.z * H * W;
    // the tile with its 5-pixel halo, zero outside the image
    float v[ST_LOADS][2];
#pragma unroll
    for (int it = 0; it < ST_LOADS; it++) {
        int r, c;
        const bool live = tile_slot(it, r, c);
        const int gy = y0 + r - ST_R, gx = x0 + c - ST_R;
        const bool in = live && gy >= 0 && gy < H && gx >= 0 && gx < W;
        const float xa = in ? img1[plane + (size_t)gy * W + gx] : 0.f;
        const float xb = (img1b && in) ? img1b[plane + (size_t)gy * W + (W - 1 - gx)] : 0.f;
        v[it][0] = img1b ? (xa + xb) / 2.0f : xa;
        v[it][1] = in ? img2[plane + (size_t)gy * W + gx] : 0.f;
    }
    store_tile(st, v);
    __syncthreads();
    // horizontal pass: group g = (row r, columns 4 cg .. 4 cg + 3)
    for (int g = tid; g < ST_GROUPS; g += 256) {
        const int r = g >> 3, c0 = 4 * (g & 7);
        float xv[16], yv[16];
        staged_row16(st[0], r, c0, xv);
        staged_row16(st[1], r, c0, yv);
        blur4_moments(win, xv, yv, hb, r, c0);
    }
    __syncthreads();
    // vertical pass: thread = (column lx, rows 4 gq .. 4 gq + 3)
    const int lx = tid & 31, gq = tid >> 5;
    float mom[5][4];
#pragma unroll
    for (int m = 0; m < 5; m++) blur4_column(win, hb[m], 4 * gq, lx, mom[m]);
    const int gx = x0 + lx;
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
            ssim_sum += ssim;
            l1_sum += fabsf(xc - yc);
            const size_t o = plane + (size_t)gy * W + gx;
            if (avg_out) avg_out[o] = xc;
            if (dm_dmu1) {
                // map as a function of (mu1, E[x^2], E[xy]) with sigma1^2 = E[x^2] - mu1^2, sigma12 = E[xy] - mu1 mu2
                dm_dmu1[o] = 2.f * mu2 * (num2 - num1) * inv - 2.f * mu1 * ssim * (1.0f / A - 1.0f / B);
                dm_de11[o] = -ssim / B;
                dm_de12[o] = 2.f * num1 * inv;
            }
        }
    }
    const float ssum = block_sum_256<SumOrder::Chain>(ssim_sum, red);
    const float lsum = block_sum_256<SumOrder::Chain>(l1_sum, red);
    if (tid == 0) {
        // spread the per-block sums over SS_SLOTS rows: atomics on one address serialise at the memory side
        const unsigned slot = (blockIdx.x + blockIdx.y * gridDim.x + blockIdx.z * gridDim.x * gridDim.y) % SS_SLOTS;
        atomicAdd(&partials[2 * slot + 0], ssum);
        atomicAdd(&partials[2 * slot + 1], lsum);
    }
}

__global__ void __launch_bounds__(256) k_ssim_finalize(const float *__restrict__ partials, float *__restrict__ sums)
{
    __shared__ float red[4];
    float a = 0.f, b = 0.f;
    for (int i = threadIdx.x; i < SS_SLOTS; i += 256) { a += partials[2 * i]; b += partials[2 * i + 1]; }
    a = block_sum_256<SumOrder::Chain>(a, red);
    b = block_sum_256<SumOrder::Chain>(b, red);
    if (threadIdx.x == 0) { sums[0] = a; sums[1] = b; }
}

// dL/dimg1 = conv(g*dm_dmu1) + 2 x conv(g*dm_de11) + y conv(g*dm_de12) + g_l1 * sign(x - y),
// g = grads[0] / (C*H*W) (mean of the map), g_l1 = grads[1] / (C*H*W)
__global__ void __launch_bounds__(256) k_ssim_bwd(SsimWindow win_s, const float *__restrict__ img1, const float *__restrict__ img1b,
                                                  float *__restrict__ dL_dimg1b,
                                                  const float *__restrict__ img2, int H, int W, float inv_count,
                                                  const float *__restrict__ grads, const float *__restrict__ dm_dmu1,
                                                  const float *__restrict__ dm_de11, const float *__restrict__ dm_de12,
                                                  float *__restrict__ dL_dimg1)
{
    __shared__ __attribute__((aligned(16))) float sm[3][ST_HALO][ST_LD];
    __shared__ float hb[3][ST_HALO][ST_HLD];
    const SsimWindow win = window_in_vgprs(win_s);
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * ST_TILE, y0 = blockIdx.y * ST_TILE;
    const size_t plane = (size_t)blockIdx.z * H * W;
    // The three partial maps with the halo, zero outside the image.  Written out, not tile_slot / store_tile: through them this kernel
    // measured 66.25 us against 65.75 - 65.98 (eight more integer instructions for the same LDS addresses).
    float ma[3][ST_LOADS];
#pragma unroll
    for (int it = 0; it < ST_LOADS; it++) {          // all loads first (ssim_tile.h)
        const int i = tid + 256 * it;
        const int r = i / ST_HALO, c = i - r * ST_HALO;
        const int gy = y0 + r - ST_R, gx = x0 + c - ST_R;
        const bool in = i < ST_HALO * ST_HALO && gy >= 0 && gy < H && gx >= 0 && gx < W;
        const size_t o = plane + (size_t)gy * W + gx;
        ma[0][it] = in ? dm_dmu1[o] : 0.f;
        ma[1][it] = in ? dm_de11[o] : 0.f;
        ma[2][it] = in ? dm_de12[o] : 0.f;
    }
#pragma unroll
    for (int it = 0; it < ST_LOADS; it++) {
        const int i = tid + 256 * it;
        const int r = i / ST_HALO, c = i - r * ST_HALO;
        if (i < ST_HALO * ST_HALO) {
            sm[0][r][c] = ma[0][it]; sm[1][r][c] = ma[1][it]; sm[2][r][c] = ma[2][it];
        }
    }
    if (tid < 2 * ST_HALO) {
#pragma unroll
        for (int m = 0; m < 3; m++) sm[m][tid >> 1][ST_HALO + (tid & 1)] = 0.f;
    }
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
    const int lx = tid & 31, gq = tid >> 5;
    float bl[3][4];
#pragma unroll
    for (int m = 0; m < 3; m++) blur4_column(win, hb[m], 4 * gq, lx, bl[m]);
    const int gx = x0 + lx;
    const float g = grads[0] * inv_count, gl = grads[1] * inv_count;
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
            // the L1 term joins the ROUNDED SSIM term in one fma, said explicitly: as g * (..) + gl * sgn the compiler fuses one of the
            // two products and rounds the other, and which one changes with the code around it (and with it the last bit)
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

}  // namespace gsvc

using namespace gsvc;

static int ssim_forward_impl(const float *img1, const float *img1b, float *avg_out, const float *img2, int32_t C, int32_t H, int32_t W,
                             float *sums, float *workspace, float *dm_dmu1, float *dm_de11, float *dm_de12, void *stream)
{
    GSVC_REQUIRE(img1 && img2 && sums && workspace, "ssim_l1_forward: NULL pointer");
    GSVC_REQUIRE(C > 0 && H > 0 && W > 0, "ssim_l1_forward: bad shape");
    GSVC_REQUIRE((dm_dmu1 && dm_de11 && dm_de12) || (!dm_dmu1 && !dm_de11 && !dm_de12),
                 "ssim_l1_forward: pass all three partial maps or none");
    hipStream_t s = (hipStream_t)stream;
    if (gsvc::zero_words_async(workspace, 2 * SS_SLOTS * sizeof(float), s) != hipSuccess) {
        set_error("ssim_l1_forward: zeroing failed");
        return GSVC_E_LAUNCH;
    }
    static const SsimWindow win = make_loss_window();
    {
        ProfScope _prof("k_ssim_fwd", s);
        hipLaunchKernelGGL(k_ssim_fwd, dim3((W + ST_TILE - 1) / ST_TILE, (H + ST_TILE - 1) / ST_TILE, C), dim3(256), 0, s,
                           win, img1, img1b, avg_out, img2, H, W, workspace, dm_dmu1, dm_de11, dm_de12);
    }
    {
        ProfScope _prof("k_ssim_finalize", s);
        hipLaunchKernelGGL(k_ssim_finalize, dim3(1), dim3(256), 0, s, workspace, sums);
    }
    return check_launch("ssim_l1_forward");
}

extern "C" int gsvc_ssim_l1_forward(const float *img1, const float *img2, int32_t C, int32_t H, int32_t W, float *sums,
                                    float *workspace, float *dm_dmu1, float *dm_de11, float *dm_de12, void *stream)
{
    return ssim_forward_impl(img1, nullptr, nullptr, img2, C, H, W, sums, workspace, dm_dmu1, dm_de11, dm_de12, stream);
}

extern "C" int gsvc_ssim_l1_pair_forward(const float *img_f, const float *img_b, const float *img2, int32_t C, int32_t H, int32_t W,
                                         float *sums, float *workspace, float *dm_dmu1, float *dm_de11, float *dm_de12,
                                         float *avg_out, void *stream)
{
    GSVC_REQUIRE(img_b, "ssim_l1_pair_forward: NULL pointer");
    return ssim_forward_impl(img_f, img_b, avg_out, img2, C, H, W, sums, workspace, dm_dmu1, dm_de11, dm_de12, stream);
}

static int ssim_backward_impl(const float *img1, const float *img1b, float *dL_dimg1b, const float *img2, int32_t C, int32_t H, int32_t W,
                              const float *grads, const float *dm_dmu1, const float *dm_de11, const float *dm_de12, float *dL_dimg1,
                              void *stream)
{
    GSVC_REQUIRE(img1 && img2 && grads && dm_dmu1 && dm_de11 && dm_de12 && dL_dimg1, "ssim_l1_backward: NULL pointer");
    GSVC_REQUIRE(C > 0 && H > 0 && W > 0, "ssim_l1_backward: bad shape");
    hipStream_t s = (hipStream_t)stream;
    static const SsimWindow win = make_loss_window();
    {
        ProfScope _prof("k_ssim_bwd", s);
        hipLaunchKernelGGL(k_ssim_bwd, dim3((W + ST_TILE - 1) / ST_TILE, (H + ST_TILE - 1) / ST_TILE, C), dim3(256), 0, s,
                           win, img1, img1b, dL_dimg1b, img2, H, W, 1.0f / ((float)C * (float)H * (float)W), grads, dm_dmu1, dm_de11,
                           dm_de12, dL_dimg1);
    }
    return check_launch("ssim_l1_backward");
}

extern "C" int gsvc_ssim_l1_backward(const float *img1, const float *img2, int32_t C, int32_t H, int32_t W,
                                     const float *grads, const float *dm_dmu1, const float *dm_de11,
                                     const float *dm_de12, float *dL_dimg1, void *stream)
{
    return ssim_backward_impl(img1, nullptr, nullptr, img2, C, H, W, grads, dm_dmu1, dm_de11, dm_de12, dL_dimg1, stream);
}

extern "C" int gsvc_ssim_l1_pair_backward(const float *img_f, const float *img_b, const float *img2, int32_t C, int32_t H, int32_t W,
                                          const float *grads, const float *dm_dmu1, const float *dm_de11, const float *dm_de12,
                                          float *dL_dimg_f, float *dL_dimg_b, void *stream)
{
    GSVC_REQUIRE(img_b && dL_dimg_b, "ssim_l1_pair_backward: NULL pointer");
    return ssim_backward_impl(img_f, img_b, dL_dimg_b, img2, C, H, W, grads, dm_dmu1, dm_de11, dm_de12, dL_dimg_f, stream);
}
