// gsvc_amd/csrc/metrics.hip — video quality metrics as kernels, gfx950: the per-plane sum of squared code differences of two
// frame buffers (PSNR-Y / -U / -V on the codes) and a fused MS-SSIM.
//
// gsvc_frames_sse   one launch for the n frames of a chunk (frame = blockIdx.y).  The planes of a frame are contiguous, so a frame
//   is ONE flat run of samples and a plane is a range of sample indices: plane(s) = (s >= HW) + (s >= HW + chroma samples); rgb24's
//   channel is s mod 3.  A lane's three accumulators are 64-bit (32-bit partial sums for the 16 pixels of an rgb24 unit); the
//   64-bit three-plane reduction is add_block_sums of frames_common.h, shared with k_picture_hash, as are the sample helpers.
//   Integer addition is associative: the result is the same bits in every run.
//     wide path   (both bases and, for n > 1, both strides 16-byte aligned): a lane takes 16 bytes of a and of b per unit
//                 (rgb24: 48 bytes = three vectors per unit)
//     edge path   one sample per lane, at any alignment (deep formats: even).
//   Nothing past the last sample of a frame is read.  The host part (checks, memset, launch shape, dispatch) is frames_sums_setup.
// gsvc_msssim       per scale one launch of k_msssim_scale (32x32 outputs of the VALID 11-tap blur per workgroup: the 42x42 inputs
//   of both pictures staged in LDS, the five moments blurred separably by the tile blur of ssim_tile.h, which the SSIM loss kernels
//   share) and, between scales, one launch of k_msssim_pool (2x2 mean, a leading zero row /
//   column for an odd side) — pooling is a kernel of its own: its windows start at -1 on an odd side and so do not tile with the
//   blur's outputs.  A tile writes ONE float partial; k_msssim_finalize adds the partials of a (scale, plane) in a fixed order in
//   double.  No float atomics: two runs give the same bits.
//   The samples are CENTRED before the moments: a workgroup subtracts the value of one of its pixels (cx of x, cy of y) on the way
//   from LDS to the registers.  Variances and the covariance do not change under a shift, mu = m + c, and E[x^2] - mu^2 no longer
//   subtracts two numbers near 0.5 to get one near 1e-4: that cancellation is the float32 error of the tensor-expression form
//   (DESIGN section 8e).
#include "frames_common.h"
#include "msssim_layout.h"
#include "reduce.h"
#include "ssim_tile.h"

#include <cmath>
#include <type_traits>

namespace gsvc {

// ============================================================================================================================
// plane SSE on codes
// ============================================================================================================================
struct SseArgs {
    const uint8_t *a, *b;
    long long stride_a, stride_b;
    unsigned long long *out;           // [n, 3]
    SampleRun run;
};

__device__ __forceinline__ uint32_t sq_diff(uint32_t x, uint32_t y)
{
    const uint32_t d = x > y ? x - y : y - x;
    return d * d;                       // 65535^2 = 4 294 836 225 < 2^32
}

// plane of the flat sample index s
template <bool RGB>
__device__ __forceinline__ int sse_plane(const SampleRun &g, long long s)
{
    return RGB ? (int)((uint32_t)s % 3u) : (s >= g.p0) + (s >= g.p1);
}

// the walk of frames_common.h (SampleRun); the per-sample work: the squared difference of the two buffers' codes
template <int BPS, bool RGB, bool WIDE>
__global__ void __launch_bounds__(256) k_frames_sse(SseArgs args)
{
    const SampleRun &g = args.run;
    const uint8_t *a = args.a + (size_t)blockIdx.y * (size_t)args.stride_a;
    const uint8_t *b = args.b + (size_t)blockIdx.y * (size_t)args.stride_b;
    unsigned long long acc[3] = {0ull, 0ull, 0ull};
    const long long first = (long long)blockIdx.x * (256 * SUMS_PER_LANE) + threadIdx.x;
    if (WIDE) {
        constexpr int SPV = 16 / BPS;                    // samples of a 16-byte vector
        constexpr int SPU = RGB ? 3 * SPV : SPV;         // samples of a unit
        constexpr int NW = SPU * BPS / 4;                // its 32-bit words
        const long long units = g.samples / SPU, tail0 = units * SPU;
#pragma unroll
        for (int j = 0; j < SUMS_PER_LANE; j++) {
            const long long unit = first + 256 * j;
            if (unit < units) {
                const long long s0 = unit * SPU;
                uint32_t wa[NW], wb[NW];
                load_words<4 * NW>(a + s0 * BPS, wa);
                load_words<4 * NW>(b + s0 * BPS, wb);
                if (RGB) {
                    uint32_t t[3] = {0u, 0u, 0u};        // 16 squares of at most 255^2 each: 32 bits hold them
#pragma unroll
                    for (int k = 0; k < SPU; k++) t[k % 3] += sq_diff(code_of<1>(wa, k), code_of<1>(wb, k));
                    acc[0] += t[0];
                    acc[1] += t[1];
                    acc[2] += t[2];
                } else {
                    const int pf = sse_plane<false>(g, s0), pl = sse_plane<false>(g, s0 + SPV - 1);
                    if (pf == pl) {
                        unsigned long long t = 0ull;
#pragma unroll
                        for (int k = 0; k < SPV; k++) t += sq_diff(code_of<BPS>(wa, k), code_of<BPS>(wb, k));
                        add_to_plane(acc, pf, t);
                    } else {                              // a plane boundary inside the vector
#pragma unroll
                        for (int k = 0; k < SPV; k++)
                            add_to_plane(acc, sse_plane<false>(g, s0 + k), sq_diff(code_of<BPS>(wa, k), code_of<BPS>(wb, k)));
                    }
                }
            } else {
                const long long s = tail0 + (unit - units);
                if (s < g.samples) add_to_plane(acc, sse_plane<RGB>(g, s), sq_diff(code_at<BPS>(a, s), code_at<BPS>(b, s)));
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < SUMS_PER_LANE; j++) {
            const long long s = first + 256 * j;
            if (s < g.samples) add_to_plane(acc, sse_plane<RGB>(g, s), sq_diff(code_at<BPS>(a, s), code_at<BPS>(b, s)));
        }
    }
    add_block_sums(acc, args.out + 3 * (size_t)blockIdx.y);
}

// ============================================================================================================================
// fused MS-SSIM
// ============================================================================================================================
// a sample as a float: codes are DIVIDED by the peak (an IEEE float32 division = torch's uint -> float32 -> div(peak))
template <typename T>
__device__ __forceinline__ float ms_sample(const T *p, size_t i, float peak)
{
    if (std::is_same<T, float>::value) return (float)p[i];
    return (float)p[i] / peak;
}

struct MsPicture {
    const void *x, *y;
    long long x_row, x_plane, y_row, y_plane;        // pitches in samples
    float peak;
};

// one scale: partials[plane * tiles + tile] = the sum over the tile's valid outputs of the cs map (last = 0) or the SSIM map (last = 1)
template <typename T>
__global__ void __launch_bounds__(256) k_msssim_scale(SsimWindow win_s, MsPicture pic, int H, int W, int last, float *__restrict__ partials)
{
    __shared__ __attribute__((aligned(16))) float st[2][ST_HALO][ST_LD];   // the staged pictures: x, y
    __shared__ float hb[5][ST_HALO][ST_HLD];
    __shared__ float red[4];
    const SsimWindow win = window_in_vgprs(win_s);
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * ST_TILE, y0 = blockIdx.y * ST_TILE;
    const int Hv = H - (ST_TAPS - 1), Wv = W - (ST_TAPS - 1);       // the valid outputs
    const T *px = reinterpret_cast<const T *>(pic.x) + (size_t)blockIdx.z * (size_t)pic.x_plane;
    const T *py = reinterpret_cast<const T *>(pic.y) + (size_t)blockIdx.z * (size_t)pic.y_plane;
    // the 42x42 inputs of the tile's valid outputs (no offset), zero past the picture
    float v[ST_LOADS][2];
#pragma unroll
    for (int it = 0; it < ST_LOADS; it++) {
        int r, c;
        const bool live = tile_slot(it, r, c);
        const int gy = y0 + r, gx = x0 + c;
        const bool in = live && gy < H && gx < W;
        v[it][0] = in ? ms_sample<T>(px, (size_t)gy * (size_t)pic.x_row + gx, pic.peak) : 0.f;
        v[it][1] = in ? ms_sample<T>(py, (size_t)gy * (size_t)pic.y_row + gx, pic.peak) : 0.f;
    }
    store_tile(st, v);
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
            if (y0 + 4 * gq + j < Hv) {          // (rows of hb below the picture were not written: their outputs are not taken)
                const float m1 = mom[0][j], m2 = mom[1][j];
                const float s1 = mom[2][j] - m1 * m1, s2 = mom[3][j] - m2 * m2, s12 = mom[4][j] - m1 * m2;
                const float cs = (2.f * s12 + SSIM_C2) / (s1 + s2 + SSIM_C2);
                const float mu1 = m1 + cx, mu2 = m2 + cy;
                const float lum = (2.f * mu1 * mu2 + SSIM_C1) / (mu1 * mu1 + mu2 * mu2 + SSIM_C1);
                sum += last ? lum * cs : cs;
            }
        }
    }
    const float total = block_sum_256<SumOrder::Pairs, Slot::Once>(sum, red);
    if (tid == 0) partials[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = total;
}

// 2x2 mean of both pictures: out(i, j) = (in(2i - ph, 2j - pw) + in(2i - ph, 2j - pw + 1) + in(2i - ph + 1, ..) + ..) / 4 with ph = H % 2,
// pw = W % 2 and index -1 read as zero (the padded cell counts in the divisor); the sum runs row by row as torch's avg_pool2d does
template <typename T>
__global__ void __launch_bounds__(256) k_msssim_pool(MsPicture pic, int H, int W, int H2, int W2, float *__restrict__ out_x,
                                                     float *__restrict__ out_y)
{
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= H2 * W2) return;
    const int i = o / W2, j = o - i * W2;
    const int r0 = 2 * i - (H & 1), c0 = 2 * j - (W & 1);
    const T *px = reinterpret_cast<const T *>(pic.x) + (size_t)blockIdx.y * (size_t)pic.x_plane;
    const T *py = reinterpret_cast<const T *>(pic.y) + (size_t)blockIdx.y * (size_t)pic.y_plane;
    float sx = 0.f, sy = 0.f;
#pragma unroll
    for (int dr = 0; dr < 2; dr++)
#pragma unroll
        for (int dc = 0; dc < 2; dc++) {
            const int r = r0 + dr, c = c0 + dc;
            const bool in = r >= 0 && c >= 0;            // (r <= H - 1 and c <= W - 1 by construction)
            sx += in ? ms_sample<T>(px, (size_t)r * (size_t)pic.x_row + c, pic.peak) : 0.f;
            sy += in ? ms_sample<T>(py, (size_t)r * (size_t)pic.y_row + c, pic.peak) : 0.f;
        }
    const size_t at = (size_t)blockIdx.y * ((size_t)H2 * W2) + o;
    out_x[at] = 0.25f * sx;
    out_y[at] = 0.25f * sy;
}

struct MsFinalize {
    long long offset[MS_SCALES];       // first partial of a scale
    int tiles[MS_SCALES];              // tiles of one plane
    double inv_count[MS_SCALES];       // 1 / valid outputs of one plane
};

// out[scale, plane] = (the partials of the plane's tiles, added in a fixed order in double) / outputs: lane t takes the tiles
// t, t + 256, ... in rising order, then a tree over the 256 lanes whose shape does not depend on anything
__global__ void __launch_bounds__(256) k_msssim_finalize(MsFinalize f, const float *__restrict__ partials, int P, double *__restrict__ out)
{
    __shared__ double red[256];
    const int plane = blockIdx.x, scale = blockIdx.y, n = f.tiles[scale];
    const float *p = partials + f.offset[scale] + (size_t)plane * n;
    double a = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) a += (double)p[i];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[(size_t)scale * P + plane] = red[0] * f.inv_count[scale];
}

template <typename T>
static void ms_launch_first(const SsimWindow &win, const MsPicture &pic, const MsLayout &L, int32_t P, float *pyr1, float *partials,
                            hipStream_t s)
{
    {
        ProfScope _p("k_msssim_scale", s);
        hipLaunchKernelGGL(k_msssim_scale<T>, dim3(L.tx[0], L.ty[0], P), dim3(256), 0, s, win, pic, L.h[0], L.w[0], 0, partials);
    }
    {
        ProfScope _p("k_msssim_pool", s);
        const int outs = L.h[1] * L.w[1];
        hipLaunchKernelGGL(k_msssim_pool<T>, dim3((outs + 255) / 256, P), dim3(256), 0, s, pic, L.h[0], L.w[0], L.h[1], L.w[1], pyr1,
                           pyr1 + (size_t)P * outs);
    }
}

}  // namespace gsvc

using namespace gsvc;

extern "C" int gsvc_frames_sse(const uint8_t *a, int64_t a_stride, const uint8_t *b, int64_t b_stride, int32_t n, int32_t H, int32_t W,
                               int32_t layout, int32_t depth, uint64_t *out, void *stream)
{
    GSVC_REQUIRE(a && b && out, "frames_sse: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    FrameSums fs;
    GSVC_FRAMES_TRY(frames_sums_setup("frames_sse", FrameBufs{"stride", a, a_stride, b, b_stride}, n, H, W, layout, depth, out, s, fs));
    const SseArgs g = {a, b, a_stride, b_stride, reinterpret_cast<unsigned long long *>(out), fs.run};
    static void (*const kernels[3][2])(SseArgs) = GSVC_FRAME_SUMS_KERNELS(k_frames_sse);
    ProfScope _p("k_frames_sse", s);
    hipLaunchKernelGGL(kernels[fs.variant][fs.wide], fs.grid, dim3(256), 0, s, g);
    return check_launch("frames_sse");
}

extern "C" int64_t gsvc_msssim_workspace_bytes(int32_t P, int32_t H, int32_t W)
{
    if (!ms_shape_ok(P, H, W)) return -1;
    return ms_layout(P, H, W).bytes;
}

extern "C" int gsvc_msssim(const void *x, int64_t x_row_pitch, int64_t x_plane_pitch, const void *y, int64_t y_row_pitch,
                           int64_t y_plane_pitch, int32_t P, int32_t H, int32_t W, int32_t sample_type, float peak, void *workspace,
                           double *out, void *stream)
{
    GSVC_REQUIRE(x && y && workspace && out, "msssim: NULL pointer");
    GSVC_REQUIRE(P >= 1 && P <= 65535, "msssim: P must be 1 .. 65535 (got %d)", (int)P);
    GSVC_REQUIRE(H >= 1 && W >= 1 && H <= 32768 && W <= 32768, "msssim: image size must be 1 .. 32768 (got %d x %d)", (int)H, (int)W);
    GSVC_REQUIRE(H > 160 && W > 160, "msssim: image sides must exceed 160 pixels for 5 scales (got %d x %d)", (int)H, (int)W);
    GSVC_REQUIRE(sample_type == GSVC_SAMPLE_F32 || sample_type == GSVC_SAMPLE_U8 || sample_type == GSVC_SAMPLE_U16,
                 "msssim: unknown sample type %d", (int)sample_type);
    GSVC_REQUIRE(x_row_pitch >= W && y_row_pitch >= W, "msssim: row pitch %lld / %lld is shorter than a row (%d samples)",
                 (long long)x_row_pitch, (long long)y_row_pitch, (int)W);
    const int64_t need_x = (int64_t)(H - 1) * x_row_pitch + W, need_y = (int64_t)(H - 1) * y_row_pitch + W;
    GSVC_REQUIRE(P == 1 || (x_plane_pitch >= need_x && y_plane_pitch >= need_y),
                 "msssim: plane pitch %lld / %lld is shorter than a plane (%lld / %lld samples)", (long long)x_plane_pitch,
                 (long long)y_plane_pitch, (long long)need_x, (long long)need_y);
    const uintptr_t bases = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y);
    const uintptr_t mask = sample_type == GSVC_SAMPLE_F32 ? 3 : (sample_type == GSVC_SAMPLE_U16 ? 1 : 0);
    GSVC_REQUIRE((bases & mask) == 0, "msssim: a picture base is not aligned to its sample type");
    GSVC_REQUIRE(sample_type == GSVC_SAMPLE_F32 || peak > 0.f, "msssim: the peak of codes must be positive");
    GSVC_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 7) == 0,
                 "msssim: the workspace must be 16-byte and out 8-byte aligned");
    const MsLayout L = ms_layout(P, H, W);
    static const SsimWindow win = make_msssim_window();
    hipStream_t s = (hipStream_t)stream;
    uint8_t *ws = reinterpret_cast<uint8_t *>(workspace);
    float *partials = reinterpret_cast<float *>(ws + L.partials);
    MsPicture pic;
    pic.x = x;
    pic.y = y;
    pic.x_row = x_row_pitch;
    pic.y_row = y_row_pitch;
    pic.x_plane = x_plane_pitch;
    pic.y_plane = y_plane_pitch;
    pic.peak = sample_type == GSVC_SAMPLE_F32 ? 1.f : peak;
    float *pyr1 = reinterpret_cast<float *>(ws + L.pyr[1]);
    if (sample_type == GSVC_SAMPLE_F32) ms_launch_first<float>(win, pic, L, P, pyr1, partials, s);
    else if (sample_type == GSVC_SAMPLE_U8) ms_launch_first<uint8_t>(win, pic, L, P, pyr1, partials, s);
    else ms_launch_first<uint16_t>(win, pic, L, P, pyr1, partials, s);
    for (int k = 1; k < MS_SCALES; k++) {
        const int h = L.h[k], w = L.w[k];
        float *lx = reinterpret_cast<float *>(ws + L.pyr[k]);
        MsPicture lv;
        lv.x = lx;
        lv.y = lx + (size_t)P * h * w;
        lv.x_row = lv.y_row = w;
        lv.x_plane = lv.y_plane = (long long)h * w;
        lv.peak = 1.f;
        {
            ProfScope _p("k_msssim_scale", s);
            hipLaunchKernelGGL(k_msssim_scale<float>, dim3(L.tx[k], L.ty[k], P), dim3(256), 0, s, win, lv, h, w,
                               k == MS_SCALES - 1 ? 1 : 0, partials + L.part_off[k]);
        }
        if (k + 1 < MS_SCALES) {
            ProfScope _p("k_msssim_pool", s);
            const int outs = L.h[k + 1] * L.w[k + 1];
            float *nx = reinterpret_cast<float *>(ws + L.pyr[k + 1]);
            hipLaunchKernelGGL(k_msssim_pool<float>, dim3((outs + 255) / 256, P), dim3(256), 0, s, lv, h, w, L.h[k + 1], L.w[k + 1], nx,
                               nx + (size_t)P * outs);
        }
    }
    MsFinalize f;
    for (int k = 0; k < MS_SCALES; k++) {
        f.offset[k] = L.part_off[k];
        f.tiles[k] = L.tx[k] * L.ty[k];
        f.inv_count[k] = 1.0 / ((double)(L.h[k] - (ST_TAPS - 1)) * (double)(L.w[k] - (ST_TAPS - 1)));
    }
    {
        ProfScope _p("k_msssim_finalize", s);
        hipLaunchKernelGGL(k_msssim_finalize, dim3(P, MS_SCALES), dim3(256), 0, s, f, partials, P, out);
    }
    return check_launch("msssim");
}
