// gsvc_amd/csrc/tfilter.hip — motion-compensated temporal prefilter of the encoder's source frames, gfx950: the
// filter on the sample codes of a resident clip, and the noise sums its strength is estimated from.  Integers only; the arithmetic is
// stated sample by sample in include/gsvc_hip.h and gsvc_amd/tfilter.py.
//
// gsvc_tfilter_frames  k_tfilter<BPS> (BPS = bytes per sample: one body for 8-bit and deep frames).  A wave owns one 8 x 8 luma block of
//   one target frame, lane = pixel.  Per existing neighbour d = -2, -1, +1, +2 a lane rounds its flow vector to quarter pels, gathers
//   its four codes of frame t + d, forms the prediction and its squared difference; the block's SSE is one wave sum, so the block
//   index i_b and LUT_B[i_b] are the same in every lane, and the per-sample weight follows from the lane's own difference.  The chroma
//   samples under the block reuse the four block weights from registers: in 4:2:0 lanes 0 .. 15 take the 4 x 4 U samples and lanes
//   16 .. 31 the V samples, each with the vector of luma pixel (2y, 2x) by one shuffle per neighbour; in 4:4:4 two more passes of 64
//   lanes.  Every output sample is written once by a plain store: no atomics, no workspace, nothing depends on the launch geometry.
//   A partial block at the right or bottom edge keeps its absent lanes out of every load and store and counts the pixels it has.
// gsvc_noise_sums      k_noise_sums<BPS>: a workgroup takes 256 adjacent columns and 16 rows of one plane; a lane walks down its column
//   with the separable mask's row terms of three rows in registers (three loads per sample); the sums go through the 64-bit workgroup
//   reduction of frames_common.h once per workgroup (one integer atomic per workgroup: the same bits in any order).  (A first form
//   with one sample per lane paid that reduction per sample: 113 us per 1080p frame against 2.2 us for the picture hash.)
#include "frames_common.h"
#include "reduce.h"

namespace gsvc {

constexpr int TF_LUT = 64;                         // entries of a weight table
constexpr uint32_t TF_WEIGHT_MAX = 256;            // of wt[] and of a table entry: wt LUT_B LUT_P <= 2^24, a weight <= 256

struct TfArgs {
    const uint8_t *frames;
    long long stride;
    uint8_t *out;
    long long out_stride;
    const float *flows;                // [n, 4, 2, H, W]
    int T, first;
    int H, W, ch, cw;                  // the luma and the chroma plane
    int sub;                           // 1: 4:2:0
    int nbx, nblocks;                  // 8 x 8 luma blocks per row / per frame (partial ones included)
    uint32_t q[3], wt[2];
    unsigned long long qq;             // q[0]^2
    uint16_t lut_b[TF_LUT], lut_p[TF_LUT];
};

// clamp(rint(4 f), -32768, 32767): the float32 product rounded half to even.  (fmaxf / fminf return the number of (NaN, number), so
// even a flow that is not finite gives an integer in range.)
__device__ __forceinline__ int tf_mv(float f)
{
    return (int)fminf(fmaxf(rintf(4.0f * f), -32768.0f), 32767.0f);
}

// the prediction of sample (y, x) of an h x w plane (h, w >= 2) from vector (mvx, mvy) in 1 / 2^us samples.  Every position is
// clamped into the plane: nothing outside it is read, whatever the vector.
template <int BPS>
__device__ __forceinline__ uint32_t tf_pred(const uint8_t *plane, int w, int h, int x, int y, int mvx, int mvy, int us)
{
    const int px = min(max((x << us) + mvx, 0), (w - 1) << us), py = min(max((y << us) + mvy, 0), (h - 1) << us);
    const int x0 = min(px >> us, w - 2), y0 = min(py >> us, h - 2);
    const uint32_t fx = (uint32_t)(px - (x0 << us)), fy = (uint32_t)(py - (y0 << us)), u = 1u << us;
    const long long at = (long long)y0 * w + x0;
    const uint32_t a00 = code_at<BPS>(plane, at), a01 = code_at<BPS>(plane, at + 1);
    const uint32_t a10 = code_at<BPS>(plane, at + w), a11 = code_at<BPS>(plane, at + w + 1);
    const uint32_t sum = (u - fx) * (u - fy) * a00 + fx * (u - fy) * a01 + (u - fx) * fy * a10 + fx * fy * a11;          // <= 64 * 65535
    return (sum + (1u << (2 * us - 1))) >> (2 * us);
}

// one neighbour's share of a sample: w = (wB LUT_P[i_p] + 2^15) >> 16 with wB = wt LUT_B[i_b] of the sample's luma block
__device__ __forceinline__ void tf_add(uint32_t c, uint32_t pred, uint32_t wB, uint32_t q, const uint16_t *lut_p, uint32_t &num, uint32_t &den)
{
    const uint32_t ad = c > pred ? c - pred : pred - c;
    const uint32_t ip = min(63u, 128u * ad / q);
    const uint32_t w = (wB * (uint32_t)lut_p[ip] + 32768u) >> 16;
    num += w * pred;
    den += w;
}

template <int BPS>
__device__ __forceinline__ void tf_store(uint8_t *plane, long long s, uint32_t c, uint32_t num, uint32_t den)
{
    const uint32_t v = (256u * c + num + den / 2u) / den;          // den = 256 + the weights; the sum is below 1280 * 65536
    if (BPS == 1) plane[s] = (uint8_t)v;
    else reinterpret_cast<uint16_t *>(plane)[s] = (uint16_t)v;
}

template <int BPS>
__global__ void __launch_bounds__(256) k_tfilter(TfArgs a)
{
    __shared__ uint16_t s_lut_b[TF_LUT], s_lut_p[TF_LUT];
    if (threadIdx.x < TF_LUT) {
        s_lut_b[threadIdx.x] = a.lut_b[threadIdx.x];
        s_lut_p[threadIdx.x] = a.lut_p[threadIdx.x];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int blk = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (blk >= a.nblocks) return;                         // (the whole wave)
    const int k = blockIdx.y, t = a.first + k;
    const int by = blk / a.nbx, bx = blk - by * a.nbx;
    const int x = 8 * bx + (lane & 7), y = 8 * by + (lane >> 3);
    const bool valid = x < a.W && y < a.H;
    const long long px = (long long)a.H * a.W;
    const uint8_t *cur = a.frames + (size_t)t * (size_t)a.stride;
    uint8_t *dst = a.out + (size_t)k * (size_t)a.out_stride;
    const float *fl = a.flows + (size_t)k * 8 * (size_t)px + ((long long)y * a.W + x);
    const unsigned long long D = (unsigned long long)(min(8, a.W - 8 * bx) * min(8, a.H - 8 * by)) * a.qq;          // n_B q[0]^2 < 2^38

    // ---- luma: per neighbour the vector, the prediction, the block's SSE and with it the block weight
    const uint32_t c = valid ? code_at<BPS>(cur, (long long)y * a.W + x) : 0u;
    uint32_t num = 0u, den = 256u;
    int mv[4];                                            // (mvx & 0xFFFF) | mvy << 16
    uint32_t wB[4];                                       // wt LUT_B[i_b]; 0: the neighbour does not exist
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const int nt = t + (s < 2 ? s - 2 : s - 1);
        mv[s] = 0;
        wB[s] = 0u;
        if (nt < 0 || nt >= a.T) continue;                // (wave-uniform: its frame and its flow are never read)
        const uint8_t *nb = a.frames + (size_t)nt * (size_t)a.stride;
        uint32_t pred = 0u;
        if (valid) {
            const int mvx = tf_mv(fl[(2 * s) * px]), mvy = tf_mv(fl[(2 * s + 1) * px]);
            mv[s] = (mvx & 0xFFFF) | (int)((uint32_t)mvy << 16);
            pred = tf_pred<BPS>(nb, a.W, a.H, x, y, mvx, mvy, 2);
        }
        const long long diff = valid ? (long long)c - (long long)pred : 0ll;
        const unsigned long long N = 2048ull * wave_sum((unsigned long long)(diff * diff));          // < 2^11 * 2^6 * 2^32
        uint32_t ib = 0u;                                 // min(63, N / D): the largest i in 0 .. 63 with i D <= N
#pragma unroll
        for (uint32_t bit = 32u; bit; bit >>= 1) {
            const uint32_t cand = ib | bit;
            if ((unsigned long long)cand * D <= N) ib = cand;
        }
        wB[s] = a.wt[(s == 0 || s == 3) ? 1 : 0] * (uint32_t)s_lut_b[ib];
        if (valid) tf_add(c, pred, wB[s], a.q[0], s_lut_p, num, den);
    }
    if (valid) tf_store<BPS>(dst, (long long)y * a.W + x, c, num, den);

    // ---- chroma under the block, with the block weights
    const long long cpx = (long long)a.ch * a.cw;
    if (a.sub) {
        const int cp = lane >> 4, cxl = lane & 3, cyl = (lane >> 2) & 3;          // cp 0: U, 1: V; lanes 32 .. 63 have no sample
        const int cx = 4 * bx + cxl, cy = 4 * by + cyl;
        const bool cv = cp < 2 && cx < a.cw && cy < a.ch;
        const int from = 16 * cyl + 2 * cxl;              // the lane of luma pixel (2 cy, 2 cx): present whenever the chroma sample is
        const long long poff = (px + (cp == 1 ? cpx : 0ll)) * BPS, at = (long long)cy * a.cw + cx;
        const uint32_t q = a.q[cp == 1 ? 2 : 1];
        const uint32_t cc = cv ? code_at<BPS>(cur + poff, at) : 0u;
        uint32_t cnum = 0u, cden = 256u;
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const int nt = t + (s < 2 ? s - 2 : s - 1);
            if (nt < 0 || nt >= a.T) continue;
            const int m = __shfl(mv[s], from, 64);
            if (cv) {
                const uint8_t *nb = a.frames + (size_t)nt * (size_t)a.stride + poff;
                const uint32_t pred = tf_pred<BPS>(nb, a.cw, a.ch, cx, cy, (int)(int16_t)(m & 0xFFFF), m >> 16, 3);
                tf_add(cc, pred, wB[s], q, s_lut_p, cnum, cden);
            }
        }
        if (cv) tf_store<BPS>(dst + poff, at, cc, cnum, cden);
    } else {
        for (int cp = 1; cp <= 2; cp++) {
            const long long poff = cp * px * BPS, at = (long long)y * a.W + x;
            const uint32_t cc = valid ? code_at<BPS>(cur + poff, at) : 0u;
            uint32_t cnum = 0u, cden = 256u;
#pragma unroll
            for (int s = 0; s < 4; s++) {
                const int nt = t + (s < 2 ? s - 2 : s - 1);
                if (nt < 0 || nt >= a.T || !valid) continue;
                const uint8_t *nb = a.frames + (size_t)nt * (size_t)a.stride + poff;
                const uint32_t pred = tf_pred<BPS>(nb, a.W, a.H, x, y, (int)(int16_t)(mv[s] & 0xFFFF), mv[s] >> 16, 2);
                tf_add(cc, pred, wB[s], a.q[cp], s_lut_p, cnum, cden);
            }
            if (valid) tf_store<BPS>(dst + poff, at, cc, cnum, cden);
        }
    }
}

// ============================================================================================================================
// noise sums
// ============================================================================================================================
constexpr int NS_ROWS = 16;            // output rows per workgroup

struct NoiseArgs {
    const uint8_t *frames;
    long long stride;
    int H, W, ch, cw;
    int chunks_y, chunks_c;            // workgroups per row of the luma / a chroma plane (256 samples each)
    int groups_y, groups_c;            // groups of NS_ROWS rows of the luma / a chroma plane
    unsigned long long *out;           // [n, 3]
};

template <int BPS>
__global__ void __launch_bounds__(256) k_noise_sums(NoiseArgs a)
{
    // blockIdx.x: the (row group, chunk) tiles of Y, then those of U, then those of V (uniform in the workgroup)
    int b = (int)blockIdx.x, p = 0;
    const int ny = a.groups_y * a.chunks_y, nc = a.groups_c * a.chunks_c;
    if (b >= ny) {
        b -= ny;
        p = 1;
        if (b >= nc) {
            b -= nc;
            p = 2;
        }
    }
    const int chunks = p ? a.chunks_c : a.chunks_y, w = p ? a.cw : a.W, h = p ? a.ch : a.H;
    const int rg = b / chunks, x = (b - rg * chunks) * 256 + (int)threadIdx.x;
    const long long poff = p == 0 ? 0ll : (long long)a.H * a.W + (p == 2 ? (long long)a.ch * a.cw : 0ll);
    const uint8_t *plane = a.frames + (size_t)blockIdx.y * (size_t)a.stride + poff * BPS;
    // the mask is [1 -2 1]^T [1 -2 1]: a lane walks down its column with the row terms r(y) = c(y, x - 1) - 2 c(y, x) + c(y, x + 1) of
    // three rows in registers, three loads per sample
    const int ya = max(rg * NS_ROWS, 1), yb = min(rg * NS_ROWS + NS_ROWS, h - 1);          // output rows ya .. yb - 1
    uint32_t sum = 0u;                                    // <= 16 * 8 * 65535
    if (x >= 1 && x < w - 1 && ya < yb) {
        const long long at = (long long)(ya - 1) * w + x;
        int r0 = (int)code_at<BPS>(plane, at - 1) - 2 * (int)code_at<BPS>(plane, at) + (int)code_at<BPS>(plane, at + 1);
        int r1 = (int)code_at<BPS>(plane, at + w - 1) - 2 * (int)code_at<BPS>(plane, at + w) + (int)code_at<BPS>(plane, at + w + 1);
        for (int y = ya; y < yb; y++) {
            const long long below = (long long)(y + 1) * w + x;
            const int r2 = (int)code_at<BPS>(plane, below - 1) - 2 * (int)code_at<BPS>(plane, below) + (int)code_at<BPS>(plane, below + 1);
            sum += (uint32_t)abs(r0 - 2 * r1 + r2);
            r0 = r1;
            r1 = r2;
        }
    }
    unsigned long long acc[3] = {0ull, 0ull, 0ull};
    add_to_plane(acc, p, (unsigned long long)sum);
    add_block_sums(acc, a.out + 3 * (size_t)blockIdx.y);
}

static int tfilter_check_frames(const char *who, const FrameBufs &bufs, int32_t n, int32_t n_max, int32_t H, int32_t W, int32_t layout,
                                int32_t depth)
{
    GSVC_REQUIRE(layout != GSVC_FRAMES_RGB24, "%s: rgb24 frames hold no luma plane (the filter works on Y'CbCr codes)", who);
    GSVC_FRAMES_TRY(frames_check_format(who, n, n_max, layout, depth, 8, 16));
    GSVC_REQUIRE(depth == 8 || depth == 10 || depth == 12 || depth == 16, "%s: depth must be 8, 10, 12 or 16 (got %d)", who, (int)depth);
    GSVC_FRAMES_TRY(frames_check_size(who, H, W, layout));
    GSVC_REQUIRE(H >= 8 && W >= 8, "%s: image size must be at least 8 x 8 (got %d x %d)", who, (int)H, (int)W);
    GSVC_FRAMES_TRY(frames_check_strides(who, bufs, gsvc_frames_bytes(H, W, layout, depth)));
    if (depth > 8) GSVC_FRAMES_TRY(frames_check_even(who, bufs));
    return GSVC_OK;
}

}  // namespace gsvc

using namespace gsvc;

extern "C" int gsvc_tfilter_frames(const uint8_t *frames, int64_t stride, int32_t T, int32_t first, int32_t n, int32_t H, int32_t W,
                                   int32_t layout, int32_t depth, const float *flows, const uint32_t *q_host, const uint32_t *wt_host,
                                   const uint16_t *lut_b_host, const uint16_t *lut_p_host, uint8_t *out, int64_t out_stride, void *stream)
{
    const char *who = "tfilter_frames";
    GSVC_REQUIRE(frames && flows && q_host && wt_host && lut_b_host && lut_p_host && out, "tfilter_frames: NULL pointer");
    const FrameBufs bufs{"strides", frames, stride, out, out_stride};
    GSVC_FRAMES_TRY(tfilter_check_frames(who, bufs, n, GSVC_FRAMES_MAX_BATCH, H, W, layout, depth));
    GSVC_REQUIRE(T >= 1 && T <= 65535, "tfilter_frames: T must be 1 .. 65535 (got %d)", (int)T);
    GSVC_REQUIRE(first >= 0 && (int64_t)first + n <= T, "tfilter_frames: targets %d .. %lld lie outside the %d frames", (int)first,
                 (long long)first + n - 1, (int)T);
    GSVC_REQUIRE((reinterpret_cast<uintptr_t>(flows) & 3) == 0, "tfilter_frames: flows is not 4-byte aligned");
    const int64_t bytes = gsvc_frames_bytes(H, W, layout, depth);
    const uintptr_t f0 = reinterpret_cast<uintptr_t>(frames), f1 = f0 + (uintptr_t)(T - 1) * (uintptr_t)stride + (uintptr_t)bytes;
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(out), o1 = o0 + (uintptr_t)(n - 1) * (uintptr_t)out_stride + (uintptr_t)bytes;
    GSVC_REQUIRE(o1 <= f0 || f1 <= o0, "tfilter_frames: out overlaps the frames (the filter reads neighbours: it cannot work in place)");
    TfArgs g = {};
    for (int p = 0; p < 3; p++) {
        GSVC_REQUIRE(q_host[p] >= 1 && q_host[p] <= 65535, "tfilter_frames: q of plane %d must be 1 .. 65535 (got %u)", p, (unsigned)q_host[p]);
        g.q[p] = q_host[p];
    }
    for (int i = 0; i < 2; i++) {
        GSVC_REQUIRE(wt_host[i] <= TF_WEIGHT_MAX, "tfilter_frames: wt[%d] must be 0 .. 256 (got %u)", i, (unsigned)wt_host[i]);
        g.wt[i] = wt_host[i];
    }
    for (int i = 0; i < TF_LUT; i++) {
        GSVC_REQUIRE(lut_b_host[i] <= TF_WEIGHT_MAX && lut_p_host[i] <= TF_WEIGHT_MAX, "tfilter_frames: table entry %d must be 0 .. 256", i);
        g.lut_b[i] = lut_b_host[i];
        g.lut_p[i] = lut_p_host[i];
    }
    const bool sub = layout == GSVC_FRAMES_YUV420P;
    g.frames = frames; g.stride = stride;
    g.out = out; g.out_stride = out_stride;
    g.flows = flows;
    g.T = T; g.first = first;
    g.H = H; g.W = W;
    g.ch = sub ? H / 2 : H; g.cw = sub ? W / 2 : W;
    g.sub = sub;
    g.nbx = (W + 7) / 8;
    g.nblocks = g.nbx * ((H + 7) / 8);
    g.qq = (unsigned long long)g.q[0] * g.q[0];
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((g.nblocks + 3) / 4), (unsigned)n);
    ProfScope _p("k_tfilter", s);
    if (depth > 8) hipLaunchKernelGGL(k_tfilter<2>, grid, dim3(256), 0, s, g);
    else hipLaunchKernelGGL(k_tfilter<1>, grid, dim3(256), 0, s, g);
    return check_launch(who);
}

extern "C" int gsvc_noise_sums(const uint8_t *frames, int64_t stride, int32_t n, int32_t H, int32_t W, int32_t layout, int32_t depth,
                               uint64_t *out, void *stream)
{
    const char *who = "noise_sums";
    GSVC_REQUIRE(frames && out, "noise_sums: NULL pointer");
    const FrameBufs bufs{"stride", frames, stride, nullptr, 0};
    GSVC_FRAMES_TRY(tfilter_check_frames(who, bufs, n, GSVC_FRAMES_MAX_BATCH, H, W, layout, depth));
    GSVC_REQUIRE((reinterpret_cast<uintptr_t>(out) & 7) == 0, "noise_sums: out is not 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (gsvc::zero_words_async(out, (size_t)n * 3 * sizeof(uint64_t), s) != hipSuccess) {
        set_error("noise_sums: zeroing failed");
        return GSVC_E_LAUNCH;
    }
    const bool sub = layout == GSVC_FRAMES_YUV420P;
    NoiseArgs g = {};
    g.frames = frames; g.stride = stride;
    g.H = H; g.W = W;
    g.ch = sub ? H / 2 : H; g.cw = sub ? W / 2 : W;
    g.chunks_y = (g.W + 255) / 256;
    g.chunks_c = (g.cw + 255) / 256;
    g.groups_y = (g.H + NS_ROWS - 1) / NS_ROWS;
    g.groups_c = (g.ch + NS_ROWS - 1) / NS_ROWS;
    g.out = reinterpret_cast<unsigned long long *>(out);
    const dim3 grid((unsigned)(g.groups_y * g.chunks_y + 2 * g.groups_c * g.chunks_c), (unsigned)n);          // <= 3 * 2048 * 128
    ProfScope _p("k_noise_sums", s);
    if (depth > 8) hipLaunchKernelGGL(k_noise_sums<2>, grid, dim3(256), 0, s, g);
    else hipLaunchKernelGGL(k_noise_sums<1>, grid, dim3(256), 0, s, g);
    return check_launch(who);
}
