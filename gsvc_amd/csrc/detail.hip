// gsvc_amd/csrc/detail.hip — where a clip has detail, and initial anchor points drawn from that, gfx950.  Replaces the
// uniform draw of the reference's init_point_cloud (frame_cube/utils.py:6-15) when a fit asks for init="detail" (gsvc_amd/detail.py).
//
// gsvc_frames_detail   one launch for the n_out frames of a buffer (frame = blockIdx.z): out[f, cy, cx] = the sum over the pixels of cell
//   (cy, cx) of e = gx + gy + 2 gt on the luma codes as they are, gx / gy = the absolute central differences with replicated borders,
//   gt = the absolute difference to the temporal neighbour (f + 1, or f - 1 for the last of n frames, none for n = 1).
//     A workgroup of 256 owns a tile of 128 x 32 pixels = whole cells for every cell size (4, 8, 16), so every output is written once by
//       a plain store: no atomics, no zero-fill.
//     The tile and its one-pixel halo (frame f) and the tile alone (the neighbour) are staged in LDS as 16-bit codes; that is the only
//       read of HBM.  wide path: 16-byte loads (W, the bases and the stride allow it: every row of the plane then starts 16-byte
//       aligned and a vector lies wholly inside or wholly outside the picture), the halo columns one sample each.  edge path: one sample
//       per load, any W, any alignment.  Both leave the same LDS behind; what follows is one body.  (A vector's samples are stored as
//       packed 64-bit words: column 0 sits at LDS index 4.  One 16-bit store per sample cost 7 - 29 % more)
//     A lane sums the 4 x 4 pixels of one block of the tile (32 x 8 blocks = 256 lanes) from LDS; a cell of 8 or 16 is then the sum of
//       2 x 2 or 4 x 4 block sums, which go through LDS once more.  Pixels outside the picture count as nothing.
//   Sums of integers: the same bits for every launch shape and path.  Nothing outside the luma planes of the n frames is read.
//
// gsvc_detail_sample   N points from the inclusive prefix sum of a map: one lane per point, a counter-based hash (splitmix64) for its five
//   random numbers, a binary search in cdf.  The total is read on the device.  include/gsvc_hip.h has the draw in full.
#include "frames_common.h"

namespace gsvc {

constexpr int DT_W = 128, DT_H = 32;                 // the tile of a workgroup, pixels
constexpr int DT_OFF = 4;                            // LDS index of column 0: a vector's samples start 8-byte aligned
constexpr int DT_PITCH = DT_W + 8;                   // LDS row pitch in codes (272 bytes): columns -1 .. 128 at index 3 .. 132
constexpr int DT_BLOCKS_X = DT_W / 4, DT_BLOCKS_Y = DT_H / 4;
static_assert(DT_BLOCKS_X * DT_BLOCKS_Y == 256, "one 4 x 4 block per lane");

struct DetailArgs {
    const uint8_t *frames;
    long long stride;
    uint32_t *out;                     // [n_out, Hc, Wc]
    int n, H, W, cell, Hc, Wc;
};

// rows r0 .. r1 - 1 and columns c0 .. c1 - 1 (relative to the tile's origin (x0, y0)) of a luma plane into LDS, the samples inside the
// picture only; dst(r, c) = lds[(r + 1) * DT_PITCH + c + DT_OFF]
template <int BPS>
__device__ __forceinline__ void stage_samples(uint16_t *lds, const uint8_t *plane, int H, int W, int x0, int y0, int r0, int r1, int c0, int c1)
{
    const int cols = c1 - c0, count = (r1 - r0) * cols;
    for (int i = threadIdx.x; i < count; i += 256) {
        const int r = r0 + i / cols, c = c0 + i % cols;
        const int x = x0 + c, y = y0 + r;
        if (x >= 0 && x < W && y >= 0 && y < H) lds[(r + 1) * DT_PITCH + c + DT_OFF] = (uint16_t)code_at<BPS>(plane, (long long)y * W + x);
    }
}

// the same rows, columns 0 .. DT_W - 1 as 16-byte vectors (W * BPS is a multiple of 16 and the plane 16-byte aligned); LDS is written
// as packed 64-bit words
template <int BPS>
__device__ __forceinline__ void stage_vectors(uint16_t *lds, const uint8_t *plane, int H, int W, int x0, int y0, int r0, int r1)
{
    constexpr int SPV = 16 / BPS, VPR = DT_W / SPV;          // samples of a vector, vectors of a tile row
    const int count = (r1 - r0) * VPR;
    for (int i = threadIdx.x; i < count; i += 256) {
        const int r = r0 + i / VPR, c = (i % VPR) * SPV;
        const int x = x0 + c, y = y0 + r;
        if (x < W && y >= 0 && y < H) {
            uint32_t w[4];
            load_words<16>(plane + ((long long)y * W + x) * BPS, w);
            uint2 *d = reinterpret_cast<uint2 *>(lds + (r + 1) * DT_PITCH + c + DT_OFF);          // 8-byte aligned: c is a multiple of SPV
            if constexpr (BPS == 2) {          // the words are pairs of codes already
                d[0] = make_uint2(w[0], w[1]);
                d[1] = make_uint2(w[2], w[3]);
            } else {                           // four bytes -> two words of two codes
#pragma unroll
                for (int k = 0; k < 4; k++)
                    d[k] = make_uint2((w[k] & 0xFFu) | ((w[k] & 0xFF00u) << 8), ((w[k] >> 16) & 0xFFu) | ((w[k] >> 24) << 16));
            }
        }
    }
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ uint32_t absdiff(uint32_t a, uint32_t b) { return a > b ? a - b : b - a; }

template <int BPS, bool WIDE>
__global__ void __launch_bounds__(256) k_frames_detail(DetailArgs args)
{
    __shared__ __attribute__((aligned(16))) uint16_t cur[(DT_H + 2) * DT_PITCH];          // rows -1 .. 32, columns -1 .. 128 of frame f
    __shared__ __attribute__((aligned(16))) uint16_t nbr[(DT_H + 2) * DT_PITCH];          // rows 0 .. 31, columns 0 .. 127 of the neighbour (the same indexing)
    __shared__ uint32_t blk[DT_BLOCKS_Y][DT_BLOCKS_X];
    const int H = args.H, W = args.W, n = args.n;
    const int f = blockIdx.z, x0 = blockIdx.x * DT_W, y0 = blockIdx.y * DT_H;
    const int g = f + 1 < n ? f + 1 : (n > 1 ? f - 1 : -1);
    const uint8_t *pf = args.frames + (size_t)f * (size_t)args.stride;
    const uint8_t *pg = g >= 0 ? args.frames + (size_t)g * (size_t)args.stride : nullptr;
    if (WIDE) {
        stage_vectors<BPS>(cur, pf, H, W, x0, y0, -1, DT_H + 1);
        stage_samples<BPS>(cur, pf, H, W, x0, y0, -1, DT_H + 1, -1, 0);
        stage_samples<BPS>(cur, pf, H, W, x0, y0, -1, DT_H + 1, DT_W, DT_W + 1);
        if (pg) stage_vectors<BPS>(nbr, pg, H, W, x0, y0, 0, DT_H);
    } else {
        stage_samples<BPS>(cur, pf, H, W, x0, y0, -1, DT_H + 1, -1, DT_W + 1);
        if (pg) stage_samples<BPS>(nbr, pg, H, W, x0, y0, 0, DT_H, 0, DT_W);
    }
    __syncthreads();

    // the 4 x 4 block of this lane; every index below is clamped into the picture, and what of the picture the window of an inside
    // pixel can touch lies within rows -1 .. 32 and columns -1 .. 128 of the tile: staged above
    const int bx = threadIdx.x % DT_BLOCKS_X, by = threadIdx.x / DT_BLOCKS_X;
    const int px = x0 + 4 * bx, py = y0 + 4 * by;
    uint32_t sum = 0;
    if (px < W && py < H) {
        int ci[6], ri[6];
#pragma unroll
        for (int j = 0; j < 6; j++) {
            ci[j] = clampi(px + j - 1, 0, W - 1) - x0 + DT_OFF;
            ri[j] = (clampi(py + j - 1, 0, H - 1) - y0 + 1) * DT_PITCH;
        }
#pragma unroll
        for (int j = 1; j <= 4; j++) {
            if (py + j - 1 < H) {
#pragma unroll
                for (int i = 1; i <= 4; i++) {
                    if (px + i - 1 < W) {
                        const uint32_t gx = absdiff(cur[ri[j] + ci[i + 1]], cur[ri[j] + ci[i - 1]]);
                        const uint32_t gy = absdiff(cur[ri[j + 1] + ci[i]], cur[ri[j - 1] + ci[i]]);
                        const uint32_t gt = pg ? absdiff(nbr[ri[j] + ci[i]], cur[ri[j] + ci[i]]) : 0u;
                        sum += gx + gy + 2u * gt;
                    }
                }
            }
        }
    }
    const int cell = args.cell;
    uint32_t *out = args.out + (size_t)f * (size_t)args.Hc * (size_t)args.Wc;
    if (cell == 4) {
        const int cx = x0 / 4 + bx, cy = y0 / 4 + by;
        if (cx < args.Wc && cy < args.Hc) out[(size_t)cy * args.Wc + cx] = sum;
        return;
    }
    blk[by][bx] = sum;
    __syncthreads();
    const int k = cell / 4, cells_x = DT_W / cell, cells_y = DT_H / cell;          // k x k blocks per cell
    if ((int)threadIdx.x < cells_x * cells_y) {
        const int lx = threadIdx.x % cells_x, ly = threadIdx.x / cells_x;
        const int cx = x0 / cell + lx, cy = y0 / cell + ly;
        if (cx < args.Wc && cy < args.Hc) {
            uint32_t v = 0;
            for (int j = 0; j < k; j++)
                for (int i = 0; i < k; i++) v += blk[ly * k + j][lx * k + i];
            out[(size_t)cy * args.Wc + cx] = v;
        }
    }
}

// ---- the sampler --------------------------------------------------------------------------------------------------------------------
struct SampleArgs {
    const long long *cdf;
    long long cells;
    int T, H, W, cell, Hc, Wc, N;
    unsigned long long seed;
    uint32_t mix24;
    float *points;
    int *cell_of;
};

__device__ __forceinline__ unsigned long long detail_hash(unsigned long long seed, uint32_t i, uint32_t k)
{
    unsigned long long z = seed + (5ull * i + k + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ void __launch_bounds__(256) k_detail_sample(SampleArgs a)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.N) return;
    const uint32_t i = (uint32_t)idx;
    const long long D = a.cdf[a.cells - 1];
    const unsigned long long h1 = detail_hash(a.seed, i, 1);
    int t, x0, y0, cw, ch, at;
    if (D <= 0 || (uint32_t)(detail_hash(a.seed, i, 0) >> 40) < a.mix24) {
        const unsigned long long hw = (unsigned long long)a.H * (unsigned long long)a.W;
        const unsigned long long p = __umul64hi(h1, (unsigned long long)a.T * hw);
        const unsigned long long q = p % hw;
        t = (int)(p / hw);
        y0 = (int)(q / (unsigned)a.W);
        x0 = (int)(q % (unsigned)a.W);
        cw = ch = 1;
        at = (t * a.Hc + y0 / a.cell) * a.Wc + x0 / a.cell;
    } else {
        const long long r = (long long)__umul64hi(h1, (unsigned long long)D);
        long long lo = 0, hi = a.cells;          // the first index with cdf[index] > r
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (a.cdf[mid] > r) hi = mid;
            else lo = mid + 1;
        }
        at = (int)(lo < a.cells ? lo : a.cells - 1);          // (r < D = cdf[cells - 1]; a cdf that is none must not index outside)
        const int per = a.Hc * a.Wc, in = at % per;
        t = at / per;
        y0 = (in / a.Wc) * a.cell;
        x0 = (in % a.Wc) * a.cell;
        cw = min(a.cell, a.W - x0);
        ch = min(a.cell, a.H - y0);
    }
    const float k24 = 1.0f / 16777216.0f;
    const float f2 = (float)(uint32_t)(detail_hash(a.seed, i, 2) >> 40) * k24;
    const float f3 = (float)(uint32_t)(detail_hash(a.seed, i, 3) >> 40) * k24;
    const float f4 = (float)(uint32_t)(detail_hash(a.seed, i, 4) >> 40) * k24;
    a.points[3 * idx + 0] = fmaf(f2, (float)cw, (float)x0);
    a.points[3 * idx + 1] = fmaf(f3, (float)ch, (float)y0);
    a.points[3 * idx + 2] = (f4 - 0.5f) + (float)t;
    a.cell_of[idx] = at;
}

}  // namespace gsvc

using namespace gsvc;

extern "C" int gsvc_frames_detail(const uint8_t *frames, int64_t stride, int32_t n, int32_t n_out, int32_t H, int32_t W, int32_t layout,
                                  int32_t depth, int32_t cell, uint32_t *out, void *stream)
{
    const char *who = "frames_detail";
    GSVC_REQUIRE(frames && out, "%s: NULL pointer", who);
    GSVC_REQUIRE(layout != GSVC_FRAMES_RGB24, "%s: rgb24 frames hold no luma plane", who);
    GSVC_FRAMES_TRY(frames_check_format(who, n, 65535, layout, depth, 8, 16));
    GSVC_REQUIRE(depth == 8 || depth == 10 || depth == 12 || depth == 16, "%s: depth must be 8, 10, 12 or 16 (got %d)", who, (int)depth);
    GSVC_REQUIRE(cell == 4 || cell == 8 || cell == 16, "%s: cell must be 4, 8 or 16 (got %d)", who, (int)cell);
    GSVC_REQUIRE(n_out >= 1 && n_out <= n, "%s: n_out must be 1 .. n = %d (got %d)", who, (int)n, (int)n_out);
    GSVC_FRAMES_TRY(frames_check_size(who, H, W, layout));
    const FrameBufs bufs{"stride", frames, stride, nullptr, 0};
    GSVC_FRAMES_TRY(frames_check_strides(who, bufs, gsvc_frames_bytes(H, W, layout, depth)));
    const bool deep = depth > 8;
    if (deep) GSVC_FRAMES_TRY(frames_check_even(who, bufs));
    GSVC_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3) == 0, "%s: out is not 4-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    const int Hc = (H + cell - 1) / cell, Wc = (W + cell - 1) / cell;
    const DetailArgs g = {frames, stride, out, n, H, W, cell, Hc, Wc};
    const bool wide = (bufs.alignment(n) & 15) == 0 && ((int64_t)W * (deep ? 2 : 1)) % 16 == 0;
    const dim3 grid((unsigned)((W + DT_W - 1) / DT_W), (unsigned)((H + DT_H - 1) / DT_H), (unsigned)n_out);
    static void (*const kernels[2][2])(DetailArgs) = {{k_frames_detail<1, false>, k_frames_detail<1, true>},
                                                      {k_frames_detail<2, false>, k_frames_detail<2, true>}};
    ProfScope _p("k_frames_detail", s);
    hipLaunchKernelGGL(kernels[deep][wide], grid, dim3(256), 0, s, g);
    return check_launch(who);
}

extern "C" int gsvc_detail_sample(const int64_t *cdf, int64_t cells, int32_t T, int32_t H, int32_t W, int32_t cell, int32_t N, uint64_t seed,
                                  uint32_t mix24, float *points, int32_t *cell_of, void *stream)
{
    const char *who = "detail_sample";
    GSVC_REQUIRE(cdf && points && cell_of, "%s: NULL pointer", who);
    GSVC_REQUIRE(T >= 1 && T <= 65535, "%s: T must be 1 .. 65535 (got %d)", who, (int)T);
    GSVC_REQUIRE(H >= 1 && W >= 1 && H <= 32768 && W <= 32768, "%s: image size must be 1 .. 32768 (got %d x %d)", who, (int)H, (int)W);
    GSVC_REQUIRE(cell == 4 || cell == 8 || cell == 16, "%s: cell must be 4, 8 or 16 (got %d)", who, (int)cell);
    const int64_t Hc = (H + cell - 1) / cell, Wc = (W + cell - 1) / cell;
    GSVC_REQUIRE(cells == (int64_t)T * Hc * Wc, "%s: cells must be T Hc Wc = %lld (got %lld)", who, (long long)((int64_t)T * Hc * Wc),
                 (long long)cells);
    GSVC_REQUIRE(cells < ((int64_t)1 << 31), "%s: a map of %lld cells is too large (2^31 and more)", who, (long long)cells);
    GSVC_REQUIRE(mix24 <= (1u << 24), "%s: mix24 must be 0 .. 2^24 (got %u)", who, (unsigned)mix24);
    GSVC_REQUIRE(N >= 1, "%s: N must be positive (got %d)", who, (int)N);
    GSVC_REQUIRE((reinterpret_cast<uintptr_t>(cdf) & 7) == 0 && ((reinterpret_cast<uintptr_t>(points) | reinterpret_cast<uintptr_t>(cell_of)) & 3) == 0,
                 "%s: cdf must be 8-byte, points and cell_of 4-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    const SampleArgs a = {reinterpret_cast<const long long *>(cdf), cells, T, H, W, cell, (int)Hc, (int)Wc, N, seed, mix24, points, cell_of};
    ProfScope _p("k_detail_sample", s);
    hipLaunchKernelGGL(k_detail_sample, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, a);
    return check_launch(who);
}
