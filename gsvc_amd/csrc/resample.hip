// gsvc_amd/csrc/resample.hip — Lanczos-3 resampler on the sample codes of planar Y'CbCr frames, gfx950.  Integers
// only; the arithmetic is stated sample by sample in include/gsvc_hip.h and gsvc_amd/resample.py, the taps are built on the host
// (resample.filter_taps) and arrive as device arrays: per output index a first source index and up to RS_TAPS Q14 coefficients.
//
// gsvc_resample_frames  k_resample<BPS> (BPS = bytes per sample: one body for 8-bit and deep frames).  One launch covers the three planes
//   of up to 16 frames.  A workgroup of 256 threads owns a tile of RS_TW x RS_TH output samples of one plane of one frame:
//     1. it copies the tile's coefficient rows into LDS, transposed to [tap][column] for the horizontal table so that the 64 lanes of a
//        wave read 64 adjacent int16 (conflict-free), [row][tap] for the vertical one (every lane of a wave reads the same word: a
//        broadcast);
//     2. horizontal pass: the source rows the tile needs, first_y[tile's first row] .. first_y[its last row] + nt_y - 1 (at most
//        RS_ROWS = 88: 15 * 4 + 24 at ratio 4, rounded up), each clamped into the plane, are filtered into LDS as int32
//        m[row][column]: lane = column, wave = row mod 4.  A wave's 64 lanes read source samples that lie within 64 * ratio + 24
//        adjacent samples of one row: the loads of one tap are 1 .. 4 samples apart and every sample is read by nt / ratio lanes out of
//        the same lines of the vector cache; nothing but the frame itself is read from memory and the intermediate never goes there;
//     3. vertical pass: lane = column, each wave four of the sixteen rows; a lane reads m down its column (adjacent lanes, adjacent
//        words: conflict-free), accumulates in 64 bits (v_mad_i64_i32) and writes its sample once by a plain store.
//   The tap loops run to the table's nt (6 for an upscale); slots at or beyond it are never read.  No atomics, no workspace; the result
//   does not depend on the launch geometry.  Every index derived from a table is clamped — the source column and row into the plane, the
//   LDS row into the rows this workgroup filled — so no table content can make the kernel read outside a plane or its own LDS.
#include "frames_common.h"

namespace gsvc {

constexpr int RS_TAPS = 24;            // slots per coefficient row (GSVC_RESAMPLE_TAPS)
constexpr int RS_TW = 64;              // tile: output columns (one per lane of a wave)
constexpr int RS_TH = 16;              // tile: output rows
constexpr int RS_ROWS = 88;            // source rows a tile can need: (RS_TH - 1) * 4 + RS_TAPS = 84, rounded up to a multiple of 4

struct RsTable {
    const int32_t *first;              // [dst]
    const int16_t *coef;               // [dst, RS_TAPS]
    int nt;
};

struct RsArgs {
    const uint8_t *src;
    long long src_stride;
    uint8_t *dst;
    long long dst_stride;
    int H, W, ch, cw;                  // source: the luma and the chroma plane
    int oH, oW, och, ocw;              // output
    int tiles_x[2], tiles[2];          // tiles per tile row / per plane: [0] luma, [1] a chroma plane
    int depth;
    RsTable x[2], y[2];                // [0] luma, [1] chroma
};

template <int BPS>
__global__ void __launch_bounds__(256) k_resample(RsArgs a)
{
    __shared__ int32_t s_m[RS_ROWS][RS_TW];               // 22 KiB
    __shared__ int16_t s_cx[RS_TAPS][RS_TW];              // 3 KiB
    __shared__ int16_t s_cy[RS_TH][RS_TAPS];

    // blockIdx.x: the tiles of Y, then those of U, then those of V (uniform in the workgroup)
    int b = (int)blockIdx.x, p = 0;
    if (b >= a.tiles[0]) {
        b -= a.tiles[0];
        p = 1;
        if (b >= a.tiles[1]) {
            b -= a.tiles[1];
            p = 2;
        }
    }
    const int c = p ? 1 : 0;
    const int sw = c ? a.cw : a.W, sh = c ? a.ch : a.H, ow = c ? a.ocw : a.oW, oh = c ? a.och : a.oH;
    const int ty = b / a.tiles_x[c], tx = b - ty * a.tiles_x[c];
    const int x0 = tx * RS_TW, y0 = ty * RS_TH;
    const int ntx = a.x[c].nt, nty = a.y[c].nt;
    const long long s_off = p == 0 ? 0ll : (long long)a.H * a.W + (p == 2 ? (long long)a.ch * a.cw : 0ll);
    const long long d_off = p == 0 ? 0ll : (long long)a.oH * a.oW + (p == 2 ? (long long)a.och * a.ocw : 0ll);
    const uint8_t *splane = a.src + (size_t)blockIdx.y * (size_t)a.src_stride + s_off * BPS;
    uint8_t *dplane = a.dst + (size_t)blockIdx.y * (size_t)a.dst_stride + d_off * BPS;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // ---- 1. the tile's coefficients (columns and rows beyond the plane: those of its last column / row, never used for a store)
    for (int i = tid; i < RS_TW * ntx; i += 256) {
        const int col = i / ntx, k = i - col * ntx;
        s_cx[k][col] = a.x[c].coef[(long long)min(x0 + col, ow - 1) * RS_TAPS + k];
    }
    for (int i = tid; i < RS_TH * nty; i += 256) {
        const int row = i / nty, k = i - row * nty;
        s_cy[row][k] = a.y[c].coef[(long long)min(y0 + row, oh - 1) * RS_TAPS + k];
    }
    const int ylast = min(y0 + RS_TH, oh) - 1;
    const int rbase = a.y[c].first[y0];
    const int rows = min(max(a.y[c].first[ylast] + nty - rbase, 1), RS_ROWS);
    const int fx = a.x[c].first[min(x0 + lane, ow - 1)];
    __syncthreads();

    // ---- 2. horizontal: m(r, j) = (sum_k cx[j, k] a(clamp(rbase + r), clamp(fx[j] + k)) + 2^(d - 3)) >> (d - 2)
    const int hshift = a.depth - 2, hround = 1 << (a.depth - 3);
    for (int r = wave; r < rows; r += 4) {
        const int sy = min(max(rbase + r, 0), sh - 1);
        const uint8_t *row = splane + (long long)sy * sw * BPS;
        uint32_t t = 0u;                                  // two's complement: |t| < 2^31 for every table filter_taps builds
        for (int k = 0; k < ntx; k++) {
            const int sx = min(max(fx + k, 0), sw - 1);
            t += (uint32_t)((int)s_cx[k][lane] * (int)code_at<BPS>(row, sx));
        }
        s_m[r][lane] = ((int32_t)t + hround) >> hshift;
    }
    __syncthreads();

    // ---- 3. vertical: out = clamp((sum_k cy[i, k] m(fy[i] + k, j) + 2^(29 - d)) >> (30 - d), 0, 2^d - 1)
    const int vshift = 30 - a.depth, peak = (1 << a.depth) - 1;
    const long long vround = 1ll << (29 - a.depth);
    const int x = x0 + lane;
#pragma unroll
    for (int q = 0; q < RS_TH / 4; q++) {
        const int i = wave + 4 * q, y = y0 + i;
        if (y >= oh) break;                               // (wave-uniform)
        const int r0 = a.y[c].first[y] - rbase;
        long long u = 0ll;
        for (int k = 0; k < nty; k++) {
            const int r = min(max(r0 + k, 0), rows - 1);
            u += (long long)s_cy[i][k] * (long long)s_m[r][lane];
        }
        const long long v = (u + vround) >> vshift;
        const uint32_t code = (uint32_t)(v < 0 ? 0ll : (v > peak ? (long long)peak : v));
        if (x < ow) {
            const long long at = (long long)y * ow + x;
            if (BPS == 1) dplane[at] = (uint8_t)code;
            else reinterpret_cast<uint16_t *>(dplane)[at] = (uint16_t)code;
        }
    }
}

static int resample_check_side(const char *who, const char *what, int32_t src, int32_t dst)
{
    GSVC_REQUIRE(src >= 2 && dst >= 2, "%s: %s must be at least 2 (got %d -> %d)", who, what, (int)src, (int)dst);
    GSVC_REQUIRE((int64_t)src <= 4 * (int64_t)dst && (int64_t)dst <= 4 * (int64_t)src, "%s: %s changes by more than a ratio of 4 (%d -> %d)",
                 who, what, (int)src, (int)dst);
    return GSVC_OK;
}

}  // namespace gsvc

using namespace gsvc;

extern "C" int gsvc_resample_frames(const uint8_t *src, int64_t src_stride, int32_t n, int32_t H, int32_t W, int32_t layout, int32_t depth,
                                    uint8_t *dst, int64_t dst_stride, int32_t out_H, int32_t out_W,
                                    const int32_t *lx_first, const int16_t *lx_coef, int32_t lx_nt,
                                    const int32_t *ly_first, const int16_t *ly_coef, int32_t ly_nt,
                                    const int32_t *cx_first, const int16_t *cx_coef, int32_t cx_nt,
                                    const int32_t *cy_first, const int16_t *cy_coef, int32_t cy_nt, void *stream)
{
    const char *who = "resample_frames";
    GSVC_REQUIRE(src && dst && lx_first && lx_coef && ly_first && ly_coef && cx_first && cx_coef && cy_first && cy_coef,
                 "resample_frames: NULL pointer");
    GSVC_REQUIRE(layout != GSVC_FRAMES_RGB24, "resample_frames: rgb24 frames are not resampled (the filter works on planar Y'CbCr codes)");
    GSVC_FRAMES_TRY(frames_check_format(who, n, GSVC_FRAMES_MAX_BATCH, layout, depth, 8, 16));
    GSVC_REQUIRE(depth == 8 || depth == 10 || depth == 12 || depth == 16, "resample_frames: depth must be 8, 10, 12 or 16 (got %d)", (int)depth);
    GSVC_FRAMES_TRY(frames_check_size(who, H, W, layout));
    GSVC_FRAMES_TRY(frames_check_size(who, out_H, out_W, layout));
    GSVC_FRAMES_TRY(resample_check_side(who, "the height", H, out_H));
    GSVC_FRAMES_TRY(resample_check_side(who, "the width", W, out_W));
    const int32_t nts[4] = {lx_nt, ly_nt, cx_nt, cy_nt};
    for (int i = 0; i < 4; i++)
        GSVC_REQUIRE(nts[i] >= 1 && nts[i] <= RS_TAPS, "resample_frames: nt must be 1 .. %d (got %d)", RS_TAPS, (int)nts[i]);
    const int64_t in_bytes = gsvc_frames_bytes(H, W, layout, depth), out_bytes = gsvc_frames_bytes(out_H, out_W, layout, depth);
    const FrameBufs in_buf{"src_stride", src, src_stride, nullptr, 0}, out_buf{"dst_stride", dst, dst_stride, nullptr, 0};
    GSVC_FRAMES_TRY(frames_check_strides(who, in_buf, in_bytes));
    GSVC_FRAMES_TRY(frames_check_strides(who, out_buf, out_bytes));
    if (depth > 8) {
        GSVC_FRAMES_TRY(frames_check_even(who, in_buf));
        GSVC_FRAMES_TRY(frames_check_even(who, out_buf));
    }
    const uintptr_t f0 = reinterpret_cast<uintptr_t>(src), f1 = f0 + (uintptr_t)(n - 1) * (uintptr_t)src_stride + (uintptr_t)in_bytes;
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(dst), o1 = o0 + (uintptr_t)(n - 1) * (uintptr_t)dst_stride + (uintptr_t)out_bytes;
    GSVC_REQUIRE(o1 <= f0 || f1 <= o0, "resample_frames: dst overlaps src (a tile reads source rows other tiles' outputs would replace)");
    const uintptr_t t4 = reinterpret_cast<uintptr_t>(lx_first) | reinterpret_cast<uintptr_t>(ly_first) | reinterpret_cast<uintptr_t>(cx_first) |
                         reinterpret_cast<uintptr_t>(cy_first);
    const uintptr_t t2 = reinterpret_cast<uintptr_t>(lx_coef) | reinterpret_cast<uintptr_t>(ly_coef) | reinterpret_cast<uintptr_t>(cx_coef) |
                         reinterpret_cast<uintptr_t>(cy_coef);
    GSVC_REQUIRE((t4 & 3) == 0 && (t2 & 1) == 0, "resample_frames: a table is not aligned to its element");
    const bool sub = layout == GSVC_FRAMES_YUV420P;
    RsArgs g = {};
    g.src = src; g.src_stride = src_stride;
    g.dst = dst; g.dst_stride = dst_stride;
    g.H = H; g.W = W;
    g.ch = sub ? H / 2 : H; g.cw = sub ? W / 2 : W;
    g.oH = out_H; g.oW = out_W;
    g.och = sub ? out_H / 2 : out_H; g.ocw = sub ? out_W / 2 : out_W;
    g.tiles_x[0] = (g.oW + RS_TW - 1) / RS_TW;
    g.tiles_x[1] = (g.ocw + RS_TW - 1) / RS_TW;
    g.tiles[0] = g.tiles_x[0] * ((g.oH + RS_TH - 1) / RS_TH);
    g.tiles[1] = g.tiles_x[1] * ((g.och + RS_TH - 1) / RS_TH);
    g.depth = depth;
    g.x[0] = RsTable{lx_first, lx_coef, lx_nt};
    g.y[0] = RsTable{ly_first, ly_coef, ly_nt};
    g.x[1] = RsTable{cx_first, cx_coef, cx_nt};
    g.y[1] = RsTable{cy_first, cy_coef, cy_nt};
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(g.tiles[0] + 2 * g.tiles[1]), (unsigned)n);          // <= 3 * 512 * 2048
    ProfScope _p("k_resample", s);
    if (depth > 8) hipLaunchKernelGGL(k_resample<2>, grid, dim3(256), 0, s, g);
    else hipLaunchKernelGGL(k_resample<1>, grid, dim3(256), 0, s, g);
    return check_launch(who);
}
