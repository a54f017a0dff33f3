// gsvc_amd/csrc/grain.hip — film grain (section GRAN of the bitstream file), gfx950: synthesis on the delivered Y'CbCr
// frames, and the flat-block statistics of (source, decoded) the encoder fits its parameters to.  Integers only; the arithmetic is
// stated sample by sample in include/gsvc_hip.h and gsvc_amd/grain.py.
//
// gsvc_grain_apply   k_grain_apply<BPS> (BPS = bytes per sample: one body for 8-bit and deep frames).  A workgroup owns one 128 x 16
//   luma tile of one frame and the chroma tiles under it (64 x 8 each for 4:2:0, 128 x 16 for 4:4:4).  It reads its luma codes once,
//   into LDS; then plane by plane it hashes the white noise of tile + 1 halo into LDS (the halo is hash, not memory: one 64-bit
//   splitmix64 gives two horizontally adjacent samples), filters with the two 3-tap kernels out of LDS, looks the strength up at the
//   UNGRAINED luma of its own tile, adds, clamps and stores.  A lane takes 4 adjacent samples: one 4- or 8-byte store, contiguous across
//   a tile row (the narrow path, for widths and bases that do not allow it, stores them one by one).  Nothing outside the tile is read,
//   so the call works in place.  The frame index comes from the kernel arguments: the noise does not depend on the launch geometry.
// gsvc_grain_stats   k_grain_stats<BPS>: a wave takes GS_BLOCKS_PER_WAVE 8 x 8 blocks, one after the other, a lane per sample; the
//   neighbours come by shuffles, the per-block sums by the wave sums of reduce.h.  The (plane, bin) rows of a workgroup are summed in
//   LDS by 64-bit integer atomics and flushed by one global 64-bit atomic per non-zero entry: integer sums, the same bits in any order.
#include "frames_common.h"
#include "reduce.h"

namespace gsvc {

constexpr int GR_TW = 128, GR_TH = 16;               // the luma tile of a workgroup
constexpr int GR_NP = GR_TW + 4;                     // LDS pitch of the noise rows in samples: columns -1 .. 128 at index 0 .. 129
constexpr unsigned long long GR_GOLD = 0x9E3779B97F4A7C15ull;

__host__ __device__ __forceinline__ unsigned long long gr_mix(unsigned long long z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the sum of the four bytes of w, minus 510
__device__ __forceinline__ int gr_noise(uint32_t w)
{
    return (int)((w & 255u) + ((w >> 8) & 255u) + ((w >> 16) & 255u) + (w >> 24)) - 510;
}

struct GrainApplyArgs {
    uint8_t *frames;
    long long stride;
    unsigned long long seed;
    int H, W, ch, cw;                  // the luma and the chroma plane
    int sub;                           // 1: 4:2:0
    int shift;                         // depth - 8
    int lo_y, hi_y, lo_c, hi_c;        // the nominal ranges
    int vec[3];                        // per plane: 4 samples at once (the plane's width, its first sample, the base and the stride allow it)
    int kx[3], ky[3];
    uint32_t fid[GSVC_FRAMES_MAX_BATCH];
    uint16_t scale[52];                // [3][17]
};

// 4 samples of a plane row from / to memory, as one access or one by one (k < valid)
template <int BPS>
__device__ __forceinline__ void gr_load4(const uint8_t *p, bool vec, int valid, uint32_t c[4])
{
    if (vec) {
        uint32_t w[BPS];
        load_words<4 * BPS>(p, w);
#pragma unroll
        for (int k = 0; k < 4; k++) c[k] = code_of<BPS>(w, k);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) c[k] = k < valid ? code_at<BPS>(p, k) : 0u;
    }
}

template <int BPS>
__device__ __forceinline__ void gr_store4(uint8_t *p, bool vec, int valid, const uint32_t c[4])
{
    if (vec) {
        uint32_t w[BPS];
        if (BPS == 1) {
            w[0] = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
        } else {
            w[0] = c[0] | (c[1] << 16);
            w[BPS - 1] = c[2] | (c[3] << 16);
        }
        store_words<4 * BPS>(p, w);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (k < valid) {
                if (BPS == 1) p[k] = (uint8_t)c[k];
                else reinterpret_cast<uint16_t *>(p)[k] = (uint16_t)c[k];
            }
        }
    }
}

template <int BPS>
__global__ void __launch_bounds__(256) k_grain_apply(GrainApplyArgs a)
{
    __shared__ uint16_t s_luma[GR_TH][GR_TW];            // the tile's ungrained luma codes (0 outside the picture)
    __shared__ int16_t s_noise[GR_TH + 2][GR_NP];        // g of the plane in hand: rows -1 .. th, columns -1 .. tw
    __shared__ uint16_t s_scale[52];
    const int tid = threadIdx.x;
    uint8_t *frame = a.frames + (size_t)blockIdx.z * (size_t)a.stride;
    const unsigned long long fbase = a.seed + (3ull * a.fid[blockIdx.z] + 1ull) * GR_GOLD;
    const int x0 = blockIdx.x * GR_TW, y0 = blockIdx.y * GR_TH;
    if (tid < 52) s_scale[tid] = a.scale[tid];

    // ---- the luma codes of the tile, once
    uint32_t luma[2][4];
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int u = tid + 256 * j, row = u >> 5, ux = u & 31;
        const int x = x0 + 4 * ux, y = y0 + row;
        luma[j][0] = luma[j][1] = luma[j][2] = luma[j][3] = 0u;
        if (y < a.H && x < a.W) gr_load4<BPS>(frame + ((long long)y * a.W + x) * BPS, a.vec[0] != 0, a.W - x, luma[j]);
        uint32_t *dst = reinterpret_cast<uint32_t *>(&s_luma[row][4 * ux]);
        dst[0] = luma[j][0] | (luma[j][1] << 16);
        dst[1] = luma[j][2] | (luma[j][3] << 16);
    }

    for (int p = 0; p < 3; p++) {
        const bool sub = p > 0 && a.sub;
        const int pw = p ? a.cw : a.W, ph = p ? a.ch : a.H;
        const int px0 = sub ? x0 >> 1 : x0, py0 = sub ? y0 >> 1 : y0;
        const int tw = min(sub ? GR_TW / 2 : GR_TW, pw - px0), th = min(sub ? GR_TH / 2 : GR_TH, ph - py0);
        const long long poff = p == 0 ? 0ll : (long long)a.H * a.W + (p == 2 ? (long long)a.ch * a.cw : 0ll);
        const unsigned long long key = gr_mix(fbase + (unsigned long long)p * GR_GOLD);
        __syncthreads();                                  // s_luma and s_scale are written; the plane before is done with s_noise
        // ---- white noise of tile + halo: sample (y, x) sits at s_noise[y - py0 + 1][x - px0 + 1]; px0 is even, so a pair of the
        //      hash's ((x + 1) >> 1) is two adjacent columns 2 j, 2 j + 1
        const int npairs = (tw + 3) >> 1, nhash = npairs * (th + 2);
        for (int i = tid; i < nhash; i += 256) {
            const int rr = i / npairs, j = i - rr * npairs;
            const unsigned long long ctr = ((unsigned long long)(uint32_t)(py0 + rr) << 32) | (unsigned long long)(uint32_t)((px0 >> 1) + j);
            const unsigned long long h = gr_mix(key + ctr * GR_GOLD);
            const int g0 = gr_noise((uint32_t)h), g1 = gr_noise((uint32_t)(h >> 32));
            *reinterpret_cast<uint32_t *>(&s_noise[rr][2 * j]) = (uint32_t)(g0 & 0xFFFF) | ((uint32_t)g1 << 16);
        }
        __syncthreads();
        // ---- filter, strength, add, clamp, store: a lane takes 4 adjacent samples of a row
        const int upr_shift = sub ? 4 : 5;               // units per tile row: 16 or 32
        const int units = th << upr_shift;
        const int kx = a.kx[p], ky = a.ky[p];
        const int lo = p ? a.lo_c : a.lo_y, hi = p ? a.hi_c : a.hi_y;
        const bool vec = a.vec[p] != 0;
        const uint16_t *sc = s_scale + 17 * p;
        const int S = 16 - a.shift;
        for (int u = tid; u < units; u += 256) {
            const int row = u >> upr_shift, ux = u & ((1 << upr_shift) - 1);
            const int x = px0 + 4 * ux, y = py0 + row;
            if (x >= pw) continue;
            uint8_t *at = frame + (poff + (long long)y * pw + x) * BPS;
            uint32_t c[4];
            if (p == 0) {
                const uint32_t *src = reinterpret_cast<const uint32_t *>(&s_luma[row][4 * ux]);
                c[0] = src[0] & 65535u; c[1] = src[0] >> 16; c[2] = src[1] & 65535u; c[3] = src[1] >> 16;
            } else {
                gr_load4<BPS>(at, vec, pw - x, c);
            }
            int t[3][4];
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const uint32_t *nw = reinterpret_cast<const uint32_t *>(&s_noise[row + r][4 * ux]);
                const uint32_t w0 = nw[0], w1 = nw[1], w2 = nw[2];
                const int g[6] = {(int)(int16_t)(w0 & 65535u), (int)w0 >> 16, (int)(int16_t)(w1 & 65535u), (int)w1 >> 16,
                                  (int)(int16_t)(w2 & 65535u), (int)w2 >> 16};
#pragma unroll
                for (int k = 0; k < 4; k++) t[r][k] = kx * (g[k] + g[k + 2]) + 64 * g[k + 1];
            }
            uint32_t out[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int nn = (ky * (t[0][k] + t[2][k]) + 64 * t[1][k] + 2048) >> 12;
                uint32_t m;
                if (p == 0) {
                    m = c[k];
                } else if (sub) {
                    const uint32_t top = *reinterpret_cast<const uint32_t *>(&s_luma[2 * row][2 * (4 * ux + k)]);
                    const uint32_t bot = *reinterpret_cast<const uint32_t *>(&s_luma[2 * row + 1][2 * (4 * ux + k)]);
                    m = ((top & 65535u) + (top >> 16) + (bot & 65535u) + (bot >> 16) + 2u) >> 2;
                } else {
                    m = s_luma[row][4 * ux + k];
                }
                const uint32_t l = min(m >> a.shift, 255u);
                const uint32_t i = l >> 4, r = l & 15u;
                const int s = (int)(((uint32_t)sc[i] * (16u - r) + (uint32_t)sc[i + 1] * r + 8u) >> 4);
                const int grain = (nn * s + (1 << (S - 1))) >> S;
                const int code = (int)c[k];
                out[k] = (uint32_t)min(max(code + grain, min(lo, code)), max(hi, code));
            }
            gr_store4<BPS>(at, vec, pw - x, out);
        }
    }
}

// ============================================================================================================================
// statistics
// ============================================================================================================================
constexpr int GS_BLOCKS_PER_WAVE = 16;
constexpr int GS_ROWS = 3 * 16 * 6;

struct GrainStatsArgs {
    const uint8_t *src, *dec;
    long long src_stride, dec_stride;
    int H, W, ch, cw;
    int sub, shift;
    int nbx_y, nbx_c;                  // 8 x 8 blocks per row of a luma / chroma plane
    long long nb_y, nb_c;              // per plane
    uint32_t flat, max_res;            // the two thresholds at the frames' depth
    unsigned long long *out;
};

template <int BPS>
__global__ void __launch_bounds__(256) k_grain_stats(GrainStatsArgs a)
{
    __shared__ unsigned long long s_rows[GS_ROWS];
    for (int i = threadIdx.x; i < GS_ROWS; i += 256) s_rows[i] = 0ull;
    __syncthreads();
    const uint8_t *src = a.src + (size_t)blockIdx.y * (size_t)a.src_stride;
    const uint8_t *dec = a.dec + (size_t)blockIdx.y * (size_t)a.dec_stride;
    const int lane = threadIdx.x & 63, lx = lane & 7, ly = lane >> 3;
    const long long total = a.nb_y + 2 * a.nb_c;
    const long long first = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * GS_BLOCKS_PER_WAVE;
    const long long stop = min(first + GS_BLOCKS_PER_WAVE, total);
    for (long long b = first; b < stop; b++) {            // (the same trip count in every lane of a wave)
        const int p = (b >= a.nb_y) + (b >= a.nb_y + a.nb_c);
        const long long bi = b - (p == 0 ? 0ll : (p == 1 ? a.nb_y : a.nb_y + a.nb_c));
        const int nbx = p ? a.nbx_c : a.nbx_y, pw = p ? a.cw : a.W;
        const int by = (int)(bi / nbx), bx = (int)(bi - (long long)by * nbx);
        const int x = 8 * bx + lx, y = 8 * by + ly;
        const long long poff = p == 0 ? 0ll : (long long)a.H * a.W + (p == 2 ? (long long)a.ch * a.cw : 0ll);
        const long long at = poff + (long long)y * pw + x;
        const int s = (int)code_at<BPS>(src, at), d = (int)code_at<BPS>(dec, at);
        const int r = s - d;
        const int dx = __shfl_down(d, 1, 64), dy = __shfl_down(d, 8, 64);
        const uint32_t act = (lx < 7 ? (uint32_t)abs(d - dx) : 0u) + (ly < 7 ? (uint32_t)abs(d - dy) : 0u);
        uint32_t lum;
        if (p == 0) {
            lum = (uint32_t)d;
        } else if (a.sub) {
            const long long l0 = (long long)(2 * y) * a.W + 2 * x;
            lum = code_at<BPS>(dec, l0) + code_at<BPS>(dec, l0 + 1) + code_at<BPS>(dec, l0 + a.W) + code_at<BPS>(dec, l0 + a.W + 1);
        } else {
            lum = code_at<BPS>(dec, (long long)y * a.W + x);
        }
        const uint32_t A = wave_sum(act), L = wave_sum(lum);
        const uint32_t worst = wave_max((uint32_t)abs(r));
        if (A > a.flat || worst > a.max_res) continue;    // (wave-uniform)
        const int bin = (int)(min((L >> (p && a.sub ? 8 : 6)) >> a.shift, 255u) >> 4);
        const int rx = __shfl_down(r, 1, 64), ry = __shfl_down(r, 8, 64);
        const long long S1 = (long long)wave_sum(r);
        const long long S2 = wave_sum((long long)r * r);
        const long long Px = wave_sum(lx < 7 ? (long long)r * rx : 0ll);
        const long long Py = wave_sum(ly < 7 ? (long long)r * ry : 0ll);
        if (lane == 0) {
            unsigned long long *row = s_rows + (p * 16 + bin) * 6;
            atomicAdd(row + 0, 1ull);
            atomicAdd(row + 1, (unsigned long long)S1);
            atomicAdd(row + 2, (unsigned long long)S2);
            atomicAdd(row + 3, (unsigned long long)(S1 * S1));
            atomicAdd(row + 4, (unsigned long long)Px);
            atomicAdd(row + 5, (unsigned long long)Py);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < GS_ROWS; i += 256) {
        const unsigned long long v = s_rows[i];
        if (v) atomicAdd(a.out + i, v);
    }
}

static int grain_check_frames(const char *who, const FrameBufs &bufs, int32_t n, int32_t n_max, int32_t H, int32_t W, int32_t layout,
                              int32_t depth)
{
    GSVC_REQUIRE(layout != GSVC_FRAMES_RGB24, "%s: rgb24 frames hold no luma plane (grain lives in the delivered Y'CbCr domain)", who);
    GSVC_FRAMES_TRY(frames_check_format(who, n, n_max, layout, depth, 8, 16));
    GSVC_REQUIRE(depth == 8 || depth == 10 || depth == 12 || depth == 16, "%s: depth must be 8, 10, 12 or 16 (got %d)", who, (int)depth);
    GSVC_FRAMES_TRY(frames_check_size(who, H, W, layout));
    GSVC_FRAMES_TRY(frames_check_strides(who, bufs, gsvc_frames_bytes(H, W, layout, depth)));
    if (depth > 8) GSVC_FRAMES_TRY(frames_check_even(who, bufs));
    return GSVC_OK;
}

}  // namespace gsvc

using namespace gsvc;

extern "C" int gsvc_grain_apply(uint8_t *frames, int64_t stride, int32_t n, int32_t H, int32_t W, int32_t layout, int32_t depth,
                                int32_t range, const gsvc_grain_params *params, const int64_t *frame_ids_host, void *stream)
{
    const char *who = "grain_apply";
    GSVC_REQUIRE(frames && params && frame_ids_host, "grain_apply: NULL pointer");
    const FrameBufs bufs{"stride", frames, stride, nullptr, 0};
    GSVC_FRAMES_TRY(grain_check_frames(who, bufs, n, GSVC_FRAMES_MAX_BATCH, H, W, layout, depth));
    GSVC_REQUIRE(range == GSVC_FRAMES_LIMITED || range == GSVC_FRAMES_FULL, "grain_apply: unknown range %d", (int)range);
    GrainApplyArgs g = {};
    for (int p = 0; p < 3; p++) {
        GSVC_REQUIRE(params->kx[p] >= -32 && params->kx[p] <= 32 && params->ky[p] >= -32 && params->ky[p] <= 32,
                     "grain_apply: the taps of plane %d must lie in -32 .. 32 (got kx %d, ky %d)", p, (int)params->kx[p], (int)params->ky[p]);
        g.kx[p] = params->kx[p];
        g.ky[p] = params->ky[p];
        for (int i = 0; i < 17; i++) g.scale[17 * p + i] = params->scale[p][i];
    }
    for (int k = 0; k < GSVC_FRAMES_MAX_BATCH; k++) {
        const int64_t id = frame_ids_host[k < n ? k : 0];
        GSVC_REQUIRE(id >= 0 && id <= 0xFFFFFFFFll, "grain_apply: frame index %lld is outside 0 .. 2^32 - 1", (long long)id);
        g.fid[k] = (uint32_t)id;
    }
    const bool sub = layout == GSVC_FRAMES_YUV420P;
    const int bps = depth > 8 ? 2 : 1, up = 1 << (depth - 8);
    g.frames = frames;
    g.stride = stride;
    g.seed = params->seed;
    g.H = H; g.W = W;
    g.ch = sub ? H / 2 : H; g.cw = sub ? W / 2 : W;
    g.sub = sub;
    g.shift = depth - 8;
    const bool limited = range == GSVC_FRAMES_LIMITED;
    g.lo_y = g.lo_c = limited ? 16 * up : 0;
    g.hi_y = limited ? 235 * up : (1 << depth) - 1;
    g.hi_c = limited ? 240 * up : (1 << depth) - 1;
    // 4 samples at once: every row of the plane in every frame starts at a multiple of 4 samples from a base aligned to 4 samples
    const uintptr_t base_bits = reinterpret_cast<uintptr_t>(frames) | (n > 1 ? (uintptr_t)stride : 0);
    const bool base_ok = (base_bits & (uintptr_t)(4 * bps - 1)) == 0;
    const int64_t px = (int64_t)H * W, cpx = (int64_t)g.ch * g.cw;
    g.vec[0] = base_ok && W % 4 == 0;
    g.vec[1] = base_ok && g.cw % 4 == 0 && px % 4 == 0;
    g.vec[2] = base_ok && g.cw % 4 == 0 && (px + cpx) % 4 == 0;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((W + GR_TW - 1) / GR_TW), (unsigned)((H + GR_TH - 1) / GR_TH), (unsigned)n);
    ProfScope _p("k_grain_apply", s);
    if (bps == 1) hipLaunchKernelGGL(k_grain_apply<1>, grid, dim3(256), 0, s, g);
    else hipLaunchKernelGGL(k_grain_apply<2>, grid, dim3(256), 0, s, g);
    return check_launch(who);
}

extern "C" int gsvc_grain_stats(const uint8_t *src, int64_t src_stride, const uint8_t *dec, int64_t dec_stride, int32_t n, int32_t H,
                                int32_t W, int32_t layout, int32_t depth, int32_t flat_threshold, int32_t max_residual, uint64_t *out,
                                void *stream)
{
    const char *who = "grain_stats";
    GSVC_REQUIRE(src && dec && out, "grain_stats: NULL pointer");
    const FrameBufs bufs{"strides", src, src_stride, dec, dec_stride};
    GSVC_FRAMES_TRY(grain_check_frames(who, bufs, n, 65535, H, W, layout, depth));
    GSVC_REQUIRE(flat_threshold >= 0 && flat_threshold <= 65535, "grain_stats: flat_threshold must be 0 .. 65535 (got %d)", (int)flat_threshold);
    GSVC_REQUIRE(max_residual >= 0 && max_residual <= 255, "grain_stats: max_residual must be 0 .. 255 (got %d)", (int)max_residual);
    GSVC_REQUIRE((reinterpret_cast<uintptr_t>(out) & 7) == 0, "grain_stats: out is not 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (gsvc::zero_words_async(out, GS_ROWS * sizeof(uint64_t), s) != hipSuccess) {
        set_error("grain_stats: zeroing failed");
        return GSVC_E_LAUNCH;
    }
    const bool sub = layout == GSVC_FRAMES_YUV420P;
    GrainStatsArgs g = {};
    g.src = src; g.dec = dec;
    g.src_stride = src_stride; g.dec_stride = dec_stride;
    g.H = H; g.W = W;
    g.ch = sub ? H / 2 : H; g.cw = sub ? W / 2 : W;
    g.sub = sub;
    g.shift = depth - 8;
    g.nbx_y = W / 8; g.nbx_c = g.cw / 8;
    g.nb_y = (long long)(W / 8) * (H / 8);
    g.nb_c = (long long)(g.cw / 8) * (g.ch / 8);
    g.flat = (uint32_t)flat_threshold << (depth - 8);
    g.max_res = (uint32_t)max_residual << (depth - 8);
    g.out = reinterpret_cast<unsigned long long *>(out);
    const long long total = g.nb_y + 2 * g.nb_c, per_wg = 4 * GS_BLOCKS_PER_WAVE;
    if (total == 0) return GSVC_OK;                      // no whole block: the sums are zero
    const dim3 grid((unsigned)((total + per_wg - 1) / per_wg), (unsigned)n);
    ProfScope _p("k_grain_stats", s);
    if (depth > 8) hipLaunchKernelGGL(k_grain_stats<2>, grid, dim3(256), 0, s, g);
    else hipLaunchKernelGGL(k_grain_stats<1>, grid, dim3(256), 0, s, g);
    return check_launch(who);
}
