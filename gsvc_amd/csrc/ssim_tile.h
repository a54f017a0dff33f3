// gsvc_amd/csrc/ssim_tile.h — the 32x32-tile, 11-tap separable Gaussian blur that k_ssim_fwd / k_ssim_bwd (ssim.hip) and
// k_msssim_scale (metrics.hip) are written in: 256 threads, the 42x42 inputs of a tile staged in LDS, a horizontal pass into LDS
// and a vertical pass into registers.  Both passes are REGISTER-BLOCKED: a thread produces 4 adjacent outputs of a row (horizontal:
// 14 + 2 staged values per plane through four 16-byte LDS reads) or of a column (vertical: 14 LDS reads per plane), so an output
// costs 7 + 17.5 LDS reads instead of 22 + 55, and the 32x32 tile reads 1.7x its pixels from HBM instead of 2.6x (16x16).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace gsvc {

constexpr int ST_TILE = 32;
constexpr int ST_TAPS = 11;
constexpr int ST_R = ST_TAPS / 2;                // window radius
constexpr int ST_HALO = ST_TILE + ST_TAPS - 1;   // 42 staged rows / columns for 32 outputs
constexpr int ST_LD = 44;                        // row stride of the staged planes: 16-byte aligned groups of 4 columns
constexpr int ST_HLD = ST_TILE + 1;              // row stride of the horizontally blurred planes
constexpr int ST_GROUPS = ST_HALO * (ST_TILE / 4);   // groups of 4 outputs of the horizontal pass: group g = row g >> 3, columns 4 (g & 7) ..
constexpr float SSIM_C1 = 0.01f * 0.01f;
constexpr float SSIM_C2 = 0.03f * 0.03f;

struct SsimWindow {
    float w[ST_TAPS];
};

// The eleven window taps as VECTOR registers.  Passed by value they live in SGPRs, and a multiply-add that reads an SGPR issues at
// 4.5 cycles per wave where the register-only form issues at 2.7 (four waves per SIMD; DESIGN section 4b, tools/micro/valu_issue.hip)
// — and these kernels are nothing but such multiply-adds (434 of the SSIM forward's 717 vector arithmetic instructions).  The
// compiler keeps a uniform value in an SGPR whenever it can see that it is uniform: the move is hidden from it.
__device__ __forceinline__ SsimWindow window_in_vgprs(const SsimWindow &win)
{
    SsimWindow r;
#pragma unroll
    for (int k = 0; k < ST_TAPS; k++) asm volatile("v_mov_b32 %0, %1" : "=v"(r.w[k]) : "s"(win.w[k]));
    return r;
}

// The two windows: exp(-(i - 5)^2 / (2 * 1.5^2)) normalised.  They differ in where the rounding to float happens, and so in the
// last bit of some taps.
// The loss window, as the reference's torch.Tensor([...]) builds it: each tap rounded to float first, then divided by the float sum.
static SsimWindow make_loss_window()
{
    SsimWindow w;
    float g[ST_TAPS], s = 0.f;
    for (int i = 0; i < ST_TAPS; i++) g[i] = (float)std::exp(-(double)((i - ST_R) * (i - ST_R)) / (2.0 * 1.5 * 1.5));
    for (int i = 0; i < ST_TAPS; i++) s += g[i];
    for (int i = 0; i < ST_TAPS; i++) w.w[i] = g[i] / s;
    return w;
}
// The MS-SSIM window: divided in double, each tap rounded once.
static SsimWindow make_msssim_window()
{
    SsimWindow w;
    double g[ST_TAPS], s = 0.0;
    for (int i = 0; i < ST_TAPS; i++) {
        g[i] = std::exp(-(double)((i - ST_R) * (i - ST_R)) / (2.0 * 1.5 * 1.5));
        s += g[i];
    }
    for (int i = 0; i < ST_TAPS; i++) w.w[i] = (float)(g[i] / s);
    return w;
}

// Staging N planes of the tile's 42x42 inputs is two steps, so that every load of the tile is issued before the first is waited
// for (7 per thread and plane: with one load per loop iteration the block spent its time in 7 dependent memory round trips):
//     float v[ST_LOADS][N];
//     for it < ST_LOADS (unrolled): tile_slot(it, r, c), then the kernel's own loads of element (r, c) into v[it]
//     store_tile(s, v);  __syncthreads();
// The loads are the kernel's own loop, not a callable handed to one staging function: in every shape tried, a closure over the
// kernel's arguments moved the SGPR counts of k_ssim_fwd (42 -> 44) and k_ssim_bwd (38 -> 42).  k_ssim_fwd and k_msssim_scale stage
// this way; k_ssim_bwd keeps the same two steps written out (the reason stands there).
constexpr int ST_LOADS = (ST_HALO * ST_HALO + 255) / 256;   // staged elements per thread

// the it-th element a thread stages: row r, column c of the 42x42; false: past its end (it is not stored: load nothing for it)
__device__ __forceinline__ bool tile_slot(int it, int &r, int &c)
{
    const int i = threadIdx.x + 256 * it;
    r = i / ST_HALO;
    c = i - r * ST_HALO;
    return i < ST_HALO * ST_HALO;
}

// the loaded values into LDS, and zeros into the two pad columns that the 16-byte reads of the horizontal pass touch (never used in
// arithmetic: kept finite)
template <int N>
__device__ __forceinline__ void store_tile(float (&s)[N][ST_HALO][ST_LD], const float (&v)[ST_LOADS][N])
{
#pragma unroll
    for (int it = 0; it < ST_LOADS; it++) {
        int r, c;
        if (tile_slot(it, r, c)) {
#pragma unroll
            for (int n = 0; n < N; n++) s[n][r][c] = v[it][n];
        }
    }
    const int tid = threadIdx.x;
    if (tid < 2 * ST_HALO) {
#pragma unroll
        for (int n = 0; n < N; n++) s[n][tid >> 1][ST_HALO + (tid & 1)] = 0.f;
    }
}

// 16 adjacent values of a staged row (c0 a multiple of 4): four 16-byte LDS reads
__device__ __forceinline__ void staged_row16(const float (&s)[ST_HALO][ST_LD], int r, int c0, float (&v)[16])
{
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const float4 a = *reinterpret_cast<const float4 *>(&s[r][c0 + 4 * q]);
        v[4 * q] = a.x; v[4 * q + 1] = a.y; v[4 * q + 2] = a.z; v[4 * q + 3] = a.w;
    }
}

// the 11 taps onto 4 adjacent outputs from 14 adjacent inputs: out[j] = sum_k w[k] v[j + k], added in rising k
__device__ __forceinline__ void blur4(const SsimWindow &win, const float *v, float (&out)[4])
{
#pragma unroll
    for (int j = 0; j < 4; j++) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < ST_TAPS; k++) a = fmaf(win.w[k], v[j + k], a);
        out[j] = a;
    }
}

// vertical pass of one plane: outputs (rows row0 .. row0 + 3, column col) from 14 LDS reads
__device__ __forceinline__ void blur4_column(const SsimWindow &win, const float (&hb)[ST_HALO][ST_HLD], int row0, int col, float (&out)[4])
{
    float v[14];
#pragma unroll
    for (int k = 0; k < 14; k++) v[k] = hb[row0 + k][col];
    blur4(win, v, out);
}

// horizontal pass of the five moments (x, y, x^2, y^2, xy) of one group: hb[m][r][c0 .. c0 + 3] from 14 values of each picture.
// The products once per staged element (the reference blurs img1 * img1 etc.: products first), then 5 FMAs per tap.
__device__ __forceinline__ void blur4_moments(const SsimWindow &win, const float (&xv)[16], const float (&yv)[16],
                                              float (&hb)[5][ST_HALO][ST_HLD], int r, int c0)
{
    float xx[14], yy[14], xy[14];
#pragma unroll
    for (int k = 0; k < 14; k++) { xx[k] = xv[k] * xv[k]; yy[k] = yv[k] * yv[k]; xy[k] = xv[k] * yv[k]; }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
#pragma unroll
        for (int k = 0; k < ST_TAPS; k++) {
            const float w = win.w[k];
            a0 = fmaf(w, xv[j + k], a0); a1 = fmaf(w, yv[j + k], a1); a2 = fmaf(w, xx[j + k], a2);
            a3 = fmaf(w, yy[j + k], a3); a4 = fmaf(w, xy[j + k], a4);
        }
        hb[0][r][c0 + j] = a0; hb[1][r][c0 + j] = a1; hb[2][r][c0 + j] = a2; hb[3][r][c0 + j] = a3; hb[4][r][c0 + j] = a4;
    }
}

}  // namespace gsvc
