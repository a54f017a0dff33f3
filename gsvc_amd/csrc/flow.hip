// gsvc_amd/csrc/flow.hip — dense optical flow of adjacent frames, gfx950: coarse-to-fine Horn-Schunck with warping (the algorithm and
// the convention of the result: include/gsvc_hip.h, gsvc_flow_estimate).  Stencils only: no atomics, no reduction across workgroups;
// a pair's result depends on neither the batch nor the launch geometry.
//
// k_flow_blur      one pyramid step for a batch of planes: the 5-tap binomial, vertical then horizontal, replicated borders; POOL takes
//                  its samples from the 2x2 means of the source (an odd last row / column is never addressed).
// k_flow_warp      one pass over a level: Ix, Iy, c of a warp from P0, P1 and the current flow.  The central differences of the warped
//                  picture need it at the four neighbours: the pass samples P1 at five positions and stores no warped picture.  UP: the
//                  current flow is the upsampled flow of the coarser level, formed at those five pixels and stored at the centre.
// k_flow_solve     the Jacobi sweeps, blocked: a workgroup stages FL_EXT x FL_EXT cells (a tile of FL_OWN x FL_OWN owned cells and a halo of
//                  FL_K) and runs up to FL_K sweeps on them; after s sweeps the cells s or more away from the staged edge hold what s whole
//                  sweeps give — the same operations on the same values — so the owned cells are exact.  A thread keeps a strip of 4
//                  columns x 4 rows of U, V and their Ix, Iy, c, den in registers for the whole launch.  Left / right neighbours are
//                  the strips of lanes -1 / +1 of a 16-lane row (DPP row shifts, no memory); up / down neighbours are the last / first
//                  row of the strips above / below, passed through LDS: per sweep a thread writes two and reads two 16-byte rows of each
//                  component (ping-pong, one barrier per sweep).  The 16 lanes of a DPP row cover 256 contiguous bytes of an LDS row:
//                  no bank conflict, no padding.  The replicated image border is a select on the cell's own value, not halo.  A level
//                  that fits the staged cells runs its whole solve in one launch (no edge of it is a tile edge).  The last launch of a
//                  warp stores u0 + clamp(U - u0, +-max_step) instead of U.
//
// Contraction of a * b + c into one rounding is switched off in this file: the kernels then do the operations of the float32 NumPy
// restatement (tests/_flow_ref.py) one for one.
#include "common.h"

#pragma clang fp contract(off)

namespace gsvc {

constexpr int FL_EXT = 64;                   // staged cells a side
constexpr int FL_K = 4;                      // halo = sweeps per launch of a tiled level
constexpr int FL_OWN = FL_EXT - 2 * FL_K;    // 56 owned cells a side
constexpr int FL_MAX_LEVELS = 16;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// ============================================================================================================================
// pyramid
// ============================================================================================================================
template <bool POOL>
__device__ __forceinline__ float blur_sample(const float *__restrict__ p, int sw, int y, int x)
{
    if (!POOL) return p[(size_t)y * sw + x];
    const float *q = p + (size_t)(2 * y) * sw + 2 * x;
    return ((q[0] + q[1]) + (q[sw] + q[sw + 1])) * 0.25f;
}

// dst [planes, h, w] <- src (plane k at src + k * src_pitch, rows of sw samples); POOL: (h, w) = (sh / 2, sw / 2)
template <bool POOL>
__global__ void __launch_bounds__(256) k_flow_blur(const float *__restrict__ src, long long src_pitch, int sw, float *__restrict__ dst, int h,
                                                   int w)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const float *p = src + (size_t)blockIdx.z * (size_t)src_pitch;
    int ys[5];
#pragma unroll
    for (int k = 0; k < 5; k++) ys[k] = clampi(y + k - 2, 0, h - 1);
    float v[5];
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const int xc = clampi(x + k - 2, 0, w - 1);
        const float a0 = blur_sample<POOL>(p, sw, ys[0], xc), a1 = blur_sample<POOL>(p, sw, ys[1], xc), a2 = blur_sample<POOL>(p, sw, ys[2], xc);
        const float a3 = blur_sample<POOL>(p, sw, ys[3], xc), a4 = blur_sample<POOL>(p, sw, ys[4], xc);
        v[k] = ((a0 + a4) + 4.f * (a1 + a3) + 6.f * a2) * 0.0625f;
    }
    dst[(size_t)blockIdx.z * ((size_t)h * w) + (size_t)y * w + x] = ((v[0] + v[4]) + 4.f * (v[1] + v[3]) + 6.f * v[2]) * 0.0625f;
}

// ============================================================================================================================
// warp and coefficients
// ============================================================================================================================
__device__ __forceinline__ float bilinear(const float *__restrict__ a, int h, int w, float x, float y)
{
    x = fminf(fmaxf(x, 0.f), (float)(w - 1));
    y = fminf(fmaxf(y, 0.f), (float)(h - 1));
    const float x0 = fminf(floorf(x), (float)(w - 2)), y0 = fminf(floorf(y), (float)(h - 2));
    const float fx = x - x0, fy = y - y0;
    const float *q = a + (size_t)(int)y0 * w + (int)x0;
    const float a00 = q[0], a01 = q[1], a10 = q[w], a11 = q[w + 1];
    const float top = a00 + fx * (a01 - a00), bot = a10 + fx * (a11 - a10);
    return top + fy * (bot - top);
}

struct FlowField {
    float *u, *v;
    long long pitch;                   // floats between the pairs
};

struct WarpArgs {
    const float *P0, *P1;              // [n, h, w]
    FlowField cur;                     // the current flow of this level: read, or written (UP)
    FlowField coarse;                  // UP: the flow of the level below, ch x cw
    int ch, cw;
    float *Ix, *Iy, *c;                // [n, h, w]
    int h, w;
};

template <bool UP>
__device__ __forceinline__ void flow_at(const WarpArgs &g, const float *cu, const float *cv, const float *u0, const float *v0, int x, int y,
                                        float &u, float &v)
{
    if (UP) {
        const float sx = ((float)x + 0.5f) * 0.5f - 0.5f, sy = ((float)y + 0.5f) * 0.5f - 0.5f;
        u = 2.f * bilinear(cu, g.ch, g.cw, sx, sy);
        v = 2.f * bilinear(cv, g.ch, g.cw, sx, sy);
    } else {
        u = u0[(size_t)y * g.w + x];
        v = v0[(size_t)y * g.w + x];
    }
}

template <bool UP>
__global__ void __launch_bounds__(256) k_flow_warp(WarpArgs g)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int h = g.h, w = g.w;
    if (x >= w || y >= h) return;
    const size_t plane = (size_t)blockIdx.z * ((size_t)h * w);
    const float *P0 = g.P0 + plane, *P1 = g.P1 + plane;
    float *u0 = g.cur.u + (size_t)blockIdx.z * (size_t)g.cur.pitch, *v0 = g.cur.v + (size_t)blockIdx.z * (size_t)g.cur.pitch;
    const float *cu = UP ? g.coarse.u + (size_t)blockIdx.z * (size_t)g.coarse.pitch : nullptr;
    const float *cv = UP ? g.coarse.v + (size_t)blockIdx.z * (size_t)g.coarse.pitch : nullptr;
    const int xl = max(x - 1, 0), xr = min(x + 1, w - 1), yu = max(y - 1, 0), yd = min(y + 1, h - 1);
    float u, v, t0, t1;
    flow_at<UP>(g, cu, cv, u0, v0, x, y, u, v);
    const float px = (float)x + u, py = (float)y + v;
    const float Bw = bilinear(P1, h, w, px, py);
    flow_at<UP>(g, cu, cv, u0, v0, xl, y, t0, t1);
    const float Bl = bilinear(P1, h, w, (float)xl + t0, (float)y + t1);
    flow_at<UP>(g, cu, cv, u0, v0, xr, y, t0, t1);
    const float Br = bilinear(P1, h, w, (float)xr + t0, (float)y + t1);
    flow_at<UP>(g, cu, cv, u0, v0, x, yu, t0, t1);
    const float Bu = bilinear(P1, h, w, (float)x + t0, (float)yu + t1);
    flow_at<UP>(g, cu, cv, u0, v0, x, yd, t0, t1);
    const float Bd = bilinear(P1, h, w, (float)x + t0, (float)yd + t1);
    const size_t at = (size_t)y * w + x;
    const float A = P0[at];
    const float Ax = 0.5f * (P0[(size_t)y * w + xr] - P0[(size_t)y * w + xl]), Ay = 0.5f * (P0[(size_t)yd * w + x] - P0[(size_t)yu * w + x]);
    const float Bx = 0.5f * (Br - Bl), By = 0.5f * (Bd - Bu);
    const float ox = fmaxf(fmaxf(-px, px - (float)(w - 1)), 0.f), oy = fmaxf(fmaxf(-py, py - (float)(h - 1)), 0.f);
    const float m = fminf(fmaxf(1.f - fmaxf(ox, oy), 0.f), 1.f);
    const float Ix = m * (0.5f * (Ax + Bx)), Iy = m * (0.5f * (Ay + By)), It = m * (Bw - A);
    g.Ix[plane + at] = Ix;
    g.Iy[plane + at] = Iy;
    g.c[plane + at] = (It - Ix * u) - Iy * v;
    if (UP) {
        u0[at] = u;
        v0[at] = v;
    }
}

// ============================================================================================================================
// solver
// ============================================================================================================================
struct SolveArgs {
    FlowField in;                      // U, V before the first sweep of this launch
    FlowField out;
    FlowField base;                    // u0, v0 of the warp: the launch stores base + clamp(U - base, +-max_step) (u == nullptr: stores U)
    const float *Ix, *Iy, *c;          // [n, h, w]
    int h, w;
    int sweeps, halo;                  // halo = FL_K: tiles of FL_OWN; halo = 0: the level is one tile
    float alpha2, max_step;
    int vec;                           // rows of four cells may be moved as 16 bytes (w % 4 == 0, every base and pitch 16-byte aligned)
};

// the value of lane - 1 / lane + 1 of the 16-lane row; the first / last lane of a row gets its own `self`
__device__ __forceinline__ float from_left_lane(float v, float self)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(self), __float_as_int(v), 0x111, 0xf, 0xf, false));      // row_shr:1
}
__device__ __forceinline__ float from_right_lane(float v, float self)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(self), __float_as_int(v), 0x101, 0xf, 0xf, false));      // row_shl:1
}

// four cells of a row, replicated outside the picture (gy is inside it)
__device__ __forceinline__ float4 load_row4(const float *__restrict__ p, int w, int gy, int gx, bool vec)
{
    const float *row = p + (size_t)gy * w;
    if (vec && gx >= 0 && gx + 3 < w) return *reinterpret_cast<const float4 *>(row + gx);
    float4 r;
    r.x = row[clampi(gx, 0, w - 1)];
    r.y = row[clampi(gx + 1, 0, w - 1)];
    r.z = row[clampi(gx + 2, 0, w - 1)];
    r.w = row[clampi(gx + 3, 0, w - 1)];
    return r;
}

__device__ __forceinline__ void store_row4(float *__restrict__ p, int w, int gy, int gx, bool vec, float4 v)
{
    float *row = p + (size_t)gy * w;
    if (vec && gx + 3 < w) {
        *reinterpret_cast<float4 *>(row + gx) = v;
        return;
    }
    if (gx < w) row[gx] = v.x;
    if (gx + 1 < w) row[gx + 1] = v.y;
    if (gx + 2 < w) row[gx + 2] = v.z;
    if (gx + 3 < w) row[gx + 3] = v.w;
}

__device__ __forceinline__ float step_clamped(float base, float v, float max_step)
{
    return base + fminf(fmaxf(v - base, -max_step), max_step);
}

__global__ void __launch_bounds__(256) k_flow_solve(SolveArgs g)
{
    // [buffer][U / V][strip row ry][its first / last row][64 columns]
    __shared__ __attribute__((aligned(16))) float edge[2][2][FL_EXT / 4][2][FL_EXT];
    const int tid = threadIdx.x, cx = tid & 15, ry = tid >> 4;
    const int h = g.h, w = g.w;
    const int own = FL_EXT - 2 * g.halo;
    const int gx = (int)blockIdx.x * own - g.halo + 4 * cx;          // first column of the strip
    const int gy = (int)blockIdx.y * own - g.halo + 4 * ry;          // first row
    const size_t plane = (size_t)blockIdx.z * ((size_t)h * w);
    const float *Up = g.in.u + (size_t)blockIdx.z * (size_t)g.in.pitch, *Vp = g.in.v + (size_t)blockIdx.z * (size_t)g.in.pitch;
    const bool vec = g.vec != 0;
    float U[4][4], V[4][4], Ix[4][4], Iy[4][4], C[4][4], den[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int y = clampi(gy + i, 0, h - 1);
        const float4 a = load_row4(Up, w, y, gx, vec), b = load_row4(Vp, w, y, gx, vec);
        const float4 p = load_row4(g.Ix + plane, w, y, gx, vec), q = load_row4(g.Iy + plane, w, y, gx, vec), r = load_row4(g.c + plane, w, y, gx, vec);
        U[i][0] = a.x; U[i][1] = a.y; U[i][2] = a.z; U[i][3] = a.w;
        V[i][0] = b.x; V[i][1] = b.y; V[i][2] = b.z; V[i][3] = b.w;
        Ix[i][0] = p.x; Ix[i][1] = p.y; Ix[i][2] = p.z; Ix[i][3] = p.w;
        Iy[i][0] = q.x; Iy[i][1] = q.y; Iy[i][2] = q.z; Iy[i][3] = q.w;
        C[i][0] = r.x; C[i][1] = r.y; C[i][2] = r.z; C[i][3] = r.w;
#pragma unroll
        for (int j = 0; j < 4; j++) den[i][j] = 1.f / ((g.alpha2 + Ix[i][j] * Ix[i][j]) + Iy[i][j] * Iy[i][j]);
    }
    // the picture's border: the neighbour beyond it is the cell itself
    bool first_col[4], last_col[4], first_row[4], last_row[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        first_col[j] = gx + j <= 0;
        last_col[j] = gx + j >= w - 1;
        first_row[j] = gy + j <= 0;
        last_row[j] = gy + j >= h - 1;
    }
    const int ry_up = max(ry - 1, 0), ry_dn = min(ry + 1, FL_EXT / 4 - 1);
    for (int s = 0; s < g.sweeps; s++) {
        const int b = s & 1;
        *reinterpret_cast<float4 *>(&edge[b][0][ry][0][4 * cx]) = make_float4(U[0][0], U[0][1], U[0][2], U[0][3]);
        *reinterpret_cast<float4 *>(&edge[b][0][ry][1][4 * cx]) = make_float4(U[3][0], U[3][1], U[3][2], U[3][3]);
        *reinterpret_cast<float4 *>(&edge[b][1][ry][0][4 * cx]) = make_float4(V[0][0], V[0][1], V[0][2], V[0][3]);
        *reinterpret_cast<float4 *>(&edge[b][1][ry][1][4 * cx]) = make_float4(V[3][0], V[3][1], V[3][2], V[3][3]);
        __syncthreads();
        const float4 uu = *reinterpret_cast<const float4 *>(&edge[b][0][ry_up][1][4 * cx]), ud = *reinterpret_cast<const float4 *>(&edge[b][0][ry_dn][0][4 * cx]);
        const float4 vu = *reinterpret_cast<const float4 *>(&edge[b][1][ry_up][1][4 * cx]), vd = *reinterpret_cast<const float4 *>(&edge[b][1][ry_dn][0][4 * cx]);
        const float Uup[4] = {uu.x, uu.y, uu.z, uu.w}, Udn[4] = {ud.x, ud.y, ud.z, ud.w};
        const float Vup[4] = {vu.x, vu.y, vu.z, vu.w}, Vdn[4] = {vd.x, vd.y, vd.z, vd.w};
        float Un[4][4], Vn[4][4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float ul = from_left_lane(U[i][3], U[i][0]), ur = from_right_lane(U[i][0], U[i][3]);
            const float vl = from_left_lane(V[i][3], V[i][0]), vr = from_right_lane(V[i][0], V[i][3]);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const float su = U[i][j], sv = V[i][j];
                const float lu = first_col[j] ? su : (j == 0 ? ul : U[i][j == 0 ? 0 : j - 1]);
                const float ru = last_col[j] ? su : (j == 3 ? ur : U[i][j == 3 ? 3 : j + 1]);
                const float tu = first_row[i] ? su : (i == 0 ? Uup[j] : U[i == 0 ? 0 : i - 1][j]);
                const float bu = last_row[i] ? su : (i == 3 ? Udn[j] : U[i == 3 ? 3 : i + 1][j]);
                const float lv = first_col[j] ? sv : (j == 0 ? vl : V[i][j == 0 ? 0 : j - 1]);
                const float rv = last_col[j] ? sv : (j == 3 ? vr : V[i][j == 3 ? 3 : j + 1]);
                const float tv = first_row[i] ? sv : (i == 0 ? Vup[j] : V[i == 0 ? 0 : i - 1][j]);
                const float bv = last_row[i] ? sv : (i == 3 ? Vdn[j] : V[i == 3 ? 3 : i + 1][j]);
                const float Ub = 0.25f * ((lu + ru) + (tu + bu)), Vb = 0.25f * ((lv + rv) + (tv + bv));
                const float t = ((Ix[i][j] * Ub + Iy[i][j] * Vb) + C[i][j]) * den[i][j];
                Un[i][j] = Ub - Ix[i][j] * t;
                Vn[i][j] = Vb - Iy[i][j] * t;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                U[i][j] = Un[i][j];
                V[i][j] = Vn[i][j];
            }
    }
    // the owned cells of this strip: whole strips (FL_K is a multiple of 4)
    const int ex = 4 * cx, ey = 4 * ry;
    if (ex < g.halo || ex >= FL_EXT - g.halo || ey < g.halo || ey >= FL_EXT - g.halo || gx >= w) return;
    float *Uo = g.out.u + (size_t)blockIdx.z * (size_t)g.out.pitch, *Vo = g.out.v + (size_t)blockIdx.z * (size_t)g.out.pitch;
    const bool upd = g.base.u != nullptr;
    const float *Bu = upd ? g.base.u + (size_t)blockIdx.z * (size_t)g.base.pitch : nullptr;
    const float *Bv = upd ? g.base.v + (size_t)blockIdx.z * (size_t)g.base.pitch : nullptr;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int y = gy + i;
        if (y >= h) break;
        float4 a = make_float4(U[i][0], U[i][1], U[i][2], U[i][3]), b = make_float4(V[i][0], V[i][1], V[i][2], V[i][3]);
        if (upd) {
            const float4 p = load_row4(Bu, w, y, gx, vec), q = load_row4(Bv, w, y, gx, vec);
            a.x = step_clamped(p.x, a.x, g.max_step); a.y = step_clamped(p.y, a.y, g.max_step);
            a.z = step_clamped(p.z, a.z, g.max_step); a.w = step_clamped(p.w, a.w, g.max_step);
            b.x = step_clamped(q.x, b.x, g.max_step); b.y = step_clamped(q.y, b.y, g.max_step);
            b.z = step_clamped(q.z, b.z, g.max_step); b.w = step_clamped(q.w, b.w, g.max_step);
        }
        store_row4(Uo, w, y, gx, vec, a);
        store_row4(Vo, w, y, gx, vec, b);
    }
}

static_assert(FL_K % 4 == 0 && FL_EXT == 64, "k_flow_solve: a strip is 4 x 4 cells, 16 x 16 strips are staged, the halo is whole strips");

// ============================================================================================================================
// host side
// ============================================================================================================================
static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static bool field_vec_ok(const FlowField &f)
{
    return f.u == nullptr || (aligned16(f.u) && aligned16(f.v) && f.pitch % 4 == 0);
}

static dim3 pixel_grid(int h, int w, int n) { return dim3((w + 63) / 64, (h + 3) / 4, n); }

static void launch_blur(bool pool, const float *src, long long src_pitch, int sw, float *dst, int h, int w, int n, hipStream_t s)
{
    ProfScope _p(pool ? "k_flow_blur_pool" : "k_flow_blur", s);
    if (pool) hipLaunchKernelGGL(k_flow_blur<true>, pixel_grid(h, w, n), dim3(256), 0, s, src, src_pitch, sw, dst, h, w);
    else hipLaunchKernelGGL(k_flow_blur<false>, pixel_grid(h, w, n), dim3(256), 0, s, src, src_pitch, sw, dst, h, w);
}

static void launch_warp(const WarpArgs &g, bool up, int n, hipStream_t s)
{
    ProfScope _p(up ? "k_flow_warp_up" : "k_flow_warp", s);
    if (up) hipLaunchKernelGGL(k_flow_warp<true>, pixel_grid(g.h, g.w, n), dim3(256), 0, s, g);
    else hipLaunchKernelGGL(k_flow_warp<false>, pixel_grid(g.h, g.w, n), dim3(256), 0, s, g);
}

// `iters` sweeps from `start`; the result (the clamped update of `base` where base.u != nullptr) lands in `result`, which is none of
// start, base; tmp[0] and tmp[1] are two more fields (used when the level takes more than one launch)
static void launch_solve(const FlowField &start, const FlowField &base, const FlowField &result, const FlowField tmp[2], const float *Ix,
                         const float *Iy, const float *c, int n, int h, int w, float alpha, int iters, float max_step, hipStream_t s)
{
    SolveArgs g;
    g.Ix = Ix;
    g.Iy = Iy;
    g.c = c;
    g.h = h;
    g.w = w;
    g.alpha2 = alpha * alpha;
    g.max_step = max_step;
    const bool one_tile = h <= FL_EXT && w <= FL_EXT;
    g.halo = one_tile ? 0 : FL_K;
    const int own = FL_EXT - 2 * g.halo;
    const dim3 grid((w + own - 1) / own, (h + own - 1) / own, n);
    const int per = one_tile ? iters : FL_K;
    const int launches = (iters + per - 1) / per;
    FlowField src = start;
    for (int j = 0; j < launches; j++) {
        const bool last = j == launches - 1;
        g.in = src;
        g.out = last ? result : tmp[j & 1];
        g.base = last ? base : FlowField{nullptr, nullptr, 0};
        g.sweeps = min(per, iters - j * per);
        g.vec = w % 4 == 0 && aligned16(Ix) && aligned16(Iy) && aligned16(c) && (h * (long long)w) % 4 == 0 && field_vec_ok(g.in) &&
                field_vec_ok(g.out) && field_vec_ok(g.base);
        ProfScope _p("k_flow_solve", s);
        hipLaunchKernelGGL(k_flow_solve, grid, dim3(256), 0, s, g);
        src = g.out;
    }
}

struct FlowLayout {
    int levels;
    int h[FL_MAX_LEVELS], w[FL_MAX_LEVELS];
    int64_t pyr0[FL_MAX_LEVELS], pyr1[FL_MAX_LEVELS];       // byte offsets
    int64_t field[3], coef[3];
    int64_t bytes;
};

static FlowLayout flow_layout(int32_t n, int32_t H, int32_t W, int32_t max_levels, int32_t min_side)
{
    FlowLayout L;
    int h = H, w = W;
    L.levels = 0;
    int64_t at = 0;
    for (;;) {
        const int l = L.levels++;
        L.h[l] = h;
        L.w[l] = w;
        const int64_t plane = (int64_t)align_up((uint64_t)n * h * w * sizeof(float), 256);
        L.pyr0[l] = at;
        L.pyr1[l] = at + plane;
        at += 2 * plane;
        if (!(min(h, w) / 2 >= min_side && L.levels < max_levels && L.levels < FL_MAX_LEVELS)) break;
        h /= 2;
        w /= 2;
    }
    const int64_t field = (int64_t)align_up((uint64_t)n * 2 * H * W * sizeof(float), 256);
    const int64_t coef = (int64_t)align_up((uint64_t)n * H * W * sizeof(float), 256);
    for (int k = 0; k < 3; k++, at += field) L.field[k] = at;
    for (int k = 0; k < 3; k++, at += coef) L.coef[k] = at;
    L.bytes = at;
    return L;
}

static bool flow_shape_ok(int32_t n, int32_t H, int32_t W, int32_t max_levels, int32_t min_side)
{
    return n >= 1 && n <= 65535 && min_side >= 2 && max_levels >= 1 && H >= 2 && W >= 2 && H <= 32768 && W <= 32768 && min(H, W) >= min_side;
}

}  // namespace gsvc

using namespace gsvc;

extern "C" int64_t gsvc_flow_workspace_bytes(int32_t n, int32_t H, int32_t W, int32_t max_levels, int32_t min_side)
{
    if (!flow_shape_ok(n, H, W, max_levels, min_side)) return -1;
    return flow_layout(n, H, W, max_levels, min_side).bytes;
}

extern "C" int gsvc_flow_estimate(const float *luma0, const float *luma1, int64_t plane_pitch, int32_t n, int32_t H, int32_t W, float alpha,
                                  int32_t warps, int32_t iters, int32_t min_side, int32_t max_levels, float max_step, float *flow_out,
                                  void *workspace, void *stream)
{
    GSVC_REQUIRE(luma0 && luma1 && flow_out && workspace, "flow_estimate: NULL pointer");
    GSVC_REQUIRE(n >= 1 && n <= 65535, "flow_estimate: n must be 1 .. 65535 (got %d)", (int)n);
    GSVC_REQUIRE(H >= 2 && W >= 2 && H <= 32768 && W <= 32768, "flow_estimate: image size must be 2 .. 32768 (got %d x %d)", (int)H, (int)W);
    GSVC_REQUIRE(min_side >= 2, "flow_estimate: min_side must be at least 2 (got %d)", (int)min_side);
    GSVC_REQUIRE(min(H, W) >= min_side, "flow_estimate: the shorter image side (%d x %d) is below min_side %d", (int)H, (int)W, (int)min_side);
    GSVC_REQUIRE(alpha > 0.f, "flow_estimate: alpha must be positive");
    GSVC_REQUIRE(warps >= 1 && iters >= 1 && max_levels >= 1, "flow_estimate: warps, iters and max_levels must be at least 1 (got %d, %d, %d)",
                 (int)warps, (int)iters, (int)max_levels);
    GSVC_REQUIRE(max_step > 0.f, "flow_estimate: max_step must be positive");
    GSVC_REQUIRE(plane_pitch >= (int64_t)H * W, "flow_estimate: plane pitch %lld is shorter than a plane (%lld samples)", (long long)plane_pitch,
                 (long long)H * W);
    GSVC_REQUIRE(((reinterpret_cast<uintptr_t>(luma0) | reinterpret_cast<uintptr_t>(luma1) | reinterpret_cast<uintptr_t>(flow_out)) & 3) == 0,
                 "flow_estimate: a plane base is not 4-byte aligned");
    GSVC_REQUIRE(aligned16(workspace), "flow_estimate: the workspace must be 16-byte aligned");
    const FlowLayout L = flow_layout(n, H, W, max_levels, min_side);
    hipStream_t s = (hipStream_t)stream;
    uint8_t *ws = reinterpret_cast<uint8_t *>(workspace);
    auto P0 = [&](int l) { return reinterpret_cast<float *>(ws + L.pyr0[l]); };
    auto P1 = [&](int l) { return reinterpret_cast<float *>(ws + L.pyr1[l]); };
    launch_blur(false, luma0, plane_pitch, W, P0(0), H, W, n, s);
    launch_blur(false, luma1, plane_pitch, W, P1(0), H, W, n, s);
    for (int l = 1; l < L.levels; l++) {
        const long long below = (long long)L.h[l - 1] * L.w[l - 1];
        launch_blur(true, P0(l - 1), below, L.w[l - 1], P0(l), L.h[l], L.w[l], n, s);
        launch_blur(true, P1(l - 1), below, L.w[l - 1], P1(l), L.h[l], L.w[l], n, s);
    }
    float *Ix = reinterpret_cast<float *>(ws + L.coef[0]), *Iy = reinterpret_cast<float *>(ws + L.coef[1]), *Cc = reinterpret_cast<float *>(ws + L.coef[2]);
    auto field = [&](int k, int h, int w) {          // field k of the workspace laid out for a level: [n][u, v][h w]
        float *p = reinterpret_cast<float *>(ws + L.field[k]);
        return FlowField{p, p + (size_t)h * w, 2ll * h * w};
    };
    int cur = 0;
    {
        const int h = L.h[L.levels - 1], w = L.w[L.levels - 1];
        if (gsvc::zero_words_async(ws + L.field[0], (size_t)n * 2 * h * w * sizeof(float), s) != hipSuccess) {
            set_error("flow_estimate: zeroing failed");
            return GSVC_E_LAUNCH;
        }
    }
    for (int l = L.levels - 1; l >= 0; l--) {
        const int h = L.h[l], w = L.w[l];
        for (int wi = 0; wi < warps; wi++) {
            WarpArgs g;
            g.P0 = P0(l);
            g.P1 = P1(l);
            g.Ix = Ix;
            g.Iy = Iy;
            g.c = Cc;
            g.h = h;
            g.w = w;
            const bool up = wi == 0 && l < L.levels - 1;
            if (up) {
                g.coarse = field(cur, L.h[l + 1], L.w[l + 1]);
                g.ch = L.h[l + 1];
                g.cw = L.w[l + 1];
                cur = (cur + 1) % 3;
            } else {
                g.coarse = FlowField{nullptr, nullptr, 0};
                g.ch = g.cw = 0;
            }
            g.cur = field(cur, h, w);
            launch_warp(g, up, n, s);
            const FlowField tmp[2] = {field((cur + 1) % 3, h, w), field((cur + 2) % 3, h, w)};
            const bool last_warp = l == 0 && wi == warps - 1;
            // the result of a warp goes where its last launch may write: the other of the two fields that launch does not read
            const bool one_tile = h <= FL_EXT && w <= FL_EXT;
            const int launches = one_tile ? 1 : (iters + FL_K - 1) / FL_K;
            const int dst = (cur + 1 + ((launches - 1) & 1)) % 3;
            const FlowField result = last_warp ? FlowField{flow_out, flow_out + (size_t)H * W, 2ll * H * W} : field(dst, h, w);
            launch_solve(g.cur, g.cur, result, tmp, Ix, Iy, Cc, n, h, w, alpha, iters, max_step, s);
            cur = dst;
        }
    }
    return check_launch("flow_estimate");
}

extern "C" int gsvc_flow_pyramid_step(const float *src, int32_t n, int32_t sh, int32_t sw, int32_t pool, float *dst, void *stream)
{
    GSVC_REQUIRE(src && dst, "flow_pyramid_step: NULL pointer");
    GSVC_REQUIRE(n >= 1 && n <= 65535, "flow_pyramid_step: n must be 1 .. 65535 (got %d)", (int)n);
    GSVC_REQUIRE(sh >= 1 && sw >= 1 && sh <= 32768 && sw <= 32768, "flow_pyramid_step: image size must be 1 .. 32768 (got %d x %d)", (int)sh, (int)sw);
    GSVC_REQUIRE(!pool || (sh >= 2 && sw >= 2), "flow_pyramid_step: pooling needs at least 2 x 2 samples (got %d x %d)", (int)sh, (int)sw);
    const int h = pool ? sh / 2 : sh, w = pool ? sw / 2 : sw;
    launch_blur(pool != 0, src, (long long)sh * sw, sw, dst, h, w, n, (hipStream_t)stream);
    return check_launch("flow_pyramid_step");
}

extern "C" int gsvc_flow_warp(const float *P0, const float *P1, float *u0, float *v0, int32_t n, int32_t h, int32_t w, const float *coarse_u,
                              const float *coarse_v, int32_t ch, int32_t cw, float *Ix, float *Iy, float *c, void *stream)
{
    GSVC_REQUIRE(P0 && P1 && u0 && v0 && Ix && Iy && c, "flow_warp: NULL pointer");
    GSVC_REQUIRE((coarse_u == nullptr) == (coarse_v == nullptr), "flow_warp: coarse_u and coarse_v go together");
    GSVC_REQUIRE(n >= 1 && n <= 65535, "flow_warp: n must be 1 .. 65535 (got %d)", (int)n);
    GSVC_REQUIRE(h >= 2 && w >= 2 && h <= 32768 && w <= 32768, "flow_warp: image size must be 2 .. 32768 (got %d x %d)", (int)h, (int)w);
    GSVC_REQUIRE(!coarse_u || (ch >= 2 && cw >= 2 && ch <= h && cw <= w), "flow_warp: the coarse level must be 2 x 2 .. %d x %d (got %d x %d)",
                 (int)h, (int)w, (int)ch, (int)cw);
    WarpArgs g;
    g.P0 = P0;
    g.P1 = P1;
    g.cur = FlowField{u0, v0, (long long)h * w};
    g.coarse = FlowField{const_cast<float *>(coarse_u), const_cast<float *>(coarse_v), (long long)ch * cw};
    g.ch = ch;
    g.cw = cw;
    g.Ix = Ix;
    g.Iy = Iy;
    g.c = c;
    g.h = h;
    g.w = w;
    launch_warp(g, coarse_u != nullptr, n, (hipStream_t)stream);
    return check_launch("flow_warp");
}

extern "C" int gsvc_flow_solve(const float *U, const float *V, const float *Ix, const float *Iy, const float *c, const float *u0, const float *v0,
                               int32_t n, int32_t h, int32_t w, float alpha, int32_t iters, float max_step, float *out_u, float *out_v,
                               void *workspace, void *stream)
{
    GSVC_REQUIRE(U && V && Ix && Iy && c && out_u && out_v && workspace, "flow_solve: NULL pointer");
    GSVC_REQUIRE((u0 == nullptr) == (v0 == nullptr), "flow_solve: u0 and v0 go together");
    GSVC_REQUIRE(n >= 1 && n <= 65535, "flow_solve: n must be 1 .. 65535 (got %d)", (int)n);
    GSVC_REQUIRE(h >= 1 && w >= 1 && h <= 32768 && w <= 32768, "flow_solve: image size must be 1 .. 32768 (got %d x %d)", (int)h, (int)w);
    GSVC_REQUIRE(alpha > 0.f && iters >= 1, "flow_solve: alpha must be positive and iters at least 1");
    GSVC_REQUIRE(!u0 || max_step > 0.f, "flow_solve: max_step must be positive");
    GSVC_REQUIRE(aligned16(workspace), "flow_solve: the workspace must be 16-byte aligned");
    GSVC_REQUIRE(out_u != U && out_u != V && out_v != U && out_v != V && out_u != u0 && out_v != v0, "flow_solve: the result may not alias an input");
    const long long hw = (long long)h * w;
    float *t = reinterpret_cast<float *>(workspace);
    const size_t field = (size_t)align_up((uint64_t)n * 2 * hw * sizeof(float), 256) / sizeof(float);
    const FlowField tmp[2] = {FlowField{t, t + hw, 2 * hw}, FlowField{t + field, t + field + hw, 2 * hw}};
    const FlowField start{const_cast<float *>(U), const_cast<float *>(V), hw}, base{const_cast<float *>(u0), const_cast<float *>(v0), hw};
    launch_solve(start, base, FlowField{out_u, out_v, hw}, tmp, Ix, Iy, c, n, h, w, alpha, iters, max_step, (hipStream_t)stream);
    return check_launch("flow_solve");
}

extern "C" int64_t gsvc_flow_solve_workspace_bytes(int32_t n, int32_t h, int32_t w)
{
    if (n < 1 || n > 65535 || h < 1 || w < 1 || h > 32768 || w > 32768) return -1;
    return 2 * (int64_t)align_up((uint64_t)n * 2 * h * w * sizeof(float), 256);
}
