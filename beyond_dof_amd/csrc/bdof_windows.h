// Ptychography windows at fractional origins: the window stack, its exact adjoint and the derivative of a loss with respect to
// the origins — the fractional counterpart of the integer window cut that the sweeps do by index math (obj_src_row with xoff / yoff)
// and of k_window_overlap_add.
//
// Rotated frame R[z][xg][y] = row tab[z][xg] of the bound volume (rows of volNY pairs), zero outside.  Window b has the continuous
// origin (u_b, v_b) = origin[b], the pixel coordinate of its first voxel along x and along y:
//     i0 = floor(u), fx = u - i0;  j0 = floor(v), fy = v - j0;  wx = (1 - fx, fx), wy = (1 - fy, fy)
//     W_b[z][i][j] = sum_{a,c in {0,1}} wx_a wy_c R[z][i0 + i + a][j0 + j + c]
// z is untouched.  The window rows are [B][S][NX][NY] pairs: a batch of already rotated objects (obj_src_row without a table).
//
// The first part of this file is free of device code, so that a stand-alone host program can walk the origin, floor and list
// arithmetic under a sanitizer (tools/check_window_index.cpp).
#pragma once
#include <cmath>
#include <vector>

#ifdef __HIPCC__
#define BDOF_WIN_HD __host__ __device__ __forceinline__
#else
#define BDOF_WIN_HD inline
#endif

// Lower corner and the two factors (one minus the fraction, the fraction) rounded to float32 of one axis of an origin.  The
// origin is clamped first to [-(n_win + 2), n_vol + 1]: a window that far out has every tap outside either way, and the
// conversion to int stays defined (a NaN origin takes the lower clamp).
BDOF_WIN_HD void win_axis(double u, int n_vol, int n_win, int& i0, float (&w)[2]) {
    const double c = fmin(fmax(u, -(double)n_win - 2.0), (double)n_vol + 1.0);
    const double fl = floor(c);
    const double fr = fmin(fmax(c - fl, 0.0), 1.0);
    i0 = (int)fl;
    w[0] = (float)(1.0 - fr);
    w[1] = (float)fr;
}
// win_cell is the only place where an origin becomes indices and weights: the forward kernel, the adjoint and the derivative all
// call it, so their weights are the same bits.
struct WinCell {
    int i0, j0;
    float wx[2], wy[2];
};
BDOF_WIN_HD WinCell win_cell(const double* origin, int b, int NX, int NY, int volNX, int volNY) {
    WinCell c;
    win_axis(origin[2 * (size_t)b], volNX, NX, c.i0, c.wx);
    win_axis(origin[2 * (size_t)b + 1], volNY, NY, c.j0, c.wy);
    return c;
}
// the weight of tap (a, c): the float32 product of the two factors, in this order
BDOF_WIN_HD float win_weight(const WinCell& c, int a, int cc) { return c.wx[a] * c.wy[cc]; }
// Window b touches rotated-frame column xg through its rows i = xg - i0 (tap a = 0) and i - 1 (tap a = 1): NX + 1 columns
BDOF_WIN_HD bool win_touches(const WinCell& c, int xg, int NX) { return xg >= c.i0 && xg - c.i0 <= NX; }

#define BDOF_WIN_MAXLIST_SHIFTED 1024        // == BDOF_WIN_MAXLIST (bdof_kernels.h): the list of one column in LDS

// The largest number of windows that touch one column of the rotated frame (host: the entry point's check before the launch)
inline int win_max_per_column(const double* origin, int B, int NX, int NY, int volNX, int volNY) {
    if (volNX < 1 || B < 1) return 0;
    std::vector<int> step((size_t)volNX + 1, 0);
    for (int b = 0; b < B; ++b) {
        const WinCell c = win_cell(origin, b, NX, NY, volNX, volNY);
        const long long lo = c.i0 < 0 ? 0 : c.i0, hi = (long long)c.i0 + NX;          // columns lo .. hi inclusive
        if (hi < 0 || lo >= volNX) continue;
        step[(size_t)lo] += 1;
        step[(size_t)(hi + 1 < volNX ? hi + 1 : volNX)] -= 1;
    }
    int most = 0, run = 0;
    for (int x = 0; x < volNX; ++x) {
        run += step[(size_t)x];
        most = run > most ? run : most;
    }
    return most;
}

// per-workgroup records of the position derivative: their number and their share of the rows (z, i) depend on (S, NX) only
#define WIN_PG_MAX_PARTIALS 512
BDOF_WIN_HD int win_position_partials(int S, int NX) {
    const long long groups = ((long long)S * NX + 3) / 4;                  // 4 rows (waves) per workgroup pass
    return (int)(groups < WIN_PG_MAX_PARTIALS ? groups : WIN_PG_MAX_PARTIALS);
}

#ifdef __HIPCC__
#include "bdof_kernels.h"
static_assert(BDOF_WIN_MAXLIST_SHIFTED == BDOF_WIN_MAXLIST, "one list length for both overlap-add kernels");

struct WinStackArgs {
    const float2* vol;        // rows of volNY pairs: the bound volume (or its rotated copy)
    const int* tab;           // [S][volNX] of the step's angle -> source row
    const double* origin;     // [B][2] = (u, v)
    float2* rows;             // forward: out [B][S][NX][NY]; derivative: in, the window-frame gradient
    int B, S, NX, NY, volNX, volNY;
};

// the volume row behind rotated-frame row (z, xg), -1 outside the frame
__device__ __forceinline__ long long win_src_row(const WinStackArgs& a, int z, int xg) {
    return xg >= 0 && xg < a.volNX ? (long long)a.tab[(size_t)z * a.volNX + xg] : -1;
}

// Forward gather: one wave per output row (b, z, i) (4 rows per workgroup), lanes along j.  Two source rows, two columns each;
// a tap of weight 0 or outside the volume is skipped.  At fx = fy = 0 the one live tap has weight 1: the integer cut, value for value.
__global__ __launch_bounds__(256) void k_window_stack(WinStackArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t nrows = (size_t)a.B * a.S * a.NX;
    for (size_t o = (size_t)blockIdx.x * 4 + wave; o < nrows; o += (size_t)gridDim.x * 4) {
        const int i = o % a.NX;
        const size_t r = o / a.NX;
        const int z = r % a.S, b = r / a.S;
        const WinCell c = win_cell(a.origin, b, a.NX, a.NY, a.volNX, a.volNY);
        const long long r0 = win_src_row(a, z, c.i0 + i), r1 = win_src_row(a, z, c.i0 + i + 1);
        const float2* src[2] = {r0 >= 0 ? a.vol + (size_t)r0 * a.volNY : nullptr, r1 >= 0 ? a.vol + (size_t)r1 * a.volNY : nullptr};
        float2* dst = a.rows + o * a.NY;
        for (int j = lane; j < a.NY; j += 64) {
            float2 acc = make_float2(0.f, 0.f);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int ta = t >> 1, tc = t & 1;
                const int y = c.j0 + j + tc;
                const float w = win_weight(c, ta, tc);
                if (w != 0.f && src[ta] && y >= 0 && y < a.volNY) {
                    const float2 s = src[ta][y];
                    acc.x = fmaf(w, s.x, acc.x);
                    acc.y = fmaf(w, s.y, acc.y);
                }
            }
            dst[j] = acc;
        }
    }
}

// Stage 1 of the adjoint, the fractional twin of k_window_overlap_add:
//     pad[z][xg][y] = sum_b sum_{a,c} wx_a wy_c g_b[z][xg - i0_b - a][y - j0_b - c]
// One workgroup per (xg, chunk of z).  It lists the windows that touch its column (win_touches: NX + 1 columns per window) in
// LDS in ascending b — a ballot and a prefix count per 256 windows, no atomics —, sorts them by (j0, b) and streams their rows
// with the forward's weights: fixed order (j0, then b, then a, then c), so repeated calls give the same bits.  The caller has
// checked that no column holds more than BDOF_WIN_MAXLIST_SHIFTED windows (the clamp below only keeps the LDS arrays safe).
// Stage 2 is k_rot_adjoint on `pad` as a one-element batch.
struct WinShiftAdjArgs {
    const float2* grot;       // [B][S][NX][NY] window-frame gradient
    const double* origin;     // [B][2]
    int B, S, NX, NY, volNX, volNY;
};
__global__ __launch_bounds__(256) void k_window_overlap_add_shifted(WinShiftAdjArgs a, float2* pad, int z_per_wg) {
    constexpr int M = BDOF_WIN_MAXLIST_SHIFTED;
    __shared__ int ub[M], uy[M];                       // unsorted: window, j0
    __shared__ int lb[M], ly[M], lx[M];                // sorted by (j0, window): window, j0, row i = xg - i0 of tap a = 0
    __shared__ float lwx[M][2], lwy[M][2];
    __shared__ int wcount[4];
    const int xg = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int n = 0;
    for (int base = 0; base < a.B; base += 256) {
        const int b = base + (int)threadIdx.x;
        bool hit = false;
        int j0 = 0;
        if (b < a.B) {
            const WinCell c = win_cell(a.origin, b, a.NX, a.NY, a.volNX, a.volNY);
            hit = win_touches(c, xg, a.NX);
            j0 = c.j0;
        }
        const unsigned long long m = __ballot(hit);
        if (lane == 0) wcount[wave] = __popcll(m);
        __syncthreads();
        int slot = n + __popcll(m & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) slot += wcount[w];
        if (hit && slot < M) { ub[slot] = b; uy[slot] = j0; }
        n += wcount[0] + wcount[1] + wcount[2] + wcount[3];
        __syncthreads();
    }
    n = min(n, M);
    // rank sort by (j0, window index): the windows that reach a given y are one contiguous run of the list
    for (int e = threadIdx.x; e < n; e += blockDim.x) {
        const int ye = uy[e], be = ub[e];
        int rank = 0;
        for (int o = 0; o < n; ++o) rank += (uy[o] < ye) || (uy[o] == ye && ub[o] < be);
        const WinCell c = win_cell(a.origin, be, a.NX, a.NY, a.volNX, a.volNY);
        lb[rank] = be;
        ly[rank] = ye;
        lx[rank] = xg - c.i0;
        lwx[rank][0] = c.wx[0]; lwx[rank][1] = c.wx[1];
        lwy[rank][0] = c.wy[0]; lwy[rank][1] = c.wy[1];
    }
    __syncthreads();
    const int z0 = blockIdx.y * z_per_wg, z1 = min(a.S, z0 + z_per_wg);
    for (int y = threadIdx.x; y < a.volNY; y += blockDim.x) {
        // windows with j0 in [y - NY, y]: first index with j0 >= y - NY, first index with j0 > y
        int lo, hi;
        {
            int l = 0, h = n;
            while (l < h) { const int mid = (l + h) >> 1; if (ly[mid] >= y - a.NY) h = mid; else l = mid + 1; }
            lo = l;
            l = 0; h = n;
            while (l < h) { const int mid = (l + h) >> 1; if (ly[mid] > y) h = mid; else l = mid + 1; }
            hi = l;
        }
        for (int z = z0; z < z1; ++z) {
            float2 acc = make_float2(0.f, 0.f);
            for (int e = lo; e < hi; ++e) {
                const float2* g = a.grot + ((size_t)lb[e] * a.S + z) * a.NX * a.NY;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int ta = t >> 1, tc = t & 1;
                    const int i = lx[e] - ta, j = y - ly[e] - tc;
                    const float w = lwx[e][ta] * lwy[e][tc];
                    if (w != 0.f && i >= 0 && i < a.NX && j >= 0 && j < a.NY) {
                        const float2 v = g[(size_t)i * a.NY + j];
                        acc.x = fmaf(w, v.x, acc.x);
                        acc.y = fmaf(w, v.y, acc.y);
                    }
                }
            }
            pad[((size_t)z * a.volNX + xg) * a.volNY + y] = acc;
        }
    }
}

// ---- the derivative of a loss with respect to the origins --------------------------------------------------------------------------------
//     dL/du_b = sum_{z,i,j} sum_ch g_b[z][i][j] sum_c wy_c (R[z][i0+i+1][j0+j+c] - R[z][i0+i][j0+j+c])
//     dL/dv_b = sum_{z,i,j} sum_ch g_b[z][i][j] sum_a wx_a (R[z][i0+i+a][j0+j+1] - R[z][i0+i+a][j0+j])
// taken INSIDE the cell floor gives: an origin on a lattice line takes the right-hand derivative (the convention of
// k_rot_rigid_param_grad).  A corner outside the volume counts 0, a coefficient of 0 is skipped.
//
// One wave per row (b, z, i), lanes along j; grid B P, workgroup p of element b takes the rows 4 (p + k P) + wave.  Taps, tap sums
// and the product with g in float32, the sums over voxels in float64: lanes, then the wave (shuffles), then the workgroup's waves
// in wave order (LDS), one record of 2 per workgroup: partial [B][P][2].  P and a workgroup's rows depend on (S, NX) only and
// nothing is added atomically: element b has the same bits alone, in a batch and twice.
__global__ __launch_bounds__(256) void k_window_position_grad(WinStackArgs a, int P, double* __restrict__ partial) {
    __shared__ double w[4][2];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.x / P, p = blockIdx.x - b * P, nrows = a.S * a.NX;
    const WinCell c = win_cell(a.origin, b, a.NX, a.NY, a.volNX, a.volNY);
    double acc[2] = {0.0, 0.0};
    for (int r = p * 4 + wave; r < nrows; r += P * 4) {
        const int i = r % a.NX, z = r / a.NX;
        const long long r0 = win_src_row(a, z, c.i0 + i), r1 = win_src_row(a, z, c.i0 + i + 1);
        const float2* src[2] = {r0 >= 0 ? a.vol + (size_t)r0 * a.volNY : nullptr, r1 >= 0 ? a.vol + (size_t)r1 * a.volNY : nullptr};
        const float2* grow = a.rows + ((size_t)b * nrows + r) * a.NY;
        for (int j = lane; j < a.NY; j += 64) {
            float2 d[2] = {make_float2(0.f, 0.f), make_float2(0.f, 0.f)};          // dW/du, dW/dv, both channels
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int ta = t >> 1, tc = t & 1;
                const int y = c.j0 + j + tc;
                if (src[ta] && y >= 0 && y < a.volNY) {
                    const float cu = ta ? c.wy[tc] : -c.wy[tc], cv = tc ? c.wx[ta] : -c.wx[ta];
                    if (cu != 0.f || cv != 0.f) {
                        const float2 v = src[ta][y];
                        if (cu != 0.f) { d[0].x = fmaf(cu, v.x, d[0].x); d[0].y = fmaf(cu, v.y, d[0].y); }
                        if (cv != 0.f) { d[1].x = fmaf(cv, v.x, d[1].x); d[1].y = fmaf(cv, v.y, d[1].y); }
                    }
                }
            }
            const float2 g = grow[j];
            acc[0] += (double)fmaf(g.y, d[0].y, g.x * d[0].x);
            acc[1] += (double)fmaf(g.y, d[1].y, g.x * d[1].x);
        }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        double v = acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) w[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int k = threadIdx.x;
        partial[(size_t)blockIdx.x * 2 + k] = ((w[0][k] + w[1][k]) + w[2][k]) + w[3][k];
    }
}

// the P records of element b added in ascending order: out [B][2] (+= with accumulate); grid B, one wave
__global__ __launch_bounds__(64) void k_window_position_sum(const double* __restrict__ partial, int P, double* __restrict__ out, int accumulate) {
    const int b = blockIdx.x, k = threadIdx.x;
    if (k >= 2) return;
    double s = 0.0;
    for (int p = 0; p < P; ++p) s += partial[((size_t)b * P + p) * 2 + k];
    out[2 * (size_t)b + k] = accumulate ? out[2 * (size_t)b + k] + s : s;
}
#endif      // __HIPCC__
