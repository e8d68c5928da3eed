// Whole-field / tile-batch operations of the tiled ("pfft") propagator in either precision (DESIGN: cfg4).
//
//  * free-space steps of a batch of fields in ONE transform pair (rocFFT, batched 2-D, in place): field <- F^-1 ( h * F field )
//    with a caller-supplied table h[kx][ky] (the n-th power of the transfer function, 1 / (NX NY) folded in) — the long-range
//    correction of the tiled propagator applies it once per stitch range to the whole field and to the tile batch;
//  * the float64 tile path (TiledPropagator(precision='float64')): the reference's arithmetic is float64
//    (cnn_propagator/np_funcs.py:20-42, quirk Q2) and a 1024-slice stack run through float32 transforms carries 1.5e-5 of
//    rounding; here modulation, transforms (rocFFT double) and the transfer-function product are float64, unfused;
//  * the tile family: tiles cut out of a field / written back into it, and the adjoints, for every pairing of field and tile
//    precision; axpy and conversions in float64.
#pragma once
#include "bdof_generic.h"

// y += alpha x on n real numbers
template <class R>
__global__ __launch_bounds__(256) void k_f_axpy(R* __restrict__ y, const R* __restrict__ x, R alpha, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) y[i] += alpha * x[i];
}

__global__ __launch_bounds__(256) void k_f_to_double(const cf* __restrict__ src, double2* __restrict__ dst, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        dst[i] = make_double2((double)src[i].x, (double)src[i].y);
}
__global__ __launch_bounds__(256) void k_f_to_float(const double2* __restrict__ src, cf* __restrict__ dst, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        dst[i] = make_float2((float)src[i].x, (float)src[i].y);
}

// ---------------------------------------------------------------------------------------------
// The tile family.  Tiled ("pfft") propagation: a field too large for one fused plan is cut into overlapping tiles that run
// through the per-slice kernels as a batch; every few slices the tiles' cores are stitched back and the halos refilled
// (README.md:1-11 of the reference: "tiling-based Fresnel multislice propagation"; its source is on a branch that is not in the
// checkout).  Field [FX][FY] complex; tile b covers field rows x0[b] .. x0[b] + TX - 1 and columns y0[b] .. + TY - 1,
// PERIODICALLY (the whole-field FFT propagator it stands in for is periodic).  Four linear operators, each written once for a
// field of complex type F and tiles of complex type T (cf / cf, double2 / double2, and float32 tiles of a float64 field: the
// field of the float32 tiled path with the long-range correction stays in float64 — its bulk is carried by the whole-field
// free-space step in double, the tiles add the object's part); the arithmetic is done in the FIELD's real type:
//   cut    tiles_a = periodic window of the field x taper                                          k_tiles_cut
//   cut^H  field (+)= sum of the tapered (tiles_a - tiles_b) pixels at the places they were cut from  k_tiles_cut_adjoint
//   put    field[core] = (field[core] +) tiles_a (- tiles_b); pixels beyond the field's edge are dropped  k_tiles_put
//   put^H  tiles_a = the field on the tile's core, zero on the halo and beyond the field's edge    k_tiles_put_adjoint
// ---------------------------------------------------------------------------------------------
template <class F, class T>
struct TileArgs {
    F* field;           // [FX][FY]
    T* tiles_a;         // [B][TX][TY]: written by cut / put^H, read by cut^H / put
    const T* tiles_b;   // nullable: cut^H / put take tiles_a - tiles_b
    const int* x0;
    const int* y0;
    int B, FX, FY, TX, TY, hx, hy;      // put, put^H: only the core [hx, TX - hx) x [hy, TY - hy) of a tile is written back
    int taper;                          // cut, cut^H: the outermost `taper` pixels of a tile are ramped to zero (raised cosine)
    int accumulate;                     // cut^H / put: add to the field instead of overwriting it
};
template <class C> using real_of = decltype(C::x);
template <class C, class R>
__device__ __forceinline__ C make_c(R x, R y) { C c; c.x = (real_of<C>)x; c.y = (real_of<C>)y; return c; }

// A tile is propagated with its own periodic FFT: left and right edge meet, and a jump there diffracts into the tile with a
// 1/distance tail (Fresnel edge fringes) — 7e-4 of error at a 16-pixel halo.  Ramping the outer part of the halo to zero
// removes the jump; what is left travels inwards at the geometric rate only (3e-5 at the same halo, 3e-6 at 32 pixels).
template <class R> __device__ __forceinline__ R taper_weight(int i, int n, int taper);
template <> __device__ __forceinline__ float taper_weight<float>(int i, int n, int taper) {
    const int e = min(i, n - 1 - i);
    return e < taper ? 0.5f - 0.5f * __cosf(3.14159265358979f * ((float)e + 0.5f) / (float)taper) : 1.f;
}
template <> __device__ __forceinline__ double taper_weight<double>(int i, int n, int taper) {
    const int e = min(i, n - 1 - i);
    return e < taper ? 0.5 - 0.5 * cos(3.14159265358979323846 * ((double)e + 0.5) / (double)taper) : 1.0;
}
__device__ __forceinline__ int wrap_idx(int i, int n) { i %= n; return i < 0 ? i + n : i; }

template <class F, class T>
__global__ __launch_bounds__(256) void k_tiles_cut(TileArgs<F, T> a) {
    using R = real_of<F>;
    const int b = blockIdx.z;
    const int ox = a.x0[b], oy = a.y0[b];
    for (int x = blockIdx.y; x < a.TX; x += gridDim.y) {
        T* dst = a.tiles_a + ((size_t)b * a.TX + x) * a.TY;
        const F* src = a.field + (size_t)wrap_idx(ox + x, a.FX) * a.FY;
        const R wx = taper_weight<R>(x, a.TX, a.taper);
        for (int y = blockIdx.x * blockDim.x + threadIdx.x; y < a.TY; y += gridDim.x * blockDim.x) {
            const R w = wx * taper_weight<R>(y, a.TY, a.taper);
            const F v = src[wrap_idx(oy + y, a.FY)];
            dst[y] = make_c<T>(v.x * w, v.y * w);
        }
    }
}
// the adjoint of k_tiles_put (which writes cores, without wrapping)
template <class F, class T>
__global__ __launch_bounds__(256) void k_tiles_put_adjoint(TileArgs<F, T> a) {
    const int b = blockIdx.z;
    const int ox = a.x0[b], oy = a.y0[b];
    for (int x = blockIdx.y; x < a.TX; x += gridDim.y) {
        T* dst = a.tiles_a + ((size_t)b * a.TX + x) * a.TY;
        const int xg = ox + x;
        const bool xin = x >= a.hx && x < a.TX - a.hx && xg >= 0 && xg < a.FX;
        const F* src = a.field + (size_t)(xin ? xg : 0) * a.FY;
        for (int y = blockIdx.x * blockDim.x + threadIdx.x; y < a.TY; y += gridDim.x * blockDim.x) {
            const int yg = oy + y;
            const bool in = xin && y >= a.hy && y < a.TY - a.hy && yg >= 0 && yg < a.FY;
            const F v = src[in ? yg : 0];
            dst[y] = in ? make_c<T>(v.x, v.y) : make_c<T>(0.f, 0.f);
        }
    }
}
// cores back into the field; a core pixel beyond the field's edge is dropped (cores tile the field from 0, the last ones
// overhang), so every field pixel has exactly one writer
template <class F, class T>
__global__ __launch_bounds__(256) void k_tiles_put(TileArgs<F, T> a) {
    using R = real_of<F>;
    const int b = blockIdx.z;
    const int ox = a.x0[b], oy = a.y0[b];
    for (int x = a.hx + blockIdx.y; x < a.TX - a.hx; x += gridDim.y) {
        const int xg = ox + x;
        if (xg < 0 || xg >= a.FX) continue;
        F* dst = a.field + (size_t)xg * a.FY;
        const size_t row = ((size_t)b * a.TX + x) * a.TY;
        for (int y = a.hy + blockIdx.x * blockDim.x + threadIdx.x; y < a.TY - a.hy; y += gridDim.x * blockDim.x) {
            const int yg = oy + y;
            if (yg < 0 || yg >= a.FY) continue;
            const T va = a.tiles_a[row + y];
            R dx = (R)va.x, dy = (R)va.y;
            if (a.tiles_b) { const T vb = a.tiles_b[row + y]; dx -= (R)vb.x; dy -= (R)vb.y; }
            if (a.accumulate) { const F o = dst[yg]; dx += o.x; dy += o.y; }
            dst[yg] = make_c<F>(dx, dy);
        }
    }
}
// One workgroup per field row; it first lists the (tile, x) pairs that map onto its row, then every thread sums its columns
// over the list in a fixed order (deterministic, no atomics).  The list holds BDOF_TILE_MAXLIST pairs; a row with more is summed
// in chunks of whole tiles, in ascending tile order: thread 0 lists from the resume index and publishes where the next chunk
// starts, so the trip count is uniform across the workgroup; the first chunk honours `accumulate`, the later ones add to the
// field.  Any B; up to the list limit that is one chunk.  (The host sees to it that one tile alone fits: ceil(TX / FX) pairs.)
template <class F, class T>
__global__ __launch_bounds__(256) void k_tiles_cut_adjoint(TileArgs<F, T> a) {
    using R = real_of<F>;
    __shared__ int lb[BDOF_TILE_MAXLIST], lx[BDOF_TILE_MAXLIST];
    __shared__ int nlist, resume;
    for (int xg = blockIdx.x; xg < a.FX; xg += gridDim.x) {
        for (int b_next = 0; b_next < a.B;) {
            const bool first = b_next == 0;
            __syncthreads();
            if (threadIdx.x == 0) {
                int n = 0, b = b_next;
                for (; b < a.B; ++b) {
                    // tile rows x with (x0[b] + x) mod FX == xg
                    int x = wrap_idx(xg - a.x0[b], a.FX);
                    if (x < a.TX && n + (a.TX - 1 - x) / a.FX + 1 > BDOF_TILE_MAXLIST) break;      // the next chunk starts with this tile
                    for (; x < a.TX; x += a.FX) { lb[n] = b; lx[n] = x; ++n; }
                }
                nlist = n;
                resume = b;
            }
            __syncthreads();
            const int n = nlist;
            b_next = resume;
            for (int yg = threadIdx.x; yg < a.FY; yg += blockDim.x) {
                R sx = 0, sy = 0;
                for (int e = 0; e < n; ++e) {
                    const int b = lb[e], x = lx[e];
                    const R wx = taper_weight<R>(x, a.TX, a.taper);
                    for (int y = wrap_idx(yg - a.y0[b], a.FY); y < a.TY; y += a.FY) {
                        const R w = wx * taper_weight<R>(y, a.TY, a.taper);
                        const size_t o = ((size_t)b * a.TX + x) * a.TY + y;
                        const T va = a.tiles_a[o];
                        R dx = (R)va.x, dy = (R)va.y;
                        if (a.tiles_b) { const T vb = a.tiles_b[o]; dx -= (R)vb.x; dy -= (R)vb.y; }
                        sx = fma(w, dx, sx);
                        sy = fma(w, dy, sy);
                    }
                }
                F* dst = a.field + (size_t)xg * a.FY + yg;
                if (a.accumulate || !first) { sx += dst->x; sy += dst->y; }
                *dst = make_c<F>(sx, sy);
            }
        }
    }
}

// phi = c psi, c = exp(i k delta) exp(-k beta) from the caller's (delta, beta) rows (cnn_propagator/np_funcs.py:37-40), float64
struct Mod64Args {
    double2* field;      // [B][NX][NY]
    ObjView obj;         // .vol = the (delta, beta) rows themselves (not the float32 table of c - 1)
    int B, NX, NY, z;
    double k;
    double2* tape;       // nullable: phi_z is stored here too (the float64 loss + gradient paths keep every slice's)
};
__global__ __launch_bounds__(256) void k_f64_modulate(Mod64Args a) {
    const size_t n = (size_t)a.B * a.NX * a.NY;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (size_t)gridDim.x * blockDim.x) {
        const int y = idx % a.NY;
        const size_t r = idx / a.NY;
        const int x = r % a.NX, b = r / a.NX;
        const float2 db = g_mod_value(a.obj, b, x, y, a.z, a.NX);
        if (db.x == 0.f && db.y == 0.f) {                           // vacuum: c = 1
            if (a.tape) a.tape[idx] = a.field[idx];
            continue;
        }
        double s, cs;
        sincos(a.k * (double)db.x, &s, &cs);
        const double e = exp(-a.k * (double)db.y);
        const double2 v = a.field[idx];
        const double2 phi = make_double2(e * (v.x * cs - v.y * s), e * (v.x * s + v.y * cs));
        a.field[idx] = phi;
        if (a.tape) a.tape[idx] = phi;
    }
}

// D float32 copies of a float64 complex table whose roundings average to the float64 values (the dithered transform constants
// of bdof_fft.h, applied to the transfer function h): in copy d each part of entry i is rounded DOWN or UP — up in a fraction
// p = (x - lo) / (hi - lo) of the copies, spread evenly over d with a golden-ratio phase per entry — so that the mean over any
// run of L copies is x to ulp / L.  The launches of slice z take copy z mod D: a fixed float32 table is the same small
// perturbation of every slice, and its error adds up coherently (1.4e-5 of the exit wave after 1024 slices, measured with
// everything else in float64); the dithered copies' errors cancel (1e-6).
__device__ __forceinline__ float dither_round(double x, int d, double phase) {
    float lo = (float)x;
    if ((double)lo > x) lo = nextafterf(lo, -INFINITY);
    const float hi = nextafterf(lo, INFINITY);
    if ((double)lo == x) return lo;
    const double p = (x - (double)lo) / ((double)hi - (double)lo);
    return floor((d + 1) * p + phase) > floor(d * p + phase) ? hi : lo;
}
__global__ __launch_bounds__(256) void k_dither_copies(const double2* __restrict__ src, cf* __restrict__ dst, size_t n, int D) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const double2 v = src[i];
        const double g = (double)(i % 1048573) * 0.6180339887498949;
        const double ph = g - floor(g), ph2 = ph + 0.5 - floor(ph + 0.5);
        for (int d = 0; d < D; ++d) dst[(size_t)d * n + i] = make_float2(dither_round(v.x, d, ph), dither_round(v.y, d, ph2));
    }
}

// Carrier stack of a stitch range from the spectrum of the tiles' input: S_z = s_hat * H^z for z = 1 .. nz - 1, all of them in one
// pass (running product in double); h carries 1 / (NX NY), H = h * (NX NY).  spec [B][per] -> out [nz - 1][B][per]
__global__ __launch_bounds__(256) void k_carrier_spectra(const double2* __restrict__ spec, const double2* __restrict__ h, double2* __restrict__ out,
                                                         size_t per, int B, int nz, double scale_up) {
    const size_t n = per * B;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const double2 hk = h[i % per];
        const double hx = hk.x * scale_up, hy = hk.y * scale_up;            // the un-normalised H
        const double2 s0 = spec[i];
        double wx = hk.x, wy = hk.y;                                        // H^z / (NX NY), z = 1
        for (int z = 1; z < nz; ++z) {
            out[(size_t)(z - 1) * n + i] = make_double2(s0.x * wx - s0.y * wy, s0.x * wy + s0.y * wx);
            const double tx = wx * hx - wy * hy, ty = wx * hy + wy * hx;
            wx = tx; wy = ty;
        }
    }
}
