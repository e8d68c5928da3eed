// Trilinear rotation of the object under an arbitrary rigid map per batch element (laminography tilt, axis roll, centre of
// rotation, per-angle wobble) and its exact adjoint: the 3-D counterpart of k_rot_bilinear / k_rot_bilinear_adjoint, for an
// axis that is not the volume's y axis, so that y mixes and a rotated row is no longer a weighted sum of whole volume rows.
//
// prm[b] = the rows of (M | t), 12 float64: output voxel o = (x, z, y) of rotated object b samples the volume at
// p = M o + t in index coordinates (x', z', y'), trilinearly over the 8 surrounding voxels, taps outside the volume count 0.
// Volume rows [X][Z][Y], rotated rows [b][z][x][y] (the layout of already rotated objects, as for the bilinear rotation).
// M is orthonormal with det +1 (the caller's precondition): the adjoint's candidate search relies on |M a| = |a|.
#pragma once
#include "bdof_kernels.h"

using RotRigidArgs = RotArgs<double>;        // prm [B][12]

// The source point of output voxel (x, z, y) under m = (M | t): the lower corner i0 of its cell and, per axis, the two factors
// (one minus the fraction, the fraction) rounded to float32.  Coordinates in float64: the row's base point M (x, z, 0) + t, then
// one fma per axis along y (x and z are invariants of both kernels' y loops, so the base is formed once per row).
// rigid_point and rigid_weight are the only place where a coordinate or a weight is formed: the forward kernel reaches them
// through rigid_taps, the adjoint directly, so the adjoint's weights are the forward's, bit for bit.
__device__ __forceinline__ void rigid_point(const double* __restrict__ m, int x, int z, int y, int NX, int NZ, int NY, int (&i0)[3],
                                            float (&f)[3][2]) {
    const int n[3] = {NX, NZ, NY};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double base = fma(m[4 * a + 1], (double)z, fma(m[4 * a], (double)x, m[4 * a + 3]));
        const double p = fma(m[4 * a + 2], (double)y, base);
        // (a point far outside is clamped before the conversion: every tap of it is outside either way)
        const double fl = floor(fmin(fmax(p, -2.0), (double)n[a] + 1.0));
        const double fr = fmin(fmax(p - fl, 0.0), 1.0);
        i0[a] = (int)fl;
        f[a][0] = (float)(1.0 - fr);
        f[a][1] = (float)fr;
    }
}
// the weight of the cell's corner (ix, iz, iy): the float32 product of three factors, in this order
__device__ __forceinline__ float rigid_weight(const float (&f)[3][2], int ix, int iz, int iy) {
    return ((ix ? f[0][1] : f[0][0]) * (iz ? f[1][1] : f[1][0])) * (iy ? f[2][1] : f[2][0]);
}
// The eight (voxel index, weight) pairs of output voxel (x, z, y): tap i = 4 ix + 2 iz + iy; a tap outside the volume gets
// index 0 and weight 0.
__device__ __forceinline__ void rigid_taps(const double* __restrict__ m, int x, int z, int y, int NX, int NZ, int NY, int (&idx)[8],
                                           float (&wt)[8]) {
    int i0[3];
    float f[3][2];
    rigid_point(m, x, z, y, NX, NZ, NY, i0, f);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int ix = i >> 2, iz = (i >> 1) & 1, iy = i & 1;
        const int px = i0[0] + ix, pz = i0[1] + iz, py = i0[2] + iy;
        const bool in = px >= 0 && px < NX && pz >= 0 && pz < NZ && py >= 0 && py < NY;
        idx[i] = in ? (px * NZ + pz) * NY + py : 0;
        wt[i] = in ? rigid_weight(f, ix, iz, iy) : 0.f;
    }
}

// Forward gather: one wave per output row (4 rows per workgroup), lanes along y.  MOD: the rows are written as modulation
// factors c - 1 of the interpolated (delta, beta), with the per-workgroup float64 sums of c - 1 in `partial` when the
// mean-refraction carrier needs them (what k_rot_bilinear<true> does).
template <bool MOD>
__global__ __launch_bounds__(256) void k_rot_rigid(RotRigidArgs a, float k, double2* __restrict__ partial) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t nrows = (size_t)a.B * a.NZv * a.NXv;
    double sx = 0.0, sy = 0.0;
    for (size_t o = (size_t)blockIdx.x * 4 + wave; o < nrows; o += (size_t)gridDim.x * 4) {
        const int x = o % a.NXv;
        const size_t r = o / a.NXv;
        const int z = r % a.NZv, b = r / a.NZv;
        const double* m = a.prm + 12 * (size_t)b;
        float2* dst = a.rot + o * a.NYv;
        for (int y = lane; y < a.NYv; y += 64) {
            int idx[8];
            float wt[8];
            rigid_taps(m, x, z, y, a.NXv, a.NZv, a.NYv, idx, wt);
            float2 acc = make_float2(0.f, 0.f);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (wt[i] != 0.f) {
                    const float2 s = a.vol[idx[i]];
                    acc.x = fmaf(wt[i], s.x, acc.x);
                    acc.y = fmaf(wt[i], s.y, acc.y);
                }
            }
            if constexpr (MOD) {
                acc = slice_modulation_m1(acc, k);
                sx += (double)acc.x;
                sy += (double)acc.y;
            }
            dst[y] = acc;
        }
    }
    if constexpr (MOD) {
        if (partial) rot_mod_partial(sx, sy, wave, lane, partial);
    }
}

// Adjoint, as a gather (deterministic, no atomics): destination voxel v' collects w * g(o) from the outputs o of which it is a
// tap.  Such an o has its source point p = M o + t within one voxel of v' on every axis, so with o* = M^T (v' - t)
//     |o - o*|_i = |M^T (p - v')|_i < sum_j |M_ji| =: r_i <= sqrt(3):
// the candidates are the lattice points of that box (2 to 4 per axis), clipped to the rotated frame.  One wave per destination
// row, lanes along y'; a lane walks its own voxel's candidates in the fixed order (b, x, z, y ascending) and takes each one's
// weight from rigid_point / rigid_weight (v' is in the volume, so the tap is) — no exchange between lanes, so neither a ballot
// nor a compacted list is needed for the order to be fixed, and slab-wise, whole-volume and repeated runs give the same bits.
__global__ __launch_bounds__(256) void k_rot_rigid_adjoint(RotRigidArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int NX = a.NXv, NZ = a.NZv, NY = a.NYv;
    for (int d = a.d0 + blockIdx.x * 4 + wave; d < a.d1; d += gridDim.x * 4) {
        const int xp = d / NZ, zp = d - xp * NZ;             // (x', z')
        for (int yp = lane; yp < NY; yp += 64) {
            const int dest = d * NY + yp;
            float2 acc = make_float2(0.f, 0.f);
            for (int b = 0; b < a.B; ++b) {
                const double* m = a.prm + 12 * (size_t)b;
                const double v0 = xp - m[3], v1 = zp - m[7], v2 = yp - m[11];
                int lo[3], hi[3];
                const int n[3] = {NX, NZ, NY};
                // M is orthonormal to 1e-9 only (util.check_rigid), so M^T is the inverse to about 3e-9 per entry and o* is off
                // by up to that times |v' - t|_1: the slack of the box grows with the extent
                const double slack = 4e-9 * (1.0 + fabs(v0) + fabs(v1) + fabs(v2));
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const double os = fma(m[8 + i], v2, fma(m[4 + i], v1, m[i] * v0));          // (M^T (v' - t))_i
                    const double r = fabs(m[i]) + fabs(m[4 + i]) + fabs(m[8 + i]) + slack;
                    lo[i] = (int)fmax(ceil(os - r), 0.0);
                    hi[i] = (int)fmin(floor(os + r), (double)(n[i] - 1));
                }
                for (int x = lo[0]; x <= hi[0]; ++x)
                    for (int z = lo[1]; z <= hi[1]; ++z) {
                        const float2* grow = a.rot + (((size_t)b * NZ + z) * NX + x) * NY;
                        for (int y = lo[2]; y <= hi[2]; ++y) {
                            int i0[3];
                            float f[3][2];
                            rigid_point(m, x, z, y, NX, NZ, NY, i0, f);
                            const int ix = xp - i0[0], iz = zp - i0[1], iy = yp - i0[2];      // which corner of o's cell v' is: 0 or 1 each
                            if ((ix | iz | iy) & ~1) continue;
                            const float w = rigid_weight(f, ix, iz, iy);
                            if (w != 0.f) {
                                const float2 g = grow[y];
                                acc.x = fmaf(w, g.x, acc.x);
                                acc.y = fmaf(w, g.y, acc.y);
                            }
                        }
                    }
            }
            float2 o = make_float2(acc.x * a.scale, acc.y * a.scale);
            if (a.accumulate) { const float2 p = a.gvol[dest]; o.x += p.x; o.y += p.y; }
            a.gvol[dest] = o;
        }
    }
}

// ---- the derivative of a loss with respect to the map itself ---------------------------------------------------------------------------
// dL/d prm[b][a][j] = sum_o q_a(o) (x, z, y, 1)_j,   q_a(o) = sum_c g_c(o) dV_c/dp_a (p(o)),   a in x', z', y':
// g the rotated-frame gradient, dV/dp_a taken INSIDE the cell floor(p) that rigid_point gives: over the cell's 8 corners, (-1 or +1
// by the corner's bit along a) times the product of the other two axes' factors times V(corner), a corner outside the volume counting
// 0 as in rigid_taps.  A point on a lattice plane belongs to the cell floor gives it: the right-hand derivative (at zero tilt and
// roll the y fraction is exactly 0 at every voxel, so the convention is the common case, not the edge).
//
// The partial count and the rows of a workgroup depend on (NXv, NZv) only — not on the CU count, not on B — and nothing is added
// atomically: element b has the same bits alone, in a batch and twice.
#define RIGID_PG_MAX_PARTIALS 512
__host__ __device__ inline int rigid_param_partials(int NXv, int NZv) {
    const long long groups = ((long long)NXv * NZv + 3) / 4;             // 4 rows (waves) per workgroup pass
    return (int)(groups < RIGID_PG_MAX_PARTIALS ? groups : RIGID_PG_MAX_PARTIALS);
}

// One wave per output row (b, z, x), lanes along y as in k_rot_rigid; grid B P, workgroup p of element b takes the rows
// 4 (p + i P) + wave, i = 0, 1, ....  Two-factor weights, tap sums and q_a in float32; the sums over voxels in float64: per row
// the lanes keep sum q_a and sum q_a y (x and z are the row's), folded into the 12 running sums at the row's end.  Then the wave
// (shuffles), the workgroup's waves in wave order (LDS), and one record of 12 per workgroup: partial [B][P][12].
__global__ __launch_bounds__(256) void k_rot_rigid_param_grad(RotRigidArgs a, int P, double* __restrict__ partial) {
    __shared__ double w[4][12];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int NX = a.NXv, NZ = a.NZv, NY = a.NYv;
    const int b = blockIdx.x / P, p = blockIdx.x - b * P, nrows = NX * NZ;
    const double* m = a.prm + 12 * (size_t)b;
    double acc[3][4];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    for (int r = p * 4 + wave; r < nrows; r += P * 4) {
        const int x = r % NX, z = r / NX;
        const float2* grow = a.rot + ((size_t)b * nrows + r) * NY;
        double s[3] = {0.0, 0.0, 0.0}, sy[3] = {0.0, 0.0, 0.0};
        for (int y = lane; y < NY; y += 64) {
            int i0[3];
            float f[3][2];
            rigid_point(m, x, z, y, NX, NZ, NY, i0, f);
            float2 d[3] = {make_float2(0.f, 0.f), make_float2(0.f, 0.f), make_float2(0.f, 0.f)};      // dV/dp_a, both channels
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int ix = i >> 2, iz = (i >> 1) & 1, iy = i & 1;
                const int px = i0[0] + ix, pz = i0[1] + iz, py = i0[2] + iy;
                if (px >= 0 && px < NX && pz >= 0 && pz < NZ && py >= 0 && py < NY) {
                    const float2 v = a.vol[(px * NZ + pz) * NY + py];
                    const float fx = f[0][ix], fz = f[1][iz], fy = f[2][iy];
                    const float wx = ix ? fz * fy : -(fz * fy), wz = iz ? fx * fy : -(fx * fy), wy = iy ? fx * fz : -(fx * fz);
                    d[0].x = fmaf(wx, v.x, d[0].x);
                    d[0].y = fmaf(wx, v.y, d[0].y);
                    d[1].x = fmaf(wz, v.x, d[1].x);
                    d[1].y = fmaf(wz, v.y, d[1].y);
                    d[2].x = fmaf(wy, v.x, d[2].x);
                    d[2].y = fmaf(wy, v.y, d[2].y);
                }
            }
            const float2 g = grow[y];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double q = (double)fmaf(g.y, d[k].y, g.x * d[k].x);
                s[k] += q;
                sy[k] = fma(q, (double)y, sy[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            acc[k][0] = fma(s[k], (double)x, acc[k][0]);
            acc[k][1] = fma(s[k], (double)z, acc[k][1]);
            acc[k][2] += sy[k];
            acc[k][3] += s[k];
        }
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        double v = acc[i >> 2][i & 3];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) w[wave][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < 12) {
        const int i = threadIdx.x;
        partial[(size_t)blockIdx.x * 12 + i] = ((w[0][i] + w[1][i]) + w[2][i]) + w[3][i];
    }
}

// the P records of element b added in ascending order: out [B][12] (+= with accumulate); grid B, one wave
__global__ __launch_bounds__(64) void k_rot_rigid_param_sum(const double* __restrict__ partial, int P, double* __restrict__ out, int accumulate) {
    const int b = blockIdx.x, i = threadIdx.x;
    if (i >= 12) return;
    double s = 0.0;
    for (int p = 0; p < P; ++p) s += partial[((size_t)b * P + p) * 12 + i];
    out[12 * (size_t)b + i] = accumulate ? out[12 * (size_t)b + i] + s : s;
}
