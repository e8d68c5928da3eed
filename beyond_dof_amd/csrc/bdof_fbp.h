// Analytic starting volume for full field (bdof_ctf_retrieve, bdof_backproject, bdof_volume_clip_mask; DESIGN §3 "Analytic start"):
// contrast-transfer-function retrieval of the projected absorption from D detector planes, the real-space Ram-Lak filter along the
// detector's x, and the back-projection of the filtered frames through the rigid maps (M | t) the run rotates with.
//
// Retrieval, per angle b and plane d, on the work area work[d][b][x][y] (complex128, owned by the ctx):
//     k_fbp_contrast   g = m^2 / |a0|^2 - 1 in double from the float32 amplitude, 0 where the weight plane is 0 (whatever m holds)
//     (host)           work[d] <- F^-1( G_d F work[d] ): the double-precision free-space step of the rocFFT paths, G_d the host's filter
//     k_fbp_ramp       q[b][x][y] = sum_x' h[x - x'] sum_d Re work[d][b][x'][y],  h[0] = 1/4, h[m] = -1 / (pi^2 m^2) for odd m, else 0,
//                      in float64, rounded once to float32; the frame is zero outside itself (no padding, no wrap-around)
// Back-projection, a gather without atomics:
//     k_fbp_backproject   vol[p] (+)= (scale_delta, scale_beta) sum_b w_b bilinear(q_b; o_x, o_y),  o = M_b^T (p - t_b)
#pragma once
#include <hip/hip_runtime.h>

// work[d][b][x][y] = (m^2 / a0_sq - 1, 0) from meas[b][d][x][y]; wgt: [x][y] or nullptr
__global__ __launch_bounds__(256) void k_fbp_contrast(const float* __restrict__ meas, const float* __restrict__ wgt, double a0_sq,
                                                     double2* __restrict__ work, int B, int D, size_t plane) {
    const size_t n = (size_t)B * D * plane;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t pix = i % plane, f = i / plane;               // f = b D + d
        const size_t b = f / D, d = f - b * D;
        double g = 0.0;
        if (!wgt || wgt[pix] != 0.f) {
            const double m = (double)meas[i];
            g = m * m / a0_sq - 1.0;
        }
        work[(d * B + b) * plane + pix] = make_double2(g, 0.0);
    }
}

// The Ram-Lak row filter.  A workgroup takes one frame b, 64 columns y (the lanes, along the contiguous axis) and 64 output rows x;
// it walks the source rows x' in blocks of 64 staged in LDS (the planes' real parts summed in ascending d).  A wave's 16 output rows
// have one parity: waves 0 and 2 the even rows of the tile, 1 and 3 the odd ones.  Only the taps that are not zero are computed:
// the rows x' of the other parity, and the centre.  Order of the sum: per block of 64 source rows, its rows of the other parity in
// ascending x', then the centre tap if the output row lies in that block.
#define FBP_RAMP_TILE 64
__global__ __launch_bounds__(256) void k_fbp_ramp(const double2* __restrict__ work, float* __restrict__ q, int B, int D, int NX, int NY) {
    extern __shared__ double fbp_lds[];
    double* taps = fbp_lds;                                    // [NX]: h[m], m >= 0 (0 for even m > 0)
    double* tile = fbp_lds + NX;                               // [64][64]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.z, y = blockIdx.x * 64 + lane, xt = blockIdx.y * FBP_RAMP_TILE;
    const size_t plane = (size_t)NX * NY;
    const double pi2 = 3.141592653589793 * 3.141592653589793;
    for (int m = threadIdx.x; m < NX; m += blockDim.x)
        taps[m] = m == 0 ? 0.25 : (m & 1) ? -1.0 / (pi2 * ((double)m * (double)m)) : 0.0;
    const int x_first = xt + (wave & 1) + 32 * (wave >> 1);   // this wave's rows: x_first + 2 j, j < 16
    double acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.0;
    for (int s0 = 0; s0 < NX; s0 += FBP_RAMP_TILE) {
        __syncthreads();                                       // (the taps; the previous block's readers)
        for (int r = wave; r < FBP_RAMP_TILE; r += 4) {
            const int xs = s0 + r;
            double v = 0.0;
            if (xs < NX && y < NY)
                for (int d = 0; d < D; ++d) v += work[((size_t)d * B + b) * plane + (size_t)xs * NY + y].x;
            tile[r * 64 + lane] = v;
        }
        __syncthreads();
        // rows of the other parity than this wave's: r = (1 - parity), + 2, ... (s0 and xt are even)
        for (int r = 1 - (wave & 1); r < FBP_RAMP_TILE; r += 2) {
            const int xs = s0 + r;
            if (xs >= NX) break;
            const double v = tile[r * 64 + lane];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int m = x_first + 2 * j - xs;
                const int am = m < 0 ? -m : m;
                if (am < NX) acc[j] = fma(taps[am], v, acc[j]);       // (am >= NX: an output row beyond the frame, not stored)
            }
        }
        // the centre tap of the rows of this wave that lie in this block
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int r = x_first + 2 * j - s0;
            if (r >= 0 && r < FBP_RAMP_TILE) acc[j] = fma(0.25, tile[r * 64 + lane], acc[j]);
        }
    }
    if (y < NY) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int x = x_first + 2 * j;
            if (x < NX) q[(size_t)b * plane + (size_t)x * NY + y] = (float)acc[j];
        }
    }
}

// bilinear sample of one frame [NXd][NYd] at (ox, oy): coordinates in float64 (as rigid_point), the two factors per axis rounded
// to float32, their product and the four-tap sum in float32 in the order (0,0) (0,1) (1,0) (1,1); a tap outside counts 0
__device__ __forceinline__ float fbp_sample(const float* __restrict__ f, int NXd, int NYd, double ox, double oy) {
    const double flx = floor(fmin(fmax(ox, -2.0), (double)NXd + 1.0)), fly = floor(fmin(fmax(oy, -2.0), (double)NYd + 1.0));
    const double frx = fmin(fmax(ox - flx, 0.0), 1.0), fry = fmin(fmax(oy - fly, 0.0), 1.0);
    const int ix = (int)flx, iy = (int)fly;
    const float wx[2] = {(float)(1.0 - frx), (float)frx}, wy[2] = {(float)(1.0 - fry), (float)fry};
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int px = ix + i, py = iy + j;
            if (px >= 0 && px < NXd && py >= 0 && py < NYd) s = fmaf(wx[i] * wy[j], f[(size_t)px * NYd + py], s);
        }
    return s;
}

struct FbpBackArgs {
    const float* q;            // [B][NXd][NYd]
    const double* prm;         // [B][12]: rows of (M | t)
    const float* w;            // [B]
    float2* vol;               // [NXv][NZv][NYv] (delta, beta)
    int B, NXd, NYd, NXv, NZv, NYv;
    int d0, d1;                // destination rows (x' NZv + z') [d0, d1)
    int accumulate;
    float sd, sb;              // scale_delta, scale_beta
};

// One wave per destination row (x', z') (4 consecutive rows per workgroup: they read neighbouring detector rows of every frame, and
// all of a workgroup's voxels walk the frames in the same order), lanes along y'; the angle loop innermost, the two running sums in
// registers, the rows of prm and w uniform over the wave.  Each channel's sum runs in float32 in ascending b:
//     acc = fmaf(scale w_b, s_b, acc),  starting from 0, or with `accumulate` from what the volume holds
// so that a second call with the next angles continues the very sum one call over all of them forms; a voxel's arithmetic does not
// depend on the launch, so slab-wise, whole-volume and repeated calls give the same bits.
__global__ __launch_bounds__(256) void k_fbp_backproject(FbpBackArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t frame = (size_t)a.NXd * a.NYd;
    for (int d = a.d0 + blockIdx.x * 4 + wave; d < a.d1; d += gridDim.x * 4) {
        const int xp = d / a.NZv, zp = d - xp * a.NZv;
        for (int yp = lane; yp < a.NYv; yp += 64) {
            const size_t dest = (size_t)d * a.NYv + yp;
            float2 acc = a.accumulate ? a.vol[dest] : make_float2(0.f, 0.f);
            for (int b = 0; b < a.B; ++b) {
                const double* m = a.prm + 12 * (size_t)b;
                const double v0 = xp - m[3], v1 = zp - m[7], v2 = yp - m[11];
                const double ox = fma(m[8], v2, fma(m[4], v1, m[0] * v0));          // (M^T (p - t))_x
                const double oy = fma(m[10], v2, fma(m[6], v1, m[2] * v0));         // (M^T (p - t))_y
                const float s = fbp_sample(a.q + (size_t)b * frame, a.NXd, a.NYd, ox, oy);
                const float wb = a.w[b];
                acc.x = fmaf(a.sd * wb, s, acc.x);
                acc.y = fmaf(a.sb * wb, s, acc.y);
            }
            a.vol[dest] = acc;
        }
    }
}

// vol = max(vol, 0) * mask (mask per voxel, or nullptr): what an initial guess goes through before it is bound
__global__ __launch_bounds__(256) void k_fbp_clip_mask(float2* __restrict__ vol, const float* __restrict__ mask, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float2 p = vol[i];
        const float mk = mask ? mask[i] : 1.f;
        p.x = fmaxf(p.x, 0.f) * mk;
        p.y = fmaxf(p.y, 0.f) * mk;
        vol[i] = p;
    }
}
