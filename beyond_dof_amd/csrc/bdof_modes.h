// Probe modes (bdof_set_probe_modes, include/bdof.h): the recorded intensity is the incoherent sum I = sum_m |d_m|^2 over M
// orthogonal probe modes (partial coherence, fly scans; Thibault & Menzel).  Wavefield (m, j) — mode m of window j — lives at
// index m B + j of every per-wavefield buffer, so a mode is a sub-batch of B wavefields at shifted pointers and the sweeps of
// both engines stay what they are.  What couples the modes sits between the forward and the adjoint sweep, in one kernel shared
// by the resident and the generic engine, and in the sum of the per-mode gradient rows behind the adjoint sweep.
// No kernel here waits for another workgroup: the coupling across modes happens inside one thread, or between launches.
#pragma once
#include "bdof_kernels.h"

struct ModesArgs {
    const cf* e;             // [M][B][NX][NY] scattered parts of the detector waves as the forward sweep left them: every field
                             // [x][y] (far field [kx][ky]), or — e_meas_order — in the index order of one frame of meas
    cf* seed;                // [M][B][NX][NY] seeds G(d_m), every field [x][y] (far field [kx][ky]); written only with meas.  May be
                             // `e` itself unless e_meas_order: a thread reads the M values of its pixel before it writes them
    cf* out_wave;            // nullable [M][B][NX][NY]: the full detector waves d_m, frames in the order of meas
    const float* meas;       // nullable [B][NX][NY]; real-space detectors [x][y], far field the un-shifted [ky][kx]
    const double2* pdet64;   // [M][NX][NY] float64 carriers at the detector, [x][y] (far field [kx][ky])
    const float* wgt;        // WGT instances: one plane in the order of one frame of meas
    double* partial;         // [2 * gridDim.x]
    int M, B, NX, NY, far, e_meas_order;
    double seed_scale;       // 2 / (B NX NY): the measured pixels, not times M
    double mu;               // PSN instances
};

// Per pixel of each window: d_m = p_m + e_m in float64, a = sqrt(sum_m |d_m|^2), r = a - m, the ONE factor f of the data term
// (seed_weight, as every detector kernel takes it) shared by the modes, seeds f d_m rounded once.  a = 0 gives f = 0: no epsilon.
// The modes are summed in ascending m by one thread and the two sums of the loss per workgroup in wave order: a fixed order.
template <bool PSN, bool WGT>
__global__ __launch_bounds__(256) void k_modes_couple(ModesArgs a) {
    const size_t plane = (size_t)a.NX * a.NY, n = (size_t)a.B * plane;      // n: the stride from one mode to the next
    double acc = 0.0, acc2 = 0.0;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (size_t)gridDim.x * blockDim.x) {
        const int y = idx % a.NY;
        const size_t r = idx / a.NY;
        const int x = r % a.NX;
        const size_t b = r / a.NX;
        const size_t pi = (size_t)x * a.NY + y;                               // in a carrier's plane
        const size_t wi = a.far ? (size_t)y * a.NX + x : pi;                  // in a frame of meas
        const size_t oi = b * plane + wi;
        const size_t ei = a.e_meas_order ? oi : idx;
        double s = 0.0;
        for (int m = 0; m < a.M; ++m) {
            const double2 p = a.pdet64[m * plane + pi];
            const cf e = a.e[m * n + ei];
            const double dx = p.x + (double)e.x, dy = p.y + (double)e.y;
            s += dx * dx + dy * dy;
        }
        double f = 0.0;
        if (a.meas) {
            const double ab = sqrt(s), ms = (double)a.meas[oi];
            f = seed_weight<PSN, WGT, double>(ab - ms, ab, ms, a.seed_scale, a.mu, WGT ? a.wgt[wi] : 1.f, acc, acc2);
        }
        for (int m = 0; m < a.M; ++m) {
            const double2 p = a.pdet64[m * plane + pi];
            const cf e = a.e[m * n + ei];
            const double dx = p.x + (double)e.x, dy = p.y + (double)e.y;
            if (a.out_wave) a.out_wave[m * n + oi] = make_float2((float)dx, (float)dy);
            if (a.meas) a.seed[m * n + idx] = make_float2((float)(f * dx), (float)(f * dy));
        }
    }
    if (a.meas) block_store_sum2<256>(acc, acc2, a.partial + 2 * blockIdx.x);
}

// g[i] = g[0][i] + g[1][i] + ... + g[M - 1][i] on n pairs, modes in ascending order: the per-mode gradient rows [M][B][S][NX][NY]
// of the adjoint sweeps summed into the [B][S][NX][NY] that everything behind bdof_loss_grad reads (bdof_grot).  A term that is
// zero is not added: -0 + (+0) is +0, and a mode that contributes nothing must leave the other modes' sum its bits, sign of a zero
// included.
__global__ __launch_bounds__(256) void k_modes_sum_rows(float2* g, int M, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float2 v = g[i];
        for (int m = 1; m < M; ++m) {
            const float2 u = g[(size_t)m * n + i];
            if (u.x != 0.f) v.x += u.x;
            if (u.y != 0.f) v.y += u.y;
        }
        g[i] = v;
    }
}
