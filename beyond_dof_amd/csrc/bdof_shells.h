// Fourier shell / ring correlation of two (delta, beta) volumes (bdof_shell_correlation; tensorflow_recon/util.py:975-1048).
//
// A volume of pairs is the complex volume c = delta + i beta, and ONE complex transform C = F c holds both channels' spectra:
//     F_delta(k) = (C(k) + conj C(-k)) / 2,      F_beta(k) = (C(k) - conj C(-k)) / (2i).
// k_shell_widen writes c in complex128 (exact), rocFFT transforms it in place, and k_shell_sums goes over both spectra once and
// files every point's seven terms under its shell:
//     n, Re(Fa conj Fb), |Fa|^2, |Fb|^2 of delta, the same three of beta.
//
// Shells are hard and decided in integers (ShellGeom): with L the least common multiple of the axes longer than 1, Nref the
// shortest of them and w = L / Nref, a point with signed indices k_i has u = 4 sum (k_i L / N_i)^2 and lies in the shell s with
// (2s - 1)^2 w^2 <= u < (2s + 1)^2 w^2 — s = floor(Nref |f| + 1/2), |f| in cycles per voxel — whatever a compiler makes of the
// floating-point estimate the search starts from.
//
// No sum depends on arrival order (no atomics).  A wave owns the rows (x, z) = wave, wave + waves, ... and takes each row in two
// halves (k_y >= 0, k_y < 0), along which the shell index is monotone, in chunks of 64 consecutive y.  Within a chunk a segmented
// scan adds the runs of equal shell; the last lane of a run adds the run to the wave's own LDS table (the runs of one chunk have
// distinct shells, and a wave's LDS operations keep their order).  The workgroup's tables are added in wave order into
// partial[block][shells][7], and k_shell_blocks adds the blocks in block order.
#pragma once
#include <hip/hip_runtime.h>

#define BDOF_SHELL_TERMS 7
#define BDOF_SHELL_LDS_BYTES 65536      // what one workgroup's tables may take: waves x shells x 7 doubles

struct ShellGeom {
    int NX, NZ, NY;                     // the volume [X][Z][Y]
    unsigned long long sx, sz, sy;      // L / N_i (of an axis of length 1: unused, its k is 0)
    unsigned long long w;               // L / Nref
    int s_lo, s_n;                      // the shells this launch files: [s_lo, s_lo + s_n)
};

// c = delta + i beta in complex128
__global__ __launch_bounds__(256) void k_shell_widen(const float2* __restrict__ v, double2* __restrict__ c, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float2 p = v[i];
        c[i] = make_double2((double)p.x, (double)p.y);
    }
}

__device__ __forceinline__ long long shell_signed(int j, int N) { return j < (N + 1) / 2 ? j : j - N; }

// the shell of u: the floating-point estimate, then the integer rule decides
__device__ __forceinline__ int shell_of(unsigned long long u, unsigned long long w) {
    long long s = (long long)(sqrt((double)u) / (double)(2 * w) + 0.5);
    const unsigned long long lo = (unsigned long long)(2 * s - 1) * w, hi = (unsigned long long)(2 * s + 1) * w;
    if (s > 0 && lo * lo > u) --s;
    else if (hi * hi <= u) ++s;
    return (int)s;
}

// partial: [gridDim.x][s_n][7]; dynamic LDS: [waves of the block][s_n][7] doubles
__global__ __launch_bounds__(256) void k_shell_sums(const double2* __restrict__ Ca, const double2* __restrict__ Cb, ShellGeom g,
                                                   double* __restrict__ partial) {
    extern __shared__ double shell_tab[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int nent = g.s_n * BDOF_SHELL_TERMS;
    for (int i = threadIdx.x; i < waves * nent; i += blockDim.x) shell_tab[i] = 0.0;
    __syncthreads();
    double* tab = shell_tab + (size_t)wave * nent;
    const int h = (g.NY + 1) / 2;                                   // y < h: k_y >= 0
    const long long rows = (long long)g.NX * g.NZ;
    for (long long row = (long long)blockIdx.x * waves + wave; row < rows; row += (long long)gridDim.x * waves) {
        const int x = (int)(row / g.NZ), z = (int)(row % g.NZ);
        const long long kx = shell_signed(x, g.NX) * (long long)g.sx, kz = shell_signed(z, g.NZ) * (long long)g.sz;
        const unsigned long long r2 = (unsigned long long)(kx * kx) + (unsigned long long)(kz * kz);
        const size_t base = (size_t)row * g.NY;
        const size_t mbase = ((size_t)((g.NX - x) % g.NX) * g.NZ + (size_t)((g.NZ - z) % g.NZ)) * g.NY;      // the row of -k
        for (int half = 0; half < 2; ++half) {
            const int y0 = half ? h : 0, y1 = half ? g.NY : h;
            for (int yc = y0; yc < y1; yc += 64) {
                const int y = yc + lane;
                int key = -1;                                       // no point, or a shell this launch does not file
                double t[BDOF_SHELL_TERMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                if (y < y1) {
                    const long long ky = shell_signed(y, g.NY) * (long long)g.sy;
                    const int s = shell_of(4ull * (r2 + (unsigned long long)(ky * ky)), g.w) - g.s_lo;
                    if (s >= 0 && s < g.s_n) {
                        key = s;
                        const size_t my = (size_t)((g.NY - y) % g.NY);
                        const double2 a = Ca[base + y], am = Ca[mbase + my], b = Cb[base + y], bm = Cb[mbase + my];
                        // F_delta = (C(k) + conj C(-k)) / 2, F_beta = (C(k) - conj C(-k)) / (2i)
                        const double adr = 0.5 * (a.x + am.x), adi = 0.5 * (a.y - am.y), abr = 0.5 * (a.y + am.y), abi = -0.5 * (a.x - am.x);
                        const double bdr = 0.5 * (b.x + bm.x), bdi = 0.5 * (b.y - bm.y), bbr = 0.5 * (b.y + bm.y), bbi = -0.5 * (b.x - bm.x);
                        t[0] = 1.0;
                        t[1] = adr * bdr + adi * bdi;
                        t[2] = adr * adr + adi * adi;
                        t[3] = bdr * bdr + bdi * bdi;
                        t[4] = abr * bbr + abi * bbi;
                        t[5] = abr * abr + abi * abi;
                        t[6] = bbr * bbr + bbi * bbi;
                    }
                }
                // segmented inclusive scan: equal keys are contiguous, so an equal key d lanes down is the same run
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const int kd = __shfl_up(key, d, 64);
                    const bool take = lane >= d && kd == key;
#pragma unroll
                    for (int j = 0; j < BDOF_SHELL_TERMS; ++j) {
                        const double up = __shfl_up(t[j], d, 64);
                        if (take) t[j] += up;
                    }
                }
                const int knext = __shfl_down(key, 1, 64);
                if (key >= 0 && (lane == 63 || knext != key)) {
                    double* e = tab + (size_t)key * BDOF_SHELL_TERMS;
#pragma unroll
                    for (int j = 0; j < BDOF_SHELL_TERMS; ++j) e[j] += t[j];
                }
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nent; i += blockDim.x) {
        double s = shell_tab[i];
        for (int wv = 1; wv < waves; ++wv) s += shell_tab[(size_t)wv * nent + i];
        partial[(size_t)blockIdx.x * nent + i] = s;
    }
}

// out[i] = partial[0][i] + partial[1][i] + ... in block order, i < nent
__global__ __launch_bounds__(256) void k_shell_blocks(const double* __restrict__ partial, int blocks, int nent, double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nent) return;
    double s = 0.0;
    for (int b = 0; b < blocks; ++b) s += partial[(size_t)b * nent + i];
    out[i] = s;
}
