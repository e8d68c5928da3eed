// Generic-size engine: any NY x NX (e.g. the 72 x 72 ptychography probe of cnn_propagator/reconstruct_ptycho.py:106).
// The 2-D transforms are rocFFT's (batched, in place); everything else is the same physics as the fused engine written as
// point-wise kernels on real-space fields [b][x][y] (frequency domain [b][kx][ky]).  Unfused, so it moves ~2.5x the bytes
// of the fused row kernels — it exists for coverage of sizes without a hand-written plan and as an on-device cross-check.
#pragma once
#include "bdof_kernels.h"

struct GModArgs {
    cf* field;           // [B][NX][NY] eps part, updated in place
    const cf* probe;     // nullable: [NX][NY] eps part of the probe (first slice: field is written, not read)
    cf* tape;            // nullable: phi_z (eps part)
    ObjView obj;
    int B, NX, NY, z;
    cf carrier;
    const cf* pz;        // nullable: carrier field of the slice, [x][y] (bdof_set_probe_stack); the tape then holds the full phi
    cf cshift;           // a_z (cbar - 1), scalar carrier only (modulate_eps_s)
};

__device__ __forceinline__ float2 g_mod_value(const ObjView& o, int b, int x, int y, int z, int NX) {
    const long long srow = obj_src_row(o, b, x, z, NX);
    const int yg = y + (o.yoff ? o.yoff[b] : 0);
    const int yc = min(max(yg, 0), o.volNY - 1);
    const float2 v = o.vol[(size_t)(srow >= 0 ? srow : 0) * o.volNY + yc];
    const bool in = srow >= 0 && yg == yc;
    return make_float2(in ? v.x : 0.f, in ? v.y : 0.f);
}

// slice binning: c - 1 of step z's bin, the o.bin voxel slices combined as in load_obj_row_bin (bdof_kernels.h)
__device__ __forceinline__ float2 g_mod_value_bin(const ObjView& o, int b, int x, int y, int z, int NX) {
    float2 t = g_mod_value(o, b, x, y, z * o.bin, NX);
    for (int j = 1; j < o.bin; ++j) {
        const float2 u = g_mod_value(o, b, x, y, z * o.bin + j, NX);
        t = make_float2(t.x + u.x + (t.x * u.x - t.y * u.y), t.y + u.y + (t.x * u.y + t.y * u.x));
    }
    return t;
}

// BIN (here and in k_g_bwd): slice binning, a.z counts propagation steps
template <bool BIN>
__global__ __launch_bounds__(256) void k_g_modulate(GModArgs a) {
    const size_t n = (size_t)a.B * a.NX * a.NY;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (size_t)gridDim.x * blockDim.x) {
        const int y = idx % a.NY;
        const size_t r = idx / a.NY;
        const int x = r % a.NX, b = r / a.NX;
        const cf e = a.probe ? a.probe[(size_t)x * a.NY + y] : a.field[idx];
        const cf pc = a.pz ? a.pz[(size_t)x * a.NY + y] : a.carrier;
        const float2 m1 = BIN ? g_mod_value_bin(a.obj, b, x, y, a.z, a.NX) : g_mod_value(a.obj, b, x, y, a.z, a.NX);
        const cf phi = modulate_eps_s(e, pc, m1, a.cshift);
        a.field[idx] = phi;
        if (a.tape) a.tape[idx] = a.pz ? cadd(phi, pc) : phi;
    }
}

// The product of every rocFFT step: f[b][kx][ky] *= h (or its conjugate) on n = B NX NY numbers, C2 = float2 / double2.
// KYKX: the table is h[ky][kx], the fused engine's order, else h[kx][ky]; SCALED: the product times `scale` (a table that does
// not carry the transforms' 1 / (NX NY)).
// The order of the two loads is part of the arithmetic: hipcc contracts a.x t.y + a.y t.x into one product and one fma, and
// which of the two products it rounds follows the order in which a and t were loaded.  The [ky][kx] instances read the table
// first and the [kx][ky] ones the field first, as the kernels they replace did: the bits of either engine stay what they were
// (MEASUREMENTS.md, "rocFFT paths").
template <class C2, bool KYKX, bool SCALED = false>
__global__ __launch_bounds__(256) void k_hmul(C2* __restrict__ f, const C2* __restrict__ h, int NX, int NY, size_t n, int conj_h, decltype(C2::x) scale) {
    const size_t per_field = (size_t)NX * NY;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        C2 a, t;
        if (KYKX) { t = h[(i % NY) * (size_t)NX + (i / NY) % NX]; a = f[i]; }
        else { a = f[i]; t = h[i % per_field]; }
        if (conj_h) t.y = -t.y;
        C2 o;
        o.x = a.x * t.x - a.y * t.y;
        o.y = a.x * t.y + a.y * t.x;
        if (SCALED) { o.x *= scale; o.y *= scale; }
        f[i] = o;
    }
}

struct GLossArgs {
    cf* field;           // detector wave (eps part / far: un-shifted fft2), overwritten by the seed when meas != null
    cf* out_wave;        // nullable; real detectors [b][x][y], far field [b][ky][kx]
    const float* meas;   // nullable; same order as out_wave
    double* partial;     // [2 * gridDim.x]
    int B, NX, NY, far;
    double2* seed64;     // nullable [B][NX][NY]: float64 adjoint sweep (bdof_configure flag 64) — detector wave, residual and
                         // seed all formed in float64 and left here un-rounded
    int fstride = 1;     // PL instantiations only (in the bytes the alignment of `det` left empty): wavefield b of `field` is frame
                         // b * fstride of meas / out_wave — one detector plane of D, frames [B][D][NX][NY] (bdof_set_detector_planes)
    DetPlane det;        // bdof_kernels.h; pfield / pfield64 [x][y], far field [kx][ky]
};

// dst (+)= src, n complex numbers: the fan-in of the detector planes' adjoint steps
__global__ __launch_bounds__(256) void k_g_accumulate(cf* __restrict__ dst, const cf* __restrict__ src, size_t n, int first) {
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (size_t)gridDim.x * blockDim.x)
        dst[idx] = first ? src[idx] : cadd(dst[idx], src[idx]);
}

// PSN: the Poisson data term (seed_weight, bdof_kernels.h); WGT: detector weights, det.wgt in the order of one wavefield of meas
// PL: one detector plane of several (GLossArgs::fstride; real-space detectors)
template <bool PSN, bool WGT = false, bool PL = false>
__global__ __launch_bounds__(256) void k_g_loss(GLossArgs a) {
    const size_t n = (size_t)a.B * a.NX * a.NY;
    const DetPlane& det = a.det;
    double acc = 0.0, acc2 = 0.0;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (size_t)gridDim.x * blockDim.x) {
        const int y = idx % a.NY;
        const size_t r = idx / a.NY;
        const int x = r % a.NX, b = r / a.NX;
        const size_t pi = (size_t)x * a.NY + y;                                    // in the carrier field's plane
        const size_t oi = PL ? idx + (size_t)b * (a.fstride - 1) * a.NX * a.NY
                             : a.far ? ((size_t)b * a.NY + y) * a.NX + x : idx;         // in meas / out_wave
        const bool dc = x == 0 && y == 0;
        const float w = a.meas ? det_weight<WGT>(det, a.far ? (size_t)y * a.NX + x : pi) : 1.f;
        cf d = a.field[idx];
        if (a.seed64 && a.meas) {
            double2 p = make_double2(0.0, 0.0);
            if (det.pfield64) p = det.pfield64[pi];
            else if (det.pfield) { const cf q = det.pfield[pi]; p = make_double2((double)q.x, (double)q.y); }
            else if (!a.far || dc) p = det.carrier_dd;
            p = make_double2(p.x + (double)d.x, p.y + (double)d.y);
            a.seed64[idx] = seed_f64<PSN, WGT>(p, (double)a.meas[oi] + det.meas_ref, (double)det.seed_scale, det.mu, acc, acc2, w);
            if (a.out_wave) a.out_wave[oi] = make_float2((float)p.x, (float)p.y);
            continue;
        }
        if (det.meas_dev && a.meas && !a.far && !det.pfield) {
            const size_t si = PL ? oi : idx;        // (real-space detector: without PL the frame index is the field's)
            if (a.out_wave) a.out_wave[si] = cadd(d, det.carrier);
            a.field[idx] = seed_split<PSN, WGT>(d, a.meas[si], det, acc, acc2, w);
            continue;
        }
        if (det.pfield64 && a.meas) {
            cf dw;
            a.field[idx] = seed_f64<PSN, WGT>(d, det_field64(det, pi), a.meas[oi], det, acc, acc2, dw, w);
            if (a.out_wave) a.out_wave[oi] = dw;
            continue;
        }
        const cf e0 = d;
        if (det.pfield) d = cadd(d, det.pfield[pi]);
        else if (!a.far || dc) d = cadd(d, det.carrier);
        if (a.out_wave) a.out_wave[oi] = d;
        if (a.meas && det.gcar && a.far && dc) {
            seed_dc_bin<PSN, WGT>(det, b, e0, a.meas[oi], acc, acc2);
            a.field[idx] = make_float2(0.f, 0.f);       // nothing of this bin goes through the transform back
            continue;
        }
        if (a.meas) a.field[idx] = seed_plain<PSN, WGT>(d, a.meas[oi], det, acc, acc2, w);
    }
    if (a.meas) block_store_sum2<256>(acc, acc2, a.partial + 2 * blockIdx.x);
}

struct GBwdArgs {
    cf* g;               // G(phi_z) in, G(psi_z) out (in place)
    const cf* tape;      // phi_z (eps part)
    float2* grot;
    ObjView obj;
    int B, NX, NY, z;
    float k;
    cf carrier;          // cbar a_z: constant part of phi_z
    int full_tape;       // the tape holds the full phi (carrier field), not its scattered part
    AdjCarrier ac;       // gcar nullable
};

template <bool BIN>
__global__ __launch_bounds__(256) void k_g_bwd(GBwdArgs a) {
    const size_t n = (size_t)a.B * a.NX * a.NY;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (size_t)gridDim.x * blockDim.x) {
        const int y = idx % a.NY;
        const size_t r = idx / a.NY;
        const int x = r % a.NX, b = r / a.NX;
        const cf G = a.g[idx];
        const cf e = a.tape[idx];
        const cf phi = a.full_tape ? e : cadd(e, a.carrier);
        cf t = cmulc(G, phi);
        const float2 m1 = BIN ? g_mod_value_bin(a.obj, b, x, y, a.z, a.NX) : g_mod_value(a.obj, b, x, y, a.z, a.NX);
        cf Gn = cmulc(G, make_float2(1.f + m1.x, m1.y));
        if (a.ac.gcar) {
            cf gam, t0;
            adj_carrier_load(a.ac, b, gam, t0);
            t = cadd(cadd(t, cmulc(gam, e)), t0);
            Gn = cadd(Gn, cmulc(gam, csub(m1, a.ac.cbm1)));
            // the sweep ends at slice 0: leave the FULL G(psi_0) = scattered part + conj(cbar) gamma for bdof_probe_grad
            if (a.z == 0) Gn = cadd(Gn, cmulc(gam, make_float2(1.f + a.ac.cbm1.x, a.ac.cbm1.y)));
        }
        const float2 gv = make_float2(a.k * t.y, -a.k * t.x);
        if constexpr (BIN) {                  // the bin's one gradient value to each of its voxel slices
            for (int j = 0; j < a.obj.bin; ++j) a.grot[(((size_t)b * a.obj.S + a.z * a.obj.bin + j) * a.NX + x) * a.NY + y] = gv;
        } else {
            a.grot[(((size_t)b * a.obj.S + a.z) * a.NX + x) * a.NY + y] = gv;
        }
        a.g[idx] = Gn;
    }
}


// ---- float64 adjoint sweep (bdof_configure flag 64) -------------------------------------------------------------------------
// The adjoint field G is as large as the wave itself and has no known part to split off (it is driven by the data's noise), so
// its float32 transform chain sets a floor of ~3e-6 under the gradient (64 slices) — and Adam's first step of every epoch,
// lr g / (|g| + 1e-8), turns an absolute error of 1e-8 at a voxel where the gradient changes sign into a fraction of a whole
// step.  With this option the seed, the adjoint transforms (rocFFT double precision), the transfer function and
// the products conj(phi) G are float64; the forward sweep (scattered wave on its carrier) and the tape stay float32.
struct GBwd64Args {
    double2* g;          // G(phi_z) in, G(psi_z) out
    const cf* tape;      // phi_z (scattered part, or the full phi with a carrier field)
    float2* grot;
    ObjView obj;
    int B, NX, NY, z;
    double k;
    double2 carrier;     // constant part of phi_z
    int full_tape;
};
__global__ __launch_bounds__(256) void k_g_bwd64(GBwd64Args a) {
    const size_t n = (size_t)a.B * a.NX * a.NY;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (size_t)gridDim.x * blockDim.x) {
        const int y = idx % a.NY;
        const size_t r = idx / a.NY;
        const int x = r % a.NX, b = r / a.NX;
        const double2 G = a.g[idx];
        const cf e = a.tape[idx];
        const double px = (double)e.x + (a.full_tape ? 0.0 : a.carrier.x), py = (double)e.y + (a.full_tape ? 0.0 : a.carrier.y);
        const double tx = G.x * px + G.y * py, ty = G.y * px - G.x * py;             // G conj(phi)
        a.grot[(((size_t)b * a.obj.S + a.z) * a.NX + x) * a.NY + y] = make_float2((float)(a.k * ty), (float)(-a.k * tx));
        const float2 m1 = g_mod_value(a.obj, b, x, y, a.z, a.NX);
        const double cx = 1.0 + (double)m1.x, cy = (double)m1.y;
        a.g[idx] = make_double2(G.x * cx + G.y * cy, G.y * cx - G.x * cy);           // G conj(c)
    }
}
__global__ __launch_bounds__(256) void k_d_scale(double2* f, size_t n, double s) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        f[i] = make_double2(f[i].x * s, f[i].y * s);
}

// ---- float64 helpers of bdof_set_probe_field: the carrier field of a localised probe, propagated on the device ------------
__global__ __launch_bounds__(256) void k_d_copy(const double2* __restrict__ src, double2* __restrict__ dst, int n0, int n1, int transposed) {
    const size_t n = (size_t)n0 * n1;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (size_t)gridDim.x * blockDim.x)
        dst[transposed ? (idx % n1) * (size_t)n0 + idx / n1 : idx] = src[idx];
}
// dst[i] = (float2) src[i]; transposed: dst[j * n0 + i] = src[i * n1 + j] for an [n0][n1] source
__global__ __launch_bounds__(256) void k_d_to_f(const double2* __restrict__ src, cf* __restrict__ dst, int n0, int n1, int transposed) {
    const size_t n = (size_t)n0 * n1;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (size_t)gridDim.x * blockDim.x) {
        const double2 v = src[idx];
        const size_t o = transposed ? (idx % n1) * (size_t)n0 + idx / n1 : idx;
        dst[o] = make_float2((float)v.x, (float)v.y);
    }
}
