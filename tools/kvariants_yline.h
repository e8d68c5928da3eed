// What-if variants of the plain y-line slice kernels for timing in kbench_yline (development aid; MODE > 0 gives wrong results).
// The body is the kernels' form BEFORE the rotation lookups were moved to the top of the tile (obj_src_row inside the pass loop, behind
// the row's loads; hy of the trailing step requested behind the row's stores), so that the what-if table keeps its meaning:
//   MODE 0 (a): that form as it was
//   MODE 1 (b): the source row is arithmetic on (b, x, z) — a scattered row of the volume, as a rotation gives, but no lookup at all
//   MODE 2 (c): (b), and hy of the trailing step requested ahead of the row's stores
// (a) - (b) bounds what taking the lookups out of the pass loop can win, (b) - (c) what the early request of hy can.
#pragma once
#include "../beyond_dof_amd/csrc/bdof_kernels.h"

// a source row without a lookup: 18 bits of a multiplicative hash, < 512 * 512 rows (kbench_yline's volume)
__device__ __forceinline__ long long kv_src_row(const ObjView& o, int b, int x, int z, int NX) {
    return (long long)(((unsigned)((b * o.S + z) * NX + x) * 2654435761u) >> 14);
}

template <int NY, int MODE>
__global__ __launch_bounds__(BDOF_THREADS, RowCfg<NY>::MIN_WAVES) void kv_slice_y(SliceArgs a) {
    typedef RowCfg<NY> C;
    __shared__ cf smem[C::LDS_CF];
    __shared__ cf smem_tw[2][FftTw<NY>::LDS_CNT];
    __shared__ cf smem_tail[2][7 * C::T];
    const int tid = threadIdx.x % C::T, rl = threadIdx.x / C::T;
    const float sql[2] = {a.steps.sq_lead[0], a.steps.sq_lead[1]}, sqt[2] = {a.steps.sq_trail[0], a.steps.sq_trail[1]};
    FftTw<NY> tw;
    FftTw<NY>::fill(a.steps.tw_lead, smem_tw[0], smem_tail[0]);
    FftTw<NY>::fill(a.steps.tw_trail, smem_tw[1], smem_tail[1]);
    __syncthreads();
    const int NX = a.R;
    const int ntiles = a.B * NX / C::TILE;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const auto [row0, b, x0] = tile_at<C>(tile, NX);
#pragma nounroll
        for (int pass = 0; pass < C::PASSES; ++pass) {
            const int r = pass * C::RPP + rl;
            const int x = x0 + r;
            RowLds<C::T> lds{smem + r * C::RS};
            cf u[8], hv[8];
            float2 db[8];
            const cf* src = a.in + (size_t)(row0 + r) * NY;
#pragma unroll
            for (int m = 0; m < 8; ++m) u[m] = src[tid + m * C::T];
            load_obj_row(a.obj, MODE == 0 ? obj_src_row(a.obj, b, x, a.z, NX) : kv_src_row(a.obj, b, x, a.z, NX), 0, tid, C::T, db);
#pragma unroll
            for (int m = 0; m < 8; ++m) hv[m] = a.steps.h_lead[tid + m * C::T];
            tw_select(tw, smem_tw[0], smem_tail[0], sql, tid);
            line_fft<NY, -1, 1, false>(u, tw, tid, lds);
#pragma unroll
            for (int m = 0; m < 8; ++m) u[m] = cmul(u[m], hv[m]);
            line_fft<NY, +1, 2, false>(u, tw, tid, lds);
#pragma unroll
            for (int m = 0; m < 8; ++m) u[m] = modulate_eps_s(u[m], a.carrier, db[m], a.cshift);
            if constexpr (MODE == 2) {
#pragma unroll
                for (int m = 0; m < 8; ++m) hv[m] = a.steps.h_trail[tid + m * C::T];
            }
            cf* pdst = a.phi_out + (size_t)(row0 + r) * NY;
#pragma unroll
            for (int m = 0; m < 8; ++m) pdst[tid + m * C::T] = u[m];
            tw_select(tw, smem_tw[1], smem_tail[1], sqt, tid);
            if constexpr (MODE < 2) {
#pragma unroll
                for (int m = 0; m < 8; ++m) hv[m] = a.steps.h_trail[tid + m * C::T];
            }
            line_fft<NY, -1, 1, false>(u, tw, tid, lds);
            if constexpr (MODE == 2) use_from_here(hv);
#pragma unroll
            for (int m = 0; m < 8; ++m) u[m] = cmul(u[m], hv[m]);
            line_fft_partial<NY, +1, 2, false>(u, tw, tid, lds);
        }
        __syncthreads();
        transposed_tail<NY, +1, 2, false>(smem, a.out + (size_t)b * NY * NX + x0, NX, 1.f, smem_tail[1], sqt);
        __syncthreads();
    }
}

template <int NY, int MODE>
__global__ __launch_bounds__(BDOF_THREADS, RowCfg<NY>::MIN_WAVES) void kv_slice_y_adj(SliceAdjArgs a) {
    typedef RowCfg<NY> C;
    __shared__ cf smem[C::LDS_CF];
    __shared__ cf smem_tw[2][FftTw<NY>::LDS_CNT];
    __shared__ cf smem_tail[2][7 * C::T];
    const int tid = threadIdx.x % C::T, rl = threadIdx.x / C::T;
    const float sql[2] = {a.steps.sq_lead[0], a.steps.sq_lead[1]}, sqt[2] = {a.steps.sq_trail[0], a.steps.sq_trail[1]};
    FftTw<NY> tw;
    FftTw<NY>::fill(a.steps.tw_lead, smem_tw[0], smem_tail[0]);
    FftTw<NY>::fill(a.steps.tw_trail, smem_tw[1], smem_tail[1]);
    __syncthreads();
    const ObjView o = a.obj;                              // (MODE > 0 at 512 points: 24 bytes of scratch, their times are upper estimates)
    const int NX = a.R;
    const int ntiles = a.B * NX / C::TILE;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const auto [row0, b, x0] = tile_at<C>(tile, NX);
#pragma nounroll
        for (int pass = 0; pass < C::PASSES; ++pass) {
            const int r = pass * C::RPP + rl;
            const int x = x0 + r;
            RowLds<C::T> lds{smem + r * C::RS};
            const size_t off = (size_t)(row0 + r) * NY;
            cf g[8], p[8], hv[8];
            float2 db[8];
#pragma unroll
            for (int m = 0; m < 8; ++m) g[m] = a.in[off + tid + m * C::T];
#pragma unroll
            for (int m = 0; m < 8; ++m) hv[m] = a.steps.h_lead[tid + m * C::T];
            tw_select(tw, smem_tw[0], smem_tail[0], sql, tid);
            line_fft<NY, -1, 1, false>(g, tw, tid, lds);
#pragma unroll
            for (int m = 0; m < 8; ++m) g[m] = cmulc(g[m], hv[m]);
#pragma unroll
            for (int m = 0; m < 8; ++m) p[m] = a.phi[off + tid + m * C::T];
            load_obj_row(o, MODE == 0 ? obj_src_row(o, b, x, a.z, NX) : kv_src_row(o, b, x, a.z, NX), 0, tid, C::T, db);
            line_fft<NY, +1, 2, false>(g, tw, tid, lds);
            float2* gdst = a.grot + (((size_t)b * o.S + a.z) * NX + x) * NY;
            float2 gv[8];
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const cf t = cmulc(g[m], cadd(p[m], a.carrier_phi));
                gv[m] = make_float2(a.k * t.y, -a.k * t.x);
                g[m] = cmulc(g[m], make_float2(1.f + db[m].x, db[m].y));
            }
            if constexpr (MODE == 2) {
#pragma unroll
                for (int m = 0; m < 8; ++m) hv[m] = a.steps.h_trail[tid + m * C::T];
            }
#pragma unroll
            for (int m = 0; m < 8; ++m) gdst[tid + m * C::T] = gv[m];
            if constexpr (MODE < 2) {
#pragma unroll
                for (int m = 0; m < 8; ++m) hv[m] = a.steps.h_trail[tid + m * C::T];
            }
            tw_select(tw, smem_tw[1], smem_tail[1], sqt, tid);
            line_fft<NY, -1, 1, false>(g, tw, tid, lds);
            if constexpr (MODE == 2) use_from_here(hv);
#pragma unroll
            for (int m = 0; m < 8; ++m) g[m] = cmulc(g[m], hv[m]);
            line_fft_partial<NY, +1, 2, false>(g, tw, tid, lds);
        }
        __syncthreads();
        transposed_tail<NY, +1, 2, false>(smem, a.out + (size_t)b * NY * NX + x0, NX, 1.f, smem_tail[1], sqt);
        __syncthreads();
    }
}
