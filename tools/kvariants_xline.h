// What-if variants of the x-line slice kernels for timing in kbench_xline (development aid; MODE > 0 gives wrong results).
// The body is the kernels' form BEFORE their operand requests were moved (lookups through LDS behind the phase barrier, table / phi
// loads at the top of each transposed pass, behind the pass before it's stores), so that the what-if table keeps its meaning:
//   MODE 0 (a): that form as it was
//   MODE 1 (b): the transposed phase's table / phi operands are constants, no loads there (the lookups go with them)
//   MODE 2 (c): (b) and the phase's phi / gradient stores dropped as well
// (a) - (b) is what hiding the loads can win at most, (b) - (c) what the stores cost.
#pragma once
#include "../beyond_dof_amd/csrc/bdof_kernels.h"

template <int NX, bool BLK, int MODE>
__global__ __launch_bounds__(BDOF_THREADS, RowCfg<NX>::MIN_WAVES) void kv_slice_x(SliceArgs a) {
    typedef RowCfg<NX> C;
    typedef FftPlan<NX> P;
    __shared__ cf smem[C::LDS_CF];
    __shared__ cf smem_tw[2][FftTw<NX>::LDS_CNT];
    __shared__ cf smem_tail[2][7 * C::T];
    const int tid = threadIdx.x % C::T, rl = threadIdx.x / C::T;
    const float sql[2] = {a.steps.sq_lead[0], a.steps.sq_lead[1]}, sqt[2] = {a.steps.sq_trail[0], a.steps.sq_trail[1]};
    __shared__ int s_src[NX];
    FftTw<NX> tw;
    FftTw<NX>::fill(a.steps.tw_lead, smem_tw[0], smem_tail[0]);
    FftTw<NX>::fill(a.steps.tw_trail, smem_tw[1], smem_tail[1]);
    __syncthreads();
    const ObjView o = a.obj;
    const int NY = a.R;
    const int ntiles = a.B * NY / C::TILE;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const auto [row0, b, y0] = tile_at<C>(tile, NY);
        const ObjRows rows = obj_rows_of(o, b, a.z, NX);
        cf* const pdst = a.phi_out + (BLK ? (size_t)row0 * NX : (size_t)b * NX * NY);
        int src_mine = -1;
        if constexpr (MODE == 0) src_mine = (int)threadIdx.x < NX ? obj_rows_rel(rows, threadIdx.x) : -1;
#pragma nounroll
        for (int pass = 0; pass < C::PASSES; ++pass) {
            const int r = pass * C::RPP + rl;
            RowLds<C::T> lds{smem + r * C::RS};
            cf u[8], hv[8];
            const cf* src = a.in + (size_t)(row0 + r) * NX;
#pragma unroll
            for (int m = 0; m < 8; ++m) u[m] = src[tid + m * C::T];
#pragma unroll
            for (int m = 0; m < 8; ++m) hv[m] = a.steps.h_lead[tid + m * C::T];
            tw_select(tw, smem_tw[0], smem_tail[0], sql, tid);
            line_fft<NX, -1, 1, false>(u, tw, tid, lds);
#pragma unroll
            for (int m = 0; m < 8; ++m) u[m] = cmul(u[m], hv[m]);
            line_fft_partial<NX, +1, 2, false>(u, tw, tid, lds);
        }
        if constexpr (MODE == 0) { if ((int)threadIdx.x < NX) s_src[threadIdx.x] = src_mine; }
        __syncthreads();
        cf v[C::PASSES][8];
#pragma unroll
        for (int pass = 0; pass < C::PASSES; ++pass) {
            const auto [q, r, j] = transposed_at<C>(pass);
            RowLds<C::T> lds{smem + r * C::RS};
            const int yg = y0 + r, yc = min(max(yg, 0), o.volNY - 1);
            float2 db[8];
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                if constexpr (MODE == 0) {
                    const int srel = s_src[j + m * C::T];
                    const float2 t = o.vol[(size_t)(rows.plain0 + max(srel, 0)) * o.volNY + yc];
                    const bool in = srel >= 0 && yg == yc;
                    db[m] = make_float2(in ? t.x : 0.f, in ? t.y : 0.f);
                } else {
                    db[m] = make_float2(1e-6f * (m + 1), 1e-7f * (yc & 7));
                }
            }
            last_stage<NX, +1, 2, false>(v[pass], j, lds, smem_tail[0], sql);
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                v[pass][m] = modulate_eps_s(v[pass][m], a.carrier, db[m], a.cshift);
                if (MODE < 2 || v[pass][m].x == 123.456f) {      // MODE 2: keeps the value alive, practically never stores
                    if constexpr (BLK) pdst[(unsigned)(q + m * C::T * C::TILE)] = v[pass][m];
                    else pdst[(unsigned)((j + m * C::T) * NY + yg)] = v[pass][m];
                }
            }
            tw.sq = sqt;
            stage_compute<NX, -1, P::R0, 1, 0, 1, false>(v[pass], tw, j);
        }
        __syncthreads();
#pragma unroll
        for (int pass = 0; pass < C::PASSES; ++pass) {
            const auto [q, r, j] = transposed_at<C>(pass);
            RowLds<C::T> lds{smem + r * C::RS};
            stage_write<NX, P::R0, 1>(v[pass], j, lds);
        }
        __syncthreads();
#pragma nounroll
        for (int pass = 0; pass < C::PASSES; ++pass) {
            const int r = pass * C::RPP + rl;
            RowLds<C::T> lds{smem + r * C::RS};
            cf u[8], hv[8];
#pragma unroll
            for (int m = 0; m < 8; ++m) hv[m] = a.steps.h_trail[tid + m * C::T];
            tw_select(tw, smem_tw[1], smem_tail[1], sqt, tid);
            line_fft_rest<NX, -1, 1, false>(u, tw, tid, lds);
#pragma unroll
            for (int m = 0; m < 8; ++m) u[m] = cmul(u[m], hv[m]);
            line_fft_partial<NX, +1, 2, false>(u, tw, tid, lds);
        }
        __syncthreads();
        transposed_tail<NX, +1, 2, false>(smem, a.out + (size_t)b * NX * NY + y0, NY, 1.f, smem_tail[1], sqt);
        __syncthreads();
    }
}

template <int NX, int MODE>
__global__ __launch_bounds__(BDOF_THREADS, RowCfg<NX>::MIN_WAVES) void kv_slice_x_adj(SliceAdjArgs a) {
    typedef RowCfg<NX> C;
    typedef FftPlan<NX> P;
    __shared__ cf smem[C::LDS_CF];
    __shared__ cf smem_tw[2][FftTw<NX>::LDS_CNT];
    __shared__ cf smem_tail[2][7 * C::T];
    const int tid = threadIdx.x % C::T, rl = threadIdx.x / C::T;
    const float sql[2] = {a.steps.sq_lead[0], a.steps.sq_lead[1]}, sqt[2] = {a.steps.sq_trail[0], a.steps.sq_trail[1]};
    __shared__ int s_src[NX];
    FftTw<NX> tw;
    FftTw<NX>::fill(a.steps.tw_lead, smem_tw[0], smem_tail[0]);
    FftTw<NX>::fill(a.steps.tw_trail, smem_tw[1], smem_tail[1]);
    __syncthreads();
    const ObjView o = a.obj;
    const int NY = a.R;
    const int ntiles = a.B * NY / C::TILE;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const auto [row0, b, y0] = tile_at<C>(tile, NY);
        const ObjRows rows = obj_rows_of(o, b, a.z, NX);
        const cf* const psrc = a.phi + (size_t)row0 * NX;
        float2* const gdst = a.grot + ((size_t)b * o.S + a.z) * NX * NY;
        int src_mine = -1;
        if constexpr (MODE == 0) src_mine = (int)threadIdx.x < NX ? obj_rows_rel(rows, threadIdx.x) : -1;
#pragma nounroll
        for (int pass = 0; pass < C::PASSES; ++pass) {
            const int r = pass * C::RPP + rl;
            RowLds<C::T> lds{smem + r * C::RS};
            cf u[8], hv[8];
            const cf* src = a.in + (size_t)(row0 + r) * NX;
#pragma unroll
            for (int m = 0; m < 8; ++m) u[m] = src[tid + m * C::T];
#pragma unroll
            for (int m = 0; m < 8; ++m) hv[m] = a.steps.h_lead[tid + m * C::T];
            tw_select(tw, smem_tw[0], smem_tail[0], sql, tid);
            line_fft<NX, -1, 1, false>(u, tw, tid, lds);
#pragma unroll
            for (int m = 0; m < 8; ++m) u[m] = cmulc(u[m], hv[m]);
            line_fft_partial<NX, +1, 2, false>(u, tw, tid, lds);
        }
        if constexpr (MODE == 0) { if ((int)threadIdx.x < NX) s_src[threadIdx.x] = src_mine; }
        __syncthreads();
        cf v[C::PASSES][8];
#pragma unroll
        for (int pass = 0; pass < C::PASSES; ++pass) {
            const auto [q, r, j] = transposed_at<C>(pass);
            RowLds<C::T> lds{smem + r * C::RS};
            const int yg = y0 + r, yc = min(max(yg, 0), o.volNY - 1);
            float2 db[8];
            cf p[8];
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                if constexpr (MODE == 0) {
                    const int srel = s_src[j + m * C::T];
                    const float2 t = o.vol[(size_t)(rows.plain0 + max(srel, 0)) * o.volNY + yc];
                    const bool in = srel >= 0 && yg == yc;
                    db[m] = make_float2(in ? t.x : 0.f, in ? t.y : 0.f);
                    p[m] = psrc[(unsigned)(q + m * C::T * C::TILE)];
                } else {
                    db[m] = make_float2(1e-6f * (m + 1), 1e-7f * (yc & 7));
                    p[m] = make_float2(0.25f * (m + 1), 0.125f * (yc & 7));
                }
            }
            last_stage<NX, +1, 2, false>(v[pass], j, lds, smem_tail[0], sql);
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const cf t = cmulc(v[pass][m], cadd(p[m], a.carrier_phi));
                if (MODE < 2 || t.x == 123.456f) gdst[(unsigned)((j + m * C::T) * NY + yg)] = make_float2(a.k * t.y, -a.k * t.x);
                v[pass][m] = cmulc(v[pass][m], make_float2(1.f + db[m].x, db[m].y));
            }
            tw.sq = sqt;
            stage_compute<NX, -1, P::R0, 1, 0, 1, false>(v[pass], tw, j);
        }
        __syncthreads();
#pragma unroll
        for (int pass = 0; pass < C::PASSES; ++pass) {
            const auto [q, r, j] = transposed_at<C>(pass);
            RowLds<C::T> lds{smem + r * C::RS};
            stage_write<NX, P::R0, 1>(v[pass], j, lds);
        }
        __syncthreads();
#pragma nounroll
        for (int pass = 0; pass < C::PASSES; ++pass) {
            const int r = pass * C::RPP + rl;
            RowLds<C::T> lds{smem + r * C::RS};
            cf u[8], hv[8];
#pragma unroll
            for (int m = 0; m < 8; ++m) hv[m] = a.steps.h_trail[tid + m * C::T];
            tw_select(tw, smem_tw[1], smem_tail[1], sqt, tid);
            line_fft_rest<NX, -1, 1, false>(u, tw, tid, lds);
#pragma unroll
            for (int m = 0; m < 8; ++m) u[m] = cmulc(u[m], hv[m]);
            line_fft_partial<NX, +1, 2, false>(u, tw, tid, lds);
        }
        __syncthreads();
        transposed_tail<NX, +1, 2, false>(smem, a.out + (size_t)b * NX * NY + y0, NY, 1.f, smem_tail[1], sqt);
        __syncthreads();
    }
}
