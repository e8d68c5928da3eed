// Development aid (not part of the product): what do the rotation lookups inside the y-line slice kernels' pass loop cost?
// k_slice_y<512> and k_slice_y_adj<512> (plain instances) against their what-if variants (kvariants_yline.h): (a) the form before
// the lookups were moved to the top of the tile, (b) the source row as arithmetic, no lookup at all, (c) as (b) with hy of the trailing
// step requested ahead of the row's stores — and the product kernels.
// 13 and 25 wavefields per launch (a sub-batch of the flagship and the whole minibatch).  The wavefield buffers are one pair (the
// sweep's ping-pong sits in the Infinity Cache); tape, gradient slices and table are beyond it, as the sweep sees them: a ring
// of 16 tape slots and gradient slices (840 MB each at 25 fields), a 1 GiB table behind random lookups that change with the slice.
// Every launch takes the next slot of the ring (turn++), so within a repetition the kernels see different slots of it.
// The variants compute nonsense; every launch chain is checked and the program stops at the first failure.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -o tools/kbench_yline tools/kbench_yline.hip && ./tools/kbench_yline [iters] [reps]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <vector>
#include <algorithm>
#include "kvariants_yline.h"

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

static int balanced(int tiles, int cap) { if (tiles <= cap) return tiles; int r = (tiles + cap - 1) / cap; return (tiles + r - 1) / r; }

template <class F> static float time_it(F f, int iters) {
    hipEvent_t a, b;
    CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    f(); f();
    CK(hipDeviceSynchronize());
    CK(hipGetLastError());
    CK(hipEventRecord(a));
    for (int i = 0; i < iters; ++i) f();
    CK(hipEventRecord(b));
    CK(hipEventSynchronize(b));
    float ms = 0; CK(hipEventElapsedTime(&ms, a, b));
    CK(hipGetLastError());
    CK(hipEventDestroy(a)); CK(hipEventDestroy(b));
    return ms / iters;
}

int main(int argc, char** argv) {
    constexpr int N = 512, S = 16, BMAX = 25;
    const int iters = argc > 1 ? atoi(argv[1]) : 32, reps = argc > 2 ? atoi(argv[2]) : 5;
    const size_t fld = (size_t)BMAX * N * N;
    cf *in, *out, *tape, *h, *tw; float2 *vol, *grot; int *tab, *ang;
    CK(hipMalloc(&in, fld * 8)); CK(hipMalloc(&out, fld * 8)); CK(hipMalloc(&tape, fld * S * 8)); CK(hipMalloc(&grot, fld * S * 8));
    CK(hipMalloc(&h, N * 8)); CK(hipMalloc(&tw, N * 8));
    CK(hipMalloc(&vol, (size_t)N * N * N * 8)); CK(hipMalloc(&tab, (size_t)BMAX * S * N * 4)); CK(hipMalloc(&ang, BMAX * 4));
    {
        std::vector<cf> hw(N), hh(N);
        for (int j = 0; j < N; ++j) {
            hw[j] = make_float2((float)cos(-2 * M_PI * j / N), (float)sin(-2 * M_PI * j / N));
            hh[j] = make_float2((float)cos(1e-3 * j * j) / N, (float)sin(1e-3 * j * j) / N);
        }
        CK(hipMemcpy(tw, hw.data(), N * 8, hipMemcpyHostToDevice));
        CK(hipMemcpy(h, hh.data(), N * 8, hipMemcpyHostToDevice));
        std::vector<float> rnd(fld * 2);
        for (auto& v : rnd) v = (float)(rand() % 2001 - 1000) * 1e-3f;
        CK(hipMemcpy(in, rnd.data(), fld * 8, hipMemcpyHostToDevice));
        for (int s = 0; s < S; ++s) CK(hipMemcpy(tape + fld * s, rnd.data(), fld * 8, hipMemcpyHostToDevice));
        std::vector<float> v((size_t)N * N * N * 2);
        for (auto& x : v) x = 1e-9f * (float)(rand() % 1000);
        CK(hipMemcpy(vol, v.data(), v.size() * 4, hipMemcpyHostToDevice));
        std::vector<int> t((size_t)BMAX * S * N), a(BMAX);
        for (auto& x : t) x = rand() % (N * N);              // random source rows, like a generic rotation angle
        for (int b = 0; b < BMAX; ++b) a[b] = b;
        CK(hipMemcpy(tab, t.data(), t.size() * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(ang, a.data(), BMAX * 4, hipMemcpyHostToDevice));
    }
    ObjView obj{vol, tab, ang, nullptr, nullptr, S, N, N};
    hipDeviceProp_t prop; CK(hipGetDeviceProperties(&prop, 0));
    const int ncu = prop.multiProcessorCount;
    LineSteps st{tw, tw, h, h, {0.70710678f, 0.70710678f}, {0.70710678f, 0.70710678f}};
    int turn = 0;
    for (int B : {13, 25}) {
        const int tiles = B * N / RowCfg<N>::TILE, grid = balanced(tiles, ncu * 2);
        const size_t slot = (size_t)B * N * N;                // a launch's tape slot and its fields' gradient slice z: B fields
        auto fwd_args = [&] {
            const int z = turn++ % S;
            return SliceArgs{in, nullptr, out, tape + slot * z, obj, B, N, z, make_float2(1.f, 0.f), make_float2(1e-3f, 0.f), st};
        };
        auto adj_args = [&] {
            const int z = turn++ % S;
            return SliceAdjArgs{in, tape + slot * z, out, grot, obj, B, N, z, 25.3f, make_float2(1.f, 0.f), st};
        };
        const char* names[8] = {"k_slice_y<512>           product", "                     (a) before ", "                     (b) no lookup",
                                "                     (c) hy early ", "k_slice_y_adj<512>       product", "                     (a) before ",
                                "                     (b) no lookup", "                     (c) hy early "};
        float lo[8], hi[8];
        for (int k = 0; k < 8; ++k) { lo[k] = 1e9f; hi[k] = 0.f; }
        for (int rep = 0; rep < reps; ++rep) {
            float t[8];
            t[0] = time_it([&] { hipLaunchKernelGGL((k_slice_y<N, false, false>), dim3(grid), dim3(BDOF_THREADS), 0, 0, fwd_args()); }, iters);
            t[1] = time_it([&] { hipLaunchKernelGGL((kv_slice_y<N, 0>), dim3(grid), dim3(BDOF_THREADS), 0, 0, fwd_args()); }, iters);
            t[2] = time_it([&] { hipLaunchKernelGGL((kv_slice_y<N, 1>), dim3(grid), dim3(BDOF_THREADS), 0, 0, fwd_args()); }, iters);
            t[3] = time_it([&] { hipLaunchKernelGGL((kv_slice_y<N, 2>), dim3(grid), dim3(BDOF_THREADS), 0, 0, fwd_args()); }, iters);
            t[4] = time_it([&] { hipLaunchKernelGGL((k_slice_y_adj<N, false, false>), dim3(grid), dim3(BDOF_THREADS), 0, 0, adj_args()); }, iters);
            t[5] = time_it([&] { hipLaunchKernelGGL((kv_slice_y_adj<N, 0>), dim3(grid), dim3(BDOF_THREADS), 0, 0, adj_args()); }, iters);
            t[6] = time_it([&] { hipLaunchKernelGGL((kv_slice_y_adj<N, 1>), dim3(grid), dim3(BDOF_THREADS), 0, 0, adj_args()); }, iters);
            t[7] = time_it([&] { hipLaunchKernelGGL((kv_slice_y_adj<N, 2>), dim3(grid), dim3(BDOF_THREADS), 0, 0, adj_args()); }, iters);
            for (int k = 0; k < 8; ++k) { lo[k] = std::min(lo[k], t[k]); hi[k] = std::max(hi[k], t[k]); }
        }
        printf("-- %d wavefields per launch, %d tiles on %d workgroups, %d launches x %d repetitions (alternated): us per launch, least .. most\n",
               B, tiles, grid, iters, reps);
        for (int k = 0; k < 8; ++k) printf("%s  %7.2f .. %7.2f\n", names[k], lo[k] * 1e3, hi[k] * 1e3);
    }
    return 0;
}
