// Host-side check of the index arithmetic of the windows at fractional origins (beyond_dof_amd/csrc/bdof_windows.h) under a
// sanitizer: walks the forward gather, the list of a column, the (j0, b) sort, the streaming loop of the overlap-add and the
// position derivative's reads exactly as the kernels index them, over buffers sized as bdof_capi.hip sizes them (one element per
// pair), so that an index outside its buffer is the sanitizer's to report.  It also checks that the adjoint visits exactly the
// (window, tap, frame element) triples the forward gather reads — the two are transposes of each other —, that the host count of
// windows per column (win_max_per_column, the entry point's check) is the length of the longest list, and the clamp of origins
// far outside, NaN and infinite ones included.
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o check_window_index tools/check_window_index.cpp
//   ./check_window_index          (exit code 0 and "ok" when every case passes)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <map>
#include <tuple>
#include <vector>

#include "../beyond_dof_amd/csrc/bdof_windows.h"

static int fails = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            std::printf("FAILED %s: ", #cond);             \
            std::printf(__VA_ARGS__);                      \
            std::printf("\n");                             \
            ++fails;                                       \
        }                                                  \
    } while (0)

using Visit = std::map<std::tuple<int, int, int, int, int>, int>;       // (b, tap, z, xg, y) -> times

static void walk(int volNX, int S, int volNY, int NX, int NY, const std::vector<double>& origin) {
    const int B = (int)origin.size() / 2;
    std::vector<int> vol((size_t)S * volNX * volNY, 0), tab((size_t)S * volNX), rows((size_t)B * S * NX * NY, 0), pad((size_t)S * volNX * volNY, 0);
    for (size_t i = 0; i < tab.size(); ++i) tab[i] = (int)i;
    Visit fwd, adj;
    // k_window_stack / k_window_position_grad: rows (b, z, i), lanes j, taps (a, c)
    for (int b = 0; b < B; ++b) {
        const WinCell c = win_cell(origin.data(), b, NX, NY, volNX, volNY);
        CHECK(c.wx[0] >= 0.f && c.wx[0] <= 1.f && c.wx[1] >= 0.f && c.wx[1] <= 1.f && c.wy[0] >= 0.f && c.wy[1] <= 1.f, "window %d: factors", b);
        for (int z = 0; z < S; ++z)
            for (int i = 0; i < NX; ++i) {
                long long r[2];
                for (int a = 0; a < 2; ++a) {
                    const int xg = c.i0 + i + a;
                    r[a] = xg >= 0 && xg < volNX ? (long long)tab[(size_t)z * volNX + xg] : -1;
                }
                for (int j = 0; j < NY; ++j) {
                    for (int t = 0; t < 4; ++t) {
                        const int ta = t >> 1, tc = t & 1, y = c.j0 + j + tc;
                        if (r[ta] >= 0 && y >= 0 && y < volNY) {
                            vol[(size_t)r[ta] * volNY + y] += 1;                                   // the read
                            if (win_weight(c, ta, tc) != 0.f) fwd[{b, t, z, c.i0 + i + ta, y}] += 1;
                        }
                    }
                    rows[(((size_t)b * S + z) * NX + i) * NY + j] += 1;                            // the write
                }
            }
    }
    for (size_t i = 0; i < rows.size(); ++i) CHECK(rows[i] == 1, "window element %zu written %d times", i, rows[i]);
    // k_window_overlap_add_shifted: the list of column xg in ascending b, the (j0, b) sort, the run of a y, the taps
    int longest = 0;
    for (int xg = 0; xg < volNX; ++xg) {
        std::vector<int> ub, uy;
        for (int b = 0; b < B; ++b) {
            const WinCell c = win_cell(origin.data(), b, NX, NY, volNX, volNY);
            if (win_touches(c, xg, NX)) { ub.push_back(b); uy.push_back(c.j0); }
        }
        const int n = (int)ub.size();
        longest = std::max(longest, n);
        std::vector<int> lb((size_t)n, -1), ly((size_t)n), lx((size_t)n);
        for (int e = 0; e < n; ++e) {
            int rank = 0;
            for (int o = 0; o < n; ++o) rank += (uy[(size_t)o] < uy[(size_t)e]) || (uy[(size_t)o] == uy[(size_t)e] && ub[(size_t)o] < ub[(size_t)e]);
            CHECK(lb[(size_t)rank] == -1, "column %d: rank %d taken twice", xg, rank);
            lb[(size_t)rank] = ub[(size_t)e];
            ly[(size_t)rank] = uy[(size_t)e];
            lx[(size_t)rank] = xg - win_cell(origin.data(), ub[(size_t)e], NX, NY, volNX, volNY).i0;
        }
        for (int y = 0; y < volNY; ++y) {
            int lo, hi;
            {
                int l = 0, h = n;
                while (l < h) { const int mid = (l + h) >> 1; if (ly[(size_t)mid] >= y - NY) h = mid; else l = mid + 1; }
                lo = l;
                l = 0; h = n;
                while (l < h) { const int mid = (l + h) >> 1; if (ly[(size_t)mid] > y) h = mid; else l = mid + 1; }
                hi = l;
            }
            for (int z = 0; z < S; ++z) {
                for (int e = lo; e < hi; ++e) {
                    const int b = lb[(size_t)e];
                    const WinCell c = win_cell(origin.data(), b, NX, NY, volNX, volNY);
                    for (int t = 0; t < 4; ++t) {
                        const int ta = t >> 1, tc = t & 1;
                        const int i = lx[(size_t)e] - ta, j = y - ly[(size_t)e] - tc;
                        if (win_weight(c, ta, tc) != 0.f && i >= 0 && i < NX && j >= 0 && j < NY) {
                            rows[(((size_t)b * S + z) * NX + i) * NY + j] += 1;                    // the read
                            adj[{b, t, z, xg, y}] += 1;
                        }
                    }
                }
                pad[((size_t)z * volNX + xg) * volNY + y] += 1;                                    // the write
            }
            // entries outside [lo, hi) cannot reach y
            for (int e = 0; e < n; ++e)
                if (e < lo || e >= hi) CHECK(y - ly[(size_t)e] < 0 || y - ly[(size_t)e] - 1 >= NY, "column %d y %d: entry %d left out", xg, y, e);
        }
    }
    for (size_t i = 0; i < pad.size(); ++i) CHECK(pad[i] == 1, "frame element %zu written %d times", i, pad[i]);
    CHECK(fwd == adj, "the adjoint's visits are not the forward's (%zu against %zu)", adj.size(), fwd.size());
    for (const auto& kv : adj) CHECK(kv.second == 1, "a tap visited %d times", kv.second);
    const int counted = win_max_per_column(origin.data(), B, NX, NY, volNX, volNY);
    CHECK(counted == longest, "win_max_per_column %d, longest list %d", counted, longest);
}

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    int cases = 0;
    const int shapes[][5] = {{12, 3, 14, 8, 6}, {10, 2, 140, 6, 130}, {5, 3, 4, 4, 2}, {1, 1, 2, 1, 2}, {7, 2, 6, 9, 8}};
    for (const auto& s : shapes) {
        const int VX = s[0], VY = s[2], NX = s[3], NY = s[4];
        const std::vector<double> origin = {1.3, 2.7, 1.0, 2.0, -1.6, -0.35, VX - NX / 2. + 0.25, VY - NY / 2. - 0.5, VX + 3.5, 1.0,
                                            -(double)NX, 0.5, -(double)NX - 0.999, 0.0, (double)VX - 1e-9, (double)VY - 1e-9, -1e-9, -1e-9,
                                            1e300, -1e300, inf, -inf, nan, nan, 0.0, -(double)NY - 1.0, 2147483648.0, -2147483649.0};
        walk(VX, s[1], VY, NX, NY, origin);
        ++cases;
        // every fraction of a coarse lattice across the frame and beyond
        std::vector<double> sweep;
        for (double u = -NX - 2.5; u <= VX + 2.5; u += 0.75) { sweep.push_back(u); sweep.push_back(VY / 2. - u * 0.5); }
        walk(VX, s[1], VY, NX, NY, sweep);
        ++cases;
    }
    // the list's limit: 1025 windows at one origin are counted as 1025, with one moved off the frame as 1024
    std::vector<double> many((size_t)2 * 1025, 0.5);
    CHECK(win_max_per_column(many.data(), 1025, 4, 2, 5, 4) == 1025, "1025 windows on a column");
    many[14] = 7.0;
    CHECK(win_max_per_column(many.data(), 1025, 4, 2, 5, 4) == BDOF_WIN_MAXLIST_SHIFTED, "1024 windows on a column");
    CHECK(win_position_partials(3, 4) == 3 && win_position_partials(256, 72) == WIN_PG_MAX_PARTIALS && win_position_partials(1, 1) == 1, "records");
    std::printf("%s: %d walks, %d failure(s)\n", fails ? "FAILED" : "ok", cases, fails);
    return fails ? 1 : 0;
}
