// Host-side check of the slice-binning index arithmetic (beyond_dof_amd/csrc/bdof_steps.h) under a sanitizer: walks the forward
// sweep, the backward sweep, the carrier-field stack and bdof_tape_to_real's range exactly as bdof_capi.hip does, over buffers
// sized as bdof_set_slice_binning / bdof_set_probe_stack / bdof_configure size them (one element per field), and checks that
// every tape slot is written before it is read, that every voxel slice of the gradient is written exactly once, and that the
// steps of the adjoint carrier count down to zero.  An index outside its buffer is the sanitizer's to report.
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o check_binning_index tools/check_binning_index.cpp
//   ./check_binning_index          (exit code 0 and "ok" when every case passes)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../beyond_dof_amd/csrc/bdof_steps.h"

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

static void walk(int S, int bin, bool tf_all, int B) {
    const StepIndex ix{S, bin};
    const int n = ix.n();
    // exactly the sizes the library allocates, in fields / planes / slices
    std::vector<int> tape(ix.tape_fields(), 0);
    std::vector<int> stack(ix.stack_planes(), 0);
    std::vector<int> grot((size_t)B * S, 0);
    std::vector<int> mod_rows((size_t)B * S, 0);               // the no-table row formula (b S + slice): rows a step's bin reads

    // bdof_set_probe_field: one plane per step, a propagation between consecutive planes
    for (int z = 0; z < n; ++z) stack[(size_t)z] = 1;

    // forward_sweep (TAPE_HISTORY)
    for (int z = 0; z < n; ++z) {
        if (z > 0) CHECK(tape[(size_t)ix.tape_read(z)] == 1, "S %d bin %d: step %d reads tape slot %d before it is written", S, bin, z, ix.tape_read(z));
        CHECK(stack[(size_t)z] == 1, "S %d bin %d: carrier plane %d", S, bin, z);
        for (int b = 0; b < B; ++b)
            for (int j = 0; j < bin; ++j) mod_rows[(size_t)b * S + ix.slice(z, j)] += 1;
        const bool last = z == n - 1;
        if (!last) tape[(size_t)ix.tape_write(z)] = 1;         // the last step's transfer-function output (tf_all) goes to bufB, not the tape
        (void)tf_all;
    }
    for (size_t i = 0; i < mod_rows.size(); ++i) CHECK(mod_rows[i] == 1, "S %d bin %d: modulation row %zu read %d times", S, bin, i, mod_rows[i]);

    // backward sweep of bdof_loss_grad (history form) with the gradient rows of A'
    int expect_back = 0;
    for (int z = n - 1; z >= 0; --z) {
        CHECK(ix.steps_back(z) == expect_back, "S %d bin %d: step %d is %d adjoint steps back, not %d", S, bin, z, ix.steps_back(z), expect_back);
        if (z > 0) CHECK(tape[(size_t)ix.tape_read(z)] == 1, "S %d bin %d: A'_%d reads an unwritten slot", S, bin, z);
        for (int b = 0; b < B; ++b)
            for (int j = 0; j < bin; ++j) grot[((size_t)b * S + ix.first_slice(z)) + j] += 1;       // grot_z + j, as the kernel strides
        ++expect_back;
    }
    for (size_t i = 0; i < grot.size(); ++i) CHECK(grot[i] == 1, "S %d bin %d: gradient slice %zu written %d times", S, bin, i, grot[i]);

    // bdof_tape_to_real: i < n - 1 reads slot i, carrier plane i + 1; i == n - 1 the kept last wave, plane n - 1
    for (int i = 0; i < n; ++i) {
        if (i < n - 1) {
            CHECK(tape[(size_t)i] == 1, "S %d bin %d: history slot %d", S, bin, i);
            CHECK(stack[(size_t)i + 1] == 1, "S %d bin %d: plane %d", S, bin, i + 1);
        } else {
            CHECK(stack[(size_t)n - 1] == 1, "S %d bin %d: last plane", S, bin);
        }
    }
}

int main() {
    int cases = 0;
    for (int S = 1; S <= 24; ++S)
        for (int bin = 1; bin <= S + 1; ++bin) {
            const bool ok = StepIndex::valid(S, bin);
            CHECK(ok == (S % bin == 0), "valid(%d, %d)", S, bin);
            if (!ok) continue;
            for (int tf_all = 0; tf_all < 2; ++tf_all) { walk(S, bin, tf_all != 0, 3); ++cases; }
        }
    CHECK(!StepIndex::valid(6, 0) && !StepIndex::valid(6, -2) && !StepIndex::valid(0, 1) && !StepIndex::valid(6, 4), "refused arguments");
    walk(512, 1, false, 2); walk(512, 2, false, 2); walk(512, 4, true, 2); walk(512, 512, true, 2);
    cases += 4;
    std::printf("%s: %d sweeps walked, %d failure(s)\n", fails ? "FAILED" : "ok", cases, fails);
    return fails ? 1 : 0;
}
