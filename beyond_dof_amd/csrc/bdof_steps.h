// Slice binning (bdof_set_slice_binning): the host's index arithmetic between voxel slices and propagation steps, in one place
// and free of device code, so that a stand-alone host program can walk it under a sanitizer (tools/check_binning_index.cpp).
//   S voxel slices, bin per step, n = S / bin steps; step i covers the voxel slices i bin .. i bin + bin - 1.
// What exists once per step — tape slots, planes of a carrier-field stack, carrier scalars, dither copies — is indexed by the
// step; the modulation-table rows and the rotated-frame gradient [B][S][NX][NY] by the voxel slice.
#pragma once
#include <cstddef>

struct StepIndex {
    int S, bin;
    static bool valid(int S, int bin) { return S >= 1 && bin >= 1 && S % bin == 0; }      // (a shorter last bin is not carried)
    int n() const { return S / bin; }                                    // propagation steps
    int first_slice(int step) const { return step * bin; }              // of the step's bin: where its gradient rows start
    int slice(int step, int j) const { return step * bin + j; }         // j < bin
    // history tape: the transfer-function step after step z writes slot z (every step but the last); A_z and A'_z read slot z - 1
    int tape_read(int step) const { return step - 1; }                  // step > 0
    int tape_write(int step) const { return step; }
    std::size_t tape_fields() const { return (std::size_t)n(); }        // per wavefield
    std::size_t stack_planes() const { return (std::size_t)n(); }       // bdof_set_probe_stack / bdof_set_probe_field
    int steps_back(int step) const { return n() - 1 - step; }           // adjoint steps taken before A'_step runs
};
