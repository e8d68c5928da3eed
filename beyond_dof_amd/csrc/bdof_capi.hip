// libbdof.so — host side of the C ABI declared in include/bdof.h.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <cmath>
#include <algorithm>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/bdof.h"
#include "bdof_steps.h"
#include "bdof_kernels.h"
#include "bdof_conv2.h"
#include "bdof_generic.h"
#include "bdof_field.h"
#include "bdof_conv64.h"
#include "bdof_resident.h"
#include "bdof_modes.h"
#include "bdof_comm.h"
#include "bdof_rigid.h"
#include "bdof_windows.h"
#include "bdof_shells.h"
#include "bdof_fbp.h"
#include <rocfft/rocfft.h>
#include <map>
#include <optional>
#include <functional>
#include <array>

#define BDOF_ERR_ARG (-1)
#define BDOF_ERR_STATE (-2)
#define BDOF_ERR_SIZE (-3)

#define BDOF_MAX_GROUPS 4
#define BDOF_N_TIMERS 16
#define BDOF_MAX_DEVICES 64
// ---- ownership: a member's type says who releases it ------------------------------------------------------------------------
// device memory that its holder owns: n elements of T, released when the holder goes
template <typename T>
class DevBuf {
    T* p_ = nullptr;
    size_t n_ = 0;
public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept { *this = std::move(o); }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p_, o.p_); std::swap(n_, o.n_); return *this; }     // o releases what this held
    ~DevBuf() { reset(); }
    void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; n_ = 0; }
    // what is held goes BEFORE its replacement is allocated: the large buffers do not fit twice
    hipError_t alloc(size_t n) {
        reset();
        const hipError_t e = hipMalloc((void**)&p_, n * sizeof(T));
        if (e == hipSuccess) n_ = n; else p_ = nullptr;
        return e;
    }
    hipError_t room(size_t n) { return n_ >= n ? hipSuccess : alloc(n); }      // grow only
    size_t size() const { return n_; }
    explicit operator bool() const { return p_ != nullptr; }
    operator T*() const { return p_; }
};

// the forward and the inverse rocFFT plan of one (shape, batch, precision)
struct PlanPair {
    rocfft_plan fwd = nullptr, inv = nullptr;
    PlanPair() = default;
    PlanPair(PlanPair&& o) noexcept : fwd(o.fwd), inv(o.inv) { o.fwd = o.inv = nullptr; }
    ~PlanPair() {
        if (fwd) (void)rocfft_plan_destroy(fwd);
        if (inv) (void)rocfft_plan_destroy(inv);
    }
};

// what rocFFT executes with on one stream: the execution info and the work area bound to it (fft_exec_room)
struct FftExec {
    rocfft_execution_info info = nullptr;
    DevBuf<char> work;
    FftExec() = default;
    FftExec(FftExec&& o) noexcept { *this = std::move(o); }
    FftExec& operator=(FftExec&& o) noexcept { std::swap(info, o.info); work = std::move(o.work); return *this; }
    ~FftExec() { if (info) (void)rocfft_execution_info_destroy(info); }
};

// Everything bdof_configure sizes, with the flags that say what the buffers hold: a re-configure assigns a fresh Workspace, so a
// member placed here is released and reset by its type.  Members of bdof_ctx itself survive a re-configure.
struct Workspace {
    DevBuf<cf> twY, twX;
    DevBuf<cf> hs, hdet, hcomb, probe;
    // float64 real-space propagator (bdof_set_conv_f64 / bdof_loss_grad_conv_f64, bdof_conv64.h)
    DevBuf<double2> c64_probe, c64_khat, c64_psi, c64_q, c64_big, c64_tape, c64_scal, c64_part;
    int c64_ks = 0, c64_B = 0;
    DevBuf<double2> c64_h, c64_hdet;             // the transfer-function model of the float64 path (bdof_set_tf_f64)
    DevBuf<cf> hsT_d;              // the same copies in the LDS-resident kernel's [kx][ky] order
    DevBuf<cf> hs_d;               // bdof_set_transfer_f64: hs_copies dithered float32 copies of the slice step's table (bdof_field.h)
    int hs_copies = 0;
    // Fused forward sweep (bdof_set_sweep_fusion; k_slice_y / k_slice_x): the separable factors of the slice step, hy[ky] hx[kx] =
    // the table above, in sep_copies dithered float32 copies each ([copy][k]; 0: the table is not separable, or there is no float64
    // table to take them from), and the [NY][NX] table whose every row is hx of step S-2 (the hand-over to the unfused last slice)
    DevBuf<cf> hx_d, hy_d, hx_rows;
    int sep_copies = 0;
    DevBuf<cf> bufA, bufB, tape;
    int bin = 1;                   // bdof_set_slice_binning: voxel slices per propagation step (1 after every bdof_configure)
    DevBuf<float2> grot;
    DevBuf<double2> gcar, gt0;                   // adjoint carrier per wavefield (AdjCarrier, bdof_kernels.h)
    DevBuf<cf> gpsi0;                            // [Bmax][NX][NY] G(psi_0) per wavefield (bdof_enable_probe_grad)
    const cf* gpsi_src = nullptr;                // borrowed from this workspace: where the last bdof_loss_grad left it (gpsi0, or the generic engine's field)
    DevBuf<double> partial, loss_dev;
    DevBuf<float> wgt;                           // [NX][NY] detector weights in the order of one wavefield of meas; none: no weights (bdof_set_detector_weights)
    // Detector planes (bdof_set_detector_planes): D > 1 near-field planes behind the exit wave; 1 (after every bdof_configure and
    // bdof_set_physics): the one plane of bdof_set_physics, on bufA / bufB alone
    int planes = 1;
    DevBuf<cf> hdet_pl, hcomb_pl;                // [D][ky][kx] tables of the planes: the detector step's, and under tf_all combined with the slice step's
    std::vector<std::complex<double>> hdet00_pl; // [D] their DC values
    // the 2 D detector / seed fields per wavefield.  Streaming engine: [Bmax][D][NX][NY] each, det_pl the detector fields in L1
    // order and seed_pl the seeds in L2 order.  Generic engine: det_pl alone, [D][Bmax][NX][NY] real-space fields.
    DevBuf<cf> det_pl, seed_pl;
    // real-space truncated-kernel propagator (bdof_set_conv)
    bool have_conv = false;
    DevBuf<ConvTaps> taps_dev;
    int taps_copies = 1;          // dithered copies of the taps in taps_dev (bdof_set_conv_taps_f64), slice z takes copy z mod taps_copies
    DevBuf<cf> bufC, conv_scal;
    // carrier field of the real-space propagator (bdof_set_conv_probe_stack): p_0 .. p_S, float32 planes [S + 1][NX][NY]; the
    // detector plane of p_S in float64; corner pixels of p_0 and p_S (the renormalisation s = p_0[0,0] / psi_S[0,0,0])
    DevBuf<cf> cstack;
    DevBuf<double2> cdet64;
    // LDS-resident engine (small square fields, bdof_resident.h)
    bool resident = false;
    DevBuf<cf> hsT, hdetT, twR, res_carrier;
    DevBuf<cf> pstack, pdet, pdetT;              // carrier field of a localised probe (bdof_set_probe_stack); pdetT = det transposed
    DevBuf<double2> pdet64, pdetT64;             // the same planes in float64 (bdof_set_probe_field): the residual |d| - m is formed in float64
    // Probe modes (bdof_set_probe_modes; bdof_modes.h): M > 0 carrier fields, built as bdof_set_probe_field builds its one, mode m
    // at plane m of each buffer: the [M][steps][NX][NY] stacks and the [M][NX][NY] float64 detector planes, [x][y] (far field
    // [kx][ky]) — what the sweeps and k_modes_couple read; the float32 and the transposed detector planes of the single probe have
    // no reader under modes and are not built.  0: no modes, the probe of bdof_set_probe*
    int n_modes = 0;
    DevBuf<cf> m_stack;
    DevBuf<double2> m_det64;
    DevBuf<cf> m_zero;                           // zeros, max(NX NY, 2 S): the modes' eps_0 and their scalar carriers
    // rocFFT (generic-size engine, float64 paths, whole-field steps): one plan pair per (NX, NY, B, double)
    std::map<std::array<int, 4>, PlanPair> plans;
    // bdof_shell_correlation (bdof_shells.h): the forward double-precision plan of a whole volume per (NX, NZ, NY), the complex128
    // copies of the two volumes and the per-workgroup shell tables with their sum behind them — taken at first use
    std::map<std::array<int, 3>, PlanPair> vol_plans;
    DevBuf<double2> shell_a, shell_b;
    DevBuf<double> shell_part;
    DevBuf<double2> fbp_work;                    // bdof_ctf_retrieve (bdof_fbp.h): [D][B][NX][NY] complex128 contrast planes, grown on demand
    FftExec fft;                                 // of the ctx's stream
    // float64 adjoint sweep (BDOF_CFG_ADJOINT64; generic engine)
    bool have_h64 = false;
    DevBuf<double2> g64, hs64, hdet64;
};

struct bdof_ctx : Workspace {
    int device = 0;
    hipStream_t stream = nullptr;               // borrowed from the caller unless own_stream
    bool own_stream = false;
    // split of a batch over streams (Split)
    hipStream_t side[BDOF_MAX_GROUPS - 1] = {};   // side streams PROVEN to run concurrently with the ctx stream (probe_side_streams)
    int n_side = -1;                             // -1: not probed yet
    std::vector<hipStream_t> side_all;           // every candidate created (kept until the ctx dies)
    hipEvent_t ev_fork = nullptr, ev_join[BDOF_MAX_GROUPS - 1] = {};
    hipEvent_t timer[BDOF_N_TIMERS] = {};        // bdof_timer_mark
    int n_streams = -1;                          // -1 auto (1 or 2), else the number of groups to split a batch in
    int fusion = 0;                              // bdof_set_sweep_fusion: 0 never (a new ctx), 1 the forward sweep where the configuration is eligible
    int fused_last = 0;                          // what the last bdof_loss_grad ran (bdof_sweep_fused)
    int adj_fusion = 0;                          // bdof_set_adjoint_fusion: the fused adjoint sweep wherever the fused forward sweep runs
    int adj_fused_last = 0;                      // what the last bdof_loss_grad ran (bdof_adjoint_fused)
    int ncu = 256;
    int NY = 0, NX = 0, S = 0, Bmax = 0;
    bool with_grad = false;
    bool recompute = false;                      // tape-free adjoint (BDOF_CFG_RECOMPUTE): the tape holds 3 fields, not S
    // dithered twiddle tables (bdof_fft.h; BDOF_TW_DITHER=D, default 64): D copies of each table, entry j of copy d rounded up or
    // down so that the mean over the D copies is the float64 value to ulp / D; the launches of slice z take copy z mod D
    int tw_dither = 0;
    // borrowed: the caller's memory, which the caller keeps alive and releases (with the caller's stream above, and gpsi_src,
    // which points into the Workspace and is reset with it)
    const float2* obj_src = nullptr;            // caller's (delta, beta) rows
    const int *adj_off = nullptr, *adj_order = nullptr;
    const cf* range_car = nullptr;              // bdof_set_range_carrier: [nz][B][NX][NY] carrier fields of the range being swept
    int range_car_B = 0, range_car_z0 = 0;
    DevBuf<double2> car_scratch;                // bdof_range_carrier_build: [nz - 1][B][NX][NY] complex128
    hipStream_t aux = nullptr;                  // bdof_fields_free_step_aux: the whole-field step of a stitch range beside the tiles' sweeps
    hipEvent_t ev_aux_fork = nullptr, ev_aux_join = nullptr;
    FftExec fft_aux;
    bool aux_pending = false;
    bool c64_tf = false;                        // the float64 path holds the transfer-function model (bdof_set_tf_f64), not the real-space one
    std::complex<double> c64_ksum{1.0, 0.0};
    double c64_k = 0.0;
    int gpsi_B = 0;
    int npartial = 0;
    float k = 0.f;                              // the k the modulation table in c->mod was built with
    float k_fft = 0.f;                          // bdof_set_physics' k (the reference's PI literal, quirk Q1)
    std::complex<double> h00{1.0, 0.0}, hdet00{1.0, 0.0}, a0{0.0, 0.0};   // carrier splitting (bdof_kernels.h)
    std::complex<double> cbm1{0.0, 0.0};        // cbar - 1: mean modulation factor of the object minus one (modulate_eps_s)
    DevBuf<double2> cbar_dev;                   // [ncu * 16 + 1] per-workgroup sums of the modulation table, then the mean
    ConvTaps taps{};                            // bdof_set_conv
    std::complex<double> ksum{1.0, 0.0};
    float k_conv = 0.f;
    std::complex<double> c_p0{0.0, 0.0}, c_pS{0.0, 0.0};   // bdof_set_conv_probe_stack
    bool res_dirty = true, res_always = false;
    int meas_dev = 0;                           // bdof_set_meas_mode
    int loss_kind = BDOF_LOSS_LSQ;              // bdof_set_loss: the data term of bdof_loss_grad / bdof_loss_grad_tf_f64 ...
    double loss_mu = 0.0;                       // ... and, for BDOF_LOSS_POISSON, its photons per unit intensity
    bool generic = false;                       // generic-size engine (rocFFT)
    bool adj64 = false;                         // float64 adjoint sweep (BDOF_CFG_ADJOINT64; generic engine)
    int det_mode = BDOF_DET_NONE, variant = BDOF_VARIANT_NUMPY_SKIP_LAST;
    bool have_physics = false, have_probe = false, tape_valid = false, last_valid = false;
    ObjView obj{};
    bool obj_bound_mod = false;                 // bdof_set_object_bilinear: c->mod was written directly, there is no obj_src
    size_t obj_rows = 0;
    DevBuf<float2> mod;                         // c - 1 table of those rows (k_modulation_table)
    bool mod_dirty = true;
    // bdof_rotation_adjoint_adam left the table of ANOTHER volume (its x_new) in c->mod, with the row sums of the factors in
    // cbar_dev[0, mod_for_rows) and their mean at cbar_dev[mod_for_mean_at]: the next bdof_set_object takes the table over if it binds exactly
    // that volume (the record is good for that one call; everything that writes c->mod or cbar_dev drops it)
    const float2* mod_for = nullptr;
    size_t mod_for_rows = 0;
    int mod_for_NY = 0;
    bool mod_for_mean = false;                  // want_cbar when the table was written
    size_t mod_for_mean_at = 0;                 // where in cbar_dev the mean is
    bool mod_mean_pending = false;              // the table was taken over: its mean is still on the device (ensure_modulation)
    int n_angles = 0;
    int adj_ndest = 0;
    DevBuf<float2> winpad;                      // [S][volNX][volNY] rotated-frame gradient of the ptychography windows
    DevBuf<int> win_angle;                      // device copy of the batch's angle index
    DevBuf<int> heavy;                          // [1 + n_dest]: counter + deferred rows of the rotation adjoint
    DevBuf<double> prm_partial;                 // [B][P][12] per-workgroup records of bdof_rotate_rigid_param_grad (grown on demand)
    int win_volNX = 0, win_volNY = 0;           // the rotated frame of the last bdof_window_stack: what bdof_window_stack_adjoint scatters into
    // profiling
    bool prof = false;
    int prof_stride = 1;                        // time every prof_stride-th launch of a class
    unsigned prof_seen[BDOF_K_COUNT] = {0};
    std::vector<hipEvent_t> ev_pool;
    std::vector<std::pair<int, int>> ev_used;   // (class, index of start event)
    size_t ev_next = 0;
    double prof_ms[BDOF_K_COUNT] = {0};
    int prof_n[BDOF_K_COUNT] = {0};
    std::string err;
};

static int fail(bdof_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}

#define HIPC(c, call)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            return fail((c), (int)e_, std::string(#call) + ": " + hipGetErrorString(e_));          \
        }                                                                                          \
    } while (0)

// ---- argument checks shared by the entry points (0 = passed, else the code of the failure) -------------------------------------
// the status of the launches just queued
static int launched(bdof_ctx* c) {
    HIPC(c, hipGetLastError());
    return 0;
}
static int need_configured(bdof_ctx* c) {
    return c->NY ? 0 : fail(c, BDOF_ERR_STATE, "bdof_configure has not been called");
}
static int need_angles(bdof_ctx* c, const int* angle_of_b) {
    return c->obj.tab && !angle_of_b ? fail(c, BDOF_ERR_ARG, "angle_of_b required with a rotation table") : 0;
}
static int check_batch(bdof_ctx* c, int B) {
    return B < 1 || B > c->Bmax ? fail(c, BDOF_ERR_ARG, "batch size outside [1, Bmax]") : 0;
}
static int check_range(bdof_ctx* c, int z0, int nz) {
    return z0 < 0 || nz < 1 || z0 + nz > c->S ? fail(c, BDOF_ERR_ARG, "slice range outside [0, S)") : 0;
}
// ---- the model's options: which entry point carries which ----------------------------------------------------------------------
// An option is in force on a ctx (`on`) or not; an entry point states the options it carries and admit() refuses it under any
// other one that is in force, in the order of the table.  bdof_loss_grad, bdof_forward and the rest of the main path carry all
// five and make no call.
enum { CARRIES_NOTHING = 0, CARRIES_BINNING = 1, CARRIES_PLANES = 2, CARRIES_POISSON = 4, CARRIES_WEIGHTS = 8, CARRIES_MODES = 16,
       NO_DATA_TERM = CARRIES_POISSON | CARRIES_WEIGHTS };       // an entry point that computes no loss: the data term's options pass
struct ModelOption { int bit; bool (*on)(const bdof_ctx*); const char* refusal; };       // (the refusal follows the caller's name)
static const ModelOption MODEL_OPTIONS[] = {
    {CARRIES_BINNING, [](const bdof_ctx* c) { return c->bin > 1; }, " does not carry slice binning: it would run the unbinned model (bdof_set_slice_binning)"},
    {CARRIES_PLANES, [](const bdof_ctx* c) { return c->planes > 1; }, " does not carry detector planes: bdof_set_detector_planes(ctx, 1, NULL, NULL) first"},
    {CARRIES_POISSON, [](const bdof_ctx* c) { return c->loss_kind != BDOF_LOSS_LSQ; }, " computes the least-squares loss only: bdof_set_loss(BDOF_LOSS_LSQ) first"},
    {CARRIES_WEIGHTS, [](const bdof_ctx* c) { return (bool)c->wgt; }, " does not carry detector weights: bdof_set_detector_weights(ctx, NULL) first"},
    {CARRIES_MODES, [](const bdof_ctx* c) { return c->n_modes > 0; }, " does not carry probe modes: bdof_set_probe_modes(ctx, 0, NULL, NULL, NULL) first"},
};
// (no ctx: passes, and the entry point's own argument check answers)
static int admit(bdof_ctx* c, const char* who, int carries) {
    if (!c) return 0;
    for (const ModelOption& o : MODEL_OPTIONS)
        if (!(carries & o.bit) && o.on(c)) return fail(c, BDOF_ERR_STATE, std::string(who) + o.refusal);
    return 0;
}

// The reverse direction: the modes of a ctx that an option can collide with.  A setter names the ones that do not carry its
// option, in the order it reports them.
struct CtxMode { bool (*on)(const bdof_ctx*); const char* name; };
static const CtxMode MODE_RESIDENT = {[](const bdof_ctx* c) { return c->res_always; }, "the LDS-resident engine (BDOF_CFG_ALWAYS_RESIDENT)"};
static const CtxMode MODE_RECOMPUTE = {[](const bdof_ctx* c) { return c->recompute; }, "the tape-free adjoint (BDOF_CFG_RECOMPUTE)"};
static const CtxMode MODE_ADJOINT64 = {[](const bdof_ctx* c) { return c->adj64; }, "the float64 adjoint sweep (BDOF_CFG_ADJOINT64)"};
static const CtxMode MODE_NO_GROT = {[](const bdof_ctx* c) { return c->with_grad && !c->grot; }, "a ctx without the gradient workspace (BDOF_CFG_NO_GROT)"};
static const CtxMode MODE_NOT_NEAR = {[](const bdof_ctx* c) { return c->det_mode != BDOF_DET_NEAR; }, "a detector mode other than BDOF_DET_NEAR"};
static const CtxMode MODE_CONV = {[](const bdof_ctx* c) { return c->have_conv; }, "the real-space propagator (bdof_set_conv)"};
static const CtxMode MODE_CARRIER_FIELD = {[](const bdof_ctx* c) { return (bool)c->pstack; }, "a carrier field (bdof_set_probe_stack / bdof_set_probe_field)"};
static const CtxMode MODE_RANGE_CARRIER = {[](const bdof_ctx* c) { return c->range_car != nullptr; }, "range carriers (bdof_set_range_carrier)"};
static const CtxMode MODE_STREAMING_ONLY = {[](const bdof_ctx* c) { return !c->resident && !c->generic; }, "a ctx whose only engine is the streaming one"};
static const CtxMode MODE_PROBE_MODES = {[](const bdof_ctx* c) { return c->n_modes > 0; }, "probe modes (bdof_set_probe_modes)"};
// "<setter>: <mode> does not carry <option>" for the first of `refused` that is on
static int refuse_modes(bdof_ctx* c, const char* setter, const char* option, std::initializer_list<const CtxMode*> refused) {
    for (const CtxMode* m : refused)
        if (m->on(c)) return fail(c, BDOF_ERR_STATE, std::string(setter) + ": " + m->name + " does not carry " + option);
    return 0;
}
// back to the one plane of bdof_set_physics: tables and the planes' fields go
static void drop_planes(bdof_ctx* c) {
    c->planes = 1;
    c->hdet_pl.reset(); c->hcomb_pl.reset(); c->det_pl.reset(); c->seed_pl.reset();
    c->hdet00_pl.clear();
}
// back to the probe of bdof_set_probe*: the modes' carrier fields go
static void drop_modes(bdof_ctx* c) {
    c->n_modes = 0;
    c->m_stack.reset(); c->m_det64.reset(); c->m_zero.reset();
}

// ---- what a change voids ---------------------------------------------------------------------------------------------------
// State the ctx derives from what it is handed, by the flag that says whether it still holds ...
enum { V_TWIN64 = 1,        // c64_tf, c64_ks: the float64 twin handed over (bdof_set_tf_f64 / bdof_set_conv_f64) held the previous model
       V_RESIDENT = 2,      // res_dirty: the resident engine's carrier constants (resident_run uploads them again)
       V_MODULATION = 4,    // mod_dirty, mod_mean_pending: the table c - 1 in c->mod and its mean (ensure_modulation rebuilds them)
       V_MOD_RECORD = 8,    // mod_for: the table bdof_rotation_adjoint_adam left for another volume
       V_HISTORY = 16,      // tape_valid: the per-slice history of bdof_forward(keep_tape)
       V_LAST_WAVE = 32,    // last_valid: ... and its last slice's wave in bufA
       V_COPIES = 64,       // hs_copies, sep_copies: dithered copies of the slice step and of its separable factors (bdof_set_transfer_f64 follows)
       V_H64 = 128,         // have_h64: the float64 adjoint's tables (bdof_set_physics_f64 follows)
       V_PLANES = 256,      // planes: detector planes belong to the physics that go (drop_planes; bdof_set_detector_planes follows)
       V_GPSI = 512,        // gpsi_src: where the last bdof_loss_grad left G(psi_0)
       V_MODES = 1024 };    // n_modes: probe modes were propagated with the physics that go (drop_modes; bdof_set_probe_modes follows)
// ... and the one statement of which cause voids what (DESIGN §4 has the same table).  No setter or entry point assigns these
// flags itself.  It records what the code did when it was written down, uneven places included (MEASUREMENTS.md lists them).
enum Cause { CHANGED_CONFIGURATION, CHANGED_BINNING, CHANGED_PHYSICS, CHANGED_SLICE_STEP_F64, CHANGED_PROBE, CHANGED_CARRIER_FIELD,
             CHANGED_CARRIER_FIELD_F64, CHANGED_CONV_TAPS, CHANGED_CONV_CARRIER_FIELD, CHANGED_OBJECT, CHANGED_DETECTOR_PLANES,
             CHANGED_MODULATION_K, CHANGED_MOD_OVERWRITTEN, CHANGED_MEAN_MODULATION, TAPE_OVERWRITTEN, PROBE_GRADIENT_GONE, CHANGED_PROBE_MODES };
static const struct { Cause cause; int voids; } VOIDS[] = {
    {CHANGED_CONFIGURATION, V_RESIDENT | V_HISTORY},             // bdof_configure (beside the fresh Workspace, which resets what it holds)
    {CHANGED_BINNING, V_MODULATION | V_RESIDENT | V_HISTORY | V_LAST_WAVE},                     // bdof_set_slice_binning
    {CHANGED_PHYSICS, V_TWIN64 | V_PLANES | V_MODES | V_RESIDENT | V_H64 | V_COPIES | V_MODULATION},      // bdof_set_physics
    {CHANGED_SLICE_STEP_F64, V_COPIES | V_RESIDENT},             // bdof_set_transfer_f64: the previous table's copies go before the new ones come
    {CHANGED_PROBE, V_TWIN64 | V_RESIDENT | V_MODULATION},       // bdof_set_probe: whether the mean modulation rides on the carrier depends on a0 (want_cbar)
    {CHANGED_CARRIER_FIELD, V_MODULATION},                       // bdof_set_probe_stack, set or cleared
    {CHANGED_CARRIER_FIELD_F64, V_RESIDENT | V_MODULATION},      // bdof_set_probe_field: a carrier field that also zeroes the probe and a0
    {CHANGED_CONV_TAPS, V_TWIN64 | V_MODULATION},                // bdof_set_conv
    {CHANGED_CONV_CARRIER_FIELD, 0},                             // bdof_set_conv_probe_stack: the sweeps read the stack itself, nothing derived is kept
    {CHANGED_OBJECT, V_MODULATION | V_MOD_RECORD},               // bdof_set_object, bdof_set_object_bilinear — see changed()
    {CHANGED_DETECTOR_PLANES, V_PLANES | V_HISTORY | V_LAST_WAVE},      // bdof_set_detector_planes with D > 1 tables
    {CHANGED_MODULATION_K, V_MODULATION},                        // the table was built with another k, or with the mean riding differently
    {CHANGED_MOD_OVERWRITTEN, V_MODULATION | V_MOD_RECORD},      // c->mod or cbar_dev is being written for something else than the bound object
    {CHANGED_MEAN_MODULATION, V_RESIDENT},                       // cbar came out different: the carrier scalars move
    {TAPE_OVERWRITTEN, V_HISTORY | V_LAST_WAVE},                 // a sweep has overwritten the tape
    {PROBE_GRADIENT_GONE, V_GPSI},                               // a sweep that leaves no G(psi_0), or its buffer went
    {CHANGED_PROBE_MODES, V_MODES | V_HISTORY | V_LAST_WAVE | V_GPSI},      // bdof_set_probe_modes, set or removed (bdof_configure: the fresh Workspace)
};
static void changed(bdof_ctx* c, Cause cause) {
    int v = 0;
    for (const auto& row : VOIDS) if (row.cause == cause) v = row.voids;
    // a new binding of the volume bdof_rotation_adjoint_adam has just left the table of: nothing to rebuild, its mean to fetch
    const bool taken_over = cause == CHANGED_OBJECT && c->mod_for && c->obj_src == c->mod_for && c->obj_rows == c->mod_for_rows && c->obj.volNY == c->mod_for_NY;
    if (v & V_TWIN64) { c->c64_tf = false; c->c64_ks = 0; }
    if (v & V_RESIDENT) c->res_dirty = true;
    if (v & V_MODULATION) { c->mod_dirty = !taken_over; c->mod_mean_pending = taken_over; }
    if (v & V_MOD_RECORD) c->mod_for = nullptr;
    if (v & V_HISTORY) c->tape_valid = false;
    if (v & V_LAST_WAVE) c->last_valid = false;
    if (v & V_COPIES) c->hs_copies = c->sep_copies = 0;
    if (v & V_H64) c->have_h64 = false;
    if (v & V_PLANES) drop_planes(c);
    if (v & V_GPSI) c->gpsi_src = nullptr;
    if (v & V_MODES) drop_modes(c);
}
// what makes it good again: the tape after bdof_forward(keep_tape), the table in c->mod, the resident engine's constants, a twin handed over
static void tape_holds(bdof_ctx* c, bool history, bool last) { c->tape_valid = history; c->last_valid = last; }
static void modulation_current(bdof_ctx* c) { c->mod_dirty = false; c->mod_mean_pending = false; }
static void resident_current(bdof_ctx* c) { c->res_dirty = false; }
static void twin64_holds(bdof_ctx* c, bool tf, int ks) { c->c64_tf = tf; c->c64_ks = ks; }

// ---- the setters' opening and their uploads ----------------------------------------------------------------------------------
// Every setter opens in one order: a ctx, a configuration, the ctx's device (a process may hold ctxs on several), and — drain —
// the ctx stream drained, because launches in flight may still read what the setter is about to free or overwrite.
static int enter_setter(bdof_ctx* c, bool drain) {
    if (!c) return BDOF_ERR_ARG;
    if (int r = need_configured(c)) return r;
    HIPC(c, hipSetDevice(c->device));
    if (drain) HIPC(c, hipStreamSynchronize(c->stream));
    return 0;
}
// n elements of a host table into buf, which is allocated FRESH (what it held goes first: DevBuf::alloc), only GROWn, or KEPT
// where it holds something already.  A blocking copy: the host table may go when this returns.
enum Room { FRESH, GROW, KEEP };
template <class T> static int upload(bdof_ctx* c, DevBuf<T>& buf, const void* host, size_t n, Room room) {
    if (room == FRESH || (room == KEEP && !buf)) HIPC(c, buf.alloc(n));
    else if (room == GROW) HIPC(c, buf.room(n));
    HIPC(c, hipMemcpy(buf, host, n * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}
// an interleaved complex table [rows][cols] as [cols][rows]
template <class T> static std::vector<T> transposed(const T* t, int rows, int cols) {
    std::vector<T> out((size_t)2 * rows * cols);
    for (int i = 0; i < rows; ++i)
        for (int j = 0; j < cols; ++j) {
            out[2 * ((size_t)j * rows + i)] = t[2 * ((size_t)i * cols + j)];
            out[2 * ((size_t)j * rows + i) + 1] = t[2 * ((size_t)i * cols + j) + 1];
        }
    return out;
}
// tf_all + near detector: the two consecutive steps F^-1 hdet_j F F^-1 hs F collapse into one with the table hs hdet_j n, formed
// in double and rounded once; D tables [D][n] of the detector steps, n = NX NY (the transforms' 1 / n sits in both factors)
static std::vector<float> combined(const float* hs, const float* hs_det, size_t n, int D) {
    std::vector<float> comb(2 * n * D);
    const double nn = (double)n;
    for (int j = 0; j < D; ++j)
        for (size_t i = 0; i < n; ++i) {
            const double ar = hs[2 * i], ai = hs[2 * i + 1], br = hs_det[2 * (j * n + i)], bi = hs_det[2 * (j * n + i) + 1];
            comb[2 * (j * n + i)] = (float)((ar * br - ai * bi) * nn);
            comb[2 * (j * n + i) + 1] = (float)((ar * bi + ai * br) * nn);
        }
    return comb;
}
// propagation steps of a sweep: the voxel depth over the slice binning
static StepIndex steps(const bdof_ctx* c) { return StepIndex{c->S, c->bin}; }
static int n_steps(const bdof_ctx* c) { return steps(c).n(); }
static bool loss_is_poisson(const bdof_ctx* c) { return c->loss_kind == BDOF_LOSS_POISSON; }
static int check_taper(bdof_ctx* c, int TX, int TY, int taper) {
    return taper < 0 || 2 * taper > TX || 2 * taper > TY ? fail(c, BDOF_ERR_ARG, "taper must fit the tile") : 0;
}
static int check_halo(bdof_ctx* c, int TX, int TY, int halo_x, int halo_y) {
    return halo_x < 0 || halo_y < 0 || 2 * halo_x >= TX || 2 * halo_y >= TY ? fail(c, BDOF_ERR_ARG, "halo must leave a core") : 0;
}

// A sub-batch: wavefields b0 .. b0 + B - 1 of the call's batch, launched on stream st.  Every launcher of the streaming and conv
// engines takes the sub-batch it works on; the ctx's buffers hold the whole batch and the launchers offset into them.
struct Group { int b0, B; hipStream_t st; };
// the whole batch on the ctx stream: the launches that run without a split, or after its join
static Group whole(const bdof_ctx* c, int B) { return Group{0, B, c->stream}; }

// Mean-refraction carrier (modulate_eps_s): constant part of the wave entering slice z, a_z = a_0 (cbar H00)^z
// (H00 = DC value of the transfer function, cbar = mean modulation factor of the object).  With slice binning z counts
// propagation steps, cbar is that of a bin (modulation_done) and H00 that of the bin's step.
static std::complex<double> carrier_z(const bdof_ctx* c, int z) { return c->a0 * std::pow((1.0 + c->cbm1) * c->h00, z); }
static cf cfl(std::complex<double> a) { return make_float2((float)a.real(), (float)a.imag()); }
static cf carrier_at(const bdof_ctx* c, int z) { return cfl(carrier_z(c, z)); }
static cf cshift_at(const bdof_ctx* c, int z) { return cfl(carrier_z(c, z) * c->cbm1); }                  // a_z (cbar - 1)
static cf carrier_phi_at(const bdof_ctx* c, int z) { return cfl(carrier_z(c, z) * (1.0 + c->cbm1)); }      // constant part of phi_z
// a transfer-function step follows the last slice: variant tf_all, except in front of a far-field detector
// (|F P phi| = |H F phi| = |F phi|)
static bool step_after_last(const bdof_ctx* c) { return c->variant == BDOF_VARIANT_TF_ALL && c->det_mode != BDOF_DET_FAR; }
// constant part of the detector wave (real-space detectors) / of the wave whose fft2 is the far field
// plane: which of the detector planes (bdof_set_detector_planes; 0 with one plane)
static std::complex<double> carrier_end(const bdof_ctx* c, int plane = 0) {
    std::complex<double> a = carrier_z(c, n_steps(c) - 1) * (1.0 + c->cbm1);
    if (step_after_last(c)) a *= c->h00;
    if (c->det_mode == BDOF_DET_NEAR) a *= c->planes > 1 ? c->hdet00_pl[plane] : c->hdet00;
    return a;
}
static std::complex<double> carrier_det(const bdof_ctx* c, int plane = 0) {
    std::complex<double> a = carrier_end(c, plane);
    if (c->det_mode == BDOF_DET_FAR) a *= (double)c->NX * (double)c->NY;
    return a;
}
// the object's mean modulation factor rides on the carrier when the carrier is a scalar of the transfer-function path
static bool want_cbar(const bdof_ctx* c) { return std::abs(c->a0) > 0.0 && !c->pstack && !c->have_conv; }

// far-field detector + plane-wave carrier: the DC seed of the adjoint is carried as a float64 scalar (AdjCarrier)
static bool use_adj_carrier(const bdof_ctx* c) {
    return c->det_mode == BDOF_DET_FAR && !c->pstack && c->gcar && std::abs(c->a0) > 0.0;
}
static double2 d2(std::complex<double> v) { return make_double2(v.real(), v.imag()); }
// conj(H00)^n: what the adjoint carrier picks up in n adjoint transfer-function steps
static AdjCarrier adj_carrier_at(const bdof_ctx* c, const Group& g, int steps_back) {
    if (!use_adj_carrier(c)) return AdjCarrier{nullptr, nullptr, make_double2(1.0, 0.0), make_float2(0.f, 0.f)};
    return AdjCarrier{c->gcar + g.b0, c->gt0 + g.b0, d2(std::pow(std::conj((1.0 + c->cbm1) * c->h00), steps_back)), cfl(c->cbm1)};
}

// ---- the detector plane (DetPlane, bdof_kernels.h) ------------------------------------------------------------------------
static void set_carrier(DetPlane& d, std::complex<double> a) {
    d.carrier = cfl(a);
    d.carrier_dd = d2(a);
    d.abs_carrier = sqrtf(fmaf(d.carrier.x, d.carrier.x, d.carrier.y * d.carrier.y));      // of the float32 carrier, in float32
}
// a plane to write a wave out at: a carrier (scalar, or one of the ctx's fields and then its float64 twin) and nothing to fit
static DetPlane wave_plane(const bdof_ctx* c, std::complex<double> carrier, const cf* pfield = nullptr) {
    DetPlane d;
    set_carrier(d, carrier);
    d.pfield = pfield;
    d.pfield64 = !pfield ? nullptr : pfield == c->pdet ? c->pdet64 : pfield == c->pdetT ? c->pdetT64 : nullptr;
    return d;
}
// The detector plane and data term of the transfer-function engines for a batch of B wavefields, with the adjoint carriers of
// its sub-batch g; pfield: the carrier field at the detector in the layout of the kernel that gets the plane, or null.
// plane: which of the ctx's detector planes.  They share the data term: its mean runs over the B * planes frames of the batch.
static DetPlane det_plane(const bdof_ctx* c, const Group& g, int B, const cf* pfield, int plane = 0) {
    DetPlane d = wave_plane(c, carrier_det(c, plane), pfield);
    d.a_end = d2(carrier_end(c, plane));
    d.meas_dev = c->meas_dev;
    if (c->meas_dev) {
        // bdof_set_meas_mode(1): the host subtracted |a_0| from the amplitudes; the detector carrier has modulus |a_0| |cbar|^S
        d.meas_ref = std::abs(c->a0);
        d.dref = (float)(std::abs(carrier_end(c, plane)) - std::abs(c->a0));
    }
    d.seed_scale = 2.f / ((float)(B * c->planes) * (float)c->NX * (float)c->NY);
    d.mu = c->loss_mu;
    d.wgt = c->wgt;
    // Set whenever the ctx carries an adjoint carrier, whatever the launch does: the kernels write them only where they fit
    // (a.meas) and reach the DC bin's test (k_row_loss<FAR>; k_g_loss, after its seed64 branch has taken every bin of a float64
    // adjoint), and nothing reads them unless an adjoint sweep follows.
    if (use_adj_carrier(c)) { d.gcar = c->gcar + g.b0; d.gt0 = c->gt0 + g.b0; }
    return d;
}

static bool supported_n(int n) { return n == 64 || n == 128 || n == 256 || n == 512 || n == 1024; }

// ---- profiling helpers -----------------------------------------------------------------------
struct ProfScope {
    bdof_ctx* c;
    int cls;
    hipStream_t st;       // the stream the launch goes to
    bool on;
    bool ext;             // the launch itself carries the events (BDOF_LAUNCH -> hipExtLaunchKernelGGL): nothing is recorded here
    size_t idx = 0;
    ProfScope(bdof_ctx* c_, int cls_, hipStream_t st_, bool ext_ = false) : c(c_), cls(cls_), st(st_), on(c_->prof), ext(ext_) {
        if (on && c->prof_stride > 1 && cls <= BDOF_K_ROW_BWD) on = (c->prof_seen[cls]++ % (unsigned)c->prof_stride) == 0;
        if (!on) return;
        if (c->ev_next + 2 > c->ev_pool.size()) {
            size_t old = c->ev_pool.size();
            c->ev_pool.resize(old + 4096);
            for (size_t i = old; i < c->ev_pool.size(); ++i) (void)hipEventCreate(&c->ev_pool[i]);
        }
        idx = c->ev_next;
        c->ev_next += 2;
        if (!ext) (void)hipEventRecord(c->ev_pool[idx], st);
    }
    hipEvent_t e0() const { return c->ev_pool[idx]; }
    hipEvent_t e1() const { return c->ev_pool[idx + 1]; }
    ~ProfScope() {
        if (!on) return;
        if (!ext) (void)hipEventRecord(c->ev_pool[idx + 1], st);
        c->ev_used.emplace_back(cls, (int)idx);
    }
};
// A timed launch of the per-slice kernel classes: hipExtLaunchKernelGGL stamps the two events with the dispatch's own begin
// and end (what rocprofv3 reports), where an event pair recorded around the launch also contains the ~2.5 us between the
// start marker and the first wave.
#define BDOF_LAUNCH(ps, kernel, grid, blk, shmem, stream, ...)                                                     \
    do {                                                                                                           \
        if ((ps).on) hipExtLaunchKernelGGL(kernel, grid, blk, shmem, stream, (ps).e0(), (ps).e1(), 0, __VA_ARGS__); \
        else hipLaunchKernelGGL(kernel, grid, blk, shmem, stream, __VA_ARGS__);                                    \
    } while (0)

static void prof_collect(bdof_ctx* c) {
    for (auto& u : c->ev_used) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->ev_pool[u.second], c->ev_pool[u.second + 1]) == hipSuccess) {
            c->prof_ms[u.first] += ms;
            c->prof_n[u.first] += 1;
        }
    }
    c->ev_used.clear();
    c->ev_next = 0;
}

// ---- launches --------------------------------------------------------------------------------
// Persistent grids: at most `per_cu` workgroups per CU, and every workgroup gets the same number of tiles.
static int balanced_grid(const bdof_ctx* c, int tiles, int per_cu) {
    const int cap = c->ncu * per_cu;
    if (tiles <= cap) return tiles;
    const int rounds = (tiles + cap - 1) / cap;
    return (tiles + rounds - 1) / rounds;
}
// element-wise kernels: 256 elements per workgroup, at most 16 workgroups per CU (they stride over the rest)
static int g_elem_grid(const bdof_ctx* c, size_t n) { return (int)std::min<size_t>((n + 255) / 256, (size_t)c->ncu * 16); }
template <int N> static int rows_grid(const bdof_ctx* c, int B, int R) {
    return balanced_grid(c, B * R / RowCfg<N>::TILE, N >= 1024 ? 1 : 2);
}

// Line length -> template argument N_: every size of the streaming engine, or those of at most 512 points (the fused sweep's)
#define N_CASE(v, ...) case v: { constexpr int N_ = v; __VA_ARGS__; } break;
#define N_CASES_512(...) N_CASE(64, __VA_ARGS__) N_CASE(128, __VA_ARGS__) N_CASE(256, __VA_ARGS__) N_CASE(512, __VA_ARGS__)
#define DISPATCH_N(n, ...) switch (n) { N_CASES_512(__VA_ARGS__) N_CASE(1024, __VA_ARGS__) default: break; }
#define DISPATCH_N_512(n, ...) switch (n) { N_CASES_512(__VA_ARGS__) default: break; }

// Runtime choice -> template argument: f(std::integral_constant<int, v>) for v in [0, N) (values from N - 1 up take N - 1),
// f(std::true_type / false_type) for a bool; the constant converts to its value where a template argument is expected.
template <int N, int I = 0, class F> static auto with_int(int v, F&& f) {
    if constexpr (I + 1 < N) { if (v != I) return with_int<N, I + 1>(v, f); }
    return f(std::integral_constant<int, I>{});
}
template <class F> static auto with_bool(bool v, F&& f) { return v ? f(std::true_type{}) : f(std::false_type{}); }

// ---- sub-batches --------------------------------------------------------------------------------
// A batch whose tile count fills the chip's workgroup slots badly (25 wavefields of 512 rows = 800 tiles on 512 slots:
// every launch runs as two rounds at 78 % occupancy) is split in two groups that run the same kernel sequence on two
// streams: the groups have no dependencies on each other, so one group's kernels fill the slots the other leaves idle
// and the per-launch round quantisation disappears.  Split holds the groups of one call; every launcher takes its Group.

// HIP maps streams onto a small pool of hardware queues (4 per process by default, GPU_MAX_HW_QUEUES): two streams that
// share a queue run their kernels one after the other, and which streams collide depends on every other stream in the
// process (torch's, RCCL's ...).  Splitting a batch over two such streams only adds launches.  So side streams are
// admitted by measurement: a 200-us spin kernel on each of two streams takes ~200 us when they overlap, ~400 when not.
__global__ void k_spin(long long ticks, int* sink) {
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) {}
    if (sink && ticks < 0) *sink = 1;
}

static bool streams_overlap(bdof_ctx* c, hipStream_t a, hipStream_t b) {
    hipEvent_t e0, e1, ef, ej;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return false;
    (void)hipEventCreateWithFlags(&ef, hipEventDisableTiming);
    (void)hipEventCreateWithFlags(&ej, hipEventDisableTiming);
    const long long ticks = 20000;                 // wall_clock64 counts at 100 MHz: 200 us
    float best = 1e30f;
    for (int rep = 0; rep < 3; ++rep) {            // the first round also pays the lazy creation of the queues
        (void)hipEventRecord(e0, a);
        (void)hipEventRecord(ef, a);
        (void)hipStreamWaitEvent(b, ef, 0);
        hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, a, ticks, (int*)nullptr);
        hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, b, ticks, (int*)nullptr);
        (void)hipEventRecord(ej, b);
        (void)hipStreamWaitEvent(a, ej, 0);
        (void)hipEventRecord(e1, a);
        if (hipStreamSynchronize(a) != hipSuccess) { best = 1e30f; break; }
        float ms = 1e30f;
        if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess && ms < best) best = ms;
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipEventDestroy(ef); (void)hipEventDestroy(ej);
    (void)c;
    return best < 0.3f;                            // 0.2 ms when concurrent, 0.4 ms when serialised
}

static void probe_side_streams(bdof_ctx* c) {
    c->n_side = 0;
    for (int cand = 0; cand < 8 && c->n_side < BDOF_MAX_GROUPS - 1; ++cand) {
        hipStream_t s = nullptr;
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) break;
        c->side_all.push_back(s);
        bool ok = streams_overlap(c, c->stream, s);
        for (int i = 0; ok && i < c->n_side; ++i) ok = streams_overlap(c, c->side[i], s);
        if (ok) c->side[c->n_side++] = s;
    }
}

static int batch_groups(bdof_ctx* c, int B, int rows_per_b, int tile, Group (&g)[BDOF_MAX_GROUPS]) {
    g[0] = Group{0, B, c->stream};
    const int slots = c->ncu * 2;
    const long tiles = (long)B * rows_per_b / tile;
    int n = c->n_streams;
    if (n < 0) n = (B >= 4 && tiles >= slots) ? 2 : 1;      // measured: +3..12 % from 512 tiles up, a loss below
    if (n > BDOF_MAX_GROUPS) n = BDOF_MAX_GROUPS;
    if (n > B) n = B;
    if (n <= 1) return 1;
    if (c->n_side < 0) probe_side_streams(c);
    if (n > 1 + c->n_side) n = 1 + c->n_side;
    if (n <= 1) return 1;
    for (int i = 0, b0 = 0; i < n; ++i) {
        const int Bg = B / n + (i < B % n ? 1 : 0);
        g[i] = Group{b0, Bg, i == 0 ? c->stream : c->side[i - 1]};
        b0 += Bg;
    }
    return n;
}
// The split of one call's batch: open() forms the groups and makes the side streams wait for what the ctx stream has queued,
// `for (const Group& g : split)` visits them, close() makes the ctx stream wait for every side stream.
struct Split {
    Group g[BDOF_MAX_GROUPS];
    int n = 0;
    const Group* begin() const { return g; }
    const Group* end() const { return g + n; }
    int open(bdof_ctx* c, int B, int rows_per_b, int tile) {
        n = batch_groups(c, B, rows_per_b, tile, g);
        if (n > 1) HIPC(c, hipEventRecord(c->ev_fork, c->stream));
        for (int i = 1; i < n; ++i) HIPC(c, hipStreamWaitEvent(g[i].st, c->ev_fork, 0));
        return 0;
    }
    int close(bdof_ctx* c) const {
        for (int i = 1; i < n; ++i) {
            HIPC(c, hipEventRecord(c->ev_join[i - 1], g[i].st));
            HIPC(c, hipStreamWaitEvent(c->stream, c->ev_join[i - 1], 0));
        }
        return 0;
    }
};

static ObjView sub_obj(const bdof_ctx* c, const Group& g) {
    ObjView o = c->obj;
    const int b0 = g.b0;
    if (b0) {
        if (o.tab) { o.angle_of_b += b0; }
        else { o.vol += (size_t)b0 * c->S * c->NX * o.volNY; }
        if (o.xoff) o.xoff += b0;
        if (o.yoff) o.yoff += b0;
    }
    return o;
}
// copy d of a dithered constant: the float32 below or above v, the upper one in a fraction p = (v - below) / ulp of the copies,
// spread evenly (copy d takes it iff floor((d + 1) p + phase) > floor(d p + phase)): the mean over any run of copies is v to
// ulp / (length of the run)
static float dither_pick(double v, int d, double phase) {
    const float r = (float)v;
    float f0 = r, f1 = r;
    if ((double)r > v) f0 = std::nextafterf(r, -4.f); else if ((double)r < v) f1 = std::nextafterf(r, 4.f); else return r;
    const double p = (v - (double)f0) / ((double)f1 - (double)f0);
    return std::floor((d + 1) * p + phase) > std::floor(d * p + phase) ? f1 : f0;
}

// sqrt(1/2) of a slice launch for the transforms compiled with ROUND 1 / ROUND 2 (bdof_fft.h): the nearest float32 and its upper
// neighbour (one transform in four rounds up: the defects cancel to a quarter) — or, with dithered tables, one value for both,
// the upper neighbour in 20.3 % of the slices so that the mean over the slices is sqrt(1/2)
static void sq_of(const bdof_ctx* c, unsigned key, float (&sq)[2]) {
    if (c->tw_dither > 0) sq[0] = sq[1] = dither_pick(0.70710678118654752440, (int)(key % (unsigned)c->tw_dither), 0.5);
    else { sq[0] = 0.70710678118654752f; sq[1] = 0.70710682868957520f; }
}
// the table copy of a slice launch
static const cf* tw_of(bdof_ctx* c, const cf* base, int N, unsigned key) {
    return c->tw_dither > 0 ? base + (size_t)(key % (unsigned)c->tw_dither) * 2 * N : base;
}

template <class T> static T* sub_field(const bdof_ctx* c, const Group& g, T* p) { return p ? p + (size_t)g.b0 * c->NX * c->NY : p; }

// A_z: L1 (or the probe) -> L2 (tstore) or L1 (plain)
static const cf* slice_carrier_field(const bdof_ctx* c, int z) { return c->pstack ? c->pstack + (size_t)z * c->NX * c->NY : nullptr; }

// start != nullptr: slice z starts from the real-space fields start[b] (scattered part) instead of the hybrid `in` — the
// first slice of a range (bdof_forward_range); z == 0 without `start` starts from the probe shared by the batch.
static void launch_row_fwd(bdof_ctx* c, const Group& g, int z, const cf* in, cf* out, bool tstore, cf* phi_out = nullptr, const cf* start = nullptr) {
    ProfScope ps(c, BDOF_K_ROW_FWD, g.st, true);
    RowFwdArgs a{sub_field(c, g, in), start ? sub_field(c, g, start) : c->probe, sub_field(c, g, out), sub_field(c, g, phi_out), sub_obj(c, g), g.B, c->NX, z,
                 c->k, carrier_at(c, z), tw_of(c, c->twY, c->NY, (unsigned)z), slice_carrier_field(c, z), cshift_at(c, z), 0, 1.f, start ? 1 : 0};
    sq_of(c, (unsigned)z, a.sq);
    a.pz_b = 0;
    if (c->range_car) {          // every wavefield of the range rides on its own carrier field
        a.pz = c->range_car + ((size_t)(z - c->range_car_z0) * c->range_car_B + g.b0) * c->NX * c->NY;
        a.pz_b = c->NX;
    }
    DISPATCH_N(c->NY, with_bool(z == 0 || start, [&](auto FIRST) { with_bool(tstore, [&](auto TSTORE) { with_bool(a.pz != nullptr, [&](auto PF) {
        with_bool(c->bin > 1, [&](auto BIN) {
            BDOF_LAUNCH(ps, (k_row_fwd<N_, FIRST, TSTORE, PF, false, BIN>), dim3(rows_grid<N_>(c, g.B, c->NX)), dim3(BDOF_THREADS), 0, g.st, a);
        });
    }); }); }));
}

// A_z^-1 (tape-free adjoint): scattered part of phi_z (L1 hybrid, or real space) -> R eps(psi_z) in L2
static void launch_row_unmod(bdof_ctx* c, const Group& g, int z, const cf* in, cf* out, bool real_in, float in_scale) {
    ProfScope ps(c, BDOF_K_ROW_FWD, g.st, true);
    RowFwdArgs a{sub_field(c, g, in), c->probe, sub_field(c, g, out), nullptr, sub_obj(c, g), g.B, c->NX, z, c->k, carrier_at(c, z), tw_of(c, c->twY, c->NY, (unsigned)z),
                 slice_carrier_field(c, z), cshift_at(c, z), real_in ? 1 : 0, in_scale, 0};
    a.pz_b = 0;
    sq_of(c, (unsigned)z, a.sq);
    DISPATCH_N(c->NY, with_bool(a.pz != nullptr, [&](auto PF) {
        BDOF_LAUNCH(ps, (k_row_fwd<N_, false, true, PF, true>), dim3(rows_grid<N_>(c, g.B, c->NX)), dim3(BDOF_THREADS), 0, g.st, a);
    }));
}

// B: L2 -> L1
// key: the slice whose copy of the dithered constants the launch takes (tw_of, sq_of, and of the slice step's table when h is
// c->hs).  The step between slices z-1 and z runs with copy z-1 in the forward sweep (it follows A_{z-1}); its adjoint, which
// follows A'_z, is handed z-1 too, so that the adjoint step is the transpose of the very operator the forward sweep applied.
static void launch_row_prop(bdof_ctx* c, const Group& g, const cf* in, cf* out, const cf* h, float scale, int conj_h, int key, int cls = BDOF_K_COL_PROP) {
    ProfScope ps(c, cls, g.st, true);
    const unsigned tick = (unsigned)key;
    if (h == c->hs && c->hs_copies > 0) h = c->hs_d + (size_t)(tick % (unsigned)c->hs_copies) * c->NX * c->NY;      // the slice's dithered copy
    RowPropArgs a{sub_field(c, g, in), sub_field(c, g, out), h, g.B, c->NY, scale, conj_h, tw_of(c, c->twX, c->NX, tick)};
    sq_of(c, tick, a.sq);
    DISPATCH_N(c->NX, {
        BDOF_LAUNCH(ps, (k_row_prop<N_, false>), dim3(rows_grid<N_>(c, g.B, c->NY)), dim3(BDOF_THREADS), 0, g.st, a);
    });
}

// Detector planes (bdof_set_detector_planes).  The planes' fields of sub-batch g: D fields per wavefield.
template <class T> static T* sub_planes(const bdof_ctx* c, const Group& g, T* p) { return p ? p + (size_t)g.b0 * c->planes * c->NX * c->NY : p; }
// the tables the streaming engine steps to the planes with: from R phi_{S-1}, so under tf_all combined with the slice step's
static const cf* plane_tables(const bdof_ctx* c) { return c->variant == BDOF_VARIANT_TF_ALL ? c->hcomb_pl : c->hdet_pl; }
// fan-out: L2 lines of bufA -> det_pl (L1, one field per plane); fan-in: the planes' seeds in seed_pl (L2) -> g_hat(phi_{S-1}) in
// bufB (L1).  key: as launch_row_prop's — the last step's, which the one plane's detector step takes too.
static void launch_row_planes(bdof_ctx* c, const Group& g, bool gather, int key, int cls) {
    ProfScope ps(c, cls, g.st, true);
    const unsigned tick = (unsigned)key;
    RowPlanesArgs a{gather ? sub_planes<const cf>(c, g, c->seed_pl) : sub_field<const cf>(c, g, c->bufA),
                    gather ? sub_field<cf>(c, g, c->bufB) : sub_planes<cf>(c, g, c->det_pl), plane_tables(c), g.B, c->NY, c->planes,
                    tw_of(c, c->twX, c->NX, tick)};
    sq_of(c, tick, a.sq);
    DISPATCH_N(c->NX, {
        if (gather) BDOF_LAUNCH(ps, (k_row_prop_gather<N_>), dim3(rows_grid<N_>(c, g.B, c->NY)), dim3(BDOF_THREADS), 0, g.st, a);
        else BDOF_LAUNCH(ps, (k_row_prop_fan<N_>), dim3(rows_grid<N_>(c, g.B, c->NY)), dim3(BDOF_THREADS), 0, g.st, a);
    });
}

// ---- the fused forward sweep (k_slice_y / k_slice_x, bdof_kernels.h) ------------------------------------------------------------
// Which sweep bdof_loss_grad runs: 1 = the fused forward sweep, 0 = the two-kernel sweep.  Eligible: the streaming engine with the
// tape, one voxel slice per step, a scalar carrier, a real-space or no detector, no window offsets, no probe gradient, a separable
// slice step (build_separable), S even and >= 4, lines of at most 512 points (at 1024 a line spans two waves and the transposed
// phase would hold 64 values per thread).
static int fused_mode(const bdof_ctx* c) {
    if (c->fusion < 1 || c->sep_copies < 1 || c->recompute || c->bin != 1 || c->pstack || c->range_car) return 0;
    if (c->det_mode == BDOF_DET_FAR || c->obj.xoff || c->obj.yoff || c->gpsi0) return 0;
    if (c->S < 4 || (c->S & 1) || c->NX > 512 || c->NY > 512) return 0;
    return 1;
}
// The two steps of a slice kernel on x-lines (hx, twX) or y-lines (hy, twY): twiddles, h and sqrt(1/2) of copy `lead` of every
// dithered constant for the leading step, of copy `trail` for the trailing one.
static LineSteps line_steps(bdof_ctx* c, bool x_lines, unsigned lead, unsigned trail) {
    const int N = x_lines ? c->NX : c->NY;
    const cf* tw = x_lines ? c->twX : c->twY;
    const cf* h = x_lines ? c->hx_d : c->hy_d;
    const unsigned D = (unsigned)c->sep_copies;
    LineSteps s{tw_of(c, tw, N, lead), tw_of(c, tw, N, trail), h + (size_t)(lead % D) * N, h + (size_t)(trail % D) * N};
    sq_of(c, lead, s.sq_lead);
    sq_of(c, trail, s.sq_trail);
    return s;
}
// Slice z of the fused forward sweep: even z on y-lines ([b][x][y] -> [b][y][x]), odd z on x-lines (back); phi_z goes to `phi`.
// The leading step takes copy z-1 of every dithered constant, the trailing one copy z.
// blk (the fused adjoint sweep will read the tape): an odd slot takes the tile-block layout of k_slice_x<BLK>.
static void launch_slice(bdof_ctx* c, const Group& g, int z, const cf* in, cf* out, cf* phi, bool blk = false) {
    ProfScope ps(c, BDOF_K_ROW_FWD, g.st, true);
    const bool xl = (z & 1) != 0;
    const int N = xl ? c->NX : c->NY, R = xl ? c->NY : c->NX;
    SliceArgs a{sub_field(c, g, in), c->probe, sub_field(c, g, out), sub_field(c, g, phi), sub_obj(c, g), g.B, R, z, carrier_at(c, z), cshift_at(c, z),
                line_steps(c, xl, (unsigned)(z > 0 ? z - 1 : 0), (unsigned)z)};
    if (xl) {
        DISPATCH_N_512(N, with_bool(blk, [&](auto BLK) {
            BDOF_LAUNCH(ps, (k_slice_x<N_, BLK>), dim3(rows_grid<N_>(c, g.B, R)), dim3(BDOF_THREADS), 0, g.st, a);
        }));
    } else {
        DISPATCH_N_512(N, with_bool(z == 0, [&](auto FIRST) { with_bool(z == c->S - 2, [&](auto TAIL) {
            BDOF_LAUNCH(ps, (k_slice_y<N_, FIRST, TAIL>), dim3(rows_grid<N_>(c, g.B, R)), dim3(BDOF_THREADS), 0, g.st, a);
        }); }));
    }
}

// Slice z <= S-2 of the fused adjoint sweep (k_slice_y_adj / k_slice_x_adj): even z on y-lines ([b][x][y] -> [b][y][x]; at S-2 from
// g_hat in L1 order), odd z on x-lines (back), phi_z from `phi` (odd z: the blocked slot).  The leading step takes copy z of every
// dithered constant, the trailing one copy z-1: the transposes of the steps launch_slice applied.
static void launch_slice_adj(bdof_ctx* c, const Group& g, int z, const cf* in, cf* out, const cf* phi) {
    ProfScope ps(c, BDOF_K_ROW_BWD, g.st, true);
    const bool xl = (z & 1) != 0;
    const int N = xl ? c->NX : c->NY, R = xl ? c->NY : c->NX;
    SliceAdjArgs a{sub_field(c, g, in), sub_field(c, g, phi), sub_field(c, g, out), c->grot + (size_t)g.b0 * c->S * c->NX * c->NY, sub_obj(c, g), g.B, R, z,
                   c->k, carrier_phi_at(c, z), line_steps(c, xl, (unsigned)z, (unsigned)(z > 0 ? z - 1 : 0))};
    if (xl) {
        DISPATCH_N_512(N, BDOF_LAUNCH(ps, (k_slice_x_adj<N_>), dim3(rows_grid<N_>(c, g.B, R)), dim3(BDOF_THREADS), 0, g.st, a));
    } else {
        DISPATCH_N_512(N, with_bool(z == c->S - 2, [&](auto HEAD) { with_bool(z == 0, [&](auto LAST) {
            BDOF_LAUNCH(ps, (k_slice_y_adj<N_, HEAD, LAST>), dim3(rows_grid<N_>(c, g.B, R)), dim3(BDOF_THREADS), 0, g.st, a);
        }); }));
    }
}

// A'_z: L1 (g) + phi tape -> L2 (g)
// hist: 0 = `tape` is the phi tape of slice z; 1 = `tape` is psi_hat_z of the history tape; 2 = slice 0 of the history mode
struct GradTarget {            // where A'_z leaves the gradient rows / G(psi_z): the ctx's own buffers unless a range sweep says otherwise
    float2* grot = nullptr;    // [B][S_][NX][NY]
    int S_ = 0, z_ = 0;
    cf* gpsi = nullptr;        // real-space G(psi_z), [B][NX][NY]
};
static void launch_row_bwd(bdof_ctx* c, const Group& g, int z, const cf* gin, const cf* tape, cf* gout, int hist = 0, float tape_scale = 1.f,
                           const GradTarget* gt = nullptr) {
    ProfScope ps(c, BDOF_K_ROW_BWD, g.st, true);
    float2* grot = gt && gt->grot ? gt->grot + (size_t)g.b0 * gt->S_ * c->NX * c->NY : c->grot + (size_t)g.b0 * c->S * c->NX * c->NY;
    RowBwdArgs a{sub_field(c, g, gin), hist == 2 ? c->probe : sub_field(c, g, tape), sub_field(c, g, gout),
                 grot, sub_obj(c, g), g.B, c->NX, z, c->k, carrier_at(c, z), tw_of(c, c->twY, c->NY, (unsigned)z),
                 slice_carrier_field(c, z), adj_carrier_at(c, g, steps(c).steps_back(z)), cshift_at(c, z), carrier_phi_at(c, z), tape_scale,
                 gt && gt->gpsi ? sub_field(c, g, gt->gpsi) : (z == 0 ? sub_field<cf>(c, g, c->gpsi0) : nullptr),
                 gt && gt->grot ? gt->S_ : c->S, gt && gt->grot ? gt->z_ : steps(c).first_slice(z)};
    sq_of(c, (unsigned)z, a.sq);
    // carrier form: 0 scalar, 1 field (PF), 2 far field + plane-wave carrier (GC; never together with a carrier field)
    const int form = a.ac.gcar ? 2 : a.pz ? 1 : 0;
    if (c->bin > 1) {            // slice binning: the history-mode sweep's two forms (HIST 1, and 2 at step 0) — the only ones it launches
        DISPATCH_N(c->NY, with_bool(hist == 2, [&](auto H2) { with_int<3>(form, [&](auto FORM) {
            BDOF_LAUNCH(ps, (k_row_bwd<N_, H2 ? 2 : 1, FORM == 1, FORM == 2, true>), dim3(rows_grid<N_>(c, g.B, c->NX)), dim3(BDOF_THREADS), 0, g.st, a);
        }); }));
        return;
    }
    DISPATCH_N(c->NY, with_int<4>(hist, [&](auto HIST) { with_int<3>(form, [&](auto FORM) {
        BDOF_LAUNCH(ps, (k_row_bwd<N_, HIST, FORM == 1, FORM == 2>), dim3(rows_grid<N_>(c, g.B, c->NX)), dim3(BDOF_THREADS), 0, g.st, a);
    }); }));
}

// The grid of a detector launch that leaves loss partials.  A workgroup leaves ONE float64 partial for all the tiles it runs, and
// k_sum_partials adds the partials by their index: with the grid balanced over the sub-batch (rows_grid), which tiles share a
// partial depends on how the batch was split, and the loss of one and of two sub-batch streams differed in its last bit (129
// fields of 64 x 512).  per_tile: every workgroup takes one tile, so the partials are per tile and, the sub-batches coming in the
// batch's order, in the batch's tile order whatever the split.  bdof_loss_grad asks for it where loss_tiles_fit says so: one
// detector plane (with D planes the partials come sub-batch by sub-batch, plane by plane: that order does depend on the split)
// and a batch whose tiles fit the partial buffer.  Beyond that, and in every other caller (bdof_loss, the float64 and the
// real-space paths), the grid is the balanced one, as before: their partials group by launch, and a batch that large may still
// differ in the last bit between splits.  A sub-batch of at most 2 ncu tiles (the flagship's) has one tile per workgroup either way.
template <int N> static int loss_grid(const bdof_ctx* c, int B, int R, bool per_tile) {
    return per_tile ? B * R / RowCfg<N>::TILE : rows_grid<N>(c, B, R);
}
static bool loss_tiles_fit(const bdof_ctx* c, int B, bool far) {
    if (c->planes > 1) return false;
    long long tiles = 0;
    DISPATCH_N(far ? c->NX : c->NY, tiles = (long long)B * (far ? c->NY : c->NX) / RowCfg<N_>::TILE);
    return tiles > 0 && tiles <= c->npartial;
}

// The detector kernels of the streaming engine on sub-batch g; with meas they leave their partial sums from slot `part` on and
// return how many (= the grid; per_tile: loss_grid).
static LossArgs loss_args(bdof_ctx* c, const Group& g, const DetPlane& det, const cf* in, cf* out_hyb, cf* out_wave, const float* meas,
                          float in_scale, float out_scale, int part) {
    LossArgs a{};
    a.in = sub_field(c, g, in);
    a.out_hyb = sub_field(c, g, out_hyb);
    a.out_wave = sub_field(c, g, out_wave);
    a.meas = sub_field(c, g, meas);
    a.partial = c->partial + 2 * part;
    a.B = g.B;
    a.in_scale = in_scale;
    a.out_scale = out_scale;
    a.det = det;
    return a;
}
// Real-space detector on L1 rows.
static int launch_loss_real(bdof_ctx* c, const Group& g, const DetPlane& det, const cf* in, cf* out_hyb, bool tstore, cf* out_wave, const float* meas,
                            float in_scale, float out_scale, int part = 0, bool per_tile = false) {
    ProfScope ps(c, BDOF_K_LOSS, g.st);
    LossArgs a = loss_args(c, g, det, in, out_hyb, out_wave, meas, in_scale, out_scale, part);
    a.R = c->NX;
    a.twiddle = c->twY;
    int grid = 0;
    DISPATCH_N(c->NY, grid = loss_grid<N_>(c, g.B, c->NX, per_tile); with_bool(tstore, [&](auto TSTORE) { with_bool(meas && loss_is_poisson(c), [&](auto PSN) {
        with_bool(meas && det.wgt, [&](auto WGT) { hipLaunchKernelGGL((k_row_loss<N_, false, TSTORE, PSN, WGT>), dim3(grid), dim3(BDOF_THREADS), 0, g.st, a); });
    }); }));
    return grid;
}

// Plane j of the detector planes on the L1 rows of det_pl: the real-space detector once per plane, each launch with its own
// DetPlane.  Frames (meas, out_wave) and fields are [B][D][NX][NY], so a launch strides D fields from wavefield to wavefield
// (k_row_loss<PL>); with meas the seed goes transposed to seed_pl.
static int launch_loss_plane(bdof_ctx* c, const Group& g, const DetPlane& det, int j, cf* out_wave, const float* meas, int part = 0) {
    ProfScope ps(c, BDOF_K_LOSS, g.st);
    const size_t pl = (size_t)c->NX * c->NY;
    LossPlaneArgs a;
    static_cast<LossArgs&>(a) = loss_args(c, g, det, nullptr, nullptr, nullptr, nullptr, 1.f, 1.f, part);
    a.in = sub_planes<const cf>(c, g, c->det_pl) + j * pl;
    a.out_hyb = meas ? sub_planes<cf>(c, g, c->seed_pl) + j * pl : nullptr;
    a.out_wave = out_wave ? sub_planes(c, g, out_wave) + j * pl : nullptr;
    a.meas = meas ? sub_planes(c, g, meas) + j * pl : nullptr;
    a.fstride = c->planes;
    a.R = c->NX;
    a.twiddle = c->twY;
    int grid = 0;
    DISPATCH_N(c->NY, grid = rows_grid<N_>(c, g.B, c->NX); with_bool(meas && loss_is_poisson(c), [&](auto PSN) {
        with_bool(meas && det.wgt, [&](auto WGT) { hipLaunchKernelGGL((k_row_loss<N_, false, true, PSN, WGT, true>), dim3(grid), dim3(BDOF_THREADS), 0, g.st, a); });
    }));
    return grid;
}

// Far-field detector on L2 rows; the seed goes back transposed into L1.
static int launch_loss_far(bdof_ctx* c, const Group& g, const DetPlane& det, const cf* in, cf* out_hyb, cf* out_wave, const float* meas,
                           float in_scale, float out_scale, int part = 0, bool per_tile = false) {
    ProfScope ps(c, BDOF_K_LOSS, g.st);
    LossArgs a = loss_args(c, g, det, in, out_hyb, out_wave, meas, in_scale, out_scale, part);
    a.R = c->NY;
    a.twiddle = c->twX;
    int grid = 0;
    DISPATCH_N(c->NX, grid = loss_grid<N_>(c, g.B, c->NY, per_tile); with_bool(meas && loss_is_poisson(c), [&](auto PSN) {
        with_bool(meas && det.wgt, [&](auto WGT) { hipLaunchKernelGGL((k_row_loss<N_, true, true, PSN, WGT>), dim3(grid), dim3(BDOF_THREADS), 0, g.st, a); });
    }));
    return grid;
}

// ---- the sweeps of the streaming engine ---------------------------------------------------------------------------
// bufA is the L2-type scratch (row kernels' transposed output), bufB the L1-type scratch.
// Where the forward sweep leaves the field the detector step starts from, and how that step reads it:
//   DET_NONE, numpy_skip_last : bufA = R phi_{S-1} in L1 order (plain store), un-normalised (scale 1 / NY)
//   DET_NONE, tf_all          : bufB = psi_hat_S (L1), made with the slice step's table
//   DET_NEAR                  : bufB = d_hat (L1)    (tf_all: one step with the combined transfer function)
//   DET_NEAR, D > 1 planes    : det_pl = d_hat_j (L1), [B][D] fields (launch_row_planes; bdof_set_detector_planes)
//   DET_FAR                   : bufA = R phi_{S-1} in L2 order, un-normalised (|fft2| is unchanged by the
//                               unit-modulus transfer function, so tf_all needs no extra step here)
struct DetRoute {
    bool far;              // the far-field kernel on L2 rows (launch_loss_far), else the real-space one on L1 rows
    const cf* in;          // the buffer the detector kernel reads
    float in_scale;
    const cf* h;           // table of the transfer-function step that makes `in` of the last slice's R phi_{S-1}; null: none
    const cf* pfield;      // the carrier field at the detector (probe stack) in the kernel's layout
};
static DetRoute det_route(const bdof_ctx* c) {
    const bool tf_all = c->variant == BDOF_VARIANT_TF_ALL;
    if (c->det_mode == BDOF_DET_FAR) return DetRoute{true, c->bufA, 1.f, nullptr, c->pdetT};
    if (c->det_mode == BDOF_DET_NONE && !tf_all) return DetRoute{false, c->bufA, 1.f / (float)c->NY, nullptr, c->pdet};
    return DetRoute{false, c->bufB, 1.f, c->det_mode == BDOF_DET_NONE ? c->hs : tf_all ? c->hcomb : c->hdet, c->pdet};
}

enum { TAPE_NONE = 0, TAPE_HISTORY = 1, TAPE_LAST = 2 };
// Every group of the split runs A_z then the transfer-function step, slice by slice, on its own stream; each launch is handed
// its group and the slice z whose copy of the dithered constants it takes (the step after A_z takes copy z, as A_z does).
// TAPE_LAST (tape-free adjoint): only the real-space phi_{S-1} is kept (tape slot 0); the adjoint sweep marches it back.
// TAPE_HISTORY keeps psi_hat_{z+1} (the transfer-function step's output) per slice: probe_array of np_funcs.py:43.
// fused (fused_mode; TAPE_HISTORY only): slices 0 .. S-2 run as one k_slice_y / k_slice_x launch each, ping-ponging bufA / bufB in
// real space; tape slot z holds the scattered part of phi_z (z <= S-2) and slot S-1 psi_hat_{S-1}, which one k_row_prop launch with
// the hx-only table makes of the ky-domain lines k_slice_y<TAIL> left in bufA.  The last slice and the detector run as always.
// adj_fused: the fused adjoint sweep follows — the odd slots take k_slice_x<BLK>'s tile blocks, which only k_slice_x_adj reads.
static void forward_sweep(bdof_ctx* c, const Split& split, int tape_mode, bool fused = false, bool adj_fused = false) {
    const size_t fld = (size_t)c->Bmax * c->NX * c->NY;
    const DetRoute dr = det_route(c);
    const int nz = n_steps(c);
    for (int z = 0; z < nz; ++z) {
        const cf* in = nullptr;
        if (z > 0) in = tape_mode == TAPE_HISTORY ? c->tape + (size_t)steps(c).tape_read(z) * fld : c->bufB;
        const bool last = z == nz - 1;
        if (fused && last) in = c->tape + (size_t)z * fld;
        if (fused && !last) {
            for (const Group& g : split) {
                launch_slice(c, g, z, (z & 1) ? c->bufA : c->bufB, (z & 1) ? c->bufB : c->bufA, c->tape + (size_t)z * fld, adj_fused);
                if (z == nz - 2) launch_row_prop(c, g, c->bufA, c->tape + (size_t)(nz - 1) * fld, c->hx_rows, 1.f, 0, z, BDOF_K_LOSS);
            }
            continue;
        }
        cf* phi = tape_mode == TAPE_LAST && last ? c->tape : nullptr;
        for (const Group& g : split) {
            if (!last) {
                launch_row_fwd(c, g, z, in, c->bufA, true, phi);
                launch_row_prop(c, g, c->bufA, tape_mode == TAPE_HISTORY ? c->tape + (size_t)steps(c).tape_write(z) * fld : c->bufB, c->hs, 1.f, 0, z);
            } else {
                launch_row_fwd(c, g, z, in, c->bufA, dr.far || dr.h, phi);
                // (fused route: the step's few remaining transfer-function launches outside the adjoint sweep are filed with the detector)
                if (c->planes > 1) launch_row_planes(c, g, false, z, fused ? BDOF_K_LOSS : BDOF_K_COL_PROP);      // the fan-out to det_pl
                else if (dr.h) launch_row_prop(c, g, c->bufA, c->bufB, dr.h, 1.f, 0, z, fused ? BDOF_K_LOSS : BDOF_K_COL_PROP);
            }
        }
    }
}

// One step of the tape-free march back (BDOF_CFG_RECOMPUTE): P is unitary and c_z is invertible, so the forward
// wave is marched BACK beside the adjoint field instead of being stored per slice, phi_{z-1} = P^H (phi_z / c_z).
// A'_z of form `hist` on the adjoint field (bufB -> bufA) with phi_z from `phi` (real space: phi_real); `step`: the adjoint
// transfer-function step to the slice below (bufA -> bufB); `march`: phi_{z-1} into rc1 (L1), through R eps(psi_z) in rc2 (L2).
static void march_back(bdof_ctx* c, const Group& g, int z, int hist, const cf* phi, bool phi_real, bool step, bool march, cf* rc1, cf* rc2,
                       const GradTarget* gt = nullptr) {
    launch_row_bwd(c, g, z, c->bufB, phi, step ? c->bufA : nullptr, hist, 1.f, gt);
    if (step) launch_row_prop(c, g, c->bufA, c->bufB, c->hs, 1.f, 1, z - 1);
    if (march) {
        launch_row_unmod(c, g, z, phi, rc2, phi_real, 1.f);
        launch_row_prop(c, g, rc2, rc1, c->hs, 1.f, 1, z - 1);
    }
}

// The backward sweep of bdof_loss_grad from the seed g_hat(phi_{S-1}) in bufB: A'_z (L1 -> L2), then the adjoint
// transfer-function step (L2 -> L1), in the form that matches what the forward sweep left on the tape.
//   history  : A'_z recomputes phi_z from psi_hat_z, which the transfer-function kernel writes anyway (one more transform per
//              launch, no tape write in A_z: 104 instead of 112 B per pixel per slice-step, 67.6 -> 65.3 ms per step at 512^3 x 25)
//   fused    : the tape holds phi_z itself (HIST 0) below the last slice, whose psi_hat sits in slot S-1
//   adj_fused: below the top slice (A'_{S-1} and its adjoint step, as above) one launch_slice_adj per slice, ping-ponging bufB / bufA
//              in real space as the forward sweep does: 1 + 1 + (S - 1) launches where the other forms take 2 S - 1
//   tape-free: one A_z^-1 launch and one more adjoint transfer-function launch per slice (+40 B per pixel per slice-step), S - 3
//              fields per wavefield less memory.  phi_{S-1} is kept by the forward sweep (real space, tape slot 0); slots 1 / 2
//              hold the marched-back wave in L1 / L2 order; slice 0 takes phi_0 from the probe as the history form does.
static void adjoint_sweep(bdof_ctx* c, const Split& split, bool fused, bool adj_fused = false) {
    const size_t fld = (size_t)c->Bmax * c->NX * c->NY;
    const int nz = n_steps(c);
    for (int z = nz - 1; z >= 0; --z) {
        const bool top = z == nz - 1;
        for (const Group& g : split) {
            if (c->recompute) {
                march_back(c, g, z, z == 0 ? 2 : top ? 0 : 3, top ? c->tape : c->tape + fld, top, z > 0, z > 1, c->tape + fld, c->tape + 2 * fld);
                continue;
            }
            if (adj_fused && !top) {
                launch_slice_adj(c, g, z, (z & 1) ? c->bufA : c->bufB, (z & 1) ? c->bufB : c->bufA, c->tape + (size_t)z * fld);
                continue;
            }
            if (fused) launch_row_bwd(c, g, z, c->bufB, c->tape + (size_t)z * fld, z > 0 ? c->bufA : nullptr, top ? 1 : 0);
            else launch_row_bwd(c, g, z, c->bufB, z > 0 ? c->tape + (size_t)steps(c).tape_read(z) * fld : nullptr, z > 0 ? c->bufA : nullptr, z > 0 ? 1 : 2);
            if (z > 0) launch_row_prop(c, g, c->bufA, c->bufB, c->hs, 1.f, 1, z - 1);
        }
    }
}

// (Re)build the modulation table c - 1 = exp(i k delta - k beta) - 1 of the object rows when the object or k changed.
// room for n modulation factors and, if the mean-refraction carrier is in use, for the per-workgroup sums of a pass
static int modulation_room(bdof_ctx* c, size_t n, bool mean) {
    HIPC(c, c->mod.room(n));
    if (mean) HIPC(c, c->cbar_dev.room((size_t)c->ncu * 16 + 1));
    return 0;
}
// after a pass that left c - 1 in c->mod (and `grid` partial sums in cbar_dev if mean): mean to the host, object bound
// c - 1 is in c->mod and, if mean, its mean in cbar_dev[at]: mean to the host, object bound
static int modulation_bound(bdof_ctx* c, size_t at, bool mean) {
    std::complex<double> cb(0.0, 0.0);
    if (mean) {
        // cbar is needed by the HOST (it forms the carrier scalars in float64): one small read-back per object update
        double2 m;
        HIPC(c, hipMemcpyAsync(&m, c->cbar_dev + at, sizeof(double2), hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipStreamSynchronize(c->stream));
        cb = std::complex<double>(m.x, m.y);
        // slice binning: a step's carrier picks up the mean factor of its whole bin, cbar^bin (exact algebra for any cbar)
        if (c->bin > 1) cb = std::pow(1.0 + cb, c->bin) - 1.0;
    }
    if (cb != c->cbm1) { c->cbm1 = cb; changed(c, CHANGED_MEAN_MODULATION); }
    c->obj.vol = c->mod;
    modulation_current(c);
    return 0;
}
static int modulation_done(bdof_ctx* c, size_t n, int grid, bool mean) {
    HIPC(c, hipGetLastError());
    changed(c, CHANGED_MOD_OVERWRITTEN);
    if (mean) hipLaunchKernelGGL(k_sum_mean, dim3(1), dim3(256), 0, c->stream, c->cbar_dev, grid, 1.0 / (double)n, c->cbar_dev + grid);
    return modulation_bound(c, grid, mean);
}

static int ensure_modulation(bdof_ctx* c) {
    // (a table taken over from bdof_rotation_adjoint_adam stands only while the mean rides on the carrier as it did then)
    if (!c->mod_dirty && c->mod_mean_pending && c->mod_for_mean != want_cbar(c)) changed(c, CHANGED_MODULATION_K);
    if (!c->mod_dirty) return c->mod_mean_pending ? modulation_bound(c, c->mod_for_mean_at, c->mod_for_mean) : 0;
    if (!c->obj_src) return fail(c, BDOF_ERR_STATE, "the object was bound as modulation factors (bdof_set_object_bilinear): bind it again for this propagator");
    const size_t n = c->obj_rows * (size_t)c->obj.volNY;
    const bool mean = want_cbar(c);
    int r = modulation_room(c, n, mean);
    if (r) return r;
    const int grid = g_elem_grid(c, n);
    hipLaunchKernelGGL(k_modulation_table, dim3(grid), dim3(256), 0, c->stream, c->obj_src, c->mod, n, c->k, mean ? c->cbar_dev : nullptr);
    return modulation_done(c, n, grid, mean);
}

static int ensure_modulation_k(bdof_ctx* c, float k) {
    // the conv propagator's k uses numpy's pi, the FFT path's the reference's literal (quirk Q1): one table per k
    if (c->k != k) { c->k = k; changed(c, CHANGED_MODULATION_K); }
    return ensure_modulation(c);
}

// =================================================================================================
// Generic-size engine (rocFFT).  Fields are real-space [b][x][y] in bufA; the tape holds phi_z.
// =================================================================================================
static bool g_rocfft_ready = false;

#define RFC(c, call)                                                                                \
    do {                                                                                            \
        rocfft_status s_ = (call);                                                                  \
        if (s_ != rocfft_status_success) return fail((c), BDOF_ERR_STATE, std::string(#call) + ": rocfft status " + std::to_string((int)s_)); \
    } while (0)

// rocFFT's execution info of stream `st`, with a work area of at least `need` bytes bound to it.  The area only grows, and the
// stream drains before the old one goes: queued transforms may still use it.
static int fft_exec_room(bdof_ctx* c, FftExec& x, hipStream_t st, size_t need) {
    if (!x.info) {
        RFC(c, rocfft_execution_info_create(&x.info));
        RFC(c, rocfft_execution_info_set_stream(x.info, (void*)st));
    }
    if (x.work.size() < need) {
        HIPC(c, hipStreamSynchronize(st));
        HIPC(c, x.work.alloc(need));
    }
    if (x.work.size()) RFC(c, rocfft_execution_info_set_work_buffer(x.info, x.work, x.work.size()));
    return 0;
}

// the cached in-place 2-D plans of B fields [NX][NY] (the cache keeps them), created at first use; c->fft is ready to execute them
// on the ctx's stream
static int field_plans(bdof_ctx* c, int NX, int NY, int B, bool dbl, rocfft_plan* fwd, rocfft_plan* inv) {
    if (!g_rocfft_ready) { RFC(c, rocfft_setup()); g_rocfft_ready = true; }
    const std::array<int, 4> key{NX, NY, B, dbl ? 1 : 0};
    auto it = c->plans.find(key);
    size_t need = 0;                                                    // a cached pair's work area is there already
    if (it == c->plans.end()) {
        const size_t lengths[2] = {(size_t)NY, (size_t)NX};             // fastest dimension first
        const rocfft_precision prec = dbl ? rocfft_precision_double : rocfft_precision_single;
        PlanPair p;
        RFC(c, rocfft_plan_create(&p.fwd, rocfft_placement_inplace, rocfft_transform_type_complex_forward, prec, 2, lengths, (size_t)B, nullptr));
        RFC(c, rocfft_plan_create(&p.inv, rocfft_placement_inplace, rocfft_transform_type_complex_inverse, prec, 2, lengths, (size_t)B, nullptr));
        size_t w1 = 0, w2 = 0;
        RFC(c, rocfft_plan_get_work_buffer_size(p.fwd, &w1));
        RFC(c, rocfft_plan_get_work_buffer_size(p.inv, &w2));
        need = std::max(w1, w2);
        it = c->plans.emplace(key, std::move(p)).first;
    }
    if (int r = fft_exec_room(c, c->fft, c->stream, need)) return r;
    *fwd = it->second.fwd;
    *inv = it->second.inv;
    return 0;
}

// the transfer function of the step after slice z: its dithered float32 copy where the caller handed the float64 table over
static const cf* hs_slice(const bdof_ctx* c, int z) {
    return c->hs_copies > 0 ? c->hs_d + (size_t)((unsigned)z % (unsigned)c->hs_copies) * c->NX * c->NY : c->hs;
}

// The one free-space step of the rocFFT paths, in place on B fields [NX][NY] of either precision: fields <- F^-1' ( h * F fields ),
// queued on stream st, whose execution info x is (c->fft and c->stream, or the auxiliary pair once bdof_fields_free_step_aux has
// given it room).  The table is h[kx][ky], or the fused engine's h[ky][kx]; it carries the transforms' 1 / (NX NY), unless
// scale says otherwise (float64 [kx][ky] tables only).  prof_cls: the profiling class the step is filed under, if any.
enum TableOrder { H_KXKY, H_KYKX };
static int free_step(bdof_ctx* c, FftExec& x, hipStream_t st, void* fields, int B, int NX, int NY, const void* h, TableOrder order, int conj_h,
                     bool dbl, int prof_cls = -1, double scale = 1.0) {
    rocfft_plan pf, pi;
    if (int r = field_plans(c, NX, NY, B, dbl, &pf, &pi)) return r;
    std::optional<ProfScope> ps;
    if (prof_cls >= 0) ps.emplace(c, prof_cls, st);
    void* buf[1] = {fields};
    const size_t n = (size_t)B * NX * NY;
    const dim3 grid(g_elem_grid(c, n));
    RFC(c, rocfft_execute(pf, buf, nullptr, x.info));
    if (scale != 1.0)
        hipLaunchKernelGGL((k_hmul<double2, false, true>), grid, dim3(256), 0, st, (double2*)fields, (const double2*)h, NX, NY, n, conj_h, scale);
    else with_bool(order == H_KYKX, [&](auto KYKX) {
        if (dbl) hipLaunchKernelGGL((k_hmul<double2, KYKX>), grid, dim3(256), 0, st, (double2*)fields, (const double2*)h, NX, NY, n, conj_h, 1.0);
        else hipLaunchKernelGGL((k_hmul<float2, KYKX>), grid, dim3(256), 0, st, (float2*)fields, (const float2*)h, NX, NY, n, conj_h, 1.f);
    });
    RFC(c, rocfft_execute(pi, buf, nullptr, x.info));
    return 0;
}
// a transfer-function step of the generic engine's ctx fields (tables in the fused engine's order), filed under BDOF_K_COL_PROP
static int generic_prop(bdof_ctx* c, int B, void* field, const void* h, int conj_h, bool dbl = false) {
    return free_step(c, c->fft, c->stream, field, B, c->NX, c->NY, h, H_KYKX, conj_h, dbl, BDOF_K_COL_PROP);
}

// Forward sweep; leaves the field the detector starts from in bufA (eps part) and returns its carrier.
static int generic_forward_sweep(bdof_ctx* c, int B, bool tape, rocfft_plan pf, std::complex<double>* carrier_out) {
    const size_t fld = (size_t)c->Bmax * c->NX * c->NY;
    const size_t n = (size_t)B * c->NX * c->NY;
    std::complex<double> a = c->a0;
    int r;
    const int nz = n_steps(c);
    for (int z = 0; z < nz; ++z) {
        {
            ProfScope ps(c, BDOF_K_ROW_FWD, c->stream);
            GModArgs m{c->bufA, z == 0 ? c->probe : nullptr, tape ? c->tape + (size_t)z * fld : nullptr, c->obj, B, c->NX, c->NY, z,
                       make_float2((float)a.real(), (float)a.imag()), c->pstack ? c->pstack + (size_t)z * c->NX * c->NY : nullptr,
                       cfl(a * c->cbm1)};
            with_bool(c->bin > 1, [&](auto BIN) { hipLaunchKernelGGL(k_g_modulate<BIN>, dim3(g_elem_grid(c, n)), dim3(256), 0, c->stream, m); });
            a *= 1.0 + c->cbm1;                  // mean-refraction carrier: phi_z rides on cbar a_z
        }
        if (z < nz - 1 || step_after_last(c)) {
            if ((r = generic_prop(c, B, c->bufA, hs_slice(c, z), 0))) return r;      // the slice's dithered copy of H
            a *= c->h00;
        }
    }
    if (c->det_mode == BDOF_DET_NEAR && c->planes > 1) {
        // detector planes: the sweep ends in front of the detector step (generic_to_planes takes it from here)
    } else if (c->det_mode == BDOF_DET_NEAR) {
        if ((r = generic_prop(c, B, c->bufA, c->hdet, 0))) return r;
        a *= c->hdet00;
    } else if (c->det_mode == BDOF_DET_FAR) {
        void* buf[1] = {c->bufA};
        RFC(c, rocfft_execute(pf, buf, nullptr, c->fft.info));
        a *= (double)c->NX * (double)c->NY;
    }
    *carrier_out = a;
    return 0;
}

// k_g_loss on a [B][NX][NY] field (the ctx's detector kind decides the layout of meas / out_wave)
static GLossArgs g_loss_args(bdof_ctx* c, int B, const DetPlane& det, cf* field, cf* out_wave, const float* meas) {
    GLossArgs la{};
    la.field = field;
    la.out_wave = out_wave;
    la.meas = meas;
    la.partial = c->partial;
    la.B = B;
    la.NX = c->NX;
    la.NY = c->NY;
    la.far = c->det_mode == BDOF_DET_FAR;
    la.det = det;
    return la;
}

// Detector planes on the generic engine: plane j's field of the batch, [D][Bmax][NX][NY] in det_pl
static cf* generic_plane(const bdof_ctx* c, int j) { return c->det_pl + (size_t)j * c->Bmax * c->NX * c->NY; }
// the wave in front of the detector step (bufA) stepped to every plane: one copy and one generic_prop per plane
static int generic_to_planes(bdof_ctx* c, int B) {
    const size_t n = (size_t)B * c->NX * c->NY;
    for (int j = 0; j < c->planes; ++j) {
        HIPC(c, hipMemcpyAsync(generic_plane(c, j), c->bufA, n * sizeof(cf), hipMemcpyDeviceToDevice, c->stream));
        if (int r = generic_prop(c, B, generic_plane(c, j), c->hdet_pl + (size_t)j * c->NX * c->NY, 0)) return r;
    }
    return 0;
}

static int generic_forward(bdof_ctx* c, int B, void* out_wave, bool keep_tape) {
    rocfft_plan pf, pi;
    int r = field_plans(c, c->NX, c->NY, B, false, &pf, &pi);
    if (r) return r;
    std::complex<double> a;
    if ((r = generic_forward_sweep(c, B, keep_tape, pf, &a))) return r;
    if (out_wave && c->planes > 1) {
        if ((r = generic_to_planes(c, B))) return r;
        const size_t n = (size_t)B * c->NX * c->NY;
        for (int j = 0; j < c->planes; ++j) {
            GLossArgs la = g_loss_args(c, B, wave_plane(c, a * c->hdet00_pl[j]), generic_plane(c, j), (cf*)out_wave + (size_t)j * c->NX * c->NY, nullptr);
            la.fstride = c->planes;
            hipLaunchKernelGGL((k_g_loss<false, false, true>), dim3(g_elem_grid(c, n)), dim3(256), 0, c->stream, la);
        }
    } else if (out_wave) {
        const size_t n = (size_t)B * c->NX * c->NY;
        const GLossArgs la = g_loss_args(c, B, wave_plane(c, a, c->pdet), c->bufA, (cf*)out_wave, nullptr);
        hipLaunchKernelGGL(k_g_loss<false>, dim3(g_elem_grid(c, n)), dim3(256), 0, c->stream, la);
    }
    return 0;
}

static int generic_loss_grad(bdof_ctx* c, int B, const float* meas, void* out_wave) {
    rocfft_plan pf, pi;
    int r = field_plans(c, c->NX, c->NY, B, false, &pf, &pi);
    if (r) return r;
    const size_t fld = (size_t)c->Bmax * c->NX * c->NY;
    const size_t n = (size_t)B * c->NX * c->NY;
    std::complex<double> a;
    if ((r = generic_forward_sweep(c, B, true, pf, &a))) return r;
    const int egrid = g_elem_grid(c, n);
    const bool f64 = c->adj64;
    if (f64 && !c->have_h64) return fail(c, BDOF_ERR_STATE, "float64 adjoint: bdof_set_physics_f64 has not been called");
    if (c->planes > 1) {
        // Detector planes: the data term once per plane on its own field (the carrier as the sweep's recurrence left it, times
        // the plane's DC value), the adjoint detector step per plane, and the sum of the D results in bufA
        if ((r = generic_to_planes(c, B))) return r;
        const size_t pl = (size_t)c->NX * c->NY;
        const int lgrid = std::min(egrid, c->npartial);
        for (int j = 0; j < c->planes; ++j) {
            ProfScope ps(c, BDOF_K_LOSS, c->stream);
            DetPlane det = det_plane(c, whole(c, B), B, nullptr, j);
            set_carrier(det, a * c->hdet00_pl[j]);
            GLossArgs la = g_loss_args(c, B, det, generic_plane(c, j), out_wave ? (cf*)out_wave + j * pl : nullptr, meas + j * pl);
            la.fstride = c->planes;
            la.partial = c->partial + (size_t)2 * j * lgrid;
            with_bool(loss_is_poisson(c), [&](auto PSN) { with_bool(det.wgt != nullptr, [&](auto WGT) {
                hipLaunchKernelGGL((k_g_loss<PSN, WGT, true>), dim3(lgrid), dim3(256), 0, c->stream, la);
            }); });
        }
        hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, c->stream, c->partial, lgrid * c->planes, 1.0 / ((double)B * c->planes * c->NX * c->NY), c->loss_dev);
        for (int j = 0; j < c->planes; ++j) {
            if ((r = generic_prop(c, B, generic_plane(c, j), c->hdet_pl + j * pl, 1))) return r;
            hipLaunchKernelGGL(k_g_accumulate, dim3(egrid), dim3(256), 0, c->stream, c->bufA, generic_plane(c, j), n, j == 0 ? 1 : 0);
        }
    } else {
        ProfScope ps(c, BDOF_K_LOSS, c->stream);
        DetPlane det = det_plane(c, whole(c, B), B, c->pdet);
        set_carrier(det, a);                       // the carrier as the sweep's own recurrence left it
        GLossArgs la = g_loss_args(c, B, det, c->bufA, (cf*)out_wave, meas);
        la.seed64 = f64 ? c->g64 : nullptr;        // float64 adjoint: every bin's seed stays in float64, no adjoint carrier to split off
        with_bool(loss_is_poisson(c), [&](auto PSN) { with_bool(meas && det.wgt, [&](auto WGT) {
            hipLaunchKernelGGL((k_g_loss<PSN, WGT>), dim3(egrid), dim3(256), 0, c->stream, la);
        }); });
    }
    if (c->planes == 1)
        hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, c->stream, c->partial, egrid, 1.0 / ((double)B * c->NX * c->NY), c->loss_dev);
    if (f64) {
        // float64 adjoint sweep: g64 holds the seed G(d)
        rocfft_plan pf64, pi64;
        if ((r = field_plans(c, c->NX, c->NY, B, true, &pf64, &pi64))) return r;
        void* b64[1] = {c->g64};
        if (c->det_mode == BDOF_DET_NEAR) { if ((r = generic_prop(c, B, c->g64, c->hdet64, 1, true))) return r; }
        else if (c->det_mode == BDOF_DET_FAR) RFC(c, rocfft_execute(pi64, b64, nullptr, c->fft.info));
        for (int z = c->S - 1; z >= 0; --z) {
            if ((z < c->S - 1 || step_after_last(c)) && (r = generic_prop(c, B, c->g64, c->hs64, 1, true))) return r;
            ProfScope ps(c, BDOF_K_ROW_BWD, c->stream);
            GBwd64Args ba{c->g64, c->tape + (size_t)z * fld, c->grot, c->obj, B, c->NX, c->NY, z, (double)c->k,
                          d2(carrier_z(c, z) * (1.0 + c->cbm1)), c->pstack ? 1 : 0};
            hipLaunchKernelGGL(k_g_bwd64, dim3(egrid), dim3(256), 0, c->stream, ba);
        }
        // G(psi_0) for bdof_probe_grad, where the float32 sweep leaves it
        hipLaunchKernelGGL(k_d_to_f, dim3(egrid), dim3(256), 0, c->stream, c->g64, c->bufA, B * c->NX, c->NY, 0);
        return 0;
    }
    // adjoint of the detector step: bufA now holds the seed G(d)
    void* buf[1] = {c->bufA};
    if (c->det_mode == BDOF_DET_NEAR && c->planes > 1) {
        // (detector planes: done above, plane by plane)
    } else if (c->det_mode == BDOF_DET_NEAR) {
        if ((r = generic_prop(c, B, c->bufA, c->hdet, 1))) return r;
    } else if (c->det_mode == BDOF_DET_FAR) {
        RFC(c, rocfft_execute(pi, buf, nullptr, c->fft.info));            // F^H = unnormalised inverse
    }
    const int nz = n_steps(c);
    for (int z = nz - 1; z >= 0; --z) {
        if ((z < nz - 1 || step_after_last(c)) && (r = generic_prop(c, B, c->bufA, hs_slice(c, z), 1))) return r;      // conj of the forward step's copy
        ProfScope ps(c, BDOF_K_ROW_BWD, c->stream);
        GBwdArgs ba{c->bufA, c->tape + (size_t)z * fld, c->grot, c->obj, B, c->NX, c->NY, z, c->k, carrier_phi_at(c, z), c->pstack ? 1 : 0,
                    adj_carrier_at(c, whole(c, B), steps(c).steps_back(z))};
        with_bool(c->bin > 1, [&](auto BIN) { hipLaunchKernelGGL(k_g_bwd<BIN>, dim3(egrid), dim3(256), 0, c->stream, ba); });
    }
    return 0;
}

// the dynamic LDS limit of kernel K, raised once per device (the attribute is per device: a process may hold ctxs on several)
template <auto K> static int max_lds_once(bdof_ctx* c, int bytes) {
    static bool attr_set[BDOF_MAX_DEVICES] = {};
    if (!attr_set[c->device % BDOF_MAX_DEVICES]) {
        HIPC(c, hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        attr_set[c->device % BDOF_MAX_DEVICES] = true;
    }
    return 0;
}

// ---- LDS-resident engine ---------------------------------------------------------------------------
template <int N, int T, int WPE, bool PSN, bool WGT, bool SEEDED = false> static int resident_launch_t(bdof_ctx* c, const ResArgs& a, int grid, int* waves) {
    *waves = T / 64;
    const size_t lds = sizeof(cf) * ((size_t)N * (N | 1) + 2 * N) + sizeof(long long) * 3 * N;
    if (int r = max_lds_once<k_resident<N, T, WPE, PSN, WGT, SEEDED>>(c, (int)lds)) return r;
    hipLaunchKernelGGL((k_resident<N, T, WPE, PSN, WGT, SEEDED>), dim3(grid), dim3(T), lds, c->stream, a);
    return 0;
}
// seeded: the adjoint sweep alone, from the seeds in a.out_wave (k_resident's SEEDED instance; the data term is outside it)
template <int N> static int resident_launch(bdof_ctx* c, const ResArgs& a, int grid, int* waves, bool seeded) {
    if (seeded) return resident_launch_t<N, ResPlan<N>::T, ResPlan<N>::WPE, false, false, true>(c, a, grid, waves);
    return with_bool(a.meas && loss_is_poisson(c), [&](auto PSN) { return with_bool(a.meas && a.det.wgt, [&](auto WGT) {
        return resident_launch_t<N, ResPlan<N>::T, ResPlan<N>::WPE, PSN, WGT>(c, a, grid, waves);
    }); });
}

// One workgroup per wavefield: against the streaming kernels (sizes with a fused plan) the resident engine wins once the
// batch fills a good part of the chip (measured at 64^2 / 128^2: 400 / 100 wavefields 4.6x / 1.5x faster, 25 slower);
// sizes without a fused plan always take it (the alternative is the unfused rocFFT engine).
static bool use_resident(const bdof_ctx* c, int B) {
    if (!c->resident || c->recompute || c->bin > 1 || c->planes > 1) return false;      // slice binning, detector planes: the streaming and generic engines only
    // far field + plane-wave carrier needs the adjoint carrier (AdjCarrier), which the resident kernel does not carry: the
    // streaming / generic engines take that case (plane-wave full-field at a resident-plan size)
    if (c->det_mode == BDOF_DET_FAR && !c->pstack && std::abs(c->a0) > 0.0) return false;
    return c->generic || c->res_always || B * 4 >= c->ncu;
}

// What every launch of the resident kernel on B wavefields shares: tables, object, shapes.  The caller adds the probe and its
// carriers, the tape, the detector plane and the buffers the launch reads and writes.
static ResArgs resident_args(const bdof_ctx* c, int B) {
    const bool hdith = c->hs_copies > 0 && c->hsT_d;
    ResArgs a{};
    a.hsT = hdith ? c->hsT_d : c->hsT;
    a.hD = hdith ? c->hs_copies : 0;
    a.hdetT = c->hdetT;
    a.tape_stride = (size_t)c->Bmax * c->NX * c->NY;
    a.obj = c->obj;
    a.twiddle = c->twR;
    a.B = B;
    a.S = c->S;
    a.det_mode = c->det_mode;
    a.tf_all = c->variant == BDOF_VARIANT_TF_ALL ? 1 : 0;
    a.k = c->k;
    return a;
}
// the launch of the plan of the ctx's size; grid: the workgroups of the launch, *waves: the waves of each
static int resident_grid(const bdof_ctx* c, int B) { return B < c->npartial ? B : c->npartial; }
static int resident_dispatch(bdof_ctx* c, const ResArgs& a, int* waves, bool seeded = false) {
    const int grid = resident_grid(c, a.B);
    switch (c->NX) {
        case 32: return resident_launch<32>(c, a, grid, waves, seeded);
        case 36: return resident_launch<36>(c, a, grid, waves, seeded);
        case 48: return resident_launch<48>(c, a, grid, waves, seeded);
        case 64: return resident_launch<64>(c, a, grid, waves, seeded);
        case 72: return resident_launch<72>(c, a, grid, waves, seeded);
        case 80: return resident_launch<80>(c, a, grid, waves, seeded);
        case 96: return resident_launch<96>(c, a, grid, waves, seeded);
        case 128: return resident_launch<128>(c, a, grid, waves, seeded);
        default: return fail(c, BDOF_ERR_SIZE, "no resident plan for this size");
    }
}

static int resident_run(bdof_ctx* c, int B, const float* meas, void* out_wave, bool do_grad) {
    if (c->res_dirty) {
        std::vector<cf> car(2 * (size_t)c->S);
        for (int z = 0; z < c->S; ++z) { car[z] = carrier_at(c, z); car[c->S + z] = cshift_at(c, z); }
        HIPC(c, hipStreamSynchronize(c->stream));
        if (int r = upload(c, c->res_carrier, car.data(), car.size(), KEEP)) return r;
        resident_current(c);
    }
    ProfScope ps(c, BDOF_K_ROW_FWD, c->stream);
    const bool grad = do_grad && meas;
    ResArgs a = resident_args(c, B);
    a.probe = c->probe;
    a.tape = grad ? c->tape : nullptr;
    a.grot = c->grot;
    a.gpsi0 = grad ? c->gpsi0 : nullptr;
    a.carrier = c->res_carrier;
    a.pstack = c->pstack;
    a.meas = meas;
    a.out_wave = (cf*)out_wave;
    a.partial = c->partial;
    a.do_grad = grad ? 1 : 0;
    a.det = det_plane(c, whole(c, B), B, c->pdet);
    const int grid = resident_grid(c, B);
    int waves = 1;
    if (int r = resident_dispatch(c, a, &waves)) return r;
    if (meas)
        hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, c->stream, c->partial, grid * waves, 1.0 / ((double)B * c->NX * c->NY),
                           c->loss_dev);
    return launched(c);
}

// ---- probe modes (bdof_set_probe_modes; bdof_modes.h) -----------------------------------------------------------------------
// Three phases per call, B windows and M modes, wavefield (m, j) at index m B + j of bufA, bufB, the tape, gpsi0 and — until the
// last launch — of the gradient rows: (1) the forward sweep of every wavefield, which leaves the scattered part of its detector
// wave; (2) k_modes_couple: the data term on sum_m |d_m|^2 and the M seeds; (3) the adjoint sweep of every wavefield into its own
// rows [m B + j][S] of grot, then k_modes_sum_rows: [B][S][NX][NY] with the modes summed, what bdof_grot promises.  The rows fit:
// grot holds Bmax wavefields and B M <= Bmax.  The object view and the offsets are per window, so every kernel that reads them
// is launched per mode on its sub-batch of B; the transforms of the generic engine run batched over all B M fields.
static bool modes_resident(const bdof_ctx* c) { return c->resident; }      // else the generic engine (MODE_STREAMING_ONLY is refused)
static size_t modes_sub(const bdof_ctx* c, int B, int m) { return (size_t)m * B * c->NX * c->NY; }      // mode m's sub-batch in a field buffer

// phase 1, resident: one launch per mode of the forward instance, the tape handed in when a gradient follows; a detector plane
// without a carrier, so bufA receives the scattered parts alone, in the order of meas
static int modes_resident_forward(bdof_ctx* c, int B, bool tape) {
    ProfScope ps(c, BDOF_K_ROW_FWD, c->stream);
    for (int m = 0; m < c->n_modes; ++m) {
        ResArgs a = resident_args(c, B);
        a.probe = c->m_zero;
        a.carrier = c->m_zero;
        a.pstack = c->m_stack + (size_t)m * c->S * c->NX * c->NY;
        a.tape = tape ? c->tape + modes_sub(c, B, m) : nullptr;
        a.out_wave = c->bufA + modes_sub(c, B, m);
        int waves;
        if (int r = resident_dispatch(c, a, &waves)) return r;
    }
    return 0;
}
// phase 3, resident: one launch per mode of the seeded instance, seeds in bufB
static int modes_resident_adjoint(bdof_ctx* c, int B) {
    ProfScope ps(c, BDOF_K_ROW_BWD, c->stream);
    for (int m = 0; m < c->n_modes; ++m) {
        ResArgs a = resident_args(c, B);
        a.carrier = c->m_zero;
        a.pstack = c->m_stack + (size_t)m * c->S * c->NX * c->NY;
        a.tape = c->tape + modes_sub(c, B, m);
        a.out_wave = c->bufB + modes_sub(c, B, m);
        a.grot = c->grot + modes_sub(c, B, m) * c->S;
        a.gpsi0 = c->gpsi0 ? c->gpsi0 + modes_sub(c, B, m) : nullptr;
        a.do_grad = 1;
        int waves;
        if (int r = resident_dispatch(c, a, &waves, true)) return r;
    }
    return 0;
}
// phase 1, generic: the forward sweep of generic_forward_sweep with the modulation per mode; bufA ends as the scattered parts
// of the detector waves, [x][y] (far field [kx][ky])
static int modes_generic_forward(bdof_ctx* c, int B, bool tape) {
    const int BM = B * c->n_modes, nz = n_steps(c);
    const size_t fld = (size_t)c->Bmax * c->NX * c->NY, pl = (size_t)c->NX * c->NY, n = (size_t)B * pl;
    const cf zero = make_float2(0.f, 0.f);
    rocfft_plan pf, pi;
    int r = field_plans(c, c->NX, c->NY, BM, false, &pf, &pi);
    if (r) return r;
    for (int z = 0; z < nz; ++z) {
        for (int m = 0; m < c->n_modes; ++m) {
            ProfScope ps(c, BDOF_K_ROW_FWD, c->stream);
            GModArgs ma{c->bufA + modes_sub(c, B, m), z == 0 ? (const cf*)c->m_zero : nullptr, tape ? c->tape + (size_t)z * fld + modes_sub(c, B, m) : nullptr,
                        c->obj, B, c->NX, c->NY, z, zero, c->m_stack + ((size_t)m * nz + z) * pl, zero};
            hipLaunchKernelGGL(k_g_modulate<false>, dim3(g_elem_grid(c, n)), dim3(256), 0, c->stream, ma);
        }
        if ((z < nz - 1 || step_after_last(c)) && (r = generic_prop(c, BM, c->bufA, hs_slice(c, z), 0))) return r;
    }
    if (c->det_mode == BDOF_DET_NEAR) return generic_prop(c, BM, c->bufA, c->hdet, 0);
    if (c->det_mode == BDOF_DET_FAR) {
        void* buf[1] = {c->bufA};
        RFC(c, rocfft_execute(pf, buf, nullptr, c->fft.info));
    }
    return 0;
}
// phase 3, generic: the adjoint loop of generic_loss_grad on the seeds in bufA, k_g_bwd per mode; G(psi_0) stays in bufA
static int modes_generic_adjoint(bdof_ctx* c, int B) {
    const int BM = B * c->n_modes, nz = n_steps(c);
    const size_t fld = (size_t)c->Bmax * c->NX * c->NY, n = (size_t)B * c->NX * c->NY;
    rocfft_plan pf, pi;
    int r = field_plans(c, c->NX, c->NY, BM, false, &pf, &pi);
    if (r) return r;
    void* buf[1] = {c->bufA};
    if (c->det_mode == BDOF_DET_NEAR) { if ((r = generic_prop(c, BM, c->bufA, c->hdet, 1))) return r; }
    else if (c->det_mode == BDOF_DET_FAR) RFC(c, rocfft_execute(pi, buf, nullptr, c->fft.info));            // F^H = unnormalised inverse
    const AdjCarrier none{nullptr, nullptr, make_double2(1.0, 0.0), make_float2(0.f, 0.f)};
    for (int z = nz - 1; z >= 0; --z) {
        if ((z < nz - 1 || step_after_last(c)) && (r = generic_prop(c, BM, c->bufA, hs_slice(c, z), 1))) return r;
        for (int m = 0; m < c->n_modes; ++m) {
            ProfScope ps(c, BDOF_K_ROW_BWD, c->stream);
            GBwdArgs ba{c->bufA + modes_sub(c, B, m), c->tape + (size_t)z * fld + modes_sub(c, B, m), c->grot + modes_sub(c, B, m) * c->S, c->obj,
                        B, c->NX, c->NY, z, c->k, make_float2(0.f, 0.f), 1, none};
            hipLaunchKernelGGL(k_g_bwd<false>, dim3(g_elem_grid(c, n)), dim3(256), 0, c->stream, ba);
        }
    }
    return 0;
}
// phase 2: meas == nullptr writes the detector waves alone (bdof_forward)
static void modes_couple(bdof_ctx* c, int B, const float* meas, void* out_wave) {
    ProfScope ps(c, BDOF_K_LOSS, c->stream);
    const size_t n = (size_t)B * c->NX * c->NY;
    const bool res = modes_resident(c);
    ModesArgs a{};
    a.e = c->bufA;
    a.seed = res ? c->bufB : c->bufA;
    a.out_wave = (cf*)out_wave;
    a.meas = meas;
    a.pdet64 = c->m_det64;
    a.wgt = c->wgt;
    a.partial = c->partial;
    a.M = c->n_modes; a.B = B; a.NX = c->NX; a.NY = c->NY;
    a.far = c->det_mode == BDOF_DET_FAR;
    a.e_meas_order = res ? 1 : 0;
    a.seed_scale = 2.0 / ((double)B * c->NX * c->NY);
    a.mu = c->loss_mu;
    const int grid = g_elem_grid(c, n);
    with_bool(meas && loss_is_poisson(c), [&](auto PSN) { with_bool(meas && c->wgt, [&](auto WGT) {
        hipLaunchKernelGGL((k_modes_couple<PSN, WGT>), dim3(grid), dim3(256), 0, c->stream, a);
    }); });
    if (meas) hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, c->stream, c->partial, grid, 1.0 / ((double)B * c->NX * c->NY), c->loss_dev);
}
static int check_modes_batch(bdof_ctx* c, int B) {
    return (long long)B * c->n_modes > c->Bmax ? fail(c, BDOF_ERR_ARG, "probe modes: windows times modes must not exceed Bmax (B M <= Bmax)") : 0;
}
static int modes_forward(bdof_ctx* c, int B, void* out_wave) {
    int r = modes_resident(c) ? modes_resident_forward(c, B, false) : modes_generic_forward(c, B, false);
    if (r) return r;
    if (out_wave) modes_couple(c, B, nullptr, out_wave);
    return launched(c);
}
static int modes_loss_grad(bdof_ctx* c, int B, const float* meas, void* out_wave) {
    const bool res = modes_resident(c);
    int r = res ? modes_resident_forward(c, B, true) : modes_generic_forward(c, B, true);
    if (r) return r;
    modes_couple(c, B, meas, out_wave);
    if ((r = res ? modes_resident_adjoint(c, B) : modes_generic_adjoint(c, B))) return r;
    if (c->n_modes > 1) {
        const size_t rows = (size_t)B * c->S * c->NX * c->NY;
        hipLaunchKernelGGL(k_modes_sum_rows, dim3(g_elem_grid(c, rows)), dim3(256), 0, c->stream, c->grot, c->n_modes, rows);
    }
    c->gpsi_src = res ? (const cf*)c->gpsi0 : (const cf*)c->bufA;
    return launched(c);
}

static int check_ready(bdof_ctx* c, int B) {
    if (!c) return BDOF_ERR_ARG;
    if (int r = need_configured(c)) return r;
    if (!c->have_physics) return fail(c, BDOF_ERR_STATE, "bdof_set_physics has not been called");
    if (!c->have_probe && !c->n_modes) return fail(c, BDOF_ERR_STATE, "bdof_set_probe has not been called");
    if (!c->obj_src && !c->obj_bound_mod) return fail(c, BDOF_ERR_STATE, "bdof_set_object has not been called");
    return check_batch(c, B);
}

// ---- the tile family: tiles cut out of a field / written back into it, and the adjoints ---------------------------------------
// Every entry point fills the TileArgs of its precision pairing and hands it to launch_tiles: shapes, taper (gathers) and halo (scatters) are
// checked — the one an entry point does not take is 0 and passes — then one launch of 256-thread workgroups on the ctx stream,
// over the tiles' rows (TILE_GRID: y blocks of 256, up to 64 workgroups along x, one z per tile) or over the field's rows
// (FIELD_GRID: the adjoints that sum the tiles into the field).
enum TileGrid { TILE_GRID, FIELD_GRID };
template <class Args>
static int launch_tiles(bdof_ctx* c, const void* field, const void* tiles, TileGrid shape, void (*kernel)(Args), const Args& a) {
    if (!c || !field || !tiles || !a.x0 || !a.y0) return BDOF_ERR_ARG;
    if (a.B < 1 || a.FX < 1 || a.FY < 1 || a.TX < 1 || a.TY < 1) return fail(c, BDOF_ERR_ARG, "bad tile / field shape");
    int r;
    if ((r = check_taper(c, a.TX, a.TY, a.taper)) || (r = check_halo(c, a.TX, a.TY, a.hx, a.hy))) return r;
    // the field-row kernels list whole tiles, BDOF_TILE_MAXLIST (tile, row) pairs at a time (any B): one tile alone must fit
    if (shape == FIELD_GRID && (a.TX + a.FX - 1) / a.FX > BDOF_TILE_MAXLIST)
        return fail(c, BDOF_ERR_SIZE, "a tile wraps onto one field row more often than a workgroup lists (TX <= 1024 FX)");
    HIPC(c, hipSetDevice(c->device));
    const dim3 grid = shape == TILE_GRID ? dim3((a.TY + 255) / 256, std::min(a.TX, 64), a.B) : dim3(std::min(a.FX, c->ncu * 8));
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, c->stream, a);
    return launched(c);
}

extern "C" {

int bdof_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int bdof_device_pci_bus_id(int device, char* out, int len) {
    if (!out || len < 16) return BDOF_ERR_ARG;
    out[0] = 0;
    return (int)hipDeviceGetPCIBusId(out, len, device);
}

// stream-ordered time stamps on the ctx stream: bdof_timer_mark(slot) now, bdof_timer_elapsed(a, b) after a sync
int bdof_timer_mark(bdof_ctx* c, int slot) {
    if (!c || slot < 0 || slot >= BDOF_N_TIMERS) return BDOF_ERR_ARG;
    HIPC(c, hipSetDevice(c->device));
    if (!c->timer[slot]) HIPC(c, hipEventCreate(&c->timer[slot]));
    HIPC(c, hipEventRecord(c->timer[slot], c->stream));
    return 0;
}
int bdof_timer_elapsed(bdof_ctx* c, int slot_a, int slot_b, double* ms) {
    if (!c || !ms || slot_a < 0 || slot_a >= BDOF_N_TIMERS || slot_b < 0 || slot_b >= BDOF_N_TIMERS) return BDOF_ERR_ARG;
    if (!c->timer[slot_a] || !c->timer[slot_b]) return fail(c, BDOF_ERR_STATE, "bdof_timer_elapsed: slot never marked");
    HIPC(c, hipEventSynchronize(c->timer[slot_b]));
    float f = 0.f;
    HIPC(c, hipEventElapsedTime(&f, c->timer[slot_a], c->timer[slot_b]));
    *ms = (double)f;
    return 0;
}

int bdof_ctx_create(bdof_ctx** out, int device, void* stream) {
    if (!out) return BDOF_ERR_ARG;
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) return e != hipSuccess ? (int)e : (int)hipErrorNoDevice;
    if (device < 0 || device >= n) return BDOF_ERR_ARG;
    bdof_ctx* c = new bdof_ctx();
    c->device = device;
    e = hipSetDevice(device);
    if (e != hipSuccess) { delete c; return (int)e; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->ncu = prop.multiProcessorCount;
    if (stream) { c->stream = (hipStream_t)stream; }
    else {
        e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        if (e != hipSuccess) { delete c; return (int)e; }
        c->own_stream = true;
    }
    (void)hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming);
    for (int i = 0; i < BDOF_MAX_GROUPS - 1; ++i) (void)hipEventCreateWithFlags(&c->ev_join[i], hipEventDisableTiming);
    if (const char* e = std::getenv("BDOF_STREAMS")) c->n_streams = std::atoi(e);
    *out = c;
    return 0;
}

void bdof_ctx_destroy(bdof_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (auto& e : c->ev_pool) (void)hipEventDestroy(e);
    for (auto& e : c->timer) if (e) (void)hipEventDestroy(e);
    for (hipStream_t s : c->side_all) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
    if (c->aux) { (void)hipStreamSynchronize(c->aux); (void)hipStreamDestroy(c->aux); }
    if (c->ev_aux_fork) (void)hipEventDestroy(c->ev_aux_fork);
    if (c->ev_aux_join) (void)hipEventDestroy(c->ev_aux_join);
    for (int i = 0; i < BDOF_MAX_GROUPS - 1; ++i)
        if (c->ev_join[i]) (void)hipEventDestroy(c->ev_join[i]);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;                                    // every stream has drained: the owning members release the device memory and the plans
}

const char* bdof_last_error(const bdof_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

int bdof_sync(bdof_ctx* c) {
    if (!c) return BDOF_ERR_ARG;
    HIPC(c, hipStreamSynchronize(c->stream));
    return 0;
}

// exp(-2 pi i j / N) in float32, rounded so that the MODULUS is as close to one as float32 allows: among the roundings
// of (cos, sin) up or down (each candidate within one ulp of the true value) the pair with the smallest | |w|^2 - 1 |.
// Plain round-to-nearest leaves every twiddle with a modulus error of +-3e-8; the factors do not average out along the
// paths of a transform, a chain of hundreds of transforms then drifts in energy.
static cf unit_twiddle(double c, double s) {
    const float c0 = (float)c, s0 = (float)s;
    const float cc[3] = {c0, std::nextafterf(c0, 2.f), std::nextafterf(c0, -2.f)};
    const float ss[3] = {s0, std::nextafterf(s0, 2.f), std::nextafterf(s0, -2.f)};
    float bc = c0, bs = s0;
    double best = std::fabs((double)c0 * c0 + (double)s0 * s0 - 1.0);
    for (float x : cc)
        for (float y : ss) {
            if (std::fabs((double)x - c) > std::fabs((double)std::nextafterf(c0, 2.f) - (double)c0)) continue;      // > 1 ulp away
            if (std::fabs((double)y - s) > std::fabs((double)std::nextafterf(s0, 2.f) - (double)s0)) continue;
            const double e = std::fabs((double)x * x + (double)y * y - 1.0);
            if (e < best) { best = e; bc = x; bs = y; }
        }
    return make_float2(bc, bs);
}

// D copies (D <= 1: one copy, nearest rounding with the modulus kept closest to one) of the twiddle table of length N; per copy
// N hi values, then N lo values (the float32 rounding error of the hi ones), (re, im) pairs
static void fill_twiddle_tables(int N, int D, cf* t) {
    const int copies = D > 1 ? D : 1;
    for (int d = 0; d < copies; ++d)
        for (int j = 0; j < N; ++j) {
            const double ang = -2.0 * M_PI * (double)j / (double)N;
            cf* td = t + (size_t)d * 2 * N;
            if (D > 1) {
                // golden-ratio phases: a different offset of the up / down pattern for every entry and component
                const double ph1 = std::fmod(0.6180339887498949 * (2 * j + 1), 1.0), ph2 = std::fmod(0.6180339887498949 * (2 * j + 2) + 0.37, 1.0);
                td[j] = make_float2(dither_pick(std::cos(ang), d, ph1), dither_pick(std::sin(ang), d, ph2));
            } else td[j] = unit_twiddle(std::cos(ang), std::sin(ang));
            td[(size_t)N + j] = make_float2((float)(std::cos(ang) - (double)td[j].x), (float)(std::sin(ang) - (double)td[j].y));
        }
}

int bdof_twiddle_tables(int N, int D, float* out) {
    if (N < 1 || D < 0 || D > 256 || !out) return BDOF_ERR_ARG;
    fill_twiddle_tables(N, D, (cf*)out);
    return 0;
}

static int upload_twiddle(bdof_ctx* c, int N, DevBuf<cf>& dst, bool dither = true) {
    const int D = dither && c->tw_dither > 1 ? c->tw_dither : 1;
    std::vector<cf> t((size_t)N * 2 * D);
    fill_twiddle_tables(N, D, t.data());
    HIPC(c, dst.alloc(t.size()));
    HIPC(c, hipMemcpyAsync(dst, t.data(), sizeof(cf) * t.size(), hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return 0;
}

int bdof_configure(bdof_ctx* c, int NY, int NX, int S, int Bmax, int with_grad) {
    if (!c) return BDOF_ERR_ARG;
    if (NY < 1 || NX < 1 || S < 1 || Bmax < 1) return fail(c, BDOF_ERR_ARG, "NY, NX, S and Bmax must be >= 1");
    const bool generic = (with_grad & (BDOF_CFG_GENERIC | BDOF_CFG_ADJOINT64)) != 0 || !supported_n(NY) || !supported_n(NX);
    if (generic && (size_t)NY * NX > ((size_t)1 << 26)) return fail(c, BDOF_ERR_SIZE, "wavefield too large");
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    static_cast<Workspace&>(*c) = Workspace{};       // the previous configuration's buffers, plans and flags go before the new ones come
    c->NY = NY; c->NX = NX; c->S = S; c->Bmax = Bmax; c->with_grad = (with_grad & BDOF_CFG_GRAD) != 0;
    c->obj.bin = 1;                                  // slice binning is not sticky: bdof_set_slice_binning follows, or there is none
    c->generic = generic;
    // dithered transform constants (bdof_fft.h): 64 copies of each table by default, BDOF_TW_DITHER=0 for one plain table
    { const char* e = std::getenv("BDOF_TW_DITHER"); c->tw_dither = e ? std::max(0, std::min(256, atoi(e))) : 64; if (c->tw_dither == 1) c->tw_dither = 0; }
    c->recompute = (with_grad & BDOF_CFG_RECOMPUTE) != 0 && !generic;      // the streaming engine's option; the others keep their tapes
    c->adj64 = (with_grad & BDOF_CFG_ADJOINT64) != 0 && c->with_grad;
    c->resident = (with_grad & (BDOF_CFG_GENERIC | BDOF_CFG_NO_RESIDENT | BDOF_CFG_ADJOINT64)) == 0 && NX == NY && resident_supported(NX);
    c->res_always = (with_grad & BDOF_CFG_ALWAYS_RESIDENT) != 0;
    changed(c, CHANGED_CONFIGURATION);
    c->have_physics = c->have_probe = false;
    int r;
    if (c->resident) {
        if ((r = upload_twiddle(c, NX, c->twR, false))) return r;       // one launch runs all slices: one table
        HIPC(c, c->hsT.alloc((size_t)NX * NY));
        HIPC(c, c->hdetT.alloc((size_t)NX * NY));
        HIPC(c, c->res_carrier.alloc(2 * (size_t)S));
    }
    if (!generic) {
        if ((r = upload_twiddle(c, NY, c->twY))) return r;
        if ((r = upload_twiddle(c, NX, c->twX))) return r;
    }
    const size_t fld = (size_t)Bmax * NX * NY;
    HIPC(c, c->hs.alloc((size_t)NX * NY));
    HIPC(c, c->hdet.alloc((size_t)NX * NY));
    HIPC(c, c->hcomb.alloc((size_t)NX * NY));
    HIPC(c, c->probe.alloc((size_t)NX * NY));
    HIPC(c, c->bufA.alloc(fld));
    HIPC(c, c->bufB.alloc(fld));
    if (c->with_grad) {
        // tape-free adjoint: phi_{S-1} (real space) + the two fields the marched-back wave alternates between
        const bool small_tape = c->recompute && !(c->resident && c->res_always);
        c->recompute = small_tape;
        HIPC(c, c->tape.alloc(fld * (size_t)(small_tape ? std::min(S, 3) : S)));
        // BDOF_CFG_NO_GROT: the caller sweeps slice ranges into gradient buffers of its own (bdof_adjoint_range, the tiled path),
        // where [Bmax][S] rows would not fit — 260 GB for 121 tiles of 512^2 x 1024 slices
        if ((with_grad & BDOF_CFG_NO_GROT) == 0) HIPC(c, c->grot.alloc(fld * (size_t)S));
        HIPC(c, c->gcar.alloc((size_t)Bmax));
        HIPC(c, c->gt0.alloc((size_t)Bmax));
    }
    if (c->adj64) {
        HIPC(c, c->g64.alloc(fld));
        HIPC(c, c->hs64.alloc((size_t)NX * NY));
        HIPC(c, c->hdet64.alloc((size_t)NX * NY));
    }
    c->npartial = c->ncu * 16 + 64;
    // the resident kernel leaves one pair per workgroup AND wave (up to 16 waves)
    HIPC(c, c->partial.alloc((size_t)2 * c->npartial * (c->resident ? 16 : 1)));
    HIPC(c, c->loss_dev.alloc(1));
    HIPC(c, hipMemsetAsync(c->loss_dev, 0, sizeof(double), c->stream));
    return 0;
}

int bdof_set_slice_binning(bdof_ctx* c, int bin) {
    if (int r = enter_setter(c, true)) return r;
    if (!StepIndex::valid(c->S, bin)) return fail(c, BDOF_ERR_ARG, "bdof_set_slice_binning: bin must be >= 1 and divide S (a shorter last bin is not carried)");
    if (c->have_physics || c->have_probe)
        return fail(c, BDOF_ERR_STATE, "bdof_set_slice_binning comes right after bdof_configure: the tables of bdof_set_physics and the carrier fields are per propagation step");
    if (bin > 1)
        if (int r = refuse_modes(c, "bdof_set_slice_binning", "slice binning", {&MODE_RESIDENT, &MODE_RECOMPUTE, &MODE_ADJOINT64, &MODE_NO_GROT})) return r;
    if (c->with_grad && bin != c->bin) HIPC(c, c->tape.alloc((size_t)c->Bmax * c->NX * c->NY * StepIndex{c->S, bin}.tape_fields()));     // one field per step
    c->bin = c->obj.bin = bin;
    changed(c, CHANGED_BINNING);
    return 0;
}

int bdof_set_physics(bdof_ctx* c, double k, const float* hs, const float* hs_det, const double* h00, const double* hdet00,
                     int det_mode, int variant) {
    if (!c || !hs || !h00) return BDOF_ERR_ARG;
    if (int r = enter_setter(c, false)) return r;
    if (det_mode < 0 || det_mode > 2 || variant < 0 || variant > 1) return fail(c, BDOF_ERR_ARG, "bad det_mode / variant");
    if (det_mode == BDOF_DET_NEAR && !hs_det) return fail(c, BDOF_ERR_ARG, "hs_det required for BDOF_DET_NEAR");
    const size_t n = (size_t)c->NX * c->NY, bytes = sizeof(cf) * n;
    if (c->planes > 1) HIPC(c, hipStreamSynchronize(c->stream));      // launches in flight may still read the planes that go
    changed(c, CHANGED_PHYSICS);
    HIPC(c, hipMemcpyAsync(c->hs, hs, bytes, hipMemcpyHostToDevice, c->stream));
    if (hs_det) {
        HIPC(c, hipMemcpyAsync(c->hdet, hs_det, bytes, hipMemcpyHostToDevice, c->stream));
        const std::vector<float> comb = combined(hs, hs_det, n, 1);
        HIPC(c, hipMemcpyAsync(c->hcomb, comb.data(), bytes, hipMemcpyHostToDevice, c->stream));
        HIPC(c, hipStreamSynchronize(c->stream));
    }
    if (c->resident) {
        // the resident kernel multiplies the field image [kx][ky] element by element: tables in that order
        if (int r = upload(c, c->hsT, transposed(hs, c->NY, c->NX).data(), n, KEEP)) return r;
        if (hs_det)
            if (int r = upload(c, c->hdetT, transposed(hs_det, c->NY, c->NX).data(), n, KEEP)) return r;
    }
    HIPC(c, hipStreamSynchronize(c->stream));
    c->k = c->k_fft = (float)k;
    c->h00 = std::complex<double>(h00[0], h00[1]);
    c->hdet00 = hdet00 ? std::complex<double>(hdet00[0], hdet00[1]) : std::complex<double>(1.0, 0.0);
    c->det_mode = det_mode;
    c->variant = variant;
    c->have_physics = true;
    return 0;
}

// The separable factors of the slice step for the fused forward sweep, from the float64 table H[ky][kx] (1 / (NX NY) folded in):
//     hx[kx] = H[0][kx] / H[0][0] / NX,   hy[ky] = H[ky][0] NX      =>  hy[ky] hx[kx] = H[ky][kx],
// so that Fx^-1 hx Fx is Px with its normalisation (a constant passes unchanged) and Fy^-1 hy Fy is Py with 1 / NY and the step's
// phase H00.  Separability is checked here, in float64: max |H[ky][kx] H00 - H[ky][0] H[0][kx]| <= 1e-14 |H00|^2; a table that
// fails (an impulse-response kernel, anything set by hand) leaves sep_copies = 0 and the sweep unfused.  D copies of each, dithered
// over the slices exactly as the 2-D table is (k_dither_copies: the entry's golden-ratio phase, up in a fraction p of the copies).
static int build_separable(bdof_ctx* c, const double* hs64, int D) {
    typedef std::complex<double> cd;
    c->sep_copies = 0;
    const int NX = c->NX, NY = c->NY;
    if (c->generic || NX > 512 || NY > 512 || c->S < 2 || D < 1) return 0;
    auto H = [&](int ky, int kx) { const size_t i = (size_t)ky * NX + kx; return cd(hs64[2 * i], hs64[2 * i + 1]); };
    const cd h00 = H(0, 0);
    const double tol = 1e-14 * std::norm(h00);
    if (!(std::norm(h00) > 0.0)) return 0;
    for (int ky = 0; ky < NY; ++ky) {
        const cd hy0 = H(ky, 0);
        for (int kx = 0; kx < NX; ++kx)
            if (!(std::abs(H(ky, kx) * h00 - hy0 * H(0, kx)) <= tol)) return 0;
    }
    auto copies = [&](int n, auto value, std::vector<cf>& t) {
        t.resize((size_t)D * n);
        for (int i = 0; i < n; ++i) {
            const cd v = value(i);
            const double g = (double)(i % 1048573) * 0.6180339887498949;
            const double ph = g - std::floor(g), ph2 = ph + 0.5 - std::floor(ph + 0.5);
            for (int d = 0; d < D; ++d) t[(size_t)d * n + i] = make_float2(dither_pick(v.real(), d, ph), dither_pick(v.imag(), d, ph2));
        }
    };
    std::vector<cf> hx, hy, rows((size_t)NX * NY);
    copies(NX, [&](int kx) { return H(0, kx) / h00 / (double)NX; }, hx);
    copies(NY, [&](int ky) { return H(ky, 0) * (double)NX; }, hy);
    const cf* hx_top = hx.data() + (size_t)((c->S - 2) % D) * NX;
    for (int ky = 0; ky < NY; ++ky) std::copy(hx_top, hx_top + NX, rows.begin() + (size_t)ky * NX);
    int r;
    if ((r = upload(c, c->hx_d, hx.data(), hx.size(), FRESH)) || (r = upload(c, c->hy_d, hy.data(), hy.size(), FRESH)) ||
        (r = upload(c, c->hx_rows, rows.data(), rows.size(), FRESH))) return r;
    c->sep_copies = D;
    return 0;
}

// D dithered float32 copies of a float64 table of n complex entries into dst (k_dither_copies, bdof_field.h), through the device
// scratch tmp of n entries; drains the ctx stream, so the host table and tmp may go when this returns
static int dither_copies(bdof_ctx* c, DevBuf<cf>& dst, const double* host64, size_t n, int D, DevBuf<double2>& tmp) {
    hipError_t e = dst.alloc((size_t)D * n);
    if (e != hipSuccess) return fail(c, (int)e, "hipMalloc of the dithered transfer-function copies failed");
    e = hipMemcpy(tmp, host64, n * sizeof(double2), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_dither_copies, dim3(g_elem_grid(c, n)), dim3(256), 0, c->stream, tmp, dst, n, D);
        e = hipStreamSynchronize(c->stream);
    }
    return e == hipSuccess ? 0 : fail(c, (int)e, "building the dithered transfer-function copies failed");
}

// The slice step's transfer function in float64 ([ky][kx], 1 / (NX NY) folded in — what bdof_set_physics' hs was rounded from):
// the streaming engine's per-slice launches then multiply by DITHERED float32 copies of it, copy z mod D for slice z
// (bdof_field.h: k_dither_copies; D = BDOF_H_DITHER, default 64 capped at 256 MiB of tables, 0 = off), the adjoint step by the
// conjugate of the copy the forward step used.  A fixed float32 table is the same perturbation of every slice: its error grows
// linearly with the number of slices (np_funcs.py:42 runs float64).
int bdof_set_transfer_f64(bdof_ctx* c, const double* hs64) {
    if (!c || !hs64) return BDOF_ERR_ARG;
    if (!c->have_physics) return fail(c, BDOF_ERR_STATE, "bdof_set_physics has not been called");
    const char* env = std::getenv("BDOF_H_DITHER");
    const size_t n = (size_t)c->NX * c->NY;
    int D = env ? std::max(0, std::min(256, atoi(env))) : 64;
    while (D > 1 && (size_t)D * n * sizeof(cf) > ((size_t)256 << 20)) D /= 2;
    changed(c, CHANGED_SLICE_STEP_F64);
    if (D < 2) return 0;
    if (int r = enter_setter(c, true)) return r;
    c->hs_d.reset();
    c->hsT_d.reset();
    DevBuf<double2> tmp;
    HIPC(c, tmp.alloc(n));
    if (int r = dither_copies(c, c->hs_d, hs64, n, D, tmp)) return r;
    // the LDS-resident kernel multiplies its field image [kx][ky] element by element: the same copies, transposed
    if (c->resident)
        if (int r = dither_copies(c, c->hsT_d, transposed(hs64, c->NY, c->NX).data(), n, D, tmp)) return r;
    c->hs_copies = D;
    return build_separable(c, hs64, D);
}

int bdof_set_physics_f64(bdof_ctx* c, const double* hs, const double* hs_det) {
    if (!c || !hs) return BDOF_ERR_ARG;
    if (!c->adj64) return fail(c, BDOF_ERR_STATE, "bdof_set_physics_f64 needs bdof_configure with flag 64 (float64 adjoint sweep)");
    if (!c->have_physics) return fail(c, BDOF_ERR_STATE, "bdof_set_physics has not been called");
    if (c->det_mode == BDOF_DET_NEAR && !hs_det) return fail(c, BDOF_ERR_ARG, "hs_det required for BDOF_DET_NEAR");
    int r = enter_setter(c, true);
    if (r) return r;
    const size_t n = (size_t)c->NX * c->NY;
    if ((r = upload(c, c->hs64, hs, n, KEEP)) || (hs_det && (r = upload(c, c->hdet64, hs_det, n, KEEP)))) return r;
    c->have_h64 = true;
    return 0;
}

int bdof_set_probe(bdof_ctx* c, const float* probe, double a0_re, double a0_im) {
    if (!c || !probe) return BDOF_ERR_ARG;
    if (int r = enter_setter(c, false)) return r;
    changed(c, CHANGED_PROBE);
    HIPC(c, hipMemcpyAsync(c->probe, probe, sizeof(cf) * c->NX * c->NY, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    c->a0 = std::complex<double>(a0_re, a0_im);
    c->have_probe = true;
    return 0;
}

int bdof_set_meas_mode(bdof_ctx* c, int mode) {
    if (!c) return BDOF_ERR_ARG;
    if (mode != 0 && mode != 1) return fail(c, BDOF_ERR_ARG, "bdof_set_meas_mode: mode must be 0 or 1");
    c->meas_dev = mode;
    return 0;
}

int bdof_set_loss(bdof_ctx* c, int kind, double multiplier) {
    if (!c) return BDOF_ERR_ARG;
    if (kind != BDOF_LOSS_LSQ && kind != BDOF_LOSS_POISSON) return fail(c, BDOF_ERR_ARG, "bdof_set_loss: kind must be BDOF_LOSS_LSQ or BDOF_LOSS_POISSON");
    if (!(multiplier > 0.0)) return fail(c, BDOF_ERR_ARG, "bdof_set_loss: multiplier must be > 0");
    c->loss_kind = kind;
    c->loss_mu = multiplier;
    return 0;
}

int bdof_set_detector_weights(bdof_ctx* c, const float* w) {
    if (int r = enter_setter(c, true)) return r;       // launches in flight may still read the plane that goes
    if (!w) { c->wgt.reset(); return 0; }
    return upload(c, c->wgt, w, (size_t)c->NX * c->NY, GROW);
}

int bdof_set_detector_planes(bdof_ctx* c, int D, const float* hs_det, const double* hdet00) {
    if (int r = enter_setter(c, true)) return r;      // launches in flight may still read the tables and fields that go
    if (D < 1 || D > BDOF_MAX_PLANES) return fail(c, BDOF_ERR_ARG, "bdof_set_detector_planes: the number of detector planes must be in [1, BDOF_MAX_PLANES]");
    if (D == 1 || !hs_det) { drop_planes(c); return 0; }
    if (!hdet00) return fail(c, BDOF_ERR_ARG, "bdof_set_detector_planes: hdet00 required with the tables");
    if (!c->have_physics) return fail(c, BDOF_ERR_STATE, "bdof_set_detector_planes comes after bdof_set_physics");
    if (int r = refuse_modes(c, "bdof_set_detector_planes", "detector planes",
                             {&MODE_NOT_NEAR, &MODE_RECOMPUTE, &MODE_ADJOINT64, &MODE_CONV, &MODE_CARRIER_FIELD, &MODE_RANGE_CARRIER, &MODE_PROBE_MODES})) return r;
    changed(c, CHANGED_DETECTOR_PLANES);
    const size_t n = (size_t)c->NX * c->NY, fields = (size_t)c->Bmax * D * n;
    // the combined tables of tf_all, formed as bdof_set_physics forms its one: from the float32 slice step the ctx holds
    std::vector<float> hs(2 * n);
    HIPC(c, hipMemcpy(hs.data(), c->hs, sizeof(cf) * n, hipMemcpyDeviceToHost));
    int r;
    if ((r = upload(c, c->hdet_pl, hs_det, n * D, FRESH)) || (r = upload(c, c->hcomb_pl, combined(hs.data(), hs_det, n, D).data(), n * D, FRESH))) return r;
    HIPC(c, c->det_pl.alloc(fields));
    if (c->with_grad && !c->generic) HIPC(c, c->seed_pl.alloc(fields));
    // every plane's launch leaves its own partial sums: room for D times those of one plane
    HIPC(c, c->partial.room((size_t)2 * c->npartial * D * (c->resident ? 16 : 1)));
    for (int j = 0; j < D; ++j) c->hdet00_pl.push_back(std::complex<double>(hdet00[2 * j], hdet00[2 * j + 1]));
    c->planes = D;
    return 0;
}

int bdof_adjoint_carrier(bdof_ctx* c, int B, double* gcar, double* gt0) {
    if (!c || !gcar || !gt0) return BDOF_ERR_ARG;
    int r;
    if ((r = need_configured(c)) || (r = check_batch(c, B))) return r;
    if (!use_adj_carrier(c) || c->adj64) return 0;      // (the float64 adjoint keeps every bin's seed in its own field)
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    HIPC(c, hipMemcpy(gcar, c->gcar, sizeof(double2) * B, hipMemcpyDeviceToHost));
    HIPC(c, hipMemcpy(gt0, c->gt0, sizeof(double2) * B, hipMemcpyDeviceToHost));
    return 1;
}

int bdof_probe_stack_supported(bdof_ctx* c) {
    // every engine of the transfer-function path carries it (the real-space propagator of bdof_set_conv does not)
    return c && c->NY > 0 ? 1 : 0;
}

int bdof_set_probe_stack(bdof_ctx* c, const float* stack, const float* det) {
    int r = enter_setter(c, true);
    if (r) return r;
    c->pstack.reset(); c->pdet.reset(); c->pdetT.reset();
    c->pdet64.reset(); c->pdetT64.reset();                     // a host-supplied stack comes in float32 only
    changed(c, CHANGED_CARRIER_FIELD);
    if (!stack && !det) return 0;
    if (!stack || !det) return fail(c, BDOF_ERR_ARG, "bdof_set_probe_stack: both arrays or neither");
    if ((r = admit(c, "a carrier field (bdof_set_probe_stack)", CARRIES_BINNING | CARRIES_MODES | NO_DATA_TERM))) return r;
    const size_t n = (size_t)c->NX * c->NY;
    if ((r = upload(c, c->pstack, stack, n * steps(c).stack_planes(), FRESH))) return r;       // one plane per propagation step
    if ((r = upload(c, c->pdet, det, n, FRESH))) return r;
    // the streaming far-field detector works on rows [ky][kx]: the same field transposed
    return upload(c, c->pdetT, transposed(det, c->NX, c->NY).data(), n, FRESH);
}

// The carrier field of a localised probe (bdof_set_probe_stack) computed ON THE DEVICE in float64: S - 1 transfer-function steps
// of one field with rocFFT's double-precision plans (np_funcs.py:42 without an object), each plane rounded once into the
// float32 stack.  A probe that changes every Adam step (probe_type='optimizable') then costs ~4 small launches per slice
// instead of 2 S host FFTs and a 1-GiB upload.
// The carrier field of ONE probe, queued on the ctx stream: dp (device [NX][NY] complex128, overwritten) stepped through free
// space with the tables dh / dhd ([kx][ky], without the transforms' 1 / n; dhd: the detector step, BDOF_DET_NEAR only); every
// plane rounded once into `stack`, the detector plane into det / detT (transposed) and unrounded into det64 / detT64 — each of
// the four where the caller has a reader for it (null: not written).
struct CarrierField { cf *stack, *det, *detT; double2 *det64, *detT64; };
static int build_carrier_field(bdof_ctx* c, double2* dp, const double2* dh, const double2* dhd, const CarrierField& out) {
    const size_t n = (size_t)c->NX * c->NY;
    rocfft_plan pf, pi;
    int r;
    if ((r = field_plans(c, c->NX, c->NY, 1, true, &pf, &pi))) return r;       // fields are [x][y]
    const int nz = n_steps(c);                                   // one plane per propagation step (dh: the step's own table)
    const int grid = g_elem_grid(c, n);
    void* buf[1] = {dp};
    auto step = [&](const double2* h) {      // the caller's tables come without the transforms' 1 / n
        return free_step(c, c->fft, c->stream, dp, 1, c->NX, c->NY, h, H_KXKY, 0, true, -1, 1.0 / (double)n);
    };
    for (int z = 0; z < nz; ++z) {
        hipLaunchKernelGGL(k_d_to_f, dim3(grid), dim3(256), 0, c->stream, dp, out.stack + (size_t)z * n, c->NX, c->NY, 0);
        if ((z < nz - 1 || step_after_last(c)) && (r = step(dh))) return r;
    }
    if (c->det_mode == BDOF_DET_FAR) RFC(c, rocfft_execute(pf, buf, nullptr, c->fft.info));
    else if (c->det_mode == BDOF_DET_NEAR && (r = step(dhd))) return r;
    if (out.det) hipLaunchKernelGGL(k_d_to_f, dim3(grid), dim3(256), 0, c->stream, dp, out.det, c->NX, c->NY, 0);
    if (out.detT) hipLaunchKernelGGL(k_d_to_f, dim3(grid), dim3(256), 0, c->stream, dp, out.detT, c->NX, c->NY, 1);
    // ... and unrounded: the detector kernels add the scattered wave to these and take |d| - m in float64 (seed_f64)
    if (out.det64) hipLaunchKernelGGL(k_d_copy, dim3(grid), dim3(256), 0, c->stream, dp, out.det64, c->NX, c->NY, 0);
    if (out.detT64) hipLaunchKernelGGL(k_d_copy, dim3(grid), dim3(256), 0, c->stream, dp, out.detT64, c->NX, c->NY, 1);
    HIPC(c, hipGetLastError());
    return 0;
}

int bdof_set_probe_field(bdof_ctx* c, const double* probe, const double* hT, const double* hdetT) {
    if (!c || !probe || !hT) return BDOF_ERR_ARG;
    if (!c->have_physics) return fail(c, BDOF_ERR_STATE, "bdof_set_physics has not been called");
    if (c->det_mode == BDOF_DET_NEAR && !hdetT) return fail(c, BDOF_ERR_ARG, "hdetT required for BDOF_DET_NEAR");
    int r = admit(c, "a carrier field (bdof_set_probe_field)", CARRIES_BINNING | CARRIES_MODES | NO_DATA_TERM);
    if (r || (r = enter_setter(c, true))) return r;
    const size_t n = (size_t)c->NX * c->NY;
    DevBuf<double2> dp, dh, dhd;
    if ((r = upload(c, dp, probe, n, FRESH)) || (r = upload(c, dh, hT, n, FRESH)) || (hdetT && (r = upload(c, dhd, hdetT, n, FRESH)))) return r;
    c->pstack.reset(); c->pdet.reset(); c->pdetT.reset();
    c->pdet64.reset(); c->pdetT64.reset();
    HIPC(c, c->pstack.alloc(n * (size_t)n_steps(c)));
    HIPC(c, c->pdet.alloc(n));
    HIPC(c, c->pdetT.alloc(n));
    HIPC(c, c->pdet64.alloc(n));
    HIPC(c, c->pdetT64.alloc(n));
    if ((r = build_carrier_field(c, dp, dh, dhd, CarrierField{c->pstack, c->pdet, c->pdetT, c->pdet64, c->pdetT64}))) return r;
    HIPC(c, hipStreamSynchronize(c->stream));         // the temporaries go when this returns: nothing queued may still read them
    // the wave is carried as p_z + eps_z with eps_0 = 0: no probe of its own, no scalar carrier
    HIPC(c, hipMemsetAsync(c->probe, 0, sizeof(cf) * n, c->stream));
    c->a0 = 0.0;
    changed(c, CHANGED_CARRIER_FIELD_F64);
    c->have_probe = true;
    return 0;
}

// Probe modes: M carrier fields, each built as bdof_set_probe_field builds its one.  They live beside the probe of
// bdof_set_probe* (which M = 0 goes back to) and take its place in bdof_forward / bdof_loss_grad while they are in force.
int bdof_set_probe_modes(bdof_ctx* c, int M, const double* probes, const double* hT, const double* hdetT) {
    int r = enter_setter(c, true);
    if (r) return r;
    if (M == 0 || !probes) { changed(c, CHANGED_PROBE_MODES); return 0; }
    if (M < 1 || M > BDOF_MAX_MODES) return fail(c, BDOF_ERR_ARG, "bdof_set_probe_modes: the number of probe modes must be in [1, BDOF_MAX_MODES]");
    if (!hT) return fail(c, BDOF_ERR_ARG, "bdof_set_probe_modes: hT required with the probe modes");
    if (!c->have_physics) return fail(c, BDOF_ERR_STATE, "bdof_set_probe_modes (probe modes) comes after bdof_set_physics");
    if (c->det_mode == BDOF_DET_NEAR && !hdetT) return fail(c, BDOF_ERR_ARG, "bdof_set_probe_modes: hdetT required for BDOF_DET_NEAR");
    if ((r = admit(c, "probe modes (bdof_set_probe_modes)", CARRIES_MODES | NO_DATA_TERM))) return r;
    if ((r = refuse_modes(c, "bdof_set_probe_modes", "probe modes",
                          {&MODE_STREAMING_ONLY, &MODE_RECOMPUTE, &MODE_ADJOINT64, &MODE_NO_GROT, &MODE_CONV, &MODE_RANGE_CARRIER}))) return r;
    const size_t n = (size_t)c->NX * c->NY, nz = (size_t)n_steps(c);
    DevBuf<double2> dp, dh, dhd;
    if ((r = upload(c, dp, probes, n * M, FRESH)) || (r = upload(c, dh, hT, n, FRESH)) || (hdetT && (r = upload(c, dhd, hdetT, n, FRESH)))) return r;
    changed(c, CHANGED_PROBE_MODES);
    HIPC(c, c->m_stack.alloc(n * nz * M));
    HIPC(c, c->m_det64.alloc(n * M));
    const size_t nzero = std::max(n, (size_t)2 * c->S);
    HIPC(c, c->m_zero.alloc(nzero));
    HIPC(c, hipMemsetAsync(c->m_zero, 0, sizeof(cf) * nzero, c->stream));
    for (int m = 0; m < M; ++m) {
        const CarrierField out{c->m_stack + m * nz * n, nullptr, nullptr, c->m_det64 + m * n, nullptr};
        if ((r = build_carrier_field(c, dp + m * n, dh, dhd, out))) { drop_modes(c); return r; }
    }
    HIPC(c, hipStreamSynchronize(c->stream));         // the temporaries go when this returns: nothing queued may still read them
    c->n_modes = M;
    return 0;
}

int bdof_set_object(bdof_ctx* c, const void* vol, long long n_rows, int volNY, const int* tab, int volNX, int n_angles) {
    if (!c || !vol || n_rows < 1) return BDOF_ERR_ARG;
    if (int r = need_configured(c)) return r;
    if (volNY < 1) return fail(c, BDOF_ERR_ARG, "volNY must be >= 1");
    if (tab && (volNX < 1 || n_angles < 1)) return fail(c, BDOF_ERR_ARG, "volNX and n_angles must be >= 1 with a table");
    if (!tab && volNY != c->NY) return fail(c, BDOF_ERR_ARG, "without a rotation table volNY must equal NY");
    c->obj_src = (const float2*)vol;
    c->obj_bound_mod = false;
    c->obj_rows = (size_t)n_rows;
    c->obj.vol = nullptr;
    c->obj.volNY = volNY;
    changed(c, CHANGED_OBJECT);
    c->obj.tab = tab;
    c->obj.volNX = tab ? volNX : c->NX;
    c->obj.S = c->S;
    c->obj.bin = c->bin;
    c->n_angles = tab ? n_angles : 0;
    return 0;
}

int bdof_set_rotation_adjoint(bdof_ctx* c, const int* off, const int* order, int n_dest) {
    if (!c || !off || !order || n_dest < 1) return BDOF_ERR_ARG;
    c->adj_off = off; c->adj_order = order; c->adj_ndest = n_dest;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, c->heavy.alloc((size_t)n_dest + 1));
    return 0;
}

static void set_batch_views(bdof_ctx* c, const int* angle_of_b, const int* xoff, const int* yoff) {
    c->obj.angle_of_b = angle_of_b;
    c->obj.xoff = xoff;
    c->obj.yoff = yoff;
}
// What every batch call does once its arguments have passed: the device, the batch's index arrays, the modulation table for k
static int begin_batch(bdof_ctx* c, const int* angle_of_b, const int* xoff, const int* yoff, float k) {
    HIPC(c, hipSetDevice(c->device));
    set_batch_views(c, angle_of_b, xoff, yoff);
    return ensure_modulation_k(c, k);
}
// the batch's view of the caller's (delta, beta) rows: the float64 paths modulate from the rows, not from the table c->mod
static ObjView rows_view(const bdof_ctx* c, const int* angle_of_b, const int* xoff, const int* yoff) {
    ObjView o = c->obj;
    o.vol = c->obj_src;
    o.angle_of_b = angle_of_b;
    o.xoff = xoff;
    o.yoff = yoff;
    return o;
}

int bdof_forward(bdof_ctx* c, int B, const int* angle_of_b, const int* xoff, const int* yoff, void* out_wave, int keep_tape) {
    int r;
    if ((r = check_ready(c, B)) || (r = need_angles(c, angle_of_b))) return r;
    if (keep_tape && !c->with_grad) return fail(c, BDOF_ERR_STATE, "keep_tape needs bdof_configure(with_grad=1)");
    if (keep_tape && c->recompute) return fail(c, BDOF_ERR_STATE, "the per-slice history is not kept in tape-free (recompute) mode");
    if (c->n_modes && keep_tape) return fail(c, BDOF_ERR_STATE, "the per-slice history is not kept under probe modes");
    if (c->n_modes && (r = check_modes_batch(c, B))) return r;
    if ((r = begin_batch(c, angle_of_b, xoff, yoff, c->k_fft))) return r;
    if (c->n_modes) {
        changed(c, TAPE_OVERWRITTEN);
        return modes_forward(c, B, out_wave);
    }
    if (use_resident(c, B) && !keep_tape) {
        if ((r = resident_run(c, B, nullptr, out_wave, false))) return r;
        changed(c, TAPE_OVERWRITTEN);
        return 0;
    }
    if (c->generic) {
        if (keep_tape) return fail(c, BDOF_ERR_STATE, "the per-slice history is not kept by the generic-size engine");
        if ((r = generic_forward(c, B, out_wave, false))) return r;
        changed(c, TAPE_OVERWRITTEN);
        return launched(c);
    }
    Split split;
    if ((r = split.open(c, B, c->NX, 16))) return r;
    forward_sweep(c, split, keep_tape ? TAPE_HISTORY : TAPE_NONE);
    if ((r = split.close(c))) return r;
    tape_holds(c, keep_tape != 0, false);
    const DetRoute dr = det_route(c);
    const Group all = whole(c, B);
    if (out_wave && c->planes > 1) {
        for (int j = 0; j < c->planes; ++j) launch_loss_plane(c, all, wave_plane(c, carrier_det(c, j)), j, (cf*)out_wave, nullptr);
    } else if (out_wave) {
        const DetPlane det = wave_plane(c, carrier_det(c), dr.pfield);
        if (dr.far) launch_loss_far(c, all, det, dr.in, nullptr, (cf*)out_wave, nullptr, 1.f, 1.f);
        else launch_loss_real(c, all, det, dr.in, nullptr, false, (cf*)out_wave, nullptr, dr.in_scale, 1.f);
    }
    if (keep_tape && c->variant != BDOF_VARIANT_TF_ALL) {
        // probe_array[S-1] = phi_{S-1} (np_funcs.py:41-43): keep R phi_{S-1} in L1 order in bufA
        if (!(c->det_mode == BDOF_DET_NONE)) {
            const size_t fld = (size_t)c->Bmax * c->NX * c->NY;
            const int nz = n_steps(c);
            const cf* in = nz > 1 ? c->tape + (size_t)(nz - 2) * fld : nullptr;   // psi_hat_{S-1}
            launch_row_fwd(c, all, nz - 1, in, c->bufA, false);
        }
        tape_holds(c, true, true);
    }
    return launched(c);
}

// The range sweep behind bdof_forward_range (h = c->hs: the ctx's slice step, in its dithered copies) and bdof_forward_range_h
// (h: the caller's table for every transfer-function step of the range).
static int forward_range(bdof_ctx* c, int B, const int* angle_of_b, const int* xoff, const int* yoff, int z0, int nz,
                         const void* in_real, void* out_real, int prop_last, const cf* h) {
    int r = check_ready(c, B);
    if (r) return r;
    if (!in_real || !out_real) return BDOF_ERR_ARG;
    if ((r = check_range(c, z0, nz))) return r;
    if (c->generic) return fail(c, BDOF_ERR_SIZE, "bdof_forward_range runs on the fused streaming kernels (NY, NX powers of two in 64..1024)");
    if ((r = need_angles(c, angle_of_b))) return r;
    if (c->range_car && (B != c->range_car_B || z0 != c->range_car_z0))
        return fail(c, BDOF_ERR_ARG, "the range carriers (bdof_set_range_carrier) were handed over for another batch / first slice");
    if ((r = begin_batch(c, angle_of_b, xoff, yoff, c->k_fft))) return r;
    Split split;
    if ((r = split.open(c, B, c->NX, 16))) return r;
    for (int z = z0; z < z0 + nz; ++z) {
        const bool step = z < z0 + nz - 1 || prop_last;
        for (const Group& g : split) {
            launch_row_fwd(c, g, z, c->bufB, c->bufA, step, nullptr, z == z0 ? (const cf*)in_real : nullptr);
            if (step) launch_row_prop(c, g, c->bufA, c->bufB, h, 1.f, 0, z);
        }
    }
    // real-space wave after the range: psi_{z0+nz} (prop_last) or phi_{z0+nz-1}
    const int zl = z0 + nz - 1;
    for (const Group& g : split) {
        if (prop_last)
            launch_loss_real(c, g, wave_plane(c, carrier_z(c, zl + 1), zl + 1 < c->S ? slice_carrier_field(c, zl + 1) : c->pdet),
                             c->bufB, nullptr, false, (cf*)out_real, nullptr, 1.f, 1.f);
        else
            launch_loss_real(c, g, wave_plane(c, carrier_z(c, zl) * (1.0 + c->cbm1), slice_carrier_field(c, zl)),
                             c->bufA, nullptr, false, (cf*)out_real, nullptr, 1.f / c->NY, 1.f);
    }
    if ((r = split.close(c))) return r;
    changed(c, TAPE_OVERWRITTEN);
    return launched(c);
}

int bdof_forward_range(bdof_ctx* c, int B, const int* angle_of_b, const int* xoff, const int* yoff, int z0, int nz,
                       const void* in_real, void* out_real, int prop_last) {
    if (int r = admit(c, "bdof_forward_range", NO_DATA_TERM)) return r;
    if (!c) return BDOF_ERR_ARG;
    return forward_range(c, B, angle_of_b, xoff, yoff, z0, nz, in_real, out_real, prop_last, c->hs);
}

// Carrier fields for the NEXT bdof_forward_range calls over slices z0 .. z0 + nz - 1 of B wavefields: stack [nz][B][NX][NY] complex64
// (device), wavefield b's free-space propagation to the entrance of each of those slices.  The range is then swept on
// psi_z = p_z + eps_z with only eps in the float32 transforms, `in_real` is the scattered part entering the range (zeros when the
// carrier IS the incoming wave) and `out_real` receives the scattered part leaving it — for the tiles of a corrected stitch range
// exactly T psi - T_free psi, without the round-off of two full-amplitude sweeps.  NULL removes the stack.
int bdof_set_range_carrier(bdof_ctx* c, const void* stack, int B, int z0, int nz) {
    if (int r = admit(c, "bdof_set_range_carrier", NO_DATA_TERM)) return r;
    if (!c) return BDOF_ERR_ARG;
    if (!stack) { c->range_car = nullptr; c->range_car_B = 0; return 0; }
    if (int r = need_configured(c)) return r;
    if (c->pstack || c->a0 != std::complex<double>(0.0, 0.0))
        return fail(c, BDOF_ERR_STATE, "range carriers replace the ctx's own probe carrier: bind a zero probe (bdof_set_probe, a0 = 0) and no probe stack");
    if (B < 1 || B > c->Bmax || z0 < 0 || nz < 1 || z0 + nz > c->S) return fail(c, BDOF_ERR_ARG, "batch / slice range outside the configuration");
    c->range_car = (const cf*)stack;
    c->range_car_B = B;
    c->range_car_z0 = z0;
    return 0;
}

int bdof_forward_range_h(bdof_ctx* c, int B, const int* angle_of_b, const int* xoff, const int* yoff, int z0, int nz,
                         const void* in_real, void* out_real, int prop_last, const void* h) {
    if (int r = admit(c, "bdof_forward_range_h", NO_DATA_TERM)) return r;
    if (!c || !h) return BDOF_ERR_ARG;
    return forward_range(c, B, angle_of_b, xoff, yoff, z0, nz, in_real, out_real, prop_last, (const cf*)h);
}

// real-space fields [b][x][y] -> R (transposed, L2): what a transfer-function launch takes
// (defined at the kernel's first use in the file, where the inline launches stood: templates are instantiated in the order of
// first use, and hipcc commutes a few additions in six kernels when that order changes — MEASUREMENTS.md, device-code check)
static void launch_real_to_hyb(bdof_ctx* c, const Group& g, const cf* in, cf* out) {
    RealToHybArgs a{sub_field(c, g, in), sub_field(c, g, out), g.B, c->NX, c->twY};
    DISPATCH_N(c->NY, { hipLaunchKernelGGL((k_row_real_to_hyb<N_>), dim3(rows_grid<N_>(c, g.B, c->NX)), dim3(BDOF_THREADS), 0, g.st, a); });
}

// Adjoint of bdof_forward_range(prop_last = 1) in the tape-free form: the forward wave is marched back from the range's end
// state beside the adjoint field.  end_real: psi_{z0+nz} (what bdof_forward_range returned), g_end_real: G(psi_{z0+nz});
// g_start_real receives G(psi_{z0}); the gradient rows of the range go to grot_range [B][nz][NX][NY] (pairs).
int bdof_adjoint_range(bdof_ctx* c, int B, const int* angle_of_b, const int* xoff, const int* yoff, int z0, int nz,
                       const void* end_real, const void* g_end_real, void* g_start_real, void* grot_range) {
    if (int r = admit(c, "bdof_adjoint_range", NO_DATA_TERM)) return r;
    int r = check_ready(c, B);
    if (r) return r;
    if (!end_real || !g_end_real || !g_start_real || !grot_range) return BDOF_ERR_ARG;
    if ((r = check_range(c, z0, nz))) return r;
    if (c->generic) return fail(c, BDOF_ERR_SIZE, "bdof_adjoint_range runs on the fused streaming kernels");
    if (!c->with_grad || !c->tape) return fail(c, BDOF_ERR_STATE, "bdof_adjoint_range needs bdof_configure(with_grad=1)");
    if (c->S < 2) return fail(c, BDOF_ERR_SIZE, "bdof_adjoint_range needs at least two tape fields (S >= 2)");
    if ((r = need_angles(c, angle_of_b))) return r;
    if ((r = begin_batch(c, angle_of_b, xoff, yoff, c->k_fft))) return r;
    const size_t fld = (size_t)c->Bmax * c->NX * c->NY;
    cf* const rc1 = c->tape;                       // marched-back phi_hat_z (L1)
    cf* const rc2 = c->tape + fld;                 // R eps(psi_z) (L2)
    Split split;
    if ((r = split.open(c, B, c->NX, 16))) return r;
    const int zt = z0 + nz - 1;
    for (const Group& g : split) {
        // phi_{zt} = P^H psi_{zt+1} and G(phi_{zt}) = P^H G(psi_{zt+1}): real space -> R (transposed) -> adjoint step
        launch_real_to_hyb(c, g, (const cf*)end_real, c->bufA);
        launch_row_prop(c, g, c->bufA, rc1, c->hs, 1.f, 1, zt);
        launch_real_to_hyb(c, g, (const cf*)g_end_real, c->bufA);
        launch_row_prop(c, g, c->bufA, c->bufB, c->hs, 1.f, 1, zt);
    }
    for (int z = zt; z >= z0; --z) {
        for (const Group& g : split) {
            GradTarget gt;
            gt.grot = (float2*)grot_range; gt.S_ = nz; gt.z_ = z - z0;
            gt.gpsi = z == z0 ? (cf*)g_start_real : nullptr;
            march_back(c, g, z, 3, rc1, false, z > z0, z > z0, rc1, rc2, &gt);
        }
    }
    if ((r = split.close(c))) return r;
    changed(c, TAPE_OVERWRITTEN);
    changed(c, PROBE_GRADIENT_GONE);
    return launched(c);
}

// loss = mean((|field| - meas)^2) over n = FX * FY pixels (left on the device, bdof_get_loss) and, in place of the field,
// the adjoint seed 2 (|d| - m) d / |d| / n — the detector-less (free_prop_cm None) loss of a whole field
int bdof_field_loss_seed(bdof_ctx* c, void* field, const float* meas, int FX, int FY) {
    if (!c || !field || !meas || FX < 1 || FY < 1) return BDOF_ERR_ARG;
    if (!c->partial) return fail(c, BDOF_ERR_STATE, "bdof_configure has not been called");
    if (int r = admit(c, "bdof_field_loss_seed", CARRIES_BINNING | CARRIES_PLANES | CARRIES_MODES)) return r;      // (a whole field: no sweep, no detector step)
    HIPC(c, hipSetDevice(c->device));
    const size_t n = (size_t)FX * FY;
    const int egrid = g_elem_grid(c, n);
    DetPlane det;                               // no carrier: the field is the whole wave
    det.seed_scale = (float)(2.0 / (double)n);
    GLossArgs la = g_loss_args(c, 1, det, (cf*)field, nullptr, meas);
    la.NX = FX;                                 // a field of its own shape, in real space
    la.NY = FY;
    la.far = 0;
    hipLaunchKernelGGL(k_g_loss<false>, dim3(egrid), dim3(256), 0, c->stream, la);
    hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, c->stream, c->partial, egrid, 1.0 / (double)n, c->loss_dev);
    return launched(c);
}

int bdof_tiles_gather(bdof_ctx* c, const void* field, int FX, int FY, void* tiles, int B, int TX, int TY, const int* x0, const int* y0,
                      int taper) {
    return launch_tiles(c, field, tiles, TILE_GRID, k_tiles_cut<cf, cf>, TileArgs<cf, cf>{(cf*)field, (cf*)tiles, nullptr, x0, y0, B, FX, FY, TX, TY, 0, 0, taper, 0});
}

int bdof_tiles_scatter(bdof_ctx* c, const void* tiles, void* field, int FX, int FY, int B, int TX, int TY, const int* x0, const int* y0,
                       int halo_x, int halo_y) {
    return launch_tiles(c, field, tiles, TILE_GRID, k_tiles_put<cf, cf>, TileArgs<cf, cf>{(cf*)field, (cf*)tiles, nullptr, x0, y0, B, FX, FY, TX, TY, halo_x, halo_y, 0, 0});
}

// adjoint of bdof_tiles_scatter: tiles = the field on every tile's core, zero elsewhere
int bdof_tiles_scatter_adjoint(bdof_ctx* c, const void* field, int FX, int FY, void* tiles, int B, int TX, int TY, const int* x0, const int* y0,
                               int halo_x, int halo_y) {
    return launch_tiles(c, field, tiles, TILE_GRID, k_tiles_put_adjoint<cf, cf>, TileArgs<cf, cf>{(cf*)field, (cf*)tiles, nullptr, x0, y0, B, FX, FY, TX, TY, halo_x, halo_y, 0, 0});
}

// adjoint of bdof_tiles_gather: field = sum of the tiles' pixels, weighted with the taper, at the positions they were cut from
int bdof_tiles_gather_adjoint(bdof_ctx* c, const void* tiles, void* field, int FX, int FY, int B, int TX, int TY, const int* x0, const int* y0,
                              int taper) {
    return launch_tiles(c, field, tiles, FIELD_GRID, k_tiles_cut_adjoint<cf, cf>, TileArgs<cf, cf>{(cf*)field, (cf*)tiles, nullptr, x0, y0, B, FX, FY, TX, TY, 0, 0, taper, 0});
}

// object gradient of a slice range of tiles, added into the volume gradient rows (see k_tiles_grad_add)
int bdof_tiles_grad_add(bdof_ctx* c, const void* grot_range, void* gvol, int B, int TX, int TY, const int* x0, const int* y0, int z0, int nz) {
    if (!c || !grot_range || !gvol || !x0 || !y0 || B < 1) return BDOF_ERR_ARG;
    if (!c->obj.tab) return fail(c, BDOF_ERR_STATE, "bdof_set_object with a table has not been called");
    if (int r = check_range(c, z0, nz)) return r;
    HIPC(c, hipSetDevice(c->device));
    TileGradArgs a{(const float2*)grot_range, (float2*)gvol, c->obj.tab, x0, y0, B, TX, TY, c->obj.volNX, c->obj.volNY, z0, nz, 1};
    hipLaunchKernelGGL(k_tiles_grad_add, dim3(std::min(c->obj.volNX, c->ncu * 8)), dim3(256), 0, c->stream, a);
    return launched(c);
}

// ---- whole-field / tile-batch operations in either precision (bdof_field.h) ------------------------------------------------
// fields[b] <- F^-1 ( h * F fields[b] ) for B fields [NX][NY] in place; h[kx][ky] carries 1 / (NX NY) (and any power of the
// transfer function: np_funcs.py:42 composes in free space); is_double: complex128 fields and table, else complex64
int bdof_fields_free_step(bdof_ctx* c, void* fields, int B, int NX, int NY, const void* h, int conj_h, int is_double) {
    if (!c || !fields || !h || B < 1 || NX < 1 || NY < 1) return BDOF_ERR_ARG;
    HIPC(c, hipSetDevice(c->device));
    if (int r = free_step(c, c->fft, c->stream, fields, B, NX, NY, h, H_KXKY, conj_h, is_double != 0)) return r;
    return launched(c);
}

// The same step on an AUXILIARY stream: it starts after everything queued on the ctx's stream so far (first copying `src` into
// `fields` there, if given) and runs beside what the ctx's stream is handed next — the whole-field step of a stitch range beside the
// tiles' carrier steps and sweeps (tiling.TiledPropagator).  bdof_aux_join makes the ctx's stream wait for it.  One step in
// flight at a time; own rocFFT execution info and work buffer.
int bdof_fields_free_step_aux(bdof_ctx* c, void* fields, const void* src, int B, int NX, int NY, const void* h, int conj_h, int is_double) {
    if (!c || !fields || !h || B < 1 || NX < 1 || NY < 1) return BDOF_ERR_ARG;
    if (c->aux_pending) return fail(c, BDOF_ERR_STATE, "an auxiliary step is in flight: bdof_aux_join first");
    HIPC(c, hipSetDevice(c->device));
    rocfft_plan pf, pi;
    int r = field_plans(c, NX, NY, B, is_double != 0, &pf, &pi);
    if (r) return r;
    if (!c->aux) {
        HIPC(c, hipStreamCreateWithFlags(&c->aux, hipStreamNonBlocking));
        HIPC(c, hipEventCreateWithFlags(&c->ev_aux_fork, hipEventDisableTiming));
        HIPC(c, hipEventCreateWithFlags(&c->ev_aux_join, hipEventDisableTiming));
    }
    size_t w1 = 0, w2 = 0;
    RFC(c, rocfft_plan_get_work_buffer_size(pf, &w1));
    RFC(c, rocfft_plan_get_work_buffer_size(pi, &w2));
    if ((r = fft_exec_room(c, c->fft_aux, c->aux, std::max(w1, w2)))) return r;
    const size_t n = (size_t)NX * NY * B, esz = is_double ? sizeof(double2) : sizeof(float2);
    HIPC(c, hipEventRecord(c->ev_aux_fork, c->stream));
    HIPC(c, hipStreamWaitEvent(c->aux, c->ev_aux_fork, 0));
    c->aux_pending = true;
    if (src) HIPC(c, hipMemcpyAsync(fields, src, n * esz, hipMemcpyDeviceToDevice, c->aux));
    if ((r = free_step(c, c->fft_aux, c->aux, fields, B, NX, NY, h, H_KXKY, conj_h, is_double != 0))) return r;
    return launched(c);
}

// The carrier stack of a stitch range (bdof_set_range_carrier) in one call: p0 [B][NX][NY] complex128 (device; overwritten) are
// the wavefields entering the range; stack [nz][B][NX][NY] complex64 receives p_z = F^-1(H^z F p0), z = 0 .. nz - 1 — the
// free-space propagation of each to the entrance of every slice of the range, formed in double: one forward transform, the nz - 1
// spectra s_hat H^z by a running product, ONE batched inverse transform of all of them, one conversion.  h: complex128 [kx][ky],
// ifftshift(H) / (NX NY).
int bdof_range_carrier_build(bdof_ctx* c, void* p0, void* stack, int B, int NX, int NY, const void* h, int nz) {
    if (int r = admit(c, "bdof_range_carrier_build", NO_DATA_TERM)) return r;
    if (!c || !p0 || !stack || !h || B < 1 || NX < 1 || NY < 1 || nz < 1) return BDOF_ERR_ARG;
    HIPC(c, hipSetDevice(c->device));
    const size_t per = (size_t)NX * NY, n = per * B;
    hipLaunchKernelGGL(k_f_to_float, dim3(g_elem_grid(c, n)), dim3(256), 0, c->stream, (const double2*)p0, (cf*)stack, n);
    if (nz > 1) {
        const size_t need = n * (size_t)(nz - 1);
        if (c->car_scratch.size() < need) {
            HIPC(c, hipStreamSynchronize(c->stream));
            HIPC(c, c->car_scratch.alloc(need));
        }
        rocfft_plan pf, pi, qf, qi;
        // the two plan pairs share c->fft's work area, which only grows: after the second call it has room for both
        int r = field_plans(c, NX, NY, B, true, &pf, &pi);
        if (r) return r;
        if ((r = field_plans(c, NX, NY, B * (nz - 1), true, &qf, &qi))) return r;
        void* b0[1] = {p0};
        RFC(c, rocfft_execute(pf, b0, nullptr, c->fft.info));
        hipLaunchKernelGGL(k_carrier_spectra, dim3(g_elem_grid(c, n)), dim3(256), 0, c->stream, (const double2*)p0, (const double2*)h, c->car_scratch,
                           per, B, nz, (double)NX * (double)NY);
        void* b1[1] = {c->car_scratch};
        RFC(c, rocfft_execute(qi, b1, nullptr, c->fft.info));
        hipLaunchKernelGGL(k_f_to_float, dim3(g_elem_grid(c, need)), dim3(256), 0, c->stream, (const double2*)c->car_scratch, (cf*)stack + n, need);
    }
    return launched(c);
}

int bdof_aux_join(bdof_ctx* c) {
    if (!c) return BDOF_ERR_ARG;
    if (!c->aux_pending) return 0;
    HIPC(c, hipSetDevice(c->device));
    c->aux_pending = false;
    HIPC(c, hipEventRecord(c->ev_aux_join, c->aux));
    HIPC(c, hipStreamWaitEvent(c->stream, c->ev_aux_join, 0));
    return 0;
}

// y += alpha x on n complex numbers (either precision)
int bdof_caxpy(bdof_ctx* c, void* y, const void* x, double alpha, size_t n, int is_double) {
    if (!c || !y || !x) return BDOF_ERR_ARG;
    HIPC(c, hipSetDevice(c->device));
    if (is_double) hipLaunchKernelGGL(k_f_axpy<double>, dim3(g_elem_grid(c, 2 * n)), dim3(256), 0, c->stream, (double*)y, (const double*)x, alpha, 2 * n);
    else hipLaunchKernelGGL(k_f_axpy<float>, dim3(g_elem_grid(c, 2 * n)), dim3(256), 0, c->stream, (float*)y, (const float*)x, (float)alpha, 2 * n);
    return launched(c);
}

// complex64 <-> complex128 copies of n numbers
int bdof_c_convert(bdof_ctx* c, void* dst, const void* src, size_t n, int to_double) {
    if (!c || !dst || !src) return BDOF_ERR_ARG;
    HIPC(c, hipSetDevice(c->device));
    if (to_double) hipLaunchKernelGGL(k_f_to_double, dim3(g_elem_grid(c, n)), dim3(256), 0, c->stream, (const cf*)src, (double2*)dst, n);
    else hipLaunchKernelGGL(k_f_to_float, dim3(g_elem_grid(c, n)), dim3(256), 0, c->stream, (const double2*)src, (cf*)dst, n);
    return launched(c);
}

int bdof_tiles_gather_f64(bdof_ctx* c, const void* field, int FX, int FY, void* tiles, int B, int TX, int TY, const int* x0, const int* y0,
                          int taper) {
    return launch_tiles(c, field, tiles, TILE_GRID, k_tiles_cut<double2, double2>,
                        TileArgs<double2, double2>{(double2*)field, (double2*)tiles, nullptr, x0, y0, B, FX, FY, TX, TY, 0, 0, taper, 0});
}

int bdof_tiles_scatter_f64(bdof_ctx* c, const void* tiles, void* field, int FX, int FY, int B, int TX, int TY, const int* x0, const int* y0,
                           int halo_x, int halo_y) {
    return launch_tiles(c, field, tiles, TILE_GRID, k_tiles_put<double2, double2>,
                        TileArgs<double2, double2>{(double2*)field, (double2*)tiles, nullptr, x0, y0, B, FX, FY, TX, TY, halo_x, halo_y, 0, 0});
}

// complex64 tiles cut out of a complex128 field (tapered, periodic) / written back into it:
// field[core] = (accumulate ? field[core] : 0) + tiles_a - tiles_b (tiles_b nullable), the sum formed in float64
int bdof_tiles_gather_mixed(bdof_ctx* c, const void* field64, int FX, int FY, void* tiles, int B, int TX, int TY, const int* x0, const int* y0,
                            int taper) {
    return launch_tiles(c, field64, tiles, TILE_GRID, k_tiles_cut<double2, cf>,
                        TileArgs<double2, cf>{(double2*)field64, (cf*)tiles, nullptr, x0, y0, B, FX, FY, TX, TY, 0, 0, taper, 0});
}

// adjoint of bdof_tiles_scatter_diff64 w.r.t. tiles_a: complex64 tiles = the complex128 field on every tile's core, zero elsewhere
int bdof_tiles_scatter_adjoint_mixed(bdof_ctx* c, const void* field64, int FX, int FY, void* tiles, int B, int TX, int TY, const int* x0,
                                     const int* y0, int halo_x, int halo_y) {
    return launch_tiles(c, field64, tiles, TILE_GRID, k_tiles_put_adjoint<double2, cf>,
                        TileArgs<double2, cf>{(double2*)field64, (cf*)tiles, nullptr, x0, y0, B, FX, FY, TX, TY, halo_x, halo_y, 0, 0});
}

// adjoint of bdof_tiles_gather_mixed, on a difference of tiles: field64 (+)= sum of the tapered (tiles_a - tiles_b) pixels at the
// positions they were cut from (periodically); tiles_b nullable
int bdof_tiles_gather_adjoint_diff64(bdof_ctx* c, const void* tiles_a, const void* tiles_b, void* field64, int FX, int FY, int B, int TX, int TY,
                                     const int* x0, const int* y0, int taper, int accumulate) {
    return launch_tiles(c, field64, tiles_a, FIELD_GRID, k_tiles_cut_adjoint<double2, cf>,
                        TileArgs<double2, cf>{(double2*)field64, (cf*)tiles_a, (const cf*)tiles_b, x0, y0, B, FX, FY, TX, TY, 0, 0, taper, accumulate});
}

int bdof_tiles_scatter_diff64(bdof_ctx* c, const void* tiles_a, const void* tiles_b, void* field64, int FX, int FY, int B, int TX, int TY,
                              const int* x0, const int* y0, int halo_x, int halo_y, int accumulate) {
    return launch_tiles(c, field64, tiles_a, TILE_GRID, k_tiles_put<double2, cf>,
                        TileArgs<double2, cf>{(double2*)field64, (cf*)tiles_a, (const cf*)tiles_b, x0, y0, B, FX, FY, TX, TY, halo_x, halo_y, 0, accumulate});
}

// ---- the float64 model: one sweep under bdof_forward_range_f64 and the two twins ------------------------------------------------
// What the models that run it differ in: the step behind a slice, and what the real-space model does to the exit wave in front
// of the detector.  Each hook runs forward on the wave or, adj, as its adjoint on the wave's gradient, in place.
struct Model64 {
    double k;                                  // 2 pi dz / lambda
    bool step_last;                            // a step follows the last slice of the range as well
    std::function<int(bool adj)> step;
    std::function<int(bool adj)> exit_wave;    // (empty: none)
};
// psi [B][NX][NY] complex128 on the ctx's stream (first the probe broadcast into it, if given) through slices z0 .. z0 + nz - 1 of
// the object seen through o; tape (nullable): [nz][B][NX][NY], receives the modulated waves.  meas == null: that is all.  Else the
// ctx's detector and data term follow (loss for bdof_get_loss) and the adjoint sweep down the tape: gradient rows in bdof_grot.
static int sweep_f64(bdof_ctx* c, const Model64& m, const ObjView& o, int B, double2* psi, const double2* probe, int z0, int nz, double2* tape,
                     const float* meas, double meas_ref) {
    const int NX = c->NX, NY = c->NY;
    const size_t per = (size_t)NX * NY, n = per * B;
    const int eg = g_elem_grid(c, n);
    int r;
    rocfft_plan pf = nullptr, pi = nullptr;                                    // the far-field detector's transforms
    if (meas && (r = field_plans(c, NX, NY, B, true, &pf, &pi))) return r;
    if (probe) hipLaunchKernelGGL(k_c64_bcast, dim3(eg), dim3(256), 0, c->stream, probe, psi, B, per);
    for (int z = z0; z < z0 + nz; ++z) {
        Mod64Args ma{psi, o, B, NX, NY, z, m.k, tape ? tape + (size_t)(z - z0) * n : nullptr};
        hipLaunchKernelGGL(k_f64_modulate, dim3(eg), dim3(256), 0, c->stream, ma);
        if ((z < z0 + nz - 1 || m.step_last) && (r = m.step(false))) return r;
    }
    if (!meas) return 0;
    if (m.exit_wave && (r = m.exit_wave(false))) return r;
    const bool far = c->det_mode == BDOF_DET_FAR, near = c->det_mode == BDOF_DET_NEAR;
    void* buf[1] = {psi};
    if (near) { if ((r = free_step(c, c->fft, c->stream, psi, B, NX, NY, c->c64_hdet, H_KXKY, 0, true))) return r; }
    else if (far) RFC(c, rocfft_execute(pf, buf, nullptr, c->fft.info));       // un-shifted, un-normalised fft2
    const int lgrid = std::min(eg, c->npartial);
    with_bool(loss_is_poisson(c), [&](auto PSN) { with_bool((bool)c->wgt, [&](auto WGT) {
        hipLaunchKernelGGL((k_c64_loss<PSN, WGT>), dim3(lgrid), dim3(256), 0, c->stream, psi, meas, c->partial, B, NX, NY, far ? 1 : 0, meas_ref, 2.0 / (double)n,
                           c->loss_mu, (const float*)c->wgt);
    }); });
    hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, c->stream, c->partial, lgrid, 1.0 / (double)n, c->loss_dev);
    if (near) { if ((r = free_step(c, c->fft, c->stream, psi, B, NX, NY, c->c64_hdet, H_KXKY, 1, true))) return r; }
    else if (far) RFC(c, rocfft_execute(pi, buf, nullptr, c->fft.info));       // F^H: the un-normalised inverse
    if (m.exit_wave && (r = m.exit_wave(true))) return r;
    for (int z = z0 + nz - 1; z >= z0; --z) {
        if ((z < z0 + nz - 1 || m.step_last) && (r = m.step(true))) return r;
        C64BwdArgs ba{psi, tape + (size_t)(z - z0) * n, c->grot, o, B, NX, NY, c->S, z, m.k};
        hipLaunchKernelGGL(k_c64_bwd, dim3(eg), dim3(256), 0, c->stream, ba);
    }
    changed(c, TAPE_OVERWRITTEN);
    changed(c, PROBE_GRADIENT_GONE);
    return 0;
}

// bdof_forward_range in float64 on caller-owned complex128 fields [B][NX][NY], in place: slices z0 .. z0+nz-1 of the bound object
// seen through the windows (xoff, yoff); modulation from the caller's (delta, beta) rows with k in float64, transforms by
// rocFFT in double precision, h[kx][ky] = the transfer function / (NX NY) in float64.  cnn_propagator/np_funcs.py:36-43.
int bdof_forward_range_f64(bdof_ctx* c, int B, const int* angle_of_b, const int* xoff, const int* yoff, int z0, int nz, void* fields,
                           const void* h, double k, int prop_last) {
    if (int r = admit(c, "bdof_forward_range_f64", NO_DATA_TERM)) return r;
    if (!c || !fields || !h) return BDOF_ERR_ARG;
    if (int r = need_configured(c)) return r;
    if (!c->obj_src) return fail(c, BDOF_ERR_STATE, "bdof_set_object (with (delta, beta) rows) has not been called");
    if (B < 1) return fail(c, BDOF_ERR_ARG, "batch size must be positive");
    int r;
    if ((r = check_range(c, z0, nz)) || (r = need_angles(c, angle_of_b))) return r;
    HIPC(c, hipSetDevice(c->device));
    const Model64 m{k, prop_last != 0, [&](bool) { return free_step(c, c->fft, c->stream, fields, B, c->NX, c->NY, h, H_KXKY, 0, true); }, nullptr};
    if ((r = sweep_f64(c, m, rows_view(c, angle_of_b, xoff, yoff), B, (double2*)fields, nullptr, z0, nz, nullptr, nullptr, 0.0))) return r;
    return launched(c);
}

// What the two float64 twins ask before they run: a batch of measurements, the twin's own model held (`held`, else `text`), the
// object as (delta, beta) rows, the gradient workspace, a batch within Bmax and its angles
static int ready_f64(bdof_ctx* c, int B, const int* angle_of_b, const float* meas, bool held, const char* text) {
    if (!c || !meas) return BDOF_ERR_ARG;
    if (!held) return fail(c, BDOF_ERR_STATE, text);
    if (!c->obj_src) return fail(c, BDOF_ERR_STATE, "bdof_set_object (with (delta, beta) rows) has not been called");
    if (!c->grot || !c->partial) return fail(c, BDOF_ERR_STATE, "bdof_configure(with_grad = 1) needed");
    if (int r = check_batch(c, B)) return r;
    return need_angles(c, angle_of_b);
}

// ---- the real-space propagator in float64 (bdof_conv64.h) -------------------------------------------------------------------
// Buffers of the float64 paths for B wavefields: the wave, the tape of S slices and, for the real-space model, the renormalised
// exit wave and the padded grid.  Allocated when the model is handed over (for Bmax), so that a device without room for them says
// so at set-up and not in the middle of a run.
static int c64_room(bdof_ctx* c, int B, bool tf, size_t M) {
    const size_t n = (size_t)c->NX * c->NY * B;
    const bool have = c->c64_B >= B && c->c64_psi && c->c64_tape && (tf || (c->c64_q && c->c64_big));
    if (have) return 0;
    HIPC(c, hipStreamSynchronize(c->stream));
    c->c64_psi.reset(); c->c64_q.reset(); c->c64_big.reset(); c->c64_tape.reset();      // all four go before any comes back
    c->c64_B = 0;
    HIPC(c, c->c64_psi.alloc(n));
    HIPC(c, c->c64_tape.alloc((size_t)c->S * n));
    if (!tf) {
        HIPC(c, c->c64_q.alloc(n));
        HIPC(c, c->c64_big.alloc(M * M * (size_t)B));
    }
    c->c64_B = B;
    return 0;
}

// probe: host complex128 [NX][NY]; khat: host complex128 [M][M], M = NX + ks - 1 = NY + ks - 1, the 2-D transform of the ks x ks
// kernel zero-padded to M x M, transposed to [kx][ky] and divided by M^2; ksum = sum of the kernel's taps (the padding constant's
// recursion, propagation.py:91,99); k = 2 pi dz / lambda with numpy's pi (propagation.py:25)
int bdof_set_conv_f64(bdof_ctx* c, const double* probe, const double* khat, int ks, double ksum_re, double ksum_im, double k) {
    if (int r = admit(c, "bdof_set_conv_f64", NO_DATA_TERM)) return r;
    if (!c || !probe || !khat) return BDOF_ERR_ARG;
    int r = enter_setter(c, true);
    if (r) return r;
    if (c->NX != c->NY) return fail(c, BDOF_ERR_SIZE, "the float64 real-space path takes square wavefields");
    if (ks < 1 || ks % 2 == 0 || ks >= c->NX) return fail(c, BDOF_ERR_ARG, "kernel_size must be odd and smaller than the field");
    const size_t n = (size_t)c->NX * c->NY, M = (size_t)c->NX + ks - 1;
    if (c->c64_ks != ks) {
        c->c64_khat.reset(); c->c64_big.reset();
        c->c64_B = 0;
    }
    if (!c->c64_scal) HIPC(c, c->c64_scal.alloc(2));
    if (!c->c64_part) HIPC(c, c->c64_part.alloc((size_t)c->ncu * 16));
    if ((r = upload(c, c->c64_probe, probe, n, KEEP)) || (r = upload(c, c->c64_khat, khat, M * M, KEEP))) return r;
    twin64_holds(c, false, ks);
    c->c64_ksum = std::complex<double>(ksum_re, ksum_im);
    c->c64_k = k;
    return c64_room(c, c->Bmax, false, M);
}

// the step to a detector at a finite distance for the float64 real-space path (propagation.py:122-127: one transfer-function
// step of the renormalised exit wave): hdetT host complex128 [kx][ky], ifftshift(H_det) / (NX NY); NULL removes it
int bdof_set_conv_f64_detector(bdof_ctx* c, const double* hdetT) {
    if (int r = admit(c, "bdof_set_conv_f64_detector", NO_DATA_TERM)) return r;
    if (int r = enter_setter(c, true)) return r;
    if (!hdetT) { c->c64_hdet.reset(); return 0; }
    return upload(c, c->c64_hdet, hdetT, (size_t)c->NX * c->NY, KEEP);
}

// bdof_loss_grad_conv with every quantity in float64: loss left for bdof_get_loss, gradient rows in the ctx's rotated-frame
// buffer (bdof_grot) like every other engine, so bdof_rotation_adjoint / bdof_window_rotation_adjoint follow unchanged.
// meas: device float, laid out as for bdof_loss_grad_conv (far field: [b][ky][kx] un-shifted, else [b][x][y]); meas_ref: what
// the host subtracted from the amplitudes (bdof_set_meas_mode 1), 0 otherwise.  Detector: none, far field, or near field after
// bdof_set_conv_f64_detector.
int bdof_loss_grad_conv_f64(bdof_ctx* c, int B, const int* angle_of_b, const int* xoff, const int* yoff, const float* meas, double meas_ref) {
    if (int r = admit(c, "bdof_loss_grad_conv_f64", CARRIES_NOTHING)) return r;
    int r = ready_f64(c, B, angle_of_b, meas, c && c->c64_ks && !c->c64_tf, "bdof_set_conv_f64 has not been called");
    if (r) return r;
    if (c->det_mode == BDOF_DET_NEAR && !c->c64_hdet)
        return fail(c, BDOF_ERR_STATE, "near-field detector: bdof_set_conv_f64_detector has not been called");
    HIPC(c, hipSetDevice(c->device));
    const int N = c->NX, ks = c->c64_ks, p = (ks - 1) / 2, M = N + ks - 1;
    const size_t n = (size_t)N * N * B, nbig = (size_t)M * M * B;
    if ((r = c64_room(c, B, false, (size_t)M))) return r;
    const int eg = g_elem_grid(c, n), egb = g_elem_grid(c, nbig);
    double2 *psi = c->c64_psi, *big = c->c64_big;
    std::complex<double> edge(1.0, 0.0);
    Model64 m{c->c64_k, true};
    // constant pad, valid convolution on the padded grid, crop; adjoint: embed, circular correlation, crop to the un-padded pixels
    m.step = [&](bool adj) -> int {
        hipLaunchKernelGGL(k_c64_pad, dim3(egb), dim3(256), 0, c->stream, psi, big, B, N, M, adj ? ks - 1 : p, adj ? make_double2(0.0, 0.0) : d2(edge));
        if (int e = free_step(c, c->fft, c->stream, big, B, M, M, c->c64_khat, H_KXKY, adj, true)) return e;
        hipLaunchKernelGGL(k_c64_crop, dim3(eg), dim3(256), 0, c->stream, big, psi, B, N, M, adj ? p : ks - 1);
        if (!adj) edge *= c->c64_ksum;
        return 0;
    };
    // q = s P, s = psi_0[0,0,0] / P[0,0,0] (one scalar for the batch), kept in c64_q; adjoint: through the corner pixel
    m.exit_wave = [&](bool adj) -> int {
        const int dgrid = std::min(eg, c->ncu * 16);
        if (adj) {
            hipLaunchKernelGGL(k_c64_dot, dim3(dgrid), dim3(256), 0, c->stream, psi, c->c64_q, n, c->c64_part);
            hipLaunchKernelGGL(k_c64_scale, dim3(eg), dim3(256), 0, c->stream, psi, n, c->c64_scal, 1);
            hipLaunchKernelGGL(k_c64_corner_adj, dim3(1), dim3(1), 0, c->stream, psi, c->c64_part, dgrid, c->c64_scal);
            return 0;
        }
        double2 init;
        HIPC(c, hipMemcpyAsync(&init, c->c64_probe, sizeof(double2), hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipStreamSynchronize(c->stream));
        hipLaunchKernelGGL(k_c64_corner, dim3(1), dim3(1), 0, c->stream, psi, init, c->c64_scal);
        hipLaunchKernelGGL(k_c64_scale, dim3(eg), dim3(256), 0, c->stream, psi, n, c->c64_scal, 0);
        HIPC(c, hipMemcpyAsync(c->c64_q, psi, n * sizeof(double2), hipMemcpyDeviceToDevice, c->stream));
        return 0;
    };
    if ((r = sweep_f64(c, m, rows_view(c, angle_of_b, xoff, yoff), B, psi, c->c64_probe, 0, c->S, c->c64_tape, meas, meas_ref))) return r;
    return launched(c);
}

// ---- the transfer-function model in float64 on the same context -------------------------------------------------------------
// probe: host complex128 [NX][NY]; hT / hdetT (nullable: no near-field detector step): host complex128 [kx][ky], the
// ifftshift-ed transfer functions / (NX NY); k = 2 pi dz / lambda as bdof_set_physics has it
int bdof_set_tf_f64(bdof_ctx* c, const double* probe, const double* hT, const double* hdetT, double k) {
    if (int r = admit(c, "bdof_set_tf_f64", NO_DATA_TERM)) return r;
    if (!c || !probe || !hT) return BDOF_ERR_ARG;
    int r = enter_setter(c, true);
    if (r) return r;
    if (c->det_mode == BDOF_DET_NEAR && !hdetT) return fail(c, BDOF_ERR_ARG, "a near-field detector needs its transfer function in float64 too");
    const size_t n = (size_t)c->NX * c->NY;
    if ((r = upload(c, c->c64_probe, probe, n, KEEP)) || (r = upload(c, c->c64_h, hT, n, KEEP)) ||
        (hdetT && (r = upload(c, c->c64_hdet, hdetT, n, KEEP)))) return r;
    twin64_holds(c, true, 1);
    c->c64_k = k;
    return c64_room(c, c->Bmax, true, 0);
}

// bdof_loss_grad with every quantity in float64 (np_funcs.py:15-65 as autograd differentiates it in the reference: modulation
// from the (delta, beta) rows, F^-1 H F per slice by rocFFT in double, magnitude loss, adjoint sweep): loss for bdof_get_loss,
// gradient rows in bdof_grot.  Unfused — the accuracy path of the first minibatch of an epoch, and a float64 twin of the fused
// kernels on the device.  meas: device float, laid out as for bdof_loss_grad (+ meas_ref under bdof_set_meas_mode(1)).
int bdof_loss_grad_tf_f64(bdof_ctx* c, int B, const int* angle_of_b, const int* xoff, const int* yoff, const float* meas, double meas_ref) {
    if (int r = admit(c, "bdof_loss_grad_tf_f64", NO_DATA_TERM)) return r;
    int r = ready_f64(c, B, angle_of_b, meas, c && c->c64_tf, "bdof_set_tf_f64 has not been called");
    if (r) return r;
    HIPC(c, hipSetDevice(c->device));
    if ((r = c64_room(c, B, true, 0))) return r;
    double2* psi = c->c64_psi;
    const Model64 m{c->c64_k, step_after_last(c),
                    [&](bool adj) { return free_step(c, c->fft, c->stream, psi, B, c->NX, c->NY, c->c64_h, H_KXKY, adj, true); }, nullptr};
    if ((r = sweep_f64(c, m, rows_view(c, angle_of_b, xoff, yoff), B, psi, c->c64_probe, 0, c->S, c->c64_tape, meas, meas_ref))) return r;
    return launched(c);
}

int bdof_tape_to_real(bdof_ctx* c, int i, int B, void* out) {
    int r = check_ready(c, B);
    if (r) return r;
    if (!out) return BDOF_ERR_ARG;
    if (!c->tape_valid) return fail(c, BDOF_ERR_STATE, "no history: run bdof_forward(keep_tape=1) first");
    const int nz = n_steps(c);
    if (i < 0 || i >= nz) return fail(c, BDOF_ERR_ARG, "slice index outside [0, S / slice binning)");
    const size_t fld = (size_t)c->Bmax * c->NX * c->NY;
    if (i < nz - 1) {
        launch_loss_real(c, whole(c, B), wave_plane(c, carrier_z(c, i + 1), slice_carrier_field(c, i + 1)), c->tape + (size_t)i * fld, nullptr, false,
                         (cf*)out, nullptr, 1.f, 1.f);
    } else {
        if (!c->last_valid)
            return fail(c, BDOF_ERR_STATE, "the last slice's wave is only kept after bdof_forward(keep_tape=1) with the numpy_skip_last variant");
        launch_loss_real(c, whole(c, B), wave_plane(c, carrier_z(c, nz - 1) * (1.0 + c->cbm1), slice_carrier_field(c, nz - 1)), c->bufA, nullptr, false,
                         (cf*)out, nullptr, 1.f / c->NY, 1.f);
    }
    return launched(c);
}

int bdof_loss_grad(bdof_ctx* c, int B, const int* angle_of_b, const int* xoff, const int* yoff, const float* meas, void* out_wave) {
    int r = check_ready(c, B);
    if (r) return r;
    if (!meas) return BDOF_ERR_ARG;
    if (c->meas_dev && (c->det_mode == BDOF_DET_FAR || c->pstack || c->n_modes))
        return fail(c, BDOF_ERR_STATE, "bdof_set_meas_mode(1) needs a real-space detector and a scalar carrier (not a carrier field, not probe modes)");
    if (!c->with_grad || !c->grot) return fail(c, BDOF_ERR_STATE, "bdof_loss_grad needs bdof_configure(with_grad=1) with the gradient workspace (not flag 32)");
    if ((r = need_angles(c, angle_of_b))) return r;
    if (c->n_modes && (r = check_modes_batch(c, B))) return r;
    if ((r = begin_batch(c, angle_of_b, xoff, yoff, c->k_fft))) return r;
    c->gpsi_src = c->gpsi0;
    c->gpsi_B = B;
    c->fused_last = c->adj_fused_last = 0;
    if (c->n_modes) {
        changed(c, TAPE_OVERWRITTEN);
        return modes_loss_grad(c, B, meas, out_wave);
    }
    if (use_resident(c, B)) {
        if ((r = resident_run(c, B, meas, out_wave, true))) return r;
        changed(c, TAPE_OVERWRITTEN);
        return 0;
    }
    if (c->generic) {
        if ((r = generic_loss_grad(c, B, meas, out_wave))) return r;
        changed(c, TAPE_OVERWRITTEN);
        c->gpsi_src = c->bufA;                  // the adjoint sweep ends with G(psi_0) in the field buffer, [b][x][y]
        return launched(c);
    }
    Split split;
    if ((r = split.open(c, B, c->NX, 16))) return r;
    const bool fused = fused_mode(c) != 0;
    const bool adj_fused = fused && c->adj_fusion != 0;
    c->fused_last = fused ? 1 : 0;
    c->adj_fused_last = adj_fused ? 1 : 0;
    forward_sweep(c, split, c->recompute ? TAPE_LAST : TAPE_HISTORY, fused, adj_fused);
    changed(c, TAPE_OVERWRITTEN);      // the tape holds an incomplete history (or phi_{S-1} alone), not what bdof_tape_to_real expects
    int npart = 0;
    // Detector + seed.  Afterwards bufB holds g_hat(phi_{S-1}) (L1 order, normalised hybrid).
    const DetRoute dr = det_route(c);
    const bool per_tile = loss_tiles_fit(c, B, dr.far);      // (loss_grid)
    for (const Group& g : split) {
        if (c->planes > 1) {
            // one real-space detector launch per plane on det_pl, the seeds (transposed) to seed_pl, then the fan-in to bufB
            for (int j = 0; j < c->planes; ++j)
                npart += launch_loss_plane(c, g, det_plane(c, g, B, nullptr, j), j, (cf*)out_wave, meas, npart);
            launch_row_planes(c, g, true, n_steps(c) - 1, fused ? BDOF_K_LOSS : BDOF_K_COL_PROP);
            continue;
        }
        const DetPlane det = det_plane(c, g, B, dr.pfield);      // the whole batch's seed scale
        if (dr.far) {
            npart += launch_loss_far(c, g, det, dr.in, c->bufB, (cf*)out_wave, meas, 1.f, 1.f, npart, per_tile);
        } else if (!dr.h) {
            npart += launch_loss_real(c, g, det, dr.in, c->bufB, false, (cf*)out_wave, meas, dr.in_scale, dr.in_scale, npart, per_tile);
        } else {
            // the detector wave came out of a transfer-function step: seed -> R (transposed) -> adjoint step
            npart += launch_loss_real(c, g, det, dr.in, c->bufA, true, (cf*)out_wave, meas, 1.f, 1.f, npart, per_tile);
            launch_row_prop(c, g, c->bufA, c->bufB, dr.h, 1.f, 1, n_steps(c) - 1, fused ? BDOF_K_LOSS : BDOF_K_COL_PROP);
        }
    }
    adjoint_sweep(c, split, fused, adj_fused);
    if ((r = split.close(c))) return r;
    hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, c->stream, c->partial, npart,
                       1.0 / ((double)B * c->planes * c->NX * c->NY), c->loss_dev);
    return launched(c);
}


// =================================================================================================
// Real-space truncated-kernel propagator (cnn_propagator/propagation.py:18-133)
// =================================================================================================
int bdof_set_conv(bdof_ctx* c, const float* ky, const float* kx, int ks, double e_re, double e_im, double ksum_re,
                  double ksum_im, double k) {
    if (int r = admit(c, "bdof_set_conv", NO_DATA_TERM)) return r;
    if (!c || !ky || !kx) return BDOF_ERR_ARG;
    if (int r = enter_setter(c, false)) return r;
    if (ks < 1 || ks > BDOF_CONV_MAXK || ks % 2 == 0) return fail(c, BDOF_ERR_ARG, "kernel_size must be odd and <= 33");
    if (c->generic || c->NX % BDOF_CONV_TX || c->NY % BDOF_CONV_TY)
        return fail(c, BDOF_ERR_SIZE, "the conv propagator needs power-of-two wavefields (tiles are 32 x 64)");
    changed(c, CHANGED_CONV_TAPS);
    for (int i = 0; i < ks; ++i) {
        c->taps.ky[i] = make_float2(ky[2 * i], ky[2 * i + 1]);
        c->taps.kx[i] = make_float2(kx[2 * i], kx[2 * i + 1]);
    }
    c->taps.e = make_float2((float)e_re, (float)e_im);
    c->taps.ks = ks;
    c->ksum = std::complex<double>(ksum_re, ksum_im);
    c->k_conv = (float)k;
    const size_t fld = (size_t)c->Bmax * c->NX * c->NY;
    if (!c->bufC) HIPC(c, c->bufC.alloc(fld));
    if (!c->conv_scal) HIPC(c, c->conv_scal.alloc(4));
    HIPC(c, hipStreamSynchronize(c->stream));                  // a sweep still in flight reads the previous taps
    if (c->taps_copies != 1) c->taps_dev.reset();
    c->taps_copies = 1;
    if (int r = upload(c, c->taps_dev, &c->taps, 1, KEEP)) return r;
    c->have_conv = true;
    return 0;
}

int bdof_set_conv_taps_f64(bdof_ctx* c, const double* ky, const double* kx, double e_re, double e_im) {
    if (int r = admit(c, "bdof_set_conv_taps_f64", NO_DATA_TERM)) return r;
    if (!c || !ky || !kx) return BDOF_ERR_ARG;
    if (!c->have_conv) return fail(c, BDOF_ERR_STATE, "bdof_set_conv has not been called");
    const int D = c->tw_dither;
    if (D < 2) return 0;                                       // BDOF_TW_DITHER=0: the nearest-rounded taps of bdof_set_conv stay
    if (int r = enter_setter(c, false)) return r;
    std::vector<ConvTaps> t((size_t)D, c->taps);
    const int ks = c->taps.ks;
    for (int d = 0; d < D; ++d) {
        for (int i = 0; i < ks; ++i) {
            // a phase of its own for each of the 4 ks + 2 numbers (golden-ratio sequence), as for the twiddle tables
            const double ph = 0.6180339887498949 * (4 * i + 1);
            t[d].ky[i] = make_float2(dither_pick(ky[2 * i], d, std::fmod(ph, 1.0)), dither_pick(ky[2 * i + 1], d, std::fmod(ph + 0.6180339887498949, 1.0)));
            t[d].kx[i] = make_float2(dither_pick(kx[2 * i], d, std::fmod(ph + 2 * 0.6180339887498949, 1.0)),
                                     dither_pick(kx[2 * i + 1], d, std::fmod(ph + 3 * 0.6180339887498949, 1.0)));
        }
        t[d].e = make_float2(dither_pick(e_re, d, 0.25), dither_pick(e_im, d, 0.75));
    }
    HIPC(c, hipStreamSynchronize(c->stream));                  // a sweep still in flight reads the previous taps
    if (int r = upload(c, c->taps_dev, t.data(), (size_t)D, FRESH)) return r;
    c->taps_copies = D;
    return 0;
}

}  // extern "C"  (helpers below have C++ linkage)

static cf conv_carrier(const bdof_ctx* c, int z) {        // a_z = a_0 sum(K)^z
    const std::complex<double> a = c->a0 * std::pow(c->ksum, z);
    return make_float2((float)a.real(), (float)a.imag());
}
static cf conv_pad(const bdof_ctx* c, int z) {            // padding constant of eps: edge_val_z - a_z = (1 - a_0) sum(K)^z
    const std::complex<double> a = (1.0 - c->a0) * std::pow(c->ksum, z);
    return make_float2((float)a.real(), (float)a.imag());
}

static int conv_lds_bytes(const bdof_ctx* c) {
    const int h = (c->taps.ks - 1) / 2;
    const int TXH = BDOF_CONV_TX + 2 * h, TYH = BDOF_CONV_TY + 2 * h;
    return (TXH * (TYH | 1) + TXH * (BDOF_CONV_TY + 1)) * (int)sizeof(cf);
}

// BDOF_CONV_TILING=1 keeps the first tiling (k_conv, 32 x 64 tiles through staging registers) for every size; read at every
// launch so that one process can run both (tests/test_gpu_conv.py compares them)
static int conv_tiling() {
    const char* e = getenv("BDOF_CONV_TILING");
    return e && e[0] == '1' ? 1 : 2;
}

template <bool BWD, int H, bool PF> static int launch_conv_hp(bdof_ctx* c, ConvArgs& a, ProfScope& ps) {      // on ps.st
    if constexpr (H == 2 || H == 4 || H == 8) {
        // second tiling (bdof_conv2.h): 64 x 32 tiles by LDS-DMA, static LDS, two workgroups per CU by registers
        if (conv_tiling() != 1 && a.NX % Conv2Cfg<H>::TX == 0 && a.NY % Conv2Cfg<H>::TY == 0) {
            // 8 runs of strips (bdof_conv2.h, XCD-aware order), nwg workgroups each: as few rounds as the workgroups per CU
            // allow, and the workgroup count that fills the last round best
            auto plan = [&](int tx, int per_cu) {
                const int nstrips = a.B * (a.NX / tx);
                const int run_tiles = ((nstrips + 7) / 8) * (a.NY / Conv2Cfg<H>::TY);
                const int slots = std::max(1, c->ncu * per_cu / 8);
                const int rounds = (run_tiles + slots - 1) / slots;
                return 8 * ((run_tiles + rounds - 1) / rounds);
            };
            BDOF_LAUNCH(ps, (k_conv2<BWD, H, PF>), dim3(plan(Conv2Cfg<H>::TX, 2)), dim3(Conv2Cfg<H>::THREADS), 0, ps.st, a);
            return 0;
        }
    }
    if (int r = max_lds_once<k_conv<BWD, H, PF>>(c, 160 * 1024 - 1024)) return r;
    const int tiles = a.B * (a.NX / BDOF_CONV_TX) * (a.NY / BDOF_CONV_TY);
    const int grid = balanced_grid(c, tiles, 2);
    BDOF_LAUNCH(ps, (k_conv<BWD, H, PF>), dim3(grid), dim3(BDOF_CONV_THREADS), conv_lds_bytes(c), ps.st, a);
    return 0;
}

// one slice of the conv sweeps on g's stream; `a` addresses g's wavefields already
template <bool BWD> static int launch_conv(bdof_ctx* c, const Group& g, ConvArgs& a) {
    ProfScope ps(c, BWD ? BDOF_K_ROW_BWD : BDOF_K_ROW_FWD, g.st, true);
    // register-window fast paths for the common kernel sizes 5, 9, 17, 33 (H = 2, 4, 8, 16 = 2^L), the generic window H = 0 otherwise
    const int h = (c->taps.ks - 1) / 2;
    const int log_h = h == 2 ? 1 : h == 4 ? 2 : h == 8 ? 3 : h == 16 ? 4 : 0;
    return with_int<5>(log_h, [&](auto L) { return with_bool(a.pfield != nullptr, [&](auto PF) {
        return launch_conv_hp<BWD, (L ? 1 << L : 0), PF>(c, a, ps);
    }); });
}

// the conv sweeps' sub-batches: tiles of 32 x 32 pixels, two workgroups per CU
static int conv_split(bdof_ctx* c, int B, Split* split) { return split->open(c, B, (c->NX / 32) * (c->NY / 32), 2); }

// forward sweep of the conv propagator; leaves psi_S (eps part) in bufB and the scalars in conv_scal
static int conv_forward_sweep(bdof_ctx* c, int B, bool tape) {
    const size_t fld = (size_t)c->Bmax * c->NX * c->NY;
    const size_t n = (size_t)B * c->NX * c->NY, plane = (size_t)c->NX * c->NY;
    const int egrid = g_elem_grid(c, n);
    const bool cs = c->cstack != nullptr;           // carrier field: eps is the scattered wave alone, padded with zeros
    const cf zero = make_float2(0.f, 0.f);
    ObjView obj = c->obj;
    cf* cur = tape ? c->tape : c->bufA;
    ConvInitArgs ia{c->probe, cur, obj, B, c->NX, c->NY, conv_carrier(c, 0), cs ? c->cstack : nullptr};
    hipLaunchKernelGGL(k_conv_init, dim3(egrid), dim3(256), 0, c->stream, ia);
    int r;
    // sub-batches on streams of their own, as on the transfer-function path (Split): the ramp and tail of one group's
    // launch are filled by the other's; the slices of a group follow each other on its stream, the groups meet again at the
    // detector (the renormalisation reads batch element 0)
    Split split;
    if ((r = conv_split(c, B, &split))) return r;
    for (const Group& g : split) {
        const size_t off = (size_t)g.b0 * plane;
        const ObjView gobj = sub_obj(c, g);
        cf* gcur = cur;
        for (int z = 0; z < c->S; ++z) {
            const bool last = z == c->S - 1;
            cf* out = last ? c->bufB : (tape ? c->tape + (size_t)(z + 1) * fld : (gcur == c->bufA ? c->bufC : c->bufA));
            ConvArgs a{gcur + off, out + off, nullptr, nullptr, gobj, g.B, c->NX, c->NY, last ? -1 : z + 1, cs ? zero : conv_pad(c, z),
                       conv_carrier(c, z + 1), c->k_conv, c->taps_dev + z % c->taps_copies, c->taps.ks,
                       cs && !last ? c->cstack + (size_t)(z + 1) * plane : nullptr};
            if ((r = launch_conv<false>(c, g, a))) return r;
            gcur = out;
        }
    }
    if ((r = split.close(c))) return r;
    hipLaunchKernelGGL(k_conv_scalars, dim3(1), dim3(64), 0, c->stream, c->bufB, cs ? cfl(c->c_pS) : conv_carrier(c, c->S), c->probe,
                       cs ? cfl(c->c_p0) : conv_carrier(c, 0), c->conv_scal);
    return 0;
}

// The one read-back of the conv path: the corner pixel (batch element 0) of each of the device fields `dev` (two at the most), to
// float64 scalars on the host; 8 bytes each and one drain of the ctx stream for all of them
static int conv_corner(bdof_ctx* c, std::initializer_list<const cf*> dev, std::complex<double>* out) {
    cf px[2];
    int i = 0;
    for (const cf* d : dev) HIPC(c, hipMemcpyAsync(&px[i++], d, sizeof(cf), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    for (int j = 0; j < i; ++j) out[j] = std::complex<double>(px[j].x, px[j].y);
    return 0;
}
// carrier field: the renormalisation s = p_0[0,0] / (p_S[0,0] + eps_S[0,0,0]) in float64
static int conv_scale64(bdof_ctx* c, double2* s64) {
    std::complex<double> e0;
    if (int r = conv_corner(c, {c->bufB}, &e0)) return r;
    const std::complex<double> sd = c->c_p0 / (c->c_pS + e0);
    *s64 = make_double2(sd.real(), sd.imag());
    return 0;
}

static int conv_check(bdof_ctx* c, int B, const int* angle_of_b) {
    int r = check_ready(c, B);
    if (r) return r;
    if (!c->have_conv) return fail(c, BDOF_ERR_STATE, "bdof_set_conv has not been called");
    return need_angles(c, angle_of_b);
}

// k_conv_final over B wavefields: q = s (a_S + eps) into `out`.  With a carrier field, or residual splitting (`split`), the
// constant a_S stays out and only the scattered part s eps is formed.
static ConvFinalArgs conv_final_args(bdof_ctx* c, int B, const cf* psi_eps, cf* out, bool split) {
    ConvFinalArgs fa{};
    fa.psi_eps = psi_eps;
    fa.out = out;
    fa.scal = c->conv_scal;
    fa.carrier_end = (split || c->cstack) ? make_float2(0.f, 0.f) : conv_carrier(c, c->S);
    fa.plane = (size_t)c->NX * c->NY;
    fa.n = (size_t)B * fa.plane;
    return fa;
}

// The detector stage of the conv path behind a real-space (near) or far-field detector, from eps_S in bufB: the renormalised wave
// through the detector transforms to out_wave and, with meas, the data term (returns the number of partial sums) and its seed
// back to real space, scaled, in *seed.  bdof_forward_conv is bdof_loss_grad_conv without meas.  The detector transforms see no
// scalar carrier (the renormalised wave carries its own; under residual splitting — meas with bdof_set_meas_mode(1) — det does).
// Carrier field: only the scattered part s eps_S goes through them in float32; the carrier's detector plane comes in float64,
// times s (det.pfield64, det.pscale).
static int conv_detector(bdof_ctx* c, int B, const DetPlane& det, const float* meas, cf* out_wave, cf** seed) {
    const size_t n = (size_t)B * c->NX * c->NY;
    const int egrid = g_elem_grid(c, n);
    const ConvFinalArgs fa = conv_final_args(c, B, c->bufB, c->bufA, meas && c->meas_dev != 0);
    hipLaunchKernelGGL((k_conv_final<0>), dim3(egrid), dim3(256), 0, c->stream, fa);
    const Group all = whole(c, B);
    launch_real_to_hyb(c, all, c->bufA, c->bufC);
    int npart;
    if (c->det_mode == BDOF_DET_NEAR) {
        // the detector step and its adjoint take copy 0 of the dithered constants, whatever ran on the ctx before
        launch_row_prop(c, all, c->bufC, c->bufA, c->hdet, 1.f, 0, 0);                                               // d_hat (L1)
        npart = launch_loss_real(c, all, det, c->bufA, meas ? (cf*)c->bufC : nullptr, meas != nullptr, out_wave, meas, 1.f, 1.f);
        if (meas) launch_row_prop(c, all, c->bufC, c->bufA, c->hdet, 1.f, 1, 0);                                     // g_hat(q) (L1)
    } else {
        npart = launch_loss_far(c, all, det, c->bufC, meas ? (cf*)c->bufA : nullptr, out_wave, meas, 1.f, 1.f);      // g_hat(q) (L1)
    }
    if (!meas) return 0;
    launch_loss_real(c, all, DetPlane{}, c->bufA, nullptr, false, c->bufC, nullptr, 1.f, 1.f);        // G(q), real space
    hipLaunchKernelGGL(k_conv_scale_seed, dim3(egrid), dim3(256), 0, c->stream, c->bufC, c->conv_scal, n);
    *seed = c->bufC;
    return npart;
}


extern "C" {

int bdof_set_conv_probe_stack(bdof_ctx* c, const float* stack, const double* det64, double p0_re, double p0_im, double pS_re, double pS_im) {
    if (int r = admit(c, "bdof_set_conv_probe_stack", NO_DATA_TERM)) return r;
    int r = enter_setter(c, true);
    if (r) return r;
    c->cstack.reset();
    c->cdet64.reset();
    changed(c, CHANGED_CONV_CARRIER_FIELD);
    if (!stack && !det64) return 0;
    if (!stack || !det64) return fail(c, BDOF_ERR_ARG, "bdof_set_conv_probe_stack: both arrays or neither");
    if (!c->have_conv) return fail(c, BDOF_ERR_STATE, "bdof_set_conv has not been called");
    const size_t plane = (size_t)c->NX * c->NY;
    if ((r = upload(c, c->cstack, stack, plane * (size_t)(c->S + 1), FRESH)) || (r = upload(c, c->cdet64, det64, plane, FRESH))) return r;
    c->c_p0 = std::complex<double>(p0_re, p0_im);
    c->c_pS = std::complex<double>(pS_re, pS_im);
    return 0;
}

int bdof_forward_conv(bdof_ctx* c, int B, const int* angle_of_b, const int* xoff, const int* yoff, void* out_wave) {
    if (int r = admit(c, "bdof_forward_conv", NO_DATA_TERM)) return r;
    int r = conv_check(c, B, angle_of_b);
    if (r) return r;
    if (!out_wave) return BDOF_ERR_ARG;
    if ((r = begin_batch(c, angle_of_b, xoff, yoff, c->k_conv))) return r;
    if ((r = conv_forward_sweep(c, B, false))) return r;
    changed(c, TAPE_OVERWRITTEN);
    const bool cs = c->cstack != nullptr;
    if (c->det_mode == BDOF_DET_NONE) {
        ConvFinalArgs fa = conv_final_args(c, B, c->bufB, (cf*)out_wave, false);
        fa.pfield = cs ? c->cstack + (size_t)c->S * fa.plane : nullptr;
        hipLaunchKernelGGL((k_conv_final<0>), dim3(g_elem_grid(c, fa.n)), dim3(256), 0, c->stream, fa);
    } else {
        DetPlane det;
        if (cs && (r = conv_scale64(c, &det.pscale))) return r;
        det.pfield64 = cs ? c->cdet64 : nullptr;
        conv_detector(c, B, det, nullptr, (cf*)out_wave, nullptr);
    }
    return launched(c);
}

int bdof_loss_grad_conv(bdof_ctx* c, int B, const int* angle_of_b, const int* xoff, const int* yoff, const float* meas, void* out_wave) {
    if (int r = admit(c, "bdof_loss_grad_conv", CARRIES_NOTHING)) return r;
    int r = conv_check(c, B, angle_of_b);
    if (r) return r;
    if (!meas) return BDOF_ERR_ARG;
    // residual splitting at the detector (bdof_set_meas_mode(1): meas holds m - |a_0|), real-space detectors: the renormalised
    // wave is kept as A + e', A = s a_S a float64 scalar formed on the host from the corner pixel, and |A + e'| - m is
    // evaluated without the cancellation of two numbers of size one (seed_split) — as on the transfer-function path
    const bool split = c->meas_dev != 0;
    if (split && (c->det_mode == BDOF_DET_FAR || std::abs(c->a0) == 0.0))
        return fail(c, BDOF_ERR_STATE, "bdof_set_meas_mode(1) needs a plane-wave carrier and a real-space detector");
    if (!c->with_grad) return fail(c, BDOF_ERR_STATE, "bdof_loss_grad_conv needs bdof_configure(with_grad=1)");
    changed(c, PROBE_GRADIENT_GONE);         // the real-space propagator does not export the probe gradient
    if ((r = begin_batch(c, angle_of_b, xoff, yoff, c->k_conv))) return r;
    if ((r = conv_forward_sweep(c, B, true))) return r;
    changed(c, TAPE_OVERWRITTEN);
    const size_t fld = (size_t)c->Bmax * c->NX * c->NY;
    const size_t n = (size_t)B * c->NX * c->NY;
    const int egrid = g_elem_grid(c, n);
    const double seed_scale = 2.0 / ((double)B * c->NX * c->NY);
    const cf zero = make_float2(0.f, 0.f);
    cf* gp;
    int npart;
    // The detector plane of the renormalised wave.  From the ctx (det_plane) it keeps the data term only: meas_dev, meas_ref, mu.
    // Everything about the carrier is this path's own — the transfer-function recurrence behind det_plane's carrier, a_end and
    // dref does not describe this wave — and is set or cleared here by name.
    DetPlane det = det_plane(c, whole(c, B), B, nullptr);
    det.seed_scale = (float)seed_scale;
    det.gcar = det.gt0 = nullptr;       // the far-field kernel adds no DC carrier here, so there is no adjoint carrier either
    det.a_end = make_double2(0.0, 0.0);
    det.dref = 0.f;
    set_carrier(det, 0.0);              // split: A (times Hdet[0,0] for the near detector), the constant part of the detector wave
    if (split) {
        std::complex<double> px[2];     // corner pixel of batch element 0: scattered part of psi_S and of the probe
        if ((r = conv_corner(c, {c->bufB, c->probe}, px))) return r;
        const std::complex<double> aS = c->a0 * std::pow(c->ksum, c->S);
        const std::complex<double> sd = (c->a0 + px[1]) / (aS + px[0]);
        std::complex<double> A = sd * aS;
        if (c->det_mode == BDOF_DET_NEAR) A *= c->hdet00;
        set_carrier(det, A);
        if (c->det_mode == BDOF_DET_NONE) det.abs_carrier = (float)std::abs(A);      // k_conv_final: |A| rounded once, from float64
        det.dref = (float)(std::abs(A) - std::abs(c->a0));
    }
    const bool cs = c->cstack != nullptr;
    const size_t plane = (size_t)c->NX * c->NY;
    if (cs) {
        if ((r = conv_scale64(c, &det.pscale))) return r;
        det.pfield64 = c->cdet64;
    }
    if (c->det_mode == BDOF_DET_NONE && cs) {
        // q = s (p_S + eps_S): the scattered part in float32, the residual against s p_S in float64 (seed_f64), seed in place
        const ConvFinalArgs fa = conv_final_args(c, B, c->bufB, c->bufA, split);
        hipLaunchKernelGGL((k_conv_final<0>), dim3(egrid), dim3(256), 0, c->stream, fa);
        det.pfield = c->cstack + (size_t)c->S * plane;
        const GLossArgs la = g_loss_args(c, B, det, c->bufA, (cf*)out_wave, meas);
        hipLaunchKernelGGL(k_g_loss<false>, dim3(egrid), dim3(256), 0, c->stream, la);
        hipLaunchKernelGGL(k_conv_scale_seed, dim3(egrid), dim3(256), 0, c->stream, c->bufA, c->conv_scal, n);
        npart = egrid;
        gp = c->bufA;
    } else if (c->det_mode == BDOF_DET_NONE) {
        ConvFinalArgs fa = conv_final_args(c, B, c->bufB, (cf*)out_wave, split);
        fa.out2 = c->bufA;
        fa.meas = meas;
        fa.partial = c->partial;
        fa.det = det;
        hipLaunchKernelGGL((k_conv_final<1>), dim3(egrid), dim3(256), 0, c->stream, fa);
        npart = egrid;
        gp = c->bufA;
    } else {
        npart = conv_detector(c, B, det, meas, (cf*)out_wave, &gp);
    }
    hipLaunchKernelGGL(k_conv_finish, dim3(1), dim3(256), 0, c->stream, c->partial, npart, 2, 1.0 / ((double)B * c->NX * c->NY),
                       seed_scale, c->loss_dev, gp, c->conv_scal);
    // backward sweep, in the same sub-batches
    Split groups;
    if ((r = conv_split(c, B, &groups))) return r;
    for (const Group& g : groups) {
        const size_t off = (size_t)g.b0 * plane;
        const ObjView gobj = sub_obj(c, g);
        cf* gcur = gp;
        for (int z = c->S - 1; z >= 0; --z) {
            cf* gout = gcur == c->bufB ? c->bufA : c->bufB;
            ConvArgs a{gcur + off, gout + off, c->tape + (size_t)z * fld + off, c->grot + (size_t)g.b0 * c->S * plane, gobj, g.B, c->NX, c->NY, z,
                       zero, conv_carrier(c, z), c->k_conv, c->taps_dev + z % c->taps_copies, c->taps.ks, cs ? c->cstack + (size_t)z * plane : nullptr};
            if ((r = launch_conv<true>(c, g, a))) return r;
            gcur = gout;
        }
    }
    if ((r = groups.close(c))) return r;
    return launched(c);
}

int bdof_enable_probe_grad(bdof_ctx* c, int enable) {
    if (int r = enter_setter(c, false)) return r;
    if (enable && !c->gpsi0) {
        if (!c->with_grad) return fail(c, BDOF_ERR_STATE, "the probe gradient needs bdof_configure(with_grad=1)");
        HIPC(c, c->gpsi0.alloc((size_t)c->Bmax * c->NX * c->NY));
    } else if (!enable && c->gpsi0) {
        HIPC(c, hipStreamSynchronize(c->stream));
        c->gpsi0.reset();
    }
    changed(c, PROBE_GRADIENT_GONE);
    return 0;
}

int bdof_probe_grad(bdof_ctx* c, void* out, int accumulate) {
    if (!c || !out) return BDOF_ERR_ARG;
    if (!c->gpsi0) return fail(c, BDOF_ERR_STATE, "bdof_enable_probe_grad(1) has not been called");
    if (!c->gpsi_src) return fail(c, BDOF_ERR_STATE, "no gradient sweep since the probe gradient was enabled (bdof_loss_grad first)");
    if (int r = admit(c, "bdof_probe_grad", CARRIES_BINNING | CARRIES_PLANES | NO_DATA_TERM)) return r;      // (bdof_probe_grad_modes)
    HIPC(c, hipSetDevice(c->device));
    const size_t n = (size_t)c->NX * c->NY;
    hipLaunchKernelGGL(k_sum_fields, dim3((unsigned)std::min<size_t>((n + 255) / 256, (size_t)c->ncu * 8)), dim3(256), 0, c->stream, c->gpsi_src,
                       (cf*)out, c->gpsi_B, n, accumulate);
    return launched(c);
}

// the gradient w.r.t. mode m: its sub-batch of G(psi_0) summed over the windows, k_sum_fields per mode
int bdof_probe_grad_modes(bdof_ctx* c, void* out, int accumulate) {
    if (!c || !out) return BDOF_ERR_ARG;
    if (!c->n_modes) return fail(c, BDOF_ERR_STATE, "bdof_probe_grad_modes: no probe modes are set (bdof_set_probe_modes)");
    if (!c->gpsi0) return fail(c, BDOF_ERR_STATE, "bdof_enable_probe_grad(1) has not been called");
    if (!c->gpsi_src) return fail(c, BDOF_ERR_STATE, "no gradient sweep since the probe gradient was enabled (bdof_loss_grad first)");
    HIPC(c, hipSetDevice(c->device));
    const size_t n = (size_t)c->NX * c->NY;
    for (int m = 0; m < c->n_modes; ++m)
        hipLaunchKernelGGL(k_sum_fields, dim3((unsigned)std::min<size_t>((n + 255) / 256, (size_t)c->ncu * 8)), dim3(256), 0, c->stream,
                           c->gpsi_src + modes_sub(c, c->gpsi_B, m), (cf*)out + (size_t)m * n, c->gpsi_B, n, accumulate);
    return launched(c);
}

int bdof_get_loss(bdof_ctx* c, double* loss) {
    if (!c || !loss) return BDOF_ERR_ARG;
    HIPC(c, hipMemcpyAsync(loss, c->loss_dev, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return 0;
}

void* bdof_grot(bdof_ctx* c) { return c ? (void*)c->grot : nullptr; }
void* bdof_tape_slot(bdof_ctx* c, int slot) {
    if (!c || !c->tape || slot < 0) return nullptr;
    const size_t fld = (size_t)c->Bmax * c->NX * c->NY;
    return (size_t)(slot + 1) * fld <= c->tape.size() ? (void*)(c->tape + (size_t)slot * fld) : nullptr;
}

int bdof_modulation_table(bdof_ctx* c, const void** table, size_t* n, double* mean_m1) {
    if (!c || !table || !n) return BDOF_ERR_ARG;
    if (int r = need_configured(c)) return r;
    if (!c->have_physics) return fail(c, BDOF_ERR_STATE, "bdof_set_physics has not been called");
    if (!c->obj_src && !c->obj_bound_mod) return fail(c, BDOF_ERR_STATE, "bdof_set_object has not been called");
    HIPC(c, hipSetDevice(c->device));
    if (int r = ensure_modulation(c)) return r;
    *table = (const float2*)c->mod;
    *n = c->obj_rows * (size_t)c->obj.volNY;
    if (mean_m1) { mean_m1[0] = c->cbm1.real(); mean_m1[1] = c->cbm1.imag(); }
    return 0;
}

int bdof_rotation_adjoint_rows(bdof_ctx* c, int B, const int* angle_of_b, void* gvol, int row0, int n_rows, int accumulate,
                               float scale) {
    if (!c || !gvol || !angle_of_b) return BDOF_ERR_ARG;
    if (!c->grot) return fail(c, BDOF_ERR_STATE, "no gradient workspace (configure with_grad=1)");
    if (!c->adj_off) return fail(c, BDOF_ERR_STATE, "bdof_set_rotation_adjoint has not been called");
    if (int r = check_batch(c, B)) return r;
    if (c->NY % 2) return fail(c, BDOF_ERR_SIZE, "the rotation adjoint needs an even NY");
    if (row0 < 0 || n_rows < 0 || (long long)row0 + n_rows > c->adj_ndest) return fail(c, BDOF_ERR_ARG, "destination rows outside the volume");
    if (n_rows == 0) return 0;
    HIPC(c, hipSetDevice(c->device));
    ProfScope ps(c, BDOF_K_ROT_ADJ, c->stream);
    RotAdjK<false> a;
    static_cast<RotAdjArgs&>(a) = RotAdjArgs{c->grot, (float2*)gvol, c->adj_off, c->adj_order, angle_of_b, B, c->S * c->NX, c->adj_ndest, c->NY,
                                             accumulate, scale, c->heavy, c->heavy + 1, row0, row0 + n_rows};
    HIPC(c, hipMemsetAsync(c->heavy, 0, sizeof(int), c->stream));
    int need = (n_rows + 3) / 4;
    int grid = need < c->ncu * 8 ? need : c->ncu * 8;
    hipLaunchKernelGGL(k_rot_adjoint<false>, dim3(grid), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(k_rot_adjoint_heavy<false>, dim3(c->ncu * 8), dim3(256), 0, c->stream, a);
    return launched(c);
}

int bdof_rotation_adjoint(bdof_ctx* c, int B, const int* angle_of_b, void* gvol, int accumulate, float scale) {
    if (!c) return BDOF_ERR_ARG;
    return bdof_rotation_adjoint_rows(c, B, angle_of_b, gvol, 0, c->adj_ndest, accumulate, scale);
}

}  // extern "C"  (two steps that both window adjoints take)
// the device copy of the batch's one angle, for stage 2
static int window_pad_angle(bdof_ctx* c, int angle) {
    if (!c->win_angle) HIPC(c, c->win_angle.alloc(1));
    HIPC(c, hipMemsetD32Async((hipDeviceptr_t)c->win_angle, angle, 1, c->stream));
    return 0;
}
// stage 2: rotated frame (c->winpad, n_src rows of volNY pairs) -> volume (the full-field rotation adjoint with a batch of one)
static int window_pad_adjoint(bdof_ctx* c, int n_src, int volNY, void* gvol, int accumulate, float scale) {
    RotAdjK<false> r;
    static_cast<RotAdjArgs&>(r) = RotAdjArgs{c->winpad, (float2*)gvol, c->adj_off, c->adj_order, c->win_angle, 1, n_src, c->adj_ndest, volNY,
                                             accumulate, scale, c->heavy, c->heavy + 1, 0, c->adj_ndest};
    HIPC(c, hipMemsetAsync(c->heavy, 0, sizeof(int), c->stream));
    const int needwg = (c->adj_ndest + 3) / 4;
    hipLaunchKernelGGL(k_rot_adjoint<false>, dim3(needwg < c->ncu * 8 ? needwg : c->ncu * 8), dim3(256), 0, c->stream, r);
    hipLaunchKernelGGL(k_rot_adjoint_heavy<false>, dim3(c->ncu * 8), dim3(256), 0, c->stream, r);
    return launched(c);
}
extern "C" {

int bdof_window_rotation_adjoint(bdof_ctx* c, int B, int angle, const int* xoff, const int* yoff, void* gvol,
                                 int accumulate, float scale) {
    if (!c || !gvol || !xoff || !yoff) return BDOF_ERR_ARG;
    if (!c->grot) return fail(c, BDOF_ERR_STATE, "no gradient workspace (configure with_grad=1)");
    if (!c->adj_off || !c->obj.tab) return fail(c, BDOF_ERR_STATE, "rotation tables have not been set");
    if (int r = check_batch(c, B)) return r;
    if (angle < 0 || angle >= c->n_angles) return fail(c, BDOF_ERR_ARG, "angle index outside the rotation tables");
    HIPC(c, hipSetDevice(c->device));
    if (c->obj.volNY % 2) return fail(c, BDOF_ERR_SIZE, "the rotation adjoint needs an even volume NY");
    ProfScope ps(c, BDOF_K_ROT_ADJ, c->stream);
    const int n_src = c->S * c->obj.volNX;
    WinAdjArgs a{c->grot, (float2*)gvol, c->adj_off + (size_t)angle * (c->adj_ndest + 1), c->adj_order + (size_t)angle * n_src,
                 xoff, yoff, B, c->S, c->NX, c->NY, c->obj.volNX, c->obj.volNY, c->adj_ndest, accumulate, scale};
    if (B > BDOF_WIN_MAXLIST) {
        // more windows than the overlap-add kernel lists per column: direct (slow) gather
        int grid = c->adj_ndest < c->ncu * 16 ? c->adj_ndest : c->ncu * 16;
        hipLaunchKernelGGL(k_window_rot_adjoint, dim3(grid), dim3(256), 0, c->stream, a);
        return launched(c);
    }
    const size_t need = (size_t)n_src * c->obj.volNY;
    if (c->winpad.size() < need) {
        HIPC(c, hipStreamSynchronize(c->stream));
        HIPC(c, c->winpad.alloc(need));
    }
    if (int r = window_pad_angle(c, angle)) return r;
    // stage 1: windows -> rotated frame
    const int z_per_wg = 8;
    hipLaunchKernelGGL(k_window_overlap_add, dim3(c->obj.volNX, (c->S + z_per_wg - 1) / z_per_wg), dim3(256), 0, c->stream, a,
                       c->winpad, z_per_wg);
    return window_pad_adjoint(c, n_src, c->obj.volNY, gvol, accumulate, scale);
}

static AdamArgs adam_args(const void* x_old, void* x_new, const void* g, void* m, void* v, const float* mask, int NXv, int NZv, int NYv,
                          float g_scale, float alpha_d, float alpha_b, float gamma, float lr, float b1, float b2, float eps, int i_batch,
                          int clip, int x0, int nx) {
    // b1, b2 arrive as float32 (0.999f = 0.99900001287...); the reference's are Python floats.  The decimal the caller meant is
    // recovered (7 significant digits) so that 1 - b and the bias corrections are those of the float64 reference.
    const double b1d = std::round((double)b1 * 1e7) / 1e7, b2d = std::round((double)b2 * 1e7) / 1e7;
    const double bc1 = 1.0 - std::pow(b1d, (double)(i_batch + 1));
    const double bc2 = 1.0 - std::pow(b2d, (double)(i_batch + 1));
    return AdamArgs{(const float2*)x_old, (float2*)x_new, (const float2*)g, (float2*)m, (float2*)v, mask, NXv, NZv, NYv,
                    g_scale, alpha_d, alpha_b, gamma, lr, (float)b1d, (float)b2d, eps, (float)(1.0 / bc1), (float)(1.0 / bc2),
                    (float)(1.0 - b1d), (float)(1.0 - b2d), clip, x0, x0 + nx};
}

int bdof_adam_step_slab(bdof_ctx* c, const void* x_old, void* x_new, const void* g, void* m, void* v, const float* mask,
                        int NXv, int NZv, int NYv, float g_scale, float alpha_d, float alpha_b, float gamma,
                        float lr, float b1, float b2, float eps, int i_batch, int clip, int x0, int nx) {
    if (!c || !x_old || !x_new || !g || !m || !v) return BDOF_ERR_ARG;
    if (x_old == x_new) return fail(c, BDOF_ERR_ARG, "x_new must not alias x_old (the TV stencil reads pre-update neighbours)");
    if (NXv < 1 || NZv < 1 || NYv < 1 || i_batch < 0) return fail(c, BDOF_ERR_ARG, "bad volume shape / i_batch");
    if (x0 < 0 || nx < 0 || (long long)x0 + nx > NXv) return fail(c, BDOF_ERR_ARG, "slab outside the volume");
    if (nx == 0) return 0;
    HIPC(c, hipSetDevice(c->device));
    ProfScope ps(c, BDOF_K_ADAM, c->stream);
    const AdamArgs a = adam_args(x_old, x_new, g, m, v, mask, NXv, NZv, NYv, g_scale, alpha_d, alpha_b, gamma, lr, b1, b2, eps, i_batch, clip,
                                 x0, nx);
    const size_t n = (size_t)nx * NZv * NYv;
    int grid = g_elem_grid(c, n);
    grid = (grid + 7) / 8 * 8;                       // k_adam deals the range to the 8 XCDs by blockIdx % 8
    hipLaunchKernelGGL(k_adam, dim3(grid), dim3(256), 0, c->stream, a);
    return launched(c);
}

int bdof_adam_step(bdof_ctx* c, const void* x_old, void* x_new, const void* g, void* m, void* v, const float* mask,
                   int NXv, int NZv, int NYv, float g_scale, float alpha_d, float alpha_b, float gamma,
                   float lr, float b1, float b2, float eps, int i_batch, int clip) {
    return bdof_adam_step_slab(c, x_old, x_new, g, m, v, mask, NXv, NZv, NYv, g_scale, alpha_d, alpha_b, gamma, lr, b1, b2, eps,
                               i_batch, clip, 0, NXv);
}

// The tail of a step on one rank in one pass over the volume: bdof_rotation_adjoint_rows + bdof_adam_step + the modulation
// table of x_new (k_rot_adjoint<true>, k_rot_adjoint_heavy<true>, k_sum_chunks + k_sum_mean over the row sums).
int bdof_rotation_adjoint_adam(bdof_ctx* c, int B, const int* angle_of_b, void* gvol, int row0, int n_rows, int accumulate, float scale,
                               const void* x_old, void* x_new, void* m, void* v, const float* mask, int NXv, int NZv, int NYv,
                               float g_scale, float alpha_d, float alpha_b, float gamma, float lr, float b1, float b2, float eps,
                               int i_batch, int clip) {
    if (!c || !angle_of_b || !x_old || !x_new || !m || !v) return BDOF_ERR_ARG;
    if (int r = need_configured(c)) return r;
    const char* who = "bdof_rotation_adjoint_adam";
    if (accumulate) return fail(c, BDOF_ERR_STATE, std::string(who) + " does not carry accumulate: the update needs the whole gradient (bdof_rotation_adjoint_rows, then bdof_adam_step)");
    if (c->obj_bound_mod) return fail(c, BDOF_ERR_STATE, std::string(who) + " does not carry the bilinear rotation (bdof_set_object_bilinear): bdof_rotate_bilinear_adjoint, then bdof_adam_step");
    if (!c->obj_src) return fail(c, BDOF_ERR_STATE, std::string(who) + " needs an object bound as (delta, beta) rows (bdof_set_object)");
    if (!c->grot) return fail(c, BDOF_ERR_STATE, "no gradient workspace (configure with_grad=1)");
    if (!c->adj_off) return fail(c, BDOF_ERR_STATE, "bdof_set_rotation_adjoint has not been called");
    if (row0 != 0 || n_rows != c->adj_ndest) return fail(c, BDOF_ERR_STATE, std::string(who) + " does not carry a row range: it updates the whole volume (bdof_rotation_adjoint_rows, then bdof_adam_step_slab)");
    if (int r = check_batch(c, B)) return r;
    if (c->NY % 2) return fail(c, BDOF_ERR_SIZE, "the rotation adjoint needs an even NY");
    if (x_old == x_new) return fail(c, BDOF_ERR_ARG, "x_new must not alias x_old (the TV stencil reads pre-update neighbours)");
    if (NXv < 1 || NZv < 1 || NYv < 1 || i_batch < 0) return fail(c, BDOF_ERR_ARG, "bad volume shape / i_batch");
    if (NYv != c->NY || (long long)NXv * NZv != c->adj_ndest || c->obj_rows != (size_t)c->adj_ndest || c->obj.volNY != NYv)
        return fail(c, BDOF_ERR_ARG, "the volume must be the bound object's: [NXv][NZv] = the rotation adjoint's destination rows, of NY pairs");
    if (!c->have_physics) return fail(c, BDOF_ERR_STATE, "bdof_set_physics has not been called");
    HIPC(c, hipSetDevice(c->device));
    const size_t n = (size_t)c->adj_ndest * NYv;
    const bool mean = want_cbar(c);
    HIPC(c, c->mod.room(n));
    // row sums [n_dest], their sums chunk by chunk [n_chunks], the mean
    const int chunk = 1024, n_chunks = (c->adj_ndest + chunk - 1) / chunk;
    const size_t mean_at = (size_t)c->adj_ndest + n_chunks;
    if (mean) HIPC(c, c->cbar_dev.room(std::max((size_t)c->ncu * 16, mean_at) + 1));
    // c->mod stops being the bound object's table here
    changed(c, CHANGED_MOD_OVERWRITTEN);
    ProfScope ps(c, BDOF_K_ROT_ADJ, c->stream);
    RotAdjK<true> a;
    static_cast<RotAdjArgs&>(a) = RotAdjArgs{c->grot, (float2*)gvol, c->adj_off, c->adj_order, angle_of_b, B, c->S * c->NX, c->adj_ndest, c->NY,
                                             0, scale, c->heavy, c->heavy + 1, 0, c->adj_ndest};
    a.adam = adam_args(x_old, x_new, nullptr, m, v, mask, NXv, NZv, NYv, g_scale, alpha_d, alpha_b, gamma, lr, b1, b2, eps, i_batch, clip, 0, NXv);
    a.mod = c->mod;
    a.rowsum = mean ? (double2*)c->cbar_dev : nullptr;
    a.k = c->k;
    HIPC(c, hipMemsetAsync(c->heavy, 0, sizeof(int), c->stream));
    const int need = (c->adj_ndest + 3) / 4;
    hipLaunchKernelGGL(k_rot_adjoint<true>, dim3(need < c->ncu * 8 ? need : c->ncu * 8), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(k_rot_adjoint_heavy<true>, dim3(c->ncu * 8), dim3(256), 0, c->stream, a);
    if (mean) {
        hipLaunchKernelGGL(k_sum_chunks, dim3(n_chunks), dim3(256), 0, c->stream, c->cbar_dev, c->adj_ndest, chunk, c->cbar_dev + c->adj_ndest);
        hipLaunchKernelGGL(k_sum_mean, dim3(1), dim3(256), 0, c->stream, c->cbar_dev + c->adj_ndest, n_chunks, 1.0 / (double)n, c->cbar_dev + mean_at);
    }
    if (int r = launched(c)) return r;
    c->mod_for = (const float2*)x_new;
    c->mod_for_rows = (size_t)c->adj_ndest;
    c->mod_for_NY = NYv;
    c->mod_for_mean = mean;
    c->mod_for_mean_at = mean_at;
    return 0;
}

}  // extern "C"  (the host paths below are templates)

// ---- the materialised rotations: bilinear (k_rot_bilinear*) and trilinear under a rigid map per batch element (bdof_rigid.h) ----
// One host path per operation — rotate, bind as modulation factors, adjoint — over a traits struct per kind: the entry points' names
// for the messages, the prm type, the shape rule and the two launches.
// What both kinds bind once their own shape checks have passed: the B rotated objects of
// a (NX, S, NY) volume are bound as modulation factors (there is no (delta, beta) source to rebuild the table from), with room for
// the table and, if the mean-refraction carrier is in use (*mean), for the per-workgroup sums of the pass that fills it.
static int bind_rotated_objects(bdof_ctx* c, int NXv, int NZv, int NYv, int B, int conv, bool* mean) {
    if (NYv != c->NY || NXv != c->NX || NZv != c->S) return fail(c, BDOF_ERR_ARG, "the volume must be (NX, S, NY) of the configured wavefields");
    if (B > c->Bmax) return fail(c, BDOF_ERR_ARG, "batch size outside [1, Bmax]");
    if (conv && !c->have_conv) return fail(c, BDOF_ERR_STATE, "bdof_set_conv has not been called");
    // set the binding first: want_cbar looks at the physics and probe only
    c->obj_src = nullptr;
    c->obj_bound_mod = true;
    c->obj_rows = (size_t)B * NZv * NXv;
    c->obj.volNY = NYv;
    c->obj.tab = nullptr;
    c->obj.volNX = c->NX;
    c->obj.S = c->S;
    c->n_angles = 0;
    c->k = conv ? c->k_conv : c->k_fft;
    changed(c, CHANGED_OBJECT);
    *mean = want_cbar(c);
    return modulation_room(c, c->obj_rows * NYv, *mean);
}

struct RotBilinear {
    using Prm = double4;
    static constexpr const char *rotate = "bdof_rotate_bilinear", *set_object = "bdof_set_object_bilinear", *adjoint = "bdof_rotate_bilinear_adjoint";
    // an even NY: rotated rows are bound as rows of float4 pairs
    static int shape(bdof_ctx* c, const char* who, int NXv, int NZv, int NYv, int) {
        if (NXv < 1 || NZv < 1 || NYv < 2 || NYv % 2) return fail(c, BDOF_ERR_SIZE, std::string(who) + " needs an even NY");
        return 0;
    }
    template <bool MOD> static void forward(bdof_ctx* c, int grid, const RotArgs<Prm>& a, float k, double2* partial) {
        hipLaunchKernelGGL((k_rot_bilinear<MOD>), dim3(grid), dim3(256), 0, c->stream, a, k, partial);
    }
    static int back(bdof_ctx* c, int grid, const RotArgs<Prm>& a) {
        const int nv4 = (a.NYv / 2 + 63) / 64;
        if (nv4 <= 1) hipLaunchKernelGGL((k_rot_bilinear_adjoint<1>), dim3(grid), dim3(256), 0, c->stream, a);
        else if (nv4 <= 2) hipLaunchKernelGGL((k_rot_bilinear_adjoint<2>), dim3(grid), dim3(256), 0, c->stream, a);
        else if (nv4 <= 4) hipLaunchKernelGGL((k_rot_bilinear_adjoint<4>), dim3(grid), dim3(256), 0, c->stream, a);
        else if (nv4 <= 8) hipLaunchKernelGGL((k_rot_bilinear_adjoint<8>), dim3(grid), dim3(256), 0, c->stream, a);
        else return fail(c, BDOF_ERR_SIZE, "bdof_rotate_bilinear_adjoint: NY <= 1024");
        return 0;
    }
};
struct RotRigid {
    using Prm = double;
    static constexpr const char *rotate = "bdof_rotate_rigid", *set_object = "bdof_set_object_rigid", *adjoint = "bdof_rotate_rigid_adjoint",
                                *param_grad = "bdof_rotate_rigid_param_grad";
    // an even NY as for the bilinear kind, and a volume and a rotated batch whose voxel indices the kernels hold in an int
    static int shape(bdof_ctx* c, const char* who, int NXv, int NZv, int NYv, int B) {
        if (int r = RotBilinear::shape(c, who, NXv, NZv, NYv, B)) return r;
        if ((long long)NXv * NZv * NYv > 0x7fffffffLL || (long long)B * NXv * NZv > 0x7fffffffLL)
            return fail(c, BDOF_ERR_SIZE, std::string(who) + ": NX * NZ * NY and B * NX * NZ must be below 2^31");
        return 0;
    }
    template <bool MOD> static void forward(bdof_ctx* c, int grid, const RotArgs<Prm>& a, float k, double2* partial) {
        hipLaunchKernelGGL((k_rot_rigid<MOD>), dim3(grid), dim3(256), 0, c->stream, a, k, partial);
    }
    static int back(bdof_ctx* c, int grid, const RotArgs<Prm>& a) { hipLaunchKernelGGL(k_rot_rigid_adjoint, dim3(grid), dim3(256), 0, c->stream, a); return 0; }
};

template <class K>       // the B rotated objects as plain (delta, beta) rows
static int rotate_rows(bdof_ctx* c, const void* vol, int NXv, int NZv, int NYv, const double* prm, int B, void* out_rows) {
    if (!c || !vol || !prm || !out_rows || B < 1) return BDOF_ERR_ARG;
    if (int r = K::shape(c, K::rotate, NXv, NZv, NYv, B)) return r;
    HIPC(c, hipSetDevice(c->device));
    RotArgs<typename K::Prm> a{(const float2*)vol, (float2*)out_rows, nullptr, (const typename K::Prm*)prm, B, NXv, NZv, NYv, 0, 0, 0, 1.f};
    const size_t nrows = (size_t)B * NZv * NXv;
    const int grid = (int)std::min<size_t>((nrows + 3) / 4, (size_t)c->ncu * 16);
    K::template forward<false>(c, grid, a, 0.f, nullptr);
    return launched(c);
}

// rotate_rows + bdof_set_object in one pass: the B rotated objects are written straight into the ctx's modulation
// table as factors c - 1 (no rotated (delta, beta) copy, no second pass over B volumes) and bound as the batch's objects.
template <class K>
static int set_object_rotated(bdof_ctx* c, const void* vol, int NXv, int NZv, int NYv, const double* prm, int B, int conv) {
    if (int r = admit(c, K::set_object, CARRIES_PLANES | CARRIES_MODES | NO_DATA_TERM)) return r;
    if (!c || !vol || !prm || B < 1) return BDOF_ERR_ARG;
    int r = enter_setter(c, false);
    if (r) return r;
    if ((r = K::shape(c, K::set_object, NXv, NZv, NYv, B))) return r;
    bool mean;
    if ((r = bind_rotated_objects(c, NXv, NZv, NYv, B, conv, &mean))) return r;
    const size_t nrows = c->obj_rows, n = nrows * NYv;
    RotArgs<typename K::Prm> a{(const float2*)vol, c->mod, nullptr, (const typename K::Prm*)prm, B, NXv, NZv, NYv, 0, 0, 0, 1.f};
    const int grid = (int)std::min<size_t>((nrows + 3) / 4, (size_t)c->ncu * 16);
    K::template forward<true>(c, grid, a, c->k, mean ? c->cbar_dev : (double2*)nullptr);
    return modulation_done(c, n, grid, mean);
}

template <class K>
static int rotate_adjoint(bdof_ctx* c, const void* grot, int NXv, int NZv, int NYv, const double* prm, int B, void* gvol, int row0,
                          int n_rows, int accumulate, float scale) {
    if (!c || !grot || !prm || !gvol || B < 1) return BDOF_ERR_ARG;
    if (int r = K::shape(c, K::adjoint, NXv, NZv, NYv, B)) return r;
    if (row0 < 0 || n_rows < 0 || (long long)row0 + n_rows > (long long)NXv * NZv) return fail(c, BDOF_ERR_ARG, "destination rows outside the volume");
    if (n_rows == 0) return 0;
    HIPC(c, hipSetDevice(c->device));
    ProfScope ps(c, BDOF_K_ROT_ADJ, c->stream);
    RotArgs<typename K::Prm> a{nullptr, (float2*)grot, (float2*)gvol, (const typename K::Prm*)prm, B, NXv, NZv, NYv, row0, row0 + n_rows, accumulate, scale};
    if (int r = K::back(c, std::min((n_rows + 3) / 4, c->ncu * 16), a)) return r;
    return launched(c);
}

// dL/d(M | t) of the rigid kind only (bdof_rigid.h): the shape rule of its other three calls, the rotated-frame gradient the
// adjoint would take (grot; nullptr: the ctx's own), per-workgroup float64 records in the ctx's prm_partial, then their sum per b.
static int rigid_param_grad(bdof_ctx* c, const void* vol, const void* grot, int NXv, int NZv, int NYv, const double* prm, int B, double* out,
                            int accumulate) {
    using K = RotRigid;
    if (!c || !vol || !prm || !out || B < 1) return BDOF_ERR_ARG;
    if (int r = K::shape(c, K::param_grad, NXv, NZv, NYv, B)) return r;
    if (!grot) {
        if (!c->grot) return fail(c, BDOF_ERR_STATE, std::string(K::param_grad) + ": the ctx holds no rotated-frame gradient (bdof_grot)");
        if ((size_t)B * NXv * NZv * NYv > c->grot.size()) return fail(c, BDOF_ERR_ARG, std::string(K::param_grad) + ": B rotated objects do not fit bdof_grot");
        grot = (const float2*)c->grot;
    }
    HIPC(c, hipSetDevice(c->device));
    const int P = rigid_param_partials(NXv, NZv);
    HIPC(c, c->prm_partial.room((size_t)B * P * 12));
    RotArgs<K::Prm> a{(const float2*)vol, (float2*)grot, nullptr, prm, B, NXv, NZv, NYv, 0, 0, accumulate, 1.f};
    hipLaunchKernelGGL(k_rot_rigid_param_grad, dim3((unsigned)((size_t)B * P)), dim3(256), 0, c->stream, a, P, (double*)c->prm_partial);
    hipLaunchKernelGGL(k_rot_rigid_param_sum, dim3(B), dim3(64), 0, c->stream, (const double*)c->prm_partial, P, out, accumulate);
    return launched(c);
}

extern "C" {

int bdof_rotate_bilinear(bdof_ctx* c, const void* vol, int NXv, int NZv, int NYv, const double* prm, int B, void* out_rows) {
    return rotate_rows<RotBilinear>(c, vol, NXv, NZv, NYv, prm, B, out_rows);
}
int bdof_set_object_bilinear(bdof_ctx* c, const void* vol, int NXv, int NZv, int NYv, const double* prm, int B, int conv) {
    return set_object_rotated<RotBilinear>(c, vol, NXv, NZv, NYv, prm, B, conv);
}
int bdof_rotate_bilinear_adjoint(bdof_ctx* c, const void* grot, int NXv, int NZv, int NYv, const double* prm, int B, void* gvol, int row0,
                                 int n_rows, int accumulate, float scale) {
    return rotate_adjoint<RotBilinear>(c, grot, NXv, NZv, NYv, prm, B, gvol, row0, n_rows, accumulate, scale);
}
int bdof_rotate_rigid(bdof_ctx* c, const void* vol, int NXv, int NZv, int NYv, const double* prm, int B, void* out_rows) {
    return rotate_rows<RotRigid>(c, vol, NXv, NZv, NYv, prm, B, out_rows);
}
int bdof_set_object_rigid(bdof_ctx* c, const void* vol, int NXv, int NZv, int NYv, const double* prm, int B, int conv) {
    return set_object_rotated<RotRigid>(c, vol, NXv, NZv, NYv, prm, B, conv);
}
int bdof_rotate_rigid_adjoint(bdof_ctx* c, const void* grot, int NXv, int NZv, int NYv, const double* prm, int B, void* gvol, int row0,
                              int n_rows, int accumulate, float scale) {
    return rotate_adjoint<RotRigid>(c, grot, NXv, NZv, NYv, prm, B, gvol, row0, n_rows, accumulate, scale);
}
int bdof_rotate_rigid_param_grad(bdof_ctx* c, const void* vol, const void* grot, int NXv, int NZv, int NYv, const double* prm, int B, double* out,
                                 int accumulate) {
    return rigid_param_grad(c, vol, grot, NXv, NZv, NYv, prm, B, out, accumulate);
}

}  // extern "C"

// ---- ptychography windows at fractional origins (bdof_windows.h) ------------------------------------------------------------------
// The shape rule of the three calls: even NY of the windows and of the volume (rows are bound and summed as float4 pairs), and a
// rotated frame and a window batch whose row indices the kernels hold in an int.
static int window_shape(bdof_ctx* c, const char* who, int volNX, int volNY, int B) {
    if (volNX < 1 || volNY < 1) return fail(c, BDOF_ERR_ARG, std::string(who) + ": bad volume shape");
    if (c->NY % 2 || volNY % 2) return fail(c, BDOF_ERR_SIZE, std::string(who) + " needs an even NY of the windows and of the volume");
    if ((long long)volNX * c->S * volNY > 0x7fffffffLL || (long long)B * c->S * c->NX > 0x7fffffffLL)
        return fail(c, BDOF_ERR_SIZE, std::string(who) + ": volNX * S * volNY and B * S * NX must be below 2^31");
    return 0;
}
// the window-frame gradient a call reads: the caller's, or the ctx's own
static int window_grot(bdof_ctx* c, const char* who, const void*& grot, int B) {
    if (grot) return 0;
    if (!c->grot) return fail(c, BDOF_ERR_STATE, std::string(who) + ": the ctx holds no gradient workspace (bdof_grot)");
    if ((size_t)B * c->S * c->NX * c->NY > c->grot.size()) return fail(c, BDOF_ERR_ARG, std::string(who) + ": B windows do not fit bdof_grot");
    grot = (const float2*)c->grot;
    return 0;
}

extern "C" {

int bdof_window_stack(bdof_ctx* c, const void* vol, int volNX, int volNY, const int* tab, const double* origin, int B, void* out_rows) {
    const char* who = "bdof_window_stack";
    if (!c || !vol || !tab || !origin || !out_rows) return BDOF_ERR_ARG;
    if (int r = need_configured(c)) return r;
    if (int r = check_batch(c, B)) return r;
    if (int r = window_shape(c, who, volNX, volNY, B)) return r;
    HIPC(c, hipSetDevice(c->device));
    WinStackArgs a{(const float2*)vol, tab, origin, (float2*)out_rows, B, c->S, c->NX, c->NY, volNX, volNY};
    const size_t nrows = (size_t)B * c->S * c->NX;
    hipLaunchKernelGGL(k_window_stack, dim3((unsigned)std::min<size_t>((nrows + 3) / 4, (size_t)c->ncu * 16)), dim3(256), 0, c->stream, a);
    c->win_volNX = volNX;
    c->win_volNY = volNY;
    return launched(c);
}

int bdof_window_stack_adjoint(bdof_ctx* c, const void* grot, int angle, const double* origin, int B, void* gvol, int accumulate, float scale) {
    const char* who = "bdof_window_stack_adjoint";
    if (!c || !origin || !gvol) return BDOF_ERR_ARG;
    if (int r = need_configured(c)) return r;
    if (!c->adj_off) return fail(c, BDOF_ERR_STATE, std::string(who) + ": bdof_set_rotation_adjoint has not been called");
    if (!c->win_volNX) return fail(c, BDOF_ERR_STATE, std::string(who) + ": no bdof_window_stack has been run (it sets the rotated frame the windows lie in)");
    if (int r = check_batch(c, B)) return r;
    if (angle < 0) return fail(c, BDOF_ERR_ARG, std::string(who) + ": angle index outside the rotation tables");
    const int volNX = c->win_volNX, volNY = c->win_volNY;
    if (int r = window_shape(c, who, volNX, volNY, B)) return r;
    if (int r = window_grot(c, who, grot, B)) return r;
    HIPC(c, hipSetDevice(c->device));
    if (B > BDOF_WIN_MAXLIST) {
        // only then can a column's list overflow: count on the host, refuse, never truncate
        std::vector<double> host((size_t)2 * B);
        HIPC(c, hipMemcpyAsync(host.data(), origin, sizeof(double) * host.size(), hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipStreamSynchronize(c->stream));
        if (win_max_per_column(host.data(), B, c->NX, c->NY, volNX, volNY) > BDOF_WIN_MAXLIST)
            return fail(c, BDOF_ERR_SIZE, std::string(who) + ": more than BDOF_WIN_MAXLIST (1024) windows touch one column of the rotated frame");
    }
    ProfScope ps(c, BDOF_K_ROT_ADJ, c->stream);
    const int n_src = c->S * volNX;
    const size_t need = (size_t)n_src * volNY;
    if (c->winpad.size() < need) {
        HIPC(c, hipStreamSynchronize(c->stream));
        HIPC(c, c->winpad.alloc(need));
    }
    if (int r = window_pad_angle(c, angle)) return r;
    WinShiftAdjArgs a{(const float2*)grot, origin, B, c->S, c->NX, c->NY, volNX, volNY};
    const int z_per_wg = 8;
    hipLaunchKernelGGL(k_window_overlap_add_shifted, dim3(volNX, (c->S + z_per_wg - 1) / z_per_wg), dim3(256), 0, c->stream, a,
                       (float2*)c->winpad, z_per_wg);
    return window_pad_adjoint(c, n_src, volNY, gvol, accumulate, scale);
}

int bdof_window_position_grad(bdof_ctx* c, const void* vol, int volNX, int volNY, const int* tab, const void* grot, const double* origin, int B,
                              double* out, int accumulate) {
    const char* who = "bdof_window_position_grad";
    if (!c || !vol || !tab || !origin || !out) return BDOF_ERR_ARG;
    if (int r = need_configured(c)) return r;
    if (int r = check_batch(c, B)) return r;
    if (int r = window_shape(c, who, volNX, volNY, B)) return r;
    if (int r = window_grot(c, who, grot, B)) return r;
    HIPC(c, hipSetDevice(c->device));
    const int P = win_position_partials(c->S, c->NX);
    HIPC(c, c->prm_partial.room((size_t)B * P * 2));           // (shared with bdof_rotate_rigid_param_grad: the calls are stream-ordered)
    WinStackArgs a{(const float2*)vol, tab, origin, (float2*)grot, B, c->S, c->NX, c->NY, volNX, volNY};
    hipLaunchKernelGGL(k_window_position_grad, dim3((unsigned)((size_t)B * P)), dim3(256), 0, c->stream, a, P, (double*)c->prm_partial);
    hipLaunchKernelGGL(k_window_position_sum, dim3(B), dim3(64), 0, c->stream, (const double*)c->prm_partial, P, out, accumulate);
    return launched(c);
}

int bdof_regularizer_value(bdof_ctx* c, const void* x, int NXv, int NZv, int NYv, double* sums) {
    if (!c || !x || !sums) return BDOF_ERR_ARG;
    if (NXv < 1 || NZv < 1 || NYv < 1) return fail(c, BDOF_ERR_ARG, "bad volume shape");
    if (!c->partial) return fail(c, BDOF_ERR_STATE, "bdof_configure has not been called");
    HIPC(c, hipSetDevice(c->device));
    const size_t n = (size_t)NXv * NZv * NYv;
    const int grid = (int)std::min<size_t>((n + 255) / 256, (size_t)(2 * c->npartial / 3));
    hipLaunchKernelGGL(k_reg_value, dim3(grid), dim3(256), 0, c->stream, (const float2*)x, NXv, NZv, NYv, c->partial);
    HIPC(c, hipGetLastError());
    std::vector<double> p(3 * (size_t)grid);
    HIPC(c, hipMemcpyAsync(p.data(), c->partial, sizeof(double) * p.size(), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    sums[0] = sums[1] = sums[2] = 0.0;
    for (int b = 0; b < grid; ++b) for (int j = 0; j < 3; ++j) sums[j] += p[3 * (size_t)b + j];
    return 0;
}

// ---- Fourier shell correlation (bdof_shells.h) --------------------------------------------------------------------------------
// the cached forward double-precision plan of one whole volume [NX][NZ][NY], over its axes longer than 1, in place; c->fft is ready
static int volume_plan(bdof_ctx* c, int NX, int NZ, int NY, rocfft_plan* fwd) {
    if (!g_rocfft_ready) { RFC(c, rocfft_setup()); g_rocfft_ready = true; }
    const std::array<int, 3> key{NX, NZ, NY};
    auto it = c->vol_plans.find(key);
    size_t need = 0;                                                    // a cached plan's work area is there already
    if (it == c->vol_plans.end()) {
        size_t lengths[3], dims = 0;                                    // fastest dimension first
        for (int n : {NY, NZ, NX}) if (n > 1) lengths[dims++] = (size_t)n;
        PlanPair p;
        RFC(c, rocfft_plan_create(&p.fwd, rocfft_placement_inplace, rocfft_transform_type_complex_forward, rocfft_precision_double, dims, lengths, 1, nullptr));
        RFC(c, rocfft_plan_get_work_buffer_size(p.fwd, &need));
        it = c->vol_plans.emplace(key, std::move(p)).first;
    }
    if (int r = fft_exec_room(c, c->fft, c->stream, need)) return r;
    *fwd = it->second.fwd;
    return 0;
}

// C = F (delta + i beta) of one volume in `spec`, unnormalised
static int volume_spectrum(bdof_ctx* c, const void* vol, int NXv, int NZv, int NYv, DevBuf<double2>& spec) {
    const size_t n = (size_t)NXv * NZv * NYv;
    if (spec.size() < n) {
        HIPC(c, hipStreamSynchronize(c->stream));
        HIPC(c, spec.alloc(n));
    }
    rocfft_plan pf;
    if (int r = volume_plan(c, NXv, NZv, NYv, &pf)) return r;
    hipLaunchKernelGGL(k_shell_widen, dim3(g_elem_grid(c, n)), dim3(256), 0, c->stream, (const float2*)vol, (double2*)spec, n);
    void* buf[1] = {(double2*)spec};
    RFC(c, rocfft_execute(pf, buf, nullptr, c->fft.info));
    return launched(c);
}

int bdof_shell_correlation(bdof_ctx* c, const void* vol_a, const void* vol_b, int NXv, int NZv, int NYv, int n_shells, double* out) {
    const char* who = "bdof_shell_correlation";
    if (!c || !vol_a || !vol_b || !out) return BDOF_ERR_ARG;
    if (NXv < 1 || NZv < 1 || NYv < 1) return fail(c, BDOF_ERR_ARG, "bad volume shape");
    if (n_shells < 1) return fail(c, BDOF_ERR_SIZE, std::string(who) + ": n_shells must be at least 1");
    // Nref and L over the axes longer than 1
    long long L = 1, Nref = 0;
    int long_axes = 0;
    for (long long n : {(long long)NXv, (long long)NZv, (long long)NYv}) {
        if (n == 1) continue;
        ++long_axes;
        Nref = Nref ? std::min(Nref, n) : n;
        long long a = L, b = n;
        while (b) { const long long t = a % b; a = b; b = t; }
        L = L / a * n;                                                  // at most 2^30 * (2^31 - 1) before the check
        if (L > (1ll << 30)) return fail(c, BDOF_ERR_SIZE, std::string(who) + ": the least common multiple of the axes exceeds 2^30");
    }
    if (long_axes < 2) return fail(c, BDOF_ERR_SIZE, std::string(who) + ": fewer than two axes longer than 1");
    if (Nref < 4) return fail(c, BDOF_ERR_SIZE, std::string(who) + ": the shortest axis must have at least 4 points");
    HIPC(c, hipSetDevice(c->device));
    if (int r = volume_spectrum(c, vol_a, NXv, NZv, NYv, c->shell_a)) return r;
    if (vol_b != vol_a) if (int r = volume_spectrum(c, vol_b, NXv, NZv, NYv, c->shell_b)) return r;
    const double2* Ca = c->shell_a;
    const double2* Cb = vol_b != vol_a ? c->shell_b : c->shell_a;
    ShellGeom g{NXv, NZv, NYv, (unsigned long long)(L / NXv), (unsigned long long)(L / NZv), (unsigned long long)(L / NYv), (unsigned long long)(L / Nref), 0, 0};
    // A launch files as many shells as one wave's table holds in LDS; shells beyond that take further passes over the spectra.
    // The grid depends on the shape and n_shells alone: the same call adds in the same order.
    const int window = BDOF_SHELL_LDS_BYTES / (int)(BDOF_SHELL_TERMS * sizeof(double));
    const long long rows = (long long)NXv * NZv;
    std::vector<double> host((size_t)std::min(n_shells, window) * BDOF_SHELL_TERMS);
    for (int s_lo = 0; s_lo < n_shells; s_lo += window) {
        g.s_lo = s_lo;
        g.s_n = std::min(n_shells - s_lo, window);
        const int nent = g.s_n * BDOF_SHELL_TERMS;
        const int waves = std::max(1, std::min(4, window / g.s_n));
        const int blocks = (int)std::min<long long>((rows + waves - 1) / waves, (long long)c->ncu * 4);
        const size_t need = ((size_t)blocks + 1) * nent;
        if (c->shell_part.size() < need) {
            HIPC(c, hipStreamSynchronize(c->stream));
            HIPC(c, c->shell_part.alloc(need));
        }
        double* sum = (double*)c->shell_part + (size_t)blocks * nent;
        hipLaunchKernelGGL(k_shell_sums, dim3(blocks), dim3(64 * waves), (size_t)waves * nent * sizeof(double), c->stream, Ca, Cb, g, (double*)c->shell_part);
        hipLaunchKernelGGL(k_shell_blocks, dim3((nent + 255) / 256), dim3(256), 0, c->stream, (const double*)c->shell_part, blocks, nent, sum);
        HIPC(c, hipGetLastError());
        HIPC(c, hipMemcpyAsync(host.data(), sum, sizeof(double) * nent, hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipStreamSynchronize(c->stream));
        std::copy(host.begin(), host.begin() + nent, out + (size_t)s_lo * BDOF_SHELL_TERMS);
    }
    return 0;
}

// ---- analytic starting volume (bdof_fbp.h) ----------------------------------------------------------------------------------------
int bdof_ctf_retrieve(bdof_ctx* c, const void* meas, const void* wgt, double a0_sq, const void* filters, int B, int D, int NX, int NY, void* q) {
    const char* who = "bdof_ctf_retrieve";
    if (!c || !meas || !filters || !q || B < 1 || NX < 1 || NY < 1) return BDOF_ERR_ARG;
    if (D < 1 || D > BDOF_MAX_PLANES) return fail(c, BDOF_ERR_ARG, std::string(who) + ": D outside [1, BDOF_MAX_PLANES]");
    if (!(a0_sq > 0.0) || !std::isfinite(a0_sq)) return fail(c, BDOF_ERR_ARG, std::string(who) + ": |a0|^2 must be finite and > 0");
    if (NX > 4096) return fail(c, BDOF_ERR_SIZE, std::string(who) + ": NX <= 4096 (the ramp kernel's tap table and column block share LDS)");
    if ((long long)B * D * NX * NY > 0x7fffffffLL) return fail(c, BDOF_ERR_SIZE, std::string(who) + ": B * D * NX * NY must be below 2^31");
    HIPC(c, hipSetDevice(c->device));
    const size_t plane = (size_t)NX * NY, n = (size_t)B * D * plane;
    if (c->fbp_work.size() < n) {
        HIPC(c, hipStreamSynchronize(c->stream));
        HIPC(c, c->fbp_work.alloc(n));
    }
    double2* work = c->fbp_work;
    hipLaunchKernelGGL(k_fbp_contrast, dim3(g_elem_grid(c, n)), dim3(256), 0, c->stream, (const float*)meas, (const float*)wgt, a0_sq, work, B, D, plane);
    for (int d = 0; d < D; ++d)
        if (int r = free_step(c, c->fft, c->stream, work + (size_t)d * B * plane, B, NX, NY, (const double2*)filters + (size_t)d * plane, H_KXKY, 0, true)) return r;
    const dim3 grid((NY + 63) / 64, (NX + FBP_RAMP_TILE - 1) / FBP_RAMP_TILE, B);
    hipLaunchKernelGGL(k_fbp_ramp, grid, dim3(256), ((size_t)NX + FBP_RAMP_TILE * 64) * sizeof(double), c->stream, (const double2*)work, (float*)q, B, D, NX, NY);
    return launched(c);
}

int bdof_backproject(bdof_ctx* c, const void* q, int NXd, int NYd, const double* prm, const float* w, int B, void* vol, int NXv, int NZv, int NYv,
                     int row0, int n_rows, int accumulate, float scale_delta, float scale_beta) {
    const char* who = "bdof_backproject";
    if (!c || !q || !prm || !w || !vol || B < 1) return BDOF_ERR_ARG;
    if (NXd < 1 || NYd < 1 || NXv < 1 || NZv < 1 || NYv < 1) return fail(c, BDOF_ERR_ARG, std::string(who) + ": bad shape");
    if ((long long)NXv * NZv * NYv > 0x7fffffffLL || (long long)NXd * NYd > 0x7fffffffLL)
        return fail(c, BDOF_ERR_SIZE, std::string(who) + ": NX * NZ * NY of the volume and NX * NY of a frame must be below 2^31");
    if (row0 < 0 || n_rows < 0 || (long long)row0 + n_rows > (long long)NXv * NZv) return fail(c, BDOF_ERR_ARG, std::string(who) + ": destination rows outside the volume");
    if (n_rows == 0) return 0;
    HIPC(c, hipSetDevice(c->device));
    FbpBackArgs a{(const float*)q, prm, w, (float2*)vol, B, NXd, NYd, NXv, NZv, NYv, row0, row0 + n_rows, accumulate, scale_delta, scale_beta};
    hipLaunchKernelGGL(k_fbp_backproject, dim3(std::min((n_rows + 3) / 4, c->ncu * 16)), dim3(256), 0, c->stream, a);
    return launched(c);
}

int bdof_volume_clip_mask(bdof_ctx* c, void* vol, const float* mask, size_t n) {
    if (!c || !vol) return BDOF_ERR_ARG;
    if (n == 0) return 0;
    HIPC(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_fbp_clip_mask, dim3(g_elem_grid(c, n)), dim3(256), 0, c->stream, (float2*)vol, mask, n);
    return launched(c);
}

void* bdof_stream(bdof_ctx* c) { return c ? (void*)c->stream : nullptr; }

int bdof_mask_shrink(bdof_ctx* c, const void* x, float* mask, size_t n, float thresh) {
    if (!c || !x || !mask) return BDOF_ERR_ARG;
    HIPC(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_mask_shrink, dim3(g_elem_grid(c, n)), dim3(256), 0, c->stream, (const float2*)x, mask, n, thresh);
    return launched(c);
}

int bdof_gather_fields(bdof_ctx* c, void* dst, const void* src, const int* idx, int B, size_t bytes_per_field) {
    if (!c || !dst || !src || !idx || B < 1) return BDOF_ERR_ARG;
    if (bytes_per_field % 4) return fail(c, BDOF_ERR_SIZE, "bdof_gather_fields: fields must be multiples of 4 bytes");
    HIPC(c, hipSetDevice(c->device));
    if (bytes_per_field % 16) {
        const size_t n4 = bytes_per_field / 4;
        const int gx4 = (int)std::min<size_t>((n4 + 255) / 256, 64);
        hipLaunchKernelGGL(k_gather_fields4, dim3(gx4, B < 1024 ? B : 1024), dim3(256), 0, c->stream, (float*)dst, (const float*)src, idx, B, n4);
        return launched(c);
    }
    const size_t n16 = bytes_per_field / 16;
    const int gx = (int)std::min<size_t>((n16 + 255) / 256, 64);
    hipLaunchKernelGGL(k_gather_fields, dim3(gx, B < 1024 ? B : 1024), dim3(256), 0, c->stream, (float4*)dst, (const float4*)src, idx, B, n16);
    return launched(c);
}

int bdof_set_sweep_fusion(bdof_ctx* c, int mode) {
    if (!c) return BDOF_ERR_ARG;
    if (mode < 0 || mode > 2) return fail(c, BDOF_ERR_ARG, "bdof_set_sweep_fusion: mode must be 0, 1 or 2");
    c->fusion = std::min(mode, 1);      // the highest stage this library carries
    return 0;
}
int bdof_sweep_fused(bdof_ctx* c) { return c ? c->fused_last : 0; }

int bdof_set_adjoint_fusion(bdof_ctx* c, int on) {
    if (!c) return BDOF_ERR_ARG;
    if (on < 0 || on > 1) return fail(c, BDOF_ERR_ARG, "bdof_set_adjoint_fusion: on must be 0 or 1");
    c->adj_fusion = on;
    return 0;
}
int bdof_adjoint_fused(bdof_ctx* c) { return c ? c->adj_fused_last : 0; }

int bdof_set_streams(bdof_ctx* c, int n) {
    if (!c) return -1;
    if (n == 0 || n > BDOF_MAX_GROUPS) return fail(c, -2, "bdof_set_streams: n must be -1 or 1..4");
    c->n_streams = n < 0 ? -1 : n;
    return 0;
}

int bdof_batch_groups(bdof_ctx* c, int B) {
    if (!c || B < 1 || !c->NX) return -1;
    if (c->generic) return 1;
    Group g[BDOF_MAX_GROUPS];
    return batch_groups(c, B, c->NX, 16, g);
}

int bdof_profile_enable(bdof_ctx* c, int enable) {
    if (!c) return BDOF_ERR_ARG;
    HIPC(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    if (enable) { for (int i = 0; i < BDOF_K_COUNT; ++i) { c->prof_ms[i] = 0; c->prof_n[i] = 0; c->prof_seen[i] = 0; } }
    c->prof = enable != 0;
    c->prof_stride = enable > 1 ? enable : 1;
    return 0;
}

int bdof_profile_read(bdof_ctx* c, int kernel_class, int* n_launches, double* total_ms) {
    if (!c || kernel_class < 0 || kernel_class >= BDOF_K_COUNT) return BDOF_ERR_ARG;
    HIPC(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    if (n_launches) *n_launches = c->prof_n[kernel_class];
    if (total_ms) *total_ms = c->prof_ms[kernel_class];
    return 0;
}

int bdof_device_mem(bdof_ctx* c, size_t* free_bytes, size_t* total_bytes) {
    if (!c || !free_bytes || !total_bytes) return BDOF_ERR_ARG;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipMemGetInfo(free_bytes, total_bytes));
    return 0;
}

int bdof_malloc(void** ptr, size_t bytes) {
    if (!ptr) return BDOF_ERR_ARG;
    return (int)hipMalloc(ptr, bytes);
}
int bdof_ctx_malloc(bdof_ctx* c, void** ptr, size_t bytes) {
    if (!c || !ptr) return BDOF_ERR_ARG;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipMalloc(ptr, bytes));
    return 0;
}
int bdof_free(void* ptr) { return (int)hipFree(ptr); }
// the caller writes device memory through the ctx: a table bdof_rotation_adjoint_adam left for that memory is no longer its table
static void wrote(bdof_ctx* c, const void* dst, size_t bytes) {
    if (!c->mod_for) return;
    const char *d = (const char*)dst, *t = (const char*)c->mod_for;
    if (d < t + c->mod_for_rows * c->mod_for_NY * sizeof(float2) && t < d + bytes) c->mod_for = nullptr;
}

int bdof_memcpy_h2d(bdof_ctx* c, void* dst, const void* src, size_t bytes) {
    if (!c) return BDOF_ERR_ARG;
    wrote(c, dst, bytes);
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return 0;
}
int bdof_memcpy_d2h(bdof_ctx* c, void* dst, const void* src, size_t bytes) {
    if (!c) return BDOF_ERR_ARG;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return 0;
}
int bdof_memset(bdof_ctx* c, void* dst, int value, size_t bytes) {
    if (!c) return BDOF_ERR_ARG;
    wrote(c, dst, bytes);
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipMemsetAsync(dst, value, bytes, c->stream));
    return 0;
}

int bdof_memcpy_d2d(bdof_ctx* c, void* dst, const void* src, size_t bytes) {
    if (!c) return BDOF_ERR_ARG;
    wrote(c, dst, bytes);
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}


// =================================================================================================
// Collectives (RCCL over xGMI): comm.Allreduce(this_grads, grads) of cnn_propagator/fullfield.py:348-351
// =================================================================================================
static int comm_fail(bdof_comm* m, int code, const std::string& msg) {
    if (m) m->err = msg;
    g_rccl.err = msg;
    return code;
}
#define NCCLC(m, call)                                                                                     \
    do {                                                                                                   \
        ncclResult_t r_ = (call);                                                                          \
        if (r_ != ncclSuccess)                                                                             \
            return comm_fail((m), 1000 + (int)r_, std::string(#call) + ": " + g_rccl.GetErrorString(r_));  \
    } while (0)
#define HIPM(m, call)                                                                                      \
    do {                                                                                                   \
        hipError_t e_ = (call);                                                                            \
        if (e_ != hipSuccess) return comm_fail((m), (int)e_, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

int bdof_comm_unique_id(void* id, size_t bytes) {
    if (!id || bytes < sizeof(ncclUniqueId)) return BDOF_ERR_ARG;
    if (!rccl_load()) return BDOF_ERR_STATE;
    ncclUniqueId u;
    ncclResult_t r = g_rccl.GetUniqueId(&u);
    if (r != ncclSuccess) { g_rccl.err = std::string("ncclGetUniqueId: ") + g_rccl.GetErrorString(r); return 1000 + (int)r; }
    std::memcpy(id, &u, sizeof(u));
    return 0;
}

const char* bdof_comm_last_error(const bdof_comm* m) { return m ? m->err.c_str() : g_rccl.err.c_str(); }

void bdof_comm_destroy(bdof_comm* m);

int bdof_comm_create(bdof_comm** out, int device, int nranks, int rank, const void* id, size_t bytes) {
    if (!out || !id || bytes < sizeof(ncclUniqueId) || nranks < 1 || rank < 0 || rank >= nranks) return BDOF_ERR_ARG;
    *out = nullptr;
    if (!rccl_load()) return BDOF_ERR_STATE;
    bdof_comm* m = new bdof_comm();
    m->device = device; m->nranks = nranks; m->rank = rank;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&m->ev_in, hipEventDisableTiming);
    for (int i = 0; e == hipSuccess && i < BDOF_COMM_TICKETS; ++i) e = hipEventCreateWithFlags(&m->ticket[i], hipEventDisableTiming);
    if (e != hipSuccess) { g_rccl.err = std::string("bdof_comm_create: ") + hipGetErrorString(e); bdof_comm_destroy(m); return (int)e; }
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof(u));
    ncclResult_t r = g_rccl.CommInitRank(&m->comm, nranks, u, rank);
    if (r != ncclSuccess) {
        g_rccl.err = std::string("ncclCommInitRank: ") + g_rccl.GetErrorString(r);
        m->comm = nullptr;
        bdof_comm_destroy(m);                  // releases the stream and the events created above
        return 1000 + (int)r;
    }
    *out = m;
    return 0;
}

void bdof_comm_destroy(bdof_comm* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    if (m->comm) (void)g_rccl.CommDestroy(m->comm);
    for (int i = 0; i < BDOF_COMM_TICKETS; ++i) if (m->ticket[i]) (void)hipEventDestroy(m->ticket[i]);
    if (m->ev_in) (void)hipEventDestroy(m->ev_in);
    if (m->stream) (void)hipStreamDestroy(m->stream);
    delete m;
}

int bdof_comm_size(const bdof_comm* m) { return m ? m->nranks : 0; }
int bdof_comm_rank(const bdof_comm* m) { return m ? m->rank : -1; }

// the communicator's stream picks up behind everything the ctx stream holds now
static int comm_enter(bdof_comm* m, bdof_ctx* c) {
    if (!m || !c) return BDOF_ERR_ARG;
    if (m->device != c->device) return comm_fail(m, BDOF_ERR_ARG, "communicator and ctx live on different devices");
    HIPM(m, hipSetDevice(m->device));
    HIPM(m, hipEventRecord(m->ev_in, c->stream));
    HIPM(m, hipStreamWaitEvent(m->stream, m->ev_in, 0));
    return 0;
}
static int comm_leave(bdof_comm* m, int* ticket) {
    const unsigned t = m->next++ % BDOF_COMM_TICKETS;
    HIPM(m, hipEventRecord(m->ticket[t], m->stream));
    if (ticket) *ticket = (int)t;
    return 0;
}

int bdof_allreduce_grad(bdof_comm* m, bdof_ctx* c, void* buf, size_t count, int* ticket) {
    int r = comm_enter(m, c);
    if (r) return r;
    if (!buf) return comm_fail(m, BDOF_ERR_ARG, "null buffer");
    if (count) NCCLC(m, g_rccl.AllReduce(buf, buf, count, ncclFloat, ncclSum, m->comm, m->stream));
    return comm_leave(m, ticket);
}

int bdof_reduce_scatter_grad(bdof_comm* m, bdof_ctx* c, void* buf, size_t count_per_rank, int* ticket) {
    int r = comm_enter(m, c);
    if (r) return r;
    if (!buf) return comm_fail(m, BDOF_ERR_ARG, "null buffer");
    if (count_per_rank)
        NCCLC(m, g_rccl.ReduceScatter(buf, (float*)buf + (size_t)m->rank * count_per_rank, count_per_rank, ncclFloat, ncclSum, m->comm, m->stream));
    return comm_leave(m, ticket);
}

int bdof_allgather_volume(bdof_comm* m, bdof_ctx* c, void* buf, size_t count_per_rank, int* ticket) {
    int r = comm_enter(m, c);
    if (r) return r;
    if (!buf) return comm_fail(m, BDOF_ERR_ARG, "null buffer");
    if (count_per_rank)
        NCCLC(m, g_rccl.AllGather((const float*)buf + (size_t)m->rank * count_per_rank, buf, count_per_rank, ncclFloat, m->comm, m->stream));
    return comm_leave(m, ticket);
}

int bdof_bcast_volume(bdof_comm* m, bdof_ctx* c, void* buf, size_t count, int root, int* ticket) {
    int r = comm_enter(m, c);
    if (r) return r;
    if (!buf || root < 0 || root >= m->nranks) return comm_fail(m, BDOF_ERR_ARG, "bad buffer / root");
    if (count) NCCLC(m, g_rccl.Broadcast(buf, buf, count, ncclFloat, root, m->comm, m->stream));
    return comm_leave(m, ticket);
}

int bdof_comm_wait(bdof_comm* m, bdof_ctx* c, int ticket) {
    if (!m || !c || ticket < 0 || ticket >= BDOF_COMM_TICKETS) return BDOF_ERR_ARG;
    HIPM(m, hipSetDevice(m->device));
    HIPM(m, hipStreamWaitEvent(c->stream, m->ticket[ticket], 0));
    return 0;
}

int bdof_comm_sync(bdof_comm* m) {
    if (!m) return BDOF_ERR_ARG;
    HIPM(m, hipSetDevice(m->device));
    HIPM(m, hipStreamSynchronize(m->stream));
    return 0;
}

}  // extern "C"
