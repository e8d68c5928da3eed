/* bdof.h — C ABI of libbdof.so: MI355X-native multislice Fresnel forward + adjoint + Adam.
 *
 * The reference (mdw771/beyond_dof) has no FFI layer; its only seam is a set of Python call
 * signatures.  Each entry point below names the reference interface it replaces
 * (paths relative to the reference checkout).  The Python host in beyond_dof_amd/ binds these
 * with ctypes and re-exposes the reference's own function names.
 *
 * Conventions
 *   - every call returns int: 0 ok, <0 bdof argument/state error, >0 hipError_t; text via
 *     bdof_last_error(ctx).
 *   - device buffers passed in are caller-owned raw device pointers; the library never frees them.
 *   - one ctx <-> one device <-> one stream; calls are asynchronous on that stream until
 *     bdof_sync / bdof_get_loss; a ctx is not thread-safe.
 *   - complex = interleaved float (re, im); "pair" = interleaved float (delta, beta).
 *
 * Internal data layout:
 *   wavefields        [b][x][y]            y fastest (y = tomographic rotation axis, reference axis 0)
 *   object rows       [row][y]   of pairs  full-field: row = x*Z + z of the un-rotated volume
 *   rotated gradient  [b][z][x][y] of pairs
 */
#ifndef BDOF_H
#define BDOF_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct bdof_ctx bdof_ctx;

enum { BDOF_DET_NONE = 0, BDOF_DET_NEAR = 1, BDOF_DET_FAR = 2 };      /* free_prop_cm None / float / 'inf'  (np_funcs.py:45-61) */
enum { BDOF_VARIANT_NUMPY_SKIP_LAST = 0, BDOF_VARIANT_TF_ALL = 1 };   /* np_funcs.py:41 vs tensorflow_recon/util.py:465-483 */
enum { BDOF_K_ROW_FWD = 0, BDOF_K_COL_PROP = 1, BDOF_K_ROW_BWD = 2, BDOF_K_LOSS = 3, BDOF_K_ROT_ADJ = 4, BDOF_K_ADAM = 5, BDOF_K_COUNT = 6 };
enum { BDOF_CFG_GRAD = 1, BDOF_CFG_GENERIC = 2, BDOF_CFG_NO_RESIDENT = 4, BDOF_CFG_ALWAYS_RESIDENT = 8, BDOF_CFG_RECOMPUTE = 16,
       BDOF_CFG_NO_GROT = 32, BDOF_CFG_ADJOINT64 = 64 };                /* bdof_configure's with_grad flags */

/* lifecycle.  `stream` is a hipStream_t (NULL: the library creates its own). */
int bdof_ctx_create(bdof_ctx** out, int device, void* stream);
void bdof_ctx_destroy(bdof_ctx* ctx);
const char* bdof_last_error(const bdof_ctx* ctx);
int bdof_sync(bdof_ctx* ctx);
void* bdof_stream(bdof_ctx* ctx);   /* the ctx's hipStream_t, for ordering foreign work (collectives) against it */
int bdof_device_count(void);

/* Host only (no device is touched): the twiddle tables bdof_configure uploads for transforms of length N, as D copies of
 * [N hi (re, im)][N lo (re, im)] float32 — exp(-2 pi i j / N) with lo = the rounding error of hi.  D >= 2: the dithered copies
 * (entry j of copy d is the float32 below or above the float64 value, the upper one in the fraction of the copies that makes the
 * mean over the copies equal the float64 value to ulp / D; DESIGN §5 "Dithered transform constants"); D = 0 or 1: one copy,
 * rounded to nearest with the modulus kept closest to one.  out: 4 N max(D, 1) floats.  Exposed for the tests. */
int bdof_twiddle_tables(int N, int D, float* out);
int bdof_device_pci_bus_id(int device, char* out, int len);      /* "0000:c1:00.0": which physical GPU a rank really got */
/* Stream-ordered time stamps on the ctx stream (16 slots): mark now, read the interval after the work has run — how the
 * bench reports the tail of a step (rotation adjoint, gradient exchange, Adam) without a host synchronisation inside it. */
int bdof_timer_mark(bdof_ctx* ctx, int slot);
int bdof_timer_elapsed(bdof_ctx* ctx, int slot_a, int slot_b, double* ms);

/* Workspace for wavefields of NY x NX, S slices, up to Bmax wavefields per launch.  Three engines sit behind the same calls:
 *   - fused streaming kernels (hand-written FFTs, field in HBM): NY, NX powers of two in 64..1024;
 *   - LDS-resident kernel (the whole field stays in one CU's LDS through all slices, one launch per minibatch): square
 *     fields of 32, 36, 48, 64, 72, 80, 96 or 128 pixels — the probes of the ptychography drivers
 *     (cnn_propagator/reconstruct_ptycho.py:106); chosen when no fused plan exists or the batch has >= CUs/4 wavefields;
 *   - generic-size engine (rocFFT + point-wise kernels): every other size.
 * with_grad: an OR of BDOF_CFG_* flags.  BDOF_CFG_GRAD allocate the tape (S fields per wavefield) and the rotated-frame
 * gradient; BDOF_CFG_GENERIC force the generic-size engine (cross-checks); BDOF_CFG_NO_RESIDENT never use the resident engine;
 * BDOF_CFG_ALWAYS_RESIDENT use it for every batch size; BDOF_CFG_RECOMPUTE tape-free adjoint of the streaming engine: 3 tape
 * fields instead of S, the forward wave is marched back beside the adjoint field; BDOF_CFG_NO_GROT no
 * rotated-frame gradient workspace (range sweeps with caller-owned buffers, bdof_adjoint_range); BDOF_CFG_ADJOINT64 float64
 * adjoint sweep (accuracy option; runs on the generic-size engine whatever the size): seed, adjoint transforms (rocFFT double
 * precision), transfer function and the products conj(phi) G in float64, forward sweep and tape in float32 — what autograd's
 * float64 tape gives the reference (cnn_propagator/fullfield.py:329, ptychography.py:248); follow bdof_set_physics with
 * bdof_set_physics_f64.
 * Environment read here: BDOF_TW_DITHER=D — number of dithered copies of the transform constants the per-slice kernels walk
 * (default 64; 0: one plain float32 table, round 2's behaviour; DESIGN §5 "Dithered transform constants").
 * Replaces the per-call allocations of multislice_propagate_batch_numpy
 * (cnn_propagator/np_funcs.py:20,43) and of autograd's tape (cnn_propagator/fullfield.py:329). */
int bdof_configure(bdof_ctx* ctx, int NY, int NX, int S, int Bmax, int with_grad);

/* Slice binning: one propagation step per `bin` voxel slices (Adorym's `binning`; a step only has to stay below the depth of
 * focus).  S of bdof_configure stays the VOXEL depth — the stride of tab[angle][z][x], of the rows (b*S+z)*NX+x and of the
 * rotated-frame gradient [B][S][NX][NY] — and n = S / bin steps are taken: for step i = 0 .. n-1
 *     c_i = prod_j exp(i k delta[i bin + j] - k beta[i bin + j]), j < bin   (k per voxel, unchanged; exact for phase and absorption)
 *     phi_i = c_i psi_i ;  psi_{i+1} = P_bin phi_i,  P_bin the transfer-function step of get_kernel(bin * delta_nm, ...)
 * with the step taken for i < n-1 (numpy_skip_last) or every i (tf_all) as without binning; detector step, loss and seed are
 * unchanged.  Every voxel slice of a bin receives the bin's one gradient row, g_delta[i bin + j] = k Im(conj(phi_i) G(phi_i)),
 * g_beta[i bin + j] = -k Re(conj(phi_i) G(phi_i)).  bin = 1 is the model without the option, bit for bit.
 * Call order: bdof_configure, bdof_set_slice_binning, bdof_set_physics (hs, h00 and the tables of bdof_set_transfer_f64 /
 * bdof_set_probe_field built for bin * delta_nm; k and the detector tables as before), then probe and object as usual.
 * bdof_configure puts bin back to 1 (not sticky, unlike bdof_set_loss).  bin >= 1 and S % bin == 0, else an argument error (a
 * shorter last bin is not carried); after bdof_set_physics / bdof_set_probe a state error.  The call sizes the tape to n fields
 * per wavefield; the carrier-field stack of bdof_set_probe_stack has n planes, bdof_tape_to_real takes i < n, the carrier
 * scalars and the dithered constants run over the steps.
 * With bin > 1 only the streaming and the generic-size engine run (never the LDS-resident one), and what does not carry the
 * option returns a state error instead of running the unbinned model: a ctx configured with BDOF_CFG_ALWAYS_RESIDENT,
 * BDOF_CFG_RECOMPUTE, BDOF_CFG_ADJOINT64 or BDOF_CFG_NO_GROT (refused here), bdof_set_conv and every *_conv* call, bdof_set_tf_f64 /
 * bdof_loss_grad_tf_f64, bdof_forward_range*, bdof_adjoint_range, bdof_set_range_carrier / bdof_range_carrier_build and
 * bdof_set_object_bilinear. */
int bdof_set_slice_binning(bdof_ctx* ctx, int bin);

/* Physics.  k = 2*PI*delta_nm/lambda_nm (np_funcs.py:32).  hs / hs_det: HOST arrays [NX][NY] complex,
 * hs[kx][ky] = ifftshift(get_kernel(...))[ky][kx] / (NX*NY)   (cnn_propagator/util.py:82-102, np_funcs.py:42);
 * the host computes them in float64 exactly as the reference does and rounds once to float32.
 * hs_det may be NULL unless det_mode == BDOF_DET_NEAR.  h00 / hdet00: (re, im) of the un-scaled DC values
 * ifftshift(H)[0][0] in float64 — the factor a constant wave picks up in one step (carrier splitting, below). */
int bdof_set_physics(bdof_ctx* ctx, double k, const float* hs, const float* hs_det, const double* h00, const double* hdet00,
                     int det_mode, int variant);

/* The same two tables in float64 (HOST arrays of complex128, layout and 1/(NX*NY) scaling of hs / hs_det) for the float64
 * adjoint sweep of bdof_configure flag 64; call after every bdof_set_physics. */
int bdof_set_physics_f64(bdof_ctx* ctx, const double* hs, const double* hs_det);

/* Probe wavefront (np_funcs.py:20-21; cnn_propagator/fullfield.py:276-314), split as probe = a0 + eps: `probe_eps` is
 * the HOST array [NX][NY] complex of eps, a0 any complex constant (0 for a general probe, the plane-wave amplitude for a
 * plane probe).  The library carries a0 through the slices exactly (a_{z+1} = a_z * h00, float64 on the host) and runs
 * only eps through the float32 FFTs, so round-off scales with the scattered field, not with the full wave. */
int bdof_set_probe(bdof_ctx* ctx, const float* probe_eps, double a0_re, double a0_im);

/* Carrier FIELD for a localised probe (all three engines of the transfer-function path).  stack: HOST array [S][NX][NY] complex, the probe propagated
 * through free space to the entrance of every slice, p_0 = probe, p_{z+1} = ifft2(ifftshift(fftshift(fft2 p_z) H))
 * (np_funcs.py:42 without an object), computed by the host in float64; det: HOST [NX][NY], the same wave at the detector
 * (no detector: p_{S-1}, or p_S with the tf_all variant; near field: one more step with the detector kernel; far field:
 * the un-shifted, un-normalised fft2 of it, indexed [kx][ky]).  The wave is then carried as psi_z = p_z + eps_z and only
 * the scattered part eps runs through the float32 transforms, whose round-off therefore scales with the scattered field —
 * what the scalar a0 of bdof_set_probe does for a plane wave.  Call bdof_set_probe with a zero array (eps_0 = 0, a0 = 0).
 * NULL, NULL removes the stack.  bdof_probe_stack_supported: 1 once bdof_configure has run (the real-space propagator of
 * bdof_set_conv does not use the stack). */
int bdof_probe_stack_supported(bdof_ctx* ctx);
int bdof_set_probe_stack(bdof_ctx* ctx, const float* stack, const float* det);

/* The same carrier field computed by the library, on the device, in float64: probe HOST [NX][NY] complex128; hT / hdetT HOST
 * [kx][ky] complex128 = ifftshift(get_kernel(...)) transposed, NOT divided by NX*NY (hdetT: the detector distance, NULL unless
 * det_mode == BDOF_DET_NEAR).  Replaces bdof_set_probe + bdof_set_probe_stack for a localised probe: no host FFTs, so a probe
 * that changes every step (probe_type='optimizable', tensorflow_recon/fullfield.py:311-327) stays cheap. */
int bdof_set_probe_field(bdof_ctx* ctx, const double* probe, const double* hT, const double* hdetT);

/* Object.  vol: n_rows device rows of volNY (delta, beta) pairs.  Call again whenever that memory has been modified: the
 * library keeps a table of the modulation factors exp(i k delta - k beta) - 1 of these rows and rebuilds it lazily.
 *  tab == NULL: row(b,z,x) = (b*S+z)*NX+x, i.e. the caller
 * supplies already rotated objects (the grid_delta_batch/grid_beta_batch arguments of
 * multislice_propagate_batch_numpy).  tab != NULL (device, [n_angles][S][volNX] int32): fused
 * nearest-neighbour rotation gather, row = tab[angle][z][x]  (apply_rotation, cnn_propagator/util.py:377-402
 * with the tables of save_rotation_lookup, util.py:294-347). */
int bdof_set_object(bdof_ctx* ctx, const void* vol, long long n_rows, int volNY, const int* tab, int volNX, int n_angles);

/* Inverse rotation tables for the gradient (device): off [n_angles][n_dest+1], order [n_angles][S*volNX]. */
int bdof_set_rotation_adjoint(bdof_ctx* ctx, const int* off, const int* order, int n_dest);

/* Forward model only: replaces multislice_propagate_batch_numpy (np_funcs.py:15-65).
 * angle_of_b / xoff / yoff: device int32 [B] or NULL.  out_wave: device [B][NX][NY] complex, detector
 * wave (far field: un-shifted fft2, the caller applies fftshift).  keep_tape != 0 keeps the per-slice
 * hybrid fields for bdof_tape_to_real (needs with_grad). */
int bdof_forward(bdof_ctx* ctx, int B, const int* angle_of_b, const int* xoff, const int* yoff, void* out_wave, int keep_tape);

/* Slices z0 .. z0+nz-1 only, from caller-supplied real-space fields: in_real [B][NX][NY] complex is the (scattered part of
 * the) wave entering slice z0, one field per wavefield; out_real receives the wave after the range in real space —
 * psi_{z0+nz} if prop_last (a transfer-function step follows the last slice of the range), else phi_{z0+nz-1}.  Fused
 * streaming kernels only.  The building block of the tiled propagation below; np_funcs.py:36-43 restricted to a range. */
int bdof_forward_range(bdof_ctx* ctx, int B, const int* angle_of_b, const int* xoff, const int* yoff, int z0, int nz,
                       const void* in_real, void* out_real, int prop_last);

/* Tiled ("pfft") Fresnel propagation (the reference's README.md:1-11; its scripts are on a branch absent from the checkout,
 * BASELINE cfg4): a field [FX][FY] complex too large for one fused plan is cut into B overlapping tiles [TX][TY] with origins
 * (x0[b], y0[b]) (device int32; periodic in the field, like the whole-field FFT propagator they replace); the tiles run
 * through bdof_forward_range as a batch with the object windowed by the same origins; every few slices the cores (tile minus
 * a halo of halo_x / halo_y pixels per side) are written back and the tiles re-cut, which refreshes the halos before the
 * wrap-around of a tile's own periodic boundary has crossed them (it advances lambda dz / (2 dx^2) pixels per slice).  The
 * outermost `taper` pixels of every gathered tile are ramped to zero (raised cosine): without the ramp the jump where a tile's
 * left and right edge meet diffracts into it with a 1/distance tail. */
int bdof_tiles_gather(bdof_ctx* ctx, const void* field, int FX, int FY, void* tiles, int B, int TX, int TY, const int* x0, const int* y0,
                      int taper);
int bdof_tiles_scatter(bdof_ctx* ctx, const void* tiles, void* field, int FX, int FY, int B, int TX, int TY, const int* x0, const int* y0,
                       int halo_x, int halo_y);

/* Gradient of the tiled path (tape-free, range by range, last range first).  bdof_adjoint_range is the adjoint of
 * bdof_forward_range(prop_last = 1): end_real = the psi_{z0+nz} that call returned, g_end_real = G(psi_{z0+nz}) (both device
 * [B][NX][NY] complex); g_start_real receives G(psi_{z0}); the gradient rows of the range's slices go to grot_range, device
 * [B][nz][NX][NY] pairs (a ctx configured with with_grad | 16 | 32 has no [B][S] gradient workspace of its own: 260 GB for
 * 121 tiles of 512^2 x 1024 slices).  The forward wave is marched back from end_real beside the adjoint field.
 * bdof_tiles_scatter_adjoint / bdof_tiles_gather_adjoint: adjoints of the two stitching steps; bdof_tiles_grad_add: the
 * range's gradient rows added into the volume gradient gvol (rows of volNY pairs, the object's own layout) through the table
 * of bdof_set_object — which must be injective in x for every slice (no rotation: the tiled path runs one pre-rotated object).
 * bdof_tiles_gather_adjoint (and bdof_tiles_gather_adjoint_diff64) and bdof_tiles_grad_add take any number of tiles B, however
 * many of them meet on one field row or volume column: the kernels sum them in ascending tile order, 1024 (tile, row) pairs at
 * a time.  Only a single tile that wraps onto one field row more than 1024 times (TX > 1024 FX) is refused, BDOF_ERR_SIZE (-3).
 * bdof_field_loss_seed: loss mean((|field| - meas)^2) (bdof_get_loss) and, in place, its seed — fullfield.py:106 on a field. */
int bdof_adjoint_range(bdof_ctx* ctx, int B, const int* angle_of_b, const int* xoff, const int* yoff, int z0, int nz,
                       const void* end_real, const void* g_end_real, void* g_start_real, void* grot_range);
int bdof_tiles_scatter_adjoint(bdof_ctx* ctx, const void* field, int FX, int FY, void* tiles, int B, int TX, int TY, const int* x0,
                               const int* y0, int halo_x, int halo_y);
int bdof_tiles_gather_adjoint(bdof_ctx* ctx, const void* tiles, void* field, int FX, int FY, int B, int TX, int TY, const int* x0,
                              const int* y0, int taper);
int bdof_tiles_grad_add(bdof_ctx* ctx, const void* grot_range, void* gvol, int B, int TX, int TY, const int* x0, const int* y0, int z0, int nz);
int bdof_field_loss_seed(bdof_ctx* ctx, void* field, const float* meas, int FX, int FY);

/* Long-range correction and float64 path of the tiled propagator (round 4; DESIGN "cfg4").
 * The band-limited whole-field propagator of np_funcs.py:42 has alternating tails ~ lambda dz n / (2 pi x^2) after n slices that
 * reach across the whole field; a tile never sees sources beyond its halo, and at 1024 slices that alone is 2.2e-5 of the exit
 * wave — in float64, whatever the stitch interval.  Free space composes (P^n = F^-1 H^n F), so once per stitch range the part
 * the tiles miss is added back: D psi_in = (whole-field free-space step over the range) - (the tiles' own, stitched), exact
 * to first order in the object's phase over one range; with ranges shorter than the band edge's phase-winding length
 * (4 dx^2 / (lambda dz) = 16 slices at 5 keV / 1 nm) the tiling error drops to 1e-6.
 * bdof_fields_free_step: fields[b] <- F^-1 ( h * F fields[b] ) for B fields [NX][NY] in place (rocFFT, one batched transform
 *   pair); h[kx][ky] (device) carries 1 / (NX NY) and whatever power of the transfer function the caller folded in;
 *   conj_h: the adjoint step; is_double: complex128 fields and table, else complex64.  Any NX, NY rocFFT takes.
 * bdof_caxpy: y += alpha x on n complex numbers; bdof_c_convert: complex64 <-> complex128 copy.
 * bdof_tiles_gather_f64 / bdof_tiles_scatter_f64: bdof_tiles_gather / bdof_tiles_scatter on complex128 fields and tiles.
 * bdof_forward_range_f64: bdof_forward_range on caller-owned complex128 fields [B][NX][NY] IN PLACE, everything in float64 —
 *   what the reference computes in (np_funcs.py:20-42 promote to complex128, quirk Q2): c = exp(i k delta) exp(-k beta) from
 *   the (delta, beta) rows of bdof_set_object, rocFFT double-precision transforms, h[kx][ky] / (NX NY) in float64 (device).
 *   Unfused (an accuracy path, ~4x the time of the fused float32 kernels): a 1024-slice stack through float32 transforms
 *   carries 1.5e-5 of rounding, this path none. */
/* The slice step's transfer function in float64 ([ky][kx], 1 / (NX NY) folded in: what bdof_set_physics' hs was rounded from;
 * call it after bdof_set_physics).  The streaming engine's per-slice launches then multiply by dithered float32 copies of it —
 * copy z mod D for slice z, the adjoint step by the conjugate of the copy its forward step used — whose roundings average to the
 * float64 values: a fixed float32 table is the same perturbation in every slice and its error grows linearly with depth
 * (1.4e-5 of the exit wave after 1024 slices with everything else in float64; 1e-6 with the copies).  np_funcs.py:42 multiplies
 * by a complex128 H.  D = env BDOF_H_DITHER (default 64, at most 256 MiB of copies; 0 switches it off). */
int bdof_set_transfer_f64(bdof_ctx* ctx, const double* hs64);
/* bdof_forward_range with the table of its transfer-function steps supplied by the caller (device, [ky][kx] complex64 like hs):
 * the tiled propagator's free-space step over a whole stitch range (H^n) through the fused kernels. */
/* Carrier fields for the next bdof_forward_range calls over slices z0 .. z0 + nz - 1 of B wavefields: device stack [nz][B][NX][NY]
 * complex64, wavefield b's free-space propagation to the entrance of each slice (formed in double by the caller:
 * bdof_fields_free_step + bdof_c_convert).  The range is swept on psi_z = p_z + eps_z with only eps in the float32 transforms;
 * in_real is the scattered part entering the range, out_real the scattered part leaving it — for the tiles of a corrected stitch
 * range (np_funcs.py:36-43 on a tile) T psi - T_free psi itself.  Needs a zero ctx probe (bdof_set_probe with a0 = 0, no probe
 * stack).  NULL removes the stack. */
int bdof_set_range_carrier(bdof_ctx* ctx, const void* stack, int B, int z0, int nz);
/* bdof_fields_free_step on an auxiliary stream: starts after everything queued on the ctx's stream so far (first copying `src`
 * into `fields` there, if not NULL) and runs beside what the ctx's stream is handed next; bdof_aux_join makes the ctx's stream
 * wait for it.  One step in flight at a time.  (The whole-field free-space step of a stitch range, F^-1 H^n F of np_funcs.py:42,
 * beside the tiles' sweeps.) */
int bdof_fields_free_step_aux(bdof_ctx* ctx, void* fields, const void* src, int B, int NX, int NY, const void* h, int conj_h, int is_double);
int bdof_aux_join(bdof_ctx* ctx);
/* The carrier stack of bdof_set_range_carrier in one call: p0 device complex128 [B][NX][NY] (the wavefields entering the range;
 * overwritten), stack device complex64 [nz][B][NX][NY] <- F^-1(H^z F p0), z = 0 .. nz - 1, formed in double (one forward
 * transform, the spectra by a running product, one batched inverse transform); h complex128 [kx][ky], ifftshift(H) / (NX NY). */
int bdof_range_carrier_build(bdof_ctx* ctx, void* p0, void* stack, int B, int NX, int NY, const void* h, int nz);
int bdof_forward_range_h(bdof_ctx* ctx, int B, const int* angle_of_b, const int* xoff, const int* yoff, int z0, int nz,
                         const void* in_real, void* out_real, int prop_last, const void* h);
int bdof_fields_free_step(bdof_ctx* ctx, void* fields, int B, int NX, int NY, const void* h, int conj_h, int is_double);
int bdof_caxpy(bdof_ctx* ctx, void* y, const void* x, double alpha, size_t n, int is_double);
int bdof_c_convert(bdof_ctx* ctx, void* dst, const void* src, size_t n, int to_double);
int bdof_tiles_gather_f64(bdof_ctx* ctx, const void* field, int FX, int FY, void* tiles, int B, int TX, int TY, const int* x0,
                          const int* y0, int taper);
int bdof_tiles_scatter_f64(bdof_ctx* ctx, const void* tiles, void* field, int FX, int FY, int B, int TX, int TY, const int* x0,
                           const int* y0, int halo_x, int halo_y);
/* The float32 tiled path with the long-range correction keeps its FIELD in complex128: the whole-field free-space step carries
 * the bulk of the wave in double, the complex64 tiles (fused kernels) add the object's part, T psi - T_free psi.
 * bdof_tiles_gather_mixed: complex64 tiles cut out of the complex128 field (tapered, periodic);
 * bdof_tiles_scatter_diff64: field[core] = (accumulate ? field[core] : 0) + tiles_a - tiles_b (tiles_b nullable), in float64. */
int bdof_tiles_gather_mixed(bdof_ctx* ctx, const void* field64, int FX, int FY, void* tiles, int B, int TX, int TY, const int* x0,
                            const int* y0, int taper);
int bdof_tiles_scatter_diff64(bdof_ctx* ctx, const void* tiles_a, const void* tiles_b, void* field64, int FX, int FY, int B, int TX, int TY,
                              const int* x0, const int* y0, int halo_x, int halo_y, int accumulate);
/* Their adjoints, for the gradient through the corrected tiled model: bdof_tiles_scatter_adjoint_mixed (complex64 tiles = the
 * complex128 field on every tile's core, zero elsewhere) and bdof_tiles_gather_adjoint_diff64 (field64 (+)= the tapered, periodic
 * scatter-add of tiles_a - tiles_b; deterministic gather form). */
int bdof_tiles_scatter_adjoint_mixed(bdof_ctx* ctx, const void* field64, int FX, int FY, void* tiles, int B, int TX, int TY, const int* x0,
                                     const int* y0, int halo_x, int halo_y);
int bdof_tiles_gather_adjoint_diff64(bdof_ctx* ctx, const void* tiles_a, const void* tiles_b, void* field64, int FX, int FY, int B, int TX,
                                     int TY, const int* x0, const int* y0, int taper, int accumulate);
int bdof_forward_range_f64(bdof_ctx* ctx, int B, const int* angle_of_b, const int* xoff, const int* yoff, int z0, int nz,
                           void* fields, const void* h, double k, int prop_last);

/* probe_array[i] of np_funcs.py:43 (wave after slice i), device out [B][NX][NY]; valid after a
 * bdof_forward(keep_tape=1) (bdof_loss_grad reuses the tape for its own purposes and invalidates it). */
int bdof_tape_to_real(bdof_ctx* ctx, int i, int B, void* out);

/* Loss + gradient: replaces loss_grad = autograd.grad(calculate_loss,[0,1]) for the multislice part
 * (cnn_propagator/fullfield.py:93-106,329,345; cnn_propagator/ptychography.py:30-81,248,301).
 * meas: device float [B][NX][NY] = |measured| in this library's index order (far field: un-shifted).
 * loss = mean((|d|-meas)^2) is left on the device (bdof_get_loss); the gradient w.r.t. the rotated /
 * windowed (delta,beta) is left in the ctx (bdof_grot). out_wave may be NULL. */
int bdof_loss_grad(bdof_ctx* ctx, int B, const int* angle_of_b, const int* xoff, const int* yoff, const float* meas, void* out_wave);
int bdof_get_loss(bdof_ctx* ctx, double* loss);
/* Gradient w.r.t. the probe: with bdof_enable_probe_grad(1) every bdof_loss_grad also keeps G(psi_0) = dL/dRe psi_0 + i dL/dIm psi_0
 * of each wavefield; bdof_probe_grad sums it over the batch into out (device [NX][NY] complex, accumulate != 0: added to it).
 * The probe is shared by the wavefields of a minibatch, so this is the gradient of the loss w.r.t. (probe_real, probe_imag) —
 * the trainable probe of tensorflow_recon/fullfield.py:311-327,442-455 (probe_type='optimizable'). */
int bdof_enable_probe_grad(bdof_ctx* ctx, int enable);
int bdof_probe_grad(bdof_ctx* ctx, void* out, int accumulate);
/* mode 1: the `meas` arrays of bdof_loss_grad hold |measured| - |a0| instead of |measured| (a0: the plane-wave part handed
 * to bdof_set_probe; every transfer-function step has unit modulus at DC, so |a0| is the carrier's modulus at the detector
 * too).  The residual is then formed as (|a + e| - |a|) - (m - |a|) with |a + e| - |a| evaluated without cancellation —
 * three times more accurate gradients for plane-wave illumination.  Real-space detectors (none / near) and a scalar carrier
 * only; mode 0 (default): plain amplitudes.  bdof_loss_grad_conv honours it too: there the constant part of the detector
 * wave is A = s a_S with s the corner-pixel renormalisation of propagation.py:79,109-110, formed in float64 per call. */
int bdof_set_meas_mode(bdof_ctx* ctx, int mode);
/* The data term bdof_loss_grad and bdof_loss_grad_tf_f64 minimise (sticky on the ctx; default BDOF_LOSS_LSQ, whose results this
 * call does not move by a bit).  BDOF_LOSS_POISSON: the photon-counting likelihood of amplitudes m measured with `multiplier`
 * photons per unit intensity (mu; tensorflow_recon/ptychography.py's poisson_multiplier), as its deviance, per pixel with a = |d|
 *     L = mean( mu (a^2 - m^2 - 2 m^2 ln(a / m)) )          (m = 0: mu a^2)
 * — the reference's commented mu a^2 - mu m^2 ln(mu a^2) minus its value at a perfect fit: the same gradient, zero at a = m and
 * ~ 2 mu (a - m)^2 near it, where the raw form carries a constant of order mu ln mu per pixel that hides the loss's relative
 * change.  Seed G(d) = (2 mu / n) (1 - m^2 / a^2) d: the least-squares seed times mu (a + m) / a, so the residual a - m is
 * formed exactly as for BDOF_LOSS_LSQ (residual splitting, float64 carrier field, float64 DC bin).  Pixels with a = 0 contribute
 * nothing; there is no epsilon.  bdof_get_loss returns L.  multiplier must be > 0 (it is ignored by BDOF_LOSS_LSQ).
 * With BDOF_LOSS_POISSON set, bdof_loss_grad_conv, bdof_loss_grad_conv_f64 and bdof_field_loss_seed fail (bdof_last_error). */
#define BDOF_LOSS_LSQ 0
#define BDOF_LOSS_POISSON 1
int bdof_set_loss(bdof_ctx* ctx, int kind, double multiplier);

/* Detector weights: one plane w >= 0 (finite, float32) shared by every measurement of the run — a property of the detector: dead
 * and hot pixels, a beamstop, module gaps (w = 0), or a per-pixel confidence.  With l the per-pixel term of the data term set by
 * bdof_set_loss (least squares: (|d| - m)^2; Poisson: the deviance above) and B wavefields of NX NY pixels
 *     L    = sum(w l) / (B NX NY)          — the divisor stays the pixel count, NOT sum(w)
 *     G(d) = w (the unweighted seed)
 * for bdof_loss_grad (every engine) and bdof_loss_grad_tf_f64; the far field's float64 DC bin carries w as well (a beamstop on it
 * leaves exactly no adjoint carrier).  w == 1 everywhere gives the results of no weights bit for bit, and so does clearing them.
 * w: HOST pointer to [NX][NY] floats in the index order of ONE wavefield of `meas` — real-space detectors [x][y], far field the
 * un-shifted [ky][kx]; the library copies it into a buffer the ctx owns.  NULL clears the weights; bdof_configure clears them too
 * (the shape may change), and before bdof_configure the call is a state error.
 * A pixel with w = 0 takes no part only if its amplitude is finite (0 NaN is NaN): the caller zeroes `meas` where w == 0 before
 * it uploads (MultisliceEngine.meas_layout does).
 * With weights set, bdof_loss_grad_conv, bdof_loss_grad_conv_f64 and bdof_field_loss_seed fail (bdof_last_error). */
int bdof_set_detector_weights(bdof_ctx* ctx, const float* w);

/* Detector planes: D >= 1 near-field planes per wavefield, at distances z_0 .. z_{D-1} behind the exit wave (propagation-based
 * phase contrast recorded at several distances, holotomography).  With psi the wave that enters the detector step — phi_{S-1}
 * under numpy_skip_last, P phi_{S-1} under tf_all — and P(z_j) the step with plane j's transfer function
 *     d_j  = P(z_j) psi                                    j = 0 .. D-1, in the order given
 *     L    = sum_j sum(l(d_j, m_j)) / (B D NX NY)          — the data term of bdof_set_loss as the mean over B D frames;
 *                                                            the seed scale is 2 / (B D NX NY)
 *     G(psi) = sum_j P(z_j)^H G(d_j)                       — the sweep back through the object is unchanged
 * hs_det: HOST [D][ky][kx] complex64 tables, each as bdof_set_physics takes its one hs_det (un-shifted, 1/(NX NY) folded in);
 * hdet00: HOST [D] complex128 DC values (re, im) of the un-folded tables.  Valid after bdof_set_physics with BDOF_DET_NEAR.
 * With D > 1 set, `meas` of bdof_loss_grad and `out_wave` of bdof_forward / bdof_loss_grad are [B][D][NX][NY]; detector
 * weights stay one plane, shared by all D; residual splitting carries over (every transfer function has unit modulus at DC).
 * D = 1, or hs_det = NULL, goes back to the one plane of bdof_set_physics, whose results this call does not move by a bit; so
 * do bdof_configure and bdof_set_physics (the planes do not survive them).  D outside [1, BDOF_MAX_PLANES]: BDOF_ERR_ARG.
 * Carried by the streaming engine (two-kernel and fused sweeps, slice binning) and the generic engine; the resident engine is
 * not taken.  Everything else refuses, with "detector planes" in bdof_last_error: BDOF_CFG_RECOMPUTE, BDOF_CFG_ADJOINT64 and
 * bdof_loss_grad_tf_f64, the real-space propagator (bdof_*_conv*), a carrier field (bdof_set_probe_stack /
 * bdof_set_probe_field), the range calls (bdof_forward_range*, bdof_adjoint_range, bdof_set_range_carrier), and a detector
 * mode other than BDOF_DET_NEAR. */
#define BDOF_MAX_PLANES 8
int bdof_set_detector_planes(bdof_ctx* ctx, int D, const float* hs_det, const double* hdet00);

/* Probe modes (mixed states): a beam that is not fully coherent, or a fly scan smeared along its path, records the INCOHERENT sum
 * of M >= 1 orthogonal probe modes P_0 .. P_{M-1} (Thibault & Menzel; Adorym's n_probe_modes).  For window j of a batch of B
 *     psi_{j,m} = the multislice model under probe P_m          one sweep per (window, mode), the model of every other call
 *     d_{j,m}   = the detector step of psi_{j,m}                none / near field / far field, as bdof_set_physics set it
 *     a_j       = sqrt( sum_m |d_{j,m}|^2 )                     per pixel
 *     L         = sum_j sum_pix w l(a_j, m_j) / (B NX NY)       l: the data term of bdof_set_loss, w: the detector weights; the
 *                                                               divisor is the number of measured pixels, NOT times M
 *     G(d_{j,m}) = f_j d_{j,m}                                  f_j: the data term's one factor per pixel (for least squares
 *                                                               (2 / (B NX NY)) w (a_j - m_j) / a_j), formed once in float64 and shared
 *                                                               by the modes; a_j = 0 gives 0, there is no epsilon
 * The volume gradient is the sum over the modes of each sweep's k Im / -k Re (conj(phi) G(phi)); the gradient w.r.t. mode m is
 * sum_j G(psi_{0; j,m}).  M = 1 is the model of bdof_set_probe_field.  A mode that is identically zero contributes nothing, and
 * a unitary mix P'_m = sum_n U_mn P_n leaves L and the volume gradient unchanged.
 * bdof_set_probe_modes: probes HOST [M][NX][NY] complex128; hT / hdetT as for bdof_set_probe_field.  The library builds, on the
 * device in float64, M carrier stacks and M float64 detector carriers with the code bdof_set_probe_field builds its one with
 * (the float32 and transposed detector planes of the single probe have no reader under modes and are not built); they live beside
 * the probe of bdof_set_probe* and take its place while they are in force.  M = 0 or probes = NULL removes the modes and goes back
 * to whatever bdof_set_probe* last set, whose results this call does not move by a bit; bdof_configure and bdof_set_physics drop
 * the modes too (the carriers were propagated with the physics that go).  M outside [0, BDOF_MAX_MODES]: BDOF_ERR_ARG.
 * With modes in force B of bdof_forward and bdof_loss_grad stays the number of WINDOWS: angle_of_b, xoff, yoff and meas stay [B];
 * out_wave, where given, is [M][B][NX][NY] detector waves (frames in the order of meas); B M <= Bmax, else BDOF_ERR_ARG — a
 * wavefield per (window, mode) is swept and taped, so the tape costs M times what it costs without modes.  After bdof_loss_grad
 * bdof_grot holds [B][S][NX][NY] with the modes ALREADY SUMMED: bdof_rotation_adjoint, bdof_window_rotation_adjoint,
 * bdof_window_stack_adjoint, bdof_window_position_grad and the rotate_*_adjoint / _param_grad calls run on it unchanged.
 * bdof_probe_grad_modes: out device [M][NX][NY] complex, the sum over the windows of G(psi_0) per mode (accumulate != 0: added to
 * what is there); needs bdof_enable_probe_grad(1) before the bdof_loss_grad.  bdof_probe_grad refuses under modes.
 * Carried by the LDS-resident engine — at every batch size, whenever the size has a resident plan and the ctx allows the engine —
 * and otherwise by the generic engine: both loss kinds, detector weights, both variants, all three detector modes.  Everything
 * else refuses with BDOF_ERR_STATE and "probe modes" in bdof_last_error: a ctx whose only engine is the streaming one (a
 * power-of-two size without a resident plan, or BDOF_CFG_NO_RESIDENT, unless BDOF_CFG_GENERIC), BDOF_CFG_RECOMPUTE,
 * BDOF_CFG_ADJOINT64, BDOF_CFG_NO_GROT, slice binning, detector planes, the real-space propagator (bdof_*_conv*), the float64
 * twins (bdof_set_tf_f64 / bdof_loss_grad_tf_f64), the range calls (bdof_forward_range*, bdof_adjoint_range,
 * bdof_set_range_carrier / bdof_range_carrier_build), bdof_forward(keep_tape) and bdof_set_meas_mode(1). */
#define BDOF_MAX_MODES 8
int bdof_set_probe_modes(bdof_ctx* ctx, int M, const double* probes, const double* hT, const double* hdetT);
int bdof_probe_grad_modes(bdof_ctx* ctx, void* out, int accumulate);

/* The adjoint carrier the last bdof_loss_grad left (far-field detector under a plane-wave probe on the streaming and generic
 * engines): per wavefield the float64 seed of the DC bin, gcar[b], and conj(a_end) gcar[b], gt0[b] — HOST arrays of B complex
 * doubles (re, im).  Returns 1 and fills them where the configuration carries the DC seed that way, 0 (nothing written) where it
 * does not, < 0 on an error.  For checks: a detector weight of 0 on the DC bin (a beamstop) leaves both exactly 0. */
int bdof_adjoint_carrier(bdof_ctx* ctx, int B, double* gcar, double* gt0);

/* Real-space truncated-kernel propagator: replaces multislice_propagate_cnn (cnn_propagator/propagation.py:18-133), the
 * forward model cnn_propagator/fullfield.py:87,102 and ptychography.py:74 literally call.  The cropped kernel is separable,
 * K[p][q] = e * ky[p] * kx[q] (ky, kx: HOST complex arrays of ks taps, ks odd <= 33); ksum = sum of K (the factor of the
 * padding constant per slice, propagation.py:104); k = 2*np.pi*delta_nm/lambda_nm (propagation.py:25).  The detector step
 * and the probe are those of bdof_set_physics / bdof_set_probe.  bdof_forward_conv / bdof_loss_grad_conv mirror
 * bdof_forward / bdof_loss_grad (same arguments, gradient left in bdof_grot). */
int bdof_set_conv(bdof_ctx* ctx, const float* ky, const float* kx, int ks, double e_re, double e_im, double ksum_re,
                  double ksum_im, double k);
/* Optional, after bdof_set_conv: the same taps in float64 (HOST complex128 arrays of ks taps, and e).  The library then keeps
 * BDOF_TW_DITHER (default 64) copies of the float32 taps whose roundings average to these values and runs slice z with copy
 * z mod D, as it does with the transform constants of the transfer-function path (bdof_configure) — the taps are the same small
 * perturbation of every slice otherwise.  A no-op with BDOF_TW_DITHER=0. */
int bdof_set_conv_taps_f64(bdof_ctx* ctx, const double* ky, const double* kx, double e_re, double e_im);
/* Carrier FIELD of the real-space propagator, for a probe with no dominant constant part (a localised ptychography probe —
 * what cnn_propagator/ptychography.py:74-76 runs): stack = HOST [S + 1][NX][NY] complex64, the probe carried through EMPTY
 * space by the same padded convolution, p_0 = probe, p_{z+1} = K * pad(p_z, edge_z), edge_{z+1} = sum(K) edge_z, edge_0 = 1
 * (propagation.py:79-104 without an object), computed by the host in float64; det64 = HOST [NX][NY] complex128, the detector
 * plane of p_S before the renormalisation (no detector: p_S; near field: one transfer-function step of it; far field: its
 * un-shifted, un-normalised fft2 indexed [ky][kx]); p0 / pS: the corner pixels p_0[0,0], p_S[0,0] in float64 (the
 * renormalisation s = probe[0,0] / psi_S[0,0,0], propagation.py:109-110, is formed against them).  The wave is then carried as
 * psi_z = p_z + eps_z, eps zero-padded, and |d| - m is taken in float64 against s * det64.  Call bdof_set_probe with a zero
 * array and a0 = 0 first, and again after every bdof_set_conv.  NULL, NULL removes the stack. */
int bdof_set_conv_probe_stack(bdof_ctx* ctx, const float* stack, const double* det64, double p0_re, double p0_im, double pS_re, double pS_im);
/* The same loss + gradient entirely in float64 (bdof_conv64.h): the reference differentiates this forward model in float64
 * (autograd on numpy float64, cnn_propagator/ptychography.py:248,301), and for far-field ptychography the float32 kernels stop at
 * 1.5e-5 of its reconstructed delta (golden vector G14) — all of it in the wake of the corner pixel through which the
 * renormalisation of propagation.py:109-110 feeds sum(G conj q) back into the stack.  An accuracy path for the first minibatch of
 * an epoch (adjoint_precision='first-step'), unfused: every slice's pad + 'valid' convolution is one rocFFT double-precision
 * transform pair on the padded (N + ks - 1)^2 grid (overlap-save; its adjoint the circular correlation of the embedded adjoint
 * field), everything else point-wise in double.  bdof_set_conv_f64: probe host complex128 [NX][NY]; khat host complex128
 * [M][M], M = N + ks - 1: fft2 of the kernel zero-padded to M x M, transposed to [kx][ky], / M^2; ksum = sum of its taps; k as
 * for bdof_set_conv.  bdof_loss_grad_conv_f64: meas as for bdof_loss_grad_conv (+ meas_ref, what the host subtracted under
 * bdof_set_meas_mode(1)); loss by bdof_get_loss; gradient rows in bdof_grot.  Square fields; detector none or far field — a
 * near-field detector (propagation.py:122-127: one transfer-function step of the renormalised exit wave) after
 * bdof_set_conv_f64_detector(ctx, hdetT): host complex128 [kx][ky], ifftshift(H_det) / (NX NY). */
int bdof_set_conv_f64(bdof_ctx* ctx, const double* probe, const double* khat, int ks, double ksum_re, double ksum_im, double k);
int bdof_loss_grad_conv_f64(bdof_ctx* ctx, int B, const int* angle_of_b, const int* xoff, const int* yoff, const float* meas,
                            double meas_ref);
int bdof_set_conv_f64_detector(bdof_ctx* ctx, const double* hdetT);
/* The transfer-function model (cnn_propagator/np_funcs.py:15-65) in float64 on the same context: what autograd differentiates in
 * the reference (cnn_propagator/ptychography.py:248,301; fullfield.py:329,345) — modulation from the (delta, beta) rows, the step
 * after a slice as one rocFFT double-precision transform pair with H in float64, detector step (none / near field / far field),
 * magnitude loss, adjoint sweep.  Unfused; the accuracy path for the first minibatch of an epoch (adjoint_precision='first-step')
 * and a float64 twin of the fused kernels on the device.  bdof_set_tf_f64: probe host complex128 [NX][NY]; hT / hdetT (NULL
 * without a near-field detector): host complex128 [kx][ky], ifftshift(H) / (NX NY); k as for bdof_set_physics.
 * bdof_loss_grad_tf_f64: arguments as bdof_loss_grad_conv_f64; loss by bdof_get_loss, gradient rows in bdof_grot.
 * bdof_set_physics, bdof_set_probe and bdof_set_conv drop what either float64 path was handed (it described the previous model):
 * hand it over again after them, or the float64 calls fail with BDOF_ERR_STATE. */
int bdof_set_tf_f64(bdof_ctx* ctx, const double* probe, const double* hT, const double* hdetT, double k);
int bdof_loss_grad_tf_f64(bdof_ctx* ctx, int B, const int* angle_of_b, const int* xoff, const int* yoff, const float* meas, double meas_ref);
int bdof_forward_conv(bdof_ctx* ctx, int B, const int* angle_of_b, const int* xoff, const int* yoff, void* out_wave);
int bdof_loss_grad_conv(bdof_ctx* ctx, int B, const int* angle_of_b, const int* xoff, const int* yoff, const float* meas, void* out_wave);
void* bdof_grot(bdof_ctx* ctx);      /* device [B][S][NX][NY] pairs */
/* Field `slot` of the ctx's tape, device [Bmax][NX][NY] complex64 (NULL: no tape, or no such slot), as the last sweep left it; for
 * inspection and tests.  After a bdof_loss_grad that ran the fused forward sweep (bdof_sweep_fused) slot z <= S-2 holds the
 * real-space scattered part of phi_z, the wave behind slice z of np_funcs.py:37-40 less its constant part, and slot S-1 psi_hat_{S-1};
 * after the two-kernel sweep slot z holds psi_hat_{z+1}.  When the fused adjoint sweep ran too (bdof_adjoint_fused) the odd slots
 * z <= S-3 hold the same values in tile blocks, [b][NY / T][NX][T] with T = max(16, 4096 / NX) rows of y per tile: entry
 * ((b NY / T + y / T) NX + x) T + y % T is phi_z[b][x][y].  Even slots keep [b][x][y]. */
void* bdof_tape_slot(bdof_ctx* ctx, int slot);
/* Read-only view of the table of modulation factors c - 1 = exp(i k delta) exp(-k beta) - 1 that every sweep reads: one entry per
 * (delta, beta) pair of the bound object, in the object's own order.  Builds the table if it is stale (the pass the sweeps run),
 * with the k of bdof_set_physics or of the last sweep (the real-space propagator's differs).  table: the device address, n: its
 * length in float2 entries; mean_m1 (nullable, [2]): the mean factor minus one that the host forms the carrier scalars from —
 * with slice binning that of a bin, cbar^bin - 1; (0, 0) when no mean rides on the carrier (no plane-wave part in the probe, a
 * carrier field, the real-space propagator).  Valid until the object, the physics or the probe change.  BDOF_ERR_STATE without
 * an object or without physics, and when the object was bound by bdof_set_object_bilinear and the physics or the probe changed
 * since (there are no (delta, beta) rows to build the table from: bind it again).  Domain and accuracy of the factors: DESIGN §5. */
int bdof_modulation_table(bdof_ctx* ctx, const void** table, size_t* n, double* mean_m1);

/* Adjoint of the rotation gather: gvol[dest][y] (+)= scale * sum over the batch of the rows gathered
 * from dest.  gvol: device [n_dest][NY] pairs. */
int bdof_rotation_adjoint(bdof_ctx* ctx, int B, const int* angle_of_b, void* gvol, int accumulate, float scale);
/* The same for destination rows [row0, row0 + n_rows) only (gvol is still the base of the whole gradient volume): lets
 * the host pipeline rotation adjoint -> all-reduce -> Adam slab by slab, hiding them behind the collective
 * (comm.Allreduce(this_grads, grads), cnn_propagator/fullfield.py:348-351). */
int bdof_rotation_adjoint_rows(bdof_ctx* ctx, int B, const int* angle_of_b, void* gvol, int row0, int n_rows, int accumulate,
                               float scale);

/* Bilinear rotation — the TF twin's tf_rotate(obj, theta, interpolation='BILINEAR') (tensorflow_recon/fullfield.py:96; the cnn
 * variant's nearest-neighbour tables are the fused path of bdof_set_object).  vol: device [NXv][NZv][NYv] pairs; prm: DEVICE
 * float64 [B][4] = (cos, sin, x_off, y_off) of tf.contrib.image.angles_to_projective_transforms for images of height NXv and
 * width NZv: output pixel (h, w) = (x, z) samples the input at (sin w + cos h + y_off, cos w - sin h + x_off), zeros outside.
 * out_rows: device [B][NZv][NXv][NYv] pairs — hand it to bdof_set_object(out_rows, B*NZv*NXv, NYv, NULL, 0, 0) as a batch of
 * already rotated objects.  The adjoint takes the rotated-frame gradient bdof_grot() back to volume rows [row0, row0+n_rows)
 * of gvol (deterministic gather; same slab interface as bdof_rotation_adjoint_rows). */
int bdof_rotate_bilinear(bdof_ctx* ctx, const void* vol, int NXv, int NZv, int NYv, const double* prm, int B, void* out_rows);
/* The two calls above in one pass (what FullfieldSolver(rotation='bilinear') runs every step): the B rotated objects are
 * written straight into the ctx's table of modulation factors exp(i k (delta + i beta) dz) - 1 and bound as the batch's objects
 * — no rotated (delta, beta) copy, no second pass over B volumes.  The volume must be (NX, S, NY) of the configured wavefields.
 * conv != 0: factors for the real-space propagator's k (bdof_set_conv), which the conv entry points then use. */
int bdof_set_object_bilinear(bdof_ctx* ctx, const void* vol, int NXv, int NZv, int NYv, const double* prm, int B, int conv);
int bdof_rotate_bilinear_adjoint(bdof_ctx* ctx, const void* grot, int NXv, int NZv, int NYv, const double* prm, int B, void* gvol, int row0,
                                 int n_rows, int accumulate, float scale);

/* Trilinear rotation under an arbitrary rigid map per batch element (laminography tilt, axis roll, centre of rotation, per-angle
 * wobble) and its exact adjoint: the 3-D counterpart of the three calls above, with the same semantics, layouts, admission rules
 * and state.  vol: device [NXv][NZv][NYv] pairs; prm: DEVICE float64 [B][12], the rows of (M | t): output voxel o = (x, z, y) of
 * rotated object b samples the volume at p = M o + t in index coordinates (x', z', y'), trilinearly over the 8 surrounding
 * voxels, a tap outside the volume counting 0 (scipy.ndimage.affine_transform(order=1, mode='grid-constant', cval=0)).
 * Coordinates are formed in float64, a weight is the float32 product of three float32 factors; the adjoint uses the forward's
 * weights bit for bit and is a deterministic gather (no atomics: slab-wise, whole-volume and repeated calls give the same bits).
 * PRECONDITION: M is orthonormal with det +1.  The adjoint finds the outputs that touch a voxel in the box |o - M^T (v' - t)|_i <
 * sum_j |M_ji|, which holds because M preserves distances; prm is a device pointer, so the library cannot check it (the Python
 * layer does, util.check_rigid).  With a sheared or scaled M the adjoint silently misses contributions.
 * out_rows: device [B][NZv][NXv][NYv] pairs, as for bdof_rotate_bilinear.  bdof_set_object_rigid is bdof_rotate_rigid +
 * bdof_set_object in one pass (the volume must be (NX, S, NY) of the configured wavefields; the object is bound as modulation
 * factors, so bdof_rotation_adjoint_adam and, after a change of physics or probe, bdof_modulation_table refuse it exactly as
 * they refuse bdof_set_object_bilinear's).  bdof_rotate_rigid_adjoint keeps the slab interface (row0, n_rows, accumulate, scale).
 * BDOF_ERR_SIZE: an odd NY, NXv * NZv * NYv or B * NXv * NZv of 2^31 or more. */
int bdof_rotate_rigid(bdof_ctx* ctx, const void* vol, int NXv, int NZv, int NYv, const double* prm, int B, void* out_rows);
int bdof_set_object_rigid(bdof_ctx* ctx, const void* vol, int NXv, int NZv, int NYv, const double* prm, int B, int conv);
int bdof_rotate_rigid_adjoint(bdof_ctx* ctx, const void* grot, int NXv, int NZv, int NYv, const double* prm, int B, void* gvol, int row0,
                              int n_rows, int accumulate, float scale);
/* The derivative of the loss with respect to the map itself, from what the three calls above leave on the device: the volume, the
 * rows prm and the rotated-frame gradient grot ([B][NZv][NXv][NYv] pairs; NULL: the ctx's own, bdof_grot()).  With o~ = (x, z, y, 1)
 *     out[b][a][j] = sum_o q_a(o) o~_j,   q_a(o) = sum_c grot_c(o) dV_c/dp_a (p(o)),   a in (x', z', y'), j in 0..3,
 * the layout of prm: DEVICE float64 [B][12] (accumulate != 0: added to what is there).  dV/dp_a is taken inside the cell floor(p)
 * of the forward map — over its 8 corners, -1 or +1 by the corner's bit along a, times the other two axes' factors, times V(corner),
 * a corner outside the volume counting 0.  A point ON a lattice plane belongs to the cell floor gives it, so it takes the
 * RIGHT-HAND derivative; at zero tilt and roll that is every voxel's y.  Weights, tap sums and q_a in float32 (the forward's cell
 * and fractions, bit for bit), the sums over voxels in float64, in per-workgroup records whose number and rows depend on
 * (NXv, NZv) only, added in a fixed order without atomics: element b has the same bits alone, in a batch and in a repeated call.
 * Shape rules and error codes are bdof_rotate_rigid_adjoint's (BDOF_ERR_SIZE: an odd NY, the 2^31 limits). */
int bdof_rotate_rigid_param_grad(bdof_ctx* ctx, const void* vol, const void* grot, int NXv, int NZv, int NYv, const double* prm, int B,
                                 double* out /* DEVICE [B][12] */, int accumulate);

/* Ptychography: adjoint of rotate + zero-pad + per-position window (cnn_propagator/ptychography.py:32-34,42-73) for a
 * batch whose elements all use rotation angle `angle` and windows at (xoff[b], yoff[b]); gvol: device [n_dest][volNY] pairs. */
int bdof_window_rotation_adjoint(bdof_ctx* ctx, int B, int angle, const int* xoff, const int* yoff, void* gvol,
                                 int accumulate, float scale);

/* Ptychography windows at FRACTIONAL origins (sub-pixel probe positions): the window stack, its exact adjoint and the derivative
 * of the loss with respect to the origins.  Window size (NX, NY) and depth S are the configured wavefield's.  Rotated frame
 * R[z][xg][y] = row tab[z][xg] of vol (rows of volNY pairs; tab: DEVICE [S][volNX], the table of the batch's ONE angle), zero
 * outside.  origin: DEVICE float64 [B][2] = (u_b, v_b), the pixel coordinate of window b's first voxel along x and along y:
 *     i0 = floor(u), fx = u - i0;  j0 = floor(v), fy = v - j0       (in float64; a negative origin floors downwards)
 *     W_b[z][i][j] = sum_{a,c in {0,1}} wx_a wy_c R[z][i0 + i + a][j0 + j + c],   wx = (1 - fx, fx), wy = (1 - fy, fy)
 * with the factors rounded to float32 and a weight their float32 product wx_a wy_c; a tap of weight 0 or outside the volume is
 * skipped, so at fx = fy = 0 the window is the integer cut of the sweeps' index math, value for value.  All three calls form
 * (i0, j0, weights) with one function: the same bits.
 * bdof_window_stack writes out_rows, device [B][S][NX][NY] pairs — a batch of already rotated objects for
 * bdof_set_object(ctx, out_rows, B S NX, NY, NULL, 0, 0) — and records (volNX, volNY) in the ctx as the rotated frame of the windows.
 * bdof_window_stack_adjoint: grot (device [B][S][NX][NY] pairs; NULL: the ctx's own, bdof_grot()) -> gvol, device [n_dest][volNY]
 * pairs, as bdof_window_rotation_adjoint: first pad[z][xg][y] = sum_b sum_{a,c} wx_a wy_c grot_b[z][xg - i0_b - a][y - j0_b - c], a
 * deterministic gather in the fixed order (j0, then b, then a, then c), then the rotation adjoint of `pad` under angle `angle` of
 * the tables of bdof_set_rotation_adjoint (which it needs; a bound table it does NOT need: the bound object is the stack).  The
 * rotated frame is that of the last bdof_window_stack (BDOF_ERR_STATE without one).  gvol = scale * result (+ gvol with
 * accumulate != 0).  More than BDOF_WIN_MAXLIST = 1024 windows on one column of the rotated frame (a window touches NX + 1
 * columns): BDOF_ERR_SIZE, checked on the host before anything is launched — nothing is ever dropped silently.
 * bdof_window_position_grad: out, DEVICE float64 [B][2] = (dL/du_b, dL/dv_b) (accumulate != 0: added to what is there),
 *     dL/du_b = sum_{z,i,j} sum_channels grot_b[z][i][j] sum_c wy_c (R[z][i0+i+1][j0+j+c] - R[z][i0+i][j0+j+c])
 * and the same with x and y exchanged for dL/dv_b, taken INSIDE the cell floor gives: an origin on a lattice line takes the
 * RIGHT-HAND derivative, as bdof_rotate_rigid_param_grad does.  Taps and products in float32, sums over voxels in float64 in
 * per-workgroup records whose number and rows depend on (S, NX) only, added in a fixed order without atomics: element b has the
 * same bits alone, in a batch and in a repeated call.
 * BDOF_ERR_SIZE: an odd NY (of the windows or of the volume), volNX * S * volNY or B * S * NX of 2^31 or more. */
int bdof_window_stack(bdof_ctx* ctx, const void* vol, int volNX, int volNY, const int* tab, const double* origin /* DEVICE [B][2] */, int B,
                      void* out_rows);
int bdof_window_stack_adjoint(bdof_ctx* ctx, const void* grot, int angle, const double* origin, int B, void* gvol, int accumulate,
                              float scale);
int bdof_window_position_grad(bdof_ctx* ctx, const void* vol, int volNX, int volNY, const int* tab, const void* grot, const double* origin,
                              int B, double* out /* DEVICE [B][2] */, int accumulate);

/* Fused regulariser gradient + Adam + mask + clip on a volume [NXv][NZv][NYv] of pairs.
 * Replaces cnn_propagator/fullfield.py:109-118 (gradient of the L1 + TV terms), apply_gradient_adam
 * (cnn_propagator/util.py:280-291) and the constraints of fullfield.py:359-362.  g is the data-term
 * gradient summed over ranks; g_scale = 1/size (fullfield.py:351). */
int bdof_adam_step(bdof_ctx* ctx, const void* x_old, void* x_new, const void* g, void* m, void* v, const float* mask,
                   int NXv, int NZv, int NYv, float g_scale, float alpha_d, float alpha_b, float gamma,
                   float lr, float b1, float b2, float eps, int i_batch, int clip);
/* The same for the slab x in [x0, x0 + nx) of the [X][Z][Y] volume (all pointers are still those of the whole volume). */
int bdof_adam_step_slab(bdof_ctx* ctx, const void* x_old, void* x_new, const void* g, void* m, void* v, const float* mask,
                        int NXv, int NZv, int NYv, float g_scale, float alpha_d, float alpha_b, float gamma,
                        float lr, float b1, float b2, float eps, int i_batch, int clip, int x0, int nx);

/* The tail of a step on ONE rank in one pass over the volume: bdof_rotation_adjoint_rows, bdof_adam_step and the table of
 * modulation factors of x_new, without writing the volume gradient and reading it and x_new back.  The arguments are those of
 * the two calls; gvol may be NULL (the gradient is then not kept; otherwise it is stored as well, the bits of
 * bdof_rotation_adjoint_rows).  m, v, x_new come out bit for bit as from the two calls, the table as from the pass
 * bdof_set_object(x_new) would trigger; its mean is summed in another (fixed) order: per destination row over its lanes, then over
 * chunks of 1024 rows, then over the chunks; longest addition chain D = max(2 ceil(NY / 128) + 6, 2 ceil(NY / 512) + 9) + 4 + 8 +
 * ceil(ceil(n_dest / 1024) / 256) + 8 (35 for 512^3), so it
 * may differ from that pass's in the last bits of a double (by at most (D + 2) 2^-53 mean|factor|).
 * BDOF_ERR_STATE for what the call does not carry: accumulate != 0, a row range other than the whole volume, the bilinear
 * rotation (an object bound by bdof_set_object_bilinear), no object bound as (delta, beta) rows; BDOF_ERR_ARG when x_new aliases
 * x_old or [NXv][NZv][NYv] is not the bound object's shape.
 * Whose table the ctx holds afterwards: the ctx records the address x_new (with its row count and NY).  The object bound before
 * stays bound but its table is stale (a sweep without rebinding rebuilds it).  The NEXT bdof_set_object consumes the record: if
 * it binds exactly that address, row count and NY, the table is taken over and the next sweep builds none (it only reads the
 * mean back); any other bdof_set_object, and every later one on the same address, rebuilds as always — so "call again whenever
 * that memory has been modified" keeps holding.  The record is dropped by bdof_memcpy_h2d / bdof_memset / bdof_memcpy_d2d into
 * that memory, bdof_set_object_bilinear and any rebuild of the table; a taken-over table is rebuilt when k changes or the probe /
 * propagator change whether the mean rides on the carrier. */
int bdof_rotation_adjoint_adam(bdof_ctx* ctx, int B, const int* angle_of_b, void* gvol, int row0, int n_rows, int accumulate, float scale,
                               const void* x_old, void* x_new, void* m, void* v, const float* mask, int NXv, int NZv, int NYv,
                               float g_scale, float alpha_d, float alpha_b, float gamma, float lr, float b1, float b2, float eps,
                               int i_batch, int clip);

/* dst[b] = src[idx[b]] for B fields of bytes_per_field bytes (a multiple of 4; 16-byte copies when it is a multiple of 16;
 * idx: device int32 [B]) in one launch:
 * this_prj_batch = prj[this_ind_batch] (cnn_propagator/fullfield.py:344) on the device-resident stack of amplitudes. */
int bdof_gather_fields(bdof_ctx* ctx, void* dst, const void* src, const int* idx, int B, size_t bytes_per_field);

/* Value of the regulariser terms of the loss (cnn_propagator/fullfield.py:109-118; total_variation_3d, util.py:61-70) on a
 * volume [NXv][NZv][NYv] of pairs: sums[0] = sum|delta|, sums[1] = sum|beta|, sums[2] = TV(delta) (periodic, anisotropic).
 * The caller weights them (alpha_d, alpha_b, gamma).  Synchronous (three numbers come back). */
int bdof_regularizer_value(bdof_ctx* ctx, const void* x, int NXv, int NZv, int NYv, double* sums);

/* Fourier shell correlation of two volumes (tensorflow_recon/util.py:975-1048, fourier_shell_correlation / fourier_ring_correlation):
 * the per-shell sums from which the host forms the curve and its thresholds.  vol_a, vol_b: DEVICE volumes [NXv][NZv][NYv] of
 * (delta, beta) pairs, the solvers' layout; they may be the same pointer, neither is written.  out: HOST [n_shells][7], row s =
 *   n_points of shell s,
 *   sum Re(F_a conj F_b), sum |F_a|^2, sum |F_b|^2 of the delta channel,
 *   the same three sums of the beta channel,
 * F the unnormalised discrete Fourier transform over the axes longer than 1 (one of length 1: rings of 2-D arrays), computed in
 * float64: each volume is widened to complex128 delta + i beta, one rocFFT transform C gives both channels, F_delta(k) =
 * (C(k) + conj C(-k)) / 2 and F_beta(k) = (C(k) - conj C(-k)) / (2i).  Sums, not ratios: sum_s |F_a|^2 = N sum a^2 (Parseval).
 * Shells are hard and exact.  With Nref the shortest and L the least common multiple of the axes longer than 1, w = L / Nref,
 * and the signed index k_i = j for j < (N_i + 1) / 2, else j - N_i: u = 4 sum (k_i L / N_i)^2 in 64-bit integers, and the
 * point lies in the shell s with (2s - 1)^2 w^2 <= u < (2s + 1)^2 w^2 (s = 0 for u < w^2) — s = floor(rho + 1/2), rho = Nref |f|,
 * f in cycles per voxel; on a cube the rounded index radius.  The reference's shells have Gaussian-blurred edges around the same
 * centre line; those are not reproduced.  Points of a shell >= n_shells are dropped.
 * No floating-point atomics: the same call gives the same bits.  Synchronous (host numbers come back); needs no bdof_configure.
 * The ctx keeps the complex128 workspace (16 bytes per voxel and distinct volume), the plan and rocFFT's work area from the first
 * call until it is destroyed or configured again.
 * BDOF_ERR_SIZE: L > 2^30, fewer than two axes longer than 1, Nref < 4, n_shells < 1. */
int bdof_shell_correlation(bdof_ctx* ctx, const void* vol_a, const void* vol_b, int NXv, int NZv, int NYv, int n_shells, double* out);

/* ---- analytic starting volume for full field (csrc/bdof_fbp.h; DESIGN §3 "Analytic start") ----
 * Contrast-transfer-function retrieval and Ram-Lak filter of B angles at once.  meas: DEVICE amplitudes [B][D][NX][NY] float32, D
 * detector planes per angle in the layout the full-field solver stages; wgt: DEVICE [NX][NY] float32 weight plane or NULL — where
 * it is 0 the contrast is 0 whatever meas holds there (NaN included); a0_sq = |a0|^2 of the plane-wave probe; filters: DEVICE
 * complex128 [D][kx][ky] in the un-shifted index order of the transforms, G_d = conj(C_d) / (sum_d |C_d|^2 + regulariser) / (NX NY)
 * with C_d the (in general complex, Hermitian) transfer of the projected quantity to the contrast of plane d (analytic.ctf_transfer).
 *   g_d = m_d^2 / a0_sq - 1 (double, from the float32 amplitude),   P = sum_d Re F^-1(G_d F g_d)   (double-precision rocFFT, any NX, NY),
 *   q[b][x][y] = sum_x' h[x - x'] P[b][x'][y],  h[0] = 1/4, h[m] = -1 / (pi^2 m^2) for odd m, 0 for even m != 0
 * — the exact real-space Ram-Lak filter along x, the frame zero outside itself (no padding, no wrap-around), summed in float64 and
 * rounded once: q is float32 [B][NX][NY].  The ctx keeps the complex128 work area (B D NX NY 16 bytes), grown on demand, until it
 * is destroyed or configured again (it lies with the buffers bdof_configure replaces).  Needs no bdof_configure.
 * BDOF_ERR_ARG: D outside [1, BDOF_MAX_PLANES], a0_sq not finite or <= 0.  BDOF_ERR_SIZE: NX > 4096, B D NX NY of 2^31 or more. */
int bdof_ctf_retrieve(bdof_ctx* ctx, const void* meas, const void* wgt, double a0_sq, const void* filters, int B, int D, int NX, int NY,
                      void* q);

/* Back-projection of B filtered frames q [B][NXd][NYd] (float32) through rigid maps prm (DEVICE float64 [B][12], the rows of
 * (M | t) of bdof_rotate_rigid: beam-frame voxel o = (x, z, y) samples the volume at p = M o + t) into destination rows
 * [row0, row0 + n_rows) of the volume [NXv][NZv][NYv] of (delta, beta) pairs (row = x' NZv + z'; the slab interface of
 * bdof_rotate_rigid_adjoint):
 *   vol[p] (+)= (scale_delta, scale_beta) sum_b w_b bilinear(q_b; o_x, o_y),   o = M_b^T (p - t_b),   w: DEVICE float32 [B].
 * The detector's size is independent of the volume's; a tap outside the detector counts 0.  Coordinates in float64, the two
 * bilinear factors per axis, their product and the four-tap sum in float32; each channel's sum over b in float32 in ascending b as
 * acc = fmaf(scale w_b, s_b, acc), from 0 or, with accumulate, from what the volume holds — so a call per batch of angles with
 * accumulate from the second on forms the very sum of one call over all of them.  A gather without atomics: slab-wise,
 * whole-volume and repeated calls give the same bits.  Needs no bdof_configure.
 * BDOF_ERR_SIZE: NXv NZv NYv or NXd NYd of 2^31 or more.  BDOF_ERR_ARG: rows outside the volume. */
int bdof_backproject(bdof_ctx* ctx, const void* q, int NXd, int NYd, const double* prm, const float* w, int B, void* vol, int NXv, int NZv,
                     int NYv, int row0, int n_rows, int accumulate, float scale_delta, float scale_beta);

/* vol = max(vol, 0) * mask over n voxels of (delta, beta) pairs, in place (mask: DEVICE float32 [n] or NULL): the clip and the
 * finite-support mask every initial guess goes through (cnn_propagator/fullfield.py:258-262), for a volume formed on the device. */
int bdof_volume_clip_mask(bdof_ctx* ctx, void* vol, const float* mask, size_t n);

/* Shrink-wrap (cnn_propagator/fullfield.py:365-368): mask[i] *= (delta[i] > thresh) over n voxels. */
int bdof_mask_shrink(bdof_ctx* ctx, const void* x, float* mask, size_t n, float thresh);

/* Sub-batch streams of the fused FFT engine.  A batch whose tiles (B*NX/16 workgroups per launch) cover at least the
 * chip's resident workgroup slots is split in groups that run the same kernel sequence concurrently on side streams
 * (no dependencies between wavefields of one minibatch: fullfield.py:95-103 is a plain loop over the batch), so the
 * partly filled last round of one launch is covered by the other group's kernels.  n = -1 automatic (1 or 2 groups),
 * 1..4 fixed.  bdof_batch_groups returns the number of groups a batch of B wavefields runs as. */
int bdof_set_streams(bdof_ctx* ctx, int n);
int bdof_batch_groups(bdof_ctx* ctx, int B);

/* Fused forward sweep of bdof_loss_grad (streaming engine).  The Fresnel transfer function of np_funcs.py:42 (cnn_propagator/
 * util.py:73-102) is separable, H(u, v) = Hx(u) Hy(v), so the slice chain of np_funcs.py:37-43 regroups into kernels that work on
 * lines of one direction — "finish the previous step along my lines, modulate, start the next step along my lines" — one launch and
 * one trip of the wavefield through memory per slice where the two-kernel sweep takes two (32 instead of 40 B per pixel and slice).
 * mode: 0 never, 1 the forward sweep (the adjoint sweep reads the phi tape it leaves); 2 is accepted and runs 1, the highest
 * stage this switch carries (the fused adjoint sweep has a switch of its own, bdof_set_adjoint_fusion below).  A new ctx starts at 0: the two routes agree to float32 rounding, not bit for
 * bit, and callers of this ABI compare bdof_loss_grad bit for bit with the tape-free adjoint (BDOF_CFG_RECOMPUTE), whose forward
 * sweep is not fused; the full-field solver of the Python host switches to the highest stage.  The fused route is taken where the configuration is
 * eligible: tape (not BDOF_CFG_RECOMPUTE), no slice binning, scalar carrier, BDOF_DET_NONE / BDOF_DET_NEAR, no window offsets, no
 * probe gradient, S even and >= 4, NX, NY <= 512, and a transfer function that bdof_set_transfer_f64 found separable in float64
 * while it built its dithered copies (BDOF_H_DITHER below 2 builds none: no fused route then)
 * (max |H[ky][kx] H[0][0] - H[ky][0] H[0][kx]| <= 1e-14 |H[0][0]|^2).  Everything else runs the two-kernel sweep, as does every
 * other entry point.  bdof_sweep_fused: the mode the last bdof_loss_grad actually ran (0 before the first). */
int bdof_set_sweep_fusion(bdof_ctx* ctx, int mode);
int bdof_sweep_fused(bdof_ctx* ctx);
/* The fused adjoint sweep of bdof_loss_grad: below the top slice one kernel per slice, on lines of alternating direction, through
 * the transposes of the separable steps (40 B per pixel and slice where the two-kernel adjoint moves 56).  A switch of its own
 * beside bdof_set_sweep_fusion, whose modes and query stay what they were: on = 1 takes the route wherever the fused forward sweep
 * runs (bdof_set_sweep_fusion(1) and an eligible configuration), on = 0 (a new ctx) never.  The forward sweep then leaves its odd
 * tape slots in tile blocks (bdof_tape_slot); its arithmetic, the loss and the detector wave do not change.  The gradient rows
 * agree with the two-kernel adjoint's to float32 rounding.  bdof_adjoint_fused: 1 if the last bdof_loss_grad ran the fused adjoint
 * sweep (0 before the first, and after every other configuration). */
int bdof_set_adjoint_fusion(bdof_ctx* ctx, int on);
int bdof_adjoint_fused(bdof_ctx* ctx);

/* Per-kernel-class timing with HIP events on the stream of each launch (bench.py roofline leg).  enable = 0 off, 1 every launch,
 * n > 1 every n-th launch of the per-slice kernel classes (two event records per launch cost ~9 us of stream time). */
int bdof_profile_enable(bdof_ctx* ctx, int enable);
int bdof_profile_read(bdof_ctx* ctx, int kernel_class, int* n_launches, double* total_ms);

/* ---- Collectives: the gradient exchange of the data-parallel loop ------------------------------------------------
 * Replaces comm.Allreduce(this_grads, grads) (mpi4py, host float64 buffers: cnn_propagator/fullfield.py:348-351,
 * ptychography.py:302-306) with RCCL over xGMI on device float32 buffers, one process per GPU.  librccl is opened at
 * run time by the first bdof_comm_* call; single-GPU use never loads it.
 *   bdof_comm_unique_id   rank 0 makes the 128-byte id (ncclGetUniqueId); the host hands it to every rank over any
 *                         channel it likes (the Python host: a unix-domain socket rendezvous, comm.py);
 *   bdof_comm_create      ncclCommInitRank on `device` (collective: every rank calls it);
 *   bdof_allreduce_grad   in-place SUM of `count` floats;
 *   bdof_reduce_scatter_grad / bdof_allgather_volume   in place on a buffer of nranks * count_per_rank floats: after the
 *                         reduce-scatter rank r holds the sum in its part [r*count, (r+1)*count); the all-gather
 *                         distributes every rank's part — the "reduce-scatter -> Adam on 1/N -> all-gather" form of
 *                         the step, same wire bytes as the all-reduce and 1/N of the Adam traffic;
 *   bdof_bcast_volume     in-place broadcast from `root` (initial guess of rank 0, ptychography.py:169-208).
 * Every collective runs on the communicator's own stream, ordered BEHIND the work the ctx stream holds at the call, and
 * returns a ticket; bdof_comm_wait(comm, ctx, ticket) makes the ctx stream wait for it (stream-side, no host block), so
 * kernels enqueued between the two calls overlap the transfer.  Tickets are a ring of 256.  Errors: 1000 + ncclResult_t,
 * text via bdof_comm_last_error (NULL: the error of a failed create / unique_id). */
typedef struct bdof_comm bdof_comm;
int bdof_comm_unique_id(void* id, size_t bytes);
int bdof_comm_create(bdof_comm** out, int device, int nranks, int rank, const void* id, size_t bytes);
void bdof_comm_destroy(bdof_comm* comm);
const char* bdof_comm_last_error(const bdof_comm* comm);
int bdof_comm_size(const bdof_comm* comm);
int bdof_comm_rank(const bdof_comm* comm);
int bdof_allreduce_grad(bdof_comm* comm, bdof_ctx* ctx, void* buf, size_t count, int* ticket);
int bdof_reduce_scatter_grad(bdof_comm* comm, bdof_ctx* ctx, void* buf, size_t count_per_rank, int* ticket);
int bdof_allgather_volume(bdof_comm* comm, bdof_ctx* ctx, void* buf, size_t count_per_rank, int* ticket);
int bdof_bcast_volume(bdof_comm* comm, bdof_ctx* ctx, void* buf, size_t count, int root, int* ticket);
int bdof_comm_wait(bdof_comm* comm, bdof_ctx* ctx, int ticket);
int bdof_comm_sync(bdof_comm* comm);

/* Device memory helpers for hosts without an allocator of their own.  bdof_malloc allocates on the calling thread's
 * current device, bdof_ctx_malloc on the ctx's device. */
int bdof_ctx_malloc(bdof_ctx* ctx, void** ptr, size_t bytes);
int bdof_device_mem(bdof_ctx* ctx, size_t* free_bytes, size_t* total_bytes);   /* hipMemGetInfo of the ctx's device */
int bdof_malloc(void** ptr, size_t bytes);
int bdof_free(void* ptr);
int bdof_memcpy_h2d(bdof_ctx* ctx, void* dst, const void* src, size_t bytes);
int bdof_memcpy_d2h(bdof_ctx* ctx, void* dst, const void* src, size_t bytes);
int bdof_memset(bdof_ctx* ctx, void* dst, int value, size_t bytes);
int bdof_memcpy_d2d(bdof_ctx* ctx, void* dst, const void* src, size_t bytes);   /* asynchronous on the ctx stream */

#ifdef __cplusplus
}
#endif
#endif
