/*
 * mrx.h -- C ABI of libmrx, the MI355X (gfx950) implementation of maria's
 * atmospheric-turbulence + time-ordered-data (TOD) synthesis hot path.
 *
 * The reference (thomaswmorris/maria) is pure Python and has no FFI for this
 * path; the entry points below are what a ctypes binding placed at the
 * reference's own Python seams would call.  Each function cites the reference
 * code (file:line under maria/) whose arithmetic it replaces.
 *
 * Conventions
 *  - every function returns 0 (MRX_OK) or a negative mrx_status; nothing throws.
 *    mrx_last_error(ctx) returns a human-readable message for the last failure.
 *  - the CALLER owns every buffer.  Pointers named d_* are DEVICE pointers
 *    (e.g. torch-ROCm tensor.data_ptr()); everything else is host memory that
 *    is only read during the call.
 *  - all work is enqueued on the HIP stream bound with mrx_set_stream()
 *    (default: the null stream); no call synchronises the device except
 *    mrx_read_flags() and mrx_synchronize().
 *  - one mrx_ctx per host thread per device.
 *  - coarse (atmosphere-rate) arrays are TIME-MAJOR: index [t * D + d] with
 *    D = detector rows of this shard; the full-rate TOD is DETECTOR-MAJOR
 *    [d * ld + s], the reference's (ndet, nt) layout (sim/atmosphere.py:72-82).
 */
#ifndef MRX_H_
#define MRX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRX_VERSION 150 /* 0.2.0 (120): mrx_spline_upsample_fused, mrx_allgather_tod_p2p, mrx_exchange_screens,
                           mrx_resample_columns; MRX_OPT_SAMPLE_TILES retired.  130: mrx_screen_amplitudes,
                           mrx_screen_desc.d_amp, mrx_screen_generate_3d(..., d_amp), mrx_streams_concurrent.
                           131: mrx_coarse_to_krj_keep_tail.  140: mrx_screen_desc.periodic_beam,
                           mrx_noise_generate_krj, the noise generator's two-rate form.  141: mrx_atm_synthesize,
                           MRX_FLAG_HANDOVER.  142: mrx_atm_synthesize_krj, MRX_OPT_WRITER_PER_TILE.  150: mrx_map_cal.steps_per_tile
                           (the struct's reserved word), MRX_OPT_GAUSS_ACCUM, MRX_OPT_SYNTH_ACQUIRE; mrx_map_sample reads a map
                           of less than 2 GiB through a context-owned copy */

typedef enum mrx_status {
  MRX_OK = 0,
  MRX_ERR_INVALID = -1,  /* bad argument (null pointer, non-positive size ...) */
  MRX_ERR_HIP = -2,      /* a HIP runtime call failed; see mrx_last_error    */
  MRX_ERR_NO_DEVICE = -3,
  MRX_ERR_UNSUPPORTED = -4, /* shape outside what the kernels are built for  */
  MRX_ERR_ALLOC = -5
} mrx_status;

/* bits of the device flag word written by the sampling kernel */
#define MRX_FLAG_SCREEN_OOB 1u /* a line of sight left a layer's screen: the
                                  reference raises RuntimeError "introduced nans"
                                  (atmosphere/atmosphere.py:368-369)            */
#define MRX_FLAG_TABLE_OOB 2u  /* (pwv, el) left the emission table: jax fill
                                  value NaN (band/band.py:283-286); not raised for
                                  a sample whose pwv is NaN because it left a screen */
#define MRX_FLAG_NAN 4u        /* a NaN reached the output                      */
#define MRX_FLAG_HANDOVER 8u   /* mrx_atm_synthesize: a writer gave up waiting for the sampler (its bound of
                                  ~seconds; the call's TOD is then invalid)     */

typedef struct mrx_ctx mrx_ctx;
typedef struct mrx_atm_plan mrx_atm_plan;
typedef struct mrx_comm mrx_comm;

/* ---- context ------------------------------------------------------------ */

int mrx_version(void);
/* Creates a context on HIP device `device`.  Fails with MRX_ERR_NO_DEVICE when
 * no gfx950 device is visible: there is no CPU fallback in this library. */
int mrx_init(int device, mrx_ctx** ctx);
int mrx_destroy(mrx_ctx* ctx);
/* Bind the hipStream_t all later calls enqueue on (pass NULL for the null
 * stream).  The stream stays owned by the caller. */
int mrx_set_stream(mrx_ctx* ctx, void* hip_stream);
/* Do kernels on the context's stream and on `other_stream` (a hipStream_t) run side by side?  HIP spreads
 * the streams of a process round-robin over a few hardware queues (four by default); two streams on one
 * queue take turns, whatever the events between them say.  A caller that pipelines work over two streams
 * (DevicePath.run: the sampler of block b+1 beside the writer of block b) asks this once and takes another
 * stream when the answer is 0 -- one new stream in four shares the current stream's queue, and the
 * pipelined step then runs as slowly as the serial one (2.9 instead of 2.1 ms).  Two 150 us spin kernels, timed;
 * synchronises both streams.  The library's own side streams (mrx_noise_generate) are chosen the same way. */
int mrx_streams_concurrent(mrx_ctx* ctx, void* other_stream, int* concurrent);
int mrx_synchronize(mrx_ctx* ctx);
/* Options (default 0).
 *  MRX_OPT_POINTING_CHAIN = 1: mrx_atm_sample follows the reference's float32
 *    chain literally (atan2 -> phi, asin -> theta, tan/cos/sin of those).  The
 *    default evaluates the same ground projection directly from the unit
 *    line-of-sight vector: equal up to the float32 rounding noise of the chain,
 *    better conditioned near the zenith, and ~3x fewer instructions.
 *  MRX_OPT_AXIS_LITERAL = 1: mrx_atm_sample finds cell and weight on every screen axis with
 *    jax's float32 rule (searchsorted on the float32 nodes, weight (x - lo)/(hi - lo)), also on
 *    uniform axes.  The default computes the position in pixels on axes whose uniform hint
 *    verified (a float64 anchor per step and layer + the lane's float32 offset from it, good to
 *    ~4e-6 pixel): equal to the literal rule up to the float32 rounding of the reference's own
 *    coordinates (~2e-4 pixel, ~1e-8 of the loading), at a third of the instructions.
 *    MRX_OPT_POINTING_CHAIN implies the literal rule.
 *  MRX_OPT_SAMPLE_TIMES = 1|2|4: coarse time steps per thread in mrx_atm_sample
 *    (tuning; 0 = library default). */
enum {
  MRX_OPT_POINTING_CHAIN = 0,
  MRX_OPT_AXIS_LITERAL = 1,
  MRX_OPT_SAMPLE_TIMES = 2,
  MRX_OPT_SAMPLE_CHUNK = 3, /* time steps per workgroup (tuning; 0 = automatic) */
  MRX_OPT_UPSAMPLE_GROUPS = 4, /* 16-row detector tiles per workgroup of the TOD
                                  writer (tuning; 0 = automatic) */
  MRX_OPT_NOISE_GENERIC = 5, /* bit 0: the LDS second pass even where the register one applies;
                                bit 1: the Stockham first pass even where the radix-16 register
                                one applies; bit 2: the lanes' first batches of equal length
                                (tests, A/B runs) */
  MRX_OPT_SAMPLE_WGS_PER_CU = 6, /* mrx_atm_sample runs as a resident grid of this many workgroups
                                    per CU that walk the work items (tuning; 0 = default, 8) */
  MRX_OPT_WRITER_PER_TILE = 7, /* 1: mrx_spline_upsample_fused launches one workgroup per tile instead of a resident
                                  grid over a tile queue (the default, 6 % faster alone): for a launch that shares the
                                  chip with kernels launched after it on another stream -- a resident grid never makes
                                  room for them.  (Slot of the retired MRX_OPT_SAMPLE_TILES.) */
  MRX_OPT_NOISE_LANES = 8, /* streams mrx_noise_generate spreads its batches over (1..4; 0 = automatic:
                              up to 4, each with at least 128 detectors of the work buffer) */
  MRX_OPT_SCREEN_STOCKHAM = 9, /* 1: the screen generator's transforms as LDS Stockham passes even
                                  where the register transforms apply (tests, A/B runs) */
  MRX_OPT_SYNTH_WGS_PER_CU = 10, /* mrx_atm_synthesize: resident workgroups per CU of its one grid (1..5; 0 = as many as
                                    fit, 5).  Timing sweeps, and the tests' way to vary who runs beside whom */
  MRX_OPT_SYNTH_TILE_ORDER = 11, /* mrx_atm_synthesize: 0 = the tiles of a detector block time tile by time tile (all its row groups
                                    side by side: the writers follow the samplers a few chunks behind); 1 = row group by row group, the
                                    time tiles of a row group in a row (the order the chip stores fastest; a block's tiles then wait
                                    for the whole block: give block_rows) */
  MRX_OPT_GAUSS_ACCUM = 12, /* mrx_gauss_smooth2d / mrx_map_smooth: 0 = float32 products summed over 16 taps and those sums
                               in float64 from radius 16 on (<= 1e-6 of scipy's float64 sums, twice as fast), scipy's float64
                               arithmetic below; 1 = float64 always ("exact": <= 2.5e-7, float32 roundings of the result);
                               2 = the blocked sums at every radius */
  MRX_OPT_SYNTH_ACQUIRE = 13, /* mrx_atm_synthesize: 1 = a writer tile's workgroup runs an agent-scope acquire (and waits for it)
                                 once the chunks it needs are in, before it loads them -- the hand-over form that is valid
                                 whatever a CU holds; 0 (default) = write-through stores, drained waves and sc1 loads alone,
                                 measured valid and 2 % faster */
  MRX_OPT_WRITER_GENERAL = 14, /* mrx_spline_upsample_fused / mrx_atm_synthesize: 1 = the writer's row loop reads a row's
                                  coefficients once per SAMPLE everywhere; 0 (default) = once per thread and row in every
                                  wave whose threads' four samples each lie in one knot interval.  Same bits either way:
                                  the A/B switch and the tests' reference */
  MRX_OPT_COUNT = 15
};
int mrx_set_option(mrx_ctx* ctx, int option, int value);
const char* mrx_last_error(const mrx_ctx* ctx);
/* Device properties the host side sizes launches with. */
int mrx_device_info(const mrx_ctx* ctx, int* n_cu, int* lds_bytes_per_cu,
                    size_t* hbm_bytes, char* name, int name_len);

/* HIP-event timer on the bound stream (bench.py's live kernel timing; a
 * torch.cuda.Event only sees torch's own current stream). */
int mrx_timer_start(mrx_ctx* ctx);
int mrx_timer_stop(mrx_ctx* ctx, float* elapsed_ms); /* synchronises */

/* ---- turbulent layer stack + emission tables (the "plan") ---------------- */

/* One turbulent layer = one smoothed screen on a rectilinear grid in the
 * process frame (atmosphere/atmosphere.py:317-373).  A line of sight with
 * unit-height ground projection (px, py) (coords/coordinates.py:333-349,
 * z = 1) hits the layer at
 *     e = h*(px*r00 + py*r10) + d_off_e[t]
 *     c = h*(px*r01 + py*r11) + d_off_c[t]
 * where (r..) is process.transform (utils/rotations.py:45-77) and
 * d_off_*[t] = (cumsum(timestep*(vx,vy,0)) + (0,0,h)) @ transform, columns 0/1
 * (atmosphere/atmosphere.py:318-319,346-347), evaluated by the host in f64. */
typedef struct mrx_layer {
  const float* d_values; /* [n_e][n_c] f32, smoothed screen (:341-344)        */
  const float* d_axis_e; /* [n_e] f32 grid nodes = float32(process.extrusion)  */
  const float* d_axis_c; /* [n_c] f32 = float32(process.cross_section[mask,0]) */
  const double* d_off_e; /* [Ta] f64                                           */
  const double* d_off_c; /* [Ta] f64                                           */
  int32_t n_e, n_c;
  double h;              /* layer.h, metres                                    */
  double r00, r10, r01, r11;
  /* Optional uniform-axis hint: the float64 grids behind the two axes are
   * extrusion[i] = e0 + i*de (np.arange, atmosphere.py:241-245) and
   * cross_section[i] = c0 + i*dc (np.linspace, :208-219).  When
   * float32(e0 + i*de) reproduces every node of d_axis_e to one float32 ulp (checked on
   * the device at plan creation; the float64 grid is itself rounded, so a node in ~1e5 parts
   * from the model by an ulp) the kernel works in pixel coordinates, (x - e0)/de in float64,
   * instead of searching the axis (see MRX_OPT_AXIS_LITERAL).  Set de / dc to 0 when unknown.
   * Screens of 2^22 nodes a side or 4 GiB and more take the general kernel. */
  double e0, de, c0, dc;
  float pwv_rms;         /* float32(layer.pwv_rms), extrusion.py:100-105       */
  int32_t reserved;
} mrx_layer;

/* Band-integrated emission table (band/band.py:264-286).  The reference does
 * a trilinear lookup at (T0, pwv, el) with scalar T0; the host passes the two
 * temperature slabs that bracket T0 and T0's normalised distance between them
 * so the kernel reproduces the reference's 8-term float32 sum term by term. */
typedef struct mrx_band_table {
  const float* d_values;   /* [2][n_pwv][n_el] f32: slab iT then slab iT+1    */
  const float* d_axis_pwv; /* [n_pwv] f32, spectrum.side_zenith_pwv (mm)      */
  const float* d_axis_el;  /* [n_el]  f32, spectrum.side_elevation (rad)      */
  int32_t n_pwv, n_el;
  float w_t;               /* float32 (T0 - T[iT]) / (T[iT+1] - T[iT])        */
  int32_t t_oob;           /* 1 if T0 lies outside the table (result NaN)     */
  /* interpolation_method="cubic" (band/band.py:288-300): the table interpolated linearly to
   * T0 (scipy interp1d, float64) and then scipy's RegularGridInterpolator(method="cubic") on
   * (pwv, el), i.e. the tensor-product not-a-knot cubic spline, float64.  The host expands
   * that spline into one bicubic polynomial per grid cell:
   *   d_cubic = [n_pwv float64 pwv nodes][n_el float64 el nodes]
   *             [(n_pwv-1)*(n_el-1) cells, row-major (pwv, el)][16]: c[4*k + m] multiplies
   *             (pwv - pwv_i)^m (el - el_j)^k.
   * NULL selects the linear (jax, float32) lookup above.  A sample outside the grid sets
   * MRX_FLAG_TABLE_OOB (scipy raises ValueError there). */
  const double* d_cubic;
} mrx_band_table;

/* Builds the device-resident plan from the layer and table descriptors (host
 * structs holding device pointers): packs the wind offsets of all layers
 * [n_t][n_layers], copies the band tables into one buffer (staged in LDS by the
 * kernel) and verifies the uniform-axis hints.  The screens (d_values) and axis
 * arrays must stay alive while the plan is in use; the screens may be
 * rewritten in place between calls (a new realisation), the rest may not.
 * n_t = length of every d_off_e / d_off_c array = Ta of mrx_atm_sample. */
int mrx_atm_plan_create(mrx_ctx* ctx, const mrx_layer* layers, int n_layers,
                        const mrx_band_table* tables, int n_tables, int n_t,
                        mrx_atm_plan** plan);
int mrx_atm_plan_destroy(mrx_ctx* ctx, mrx_atm_plan* plan);
/* Diagnostics: number of layer axes (0..2*n_layers) that passed the uniform
 * check, and whether the band tables fit the kernel's LDS stage. */
int mrx_atm_plan_info(mrx_ctx* ctx, const mrx_atm_plan* plan, int* uniform_axes,
                      int* tables_in_lds);

/* ---- hot path ------------------------------------------------------------- */

/* Fused coarse-rate sampling: detector pointing (coords/transforms.py:10-29 via
 * coordinates.py:378-386), ground projection (coordinates.py:333-349),
 * wind-advected bilinear gather through the layer stack
 * (atmosphere/atmosphere.py:346-373, jax RegularGridInterpolator "linear",
 * float32), emission lookup (band/band.py:264-286) and Mueller weight
 * (sim/atmosphere.py:64-65, array/array.py:204-218).
 *
 *  d_az, d_el     [Ta]  float32 coarse boresight (coordinates.py:286-304)
 *  d_dx, d_dy     [D]   float32 detector offsets (radians)
 *  d_band         [D]   table index of each detector row, 0 <= band < n_tables
 *  d_mueller00    [D]   mueller()[:,0,0]
 *  pwv0                 weather.pwv (mm)  (atmosphere.py:309)
 *  d_pwv          [Ta*D] f64 zenith-scaled pwv, time-major; may be NULL
 *  d_loading      [Ta*D] f32 band power in pW, time-major
 *  d_flags        one uint32 device word, OR-ed with MRX_FLAG_* (never cleared
 *                 by the kernel; clear it with mrx_clear_flags)
 */
int mrx_atm_sample(mrx_ctx* ctx, const mrx_atm_plan* plan, const float* d_az,
                   const float* d_el, int Ta, const float* d_dx,
                   const float* d_dy, const int32_t* d_band,
                   const float* d_mueller00, int D, double pwv0, double* d_pwv,
                   float* d_loading, uint32_t* d_flags);

int mrx_clear_flags(mrx_ctx* ctx, uint32_t* d_flags);
int mrx_read_flags(mrx_ctx* ctx, const uint32_t* d_flags, uint32_t* host_flags);

/* Not-a-knot cubic spline through the coarse samples of every detector:
 * scipy interp1d(kind="cubic") == make_interp_spline(k=3) as called at
 * sim/atmosphere.py:72-82.  Knots are uniform (coordinates.py:292,
 * np.arange).  Writes for every knot the pair (y, m) with m = h^2/6 * S''(x),
 * solved in float64, so that on [x_j, x_j+1], u = (x - x_j)/h:
 *   S = (1-u) y_j + u y_j+1 + ((1-u)^3 - (1-u)) m_j + (u^3 - u) m_j+1.
 *  d_y  [Ta*D] f32 time-major;  d_ym [Ta*D][2] f32 time-major.  Ta >= 4. */
int mrx_spline_prepare(mrx_ctx* ctx, const float* d_y, int D, int Ta,
                       float* d_ym);

/* Evaluates the spline at the full-rate sample times and writes the TOD
 * (sim/atmosphere.py:72-82, cast to float32), optionally scaled per detector
 * (gain error, sim/simulation.py:239-247; pW->K_RJ, tod/tod.py:106-142).
 * Beyond the last knot the last polynomial piece is extended, which is what
 * fill_value="extrapolate" does.
 *  ta0, dta       first coarse time and coarse step (s)
 *  d_t     [T]    f64 full-rate sample times, ascending
 *  d_scale [D]    f32 per-detector factor, or NULL
 *  d_rows  [D]    destination row of each detector, or NULL for the identity:
 *                 a caller that keeps its detectors in a locality order (see
 *                 maria_amd/pipeline.py) still gets the TOD in its own row order
 *  d_out          f32, element (d, s) at d_out[d * ld_out + s] */
int mrx_spline_upsample(mrx_ctx* ctx, const float* d_ym, int D, int Ta,
                        double ta0, double dta, const double* d_t, int T,
                        const float* d_scale, const int32_t* d_rows,
                        float* d_out, size_t ld_out);

/* mrx_spline_prepare + mrx_spline_upsample in ONE kernel (sim/atmosphere.py:72-82): the
 * writer reads the raw coarse samples d_y [Ta*D] f32 time-major -- mrx_atm_sample's
 * d_loading as it is -- and solves the second derivatives of the knots its own tile of
 * 1024 samples touches in the tile prologue (the same twisted factorisation, started
 * 16 knots outside the tile or at the true not-a-knot end).  No (y, m) buffer, no solve
 * launch.  Same result as the two-call form to float32 rounding of m (<= 1e-7 of y).
 * Arguments as mrx_spline_upsample.  A tile whose samples span more knots than the LDS
 * image holds (upsampling ratios T/Ta below ~4) is walked in segments: correct at any
 * ratio, fastest from ~18 up (maria's ratios: 5 at 50 Hz, 40 at 400 Hz). */
int mrx_spline_upsample_fused(mrx_ctx* ctx, const float* d_y, int D, int Ta,
                              double ta0, double dta, const double* d_t, int T,
                              const float* d_scale, const int32_t* d_rows,
                              float* d_out, size_t ld_out);

/* Atmosphere -> TOD for one observation in ONE launch: mrx_atm_sample followed by
 * mrx_spline_upsample_fused -- the reference's _simulate_atmosphere from the layer loop to the
 * interpolation at the sample rate (atmosphere/atmosphere.py:317-373, sim/atmosphere.py:43-82) --,
 * with the hand-over from the sampling to the writing on the device, TIME CHUNK by time chunk: one
 * resident grid takes sampler work items (a time chunk of 256 detectors) and TOD tiles (1024 samples
 * of 32 rows) from two queues; a tile is written once the two or three chunks around its samples are
 * in (a counter per chunk; write-through stores, an sc1 poll, a workgroup barrier, sc1 loads), and a
 * workgroup whose tile is not ready samples one work item instead of waiting, so the two kinds of
 * work balance themselves and the launch cannot stall whatever is resident.  The first TOD tile
 * starts after the first chunks instead of after a whole sampling launch, all detectors of a chunk
 * share one pass over the screens' footprint, and no launch boundary or stream event separates
 * anything.  Bit-identical to the two calls.
 *  block_rows        detectors per block of the coarse array, rounded up to a multiple of 256; <= 0:
 *                    the library's choice (mrx_atm_synthesize_block_rows tells) -- blocks of about 5 000
 *                    rows while the plan's screens fit the Infinity Cache, one block beyond (every block
 *                    walks the screens' track again), never more than 4 * Ta * rows < 2^31 allows (a block's
 *                    coarse array is addressed with 32-bit offsets)
 *  sampler_wgs       workgroups that ONLY sample while work items remain (they write afterwards);
 *                    <= 0: MRX_OPT_SAMPLE_WGS_PER_CU per CU (unset: 2).  The others write and sample
 *                    where they would wait
 *  d_coarse          f32, out (scratch the caller may read), 128-byte aligned, Ta * round_up(D, 32)
 *                    floats: the coarse loading in pW, block b (rows b*block_rows ...) as its own
 *                    time-major array at d_coarse + Ta * b * block_rows, [Ta][pitch] with
 *                    pitch = its rows rounded up to 32 (the columns past the last row: padding)
 *  d_pwv             f64, out, or NULL: the zenith-scaled pwv of every coarse sample (what mrx_atm_sample's
 *                    d_pwv receives: atmosphere.py:373; the map mixin's calibration reads it,
 *                    sim/map.py:117-135), block b as its own time-major array [Ta][rows of b] at
 *                    d_pwv + Ta * b * block_rows -- one [Ta][D] array where the rows are one block
 *  other arguments   as mrx_atm_sample (d_az ... pwv0, d_flags) and mrx_spline_upsample
 *                    (ta0 ... ld_out); MRX_OPT_SAMPLE_CHUNK: coarse steps per time chunk (unset: by size)
 * MRX_ERR_UNSUPPORTED (nothing launched) for plans or options the pixel-coordinate sampler
 * does not take -- a layer on a non-uniform axis, MRX_OPT_AXIS_LITERAL, MRX_OPT_POINTING_CHAIN,
 * bicubic band tables --: use the two calls there.  MRX_FLAG_HANDOVER in d_flags: see above. */
int mrx_atm_synthesize(mrx_ctx* ctx, const mrx_atm_plan* plan, const float* d_az, const float* d_el,
                       int Ta, const float* d_dx, const float* d_dy, const int32_t* d_band,
                       const float* d_mueller00, int D, double pwv0, float* d_coarse, int block_rows,
                       int sampler_wgs, uint32_t* d_flags, double ta0, double dta, const double* d_t, int T,
                       const float* d_scale, const int32_t* d_rows, float* d_out, size_t ld_out, double* d_pwv);

/* The rows per block mrx_atm_synthesize lays d_coarse (and d_pwv) out in for `block_rows` (<= 0: the library's
 * choice, which depends on the plan's screens: see the call) -- for a caller that reads the coarse arrays back. */
int mrx_atm_synthesize_block_rows(mrx_ctx* ctx, const mrx_atm_plan* plan, int D, int Ta, int block_rows, int* rows_out);

/* mrx_atm_synthesize with TOD.to("K_RJ") applied on the coarse grid (tod/tod.py:106-142 before the spline, as
 * mrx_coarse_to_krj does between the two calls -- same functions, same operands, same bits): the sampler role divides
 * every coarse sample by den_band(d)(el_det(d, j)) before it stores it, and the writer role then writes K_RJ at the
 * pW writer's cost.  Use it where mrx_coarse_to_krj applies (the caller bounds the form's error:
 * DevicePath.coarse_krj_bound).
 *  d_cal_dx, d_cal_dy [D]   detector offsets as the calibration holds them (mrx_coarse_to_krj's d_dx, d_dy)
 *  d_cal_axis_el [n_el], d_cal_values [n_bands][n_el], n_el, n_bands   as mrx_coarse_to_krj; the cell table
 *                           (16 (n_el - 1) n_bands bytes) must fit the launch's LDS beside the sampler's:
 *                           MRX_ERR_UNSUPPORTED otherwise
 *  d_tail_pw, tail_knots, ld_tail   as mrx_coarse_to_krj_keep_tail: the last tail_knots knots of every detector IN
 *                           pW, element (k, d) at d_tail_pw[k * ld_tail + d] (d: the row in this call's D), for the
 *                           samples past the last knot, which take the per-sample form; NULL / 0: not kept
 *  T                        the samples the writer role writes: those up to the last knot when a tail is kept
 *  d_coarse                 holds K_RJ afterwards */
int mrx_atm_synthesize_krj(mrx_ctx* ctx, const mrx_atm_plan* plan, const float* d_az, const float* d_el,
                           int Ta, const float* d_dx, const float* d_dy, const int32_t* d_band,
                           const float* d_mueller00, int D, double pwv0, float* d_coarse, int block_rows,
                           int sampler_wgs, uint32_t* d_flags, double ta0, double dta, const double* d_t, int T,
                           const float* d_scale, const int32_t* d_rows, float* d_out, size_t ld_out,
                           const float* d_cal_dx, const float* d_cal_dy, const float* d_cal_axis_el,
                           const float* d_cal_values, int n_el, int n_bands, float* d_tail_pw, int tail_knots,
                           size_t ld_tail, double* d_pwv);

/* mrx_spline_upsample fused with TOD.to("K_RJ") (tod/tod.py:106-142): each sample
 * is divided by den_b(el) = (0.5 if polarized else 1) * k_B * 1e12 *
 * Int tau_b(nu) exp(-opacity(nu)) dnu (calibration/functions.py:73-90,
 * band/band.py:235-255), looked up on the elevation axis at the detector's own
 * full-rate elevation, which the kernel recomputes from the full-rate boresight
 * elevation and the (rolled) detector offsets (sim/observation.py:55-58,
 * coords/transforms.py:14-28, float32).  The host collapses each band's
 * transmission-integral table at the observation's scalar base temperature and
 * zenith pwv (tod.py:94-97) onto the elevation axis:
 *  d_bore_el     [T]   float32 full-rate boresight elevation
 *  d_dx, d_dy    [D]   float32 offsets of observation.coords (rolled), radians
 *  d_band        [D]   band index of each detector row
 *  d_cal_axis_el [n_el] float32 elevation axis (rad); d_cal_values [n_bands][n_el]
 * A detector elevation outside the axis gives NaN, as jax's interpolator does. */
int mrx_spline_upsample_krj(mrx_ctx* ctx, const float* d_ym, int D, int Ta,
                            double ta0, double dta, const double* d_t, int T,
                            const float* d_scale, const int32_t* d_rows,
                            const float* d_bore_el, const float* d_dx,
                            const float* d_dy, const int32_t* d_band,
                            const float* d_cal_axis_el,
                            const float* d_cal_values, int n_el, int n_bands,
                            float* d_out, size_t ld_out);

/* TOD.to("K_RJ") applied to the COARSE loading before the spline: d_out[j * D + d] =
 * d_loading[j * D + d] / den_band(d)(el_det(d, j)), time-major like mrx_atm_sample's output,
 * with the detector elevation of coarse step j from the coarse boresight elevation (the same
 * float32 formula as mrx_spline_upsample_krj).  mrx_spline_prepare + mrx_spline_upsample of
 * d_out then give the K_RJ TOD at the pW writer's cost (HBM-bound instead of arithmetic-bound).
 * It is S[y / g] in place of the reference's S[y] / g (S the spline, g = den(el_det(t))): the
 * two differ by the spline's interpolation error on g alone -- g is smooth in time but for the
 * kinks where a detector's elevation crosses a node of the table's axis, where the error is at
 * most 0.25 x (jump of the relative slope of den at the node) x (elevation step per coarse
 * sample).  The caller bounds that on the host and takes mrx_spline_upsample_krj when it is
 * not far below the tolerance (maria_amd/pipeline.py: DevicePath.coarse_krj_bound).
 * d_out may be d_loading (conversion in place). */
int mrx_coarse_to_krj(mrx_ctx* ctx, const float* d_loading, int D, int Ta, const float* d_bore_el_coarse,
                      const float* d_dx, const float* d_dy, const int32_t* d_band,
                      const float* d_cal_axis_el, const float* d_cal_values, int n_el, int n_bands,
                      float* d_out);

/* The same, and the loading in pW of the last `tail_knots` coarse steps kept aside as it is read:
 * d_tail_pw[k * ld_tail + d] = d_loading[(Ta - tail_knots + k) * D + d].  The samples past the last
 * coarse knot are not written in the coarse form (an extrapolated spline of y / g is not the
 * reference's extrapolated spline of y, divided; maria/sim/atmosphere.py:72-82 extrapolates): the caller
 * converts them one by one from these knots (mrx_spline_prepare + mrx_spline_upsample_krj on the window),
 * and d_out may be d_loading.  d_tail_pw = NULL or tail_knots = 0: mrx_coarse_to_krj. */
int mrx_coarse_to_krj_keep_tail(mrx_ctx* ctx, const float* d_loading, int D, int Ta, const float* d_bore_el_coarse,
                                const float* d_dx, const float* d_dy, const int32_t* d_band,
                                const float* d_cal_axis_el, const float* d_cal_values, int n_el, int n_bands,
                                float* d_out, float* d_tail_pw, int tail_knots, size_t ld_tail);

/* TOD.to("K_RJ") of a field that is already at the full rate -- the noise (and later map /
 * cmb) fields, tod/tod.py:106-142 -- in place: d_data[row(d) * ld + s] *= d_scale[d] /
 * den_band(d)(el(d, s)), with the arguments of mrx_spline_upsample_krj. */
int mrx_tod_to_krj(mrx_ctx* ctx, float* d_data, size_t ld, int D, int T,
                   const float* d_scale, const int32_t* d_rows,
                   const float* d_bore_el, const float* d_dx, const float* d_dy,
                   const int32_t* d_band, const float* d_cal_axis_el,
                   const float* d_cal_values, int n_el, int n_bands);

/* The way back, TOD.to("pW") of a K_RJ field in place: d_data *= d_scale[d] * den(el(d, s));
 * same arguments.  (tests/noise/test_noise.py:14 converts the default-unit TOD this way.) */
int mrx_tod_from_krj(mrx_ctx* ctx, float* d_data, size_t ld, int D, int T,
                     const float* d_scale, const int32_t* d_rows,
                     const float* d_bore_el, const float* d_dx, const float* d_dy,
                     const int32_t* d_band, const float* d_cal_axis_el,
                     const float* d_cal_values, int n_el, int n_bands);

/* Full-rate detector pointing: Coordinates.broadcast at the sample rate
 * (coords/coordinates.py:378-386 via transforms.py:10-29, float32;
 * sim/observation.py:55-58).  d_az, d_el [T] float32 boresight; d_dx, d_dy [D];
 * outputs [D][ld_out] float32 azimuth and elevation (radians). */
int mrx_pointing_broadcast(mrx_ctx* ctx, const float* d_az, const float* d_el,
                           int T, const float* d_dx, const float* d_dy, int D,
                           float* d_az_out, float* d_el_out, size_t ld_out);

/* Linear upsample of the coarse pwv to the full rate
 * (sim/atmosphere.py:30-37, interp1d linear + extrapolate); only the map/cmb
 * mixins consume it.  d_pwv [Ta*D] f64 time-major -> d_out [D][ld_out] f32. */
int mrx_linear_upsample(mrx_ctx* ctx, const double* d_pwv, int D, int Ta,
                        double ta0, double dta, const double* d_t, int T,
                        float* d_out, size_t ld_out);

/* ---- screens -------------------------------------------------------------- */

/* Separable Gaussian filter with scipy.ndimage.gaussian_filter semantics
 * (order 0, mode="reflect", radius int(truncate*sigma+0.5), axis 0 then axis 1,
 * float64 accumulation, float32 storage between the passes).  Serves the
 * per-layer screen smoothing (atmosphere/atmosphere.py:341-344) and
 * ProjectionMap.smooth (map/projection.py:485-504).  A sigma <= 1e-15 skips
 * that axis as scipy does.  d_tmp is ny*nx floats of scratch; in == out is
 * allowed.
 * Non-finite input spreads as in scipy and no further: a NaN makes the pixels
 * whose window holds it NaN (+-radius per filtered axis, folded back at a
 * reflecting edge), an Inf makes them Inf of its sign (NaN where +Inf and -Inf,
 * or a pass's Inf and NaN, meet in one window); every other pixel is the finite
 * value scipy gives, to the bound of MRX_OPT_GAUSS_ACCUM.  A radius whose tile
 * does not fit the LDS (3574 along x or along a y that runs transposed, 238
 * along a directly filtered y) returns MRX_ERR_UNSUPPORTED before d_out is
 * written. */
int mrx_gauss_smooth2d(mrx_ctx* ctx, const float* d_in, float* d_out,
                       float* d_tmp, int ny, int nx, double sigma_y,
                       double sigma_x, double truncate);

/* Linear resampling of every row of a screen onto new column positions:
 *   d_out[e * ld_out + j] = d_scale[j] * ((1 - d_w[j]) * d_in[e * ld_in + d_idx[j]] + d_w[j] * d_in[e * ld_in + d_idx[j] + 1]).
 * model="3d": every layer of the one process has its own cross-section grid, coarser with height
 * (atmosphere/atmosphere.py:208-219, extrusion.py:20-22), while the layers are planes of one volume
 * generated on one grid; the host gives the bracketing column, the weight and a variance factor
 * (1 / sqrt((1-w)^2 + w^2 + 2 w (1-w) rho(step)): a linear blend of two unit-variance samples has
 * less than unit variance) per output column.  0 <= d_idx[j] <= n_in - 2. */
int mrx_resample_columns(mrx_ctx* ctx, const float* d_in, int n_e, int n_in, size_t ld_in, const int32_t* d_idx,
                         const float* d_w, const float* d_scale, int n_out, float* d_out, size_t ld_out);

/* ProjectionMap.smooth (map/projection.py:485-504): numer = G(data*weight),
 * denom = G(weight), out = denom > 0 ? numer/denom : 0; d_weight may be NULL
 * (weight == 1).  d_denom_out may be NULL.  d_tmp: 2*ny*nx floats.
 * A binned map's unhit pixels (NaN data, weight 0) behave as in the reference:
 * data*weight is NaN there, so out is NaN over that pixel's window and nowhere
 * else (mrx_gauss_smooth2d's non-finite rule, on numer and denom alike); an
 * infinite weight gives Inf / Inf = NaN over its window.  Give unhit pixels a
 * finite value (0) to have them ignored instead. */
int mrx_map_smooth(mrx_ctx* ctx, const float* d_data, const float* d_weight,
                   float* d_out, float* d_denom_out, float* d_tmp, int ny,
                   int nx, double sigma_y, double sigma_x);

/* Turbulent screen generator: Philox-4x32-10 normals on the Hermitian half of k
 * space, times the square root of the Matern / von Karman spectrum
 *     PSD(k) ~ (k0^2 + |k|^2)^-(nu + 1),  k0 = sqrt(2 nu)/r0
 * (functions/__init__.py:30-39 is the covariance this is the transform of),
 * then a 2-D complex-to-real inverse FFT scaled to unit variance.  Replaces the
 * autoregressive generator (atmosphere/process.py:191-209) with a different
 * algorithm of the same target covariance; parity is statistical.
 * Spectrum cell (ky, kx), 0 <= kx <= nx/2, is amp(k) (a + i b)/sqrt 2 with (a, b) the
 * Box-Muller pair of Philox words (0,1) [ky < ny/2] or (2,3) [ky >= ny/2] of
 * counter (kx, ky mod ny/2, stream, 0), key = seed; the columns kx = 0 and nx/2 are
 * made Hermitian in ky from their cells ky < ny/2 (cells ky = 0, ny/2: amp a).
 * ny, nx powers of two in [64, 8192].
 *
 * mrx_screen_generate_batch makes n_screens screens that share one FFT domain (the
 * layers of an atmosphere) in two launches, with the beam smoothing of
 * atmosphere/atmosphere.py:341-344 (scipy.ndimage.gaussian_filter: reflect, truncate 4)
 * folded in: along y on the half spectra between the two FFT passes, along x on the
 * finished row; float32 accumulation (equal to mrx_gauss_smooth2d of the unsmoothed
 * screen to ~1e-6 of its rms) -- or, per screen (periodic_beam), as a factor of the spectrum.  Only the top-left out_ny x out_nx block of the
 * periodic domain is smoothed and written (reflection at ITS edges): a layer may use a
 * larger FFT domain than its grid so that opposite edges decorrelate. */
typedef struct mrx_screen_desc {
  float* d_out;            /* [out_ny][ld_out] f32                                  */
  uint32_t stream;         /* Philox stream of this screen (the layer index)        */
  int32_t out_ny, out_nx;  /* written block; 0 = the whole domain                   */
  int32_t periodic_beam;   /* 0: the beam as scipy applies it to the written block (reflection at its
                              edges).  1: the same truncated, normalised taps as a convolution on the
                              PERIODIC FFT domain, folded into the spectrum (the two stencils, a quarter
                              of the generator's arithmetic, disappear): pixels at least the stencil
                              radius int(4 sigma + 0.5) from every edge of the written block are the
                              same to rounding, nearer ones see the field beyond the edge instead of its
                              mirror image.  For callers whose lines of sight keep that distance.      */
  size_t ld_out;           /* row pitch in floats; 0 = out_nx                        */
  double dy, dx;           /* grid steps (m)                                         */
  double r0, nu;           /* outer scale (m), Matern smoothness                     */
  double sigma_y, sigma_x; /* beam sigma in pixels along y / x; 0 = no smoothing     */
  const float* d_amp;      /* amplitude table of mrx_screen_amplitudes for this FFT domain
                              (dy, dx, r0, nu are then ignored), or NULL: the power law */
} mrx_screen_desc;
/* floats of scratch for n_screens screens: 2 * n_screens * (nx/2 + 1) * (ny + 16) */
int mrx_screen_work_floats(int ny, int nx, int n_screens, size_t* floats);
int mrx_screen_generate_batch(mrx_ctx* ctx, uint64_t seed, int ny, int nx,
                              const mrx_screen_desc* screens, int n_screens,
                              float* d_work, size_t work_floats);
/* model="3d" (atmosphere/atmosphere.py:28,141-279, extrusion.py:69-77): ONE process holds many
 * layers whose turbulence is correlated vertically -- a Matern(nu = 1/3, r0) field in three
 * dimensions, PSD(k) ~ (k0^2 + |k|^2)^-(nu + 3/2), sampled on the layers' heights.  Three transform
 * passes on a periodic nh x ny x nx domain (powers of two; nh in [8, 2048]): along h per (ky, kx)
 * cell, keeping only the requested height planes (linear interpolation between the two FFT planes
 * around plane_pos[p], in units of dh from plane 0, times plane_scale[p] -- the caller's variance
 * correction 1/sqrt((1-w)^2 + w^2 + 2 w (1-w) rho(dh)), or NULL); then the two passes of
 * mrx_screen_generate_batch per plane, with the beam smoothing folded in.  `planes[p]` gives each
 * plane's output block and beam (d_out, out_ny, out_nx, ld_out, sigma_y, sigma_x; the other fields are
 * ignored).  Cell (kz, ky, kx) uses Philox counter (kx, ky, stream << 16 | kz mod nh/2, 0x33440000). */
int mrx_screen3d_work_floats(int nh, int ny, int nx, int n_planes, size_t* floats);
int mrx_screen_generate_3d(mrx_ctx* ctx, uint64_t seed, uint32_t stream, int nh, int ny, int nx,
                           double dh, double dy, double dx, double r0, double nu,
                           const double* plane_pos, const double* plane_scale,
                           const mrx_screen_desc* planes, int n_planes, float* d_work,
                           size_t work_floats, const float* d_amp);

/* A flat-sky CMB patch: T, Q, U on a periodic ny x nx domain (powers of two in [64, 8192]) of square pixels of
 * `res` radians, Lx = nx res, Ly = ny res,
 *     m_X(x_j) = sum_k a_X(k) exp(i k.x_j),   k = 2 pi (fx / Lx, fy / Ly), signed integer fx, fy,   l = |k|.
 * Per cell of the half plane kx = 0 .. nx/2, with g1, g2, g3 independent unit complex Gaussians (E |g|^2 = 1):
 *     T = cT(l) g1,   E = cTE(l) g1 + cE(l) g2,   B = cB(l) g3,
 *     Q = E cos 2phi - B sin 2phi,   U = E sin 2phi + B cos 2phi,   phi = atan2(ky, kx)
 * (y is the row axis of the output, x its column axis).  `table` is a HOST array [n_ell][4] float32, row = integer
 * l from 0, columns cT = sqrt C_TT, cTE = C_TE / sqrt C_TT, cE = sqrt max(C_EE - C_TE^2 / C_TT, 0), cB = sqrt C_BB,
 * each times 1 / sqrt(Lx Ly) so that <|a_T|^2> = C_TT / (Lx Ly) ...: the fields come out in the units of sqrt C_l
 * (K_CMB).  The four coefficients are interpolated linearly in l (float64 l and weight, float32 coefficients);
 * cells with l beyond the last row get zero, as does l = 0.
 * Nyquist lines: the cells with |fx| = nx/2 or |fy| = ny/2 are zero in all three fields.  sin 2phi is odd there,
 * so a Hermitian Q / U pair does not exist for them, and power left in them mixes E into B.
 * The self-mirrored column kx = 0 holds independent cells for every ky and is made Hermitian by pass 1 as the 3-D
 * generator's is, S' = (S[ky] + conj S[-ky]) / sqrt 2, alike in T, Q and U: there cos 2phi = -1 and sin 2phi = 0,
 * so Q' = -E', U' = -B' and the T-E covariance is kept.
 * Draws: cell pair (ky = iy, iy + ny/2), iy < ny/2, of column kx uses the three Philox counters
 * (kx, iy, stream, 0x434d4200 | d), d = 0, 1, 2, key = seed: words (0,1) are the Box-Muller pair of g_{d+1} / sqrt 2
 * for cell iy, words (2,3) that for cell iy + ny/2.  Counter word 3 is 0 for the 2-D screens, 0x33440000 for the
 * 3-D ones and an ASCII tag for each noise series: no counter coincides.
 * Then the two passes of mrx_screen_generate_batch per field (normalisation 1).  `fields[3]` gives the output block of
 * T, Q and U as mrx_screen_generate_3d's `planes` do (d_out, out_ny, out_nx, ld_out: the top-left block of the domain;
 * the other fields are ignored).  d_work: mrx_cmb_work_floats floats (the three half spectra, the normalisation, the
 * table's device copy), 16-byte aligned. */
int mrx_cmb_work_floats(int ny, int nx, int n_ell, size_t* floats);
int mrx_cmb_generate(mrx_ctx* ctx, uint64_t seed, uint32_t stream, int ny, int nx, double res, const float* table,
                     int n_ell, const mrx_screen_desc* fields, float* d_work, size_t work_floats);

/* Band powers of two maps from their half-plane modes: the binned sums behind TT, EE, BB, TE, TB, EB.
 * d_a1, d_a2: [3][ny][nx/2 + 1] complex128 (re, im interleaved), the modes of T, Q, U in numpy.fft.rfft2's layout
 * (rows fy as fftfreq orders them, columns fx = 0 .. nx/2); d_a2 == d_a1 gives the auto spectra.  ny and nx are even
 * and at least 8, not necessarily powers of two; `res` is the pixel size in radians.  Per cell, all in float64:
 *     k = 2 pi (fx / (nx res), fy / (ny res)),   l^2 = kx^2 + ky^2,
 *     cos 2phi = (kx^2 - ky^2) / l^2,   sin 2phi = 2 kx ky / l^2,
 *     E = Q cos 2phi + U sin 2phi,   B = -Q sin 2phi + U cos 2phi
 * -- the convention of mrx_cmb_generate above (x the column axis, y the row axis, phi = atan2(ky, kx)), inverted, and of
 * tests/cmb_ref.py's modes_of.  A cell is dropped when k = 0, when it lies on either Nyquist line (fx = nx/2 or
 * |fy| = ny/2: sin 2phi is odd there, see mrx_cmb_generate) or when l is outside [edges[0], edges[n_bins]).  A kept cell
 * lies in bin b when edges[b]^2 <= l^2 < edges[b+1]^2 and has the weight w = 2 for 0 < fx < nx/2 (its mirror carries the
 * same real parts) and w = 1 in the column fx = 0.  `edges` is a HOST array of n_bins + 1 finite, strictly ascending
 * values >= 0, n_bins in 1 .. 1024.  d_sums [n_bins][8] receives per bin
 *     sum w,  sum w l,  then sum w XY for XY = TT, EE, BB, TE, TB, EB,   XY = (Re(a1_X conj a2_Y) + Re(a1_Y conj a2_X)) / 2.
 * No floating-point atomics: the order of every sum is a function of (ny, nx, edges) alone, so two calls give the same
 * bits.  d_work: mrx_band_power_work_bytes bytes, 16-byte aligned like d_a1 and d_a2; its contents on entry do not
 * matter.  The call uploads the edges and waits for that copy. */
int mrx_band_power_work_bytes(int ny, int nx, int n_bins, size_t* bytes);
int mrx_map_band_powers(mrx_ctx* ctx, const double* d_a1, const double* d_a2, int ny, int nx, double res,
                        const double* edges, int n_bins, double* d_sums, void* d_work, size_t work_bytes);

/* Covariance-matched amplitudes (circulant embedding) for the generators above.  The power law is
 * the continuous transform of the Matern covariance cut at the grid's Nyquist wavenumber; for rough
 * fields (nu = 1/3 in three dimensions, atmosphere/atmosphere.py:249) most of the one-pixel structure
 * lies beyond it.  This table holds sqrt(max(lambda, 0)) with lambda the eigenvalues of the
 * covariance ITSELF on the periodic nh x ny x nx grid (nh = 0: two dimensions),
 *     lambda[k] = sum_d rho_per(d) cos(2 pi k.d / N),   rho_per(d) = sum over images n of rho(|d + n L| / r0)
 * (images summed, not the distance wrapped: the periodic covariance stays positive definite; images
 * beyond x_cut outer scales -- where rho < 1e-10 -- are skipped), so that the structure function of the
 * screens is Matern's from one pixel up.  The header of the table normalises the screens by
 * sum(lambda) / rho_per(0): their variance is rho_per(0) = 1 + the images' share (1.01 at L = 5 r0) and
 * their structure function 2 (rho_per(0) - rho_per(d)), in which the images cancel to second order.
 * rho is the exact Matern correlation (functions/__init__.py:30-39) read from the caller's HOST tables
 * log_cov[i] = log rho(x_i), log_sf[i] = log(1 - rho(x_i)) at log x_i = log_first + i log_step, x = r / r0
 * (8192 nodes from 1e-6 to 1e3: four-point Lagrange interpolation in log x is then good to 1e-11; finite
 * values only): rho(0) = 1 and, with x = max(|r| / r0, x_first), t = 1/(1 + x^2), rho = t (1 - exp(LSF(x))) +
 * (1 - t) exp(LCOV(x)), the blend of functions/__init__.py:70-73.  (The reference's
 * approximate_normalized_matern itself -- 1024 nodes, linear, good to 1e-5 -- is no longer positive
 * definite on a grid at that accuracy: its clipped eigenvalues come back as 50 % too much structure at
 * one pixel.)  float64 on the device, direct
 * cosine sums over the even half axes: a set-up step, once per geometry (8 x 2048^2 layers of two
 * outer scales: milliseconds; a 64 x 4096 x 512 volume: about a second).  d_table
 * (mrx_screen_amp_floats' table_floats; 16-byte aligned) is then passed as mrx_screen_desc.d_amp
 * (nh = 0) or mrx_screen_generate_3d's d_amp. */
int mrx_screen_amp_floats(int nh, int ny, int nx, int n_radial, size_t* table_floats, size_t* work_floats);
int mrx_screen_amplitudes(mrx_ctx* ctx, int nh, int ny, int nx, double dh, double dy, double dx, double r0,
                          const double* log_cov, const double* log_sf, int n_radial, double log_first,
                          double log_step, double x_cut, float* d_table, float* d_work, size_t work_floats);

/* One unsmoothed screen over the whole domain.  d_work: mrx_screen_work_floats(ny, nx, 1)
 * floats (a buffer of 2*ny*nx float2, the size earlier versions asked for, is ample). */
int mrx_screen_generate(mrx_ctx* ctx, uint64_t seed, uint32_t stream, int ny,
                        int nx, double dy, double dx, double r0, double nu,
                        float* d_out, float* d_work);

/* Sum over the FFT grid of the un-normalised PSD, reduced on the device
 * (float64); mrx_screen_generate uses it internally, exposed for tests. */
int mrx_screen_psd_sum(mrx_ctx* ctx, int ny, int nx, double dy, double dx,
                       double r0, double nu, double* host_sum);

/* ---- multi-GPU --------------------------------------------------------- */

/* Detectors shard across the GPUs of a node in equal blocks of contiguous rows (the last may
 * be short); the data path itself needs no collective.  The epilogue the reference's seam
 * implies -- one [ndet, nt] array per observation, sim/simulation.py:266-272 -- is ONE RCCL
 * all-gather over xGMI: the TOD is detector-major, so the gathered array is the concatenation
 * of the shards and nothing is packed or staged.
 *
 * mrx_comm_unique_id (rank 0; the caller hands the MRX_COMM_ID_BYTES bytes to every rank by
 * whatever channel it has: torch.distributed, MPI, a file) + mrx_comm_create = ncclGetUniqueId +
 * ncclCommInitRank on the context's device; mrx_comm_wrap adopts an ncclComm_t the caller
 * already owns.  RCCL is loaded at first use (dlopen), not at library load. */
#define MRX_COMM_ID_BYTES 128
int mrx_comm_unique_id(mrx_ctx* ctx, void* id_out);
int mrx_comm_create(mrx_ctx* ctx, const void* id, int world, int rank, mrx_comm** comm);
int mrx_comm_wrap(mrx_ctx* ctx, void* nccl_comm, int world, int rank, mrx_comm** comm);
int mrx_comm_destroy(mrx_ctx* ctx, mrx_comm* comm);
/* d_full[r * count + i] = rank r's d_shard[i], for every rank, enqueued on the context's
 * stream.  count = rows_per_rank * ld floats: every rank passes the same count (pad the last
 * shard's rows).  In place when d_shard == d_full + rank * count, i.e. when the writer put the
 * shard straight into its slot of the full TOD (mrx_spline_upsample's d_out / ld_out). */
int mrx_allgather_tod(mrx_ctx* ctx, mrx_comm* comm, const float* d_shard, float* d_full,
                      size_t count);

/* The same gather as world - 1 direct sends + world - 1 receives in one RCCL group instead of
 * one ncclAllGather: every pair of the node's GPUs has its own xGMI link, so each rank pushes
 * its shard to all peers at once (shard / link rate, against (world - 1) x that around a ring;
 * SURVEY section 5).  Same arguments and result as mrx_allgather_tod; which of the two is
 * faster on a given node is for the caller to measure (bench.py --gather-algo). */
int mrx_allgather_tod_p2p(mrx_ctx* ctx, mrx_comm* comm, const float* d_shard, float* d_full,
                          size_t count);

/* Layer-sharded screen generation (strong scaling: the screens are replicated work): rank
 * l % world generated layer l (mrx_screen_generate_batch with its own layers only); one
 * ncclBroadcast per layer from its owner, all in one group, fills the other ranks' buffers in
 * place.  Screens are functions of (seed, layer), so the result equals what every rank would
 * have generated itself (atmosphere/process.py:191-209 has no counterpart: the reference is
 * one process).  d_screens [n_layers] device pointers (host array), counts [n_layers] floats. */
int mrx_exchange_screens(mrx_ctx* ctx, mrx_comm* comm, float* const* d_screens, const size_t* counts,
                         int n_layers);

/* ---- map sampling --------------------------------------------- */

/* A celestial map as MapMixin._sample_maps sees it after smoothing, conversion to K_RJ and
 * the parity flip (sim/map.py:72-73,104-109): */
typedef struct mrx_sky_map {
  const float* d_values;  /* [n_channels][n_stokes][n_eta][n_xi] float32, K_RJ */
  int n_channels, n_stokes, n_eta, n_xi;
  double eta0, deta;      /* eta[i] = eta0 + i * deta, rad (np.linspace, projection.py:122-123;
                             deta < 0 after the parity flip) */
  double xi0, dxi;        /* xi[j] = xi0 + j * dxi */
  double center_phi, center_theta; /* map centre in the map's frame, rad */
  int bilinear;           /* 1: bilinear sampling, 0: nearest pixel (map_kwargs) */
  int reserved;
} mrx_sky_map;

/* K_RJ -> pW of each channel (sim/map.py:117-135, band/band.py:235-255): with an atmosphere
 * the channel's transmission integral, collapsed by the host at the scalar base temperature
 * onto (zenith pwv, elevation), is looked up per sample at the detector's elevation and its
 * zenith-scaled pwv -- the coarse series of mrx_atm_sample, interpolated linearly
 * (sim/atmosphere.py:30-37); without one, a scalar per channel. */
typedef struct mrx_map_cal {
  const float* d_table;    /* [n_channels][n_pwv][n_el] float32, or NULL */
  const float* d_axis_pwv; /* [n_pwv] */
  const float* d_axis_el;  /* [n_el] */
  int n_pwv, n_el;
  const double* d_pwv;     /* [Ta][D] coarse zenith-scaled pwv, time-major */
  int Ta;
  int steps_per_tile;      /* the most coarse steps of the pwv series that 1024 consecutive samples meet (ceil(1025 dt / dta) + 1), or 0 if the
                            * caller does not know: sizes the LDS table of the calibration's interval form (a tile that meets more
                            * takes the per-sample form: correct, slower) */
  double ta0, dta;         /* first coarse time and coarse step (s) */
  const double* d_t;       /* [T] full-rate sample times */
  const double* d_scalar;  /* [n_channels] Int passband dnu (device), used when d_table is NULL */
} mrx_map_cal;

/* obs.loading["map"] for the D detectors of one band (sim/map.py:76-172): detector pointing
 * from the boresight and offsets (float32 chain of coords/transforms.py:10-29), rotation
 * into the map's frame by the per-sample 3x3 (coords/coordinates.py:184-236; NULL for a map
 * in the az/el frame), offsets from the map centre (transforms.py:36-53), the pointing-matrix
 * row of utils/linalg.py:9-58 with the Stokes weights of map/projection.py:134-179, K_RJ -> pW
 * per channel, float32 accumulation over channels, and the [0.25, 0.5, 0.25] convolution
 * along time (scipy reflect mode, map.py:170), in one pass.
 *  d_az, d_el   [T] float32 full-rate boresight
 *  d_transform  [T][3][3] float64 transform stack (row vector times matrix), or NULL
 *  d_dx, d_dy   [D] float32 offsets of observation.coords (rolled), radians
 *  d_stokes_w   [D][n_stokes] float64: Mueller[d, 0, stokes] (array/array.py:204-221)
 *  d_out        [D][ld_out] float32, pW
 * The map (all channels and Stokes planes) must be smaller than 2 GiB: the sampler reads it through a copy with its
 * row pairs interleaved -- a cell's four corners in 16 contiguous bytes, one gather a sample and plane -- which every call
 * builds into memory the context owns (twice the map's bytes, kept between calls; calls on one context are ordered).
 * With MRX_OPT_POINTING_CHAIN the planes are read as they are (below 4 GiB). */
int mrx_map_sample(mrx_ctx* ctx, const mrx_sky_map* map, const mrx_map_cal* cal,
                   const float* d_az, const float* d_el, int T, const double* d_transform,
                   const float* d_dx, const float* d_dy, const double* d_stokes_w, int D,
                   float* d_out, size_t ld_out);

/* mrx_map_sample with the gain and TOD.to("K_RJ") (tod/tod.py:106-142) on its store:
 *   d_out[d][s] = S(d, s) * d_scale[d] / den_band(d)(el(d, s)),
 * S the pW field mrx_map_sample writes, the division exactly as mrx_tod_to_krj performs it on a finished field (the same
 * per-tile elevation model from the same 1024 samples, the same lookup) -- the same bits as mrx_map_sample followed by
 * mrx_tod_to_krj with that d_scale, without the second pass over the field.
 *  d_scale                      [D] float32 or NULL (1): the gain error (sim/simulation.py:239-247)
 *  d_bore_el                    [T] float32 full-rate boresight elevation
 *  d_krj_dx, d_krj_dy, d_band   [D] float32 offsets and int32 band index of this call's rows, as mrx_tod_to_krj takes them
 *  d_cal_axis_el, d_cal_values  [n_el], [n_bands][n_el] float32: the bands' collapsed transmission integrals
 * MRX_ERR_UNSUPPORTED (nothing launched) with MRX_OPT_POINTING_CHAIN: sample in pW and convert there. */
int mrx_map_sample_krj(mrx_ctx* ctx, const mrx_sky_map* map, const mrx_map_cal* cal,
                       const float* d_az, const float* d_el, int T, const double* d_transform,
                       const float* d_dx, const float* d_dy, const double* d_stokes_w, int D,
                       const float* d_scale, const float* d_bore_el, const float* d_krj_dx, const float* d_krj_dy,
                       const int32_t* d_band, const float* d_cal_axis_el, const float* d_cal_values, int n_el, int n_bands,
                       float* d_out, size_t ld_out);

/* BinMapper.run for one TOD (mappers/bin_mapper.py:84-120): the transpose of the pointing
 * matrix of mrx_map_sample, map_sum += (W * D) @ P and map_wgt += W @ |P|, as float64 atomic
 * adds into the caller's (zeroed or running) maps; the map itself is sum / wgt.  `map` gives
 * the grid (d_values is not read; bilinear = 0 is the mapper's default).
 *  d_tod     [D][ld_tod] float32 signal (the sum of the TOD's fields)
 *  d_weight  [D][ld_weight] float32 sample weights, or NULL for ones (tod.weight's default)
 *  d_channel [D] map channel of each detector (the nu plane whose frequency is the
 *            detector's band centre, map/projection.py:152-155), or NULL for 0
 *  d_sum, d_wgt  [n_stokes][n_channels][n_eta][n_xi] float64
 * Pointing arguments as mrx_map_sample.  Summation order is not fixed (atomics): results
 * agree with a serial sum to float64 rounding. */
int mrx_bin_map(mrx_ctx* ctx, const mrx_sky_map* map, const float* d_tod, size_t ld_tod,
                const float* d_weight, size_t ld_weight, const float* d_az, const float* d_el, int T,
                const double* d_transform, const float* d_dx, const float* d_dy,
                const double* d_stokes_w, const int32_t* d_channel, int D, double* d_sum,
                double* d_wgt);

/* The same without global atomics on scattered pixels -- they execute at the memory side at a
 * tenth of the contiguous rate, and the focal plane is sparser than the map, so nothing merges on
 * the way.  The samples are routed to the map instead: every sample's pixel(s) are computed
 * once, a tile's contributions (nearest pixel: 16 detectors x 1024 samples, one each; bilinear:
 * 8 x 256, up to four each) are sorted by map region (64 x 32 pixels of one plane) into the
 * tile's slot of the work buffer, and each region's segments are then summed in LDS (float64)
 * and added to the map as whole rows.  Same arguments and same result to float64 rounding (the
 * order of the sums differs).  MRX_ERR_UNSUPPORTED for maps of more than 2048 regions
 * (n_channels * ceil(n_eta / 32) * ceil(n_xi / 64)): call mrx_bin_map.
 *  d_work   16-byte aligned; mrx_bin_map_work_bytes gives the least size (one column of tiles:
 *           all detectors x one tile of samples) and the size that takes all T samples in one
 *           go (16 bytes per contribution: 16 per sample nearest, 64 bilinear, + 4 bytes per
 *           (region, tile)); with less the call walks the time axis in chunks. */
int mrx_bin_map_work_bytes(const mrx_sky_map* map, int D, int T, size_t* min_bytes, size_t* full_bytes);
int mrx_bin_map_bucketed(mrx_ctx* ctx, const mrx_sky_map* map, const float* d_tod, size_t ld_tod,
                         const float* d_weight, size_t ld_weight, const float* d_az, const float* d_el, int T,
                         const double* d_transform, const float* d_dx, const float* d_dy,
                         const double* d_stokes_w, const int32_t* d_channel, int D, double* d_sum,
                         double* d_wgt, void* d_work, size_t work_bytes);

/* ---- maximum-likelihood map-making (white-noise GLS, MaximumLikelihoodMapper) ---------- */

/* The operators of  (P^T W P) m = P^T W d.  P is the Stokes-weighted pointing matrix that mrx_bin_map transposes, signed
 * (no |.|): row (d, s) holds w_k(d) b_c at pixel c of plane (k, channel(d)), with the binning's pixels and float32 corner
 * weights b_c (bit for bit: the same device code).  W is diagonal: d_weight[d][s] (or 1) times d_det_weight[d] (or 1).
 * Maps are [n_stokes][n_channels][n_eta][n_xi] float64, the layout of mrx_bin_map's d_sum; `map` gives the grid
 * (d_values is not read).  Pointing arguments as mrx_bin_map; MRX_OPT_POINTING_CHAIN selects the float32 chain.
 *
 * The forward operator, the exact transpose of mrx_bin_map's d_sum (no calibration, no time kernel: not mrx_map_sample):
 *   d_out[d][s] = beta d_out[d][s] + alpha sum_k w_k(d) sum_c b_c d_x[k][channel(d)][pix_c(d, s)]
 * accumulated in float64 and rounded once to float32.  beta = 0: d_out is not read.
 *  d_x    [n_stokes][n_channels][n_eta][n_xi] float64
 *  d_out  [D][ld_out] float32 */
int mrx_map_project(mrx_ctx* ctx, const mrx_sky_map* map, const double* d_x, const float* d_az, const float* d_el, int T,
                    const double* d_transform, const float* d_dx, const float* d_dy, const double* d_stokes_w,
                    const int32_t* d_channel, int D, double alpha, double beta, float* d_out, size_t ld_out);

/* The normal operator:  d_y += P^T W P d_x,  with no TOD-sized intermediate: (P x)_s is gathered per sample in float64
 * and W (P x)_s b_c is routed to map regions and summed as mrx_bin_map_bucketed routes W D b_c.  Maps of more than 2048
 * regions, or d_work = NULL, take float64 atomics with run merging instead.  The result equals P^T W P x to float64
 * rounding (the order of the sums differs between the forms).
 *  d_weight      [D][ld_weight] float32 per-sample weights, or NULL (ones)
 *  d_det_weight  [D] float64 per-detector weights, or NULL (ones)
 *  d_work        16-byte aligned, at least mrx_map_normal_work_bytes' minimum (one column of tiles); with less than its
 *                full size the call walks the time axis in chunks.  The query gives 0 and 0 for maps the routed form does
 *                not take. */
int mrx_map_normal_work_bytes(const mrx_sky_map* map, int D, int T, size_t* min_bytes, size_t* full_bytes);
int mrx_map_normal_apply(mrx_ctx* ctx, const mrx_sky_map* map, const double* d_x, const float* d_weight, size_t ld_weight,
                         const double* d_det_weight, const float* d_az, const float* d_el, int T, const double* d_transform,
                         const float* d_dx, const float* d_dy, const double* d_stokes_w, const int32_t* d_channel, int D,
                         double* d_y, void* d_work, size_t work_bytes);

/* The block diagonal of P^T W P: per pixel and channel the n_stokes x n_stokes block
 *   d_blocks[idx(k, l)][c][p] += sum over samples at p of W b_c^2 w_k w_l,   k <= l, idx row-major over the upper triangle
 * (n_stokes (n_stokes + 1) / 2 planes per channel: I,I  I,Q  I,U  Q,Q  Q,U  U,U for IQU), float64 atomics with run
 * merging into the caller's (zeroed or running) planes.  Weights as mrx_map_normal_apply. */
int mrx_bin_map_blocks(mrx_ctx* ctx, const mrx_sky_map* map, const float* d_weight, size_t ld_weight,
                       const double* d_det_weight, const float* d_az, const float* d_el, int T, const double* d_transform,
                       const float* d_dx, const float* d_dy, const double* d_stokes_w, const int32_t* d_channel, int D,
                       double* d_blocks);

/* Per pixel and channel, z = H^-1 r in float64 (n_stokes <= 3, by H = L D L^T), H from mrx_bin_map_blocks' layout.
 * A block with a pivot <= 0 (H[0][0] among them), or a reciprocal condition number 1 / (|H|_1 |H^-1|_1) below `rcond`
 * is not solved: z = NaN there when nan_invalid, else 0 (the preconditioner's form).  d_z may be d_rhs.
 *  d_blocks  [n_stokes (n_stokes + 1) / 2][n_channels][n_pix],  d_rhs, d_z  [n_stokes][n_channels][n_pix] float64
 *  d_mask    [n_channels][n_pix] uint8: 1 where solved, or NULL */
int mrx_map_block_solve(mrx_ctx* ctx, int n_stokes, int n_channels, long long n_pix, const double* d_blocks,
                        const double* d_rhs, double rcond, int nan_invalid, double* d_z, uint8_t* d_mask);

/* ---- destriping (DestripingMapper) ---------------------------------------- */

/* The operators of the destriper's baseline system.  Per TOD  d = P m + F a + n:  F expands the per-detector baseline
 * amplitudes a[d][b] to samples, baseline b covering samples [b L, min((b + 1) L, T)) (the last one may be shorter), so a
 * detector has nb = ceil(T / L) baselines; P, W, the grid and the pointing arguments are mrx_map_normal_apply's.  Both take
 * nearest-pixel pointing only (MRX_ERR_UNSUPPORTED for a bilinear map) and L >= 16 samples (MRX_ERR_INVALID below; L > T
 * gives one baseline a detector); MRX_OPT_POINTING_CHAIN selects the float32 chain.
 *
 * The baseline reduction, F^T W mu (tod - alpha P x) in one pass:
 *   d_y[d][b]    += sum_{s in b} W_s mu_s (d_tod[d][s] - alpha (P x)_s)
 *   d_hits[d][b] += sum_{s in b} W_s mu_s
 * mu_s = d_mask[channel(d)][pixel(d, s)] (the block solve's mask: 1 where solved), or 1 with d_mask = NULL.  d_tod = NULL
 * reads no TOD (0), d_x = NULL projects no map; d_y or d_hits may be NULL (not both).  Summed per (detector, baseline) in
 * float64, one atomic per baseline and tile of 1024 samples.
 *  d_tod   [D][ld_tod] float32,  d_x  [n_stokes][n_channels][n_eta][n_xi] float64
 *  d_y, d_hits  [D][nb] float64 (added to) */
int mrx_baseline_reduce(mrx_ctx* ctx, const mrx_sky_map* map, const float* d_tod, size_t ld_tod, const double* d_x,
                        double alpha, const float* d_weight, size_t ld_weight, const double* d_det_weight,
                        const uint8_t* d_mask, int L, const float* d_az, const float* d_el, int T, const double* d_transform,
                        const float* d_dx, const float* d_dy, const double* d_stokes_w, const int32_t* d_channel, int D,
                        double* d_y, double* d_hits);

/* The baselines binned:  d_y += P^T W F a,  with no TOD-sized intermediate: W a[d][s / L] is routed to map regions and
 * summed as mrx_map_normal_apply routes W (P x)_s.  Maps of more than 2048 regions, or d_work = NULL, take float64 atomics
 * with run merging instead.  mrx_map_normal_work_bytes sizes d_work (the same 16-byte entries and chunks).
 *  d_amp  [D][nb] float64,  d_y  [n_stokes][n_channels][n_eta][n_xi] float64 (added to) */
int mrx_bin_map_baselines(mrx_ctx* ctx, const mrx_sky_map* map, const double* d_amp, int L, const float* d_weight,
                          size_t ld_weight, const double* d_det_weight, const float* d_az, const float* d_el, int T,
                          const double* d_transform, const float* d_dx, const float* d_dy, const double* d_stokes_w,
                          const int32_t* d_channel, int D, double* d_y, void* d_work, size_t work_bytes);

/* ---- the destriper's prior on the offsets (DestripingMapper(baseline_prior=...)) ---------------- */

/* Madam's C_a^-1 for D detectors of nb baselines each: s_d T, T the weighted graph Laplacian over one detector's
 * baselines (maria_amd/destripe_prior.py),
 *   (T a)_b = sum_{k=1..K} w_k ( [b + k < nb] (a_b - a_{b+k}) + [b - k >= 0] (a_b - a_{b-k}) ),
 * T 1 = 0 exactly.  Float64 throughout, independent of the map.  All three refuse (MRX_ERR_INVALID) K outside 1 .. 64,
 * Kp outside 0 .. 16, nb < 1 and a negative (or NaN) scale; a check of the scales copies them to the host.
 *  d_w  [K] float64 (signed),  d_scale  [D] float64 >= 0,  d_hits, d_a, d_y, d_r, d_z  [D][nb] float64 */

/* d_y = d_hits * d_a + s_d T d_a (overwritten; d_hits = NULL: no diagonal term).  One workgroup per detector and tile of
 * 256 baselines, the tile with its K-baseline halo in LDS.  d_y must not be d_a. */
int mrx_baseline_prior_apply(mrx_ctx* ctx, int D, int nb, int K, const double* d_w, const double* d_scale,
                             const double* d_hits, const double* d_a, double* d_y);

/* The banded LDL^T of diag(hits) + s_d T_Kp per detector, T_Kp the Laplacian of the first Kp weights (its own diagonal).
 * d_ok[d] = 1 where every pivot is > 0 and the detector has a hit, else 0 (its factor is then not written).  One lane
 * per detector, sequential along b, 64 detectors a workgroup with the (Kp + 1)^2 window in LDS.  Layout, by column and
 * coalesced for the solve:  d_factor[(b (Kp + 1) + j) D + d] = 1 / D_b (j = 0), L[b + j][b] (j >= 1; 0 past nb)
 *  d_factor  [nb][Kp + 1][D] float64 (D nb (Kp + 1) 8 bytes),  d_ok  [D] uint8;  d_w, d_scale unused when Kp = 0 */
int mrx_baseline_band_factor(mrx_ctx* ctx, int D, int nb, int Kp, const double* d_w, const double* d_scale,
                             const double* d_hits, double* d_factor, uint8_t* d_ok);

/* d_z = (diag(hits) + s_d T_Kp)^-1 d_r from mrx_baseline_band_factor's factor; d_z = 0 for the detectors with ok = 0.
 * One lane per detector (forward and back substitution along b, the band in registers), 64 a workgroup.  d_z may be
 * d_r. */
int mrx_baseline_band_solve(mrx_ctx* ctx, int D, int nb, int Kp, const double* d_factor, const uint8_t* d_ok,
                            const double* d_r, double* d_z);

/* ---- detector noise spectra (maria_amd/noise_estimate.py) ------------------------------------------ */

/* scipy.signal.welch(x, fs, nperseg=nperseg) of every row with scipy's defaults: periodic Hann window, noverlap =
 * nperseg / 2, each segment's mean (summed in float64) removed before the window, one-sided density, mean over the
 * (T - nperseg) / (nperseg / 2) + 1 segments (trailing samples dropped, never read).  nperseg a power of two in
 * 256 .. 8192 (MRX_ERR_UNSUPPORTED otherwise); T < nperseg, ld < T, D < 1, fs <= 0 and null pointers are refused
 * (MRX_ERR_INVALID) with d_psd untouched.  One workgroup per row reads the row once; a NaN spoils its own row only.
 *  d_x    [D][ld] float32
 *  d_psd  [D][nperseg / 2 + 1] float32, signal units^2 / Hz */
int mrx_tod_welch(mrx_ctx* ctx, const float* d_x, size_t ld, int D, int T, int nperseg, double fs, float* d_psd);

/* ---- the inverse-noise filter of the correlated-noise GLS map (maria_amd/noise_filter.py) ------------ */

/* y[d] = s ⊙ (k_d ⊛ (s ⊙ x[d])): the linear (non-circular) convolution of each row with a symmetric per-detector kernel of
 * lags k_d[0..K] (k_d[-t] = k_d[t]), samples outside [0, T) zero (a finite Toeplitz section).  Overlap-save in float32
 * transforms of 4096 (K <= 512) or 8192 points; one workgroup per row reads each sample once, so d_y == d_x (with
 * ld_y == ld_x) filters in place.  A NaN spoils its own row only.
 *  d_x, d_y   [D][ld] float32
 *  d_lags     [D][K + 1] float64
 *  d_sqrt_w   [D][ld_w] float32 per-sample factor s (ld_w = 0: one row shared by every detector), or NULL (ones)
 * 0 <= K <= 2048; anything else, null pointers, D < 1, T < 1, ld < T, or d_y == d_x with ld_y != ld_x -> MRX_ERR_INVALID
 * with d_y untouched */
int mrx_tod_noise_filter(mrx_ctx* ctx, const float* d_x, size_t ld_x, float* d_y, size_t ld_y, int D, int T,
                         const double* d_lags, int K, const float* d_sqrt_w, size_t ld_w);

/* ---- noise shared across detectors in the GLS map: m common modes (maria_amd/noise_modes.py) --------- */

/* y[d] = s ⊙ (k_d ⊛ (s ⊙ (x[d] - sum_j U[d, j] b[j]))): mrx_tod_noise_filter of the rows less their rank-m part.  Two
 * passes: y = x - U b (float32, streaming: x read once, y written once), then the filter of y in place; d_y == d_x (with
 * ld_y == ld_x) works in place.  m = 0 is mrx_tod_noise_filter, bit for bit (U and b are not read).
 *  d_U  [D][m] float64 coupling of detector d to mode j
 *  d_b  [m][T] float32 mode series
 * mrx_tod_noise_filter's refusals, m outside 0 .. 16, or (m > 0) a null U or b -> MRX_ERR_INVALID with d_y untouched */
int mrx_tod_noise_filter_modes(mrx_ctx* ctx, const float* d_x, size_t ld_x, float* d_y, size_t ld_y, int D, int T,
                               const double* d_lags, int K, const float* d_sqrt_w, size_t ld_w, const double* d_U, int m,
                               const float* d_b);

/* a[j, t] = sum_d U[d, j] x[d, t], summed in float64: the projection of a [D][ld_x] float32 TOD onto m <= 16 detector
 * patterns, reading every sample once.  Deterministic (no atomics: the partial sums of a sample meet in one workgroup).
 *  d_U  [D][m] float64
 *  d_a  [m][T] float64
 * null pointers, D < 1, T < 1, m outside 1 .. 16 or ld_x < T -> MRX_ERR_INVALID with d_a untouched */
int mrx_tod_mode_project(mrx_ctx* ctx, const float* d_x, size_t ld_x, int D, int T, const double* d_U, int m, double* d_a);

/* ---- anti-aliased downsampling of a TOD (maria_amd/downsample.py) ------------------------------------ */

/* y[d][j] = ( sum_i h[H + i] x[d][j q + i] ) / ( sum_i h[H + i] ),   both sums over -H <= i <= H with 0 <= j q + i < T,
 * H = (n_taps - 1) / 2,  j = 0 .. T_out - 1,  T_out = (T + q - 1) / q.
 * Products and sums in float64 (x float32, taps float64), the quotient in float64, rounded ONCE to float32.
 * Output sample j belongs to input time t[j q] (zero phase for symmetric taps); T_out = len(range(0, T, q)).
 * Orientation: a CORRELATION, h's index grows along the sample index (d_taps[0] meets x[j q - H], d_taps[n_taps - 1]
 * meets x[j q + H]).  For symmetric taps this is scipy.signal.resample_poly(x, 1, q, window=h) divided by the same call
 * on a row of ones; for general taps pass window=h[::-1].
 * Edges: taps that fall outside [0, T) are dropped and the rest renormalised (the denominator above), so a constant row
 * maps onto itself; where the denominator is 0 the result is whatever the division gives.
 *  d_x     [D][ld_x] float32, read only
 *  d_taps  [n_taps] float64
 *  d_y     [D][ld_y] float32; nothing is written past T_out in a row
 * No alignment beyond 4 bytes is asked of the pointers or pitches.  q outside 2 .. 32, n_taps even or outside 1 .. 1025,
 * D < 1, T < 1, ld_x < T, ld_y < T_out, d_y == d_x or a null pointer -> MRX_ERR_INVALID with d_y untouched */
int mrx_tod_decimate(mrx_ctx* ctx, const float* d_x, size_t ld_x, int D, int T, int q,
                     const double* d_taps, int n_taps, float* d_y, size_t ld_y);

/* ---- glitch flags and gap filling of a TOD (maria_amd/flagging.py) ----------------------------------- */

/* r[d][t] = x[d][t] - med[d][t], one float32 subtraction, where med[d][t] is the median of the 2 h + 1 values
 * x[d][clamp(t + i, 0, T - 1)], -h <= i <= h, h = half_window: scipy.ndimage.median_filter(x, size=(1, 2 h + 1),
 * mode="nearest").  The median is a selection, so r is reproducible bit for bit.  Inputs must be finite: the result on
 * NaN or inf is unspecified.
 *  d_x  [D][ld_x] float32, read only
 *  d_r  [D][ld_r] float32; nothing is written past T in a row
 * No alignment beyond 4 bytes is asked of the pointers or pitches.  half_window outside 1 .. 15, D < 1, T < 1, a pitch < T,
 * d_r == d_x or a null pointer -> MRX_ERR_INVALID with d_r untouched */
int mrx_tod_median_residual(mrx_ctx* ctx, const float* d_x, size_t ld_x, int D, int T, int half_window,
                            float* d_r, size_t ld_r);

/* Glitch flags of a TOD from the residual above.  Sample s of row d is a DETECTION if |r[d][s]| > d_thresh[d] (strict;
 * a NaN threshold detects nothing, a negative one every sample).  flags[d][t] = 1 where t is a detection, else 2 where
 * some detection s has t - grow_after <= s <= t + grow_before (a detection flags grow_before samples before itself and
 * grow_after samples after itself, clipped to the row), else 0.  Every byte of [0, T) of every row is written.
 *  d_thresh  [D] float32
 *  d_flags   [D][ld_f] uint8; no alignment is asked (4-byte stores where pointer and pitch allow them, bytes otherwise)
 *  d_count   [D] uint32 number of nonzero flags of each row, OVERWRITTEN (one integer atomic a tile), or NULL
 * mrx_tod_median_residual's refusals on x, ld_f < T, a grow_* outside 0 .. 64 or a null d_thresh or d_flags ->
 * MRX_ERR_INVALID with d_flags and d_count untouched */
int mrx_tod_glitch_flag(mrx_ctx* ctx, const float* d_x, size_t ld_x, int D, int T, int half_window,
                        const float* d_thresh, int grow_before, int grow_after,
                        uint8_t* d_flags, size_t ld_f, uint32_t* d_count);

/* Fill the flagged samples of a TOD in place.  For every maximal run [a, b) of nonzero flags of a row: L = the unflagged
 * indices of [max(0, a - n_fit), a), R = those of [b, min(T, b + n_fit)); (tL, yL), (tR, yR) the float64 means of the
 * indices and samples of L and R;  x[d][t] = yL + (yR - yL) (t - tL) / (tR - tL) for a <= t < b, in float64, rounded ONCE
 * to float32.  A run that starts at 0 gets yR, one that ends at T gets yL, a row flagged from end to end is left as it
 * is.  Only flagged samples are written and only unflagged ones are read.  No noise realisation is added.
 * One thread fills a run: meant for sparse flags; correct, and bounded by T, for any run length.
 *  d_x       [D][ld_x] float32, in place
 *  d_flags   [D][ld_f] uint8, read only
 *  d_filled  [D] uint32 number of samples written in each row, OVERWRITTEN, or NULL
 * n_fit outside 1 .. 16, D < 1, T < 1, a pitch < T or a null d_x or d_flags -> MRX_ERR_INVALID with d_x and d_filled
 * untouched */
int mrx_tod_gap_fill(mrx_ctx* ctx, float* d_x, size_t ld_x, int D, int T, const uint8_t* d_flags, size_t ld_f,
                     int n_fit, uint32_t* d_filled);

/* ---- jumps of a TOD: step statistic, peaks, heights, repair (maria_amd/jumps.py) ----------------------- */

/* Common to the four entries below.  Rows are [D][ld] with unit stride along time; no alignment beyond the element size
 * is asked of a pointer or pitch (16-byte accesses of float32 rows and 4-byte accesses of flags where pointer and pitch
 * allow them, narrow ones otherwise), and nothing is written past T in a row.  d_flags [D][ld_f] uint8 or NULL: sample u
 * of a row is VALID if 0 <= u < T and its flag is 0 (every sample of the row when d_flags is NULL).  Inputs must be
 * finite: the result on NaN or inf is unspecified.  w = window, g = gap, m = min_count. */

/* The step statistic: the mean after a sample less the mean before it.  For row d and t = 0 .. T - 1:
 *   L(t) = the valid u of [t - g - w, t - g),   R(t) = the valid u of [t + g, t + g + w)
 *   s[d][t] = |L| >= m and |R| >= m ? (float)(sum over R of x / |R| - sum over L of x / |L|) : 0.0f
 * Sums, quotients and the difference are float64, the result is rounded ONCE.  The sums are differences of float64
 * prefix sums over a tile of 1024 samples and its halo, formed in an order that is a function of T, w and g alone: the
 * same inputs give the same bits on every call.
 *  d_x  [D][ld_x] float32, read only
 *  d_s  [D][ld_s] float32, OVERWRITTEN in [0, T) of each row
 * window outside 2 .. 256, gap outside 0 .. 64, min_count outside 1 .. window, D < 1, T < 1, a pitch (of an array that
 * is given) < T, d_s == d_x or a null d_x or d_s -> MRX_ERR_INVALID with d_s untouched */
int mrx_tod_step_stat(mrx_ctx* ctx, const float* d_x, size_t ld_x, const uint8_t* d_flags, size_t ld_f, int D, int T,
                      int window, int gap, int min_count, float* d_s, size_t ld_s);

/* The peaks of |s|.  Sample t of row d is a PEAK if
 *   |s[d][t]| > d_thresh[d]                                   (strict; a NaN threshold finds nothing)
 *   |s[d][u]| <  |s[d][t]| for every u of [t - sep, t) inside the row
 *   |s[d][u]| <= |s[d][t]| for every u of (t, t + sep] inside the row
 * so the earliest sample of a plateau wins and two peaks are always more than sep apart.  flags[d][t] = 1 at a peak,
 * else 2 where some peak p has t - grow_after <= p <= t + grow_before, else 0.  Every byte of [0, T) of every row is
 * written.  Comparisons only: reproducible bit for bit.
 *  d_s       [D][ld_s] float32, read only
 *  d_thresh  [D] float32
 *  d_flags   [D][ld_f] uint8
 *  d_count   [D] uint32 number of PEAKS of each row, OVERWRITTEN (one integer atomic a tile), or NULL
 * sep outside 1 .. 512, a grow_* outside 0 .. 64, D < 1, T < 1, a pitch < T or a null d_s, d_thresh or d_flags ->
 * MRX_ERR_INVALID with d_flags and d_count untouched */
int mrx_tod_jump_find(mrx_ctx* ctx, const float* d_s, size_t ld_s, int D, int T, const float* d_thresh, int sep,
                      int grow_before, int grow_after, uint8_t* d_flags, size_t ld_f, uint32_t* d_count);

/* The height of each listed jump.  The jumps are listed row after row: row d owns d_pos[d_row_start[d] ..
 * d_row_start[d + 1]), ascending.  For jump j of row d at p = pos[j], with the row's neighbouring jumps p- = pos[j - 1]
 * and p+ = pos[j + 1] where they exist:
 *   lo = max(0, p - g - w, p- + g),   hi = min(T, p + g + w, p+ - g)
 *   L = the valid u of [lo, p - g),   R = the valid u of [p + g, hi)
 *   ok[j]     = |L| >= m and |R| >= m
 *   height[j] = ok ? sum over R of x / |R| - sum over L of x / |L| : 0.0         (float64 throughout)
 * The windows are clipped so that one jump's estimate never averages across another.  REPRODUCIBLE: the order of the
 * additions is a function of the list and T alone (no atomics).
 *  d_x          [D][ld_x] float32, read only
 *  d_row_start  [D + 1] int32, non-decreasing from 0 to n
 *  d_pos        [n] int32
 *  d_height     [n] float64, d_ok [n] uint8: entry j OVERWRITTEN for every j some row owns
 * An entry of d_pos is clamped into [0, T - 1] and a bound read from d_row_start into [0, n]: bad lists give wrong
 * heights, never an access outside the arrays.  n = 0 is a valid call that does nothing (d_pos, d_height and d_ok may
 * then be NULL).  mrx_tod_step_stat's refusals on window, gap, min_count, D, T and the pitches, n < 0, a null d_x or
 * d_row_start, or with n > 0 a null d_pos, d_height or d_ok -> MRX_ERR_INVALID with the outputs untouched */
int mrx_tod_jump_height(mrx_ctx* ctx, const float* d_x, size_t ld_x, const uint8_t* d_flags, size_t ld_f, int D, int T,
                        const int32_t* d_row_start, const int32_t* d_pos, int n, int window, int gap, int min_count,
                        double* d_height, uint8_t* d_ok);

/* Take the listed jumps out.  With k(t) = the number of jumps of row d with pos <= t (lists as above):
 *   y[d][t] = k(t) == 0 ? x[d][t] : (float)((double)x[d][t] - cum[row_start[d] + k(t) - 1])
 * where d_cum [n] float64 is the caller's inclusive cumulative sum of the heights within each row.  One float64
 * subtraction rounded once: reproducible bit for bit.
 *  d_y  [D][ld_y] float32; d_y == d_x (with ld_y == ld_x) works in place
 * The bounds read from d_row_start are clamped into [0, n]; n = 0 copies x (d_pos and d_cum may then be NULL).
 * D < 1, T < 1, n < 0, ld_x < T, ld_y < T, a null d_x, d_y or d_row_start, with n > 0 a null d_pos or d_cum, or
 * d_y == d_x with ld_y != ld_x -> MRX_ERR_INVALID with d_y untouched */
int mrx_tod_jump_fix(mrx_ctx* ctx, const float* d_x, size_t ld_x, int D, int T, const int32_t* d_row_start,
                     const int32_t* d_pos, const double* d_cum, int n, float* d_y, size_t ld_y);

/* ---- templates synchronous with a per-sample key: ground pickup in azimuth bins (maria_amd/ground.py) - */

/* For row d and bin k, with kept(d, k) = the indices t of bin k with 0 <= t < T and flags[d][t] == 0 (all of them when
 * d_flags is NULL):
 *   hits[d][k]     = |kept(d, k)|
 *   sum[d][k]      = sum over kept(d, k) of ((double)x[d][t] - (double)model[d][t])      (no model term when d_model is NULL)
 *   template[d][k] = hits >= max(min_hits, 1) ? (float)(sum / (double)hits) : 0.0f       (float64 quotient, rounded ONCE)
 * The bins are lists shared by every row: bin k owns the sample indices d_order[d_start[k] .. d_start[k + 1]); a sample
 * in no bin is absent from d_order.  The sums are float64 and REPRODUCIBLE: the order of the additions is a function of
 * the bin's list alone (no atomics), so the same inputs give the same bits on every call, and a row's result does not
 * depend on which other rows share the call.
 *  d_x         [D][ld_x] float32, read only
 *  d_model     [D][ld_m] float32, read only, or NULL
 *  d_flags     [D][ld_f] uint8, read only, or NULL; a nonzero flag keeps the sample out
 *  d_order     [n_order] int32 sample indices, bin after bin
 *  d_start     [K + 1] int32, non-decreasing from 0 to n_order
 *  d_sum       [D][K] float64, OVERWRITTEN, or NULL
 *  d_hits      [D][K] uint32, OVERWRITTEN, or NULL
 *  d_template  [D][K] float32, OVERWRITTEN, or NULL
 * An entry of d_order outside [0, T) is skipped (an unsigned comparison; nothing is read through it), and the bounds
 * read from d_start are clamped into [0, n_order]: bad lists give wrong sums, never an access outside the arrays.  No
 * alignment beyond the element size is asked of the pointers or pitches.  D < 1, T < 1, K outside 1 .. 4096, n_order
 * outside 0 .. T, min_hits < 0, a pitch (of an array that is given) < T, a null d_x, d_order or d_start, or all three
 * outputs null -> MRX_ERR_INVALID with the outputs untouched */
int mrx_tod_bin_reduce(mrx_ctx* ctx, const float* d_x, size_t ld_x, const float* d_model, size_t ld_m,
                       const uint8_t* d_flags, size_t ld_f, int D, int T,
                       const int32_t* d_order, int n_order, const int32_t* d_start, int K, int min_hits,
                       double* d_sum, uint32_t* d_hits, float* d_template);

/* y[d][t] = x[d][t] + sign * template[d][d_bin[t]], sign = -1 or +1: one float32 subtraction or addition.  Where d_bin[t]
 * is outside 0 .. K - 1 (by convention -1) y[d][t] = x[d][t]: an unsigned comparison, and no template entry is read.
 *  d_x         [D][ld_x] float32
 *  d_bin       [T] int32, shared by every row
 *  d_template  [D][K] float32
 *  d_y         [D][ld_y] float32; d_y == d_x (with ld_y == ld_x) works in place; nothing is written past T in a row
 * 16-byte accesses where d_x, d_y, d_bin and both pitches allow them, 4-byte ones otherwise: no alignment beyond 4 bytes
 * is asked.  D < 1, T < 1, K outside 1 .. 4096, sign not -1 or +1, ld_x < T, ld_y < T or a null pointer ->
 * MRX_ERR_INVALID with d_y untouched */
int mrx_tod_bin_apply(mrx_ctx* ctx, const float* d_x, size_t ld_x, int D, int T, const int32_t* d_bin,
                      const float* d_template, int K, int sign, float* d_y, size_t ld_y);

/* ---- the common mode and other shared time templates: a flag-aware regression (maria_amd/regress.py) -- */

/* Common to the three entries below.  G groups, 1 <= G <= 16.  d_group [D] int32 names each row's group, NULL: every row
 * in group 0; a row whose entry is outside 0 .. G - 1 (by convention -1; an unsigned comparison) takes part in nothing.
 * d_flags [D][ld_f] uint8 or NULL: a nonzero flag keeps the sample out of SUMS, never out of the subtraction.
 * d_model [D][ld_m] float32 or NULL.  term(d, t) = (double)x[d][t] - (double)model[d][t], one rounding, plain
 * (double)x[d][t] when d_model is NULL.  Every operation written below is one float64 rounding (no fused
 * multiply-add).  The sums are REPRODUCIBLE, without atomics: a sum over rows is added in the ascending row order of the
 * group, a sum over time in an order that is a function of T alone (not of K, D, the flags, the pointers' alignment or
 * the other rows of the call), so the same inputs give the same bits on every call.  Inputs are never modified.  No
 * alignment beyond the element size is asked of any pointer or pitch: a thread's four consecutive samples are one
 * 16-byte access (flags: 4-byte) where the pointer and the pitch allow it, four accesses otherwise.  Nothing is written
 * past T in a row. */

/* The weighted mean across the rows of each group, sample by sample.  For group g and sample t, over the rows d of group
 * g with flags[d][t] == 0, in ascending d:
 *   S[g][t]    = sum of u[d] * (term(d, t) - off[d])
 *   W[g][t]    = sum of v[d]
 *   mean[g][t] = W > 0 ? (float)(S / W) : 0.0f                      (float64 quotient, rounded ONCE)
 * Rows of other groups (or of none) do not enter the order: adding such rows to a call leaves a group's bits as they are.
 *  d_x     [D][ld_x] float32
 *  d_u, d_v [D] float64;  d_off [D] float64 or NULL (zeros)
 *  d_S     [G][T] float64, OVERWRITTEN, or NULL
 *  d_W     [G][T] float64, OVERWRITTEN, or NULL
 *  d_mean  [G][ld_c] float32, OVERWRITTEN in [0, T) of each row, or NULL
 * D < 1, T < 1, G outside 1 .. 16, a pitch (of an array that is given) < T, a null d_x, d_u or d_v, or all three outputs
 * null -> MRX_ERR_INVALID with the outputs untouched */
int mrx_tod_column_mean(mrx_ctx* ctx, const float* d_x, size_t ld_x, const float* d_model, size_t ld_m,
                        const uint8_t* d_flags, size_t ld_f, int D, int T, const int32_t* d_group, int G,
                        const double* d_u, const double* d_v, const double* d_off,
                        double* d_S, double* d_W, float* d_mean, size_t ld_c);

/* Each row's normal equations against its group's K templates d_B [G][K][ld_b] float32, 1 <= K <= 8.  For row d with
 * g = group[d] and kept(d) = { t : flags[d][t] == 0 }:
 *   N[d][i][j] = sum over kept(d) of (double)B[g][i][t] * (double)B[g][j][t]   (the product of two float32 is exact)
 *   r[d][i]    = sum over kept(d) of (double)B[g][i][t] * term(d, t)           (the product one rounding)
 *   hits[d]    = |kept(d)|
 * N is the full symmetric K x K matrix.  A row outside every group gets zeros.  A row's sums do not depend on which
 * rows share the call.
 *  d_N     [D][K][K] float64, OVERWRITTEN
 *  d_r     [D][K] float64, OVERWRITTEN
 *  d_hits  [D] uint32, OVERWRITTEN, or NULL
 * D < 1, T < 1, G outside 1 .. 16, K outside 1 .. 8, a pitch (of an array that is given) < T, or a null d_x, d_B, d_N or
 * d_r -> MRX_ERR_INVALID with the outputs untouched */
int mrx_tod_regress_normal(mrx_ctx* ctx, const float* d_x, size_t ld_x, const float* d_model, size_t ld_m,
                           const uint8_t* d_flags, size_t ld_f, int D, int T, const int32_t* d_group, int G,
                           const float* d_B, size_t ld_b, int K, double* d_N, double* d_r, uint32_t* d_hits);

/* Subtract (sign -1) or add (sign +1) each row's fitted combination of its group's templates, d_a [D][K] float64:
 *   s = 0.0; for i = 0 .. K - 1: s = s + a[d][i] * (double)B[g][i][t]          (two roundings a step, in this order)
 *   y[d][t] = x[d][t] + sign * (float)s                                        (one float32 operation)
 * A row outside every group is copied.  d_y == d_x with ld_y == ld_x works in place.
 * D < 1, T < 1, G outside 1 .. 16, K outside 1 .. 8, sign not -1 or +1, ld_x, ld_y or ld_b < T, a null d_x, d_B, d_a or
 * d_y, or d_y == d_x with ld_y != ld_x -> MRX_ERR_INVALID with d_y untouched */
int mrx_tod_regress_apply(mrx_ctx* ctx, const float* d_x, size_t ld_x, int D, int T, const int32_t* d_group, int G,
                          const float* d_B, size_t ld_b, int K, const double* d_a, int sign, float* d_y, size_t ld_y);

/* ---- planar and quadratic sky subtraction: a fit ACROSS the rows, sample by sample (maria_amd/sky_polynomial.py,
 * DESIGN 3.36) ------------------------------------------------------------------------------------------------------- */

/* Common to the two entries below.  The groups (1 <= G <= 16, a row whose entry is outside 0 .. G - 1 takes part in
 * nothing), d_flags, d_model, their pitches, term(d, t), the single float64 roundings (no fused multiply-add), the
 * absence of atomics, the alignment (none beyond the element size), "nothing is written past T" and "inputs are never
 * modified" are those of the block above mrx_tod_column_mean.  d_P [D][K] float64, 1 <= K <= 6: the value of each of
 * the K basis functions at the row (its detector's focal-plane position; maria_amd.sky_polynomial.basis). */

/* The least-squares fit of the K basis functions across the rows of each group, at every sample: the transpose of
 * mrx_tod_regress_normal.  A row takes part iff it is in a group and v[d] > 0; other rows are not read at all.  For
 * group g and sample t, over the participating rows d with flags[d][t] == 0, in ascending d:
 *   r[i]    = sum of (u[d] * P[d][i]) * (term(d, t) - off[d])
 *   N[i][j] = sum of (v[d] * P[d][i]) * P[d][j]                      for i <= j
 *   hits    = their number
 * The order of the additions is the ascending row order of the group; it does not depend on the other rows or the other
 * samples of the call, on alignment or on K (at K = 1 with P = 1, N and r are the bits of mrx_tod_column_mean's W and S).
 * Then, in float64, every operation one rounding, the solve of N c = r:
 *   s_i  = 1.0 / sqrt(N_ii);   M_ij = (N_ij * s_i) * s_j  (i <= j);   b_i = r_i * s_i
 *   for j = 0 .. K - 1:   p_j = M_jj;  for k = 0 .. j - 1: p_j = p_j - L_jk * L_jk;   L_jj = sqrt(p_j);  q_j = 1.0 / L_jj
 *                         for i = j + 1 .. K - 1:  w = M_ji;  for k = 0 .. j - 1: w = w - L_ik * L_jk;   L_ij = w * q_j
 *   for i = 0 .. K - 1:   w = b_i;  for k = 0 .. i - 1: w = w - L_ik * z_k;   z_i = w * q_i
 *   for i = K - 1 .. 0:   w = z_i;  for k = i + 1 .. K - 1: w = w - L_ki * a_k;   a_i = w * q_i
 *   c_i  = a_i * s_i
 * The sample is fitted iff hits >= max(min_hits, K), every N_ii > 0 and every pivot p_j >= rcond (a NaN compares
 * false): the verdict of maria_amd.regress.solve.  A sample that is not fitted gets c = 0 and ok = 0.
 *  d_x     [D][ld_x] float32
 *  d_u, d_v [D] float64;  d_off [D] float64 or NULL (zeros)
 *  d_c     [G][K][ld_c] float64, OVERWRITTEN in [0, T) of each row
 *  d_ok    [G][T] uint8, OVERWRITTEN (1: fitted)
 *  d_hits  [G][T] uint32, OVERWRITTEN, or NULL
 *  d_N     [G][K (K + 1) / 2][T] float64, the upper triangle row after row, OVERWRITTEN, or NULL
 *  d_r     [G][K][T] float64, OVERWRITTEN, or NULL
 * D < 1, T < 1, G outside 1 .. 16, K outside 1 .. 6, a pitch (of an array that is given) < T, rcond outside [0, 1),
 * min_hits < 1, or a null d_x, d_P, d_u, d_v, d_c or d_ok -> MRX_ERR_INVALID with the outputs untouched */
int mrx_tod_column_fit(mrx_ctx* ctx, const float* d_x, size_t ld_x, const float* d_model, size_t ld_m,
                       const uint8_t* d_flags, size_t ld_f, int D, int T, const int32_t* d_group, int G,
                       const double* d_P, int K, const double* d_u, const double* d_v, const double* d_off,
                       int min_hits, double rcond, double* d_c, size_t ld_c, uint8_t* d_ok, uint32_t* d_hits,
                       double* d_N, double* d_r);

/* Subtract (sign -1) or add (sign +1) each row's share of its group's fitted surface.  For a row d of group g:
 *   s = 0.0; for i = 0 .. K - 1: s = s + c[g][i][t] * P[d][i]                  (two roundings a step, in this order)
 *   y[d][t] = x[d][t] + sign * (float)(e[d] + h[d] * s)                        (one float32 operation)
 * d_e [D] float64 or NULL (zeros), d_h [D] float64.  A row outside every group is copied.  d_y == d_x with
 * ld_y == ld_x works in place.
 * D < 1, T < 1, G outside 1 .. 16, K outside 1 .. 6, sign not -1 or +1, ld_x, ld_y or ld_c < T, a null d_x, d_P, d_c,
 * d_h or d_y, or d_y == d_x with ld_y != ld_x -> MRX_ERR_INVALID with d_y untouched */
int mrx_tod_column_apply(mrx_ctx* ctx, const float* d_x, size_t ld_x, int D, int T, const int32_t* d_group, int G,
                         const double* d_P, int K, const double* d_c, size_t ld_c, const double* d_e,
                         const double* d_h, int sign, float* d_y, size_t ld_y);

/* ---- the subscan polynomial filter: a Legendre fit per (row, segment) (maria_amd/subscans.py) ---------- */

/* Common to the two entries below.  d_flags, d_model, their pitches, term(d, t), the single float64 roundings (no fused
 * multiply-add), the absence of atomics, the alignment (none beyond the element size), "nothing is written past T" and
 * "inputs are never modified" are those of the block above mrx_tod_column_mean.
 * Segments: d_bound [S + 1] int32 on the device, S >= 1.  Segment s is [lo, hi) with lo = clamp(bound[s], 0, T) and
 * hi = clamp(bound[s + 1], 0, T); hi <= lo: the segment is empty.  Samples in no segment belong to nothing.  The kernels
 * clamp, so that no content of d_bound makes them read or write out of range; ascending order is the caller's business
 * (where segments overlap, mrx_tod_segment_apply gives a sample to one of them).
 * The basis of a segment of L = hi - lo samples, 1 <= K <= 8:
 *   u(t)    = L > 1 ? (double)(2 * (t - lo) - (L - 1)) / (double)(L - 1) : 0.0     (integer numerator, one division)
 *   P_0 = 1.0;  P_1 = u
 *   P_{n+1} = ((((double)(2n + 1) * u) * P_n) - ((double)n * P_{n-1})) * c_n,   c_n = 1.0 / (double)(n + 1), rounded once */

/* The normal equations of every (row, segment).  For row d, segment s and kept = { t in the segment : flags[d][t] == 0 }:
 *   N[d][s][i][j] = sum over kept of P_i * P_j                       (the product one rounding; the full symmetric matrix)
 *   r[d][s][i]    = sum over kept of P_i * term(d, t)
 *   hits[d][s]    = |kept|
 * An empty segment gets zeros.  The sums of a (row, segment) are added in an order that is a function of lo and hi alone
 * (not of K, D, S, the flags, the pitches, the pointers' alignment or what else is in the call): the same inputs give the
 * same bits on every call, and for a row or a segment computed alone.
 *  d_x     [D][ld_x] float32
 *  d_N     [D][S][K][K] float64, OVERWRITTEN
 *  d_r     [D][S][K] float64, OVERWRITTEN
 *  d_hits  [D][S] uint32, OVERWRITTEN, or NULL
 * D < 1, T < 1, S < 1, K outside 1 .. 8, a pitch (of an array that is given) < T, or a null d_x, d_bound, d_N or d_r ->
 * MRX_ERR_INVALID with the outputs untouched */
int mrx_tod_segment_normal(mrx_ctx* ctx, const float* d_x, size_t ld_x, const float* d_model, size_t ld_m,
                           const uint8_t* d_flags, size_t ld_f, int D, int T, const int32_t* d_bound, int S, int K,
                           double* d_N, double* d_r, uint32_t* d_hits);

/* Subtract (sign -1) or add (sign +1) each segment's polynomial, d_a [D][S][K] float64:
 *   s = 0.0; for i = 0 .. K - 1: s = s + a[d][seg][i] * P_i(u(t))               (two roundings a step, in this order)
 *   y[d][t] = x[d][t] + sign * (float)s                                        (one float32 operation)
 * Samples in no segment are copied.  d_y == d_x with ld_y == ld_x works in place.
 * D < 1, T < 1, S < 1, K outside 1 .. 8, sign not -1 or +1, ld_x or ld_y < T, a null d_x, d_bound, d_a or d_y, or
 * d_y == d_x with ld_y != ld_x -> MRX_ERR_INVALID with d_y untouched */
int mrx_tod_segment_apply(mrx_ctx* ctx, const float* d_x, size_t ld_x, int D, int T, const int32_t* d_bound, int S, int K,
                          const double* d_a, int sign, float* d_y, size_t ld_y);

/* The frozen projector of the subscan filter, in place on d_x, forward or transposed (maria_amd/subscans.py: freeze,
 * project).  With M = (flags == 0), T the segment's basis and A = d_A[d][s] (the caller's N^-1, symmetric):
 *   transpose 0:  F   = I - T A T^t M        transpose 1:  F^t = I - M T A T^t
 * For every (row, segment) with d_ok[d][s] != 0 and hi > lo:
 *   pass 1   r[i] = sum of P_i * (double)x[d][t] over the segment's t with flags[d][t] == 0 (transpose 0: a flagged
 *            sample is selected away, never multiplied) or over all of its t (transpose 1), added in the order of
 *            mrx_tod_segment_normal's r: the same bits as that entry gives for the same x and flags (without flags)
 *   solve    a[i] = s, with s = 0.0; for j = 0 .. K - 1: s = s + A[i][j] * r[j]
 *   pass 2   x[d][t] = x[d][t] - (float)s2, with s2 = 0.0; for i = 0 .. K - 1: s2 = s2 + a[i] * P_i(u(t))
 *            (mrx_tod_segment_apply's expression, sign -1) on every t of the segment (transpose 0) or on those with
 *            flags[d][t] == 0 (transpose 1)
 * and d_a[d][s] = a.  A pair with d_ok == 0, or an empty segment, is neither read nor written in d_x; its d_a is zeros.
 * Samples in no segment are untouched.  d_flags NULL: nothing is flagged.  Segments must not overlap (ascending bounds:
 * the caller's business, as above); the bounds are clamped.  No atomics: the same bits on every call, for a row or a
 * segment computed alone, and at any alignment.
 *  d_x     [D][ld_x] float32, MODIFIED in place
 *  d_A     [D][S][K][K] float64
 *  d_ok    [D][S] uint8
 *  d_a     [D][S][K] float64, OVERWRITTEN, or NULL
 * D < 1, T < 1, S < 1, K outside 1 .. 8, transpose not 0 or 1, ld_x < T, ld_f < T with flags given, or a null d_x,
 * d_bound, d_A or d_ok -> MRX_ERR_INVALID with d_x and d_a untouched */
int mrx_tod_segment_project(mrx_ctx* ctx, float* d_x, size_t ld_x, const uint8_t* d_flags, size_t ld_f, int D, int T,
                            const int32_t* d_bound, int S, int K, const double* d_A, const uint8_t* d_ok, int transpose,
                            double* d_a);

/* ---- narrow spectral lines: an amplitude and a phase per (row, segment) (maria_amd/lines.py) ----------- */

/* Common to the two entries below.  d_flags, d_model, their pitches, term(d, t), the single float64 roundings (no fused
 * multiply-add), the absence of atomics, the alignment (none beyond the element size), "nothing is written past T" and
 * "inputs are never modified" are those of the block above mrx_tod_column_mean; d_bound [S + 1], its clamping to 0 .. T
 * in the kernels and the empty segment are those of the block above mrx_tod_segment_normal.
 * The basis of a segment [lo, hi) of n = hi - lo samples for row d: n_poly in 0 .. 2 baseline functions and the two
 * carriers of each of L lines, 1 <= L <= 3; K = n_poly + 2 L <= 8.  d_nu [D][L] float64 on the device: the frequency of
 * line l in row d in cycles a sample, read as given (no range is enforced; a non-finite entry makes the sums of its own
 * row NaN and nothing else).
 *   B_0 = P_0 = 1.0,  B_1 = P_1 = u(t)          (the first n_poly of them: u and P of the block above
 *                                                mrx_tod_segment_normal, a local baseline that keeps a drift out of the line)
 *   theta = nu[d][l] * (double)t                (t the sample's index from the START OF THE ROW, not of the segment: the
 *                                                phase is continuous across segments; the product one rounding)
 *   q     = theta - rint(theta)                 (exact: |q| <= 1/2 lies on theta's own grid)
 *   B_{n_poly + 2 l}     = cospi(2.0 * q)       (2.0 * q exact; cospi and sinpi the device library's float64 functions,
 *   B_{n_poly + 2 l + 1} = sinpi(2.0 * q)        exactly 0 and +-1 at the quarter cycles)
 * Every carrier is evaluated at its own sample; nothing is carried from one sample to the next. */

/* The normal equations of every (row, segment).  For row d, segment s and kept = { t in the segment : flags[d][t] == 0 }:
 *   N[d][s][i][j] = sum over kept of B_i * B_j                       (the product one rounding; the full symmetric matrix)
 *   r[d][s][i]    = sum over kept of B_i * term(d, t)
 *   hits[d][s]    = |kept|
 * A flagged sample is selected away, never multiplied: what it holds (1e30 and NaN included) changes no bit.  An unflagged
 * NaN stays in the r of its own (row, segment).  An empty segment gets zeros.  The sums of a (row, segment) are added in an
 * order that is a function of lo and hi alone (mrx_tod_segment_normal's; not of L, n_poly, D, S, the flags, the pitches,
 * the pointers' alignment or what else is in the call): the same inputs give the same bits on every call, and for a row
 * or a segment computed alone.
 *  d_x     [D][ld_x] float32
 *  d_N     [D][S][K][K] float64, OVERWRITTEN
 *  d_r     [D][S][K] float64, OVERWRITTEN
 *  d_hits  [D][S] uint32, OVERWRITTEN, or NULL
 * D < 1, T < 1, S < 1, L outside 1 .. 3, n_poly outside 0 .. 2, a pitch (of an array that is given) < T, or a null d_x,
 * d_bound, d_nu, d_N or d_r -> MRX_ERR_INVALID with the outputs untouched */
int mrx_tod_line_normal(mrx_ctx* ctx, const float* d_x, size_t ld_x, const float* d_model, size_t ld_m,
                        const uint8_t* d_flags, size_t ld_f, int D, int T, const int32_t* d_bound, int S,
                        const double* d_nu, int L, int n_poly, double* d_N, double* d_r, uint32_t* d_hits);

/* Subtract (sign -1) or add (sign +1) each segment's lines, d_a [D][S][K] float64.  Only the carriers are applied: the
 * baseline coefficients a[..][0 .. n_poly - 1] are nuisance parameters and are not read.
 *   s = 0.0; for i = n_poly .. K - 1: s = s + a[d][seg][i] * B_i               (two roundings a step, in this order)
 *   y[d][t] = x[d][t] + sign * (float)s                                        (one float32 operation)
 * Samples in no segment are copied.  d_y == d_x with ld_y == ld_x works in place.
 * D < 1, T < 1, S < 1, L outside 1 .. 3, n_poly outside 0 .. 2, sign not -1 or +1, ld_x or ld_y < T, a null d_x, d_bound,
 * d_nu, d_a or d_y, or d_y == d_x with ld_y != ld_x -> MRX_ERR_INVALID with d_y untouched */
int mrx_tod_line_apply(mrx_ctx* ctx, const float* d_x, size_t ld_x, int D, int T, const int32_t* d_bound, int S,
                       const double* d_nu, int L, int n_poly, const double* d_a, int sign, float* d_y, size_t ld_y);

/* ---- statistics per (row, segment) and the flagging of whole segments (maria_amd/cuts.py) ------------- */

/* Common to the two entries below.  d_flags, d_model, their pitches, term(d, t), the single float64 roundings (no fused
 * multiply-add), the absence of atomics, the alignment (none beyond the element size), "nothing is written past T" and
 * "inputs are never modified" are those of the block above mrx_tod_column_mean; d_bound [S + 1], its clamping to 0 .. T
 * in the kernels and the empty segment are those of the block above mrx_tod_segment_normal. */

/* The moments of every (row, segment).  For row d, segment s = [lo, hi), kept = { t in [lo, hi) : flags[d][t] == 0 } and
 * n = |kept|:
 *   count[d][s][0] = n
 *   count[d][s][1] = p, the number of t with t and t + 1 both in [lo, hi) and both kept
 *   stat[d][s][0]  = mu = (sum over kept of term(d, t)) / (double)n                     (one sum, one division)
 *   stat[d][s][1]  = M2 = sum over kept of e * e,        e = term(d, t) - mu            (mu: the rounded value stored)
 *   stat[d][s][2]  = M3 = sum over kept of (e * e) * e
 *   stat[d][s][3]  = M4 = sum over kept of (e * e) * (e * e)
 *   stat[d][s][4]  = min, stat[d][s][5] = max of term(d, t) over kept                   (exact)
 *   stat[d][s][6]  = D2 = sum over the p pairs of (term(d, t + 1) - term(d, t))^2
 *   stat[d][s][7]  = 0.0, reserved
 * n == 0: all eight values are 0.0; p == 0: D2 = 0.0.  A flagged sample is selected away, never multiplied: the results
 * do not depend on what flagged samples hold (1e30 and NaN included).  An unflagged NaN makes stat[d][s][0 .. 6] of its own
 * (row, segment) NaN and nothing else.  Every sum of a (row, segment) is added in an order that is a function of lo and hi
 * alone (not of D, S, the flags, the model, the pitches, the pointers' alignment or what else is in the call): the same
 * inputs give the same bits on every call, and for a row or a segment computed alone.  A sum of L terms is within
 * L 2^-53 sum|terms| of the exact sum of its rounded terms, to first order.
 *  d_x      [D][ld_x] float32
 *  d_stat   [D][S][8] float64, OVERWRITTEN
 *  d_count  [D][S][2] uint32, OVERWRITTEN
 * D < 1, T < 1, S < 1, a pitch (of an array that is given) < T, or a null d_x, d_bound, d_stat or d_count ->
 * MRX_ERR_INVALID with the outputs untouched */
int mrx_tod_segment_moments(mrx_ctx* ctx, const float* d_x, size_t ld_x, const float* d_model, size_t ld_m,
                            const uint8_t* d_flags, size_t ld_f, int D, int T, const int32_t* d_bound, int S,
                            double* d_stat, uint32_t* d_count);

/* Flag whole segments IN PLACE: flags[d][t] |= value for every t of a segment s with d_mask[d][s] != 0.  Samples in no
 * segment, the segments whose mask is 0 and the bytes past T of a row are untouched.  Where segments overlap a sample
 * belongs to one of them, as in mrx_tod_segment_apply.
 *  d_flags  [D][ld_f] uint8
 *  d_mask   [D][S] uint8
 * D < 1, T < 1, S < 1, value outside 1 .. 255, ld_f < T, or a null d_flags, d_bound or d_mask -> MRX_ERR_INVALID with
 * the flags untouched */
int mrx_tod_segment_flag(mrx_ctx* ctx, uint8_t* d_flags, size_t ld_f, int D, int T, const int32_t* d_bound, int S,
                         const uint8_t* d_mask, int value);

/* ---- the covariance between detectors: the flag-aware Gram matrix (maria_amd/covariance.py) ----------- */

/* The samples of one float32 chain of mrx_tod_gram: time is cut at the multiples of MRX_GRAM_BLOCK from t = 0. */
#define MRX_GRAM_BLOCK 256

/* G = Z Z^T over the rows a list names.  d_flags, d_model, their pitches, term(d, t), the alignment (none beyond the
 * element size), "nothing is read past T in a row" and "inputs are never modified" are those of the block above
 * mrx_tod_column_mean.
 *  d_rows    [R] int32, the rows that take part, in any order (a row may be named twice); NULL: R = D and row i is i.  An
 *            entry outside 0 .. D - 1 (an unsigned comparison) is a row of zeros: its row and column of G and n are 0
 *  d_center  [D] float64, indexed by the row of x; NULL: zeros
 *   z(d, t)  = flags[d][t] == 0 ? (float)(term(d, t) - center[d]) : 0.0f     (one float64 subtraction, one rounding to
 *              float32).  A flagged sample is selected away, never multiplied: 1e30 or NaN under a flag changes no bit.
 *              An unflagged NaN makes row and column i of G NaN and nothing else
 *   G[i][j]  = sum over t of z(rows[i], t) * z(rows[j], t)
 *   n[i][j]  = |{ t : flags[rows[i]][t] == 0 and flags[rows[j]][t] == 0 }|, exact; T for rows in range when d_flags is NULL
 * G[i][j] and G[j][i] are the same bits: only the 128 x 128 tiles on and above the diagonal are computed, the rest is
 * their mirror.
 * Order of a sum.  Inside a block [b MRX_GRAM_BLOCK, min((b + 1) MRX_GRAM_BLOCK, T)) it is the float32 chain
 *   s = 0.0f; for t ascending: s = fmaf(z_i(t), z_j(t), s)
 * (v_mfma_f32_32x32x2_f32, which is that chain bit for bit); the block sums are added in float64 in ascending b from 0.0,
 * one rounding each.  The order is a function of T alone: not of R, D, the row list, the flags, the pitches, the
 * pointers' alignment or what else is in the call.  Time is not split across workgroups; no atomics.  The same inputs
 * give the same bits on every call, and G[i][j] depends on rows[i], rows[j] and T only.  To first order
 *   |G[i][j] - exact| <= (MRX_GRAM_BLOCK * 2^-24 + ceil(T / MRX_GRAM_BLOCK) * 2^-53) * sum over t of |z_i(t) z_j(t)|
 * against the exact sum of the products of the rounded z.
 *  d_x   [D][ld_x] float32
 *  d_G   [R][R] float64, OVERWRITTEN
 *  d_n   [R][R] uint32, OVERWRITTEN, or NULL.  With d_flags it is a second pass of the same kernel on the 0/1 weights
 *        (their float32 block sums are exact integers); without d_flags a fill; with d_n NULL nothing is launched for it
 * D < 1, T < 1, R < 1, a pitch (of an array that is given) < T, or a null d_x or d_G -> MRX_ERR_INVALID with the outputs
 * untouched */
int mrx_tod_gram(mrx_ctx* ctx, const float* d_x, size_t ld_x, const float* d_model, size_t ld_m,
                 const uint8_t* d_flags, size_t ld_f, int D, int T, const int32_t* d_rows, int R,
                 const double* d_center, double* d_G, uint32_t* d_n);

/* ---- beam, pointing offset and gain per detector from a source scan (maria_amd/beamfit.py) ------------- */

/* Common to the two entries below.  The pointing arguments are mrx_bin_map's, in its order (d_az, d_el [T] float32,
 * d_transform [T][9] float64 or NULL, d_dx, d_dy [D] float32), and the offsets (ox, oy) of detector d at sample t from the
 * frame's centre (center_phi, center_theta, radians) are the float32 numbers the binning computes for a map of that
 * centre: steps 1-3 of mrx_map_sample.hip (mrx_map_pointing.h) in the composed form, by the same code built with the same flags
 * (mrx_map_pointing.h: sample_const, make_det_const, sample_offsets).  With MRX_OPT_POINTING_CHAIN set both return
 * MRX_ERR_UNSUPPORTED and launch nothing.
 *  d_src   [T][2] float32 or NULL: the source's offsets (src_x, src_y) from that centre at every sample (a planet that
 *          moves); NULL: the source sits at the centre, (0, 0)
 *  (u, v) = ((double)ox - (double)src_x(t), (double)oy - (double)src_y(t))
 * d_flags [D][ld_f] uint8 of any pitch, no alignment beyond the element's.  No atomics: the same inputs give the same
 * bits on every call. */

/* The per-sample source mask:  flags[d][t] |= value  where u u + v v <= radius radius (inside = 1) or > radius radius
 * (inside = 0), (ox, oy) from the detector's d_dx, d_dy; float64 products and one sum, compared with the float64 product
 * radius radius.  One streaming pass in the TOD tile (16 rows x 1024 samples); a byte is written only where a bit is set,
 * and nothing outside the D x T flags is touched.
 * D < 1, T < 1, ld_f < T, value outside 1 .. 255, inside not 0 or 1, a radius that is negative or not finite, a centre
 * that is not finite, or a null d_az, d_el, d_dx, d_dy or d_flags -> MRX_ERR_INVALID with the flags untouched */
int mrx_tod_source_flag(mrx_ctx* ctx, const float* d_az, const float* d_el, int T, const double* d_transform,
                        const float* d_dx, const float* d_dy, int D, double center_phi, double center_theta,
                        const float* d_src, double radius, int inside, int value, uint8_t* d_flags, size_t ld_f);

/* The Gauss-Newton sums of a Gaussian beam model per detector at the trial parameters d_param [D][K] float64:
 *   K = 5: (A, dx, dy, w, c)          q = w (u u + v v)                       w = 1 / sigma^2
 *   K = 7: (A, dx, dy, a, b, cc, c)   q = a (u u) + 2 b (u v) + cc (v v)      a quadratic form: no angle
 *   term = (double)x[d][t] - (double)model[d][t]  (plain (double)x without a model)
 *   g = exp(-q / 2);   m = A g + c;   r = term - m
 * The row's trial (dx, dy) are rounded to float32 and go through make_det_const and sample_offsets IN PLACE of
 * d_dx[d], d_dy[d] (which this entry does not read: they may be NULL): at the optimum the offsets the fit saw are the
 * bits the binning will see.  u, v are taken to float64 from the float32 offsets; everything after is float64, one
 * rounding an operation (no fused multiply-add).  J = dm/dparam:
 *   J_A = g;  J_c = 1;  m_u = -(A g) (w u | a u + b v);  m_v = -(A g) (w v | b u + cc v)
 *   J_w = -(A g) (u u + v v) / 2       |   J_a = -(A g) (u u) / 2,  J_b = -(A g) (u v),  J_cc = -(A g) (v v) / 2
 *   J_dx = m_u d ox/d dx + m_v d oy/d dx,   J_dy likewise, with
 *   d(ox, oy)/d(dx, dy) = -f (dc/d. @ G):  c = (-dy s, cos r, -dx s) the detector's unit vector, s = sin r / r,
 *   h = (cos r - s) / r^2 (its series below r^2 = 0.09, make_det_const's threshold),
 *   dc/ddx = (-dx dy h, -dx s, -s - dx^2 h),  dc/ddy = (-s - dy^2 h, -dy s, -dx dy h),
 *   G the sample's composed rotation (dz = c @ G, float32 as sample_const stores it) and f the asin(r)/r factor of
 *   sample_offsets, HELD CONSTANT in the derivative.  What that neglects is of relative order |dz|^2 (the squared
 *   angle between the detector's direction and the frame's centre); the residual r itself is exact, so the fixed point
 *   of the iteration is the least-squares one to that order.
 * Per row over the samples whose flag is 0 (all of them without d_flags), with nv = 1 + K (K + 1) / 2 + K:
 *   d_count[d] = hits
 *   d_out[d][0] = chi2 = sum r r;   d_out[d][1 ..] = the upper triangle of JtJ row by row ((0,0), (0,1) .. (K-1,K-1));
 *   d_out[d][1 + K (K + 1) / 2 ..] = Jtr = sum J_i r
 * Order of the sums: a thread owns 4 consecutive samples of each tile of 1024, adds its kept samples ascending, the 64
 * lanes of a wave meet in a butterfly (xor 32 .. 1), a wave adds tile after tile of its chunk of 16 tiles, the 4 waves of
 * a chunk are added in wave order and a row's chunks in ascending order: a function of T alone.  A wave's worth of
 * samples without a kept one is skipped (it would add +0.0), so a scan whose window is a few per cent of the samples
 * costs about one read of the flags.  A flagged sample's value is never read: what it holds (NaN included) changes no
 * bit.  A row with nothing kept gives zeros and hits = 0.  Inputs are never modified.
 *  d_x, d_model  [D][ld] float32, the model or NULL;  d_out [D][nv] float64 and d_count [D] int32, OVERWRITTEN
 *  d_work  8-byte aligned, at least mrx_tod_beam_normal_work_bytes(D, T, K): the sums per (row, chunk), the trial
 *          offsets in float32 and the samples' rotations G [T][6] (sample_const once per call for all rows)
 * D < 1, T < 1, K not 5 or 7, a pitch (of an array that is given) < T, a centre that is not finite, a work buffer
 * too small or misaligned, or a null d_x, d_az, d_el, d_param, d_out, d_count or d_work -> MRX_ERR_INVALID with the
 * outputs untouched */
int mrx_tod_beam_normal_work_bytes(int D, int T, int K, size_t* bytes);
int mrx_tod_beam_normal(mrx_ctx* ctx, const float* d_x, size_t ld_x, const float* d_model, size_t ld_m,
                        const uint8_t* d_flags, size_t ld_f, const float* d_az, const float* d_el, int T,
                        const double* d_transform, const float* d_dx, const float* d_dy, int D, double center_phi,
                        double center_theta, const float* d_src, const double* d_param, int K, double* d_out,
                        int32_t* d_count, void* d_work, size_t work_bytes);

/* ---- detector time constants: the one-pole lag and its exact inverse (maria_amd/time_constants.py) ------ */

/* Common to the two entries below.  A detector answers optical power through a one-pole low-pass of time constant tau;
 * at the sample rate fs its pole is a = exp(-1 / (fs tau)).
 *  d_x, d_y  [D][ld] float32, pitches in elements; no alignment beyond the element size (16-byte accesses where
 *            pointer and pitch allow it)
 *  d_a       [D] float64 on the device: the pole of every row.  a = 0: no lag.  A row whose a is not in [0, 1), NaN
 *            included, is copied, and so is a row with a = 0, bit for bit: no content of d_a makes a kernel read or
 *            write out of range, and none makes the lag turn finite samples into Inf or NaN (its results are convex
 *            combinations of samples).  The inverse has the gain (1 + a) / (1 - a) of its definition
 *  init      0: zero state before the first sample (scipy.signal.lfilter without zi); 1: steady state, the detector has
 *            seen x[0] for ever
 * Every operation written below is one float64 rounding (no fused multiply-add).  No atomics, and no workgroup waits for
 * another: every bit of a row's result is a function of that row's samples, its a, T and init alone, not of D, the
 * pitches, the pointers' alignment or what else is in the call.  The output with the same pitch as the input and
 * d_y == d_x works in place.  Nothing is written past T in a row; inputs are otherwise never modified.
 * D < 1, T < 1, a pitch < T, init not 0 or 1, a null d_x, d_a or d_y, or d_y == d_x with ld_y != ld_x ->
 * MRX_ERR_INVALID with the output untouched */

/* The lag.  With g = 1.0 - a the result is the float32 rounding of the serial float64 recurrence
 *   y64[0] = init ? (double)x[0] : g * (double)x[0]
 *   y64[t] = a * y64[t - 1] + g * (double)x[t]
 *   y[t]   = (float)y64[t]
 * evaluated time-parallel (a scan of the affine maps s -> a^k s + B over tiles of 1024 samples, powers of a and the
 * carry from tile to tile in float64; one workgroup a row): |y - y64| <= 2^-24 |y64| + 64 * 2^-53 * max|x| / (1 - a). */
int mrx_tod_onepole(mrx_ctx* ctx, const float* d_x, size_t ld_x, int D, int T, const double* d_a, int init, float* d_y,
                    size_t ld_y);

/* The exact inverse, a two-tap FIR.  With r = 1.0 / (1.0 - a), in this order:
 *   x[0] = init ? y[0] : (float)((double)y[0] * r)
 *   x[t] = (float)(((double)y[t] - a * (double)y[t - 1]) * r)
 * the same bits as these lines on the host.  Of a float32 TOD that mrx_tod_onepole made it returns the input to
 *   |x' - x| <= 2^-24 |x| + (1 + a) / (1 - a) * 2^-23 * max|y|. */
int mrx_tod_onepole_inverse(mrx_ctx* ctx, const float* d_y, size_t ld_y, int D, int T, const double* d_a, int init,
                            float* d_x, size_t ld_x);

/* ---- a rotating half-wave plate (maria_amd/hwp.py) ---------------------------------------------------- */

/* The lock-in decimator.  With the carrier c[t] = (cos 4 chi(t), sin 4 chi(t)), H = (n_taps - 1) / 2 and
 * T_out = (T + q - 1) / q, for j = 0 .. T_out - 1 and every sum over -H <= i <= H with 0 <= j q + i < T:
 *   y_t[d][j] =     sum_i hT[H + i]               x[d][j q + i] / sum_i hT[H + i]
 *   y_q[d][j] = 2 * sum_i hP[H + i] c[j q + i][0] x[d][j q + i] / sum_i hP[H + i]
 *   y_u[d][j] = 2 * sum_i hP[H + i] c[j q + i][1] x[d][j q + i] / sum_i hP[H + i]
 * The products c x are float64, one rounding; each sum runs over the tap index ascending as acc = fma(h, term, acc) in
 * float64 from 0; the quotient is float64 and the result rounded ONCE to float32.  y_t is mrx_tod_decimate(x, q, hT)
 * bit for bit.  Orientation, edges (taps outside the row dropped, the rest renormalised) and the time of output j
 * (t[j q]) are mrx_tod_decimate's.  The kernel does no trigonometry: the carrier is taken as given.
 *  d_x        [D][ld_x] float32, read only
 *  d_carrier  [T][2] float64
 *  d_taps_t   [n_taps] float64 (hT); may be NULL where d_t is
 *  d_taps_p   [n_taps] float64 (hP)
 *  d_t        [D][ld_y] float32, or NULL: polarisation only (d_q and d_u then hold the bits of the three-output call)
 *  d_q, d_u   [D][ld_y] float32; nothing is written past T_out in a row
 * No alignment beyond the element size is asked of the pointers or pitches.  q outside 2 .. 32, n_taps even or outside
 * 1 .. 1025, D < 1, T < 1, ld_x < T, ld_y < T_out, an output equal to d_x or to another output, or a null pointer other
 * than d_t (with it, d_taps_t) -> MRX_ERR_INVALID with the outputs untouched */
int mrx_tod_demodulate(mrx_ctx* ctx, const float* d_x, size_t ld_x, int D, int T, int q, const double* d_carrier,
                       const double* d_taps_t, const double* d_taps_p, int n_taps, float* d_t, float* d_q, float* d_u,
                       size_t ld_y);

/* The simulation's combine: out[d][t] = (float) fma(s[d][t], c[t][1], fma(c_[d][t], c[t][0], i[d][t])) in float64 on the
 * float32 fields i, c_ (= d_c) and s, one rounding: i + c_ cos 4 chi + s sin 4 chi.
 *  d_i, d_c, d_s  [D][ld_in] float32
 *  d_carrier      [T][2] float64
 *  d_out          [D][ld_out] float32; d_out == d_i with ld_out == ld_in works in place; nothing is written past T in a row
 * No alignment beyond the element size (16-byte accesses where pointer and pitch allow it).  D < 1, T < 1, a pitch < T,
 * d_out equal to d_c or d_s, d_out == d_i with ld_out != ld_in, or a null pointer -> MRX_ERR_INVALID with d_out untouched */
int mrx_tod_hwp_modulate(mrx_ctx* ctx, const float* d_i, const float* d_c, const float* d_s, size_t ld_in, int D, int T,
                         const double* d_carrier, float* d_out, size_t ld_out);

/* ---- TOD pre-processing for the mappers (tod/processing.py:91-204) --------------------- */

/* remove_slope (D -= linspace(D[:, 0], D[:, -1], T), processing.py:99-105) and / or window
 * (D *= w, processing.py:139-146) on a [D][ld] float32 TOD in place, each step rounded to
 * float32 as the reference's in-place numpy operations do.
 *  d_window [T] float64 window (scipy.signal.windows.*, host) or NULL
 *  d_work   2 * D doubles of scratch (only read when remove_slope is set) */
int mrx_tod_detrend_window(mrx_ctx* ctx, float* d_data, size_t ld, int D, int T, int remove_slope,
                           const double* d_window, double* d_work);

/* scipy.signal.sosfilt along time (utils/signal/filters.py:46-69; zero initial state,
 * transposed direct form II, float64) of every row, optionally after remove_slope
 * (processing.py:151): the low-pass and the high-pass of process_tod are one cascade.  The
 * recursion is time-parallel: chunks of mrx_sosfilt_chunk() samples are run from a zero state,
 * chained through the chunk transition matrix and run again from their true initial state; the
 * result equals the serial loop up to float64 rounding.
 *  sos            [n_sections][6] host array (b0 b1 b2 a0 a1 a2), n_sections <= 8
 *  d_chunk_matrix [2 n][2 n] float64, device: the state transition of the cascade over one
 *                 chunk, state order (z0, z1) per section (maria_amd/tod_processing.py builds it)
 *  d_in, d_out    [D][ld] float32; may be the same buffer
 *  d_work         mrx_sosfilt_work_doubles(D, T, n_sections) doubles */
int mrx_sosfilt_chunk(void);
int mrx_sosfilt_work_doubles(int D, int T, int n_sections, size_t* doubles);
int mrx_sosfilt(mrx_ctx* ctx, const double* sos, int n_sections, const double* d_chunk_matrix,
                const float* d_in, size_t ld_in, int D, int T, int remove_slope, float* d_out,
                size_t ld_out, double* d_work);

/* The transpose of mrx_tod_detrend_window, x = S^T diag(w) y in place on a [D][ld] float32 TOD: the adjoint of
 * remove_slope (processing.py:99-105) after that of window (processing.py:139-146), for the filter-aware map's
 * F^T.  u = w y in float64, stored as float32; S^T u = u - e_0 sum_t (1 - t/(T-1)) u_t
 * - e_{T-1} sum_t t/(T-1) u_t, the two sums per row in float64 by a fixed tree (no atomics: bit-identical run to
 * run) and the two end samples rounded once.  Either part is optional.
 *  d_window [T] float64 window or NULL */
int mrx_tod_detrend_window_transpose(mrx_ctx* ctx, float* d_data, size_t ld, int D, int T, int remove_slope,
                                     const double* d_window);

/* The transpose of mrx_sosfilt, out = [S^T] H^T in: H^T = J H J with J the time reversal (H of
 * utils/signal/filters.py:46-69 is causal with zero initial state), then, with remove_slope, the adjoint S^T of the
 * slope removal mrx_sosfilt does first (processing.py:151).  mrx_sosfilt's arguments, scratch size, time-parallel scheme
 * (the chunks stay aligned from sample 0, each is walked backwards and they are chained from the last to the first
 * with the same chunk matrix) and refusals.  The two row sums of S^T are taken as <H a, in> and <H b, in>, a and b the
 * line's weights: float64 trees over the input, bit-identical run to run; H a and H b are filtered serially on the
 * host once per (cascade, T) and kept on the device by the context. */
int mrx_sosfilt_transpose(mrx_ctx* ctx, const double* sos, int n_sections, const double* d_chunk_matrix,
                          const float* d_in, size_t ld_in, int D, int T, int remove_slope, float* d_out,
                          size_t ld_out, double* d_work);

/* Test hook for the in-LDS inverse FFT both generators are built on: `rows` independent rows
 * of n << interleave_log2 complex float32 values, each holding 2^interleave_log2 interleaved
 * sequences of length n (a power of two >= 4; at most 8192 values per row); unnormalised
 * (numpy.fft.ifft(x) * n).  interleave_log2 = -1: the 64-point register transform, n = 64;
 * -2: the 4096-point workgroup transform (three radix-16 register passes), n = 4096;
 * -3: its 16 x RB x 16 form for n = 1024, 2048, 4096 (16 / RB rows per workgroup). */
int mrx_fft_rows(mrx_ctx* ctx, const float* d_in, int rows, int n, int interleave_log2,
                 float* d_out);

/* ---- detector noise ----------------------------------------- */

/* White + 1/f noise with spatially correlated modes: sim/noise.py:18-63 and
 * noise/generation.py:11-51,
 *   noise[d,t] = scale_d (sqrt(fs) w[d,t] + sqrt(c) sum_m B[d,m] M_m[t] + sqrt(1-c) p_d[t]),
 * w white N(0,1); p_d independent pink series with two-sided spectrum (knee/2)/|f| (equal
 * to the white level at f = knee); M_m = sqrt(fs) w'_m + P_m the modes (white + pink, the
 * generator applied to itself, generation.py:41-43); c = corr_prop.  The reference
 * filters white noise with a length-T FFT per detector; here all three parts of a detector
 * are synthesised in the frequency domain on a power-of-two period N >= T (one draw per cell
 * of variance fs/N + (1-c) knee/|k|; a four-step FFT whose real and imaginary parts serve two
 * detectors; the modes enter as tabulated Hermitian spectra) and cut to T samples (any T of
 * the N samples of white noise of period N are independent): same spectrum, different realisation and
 * period -- statistical parity, like the screens.  As in the reference, whose period is the
 * TOD itself, the pink and correlated parts carry no power below fs/T and have zero mean over
 * the T samples (the cells below ceil(N/T) are dropped, the window mean is subtracted).  With knee = 0 the
 * output is white only and neither the basis nor the work buffer is used.
 *  det_offset   global index of row 0 (even): the draws of detector det_offset + d depend on
 *               (seed, det_offset + d) only, the modes on the seed only -- shards of one
 *               band generated on different GPUs share their modes and nothing else
 *  d_basis [D][n_modes] spatial basis (utils/linalg.py:105-126, host), or NULL with n_modes 0
 *  d_scale [D]  1e12 * NEP per detector (noise.py:62), or NULL
 *  d_loading    [D][ld_loading] float32 total optical loading (pW) or NULL: the amplitude of
 *               sample (d,t) is d_scale[d] + per_loading * d_loading[d,t], per_loading =
 *               1e12 * NEP_per_loading (noise.py:35-37); must not alias an accumulating d_out
 *  d_out        [D][ld_out] float32, written (accumulate = 0) or added to (accumulate = 1:
 *               noise straight into an existing TOD)
 *  d_work       16-byte aligned scratch of work_floats floats; mrx_noise_work_floats(T,
 *               n_modes, batch) gives the size that holds `batch` detectors in flight
 *               (4 N + 8 bytes per detector + 8 N per mode).  From 256 detectors up the batches
 *               are spread over up to four streams (the context's stream forks and joins: the call
 *               is ordered on it like any other), each with an equal share of the buffer:
 *               1024 detectors in flight is a good size (MRX_OPT_NOISE_LANES).
 * mrx_noise_period: N = n1 * n2 for T samples (T <= 2^23). */
int mrx_noise_period(int T, int* n1, int* n2);
int mrx_noise_work_floats(int T, int n_modes, int batch, size_t* floats);
int mrx_noise_generate(mrx_ctx* ctx, uint64_t seed, int D, int det_offset, int T,
                       double sample_rate, double knee, double corr_prop,
                       const float* d_basis, int n_modes, const float* d_scale,
                       const float* d_loading, size_t ld_loading, double per_loading,
                       float* d_out, size_t ld_out, int accumulate,
                       float* d_work, size_t work_floats);
/* Two-rate form (chosen by the library: fs, knee and T decide).  Where the pink part at a quarter (half) of the
 * Nyquist frequency has fallen below 2 % of the white level -- 2 rate knee / fs <= 0.02: rate 4 at 400 Hz and a knee
 * of 1 Hz -- and T >= 32768, the pink and correlated-pink parts are synthesised at fs / rate (a period, a scratch
 * round trip and an arithmetic rate times smaller), interpolated with the four-point Catmull-Rom cubic, and the white
 * parts -- the detectors' own and the modes', which reach the Nyquist frequency -- are drawn per sample as the field is
 * written.  What changes against the one-rate form: no pink power between fs / (2 rate) and fs / 2 (< 2 % of the
 * spectrum there) and the interpolation's roll-off of the pink part in the octave below (smaller still); white level,
 * modes' covariance, zero pink mean over the TOD, shard / batch independence as before.  MRX_OPT_NOISE_GENERIC bit 8
 * keeps the one-rate form.
 *
 * mrx_noise_generate_krj: the field in K_RJ (tod/tod.py:106-142): every sample divided by den_band(d)(el(d, t)) as
 * mrx_tod_to_krj does (same elevation model, same lookup), with d_bore_el [T] and d_dx, d_dy, d_band [D] indexed like
 * the rows of d_out.  In the two-rate form the division rides on the writer's store (the field is written once);
 * otherwise the call is mrx_noise_generate followed by mrx_tod_to_krj. */
int mrx_noise_generate_krj(mrx_ctx* ctx, uint64_t seed, int D, int det_offset, int T,
                           double sample_rate, double knee, double corr_prop,
                           const float* d_basis, int n_modes, const float* d_scale,
                           const float* d_loading, size_t ld_loading, double per_loading,
                           float* d_out, size_t ld_out,
                           float* d_work, size_t work_floats,
                           const float* d_bore_el, const float* d_dx, const float* d_dy, const int32_t* d_band,
                           const float* d_cal_axis_el, const float* d_cal_values, int n_el, int n_bands);

/* Philox-4x32-10 standard normals, the generator behind the screens, exposed
 * so tests can check the stream against the published known-answer vectors.
 * counter = (i, 0, stream, 0), key = seed; d_out[i] for i < n. */
int mrx_philox_normal(mrx_ctx* ctx, uint64_t seed, uint32_t stream, size_t n,
                      float* d_out);
int mrx_philox_raw(mrx_ctx* ctx, uint64_t seed, uint32_t c0, uint32_t c1,
                   uint32_t c2, uint32_t c3, uint32_t host_out[4]);

#ifdef __cplusplus
}
#endif
#endif /* MRX_H_ */
