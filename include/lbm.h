/* lbm.h -- C ABI of liblbm_hip.so: MI355X-native D2Q9 lid-driven-cavity lattice-Boltzmann hot path.
 *
 * Drop-in boundary for the PyCUDA usage of the reference's GPU script.  Each entry point
 * cites the reference interface it replaces (paths relative to the reference repo root).
 * Plain C types only: no torch / C++ types cross this boundary.  Every function returning
 * int returns LBM_OK (0) or a negative lbm_status; the text is available from
 * lbm_last_error().  No C++ exception crosses the ABI.  One host thread per context.
 *
 * Host array convention (same as the reference scripts): fin[9][X][Y], u[2][X][Y],
 * rho[X][Y], C order, y fastest, y = 0 is the moving lid (MRT.py:192-209,
 * MRT_GPU.py:207-229).  On the device the library keeps one padded plane per direction,
 * x fastest (the transposition the reference does on the host at MRT_GPU.py:283-289 and
 * MRT_GPU.py:758-760 is done inside lbm_set_state / lbm_get_fields).
 */
#ifndef LBM_H
#define LBM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LBM_ABI_VERSION 4

typedef enum lbm_status {
    LBM_OK = 0,
    LBM_ERR_INVALID = -1, /* bad argument / unsupported combination */
    LBM_ERR_HIP = -2,     /* a HIP runtime call failed (text in lbm_last_error) */
    LBM_ERR_NOMEM = -3,
    LBM_ERR_STATE = -4,   /* call not valid in the current context state */
    LBM_ERR_COMM = -5     /* RCCL failure */
} lbm_status;

enum { LBM_F32 = 0, LBM_F64 = 1 };                      /* storage and arithmetic type */
enum { LBM_SRT = 0, LBM_TRT = 1, LBM_MRT = 2 };         /* RT = 'SRT' | 'TRT' | 'MRT'  (MRT_GPU.py:48) */
enum { LBM_SEM_MRT_PY = 0, LBM_SEM_MRT_GPU = 1,        /* streaming windows + wall rules of MRT.py:404-453
                                                           or of MRT_GPU.py:412,674-692 (wet-node walls) */
       LBM_SEM_BOUNCE_BACK = 2 };                       /* half-way bounce-back walls (link-based, the reference's "BB" option,
                                                           MRT_GPU.py:281): every lattice cell is a fluid cell, the walls sit half
                                                           a cell outside the lattice, the lid half a cell beyond global row 0.
                                                           The slot k of cell (x, y) pulls from (x - cx_k, y + cy_k); a source
                                                           outside the lattice gives the cell's own post-collision population of
                                                           the opposite direction instead, plus -- source row above the lid --
                                                           Ladd's moving-wall term 6 w_k rho_w (c_k . u_lid) = cx_k (rho_w uLB) / 6
                                                           (diagonals only), rho_w = the density of the cell's last macroscopic
                                                           state.  No macroscopic override on any cell.  Relaxation rates as
                                                           MRT_GPU (omega_eps = 1.2).  Not with turb = 1, arith = promoted,
                                                           kernel = PUSH / VEC or LBM_FLAG_STREAM_WALLS / STREAM_PAIRS. */
enum { LBM_SEM_BOUNCE_BACK_SOLID = 3 };                 /* LBM_SEM_BOUNCE_BACK plus a per-cell solid mask (lbm_set_solid below): a source that is
                                                           a solid cell inside the lattice bounces like a source outside it, with nothing
                                                           added.  Whole lattices only (no slabs), one step per launch: kernel = AUTO
                                                           (k_step_solid, 16 B per access; k_step_generic where nx is no multiple of the
                                                           vector width) or GENERIC.  LBM_FLAG_SOLID_TILES: 3 .. 5 steps per launch on the
                                                           tile kernel instead. */
enum { LBM_KERNEL_AUTO = 0,      /* fastest applicable: STREAM (large lattices), TB (lattices from 64 x 64 cells), else VEC, else GENERIC */
       LBM_KERNEL_GENERIC = 1,   /* one step per launch, one thread per cell (all semantics) */
       LBM_KERNEL_VEC = 2,       /* one step per launch, 16 B per access (MRT_GPU semantics) */
       LBM_KERNEL_TB = 3,        /* several (3 .. 5) time steps per launch: tiles through LDS + the wall frame */
       LBM_KERNEL_PUSH = 4,      /* the reference's own scheme for A/B: collide-and-push into a persistent second array, then a
                                    wall-rule + copy kernel (funRT + funBC, MRT_GPU.py:339-698); one whole lattice, no closure */
       LBM_KERNEL_STREAM = 5 };  /* up to 8 time steps per launch, streamed down column strips (rows held in registers, neighbour rows
                                    through LDS): what AUTO picks for large lone lattices; otherwise as TB */
enum { LBM_LAYOUT_AUTO = 0, LBM_LAYOUT_PLANES = 1, LBM_LAYOUT_ROWS = 2 }; /* device arrays: [k][y][x] or [y][k][x] */
enum { LBM_ARITH_STRICT = 0, LBM_ARITH_FAST = 1, LBM_ARITH_PROMOTED = 2 };
enum { LBM_SIDE_LOW = 0, LBM_SIDE_HIGH = 1 };           /* slab neighbour towards smaller / larger y */
/* lbm_params.flags: A/B switches of the launch plan (all off = the measured defaults); results never depend on them */
enum { LBM_FLAG_NO_DEEP_HALO = 1,        /* between slabs: a one-row exchange after every frame pass of a multi-step launch instead
                                            of ONE exchange of S complete rows per launch */
       LBM_FLAG_FRAME_UNFUSED = 2,       /* one launch per frame pass instead of all passes inside the tile launch */
       LBM_FLAG_FRAME_FUSED_BATCH = 4,   /* (r01: batches too run the frame passes inside the tile launch; the default since r02, accepted) */
       LBM_FLAG_NO_FRAME_LDS = 8,        /* intermediate frame passes through scratch lattices instead of LDS windows */
       LBM_FLAG_NT_ON = 16,              /* non-temporal loads / stores on (default: lattices above 192 MiB) ... */
       LBM_FLAG_NT_OFF = 32,             /* ... or off */
       LBM_FLAG_COMM_PRIORITY_OFF = 64,  /* communication stream at the compute stream's priority */
       LBM_FLAG_EAGER_LAG = 128,         /* every lbm_step() call ends with a single step (so that the lattice of the step before
                                            the last exists) instead of recomputing it when lbm_get_fields asks for u / rho */
       LBM_FLAG_FRAME_BESIDE_ON = 512,   /* kernel STREAM, lone lattice: the wall frame as a kernel of its own on the second stream, beside the */
       LBM_FLAG_FRAME_BESIDE_OFF = 1024, /* streaming workgroups, always / never (default: when the streaming kernel variant leaves registers free) */
       LBM_FLAG_FRAME_NARROW = 2048,     /* frame passes that go through the scratch lattices: workgroups of 256 threads instead of 1024 */
       LBM_FLAG_NO_EDGE_FIRST = 4096,    /* streaming kernel between slabs: do not hold the bulk launch back behind the edge launch */
       LBM_FLAG_NO_EDGE_RESERVE = 8192,  /* ... and do not plan a one-round bulk launch on fewer CUs to leave some to the edge workgroups */
       LBM_FLAG_NO_XCD_BANDS = 16384,    /* streaming kernel: workgroup i takes segment i (default: every XCD a contiguous run of segments) */
       LBM_FLAG_NO_TAIL_TILES = 32768,   /* streaming contexts with a wall frame: units of 3 .. 5 steps through the streaming kernel too (default:
                                            the tile kernel; with the walls inside the tails stay on the streaming kernel anyway) */
       LBM_FLAG_STREAM_WALLS = 65536,    /* kernel STREAM, MRT_GPU semantics, a lone lattice or a slab with the deep halo: the cells next to the walls */
       LBM_FLAG_NO_STREAM_WALLS = 262144,/* inside the streaming kernel (k_stream_walls / k_stream_walls_slab: no frame), always / never (default: for the
                                            operator variants whose kernel keeps its level loop free of scratch traffic -- MRT, SRT, no closure) */
       LBM_FLAG_STREAM_PAIRS = 131072,   /* ... the walls inside AND two rows per wave, twelve waves, at most 10 steps per launch (k_stream_pairs:
                                            an r03 experiment, no faster than k_stream_walls -- DESIGN 2.4; kept for A/B) */
       LBM_FLAG_SOLID_TILES = 524288 };  /* LBM_SEM_BOUNCE_BACK_SOLID only (refused elsewhere), kernel = AUTO or TB: the lattice with its solid cells
                                            steps 3 .. 5 steps per launch on the tile kernel, planned exactly as LBM_SEM_BOUNCE_BACK with kernel = TB
                                            plans the same lattice (steps per launch, frame, segments, units); tails and the first step after an
                                            upload stay on k_step_solid.  The same bits as one step per launch.  Needs nx % (16 / sizeof(real)) == 0
                                            and a size kernel = TB accepts; tb_steps 3 .. 5.  Opt-in: without it nothing changes */

/* The knobs of the reference script (MRT_GPU.py:38-93) as run-time parameters.  The
 * reference bakes them into the CUDA source by '%'-formatting (MRT_GPU.py:422,531,662) and
 * recompiles per parameter set; here the code object is compiled ahead of time for gfx950. */
typedef struct lbm_params {
    int32_t struct_size; /* = sizeof(lbm_params) */
    int32_t nx;          /* xsize */
    int32_t ny;          /* ysize of the WHOLE lattice */
    int32_t y0;          /* first global row owned by this context (0 when not slab-decomposed) */
    int32_t ny_local;    /* rows owned by this context (= ny when not slab-decomposed, >= 2) */
    int32_t dtype;       /* LBM_F32 | LBM_F64 */
    int32_t collision;   /* LBM_SRT | LBM_TRT | LBM_MRT */
    int32_t semantics;   /* LBM_SEM_MRT_PY | LBM_SEM_MRT_GPU | LBM_SEM_BOUNCE_BACK | LBM_SEM_BOUNCE_BACK_SOLID */
    int32_t kernel;      /* LBM_KERNEL_* */
    int32_t turb;        /* 0 | 1: Smagorinsky closure of MRT_GPU.py:368-387 (MRT_GPU semantics only) */
    int32_t device;      /* HIP device ordinal (reference: cuda.Device(0), MRT_GPU.py:29) */
    int32_t layout;      /* LBM_LAYOUT_* (device-side only; host arrays are unaffected) */
    int32_t batch;       /* 0 / 1: one lattice.  B > 1: B independent cavities of the same size and scheme advanced by
                            the same launches, each with its own relaxation rates -- the Reynolds sweep that
                            MRT_GPU_datagen.py:55-57,879-902 runs one lattice after the other.  Host arrays gain a
                            leading [B] axis.  Not combinable with slabs. */
    int32_t arith;       /* LBM_ARITH_STRICT (0, default): every operation in the reference's order, results bit-identical to
                            the CPU restatement in oracle/.  LBM_ARITH_FAST: the MRT operator in an algebraically identical
                            factored form with fused multiply-adds (about half the arithmetic); u = j * rcp(rho) and the
                            Smagorinsky closure's divisions / square root by the hardware's reciprocal / square-root
                            instructions (fp32: 1 ulp; fp64: refined by Newton steps).
                            Results agree with the strict form to rounding, not bit for bit.  MRT_GPU semantics only
                            (with LBM_SEM_MRT_PY the strict form is used).
                            LBM_ARITH_PROMOTED: the arithmetic of MRT_GPU.py's CUDA text -- the strict form, with the
                            sub-expressions that its double literals make double (equilibrium bracket, MRT m_eq sums,
                            Smagorinsky tau) evaluated in double and rounded to float once; fp32 results bit-identical to
                            the oracles' promote = True.  fp64: the same as STRICT.  MRT_GPU semantics only (rejected with
                            LBM_SEM_MRT_PY); not with LBM_FLAG_STREAM_PAIRS. */
    int32_t ny_local_min; /* slabs: the smallest ny_local of ALL ranks (0: = ny_local).  The launch plan (steps per launch, frame
                            width, deep halo) is derived from it, so that every rank of a decomposition runs the same exchange
                            protocol whatever its own share of the rows; lbm_comm_init() cross-checks the plan with both neighbours. */
    int32_t tb_steps;    /* 0: measured default.  2 .. 5 (STREAM: 2 .. 8; a lone MRT_GPU lattice, two rows per wave: 2 .. 10): time steps per launch of the multi-step path (A/B, tests) */
    int32_t frame_seg;   /* 0: default by lattice size.  >= 8: cells of the wall frame per workgroup of the fused frame passes */
    int32_t flags;       /* LBM_FLAG_* bits, 0 = defaults */
    double uLB;          /* lid velocity, MRT_GPU.py:57 */
    double omega;        /* = omegap = omega_nu, MRT_GPU.py:65 */
    double omegam;       /* TRT, MRT_GPU.py:80 */
    double omega_e;      /* MRT, MRT_GPU.py:89 */
    double omega_eps;    /* MRT, MRT_GPU.py:90 */
    double omega_q;      /* MRT, MRT_GPU.py:90 */
} lbm_params;

typedef struct lbm_ctx lbm_ctx;

/* --- library ----------------------------------------------------------------------- */
int lbm_abi_version(void);
/* replaces: pycuda.autoinit device discovery (MRT_GPU.py:23-30) */
int lbm_device_count(void);

/* --- context ----------------------------------------------------------------------- */
/* replaces: import pycuda.autoinit + cuda.mem_alloc x8 + SourceModule/get_function
 * (MRT_GPU.py:23-30,309-316,701-703).  Returns NULL on failure with the reason in err. */
lbm_ctx* lbm_create(const lbm_params* p, char* err, size_t errlen);
/* replaces: PyCUDA garbage-collected DeviceAllocation / context teardown at exit */
void lbm_destroy(lbm_ctx* c);
const char* lbm_last_error(const lbm_ctx* c);

/* --- state in ---------------------------------------------------------------------- */
/* replaces: fin = equ(rho=1, InitVel) on the host + memcpy_htod (MRT_GPU.py:262-267,323-328);
 * computed on the device. */
int lbm_init_equilibrium(lbm_ctx* c);
/* replaces: per-plane transpose + cuda.memcpy_htod(fin_g, fin) (MRT_GPU.py:283-289,323).
 * fin_host is the WHOLE-lattice array fin[9][nx][ny]; the context reads its own rows
 * y0 .. y0+ny_local-1.  host_dtype is LBM_F32 or LBM_F64 (converted if it differs).
 * With batch = B > 1: fin[B][9][nx][ny]. */
int lbm_set_state(lbm_ctx* c, const void* fin_host, int host_dtype);

/* replaces: the per-Reynolds-number recompilation of the kernel source (MRT_GPU_datagen.py:57,63-93 -> 701-703):
 * sets the relaxation rates of lattice `index` of the batch (0 for a single lattice) for all later steps. */
int lbm_set_relaxation(lbm_ctx* c, int index, double omega, double omegam, double omega_e, double omega_eps,
                       double omega_q);

/* --- time loop --------------------------------------------------------------------- */
/* replaces: funRT(...); funBC(...) launched from the Python loop (MRT_GPU.py:707-732).
 * Enqueues nsteps fused steps and returns without waiting (errors surface at the next
 * synchronising call, like pycuda LaunchError).  Large lattices advance several steps per launch
 * (lbm_next_unit).  With an RCCL communicator attached the halo exchange with the slab neighbours is
 * part of every launch unit.  A slab (y0 > 0 or y0 + ny_local < ny) WITHOUT a communicator is refused
 * (LBM_ERR_STATE): its ghost rows would never be filled -- use the externally driven calls below. */
int lbm_step(lbm_ctx* c, int nsteps);
/* replaces: the implicit synchronisation of cuda.memcpy_dtoh (MRT_GPU.py:755) */
int lbm_sync(lbm_ctx* c);
/* replaces: the commented cuda.Event timing (MRTTiledPull.py:364-365,536-549): runs nsteps
 * steps between two HIP events on the compute stream and returns the elapsed milliseconds (automatic samples of the time
 * statistics, of a monitor series and of the residual included, lbm_stats_begin / lbm_monitor_begin / lbm_residual_begin) */
int lbm_time_steps(lbm_ctx* c, int nsteps, double* ms);
/* iterations performed since the last lbm_init_equilibrium / lbm_set_state */
long long lbm_steps_done(const lbm_ctx* c);
/* The launch plan of lbm_step(): number of time steps the next launch unit advances when `steps_left` remain
 * (1 = a single step; S > 1 = one multi-step launch of S steps).  Depends only on the parameters, ny_local_min and
 * whether the lattice has just been uploaded -- the same on every rank of a decomposition. */
int lbm_next_unit(const lbm_ctx* c, int steps_left);

/* The launch plan as text (for logs and for bench.py's roofline line): one line of `key=value` pairs -- kernel of the multi-step
 * units (k_stream | k_stepS_deep | k_step2_deep | none), steps per launch, frame width, workgroups and strip rows of a launch, ...
 * Returns the length written (truncated to len - 1), negative on a bad argument. */
int lbm_describe(const lbm_ctx* c, char* buf, size_t len);
/* Dry run, NO device needed: the text lbm_describe() would give for lbm_create(p), followed by ` units=S1,S2,...` -- the launch units
 * lbm_step(steps) would run from a freshly initialised lattice.  Derived from lbm_params alone, so a launcher can check, before any
 * rank touches a GPU, that all ranks of a decomposition plan the same kernel / steps per launch / frame / deep halo and the same
 * units (lbm_comm_init cross-checks the same items at run time).  ncu: compute units to plan for (0 = 256).  Invalid parameters:
 * returns a negative status and writes `error: <reason>`.  (No counterpart in the reference, which runs one GPU.) */
int lbm_plan(const lbm_params* p, int ncu, int steps, char* buf, size_t len);

/* --- state out --------------------------------------------------------------------- */
/* replaces: cuda.memcpy_dtoh(fin, ftemp_g); memcpy_dtoh(rho, rho_g); memcpy_dtoh(u, u_g)
 * + transposes (MRT_GPU.py:755-760).  Synchronises.  u_host[2][nx][ny], rho_host[nx][ny]
 * receive the macroscopic fields computed in the LAST iteration (one-step lag of the
 * reference: u_g/rho_g are written inside funRT before collide/stream); fin_host
 * [9][nx][ny] receives the current populations (post stream + wall rules).  Any pointer
 * may be NULL.  Whole-lattice arrays; only this context's rows are written.
 * With batch = B > 1: u_host[B][2][nx][ny], rho_host[B][nx][ny], fin_host[B][9][nx][ny].
 * (When the last launch unit advanced S > 1 steps, the lattice of the step before the last is recomputed here from the
 * unit's source lattice, S - 1 steps, bit-identically; nothing of that is on the path of lbm_step.) */
int lbm_get_fields(lbm_ctx* c, void* u_host, void* rho_host, void* fin_host, int host_dtype);
/* replaces: the download of u_g + np.mean(u) of the convergence test (MRT_GPU.py:883, MRT_GPU_datagen.py:862-871) by a
 * reduction on the device: mean_out[b] = mean over both components and all cells of this context's rows of the u that
 * lbm_get_fields would return, accumulated in double in a fixed order (deterministic); one double per lattice of the batch
 * crosses PCIe.  (The reference's criterion is defined on NumPy's float32 pairwise mean of the downloaded field; the two
 * means differ in the last bits of a float -- the host form stays available through lbm_get_fields.) */
int lbm_mean_u(lbm_ctx* c, double* mean_out);
/* replaces: taus_g (MRT_GPU.py:387; never downloaded by the reference, its dashboard prints mean(tauS), MRT_GPU.py:862-866).
 * tau_host[nx][ny] receives the relaxation time tau + tau_turbulent of the LAST iteration; with turb = 0 the constant
 * 1 / omega.  With batch = B > 1: tau_host[B][nx][ny]. */
int lbm_get_tau(lbm_ctx* c, void* tau_host, int host_dtype);

/* --- the samplers: what the time statistics, the run monitor and the field residual share ------------------------------- */
/* A SAMPLE at step count n is exactly the u[2][X][Y] and rho[X][Y] that lbm_get_fields would return right after n steps (the same
 * lagged lattice, gather + macros, wall overrides), whatever the kernel route, dtype, operator, arithmetic, closure, semantics, batch
 * or slab.  lbm_<sampler>_sample takes the sample of the fields lbm_get_fields would return now; it returns LBM_ERR_STATE before the
 * first step and while the sampler is off.
 *
 * THE SCHEDULE.  lbm_<sampler>_begin(..., every, ...) records n0 = lbm_steps_done().  every > 0: lbm_step (and lbm_time_steps, whose
 * time then includes the samples) samples by itself at step counts n0 + every, n0 + 2 every, ...; after any lbm_step call exactly the
 * samples with n <= lbm_steps_done() have been taken.  The sample of n is taken from the lattice after n - 1 steps, so the launch
 * units are cut where one starts at n - 1: an `every` below the steps per launch (8 on the streaming path) shortens the units --
 * correct, but slower.  Every sampler keeps its own schedule; the units are cut at the earliest next sample of the three, and
 * samplers due at the same step count read the same lattice, the statistics first, then the monitor, then the residual.
 * lbm_step_unit and the split-step calls refuse to run (LBM_ERR_STATE) while any sampler samples automatically.  every = 0: manual
 * sampling only.  On a slab every > 0 is LBM_ERR_STATE (the cuts would split the launch units, and ranks that began differently would
 * post different exchanges): slabs call lbm_<sampler>_sample at the same step counts on every rank and the host combines the results.
 * Calling _begin again restarts the sampler.  lbm_<sampler>_end stops it and frees what _begin allocated; lbm_init_equilibrium,
 * lbm_set_state and lbm_destroy end every sampler too, and none is part of a checkpoint.
 * The force on the bodies of a solid mask (lbm_force_*, below) is a fourth sampler on this schedule, enqueued last, with its own
 * instant: its sample of step count n is defined on the lattice after n steps, not n - 1, so a launch unit is cut to END at n and the
 * sample follows that unit, also where the unit is the last of an lbm_step call.
 *
 * A SERIES (monitor, residual, force).  _begin allocates room for `capacity` samples, capacity x batch records on the device (there, never
 * inside lbm_step).  A sample writes the next free slot; nothing returns to the host before lbm_<sampler>_read.  With the buffer full a
 * sample leaves no record and is counted in `dropped`; stepping is unaffected.  _read synchronises; *count = records held, *dropped =
 * samples that left none; records_out[min(count, max_records)][batch] receives the oldest records (may be NULL with max_records = 0).
 * The series goes on.  _read returns LBM_ERR_STATE while no series is on.
 *
 * THE TREE (monitor, residual, topology).  Sums, extrema and their cells are reduced without atomics in a fixed order: a lane folds
 * its cells in grid-stride order, the 64 lanes of a wave combine by shuffles (offsets 32, 16, ..., 1), the waves of a workgroup in
 * index order, then the workgroups' partial results in index order.  Results are therefore identical from run to run, between manual
 * and automatic samples, and between a one-shot call and a series.  An extremum's cell is chosen by an explicit total order (value,
 * x, y), never by "first seen".
 * A NULL context is LBM_ERR_INVALID everywhere. */

/* --- time statistics ------------------------------------------------------------------- */
/* No reference counterpart: the time-mean velocity and density and the Reynolds stresses over a window of iterations, accumulated
 * on the device (the LES run of MRT_GPU.py:46-49 needs them), from the samples defined above.  The device keeps six double sums per cell, S_u, S_v, S_rho, S_uu, S_vv, S_uv: every sample value converted to double,
 * every product rounded in double and then added (no FMA contraction), samples added in sample order (one thread per cell, no
 * atomics).  The read-out S / count is one IEEE double division, so the results are bit-identical to the host loop
 *     step(k); u, rho = get_fields(); acc += u.astype(f64); acc2 += u64 * u64; ...; acc / count.
 *
 * lbm_stats_begin: allocates the sums on the first call (48 B per cell and lattice; never inside lbm_step), zeroes them and starts the
 *   schedule (above); after any lbm_step call the count covers exactly the samples with n <= lbm_steps_done().
 * lbm_stats_sample: adds what lbm_get_fields returns now.
 * lbm_stats_get: means over the samples, float64, whole-lattice host arrays mean_u[2][X][Y], mean_rho[X][Y], second[3][X][Y] (E[uu],
 *   E[vv], E[uv]); with batch = B a leading [B].  Only the context's own rows are written; any pointer may be NULL.  With
 *   count == 0 only *count is written.
 * lbm_stats_end: stops sampling and frees the sums.
 * lbm_stats_sample / _get return LBM_ERR_STATE while statistics are off. */
int lbm_stats_begin(lbm_ctx* c, int every);
int lbm_stats_sample(lbm_ctx* c);
int lbm_stats_get(lbm_ctx* c, double* mean_u, double* mean_rho, double* second, long long* count);
int lbm_stats_end(lbm_ctx* c);

/* --- run monitor ------------------------------------------------------------------------- */
/* replaces: what an output iteration of MRT_GPU.py:752-889 computes from the downloaded u and rho -- the two NaN-masked arg-mins of
 * |u|^2 (vortex search, MRT_GPU.py:764-778), np.mean(u), the middle column and row -- by ONE pass over the lattice on the device that
 * leaves a small record per lattice; no field crosses PCIe.  The SAMPLE is the one defined above, of lbm_get_fields(host_dtype): every
 * value is first rounded to host_dtype, as lbm_get_fields does, then converted to double; everything below is computed in double without contraction.  Per cell
 *     q = (ux * ux + uy * uy) / (uLB * uLB)         (each product rounded, then the sum, then one IEEE division by the double uLB * uLB)
 * which is the `usq` of the reference's search operation for operation.
 *
 * lbm_monitor_spec: host_dtype (LBM_F32 | LBM_F64); the search window [x_lo, x_hi) x [y_lo, y_hi), y in GLOBAL rows; nboxes <= 4
 *   exclusion boxes box[i] = {x_lo, x_hi, y_lo, y_hi} in the same form; nprobes <= 8 probe cells probe[i] = {x, global y}.  Window and
 *   boxes need 0 <= lo <= hi <= nx (ny); a probe must be a cell of the lattice.  Anything else is LBM_ERR_INVALID.
 * lbm_monitor_record (all doubles, one per lattice of the batch):
 *   step       the step count whose fields it describes
 *   nonfinite  own cells where any of ux, uy, rho is not finite; those cells are left out of everything else but the probes
 *   sum_ux, sum_uy, sum_rho, sum_q   sums over the context's own finite cells, walls included
 *   max_q      the maximum of q over the same cells (-inf when there is none)
 *   min_q, min_x, min_y   the minimum of q over the finite cells inside the window and outside every box, with its cell (global y);
 *              ties go to the smaller x, then the smaller y -- the first hit of np.nanargmin on the [X][Y] host array.  No candidate:
 *              min_q = +inf, min_x = min_y = -1
 *   probe[i]   ux, uy, rho at probe cell i; NaN for unused probes and for probes outside this context's rows
 * Reduced by the tree described above.
 *
 * lbm_monitor: one record per lattice of the fields lbm_get_fields would return now (records_out[batch]); synchronises.
 *   LBM_ERR_STATE before the first step.
 * lbm_monitor_begin / _sample / _read / _end: a series of these records with the schedule above; a sample that finds the buffer
 *   full is not taken.  spec == NULL, every < 0 or capacity < 1: LBM_ERR_INVALID.
 * lbm_get_lines: the column x and the global row gy of the fields lbm_get_fields(host_dtype) would return, the same bits:
 *   col_out[B][3][NY] receives ux, uy, rho of column x (own rows only), row_out[B][3][nx] those of row gy (written only if this
 *   context owns that row).  Either pointer may be NULL (its index is then ignored).  Synchronises. */
enum { LBM_MONITOR_MAX_BOXES = 4, LBM_MONITOR_MAX_PROBES = 8 };
typedef struct lbm_monitor_spec {
    int32_t struct_size;  /* = sizeof(lbm_monitor_spec) */
    int32_t host_dtype;
    int32_t x_lo;
    int32_t x_hi;
    int32_t y_lo;
    int32_t y_hi;
    int32_t nboxes;
    int32_t nprobes;
    int32_t box[4][4];
    int32_t probe[8][2];
} lbm_monitor_spec;
typedef struct lbm_monitor_record {
    double step;
    double nonfinite;
    double sum_ux;
    double sum_uy;
    double sum_rho;
    double sum_q;
    double max_q;
    double min_q;
    double min_x;
    double min_y;
    double probe[8][3];
} lbm_monitor_record;
int lbm_monitor(lbm_ctx* c, const lbm_monitor_spec* spec, lbm_monitor_record* records_out);
int lbm_monitor_begin(lbm_ctx* c, const lbm_monitor_spec* spec, int every, int capacity);
int lbm_monitor_sample(lbm_ctx* c);
int lbm_monitor_read(lbm_ctx* c, lbm_monitor_record* records_out, int max_records, long long* count, long long* dropped);
int lbm_monitor_end(lbm_ctx* c);
int lbm_get_lines(lbm_ctx* c, int x, int gy, void* col_out, void* row_out, int host_dtype);

/* --- field residual ------------------------------------------------------------------------ */
/* No reference counterpart (the reference's stop rule watches np.mean(u), MRT_GPU.py:883-889): the change of the sampled u and rho
 * between two consecutive samples, reduced on the device to one small record per lattice -- the field residual of a steady run.  The
 * previous sample stays on the device as a snapshot; no field crosses PCIe.  The SAMPLE is the monitor's: the one defined above, of
 * lbm_get_fields(host_dtype), every value first rounded to host_dtype, then converted to double; everything below is computed in double without contraction.
 *
 * The snapshot holds ux, uy, rho of the previous sample for every own cell; after a sample it holds the current sample's values,
 * bit-preserving, for cells that are not finite too.  (Only the values are specified; the library stores them in the type
 * lbm_get_fields(host_dtype) hands out, 12 or 24 B per cell and lattice.)
 * Per cell, with pux, puy, prho the snapshot's values:
 *     dux = ux - pux;  duy = uy - puy;  d2 = dux * dux + duy * duy        (each product rounded, then the sum)
 *     u2 = ux * ux + uy * uy
 *     dr = rho - prho;  dr2 = dr * dr
 * A cell takes part only if all six values ux, uy, rho, pux, puy, prho are finite.
 * lbm_residual_record (all doubles, one per lattice of the batch):
 *   step, step_prev   the step counts of the two samples
 *   cells             own cells that take part
 *   nonfinite         own cells that do not
 *   sum_du2, sum_u2, sum_drho2   sums of d2, u2, dr2 over the cells that take part
 *   max_du2, max_x, max_y   the maximum of d2 over the same cells with its cell (global y); ties go to the smaller x, then the smaller y
 *                     (an explicit order on (d2, x, y), as the monitor's minimum) -- the first hit of np.argmax on the [X][Y] host array
 *   max_drho2         the maximum of dr2
 *   No cell takes part: max_du2 = max_drho2 = -inf, max_x = max_y = -1.
 * Reduced by the tree described above.
 *
 * lbm_residual_begin / _sample / _read / _end: a series of these records with the schedule above; _begin also allocates the snapshot
 *   and the partial results.  The FIRST sample after _begin only fills the snapshot; every later sample appends one record and then
 *   replaces the snapshot; a sample that finds the buffer full still refreshes the snapshot.  host_dtype other than LBM_F32 / LBM_F64,
 *   every < 0 or capacity < 1: LBM_ERR_INVALID. */
typedef struct lbm_residual_record {
    double step;
    double step_prev;
    double cells;
    double nonfinite;
    double sum_du2;
    double sum_u2;
    double sum_drho2;
    double max_du2;
    double max_x;
    double max_y;
    double max_drho2;
} lbm_residual_record;
int lbm_residual_begin(lbm_ctx* c, int host_dtype, int every, int capacity);
int lbm_residual_sample(lbm_ctx* c);
int lbm_residual_read(lbm_ctx* c, lbm_residual_record* records_out, int max_records, long long* count, long long* dropped);
int lbm_residual_end(lbm_ctx* c);

/* --- flow topology: stream function, vorticity, vortex extrema ------------------------------- */
/* replaces: the streamline panel of an output iteration (MRT_GPU.py:808-817) and the comparison with the vortex table of Ghia, Ghia &
 * Shin, for which the reference downloads u: the stream function psi and the vorticity omega of the sampled fields, and the extrema
 * of psi inside up to eight windows, computed on the device; the record path moves no field across PCIe.  The SAMPLE is the monitor's:
 * exactly the u[2][X][Y] that lbm_get_fields(host_dtype) would return now (same lagged lattice, gather + macros, wall overrides, whatever
 * the kernel route), every value rounded to host_dtype, then converted to double.  Everything below is computed in double without
 * contraction and is defined operation for operation, so the device equals the NumPy restatement (topology.host_topology,
 * topology.host_stream_function) bit for bit.
 *
 * The index y runs away from the lid and u[1] > 0 points towards the lid (slot k pulls from y + cy_k), so (x, Y = -y) with (ux, uy) is a
 * right-handed frame.
 * Stream function, ux = d psi / dY, uy = -d psi / dx, integrated along x from the left wall, row by row (a row never needs another row):
 *     t[0][y] = 0;  t[x][y] = 0.5 * (uy[x - 1][y] + uy[x][y])  for x >= 1
 *   summed in a fixed two-level order: blocks of LBM_TOPOLOGY_BLOCK = 64 cells of x (the last may be shorter); inside a block within[x] is
 *   the running sum of t taken strictly left to right, starting AS the block's first term; across blocks off[0] = 0,
 *   off[b + 1] = off[b] + (the last within of block b), strictly in order;
 *     psi[x][y] = -(off[block of x] + within[x]).
 *   In NumPy:  for b in range(0, X, 64): c = np.cumsum(t[b:b+64], axis=0); psi[b:b+64] = -(off + c); off = off + c[-1]
 * Vorticity, omega = d uy / dx - d ux / dY = dvdx + dudy (one addition):
 *     dvdx[x] = 0.5 * (uy[x + 1] - uy[x - 1]) inside, uy[1] - uy[0] at x = 0, uy[X - 1] - uy[X - 2] at x = X - 1; dudy the same along the
 *   index y with ux.  omega is counter-clockwise positive; Ghia's table lists -omega.
 * Extrema of psi in a window [x_lo, x_hi) x [y_lo, y_hi): the minimum and the maximum over the cells whose psi is finite, each with its
 *   cell and the omega of that cell (the same bits as the omega field).  Ties go to the smaller x, then the smaller y, for the minimum
 *   and the maximum alike (an explicit order on (psi, x, y), as the monitor's minimum).  No candidate: psi = +inf (minimum) / -inf
 *   (maximum), cell (-1, -1), omega = NaN.
 * closure: the maximum of |psi[X - 1][y]| over the rows where it is finite (-inf if there is none) -- the net flux each row fails to
 *   close.  A quality figure: the wet-node walls do not conserve mass, so it is not zero, and an extremum whose |psi| is not well above
 *   it (the secondary corner eddies on a coarse lattice) is not resolved by this psi.
 *
 * lbm_topology_spec: struct_size, host_dtype (LBM_F32 | LBM_F64), nwindows <= LBM_TOPOLOGY_MAX_WINDOWS, window[i] = {x_lo, x_hi, y_lo,
 *   y_hi} with 0 <= lo <= hi <= nx (ny); anything else is LBM_ERR_INVALID.  The windows are common to the lattices of a batch.
 * lbm_topology_record (all doubles, one per lattice of the batch): step, closure, window[i].min / .max = {psi, x, y, omega}; windows
 *   beyond nwindows: psi = omega = NaN, cell (-1, -1).
 * lbm_topology: records_out[batch] of the fields lbm_get_fields would return now; synchronises.  LBM_ERR_STATE before the first step.
 * lbm_get_stream_function: the fields whose extrema those are, float64, host layout: psi_out[B][X][Y], omega_out[B][X][Y]; either may be
 *   NULL.  Synchronises; LBM_ERR_STATE before the first step.
 * Both return LBM_ERR_STATE on a slab: omega needs rows of the neighbour, and a table over slabs needs a combining step on the host;
 *   psi itself is row-local, which keeps that later step small.
 * Device memory is allocated at the first call (never inside lbm_step) and freed by lbm_destroy: the record path takes X * Y / 64 doubles
 *   of block sums plus one partial result per workgroup; the field path stages two double fields. */
enum { LBM_TOPOLOGY_MAX_WINDOWS = 8, LBM_TOPOLOGY_BLOCK = 64 };
typedef struct lbm_topology_spec {
    int32_t struct_size;  /* = sizeof(lbm_topology_spec) */
    int32_t host_dtype;
    int32_t nwindows;
    int32_t reserved;     /* 0 */
    int32_t window[8][4];
} lbm_topology_spec;
typedef struct lbm_topology_extremum {
    double psi;
    double x;
    double y;
    double omega;
} lbm_topology_extremum;
typedef struct lbm_topology_record {
    double step;
    double closure;
    struct {
        lbm_topology_extremum min;
        lbm_topology_extremum max;
    } window[8];
} lbm_topology_record;
int lbm_topology(lbm_ctx* c, const lbm_topology_spec* spec, lbm_topology_record* records_out);
int lbm_get_stream_function(lbm_ctx* c, double* psi_out, double* omega_out, int host_dtype);

/* --- solid obstacles and the force on them ---------------------------------------------------- */
/* No reference counterpart (the reference runs the empty box): solid cells inside the bounce-back cavity, LBM_SEM_BOUNCE_BACK_SOLID.
 * The mask is mask[X][Y] uint8, host layout (y fastest, y = 0 the lid); with batch = B mask[B][X][Y], every lattice its own.  Nonzero
 * means solid.  Any mask with at least one fluid cell per lattice is valid: solid cells may touch the walls, the lid and each other,
 * and may enclose fluid.
 *
 * Fluid cell, slot k = 1 .. 8, source (x - cx_k, y + cy_k):
 *   source outside the lattice        exactly the LBM_SEM_BOUNCE_BACK rule, lid term included;
 *   source inside and solid           the cell's own post-collision population of the opposite direction, nothing added (obstacles
 *                                     are at rest, until lbm_set_body_motion below gives their surfaces a velocity);
 *   otherwise                         the source's post-collision population of direction k.
 *   Moments, collision, rates, the first step after an upload and the parked lid density are those of LBM_SEM_BOUNCE_BACK.
 * Solid cell: never updated.  Its populations are the constants w_k (4/9, 1/9, 1/36) rounded to the lattice type -- the rest
 *   equilibrium at rho = 1 -- in both lattices, and a gather on it returns them.  Every export and every sampler therefore sees
 *   fin_k = w_k, u = exactly 0 and rho = the sum of the nine w_k in the order of the moments there; nothing is NaN, and the stream
 *   function integrates uy = 0 through a body.
 *
 * lbm_set_solid: LBM_ERR_STATE on a context of another semantics; LBM_ERR_INVALID for a mask that leaves a lattice no fluid cell.
 *   Ends every sampler, stores the mask, derives the link plane (one more plane of both lattices; per cell bit k - 1: the source of
 *   slot k is a solid cell inside the lattice, bit 8: the cell is solid) and performs lbm_init_equilibrium; solid cells then hold w_k.
 *   A later lbm_set_state ignores the host values of solid cells and writes w_k there.  A fresh context has the all-fluid mask.
 * lbm_get_solid: mask_out[B][X][Y] receives 0 / 1.
 * lbm_solid_force: the momentum-exchange force of the fluid on all solid cells of each lattice, out[batch], all doubles:
 *   step    the step count
 *   links   the (fluid cell, slot k) pairs whose source is a solid cell inside the lattice
 *   fx, fy  sum over the links of 2 c_opp(k) f, f = the fluid cell's post-collision population of direction opp(k) as the lattice holds it
 *           after the last step, converted to double first.  Components as u: fy > 0 points to the lid.  f equals what lbm_get_fields
 *           returns as fin_k of that cell, so the host restatement is F = sum_links 2 c_opp(k) fin_k(x, y).
 *   Reduced by the tree described with the samplers: a lane folds its cells in grid-stride order (slots k = 1 .. 8 in order), no
 *   atomics, the same bits from run to run.  Synchronises.  LBM_ERR_STATE before the first step.  The partial results are allocated
 *   at the first call (never inside lbm_step) and freed by lbm_destroy. */
typedef struct lbm_solid_force_record {
    double step;
    double links;
    double fx;
    double fy;
} lbm_solid_force_record;
int lbm_set_solid(lbm_ctx* c, const uint8_t* mask);
int lbm_get_solid(lbm_ctx* c, uint8_t* mask_out);
int lbm_solid_force(lbm_ctx* c, lbm_solid_force_record* out);

/* --- the bodies of a mask: force and torque on each, one-shot and as a series ------------------ */
/* No reference counterpart.  The solid cells of a lattice are split into nbodies bodies by a label per cell, and every LINK -- a (fluid
 * cell (x, y), slot k) pair whose source (x - cx_k, y + cy_k) is a solid cell -- belongs to the body of its source cell.  Two bodies
 * that touch share no link: a link's own cell is fluid.
 *
 * lbm_set_solid_bodies: body[B][X][Y] int32, the host layout of the mask; on every solid cell a value in [0, nbodies), ignored on
 *   fluid cells; 1 <= nbodies <= 256.  centre[B][nbodies][2] = (x0, y0) of each body in index coordinates; NULL takes each body's
 *   centroid, the mean of its cells' indices in double.  A body without cells gets the centre (0, 0) and has no links.
 *   LBM_ERR_STATE on a context of another semantics; LBM_ERR_INVALID for a label out of range on a solid cell, a centre that is not
 *   finite or another bad argument.  Touches neither the lattice nor the step count; ends a running force series and nothing else.
 *   From the mask and the labels it derives one link list per lattice, sorted by body, then by cell in [y][x] order, then by k, and
 *   uploads it (there and in lbm_set_solid, never inside lbm_step), so that a sample costs O(links), not a pass over the lattice.
 *   lbm_set_solid resets to the default, which is also a fresh context's: one body that holds every solid cell, centred at its centroid.
 * lbm_get_solid_bodies: body_out[B][X][Y] receives the labels (-1 on fluid cells), centre_out[B][nbodies][2] the centres; either may
 *   be NULL.  lbm_solid_body_count: nbodies (0 for a NULL context or one of another semantics).
 * lbm_body_force: out[B][nbodies], all doubles:
 *   step    the step count
 *   body    the body's label
 *   links   the links of the body
 *   fx, fy  sum over them of tx = 2 cx_opp(k) f and ty = 2 cy_opp(k) f, f exactly the population lbm_solid_force uses
 *   tz      sum over them of rx ty + ry tx, (rx, ry) = (x - cx_k / 2 - x0, y + cy_k / 2 - y0) the link's midpoint relative to the
 *           body's centre.  The index y grows AWAY from the lid while fy > 0 points TO the lid, so this is the z-moment in the frame
 *           drawn with the lid on top (X = x, Y = -y): X Fy - Y Fx, positive counter-clockwise.
 *   Every term is formed in double without contraction, each product rounded, then rx ty + ry tx, then the sum.  Reduced per body by
 *   THE TREE, without atomics: the body's range of the list is cut into chunks of 2048 links, a workgroup folds one chunk (lane t its
 *   links t, t + 256, ...), and one wave per body folds the chunks' results in order.  The bits depend on the list and the lattice
 *   alone: they are the same from run to run, in this call and in a series, for a lattice alone and as a member of a batch, and on
 *   either kernel route.  A body without links has links = fx = fy = tz = 0.  Synchronises.  LBM_ERR_STATE before the first step and
 *   on a context of another semantics, as lbm_solid_force, whose records and bits are unchanged.
 * lbm_force_begin / _sample / _read / _end: A SERIES of these records on THE SCHEDULE, a sample being batch x nbodies records.  With
 *   n0 = lbm_steps_done() at _begin and every > 0 the records carry step = n0 + every, n0 + 2 every, ..., each bit for bit what
 *   lbm_body_force returns when called at that step count; after any lbm_step call exactly the samples with n <= lbm_steps_done()
 *   have been taken.  With LBM_FLAG_SOLID_TILES a multi-step unit ends at every sample.  _begin: LBM_ERR_INVALID for every < 0 or
 *   capacity < 1, LBM_ERR_STATE before the first step.  lbm_force_sample records the force of the lattice as it is now.  The series
 *   ends on lbm_force_end, lbm_set_solid_bodies, lbm_set_solid, lbm_init_equilibrium, lbm_set_state and lbm_destroy. */
typedef struct lbm_body_force_record {
    double step;
    double body;
    double links;
    double fx;
    double fy;
    double tz;
} lbm_body_force_record;
int lbm_set_solid_bodies(lbm_ctx* c, const int32_t* body, int nbodies, const double* centre);
int lbm_get_solid_bodies(lbm_ctx* c, int32_t* body_out, double* centre_out);
int lbm_solid_body_count(lbm_ctx* c);
int lbm_body_force(lbm_ctx* c, lbm_body_force_record* out);
int lbm_force_begin(lbm_ctx* c, int every, int capacity);
int lbm_force_sample(lbm_ctx* c);
int lbm_force_read(lbm_ctx* c, lbm_body_force_record* records_out, int max_records, long long* count, long long* dropped);
int lbm_force_end(lbm_ctx* c);

/* --- moving bodies: a wall velocity on the surface of each body ----------------------------------- */
/* No reference counterpart.  A body keeps its cells and its SURFACE moves: every link of body b carries Ladd's moving-wall term, the term
 * the lid has, for the body's motion (Ux, Uy, Om) -- Ux, Uy in the components of u (Uy > 0 points to the lid), Om in radians per step,
 * counter-clockwise positive in the frame drawn with the lid on top, the frame of tz.  Exact for a circular body that rotates; for a
 * translating body the usual fixed-shape approximation, good for small displacements.  Bodies never change the cells they occupy.
 *
 * With tz's midpoint (rx, ry) = (x - cx_k / 2 - x0, y + cy_k / 2 - y0) of the link (cell (x, y), slot k) relative to the body's centre:
 *     uwx = Ux + Om ry;  uwy = Uy + Om rx;  delta = (6 w_k) (cx_k uwx + cy_k uwy)
 *   formed on the host in double without contraction, every product and sum rounded in the order written, 6 w_k = 2/3 (k <= 4) or 1/6
 *   rounded once to double; rho_0 = 1 stands for the density, so delta is a constant of the link.  The result is rounded once to the
 *   lattice type.
 * Step: a cell stores fpost_opp(k) + delta in slot opp(k) where it stored fpost_opp(k), one add in the lattice type.  Only the cell's own
 *   bounce reads that slot, so every gather, export and sampler is unchanged: lbm_get_fields returns the arriving population as fin_k(x, y),
 *   and a lbm_set_state of that fin is an exact restart.  The first step after an upload stores with delta like every other step; a
 *   motion set after n steps first shows in the store of step n + 1.
 * Force: on a link f_in = f, the population the lattice holds, and f_out = f - delta, so lbm_solid_force, lbm_body_force and the force
 *   series sum (tx, ty) = c_opp(k) (2 f - delta), delta the rounded value converted to double -- with delta = 0 the bits of
 *   2 c_opp(k) f; midpoint, order of operations and tree as described above.
 * Mass: in exact arithmetic the sum of delta over the links of a lattice is zero whenever no two touching bodies move differently and no
 *   moving body pumps through the lattice's edge.  The call forms S = sum delta and A = sum |delta| per lattice, in double over the sorted
 *   link list, and refuses a motion with |S| > links * 2^-52 * A: a belt on a wall (tangential motion) and a rotating ring that touches the
 *   perimeter pass, a block on a wall with a wall-normal velocity does not.
 *
 * lbm_set_body_motion: motion[B][nbodies][3] = (Ux, Uy, Om) of every body; NULL means all zero.  LBM_ERR_STATE on a context of another
 *   semantics, and for a nonzero motion on a LBM_FLAG_SOLID_TILES context (the tile kernel keeps obstacles at rest); LBM_ERR_INVALID for a
 *   value that is not finite and for a motion the flux check refuses (the text names the net flux).  Touches neither the lattice nor the
 *   step count and ends no sampler.  Builds the table of the deltas on the host and uploads it (there, never inside lbm_step).  An
 *   all-zero motion frees the table: the context then launches the kernels of obstacles at rest and gives their bits.  lbm_set_solid and
 *   lbm_set_solid_bodies reset every body to rest.  lbm_describe appends ` wall_motion=1` while a nonzero motion is set.
 * lbm_get_body_motion: motion_out[B][nbodies][3] receives the motion as set (all zero at rest). */
int lbm_set_body_motion(lbm_ctx* c, const double* motion);
int lbm_get_body_motion(lbm_ctx* c, double* motion_out);

/* --- curved obstacle surfaces: a wall distance per link, interpolated bounce-back ------------------- */
/* No reference counterpart.  Without a shape every wall sits half-way along its link, so a round body is a staircase and force, torque
 * and motion are first order in the lattice spacing.  With a shape every link carries q, the fraction of the link from the fluid cell
 * (x, y) to the wall, towards the source (x - cx_k, y + cy_k), and bounces by Bouzidi, Firdaouss and Lallemand's linear interpolation,
 * second order.  Opt-in: a context that never sets a shape launches the kernels it always did and gives their bits.  A shaped lattice does
 * NOT conserve its mass (the interpolation weights two populations): it trades mass conservation for accuracy.
 *
 * Per link (cell P = (x, y), slot k, body b), on the host in double without contraction, every operation rounded in the order written:
 *     near = q < 1/2 and N = (x + cx_k, y - cy_k) is a fluid cell inside the lattice; a link with q < 1/2 whose N is no such cell (a
 *       fluid cell between two bodies, or against a wall) falls back to the effective q = 1/2
 *     a = near ? 2 q : 1 / (2 q)
 *     (rx, ry) = ((x - q cx_k) - x0, (y + q cy_k) - y0)      the wall point; at q = 1/2 the bits of the midpoint of lbm_body_force
 *     delta = (6 w_k) (cx_k uwx + cy_k uwy), uwx = Ux + Om ry, uwy = Uy + Om rx      as lbm_set_body_motion forms it, at the wall point
 *     d = near ? delta : a delta
 *   a and d are rounded once to the lattice type.  The flux check of lbm_set_body_motion is unchanged: it is formed from the deltas of
 *   the same motion at q = 1/2.
 * The rule, on the read side -- the same in the step kernels and in every gather, in the lattice type, no contraction:
 *     own = fpost_opp(k)(P);   other = near ? fpost_opp(k)(N) : fpost_k(P)
 *     a == 1:     g_k = own + d                                       (a select, not a multiply by zero)
 *     otherwise:  t1 = a own;  b = 1 - a;  t2 = b other;  g_k = (t1 + t2) + d
 *   Sources outside the lattice and the lid term are applied afterwards as without a shape.
 * Stores of a shaped context are the pure post-collision values: there is no store-side add, and the raw first step after an upload
 * applies nothing.  lbm_get_fields returns the arriving populations with the rule applied, and lbm_set_state of that fin is an exact
 * restart.  THE DIFFERENCE from a context without a shape, which adds a motion's term where it stores: here a motion set after n steps
 * shows in the populations arriving for step n + 1, and in every export and sampler from that moment.
 * Force (lbm_solid_force, lbm_body_force, the force series): per link f_out = fpost_opp(k)(P) as the lattice holds it, f_in = g_k, both
 *   converted to double, (tx, ty) = c_opp(k) (f_out + f_in), tz = rx ty + ry tx with the wall point above; tree, order and chunks as
 *   without a shape; lbm_solid_force equals the bodies' sum.
 *
 * lbm_set_solid_shape: q[B][8][X][Y] doubles in the host layout of the mask, plane k - 1 for slot k.  On every link 0 < q <= 1 and
 *   finite, else LBM_ERR_INVALID (the text names the first offending link: lattices in order, cells in [y][x] order, then k); values
 *   off the links are ignored.  NULL clears the shape: the context returns to the half-way rule and its kernels.  LBM_ERR_STATE on a
 *   context of another semantics, on a LBM_FLAG_SOLID_TILES context (the tile kernel keeps the half-way rule), and -- for setting and
 *   for clearing -- while a nonzero body motion is set: a context without a shape keeps the motion's term on the store side, a shaped one
 *   on the read side, and switching under a stored term would corrupt one step.  The order is the shape first, then the motion.
 *   Touches neither the lattice nor the step count and ends no sampler.  Builds the tables on the host and uploads them (there and in
 *   lbm_set_solid_bodies / lbm_set_body_motion, never inside lbm_step).  lbm_set_solid resets the shape; lbm_set_solid_bodies keeps q and
 *   rebuilds what depends on labels and centres.  lbm_describe appends ` wall_shape=1` while a shape is set.
 * lbm_get_solid_shape: q_out[B][8][X][Y] receives the effective q on the links (after the fallback) and 0 elsewhere; all 0 without a
 *   shape. */
int lbm_set_solid_shape(lbm_ctx* c, const double* q);
int lbm_get_solid_shape(lbm_ctx* c, double* q_out);

/* --- open boundaries: held outlet cells and a wall velocity per solid cell -------------------------- */
/* No reference counterpart.  The two pieces that turn the closed cavity into a stream or a channel (LBM_SEM_BOUNCE_BACK_SOLID only): cells
 * that keep prescribed populations -- a pressure or far-field outlet, a reservoir -- and a wall velocity on single solid cells -- a velocity
 * bounce-back inlet with any profile.  Bodies, force series, shapes, samplers, topology and checkpoints work on such a lattice unchanged.
 *
 * Hold cells.  A hold cell is never updated: it holds f_k, rounded once to the lattice type, in both lattices, the way a solid cell holds
 *   w_k.  It is NOT a wall: a neighbour pulls f_k from it by the plain pull.  In plane K_LINK the hold cell's own word is exactly 512 (bit
 *   9, no link bits: it reads no wall table), and no neighbour's word has a bit for it.  A gather on it returns the nine stored values, so
 *   every export and sampler sees fin_k = the held value and u, rho its moments.  For the `near` test of a shape a hold cell is no fluid
 *   cell (the effective q = 1/2 applies), and no link of the force lists starts at one.
 * lbm_set_open_cells: hold[B][X][Y] in the layout of the mask, nonzero = hold cell, NULL (or all zero) clears; f[B][9][X][Y] doubles, read
 *   on hold cells only.  Ends every sampler, stores the cells, rewrites plane K_LINK and performs lbm_init_equilibrium, as lbm_set_solid
 *   does; after every initialisation and lbm_set_state the hold cells are written again from the context's table (host values there are
 *   ignored).  LBM_ERR_INVALID: a hold cell that is solid, a value on a hold cell that is not finite or is negative, a lattice left without
 *   a fluid cell, hold without f.  LBM_ERR_STATE: another semantics; a LBM_FLAG_SOLID_TILES context (the tile kernel never sees bit 9);
 *   a shape, a nonzero motion or a nonzero wall velocity is set -- geometry comes first.  lbm_set_solid clears the hold cells;
 *   lbm_set_solid_bodies keeps them.  lbm_describe appends ` open_cells=1` while there are any.
 * lbm_get_open_cells: hold_out[B][X][Y] receives 0 / 1, f_out[B][9][X][Y] the values as given on the hold cells and 0 elsewhere; either
 *   may be NULL.
 *
 * Wall velocity per solid cell.  uw[B][2][X][Y], components as u, read on solid cells only.  For a link with the fluid cell P, slot k and
 *   the source solid cell S = (x - cx_k, y + cy_k) the delta of lbm_set_body_motion becomes
 *       delta = delta_body + (6 w_k) (cx_k uwx(S) + cy_k uwy(S))
 *   in double without contraction: the rigid-body term first, formed exactly as above (at the wall point under a shape); then the cell
 *   term, each product and sum rounded in the order written; then the add.  From there everything is what a motion does: the store-side
 *   add, `d = near ? delta : a delta` of a shape's table, (2 f - delta) in the forces.  One table holds both; each of the two calls
 *   rebuilds it from both, in either order.
 * Flux check: a lattice with at least one hold cell is open and the check of lbm_set_body_motion is waived for it; a lattice without one
 *   is checked as before, with the cell terms inside S and A.
 * lbm_set_wall_velocity: NULL means all zero.  The rules of lbm_set_body_motion: LBM_ERR_STATE on another semantics and, nonzero, on a
 *   LBM_FLAG_SOLID_TILES context; LBM_ERR_INVALID for a value on a solid cell that is not finite and for a refused flux; the shape first,
 *   then velocities (lbm_set_solid_shape refuses while one is set); touches neither the lattice nor the step count and ends no sampler.
 *   An all-zero motion with an all-zero velocity frees the table: the context launches the kernels of obstacles at rest.  lbm_set_solid
 *   resets it; lbm_set_solid_bodies keeps it and rebuilds the table for the new labels and centres (and may therefore refuse a flux).
 *   lbm_describe appends ` wall_velocity=1` while a nonzero velocity is set.
 * lbm_get_wall_velocity: uw_out[B][2][X][Y] receives the velocity as set on solid cells and 0 elsewhere. */
int lbm_set_open_cells(lbm_ctx* c, const uint8_t* hold, const double* f);
int lbm_get_open_cells(lbm_ctx* c, uint8_t* hold_out, double* f_out);
int lbm_set_wall_velocity(lbm_ctx* c, const double* uw);
int lbm_get_wall_velocity(lbm_ctx* c, double* uw_out);

/* --- periodic sides and a uniform driving force ---------------------------------------------------- */
/* No reference counterpart.  What force-driven and periodic flows need (LBM_SEM_BOUNCE_BACK_SOLID only): Poiseuille flow without an inlet,
 * a periodic array of obstacles, periodic Couette flow, Taylor-Green decay.  Each works without the other: a closed box under gravity is
 * legal, and so is a periodic lattice without a force.
 *
 * Image cells.  With px, columns 0 and nx - 1 are image columns of the columns nx - 2 and 1, and the periodic domain is columns
 *   1 .. nx - 2; with py the same holds for rows 0 and ny - 1; with both the four corners are images of the diagonally opposite real cells.
 *   The partner of an image cell, x -> nx - 2 if x == 0, 1 if x == nx - 1 (likewise y), is always a real cell.  An image cell whose partner
 *   is not solid is a hold cell (its word in plane K_LINK is exactly 512): never updated, pulled from by the plain pull, no force link
 *   starts at it, no fluid cell for the `near` test of a shape.  An image cell whose partner is solid must be solid.  After every single
 *   step, and behind the constants of the solid and hold cells after every initialisation and lbm_set_state (there on both lattices), the
 *   kernel k_wrap copies the nine slots of every partner into its image, on the compute stream.  The lattice holds post-collision
 *   populations, so the image's neighbours pull exactly what they would pull across the seam.
 * lbm_set_periodic: geometry -- it ends every sampler, rewrites plane K_LINK and the bodies' tables and performs lbm_init_equilibrium, as
 *   lbm_set_open_cells does.  LBM_ERR_INVALID (the text names the first offending cell, index x * ny + y): the mask differs from its own
 *   wrap on an image cell; the body labels differ from their own wrap (lbm_set_solid_bodies checks the same when called later); a user
 *   hold cell on an image cell (lbm_set_open_cells refuses it likewise); nx < 4 with px, ny < 4 with py; a lattice left without a fluid
 *   cell.  LBM_ERR_STATE: another semantics; a LBM_FLAG_SOLID_TILES context; a shape, a nonzero motion or a nonzero wall velocity is set --
 *   geometry comes first.  lbm_set_solid clears the periodic sides; lbm_set_open_cells and lbm_set_solid_bodies keep them.
 *   lbm_set_periodic(c, 0, 0) restores the closed box, its kernels and its bits.  lbm_describe appends ` periodic=x`, ` periodic=y` or
 *   ` periodic=xy` while a side is periodic.
 *   Limits.  The exported arrays include the image cells, and the device samplers (statistics, monitor, residual, topology) count them as
 *   cells.  lbm_get_open_cells reports the user's hold cells only.  The torque of a body that crosses the seam is meaningless; its force is
 *   right: every physical link is counted once, from its real fluid cell.  The flux check of a motion is waived, as on every lattice with
 *   hold cells.  Under a shape a near link whose next fluid cell is an image falls back to q = 1/2: keep shaped bodies two cells from the
 *   seam.  Wall velocities and wall distances on image solids are the caller's to wrap.  One step per launch, no slabs.
 * lbm_get_periodic: *px_out, *py_out receive 0 / 1; either may be NULL.
 *
 * Driving force.  (fx, fy) is the force density per cell, in the components of u.  On the host, in double without contraction and in this
 *   order, F_k = (3 w_k) (cx_k fx + cy_k fy) for k = 1 .. 8, 3 w_k = 1/3 (k <= 4) or 1/12, each rounded once to the lattice type.  Every
 *   collision of a cell that is neither solid nor held is followed by f*_k = f*_k + F_k, one add in the lattice type, never fused (arith =
 *   fast too), in the raw first step too, before the delta of a moving wall.  The scheme is the first-order one: the equilibrium uses the
 *   bare velocity, the physical velocity is (sum c f + F / 2) / rho, and the exports and samplers keep reporting the bare moments.  It is
 *   exact for a steady uniform driver; the one force that varies in space and time is lbm_set_buoyancy's, by this same scheme.  All lattices
 *   of a batch share one force.
 * lbm_set_driving_force: may be called at any time; it touches neither the lattice nor the step count and ends no sampler.
 *   LBM_ERR_INVALID: a value that is not finite.  LBM_ERR_STATE, for a nonzero force: another semantics, a LBM_FLAG_SOLID_TILES context.
 *   (0, 0) restores the launches and the bits of a context without a force.  lbm_describe appends ` driving_force=1` while it is nonzero.
 * lbm_get_driving_force: *fx_out, *fy_out receive the force as set; either may be NULL. */
int lbm_set_periodic(lbm_ctx* c, int px, int py);
int lbm_get_periodic(lbm_ctx* c, int* px_out, int* py_out);
int lbm_set_driving_force(lbm_ctx* c, double fx, double fy);
int lbm_get_driving_force(lbm_ctx* c, double* fx_out, double* fy_out);

/* --- a passive scalar on an obstacle lattice: temperature or dye ------------------------------------ */
/* No reference counterpart.  An advected, diffusing scalar C carried by the flow of a LBM_SEM_BOUNCE_BACK_SOLID context (a lone lattice,
 * one step per launch, batch = 1): a second set of nine populations g_k on the flow's own D2Q9 stencil, weights and (x, y) conventions, in
 * two ping-pong lattices of the flow's layout that hold post-collision populations and are pulled from, as the flow's are.  The scalar has
 * no link plane: it reads the flow's.  It never acts on the flow unless lbm_set_buoyancy: the flow's bits with a
 * scalar are those without.
 *
 * One scalar step of a cell that is neither solid nor held, every operation in the lattice type, none fused, in the order written:
 *   gather   g_k = g*_k(x - cx_k, y + cy_k).  A source outside the lattice: g_k = g*_opp(k) of the cell itself (the box edges and the lid
 *            are adiabatic; the lid adds nothing).  A source that is a solid cell (bit k - 1 of the cell's link word): adiabatic,
 *            g_k = g*_opp(k); Dirichlet with the value Cw (anti-bounce-back), g_k = t - g*_opp(k), t = 2 w_k Cw formed in double and rounded
 *            once to the lattice type (one table row per fluid cell with a Dirichlet link, built on the host).
 *   moments  C = (((((((g_0 + g_1) + g_2) + g_3) + g_4) + g_5) + g_6) + g_7) + g_8.  (ux, uy): the moments of the flow lattice that the
 *            flow step of the same lbm_step iteration has just written, image cells wrapped -- the bits lbm_get_fields exports, in the
 *            lattice type, after the NEXT step (under a shape, through the shaped gather).  A driving force's half-force shift is NOT
 *            added: the scalar is advected by the bare moment.
 *   collide  TRT on the pairs (a, b) = (1, 3), (2, 4), (5, 7), (6, 8), cu = c_a.u:  g*_0 = g_0 - w+ (g_0 - w_0 C);
 *            gp = (g_a + g_b) / 2;  gm = (g_a - g_b) / 2;  e = w_a C;  dp = w+ (gp - e);  dm = w- (gm - (3 e) cu);
 *            g*_a = (g_a - dp) - dm;  g*_b = (g_b - dp) + dm.
 *            In double on the host: tm = 3 D + 1/2, w- = 1 / tm, w+ = 1 / (magic / (tm - 1/2) + 1/2), each rounded once to the lattice
 *            type.  magic is the TRT product (1/w+ - 1/2)(1/w- - 1/2), 1/4 by convention; BGK is magic = (3 D)^2.
 *   There is one arithmetic: under a flow with arith = fast the scalar kernel is the same code fed other velocities.
 * Solid cells store zeros.  A hold cell of the flow is a hold cell of the scalar: a user's hold cell (lbm_set_open_cells) keeps
 *   g_k = (w_k Ch) (1 + 3 (cx_k ux + cy_k uy)), formed in double in this order and rounded once, (ux, uy) the moments of the flow
 *   populations it holds (as given, in double), Ch its hold value, or its initial value where hold_value is NULL; an image cell of a
 *   periodic side is refreshed from its partner after every scalar step by the k_wrap launch on the scalar lattice.
 * The first scalar step after lbm_scalar_begin or lbm_scalar_set_state is raw, as the flow's: the lattice holds plain populations, which
 *   are collided without streaming.  Inside lbm_step (and lbm_step_finish) every flow step and its wrap are followed by the scalar step
 *   and its wrap, on the compute stream.
 * Limits.  Wall velocities, body motions and shapes do not enter the scalar's wall rule, which stays half-way (the velocity it is
 *   advected by is the one every export sees).  The scheme is not positivity-preserving.  A held outlet holds a value; there is no
 *   convective or zero-gradient outlet.  Nothing feeds back on the flow but lbm_set_buoyancy (below).
 *
 * lbm_scalar_begin: arrays [X][Y] in the host layout of lbm_set_solid's mask.  c0: the initial values (read on cells that are not
 *   solid); the lattice starts from the plain populations w_k C0, weight and C0 rounded to the lattice type.  dirichlet (NULL: none):
 *   nonzero marks a solid cell that holds wall_value there; every other solid cell is adiabatic.  hold_value (NULL: the initial values):
 *   read on the user's hold cells.  Replaces a scalar that is active.  LBM_ERR_STATE with a reason: another semantics, a slab, batch > 1, a
 *   LBM_FLAG_SOLID_TILES context.  LBM_ERR_INVALID with a reason: D or magic not finite or <= 0; c0 NULL or not finite on a cell that is
 *   not solid; a Dirichlet flag on a cell that is not solid; a Dirichlet cell without a finite wall value; a hold value that is not
 *   finite.  lbm_describe appends ` scalar=D,magic` while a scalar is active.
 * Whatever ends the samplers and restarts the lattice because the geometry changed -- lbm_set_solid, lbm_set_open_cells,
 *   lbm_set_periodic -- ends the scalar.  lbm_set_state and lbm_init_equilibrium keep it and leave its populations alone;
 *   lbm_set_solid_bodies, motions, shapes and the driving force keep it too.
 * lbm_scalar_end: ends the scalar and frees its lattices and tables; LBM_OK without one.  The flow's launches, bits and describe text are
 *   then those of a context that never had one.
 * lbm_scalar_active: 1 and the parameters (either pointer may be NULL) while a scalar is active, 0 otherwise.
 * lbm_scalar_get: g_out[9][X][Y] receives the arriving populations of the current state (what the next scalar step gathers: zeros on solid
 *   cells, the held values on hold cells); conc_out[X][Y] receives C of the state the last scalar step started from -- the one-step lag
 *   of lbm_get_fields, so that C and u of one call belong to the same iteration; before the first step, of the state as set.  Either may be
 *   NULL.
 * lbm_scalar_get_stored: g_out[9][X][Y] receives the post-collision populations as the lattice holds them (what lbm_scalar_flux reads).
 * lbm_scalar_set_state: plain populations g[9][X][Y]; values on solid and hold cells are ignored; the next scalar step is raw.  The
 *   populations of lbm_scalar_get continue a run bit for bit (with lbm_set_state of the flow's).
 * lbm_scalar_totals: over the cells that are neither solid nor image cells of a periodic side, of C as lbm_scalar_get returns it,
 *   converted to double: their count, the sum, the minimum and the maximum, by the fixed tree of the samplers.  step: scalar steps since
 *   lbm_scalar_begin or lbm_scalar_set_state.
 * lbm_scalar_flux: out[nbodies] (lbm_solid_body_count), one record per body over the links of the list lbm_body_force walks:
 *   flux = sum of (double)g_k - (double)g*_opp(k), g_k what the next gather returns for the link -- the scalar that enters the fluid from
 *   the body per step; an exact zero on adiabatic links.  LBM_ERR_STATE before the first scalar step. */
typedef struct lbm_scalar_record {
    double step, cells, sum, min, max;
} lbm_scalar_record;
typedef struct lbm_scalar_flux_record {
    double step, links, flux;
} lbm_scalar_flux_record;
int lbm_scalar_begin(lbm_ctx* c, double diffusivity, double magic, const double* c0, const uint8_t* dirichlet, const double* wall_value,
                     const double* hold_value);
int lbm_scalar_end(lbm_ctx* c);
int lbm_scalar_active(const lbm_ctx* c, double* diffusivity_out, double* magic_out);
int lbm_scalar_get(lbm_ctx* c, void* conc_out, void* g_out, int host_dtype);
int lbm_scalar_get_stored(lbm_ctx* c, void* g_out, int host_dtype);
int lbm_scalar_set_state(lbm_ctx* c, const void* g_host, int host_dtype);
int lbm_scalar_totals(lbm_ctx* c, lbm_scalar_record* out);
int lbm_scalar_flux(lbm_ctx* c, lbm_scalar_flux_record* out);

/* --- Boussinesq buoyancy: the scalar acts on the flow ------------------------------------------------ */
/* No reference counterpart.  With buoyancy (ax, ay, c_ref) set, (ax, ay) is the acceleration per unit of C in the components of u (hot
 * fluid that rises toward the lid row y = 0 is ay > 0).  On the host, in double without contraction, B_k = (3 w_k) (cx_k ax + cy_k ay) for
 * k = 1 .. 8 -- the arithmetic of the driving force's F_k; each B_k and c_ref are rounded once to the lattice type.  Every collision of a
 * cell that is neither solid nor held is followed by
 *     t = Cp - c_ref;   d_k = F_k + B_k t;   f*_k = f*_k + d_k     (k = 1 .. 8)
 * every operation in the lattice type, none fused (arith = fast too); F_k are the constants of lbm_set_driving_force, zeros without one.
 * The one add to f*_k sits where the driving force's sits: in the raw first step too, before the delta of a moving wall, before the solid
 * and the hold cells are pinned.  The density does not enter (rho0 = 1).
 * Cp is the buoyancy plane, one value per cell in the lattice type, owned by the scalar: the C that the most recent scalar step summed;
 * after lbm_set_buoyancy, lbm_scalar_begin and lbm_scalar_set_state, C of the state as it is -- at every moment what lbm_scalar_get's
 * conc_out returns.  Inside lbm_step the order stays flow step, wrap, scalar step, wrap: flow step n + 1 reads the C that scalar step n
 * summed, scalar step n the velocity of the lattice flow step n wrote.  The coupling is sequential and explicit.
 * With buoyancy set the flow's bits are no longer those of a context without a scalar.
 * Limits.  The first-order forcing of the driving force: the equilibrium uses the bare velocity, the physical velocity is
 *   (sum c f + a (C - c_ref) / 2) / rho, the scalar is advected by the bare moment and every export and sampler reports the bare moment.
 *   No shaped lattice, no LBM_FLAG_SOLID_TILES, no slab, no batch.  One flow launch and one scalar launch per step.
 * lbm_set_buoyancy: needs an active scalar (else LBM_ERR_STATE with a reason); allocates and fills the plane; touches neither lattice nor
 *   the step counts and ends no sampler; may be called again at any time with other values.  (ax, ay) = (0, 0) frees the plane and restores
 *   the launches, the bits and the lbm_describe text of a context without it.  LBM_ERR_INVALID: a value that is not finite.  LBM_ERR_STATE
 *   with a reason: a shape is set; a LBM_FLAG_SOLID_TILES context.  While it is set lbm_set_solid_shape is refused with a reason, and
 *   lbm_describe appends ` buoyancy=1`.  Everything that ends the scalar ends the buoyancy first: lbm_scalar_end, lbm_set_solid,
 *   lbm_set_open_cells, lbm_set_periodic.  Motions, wall velocities, bodies, the driving force and a lbm_scalar_begin that replaces the
 *   scalar keep it.
 * lbm_get_buoyancy: returns 1 while it is set, else 0 (the values are then zeros); any pointer may be NULL.
 * lbm_set_buoyancy_plane: conc[X][Y] (the host layout, as lbm_scalar_get's conc_out) replaces the plane, each value rounded once to the
 *   lattice type.  What a restart needs on top of the two states: after lbm_set_state and lbm_scalar_set_state the plane holds C of the
 *   scalar state as set, while the run that wrote the states would next read the C of one scalar step earlier -- lbm_scalar_get's conc_out
 *   at that moment; with it uploaded here the run continues bit for bit.  LBM_ERR_STATE without buoyancy. */
int lbm_set_buoyancy(lbm_ctx* c, double ax, double ay, double c_ref);
int lbm_set_buoyancy_plane(lbm_ctx* c, const void* conc_host, int host_dtype);
int lbm_get_buoyancy(lbm_ctx* c, double* ax_out, double* ay_out, double* c_ref_out);

/* --- sub-grid viscosity of an obstacle lattice ------------------------------------------------------- */
/* No reference counterpart (the reference's closure, turb = 1, stays what it is and stays refused on these lattices).  The local
 * Smagorinsky closure of Hou et al. (1996) on a LBM_SEM_BOUNCE_BACK_SOLID context at one step per launch; the mask may be empty, which is
 * the plain bounce-back cavity.  After the gather a cell that is neither solid nor held has populations f_k and the moments rho, ux, uy
 * that its collision takes; with S.. the plain sums of c c f_k in the order of k,
 *     Pxx = Sxx - (rho / 3 + (rho ux) ux)   Pyy = Syy - (rho / 3 + (rho uy) uy)   Pxy = Sxy - (rho ux) uy
 *     N   = sqrt((Pxx Pxx + 2 (Pxy Pxy)) + Pyy Pyy)
 *     tau = 0.5 (tau0 + sqrt(tau0 tau0 + (k N) / rho)),   tau0 = 1 / omega of the lattice,   k = 18 sqrt(2) cs2
 * every operation in the lattice type in the order written (k is formed in double and rounded once); arith = fast takes its reciprocal
 * and square-root instructions for the two divisions and the two square roots.  1 / tau enters the collision of that step where the
 * lattice's viscous rate would: SRT's omega, TRT's omega+, MRT's omega_nu.  The eddy viscosity is nu_t = cs2 |S|, |S| = sqrt(2 S:S).
 * There is no history and no plane: the layout is untouched, the driving force and the wall terms are added after the collision as
 * before.  Each lattice of a batch has its own tau0; all share cs2.
 * Limits.  No wall damping (Van Driest).  A passive scalar keeps its molecular diffusivity; with buoyancy the closure is refused (an eddy
 *   diffusivity would be needed).  No LBM_FLAG_SOLID_TILES, no slab.
 * lbm_set_subgrid: may be called at any time; it touches neither the lattice nor the step count and ends no sampler.  cs2 = 0 clears it
 *   and restores the launches, the bits and the lbm_describe text of a context without it; cs2 > 0 appends ` subgrid=<cs2>` to that
 *   text.  LBM_ERR_INVALID: cs2 negative or not finite.  LBM_ERR_STATE with a reason, for cs2 > 0: another semantics, a
 *   LBM_FLAG_SOLID_TILES context, buoyancy is set.  While cs2 > 0 lbm_set_buoyancy is refused with a reason.
 * lbm_get_subgrid: cs2 as set, 0 without it.
 * lbm_get_tau on such a context: the tau of the step that starts from the current state, gathered through the view of the exported
 *   fields under the context's wall rule; a solid cell and a hold cell (lbm_set_open_cells, the image cells of lbm_set_periodic), which no
 *   step updates, report tau0. */
int lbm_set_subgrid(lbm_ctx* c, double cs2);
int lbm_get_subgrid(lbm_ctx* c, double* cs2_out);

/* --- per-cell relaxation rates of an obstacle lattice: a viscosity field ------------------------------ */
/* No reference counterpart.  On a LBM_SEM_BOUNCE_BACK_SOLID context at one step per launch every cell that is neither solid nor held takes
 * its own rates into the collision, the same operations on a value per cell; nothing else of the step changes: the driving force and the
 * wall terms are added after the collision as before, and the raw first step after lbm_set_state uses the field too.
 *   omega[B][nx][ny], indexed like tau_host of lbm_get_tau (B = 1 for a single lattice): the viscous rate of each cell -- SRT's omega,
 *     TRT's omega+, MRT's omega_nu; nu = (1 / omega - 1/2) / 3 in lattice units.  MRT's other rates (omega_e, omega_eps, omega_q) stay the
 *     lattice's.
 *   omegam, the same shape, or NULL: TRT's omega- of each cell.  NULL: every cell keeps the lattice's omegam.  A two-layer Poiseuille flow
 *     is exact only with the magic parameter (1/omega+ - 1/2)(1/omega- - 1/2) kept per cell; with a uniform omega- it is second order.
 * Each value is rounded once to the lattice type on the host and kept in one read-only plane per rate and lattice on the device.
 * lbm_set_relaxation_field: may be called at any time; it touches neither the lattice nor the step count and ends no sampler, and it
 *   survives lbm_set_solid, lbm_set_relaxation and the other setters (a later lbm_set_relaxation changes the rates of solid and hold cells'
 *   reports and MRT's other rates only).  omega = NULL (omegam NULL too) clears the field and restores the launches, the bits and the
 *   lbm_describe text of a context without it; while a field is set that text gains ` relax_field` (` relax_field+m` with omegam).
 *   LBM_ERR_INVALID: a value that is not finite or not in (0, 2) -- the message names the first offending cell; values at solid and hold
 *   cells are checked the same way but never used.  LBM_ERR_STATE with a reason: another semantics (which covers slabs: an obstacle
 *   lattice is whole), a LBM_FLAG_SOLID_TILES context, buoyancy is set, omegam on a context whose collision is not TRT.  While a field is
 *   set lbm_set_buoyancy is refused with a reason (the pairing would be one more set of kernel twins).  A passive scalar keeps its own
 *   diffusivity.
 * With lbm_set_subgrid(cs2 > 0): tau0 of the closure is 1 / omega of the cell, one division in the lattice type; omega- stays the cell's.
 * lbm_get_relaxation_field: 1 and the planes as the device holds them (rounded to the lattice type; omegam_out untouched without an
 *   omega- plane; either pointer may be NULL) if a field is set, 0 if not.
 * lbm_get_tau on such a context: a cell that is neither solid nor held reports the tau of the step that starts from the current state --
 *   1 / omega of the cell in the lattice type, or the closure's value on that tau0; solid and hold cells report the lattice's tau0. */
int lbm_set_relaxation_field(lbm_ctx* c, const double* omega, const double* omegam);
int lbm_get_relaxation_field(lbm_ctx* c, double* omega_out, double* omegam_out);

/* --- shear-dependent viscosity of an obstacle lattice: a rheology table -------------------------------- */
/* No reference counterpart.  A generalised Newtonian fluid: the viscosity of a cell is a function nu(gdot) of its own shear rate.  On a
 * LBM_SEM_BOUNCE_BACK_SOLID context at one step per launch every cell that is neither solid nor held takes, once per step, from its gathered
 * populations f and the moments rho, ux, uy its collision takes anyway,
 *     jx = rho ux                      jy = rho uy
 *     a  = ((f1 + f3) - (f2 + f4)) - (jx ux - jy uy)          (= Pxx - Pyy of the non-equilibrium momentum flux)
 *     b  = (((f5 - f6) + f7) - f8) - jx uy                    (= Pxy)
 *     N  = sqrt(0.5 (a a) + 2 (b b))                          (the Frobenius norm of its deviatoric part)
 *     g  = N / rho
 *     s  = g * inv_dg                  inv_dg = (n - 1) / g_max, formed in double, rounded once to the lattice type
 *     sc = fmax(fmin(s, n - 1), 0)     (C fmin / fmax: a NaN s gives n - 1)
 *     i  = min((int) sc, n - 2)        fr = sc - i
 *     w_nu = t[i] + fr * d[i]          and, with omegam,  w_m = tm[i] + fr * dm[i]
 * every operation in the lattice type, one rounding each, in the order written, none fused (arith = fast: its own square root and division,
 * and a fused interpolation).  w_nu enters the collision as SRT's omega, TRT's omega+, MRT's omega_nu; w_m as TRT's omega-.  Nothing else of
 * the step changes: the driving force and the wall terms are added after the collision as before, solid and hold cells are pinned, and the
 * raw first step after lbm_set_state uses the table too.  i lies in [0, n - 2] for every state of the lattice, a blown-up one included;
 * beyond g_max the table holds its last entry.
 * Why a table in g: with tau = 1/2 + 3 nu the shear rate is gdot = (3 / sqrt 2) g / tau, which needs the tau that nu(gdot) yields.  The
 * caller solves that once -- g = (sqrt 2 / 3) gdot (1/2 + 3 nu(gdot)) increases strictly wherever the stress nu gdot does not fall -- and
 * tabulates omega = 1 / tau over g; the device needs g alone, no history, no plane and no store.
 *   omega[n]: omega at g_i = i g_max / (n - 1), each value rounded once to the lattice type on the host; the slopes d[i] = t[i + 1] - t[i]
 *     are formed in the lattice type on the host, d[n - 1] = 0.  2 <= n <= 65536.  One table per context, shared by every lattice of a batch.
 *   omegam[n] or NULL: TRT's omega- at the same g_i.  NULL: every cell keeps the lattice's omegam.
 *   g_max: the shear of the last entry, finite and positive.
 * lbm_set_rheology: may be called at any time; it touches neither the lattice nor the step count and ends no sampler, and it survives
 *   lbm_set_solid and the other setters.  omega = NULL (omegam NULL too; n and g_max ignored) clears the table and restores the launches, the
 *   bits and the lbm_describe text of a context without it; while a table is set that text gains ` rheology=<n>` (` rheology=<n>+m` with
 *   omegam).  LBM_ERR_INVALID: an entry that is not finite or not in (0, 2) -- the message names its index; n out of range; g_max not finite
 *   or not positive.  LBM_ERR_STATE with a reason: another semantics (which covers slabs), a LBM_FLAG_SOLID_TILES context, omegam on a
 *   context whose collision is not TRT, and buoyancy, a sub-grid constant or a relaxation field set -- each pairing would be one more set
 *   of kernel twins; while a table is set lbm_set_buoyancy, lbm_set_subgrid (cs2 > 0) and lbm_set_relaxation_field refuse in turn.
 * lbm_get_rheology: 1 and the table as the device holds it (rounded to the lattice type; omegam_out untouched without omegam; any pointer
 *   may be NULL) if a table is set, 0 if not.
 * lbm_get_tau on such a context: a cell that is neither solid nor held reports 1 / w_nu, one division in the lattice type, of the step that
 *   starts from the current state; solid and hold cells report the lattice's tau0.
 * lbm_get_shear: g of the rule above for every cell of the current state, indexed like tau_host of lbm_get_tau, with or without a table;
 *   solid and hold cells report 0.  LBM_ERR_STATE on another semantics. */
int lbm_set_rheology(lbm_ctx* c, const double* omega, const double* omegam, int n, double g_max);
int lbm_get_rheology(lbm_ctx* c, double* omega_out, double* omegam_out, int* n_out, double* g_max_out);
int lbm_get_shear(lbm_ctx* c, void* g_host, int host_dtype);

/* --- slab decomposition, externally driven exchange ---------------------------------- */
/* No reference counterpart (the reference is single-GPU, MRT_GPU.py:29).  A step of a slab
 * is split so that a host-language driver can move halos with any transport:
 *     lbm_step_edges()      rows 0 and ny_local-1 (read the ghost rows imported last)
 *     lbm_step_interior()   rows 1 .. ny_local-2
 *     lbm_step_finish()     swap lattices, count the step
 *     lbm_halo_export(side) on both neighbours -> transport -> lbm_halo_import(side)
 * i.e. every step is followed by the exchange of the rows it wrote (lbm_get_fields needs
 * current ghost rows to return the populations of the slab's first and last row).
 * lbm_halo_elems() = elements of one packed halo (3 planes x nx).  buf may be device or
 * host memory.
 *
 * Multi-step launch units between slabs (MRT_GPU semantics; what lbm_step runs when lbm_next_unit() > 1): before a unit of
 * S steps every slab hands the S COMPLETE rows next to each interface to its neighbour --
 *     lbm_halo_export_rows(side, S) -> transport -> lbm_halo_import_rows(side, S)      (lbm_halo_rows_elems(S) elements)
 * -- then lbm_step_unit(S) advances the slab S steps with no further communication: the frame passes recompute a shrinking
 * band of the neighbour's rows.  lbm_step_unit is exactly the launch sequence lbm_step uses between ranks (same kernels,
 * streams and events), minus the RCCL calls; lbm_step = this protocol with the transport inside.
 * Limits: 1 <= nrows <= 9 (a lattice carries 10 ghost rows per side; the tenth serves the recomputation of the lagged fields) and
 * nrows <= ny_local; unit_steps = 3 .. the context's steps per launch (at most 8; exactly 2 for tb_steps = 2), and lbm_next_unit
 * never plans a unit shorter than 4 on a slab. */
int lbm_halo_elems(const lbm_ctx* c);
int lbm_halo_export(lbm_ctx* c, int side, void* buf);
int lbm_halo_import(lbm_ctx* c, int side, const void* buf);
int lbm_step_edges(lbm_ctx* c);
int lbm_step_interior(lbm_ctx* c);
int lbm_step_finish(lbm_ctx* c);
long long lbm_halo_rows_elems(const lbm_ctx* c, int nrows);
int lbm_halo_export_rows(lbm_ctx* c, int side, int nrows, void* buf);
int lbm_halo_import_rows(lbm_ctx* c, int side, int nrows, const void* buf);
int lbm_step_unit(lbm_ctx* c, int unit_steps);

/* --- slab decomposition, RCCL exchange inside lbm_step -------------------------------- */
/* uid_out: 128 bytes (ncclUniqueId) created on one rank and distributed by the caller
 * (e.g. torch.distributed broadcast).  After lbm_comm_init, lbm_step() exchanges halos with
 * rank-1 / rank+1 by ncclSend/ncclRecv on a second HIP stream, overlapped with the
 * interior rows: one row of three directions before a single step; before a launch that advances S
 * steps, the S complete rows next to each interface in one message per side (MRT_GPU semantics).
 * Rank r must hold the r-th slab from the lid (rank 0: y0 = 0, last rank: y0 + ny_local = ny).  lbm_comm_init compares
 * the launch plan (steps per launch, frame width, deep halo, row pitch, planes) with both neighbours and fails with
 * LBM_ERR_STATE if they differ (pass the same lbm_params.ny_local_min on every rank).
 * RCCL is bound with dlopen on the first lbm_comm_* call and the copy already mapped in the process is the one taken.  A process
 * that also loads PyTorch must import it BEFORE that call: created a communicator first and imported torch afterwards, it aborts in
 * the exit handlers (the Python host takes care of the order itself, solver._one_rccl). */
int lbm_comm_unique_id(void* uid_out128);
int lbm_comm_init(lbm_ctx* c, int nranks, int rank, const void* uid128);
/* Diagnostic for one-GPU machines: attaches a ONE-rank RCCL communicator and makes the slab its own
 * neighbour on both sides (its last row arrives in its top ghost row and vice versa, i.e. periodic in y),
 * so that lbm_step() runs the complete exchange path -- edge/interior split, second stream, events,
 * ncclSend/ncclRecv from and into lattice memory.  Only for a slab with y0 > 0 and y0 + ny_local < ny. */
int lbm_comm_loopback(lbm_ctx* c);

/* --- measurement --------------------------------------------------------------------- */
/* Device-to-device streaming copy of `bytes` bytes (read + write), `iters` times; returns
 * achieved (read+write) GB/s: the achievable-bandwidth denominator next to the 8 TB/s peak. */
int lbm_copy_bandwidth(lbm_ctx* c, size_t bytes, int iters, double* gbps);
/* About `ms` milliseconds of packed fp32 fused multiply-adds on every CU (nothing else: no memory traffic); returns the achieved
 * TFLOP/s -- the arithmetic counterpart of lbm_copy_bandwidth, and what bench.py uses, after the copies, to bring the device to the
 * clocks of an arithmetic-bound load before the warm-up steps. */
int lbm_fma_rate(lbm_ctx* c, double ms, double* tflops);

#ifdef __cplusplus
}
#endif
#endif /* LBM_H */
