// lbm_host.hpp -- what the host-side translation units of liblbm_hip.so share: the launch plan (struct Plan), the context (struct
// lbm_ctx), the lazily bound RCCL table, the error macros, the variant dispatcher and the prototypes of every host function that
// crosses a unit.
//   lbm_hip.hip     context life cycle, state upload / field export, probes; what every reader of the exported state starts and
//                   ends with (reader_source, records_to_host)                            (C ABI: create .. get_tau, probes)
//   lbm_plan.hip    parameter validation, launch planning, unit sequence, the dry run    (C ABI: next_unit, describe, plan)
//   lbm_launch.hip  kernel launches and the step loop (run_unit, the lagged lattice)      (C ABI: step*, time_steps)
//   lbm_sampling.hip what the samplers share (schedule: lbm_schedule.hpp; record series; the sampling prologue), the time statistics
//                                                                                          (C ABI: stats_*)
//   lbm_comm.hip    RCCL binding, halo exchanges, host-transported halos                 (C ABI: halo_*, comm_*)
//   lbm_monitor.hip the run monitor and the line export (kernels: lbm_monitor.hpp)        (C ABI: monitor*, get_lines)
//   lbm_residual.hip the field residual (kernels: lbm_residual.hpp)                        (C ABI: residual_*)
//   lbm_topology.hip stream function, vorticity, extrema of psi (kernels: lbm_topology.hpp) (C ABI: topology, get_stream_function)
//   lbm_solid.hip   solid obstacles: the mask and its link plane, the hold cells, the force on the obstacles (k_solid_force); periodic
//                   sides (k_wrap) and the driving force
//                                                                                          (C ABI: set_solid, get_solid, solid_force, set_open_cells, get_open_cells,
//                                                                                           set_periodic, get_periodic, set_driving_force, get_driving_force)
//                   (step kernels, every wall mode: k_step_solid, k_step_generic_wall of lbm_solid.hpp; the mode: with_wall_bits below)
//   lbm_bodies.hip  the one writer of the obstacle state (struct Obstacles); the bodies of a mask: force and torque on each, one-shot
//                   and as a series                                                          (C ABI: set_solid_bodies, get_solid_bodies, body_force, force_*)
//   lbm_body_motion.hip the wall velocity of moving bodies and of single solid cells: its tables (C ABI: set_body_motion, get_body_motion,
//                                                                                          set_wall_velocity, get_wall_velocity)
//   lbm_body_shape.hip  curved obstacle surfaces, a wall distance per link: its tables         (C ABI: set_solid_shape, get_solid_shape)
//   lbm_scalar.hip  the passive scalar of an obstacle lattice: its lattices, tables and step (kernels: lbm_scalar.hpp); the buoyancy
//                                                                                          (C ABI: scalar_*, set_buoyancy, get_buoyancy, set_buoyancy_plane)
// one header of device code that the step units never see:
//   lbm_fields.hpp  the exported state ("what lbm_get_fields would return"): the view Fields that every reader kernel takes -- built
//                   on the host by fields_of below alone -- and the kernels of the field export, lbm_mean_u and the statistics
// and six headers free of HIP, each driven by a CPU test through a program of its own:
//   lbm_schedule.hpp the schedule of automatic sampling
//   lbm_devmem.hpp   the owner of a device allocation, and several tables uploaded into one (the device: HipMem below)
//   lbm_bodies.hpp   the labels of a mask's bodies, their centroids, the link list and its chunks; the tables of a batch
//   lbm_wall_motion.hpp the moving-wall term of every link, the flux check; the tables of a batch
//   lbm_wall_shape.hpp the interpolated bounce-back of every link from its wall distance; the tables of a batch
//   lbm_periodic.hpp periodic sides: the partner of an image cell, the wrap check, the hold cells; the constants of the driving force
//   lbm_order.hpp    the ordering of the two streams: the state carried between units, the skeletons of a unit, the argument
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types and prototypes only: RCCL is bound lazily with dlopen (see rccl_api)
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/lbm.h"
#include "lbm_schedule.hpp"
#include "lbm_order.hpp"
#include "lbm_devmem.hpp"
#include "lbm_bodies.hpp"
#include "lbm_periodic.hpp"
#include "lbm_solid.hpp"  // k_step_solid, k_step_generic_wall, extern (compiled per wall mode in lbm_solid{,_move,_shape,_buoy}_f32/f64.hip, lbm_solid_sgs*, lbm_solid_relax*, lbm_solid_rheo*)
#include "lbm_fields.hpp" // the view of the exported state and the kernels of the field export
#include "lbm_inst.hpp"   // the kernels, and extern template declarations of the multi-step ones (compiled in lbm_{tiles,stream*}_f32/f64.hip)

// ------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------
constexpr int LAT_LAG = 9;    // lat[LAT_LAG]: the lattice of the step before the last, recomputed on demand (lazy one-step lag)
constexpr int NLAT = 10;

// The kernel of the multi-step launch units (ordered: the streaming kernels last, the two with the walls inside after the one with
// a wall frame):
//   none          one step per launch
//   tile2         k_step2_deep: two steps per launch
//   tile          k_stepS_deep: three to five steps per launch, in-place LDS tiles (+ the wall frame)
//   stream        k_stream: the strip-streaming kernel (lbm_stream.hpp, up to 8 steps per launch); its wall frame inside the launch or beside it
//   stream_walls  k_stream_walls / k_stream_walls_slab: ... with the walls inside (no frame)
//   stream_pairs  k_stream_pairs: ... and two rows per wave (twelve waves, up to 10 steps per launch; a lone lattice)
enum class Kern { none, tile2, tile, stream, stream_walls, stream_pairs };

// The launch plan: which kernels run, in which units, with which halo protocol.  A pure function of lbm_params and the device's
// compute units (make_plan, lbm_plan.hip -- the only writer), so that neighbouring slabs derive the same one (lbm_comm_init
// cross-checks) and the dry run lbm_plan describes what lbm_create builds.  A context holds it const.
struct Plan {
    // ---- geometry and sizes
    int es = 0;  // element size
    Geo geo{};
    int nplanes = Q;            // planes of a lattice: the populations (+ the two Smagorinsky history planes)
    int semantics = LBM_SEM_MRT_GPU;   // lbm_params.semantics, for the readers of the plan alone (describe_plan)
    int batch = 1;              // independent lattices per buffer (lbm_params.batch)
    long long bstride = 0;      // elements from one lattice of the batch to the next
    size_t lat_bytes = 0;
    int ncu = 256;              // compute units of the device (the streaming kernel runs one workgroup per CU)
    // ---- kernel choice
    bool use_vec = false;       // vector kernel (MRT_GPU.py semantics, nx multiple of the vector width)
    bool use_nt = false;        // non-temporal loads/stores: lattice far larger than the 256 MiB Infinity Cache
    bool push = false;          // LBM_KERNEL_PUSH: the reference's two-launch push scheme (lat[0], lat[1]: fin ping-pong; lat[2]: ftemp)
    Kern kern = Kern::none;     // several steps per launch (temporal blocking): by which kernel
    int tb_steps = 2;           // steps per launch: two, three to five (tile kernel), up to eight (streaming kernel), ten (pairs)
    int tb_f = TB_F;            // frame width
    bool tail_tiles = false;    // streaming contexts (lone, fp32): units of 3 .. 5 steps through the tile kernel (A/B: LBM_FLAG_NO_TAIL_TILES)
    bool solid_tiles = false;   // LBM_SEM_BOUNCE_BACK_SOLID with LBM_FLAG_SOLID_TILES: kern = tile, planned as LBM_SEM_BOUNCE_BACK with kernel = TB
    // ---- the frame
    bool frame_fused = true;    // all frame passes of a multi-step in one launch (LBM_FLAG_FRAME_UNFUSED: one launch per pass)
    bool frame_lds = true;      // ... keeping the intermediate passes in LDS when their windows fit (LBM_FLAG_NO_FRAME_LDS: scratch lattices)
    bool frame_wide = true;     // frame passes through the scratch lattices: workgroups of 1024 threads (A/B: LBM_FLAG_FRAME_NARROW)
    bool frame_beside = false;  // Kern::stream on a lone lattice: the frame passes as a kernel of their own on the second stream, BESIDE the
                                // streaming workgroups (no LDS, ~70 VGPRs: fits next to them when the streaming kernel leaves registers)
    int frame_seg = 64;         // cells of the frame per workgroup of the fused frame passes (lbm_params.frame_seg)
    // ---- switches
    bool deep_halo = false;     // multi-steps between slabs exchange once per launch (MRT_GPU semantics; LBM_FLAG_NO_DEEP_HALO disables)
    bool lazy_lag = true;       // (LBM_FLAG_EAGER_LAG: every lbm_step call ends with a single step instead)
    bool xcd_bands = true;      // streaming kernel: contiguous runs of segments per XCD (A/B: LBM_FLAG_NO_XCD_BANDS)
    bool edge_first = true;     // streaming kernel between slabs: release the bulk launch behind the edge launch (A/B: LBM_FLAG_NO_EDGE_FIRST)
    bool edge_reserve = true;   // streaming kernel between slabs: a one-round bulk launch leaves CUs to the edge workgroups (A/B: LBM_FLAG_NO_EDGE_RESERVE)
    bool comm_priority = true;  // the halo exchange stream at the highest priority (A/B: LBM_FLAG_COMM_PRIORITY_OFF, the compute stream's)
};

// Device memory has one owner each (lbm_devmem.hpp): nothing else in these units allocates or frees.
struct HipMem {
    static constexpr const char *ALLOC = "hipMalloc", *COPY = "hipMemcpy";
    static const char* text(hipError_t e) { return e == hipSuccess ? nullptr : hipGetErrorString(e); }
    static const char* alloc(void** p, size_t bytes) { return text(hipMalloc(p, bytes)); }
    static void free(void* p) { (void)hipFree(p); }
    static const char* copy(void* dst, const void* src, size_t bytes) { return text(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); }
};
using DevBuf = lbmhost::DevMem<HipMem>;

// The records of a series on the device, [capacity][batch] (empty while it is off), and how many samples it holds and has dropped
// (series_* in lbm_sampling.hip).
struct Series {
    DevBuf dev;
    size_t sample_bytes = 0;    // one sample: the records of the batch
    long long capacity = 0, count = 0, dropped = 0;
};

// The tables of the bodies on the device (body_tables, lbm_bodies.hip), all inside the one allocation `base`, laid out by
// lbmhost::BodyParts (lbm_bodies.hpp): the link list of every lattice, one after the other; chunks[batch][maxchunks]; first[batch]
// [nbodies + 1], each body's range of chunks; centre[batch][nbodies][2]; then the workgroups' partial results of one pass and the
// records of the one-shot call.
struct BodyTables {
    DevBuf base;
    const lbmhost::BodyLink* links = nullptr;
    const lbmhost::BodyChunk* chunks = nullptr;
    const int32_t* first = nullptr;
    const double* centre = nullptr;
    double* partial = nullptr;
    double* rec = nullptr;
    int maxchunks = 1;
};

// The tables of a nonzero body motion on the device (motion_tables, lbm_body_motion.hip), all inside the one allocation `base`, laid
// out by lbmhost::MotionParts (lbm_wall_motion.hpp): cell_row[batch][ny][nx], -1 or the cell's row in delta[rows][8] (the lattice
// type; slot k - 1: Ladd's term of the cell's link k), and link_delta, one double per entry of BodyTables::links: the same terms as
// the lattice adds them, for k_body_force.
struct MotionTables {
    DevBuf base;
    const int32_t* cell_row = nullptr;
    const void* delta = nullptr;
    const double* link_delta = nullptr;
};

// The tables of a shape on the device (shape_tables, lbm_body_shape.hip), all inside the one allocation `base`, laid out by
// lbmhost::ShapeParts (lbm_wall_shape.hpp): cell_row[batch][ny][nx], -1 or the cell's row in ad[rows][16] (the lattice type; a and d of
// the cell's eight links) and near[rows]; link_q, one double per entry of BodyTables::links: the effective q, for the wall point of the
// torque.  The moving-wall term of a shaped context is the d of these tables: they are rebuilt by every call that changes the labels,
// the centres or the motion, and MotionTables stays empty.
struct ShapeTables {
    DevBuf base;
    const int32_t* cell_row = nullptr;
    const void* ad = nullptr;
    const uint8_t* near = nullptr;
    const double* link_q = nullptr;
    template <typename R>
    ShapeTable<R> table() const { return ShapeTable<R>{cell_row, (const R*)ad, near}; }
};

// The hold cells on the device (open_tables, lbm_solid.hip), all inside the one allocation `base`: cell[n][3] = (lattice, x, y) of every
// hold cell and val[n][9] in the lattice type, the populations it holds -- what k_open_fix writes into both lattices after every
// initialisation and upload.  Empty without hold cells.
struct OpenTables {
    DevBuf base;
    const int32_t* cell = nullptr;
    const void* val = nullptr;
    int n = 0;
};

// Solid obstacles (LBM_SEM_BOUNCE_BACK_SOLID; empty in the other semantics).  Three levels of host state, each with what the device
// holds of it; obstacles_change (lbm_bodies.hip) is the only writer: a change at one level resets the levels below it.
//   mask    as lbm_set_solid stored it, 0 / 1, [batch][nx][ny] (all fluid in a fresh context); its link plane lives in the lattices
//   bodies  label[batch][nx][ny], -1 on fluid cells, centre[batch][nbodies][2]; one body that holds every solid cell after
//           lbm_create and lbm_set_solid.  body: the tables; force_series: the records of lbm_force_begin, [capacity][batch][nbodies]
//   motion  motion[batch][nbodies][3] = (Ux, Uy, Om), all zero after lbm_create, lbm_set_solid and lbm_set_solid_bodies.  moving: the
//           tables, empty while every body is at rest -- then the step and the force run the kernels of obstacles that never move
//   shape   beside the motion, not below it: shape_q[batch][8][nx][ny] as lbm_set_solid_shape took it (empty without a shape), shape_eff
//           the effective q (what lbm_get_solid_shape returns), shaped: the tables.  A new mask drops the shape; new bodies and a new
//           motion rebuild the tables from shape_q; the shape itself changes only while every body is at rest.
//   open    below the mask, beside the bodies (lbm_set_open_cells): hold[batch][nx][ny], 0 / 1 (empty without hold cells), hold_f[cells][9]
//           the populations of the hold cells in the order of hold (lattice, x, y), open: the tables.  A new mask drops them; they change
//           only while there is no shape, no motion and no wall velocity, and rebuild the bodies' tables (no link starts at a hold cell).
//   wall_uw with the motion (lbm_set_wall_velocity): uw[batch][2][nx][ny], empty while all zero; its term is part of the one table of the
//           deltas (`moving`, or the d of `shaped`), which every call at the level of the motion rebuilds from both.  A new mask drops
//           it, new bodies keep it.
//   periodic beside the hold cells (lbm_set_periodic): per_x, per_y, and hold_all[batch][nx][ny] = hold and every image cell that is not
//           solid -- what the link planes and every table see as the hold cells (hold_or_null); hold and hold_f stay the user's.  Empty
//           while no side is periodic.  A new mask clears it; lbm_set_open_cells keeps it.
// force_part: the workgroups' partial results of lbm_solid_force and, behind them, its records (allocated on first use, kept).
enum class ObsLevel { mask, bodies, motion, shape, open };
struct Obstacles {
    std::vector<uint8_t> mask;
    int nbodies = 1;
    std::vector<int32_t> label;
    std::vector<double> centre;
    BodyTables body;
    Series force_series;
    std::vector<double> motion;
    MotionTables moving;
    std::vector<double> shape_q, shape_eff;
    ShapeTables shaped;
    std::vector<uint8_t> hold;
    std::vector<double> hold_f;
    OpenTables open;
    std::vector<double> wall_uw;
    bool per_x = false, per_y = false;
    std::vector<uint8_t> hold_all;
    DevBuf force_part;
    bool periodic() const { return per_x || per_y; }
    const uint8_t* hold_or_null() const { return !hold_all.empty() ? hold_all.data() : (hold.empty() ? nullptr : hold.data()); }
    const double* uw_or_null() const { return wall_uw.empty() ? nullptr : wall_uw.data(); }
    bool moves() const {
        return !wall_uw.empty() || std::any_of(motion.begin(), motion.end(), [](double v) { return v != 0.0; });
    }
};

// The passive scalar (lbm_scalar_*, lbm_scalar.hip; kernels and host tables: lbm_scalar.hpp), empty while none is active: the two
// ping-pong lattices in the flow's layout, lat[cur] the source of the next scalar step and raw[i] != 0 while lat[i] holds plain
// populations; the wall-value table (cell_row[ny][nx], val[rows][8] in the lattice type, bits[rows]) and the constants of the user's hold
// cells (hold_cell[n][2] = (x, y), hold_val[n][9] in the lattice type), each inside one allocation; part: the workgroups' partial results
// of the totals and of the flux and, behind them, their records (allocated on first use, kept).  steps: scalar steps since
// lbm_scalar_begin or lbm_scalar_set_state.
struct ScalarState {
    bool active = false;
    double D = 0.0, magic = 0.0;
    DevBuf lat[2];
    int raw[2] = {1, 1};
    int cur = 0;
    long long steps = 0;
    DevBuf walls, holds, part;
    const int32_t* cell_row = nullptr;
    const void* val = nullptr;
    const uint8_t* bits = nullptr;
    const int32_t* hold_cell = nullptr;
    const void* hold_val = nullptr;
    int nhold = 0;
    // Buoyancy (lbm_set_buoyancy), part of the scalar's state so that whatever ends the scalar ends it first: buoy = (ax, ay, c_ref) and cp,
    // the buoyancy plane -- one plane of the flow's rows and type (buoy_at, lbm_device.hpp) that holds the C the most recent scalar step summed (after
    // lbm_set_buoyancy, lbm_scalar_begin and lbm_scalar_set_state: C of the state as it is, scalar_fill_plane).  Empty while none is set.
    bool buoyant = false;
    double buoy[3] = {0.0, 0.0, 0.0};
    DevBuf cp;
};

// Run state.  What was decided once is in `plan`; p stays for the fields later code branches on (dtype, collision, semantics, turb,
// arith, device) and for the relaxation rates, which lbm_set_relaxation rewrites.
struct lbm_ctx {
    lbm_ctx(const lbm_params& p_, const Plan& plan_) : p(p_), plan(plan_) {}
    lbm_params p;
    const Plan plan;
    DevBuf lat[NLAT];           // [0], [1]: the two lattices; [2] .. [8]: frame scratch of the multi-step; [LAT_LAG]: see above
    int raw[NLAT] = {1, 1, 0, 0, 0, 0, 0, 0, 0, 0};
    int cur = 0;  // lat[cur] is the source of the next step
    long long nsteps = 0;
    // One-step lag of u / rho: the fields of the last iteration are moments of the state it started from.
    // After a single step that state is still in lat[cur ^ 1] (lag = 0).  After a launch unit of S steps lat[cur ^ 1] holds the
    // state S steps back: lag = S - 1 steps are recomputed from it into lat[LAT_LAG] when lbm_get_fields / lbm_mean_u /
    // lbm_get_tau ask (lag_valid: done already) -- bit-identical, and off the path of lbm_step.
    int lag = 0;
    bool lag_valid = false;
    hipStream_t s_compute = nullptr, s_comm = nullptr;
    hipEvent_t ev_edges = nullptr, ev_halo = nullptr, ev_int = nullptr, ev_go = nullptr, ev_t0 = nullptr, ev_t1 = nullptr;
    DevBuf stage;               // host <-> lattice staging (ensure_stage)
    DevBuf red_dev;             // lbm_mean_u: partial sums + results
    // The samplers (lbm_sampling.hip).  sampler[i]: the schedule of automatic sampling, which takes the sample of step count n from
    // lat[cur] when a unit would start at n - 1 (step_many) -- the force sampler: when a unit has ended at n; a Series: the records of a
    // series on the device, empty while it is off.
    lbmhost::Sampler sampler[lbmhost::NSCHEDULED];
    // Time statistics (lbm_stats_*): six double sums per cell (k_stats_accumulate), empty while statistics are off.
    DevBuf stats_dev;
    long long stats_count = 0;  // samples enqueued
    // Run monitor (lbm_monitor*, lbm_monitor.hip): mon_part holds the workgroups' partial results of one pass and, behind them, the
    // records of the one-shot call (allocated on first use, kept).
    DevBuf mon_part;
    Series mon_series;
    lbm_monitor_spec mon_spec{};
    // Field residual (lbm_residual_*, lbm_residual.hip): res_snap holds the previous sample (ux, uy, rho of every own cell, in the type
    // lbm_get_fields(res_host_dtype) hands out), res_part the workgroups' partial results of one pass; empty while the residual is off.
    // res_prev: the step count of the snapshot (-1: no sample yet).
    DevBuf res_snap, res_part;
    Series res_series;
    int res_host_dtype = LBM_F32;
    long long res_prev = -1;
    // Flow topology (lbm_topology, lbm_get_stream_function; lbm_topology.hip): topo_part holds the block sums, the partial results and
    // the records of the record path, topo_fields the staged psi and omega of the field path; each allocated on first use, kept.
    DevBuf topo_part, topo_fields;
    Obstacles obs;              // (above)
    ScalarState scalar;         // (above)
    double drive[2] = {0.0, 0.0};   // the driving force (lbm_set_driving_force): (fx, fy); no geometry, so it outlives every obstacle call
    bool driven() const { return drive[0] != 0.0 || drive[1] != 0.0; }
    double subgrid = 0.0;           // the sub-grid constant Cs2 (lbm_set_subgrid), 0 without the closure; no geometry and no history either
    // A relaxation field (lbm_set_relaxation_field), empty while none is set: relax_w the plane of the cells' viscous rates, relax_wm the
    // plane of TRT's odd rates or empty -- read-only, in the lattice type, rows as the buoyancy plane's (buoy_at), lattice b of a batch at
    // b * buoy_elems; ghost and pad elements hold the rate the lattice had when the field was set.  No geometry and no history.
    DevBuf relax_w, relax_wm;
    bool relax_field() const { return (bool)relax_w; }
    // A rheology table (lbm_set_rheology), empty while none is set: rheo_tab the table as rheology_table (lbm_rheology.hpp) lays it out, in
    // the lattice type, one for every lattice of a batch; rheo_w / rheo_wm the entries as the device holds them (rounded to the lattice
    // type; rheo_wm empty without TRT's odd rate), rheo_gmax the shear of the last entry.  No geometry and no history.
    DevBuf rheo_tab;
    std::vector<double> rheo_w, rheo_wm;
    double rheo_gmax = 0.0;
    bool rheology() const { return (bool)rheo_tab; }
    ncclComm_t comm = nullptr;
    int nranks = 1, rank = 0;
    bool loopback = false;      // diagnostic: 1-rank communicator, the slab exchanges halos with itself
    lbmhost::Order order;       // what the two streams carry from one unit to the next (lbm_order.hpp); its device: HipDev below
    DevBuf relax_dev;           // batch > 1: Relax<real>[batch] on the device
    std::string err;
};

namespace lbmhost {

// RCCL entry points, resolved on first use.  liblbm_hip.so carries no DT_NEEDED on librccl:
// single-GPU processes never load it, and in a process that also runs torch.distributed the
// dlopen below returns the RCCL that is already mapped (same SONAME), so both share one.
struct rccl_api {
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    bool ok = false;
    std::string err;
};

inline int fail(lbm_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}
// what DevBuf::alloc / ensure said: "" or the error
inline int alloc_ok(lbm_ctx* c, const std::string& err) { return err.empty() ? LBM_OK : fail(c, LBM_ERR_NOMEM, err); }
// The refusal of the obstacle calls in a context of another semantics.
inline int need_solid(lbm_ctx* c, const char* call) {
    if (c->p.semantics == LBM_SEM_BOUNCE_BACK_SOLID) return LBM_OK;
    return fail(c, LBM_ERR_STATE, std::string(call) + ": this context has no solid mask (create it with semantics = LBM_SEM_BOUNCE_BACK_SOLID)");
}
// The refusal of a setter in a context on the multi-step tile kernel (LBM_FLAG_SOLID_TILES); lacks: what that kernel does not do.
inline int need_one_step(lbm_ctx* c, const char* call, const char* lacks) {
    if (!c->plan.solid_tiles) return LBM_OK;
    return fail(c, LBM_ERR_STATE, std::string(call) + ": the tile kernel " + lacks + " (LBM_FLAG_SOLID_TILES takes none; create the context without the flag)");
}

#define HIP_TRY(c, expr)                                                                               \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return fail((c), LBM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));          \
    } while (0)

#define NCCL_TRY(c, expr)                                                                              \
    do {                                                                                               \
        ncclResult_t r_ = (expr);                                                                      \
        if (r_ != ncclSuccess)                                                                         \
            return fail((c), LBM_ERR_COMM, std::string(#expr) + ": " + rccl().GetErrorString(r_));     \
    } while (0)

// The device of c->order: its events and streams are the context's.
struct HipDev {
    lbm_ctx* c;
    hipStream_t stream(Stream s) const { return s == Stream::COMPUTE ? c->s_compute : c->s_comm; }
    hipEvent_t event(Event e) const { return e == Event::INT ? c->ev_int : e == Event::EDGES ? c->ev_edges : e == Event::GO ? c->ev_go : c->ev_halo; }
    int record(Event e, Stream s) {
        HIP_TRY(c, hipEventRecord(event(e), stream(s)));
        return LBM_OK;
    }
    int wait(Stream s, Event e) {
        HIP_TRY(c, hipStreamWaitEvent(stream(s), event(e), 0));
        return LBM_OK;
    }
};

template <typename R>
Relax<R> relax_of(const lbm_params& p) {
    Relax<R> w;
    w.uLB = (R)p.uLB; w.w_nu = (R)p.omega; w.w_m = (R)p.omegam;
    w.w_e = (R)p.omega_e; w.w_eps = (R)p.omega_eps; w.w_q = (R)p.omega_q;
    return w;
}

// The driving force as the one-step obstacle kernels take it: F_k in double (drive_terms), each rounded once to the lattice type.
template <typename R>
Drive<R> drive_of(const lbm_ctx* c) {
    Drive<R> d{};
    if (!c->driven()) return d;
    double f[8];
    drive_terms(c->drive[0], c->drive[1], f);
    for (int k = 0; k < 8; ++k) d.f[k] = (R)f[k];
    d.on = 1;
    return d;
}

// Buoyancy as the one-step obstacle kernels take it: B_k in double (the arithmetic of drive_terms on (ax, ay)) and c_ref, each rounded
// once to the lattice type, and the plane.
template <typename R>
Buoy<R> buoy_of(const lbm_ctx* c) {
    Buoy<R> b{};
    double f[8];
    drive_terms(c->scalar.buoy[0], c->scalar.buoy[1], f);
    for (int k = 0; k < 8; ++k) b.b[k] = (R)f[k];
    b.c_ref = (R)c->scalar.buoy[2];
    b.cp = c->scalar.cp.as<const R>();
    return b;
}

// The sub-grid constant as the kernels take it: k = 18 sqrt(2) Cs2 in double, rounded once to the lattice type (subgrid_tau, lbm_device.hpp).
template <typename R>
R sgs_k(const lbm_ctx* c) {
    return (R)((18.0 * std::sqrt(2.0)) * c->subgrid);
}

template <typename R>
Batch<R> batch_of(const lbm_ctx* c) {
    return Batch<R>{c->plan.bstride, c->plan.batch > 1 ? c->relax_dev.as<const Relax<R>>() : nullptr};
}

// output lattices of the S frame passes lat[from] -> lat[to]: the scratch lattices (null when never needed, see ensure_scratch), then lat[to]
template <typename R>
FramePtrs<R> frame_ptrs(const lbm_ctx* c, int from, int to, int S) {
    FramePtrs<R> fp;
    fp.src = c->lat[from].as<const R>();
    for (int i = 0; i < 8; ++i) fp.pass[i] = (i < S - 1 ? c->lat[2 + i] : c->lat[to]).as<R>();
    return fp;
}

inline dim3 grid_rows(const lbm_ctx* c, int nrows) { return dim3((c->plan.geo.nx + BLK - 1) / BLK, nrows, c->plan.batch); }
// grid of the host-layout <-> lattice kernels: tiles of trx<R>() columns x 32 rows
template <typename R>
dim3 grid_tiles(const lbm_ctx* c) { return dim3((c->plan.geo.nx + trx<R>() - 1) / trx<R>(), (c->plan.geo.ny + 31) / 32, c->plan.batch); }

// Run-time parameters -> compile-time kernel variant (real type, collision operator, semantics, Smagorinsky).
// (The sub-grid closure and the relaxation field of an obstacle lattice are bits of the wall mode, not of the variant: with_wall_step.)
template <typename R_, int COLL_, int SEM_, bool TURB_>
struct Variant {
    using R = R_;
    static constexpr int COLL = COLL_, SEM = SEM_;
    static constexpr bool TURB = TURB_;
};

// arith = promoted: fp32 takes the promoted operators, fp64 the strict ones (the promotion's casts are no-ops there).
template <typename F>
void dispatch(const lbm_params& p, F&& f) {
    auto by_sem = [&](auto real, auto coll) {
        using R = decltype(real);
        constexpr int C = decltype(coll)::value;
        constexpr int CS = C == C_MRT_FAST ? C_MRT : (C == C_SRT_FAST ? C_SRT : (C == C_TRT_FAST ? C_TRT : C));
        if constexpr (coll_is_prom(C)) {   // (MRT_GPU semantics only: validate_params)
            if (p.turb) f(Variant<R, C, SEM_GPU, true>{});
            else f(Variant<R, C, SEM_GPU, false>{});
        } else {
            if (p.semantics == LBM_SEM_MRT_PY) f(Variant<R, CS, SEM_PY, false>{});   // (arith = fast: MRT_GPU semantics only)
            else if (p.semantics == LBM_SEM_BOUNCE_BACK) f(Variant<R, C, SEM_BB, false>{});   // (strict and fast; no closure: validate_params)
            else if (p.semantics == LBM_SEM_BOUNCE_BACK_SOLID) f(Variant<R, C, SEM_SOLID, false>{});   // (the same, one step per launch)
            else if (p.turb) f(Variant<R, C, SEM_GPU, true>{});
            else f(Variant<R, C, SEM_GPU, false>{});
        }
    };
    auto pick = [&](auto real, auto strict, auto fast, auto prom) {
        if (p.arith == LBM_ARITH_FAST) by_sem(real, fast);
        else if constexpr (std::is_same<decltype(real), float>::value) {
            if (p.arith == LBM_ARITH_PROMOTED) by_sem(real, prom);
            else by_sem(real, strict);
        } else {
            by_sem(real, strict);
        }
    };
    auto by_coll = [&](auto real) {
        switch (p.collision) {
            case LBM_SRT:
                pick(real, std::integral_constant<int, C_SRT>{}, std::integral_constant<int, C_SRT_FAST>{}, std::integral_constant<int, C_SRT_PROM>{});
                break;
            case LBM_TRT:
                pick(real, std::integral_constant<int, C_TRT>{}, std::integral_constant<int, C_TRT_FAST>{}, std::integral_constant<int, C_TRT_PROM>{});
                break;
            default:
                pick(real, std::integral_constant<int, C_MRT>{}, std::integral_constant<int, C_MRT_FAST>{}, std::integral_constant<int, C_MRT_PROM>{});
                break;
        }
    };
    if (p.dtype == LBM_F32) by_coll(float{});
    else by_coll(double{});
}
// The view of lat[which] for the kernels that read the exported state (VT: the context's Variant): the one place outside the step
// launchers that pairs a lattice with its raw flag, the lid velocity and the batch stride.  which: reader_source's for what
// lbm_get_fields exports now; c->cur for the sample of the iteration about to start (sample_if_due) and for the populations.
template <typename VT, bool SHAPE = false>
Fields<typename VT::R, VT::SEM, coll_is_prom(VT::COLL), SHAPE> fields_of(const lbm_ctx* c, int which) {
    using R = typename VT::R;
    Fields<R, VT::SEM, coll_is_prom(VT::COLL), SHAPE> f;
    f.src = c->lat[which].as<const R>();
    f.geo = c->plan.geo;
    f.raw = c->raw[which];
    f.uLB = (R)c->p.uLB;
    f.bstride = c->plan.bstride;
    if constexpr (SHAPE) f.sh = c->obs.shaped.template table<R>();
    return f;
}
// ... and what every launcher of a reader kernel goes through: launch(view), the view with the shape table compiled in while a shape
// is set (lbm_set_solid_shape), the plain one otherwise.  The kernel takes decltype(view)::SHAPED as its last template argument.
template <typename VT, typename F>
void with_fields(const lbm_ctx* c, int which, F&& launch) {
    if constexpr (VT::SEM == SEM_SOLID) {
        if (c->obs.shaped.base) {
            launch(fields_of<VT, true>(c, which));
            return;
        }
    }
    launch(fields_of<VT, false>(c, which));
}
// The rheology table as the kernels take it (Rheo, lbm_device.hpp); tab null without one
template <typename R>
Rheo<R> rheo_of(const lbm_ctx* c) {
    Rheo<R> rh{};
    if (!c->rheology()) return rh;
    const int n = (int)c->rheo_w.size();
    rh.tab = c->rheo_tab.as<const R>();
    rh.inv_dg = rheology_inv_dg<R>(n, c->rheo_gmax);
    rh.nm1 = n - 1;
    rh.has_m = c->rheo_wm.empty() ? 0 : 1;
    return rh;
}
// The mode of the obstacle wall rule (WallArg, lbm_device.hpp: base | bits), and the one place that reads the obstacle state to pick the
// base and to fill the mode: launch(wa, link), wa the tables of the base -- a shape (which carries a motion's term in its table), else a
// nonzero motion, else nothing -- with the fields of every bit of BITS, and link the base's double per entry of BodyTables::links (link_q,
// link_delta, null).  The kernel takes decltype(wa)::MODE as its last template argument and wa as its last argument.
template <typename R, int BITS, typename F>
void with_wall_bits(const lbm_ctx* c, F&& launch) {
    const ShapeTables& sh = c->obs.shaped;
    const MotionTables& m = c->obs.moving;
    auto filled = [&](auto wa, const double* link) {
        if constexpr (wall_buoyant(BITS)) wa.by = buoy_of<R>(c);
        if constexpr (wall_subgrid(BITS)) wa.sgs = sgs_k<R>(c);   // (k = 18 sqrt(2) Cs2)
        if constexpr (wall_relax(BITS)) {
            wa.rw = c->relax_w.as<const R>();
            wa.rwm = c->relax_wm.as<const R>();
        }
        if constexpr (wall_rheo(BITS)) wa.rh = rheo_of<R>(c);
        launch(wa, link);
    };
    if constexpr (!wall_buoyant(BITS)) {   // (no buoyant mode with a shape: lbm_set_buoyancy and lbm_set_solid_shape refuse each other)
        if (sh.base) {
            WallArg<R, WALL_SHAPE | BITS> wa{};
            wa.sh = sh.template table<R>();
            return filled(wa, sh.link_q);
        }
    }
    if (m.base) {
        WallArg<R, WALL_MOVE | BITS> wa{};
        wa.cell_row = m.cell_row;
        wa.delta = (const R*)m.delta;
        return filled(wa, m.link_delta);
    }
    filled(WallArg<R, WALL_REST | BITS>{}, (const double*)nullptr);
}
// The force kernels: the base alone -- what they read of the lattice changes with no bit.
template <typename VT, typename F>
void with_wall(const lbm_ctx* c, F&& launch) { with_wall_bits<typename VT::R, 0>(c, launch); }
// The step kernels (launch_rows): the bits of the context's run state -- a relaxation field (lbm_set_relaxation_field) and the sub-grid
// closure (lbm_set_subgrid), alone or together, else buoyancy (lbm_set_buoyancy), which the setters let stand beside neither, else a
// rheology table (lbm_set_rheology), which they let stand beside none of the three.
template <typename VT, typename F>
void with_wall_step(const lbm_ctx* c, F&& launch) {
    using R = typename VT::R;
    const bool sgs = c->subgrid > 0.0, field = c->relax_field();
    if (sgs && field) with_wall_bits<R, WALL_SGS | WALL_RELAX>(c, launch);
    else if (field) with_wall_bits<R, WALL_RELAX>(c, launch);
    else if (sgs) with_wall_bits<R, WALL_SGS>(c, launch);
    else if (c->scalar.buoyant) with_wall_bits<R, WALL_BUOY>(c, launch);
    else if (c->rheology()) with_wall_bits<R, WALL_RHEO>(c, launch);
    else with_wall_bits<R, 0>(c, launch);
}
// A launcher's body: f(Variant) enqueues the kernels of the context's variant, then the launch error check
template <typename F>
int launch_variant(lbm_ctx* c, F&& f) {
    dispatch(c->p, f);
    HIP_TRY(c, hipGetLastError());
    return LBM_OK;
}
// segments of L cells that cover n cells of a frame strip (the fused frame passes run one workgroup per segment, frame_passes)
inline int frame_segs(int n, int L) { return (n + L - 1) / L; }
struct StreamPlan { int nstrips, nsegy, H; };
// Is a multi-step kernel compiled for the semantics?  The tile kernel and the frame passes: for all of them (solid obstacles run them
// with LBM_FLAG_SOLID_TILES, one step per launch otherwise: Plan::solid_tiles); the streaming kernels and the frame beside them
// (`streaming_kernel`): not with solid obstacles.
constexpr bool sem_multi_step(int sem, bool streaming_kernel = false) { return sem != SEM_SOLID || !streaming_kernel; }

// Waiting for the device: poll for a short while, then block.  A blocking hipStreamSynchronize / hipEventSynchronize wakes the host
// tens of microseconds after the work is done -- 5 % of the driver's 20-step window of 1.1 ms (profiles/r02_logs/unit_times.log);
// a run that is still busy after SPIN_US hands the core back.
constexpr long long SPIN_US = 3000;
template <typename Q>
bool spin_until_ready(Q&& query) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = query();
        if (e == hipSuccess) return true;
        if (e != hipErrorNotReady) { (void)hipGetLastError(); return false; }
        if (std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() > SPIN_US) return false;
    }
}

// Is there a slab beyond this side?  Geometry decides (the slab does not touch the lid / the bottom wall there): the frame
// passes of a multi-step extend into the ghost rows of such a side whatever moves the rows -- RCCL between ranks
// (lbm_comm_init checks that rank r holds the r-th slab), the loopback diagnostic, or the caller (lbm_halo_*_rows).
inline bool has_neighbour(const Plan& pl, int side) {
    return side == LBM_SIDE_LOW ? pl.geo.y0 > 0 : pl.geo.y0 + pl.geo.ny < pl.geo.NY;
}
inline int neighbours(const Plan& pl) { return (has_neighbour(pl, LBM_SIDE_LOW) ? 1 : 0) + (has_neighbour(pl, LBM_SIDE_HIGH) ? 1 : 0); }
inline bool is_slab(const Plan& pl) { return neighbours(pl) > 0; }
// the library itself moves the halos (RCCL between ranks, or the one-GPU loopback)
inline bool own_transport(const lbm_ctx* c) { return c->comm != nullptr && (c->nranks > 1 || c->loopback); }
inline bool streaming(const Plan& pl) { return pl.kern >= Kern::stream; }
inline bool walls_inside(const Plan& pl) { return pl.kern >= Kern::stream_walls; }

// How a launch unit of S >= 2 steps runs (unit_route):
//   one_launch    a lone lattice: frame and bulk (or the walls inside) in ONE launch on s_compute
//   edges_bulk    a slab under the streaming kernel: the edge launch (launch_stream_edges), then the bulk launch
//   fused_frame   all frame passes in one launch (launch_frame_multi / k_frame_beside), then the bulk launch
//   frame_passes  one launch per frame pass (launch_frame), then the bulk launch
//   single_steps  S single steps (the replay of the lagged lattice only)
enum class Route { one_launch, edges_bulk, fused_frame, frame_passes, single_steps };

// Deep halo for a multi-step of S steps: the S complete rows (all planes, ghost columns included) next to each interface go to
// the neighbour's ghost rows in ONE message per side; the S frame passes then recompute a shrinking band of the neighbour's
// rows (rows -(S - i) .. for pass i) instead of exchanging one row per pass.  RCCL's latency per exchange, not its bandwidth,
// is what the per-pass scheme cannot hide: 739 KB once instead of 5 x 48 KB.  MRT_GPU semantics only: there a
// side-wall cell overwrites the slots it does not stream by the wall rule, so nothing a cell needs lives in the ghost columns
// of a ghost row (MRT.py's left wall reads parked values).
//
// The rows are described once, as blocks of contiguous elements, for RCCL (below) and for the externally driven exchange
// (lbm_halo_export_rows / lbm_halo_import_rows): [y][k][x] layout: S rows of all planes are ONE block; [k][y][x]: one per plane.
struct RowBlocks {
    int n = 0;
    char* ptr[Q + 2];
    size_t elems = 0;   // per block
};

// ---- host functions that cross a unit (defined in the unit the name of which is given) ----
// lbm_hip.hip
int ensure_stage(lbm_ctx* c, size_t bytes);
int ensure_field_stage(lbm_ctx* c);
int sync_all(lbm_ctx* c);
int reader_source(lbm_ctx* c, const std::string& call, bool needs_step, int* which);
int records_to_host(lbm_ctx* c, const void* dev, size_t bytes, void* out);
int host_to_stage(lbm_ctx* c, const void* host, int host_dtype, int planes);
int stage_to_host(lbm_ctx* c, const void* stage, void* host, int host_dtype, int planes);
// lbm_plan.hip
bool frame_lds_fits(const Plan& pl, int S, bool deep_rows, int extra = 0, long long budget = FRAME_LDS_BYTES);
int pairs_waves(int S);
StreamPlan plan_stream_on(const Plan& pl, int S, int ncu, long long* cost_out);
StreamPlan plan_stream(const Plan& pl, int S);
bool lag_replayable(const Plan& pl, int S);
int unit_steps(const Plan& pl, int left, bool raw, bool own_transport);
Route unit_route(const Plan& pl, int S, bool replay);
std::string validate_params(const lbm_params* p);
bool make_plan(const lbm_params& p, int ncu, bool device, Plan& pl, std::string& err);
// lbm_launch.hip
int ensure_scratch(lbm_ctx* c, int n);
int launch_rows(lbm_ctx* c, int from, int to, int row0, int stride, int nrows, hipStream_t s);
int launch_frame(lbm_ctx* c, int from, int to, int W, hipStream_t s, int elo = 0, int ehi = 0);
int launch_frame_multi(lbm_ctx* c, int from, int to, int S, hipStream_t s, bool lo, bool hi, int extra = 0);
int launch_stream(lbm_ctx* c, int from, int to, hipStream_t s, int S, bool with_frame);
int launch_stream_edges(lbm_ctx* c, int from, int to, hipStream_t s, int S, bool lo, bool hi, int extra);
int warm_stream(lbm_ctx* c);
int launch_deep(lbm_ctx* c, int from, int to, hipStream_t s, int steps, bool with_frame = false);
void finish_unit(lbm_ctx* c, int S);
int run_unit(lbm_ctx* c, bool* comm_used, int S, bool rccl_x);
int prev_lattice(lbm_ctx* c, int* which);
int push_step(lbm_ctx* c);
int push_reset(lbm_ctx* c);
int step_many(lbm_ctx* c, int nsteps);
// lbm_sampling.hip
int series_alloc(lbm_ctx* c, Series& s, size_t record_bytes, int capacity, const char* what);
void* series_slot(Series& s);
int series_read(lbm_ctx* c, const Series* (*series)(const lbm_ctx*), const char* call, void* records_out, int max_records, long long* count,
                long long* dropped);
int sampler_begin(lbm_ctx* c, int sampler, int every);
int sample_now(lbm_ctx* c, int sampler, bool on);
int sample_if_due(lbm_ctx* c);
int sample_after_unit(lbm_ctx* c);
void sampler_free(lbm_ctx* c, int sampler);
int sampler_end(lbm_ctx* c, int sampler);
// lbm_monitor.hip
int monitor_series_sample(lbm_ctx* c, int which, long long step);
// lbm_solid.hip
int solid_fix(lbm_ctx* c);
int solid_copy_links(lbm_ctx* c, int to);
int periodic_wrap(lbm_ctx* c, int which, hipStream_t s);
int periodic_wrap_lattice(lbm_ctx* c, void* lat, hipStream_t s);
// lbm_scalar.hip
int scalar_step(lbm_ctx* c);
void scalar_free(lbm_ctx* c);
// lbm_bodies.hip
int obstacles_change(lbm_ctx* c, ObsLevel level, Obstacles& next, int (*before_commit)(lbm_ctx*, const Obstacles&) = nullptr,
                     const char* call = "lbm_set_body_motion");
int force_series_sample(lbm_ctx* c);
// lbm_body_motion.hip
int motion_tables(lbm_ctx* c, const Obstacles& next, MotionTables& out, bool check_only = false, const char* call = "lbm_set_body_motion");
// lbm_body_shape.hip
int shape_tables(lbm_ctx* c, const Obstacles& next, const std::vector<double>& q, ShapeTables& out, std::vector<double>* q_eff);
// lbm_residual.hip
int residual_series_sample(lbm_ctx* c, int which, long long step);
void residual_free(lbm_ctx* c);
// lbm_comm.hip
rccl_api& rccl();
void halo_range(const lbm_ctx* c, int k, int* lo, int* hi);
const int* side_planes(int side);
char* plane_row(lbm_ctx* c, int which, int k, int y);
int enqueue_exchange(lbm_ctx* c, int which);
RowBlocks deep_blocks(lbm_ctx* c, int which, int r0, int S);
int deep_send_row0(const lbm_ctx* c, int side, int S);
int deep_recv_row0(const lbm_ctx* c, int side, int S);
int enqueue_deep_exchange(lbm_ctx* c, int which, int S);
}  // namespace lbmhost
