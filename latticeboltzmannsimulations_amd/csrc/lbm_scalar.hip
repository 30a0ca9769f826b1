// lbm_scalar.hip -- liblbm_hip.so: the passive scalar of an obstacle lattice (lbm_scalar_begin, lbm_scalar_end, lbm_scalar_active,
// lbm_scalar_get, lbm_scalar_get_stored, lbm_scalar_set_state, lbm_scalar_totals, lbm_scalar_flux, and the buoyancy through which it acts on
// the flow, lbm_set_buoyancy, lbm_get_buoyancy, lbm_set_buoyancy_plane, of the C ABI declared in include/lbm.h;
// LBM_SEM_BOUNCE_BACK_SOLID, a lone lattice, one step per launch).  The rule, the kernels and the host tables are lbm_scalar.hpp's; here:
// the state (ScalarState, lbm_host.hpp), the step that run_unit enqueues behind every flow step, the uploads and the exports.  gfx950
// only.  DESIGN.md 2.10.
#include <cmath>

#include "lbm_host.hpp"
#include "lbm_scalar.hpp"

namespace lbmhost {

static_assert(sizeof(lbm_scalar_record) == 5 * sizeof(double) && sizeof(lbm_scalar_flux_record) == 3 * sizeof(double), "record layout");

template <typename R>
static ScalarArg<R> scalar_arg(const lbm_ctx* c) {
    const ScalarState& sc = c->scalar;
    double wp = 0.0, wm = 0.0;
    scalar_rates(sc.D, sc.magic, &wp, &wm);
    return ScalarArg<R>{(R)wp, (R)wm, sc.cell_row, (const R*)sc.val, sc.bits};
}

// One scalar step, lat[cur] -> lat[cur ^ 1], from the flow lattice the flow step has just written (c->cur, its image cells wrapped), then
// the scalar's own wrap; on s_compute.
int scalar_step(lbm_ctx* c) {
    ScalarState& sc = c->scalar;
    const int a = sc.cur, b = sc.cur ^ 1;
    int rc = launch_variant(c, [&](auto v) {
        using VT = decltype(v);
        using R = typename VT::R;
        if constexpr (VT::SEM == SEM_SOLID) {
            constexpr int V = 16 / (int)sizeof(R);
            const Geo& g = c->plan.geo;
            const R* src = sc.lat[a].as<const R>();
            R* dst = sc.lat[b].as<R>();
            with_fields<VT>(c, c->cur, [&](auto f) {
                constexpr bool SHAPED = decltype(f)::SHAPED;
                if constexpr (!SHAPED) {
                    if (sc.buoyant) {   // (buoyancy, never with a shape: the same step, and the C it sums into the buoyancy plane)
                        R* cp = sc.cp.as<R>();
                        if (c->plan.use_vec) {
                            const int nxb = (g.nx / V + BLK - 1) / BLK, nblocks = nxb * g.ny;
                            if (c->plan.use_nt)
                                hipLaunchKernelGGL((k_scalar_step_cp<R, true>), dim3(nblocks), dim3(BLK), 0, c->s_compute, src, dst, f, scalar_arg<R>(c), sc.raw[a],
                                                   nxb, nblocks, cp);
                            else
                                hipLaunchKernelGGL((k_scalar_step_cp<R, false>), dim3(nblocks), dim3(BLK), 0, c->s_compute, src, dst, f, scalar_arg<R>(c), sc.raw[a],
                                                   nxb, nblocks, cp);
                        } else {
                            hipLaunchKernelGGL((k_scalar_generic_cp<R>), dim3((g.nx + BLK - 1) / BLK, g.ny), dim3(BLK), 0, c->s_compute, src, dst, f,
                                               scalar_arg<R>(c), sc.raw[a], cp);
                        }
                        return;
                    }
                }
                if (c->plan.use_vec) {
                    const int nxb = (g.nx / V + BLK - 1) / BLK, nblocks = nxb * g.ny;
                    if (c->plan.use_nt)
                        hipLaunchKernelGGL((k_scalar_step<R, true, SHAPED>), dim3(nblocks), dim3(BLK), 0, c->s_compute, src, dst, f, scalar_arg<R>(c), sc.raw[a], nxb,
                                           nblocks);
                    else
                        hipLaunchKernelGGL((k_scalar_step<R, false, SHAPED>), dim3(nblocks), dim3(BLK), 0, c->s_compute, src, dst, f, scalar_arg<R>(c), sc.raw[a], nxb,
                                           nblocks);
                } else {
                    hipLaunchKernelGGL((k_scalar_generic<R, SHAPED>), dim3((g.nx + BLK - 1) / BLK, g.ny), dim3(BLK), 0, c->s_compute, src, dst, f, scalar_arg<R>(c),
                                       sc.raw[a]);
                }
            });
        }
    });
    if (rc == LBM_OK) rc = periodic_wrap_lattice(c, sc.lat[b].get(), c->s_compute);
    if (rc) return rc;
    sc.cur = b;
    sc.raw[b] = 0;
    ++sc.steps;
    return LBM_OK;
}

// The buoyancy plane from the scalar lattice `which` as it is (k_scalar_plane): C as lbm_scalar_get's conc_out forms it; on s_compute.
static int scalar_fill_plane(lbm_ctx* c, int which) {
    ScalarState& sc = c->scalar;
    const Geo& g = c->plan.geo;
    return launch_variant(c, [&](auto v) {
        using R = typename decltype(v)::R;
        hipLaunchKernelGGL((k_scalar_plane<R>), dim3((g.nx + BLK - 1) / BLK, g.ny), dim3(BLK), 0, c->s_compute, sc.lat[which].as<const R>(), c->lat[0].as<const R>(),
                           g, scalar_arg<R>(c), sc.raw[which], sc.cp.as<R>());
    });
}

// The scalar ends (and with it the buoyancy): its lattices and tables are freed.  The caller has synchronised the streams.
void scalar_free(lbm_ctx* c) { c->scalar = ScalarState{}; }

// Plain populations g[9][nx][ny] of the lattice type in the staging buffer -> lat[0]; then the zeros of the solid cells and the constants
// of the hold cells in both lattices, and the image cells of both; the next step is raw.
static int scalar_from_stage(lbm_ctx* c) {
    ScalarState& sc = c->scalar;
    const Geo& g = c->plan.geo;
    int rc = launch_variant(c, [&](auto v) {
        using R = typename decltype(v)::R;
        const dim3 grid((g.nx + BLK - 1) / BLK, g.ny);
        hipLaunchKernelGGL((k_scalar_import<R>), grid, dim3(BLK), 0, c->s_compute, c->stage.as<const R>(), sc.lat[0].as<R>(), g);
        hipLaunchKernelGGL((k_scalar_fix<R>), grid, dim3(BLK), 0, c->s_compute, sc.lat[0].as<R>(), sc.lat[1].as<R>(), c->lat[0].as<const R>(), g);
        if (sc.nhold > 0)
            hipLaunchKernelGGL((k_scalar_hold_fix<R>), dim3((sc.nhold + BLK - 1) / BLK), dim3(BLK), 0, c->s_compute, sc.lat[0].as<R>(), sc.lat[1].as<R>(), g,
                               sc.hold_cell, (const R*)sc.hold_val, sc.nhold);
    });
    for (int l = 0; l < 2 && rc == LBM_OK; ++l) rc = periodic_wrap_lattice(c, sc.lat[l].get(), c->s_compute);
    if (rc) return rc;
    sc.cur = 0;
    sc.raw[0] = sc.raw[1] = 1;
    sc.steps = 0;
    if (sc.buoyant) {   // (buoyancy: the plane holds C of the state just set)
        rc = scalar_fill_plane(c, 0);
        if (rc) return rc;
    }
    HIP_TRY(c, hipStreamSynchronize(c->s_compute));
    return LBM_OK;
}

// What the calls on an active scalar start with.
static int scalar_ready(lbm_ctx* c, const char* call) {
    if (!c->scalar.active) return fail(c, LBM_ERR_STATE, std::string(call) + ": no scalar is active (lbm_scalar_begin)");
    HIP_TRY(c, hipSetDevice(c->p.device));
    return sync_all(c);
}
// the lattice whose arriving populations the last scalar step started from (the one-step lag of lbm_get_fields): lat[cur ^ 1] after a step
static int scalar_lagged(const ScalarState& sc) { return sc.steps > 0 ? sc.cur ^ 1 : sc.cur; }

template <typename R>
static std::vector<char> rounded(const std::vector<double>& v) {
    std::vector<char> out(v.size() * sizeof(R));
    for (size_t i = 0; i < v.size(); ++i) ((R*)out.data())[i] = (R)v[i];
    return out;
}
}  // namespace lbmhost

using namespace lbmhost;

extern "C" {

int lbm_scalar_begin(lbm_ctx* c, double diffusivity, double magic, const double* c0, const uint8_t* dirichlet, const double* wall_value,
                     const double* hold_value) {
    if (!c) return LBM_ERR_INVALID;
    if (c->p.semantics != LBM_SEM_BOUNCE_BACK_SOLID)
        return fail(c, LBM_ERR_STATE, "lbm_scalar_begin: the scalar runs on obstacle lattices only (create the context with semantics = "
                                      "LBM_SEM_BOUNCE_BACK_SOLID; an all-fluid mask is fine)");
    if (is_slab(c->plan)) return fail(c, LBM_ERR_STATE, "lbm_scalar_begin: the scalar knows no slabs (a lone lattice only)");
    if (c->plan.batch > 1) return fail(c, LBM_ERR_STATE, "lbm_scalar_begin: the scalar knows no batches (batch = 1 only)");
    if (c->plan.solid_tiles)
        return fail(c, LBM_ERR_STATE, "lbm_scalar_begin: the scalar follows single steps (LBM_FLAG_SOLID_TILES runs several per launch; create the "
                                      "context without the flag)");
    if (!std::isfinite(diffusivity) || diffusivity <= 0.0) return fail(c, LBM_ERR_INVALID, "lbm_scalar_begin: the diffusivity must be finite and > 0");
    if (!std::isfinite(magic) || magic <= 0.0) return fail(c, LBM_ERR_INVALID, "lbm_scalar_begin: the TRT product (magic) must be finite and > 0");
    if (!c0) return fail(c, LBM_ERR_INVALID, "lbm_scalar_begin: the initial values are missing (c0 is NULL)");
    const int nx = c->plan.geo.nx, ny = c->plan.geo.ny;
    const size_t n = (size_t)nx * ny;
    const std::vector<uint8_t>& mask = c->obs.mask;
    const std::vector<uint8_t>& hold = c->obs.hold;   // (the user's; the image cells hold what the wrap gives them)
    for (size_t i = 0; i < n; ++i) {
        if (!mask[i] && !std::isfinite(c0[i])) return fail(c, LBM_ERR_INVALID, "lbm_scalar_begin: the initial value of cell " + std::to_string(i) + " is not finite");
        if (dirichlet && dirichlet[i]) {
            if (!mask[i])
                return fail(c, LBM_ERR_INVALID, "lbm_scalar_begin: Dirichlet cell " + std::to_string(i) + " is not a solid cell (a wall value lives on solid cells)");
            if (!wall_value || !std::isfinite(wall_value[i]))
                return fail(c, LBM_ERR_INVALID, "lbm_scalar_begin: the wall value of Dirichlet cell " + std::to_string(i) + " is missing or not finite");
        }
        if (hold_value && !hold.empty() && hold[i] && !std::isfinite(hold_value[i]))
            return fail(c, LBM_ERR_INVALID, "lbm_scalar_begin: the hold value of hold cell " + std::to_string(i) + " is not finite");
    }
    HIP_TRY(c, hipSetDevice(c->p.device));
    int rc = sync_all(c);
    if (rc == LBM_OK) rc = ensure_field_stage(c);
    if (rc) return rc;
    const bool f32 = c->plan.es == 4;
    // everything is built aside; the context's scalar changes only at the end
    ScalarState next;
    next.D = diffusivity;
    next.magic = magic;
    for (int l = 0; l < 2; ++l) {
        rc = alloc_ok(c, next.lat[l].alloc(c->plan.lat_bytes, "scalar lattice"));
        if (rc) return rc;
        HIP_TRY(c, hipMemsetAsync(next.lat[l].get(), 0, c->plan.lat_bytes, c->s_compute));   // (ghost cells are read, never used: numbers)
    }
    {   // the wall values
        const ScalarWalls t = scalar_wall_table(mask.data(), c->obs.hold_or_null(), dirichlet, wall_value, nx, ny);
        const std::vector<char> val = f32 ? rounded<float>(t.val) : rounded<double>(t.val);
        Pack<HipMem> p = upload<HipMem>({{t.cell_row.data(), t.cell_row.size() * sizeof(int32_t)}, {val.data(), val.size()}, {t.bits.data(), t.bits.size()}},
                                        "scalar wall values");
        if (!p.err.empty()) return fail(c, p.no_memory ? LBM_ERR_NOMEM : LBM_ERR_HIP, p.err);
        next.cell_row = p.at<const int32_t>(0);
        next.val = p.at<const void>(1);
        next.bits = p.at<const uint8_t>(2);
        next.walls = std::move(p.buf);
    }
    if (!hold.empty()) {   // the user's hold cells, in the order of hold_f: x, then y
        std::vector<int32_t> cell;
        std::vector<double> vals;
        size_t at = 0;
        for (size_t i = 0; i < n; ++i)
            if (hold[i]) {
                double g[9];
                scalar_hold_values(c->obs.hold_f.data() + at, hold_value ? hold_value[i] : c0[i], g);
                at += Q;
                cell.push_back((int32_t)(i / ny));
                cell.push_back((int32_t)(i % ny));
                vals.insert(vals.end(), g, g + 9);
            }
        const std::vector<char> val = f32 ? rounded<float>(vals) : rounded<double>(vals);
        Pack<HipMem> p = upload<HipMem>({{cell.data(), cell.size() * sizeof(int32_t)}, {val.data(), val.size()}}, "scalar hold cells");
        if (!p.err.empty()) return fail(c, p.no_memory ? LBM_ERR_NOMEM : LBM_ERR_HIP, p.err);
        next.hold_cell = p.at<const int32_t>(0);
        next.hold_val = p.at<const void>(1);
        next.nhold = (int)(cell.size() / 2);
        next.holds = std::move(p.buf);
    }
    // the initial state: plain populations w_k C0, the weight and C0 rounded to the lattice type, one product in it
    std::vector<char> g0(Q * n * (size_t)c->plan.es);
    for (int k = 0; k < Q; ++k)
        for (size_t i = 0; i < n; ++i) {
            if (f32) ((float*)g0.data())[k * n + i] = mask[i] ? 0.0f : (float)scalar_weight(k) * (float)c0[i];
            else ((double*)g0.data())[k * n + i] = mask[i] ? 0.0 : scalar_weight(k) * c0[i];
        }
    rc = host_to_stage(c, g0.data(), c->p.dtype, Q);
    if (rc) return rc;
    if (c->scalar.buoyant) {   // (replacing a buoyant scalar: the buoyancy stays, its plane is filled from the new state below)
        next.buoyant = true;
        for (int i = 0; i < 3; ++i) next.buoy[i] = c->scalar.buoy[i];
        next.cp = std::move(c->scalar.cp);
    }
    c->scalar = std::move(next);
    c->scalar.active = true;
    rc = scalar_from_stage(c);
    if (rc) scalar_free(c);
    return rc;
}

int lbm_scalar_end(lbm_ctx* c) {
    if (!c) return LBM_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->p.device));
    const int rc = sync_all(c);
    if (rc) return rc;
    scalar_free(c);
    return LBM_OK;
}

int lbm_set_buoyancy(lbm_ctx* c, double ax, double ay, double c_ref) {
    if (!c) return LBM_ERR_INVALID;
    if (!std::isfinite(ax) || !std::isfinite(ay) || !std::isfinite(c_ref))
        return fail(c, LBM_ERR_INVALID, "lbm_set_buoyancy: the acceleration and the reference value must be finite");
    int rc = need_one_step(c, "lbm_set_buoyancy", "adds no force");   // (such a context cannot have a scalar either: the reason that helps comes first)
    if (rc) return rc;
    if (!c->scalar.active) return fail(c, LBM_ERR_STATE, "lbm_set_buoyancy: no scalar is active (lbm_scalar_begin first: the buoyancy acts through its C)");
    const bool on = ax != 0.0 || ay != 0.0;
    if (on && c->obs.shaped.base)
        return fail(c, LBM_ERR_STATE, "lbm_set_buoyancy: a shape is set (the shaped kernels add no buoyancy; clear the shape with "
                                      "lbm_set_solid_shape(NULL) first)");
    if (on && c->subgrid > 0.0)
        return fail(c, LBM_ERR_STATE, "lbm_set_buoyancy: a sub-grid constant is set (a buoyant flow with the closure needs an eddy diffusivity for the "
                                      "scalar, which there is none; clear it with lbm_set_subgrid(c, 0) first)");
    if (on && c->relax_field())
        return fail(c, LBM_ERR_STATE, "lbm_set_buoyancy: a relaxation field is set (the buoyant kernels read no rate planes: every such pairing is one more "
                                      "set of kernel twins; clear it with lbm_set_relaxation_field(c, NULL, NULL) first)");
    if (on && c->rheology())
        return fail(c, LBM_ERR_STATE, "lbm_set_buoyancy: a rheology table is set (the buoyant kernels read no rheology table: every such pairing is one "
                                      "more set of kernel twins; clear it with lbm_set_rheology(c, NULL, NULL, 0, 0) first)");
    HIP_TRY(c, hipSetDevice(c->p.device));
    rc = sync_all(c);
    if (rc) return rc;
    ScalarState& sc = c->scalar;
    if (!on) {   // the launches, the bits and the describe text of a context without it
        sc.buoyant = false;
        sc.buoy[0] = sc.buoy[1] = sc.buoy[2] = 0.0;
        sc.cp = DevBuf{};
        return LBM_OK;
    }
    if (!sc.cp) {
        DevBuf plane;
        const size_t bytes = (size_t)buoy_elems(c->plan.geo) * (size_t)c->plan.es;   // (rows of pitch elements: not Geo::plane, one row in the rows layout)
        rc = alloc_ok(c, plane.alloc(bytes, "buoyancy plane"));
        if (rc) return rc;
        HIP_TRY(c, hipMemsetAsync(plane.get(), 0, bytes, c->s_compute));   // (ghost cells: never read)
        sc.cp = std::move(plane);
        rc = scalar_fill_plane(c, scalar_lagged(sc));
        if (rc == LBM_OK && hipStreamSynchronize(c->s_compute) != hipSuccess) rc = fail(c, LBM_ERR_HIP, "lbm_set_buoyancy: filling the plane failed");
        if (rc) {
            sc.cp = DevBuf{};
            return rc;
        }
    }
    sc.buoyant = true;
    sc.buoy[0] = ax;
    sc.buoy[1] = ay;
    sc.buoy[2] = c_ref;
    return LBM_OK;
}

int lbm_set_buoyancy_plane(lbm_ctx* c, const void* conc_host, int host_dtype) {
    if (!c || !conc_host || (host_dtype != LBM_F32 && host_dtype != LBM_F64)) return fail(c, LBM_ERR_INVALID, "lbm_set_buoyancy_plane: bad argument");
    if (!c->scalar.buoyant) return fail(c, LBM_ERR_STATE, "lbm_set_buoyancy_plane: no buoyancy is set (lbm_set_buoyancy)");
    int rc = scalar_ready(c, "lbm_set_buoyancy_plane");
    if (rc == LBM_OK) rc = ensure_field_stage(c);
    if (rc == LBM_OK) rc = host_to_stage(c, conc_host, host_dtype, 1);
    if (rc) return rc;
    const Geo& g = c->plan.geo;
    rc = launch_variant(c, [&](auto v) {
        using R = typename decltype(v)::R;
        hipLaunchKernelGGL((k_scalar_plane_import<R>), dim3((g.nx + BLK - 1) / BLK, g.ny), dim3(BLK), 0, c->s_compute, c->stage.as<const R>(),
                           c->scalar.cp.as<R>(), g);
    });
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->s_compute));
    return LBM_OK;
}

int lbm_get_buoyancy(lbm_ctx* c, double* ax_out, double* ay_out, double* c_ref_out) {
    if (!c) return LBM_ERR_INVALID;
    const ScalarState& sc = c->scalar;
    if (ax_out) *ax_out = sc.buoyant ? sc.buoy[0] : 0.0;
    if (ay_out) *ay_out = sc.buoyant ? sc.buoy[1] : 0.0;
    if (c_ref_out) *c_ref_out = sc.buoyant ? sc.buoy[2] : 0.0;
    return sc.buoyant ? 1 : 0;
}

int lbm_scalar_active(const lbm_ctx* c, double* diffusivity_out, double* magic_out) {
    if (!c) return LBM_ERR_INVALID;
    if (!c->scalar.active) return 0;
    if (diffusivity_out) *diffusivity_out = c->scalar.D;
    if (magic_out) *magic_out = c->scalar.magic;
    return 1;
}

int lbm_scalar_set_state(lbm_ctx* c, const void* g_host, int host_dtype) {
    if (!c || !g_host || (host_dtype != LBM_F32 && host_dtype != LBM_F64)) return fail(c, LBM_ERR_INVALID, "lbm_scalar_set_state: bad argument");
    int rc = scalar_ready(c, "lbm_scalar_set_state");
    if (rc == LBM_OK) rc = ensure_field_stage(c);
    if (rc == LBM_OK) rc = host_to_stage(c, g_host, host_dtype, Q);
    return rc ? rc : scalar_from_stage(c);
}

// which: the scalar lattice; raw: its flag, or 1 for the stored values as they are
static int scalar_export(lbm_ctx* c, int which, int raw, bool want_g, bool want_c) {
    const ScalarState& sc = c->scalar;
    const Geo& g = c->plan.geo;
    const size_t n = (size_t)g.nx * g.ny;
    return launch_variant(c, [&](auto v) {
        using R = typename decltype(v)::R;
        R* st = c->stage.as<R>();
        hipLaunchKernelGGL((k_scalar_export<R>), dim3((g.nx + BLK - 1) / BLK, g.ny), dim3(BLK), 0, c->s_compute, sc.lat[which].as<const R>(),
                           c->lat[0].as<const R>(), g, scalar_arg<R>(c), raw, want_g ? st : (R*)nullptr, want_c ? st + Q * n : (R*)nullptr);
    });
}

int lbm_scalar_get(lbm_ctx* c, void* conc_out, void* g_out, int host_dtype) {
    if (!c || (host_dtype != LBM_F32 && host_dtype != LBM_F64)) return fail(c, LBM_ERR_INVALID, "lbm_scalar_get: bad argument");
    int rc = scalar_ready(c, "lbm_scalar_get");
    if (rc == LBM_OK) rc = ensure_field_stage(c);
    if (rc) return rc;
    const ScalarState& sc = c->scalar;
    const size_t n = (size_t)c->plan.geo.nx * c->plan.geo.ny;
    if (g_out) rc = scalar_export(c, sc.cur, sc.raw[sc.cur], true, false);
    if (rc == LBM_OK && conc_out) rc = scalar_export(c, scalar_lagged(sc), sc.raw[scalar_lagged(sc)], false, true);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->s_compute));
    if (g_out) rc = stage_to_host(c, c->stage.get(), g_out, host_dtype, Q);
    if (rc == LBM_OK && conc_out) rc = stage_to_host(c, c->stage.as<const char>() + Q * n * c->plan.es, conc_out, host_dtype, 1);
    return rc;
}

int lbm_scalar_get_stored(lbm_ctx* c, void* g_out, int host_dtype) {
    if (!c || !g_out || (host_dtype != LBM_F32 && host_dtype != LBM_F64)) return fail(c, LBM_ERR_INVALID, "lbm_scalar_get_stored: bad argument");
    int rc = scalar_ready(c, "lbm_scalar_get_stored");
    if (rc == LBM_OK) rc = ensure_field_stage(c);
    if (rc == LBM_OK) rc = scalar_export(c, c->scalar.cur, 1, true, false);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->s_compute));
    return stage_to_host(c, c->stage.get(), g_out, host_dtype, Q);
}

int lbm_scalar_totals(lbm_ctx* c, lbm_scalar_record* out) {
    if (!c || !out) return fail(c, LBM_ERR_INVALID, "lbm_scalar_totals: bad argument");
    int rc = scalar_ready(c, "lbm_scalar_totals");
    if (rc) return rc;
    ScalarState& sc = c->scalar;
    rc = alloc_ok(c, sc.part.ensure(((size_t)SCALAR_BLOCKS * ScalarTotAcc::VALS + 5) * sizeof(double), "scalar totals"));
    if (rc) return rc;
    double* part = sc.part.as<double>();
    double* rec = part + (size_t)SCALAR_BLOCKS * ScalarTotAcc::VALS;
    const int which = scalar_lagged(sc);
    rc = launch_variant(c, [&](auto v) {
        using R = typename decltype(v)::R;
        hipLaunchKernelGGL((k_scalar_totals<R>), dim3(SCALAR_BLOCKS), dim3(BLK), 0, c->s_compute, sc.lat[which].as<const R>(), c->lat[0].as<const R>(), c->plan.geo,
                           scalar_arg<R>(c), sc.raw[which], c->obs.per_x ? 1 : 0, c->obs.per_y ? 1 : 0, part);
        hipLaunchKernelGGL(k_scalar_totals_final, dim3(1), dim3(RED_WAVE), 0, c->s_compute, (const double*)part, SCALAR_BLOCKS, (double)sc.steps, rec);
    });
    if (rc) return rc;
    return records_to_host(c, rec, sizeof(lbm_scalar_record), out);
}

int lbm_scalar_flux(lbm_ctx* c, lbm_scalar_flux_record* out) {
    if (!c || !out) return fail(c, LBM_ERR_INVALID, "lbm_scalar_flux: bad argument");
    int rc = scalar_ready(c, "lbm_scalar_flux");
    if (rc) return rc;
    ScalarState& sc = c->scalar;
    if (sc.steps == 0 || sc.raw[sc.cur])
        return fail(c, LBM_ERR_STATE, "lbm_scalar_flux: no scalar step yet (the lattice holds post-collision populations after one)");
    const BodyTables& t = c->obs.body;
    const int nbodies = c->obs.nbodies;
    rc = alloc_ok(c, sc.part.ensure(((size_t)t.maxchunks * ScalarFluxAcc::VALS + (size_t)nbodies * 3) * sizeof(double), "scalar flux"));
    if (rc) return rc;
    double* part = sc.part.as<double>();
    double* rec = part + (size_t)t.maxchunks * ScalarFluxAcc::VALS;
    rc = launch_variant(c, [&](auto v) {
        using R = typename decltype(v)::R;
        hipLaunchKernelGGL((k_scalar_flux<R>), dim3(t.maxchunks), dim3(BLK), 0, c->s_compute, sc.lat[sc.cur].as<const R>(), c->plan.geo, scalar_arg<R>(c), t.links,
                           t.chunks, part);
        hipLaunchKernelGGL(k_scalar_flux_final, dim3(nbodies), dim3(RED_WAVE), 0, c->s_compute, (const double*)part, t.first, (double)sc.steps, rec);
    });
    if (rc) return rc;
    return records_to_host(c, rec, (size_t)nbodies * sizeof(lbm_scalar_flux_record), out);
}
}  // extern "C"
