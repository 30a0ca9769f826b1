// lbm_topology.hip -- liblbm_hip.so: the flow topology (lbm_topology, lbm_get_stream_function) of the C ABI declared in include/lbm.h:
// stream function, vorticity and the extrema of psi in up to eight windows of the fields lbm_get_fields would return.  The kernels are
// in lbm_topology.hpp.  gfx950 only.  DESIGN.md 2.8.
#include "lbm_host.hpp"
#include "lbm_topology.hpp"

namespace lbmhost {

static_assert(sizeof(lbm_topology_record) == (2 + 8 * LBM_TOPOLOGY_MAX_WINDOWS) * sizeof(double), "record layout");
static_assert(sizeof(lbm_topology_spec) == (4 + 4 * LBM_TOPOLOGY_MAX_WINDOWS) * sizeof(int32_t), "spec layout");

// "" or what is wrong with the spec for this context
static std::string check_spec(const lbm_ctx* c, const lbm_topology_spec* s) {
    if (!s) return "null spec";
    if (s->struct_size != (int32_t)sizeof(lbm_topology_spec)) return "struct_size is not sizeof(lbm_topology_spec)";
    if (s->host_dtype != LBM_F32 && s->host_dtype != LBM_F64) return "host_dtype must be LBM_F32 or LBM_F64";
    if (s->nwindows < 0 || s->nwindows > LBM_TOPOLOGY_MAX_WINDOWS) return "nwindows must be 0 .. " + std::to_string((int)LBM_TOPOLOGY_MAX_WINDOWS);
    const int nx = c->plan.geo.nx, NY = c->plan.geo.NY;
    auto range = [](int lo, int hi, int n) { return 0 <= lo && lo <= hi && hi <= n; };
    for (int i = 0; i < s->nwindows; ++i)
        if (!range(s->window[i][0], s->window[i][1], nx) || !range(s->window[i][2], s->window[i][3], NY)) return "a window is not inside the lattice";
    return "";
}

// The tiles of one lattice: blocks of x, tiles of rows.
struct TopoGrid {
    int nb, nty;
    size_t nwg() const { return (size_t)nb * nty; }
};
static TopoGrid topo_grid(const lbm_ctx* c) {
    return TopoGrid{(c->plan.geo.nx + TOPO_W - 1) / TOPO_W, (c->plan.geo.ny + TOPO_ROWS - 1) / TOPO_ROWS};
}

// Device memory of the record path, per lattice: the block sums / offsets [nb][ny], |psi| at the right wall [ny], the partial results
// [MAX_WINDOWS][nwg][TOPO_PART], the record.  Allocated on first use, kept.
struct TopoBuf {
    double *total, *close, *partial;
    lbm_topology_record* rec;
};
static TopoBuf topo_buf(const lbm_ctx* c) {
    const TopoGrid g = topo_grid(c);
    const size_t B = c->plan.batch, ny = c->plan.geo.ny;
    TopoBuf b;
    b.total = c->topo_part.as<double>();
    b.close = b.total + B * g.nb * ny;
    b.partial = b.close + B * ny;
    b.rec = (lbm_topology_record*)(b.partial + B * LBM_TOPOLOGY_MAX_WINDOWS * g.nwg() * TOPO_PART);
    return b;
}
static int ensure_topo(lbm_ctx* c, bool fields) {
    const TopoGrid g = topo_grid(c);
    const size_t B = c->plan.batch, ny = c->plan.geo.ny;
    const size_t bytes = B * (((size_t)g.nb * ny + ny + LBM_TOPOLOGY_MAX_WINDOWS * g.nwg() * TOPO_PART) * sizeof(double) + sizeof(lbm_topology_record));
    const int rc = alloc_ok(c, c->topo_part.ensure(bytes, "topology"));
    if (rc || !fields) return rc;
    // psi, then omega: [batch][nx][ny] each
    return alloc_ok(c, c->topo_fields.ensure((size_t)2 * B * c->plan.geo.nx * ny * sizeof(double), "stream function"));
}

// psi of lat[which] on the compute stream: block sums, offsets, then the extrema of the spec's windows (and psi itself into psi_out when
// that is not null); with_record: the final pass into the record buffer.
static int topology_enqueue(lbm_ctx* c, int which, const TopoSpec& sp, long long step, double* psi_out, bool with_record) {
    const TopoGrid g = topo_grid(c);
    const TopoBuf b = topo_buf(c);
    const dim3 tiles(g.nb, g.nty, c->plan.batch);
    return launch_variant(c, [&](auto v) {
        using VT = decltype(v);
        using R = typename VT::R;
        constexpr bool PROM = coll_is_prom(VT::COLL);
        with_fields<VT>(c, which, [&](auto f) {
        constexpr bool SH = decltype(f)::SHAPED;
        hipLaunchKernelGGL((k_topo_totals<R, VT::SEM, PROM, SH>), tiles, dim3(BLK), 0, c->s_compute, f, sp.host_f32, b.total);
        hipLaunchKernelGGL(k_topo_offsets, dim3((c->plan.geo.ny + BLK - 1) / BLK, 1, c->plan.batch), dim3(BLK), 0, c->s_compute, b.total, g.nb,
                           c->plan.geo.ny, b.close);
        if (psi_out)
            hipLaunchKernelGGL((k_topo_extrema<R, VT::SEM, PROM, true, SH>), tiles, dim3(BLK), 0, c->s_compute, f, sp, (const double*)b.total, b.partial,
                               psi_out);
        else
            hipLaunchKernelGGL((k_topo_extrema<R, VT::SEM, PROM, false, SH>), tiles, dim3(BLK), 0, c->s_compute, f, sp, (const double*)b.total, b.partial,
                               (double*)nullptr);
        if (with_record)
            hipLaunchKernelGGL((k_topo_final<R, VT::SEM, PROM, SH>), dim3(LBM_TOPOLOGY_MAX_WINDOWS, c->plan.batch), dim3(BLK), 0, c->s_compute,
                               (const double*)b.partial, (int)g.nwg(), (const double*)b.close, f, sp, (double)step, (double*)b.rec);
        });
    });
}

}  // namespace lbmhost

using namespace lbmhost;

extern "C" {

int lbm_topology(lbm_ctx* c, const lbm_topology_spec* spec, lbm_topology_record* records_out) {
    if (!c || !spec || !records_out) return fail(c, LBM_ERR_INVALID, "lbm_topology: bad argument");
    const std::string bad = check_spec(c, spec);
    if (!bad.empty()) return fail(c, LBM_ERR_INVALID, "lbm_topology: " + bad);
    if (is_slab(c->plan)) return fail(c, LBM_ERR_STATE, "lbm_topology: not on a slab (omega needs rows of the neighbour)");
    int which = 0;
    int rc = reader_source(c, "lbm_topology", true, &which);
    if (rc == LBM_OK) rc = ensure_topo(c, false);
    if (rc) return rc;
    TopoSpec sp{};
    sp.host_f32 = spec->host_dtype == LBM_F32;
    sp.nwindows = spec->nwindows;
    for (int i = 0; i < spec->nwindows; ++i)
        for (int j = 0; j < 4; ++j) sp.win[i][j] = spec->window[i][j];
    rc = topology_enqueue(c, which, sp, c->nsteps, nullptr, true);
    if (rc) return rc;
    return records_to_host(c, topo_buf(c).rec, (size_t)c->plan.batch * sizeof(lbm_topology_record), records_out);
}

int lbm_get_stream_function(lbm_ctx* c, double* psi_out, double* omega_out, int host_dtype) {
    if (!c || (host_dtype != LBM_F32 && host_dtype != LBM_F64)) return fail(c, LBM_ERR_INVALID, "lbm_get_stream_function: bad argument");
    if (is_slab(c->plan)) return fail(c, LBM_ERR_STATE, "lbm_get_stream_function: not on a slab (omega needs rows of the neighbour)");
    int which = 0;
    int rc = reader_source(c, "lbm_get_stream_function", true, &which);
    if (rc || (!psi_out && !omega_out)) return rc;
    rc = ensure_topo(c, true);
    if (rc) return rc;
    const int nx = c->plan.geo.nx, ny = c->plan.geo.ny, B = c->plan.batch;
    const size_t n = (size_t)nx * ny;
    double* psi_dev = c->topo_fields.as<double>();
    double* omega_dev = psi_dev + (size_t)B * n;
    if (psi_out) {
        TopoSpec sp{};
        sp.host_f32 = host_dtype == LBM_F32;
        rc = topology_enqueue(c, which, sp, c->nsteps, psi_dev, false);
        if (rc) return rc;
        HIP_TRY(c, hipMemcpyAsync(psi_out, psi_dev, (size_t)B * n * sizeof(double), hipMemcpyDeviceToHost, c->s_compute));
    }
    if (omega_out) {
        // u as the field export stages it (host layout, the lattice's type), then omega from it, one thread per cell
        rc = ensure_field_stage(c);
        if (rc) return rc;
        rc = launch_variant(c, [&](auto v) {
            using VT = decltype(v);
            using R = typename VT::R;
            with_fields<VT>(c, which, [&](auto f) {
                hipLaunchKernelGGL((k_export_macro<R, VT::SEM, coll_is_prom(VT::COLL), decltype(f)::SHAPED>), grid_tiles<R>(c), dim3(BLK), 0, c->s_compute, f,
                                   c->stage.as<R>());
            });
            hipLaunchKernelGGL((k_topo_omega<R>), dim3((unsigned)((n + BLK - 1) / BLK), 1, B), dim3(BLK), 0, c->s_compute, c->stage.as<const R>(), nx, ny,
                               (int)(host_dtype == LBM_F32), omega_dev);
        });
        if (rc) return rc;
        HIP_TRY(c, hipMemcpyAsync(omega_out, omega_dev, (size_t)B * n * sizeof(double), hipMemcpyDeviceToHost, c->s_compute));
    }
    HIP_TRY(c, hipStreamSynchronize(c->s_compute));
    return LBM_OK;
}
}  // extern "C"
