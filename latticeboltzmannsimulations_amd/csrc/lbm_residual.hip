// lbm_residual.hip -- liblbm_hip.so: the field residual (lbm_residual_begin / _sample / _read / _end) of the C ABI declared in
// include/lbm.h: the change of the sampled u and rho between two consecutive samples, reduced on the device to one record per
// lattice; the previous sample stays on the device as a snapshot.  The kernels are in lbm_residual.hpp; the automatic samples are
// taken by sample_if_due (lbm_sampling.hip) through residual_series_sample.  gfx950 only.  DESIGN.md 2.9.
#include "lbm_host.hpp"
#include "lbm_residual.hpp"

namespace lbmhost {

constexpr int RES_BLOCKS = 1024;   // partial results per lattice (as the monitor's pass)

static_assert(sizeof(lbm_residual_record) == (2 + RES_VALS) * sizeof(double), "record layout");

// the snapshot's element: what lbm_get_fields(host_dtype) hands out
static bool snap_is_f32(const lbm_ctx* c) { return c->p.dtype == LBM_F32 || c->res_host_dtype == LBM_F32; }
static long long snap_groups(const lbm_ctx* c) {
    const int cpl = snap_is_f32(c) ? ResGroup<float>::CPL : ResGroup<double>::CPL;
    return (long long)c->plan.geo.ny * ((c->plan.geo.nx + cpl - 1) / cpl);
}
static int res_blocks(const lbm_ctx* c) { return (int)std::min<long long>((snap_groups(c) + BLK - 1) / BLK, RES_BLOCKS); }

// One sample of lat[which] (the lattice whose gathered populations are the state the sampled iteration starts from), on the compute
// stream: the pass that compares with the snapshot and replaces it; then, unless this is the series' first sample or its buffer is
// full, the final pass into the series' next slot.
int residual_series_sample(lbm_ctx* c, int which, long long step) {
    const int blocks = res_blocks(c);
    const int rc = launch_variant(c, [&](auto v) {
        using VT = decltype(v);
        using R = typename VT::R;
        constexpr bool PROM = coll_is_prom(VT::COLL);
        const dim3 grid(blocks, 1, c->plan.batch);
        if constexpr (std::is_same<R, double>::value) {
            if (!snap_is_f32(c)) {
                with_fields<VT>(c, which, [&](auto f) {
                    hipLaunchKernelGGL((k_residual<double, double, VT::SEM, PROM, decltype(f)::SHAPED>), grid, dim3(BLK), 0, c->s_compute, f,
                                       c->res_snap.as<double>(), c->res_part.as<double>());
                });
                return;
            }
        }
        with_fields<VT>(c, which, [&](auto f) {
            hipLaunchKernelGGL((k_residual<R, float, VT::SEM, PROM, decltype(f)::SHAPED>), grid, dim3(BLK), 0, c->s_compute, f, c->res_snap.as<float>(),
                               c->res_part.as<double>());
        });
    });
    if (rc) return rc;
    const long long prev = c->res_prev;
    c->res_prev = step;
    if (prev < 0) return LBM_OK;   // the first sample only fills the snapshot
    void* slot = series_slot(c->res_series);
    if (!slot) return LBM_OK;
    hipLaunchKernelGGL(k_residual_final, dim3(c->plan.batch), dim3(RED_WAVE), 0, c->s_compute, c->res_part.as<const double>(), blocks, (double)step,
                       (double)prev, (double*)slot);
    HIP_TRY(c, hipGetLastError());
    ++c->res_series.count;
    return LBM_OK;
}

// The residual off (sampler_free): what lbm_residual_begin allocated, and no snapshot.
void residual_free(lbm_ctx* c) {
    c->res_snap.release();
    c->res_part.release();
    c->res_series = Series{};
    c->res_prev = -1;
}
}  // namespace lbmhost

using namespace lbmhost;

extern "C" {

int lbm_residual_begin(lbm_ctx* c, int host_dtype, int every, int capacity) {
    if (!c || (host_dtype != LBM_F32 && host_dtype != LBM_F64) || every < 0 || capacity < 1)
        return fail(c, LBM_ERR_INVALID, "lbm_residual_begin: bad argument");
    int rc = sampler_begin(c, SMP_RESIDUAL, every);
    if (rc) return rc;
    sampler_free(c, SMP_RESIDUAL);
    c->res_host_dtype = host_dtype;
    const size_t snap_bytes = (size_t)c->plan.batch * 3 * (size_t)snap_groups(c) * 16;
    const size_t part_bytes = (size_t)c->plan.batch * RES_BLOCKS * RES_VALS * sizeof(double);
    rc = alloc_ok(c, c->res_snap.alloc(snap_bytes, "residual"));
    if (rc == LBM_OK) rc = alloc_ok(c, c->res_part.alloc(part_bytes, "residual"));
    if (rc == LBM_OK) rc = series_alloc(c, c->res_series, sizeof(lbm_residual_record), capacity, "residual series");
    if (rc) {
        sampler_free(c, SMP_RESIDUAL);
        return rc;
    }
    // (the first sample reads the snapshot like every other and discards what it reduces: give it defined values)
    HIP_TRY(c, hipMemsetAsync(c->res_snap.get(), 0, snap_bytes, c->s_compute));
    c->sampler[SMP_RESIDUAL].arm(c->nsteps, every);
    return LBM_OK;
}

int lbm_residual_sample(lbm_ctx* c) { return sample_now(c, SMP_RESIDUAL, c && c->res_snap); }

int lbm_residual_read(lbm_ctx* c, lbm_residual_record* records_out, int max_records, long long* count, long long* dropped) {
    return series_read(c, [](const lbm_ctx* x) { return &x->res_series; }, "lbm_residual_read", records_out, max_records, count, dropped);
}

int lbm_residual_end(lbm_ctx* c) { return sampler_end(c, SMP_RESIDUAL); }
}  // extern "C"
