// lbm_sampling.hip -- liblbm_hip.so: what the samplers (time statistics, run monitor, field residual) share -- the record series, the
// prologue of the lbm_*_sample calls, the automatic samples of the step loop (schedule: lbm_schedule.hpp) -- and the time statistics
// (lbm_stats_*) of the C ABI declared in include/lbm.h.  gfx950 only.  DESIGN.md 2.6, 2.7.
#include "lbm_host.hpp"

namespace lbmhost {

// ---- a series of records on the device ----
// Room for `capacity` samples of batch records each; s is off.
int series_alloc(lbm_ctx* c, Series& s, size_t record_bytes, int capacity, const char* what) {
    const size_t sample_bytes = record_bytes * c->plan.batch;
    const int rc = alloc_ok(c, s.dev.alloc((size_t)capacity * sample_bytes, what));
    if (rc) return rc;
    s.sample_bytes = sample_bytes;
    s.capacity = capacity;
    return LBM_OK;
}
// The slot of the next sample (the caller counts it once it is enqueued), or null: the buffer is full, the sample is counted as dropped.
void* series_slot(Series& s) {
    if (s.count < s.capacity) return s.dev.as<char>() + (size_t)s.count * s.sample_bytes;
    ++s.dropped;
    return nullptr;
}
// lbm_monitor_read / lbm_residual_read / lbm_force_read.  series(c): the context's series, asked for once c is known not to be null.
int series_read(lbm_ctx* c, const Series* (*series)(const lbm_ctx*), const char* call, void* records_out, int max_records, long long* count,
                long long* dropped) {
    if (!c || max_records < 0 || (max_records > 0 && !records_out)) return fail(c, LBM_ERR_INVALID, std::string(call) + ": bad argument");
    const Series& s = *series(c);
    if (!s.dev) return fail(c, LBM_ERR_STATE, std::string(call) + ": no series is on (the matching _begin call)");
    HIP_TRY(c, hipSetDevice(c->p.device));
    const int rc = sync_all(c);
    if (rc) return rc;
    if (count) *count = s.count;
    if (dropped) *dropped = s.dropped;
    const long long n = std::min<long long>(s.count, max_records);
    if (n > 0) HIP_TRY(c, hipMemcpy(records_out, s.dev.get(), (size_t)n * s.sample_bytes, hipMemcpyDeviceToHost));
    return LBM_OK;
}

// ---- the three samplers ----
// The prologue of lbm_*_begin.  (Automatic sampling cuts the units of lbm_step, which a slab's neighbours would have to cut alike.)
int sampler_begin(lbm_ctx* c, int sampler, int every) {
    if (every > 0 && is_slab(c->plan))
        return fail(c, LBM_ERR_STATE, std::string(SAMPLER_CALLS[sampler]) + "_begin: no automatic sampling on a slab (every = 0, and " + SAMPLER_CALLS[sampler] +
                                          "_sample at the same step counts on every slab)");
    HIP_TRY(c, hipSetDevice(c->p.device));
    return sync_all(c);
}

// One sample of the time statistics from lat[which] (the lattice whose gathered populations are the state the sampled iteration
// starts from), on the compute stream.
static int stats_accumulate(lbm_ctx* c, int which) {
    constexpr long long STATS_BLOCKS = 2048;   // grid-stride beyond that (a pure streaming kernel)
    const long long npairs = (long long)c->plan.geo.ny * ((c->plan.geo.nx + 1) / 2);
    const int blocks = (int)std::min<long long>((npairs + BLK - 1) / BLK, STATS_BLOCKS);
    const int rc = launch_variant(c, [&](auto v) {
        using VT = decltype(v);
        using R = typename VT::R;
        with_fields<VT>(c, which, [&](auto f) {
            hipLaunchKernelGGL((k_stats_accumulate<R, VT::SEM, coll_is_prom(VT::COLL), decltype(f)::SHAPED>), dim3(blocks, 1, c->plan.batch), dim3(BLK), 0,
                               c->s_compute, f, c->stats_dev.as<double>());
        });
    });
    if (rc) return rc;
    ++c->stats_count;
    return LBM_OK;
}

// one sample of step count `step` from lat[which], on the compute stream
static int sample_from(lbm_ctx* c, int sampler, int which, long long step) {
    switch (sampler) {
        case SMP_STATS: return stats_accumulate(c, which);
        case SMP_MONITOR: return monitor_series_sample(c, which, step);
        default: return residual_series_sample(c, which, step);
    }
}

// lbm_stats_sample / lbm_monitor_sample / lbm_residual_sample: a sample of what lbm_get_fields exports now (reader_source: the
// lattice the last iteration started from).  on: the sampler has been begun.
int sample_now(lbm_ctx* c, int sampler, bool on) {
    if (!c) return LBM_ERR_INVALID;
    const std::string stem = SAMPLER_CALLS[sampler];
    if (!on) return fail(c, LBM_ERR_STATE, stem + "_sample: nothing to sample into (" + stem + "_begin)");
    int which = 0;
    const int rc = reader_source(c, stem + "_sample", true, &which);
    if (rc) return rc;
    return sample_from(c, sampler, which, c->nsteps);
}

// Automatic sampling (a lone lattice), before every unit of step_many: the field samples of step count nsteps + 1, from lat[cur] with its raw
// flag -- no lag replay; a call that ends at n - 1 takes the sample of n at the start of the next call.  The samplers keep their own
// schedules; a step count due for several is read by each of them, in the order of the enum.
int sample_if_due(lbm_ctx* c) {
    bool due[NSAMPLERS], any = false;
    for (int i = 0; i < NSAMPLERS; ++i) any |= due[i] = c->sampler[i].due(c->nsteps);
    if (!any) return LBM_OK;
    // (frame work of the last unit on the second stream wrote part of lat[cur], and s_comm must not rewrite it before the sample has read it)
    HipDev dev{c};
    int rc = c->order.one_stream(dev);
    for (int i = 0; i < NSAMPLERS && rc == LBM_OK; ++i)
        if (due[i]) rc = sample_from(c, i, c->cur, c->nsteps + 1);
    if (rc) return rc;
    for (int i = 0; i < NSAMPLERS; ++i)
        if (due[i]) c->sampler[i].advance();
    return LBM_OK;
}

// After every unit of step_many: the force sample of step count nsteps where one is due, from lat[cur], the lattice after nsteps steps.
int sample_after_unit(lbm_ctx* c) {
    Sampler& s = c->sampler[SMP_FORCE];
    if (!s.due(c->nsteps)) return LBM_OK;
    HipDev dev{c};   // (as sample_if_due)
    int rc = c->order.one_stream(dev);
    if (rc == LBM_OK) rc = force_series_sample(c);
    if (rc) return rc;
    s.advance();
    return LBM_OK;
}

// A sampler off: what its _begin allocated freed, its schedule cleared (lbm_*_end, and whatever replaces the state: init / upload /
// destroy).  The caller has synchronised the streams.
void sampler_free(lbm_ctx* c, int sampler) {
    if (sampler == SMP_STATS) {
        c->stats_dev.release();
        c->stats_count = 0;
    } else if (sampler == SMP_MONITOR) {
        c->mon_series = Series{};
    } else if (sampler == SMP_FORCE) {
        c->obs.force_series = Series{};
    } else {
        residual_free(c);
    }
    c->sampler[sampler].clear();
}
// lbm_*_end
int sampler_end(lbm_ctx* c, int sampler) {
    if (!c) return LBM_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->p.device));
    const int rc = sync_all(c);
    if (rc) return rc;
    sampler_free(c, sampler);
    return LBM_OK;
}
}  // namespace lbmhost

using namespace lbmhost;

extern "C" {

int lbm_stats_begin(lbm_ctx* c, int every) {
    if (!c || every < 0) return fail(c, LBM_ERR_INVALID, "lbm_stats_begin: bad argument");
    const int rc = sampler_begin(c, SMP_STATS, every);
    if (rc) return rc;
    const size_t bytes = (size_t)c->plan.batch * 6 * c->plan.geo.ny * (2 * ((c->plan.geo.nx + 1) / 2)) * sizeof(double);
    if (const int bad = alloc_ok(c, c->stats_dev.ensure(bytes, "statistics"))) return bad;
    HIP_TRY(c, hipMemsetAsync(c->stats_dev.get(), 0, bytes, c->s_compute));
    c->stats_count = 0;
    c->sampler[SMP_STATS].arm(c->nsteps, every);
    return LBM_OK;
}

int lbm_stats_sample(lbm_ctx* c) { return sample_now(c, SMP_STATS, c && c->stats_dev); }

int lbm_stats_get(lbm_ctx* c, double* mean_u, double* mean_rho, double* second, long long* count) {
    if (!c) return LBM_ERR_INVALID;
    if (!c->stats_dev) return fail(c, LBM_ERR_STATE, "lbm_stats_get: statistics are off (lbm_stats_begin)");
    HIP_TRY(c, hipSetDevice(c->p.device));
    int rc = sync_all(c);
    if (rc) return rc;
    if (count) *count = c->stats_count;
    if (c->stats_count == 0) return LBM_OK;
    const int nx = c->plan.geo.nx, ny = c->plan.geo.ny, NY = c->plan.geo.NY, y0 = c->plan.geo.y0, nxa = 2 * ((nx + 1) / 2);
    const size_t hn = (size_t)nx * NY, dn = (size_t)ny * nxa;
    const double n = (double)c->stats_count;
    std::vector<double> pl(dn);
    for (int b = 0; b < c->plan.batch; ++b)
        for (int q = 0; q < 6; ++q) {   // device [b][q][y][x] -> host [b][2][x][Y] (u), [b][x][Y] (rho), [b][3][x][Y] (second moments)
            double* dst = q < 2 ? (mean_u ? mean_u + ((size_t)b * 2 + q) * hn : nullptr)
                        : q == 2 ? (mean_rho ? mean_rho + (size_t)b * hn : nullptr)
                                 : (second ? second + ((size_t)b * 3 + q - 3) * hn : nullptr);
            if (!dst) continue;
            HIP_TRY(c, hipMemcpy(pl.data(), c->stats_dev.as<double>() + ((size_t)b * 6 + q) * dn, dn * sizeof(double), hipMemcpyDeviceToHost));
            for (int x = 0; x < nx; ++x)
                for (int y = 0; y < ny; ++y) dst[(size_t)x * NY + y0 + y] = pl[(size_t)y * nxa + x] / n;
        }
    return LBM_OK;
}

int lbm_stats_end(lbm_ctx* c) { return sampler_end(c, SMP_STATS); }
}  // extern "C"
