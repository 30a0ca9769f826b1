// lbm_monitor.hip -- liblbm_hip.so: the run monitor (lbm_monitor, lbm_monitor_begin / _sample / _read / _end) and the export of one
// column and one row (lbm_get_lines) of the C ABI declared in include/lbm.h.  The kernels are in lbm_monitor.hpp; the automatic
// samples of a series are taken by sample_if_due (lbm_sampling.hip) through monitor_series_sample.  gfx950 only.  DESIGN.md 2.7.
#include "lbm_host.hpp"
#include "lbm_monitor.hpp"

namespace lbmhost {

constexpr int MON_BLOCKS = 1024;   // partial results per lattice (as lbm_mean_u: enough workgroups to keep every CU's loads in flight)

static_assert(sizeof(lbm_monitor_record) == (1 + MON_VALS + 3 * LBM_MONITOR_MAX_PROBES) * sizeof(double), "record layout");

// "" or what is wrong with the spec for this context
static std::string check_spec(const lbm_ctx* c, const lbm_monitor_spec* s) {
    if (!s) return "null spec";
    if (s->struct_size != (int32_t)sizeof(lbm_monitor_spec)) return "struct_size is not sizeof(lbm_monitor_spec)";
    if (s->host_dtype != LBM_F32 && s->host_dtype != LBM_F64) return "host_dtype must be LBM_F32 or LBM_F64";
    const int nx = c->plan.geo.nx, NY = c->plan.geo.NY;
    auto range = [](int lo, int hi, int n) { return 0 <= lo && lo <= hi && hi <= n; };
    if (!range(s->x_lo, s->x_hi, nx) || !range(s->y_lo, s->y_hi, NY)) return "the window is not inside the lattice";
    if (s->nboxes < 0 || s->nboxes > LBM_MONITOR_MAX_BOXES) return "nboxes must be 0 .. " + std::to_string((int)LBM_MONITOR_MAX_BOXES);
    if (s->nprobes < 0 || s->nprobes > LBM_MONITOR_MAX_PROBES) return "nprobes must be 0 .. " + std::to_string((int)LBM_MONITOR_MAX_PROBES);
    for (int b = 0; b < s->nboxes; ++b)
        if (!range(s->box[b][0], s->box[b][1], nx) || !range(s->box[b][2], s->box[b][3], NY)) return "an exclusion box is not inside the lattice";
    for (int i = 0; i < s->nprobes; ++i)
        if (s->probe[i][0] < 0 || s->probe[i][0] >= nx || s->probe[i][1] < 0 || s->probe[i][1] >= NY) return "a probe is not a cell of the lattice";
    return "";
}

static MonSpec kernel_spec(const lbm_monitor_spec& s) {
    MonSpec m{};
    m.host_f32 = s.host_dtype == LBM_F32;
    m.x_lo = s.x_lo; m.x_hi = s.x_hi; m.y_lo = s.y_lo; m.y_hi = s.y_hi;
    m.nboxes = s.nboxes; m.nprobes = s.nprobes;
    for (int b = 0; b < LBM_MONITOR_MAX_BOXES; ++b)
        for (int j = 0; j < 4; ++j) m.box[b][j] = s.box[b][j];
    for (int i = 0; i < LBM_MONITOR_MAX_PROBES; ++i)
        for (int j = 0; j < 2; ++j) m.probe[i][j] = s.probe[i][j];
    return m;
}

static int mon_blocks(const lbm_ctx* c) {
    const long long n = (long long)c->plan.geo.nx * c->plan.geo.ny;
    return (int)std::min<long long>((n + BLK - 1) / BLK, MON_BLOCKS);
}

// the partial results of one pass, and behind them the records of the one-shot call
static int ensure_partials(lbm_ctx* c) {
    const size_t bytes = (size_t)c->plan.batch * ((size_t)MON_BLOCKS * MON_VALS * sizeof(double) + sizeof(lbm_monitor_record));
    return alloc_ok(c, c->mon_part.ensure(bytes, "monitor"));
}
static lbm_monitor_record* one_shot_records(lbm_ctx* c) {
    return (lbm_monitor_record*)(c->mon_part.as<double>() + (size_t)c->plan.batch * MON_BLOCKS * MON_VALS);
}

// One sample of lat[which] (the lattice whose gathered populations are the state the sampled iteration starts from) into rec[batch],
// on the compute stream: the fused pass, then the final pass.
static int monitor_enqueue(lbm_ctx* c, int which, const lbm_monitor_spec& spec, long long step, lbm_monitor_record* rec) {
    const MonSpec sp = kernel_spec(spec);
    const int blocks = mon_blocks(c);
    const double den = c->p.uLB * c->p.uLB;
    return launch_variant(c, [&](auto v) {
        using VT = decltype(v);
        using R = typename VT::R;
        with_fields<VT>(c, which, [&](auto f) {
            constexpr bool SH = decltype(f)::SHAPED;
            hipLaunchKernelGGL((k_monitor<R, VT::SEM, coll_is_prom(VT::COLL), SH>), dim3(blocks, 1, c->plan.batch), dim3(BLK), 0, c->s_compute, f, den, sp,
                               c->mon_part.as<double>());
            hipLaunchKernelGGL((k_monitor_final<R, VT::SEM, coll_is_prom(VT::COLL), SH>), dim3(c->plan.batch), dim3(RED_WAVE), 0, c->s_compute,
                               c->mon_part.as<const double>(), blocks, f, sp, (double)step, (double*)rec);
        });
    });
}

// The next sample of the series from lat[which], unless its buffer is full.
int monitor_series_sample(lbm_ctx* c, int which, long long step) {
    void* slot = series_slot(c->mon_series);
    if (!slot) return LBM_OK;
    const int rc = monitor_enqueue(c, which, c->mon_spec, step, (lbm_monitor_record*)slot);
    if (rc) return rc;
    ++c->mon_series.count;
    return LBM_OK;
}

}  // namespace lbmhost

using namespace lbmhost;

extern "C" {

int lbm_monitor(lbm_ctx* c, const lbm_monitor_spec* spec, lbm_monitor_record* records_out) {
    if (!c || !spec || !records_out) return fail(c, LBM_ERR_INVALID, "lbm_monitor: bad argument");
    const std::string bad = check_spec(c, spec);
    if (!bad.empty()) return fail(c, LBM_ERR_INVALID, "lbm_monitor: " + bad);
    int which = 0;
    int rc = reader_source(c, "lbm_monitor", true, &which);
    if (rc == LBM_OK) rc = ensure_partials(c);
    if (rc == LBM_OK) rc = monitor_enqueue(c, which, *spec, c->nsteps, one_shot_records(c));
    if (rc) return rc;
    return records_to_host(c, one_shot_records(c), (size_t)c->plan.batch * sizeof(lbm_monitor_record), records_out);
}

int lbm_monitor_begin(lbm_ctx* c, const lbm_monitor_spec* spec, int every, int capacity) {
    if (!c || !spec || every < 0 || capacity < 1) return fail(c, LBM_ERR_INVALID, "lbm_monitor_begin: bad argument");
    const std::string bad = check_spec(c, spec);
    if (!bad.empty()) return fail(c, LBM_ERR_INVALID, "lbm_monitor_begin: " + bad);
    int rc = sampler_begin(c, SMP_MONITOR, every);
    if (rc == LBM_OK) rc = ensure_partials(c);
    if (rc) return rc;
    sampler_free(c, SMP_MONITOR);
    rc = series_alloc(c, c->mon_series, sizeof(lbm_monitor_record), capacity, "monitor series");
    if (rc) return rc;
    c->mon_spec = *spec;
    c->sampler[SMP_MONITOR].arm(c->nsteps, every);
    return LBM_OK;
}

int lbm_monitor_sample(lbm_ctx* c) { return sample_now(c, SMP_MONITOR, c && c->mon_series.dev); }

int lbm_monitor_read(lbm_ctx* c, lbm_monitor_record* records_out, int max_records, long long* count, long long* dropped) {
    return series_read(c, [](const lbm_ctx* x) { return &x->mon_series; }, "lbm_monitor_read", records_out, max_records, count, dropped);
}

int lbm_monitor_end(lbm_ctx* c) { return sampler_end(c, SMP_MONITOR); }

int lbm_get_lines(lbm_ctx* c, int x, int gy, void* col_out, void* row_out, int host_dtype) {
    if (!c || (host_dtype != LBM_F32 && host_dtype != LBM_F64)) return fail(c, LBM_ERR_INVALID, "lbm_get_lines: bad argument");
    const int nx = c->plan.geo.nx, ny = c->plan.geo.ny, NY = c->plan.geo.NY, y0 = c->plan.geo.y0, B = c->plan.batch;
    if (col_out && (x < 0 || x >= nx)) return fail(c, LBM_ERR_INVALID, "lbm_get_lines: column outside the lattice");
    if (row_out && (gy < 0 || gy >= NY)) return fail(c, LBM_ERR_INVALID, "lbm_get_lines: row outside the lattice");
    int which = 0;
    int rc = reader_source(c, "lbm_get_lines", false, &which);
    if (rc) return rc;
    const int cx = col_out ? x : -1;
    const int ly = row_out && gy >= y0 && gy < y0 + ny ? gy - y0 : -1;
    if (cx < 0 && ly < 0) return LBM_OK;
    const size_t per = (size_t)3 * (ny + nx);   // (no more than the fields: 3 (nx + ny) <= 12 nx ny)
    rc = ensure_field_stage(c);
    if (rc) return rc;
    rc = launch_variant(c, [&](auto v) {
        using VT = decltype(v);
        using R = typename VT::R;
        with_fields<VT>(c, which, [&](auto f) {
            hipLaunchKernelGGL((k_export_lines<R, VT::SEM, coll_is_prom(VT::COLL), decltype(f)::SHAPED>), dim3((ny + nx + BLK - 1) / BLK, 1, B), dim3(BLK), 0,
                               c->s_compute, f, cx, ly, c->stage.as<R>());
        });
    });
    if (rc) return rc;
    std::vector<char> tmp(per * B * c->plan.es);
    HIP_TRY(c, hipMemcpyAsync(tmp.data(), c->stage.get(), tmp.size(), hipMemcpyDeviceToHost, c->s_compute));
    HIP_TRY(c, hipStreamSynchronize(c->s_compute));
    // staging of lattice b: [3][ny] of the column, then [3][nx] of the row, in the lattice's type; the host arrays in host_dtype
    auto put = [&](void* dst, size_t di, size_t si) {
        if (c->p.dtype == LBM_F32) {
            const float v = ((const float*)tmp.data())[si];
            if (host_dtype == LBM_F32) ((float*)dst)[di] = v; else ((double*)dst)[di] = (double)v;
        } else {
            const double v = ((const double*)tmp.data())[si];
            if (host_dtype == LBM_F32) ((float*)dst)[di] = (float)v; else ((double*)dst)[di] = v;
        }
    };
    for (int b = 0; b < B; ++b)
        for (int q = 0; q < 3; ++q) {
            if (cx >= 0)
                for (int y = 0; y < ny; ++y) put(col_out, ((size_t)b * 3 + q) * NY + y0 + y, b * per + (size_t)q * ny + y);
            if (ly >= 0)
                for (int i = 0; i < nx; ++i) put(row_out, ((size_t)b * 3 + q) * nx + i, b * per + (size_t)3 * ny + (size_t)q * nx + i);
        }
    return LBM_OK;
}
}  // extern "C"
