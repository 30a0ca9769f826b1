// lbm_hip.hip -- liblbm_hip.so: context life cycle, state upload, field export (with the prologue and the epilogue that every reader of
// the exported state shares) and the bandwidth / FMA probes of the C ABI declared in include/lbm.h (the other host units are listed in lbm_host.hpp, which holds the shared declarations).
// gfx950 only.  See DESIGN.md for the data layout and the per-kernel roofline notes.
#include "lbm_host.hpp"

namespace lbmhost {

// (not a template: defined in this translation unit only)
__global__ __launch_bounds__(BLK) void k_copy16(const uint4* __restrict__ a, uint4* __restrict__ b, size_t n) {
    size_t i = (size_t)blockIdx.x * BLK + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * BLK;
    for (; i < n; i += stride) b[i] = a[i];
}

// fp32 fused multiply-add rate probe (lbm_fma_rate): 16 independent packed FMAs per thread and iteration, nothing else
__global__ __launch_bounds__(BLK) void k_fma_burn(float* __restrict__ sink, int iters, float seed) {
    typedef float f2 __attribute__((ext_vector_type(2)));
    f2 a[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = f2{seed + (float)i, seed - (float)threadIdx.x * 1e-6f};
    const f2 m = f2{0.999f, 1.001f}, b = f2{1e-3f, -1e-3f};
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int i = 0; i < 8; ++i) a[i] = __builtin_elementwise_fma(a[i], m, b);
    }
    f2 t = a[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) t += a[i];
    if (t.x + t.y == 123456.789f) sink[blockIdx.x * BLK + threadIdx.x] = t.x;   // (never true in practice: keeps the loop alive)
}

// out[z] = scale * (partial[z * nper + 0] + partial[z * nper + 1] + ...), added in index order by one thread per lattice
__global__ __launch_bounds__(BLK) void k_reduce_final(const double* __restrict__ partial, int nper, int nlat, double scale, double* __restrict__ out) {
    const int z = blockIdx.x * BLK + threadIdx.x;
    if (z >= nlat) return;
    double a = 0.0;
    for (int i = 0; i < nper; ++i) a += partial[(size_t)z * nper + i];
    out[z] = scale * a;
}

int ensure_stage(lbm_ctx* c, size_t bytes) { return alloc_ok(c, c->stage.ensure(bytes, "staging")); }
// the staging buffer of the state upload and of every field export: twelve planes' worth per lattice (the populations take nine)
int ensure_field_stage(lbm_ctx* c) { return ensure_stage(c, (size_t)12 * c->plan.geo.nx * c->plan.geo.ny * c->plan.es * c->plan.batch); }
int sync_all(lbm_ctx* c) {
    if (!spin_until_ready([&] { return hipStreamQuery(c->s_compute); })) HIP_TRY(c, hipStreamSynchronize(c->s_compute));
    if (!spin_until_ready([&] { return hipStreamQuery(c->s_comm); })) HIP_TRY(c, hipStreamSynchronize(c->s_comm));
    return LBM_OK;
}

// What every reader of the exported state starts with: the refusal before the first step (needs_step: the calls that have one), the
// device, both streams idle, then the lattice the last iteration started from (prev_lattice: still intact after a single step,
// recomputed after a multi-step unit) -- *which is what fields_of takes.
int reader_source(lbm_ctx* c, const std::string& call, bool needs_step, int* which) {
    if (needs_step && c->nsteps == 0) return fail(c, LBM_ERR_STATE, call + ": no step yet (the fields of an iteration exist after it)");
    HIP_TRY(c, hipSetDevice(c->p.device));
    const int rc = sync_all(c);
    return rc ? rc : prev_lattice(c, which);
}
// ... and what the one-shot calls end with: the records enqueued on the compute stream, on the host.
int records_to_host(lbm_ctx* c, const void* dev, size_t bytes, void* out) {
    HIP_TRY(c, hipMemcpyAsync(out, dev, bytes, hipMemcpyDeviceToHost, c->s_compute));
    HIP_TRY(c, hipStreamSynchronize(c->s_compute));
    return LBM_OK;
}

// host <-> staging helpers.  Host arrays are whole-lattice [planes][nx][NY]; staging is
// [planes][nx][ny_local].
template <typename D, typename S>
void convert_rows(D* dst, const S* src, size_t planes_nx, int ny, int NY, int y0, bool to_host) {
    for (size_t r = 0; r < planes_nx; ++r)
        for (int y = 0; y < ny; ++y) {
            if (to_host) dst[r * NY + y0 + y] = (D)src[r * ny + y];
            else dst[r * ny + y] = (D)src[r * NY + y0 + y];
        }
}

int host_to_stage(lbm_ctx* c, const void* host, int host_dtype, int planes) {
    const int nx = c->plan.geo.nx, ny = c->plan.geo.ny, NY = c->plan.geo.NY, y0 = c->plan.geo.y0;
    const size_t rows = (size_t)planes * nx;
    if (host_dtype == c->p.dtype) {
        HIP_TRY(c, hipMemcpy2D(c->stage.get(), (size_t)ny * c->plan.es, (const char*)host + (size_t)y0 * c->plan.es, (size_t)NY * c->plan.es,
                               (size_t)ny * c->plan.es, rows, hipMemcpyHostToDevice));
        return LBM_OK;
    }
    std::vector<char> tmp(rows * ny * c->plan.es);
    if (c->p.dtype == LBM_F32) convert_rows((float*)tmp.data(), (const double*)host, rows, ny, NY, y0, false);
    else convert_rows((double*)tmp.data(), (const float*)host, rows, ny, NY, y0, false);
    HIP_TRY(c, hipMemcpy(c->stage.get(), tmp.data(), tmp.size(), hipMemcpyHostToDevice));
    return LBM_OK;
}

int stage_to_host(lbm_ctx* c, const void* stage, void* host, int host_dtype, int planes) {
    const int nx = c->plan.geo.nx, ny = c->plan.geo.ny, NY = c->plan.geo.NY, y0 = c->plan.geo.y0;
    const size_t rows = (size_t)planes * nx;
    if (host_dtype == c->p.dtype) {
        HIP_TRY(c, hipMemcpy2D((char*)host + (size_t)y0 * c->plan.es, (size_t)NY * c->plan.es, stage, (size_t)ny * c->plan.es,
                               (size_t)ny * c->plan.es, rows, hipMemcpyDeviceToHost));
        return LBM_OK;
    }
    std::vector<char> tmp(rows * ny * c->plan.es);
    HIP_TRY(c, hipMemcpy(tmp.data(), stage, tmp.size(), hipMemcpyDeviceToHost));
    if (c->p.dtype == LBM_F32) convert_rows((double*)host, (const float*)tmp.data(), rows, ny, NY, y0, true);
    else convert_rows((float*)host, (const double*)tmp.data(), rows, ny, NY, y0, true);
    return LBM_OK;
}

// the populations of lat[cur] as they are now
int export_fin(lbm_ctx* c) {
    return launch_variant(c, [&](auto v) {
        using VT = decltype(v);
        using R = typename VT::R;
        with_fields<VT>(c, c->cur, [&](auto f) {
            hipLaunchKernelGGL((k_export_fin<R, VT::SEM, coll_is_prom(VT::COLL), decltype(f)::SHAPED>), grid_tiles<R>(c), dim3(BLK), 0, c->s_compute, f, c->stage.as<R>());
        });
    });
}

// the fields of the LAST iteration: the moments of the state that iteration started from (which: reader_source's)
int export_macro(lbm_ctx* c, int which) {
    return launch_variant(c, [&](auto v) {
        using VT = decltype(v);
        using R = typename VT::R;
        with_fields<VT>(c, which, [&](auto f) {
            hipLaunchKernelGGL((k_export_macro<R, VT::SEM, coll_is_prom(VT::COLL), decltype(f)::SHAPED>), grid_tiles<R>(c), dim3(BLK), 0, c->s_compute, f, c->stage.as<R>());
        });
    });
}

// (MRT.py semantics with arith = fast runs the strict variant, so FAST is false there; that case has no closure (validate_params), and
// either instantiation writes the same 1 / omega.  The closure gathers in MRT_GPU.py semantics, whatever the context's: turb = 0 elsewhere)
int export_tau(lbm_ctx* c, int which) {
    return launch_variant(c, [&](auto v) {
        using VT = decltype(v);
        using R = typename VT::R;
        if constexpr (VT::SEM == SEM_SOLID) {
            // the sub-grid closure (lbm_set_subgrid): the tau of the step that starts from the current state, lat[cur], through the view
            // ... and with a relaxation field (lbm_set_relaxation_field) the cell's own tau0, with and without the closure
            if (c->relax_field()) {
                with_fields<VT>(c, c->cur, [&](auto f) {
                    const R* const rw = c->relax_w.as<const R>();
                    if (c->subgrid > 0.0)
                        hipLaunchKernelGGL((k_export_tau_relax<R, coll_is_fast(VT::COLL), decltype(f)::SHAPED, true>), grid_tiles<R>(c), dim3(BLK), 0, c->s_compute, f,
                                           relax_of<R>(c->p), batch_of<R>(c), sgs_k<R>(c), rw, c->stage.as<R>());
                    else
                        hipLaunchKernelGGL((k_export_tau_relax<R, coll_is_fast(VT::COLL), decltype(f)::SHAPED, false>), grid_tiles<R>(c), dim3(BLK), 0, c->s_compute, f,
                                           relax_of<R>(c->p), batch_of<R>(c), (R)0, rw, c->stage.as<R>());
                });
                return;
            }
            if (c->rheology()) {   // (lbm_set_rheology: 1 / w_nu of the step that starts from lat[cur])
                with_fields<VT>(c, c->cur, [&](auto f) {
                    hipLaunchKernelGGL((k_export_rheology<R, coll_is_fast(VT::COLL), decltype(f)::SHAPED>), grid_tiles<R>(c), dim3(BLK), 0, c->s_compute, f,
                                       relax_of<R>(c->p), batch_of<R>(c), rheo_of<R>(c), c->stage.as<R>(), (R*)nullptr);
                });
                return;
            }
            if (c->subgrid > 0.0) {
                with_fields<VT>(c, c->cur, [&](auto f) {
                    hipLaunchKernelGGL((k_export_tau_subgrid<R, coll_is_fast(VT::COLL), decltype(f)::SHAPED>), grid_tiles<R>(c), dim3(BLK), 0, c->s_compute, f,
                                       relax_of<R>(c->p), batch_of<R>(c), sgs_k<R>(c), c->stage.as<R>());
                });
                return;
            }
        }
        hipLaunchKernelGGL((k_export_tau<R, coll_is_fast(VT::COLL), coll_is_prom(VT::COLL)>), grid_tiles<R>(c), dim3(BLK), 0, c->s_compute,
                           fields_of<Variant<R, VT::COLL, SEM_GPU, VT::TURB>>(c, which), relax_of<R>(c->p), batch_of<R>(c), c->p.turb, c->stage.as<R>());
    });
}

// the shear g = N / rho of the current state, lat[cur], through the view (lbm_get_shear): the kernel of the rheology table, its other output
int export_shear(lbm_ctx* c) {
    return launch_variant(c, [&](auto v) {
        using VT = decltype(v);
        using R = typename VT::R;
        if constexpr (VT::SEM == SEM_SOLID) {
            with_fields<VT>(c, c->cur, [&](auto f) {
                hipLaunchKernelGGL((k_export_rheology<R, coll_is_fast(VT::COLL), decltype(f)::SHAPED>), grid_tiles<R>(c), dim3(BLK), 0, c->s_compute, f,
                                   relax_of<R>(c->p), batch_of<R>(c), Rheo<R>{}, (R*)nullptr, c->stage.as<R>());
            });
        }
    });
}

constexpr int RED_BLOCKS = 1024;   // partial sums per lattice of lbm_mean_u

int reduce_u(lbm_ctx* c, int which) {
    return launch_variant(c, [&](auto v) {
        using VT = decltype(v);
        using R = typename VT::R;
        with_fields<VT>(c, which, [&](auto f) {
            hipLaunchKernelGGL((k_reduce_u<R, VT::SEM, coll_is_prom(VT::COLL), decltype(f)::SHAPED>), dim3(RED_BLOCKS, 1, c->plan.batch), dim3(BLK), 0,
                               c->s_compute, f, c->red_dev.as<double>());
        });
    });
}

// What lbm_init_equilibrium and lbm_set_state share: the samplers ended, the run state of a fresh lattice in lat[0].  The caller
// has synchronised the streams.
static void reset_run_state(lbm_ctx* c) {
    for (int i = 0; i < NSCHEDULED; ++i) sampler_free(c, i);
    c->cur = 0; c->raw[0] = 1; c->raw[1] = 1; c->nsteps = 0; c->lag = 0; c->lag_valid = false;
    c->order.reset();
}
}  // namespace lbmhost

using namespace lbmhost;

extern "C" {


int lbm_abi_version(void) { return LBM_ABI_VERSION; }

int lbm_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

lbm_ctx* lbm_create(const lbm_params* p, char* err, size_t errlen) {
    auto bail = [&](const std::string& m) -> lbm_ctx* {
        if (err && errlen) { std::snprintf(err, errlen, "%s", m.c_str()); }
        return nullptr;
    };
    {
        const std::string bad = validate_params(p);
        if (!bad.empty()) return bail(bad);
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) return bail(std::string("no HIP device: ") + hipGetErrorString(e));
    if (p->device < 0 || p->device >= ndev) return bail("device ordinal out of range");
    if ((e = hipSetDevice(p->device)) != hipSuccess) return bail(std::string("hipSetDevice: ") + hipGetErrorString(e));

    hipDeviceProp_t prop;
    const int ncu = hipGetDeviceProperties(&prop, p->device) == hipSuccess && prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    Plan plan;
    std::string plan_err;
    if (!make_plan(*p, ncu, true, plan, plan_err)) return bail(plan_err);
    lbm_ctx* c = new (std::nothrow) lbm_ctx(*p, plan);
    if (!c) return bail("out of host memory");
#ifdef LBM_DEBUG
    c->order.debug_no_exchange_ready = std::getenv("LBM_DEBUG_NO_EXCHANGE_READY") != nullptr;
#endif
    const size_t bytes = c->plan.lat_bytes;
    auto cleanup = [&](const std::string m) -> lbm_ctx* { lbm_destroy(c); return bail(m); };   // (m by value: it may be c->err)
    if ((e = hipStreamCreateWithFlags(&c->s_compute, hipStreamNonBlocking)) != hipSuccess) return cleanup("hipStreamCreate");
    {   // halo exchange stream at the highest priority: its (tiny) RCCL kernels must not queue behind the
        // thousands of workgroups of the interior kernel they are meant to overlap
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        if (!c->plan.comm_priority) hi = lo;   // A/B: same priority as the compute stream
        if ((e = hipStreamCreateWithPriority(&c->s_comm, hipStreamNonBlocking, hi)) != hipSuccess) return cleanup("hipStreamCreate");
    }
    // (the events between the two streams of this context order kernels of ONE device: no system-scope release with every record -- a
    // slab's unit records two and waits for two; 4096 x 512 slab in loopback 189 -> 195 GLUPS, 4096 x 1024 246 -> 251)
    constexpr unsigned LBM_EVENT_FENCE = hipEventDisableSystemFence;
    if ((e = hipEventCreateWithFlags(&c->ev_edges, hipEventDisableTiming | LBM_EVENT_FENCE)) != hipSuccess) return cleanup("hipEventCreate");
    if ((e = hipEventCreateWithFlags(&c->ev_halo, hipEventDisableTiming)) != hipSuccess) return cleanup("hipEventCreate");
    if ((e = hipEventCreateWithFlags(&c->ev_int, hipEventDisableTiming | LBM_EVENT_FENCE)) != hipSuccess) return cleanup("hipEventCreate");
    if ((e = hipEventCreateWithFlags(&c->ev_go, hipEventDisableTiming | LBM_EVENT_FENCE)) != hipSuccess) return cleanup("hipEventCreate");
    if ((e = hipEventCreate(&c->ev_t0)) != hipSuccess) return cleanup("hipEventCreate");
    if ((e = hipEventCreate(&c->ev_t1)) != hipSuccess) return cleanup("hipEventCreate");
    // the two lattices (+ ftemp of the push scheme); the scratch lattices of the frame passes come on first use (ensure_scratch)
    for (int i = 0; i < (c->plan.push ? 3 : 2); ++i) {
        if (alloc_ok(c, c->lat[i].alloc(bytes, "lattice")) != LBM_OK) return cleanup(c->err);
        // on the compute stream: the streams are non-blocking, a null-stream memset would race with the kernels
        if ((e = hipMemsetAsync(c->lat[i].get(), 0, bytes, c->s_compute)) != hipSuccess) return cleanup(std::string("hipMemset: ") + hipGetErrorString(e));
    }
    if (p->semantics == LBM_SEM_BOUNCE_BACK_SOLID) {   // all fluid: one body without a cell, at rest
        Obstacles next;
        next.mask.assign((size_t)c->plan.batch * p->nx * p->ny, 0);
        if (obstacles_change(c, ObsLevel::mask, next) != LBM_OK) return cleanup(c->err);
    }
    if (c->plan.batch > 1) {   // every lattice starts with the rates of lbm_params; lbm_set_relaxation() changes them one by one
        const size_t rb = c->plan.es == 4 ? sizeof(Relax<float>) : sizeof(Relax<double>);
        if (alloc_ok(c, c->relax_dev.alloc(rb * c->plan.batch, "relaxation")) != LBM_OK) return cleanup(c->err);
        for (int i = 0; i < c->plan.batch; ++i)
            if (lbm_set_relaxation(c, i, p->omega, p->omegam, p->omega_e, p->omega_eps, p->omega_q) != LBM_OK) return cleanup(c->err);
    }
    if (lbm_init_equilibrium(c) != LBM_OK) return cleanup(c->err);
    if (c->plan.tail_tiles && warm_stream(c) != LBM_OK) return cleanup("warm-up launch of the streaming kernel");   // (see warm_stream)
    return c;
}

void lbm_destroy(lbm_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->p.device);
    if (c->s_compute) (void)hipStreamSynchronize(c->s_compute);
    if (c->s_comm) (void)hipStreamSynchronize(c->s_comm);
    if (c->comm && rccl().ok) (void)rccl().CommDestroy(c->comm);
    if (c->ev_edges) (void)hipEventDestroy(c->ev_edges);
    if (c->ev_halo) (void)hipEventDestroy(c->ev_halo);
    if (c->ev_int) (void)hipEventDestroy(c->ev_int);
    if (c->ev_go) (void)hipEventDestroy(c->ev_go);
    if (c->ev_t0) (void)hipEventDestroy(c->ev_t0);
    if (c->ev_t1) (void)hipEventDestroy(c->ev_t1);
    if (c->s_compute) (void)hipStreamDestroy(c->s_compute);
    if (c->s_comm) (void)hipStreamDestroy(c->s_comm);
    delete c;   // (and with it every buffer: each is a DevBuf)
}

const char* lbm_last_error(const lbm_ctx* c) { return c ? c->err.c_str() : "null context"; }

int lbm_init_equilibrium(lbm_ctx* c) {
    if (!c) return LBM_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->p.device));
    int rc = sync_all(c);
    if (rc) return rc;
    reset_run_state(c);
    const dim3 g = grid_rows(c, c->plan.geo.ny);
    rc = launch_variant(c, [&](auto v) {
        using VT = decltype(v);
        using R = typename VT::R;
        hipLaunchKernelGGL((k_init<R, coll_is_prom(VT::COLL)>), g, dim3(BLK), 0, c->s_compute, c->lat[0].as<R>(), c->plan.geo, (R)c->p.uLB, c->p.turb, c->plan.bstride);
    });
    if (rc == LBM_OK) rc = solid_fix(c);
    if (rc) return rc;
    return push_reset(c);
}

int lbm_set_state(lbm_ctx* c, const void* fin_host, int host_dtype) {
    if (!c || !fin_host || (host_dtype != LBM_F32 && host_dtype != LBM_F64)) return fail(c, LBM_ERR_INVALID, "lbm_set_state: bad argument");
    HIP_TRY(c, hipSetDevice(c->p.device));
    int rc = sync_all(c);
    if (rc) return rc;
    rc = ensure_field_stage(c);
    if (rc) return rc;
    rc = host_to_stage(c, fin_host, host_dtype, Q * c->plan.batch);   // [B][9][nx][ny] is B * 9 planes
    if (rc) return rc;
    reset_run_state(c);
    rc = launch_variant(c, [&](auto v) {
        using VT = decltype(v);
        using R = typename VT::R;
        hipLaunchKernelGGL((k_import<R, coll_is_prom(VT::COLL)>), grid_tiles<R>(c), dim3(BLK), 0, c->s_compute, c->stage.as<const R>(), c->lat[0].as<R>(), c->plan.geo,
                           (R)c->p.uLB, c->p.turb, c->plan.bstride);
    });
    if (rc == LBM_OK) rc = solid_fix(c);   // (solid cells: w_k, whatever the host array holds there)
    if (rc) return rc;
    rc = push_reset(c);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->s_compute));
    return LBM_OK;
}

int lbm_set_relaxation(lbm_ctx* c, int index, double omega, double omegam, double omega_e, double omega_eps, double omega_q) {
    if (!c || index < 0 || index >= c->plan.batch) return fail(c, LBM_ERR_INVALID, "lbm_set_relaxation: index out of range");
    HIP_TRY(c, hipSetDevice(c->p.device));
    lbm_params q = c->p;
    q.omega = omega; q.omegam = omegam; q.omega_e = omega_e; q.omega_eps = omega_eps; q.omega_q = omega_q;
    if (c->plan.batch == 1) {   // rates travel by value with every launch
        c->p = q;
        return LBM_OK;
    }
    // ordered behind the steps already enqueued: the copy goes through the compute stream (pageable source, so the call
    // returns only after the runtime has staged it)
    HIP_TRY(c, hipStreamSynchronize(c->s_comm));
    if (c->plan.es == 4) {
        const Relax<float> w = relax_of<float>(q);
        HIP_TRY(c, hipMemcpyAsync(c->relax_dev.as<Relax<float>>() + index, &w, sizeof(w), hipMemcpyHostToDevice, c->s_compute));
    } else {
        const Relax<double> w = relax_of<double>(q);
        HIP_TRY(c, hipMemcpyAsync(c->relax_dev.as<Relax<double>>() + index, &w, sizeof(w), hipMemcpyHostToDevice, c->s_compute));
    }
    HIP_TRY(c, hipStreamSynchronize(c->s_compute));
    return LBM_OK;
}

int lbm_sync(lbm_ctx* c) {
    if (!c) return LBM_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->p.device));
    return sync_all(c);
}

long long lbm_steps_done(const lbm_ctx* c) { return c ? c->nsteps : -1; }

int lbm_get_fields(lbm_ctx* c, void* u_host, void* rho_host, void* fin_host, int host_dtype) {
    if (!c || (host_dtype != LBM_F32 && host_dtype != LBM_F64)) return fail(c, LBM_ERR_INVALID, "lbm_get_fields: bad argument");
    int which = 0;   // (the populations alone: lat[cur] as it is, no replay of the lagged lattice)
    int rc = u_host || rho_host ? reader_source(c, "lbm_get_fields", false, &which) : lbm_sync(c);
    if (rc == LBM_OK) rc = ensure_field_stage(c);
    if (rc) return rc;
    const size_t n = (size_t)c->plan.geo.nx * c->plan.geo.ny;
    const size_t hes = host_dtype == LBM_F32 ? 4 : 8;
    if (u_host || rho_host) {
        rc = export_macro(c, which);
        if (rc) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->s_compute));
        for (int b = 0; b < c->plan.batch; ++b) {   // staging of lattice b: [ux | uy | rho]; host: u[B][2][nx][NY], rho[B][nx][NY]
            const char* st = c->stage.as<const char>() + (size_t)b * 3 * n * c->plan.es;
            const size_t hn = (size_t)c->plan.geo.nx * c->plan.geo.NY * hes;
            if (u_host) { rc = stage_to_host(c, st, (char*)u_host + (size_t)b * 2 * hn, host_dtype, 2); if (rc) return rc; }
            if (rho_host) { rc = stage_to_host(c, st + 2 * n * c->plan.es, (char*)rho_host + (size_t)b * hn, host_dtype, 1); if (rc) return rc; }
        }
    }
    if (fin_host) {
        rc = export_fin(c);
        if (rc) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->s_compute));
        rc = stage_to_host(c, c->stage.get(), fin_host, host_dtype, Q * c->plan.batch);
        if (rc) return rc;
    }
    return LBM_OK;
}

int lbm_mean_u(lbm_ctx* c, double* mean_out) {
    if (!c || !mean_out) return fail(c, LBM_ERR_INVALID, "lbm_mean_u: bad argument");
    int which = 0;
    int rc = reader_source(c, "lbm_mean_u", false, &which);
    if (rc == LBM_OK) rc = alloc_ok(c, c->red_dev.ensure(((size_t)RED_BLOCKS + 1) * c->plan.batch * sizeof(double), "reduction"));
    if (rc == LBM_OK) rc = reduce_u(c, which);
    if (rc) return rc;
    double* res = c->red_dev.as<double>() + (size_t)RED_BLOCKS * c->plan.batch;
    const double scale = 1.0 / (2.0 * (double)c->plan.geo.nx * (double)c->plan.geo.ny);
    hipLaunchKernelGGL(k_reduce_final, dim3((c->plan.batch + BLK - 1) / BLK), dim3(BLK), 0, c->s_compute, c->red_dev.as<double>(), RED_BLOCKS, c->plan.batch, scale, res);
    HIP_TRY(c, hipGetLastError());
    return records_to_host(c, res, (size_t)c->plan.batch * sizeof(double), mean_out);
}

int lbm_get_tau(lbm_ctx* c, void* tau_host, int host_dtype) {
    if (!c || !tau_host || (host_dtype != LBM_F32 && host_dtype != LBM_F64)) return fail(c, LBM_ERR_INVALID, "lbm_get_tau: bad argument");
    int which = 0;
    int rc = reader_source(c, "lbm_get_tau", false, &which);
    if (rc == LBM_OK) rc = ensure_field_stage(c);
    if (rc == LBM_OK) rc = export_tau(c, which);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->s_compute));
    return stage_to_host(c, c->stage.get(), tau_host, host_dtype, c->plan.batch);
}

int lbm_get_shear(lbm_ctx* c, void* g_host, int host_dtype) {
    if (!c || !g_host || (host_dtype != LBM_F32 && host_dtype != LBM_F64)) return fail(c, LBM_ERR_INVALID, "lbm_get_shear: bad argument");
    int rc = need_solid(c, "lbm_get_shear");
    if (rc) return rc;
    int which = 0;
    rc = reader_source(c, "lbm_get_shear", false, &which);
    if (rc == LBM_OK) rc = ensure_field_stage(c);
    if (rc == LBM_OK) rc = export_shear(c);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->s_compute));
    return stage_to_host(c, c->stage.get(), g_host, host_dtype, c->plan.batch);
}

int lbm_copy_bandwidth(lbm_ctx* c, size_t bytes, int iters, double* gbps) {
    if (!c || !gbps || iters < 1 || bytes < 16) return fail(c, LBM_ERR_INVALID, "lbm_copy_bandwidth: bad argument");
    HIP_TRY(c, hipSetDevice(c->p.device));
    bytes &= ~(size_t)15;
    DevBuf src, dst;
    if (!src.alloc(bytes, "").empty() || !dst.alloc(bytes, "").empty()) return fail(c, LBM_ERR_NOMEM, "lbm_copy_bandwidth: hipMalloc failed");
    const uint4* a = src.as<const uint4>();
    uint4* b = dst.as<uint4>();
    (void)hipMemsetAsync(src.get(), 1, bytes, c->s_compute);
    const size_t n = bytes / 16;
    const int blocks = 256 * 8;
    hipLaunchKernelGGL(k_copy16, dim3(blocks), dim3(BLK), 0, c->s_compute, a, b, n);
    (void)hipEventRecord(c->ev_t0, c->s_compute);
    for (int i = 0; i < iters; ++i)
        hipLaunchKernelGGL(k_copy16, dim3(blocks), dim3(BLK), 0, c->s_compute, a, b, n);
    (void)hipEventRecord(c->ev_t1, c->s_compute);
    hipError_t e = hipEventSynchronize(c->ev_t1);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, c->ev_t0, c->ev_t1);
    if (e != hipSuccess) return fail(c, LBM_ERR_HIP, std::string("lbm_copy_bandwidth: ") + hipGetErrorString(e));
    *gbps = 2.0 * (double)bytes * iters / (ms * 1e-3) / 1e9;
    return LBM_OK;
}

int lbm_fma_rate(lbm_ctx* c, double ms_total, double* tflops) {
    if (!c || !tflops || !(ms_total > 0) || ms_total > 2000) return fail(c, LBM_ERR_INVALID, "lbm_fma_rate: bad argument (0 < ms <= 2000)");
    HIP_TRY(c, hipSetDevice(c->p.device));
    const int blocks = c->plan.ncu * 8, iters = 4096;
    DevBuf buf;
    const std::string bad = buf.alloc((size_t)blocks * BLK * sizeof(float), "fma sink");
    if (!bad.empty()) return fail(c, LBM_ERR_HIP, bad);
    float* sink = buf.as<float>();
    auto run = [&](int n, float* ms) -> hipError_t {
        (void)hipEventRecord(c->ev_t0, c->s_compute);
        for (int i = 0; i < n; ++i) hipLaunchKernelGGL(k_fma_burn, dim3(blocks), dim3(BLK), 0, c->s_compute, sink, iters, 1.0f + (float)i);
        (void)hipEventRecord(c->ev_t1, c->s_compute);
        hipError_t e = hipEventSynchronize(c->ev_t1);
        if (e == hipSuccess) e = hipEventElapsedTime(ms, c->ev_t0, c->ev_t1);
        return e;
    };
    float ms1 = 0.f, ms = 0.f;
    hipError_t e = run(1, &ms1);                                    // calibration (also the first, slower, launch)
    const int n = e == hipSuccess && ms1 > 0 ? std::max(1, (int)(ms_total / ms1)) : 1;
    if (e == hipSuccess) e = run(n, &ms);
    if (e != hipSuccess) return fail(c, LBM_ERR_HIP, std::string("lbm_fma_rate: ") + hipGetErrorString(e));
    // per thread and iteration: 16 packed FMAs = 32 FMAs = 64 flop
    *tflops = (double)n * blocks * BLK * (double)iters * 64.0 / (ms * 1e-3) / 1e12;
    return LBM_OK;
}
}  // extern "C"
