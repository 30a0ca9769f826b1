// lbm_bodies.hip -- liblbm_hip.so: the force and the torque on each body of a solid mask (lbm_set_solid_bodies, lbm_get_solid_bodies,
// lbm_solid_body_count, lbm_body_force and the series lbm_force_* of the C ABI declared in include/lbm.h; LBM_SEM_BOUNCE_BACK_SOLID).
// The labels, the centres and the link list are host work (lbm_bodies.hpp), uploaded here whenever the mask or the labels change; a
// sample walks the list, O(links), and reduces per body by the tree of lbm_reduce.hpp.  gfx950 only.  DESIGN.md 2.10.
#include <cmath>

#include "lbm_host.hpp"
#include "lbm_reduce.hpp"

namespace lbmhost {

static_assert(sizeof(lbm_body_force_record) == 6 * sizeof(double), "record layout");
static_assert(sizeof(BodyLink) == 8 && sizeof(BodyChunk) == 16, "table layout");
constexpr bool body_vectors_match() {
    for (int k = 0; k < Q; ++k)
        if (BODY_CX[k] != cxk(k) || BODY_CY[k] != cyk(k)) return false;
    return true;
}
static_assert(body_vectors_match(), "lbm_bodies.hpp restates the lattice vectors");
constexpr int REC = 6;   // doubles of a record

// The terms of one link, in double without contraction: f = the cell's post-collision population of direction opp(k) as the lattice
// holds it (what k_solid_force reads), tx = 2 cx_opp(k) f, ty = 2 cy_opp(k) f, and with the link's midpoint relative to the centre,
// (rx, ry) = (x - cx_k / 2 - x0, y + cy_k / 2 - y0) (the half-integers are exact, one rounding per component),
//     links += 1, fx += tx, fy += ty, tz += rx ty + ry tx.
struct BodyAcc {
    double links, fx, fy, tz;
    static constexpr int VALS = 4;
    static __device__ __forceinline__ BodyAcc identity() { return BodyAcc{0.0, 0.0, 0.0, 0.0}; }
    static __device__ __forceinline__ void fold(BodyAcc& a, const BodyAcc& b) {
#pragma clang fp contract(off)
        a.links = a.links + b.links;
        a.fx = a.fx + b.fx;
        a.fy = a.fy + b.fy;
        a.tz = a.tz + b.tz;
    }
    template <typename F>
    __device__ __forceinline__ void each(F&& f) { f(links); f(fx); f(fy); f(tz); }
};

// One workgroup per chunk of the list (BODY_CHUNK links of one body; grid x: the chunks of a lattice, padded to the longest of the
// batch with empty ones; grid z: the lattice).  Lane t folds links t, t + BLK, .. of its chunk in this order; then the tree.  The
// chunks are cut from the list alone, so a lattice's partial results are the same alone and in a batch.
// MOVE (k_body_force_move, while a body motion is set): f_out = f - delta, so (tx, ty) = c_opp(k) (2 f - delta), delta the link's entry
// of link_delta -- the term as the lattice adds it, a double; the midpoint, the order and the tree are the same.
template <typename R, bool MOVE>
__device__ __forceinline__ void body_force_chunk(const R* __restrict__ src, const Geo& geo, long long bstride, const BodyLink* __restrict__ links,
                                                 const BodyChunk* __restrict__ chunks, const double* __restrict__ centre, int nbodies,
                                                 double* __restrict__ partial, const double* __restrict__ link_delta) {
#pragma clang fp contract(off)
    __shared__ double sh[BLK / RED_WAVE][BodyAcc::VALS];
    const size_t slot = (size_t)blockIdx.z * gridDim.x + blockIdx.x;
    const BodyChunk ch = chunks[slot];
    src += blockIdx.z * bstride;
    BodyAcc a = BodyAcc::identity();
    if (ch.n > 0) {
        const double x0 = centre[((size_t)blockIdx.z * nbodies + ch.body) * 2], y0 = centre[((size_t)blockIdx.z * nbodies + ch.body) * 2 + 1];
        for (int i = threadIdx.x; i < ch.n; i += BLK) {
            const BodyLink l = links[ch.begin + i];
            const int x = l.x, y = l.yk >> 4, k = l.yk & 15, o = opp(k);
            const double f = (double)src[o * geo.plane + geo.at(x, y)];
            double tx, ty;
            if (MOVE) {
                const double t = 2.0 * f - link_delta[ch.begin + i];
                tx = (double)cxk(o) * t;
                ty = (double)cyk(o) * t;
            } else {
                tx = (double)(2 * cxk(o)) * f;
                ty = (double)(2 * cyk(o)) * f;
            }
            const double rx = ((double)x - 0.5 * (double)cxk(k)) - x0, ry = ((double)y + 0.5 * (double)cyk(k)) - y0;
            a.links = a.links + 1.0;
            a.fx = a.fx + tx;
            a.fy = a.fy + ty;
            a.tz = a.tz + (rx * ty + ry * tx);
        }
    }
    red_wave(a);
    if (red_workgroup<BodyAcc, BLK / RED_WAVE>(a, sh)) red_store(partial + slot * BodyAcc::VALS, a);
}

template <typename R>
__global__ __launch_bounds__(BLK) void k_body_force(const R* __restrict__ src, Geo geo, long long bstride, const BodyLink* __restrict__ links,
                                                    const BodyChunk* __restrict__ chunks, const double* __restrict__ centre, int nbodies,
                                                    double* __restrict__ partial) {
    body_force_chunk<R, false>(src, geo, bstride, links, chunks, centre, nbodies, partial, nullptr);
}

template <typename R>
__global__ __launch_bounds__(BLK) void k_body_force_move(const R* __restrict__ src, Geo geo, long long bstride, const BodyLink* __restrict__ links,
                                                         const BodyChunk* __restrict__ chunks, const double* __restrict__ centre, int nbodies,
                                                         double* __restrict__ partial, const double* __restrict__ link_delta) {
    body_force_chunk<R, true>(src, geo, bstride, links, chunks, centre, nbodies, partial, link_delta);
}

// The final pass, one wave per body and lattice over the body's chunks: rec[z][body] = {step, body, links, fx, fy, tz}
__global__ __launch_bounds__(RED_WAVE) void k_body_force_final(const double* __restrict__ partial, const int32_t* __restrict__ first, int maxchunks,
                                                               double step, double* __restrict__ rec) {
    const int body = blockIdx.x, nbodies = gridDim.x, z = blockIdx.y;
    const int32_t* f = first + (size_t)z * (nbodies + 1);
    const BodyAcc a = red_final<BodyAcc>(partial + ((size_t)z * maxchunks + f[body]) * BodyAcc::VALS, f[body + 1] - f[body]);
    if (threadIdx.x == 0) {
        double* r = rec + ((size_t)z * nbodies + body) * REC;
        r[0] = step;
        r[1] = (double)body;
        red_store(r + 2, a);
    }
}

void bodies_free(lbm_ctx* c) {
    if (c->body.base) (void)hipFree(c->body.base);
    c->body = BodyTables{};
}

// The tables of the context's mask, labels and centres, built on the host and uploaded; the old ones are freed once the new ones are in
// place.  The caller has synchronised the streams.
int bodies_upload(lbm_ctx* c) {
    const int B = c->plan.batch, nb = c->nbodies, nx = c->plan.geo.nx, ny = c->plan.geo.ny;
    const size_t n = (size_t)nx * ny;
    std::vector<BodyLink> links;
    std::vector<long long> start((size_t)B * (nb + 1));
    std::vector<std::vector<BodyChunk>> chunks(B);
    std::vector<int32_t> first((size_t)B * (nb + 1));
    size_t maxchunks = 1;
    for (int b = 0; b < B; ++b) {
        body_links(c->solid_mask.data() + b * n, c->body_label.data() + b * n, nx, ny, nb, links, start.data() + (size_t)b * (nb + 1));
        body_chunks(start.data() + (size_t)b * (nb + 1), nb, chunks[b], first.data() + (size_t)b * (nb + 1));
        maxchunks = std::max(maxchunks, chunks[b].size());
    }
    if (maxchunks > 0x7fffffffu) return fail(c, LBM_ERR_INVALID, "the mask has too many links for the force tables");
    std::vector<BodyChunk> table(B * maxchunks, BodyChunk{0, 0, 0});
    for (int b = 0; b < B; ++b) std::copy(chunks[b].begin(), chunks[b].end(), table.begin() + b * maxchunks);
    auto pad8 = [](size_t v) { return (v + 7) & ~(size_t)7; };
    const size_t o_chunks = std::max<size_t>(8, links.size() * sizeof(BodyLink)), o_first = o_chunks + table.size() * sizeof(BodyChunk),
                 o_centre = o_first + pad8(first.size() * sizeof(int32_t)), o_partial = o_centre + c->body_centre.size() * sizeof(double),
                 o_rec = o_partial + B * maxchunks * BodyAcc::VALS * sizeof(double), bytes = o_rec + (size_t)B * nb * REC * sizeof(double);
    char* base = nullptr;
    hipError_t e = hipMalloc((void**)&base, bytes);
    if (e != hipSuccess) return fail(c, LBM_ERR_NOMEM, std::string("hipMalloc(body tables): ") + hipGetErrorString(e));
    e = links.empty() ? hipSuccess : hipMemcpy(base, links.data(), links.size() * sizeof(BodyLink), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(base + o_chunks, table.data(), table.size() * sizeof(BodyChunk), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(base + o_first, first.data(), first.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(base + o_centre, c->body_centre.data(), c->body_centre.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(base);
        return fail(c, LBM_ERR_HIP, std::string("hipMemcpy(body tables): ") + hipGetErrorString(e));
    }
    bodies_free(c);
    motion_rest(c);   // (new labels or a new mask: every body at rest again)
    c->body.base = base;
    c->body.links = (const BodyLink*)base;
    c->body.chunks = (const BodyChunk*)(base + o_chunks);
    c->body.first = (const int32_t*)(base + o_first);
    c->body.centre = (const double*)(base + o_centre);
    c->body.partial = (double*)(base + o_partial);
    c->body.rec = (double*)(base + o_rec);
    c->body.maxchunks = (int)maxchunks;
    return LBM_OK;
}

// The default: one body that holds every solid cell, centred at its centroid (a fresh context, and after every lbm_set_solid).
int bodies_default(lbm_ctx* c) {
    if (c->p.semantics != LBM_SEM_BOUNCE_BACK_SOLID) return LBM_OK;
    const int B = c->plan.batch;
    const size_t n = (size_t)c->plan.geo.nx * c->plan.geo.ny;
    c->nbodies = 1;
    c->body_label.resize(B * n);
    for (size_t i = 0; i < B * n; ++i) c->body_label[i] = c->solid_mask[i] ? 0 : -1;
    c->body_centre.assign((size_t)B * 2, 0.0);
    for (int b = 0; b < B; ++b)
        body_centroids(c->solid_mask.data() + b * n, c->body_label.data() + b * n, c->plan.geo.nx, c->plan.geo.ny, 1, c->body_centre.data() + 2 * b);
    return bodies_upload(c);
}

// One sample from lat[cur], the lattice after c->nsteps steps, into rec[batch][nbodies] on the device; on the compute stream.
static int body_force_enqueue(lbm_ctx* c, double* rec) {
    const BodyTables& t = c->body;
    return launch_variant(c, [&](auto v) {
        using R = typename decltype(v)::R;
        if (c->motion.base)
            hipLaunchKernelGGL((k_body_force_move<R>), dim3(t.maxchunks, 1, c->plan.batch), dim3(BLK), 0, c->s_compute, (const R*)c->lat[c->cur],
                               c->plan.geo, c->plan.bstride, t.links, t.chunks, t.centre, c->nbodies, t.partial, c->motion.link_delta);
        else
            hipLaunchKernelGGL((k_body_force<R>), dim3(t.maxchunks, 1, c->plan.batch), dim3(BLK), 0, c->s_compute, (const R*)c->lat[c->cur], c->plan.geo,
                               c->plan.bstride, t.links, t.chunks, t.centre, c->nbodies, t.partial);
        hipLaunchKernelGGL(k_body_force_final, dim3(c->nbodies, c->plan.batch), dim3(RED_WAVE), 0, c->s_compute, (const double*)t.partial, t.first,
                           t.maxchunks, (double)c->nsteps, rec);
    });
}

// The next sample of the series (lbm_force_sample, and sample_after_unit of the step loop).
int force_series_sample(lbm_ctx* c) {
    void* slot = series_slot(c->force_series);
    if (!slot) return LBM_OK;
    const int rc = body_force_enqueue(c, (double*)slot);
    if (rc) return rc;
    ++c->force_series.count;
    return LBM_OK;
}

// What the calls share: a context with a mask whose lattice holds post-collision populations.
static int force_ready(lbm_ctx* c, const char* call, bool stepped) {
    if (c->p.semantics != LBM_SEM_BOUNCE_BACK_SOLID)
        return fail(c, LBM_ERR_STATE, std::string(call) + ": this context has no solid mask (create it with semantics = LBM_SEM_BOUNCE_BACK_SOLID)");
    if (stepped && (c->nsteps == 0 || c->raw[c->cur]))
        return fail(c, LBM_ERR_STATE, std::string(call) + ": no step yet (the lattice holds post-collision populations after one)");
    return LBM_OK;
}
}  // namespace lbmhost

using namespace lbmhost;

extern "C" {

int lbm_set_solid_bodies(lbm_ctx* c, const int32_t* body, int nbodies, const double* centre) {
    if (!c) return LBM_ERR_INVALID;
    int rc = force_ready(c, "lbm_set_solid_bodies", false);
    if (rc) return rc;
    if (!body || nbodies < 1 || nbodies > BODY_MAX) return fail(c, LBM_ERR_INVALID, "lbm_set_solid_bodies: bad argument (1 <= nbodies <= 256)");
    const int B = c->plan.batch;
    const size_t n = (size_t)c->plan.geo.nx * c->plan.geo.ny;
    const long long bad = body_bad_label(c->solid_mask.data(), body, B * n, nbodies);
    if (bad >= 0)
        return fail(c, LBM_ERR_INVALID, "lbm_set_solid_bodies: the label of solid cell " + std::to_string(bad) + " is not in [0, nbodies)");
    for (size_t i = 0; centre && i < (size_t)B * nbodies * 2; ++i)
        if (!std::isfinite(centre[i])) return fail(c, LBM_ERR_INVALID, "lbm_set_solid_bodies: a centre is not finite");
    HIP_TRY(c, hipSetDevice(c->p.device));
    rc = sync_all(c);
    if (rc) return rc;
    sampler_free(c, SMP_FORCE);
    // (as lbm_set_solid: the context changes once the new tables are on the device)
    std::vector<int32_t> label(B * n);
    for (size_t i = 0; i < B * n; ++i) label[i] = c->solid_mask[i] ? body[i] : -1;
    std::vector<double> cen((size_t)B * nbodies * 2);
    for (int b = 0; b < B; ++b) {
        if (centre) std::copy(centre + (size_t)b * nbodies * 2, centre + (size_t)(b + 1) * nbodies * 2, cen.begin() + (size_t)b * nbodies * 2);
        else body_centroids(c->solid_mask.data() + b * n, label.data() + b * n, c->plan.geo.nx, c->plan.geo.ny, nbodies, cen.data() + (size_t)b * nbodies * 2);
    }
    std::swap(c->nbodies, nbodies);
    c->body_label.swap(label);
    c->body_centre.swap(cen);
    rc = bodies_upload(c);
    if (rc) {
        std::swap(c->nbodies, nbodies);
        c->body_label.swap(label);
        c->body_centre.swap(cen);
    }
    return rc;
}

int lbm_get_solid_bodies(lbm_ctx* c, int32_t* body_out, double* centre_out) {
    if (!c) return LBM_ERR_INVALID;
    const int rc = force_ready(c, "lbm_get_solid_bodies", false);
    if (rc) return rc;
    if (body_out) std::memcpy(body_out, c->body_label.data(), c->body_label.size() * sizeof(int32_t));
    if (centre_out) std::memcpy(centre_out, c->body_centre.data(), c->body_centre.size() * sizeof(double));
    return LBM_OK;
}

int lbm_solid_body_count(lbm_ctx* c) { return c && c->p.semantics == LBM_SEM_BOUNCE_BACK_SOLID ? c->nbodies : 0; }

int lbm_body_force(lbm_ctx* c, lbm_body_force_record* out) {
    if (!c || !out) return fail(c, LBM_ERR_INVALID, "lbm_body_force: bad argument");
    int rc = force_ready(c, "lbm_body_force", true);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->p.device));
    rc = sync_all(c);
    if (rc == LBM_OK) rc = body_force_enqueue(c, c->body.rec);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(out, c->body.rec, (size_t)c->plan.batch * c->nbodies * sizeof(lbm_body_force_record), hipMemcpyDeviceToHost, c->s_compute));
    HIP_TRY(c, hipStreamSynchronize(c->s_compute));
    return LBM_OK;
}

int lbm_force_begin(lbm_ctx* c, int every, int capacity) {
    if (!c || every < 0 || capacity < 1) return fail(c, LBM_ERR_INVALID, "lbm_force_begin: bad argument");
    int rc = force_ready(c, "lbm_force_begin", true);
    if (rc == LBM_OK) rc = sampler_begin(c, SMP_FORCE, every);
    if (rc) return rc;
    sampler_free(c, SMP_FORCE);
    rc = series_alloc(c, c->force_series, (size_t)c->nbodies * sizeof(lbm_body_force_record), capacity, "force series");
    if (rc) return rc;
    c->sampler[SMP_FORCE].arm(c->nsteps, every, 1);
    return LBM_OK;
}

int lbm_force_sample(lbm_ctx* c) {
    if (!c) return LBM_ERR_INVALID;
    if (!c->force_series.dev) return fail(c, LBM_ERR_STATE, "lbm_force_sample: nothing to sample into (lbm_force_begin)");
    int rc = force_ready(c, "lbm_force_sample", true);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->p.device));
    rc = sync_all(c);
    return rc ? rc : force_series_sample(c);
}

int lbm_force_read(lbm_ctx* c, lbm_body_force_record* records_out, int max_records, long long* count, long long* dropped) {
    return series_read(c, &lbm_ctx::force_series, "lbm_force_read", records_out, max_records, count, dropped);
}

int lbm_force_end(lbm_ctx* c) { return sampler_end(c, SMP_FORCE); }
}  // extern "C"
