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
// The term of a link by the mode of the wall rule (WallArg), as k_solid_force; link: the mode's double per entry of the list.
//   WALL_REST   (tx, ty) = 2 c_opp(k) f; the arm of the torque is the link's midpoint, q = 1/2
//   WALL_MOVE   f_out = f - delta, so (tx, ty) = c_opp(k) (2 f - delta), delta = link[i] (link_delta) -- the term as the lattice adds it, a
//               double; the midpoint again
//   WALL_SHAPE  f_out = f, f_in = shape_link, (tx, ty) = c_opp(k) (f_out + f_in), and the arm is the wall point,
//               (rx, ry) = ((x - q cx_k) - x0, (y + q cy_k) - y0), q = link[i] (link_q, the effective q)
template <typename R, int WALL>
__global__ __launch_bounds__(BLK) void k_body_force(const R* __restrict__ src, Geo geo, long long bstride, const BodyLink* __restrict__ links,
                                                    const BodyChunk* __restrict__ chunks, const double* __restrict__ centre, int nbodies,
                                                    double* __restrict__ partial, WallArg<R, WALL> wa, const double* __restrict__ link) {
#pragma clang fp contract(off)
    __shared__ double shm[BLK / RED_WAVE][BodyAcc::VALS];
    const size_t slot = (size_t)blockIdx.z * gridDim.x + blockIdx.x;
    const BodyChunk ch = chunks[slot];
    src += blockIdx.z * bstride;
    wall_batch(wa, blockIdx.z, geo);
    BodyAcc a = BodyAcc::identity();
    if (ch.n > 0) {
        const double x0 = centre[((size_t)blockIdx.z * nbodies + ch.body) * 2], y0 = centre[((size_t)blockIdx.z * nbodies + ch.body) * 2 + 1];
        for (int i = threadIdx.x; i < ch.n; i += BLK) {
            const BodyLink l = links[ch.begin + i];
            const int x = l.x, y = l.yk >> 4, k = l.yk & 15, o = opp(k);
            const R own = src[o * geo.plane + geo.at(x, y)];
            double tx, ty, q = 0.5;
            if constexpr (WALL == WALL_REST) {
                const double f = (double)own;
                tx = (double)(2 * cxk(o)) * f;
                ty = (double)(2 * cyk(o)) * f;
            } else {
                double t;
                if constexpr (WALL == WALL_MOVE) {
                    t = 2.0 * (double)own - link[ch.begin + i];
                } else {
                    const long long row = wa.sh.cell_row[(long long)y * geo.nx + x];
                    t = (double)own + (double)(row >= 0 ? shape_link<R, Geo>(src, geo, wa.sh.ad + row * 16, wa.sh.near[row], k, x, y, own) : own);
                    q = link[ch.begin + i];
                }
                tx = (double)cxk(o) * t;
                ty = (double)cyk(o) * t;
            }
            const double rx = ((double)x - q * (double)cxk(k)) - x0, ry = ((double)y + q * (double)cyk(k)) - y0;
            a.links = a.links + 1.0;
            a.fx = a.fx + tx;
            a.fy = a.fy + ty;
            a.tz = a.tz + (rx * ty + ry * tx);
        }
    }
    red_wave(a);
    if (red_workgroup<BodyAcc, BLK / RED_WAVE>(a, shm)) red_store(partial + slot * BodyAcc::VALS, a);
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

// The tables of the mask, labels and centres of `o` (lbm_bodies.hpp lays them out), built on the host and uploaded into `out`.  hold:
// the hold cells (null: none), at which no link starts.
static int body_tables(lbm_ctx* c, const std::vector<uint8_t>& mask, const Obstacles& o, BodyTables& out, const uint8_t* hold) {
    const BodyParts t = body_parts(mask.data(), o.label.data(), o.centre.data(), c->plan.batch, c->plan.geo.nx, c->plan.geo.ny, o.nbodies, BodyAcc::VALS, REC,
                                   hold);
    if (t.maxchunks > 0x7fffffffu) return fail(c, LBM_ERR_INVALID, "the mask has too many links for the force tables");
    Pack<HipMem> p = upload<HipMem>(t.parts(), "body tables");
    if (!p.err.empty()) return fail(c, p.no_memory ? LBM_ERR_NOMEM : LBM_ERR_HIP, p.err);
    out.links = p.at<const BodyLink>(BodyParts::LINKS);
    out.chunks = p.at<const BodyChunk>(BodyParts::CHUNKS);
    out.first = p.at<const int32_t>(BodyParts::FIRST);
    out.centre = p.at<const double>(BodyParts::CENTRE);
    out.partial = p.at<double>(BodyParts::PARTIAL);
    out.rec = p.at<double>(BodyParts::REC);
    out.maxchunks = (int)t.maxchunks;
    out.base = std::move(p.buf);
    return LBM_OK;
}

// The one writer of c->obs.  `next` holds the new host state of `level` (mask; nbodies, label, centre; motion and wall_uw) and nothing
// else.  The levels below it are reset -- a new mask: one body that holds every solid cell, centred at its centroid, no hold cells, no
// wall velocity; new bodies: every body at rest (the wall velocity per cell stays) -- the tables of everything that changed are built
// aside, and only then does the context change, by moves: on any failure its obstacle state is what it was.  before_commit runs between
// the two (lbm_set_solid, lbm_set_open_cells: the link planes).  The caller has synchronised the streams.  The shape
// (lbm_set_solid_shape) stands beside the motion: ObsLevel::shape replaces or clears it (next.shape_q, every surface at rest: the caller
// checked) and touches nothing else; a new mask drops it; new bodies and a new motion keep q and rebuild its tables, which then carry
// the motion's term -- a shaped context never holds MotionTables.  ObsLevel::motion takes both halves of the wall velocity, the bodies'
// motion and the cells' own (lbm_set_body_motion and lbm_set_wall_velocity each pass the other's as the context holds it; `call`: who,
// for the refusal of the flux check).  ObsLevel::open (lbm_set_open_cells; nothing moves and there is no shape: the caller checked):
// next.hold, next.hold_f and next.open replace the hold cells, and the bodies' tables are rebuilt, since no link starts at a hold cell.
int obstacles_change(lbm_ctx* c, ObsLevel level, Obstacles& next, int (*before_commit)(lbm_ctx*, const Obstacles&), const char* call) {
    Obstacles& cur = c->obs;
    const int B = c->plan.batch, nx = c->plan.geo.nx, ny = c->plan.geo.ny;
    const size_t n = (size_t)nx * ny;
    int rc = LBM_OK;
    if (level == ObsLevel::mask) {
        next.nbodies = 1;
        next.label.resize(B * n);
        for (size_t i = 0; i < B * n; ++i) next.label[i] = next.mask[i] ? 0 : -1;
        next.centre.assign((size_t)B * 2, 0.0);
        for (int b = 0; b < B; ++b) body_centroids(next.mask.data() + b * n, next.label.data() + b * n, nx, ny, 1, next.centre.data() + 2 * b);
    }
    const bool shaped = level != ObsLevel::mask && !cur.shape_q.empty();   // (the levels that keep a shape)
    if (level == ObsLevel::shape) {
        if (!next.shape_q.empty()) {
            next.nbodies = cur.nbodies; next.label = cur.label; next.centre = cur.centre; next.motion = cur.motion;
            rc = shape_tables(c, next, next.shape_q, next.shaped, &next.shape_eff);
        }
        if (rc) return rc;
        cur.shape_q = std::move(next.shape_q);
        cur.shape_eff = std::move(next.shape_eff);
        cur.shaped = std::move(next.shaped);
        return LBM_OK;
    }
    if (level == ObsLevel::open) {
        next.nbodies = cur.nbodies; next.label = cur.label; next.centre = cur.centre;
        rc = body_tables(c, cur.mask, next, next.body, next.hold_or_null());
        if (rc == LBM_OK && before_commit) rc = before_commit(c, next);
        if (rc) return rc;
        sampler_free(c, SMP_FORCE);   // (its link list changed)
        scalar_free(c);               // (geometry: its wall values and hold cells refer to the old one)
        cur.body = std::move(next.body);
        cur.hold = std::move(next.hold);
        cur.hold_f = std::move(next.hold_f);
        cur.open = std::move(next.open);
        cur.per_x = next.per_x;
        cur.per_y = next.per_y;
        cur.hold_all = std::move(next.hold_all);
        return LBM_OK;
    }
    if (level != ObsLevel::motion) {
        next.motion.assign((size_t)B * next.nbodies * 3, 0.0);
        if (level == ObsLevel::bodies) next.wall_uw = cur.wall_uw;   // (a new mask: none)
        rc = body_tables(c, level == ObsLevel::mask ? next.mask : cur.mask, next, next.body, level == ObsLevel::mask ? nullptr : cur.hold_or_null());
        if (rc == LBM_OK && shaped) rc = motion_tables(c, next, next.moving, true, call);
        if (rc == LBM_OK && shaped) rc = shape_tables(c, next, cur.shape_q, next.shaped, &next.shape_eff);
        else if (rc == LBM_OK && level == ObsLevel::bodies) rc = motion_tables(c, next, next.moving, false, call);
    } else {
        next.nbodies = cur.nbodies; next.label = cur.label; next.centre = cur.centre;
        rc = motion_tables(c, next, next.moving, shaped, call);
        if (rc == LBM_OK && shaped) rc = shape_tables(c, next, cur.shape_q, next.shaped, &next.shape_eff);
    }
    if (rc == LBM_OK && before_commit) rc = before_commit(c, next);
    if (rc) return rc;
    if (level == ObsLevel::mask) {
        scalar_free(c);   // (a new mask ends the scalar, as it ends the shape and the hold cells)
        cur.mask = std::move(next.mask);
        cur.shape_q.clear();
        cur.shape_eff.clear();
        cur.shaped = ShapeTables{};
        cur.hold.clear();
        cur.hold_f.clear();
        cur.open = OpenTables{};
        cur.per_x = cur.per_y = false;
        cur.hold_all.clear();
    }
    if (shaped) {
        cur.shape_eff = std::move(next.shape_eff);
        cur.shaped = std::move(next.shaped);
    }
    if (level != ObsLevel::motion) {
        sampler_free(c, SMP_FORCE);   // (its records are per body)
        cur.nbodies = next.nbodies;
        cur.label = std::move(next.label);
        cur.centre = std::move(next.centre);
        cur.body = std::move(next.body);
    }
    cur.motion = std::move(next.motion);
    cur.wall_uw = std::move(next.wall_uw);
    cur.moving = std::move(next.moving);
    return LBM_OK;
}

// One sample from lat[cur], the lattice after c->nsteps steps, into rec[batch][nbodies] on the device; on the compute stream.
static int body_force_enqueue(lbm_ctx* c, double* rec) {
    const BodyTables& t = c->obs.body;
    const int nbodies = c->obs.nbodies;
    return launch_variant(c, [&](auto v) {
        using VT = decltype(v);
        using R = typename VT::R;
        with_wall<VT>(c, [&](auto wa, const double* link) {
            hipLaunchKernelGGL((k_body_force<R, decltype(wa)::MODE>), dim3(t.maxchunks, 1, c->plan.batch), dim3(BLK), 0, c->s_compute,
                               c->lat[c->cur].as<const R>(), c->plan.geo, c->plan.bstride, t.links, t.chunks, t.centre, nbodies, t.partial, wa, link);
        });
        hipLaunchKernelGGL(k_body_force_final, dim3(nbodies, c->plan.batch), dim3(RED_WAVE), 0, c->s_compute, (const double*)t.partial, t.first,
                           t.maxchunks, (double)c->nsteps, rec);
    });
}

// The next sample of the series (lbm_force_sample, and sample_after_unit of the step loop).
int force_series_sample(lbm_ctx* c) {
    void* slot = series_slot(c->obs.force_series);
    if (!slot) return LBM_OK;
    const int rc = body_force_enqueue(c, (double*)slot);
    if (rc) return rc;
    ++c->obs.force_series.count;
    return LBM_OK;
}

// What the calls share: a context with a mask whose lattice holds post-collision populations.
static int force_ready(lbm_ctx* c, const char* call, bool stepped) {
    const int rc = need_solid(c, call);
    if (rc) return rc;
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
    const std::vector<uint8_t>& mask = c->obs.mask;
    const long long bad = body_bad_label(mask.data(), body, B * n, nbodies);
    if (bad >= 0)
        return fail(c, LBM_ERR_INVALID, "lbm_set_solid_bodies: the label of solid cell " + std::to_string(bad) + " is not in [0, nbodies)");
    for (int b = 0; b < B && c->obs.periodic(); ++b) {   // (periodic sides: an image cell belongs to the body of its partner)
        bool lab = false;
        const long long bad_img = periodic_bad_cell(mask.data() + b * n, body + b * n, c->plan.geo.nx, c->plan.geo.ny, c->obs.per_x, c->obs.per_y, &lab);
        if (bad_img >= 0)
            return fail(c, LBM_ERR_INVALID, "lbm_set_solid_bodies: lattice " + std::to_string(b) + ": the body label of image cell " + std::to_string(bad_img) +
                                                " differs from its partner's");
    }
    for (size_t i = 0; centre && i < (size_t)B * nbodies * 2; ++i)
        if (!std::isfinite(centre[i])) return fail(c, LBM_ERR_INVALID, "lbm_set_solid_bodies: a centre is not finite");
    HIP_TRY(c, hipSetDevice(c->p.device));
    rc = sync_all(c);
    if (rc) return rc;
    Obstacles next;
    next.nbodies = nbodies;
    next.label.resize(B * n);
    for (size_t i = 0; i < B * n; ++i) next.label[i] = mask[i] ? body[i] : -1;
    if (centre) next.centre.assign(centre, centre + (size_t)B * nbodies * 2);
    else next.centre.resize((size_t)B * nbodies * 2);
    for (int b = 0; b < B && !centre; ++b)
        body_centroids(mask.data() + b * n, next.label.data() + b * n, c->plan.geo.nx, c->plan.geo.ny, nbodies, next.centre.data() + (size_t)b * nbodies * 2);
    return obstacles_change(c, ObsLevel::bodies, next, nullptr, "lbm_set_solid_bodies");
}

int lbm_get_solid_bodies(lbm_ctx* c, int32_t* body_out, double* centre_out) {
    if (!c) return LBM_ERR_INVALID;
    const int rc = force_ready(c, "lbm_get_solid_bodies", false);
    if (rc) return rc;
    if (body_out) std::memcpy(body_out, c->obs.label.data(), c->obs.label.size() * sizeof(int32_t));
    if (centre_out) std::memcpy(centre_out, c->obs.centre.data(), c->obs.centre.size() * sizeof(double));
    return LBM_OK;
}

int lbm_solid_body_count(lbm_ctx* c) { return c && c->p.semantics == LBM_SEM_BOUNCE_BACK_SOLID ? c->obs.nbodies : 0; }

int lbm_body_force(lbm_ctx* c, lbm_body_force_record* out) {
    if (!c || !out) return fail(c, LBM_ERR_INVALID, "lbm_body_force: bad argument");
    int rc = force_ready(c, "lbm_body_force", true);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->p.device));
    rc = sync_all(c);
    if (rc == LBM_OK) rc = body_force_enqueue(c, c->obs.body.rec);
    if (rc) return rc;
    return records_to_host(c, c->obs.body.rec, (size_t)c->plan.batch * c->obs.nbodies * sizeof(lbm_body_force_record), out);
}

int lbm_force_begin(lbm_ctx* c, int every, int capacity) {
    if (!c || every < 0 || capacity < 1) return fail(c, LBM_ERR_INVALID, "lbm_force_begin: bad argument");
    int rc = force_ready(c, "lbm_force_begin", true);
    if (rc == LBM_OK) rc = sampler_begin(c, SMP_FORCE, every);
    if (rc) return rc;
    sampler_free(c, SMP_FORCE);
    rc = series_alloc(c, c->obs.force_series, (size_t)c->obs.nbodies * sizeof(lbm_body_force_record), capacity, "force series");
    if (rc) return rc;
    c->sampler[SMP_FORCE].arm(c->nsteps, every, 1);
    return LBM_OK;
}

int lbm_force_sample(lbm_ctx* c) {
    if (!c) return LBM_ERR_INVALID;
    if (!c->obs.force_series.dev) return fail(c, LBM_ERR_STATE, "lbm_force_sample: nothing to sample into (lbm_force_begin)");
    int rc = force_ready(c, "lbm_force_sample", true);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->p.device));
    rc = sync_all(c);
    return rc ? rc : force_series_sample(c);
}

int lbm_force_read(lbm_ctx* c, lbm_body_force_record* records_out, int max_records, long long* count, long long* dropped) {
    return series_read(c, [](const lbm_ctx* x) { return &x->obs.force_series; }, "lbm_force_read", records_out, max_records, count, dropped);
}

int lbm_force_end(lbm_ctx* c) { return sampler_end(c, SMP_FORCE); }
}  // extern "C"
