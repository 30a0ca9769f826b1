// lbm_body_shape.hip -- liblbm_hip.so: curved obstacle surfaces (lbm_set_solid_shape, lbm_get_solid_shape of the C ABI declared in
// include/lbm.h; LBM_SEM_BOUNCE_BACK_SOLID).  Every link carries the fraction q of its length at which the wall sits; the coefficients of
// the interpolated bounce-back and the moving-wall term at the wall point are built on the host (lbm_wall_shape.hpp) and uploaded here and
// in the other set_* calls, never inside lbm_step.  The step kernels that apply the rule are k_step_solid / k_step_generic_wall in their mode
// WALL_SHAPE (lbm_solid.hpp), the readers see it through Fields (lbm_fields.hpp), the force kernels are k_solid_force / k_body_force in the
// same mode; with_wall (lbm_host.hpp) picks it only while a shape is set.  gfx950 only.  DESIGN.md 2.10.
#include <cmath>

#include "lbm_host.hpp"
#include "lbm_wall_shape.hpp"

namespace lbmhost {

// The tables of the shape q over the mask the context holds and the labels, centres and motion of `next` (lbm_wall_shape.hpp lays them
// out, link_q in the order of the link list the device holds: body_tables), uploaded into `out`; *q_eff: the effective q.
int shape_tables(lbm_ctx* c, const Obstacles& next, const std::vector<double>& q, ShapeTables& out, std::vector<double>* q_eff) {
    ShapeParts t = shape_parts(c->obs.mask.data(), next.label.data(), next.centre.data(), next.motion.data(), q.data(), c->plan.batch, c->plan.geo.nx,
                               c->plan.geo.ny, next.nbodies, c->plan.es == 4, c->obs.hold_or_null(), next.uw_or_null());
    if (t.too_many_rows) return fail(c, LBM_ERR_INVALID, "lbm_set_solid_shape: too many cells with links");
    Pack<HipMem> p = upload<HipMem>(t.parts(), "solid shape tables");
    if (!p.err.empty()) return fail(c, p.no_memory ? LBM_ERR_NOMEM : LBM_ERR_HIP, p.err);
    out.cell_row = p.at<const int32_t>(ShapeParts::CELL_ROW);
    out.ad = p.at<const void>(ShapeParts::AD);
    out.near = p.at<const uint8_t>(ShapeParts::NEAR);
    out.link_q = p.at<const double>(ShapeParts::LINK_Q);
    out.base = std::move(p.buf);
    *q_eff = std::move(t.q_eff);
    return LBM_OK;
}
}  // namespace lbmhost

using namespace lbmhost;

extern "C" {

int lbm_set_solid_shape(lbm_ctx* c, const double* q) {
    if (!c) return LBM_ERR_INVALID;
    int rc = need_solid(c, "lbm_set_solid_shape");
    if (rc) return rc;
    if (c->plan.solid_tiles)
        return fail(c, LBM_ERR_STATE, "lbm_set_solid_shape: the tile kernel keeps the half-way rule (LBM_FLAG_SOLID_TILES takes no shape; create the "
                                      "context without the flag)");
    if (c->obs.moves())
        return fail(c, LBM_ERR_STATE, "lbm_set_solid_shape: a body motion or a wall velocity is set (the shape is set or cleared while every surface "
                                      "is at rest: the shape first, then lbm_set_body_motion and lbm_set_wall_velocity)");
    if (q && c->scalar.buoyant)
        return fail(c, LBM_ERR_STATE, "lbm_set_solid_shape: buoyancy is set (the shaped kernels add no buoyancy; clear it with lbm_set_buoyancy(c, 0, 0, 0) "
                                      "first)");
    const Geo& g = c->plan.geo;
    Obstacles next;
    if (q) {
        ShapeBad bad;
        if (shape_bad_link(c->obs.mask.data(), q, c->plan.batch, g.nx, g.ny, &bad)) {
            char text[256];
            std::snprintf(text, sizeof text, "lbm_set_solid_shape: lattice %d: q = %.17g on the link of cell (%d, %d), slot %d is not a finite value in (0, 1]",
                          bad.lattice, bad.q, bad.x, bad.y, bad.k);
            return fail(c, LBM_ERR_INVALID, text);
        }
        next.shape_q.assign(q, q + (size_t)c->plan.batch * 8 * g.nx * g.ny);
    }
    HIP_TRY(c, hipSetDevice(c->p.device));
    rc = sync_all(c);
    return rc ? rc : obstacles_change(c, ObsLevel::shape, next);
}

int lbm_get_solid_shape(lbm_ctx* c, double* q_out) {
    if (!c || !q_out) return fail(c, LBM_ERR_INVALID, "lbm_get_solid_shape: bad argument");
    const int rc = need_solid(c, "lbm_get_solid_shape");
    if (rc) return rc;
    const size_t n = (size_t)c->plan.batch * 8 * c->plan.geo.nx * c->plan.geo.ny;
    if (c->obs.shape_eff.empty()) std::memset(q_out, 0, n * sizeof(double));
    else std::memcpy(q_out, c->obs.shape_eff.data(), n * sizeof(double));
    return LBM_OK;
}
}  // extern "C"
