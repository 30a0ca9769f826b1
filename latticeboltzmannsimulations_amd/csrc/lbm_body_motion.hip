// lbm_body_motion.hip -- liblbm_hip.so: the wall velocity of moving bodies (lbm_set_body_motion, lbm_get_body_motion of the C ABI declared
// in include/lbm.h; LBM_SEM_BOUNCE_BACK_SOLID).  A body keeps its cells and its surface moves: every link carries Ladd's term, a constant
// of the link, built on the host (lbm_wall_motion.hpp) and uploaded here, never inside lbm_step.  The step kernels that add it are
// k_step_solid / k_step_generic_wall in their mode WALL_MOVE (lbm_solid.hpp), the force kernels that subtract it k_solid_force / k_body_force
// in the same mode; with_wall (lbm_host.hpp) picks it only while a nonzero motion is set.  gfx950 only.  DESIGN.md 2.10.
#include <cmath>

#include "lbm_host.hpp"
#include "lbm_wall_motion.hpp"

namespace lbmhost {

// The tables of next.motion over the mask, the labels and the centres the context holds (lbm_wall_motion.hpp lays them out, in the order
// of the link list the device holds: body_tables), uploaded into `out`; every body at rest: none, and `out` stays empty.  check_only (a
// context with a shape, whose own table carries the term): the flux check alone, formed from the deltas at the links' midpoints.
int motion_tables(lbm_ctx* c, const Obstacles& next, MotionTables& out, bool check_only) {
    if (std::all_of(next.motion.begin(), next.motion.end(), [](double v) { return v == 0.0; })) return LBM_OK;
    const Obstacles& o = c->obs;
    const MotionParts t = motion_parts(o.mask.data(), o.label.data(), o.centre.data(), next.motion.data(), c->plan.batch, c->plan.geo.nx, c->plan.geo.ny,
                                       o.nbodies, c->plan.es == 4);
    if (t.refusal == MotionParts::OPEN_FLUX) {
        char text[320];
        std::snprintf(text, sizeof text,
                      "lbm_set_body_motion: lattice %d: the motion has a net flux of %.6g through its %zu links (sum of |delta| %.6g): a moving "
                      "body pumps through a wall, or two touching bodies move differently, and the cavity would not keep its mass",
                      t.lattice, t.S, t.links, t.A);
        return fail(c, LBM_ERR_INVALID, text);
    }
    if (t.refusal == MotionParts::TOO_MANY_ROWS) return fail(c, LBM_ERR_INVALID, "lbm_set_body_motion: too many cells with links");
    if (check_only) return LBM_OK;
    Pack<HipMem> p = upload<HipMem>(t.parts(), "body motion tables");
    if (!p.err.empty()) return fail(c, p.no_memory ? LBM_ERR_NOMEM : LBM_ERR_HIP, p.err);
    out.cell_row = p.at<const int32_t>(MotionParts::CELL_ROW);
    out.delta = p.at<const void>(MotionParts::DELTA);
    out.link_delta = p.at<const double>(MotionParts::LINK_DELTA);
    out.base = std::move(p.buf);
    return LBM_OK;
}
}  // namespace lbmhost

using namespace lbmhost;

extern "C" {

int lbm_set_body_motion(lbm_ctx* c, const double* motion) {
    if (!c) return LBM_ERR_INVALID;
    int rc = need_solid(c, "lbm_set_body_motion");
    if (rc) return rc;
    const size_t nm = (size_t)c->plan.batch * c->obs.nbodies * 3;
    Obstacles next;
    next.motion.assign(nm, 0.0);   // (no motion given: every body at rest)
    if (motion) next.motion.assign(motion, motion + nm);
    bool moving = false;
    for (double v : next.motion) {
        if (!std::isfinite(v)) return fail(c, LBM_ERR_INVALID, "lbm_set_body_motion: a velocity or a rotation rate is not finite");
        moving = moving || v != 0.0;
    }
    if (moving && c->plan.solid_tiles)
        return fail(c, LBM_ERR_STATE, "lbm_set_body_motion: the tile kernel keeps obstacles at rest (LBM_FLAG_SOLID_TILES takes no nonzero motion; "
                                      "create the context without the flag)");
    HIP_TRY(c, hipSetDevice(c->p.device));
    rc = sync_all(c);
    return rc ? rc : obstacles_change(c, ObsLevel::motion, next);
}

int lbm_get_body_motion(lbm_ctx* c, double* motion_out) {
    if (!c || !motion_out) return fail(c, LBM_ERR_INVALID, "lbm_get_body_motion: bad argument");
    const int rc = need_solid(c, "lbm_get_body_motion");
    if (rc) return rc;
    std::memcpy(motion_out, c->obs.motion.data(), c->obs.motion.size() * sizeof(double));
    return LBM_OK;
}
}  // extern "C"
