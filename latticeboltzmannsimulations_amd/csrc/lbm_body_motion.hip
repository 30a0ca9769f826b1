// lbm_body_motion.hip -- liblbm_hip.so: the wall velocity of moving bodies and of single solid cells (lbm_set_body_motion,
// lbm_get_body_motion, lbm_set_wall_velocity, lbm_get_wall_velocity of the C ABI declared in include/lbm.h; LBM_SEM_BOUNCE_BACK_SOLID).  A body keeps its cells and its surface moves: every link carries Ladd's term, a constant
// of the link, built on the host (lbm_wall_motion.hpp) and uploaded here, never inside lbm_step.  The step kernels that add it are
// k_step_solid / k_step_generic_wall in their mode WALL_MOVE (lbm_solid.hpp), the force kernels that subtract it k_solid_force / k_body_force
// in the same mode; with_wall (lbm_host.hpp) picks it only while a nonzero motion is set.  gfx950 only.  DESIGN.md 2.10.
#include <cmath>

#include "lbm_host.hpp"
#include "lbm_wall_motion.hpp"

namespace lbmhost {

// The tables of next.motion and next.wall_uw over the mask and the hold cells the context holds and the labels and centres of `next`
// (lbm_wall_motion.hpp lays them out, in the order of the link list the device holds: body_tables), uploaded into `out`; every surface at
// rest: none, and `out` stays empty.  check_only (a context with a shape, whose own table carries the term): the flux check alone, formed
// from the deltas at the links' midpoints.  call: the name in front of a refusal.
int motion_tables(lbm_ctx* c, const Obstacles& next, MotionTables& out, bool check_only, const char* call) {
    if (!next.moves()) return LBM_OK;
    const Obstacles& o = c->obs;
    const MotionParts t = motion_parts(o.mask.data(), next.label.data(), next.centre.data(), next.motion.data(), c->plan.batch, c->plan.geo.nx,
                                       c->plan.geo.ny, next.nbodies, c->plan.es == 4, o.hold_or_null(), next.uw_or_null());
    if (t.refusal == MotionParts::OPEN_FLUX) {
        char text[360];
        std::snprintf(text, sizeof text,
                      "%s: lattice %d: the motion has a net flux of %.6g through its %zu links (sum of |delta| %.6g): a moving "
                      "body pumps through a wall, or two touching bodies move differently, and the cavity would not keep its mass",
                      call, t.lattice, t.S, t.links, t.A);
        return fail(c, LBM_ERR_INVALID, text);
    }
    if (t.refusal == MotionParts::TOO_MANY_ROWS) return fail(c, LBM_ERR_INVALID, std::string(call) + ": too many cells with links");
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
    next.wall_uw = c->obs.wall_uw;   // (the other half of the one table)
    HIP_TRY(c, hipSetDevice(c->p.device));
    rc = sync_all(c);
    return rc ? rc : obstacles_change(c, ObsLevel::motion, next, nullptr, "lbm_set_body_motion");
}

int lbm_get_body_motion(lbm_ctx* c, double* motion_out) {
    if (!c || !motion_out) return fail(c, LBM_ERR_INVALID, "lbm_get_body_motion: bad argument");
    const int rc = need_solid(c, "lbm_get_body_motion");
    if (rc) return rc;
    std::memcpy(motion_out, c->obs.motion.data(), c->obs.motion.size() * sizeof(double));
    return LBM_OK;
}

int lbm_set_wall_velocity(lbm_ctx* c, const double* uw) {
    if (!c) return LBM_ERR_INVALID;
    int rc = need_solid(c, "lbm_set_wall_velocity");
    if (rc) return rc;
    const size_t n = (size_t)c->plan.geo.nx * c->plan.geo.ny, B = (size_t)c->plan.batch;
    Obstacles next;
    bool moving = false;
    if (uw) {   // (read on solid cells only; stored as zero elsewhere)
        next.wall_uw.assign(B * 2 * n, 0.0);
        for (size_t b = 0; b < B; ++b)
            for (size_t j = 0; j < 2; ++j)
                for (size_t i = 0; i < n; ++i) {
                    if (!c->obs.mask[b * n + i]) continue;
                    const double v = uw[(b * 2 + j) * n + i];
                    if (!std::isfinite(v)) return fail(c, LBM_ERR_INVALID, "lbm_set_wall_velocity: a velocity of a solid cell is not finite");
                    next.wall_uw[(b * 2 + j) * n + i] = v;
                    moving = moving || v != 0.0;
                }
    }
    if (!moving) next.wall_uw.clear();   // (all zero: no term, and with every body at rest no table)
    if (moving && c->plan.solid_tiles)
        return fail(c, LBM_ERR_STATE, "lbm_set_wall_velocity: the tile kernel keeps obstacles at rest (LBM_FLAG_SOLID_TILES takes no nonzero wall "
                                      "velocity; create the context without the flag)");
    next.motion = c->obs.motion;   // (the other half of the one table)
    HIP_TRY(c, hipSetDevice(c->p.device));
    rc = sync_all(c);
    return rc ? rc : obstacles_change(c, ObsLevel::motion, next, nullptr, "lbm_set_wall_velocity");
}

int lbm_get_wall_velocity(lbm_ctx* c, double* uw_out) {
    if (!c || !uw_out) return fail(c, LBM_ERR_INVALID, "lbm_get_wall_velocity: bad argument");
    const int rc = need_solid(c, "lbm_get_wall_velocity");
    if (rc) return rc;
    const size_t n = (size_t)c->plan.batch * 2 * c->plan.geo.nx * c->plan.geo.ny;
    if (c->obs.wall_uw.empty()) std::memset(uw_out, 0, n * sizeof(double));
    else std::memcpy(uw_out, c->obs.wall_uw.data(), n * sizeof(double));
    return LBM_OK;
}
}  // extern "C"
