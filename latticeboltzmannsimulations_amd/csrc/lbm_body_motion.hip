// lbm_body_motion.hip -- liblbm_hip.so: the wall velocity of moving bodies (lbm_set_body_motion, lbm_get_body_motion of the C ABI declared
// in include/lbm.h; LBM_SEM_BOUNCE_BACK_SOLID).  A body keeps its cells and its surface moves: every link carries Ladd's term, a constant
// of the link, built on the host (lbm_wall_motion.hpp) and uploaded here, never inside lbm_step.  The step kernels that add it are
// k_step_solid_move / k_step_generic_move (lbm_solid_move.hpp), the force kernels that subtract it k_solid_force_move / k_body_force_move;
// all of them run only while a nonzero motion is set.  gfx950 only.  DESIGN.md 2.10.
#include <cmath>

#include "lbm_host.hpp"
#include "lbm_wall_motion.hpp"

namespace lbmhost {

// Every body at rest: the tables are freed and the step and the force return to the kernels of obstacles at rest.  The caller has
// synchronised the streams.
void motion_rest(lbm_ctx* c) {
    if (c->motion.base) (void)hipFree(c->motion.base);
    c->motion = MotionTables{};
    c->body_motion.assign(c->p.semantics == LBM_SEM_BOUNCE_BACK_SOLID ? (size_t)c->plan.batch * c->nbodies * 3 : 0, 0.0);
}

template <typename R>
static void round_rows(const std::vector<double>& rows, std::vector<char>& out) {
    out.resize(rows.size() * sizeof(R));
    R* o = (R*)out.data();
    for (size_t i = 0; i < rows.size(); ++i) o[i] = (R)rows[i];
}
}  // namespace lbmhost

using namespace lbmhost;

extern "C" {

int lbm_set_body_motion(lbm_ctx* c, const double* motion) {
    if (!c) return LBM_ERR_INVALID;
    if (c->p.semantics != LBM_SEM_BOUNCE_BACK_SOLID)
        return fail(c, LBM_ERR_STATE, "lbm_set_body_motion: this context has no solid mask (create it with semantics = LBM_SEM_BOUNCE_BACK_SOLID)");
    const int B = c->plan.batch, nb = c->nbodies, nx = c->plan.geo.nx, ny = c->plan.geo.ny;
    const size_t n = (size_t)nx * ny, nm = (size_t)B * nb * 3;
    bool moving = false;
    for (size_t i = 0; motion && i < nm; ++i) {
        if (!std::isfinite(motion[i])) return fail(c, LBM_ERR_INVALID, "lbm_set_body_motion: a velocity or a rotation rate is not finite");
        moving = moving || motion[i] != 0.0;
    }
    if (moving && c->plan.solid_tiles)
        return fail(c, LBM_ERR_STATE, "lbm_set_body_motion: the tile kernel keeps obstacles at rest (LBM_FLAG_SOLID_TILES takes no nonzero motion; "
                                      "create the context without the flag)");
    HIP_TRY(c, hipSetDevice(c->p.device));
    int rc = sync_all(c);
    if (rc) return rc;
    if (!moving) {
        motion_rest(c);
        return LBM_OK;
    }
    // the tables of every lattice, in the order of the link list the device holds (bodies_upload)
    const bool f32 = c->plan.es == 4;
    std::vector<int32_t> cell_row(B * n);
    std::vector<double> rows, link_delta;
    for (int b = 0; b < B; ++b) {
        std::vector<BodyLink> links;
        std::vector<long long> start((size_t)nb + 1);
        body_links(c->solid_mask.data() + b * n, c->body_label.data() + b * n, nx, ny, nb, links, start.data());
        const WallMotion m = wall_motion(links, start.data(), nx, ny, nb, c->body_centre.data() + (size_t)b * nb * 2, motion + (size_t)b * nb * 3,
                                         (long long)(rows.size() / 8));
        if (!wall_motion_closed(m)) {
            char text[320];
            std::snprintf(text, sizeof text,
                          "lbm_set_body_motion: lattice %d: the motion has a net flux of %.6g through its %zu links (sum of |delta| %.6g): a moving "
                          "body pumps through a wall, or two touching bodies move differently, and the cavity would not keep its mass",
                          b, m.S, m.delta.size(), m.A);
            return fail(c, LBM_ERR_INVALID, text);
        }
        if (rows.size() / 8 + m.rows.size() / 8 > 0x7fffffffu) return fail(c, LBM_ERR_INVALID, "lbm_set_body_motion: too many cells with links");
        std::copy(m.cell_row.begin(), m.cell_row.end(), cell_row.begin() + b * n);
        rows.insert(rows.end(), m.rows.begin(), m.rows.end());
        for (double d : m.delta) link_delta.push_back(wall_delta_rounded(d, f32));
    }
    std::vector<char> delta;
    if (f32) round_rows<float>(rows, delta);
    else round_rows<double>(rows, delta);
    auto pad16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t o_delta = pad16(cell_row.size() * sizeof(int32_t)), o_link = o_delta + pad16(std::max<size_t>(16, delta.size())),
                 bytes = o_link + std::max<size_t>(16, link_delta.size() * sizeof(double));
    char* base = nullptr;
    hipError_t e = hipMalloc((void**)&base, bytes);
    if (e != hipSuccess) return fail(c, LBM_ERR_NOMEM, std::string("hipMalloc(body motion tables): ") + hipGetErrorString(e));
    e = hipMemcpy(base, cell_row.data(), cell_row.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && !delta.empty()) e = hipMemcpy(base + o_delta, delta.data(), delta.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && !link_delta.empty()) e = hipMemcpy(base + o_link, link_delta.data(), link_delta.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(base);
        return fail(c, LBM_ERR_HIP, std::string("hipMemcpy(body motion tables): ") + hipGetErrorString(e));
    }
    motion_rest(c);
    c->body_motion.assign(motion, motion + nm);
    c->motion.base = base;
    c->motion.cell_row = (const int32_t*)base;
    c->motion.delta = base + o_delta;
    c->motion.link_delta = (const double*)(base + o_link);
    return LBM_OK;
}

int lbm_get_body_motion(lbm_ctx* c, double* motion_out) {
    if (!c || !motion_out) return fail(c, LBM_ERR_INVALID, "lbm_get_body_motion: bad argument");
    if (c->p.semantics != LBM_SEM_BOUNCE_BACK_SOLID)
        return fail(c, LBM_ERR_STATE, "lbm_get_body_motion: this context has no solid mask (create it with semantics = LBM_SEM_BOUNCE_BACK_SOLID)");
    std::memcpy(motion_out, c->body_motion.data(), c->body_motion.size() * sizeof(double));
    return LBM_OK;
}
}  // extern "C"
