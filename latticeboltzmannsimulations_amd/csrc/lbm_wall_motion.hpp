// lbm_wall_motion.hpp -- the wall velocity of moving bodies (lbm_set_body_motion; contract in include/lbm.h): Ladd's term
// of every link of the list of lbm_bodies.hpp, its sums for the flux check, and the per-cell table the step kernels read; then the tables
// of a whole batch as the device holds them, or the refusal of the flux check (motion_parts).  Arrays are in the host layout of the mask,
// [nx][ny] with y fastest, one lattice at a time.  Plain C++, nothing from HIP: tests/test_body_motion_cpu.py and tests/test_devmem_cpu.py
// drive it from programs of their own.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "lbm_bodies.hpp"

// every product and every sum below is rounded on its own: no fused multiply-add, whatever the compiler's default
#if defined(__clang__)
#define LBM_WM_NO_CONTRACT _Pragma("clang fp contract(off)")
#define LBM_WM_ATTR
#elif defined(__GNUC__)
#define LBM_WM_NO_CONTRACT
#define LBM_WM_ATTR __attribute__((optimize("fp-contract=off")))
#else
#define LBM_WM_NO_CONTRACT
#define LBM_WM_ATTR
#endif

namespace lbmhost {

// delta of the link (cell (x, y), slot k) of a body with the centre (x0, y0) and the motion (Ux, Uy, Om): 6 w_k (c_k . u_w) at rho_0 = 1,
// u_w the body's velocity at the link's midpoint -- the midpoint of tz, (rx, ry) = (x - cx_k / 2 - x0, y + cy_k / 2 - y0):
//     uwx = Ux + Om ry;  uwy = Uy + Om rx;  delta = (6 w_k) (cx_k uwx + cy_k uwy),        6 w_k = 2/3 (k <= 4) or 1/6, rounded once.
// Ux, Uy in the components of u (Uy > 0 points to the lid); Om counter-clockwise positive in the frame drawn with the lid on top.
LBM_WM_ATTR inline double wall_delta(int x, int y, int k, double x0, double y0, double Ux, double Uy, double Om) {
    LBM_WM_NO_CONTRACT
    const double rx = ((double)x - 0.5 * (double)BODY_CX[k]) - x0, ry = ((double)y + 0.5 * (double)BODY_CY[k]) - y0;
    const double uwx = Ux + Om * ry, uwy = Uy + Om * rx;
    const double w6 = k < 5 ? 2.0 / 3.0 : 1.0 / 6.0;
    return w6 * ((double)BODY_CX[k] * uwx + (double)BODY_CY[k] * uwy);
}

// The wall velocity of a solid cell (lbm_set_wall_velocity): what the source cell S = (x - cx_k, y + cy_k) of a link adds to the link's
// delta, (6 w_k) (cx_k uwx(S) + cy_k uwy(S)), every product and sum rounded in the order written, 6 w_k as wall_delta rounds it.  The
// link's delta is then wall_delta(...) + wall_cell_term(...), one more add.
LBM_WM_ATTR inline double wall_cell_term(int k, double uwx, double uwy) {
    LBM_WM_NO_CONTRACT
    const double w6 = k < 5 ? 2.0 / 3.0 : 1.0 / 6.0;
    return w6 * ((double)BODY_CX[k] * uwx + (double)BODY_CY[k] * uwy);
}
// ... of the link (cell (x, y), slot k) from uw[2][nx][ny] of its lattice (the components as u, the host layout of the mask)
inline double wall_cell_term_at(const double* uw, int nx, int ny, int x, int y, int k) {
    const size_t s = (size_t)(x - BODY_CX[k]) * ny + (size_t)(y + BODY_CY[k]);
    return wall_cell_term(k, uw[s], uw[(size_t)nx * ny + s]);
}

// delta as the lattice holds it: rounded once to the lattice type, then a double again (what the force subtracts)
inline double wall_delta_rounded(double d, bool f32) { return f32 ? (double)(float)d : d; }

// What lbm_set_body_motion derives for one lattice.
struct WallMotion {
    std::vector<double> delta;      // per link, in the order of the list, in double (not yet rounded to the lattice type)
    double S = 0.0, A = 0.0;        // sum of delta and of |delta| over the list, in its order: the net flux through the links and its scale
    std::vector<int32_t> cell_row;  // [ny][nx], x fastest (as the lattice's rows): -1, or the row of the cell in `rows`
    std::vector<double> rows;       // [rows][8]: slot k - 1 holds the delta of the cell's link k, 0 where it has none
};

// links[start[0] .. start[nbodies]) of one lattice (body_links), centre[nbodies][2], motion[nbodies][3] = (Ux, Uy, Om).  row_base: the
// rows of this lattice follow that many rows of the lattices before it (a batch shares one table).  uw (null: none): the wall velocity
// per solid cell of this lattice, uw[2][nx][ny], whose term every link adds to the rigid-body one (wall_cell_term).
LBM_WM_ATTR inline WallMotion wall_motion(const std::vector<BodyLink>& links, const long long* start, int nx, int ny, int nbodies, const double* centre,
                                          const double* motion, long long row_base = 0, const double* uw = nullptr) {
    LBM_WM_NO_CONTRACT
    WallMotion m;
    m.delta.resize((size_t)(start[nbodies] - start[0]));
    m.cell_row.assign((size_t)nx * ny, -1);
    long long nrows = 0;
    for (int b = 0; b < nbodies; ++b)
        for (long long i = start[b]; i < start[b + 1]; ++i) {
            const int x = links[(size_t)i].x, y = links[(size_t)i].yk >> 4, k = links[(size_t)i].yk & 15;
            double d = wall_delta(x, y, k, centre[2 * b], centre[2 * b + 1], motion[3 * b], motion[3 * b + 1], motion[3 * b + 2]);
            if (uw) d = d + wall_cell_term_at(uw, nx, ny, x, y, k);
            m.delta[(size_t)(i - start[0])] = d;
            m.S = m.S + d;
            m.A = m.A + std::fabs(d);
            int32_t& row = m.cell_row[(size_t)y * nx + x];
            if (row < 0) {
                row = (int32_t)(row_base + nrows++);
                m.rows.resize((size_t)nrows * 8, 0.0);
            }
            m.rows[(size_t)(row - row_base) * 8 + (k - 1)] = d;
        }
    return m;
}

// The flux check: in exact arithmetic S = 0 whenever no two touching bodies move differently and no moving body pumps through the
// lattice's edge (the discrete divergence theorem); the rounding of the sum stays below links * 2^-52 * A, and one leaking link is a
// whole delta.  True: the motion conserves the lattice's mass.
inline bool wall_motion_closed(const WallMotion& m) { return !(std::fabs(m.S) > (double)m.delta.size() * 0x1p-52 * m.A); }

// The tables of a nonzero motion of a whole batch (mask and label [batch][nx][ny], centre[batch][nbodies][2], motion[batch][nbodies][3])
// as the device holds them in one allocation: cell_row[batch][ny][nx]; delta[rows][8], already rounded to the lattice type (f32: float);
// link_delta, one double per entry of the batch's link list (body_parts), the same terms as the lattice adds them.  Or why there are
// none: the first lattice whose motion fails the flux check, with its sums and its count of links, or too many rows for cell_row.
// hold[batch][nx][ny] (null: none): the hold cells of lbm_set_open_cells -- no link starts at one (body_links), and a lattice that has
// one is open: the flux check is waived for it.  uw[batch][2][nx][ny] (null: none): the wall velocity per solid cell (wall_motion).
struct MotionParts {
    enum { CELL_ROW, DELTA, LINK_DELTA };
    enum Refusal { NONE, OPEN_FLUX, TOO_MANY_ROWS };
    std::vector<int32_t> cell_row;
    std::vector<char> delta;
    std::vector<double> link_delta;
    Refusal refusal = NONE;
    int lattice = 0;                // OPEN_FLUX: which lattice, and its S, A and links
    double S = 0.0, A = 0.0;
    size_t links = 0;
    std::vector<Part> parts() const {
        return {{cell_row.data(), cell_row.size() * sizeof(int32_t)}, {delta.data(), delta.size()}, {link_delta.data(), link_delta.size() * sizeof(double)}};
    }
};
inline MotionParts motion_parts(const uint8_t* mask, const int32_t* label, const double* centre, const double* motion, int batch, int nx, int ny,
                                int nbodies, bool f32, const uint8_t* hold = nullptr, const double* uw = nullptr) {
    const size_t n = (size_t)nx * ny;
    MotionParts t;
    t.cell_row.resize(batch * n);
    std::vector<double> rows;
    for (int b = 0; b < batch; ++b) {
        std::vector<BodyLink> links;
        std::vector<long long> start((size_t)nbodies + 1);
        const uint8_t* h = hold ? hold + b * n : nullptr;
        body_links(mask + b * n, label + b * n, nx, ny, nbodies, links, start.data(), h);
        const WallMotion m = wall_motion(links, start.data(), nx, ny, nbodies, centre + (size_t)b * nbodies * 2, motion + (size_t)b * nbodies * 3,
                                         (long long)(rows.size() / 8), uw ? uw + (size_t)b * 2 * n : nullptr);
        const bool open = h && std::any_of(h, h + n, [](uint8_t v) { return v != 0; });
        if (!open && !wall_motion_closed(m)) {
            t.refusal = MotionParts::OPEN_FLUX; t.lattice = b; t.S = m.S; t.A = m.A; t.links = m.delta.size();
            return t;
        }
        if (rows.size() / 8 + m.rows.size() / 8 > 0x7fffffffu) {
            t.refusal = MotionParts::TOO_MANY_ROWS;
            return t;
        }
        std::copy(m.cell_row.begin(), m.cell_row.end(), t.cell_row.begin() + b * n);
        rows.insert(rows.end(), m.rows.begin(), m.rows.end());
        for (double d : m.delta) t.link_delta.push_back(wall_delta_rounded(d, f32));
    }
    t.delta.resize(rows.size() * (f32 ? sizeof(float) : sizeof(double)));
    for (size_t i = 0; i < rows.size(); ++i) {
        if (f32) ((float*)t.delta.data())[i] = (float)rows[i];
        else ((double*)t.delta.data())[i] = rows[i];
    }
    return t;
}
}  // namespace lbmhost
