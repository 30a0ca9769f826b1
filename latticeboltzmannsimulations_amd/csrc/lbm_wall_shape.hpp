// lbm_wall_shape.hpp -- curved obstacle surfaces (lbm_set_solid_shape; contract in include/lbm.h): from the wall distance
// q of every link of the list of lbm_bodies.hpp, the coefficients of the interpolated bounce-back (a, near), the wall point, the
// moving-wall term there (d), the per-cell table the step kernels and the gathers read, and the per-link distances of the torque; then
// the tables of a whole batch as the device holds them (shape_parts).  Arrays are in the host layout of the mask, [nx][ny] with y fastest;
// q is q[batch][8][nx][ny], plane k - 1 for slot k.  Plain C++, nothing from HIP: tests/test_solid_shape_cpu.py drives it from a program of
// its own.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "lbm_wall_motion.hpp"

namespace lbmhost {

// What one link (cell (x, y), slot k) of a body with the centre (x0, y0) and the motion (Ux, Uy, Om) derives from its q, in double, every
// operation rounded in the order written:
//     near = q < 1/2 and the next cell N = (x + cx_k, y - cy_k) is a fluid cell inside the lattice (next_fluid);
//     q < 1/2 without such a cell: the effective q is 1/2 (the half-way rule);
//     a = near ? 2 q : 1 / (2 q)
//     (rx, ry) = ((x - q cx_k) - x0, (y + q cy_k) - y0)              the wall point; at q = 1/2 the bits of wall_delta's midpoint
//     delta = (6 w_k) (cx_k uwx + cy_k uwy),  uwx = Ux + Om ry,  uwy = Uy + Om rx        as wall_delta forms it
//     d = near ? delta : a delta
struct ShapeLink {
    double q, a, d, rx, ry;
    bool near;
};
// cell (null: none): the term of the source cell's own wall velocity (wall_cell_term, lbm_wall_motion.hpp), added to delta before d.
LBM_WM_ATTR inline ShapeLink shape_link(int x, int y, int k, double q, bool next_fluid, double x0, double y0, double Ux, double Uy, double Om,
                                        const double* cell = nullptr) {
    LBM_WM_NO_CONTRACT
    ShapeLink l;
    l.near = q < 0.5 && next_fluid;
    l.q = (q < 0.5 && !next_fluid) ? 0.5 : q;
    l.a = l.near ? 2.0 * l.q : 1.0 / (2.0 * l.q);
    l.rx = ((double)x - l.q * (double)BODY_CX[k]) - x0;
    l.ry = ((double)y + l.q * (double)BODY_CY[k]) - y0;
    const double uwx = Ux + Om * l.ry, uwy = Uy + Om * l.rx;
    const double w6 = k < 5 ? 2.0 / 3.0 : 1.0 / 6.0;
    double delta = w6 * ((double)BODY_CX[k] * uwx + (double)BODY_CY[k] * uwy);
    if (cell) delta = delta + *cell;
    l.d = l.near ? delta : l.a * delta;
    return l;
}

inline size_t shape_q_index(int b, int k, int x, int y, int nx, int ny) { return (((size_t)b * 8 + (size_t)(k - 1)) * nx + x) * ny + y; }

// The first link whose q is not a finite value in (0, 1], lattices in order, cells in [y][x] order, then k: true, and where.
struct ShapeBad {
    int lattice, x, y, k;
    double q;
};
inline bool shape_bad_link(const uint8_t* mask, const double* q, int batch, int nx, int ny, ShapeBad* bad) {
    const size_t n = (size_t)nx * ny;
    for (int b = 0; b < batch; ++b) {
        const uint8_t* m = mask + b * n;
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                if (m[(size_t)x * ny + y]) continue;
                for (int k = 1; k < 9; ++k) {
                    const int sx = x - BODY_CX[k], sy = y + BODY_CY[k];
                    if (sx < 0 || sx >= nx || sy < 0 || sy >= ny || !m[(size_t)sx * ny + sy]) continue;
                    const double v = q[shape_q_index(b, k, x, y, nx, ny)];
                    if (!(std::isfinite(v) && v > 0.0 && v <= 1.0)) {
                        *bad = ShapeBad{b, x, y, k, v};
                        return true;
                    }
                }
            }
    }
    return false;
}

// The tables of a shape over a whole batch (mask and label [batch][nx][ny], centre[batch][nbodies][2], motion[batch][nbodies][3],
// q[batch][8][nx][ny]) as the device holds them in one allocation: cell_row[batch][ny][nx], -1 or the cell's row; ad[rows][16], already
// rounded to the lattice type (f32: float), a in slots 0 .. 7 (1 where the cell has no link k), d in slots 8 .. 15; near[rows], bit
// k - 1; link_q, the effective q of every entry of the batch's link list (body_parts), for the wall point of the torque.  q_eff: what
// lbm_get_solid_shape returns, the effective q on the links and 0 elsewhere (host only).  too_many_rows: no tables.
// hold[batch][nx][ny] (null: none): the hold cells of lbm_set_open_cells, no fluid cells -- no link starts at one and none is a link's
// next fluid cell.  uw[batch][2][nx][ny] (null: none): the wall velocity per solid cell, whose term joins delta.
struct ShapeParts {
    enum { CELL_ROW, AD, NEAR, LINK_Q };
    std::vector<int32_t> cell_row;
    std::vector<char> ad;
    std::vector<uint8_t> near;
    std::vector<double> link_q;
    std::vector<double> q_eff;
    bool too_many_rows = false;
    std::vector<Part> parts() const {
        return {{cell_row.data(), cell_row.size() * sizeof(int32_t)}, {ad.data(), ad.size()}, {near.data(), near.size()},
                {link_q.data(), link_q.size() * sizeof(double)}};
    }
};
inline ShapeParts shape_parts(const uint8_t* mask, const int32_t* label, const double* centre, const double* motion, const double* q, int batch,
                              int nx, int ny, int nbodies, bool f32, const uint8_t* hold = nullptr, const double* uw = nullptr) {
    const size_t n = (size_t)nx * ny;
    ShapeParts t;
    t.cell_row.assign(batch * n, -1);
    t.q_eff.assign((size_t)batch * 8 * n, 0.0);
    std::vector<double> rows;   // [rows][16]
    for (int b = 0; b < batch; ++b) {
        const uint8_t* m = mask + b * n;
        std::vector<BodyLink> links;
        std::vector<long long> start((size_t)nbodies + 1);
        const uint8_t* h = hold ? hold + b * n : nullptr;
        body_links(m, label + b * n, nx, ny, nbodies, links, start.data(), h);
        for (int body = 0; body < nbodies; ++body) {
            const double* cen = centre + ((size_t)b * nbodies + body) * 2;
            const double* mot = motion + ((size_t)b * nbodies + body) * 3;
            for (long long i = start[body]; i < start[body + 1]; ++i) {
                const int x = links[(size_t)i].x, y = links[(size_t)i].yk >> 4, k = links[(size_t)i].yk & 15;
                const int fx = x + BODY_CX[k], fy = y - BODY_CY[k];
                const bool next_fluid = fx >= 0 && fx < nx && fy >= 0 && fy < ny && !m[(size_t)fx * ny + fy] && !(h && h[(size_t)fx * ny + fy]);
                const double cell = uw ? wall_cell_term_at(uw + (size_t)b * 2 * n, nx, ny, x, y, k) : 0.0;
                const ShapeLink l = shape_link(x, y, k, q[shape_q_index(b, k, x, y, nx, ny)], next_fluid, cen[0], cen[1], mot[0], mot[1], mot[2],
                                               uw ? &cell : nullptr);
                int32_t& row = t.cell_row[b * n + (size_t)y * nx + x];
                if (row < 0) {
                    if (rows.size() / 16 >= 0x7fffffffu) {
                        t.too_many_rows = true;
                        return t;
                    }
                    row = (int32_t)(rows.size() / 16);
                    rows.resize(rows.size() + 16, 0.0);
                    for (int j = 0; j < 8; ++j) rows[(size_t)row * 16 + j] = 1.0;
                    t.near.push_back(0);
                }
                rows[(size_t)row * 16 + (k - 1)] = l.a;
                rows[(size_t)row * 16 + 8 + (k - 1)] = l.d;
                if (l.near) t.near[(size_t)row] |= (uint8_t)(1u << (k - 1));
                t.link_q.push_back(l.q);
                t.q_eff[shape_q_index(b, k, x, y, nx, ny)] = l.q;
            }
        }
    }
    t.ad.resize(rows.size() * (f32 ? sizeof(float) : sizeof(double)));
    for (size_t i = 0; i < rows.size(); ++i) {
        if (f32) ((float*)t.ad.data())[i] = (float)rows[i];
        else ((double*)t.ad.data())[i] = rows[i];
    }
    return t;
}
}  // namespace lbmhost
