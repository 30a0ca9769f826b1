// lbm_periodic.hpp -- periodic sides and the uniform driving force of an obstacle lattice (lbm_set_periodic, lbm_set_driving_force;
// contract in include/lbm.h): the partner of an image cell, the check that a mask and its labels equal their own wrap,
// the hold cells of a periodic lattice, and the eight constants of the force.  Arrays are in the host layout of the mask, [nx][ny] with y
// fastest, one lattice at a time.  Plain C++, nothing from HIP: tests/test_periodic_cpu.py drives it from a program of its own.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "lbm_wall_motion.hpp"   // (BODY_CX, BODY_CY; LBM_WM_ATTR, LBM_WM_NO_CONTRACT)

namespace lbmhost {

// Periodic in a direction of n cells: cells 0 and n - 1 are images of the real cells n - 2 and 1; every other cell is its own partner.
// The partner of an image is always a real cell.
constexpr int periodic_partner(int i, int n, bool periodic) { return !periodic ? i : (i == 0 ? n - 2 : (i == n - 1 ? 1 : i)); }
constexpr bool periodic_image(int x, int y, int nx, int ny, bool px, bool py) {
    return (px && (x == 0 || x == nx - 1)) || (py && (y == 0 || y == ny - 1));
}
// how many image cells a lattice has: the two columns whole, the two rows without the columns' cells
constexpr long long periodic_images(int nx, int ny, bool px, bool py) {
    return (px ? 2LL * ny : 0LL) + (py ? 2LL * (px ? nx - 2 : nx) : 0LL);
}

// The first image cell (index x * ny + y, in this order) at which the mask, or the labels (null: not checked; read on solid cells only),
// differ from their own wrap -- the value at the cell's partner; -1: none.  *labels_differ: which of the two it was.
inline long long periodic_bad_cell(const uint8_t* mask, const int32_t* label, int nx, int ny, bool px, bool py, bool* labels_differ = nullptr) {
    for (int x = 0; x < nx; ++x)
        for (int y = 0; y < ny; ++y) {
            if (!periodic_image(x, y, nx, ny, px, py)) continue;
            const size_t i = (size_t)x * ny + y, p = (size_t)periodic_partner(x, nx, px) * ny + periodic_partner(y, ny, py);
            const bool m = mask[i] != 0;
            if (m != (mask[p] != 0)) {
                if (labels_differ) *labels_differ = false;
                return (long long)i;
            }
            if (m && label && label[i] != label[p]) {
                if (labels_differ) *labels_differ = true;
                return (long long)i;
            }
        }
    return -1;
}

// The hold cells of a periodic lattice: the user's (hold, null: none) and every image cell that is not solid.  out[nx][ny], 0 / 1.
// Returns the index of the first image cell that is a user hold cell (refused: an image holds its partner's populations), or -1.
inline long long periodic_hold(const uint8_t* mask, const uint8_t* hold, int nx, int ny, bool px, bool py, uint8_t* out) {
    long long bad = -1;
    for (int x = 0; x < nx; ++x)
        for (int y = 0; y < ny; ++y) {
            const size_t i = (size_t)x * ny + y;
            const bool img = periodic_image(x, y, nx, ny, px, py), h = hold && hold[i];
            if (img && h && bad < 0) bad = (long long)i;
            out[i] = (h || (img && !mask[i])) ? 1 : 0;
        }
    return bad;
}

// The driving force (lbm_set_driving_force): what every collision of a cell that is neither solid nor held adds to its post-collision
// population of direction k, F_k = (3 w_k) (cx_k fx + cy_k fy), 3 w_k = 1/3 (k <= 4) or 1/12, in double, every product and sum rounded in
// the order written; out[k - 1], k = 1 .. 8 (F_0 = 0).  The caller rounds each once to the lattice type.
LBM_WM_ATTR inline void drive_terms(double fx, double fy, double (&out)[8]) {
    LBM_WM_NO_CONTRACT
    for (int k = 1; k < 9; ++k) {
        const double w3 = k < 5 ? 1.0 / 3.0 : 1.0 / 12.0;
        out[k - 1] = w3 * ((double)BODY_CX[k] * fx + (double)BODY_CY[k] * fy);
    }
}
}  // namespace lbmhost
