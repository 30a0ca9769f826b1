// open_flow_model.cpp -- the host tables of a lattice with hold cells and a wall velocity per solid cell (csrc/lbm_wall_motion.hpp:
// motion_parts; csrc/lbm_wall_shape.hpp: shape_parts; over body_links of csrc/lbm_bodies.hpp) driven without a device, for
// tests/test_open_flow_cpu.py.  argv[1] names the case file, argv[2] is 1 for an fp32 lattice and 0 for fp64.  The file holds
//   nx ny nbodies has_uw has_q, then nx * ny values each of the mask, the labels and the hold cells (0 / 1; all zero: none), in the host
//   layout [x][y], then nbodies lines x0 y0 Ux Uy Om, then (has_uw) 2 * nx * ny velocities, then (has_q) 8 * nx * ny wall distances,
//   every double as a hexadecimal floating-point number,
// and the program prints, every double as a hexadecimal floating-point number,
//   link x y k body                                the list as the tables use it (no link starts at a hold cell)
//   refusal r lattice S A links                    of motion_parts (0: none, 1: the flux check)
//   ld v                                           link_delta per link, as the lattice adds it (absent after a refusal)
//   cell x y row d_1 .. d_8                        the rows of the table of the deltas, in the lattice type
//   srow x y row near a_1 .. a_8 d_1 .. d_8 / lq v the rows of the shape's table and the effective q per link (has_q)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lbm_wall_shape.hpp"

using namespace lbmhost;

static double at(const std::vector<char>& t, size_t i, bool f32) { return f32 ? (double)((const float*)t.data())[i] : ((const double*)t.data())[i]; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const bool f32 = std::atoi(argv[2]) != 0;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int nx = 0, ny = 0, nb = 0, has_uw = 0, has_q = 0;
    if (std::fscanf(f, "%d %d %d %d %d", &nx, &ny, &nb, &has_uw, &has_q) != 5 || nx < 1 || ny < 1 || nb < 1 || nb > BODY_MAX) return 2;
    const size_t n = (size_t)nx * ny;
    std::vector<uint8_t> mask(n), hold(n);
    std::vector<int32_t> body(n);
    bool any_hold = false;
    for (int which = 0; which < 3; ++which)
        for (size_t i = 0; i < n; ++i) {
            int v = 0;
            if (std::fscanf(f, "%d", &v) != 1) return 2;
            if (which == 0) mask[i] = (uint8_t)v;
            else if (which == 1) body[i] = v;
            else { hold[i] = (uint8_t)v; any_hold = any_hold || v != 0; }
        }
    std::vector<double> centre(2 * (size_t)nb), motion(3 * (size_t)nb), uw, q;
    for (int b = 0; b < nb; ++b)
        if (std::fscanf(f, "%la %la %la %la %la", &centre[2 * b], &centre[2 * b + 1], &motion[3 * b], &motion[3 * b + 1], &motion[3 * b + 2]) != 5) return 2;
    if (has_uw) {
        uw.resize(2 * n);
        for (double& v : uw)
            if (std::fscanf(f, "%la", &v) != 1) return 2;
    }
    if (has_q) {
        q.resize(8 * n);
        for (double& v : q)
            if (std::fscanf(f, "%la", &v) != 1) return 2;
    }
    std::fclose(f);
    const uint8_t* h = any_hold ? hold.data() : nullptr;
    const double* u = has_uw ? uw.data() : nullptr;
    std::vector<BodyLink> links;
    std::vector<long long> start(nb + 1);
    body_links(mask.data(), body.data(), nx, ny, nb, links, start.data(), h);
    for (int b = 0; b < nb; ++b)
        for (long long i = start[b]; i < start[b + 1]; ++i) std::printf("link %d %d %d %d\n", links[i].x, links[i].yk >> 4, links[i].yk & 15, b);
    const MotionParts t = motion_parts(mask.data(), body.data(), centre.data(), motion.data(), 1, nx, ny, nb, f32, h, u);
    std::printf("refusal %d %d %a %a %zu\n", (int)t.refusal, t.lattice, t.S, t.A, t.links);
    if (t.refusal == MotionParts::NONE) {
        for (double d : t.link_delta) std::printf("ld %a\n", d);
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                const int32_t row = t.cell_row[(size_t)y * nx + x];
                if (row < 0) continue;
                std::printf("cell %d %d %d", x, y, row);
                for (int k = 0; k < 8; ++k) std::printf(" %a", at(t.delta, (size_t)row * 8 + k, f32));
                std::printf("\n");
            }
    }
    if (has_q) {
        const ShapeParts s = shape_parts(mask.data(), body.data(), centre.data(), motion.data(), q.data(), 1, nx, ny, nb, f32, h, u);
        if (s.too_many_rows) return 3;
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                const int32_t row = s.cell_row[(size_t)y * nx + x];
                if (row < 0) continue;
                std::printf("srow %d %d %d %d", x, y, row, (int)s.near[(size_t)row]);
                for (int k = 0; k < 16; ++k) std::printf(" %a", at(s.ad, (size_t)row * 16 + k, f32));
                std::printf("\n");
            }
        for (double v : s.link_q) std::printf("lq %a\n", v);
    }
    return 0;
}
