// wall_motion_model.cpp -- the host side of the moving bodies (csrc/lbm_wall_motion.hpp: wall_motion, wall_motion_closed, over body_links
// of csrc/lbm_bodies.hpp) driven without a device, for tests/test_body_motion_cpu.py.  Reads from the file named by argv[1]
//   nx ny nbodies, then nx * ny mask values (0 / 1) and nx * ny labels, both in the host layout [x][y], then nbodies lines
//   x0 y0 Ux Uy Om as hexadecimal floating-point numbers,
// and prints, every double as a hexadecimal floating-point number,
//   link x y k body delta delta_as_float / S s / A a / closed 0|1 / rows n / cell x y row d_1 .. d_8 (the cells that have a row).
// The table is built with row_base = 5, as for a lattice that follows another in a batch.
#include <cstdio>
#include <vector>

#include "lbm_wall_motion.hpp"

using namespace lbmhost;

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int nx = 0, ny = 0, nb = 0;
    if (std::fscanf(f, "%d %d %d", &nx, &ny, &nb) != 3 || nx < 1 || ny < 1 || nb < 1 || nb > BODY_MAX) return 2;
    const size_t n = (size_t)nx * ny;
    std::vector<uint8_t> mask(n);
    std::vector<int32_t> body(n);
    for (size_t i = 0; i < n; ++i) {
        int v = 0;
        if (std::fscanf(f, "%d", &v) != 1) return 2;
        mask[i] = (uint8_t)v;
    }
    for (size_t i = 0; i < n; ++i)
        if (std::fscanf(f, "%d", &body[i]) != 1) return 2;
    std::vector<double> centre(2 * (size_t)nb), motion(3 * (size_t)nb);
    for (int b = 0; b < nb; ++b)
        if (std::fscanf(f, "%la %la %la %la %la", &centre[2 * b], &centre[2 * b + 1], &motion[3 * b], &motion[3 * b + 1], &motion[3 * b + 2]) != 5) return 2;
    std::fclose(f);
    std::vector<BodyLink> links;
    std::vector<long long> start(nb + 1);
    body_links(mask.data(), body.data(), nx, ny, nb, links, start.data());
    const long long base = 5;
    const WallMotion m = wall_motion(links, start.data(), nx, ny, nb, centre.data(), motion.data(), base);
    for (int b = 0; b < nb; ++b)
        for (long long i = start[b]; i < start[b + 1]; ++i)
            std::printf("link %d %d %d %d %a %a\n", links[i].x, links[i].yk >> 4, links[i].yk & 15, b, m.delta[i], wall_delta_rounded(m.delta[i], true));
    std::printf("S %a\nA %a\nclosed %d\nrows %zu\n", m.S, m.A, wall_motion_closed(m) ? 1 : 0, m.rows.size() / 8);
    for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x) {
            const int32_t row = m.cell_row[(size_t)y * nx + x];
            if (row < 0) continue;
            std::printf("cell %d %d %d", x, y, row);
            for (int k = 0; k < 8; ++k) std::printf(" %a", m.rows[(size_t)(row - base) * 8 + k]);
            std::printf("\n");
        }
    return 0;
}
