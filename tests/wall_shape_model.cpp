// wall_shape_model.cpp -- the host side of curved obstacle surfaces (csrc/lbm_wall_shape.hpp: shape_bad_link, shape_parts, over body_links of
// csrc/lbm_bodies.hpp) driven without a device, for tests/test_solid_shape_cpu.py.  Reads from the file named by argv[1]
//   nx ny nbodies batch f32, then per lattice nx * ny mask values (0 / 1) and nx * ny labels, both in the host layout [x][y], nbodies
//   lines x0 y0 Ux Uy Om and 8 * nx * ny values of q ([k - 1][x][y]), all doubles as hexadecimal floating-point numbers,
// and prints, every double as a hexadecimal floating-point number,
//   bad lattice x y k q                                   a q that is refused, and nothing else; or
//   link q                                                the effective q of every entry of the batch's link list, in its order
//   cell lattice x y row near a_1 .. a_8 d_1 .. d_8       the cells that have a row, the table's values (the lattice type) as doubles
//   qeff lattice k x y q                                  the nonzero entries of the effective q
//   rows n
#include <cstdio>
#include <vector>

#include "lbm_wall_shape.hpp"

using namespace lbmhost;

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int nx = 0, ny = 0, nb = 0, B = 0, f32 = 0;
    if (std::fscanf(f, "%d %d %d %d %d", &nx, &ny, &nb, &B, &f32) != 5 || nx < 1 || ny < 1 || nb < 1 || nb > BODY_MAX || B < 1) return 2;
    const size_t n = (size_t)nx * ny;
    std::vector<uint8_t> mask(B * n);
    std::vector<int32_t> body(B * n);
    std::vector<double> centre(2 * (size_t)nb * B), motion(3 * (size_t)nb * B), q(8 * n * B);
    for (int l = 0; l < B; ++l) {
        for (size_t i = 0; i < n; ++i) {
            int v = 0;
            if (std::fscanf(f, "%d", &v) != 1) return 2;
            mask[l * n + i] = (uint8_t)v;
        }
        for (size_t i = 0; i < n; ++i)
            if (std::fscanf(f, "%d", &body[l * n + i]) != 1) return 2;
        for (int b = 0; b < nb; ++b) {
            double* c = &centre[2 * ((size_t)l * nb + b)];
            double* m = &motion[3 * ((size_t)l * nb + b)];
            if (std::fscanf(f, "%la %la %la %la %la", c, c + 1, m, m + 1, m + 2) != 5) return 2;
        }
        for (size_t i = 0; i < 8 * n; ++i)
            if (std::fscanf(f, "%la", &q[l * 8 * n + i]) != 1) return 2;
    }
    std::fclose(f);
    ShapeBad bad;
    if (shape_bad_link(mask.data(), q.data(), B, nx, ny, &bad)) {
        std::printf("bad %d %d %d %d %a\n", bad.lattice, bad.x, bad.y, bad.k, bad.q);
        return 0;
    }
    const ShapeParts t = shape_parts(mask.data(), body.data(), centre.data(), motion.data(), q.data(), B, nx, ny, nb, f32 != 0);
    if (t.too_many_rows) return 3;
    for (size_t i = 0; i < t.link_q.size(); ++i) std::printf("link %a\n", t.link_q[i]);
    for (int l = 0; l < B; ++l)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                const int32_t row = t.cell_row[l * n + (size_t)y * nx + x];
                if (row < 0) continue;
                std::printf("cell %d %d %d %d %d", l, x, y, row, (int)t.near[(size_t)row]);
                for (int j = 0; j < 16; ++j)
                    std::printf(" %a", f32 ? (double)((const float*)t.ad.data())[(size_t)row * 16 + j] : ((const double*)t.ad.data())[(size_t)row * 16 + j]);
                std::printf("\n");
            }
    for (int l = 0; l < B; ++l)
        for (int k = 1; k < 9; ++k)
            for (int x = 0; x < nx; ++x)
                for (int y = 0; y < ny; ++y) {
                    const double v = t.q_eff[shape_q_index(l, k, x, y, nx, ny)];
                    if (v != 0.0) std::printf("qeff %d %d %d %d %a\n", l, k, x, y, v);
                }
    std::printf("rows %zu\n", t.near.size());
    return 0;
}
