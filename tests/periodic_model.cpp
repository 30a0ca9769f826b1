// periodic_model.cpp -- the host logic of periodic sides and of the driving force (csrc/lbm_periodic.hpp) driven without a device, for
// tests/test_periodic_cpu.py.  argv[1] names the case file.  The file holds
//   nx ny px py fx fy (the force as hexadecimal floating-point numbers), then nx * ny values each of the mask, the labels and the user's
//   hold cells (0 / 1; all zero: none), in the host layout [x][y],
// and the program prints
//   images n                       how many image cells the lattice has
//   partner x y sx sy              of every image cell, in the order x, then y
//   bad i labels                   the first cell whose mask (labels = 0) or label (1) differs from its own wrap, -1: none
//   holdbad i                      the first image cell that is a user hold cell, -1: none
//   hold v ...                     the hold cells of the periodic lattice, nx * ny values in the host layout
//   drive F_1 .. F_8               the constants of the force, every double as a hexadecimal floating-point number
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lbm_periodic.hpp"

using namespace lbmhost;

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int nx = 0, ny = 0, px = 0, py = 0;
    double fx = 0.0, fy = 0.0;
    if (std::fscanf(f, "%d %d %d %d %la %la", &nx, &ny, &px, &py, &fx, &fy) != 6 || nx < 1 || ny < 1) return 2;
    const size_t n = (size_t)nx * ny;
    std::vector<uint8_t> mask(n), hold(n), all(n);
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
    std::fclose(f);
    const bool x = px != 0, y = py != 0;
    long long images = 0;
    for (int i = 0; i < nx; ++i)
        for (int j = 0; j < ny; ++j)
            if (periodic_image(i, j, nx, ny, x, y)) {
                std::printf("partner %d %d %d %d\n", i, j, periodic_partner(i, nx, x), periodic_partner(j, ny, y));
                ++images;
            }
    if (images != periodic_images(nx, ny, x, y)) return 3;
    std::printf("images %lld\n", images);
    bool lab = false;
    const long long bad = periodic_bad_cell(mask.data(), body.data(), nx, ny, x, y, &lab);
    std::printf("bad %lld %d\n", bad, bad >= 0 && lab ? 1 : 0);
    std::printf("holdbad %lld\n", periodic_hold(mask.data(), any_hold ? hold.data() : nullptr, nx, ny, x, y, all.data()));
    std::printf("hold");
    for (size_t i = 0; i < n; ++i) std::printf(" %d", (int)all[i]);
    std::printf("\n");
    double d[8];
    drive_terms(fx, fy, d);
    std::printf("drive");
    for (int k = 0; k < 8; ++k) std::printf(" %a", d[k]);
    std::printf("\n");
    return 0;
}
