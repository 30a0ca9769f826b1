// scalar_model.cpp -- the host logic of the passive scalar (csrc/lbm_scalar.hpp, its host part) driven without a device, for
// tests/test_scalar_cpu.py.  argv[1] names the case file.  The file holds
//   nx ny D magic (the two as hexadecimal floating-point numbers), then nx * ny values each of the mask, the hold cells and the Dirichlet
//   flags (0 / 1), then nx * ny wall values (hexadecimal floating-point numbers), all in the host layout [x][y]; then nine flow populations
//   and a hold value (hexadecimal),
// and the program prints, every double as a hexadecimal floating-point number,
//   rates w+ w-                    the two relaxation rates
//   cell_row v ...                 ny * nx values, x fastest
//   row r bits v1 .. v8            one line per row of the table
//   hold g0 .. g8                  what a hold cell with those populations and that value keeps
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lbm_scalar.hpp"

using namespace lbmhost;

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int nx = 0, ny = 0;
    double D = 0.0, magic = 0.0;
    if (std::fscanf(f, "%d %d %la %la", &nx, &ny, &D, &magic) != 4 || nx < 1 || ny < 1) return 2;
    const size_t n = (size_t)nx * ny;
    std::vector<uint8_t> mask(n), hold(n), dir(n);
    std::vector<double> wv(n);
    for (int which = 0; which < 3; ++which)
        for (size_t i = 0; i < n; ++i) {
            int v = 0;
            if (std::fscanf(f, "%d", &v) != 1) return 2;
            (which == 0 ? mask : which == 1 ? hold : dir)[i] = (uint8_t)v;
        }
    for (size_t i = 0; i < n; ++i)
        if (std::fscanf(f, "%la", &wv[i]) != 1) return 2;
    double pops[9], Ch = 0.0;
    for (int k = 0; k < 9; ++k)
        if (std::fscanf(f, "%la", &pops[k]) != 1) return 2;
    if (std::fscanf(f, "%la", &Ch) != 1) return 2;
    std::fclose(f);
    double wp = 0.0, wm = 0.0;
    scalar_rates(D, magic, &wp, &wm);
    std::printf("rates %a %a\n", wp, wm);
    const ScalarWalls t = scalar_wall_table(mask.data(), hold.data(), dir.data(), wv.data(), nx, ny);
    std::printf("cell_row");
    for (size_t i = 0; i < n; ++i) std::printf(" %d", (int)t.cell_row[i]);
    std::printf("\n");
    for (size_t r = 0; r < t.bits.size(); ++r) {
        std::printf("row %zu %d", r, (int)t.bits[r]);
        for (int k = 0; k < 8; ++k) std::printf(" %a", t.val[r * 8 + k]);
        std::printf("\n");
    }
    double g[9];
    scalar_hold_values(pops, Ch, g);
    std::printf("hold");
    for (int k = 0; k < 9; ++k) std::printf(" %a", g[k]);
    std::printf("\n");
    return 0;
}
