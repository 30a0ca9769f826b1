// body_links_model.cpp -- the host side of the per-body force (csrc/lbm_bodies.hpp: body_bad_label, body_centroids, body_links,
// body_chunks) driven without a device, for tests/test_body_force_cpu.py.  Reads from the file named by argv[1]
//   nx ny nbodies, then nx * ny mask values (0 / 1) and nx * ny labels, both in the host layout [x][y],
// and prints
//   bad i / centre b x0 y0 (17 significant digits) / start s_0 .. s_nbodies / link x y k body / first f_0 .. f_nbodies /
//   chunk begin n body
// The list is built twice into one vector, as for a batch of two equal lattices: the second lattice's ranges start where the first ends.
#include <cstdio>
#include <vector>

#include "lbm_bodies.hpp"

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
    std::fclose(f);
    const long long bad = body_bad_label(mask.data(), body.data(), n, nb);
    std::printf("bad %lld\n", bad);
    if (bad >= 0) return 0;
    std::vector<double> centre(2 * (size_t)nb);
    body_centroids(mask.data(), body.data(), nx, ny, nb, centre.data());
    for (int b = 0; b < nb; ++b) std::printf("centre %d %.17g %.17g\n", b, centre[2 * b], centre[2 * b + 1]);
    std::vector<BodyLink> links;
    std::vector<BodyChunk> chunks;
    for (int lattice = 0; lattice < 2; ++lattice) {
        std::vector<long long> start(nb + 1);
        std::vector<int32_t> first(nb + 1);
        body_links(mask.data(), body.data(), nx, ny, nb, links, start.data());
        std::printf("start");
        for (long long s : start) std::printf(" %lld", s);
        std::printf("\n");
        for (int b = 0; b < nb; ++b)
            for (long long i = start[b]; i < start[b + 1]; ++i) std::printf("link %d %d %d %d\n", links[i].x, links[i].yk >> 4, links[i].yk & 15, b);
        const size_t c0 = chunks.size();
        body_chunks(start.data(), nb, chunks, first.data());
        std::printf("first");
        for (int32_t v : first) std::printf(" %d", v);
        std::printf("\n");
        for (size_t i = c0; i < chunks.size(); ++i) std::printf("chunk %lld %d %d\n", chunks[i].begin, chunks[i].n, chunks[i].body);
    }
    return 0;
}
