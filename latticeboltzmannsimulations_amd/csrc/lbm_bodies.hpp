// lbm_bodies.hpp -- the bodies of a solid mask (lbm_set_solid_bodies; contract in include/lbm.h): the check of the
// labels, the centroids, and the link list that k_body_force (lbm_bodies.hip) walks, with its cut into chunks; then the tables of a
// whole batch as the device holds them (body_parts).  Arrays are in the host layout of the mask, [nx][ny] with y fastest, one lattice at
// a time.  Plain C++, nothing from HIP: tests/test_body_force_cpu.py and tests/test_devmem_cpu.py drive it from programs of their own.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "lbm_devmem.hpp"

namespace lbmhost {

constexpr int BODY_MAX = 256;      // bodies per lattice
constexpr int BODY_CHUNK = 2048;   // links of one body that one workgroup reduces (8 per lane)

// the lattice vectors (= cxk, cyk of lbm_device.hpp; lbm_bodies.hip asserts it): slot k of cell (x, y) pulls from (x - cx, y + cy)
constexpr int BODY_CX[9] = {0, 1, 0, -1, 0, 1, -1, -1, 1};
constexpr int BODY_CY[9] = {0, 0, 1, 0, -1, 1, 1, -1, -1};

// One link: the fluid cell (x, y) and the slot k = yk & 15 (y = yk >> 4) whose source is a solid cell.  Its body is that of the segment
// of the list it lies in.
struct BodyLink {
    int32_t x, yk;
};
// links [begin, begin + n) of the list, all of `body`: the work of one workgroup (n = 0: padding)
struct BodyChunk {
    long long begin;
    int32_t n, body;
};

// The first solid cell whose label is outside [0, nbodies), or -1.
inline long long body_bad_label(const uint8_t* mask, const int32_t* body, size_t cells, int nbodies) {
    for (size_t i = 0; i < cells; ++i)
        if (mask[i] && (body[i] < 0 || body[i] >= nbodies)) return (long long)i;
    return -1;
}

// centre[nbodies][2]: the mean of the indices (x, y) of each body's cells, the sums exact in double; (0, 0) for a body without cells
inline void body_centroids(const uint8_t* mask, const int32_t* body, int nx, int ny, int nbodies, double* centre) {
    std::vector<double> sx(nbodies, 0.0), sy(nbodies, 0.0), n(nbodies, 0.0);
    for (int x = 0; x < nx; ++x)
        for (int y = 0; y < ny; ++y) {
            const size_t i = (size_t)x * ny + y;
            if (!mask[i]) continue;
            sx[body[i]] += x;
            sy[body[i]] += y;
            n[body[i]] += 1.0;
        }
    for (int b = 0; b < nbodies; ++b) {
        centre[2 * b] = n[b] > 0.0 ? sx[b] / n[b] : 0.0;
        centre[2 * b + 1] = n[b] > 0.0 ? sy[b] / n[b] : 0.0;
    }
}

// The link list of one lattice, appended to `links`: sorted by body, then by cell in [y][x] order, then by k.  start[nbodies + 1]
// receives the bodies' ranges, as indices into `links`.  hold (lbm_set_open_cells; null: none): the hold cells of the lattice, which are
// no fluid cells -- a hold cell is never updated and bounces nothing, so no link starts at one.
inline void body_links(const uint8_t* mask, const int32_t* body, int nx, int ny, int nbodies, std::vector<BodyLink>& links, long long* start,
                       const uint8_t* hold = nullptr) {
    auto each = [&](auto&& f) {
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                if (mask[(size_t)x * ny + y] || (hold && hold[(size_t)x * ny + y])) continue;
                for (int k = 1; k < 9; ++k) {
                    const int sx = x - BODY_CX[k], sy = y + BODY_CY[k];
                    if (sx < 0 || sx >= nx || sy < 0 || sy >= ny || !mask[(size_t)sx * ny + sy]) continue;
                    f(x, y, k, body[(size_t)sx * ny + sy]);
                }
            }
    };
    std::vector<long long> fill(nbodies + 1, 0);
    each([&](int, int, int, int b) { ++fill[b + 1]; });
    const long long base = (long long)links.size();
    start[0] = base;
    for (int b = 0; b < nbodies; ++b) start[b + 1] = start[b] + fill[b + 1];
    links.resize((size_t)start[nbodies]);
    for (int b = 0; b < nbodies; ++b) fill[b] = start[b];
    each([&](int x, int y, int k, int b) { links[(size_t)fill[b]++] = BodyLink{x, y * 16 + k}; });
}

// The chunks of one lattice appended to `chunks`: each body's range cut every BODY_CHUNK links, bodies in order.  first[nbodies + 1]
// receives the bodies' ranges of chunks, counted from the lattice's first chunk.
inline void body_chunks(const long long* start, int nbodies, std::vector<BodyChunk>& chunks, int32_t* first) {
    const size_t base = chunks.size();
    for (int b = 0; b < nbodies; ++b) {
        first[b] = (int32_t)(chunks.size() - base);
        for (long long i = start[b]; i < start[b + 1]; i += BODY_CHUNK)
            chunks.push_back(BodyChunk{i, (int32_t)(start[b + 1] - i < BODY_CHUNK ? start[b + 1] - i : BODY_CHUNK), b});
    }
    first[nbodies] = (int32_t)(chunks.size() - base);
}

// The tables of the bodies of a whole batch (mask and label [batch][nx][ny], centre[batch][nbodies][2]) as the device holds them in one
// allocation: the link list of every lattice, one after the other; chunks[batch][maxchunks], padded with empty chunks to the longest
// lattice's; first[batch][nbodies + 1]; centre; then, only reserved, the workgroups' partial results of one pass (acc_vals doubles per
// chunk) and the records of the one-shot call (rec_vals doubles per body).  hold: the hold cells [batch][nx][ny] (null: none), see body_links.
struct BodyParts {
    enum { LINKS, CHUNKS, FIRST, CENTRE, PARTIAL, REC };
    std::vector<BodyLink> links;
    std::vector<BodyChunk> chunks;
    std::vector<int32_t> first;
    std::vector<double> centre;
    size_t maxchunks = 1, partial_bytes = 0, rec_bytes = 0;
    std::vector<Part> parts() const {
        return {{links.data(), links.size() * sizeof(BodyLink)}, {chunks.data(), chunks.size() * sizeof(BodyChunk)},
                {first.data(), first.size() * sizeof(int32_t)}, {centre.data(), centre.size() * sizeof(double)},
                {nullptr, partial_bytes}, {nullptr, rec_bytes}};
    }
};
inline BodyParts body_parts(const uint8_t* mask, const int32_t* label, const double* centre, int batch, int nx, int ny, int nbodies, int acc_vals,
                            int rec_vals, const uint8_t* hold = nullptr) {
    const size_t n = (size_t)nx * ny, B = (size_t)batch, nb1 = (size_t)nbodies + 1;
    BodyParts t;
    std::vector<long long> start(nb1);
    std::vector<std::vector<BodyChunk>> chunks(B);
    t.first.resize(B * nb1);
    for (size_t b = 0; b < B; ++b) {
        body_links(mask + b * n, label + b * n, nx, ny, nbodies, t.links, start.data(), hold ? hold + b * n : nullptr);
        body_chunks(start.data(), nbodies, chunks[b], t.first.data() + b * nb1);
        if (chunks[b].size() > t.maxchunks) t.maxchunks = chunks[b].size();
    }
    t.chunks.assign(B * t.maxchunks, BodyChunk{0, 0, 0});
    for (size_t b = 0; b < B; ++b) std::copy(chunks[b].begin(), chunks[b].end(), t.chunks.begin() + b * t.maxchunks);
    t.centre.assign(centre, centre + B * nbodies * 2);
    t.partial_bytes = B * t.maxchunks * acc_vals * sizeof(double);
    t.rec_bytes = B * nbodies * rec_vals * sizeof(double);
    return t;
}
}  // namespace lbmhost
