/* Driver for the extracted kernel text: included at the END of the generated translation unit, after the two kernels.
 * Restates the host side of a time step of MRT_GPU.py (lines 292-296: block and grid; 724-732: funRT, then funBC, same launch
 * shape), with the threads of each launch called one after the other.  Arrays are the script's device layout, i = x + y*xsize.
 *
 * order: 0 ascending (block, thread), 1 descending, >= 2 a shuffle seeded with `order`.  The result must not depend on it
 * (tests/test_mrt_gpu_text_cpu.py asserts that); that is what makes a sequential run a statement of the CUDA program.
 * Returns 1 for a shape the text is not defined on: it derives xsize from blockDim*gridDim. */
#include <cstdint>
#include <vector>

static inline void reftext_place(int id, int bx, int by, int gx) {
    const int per = bx * by, block = id / per, thread = id % per;
    blockIdx.x = (unsigned)(block % gx); blockIdx.y = (unsigned)(block / gx); blockIdx.z = 0;
    threadIdx.x = (unsigned)(thread % bx); threadIdx.y = (unsigned)(thread / bx); threadIdx.z = 0;
}

extern "C" int step(float* fin, float* ftemp, float* feq, float* rho, float* u, float* taus, int nx, int ny, int nsteps, int order) {
    const int warp = 32;
    const int bx = nx < warp ? nx : warp, by = ny < warp ? ny : warp;
    const int gx = (nx + warp - 1) / warp, gy = (ny + warp - 1) / warp;
    if (nx < 1 || ny < 1 || bx * gx != nx || by * gy != ny) return 1;
    blockDim.x = (unsigned)bx; blockDim.y = (unsigned)by; blockDim.z = 1;
    gridDim.x = (unsigned)gx; gridDim.y = (unsigned)gy; gridDim.z = 1;
    const int n = nx * ny;
    std::vector<int> ids((size_t)n);
    for (int i = 0; i < n; ++i) ids[(size_t)i] = order == 1 ? n - 1 - i : i;
    if (order >= 2) { /* Fisher-Yates on a splitmix64 stream: the same permutation wherever this is compiled */
        uint64_t s = (uint64_t)order;
        for (int i = n - 1; i > 0; --i) {
            s += 0x9E3779B97F4A7C15ull;
            uint64_t z = s;
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            z ^= z >> 31;
            const int j = (int)(z % (uint64_t)(i + 1));
            const int t = ids[(size_t)i]; ids[(size_t)i] = ids[(size_t)j]; ids[(size_t)j] = t;
        }
    }
    for (int it = 0; it < nsteps; ++it) {
        for (int i = 0; i < n; ++i) { reftext_place(ids[(size_t)i], bx, by, gx); funRT(fin, ftemp, feq, rho, u, taus); }
        for (int i = 0; i < n; ++i) { reftext_place(ids[(size_t)i], bx, by, gx); funBC(ftemp, feq, fin); }
    }
    return 0;
}
