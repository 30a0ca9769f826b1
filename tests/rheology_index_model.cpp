// rheology_index_model.cpp -- TEST HELPER: rheology_index and rheology_table of csrc/lbm_rheology.hpp on the host, for every kind of input a
// lattice can hand over (tests/test_rheology_cpu.py builds and runs it, with the address and undefined-behaviour sanitizers where the
// compiler has them).  For every table size and every input: i in [0, n - 2], fr in [0, 1], and the interpolation reads inside the table.
// Prints one "ok <type> <cases>" line per real type, or "FAILED ..." lines.
#include <cfloat>
#include <cstdio>
#include <limits>
#include <vector>

#include "lbm_rheology.hpp"

template <typename R>
static int run(const char* name) {
    int bad = 0, cases = 0;
    const R inf = std::numeric_limits<R>::infinity(), nan = std::numeric_limits<R>::quiet_NaN();
    for (int n : {2, 3, 17, 256, 4096, 65536}) {
        std::vector<double> omega((size_t)n), omegam((size_t)n);
        for (int i = 0; i < n; ++i) omega[i] = 0.6 + 1.3 * ((i * 7919) % n) / n, omegam[i] = 1.9 - omega[i] * 0.5;
        const std::vector<R> t = rheology_table<R>(omega.data(), omegam.data(), n);
        if (t.size() != (size_t)n * RHEO_STRIDE || t[(size_t)(n - 1) * RHEO_STRIDE + 1] != (R)0 || t[(size_t)(n - 1) * RHEO_STRIDE + 3] != (R)0) {
            std::printf("FAILED %s table n=%d\n", name, n);
            ++bad;
        }
        const R nm1 = (R)(n - 1);
        const R in[] = {nan, -nan, inf, -inf, (R)-1, (R)-0.0, (R)0, std::numeric_limits<R>::denorm_min(), std::numeric_limits<R>::min(), (R)0.25,
                        (R)0.999999, (R)1, (R)1.5, nm1 - (R)1, nm1 - (R)0.5, std::nextafter(nm1, (R)0), nm1, std::nextafter(nm1, inf), nm1 + (R)1,
                        (R)1e30, std::numeric_limits<R>::max(), -std::numeric_limits<R>::max(), (R)2147483648.0, (R)-2147483649.0, (R)4294967296.0};
        for (const R s : in) {
            R fr = (R)-7;
            const int i = rheology_index<R>(s, n - 1, fr);
            ++cases;
            const bool ok = i >= 0 && i <= n - 2 && fr >= (R)0 && fr <= (R)1;
            if (!ok) {
                std::printf("FAILED %s n=%d s=%a i=%d fr=%a\n", name, n, (double)s, i, (double)fr);
                ++bad;
                continue;
            }
            // the loads of rheology_lookup: the entry's four reals (the sanitizer watches the bounds)
            const R* const e = t.data() + (size_t)i * RHEO_STRIDE;
            const R w = e[0] + fr * e[1], wm = e[2] + fr * e[3];
            if (!(w > (R)0 && w < (R)2 && wm > (R)0 && wm < (R)2)) {
                std::printf("FAILED %s n=%d s=%a w=%a wm=%a\n", name, n, (double)s, (double)w, (double)wm);
                ++bad;
            }
            // in range: the index is the floor and the fraction the rest; at and beyond the top: the last interval, fr = 1
            if (s >= (R)0 && s < nm1 && (i != (int)s || fr != s - (R)(int)s)) {
                std::printf("FAILED %s n=%d s=%a not the floor: i=%d fr=%a\n", name, n, (double)s, i, (double)fr);
                ++bad;
            }
            if ((s >= nm1 || s != s) && (i != n - 2 || fr != (R)1)) {
                std::printf("FAILED %s n=%d s=%a not the top: i=%d fr=%a\n", name, n, (double)s, i, (double)fr);
                ++bad;
            }
            if (s <= (R)0 && (i != 0 || fr != (R)0)) {
                std::printf("FAILED %s n=%d s=%a not the bottom: i=%d fr=%a\n", name, n, (double)s, i, (double)fr);
                ++bad;
            }
        }
    }
    if (!bad) std::printf("ok %s %d\n", name, cases);
    return bad;
}

int main() {
    int bad = run<float>("float");
    bad += run<double>("double");
    // the slopes are formed in the lattice type: d = (R)w[i + 1] - (R)w[i], one rounding
    const double w[3] = {0.1 + 1e-9, 0.7 + 3e-9, 1.3};
    const std::vector<float> t = rheology_table<float>(w, nullptr, 3);
    const float d0 = (float)w[1] - (float)w[0];
    if (t[0] != (float)w[0] || t[1] != d0 || t[2] != 0.f || t[3] != 0.f || t[4] != (float)w[1]) {
        std::printf("FAILED slopes\n");
        ++bad;
    } else {
        std::printf("ok slopes 1\n");
    }
    return bad ? 1 : 0;
}
