// lbm_rheology.hpp -- the rheology table of the obstacle lattices (lbm_set_rheology; contract in include/lbm.h): the index
// into the table, safe for any state of the lattice, and the table as the device holds it.  The rule itself is rheology_rates of
// lbm_device.hpp.  Plain C++ outside a HIP compile: tests/test_rheology_cpu.py drives both functions from a host program of its own.
#pragma once
#include <cmath>
#include <vector>

#ifdef __HIPCC__
#define LBM_RHEO_HD __host__ __device__ __forceinline__
#else
#define LBM_RHEO_HD inline
#endif

constexpr int RHEO_MIN_ENTRIES = 2, RHEO_MAX_ENTRIES = 65536;
constexpr int RHEO_STRIDE = 4;   // reals per entry: t, d, tm, dm

// s = g * inv_dg, the cell's place in the table in units of one interval; nm1 = n - 1 >= 1.  Returns the interval i in [0, n - 2] and
// fr = sc - i in [0, 1], sc = s clamped to [0, n - 1] -- for EVERY s: a lattice that has blown up hands over negative values, infinities
// and NaNs.  C fmin / fmax return the other argument for a NaN, so a NaN s gives sc = n - 1: the last interval, fr = 1.  The integer is
// clamped on both sides once more, so the index does not rest on what the conversion makes of a value the clamp let through.
LBM_RHEO_HD float rheo_min(float a, float b) { return __builtin_fminf(a, b); }
LBM_RHEO_HD float rheo_max(float a, float b) { return __builtin_fmaxf(a, b); }
LBM_RHEO_HD double rheo_min(double a, double b) { return __builtin_fmin(a, b); }
LBM_RHEO_HD double rheo_max(double a, double b) { return __builtin_fmax(a, b); }
template <typename R>
LBM_RHEO_HD int rheology_index(R s, int nm1, R& fr) {
    const R sc = rheo_max(rheo_min(s, (R)nm1), (R)0);
    int i = (int)sc;
    i = i < nm1 - 1 ? i : nm1 - 1;
    i = i > 0 ? i : 0;
    fr = sc - (R)i;
    return i;
}

// The table as the device holds it, n entries of RHEO_STRIDE reals: t[i] = omega[i] rounded once to the lattice type, d[i] = t[i + 1] -
// t[i] formed in the lattice type (d[n - 1] = 0), then the same pair of omegam, zeros without it -- value and slope side by side, so a
// lane fetches a rate's pair with one load.
template <typename R>
std::vector<R> rheology_table(const double* omega, const double* omegam, int n) {
    std::vector<R> t((size_t)n * RHEO_STRIDE, (R)0);
    for (int part = 0; part < 2; ++part) {
        const double* const v = part ? omegam : omega;
        if (!v) continue;
        for (int i = 0; i < n; ++i) {
            const R a = (R)v[i];
            volatile R d = i + 1 < n ? (R)v[i + 1] - a : (R)0;   // (volatile: one rounding in R, whatever the host's excess precision)
            t[(size_t)i * RHEO_STRIDE + 2 * part] = a;
            t[(size_t)i * RHEO_STRIDE + 2 * part + 1] = d;
        }
    }
    return t;
}
// inv_dg = (n - 1) / g_max, formed in double, rounded once
template <typename R>
R rheology_inv_dg(int n, double g_max) { return (R)((double)(n - 1) / g_max); }
