// lbm_schedule.hpp -- the schedule of automatic sampling (lbm_stats_begin / lbm_monitor_begin / lbm_residual_begin with every > 0),
// one Sampler per feature.  The sample of step count n is the macroscopic state of the lattice after n - 1 steps, so the step loop
// (step_many) cuts its units where one would start at n - 1 and takes the sample there: "sample whatever is due, then advance by
// at most steps_to_cut".  Plain C++, nothing from HIP: tests/test_schedule_cpu.py drives it from a program of its own.
#pragma once

namespace lbmhost {

// The samplers, in the order in which those due at the same step count are enqueued.
enum { SMP_STATS, SMP_MONITOR, SMP_RESIDUAL, NSAMPLERS };
constexpr const char* SAMPLER_CALLS[NSAMPLERS] = {"lbm_stats", "lbm_monitor", "lbm_residual"};   // the stem of its _begin / _sample calls

struct Sampler {
    int every = 0;        // steps between two automatic samples (0: none)
    long long next = 0;   // the step count of the next one
    void arm(long long nsteps, int every_) { every = every_; next = nsteps + every_; }
    void clear() { every = 0; next = 0; }
    bool due(long long nsteps) const { return every > 0 && nsteps + 1 == next; }
    void advance() { next += every; }
};

// steps a unit may spend from step count nsteps before the next cut: the earliest sampler's next sample (left with all of them off)
inline long long steps_to_cut(const Sampler (&s)[NSAMPLERS], long long nsteps, long long left) {
    for (const Sampler& m : s)
        if (m.every > 0 && m.next - 1 - nsteps < left) left = m.next - 1 - nsteps;
    return left;
}

// the stem of the calls of a sampler that samples automatically, or null
inline const char* automatic_sampler(const Sampler (&s)[NSAMPLERS]) {
    for (int i = 0; i < NSAMPLERS; ++i)
        if (s[i].every > 0) return SAMPLER_CALLS[i];
    return nullptr;
}
}  // namespace lbmhost
