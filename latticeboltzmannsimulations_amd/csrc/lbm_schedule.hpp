// lbm_schedule.hpp -- the schedule of automatic sampling (lbm_stats_begin / lbm_monitor_begin / lbm_residual_begin / lbm_force_begin
// with every > 0), one Sampler per feature.  The sample of step count n of a field sampler is the macroscopic state of the lattice
// after n - 1 steps, so the step loop (step_many) cuts its units where one would start at n - 1 and takes the sample there: "sample
// whatever is due, then advance by at most steps_to_cut".  The force on the bodies of step count n is defined on the lattice after n
// steps (after = 1): a unit ends at n and the sample follows it, also where that unit is the call's last.  Plain C++, nothing from
// HIP: tests/test_schedule_cpu.py and tests/test_body_force_cpu.py drive it from programs of their own.
#pragma once

namespace lbmhost {

// The samplers, in the order in which those due at the same step count are enqueued.  NSAMPLERS counts the field samplers, which
// sample before a unit; SMP_FORCE samples after one; a context holds NSCHEDULED of them.
enum { SMP_STATS, SMP_MONITOR, SMP_RESIDUAL, NSAMPLERS, SMP_FORCE = NSAMPLERS, NSCHEDULED };
constexpr const char* SAMPLER_CALLS[NSCHEDULED] = {"lbm_stats", "lbm_monitor", "lbm_residual", "lbm_force"};   // the stem of its _begin / _sample calls

struct Sampler {
    int every = 0;        // steps between two automatic samples (0: none)
    long long next = 0;   // the step count of the next one
    int after = 0;        // 0: the sample of n reads the lattice after n - 1 steps; 1: after n steps
    void arm(long long nsteps, int every_, int after_ = 0) { every = every_; next = nsteps + every_; after = after_; }
    void clear() { every = 0; next = 0; after = 0; }
    bool due(long long nsteps) const { return every > 0 && nsteps + 1 - after == next; }
    void advance() { next += every; }
};

// steps a unit may spend from step count nsteps before the next cut: the earliest sampler's next sample (left with all of them off)
template <int N>
inline long long steps_to_cut(const Sampler (&s)[N], long long nsteps, long long left) {
    for (const Sampler& m : s)
        if (m.every > 0 && m.next - 1 + m.after - nsteps < left) left = m.next - 1 + m.after - nsteps;
    return left;
}

// the stem of the calls of a sampler that samples automatically, or null
template <int N>
inline const char* automatic_sampler(const Sampler (&s)[N]) {
    for (int i = 0; i < N; ++i)
        if (s[i].every > 0) return SAMPLER_CALLS[i];
    return nullptr;
}
}  // namespace lbmhost
